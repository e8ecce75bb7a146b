"""savgol_streambank_push_block_multi_i16 against its twins, word for word.

Every case makes banks A_k for the multi call and twins B_k -- the same configuration and flags -- and gives A_k and B_k the same history through fp32
calls (bank k's own: histories may differ inside one call).  Then the A banks take ONE savgol_streambank_push_block_multi_i16 and every B_k its own
single savgol_streambank_push_block_i16 on the same pointers' alignment.  Signals come from tests.stream_seams.signal, scaled to the call's amplitude
and quantised to int16 on the CPU (tests/stream_multi_i16.py; the amplitudes are held to their purpose on the CPU in
tests/test_stream_multi_i16_host.py); samples and outputs sit in stream_seams.Guarded buffers (a row of `streams` int16 words is a row of streams / 2 of
its 4-byte elements, so an offset of one element is 4 bytes).  After every call: output k equals twin k's as 16- or 32-bit words (fp32: NaN positions
coincide, payloads free); rows of ticks without an output and the guards still hold the guard; d_samples and its guards are unchanged; produced[k], the
return value and the counters are equal; at least half of the expected int16 words lie strictly inside the range (saturation is tested on purpose, in a
case of its own).  After the last call both flushes are bit-equal and the savgol_streambank_save blobs byte-equal.  One case per (half window, bank kind)
also holds the outputs to savgol_streambank_push_block_multi on x.float() (fp32, aligned), converted with to_i16 on the CPU.
_route must answer the shipped rule (include/savgol_hip.h), restated in tests/stream_multi_i16.py: a build that only ever fell back to single calls does
not pass.  No tolerance anywhere: the bar is bit equality."""
import ctypes as C

import numpy as np
import pytest

from tests import stream_multi_i16 as mi
from tests import stream_seams as seams
from tests._util import bits

pytestmark = pytest.mark.gpu

f32 = np.float32
NAME = "savgol_streambank_push_block_multi_i16"
GUARD_BITS = bits(np.array([seams.GUARD], f32))[0]


@pytest.fixture(scope="module")
def torch_gpu(sg):
    import torch
    assert torch.cuda.is_available() and sg.device_count() > 0, sg.last_error()
    return torch


def tdtype(torch, name):
    return {"i16": torch.int16, "f32": torch.float32}[name]


def words_of(torch, t):
    """a CPU tensor of int16 / fp32 elements as its 16- or 32-bit words"""
    if t.dtype == torch.float32:
        return t.contiguous().view(torch.int32).numpy().view(np.uint32)
    return t.contiguous().numpy().view(np.uint16)


def same_words(got, want, name, what):
    """bit equality of two arrays of storage words; fp32: NaN positions coincide, NaN payloads are free"""
    assert got.shape == want.shape and got.dtype == want.dtype, what
    gn = np.isnan(got.view(f32)) if name == "f32" else np.zeros(got.shape, bool)
    wn = np.isnan(want.view(f32)) if name == "f32" else np.zeros(want.shape, bool)
    assert np.array_equal(gn, wn), (what, "NaN positions")
    bad = (got != want) & ~gn
    if bad.any():
        at = tuple(int(v) for v in np.argwhere(bad)[0])
        raise AssertionError((what, f"{int(bad.sum())} of {bad.size} words differ, first at {at}: got {got[at]:#x} want {want[at]:#x}"))


class Buf:
    """rows x streams elements of a storage type inside a stream_seams.Guarded buffer, `off` 4-byte elements off the 16-byte grid"""

    def __init__(self, torch, rows, streams, name, off=0, host_words=None):
        self.name, self.rows, self.streams = name, rows, streams
        cols = streams if name == "f32" else streams // 2
        host = None if host_words is None else np.ascontiguousarray(host_words).view(f32).reshape(rows, cols)
        self.g = seams.Guarded(torch, rows, cols, off, host)

    def ptr(self):
        return self.g.ptr(0)

    def read(self):
        """(the whole buffer as fp32 words, the rows as storage words)"""
        flat = self.g.host()
        body = self.g.body(flat)
        return flat, (bits(body) if self.name == "f32" else np.ascontiguousarray(body).view(np.uint16).reshape(self.rows, self.streams))


def arr(vals):
    return (C.c_void_p * len(vals))(*vals)


def run_case(sg, sgo, torch, streams, specs, calls, out, offset=0.0, off_in=0, off_out=(), seed=0, pin=False, follow=False, mutate=None, history=None,
             saturating=False, what=""):
    """specs: (n, m, d, dt, fma, history ticks) per bank; calls: the ticks of each multi call.  mutate(xq): edits the int16 samples; history(past): edits
    the fp32 rows the banks take before the first call (NaN and +-Inf can only reach a ring that way).
    Returns (output words compared, calls that were fused, the A banks' output words of the last call per bank)."""
    K = len(specs)
    what = (what, streams, specs, calls, out, offset, off_in, off_out)
    L_ = sg.lib()
    st = torch.cuda.current_stream().cuda_stream
    OT = {"i16": sg.SAVGOL_HIP_I16, "f32": sg.SAVGOL_HIP_F32}[out]
    n0 = specs[0][0]
    total = sum(calls)
    xq = torch.from_numpy(mi.quantise(streams, n0, total, seed, offset))     # int16, quantised on the CPU
    if mutate is not None:
        mutate(xq)
    x32 = xq.float()                                                           # widened exactly
    past = mi.quantise(streams, n0, max(max(s[5] for s in specs), 1), seed + 1, offset).astype(f32)
    if history is not None:
        history(past)
    sets = 3 if pin else 2                                                     # A: the multi call, B: the twins, C: the fp32 fused call on widened samples
    banks = [[sg.StreamBank(streams, s[0], s[1], s[2], s[3], fma=bool(s[4])) for s in specs] for _ in range(sets)]
    A, B = banks[0], banks[1]
    for k, s in enumerate(specs):
        if s[5]:
            h = torch.from_numpy(past[:s[5]]).cuda()
            rs = [bs[k].push_block(h, s[5], torch.empty_like(h)) for bs in banks]
            assert len(set(rs)) == 1 and rs[0] >= 0, (what, sg.last_error())
    off_out = tuple(off_out) + (0,) * (K - len(off_out))
    t = words = fused_calls = 0
    last = None
    for L in calls:
        xin = Buf(torch, L, streams, "i16", off_in, words_of(torch, xq[t:t + L]))
        oa = [Buf(torch, L, streams, out, off_out[k]) for k in range(K)]
        ob = [Buf(torch, L, streams, out, off_out[k]) for k in range(K)]                     # the twin takes the same pointers' alignment
        mis = ((off_in * 4) | max(o * 4 for o in off_out)) & 15
        route = sg.push_block_multi_i16_route(A, xin.ptr(), L, [o.ptr() for o in oa], out)
        assert route == mi.expected_route(specs, streams, L, mis), (what, L, route, sg.last_error())
        fused_calls += route > 0
        before = [a.counters for a in A]
        assert sg.push_block_multi_i16_route(A, xin.ptr(), L, [o.ptr() for o in oa], out) == route and [a.counters for a in A] == before
        produced = (C.c_int * K)()
        rc = L_.savgol_streambank_push_block_multi_i16(arr([a.ptr for a in A]), K, xin.ptr(), L, arr([o.ptr() for o in oa]), OT, produced, st)
        pa = list(produced)
        pb = [B[k].push_block_i16(xin.ptr(), L, ob[k].ptr(), out) for k in range(K)]
        torch.cuda.synchronize()
        assert rc == min(pb) and pa == pb and min(pb) >= 0, (what, L, rc, pa, pb, sg.last_error())
        assert [a.counters for a in A] == [b.counters for b in B], (what, L)
        assert np.array_equal(bits(xin.g.host()), bits(xin.g.want)), (what, L, "d_samples or its guards were written")
        want32 = None
        if pin:
            blk = x32[t:t + L].cuda()
            oc = [torch.full((L, streams), float(seams.GUARD), device="cuda") for _ in range(K)]
            assert sg.push_block_multi_route(banks[2], blk, L, oc) == route, (what, "the fp32 fused call takes another route")
            assert sg.push_block_multi(banks[2], blk, L, oc) == pb, (what, sg.last_error())
            torch.cuda.synchronize()
            want32 = [o.cpu() for o in oc]
        last = []
        for k in range(K):
            fa, ra = oa[k].read()
            fb, rb = ob[k].read()
            assert oa[k].g.outside_intact(fa) and ob[k].g.outside_intact(fb), (what, L, k, "guards around d_out")
            silent = L - pb[k]
            assert (bits(oa[k].g.body(fa)[:silent]) == GUARD_BITS).all(), (what, L, k, "a row of a tick without an output was written")
            if out == "i16" and not saturating and pb[k]:
                assert mi.inside_enough(rb[silent:].view(np.int16)), (what, L, k, "fewer than half of the expected words are inside the int16 range")
            same_words(ra[silent:], rb[silent:], out, (what, L, k))
            words += ra[silent:].size
            if pin and pb[k]:
                exp = want32[k][silent:] if out == "f32" else mi.to_i16(torch, want32[k][silent:])
                same_words(ra[silent:], words_of(torch, exp), out, (what, L, k, "the fp32 fused call on widened samples, converted once on the CPU"))
            last.append(ra[silent:])
        t += L
    if follow:
        # the banks the multi call left take a tick push, a fp32 block push, a single int16 block push and a 16-bit float multi push like their twins
        more = mi.quantise(streams, n0, 1 + 40 + 70 + 97, seed + 2, offset)
        row = torch.from_numpy(more[0].astype(f32)).cuda()
        blk = torch.from_numpy(more[1:41].astype(f32)).cuda()
        x16 = torch.from_numpy(more[41:111]).cuda()
        lastx = torch.from_numpy(more[111:].astype(f32)).to(torch.bfloat16).cuda()
        got = []
        for bs in (A, B):
            outs = []
            for bank in bs:
                o1 = torch.full((streams,), float(seams.GUARD), device="cuda")
                o2 = torch.full((40, streams), float(seams.GUARD), device="cuda")
                o3 = torch.full((70, streams), -7, dtype=torch.int16, device="cuda")
                r = (bank.push(row, o1), bank.push_block(blk, 40, o2), bank.push_block_i16(x16, 70, o3))
                outs.append((r, o1, o2, o3))
            o4 = [torch.full((97, streams), float(seams.GUARD), dtype=torch.bfloat16, device="cuda") for _ in bs]
            got.append((outs, sg.push_block_multi_h16(bs, lastx, "bf16", 97, o4), o4))
        torch.cuda.synchronize()
        assert got[0][1] == got[1][1], (what, "16-bit float multi push after the int16 multi call")
        for k in range(K):
            a, b = got[0][0][k], got[1][0][k]
            assert a[0] == b[0] and min(a[0]) >= 0, (what, "follow-ups", a[0], b[0])
            assert torch.equal(a[1].view(torch.int32), b[1].view(torch.int32)), (what, k, "tick push after the multi call")
            assert torch.equal(a[2].view(torch.int32), b[2].view(torch.int32)), (what, k, "fp32 block push after the multi call")
            assert torch.equal(a[3], b[3]), (what, k, "single int16 block push after the multi call")
            assert torch.equal(got[0][2][k].view(torch.int16), got[1][2][k].view(torch.int16)), (what, k, "16-bit float multi push after the multi call")
    for k in range(K):
        rows = specs[k][0]
        fa = torch.full((2, rows, streams), float(seams.GUARD), device="cuda")
        fb = torch.full((2, rows, streams), float(seams.GUARD), device="cuda")
        assert A[k].flush_leading(fa[0], rows) == B[k].flush_leading(fb[0], rows), what
        assert A[k].flush(fa[1], rows) == B[k].flush(fb[1], rows), what
        torch.cuda.synchronize()
        assert torch.equal(fa.view(torch.int32), fb.view(torch.int32)), (what, k, "flush rows")
        assert np.array_equal(A[k].save(), B[k].save()), (what, k, "save blobs")
    for bs in banks:
        for bank in bs:
            bank.close()
    return words, fused_calls, last


def histories(n):
    return [0, n, 2 * n + 1, 2 * n]                                             # empty, shorter than a window, full, one short of full


@pytest.mark.parametrize("n,fma", [(n, fma) for n in mi.HALF_WINDOWS for fma in (0, 1)])
def test_multi_i16_block_push_equals_its_twins(sg, sgo, torch_gpu, n, fma):
    """2, 3 and 4 banks x both output types; every sequence runs all seven lengths on the same banks, rotated so that each sequence meets its banks'
    first histories (empty, shorter than a window, full) with another length; 256 streams, 128 for one sequence; one sequence pinned to the fp32 call"""
    F = mi.filters_for(n, sgo)
    H = histories(n)
    words = fused = calls_made = 0
    i = 0
    for K in (2, 3, 4):
        for out in mi.OUTS:
            specs = [(n, *F[k % 3], fma, H[(i + k) % 4]) for k in range(K)]
            calls = mi.TICKS[i + 1:] + mi.TICKS[:i + 1]                          # starts at 65, 95, 96, 97, 128, 161 ticks
            streams = 128 if (K, out) == (2, "f32") else 256
            w, fc, _ = run_case(sg, sgo, torch_gpu, streams, specs, calls, out, seed=1000 * n + 10 * i + fma, pin=(K, out) == (3, "i16"))
            shipped = n <= mi.FUSED_MAX_N[(fma, 2 if K == 4 else K)]
            assert fc == (len(calls) - 1 if shipped else 0), (n, fma, K, out, fc)   # every length but 64 ticks is fused up to the bound, none above it
            words += w
            fused += fc
            calls_made += len(calls)
            i += 1
    assert words > 1000 * calls_made
    print(f"n={n} {'fused' if fma else 'bit-exact'} bank: {calls_made} calls ({fused} fused), {words} output words compared")


@pytest.mark.parametrize("n,fma", [(n, fma) for n in mi.HALF_WINDOWS for fma in (0, 1)])
def test_multi_i16_pinned_to_the_fp32_fused_call(sg, sgo, torch_gpu, n, fma):
    """fresh banks, three filters in one launch, then a second call on the banks the first one left, both output types: the outputs are
    savgol_streambank_push_block_multi's on x.float(), converted with to_i16 on the CPU; on the fused bank also with the streams riding at RIDE counts
    (what the centring exists for)"""
    F = mi.filters_for(n, sgo)
    for j, out in enumerate(mi.OUTS):
        specs = [(n, *F[k], fma, (0, n, 2 * n + 1)[(k + j) % 3]) for k in range(3)]
        w, fc, _ = run_case(sg, sgo, torch_gpu, 256, specs, [97, 65], out, seed=77 * n + j, pin=True)
        assert w > 0 and fc == (2 if n <= mi.FUSED_MAX_N[(fma, 3)] else 0)
    if fma:
        specs = [(n, *F[k], fma, (0, 2 * n, n)[k]) for k in range(3)]
        w, fc, _ = run_case(sg, sgo, torch_gpu, 256, specs, [161], "i16", offset=mi.RIDE, seed=78 * n, pin=True)
        assert w > 0 and fc == (1 if n <= mi.FUSED_MAX_N[(fma, 3)] else 0)


@pytest.mark.parametrize("fma", [0, 1])
def test_multi_i16_unfused_routes_equal_their_twins(sg, sgo, torch_gpu, fma):
    """calls the rule sends to single int16 calls: the samples or one output 4 bytes off the 16-byte grid, 130 streams, mixed half windows, mixed bank
    kinds, n = 9 -- every one answers 0 from _route (asserted in run_case against the restated rule) and equals its twins word for word"""
    n = 5
    F = mi.filters_for(n, sgo)

    def spec(fi, h, nn=n, flag=fma):
        f = F[fi % 3] if nn == n else mi.filters_for(nn, sgo)[fi % 3]
        return (nn, f[0], f[1], f[2], flag, h)

    todo = [(256, [spec(0, n), spec(1, 0)], dict(off_in=1)),
            (256, [spec(0, 0), spec(1, n), spec(2, 0)], dict(off_out=(0, 1, 0))),
            (130, [spec(0, 0), spec(1, n), spec(2, 2 * n + 1)], {}),
            (256, [spec(0, 0), spec(1, n, nn=n + 1), spec(2, 0)], {}),
            (256, [spec(0, 0), spec(1, 0, flag=1 - fma)], {}),
            (256, [spec(0, 0, nn=9), spec(1, 9, nn=9), spec(2, 19, nn=9), spec(0, 4, nn=9)], {})]
    for i, (streams, specs, kw) in enumerate(todo):
        for out in mi.OUTS:
            w, fc, _ = run_case(sg, sgo, torch_gpu, streams, specs, [97, 161], out, seed=300 + 10 * i + fma, what="unfused", **kw)
            assert w > 0 and fc == 0, (i, out, fc)


@pytest.mark.parametrize("fma", [0, 1])
def test_multi_i16_same_filter_twice_gives_equal_outputs(sg, sgo, torch_gpu, fma):
    torch = torch_gpu
    S, n, T = 256, 5, 96
    x = torch.from_numpy(mi.quantise(S, n, T, 3)).cuda()
    banks = [sg.StreamBank(S, n, 2, 1, 1e-3, fma=bool(fma)) for _ in range(2)]
    outs = [torch.full((T, S), -7, dtype=torch.int16, device="cuda") for _ in range(2)]
    assert sg.push_block_multi_i16_route(banks, x, T, outs) == 1
    assert sg.push_block_multi_i16(banks, x, T, outs) == [T - 2 * n] * 2
    torch.cuda.synchronize()
    assert torch.equal(outs[0], outs[1])
    assert bool((outs[0][:2 * n] == -7).all()) and not bool((outs[0][2 * n:] == -7).all())
    for b in banks:
        b.close()


@pytest.mark.parametrize("fma", [0, 1])
def test_multi_i16_extreme_samples_and_saturation(sg, sgo, torch_gpu, fma):
    """int16 samples at 32767 and -32768 -- whole streams, single ticks on the first and the last row of body tiles (band 2: ticks 64..95, band 3:
    96..127), in the eight rows a tile's centre sums (n = 4: ticks 56..63, 88..95) and on both sides of a strip seam (streams 127 | 128).  Then the
    saturating case, exempt from the half-inside condition: ramps of 80 counts per tick through the d = 1, dt = 1e-3 bank give 80 000 per time unit and
    pin 32767, the falling ramp -32768, while the other streams stay ordinary"""
    torch = torch_gpu
    n = 4
    F = mi.filters_for(n, sgo)
    specs = [(n, f[0], f[1], f[2], fma, h) for f, h in zip(F, (0, 9, 4))]

    def extremes(x):
        x[:, 3] = 32767
        x[:, 4] = -32768
        x[:, 127] = -32768
        x[:, 128] = 32767
        x[64, 5] = 32767
        x[95, 6] = -32768
        x[96, 7] = 32767
        x[58, 12] = -32768
        x[90, 13] = 32767
        x[64, 126] = -32768
        x[95, 129] = 32767
        x[:, 8] = 0

    for out in mi.OUTS:
        w, fc, last = run_case(sg, sgo, torch, 256, specs, [161], out, seed=5, mutate=extremes, pin=True, what="extremes")
        assert w > 0 and fc == 1
        if out == "i16":
            smooth = last[0].view(np.int16)
            assert (smooth[:, 3] == 32767).all() and (smooth[:, 4] == -32768).all() and (smooth[:, 8] == 0).all()

    def ramps(x):
        T = x.shape[0]
        ramp = (80 * torch.arange(T, dtype=torch.int32)).to(torch.int16)
        assert 80 * (T - 1) <= 32767
        x[:, 10] = ramp
        x[:, 11] = -ramp
        x[:, 129] = ramp

    w, fc, last = run_case(sg, sgo, torch, 256, specs, [161], "i16", seed=6, mutate=ramps, pin=True, saturating=True, what="saturation")
    assert w > 0 and fc == 1
    slope = last[1].view(np.int16)[2 * n:]                                     # bank 1: d = 1, dt = 1e-3, its ring was full: windows of the call's own rows
    assert (slope[:, 10] == 32767).all() and (slope[:, 11] == -32768).all() and (slope[:, 129] == 32767).all()
    assert mi.inside_enough(slope)                                             # the other streams are ordinary ones
    w, fc, last = run_case(sg, sgo, torch, 256, specs, [161], "f32", seed=6, mutate=ramps, pin=True, what="saturation, fp32 out")
    assert fc == 1 and (last[1].view(f32)[2 * n:, 10] > 70000).all() and (last[1].view(f32)[2 * n:, 11] < -70000).all()


@pytest.mark.parametrize("fma", [0, 1])
def test_multi_i16_special_values_from_history(sg, sgo, torch_gpu, fma):
    """NaN and +-Inf in a few streams of the rings, put there by fp32 pushes before the fused call: the first 2n rows of the call (its head) see them.  An
    int16 output holds 0 where the twin's fp32 value is NaN and the saturated values where it is +-Inf; an fp32 output holds NaN at the twin's positions"""
    torch = torch_gpu
    n = 5
    H = 2 * n + 1
    F = mi.filters_for(n, sgo)
    specs = [(n, f[0], f[1], f[2], fma, H) for f in F]

    def history(past):
        past[3, 5] = np.inf
        past[5, 6] = -np.inf
        past[H - 1, 7] = np.nan                                                # the newest sample of the ring: in every window of the first 2n rows
        past[H - 1, 8] = np.inf
        past[2, 129] = -np.inf

    res = {}
    for out in mi.OUTS:
        w, fc, last = run_case(sg, sgo, torch, 256, specs, [97], out, seed=8, history=history, pin=True, what="history")
        assert w > 0 and fc == 1
        res[out] = last
    smooth32, smooth16 = res["f32"][0].view(f32)[:2 * n], res["i16"][0].view(np.int16)[:2 * n]
    assert np.isnan(smooth32[:, 7]).all() and (smooth16[:, 7] == 0).all()
    assert (smooth32[:, 8] == np.inf).any() and (smooth32[:, 6] == -np.inf).any()
    assert (smooth16[smooth32 == np.inf] == 32767).all() and (smooth16[smooth32 == -np.inf] == -32768).all()
    for k in range(3):
        a32, a16 = res["f32"][k].view(f32), res["i16"][k].view(np.int16)
        assert np.isnan(a32[:2 * n, 7]).all() and (a16[np.isnan(a32)] == 0).all()


@pytest.mark.parametrize("fma", [0, 1])
def test_multi_i16_follow_on_calls(sg, sgo, torch_gpu, fma):
    """the banks a fused call left take a tick push, an fp32 block push, a single int16 push and a 16-bit float multi push like their twins"""
    n = 6
    F = mi.filters_for(n, sgo)
    specs = [(n, *F[k], fma, (0, n, 2 * n + 1)[k]) for k in range(3)]
    w, fc, _ = run_case(sg, sgo, torch_gpu, 256, specs, [97, 65], "i16", seed=91 + fma, follow=True, what="follow-on")
    assert w > 0 and fc == 2


def test_multi_i16_refusals(sg, torch_gpu):
    """every refusal returns -1 with a text naming the call before anything is enqueued, in the header's order: each case below also carries the fault
    of the NEXT check, and the earlier one is named; counters and save blobs unchanged, every buffer still all guard"""
    torch = torch_gpu
    S, n, T = 256, 4, 97
    banks = [sg.StreamBank(S, n, 2, d, 1.0, fma=True) for d in (0, 1, 2)]
    other = sg.StreamBank(128, n, 2, 0, 1.0, fma=True)
    warm = torch.zeros((20, S), device="cuda")
    for b in banks:
        assert b.push_block(warm, 20, torch.empty_like(warm)) == 12
    torch.cuda.synchronize()
    blobs, counters = [b.save() for b in banks], [b.counters for b in banks]
    buf = torch.full((12 * T, S), -7, dtype=torch.int16, device="cuda")
    row = 2 * S                                                            # bytes of an int16 row
    src = buf.data_ptr()
    o = [src + (2 + 3 * k) * T * row for k in range(3)]                    # three rows apart: room for fp32 outputs
    L = sg.lib()
    st = torch.cuda.current_stream().cuda_stream
    F32, F16, BF16, I16 = sg.SAVGOL_HIP_F32, sg.SAVGOL_HIP_F16, sg.SAVGOL_HIP_BF16, sg.SAVGOL_HIP_I16
    far = [src + (1 << 44), src + (1 << 45), src + (1 << 46)]

    def refused(text, bank_list, count, samples, ticks, outs, ot):
        for fn, tail, who in ((L.savgol_streambank_push_block_multi_i16, (None, st), NAME), (L.savgol_streambank_push_block_multi_i16_route, (), NAME + "_route")):
            head = (arr([getattr(b, "ptr", b) for b in bank_list]) if bank_list is not None else None, count, samples, ticks,
                    arr(outs) if outs is not None else None, ot)
            assert fn(*head, *tail) == -1, text
            err = sg.last_error()
            assert err.startswith(who + ":") and text in err, (text, err)
            assert [b.counters for b in banks] == counters

    twice = [banks[0], banks[1], banks[0]]
    refused("NULL pointer", banks, 0, None, T, o, I16)                                          # 1 (+ 2)
    refused("NULL pointer", None, 3, src, T, o, I16)
    refused("NULL pointer", banks, 3, src, T, None, I16)
    refused("outside 1..4", [banks[0], None, banks[2]], 0, src, T, o, I16)                      # 2 (+ 3)
    refused("outside 1..4", banks + [other, other], 5, src, T, o + o[:2], I16)
    refused("NULL pointer: banks[1]", [banks[0], None, banks[2]], 3, src, T, o, BF16)           # 3 (+ 4)
    refused("NULL pointer: d_outs[2]", banks, 3, src, T, [o[0], o[1], None], BF16)
    for ot, text in ((F16, "output type f16 (1)"), (BF16, "output type bf16 (2)"), (9, "output type unknown (9)"), (-1, "output type unknown (-1)")):
        refused(text, twice, 3, src, T, o, ot)                                                  # 4 (+ 5)
    refused("listed twice", [banks[0], other, banks[0]], 3, src, T, o, I16)                     # 5 (+ 6)
    banks[1].service_start()
    try:
        refused("streams", [banks[0], other, banks[1]], 3, src, T, o, I16)                      # 6 (+ 7)
        refused("tick service", banks, 3, src, (1 << 30) + 1, far, I16)                         # 7 (+ 8)
    finally:
        banks[1].service_stop()
    refused("2^30", banks, 3, src, (1 << 30) + 1, [src, far[1], far[2]], I16)                   # 8 (+ 9)
    # 9: byte-wise, each buffer with its own element size.  int16 -> int16: the same rows ... one shared element at either end
    for shift in (0, row, -row, T * row - 2, -(T * row - 2)):
        refused("d_samples and d_outs[1] overlap", banks, 3, o[1] + shift, T, o, I16)
    for shift in (0, T * row - 2, -(T * row - 2)):
        refused("d_outs[0] and d_outs[2] overlap", banks, 3, src, T, [o[0], o[1], o[0] + shift], I16)
    # int16 -> fp32: an output is twice as long as the samples: its last four bytes on the samples' first, and the samples' last two bytes on its first
    refused("d_samples and d_outs[0] overlap", banks, 3, o[0] + 2 * T * row - 4, T, o, F32)
    refused("d_samples and d_outs[0] overlap", banks, 3, o[0] - (T * row - 2), T, o, F32)
    refused("d_outs[0] and d_outs[1] overlap", banks, 3, src, T, [o[0], o[0] + 2 * T * row - 4, o[2]], F32)
    # both faults of check 9 at once: the samples come first
    refused("d_samples and d_outs[0] overlap", banks, 3, o[0], T, [o[0], o[0], o[2]], I16)
    assert sg.push_block_multi_i16(banks, src, 0, o) == [0, 0, 0] and [b.counters for b in banks] == counters
    assert L.savgol_streambank_push_block_multi_i16(arr([b.ptr for b in banks]), 3, src, 0, arr(o), I16, None, st) == 0
    torch.cuda.synchronize()
    assert bool((buf == -7).all())
    for b, blob in zip(banks, blobs):
        assert np.array_equal(b.save(), blob)
    # the 16-bit float fused call keeps refusing int16
    assert L.savgol_streambank_push_block_multi_h16(arr([b.ptr for b in banks]), 3, src, I16, T, arr(o), I16, None, st) == -1
    assert "savgol_streambank_push_block_multi_h16" in sg.last_error()
    # buffers that touch end to start are served (fp32 outputs right behind the samples); produced may be NULL and the return value is the smallest count
    touching = [src + T * row, src + 3 * T * row, src + 5 * T * row]
    assert L.savgol_streambank_push_block_multi_i16(arr([b.ptr for b in banks]), 3, src, T, arr(touching), F32, None, st) == T, sg.last_error()
    torch.cuda.synchronize()
    for b in banks + [other]:
        b.close()


def test_multi_i16_refuses_a_bank_on_another_device(sg, torch_gpu):
    torch = torch_gpu
    if torch.cuda.device_count() < 2:
        pytest.skip("one GPU")
    banks = [sg.StreamBank(256, 4, 2, d, 1.0) for d in (0, 1)]
    buf = torch.full((3 * 97, 256), -7, dtype=torch.int16, device="cuda:0")
    try:
        assert sg.lib().savgol_hip_set_device(1) == 0
        with pytest.raises(RuntimeError, match="lives on device 0"):
            sg.push_block_multi_i16(banks, buf[:97], 97, [buf[97:194], buf[194:]])
        assert NAME in sg.last_error()
    finally:
        sg.lib().savgol_hip_set_device(0)
    assert [b.counters for b in banks] == [(0, 0), (0, 0)]
    for b in banks:
        b.close()


@pytest.mark.parametrize("out", ["i16", "f32"])
def test_multi_i16_fused_call_in_a_graph(sg, sgo, torch_gpu, out):
    """after one warm-up call a fused call (one widen, three heads and conversions, one body launch, three tail stores; one stream-ordered allocation /
    free pair from the library's pool) is captured and replays to the twins' bits on reset banks"""
    torch = torch_gpu
    S, n, T = 256, 5, 161
    F = mi.filters_for(n, sgo)
    x = torch.from_numpy(mi.quantise(S, n, T, 9)).cuda()
    twins = [sg.StreamBank(S, n, f[0], f[1], f[2], fma=True) for f in F]
    want = [torch.full((T, S), -7, dtype=tdtype(torch, out), device="cuda") for _ in F]
    for tw, w in zip(twins, want):
        assert tw.push_block_i16(x, T, w, out) == T - 2 * n, sg.last_error()
    torch.cuda.synchronize()
    blobs = [tw.save() for tw in twins]
    banks = [sg.StreamBank(S, n, f[0], f[1], f[2], fma=True) for f in F]
    warm = [torch.full_like(w, -7) for w in want]
    assert sg.push_block_multi_i16_route(banks, x, T, warm, out) == 1
    assert sg.push_block_multi_i16(banks, x, T, warm, out) == [T - 2 * n] * 3
    torch.cuda.synchronize()
    view = torch.int32 if out == "f32" else torch.int16
    for o, w in zip(warm, want):
        assert torch.equal(o.view(view), w.view(view))
    res = [torch.full_like(w, -7) for w in want]
    for b in banks:
        b.reset()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(s):
        with torch.cuda.graph(g, stream=s):
            assert sg.push_block_multi_i16(banks, x, T, res, out, stream=s) == [T - 2 * n] * 3, sg.last_error()
    for o in res:
        o.fill_(-7)
    torch.cuda.synchronize()
    g.replay()
    torch.cuda.synchronize()
    for o, w in zip(res, want):
        assert torch.equal(o.view(view), w.view(view))
    for b, blob in zip(banks, blobs):
        assert np.array_equal(b.save(), blob)
        b.close()
    for tw in twins:
        tw.close()
