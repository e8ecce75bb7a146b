"""savgol_streambank_push_block_multi_h16 against its twins, bit for bit.

Every case makes banks A_k for the multi call and twins B_k -- the same configuration and flags -- and gives A_k and B_k the same history through fp32
calls (bank k's own: histories may differ inside one call).  Then the A banks take ONE savgol_streambank_push_block_multi_h16 and every B_k its own
single savgol_streambank_push_block_h16 on the same pointers' alignment.  Signals come from tests.stream_seams.signal, rounded into the input type on
the CPU; samples and outputs sit in stream_seams.Guarded buffers (a row of `streams` 16-bit words is a row of streams / 2 of its 4-byte elements, so an
offset of one element is 4 bytes).  After every call: output k equals twin k's as 16- or 32-bit words (NaN positions coincide, payloads free); rows of
ticks without an output and the guards still hold the guard; d_samples and its guards are unchanged; produced[k], the return value and the counters
are equal.  After the last call both flushes are bit-equal and the savgol_streambank_save blobs byte-equal.  One case per (half window, bank kind) also
holds the outputs to savgol_streambank_push_block_multi on the samples widened in torch (fp32, aligned), rounded once with torch's nearest-even cast.
_route must answer the shipped rule (include/savgol_hip.h), restated here: a build that only ever fell back to single calls does not pass.
No tolerance anywhere: the bar is bit equality."""
import ctypes as C

import numpy as np
import pytest

from tests import stream_seams as seams
from tests._util import bits

pytestmark = pytest.mark.gpu

f32 = np.float32
NAME = "savgol_streambank_push_block_multi_h16"
FUSED_MAX_N = {(0, 2): 8, (0, 3): 8, (1, 2): 8, (1, 3): 8}   # the shipped bounds: (fused bank?, outputs per launch) -> the largest fused half window
FILTERS = [(2, 0, 1.0), (2, 1, 1e-3), (3, 2, 0.5)]           # smoothing (uncentred), first and second derivative (centred on the fused bank): three dt_inv in one launch
TICKS = [64, 65, 95, 96, 97, 128, 161]                       # no body | one partial band ... | two bands | four bands, the last of one row
ALL_PAIRS = [("bf16", "bf16"), ("f16", "f16"), ("f16", "f32"), ("bf16", "f32")]
GUARD_BITS = bits(np.array([seams.GUARD], f32))[0]


@pytest.fixture(scope="module")
def torch_gpu(sg):
    import torch
    assert torch.cuda.is_available() and sg.device_count() > 0, sg.last_error()
    return torch


def tdtype(torch, name):
    return {"f16": torch.float16, "bf16": torch.bfloat16, "f32": torch.float32}[name]


def words_of(torch, t):
    """a CPU tensor of fp16 / bf16 / fp32 elements as its 16- or 32-bit words"""
    if t.dtype == torch.float32:
        return t.contiguous().view(torch.int32).numpy().view(np.uint32)
    return t.contiguous().view(torch.int16).numpy().view(np.uint16)


def nan_words(w, name):
    if name == "f32":
        return np.isnan(w.view(f32))
    return (w & 0x7fff) > (0x7c00 if name == "f16" else 0x7f80)


def same_words(got, want, name, what):
    """bit equality of two arrays of storage words; NaN positions coincide, NaN payloads are free"""
    assert got.shape == want.shape and got.dtype == want.dtype, what
    gn, wn = nan_words(got, name), nan_words(want, name)
    assert np.array_equal(gn, wn), (what, "NaN positions")
    bad = (got != want) & ~gn
    if bad.any():
        at = tuple(int(v) for v in np.argwhere(bad)[0])
        raise AssertionError((what, f"{int(bad.sum())} of {bad.size} words differ, first at {at}: got {got[at]:#x} want {want[at]:#x}"))


def filters_for(n, sgo):
    out = [f if f[0] <= 2 * n and sgo.weights(n, f[0], f[1]) is not None else (2, f[1], f[2]) for f in FILTERS]
    assert all(sgo.weights(n, f[0], f[1]) is not None for f in out)
    return out


def expected_route(specs, streams, ticks, misaligned):
    """the shipped rule: fused launches of a call, 0 = single 16-bit calls"""
    n, fma = specs[0][0], specs[0][4]
    per = 2 if len(specs) == 4 else len(specs)
    fused = (len(specs) >= 2 and all(s[0] == n and s[4] == fma for s in specs) and n <= FUSED_MAX_N.get((fma, per), 0) and streams % 128 == 0 and
             not misaligned and ticks > 64)
    return (2 if len(specs) == 4 else 1) if fused else 0


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


def run_case(sg, sgo, torch, streams, specs, calls, pair, offset=0.0, off_in=0, off_out=(), seed=0, pin=False, follow=False, mutate=None, what=""):
    """specs: (n, m, d, dt, fma, history ticks) per bank; calls: the ticks of each multi call.  Returns (output words compared, calls that were fused)."""
    K = len(specs)
    what = (what, streams, specs, calls, pair, offset, off_in, off_out)
    L_ = sg.lib()
    st = torch.cuda.current_stream().cuda_stream
    IT, OT = sg._STORAGE[pair[0]], sg._STORAGE[pair[1]]
    idt, odt = tdtype(torch, pair[0]), tdtype(torch, pair[1])
    case = seams.Case("multi_h16", streams, 0, 0, specs[0][0], 2, 0, 1.0, 0, offset, ())
    total = sum(calls)
    xq = torch.from_numpy(seams.signal(case, total, seed)).to(idt)           # quantised into the input type on the CPU, nearest even
    if mutate is not None:
        mutate(xq)
    x32 = xq.float()                                                           # widened exactly
    past = seams.signal(case, max(max(s[5] for s in specs), 1), seed + 1)
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
    for L in calls:
        xin = Buf(torch, L, streams, pair[0], off_in, words_of(torch, xq[t:t + L]))
        oa = [Buf(torch, L, streams, pair[1], off_out[k]) for k in range(K)]
        ob = [Buf(torch, L, streams, pair[1], off_out[k]) for k in range(K)]                 # the twin takes the same pointers' alignment
        mis = ((off_in * 4) | max(o * 4 for o in off_out)) & 15
        route = sg.push_block_multi_h16_route(A, xin.ptr(), pair[0], L, [o.ptr() for o in oa], pair[1])
        assert route == expected_route(specs, streams, L, mis), (what, L, route, sg.last_error())
        fused_calls += route > 0
        before = [a.counters for a in A]
        assert sg.push_block_multi_h16_route(A, xin.ptr(), pair[0], L, [o.ptr() for o in oa], pair[1]) == route and [a.counters for a in A] == before
        produced = (C.c_int * K)()
        rc = L_.savgol_streambank_push_block_multi_h16(arr([a.ptr for a in A]), K, xin.ptr(), IT, L, arr([o.ptr() for o in oa]), OT, produced, st)
        pa = list(produced)
        pb = [B[k].push_block_h16(xin.ptr(), pair[0], L, ob[k].ptr(), pair[1]) for k in range(K)]
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
        for k in range(K):
            fa, ra = oa[k].read()
            fb, rb = ob[k].read()
            assert oa[k].g.outside_intact(fa) and ob[k].g.outside_intact(fb), (what, L, k, "guards around d_out")
            silent = L - pb[k]
            assert (bits(oa[k].g.body(fa)[:silent]) == GUARD_BITS).all(), (what, L, k, "a row of a tick without an output was written")
            same_words(ra[silent:], rb[silent:], pair[1], (what, L, k))
            words += ra[silent:].size
            if pin and pb[k]:
                same_words(ra[silent:], words_of(torch, want32[k][silent:].to(odt)), pair[1], (what, L, k, "the fp32 fused call on widened samples, rounded once"))
        t += L
    if follow:
        # the banks the multi call left take a tick push, a fp32 block push, a single 16-bit block push and a fp32 multi push like their twins
        more = seams.signal(case, 1 + 40 + 70 + 97, seed + 2)
        row = torch.from_numpy(more[0]).cuda()
        blk = torch.from_numpy(more[1:41]).cuda()
        x16 = torch.from_numpy(more[41:111]).to(torch.bfloat16).cuda()
        last = torch.from_numpy(more[111:]).cuda()
        got = []
        for bs in (A, B):
            outs = []
            for bank in bs:
                o1 = torch.full((streams,), float(seams.GUARD), device="cuda")
                o2 = torch.full((40, streams), float(seams.GUARD), device="cuda")
                o3 = torch.full((70, streams), float(seams.GUARD), dtype=torch.bfloat16, device="cuda")
                r = (bank.push(row, o1), bank.push_block(blk, 40, o2), bank.push_block_h16(x16, "bf16", 70, o3))
                outs.append((r, o1, o2, o3))
            o4 = [torch.full((97, streams), float(seams.GUARD), device="cuda") for _ in bs]
            got.append((outs, sg.push_block_multi(bs, last, 97, o4), o4))
        torch.cuda.synchronize()
        assert got[0][1] == got[1][1], (what, "fp32 multi push after the 16-bit multi call")
        for k in range(K):
            a, b = got[0][0][k], got[1][0][k]
            assert a[0] == b[0] and min(a[0]) >= 0, (what, "follow-ups", a[0], b[0])
            assert torch.equal(a[1].view(torch.int32), b[1].view(torch.int32)), (what, k, "tick push after the multi call")
            assert torch.equal(a[2].view(torch.int32), b[2].view(torch.int32)), (what, k, "fp32 block push after the multi call")
            assert torch.equal(a[3].view(torch.int16), b[3].view(torch.int16)), (what, k, "16-bit block push after the multi call")
            assert torch.equal(got[0][2][k].view(torch.int32), got[1][2][k].view(torch.int32)), (what, k, "fp32 multi push after the multi call")
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
    return words, fused_calls


def case_list(n, fma, F):
    """(streams, specs, calls, pair, keywords) of one (half window, bank kind): a pure function.  Not a cross product: every value of every axis occurs."""
    out = []
    H = [0, n, 2 * n, 2 * n + 1]

    def spec(fi, h, nn=n, flag=fma):
        f = F[fi % 3]
        return (nn, f[0], f[1], f[2], flag, h)

    def add(streams, specs, calls, **kw):
        out.append((streams, specs, calls, ALL_PAIRS[(len(out) + n) % 4], kw))

    # every length x count 2, 3, 4; histories round robin and different inside one call; 256 streams, 2176 = 17 strips (a narrower last group) and 128
    for i, L in enumerate(TICKS):
        count = 2 + i % 3
        streams = (256, 2176, 128)[i % 3] if L != 161 else 2176
        add(streams, [spec(k, H[(i + k) % 4]) for k in range(count)], [L])
    # fresh banks, three filters in one launch, then a second multi call on the banks the first one left; follow-ups on the same banks; pinned to the
    # fp32 fused call
    add(256, [spec(k, 0) for k in range(3)], [97, 65], follow=True, pin=True)
    add(128, [spec(k + 1, 2 * n + 1) for k in range(4)], [161])
    add(256, [spec(1, n), spec(1, n)], [96])                                     # the same filter twice: two outputs that must be equal
    # one pointer 4 or 8 bytes off the 16-byte grid: single calls, the same bits
    add(256, [spec(0, n), spec(1, 0)], [97], off_in=1)
    add(256, [spec(0, 0), spec(1, n), spec(2, 0)], [97], off_out=(0, 2, 0))
    # a mixed-flag and a mixed-half-window call: single calls
    add(256, [spec(0, 0), spec(1, 0, flag=1 - fma)], [97])
    add(256, [spec(0, 0), spec(1, n, nn=n + 1), spec(2, 0)], [97])
    if fma:
        # what centring exists for: derivative banks on streams riding on an offset of 1000, beside a smoothing bank
        add(256, [spec(k, (0, 2 * n, n)[k]) for k in range(3)], [161], offset=1000.0)
    return out


@pytest.mark.parametrize("n,fma", [(n, fma) for n in (1, 4, 5, 7, 8) for fma in (0, 1)] + [(9, 0), (9, 1), (16, 0), (16, 1)])
def test_multi_h16_block_push_equals_its_twins(sg, sgo, torch_gpu, n, fma):
    F = filters_for(n, sgo)
    todo = case_list(n, fma, F)
    assert {c[3] for c in todo} == set(ALL_PAIRS)
    words = fused = 0
    for i, (streams, specs, calls, pair, kw) in enumerate(todo):
        w, fc = run_case(sg, sgo, torch_gpu, streams, specs, calls, pair, seed=1000 * n + 10 * i + fma, **kw)
        words += w
        fused += fc > 0
        assert (fc > 0) == any(expected_route(specs, streams, L, kw.get("off_in", 0) or any(kw.get("off_out", ()))) for L in calls)
    # n <= 8: every case but the no-body length, the two off-grid pointers, the mixed flag and the mixed half window is fused; n = 9 and 16 (a fused-bank
    # derivative filter among them): every call is single 16-bit calls
    shipped = n <= min(FUSED_MAX_N[(fma, 2)], FUSED_MAX_N[(fma, 3)])
    assert fused == (len(todo) - 5 if shipped else 0), (n, fma, fused, len(todo))
    assert words > 1000 * len(todo)
    print(f"n={n} {'fused' if fma else 'bit-exact'} bank: {len(todo)} cases ({fused} with a fused call), {words} output words compared")


@pytest.mark.parametrize("fma", [0, 1])
def test_multi_h16_same_filter_twice_gives_equal_outputs(sg, sgo, torch_gpu, fma):
    torch = torch_gpu
    S, n, T = 256, 5, 96
    x = torch.from_numpy(seams.signal(seams.Case("twice", S, 0, 0, n, 2, 1, 1e-3, fma, 0.0, ()), T, 3)).to(torch.bfloat16).cuda()
    banks = [sg.StreamBank(S, n, 2, 1, 1e-3, fma=bool(fma)) for _ in range(2)]
    outs = [torch.full((T, S), float(seams.GUARD), dtype=torch.bfloat16, device="cuda") for _ in range(2)]
    assert sg.push_block_multi_h16_route(banks, x, "bf16", T, outs) == 1
    assert sg.push_block_multi_h16(banks, x, "bf16", T, outs) == [T - 2 * n] * 2
    torch.cuda.synchronize()
    assert torch.equal(outs[0].view(torch.int16), outs[1].view(torch.int16))
    assert bool((outs[0][:2 * n] == float(seams.GUARD)).all()) and not bool((outs[0][2 * n:] == float(seams.GUARD)).all())
    for b in banks:
        b.close()


@pytest.mark.parametrize("fma", [0, 1])
def test_multi_h16_special_values(sg, sgo, torch_gpu, fma):
    """fp16 input holding NaN, +-Inf, subnormals and signed zeros on the first and the last row of body tiles (band 2: ticks 64..95, band 3: 96..127), in
    the eight rows a tile's centre sums (n = 4: ticks 56..63 and 88..95) and on both sides of a strip seam (streams 127 | 128); ramps whose derivative
    overflows fp16 on the way out (+-Inf): NaN positions coincide with the twins', every other word is bit-equal"""
    torch = torch_gpu

    def mutate(x):
        w = x.view(torch.int16)
        T = x.shape[0]
        w[:, 3] = torch.arange(T, dtype=torch.int16) % 1024                          # +0 and positive subnormals
        w[:, 4] = (torch.arange(T, dtype=torch.int16) % 1024) | -32768               # -0 and negative subnormals
        w[:, 127] = w[:, 3]
        w[:, 128] = w[:, 4]
        x[64, 5] = float("nan")                                                      # a body tile's first row
        x[95, 6] = float("inf")                                                      # ... and its last
        x[96, 7] = float("-inf")
        x[58, 12] = float("nan")                                                     # inside band 2's centre rows
        x[90, 13] = float("inf")                                                     # inside band 3's
        x[64, 126] = float("inf")
        x[95, 129] = float("nan")
        x[:, 8] = 0.0
        x[:, 9] = -0.0
        x[:, 10] = 80.0 * torch.arange(T, dtype=torch.float32)                       # a ramp whose derivative (x 1000) overflows fp16 on the way out: +Inf
        x[:, 11] = -80.0 * torch.arange(T, dtype=torch.float32)
        x[:, 130] = x[:, 10]

    F = filters_for(4, sgo)
    specs = [(4, f[0], f[1], f[2], fma, h) for f, h in zip(F, (0, 9, 4))]
    for pair in (("f16", "f16"), ("f16", "f32")):
        w, fc = run_case(sg, sgo, torch, 256, specs, [161], pair, seed=5, mutate=mutate, pin=True, what="specials")
        assert w > 0 and fc == 1
    w, fc = run_case(sg, sgo, torch, 256, specs[:2], [97], ("f16", "f16"), seed=6, offset=100.0, mutate=mutate, what="specials, offset")
    assert w > 0 and fc == 1


def test_multi_h16_refusals(sg, torch_gpu):
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
    buf = torch.full((12 * T, S), float(seams.GUARD), dtype=torch.bfloat16, device="cuda")
    row = 2 * S                                                            # bytes of a 16-bit row
    src = buf.data_ptr()
    o = [src + (2 + 3 * k) * T * row for k in range(3)]                    # three rows apart: room for fp32 outputs
    L = sg.lib()
    st = torch.cuda.current_stream().cuda_stream
    F32, F16, BF16 = sg.SAVGOL_HIP_F32, sg.SAVGOL_HIP_F16, sg.SAVGOL_HIP_BF16
    far = [src + (1 << 44), src + (1 << 45), src + (1 << 46)]

    def refused(text, bank_list, count, samples, it, ticks, outs, ot):
        for fn, tail, who in ((L.savgol_streambank_push_block_multi_h16, (None, st), NAME), (L.savgol_streambank_push_block_multi_h16_route, (), NAME + "_route")):
            head = (arr([getattr(b, "ptr", b) for b in bank_list]) if bank_list is not None else None, count, samples, it, ticks,
                    arr(outs) if outs is not None else None, ot)
            assert fn(*head, *tail) == -1, text
            err = sg.last_error()
            assert err.startswith(who + ":") and text in err, (text, err)
            assert [b.counters for b in banks] == counters

    twice = [banks[0], banks[1], banks[0]]
    refused("NULL pointer", banks, 0, None, BF16, T, o, BF16)                                   # 1 (+ 2)
    refused("NULL pointer", None, 3, src, BF16, T, o, BF16)
    refused("NULL pointer", banks, 3, src, BF16, T, None, BF16)
    refused("outside 1..4", [banks[0], None, banks[2]], 0, src, BF16, T, o, BF16)               # 2 (+ 3)
    refused("outside 1..4", banks + [other, other], 5, src, BF16, T, o + o[:2], BF16)
    refused("NULL pointer: banks[1]", [banks[0], None, banks[2]], 3, src, F32, T, o, BF16)      # 3 (+ 4)
    refused("NULL pointer: d_outs[2]", banks, 3, src, F32, T, [o[0], o[1], None], BF16)
    for it, ot, text in ((F32, F32, "f32 -> f32"), (F16, BF16, "f16 -> bf16"), (BF16, F16, "bf16 -> f16"), (F32, BF16, "f32 -> bf16"), (9, F32, "unknown -> f32")):
        refused(text, twice, 3, src, it, T, o, ot)                                              # 4 (+ 5)
    refused("listed twice", [banks[0], other, banks[0]], 3, src, BF16, T, o, BF16)              # 5 (+ 6)
    banks[1].service_start()
    try:
        refused("streams", [banks[0], other, banks[1]], 3, src, BF16, T, o, BF16)               # 6 (+ 7)
        refused("tick service", banks, 3, src, BF16, (1 << 30) + 1, far, BF16)                  # 7 (+ 8)
    finally:
        banks[1].service_stop()
    refused("2^30", banks, 3, src, BF16, (1 << 30) + 1, [src, far[1], far[2]], BF16)            # 8 (+ 9)
    # 9: byte-wise, each buffer with its own element size.  16 -> 16 bit: the same rows ... one shared element at either end
    for shift in (0, row, -row, T * row - 2, -(T * row - 2)):
        refused("d_samples and d_outs[1] overlap", banks, 3, o[1] + shift, BF16, T, o, BF16)
    for shift in (0, T * row - 2, -(T * row - 2)):
        refused("d_outs[0] and d_outs[2] overlap", banks, 3, src, BF16, T, [o[0], o[1], o[0] + shift], BF16)
    # 16 bit -> fp32: an output is twice as long as the samples: its last four bytes on the samples' first, and the samples' last two bytes on its first
    refused("d_samples and d_outs[0] overlap", banks, 3, o[0] + 2 * T * row - 4, BF16, T, o, F32)
    refused("d_samples and d_outs[0] overlap", banks, 3, o[0] - (T * row - 2), BF16, T, o, F32)
    refused("d_outs[0] and d_outs[1] overlap", banks, 3, src, BF16, T, [o[0], o[0] + 2 * T * row - 4, o[2]], F32)
    # both faults of check 9 at once: the samples come first
    refused("d_samples and d_outs[0] overlap", banks, 3, o[0], BF16, T, [o[0], o[0], o[2]], BF16)
    assert sg.push_block_multi_h16(banks, src, "bf16", 0, o) == [0, 0, 0] and [b.counters for b in banks] == counters
    assert L.savgol_streambank_push_block_multi_h16(arr([b.ptr for b in banks]), 3, src, BF16, 0, arr(o), BF16, None, st) == 0
    torch.cuda.synchronize()
    assert bool((buf == float(seams.GUARD)).all())
    for b, blob in zip(banks, blobs):
        assert np.array_equal(b.save(), blob)
    # buffers that touch end to start are served (fp32 outputs right behind the samples); produced may be NULL and the return value is the smallest count
    touching = [src + T * row, src + 3 * T * row, src + 5 * T * row]
    assert L.savgol_streambank_push_block_multi_h16(arr([b.ptr for b in banks]), 3, src, BF16, T, arr(touching), F32, None, st) == T, sg.last_error()
    torch.cuda.synchronize()
    for b in banks + [other]:
        b.close()


def test_multi_h16_refuses_a_bank_on_another_device(sg, torch_gpu):
    torch = torch_gpu
    if torch.cuda.device_count() < 2:
        pytest.skip("one GPU")
    banks = [sg.StreamBank(256, 4, 2, d, 1.0) for d in (0, 1)]
    buf = torch.full((3 * 97, 256), float(seams.GUARD), dtype=torch.bfloat16, device="cuda:0")
    try:
        assert sg.lib().savgol_hip_set_device(1) == 0
        with pytest.raises(RuntimeError, match="lives on device 0"):
            sg.push_block_multi_h16(banks, buf[:97], "bf16", 97, [buf[97:194], buf[194:]])
        assert NAME in sg.last_error()
    finally:
        sg.lib().savgol_hip_set_device(0)
    assert [b.counters for b in banks] == [(0, 0), (0, 0)]
    for b in banks:
        b.close()


@pytest.mark.parametrize("pair", [("bf16", "bf16"), ("f16", "f32")])
def test_multi_h16_fused_call_in_a_graph(sg, sgo, torch_gpu, pair):
    """after one warm-up call a fused call (one widen, three heads and rounds, one body launch, three tail stores; one stream-ordered allocation / free
    pair from the library's pool) is captured and replays to the same bits on reset banks"""
    torch = torch_gpu
    S, n, T = 256, 5, 161
    F = filters_for(n, sgo)
    case = seams.Case("graph", S, 0, 0, n, 2, 0, 1.0, 1, 0.0, ())
    x = torch.from_numpy(seams.signal(case, T, 9)).to(tdtype(torch, pair[0])).cuda()
    banks = [sg.StreamBank(S, n, f[0], f[1], f[2], fma=True) for f in F]
    want = [torch.full((T, S), float(seams.GUARD), dtype=tdtype(torch, pair[1]), device="cuda") for _ in F]
    assert sg.push_block_multi_h16_route(banks, x, pair[0], T, want, pair[1]) == 1
    assert sg.push_block_multi_h16(banks, x, pair[0], T, want, pair[1]) == [T - 2 * n] * 3
    torch.cuda.synchronize()
    blobs = [b.save() for b in banks]
    out = [torch.full_like(w, float(seams.GUARD)) for w in want]
    for b in banks:
        b.reset()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(s):
        with torch.cuda.graph(g, stream=s):
            assert sg.push_block_multi_h16(banks, x, pair[0], T, out, pair[1], stream=s) == [T - 2 * n] * 3, sg.last_error()
    for o in out:
        o.fill_(float(seams.GUARD))
    torch.cuda.synchronize()
    g.replay()
    torch.cuda.synchronize()
    view = torch.int32 if pair[1] == "f32" else torch.int16
    for o, w in zip(out, want):
        assert torch.equal(o.view(view), w.view(view))
    for b, blob in zip(banks, blobs):
        assert np.array_equal(b.save(), blob)
        b.close()
