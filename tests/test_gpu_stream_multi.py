"""savgol_streambank_push_block_multi against its twins, bit for bit.

Every case makes banks A_k for the multi call and twins B_k -- the same configuration and flags -- for the single calls, and gives A_k and B_k the same
history (bank k's own: histories may differ inside one call).  Then the A banks take ONE savgol_streambank_push_block_multi and every B_k its own
savgol_streambank_push_block on the same samples.  Signals come from tests.stream_seams.signal; samples and outputs sit in stream_seams.Guarded tensors.
After every call: output k equals twin k's bit for bit (NaN positions coincide, payloads free); rows of ticks without an output and the guards still hold
the guard value; d_samples and its guards are unchanged; produced[k], the return value and the counters are equal.  After the last call both flushes
are bit-equal and the savgol_streambank_save blobs byte-equal.  For every half window one bit-exact-bank case also holds the twin itself to
stream_seams.dot_rows (the reference's order, pinned to the oracle in tests/test_stream_block_forms.py).  _route must answer the shipped rule
(include/savgol_hip.h): a build that only ever fell back to single calls does not pass.  No tolerance anywhere: the bar is bit equality."""
import ctypes as C

import numpy as np
import pytest

from tests import stream_seams as seams
from tests._util import bits

pytestmark = pytest.mark.gpu

f32 = np.float32
NAME = "savgol_streambank_push_block_multi"
FUSED_MAX_N = 8                                              # the shipped bound, both bank kinds, two and three outputs per launch
FILTERS = [(2, 0, 1.0), (2, 1, 1e-3), (3, 2, 0.5)]           # smoothing (uncentred), first and second derivative (centred on the fused bank): three dt_inv in one launch
TICKS = [64, 65, 95, 96, 97, 128, 161]                       # no body | one partial band ... | two bands | four bands, the last of one row


@pytest.fixture(scope="module")
def torch_gpu(sg):
    import torch
    assert torch.cuda.is_available() and sg.device_count() > 0, sg.last_error()
    return torch


def filters_for(n, sgo):
    out = [f if f[0] <= 2 * n and sgo.weights(n, f[0], f[1]) is not None else (2, f[1], f[2]) for f in FILTERS]
    assert all(sgo.weights(n, f[0], f[1]) is not None for f in out)
    return out


def same_words(got, want, what):
    """bit equality of two fp32 arrays; NaN positions coincide, NaN payloads are free"""
    assert got.shape == want.shape, what
    gn, wn = np.isnan(got), np.isnan(want)
    assert np.array_equal(gn, wn), (what, "NaN positions")
    bad = (bits(got) != bits(want)) & ~gn
    if bad.any():
        at = tuple(int(v) for v in np.argwhere(bad)[0])
        raise AssertionError((what, f"{int(bad.sum())} of {bad.size} words differ, first at {at}: got {got[at]!r} want {want[at]!r}"))


def expected_route(specs, streams, ticks, misaligned):
    """the shipped rule: fused launches of a call, 0 = single calls"""
    n, fma = specs[0][0], specs[0][4]
    fused = (len(specs) >= 2 and all(s[0] == n and s[4] == fma for s in specs) and n <= FUSED_MAX_N and streams % 128 == 0 and not misaligned and ticks > 64)
    return (2 if len(specs) == 4 else 1) if fused else 0


def run_case(sg, sgo, torch, streams, specs, calls, offset=0.0, off_in=0, off_out=(), seed=0, pin=False, follow=False, mutate=None, what=""):
    """specs: (n, m, d, dt, fma, history ticks) per bank; calls: the ticks of each multi call.  Returns the output words compared."""
    K = len(specs)
    what = (what, streams, specs, calls, offset, off_in, off_out)
    case = seams.Case("multi", streams, 0, 0, specs[0][0], 2, 0, 1.0, 0, offset, ())
    total = sum(calls)
    x = seams.signal(case, total, seed)
    if mutate is not None:
        mutate(x)
    past = seams.signal(case, max(max(s[5] for s in specs), 1), seed + 1)
    A = [sg.StreamBank(streams, s[0], s[1], s[2], s[3], fma=bool(s[4])) for s in specs]
    B = [sg.StreamBank(streams, s[0], s[1], s[2], s[3], fma=bool(s[4])) for s in specs]
    for k, s in enumerate(specs):
        if s[5]:
            h = torch.from_numpy(past[:s[5]]).cuda()
            ra, rb = A[k].push_block(h, s[5], torch.empty_like(h)), B[k].push_block(h, s[5], torch.empty_like(h))
            assert ra == rb >= 0, (what, sg.last_error())
    off_out = tuple(off_out) + (0,) * (K - len(off_out))
    t = words = 0
    for L in calls:
        xin = seams.Guarded(torch, L, streams, off_in, x[t:t + L])
        oa = [seams.Guarded(torch, L, streams, off_out[k]) for k in range(K)]
        ob = [seams.Guarded(torch, L, streams, off_out[k]) for k in range(K)]               # the twin takes the same pointers' alignment
        mis = ((off_in * 4) | max(o * 4 for o in off_out)) & 15
        route = sg.push_block_multi_route(A, xin.ptr(0), L, [o.ptr(0) for o in oa])
        assert route == expected_route(specs, streams, L, mis), (what, L, route, sg.last_error())
        before = [a.counters for a in A]
        assert sg.push_block_multi_route(A, xin.ptr(0), L, [o.ptr(0) for o in oa]) == route and [a.counters for a in A] == before
        pa = sg.push_block_multi(A, xin.ptr(0), L, [o.ptr(0) for o in oa])
        pb = [B[k].push_block(xin.ptr(0), L, ob[k].ptr(0)) for k in range(K)]
        torch.cuda.synchronize()
        assert pa == pb and min(pb) >= 0, (what, L, pa, pb, sg.last_error())
        assert [a.counters for a in A] == [b.counters for b in B], (what, L)
        assert np.array_equal(bits(xin.host()), bits(xin.want)), (what, L, "d_samples or its guards were written")
        for k in range(K):
            ga, gb = oa[k].host(), ob[k].host()
            assert oa[k].outside_intact(ga) and ob[k].outside_intact(gb), (what, L, k, "guards around d_out")
            ra, rb = oa[k].body(ga), ob[k].body(gb)
            silent = L - pb[k]
            assert np.array_equal(bits(ra[:silent]), bits(np.full((silent, streams), seams.GUARD, f32))), (what, L, k, "a row of a tick without an output was written")
            same_words(ra[silent:], rb[silent:], (what, L, k))
            words += ra[silent:].size
            if pin and not specs[k][4] and pb[k]:
                filt = sgo.Filter(*specs[k][:4])
                hist = np.concatenate([past[:specs[k][5]], x[:t + L]])
                ref = seams.dot_rows(filt.center, filt.dt_inv, hist, f32)[-pb[k]:]
                assert seams.same_bits(rb[silent:], ref), (what, L, k, "the fp32 twin left the oracle's bits")
        t += L
    if follow:
        # the banks the multi call left take a tick push, a fp32 block push and a 16-bit block push like their twins
        more = seams.signal(case, 1 + 40 + 70, seed + 2)
        row = torch.from_numpy(more[0]).cuda()
        blk = torch.from_numpy(more[1:41]).cuda()
        x16 = torch.from_numpy(more[41:]).to(torch.bfloat16).cuda()
        for k in range(K):
            outs = []
            for bank in (A[k], B[k]):
                o1 = torch.full((streams,), float(seams.GUARD), device="cuda")
                o2 = torch.full((40, streams), float(seams.GUARD), device="cuda")
                o3 = torch.full((70, streams), float(seams.GUARD), dtype=torch.bfloat16, device="cuda")
                r = (bank.push(row, o1), bank.push_block(blk, 40, o2), bank.push_block_h16(x16, "bf16", 70, o3))
                outs.append((r, o1, o2, o3))
            torch.cuda.synchronize()
            assert outs[0][0] == outs[1][0] and min(outs[0][0]) >= 0, (what, "follow-ups", outs[0][0], outs[1][0])
            assert torch.equal(outs[0][1].view(torch.int32), outs[1][1].view(torch.int32)), (what, k, "tick push after the multi call")
            assert torch.equal(outs[0][2].view(torch.int32), outs[1][2].view(torch.int32)), (what, k, "fp32 block push after the multi call")
            assert torch.equal(outs[0][3].view(torch.int16), outs[1][3].view(torch.int16)), (what, k, "16-bit block push after the multi call")
    for k in range(K):
        rows = specs[k][0]
        fa = torch.full((2, rows, streams), float(seams.GUARD), device="cuda")
        fb = torch.full((2, rows, streams), float(seams.GUARD), device="cuda")
        assert A[k].flush_leading(fa[0], rows) == B[k].flush_leading(fb[0], rows), what
        assert A[k].flush(fa[1], rows) == B[k].flush(fb[1], rows), what
        torch.cuda.synchronize()
        assert torch.equal(fa.view(torch.int32), fb.view(torch.int32)), (what, k, "flush rows")
        assert np.array_equal(A[k].save(), B[k].save()), (what, k, "save blobs")
    for bank in A + B:
        bank.close()
    return words


def case_list(n, fma, F):
    """(streams, specs, calls, keywords) of one (half window, bank kind): a pure function.  Not a cross product: every value of every axis occurs."""
    out = []
    H = [0, n, 2 * n, 2 * n + 1]

    def spec(fi, h, nn=n, flag=fma):
        f = F[fi % 3]
        return (nn, f[0], f[1], f[2], flag, h)

    # every length x count 2, 3, 4; histories round robin and different inside one call; 256 streams, 2176 = 17 strips (a narrower last group) and 128
    for i, L in enumerate(TICKS):
        count = 2 + i % 3
        streams = (256, 2176, 128)[i % 3] if L != 161 else 2176
        out.append((streams, [spec(k, H[(i + k) % 4]) for k in range(count)], [L], dict(pin=(i == 2))))
    # fresh banks, three filters in one launch, then a second multi call on the banks the first one left; follow-ups on the same banks
    out.append((256, [spec(k, 0) for k in range(3)], [97, 65], dict(follow=True, pin=True)))
    out.append((128, [spec(k + 1, 2 * n + 1) for k in range(4)], [161], dict()))
    out.append((256, [spec(1, n), spec(1, n)], [96], dict()))                                   # the same filter twice: two outputs that must be equal
    # one pointer 4 bytes off the 16-byte grid: single calls, the same bits
    out.append((256, [spec(0, n), spec(1, 0)], [97], dict(off_in=1)))
    out.append((256, [spec(0, 0), spec(1, n), spec(2, 0)], [97], dict(off_out=(0, 1, 0))))
    # a mixed-flag and a mixed-half-window call: single calls
    out.append((256, [spec(0, 0), spec(1, 0, flag=1 - fma)], [97], dict()))
    out.append((256, [spec(0, 0), spec(1, n, nn=n + 1), spec(2, 0)], [97], dict()))
    if fma:
        # what centring exists for: derivative banks on streams riding on an offset of 1000, beside a smoothing bank
        out.append((256, [spec(k, (0, 2 * n, n)[k]) for k in range(3)], [161], dict(offset=1000.0)))
    return out


@pytest.mark.parametrize("n,fma", [(n, fma) for n in (1, 4, 5, 6, 8) for fma in (0, 1)] + [(9, 0), (9, 1), (16, 0), (16, 1)])
def test_multi_block_push_equals_its_twins(sg, sgo, torch_gpu, n, fma):
    F = filters_for(n, sgo)
    todo = case_list(n, fma, F)
    words = fused = 0
    for i, (streams, specs, calls, kw) in enumerate(todo):
        words += run_case(sg, sgo, torch_gpu, streams, specs, calls, seed=1000 * n + 10 * i + fma, **kw)
        fused += any(expected_route(specs, streams, L, kw.get("off_in", 0) or any(kw.get("off_out", ()))) for L in calls)
    # n <= 8: most cases are fused; n = 9 and 16 (a fused-bank derivative filter among them): every call is single calls
    assert fused == (0 if n > FUSED_MAX_N else len(todo) - 5), (n, fma, fused, len(todo))
    assert words > 1000 * len(todo)
    print(f"n={n} {'fused' if fma else 'bit-exact'} bank: {len(todo)} cases ({fused} with a fused call), {words} output words compared")


@pytest.mark.parametrize("fma", [0, 1])
def test_multi_special_values(sg, sgo, torch_gpu, fma):
    """NaN and +-Inf samples in rows that the eight rows of a body tile's centre include (n = 4, band 2: ticks 56..63; band 3: 88..95), signed zeros,
    a stream of zeros: NaN positions coincide with the twins', every other word is bit-equal"""
    def mutate(x):
        x[58, 5] = np.nan
        x[60, 6] = np.inf
        x[57, 7] = -np.inf
        x[90, 200] = np.nan
        x[93, 201] = np.inf
        x[:, 8] = 0.0
        x[:, 9] = -0.0
        x[x.shape[0] - 3, 10] = np.nan                                     # an ordinary row of the last band

    F = filters_for(4, sgo)
    specs = [(4, f[0], f[1], f[2], fma, h) for f, h in zip(F, (0, 9, 4))]
    assert run_case(sg, sgo, torch_gpu, 256, specs, [161], seed=5, mutate=mutate, what="specials") > 0
    assert run_case(sg, sgo, torch_gpu, 256, specs[:2], [97], seed=6, offset=1000.0, mutate=mutate, what="specials, offset") > 0


def test_multi_refusals(sg, torch_gpu):
    """every refusal returns -1 with a text naming the call before anything is enqueued: counters and save blobs unchanged, every output still all guard"""
    torch = torch_gpu
    S, n, T = 256, 4, 97
    banks = [sg.StreamBank(S, n, 2, d, 1.0, fma=True) for d in (0, 1, 2)]
    other = sg.StreamBank(128, n, 2, 0, 1.0, fma=True)
    warm = torch.zeros((20, S), device="cuda")
    for b in banks:
        assert b.push_block(warm, 20, torch.empty_like(warm)) == 12
    torch.cuda.synchronize()
    blobs, counters = [b.save() for b in banks], [b.counters for b in banks]
    buf = torch.full((8 * T, S), float(seams.GUARD), device="cuda")
    src = buf[:T].data_ptr()
    o = [buf[(2 + 2 * k) * T:].data_ptr() for k in range(3)]
    row = 4 * S
    L = sg.lib()
    st = torch.cuda.current_stream().cuda_stream

    def arr(vals):
        return (C.c_void_p * len(vals))(*vals)

    def refused(text, bank_list, count, samples, ticks, outs):
        for fn, tail, who in ((L.savgol_streambank_push_block_multi, (None, st), NAME), (L.savgol_streambank_push_block_multi_route, (), NAME + "_route")):
            assert fn(arr([getattr(b, "ptr", b) for b in bank_list]), count, samples, ticks, arr(outs), *tail) == -1, text
            err = sg.last_error()
            assert err.startswith(who + ":") and text in err, (text, err)
            assert [b.counters for b in banks] == counters

    refused("outside 1..4", banks, 0, src, T, o)
    refused("NULL pointer: banks[1]", [banks[0], None, banks[2]], 3, src, T, o)
    refused("NULL pointer: d_outs[2]", banks, 3, src, T, [o[0], o[1], None])
    refused("listed twice", [banks[0], banks[1], banks[0]], 3, src, T, o)
    refused("streams", [banks[0], other], 2, src, T, o[:2])
    refused("2^30", banks, 3, src, (1 << 30) + 1, [src + (1 << 44), src + (1 << 45), src + (1 << 46)])
    for shift in (0, row, -row, T * row - 4, -(T * row - 4)):              # the samples and an output: the same rows ... one shared element at either end
        refused("d_samples and d_outs[1] overlap", banks, 3, o[1] + shift, T, o)
    for shift in (0, T * row - 4, -(T * row - 4)):                         # two outputs
        refused("d_outs[0] and d_outs[2] overlap", banks, 3, src, T, [o[0], o[1], o[0] + shift])
    banks[1].service_start()
    try:
        refused("tick service", banks, 3, src, T, o)
    finally:
        banks[1].service_stop()
    assert sg.push_block_multi(banks, src, 0, o) == [0, 0, 0] and [b.counters for b in banks] == counters
    assert L.savgol_streambank_push_block_multi(arr([b.ptr for b in banks]), 3, src, 0, arr(o), None, st) == 0
    torch.cuda.synchronize()
    assert bool((buf == float(seams.GUARD)).all())
    for b, blob in zip(banks, blobs):
        assert np.array_equal(b.save(), blob)
    # buffers that touch end to start are served; produced may be NULL and the return value is the smallest count
    touching = [src + T * row, src + 2 * T * row, src + 3 * T * row]
    assert L.savgol_streambank_push_block_multi(arr([b.ptr for b in banks]), 3, src, T, arr(touching), None, st) == T, sg.last_error()
    torch.cuda.synchronize()
    for b in banks + [other]:
        b.close()


def test_multi_refuses_a_bank_on_another_device(sg, torch_gpu):
    torch = torch_gpu
    if torch.cuda.device_count() < 2:
        pytest.skip("one GPU")
    banks = [sg.StreamBank(256, 4, 2, d, 1.0) for d in (0, 1)]
    buf = torch.full((3 * 97, 256), float(seams.GUARD), device="cuda:0")
    try:
        assert sg.lib().savgol_hip_set_device(1) == 0
        with pytest.raises(RuntimeError, match="lives on device 0"):
            sg.push_block_multi(banks, buf[:97], 97, [buf[97:194], buf[194:]])
        assert NAME in sg.last_error()
    finally:
        sg.lib().savgol_hip_set_device(0)
    assert [b.counters for b in banks] == [(0, 0), (0, 0)]
    for b in banks:
        b.close()


def test_multi_fused_call_in_a_graph(sg, sgo, torch_gpu):
    """after one warm-up call a fused call (three heads, one body launch, three tail stores; no allocation) is captured and replays to the same bits on
    reset banks"""
    torch = torch_gpu
    S, n, T = 256, 5, 161
    F = filters_for(n, sgo)
    case = seams.Case("graph", S, 0, 0, n, 2, 0, 1.0, 1, 0.0, ())
    x = torch.from_numpy(seams.signal(case, T, 9)).cuda()
    banks = [sg.StreamBank(S, n, f[0], f[1], f[2], fma=True) for f in F]
    want = [torch.full((T, S), float(seams.GUARD), device="cuda") for _ in F]
    assert sg.push_block_multi_route(banks, x, T, want) == 1
    assert sg.push_block_multi(banks, x, T, want) == [T - 2 * n] * 3
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
            assert sg.push_block_multi(banks, x, T, out, stream=s) == [T - 2 * n] * 3, sg.last_error()
    for o in out:
        o.fill_(float(seams.GUARD))
    torch.cuda.synchronize()
    g.replay()
    torch.cuda.synchronize()
    for o, w in zip(out, want):
        assert torch.equal(o.view(torch.int32), w.view(torch.int32))
    for b, blob in zip(banks, blobs):
        assert np.array_equal(b.save(), blob)
        b.close()
