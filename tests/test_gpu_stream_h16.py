"""savgol_streambank_push_block_h16 against its twin, bit for bit.

Every case makes two fresh banks of the same configuration and flags and gives both the same history through fp32 calls.  Then bank A takes the 16-bit
call and bank B -- the twin -- the fp32 savgol_streambank_push_block on the same samples widened (tensor.float(): exact) in fresh, aligned fp32 tensors.
Signals come from tests.stream_seams.signal, rounded into the input type first.  Expected rows are B's rows rounded on the CPU with tensor.to(dtype):
round to nearest even, checked below on ties, overflow and subnormals of both types.  A's buffers sit inside larger tensors pre-filled with a guard.
After every call: the output rows equal the expected ones bit for bit (NaN positions coincide, payloads free); rows of ticks without an output and the
guards around d_out are still the guard; d_samples and its guards are unchanged; return values and counters are equal.  After the last call both
flushes are bit-equal and the savgol_streambank_save blobs byte-equal.  For every half window one bit-exact-bank case also holds B itself to
stream_seams.dot_rows (the reference's order, pinned to the oracle in tests/test_stream_block_forms.py) on the widened input.
No tolerance anywhere: the bar is bit equality."""
import numpy as np
import pytest

from tests import stream_seams as seams

pytestmark = pytest.mark.gpu

HALF_WINDOWS = [1, 5, 6, 11, 12, 16, 17, 20, 21, 32]       # the seams of the launch tables, the moment range and the lo / hi objects
ALL_PAIRS = [("bf16", "bf16"), ("f16", "f16"), ("f16", "f32"), ("bf16", "f32")]
GUARD = -7.0
GUARD_ROWS = 2
STAGED_MAX = 1 << 24


@pytest.fixture(scope="module")
def torch_gpu(sg):
    import torch
    assert torch.cuda.is_available() and sg.device_count() > 0, sg.last_error()
    return torch


def tdtype(torch, name):
    return {"f16": torch.float16, "bf16": torch.bfloat16, "f32": torch.float32}[name]


def as_int(torch, t):
    return t.view(torch.int32 if t.dtype == torch.float32 else torch.int16)


def same_words(torch, got, want, what):
    """bit equality; NaN positions coincide, NaN payloads are free"""
    assert got.shape == want.shape and got.dtype == want.dtype, what
    gn, wn = torch.isnan(got), torch.isnan(want)
    assert torch.equal(gn, wn), (what, "NaN positions")
    a, b = as_int(torch, got).masked_fill(gn, 0), as_int(torch, want).masked_fill(wn, 0)
    if not torch.equal(a, b):
        bad = (a != b).nonzero()
        raise AssertionError((what, f"{bad.shape[0]} of {a.numel()} words differ, first at {bad[0].tolist()}: got {got[tuple(bad[0])].item()!r} want {want[tuple(bad[0])].item()!r}"))


def chunk_ticks(streams, ticks):
    """the staged route's chunks, as include/savgol_hip.h states them"""
    return ticks if streams * ticks <= STAGED_MAX else max(64, (STAGED_MAX // streams) & ~63)


class Guarded:
    """[ticks][streams] rows of `dtype` inside a larger tensor pre-filled with the guard, `off` elements off the tensor's (aligned) base"""

    def __init__(self, torch, ticks, streams, dtype, off=0):
        self.g = GUARD_ROWS * streams
        self.count = ticks * streams
        self.whole = torch.full((2 * self.g + off + self.count + 8,), GUARD, dtype=dtype, device="cuda")
        self.lo = self.g + off
        self.rows = self.whole[self.lo:self.lo + self.count].view(ticks, streams)
        self.torch = torch

    def ptr(self):
        return self.rows.data_ptr()

    def guards_intact(self):
        t = self.torch
        return bool((self.whole[:self.lo] == GUARD).all()) and bool((self.whole[self.lo + self.count:] == GUARD).all())


def run_case(sg, torch, streams, n, filt, fma, pair, calls, off_in=0, off_out=0, offset=0.0, seed=0, twin_chunks=False, pin=None, mutate=None, what=""):
    """calls: ("tick", k) = k fp32 pushes on both banks, ("block", L) = one fp32 block push on both, ("h16", L) = the 16-bit call on A, the fp32 block push on B"""
    m, d, dt = filt
    what = (what, streams, n, filt, fma, pair, calls, off_in, off_out)
    idt, odt = tdtype(torch, pair[0]), tdtype(torch, pair[1])
    total = sum(k for _, k in calls)
    case = seams.Case("h16", streams, 0, 0, n, m, d, dt, fma, offset, ())
    xq = torch.from_numpy(seams.signal(case, total, seed)).to(idt)           # quantised into the input type on the CPU, nearest even
    if mutate is not None:
        mutate(xq)
    x32 = xq.float().cuda()                                                   # widened exactly
    xq = xq.cuda()
    A, B = sg.StreamBank(streams, n, m, d, dt, fma=bool(fma)), sg.StreamBank(streams, n, m, d, dt, fma=bool(fma))
    t = words = 0
    for kind, k in calls:
        if kind == "tick":
            for i in range(k):
                row = x32[t + i].clone()
                oa, ob = torch.full((streams,), GUARD, device="cuda"), torch.full((streams,), GUARD, device="cuda")
                assert A.push(row, oa) == B.push(row, ob) >= 0, what
        elif kind == "block":
            blk = x32[t:t + k].clone()
            oa, ob = torch.full((k, streams), GUARD, device="cuda"), torch.full((k, streams), GUARD, device="cuda")
            assert A.push_block(blk, k, oa) == B.push_block(blk, k, ob) >= 0, what
            assert torch.equal(oa, ob), what
        else:
            src, dst = Guarded(torch, k, streams, idt, off_in), Guarded(torch, k, streams, odt, off_out)
            src.rows.copy_(xq[t:t + k])
            keep = src.whole.clone()
            ra = A.push_block_h16(src.ptr(), pair[0], k, dst.ptr(), pair[1])
            assert ra >= 0, (what, sg.last_error())
            blk = x32[t:t + k].clone()
            ob = torch.full((k, streams), GUARD, device="cuda")
            step = chunk_ticks(streams, k) if twin_chunks else k
            rb = 0
            for done in range(0, k, step):
                part = min(step, k - done)
                r = B.push_block(blk[done:done + part], part, ob[done:done + part])
                assert r >= 0, (what, sg.last_error())
                rb += r
            torch.cuda.synchronize()
            assert ra == rb and A.counters == B.counters, (what, ra, rb, A.counters, B.counters)
            want = ob[k - rb:].cpu().to(odt).cuda()                          # rounded once, on the CPU
            same_words(torch, dst.rows[k - rb:], want, what)
            words += want.numel()
            assert bool((dst.rows[:k - rb] == GUARD).all()), (what, "a row of a tick without an output was written")
            assert dst.guards_intact(), (what, "guards around d_out")
            assert torch.equal(as_int(torch, src.whole), as_int(torch, keep)), (what, "d_samples or its guards changed")
            if pin is not None and rb:
                # the yardstick itself: B's fp32 rows against the reference's order on the widened input (bit-exact bank only)
                hist = x32[:t + k].cpu().numpy()
                ref = seams.dot_rows(pin.center, pin.dt_inv, hist, np.float32)[-rb:]
                assert seams.same_bits(ob[k - rb:].cpu().numpy(), ref), (what, "the fp32 twin left the oracle's bits")
        t += k
    rows = min(n, 32)
    fa, fb = torch.full((2, rows, streams), GUARD, device="cuda"), torch.full((2, rows, streams), GUARD, device="cuda")
    assert A.flush_leading(fa[0], rows) == B.flush_leading(fb[0], rows), what
    assert A.flush(fa[1], rows) == B.flush(fb[1], rows), what
    torch.cuda.synchronize()
    assert torch.equal(fa.view(torch.int32), fb.view(torch.int32)), (what, "flush rows")
    assert np.array_equal(A.save(), B.save()), (what, "save blobs")
    A.close()
    B.close()
    return words


def test_cpu_rounding_is_nearest_even(torch_gpu):
    """tensor.to(dtype) on the CPU, the rounding the expected values go through: ties to even, overflow to Inf, gradual underflow"""
    torch = torch_gpu
    f16 = [(1 + 2.0 ** -11, 1.0), (1 + 3 * 2.0 ** -11, 1 + 2.0 ** -9), (65519.0, 65504.0), (65520.0, float("inf")), (-65520.0, float("-inf")),
           (2.0 ** -25, 0.0), (3 * 2.0 ** -25, 2.0 ** -23), (2.0 ** -24, 2.0 ** -24), (1.5 * 2.0 ** -24, 2.0 ** -23), (-0.0, -0.0)]
    bf16 = [(1 + 2.0 ** -8, 1.0), (1 + 3 * 2.0 ** -8, 1 + 2.0 ** -6), (3.3895313892515355e38, 3.3895313892515355e38), (3.4e38, float("inf")),
            (2.0 ** -134, 0.0), (3 * 2.0 ** -134, 2.0 ** -132), (2.0 ** -133, 2.0 ** -133)]
    for dtype, table in ((torch.float16, f16), (torch.bfloat16, bf16)):
        src = torch.tensor([a for a, _ in table], dtype=torch.float32)
        want = torch.tensor([b for _, b in table], dtype=torch.float64)
        got = src.to(dtype)
        assert torch.equal(got.double(), want), (dtype, got.double().tolist())
        assert torch.equal(torch.signbit(got), torch.signbit(src))


def case_list(n, fma):
    """(streams, pair, calls, off_in, off_out, offset, filter index, pinned?) of one (half window, bank): a pure function"""
    ws = 2 * n + 1
    F = seams.bank_filters(n, fma)
    H = [0, 1, 2 * n - 1, 2 * n, 2 * n + 2, 2 * n % 32]
    TL = [64, 65, 95, 96, 97, 128, 64 + 32 * 3 + 7]
    pairs = ALL_PAIRS if n in (5, 16, 32) else ALL_PAIRS[:1]
    out = []

    def add(streams, calls, fi, off_in=0, off_out=0, offset=0.0, pair=None, pin=False):
        calls = tuple((kind, int(k)) for kind, k in calls if k > 0)
        out.append((streams, pair or pairs[len(out) % len(pairs)], calls, off_in, off_out, offset, fi % len(F), pin))

    # ---- the tile route: whole strips, at least 64 ticks ----
    i = 0
    for streams in (256, 2176):                                            # 2176 = 17 strips: the moment tiles' last group of one
        for L in TL:
            for fi in range(len(F) if streams == 256 else 1):
                add(streams, [("tick", H[i % len(H)]), ("h16", L)], fi + (i if streams == 2176 else 0), pin=not fma and fi == 0)
                i += 1
    for pair in pairs:                                                     # every pair on one shape, a full ring behind it
        add(256, [("tick", ws + 2), ("h16", 97)], 0, pair=pair)
        add(260, [("tick", 1), ("h16", ws)], 0, pair=pair)
    add(16512, [("h16", 97)], 0)                                           # 129 strips: the empty tail of the tile order
    # ---- the staged route ----
    for si, streams in enumerate((1, 130, 260, 777)):
        for j, L in enumerate((1, 2 * n, ws, 63, 16 * ws)):
            add(streams, [("tick", H[(si + j) % len(H)]), ("h16", L)], si + j)
    add(256, [("tick", n), ("h16", 97)], 0, off_in=1)                      # 2 bytes off
    add(256, [("tick", n), ("h16", 97)], 1, off_in=4)                      # 8 bytes off
    add(256, [("tick", n), ("h16", 97)], 2, off_out=1)
    # ---- hand-over between the 16-bit call, ticks and the fp32 block push ----
    for fi in range(len(F)):
        add(256, [("h16", 96), ("tick", 3), ("h16", 63), ("block", 40), ("h16", 65)], fi)
    # ---- what centring exists for: derivative filters on the fused bank, streams riding on 1000 ----
    if fma:
        for fi, f in enumerate(F):
            if f[1] > 0:
                add(256, [("tick", 2 * n % 32), ("h16", 97)], fi, offset=1000.0)
                add(130, [("tick", 1), ("h16", 16 * ws)], fi, offset=1000.0)
    return out


@pytest.mark.parametrize("n,fma", [(n, fma) for n in HALF_WINDOWS for fma in (0, 1)])
def test_h16_block_push_equals_its_twin(sg, sgo, torch_gpu, n, fma):
    F = seams.bank_filters(n, fma)
    todo = case_list(n, fma)
    assert {c[1] for c in todo} == set(ALL_PAIRS if n in (5, 16, 32) else ALL_PAIRS[:1])
    pinned = words = 0
    for k, (streams, pair, calls, off_in, off_out, offset, fi, pin) in enumerate(todo):
        f = F[fi]
        words += run_case(sg, torch_gpu, streams, n, f, fma, pair, calls, off_in, off_out, offset, seed=1000 * n + 10 * k + fma,
                 pin=sgo.Filter(n, f[0], f[1], f[2]) if pin else None)
        pinned += bool(pin)
    assert (fma or pinned >= 1) and words > 1000 * len(todo)
    print(f"n={n} {'fused' if fma else 'bit-exact'} bank: {len(todo)} cases, {words} output words compared, {pinned} cases pinned to the oracle's order")


def test_h16_chunked_call_equals_the_chunked_twin(sg, torch_gpu):
    """130 streams x enough ticks to pass 2^24 stream-ticks, on a fused derivative bank: the twin takes the same fp32 block pushes chunk by chunk"""
    streams = 130
    ticks = STAGED_MAX // streams + 100
    assert streams * ticks > STAGED_MAX and chunk_ticks(streams, ticks) == 129024 < ticks
    words = run_case(sg, torch_gpu, streams, 16, (2, 1, 1e-3), 1, ("bf16", "bf16"), (("tick", 3), ("h16", ticks)), seed=77, twin_chunks=True, what="chunked")
    assert words == (ticks + 3 - 32) * streams


@pytest.mark.parametrize("fma", [0, 1])
def test_h16_special_values(sg, torch_gpu, fma):
    """fp16 input holding subnormals, +-0, +-Inf and NaN in a few streams, on both routes: NaN positions coincide, every other word is bit-equal"""
    torch = torch_gpu

    def mutate(x):
        bits = x.view(torch.int16)
        T = x.shape[0]
        bits[:, 3] = torch.arange(T, dtype=torch.int16) % 1024                       # +0 and positive subnormals
        bits[:, 4] = (torch.arange(T, dtype=torch.int16) % 1024) | -32768            # -0 and negative subnormals
        x[T // 2, 5] = float("inf")
        x[T // 3, 6] = float("-inf")
        x[T // 2, 7] = float("nan")
        x[:, 8] = 0.0
        x[:, 9] = -0.0
        x[:, 10] = 80.0 * torch.arange(T, dtype=torch.float32)                       # a ramp whose derivative (x 1000) overflows fp16 on the way out: +Inf
        x[:, 11] = -80.0 * torch.arange(T, dtype=torch.float32)
        x[:, 129] = x[:, 3]

    for streams, L in ((256, 97), (130, 63)):
        for pair in (("f16", "f16"), ("f16", "f32")):
            for filt in ((2, 0, 1.0), (2, 1, 1e-3)):
                run_case(sg, torch, streams, 5, filt, fma, pair, (("tick", 11), ("h16", L)), seed=5, mutate=mutate, what="specials")


def test_h16_refusals(sg, torch_gpu):
    """every refusal returns -1 with its text before anything is enqueued: counters and save blob unchanged, d_out still all guard"""
    torch = torch_gpu
    S, n, T = 256, 8, 64
    bank = sg.StreamBank(S, n, 2, 0, 1.0)
    warm = torch.zeros((20, S), device="cuda")
    assert bank.push_block(warm, 20, torch.empty_like(warm)) == 4
    torch.cuda.synchronize()
    blob, counters = bank.save(), bank.counters
    buf = torch.full((4 * T, S), GUARD, dtype=torch.float16, device="cuda")
    src, dst = buf[:T], buf[2 * T:3 * T]
    L = sg.lib()
    F16, BF16, F32 = sg.SAVGOL_HIP_F16, sg.SAVGOL_HIP_BF16, sg.SAVGOL_HIP_F32
    name = "savgol_streambank_push_block_h16"

    def refused(text, *args):
        assert L.savgol_streambank_push_block_h16(*args) == -1, text
        err = sg.last_error()
        assert name in err and text in err, (text, err)
        assert bank.counters == counters

    st = torch.cuda.current_stream().cuda_stream
    refused("NULL pointer", None, src.data_ptr(), F16, T, dst.data_ptr(), F16, st)
    refused("NULL pointer", bank.ptr, None, F16, T, dst.data_ptr(), F16, st)
    refused("NULL pointer", bank.ptr, src.data_ptr(), F16, T, None, F16, st)
    for it, ot, text in ((F32, F32, "f32 -> f32"), (F16, BF16, "f16 -> bf16"), (BF16, F16, "bf16 -> f16"), (F32, F16, "f32 -> f16"), (7, F16, "unknown -> f16")):
        refused(text, bank.ptr, src.data_ptr(), it, T, dst.data_ptr(), ot, st)
    row = S * 2
    for shift in (0, -row, row, T * row - 2, -(T * row - 2)):                 # 16 -> 16 bit: the same rows ... one shared element at either end
        refused("overlap", bank.ptr, src.data_ptr() + T * row, F16, T, src.data_ptr() + T * row + shift, F16, st)
    # 16 bit -> fp32: the output range is twice as long, compared byte-wise: its last two bytes on the samples' first two, and the samples' last two on its first
    refused("overlap", bank.ptr, buf.data_ptr() + 2 * T * row, F16, T, buf.data_ptr() + 2, F32, st)
    refused("overlap", bank.ptr, buf.data_ptr(), F16, T, buf.data_ptr() + T * row - 2, F32, st)
    refused("2^30", bank.ptr, src.data_ptr(), F16, (1 << 30) + 1, buf.data_ptr() + (1 << 40), F16, st)
    assert bank.push_block_h16(src, "f16", 0, dst) == 0 and bank.counters == counters
    bank.service_start()
    try:
        refused("tick service", bank.ptr, src.data_ptr(), F16, T, dst.data_ptr(), F16, st)
    finally:
        bank.service_stop()
    torch.cuda.synchronize()
    assert bool((buf == GUARD).all()) and np.array_equal(bank.save(), blob)
    # touching end to start is served: fp32 outputs right behind the samples
    assert L.savgol_streambank_push_block_h16(bank.ptr, buf.data_ptr(), F16, T, buf.data_ptr() + T * row, F32, st) == T, sg.last_error()
    torch.cuda.synchronize()
    bank.close()


def test_h16_refuses_a_bank_on_another_device(sg, torch_gpu):
    torch = torch_gpu
    if torch.cuda.device_count() < 2:
        pytest.skip("one GPU")
    bank = sg.StreamBank(256, 8, 2, 0, 1.0)
    buf = torch.full((128, 256), GUARD, dtype=torch.float16, device="cuda:0")
    try:
        assert sg.lib().savgol_hip_set_device(1) == 0
        assert bank.push_block_h16(buf[:64], "f16", 64, buf[64:]) == -1
        assert "savgol_streambank_push_block_h16" in sg.last_error() and "lives on device 0" in sg.last_error()
    finally:
        sg.lib().savgol_hip_set_device(0)
    assert bank.counters == (0, 0)
    bank.close()


@pytest.mark.parametrize("fma,pair", [(1, ("bf16", "bf16")), (0, ("f16", "f32"))])
def test_h16_tile_route_in_a_graph(sg, torch_gpu, fma, pair):
    """after one warm-up call a tile-route call (head, body, tail store, one scratch allocation) is captured and replays to the same bits on a reset bank"""
    torch = torch_gpu
    S, n, T = 256, 16, 167
    case = seams.Case("graph", S, 0, 0, n, 2, 1, 1e-3, fma, 0.0, ())
    x = torch.from_numpy(seams.signal(case, T, 9)).to(tdtype(torch, pair[0])).cuda()
    bank = sg.StreamBank(S, n, 2, 1, 1e-3, fma=bool(fma))
    want = torch.full((T, S), GUARD, dtype=tdtype(torch, pair[1]), device="cuda")
    assert bank.push_block_h16(x, pair[0], T, want, pair[1]) == T - 2 * n
    torch.cuda.synchronize()
    blob = bank.save()
    out = torch.full_like(want, GUARD)
    bank.reset()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(s):
        with torch.cuda.graph(g, stream=s):
            assert bank.push_block_h16(x, pair[0], T, out, pair[1], stream=s) == T - 2 * n, sg.last_error()
    out.fill_(GUARD)
    torch.cuda.synchronize()
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(as_int(torch, out), as_int(torch, want))
    assert np.array_equal(bank.save(), blob)
    bank.close()
