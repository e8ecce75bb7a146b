"""savgol_streambank_push_block_i16 against its twin, bit for bit.

Every case makes fresh banks of the same configuration and flags and gives all of them the same history through fp32 calls.  Then bank A (one per
output type of the case) takes the int16 call and bank B -- the twin -- the fp32 savgol_streambank_push_block on the same samples widened
(tensor.float(): exact) in fresh, aligned fp32 tensors; B runs once per case and serves every output type.  Signals come from
tests.stream_seams.signal, scaled to an amplitude in counts chosen per filter (amplitude() below) and quantised to int16 on the CPU.  Expected int16
rows are B's rows converted on the CPU -- torch.round / nan_to_num / clamp / cast: round to nearest even, saturate, NaN gives 0, checked below on
ties, both ends of the range, +-Inf and NaN; expected fp32 rows are B's rows themselves.  A's buffers sit inside larger tensors pre-filled with a
guard.  After every call: the output rows equal the expected ones bit for bit (fp32: NaN positions coincide, payloads free); rows of ticks without
an output and the guards around d_out are still the guard; d_samples and its guards are unchanged; return values and counters are equal.  After the
last call both flushes are bit-equal and the savgol_streambank_save blobs byte-equal.  For every half window one bit-exact-bank case also holds B
itself to stream_seams.dot_rows (the reference's order, pinned to the oracle in tests/test_stream_block_forms.py) on the widened input.  Every
int16 -> int16 case asserts that at least half of its expected words lie strictly inside (-32768, 32767): saturation is tested on purpose, in a case
of its own.  No tolerance anywhere: the bar is bit equality."""
import numpy as np
import pytest

from tests import stream_seams as seams

pytestmark = pytest.mark.gpu

HALF_WINDOWS = [1, 5, 6, 11, 12, 16, 17, 20, 21, 32]       # the seams of the launch tables, the moment range and the lo / hi objects
BOTH = ("i16", "f32")
GUARD = -7.0
GUARD_ROWS = 2
STAGED_MAX = 1 << 24
RIDE = 30000.0                                              # counts the streams of the centring cases ride at


@pytest.fixture(scope="module")
def torch_gpu(sg):
    import torch
    assert torch.cuda.is_available() and sg.device_count() > 0, sg.last_error()
    return torch


def tdtype(torch, name):
    return {"i16": torch.int16, "f32": torch.float32}[name]


def as_int(torch, t):
    return t.view(torch.int32 if t.dtype == torch.float32 else torch.int16)


def to_i16(torch, w):
    """the contract's conversion of fp32 rows, on the CPU (as tests/test_gpu_1d_i16.py): nearest even, saturated, NaN -> 0"""
    assert w.device.type == "cpu" and w.dtype == torch.float32
    return torch.clamp(torch.nan_to_num(torch.round(w), nan=0.0), -32768, 32767).to(torch.int16)


def amplitude(n, filt, offset=0.0):
    """counts per unit of stream_seams.signal (a tone of 0.5 .. 1.5 plus noise of 0.4), by filter: the int16 OUTPUT must stay inside the range for at
    least half of its words (asserted per case) and still be tens of counts large.  Smoothing: the samples themselves fill most of the range.
    d = 1, dt = 1e-3: the output is 1000 x the slope per tick (at n = 1 the noise alone gives 0.28 x 1000 x the amplitude; the tone 70 x).
    d = 2, dt = 0.5: 4 x the second difference, which at n = 1 is 2.4 x the noise and falls with n^2.5: the amplitude grows with n^2 up to the
    smoothing banks'.  Streams riding at RIDE keep a swing of a few hundred counts so that the samples stay under 32767."""
    m, d, dt = filt
    if d == 1:
        return 60.0
    if offset:
        return 300.0
    if d == 2:
        return min(8000.0, 300.0 * n * n)
    return 8000.0


def quantise(case, ticks, seed, amp):
    """stream_seams.signal scaled to `amp` counts around case.offset counts -> int16, on the CPU"""
    x = seams.signal(case._replace(offset=0.0), ticks, seed).astype(np.float64) * amp + case.offset
    return np.clip(np.rint(x), -32768, 32767).astype(np.int16)


def same_words(torch, got, want, what):
    """bit equality; fp32: NaN positions coincide, NaN payloads are free"""
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

    def ptr(self):
        return self.rows.data_ptr()

    def guards_intact(self):
        return bool((self.whole[:self.lo] == GUARD).all()) and bool((self.whole[self.lo + self.count:] == GUARD).all())


def run_case(sg, torch, streams, n, filt, fma, outs, calls, off_in=0, off_out=0, offset=0.0, seed=0, twin_chunks=False, pin=None, mutate=None,
             history=None, saturating=False, what=""):
    """calls: ("tick", k) = k fp32 pushes on every bank, ("block", L) = one fp32 block push on every bank, ("i16", L) = the int16 call on the A banks
    (one per output type in `outs`), the fp32 block push on B.  mutate(xq): edits the int16 samples; history(x32): edits the widened samples (the
    rows that fp32 calls push: NaN and +-Inf can only reach the ring that way).  Returns the words compared and B's rows of the last int16 call."""
    m, d, dt = filt
    what = (what, streams, n, filt, fma, outs, calls, off_in, off_out, offset)
    total = sum(k for _, k in calls)
    case = seams.Case("i16", streams, 0, 0, n, m, d, dt, fma, offset, ())
    xq = torch.from_numpy(quantise(case, total, seed, amplitude(n, filt, offset)))
    if mutate is not None:
        mutate(xq)
    x32 = xq.float()                                                          # widened exactly
    if history is not None:
        history(x32)
    x32, xq = x32.cuda(), xq.cuda()
    A = {o: sg.StreamBank(streams, n, m, d, dt, fma=bool(fma)) for o in outs}
    B = sg.StreamBank(streams, n, m, d, dt, fma=bool(fma))
    banks = list(A.values()) + [B]
    t = words = 0
    last = None
    for kind, k in calls:
        if kind == "tick":
            for i in range(k):
                row = x32[t + i].clone()
                rcs = [b.push(row, torch.full((streams,), GUARD, device="cuda")) for b in banks]
                assert len(set(rcs)) == 1 and rcs[0] >= 0, what
        elif kind == "block":
            blk = x32[t:t + k].clone()
            res = [torch.full((k, streams), GUARD, device="cuda") for _ in banks]
            rcs = [b.push_block(blk, k, o) for b, o in zip(banks, res)]
            assert len(set(rcs)) == 1 and rcs[0] >= 0, what
            assert all(torch.equal(o, res[-1]) for o in res), what
        else:
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
            twin_rows = ob[k - rb:].cpu()
            if pin is not None and rb:
                # the yardstick itself: B's fp32 rows against the reference's order on the widened input (bit-exact bank only)
                hist = x32[:t + k].cpu().numpy()
                ref = seams.dot_rows(pin.center, pin.dt_inv, hist, np.float32)[-rb:]
                assert seams.same_bits(twin_rows.numpy(), ref), (what, "the fp32 twin left the oracle's bits")
            for o in outs:
                src, dst = Guarded(torch, k, streams, torch.int16, off_in), Guarded(torch, k, streams, tdtype(torch, o), off_out)
                src.rows.copy_(xq[t:t + k])
                keep = src.whole.clone()
                ra = A[o].push_block_i16(src.ptr(), k, dst.ptr(), o)
                assert ra >= 0, (what, o, sg.last_error())
                torch.cuda.synchronize()
                assert ra == rb and A[o].counters == B.counters, (what, o, ra, rb, A[o].counters, B.counters)
                want = twin_rows if o == "f32" else to_i16(torch, twin_rows)  # converted once, on the CPU
                if o == "i16" and not saturating and want.numel():
                    inside = int(((want > -32768) & (want < 32767)).sum())
                    assert 2 * inside >= want.numel(), (what, f"only {inside} of {want.numel()} expected words are inside the int16 range: the case tests saturation")
                same_words(torch, dst.rows[k - rb:], want.cuda(), (what, o))
                words += want.numel()
                assert bool((dst.rows[:k - rb] == GUARD).all()), (what, o, "a row of a tick without an output was written")
                assert dst.guards_intact(), (what, o, "guards around d_out")
                assert torch.equal(src.whole, keep), (what, o, "d_samples or its guards changed")
            last = twin_rows
        t += k
    rows = min(n, 32)
    fl = [torch.full((2, rows, streams), GUARD, device="cuda") for _ in banks]
    assert len({b.flush_leading(f[0], rows) for b, f in zip(banks, fl)}) == 1, what
    assert len({b.flush(f[1], rows) for b, f in zip(banks, fl)}) == 1, what
    torch.cuda.synchronize()
    blob = B.save()
    for o, f in zip(outs, fl):
        assert torch.equal(f.view(torch.int32), fl[-1].view(torch.int32)), (what, o, "flush rows")
        assert np.array_equal(A[o].save(), blob), (what, o, "save blobs")
    for b in banks:
        b.close()
    return words, last


def test_cpu_conversion_is_the_contracts(torch_gpu):
    """round / nan_to_num / clamp / cast on the CPU, the conversion the expected values go through: ties to even, both ends saturate, +-Inf, NaN -> 0"""
    torch = torch_gpu
    table = [(0.5, 0), (-0.5, 0), (1.5, 2), (-1.5, -2), (2.5, 2), (-2.5, -2), (0.49999997, 0), (0.50000006, 1), (32766.5, 32766), (32767.0, 32767),
             (32767.5, 32767), (32768.0, 32767), (-32768.0, -32768), (-32768.5, -32768), (-32769.0, -32768), (1e9, 32767), (-1e9, -32768), (3e38, 32767),
             (float("inf"), 32767), (float("-inf"), -32768), (float("nan"), 0), (-0.0, 0), (123.0, 123), (-7.49, -7)]
    src = torch.tensor([a for a, _ in table], dtype=torch.float32)
    got = to_i16(torch, src)
    assert got.dtype == torch.int16 and got.tolist() == [b for _, b in table], got.tolist()


def case_list(n, fma):
    """(streams, calls, off_in, off_out, offset, filter index, pinned?) of one (half window, bank): a pure function"""
    ws = 2 * n + 1
    F = seams.bank_filters(n, fma)
    H = [0, 1, 2 * n - 1, 2 * n, 2 * n + 2, 2 * n % 32]
    TL = [64, 65, 95, 96, 97, 128, 64 + 32 * 3 + 7]
    out = []

    def add(streams, calls, fi, off_in=0, off_out=0, offset=0.0, pin=False):
        calls = tuple((kind, int(k)) for kind, k in calls if k > 0)
        out.append((streams, calls, off_in, off_out, offset, fi % len(F), pin))

    # ---- the tile route: whole strips, at least 64 ticks ----
    i = 0
    for streams in (256, 2176):                                            # 2176 = 17 strips: the moment tiles' last group of one
        for L in TL:
            for fi in range(len(F) if streams == 256 else 1):
                add(streams, [("tick", H[i % len(H)]), ("i16", L)], fi + (i if streams == 2176 else 0), pin=not fma and fi == 0)
                i += 1
    add(256, [("tick", ws + 2), ("i16", 97)], 0)                           # a full ring behind the call
    add(260, [("tick", 1), ("i16", ws)], 0)
    add(16512, [("i16", 97)], 0)                                           # 129 strips: the empty tail of the tile order
    # ---- the staged route ----
    for si, streams in enumerate((1, 130, 260, 777)):
        for j, L in enumerate((1, 2 * n, ws, 63, 16 * ws)):
            add(streams, [("tick", H[(si + j) % len(H)]), ("i16", L)], si + j)
    add(256, [("tick", n), ("i16", 97)], 0, off_in=1)                      # the input 2 bytes off
    add(256, [("tick", n), ("i16", 97)], 1, off_in=4)                      # 8 bytes off
    add(256, [("tick", n), ("i16", 97)], 2, off_out=1)                     # the output one element off (2 bytes as int16)
    # ---- hand-over between the int16 call, ticks and the fp32 block push ----
    for fi in range(len(F)):
        add(256, [("i16", 96), ("tick", 3), ("i16", 63), ("block", 40), ("i16", 65)], fi)
    # ---- what centring exists for: derivative filters on the fused bank, streams riding at 30 000 counts with a swing of a few hundred ----
    if fma:
        for fi, f in enumerate(F):
            if f[1] > 0:
                add(256, [("tick", 2 * n % 32), ("i16", 97)], fi, offset=RIDE)
                add(130, [("tick", 1), ("i16", 16 * ws)], fi, offset=RIDE)
    return out


@pytest.mark.parametrize("n,fma", [(n, fma) for n in HALF_WINDOWS for fma in (0, 1)])
def test_i16_block_push_equals_its_twin(sg, sgo, torch_gpu, n, fma):
    F = seams.bank_filters(n, fma)
    todo = case_list(n, fma)
    outs = BOTH if n in (5, 16, 32) else BOTH[:1]                          # both outputs on every shape at the three half windows, int16 -> int16 elsewhere
    pinned = words = 0
    for k, (streams, calls, off_in, off_out, offset, fi, pin) in enumerate(todo):
        f = F[fi]
        words += run_case(sg, torch_gpu, streams, n, f, fma, outs, calls, off_in, off_out, offset, seed=1000 * n + 10 * k + fma,
                          pin=sgo.Filter(n, f[0], f[1], f[2]) if pin else None)[0]
        pinned += bool(pin)
    assert (fma or pinned >= 1) and words > 1000 * len(todo) * len(outs)
    print(f"n={n} {'fused' if fma else 'bit-exact'} bank: {len(todo)} cases x {len(outs)} outputs, {words} output words compared, {pinned} cases pinned to the oracle's order")


def test_i16_chunked_call_equals_the_chunked_twin(sg, torch_gpu):
    """130 streams x enough ticks to pass 2^24 stream-ticks, on a fused derivative bank: the twin takes the same fp32 block pushes chunk by chunk"""
    streams = 130
    ticks = STAGED_MAX // streams + 100
    assert streams * ticks > STAGED_MAX and chunk_ticks(streams, ticks) == 129024 < ticks
    words, _ = run_case(sg, torch_gpu, streams, 16, (2, 1, 1e-3), 1, ("i16",), (("tick", 3), ("i16", ticks)), seed=77, twin_chunks=True, what="chunked")
    assert words == (ticks + 3 - 32) * streams


@pytest.mark.parametrize("fma", [0, 1])
def test_i16_saturation(sg, torch_gpu, fma):
    """a ramp of 80 counts per tick through a d = 1, dt = 1e-3 bank: 80 000 per time unit pins +32767, the falling ramp -32768; both routes"""
    torch = torch_gpu

    def mutate(x):
        T = x.shape[0]
        ramp = (80 * torch.arange(T, dtype=torch.int32)).to(torch.int16)
        assert 80 * (T - 1) <= 32767
        x[:, 10] = ramp
        x[:, 11] = -ramp
        x[:, 129] = ramp

    for streams, L in ((256, 97), (130, 63)):
        words, twin_rows = run_case(sg, torch, streams, 5, (2, 1, 1e-3), fma, BOTH, (("tick", 11), ("i16", L)), seed=5, mutate=mutate, saturating=True, what="saturation")
        want = to_i16(torch, twin_rows)
        assert bool((twin_rows[:, 10] > 70000).all()) and bool((twin_rows[:, 11] < -70000).all())
        assert bool((want[:, 10] == 32767).all()) and bool((want[:, 11] == -32768).all()) and bool((want[:, 129] == 32767).all())
        inside = (want > -32768) & (want < 32767)
        assert 2 * int(inside.sum()) >= want.numel()                        # the other streams are ordinary ones


@pytest.mark.parametrize("fma", [0, 1])
def test_i16_special_values_from_history(sg, torch_gpu, fma):
    """NaN and +-Inf in a few streams of the ring, put there by fp32 pushes before the int16 call: the first 2n rows of the call see them.  int16 output
    holds 0 where the twin holds NaN and the saturated values where it holds +-Inf; fp32 output holds NaN at the twin's positions.  Both routes."""
    torch = torch_gpu
    n, H = 5, 11

    def history(x32):
        x32[3, 5] = float("inf")
        x32[5, 6] = float("-inf")
        x32[H - 1, 7] = float("nan")                                           # the newest sample of the ring: in every window of the first 2n rows
        x32[H - 1, 8] = float("inf")
        x32[2, 129] = float("-inf")
        assert bool(torch.isfinite(x32[H:]).all())                             # the int16 call's own samples are ordinary

    for streams, L in ((256, 97), (130, 63)):
        for filt in ((2, 0, 1.0), (2, 1, 1e-3)):
            words, twin_rows = run_case(sg, torch, streams, n, filt, fma, BOTH, (("tick", H), ("i16", L)), seed=6, history=history, what="history")
            head = twin_rows[:2 * n]
            assert bool(torch.isnan(head[:, 7]).all()) and bool(torch.isfinite(head[:, [5, 6, 8, 129]]).logical_not().any(dim=0).all())
            want = to_i16(torch, head)
            assert bool((want[:, 7] == 0).all())
            inf = torch.isinf(head)
            assert bool((want[inf & (head > 0)] == 32767).all()) and bool((want[inf & (head < 0)] == -32768).all())
            if filt[1] == 0:
                assert bool((head == float("inf")).any()) and bool((head == float("-inf")).any())


def test_i16_refusals(sg, torch_gpu):
    """every refusal, in the header's order, returns -1 with its text before anything is enqueued: counters and save blob unchanged, d_out still all guard"""
    torch = torch_gpu
    S, n, T = 256, 8, 64
    bank = sg.StreamBank(S, n, 2, 0, 1.0)
    warm = torch.zeros((20, S), device="cuda")
    assert bank.push_block(warm, 20, torch.empty_like(warm)) == 4
    torch.cuda.synchronize()
    blob, counters = bank.save(), bank.counters
    buf = torch.full((4 * T, S), GUARD, dtype=torch.int16, device="cuda")
    src, dst = buf[:T], buf[2 * T:3 * T]
    L = sg.lib()
    I16, F16, BF16, F32 = sg.SAVGOL_HIP_I16, sg.SAVGOL_HIP_F16, sg.SAVGOL_HIP_BF16, sg.SAVGOL_HIP_F32
    name = "savgol_streambank_push_block_i16"
    far = buf.data_ptr() + (1 << 40)

    def refused(text, *args):
        assert L.savgol_streambank_push_block_i16(*args) == -1, text
        err = sg.last_error()
        assert name in err and text in err, (text, err)
        assert bank.counters == counters

    st = torch.cuda.current_stream().cuda_stream
    # 1. a NULL pointer (before the type)
    refused("NULL pointer", None, src.data_ptr(), T, dst.data_ptr(), I16, st)
    refused("NULL pointer", bank.ptr, None, T, dst.data_ptr(), I16, st)
    refused("NULL pointer", bank.ptr, src.data_ptr(), T, None, I16, st)
    refused("NULL pointer", bank.ptr, None, T, dst.data_ptr(), F16, st)
    # 2. the output type, named (before the tick service, the length and the overlap)
    for ot, text in ((F16, "output type f16 (1)"), (BF16, "output type bf16 (2)"), (7, "output type unknown (7)"), (-1, "output type unknown (-1)")):
        refused(text, bank.ptr, src.data_ptr(), T, dst.data_ptr(), ot, st)
    refused("output type f16 (1)", bank.ptr, src.data_ptr(), (1 << 30) + 1, src.data_ptr(), F16, st)
    # 4. no ticks: 0, whatever the buffers share;  5. more than 2^30 ticks (before the overlap)
    assert L.savgol_streambank_push_block_i16(bank.ptr, src.data_ptr(), 0, src.data_ptr(), I16, st) == 0 and bank.counters == counters
    assert bank.push_block_i16(src, 0, dst) == 0 and bank.counters == counters
    refused("2^30", bank.ptr, src.data_ptr(), (1 << 30) + 1, far, I16, st)
    refused("2^30", bank.ptr, src.data_ptr(), (1 << 30) + 1, src.data_ptr(), I16, st)
    # 6. shared bytes.  int16 -> int16: the same rows ... one shared element at either end
    row = S * 2
    for shift in (0, -row, row, T * row - 2, -(T * row - 2)):
        refused("overlap", bank.ptr, src.data_ptr() + T * row, T, src.data_ptr() + T * row + shift, I16, st)
    # int16 -> fp32: the output range is twice as long, compared byte-wise: its last two bytes on the samples' first two, and the samples' last two on its first
    refused("overlap", bank.ptr, buf.data_ptr() + 2 * T * row, T, buf.data_ptr() + 2, F32, st)
    refused("overlap", bank.ptr, buf.data_ptr(), T, buf.data_ptr() + T * row - 2, F32, st)
    # 3. the tick service running: before the length and the overlap, after the type
    bank.service_start()
    try:
        refused("tick service", bank.ptr, src.data_ptr(), T, dst.data_ptr(), I16, st)
        refused("tick service", bank.ptr, src.data_ptr(), (1 << 30) + 1, src.data_ptr(), I16, st)
        refused("tick service", bank.ptr, src.data_ptr(), 0, dst.data_ptr(), I16, st)
        refused("output type bf16 (2)", bank.ptr, src.data_ptr(), T, dst.data_ptr(), BF16, st)
    finally:
        bank.service_stop()
    torch.cuda.synchronize()
    assert bool((buf == GUARD).all()) and np.array_equal(bank.save(), blob)
    # touching end to start is served: fp32 outputs right behind the samples, int16 outputs right in front of them
    assert L.savgol_streambank_push_block_i16(bank.ptr, buf.data_ptr(), T, buf.data_ptr() + T * row, F32, st) == T, sg.last_error()
    assert L.savgol_streambank_push_block_i16(bank.ptr, buf.data_ptr() + 3 * T * row, T, buf.data_ptr() + 2 * T * row, I16, st) == T, sg.last_error()
    torch.cuda.synchronize()
    # the 16-bit float call keeps refusing int16
    assert L.savgol_streambank_push_block_h16(bank.ptr, src.data_ptr(), I16, T, dst.data_ptr(), I16, st) == -1
    assert "savgol_streambank_push_block_h16" in sg.last_error() and "unknown -> unknown" in sg.last_error()
    bank.close()


def test_i16_refuses_a_bank_on_another_device(sg, torch_gpu):
    torch = torch_gpu
    if torch.cuda.device_count() < 2:
        pytest.skip("one GPU")
    bank = sg.StreamBank(256, 8, 2, 0, 1.0)
    buf = torch.full((128, 256), GUARD, dtype=torch.int16, device="cuda:0")
    try:
        assert sg.lib().savgol_hip_set_device(1) == 0
        assert bank.push_block_i16(buf[:64], 64, buf[64:]) == -1
        assert "savgol_streambank_push_block_i16" in sg.last_error() and "lives on device 0" in sg.last_error()
    finally:
        sg.lib().savgol_hip_set_device(0)
    assert bank.counters == (0, 0)
    bank.close()


@pytest.mark.parametrize("fma,out", [(1, "i16"), (0, "f32")])
def test_i16_tile_route_in_a_graph(sg, torch_gpu, fma, out):
    """after one warm-up call a tile-route call (head, body, tail store, one scratch allocation) is captured and replays to the twin's bits on a reset bank"""
    torch = torch_gpu
    S, n, T = 256, 16, 167
    filt = (2, 1, 1e-3)
    case = seams.Case("graph", S, 0, 0, n, *filt, fma, 0.0, ())
    xq = torch.from_numpy(quantise(case, T, 9, amplitude(n, filt)))
    twin = sg.StreamBank(S, n, *filt, fma=bool(fma))
    ref = torch.full((T, S), GUARD, device="cuda")
    assert twin.push_block(xq.float().cuda(), T, ref) == T - 2 * n
    torch.cuda.synchronize()
    blob = twin.save()
    ref = ref.cpu()
    ref[2 * n:] = ref[2 * n:] if out == "f32" else to_i16(torch, ref[2 * n:]).float()
    want = ref.to(tdtype(torch, out)).cuda()                                 # rows without an output: the guard, exact in both types
    x = xq.cuda()
    bank = sg.StreamBank(S, n, *filt, fma=bool(fma))
    warm = torch.full((T, S), GUARD, dtype=tdtype(torch, out), device="cuda")
    assert bank.push_block_i16(x, T, warm, out) == T - 2 * n
    torch.cuda.synchronize()
    assert torch.equal(as_int(torch, warm), as_int(torch, want))
    res = torch.full_like(want, GUARD)
    bank.reset()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(s):
        with torch.cuda.graph(g, stream=s):
            assert bank.push_block_i16(x, T, res, out, stream=s) == T - 2 * n, sg.last_error()
    res.fill_(GUARD)
    torch.cuda.synchronize()
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(as_int(torch, res), as_int(torch, want))
    assert np.array_equal(bank.save(), blob)
    bank.close()
    twin.close()
