"""GPU tests of the int16-storage 1-D batch call (savgol_apply[_valid]_batch_i16, sg_k1d_st16.hpp).  The contract: the output equals, bit for bit, the
EXISTING fp32 call on the widened input under SAVGOL_BATCH_TILE_NARROW; for int16 output that result rounded to nearest even, saturated to
[-32768, 32767], NaN -> 0 (torch.round / nan_to_num / clamp / cast on the CPU) -- every half window, boundary mode, VALID, derivative, both output
types and every served flag; ragged lengths, odd pitches and shifted bases with guarded sentinel-filled outputs; +-Inf / NaN results; derivative
filters on a large offset; the fp64 oracle; refused calls launch nothing; one full-size run; graph capture.  Expected values never come from the code
under test."""
import numpy as np
import pytest

from tests._util import check, fp32_bar, normwise

pytestmark = pytest.mark.gpu

MODES = (0, 1, 2, 3)
OUTS = ("i16", "f32")
SENTINEL = 0x5A5B                                                    # what int16 outputs are pre-filled with (23131)


@pytest.fixture(scope="module")
def torch_gpu(sg):
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    assert sg.device_count() > 0, sg.last_error()
    return torch


def tdtype(torch, name):
    return {"i16": torch.int16, "f32": torch.float32}[name]


def filter_sets(n):
    """those of tests/test_gpu_1d_h16.py: d = 0 / 1 / 2 with mixed poly_order and time_step; (4, 0) and (4, 1) take the block moments from n = 20"""
    m4 = min(4, 2 * n)
    return [(m4, 0, 1.0), (m4, 1, 1.0), (m4, 2, 0.25), (2, 0, 1.0), (min(3, 2 * n), 1, 0.5)]


def full_scale(rng, shape):
    """full-scale random int16 with both ends of the range, and plateaus at either end longer than any window with steps between them: a smoothing
    filter returns the plateau's value inside it and overshoots next to the step, so the int16 output reaches both ends and saturates"""
    x = rng.integers(-32768, 32768, shape).astype(np.int16)
    x[:, 0], x[:, 1] = -32768, 32767
    for start in (100, 2048 - 150, 4500):
        x[:, start:start + 100] = 32767
        x[:, start + 100:start + 200] = -32768
        x[:, start + 200:start + 300] = 32767
    return x


def small_signal(rng, shape):
    t = np.arange(shape[-1], dtype=np.float64)
    return np.clip(np.rint(150.0 * np.sin(0.013 * t) + 30.0 * np.sin(0.41 * t + 1.0) + rng.normal(0, 10.0, shape)), -200, 200).astype(np.int16)


def oracle_signal(rng, shape):
    t = np.arange(shape[-1], dtype=np.float64)
    return np.rint(12000.0 * np.sin(0.013 * t) + 1800.0 * np.sin(0.41 * t + 1.0) + rng.normal(0, 1200.0, shape)).astype(np.int16)


def sentinel(torch, dtype, count):
    if dtype == torch.float32:
        return torch.full((count,), float("nan"), dtype=dtype, device="cuda")
    return torch.full((count,), SENTINEL, dtype=dtype, device="cuda")


def untouched(torch, t):
    return bool(torch.isnan(t).all()) if t.dtype == torch.float32 else bool((t == SENTINEL).all())


def alloc(torch, dtype, rows, ld, shift=0):
    """(base, view): a [rows, ld] device view starting `shift` elements into its sentinel-filled storage, 8 guard elements behind it"""
    base = sentinel(torch, dtype, rows * ld + shift + 8)
    return base, base[shift:shift + rows * ld].view(rows, ld)


def as_int(torch, t):
    return t.contiguous().view(torch.int16 if t.element_size() == 2 else torch.int32)


def twin(sg, torch, f, x16, valid, flags):
    """the contract's right-hand side: the existing fp32 call on the widened input (narrow tile); host fp32 tensor"""
    ch, length = x16.shape
    xw = x16.float().contiguous()
    out_len = length - 2 * f.n if valid else length
    ref = torch.full((ch, out_len), float("nan"), dtype=torch.float32, device="cuda")
    f.apply_batch(xw, ref, ch, length, length, out_len, valid=valid, flags=flags | sg.SAVGOL_BATCH_TILE_NARROW)
    torch.cuda.synchronize()
    return ref.cpu()


def to_out(torch, want32, out_name):
    """fp32 -> the output type on the CPU: round to nearest even, NaN -> 0, saturate (+-Inf included), cast"""
    if out_name == "f32":
        return want32
    return torch.clamp(torch.nan_to_num(torch.round(want32), nan=0.0), -32768.0, 32767.0).to(torch.int16)


def same(torch, got, want, label):
    """bit for bit where the expected value is not NaN; the NaN masks coincide (payloads are free)"""
    got = got.cpu()
    if want.dtype == torch.float32:
        gn, wn = torch.isnan(got), torch.isnan(want)
        assert torch.equal(gn, wn), (label, "NaN masks differ", int((gn != wn).sum()))
        diff = (as_int(torch, got) != as_int(torch, want)) & ~wn
    else:
        diff = got != want
    assert not bool(diff.any()), (label, int(diff.sum()), "values differ")


def run_case(sg, torch, f, xh, out_name, valid=False, flags=0, in_shift=0, out_shift=0, in_pad=0, out_pad=0, want32=None):
    """xh: host int16 tensor [channels, length].  Runs the int16 call on the given layout, checks the contract, the pitch padding and the guards;
    returns (device output [channels, out_len], expected host tensor)."""
    ch, length = xh.shape
    out_len = length - 2 * f.n if valid else length
    in_ld, out_ld = length + in_pad, out_len + out_pad
    _, x = alloc(torch, torch.int16, ch, in_ld, in_shift)
    x[:, :length] = xh.cuda()
    obase, out = alloc(torch, tdtype(torch, out_name), ch, out_ld, out_shift)
    f.apply_batch_i16(x, out, ch, length, in_ld, out_ld, out_dtype=out_name, valid=valid, flags=flags)
    torch.cuda.synchronize()
    if want32 is None:
        want32 = twin(sg, torch, f, x[:, :length], valid, flags)
    want = to_out(torch, want32, out_name)
    label = (f.n, out_name, valid, flags, (in_shift, out_shift, in_pad, out_pad), length)
    same(torch, out[:, :out_len], want, label)
    # nothing outside the rows: the pitch padding, the elements before the base and the guards behind the last row keep their sentinel
    if out_pad:
        assert untouched(torch, out[:, out_len:]), (label, "pitch padding written")
    assert untouched(torch, obase[:out_shift]) and untouched(torch, obase[out_shift + ch * out_ld:]), (label, "guard written")
    return out[:, :out_len], want


# ------------------------------------------------------------------------------------------------
# 1. the contract: N = 1..32, every boundary mode, full and VALID, d = 0 / 1 / 2, both output types, with and without PLAIN_SUMMATION / CORRECT_LEADING_EDGE
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", range(1, 33))
def test_i16_bit_identical_to_the_fp32_call(sg, torch_gpu, n):
    torch = torch_gpu
    rng = np.random.default_rng(3600 + n)
    flag_sets = (0, sg.SAVGOL_BATCH_PLAIN_SUMMATION, sg.SAVGOL_BATCH_CORRECT_LEADING_EDGE,
                 sg.SAVGOL_BATCH_PLAIN_SUMMATION | sg.SAVGOL_BATCH_CORRECT_LEADING_EDGE | sg.SAVGOL_BATCH_TILE_NARROW)
    overshoot = False
    # 3 x 9004: five narrow tiles, channel ends and full interior tiles
    for what, xh in (("full scale", torch.from_numpy(full_scale(rng, (3, 9004)))), ("+-200 counts", torch.from_numpy(small_signal(rng, (3, 9004))))):
        xd = xh.cuda()
        for (m, d, dt) in filter_sets(n):
            for mode, valid in [(mo, False) for mo in MODES] + [(0, True)]:
                f = sg.Filter(n, m, d, dt, mode)
                for flags in flag_sets if what == "full scale" else (0,):
                    if flags & sg.SAVGOL_BATCH_CORRECT_LEADING_EDGE and (mode != 0 or valid or not d & 1):
                        continue                                    # the flag only acts on the POLYNOMIAL leading edge of odd derivatives
                    want32 = twin(sg, torch, f, xd, valid, flags)
                    for out_name in OUTS:
                        run_case(sg, torch, f, xh, out_name, valid=valid, flags=flags, want32=want32)
                    if what == "full scale" and d == 0:
                        # both ends of the int16 range are reached (the plateaus), and from n = 2 the twin leaves it (the overshoot at the steps)
                        want16 = to_out(torch, want32, "i16")
                        assert int(want16.min()) == -32768 and int(want16.max()) == 32767, (n, m, mode, valid, flags)
                        overshoot = overshoot or bool((want32 > 32767.5).any() and (want32 < -32768.5).any())
    assert overshoot or n == 1, "no smoothing case saturated"


def test_i16_correct_leading_edge_acts(sg, torch_gpu):
    """the flag reaches the edge items: the leading n outputs of an odd derivative change sign, nothing else changes"""
    torch = torch_gpu
    xh = torch.from_numpy(small_signal(np.random.default_rng(3650), (2, 5000)))
    for n in (3, 24):
        f = sg.Filter(n, 3, 1, 1.0, 0)
        a, _ = run_case(sg, torch, f, xh, "f32")
        b, _ = run_case(sg, torch, f, xh, "f32", flags=sg.SAVGOL_BATCH_CORRECT_LEADING_EDGE)
        assert torch.equal(b[:, :n], -a[:, :n]) and torch.equal(as_int(torch, b[:, n:]), as_int(torch, a[:, n:])) and bool((a[:, :n] != 0).any())


# ------------------------------------------------------------------------------------------------
# 2. layout: ragged lengths, pitches, shifted bases (the element-wise paths), guarded sentinel-filled outputs, more than 65 536 channels
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [2, 7, 24, 32])
def test_i16_ragged_lengths_pitches_and_shifted_bases(sg, torch_gpu, n):
    torch = torch_gpu
    rng = np.random.default_rng(3800 + n)
    na = (n + 3) // 4 * 4
    lengths = [2048, 2047, 2049, 2 * 2048 + na - 1, 2 * 2048 + 1, 2 * n + 1]     # one tile, tile -+ 1, a last tile shorter than NA, the minimum
    layouts = [(0, 0, 0, 0), (1, 2, 3, 1), (2, 3, 0, 5), (3, 1, 1, 0), (5, 5, 4, 4), (0, 0, 4, 8), (4, 4, 0, 0)]     # in_shift, out_shift, in_pad, out_pad
    case = 0
    for length in lengths:
        xh = torch.from_numpy(full_scale(rng, (3, max(length, 5000)))[:, :length].copy())
        for layout in layouts:
            for out_name in OUTS:
                mode, valid = MODES[case % 4], case % 3 == 2
                d = (0, 1, 2)[case % 3]
                case += 1
                f = sg.Filter(n, 4, d, 1.0 if d == 0 else 0.5, mode)
                run_case(sg, torch, f, xh, out_name, valid=valid, in_shift=layout[0], out_shift=layout[1], in_pad=layout[2], out_pad=layout[3])


def test_i16_many_short_channels(sg, torch_gpu):
    torch = torch_gpu
    rng = np.random.default_rng(3900)
    xh = torch.from_numpy(rng.integers(-32768, 32768, (70000, 100)).astype(np.int16))
    for out_name, n, mode in (("i16", 5, 0), ("f32", 21, 1), ("i16", 5, 2)):
        run_case(sg, torch, sg.Filter(n, 3, 1, 1.0, mode), xh, out_name, out_pad=1)


# ------------------------------------------------------------------------------------------------
# 3. non-finite results: a first derivative whose 1 / time_step overflows fp32.  Ramps give +-Inf, constant rows 0 x Inf = NaN
# ------------------------------------------------------------------------------------------------
def test_i16_inf_and_nan_results_saturate_and_zero(sg, torch_gpu):
    torch = torch_gpu
    length = 5000
    t = np.arange(length)
    xh = torch.from_numpy(np.stack([t % 3000, -(t % 3000), np.full(length, 1234), np.zeros(length, np.int64), 3 * (t % 1000) - 1500]).astype(np.int16))
    for n, m in ((4, 2), (24, 3)):
        for mode, valid in ((0, False), (1, False), (0, True)):
            f = sg.Filter(n, m, 1, 1e-39, mode)                      # dt_scale is subnormal: its reciprocal is +Inf
            want32 = twin(sg, torch, f, xh.cuda(), valid, 0)
            pinf, ninf, nan = want32 == float("inf"), want32 == float("-inf"), torch.isnan(want32)
            assert bool(pinf.any()) and bool(ninf.any()) and bool(nan.any()), (n, mode, valid, int(pinf.sum()), int(ninf.sum()), int(nan.sum()))
            assert bool((pinf | ninf | nan).all())
            out32, _ = run_case(sg, torch, f, xh, "f32", valid=valid, want32=want32)
            out16, _ = run_case(sg, torch, f, xh, "i16", valid=valid, want32=want32)
            out16 = out16.cpu()
            assert bool((out16[pinf] == 32767).all()) and bool((out16[ninf] == -32768).all()) and bool((out16[nan] == 0).all())


# ------------------------------------------------------------------------------------------------
# 4. the JOB_CENTRE route: derivative filters on rows whose offset is 100 x their variation
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [5, 24])
def test_i16_centred_derivatives_on_an_offset_signal(sg, torch_gpu, n):
    torch = torch_gpu
    rng = np.random.default_rng(3700 + n)
    t = np.arange(9004, dtype=np.float64)
    xh = torch.from_numpy(np.rint(30000.0 + 250.0 * np.sin(0.013 * t) + 30.0 * np.sin(0.41 * t + 1.0) + rng.uniform(-20, 20, (3, 9004))).astype(np.int16))
    assert int(xh.min()) >= 29700 and int(xh.max()) <= 30300
    for out_name in OUTS:
        for d in (1, 2):
            for mode in MODES:
                run_case(sg, torch, sg.Filter(n, 4, d, 0.5, mode), xh, out_name)
            run_case(sg, torch, sg.Filter(n, 4, d, 0.5, 0), xh, out_name, valid=True)


# ------------------------------------------------------------------------------------------------
# 5. against the fp64 oracle of the widened input.  fp32 output: the project's fp32 rule.  int16 output (smoothing filters): one rounding to an
#    integer (0.5) on top of the fp32 result's own normwise error
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 2, 5, 8, 12, 16, 19, 24, 32])
def test_i16_against_fp64_oracle(sg, sgo, torch_gpu, n):
    torch = torch_gpu
    rng = np.random.default_rng(4200 + n)
    x16 = torch.from_numpy(oracle_signal(rng, (2, 12011)))
    xw = x16.float().numpy()                                        # the widened input, exactly
    xd = x16.cuda()
    for (m, d, dt) in filter_sets(n):
        for mode, valid in [(mo, False) for mo in MODES] + [(0, True)]:
            o = sgo.Filter(n, m, d, dt, mode)
            ref = o.apply_f64(xw.astype(np.float64))
            r32 = o.apply(xw)
            if valid:
                ref, r32 = ref[:, n:-n], r32[:, n:-n]
            bar32 = fp32_bar(normwise(r32, ref))
            f = sg.Filter(n, m, d, dt, mode)
            y = f.apply_tensor_i16(xd, valid=valid, out_dtype=torch.float32)
            check(normwise(y.cpu().numpy(), ref), bar32, (n, m, d, dt, mode, valid, "f32"))
            if d == 0:
                top = float(np.max(np.abs(ref)))
                assert top < 32767.0, (n, m, mode, top)             # nothing saturates: every element is compared
                y16 = f.apply_tensor_i16(xd, valid=valid).cpu().numpy().astype(np.float64)
                assert y16.shape == ref.shape
                check(float(np.max(np.abs(y16 - ref))), 0.5 + bar32 * top, (n, m, d, dt, mode, valid, "i16"))


# ------------------------------------------------------------------------------------------------
# 6. refusals on the device: no launch, the outputs keep their sentinel
# ------------------------------------------------------------------------------------------------
def test_i16_refusals_launch_nothing(sg, torch_gpu):
    torch = torch_gpu
    ch, length = 4, 5000
    x = torch.from_numpy(small_signal(np.random.default_rng(4300), (ch, length))).cuda()
    out = sentinel(torch, torch.int16, ch * length).view(ch, length)
    out32 = sentinel(torch, torch.float32, ch * length).view(ch, length)
    f = sg.Filter(8, 3, 1)
    bad = [
        (dict(flags=sg.SAVGOL_BATCH_REFERENCE_SUMMATION), out, "REFERENCE_SUMMATION"),
        (dict(flags=sg.SAVGOL_BATCH_TILE_WIDE), out, "TILE_WIDE"),
        (dict(flags=sg.SAVGOL_BATCH_MOMENT_F64), out, "belong to other calls"),
        (dict(flags=sg.SAVGOL_BATCH_BOUNDARY_AWARE), out, "belong to other calls"),
        (dict(flags=0x1000), out, "bad flags 0x1000"),
        (dict(in_ld=length - 1), out, "row pitch smaller than the row"),
        (dict(out_dtype="f32", out_ld=length - 17), out32, "row pitch smaller than the row"),
    ]
    for kw, o, text in bad:
        for valid in (False, True):
            with pytest.raises(RuntimeError, match=text):
                f.apply_batch_i16(x, o, ch, length, valid=valid, **kw)
    lib = sg.lib()
    for ot in (sg.SAVGOL_HIP_F16, sg.SAVGOL_HIP_BF16, 7):
        assert lib.savgol_apply_batch_i16(f.ptr, x.data_ptr(), out.data_ptr(), ot, ch, length, length, length, 0, None) == -1
        assert "is not served" in sg.last_error() and "savgol_apply_batch_i16" in sg.last_error()
    assert lib.savgol_apply_batch_i16(f.ptr, x.data_ptr(), out.data_ptr(), sg.SAVGOL_HIP_I16, ch, 10, 10, 10, 0, None) == -1
    assert "data length (10) < window size (17)" in sg.last_error()
    torch.cuda.synchronize()
    assert untouched(torch, out) and untouched(torch, out32)
    # in place and shifted overlaps: the input is untouched
    before = x.clone()
    flat = x.view(-1)
    for target in (x, flat[1:], flat[length - 3:]):
        with pytest.raises(RuntimeError, match="d_in and d_out overlap"):
            f.apply_batch_i16(x, target, ch - 1, length)
    torch.cuda.synchronize()
    assert torch.equal(x, before)


# ------------------------------------------------------------------------------------------------
# 7. full size: 4096 x 2^20, n = 32, m = 4, int16 -> int16
# ------------------------------------------------------------------------------------------------
def test_i16_full_size(sg, torch_gpu):
    torch = torch_gpu
    channels, length = 4096, 1 << 20
    free, _ = torch.cuda.mem_get_info()
    assert free > 3 * 2 * channels * length, "the headline shape needs 24 GiB of free device memory"
    x = torch.empty((channels, length), dtype=torch.int16, device="cuda")
    t = torch.arange(length, dtype=torch.float32, device="cuda")
    g = torch.Generator(device="cuda").manual_seed(4600)
    part = 256
    for r0 in range(0, channels, part):
        phase = torch.arange(r0, r0 + part, dtype=torch.float32, device="cuda")[:, None]
        noise = torch.randint(-1500, 1501, (part, length), dtype=torch.int16, device="cuda", generator=g)
        x[r0:r0 + part] = (torch.round(20000.0 * torch.sin(0.003 * t[None, :] + phase)) + noise).to(torch.int16)
        del noise
    f = sg.Filter(32, 4, 0, 1.0, 0)
    y = f.apply_tensor_i16(x)
    torch.cuda.synchronize()
    # a fixed sample of rows (the first and last, the rows either side of every 1024, some in between) against the twin, every column
    rows = torch.tensor([0, 1, 511, 1023, 1024, 1777, 2047, 2048, 3071, 3072, 4000, 4094, 4095], device="cuda")
    want = to_out(torch, twin(sg, torch, f, x[rows], False, 0), "i16")
    same(torch, y[rows], want, "headline rows")
    assert int(want.max()) > 15000 and int(want.min()) < -15000
    del x, y
    torch.cuda.empty_cache()


# ------------------------------------------------------------------------------------------------
# 8. graph capture
# ------------------------------------------------------------------------------------------------
def test_i16_graph_capture(sg, torch_gpu):
    """after one warm-up call with the same filter the call only enqueues: it captures into a graph and replays (twice) to the eager call's bits"""
    torch = torch_gpu
    rng = np.random.default_rng(4700)
    for out_name, n in (("i16", 12), ("f32", 24)):
        xh = torch.from_numpy(oracle_signal(rng, (8, 40000)))
        x = xh.cuda()
        f = sg.Filter(n, 4, 1, 1.0, 0)
        eager = f.apply_tensor_i16(x, out_dtype=tdtype(torch, out_name))          # the warm-up
        torch.cuda.synchronize()
        out = sentinel(torch, tdtype(torch, out_name), 8 * 40000).view(8, 40000)
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        g = torch.cuda.CUDAGraph()
        with torch.cuda.stream(s):
            with torch.cuda.graph(g, stream=s):
                f.apply_batch_i16(x, out, 8, 40000, out_dtype=out_name, stream=s)
        for _ in range(2):
            out.copy_(sentinel(torch, tdtype(torch, out_name), 8 * 40000).view(8, 40000))
            g.replay()
            torch.cuda.synchronize()
            assert torch.equal(as_int(torch, out), as_int(torch, eager))
        same(torch, out, to_out(torch, twin(sg, torch, f, x, False, 0), out_name), ("graph", out_name))
