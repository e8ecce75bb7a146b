"""GPU tests of the 16-bit-storage 1-D batch call (savgol_apply[_valid]_batch_h16, sg_k1d_st16.hpp).  The contract: the output equals, bit for bit, the
EXISTING fp32 call on the widened input under SAVGOL_BATCH_TILE_NARROW, rounded to nearest even into the output type (torch's CPU cast) -- every half
window, boundary mode, VALID, derivative, type pair and served flag; ragged lengths, odd pitches and shifted bases with guarded NaN-filled outputs;
Inf / NaN / subnormal / overflowing values; the fp64 oracle within u + (1 + u) x the fp32 bar; refused calls launch nothing; one full-size run; graph
capture.  Expected values never come from the code under test."""
import numpy as np
import pytest

from tests._util import check, fp32_bar, normwise

pytestmark = pytest.mark.gpu

MODES = (0, 1, 2, 3)
PAIRS = (("f16", "f16"), ("bf16", "bf16"), ("f16", "f32"), ("bf16", "f32"))
UNIT = {"f16": 2.0 ** -11, "bf16": 2.0 ** -8, "f32": 0.0}            # unit roundoff of the output type


@pytest.fixture(scope="module")
def torch_gpu(sg):
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    assert sg.device_count() > 0, sg.last_error()
    return torch


def tdtype(torch, name):
    return {"f16": torch.float16, "bf16": torch.bfloat16, "f32": torch.float32}[name]


def signal(rng, shape, offset=0.0, amp=2.0):
    t = np.arange(shape[-1], dtype=np.float64)
    return (offset + np.sin(0.013 * t) * amp + 0.15 * amp * np.sin(0.41 * t + 1.0) + rng.normal(0, 0.1 * amp, shape)).astype(np.float32)


def filter_sets(n):
    """d = 0 / 1 / 2 with mixed poly_order and time_step (poly_order capped below the window); (4, 0) and (4, 1) take the block moments from n = 20"""
    m4 = min(4, 2 * n)
    return [(m4, 0, 1.0), (m4, 1, 1.0), (m4, 2, 0.25), (2, 0, 1.0), (min(3, 2 * n), 1, 0.5)]


def alloc(torch, dtype, rows, ld, shift=0):
    """(base, view): a [rows, ld] device view starting `shift` elements into its NaN-filled storage, 8 guard elements behind it"""
    base = torch.full((rows * ld + shift + 8,), float("nan"), dtype=dtype, device="cuda")
    return base, base[shift:shift + rows * ld].view(rows, ld)


def as_int(torch, t):
    return t.contiguous().view(torch.int16 if t.element_size() == 2 else torch.int32)


def expected(sg, torch, f, x16, out_name, valid, flags):
    """the contract's right-hand side: the existing fp32 call on the widened input (narrow tile), cast on the CPU (round to nearest even)"""
    ch, length = x16.shape
    xw = x16.float().contiguous()
    out_len = length - 2 * f.n if valid else length
    ref = torch.full((ch, out_len), float("nan"), dtype=torch.float32, device="cuda")
    f.apply_batch(xw, ref, ch, length, length, out_len, valid=valid, flags=flags | sg.SAVGOL_BATCH_TILE_NARROW)
    torch.cuda.synchronize()
    return ref.cpu().to(tdtype(torch, out_name))


def same_after_rounding(torch, got, want, label):
    """bit for bit where the expected value is not NaN; the NaN masks coincide (payloads are free)"""
    got = got.cpu()
    gn, wn = torch.isnan(got), torch.isnan(want)
    assert torch.equal(gn, wn), (label, "NaN masks differ", int((gn != wn).sum()))
    a, b = as_int(torch, got), as_int(torch, want)
    diff = (a != b) & ~wn
    assert not bool(diff.any()), (label, int(diff.sum()), "values differ")


def run_case(sg, torch, f, xh16, pair, valid=False, flags=0, in_shift=0, out_shift=0, in_pad=0, out_pad=0, want=None):
    """xh16: host tensor [channels, length] of the input type.  Runs the 16-bit call on the given layout, checks the contract, the pitch padding and
    the guards; returns (device output [channels, out_len], expected host tensor)."""
    in_name, out_name = pair
    ch, length = xh16.shape
    out_len = length - 2 * f.n if valid else length
    in_ld, out_ld = length + in_pad, out_len + out_pad
    _, x = alloc(torch, xh16.dtype, ch, in_ld, in_shift)
    x[:, :length] = xh16.cuda()
    obase, out = alloc(torch, tdtype(torch, out_name), ch, out_ld, out_shift)
    f.apply_batch(x, out, ch, length, in_ld, out_ld, dtype=in_name, out_dtype=out_name, valid=valid, flags=flags)
    torch.cuda.synchronize()
    if want is None:
        want = expected(sg, torch, f, x[:, :length], out_name, valid, flags)
    label = (f.n, pair, valid, flags, (in_shift, out_shift, in_pad, out_pad), length)
    same_after_rounding(torch, out[:, :out_len], want, label)
    # nothing outside the rows: the pitch padding, the elements before the base and the guards behind the last row are still NaN
    if out_pad:
        assert bool(torch.isnan(out[:, out_len:]).all()), (label, "pitch padding written")
    assert bool(torch.isnan(obase[:out_shift]).all()) and bool(torch.isnan(obase[out_shift + ch * out_ld:]).all()), (label, "guard written")
    return out[:, :out_len], want


def host16(torch, xh, in_name):
    return torch.from_numpy(np.ascontiguousarray(xh)).to(tdtype(torch, in_name))


# ------------------------------------------------------------------------------------------------
# 1. the contract: N = 1..32, every boundary mode, full and VALID, d = 0 / 1 / 2, four type pairs, with and without PLAIN_SUMMATION / CORRECT_LEADING_EDGE
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", range(1, 33))
def test_h16_bit_identical_to_rounded_fp32_call(sg, torch_gpu, n):
    torch = torch_gpu
    rng = np.random.default_rng(1600 + n)
    xh = signal(rng, (3, 9004))                                     # five narrow tiles: channel ends and full interior tiles
    flag_sets = (0, sg.SAVGOL_BATCH_PLAIN_SUMMATION, sg.SAVGOL_BATCH_CORRECT_LEADING_EDGE,
                 sg.SAVGOL_BATCH_PLAIN_SUMMATION | sg.SAVGOL_BATCH_CORRECT_LEADING_EDGE | sg.SAVGOL_BATCH_TILE_NARROW)
    for in_name in ("f16", "bf16"):
        x16 = host16(torch, xh, in_name)
        xd = x16.cuda()
        for (m, d, dt) in filter_sets(n):
            for mode, valid in [(mo, False) for mo in MODES] + [(0, True)]:
                f = sg.Filter(n, m, d, dt, mode)
                for flags in flag_sets:
                    if flags & sg.SAVGOL_BATCH_CORRECT_LEADING_EDGE and (mode != 0 or valid or not d & 1):
                        continue                                    # the flag only acts on the POLYNOMIAL leading edge of odd derivatives
                    want32 = expected(sg, torch, f, xd, "f32", valid, flags)
                    for pair in PAIRS:
                        if pair[0] == in_name:
                            run_case(sg, torch, f, x16, pair, valid=valid, flags=flags, want=want32.to(tdtype(torch, pair[1])))


def test_h16_correct_leading_edge_acts(sg, torch_gpu):
    """the flag reaches the edge items: the leading n outputs of an odd derivative change sign, nothing else changes"""
    torch = torch_gpu
    xh = signal(np.random.default_rng(1650), (2, 5000))
    for n in (3, 24):
        f = sg.Filter(n, 3, 1, 1.0, 0)
        for pair in PAIRS:
            x16 = host16(torch, xh, pair[0])
            a, _ = run_case(sg, torch, f, x16, pair)
            b, _ = run_case(sg, torch, f, x16, pair, flags=sg.SAVGOL_BATCH_CORRECT_LEADING_EDGE)
            assert torch.equal(b[:, :n].float(), -a[:, :n].float()) and torch.equal(as_int(torch, b[:, n:]), as_int(torch, a[:, n:]))


@pytest.mark.parametrize("n", [3, 8, 20, 32])
def test_h16_centred_derivatives_on_an_offset_signal(sg, torch_gpu, n):
    """the JOB_CENTRE route: a signal whose offset is 100 x its variation"""
    torch = torch_gpu
    rng = np.random.default_rng(1700 + n)
    xh = signal(rng, (3, 9004), offset=200.0, amp=2.0)
    for pair in PAIRS:
        x16 = host16(torch, xh, pair[0])
        for d in (1, 2):
            for mode in MODES:
                run_case(sg, torch, sg.Filter(n, 4, d, 0.5, mode), x16, pair)
            run_case(sg, torch, sg.Filter(n, 4, d, 0.5, 0), x16, pair, valid=True)


# ------------------------------------------------------------------------------------------------
# 2. layout: ragged lengths, pitches, shifted bases (the scalar paths), guarded NaN-filled outputs, more than 65 536 channels
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [2, 7, 24, 32])
def test_h16_ragged_lengths_pitches_and_shifted_bases(sg, torch_gpu, n):
    torch = torch_gpu
    rng = np.random.default_rng(1800 + n)
    na = (n + 3) // 4 * 4
    lengths = [2048, 2047, 2049, 2 * 2048 + max(na - 1, 1), 2 * 2048 + 1, 2 * n + 1]     # one tile, tile -+ 1, a last tile shorter than NA, the minimum
    layouts = [(0, 0, 0, 0), (1, 2, 3, 1), (2, 3, 0, 5), (3, 1, 1, 0), (5, 5, 4, 4), (0, 0, 4, 8), (4, 4, 0, 0)]     # in_shift, out_shift, in_pad, out_pad
    case = 0
    for length in lengths:
        xh = signal(rng, (3, length))
        for layout in layouts:
            for pair in PAIRS:
                mode, valid = MODES[case % 4], case % 3 == 2
                d = (0, 1, 2)[case % 3] if n > 1 else 0
                case += 1
                f = sg.Filter(n, 4, d, 1.0 if d == 0 else 0.5, mode)
                run_case(sg, torch, f, host16(torch, xh, pair[0]), pair, valid=valid, in_shift=layout[0], out_shift=layout[1], in_pad=layout[2], out_pad=layout[3])


def test_h16_many_short_channels(sg, torch_gpu):
    torch = torch_gpu
    rng = np.random.default_rng(1900)
    xh = signal(rng, (70000, 100))
    for pair, n, mode in ((("bf16", "bf16"), 5, 0), (("f16", "f32"), 21, 1), (("f16", "f16"), 5, 2)):
        run_case(sg, torch, sg.Filter(n, 3, 1, 1.0, mode), host16(torch, xh, pair[0]), pair, out_pad=1)


# ------------------------------------------------------------------------------------------------
# 3. special values
# ------------------------------------------------------------------------------------------------
def test_h16_inf_and_nan_samples(sg, torch_gpu):
    """the NaN / Inf footprint of the fp32 call on the widened input"""
    torch = torch_gpu
    rng = np.random.default_rng(2000)
    xh = signal(rng, (4, 9004))
    for at, v in ((3, np.inf), (700, -np.inf), (2047, np.nan), (2048, np.inf), (4100, np.nan), (9003, -np.inf), (6000, np.inf), (6001, -np.inf)):
        xh[at % 4, at] = v
    for n, m, d in ((4, 2, 0), (12, 4, 1), (24, 4, 0), (32, 4, 2)):
        for mode in MODES:
            for pair in PAIRS:
                out, want = run_case(sg, torch, sg.Filter(n, m, d, 1.0, mode), host16(torch, xh, pair[0]), pair)
                assert bool(torch.isnan(want).any()) and bool(torch.isinf(want).any())
                assert torch.equal(torch.isinf(out.cpu()), torch.isinf(want))


def test_h16_fp16_subnormal_inputs_widen_exactly(sg, torch_gpu):
    torch = torch_gpu
    rng = np.random.default_rng(2100)
    bits = rng.integers(1, 1024, (3, 6000)).astype(np.int16) | (rng.integers(0, 2, (3, 6000)).astype(np.int16) << 15)      # every fp16 subnormal, both signs
    x16 = torch.from_numpy(bits).view(torch.float16)
    assert float(x16.float().abs().max()) < 2.0 ** -14
    for n, m in ((1, 0), (6, 2), (24, 4)):
        out, want = run_case(sg, torch, sg.Filter(n, m, 0, 1.0, 1), x16, ("f16", "f32"))
        assert float(want.abs().max()) > 0.0 and torch.equal(as_int(torch, out.cpu()), as_int(torch, want))
        run_case(sg, torch, sg.Filter(n, m, 0, 1.0, 1), x16, ("f16", "f16"))


def test_h16_overflow_to_fp16_gives_inf(sg, torch_gpu):
    """results beyond 65504: +-Inf in fp16 output (IEEE rounding), finite in bf16 and fp32 output"""
    torch = torch_gpu
    t = np.arange(9004, dtype=np.float64)
    xh = np.stack([4000.0 * np.sin(0.05 * t), 4000.0 * np.cos(0.05 * t)]).astype(np.float32)
    for n in (5, 24):
        f = sg.Filter(n, 3, 1, 1e-3, 1)                            # d/dt with time_step 1e-3: amplitude 2e5
        out, want = run_case(sg, torch, f, host16(torch, xh, "f16"), ("f16", "f16"))
        o = out.cpu()
        assert bool((o == float("inf")).any()) and bool((o == float("-inf")).any()) and not bool(torch.isnan(o).any())
        for pair in (("f16", "f32"), ("bf16", "bf16"), ("bf16", "f32")):
            out, _ = run_case(sg, torch, f, host16(torch, xh, pair[0]), pair)
            assert bool(torch.isfinite(out).all()) and float(out.float().abs().max()) > 65504.0


# ------------------------------------------------------------------------------------------------
# 4. against the fp64 oracle of the widened input: one rounding to nearest of a result that already meets the project's fp32 rule
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 2, 5, 8, 12, 16, 19, 24, 32])
def test_h16_against_fp64_oracle(sg, sgo, torch_gpu, n):
    torch = torch_gpu
    rng = np.random.default_rng(2200 + n)
    for in_name, amp in (("f16", 2.0), ("bf16", 60.0)):
        x16 = host16(torch, signal(rng, (2, 12011), amp=amp), in_name)
        xw = x16.float().numpy()                                    # the widened input, exactly
        for (m, d, dt) in filter_sets(n):
            for mode, valid in [(mo, False) for mo in MODES] + [(0, True)]:
                o = sgo.Filter(n, m, d, dt, mode)
                ref = o.apply_f64(xw.astype(np.float64))
                r32 = o.apply(xw)
                if valid:
                    ref, r32 = ref[:, n:-n], r32[:, n:-n]
                bar32 = fp32_bar(normwise(r32, ref))
                f = sg.Filter(n, m, d, dt, mode)
                for pair in PAIRS:
                    if pair[0] != in_name:
                        continue
                    y = f.apply_tensor(x16.cuda(), valid=valid, flags=0, out_dtype=tdtype(torch, pair[1]))
                    u = UNIT[pair[1]]
                    check(normwise(y.float().cpu().numpy(), ref), u + (1.0 + u) * bar32, (n, m, d, dt, mode, valid, pair))


# ------------------------------------------------------------------------------------------------
# 5. refusals on the device: no launch, the outputs are still NaN-filled
# ------------------------------------------------------------------------------------------------
def test_h16_refusals_launch_nothing(sg, torch_gpu):
    torch = torch_gpu
    ch, length = 4, 5000
    x = host16(torch, signal(np.random.default_rng(2300), (ch, length)), "f16").cuda()
    out = torch.full((ch, length), float("nan"), dtype=torch.float16, device="cuda")
    out32 = torch.full((ch, length), float("nan"), dtype=torch.float32, device="cuda")
    f = sg.Filter(8, 3, 1)
    bad = [
        (dict(dtype="f16", flags=sg.SAVGOL_BATCH_REFERENCE_SUMMATION), out, "REFERENCE_SUMMATION"),
        (dict(dtype="f16", flags=sg.SAVGOL_BATCH_TILE_WIDE), out, "TILE_WIDE"),
        (dict(dtype="f16", flags=sg.SAVGOL_BATCH_MOMENT_F64), out, "belong to other calls"),
        (dict(dtype="f16", flags=sg.SAVGOL_BATCH_BOUNDARY_AWARE), out, "belong to other calls"),
        (dict(dtype="f16", out_dtype="bf16"), out, "f16 -> bf16"),
        (dict(dtype="bf16", out_dtype="f16"), out, "bf16 -> f16"),
        (dict(dtype="f16", in_ld=length - 1), out, "row pitch smaller than the row"),
        (dict(dtype="f16", out_dtype="f32", out_ld=length - 17), out32, "row pitch smaller than the row"),
    ]
    for kw, o, text in bad:
        for valid in (False, True):
            with pytest.raises(RuntimeError, match=text.replace(">", r"\>")):
                f.apply_batch(x, o, ch, length, valid=valid, **kw)
    lib = sg.lib()
    assert lib.savgol_apply_batch_h16(f.ptr, x.data_ptr(), sg.SAVGOL_HIP_F32, out32.data_ptr(), sg.SAVGOL_HIP_F32, ch, length, length, length, 0, None) == -1
    assert "f32 -> f32" in sg.last_error()
    assert lib.savgol_apply_batch_h16(f.ptr, x.data_ptr(), sg.SAVGOL_HIP_F16, out.data_ptr(), sg.SAVGOL_HIP_F16, ch, 10, 10, 10, 0, None) == -1
    assert "data length (10) < window size (17)" in sg.last_error()
    torch.cuda.synchronize()
    assert bool(torch.isnan(out).all()) and bool(torch.isnan(out32).all())
    # in place and shifted overlaps: the input is untouched
    before = x.clone()
    flat = x.view(-1)
    for target in (x, flat[1:], flat[length - 3:]):
        with pytest.raises(RuntimeError, match="d_in and d_out overlap"):
            f.apply_batch(x, target, ch - 1, length, dtype="f16")
    torch.cuda.synchronize()
    assert torch.equal(as_int(torch, x), as_int(torch, before))


# ------------------------------------------------------------------------------------------------
# 6. full size: 4096 x 2^20, n = 32, m = 4, bf16 -> bf16
# ------------------------------------------------------------------------------------------------
def test_h16_full_size(sg, torch_gpu):
    torch = torch_gpu
    channels, length = 4096, 1 << 20
    free, _ = torch.cuda.mem_get_info()
    assert free > 5 * 4 * channels * length, "the headline shape needs 40 GiB of free device memory"
    x32 = torch.empty((channels, length), dtype=torch.float32, device="cuda")
    sg.synth(x32)
    x = x32.to(torch.bfloat16)
    del x32
    f = sg.Filter(32, 4, 0, 1.0, 0)
    y = f.apply_tensor(x)
    torch.cuda.synchronize()
    # the fp32 call on the whole widened batch, 1024 rows at a time; compared on a fixed sample of columns of EVERY row (row ends and tile seams
    # included) and on every column of the first and the last row of each part
    cols = torch.cat([torch.arange(0, 96), torch.arange(2048 - 48, 2048 + 48), torch.arange(7, length, 4099), torch.arange(length - 96, length)]).cuda()
    part = 1024
    for r0 in range(0, channels, part):
        xw = x[r0:r0 + part].float()
        ref = torch.empty_like(xw)
        f.apply_batch(xw, ref, part, length, flags=sg.SAVGOL_BATCH_TILE_NARROW)
        torch.cuda.synchronize()
        same_after_rounding(torch, y[r0:r0 + part][:, cols], ref[:, cols].cpu().to(torch.bfloat16), ("headline columns", r0))
        same_after_rounding(torch, y[[r0, r0 + part - 1]], ref[[0, part - 1]].cpu().to(torch.bfloat16), ("headline rows", r0))
        del xw, ref
    del x, y
    torch.cuda.empty_cache()


# ------------------------------------------------------------------------------------------------
# 7. graph capture
# ------------------------------------------------------------------------------------------------
def test_h16_graph_capture(sg, torch_gpu):
    """after one warm-up call with the same filter the call only enqueues: it captures into a graph and replays to the same bits"""
    torch = torch_gpu
    rng = np.random.default_rng(2700)
    for pair, n in ((("bf16", "bf16"), 12), (("f16", "f32"), 24)):
        x = host16(torch, signal(rng, (8, 40000)), pair[0]).cuda()
        f = sg.Filter(n, 4, 1, 1.0, 0)
        want = f.apply_tensor(x, out_dtype=tdtype(torch, pair[1]))
        out = torch.full((8, 40000), float("nan"), dtype=tdtype(torch, pair[1]), device="cuda")
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        g = torch.cuda.CUDAGraph()
        with torch.cuda.stream(s):
            with torch.cuda.graph(g, stream=s):
                f.apply_batch(x, out, 8, 40000, dtype=pair[0], out_dtype=pair[1], stream=s)
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(as_int(torch, out), as_int(torch, want))
        same_after_rounding(torch, out, expected(sg, torch, f, x, pair[1], False, 0), ("graph", pair))
