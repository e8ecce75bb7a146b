"""GPU tests of the fused multi-output 1-D call on 16-bit storage (savgol_apply[_valid]_multi_batch_h16, sg_k1d_multi_st16.hpp).  The contract: output k
equals, bit for bit, the EXISTING 16-bit single call with SAVGOL_BATCH_PLAIN_SUMMATION, and output k of the EXISTING fp32 fused call on the widened
input under SAVGOL_BATCH_TILE_NARROW rounded to nearest even into the output type (torch's CPU cast) -- every half window, boundary mode, VALID, both
input types and both output choices, counts 2 / 3 / 4 in mixes that put a derivative first, two smoothing filters together, only smoothing (no
centring) and only derivatives (nraw = 0), with and without CORRECT_LEADING_EDGE; shifted bases, odd pitches and guarded NaN-filled outputs; the
centred route on an offset signal against the fp64 oracle; Inf / NaN / subnormal / overflowing values; refused calls launch nothing; graph capture;
the edge-item indexing across many channels.  Expected values never come from the code under test.  Equality is exact apart from NaN payloads."""
import ctypes as C

import numpy as np
import pytest

from tests._util import check, fp32_bar, normwise
from tests.test_gpu_1d_h16 import MODES, PAIRS, UNIT, alloc, as_int, host16, signal, tdtype

pytestmark = pytest.mark.gpu

TILE = 2048                                                          # samples of the narrow tile


@pytest.fixture(scope="module")
def torch_gpu(sg):
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    assert sg.device_count() > 0, sg.last_error()
    return torch


def lengths(n):
    """the minimum, one tile -1 / exact / +1, two tiles and a 3-sample third, five tiles with a partial end"""
    return (2 * n + 1, TILE - 1, TILE, TILE + 1, 2 * TILE + 3, 9004)


def pool(n, mode):
    """[(poly_order, derivative, time_step)] the mixes draw from: 0 / 3 smoothing, 1 / 2 / 4 derivatives (poly_order capped below the window)"""
    m4 = min(4, 2 * n)
    return [(m4, 0, 1.0), (m4, 1, 1.0), (m4, 2, 0.25), (2, 0, 1.0), (min(3, 2 * n), 1, 0.5)]


# indices into pool(): a derivative first | two smoothing filters together | all smoothing (no centring) | all derivatives (nraw = 0) |
# four: a launch of (derivative, smoothing) and one of (smoothing, derivative) | four, the second launch all derivatives
MIXES = ((1, 0), (0, 3, 1), (3, 0), (1, 2, 4), (1, 0, 3, 2), (0, 3, 4, 2))


def same_bits(torch, got, want, label):
    """on the device: the NaN masks coincide (payloads are free), every other element is equal bit for bit"""
    assert got.shape == want.shape and got.dtype == want.dtype, (label, got.shape, want.shape)
    gn, wn = torch.isnan(got), torch.isnan(want)
    a, b = as_int(torch, got), as_int(torch, want.to(got.device))
    ok = bool(torch.equal(gn, wn.to(got.device))) and not bool(((a != b) & ~gn).any())
    assert ok, (label, "NaN masks differ" if not torch.equal(gn, wn.to(got.device)) else f"{int(((a != b) & ~gn).sum())} values differ")


def singles(sg, torch, filters, x, pair, valid, flags):
    """the contract's first right-hand side: the existing 16-bit single call with PLAIN_SUMMATION, one per filter"""
    return [f.apply_tensor(x, valid=valid, flags=flags | sg.SAVGOL_BATCH_PLAIN_SUMMATION, out_dtype=tdtype(torch, pair[1])) for f in filters]


def rounded_fp32_multi(sg, torch, filters, x, pair, valid, flags):
    """the second: the existing fp32 fused call on the widened input (narrow tile), cast on the CPU (round to nearest even)"""
    ys = sg.apply_multi_tensor(filters, x.float().contiguous(), valid=valid, flags=flags | sg.SAVGOL_BATCH_TILE_NARROW)
    torch.cuda.synchronize()
    return [y.cpu().to(tdtype(torch, pair[1])) for y in ys]


def run_multi(sg, torch, filters, xh16, pair, valid=False, flags=0, in_shift=0, out_shifts=None, in_pad=0, out_pad=0):
    """xh16: host or device tensor [channels, length] of the input type.  Runs the fused 16-bit call on the given layout (every output in NaN-filled
    storage of its own, shifted by out_shifts[k] elements), checks that nothing outside the rows was written; returns the outputs [channels, out_len]."""
    ch, length = xh16.shape
    n = filters[0].n
    out_len = length - 2 * n if valid else length
    in_ld, out_ld = length + in_pad, out_len + out_pad
    out_shifts = [0] * len(filters) if out_shifts is None else out_shifts
    _, x = alloc(torch, xh16.dtype, ch, in_ld, in_shift)
    x[:, :length] = xh16.cuda()
    bufs = [alloc(torch, tdtype(torch, pair[1]), ch, out_ld, s) for s in out_shifts]
    sg.apply_multi_batch(filters, x, [o for _, o in bufs], ch, length, in_ld, out_ld, flags=flags, valid=valid, dtype=pair[0], out_dtype=pair[1])
    torch.cuda.synchronize()
    label = (n, pair, valid, flags, (in_shift, out_shifts, in_pad, out_pad), length)
    for k, ((base, out), s) in enumerate(zip(bufs, out_shifts)):
        if out_pad:
            assert bool(torch.isnan(out[:, out_len:]).all()), (label, k, "pitch padding written")
        assert bool(torch.isnan(base[:s]).all()) and bool(torch.isnan(base[s + ch * out_ld:]).all()), (label, k, "guard written")
    return [out[:, :out_len] for _, out in bufs]


# ------------------------------------------------------------------------------------------------
# 1. the contract: N = 1..32, every boundary mode and VALID, four type pairs, counts 2 / 3 / 4, with and without CORRECT_LEADING_EDGE
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", range(1, 33))
def test_multi_h16_bit_identical_to_the_single_calls_and_the_rounded_fp32_call(sg, torch_gpu, n):
    torch = torch_gpu
    rng = np.random.default_rng(3100 + n)
    CLE = sg.SAVGOL_BATCH_CORRECT_LEADING_EDGE
    for length in lengths(n):
        xh = signal(rng, (3, length))
        for in_name in ("f16", "bf16"):
            x = host16(torch, xh, in_name).cuda()
            for mode, valid in [(mo, False) for mo in MODES] + [(0, True)]:
                fs = [sg.Filter(n, m, d, dt, mode) for m, d, dt in pool(n, mode)]
                for flags in (0, CLE) if (mode == 0 and not valid) else (0,):       # the flag only acts on the POLYNOMIAL leading edge of odd derivatives
                    for pair in PAIRS:
                        if pair[0] != in_name:
                            continue
                        want = singles(sg, torch, fs, x, pair, valid, flags)
                        for mix in MIXES:
                            got = sg.apply_multi_tensor([fs[i] for i in mix], x, valid=valid, flags=flags, out_dtype=tdtype(torch, pair[1]))
                            for k, i in enumerate(mix):
                                same_bits(torch, got[k], want[i], (n, length, pair, mode, valid, flags, mix, k, "single call"))
                        if length in (TILE + 1, 9004):
                            # the subset held against the fp32 fused call as well: three outputs, and four (two launches)
                            for mix in (MIXES[1], MIXES[4]):
                                got = sg.apply_multi_tensor([fs[i] for i in mix], x, valid=valid, flags=flags, out_dtype=tdtype(torch, pair[1]))
                                ref = rounded_fp32_multi(sg, torch, [fs[i] for i in mix], x, pair, valid, flags)
                                for k in range(len(mix)):
                                    same_bits(torch, got[k], ref[k], (n, length, pair, mode, valid, flags, mix, k, "rounded fp32 fused call"))


def test_multi_h16_correct_leading_edge_acts(sg, torch_gpu):
    """the flag reaches every output's edge items: the leading n outputs of the odd derivative change sign, nothing else changes"""
    torch = torch_gpu
    xh = signal(np.random.default_rng(3150), (2, 5000))
    for n in (3, 24):
        fs = [sg.Filter(n, 4, 0), sg.Filter(n, 3, 1), sg.Filter(n, 4, 2)]
        for pair in PAIRS:
            x = host16(torch, xh, pair[0]).cuda()
            a = sg.apply_multi_tensor(fs, x, out_dtype=tdtype(torch, pair[1]))
            b = sg.apply_multi_tensor(fs, x, flags=sg.SAVGOL_BATCH_CORRECT_LEADING_EDGE, out_dtype=tdtype(torch, pair[1]))
            assert torch.equal(b[1][:, :n].float(), -a[1][:, :n].float()) and torch.equal(as_int(torch, b[1][:, n:]), as_int(torch, a[1][:, n:]))
            for k in (0, 2):
                assert torch.equal(as_int(torch, a[k]), as_int(torch, b[k]))


# ------------------------------------------------------------------------------------------------
# 2. layouts: bases shifted by 1..4 elements, odd pitches, fp32 output 8-byte but not 16-byte aligned, NaN-filled storage with guards
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [2, 7, 24, 32])
def test_multi_h16_shifted_bases_pitches_and_guards(sg, torch_gpu, n):
    torch = torch_gpu
    rng = np.random.default_rng(3200 + n)
    # in_shift, out_shifts (one per output), in_pad, out_pad; (0, (2, 2, 2), ..): fp32 output rows 8-byte aligned only, 16-bit rows 4-byte aligned
    layouts = [(0, (0, 0, 0), 0, 0), (1, (2, 3, 4), 3, 1), (2, (3, 1, 2), 0, 5), (3, (1, 4, 0), 1, 0), (4, (4, 2, 1), 4, 4), (0, (2, 2, 2), 4, 8), (4, (0, 4, 2), 0, 0),
               (0, (2, 0, 2), 1, 3)]
    case = 0
    for length in lengths(n):
        xh = signal(rng, (3, length))
        for layout in layouts:
            for pair in PAIRS:
                mode, valid = MODES[case % 4], case % 3 == 2
                mix = MIXES[case % 4] if case % 5 else (0, 1, 2)
                case += 1
                fs = [sg.Filter(n, m, d, dt, mode) for m, d, dt in pool(n, mode)]
                x = host16(torch, xh, pair[0])
                got = run_multi(sg, torch, [fs[i] for i in mix], x, pair, valid=valid, in_shift=layout[0], out_shifts=layout[1][:len(mix)], in_pad=layout[2],
                                out_pad=layout[3])
                want = singles(sg, torch, fs, x.cuda(), pair, valid, 0)
                for k, i in enumerate(mix):
                    same_bits(torch, got[k].contiguous(), want[i], (n, length, layout, pair, mode, valid, mix, k))


# ------------------------------------------------------------------------------------------------
# 3. the centred route: derivative outputs on a signal whose offset is 100 x its variation
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [3, 8, 20, 32])
def test_multi_h16_centred_derivatives_on_an_offset_signal(sg, sgo, torch_gpu, n):
    torch = torch_gpu
    rng = np.random.default_rng(3300 + n)
    xh = signal(rng, (3, 9004), offset=200.0, amp=2.0)
    for in_name in ("f16", "bf16"):
        x16 = host16(torch, xh, in_name)
        xw = x16.float().numpy()                                    # the widened input, exactly
        x = x16.cuda()
        for mode, valid in [(mo, False) for mo in MODES] + [(0, True)]:
            specs = [(4, 1, 0.5), (4, 2, 0.5), (3, 1, 1.0)]
            fs = [sg.Filter(n, m, d, dt, mode) for m, d, dt in specs]
            bars = []
            for m, d, dt in specs:
                o = sgo.Filter(n, m, d, dt, mode)
                ref, r32 = o.apply_f64(xw.astype(np.float64)), o.apply(xw)
                if valid:
                    ref, r32 = ref[:, n:-n], r32[:, n:-n]
                bars.append((ref, fp32_bar(normwise(r32, ref))))
            for pair in PAIRS:
                if pair[0] != in_name:
                    continue
                got = sg.apply_multi_tensor(fs, x, valid=valid, out_dtype=tdtype(torch, pair[1]))
                want = singles(sg, torch, fs, x, pair, valid, 0)
                u = UNIT[pair[1]]
                for k in range(3):
                    same_bits(torch, got[k], want[k], (n, pair, mode, valid, k))
                    ref, bar32 = bars[k]
                    check(normwise(got[k].float().cpu().numpy(), ref), u + (1.0 + u) * bar32, (n, specs[k], mode, valid, pair))


# ------------------------------------------------------------------------------------------------
# 4. special values
# ------------------------------------------------------------------------------------------------
def test_multi_h16_inf_and_nan_samples(sg, torch_gpu):
    """the NaN / Inf footprint of the single call, output by output"""
    torch = torch_gpu
    rng = np.random.default_rng(3400)
    xh = signal(rng, (4, 9004))
    for at, v in ((3, np.inf), (700, -np.inf), (2047, np.nan), (2048, np.inf), (4100, np.nan), (9003, -np.inf), (6000, np.inf), (6001, -np.inf)):
        xh[at % 4, at] = v
    for n in (4, 12, 24, 32):
        for mode in MODES:
            fs = [sg.Filter(n, m, d, dt, mode) for m, d, dt in pool(n, mode)]
            for pair in PAIRS:
                x = host16(torch, xh, pair[0]).cuda()
                want = singles(sg, torch, fs, x, pair, False, 0)
                for mix in ((0, 1, 2), (1, 4), (3, 0)):
                    got = sg.apply_multi_tensor([fs[i] for i in mix], x, out_dtype=tdtype(torch, pair[1]))
                    for k, i in enumerate(mix):
                        assert bool(torch.isnan(want[i]).any()) and bool(torch.isinf(want[i]).any())
                        same_bits(torch, got[k], want[i], (n, mode, pair, mix, k))
                        assert torch.equal(torch.isinf(got[k]), torch.isinf(want[i]))


def test_multi_h16_fp16_subnormal_inputs_widen_exactly(sg, torch_gpu):
    torch = torch_gpu
    rng = np.random.default_rng(3500)
    bits = rng.integers(1, 1024, (3, 6000)).astype(np.int16) | (rng.integers(0, 2, (3, 6000)).astype(np.int16) << 15)      # every fp16 subnormal, both signs
    x = torch.from_numpy(bits).view(torch.float16).cuda()
    assert float(x.float().abs().max()) < 2.0 ** -14
    for n, m in ((1, 0), (6, 2), (24, 4)):
        fs = [sg.Filter(n, m, 0, 1.0, 1), sg.Filter(n, max(m, 1), 1, 1.0, 1)]
        for pair in (("f16", "f32"), ("f16", "f16")):
            got = sg.apply_multi_tensor(fs, x, out_dtype=tdtype(torch, pair[1]))
            want = singles(sg, torch, fs, x, pair, False, 0)
            ref = rounded_fp32_multi(sg, torch, fs, x, pair, False, 0)
            for k in range(2):
                assert float(want[k].float().abs().max()) > 0.0
                same_bits(torch, got[k], want[k], (n, pair, k))
                same_bits(torch, got[k], ref[k], (n, pair, k, "rounded fp32 fused call"))


def test_multi_h16_overflow_to_fp16_gives_inf(sg, torch_gpu):
    """results beyond 65504: +-Inf in fp16 output (IEEE rounding), finite in bf16 and fp32 output; the smoothing output beside it stays finite"""
    torch = torch_gpu
    t = np.arange(9004, dtype=np.float64)
    xh = np.stack([4000.0 * np.sin(0.05 * t), 4000.0 * np.cos(0.05 * t)]).astype(np.float32)
    for n in (5, 24):
        fs = [sg.Filter(n, 3, 1, 1e-3, 1), sg.Filter(n, 2, 0, 1.0, 1)]        # d/dt with time_step 1e-3: amplitude 2e5
        for pair in PAIRS:
            x = host16(torch, xh, pair[0]).cuda()
            got = sg.apply_multi_tensor(fs, x, out_dtype=tdtype(torch, pair[1]))
            want = singles(sg, torch, fs, x, pair, False, 0)
            for k in range(2):
                same_bits(torch, got[k], want[k], (n, pair, k))
            assert bool(torch.isfinite(got[1]).all())
            if pair == ("f16", "f16"):
                assert bool((got[0] == float("inf")).any()) and bool((got[0] == float("-inf")).any()) and not bool(torch.isnan(got[0]).any())
            else:
                assert bool(torch.isfinite(got[0]).all()) and float(got[0].float().abs().max()) > 65504.0


# ------------------------------------------------------------------------------------------------
# 5. refusals on the device: no launch, the outputs are still NaN-filled
# ------------------------------------------------------------------------------------------------
def test_multi_h16_refusals_launch_nothing(sg, torch_gpu):
    torch = torch_gpu
    ch, length = 4, 5000
    x = host16(torch, signal(np.random.default_rng(3600), (ch, length)), "f16").cuda()
    outs = [torch.full((ch, length), float("nan"), dtype=torch.float16, device="cuda") for _ in range(3)]
    outs32 = [torch.full((ch, length), float("nan"), dtype=torch.float32, device="cuda") for _ in range(3)]
    fs = [sg.Filter(8, 4, 0), sg.Filter(8, 3, 1), sg.Filter(8, 4, 2)]
    bad = [
        (dict(dtype="f16", flags=sg.SAVGOL_BATCH_REFERENCE_SUMMATION), outs, "REFERENCE_SUMMATION"),
        (dict(dtype="f16", flags=sg.SAVGOL_BATCH_TILE_WIDE), outs, "TILE_WIDE"),
        (dict(dtype="f16", flags=sg.SAVGOL_BATCH_MOMENT_F64), outs, "belong to other calls"),
        (dict(dtype="f16", flags=sg.SAVGOL_BATCH_BOUNDARY_AWARE), outs, "belong to other calls"),
        (dict(dtype="f16", flags=0x1000), outs, "bad flags"),
        (dict(dtype="f16", out_dtype="bf16"), outs, "f16 -> bf16"),
        (dict(dtype="bf16", out_dtype="f16"), outs, "bf16 -> f16"),
        (dict(dtype="f16", in_ld=length - 1), outs, "row pitch smaller than the row"),
        (dict(dtype="f16", out_dtype="f32", out_ld=length - 17), outs32, "row pitch smaller than the row"),
        (dict(dtype="f16", filters=[fs[0], sg.Filter(9, 3, 1)]), outs[:2], "half_window"),
        (dict(dtype="f16", filters=[fs[0], sg.Filter(8, 3, 1, 1.0, sg.SAVGOL_BOUNDARY_REFLECT)]), outs[:2], "boundary"),
        (dict(dtype="f16", length=10, in_ld=length, out_ld=length), outs, r"data length \(10\) < window size \(17\)"),
        (dict(dtype="f16"), [outs[0], outs[1], outs[0]], r"d_outs\[0\] and d_outs\[2\] overlap"),
        (dict(dtype="f16", channels=ch - 1), [outs[0], outs[0].view(-1)[length - 1:], outs[2]], r"d_outs\[0\] and d_outs\[1\] overlap"),     # one element shared
    ]
    for kw, o, text in bad:
        kw = dict(kw)
        filters, L, channels = kw.pop("filters", fs), kw.pop("length", length), kw.pop("channels", ch)
        for valid in (False, True):
            with pytest.raises(RuntimeError, match=text.replace(">", r"\>")):
                sg.apply_multi_batch(filters, x, o[:len(filters)], channels, L, valid=valid, **kw)
    F = sg.lib().savgol_apply_multi_batch_h16
    for count in (0, 5):
        ptrs = (C.c_void_p * 5)(*[o.data_ptr() for o in (outs + outs32)[:5]])
        farr = (C.POINTER(sg.SavgolFilter) * 5)(*[fs[k % 3].ptr for k in range(5)])
        assert F(farr, count, x.data_ptr(), sg.SAVGOL_HIP_F16, ptrs, sg.SAVGOL_HIP_F16, ch, length, length, length, 0, None) == -1
        assert f"count {count} outside 1..4" in sg.last_error()
    torch.cuda.synchronize()
    assert all(bool(torch.isnan(o).all()) for o in outs + outs32)
    # in place and shifted overlaps with the input: the input is untouched
    before = x.clone()
    flat = x.view(-1)
    for target in (x, flat[1:], flat[length - 3:]):
        with pytest.raises(RuntimeError, match=r"d_outs\[1\] overlaps d_in"):
            sg.apply_multi_batch(fs, x, [outs[0], target, outs[2]], ch - 1, length, dtype="f16")
    torch.cuda.synchronize()
    assert torch.equal(as_int(torch, x), as_int(torch, before)) and all(bool(torch.isnan(o).all()) for o in outs)


# ------------------------------------------------------------------------------------------------
# 6. graph capture
# ------------------------------------------------------------------------------------------------
def test_multi_h16_graph_capture(sg, torch_gpu):
    """after one warm-up call with the same filters the call only enqueues: a count-3 call captures into a graph and replays to the eager bits"""
    torch = torch_gpu
    rng = np.random.default_rng(3700)
    for pair, n in ((("bf16", "bf16"), 12), (("f16", "f32"), 24)):
        x = host16(torch, signal(rng, (8, 40000)), pair[0]).cuda()
        fs = [sg.Filter(n, 4, 0, 1.0, 0), sg.Filter(n, 4, 1, 1.0, 0), sg.Filter(n, 4, 2, 0.5, 0)]
        want = sg.apply_multi_tensor(fs, x, out_dtype=tdtype(torch, pair[1]))
        outs = [torch.full((8, 40000), float("nan"), dtype=tdtype(torch, pair[1]), device="cuda") for _ in fs]
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        g = torch.cuda.CUDAGraph()
        with torch.cuda.stream(s):
            with torch.cuda.graph(g, stream=s):
                sg.apply_multi_batch(fs, x, outs, 8, 40000, dtype=pair[0], out_dtype=pair[1], stream=s)
        g.replay()
        torch.cuda.synchronize()
        single = singles(sg, torch, fs, x, pair, False, 0)
        for k in range(3):
            assert torch.equal(as_int(torch, outs[k]), as_int(torch, want[k]))
            same_bits(torch, outs[k], single[k], ("graph", pair, k))


# ------------------------------------------------------------------------------------------------
# 7. many channels: the edge items' indexing (channel it / 2K, output (it % 2K) / 2, end it % 2) and the tile -> channel map
# ------------------------------------------------------------------------------------------------
def test_multi_h16_edge_items_across_many_channels(sg, torch_gpu):
    torch = torch_gpu
    rng = np.random.default_rng(3800)
    xh = signal(rng, (100, 2 * TILE + 3))
    for pair, n, mix in ((("bf16", "bf16"), 5, (1, 0, 2)), (("f16", "f32"), 21, (0, 1)), (("f16", "f16"), 32, (1, 0, 3, 2))):
        fs = [sg.Filter(n, m, d, dt, 0) for m, d, dt in pool(n, 0)]                # POLYNOMIAL: 2 K edge items per channel
        x = host16(torch, xh, pair[0])
        got = run_multi(sg, torch, [fs[i] for i in mix], x, pair, out_pad=1)
        want = singles(sg, torch, fs, x.cuda(), pair, False, 0)
        for k, i in enumerate(mix):
            same_bits(torch, got[k].contiguous(), want[i], (n, pair, mix, k))
