"""GPU tests of the fused multi-output 1-D call on int16 storage (savgol_apply[_valid]_multi_batch_i16, sg_k1d_multi_st16.hpp).  The contract: output k
equals, bit for bit, the EXISTING int16 single call with SAVGOL_BATCH_PLAIN_SUMMATION, and output k of the EXISTING fp32 fused call on the widened
input under SAVGOL_BATCH_TILE_NARROW, converted once on the CPU (round to nearest even, saturate, NaN -> 0: to_out) -- every half window, boundary
mode, VALID, both output types, counts 2 / 3 / 4 in mixes that put a derivative first, two smoothing filters together, only smoothing (no centring)
and only derivatives (nraw = 0), with and without CORRECT_LEADING_EDGE; saturation and overflow to +-Inf; shifted bases, odd pitches and guarded
sentinel-filled outputs; the centred route on an offset signal against the fp64 oracle; refused calls launch nothing; graph capture; the edge-item
indexing across many channels.  Expected values never come from the code under test.  Equality is exact apart from NaN payloads."""
import ctypes as C

import numpy as np
import pytest

from tests._util import check, fp32_bar, normwise
from tests.test_gpu_1d_i16 import MODES, OUTS, alloc, full_scale, oracle_signal, same, sentinel, small_signal, tdtype, to_out, untouched
from tests.test_gpu_1d_multi_h16 import MIXES, TILE, lengths, pool

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch_gpu(sg):
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    assert sg.device_count() > 0, sg.last_error()
    return torch


def singles(sg, torch, filters, x, out_name, valid, flags):
    """the contract's first right-hand side: the existing int16 single call with PLAIN_SUMMATION, one per filter; host tensors"""
    ys = [f.apply_tensor_i16(x, valid=valid, flags=flags | sg.SAVGOL_BATCH_PLAIN_SUMMATION, out_dtype=tdtype(torch, out_name)) for f in filters]
    torch.cuda.synchronize()
    return [y.cpu() for y in ys]


def fp32_multi(sg, torch, filters, x, valid, flags):
    """the second: the existing fp32 fused call on the widened input (narrow tile); host fp32 tensors, to be converted by to_out"""
    ys = sg.apply_multi_tensor(filters, x.float().contiguous(), valid=valid, flags=flags | sg.SAVGOL_BATCH_TILE_NARROW)
    torch.cuda.synchronize()
    return [y.cpu() for y in ys]


def run_multi(sg, torch, filters, xh, out_name, valid=False, flags=0, in_shift=0, out_shifts=None, in_pad=0, out_pad=0):
    """xh: host int16 tensor [channels, length].  Runs the fused int16 call on the given layout (every output in sentinel-filled storage of its own,
    shifted by out_shifts[k] elements), checks that nothing outside the rows was written; returns the outputs [channels, out_len]."""
    ch, length = xh.shape
    n = filters[0].n
    out_len = length - 2 * n if valid else length
    in_ld, out_ld = length + in_pad, out_len + out_pad
    out_shifts = [0] * len(filters) if out_shifts is None else out_shifts
    _, x = alloc(torch, torch.int16, ch, in_ld, in_shift)
    x[:, :length] = xh.cuda()
    bufs = [alloc(torch, tdtype(torch, out_name), ch, out_ld, s) for s in out_shifts]
    sg.apply_multi_batch_i16(filters, x, [o for _, o in bufs], ch, length, in_ld, out_ld, out_dtype=out_name, flags=flags, valid=valid)
    torch.cuda.synchronize()
    label = (n, out_name, valid, flags, (in_shift, out_shifts, in_pad, out_pad), length)
    for k, ((base, out), s) in enumerate(zip(bufs, out_shifts)):
        if out_pad:
            assert untouched(torch, out[:, out_len:]), (label, k, "pitch padding written")
        assert untouched(torch, base[:s]) and untouched(torch, base[s + ch * out_ld:]), (label, k, "guard written")
    return [out[:, :out_len] for _, out in bufs]


# ------------------------------------------------------------------------------------------------
# 1. the contract: N = 1..32, every boundary mode and VALID, both output types, counts 2 / 3 / 4, with and without CORRECT_LEADING_EDGE
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", range(1, 33))
def test_multi_i16_bit_identical_to_the_single_calls_and_the_converted_fp32_call(sg, torch_gpu, n):
    torch = torch_gpu
    rng = np.random.default_rng(5100 + n)
    CLE = sg.SAVGOL_BATCH_CORRECT_LEADING_EDGE
    unsaturated = False
    for length in lengths(n):
        # full_scale places its plateaus up to sample 4800: cut from a long row
        for what, xh in (("+-200 counts", small_signal(rng, (3, length))), ("full scale", full_scale(rng, (3, max(length, 5000)))[:, :length].copy())):
            x = torch.from_numpy(xh).cuda()
            for mode, valid in [(mo, False) for mo in MODES] + [(0, True)]:
                fs = [sg.Filter(n, m, d, dt, mode) for m, d, dt in pool(n, mode)]
                for flags in (0, CLE) if (mode == 0 and not valid) else (0,):       # the flag only acts on the POLYNOMIAL leading edge of odd derivatives
                    for out_name in OUTS:
                        want = singles(sg, torch, fs, x, out_name, valid, flags)
                        if what == "+-200 counts" and out_name == "i16":
                            unsaturated = unsaturated or all(int(w.abs().max()) < 32767 for w in want)
                        for mix in MIXES:
                            got = sg.apply_multi_tensor_i16([fs[i] for i in mix], x, valid=valid, flags=flags, out_dtype=tdtype(torch, out_name))
                            for k, i in enumerate(mix):
                                same(torch, got[k], want[i], (n, length, what, out_name, mode, valid, flags, mix, k, "single call"))
                        if length in (TILE + 1, 9004):
                            # held against the fp32 fused call as well: three outputs, and four (two launches)
                            for mix in (MIXES[1], MIXES[3], MIXES[4], MIXES[5]):
                                got = sg.apply_multi_tensor_i16([fs[i] for i in mix], x, valid=valid, flags=flags, out_dtype=tdtype(torch, out_name))
                                ref = fp32_multi(sg, torch, [fs[i] for i in mix], x, valid, flags)
                                for k in range(len(mix)):
                                    same(torch, got[k], to_out(torch, ref[k], out_name), (n, length, what, out_name, mode, valid, flags, mix, k, "fp32 fused call"))
    assert unsaturated, "every int16 output of the small signal saturated"


def test_multi_i16_correct_leading_edge_acts(sg, torch_gpu):
    """the flag reaches every output's edge items: the leading n outputs of the odd derivative change sign, nothing else changes"""
    torch = torch_gpu
    x = torch.from_numpy(small_signal(np.random.default_rng(5150), (2, 5000))).cuda()
    for n in (3, 24):
        fs = [sg.Filter(n, 4, 0), sg.Filter(n, 3, 1), sg.Filter(n, 4, 2)]
        for out_name in OUTS:
            a = sg.apply_multi_tensor_i16(fs, x, out_dtype=tdtype(torch, out_name))
            b = sg.apply_multi_tensor_i16(fs, x, flags=sg.SAVGOL_BATCH_CORRECT_LEADING_EDGE, out_dtype=tdtype(torch, out_name))
            assert torch.equal(b[1][:, :n], -a[1][:, :n]) and torch.equal(b[1][:, n:], a[1][:, n:]) and bool((a[1][:, :n] != 0).any())
            for k in (0, 2):
                assert torch.equal(a[k], b[k])


# ------------------------------------------------------------------------------------------------
# 2. saturation and the one conversion
# ------------------------------------------------------------------------------------------------
def test_multi_i16_saturates_once_per_output(sg, torch_gpu):
    """full-scale input: the smoothing output reaches both ends of the int16 range without being saturated throughout; a d/dt filter with
    time_step 1e-3 beside it saturates in int16 and is finite beyond the range in fp32"""
    torch = torch_gpu
    rng = np.random.default_rng(5200)
    x = torch.from_numpy(full_scale(rng, (3, 9004))).cuda()
    for n in (2, 5, 24):
        for mode in MODES:
            # a condition on the inputs, on the fp32 twin (not the call under test): two smoothing filters and a derivative of pool() reach both ends
            # of the range, and fewer than half of all their elements are saturated
            mixed = [sg.Filter(n, m, d, dt, mode) for m, d, dt in (pool(n, mode)[i] for i in MIXES[1])]
            ref = fp32_multi(sg, torch, mixed, x, False, 0)
            want16 = [to_out(torch, r, "i16") for r in ref]
            assert min(int(w.min()) for w in want16) == -32768 and max(int(w.max()) for w in want16) == 32767, (n, mode)
            assert all(int(w.min()) == -32768 and int(w.max()) == 32767 for w in want16[:2]), (n, mode)       # the smoothing outputs: the plateaus
            sat = sum(int(((w == -32768) | (w == 32767)).sum()) for w in want16)
            assert sat < sum(w.numel() for w in want16) // 2, (n, mode, sat)
            got = sg.apply_multi_tensor_i16(mixed, x)
            for k in range(3):
                same(torch, got[k], want16[k], (n, mode, k, "mixed"))
            # d/dt with time_step 1e-3 beside a smoothing filter
            fs = [sg.Filter(n, 3, 1, 1e-3, mode), sg.Filter(n, min(4, 2 * n), 0, 1.0, mode)]
            ref = fp32_multi(sg, torch, fs, x, False, 0)
            want16 = [to_out(torch, r, "i16") for r in ref]
            assert bool(torch.isfinite(ref[0]).all()) and float(ref[0].abs().max()) > 32767.0
            assert bool(((want16[0] == 32767) & (ref[0] > 40000.0)).any()) and bool(((want16[0] == -32768) & (ref[0] < -40000.0)).any())
            for out_name in OUTS:
                got = sg.apply_multi_tensor_i16(fs, x, out_dtype=tdtype(torch, out_name))
                single = singles(sg, torch, fs, x, out_name, False, 0)
                for k in range(2):
                    same(torch, got[k], to_out(torch, ref[k], out_name), (n, mode, out_name, k, "fp32 fused call"))
                    same(torch, got[k], single[k], (n, mode, out_name, k, "single call"))
                if out_name == "f32":
                    assert bool(torch.isfinite(got[0]).all()) and float(got[0].abs().max()) > 32767.0
            # the smoothing output beside the saturating one is the smoothing output beside an ordinary derivative
            tame = sg.apply_multi_tensor_i16([sg.Filter(n, 3, 1, 1.0, mode), fs[1]], x)
            got = sg.apply_multi_tensor_i16(fs, x)
            assert torch.equal(got[1], tame[1])


def test_multi_i16_overflow_to_inf_saturates(sg, torch_gpu):
    """a time_step so small that the fp32 results of a full-scale square wave overflow: +-Inf in fp32 output, 32767 / -32768 in int16 output, the
    masks those of the single call and of the fp32 fused call"""
    torch = torch_gpu
    t = np.arange(9004)
    square = np.where((t // 37) % 2 == 0, 32767, -32768).astype(np.int16)
    x = torch.from_numpy(np.stack([square, -1 - square, np.roll(square, 11)])).cuda()
    for n in (5, 24):
        for mode, valid in ((0, False), (1, False), (0, True)):
            fs = [sg.Filter(n, 3, 1, 1e-36, mode), sg.Filter(n, 2, 0, 1.0, mode), sg.Filter(n, 4, 1, 1e-36, mode)]
            ref = fp32_multi(sg, torch, fs, x, valid, 0)
            for k in (0, 2):
                assert bool((ref[k] == float("inf")).any()) and bool((ref[k] == float("-inf")).any()), (n, mode, valid, k)
            assert bool(torch.isfinite(ref[1]).all())
            got32 = sg.apply_multi_tensor_i16(fs, x, valid=valid, out_dtype=torch.float32)
            got16 = sg.apply_multi_tensor_i16(fs, x, valid=valid)
            single32 = singles(sg, torch, fs, x, "f32", valid, 0)
            single16 = singles(sg, torch, fs, x, "i16", valid, 0)
            for k in range(3):
                same(torch, got32[k], ref[k], (n, mode, valid, k, "f32"))
                same(torch, got32[k], single32[k], (n, mode, valid, k, "f32, single call"))
                same(torch, got16[k], to_out(torch, ref[k], "i16"), (n, mode, valid, k, "i16"))
                same(torch, got16[k], single16[k], (n, mode, valid, k, "i16, single call"))
                g32, g16 = got32[k].cpu(), got16[k].cpu()
                assert torch.equal(torch.isinf(g32), torch.isinf(single32[k]))
                assert bool((g16[g32 == float("inf")] == 32767).all()) and bool((g16[g32 == float("-inf")] == -32768).all())
                assert bool((g16[torch.isnan(g32)] == 0).all())


# ------------------------------------------------------------------------------------------------
# 3. layouts: bases shifted by 1..4 elements, odd pitches, fp32 output 8-byte but not 16-byte aligned, sentinel-filled storage with guards
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [2, 7, 24, 32])
def test_multi_i16_shifted_bases_pitches_and_guards(sg, torch_gpu, n):
    torch = torch_gpu
    rng = np.random.default_rng(5300 + n)
    # in_shift, out_shifts (one per output), in_pad, out_pad; (0, (2, 2, 2), ..): fp32 output rows 8-byte aligned only, int16 rows 4-byte aligned
    layouts = [(0, (0, 0, 0, 0), 0, 0), (1, (2, 3, 4, 1), 3, 1), (2, (3, 1, 2, 4), 0, 5), (3, (1, 4, 0, 2), 1, 0), (4, (4, 2, 1, 3), 4, 4), (0, (2, 2, 2, 2), 4, 8),
               (4, (0, 4, 2, 0), 0, 0), (0, (2, 0, 2, 0), 1, 3)]
    case = 0
    for length in lengths(n):
        xh = torch.from_numpy(oracle_signal(rng, (3, length)))
        for layout in layouts:
            for out_name in OUTS:
                mode, valid = MODES[case % 4], case % 3 == 2
                mix = MIXES[case % 6] if case % 5 else (0, 1, 2)
                case += 1
                fs = [sg.Filter(n, m, d, dt, mode) for m, d, dt in pool(n, mode)]
                got = run_multi(sg, torch, [fs[i] for i in mix], xh, out_name, valid=valid, in_shift=layout[0], out_shifts=layout[1][:len(mix)], in_pad=layout[2],
                                out_pad=layout[3])
                want = singles(sg, torch, fs, xh.cuda(), out_name, valid, 0)
                for k, i in enumerate(mix):
                    same(torch, got[k].contiguous(), want[i], (n, length, layout, out_name, mode, valid, mix, k))


# ------------------------------------------------------------------------------------------------
# 4. the centred route: derivative outputs on a signal whose offset is 100 x its variation
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [3, 8, 20, 32])
def test_multi_i16_centred_derivatives_on_an_offset_signal(sg, sgo, torch_gpu, n):
    """fp32 output: the project's fp32 bar against the fp64 oracle.  int16 output: |clip(rint(y)) - clip(ref)| <= |rint(y) - ref| <= 0.5 + |y - ref|
    (clipping to the int16 range moves no two values apart), so that bar plus half a count relative to the output's norm; the expected values are
    clipped because the modes that pad the offset signal with zeros leave the range at the channel ends."""
    torch = torch_gpu
    rng = np.random.default_rng(5400 + n)
    t = np.arange(9004, dtype=np.float64)
    x16 = torch.from_numpy(np.rint(20000.0 + 170.0 * np.sin(0.013 * t) + 20.0 * np.sin(0.41 * t + 1.0) + rng.uniform(-10, 10, (3, 9004))).astype(np.int16))
    assert int(x16.min()) >= 19800 and int(x16.max()) <= 20200
    xw = x16.float().numpy()                                        # the widened input, exactly
    x = x16.cuda()
    specs = [(4, 1, 0.5), (4, 2, 0.5), (3, 1, 1.0)]
    for mode, valid in [(mo, False) for mo in MODES] + [(0, True)]:
        fs = [sg.Filter(n, m, d, dt, mode) for m, d, dt in specs]
        bars = []
        for m, d, dt in specs:
            o = sgo.Filter(n, m, d, dt, mode)
            ref, r32 = o.apply_f64(xw.astype(np.float64)), o.apply(xw)
            if valid:
                ref, r32 = ref[:, n:-n], r32[:, n:-n]
            bars.append((ref, fp32_bar(normwise(r32, ref))))
        for out_name in OUTS:
            got = sg.apply_multi_tensor_i16(fs, x, valid=valid, out_dtype=tdtype(torch, out_name))
            want = singles(sg, torch, fs, x, out_name, valid, 0)
            for k in range(3):
                same(torch, got[k], want[k], (n, out_name, mode, valid, k))
                ref, bar32 = bars[k]
                y = got[k].cpu().numpy().astype(np.float64)
                top = float(np.max(np.abs(ref)))
                if out_name == "f32":
                    check(normwise(y, ref), bar32, (n, specs[k], mode, valid, "f32"))
                else:
                    check(float(np.max(np.abs(y - np.clip(ref, -32768.0, 32767.0)))) / top, bar32 + 0.5 / top, (n, specs[k], mode, valid, "i16"))


# ------------------------------------------------------------------------------------------------
# 5. refusals on the device: no launch, the outputs keep their sentinels
# ------------------------------------------------------------------------------------------------
def test_multi_i16_refusals_launch_nothing(sg, torch_gpu):
    torch = torch_gpu
    ch, length = 4, 5000
    x = torch.from_numpy(small_signal(np.random.default_rng(5600), (ch, length))).cuda()
    outs = [sentinel(torch, torch.int16, ch * length).view(ch, length) for _ in range(3)]
    outs32 = [sentinel(torch, torch.float32, ch * length).view(ch, length) for _ in range(3)]
    fs = [sg.Filter(8, 4, 0), sg.Filter(8, 3, 1), sg.Filter(8, 4, 2)]
    bad = [
        (dict(flags=sg.SAVGOL_BATCH_REFERENCE_SUMMATION), outs, "REFERENCE_SUMMATION"),
        (dict(flags=sg.SAVGOL_BATCH_TILE_WIDE), outs, "TILE_WIDE"),
        (dict(flags=sg.SAVGOL_BATCH_MOMENT_F64), outs, "belong to other calls"),
        (dict(flags=sg.SAVGOL_BATCH_BOUNDARY_AWARE), outs, "belong to other calls"),
        (dict(flags=0x1000), outs, "bad flags"),
        (dict(in_ld=length - 1), outs, "row pitch smaller than the row"),
        (dict(out_dtype="f32", out_ld=length - 17), outs32, "row pitch smaller than the row"),
        (dict(filters=[fs[0], sg.Filter(9, 3, 1)]), outs[:2], "half_window"),
        (dict(filters=[fs[0], sg.Filter(8, 3, 1, 1.0, sg.SAVGOL_BOUNDARY_REFLECT)]), outs[:2], "boundary"),
        (dict(length=10, in_ld=length, out_ld=length), outs, r"data length \(10\) \< window size \(17\)"),
        (dict(), [outs[0], outs[1], outs[0]], r"d_outs\[0\] and d_outs\[2\] overlap"),
        (dict(channels=ch - 1), [outs[0], outs[0].view(-1)[length - 1:], outs[2]], r"d_outs\[0\] and d_outs\[1\] overlap"),     # one element shared
        (dict(out_dtype="f32", channels=ch - 1), [outs32[0], outs32[1], outs32[1].view(-1)[length - 1:]], r"d_outs\[1\] and d_outs\[2\] overlap"),
    ]
    for kw, o, text in bad:
        kw = dict(kw)
        filters, L, channels = kw.pop("filters", fs), kw.pop("length", length), kw.pop("channels", ch)
        for valid in (False, True):
            with pytest.raises(RuntimeError, match=text):
                sg.apply_multi_batch_i16(filters, x, o[:len(filters)], channels, L, valid=valid, **kw)
    F = sg.lib().savgol_apply_multi_batch_i16
    ptrs = (C.c_void_p * 5)(*[o.data_ptr() for o in (outs + outs32)[:5]])
    farr = (C.POINTER(sg.SavgolFilter) * 5)(*[fs[k % 3].ptr for k in range(5)])
    for count in (0, 5):
        assert F(farr, count, x.data_ptr(), ptrs, sg.SAVGOL_HIP_I16, ch, length, length, length, 0, None) == -1
        assert f"count {count} outside 1..4" in sg.last_error()
    for ot in (sg.SAVGOL_HIP_F16, sg.SAVGOL_HIP_BF16, 7):
        assert F(farr, 3, x.data_ptr(), ptrs, ot, ch, length, length, length, 0, None) == -1
        assert "is not served" in sg.last_error() and "savgol_apply_multi_batch_i16" in sg.last_error()
    torch.cuda.synchronize()
    assert all(untouched(torch, o) for o in outs + outs32)
    # in place and shifted overlaps with the input: the input is untouched
    before = x.clone()
    flat = x.view(-1)
    for target in (x, flat[1:], flat[length - 3:]):
        with pytest.raises(RuntimeError, match=r"d_outs\[1\] overlaps d_in"):
            sg.apply_multi_batch_i16(fs, x, [outs[0], target, outs[2]], ch - 1, length)
    # count 1 in place: refused in the call's own words, not handed on
    with pytest.raises(RuntimeError, match=r"d_outs\[0\] overlaps d_in"):
        sg.apply_multi_batch_i16(fs[:1], x, [x], ch, length)
    torch.cuda.synchronize()
    assert torch.equal(x, before) and all(untouched(torch, o) for o in outs)


# ------------------------------------------------------------------------------------------------
# 6. graph capture
# ------------------------------------------------------------------------------------------------
def test_multi_i16_graph_capture(sg, torch_gpu):
    """after one warm-up call with the same filters the call only enqueues: a count-3 call captures into a graph and replays to the eager bits"""
    torch = torch_gpu
    rng = np.random.default_rng(5700)
    for out_name, n in (("i16", 12), ("f32", 24)):
        x = torch.from_numpy(oracle_signal(rng, (8, 40000))).cuda()
        fs = [sg.Filter(n, 4, 0, 1.0, 0), sg.Filter(n, 4, 1, 1.0, 0), sg.Filter(n, 4, 2, 0.5, 0)]
        want = sg.apply_multi_tensor_i16(fs, x, out_dtype=tdtype(torch, out_name))          # the warm-up
        torch.cuda.synchronize()
        outs = [sentinel(torch, tdtype(torch, out_name), 8 * 40000).view(8, 40000) for _ in fs]
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        g = torch.cuda.CUDAGraph()
        with torch.cuda.stream(s):
            with torch.cuda.graph(g, stream=s):
                sg.apply_multi_batch_i16(fs, x, outs, 8, 40000, out_dtype=out_name, stream=s)
        g.replay()
        torch.cuda.synchronize()
        single = singles(sg, torch, fs, x, out_name, False, 0)
        for k in range(3):
            same(torch, outs[k], want[k].cpu(), ("graph", out_name, k, "eager"))
            same(torch, outs[k], single[k], ("graph", out_name, k, "single call"))
            assert not untouched(torch, outs[k][:, :1])


# ------------------------------------------------------------------------------------------------
# 7. many channels: the edge items' indexing (channel it / 2K, output (it % 2K) / 2, end it % 2) and the tile -> channel map
# ------------------------------------------------------------------------------------------------
def test_multi_i16_edge_items_across_many_channels(sg, torch_gpu):
    torch = torch_gpu
    rng = np.random.default_rng(5800)
    xh = torch.from_numpy(oracle_signal(rng, (100, 2 * TILE + 3)))
    for out_name, n, mix in (("i16", 5, (1, 0, 2)), ("f32", 21, (0, 1)), ("i16", 32, (1, 0, 3, 2))):
        fs = [sg.Filter(n, m, d, dt, 0) for m, d, dt in pool(n, 0)]                # POLYNOMIAL: 2 K edge items per channel
        got = run_multi(sg, torch, [fs[i] for i in mix], xh, out_name, out_pad=1)
        want = singles(sg, torch, fs, xh.cuda(), out_name, False, 0)
        for k, i in enumerate(mix):
            same(torch, got[k].contiguous(), want[i], (n, out_name, mix, k))
