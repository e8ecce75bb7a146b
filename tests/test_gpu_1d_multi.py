"""GPU tests of the fused multi-output 1-D call (savgol_apply[_valid]_multi_batch_f32, sg_k1d_multi.hpp): output k is bit-identical to the single
_ex call with SAVGOL_BATCH_PLAIN_SUMMATION (every half window, every boundary mode, VALID, mixed poly_order / time_step, unaligned rows and pitches,
CORRECT_LEADING_EDGE, offset-heavy signals, the routes that stay single calls) and within the fp32 bar of the fp64 oracle; refused calls launch nothing."""
import numpy as np
import pytest

from tests._util import check, fp32_bar, normwise, same_bits

pytestmark = pytest.mark.gpu

MODES = (0, 1, 2, 3)


@pytest.fixture(scope="module")
def torch_gpu(sg):
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    assert sg.device_count() > 0, sg.last_error()
    return torch


def signal(rng, shape, offset=0.0):
    t = np.arange(shape[-1], dtype=np.float64)
    return (offset + np.sin(0.013 * t) * 2.0 + 0.3 * np.sin(0.41 * t + 1.0) + rng.normal(0, 0.2, shape)).astype(np.float32)


def filter_sets(n):
    """(m = 4: d = 0, 1, 2), (m = 2: d = 0, 1) and a mixed poly_order / time_step set of four; poly_order capped below the window"""
    m4 = min(4, 2 * n)
    return [
        [(m4, 0, 1.0), (m4, 1, 1.0), (m4, 2, 1.0)],
        [(2, 0, 1.0), (2, 1, 1.0)],
        [(min(3, 2 * n), 1, 0.5), (2, 0, 1.0), (m4, 2, 0.25), (min(3, 2 * n), 0, 1.0)],
    ]


def alloc(torch, rows, ld, shift=0):
    """a [rows, ld] fp32 device view starting `shift` floats into its storage (unaligned rows when shift % 4 != 0), NaN-filled"""
    base = torch.full((rows * ld + shift + 8,), float("nan"), dtype=torch.float32, device="cuda")
    return base[shift:shift + rows * ld].view(rows, ld)


def fused(sg, filters, x, outs, channels, length, in_ld, out_ld, flags=0, valid=False):
    sg.apply_multi_batch(filters, x, outs, channels, length, in_ld, out_ld, flags=flags, valid=valid)


def single(sg, f, x, out, channels, length, in_ld, out_ld, flags=0, valid=False):
    f.apply_batch(x, out, channels, length, in_ld, out_ld, valid=valid, flags=flags | sg.SAVGOL_BATCH_PLAIN_SUMMATION)


def run_and_compare(sg, torch, filters, xh, flags=0, valid=False, in_shift=0, out_shifts=None, in_pad=0, out_pad=0):
    """fused call and the single calls on the same layout; returns the fused outputs (host, [channels, out_len])"""
    channels, length = xh.shape
    n = filters[0].n
    out_len = length - 2 * n if valid else length
    in_ld, out_ld = length + in_pad, out_len + out_pad
    x = alloc(torch, channels, in_ld, in_shift)
    x[:, :length] = torch.from_numpy(xh).cuda()
    shifts = out_shifts or [0] * len(filters)
    outs = [alloc(torch, channels, out_ld, s) for s in shifts]
    fused(sg, filters, x, outs, channels, length, in_ld, out_ld, flags, valid)
    ref = alloc(torch, channels, out_ld, shifts[0])
    got = []
    for k, f in enumerate(filters):
        ref.fill_(float("nan"))
        single(sg, f, x, ref, channels, length, in_ld, out_ld, flags, valid)
        torch.cuda.synchronize()
        a, b = outs[k][:, :out_len].cpu().numpy(), ref[:, :out_len].cpu().numpy()
        assert same_bits(a, b), (k, n, valid, flags, int(np.sum(a.view(np.uint32) != b.view(np.uint32))))
        if out_pad:                                                 # nothing written into the pitch padding
            assert torch.isnan(outs[k][:, out_len:]).all()
        got.append(a)
    return got


# ------------------------------------------------------------------------------------------------
# 1. bit identity with the single calls: N = 1..32, every boundary mode, full and VALID, count 2 / 3 / 4
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", range(1, 33))
def test_multi_bit_identical_to_single_calls(sg, torch_gpu, n):
    torch = torch_gpu
    rng = np.random.default_rng(100 + n)
    xh = signal(rng, (3, 70001))
    for fs in filter_sets(n):
        for mode in MODES:
            filters = [sg.Filter(n, m, d, dt, mode) for (m, d, dt) in fs]
            run_and_compare(sg, torch, filters, xh)
        run_and_compare(sg, torch, [sg.Filter(n, m, d, dt, 0) for (m, d, dt) in fs], xh, valid=True)


# ------------------------------------------------------------------------------------------------
# 2. against the fp64 oracle: every output within fp32_bar(the reference's own error)
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 2, 5, 8, 12, 16, 19, 24, 32])
def test_multi_against_fp64_oracle(sg, sgo, torch_gpu, n):
    torch = torch_gpu
    rng = np.random.default_rng(200 + n)
    xh = signal(rng, (2, 30011))
    x = torch.from_numpy(xh).cuda()
    for fs in filter_sets(n):
        for mode in MODES:
            filters = [sg.Filter(n, m, d, dt, mode) for (m, d, dt) in fs]
            ys = sg.apply_multi_tensor(filters, x)
            for (m, d, dt), y in zip(fs, ys):
                o = sgo.Filter(n, m, d, dt, mode)
                ref = o.apply_f64(xh.astype(np.float64))
                check(normwise(y.cpu().numpy(), ref), fp32_bar(normwise(o.apply(xh), ref)), (n, m, d, dt, mode))
        filters = [sg.Filter(n, m, d, dt, 0) for (m, d, dt) in fs]
        ys = sg.apply_multi_tensor(filters, x, valid=True)
        for (m, d, dt), y in zip(fs, ys):
            o = sgo.Filter(n, m, d, dt, 0)
            ref = o.apply_f64(xh.astype(np.float64))[:, n:-n]
            check(normwise(y.cpu().numpy(), ref), fp32_bar(normwise(o.apply(xh)[:, n:-n], ref)), (n, m, d, dt, "valid"))


# ------------------------------------------------------------------------------------------------
# 3. offset-heavy signals: smoothing on the raw tile, derivatives on the centred one, in one call
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [3, 8, 20, 32])
def test_multi_offset_signal(sg, sgo, torch_gpu, n):
    torch = torch_gpu
    rng = np.random.default_rng(300 + n)
    xh = signal(rng, (3, 50003), offset=1e3)
    for mode in MODES:
        filters = [sg.Filter(n, 4, d, 1.0, mode) for d in (0, 1, 2)]
        ys = run_and_compare(sg, torch, filters, xh)
        for d, y in zip((0, 1, 2), ys):
            o = sgo.Filter(n, 4, d, 1.0, mode)
            ref = o.apply_f64(xh.astype(np.float64))
            check(normwise(y, ref), fp32_bar(normwise(o.apply(xh), ref)), (n, d, mode, "offset 1e3"))


# ------------------------------------------------------------------------------------------------
# 4. unaligned input, outputs of different alignments, odd pitches; CORRECT_LEADING_EDGE on odd derivatives
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [2, 7, 16, 29])
def test_multi_unaligned_and_pitched(sg, torch_gpu, n):
    torch = torch_gpu
    rng = np.random.default_rng(400 + n)
    xh = signal(rng, (5, 9001))
    for mode in MODES:
        filters = [sg.Filter(n, 4, d, 0.5, mode) for d in (0, 1, 2)]
        run_and_compare(sg, torch, filters, xh, in_shift=1, out_shifts=[0, 1, 2], in_pad=3, out_pad=1)
        run_and_compare(sg, torch, filters, xh, in_shift=2, out_shifts=[3, 0, 0], in_pad=0, out_pad=4)
        run_and_compare(sg, torch, filters, xh, valid=True, in_shift=0, out_shifts=[1, 0, 3], in_pad=1, out_pad=2)
    filters = [sg.Filter(n, 4, d, 1.0, 0) for d in (1, 0, 3)]
    for flags in (sg.SAVGOL_BATCH_CORRECT_LEADING_EDGE, sg.SAVGOL_BATCH_CORRECT_LEADING_EDGE | sg.SAVGOL_BATCH_TILE_NARROW):
        ys = run_and_compare(sg, torch, filters, xh, flags=flags)
        # the leading edge of an odd derivative is negated against the reference's quirk: compare with the uncorrected call
        plain = run_and_compare(sg, torch, filters, xh)
        assert same_bits(ys[0][:, :n], -plain[0][:, :n]) and same_bits(ys[0][:, n:], plain[0][:, n:])
        assert same_bits(ys[1], plain[1])


# ------------------------------------------------------------------------------------------------
# 5. routes that stay single calls: reference summation (= the reference's bits), the wide tile for derivatives, channels beyond 2^30 samples
# ------------------------------------------------------------------------------------------------
def test_multi_reference_summation(sg, sgo, torch_gpu):
    torch = torch_gpu
    rng = np.random.default_rng(500)
    xh = signal(rng, (3, 20011))
    for n in (2, 5, 16, 32):
        for mode in MODES:
            filters = [sg.Filter(n, 4, d, 0.5, mode) for d in (0, 1, 2)]
            ys = run_and_compare(sg, torch, filters, xh, flags=sg.SAVGOL_BATCH_REFERENCE_SUMMATION)
            for d, y in zip((0, 1, 2), ys):
                assert same_bits(y, sgo.Filter(n, 4, d, 0.5, mode).apply(xh)), (n, mode, d)


def test_multi_wide_tile_route(sg, torch_gpu):
    """half windows <= 18 on batches of 16384 wide tiles: the single call's derivative outputs take the wide tile, the multi call keeps their bits"""
    torch = torch_gpu
    rng = np.random.default_rng(501)
    xh = signal(rng, (1100, 65536))
    for n in (5, 16):
        filters = [sg.Filter(n, 4, d, 1.0, 0) for d in (0, 1, 2)]
        run_and_compare(sg, torch, filters, xh)
        run_and_compare(sg, torch, filters, xh, flags=sg.SAVGOL_BATCH_TILE_NARROW)
        run_and_compare(sg, torch, filters[:2], xh[:4], flags=sg.SAVGOL_BATCH_TILE_WIDE)


def test_multi_long_channel_route(sg, torch_gpu):
    """one channel longer than 2^30 samples: the single calls' sub-row route, compared on the device"""
    torch = torch_gpu
    length = (1 << 30) + 4099
    free, _ = torch.cuda.mem_get_info()
    if free < 6 * 4 * length + (2 << 30):
        pytest.skip("not enough device memory for a 2^30-sample channel and four outputs")
    x = torch.empty((1, length), dtype=torch.float32, device="cuda")
    sg.synth(x)
    filters = [sg.Filter(9, 3, d, 1.0, mode) for d, mode in ((0, 0), (1, 0))]
    outs = [torch.empty_like(x) for _ in filters]
    sg.apply_multi_batch(filters, x, outs, 1, length)
    ref = torch.empty_like(x)
    for f, y in zip(filters, outs):
        single(sg, f, x, ref, 1, length, length, length)
        torch.cuda.synchronize()
        assert torch.equal(y.view(torch.int32), ref.view(torch.int32))
    del x, outs, ref
    torch.cuda.empty_cache()


# ------------------------------------------------------------------------------------------------
# 6. refusals on the device: no launch, targets unchanged
# ------------------------------------------------------------------------------------------------
def test_multi_refusals_launch_nothing(sg, torch_gpu):
    torch = torch_gpu
    channels, length = 4, 5000
    buf = torch.arange(6 * channels * length, dtype=torch.float32, device="cuda")
    before = buf.clone()
    x = buf[:channels * length].view(channels, length)
    o1 = buf[channels * length:2 * channels * length].view(channels, length)
    o2 = buf[2 * channels * length:3 * channels * length].view(channels, length)
    filters = [sg.Filter(8, 3, d) for d in (0, 1)]
    for outs, text in (([o1, o1], "overlap"), ([o1, x], "overlaps d_in"), ([buf[channels * length + 100:], o2], "d_outs[0] and d_outs[1] overlap"),
                       ([buf[10:], o2], "overlaps d_in")):
        with pytest.raises(RuntimeError, match=text.replace("[", r"\[").replace("]", r"\]")):
            sg.apply_multi_batch(filters, x, outs, channels, length)
    torch.cuda.synchronize()
    assert torch.equal(buf, before)


# ------------------------------------------------------------------------------------------------
# 7. full size: 4096 x 2^20, n = 32, m = 4, d = 0 / 1 / 2, POLYNOMIAL
# ------------------------------------------------------------------------------------------------
def test_multi_full_size(sg, sgo, torch_gpu):
    torch = torch_gpu
    channels, length = 4096, 1 << 20
    free, _ = torch.cuda.mem_get_info()
    if free < 5 * 4 * channels * length + (2 << 30):
        pytest.skip("not enough device memory for the headline shape and four outputs")
    x = torch.empty((channels, length), dtype=torch.float32, device="cuda")
    sg.synth(x)
    filters = [sg.Filter(32, 4, d, 1.0, 0) for d in (0, 1, 2)]
    ys = sg.apply_multi_tensor(filters, x)
    ref = torch.empty_like(x)
    rows = [0, channels // 2, channels - 1]
    xs = x[rows].cpu().numpy()
    for d, f, y in zip((0, 1, 2), filters, ys):
        single(sg, f, x, ref, channels, length, length, length)
        torch.cuda.synchronize()
        assert torch.equal(y.view(torch.int32), ref.view(torch.int32)), d
        o = sgo.Filter(32, 4, d, 1.0, 0)
        r64 = o.apply_f64(xs.astype(np.float64))
        got = y[rows].cpu().numpy()
        assert same_bits(got, ref[rows].cpu().numpy())
        check(normwise(got, r64), fp32_bar(normwise(o.apply(xs), r64)), ("headline", d))
    del x, ys, ref
    torch.cuda.empty_cache()


def test_multi_graph_capture(sg, torch_gpu):
    """after one warm-up call with the same filters the call only enqueues: it captures into a graph and replays to the same bits"""
    torch = torch_gpu
    rng = np.random.default_rng(700)
    x = torch.from_numpy(signal(rng, (8, 40000))).cuda()
    filters = [sg.Filter(12, 4, d, 1.0, 1) for d in (0, 1, 2)]
    want = sg.apply_multi_tensor(filters, x)
    outs = [torch.full_like(x, float("nan")) for _ in filters]
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(s):
        with torch.cuda.graph(g, stream=s):
            sg.apply_multi_batch(filters, x, outs, 8, 40000, stream=s)
    g.replay()
    torch.cuda.synchronize()
    for a, b in zip(outs, want):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))
