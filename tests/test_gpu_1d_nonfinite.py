"""GPU: the 1-D batch calls are held to the reference's NaN / Inf footprint.

The reference's loops skip no tap, so one non-finite sample makes non-finite exactly the outputs whose window, after the boundary remap, contains it (the
POLYNOMIAL edge rows: all of an end's n outputs when any of its 2n + 1 samples is special).  Every case below runs on the signals of tests/nonfinite_1d.py (a NaN
and a +-Inf staircase through every residue mod 64, the channel ends, every tile seam, two Infs in one window, a control channel) and is held to ONE rule,
hold(); expected values come from the oracle only:
  * sentinel      outputs live on a padded pitch in sentinel-filled storage with guards before and after: everything outside the stored outputs still holds it
                  (the input's pitch padding holds NaN: a kernel that read it would widen the footprint);
  * footprint     ~isfinite(got) == ~isfinite(oracle fp64 output), element for element;
  * NaN in        where a NaN input is in the window (the geometric rule), got is NaN;
  * kinds         tap-by-tap routes: isnan / isposinf / isneginf are the oracle's.  REFERENCE_SUMMATION: the three masks and the finite bits are those of the
                  oracle's fp32 restatement of the reference.  Block-moment routes (fp32 at n >= 20 by default, fp64 under rel_tol >= 1e-6 at n >= 24, the
                  16-bit calls on them): non-finite is the rule -- an Inf inside a group's common block makes every moment of the block Inf, and their
                  mixed-sign sum NaN (include/savgol_hip.h says so);
  * finite        check(normwise(got[fin], oracle[fin]), bar): the project's own bars -- fp32: fp32_bar(the reference's own fp32 error on the same outputs),
                  fp64: 1e-12, the tolerance call: 1e-6; fin covers at least 1 - MAX_SHARE of every channel's stored outputs.
Each route runs under the four boundary modes and VALID where it has a VALID form (the in-place and the strided calls have none), on the filters of
filter_sets(n) (tests/test_gpu_1d_h16.py): d = 0 / 1 / 2, so the centred derivative tiles (JOB_CENTRE) run at every half window."""
import ctypes as C

import numpy as np
import pytest

from tests import nonfinite_1d as nf
from tests._util import check, fp32_bar, normwise, same_bits
from tests.test_gpu_1d_h16 import filter_sets
from tests.test_nonfinite_1d_rule import HALF_WINDOWS

pytestmark = pytest.mark.gpu

GUARD = 8
# layout: (floats the input base is off a 16-byte boundary, input pitch, the same for the output)
LAYOUTS = {"aligned": (0, nf.LENGTH + 3, 0, nf.LENGTH + 3), "ragged": (1, nf.LENGTH + 2, 1, nf.LENGTH + 4)}
TOL_F64, TOL_CALL = 1e-12, 1e-6
STATS = {"calls": 0, "channels": 0, "specials": 0, "share": 0.0}


def halves(*ns):
    """the half windows of a route; tests/test_nonfinite_1d_rule.py (CPU) holds the signals of exactly these to the oracle"""
    assert set(ns) <= set(HALF_WINDOWS), sorted(set(ns) - set(HALF_WINDOWS))
    return list(ns)


@pytest.fixture(scope="module")
def torch_gpu(sg):
    import torch
    assert torch.cuda.is_available() and sg.device_count() > 0, sg.last_error()
    return torch


def where(mask):
    idx = np.argwhere(mask)
    return f"{len(idx)} outputs, first (channel, sample) {idx[:4].tolist()}"


def kinds_equal(got, want, sel, label, whose):
    for name, cls in (("NaN", np.isnan), ("+Inf", np.isposinf), ("-Inf", np.isneginf)):
        diff = (cls(got) != cls(want)) & sel
        assert not diff.any(), (label, f"{name} positions differ from {whose}: " + where(diff))


def hold(got, x, o, mode, label, kinds, bar="fp32"):
    """the rule, on every channel of the batch.  got [channels][length]: the call's outputs in the coordinates of the input; x: what the call's arithmetic saw;
    o: the oracle's filter; kinds: "exact" | "nonfinite" | "reference"; bar: "fp32" or a number"""
    n = o.n
    sel = np.broadcast_to(nf.stored(x.shape[1], n, mode)[None, :], x.shape)
    fp_hi, hi = nf.oracle_footprint(o, x, mode)
    fp_got = ~np.isfinite(got) & sel
    per_channel = fp_hi.sum(axis=1) / sel.sum(axis=1)
    STATS["share"] = max(STATS["share"], float(per_channel.max()))
    assert per_channel.max() <= nf.MAX_SHARE and per_channel[-1] == 0.0, (label, "a channel is too full of specials", per_channel)
    assert (fp_got & ~fp_hi).sum() == 0, (label, "non-finite where the window holds no special: " + where(fp_got & ~fp_hi))
    assert (fp_hi & ~fp_got).sum() == 0, (label, "finite where the window holds a special: " + where(fp_hi & ~fp_got))
    nan_fp = nf.footprint(np.isnan(x), n, mode)
    assert (nan_fp & ~np.isnan(got)).sum() == 0, (label, "a NaN in the window is not a NaN out: " + where(nan_fp & ~np.isnan(got)))
    fin = sel & ~fp_hi
    assert (fin.sum(axis=1) >= (1.0 - nf.MAX_SHARE) * sel.sum(axis=1)).all(), label
    ref32 = None
    if kinds == "reference" or bar == "fp32":
        ref32 = o.apply(np.ascontiguousarray(x, np.float32), nf.POLYNOMIAL if mode == nf.VALID else mode)
    if kinds == "exact":
        kinds_equal(got, hi, sel, label, "the oracle's")
    elif kinds == "reference":
        kinds_equal(got, ref32, sel, label, "the reference's")
        assert same_bits(got[fin], ref32[fin]), (label, "finite outputs are not the reference's bits: " + where((got != ref32) & fin))
    else:
        assert kinds == "nonfinite", kinds
    limit = fp32_bar(normwise(ref32[fin], hi[fin])) if bar == "fp32" else bar
    check(normwise(got[fin], hi[fin]), limit, label)
    STATS["calls"] += 1
    STATS["channels"] += x.shape[0]
    STATS["specials"] += int((~np.isfinite(x)).sum())


def rows(torch, host, channels, pitch, shift, fill, tdt):
    """[channels][pitch] rows `shift` elements off a 16-byte boundary inside storage filled with `fill`, GUARD elements before and after; host [channels][len]
    (or None) goes into the head of the rows.  Returns (the whole storage, the rows)"""
    flat = torch.full((GUARD + shift + channels * pitch + GUARD,), fill, dtype=tdt, device="cuda")
    view = flat[GUARD + shift:GUARD + shift + channels * pitch].view(channels, pitch)
    assert view.data_ptr() % 16 == (shift * flat.element_size()) % 16
    if host is not None:
        view[:, :host.shape[1]] = torch.from_numpy(np.ascontiguousarray(host)).cuda()
    return flat, view


def unpack(flat, channels, length, n, pitch, shift, mode, label, dtype):
    """the stored outputs of a sentinel-filled storage in the coordinates of the input; everything else must still hold the sentinel"""
    host = flat.cpu().numpy()
    body = host[GUARD + shift:GUARD + shift + channels * pitch].reshape(channels, pitch)
    out_len = length - 2 * n if mode == nf.VALID else length
    assert np.all(host[:GUARD + shift] == nf.SENTINEL) and np.all(host[GUARD + shift + channels * pitch:] == nf.SENTINEL), (label, "a guard was written")
    assert np.all(body[:, out_len:] == nf.SENTINEL), (label, "written past the stored outputs: " + where(body[:, out_len:] != nf.SENTINEL))
    got = np.full((channels, length), nf.SENTINEL, dtype)
    if mode == nf.VALID:
        got[:, n:length - n] = body[:, :out_len]
    else:
        got[:] = body[:, :length]
    return got


def moment_terms(sg, f, dtype):
    """block moments the kernel of this filter uses on the fp32 default route / the fp64 tolerance route (0: tap by tap) -- the library's own diagnostic"""
    if dtype == "f32":
        return sg.lib().savgol_hip_momenth_table(f.ptr, (C.c_float * 400)())
    return sg.lib().savgol_hip_moment64_table(f.ptr, (C.c_double * 278)())


def run_single(sg, sgo, torch, n, filt, mode, dtype="f32", flags=None, rel_tol=None, layout="aligned", in_place=False, route=""):
    m, d, dt = filt
    x = nf.signals_for(n)[0]
    channels, length = x.shape
    tdt, ndt = (torch.float32, np.float32) if dtype == "f32" else (torch.float64, np.float64)
    boundary = nf.POLYNOMIAL if mode == nf.VALID else mode
    f, o = sg.Filter(n, m, d, dt, boundary), sgo.Filter(n, m, d, dt, boundary)
    in_shift, in_ld, out_shift, out_ld = LAYOUTS[layout]
    label = (route, dtype, n, filt, mode, flags, rel_tol, layout)
    if in_place:
        out_flat, d_in = rows(torch, x.astype(ndt), channels, in_ld, in_shift, nf.SENTINEL, tdt)
        d_out, out_shift, out_ld = d_in, in_shift, in_ld
    else:
        _, d_in = rows(torch, x.astype(ndt), channels, in_ld, in_shift, float("nan"), tdt)
        out_flat, d_out = rows(torch, None, channels, out_ld, out_shift, nf.SENTINEL, tdt)
    f.apply_batch(d_in, d_out, channels, length, in_ld, out_ld, dtype=dtype, valid=mode == nf.VALID, flags=flags, rel_tol=rel_tol)
    torch.cuda.synchronize()
    got = unpack(out_flat, channels, length, n, out_ld, out_shift, mode, label, ndt)
    # which rule for the kinds: restated here from the header's text (SAVGOL_HIP_OPT_PLAIN_SUMMATION, savgol_apply_batch_f64_tol).  The weaker rule is only
    # taken where the library's own diagnostic has a block-moment table for the filter as well
    if dtype == "f32":
        tap_by_tap = bool(n < 20 or m < 2 or d > 1 or (flags is not None and flags & (sg.SAVGOL_BATCH_PLAIN_SUMMATION | sg.SAVGOL_BATCH_REFERENCE_SUMMATION)))
        bar = "fp32"
    else:
        tap_by_tap = rel_tol is None or n < 24
        bar = TOL_F64 if rel_tol is None else TOL_CALL
    assert tap_by_tap or moment_terms(sg, f, dtype) > 0, label
    reference = flags is not None and flags & sg.SAVGOL_BATCH_REFERENCE_SUMMATION
    hold(got, x, o, mode, label, "reference" if reference else "exact" if tap_by_tap else "nonfinite", bar)
    f.close()


def every(sg, sgo, torch, n, modes=nf.MODES, **call):
    for filt in filter_sets(n):
        for mode in modes:
            run_single(sg, sgo, torch, n, filt, mode, **call)


# ---- fp32, the default call: tap by tap below 20, the block-moment kernel from 20 on (d = 2 stays tap by tap there) ----
@pytest.mark.parametrize("n", halves(1, 3, 4, 9, 13, 18, 19, 20, 21, 24, 27, 31, 32))
def test_fp32_default(sg, sgo, torch_gpu, n):
    every(sg, sgo, torch_gpu, n, route="default")


@pytest.mark.parametrize("n", halves(4, 20, 32))
def test_fp32_plain_summation(sg, sgo, torch_gpu, n):
    every(sg, sgo, torch_gpu, n, flags=sg.SAVGOL_BATCH_PLAIN_SUMMATION, route="plain")


@pytest.mark.parametrize("n", halves(4, 20, 32))
def test_fp32_reference_summation(sg, sgo, torch_gpu, n):
    every(sg, sgo, torch_gpu, n, flags=sg.SAVGOL_BATCH_REFERENCE_SUMMATION, route="reference")


@pytest.mark.parametrize("width", ["narrow", "wide"])
@pytest.mark.parametrize("n", halves(1, 12, 13, 18))
def test_fp32_tile_widths(sg, sgo, torch_gpu, n, width):
    every(sg, sgo, torch_gpu, n, flags=sg.SAVGOL_BATCH_TILE_NARROW if width == "narrow" else sg.SAVGOL_BATCH_TILE_WIDE, route=width)


@pytest.mark.parametrize("n", halves(5, 20, 32))
def test_fp32_ragged_layout(sg, sgo, torch_gpu, n):
    """base one float off 16 bytes, pitch != length, input and output: the scalar staging and store paths"""
    every(sg, sgo, torch_gpu, n, layout="ragged", route="ragged")


# ---- fp64: the default (tap by tap, 1e-12), the tolerance call (block moments from 24 on, 1e-6), the wide tile ----
@pytest.mark.parametrize("n", halves(3, 16, 24, 27, 32))
def test_fp64_default(sg, sgo, torch_gpu, n):
    every(sg, sgo, torch_gpu, n, dtype="f64", route="default")


@pytest.mark.parametrize("n", halves(24, 27, 32))
def test_fp64_tolerance_call(sg, sgo, torch_gpu, n):
    every(sg, sgo, torch_gpu, n, dtype="f64", rel_tol=1e-6, route="tolerance")


@pytest.mark.parametrize("n", halves(3, 16, 24))
def test_fp64_wide_tile(sg, sgo, torch_gpu, n):
    every(sg, sgo, torch_gpu, n, dtype="f64", flags=sg.SAVGOL_BATCH_TILE_WIDE, route="wide")


# ---- in place (d_out == d_in, the full-length entry points): the specials sit in the stashed halos and channel ends too ----
IN_PLACE = [("f32", n, None) for n in halves(5, 20, 32)] + [("f64", n, None) for n in halves(16, 32)] + [("f64", n, 1e-6) for n in halves(16, 32)]


@pytest.mark.parametrize("dtype,n,rel_tol", IN_PLACE)
def test_in_place(sg, sgo, torch_gpu, dtype, n, rel_tol):
    every(sg, sgo, torch_gpu, n, modes=nf.MODES[:4], dtype=dtype, rel_tol=rel_tol, in_place=True, route="in place")


# ---- the fused multi-output call: three outputs (d = 0, 1, 2) from one read, each under the rule of its own filter; tap by tap (the single PLAIN call's bits) ----
@pytest.mark.parametrize("mode", nf.MODES)
@pytest.mark.parametrize("n", halves(4, 16, 32))
def test_fused_multi_output(sg, sgo, torch_gpu, n, mode):
    torch = torch_gpu
    x = nf.signals_for(n)[0]
    channels, length = x.shape
    boundary = nf.POLYNOMIAL if mode == nf.VALID else mode
    sets = filter_sets(n)[:3]
    assert [d for _, d, _ in sets] == [0, 1, 2]
    fs = [sg.Filter(n, m, d, dt, boundary) for m, d, dt in sets]
    in_shift, in_ld, out_shift, out_ld = LAYOUTS["aligned"]
    _, d_in = rows(torch, x, channels, in_ld, in_shift, float("nan"), torch.float32)
    outs = [rows(torch, None, channels, out_ld, out_shift, nf.SENTINEL, torch.float32) for _ in fs]
    sg.apply_multi_batch(fs, d_in, [view for _, view in outs], channels, length, in_ld, out_ld, flags=0, valid=mode == nf.VALID)
    torch.cuda.synchronize()
    for (m, d, dt), (flat, _) in zip(sets, outs):
        label = ("fused", n, (m, d, dt), mode)
        hold(unpack(flat, channels, length, n, out_ld, out_shift, mode, label, np.float32), x, sgo.Filter(n, m, d, dt, boundary), mode, label, "exact")


# ---- the strided calls on 16-byte records: POLYNOMIAL edges whatever config.boundary says, the configured mode under BOUNDARY_AWARE ----
def records(torch, x, seed):
    """[channels][length][4] records in sentinel-guarded storage: the signal in field 1, finite noise in the others.  Returns (host copy, storage, records)"""
    channels, length = x.shape
    aos = np.random.default_rng(seed).normal(0, 1, (channels, length, 4)).astype(np.float32)
    aos[:, :, 1] = x
    flat = torch.full((GUARD + aos.size + GUARD,), nf.SENTINEL, dtype=torch.float32, device="cuda")
    view = flat[GUARD:GUARD + aos.size].view(aos.shape)
    view.copy_(torch.from_numpy(aos))
    return aos, flat, view


def records_back(flat, aos, written, label):
    host = flat.cpu().numpy()
    assert np.all(host[:GUARD] == nf.SENTINEL) and np.all(host[GUARD + aos.size:] == nf.SENTINEL), (label, "a guard was written")
    got = host[GUARD:GUARD + aos.size].reshape(aos.shape)
    keep = [k for k in range(4) if k not in written]
    assert same_bits(got[:, :, keep], aos[:, :, keep]), (label, "a field no job writes has changed")
    return got


@pytest.mark.parametrize("aware", [False, True])
@pytest.mark.parametrize("n", halves(5, 32))
def test_strided_call(sg, sgo, torch_gpu, n, aware):
    torch = torch_gpu
    x = nf.signals_for(n)[0]
    channels, length = x.shape
    flags = sg.SAVGOL_BATCH_BOUNDARY_AWARE if aware else 0
    for m, d, dt in filter_sets(n):
        for mode in nf.MODES[:4]:
            aos, flat, view = records(torch, x, 5 * n + mode)
            f = sg.Filter(n, m, d, dt, mode)
            assert sg.lib().savgol_apply_strided_batch_f32_ex(f.ptr, view.data_ptr(), 16, 4, length * 16, view.data_ptr(), 16, 12, length * 16, channels, length,
                                                              flags, None) == 0, sg.last_error()
            torch.cuda.synchronize()
            label = ("strided", n, (m, d, dt), mode, aware)
            got = records_back(flat, aos, (3,), label)
            served = mode if aware else nf.POLYNOMIAL                    # the reference's savgol_apply_strided ignores config.boundary
            hold(np.ascontiguousarray(got[:, :, 3]), x, sgo.Filter(n, m, d, dt, served), served, label, "exact")
            f.close()


@pytest.mark.parametrize("aware", [False, True])
@pytest.mark.parametrize("n", halves(5, 32))
def test_strided_multi_field_call(sg, sgo, torch_gpu, n, aware):
    """three fields from one pass over the records (one fused launch): value, first and second derivative of field 1 into fields 3, 0 and 2"""
    torch = torch_gpu
    x = nf.signals_for(n)[0]
    channels, length = x.shape
    flags = sg.SAVGOL_BATCH_BOUNDARY_AWARE if aware else 0
    sets = filter_sets(n)[:3]
    for mode in nf.MODES[:4]:
        aos, flat, view = records(torch, x, 7 * n + mode)
        fs = [sg.Filter(n, m, d, dt, mode) for m, d, dt in sets]
        jobs = [(fs[0], 4, 12), (fs[1], 4, 0), (fs[2], 4, 8)]
        assert sg.apply_strided_multi_batch_route(jobs, view, 16, length * 16, view, 16, length * 16, channels, length, flags=flags) == 1, sg.last_error()
        sg.apply_strided_multi_batch(jobs, view, 16, length * 16, view, 16, length * 16, channels, length, flags=flags)
        torch.cuda.synchronize()
        got = records_back(flat, aos, (3, 0, 2), ("strided multi", n, mode, aware))
        served = mode if aware else nf.POLYNOMIAL
        for (m, d, dt), field in zip(sets, (3, 0, 2)):
            hold(np.ascontiguousarray(got[:, :, field]), x, sgo.Filter(n, m, d, dt, served), served, ("strided multi", n, (m, d, dt), mode, aware), "exact")


# ---- 16-bit storage: the fp32 call's NaN mask and bits (their own run_case; that fp32 call is held to the oracle on the same signal above), and the
# ---- oracle's footprint on the widened input directly ----
def widened_footprint(torch, out, wide, o, mode, label):
    got = np.full(wide.shape, nf.SENTINEL, np.float32)
    host = out.float().cpu().numpy()                                    # widening is exact and keeps every class
    if mode == nf.VALID:
        got[:, o.n:wide.shape[1] - o.n] = host
    else:
        got[:] = host
    sel = nf.stored(wide.shape[1], o.n, mode)[None, :]
    fp_hi, _ = nf.oracle_footprint(o, wide, mode)
    fp_got = ~np.isfinite(got) & sel
    assert (fp_got & ~fp_hi).sum() == 0, (label, "non-finite where the window holds no special: " + where(fp_got & ~fp_hi))
    assert (fp_hi & ~fp_got).sum() == 0, (label, "finite where the window holds a special: " + where(fp_hi & ~fp_got))
    nan_fp = nf.footprint(np.isnan(wide), o.n, mode)
    assert (nan_fp & ~np.isnan(got)).sum() == 0, (label, "a NaN in the window is not a NaN out: " + where(nan_fp & ~np.isnan(got)))
    STATS["share"] = max(STATS["share"], float((fp_hi.sum(axis=1) / sel.sum()).max()))
    STATS["calls"] += 1
    STATS["channels"] += wide.shape[0]
    STATS["specials"] += int((~np.isfinite(wide)).sum())


def quantised(torch, x, name):
    """(host tensor of the 16-bit type, the widened fp32 array the call's arithmetic sees): values of a few units, nothing overflows either type"""
    from tests.test_gpu_1d_h16 import host16
    x16 = host16(torch, x, name)
    wide = x16.float().numpy()
    assert np.array_equal(np.isnan(wide), np.isnan(x)) and np.array_equal(np.isposinf(wide), np.isposinf(x)) and np.array_equal(np.isneginf(wide), np.isneginf(x))
    return x16, wide


@pytest.mark.parametrize("pair", [("f16", "f16"), ("bf16", "bf16"), ("f16", "f32"), ("bf16", "f32")])
@pytest.mark.parametrize("n", halves(20, 32))
def test_h16_single_call(sg, sgo, torch_gpu, n, pair):
    from tests.test_gpu_1d_h16 import run_case
    torch = torch_gpu
    x16, wide = quantised(torch, nf.signals_for(n)[0], pair[0])
    for m, d, dt in filter_sets(n):
        for mode in nf.MODES:
            boundary = nf.POLYNOMIAL if mode == nf.VALID else mode
            out, _ = run_case(sg, torch, sg.Filter(n, m, d, dt, boundary), x16, pair, valid=mode == nf.VALID, in_pad=3, out_pad=3)
            widened_footprint(torch, out, wide, sgo.Filter(n, m, d, dt, boundary), mode, ("h16", n, pair, (m, d, dt), mode))


@pytest.mark.parametrize("pair", [("f16", "f16"), ("bf16", "bf16"), ("f16", "f32"), ("bf16", "f32")])
@pytest.mark.parametrize("n", halves(20, 32))
def test_h16_fused_call(sg, sgo, torch_gpu, n, pair):
    from tests.test_gpu_1d_multi_h16 import rounded_fp32_multi, run_multi, same_bits as same_bits_h16
    torch = torch_gpu
    x16, wide = quantised(torch, nf.signals_for(n)[0], pair[0])
    sets = filter_sets(n)[:3]
    for mode in nf.MODES:
        boundary = nf.POLYNOMIAL if mode == nf.VALID else mode
        fs = [sg.Filter(n, m, d, dt, boundary) for m, d, dt in sets]
        outs = run_multi(sg, torch, fs, x16, pair, valid=mode == nf.VALID, in_pad=3, out_pad=3)
        want = rounded_fp32_multi(sg, torch, fs, x16.cuda(), pair, mode == nf.VALID, 0)
        for k, (m, d, dt) in enumerate(sets):
            label = ("fused h16", n, pair, (m, d, dt), mode)
            same_bits_h16(torch, outs[k].contiguous(), want[k], label)
            widened_footprint(torch, outs[k], wide, sgo.Filter(n, m, d, dt, boundary), mode, label)


def test_report(torch_gpu):
    """how much the cases above looked at (runs last in this file)"""
    print(f"\n1-D non-finite rule: {STATS['calls']} calls, {STATS['channels']} channels and {STATS['specials']} special samples checked, "
          f"largest non-finite share of a channel's stored outputs {100 * STATS['share']:.1f} %")
    assert STATS["share"] <= nf.MAX_SHARE
