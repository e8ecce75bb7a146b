"""GPU: the 2-D calls are held to the reference's NaN / Inf footprint.

The reference's dense loop skips no tap (src/savgol2d.c:374-393), so one non-finite pixel makes non-finite exactly the outputs whose window, after the border
remap, contains it.  Every case below runs on the frames of tests/nonfinite_2d.py (a staircase of specials through every row phase and column position, the
frame's corners and borders, a strip seam, two opposite Infs in one window) and is held to ONE rule, hold(); expected values come from the oracle only:
  * sentinel      pixels outside the stored region still hold the sentinel;
  * footprint     ~isfinite(got) == ~isfinite(oracle fp64 frame) inside it, element for element;
  * NaN pixels    where a NaN input is in the window, got is NaN;
  * finite pixels check(normwise(got, hi), bar2d(...)) over the finite pixels: the project's one parity rule (tests/test_gpu_2d.py, tests/_util.py), no new tolerance;
  * method 1      keeps the reference's order: isnan / isposinf / isneginf are those of the oracle's fp32 restatement, the finite pixels its bits;
  * rectangular windows on methods 0 / 2 (the header's caveat: zero-padded factors): the footprint contains the rectangular window's and lies inside the
    square window's of the larger half;
  * the sign of an Inf on the separable kernels is not asserted (two terms may meet as Inf - Inf): non-finite is the rule there."""
import threading
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

from tests import nonfinite_2d as nf
from tests._util import check, fp32_bar, normwise, same_bits
from tests.test_gpu_2d import bar2d

pytestmark = pytest.mark.gpu
MODES = [nf.VALID, nf.CONSTANT, nf.REFLECT]
KINDS = ["aligned", "ragged"]
DELTA = (0.5, 2.0)
FUSED_DELTA = (0.5, 0.25)                                       # the fused calls: the steps of test_fused_gradient_hessian_laplacian_batch (tests/test_gpu_2d.py)
STATS = {"calls": 0, "frames": 0, "specials": 0, "share": 0.0}
_STATS_LOCK = threading.Lock()
_DEVICE = {}


class _Pool:
    """the oracle runs outside the interpreter lock: one frame per thread.  Made at first use (never at collection), shut down by the file's last test"""
    pool = None

    @classmethod
    def map(cls, fn, items):
        if cls.pool is None:
            cls.pool = ThreadPoolExecutor(8)
        return cls.pool.map(fn, items)

    @classmethod
    def close(cls):
        if cls.pool is not None:
            cls.pool.shutdown()
            cls.pool = None


_POOL = _Pool


@pytest.fixture(scope="module")
def torch_gpu(sg):
    import torch
    assert torch.cuda.is_available() and sg.device_count() > 0, sg.last_error()
    return torch


def on_device(torch, kind, n):
    """the frames of (kind, n) on the device, uploaded once: (host frames, cols, shift, device view [B][rows][stride])"""
    key = (kind, n)
    if key not in _DEVICE:
        x, cols, shift, count, _ = nf.frames_for(kind, n)
        flat = torch.zeros(x.size + 8, dtype=torch.float32, device="cuda")
        view = flat[shift:shift + x.size].view(x.shape)
        view.copy_(torch.from_numpy(np.array(x)))
        assert view.data_ptr() % 16 == 4 * shift
        _DEVICE[key] = (x, cols, shift, view, count)
    return _DEVICE[key]


def fresh(torch, shape, shift):
    """an output stack pre-filled with the sentinel, its base `shift` floats off a 16-byte boundary"""
    size = int(np.prod(shape))
    flat = torch.full((size + 8,), nf.SENTINEL, dtype=torch.float32, device="cuda")
    return flat[shift:shift + size].view(shape)


def where(mask):
    idx = np.argwhere(mask)
    return f"{len(idx)} pixels, first (row, column) {idx[:4].tolist()}"


def hold(got, x, cols, o, b, label, reference_order=False, square=0, hi=None, bar=None):
    """the rule, on every frame of the batch.  got [B][rows][stride]: the call's frames (fp32 on the host); o: the oracle's filter; hi: the expected fp64 frames
    when they are not o's own (the Laplacian); bar(k, fin): the finite pixels' bar when it is not bar2d's; square: the larger half of a rectangular window"""
    rows, stride = x.shape[1:]
    sel = nf.stored(rows, cols, stride, o.nx, o.ny, b)
    frames = range(x.shape[0])
    if hi is None:
        hi = list(_POOL.map(lambda k: o.apply_f64acc(x[k], cols, b), frames))

    def one(k):
        g, h = got[k], hi[k]
        assert np.all(g[~sel] == nf.SENTINEL), (label, k, "written outside the stored region: " + where((g != nf.SENTINEL) & ~sel))
        fp_got, fp_hi = ~np.isfinite(g) & sel, ~np.isfinite(h) & sel
        with _STATS_LOCK:
            STATS["share"] = max(STATS["share"], fp_hi.sum() / sel.sum())
        assert fp_hi.sum() <= nf.MAX_SHARE * sel.sum(), (label, k, "the frame is too full of specials")
        if not square:
            assert (fp_got & ~fp_hi).sum() == 0, (label, k, "non-finite where the window holds no special: " + where(fp_got & ~fp_hi))
            assert (fp_hi & ~fp_got).sum() == 0, (label, k, "finite where the window holds a special: " + where(fp_hi & ~fp_got))
        else:
            outer = nf.footprint(~np.isfinite(x[k]), cols, square, square, b) if b else nf.footprint(~np.isfinite(x[k]), cols, square, square, nf.CONSTANT) & sel
            assert (fp_hi & ~fp_got).sum() == 0, (label, k, "finite where the rectangular window holds a special: " + where(fp_hi & ~fp_got))
            assert (fp_got & ~outer).sum() == 0, (label, k, "non-finite outside the square window: " + where(fp_got & ~outer))
        nan_fp = nf.footprint(np.isnan(x[k]), cols, o.nx, o.ny, b)
        assert (nan_fp & ~np.isnan(g)).sum() == 0, (label, k, "a NaN in the window is not a NaN out: " + where(nan_fp & ~np.isnan(g)))
        fin = sel & ~fp_got & ~fp_hi
        assert fin.sum() >= (1.0 - nf.MAX_SHARE) * sel.sum() * (0.5 if square else 1.0)
        if reference_order:
            ref32 = o.apply(x[k], cols, b, out=np.full((rows, stride), nf.SENTINEL, np.float32))
            for name, cls in (("NaN", np.isnan), ("+Inf", np.isposinf), ("-Inf", np.isneginf)):
                assert np.array_equal(cls(g) & sel, cls(ref32) & sel), (label, k, name + " positions differ from the reference's: " + where((cls(g) != cls(ref32)) & sel))
            assert same_bits(g[fin], ref32[fin]), (label, k, "finite pixels are not the reference's bits")
        value = normwise(g[fin], h[fin])
        limit = bar2d(o, x[k], cols, b, h, fin) if bar is None else bar(k, fin)
        return value, limit

    results = list(_POOL.map(one, frames))
    for k, (value, limit) in enumerate(results):
        check(value, limit, (label, k))
    STATS["calls"] += 1
    STATS["frames"] += x.shape[0]
    STATS["specials"] += int((~np.isfinite(x)).sum())


def run_filter(sg, sgo, torch, kind, filt, b, method, label, **rule):
    nx, ny, order, dx, dy = filt
    x, cols, shift, d, _ = on_device(torch, kind, max(nx, ny))
    images, rows, stride = x.shape
    f = sg.Filter2D(nx, ny, order, dx, dy, *DELTA)
    o = sgo.Filter2D(nx, ny, order, dx, dy, *DELTA)
    got = fresh(torch, x.shape, shift)
    f.apply_batch(d, got, rows, cols, images, in_stride=stride, out_stride=stride, boundary=b, method=method)
    torch.cuda.synchronize()
    hold(got.cpu().numpy(), x, cols, o, b, (label, kind, filt, b, method), **rule)
    f.close()


def low(n, order=3):
    """order 3, or order 2 where order 3 exceeds 2n (as the existing kernel tests choose)"""
    return order if order <= 2 * n else 2


# ---- method 2, smoothing: the additive form (order <= 3) and the general two-term form (order 4) ----
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("b", MODES)
@pytest.mark.parametrize("n", range(1, 17))
def test_method2_smoothing(sg, sgo, torch_gpu, n, b, kind):
    run_filter(sg, sgo, torch_gpu, kind, (n, n, low(n), 0, 0), b, 2, "additive")
    if n >= 2:
        run_filter(sg, sgo, torch_gpu, kind, (n, n, 4, 0, 0), b, 2, "order 4")


# ---- method 2, derivative frames: one-term tiles / the walk at n = 15, 16; sg_2d_hf.hip (one launch, and the accumulating second); y-dominant; mixed ----
DERIVATIVES = [("gx", 3, 1, 0), ("gy", 3, 0, 1), ("xx2", 2, 2, 0), ("xx4", 4, 2, 0), ("yy", 3, 0, 2), ("xy", 3, 1, 1)]


# (a window of 2n + 1 samples has no order above 2n: order 3 becomes 2 at n = 1, as in the existing kernel tests, and order 4 does not exist there)
DERIVATIVE_CASES = [(n, name, low(n, order) if order == 3 else order, dx, dy) for n in range(1, 17) for name, order, dx, dy in DERIVATIVES if order != 4 or n >= 2]


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("b", MODES)
@pytest.mark.parametrize("n,name,order,dx,dy", DERIVATIVE_CASES)
def test_method2_derivative_frames(sg, sgo, torch_gpu, n, name, order, dx, dy, b, kind):
    run_filter(sg, sgo, torch_gpu, kind, (n, n, order, dx, dy), b, 2, name)


# ---- method 3: the tile kernel, plain and on centred samples (SepPlan.centre) ----
# (d = (1,2) needs order 3, which a window of three samples does not have: no such case at n = 1)
TILE_CASES = [(n, dx, dy) for n in (1, 2, 5, 7, 8, 12, 16) for dx, dy in ((0, 0), (2, 0), (0, 2), (1, 2)) if dx + dy <= low(n)]


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("b", MODES)
@pytest.mark.parametrize("n,dx,dy", TILE_CASES)
def test_method3_tile_kernel(sg, sgo, torch_gpu, n, dx, dy, b, kind):
    run_filter(sg, sgo, torch_gpu, kind, (n, n, low(n), dx, dy), b, 3, "tile kernel")


# ---- method 1: the reference's order, so the reference's NaN / +Inf / -Inf positions and bits ----
@pytest.mark.parametrize("b", MODES)
@pytest.mark.parametrize("dx,dy", [(0, 0), (1, 0)])
@pytest.mark.parametrize("nx,ny", [(1, 1), (4, 4), (8, 8), (4, 6), (12, 5)])
def test_method1_reference_order(sg, sgo, torch_gpu, nx, ny, dx, dy, b):
    run_filter(sg, sgo, torch_gpu, "ragged", (nx, ny, low(min(nx, ny)), dx, dy), b, 1, "dense", reference_order=True)


# ---- rectangular windows on method 2: zero-padded factors, the header's caveat, held from both sides ----
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("b", MODES)
@pytest.mark.parametrize("nx,ny", [(4, 7), (7, 4), (12, 2)])
def test_method2_rectangular_windows(sg, sgo, torch_gpu, nx, ny, b, kind):
    run_filter(sg, sgo, torch_gpu, kind, (nx, ny, 3, 0, 0), b, 2, "rectangular", square=max(nx, ny))


# ---- the fused device calls: every frame written under the rule of its own (dx, dy) filter ----
@pytest.mark.parametrize("b", MODES)
@pytest.mark.parametrize("n", [2, 7, 9])
def test_fused_gradient_hessian_laplacian(sg, sgo, torch_gpu, n, b):
    """Sampling steps FUSED_DELTA.  With this file's other steps, (0.5, 2.0), the Laplacian is x-dominant and its finite pixels miss the parity bar: ADVICE.md."""
    torch = torch_gpu
    DELTA = FUSED_DELTA
    x, cols, shift, d, _ = on_device(torch, "aligned", n)
    images, rows, stride = x.shape
    pitch = rows * stride
    L = sg.lib()
    outs = {name: fresh(torch, x.shape, shift) for name in ("gx", "gy", "xx", "xy", "yy", "lap")}
    assert L.savgol2d_gradient_batch_f32(n, n, 3, d.data_ptr(), rows, cols, stride, pitch, outs["gx"].data_ptr(), outs["gy"].data_ptr(), stride, pitch, images,
                                         *DELTA, b, None) == 0, sg.last_error()
    assert L.savgol2d_hessian_batch_f32(n, n, 3, d.data_ptr(), rows, cols, stride, pitch, outs["xx"].data_ptr(), outs["xy"].data_ptr(), outs["yy"].data_ptr(),
                                        stride, pitch, images, *DELTA, b, None) == 0, sg.last_error()
    assert L.savgol2d_laplacian_batch_f32(n, n, 3, d.data_ptr(), rows, cols, stride, pitch, outs["lap"].data_ptr(), stride, pitch, images, *DELTA, b, None) == 0, sg.last_error()
    torch.cuda.synchronize()
    for name, (dx, dy) in (("gx", (1, 0)), ("gy", (0, 1)), ("xx", (2, 0)), ("xy", (1, 1)), ("yy", (0, 2))):
        hold(outs[name].cpu().numpy(), x, cols, sgo.Filter2D(n, n, 3, dx, dy, *DELTA), b, ("fused", name, n, b))
    # the Laplacian: xx and yy share a window, so the union of their footprints is that window's; finite pixels against the oracle's xx + yy, the bar from
    # the reference's own xx + yy (src/savgol2d.c:598-613) as test_fused_gradient_hessian_laplacian_batch has it
    oxx, oyy = sgo.Filter2D(n, n, 3, 2, 0, *DELTA), sgo.Filter2D(n, n, 3, 0, 2, *DELTA)
    def summed(k):
        with np.errstate(invalid="ignore"):                                  # Inf + -Inf where the two frames disagree on a sign: NaN, as it should be
            return oxx.apply_f64acc(x[k], cols, b) + oyy.apply_f64acc(x[k], cols, b)

    want = list(_POOL.map(summed, range(images)))

    def bar(k, fin):
        with np.errstate(invalid="ignore"):
            ref32 = oxx.apply(x[k], cols, b if b else 1) + oyy.apply(x[k], cols, b if b else 1)
        return fp32_bar(normwise(ref32[fin], want[k][fin]))

    hold(outs["lap"].cpu().numpy(), x, cols, oxx, b, ("fused", "laplacian", n, b), hi=want, bar=bar)


# ---- 16-bit storage: the output's non-finite set is the oracle's on the widened frame, on both routes ----
@pytest.mark.parametrize("pair", [("f16", "f32"), ("bf16", "bf16")])
@pytest.mark.parametrize("b", [nf.REFLECT, nf.CONSTANT])
@pytest.mark.parametrize("route", ["tiles", "staged"])
def test_h16_storage(sg, sgo, torch_gpu, route, b, pair):
    torch = torch_gpu
    n = 7
    x, cols, _, _, _ = nf.frames_for("aligned" if route == "tiles" else "ragged", n)
    images, rows, stride = x.shape
    tdt = {"f16": torch.float16, "bf16": torch.bfloat16, "f32": torch.float32}
    xq = torch.from_numpy(np.array(x)).to(tdt[pair[0]])                      # quantised on the CPU, nearest even; O(1) values: nothing overflows either type
    wide = xq.float().numpy()                                               # the widened frame: what the call's arithmetic sees
    assert np.array_equal(np.isnan(wide), np.isnan(x)) and np.array_equal(np.isinf(wide), np.isinf(x))
    d_in = xq.cuda()
    d_out = torch.full(x.shape, nf.SENTINEL, dtype=tdt[pair[1]], device="cuda")
    f = sg.Filter2D(n, n, 3)
    o = sgo.Filter2D(n, n, 3)
    it, ot = sg._STORAGE[pair[0]], sg._STORAGE[pair[1]]
    taken = sg.lib().savgol2d_apply_batch_h16_route(f.ptr, d_in.data_ptr(), it, rows, cols, stride, rows * stride, d_out.data_ptr(), ot, stride, rows * stride, images, b, 0)
    assert taken == (1 if route == "tiles" else 0), (taken, sg.last_error())
    f.apply_batch_h16(d_in, pair[0], d_out, rows, cols, images, out_dtype=pair[1], in_stride=stride, out_stride=stride, boundary=b)
    torch.cuda.synchronize()
    got = d_out.float().cpu().numpy()                                       # widening is exact and keeps every class
    sel = nf.stored(rows, cols, stride, n, n, b)
    for k in range(images):
        fp_hi, hi = nf.oracle_footprint(o, wide[k], cols, b)
        fp_got = ~np.isfinite(got[k]) & sel
        assert np.all(got[k][~sel] == nf.SENTINEL), (route, b, pair, k)
        assert (fp_got & ~fp_hi).sum() == 0, (route, b, pair, k, "non-finite where the window holds no special: " + where(fp_got & ~fp_hi))
        assert (fp_hi & ~fp_got).sum() == 0, (route, b, pair, k, "finite where the window holds a special: " + where(fp_hi & ~fp_got))
        assert np.all(np.isnan(got[k][nf.footprint(np.isnan(wide[k]), cols, n, n, b)])), (route, b, pair, k, "a NaN in the window is not a NaN out")
        STATS["share"] = max(STATS["share"], fp_hi.sum() / sel.sum())
    STATS["calls"] += 1
    STATS["frames"] += images
    STATS["specials"] += int((~np.isfinite(x)).sum())
    f.close()


def test_report(torch_gpu):
    """how much the cases above looked at (runs last in this file)"""
    print(f"\n2-D non-finite rule: {STATS['calls']} calls, {STATS['frames']} frames and {STATS['specials']} special pixels checked, "
          f"largest non-finite share of a frame's stored pixels {100 * STATS['share']:.1f} %")
    _DEVICE.clear()
    _POOL.close()
    assert STATS["share"] <= nf.MAX_SHARE
