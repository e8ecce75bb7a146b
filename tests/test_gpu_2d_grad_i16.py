"""savgol2d_gradient_batch_i16 against its twin, bit for bit (the method of tests/test_gpu_2d_i16.py, whose counts / to_i16 and the Guarded buffers, frames,
SW, HL and same_words of tests/test_gpu_2d_h16.py it uses).

The input is int16 counts on the CPU.  The call under test runs on frames inside larger guard-filled tensors, with a stride larger than cols and a pitch
larger than rows x stride, one guarded stack per output frame.  The twin -- savgol2d_gradient_batch_f32 with the same windows, order, deltas and boundary --
runs on x.float() (exact) in fresh aligned fp32 tensors with stride = cols rounded up to 4, pre-filled with the guard, so the twin itself shows which
pixels it writes.  Expected: for fp32 the twin's words themselves, for int16 to_i16(twin) on the CPU.  The WHOLE guarded buffers are compared: every pixel
the twin did not write (the VALID border), the pad columns, the gaps between frames, the guards around each stack and the whole buffer of a frame that was
not requested must still be the guard, and the input with its guards must be unchanged.  No tolerance: the bar is bit equality.

Geometry restated from Hf<N> (csrc/sg_2d_hf.hip) and Roll<N> (csrc/sg_2d_roll.hip): a strip stores SW = 4 (64 - 2 HL) columns; gy's tile is 20 rows; gx's
ring has U = 2n + 1 + P slots, P = 5 at odd half windows and 3 at even ones.  A 3 x 3 window holds order 2 at most (ten terms do not fit nine pixels: the
configuration is refused), so n = 1 runs order 2 only."""
import os
import subprocess
import sys

import numpy as np
import pytest

from tests._util import check, fp32_bar, normwise
from tests.test_gpu_2d_h16 import GUARD, HL, SW, Guarded, as_int, frames, same_words
from tests.test_gpu_2d_i16 import counts, to_i16

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUTS = ("i16", "f32")
VALID, CONSTANT, REFLECT = 0, 1, 2
SWITCH = "SAVGOL_HIP_2D_GRAD_I16_DIRECT"
NAME = "savgol2d_gradient_batch_i16"
# what the twin's frames are pre-filled with: not a value a gradient of integer counts takes (a difference of counts over a small window is often a whole
# number, -7.0 among them, which is why the twin does not use the tested buffers' guard)
TWIN_GUARD = -7.12345e-20


def U(n):
    return 2 * n + 1 + (5 if n & 1 else 3)


@pytest.fixture(scope="module")
def torch_gpu(sg):
    import torch
    assert torch.cuda.is_available() and sg.device_count() > 0, sg.last_error()
    return torch


def shape_list(n):
    """(rows, cols): every column count with one row count in turn -- the first strip, the edge strips and the first all-interior strip against a tile seam of
    the gy tile, the gx ring wrapping twice, more than one band and a short last band"""
    sw, hl = SW(n), HL(n)
    cols = [32, 36, sw, sw + 4, sw + 256 - 4 * hl - 4, sw + 256 - 4 * hl, 2 * sw + 40]
    rows = [3, 2 * n + 1, 20, 21, 43, 2 * U(n) + 3, 8 * n + 5]
    return [(rows[(i + 1) % len(rows)], c) for i, c in enumerate(cols)]


def run_case(sg, torch, n, order, rows, cols, images, boundary, out, want=(True, True), deltas=(1.0, 1.0), off_in=0, off_gx=0, off_gy=0, pad=4, gap=8, seed=0, xq=None,
             route=None, amplitude="inside", what="", keep_out=None):
    """one call against its twin.  n: the half window, or (nx, ny).  want: which of (gx, gy) are requested.  route: what savgol2d_gradient_batch_i16_route must
    answer for the very arguments of the call (None: not asked).  amplitude "inside": fewer than 1 % of the twin's pixels lie outside the int16 range and
    their median magnitude is at least 2 counts -- four times the half count an int16 output hides (a three-row frame has little of a y gradient; the fp32
    output of the same case holds the twin's bits themselves); None: the case states its own.  keep_out: a list that receives
    (xq, [twin gx, twin gy], [got gx, got gy]) with None for a frame that was not requested."""
    nx, ny = (n, n) if isinstance(n, int) else n
    what = (what, nx, ny, order, rows, cols, images, boundary, out, want, deltas, off_in, off_gx, off_gy, pad, gap)
    odt = torch.int16 if out == "i16" else torch.float32
    if xq is None:
        xq = counts(torch, images, rows, cols, seed)
    src = Guarded(torch, images, rows, cols, torch.int16, off_in, pad, gap)
    dst = [Guarded(torch, images, rows, cols, odt, off, pad, gap) for off in (off_gx, off_gy)]
    src.stack.copy_(xq)
    keep = src.whole.clone()
    ptrs = [d.ptr() if w else None for d, w in zip(dst, want)]
    layout = dict(out_dtype=out, in_stride=src.stride, out_stride=dst[0].stride, in_pitch=src.pitch, out_pitch=dst[0].pitch, delta_x=deltas[0], delta_y=deltas[1],
                  boundary=boundary)
    if route is not None:
        took = sg.gradient_batch_i16_route(nx, ny, order, src.ptr(), ptrs[0], ptrs[1], rows, cols, images, **layout)
        assert took == route, (what, "route", took, sg.last_error())
    sg.gradient_batch_i16(nx, ny, order, src.ptr(), ptrs[0], ptrs[1], rows, cols, images, **layout)
    # the twin: fresh aligned fp32 tensors, stride = cols rounded up to 4, pitch = rows x stride
    s4 = (cols + 3) // 4 * 4
    tin = torch.zeros((images, rows, s4), dtype=torch.float32, device="cuda")
    tin[:, :, :cols] = xq.float().cuda()                                      # widened exactly
    tout = [torch.full((images, rows, s4), TWIN_GUARD, dtype=torch.float32, device="cuda") if w else None for w in want]
    assert tin.data_ptr() % 16 == 0 and all(t is None or t.data_ptr() % 16 == 0 for t in tout)
    rc = sg.lib().savgol2d_gradient_batch_f32(nx, ny, order, tin.data_ptr(), rows, cols, s4, rows * s4, tout[0].data_ptr() if want[0] else None,
                                              tout[1].data_ptr() if want[1] else None, s4, rows * s4, images, deltas[0], deltas[1], boundary, sg._stream(None))
    assert rc == 0, (what, sg.last_error())
    torch.cuda.synchronize()
    region = torch.zeros((images, rows, cols), dtype=torch.bool)
    if boundary == VALID:
        region[:, ny:rows - ny, nx:cols - nx] = True
    else:
        region[...] = True
    twins, gots = [None, None], [None, None]
    for i, name in enumerate(("gx", "gy")):
        if not want[i]:
            assert dst[i].outside_is_guard(keep=torch.zeros((images, rows, cols), dtype=torch.bool, device="cuda")), (what, name, "a frame that was not requested was written")
            continue
        twin = tout[i][:, :, :cols].cpu()
        wrote = as_int(torch, twin) != as_int(torch, torch.tensor([TWIN_GUARD]))     # the twin defines the footprint ...
        if amplitude is not None:
            assert torch.equal(wrote, region), (what, name, "the twin's footprint")   # ... which is the frame, or VALID's interior
        else:
            wrote = region                                                    # (a case with its own values may hold the guard's value as a result)
        assert bool((tout[i][:, :, cols:] == TWIN_GUARD).all()), (what, name)
        t = twin[wrote]
        if amplitude == "inside":
            outside = float(((t < -32768) | (t > 32767)).float().mean())
            assert bool(torch.isfinite(t).all()) and outside < 0.01 and float(t.abs().median()) >= 2.0, (what, name, outside, float(t.abs().median()))
        expect = to_i16(torch, twin) if out == "i16" else twin                # converted once, on the CPU
        got = dst[i].stack.cpu()
        same_words(torch, got[wrote], expect[wrote], (what, name))
        assert dst[i].outside_is_guard(keep=wrote.cuda()), (what, name, "a pixel the twin does not write, a pad column, a gap or a guard was written")
        twins[i], gots[i] = twin, got
    assert torch.equal(src.whole, keep), (what, "the input or its guards changed")
    if keep_out is not None:
        keep_out.append((xq, twins, gots))


SEAMS = [(n, order) for n in range(1, 8) for order in (2, 3) if (2 * n + 1) ** 2 >= (order + 1) * (order + 2) // 2]


@pytest.mark.parametrize("n,order", SEAMS)
def test_seams_equal_the_twin(sg, sgo, torch_gpu, n, order):
    """order 2 (one term per frame) and order 3 (two): the direct route at every strip, tile, ring and band seam, all boundary modes a shape admits, both
    output types; one fp32 output per half window also against the fp64 oracle on the widened frames -- at order 3, and at order 2 for n = 1, which has
    no order 3"""
    torch = torch_gpu
    cases = valid_cases = 0
    anchored = not (order == 3 or n == 1)                                     # every half window is anchored once: the assert below holds each to it
    for k, (rows, cols) in enumerate(shape_list(n)):
        for b in (VALID, CONSTANT, REFLECT):
            if b == VALID and (rows <= 2 * n or cols <= 2 * n):
                continue                                                      # the call refuses these: not a shape VALID admits
            for out in OUTS:
                keep = []
                run_case(sg, torch, n, order, rows, cols, 2, b, out, seed=100 * n + 10 * order + k, route=1, keep_out=keep)
                cases += 1
                if out == "f32" and b == REFLECT and not anchored and rows > 20 and cols > SW(n):
                    # the anchor: the outputs themselves against the double-accumulation oracle on the widened input, under the project's bar:
                    # 1e-6, or 1.1 x the error of the reference's own dense fp32 sum on this frame
                    xq, _, gots = keep[0]
                    img = np.ascontiguousarray(xq[0].float().numpy())
                    for i, (dx, dy) in enumerate(((1, 0), (0, 1))):
                        o = sgo.Filter2D(n, n, order, dx, dy)
                        hi, ref32 = o.apply_f64acc(img, cols, b), o.apply(img, cols, b)
                        check(normwise(gots[i][0].numpy(), hi), fp32_bar(normwise(ref32, hi)), ("grad i16 anchor", n, dx, dy))
                    anchored = True
            valid_cases += b == VALID
    assert valid_cases >= 3 and anchored, (valid_cases, anchored)
    print(f"n={n} order={order}: {cases} calls held to their twins, {valid_cases} shapes of them VALID")


@pytest.mark.parametrize("order,n", [(1, 1), (1, 4), (1, 7), (4, 2), (4, 5), (4, 7)])
def test_orders_1_and_4_on_the_direct_route(sg, torch_gpu, order, n):
    """the other two orders the host rule sends to the direct route: order 1 (one term per frame, the plane fit) and order 4 (two terms, the factors of
    another fit than order 3's; a 3 x 3 window does not hold it) -- an edge-strip frame and one with an all-interior strip, a tile seam in each"""
    k = 0
    for rows, cols in ((43, SW(n) + 4), (21, 2 * SW(n) + 40)):
        for b in (VALID, REFLECT):
            for out in OUTS:
                run_case(sg, torch_gpu, n, order, rows, cols, 2, b, out, seed=1000 * order + 10 * n + k, route=1, what="orders 1 and 4"); k += 1


@pytest.mark.parametrize("out", OUTS)
def test_one_output_only(sg, torch_gpu, out):
    """gx alone and gy alone, on both routes: the other stack, guards and all, stays untouched"""
    for want in ((True, False), (False, True)):
        for b in (VALID, REFLECT):
            run_case(sg, torch_gpu, 5, 3, 43, SW(5) + 4, 2, b, out, want=want, seed=7, route=1, what="one output")
            run_case(sg, torch_gpu, 5, 3, 43, 67, 2, b, out, want=want, seed=8, route=0, what="one output, staged")
    # the frame that is not requested does not count for the route: its pointer is NULL, whatever its buffer's alignment would have been
    run_case(sg, torch_gpu, 5, 2, 43, SW(5) + 4, 2, REFLECT, out, want=(True, False), off_gy=1, seed=9, route=1, what="one output")


@pytest.mark.parametrize("out", OUTS)
def test_values(sg, torch_gpu, out):
    """counts riding at 30 000 with +-50 of structure (what the horizontal-first order exists for), a saturating case with plateaus at both rails, a constant
    frame (the twin's words, not assumed zero), and deltas whose scale overflows; ties on the way out: test_ties_on_the_way_out"""
    torch = torch_gpu
    rows, cols = 45, SW(4) + 4
    for n, order in ((4, 3), (7, 2)):
        cols = SW(n) + 4
        riding = (30000.0 + torch.round(50.0 * (frames(torch, 2, rows, cols, 41) - 0.5))).to(torch.int16)
        assert int(riding.min()) > 29000 and int(riding.max()) < 31000
        for b in (REFLECT, VALID):
            keep = []
            run_case(sg, torch, n, order, rows, cols, 2, b, out, xq=riding, route=1, amplitude=None, what="riding", keep_out=keep)
            _, twins, _ = keep[0]
            for t in twins:                                                   # the structure's gradient, not the offset's: a few counts per sample
                inner = t[:, n:rows - n, n:cols - n]
                assert 0.3 < float(inner.abs().median()) < 100.0, float(inner.abs().median())
    # saturation: plateaus at both rails, deltas of 1/64 -- a step of 65 535 counts is a gradient far beyond the int16 range
    n, order, cols = 4, 3, SW(4) + 4
    sat = counts(torch, 2, rows, cols, 42)
    sat[1, 10:35, 20:120] = 32767
    sat[1, 10:35, 130:230] = -32768
    for b in (REFLECT, VALID):
        keep = []
        run_case(sg, torch, n, order, rows, cols, 2, b, out, xq=sat, deltas=(1.0 / 64, 1.0 / 64), route=1, amplitude=None, what="saturating", keep_out=keep)
        _, twins, gots = keep[0]
        for t, g in zip(twins, gots):
            region = t[1, n:rows - n, n:cols - n]
            over, under = int((region > 32767.5).sum()), int((region < -32768.5).sum())
            assert over >= 10 and under >= 10 and bool(torch.isfinite(region).all()), (over, under)
            if out == "i16":
                gr = g[1, n:rows - n, n:cols - n]
                assert int(gr[region > 32767.5].min()) == 32767 and int(gr[region < -32768.5].max()) == -32768
        # a constant frame: both gradients are whatever the twin makes of it
        for level in (0, 30000, -32768):
            run_case(sg, torch, n, order, rows, cols, 2, b, out, xq=torch.full((2, rows, cols), level, dtype=torch.int16), route=1, amplitude=None, what=("constant", level))
    # a delta small enough for 1 / delta to overflow fp32: accepted by the fp32 call; NaN positions coincide (fp32 out) and are 0 (int16 out), Inf saturates
    keep = []
    run_case(sg, torch, n, order, rows, cols, 2, REFLECT, out, deltas=(1e-39, 1e-39), seed=43, route=1, amplitude=None, what="overflowing scale", keep_out=keep)
    _, twins, gots = keep[0]
    assert all(not bool(torch.isfinite(t).all()) for t in twins), "the scale did not overflow: the case does not test what it says"
    if out == "i16":
        for t, g in zip(twins, gots):
            assert bool((g[torch.isnan(t)] == 0).all())


def test_ties_on_the_way_out(sg, torch_gpu):
    """deltas of 1/16 put the gradient at thousands of counts, where fp32 resolves 2^-10: the twin's frames hold exact halves, which the int16 output must
    round to even"""
    torch = torch_gpu
    n, order, rows = 4, 3, 45
    keep = []
    run_case(sg, torch, n, order, rows, SW(n) + 4, 2, REFLECT, "i16", deltas=(1.0 / 16, 1.0 / 16), seed=44, route=1, amplitude=None, what="ties", keep_out=keep)
    _, twins, gots = keep[0]
    ties = 0
    for t, g in zip(twins, gots):
        tie = ((t - torch.floor(t)) == 0.5) & (t.abs() < 32767)
        ties += int(tie.sum())
        assert bool((g[tie] % 2 == 0).all())
    assert ties >= 1, "no tie in these frames: the case does not test what it says"


def test_staged_route(sg, torch_gpu):
    """everything the host rule sends to the twin itself: the same contract"""
    torch = torch_gpu
    k = 0
    for b in (VALID, CONSTANT, REFLECT):
        for out in OUTS:
            for n, order in ((8, 3), (12, 2), (5, 5), ((5, 3), 3)):
                run_case(sg, torch, n, order, 60, 64, 2, b, out, seed=k, route=0, what="staged window"); k += 1
            run_case(sg, torch, 5, 3, 45, 67, 2, b, out, seed=k, route=0, what="staged cols"); k += 1
            for kw in (dict(off_in=1), dict(off_gx=1), dict(off_gy=1)):
                run_case(sg, torch, 5, 3, 45, 64, 2, b, out, seed=k, route=0, what="staged base", **kw); k += 1


def test_staged_pieces_do_not_change_bits(sg, torch_gpu):
    """11 frames of 1024 x 1024 are 10 + 1 frames on the staged route (three fp32 sides of floor(2^25 / 3) floats); the twin is one call"""
    run_case(sg, torch_gpu, 8, 3, 1024, 1024, 11, REFLECT, "i16", pad=0, gap=0, seed=9, route=0, what="piece seam")


def test_xcd_chunk_order(sg, torch_gpu):
    """110 frames of 200 x 64 at n = 7: gy's 1100 tiles in 550 blocks, XCD chunks of 65 blocks -- the chunked order engages and the last span is partial"""
    for out in OUTS:
        run_case(sg, torch_gpu, 7, 3, 200, 64, 110, REFLECT, out, pad=0, gap=0, seed=5, route=1, what="xcd chunks")
        run_case(sg, torch_gpu, 7, 2, 200, 64, 110, VALID, out, seed=6, route=1, what="xcd chunks")


CHILD = """
import sys
sys.path.insert(0, {root!r})
import torch
from __graft_entry__ import load_package
from tests import test_gpu_2d_grad_i16 as T
sg = load_package()
for b in (0, 1, 2):
    for out in T.OUTS:
        T.run_case(sg, torch, 7, 3, 43, T.SW(7) + 4, 2, b, out, seed=3, what="child", route=0)       # a shape the direct route takes with both switches on
print("child ok")
"""


@pytest.mark.parametrize("switch", [SWITCH, "SAVGOL_HIP_ROLL_TILE"])
def test_switches(torch_gpu, switch):
    """a shape of the direct route with the call's switch at 0, and with the fp32 call's own tiles off (the twin's are off there too): the same
    expectation, in a fresh child process each"""
    env = dict(os.environ, **{switch: "0"})
    out = subprocess.run([sys.executable, "-c", CHILD.format(root=ROOT)], env=env, cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "child ok" in out.stdout, (out.stdout[-2000:], out.stderr[-4000:])


@pytest.mark.parametrize("out", OUTS)
@pytest.mark.parametrize("route", ["direct", "staged"])
def test_capture_and_replay(sg, torch_gpu, route, out):
    """after one warm-up call the call only enqueues: captured into a graph and replayed, it writes the eager call's words"""
    torch = torch_gpu
    rows, cols, images = 43, (SW(7) + 4 if route == "direct" else 67), 3
    odt = torch.int16 if out == "i16" else torch.float32
    x = counts(torch, images, rows, cols, 12).cuda()
    want = [torch.full((images, rows, cols), GUARD, dtype=odt, device="cuda") for _ in range(2)]
    args = (7, 7, 3, x)
    kw = dict(out_dtype=out, boundary=VALID, delta_x=0.5)
    assert sg.gradient_batch_i16_route(*args, want[0], want[1], rows, cols, images, **kw) == (1 if route == "direct" else 0)
    sg.gradient_batch_i16(*args, want[0], want[1], rows, cols, images, **kw)       # eager, and the warm-up
    torch.cuda.synchronize()
    res = [torch.full_like(w, GUARD) for w in want]
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(s):
        with torch.cuda.graph(g, stream=s):
            sg.gradient_batch_i16(*args, res[0], res[1], rows, cols, images, stream=s, **kw)
    for r in res:
        r.fill_(GUARD)
    torch.cuda.synchronize()
    g.replay()
    torch.cuda.synchronize()
    for r, w in zip(res, want):
        assert torch.equal(as_int(torch, r), as_int(torch, w))
        assert bool((w[:, 7:rows - 7, 7:cols - 7] != GUARD).any()) and bool((w[:, :7] == GUARD).all())


def test_refusals_on_the_device(sg, torch_gpu):
    """every refusal in the header's order on device pointers; nothing is written; images == 0 and no requested frame return 0"""
    torch = torch_gpu
    L = sg.lib()
    I16, F32 = sg.SAVGOL_HIP_I16, sg.SAVGOL_HIP_F32
    rows, cols = 40, 64
    buf = torch.full((12 * rows * cols,), int(GUARD), dtype=torch.int16, device="cuda")
    p = buf.data_ptr()
    frame = rows * cols * 2
    gx, gy = p + 4 * frame, p + 8 * frame

    def go(nx=3, ny=3, order=3, d_in=p, r=rows, stride=cols, ox=gx, oy=gy, ot=I16, ostride=cols, images=1, dx=1.0, b=1):
        return L.savgol2d_gradient_batch_i16(nx, ny, order, d_in, r, cols, stride, r * stride, ox, oy, ot, ostride, r * ostride, images, dx, 1.0, b, None)

    def refused(text, **kw):
        assert go(**kw) == -1, text
        err = sg.last_error()
        assert NAME in err and text in err, (text, err)
        torch.cuda.synchronize()
        assert bool((buf == int(GUARD)).all()), text

    refused("out_type 2", ot=sg.SAVGOL_HIP_BF16, d_in=None)
    refused("NULL pointer", d_in=None, nx=0)
    refused("invalid configuration", nx=0, r=0)
    refused("invalid configuration", order=0)
    refused("invalid configuration", dx=0.0, ox=p)
    refused("bad image geometry", stride=cols - 1, ox=p)
    refused("bad image geometry", ostride=cols - 1)
    refused("image smaller than the window", r=6, b=0)
    refused("input and output frames overlap", ox=p)
    refused("input and output frames overlap", oy=p + 2 * frame - 2, images=2)
    refused("input and output frames overlap", d_in=gx, ot=F32, oy=None, ox=p + 2, images=2)       # the fp32 stack's last two bytes on the input's first
    refused("the two output frames overlap", oy=gx)
    refused("the two output frames overlap", oy=gx + 2 * frame - 2, images=2)
    assert go(ox=p, images=0) == 0 and go(ox=None, oy=None, ot=9, d_in=None) == 0
    torch.cuda.synchronize()
    assert bool((buf == int(GUARD)).all())
    # touching end to start is served: fp32 gx right behind the int16 input, gy right behind gx
    assert go(images=2, ot=F32, ox=p + 2 * frame, oy=p + 6 * frame) == 0, sg.last_error()
    torch.cuda.synchronize()
    assert bool((buf[:2 * rows * cols] == int(GUARD)).all()) and bool((buf[2 * rows * cols:10 * rows * cols] != int(GUARD)).any()) and bool((buf[10 * rows * cols:] == int(GUARD)).all())
