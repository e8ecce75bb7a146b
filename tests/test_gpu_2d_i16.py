"""savgol2d_apply_batch_i16 against its twin, bit for bit (the method of tests/test_gpu_2d_h16.py, whose Guarded buffers and frames() it uses).

The input is frames() scaled to counts (amplitude 8000: all but a few samples in a million inside +-22 000, every one inside +-30 000) and rounded to int16 on the CPU.  The call under test runs on frames
inside larger guard-filled tensors, with a stride larger than cols and a pitch larger than rows x stride.  The twin -- savgol2d_apply_batch_f32 with
the same filter, boundary and method -- runs on x.float() (exact) in fresh aligned fp32 tensors with stride = cols rounded up to 4, pre-filled with the
guard, so the twin itself shows which pixels it writes.  Expected output: for fp32 the twin's words themselves, for int16 to_i16(twin) on the CPU
(round to nearest even, NaN -> 0, clamp, cast: tests/test_gpu_stream_i16.py).  Words are compared, no tolerance.  Every pixel the twin did not write
(the VALID border), the pad columns, the gaps between frames and the guards around the stack must still be the guard, and the input with its guards
must be unchanged.

An int16 output hides any error under half a count, so every shape and mode runs int16 -> fp32 as well: that run holds the twin's bits themselves.
Every case on frames() asserts on the TWIN's output that fewer than 1 % of its pixels lie outside [-32768, 32767] and that its median magnitude is at
least 50 counts: the input tests what it says.  The cases that are about saturation or constants say so and assert their own condition instead."""
import os
import subprocess
import sys

import numpy as np
import pytest

from tests._util import check, fp32_bar, normwise
from tests.test_gpu_2d_h16 import GUARD, HL, SW, TR, Guarded, as_int, frames, shape_list

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HALF_WINDOWS = [1, 4, 5, 7, 8, 10, 12, 14, 16]
OUTS = ("i16", "f32")
AMPLITUDE = 8000.0
VALID, CONSTANT, REFLECT = 0, 1, 2


@pytest.fixture(scope="module")
def torch_gpu(sg):
    import torch
    assert torch.cuda.is_available() and sg.device_count() > 0, sg.last_error()
    return torch


def to_i16(torch, w):
    """the contract's conversion of fp32 pixels, on the CPU (as tests/test_gpu_stream_i16.py): nearest even, saturated, NaN -> 0"""
    assert w.device.type == "cpu" and w.dtype == torch.float32
    return torch.clamp(torch.nan_to_num(torch.round(w), nan=0.0), -32768, 32767).to(torch.int16)


def counts(torch, images, rows, cols, seed):
    x = torch.round(AMPLITUDE * frames(torch, images, rows, cols, seed))
    assert float(x.abs().max()) <= 30000.0                                     # 8000 x (1.5 + 0.3 x 5.6 sigma at most): the cast below saturates nothing
    return x.to(torch.int16)


def same_words(torch, got, want, what):
    assert got.shape == want.shape and got.dtype == want.dtype, what
    a, b = as_int(torch, got), as_int(torch, want)
    if not torch.equal(a, b):
        bad = (a != b).nonzero()
        raise AssertionError((what, f"{bad.shape[0]} of {a.numel()} words differ, first at {bad[0].tolist()}: got {got[tuple(bad[0])].item()!r} want {want[tuple(bad[0])].item()!r}"))


def run_case(sg, torch, filt, rows, cols, images, boundary, out, method=0, off_in=0, off_out=0, pad=4, gap=8, seed=0, mutate=None, what="", twin_out=None,
             amplitude="inside", route=None, pad_in=None, pad_out=None, gap_in=None, gap_out=None):
    """one call against its twin; returns (the twin's fp32 frames [images][rows][cols] on the CPU, the mask of the pixels it wrote).
    route: 1 = TILES, 0 = STAGED -- what savgol2d_apply_batch_i16_route must answer for the very arguments of the call (None: not asked).
    pad_in / pad_out / gap_in / gap_out: the stride's and the pitch's excess of one side alone (default: pad, gap).
    amplitude: "inside" = the conditions of the module's docstring; "saturating" = more than half of the twin's pixels lie outside the int16 range;
    None = the case states its own"""
    pad_in, pad_out = (pad if pad_in is None else pad_in), (pad if pad_out is None else pad_out)
    gap_in, gap_out = (gap if gap_in is None else gap_in), (gap if gap_out is None else gap_out)
    what = (what, filt, rows, cols, images, boundary, out, method, off_in, off_out, pad_in, pad_out, gap_in, gap_out)
    odt = torch.int16 if out == "i16" else torch.float32
    f = sg.Filter2D(*filt)
    xq = counts(torch, images, rows, cols, seed)
    if mutate is not None:
        mutate(xq)
    src, dst = Guarded(torch, images, rows, cols, torch.int16, off_in, pad_in, gap_in), Guarded(torch, images, rows, cols, odt, off_out, pad_out, gap_out)
    src.stack.copy_(xq)
    keep = src.whole.clone()
    layout = dict(out_dtype=out, in_stride=src.stride, out_stride=dst.stride, in_pitch=src.pitch, out_pitch=dst.pitch, boundary=boundary, method=method)
    if route is not None:
        took = f.apply_batch_i16_route(src.ptr(), dst.ptr(), rows, cols, images, **layout)
        assert took == route, (what, "route", took, sg.last_error())
    f.apply_batch_i16(src.ptr(), dst.ptr(), rows, cols, images, **layout)
    # the twin: fresh aligned fp32 tensors, stride = cols rounded up to 4, pitch = rows x stride
    s4 = (cols + 3) // 4 * 4
    tin = torch.zeros((images, rows, s4), dtype=torch.float32, device="cuda")
    tin[:, :, :cols] = xq.float().cuda()                                      # widened exactly
    tout = torch.full((images, rows, s4), GUARD, dtype=torch.float32, device="cuda")
    assert tin.data_ptr() % 16 == 0 and tout.data_ptr() % 16 == 0
    f.apply_batch(tin, tout, rows, cols, images, in_stride=s4, out_stride=s4, boundary=boundary, method=method)
    torch.cuda.synchronize()
    twin = tout[:, :, :cols].cpu()
    wrote = as_int(torch, twin) != as_int(torch, torch.tensor([GUARD]))         # the twin defines the footprint ...
    region = torch.zeros((images, rows, cols), dtype=torch.bool)
    nx, ny = filt[0], filt[1]
    if boundary == VALID:
        region[:, ny:rows - ny, nx:cols - nx] = True
    else:
        region[...] = True
    assert torch.equal(wrote, region), (what, "the twin's footprint")          # ... which is the frame, or VALID's interior
    assert bool((tout[:, :, cols:] == GUARD).all()), what
    t = twin[wrote]
    assert bool(torch.isfinite(t).all()), what
    outside = float(((t < -32768) | (t > 32767)).float().mean())
    if amplitude == "inside":
        assert outside < 0.01 and float(t.abs().median()) >= 50.0, (what, outside, float(t.abs().median()))
    elif amplitude == "saturating":
        assert outside > 0.5, (what, outside)
    want = to_i16(torch, twin) if out == "i16" else twin                      # converted once, on the CPU
    got = dst.stack.cpu()
    same_words(torch, got[wrote], want[wrote], what)
    assert dst.outside_is_guard(keep=wrote.cuda()), (what, "a pixel the twin does not write, a pad column, a gap or a guard was written")
    assert torch.equal(src.whole, keep), (what, "the input or its guards changed")
    if twin_out is not None:
        twin_out.append((xq, twin, got))
    f.close()
    return twin, wrote


def test_cpu_conversion_is_the_contracts(torch_gpu):
    """to_i16, the conversion the expected words go through: ties to even, saturation, NaN -> 0"""
    torch = torch_gpu
    table = [(0.5, 0), (1.5, 2), (2.5, 2), (-0.5, 0), (-1.5, -2), (-2.5, -2), (32766.5, 32766), (32767.49, 32767), (32767.5, 32767), (40000.0, 32767),
             (-32768.5, -32768), (-40000.0, -32768), (float("inf"), 32767), (float("-inf"), -32768), (float("nan"), 0), (123.4, 123)]
    got = to_i16(torch, torch.tensor([a for a, _ in table], dtype=torch.float32))
    assert got.tolist() == [b for _, b in table]


@pytest.mark.parametrize("n", HALF_WINDOWS)
def test_tile_shapes_equal_the_twin(sg, sgo, torch_gpu, n):
    """order-3 smoothing (config 4's class; order 2 at n = 1): the tile route at every strip and tile seam, all boundary modes a shape admits, both output
    types everywhere; one int16 -> fp32 output per half window also against the fp64 oracle on the widened input"""
    torch = torch_gpu
    order = min(3, 2 * n)
    filt = (n, n, order)
    f = sg.Filter2D(*filt)
    cases = valid_cases = 0
    anchored = False
    for k, (rows, cols) in enumerate(shape_list(n)):
        for b in (VALID, CONSTANT, REFLECT):
            if b == VALID and (rows <= 2 * n or cols <= 2 * n):
                continue                                                      # the call refuses these: not a shape VALID admits
            for out in OUTS:
                # the layout run_case builds keeps quads aligned: the call takes the tiles (asked of the rule itself, on stand-in addresses)
                assert f.apply_batch_i16_route(1 << 32, 1 << 40, rows, cols, 2, out_dtype=out, in_stride=cols + 4, out_stride=cols + 4, in_pitch=rows * (cols + 4) + 8,
                                               out_pitch=rows * (cols + 4) + 8, boundary=b) == 1, (n, rows, cols, b, out)
                keep = []
                run_case(sg, torch, filt, rows, cols, 2, b, out, seed=100 * n + k, twin_out=keep, route=1)
                cases += 1
                if out == "f32" and b == REFLECT and not anchored and rows > TR[n] and cols > SW(n):
                    # the anchor: the output itself (the twin's fp32 pixels) against the double-accumulation oracle on the widened input, under the
                    # project's bar: 1e-6, or 1.1 x the error of the reference's own dense fp32 sum on this frame
                    xq, twin, got = keep[0]
                    img = np.ascontiguousarray(xq[0].float().numpy())
                    o = sgo.Filter2D(n, n, order)
                    hi, ref32 = o.apply_f64acc(img, cols, b), o.apply(img, cols, b)
                    check(normwise(got[0].numpy(), hi), fp32_bar(normwise(ref32, hi)), ("i16 anchor", n, b))
                    anchored = True
            valid_cases += b == VALID
    assert valid_cases >= 3 and anchored, (valid_cases, anchored)
    f.close()
    print(f"n={n}: {cases} calls held to their twins, {valid_cases} shapes of them VALID")


@pytest.mark.parametrize("out", OUTS)
def test_values(sg, torch_gpu, out):
    """plateaus at both ends of the range whose fitted overshoot saturates, ties on the way out, a frame of zeros, a frame of -32768 -- on the tile route
    and, one pointer 2 bytes off, on the staged route"""
    torch = torch_gpu
    rows, cols = 200, 256
    filt = (4, 4, 3)

    def plateaus(x):
        x[1, 100:160, 20:120] = 32767                                         # the fit overshoots just inside a plateau's edges: finite in fp32, beyond the
        x[1, 100:160, 130:230] = -32768                                       # range, clamped on the way out

    f = sg.Filter2D(*filt)
    for off_in in (0, 1):
        assert f.apply_batch_i16_route((1 << 32) + 2 * off_in, 1 << 40, rows, cols, 2, out_dtype=out, in_stride=cols + 4, out_stride=cols + 4,
                                       in_pitch=rows * (cols + 4) + 8, out_pitch=rows * (cols + 4) + 8, boundary=REFLECT) == 1 - off_in
        for b in (REFLECT, VALID):
            keep = []
            # (a smoothed plateau at the range's end lies a rounding error inside or outside it: the amplitude conditions are asked of frame 0, which has none)
            run_case(sg, torch, filt, rows, cols, 2, b, out, off_in=off_in, seed=31, mutate=plateaus, what="values", twin_out=keep, amplitude=None, route=1 - off_in)
            xq, twin, got = keep[0]
            plain = twin[0, 4:rows - 4, 4:cols - 4]
            assert float(((plain < -32768) | (plain > 32767)).float().mean()) < 0.01 and float(plain.abs().median()) >= 50.0
            region = twin[1, 90:170, 10:240]
            over, under = int((region > 32767.5).sum()), int((region < -32768.5).sum())
            assert over >= 10 and under >= 10 and bool(torch.isfinite(region).all()), (over, under)
            if out == "i16":
                assert int(got[1, 90:170, 10:240][region > 32767.5].min()) == 32767 and int(got[1, 90:170, 10:240][region < -32768.5].max()) == -32768
            inner = twin[:, 4:rows - 4, 4:cols - 4]
            ties = int(((inner - torch.floor(inner)) == 0.5).sum())
            assert ties >= 1, "no tie in this frame: the case does not test what it says"
            for level in (0, -32768):
                def constant(x, level=level):
                    x[...] = level
                keep = []
                run_case(sg, torch, filt, rows, cols, 2, b, out, off_in=off_in, seed=32, mutate=constant, what=("constant", level), twin_out=keep, amplitude=None, route=1 - off_in)
                xq, twin, got = keep[0]
                inner = got[:, 4:rows - 4, 4:cols - 4]
                if level == 0:
                    assert bool((inner == 0).all())
                elif out == "i16":
                    assert bool((inner == -32768).all())
                else:
                    assert float((inner.double() + 32768.0).abs().max()) < 0.05
    f.close()


def test_xcd_chunk_order(sg, torch_gpu):
    """110 frames of 200 x 64 at n = 7: 1100 tiles in 550 blocks, XCD chunks of 65 blocks -- the chunked order engages and the last span is partial"""
    run_case(sg, torch_gpu, (7, 7, 3), 200, 64, 110, REFLECT, "i16", pad=0, gap=0, seed=5, what="xcd chunks", route=1)
    run_case(sg, torch_gpu, (7, 7, 3), 200, 64, 110, REFLECT, "f32", pad=0, gap=0, seed=5, what="xcd chunks", route=1)
    run_case(sg, torch_gpu, (7, 7, 3), 200, 64, 110, VALID, "i16", seed=6, what="xcd chunks", route=1)
    run_case(sg, torch_gpu, (7, 7, 3), 200, 64, 110, VALID, "f32", seed=6, what="xcd chunks", route=1)


def test_staged_route(sg, torch_gpu):
    """everything the host rule sends to the twin itself: the same contract"""
    torch = torch_gpu
    n = 7
    smooth = (n, n, 3)
    k = 0
    for b in (VALID, CONSTANT, REFLECT):
        for cols in (67, 28, 66):                                             # cols % 4 != 0, narrower than 32
            for out in OUTS:
                run_case(sg, torch, smooth, 45, cols, 2, b, out, seed=k, what="staged cols", route=0); k += 1
        # each base, stride and pitch off its grid, one at a time: every one of them alone sends the call to the staged route
        for kw in (dict(off_in=1), dict(off_in=2), dict(off_out=1), dict(off_out=2), dict(pad_in=3), dict(pad_out=3), dict(gap_in=6), dict(gap_out=6)):
            for out in OUTS:
                run_case(sg, torch, smooth, 45, 64, 2, b, out, seed=k, what="staged alignment", route=0, **kw); k += 1
        # x- and y-dominant derivative filters, order 4, a rectangular window with method 0 falling to the dense kernel
        # (the second derivative on a grid of 0.5: per sample it is 48 counts in the median on these frames, under the 50 every case asks of its twin)
        for filt in ((5, 5, 3, 1, 0), (5, 5, 3, 0, 1), (5, 5, 3, 2, 0, 0.5, 1.0), (4, 4, 4), (3, 5, 4), (9, 16, 6)):
            run_case(sg, torch, filt, 60, 64, 2, b, OUTS[k % 2], seed=k, what="staged filter", route=0); k += 1
        for out in OUTS:
            run_case(sg, torch, smooth, 45, 64, 2, b, out, method=3, seed=k, what="staged method 3", route=0); k += 1
            run_case(sg, torch, smooth, 45, 64, 2, b, out, method=2, seed=k, what="method 2 (tiles)", route=1); k += 1
            # d/dx on a grid of 0.01: the derivative in counts per unit is a hundred times the one per sample -- most outputs saturate
            run_case(sg, torch, (5, 5, 3, 1, 0, 0.01, 1.0), 60, 64, 2, b, out, seed=k, what="saturating derivative", amplitude="saturating", route=0); k += 1


def test_rectangular_smoothing_window_on_a_tileable_frame(sg, torch_gpu):
    """half windows 5 x 3 and 3 x 5 on a frame the tiles would take: the twin takes its general two-term tile and this call the staged route
    (tests/test_i16_2d_host.py holds the route); the same contract"""
    for b in (VALID, CONSTANT, REFLECT):
        for out in OUTS:
            run_case(sg, torch_gpu, (5, 3, 3), 43, SW(5) + 4, 2, b, out, seed=b, what="rectangular", route=0)
            run_case(sg, torch_gpu, (3, 5, 3), 43, SW(5) + 4, 2, b, out, seed=b, what="rectangular", route=0)


def test_staged_pieces_do_not_change_bits(sg, torch_gpu):
    """5 frames of 2049 x 2047 are 3 + 2 frames of 2^24-pixel pieces on the staged route; the twin is one unchunked call"""
    run_case(sg, torch_gpu, (7, 7, 3), 2049, 2047, 5, REFLECT, "i16", pad=1, gap=0, seed=9, what="chunk seam", route=0)


CHILD = """
import sys
sys.path.insert(0, {root!r})
import torch
from __graft_entry__ import load_package
from tests import test_gpu_2d_i16 as T
sg = load_package()
for b in (0, 1, 2):
    for out in T.OUTS:
        T.run_case(sg, torch, (7, 7, 3), 43, T.SW(7) + 4, 2, b, out, seed=3, what="child", route=0)       # a shape the tiles take with both switches on
print("child ok")
"""


@pytest.mark.parametrize("switch", ["SAVGOL_HIP_2D_I16_TILES", "SAVGOL_HIP_ROLL_TILE"])
def test_switches(torch_gpu, switch):
    """a tile-able shape with the int16 tiles off, and with the fp32 call's own tiles off (the twin's are off there too): the same expectation, in a
    fresh child process each"""
    env = dict(os.environ, **{switch: "0"})
    out = subprocess.run([sys.executable, "-c", CHILD.format(root=ROOT)], env=env, cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "child ok" in out.stdout, (out.stdout[-2000:], out.stderr[-4000:])


@pytest.mark.parametrize("out", OUTS)
@pytest.mark.parametrize("route", ["tiles", "staged"])
def test_capture_and_replay(sg, torch_gpu, route, out):
    """after one warm-up call the call only enqueues: captured into a graph and replayed, it writes the eager call's words"""
    torch = torch_gpu
    rows, cols, images = 43, (SW(7) + 4 if route == "tiles" else 67), 3
    odt = torch.int16 if out == "i16" else torch.float32
    f = sg.Filter2D(7, 7, 3)
    x = counts(torch, images, rows, cols, 12).cuda()
    want = torch.full((images, rows, cols), GUARD, dtype=odt, device="cuda")
    assert f.apply_batch_i16_route(x, want, rows, cols, images, out_dtype=out, boundary=VALID) == (1 if route == "tiles" else 0)
    f.apply_batch_i16(x, want, rows, cols, images, out_dtype=out, boundary=VALID)       # eager, and the warm-up
    torch.cuda.synchronize()
    res = torch.full_like(want, GUARD)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(s):
        with torch.cuda.graph(g, stream=s):
            f.apply_batch_i16(x, res, rows, cols, images, out_dtype=out, boundary=VALID, stream=s)
    res.fill_(GUARD)
    torch.cuda.synchronize()
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(as_int(torch, res), as_int(torch, want))
    assert bool((want[:, 7:rows - 7, 7:cols - 7] != GUARD).any()) and bool((want[:, :7] == GUARD).all())
    f.close()


def test_refusals_on_the_device(sg, torch_gpu):
    """every refusal in the header's order on device pointers; nothing is written; images == 0 returns 0"""
    torch = torch_gpu
    L = sg.lib()
    I16, F32 = sg.SAVGOL_HIP_I16, sg.SAVGOL_HIP_F32
    rows, cols = 40, 64
    f = sg.Filter2D(3, 3, 3)
    buf = torch.full((8 * rows * cols,), int(GUARD), dtype=torch.int16, device="cuda")
    p = buf.data_ptr()
    frame = rows * cols * 2
    q = p + 4 * frame

    def refused(text, *args):
        assert L.savgol2d_apply_batch_i16(*args) == -1, text
        err = sg.last_error()
        assert "savgol2d_apply_batch_i16" in err and text in err, (text, err)

    refused("method 1", f.ptr, p, rows, cols, cols, rows * cols, q, I16, cols, rows * cols, 1, 1, 1, None)
    refused("method 5", f.ptr, p, rows, cols, cols, rows * cols, q, I16, cols, rows * cols, 1, 1, 5, None)
    refused("out_type 2", f.ptr, p, rows, cols, cols, rows * cols, q, sg.SAVGOL_HIP_BF16, cols, rows * cols, 1, 1, 0, None)
    refused("NULL pointer", f.ptr, None, rows, cols, cols, rows * cols, q, I16, cols, rows * cols, 1, 1, 0, None)
    refused("NULL pointer", None, p, rows, cols, cols, rows * cols, q, I16, cols, rows * cols, 1, 1, 0, None)
    import ctypes as C
    bad = type(f.ptr.contents)()
    C.memmove(C.byref(bad), f.ptr, C.sizeof(bad))
    bad.window_width += 2
    refused("not a valid Savgol2DFilter", C.pointer(bad), p, rows, cols, cols, rows * cols, q, I16, cols, rows * cols, 1, 1, 0, None)
    refused("bad image geometry", f.ptr, p, rows, cols, cols - 1, rows * cols, q, I16, cols, rows * cols, 1, 1, 0, None)
    refused("bad image geometry", f.ptr, p, 0, cols, cols, rows * cols, q, I16, cols, rows * cols, 1, 1, 0, None)
    refused("image smaller than the window", f.ptr, p, 6, cols, cols, 6 * cols, q, I16, cols, 6 * cols, 1, 0, 0, None)
    refused("overlap", f.ptr, p, rows, cols, cols, rows * cols, p, I16, cols, rows * cols, 1, 1, 0, None)
    refused("overlap", f.ptr, p, rows, cols, cols, rows * cols, p + 2 * frame - 2, I16, cols, rows * cols, 2, 1, 0, None)
    refused("overlap", f.ptr, q, rows, cols, cols, rows * cols, p + 2, F32, cols, rows * cols, 2, 1, 0, None)      # the fp32 stack's last two bytes on the input's first
    refused("overlap", f.ptr, p, rows, cols, cols, rows * cols, p + 2 * frame - 4, F32, cols, rows * cols, 2, 1, 3, None)
    assert L.savgol2d_apply_batch_i16(f.ptr, p, rows, cols, cols, rows * cols, p, I16, cols, rows * cols, 0, 1, 0, None) == 0     # no images: nothing to do
    torch.cuda.synchronize()
    assert bool((buf == int(GUARD)).all())
    # touching end to start is served: fp32 frames right behind the int16 ones
    assert L.savgol2d_apply_batch_i16(f.ptr, p, rows, cols, cols, rows * cols, p + 2 * frame, F32, cols, rows * cols, 2, 1, 0, None) == 0, sg.last_error()
    torch.cuda.synchronize()
    f.close()
