"""savgol2d_apply_batch_h16 against its twin, bit for bit (the method of tests/test_gpu_stream_h16.py).

The input is quantised into the input type on the CPU.  The call under test runs on frames inside larger guard-filled tensors, with a stride larger
than cols and a pitch larger than rows x stride.  The twin -- savgol2d_apply_batch_f32 with the same filter, boundary and method -- runs on x.float()
(exact) in fresh aligned fp32 tensors with stride = cols rounded up to 4, pre-filled with the guard, so the twin itself shows which pixels it writes.
Expected output: twin.to(dtype) on the CPU (nearest even: checked first, on ties, overflow and subnormals of both types).  Words are compared; NaN
positions must coincide; every pixel the twin did not write (the VALID border), the pad columns, the gaps between frames and the guards around the
stack must still be the guard, and the input with its guards must be unchanged.  No tolerance: the bar is bit equality.

Geometry restated from Roll<N> and roll_tile_rows (csrc/sg_2d_roll.hip): a strip stores SW = 4 (64 - 2 HL) columns with HL = 2 (n <= 4), 4 (n = 5, 6),
ceil(n / 4) above; a tile is TR rows."""
import os
import subprocess
import sys

import numpy as np
import pytest

from tests._util import check, fp32_bar, normwise

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HALF_WINDOWS = [1, 4, 5, 7, 8, 10, 12, 14, 16]             # every HL class, both occupancy classes, the TR classes
ALL_PAIRS = [("bf16", "bf16"), ("f16", "f16"), ("f16", "f32"), ("bf16", "f32")]
GUARD = -7.0
TR = {**{n: 20 for n in range(1, 8)}, 8: 14, 9: 14, 10: 10, 11: 20, 12: 20, 13: 18, 14: 16, 15: 18, 16: 18}
VALID, CONSTANT, REFLECT = 0, 1, 2


def HL(n):
    return 2 if n <= 4 else (4 if n <= 6 else (n + 3) // 4)


def SW(n):
    return 4 * (64 - 2 * HL(n))


@pytest.fixture(scope="module")
def torch_gpu(sg):
    import torch
    assert torch.cuda.is_available() and sg.device_count() > 0, sg.last_error()
    return torch


def tdtype(torch, name):
    return {"f16": torch.float16, "bf16": torch.bfloat16, "f32": torch.float32}[name]


def as_int(torch, t):
    return t.view(torch.int32 if t.dtype == torch.float32 else torch.int16)


def same_words(torch, got, want, what):
    """bit equality; NaN positions coincide, NaN payloads are free"""
    assert got.shape == want.shape and got.dtype == want.dtype, what
    gn, wn = torch.isnan(got), torch.isnan(want)
    assert torch.equal(gn, wn), (what, "NaN positions")
    a, b = as_int(torch, got).masked_fill(gn, 0), as_int(torch, want).masked_fill(wn, 0)
    if not torch.equal(a, b):
        bad = (a != b).nonzero()
        raise AssertionError((what, f"{bad.shape[0]} of {a.numel()} words differ, first at {bad[0].tolist()}: got {got[tuple(bad[0])].item()!r} want {want[tuple(bad[0])].item()!r}"))


def frames(torch, images, rows, cols, seed):
    """smooth structure plus noise, O(1): fp32 on the CPU"""
    g = torch.Generator().manual_seed(seed)
    y = torch.arange(rows, dtype=torch.float32)[None, :, None]
    x = torch.arange(cols, dtype=torch.float32)[None, None, :]
    k = torch.arange(images, dtype=torch.float32)[:, None, None]
    return torch.sin(0.11 * x + 0.3 * k) * torch.cos(0.07 * y) + 0.5 + 0.3 * torch.randn((images, rows, cols), generator=g)


class Guarded:
    """`images` frames of rows x cols of `dtype`, row stride cols + pad, pitch rows x stride + gap, `off` elements off the (aligned) base of a larger
    tensor pre-filled with the guard"""

    def __init__(self, torch, images, rows, cols, dtype, off=0, pad=4, gap=8):
        self.stride, self.torch = cols + pad, torch
        self.pitch = rows * self.stride + gap
        lead = 64 + off
        self.whole = torch.full((lead + images * self.pitch + 64,), GUARD, dtype=dtype, device="cuda")
        self.stack = torch.as_strided(self.whole, (images, rows, cols), (self.pitch, self.stride, 1), lead)

    def ptr(self):
        return self.stack.data_ptr()

    def outside_is_guard(self, keep=None):
        """everything but the frames' pixels (keep: and but those of them the twin wrote) is still the guard"""
        t = self.torch
        mask = t.zeros_like(self.whole, dtype=t.bool)
        view = t.as_strided(mask, self.stack.shape, self.stack.stride(), self.stack.storage_offset())
        view[...] = True if keep is None else keep
        return bool((self.whole[~mask] == GUARD).all())


def run_case(sg, torch, filt, rows, cols, images, boundary, pair, method=0, off_in=0, off_out=0, pad=4, gap=8, seed=0, mutate=None, what="", twin_out=None):
    """one call against its twin; returns (the twin's fp32 frames [images][rows][cols] on the CPU, the mask of the pixels it wrote)"""
    what = (what, filt, rows, cols, images, boundary, pair, method, off_in, off_out, pad, gap)
    idt, odt = tdtype(torch, pair[0]), tdtype(torch, pair[1])
    f = sg.Filter2D(*filt)
    xq = frames(torch, images, rows, cols, seed).to(idt)                      # quantised into the input type on the CPU, nearest even
    if mutate is not None:
        mutate(xq)
    src, dst = Guarded(torch, images, rows, cols, idt, off_in, pad, gap), Guarded(torch, images, rows, cols, odt, off_out, pad, gap)
    src.stack.copy_(xq)
    keep = src.whole.clone()
    f.apply_batch_h16(src.ptr(), pair[0], dst.ptr(), rows, cols, images, out_dtype=pair[1], in_stride=src.stride, out_stride=dst.stride,
                      in_pitch=src.pitch, out_pitch=dst.pitch, boundary=boundary, method=method)
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
    want = twin.to(odt)                                                       # rounded once, on the CPU
    got = dst.stack.cpu()
    same_words(torch, got[wrote], want[wrote], what)
    assert dst.outside_is_guard(keep=wrote.cuda()), (what, "a pixel the twin does not write, a pad column, a gap or a guard was written")
    assert torch.equal(as_int(torch, src.whole), as_int(torch, keep)), (what, "the input or its guards changed")
    if twin_out is not None:
        twin_out.append((xq, twin, got))
    f.close()
    return twin, wrote


def test_cpu_rounding_is_nearest_even(torch_gpu):
    """tensor.to(dtype) on the CPU, the rounding the expected values go through: ties to even, overflow to Inf, gradual underflow"""
    torch = torch_gpu
    f16 = [(1 + 2.0 ** -11, 1.0), (1 + 3 * 2.0 ** -11, 1 + 2.0 ** -9), (65519.0, 65504.0), (65520.0, float("inf")), (-65520.0, float("-inf")),
           (2.0 ** -25, 0.0), (3 * 2.0 ** -25, 2.0 ** -23), (2.0 ** -24, 2.0 ** -24), (1.5 * 2.0 ** -24, 2.0 ** -23), (-0.0, -0.0)]
    bf16 = [(1 + 2.0 ** -8, 1.0), (1 + 3 * 2.0 ** -8, 1 + 2.0 ** -6), (3.3895313892515355e38, 3.3895313892515355e38), (3.4e38, float("inf")),
            (2.0 ** -134, 0.0), (3 * 2.0 ** -134, 2.0 ** -132), (2.0 ** -133, 2.0 ** -133)]
    for dtype, table in ((torch.float16, f16), (torch.bfloat16, bf16)):
        src = torch.tensor([a for a, _ in table], dtype=torch.float32)
        want = torch.tensor([b for _, b in table], dtype=torch.float64)
        got = src.to(dtype)
        assert torch.equal(got.double(), want), (dtype, got.double().tolist())
        assert torch.equal(torch.signbit(got), torch.signbit(src))


def shape_list(n):
    """(rows, cols) of one half window: every column count with one row count in turn, the narrowest frame with every row count"""
    sw, hl, tr = SW(n), HL(n), TR[n]
    cols = [32, 36, sw, sw + 4, sw + 256 - 4 * hl - 4, sw + 256 - 4 * hl, 2 * sw + 40]
    rows = [3, 2 * n + 1, tr, tr + 1, 2 * tr + 3]
    out = [(rows[(i + 1) % len(rows)], c) for i, c in enumerate(cols)]
    out += [(r, 32) for r in rows] + [(3, sw + 4), (2 * tr + 3, sw + 256 - 4 * hl)]
    return list(dict.fromkeys(out))


@pytest.mark.parametrize("n", HALF_WINDOWS)
def test_tile_shapes_equal_the_twin(sg, sgo, torch_gpu, n):
    """order-3 smoothing (config 4's class; order 2 at n = 1): the tile route at every strip and tile seam, all boundary modes a shape admits; bf16 -> bf16 everywhere, all
    four pairs on one shape per mode; one bf16 -> f32 output per half window also against the fp64 oracle on the widened input"""
    torch = torch_gpu
    order = min(3, 2 * n)                                                     # a 3 x 3 window holds order 2 at most: the same additive class
    filt = (n, n, order)
    cases = valid_cases = 0
    for k, (rows, cols) in enumerate(shape_list(n)):
        for b in (VALID, CONSTANT, REFLECT):
            if b == VALID and (rows <= 2 * n or cols <= 2 * n):
                continue                                                      # the call refuses these: not a shape VALID admits
            run_case(sg, torch, filt, rows, cols, 2, b, ALL_PAIRS[0], seed=100 * n + k)
            cases += 1
            valid_cases += b == VALID
    assert valid_cases >= 3, valid_cases
    rows, cols = TR[n] + 1 if TR[n] + 1 > 2 * n else 2 * n + 3, SW(n) + 4
    for b in (VALID, CONSTANT, REFLECT):
        for pair in ALL_PAIRS:
            keep = []
            run_case(sg, torch, filt, rows, cols, 2, b, pair, seed=7 * n + b, twin_out=keep)
            cases += 1
            if pair == ("bf16", "f32") and b == REFLECT:
                # the anchor: the output itself (the twin's fp32 pixels) against the double-accumulation oracle on the widened input, under the project's
                # bar: 1e-6, or 1.1 x the error of the reference's own dense fp32 sum on this frame
                xq, twin, got = keep[0]
                img = np.ascontiguousarray(xq[0].float().numpy())
                o = sgo.Filter2D(n, n, order)
                hi, ref32 = o.apply_f64acc(img, cols, b), o.apply(img, cols, b)
                check(normwise(got[0].numpy(), hi), fp32_bar(normwise(ref32, hi)), ("h16 anchor", n, b))
    print(f"n={n}: {cases} calls held to their twins, {valid_cases} of them VALID")


@pytest.mark.parametrize("pair", [("f16", "f16"), ("bf16", "bf16"), ("f16", "f32")])
def test_values(sg, torch_gpu, pair):
    """ties on the way out, fp16 overflow, subnormal inputs, a NaN and an Inf pixel in the interior and in the reflected border -- on the tile route and,
    one pointer 2 bytes off, on the staged route"""
    torch = torch_gpu
    idt = tdtype(torch, pair[0])
    rows, cols = (200, 256) if pair[0] == "f16" else (400, 512)

    def mutate(x):
        bits = x.view(torch.int16)
        bits[0, 40:60, 8:200] = (torch.arange(192, dtype=torch.int16) % 128)[None, :]          # +0 and positive subnormals of either type
        bits[0, 70:90, 8:200] = (torch.arange(192, dtype=torch.int16) % 128)[None, :] | -32768   # -0 and negative subnormals
        if pair[0] == "f16":
            x[1, 100:160, 20:120] = 65504.0                                   # a plateau at fp16's largest finite value: the fit overshoots just inside its
            x[1, 100:160, 130:230] = -65504.0                                 # edges, finite in fp32 and beyond 65504: +-Inf on the way out to fp16
        x[0, 120, 100] = float("nan")
        x[0, 150, 30] = float("inf")
        x[1, 1, 2] = float("nan")                                            # within n of two borders: reflected
        x[1, rows - 2, cols - 1] = float("-inf")

    for off_in in (0, 1):
        for b in (REFLECT, VALID):
            keep = []
            run_case(sg, torch, (4, 4, 3), rows, cols, 2, b, pair, off_in=off_in, seed=31, mutate=mutate, what="values", twin_out=keep)
            xq, twin, got = keep[0]
            w = twin.view(torch.int32)
            half = 0x1000 if pair[1] == "f16" else 0x8000                    # fp32 words exactly between two neighbours of the output type
            ties = int(((w & (2 * half - 1)) == half).sum()) if pair[1] != "f32" else 1
            assert ties >= 1, "no tie in this frame: the case does not test what it says"
            assert int(torch.isnan(twin).sum()) >= 4 and (pair != ("f16", "f16") or int(torch.isinf(got).sum()) > int(torch.isinf(twin).sum()))
            sub = xq.float().abs()
            assert int(((sub > 0) & (sub < (2.0 ** -14 if pair[0] == "f16" else 2.0 ** -126))).sum()) > 1000
    assert idt in (torch.float16, torch.bfloat16)


def test_xcd_chunk_order(sg, torch_gpu):
    """110 frames of 200 x 64 at n = 7: 1100 tiles in 550 blocks, XCD chunks of 65 blocks -- the chunked order engages and the last span is partial"""
    run_case(sg, torch_gpu, (7, 7, 3), 200, 64, 110, REFLECT, ("bf16", "bf16"), pad=0, gap=0, seed=5, what="xcd chunks")
    run_case(sg, torch_gpu, (7, 7, 3), 200, 64, 110, VALID, ("f16", "f32"), seed=6, what="xcd chunks")


def test_staged_route(sg, torch_gpu):
    """everything the host rule sends to the twin itself: the same contract"""
    torch = torch_gpu
    n = 7
    smooth = (n, n, 3)
    k = 0
    for b in (VALID, CONSTANT, REFLECT):
        for cols in (67, 28, 66):                                             # cols % 4 != 0, narrower than 32
            run_case(sg, torch, smooth, 45, cols, 2, b, ALL_PAIRS[k % 4], seed=k, what="staged cols"); k += 1
        for kw in (dict(off_in=1), dict(off_in=2), dict(off_out=1), dict(off_out=2), dict(pad=3), dict(gap=6)):       # each pointer off its grid, one at a time
            for pair in (("bf16", "bf16"), ("f16", "f32")):
                run_case(sg, torch, smooth, 45, 64, 2, b, pair, seed=k, what="staged alignment", **kw); k += 1
        for filt in ((5, 5, 3, 1, 0), (5, 5, 3, 0, 1), (5, 5, 3, 2, 0), (4, 4, 4), (3, 5, 4), (9, 16, 6)):                 # x- and y-dominant derivative filters, order 4,
            run_case(sg, torch, filt, 60, 64, 2, b, ALL_PAIRS[k % 4], seed=k, what="staged filter"); k += 1          # a rectangular window, method 0 falling to the dense kernel
        run_case(sg, torch, smooth, 45, 64, 2, b, ("bf16", "bf16"), method=3, seed=k, what="staged method 3"); k += 1
        run_case(sg, torch, smooth, 45, 64, 2, b, ("f16", "f16"), method=2, seed=k, what="method 2 (tiles)"); k += 1


def test_rectangular_smoothing_window_on_a_tileable_frame(sg, torch_gpu):
    """half windows 5 x 3 and 3 x 5 on a frame the tiles would take: the fp32 call runs them on zero-padded factors, which are not the additive form, so the
    twin takes its general two-term tile and this call the staged route (tests/test_h16_2d_host.py holds the route); the same contract"""
    for b in (VALID, CONSTANT, REFLECT):
        for pair in (("bf16", "bf16"), ("f16", "f32")):
            run_case(sg, torch_gpu, (5, 3, 3), 43, SW(5) + 4, 2, b, pair, seed=b, what="rectangular")
            run_case(sg, torch_gpu, (3, 5, 3), 43, SW(5) + 4, 2, b, pair, seed=b, what="rectangular")


def test_staged_pieces_do_not_change_bits(sg, torch_gpu):
    """5 frames of 2049 x 2047 are 3 + 2 frames of 2^24-pixel pieces on the staged route; the twin is one unchunked call"""
    run_case(sg, torch_gpu, (7, 7, 3), 2049, 2047, 5, REFLECT, ("bf16", "bf16"), pad=1, gap=0, seed=9, what="chunk seam")


CHILD = """
import sys
sys.path.insert(0, {root!r})
import torch
from __graft_entry__ import load_package
from tests import test_gpu_2d_h16 as T
sg = load_package()
for b in (0, 1, 2):
    for pair in (("bf16", "bf16"), ("f16", "f32")):
        T.run_case(sg, torch, (7, 7, 3), 43, T.SW(7) + 4, 2, b, pair, seed=3, what="child")
print("child ok")
"""


@pytest.mark.parametrize("switch", ["SAVGOL_HIP_2D_H16_TILES", "SAVGOL_HIP_ROLL_TILE"])
def test_switches(torch_gpu, switch):
    """a tile-able shape with the 16-bit tiles off, and with the fp32 call's own tiles off (the twin's are off there too): the same expectation, in a
    fresh child process each"""
    env = dict(os.environ, **{switch: "0"})
    out = subprocess.run([sys.executable, "-c", CHILD.format(root=ROOT)], env=env, cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "child ok" in out.stdout, (out.stdout[-2000:], out.stderr[-4000:])


@pytest.mark.parametrize("route", ["tiles", "staged"])
def test_capture_and_replay(sg, torch_gpu, route):
    """after one warm-up call the call only enqueues: captured into a graph and replayed, it writes the eager call's words"""
    torch = torch_gpu
    rows, cols, images = 43, (SW(7) + 4 if route == "tiles" else 67), 3
    f = sg.Filter2D(7, 7, 3)
    x = frames(torch, images, rows, cols, 12).to(torch.bfloat16).cuda()
    want = torch.full((images, rows, cols), GUARD, dtype=torch.bfloat16, device="cuda")
    f.apply_batch_h16(x, "bf16", want, rows, cols, images, boundary=VALID)    # eager, and the warm-up
    torch.cuda.synchronize()
    out = torch.full_like(want, GUARD)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(s):
        with torch.cuda.graph(g, stream=s):
            f.apply_batch_h16(x, "bf16", out, rows, cols, images, boundary=VALID, stream=s)
    out.fill_(GUARD)
    torch.cuda.synchronize()
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(as_int(torch, out), as_int(torch, want))
    assert bool((want[:, 7:rows - 7, 7:cols - 7] != GUARD).any()) and bool((want[:, :7] == GUARD).all())
    f.close()


def test_refusals_on_the_device(sg, torch_gpu):
    """the geometry checks with the fp32 call's texts, then overlap compared byte-wise; nothing is written; images == 0 returns 0"""
    torch = torch_gpu
    L = sg.lib()
    F16, F32 = sg.SAVGOL_HIP_F16, sg.SAVGOL_HIP_F32
    rows, cols = 40, 64
    f = sg.Filter2D(3, 3, 3)
    buf = torch.full((8 * rows * cols,), GUARD, dtype=torch.float16, device="cuda")
    p = buf.data_ptr()
    frame = rows * cols * 2

    def refused(text, *args):
        assert L.savgol2d_apply_batch_h16(f.ptr, *args) == -1, text
        err = sg.last_error()
        assert "savgol2d_apply_batch_h16" in err and text in err, (text, err)

    refused("bad image geometry", p, F16, rows, cols, cols - 1, rows * cols, p + 4 * frame, F16, cols, rows * cols, 1, 1, 0, None)
    refused("bad image geometry", p, F16, 0, cols, cols, rows * cols, p + 4 * frame, F16, cols, rows * cols, 1, 1, 0, None)
    refused("image smaller than the window", p, F16, 6, cols, cols, 6 * cols, p + 4 * frame, F16, cols, 6 * cols, 1, 0, 0, None)
    refused("overlap", p, F16, rows, cols, cols, rows * cols, p, F16, cols, rows * cols, 1, 1, 0, None)
    refused("overlap", p, F16, rows, cols, cols, rows * cols, p + 2 * frame - 2, F16, cols, rows * cols, 2, 1, 0, None)
    refused("overlap", p + 4 * frame, F16, rows, cols, cols, rows * cols, p + 2, F32, cols, rows * cols, 2, 1, 0, None)      # the fp32 stack's last two bytes on the input's first
    refused("overlap", p, F16, rows, cols, cols, rows * cols, p + 2 * frame - 4, F32, cols, rows * cols, 2, 1, 3, None)
    assert L.savgol2d_apply_batch_h16(f.ptr, p, F16, rows, cols, cols, rows * cols, p, F16, cols, rows * cols, 0, 1, 0, None) == 0     # no images: nothing to do
    torch.cuda.synchronize()
    assert bool((buf == GUARD).all())
    # touching end to start is served: fp32 frames right behind the 16-bit ones
    assert L.savgol2d_apply_batch_h16(f.ptr, p, F16, rows, cols, cols, rows * cols, p + 2 * frame, F32, cols, rows * cols, 2, 1, 0, None) == 0, sg.last_error()
    torch.cuda.synchronize()
    f.close()
