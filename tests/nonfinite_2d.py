"""The reference's NaN / Inf footprint on 2-D frames, restated twice, and the frames the GPU tests of tests/test_gpu_2d_nonfinite.py run on.

The reference's dense loop is `sum += W[i] * in[...]` over the whole window, no tap skipped (src/savgol2d.c:374-393), so one non-finite pixel makes
non-finite exactly the outputs whose window, after the border remap (src/savgol2d.c:428-445), contains it -- a zero tap times NaN or Inf is NaN too.
  1. from the oracle:     ~isfinite(sgo.Filter2D(...).apply_f64acc(frame, cols, b)) inside the stored region          (oracle_footprint)
  2. geometrically:       output (oy, ox) is hit iff some non-finite input (iy, ix) has iy among fix(oy + w), |w| <= ny, and ix among fix(ox + w), |w| <= nx;
                          fix = the reference's remap (REFLECT, or the clamp for CONSTANT); VALID stores the interior and remaps nothing  (footprint)
tests/test_nonfinite_2d_rule.py (CPU) holds the two together; the GPU tests take their expected values from the oracle only.

The frames.  Sizes are those of the existing kernel tests.  "aligned": 120 + 2n rows x 520 columns, 16-byte aligned base (tile form, vector strips); "ragged":
97 + 2n rows x 301 columns, stride 303, base one float off (strip walk, scalar path).  Background: sin x cos + ramp + noise.  The specials alternate NaN, +Inf, -Inf:
  * a STAIRCASE of K = 50 consecutive rows, each special in a column slot of its own, slots at least 2n + 1 + 8 + 12 columns apart and dealt over the frames of the batch;
    step k sits k % 16 columns into its slot (all four positions of a lane's quad, all sixteen of the tile kernel's segment).  50 consecutive rows pass every
    phase of every tile height and ring length the kernels have (the longest: 2n + 20 = 50 and 2n + 4 = 36 at n = 16) without the test knowing either;
  * pixel (0, 0), a pixel within n of two borders, one in the last row, one in the last column;
  * columns 239 and 240 (a strip seam of the rolling kernels);
  * +Inf and -Inf n rows apart in one column: both in one window, and the row that leaves a rolling sum is Inf while another Inf is inside.
The batch is as many frames (at least 4) as keep every frame's non-finite share of the stored pixels at or below MAX_SHARE under all three boundary modes: the
comparison of the finite pixels can then not be emptied.  Wide windows on the small frame need more than 4 (a (2n + 1)^2 footprint is 4 % of its VALID interior at
n = 16), up to MAX_FRAMES."""
import functools

import numpy as np

VALID, CONSTANT, REFLECT = 0, 1, 2
SENTINEL = -5.0
MAX_SHARE = 0.25
STAIR = 50
MAX_FRAMES = 16
SHAPES = {"aligned": (120, 520, 520, 0), "ragged": (97, 301, 303, 1)}        # rows - 2n, cols, stride, floats the base is off a 16-byte boundary
SPECIALS = (np.float32(np.nan), np.float32(np.inf), np.float32(-np.inf))


def fix(i, size, boundary):
    """the reference's border remap of index i (src/savgol2d.c:428-445)"""
    if boundary == REFLECT:
        if i < 0:
            i = -i - 1
        elif i >= size:
            i = 2 * size - i - 1
    return min(max(i, 0), size - 1)


def stored(rows, cols, stride, nx, ny, boundary):
    """the pixels a call writes: the frame, or VALID's interior"""
    sel = np.zeros((rows, stride), bool)
    if boundary == VALID:
        sel[ny:rows - ny, nx:cols - nx] = True
    else:
        sel[:, :cols] = True
    return sel


@functools.lru_cache(maxsize=256)
def _reach(size, half, boundary):
    """R[o, i]: input index i is in the remapped window of output index o"""
    R = np.zeros((size, size), np.float32)
    lo, hi = (half, size - half) if boundary == VALID else (0, size)
    for o in range(lo, hi):
        for w in range(-half, half + 1):
            R[o, fix(o + w, size, CONSTANT if boundary == VALID else boundary)] = 1.0
    return R


def footprint(bad, cols, nx, ny, boundary):
    """restatement 2: bad = mask (rows x stride) of the input pixels in question; returns the mask of the outputs whose window holds one of them"""
    rows, stride = bad.shape
    hit = _reach(rows, ny, boundary) @ bad[:, :cols].astype(np.float32) @ _reach(cols, nx, boundary).T
    out = np.zeros((rows, stride), bool)
    out[:, :cols] = hit > 0
    return out & stored(rows, cols, stride, nx, ny, boundary)


def oracle_footprint(o, frame, cols, boundary):
    """restatement 1: where the oracle's fp64 frame is not finite, inside the stored region; returns (footprint, the fp64 frame)"""
    hi = o.apply_f64acc(frame, cols, boundary)
    return ~np.isfinite(hi) & stored(frame.shape[0], cols, frame.shape[1], o.nx, o.ny, boundary), hi


def special_pixels(rows, cols, n, frames):
    """[(frame, row, column)] of the specials, in the order their values alternate"""
    spacing = (2 * n + 1 + 8 + 12 + 15) // 16 * 16      # neighbouring slots hold steps whose k % 16 differ by up to 12; a multiple of 16, and so is the
    margin = (n + 2 + 15) // 16 * 16                    # margin: step k sits in column k mod 16 of a 16-column segment
    per = max(1, (cols - 2 * margin - 16) // spacing)
    r0 = n + 3
    px = []
    for k in range(STAIR):
        slot = (k // frames) % per
        px.append((k % frames, r0 + k, margin + slot * spacing + k % 16))
    low = r0 + STAIR + 7                                 # below the staircase: rows n + 60 .. 2n + 70 < 97 + 2n
    px += [(0, 0, 0), (1 % frames, rows - 2, 1), (2 % frames, rows - 1, 150), (3 % frames, low + 10, cols - 1),
           (4 % frames, low, 239), (5 % frames, low, 240)]
    return px, [(6 % frames, low + 2, 100), (6 % frames, low + 2 + n, 100)]        # the same-window pair: +Inf above -Inf


def _background(frames, rows, cols, stride, seed):
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:rows, 0:cols]
    x = np.zeros((frames, rows, stride), np.float32)
    for k in range(frames):
        x[k, :, :cols] = (np.sin(0.07 * xx + k) * np.cos(0.04 * yy) + 0.002 * xx + 0.003 * k * yy + rng.normal(0, 0.1, (rows, cols))).astype(np.float32)
    return x


def _place(x, rows, cols, n):
    frames = x.shape[0]
    px, pair = special_pixels(rows, cols, n, frames)
    for i, (f, r, c) in enumerate(px):
        x[f, r, c] = SPECIALS[i % 3]
    x[pair[0]] = np.float32(np.inf)
    x[pair[1]] = np.float32(-np.inf)
    return len(px) + 2


def share(frame, cols, n, boundary):
    """non-finite share of the pixels a square window n stores on this frame"""
    rows, stride = frame.shape
    return footprint(~np.isfinite(frame), cols, n, n, boundary).sum() / stored(rows, cols, stride, n, n, boundary).sum()


@functools.lru_cache(maxsize=None)
def frames_for(kind, n):
    """(frames [B][rows][stride] fp32 (read-only), cols, floats the device base is shifted by, number of specials, largest share over frames and modes)
    for the square window n (a rectangular window uses its larger half)"""
    extra, cols, stride, shift = SHAPES[kind]
    rows = extra + 2 * n
    for frames in range(4, MAX_FRAMES + 1):
        x = _background(frames, rows, cols, stride, 977 * n + len(kind))
        count = _place(x, rows, cols, n)
        worst = max(share(x[k], cols, n, b) for k in range(frames) for b in (VALID, CONSTANT, REFLECT))
        if worst <= MAX_SHARE:
            break
    x.setflags(write=False)
    return x, cols, shift, count, float(worst)
