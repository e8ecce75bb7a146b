"""CPU: the two restatements of the reference's NaN / Inf footprint (tests/nonfinite_2d.py) agree on the frames the GPU tests use, the oracle's fp32
restatement has the same non-finite set and the same NaN set, and no frame is so full of specials that a comparison of its finite pixels is empty."""
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

from tests import nonfinite_2d as nf


@pytest.mark.parametrize("kind", ["aligned", "ragged"])
@pytest.mark.parametrize("n", [1, 2, 5, 7, 16])
def test_the_two_restatements_agree(sgo, kind, n):
    x, cols, _, count, worst = nf.frames_for(kind, n)
    assert count == nf.STAIR + 8 and int((~np.isfinite(x)).sum()) == count, "a special was placed on another"
    assert worst <= nf.MAX_SHARE
    # a smoothing filter and two derivative filters (whose tables hold exact zeros: a zero tap times a special is NaN in the reference too), dealt over the
    # (mode, frame) pairs so that every frame meets every mode and every filter meets every mode
    filters = [(3 if n > 1 else 2, 0, 0), (2, 1, 0), (2, 0, 2)]
    jobs = [filters[(b + k) % 3] + (b, k) for b in (nf.VALID, nf.CONSTANT, nf.REFLECT) for k in range(x.shape[0])]

    def one(job):
        order, dx, dy, b, k = job
        o = sgo.Filter2D(n, n, order, dx, dy, 0.5, 2.0)
        sel = nf.stored(x.shape[1], cols, x.shape[2], n, n, b)
        fp, hi = nf.oracle_footprint(o, x[k], cols, b)
        geo = nf.footprint(~np.isfinite(x[k]), cols, n, n, b)
        ref32 = o.apply(x[k], cols, b)
        assert np.array_equal(fp, geo), (job, "oracle footprint != geometric footprint")
        assert np.array_equal(~np.isfinite(ref32) & sel, fp), (job, "the fp32 restatement's non-finite set")
        assert np.array_equal(np.isnan(ref32) & sel, np.isnan(hi) & sel), (job, "the fp32 restatement's NaN set")
        assert not np.any(geo & ~sel) and fp.sum() <= nf.MAX_SHARE * sel.sum(), job
        assert np.all(np.isnan(hi[nf.footprint(np.isnan(x[k]), cols, n, n, b)])), (job, "a NaN in the window is a NaN out")
        return fp.sum() / sel.sum()

    with ThreadPoolExecutor(8) as pool:                          # the oracle runs outside the interpreter lock
        shares = list(pool.map(one, jobs))
    assert 0 < max(shares) <= nf.MAX_SHARE


@pytest.mark.parametrize("kind", ["aligned", "ragged"])
def test_every_frame_keeps_its_finite_pixels(kind):
    """every half window the GPU tests use, all three modes (frames_for measures the share with the geometric rule, which the test above ties to the oracle)"""
    for n in range(1, 17):
        x, cols, shift, count, worst = nf.frames_for(kind, n)
        assert 4 <= x.shape[0] <= nf.MAX_FRAMES and worst <= nf.MAX_SHARE, (kind, n, x.shape, worst)
        assert x.shape[1] <= 200 + 2 * n and cols <= 724
        px, pair = nf.special_pixels(x.shape[1], cols, n, x.shape[0])
        assert len({p[1] for p in px[:nf.STAIR]}) == nf.STAIR and {p[2] % 16 for p in px[:nf.STAIR]} == set(range(16))
        assert pair[1][1] - pair[0][1] == n and pair[0][2] == pair[1][2]


def test_rectangular_footprint_is_inside_the_square_one():
    x, cols, _, _, _ = nf.frames_for("ragged", 7)
    bad = ~np.isfinite(x[0])
    for b in (nf.VALID, nf.CONSTANT, nf.REFLECT):
        rect, square = nf.footprint(bad, cols, 4, 7, b), nf.footprint(bad, cols, 7, 7, b)
        assert rect.sum() < square.sum() and not np.any(rect & ~square[:, :] & nf.stored(x.shape[1], cols, x.shape[2], 7, 7, b))
