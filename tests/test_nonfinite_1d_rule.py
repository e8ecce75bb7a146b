"""CPU: the two restatements of the reference's NaN / Inf footprint on 1-D batches (tests/nonfinite_1d.py) agree on the signals the GPU tests use, for every
half window of tests/test_gpu_1d_nonfinite.py, every boundary mode and VALID, d = 0, 1, 2; the oracle's fp32 restatement of the reference has the same
non-finite set and the same NaN set; no channel is so full of specials that a comparison of its finite outputs is empty; the staircases meet all 64 residues
and every listed special is where the helper's text says."""
import numpy as np
import pytest

from tests import nonfinite_1d as nf

# every half window a test of tests/test_gpu_1d_nonfinite.py runs (that file asserts it uses no other)
HALF_WINDOWS = (1, 3, 4, 5, 9, 12, 13, 16, 18, 19, 20, 21, 24, 27, 31, 32)


@pytest.mark.parametrize("n", HALF_WINDOWS)
def test_the_two_restatements_agree(sgo, n):
    x, count, worst, _ = nf.signals_for(n)
    bad, nan = ~np.isfinite(x), np.isnan(x)
    assert worst <= nf.MAX_SHARE
    seen = 0.0
    for order, d, dt in ((min(4, 2 * n), 0, 1.0), (min(3, 2 * n), 1, 0.5), (min(4, 2 * n), 2, 0.25)):
        if d > order:
            continue
        for mode in nf.MODES:
            o = sgo.Filter(n, order, d, dt, nf.POLYNOMIAL if mode == nf.VALID else mode)
            sel = nf.stored(x.shape[1], n, mode)[None, :]
            fp, hi = nf.oracle_footprint(o, x, mode)
            geo = nf.footprint(bad, n, mode)
            where = np.argwhere(fp != geo)
            assert len(where) == 0, (n, order, d, mode, "oracle footprint != geometric footprint", len(where), where[:4].tolist())
            ref32 = o.apply(x, nf.POLYNOMIAL if mode == nf.VALID else mode)
            assert np.array_equal(~np.isfinite(ref32) & sel, fp), (n, order, d, mode, "the fp32 restatement's non-finite set")
            assert np.array_equal(np.isnan(ref32) & sel, np.isnan(hi) & sel), (n, order, d, mode, "the fp32 restatement's NaN set")
            assert np.array_equal(np.isposinf(ref32) & sel, np.isposinf(hi) & sel), (n, order, d, mode, "the fp32 restatement's +Inf set")
            assert np.all(np.isnan(hi[nf.footprint(nan, n, mode)])), (n, order, d, mode, "a NaN in the window is a NaN out")
            share = fp.sum(axis=1) / sel.sum()
            assert share.max() <= nf.MAX_SHARE and share[-1] == 0.0, (n, order, d, mode, share)          # the cap, from the oracle alone; the control channel
            seen = max(seen, float(share.max()))
    assert 0.0 < seen <= nf.MAX_SHARE


@pytest.mark.parametrize("n", HALF_WINDOWS)
def test_every_listed_special_is_present(n):
    x, count, worst, stair_channels = nf.signals_for(n)
    channels, length = x.shape
    assert length == nf.LENGTH == 10493 and channels == stair_channels + 2 >= 4
    base, pitch = nf.slot_pitch(n, stair_channels)
    assert base % 64 == 0 and pitch % 64 == 0 and pitch >= 4 * (2 * n + 1)
    sp = nf.specials(n, stair_channels)
    for name in ("nan_stair", "inf_stair"):
        steps = sp[name]
        assert len(steps) == nf.STEPS and {s % 64 for _, s, _ in steps} == set(range(64)), (n, name, "a residue mod 64 is not met")
        assert {c for c, _, _ in steps} == set(range(stair_channels))
        for c in range(stair_channels):                                  # no two steps of a channel share a window: 2n + 1 apart and more
            at = sorted(s for cc, s, _ in sp["nan_stair"] + sp["inf_stair"] if cc == c)
            assert np.diff(at).min() > 2 * (2 * n + 1), (n, c)
        assert min(s for _, s, _ in steps) >= 4 * n + 64 and max(s for _, s, _ in steps) < length - 4 * n - 64
    assert all(np.isnan(v) for _, _, v in sp["nan_stair"])
    assert [bool(v > 0) for _, _, v in sp["inf_stair"]] == [k % 2 == 0 for k in range(nf.STEPS)] and all(np.isinf(v) for _, _, v in sp["inf_stair"])
    # the stairs run from the first tile of every width into the last whole one (the partial last tile has the channel-end specials)
    every = [s for _, s, _ in sp["nan_stair"] + sp["inf_stair"]]
    assert min(every) < 1024 and max(every) >= 2 * 4096 + 1024
    assert {s for _, s, _ in sp["ends"]} == {0, n - 1, n, 2 * n, length - 1 - 2 * n, length - 1 - n, length - 1}
    assert [s for _, s, _ in sp["seams"]] == [1023, 1024, 2047, 2048, 4095, 4096, 8191, 8192]
    assert [(s, float(v)) for _, s, v in sp["pairs"]] == [(3000, np.inf), (3000 + n, -np.inf), (6000, np.inf), (6000 + n, np.inf)]
    placed = [p for group in sp.values() for p in group]
    assert count == len(placed) == len({(c, s) for c, s, _ in placed})
    for c, s, v in placed:
        assert (np.isnan(v) and np.isnan(x[c, s])) or x[c, s] == v, (n, c, s, v)
    assert not x.flags.writeable and np.isfinite(x[-1]).all() and nf.shares(x, n).max() == worst <= nf.MAX_SHARE


def test_remap_is_the_reference_s():
    """spot values of get_padded_sample's index rule, the clamps of a window longer than the channel included"""
    assert [nf.remap(i, 10, nf.REFLECT) for i in (-1, -2, -10, -11, -30, 10, 11, 19, 20, 40)] == [0, 1, 9, 9, 9, 9, 8, 0, 0, 0]
    assert [nf.remap(i, 10, nf.PERIODIC) for i in (-1, -10, -11, 10, 25)] == [9, 0, 9, 0, 5]
    assert [nf.remap(i, 10, nf.CONSTANT) for i in (-1, -7, 10, 99)] == [0, 0, 9, 9]
    bad = np.zeros((1, 40), bool)
    bad[0, 0] = True
    assert np.flatnonzero(nf.footprint(bad, 3, nf.PERIODIC)).tolist() == [0, 1, 2, 3, 37, 38, 39]
    assert np.flatnonzero(nf.footprint(bad, 3, nf.REFLECT)).tolist() == [0, 1, 2, 3]
    assert np.flatnonzero(nf.footprint(bad, 3, nf.VALID)).tolist() == [3]
    assert np.flatnonzero(nf.footprint(bad, 3, nf.POLYNOMIAL)).tolist() == [0, 1, 2, 3]
    bad[:] = False
    bad[0, 6] = True                                                     # the last sample of the POLYNOMIAL edge window: every edge row uses it
    assert np.flatnonzero(nf.footprint(bad, 3, nf.POLYNOMIAL)).tolist() == [0, 1, 2, 3, 4, 5, 6, 7, 8, 9]
    assert np.flatnonzero(nf.footprint(bad, 3, nf.CONSTANT)).tolist() == [3, 4, 5, 6, 7, 8, 9]
