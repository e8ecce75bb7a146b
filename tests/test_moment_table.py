"""Host logic of the fp32 block-moment kernel (csrc/sg_k1d_momenth.hpp, half windows 20..32; host fit: csrc/sg_k1d_moment_fit.cpp), no GPU needed:
the constant table the kernel reads is rebuilt into outputs with the kernel's own arithmetic (fp32 FMA chains in the kernel's order, emulated in
numpy) and compared with the fp64 oracle.  The reference loop this path replaces: savgol_apply centre loop,
/root/reference/src/savgolFilter.c:763-766 with convolve_ilp :547-580.  (Round 2's whole-lane form and its table went in round 6.)
Below it, the same for the fp64 block-moment kernel (csrc/sg_k1d_moment64.hpp, half windows 24..32, savgol_hip_moment64_table): the 16 effective tap sets
rebuilt from the table must keep the promoted table's moments of order 0..2 -- what an offset, a ramp or a parabola under the signal multiplies."""
import ctypes as C

import numpy as np
import pytest

from oracle import sgo

FLOATS = 400
f32, f64 = np.float32, np.float64


def fma(a, b, c):                       # one rounding, like v_fma_f32 / v_pk_fma_f32
    return (f64(a) * f64(b) + f64(c)).astype(f32)


# ---- the half-lane form (csrc/sg_k1d_momenth.hpp; table layout in csrc/sg_k1d_host.hpp) ----
H_OFF_W, H_OFF_PHI, H_OFF_C = 0, 132, 276


def geometry_h(n):
    off = (n + 3) // 4 * 4 - n
    return off, (15 + off + 1) // 2 * 2, (off + 2 * n + 1) // 2 * 2


def table_h(sg, n, m, d):
    L = sg.lib()
    cfg = sg.SavgolConfig(n, m, d, 1.0, 0)
    f = L.savgol_create(C.byref(cfg))
    assert f
    tab = np.zeros(FLOATS, f32)
    terms = L.savgol_hip_momenth_table(f, tab.ctypes.data_as(C.POINTER(C.c_float)))
    w = np.array(f.contents.center_weights[:2 * n + 1], f32)
    L.savgol_destroy(f)
    return terms, tab, w


def emulate_h(tab, terms, x, n):
    """every 16-output group of x in the kernel's own arithmetic: x-stationary head and tail on three round-robin chains (tap pair (w[k], w[k-1])
    from the table), chains joined, block samples paired front to back into two partial moments each, the block's share added last"""
    off, lo, hi = geometry_h(n)
    bk, steps = hi - lo, (hi - lo) // 4
    wp = tab[H_OFF_W:H_OFF_W + 2 * (2 * n + 2)].reshape(-1, 2)              # wp[k] = (w[k], w[k-1])
    groups = (len(x) - 2 * n) // 16
    xp = np.concatenate([np.zeros(off, f32), x, np.zeros(8, f32)])
    X = np.stack([xp[16 * g:16 * g + 16 + 2 * n + off + 4] for g in range(groups)])
    A = np.zeros((3, 16, groups), f32)
    for i in list(range(off, lo)) + list(range(hi, off + 2 * n + 16)):
        for j in range(8):
            k = i - off - 2 * j
            if (i < lo and 0 <= k <= lo - 1 - off) or (i >= hi and hi - off - 14 <= k <= 2 * n + 1):
                A[k % 3, 2 * j] = fma(wp[k, 0], X[:, i], A[k % 3, 2 * j])
                A[k % 3, 2 * j + 1] = fma(wp[k, 1], X[:, i], A[k % 3, 2 * j + 1])
    a0 = (A[0] + A[1]).astype(f32) + A[2]
    M = np.zeros((terms, 2, groups), f32)
    for u in range(steps):
        f0, f1 = X[:, lo + 2 * u], X[:, lo + 2 * u + 1]
        b0, b1 = X[:, hi - 1 - 2 * u], X[:, hi - 2 - 2 * u]
        e = np.stack([f0 + b0, f1 + b1]).astype(f32)
        o = np.stack([f0 - b0, f1 - b1]).astype(f32)
        M[0] = e if u == 0 else (M[0] + e).astype(f32)
        for s in range(1, terms):
            ph = tab[H_OFF_PHI + (u * 6 + s - 1) * 2:H_OFF_PHI + (u * 6 + s - 1) * 2 + 2]
            v = o if s & 1 else e
            M[s] = np.stack([fma(ph[0], v[0], M[s, 0] if u else np.zeros(groups, f32)), fma(ph[1], v[1], M[s, 1] if u else np.zeros(groups, f32))])
    mu = (M[:, 0] + M[:, 1]).astype(f32)
    B = np.zeros((16, groups), f32)
    for s in range(terms - 1, -1, -1):
        c = tab[H_OFF_C + s * 16:H_OFF_C + s * 16 + 16]
        for r in range(16):
            B[r] = fma(c[r], mu[s], B[r])
    return (a0 + B).astype(f32).T.reshape(-1)


@pytest.mark.parametrize("n", [32, 31, 30, 29, 28, 27, 26, 25, 24, 23, 22, 21, 20])
@pytest.mark.parametrize("m,d,terms_expected,tol", [(4, 0, 5, 1e-6), (2, 0, 3, 1e-6), (3, 0, 3, 1e-6), (6, 0, 7, 1e-6), (4, 1, 5, 2e-6), (5, 1, 7, 2e-6)])
def test_half_lane_table_reproduces_the_filter(sg, n, m, d, terms_expected, tol):
    """the table of round 5's fp32 kernel (savgol_hip_momenth_table), rebuilt into outputs with the kernel's own arithmetic in numpy and compared with
    the double-precision convolution of the same fp32 taps; geometry and layout as csrc/sg_k1d_host.hpp states them"""
    terms, tab, w = table_h(sg, n, m, d)
    if terms == 0 and n < 24:
        pytest.skip("the fit does not reproduce this table to 3e-7 of its largest tap (n = 21, m = 5, d = 1): the filter keeps the plain sum")
    assert terms == terms_expected
    off, lo, hi = geometry_h(n)
    assert lo % 2 == 0 and hi % 2 == 0 and (hi - lo) % 4 == 0 and lo >= 15 + off and hi <= off + 2 * n + 1 and 20 <= hi - lo <= 48
    wp = tab[H_OFF_W:H_OFF_W + 2 * (2 * n + 2)].reshape(-1, 2)
    assert np.array_equal(wp[:2 * n + 1, 0], w) and wp[2 * n + 1, 0] == 0 and wp[0, 1] == 0 and np.array_equal(wp[1:, 1], w)
    x = sgo.synth_f32(5, 1, 16 * 128 + 2 * n)[0]
    got = emulate_h(tab, terms, x, n)
    ref = np.convolve(x.astype(f64), w[::-1].astype(f64), "valid")[:len(got)]
    err = np.max(np.abs(got - ref)) / np.max(np.abs(ref))
    assert err < tol, f"n={n} m={m} d={d}: normwise error {err:.3e}"


def test_paths_that_keep_the_plain_sum(sg):
    assert table_h(sg, 32, 8, 0)[0] == 0            # poly_order > 6
    assert table_h(sg, 16, 4, 0)[0] == 0 and table_h(sg, 19, 4, 0)[0] == 0      # half windows below MOMENTH_MIN_N = 20
    # a hand-edited table is not a polynomial: the fit must refuse it
    L = sg.lib()
    cfg = sg.SavgolConfig(32, 4, 0, 1.0, 0)
    f = L.savgol_create(C.byref(cfg))
    f.contents.center_weights[10] += 1e-4
    tab = np.zeros(FLOATS, f32)
    assert L.savgol_hip_momenth_table(f, tab.ctypes.data_as(C.POINTER(C.c_float))) == 0
    L.savgol_destroy(f)
    assert L.savgol_hip_momenth_table(None, tab.ctypes.data_as(C.POINTER(C.c_float))) == -1


def test_every_moment_table_is_compatible_with_the_1e6_bar(sg):
    """the fit accepts a polynomial that reproduces each fp32 tap to 3e-7 of the largest one; the taps of a whole block could
    add up.  So bound what actually reaches an output, for EVERY filter savgol_create builds at half windows 20..32 (every poly_order, every
    derivative): the kernel replaces the taps on a group's common block by sum_s c_s(r) phi_s(t), so output r carries the error
    E_r = sum_t |sum_s c_s(r) phi_s(t) - w[lo + t - r - off]|  per unit of input amplitude, against sum |w| -- the largest output a unit-amplitude
    input can produce.  E_r / sum|w| must leave the fp32 rounding of the remaining sum inside 1e-6: the worst table measures well under the 1.5e-7
    asserted here (printed with -s)."""
    worst = (0.0, None)
    covered = 0
    for n in range(20, 33):
        off, lo, hi = geometry_h(n)
        bk = hi - lo
        for m in range(0, 11):
            for d in range(0, min(m, 4) + 1):
                if 2 * n + m + 1 >= 76:
                    continue
                terms, tab, w = table_h(sg, n, m, d)
                if terms == 0:
                    continue
                covered += 1
                phi = np.ones((terms, bk), f64)
                for s in range(1, terms):
                    half = np.array([tab[H_OFF_PHI + ((t // 2) * 6 + s - 1) * 2 + (t & 1)] for t in range(bk // 2)], f64)
                    phi[s, :bk // 2] = half
                    phi[s, bk // 2:] = half[::-1] * (-1.0 if s & 1 else 1.0)
                c = np.stack([tab[H_OFF_C + s * 16:H_OFF_C + (s + 1) * 16].astype(f64) for s in range(terms)])       # [s][r]
                w_eff = c.T @ phi                                                                                   # [r][t]
                sum_abs = np.sum(np.abs(w.astype(f64)))
                for r in range(16):
                    true = w[lo - r - off:hi - r - off].astype(f64)
                    e = float(np.sum(np.abs(w_eff[r] - true)) / sum_abs)
                    if e > worst[0]:
                        worst = (e, (n, m, d, r, terms))
    print(f"moment tables checked: {covered}; worst block error / sum|w| = {worst[0]:.3e} at (n, m, d, r, terms) = {worst[1]}")
    assert covered >= 13 * 18
    assert worst[0] <= 1.5e-7, worst


# ---- the fp64 form (csrc/sg_k1d_moment64.hpp, savgol_apply[_valid]_batch_f64_tol; table: savgol_hip_moment64_table, layout in csrc/sg_k1d_host.hpp) ----
D_DOUBLES, D_MAX_PAIRS = 278, 25
D_OFF_W, D_OFF_PHI, D_OFF_C = 0, 16, 16 + D_MAX_PAIRS * 6
D_FILTERS = [(m, d) for m in range(0, 7) for d in range(0, min(m, 4) + 1)]          # every poly_order <= 6 with every derivative savgol_create accepts


def geometry_d(n):
    off = (n + 1) // 2 * 2 - n
    return off, 15 + off, off + 2 * n + 1


def table_d(sg, n, m, d):
    L = sg.lib()
    cfg = sg.SavgolConfig(n, m, d, 1.0, 0)
    f = L.savgol_create(C.byref(cfg))
    assert f
    tab = np.zeros(D_DOUBLES, f64)
    terms = L.savgol_hip_moment64_table(f, tab.ctypes.data_as(C.POINTER(C.c_double)))
    w = np.array(f.contents.center_weights[:2 * n + 1], f32)
    L.savgol_destroy(f)
    return terms, tab, w


def block_taps_d(tab, terms, n):
    """[r][t]: the tap output r applies to block sample t, sum_s c_s(r) phi_s(t) -- the back half's phi is (-1)^s times the front half's, as the
    kernel forms it from the front / back sums and differences"""
    off, lo, hi = geometry_d(n)
    bk = hi - lo
    phi = np.ones((terms, bk), f64)
    for s in range(1, terms):
        half = np.array([tab[D_OFF_PHI + t * 6 + s - 1] for t in range(bk // 2)], f64)
        phi[s, :bk // 2] = half
        phi[s, bk // 2:] = half[::-1] * (-1.0 if s & 1 else 1.0)
    c = np.stack([tab[D_OFF_C + s * 16:D_OFF_C + (s + 1) * 16] for s in range(terms)])               # [s][r]
    return c.T @ phi


def effective_taps_d(tab, terms, w, n):
    """the 16 tap sets the kernel really applies, [r][k]: block sample t is tap 15 + t - r of output r; the 15 taps on either side of the block are
    the promoted table itself (head: the table's doubles, tail: +- the same doubles through the table's exact (anti)symmetry)"""
    bk = 2 * n - 14
    w_eff = np.tile(w.astype(f64), (16, 1))
    blk = block_taps_d(tab, terms, n)
    for r in range(16):
        w_eff[r, 15 - r:15 - r + bk] = blk[r]
    return w_eff


def emulate_d(tab, terms, x, n, odd):
    """every 16-output group of x in the kernel's own order, in numpy double: head and tail tap by tap (the tail through tap[2n - k] = +-tap[k], the
    sign carried by the sample), block samples paired front to back into the moments, the block's share added last, highest moment first"""
    off, lo, hi = geometry_d(n)
    npair = (hi - lo) // 2
    W = tab[D_OFF_W:D_OFF_W + 15]
    groups = (len(x) - 2 * n) // 16
    xp = np.concatenate([np.zeros(off, f64), x, np.zeros(8, f64)])
    X = np.stack([xp[16 * g:16 * g + 16 + 2 * n + off] for g in range(groups)], axis=1)               # [i][group]
    A = np.zeros((16, groups), f64)
    for i in range(off, lo):
        for r in range(16):
            k = i - off - r
            if 0 <= k <= 14:
                A[r] = W[k] * X[i] + A[r]
    for j in range(1, 16):
        xs = -X[hi - 1 + j] if odd else X[hi - 1 + j]
        for r in range(16):
            km = r - j
            if 0 <= km <= 14:
                A[r] = W[km] * xs + A[r]
    M = np.zeros((terms, groups), f64)
    for t in range(npair):
        xf, xb = X[lo + t], X[hi - 1 - t]
        e, o = xf + xb, xf - xb
        M[0] = M[0] + e
        for s in range(1, terms):
            M[s] = tab[D_OFF_PHI + t * 6 + s - 1] * (o if s & 1 else e) + M[s]
    for s in range(terms - 1, -1, -1):
        for r in range(16):
            A[r] = tab[D_OFF_C + s * 16 + r] * M[s] + A[r]
    return A.T.reshape(-1)


def trended_inputs(length, seed):
    """the inputs of tests/test_gpu_1d.py's tolerance-path tests: sin(0.01 t) + N(0, 0.1) on an offset, a ramp, both, and one quadratic"""
    t = np.arange(length, dtype=f64)
    base = np.sin(0.01 * t) + np.random.default_rng(seed).normal(0, 0.1, length)
    cases = [(off, slope, 0.0) for off in (0.0, 10.0, 1e3) for slope in (0.0, 0.05, 0.5)] + [(1e3, 0.5, 1e-3)]
    return [((off, slope, curv), base + off + slope * t + curv * t * t) for off, slope, curv in cases]


def accepted_d(sg):
    for n in range(24, 33):
        for m, d in D_FILTERS:
            terms, tab, w = table_d(sg, n, m, d)
            if terms:
                yield n, m, d, terms, tab, w


def test_fp64_table_geometry_and_refusals(sg):
    assert sg.lib().savgol_hip_moment64_table(None, np.zeros(D_DOUBLES, f64).ctypes.data_as(C.POINTER(C.c_double))) == -1
    assert table_d(sg, 23, 4, 0)[0] == 0 and table_d(sg, 16, 4, 0)[0] == 0          # half windows below 24: the tap-by-tap kernel
    assert table_d(sg, 32, 8, 0)[0] == 0                                             # poly_order > 6
    for n in range(24, 33):
        off, lo, hi = geometry_d(n)
        assert (hi - lo) == 2 * n - 14 and (hi - lo) // 2 <= D_MAX_PAIRS and (lo + hi - 1) % 2 == 1
        for (m, d, want) in ((4, 0, 5), (4, 1, 5), (4, 2, 5), (2, 1, 3), (2, 2, 3), (3, 1, 5), (6, 2, 7), (5, 1, 7)):
            terms, tab, w = table_d(sg, n, m, d)
            if (n, m, d) == (31, 6, 2):
                assert terms == 0                      # the one of these whose fit misses a tap by more than 3e-7 of the largest: it keeps the tap-by-tap kernel
                continue
            assert terms == want, (n, m, d, terms)
            assert np.array_equal(tab[D_OFF_W:D_OFF_W + 15], w[:15].astype(f64))     # head / tail taps: the table's own, promoted exactly


def test_fp64_block_taps_keep_the_low_moments_of_the_table(sg):
    """What an offset, a ramp or a parabola under the signal multiplies.  The kernel replaces the 2n - 14 taps on a lane's common block by
    sum_s c_s(r) phi_s(t); the replaced taps differ from the promoted table by up to the table's own fp32 rounding (3e-7 of the largest tap), which is
    harmless on zero-mean data -- but a derivative filter's taps sum to ~0, so a constant c under the signal leaves c x (sum of the differences) in an
    output that does not contain c at all.  So the differences' moments of order 0, 1, 2 over the window must vanish, per output slot r:
        | sum_k (w_eff[r][k] - w[k]) ((k - n) / n)^j |  /  sum_k |w[k]|   at rounding level,   j = 0, 1, 2.
    The bar comes from the arithmetic, not from a run: c_s(r) is a least-squares fit on the block (normal equations of <= 7 near-orthogonal Legendre
    columns over <= 50 points, Gaussian elimination in double), whose residual is orthogonal to every polynomial of degree < terms (>= 3) up to the
    solve's rounding -- a few hundred ulps of double relative to sum|w|: 1e-13 (450 ulps).  A table built from a polynomial fitted to the WHOLE window
    instead measures 2e-9 ... 1e-8 at j = 0 here, which times an offset of 1e3 is 1e-5 ... 1e-4 of the output of a second-derivative filter."""
    worst = [(0.0, None)] * 3
    covered = 0
    for n, m, d, terms, tab, w in accepted_d(sg):
        covered += 1
        w64 = w.astype(f64)
        delta = effective_taps_d(tab, terms, w, n) - w64[None, :]
        z = (np.arange(2 * n + 1) - n) / n
        for j in range(3):
            v = np.abs(delta @ z ** j) / np.sum(np.abs(w64))
            r = int(np.argmax(v))
            if v[r] > worst[j][0]:
                worst[j] = (float(v[r]), (n, m, d, r, terms))
    print(f"fp64 moment tables checked: {covered}; worst |moment j of (w_eff - w)| / sum|w|: " + ", ".join(f"j={j}: {worst[j][0]:.3e} at {worst[j][1]}" for j in range(3)))
    assert covered >= 9 * 20, covered          # 25 (poly_order, derivative) pairs per half window; the fit may refuse a few (it decides, not this test)
    for j in range(3):
        assert worst[j][0] <= 1e-13, (j, worst[j])


def test_every_fp64_moment_table_is_compatible_with_the_1e6_bar(sg):
    """The fp64 sibling of test_every_moment_table_is_compatible_with_the_1e6_bar, same quantity and same 1.5e-7: per unit of input amplitude output r
    carries E_r = sum_t |sum_s c_s(r) phi_s(t) - w[15 + t - r]| against sum|w|, for EVERY filter savgol_create builds at half windows 24..32 with
    poly_order <= 6 that the fit accepts (printed with -s)."""
    worst = (0.0, None)
    covered = 0
    for n, m, d, terms, tab, w in accepted_d(sg):
        covered += 1
        w64 = w.astype(f64)
        e = np.sum(np.abs(effective_taps_d(tab, terms, w, n) - w64[None, :]), axis=1) / np.sum(np.abs(w64))
        if e.max() > worst[0]:
            worst = (float(e.max()), (n, m, d, int(np.argmax(e)), terms))
    print(f"fp64 moment tables checked: {covered}; worst block error / sum|w| = {worst[0]:.3e} at (n, m, d, r, terms) = {worst[1]}")
    assert covered >= 9 * 20, covered
    assert worst[0] <= 1.5e-7, worst


@pytest.mark.parametrize("n", [32, 31, 30, 29, 28, 27, 26, 25, 24])
def test_fp64_table_in_the_kernels_order_on_offsets_and_ramps(sg, n):
    """The table rebuilt into outputs in the kernel's own order (numpy double) on signals that are NOT zero-mean -- offsets 0 / 10 / 1e3, ramps of
    0.05 and 0.5 per sample, a parabola -- against the double convolution with the promoted fp32 taps: 1e-6, the tolerance the call states
    (include/savgol_hip.h, savgol_apply_batch_f64_tol).  No GPU: this is the check that sees a block share that does not keep the table's low moments."""
    length = 16 * 96 + 2 * n
    inputs = trended_inputs(length, 640 + n)
    for m, d in [(4, 0), (4, 1), (4, 2), (2, 1), (2, 2), (3, 1), (6, 2), (5, 1)]:
        terms, tab, w = table_d(sg, n, m, d)
        if (n, m, d) == (31, 6, 2):
            continue                                   # refused by the fit (test_fp64_table_geometry_and_refusals): no table to emulate
        assert terms > 0, (n, m, d)
        for label, x in inputs:
            got = emulate_d(tab, terms, x, n, d & 1)
            ref = np.convolve(x, w[::-1].astype(f64), "valid")[:len(got)]
            # the referee's own rounding must be far below the bar, or the comparison says nothing
            assert np.max(np.abs(x)) * 2.0 ** -53 * np.sum(np.abs(w.astype(f64))) / np.max(np.abs(ref)) < 1e-8, (n, m, d, label)
            err = np.max(np.abs(got - ref)) / np.max(np.abs(ref))
            assert err < 1e-6, f"n={n} m={m} d={d} (offset, slope, curvature)={label}: normwise error {err:.3e}"
