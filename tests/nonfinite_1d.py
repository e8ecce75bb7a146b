"""The reference's NaN / Inf footprint on 1-D batches, restated twice, and the signals the GPU tests of tests/test_gpu_1d_nonfinite.py run on.

The reference's loops skip no tap (convolve_ilp, src/savgolFilter.c:547-580; the padded edges :789-800 through get_padded_sample :442-482; the POLYNOMIAL edge
rows :773-784 apply all 2n + 1 taps of a row to the first / last 2n + 1 samples), so one non-finite sample makes non-finite exactly the outputs whose window,
after the boundary remap, contains it -- a zero tap times NaN or Inf is NaN too.
  1. from the oracle:  ~isfinite(sgo.Filter(...).apply_f64(x)); for VALID that output's [n : L - n]                                   (oracle_footprint)
  2. geometrically:    output o is hit iff some non-finite x[i] has i among remap(o - n) .. remap(o + n); remap = the reference's get_padded_sample for modes
                       1-3; mode 0 (POLYNOMIAL): the first / last n outputs are hit iff any of the first / last 2n + 1 samples is special; VALID stores the
                       interior and remaps nothing                                                                                      (footprint)
tests/test_nonfinite_1d_rule.py (CPU) holds the two together; the GPU tests take their expected values from the oracle only.

The signals.  Background: the signal() of tests/test_gpu_1d.py (two sines plus noise, zero offset).  Length 2 * 4096 + 2048 + 253 = 10493: whole interior tiles,
seams and a partial, unaligned last tile at every tile width the kernels have (1024, 2048 and 4096 samples), written here as numbers -- nothing is imported from
the library.  The channels, in order:
  * D "staircase" channels.  A NaN staircase of 64 steps and a +-Inf staircase of 64 steps (signs alternating) are dealt over them: step k of a staircase goes
    to channel k % D, slot k // D of that staircase's run of slots, and sits k % 64 samples into its slot.  Slots are S samples apart, S a multiple of 64 and at
    least 4 (2n + 1), and the first slot starts on a multiple of 64: so a step's position is k mod 64 -- every residue mod 64 is met by a NaN and by an Inf (both
    halves of an output pair, all 32 outputs of a lane, both 16-output groups of the block-moment kernel, head, block and tail of its window), and no two steps
    share a window.  S is stretched as far as both runs of slots fit; the NaN run starts 4n + 64 samples into the channel, the Inf run ends as far from its end.
    The channel ENDS are dealt over the same channels: samples 0, n - 1, n, 2n, L - 1 - 2n, L - 1 - n, L - 1 (the last sample of the POLYNOMIAL edge window among
    them), alternating NaN, +Inf, -Inf.
  * one channel with the tile SEAMS, sample pairs (1023, 1024), (2047, 2048), (4095, 4096), (8191, 8192), each pair two different specials, and the
    SAME-WINDOW PAIRS: +Inf and -Inf n apart (at 3000), +Inf and +Inf n apart (at 6000).
  * a CONTROL channel with no special at all.
D is the smallest count (at least 2, so at least 4 channels) at which the staircases fit and every channel's non-finite share of its stored outputs is at most
MAX_SHARE under all four modes and VALID: a condition on the signal, not a measurement of a kernel -- the comparison of the finite outputs cannot be emptied."""
import functools

import numpy as np

POLYNOMIAL, REFLECT, PERIODIC, CONSTANT, VALID = 0, 1, 2, 3, 4          # VALID: not a boundary mode of the library, the _valid entry points
MODES = (POLYNOMIAL, REFLECT, PERIODIC, CONSTANT, VALID)
SENTINEL = -5.0
MAX_SHARE = 0.25
LENGTH = 2 * 4096 + 2048 + 253
STEPS = 64
SEAMS = ((1023, 1024), (2047, 2048), (4095, 4096), (8191, 8192))
PAIR_OPPOSITE, PAIR_SAME = 3000, 6000
MAX_STAIR_CHANNELS = 16
NAN, PINF, NINF = np.float32(np.nan), np.float32(np.inf), np.float32(-np.inf)


def remap(i, length, mode):
    """the index get_padded_sample reads for index i (src/savgolFilter.c:442-482), modes 1-3"""
    if 0 <= i < length:
        return i
    if mode == REFLECT:
        if i < 0:
            return min(-i - 1, length - 1)
        return max(2 * length - i - 1, 0)
    if mode == PERIODIC:
        return i % length
    assert mode == CONSTANT
    return 0 if i < 0 else length - 1


def stored(length, n, mode):
    """the outputs a call writes, as a mask over the channel's samples: all of them, or VALID's interior (which the call stores from out[0] on)"""
    sel = np.ones(length, bool)
    if mode == VALID:
        sel[:n] = False
        sel[length - n:] = False
    return sel


def footprint(bad, n, mode):
    """restatement 2: bad = mask [channels][length] of the input samples in question; returns the mask of the stored outputs whose window holds one of them"""
    bad = np.atleast_2d(bad)
    channels, length = bad.shape
    hit = np.zeros((channels, length), bool)
    count = np.concatenate([np.zeros((channels, 1), np.int64), np.cumsum(bad, axis=1)], axis=1)
    o = np.arange(n, length - n)
    hit[:, n:length - n] = count[:, o + n + 1] - count[:, o - n] > 0                      # the interior: samples o - n .. o + n, no remap
    if mode == POLYNOMIAL:
        hit[:, :n] = bad[:, :2 * n + 1].any(axis=1)[:, None]                              # the edge rows use every tap on the 2n + 1 samples of their end
        hit[:, length - n:] = bad[:, length - 2 * n - 1:].any(axis=1)[:, None]
    elif mode != VALID:
        for e in list(range(n)) + list(range(length - n, length)):
            idx = sorted({remap(e + w, length, mode) for w in range(-n, n + 1)})
            hit[:, e] = bad[:, idx].any(axis=1)
    return hit & stored(length, n, mode)[None, :]


def oracle_output(o, x, mode):
    """the oracle's fp64 output for `mode` in the coordinates of the input: VALID is the interior of the full-length output (the centre loop is the same loop)"""
    return o.apply_f64(np.asarray(x, np.float64), POLYNOMIAL if mode == VALID else mode)


def oracle_footprint(o, x, mode):
    """restatement 1: where the oracle's fp64 output is not finite, among the stored outputs; returns (footprint, the fp64 output)"""
    hi = oracle_output(o, x, mode)
    return ~np.isfinite(hi) & stored(x.shape[1], o.n, mode)[None, :], hi


def background(channels, length, seed):
    """signal() of tests/test_gpu_1d.py"""
    rng = np.random.default_rng(seed)
    t = np.arange(length, dtype=np.float64)
    return (np.sin(0.013 * t) * 2.0 + 0.3 * np.sin(0.41 * t + 1.0) + rng.normal(0, 0.2, (channels, length))).astype(np.float32)


def slot_pitch(n, stair_channels, length=LENGTH):
    """(first slot, S) of the staircases dealt over `stair_channels` channels, or None when they do not fit: both a multiple of 64, S at least 4 (2n + 1) and
    stretched over the channel; the first and the last slot stay 4n + 64 samples away from the channel's ends (the ends' specials have these to themselves)"""
    base = (4 * n + 64 + 63) // 64 * 64
    slots = 2 * ((STEPS + stair_channels - 1) // stair_channels)
    pitch = (length - 2 * base - 64) // slots // 64 * 64
    least = (4 * (2 * n + 1) + 63) // 64 * 64
    return (base, pitch) if pitch >= least else None


def specials(n, stair_channels, length=LENGTH):
    """{name: [(channel, sample, value)]} for a batch of stair_channels + 2 channels"""
    base, pitch = slot_pitch(n, stair_channels, length)
    per = (STEPS + stair_channels - 1) // stair_channels
    base_inf = (length - base - 64 - (per - 1) * pitch) // 64 * 64                       # the Inf staircase ends where the NaN staircase's margin begins, mirrored
    assert base_inf >= base + per * pitch
    out = {"nan_stair": [], "inf_stair": [], "ends": [], "seams": [], "pairs": []}
    for k in range(STEPS):
        out["nan_stair"].append((k % stair_channels, base + (k // stair_channels) * pitch + k % 64, NAN))
        out["inf_stair"].append((k % stair_channels, base_inf + (k // stair_channels) * pitch + k % 64, PINF if k % 2 == 0 else NINF))
    ends = []
    for s in (0, n - 1, n, 2 * n, length - 1 - 2 * n, length - 1 - n, length - 1):
        if s not in ends:                                                                  # n = 1: n - 1 is sample 0
            ends.append(s)
    out["ends"] = [(k % stair_channels, s, (NAN, PINF, NINF)[k % 3]) for k, s in enumerate(ends)]
    seam_channel = stair_channels
    for k, (a, b) in enumerate(SEAMS):
        out["seams"] += [(seam_channel, a, (NAN, PINF, NINF)[k % 3]), (seam_channel, b, (NAN, PINF, NINF)[(k + 1) % 3])]
    out["pairs"] = [(seam_channel, PAIR_OPPOSITE, PINF), (seam_channel, PAIR_OPPOSITE + n, NINF), (seam_channel, PAIR_SAME, PINF), (seam_channel, PAIR_SAME + n, PINF)]
    return out


def shares(x, n):
    """[mode][channel]: non-finite share of the stored outputs, by the geometric rule"""
    bad = ~np.isfinite(x)
    return np.array([footprint(bad, n, mode).sum(axis=1) / stored(x.shape[1], n, mode).sum() for mode in MODES])


@functools.lru_cache(maxsize=None)
def signals_for(n):
    """(x [channels][LENGTH] fp32 (read-only), number of specials, largest share over channels and modes, stair channels) for the half window n"""
    for stair_channels in range(2, MAX_STAIR_CHANNELS + 1):
        if slot_pitch(n, stair_channels) is None:
            continue
        x = background(stair_channels + 2, LENGTH, 4409 * n + 7)
        placed = [p for group in specials(n, stair_channels).values() for p in group]
        for c, s, v in placed:
            assert 0 <= s < LENGTH and np.isfinite(x[c, s]), ("a special on another, or outside the channel", n, c, s)
            x[c, s] = v
        worst = float(shares(x, n).max())
        if worst <= MAX_SHARE:
            break
    assert worst <= MAX_SHARE, (n, worst)                                                  # the share cap: a condition on the signal
    assert int((~np.isfinite(x)).sum()) == len(placed) and np.isfinite(x[-1]).all()
    x.setflags(write=False)
    return x, len(placed), worst, stair_channels
