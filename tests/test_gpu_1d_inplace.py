"""In-place 1-D batch calls (d_out == d_in) at every tile seam and tile width, through the C ABI.

The contract (include/savgol_hip.h): an in-place call returns the OUT-OF-PLACE answer bit for bit.  enqueue_batch (csrc/sg_api_1d.cpp) gets there in
four steps -- sg1d_ends_kernel puts aside what reaches past a channel's end, the even tiles run and hand their first / last NA samples to their odd
neighbours' stash slots, the odd tiles run from those slots, the POLYNOMIAL edge rows run from edge_stash -- and the kernel half (sg1d_tile_body,
csrc/sg_k1d.hpp, the job.phase blocks) branches on the shape of the LAST tile: a last tile of fewer than NA samples makes tile T-2 take its right halo
from the third `ends` slot (T even) or fills its odd neighbour's slot partly from rows and partly from remapped samples (T odd).  This file holds
those seams:
  1. test_in_place_seam_matrix: channel lengths (T-1) TW + r for T = 2..5 and r around NA, at the narrow AND the wide tile, every boundary mode, every
     kernel family a flag word can select, three row layouts -- in place == out of place bit for bit, out of place within the project's bar of the fp64
     oracle, every guard element untouched;
  2. test_in_place_across_stash_groups: more channels than one stash group holds (the groups only occurred in the full-size config 5 test);
  3. test_in_place_takes_the_wide_tile_by_job_size: the automatic wide choice, in place.
Bars: the ones of tests/test_gpu_1d.py and no other -- fp32 bar32() = max(1e-6, 1.1 x the reference's own fp32 error on the same samples), fp64 1e-12,
fp64 block moments 1e-6 (the header's), the reference-order flag bit identity with the oracle's restatement of the reference."""
import os

import numpy as np
import pytest

from tests._util import check, fp32_bar, normwise

pytestmark = pytest.mark.gpu

GUARD = -7.0
POLYNOMIAL, PERIODIC = 0, 2
F32_HALF_WINDOWS = [1, 4, 5, 12, 13, 18, 19, 20, 23, 24, 31, 32]       # the edges of wide_vectors_per_lane, MOMENTH_MIN_N / MOMENT_MIN_N, NA == n / NA > n
F64_HALF_WINDOWS = [1, 2, 3, 16, 24, 25, 32]
MOMENTH_MIN_N, MOMENT_MIN_N = 20, 24                                    # csrc/sg_k1d_host.hpp


@pytest.fixture(scope="module")
def torch_gpu(sg):
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    assert sg.device_count() > 0, sg.last_error()
    return torch


def signal(rng, shape):
    """a tone plus white noise of comparable size: adjacent samples differ, so a halo one sample off (or from the wrong slot) moves outputs by far more than any bar"""
    t = np.arange(shape[-1], dtype=np.float64)
    return np.sin(0.013 * t) * 2.0 + 0.3 * np.sin(0.41 * t + 1.0) + rng.normal(0, 0.2, shape)


def elems_per_vector(dtype):
    return 4 if dtype == "f32" else 2


def halo(dtype, n):
    """NA: the half window rounded up to whole 16-byte vectors (K1D::NA)"""
    e = elems_per_vector(dtype)
    return (n + e - 1) // e * e


def narrow_tile(dtype):
    return 64 * 8 * elems_per_vector(dtype)


def wide_tile(dtype, n):
    """the wide tile's width where one is built (wide_vectors_per_lane, csrc/sg_k1d_host.hpp), else None"""
    if dtype == "f32":
        vpl = 16 if n <= 12 else 12 if n <= 18 else 8
    else:
        vpl = 16 if n <= 24 else 8
    return 64 * vpl * elems_per_vector(dtype) if vpl != 8 else None


def seam_lengths(dtype, n, tw):
    na = halo(dtype, n)
    rs = sorted({r for r in (1, n, na - 1, na, na + 1, tw) if 1 <= r <= tw})
    return [(t, r, (t - 1) * tw + r) for t in (2, 3, 4, 5) for r in rs if (t - 1) * tw + r >= 2 * n + 1]


def layouts(dtype, length):
    """(name, element offset of the base, pitch): 16-byte aligned rows with slack | an odd pitch (rows 1 and 2 unaligned: every tile on the element path) |
    a base shifted by one element"""
    e = elems_per_vector(dtype)
    aligned = (length + e - 1) // e * e + e
    odd = length + 1 + (length % 2)
    return [("aligned", 0, aligned), ("odd pitch", 0, odd), ("shifted base", 1, aligned)]


def where(got, want, tw, length):
    """the failing coordinates of a bitwise mismatch: channel, sample, tile, side"""
    bad = np.argwhere(got != want)
    if bad.size == 0:
        return "NaN-only difference"
    tiles = (length + tw - 1) // tw
    spots = []
    for c, i in bad[:1].tolist() + bad[-1:].tolist():
        k, p = divmod(i, tw)
        body = min(tw, length - k * tw)
        spots.append(f"channel {c} sample {i} = tile {k} of {tiles} ({'even' if k % 2 == 0 else 'odd'} phase), {p} from its left end, {body - 1 - p} from its right end")
    return f"{len(bad)} samples differ; first: {spots[0]}; last: {spots[1]}"


class Rows:
    """`channels` rows of `length` samples at pitch `ld`, `off` elements into a buffer pre-filled with GUARD (and 8 elements of it behind the last row)"""

    def __init__(self, torch, tdt, channels, length, off, ld):
        self.buf = torch.full((off + channels * ld + 8,), GUARD, dtype=tdt, device="cuda")
        self.rows = self.buf[off:off + channels * ld].view(channels, ld)
        self.ptr = self.buf.data_ptr() + off * self.buf.element_size()
        self.off, self.ld, self.channels, self.length = off, ld, channels, length

    def guards_intact(self, host):
        rows = host[self.off:self.off + self.channels * self.ld].reshape(self.channels, self.ld)
        return bool(np.all(host[:self.off] == GUARD) and np.all(rows[:, self.length:] == GUARD) and np.all(host[self.off + self.channels * self.ld:] == GUARD))


# ------------------------------------------------------------------------------------------------
# 1. the seam matrix
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype,n", [("f32", n) for n in F32_HALF_WINDOWS] + [("f64", n) for n in F64_HALF_WINDOWS])
def test_in_place_seam_matrix(sg, sgo, torch_gpu, dtype, n):
    """Three channels of (T-1) TW + r samples, T = 2..5 (T = 2: tile 0 is also tile T-2; T = 3, 5: an even last tile; T = 4: an odd one), r in
    {1, n, NA-1, NA, NA+1, TW}, TW the narrow tile (SAVGOL_BATCH_TILE_NARROW) and, where one is built, the wide tile (SAVGOL_BATCH_TILE_WIDE); a smoothing
    filter (m = min(4, 2n)) and a first derivative (dt = 0.5: JOB_CENTRE on fp32, JOB_ODD_TAPS on fp64); all four boundary modes; flag words NARROW, WIDE,
    NARROW | PLAIN_SUMMATION (fp32 n >= 20, where NARROW alone is the block-moment route), NARROW | MOMENT_F64 (fp64 n >= 24), each also with
    CORRECT_LEADING_EDGE for the derivative in POLYNOMIAL mode (edge items reading edge_stash with JOB_EDGE_NEGATE), and REFERENCE_SUMMATION (the
    staged-copy route) at one length; three row layouts in guarded buffers.  For every case:
      (a) the in-place buffer equals the out-of-place buffer of the same call bit for bit -- rows and guards, compared whole on the device;
      (b) the out-of-place rows are within the bar of the fp64 oracle (module docstring), through check();
      (c) every guard element of the out-of-place buffer -- pitch slack, in front of a shifted base, behind the last row -- is untouched (so, by (a), of
          the in-place one)."""
    torch = torch_gpu
    f32 = dtype == "f32"
    tdt, ndt = (torch.float32, np.float32) if f32 else (torch.float64, np.float64)
    na, channels = halo(dtype, n), 3
    NARROW, WIDE, PLAIN, CLE, MOM64, REFSUM = (sg.SAVGOL_BATCH_TILE_NARROW, sg.SAVGOL_BATCH_TILE_WIDE, sg.SAVGOL_BATCH_PLAIN_SUMMATION,
                                               sg.SAVGOL_BATCH_CORRECT_LEADING_EDGE, sg.SAVGOL_BATCH_MOMENT_F64, sg.SAVGOL_BATCH_REFERENCE_SUMMATION)
    narrow_words = [NARROW]
    if f32 and n >= MOMENTH_MIN_N:
        narrow_words.append(NARROW | PLAIN)
    if not f32 and n >= MOMENT_MIN_N:
        narrow_words.append(NARROW | MOM64)
    widths = [(narrow_tile(dtype), narrow_words)]
    if wide_tile(dtype, n):
        widths.append((wide_tile(dtype, n), [WIDE]))
    m = min(4, 2 * n)
    configs = [(m, 0, 1.0), (m, 1, 0.5)]
    filters = []
    for (m_, d, dt) in configs:
        try:
            o = sgo.Filter(n, m_, d, dt, 0)
        except ValueError:                                     # not a valid configuration: the library must refuse it too
            with pytest.raises(ValueError):
                sg.Filter(n, m_, d, dt, 0)
            continue
        filters.append((d, o, [sg.Filter(n, m_, d, dt, mode) for mode in range(4)]))
    assert filters
    rng = np.random.default_rng(7000 + 64 * f32 + n)
    combos = calls = 0

    def run_length(tw, t, r, length, words):
        nonlocal combos, calls
        xh = signal(rng, (channels, length)).astype(ndt)
        xd = torch.from_numpy(xh).cuda()
        bufs = [(name, Rows(torch, tdt, channels, length, off, ld), Rows(torch, tdt, channels, length, off, ld)) for (name, off, ld) in layouts(dtype, length)]
        for d, o, by_mode in filters:
            for mode in range(4):
                ref64 = o.apply_f64(xh.astype(np.float64), mode=mode)
                ref32 = o.apply(xh, mode=mode) if f32 else None
                bar = fp32_bar(normwise(ref32, ref64)) if f32 else 1e-12          # bar32() of tests/test_gpu_1d.py: the reference's own fp32 error on these samples
                fixed64, fixed32 = ref64, ref32
                if d % 2 == 1 and mode == POLYNOMIAL:                              # CORRECT_LEADING_EDGE: the first n outputs with the sign the derivative has
                    fixed64 = ref64.copy(); fixed64[:, :n] = -fixed64[:, :n]
                    if f32:
                        fixed32 = ref32.copy(); fixed32[:, :n] = -fixed32[:, :n]
                f = by_mode[mode]
                for base in words:
                    for flags in [base] + ([base | CLE] if d % 2 == 1 and mode == POLYNOMIAL else []):
                        want64, want32 = (fixed64, fixed32) if flags & CLE else (ref64, ref32)
                        combos += 1
                        for name, src, dst in bufs:
                            label = (dtype, n, d, mode, hex(flags), tw, t, r, name)
                            calls += 1
                            src.rows[:, :length] = xd
                            dst.buf.fill_(GUARD)
                            f.apply_batch(src.ptr, dst.ptr, channels, length, src.ld, dst.ld, dtype=dtype, flags=flags)
                            f.apply_batch(src.ptr, src.ptr, channels, length, src.ld, src.ld, dtype=dtype, flags=flags)
                            same = torch.equal(src.buf, dst.buf)                  # (a), and the in-place guards
                            host = dst.buf.cpu().numpy()
                            out = host[dst.off:dst.off + channels * dst.ld].reshape(channels, dst.ld)[:, :length]
                            if not same:
                                inpl = src.buf.cpu().numpy()
                                got = inpl[src.off:src.off + channels * src.ld].reshape(channels, src.ld)[:, :length]
                                assert src.guards_intact(inpl), ("in place wrote outside its rows", label)
                                assert False, ("in place differs from out of place", label, where(got, out, tw, length))
                            assert dst.guards_intact(host), ("out of place wrote outside its rows", label)                       # (c)
                            if flags & REFSUM and f32:
                                check(float(np.count_nonzero(out.view(np.uint32) != want32.view(np.uint32))), 0.5, ("words that differ from the reference's",) + label)
                            else:
                                check(normwise(out, want64), 1e-6 if flags & MOM64 else bar, label)                              # (b)

    for tw, words in widths:
        for t, r, length in seam_lengths(dtype, n, tw):
            run_length(tw, t, r, length, words)
    # the reference-order flag (fp32: the in-place call runs from a stream-ordered copy of the input; fp64 has no such kernel and ignores the flag): one length
    tw = narrow_tile(dtype)
    run_length(tw, 4, na - 1, 3 * tw + na - 1, [REFSUM])
    print(f"{dtype} n={n}: {combos} (shape, filter, mode, flags) combinations, {calls} in-place calls over three layouts")


# ------------------------------------------------------------------------------------------------
# 2. more than one stash group
# ------------------------------------------------------------------------------------------------
def stash_group_channels(dtype, n, length):
    """channels per stash group of an in-place call, by enqueue_batch's own formula (csrc/sg_api_1d.cpp): the group's stash -- one slot of 2 NA samples per
    odd tile + 4 NA per channel -- stays below 3/4 of what the scratch pool keeps (256 MiB unless SAVGOL_HIP_SCRATCH_KEEP_MB says otherwise), at least 64 MiB"""
    keep_mb = 256
    try:
        if int(os.environ.get("SAVGOL_HIP_SCRATCH_KEEP_MB", "")) >= 0:
            keep_mb = int(os.environ["SAVGOL_HIP_SCRATCH_KEEP_MB"])
    except ValueError:
        pass
    cap = max((keep_mb << 20) // 4 * 3, 64 << 20)
    tw, na, esz = narrow_tile(dtype), halo(dtype, n), 4 if dtype == "f32" else 8
    tpc = (length + tw - 1) // tw
    per_ch = ((tpc // 2) * 2 * na + 4 * na) * esz
    return cap // per_ch


@pytest.mark.parametrize("shape", ["one_tile", "two_tiles"])
@pytest.mark.parametrize("dtype", ["f32", "f64"])
def test_in_place_across_stash_groups(sg, sgo, torch_gpu, dtype, shape):
    """An in-place call works through channel groups, each with a stash of its own and its own stretch of edge_all (edge_all + c0 2 ws); until now more than
    one group only occurred in the full-size config 5 test.  n = 32, a few channels more than one group holds, (i) channels of one tile (2n + 1 samples)
    and (ii) of two tiles with 9 samples in the second; POLYNOMIAL (the second group's edge rows read edge_all past c0) and PERIODIC (tile 0's left halo
    comes from the channel's other end).  In place == out of place bit for bit over the whole batch, pitch slack included, compared on the device; oracle
    parity on the first channel, the last of group 0, the first of group 1 and the last one."""
    torch = torch_gpu
    f32 = dtype == "f32"
    tdt, esz = (torch.float32, 4) if f32 else (torch.float64, 8)
    n, m = 32, 4
    tw, e = narrow_tile(dtype), elems_per_vector(dtype)
    length = 2 * n + 1 if shape == "one_tile" else tw + 9
    group = stash_group_channels(dtype, n, length)
    channels = group + 5
    groups = (channels + group - 1) // group
    assert groups == 2
    ld = (length + e - 1) // e * e + e
    torch.cuda.empty_cache()
    free, _ = torch.cuda.mem_get_info()
    if free < 3 * channels * ld * esz + (2 << 30):
        pytest.skip(f"not enough HBM free for three buffers of {channels * ld * esz / 2**30:.1f} GiB")
    x = torch.empty((channels, ld), dtype=tdt, device="cuda")
    sg.synth(x, channel0=5)
    x[:, length:] = GUARD
    y = torch.empty_like(x)
    z = torch.empty_like(x)
    sample = [0, group - 1, group, channels - 1]
    xs = x[sample, :length].cpu().numpy()
    for mode in (POLYNOMIAL, PERIODIC):
        f = sg.Filter(n, m, 0, 1.0, mode)
        y.fill_(GUARD)
        z.copy_(x)
        f.apply_batch(x, y, channels, length, ld, ld, dtype=dtype, flags=0)
        f.apply_batch(z, z, channels, length, ld, ld, dtype=dtype, flags=0)
        if not torch.equal(z, y):
            rows = torch.nonzero((z != y).any(dim=1)).flatten()
            assert False, ("in place differs from out of place", dtype, shape, mode, f"{rows.numel()} channels, first {int(rows[0])}, last {int(rows[-1])}; group 1 starts at {group}")
        assert bool((y[:, length:] == GUARD).all()), ("pitch slack written", dtype, shape, mode)
        o = sgo.Filter(n, m, 0, 1.0, mode)
        ref = o.apply_f64(xs.astype(np.float64))
        got = y[sample, :length].cpu().numpy()
        bar = fp32_bar(normwise(o.apply(xs), ref)) if f32 else 1e-12
        for i, c in enumerate(sample):
            check(normwise(got[i], ref[i]), bar, ("stash groups", dtype, shape, mode, "channel", c))
    print(f"{dtype} {shape}: {channels} channels of {length} samples in {groups} stash groups of {group}")


# ------------------------------------------------------------------------------------------------
# 3. the automatic wide choice, in place
# ------------------------------------------------------------------------------------------------
def test_in_place_takes_the_wide_tile_by_job_size(sg, torch_gpu):
    """fp32, n = 8, 72 channels of 2^20 + 77 samples on a padded pitch (the shape of test_wide_tile_kernels_on_batches_big_enough_to_select_them): 18504 wide
    tiles, so flags 0 selects the 16-vector tile -- what a production-sized in-place call runs.  In place == out of place bit for bit, slack included, and two
    of its channels equal the SAVGOL_BATCH_TILE_NARROW call on them (a smoothing filter gives the same bits at either width)."""
    torch = torch_gpu
    n, ch, length, ld = 8, 72, (1 << 20) + 77, (1 << 20) + 80
    assert ch * ((length + 4095) // 4096) >= 16384                # WIDE_TILE_MIN_TILES
    x = torch.empty((ch, ld), dtype=torch.float32, device="cuda")
    sg.synth(x)
    x[:, length:] = GUARD
    y, z = torch.empty_like(x), torch.empty_like(x)
    two = [34, 71]
    for mode in range(4):
        f = sg.Filter(n, 4, 0, 1.0, mode)
        y.fill_(GUARD)
        z.copy_(x)
        f.apply_batch(x, y, ch, length, ld, ld, flags=0)
        f.apply_batch(z, z, ch, length, ld, ld, flags=0)
        if not torch.equal(z, y):
            rows = torch.nonzero((z != y).any(dim=1)).flatten()
            c = int(rows[0])
            cols = torch.nonzero(z[c] != y[c]).flatten()
            assert False, ("in place differs from out of place", mode, f"{rows.numel()} channels; channel {c}: {cols.numel()} samples, first {int(cols[0])} (tile {int(cols[0]) // 4096})")
        assert bool((y[:, length:] == GUARD).all()), mode
        for c in two:
            w = torch.full((1, ld), GUARD, dtype=torch.float32, device="cuda")
            f.apply_batch(x[c:c + 1], w, 1, length, ld, ld, flags=sg.SAVGOL_BATCH_TILE_NARROW)
            assert torch.equal(w[0], z[c]), (mode, c)
