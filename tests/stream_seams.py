"""The seam matrix of savgol_streambank_push_block, as plain functions (not collected by pytest; tests/test_gpu_stream_seams.py runs it in-process and,
under the environment switches, as `python -m tests.stream_seams ...` in a fresh child process; tests/test_stream_block_forms.py accounts for it on a CPU).

One entry point, four kernel families (block-moment tiles, LDS-DMA tiles, register tiles, the walk), picked by block_form (csrc/sg_stream_host.hpp) from
the half window, the bank's summation, the stream count, the call's length and the pointers' alignment.  A CASE is a fresh bank plus a sequence of calls
-- ("tick", k) = k single pushes, ("block", L) = one push_block -- on samples and outputs that live inside larger tensors pre-filled with a guard value.
After every call: return value and counters against the oracle's (oracle/sgo.py Stream on stream 0); the output rows of every stream; rows of ticks
without an output still the guard, bit for bit; every guard element around d_out; d_samples and its guards unchanged.  After the last call both flushes
on every stream, bit for bit on both banks, then 2n + 1 more tick pushes so the ring the block push left is consumed whole.

Expected values never come from the code under test.  The CPU restatement sums in the reference's order -- acc = 0; acc = acc + w[k] * x[k : k + M] for
k = 0 .. 2n in float32, then * dt_inv in float32 (taps and dt_inv from oracle/sgo.py) -- and self_check() pins it to sgo.Stream bit for bit; every case
pins stream 0 again.  Bars: the bit-exact bank 0 differing words over every stream; the fused bank check(normwise(got, ref64), fp32_bar(e_ref)) over the
whole bank with e_ref = normwise(restatement, ref64) on the same outputs (tests/_util.py: the project's one rule)."""
import argparse
import atexit
import collections
import ctypes as C
import os
import shutil
import subprocess
import sys
import tempfile

import numpy as np

from tests._util import bits, check, fp32_bar, normwise, same_bits

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32, f64 = np.float32, np.float64

# every seam in the half window: 5|6, 10|11 tile shapes of launch_bank_dma_shape; 12|13 register tiles, STREAM_MOMENT_MIN_N; 16|17 sample ring | accumulator
# ring, sg_bank_dma_launch_lo|hi; 19|20|21 the bit-exact bank's DMA rule, STREAM_MOMENT_MAX_N; 24|25, 28 PA / UA of bank_accroll_item
HALF_WINDOWS = [1, 5, 6, 10, 11, 12, 13, 16, 17, 19, 20, 21, 24, 25, 28, 32]
DMA_LENGTHS = (63, 64, 65, 95, 96, 97)                      # 32-tick tiles, at least 64 ticks: 63 falls through to the register tiles or the walk
REGISTER_LENGTHS = (31, 32, 33, 47, 48, 49)                 # 16-tick tiles, at least 32 ticks: 31 is the walk
GUARD = f32(-7.0)
GUARD_ROWS = 2
COST_LIMIT = 1.5e9                                          # sum of ticks x streams x (2n + 1) over one (n, fma): the CPU restatement's cost


def walk_lengths(n):
    ws = 2 * n + 1
    return (1, 2, 2 * n, ws, ws + 1, 16 * ws - 1, 16 * ws, 24 * ws + 5)      # from 16 ws the band search may take two bands; the last takes three, the last shorter


Case = collections.namedtuple("Case", "name streams off_in off_out n m d dt fma offset calls")


def bank_filters(n, fma):
    """(m, d, dt) of the banks a half window is run with, where the oracle accepts them.  Bit-exact: a smoothing filter and config 3's kind.  Fused: taps
    that are no polynomial of degree <= 2 (tap-by-tap tiles) | one moment | linear taps, centred, two moments | three moments | quadratic taps summing to
    zero (centre && terms >= 3: keeps the tap-by-tap tiles, centred)."""
    from oracle import sgo
    cand = [(min(4, 2 * n), 0, 1.0), (2, 1, 1e-3)]
    if fma:
        cand = [(min(4, 2 * n), 0, 1.0), (0, 0, 1.0), (2, 1, 1e-3), (2, 0, 1.0), (2, 2, 0.5)]
    out = []
    for f in cand:
        if f not in out and f[0] <= 2 * n and sgo.weights(n, f[0], f[1]) is not None:
            out.append(f)
    return out


def histories(n):
    """received0 before the block call: filling (0, 1, n, 2n - 1), just ready (2n, 2n + 1: the latter a wrapped ring at wp0 = 0), wrapped rings at wp0 = 1, n, 2n
    and 0 again, and the values that put the first output tick on row 0 and on the last row of a 32- and a 16-tick tile (2n mod TR, and one more) -- 2n mod 32
    from an empty ring is also where the centred fused bank's t0 - 2n == -received0 falls on a tile start (n = 16 and 12: 0, n = 20: 8)."""
    ws = 2 * n + 1
    vals = [0, 1, n, 2 * n - 1, 2 * n, ws, ws + 1, 2 * ws + n, ws + 2 * n, 2 * ws]
    for tr in (32, 16):
        vals += [2 * n % tr, 2 * n % tr + 1]
    return sorted(set(vals))


def expect(n, fma, streams, misaligned, ticks, dma=True):
    """the family a block call is meant for: 'TILES' (block-moment or LDS-DMA), 'REGISTER_TILES' or 'WALK'.  block_form's rule in short; the CPU accounting
    (tests/test_stream_block_forms.py) holds every label of the list to the dispatcher's own answer"""
    if dma and streams % 128 == 0 and not misaligned and ticks >= 64 and (n <= 16 or fma or n >= 20):
        return "TILES"
    if not fma and n <= 12 and streams % 4 == 0 and not misaligned and ticks >= 32:
        return "REGISTER_TILES"
    return "WALK"


def cases(n, fma, filters=None):
    """the case list of one (half window, bank): a pure function, no GPU.  Not a cross product: every value of every axis occurs (histories x lengths are
    dealt round robin, shifted per filter), and the combinations the axes exist for occur by construction."""
    ws = 2 * n + 1
    F = bank_filters(n, fma)
    if filters is not None:
        F = [F[i] for i in filters if i < len(F)]
    H = histories(n)
    W = walk_lengths(n)
    out = []

    def add(name, streams, calls, f, off_in=0, off_out=0, offset=0.0):
        calls = tuple((kind, int(k)) for kind, k in calls if k > 0)
        out.append(Case(name, streams, off_in, off_out, n, f[0], f[1], f[2], int(bool(fma)), offset, calls))

    lin = next((f for f in F if f[1] == 1), F[-1])
    for fi, f in enumerate(F):
        # whole aligned strips: LDS-DMA / block-moment tiles from 64 ticks; every history against the lengths round robin
        for i, r0 in enumerate(H):
            add("whole strips", 256, [("tick", r0), ("block", DMA_LENGTHS[(i + fi) % 6])], f)
        # one long call on whole strips: a tile form over many bands, the last partial
        add("many bands", 256, [("tick", n), ("block", 16 * ws + 32 * 3 + 7)], f)
        # hand-over: tile form -> 63 ticks (register tiles / walk) -> ticks -> tile form; the ring partly, then wholly, replaced by the tail store; the call in
        # which the bank becomes ready
        add("hand-over A", 256, [("block", 96), ("block", 63), ("tick", 3), ("block", 65)], f)
        add("hand-over B", 256, [("block", 1), ("block", 2 * n), ("block", ws)], f)
        add("hand-over C", 256, [("tick", 2 * n - 1), ("block", 2)], f)
        # 17 strips: moment tiles in groups of 16 with a last group of one strip
        add("17 strips", 2176, [("tick", H[(2 * fi + 1) % len(H)]), ("block", DMA_LENGTHS[(5 * fi + 1) % 6])], f)
    for fi, f in enumerate(F[:2]):
        # quads but not strips: register tiles for the bit-exact bank at n <= 12 (a second 256-strip of four live streams), else the walk
        for i, r0 in enumerate(H):
            add("quads", 260, [("tick", r0), ("block", REGISTER_LENGTHS[(i + fi) % 6])], f)
    # the walk: one and two streams, a partial second strip, even (8-byte path on whole strips + a partial last strip), the element path, and one pointer at a
    # time off the 16-byte grid (tiles_take ORs the three addresses): samples 8-byte aligned only, then d_out alone one element off
    for si, (streams, off_in, off_out) in enumerate(((1, 0, 0), (2, 0, 0), (130, 0, 0), (1022, 0, 0), (777, 1, 0), (256, 2, 0), (256, 0, 1))):
        for j, length in enumerate(W):
            if (j + si) % 2 == 0:
                add("walk", streams, [("tick", H[(3 * si + j) % len(H)]), ("block", length)], F[(si + j) % len(F)], off_in, off_out)
    # 129 strips: tap-by-tap DMA tiles in groups of 128 and 1, moment tiles in groups of 32 with a last group of one -- the tile order has an empty tail
    # (tile_of returns !ok).  Short calls only: the oracle's cost
    add("129 strips", 16512, [("block", 97)], F[0])
    add("129 strips", 16512, [("tick", 2 * n % 32), ("block", 64)], lin)
    if not fma and n <= 12:
        # 65 register strips: groups of 64 and 1 (register tiles: the bit-exact bank up to n = 12)
        add("65 register strips", 16388, [("tick", 1), ("block", 49)], F[0])
        add("65 register strips", 16388, [("tick", 2 * n % 16), ("block", 33)], F[-1])
    if fma:
        # what centring exists for: derivative filters on streams riding on an offset of 1000
        for f in F:
            if f[1] > 0:
                add("offset 1000, whole strips", 256, [("tick", 2 * n % 32), ("block", 97)], f, offset=1000.0)
                add("offset 1000, 17 strips", 2176, [("block", 64)], f, offset=1000.0)
                add("offset 1000, walk", 130, [("tick", 1), ("block", 16 * ws)], f, offset=1000.0)
    return out


def big_case(n, fma, f):
    """config 3's stream count x 80 ticks (the runs under SAVGOL_HIP_STREAM_DMA=0: the walk on 512 whole aligned strips)"""
    return Case("config 3's streams", 65536, 0, 0, n, f[0], f[1], f[2], int(bool(fma)), 0.0, (("block", 80),))


def select(n, fma, filters=None, streams=None, big=False):
    """the cases one run of main() makes for a (half window, bank): the list of cases(n, fma, filters); with `streams`, its aligned cases of those stream
    counts only; with `big`, big_case on the bank's first filter behind them.  main() and the CPU accounting (tests/test_stream_block_forms.py) both ask here"""
    todo = cases(n, fma, filters)
    if streams is not None:
        todo = [c for c in todo if c.streams in streams and not c.off_in and not c.off_out]
    if big:
        todo.append(big_case(n, fma, bank_filters(n, fma)[0]))
    return todo


# The runs behind the environment switches, one fresh child process each (tests/test_gpu_stream_seams.py): the switch set to 0 -> (main()'s arguments, the
# child's time limit in seconds, ~15 x what it takes on an idle machine: 5 s for the 70 M outputs under STREAM_DMA, 3 s for the 10 M under STREAM_MOMENT, 2 s).
CHILDREN = {
    "SAVGOL_HIP_STREAM_DMA": (["--n", "8", "12", "16", "--banks", "0", "1", "--filters", "0", "2", "--streams", "256", "16512", "--big"], 90),
    "SAVGOL_HIP_STREAM_MOMENT": (["--n", "12", "16", "20", "--banks", "1", "--filters", "1", "2", "3", "--streams", "256", "2176"], 60),
    "SAVGOL_HIP_SMALL_SERVICE": (["--single-stream"], 40),
}


def case_ticks(case):
    return sum(k for _, k in case.calls) + 2 * case.n + 1


def cost(case_list):
    return float(sum(case_ticks(c) * c.streams * (2 * c.n + 1) for c in case_list))


def block_calls(case):
    """(t0, ticks, misaligned) of every block call of a case: misaligned = the low four bits of the two addresses or-ed (the ring is the allocator's)"""
    t = 0
    for kind, k in case.calls:
        if kind == "block":
            yield t, k, (((case.off_in + t * case.streams) * 4) | ((case.off_out + t * case.streams) * 4)) & 15
        t += k


# ---------------------------------------------------------------------------------------------------------------
# CPU references
# ---------------------------------------------------------------------------------------------------------------
def signal(case, ticks, seed):
    """[tick][stream] fp32: a tone plus noise of comparable size, amplitude, frequency and phase different from stream to stream -- a row one tick off, or a stream
    taken from the neighbouring lane, strip or group, moves outputs far beyond any bar"""
    rng = np.random.default_rng(seed)
    s = np.arange(case.streams, dtype=f64)[None, :]
    t = np.arange(ticks, dtype=f64)[:, None]
    x = (0.5 + (s * 0.6180339887) % 1.0) * np.sin((0.05 + 0.02 * ((s * 0.3819660113) % 1.0)) * t + 0.37 * s)
    x += 0.4 * rng.standard_normal((ticks, case.streams))
    return (x + case.offset).astype(f32)


def dot_rows(w, scale, x, dtype):
    """sum_k w[k] x[k : k + M] in the reference's order (one accumulator from 0, taps ascending, multiply and add rounded separately), then * scale"""
    rows = x.shape[0] - len(w) + 1
    if rows <= 0:
        return np.zeros((0,) + x.shape[1:], dtype)
    xs = x.astype(dtype, copy=False)
    acc = np.zeros((rows,) + x.shape[1:], dtype)
    tmp = np.empty_like(acc)
    for k in range(len(w)):
        np.multiply(xs[k:k + rows], dtype(w[k]), out=tmp)
        acc += tmp
    acc *= dtype(scale)
    return acc


def flush_rows(filt, ring, leading):
    """the n edge rows of sgo_stream_flush (rows n-1 ... 0, ring walked forward from the oldest sample) / _flush_leading (rows 0 ... n-1, backward from the
    newest), oracle/sg_oracle.c; ring: [2n + 1][stream], oldest first"""
    n = filt.n
    src = ring[::-1] if leading else ring
    return np.stack([dot_rows(filt.edges[i if leading else n - 1 - i], filt.dt_inv, src, f32)[0] for i in range(n)])


def self_check(n, m, d, dt, streams=4, ticks=None, seed=0):
    """pins the restatement to sgo.Stream on a few streams, offsets up to 1000: push, flush_leading and flush, bit for bit, counters as the runner derives them"""
    from oracle import sgo
    ws = 2 * n + 1
    ticks = ticks or 3 * ws + 7
    filt = sgo.Filter(n, m, d, dt)
    rng = np.random.default_rng(1000 * n + 10 * m + d + seed)
    x = (rng.standard_normal((ticks, streams)) + np.linspace(0.0, 1000.0, streams)[None, :]).astype(f32)
    ref = dot_rows(filt.center, filt.dt_inv, x, f32)
    for s in range(streams):
        o = sgo.Stream(filt)
        seq = [o.push(v) for v in x[:, s]]
        assert [ok for _, ok in seq] == [t >= 2 * n for t in range(ticks)]
        assert same_bits(np.array([v for v, ok in seq if ok], f32), ref[:, s]), ("push", n, m, d, s)
        for cut in (ticks, ticks - n - 1):
            o = sgo.Stream(filt)
            for v in x[:cut, s]:
                o.push(v)
            for leading in (True, False):
                c, w = (o.flush_leading if leading else o.flush)(n)
                assert c == n and same_bits(w, flush_rows(filt, x[cut - ws:cut], leading)[:, s]), ("flush", leading, n, m, d, s)
            assert o.counters[:2] == (cut, cut - 2 * n + 2 * n)        # emitted: cut - 2n centre outputs, then n rows from each of the two flushes


# ---------------------------------------------------------------------------------------------------------------
# geometry: what tests/mock/stream_block_forms.cpp prints for a call
# ---------------------------------------------------------------------------------------------------------------
_mock_exe = None
_centre_terms = {}


def mock_exe():
    global _mock_exe
    if _mock_exe is None:
        tmp = tempfile.mkdtemp(prefix="stream_seams_")
        atexit.register(shutil.rmtree, tmp, ignore_errors=True)
        exe = os.path.join(tmp, "stream_block_forms")
        subprocess.run(["g++", "-O1", "-std=c++17", "-I" + os.path.join(ROOT, "savitzky-golay-filter_amd", "csrc"), "-o", exe,
                        os.path.join(ROOT, "tests", "mock", "stream_block_forms.cpp")], check=True)
        _mock_exe = exe
    return _mock_exe


def centre_and_terms(sg, case):
    """centre: the dispatcher's rule |sum w| < 1e-3 sum |w| on the oracle's taps (fused banks only); terms: savgol_hip_stream_moment_table"""
    from oracle import sgo
    key = (case.n, case.m, case.d, case.fma)
    if key not in _centre_terms:
        w = sgo.weights(case.n, case.m, case.d)[0]
        w64 = w.astype(f64)
        centre = int(bool(case.fma) and abs(w64.sum()) < 1e-3 * np.abs(w64).sum())
        c = np.zeros((3, 34), f32)
        terms = sg.lib().savgol_hip_stream_moment_table(case.n, w.ctypes.data_as(C.POINTER(C.c_float)), c.ctypes.data_as(C.POINTER(C.c_float)))
        _centre_terms[key] = (centre, max(int(terms), 0))
    return _centre_terms[key]


def mock_fields(sg, case, ticks, misaligned, dma=1, mom=1, nwaves=2048):
    centre, terms = centre_and_terms(sg, case)
    return (case.n, case.fma, case.streams, ticks, misaligned, centre, terms, dma, mom, nwaves)


def mock_geometry(fields_list):
    """one dict per call shape: the form taken, its strips / bands / group / total / grid (tile forms) or bands (the walk), and the forms offered after it"""
    text = "".join(" ".join(str(v) for v in fields) + "\n" for fields in fields_list)
    lines = subprocess.run([mock_exe()], input=text, capture_output=True, text=True, check=True).stdout.splitlines()[1:]
    assert len(lines) == len(fields_list)
    out = []
    for line in lines:
        taken = line.split(": ", 1)[1]
        name, rest = taken.split("(", 1)
        g = {"form": name, "line": line}
        inner = rest.split(")", 1)[0]
        for part in inner.split(" "):
            if "=" in part:
                key, val = part.split("=")
                g[key] = int(val)
        out.append(g)
    return out


def switches():
    return int(os.environ.get("SAVGOL_HIP_STREAM_DMA", "1") != "0"), int(os.environ.get("SAVGOL_HIP_STREAM_MOMENT", "1") != "0")


def where(sg, case, t0, ticks, misaligned, tick, stream):
    """names a failing output: stream, tick, strip, band, group and row within the tile, from the geometry the mock prints for the call's shape"""
    dma, mom = switches()
    g = mock_geometry([mock_fields(sg, case, ticks, misaligned, dma, mom)])[0]
    if g["form"] == "WALK":
        rows = (ticks + g["bands"] - 1) // g["bands"]
        return (f"stream {stream}, tick {tick} of the call (tick {t0 + tick} of the bank): WALK, strip {stream // 128} (lane {stream % 128 // 2}), band {tick // rows} of "
                f"{g['bands']} (on 2048 waves), row {tick % rows} of {rows}")
    width, tr = (256, 16) if g["form"] == "REGISTER_TILES" else (128, 32)
    strip = stream // width
    return (f"stream {stream}, tick {tick} of the call (tick {t0 + tick} of the bank): {g['form']}, strip {strip} of {g['strips']}, band {tick // tr} of {g['bands']}, "
            f"group {strip // g['group']} (strip {strip % g['group']} of its {g['group']}), row {tick % tr} of its {tr}-tick tile")


# ---------------------------------------------------------------------------------------------------------------
# the runner
# ---------------------------------------------------------------------------------------------------------------
class Guarded:
    """rows x streams floats `off` elements into a device buffer pre-filled with GUARD: GUARD_ROWS rows (rounded up to whole 256-byte lines, so `off` alone
    decides the alignment) in front, as many and 8 elements behind"""

    def __init__(self, torch, rows, streams, off, host=None):
        self.front = (GUARD_ROWS * streams + 63) // 64 * 64 + off
        self.rows, self.streams = rows, streams
        self.want = np.full(self.front + rows * streams + GUARD_ROWS * streams + 8, GUARD, f32)
        if host is not None:
            self.body(self.want)[:] = host
        self.buf = torch.from_numpy(self.want).cuda()
        self.base = self.buf.data_ptr() + 4 * self.front

    def ptr(self, row):
        return self.base + 4 * row * self.streams

    def body(self, flat):
        return flat[self.front:self.front + self.rows * self.streams].reshape(self.rows, self.streams)

    def host(self):
        return self.buf.cpu().numpy()

    def outside_intact(self, flat):
        return bool(np.array_equal(bits(flat[:self.front]), bits(self.want[:self.front])) and
                    np.array_equal(bits(flat[self.front + self.rows * self.streams:]), bits(self.want[self.front + self.rows * self.streams:])))


class Stats:
    def __init__(self):
        self.cases = self.calls = self.blocks = self.outputs = 0

    def __str__(self):
        return f"{self.cases} cases, {self.calls} calls ({self.blocks} block pushes), {self.outputs} outputs compared"


def run_case(sg, torch, case, stats, seed=0):
    from oracle import sgo
    n, S, fma = case.n, case.streams, bool(case.fma)
    ws = 2 * n + 1
    T = case_ticks(case)
    filt = sgo.Filter(n, case.m, case.d, case.dt)
    x = signal(case, T, seed)
    ref32 = dot_rows(filt.center, filt.dt_inv, x, f32)                       # row t - 2n: the output of tick t
    ref64 = dot_rows(filt.center.astype(f64), f64(filt.dt_inv), x, f64) if fma else None
    xin = Guarded(torch, T, S, case.off_in, x)
    out = Guarded(torch, T, S, case.off_out)
    oracle = sgo.Stream(filt)
    bank = sg.StreamBank(S, n, case.m, case.d, case.dt, fma=fma)
    label = (case.name, S, case.off_in, case.off_out, n, case.m, case.d, case.dt, "fused" if fma else "bit-exact", case.offset, case.calls)
    t = 0
    stats.cases += 1

    def step(kind, k):
        nonlocal t
        stats.calls += 1 if kind == "block" else k
        mis = (((case.off_in + t * S) * 4) | ((case.off_out + t * S) * 4)) & 15
        oks = [oracle.push(v) for v in x[t:t + k, 0]]
        if kind == "block":
            stats.blocks += 1
            r = bank.push_block(xin.ptr(t), k, out.ptr(t))
            assert r == sum(ok for _, ok in oks), ("push_block returned", r, sg.last_error(), label, t)
        else:
            for i in range(k):
                r = bank.push(xin.ptr(t + i), out.ptr(t + i))
                assert r == int(oks[i][1]), ("push returned", r, sg.last_error(), label, t + i)
        assert tuple(bank.counters) == tuple(oracle.counters[:2]), ("counters", bank.counters, oracle.counters, label, t)
        torch.cuda.synchronize()
        lo, hi = max(t, 2 * n), t + k
        got = out.host()
        if hi > lo:
            assert same_bits(np.array([v for v, ok in oks if ok], f32), ref32[lo - 2 * n:hi - 2 * n, 0]), ("the restatement left the oracle", label, t)
            rows = out.body(got)[lo:hi]
            want = ref32[lo - 2 * n:hi - 2 * n]
            stats.outputs += rows.size

            def spot(bad):
                i, s = np.argwhere(bad)[0]
                if kind == "block":
                    return f"{int(bad.sum())} outputs; first: " + where(sg, case, t, k, mis, int(lo - t + i), int(s))
                return f"{int(bad.sum())} outputs; first: stream {s}, tick push {lo + i} of the bank"
            if not fma:
                bad = bits(rows) != bits(want)
                if bad.any():
                    raise AssertionError(("words that differ from the reference's", spot(bad), label))
            else:
                hi64 = ref64[lo - 2 * n:hi - 2 * n]
                e_ref = normwise(want, hi64)
                value, bar = normwise(rows, hi64), fp32_bar(e_ref)
                note = ()
                if not value < bar:
                    note = (spot(np.abs(rows.astype(f64) - hi64) >= bar * np.max(np.abs(hi64))),)
                check(value, bar, ("fused bank",) + label[:10] + (kind, k, t, e_ref) + note)
            out.body(out.want)[lo:hi] = rows if fma else want
        # rows of ticks without an output and earlier rows as they were, every guard element around d_out, d_samples and its guards as uploaded
        if not np.array_equal(bits(got), bits(out.want)):
            assert out.outside_intact(got), ("a write outside d_out", label, kind, k, t)
            bad = bits(out.body(got)) != bits(out.body(out.want))
            i, s = np.argwhere(bad)[0]
            raise AssertionError(("a row that must not change was written", f"{int(bad.sum())} elements; first: tick {i} of the bank, stream {s}", label, kind, k, t))
        assert np.array_equal(bits(xin.host()), bits(xin.want)), ("d_samples or its guards were written", label, kind, k, t)
        t += k

    for kind, k in case.calls:
        step(kind, k)
    # both flushes, every stream, bit for bit on both banks (edge rows keep the reference's order on the fused bank too)
    for leading in (True, False):
        edge = Guarded(torch, n, S, 0)
        r = (bank.flush_leading if leading else bank.flush)(edge.ptr(0), n)
        c, w0 = (oracle.flush_leading if leading else oracle.flush)(n)
        assert r == c, ("flush returned", leading, r, c, label)
        assert tuple(bank.counters) == tuple(oracle.counters[:2]), ("counters after a flush", bank.counters, oracle.counters, label)
        torch.cuda.synchronize()
        if c:
            want = flush_rows(filt, x[t - ws:t], leading)
            assert same_bits(w0, want[:, 0]), ("the restatement's flush left the oracle", leading, label)
            edge.body(edge.want)[:] = want
            stats.outputs += want.size
        got = edge.host()
        if not np.array_equal(bits(got), bits(edge.want)):
            assert edge.outside_intact(got), ("a flush wrote outside its rows", leading, label)
            bad = bits(edge.body(got)) != bits(edge.body(edge.want))
            i, s = np.argwhere(bad)[0]
            raise AssertionError(("flush_leading" if leading else "flush", f"{int(bad.sum())} words differ; first: row {i}, stream {s} (strip {s // 128})", label))
    # and the ring the block push left, consumed whole
    step("tick", ws)
    assert t == T
    bank.close()


def run_list(sg, torch, case_list, stats=None, seed=0):
    stats = stats or Stats()
    for i, case in enumerate(case_list):
        run_case(sg, torch, case, stats, seed + 7919 * i)
    return stats


# ---------------------------------------------------------------------------------------------------------------
# the single-stream drop-in API and the short host-pointer calls (the launch path behind the resident small-call service)
# ---------------------------------------------------------------------------------------------------------------
def run_single_stream(sg):
    """sg.Stream (push, push_full, both flushes, the truncated burst) over every case of tests/golden/stream.npz and savgol_apply / _valid / _strided over
    tests/golden/apply1d.npz, bit for bit against the golden -- what test_single_stream_bit_exact_vs_reference_golden and
    test_savgol_apply_matches_reference_golden assert, for a process in which SAVGOL_HIP_SMALL_SERVICE=0 puts every call on the launched kernels"""
    from tests.golden.make_golden import APPLY_CASES, STREAM_CASES
    g = np.load(os.path.join(ROOT, "tests", "golden", "stream.npz"))
    for ci in range(len(STREAM_CASES)):
        n, m, d, count = (int(v) for v in g[f"s{ci}_cfg"])
        x = g[f"s{ci}_in"]
        dt = float(g[f"s{ci}_dt"])
        s = sg.Stream(n, m, d, dt)
        vals, valid = zip(*[s.push(v) for v in x])
        assert same_bits(np.array(vals, f32), g[f"s{ci}_push_val"]), ("push", ci)
        assert np.array_equal(np.array(valid), g[f"s{ci}_push_valid"]), ("push valid", ci)
        assert list(s.counters) == list(g[f"s{ci}_push_counters"]), ("push counters", ci)
        s = sg.Stream(n, m, d, dt)
        seq, counts = [], []
        for v in x:
            o = s.push_full(v)
            counts.append(o.size); seq.extend(o.tolist())
        assert np.array_equal(np.array(counts), g[f"s{ci}_full_counts"]), ("push_full counts", ci)
        assert same_bits(np.array(seq, f32), g[f"s{ci}_full_seq"]), ("push_full", ci)
        c, lead = s.flush_leading()
        assert c == int(g[f"s{ci}_flush_leading_rc"]) and same_bits(lead, g[f"s{ci}_flush_leading"]), ("flush_leading", ci)
        c, tail = s.flush()
        assert c == int(g[f"s{ci}_flush_rc"]) and same_bits(tail, g[f"s{ci}_flush"]), ("flush", ci)
        assert list(s.counters) == list(g[f"s{ci}_full_counters"]), ("push_full counters", ci)
        s = sg.Stream(n, m, d, dt)
        tr = []
        for v in x:
            tr.extend(s.push_full(v, 2).tolist())
        assert same_bits(np.array(tr, f32), g[f"s{ci}_full_trunc2"]), ("truncated burst", ci)
    print(f"single stream: {len(STREAM_CASES)} golden cases bit for bit")
    g = np.load(os.path.join(ROOT, "tests", "golden", "apply1d.npz"))
    for ci in range(len(APPLY_CASES)):
        n, m, d, length = (int(v) for v in g[f"c{ci}_cfg"])
        dt = float(g[f"c{ci}_dt"])
        x = g[f"c{ci}_in"]
        for mode in range(4):
            assert same_bits(sg.Filter(n, m, d, dt, mode).apply(x), g[f"c{ci}_mode{mode}_out"]), ("savgol_apply", ci, mode)
        f = sg.Filter(n, m, d, dt, 0)
        v = f.apply_valid(x)
        assert v.shape == g[f"c{ci}_valid_out"].shape and same_bits(v, g[f"c{ci}_valid_out"]), ("savgol_apply_valid", ci)
        src = g[f"c{ci}_strided_in"].copy()
        dst = src.copy()
        assert f.apply_strided(src, 12, 4, dst, 12, 4, length) == 0 and same_bits(dst, g[f"c{ci}_strided_out"]), ("savgol_apply_strided", ci)
    print(f"savgol_apply: {len(APPLY_CASES)} golden cases bit for bit")


def parser():
    p = argparse.ArgumentParser(description="run the stream block push's seam matrix on the GPU; exits non-zero on the first failed comparison")
    p.add_argument("--n", type=int, nargs="*", default=[], help="half windows")
    p.add_argument("--banks", type=int, nargs="*", default=[0, 1], help="0 = bit-exact, 1 = fused")
    p.add_argument("--filters", type=int, nargs="*", default=None, help="indices into bank_filters(n, fma)")
    p.add_argument("--streams", type=int, nargs="*", default=None, help="keep the aligned cases with these stream counts")
    p.add_argument("--big", action="store_true", help="add config 3's stream count x 80 ticks, on the bank's first filter")
    p.add_argument("--single-stream", action="store_true", help="the single-stream API and savgol_apply over the golden files")
    return p


def main(argv=None):
    args = parser().parse_args(argv)
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    from __graft_entry__ import load_package
    import torch
    sg = load_package()
    try:
        assert torch.cuda.is_available() and sg.device_count() > 0, sg.last_error()
        if args.single_stream:
            run_single_stream(sg)
        for n in args.n:
            for fma in args.banks:
                stats = run_list(sg, torch, select(n, fma, args.filters, args.streams, args.big), seed=100 * n + fma)
                print(f"n={n} {'fused' if fma else 'bit-exact'} bank, switches DMA={switches()[0]} MOMENT={switches()[1]}: {stats}")
    except AssertionError as e:
        print("FAILED:", e)
        return 1
    return 0


if __name__ == "__main__":
    sys.exit(main())
