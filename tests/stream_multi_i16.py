"""What tests/test_stream_multi_i16_host.py (CPU) and tests/test_gpu_stream_multi_i16.py (GPU) share: the shipped bound table restated, the banks and
half windows of the GPU test, its int16 signals and the contract's fp32 -> int16 conversion on the CPU.

AMPLITUDE.  The banks of one fused call share the samples, so a call has ONE amplitude (counts per unit of stream_seams.signal: a tone of 0.5 .. 1.5
plus noise of 0.4), and it has to suit the three filters at once.  The first derivative with dt = 1e-3 sets the upper end: its output is 1000 x the
slope per tick -- at n = 1 the noise alone gives 0.28 x 1000 x the amplitude (60 counts: a spread of 17 000, 94 % of the words inside the range), from
n = 4 the tone's slope (at most 1.5 x 0.07 per tick) dominates and 250 counts give peaks of 35 000 .. 69 000 with 95 % or more of the words inside.  The
second derivative with dt = 0.5 sets the lower end: 4 x the second difference, which falls with n^2.5 -- at 250 counts its peak is still 32 counts at
n = 9, at 60 counts it would be 8.  tests/test_stream_multi_i16_host.py holds every (half window, filter) of the GPU test to the condition on the CPU:
at least half of the expected int16 words strictly inside (-32768, 32767), the largest magnitude at least 10 counts."""
import numpy as np

from tests import stream_seams as seams

# the shipped bounds: (fused bank?, outputs per launch) -> the largest fused half window (stream_multi_i16_max_n, csrc/sg_stream_host.hpp)
FUSED_MAX_N = {(0, 2): 8, (0, 3): 8, (1, 2): 8, (1, 3): 8}
HALF_WINDOWS = [1, 4, 5, 6, 8, 9]                            # the shape table's seams (5 | 6), the bound (8) and the first unfused half window (9)
FILTERS = [(2, 0, 1.0), (2, 1, 1e-3), (3, 2, 0.5)]           # smoothing (uncentred), first and second derivative (centred on the fused bank): three dt_inv in one launch
TICKS = [64, 65, 95, 96, 97, 128, 161]                       # no body | one partial band ... | two bands | four bands, the last of one row
OUTS = ("i16", "f32")
RIDE = 30000.0                                               # counts the streams of the centring cases ride at
MIN_PEAK = 10                                                # counts: the largest expected magnitude of every (half window, filter)


def filters_for(n, sgo):
    """FILTERS at half window n; an order the window cannot carry (m = 3 at n = 1) falls back to 2"""
    out = [f if f[0] <= 2 * n and sgo.weights(n, f[0], f[1]) is not None else (2, f[1], f[2]) for f in FILTERS]
    assert all(sgo.weights(n, f[0], f[1]) is not None for f in out)
    return out


def amplitude(n):
    """counts per unit of stream_seams.signal for a call at half window n (see the module's docstring)"""
    return 60.0 if n <= 1 else 120.0 if n <= 3 else 250.0


def quantise(streams, n, ticks, seed, offset=0.0):
    """stream_seams.signal scaled to amplitude(n) counts around `offset` counts -> int16, on the CPU"""
    case = seams.Case("multi_i16", streams, 0, 0, n, 2, 0, 1.0, 0, 0.0, ())
    x = seams.signal(case, ticks, seed).astype(np.float64) * amplitude(n) + offset
    return np.clip(np.rint(x), -32768, 32767).astype(np.int16)


def to_i16(torch, w):
    """the contract's conversion of fp32 rows, on the CPU (as tests/test_gpu_stream_i16.py): nearest even, saturated, NaN -> 0"""
    assert w.device.type == "cpu" and w.dtype == torch.float32
    return torch.clamp(torch.nan_to_num(torch.round(w), nan=0.0), -32768, 32767).to(torch.int16)


def inside_enough(words):
    """the amplitude condition on an array of expected int16 words: at least half strictly inside (-32768, 32767)"""
    words = np.asarray(words).astype(np.int64)
    return 2 * int(((words > -32768) & (words < 32767)).sum()) >= words.size


def expected_route(specs, streams, ticks, misaligned):
    """the shipped rule (include/savgol_hip.h): fused launches of a call, 0 = single int16 calls.  specs: (n, m, d, dt, fma, history) per bank"""
    n, fma = specs[0][0], specs[0][4]
    per = 2 if len(specs) == 4 else len(specs)
    fused = (len(specs) >= 2 and all(s[0] == n and s[4] == fma for s in specs) and n <= FUSED_MAX_N.get((fma, per), 0) and streams % 128 == 0 and
             not misaligned and ticks > 64)
    return (2 if len(specs) == 4 else 1) if fused else 0
