"""Times savgol_streambank_push_block_multi_i16 against the single savgol_streambank_push_block_i16 calls it replaces, and against the bf16 fused call
(savgol_streambank_push_block_multi_h16) and its own single calls on the same bytes, on config 3's shape (tools, not product).

For every (bank kind, half window, set of filters, output type): blocks issued back to back (K per window, device events around the window) on a chip
kept busy first; the fused int16 call on banks A, the `count` single int16 calls on banks B, the bf16 fused call on banks C and the `count` single bf16
calls on banks D (the int16 block read as bf16 words: the same bytes in, the same bytes out), all of the same configurations, interleaved window by
window in one process, every round on fresh buffers (the earlier rounds' buffers stay allocated until the shape is done, so new pages back the new ones;
placement moves a launch by +- 3 %).  Before timing, at this size, the fused int16 outputs are asserted equal to the single calls' word for word.
Reports the median and the spread of the per-block time, the ratio to the single int16 calls (> 1: the fused call is faster; the byte bound is
4 count / (2 + 2 count) for int16 -> int16 and 6 count / (2 + 4 count) for int16 -> fp32), the bf16 fused call's ratio to ITS single calls in the same
run (the expectation the int16 ratio is reported against), the fraction of the 8 TB/s roofline at the call's own bytes, and the route the call took.
    python tools/time_stream_block_multi_i16.py [> profiles/stream_multi_i16_time.txt]
STREAMS, TICKS, HALF_WINDOWS, KINDS, OUTS, COUNTS, ROUNDS, K override the shape and the effort."""
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from __graft_entry__ import load_package

sg = load_package()
import torch

S, T = int(os.environ.get("STREAMS", "65536")), int(os.environ.get("TICKS", "4096"))
NS = [int(v) for v in os.environ.get("HALF_WINDOWS", "1,2,3,4,5,6,7,8").split(",")]
KINDS = [int(v) for v in os.environ.get("KINDS", "1,0").split(",")]
OUTS = os.environ.get("OUTS", "i16,f32").split(",")
COUNTS = [int(v) for v in os.environ.get("COUNTS", "2,3,4").split(",")]
ROUNDS, K = int(os.environ.get("ROUNDS", "5")), int(os.environ.get("K", "7"))
PEAK = 8000.0                                               # GB/s
FILTERS = [(2, 0, 1.0), (2, 1, 1e-3), (3, 2, 0.5)]           # value, velocity, acceleration: (m 2, d 0), (m 2, d 1), (m 3, d 2)
FOURTH = (4, 0, 1.0)
DTYPE = {"i16": torch.int16, "bf16": torch.bfloat16, "f32": torch.float32}


def window(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(K):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / K


def med(v):
    return statistics.median(v), min(v), max(v)


def shapes():
    for fma in KINDS:
        for n in NS:
            for out in OUTS:
                for count in COUNTS:
                    f = [g if g[0] <= 2 * n else (2, g[1], g[2]) for g in FILTERS + [FOURTH]]       # a window of 2n + 1 holds order <= 2n
                    yield n, fma, f[:count], out


def main():
    assert torch.cuda.is_available() and sg.device_count() > 0, sg.last_error()
    print(f"# {S} streams x {T} ticks, {ROUNDS} rounds of {K} blocks back to back per variant, interleaved, fresh buffers every round; ms per block: median [min .. max]")
    print("# ratio = single int16 calls' median / fused int16 call's median (> 1: the fused call is faster); bf16 = the bf16 fused call and its single calls on the "
          "same bytes, with their own ratio; frac = the call's own bytes (2 + e count per stream-tick, e = 2 or 4) / fused int16 time / 8 TB/s")
    busy = torch.randn((T, S), device="cuda")
    for _ in range(20):                                     # a chip kept busy first
        busy.mul_(1.0000001)
    for n, fma, filters, out in shapes():
        count = len(filters)
        elem = 4 if out == "f32" else 2
        hout = "f32" if out == "f32" else "bf16"
        A, B, Cb, D = ([sg.StreamBank(S, n, m, d, dt, fma=bool(fma)) for m, d, dt in filters] for _ in range(4))
        times = {"multi": [], "single": [], "h16 multi": [], "h16 single": []}
        route = None
        keep = []
        for r in range(ROUNDS + 1):
            x = torch.randint(-8000, 8000, (T, S), dtype=torch.int16, device="cuda")      # ADC counts
            xb = x.view(torch.bfloat16)                     # the same bytes, read as bf16 words
            oa, ob = ([torch.empty((T, S), dtype=DTYPE[out], device="cuda") for _ in range(count)] for _ in range(2))
            oc, od = ([torch.empty((T, S), dtype=DTYPE[hout], device="cuda") for _ in range(count)] for _ in range(2))
            keep.append((x, oa, ob, oc, od))

            def multi():
                return min(sg.push_block_multi_i16(A, x, T, oa, out))

            def single():
                return min(B[k].push_block_i16(x, T, ob[k], out) for k in range(count))

            def h16_multi():
                return min(sg.push_block_multi_h16(Cb, xb, "bf16", T, oc, hout))

            def h16_single():
                return min(D[k].push_block_h16(xb, "bf16", T, od[k], hout) for k in range(count))

            if route is None:
                route = sg.push_block_multi_i16_route(A, x, T, oa, out)
            assert multi() >= 0 and single() >= 0 and h16_multi() >= 0 and h16_single() >= 0, sg.last_error()
            torch.cuda.synchronize()
            view = torch.int32 if elem == 4 else torch.int16
            for k in range(count):                          # round 0, fresh banks on both sides: rows 2n .. T - 1 hold outputs
                lo = 2 * n if r == 0 else 0
                assert torch.equal(oa[k][lo:].view(view), ob[k][lo:].view(view)), ("the fused call left its twin's words", n, fma, filters[k], out, r)
            for name, fn in (("multi", multi), ("single", single), ("h16 multi", h16_multi), ("h16 single", h16_single)):
                ms = window(fn)
                if r:                                       # round 0 warms up
                    times[name].append(ms)
        del keep, x, xb, oa, ob, oc, od
        torch.cuda.empty_cache()
        m, s, hm, hs = (med(times[k]) for k in ("multi", "single", "h16 multi", "h16 single"))
        names = " + ".join(f"m{f[0]}d{f[1]}" for f in filters)
        bound = (2 + elem) * count / (2 + elem * count)
        print(f"n={n:2d} {'fused' if fma else 'exact'} i16->{out} {count} x ({names}): route {route} ({'fused launches' if route else 'single calls'})  "
              f"multi {m[0]:.3f} [{m[1]:.3f} .. {m[2]:.3f}]  single {s[0]:.3f} [{s[1]:.3f} .. {s[2]:.3f}]  ratio {s[0] / m[0]:.2f} x (bound {bound:.2f})  "
              f"bf16 multi {hm[0]:.3f} [{hm[1]:.3f} .. {hm[2]:.3f}]  bf16 single {hs[0]:.3f} [{hs[1]:.3f} .. {hs[2]:.3f}]  bf16 ratio {hs[0] / hm[0]:.2f} x  "
              f"i16 / bf16 multi {m[0] / hm[0]:.2f}  frac {(2 + elem * count) * S * T / m[0] / 1e6 / PEAK:.3f}", flush=True)
        for bank in A + B + Cb + D:
            bank.close()


if __name__ == "__main__":
    main()
