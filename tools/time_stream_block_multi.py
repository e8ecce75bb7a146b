"""Times savgol_streambank_push_block_multi against the single savgol_streambank_push_block calls it replaces, on config 3's shape (tools, not product).

For every (bank kind, half window, set of filters): blocks issued back to back (K per window, device events around the window) on a chip kept busy
first; the multi call on banks A and the `count` single calls on banks B of the same configurations, interleaved window by window in one process, every
round on fresh buffers (the earlier rounds' buffers stay allocated until the shape is done, so new pages back the new ones; placement moves a
launch by +- 3 %).  Before timing, at this size, the multi outputs are asserted equal to the single calls' bit for bit.  ALT=path[,path] adds further
builds of the library to the same process (tools/ab_libs.py): their multi calls are interleaved with the shipped build's, for launch-shape A/Bs.  Reports the median and the spread of the per-block time, the ratio (> 1: the multi call is faster; the byte bound is 8 count / (4 + 4 count):
1.33 x for two and four outputs, 1.5 x for three), the fraction of the 8 TB/s roofline at 4 + 4 count bytes per stream-tick, and the route the call took.
    python tools/time_stream_block_multi.py [> profiles/stream_multi_time.txt]
STREAMS, TICKS, HALF_WINDOWS, KINDS, ROUNDS, K override the shape and the effort."""
import ctypes as C
import itertools
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from __graft_entry__ import load_package

sg = load_package()
import torch

S, T = int(os.environ.get("STREAMS", "65536")), int(os.environ.get("TICKS", "4096"))
NS = [int(v) for v in os.environ.get("HALF_WINDOWS", "2,4,5,6,8,9,16").split(",")]
KINDS = [int(v) for v in os.environ.get("KINDS", "1,0").split(",")]
ROUNDS, K = int(os.environ.get("ROUNDS", "5")), int(os.environ.get("K", "7"))
ALT = [p for p in os.environ.get("ALT", "").split(",") if p]
PEAK = 8000.0                                               # GB/s
FILTERS = [(2, 0, 1.0), (2, 1, 1e-3), (3, 2, 0.5)]           # value, velocity, acceleration
FOURTH = (4, 0, 1.0)


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
            if n in (9, 16):                                # past the fused range: what the single-call route costs
                yield n, fma, FILTERS[:2] if n == 9 else FILTERS
                continue
            for count in (2, 3):
                for combo in itertools.combinations(FILTERS, count):
                    yield n, fma, list(combo)
            if n == 4:
                yield n, fma, FILTERS + [FOURTH]


def main():
    assert torch.cuda.is_available() and sg.device_count() > 0, sg.last_error()
    print(f"# {S} streams x {T} ticks, {ROUNDS} rounds of {K} blocks back to back per variant, interleaved, fresh buffers every round; ms per block: median [min .. max]")
    print("# ratio = single calls' median / multi call's median (> 1: the multi call is faster); frac = (4 + 4 count) bytes x streams x ticks / multi time / 8 TB/s")
    busy = torch.randn((T, S), device="cuda")
    for _ in range(20):                                     # a chip kept busy first
        busy.mul_(1.0000001)
    alts = []
    if ALT:
        import ab_libs
        alts = [ab_libs.load(p) for p in ALT]
        print("# alt builds, interleaved in this process: " + ", ".join(f"alt{i} = {os.path.basename(os.path.dirname(p))}" for i, p in enumerate(ALT)))
    st = torch.cuda.current_stream().cuda_stream
    for n, fma, filters in shapes():
        count = len(filters)
        A = [sg.StreamBank(S, n, m, d, dt, fma=bool(fma)) for m, d, dt in filters]
        B = [sg.StreamBank(S, n, m, d, dt, fma=bool(fma)) for m, d, dt in filters]
        # the same banks in every alt build, through its own C ABI
        alt_banks = []
        for L in alts:
            ptrs = [L.savgol_streambank_create_ex(C.byref(sg.SavgolConfig(n, m, d, dt, 0)), S, sg.SAVGOL_STREAMBANK_FMA if fma else 0) for m, d, dt in filters]
            assert all(ptrs)
            alt_banks.append(ptrs)
        times = {"multi": [], "single": []}
        times.update({f"alt{i}": [] for i in range(len(alts))})
        route = None
        keep = []
        for r in range(ROUNDS + 1):
            x = torch.randn((T, S), device="cuda")
            oa = [torch.empty_like(x) for _ in range(count)]
            ob = [torch.empty_like(x) for _ in range(count)]
            keep.append((x, oa, ob))
            outs = (C.c_void_p * count)(*[o.data_ptr() for o in oa])

            def multi():
                return min(sg.push_block_multi(A, x, T, oa))

            def single():
                return min(B[k].push_block(x, T, ob[k]) for k in range(count))

            def alt(i):
                return lambda: alts[i].savgol_streambank_push_block_multi((C.c_void_p * count)(*alt_banks[i]), count, x.data_ptr(), T, outs, None, st)

            if route is None:
                route = sg.push_block_multi_route(A, x, T, oa)
            assert multi() >= 0 and single() >= 0, sg.last_error()
            torch.cuda.synchronize()
            for k in range(count):                          # round 0, fresh banks on both sides: rows 2n .. T - 1 hold outputs
                lo = 2 * n if r == 0 else 0
                assert torch.equal(oa[k][lo:].view(torch.int32), ob[k][lo:].view(torch.int32)), ("the multi call left its twin's bits", n, fma, filters[k], r)
            runs = [("multi", multi), ("single", single)] + [(f"alt{i}", alt(i)) for i in range(len(alts))]
            for i in range(len(alts)):
                assert runs[2 + i][1]() >= 0
            for name, fn in runs:
                ms = window(fn)
                if r:                                       # round 0 warms up
                    times[name].append(ms)
        del keep, x, oa, ob
        torch.cuda.empty_cache()
        m, s = med(times["multi"]), med(times["single"])
        names = " + ".join(f"m{f[0]}d{f[1]}" for f in filters)
        print(f"n={n:2d} {'fused' if fma else 'exact'} {count} x ({names}): route {route} ({'fused launches' if route else 'single calls'})  "
              f"multi {m[0]:.3f} [{m[1]:.3f} .. {m[2]:.3f}]  single {s[0]:.3f} [{s[1]:.3f} .. {s[2]:.3f}]  ratio {s[0] / m[0]:.2f} x "
              f"(bound {8 * count / (4 + 4 * count):.2f})  frac {(4 + 4 * count) * S * T / m[0] / 1e6 / PEAK:.3f}", flush=True)
        for i in range(len(alts)):
            t = med(times[f"alt{i}"])
            print(f"      alt{i} multi {t[0]:.3f} [{t[1]:.3f} .. {t[2]:.3f}]  shipped / alt{i} {m[0] / t[0]:.2f}", flush=True)
        for bank in A + B:
            bank.close()
        for L, ptrs in zip(alts, alt_banks):
            for ptr in ptrs:
                L.savgol_streambank_destroy(ptr)


if __name__ == "__main__":
    main()
