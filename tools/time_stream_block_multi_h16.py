"""Times savgol_streambank_push_block_multi_h16 against the single savgol_streambank_push_block_h16 calls it replaces, and against the fp32 fused call on
widened samples, on config 3's shape (tools, not product).

For every (bank kind, half window, set of filters, type pair): blocks issued back to back (K per window, device events around the window) on a chip kept
busy first; the multi call on banks A, the `count` single 16-bit calls on banks B and savgol_streambank_push_block_multi on banks C (samples widened to
fp32 beforehand, outside the timed window), all of the same configurations, interleaved window by window in one process, every round on fresh buffers
(the earlier rounds' buffers stay allocated until the shape is done, so new pages back the new ones; placement moves a launch by +- 3 %).  Before
timing, at this size, the multi outputs are asserted equal to the single calls' bit for bit.  ALT=path[,path] adds further builds of the library to the
same process (tools/ab_libs.py): their multi calls are interleaved with the shipped build's, for launch-shape A/Bs.  Reports the median and the spread
of the per-block time, the ratio to the single calls (> 1: the multi call is faster; the byte bound is 4 count / (2 + 2 count) for 16 -> 16 bit and
6 count / (2 + 4 count) for 16 bit -> fp32), the ratio to the fp32 fused call, the fraction of the 8 TB/s roofline at the call's own bytes, and the
route the call took.
    python tools/time_stream_block_multi_h16.py [> profiles/stream_multi_h16_time.txt]
STREAMS, TICKS, HALF_WINDOWS, KINDS, PAIRS, ROUNDS, K override the shape and the effort."""
import ctypes as C
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
PAIRS = [tuple(p.split(":")) for p in os.environ.get("PAIRS", "bf16:bf16,bf16:f32").split(",")]
ROUNDS, K = int(os.environ.get("ROUNDS", "5")), int(os.environ.get("K", "7"))
ALT = [p for p in os.environ.get("ALT", "").split(",") if p]
PEAK = 8000.0                                               # GB/s
FILTERS = [(2, 0, 1.0), (2, 1, 1e-3), (3, 2, 0.5)]           # value, velocity, acceleration: (m 2, d 0), (m 2, d 1), (m 3, d 2)
FOURTH = (4, 0, 1.0)
DTYPE = {"f16": torch.float16, "bf16": torch.bfloat16, "f32": torch.float32}


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
            for pair in PAIRS:
                for count in (2, 3, 4):
                    f = [g if g[0] <= 2 * n else (2, g[1], g[2]) for g in FILTERS + [FOURTH]]       # a window of 2n + 1 holds order <= 2n
                    yield n, fma, f[:count], pair


def main():
    assert torch.cuda.is_available() and sg.device_count() > 0, sg.last_error()
    print(f"# {S} streams x {T} ticks, {ROUNDS} rounds of {K} blocks back to back per variant, interleaved, fresh buffers every round; ms per block: median [min .. max]")
    print("# ratio = single 16-bit calls' median / multi call's median (> 1: the multi call is faster); vs f32 = the fp32 fused call's median on widened samples / "
          "the multi call's; frac = the call's own bytes (2 + e count per stream-tick, e = 2 or 4) / multi time / 8 TB/s")
    busy = torch.randn((T, S), device="cuda")
    for _ in range(20):                                     # a chip kept busy first
        busy.mul_(1.0000001)
    alts = []
    if ALT:
        import ab_libs
        alts = [ab_libs.load(p) for p in ALT]
        print("# alt builds, interleaved in this process: " + ", ".join(f"alt{i} = {os.path.basename(os.path.dirname(p))}" for i, p in enumerate(ALT)))
    st = torch.cuda.current_stream().cuda_stream
    for n, fma, filters, pair in shapes():
        count = len(filters)
        it, ot = sg._STORAGE[pair[0]], sg._STORAGE[pair[1]]
        elem = 4 if pair[1] == "f32" else 2
        A, B, Cb = ([sg.StreamBank(S, n, m, d, dt, fma=bool(fma)) for m, d, dt in filters] for _ in range(3))
        # the same banks in every alt build, through its own C ABI
        alt_banks = []
        for L in alts:
            ptrs = [L.savgol_streambank_create_ex(C.byref(sg.SavgolConfig(n, m, d, dt, 0)), S, sg.SAVGOL_STREAMBANK_FMA if fma else 0) for m, d, dt in filters]
            assert all(ptrs)
            alt_banks.append(ptrs)
        times = {"multi": [], "single": [], "f32": []}
        times.update({f"alt{i}": [] for i in range(len(alts))})
        route = None
        keep = []
        for r in range(ROUNDS + 1):
            x32 = torch.randn((T, S), device="cuda")
            x = x32.to(DTYPE[pair[0]])
            x32 = x.float()                                 # the widened samples of the fp32 fused call
            oa = [torch.empty((T, S), dtype=DTYPE[pair[1]], device="cuda") for _ in range(count)]
            ob = [torch.empty((T, S), dtype=DTYPE[pair[1]], device="cuda") for _ in range(count)]
            oc = [torch.empty((T, S), device="cuda") for _ in range(count)]
            keep.append((x, x32, oa, ob, oc))
            outs = (C.c_void_p * count)(*[o.data_ptr() for o in oa])

            def multi():
                return min(sg.push_block_multi_h16(A, x, pair[0], T, oa, pair[1]))

            def single():
                return min(B[k].push_block_h16(x, pair[0], T, ob[k], pair[1]) for k in range(count))

            def wide():
                return min(sg.push_block_multi(Cb, x32, T, oc))

            def alt(i):
                return lambda: alts[i].savgol_streambank_push_block_multi_h16((C.c_void_p * count)(*alt_banks[i]), count, x.data_ptr(), it, T, outs, ot, None, st)

            if route is None:
                route = sg.push_block_multi_h16_route(A, x, pair[0], T, oa, pair[1])
            assert multi() >= 0 and single() >= 0 and wide() >= 0, sg.last_error()
            torch.cuda.synchronize()
            view = torch.int32 if elem == 4 else torch.int16
            for k in range(count):                          # round 0, fresh banks on both sides: rows 2n .. T - 1 hold outputs
                lo = 2 * n if r == 0 else 0
                assert torch.equal(oa[k][lo:].view(view), ob[k][lo:].view(view)), ("the multi call left its twin's bits", n, fma, filters[k], pair, r)
            runs = [("multi", multi), ("single", single), ("f32", wide)] + [(f"alt{i}", alt(i)) for i in range(len(alts))]
            for i in range(len(alts)):
                assert runs[3 + i][1]() >= 0
            for name, fn in runs:
                ms = window(fn)
                if r:                                       # round 0 warms up
                    times[name].append(ms)
        del keep, x, x32, oa, ob, oc
        torch.cuda.empty_cache()
        m, s, w = med(times["multi"]), med(times["single"]), med(times["f32"])
        names = " + ".join(f"m{f[0]}d{f[1]}" for f in filters)
        bound = (2 + elem) * count / (2 + elem * count)
        print(f"n={n:2d} {'fused' if fma else 'exact'} {pair[0]}->{pair[1]} {count} x ({names}): route {route} ({'fused launches' if route else 'single calls'})  "
              f"multi {m[0]:.3f} [{m[1]:.3f} .. {m[2]:.3f}]  single {s[0]:.3f} [{s[1]:.3f} .. {s[2]:.3f}]  ratio {s[0] / m[0]:.2f} x (bound {bound:.2f})  "
              f"f32 fused {w[0]:.3f} [{w[1]:.3f} .. {w[2]:.3f}]  vs f32 {w[0] / m[0]:.2f} x  frac {(2 + elem * count) * S * T / m[0] / 1e6 / PEAK:.3f}", flush=True)
        for i in range(len(alts)):
            t = med(times[f"alt{i}"])
            print(f"      alt{i} multi {t[0]:.3f} [{t[1]:.3f} .. {t[2]:.3f}]  shipped / alt{i} {m[0] / t[0]:.2f}", flush=True)
        for bank in A + B + Cb:
            bank.close()
        for L, ptrs in zip(alts, alt_banks):
            for ptr in ptrs:
                L.savgol_streambank_destroy(ptr)


if __name__ == "__main__":
    main()
