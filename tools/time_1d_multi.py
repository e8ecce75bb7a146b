"""The fused multi-output 1-D call (savgol_apply_multi_batch_f32) against `count` default single calls on the same buffers, HIP events.
   python tools/time_1d_multi.py [--reps 10] [--channels 4096] [--length 1048576] [--json out.json] [--case mode0] [--fused-only]
Cases: n = 32, m = 4, d = 0 / 1 / 2 in all four boundary modes (the singles take the block-moment kernel for d <= 1, the plain one for d = 2);
n = 5, m = 3, d = 0 / 1 / 2 (config 1's filter, batched) and n = 16, m = 4, d = 0 / 1 (count 2), fused with SAVGOL_BATCH_TILE_NARROW -- without it
their derivative outputs keep the single calls' wide tile and run unfused (include/savgol_hip.h).  Prints ms (median), the speed-up over the single
calls and the fraction of 8 TB/s at (4 + 4 count) bytes per input sample (the singles' own bytes are count x 8).
   python tools/time_1d_multi.py --libs lib_parent/libsavgol_hip.so lib/libsavgol_hip.so lib_parent/libsavgol_hip.so [--case ...]
instead A/Bs the FUSED call of several builds on the same buffers, interleaved inside every repetition (tools/ab_libs.py)."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PEAK = 8e12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--channels", type=int, default=4096)
    ap.add_argument("--length", type=int, default=1 << 20)
    ap.add_argument("--json", default=None)
    ap.add_argument("--case", default="", help="only the cases whose label contains this")
    ap.add_argument("--fused-only", action="store_true", help="time only the fused call (counter runs)")
    ap.add_argument("--sweep", action="store_true", help="instead: half windows 4..32, count 2 and 3, against narrow plain-summation single calls")
    ap.add_argument("--libs", nargs="+", default=None, help="A/B the fused call of these builds (list the first one again last for the run's own noise)")
    a = ap.parse_args()
    import torch
    from __graft_entry__ import load_package
    sg = load_package()
    ch, L = a.channels, a.length
    if a.libs:
        return ab_libs_main(a, sg, torch)
    x = torch.empty((ch, L), dtype=torch.float32, device="cuda")
    sg.synth(x)
    outs = [torch.empty_like(x) for _ in range(3)]

    def timed(fn):
        fn()                                                  # warm-up: plans, tables
        torch.cuda.synchronize()
        ts = []
        for _ in range(a.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            ts.append(e0.elapsed_time(e1))
        ts.sort()
        return ts[len(ts) // 2]

    cases = [(f"n32 m4 d012 mode{mode}", 32, [(4, d) for d in (0, 1, 2)], mode, 0) for mode in range(4)]
    cases += [("n5 m3 d012 narrow", 5, [(3, d) for d in (0, 1, 2)], 0, sg.SAVGOL_BATCH_TILE_NARROW),
              ("n5 m3 d012 auto", 5, [(3, d) for d in (0, 1, 2)], 0, 0),
              ("n16 m4 d01 narrow", 16, [(4, d) for d in (0, 1)], 0, sg.SAVGOL_BATCH_TILE_NARROW)]
    single_flags = None
    if a.sweep:
        cases = [(f"sweep n{n} count{k}", n, [(4, d) for d in range(k)], 0, sg.SAVGOL_BATCH_TILE_NARROW) for n in (4, 8, 12, 16, 20, 24, 28, 32) for k in (2, 3)]
        single_flags = sg.SAVGOL_BATCH_TILE_NARROW | sg.SAVGOL_BATCH_PLAIN_SUMMATION
    rows = []
    for label, n, fs, mode, flags in cases:
        if a.case not in label:
            continue
        filters = [sg.Filter(n, m, d, 1.0, mode) for (m, d) in fs]
        k = len(filters)
        t_fused = timed(lambda: sg.apply_multi_batch(filters, x, outs[:k], ch, L, flags=flags))
        if a.fused_only:
            print(json.dumps({"case": label, "fused_ms": round(t_fused, 3)}), flush=True)
            continue
        t_single = timed(lambda: [f.apply_batch(x, o, ch, L, flags=single_flags) for f, o in zip(filters, outs)])
        row = {"case": label, "channels": ch, "length": L, "count": k, "fused_ms": round(t_fused, 3), "singles_ms": round(t_single, 3),
               "speedup": round(t_single / t_fused, 3), "fused_roofline": round(ch * L * (4 + 4 * k) / (t_fused * 1e-3) / PEAK, 3),
               "singles_roofline": round(ch * L * 8 * k / (t_single * 1e-3) / PEAK, 3)}
        rows.append(row)
        print(json.dumps(row), flush=True)
    if a.json:
        with open(a.json, "w") as fh:
            json.dump(rows, fh, indent=1)


def ab_libs_main(a, sg, torch):
    import ctypes as C
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    import ab_libs
    ch, L = a.channels, a.length
    x = torch.empty((ch, L), dtype=torch.float32, device="cuda")
    sg.synth(x)
    outs = [torch.empty_like(x) for _ in range(3)]
    libs = [ab_libs.load(p) for p in a.libs]
    st = torch.cuda.current_stream().cuda_stream
    for label, n, ds, flags in (("n32 m4 d012", 32, (0, 1, 2), 0), ("n16 m4 d01 narrow", 16, (0, 1), sg.SAVGOL_BATCH_TILE_NARROW), ("n5 m3 d012 narrow", 5, (0, 1, 2), sg.SAVGOL_BATCH_TILE_NARROW)):
        if a.case not in label:
            continue
        k = len(ds)
        calls = []
        for lib in libs:
            fs = (sg._F * k)(*[ab_libs.new_filter(lib, n, 3 if n == 5 else 4, d) for d in ds])
            ptrs = (C.c_void_p * k)(*[o.data_ptr() for o in outs[:k]])

            def call(lib=lib, fs=fs, ptrs=ptrs):
                assert lib.savgol_apply_multi_batch_f32(fs, k, x.data_ptr(), ptrs, ch, L, L, L, flags, st) == 0
            calls.append(call)
        ab_libs.report(f"multi {label}", a.libs, ab_libs.alternate(calls, a.reps))


if __name__ == "__main__":
    main()
