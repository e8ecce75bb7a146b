"""The 16-bit-storage 1-D batch call (savgol_apply_batch_h16) against the fp32 call on the same shape, in one process, HIP events.
   python tools/time_1d_h16.py [--reps 8] [--pairs 3] [--channels 4096] [--length 1048576] [--n 4,8,16,24,32] [--out profiles/h16_1d_time.txt] [--only bf16-bf16]
For every half window (m = 4, d = 0, one boundary mode) it times, alternating them inside every repetition and over `--pairs` FRESH buffer pairs (placement
alone moves the fp32 headline +-3 %): savgol_apply_batch_f32_ex with default flags and with SAVGOL_BATCH_TILE_NARROW, the new call for bf16 -> bf16,
f16 -> f16 and bf16 -> f32, and savgol_hip_stream_copy of the same 16-bit buffers (the copy ceiling at 4 B per sample).  Prints and writes, per variant:
ms per launch (median over pairs x reps; min .. max of the per-pair medians), Gsamples/s, the fraction of 8 TB/s at the variant's own bytes per sample, and
the ratio to the fp32 narrow-tile call.  --only runs one variant alone (counter and trace runs).
   python tools/time_1d_h16.py --libs lib_parent/libsavgol_hip.so lib/libsavgol_hip.so lib_parent/libsavgol_hip.so [--n 5,32]
instead A/Bs the 16-bit call of several builds (bf16 -> bf16, f16 -> f16, bf16 -> f32) on the same buffers, interleaved inside every repetition
(tools/ab_libs.py)."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PEAK = 8e12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=8)
    ap.add_argument("--pairs", type=int, default=3)
    ap.add_argument("--channels", type=int, default=4096)
    ap.add_argument("--length", type=int, default=1 << 20)
    ap.add_argument("--n", default="4,8,16,24,32")
    ap.add_argument("--mode", type=int, default=0)
    ap.add_argument("--out", default=None)
    ap.add_argument("--only", default="", help="only the variant with this label")
    ap.add_argument("--libs", nargs="+", default=None, help="A/B the 16-bit call of these builds (list the first one again last for the run's own noise)")
    a = ap.parse_args()
    import torch
    from __graft_entry__ import load_package
    sg = load_package()
    if a.libs:
        return ab_libs_main(a, sg, torch)
    L = sg.lib()
    ch, length = a.channels, a.length
    samples = ch * length
    T16 = {"f16": torch.float16, "bf16": torch.bfloat16}

    def event_ms(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1)

    # label -> (bytes per sample, needs)
    variants = [("fp32 default", 8), ("fp32 narrow", 8), ("bf16-bf16", 4), ("f16-f16", 4), ("bf16-f32", 6), ("copy 16-bit", 4)]
    if a.only:
        variants = [v for v in variants if v[0] == a.only]
    lines, rows = [], []

    def emit(s):
        print(s, flush=True)
        lines.append(s)

    emit(f"# {ch} x {length}, m = 4, d = 0, boundary mode {a.mode}; {a.pairs} fresh buffer pairs x {a.reps} alternating repetitions; ms = median (min .. max of the per-pair medians)")
    for n in [int(t) for t in a.n.split(",")]:
        f = sg.Filter(n, 4, 0, 1.0, a.mode)
        per_pair = {v[0]: [] for v in variants}
        allms = {v[0]: [] for v in variants}
        keep = []                                                   # earlier pairs stay allocated, so that every pair is a fresh placement
        for _ in range(a.pairs):
            x32 = torch.empty((ch, length), dtype=torch.float32, device="cuda")
            sg.synth(x32)
            xs = {k: x32.to(t) for k, t in T16.items()}
            y32 = torch.empty_like(x32)
            ys = {k: torch.empty_like(v) for k, v in xs.items()}
            stream = torch.cuda.current_stream().cuda_stream
            calls = {
                "fp32 default": lambda: f.apply_batch(x32, y32, ch, length, flags=0),
                "fp32 narrow": lambda: f.apply_batch(x32, y32, ch, length, flags=sg.SAVGOL_BATCH_TILE_NARROW),
                "bf16-bf16": lambda: f.apply_batch(xs["bf16"], ys["bf16"], ch, length, dtype="bf16"),
                "f16-f16": lambda: f.apply_batch(xs["f16"], ys["f16"], ch, length, dtype="f16"),
                "bf16-f32": lambda: f.apply_batch(xs["bf16"], y32, ch, length, dtype="bf16", out_dtype="f32"),
                "copy 16-bit": lambda: L.savgol_hip_stream_copy(xs["bf16"].data_ptr(), ys["bf16"].data_ptr(), samples * 2, stream),
            }
            for label, _ in variants:                               # warm-up: plans, tables, code objects
                calls[label]()
            torch.cuda.synchronize()
            got = {v[0]: [] for v in variants}
            for _ in range(a.reps):
                for label, _ in variants:
                    got[label].append(event_ms(calls[label]))
            for label, _ in variants:
                per_pair[label].append(statistics.median(got[label]))
                allms[label] += got[label]
            keep.append((x32, xs, y32, ys))
        del keep
        torch.cuda.empty_cache()
        base = statistics.median(allms["fp32 narrow"]) if "fp32 narrow" in allms else None
        for label, bps in variants:
            ms = statistics.median(allms[label])
            row = {"n": n, "variant": label, "ms": round(ms, 3), "ms_min": round(min(per_pair[label]), 3), "ms_max": round(max(per_pair[label]), 3),
                   "gsamples_s": round(samples / (ms * 1e-3) / 1e9, 1), "bytes_per_sample": bps, "fraction_of_8TBs": round(samples * bps / (ms * 1e-3) / PEAK, 3),
                   "ratio_to_fp32_narrow": round(base / ms, 3) if base else None}
            rows.append(row)
            emit(json.dumps(row))
    if a.out:
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


def ab_libs_main(a, sg, torch):
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    import ab_libs
    ch, length = a.channels, a.length
    x32 = torch.empty((ch, length), dtype=torch.float32, device="cuda")
    sg.synth(x32)
    xs = {"f16": x32.to(torch.float16), "bf16": x32.to(torch.bfloat16)}
    ys = {"f16": torch.empty_like(xs["f16"]), "bf16": torch.empty_like(xs["bf16"]), "f32": x32}      # (x32 is free once it has been narrowed)
    libs = [ab_libs.load(p) for p in a.libs]
    st = torch.cuda.current_stream().cuda_stream
    code = {"f32": sg.SAVGOL_HIP_F32, "f16": sg.SAVGOL_HIP_F16, "bf16": sg.SAVGOL_HIP_BF16}
    for n in [int(t) for t in a.n.split(",")]:
        for tin, tout in (("bf16", "bf16"), ("f16", "f16"), ("bf16", "f32")):
            calls = []
            for lib in libs:
                f = ab_libs.new_filter(lib, n, 4, 0, 1.0, a.mode)

                def call(lib=lib, f=f):
                    assert lib.savgol_apply_batch_h16(f, xs[tin].data_ptr(), code[tin], ys[tout].data_ptr(), code[tout], ch, length, length, length, 0, st) == 0
                calls.append(call)
            ab_libs.report(f"h16 {tin}->{tout} n={n}", a.libs, ab_libs.alternate(calls, a.reps))


if __name__ == "__main__":
    main()
