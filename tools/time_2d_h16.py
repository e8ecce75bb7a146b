"""The 2-D batch call on 16-bit storage (savgol2d_apply_batch_h16) against the fp32 call on the same shape, in one process, HIP events.
   python tools/time_2d_h16.py [--reps 6] [--pairs 3] [--images 64] [--size 4096] [--out profiles/2d_h16_time.txt]
Every line is one (half window, boundary, type pair) of the order-3 smoothing filter and times, alternating them inside every repetition and over
`--pairs` FRESH buffer sets (earlier sets stay allocated: placement alone moves the 2-D numbers by +-3 %):
  h16     the call, tile route
  fp32    (a) savgol2d_apply_batch_f32 on the same frames in fp32 -- the parent's code, the reference point
  staged  (b) the call with SAVGOL_HIP_2D_H16_TILES=0 (the switch is read at every call): widen + fp32 call + round inside the library
  torch   (c) what a 16-bit caller did before: x.float(), the fp32 call, .to(dtype) with torch ops
The chip is kept busy for --busy seconds before a line is measured.  Prints and writes per variant: ms per call (median over pairs x reps; min .. max of
the per-pair medians), the ratio fp32 ms / variant ms ("level" inside +-3 %), and for h16 / fp32 the fraction of 8 TB/s at the variant's own bytes per
pixel (4: 16 -> 16 bit, 6: 16 bit -> fp32, 8: fp32)."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PEAK = 8e12
BOUNDARY = {"VALID": 0, "CONSTANT": 1, "REFLECT": 2}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=6)
    ap.add_argument("--pairs", type=int, default=3)
    ap.add_argument("--images", type=int, default=64)
    ap.add_argument("--size", type=int, default=4096)
    ap.add_argument("--busy", type=float, default=1.0)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    from __graft_entry__ import load_package
    sg = load_package()
    images, rows, cols = a.images, a.size, a.size
    pixels = images * rows * cols
    T16 = {"f16": torch.float16, "bf16": torch.bfloat16}
    lines_todo = [(n, "REFLECT", "bf16", "bf16") for n in (2, 4, 7, 10, 16)] + [(7, "VALID", "bf16", "bf16"), (7, "CONSTANT", "bf16", "bf16"),
                                                                                 (4, "REFLECT", "bf16", "f32"), (7, "REFLECT", "bf16", "f32")]
    out_lines = []

    def emit(s):
        print(s, flush=True)
        out_lines.append(s)

    def event_ms(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1)

    emit(f"# {images} frames of {rows} x {cols}, order 3; {a.pairs} fresh buffer sets x {a.reps} alternating repetitions after {a.busy} s of load; "
         f"ms = median (min .. max of the per-set medians); ratio = fp32 ms / variant ms, 'level' inside +-3 %")
    variants = ["h16", "fp32", "staged", "torch"]
    for n, bname, tin, tout in lines_todo:
        b = BOUNDARY[bname]
        f = sg.Filter2D(n, n, 3)
        per_set = {v: [] for v in variants}
        allms = {v: [] for v in variants}
        keep = []
        for _ in range(a.pairs):
            x32 = torch.empty((images, rows, cols), dtype=torch.float32, device="cuda")
            sg.synth(x32.view(images * rows, cols))
            x16 = x32.to(T16[tin])
            x32.copy_(x16)                                                    # the fp32 call sees the same (quantised) frames
            y32 = torch.zeros_like(x32)
            y16 = y32 if tout == "f32" else torch.zeros_like(x16)

            def h16(tiles):
                os.environ["SAVGOL_HIP_2D_H16_TILES"] = "1" if tiles else "0"
                f.apply_batch_h16(x16, tin, y16, rows, cols, images, out_dtype=tout, boundary=b)

            def by_torch():
                w = x16.float()
                o = torch.empty_like(w)
                f.apply_batch(w, o, rows, cols, images, boundary=b)
                return o if tout == "f32" else o.to(T16[tin])

            calls = {"h16": lambda: h16(True), "fp32": lambda: f.apply_batch(x32, y32, rows, cols, images, boundary=b), "staged": lambda: h16(False), "torch": by_torch}
            for v in variants:
                calls[v]()
            torch.cuda.synchronize()
            t0 = time.time()
            while time.time() - t0 < a.busy:                                  # keep the chip busy: clocks and power state of a sustained run
                calls["fp32"]()
                torch.cuda.synchronize()
            got = {v: [] for v in variants}
            for _ in range(a.reps):
                for v in variants:
                    got[v].append(event_ms(calls[v]))
            for v in variants:
                per_set[v].append(statistics.median(got[v]))
                allms[v] += got[v]
            keep.append((x32, x16, y32, y16))
        del keep
        torch.cuda.empty_cache()
        os.environ.pop("SAVGOL_HIP_2D_H16_TILES", None)
        base = statistics.median(allms["fp32"])
        bpp = {"h16": 4 if tout != "f32" else 6, "fp32": 8}
        for v in variants:
            ms = statistics.median(allms[v])
            ratio = base / ms
            row = {"n": n, "boundary": bname, "pair": f"{tin}->{tout}", "variant": v, "ms": round(ms, 3), "ms_min": round(min(per_set[v]), 3),
                   "ms_max": round(max(per_set[v]), 3), "ratio_to_fp32": round(ratio, 3), "verdict": "level" if abs(ratio - 1.0) <= 0.03 else ("ahead" if ratio > 1 else "behind")}
            if v in bpp:
                row["bytes_per_pixel"] = bpp[v]
                row["fraction_of_8TBs"] = round(pixels * bpp[v] / (ms * 1e-3) / PEAK, 3)
            emit(json.dumps(row))
        f.close()
    if a.out:
        with open(a.out, "w") as fh:
            fh.write("\n".join(out_lines) + "\n")


if __name__ == "__main__":
    main()
