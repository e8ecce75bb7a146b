"""The 2-D batch call on int16 storage (savgol2d_apply_batch_i16) against the fp32 call, the bf16 call, its own staged route and the caller's detour in
torch, on the same shape, in one process, HIP events.
   python tools/time_2d_i16.py [--reps 6] [--pairs 3] [--images 64] [--size 4096] [--out profiles/2d_i16_time.txt]
Every line is one (half window, boundary, output type) of the order-3 smoothing filter and times, alternating them inside every repetition and over
`--pairs` FRESH buffer sets (earlier sets stay allocated: placement alone moves the 2-D numbers by +-3 %):
  i16     the call, tile route (sg2d_rolling_i16_kernel)
  fp32    (a) savgol2d_apply_batch_f32 on the widened frames -- the reference point of every ratio
  bf16    (b) savgol2d_apply_batch_h16 bf16 -> bf16 (bf16 -> fp32 on the int16 -> fp32 lines) on the same BYTES: the same traffic through the tile whose
          storage types are run-time fields (sg2d_rolling_h16_kernel)
  staged  (c) the call with SAVGOL_HIP_2D_I16_TILES=0 (the switch is read at every call): widen + fp32 call + convert inside the library
  torch   (d) what an int16 caller did before: x.float(), the fp32 call, round / clamp / cast with torch ops
The chip is kept busy for --busy seconds before a line is measured.  Prints and writes per variant: ms per call (median over pairs x reps; min .. max of
the per-pair medians), the ratio fp32 ms / variant ms ("level" inside +-3 %), and for i16 / bf16 / fp32 the fraction of 8 TB/s at the variant's own bytes
per pixel (4: 16 -> 16 bit, 6: 16 bit -> fp32, 8: fp32)."""
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
    shapes = [(n, "REFLECT") for n in (2, 4, 7, 10, 16)] + [(7, "VALID"), (7, "CONSTANT")]
    lines_todo = [(n, b, tout) for n, b in shapes for tout in ("i16", "f32")]
    out_lines = []

    def emit(s):
        print(s, flush=True)
        out_lines.append(s)
        if a.out:                                                             # written as it goes: a run cut short keeps its lines
            with open(a.out, "w") as fh:
                fh.write("\n".join(out_lines) + "\n")

    def event_ms(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1)

    emit(f"# {images} frames of {rows} x {cols}, order 3; {a.pairs} fresh buffer sets x {a.reps} alternating repetitions after {a.busy} s of load; "
         f"ms = median (min .. max of the per-set medians); ratio = fp32 ms / variant ms, 'level' inside +-3 %")
    variants = ["i16", "fp32", "bf16", "staged", "torch"]
    for n, bname, tout in lines_todo:
        b = BOUNDARY[bname]
        f = sg.Filter2D(n, n, 3)
        per_set = {v: [] for v in variants}
        allms = {v: [] for v in variants}
        keep = []
        for _ in range(a.pairs):
            x32 = torch.empty((images, rows, cols), dtype=torch.float32, device="cuda")
            sg.synth(x32.view(images * rows, cols))
            # 14-bit unsigned counts, as detector data is: an int16 word below 0x4000 read as bf16 is a finite number below 2, so neither an input word
            # nor any box sum of (b) is a NaN or an Inf, which would send the bf16 tile down its cold redo paths and make (b) a comparison of something
            # else (its output is asserted finite below)
            xi = torch.round(x32 * 2000.0 + 8000.0).clamp_(0, 16000).to(torch.int16)
            x32.copy_(xi)                                                     # the fp32 call sees the same frames, widened
            xb = xi.view(torch.bfloat16)                                      # the same bytes read as bf16: the traffic is what is compared, not the values
            y32 = torch.zeros_like(x32)
            yi = y32 if tout == "f32" else torch.zeros_like(xi)
            yb = y32 if tout == "f32" else torch.zeros((images, rows, cols), dtype=torch.bfloat16, device="cuda")

            def i16(tiles):
                os.environ["SAVGOL_HIP_2D_I16_TILES"] = "1" if tiles else "0"
                f.apply_batch_i16(xi, yi, rows, cols, images, out_dtype=tout, boundary=b)

            def by_torch():
                w = xi.float()
                o = torch.empty_like(w)
                f.apply_batch(w, o, rows, cols, images, boundary=b)
                return o if tout == "f32" else torch.round(o).clamp_(-32768, 32767).to(torch.int16)

            calls = {"i16": lambda: i16(True), "fp32": lambda: f.apply_batch(x32, y32, rows, cols, images, boundary=b),
                     "bf16": lambda: f.apply_batch_h16(xb, "bf16", yb, rows, cols, images, out_dtype="bf16" if tout == "i16" else "f32", boundary=b),
                     "staged": lambda: i16(False), "torch": by_torch}
            os.environ.pop("SAVGOL_HIP_2D_I16_TILES", None)
            route = f.apply_batch_i16_route(xi, yi, rows, cols, images, out_dtype=tout, boundary=b)
            assert route == 1, f"the timed call does not take the tiles: route {route} ({sg.last_error()!r}), in {xi.data_ptr():#x}, out {yi.data_ptr():#x}"
            calls["bf16"]()
            torch.cuda.synchronize()
            assert bool(torch.isfinite(yb[0]).all()) and bool(torch.isfinite(yb[-1]).all()), "(b) ran on non-finite values: its cold paths would be timed"
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
            keep.append((x32, xi, y32, yi, yb))
        del keep
        torch.cuda.empty_cache()
        os.environ.pop("SAVGOL_HIP_2D_I16_TILES", None)
        base = statistics.median(allms["fp32"])
        bpp = {"i16": 4 if tout != "f32" else 6, "bf16": 4 if tout != "f32" else 6, "fp32": 8}
        for v in variants:
            ms = statistics.median(allms[v])
            ratio = base / ms
            row = {"n": n, "boundary": bname, "pair": f"i16->{tout}", "variant": v, "ms": round(ms, 3), "ms_min": round(min(per_set[v]), 3),
                   "ms_max": round(max(per_set[v]), 3), "ratio_to_fp32": round(ratio, 3), "verdict": "level" if abs(ratio - 1.0) <= 0.03 else ("ahead" if ratio > 1 else "behind")}
            if v in bpp:
                row["bytes_per_pixel"] = bpp[v]
                row["fraction_of_8TBs"] = round(pixels * bpp[v] / (ms * 1e-3) / PEAK, 3)
            emit(json.dumps(row))
        f.close()


if __name__ == "__main__":
    main()
