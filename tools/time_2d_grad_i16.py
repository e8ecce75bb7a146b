"""The gradient on int16 frames (savgol2d_gradient_batch_i16) against the fp32 gradient call, its own staged route, two derivative-filter calls of
savgol2d_apply_batch_i16 and the caller's detour in torch, on the same shape, in one process, HIP events.
   python tools/time_2d_grad_i16.py [--reps 6] [--pairs 3] [--images 64] [--size 4096] [--out profiles/2d_grad_i16_time.txt]
Every line is one (order, half window, boundary, output type) and times, alternating them inside every repetition and over `--pairs` FRESH buffer sets
(earlier sets stay allocated: placement alone moves the 2-D numbers by +-3 %):
  direct  (a) the call, direct route (sg2d_rolling_hf_i16_kernel for gx, sg2d_rolling_gen_i16_kernel for gy)
  fp32    (b) savgol2d_gradient_batch_f32 on the widened frames -- the reference point of every ratio
  staged  (c) the call with SAVGOL_HIP_2D_GRAD_I16_DIRECT=0 (the switch is read at every call): widen + fp32 gradient + two converts inside the library
  apply2  (d) two savgol2d_apply_batch_i16 calls with derivative filters (both staged: each widens the stack again)
  torch   (e) what an int16 caller did before: x.float(), the fp32 gradient, round / clamp / cast with torch ops
Before a line is timed, (a), (c) and (d) are asserted bit-equal to (b) converted once (on the device, at the timed size).  The chip is kept busy for
--busy seconds before a line is measured.  Prints and writes per variant: ms per call (median over sets x reps; min .. max of the per-set medians), the
ratio fp32 ms / variant ms ("level" inside +-3 %), and for direct / fp32 the fraction of 8 TB/s at the variant's own bytes per pixel (8: int16 -> int16,
12: int16 -> fp32, 16: fp32 -- each frame reads the input once and writes one output)."""
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
SWITCH = "SAVGOL_HIP_2D_GRAD_I16_DIRECT"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=6)
    ap.add_argument("--pairs", type=int, default=3)
    ap.add_argument("--images", type=int, default=64)
    ap.add_argument("--size", type=int, default=4096)
    ap.add_argument("--busy", type=float, default=1.0)
    ap.add_argument("--orders", default="2,3")
    ap.add_argument("--windows", default="2,4,7")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    from __graft_entry__ import load_package
    sg = load_package()
    L = sg.lib()
    images, rows, cols = a.images, a.size, a.size
    pixels = images * rows * cols
    lines_todo = [(order, n, b, tout) for order in map(int, a.orders.split(",")) for n in map(int, a.windows.split(",")) for b in ("REFLECT", "VALID")
                  for tout in ("i16", "f32")]
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

    def narrow(w):
        return torch.round(w).clamp_(-32768, 32767).to(torch.int16)

    emit(f"# {images} frames of {rows} x {cols}; {a.pairs} fresh buffer sets x {a.reps} alternating repetitions after {a.busy} s of load; "
         f"ms = median (min .. max of the per-set medians); ratio = fp32 ms / variant ms, 'level' inside +-3 %")
    variants = ["direct", "fp32", "staged", "apply2", "torch"]
    for order, n, bname, tout in lines_todo:
        b = BOUNDARY[bname]
        fx, fy = sg.Filter2D(n, n, order, 1, 0), sg.Filter2D(n, n, order, 0, 1)
        per_set = {v: [] for v in variants}
        allms = {v: [] for v in variants}
        keep = []
        for s in range(a.pairs):
            x32 = torch.empty((images, rows, cols), dtype=torch.float32, device="cuda")
            sg.synth(x32.view(images * rows, cols))
            xi = torch.round(x32 * 2000.0 + 8000.0).clamp_(0, 16000).to(torch.int16)       # 14-bit counts, as detector data is
            x32.copy_(xi)                                                     # the fp32 call sees the same frames, widened
            odt = torch.float32 if tout == "f32" else torch.int16
            g32 = [torch.zeros_like(x32) for _ in range(2)]
            gi = [torch.zeros((images, rows, cols), dtype=odt, device="cuda") for _ in range(2)]
            gd = [torch.zeros((images, rows, cols), dtype=odt, device="cuda") for _ in range(2)]

            def grad16(direct, outs=gi):
                os.environ[SWITCH] = "1" if direct else "0"
                sg.gradient_batch_i16(n, n, order, xi, outs[0], outs[1], rows, cols, images, out_dtype=tout, boundary=b)

            def grad32(src=x32, outs=g32):
                rc = L.savgol2d_gradient_batch_f32(n, n, order, src.data_ptr(), rows, cols, cols, rows * cols, outs[0].data_ptr(), outs[1].data_ptr(), cols, rows * cols,
                                                   images, 1.0, 1.0, b, sg._stream(None))
                assert rc == 0, sg.last_error()

            def apply2():
                fx.apply_batch_i16(xi, gd[0], rows, cols, images, out_dtype=tout, boundary=b)
                fy.apply_batch_i16(xi, gd[1], rows, cols, images, out_dtype=tout, boundary=b)

            def by_torch():
                w = xi.float()
                o = [torch.empty_like(w), torch.empty_like(w)]
                grad32(w, o)
                return o if tout == "f32" else [narrow(o[0]), narrow(o[1])]

            calls = {"direct": lambda: grad16(True), "fp32": grad32, "staged": lambda: grad16(False), "apply2": apply2, "torch": by_torch}
            os.environ.pop(SWITCH, None)
            route = sg.gradient_batch_i16_route(n, n, order, xi, gi[0], gi[1], rows, cols, images, out_dtype=tout, boundary=b)
            assert route == 1, f"the timed call does not take the direct route: {route} ({sg.last_error()!r})"
            if s == 0:
                # outputs bit-equal at the timed size, before anything is timed: (b) converted once against (a), (c) and (d)
                grad32()
                want = [g if tout == "f32" else narrow(g) for g in g32]
                for name, outs in (("direct", gi), ("staged", gi), ("apply2", gd)):
                    for o in outs:
                        o.zero_()
                    calls[name]()
                    torch.cuda.synchronize()
                    for k in range(2):
                        assert torch.equal(outs[k].view(torch.int32 if tout == "f32" else torch.int16), want[k].view(torch.int32 if tout == "f32" else torch.int16)), \
                            (name, order, n, bname, tout, "gx" if k == 0 else "gy")
                del want
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
            keep.append((x32, xi, g32, gi, gd))
        del keep
        torch.cuda.empty_cache()
        os.environ.pop(SWITCH, None)
        base = statistics.median(allms["fp32"])
        bpp = {"direct": 8 if tout != "f32" else 12, "fp32": 16}
        for v in variants:
            ms = statistics.median(allms[v])
            ratio = base / ms
            row = {"order": order, "n": n, "boundary": bname, "pair": f"i16->{tout}", "variant": v, "ms": round(ms, 3), "ms_min": round(min(per_set[v]), 3),
                   "ms_max": round(max(per_set[v]), 3), "ratio_to_fp32": round(ratio, 3), "verdict": "level" if abs(ratio - 1.0) <= 0.03 else ("ahead" if ratio > 1 else "behind")}
            if v in bpp:
                row["bytes_per_pixel"] = bpp[v]
                row["fraction_of_8TBs"] = round(pixels * bpp[v] / (ms * 1e-3) / PEAK, 3)
            emit(json.dumps(row))
        fx.close()
        fy.close()


if __name__ == "__main__":
    main()
