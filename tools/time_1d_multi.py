"""The fused multi-output 1-D call (savgol_apply_multi_batch_f32) against `count` default single calls on the same buffers, HIP events.
   python tools/time_1d_multi.py [--reps 10] [--channels 4096] [--length 1048576] [--json out.json] [--case mode0] [--fused-only]
Cases: n = 32, m = 4, d = 0 / 1 / 2 in all four boundary modes (the singles take the block-moment kernel for d <= 1, the plain one for d = 2);
n = 5, m = 3, d = 0 / 1 / 2 (config 1's filter, batched) and n = 16, m = 4, d = 0 / 1 (count 2), fused with SAVGOL_BATCH_TILE_NARROW -- without it
their derivative outputs keep the single calls' wide tile and run unfused (include/savgol_hip.h).  Prints ms (median), the speed-up over the single
calls and the fraction of 8 TB/s at (4 + 4 count) bytes per input sample (the singles' own bytes are count x 8).
   python tools/time_1d_multi.py --libs lib_parent/libsavgol_hip.so lib/libsavgol_hip.so lib_parent/libsavgol_hip.so [--case ...]
instead A/Bs the FUSED call of several builds on the same buffers, interleaved inside every repetition (tools/ab_libs.py).
   python tools/time_1d_multi.py --h16 bf16 [--out-dtype f32] [--pairs 3] [--txt profiles/multi_h16_1d_time.txt]
instead times the fused call on 16-bit storage (savgol_apply_multi_batch_h16), n = 4 / 8 / 16 / 32 and count 2 / 3, on `pairs` fresh buffer sets that
alternate inside every repetition, against: count 16-bit single calls with SAVGOL_BATCH_PLAIN_SUMMATION, the fp32 fused call on the widened data
(SAVGOL_BATCH_TILE_NARROW), and device copies of the same 16-bit buffers (the input copied into each of the count outputs: 4 count bytes per sample, against the fused call's 2 + 2 count).
   python tools/time_1d_multi.py --i16 [--out-dtype f32] [--pairs 3] [--txt profiles/multi_i16_1d_time.txt]
instead times the fused call on int16 storage (savgol_apply_multi_batch_i16), the same shapes, against: count int16 single calls with
SAVGOL_BATCH_PLAIN_SUMMATION, count int16 single calls with default flags (block moments from n = 20: what a caller has without this call), the bf16
fused call on buffers of the same size, the fp32 fused call on the widened data, and the caller's detour in torch (widen, the fp32 fused call, and for
int16 outputs round / nan_to_num / clamp / cast per output, into preallocated buffers)."""
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
    ap.add_argument("--h16", default=None, choices=("f16", "bf16"), help="instead: the fused call on 16-bit storage of this type")
    ap.add_argument("--i16", action="store_true", help="instead: the fused call on int16 storage")
    ap.add_argument("--out-dtype", default=None, choices=("f32",), help="--h16 / --i16: fp32 outputs instead of the input's type")
    ap.add_argument("--pairs", type=int, default=3, help="--h16: fresh buffer sets alternating inside every repetition")
    ap.add_argument("--txt", default=None, help="--h16: also write the table here")
    a = ap.parse_args()
    import torch
    from __graft_entry__ import load_package
    sg = load_package()
    ch, L = a.channels, a.length
    if a.libs:
        return ab_libs_main(a, sg, torch)
    if a.h16:
        return h16_main(a, sg, torch)
    if a.i16:
        return i16_main(a, sg, torch)
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


def h16_main(a, sg, torch):
    ch, L = a.channels, a.length
    t16 = {"f16": torch.float16, "bf16": torch.bfloat16}[a.h16]
    tout = torch.float32 if a.out_dtype == "f32" else t16
    in_b, out_b = 2, 4 if a.out_dtype == "f32" else 2
    x32 = torch.empty((ch, L), dtype=torch.float32, device="cuda")
    sg.synth(x32)
    # `pairs` buffer sets allocated afresh (input + three outputs each); every timed repetition runs once on each set, so the median is over placements too
    sets = []
    for _ in range(a.pairs):
        sets.append((x32.to(t16), [torch.empty((ch, L), dtype=tout, device="cuda") for _ in range(3)]))
    outs32 = [torch.empty_like(x32) for _ in range(3)]

    def timed(fns):
        for fn in fns:                                        # warm-up: plans, tables
            fn()
        torch.cuda.synchronize()
        ts = []
        for _ in range(a.reps):
            for fn in fns:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                fn()
                e1.record()
                e1.synchronize()
                ts.append(e0.elapsed_time(e1))
        ts.sort()
        return ts[len(ts) // 2], ts[0], ts[-1]

    PLAIN, NARROW = sg.SAVGOL_BATCH_PLAIN_SUMMATION, sg.SAVGOL_BATCH_TILE_NARROW
    head = f"# savgol_apply_multi_batch_h16, {ch} x {L}, {a.h16} -> {a.out_dtype or a.h16}, {a.pairs} buffer sets alternating, {a.reps} repetitions each; ms = median (min .. max)"
    cols = "# n count | fused16 ms (min .. max) | singles16 ms | fp32 fused ms | count copies ms | singles16 / fused16 | fp32 fused / fused16 | copies / fused16 | fused16 of 8 TB/s at (2 + 2 count) B"
    lines = [head, cols]
    print(head + "\n" + cols, flush=True)
    rows = []
    for n in (4, 8, 16, 32):
        for k in (2, 3):
            label = f"h16 n{n} count{k}"
            if a.case not in label:
                continue
            filters = [sg.Filter(n, 4, d, 1.0, 0) for d in range(k)]
            fused = timed([lambda x=x, o=o: sg.apply_multi_batch(filters, x, o[:k], ch, L, dtype=a.h16, out_dtype=a.out_dtype) for x, o in sets])
            single = timed([lambda x=x, o=o: [f.apply_batch(x, y, ch, L, dtype=a.h16, out_dtype=a.out_dtype, flags=PLAIN) for f, y in zip(filters, o)] for x, o in sets])
            f32 = timed([lambda: sg.apply_multi_batch(filters, x32, outs32[:k], ch, L, flags=NARROW)])
            if in_b == out_b:
                copy = timed([lambda x=x, o=o: [y.copy_(x) for y in o[:k]] for x, o in sets])
            else:
                copy = (float("nan"),) * 3
            row = {"case": label, "channels": ch, "length": L, "n": n, "count": k, "in": a.h16, "out": a.out_dtype or a.h16, "fused_ms": round(fused[0], 3),
                   "fused_min_ms": round(fused[1], 3), "fused_max_ms": round(fused[2], 3), "singles_ms": round(single[0], 3), "fp32_fused_ms": round(f32[0], 3),
                   "copy_ms": round(copy[0], 3), "speedup_over_singles": round(single[0] / fused[0], 3), "speedup_over_fp32_fused": round(f32[0] / fused[0], 3),
                   "copy_over_fused": round(copy[0] / fused[0], 3), "fused_roofline": round(ch * L * (in_b + out_b * k) / (fused[0] * 1e-3) / PEAK, 3)}
            rows.append(row)
            line = (f"{n:>3} {k} | {fused[0]:7.3f} ({fused[1]:.3f} .. {fused[2]:.3f}) | {single[0]:7.3f} | {f32[0]:7.3f} | {copy[0]:7.3f} | "
                    f"{single[0] / fused[0]:5.3f} x | {f32[0] / fused[0]:5.3f} x | {copy[0] / fused[0]:5.3f} | {row['fused_roofline']:.3f}")
            lines.append(line)
            print(line, flush=True)
    if a.txt:
        with open(a.txt, "w") as fh:
            fh.write("\n".join(lines) + "\n")
    if a.json:
        with open(a.json, "w") as fh:
            json.dump(rows, fh, indent=1)


def i16_main(a, sg, torch):
    ch, L = a.channels, a.length
    out_name = "f32" if a.out_dtype == "f32" else "i16"
    tout = torch.float32 if out_name == "f32" else torch.int16
    in_b, out_b = 2, 4 if out_name == "f32" else 2
    x32 = torch.empty((ch, L), dtype=torch.float32, device="cuda")
    sg.synth(x32)
    x32.mul_(30000.0 / float(x32.abs().max())).round_()             # x32 == widen(x16) from here on
    # `pairs` buffer sets allocated afresh (int16 input, bf16 input of the same size, three outputs); every timed repetition runs once on each set
    sets = []
    for _ in range(a.pairs):
        sets.append((x32.to(torch.int16), x32.to(torch.bfloat16), [torch.empty((ch, L), dtype=tout, device="cuda") for _ in range(3)]))
    outs32 = [torch.empty_like(x32) for _ in range(3)]
    w32 = torch.empty_like(x32)                                     # the detour's widened copy

    def timed(fns):
        for fn in fns:                                        # warm-up: plans, tables
            fn()
        torch.cuda.synchronize()
        ts = []
        for _ in range(a.reps):
            for fn in fns:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                fn()
                e1.record()
                e1.synchronize()
                ts.append(e0.elapsed_time(e1))
        ts.sort()
        return ts[len(ts) // 2], ts[0], ts[-1]

    PLAIN, NARROW = sg.SAVGOL_BATCH_PLAIN_SUMMATION, sg.SAVGOL_BATCH_TILE_NARROW
    head = f"# savgol_apply_multi_batch_i16, {ch} x {L}, i16 -> {out_name}, {a.pairs} buffer sets alternating, {a.reps} repetitions each; ms = median (min .. max)"
    cols = (f"# n count | fused i16 ms (min .. max) | plain singles ms | default singles ms | bf16 fused ms | fp32 fused ms | torch detour ms | plain singles / fused | "
            f"default singles / fused | bf16 fused / fused | fp32 fused / fused | detour / fused | fused of 8 TB/s at (2 + {out_b} count) B")
    lines = [head, cols]
    print(head + "\n" + cols, flush=True)
    rows = []
    for n in (4, 8, 16, 32):
        for k in (2, 3):
            label = f"i16 n{n} count{k}"
            if a.case not in label:
                continue
            filters = [sg.Filter(n, 4, d, 1.0, 0) for d in range(k)]

            def detour(x, o):
                w32.copy_(x)
                sg.apply_multi_batch(filters, w32, outs32[:k], ch, L, flags=NARROW)
                if out_name == "i16":
                    for y32, y in zip(outs32, o[:k]):
                        torch.round(y32, out=y32)
                        y32.nan_to_num_(nan=0.0).clamp_(-32768.0, 32767.0)
                        y.copy_(y32)

            # the contract at this size, before anything is timed: every output is the detour's
            x, _, o = sets[0]
            sg.apply_multi_batch_i16(filters, x, o[:k], ch, L, out_dtype=out_name)
            got = [y.clone() for y in o[:k]]
            detour(x, o)
            torch.cuda.synchronize()
            for j in range(k):
                want = o[j] if out_name == "i16" else outs32[j]
                assert torch.equal(got[j].view(torch.int16), want.view(torch.int16)), f"n = {n}, output {j}: the fused int16 call differs from the converted fp32 fused call"
            del got
            fused = timed([lambda x=x, o=o: sg.apply_multi_batch_i16(filters, x, o[:k], ch, L, out_dtype=out_name) for x, _, o in sets])
            plain = timed([lambda x=x, o=o: [f.apply_batch_i16(x, y, ch, L, out_dtype=out_name, flags=PLAIN) for f, y in zip(filters, o)] for x, _, o in sets])
            default = timed([lambda x=x, o=o: [f.apply_batch_i16(x, y, ch, L, out_dtype=out_name) for f, y in zip(filters, o)] for x, _, o in sets])
            as16 = (lambda y: y) if out_name == "f32" else (lambda y: y.view(torch.bfloat16))
            bf16 = timed([lambda xb=xb, o=o: sg.apply_multi_batch(filters, xb, [as16(y) for y in o[:k]], ch, L, dtype="bf16", out_dtype=a.out_dtype) for _, xb, o in sets])
            f32 = timed([lambda: sg.apply_multi_batch(filters, x32, outs32[:k], ch, L, flags=NARROW)])
            torch_ms = timed([lambda x=x, o=o: detour(x, o) for x, _, o in sets[:1]])
            row = {"case": label, "channels": ch, "length": L, "n": n, "count": k, "in": "i16", "out": out_name, "fused_ms": round(fused[0], 3),
                   "fused_min_ms": round(fused[1], 3), "fused_max_ms": round(fused[2], 3), "plain_singles_ms": round(plain[0], 3), "default_singles_ms": round(default[0], 3),
                   "bf16_fused_ms": round(bf16[0], 3), "fp32_fused_ms": round(f32[0], 3), "torch_detour_ms": round(torch_ms[0], 3),
                   "fused_roofline": round(ch * L * (in_b + out_b * k) / (fused[0] * 1e-3) / PEAK, 3)}
            rows.append(row)
            line = (f"{n:>3} {k} | {fused[0]:7.3f} ({fused[1]:.3f} .. {fused[2]:.3f}) | {plain[0]:7.3f} | {default[0]:7.3f} | {bf16[0]:7.3f} | {f32[0]:7.3f} | {torch_ms[0]:7.3f} | "
                    f"{plain[0] / fused[0]:5.3f} x | {default[0] / fused[0]:5.3f} x | {bf16[0] / fused[0]:5.3f} x | {f32[0] / fused[0]:5.3f} x | {torch_ms[0] / fused[0]:6.3f} x | "
                    f"{row['fused_roofline']:.3f}")
            lines.append(line)
            print(line, flush=True)
    if a.txt:
        with open(a.txt, "w") as fh:
            fh.write("\n".join(lines) + "\n")
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
