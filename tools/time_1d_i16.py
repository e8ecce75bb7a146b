"""The int16-storage 1-D batch call (savgol_apply_batch_i16) against the fp32 call on the same shape, in one process, HIP events.
   python tools/time_1d_i16.py [--reps 8] [--sets 3] [--channels 4096] [--length 1048576] [--n 4,8,16,24,32] [--out profiles/i16_1d_time.txt] [--only i16-i16]
For every half window (m = 4, d = 0, one boundary mode) it times, alternating them inside every repetition and over `--sets` FRESH buffer sets (placement
alone moves the fp32 headline +-3 %): savgol_apply_batch_f32_ex with SAVGOL_BATCH_TILE_NARROW on pre-widened data, the new call int16 -> int16 and
int16 -> fp32, the caller's alternative in torch for both pairs (x.float() + the fp32 call, plus round / clamp / .to(int16) for the int16 pair; into
preallocated buffers, so that the allocator is not timed), and savgol_hip_stream_copy of the same int16 buffers (the copy ceiling at 4 B per sample).
Before anything is timed, both outputs of every buffer set are asserted against the contract at this size.  Prints and writes, per variant: ms per launch
(median over sets x reps; min .. max of the per-set medians), Gsamples/s, the fraction of 8 TB/s at the variant's own bytes per sample, and the ratio to
the fp32 narrow-tile call.  --only runs one variant alone (counter and trace runs)."""
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
    ap.add_argument("--sets", type=int, default=3)
    ap.add_argument("--channels", type=int, default=4096)
    ap.add_argument("--length", type=int, default=1 << 20)
    ap.add_argument("--n", default="4,8,16,24,32")
    ap.add_argument("--mode", type=int, default=0)
    ap.add_argument("--out", default=None)
    ap.add_argument("--only", default="", help="only the variant with this label")
    a = ap.parse_args()
    import torch
    from __graft_entry__ import load_package
    sg = load_package()
    L = sg.lib()
    ch, length = a.channels, a.length
    samples = ch * length

    def event_ms(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1)

    # label -> bytes per sample the variant has to move (the torch alternatives: every pass counted)
    variants = [("fp32 narrow", 8), ("i16-i16", 4), ("i16-f32", 6), ("torch i16-i16", 2 + 4 + 8 + 4 + 4 + 4 + 2), ("torch i16-f32", 2 + 4 + 8), ("copy int16", 4)]
    if a.only:
        variants = [v for v in variants if v[0] == a.only]
    lines = []

    def emit(s):
        print(s, flush=True)
        lines.append(s)

    emit(f"# {ch} x {length}, m = 4, d = 0, boundary mode {a.mode}; {a.sets} fresh buffer sets x {a.reps} alternating repetitions; ms = median (min .. max of the per-set medians)")
    for n in [int(t) for t in a.n.split(",")]:
        f = sg.Filter(n, 4, 0, 1.0, a.mode)
        per_set = {v[0]: [] for v in variants}
        allms = {v[0]: [] for v in variants}
        keep = []                                                   # earlier sets stay allocated, so that every set is a fresh placement
        for _ in range(a.sets):
            x32 = torch.empty((ch, length), dtype=torch.float32, device="cuda")
            sg.synth(x32)
            x32.mul_(30000.0 / float(x32.abs().max())).round_()
            x16 = x32.to(torch.int16)                               # x32 == widen(x16) from here on
            y32 = torch.empty_like(x32)
            y16 = torch.empty_like(x16)
            w32 = torch.empty_like(x32)                             # the torch alternative's widened copy
            stream = torch.cuda.current_stream().cuda_stream

            def torch_f32():
                w32.copy_(x16)
                f.apply_batch(w32, y32, ch, length, flags=sg.SAVGOL_BATCH_TILE_NARROW)

            def torch_i16():
                torch_f32()
                torch.round(y32, out=y32)
                y32.clamp_(-32768.0, 32767.0)
                y16.copy_(y32)

            calls = {
                "fp32 narrow": lambda: f.apply_batch(x32, y32, ch, length, flags=sg.SAVGOL_BATCH_TILE_NARROW),
                "i16-i16": lambda: f.apply_batch_i16(x16, y16, ch, length),
                "i16-f32": lambda: f.apply_batch_i16(x16, y32, ch, length, out_dtype="f32"),
                "torch i16-i16": torch_i16,
                "torch i16-f32": torch_f32,
                "copy int16": lambda: L.savgol_hip_stream_copy(x16.data_ptr(), y16.data_ptr(), samples * 2, stream),
            }
            # the contract at this size, before anything is timed: the fp32 narrow-tile call on the widened input, converted once
            calls["fp32 narrow"]()
            want32 = y32.clone()
            calls["i16-f32"]()
            torch.cuda.synchronize()
            assert torch.equal(y32.view(torch.int32), want32.view(torch.int32)), f"n = {n}: int16 -> fp32 differs from the fp32 call"
            calls["i16-i16"]()
            torch.cuda.synchronize()
            got16 = y16.clone()
            torch.round(want32, out=want32)
            assert torch.equal(got16, want32.nan_to_num_(nan=0.0).clamp_(-32768.0, 32767.0).to(torch.int16)), f"n = {n}: int16 -> int16 differs from the converted fp32 call"
            del want32, got16
            for label, _ in variants:                               # warm-up: plans, tables, code objects
                calls[label]()
            torch.cuda.synchronize()
            got = {v[0]: [] for v in variants}
            for _ in range(a.reps):
                for label, _ in variants:
                    got[label].append(event_ms(calls[label]))
            for label, _ in variants:
                per_set[label].append(statistics.median(got[label]))
                allms[label] += got[label]
            keep.append((x32, x16, y32, y16))
            del w32
        del keep
        torch.cuda.empty_cache()
        base = statistics.median(allms["fp32 narrow"]) if "fp32 narrow" in allms else None
        for label, bps in variants:
            ms = statistics.median(allms[label])
            row = {"n": n, "variant": label, "ms": round(ms, 3), "ms_min": round(min(per_set[label]), 3), "ms_max": round(max(per_set[label]), 3),
                   "gsamples_s": round(samples / (ms * 1e-3) / 1e9, 1), "bytes_per_sample": bps, "fraction_of_8TBs": round(samples * bps / (ms * 1e-3) / PEAK, 3),
                   "ratio_to_fp32_narrow": round(base / ms, 3) if base else None}
            emit(json.dumps(row))
    if a.out:
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
