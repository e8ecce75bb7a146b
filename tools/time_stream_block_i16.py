"""Times savgol_streambank_push_block_i16 on config 3's shape against what it is read against (tools, not product).

For every (half window, bank kind) on config 3's filter (m = 2, d = 1, dt = 1e-3) and the outputs int16 -> int16 and int16 -> fp32: blocks issued back
to back (K per window, device events around the window) after a quarter of a second of load on the chip, every variant interleaved window by window in
one process, every round on a fresh set of buffers (placement moves a launch by +- 3 %).  The variants:
    fp32        savgol_streambank_push_block on the samples widened beforehand (8 B per stream-tick; the widening itself is NOT timed);
    bf16        savgol_streambank_push_block_h16, bf16 -> bf16, the same shape: the same bytes as int16 -> int16, the figure that one is read against;
    i16         savgol_streambank_push_block_i16, int16 -> int16 (4 B);
    i16->f32    savgol_streambank_push_block_i16, int16 -> fp32 (6 B);
    detour      what a caller does without the call: x.float(), the fp32 push, round / nan_to_num / clamp / cast to int16 in torch.
Reports the median and the spread of the per-block time, the fraction of the 8 TB/s roofline at the variant's bytes per stream-tick, and the ratios.
    python tools/time_stream_block_i16.py [> profiles/stream_i16_time.txt]
STREAMS, TICKS, HALF_WINDOWS, ROUNDS, K override the shape and the effort."""
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from __graft_entry__ import load_package

sg = load_package()
import torch

S, T = int(os.environ.get("STREAMS", "65536")), int(os.environ.get("TICKS", "4096"))
NS = [int(v) for v in os.environ.get("HALF_WINDOWS", "4,8,16,32").split(",")]
ROUNDS, K = int(os.environ.get("ROUNDS", "5")), int(os.environ.get("K", "7"))
PEAK = 8000.0                                               # GB/s


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


def load(busy, seconds=0.25):
    """keeps the chip busy for `seconds` so that the first timed window does not start on idle clocks"""
    t0 = time.perf_counter()
    while time.perf_counter() - t0 < seconds:
        for _ in range(10):
            busy.mul_(1.0000001)
        torch.cuda.synchronize()


def main():
    assert torch.cuda.is_available() and sg.device_count() > 0, sg.last_error()
    print(f"# {S} streams x {T} ticks, m=2 d=1 dt=1e-3; {ROUNDS} rounds of {K} blocks back to back per variant after 0.25 s of load, interleaved, fresh buffers every round")
    print("# ms per block: median [min .. max]; frac = bytes per stream-tick x streams x ticks / time / 8 TB/s")
    print("# vs fp32 = fp32 median / this median, vs bf16 = bf16 median / this median, vs detour = detour median / this median (> 1: this call is faster)")
    busy = torch.randn((T, S), device="cuda")
    for n in NS:
        for fma in (0, 1):
            bank = sg.StreamBank(S, n, 2, 1, 1e-3, fma=bool(fma))
            times = {"fp32": [], "bf16": [], "i16": [], "i16->f32": [], "detour": []}
            for r in range(ROUNDS + 1):
                xi = (torch.randn((T, S), device="cuda") * 60.0).round().to(torch.int16)
                x32 = xi.float()
                o32 = torch.empty_like(x32)
                oi = torch.empty_like(xi)
                xb = x32.to(torch.bfloat16)
                ob = torch.empty_like(xb)

                def detour():
                    w = xi.float()
                    rc = bank.push_block(w, T, o32)
                    oi.copy_(torch.clamp(torch.nan_to_num(torch.round(o32), nan=0.0), -32768, 32767).to(torch.int16))
                    return rc

                runs = {
                    "fp32": lambda: bank.push_block(x32, T, o32),
                    "bf16": lambda: bank.push_block_h16(xb, "bf16", T, ob),
                    "i16": lambda: bank.push_block_i16(xi, T, oi),
                    "i16->f32": lambda: bank.push_block_i16(xi, T, o32, "f32"),
                    "detour": detour,
                }
                for name, fn in runs.items():
                    assert fn() >= 0, sg.last_error()
                torch.cuda.synchronize()
                load(busy)
                for name, fn in runs.items():
                    ms = window(fn)
                    if r:                                   # round 0 warms up
                        times[name].append(ms)
                del xi, x32, o32, oi, xb, ob
            m = {name: med(v) for name, v in times.items()}
            print(f"n={n:2d} {'fused' if fma else 'exact'}:")
            for name, bytes_per in (("fp32", 8), ("bf16", 4), ("i16", 4), ("i16->f32", 6), ("detour", 0)):
                t = m[name]
                line = f"      {name:9s} {t[0]:7.3f} [{t[1]:7.3f} .. {t[2]:7.3f}]"
                if bytes_per:
                    line += f"  frac {bytes_per * S * T / t[0] / 1e6 / PEAK:.3f}"
                if name.startswith("i16"):
                    line += f"  vs fp32 {m['fp32'][0] / t[0]:.2f} x  vs bf16 {m['bf16'][0] / t[0]:.2f} x  vs detour {m['detour'][0] / t[0]:.2f} x"
                print(line)
            bank.close()


if __name__ == "__main__":
    main()
