"""Times savgol_streambank_push_block_h16 against the fp32 savgol_streambank_push_block on config 3's shape (tools, not product).

For every (half window, bank, filter) and the type pairs bf16 -> bf16 and bf16 -> fp32: blocks issued back to back (K per window, device events around
the window) on a chip kept busy first, the 16-bit call and the fp32 call on the same bank shape interleaved window by window in one process, every round
on a fresh pair of buffers (placement moves a launch by +- 3 %).  Reports the median and the spread of the per-block time, the fraction of the 8 TB/s
roofline at 4 B (16 -> 16) / 6 B (16 -> fp32) / 8 B (fp32) per stream-tick, the ratio against the fp32 call, and the head's cost: a 64-tick 16-bit call
(widen, two bands of fp32 tiles, round, tail store -- everything of a call but its body kernel) timed the same way, as a share of the whole call.
    python tools/time_stream_block_h16.py [> profiles/stream_h16_time.txt]
STREAMS, TICKS, HALF_WINDOWS, ROUNDS, K override the shape and the effort."""
import os
import statistics
import sys

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


def main():
    assert torch.cuda.is_available() and sg.device_count() > 0, sg.last_error()
    print(f"# {S} streams x {T} ticks, {ROUNDS} rounds of {K} blocks back to back per variant, interleaved, fresh buffers every round; ms per block: median [min .. max]")
    print("# frac = bytes per stream-tick x streams x ticks / time / 8 TB/s; ratio = fp32 median / 16-bit median (> 1: the 16-bit call is faster)")
    shapes = []
    for n in NS:
        for fma in (0, 1):
            shapes.append((n, fma, 2, 1, 1e-3))             # config 3's filter
        if n == 16:
            shapes.append((n, 1, 2, 0, 1.0))                # a smoothing filter on the fused bank
    busy = torch.randn((T, S), device="cuda")
    for _ in range(20):                                     # a chip kept busy first
        busy.mul_(1.0000001)
    for n, fma, m, d, dt in shapes:
        bank = sg.StreamBank(S, n, m, d, dt, fma=bool(fma))
        times = {"f32": [], "bf16": [], "bf16->f32": [], "head": []}
        for r in range(ROUNDS + 1):
            x32 = torch.randn((T, S), device="cuda")
            o32 = torch.empty_like(x32)
            x16 = x32.to(torch.bfloat16)
            o16 = torch.empty_like(x16)
            runs = {
                "f32": lambda: bank.push_block(x32, T, o32),
                "bf16": lambda: bank.push_block_h16(x16, "bf16", T, o16),
                "bf16->f32": lambda: bank.push_block_h16(x16, "bf16", T, o32, "f32"),
                "head": lambda: bank.push_block_h16(x16, "bf16", 64, o16),
            }
            for name, fn in runs.items():
                assert fn() >= 0, sg.last_error()
            torch.cuda.synchronize()
            for name, fn in runs.items():
                ms = window(fn)
                if r:                                       # round 0 warms up
                    times[name].append(ms)
            del x32, o32, x16, o16
        f32 = med(times["f32"])
        head = med(times["head"])
        print(f"n={n:2d} {'fused' if fma else 'exact'} m={m} d={d}: fp32 {f32[0]:.3f} [{f32[1]:.3f} .. {f32[2]:.3f}] frac {8 * S * T / f32[0] / 1e6 / PEAK:.3f}")
        for name, bytes_per in (("bf16", 4), ("bf16->f32", 6)):
            t = med(times[name])
            print(f"      {name:10s} {t[0]:.3f} [{t[1]:.3f} .. {t[2]:.3f}] frac {bytes_per * S * T / t[0] / 1e6 / PEAK:.3f}  ratio {f32[0] / t[0]:.2f} x   "
                  f"head (a 64-tick call) {head[0]:.3f} = {100 * head[0] / t[0]:.1f} % of the call")
        bank.close()


if __name__ == "__main__":
    main()
