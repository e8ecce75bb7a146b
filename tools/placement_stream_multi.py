"""savgol_streambank_push_block_multi over buffers carved out of ONE allocation with a chosen pad between them (tools, not product): does the relative
position of the K + 1 blocks decide which of the call's two placement modes a run lands in?  Four fresh allocations per pad and shape.
    python tools/placement_stream_multi.py [> profiles/stream_multi_placement.txt]"""
import os, sys, statistics
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from __graft_entry__ import load_package
sg = load_package()
import torch
S, T, K = 65536, 4096, 7
FILTERS = [(2, 0, 1.0), (2, 1, 1e-3), (3, 2, 0.5)]
def window(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(K): fn()
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) / K
busy = torch.randn((T, S), device="cuda")
for _ in range(20): busy.mul_(1.0000001)
block = S * T
for n, fma, count in ((4, 1, 2), (4, 1, 3), (8, 0, 2), (8, 0, 3)):
    banks = [sg.StreamBank(S, n, m, d, dt, fma=bool(fma)) for m, d, dt in FILTERS[:count]]
    keep = []
    for trial in range(4):
        line = []
        for pad_bytes in (0, 512, 4096, 65536, 1 << 20, (1 << 20) + 4096 + 512):
            pad = pad_bytes // 4
            big = torch.randn(((count + 1) * (block + pad) + 64,), device="cuda")
            keep.append(big)
            base = (-big.data_ptr() // 4) % 64                 # 256-byte aligned start
            ptrs = [big.data_ptr() + 4 * (base + i * (block + pad)) for i in range(count + 1)]
            fn = lambda: sg.push_block_multi(banks, ptrs[0], T, ptrs[1:])
            fn(); torch.cuda.synchronize()
            line.append(min(window(fn), window(fn)))
        print(f"n={n} fma={fma} K={count} trial {trial}: pad 0 / 512 / 4K / 64K / 1M / 1M+4.5K: " + "  ".join(f"{v:.3f}" for v in line), flush=True)
        if trial % 2 == 1:
            del keep[:]
            torch.cuda.empty_cache()
    for b in banks: b.close()
