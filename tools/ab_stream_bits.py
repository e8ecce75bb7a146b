"""Two builds of libsavgol_hip.so must give the same BITS from every form of the stream block push (walk, register tiles, LDS-DMA tiles, block-moment
tiles), in one process on the same small inputs:   python tools/ab_stream_bits.py lib_parent/libsavgol_hip.so lib/libsavgol_hip.so
Per shape the same random samples go through a fresh bank of each build in calls of 7, 2n + 3 and the remaining ticks (a filling ring, a wrapped ring,
then tiles inside the call); stream 1 rides on an offset of 1e3 and stream 2 holds a NaN (the centring of the fused bank's derivative filters and its
Inf / NaN guard).  Outputs start from the same sentinel, so ticks a call leaves alone count as well; return codes are compared too.
    1024 aligned streams x 200 ticks, n in 1, 5, 6, 8, 11, 12, 16, 17, 20, 24, 32, both banks;
    the fused bank on (m, d) = (2, 1) and (2, 2) at n in 12, 16, 20: block moments, and the tap-by-tap tiles a centred bank with three terms keeps;
    260 aligned streams, n in 1, 12, 13, bit-exact bank: register tiles whose last strip has four streams, then the walk;
    777 streams behind a pointer one float off: the walk's element path, n in 4, 16, 17, 32.
With ONE library the list is just run (what a kernel trace of one build records)."""
import ctypes as C
import sys

import torch

import ab_libs

sg = ab_libs.package()
paths = sys.argv[1:3]
libs = [ab_libs.load(p) for p in paths]
st = torch.cuda.current_stream().cuda_stream
TICKS = 200

shapes = []                                                   # (streams, pointer offset in floats, n, m, d, fma)
for n in (1, 5, 6, 8, 11, 12, 16, 17, 20, 24, 32):
    for fma in (0, 1):
        shapes.append((1024, 0, n, min(3, 2 * n), 0, fma))
for m, d in ((2, 1), (2, 2)):
    for n in (12, 16, 20):
        shapes.append((1024, 0, n, m, d, 1))
for n in (1, 12, 13):
    shapes.append((260, 0, n, min(3, 2 * n), 0, 0))
for n in (4, 16, 17, 32):
    for fma in (0, 1):
        shapes.append((777, 1, n, 3, 1, fma))

bad = 0
for S, off, n, m, d, fma in shapes:
    g = torch.Generator(device="cuda").manual_seed(n * 1000 + S + fma)
    flat = torch.randn(TICKS * S + 4, generator=g, device="cuda", dtype=torch.float32)
    x = flat[off:off + TICKS * S].view(TICKS, S)
    x[:, 1] += 1e3
    x[100, 2] = float("nan")
    results = []
    for L in libs:
        cfg = sg.SavgolConfig(n, m, d, 0.5, 0)
        bank = L.savgol_streambank_create_ex(C.byref(cfg), S, 1 if fma else 0)
        assert bank, (S, n, m, d, fma)
        oflat = torch.full((TICKS * S + 4,), -7.0, device="cuda", dtype=torch.float32)
        out = oflat[off:off + TICKS * S].view(TICKS, S)
        rcs, t = [], 0
        for k in (7, 2 * n + 3, TICKS - 7 - (2 * n + 3)):
            rcs.append(L.savgol_streambank_push_block(bank, x[t].data_ptr(), k, out[t].data_ptr(), st))
            t += k
        torch.cuda.synchronize()
        L.savgol_streambank_destroy(bank)
        results.append((rcs, oflat))
    what = f"streams={S} offset={off} n={n} m={m} d={d} fma={fma}"
    if len(libs) == 2:
        same = results[0][0] == results[1][0] and torch.equal(results[0][1].view(torch.int32), results[1][1].view(torch.int32))
        bad += not same
        print(f"{'same bits' if same else 'DIFFERS  '} {what} rc {results[0][0]} / {results[1][0]}", flush=True)
    else:
        print(f"ran       {what} rc {results[0][0]}", flush=True)

print(f"# A = {paths[0]}" + (f", B = {paths[1]}" if len(paths) == 2 else ""))
if len(libs) == 2:
    print("ALL BITS EQUAL" if not bad else f"{bad} SHAPES DIFFER")
sys.exit(1 if bad else 0)
