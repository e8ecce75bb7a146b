"""Two builds of libsavgol_hip.so must give the same BITS from every 1-D tile kernel (single fp32 / fp64, fused multi-output, 16-bit storage), in
one process on the same small inputs:   python tools/ab_1d_bits.py lib_parent/libsavgol_hip.so lib/libsavgol_hip.so
3 channels; lengths 2 TW + 5, TW - 1, 2n + 1 and 2 TW + 1 (a last tile body shorter than the halo) for every tile width; a vector-aligned and an
odd pitch; the four boundary modes and VALID; n in 1, 4, 5, 16, 19, 20, 32; derivative 0 and 1; time_step 0.5; out of place and in place; default,
narrow + plain-summation, wide-tile and (fp64) block-moment flags; 2 and 3 fused outputs; the four 16-bit type pairs.  Return codes are compared too
(a combination a build rejects must be rejected by both).  Outputs start from the same sentinel, so samples a call leaves alone count as well."""
import sys

import torch

import ab_libs

sg = ab_libs.package()
paths = sys.argv[1:3]
libs = [ab_libs.load(p) for p in paths]
CH, DT = 3, 0.5
st = torch.cuda.current_stream().cuda_stream
I = {torch.float32: torch.int32, torch.float64: torch.int64, torch.float16: torch.int16, torch.bfloat16: torch.int16}
STORE = {torch.float32: sg.SAVGOL_HIP_F32, torch.float16: sg.SAVGOL_HIP_F16, torch.bfloat16: sg.SAVGOL_HIP_BF16}
gen = torch.Generator(device="cuda").manual_seed(20)
counts = {}


def rows(length, pitch, dtype, fill=None):
    if fill is None:
        return (torch.randn((CH, pitch), generator=gen, device="cuda", dtype=torch.float32) * 3 + 40).to(dtype)   # an offset: derivative filters centre it
    return torch.full((CH, pitch), fill, device="cuda", dtype=dtype)


def check(family, what, results):
    """results: per build (return code, [tensors])"""
    (rc0, t0), (rc1, t1) = results
    ok = rc0 == rc1 and all(torch.equal(a.view(I[a.dtype]), b.view(I[b.dtype])) for a, b in zip(t0, t1))
    c = counts.setdefault(family, [0, 0, 0])
    c[0] += 1
    c[1] += rc0 != 0
    if not ok:
        c[2] += 1
        print(f"DIFFERS {family}: {what} (rc {rc0} / {rc1})", flush=True)


for n in (1, 4, 5, 16, 19, 20, 32):                             # (16: the only one of these whose wide fp32 tile has 12 vectors per lane)
    m = 2 if n == 1 else 4
    # tile widths (samples) of the kernels this half window can reach: narrow fp32, wide fp32 (16 or 12 vectors per lane), narrow and wide fp64
    for tw, dtypes in ((2048, "f32 multi h16"), (4096, "f32" if n <= 12 else ""), (3072, "f32" if 12 < n <= 18 else ""), (1024, "f64"), (2048, "f64" if n <= 24 else "")):
        for length in (2 * tw + 5, tw - 1, 2 * n + 1, 2 * tw + 1):
            for pitch in ((length + 7) // 8 * 8, length + (length % 2 == 0) + 2):
                for mode in range(4):
                    for valid in (False, True):
                        v = "valid_" if valid else ""
                        what = f"n={n} L={length} pitch={pitch} mode={mode} valid={valid}"
                        for dt in dtypes.split():
                            if dt in ("f32", "f64"):
                                dtype = torch.float32 if dt == "f32" else torch.float64
                                x = rows(length, pitch, dtype)
                                for d in (0, 1):
                                    for flags in (None, sg.SAVGOL_BATCH_TILE_NARROW | sg.SAVGOL_BATCH_PLAIN_SUMMATION, sg.SAVGOL_BATCH_TILE_WIDE,
                                                  sg.SAVGOL_BATCH_MOMENT_F64 if dt == "f64" else sg.SAVGOL_BATCH_TILE_WIDE | sg.SAVGOL_BATCH_PLAIN_SUMMATION):
                                        for inplace in (False, True):
                                            if inplace and valid:
                                                continue
                                            res = []
                                            for L in libs:
                                                f = ab_libs.new_filter(L, n, m, d, DT, mode)
                                                y = x.clone() if inplace else rows(length, pitch, dtype, -7.0)
                                                src = y if inplace else x
                                                fn = getattr(L, f"savgol_apply_{v}batch_{dt}" + ("" if flags is None else "_ex"))
                                                rc = fn(f, src.data_ptr(), y.data_ptr(), CH, length, pitch, pitch, *([] if flags is None else [flags]), st)
                                                torch.cuda.synchronize()
                                                L.savgol_destroy(f)
                                                res.append((rc, [y]))
                                            check(f"single {dt}", f"{what} d={d} flags={flags} inplace={inplace}", res)
                            elif dt == "multi":
                                x = rows(length, pitch, torch.float32)
                                for k in (2, 3):
                                    if k - 1 > m:
                                        continue
                                    res = []
                                    for L in libs:
                                        fs = [ab_libs.new_filter(L, n, m, d, DT, mode) for d in range(k)]
                                        ys = [rows(length, pitch, torch.float32, -7.0) for _ in range(k)]
                                        fn = getattr(L, f"savgol_apply_{v}multi_batch_f32")
                                        rc = fn((sg._F * k)(*fs), k, x.data_ptr(), (sg._vp * k)(*[y.data_ptr() for y in ys]), CH, length, pitch, pitch,
                                                sg.SAVGOL_BATCH_TILE_NARROW, st)
                                        torch.cuda.synchronize()
                                        for f in fs:
                                            L.savgol_destroy(f)
                                        res.append((rc, ys))
                                    check(f"multi K={k}", what, res)
                            else:
                                for tin, tout in ((torch.float16, torch.float16), (torch.bfloat16, torch.bfloat16), (torch.float16, torch.float32), (torch.bfloat16, torch.float32)):
                                    x = rows(length, pitch, tin)
                                    for d in (0, 1):
                                        res = []
                                        for L in libs:
                                            f = ab_libs.new_filter(L, n, m, d, DT, mode)
                                            y = rows(length, pitch, tout, -7.0)
                                            rc = getattr(L, f"savgol_apply_{v}batch_h16")(f, x.data_ptr(), STORE[tin], y.data_ptr(), STORE[tout], CH, length, pitch, pitch, 0, st)
                                            torch.cuda.synchronize()
                                            L.savgol_destroy(f)
                                            res.append((rc, [y]))
                                        check(f"h16 {str(tin)[6:]}->{str(tout)[6:]}", f"{what} d={d}", res)

print(f"# A = {paths[0]}, B = {paths[1]}")
bad = 0
for family, (total, rejected, differ) in sorted(counts.items()):
    bad += differ
    print(f"{family:28s} {total:6d} calls compared ({rejected} rejected by both builds alike), {differ} differ")
print("ALL BITS EQUAL" if not bad else f"{bad} CALLS DIFFER")
sys.exit(1 if bad else 0)
