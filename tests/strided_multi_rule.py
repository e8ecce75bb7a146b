"""The host rule of savgol_apply_strided_multi_batch_f32 restated in Python from the call's contract (include/savgol_hip.h, csrc/sg_k1d_strided_multi_host.hpp),
for tests/test_strided_multi_host.py (which holds the C++ rule and the library's _route to it without a GPU) and tests/test_gpu_strided_multi.py (which
checks _route against it before every call).  Not a test module.

A call is (jobs, in_stride, in_pitch, out_stride, out_pitch, channels, count, flags) with jobs = [(half_window, boundary, in_address, out_address)]:
the field ADDRESSES, base + offset."""
REF, AWARE = 1, 32                               # SAVGOL_BATCH_REFERENCE_SUMMATION, SAVGOL_BATCH_BOUNDARY_AWARE
MAX_JOBS = 16
MAX_LENGTH = 1 << 30


def per_launch(in_stride, out_stride):
    """THE SHIPPED TABLE (strided_multi_per_launch): jobs per fused launch, 0 = single calls; only measured record sizes are fused"""
    if in_stride != out_stride or in_stride not in (8, 12, 16, 20, 32, 64):
        return 0
    return 4


def disjoint(a, a_stride, a_pitch, b, b_stride, b_pitch, channels, count):
    """the single call's test: no overlap of the whole extents, or one record grid with offsets at least 4 bytes apart cyclically"""
    ae = a + (channels - 1) * a_pitch + (count - 1) * a_stride + 4
    be = b + (channels - 1) * b_pitch + (count - 1) * b_stride + 4
    if ae <= b or be <= a:
        return True
    if a_stride == b_stride and a_pitch == b_pitch and a_stride != 0 and a_pitch % a_stride == 0:
        d = abs(a - b) % a_stride
        return d >= 4 and a_stride - d >= 4
    return False


def groups(jobs, in_stride, in_pitch, out_stride, out_pitch, channels, count, flags):
    """[] = single calls, else the job counts of a fused call's groups in order (a last group of 1 is a single call)"""
    n = len(jobs)
    if n < 2 or n > MAX_JOBS or (flags & REF) or count > MAX_LENGTH:
        return []
    if any(v % 4 for v in (in_stride, out_stride, in_pitch, out_pitch)) or in_stride < 4 or out_stride < 4:
        return []
    if any(j[2] % 4 or j[3] % 4 for j in jobs):
        return []
    if any(j[0] != jobs[0][0] for j in jobs):
        return []
    if (flags & AWARE) and any(j[1] != jobs[0][1] for j in jobs):
        return []
    for k, jk in enumerate(jobs):
        for j, jj in enumerate(jobs):
            if not disjoint(jj[2], in_stride, in_pitch, jk[3], out_stride, out_pitch, channels, count):
                return []
            if j < k and not disjoint(jj[3], out_stride, out_pitch, jk[3], out_stride, out_pitch, channels, count):
                return []
    per = per_launch(in_stride, out_stride)
    if per < 2:
        return []
    return [min(per, n - k) for k in range(0, n, per)]


def launches(*call):
    """what _route returns for a call that is not refused"""
    return sum(1 for g in groups(*call) if g >= 2)
