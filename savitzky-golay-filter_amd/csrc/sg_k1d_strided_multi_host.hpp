// sg_k1d_strided_multi_host.hpp -- the one host rule of savgol_apply_strided_multi_batch_f32 (several record fields from one pass over an
// array of structs): is a call FUSED (sg1d_strided_multi_kernel, sg_k1d_strided_multi.hpp) or is it `njobs` single calls in the caller's order,
// and how are a fused call's jobs dealt to launches.  Plain C++ without HIP and without the filter struct: the API function and its _route twin
// (sg_api_1d.cpp) both ask strided_multi_plan(), and tests/mock/strided_multi_plan.cpp holds it to a restatement in Python.
//
// The contract makes the fall-back free: the call leaves memory as the single calls in order would, so everything the fused kernel cannot do
// bit for bit -- or does not do faster -- simply IS those calls.
//
// FUSED needs all of:
//   njobs >= 2;  every filter the same half window;  under SAVGOL_BATCH_BOUNDARY_AWARE the same config.boundary (without it every strided call runs
//   POLYNOMIAL edges);  no SAVGOL_BATCH_REFERENCE_SUMMATION;  every field address (base + offset), both strides and both channel pitches multiples
//   of 4, both strides >= 4 (dword loads and stores);  count <= STRIDED_MULTI_MAX_LENGTH (32-bit sample indices in a launch);
//   NO OUTPUT FIELD SHARES A BYTE WITH ANY JOB'S INPUT FIELD OR WITH ANOTHER JOB'S OUTPUT FIELD -- tiles read their halos while other tiles store, and
//   a job that reads what an earlier job wrote wants the sequential semantics of the single calls (strided_fields_disjoint, the single call's own
//   test, applied pairwise);  the record sizes lie inside the shipped table strided_multi_per_launch().
// A fused call runs the jobs in the caller's order in groups of at most strided_multi_per_launch() jobs; a LAST group of one job is a single call.
#pragma once

#include <cstddef>
#include <cstdint>

namespace sg {

constexpr int STRIDED_MULTI_MAX_JOBS = 16;                 // == SAVGOL_STRIDED_MULTI_MAX_JOBS (savgol_hip.h; sg_api_1d.cpp asserts it)
// jobs one launch of sg1d_strided_multi_kernel stages: one slab of 9.5 KB each in the wave's LDS (4 jobs: 38 KB per wave, four waves per CU)
constexpr int STRIDED_MULTI_MAX_PER_LAUNCH = 4;
constexpr size_t STRIDED_MULTI_MAX_LENGTH = (size_t)1 << 30;     // LAUNCH_MAX_LENGTH of sg_api_1d.cpp

// Two fields of `count` records in `channels` channels -- field = 4 bytes at a + c * pitch + i * stride: do they share NO byte?  The single call's
// test (savgol_apply_strided_batch_f32_ex), conservative: true where the whole extents do not overlap, or where both lie on ONE record grid (equal
// strides and pitches, whole records per pitch) with offsets at least 4 bytes apart cyclically; everything else counts as shared.
inline bool strided_fields_disjoint(uintptr_t a, size_t a_stride, size_t a_pitch, uintptr_t b, size_t b_stride, size_t b_pitch, size_t channels, size_t count)
{
    const uintptr_t ae = a + (channels - 1) * a_pitch + (count - 1) * a_stride + 4, be = b + (channels - 1) * b_pitch + (count - 1) * b_stride + 4;
    if (ae <= b || be <= a) return true;                                // the two arrays do not overlap at all
    if (a_stride == b_stride && a_pitch == b_pitch && a_stride != 0 && a_pitch % a_stride == 0) {
        const uintptr_t d = (a <= b ? b - a : a - b) % a_stride;
        return d >= 4 && a_stride - d >= 4;
    }
    return false;
}

// THE SHIPPED TABLE: how many jobs one fused launch takes for records of these sizes, 0 = the call is single calls.  By measurement
// (tools/time_strided_multi.py, profiles/strided_multi_time.txt): a shape is fused only where the fused call's median is ahead of the
// single calls it replaces by more than the single calls' own spread over buffer sets in the same run, and only measured record sizes are listed.
// Measured: equal strides of 8 / 12 / 16 / 20 / 32 / 64 bytes, both layouts, n = 5 / 16 / 32, 2 to 16 jobs: 1.94-2.77 x for two jobs per launch,
// 2.73-4.06 x for three and four, against a spread of 0.2-10.8 %.  No measured shape is level or behind, so the layout (a second array, or other
// fields of the same records) is no key; unequal strides and every other record size were not measured and take single calls.
constexpr int strided_multi_per_launch(size_t in_stride, size_t out_stride)
{
    const bool measured = in_stride == out_stride && (in_stride == 8 || in_stride == 12 || in_stride == 16 || in_stride == 20 || in_stride == 32 || in_stride == 64);
    return measured ? STRIDED_MULTI_MAX_PER_LAUNCH : 0;
}

struct StridedMultiField { int half_window, boundary; uintptr_t in, out; };     // one job: its filter's two deciding fields, its field ADDRESSES (base + offset)

struct StridedMultiPlan {
    int launches;                               // fused launches; 0 = njobs single calls
    int groups;                                 // a fused call: the groups in order, per[g] jobs each; per[g] == 1 (only the last can be) is a single call
    int per[STRIDED_MULTI_MAX_JOBS];
};

// 1 <= njobs <= STRIDED_MULTI_MAX_JOBS and channels, count >= 1 (the API has refused or returned before)
inline StridedMultiPlan strided_multi_plan(const StridedMultiField *jobs, int njobs, size_t in_stride, size_t in_pitch, size_t out_stride, size_t out_pitch,
                                           size_t channels, size_t count, bool boundary_aware, bool reference_summation)
{
    StridedMultiPlan plan = {};
    if (njobs < 2 || njobs > STRIDED_MULTI_MAX_JOBS || reference_summation || count > STRIDED_MULTI_MAX_LENGTH) return plan;
    if (in_stride % 4 || out_stride % 4 || in_pitch % 4 || out_pitch % 4 || in_stride < 4 || out_stride < 4) return plan;
    for (int k = 0; k < njobs; ++k) {
        if (jobs[k].in % 4 || jobs[k].out % 4) return plan;
        if (jobs[k].half_window != jobs[0].half_window) return plan;
        if (boundary_aware && jobs[k].boundary != jobs[0].boundary) return plan;
    }
    for (int k = 0; k < njobs; ++k)
        for (int j = 0; j < njobs; ++j) {
            if (!strided_fields_disjoint(jobs[j].in, in_stride, in_pitch, jobs[k].out, out_stride, out_pitch, channels, count)) return plan;
            if (j < k && !strided_fields_disjoint(jobs[j].out, out_stride, out_pitch, jobs[k].out, out_stride, out_pitch, channels, count)) return plan;
        }
    const int per = strided_multi_per_launch(in_stride, out_stride);
    if (per < 2) return plan;
    for (int k = 0; k < njobs; k += per) {
        const int g = njobs - k < per ? njobs - k : per;
        plan.per[plan.groups++] = g;
        if (g >= 2) ++plan.launches;
    }
    return plan;
}

}  // namespace sg
