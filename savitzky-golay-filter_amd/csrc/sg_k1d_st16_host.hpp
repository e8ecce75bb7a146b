// sg_k1d_st16_host.hpp -- what the host side needs to know about the 1-D kernels on 16-bit STORAGE (sg_k1d_st16.hpp, sg_k1d_multi_st16.hpp): the
// by-value jobs and the launchers, for both storage families -- fp16 / bf16 (`h16`: savgol_apply[_valid][_multi]_batch_h16) and int16 (`i16`:
// savgol_apply[_valid][_multi]_batch_i16).  A header of its own, so that nothing the fp32 / fp64 kernel objects are built from changes with it.
// No device code in here.
#pragma once

#include "sg_k1d_host.hpp"

namespace sg {

// storage types of a device buffer: the values of SAVGOL_HIP_F32 / _F16 / _BF16 / _I16 (include/savgol_hip.h)
enum : unsigned { STORE_F32 = 0, STORE_F16 = 1, STORE_BF16 = 2 };
enum : unsigned { STORE_I16_F32 = 0, STORE_I16 = 3 };

// A family's storage fields, as they follow the fp32 job in the kernarg (the int16 input has one type, so its block has no in_type), and the
// family's noun in the error texts.
struct H16Types {
    unsigned in_type;                   // STORE_F16 or STORE_BF16
    unsigned out_type;                  // the input's type, or STORE_F32
    static constexpr const char *NOUN = "16-bit";
};
struct I16Types {
    unsigned out_type;                  // STORE_I16 or STORE_I16_F32
    static constexpr const char *NOUN = "int16";
};

// `base` is the fp32 narrow-tile job of the widened input, field for field (out of place: no stash, no phases); `multi` the job enqueue_multi builds
// for the widened input under SAVGOL_BATCH_TILE_NARROW.  in_ld / out_ld / out_shift count elements of their own buffer's type; JOB_VEC_IN /
// JOB_VEC_OUT mean "every group of FOUR elements the tile kernels move as one vector is naturally aligned": 8 bytes for 16-bit rows, 16 bytes for fp32
// output rows.  All outputs of a fused job share out_type.  The types are wave-uniform: scalar branches at staging and at the stores.
// The fp32 job comes first and the family's fields follow it as the job's own (job.base, job.in_type, job.out_type): the kernarg layouts of
// struct { Job1D base; unsigned in_type, out_type; } and struct { Job1D base; unsigned out_type; }, and so for the fused jobs.
struct JobSt16Base      { Job1D base; };
struct JobMultiSt16Base { JobMulti1D multi; };
template <typename Types> struct JobSt16 : JobSt16Base, Types {};
template <typename Types> struct JobMultiSt16 : JobMultiSt16Base, Types {};
typedef JobSt16<H16Types>      JobH16;
typedef JobSt16<I16Types>      JobI16;
typedef JobMultiSt16<H16Types> JobMultiH16;
typedef JobMultiSt16<I16Types> JobMultiI16;
static_assert(sizeof(JobH16) == sizeof(Job1D) + 8 && sizeof(JobI16) == sizeof(Job1D) + 8 && sizeof(JobMultiH16) == sizeof(JobMulti1D) + 8 &&
              sizeof(JobMultiI16) == sizeof(JobMulti1D) + 8, "the storage fields follow the fp32 job directly (one or two words, padded to the job's 8 bytes)");
static_assert(sizeof(JobMultiH16) + sizeof(TapsMulti) < 4096 && sizeof(JobMultiI16) + sizeof(TapsMulti) < 4096, "the multi-output kernarg stays under 4 KB");

}  // namespace sg

// The launchers a family's objects export (F = h16 or i16):
//   * the plain three-chain kernel, one object per half-window group (the groups of the fp32 kernels, see the Makefile); 1 if this group owns n;
//   * the half-lane block-moment kernel (half windows 20..32), one object per moment count; 0 when enqueued;
//   * the fused kernel, one object per (output count, half-window group); 1 if this group owns n.
#define SG_ST16_GROUPS(prefix) {prefix##_g0, prefix##_g1, prefix##_g2, prefix##_g3}
#define SG_ST16_DECLARE_GROUPS(prefix, JOB, TAPS)                                                      \
    int prefix##_g0(int n, const sg::JOB *job, const sg::TAPS *taps, unsigned grid, void *stream);     \
    int prefix##_g1(int n, const sg::JOB *job, const sg::TAPS *taps, unsigned grid, void *stream);     \
    int prefix##_g2(int n, const sg::JOB *job, const sg::TAPS *taps, unsigned grid, void *stream);     \
    int prefix##_g3(int n, const sg::JOB *job, const sg::TAPS *taps, unsigned grid, void *stream);
#define SG_ST16_DECLARE(F, JOB, JOBMULTI)                                                                                \
    SG_ST16_DECLARE_GROUPS(sg1d_launch_##F, JOB, Taps)                                                                   \
    int sg1d_launch_##F##_momenth_t3(int n, const sg::JOB *job, const float *d_table, unsigned grid, void *stream);      \
    int sg1d_launch_##F##_momenth_t5(int n, const sg::JOB *job, const float *d_table, unsigned grid, void *stream);      \
    int sg1d_launch_##F##_momenth_t7(int n, const sg::JOB *job, const float *d_table, unsigned grid, void *stream);      \
    SG_ST16_DECLARE_GROUPS(sg1d_launch_multi_##F##_2, JOBMULTI, TapsMulti)                                               \
    SG_ST16_DECLARE_GROUPS(sg1d_launch_multi_##F##_3, JOBMULTI, TapsMulti)

extern "C" {
SG_ST16_DECLARE(h16, JobH16, JobMultiH16)
SG_ST16_DECLARE(i16, JobI16, JobMultiI16)

// The ONE entry point per route that the host calls (sg_k1d_st16_launch.cpp dispatches to the objects above); 0 when enqueued, -1 with the error text
// set otherwise.  sg1d_launch_i16: moment_terms = 0 takes the plain kernel with `taps`, 3 / 5 / 7 the block-moment kernel with `d_table`.  The fused
// two: k = 2 or 3 outputs.  WEAK: csrc/sg_api_1d.cpp is also linked without the kernel objects (the CPU launch record), where the symbols stay null and
// the calls refuse with "object not linked" (DESIGN 4.1d).  The h16 single route has no such entry point: it reaches its objects directly (launch_h16
// below, the block-moment table in csrc/sg_api_1d.cpp), which is what the launch record holds.
int sg1d_launch_i16(int n, int moment_terms, const sg::JobI16 *job, const sg::Taps *taps, const float *d_table, unsigned grid, void *stream) __attribute__((weak));
int sg1d_launch_multi_h16(int n, int k, const sg::JobMultiH16 *job, const sg::TapsMulti *taps, unsigned grid, void *stream) __attribute__((weak));
int sg1d_launch_multi_i16(int n, int k, const sg::JobMultiI16 *job, const sg::TapsMulti *taps, unsigned grid, void *stream) __attribute__((weak));
}

namespace sg {

// Asks the four half-window groups in turn (`groups` null: no object for this output count), then reports a failed launch.  `what` names the kernels
// in the texts ("16-bit-storage", "int16 multi-output", ...); k is the output count of a fused launch, 0 for the single kernel.
template <typename Job, typename TapsT>
inline int launch_groups16(int (*const *groups)(int, const Job *, const TapsT *, unsigned, void *), const char *what, int n, int k, const Job *job,
                           const TapsT *taps, unsigned grid, void *stream)
{
    const int hit = groups && (groups[0](n, job, taps, grid, stream) || groups[1](n, job, taps, grid, stream) ||
                               groups[2](n, job, taps, grid, stream) || groups[3](n, job, taps, grid, stream));
    if (!hit) {
        if (k) sg_set_error("no %s kernel for half_window %d, %d outputs", what, n, k);
        else sg_set_error("no %s kernel for half_window %d", what, n);
        return -1;
    }
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) { sg_set_error("%s kernel launch failed: %s", what, hipGetErrorString(e)); return -1; }
    return 0;
}

inline int launch_h16(int n, const JobH16 &job, const Taps &taps, unsigned grid, hipStream_t st)
{
    static constexpr int (*GROUPS[4])(int, const JobH16 *, const Taps *, unsigned, void *) = SG_ST16_GROUPS(sg1d_launch_h16);
    return launch_groups16(GROUPS, "16-bit-storage", n, 0, &job, &taps, grid, st);
}

}  // namespace sg
