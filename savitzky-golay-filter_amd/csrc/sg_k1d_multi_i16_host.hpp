// sg_k1d_multi_i16_host.hpp -- what the host side needs to know about the fused multi-output kernels on int16 storage (sg_k1d_multi_i16.hpp;
// savgol_apply[_valid]_multi_batch_i16): the by-value job and the launchers.  A header of its own, as JobI16 and JobMultiH16 have one, so that nothing
// the existing kernel objects are built from changes with it.  No device code in here.
#pragma once

#include "sg_k1d_host.hpp"
#include "sg_k1d_i16_host.hpp"

namespace sg {

// `multi` is the job enqueue_multi builds for the widened input under SAVGOL_BATCH_TILE_NARROW, field for field.  in_ld / out_ld / out_shift count
// elements of their own buffer's type; JOB_VEC_IN / JOB_VEC_OUT mean "every group of FOUR elements is naturally aligned" (8 bytes for int16 rows,
// 16 for fp32 output rows), as in JobI16.  All outputs share out_type, which is wave-uniform: a scalar branch at the stores.
struct JobMultiI16 {
    JobMulti1D multi;
    unsigned   out_type;                // STORE_I16 or STORE_I16_F32
};
static_assert(sizeof(JobMultiI16) + sizeof(TapsMulti) < 4096, "the multi-output kernarg stays under 4 KB");

}  // namespace sg

extern "C" {
// one object per (output count, half-window group), the groups of the fp32 kernels (see the Makefile); 1 if this group owns n
int sg1d_launch_multi_i16_2_g0(int n, const sg::JobMultiI16 *job, const sg::TapsMulti *taps, unsigned grid, void *stream);
int sg1d_launch_multi_i16_2_g1(int n, const sg::JobMultiI16 *job, const sg::TapsMulti *taps, unsigned grid, void *stream);
int sg1d_launch_multi_i16_2_g2(int n, const sg::JobMultiI16 *job, const sg::TapsMulti *taps, unsigned grid, void *stream);
int sg1d_launch_multi_i16_2_g3(int n, const sg::JobMultiI16 *job, const sg::TapsMulti *taps, unsigned grid, void *stream);
int sg1d_launch_multi_i16_3_g0(int n, const sg::JobMultiI16 *job, const sg::TapsMulti *taps, unsigned grid, void *stream);
int sg1d_launch_multi_i16_3_g1(int n, const sg::JobMultiI16 *job, const sg::TapsMulti *taps, unsigned grid, void *stream);
int sg1d_launch_multi_i16_3_g2(int n, const sg::JobMultiI16 *job, const sg::TapsMulti *taps, unsigned grid, void *stream);
int sg1d_launch_multi_i16_3_g3(int n, const sg::JobMultiI16 *job, const sg::TapsMulti *taps, unsigned grid, void *stream);

// The ONE entry point the host route calls (sg_k1d_multi_i16_launch.cpp dispatches to the eight objects above): k = 2 or 3 outputs; 0 when enqueued,
// -1 with the error text set otherwise.  WEAK: csrc/sg_api_1d.cpp is also linked without the kernel objects (the CPU launch record), where the
// symbol stays null and the call refuses with "object not linked" (DESIGN 4.1d).
int sg1d_launch_multi_i16(int n, int k, const sg::JobMultiI16 *job, const sg::TapsMulti *taps, unsigned grid, void *stream) __attribute__((weak));
}
