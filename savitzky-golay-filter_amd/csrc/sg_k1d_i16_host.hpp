// sg_k1d_i16_host.hpp -- what the host side needs to know about the int16-storage 1-D kernels (sg_k1d_i16.hpp; savgol_apply[_valid]_batch_i16):
// the by-value job and the launchers exported by their objects.  A header of its own, as JobH16 has one, so that nothing the existing kernel
// objects are built from changes with it.  No device code in here.
#pragma once

#include "sg_k1d_host.hpp"

namespace sg {

// storage types of the int16 call's output: the values of SAVGOL_HIP_F32 / SAVGOL_HIP_I16 (include/savgol_hip.h)
enum : unsigned { STORE_I16_F32 = 0, STORE_I16 = 3 };

// `base` is the fp32 narrow-tile job of the widened input, field for field (out of place: no stash, no phases).  in_ld / out_ld / out_shift count
// elements of their own buffer's type; JOB_VEC_IN / JOB_VEC_OUT mean "every group of FOUR elements the tile kernels move as one vector is naturally
// aligned": 8 bytes for int16 rows, 16 bytes for fp32 output rows.  The output type is wave-uniform: a scalar branch at the store.
struct JobI16 {
    Job1D    base;
    unsigned out_type;                  // STORE_I16 or STORE_I16_F32
};

}  // namespace sg

extern "C" {
// the plain three-chain kernel, one object per half-window group (the groups of the fp32 kernels, see the Makefile); 1 if this group owns n
int sg1d_launch_i16_g0(int n, const sg::JobI16 *job, const sg::Taps *taps, unsigned grid, void *stream);
int sg1d_launch_i16_g1(int n, const sg::JobI16 *job, const sg::Taps *taps, unsigned grid, void *stream);
int sg1d_launch_i16_g2(int n, const sg::JobI16 *job, const sg::Taps *taps, unsigned grid, void *stream);
int sg1d_launch_i16_g3(int n, const sg::JobI16 *job, const sg::Taps *taps, unsigned grid, void *stream);
// the half-lane block-moment kernel (half windows 20..32), one object per moment count; 0 when enqueued
int sg1d_launch_i16_momenth_t3(int n, const sg::JobI16 *job, const float *d_table, unsigned grid, void *stream);
int sg1d_launch_i16_momenth_t5(int n, const sg::JobI16 *job, const float *d_table, unsigned grid, void *stream);
int sg1d_launch_i16_momenth_t7(int n, const sg::JobI16 *job, const float *d_table, unsigned grid, void *stream);

// The ONE entry point the host route calls (sg_k1d_i16_launch.cpp dispatches to the seven objects above): moment_terms = 0 takes the plain kernel
// with `taps`, 3 / 5 / 7 the block-moment kernel with `d_table`; 0 when enqueued, -1 with the error text set otherwise.  WEAK: csrc/sg_api_1d.cpp
// is also linked without the kernel objects (the CPU launch record), where the symbol stays null and the call refuses with "object not linked".
int sg1d_launch_i16(int n, int moment_terms, const sg::JobI16 *job, const sg::Taps *taps, const float *d_table, unsigned grid, void *stream) __attribute__((weak));
}
