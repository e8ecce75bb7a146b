// sg_k1d_h16_host.hpp -- what the host side needs to know about the 16-bit-storage 1-D kernels (sg_k1d_h16.hpp; savgol_apply[_valid]_batch_h16):
// the by-value job and the launchers exported by their objects.  A header of its own, so that nothing the existing kernel objects are built from
// changes with it.  No device code in here.
#pragma once

#include "sg_k1d_host.hpp"

namespace sg {

// storage types of a device buffer: the values of SAVGOL_HIP_F32 / _F16 / _BF16 (include/savgol_hip.h)
enum : unsigned { STORE_F32 = 0, STORE_F16 = 1, STORE_BF16 = 2 };

// `base` is the fp32 narrow-tile job of the widened input, field for field (out of place: no stash, no phases).  in_ld / out_ld / out_shift count
// elements of their own buffer's type; JOB_VEC_IN / JOB_VEC_OUT mean "every group of FOUR elements the tile kernels move as one vector is naturally
// aligned": 8 bytes for 16-bit rows, 16 bytes for fp32 output rows.  The types are wave-uniform: a scalar branch at staging and at the store.
struct JobH16 {
    Job1D    base;
    unsigned in_type;                   // STORE_F16 or STORE_BF16
    unsigned out_type;                  // the input's type, or STORE_F32
};

}  // namespace sg

extern "C" {
// the plain three-chain kernel, one object per half-window group (the groups of the fp32 kernels, see the Makefile); 1 if this group owns n
int sg1d_launch_h16_g0(int n, const sg::JobH16 *job, const sg::Taps *taps, unsigned grid, void *stream);
int sg1d_launch_h16_g1(int n, const sg::JobH16 *job, const sg::Taps *taps, unsigned grid, void *stream);
int sg1d_launch_h16_g2(int n, const sg::JobH16 *job, const sg::Taps *taps, unsigned grid, void *stream);
int sg1d_launch_h16_g3(int n, const sg::JobH16 *job, const sg::Taps *taps, unsigned grid, void *stream);
// the half-lane block-moment kernel (half windows 20..32), one object per moment count; 0 when enqueued
int sg1d_launch_h16_momenth_t3(int n, const sg::JobH16 *job, const float *d_table, unsigned grid, void *stream);
int sg1d_launch_h16_momenth_t5(int n, const sg::JobH16 *job, const float *d_table, unsigned grid, void *stream);
int sg1d_launch_h16_momenth_t7(int n, const sg::JobH16 *job, const float *d_table, unsigned grid, void *stream);
}

namespace sg {

inline int launch_h16(int n, const JobH16 &job, const Taps &taps, unsigned grid, hipStream_t st)
{
    const int hit = sg1d_launch_h16_g0(n, &job, &taps, grid, st) || sg1d_launch_h16_g1(n, &job, &taps, grid, st) ||
                    sg1d_launch_h16_g2(n, &job, &taps, grid, st) || sg1d_launch_h16_g3(n, &job, &taps, grid, st);
    if (!hit) { sg_set_error("no 16-bit-storage kernel for half_window %d", n); return -1; }
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) { sg_set_error("16-bit-storage kernel launch failed: %s", hipGetErrorString(e)); return -1; }
    return 0;
}

}  // namespace sg
