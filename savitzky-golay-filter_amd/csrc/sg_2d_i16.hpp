// sg_2d_i16.hpp -- the 2-D batch call on int16 storage (savgol2d_apply_batch_i16): what sg_2d.hip (the call), sg_2d_roll.hip's int16 build (the
// additive tile on int16 rows, sg_2d_roll_i16.inc) and sg_2d_i16.hip (the staged route's two small kernels) share.  The route rule is the 16-bit
// float call's, unchanged: frame_plan_h16 / frame_stage_h16 of sg_2d_h16_host.hpp (the element sizes are the same).
#pragma once

#include <hip/hip_runtime.h>

#include <cstddef>

#include "sg_2d_h16_host.hpp"

namespace sg {

// The int16 tile's own job, beside an untouched Job2D: the fields roll_item reads under the same names.  The storage types are NOT here: the input is
// int16, the output's type is a template argument of the kernel (out_f32 only picks the instance on the host).
struct Job2DI16 {
    const short *in;                    // int16 rows
    void        *out;                   // int16 or fp32 rows
    int rows, cols, in_stride, out_stride;      // strides and pitches in elements of their own buffer's type
    long long in_pitch, out_pitch;
    int nx, ny;
    int boundary;
    int out_f32;                        // host side: 1 = sg2d_rolling_i16_kernel<N, TR, true>, 0 = <N, TR, false>
};

// sg_2d_roll.hip built with SG_ROLL_I16 (Makefile, ROLL_I16_RULE), one object per half-window group of the fp32 rolling kernels.  Launches
// sg2d_rolling_i16_kernel<N, TR, OUT_F32> on `images` frames: 0 = launched, 1 = not covered (another group's half window, factors that are not the
// additive form, a half window without an additive tile, SAVGOL_HIP_ROLL_TILE=0: nothing has been enqueued), -1 = error.  The route's PREDICATE is
// sg2d_launch_rolling_h16(..., job = NULL, ...) of sg_2d_h16.hpp: both ask fill_box_taps and roll_tile_rows.
int sg2d_launch_rolling_i16_g0(int n, int terms, const Job2DI16 &job, const float *factors, float scale, unsigned images, hipStream_t st);
int sg2d_launch_rolling_i16_g1(int n, int terms, const Job2DI16 &job, const float *factors, float scale, unsigned images, hipStream_t st);
int sg2d_launch_rolling_i16_g2(int n, int terms, const Job2DI16 &job, const float *factors, float scale, unsigned images, hipStream_t st);
int sg2d_launch_rolling_i16_g3(int n, int terms, const Job2DI16 &job, const float *factors, float scale, unsigned images, hipStream_t st);
int sg2d_launch_rolling_i16_g4(int n, int terms, const Job2DI16 &job, const float *factors, float scale, unsigned images, hipStream_t st);
int sg2d_launch_rolling_i16_g5(int n, int terms, const Job2DI16 &job, const float *factors, float scale, unsigned images, hipStream_t st);
int sg2d_launch_rolling_i16_g6(int n, int terms, const Job2DI16 &job, const float *factors, float scale, unsigned images, hipStream_t st);
inline int sg2d_launch_rolling_i16(int n, int terms, const Job2DI16 &job, const float *factors, float scale, unsigned images, hipStream_t st)
{
    static constexpr decltype(&sg2d_launch_rolling_i16_g0) groups[] = {sg2d_launch_rolling_i16_g0, sg2d_launch_rolling_i16_g1, sg2d_launch_rolling_i16_g2,
                                                                        sg2d_launch_rolling_i16_g3, sg2d_launch_rolling_i16_g4, sg2d_launch_rolling_i16_g5,
                                                                        sg2d_launch_rolling_i16_g6};
    for (auto group : groups) {
        const int rc = group(n, terms, job, factors, scale, images, st);
        if (rc != 1) return rc;
    }
    return 1;
}

// sg_2d_i16.hip: the staged route's two kernels.  `frames` frames of rows x cols; the fp32 side is library scratch: 16-byte aligned, row stride
// FrameStageH16::stride (cols rounded up to 4), frames back to back.
// int16 frames (any base, stride, pitch) -> scratch, widened exactly; the pad columns cols .. stride - 1 are zeroed (nothing reads them)
void sg2d_i16_widen_frames(const short *in, int in_stride, long long in_pitch, float *scratch, int rows, int cols, size_t frames, hipStream_t st);
// scratch -> frames of out_type (SAVGOL_HIP_I16: converted once by sg_i16.hpp's rule; SAVGOL_HIP_F32: copied): rows [ylo, yhi) x columns [xlo, xhi)
// only -- the pixels the fp32 call writes; nothing else of the output stack is touched
void sg2d_i16_convert_frames(const float *scratch, void *out, int out_type, int out_stride, long long out_pitch, int rows, int cols, int xlo, int xhi,
                             int ylo, int yhi, size_t frames, hipStream_t st);

}  // namespace sg
