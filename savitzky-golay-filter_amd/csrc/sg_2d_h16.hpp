// sg_2d_h16.hpp -- the 2-D batch call on 16-bit storage (savgol2d_apply_batch_h16): what sg_2d.hip (the call), sg_2d_roll.hip's 16-bit build (the
// additive tile on 16-bit rows) and sg_2d_h16.hip (the staged route's two small kernels) share.  The route rule itself is plain C++: sg_2d_h16_host.hpp.
#pragma once

#include <hip/hip_runtime.h>

#include <cstddef>

#include "sg_2d_h16_host.hpp"

namespace sg {

// The 16-bit tile's own job, beside an untouched Job2D: the fields roll_item reads under the same names, the storage types as wave-uniform flags.
struct Job2DH16 {
    const unsigned short *in;           // fp16 or bf16 rows
    unsigned char        *out;          // rows of the output's type; offsets are computed in bytes
    int rows, cols, in_stride, out_stride;      // strides and pitches in elements of their own buffer's type
    long long in_pitch, out_pitch;
    int nx, ny;
    int boundary;
    int in_bf;                          // input rows: 1 = bf16, 0 = fp16
    int out_bf;                         // 16-bit output rows: 1 = bf16, 0 = fp16
    int out_f32;                        // 1 = fp32 output rows (out_bf unused)
};

// sg_2d_roll.hip built with SG_ROLL_H16 (Makefile, ROLL_H16_RULE), one object per half-window group of the fp32 rolling kernels.
// job != NULL: launch sg2d_rolling_h16_kernel<N, TR> on `images` frames: 0 = launched, 1 = not covered (another group's half window, factors that
// are not the additive form, a half window without an additive tile, SAVGOL_HIP_ROLL_TILE=0: nothing has been enqueued), -1 = error.
// job == NULL: the PREDICATE of the route rule -- 0 when the fp32 call takes launch_roll_kernel<N, 2, 1, true, false, TR> with TR > 0 for these
// factors (fill_box_taps accepts them, the half window has an additive tile, tiles are on), else 1.  Nothing is launched.
int sg2d_launch_rolling_h16_g0(int n, int terms, const Job2DH16 *job, const float *factors, float scale, unsigned images, hipStream_t st);
int sg2d_launch_rolling_h16_g1(int n, int terms, const Job2DH16 *job, const float *factors, float scale, unsigned images, hipStream_t st);
int sg2d_launch_rolling_h16_g2(int n, int terms, const Job2DH16 *job, const float *factors, float scale, unsigned images, hipStream_t st);
int sg2d_launch_rolling_h16_g3(int n, int terms, const Job2DH16 *job, const float *factors, float scale, unsigned images, hipStream_t st);
int sg2d_launch_rolling_h16_g4(int n, int terms, const Job2DH16 *job, const float *factors, float scale, unsigned images, hipStream_t st);
int sg2d_launch_rolling_h16_g5(int n, int terms, const Job2DH16 *job, const float *factors, float scale, unsigned images, hipStream_t st);
int sg2d_launch_rolling_h16_g6(int n, int terms, const Job2DH16 *job, const float *factors, float scale, unsigned images, hipStream_t st);
inline int sg2d_launch_rolling_h16(int n, int terms, const Job2DH16 *job, const float *factors, float scale, unsigned images, hipStream_t st)
{
    static constexpr decltype(&sg2d_launch_rolling_h16_g0) groups[] = {sg2d_launch_rolling_h16_g0, sg2d_launch_rolling_h16_g1, sg2d_launch_rolling_h16_g2,
                                                                        sg2d_launch_rolling_h16_g3, sg2d_launch_rolling_h16_g4, sg2d_launch_rolling_h16_g5,
                                                                        sg2d_launch_rolling_h16_g6};
    for (auto group : groups) {
        const int rc = group(n, terms, job, factors, scale, images, st);
        if (rc != 1) return rc;
    }
    return 1;
}

// sg_2d_h16.hip: the staged route's two kernels.  `frames` frames of rows x cols; the fp32 side is library scratch: 16-byte aligned, row stride
// FrameStage::stride (cols rounded up to 4), frames back to back.
// 16-bit frames (any base, stride, pitch) -> scratch, widened exactly; the pad columns cols .. stride - 1 are zeroed (nothing reads them)
void sg2d_h16_widen_frames(const unsigned short *in, int in_stride, long long in_pitch, bool bf, float *scratch, int rows, int cols, size_t frames, hipStream_t st);
// scratch -> frames of out_type (SAVGOL_HIP_F16 / _BF16 / _F32), rounded once to nearest even (fp32: copied): rows [ylo, yhi) x columns [xlo, xhi)
// only -- the pixels the fp32 call writes; nothing else of the output stack is touched
void sg2d_h16_round_frames(const float *scratch, void *out, int out_type, int out_stride, long long out_pitch, int rows, int cols, int xlo, int xhi,
                           int ylo, int yhi, size_t frames, hipStream_t st);

}  // namespace sg
