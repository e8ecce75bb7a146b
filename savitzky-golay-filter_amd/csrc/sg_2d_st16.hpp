// sg_2d_st16.hpp -- the 2-D batch call on 16-bit STORAGE, fp32 arithmetic inside, for two storage families:
//   h16  fp16 or bf16 frames in, the same type or fp32 out   (savgol2d_apply_batch_h16)
//   i16  int16 frames in, int16 or fp32 out                   (savgol2d_apply_batch_i16)
// What sg_2d.hip (the calls), sg_2d_roll.hip's two 16-bit builds (the additive tile, sg_2d_roll_st16.inc) and sg_2d_st16.hip (the staged route's small
// kernels) share.  The route rule is plain C++ and one for both (the element sizes are the same): frame_plan_h16 / frame_stage_h16 of sg_2d_h16_host.hpp.
//
// ONE tile text (sg_2d_roll_st16_tile.inc), ONE launcher, ONE staged widen body and ONE pair of staged launchers serve both; what the families differ in
// is their policy (H16Family2D, I16Family2D -- the 2-D counterparts of sg_k1d_st16.hpp's H16Family / I16Family, under names of their own because both
// sets live in namespace sg):
//   Elem, Out          the rows' element type; what the job's output pointer points at (h16: bytes, offsets are computed in bytes; i16: void, cast to
//                      the kernel's own output type)
//   Fields             the family's block of the job (Job2DSt16::st): h16 carries the storage types as wave-uniform flags, one kernel per half window
//                      serves all four type pairs; i16 has ONE input type and its output type is a template argument of the kernel (TYPED_OUT), so
//                      out_f32 only picks the instance on the host
//   TWO_WAVES_FROM     the first half window (up to 9) whose tile is built for two waves per SIMD instead of the fp32 tile's three (sg_2d_roll_st16.inc)
//   image_out          the output rows of frame `img` of a launch
//   widen_quad / widen_one    the staged widen kernels' converts (sg_h16.hpp with a bf flag; sg_i16.hpp)
#pragma once

#include <hip/hip_runtime.h>

#include <cstddef>

#include "sg_2d_h16_host.hpp"
#include "sg_h16.hpp"
#include "sg_i16.hpp"
#include "sg_pk.hpp"

namespace sg {

// The 16-bit tile's own job, beside an untouched Job2D: the fields roll_item reads under the same names, then the family's block.
template <class F>
struct Job2DSt16 {
    const typename F::Elem *in;         // 16-bit rows
    typename F::Out        *out;        // rows of the output's type
    int rows, cols, in_stride, out_stride;      // strides and pitches in elements of their own buffer's type
    long long in_pitch, out_pitch;
    int nx, ny;
    int boundary;
    typename F::Fields st;
};

struct H16Family2D {
    typedef unsigned short Elem;
    typedef unsigned char Out;
    struct Fields {
        int in_bf;                      // input rows: 1 = bf16, 0 = fp16
        int out_bf;                     // 16-bit output rows: 1 = bf16, 0 = fp16
        int out_f32;                    // 1 = fp32 output rows (out_bf unused)
    };
    static constexpr bool TYPED_OUT = false;
    static constexpr int TWO_WAVES_FROM = 7;
    template <class TOUT>
    static __device__ __forceinline__ TOUT *image_out(const Job2DSt16<H16Family2D> &job, unsigned img) { return job.out + (long long)img * job.out_pitch * (job.st.out_f32 ? 4 : 2); }
    static __device__ __forceinline__ f32x4 widen_quad(const u32x2 raw, bool bf)
    {
        const f32x2 a = widen2(raw.x, bf), b = widen2(raw.y, bf);
        return f32x4{a.x, a.y, b.x, b.y};
    }
    static __device__ __forceinline__ float widen_one(Elem e, bool bf) { return widen1(e, bf); }
};

struct I16Family2D {
    typedef short Elem;
    typedef void Out;
    struct Fields {
        int out_f32;                    // host side: 1 = sg2d_rolling_i16_kernel<N, TR, true>, 0 = <N, TR, false>
    };
    static constexpr bool TYPED_OUT = true;
    static constexpr int TWO_WAVES_FROM = 9;
    template <class TOUT>
    static __device__ __forceinline__ TOUT *image_out(const Job2DSt16<I16Family2D> &job, unsigned img) { return static_cast<TOUT *>(job.out) + (long long)img * job.out_pitch; }
    static __device__ __forceinline__ f32x4 widen_quad(const u32x2 raw, bool)
    {
        const float4 w = widen4_i16(raw);
        return f32x4{w.x, w.y, w.z, w.w};
    }
    static __device__ __forceinline__ float widen_one(Elem e, bool) { return widen2_i16((unsigned)(unsigned short)e).x; }     // sg_i16.hpp's widening of a dword, its low element
};

typedef Job2DSt16<H16Family2D> Job2DH16;
typedef Job2DSt16<I16Family2D> Job2DI16;
static_assert(sizeof(Job2DH16) == 72 && offsetof(Job2DH16, st) == 60 && sizeof(Job2DI16) == 64 && offsetof(Job2DI16, st) == 60 && offsetof(Job2DI16, boundary) == 56,
              "the kernarg layouts: the family's block follows `boundary` directly");

// sg_2d_roll.hip built with SG_ROLL_H16 / SG_ROLL_I16 (Makefile, ROLL_ST16_RULE), one object per family and half-window group of the fp32 rolling
// kernels.  job != NULL: launch the family's tile (sg2d_rolling_h16_kernel<N, TR>, sg2d_rolling_i16_kernel<N, TR, OUT_F32>) on `images` frames:
// 0 = launched, 1 = not covered (another group's half window, factors that are not the additive form, a half window without an additive tile,
// SAVGOL_HIP_ROLL_TILE=0: nothing has been enqueued), -1 = error.  job == NULL: the same answer with nothing launched (roll16_fp32_takes_tiles below).
template <class F>
using RollSt16Launch = int(int n, int terms, const Job2DSt16<F> *job, const float *factors, float scale, unsigned images, hipStream_t st);
#define SG2D_ROLL_ST16_GROUPS(f) sg2d_launch_rolling_##f##_g0, sg2d_launch_rolling_##f##_g1, sg2d_launch_rolling_##f##_g2, sg2d_launch_rolling_##f##_g3, \
                                 sg2d_launch_rolling_##f##_g4, sg2d_launch_rolling_##f##_g5, sg2d_launch_rolling_##f##_g6
RollSt16Launch<H16Family2D> SG2D_ROLL_ST16_GROUPS(h16);
RollSt16Launch<I16Family2D> SG2D_ROLL_ST16_GROUPS(i16);
template <class F> struct RollSt16Groups;           // (a class's static member, not a variable template: that one is emitted into the device code too)
template <> struct RollSt16Groups<H16Family2D> { static constexpr RollSt16Launch<H16Family2D> *ALL[] = {SG2D_ROLL_ST16_GROUPS(h16)}; };
template <> struct RollSt16Groups<I16Family2D> { static constexpr RollSt16Launch<I16Family2D> *ALL[] = {SG2D_ROLL_ST16_GROUPS(i16)}; };
template <class F>
inline int sg2d_launch_rolling_st16(int n, int terms, const Job2DSt16<F> *job, const float *factors, float scale, unsigned images, hipStream_t st)
{
    for (auto group : RollSt16Groups<F>::ALL) {
        const int rc = group(n, terms, job, factors, scale, images, st);
        if (rc != 1) return rc;
    }
    return 1;
}
// The PREDICATE of the route rule: does the fp32 call take launch_roll_kernel<N, 2, 1, true, false, TR> with TR > 0 for these factors (fill_box_taps
// accepts them, the half window has an additive tile, tiles are on)?  A question about the fp32 call, so one for both families: the h16 objects answer
// it (every 16-bit build of sg_2d_roll.hip holds the same fill_box_taps and roll_tile_rows); nothing is launched.
inline bool roll16_fp32_takes_tiles(int n, int terms, const float *factors, float scale)
{
    return sg2d_launch_rolling_st16<H16Family2D>(n, terms, nullptr, factors, scale, 0, nullptr) == 0;
}

// ---- savgol2d_gradient_batch_i16's DIRECT route (sg_2d_grad16_host.hpp): the two kernels the fp32 gradient runs on a square window up to n = 7, on int16 rows.
// Each launcher: 0 = launched, 1 = not covered (another group's half window, factors the fp32 launcher would not take this way, SAVGOL_HIP_ROLL_TILE=0:
// nothing has been enqueued), -1 = error.  The caller has checked frame_plan_h16's layout conditions.
// gy -- sg_2d_roll.hip built with SG_ROLL_I16_GEN (Makefile, ROLL_GEN16_RULE): sg2d_rolling_gen_i16_kernel<N, NT, OUT_F32>, the general one- and two-term
// 20-row tile with the taps of the fp32 launcher's own fill_taps.  job == NULL: the same answer with nothing launched (the route rule's gy_direct).
using RollGen16Launch = int(int n, int terms, const Job2DI16 *job, const float *factors, float scale, unsigned images, hipStream_t st);
RollGen16Launch sg2d_launch_rolling_gen_i16_g0, sg2d_launch_rolling_gen_i16_g1, sg2d_launch_rolling_gen_i16_g2, sg2d_launch_rolling_gen_i16_g3;
inline int sg2d_launch_rolling_gen_i16(int n, int terms, const Job2DI16 *job, const float *factors, float scale, unsigned images, hipStream_t st)
{
    static constexpr RollGen16Launch *groups[] = {sg2d_launch_rolling_gen_i16_g0, sg2d_launch_rolling_gen_i16_g1, sg2d_launch_rolling_gen_i16_g2, sg2d_launch_rolling_gen_i16_g3};
    for (auto group : groups) {
        const int rc = group(n, terms, job, factors, scale, images, st);
        if (rc != 1) return rc;
    }
    return 1;
}
// gx -- sg_2d_hf.hip built with SG_HF_I16 (Makefile, HF_I16_RULE): sg2d_rolling_hf_i16_kernel<N, NT, OUT_F32>, one term or two of one x parity in ONE
// launch, never accumulating; sigma / sigma2 as for sg2d_launch_rolling_hf (sg_2d.hpp).
using HfI16Launch = int(int n, const Job2DI16 &job, const float *factors, float scale, float sigma, const float *factors2, float sigma2, unsigned images, int cu_count, hipStream_t st);
HfI16Launch sg2d_launch_rolling_hf_i16_g0, sg2d_launch_rolling_hf_i16_g1, sg2d_launch_rolling_hf_i16_g2, sg2d_launch_rolling_hf_i16_g3;
inline int sg2d_launch_rolling_hf_i16(int n, const Job2DI16 &job, const float *factors, float scale, float sigma, const float *factors2, float sigma2, unsigned images,
                                      int cu_count, hipStream_t st)
{
    static constexpr HfI16Launch *groups[] = {sg2d_launch_rolling_hf_i16_g0, sg2d_launch_rolling_hf_i16_g1, sg2d_launch_rolling_hf_i16_g2, sg2d_launch_rolling_hf_i16_g3};
    for (auto group : groups) {
        const int rc = group(n, job, factors, scale, sigma, factors2, sigma2, images, cu_count, st);
        if (rc != 1) return rc;
    }
    return 1;
}

// sg_2d_st16.hip: the staged route's two launchers, instantiated for both families.  `frames` frames of rows x cols; the fp32 side is library scratch:
// 16-byte aligned, row stride FrameStageH16::stride (cols rounded up to 4), frames back to back.
// 16-bit frames of in_type (any base, stride, pitch) -> scratch, widened exactly; the pad columns cols .. stride - 1 are zeroed (nothing reads them)
template <class F>
void sg2d_st16_widen_frames(const typename F::Elem *in, int in_type, int in_stride, long long in_pitch, float *scratch, int rows, int cols, size_t frames, hipStream_t st);
// scratch -> frames of out_type (h16: SAVGOL_HIP_F16 / _BF16, rounded once to nearest even; i16: SAVGOL_HIP_I16, converted once by sg_i16.hpp's rule;
// SAVGOL_HIP_F32: copied): rows [ylo, yhi) x columns [xlo, xhi) only -- the pixels the fp32 call writes; nothing else of the output stack is touched
template <class F>
void sg2d_st16_out_frames(const float *scratch, void *out, int out_type, int out_stride, long long out_pitch, int rows, int cols, int xlo, int xhi, int ylo, int yhi,
                          size_t frames, hipStream_t st);

}  // namespace sg
