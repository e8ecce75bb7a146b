// sg_2d_i16.hip -- the STAGED route of savgol2d_apply_batch_i16 (sg_2d.hip): frames of int16 rows widened into aligned fp32 scratch, and the
// pixels the fp32 call wrote converted out.  After sg2d_h16_widen_kernel / sg2d_h16_round_kernel (sg_2d_h16.hip): four elements per thread, one
// vector where the caller's quad is naturally aligned, element by element otherwise -- any base, stride and pitch.  Conversions: sg_i16.hpp only.
// The scratch side is the library's: 16-byte aligned, `stride` (a multiple of 4) floats per row, frames back to back.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "savgol_hip.h"
#include "sg_2d_i16.hpp"
#include "sg_i16.hpp"
#include "sg_pk.hpp"

namespace sg {

// thread -> (frame, row, first column of its quad): quads of a row fastest
struct QuadAtI16 { size_t frame; int row, col; };
__device__ __forceinline__ bool quad_at_i16(int rows, int stride, size_t frames, QuadAtI16 &at)
{
    const size_t q = (size_t)blockIdx.x * blockDim.x + threadIdx.x, per_row = (size_t)(stride / 4);
    const size_t r = q / per_row;
    at.col = (int)(q - r * per_row) * 4;
    at.frame = r / (size_t)rows;
    at.row = (int)(r - at.frame * (size_t)rows);
    return at.frame < frames;
}

// vec: the caller's quads are naturally aligned (8-byte base, stride and pitch multiples of 4)
__global__ __launch_bounds__(256) void sg2d_i16_widen_kernel(const short *__restrict__ in, int in_stride, long long in_pitch, float *__restrict__ scratch, int rows, int cols,
                                                             int stride, size_t frames, int vec)
{
    QuadAtI16 at;
    if (!quad_at_i16(rows, stride, frames, at)) return;
    const short *src = in + (long long)at.frame * in_pitch + (long long)at.row * in_stride + at.col;
    float *dst = scratch + (at.frame * (size_t)rows + (size_t)at.row) * (size_t)stride + at.col;
    if (vec && at.col + 4 <= cols) {
        const float4 w = widen4_i16(*reinterpret_cast<const u32x2 *>(src));
        *reinterpret_cast<f32x4 *>(dst) = f32x4{w.x, w.y, w.z, w.w};
        return;
    }
    auto one = [](short e) { return widen2_i16((unsigned)(unsigned short)e).x; };      // sg_i16.hpp's widening of a dword, its low element
    f32x4 v = f32x4{0.0f, 0.0f, 0.0f, 0.0f};                 // columns past the frame: scratch pad, zeroed
    if (at.col < cols) v.x = one(src[0]);
    if (at.col + 1 < cols) v.y = one(src[1]);
    if (at.col + 2 < cols) v.z = one(src[2]);
    if (at.col + 3 < cols) v.w = one(src[3]);
    *reinterpret_cast<f32x4 *>(dst) = v;
}

// rows [ylo, yhi) x columns [xlo, xhi) only.  vec: the caller's quads are naturally aligned (int16 output: 8-byte base; fp32 output: 16-byte base;
// stride and pitch multiples of 4)
__global__ __launch_bounds__(256) void sg2d_i16_convert_kernel(const float *__restrict__ scratch, void *__restrict__ out, int out_f32, int out_stride, long long out_pitch,
                                                               int rows, int stride, int xlo, int xhi, int ylo, int yhi, size_t frames, int vec)
{
    QuadAtI16 at;
    if (!quad_at_i16(rows, stride, frames, at)) return;
    if (at.row < ylo || at.row >= yhi || at.col + 4 <= xlo || at.col >= xhi) return;
    const f32x4 v = *reinterpret_cast<const f32x4 *>(scratch + (at.frame * (size_t)rows + (size_t)at.row) * (size_t)stride + at.col);
    const long long first = (long long)at.frame * out_pitch + (long long)at.row * out_stride + at.col;
    const bool whole = vec && at.col >= xlo && at.col + 4 <= xhi;
    const float e[4] = {v.x, v.y, v.z, v.w};
    if (out_f32) {
        float *o = static_cast<float *>(out) + first;
        if (whole) { *reinterpret_cast<f32x4 *>(o) = v; return; }
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (at.col + j >= xlo && at.col + j < xhi) o[j] = e[j];
        return;
    }
    short *o = static_cast<short *>(out) + first;
    if (whole) { *reinterpret_cast<u32x2 *>(o) = narrow4_i16(float4{v.x, v.y, v.z, v.w}); return; }
#pragma unroll
    for (int j = 0; j < 4; ++j)
        if (at.col + j >= xlo && at.col + j < xhi) o[j] = narrow1_i16(e[j]);
}

static unsigned quad_blocks_i16(int rows, int stride, size_t frames)
{
    const size_t quads = frames * (size_t)rows * (size_t)(stride / 4);
    return (unsigned)((quads + 255) / 256);
}

void sg2d_i16_widen_frames(const short *in, int in_stride, long long in_pitch, float *scratch, int rows, int cols, size_t frames, hipStream_t st)
{
    const int stride = (cols + 3) & ~3;
    const int vec = (reinterpret_cast<uintptr_t>(in) & 7u) == 0 && in_stride % 4 == 0 && in_pitch % 4 == 0;
    hipLaunchKernelGGL(sg2d_i16_widen_kernel, dim3(quad_blocks_i16(rows, stride, frames)), dim3(256), 0, st, in, in_stride, in_pitch, scratch, rows, cols, stride, frames, vec);
}

void sg2d_i16_convert_frames(const float *scratch, void *out, int out_type, int out_stride, long long out_pitch, int rows, int cols, int xlo, int xhi, int ylo, int yhi,
                             size_t frames, hipStream_t st)
{
    const int stride = (cols + 3) & ~3;
    const int f32 = out_type == SAVGOL_HIP_F32;
    const int vec = (reinterpret_cast<uintptr_t>(out) & (f32 ? 15u : 7u)) == 0 && out_stride % 4 == 0 && out_pitch % 4 == 0;
    hipLaunchKernelGGL(sg2d_i16_convert_kernel, dim3(quad_blocks_i16(rows, stride, frames)), dim3(256), 0, st, scratch, out, f32, out_stride, out_pitch, rows, stride, xlo,
                       xhi, ylo, yhi, frames, vec);
}

}  // namespace sg
