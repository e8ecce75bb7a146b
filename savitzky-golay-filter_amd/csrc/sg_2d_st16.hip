// sg_2d_st16.hip -- the STAGED route of savgol2d_apply_batch_h16 and savgol2d_apply_batch_i16 (sg_2d.hip): frames of 16-bit rows widened into aligned
// fp32 scratch, and the pixels the fp32 call wrote rounded / converted out.  After sg_h16_widen_kernel / sg_h16_round_kernel of the stream path
// (sg_stream.hip): four elements per thread, one vector where the caller's quad is naturally aligned, element by element otherwise -- any base, stride
// and pitch.  One widen body for both storage families, with the family's converts (sg_2d_st16.hpp: sg_h16.hpp with a bf flag, sg_i16.hpp).
// The scratch side is the library's: 16-byte aligned, `stride` (a multiple of 4) floats per row, frames back to back.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <type_traits>

#include "savgol_hip.h"
#include "sg_2d_st16.hpp"

namespace sg {

// thread -> (frame, row, first column of its quad): quads of a row fastest
struct QuadAt { size_t frame; int row, col; };
__device__ __forceinline__ bool quad_at(int rows, int stride, size_t frames, QuadAt &at)
{
    const size_t q = (size_t)blockIdx.x * blockDim.x + threadIdx.x, per_row = (size_t)(stride / 4);
    const size_t r = q / per_row;
    at.col = (int)(q - r * per_row) * 4;
    at.frame = r / (size_t)rows;
    at.row = (int)(r - at.frame * (size_t)rows);
    return at.frame < frames;
}

template <class F>
__device__ __forceinline__ void widen_quads(const typename F::Elem *in, int in_stride, long long in_pitch, int bf, float *scratch, int rows, int cols, int stride,
                                            size_t frames, int vec)
{
    QuadAt at;
    if (!quad_at(rows, stride, frames, at)) return;
    const typename F::Elem *src = in + (long long)at.frame * in_pitch + (long long)at.row * in_stride + at.col;
    float *dst = scratch + (at.frame * (size_t)rows + (size_t)at.row) * (size_t)stride + at.col;
    if (vec && at.col + 4 <= cols) {
        *reinterpret_cast<f32x4 *>(dst) = F::widen_quad(*reinterpret_cast<const u32x2 *>(src), bf != 0);
        return;
    }
    f32x4 v = f32x4{0.0f, 0.0f, 0.0f, 0.0f};                 // columns past the frame: scratch pad, zeroed
    if (at.col < cols) v.x = F::widen_one(src[0], bf != 0);
    if (at.col + 1 < cols) v.y = F::widen_one(src[1], bf != 0);
    if (at.col + 2 < cols) v.z = F::widen_one(src[2], bf != 0);
    if (at.col + 3 < cols) v.w = F::widen_one(src[3], bf != 0);
    *reinterpret_cast<f32x4 *>(dst) = v;
}

// vec: the caller's quads are naturally aligned (8-byte base, stride and pitch multiples of 4)
__global__ __launch_bounds__(256) void sg2d_h16_widen_kernel(const unsigned short *__restrict__ in, int in_stride, long long in_pitch, int bf, float *__restrict__ scratch,
                                                             int rows, int cols, int stride, size_t frames, int vec)
{
    widen_quads<H16Family2D>(in, in_stride, in_pitch, bf, scratch, rows, cols, stride, frames, vec);
}
__global__ __launch_bounds__(256) void sg2d_i16_widen_kernel(const short *__restrict__ in, int in_stride, long long in_pitch, float *__restrict__ scratch, int rows, int cols,
                                                             int stride, size_t frames, int vec)
{
    widen_quads<I16Family2D>(in, in_stride, in_pitch, 0, scratch, rows, cols, stride, frames, vec);
}

// The two round-out kernels keep a text each: one body for both (the family's narrowing converts behind the fp32 branch) compiled to the same
// instructions with two operands of one s_and_b64 swapped, and a fold is kept only where the instructions stay what they were.
// rows [ylo, yhi) x columns [xlo, xhi) only.  vec: the caller's quads are naturally aligned (16-bit output: 8-byte base; fp32 output: 16-byte base;
// stride and pitch multiples of 4)
__global__ __launch_bounds__(256) void sg2d_h16_round_kernel(const float *__restrict__ scratch, void *__restrict__ out, int out_type, int out_stride, long long out_pitch,
                                                             int rows, int stride, int xlo, int xhi, int ylo, int yhi, size_t frames, int vec)
{
    QuadAt at;
    if (!quad_at(rows, stride, frames, at)) return;
    if (at.row < ylo || at.row >= yhi || at.col + 4 <= xlo || at.col >= xhi) return;
    const f32x4 v = *reinterpret_cast<const f32x4 *>(scratch + (at.frame * (size_t)rows + (size_t)at.row) * (size_t)stride + at.col);
    const long long first = (long long)at.frame * out_pitch + (long long)at.row * out_stride + at.col;
    const bool whole = vec && at.col >= xlo && at.col + 4 <= xhi;
    const float e[4] = {v.x, v.y, v.z, v.w};
    if (out_type == SAVGOL_HIP_F32) {
        float *o = static_cast<float *>(out) + first;
        if (whole) { *reinterpret_cast<f32x4 *>(o) = v; return; }
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (at.col + j >= xlo && at.col + j < xhi) o[j] = e[j];
        return;
    }
    const bool bf = out_type == SAVGOL_HIP_BF16;
    unsigned short *o = static_cast<unsigned short *>(out) + first;
    if (whole) { *reinterpret_cast<u32x2 *>(o) = u32x2{narrow2(f32x2{v.x, v.y}, bf), narrow2(f32x2{v.z, v.w}, bf)}; return; }
#pragma unroll
    for (int j = 0; j < 4; ++j)
        if (at.col + j >= xlo && at.col + j < xhi) o[j] = narrow1(e[j], bf);
}
__global__ __launch_bounds__(256) void sg2d_i16_convert_kernel(const float *__restrict__ scratch, void *__restrict__ out, int out_f32, int out_stride, long long out_pitch,
                                                               int rows, int stride, int xlo, int xhi, int ylo, int yhi, size_t frames, int vec)
{
    QuadAt at;
    if (!quad_at(rows, stride, frames, at)) return;
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

static unsigned quad_blocks(int rows, int stride, size_t frames)
{
    const size_t quads = frames * (size_t)rows * (size_t)(stride / 4);
    return (unsigned)((quads + 255) / 256);
}

template <class F>
void sg2d_st16_widen_frames(const typename F::Elem *in, int in_type, int in_stride, long long in_pitch, float *scratch, int rows, int cols, size_t frames, hipStream_t st)
{
    static_assert(std::is_same<F, H16Family2D>::value || std::is_same<F, I16Family2D>::value, "no staged kernels for this storage family");
    const int stride = (cols + 3) & ~3;
    const int vec = (reinterpret_cast<uintptr_t>(in) & 7u) == 0 && in_stride % 4 == 0 && in_pitch % 4 == 0;
    const dim3 grid(quad_blocks(rows, stride, frames));
    // the h16 kernel is told whether the rows are bf16; int16 rows have one type
    if constexpr (std::is_same<F, I16Family2D>::value) hipLaunchKernelGGL(sg2d_i16_widen_kernel, grid, dim3(256), 0, st, in, in_stride, in_pitch, scratch, rows, cols, stride, frames, vec);
    else hipLaunchKernelGGL(sg2d_h16_widen_kernel, grid, dim3(256), 0, st, in, in_stride, in_pitch, in_type == SAVGOL_HIP_BF16 ? 1 : 0, scratch, rows, cols, stride, frames, vec);
}

template <class F>
void sg2d_st16_out_frames(const float *scratch, void *out, int out_type, int out_stride, long long out_pitch, int rows, int cols, int xlo, int xhi, int ylo, int yhi,
                          size_t frames, hipStream_t st)
{
    const int stride = (cols + 3) & ~3;
    const int f32 = out_type == SAVGOL_HIP_F32;
    const int vec = (reinterpret_cast<uintptr_t>(out) & (f32 ? 15u : 7u)) == 0 && out_stride % 4 == 0 && out_pitch % 4 == 0;
    const dim3 grid(quad_blocks(rows, stride, frames));
    // the h16 kernel takes the output's type, the i16 kernel whether it is fp32
    if constexpr (std::is_same<F, I16Family2D>::value) hipLaunchKernelGGL(sg2d_i16_convert_kernel, grid, dim3(256), 0, st, scratch, out, f32, out_stride, out_pitch, rows, stride, xlo, xhi, ylo, yhi, frames, vec);
    else hipLaunchKernelGGL(sg2d_h16_round_kernel, grid, dim3(256), 0, st, scratch, out, out_type, out_stride, out_pitch, rows, stride, xlo, xhi, ylo, yhi, frames, vec);
}

template void sg2d_st16_widen_frames<H16Family2D>(const unsigned short *, int, int, long long, float *, int, int, size_t, hipStream_t);
template void sg2d_st16_widen_frames<I16Family2D>(const short *, int, int, long long, float *, int, int, size_t, hipStream_t);
template void sg2d_st16_out_frames<H16Family2D>(const float *, void *, int, int, long long, int, int, int, int, int, int, size_t, hipStream_t);
template void sg2d_st16_out_frames<I16Family2D>(const float *, void *, int, int, long long, int, int, int, int, int, int, size_t, hipStream_t);

}  // namespace sg
