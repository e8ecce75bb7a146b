// sg_2d_grad16_host.hpp -- host-only rule of savgol2d_gradient_batch_i16 (no device types: g++ translation units include it too): which route a call takes,
// decided before anything is enqueued, and the pieces of its staged route.  The call and savgol2d_gradient_batch_i16_route (sg_2d.hip) both ask this rule;
// tests/mock/grad_plan_i16.cpp prints it for a table of calls.
//
// The TWIN is savgol2d_gradient_batch_f32 with the same windows, order, deltas and boundary on the frames widened exactly, in 16-byte aligned fp32 buffers
// with stride = cols rounded up to 4 and pitch rows x stride.  On a square window up to n = 7 whose requested frames have one or two terms the twin runs
// the horizontal-first kernel for gx (one launch: sg2d_rolling_hf_kernel<N, false, NT>) and the general 20-row tile for gy
// (sg2d_rolling_kernel<N, NT, 1, false, false, 20>).  DIRECT: the same two kernels reading int16 rows and storing the output's type
// (sg2d_rolling_hf_i16_kernel, sg2d_rolling_gen_i16_kernel) -- BOTH requested frames, when every one of these holds:
//   square window, 1 <= n <= GRAD_I16_DIRECT_MAX_N
//   gx_direct      (gx requested) its separable factors have one or two terms, every vector of definite parity (vector_parity), the two x factors of ONE
//                  parity: what hf_dispatch needs for its one-launch forms
//   gy_direct      (gy requested) its factors have one or two terms of definite and common parities, and two terms are not the additive form: what
//                  launch_roll needs for the general tile.  Both flags are the host's answers from sep_factors_cached -- in practice poly_order <= 4
//   frame_plan_h16's layout conditions for every requested frame, asked of frame_plan_h16 itself (sg_2d_h16_host.hpp): cols % 4 == 0 and cols >= 32; the
//                  int16 sides on 8-byte bases with stride and pitch multiples of 4; an fp32 output on a 16-byte base; rows x out_stride x element size
//                  and rows x cols x 4 under the store descriptor's 0x7fffff00
//   roll_tile_switch   SAVGOL_HIP_ROLL_TILE is not 0 (at 0 the twin's own gy leaves the tiles)
//   direct_switch      SAVGOL_HIP_2D_GRAD_I16_DIRECT is not 0 (read at every call: A/B runs and tests)
// STAGED: every other call -- the twin itself: whole frames in pieces widened ONCE into aligned fp32 scratch, the fp32 gradient scratch to scratch for the
// requested frames, each converted out.
#pragma once

#include <cstddef>
#include <cstdint>

#include "sg_2d_h16_host.hpp"

namespace sg {

constexpr int GRAD_I16_DIRECT_MAX_N = 7;
enum GradRouteI16 { GRAD_I16_STAGED, GRAD_I16_DIRECT };
struct GradShapeI16 {
    int       nx, ny;
    int       rows, cols;
    long long in_stride, in_pitch, out_stride, out_pitch;       // elements of their own buffer; both outputs share stride and pitch
    uintptr_t in_base;
    bool      want_gx, want_gy;          // which frames the caller asked for (a non-NULL pointer)
    uintptr_t gx_base, gy_base;
    int       out_elem;                  // bytes per output element: 2 or 4
    bool      gx_direct, gy_direct;      // see above; looked at only for a requested frame
    bool      roll_tile_switch;
    bool      direct_switch;
};
inline GradRouteI16 grad_plan_i16(const GradShapeI16 &s)
{
    if (!s.want_gx && !s.want_gy) return GRAD_I16_STAGED;
    if (s.nx != s.ny || s.nx < 1 || s.nx > GRAD_I16_DIRECT_MAX_N) return GRAD_I16_STAGED;
    if ((s.want_gx && !s.gx_direct) || (s.want_gy && !s.gy_direct)) return GRAD_I16_STAGED;
    if (!s.roll_tile_switch || !s.direct_switch) return GRAD_I16_STAGED;
    // the layout: frame_plan_h16 with its filter conditions granted, once per requested frame
    FrameShapeH16 f;
    f.rows = s.rows; f.cols = s.cols;
    f.in_stride = s.in_stride; f.in_pitch = s.in_pitch; f.out_stride = s.out_stride; f.out_pitch = s.out_pitch;
    f.in_base = s.in_base; f.out_elem = s.out_elem;
    f.method = 0; f.x_dominant = false; f.additive_tile = true; f.roll_tile_switch = true; f.tiles_switch = true;
    const uintptr_t outs[2] = {s.gx_base, s.gy_base};
    const bool want[2] = {s.want_gx, s.want_gy};
    for (int i = 0; i < 2; ++i) {
        if (!want[i]) continue;
        f.out_base = outs[i];
        if (frame_plan_h16(f) != FRAME_H16_TILES) return GRAD_I16_STAGED;
    }
    return GRAD_I16_DIRECT;
}

// The staged route's scratch: THREE fp32 sides (the widened frames, gx, gy) within what frame_stage_h16 allows for two -- 2 x 2^24 floats, 128 MiB -- so
// max(1, floor(2^25 / 3) / (rows x stride)) whole frames per piece, frames of `stride` = cols rounded up to 4 floats a row, back to back.  A call that asks for
// one frame keeps the same pieces (and allocates two sides): the pieces do not depend on which outputs are requested.
constexpr size_t GRAD_I16_STAGED_MAX = 2 * FRAME_H16_STAGED_MAX / 3;
inline FrameStageH16 grad_stage_i16(int rows, int cols, size_t images)
{
    FrameStageH16 g;
    g.stride = (cols + 3) & ~3;
    g.frame = (size_t)rows * (size_t)g.stride;
    g.frames = GRAD_I16_STAGED_MAX / g.frame;
    if (g.frames < 1) g.frames = 1;
    if (g.frames > images) g.frames = images;
    return g;
}

}  // namespace sg
