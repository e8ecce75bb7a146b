// sg_2d_h16_host.hpp -- host-only rules of the 2-D batch calls (no device types: g++ translation units include it too): whether two frame stacks
// share a byte (frames_overlap, every 2-D device entry point), and the route of the call on 16-bit storage (frame_plan_h16,
// savgol2d_apply_batch_h16).  tests/mock/frame_plan_h16.cpp prints both for tables of shapes.
#pragma once

#include <cstddef>
#include <cstdint>

namespace sg {

// Do two frame stacks share a byte?  EXACT for strided layouts (side-by-side views of one buffer -- in = buf[:, :cols], out = buf[:, cols:], stride
// 2 cols -- and frames interleaved at a common pitch share none).  The stacks may hold elements of different sizes (a_elem, b_elem: 2 or 4 bytes);
// strides and pitches count elements of their own stack.  Everything below is in UNITS of the smaller element: a stack is the set
// { i*pitch + r*stride + c : i < images, r < rows, c < width }, a row of the wider type being twice as many units wide.  Two fp32 stacks: the unit
// is the float and this is the test the fp32 calls have always had.
inline bool rows_share(long long a, long long sa, long long wa, long long b, long long sb, long long wb, int rows)
{
    // two single frames: merge their row intervals in address order (strides are >= the row width, so each frame's rows are sorted and disjoint)
    int ia = 0, ib = 0;
    while (ia < rows && ib < rows) {
        const long long a0 = a + ia * sa, b0 = b + ib * sb;
        if (a0 < b0 + wb && b0 < a0 + wa) return true;
        if (a0 + wa <= b0 + wb) ++ia; else ++ib;
    }
    return false;
}
inline bool frames_overlap(uintptr_t a0, size_t a_elem, long long a_pitch, long long a_stride, uintptr_t b0, size_t b_elem, long long b_pitch, long long b_stride,
                           int rows, int cols, size_t images)
{
    const size_t unit = a_elem < b_elem ? a_elem : b_elem;
    const long long ka = (long long)(a_elem / unit), kb = (long long)(b_elem / unit);
    const long long wa = cols * ka, wb = cols * kb;
    a_stride *= ka; a_pitch *= ka; b_stride *= kb; b_pitch *= kb;
    const long long a_frame = (long long)(rows - 1) * a_stride + wa, b_frame = (long long)(rows - 1) * b_stride + wb;      // units one frame spans
    const uintptr_t a1 = a0 + unit * ((size_t)(images - 1) * (size_t)a_pitch + (size_t)a_frame);
    const uintptr_t b1 = b0 + unit * ((size_t)(images - 1) * (size_t)b_pitch + (size_t)b_frame);
    if (!(a0 < b1 && b0 < a1)) return false;                                    // bounding ranges apart: the common case
    // layouts this test does not model exactly are refused as before: bases a fraction of a unit apart, frames of one batch running into
    // each other, negative pitches
    if ((a0 > b0 ? a0 - b0 : b0 - a0) % unit != 0) return true;
    if (images > 1 && (a_pitch < a_frame || b_pitch < b_frame)) return true;
    const long long delta = (a0 > b0 ? (long long)((a0 - b0) / unit) : -(long long)((b0 - a0) / unit));     // a - b in units
    if (wa == wb && a_stride == b_stride && (images == 1 || a_pitch == b_pitch)) {
        // equal widths, strides and pitches: frame i row r col c of `a` meets frame i' row r' col c' of `b` iff
        // delta = di*pitch + dr*stride + dc with |di| < images, |dr| < rows, |dc| < width.  Frames and rows of one batch do not run into
        // each other (pitch >= frame span, stride >= width), so only two candidates per level can match.
        const long long s = a_stride, p = images > 1 ? a_pitch : 0;
        auto fdiv = [](long long x, long long y) { long long q = x / y; if ((x % y != 0) && ((x < 0) != (y < 0))) --q; return q; };
        for (int ci = 0; ci < (images > 1 ? 2 : 1); ++ci) {
            const long long di = images > 1 ? fdiv(-delta, p) + ci : 0;
            if (di <= -(long long)images || di >= (long long)images) continue;
            const long long rem = -delta - di * p;                                // = dr*stride + dc
            for (int cr = 0; cr < 2; ++cr) {
                const long long dr = fdiv(rem, s) + cr;
                if (dr <= -(long long)rows || dr >= (long long)rows) continue;
                const long long dc = rem - dr * s;
                if (dc > -wa && dc < wa) return true;
            }
        }
        return false;
    }
    // different widths, strides or pitches: merge the frames' spans in address order, rows of the frame pairs whose spans intersect
    size_t ia = 0, ib = 0;
    while (ia < images && ib < images) {
        const long long fa = delta + (long long)ia * a_pitch, fb = (long long)ib * b_pitch;
        if (fa < fb + b_frame && fb < fa + a_frame && rows_share(fa, a_stride, wa, fb, b_stride, wb, rows)) return true;
        if (fa + a_frame <= fb + b_frame) ++ia; else ++ib;
    }
    return false;
}

// ---- savgol2d_apply_batch_h16: which route a call takes, decided before anything is enqueued ----
// The TWIN is savgol2d_apply_batch_f32 on the frames widened exactly, in 16-byte aligned fp32 buffers with stride = cols rounded up to 4 and pitch
// rows x stride.  TILES when the twin launches the rolling kernel's ADDITIVE TILE FORM (launch_roll_kernel<N, 2, 1, true, false, TR>, TR > 0) and the
// caller's 16-bit buffers can feed the same tiles on vector loads and stores -- every one of:
//   additive_tile   the filter's factors are the additive form (square windows: a rectangular window's zero-padded factors are not) and its half window has an additive tile:
//                   sg2d_launch_rolling_h16's predicate, which asks fill_box_taps and roll_tile_rows themselves
//   !x_dominant     (sg2d_x_dominant: such frames take the horizontal-first kernel), method 0 or 2
//   cols % 4 == 0 and cols >= 32
//   quads naturally aligned: the 16-bit side(s) on 8-byte bases with stride and pitch multiples of 4, an fp32 output on a 16-byte base
//   rows x out_stride x out_elem under the store descriptor's 0x7fffff00 -- and rows x cols x 4, the twin's own output, under it too (else the
//                   twin itself leaves the tiles for the strip walk)
//   roll_tile_switch  SAVGOL_HIP_ROLL_TILE is not 0 (at 0 the twin's own tiles are off)
//   tiles_switch    SAVGOL_HIP_2D_H16_TILES is not 0 (A/B runs and tests)
// STAGED: every other call -- the twin itself, on frames widened into aligned fp32 scratch and rounded out, whole frames per piece.
enum FrameRouteH16 { FRAME_H16_STAGED, FRAME_H16_TILES };
constexpr long long FRAME_H16_DESCRIPTOR_LIMIT = 0x7fffff00ll;
struct FrameShapeH16 {
    int       rows, cols;
    long long in_stride, in_pitch, out_stride, out_pitch;       // elements of their own buffer
    uintptr_t in_base, out_base;
    int       out_elem;                  // bytes per output element: 2 or 4
    int       method;
    bool      x_dominant;
    bool      additive_tile;
    bool      roll_tile_switch;
    bool      tiles_switch;
};
inline FrameRouteH16 frame_plan_h16(const FrameShapeH16 &s)
{
    if (!s.additive_tile || s.x_dominant || (s.method != 0 && s.method != 2) || !s.roll_tile_switch || !s.tiles_switch) return FRAME_H16_STAGED;
    if (s.cols % 4 != 0 || s.cols < 32) return FRAME_H16_STAGED;
    if ((s.in_base & 7u) != 0 || s.in_stride % 4 != 0 || s.in_pitch % 4 != 0) return FRAME_H16_STAGED;
    if ((s.out_base & (s.out_elem == 4 ? 15u : 7u)) != 0 || s.out_stride % 4 != 0 || s.out_pitch % 4 != 0) return FRAME_H16_STAGED;
    if ((long long)s.rows * s.out_stride * s.out_elem >= FRAME_H16_DESCRIPTOR_LIMIT) return FRAME_H16_STAGED;
    if ((long long)s.rows * s.cols * 4 >= FRAME_H16_DESCRIPTOR_LIMIT) return FRAME_H16_STAGED;
    return FRAME_H16_TILES;
}

// The staged route's scratch: fp32 frames of `stride` = cols rounded up to 4 floats a row, back to back; max(1, 2^24 / (rows x stride)) whole
// frames per piece -- 64 MiB per side unless one frame alone is larger.
constexpr size_t FRAME_H16_STAGED_MAX = (size_t)1 << 24;
struct FrameStageH16 { int stride; size_t frame; size_t frames; };       // floats per row, floats per frame, frames per piece
inline FrameStageH16 frame_stage_h16(int rows, int cols, size_t images)
{
    FrameStageH16 g;
    g.stride = (cols + 3) & ~3;
    g.frame = (size_t)rows * (size_t)g.stride;
    g.frames = FRAME_H16_STAGED_MAX / g.frame;
    if (g.frames < 1) g.frames = 1;
    if (g.frames > images) g.frames = images;
    return g;
}

}  // namespace sg
