// sg_k1d_strided_multi_launch.hpp -- what host and device share about sg1d_strided_multi_kernel<N> (sg_k1d_strided_multi.hpp): the by-value kernel
// arguments and the one launcher entry point.  No device code in here.
#pragma once

#include "sg_k1d_host.hpp"
#include "sg_k1d_strided_multi_host.hpp"

namespace sg {

// K = njobs (2 .. STRIDED_MULTI_MAX_PER_LAUNCH) filters of one half window on K fields of one record grid, into K fields of another (or the same) grid.
// `grid` is the single call's job on the two GRIDS: in / out are the grids' bases of this channel group (no field offset folded in), pitches, strides,
// length, the tile counts and the stored range as in JobStrided; flags = the mode byte all jobs share.  Its dt_inv and edges are unused;
// edge_items = 2 * channels * njobs: item e * njobs + k is end e (2c = leading, 2c + 1 = trailing end of channel c) of job k.
// The arrays carry job k's own: the byte offsets of its two fields from grid.in / grid.out, and the single call's dt_inv, flags and edge rows.
struct JobStridedMulti {
    JobStrided   grid;
    unsigned     njobs;
    long long    in_off[STRIDED_MULTI_MAX_PER_LAUNCH], out_off[STRIDED_MULTI_MAX_PER_LAUNCH];
    const float *edges[STRIDED_MULTI_MAX_PER_LAUNCH];      // job k's [n][2n+1] edge table, NULL = none
    float        dt_inv[STRIDED_MULTI_MAX_PER_LAUNCH];
    unsigned     flags[STRIDED_MULTI_MAX_PER_LAUNCH];      // mode byte, JOB_SCALE, JOB_EDGE_NEGATE: JobStrided::flags of the single call
};
struct TapsStridedMulti { Taps t[STRIDED_MULTI_MAX_PER_LAUNCH]; };
static_assert(sizeof(JobStridedMulti) + sizeof(TapsStridedMulti) < 4096, "the kernarg stays under 4 KB");

// One tile (or edge item) per wave and ONE wave per block: the wave's LDS is njobs slabs, sized per launch.
inline unsigned strided_multi_grid_blocks(unsigned items) { return (items + 7u) & ~7u; }

}  // namespace sg

extern "C" {
// one object per half-window group (the groups of the dense kernels); each returns 1 if it owns n
int sg1d_launch_strided_multi_g0(int n, const sg::JobStridedMulti *job, const sg::TapsStridedMulti *taps, unsigned grid, void *stream);
int sg1d_launch_strided_multi_g1(int n, const sg::JobStridedMulti *job, const sg::TapsStridedMulti *taps, unsigned grid, void *stream);
int sg1d_launch_strided_multi_g2(int n, const sg::JobStridedMulti *job, const sg::TapsStridedMulti *taps, unsigned grid, void *stream);
int sg1d_launch_strided_multi_g3(int n, const sg::JobStridedMulti *job, const sg::TapsStridedMulti *taps, unsigned grid, void *stream);
// The single entry point (sg_k1d_strided_multi_launch.cpp): picks the object that owns n, reports a failed launch; 0 = enqueued.  `grid` counts blocks
// (strided_multi_grid_blocks).  Weak: csrc/sg_api_1d.cpp links without it where a host-only build leaves the kernels out, and refuses there.
int sg1d_launch_strided_multi(int n, const sg::JobStridedMulti *job, const sg::TapsStridedMulti *taps, unsigned grid, void *stream) __attribute__((weak));
}
