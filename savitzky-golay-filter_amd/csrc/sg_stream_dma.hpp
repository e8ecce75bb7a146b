// sg_stream_dma.hpp -- device pieces shared by the LDS-DMA tile kernels of the stream block push (sg_stream_dma.hip, sg_stream_dma_multi.hip and the body
// tile sg_stream_dma_body.inc): the tile shape, the counted wait, the DMA instruction, the block-moment taps and their packing.  The arithmetic of a tile --
// the three summation forms and the block moments -- is the fragment sg_stream_dma_feed.hpp, which every kernel's `feed` lambda includes, so the 16-bit and
// fused kernels compute the fp32 kernel's bits by construction.  DmaQueue and MomGeom (plain constexpr) are in sg_stream_host.hpp.
#pragma once

#include <hip/hip_runtime.h>

#include <cstring>

#include "sg_pk.hpp"
#include "sg_stream_roll.hpp"

namespace sg {

// output ticks per tile TR: the slab is TR + 2n rows of 512 bytes, the accumulators 2 (reference order) or 4 (two FMA chains) VGPRs per tick
template <int N, int TR_> struct DmaShape {
    static constexpr int TR = TR_;
    static constexpr int ROWS = TR + 2 * N, NI = ROWS / 2, RB = 512, SLAB = ROWS * RB;
    static_assert(TR % 2 == 0, "a DMA instruction moves two rows");
};

template <int K> __device__ __forceinline__ void wait_vm()
{
    static_assert(K >= 0 && K < 64, "vmcnt is a 6-bit counter");
    asm volatile("s_waitcnt vmcnt(%0)" :: "n"(K) : "memory");
}

// one 1 KiB LDS-DMA: lane l's 16 bytes land at lds_dst + 16 l.  Inline asm (the compiler then neither counts it nor drains it at the
// first LDS read: the waits are counted by hand below); M0 is the compiler's, so it is saved and restored in the same statement.
__device__ __forceinline__ void dma16(const float *gsrc, unsigned lds_dst)
{
    unsigned keep;
    asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, off\n\ts_mov_b32 m0, %0"
                 : "=&s"(keep) : "v"(gsrc), "s"(lds_dst) : "memory");
}

// q_0 = 1, q_1(t) = t - 3.5, q_2(t) = (t - 3.5)^2 - 5.25 on t = 0..7 (orthogonal; every value exact in fp32)
template <int N, int M> struct MomTaps {
    f32x2 head[4];                                   // w[0 .. 7]        (direct taps before the first whole block: k <= 6)
    f32x2 tail[4];                                   // w[2N - 7 .. 2N]  (direct taps after the last whole block: k >= 2N - 6)
    f32x2 c[M][(MomGeom<N>::NOFF + 1) / 2];          // c[s][off]: the block at offset off = 8j - m contributes sum_s c[s][off] * moment_s
    f32x2 q[M > 1 ? M - 1 : 1][4];                   // q_s(t), s = 1 .. M - 1
};
// host: the bank's centre taps and the host fit of them (block_form asked for it) as a block-moment tile's kernel argument
template <int N, int M>
inline void pack_mom_taps(const StreamMomentFit &fit, const float *center, MomTaps<N, M> *taps)
{
    memset(taps, 0, sizeof(*taps));
    pack_taps(center, 8, taps->head);
    pack_taps(center + 2 * N - 7, 8, taps->tail);
    for (int sm = 0; sm < M; ++sm) pack_taps(fit.c[sm], MomGeom<N>::NOFF, taps->c[sm]);
    float q[2][8];
    for (int t = 0; t < 8; ++t) { q[0][t] = (float)t - 3.5f; q[1][t] = q[0][t] * q[0][t] - 5.25f; }
    for (int sm = 0; sm + 1 < M; ++sm) pack_taps(q[sm], 8, taps->q[sm]);
}

}  // namespace sg
