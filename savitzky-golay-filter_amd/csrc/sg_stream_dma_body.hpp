// sg_stream_dma_body.hpp -- what goes with the body tile of the stream block push (the fragment sg_stream_dma_body.inc): the taps of its K outputs and the
// launch of body tiles, which the fp32 fused tiles (sg_stream_dma_multi.hip) share.
#pragma once

#include <hip/hip_runtime.h>

#include "sg_stream_host.hpp"
#include "sg_stream_roll.hpp"

namespace sg {

template <int N, int K> struct MultiH16Taps { SRollTaps<N> t[K]; };

// output k's taps: the taps argument itself where the tile has one output (SRollTaps<N> or MomTaps<N, M>), else its k-th table
template <int k, class TAPS> __device__ __forceinline__ const TAPS &body_taps(const TAPS &taps) { return taps; }
template <int k, int N, int K> __device__ __forceinline__ const SRollTaps<N> &body_taps(const MultiH16Taps<N, K> &all) { return all.t[k]; }

// One launch of body tiles (WPB waves per block, a ring of DP KiB per wave); 1 = the runtime refused it
template <int WPB, int DP, class Kernel, class Job, class Taps>
static int launch_body_tiles(Kernel kernel, const Job &job, const Taps &taps, const TileGeom &geo, unsigned grid, hipStream_t st)
{
    constexpr size_t lds = (size_t)WPB * DP * 1024;
    static_assert(lds <= 160 * 1024, "the rings of one block must fit the CU's LDS");
    // more than 64 KiB of dynamic LDS needs the attribute, per (function, device): set per launch, as launch_dma_tiles (sg_stream_dma.hip) does
    if (lds > 65536 && hipFuncSetAttribute(reinterpret_cast<const void *>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess) {
        (void)hipGetLastError();
        return 1;
    }
    hipLaunchKernelGGL(kernel, dim3(grid), dim3(64 * WPB), lds, st, job, taps, geo);
    return hipGetLastError() == hipSuccess ? 0 : 1;
}

}  // namespace sg
