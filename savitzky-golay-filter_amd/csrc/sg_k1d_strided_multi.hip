// sg_k1d_strided_multi.hip -- instantiates sg1d_strided_multi_kernel<N> for N in [SG_NLO, SG_NHI] and exports one launcher for that group.
// Compiled once per half-window group of the dense kernels by the Makefile, so that the 32 instantiations build side by side.
#include "sg_k1d_strided_multi.hpp"

#if !defined(SG_NLO) || !defined(SG_NHI) || !defined(SG_FN)
#error "compile with -DSG_NLO=.. -DSG_NHI=.. -DSG_FN=symbol"
#endif

namespace sg {

template <int N, int HI>
static int dispatch_strided_multi(int n, const JobStridedMulti &job, const TapsStridedMulti &taps, unsigned grid, hipStream_t st)
{
    if (n == N) {
        const size_t lds = (size_t)job.njobs * K1D<float, N, VPL_NARROW>::SLAB;
        hipLaunchKernelGGL((sg1d_strided_multi_kernel<N>), dim3(grid), dim3(64), lds, st, job, taps);
        return 1;
    }
    if constexpr (N < HI) return dispatch_strided_multi<N + 1, HI>(n, job, taps, grid, st);
    else return 0;
}

}  // namespace sg

// returns 1 if this group owns half window n (kernel enqueued), 0 otherwise; job->njobs in 2 .. STRIDED_MULTI_MAX_PER_LAUNCH
extern "C" int SG_FN(int n, const sg::JobStridedMulti *job, const sg::TapsStridedMulti *taps, unsigned grid, void *stream)
{
    if (job->njobs < 2u || job->njobs > (unsigned)sg::STRIDED_MULTI_MAX_PER_LAUNCH) return 0;
    return sg::dispatch_strided_multi<SG_NLO, SG_NHI>(n, *job, *taps, grid, static_cast<hipStream_t>(stream));
}
