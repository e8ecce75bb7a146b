// sg_k1d_multi_st16.hip -- instantiates a storage family's fused kernel, sg1d_multi_h16_kernel<N, SG_MULTI_K> or sg1d_multi_i16_kernel<N, SG_MULTI_K>
// (sg_k1d_multi_st16.hpp), for N in [SG_NLO, SG_NHI] and exports one launcher for that (output count, half-window group).  Compiled once per
// (family, output count, group) by the Makefile, with the half-window groups of sg_k1d_inst.hip.
#include "sg_k1d_multi_st16.hpp"

#if !defined(SG_FAMILY) || !defined(SG_MULTI_K) || !defined(SG_NLO) || !defined(SG_NHI) || !defined(SG_FN)
#error "compile with -DSG_FAMILY=h16|i16 -DSG_MULTI_K=2|3 -DSG_NLO=.. -DSG_NHI=.. -DSG_FN=symbol"
#endif

namespace sg {

typedef JobMultiSt16<Family::Types> JobMulti;

template <int N, int HI>
static int dispatch_multi_st16(int n, const JobMulti &job, const TapsMulti &taps, unsigned grid, hipStream_t st)
{
    if (n == N) { hipLaunchKernelGGL((SG_FAMILY_NAME(sg1d_multi_, _kernel)<N, SG_MULTI_K>), dim3(grid), dim3(256), 0, st, job, taps); return 1; }     // `grid` counts blocks of 4 tiles
    if constexpr (N < HI) return dispatch_multi_st16<N + 1, HI>(n, job, taps, grid, st);
    else return 0;
}

}  // namespace sg

// returns 1 if this group owns half window n (kernel enqueued), 0 otherwise
extern "C" int SG_FN(int n, const sg::JobMulti *job, const sg::TapsMulti *taps, unsigned grid, void *stream)
{
    return sg::dispatch_multi_st16<SG_NLO, SG_NHI>(n, *job, *taps, grid, static_cast<hipStream_t>(stream));
}
