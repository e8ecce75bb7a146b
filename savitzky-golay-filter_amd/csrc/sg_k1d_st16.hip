// sg_k1d_st16.hip -- instantiates a storage family's plain kernel, sg1d_h16_kernel<N> or sg1d_i16_kernel<N> (sg_k1d_st16.hpp), for N in
// [SG_NLO, SG_NHI] and exports one launcher for that half-window group.  Compiled once per (family, group) by the Makefile, with the half-window
// groups of sg_k1d_inst.hip.
#include "sg_k1d_st16.hpp"

#if !defined(SG_FAMILY) || !defined(SG_NLO) || !defined(SG_NHI) || !defined(SG_FN)
#error "compile with -DSG_FAMILY=h16|i16 -DSG_NLO=.. -DSG_NHI=.. -DSG_FN=symbol"
#endif

namespace sg {

typedef JobSt16<Family::Types> Job;

template <int N, int HI>
static int dispatch_st16(int n, const Job &job, const Taps &taps, unsigned grid, hipStream_t st)
{
    if (n == N) { hipLaunchKernelGGL((SG_FAMILY_NAME(sg1d_, _kernel)<N>), dim3(grid * (4 / SG_K1D_WAVES)), dim3(64 * SG_K1D_WAVES), 0, st, job, taps); return 1; }     // `grid` counts blocks of 4 tiles
    if constexpr (N < HI) return dispatch_st16<N + 1, HI>(n, job, taps, grid, st);
    else return 0;
}

}  // namespace sg

// returns 1 if this group owns half window n (kernel enqueued), 0 otherwise
extern "C" int SG_FN(int n, const sg::Job *job, const sg::Taps *taps, unsigned grid, void *stream)
{
    return sg::dispatch_st16<SG_NLO, SG_NHI>(n, *job, *taps, grid, static_cast<hipStream_t>(stream));
}
