// sg_k1d_st16_momenth.hip -- the 16-bit-storage tile (sg_k1d_st16.hpp) of one storage family around the fp32 half-lane block-moment inner product
// (MomentHConv, sg_k1d_momenth.hpp) for half windows 20..32 and ONE moment count per object (SG_MOMENT_TERMS = 3, 5 or 7; built three times per
// family by the Makefile).  Two waves per block, as the fp32 kernel of this form (sg_k1d_momenth.hip).
#define SG_K1D_WAVES 2
#include "sg_k1d_momenth.hpp"
#include "sg_k1d_st16.hpp"

#if !defined(SG_FAMILY) || !defined(SG_MOMENT_TERMS) || !defined(SG_MOMENT_FN)
#error "compile with -DSG_FAMILY=h16|i16 -DSG_MOMENT_TERMS=3|5|7 -DSG_MOMENT_FN=symbol"
#endif

namespace sg {

typedef JobSt16<Family::Types> Job;

// sg1d_h16_momenth_kernel / sg1d_i16_momenth_kernel
template <int N, int M1>
__global__ __launch_bounds__(64 * SG_K1D_WAVES, 4) void SG_FAMILY_NAME(sg1d_, _momenth_kernel)(const Job job, const MomentArgs args)
{
    sg1d_st16_body<N, MomentHConv<N, M1>, Family>(job, args);
}

template <int N>
static int launch_st16_momenth(int n, const Job &job, const MomentArgs &args, unsigned grid, hipStream_t st)
{
    if (n == N) {
        hipLaunchKernelGGL((SG_FAMILY_NAME(sg1d_, _momenth_kernel)<N, SG_MOMENT_TERMS>), dim3(grid * (4 / SG_K1D_WAVES)), dim3(64 * SG_K1D_WAVES), 0, st, job, args);     // `grid` counts blocks of 4 tiles
        return 0;
    }
    if constexpr (N < MOMENT_MAX_N) return launch_st16_momenth<N + 1>(n, job, args, grid, st);
    else return 1;
}

}  // namespace sg

extern "C" int SG_MOMENT_FN(int n, const sg::Job *job, const float *d_table, unsigned grid, void *stream)
{
    const sg::MomentArgs args{d_table};
    if (sg::launch_st16_momenth<sg::MOMENTH_MIN_N>(n, *job, args, grid, static_cast<hipStream_t>(stream)) != 0) {
        sg_set_error("no %s-storage half-lane moment kernel for half_window %d", sg::Family::Types::NOUN, n);
        return -1;
    }
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) { sg_set_error("%s-storage half-lane moment kernel launch failed: %s", sg::Family::Types::NOUN, hipGetErrorString(e)); return -1; }
    return 0;
}
