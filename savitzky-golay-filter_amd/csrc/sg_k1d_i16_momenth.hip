// sg_k1d_i16_momenth.hip -- the int16-storage tile (sg_k1d_i16.hpp) around the fp32 half-lane block-moment inner product (MomentHConv,
// sg_k1d_momenth.hpp) for half windows 20..32 and ONE moment count per object (SG_MOMENT_TERMS = 3, 5 or 7; built three times by the Makefile).
// Two waves per block, as the fp32 kernel of this family (sg_k1d_momenth.hip).
#define SG_K1D_WAVES 2
#include "sg_k1d_momenth.hpp"
#include "sg_k1d_i16.hpp"

#if !defined(SG_MOMENT_TERMS) || !defined(SG_MOMENT_FN)
#error "compile with -DSG_MOMENT_TERMS=3|5|7 -DSG_MOMENT_FN=symbol"
#endif

namespace sg {

template <int N, int M1>
__global__ __launch_bounds__(64 * SG_K1D_WAVES, 4) void sg1d_i16_momenth_kernel(const JobI16 job, const MomentArgs args)
{
    sg1d_i16_body<N, MomentHConv<N, M1>>(job, args);
}

template <int N>
static int launch_i16_momenth(int n, const JobI16 &job, const MomentArgs &args, unsigned grid, hipStream_t st)
{
    if (n == N) {
        hipLaunchKernelGGL((sg1d_i16_momenth_kernel<N, SG_MOMENT_TERMS>), dim3(grid * (4 / SG_K1D_WAVES)), dim3(64 * SG_K1D_WAVES), 0, st, job, args);     // `grid` counts blocks of 4 tiles
        return 0;
    }
    if constexpr (N < MOMENT_MAX_N) return launch_i16_momenth<N + 1>(n, job, args, grid, st);
    else return 1;
}

}  // namespace sg

extern "C" int SG_MOMENT_FN(int n, const sg::JobI16 *job, const float *d_table, unsigned grid, void *stream)
{
    const sg::MomentArgs args{d_table};
    if (sg::launch_i16_momenth<sg::MOMENTH_MIN_N>(n, *job, args, grid, static_cast<hipStream_t>(stream)) != 0) {
        sg_set_error("no int16-storage half-lane moment kernel for half_window %d", n);
        return -1;
    }
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) { sg_set_error("int16-storage half-lane moment kernel launch failed: %s", hipGetErrorString(e)); return -1; }
    return 0;
}
