// sg_k1d_strided_multi_launch.cpp -- sg1d_launch_strided_multi: the single launcher entry point of the multi-field strided kernels.  It picks the
// object that owns the half window and reports a failed launch; csrc/sg_api_1d.cpp reaches the kernels through this symbol alone (declared weak
// there: sg_k1d_strided_multi_launch.hpp).
#include "sg_k1d_strided_multi_launch.hpp"

extern "C" int sg1d_launch_strided_multi(int n, const sg::JobStridedMulti *job, const sg::TapsStridedMulti *taps, unsigned grid, void *stream)
{
    const int hit = sg1d_launch_strided_multi_g0(n, job, taps, grid, stream) || sg1d_launch_strided_multi_g1(n, job, taps, grid, stream) ||
                    sg1d_launch_strided_multi_g2(n, job, taps, grid, stream) || sg1d_launch_strided_multi_g3(n, job, taps, grid, stream);
    if (!hit) { sg_set_error("no multi-field strided kernel for half_window %d", n); return -1; }
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) { sg_set_error("multi-field strided kernel launch failed: %s", hipGetErrorString(e)); return -1; }
    return 0;
}
