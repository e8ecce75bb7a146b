// sg_k1d_multi_i16_launch.cpp -- sg1d_launch_multi_i16: the single launcher entry point of the fused multi-output kernels on int16 storage.  It picks
// the object that owns (output count, half window) and reports a failed launch; csrc/sg_api_1d.cpp reaches the kernels through this symbol alone
// (declared weak there: sg_k1d_multi_i16_host.hpp).
#include "sg_k1d_multi_i16_host.hpp"

extern "C" int sg1d_launch_multi_i16(int n, int k, const sg::JobMultiI16 *job, const sg::TapsMulti *taps, unsigned grid, void *stream)
{
    const int hit = k == 2 ? (sg1d_launch_multi_i16_2_g0(n, job, taps, grid, stream) || sg1d_launch_multi_i16_2_g1(n, job, taps, grid, stream) ||
                              sg1d_launch_multi_i16_2_g2(n, job, taps, grid, stream) || sg1d_launch_multi_i16_2_g3(n, job, taps, grid, stream))
                  : k == 3 ? (sg1d_launch_multi_i16_3_g0(n, job, taps, grid, stream) || sg1d_launch_multi_i16_3_g1(n, job, taps, grid, stream) ||
                              sg1d_launch_multi_i16_3_g2(n, job, taps, grid, stream) || sg1d_launch_multi_i16_3_g3(n, job, taps, grid, stream))
                  : 0;
    if (!hit) { sg_set_error("no int16 multi-output kernel for half_window %d, %d outputs", n, k); return -1; }
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) { sg_set_error("int16 multi-output kernel launch failed: %s", hipGetErrorString(e)); return -1; }
    return 0;
}
