// sg_k1d_i16_launch.cpp -- sg1d_launch_i16: the single launcher entry point of the int16-storage kernels.  It picks the object that owns (moment
// count, half window) and reports a failed launch; csrc/sg_api_1d.cpp reaches the kernels through this symbol alone (declared weak there:
// sg_k1d_i16_host.hpp).
#include "sg_k1d_i16_host.hpp"

extern "C" int sg1d_launch_i16(int n, int moment_terms, const sg::JobI16 *job, const sg::Taps *taps, const float *d_table, unsigned grid, void *stream)
{
    if (moment_terms != 0) {
        // the block-moment objects report their own failures
        if (moment_terms == 3) return sg1d_launch_i16_momenth_t3(n, job, d_table, grid, stream);
        if (moment_terms == 5) return sg1d_launch_i16_momenth_t5(n, job, d_table, grid, stream);
        if (moment_terms == 7) return sg1d_launch_i16_momenth_t7(n, job, d_table, grid, stream);
        sg_set_error("no int16-storage half-lane moment kernel with %d moments", moment_terms);
        return -1;
    }
    const int hit = sg1d_launch_i16_g0(n, job, taps, grid, stream) || sg1d_launch_i16_g1(n, job, taps, grid, stream) ||
                    sg1d_launch_i16_g2(n, job, taps, grid, stream) || sg1d_launch_i16_g3(n, job, taps, grid, stream);
    if (!hit) { sg_set_error("no int16-storage kernel for half_window %d", n); return -1; }
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) { sg_set_error("int16-storage kernel launch failed: %s", hipGetErrorString(e)); return -1; }
    return 0;
}
