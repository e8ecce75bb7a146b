// sg_k1d_st16_launch.cpp -- the launcher entry points of the 16-bit-storage kernels that csrc/sg_api_1d.cpp reaches through ONE symbol each (declared
// weak there: sg_k1d_st16_host.hpp): sg1d_launch_i16, sg1d_launch_multi_h16, sg1d_launch_multi_i16.  Each picks the object that owns its (moment
// count or output count, half window) and reports a failed launch.
#include "sg_k1d_st16_host.hpp"

namespace {

template <typename Job>
using Groups = int (*const[4])(int, const Job *, const sg::TapsMulti *, unsigned, void *);

// k = 2 or 3 outputs: that count's four half-window groups
template <typename Job>
int launch_multi16(const Groups<Job> &two, const Groups<Job> &three, const char *what, int n, int k, const Job *job, const sg::TapsMulti *taps, unsigned grid,
                   void *stream)
{
    return sg::launch_groups16(k == 2 ? two : k == 3 ? three : nullptr, what, n, k, job, taps, grid, stream);
}

}  // namespace

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
    static constexpr int (*GROUPS[4])(int, const sg::JobI16 *, const sg::Taps *, unsigned, void *) = SG_ST16_GROUPS(sg1d_launch_i16);
    return sg::launch_groups16(GROUPS, "int16-storage", n, 0, job, taps, grid, stream);
}

extern "C" int sg1d_launch_multi_h16(int n, int k, const sg::JobMultiH16 *job, const sg::TapsMulti *taps, unsigned grid, void *stream)
{
    static constexpr Groups<sg::JobMultiH16> TWO = SG_ST16_GROUPS(sg1d_launch_multi_h16_2), THREE = SG_ST16_GROUPS(sg1d_launch_multi_h16_3);
    return launch_multi16(TWO, THREE, "16-bit multi-output", n, k, job, taps, grid, stream);
}

extern "C" int sg1d_launch_multi_i16(int n, int k, const sg::JobMultiI16 *job, const sg::TapsMulti *taps, unsigned grid, void *stream)
{
    static constexpr Groups<sg::JobMultiI16> TWO = SG_ST16_GROUPS(sg1d_launch_multi_i16_2), THREE = SG_ST16_GROUPS(sg1d_launch_multi_i16_3);
    return launch_multi16(TWO, THREE, "int16 multi-output", n, k, job, taps, grid, stream);
}
