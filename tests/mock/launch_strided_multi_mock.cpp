// tests/mock/launch_strided_multi_mock.cpp -- TEST INFRASTRUCTURE: the one launcher entry point of the multi-field strided kernels
// (sg1d_launch_strided_multi, which csrc/sg_api_1d.cpp declares weak), defined so that nothing touches a device: every call writes one line through
// the launch recorder's rec_note (tests/mock/launch_recorder_1d.cpp, linked next to this file by tests/test_strided_multi_host.py).  The job is
// written field by field in the words of the recorder's own strided line; pointers are plain addresses (the test hands out fake ones and knows them),
// an edge table shows as present or not (the recorder hands out real host memory for tables).
#include <cinttypes>
#include <cstdio>
#include <string>

#include "sg_k1d_strided_multi_launch.hpp"

extern "C" void rec_note(const char *text);

extern "C" int sg1d_launch_strided_multi(int n, const sg::JobStridedMulti *j, const sg::TapsStridedMulti *taps, unsigned grid, void *stream)
{
    const sg::JobStrided &g = j->grid;
    char buf[1024];
    snprintf(buf, sizeof(buf), "strided_multi n=%d njobs=%u grid=%u stream=%p in=0x%" PRIxPTR " out=0x%" PRIxPTR " in_pitch=%lld out_pitch=%lld in_stride=%lld "
             "out_stride=%lld length=%u tiles_per_channel=%u total_tiles=%u tpc_magic=%u tpc_shift=%u store_lo=%u store_hi=%u flags=0x%x edge_items=%u",
             n, j->njobs, grid, stream, (uintptr_t)g.in, (uintptr_t)g.out, g.in_pitch, g.out_pitch, g.in_stride, g.out_stride, g.length, g.tiles_per_channel,
             g.total_tiles, g.tpc_magic, g.tpc_shift, g.store_lo, g.store_hi, g.flags, g.edge_items);
    std::string s = buf;
    for (int k = 0; k < sg::STRIDED_MULTI_MAX_PER_LAUNCH; ++k) {
        uint64_t h = 0xcbf29ce484222325ull;                  // FNV-1a of job k's taps, as the recorder's digest
        const unsigned char *p = reinterpret_cast<const unsigned char *>(&taps->t[k]);
        for (size_t i = 0; i < sizeof(taps->t[k]); ++i) { h ^= p[i]; h *= 0x100000001b3ull; }
        snprintf(buf, sizeof(buf), " [%d]{in_off=%lld out_off=%lld has_edges=%d dt_inv=%a flags=0x%x taps=%016" PRIx64 "}", k, j->in_off[k], j->out_off[k],
                 j->edges[k] != nullptr, (double)j->dt_inv[k], j->flags[k], h);
        s += buf;
    }
    rec_note(s.c_str());
    return 0;
}
