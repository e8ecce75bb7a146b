// tests/mock/launch_multi_i16_mock.cpp -- TEST INFRASTRUCTURE: the one launcher entry point of the fused multi-output kernels on int16 storage
// (sg1d_launch_multi_i16, which csrc/sg_api_1d.cpp declares weak), defined so that nothing touches a device: every call writes one line through the
// launch recorder's rec_note (tests/mock/launch_recorder_1d.cpp, linked next to this file by tests/test_multi_i16_host.py).  The job is written field
// by field, in the words of the recorder's own multi line; pointers are plain addresses (the test hands out fake ones and knows them).
#include <cinttypes>
#include <cstdio>
#include <string>

#include "sg_k1d_multi_i16_host.hpp"

extern "C" void rec_note(const char *text);

extern "C" int sg1d_launch_multi_i16(int n, int k, const sg::JobMultiI16 *ji, const sg::TapsMulti *taps, unsigned grid, void *stream)
{
    const sg::JobMulti1D &j = ji->multi;
    const sg::Job1D &b = j.base;
    char buf[1024];
    snprintf(buf, sizeof(buf), "multi_i16 n=%d k=%d grid=%u stream=%p out_type=%u nraw=%u in=0x%" PRIxPTR " in_ld=%lld out_ld=%lld length=%u "
             "tiles_per_channel=%u total_tiles=%u tpc_magic=%u tpc_shift=%u store_lo=%u store_hi=%u out_shift=%u flags=0x%x edge_items=%u xcd_chunk_log2=%u",
             n, k, grid, stream, ji->out_type, j.nraw, (uintptr_t)b.in, b.in_ld, b.out_ld, b.length, b.tiles_per_channel, b.total_tiles,
             b.tpc_magic, b.tpc_shift, b.store_lo, b.store_hi, b.out_shift, b.flags, b.edge_items, b.xcd_chunk_log2);
    std::string s = buf;
    for (int o = 0; o < sg::MULTI_MAX_K; ++o) {
        uint64_t h = 0xcbf29ce484222325ull;                  // FNV-1a of output o's taps, as the recorder's digest
        const unsigned char *p = reinterpret_cast<const unsigned char *>(&taps->t[o]);
        for (size_t i = 0; i < sizeof(taps->t[o]); ++i) { h ^= p[i]; h *= 0x100000001b3ull; }
        snprintf(buf, sizeof(buf), " [%d]{out=0x%" PRIxPTR " has_edges=%d dt_inv=%a centre_sum=%a flags=0x%x taps=%016" PRIx64 "}", o, (uintptr_t)j.out[o],
                 j.edges[o] != nullptr, (double)j.dt_inv[o], (double)j.centre_sum[o], j.flags[o], h);
        s += buf;
    }
    rec_note(s.c_str());
    return 0;
}
