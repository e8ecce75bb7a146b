// tests/mock/launch_i16_mock.cpp -- TEST INFRASTRUCTURE: the one launcher entry point of the int16-storage kernels (sg1d_launch_i16, which
// csrc/sg_api_1d.cpp declares weak), defined so that nothing touches a device: every call writes one line through the launch recorder's rec_note
// (tests/mock/launch_recorder_1d.cpp, linked next to this file by tests/test_i16_host.py).  The job is written field by field, in the words of the
// recorder's own job line; pointers are plain addresses (the test hands out fake ones and knows them; a table's address follows from its name).
#include <cinttypes>
#include <cstdio>

#include "sg_k1d_i16_host.hpp"

extern "C" void rec_note(const char *text);

extern "C" int sg1d_launch_i16(int n, int moment_terms, const sg::JobI16 *ji, const sg::Taps *taps, const float *d_table, unsigned grid, void *stream)
{
    const sg::Job1D &j = ji->base;
    uint64_t h = 0xcbf29ce484222325ull;                  // FNV-1a of the taps, as the recorder's digest
    const unsigned char *p = reinterpret_cast<const unsigned char *>(taps);
    for (size_t i = 0; i < sizeof(*taps); ++i) { h ^= p[i]; h *= 0x100000001b3ull; }
    char buf[2048];
    snprintf(buf, sizeof(buf), "i16 n=%d moment_terms=%d grid=%u stream=%p taps=%016" PRIx64 " table=0x%" PRIxPTR " out_type=%u in=0x%" PRIxPTR " out=0x%" PRIxPTR
             " in_ld=%lld out_ld=%lld length=%u tiles_per_channel=%u total_tiles=%u tpc_magic=%u tpc_shift=%u store_lo=%u store_hi=%u out_shift=%u dt_inv=%a "
             "flags=0x%x edge_items=%u edges=0x%" PRIxPTR " stash=0x%" PRIxPTR " ends=0x%" PRIxPTR " edge_stash=0x%" PRIxPTR " phase=%u tpc_all=%u xcd_chunk_log2=%u "
             "centre_sum=%a", n, moment_terms, grid, stream, h, (uintptr_t)d_table, ji->out_type, (uintptr_t)j.in, (uintptr_t)j.out, j.in_ld, j.out_ld, j.length,
             j.tiles_per_channel, j.total_tiles, j.tpc_magic, j.tpc_shift, j.store_lo, j.store_hi, j.out_shift, (double)j.dt_inv, j.flags, j.edge_items,
             (uintptr_t)j.edges, (uintptr_t)j.stash, (uintptr_t)j.ends, (uintptr_t)j.edge_stash, j.phase, j.tpc_all, j.xcd_chunk_log2, (double)j.centre_sum);
    rec_note(buf);
    return 0;
}
