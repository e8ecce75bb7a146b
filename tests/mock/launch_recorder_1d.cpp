// tests/mock/launch_recorder_1d.cpp -- TEST INFRASTRUCTURE: everything csrc/sg_api_1d.cpp (with sg_weights.c and sg_k1d_moment_fit.cpp) leaves
// undefined -- the kernel launchers, the sg:: runtime functions, the error text and the HIP runtime calls -- defined so that nothing touches a
// device and every call writes one line into an in-memory log.  tests/test_launch_record_1d.py builds this with g++ next to the product's own
// host sources (libamdhip64 is not linked), drives the public C entry points and compares the log with tests/golden/launch_record_1d.txt: the
// record of WHAT THE HOST SIDE OF THE 1-D PATH ENQUEUES, taken without a GPU.  Nothing in the product links this file.
//
// A line is the call's name, its scalar arguments, the job struct field by field (never raw bytes: padding does not matter), tap tables as a
// digest of their content, and pointers by name: "<base>+<offset>" for the address ranges the test registered (rec_add_base), "scratch#k+off"
// for the k-th stream-ordered allocation since rec_reset, "arena+off" / "pinned+off" for the context's buffers, "table(salt,digest,bytes)" for
// an uploaded table.  Not logged: ctx_get, ctx_table (a plan is built once per filter content and process, so whether a call uploads depends on
// what ran before it; the table's NAME carries salt and content) and the two error queries hipGetLastError / hipGetErrorString.
#include <cinttypes>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <string>
#include <vector>

#include "sg_k1d_host.hpp"
#include "sg_k1d_h16_host.hpp"
#include "sg_runtime.hpp"

namespace {

std::string g_log;
char g_error[1024] = "";
int g_small_taken = 0;

struct Range { std::string name; uintptr_t lo, bytes; };
std::vector<Range> g_bases, g_scratch;
std::map<uintptr_t, std::string> g_tables;
constexpr uintptr_t SCRATCH_BASE = (uintptr_t)0x600000000000ull, ARENA_BASE = (uintptr_t)0x500000000000ull, ARENA_BYTES = (uintptr_t)1 << 40;
uintptr_t g_scratch_top = SCRATCH_BASE;
std::vector<unsigned char> g_pinned;            // real memory: the zero-copy host path copies through it

void logf(const char *fmt, ...) __attribute__((format(printf, 1, 2)));
void logf(const char *fmt, ...)
{
    char line[4096];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(line, sizeof(line), fmt, ap);
    va_end(ap);
    g_log += line;
    g_log += '\n';
}

uint64_t digest(const void *p, size_t n)         // FNV-1a, 64 bit
{
    const unsigned char *b = static_cast<const unsigned char *>(p);
    uint64_t h = 0xcbf29ce484222325ull;
    for (size_t i = 0; i < n; ++i) { h ^= b[i]; h *= 0x100000001b3ull; }
    return h;
}

std::string ptr(const void *p)
{
    if (!p) return "null";
    const uintptr_t a = (uintptr_t)p;
    char buf[160];
    auto in = [&](const Range &r) { return a >= r.lo && a - r.lo < r.bytes; };
    for (const Range &r : g_bases) if (in(r)) { snprintf(buf, sizeof(buf), "%s+%" PRIuPTR, r.name.c_str(), a - r.lo); return buf; }
    for (const Range &r : g_scratch) if (in(r)) { snprintf(buf, sizeof(buf), "%s+%" PRIuPTR, r.name.c_str(), a - r.lo); return buf; }
    if (a >= ARENA_BASE && a - ARENA_BASE < ARENA_BYTES) { snprintf(buf, sizeof(buf), "arena+%" PRIuPTR, a - ARENA_BASE); return buf; }
    if (!g_pinned.empty() && a >= (uintptr_t)g_pinned.data() && a - (uintptr_t)g_pinned.data() < g_pinned.size()) {
        snprintf(buf, sizeof(buf), "pinned+%" PRIuPTR, a - (uintptr_t)g_pinned.data());
        return buf;
    }
    auto t = g_tables.find(a);
    if (t != g_tables.end()) return t->second;
    return "UNKNOWN";                            // an address nobody handed out: never expected in a record
}
#define P(x) ptr(x).c_str()

std::string job1d(const sg::Job1D &j)
{
    char buf[1024];
    snprintf(buf, sizeof(buf), "in=%s out=%s in_ld=%lld out_ld=%lld length=%u tiles_per_channel=%u total_tiles=%u tpc_magic=%u tpc_shift=%u store_lo=%u "
             "store_hi=%u out_shift=%u dt_inv=%a flags=0x%x edge_items=%u edges=%s stash=%s ends=%s edge_stash=%s phase=%u tpc_all=%u xcd_chunk_log2=%u "
             "centre_sum=%a", P(j.in), P(j.out), j.in_ld, j.out_ld, j.length, j.tiles_per_channel, j.total_tiles, j.tpc_magic, j.tpc_shift, j.store_lo,
             j.store_hi, j.out_shift, (double)j.dt_inv, j.flags, j.edge_items, P(j.edges), P(j.stash), P(j.ends), P(j.edge_stash), j.phase, j.tpc_all,
             j.xcd_chunk_log2, (double)j.centre_sum);
    return buf;
}

// the half-window groups of the kernel objects (savitzky-golay-filter_amd/Makefile, k1d_lo_* / k1d_hi_*): a group launcher returns 1 when it owns n
bool owns(int group, int n)
{
    static const int lo[4] = {1, 15, 23, 29}, hi[4] = {14, 22, 28, 32};
    return n >= lo[group] && n <= hi[group];
}

int center(const char *name, int group, int n, int wide, const sg::Job1D *job, const sg::Taps *taps, unsigned grid, void *stream)
{
    if (!owns(group, n)) return 0;
    logf("%s n=%d wide=%d grid=%u stream=%p taps=%016" PRIx64 " job{%s}", name, n, wide, grid, stream, digest(taps, sizeof(*taps)), job1d(*job).c_str());
    return 1;
}

int strided(const char *name, int group, int n, const sg::JobStrided *j, const sg::Taps *taps, unsigned grid, void *stream)
{
    if (!owns(group, n)) return 0;
    logf("%s n=%d grid=%u stream=%p taps=%016" PRIx64 " job{in=%s out=%s in_pitch=%lld out_pitch=%lld in_stride=%lld out_stride=%lld length=%u "
         "tiles_per_channel=%u total_tiles=%u tpc_magic=%u tpc_shift=%u store_lo=%u store_hi=%u dt_inv=%a flags=0x%x edge_items=%u edges=%s}", name, n, grid,
         stream, digest(taps, sizeof(*taps)), P(j->in), P(j->out), j->in_pitch, j->out_pitch, j->in_stride, j->out_stride, j->length, j->tiles_per_channel,
         j->total_tiles, j->tpc_magic, j->tpc_shift, j->store_lo, j->store_hi, (double)j->dt_inv, j->flags, j->edge_items, P(j->edges));
    return 1;
}

int multi(const char *name, int group, int n, const sg::JobMulti1D *j, const sg::TapsMulti *taps, unsigned grid, void *stream)
{
    if (!owns(group, n)) return 0;
    std::string s;
    char buf[512];
    for (int k = 0; k < sg::MULTI_MAX_K; ++k) {
        snprintf(buf, sizeof(buf), " [%d]{out=%s edges=%s dt_inv=%a centre_sum=%a flags=0x%x taps=%016" PRIx64 "}", k, P(j->out[k]), P(j->edges[k]),
                 (double)j->dt_inv[k], (double)j->centre_sum[k], j->flags[k], digest(&taps->t[k], sizeof(taps->t[k])));
        s += buf;
    }
    logf("%s n=%d grid=%u stream=%p nraw=%u base{%s}%s", name, n, grid, stream, j->nraw, job1d(j->base).c_str(), s.c_str());
    return 1;
}

int h16(const char *name, int group, int n, const sg::JobH16 *j, const sg::Taps *taps, unsigned grid, void *stream)
{
    if (!owns(group, n)) return 0;
    logf("%s n=%d grid=%u stream=%p taps=%016" PRIx64 " in_type=%u out_type=%u base{%s}", name, n, grid, stream, digest(taps, sizeof(*taps)), j->in_type,
         j->out_type, job1d(j->base).c_str());
    return 1;
}

const char *copy_kind(hipMemcpyKind k)
{
    return k == hipMemcpyHostToDevice ? "H2D" : k == hipMemcpyDeviceToHost ? "D2H" : k == hipMemcpyDeviceToDevice ? "D2D" : k == hipMemcpyHostToHost ? "H2H" : "default";
}

}  // namespace

// ---- the test's handles ----
extern "C" {
void rec_reset(void)
{
    g_log.clear();
    g_error[0] = 0;
    g_bases.clear();
    g_scratch.clear();
    g_scratch_top = SCRATCH_BASE;
}
void rec_add_base(const char *name, uintptr_t address, uintptr_t bytes) { g_bases.push_back({name, address, bytes}); }
const char *rec_log(void) { return g_log.c_str(); }
void rec_note(const char *text) { logf("%s", text); }
void rec_set_small(int taken) { g_small_taken = taken; }
void rec_clear_error(void) { g_error[0] = 0; }
void rec_clear_bases(void) { g_bases.clear(); }
}

// ---- error text (sg_runtime.cpp in the product) ----
extern "C" void sg_set_error(const char *fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_error, sizeof(g_error), fmt, ap);
    va_end(ap);
}
extern "C" const char *savgol_hip_last_error(void) { return g_error; }

// ---- sg:: runtime ----
namespace sg {

DeviceCtx *ctx_get()
{
    static DeviceCtx ctx;
    ctx.ordinal = 0;
    ctx.cu_count = 256;
    return &ctx;
}

// an address derived from (salt, content): the same table has the same name whichever call asks for it first
const float *ctx_table(DeviceCtx *, const void *host, size_t bytes, uint64_t salt)
{
    const uint64_t d = digest(host, bytes);
    const uintptr_t a = (uintptr_t)0x700000000000ull + (uintptr_t)(((d ^ (salt * 0x9E3779B97F4A7C15ull)) & 0xffffffffffull) << 4);
    char buf[96];
    snprintf(buf, sizeof(buf), "table(0x%" PRIx64 ",%016" PRIx64 ",%zu)", salt, d, bytes);
    g_tables[a] = buf;
    return reinterpret_cast<const float *>(a);
}

void *ctx_arena(DeviceCtx *, size_t bytes)
{
    logf("ctx_arena bytes=%zu", bytes);
    return reinterpret_cast<void *>(ARENA_BASE);
}

void *ctx_pinned(DeviceCtx *, size_t bytes)
{
    logf("ctx_pinned bytes=%zu", bytes);
    if (g_pinned.size() < bytes) g_pinned.assign(bytes, 0);
    return g_pinned.data();
}

uint64_t scratch_keep_bytes() { return (uint64_t)256 << 20; }

void *scratch_alloc(DeviceCtx *, size_t bytes, hipStream_t st, const char *what)
{
    char name[32];
    snprintf(name, sizeof(name), "scratch#%zu", g_scratch.size());
    logf("scratch_alloc -> %s bytes=%zu stream=%p what=\"%s\"", name, bytes, (void *)st, what);
    const uintptr_t a = g_scratch_top;
    g_scratch_top += (bytes + 255) / 256 * 256 + 256;
    g_scratch.push_back({name, a, bytes ? bytes : 1});
    return reinterpret_cast<void *>(a);
}

bool scratch_free(void *p, hipStream_t st, const char *what)
{
    logf("scratch_free %s stream=%p what=\"%s\"", P(p), (void *)st, what);
    return true;
}

bool hip_ok(hipError_t e, const char *what)
{
    if (e == hipSuccess) return true;
    sg_set_error("%s: %s", what, hipGetErrorString(e));
    return false;
}

}  // namespace sg

// ---- HIP runtime: nothing is copied (the addresses are names, not memory), everything succeeds ----
extern "C" {
hipError_t hipGetLastError(void) { return hipSuccess; }
const char *hipGetErrorString(hipError_t) { return "mock"; }
hipError_t hipMemcpyAsync(void *dst, const void *src, size_t bytes, hipMemcpyKind kind, hipStream_t st)
{
    logf("hipMemcpyAsync dst=%s src=%s bytes=%zu kind=%s stream=%p", P(dst), P(src), bytes, copy_kind(kind), (void *)st);
    return hipSuccess;
}
hipError_t hipMemcpy(void *dst, const void *src, size_t bytes, hipMemcpyKind kind)
{
    logf("hipMemcpy dst=%s src=%s bytes=%zu kind=%s", P(dst), P(src), bytes, copy_kind(kind));
    return hipSuccess;
}
hipError_t hipMemcpy2DAsync(void *dst, size_t dpitch, const void *src, size_t spitch, size_t width, size_t height, hipMemcpyKind kind, hipStream_t st)
{
    logf("hipMemcpy2DAsync dst=%s dpitch=%zu src=%s spitch=%zu width=%zu height=%zu kind=%s stream=%p", P(dst), dpitch, P(src), spitch, width, height,
         copy_kind(kind), (void *)st);
    return hipSuccess;
}
hipError_t hipStreamSynchronize(hipStream_t st) { logf("hipStreamSynchronize stream=%p", (void *)st); return hipSuccess; }
// only the pipelined host path (>= 2^23 samples) uses these; the record does not cover it
hipError_t hipSetDevice(int d) { logf("hipSetDevice %d", d); return hipSuccess; }
hipError_t hipStreamCreateWithFlags(hipStream_t *st, unsigned flags) { logf("hipStreamCreateWithFlags flags=%u", flags); *st = nullptr; return hipSuccess; }
hipError_t hipEventCreateWithFlags(hipEvent_t *e, unsigned flags) { logf("hipEventCreateWithFlags flags=%u", flags); *e = nullptr; return hipSuccess; }
hipError_t hipEventDestroy(hipEvent_t) { logf("hipEventDestroy"); return hipSuccess; }
hipError_t hipEventRecord(hipEvent_t, hipStream_t st) { logf("hipEventRecord stream=%p", (void *)st); return hipSuccess; }
hipError_t hipStreamWaitEvent(hipStream_t st, hipEvent_t, unsigned flags) { logf("hipStreamWaitEvent stream=%p flags=%u", (void *)st, flags); return hipSuccess; }
}

// ---- the launchers ----
extern "C" {
#define CENTER(T, G) \
    int sg1d_launch_##T##_g##G(int n, int wide, const sg::Job1D *job, const sg::Taps *taps, unsigned grid, void *stream) \
    { return center(#T "_g" #G, G, n, wide, job, taps, grid, stream); }
CENTER(f32, 0) CENTER(f32, 1) CENTER(f32, 2) CENTER(f32, 3) CENTER(f64, 0) CENTER(f64, 1) CENTER(f64, 2) CENTER(f64, 3)
#define STRIDED(G) \
    int sg1d_launch_strided_f32_g##G(int n, const sg::JobStrided *job, const sg::Taps *taps, unsigned grid, void *stream) \
    { return strided("strided_f32_g" #G, G, n, job, taps, grid, stream); }
STRIDED(0) STRIDED(1) STRIDED(2) STRIDED(3)
#define MULTI(K, G) \
    int sg1d_launch_multi##K##_g##G(int n, const sg::JobMulti1D *job, const sg::TapsMulti *taps, unsigned grid, void *stream) \
    { return multi("multi" #K "_g" #G, G, n, job, taps, grid, stream); }
MULTI(2, 0) MULTI(2, 1) MULTI(2, 2) MULTI(2, 3) MULTI(3, 0) MULTI(3, 1) MULTI(3, 2) MULTI(3, 3)
#define H16(G) \
    int sg1d_launch_h16_g##G(int n, const sg::JobH16 *job, const sg::Taps *taps, unsigned grid, void *stream) \
    { return h16("h16_g" #G, G, n, job, taps, grid, stream); }
H16(0) H16(1) H16(2) H16(3)

// the block-moment launchers: 0 = enqueued
#define MOMENT(NAME, TABLE_T) \
    int sg1d_launch_##NAME(int n, const sg::Job1D *job, const TABLE_T *d_table, unsigned grid, void *stream) \
    { logf(#NAME " n=%d grid=%u stream=%p table=%s job{%s}", n, grid, stream, P(d_table), job1d(*job).c_str()); return 0; }
MOMENT(f32_momenth_t3, float) MOMENT(f32_momenth_t5, float) MOMENT(f32_momenth_t7, float)
MOMENT(f64_moment_t3, double) MOMENT(f64_moment_t5, double) MOMENT(f64_moment_t7, double)
#define H16_MOMENT(T) \
    int sg1d_launch_h16_momenth_t##T(int n, const sg::JobH16 *j, const float *d_table, unsigned grid, void *stream) \
    { logf("h16_momenth_t" #T " n=%d grid=%u stream=%p table=%s in_type=%u out_type=%u base{%s}", n, grid, stream, P(d_table), j->in_type, j->out_type, \
           job1d(j->base).c_str()); return 0; }
H16_MOMENT(3) H16_MOMENT(5) H16_MOMENT(7)

int sg1d_launch_ends(const void *in, long long in_ld, unsigned length, unsigned tiles_per_channel, int TW, int NA, int mode, void *stash, void *ends, void *edge_stash,
                     int ws, size_t channels, int elem_bytes, void *stream)
{
    logf("ends in=%s in_ld=%lld length=%u tiles_per_channel=%u TW=%d NA=%d mode=%d stash=%s ends=%s edge_stash=%s ws=%d channels=%zu elem_bytes=%d stream=%p", P(in),
         in_ld, length, tiles_per_channel, TW, NA, mode, P(stash), P(ends), P(edge_stash), ws, channels, elem_bytes, stream);
    return 0;
}

int sg1d_launch_reference_order_f32(const float *in, float *out, long long in_ld, long long out_ld, long long L, int n, const float *d_table, float dt_inv, int mode,
                                    int store_lo, int store_hi, int out_shift, int negate_leading, size_t channels, void *stream)
{
    logf("reference_order_f32 in=%s out=%s in_ld=%lld out_ld=%lld L=%lld n=%d table=%s dt_inv=%a mode=%d store_lo=%d store_hi=%d out_shift=%d negate_leading=%d "
         "channels=%zu stream=%p", P(in), P(out), in_ld, out_ld, L, n, P(d_table), (double)dt_inv, mode, store_lo, store_hi, out_shift, negate_leading, channels, stream);
    return 0;
}

// `center` is a HOST pointer into the caller's filter: logged by content
int sg1d_launch_refpk_f32(const float *in, float *out, long long in_ld, long long out_ld, long long length, int n, const float *center_weights, float dt_inv, int mode,
                          int store_lo, int store_hi, int out_shift, size_t channels, int cu_count, void *stream)
{
    logf("refpk_f32 in=%s out=%s in_ld=%lld out_ld=%lld length=%lld n=%d center=%016" PRIx64 " dt_inv=%a mode=%d store_lo=%d store_hi=%d out_shift=%d channels=%zu "
         "cu_count=%d stream=%p", P(in), P(out), in_ld, out_ld, length, n, digest(center_weights, sizeof(float) * (2 * (size_t)n + 1)), (double)dt_inv, mode, store_lo,
         store_hi, out_shift, channels, cu_count, stream);
    return 0;
}

int sg_launch_gather_f32(const void *base, size_t stride, size_t offset, size_t pitch, float *dst, size_t dst_ld, size_t channels, size_t count, void *st)
{
    logf("gather_f32 base=%s stride=%zu offset=%zu pitch=%zu dst=%s dst_ld=%zu channels=%zu count=%zu stream=%p", P(base), stride, offset, pitch, P(dst), dst_ld,
         channels, count, st);
    return 0;
}

int sg_launch_scatter_f32(const float *src, size_t src_ld, void *base, size_t stride, size_t offset, size_t pitch, size_t channels, size_t count, void *st)
{
    logf("scatter_f32 src=%s src_ld=%zu base=%s stride=%zu offset=%zu pitch=%zu channels=%zu count=%zu stream=%p", P(src), src_ld, P(base), stride, offset, pitch,
         channels, count, st);
    return 0;
}

// the resident small-call service: 0 = taken (`output` would hold the result), 1 = not taken; the test sets which (rec_set_small)
int sg_small_call(void *, const float *d_table, const float *input, float *output, int L, int n, int mode, int store_lo, int store_hi, int out_shift, int negate,
                  float dt_inv)
{
    logf("small_call table=%s input=%s output=%s L=%d n=%d mode=%d store_lo=%d store_hi=%d out_shift=%d negate=%d dt_inv=%a -> %s", P(d_table), P(input), P(output), L,
         n, mode, store_lo, store_hi, out_shift, negate, (double)dt_inv, g_small_taken ? "taken" : "not taken");
    return g_small_taken ? 0 : 1;
}
}
