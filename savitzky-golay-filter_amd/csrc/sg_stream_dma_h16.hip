// sg_stream_dma_h16.hip -- savgol_streambank_push_block_h16, the body of the tile route: LDS-DMA tiles on fp16 / bf16 rows.
//
// sg_bank_dma_kernel (sg_stream_dma.hip) with 16-bit rows on both ends and its own arithmetic in between (sg_stream_dma_feed.hpp, the fragment both `feed` lambdas are made of):
//   * a tile is the fp32 call's tile of the same band and strip -- 128 streams x 32 ticks, the twin's tile order -- so a row is 256 bytes and one
//     global_load_lds_dwordx4 moves FOUR rows (lane l: row l >> 4, 16-byte chunk l & 15): half the DMA requests for the same rows;
//   * a lane takes its two streams out of the slab with ONE 4-byte LDS read and widens them exactly (bf16: a shift and a mask; fp16: the hardware convert);
//   * ROWS = 32 + 2n is rounded up to whole DMAs (odd n: two pad rows, loaded from a clamped, valid address and never fed);
//   * 16 -> 16 bit: the output pair is rounded once to nearest even, packed into one dword and stored through a range-checked descriptor of
//     streams x 2 bytes, nontemporal like the fp32 store; 16 bit -> fp32 keeps the fp32 kernel's store.
// Only bands >= 2 of a call come here (block_plan_h16, sg_stream_host.hpp): every row is one of the call's own 16-bit rows and every tick has an output.
// A centred tile (fused bank, derivative filters) therefore always takes the sum of its first eight rows out of LDS, the fp32 tile's own rule.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstring>

#include "sg_h16.hpp"
#include "sg_internal.h"
#include "sg_pk.hpp"
#include "sg_runtime.hpp"
#include "sg_stream_dma.hpp"
#include "sg_stream_h16.hpp"
#include "sg_stream_roll.hpp"

namespace sg {

#ifndef SG_DMA_MAX_N
#define SG_DMA_MAX_N 32
#endif

// DP: the ring, in DMAs = KiB = four rows each
template <int N, bool FMA, int TRT, int WPB, int DP, int FCH = 2, int MOM = 0, class TAPS = SRollTaps<N>>
__global__ __launch_bounds__(64 * WPB) void sg_bank_dma_h16_kernel(const BankJobH16 job, const TAPS taps, const TileGeom geo)
{
    typedef DmaQueue<N, TRT, DP, 4> Q;
    constexpr int TR = TRT, ROWS = TR + 2 * N, NI = Q::NI, RB = 256, RING = DP * 1024;
    static_assert(DP >= 2 && DP <= NI, "ring of row quads; the first eight rows are in it together");
    static_assert(2 * N <= 64, "the head (two bands) covers every row a body tile reaches back to");
    extern __shared__ __attribute__((aligned(1024))) char lds[];
    const int lane = threadIdx.x & 63;
    const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const TileAt at = tile_of(geo, xcd_block(false) * WPB + (unsigned)wv);
    if (!at.ok) return;
    const unsigned strip = at.strip;
    const long long t0 = (long long)(at.band + job.band0) * TR;                                   // >= 2N: row 0 of the slab is tick t0 - 2N >= 0 of this call
    const unsigned ring = (unsigned)(uintptr_t)((__attribute__((address_space(3))) char *)lds) + (unsigned)wv * (unsigned)RING;   // LDS byte address, wave-uniform
    const int sub = lane >> 4, chunk = lane & 15;                                                 // row of the quad, 16-byte chunk (8 streams) of the row
    const size_t col = (size_t)strip * 128 + (size_t)chunk * 8;
    const bool ibf = job.in_type == H16_STORE_BF16, obf = job.out_type == H16_STORE_BF16, of32 = job.out_type == H16_STORE_F32;   // uniform

    f32x2 cen = f32x2{0.0f, 0.0f}, backdt = f32x2{0.0f, 0.0f};
    // source of row quad i: slab row r = tick t0 - 2N + r; rows past the call's last tick (the last band, pad rows) take the last row's address
    const long long last = (long long)job.ticks - 1;
    const bool inside = t0 - 2 * N + 4 * NI <= (long long)job.ticks;                              // uniform
    const unsigned short *const p0 = job.samples + (size_t)(t0 - 2 * N + (inside ? sub : 0)) * job.streams + col;
    const size_t pstep = 4 * job.streams;
    auto issue = [&](auto ic) {
        constexpr int i = decltype(ic)::value;
        const unsigned short *src;
        if (inside) {
            src = p0 + (size_t)i * pstep;
        } else {
            long long h = t0 - 2 * N + 4 * i + sub;
            h = h > last ? last : h;
            src = job.samples + (size_t)h * job.streams + col;
        }
        dma16(reinterpret_cast<const float *>(src), ring + (unsigned)(i % DP) * 1024u);
    };
    static_for<DP>([&](auto ic) -> bool { issue(ic); return true; });

    // ---- consume the rows in arrival order ----
    const char *mine = lds + (size_t)wv * RING + lane * 4;
    const unsigned voff = strip * 128u + 2u * (unsigned)lane;                                     // this lane's first stream
    constexpr int CH = MOM ? 1 : (FMA ? FCH : 1);
    f32x2 acc[CH][TR];
    f32x2 mom[MOM > 0 ? MOM : 1];
    auto row_in = [&](auto rc) -> unsigned {
        constexpr int r = decltype(rc)::value;
        return *reinterpret_cast<const unsigned *>(mine + ((r / 4) % DP) * 1024 + (r & 3) * RB);
    };
    auto feed = [&](auto rc, const f32x2 x) {
        constexpr int r = decltype(rc)::value;
#include "sg_stream_dma_feed.hpp"
        if constexpr (r >= 2 * N && r - 2 * N < TR) {                                             // output m = r - 2N has seen its last row
            constexpr int m = r - 2 * N;
            const long long tt = t0 + m;
            const bool has_out = tt <= last;                                                      // uniform
            // the fp32 kernel's output step, word for word: the chains' sum; fused bank: (a + c * sum_k w_k) * dt_inv in one multiply-add
            f32x2 a = acc[0][m];
            if constexpr (CH == 2) a = a + acc[1][m];
            const f32x2 y = (MOM > 0 || FMA) ? __builtin_elementwise_fma(a, f32x2{job.dt_inv, job.dt_inv}, backdt) : a * f32x2{job.dt_inv, job.dt_inv};
            const size_t orow = (size_t)(has_out ? tt : 0) * job.streams;
            // one store per output row whatever the type (the queue arithmetic is static); a row past the call stores into an empty descriptor
            if (of32) {
                const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(static_cast<float *>(job.out) + orow, 0, has_out ? (int)(job.streams * 4) : 0, 0x00020000);
                __builtin_amdgcn_raw_buffer_store_b64(__builtin_bit_cast(u32x2, y), rs, (int)(voff * 4u), 0, 2);
            } else {
                const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(static_cast<unsigned short *>(job.out) + orow, 0, has_out ? (int)(job.streams * 2) : 0, 0x00020000);
                __builtin_amdgcn_raw_buffer_store_b32(narrow2(y, obf), rs, (int)(voff * 2u), 0, 2);
            }
        }
    };
    // the centre of a centred tile: the sum of its first eight rows (all real samples here), out of LDS once the first two DMAs have landed
    if constexpr (MOM > 0 || FMA) {
        if (job.centre) {                                    // uniform; smoothing filters keep cen = 0
            f32x2 sum = f32x2{0.0f, 0.0f};
            wait_vm<(Q::younger(1, 0) > 63 ? 63 : Q::younger(1, 0))>();
            static_for<8>([&](auto rc) -> bool { sum = sum + widen2(row_in(rc), ibf); return true; });
            cen = centre_guard(sum);
            backdt = cen * f32x2{job.centre_sum * job.dt_inv, job.centre_sum * job.dt_inv};
        }
    }
    wait_vm<(Q::younger(0, 0) > 63 ? 63 : Q::younger(0, 0))>();
    unsigned x0 = row_in(std::integral_constant<int, 0>{}), x1 = row_in(std::integral_constant<int, 1>{}),
             x2 = row_in(std::integral_constant<int, 2>{}), x3 = row_in(std::integral_constant<int, 3>{});
    // Step g consumes quad g (already in x0..x3, still packed), after it has waited for quad g + 1 and issued its LDS reads, and ends by issuing DMA
    // g + DP into the ring slot quad g has just left.
    static_for<NI>([&](auto gc) -> bool {
        constexpr int g = decltype(gc)::value;
        unsigned n0 = x0, n1 = x1, n2 = x2, n3 = x3;
        if constexpr (g + 1 < NI) {
            wait_vm<(Q::younger(g + 1, g) > 63 ? 63 : Q::younger(g + 1, g))>();
            n0 = row_in(std::integral_constant<int, 4 * g + 4>{});
            n1 = row_in(std::integral_constant<int, 4 * g + 5>{});
            n2 = row_in(std::integral_constant<int, 4 * g + 6>{});
            n3 = row_in(std::integral_constant<int, 4 * g + 7>{});
            __builtin_amdgcn_sched_barrier(0);                                                    // keep these reads AHEAD of quad g's arithmetic
        }
        auto take = [&](auto rc, const unsigned raw) {
            constexpr int r = decltype(rc)::value;
            if constexpr (r < ROWS) {                                                             // pad rows are never fed
                if constexpr (MOM > 0 || FMA) feed(rc, widen2(raw, ibf) - cen);
                else feed(rc, widen2(raw, ibf));
            }
        };
        take(std::integral_constant<int, 4 * g>{}, x0);
        take(std::integral_constant<int, 4 * g + 1>{}, x1);
        take(std::integral_constant<int, 4 * g + 2>{}, x2);
        take(std::integral_constant<int, 4 * g + 3>{}, x3);
        if constexpr (g + DP < NI) {
            // quad g's slot is free once its LDS reads have returned: drain the LDS queue before the DMA may overwrite the slot
            __builtin_amdgcn_sched_barrier(0);
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            issue(std::integral_constant<int, g + DP>{});
        }
        x0 = n0; x1 = n1; x2 = n2; x3 = n3;
        return true;
    });
}

// One launch of the body's tiles (WPB waves per block, a ring of DP KiB per wave); 1 = the runtime refused it
template <int WPB, int DP, class Kernel, class Taps>
static int launch_dma_h16_tiles(Kernel kernel, const BankJobH16 &job, const Taps &taps, const TileGeom &geo, unsigned grid, hipStream_t st)
{
    constexpr size_t lds = (size_t)WPB * DP * 1024;
    static_assert(lds <= 64 * 1024, "the rings of one block fit the default dynamic LDS");
    hipLaunchKernelGGL(kernel, dim3(grid), dim3(64 * WPB), lds, st, job, taps, geo);
    return hipGetLastError() == hipSuccess ? 0 : 1;
}

template <int N> struct H16Rows { static constexpr int NI = (32 + 2 * N + 3) / 4; };

#ifndef SG_DMA_MOM_BUILD
template <int N, bool FMA, int WPB, int DPQ>
static int launch_bank_dma_h16(const float *center, const BankJobH16 &job, const TileGeom &geo, unsigned grid, hipStream_t st)
{
    SRollTaps<N> taps;
    memset(&taps, 0, sizeof(taps));
    pack_taps(center, SRoll<N>::WS, taps.w);
    constexpr int DP = DPQ < H16Rows<N>::NI ? DPQ : H16Rows<N>::NI;
    return launch_dma_h16_tiles<WPB, DP>(sg_bank_dma_h16_kernel<N, FMA, 32, WPB, DP>, job, taps, geo, grid, st);
}

// (waves per block, ring) by half window and bank: launch_bank_dma_shape's table (dma_tile_shape, sg_stream_host.hpp, restates the waves), the ring as
// deep in ROWS as the fp32 tiles' -- half the KiB
template <int N, bool FMA>
static int launch_bank_dma_h16_shape(const float *center, const BankJobH16 &job, const TileGeom &geo, unsigned grid, hipStream_t st)
{
    if constexpr (N <= 5) return launch_bank_dma_h16<N, FMA, 4, 8>(center, job, geo, grid, st);
    else if constexpr (N <= 11 && FMA) return launch_bank_dma_h16<N, FMA, 8, 6>(center, job, geo, grid, st);
    else if constexpr (N <= 10) return launch_bank_dma_h16<N, FMA, 4, 8>(center, job, geo, grid, st);
    return launch_bank_dma_h16<N, FMA, 4, 6>(center, job, geo, grid, st);
}

template <int N>
static int dispatch_bank_dma_h16(int n, int fma, const float *center, const BankJobH16 &job, const TileGeom &geo, unsigned grid, hipStream_t st)
{
    if (n == N) return fma ? launch_bank_dma_h16_shape<N, true>(center, job, geo, grid, st) : launch_bank_dma_h16_shape<N, false>(center, job, geo, grid, st);
    if constexpr (N < SG_DMA_MAX_N) return dispatch_bank_dma_h16<N + 1>(n, fma, center, job, geo, grid, st);
    else return 1;
}

#ifndef SG_DMA_MIN_N
#define SG_DMA_MIN_N 1
#endif
#ifndef SG_DMA_FN
#define SG_DMA_FN sg_bank_dma_h16_launch_all                 // the Makefile builds two objects (half windows 1..16 and 17..32) with a symbol each
#endif

int SG_DMA_FN(int n, int fma, const float *center, const BankJobH16 &job, const TileGeom &geo, unsigned grid, hipStream_t st)
{
    if (n < SG_DMA_MIN_N || n > SG_DMA_MAX_N) return 1;
    return dispatch_bank_dma_h16<SG_DMA_MIN_N>(n, fma, center, job, geo, grid, st);
}

#else      // SG_DMA_MOM_BUILD: the third object, block-moment tiles of the fused bank
template <int N, int M>
static int launch_bank_dma_h16_mom(const StreamMomentFit &fit, const float *center, const BankJobH16 &job, const TileGeom &geo, unsigned grid, hipStream_t st)
{
    constexpr int WPB = 8, DPQ = 8;                          // launch_bank_dma_mom's (8, 16 KiB): the same rows in flight
    typedef MomGeom<N> G;
    MomTaps<N, M> taps;
    memset(&taps, 0, sizeof(taps));
    pack_taps(center, 8, taps.head);
    pack_taps(center + 2 * N - 7, 8, taps.tail);
    for (int sm = 0; sm < M; ++sm) pack_taps(fit.c[sm], G::NOFF, taps.c[sm]);
    float q[2][8];
    for (int t = 0; t < 8; ++t) { q[0][t] = (float)t - 3.5f; q[1][t] = q[0][t] * q[0][t] - 5.25f; }
    for (int sm = 0; sm + 1 < M; ++sm) pack_taps(q[sm], 8, taps.q[sm]);
    constexpr int DP = DPQ < H16Rows<N>::NI ? DPQ : H16Rows<N>::NI;
    return launch_dma_h16_tiles<WPB, DP>(sg_bank_dma_h16_kernel<N, true, 32, WPB, DP, 1, M, MomTaps<N, M>>, job, taps, geo, grid, st);
}

template <int N>
static int dispatch_bank_dma_h16_mom(int n, const StreamMomentFit &fit, const float *center, const BankJobH16 &job, const TileGeom &geo, unsigned grid, hipStream_t st)
{
    if (n == N) {
        if (fit.terms == 1) return launch_bank_dma_h16_mom<N, 1>(fit, center, job, geo, grid, st);
        if (fit.terms == 2) return launch_bank_dma_h16_mom<N, 2>(fit, center, job, geo, grid, st);
        return launch_bank_dma_h16_mom<N, 3>(fit, center, job, geo, grid, st);
    }
    if constexpr (N < STREAM_MOMENT_MAX_N) return dispatch_bank_dma_h16_mom<N + 1>(n, fit, center, job, geo, grid, st);
    else return 1;
}

int sg_bank_dma_h16_launch_mom(int n, const StreamMomentFit &fit, const float *center, const BankJobH16 &job, const TileGeom &geo, unsigned grid, hipStream_t st)
{
    if (n < STREAM_MOMENT_MIN_N || n > STREAM_MOMENT_MAX_N) return 1;
    return dispatch_bank_dma_h16_mom<STREAM_MOMENT_MIN_N>(n, fit, center, job, geo, grid, st);
}

#endif

}  // namespace sg
