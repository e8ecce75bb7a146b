// sg_stream_dma_multi.hip -- savgol_streambank_push_block_multi, the body of a fused call: LDS-DMA tiles on fp32 rows with K outputs from one read of the samples.
//
// A body tile (bands >= 2 of a call: every row is one of the call's own rows, 2n <= 64, and every tick has an output) with its own text, because its rows
// travel differently from the 16-bit body tile's (sg_stream_dma_body.inc; DESIGN 4.3e says why one body over both did not ship):
//   * a tile is the fp32 call's tile of the same band and strip -- 128 streams x 32 ticks, the twins' tile order, 1 KiB row pairs (two 512-byte rows per
//     DMA, an 8-byte LDS read per lane) -- so the samples cross HBM -> LDS once for K banks: 4 + 4 K bytes per stream-tick instead of 8 K;
//   * every arriving row is read once from the slab and fed into output k's accumulators with bank k's taps, through the fragment every stream tile's
//     `feed` is made of (sg_stream_dma_feed.hpp, included once per output): output k's bits are its twin's by construction;
//   * fused bank: the sum of the tile's first eight rows is taken once out of LDS; output k runs on x - cen_k, cen_k = that centre where bank k's
//     filter is a derivative (job.centre[k]), else 0 -- a smoothing bank and a derivative bank share a launch;
//   * a finished output row issues K stores: DmaQueue's stores-per-row parameter (sg_stream_host.hpp; tests/mock/dma_queue_multi.cpp);
//   * rows past the call's last tick (the last band) take the last row's address and finish no output.
// Launched through launch_body_tiles (sg_stream_dma_body.hpp), like the 16-bit body tiles.  Only bands >= 2 come here (block_plan_multi, sg_stream_host.hpp).
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstring>

#include "sg_internal.h"
#include "sg_pk.hpp"
#include "sg_runtime.hpp"
#include "sg_stream_dma.hpp"
#include "sg_stream_dma_body.hpp"
#include "sg_stream_multi.hpp"
#include "sg_stream_roll.hpp"

namespace sg {

#ifndef SG_MULTI_FMA
#define SG_MULTI_FMA 1
#endif

template <int N, int K> struct MultiTaps { SRollTaps<N> t[K]; };

// DP: the ring, in DMAs = KiB = two rows each
template <int N, bool FMA, int K, int TRT, int WPB, int DP, int FCH = 2>
__global__ __launch_bounds__(64 * WPB) void sg_bank_dma_multi_kernel(const BankJobMulti job, const MultiTaps<N, K> all, const TileGeom geo)
{
    typedef DmaShape<N, TRT> D;
    typedef DmaQueue<N, TRT, DP, 2, K> Q;
    constexpr int TR = D::TR, NI = D::NI, RB = D::RB, RING = DP * 1024;
    constexpr int MOM = 0;
    static_assert(DP >= 4 && DP <= NI, "ring of row pairs; the first eight rows are in it together");
    static_assert(2 * N <= 64, "the head (two bands) covers every row a body tile reaches back to");
    static_assert(K >= 2 && K <= STREAM_MULTI_PER_LAUNCH, "outputs per launch");
    extern __shared__ __attribute__((aligned(1024))) char lds[];
    const int lane = threadIdx.x & 63;
    const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const TileAt at = tile_of(geo, xcd_block(false) * WPB + (unsigned)wv);
    if (!at.ok) return;
    const unsigned strip = at.strip;
    const long long t0 = (long long)(at.band + job.band0) * TR;                                   // >= 2N: row 0 of the slab is tick t0 - 2N >= 0 of this call
    const unsigned ring = (unsigned)(uintptr_t)((__attribute__((address_space(3))) char *)lds) + (unsigned)wv * (unsigned)RING;   // LDS byte address, wave-uniform
    const int sub = lane >> 5, chunk = lane & 31;                                                 // row of the pair, 16-byte chunk of the row
    const size_t col = (size_t)strip * 128 + (size_t)chunk * 4;

    // source of row pair i: slab row r = tick t0 - 2N + r; rows past the call's last tick (the last band) take the last row's address
    const long long last = (long long)job.ticks - 1;
    const bool inside = t0 + TR <= (long long)job.ticks;                                          // uniform
    const float *const p0 = job.samples + (size_t)(t0 - 2 * N + (inside ? sub : 0)) * job.streams + col;
    const size_t pstep = 2 * job.streams;
    auto issue = [&](auto ic) {
        constexpr int i = decltype(ic)::value;
        const float *src;
        if (inside) {
            src = p0 + (size_t)i * pstep;
        } else {
            long long h = t0 - 2 * N + 2 * i + sub;
            h = h > last ? last : h;
            src = job.samples + (size_t)h * job.streams + col;
        }
        dma16(src, ring + (unsigned)(i % DP) * 1024u);
    };
    static_for<DP>([&](auto ic) -> bool { issue(ic); return true; });

    // ---- consume the rows in arrival order ----
    const char *mine = lds + (size_t)wv * RING + lane * 8;
    const int row_bytes = (int)(job.streams * 4);
    const unsigned voff = (strip * 128u + 2u * (unsigned)lane) * 4u;                              // byte offset of this lane's streams in a row
    constexpr int CH = FMA ? FCH : 1;
    f32x2 accs[K][CH][TR];
    f32x2 cens[K], backdts[K];
    static_for<K>([&](auto kc) -> bool { cens[decltype(kc)::value] = f32x2{0.0f, 0.0f}; backdts[decltype(kc)::value] = f32x2{0.0f, 0.0f}; return true; });
    auto row_in = [&](auto rc) -> f32x2 {
        constexpr int r = decltype(rc)::value;
        return *reinterpret_cast<const f32x2 *>(mine + ((r / 2) % DP) * 1024 + (r & 1) * RB);
    };
    // one arriving row into output k: the fp32 kernel's `feed`, bound to bank k's accumulators, taps and (centred) sample pair
    auto feed = [&](auto kc, auto rc, const f32x2 x) {
        constexpr int k = decltype(kc)::value, r = decltype(rc)::value;
        f32x2 (&acc)[CH][TR] = accs[k];
        const SRollTaps<N> &taps = all.t[k];
        f32x2 mom[1];
        (void)mom;
#include "sg_stream_dma_feed.hpp"
        if constexpr (r >= 2 * N && r - 2 * N < TR) {                                             // output m = r - 2N has seen its last row
            constexpr int m = r - 2 * N;
            f32x2 a = acc[0][m];
            if constexpr (CH == 2) a = a + acc[1][m];

            const long long tt = t0 + m;
            const bool has_out = tt <= last;                                                      // uniform
            // the fp32 kernel's output step, word for word: the chains' sum; fused bank: (a + c * sum_k w_k) * dt_inv in one multiply-add
            const f32x2 y = (MOM > 0 || FMA) ? __builtin_elementwise_fma(a, f32x2{job.dt_inv[k], job.dt_inv[k]}, backdts[k]) : a * f32x2{job.dt_inv[k], job.dt_inv[k]};
            float *orow = job.out[k] + (size_t)(has_out ? tt : 0) * job.streams;
            const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(orow, 0, has_out ? row_bytes : 0, 0x00020000);
            __builtin_amdgcn_raw_buffer_store_b64(__builtin_bit_cast(u32x2, y), rs, (int)voff, 0, 2);   // nontemporal, as the fp32 tile's
        }
    };
    // the centre of the centred outputs: the sum of the tile's first eight rows (all real samples here), once, out of LDS after four DMAs have landed
    if constexpr (FMA) {
        bool any = false;                                    // uniform
        static_for<K>([&](auto kc) -> bool { any = any || job.centre[decltype(kc)::value] != 0; return true; });
        if (any) {
            f32x2 sum = f32x2{0.0f, 0.0f};
            wait_vm<(Q::younger(3, 0) > 63 ? 63 : Q::younger(3, 0))>();
            static_for<8>([&](auto rc) -> bool { sum = sum + row_in(rc); return true; });
            const f32x2 cen = centre_guard(sum);
            static_for<K>([&](auto kc) -> bool {
                constexpr int k = decltype(kc)::value;
                if (job.centre[k]) {                         // uniform; smoothing banks keep cen_k = 0
                    cens[k] = cen;
                    backdts[k] = cen * f32x2{job.centre_sum[k] * job.dt_inv[k], job.centre_sum[k] * job.dt_inv[k]};
                }
                return true;
            });
        }
    }
    wait_vm<(Q::younger(0, 0) > 63 ? 63 : Q::younger(0, 0))>();
    f32x2 xa = row_in(std::integral_constant<int, 0>{}), xb = row_in(std::integral_constant<int, 1>{});
    // Step g consumes pair g (already in xa, xb) for every output, after it has waited for pair g + 1 and issued its LDS reads, and ends by issuing DMA
    // g + DP into the ring slot pair g has just left.  A row without an output still issues its K stores (into empty descriptors): the queue is static.
    static_for<NI>([&](auto gc) -> bool {
        constexpr int g = decltype(gc)::value;
        f32x2 na = xa, nb = xb;
        if constexpr (g + 1 < NI) {
            wait_vm<(Q::younger(g + 1, g) > 63 ? 63 : Q::younger(g + 1, g))>();
            na = row_in(std::integral_constant<int, 2 * g + 2>{});
            nb = row_in(std::integral_constant<int, 2 * g + 3>{});
            __builtin_amdgcn_sched_barrier(0);                                                    // keep these reads AHEAD of pair g's arithmetic
        }
        auto take = [&](auto rc, const f32x2 raw) {
            static_for<K>([&](auto kc) -> bool {
                if constexpr (FMA) feed(kc, rc, raw - cens[decltype(kc)::value]);
                else feed(kc, rc, raw);
                return true;
            });
        };
        take(std::integral_constant<int, 2 * g>{}, xa);
        take(std::integral_constant<int, 2 * g + 1>{}, xb);
        if constexpr (g + DP < NI) {
            // pair g's slot is free once its LDS reads have returned: drain the LDS queue before the DMA may overwrite the slot
            __builtin_amdgcn_sched_barrier(0);
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            issue(std::integral_constant<int, g + DP>{});
        }
        xa = na; xb = nb;
        return true;
    });
}

// One launch of the body's tiles for K outputs; 1 = the runtime refused it
template <int N, bool FMA, int K, int WPB, int DPR>
static int launch_bank_dma_multi(const float *const *center, const BankJobMulti &job, const MultiPlan &plan, hipStream_t st)
{
    constexpr int DP = DPR < DmaShape<N, 32>::NI ? DPR : DmaShape<N, 32>::NI;                     // ring of row pairs, clamped to the tile
    if (plan.wpb != WPB) return 1;                                                                // the grid was laid out for another block shape
    MultiTaps<N, K> taps;
    memset(&taps, 0, sizeof(taps));
    for (int k = 0; k < K; ++k) pack_taps(center[k], SRoll<N>::WS, taps.t[k].w);
    return launch_body_tiles<WPB, DP>(sg_bank_dma_multi_kernel<N, FMA, K, 32, WPB, DP>, job, taps, plan.geo, plan.grid, st);
}

// (waves per block, ring pairs) by half window, bank and output count: multi_tile_shape (sg_stream_host.hpp) as template arguments
template <int N, bool FMA, int K>
static int launch_bank_dma_multi_shape(const float *const *center, const BankJobMulti &job, const MultiPlan &plan, hipStream_t st)
{
    constexpr MultiTileShape s = multi_tile_shape(N, FMA, K);
    return launch_bank_dma_multi<N, FMA, K, s.wpb, s.dp>(center, job, plan, st);
}

template <int N, bool FMA>
static int dispatch_bank_dma_multi(int n, int outputs, const float *const *center, const BankJobMulti &job, const MultiPlan &plan, hipStream_t st)
{
    if (n == N) {
        if constexpr (N <= stream_multi_max_n(FMA, 2)) { if (outputs == 2) return launch_bank_dma_multi_shape<N, FMA, 2>(center, job, plan, st); }
        if constexpr (N <= stream_multi_max_n(FMA, 3)) { if (outputs == 3) return launch_bank_dma_multi_shape<N, FMA, 3>(center, job, plan, st); }
        return 1;
    }
    constexpr int top = stream_multi_max_n(FMA, 2) > stream_multi_max_n(FMA, 3) ? stream_multi_max_n(FMA, 2) : stream_multi_max_n(FMA, 3);
    if constexpr (N < top) return dispatch_bank_dma_multi<N + 1, FMA>(n, outputs, center, job, plan, st);
    else return 1;
}

// the Makefile builds two objects, one per bank kind, so that they compile side by side
#if SG_MULTI_FMA
int sg_bank_dma_multi_launch_fma(int n, int outputs, const float *const *center, const BankJobMulti &job, const MultiPlan &plan, hipStream_t st)
{
    return n < 1 ? 1 : dispatch_bank_dma_multi<1, true>(n, outputs, center, job, plan, st);
}
#else
int sg_bank_dma_multi_launch_ref(int n, int outputs, const float *const *center, const BankJobMulti &job, const MultiPlan &plan, hipStream_t st)
{
    return n < 1 ? 1 : dispatch_bank_dma_multi<1, false>(n, outputs, center, job, plan, st);
}
#endif

}  // namespace sg
