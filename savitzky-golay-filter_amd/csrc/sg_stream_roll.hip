// sg_stream_roll.hip -- savgol_streambank_push_block: rolling time windows in registers.
//
// A block push is a convolution down the time axis of a [tick][stream] array (history = ring contents, then this
// call's samples).  One WAVE owns 128 adjacent streams (a lane owns 2 = one 8-byte load per tick) and walks down a
// band of ticks.  No LDS, no __syncthreads, no re-reads except the 2n warm-up rows of a band.  Per output the
// arithmetic is the reference's (src/savgol_stream.c:166-185): one fp32 accumulator starting at 0, taps in ascending
// order, multiply and add rounded separately (v_pk_mul_f32 + v_pk_add_f32: two streams per instruction) ->
// bit-identical to savgol_stream_push for every stream.  Taps sit in SGPR pairs (by-value kernarg).
//   half windows <= 16: the last 2n+1 SAMPLES of the lane's streams live in a register ring that the fully unrolled
//                       tick loop indexes with literals; each tick is one 2n+1-term chain (bank_roll_item);
//   half windows 17-32: the unrolled ring would not fit the instruction cache, so the 2n in-flight ACCUMULATORS live
//                       in registers instead and every arriving sample advances all of them by one tap
//                       (bank_accroll_item; A/B at n <= 16: 15-30 % slower than the sample ring, so both stay).
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstring>
#include <type_traits>
#include <utility>

#include "sg_internal.h"
#include "sg_pk.hpp"
#include "sg_runtime.hpp"
#include "sg_stream.hpp"
#include "sg_stream_roll.hpp"

namespace sg {

// One item: streams s0, s0+1 of every lane, output ticks t0 .. t0+nt-1.  Row r of the band = history index
// t0 - 2N + r; output tick m needs rows m .. m+2N, row r lives in ring slot r % U.
// Fused bank, derivative filters (job.centre; spread_centre): what an item's rows are centred on, from the oldest real sample in the item's reach to
// its last row.  The bit-exact bank and smoothing filters: 0.
template <int N, bool VEC, bool FMA>
__device__ __forceinline__ f32x2 bank_item_centre(const BankJob &job, size_t s0, size_t t0, int nt, bool live0, bool live1)
{
    if constexpr (FMA) {
        if (job.centre) {                                    // uniform
            return centre_guard(spread_centre<SRoll<N>::WS>(job, (long long)t0 - 2 * N, (long long)t0 + nt - 1, [&](const float *row) -> f32x2 {
                if constexpr (VEC) return *reinterpret_cast<const f32x2 *>(row + s0);
                else return f32x2{live0 ? row[s0] : 0.0f, live1 ? row[s0 + 1] : 0.0f};
            }));
        }
    }
    return f32x2{0.0f, 0.0f};
}

// row r of an item (history index t0 - 2N + r), the lane's two streams, centred
template <int N, bool VEC>
__device__ __forceinline__ f32x2 bank_item_row(const BankJob &job, size_t s0, size_t t0, int r, bool live0, bool live1, const f32x2 cen)
{
    const float *row = history_row<SRoll<N>::WS>(job, (long long)t0 - 2 * N + r);
    if constexpr (VEC) return *reinterpret_cast<const f32x2 *>(row + s0) - cen;
    else return f32x2{live0 ? row[s0] : 0.0f, live1 ? row[s0 + 1] : 0.0f} - cen;
}

template <int N, bool VEC, bool FMA>
__device__ __forceinline__ void bank_roll_item(const BankJob &job, const SRollTaps<N> &taps, size_t s0, size_t t0, int nt)
{
    typedef SRoll<N> R;
    const bool live0 = s0 < job.streams, live1 = s0 + 1 < job.streams;
    const f32x2 cen = bank_item_centre<N, VEC, FMA>(job, s0, t0, nt, live0, live1);      // fused bank, derivative filters: what the item's rows are centred on (else 0)
    const f32x2 backdt = cen * f32x2{job.centre_sum * job.dt_inv, job.centre_sum * job.dt_inv};
    auto load_row = [&](int r) -> f32x2 { return bank_item_row<N, VEC>(job, s0, t0, r, live0, live1, cen); };
    f32x2 win[R::U];
#pragma unroll
    for (int r = 0; r < R::U - 1; ++r) win[r] = load_row(r);

    for (int base = 0; base < nt; base += R::U) {
        static_for(std::make_integer_sequence<int, R::U>{}, [&](auto uc) -> bool {
            constexpr int u = decltype(uc)::value;
            const int m = base + u;
            if (m >= nt) return false;                                           // uniform
            win[(u + R::U - 1) % R::U] = load_row(m + R::U - 1);                 // the slot row m-1 left
            // sum = 0; sum += w[k] * x[k], k ascending, separate roundings.  The product of tap k+1 is issued before
            // the add of tap k so that no instruction consumes the result of the one just before it.
            f32x2 acc = f32x2{0.0f, 0.0f};
            if constexpr (FMA) {
                // the fast form (SAVGOL_STREAMBANK_FMA): one v_pk_fma_f32 per tap instead of a multiply and an add -- half the
                // vector instructions.  Two chains (even taps, odd taps) so that no multiply-add waits for the one just before it;
                // not the reference's rounding (one rounding per term, two partial sums): within 1e-6 / 2e-6 of the fp64 oracle.
                f32x2 odd = pk_mul_sgpr<1>(taps.w[0], win[(u + 1) % R::U]);
                acc = pk_mul_sgpr<0>(taps.w[0], win[u % R::U]);
                static_for(std::make_integer_sequence<int, R::WS - 2>{}, [&](auto kc) -> bool {
                    constexpr int k = decltype(kc)::value + 2;
                    if constexpr (k & 1) pk_fma_sgpr<1>(odd, taps.w[k >> 1], win[(u + k) % R::U]);
                    else                 pk_fma_sgpr<0>(acc, taps.w[k >> 1], win[(u + k) % R::U]);
                    return true;
                });
                acc = acc + odd;
            } else {
            f32x2 p = pk_mul_sgpr<0>(taps.w[0], win[u % R::U]);
            static_for(std::make_integer_sequence<int, R::WS>{}, [&](auto kc) -> bool {
                constexpr int k = decltype(kc)::value;
                f32x2 pn = p;
                if constexpr (k + 1 < R::WS) pn = pk_mul_sgpr<((k + 1) & 1)>(taps.w[(k + 1) >> 1], win[(u + k + 1) % R::U]);
                acc = acc + p;
                p = pn;
                return true;
            });
            }
            const size_t t = t0 + (size_t)m;
            if (has_output<R::WS>(job, t)) {                                     // uniform
                const f32x2 y = FMA ? __builtin_elementwise_fma(acc, f32x2{job.dt_inv, job.dt_inv}, backdt) : acc * f32x2{job.dt_inv, job.dt_inv};
                float *orow = job.out + t * job.streams;
                if constexpr (VEC) __builtin_nontemporal_store(__builtin_bit_cast(u32x2, y), reinterpret_cast<u32x2 *>(orow + s0));   // written once (round 5: as the LDS-DMA tiles)
                else { if (live0) orow[s0] = y.x; if (live1) orow[s0 + 1] = y.y; }
            }
            return true;
        });
    }
}

// The same item, accumulator stationary (half windows above STREAM_RING_MAX_N, where the unrolled ring of the version
// above would not fit the instruction cache): 2N accumulator pairs instead of 2N+1 samples live in registers and every
// arriving sample advances all of them by one tap (ref_advance, sg_stream_roll.hpp; the fused bank: one multiply-add
// per slot) -- the tick loop is 2(2N+1) instructions, not unrolled.
template <int N, bool VEC, bool FMA>
__device__ __forceinline__ void bank_accroll_item(const BankJob &job, const SRollTaps<N> &taps, size_t s0, size_t t0, int nt)
{
    typedef SRoll<N> R;
    const bool live0 = s0 < job.streams, live1 = s0 + 1 < job.streams;
    const f32x2 cen = bank_item_centre<N, VEC, FMA>(job, s0, t0, nt, live0, live1);      // fused bank, derivative filters: what the item's rows are centred on (else 0)
    const f32x2 backdt = cen * f32x2{job.centre_sum * job.dt_inv, job.centre_sum * job.dt_inv};
    auto load_row = [&](int r) -> f32x2 { return bank_item_row<N, VEC>(job, s0, t0, r, live0, live1, cen); };
    f32x2 acc[R::WS];                                        // acc[a], a = 1..2N; garbage until a real output reaches it
#pragma unroll
    for (int a = 0; a < R::WS; ++a) acc[a] = f32x2{0.0f, 0.0f};
    // rows in flight: a ring of PA registers that the row loop, unrolled PA times, indexes with literals.  (Until late in round 3
    // this was `ahead[p] = ahead[p + 1]` in a loop that was not unrolled: a register MOVE of a row still in flight has to wait for it,
    // so every iteration ended in s_waitcnt vmcnt(0) and nothing was ever ahead -- which is why these kernels lost to the sample
    // ring by 30-45 % and why more rows "ahead" made them slower.)
    // The loop is unrolled UA rows deep (hipcc drains every memory operation at the back edge: once per UA rows).
    // (ring depth x resident blocks swept in tools/r3/exp32.sh: four rows at full occupancy; eight from n = 28, +7 % at n = 32)
    constexpr int PA = N >= 28 ? 8 : 4, UA = N <= 24 ? 16 : 8;
    static_assert(UA % PA == 0, "slot = row % PA must carry over from one group of UA rows to the next");
    f32x2 ahead[PA];
#pragma unroll
    for (int p = 0; p < PA; ++p) ahead[p] = load_row(p);
    const int nrows = nt + 2 * N;
    for (int r0 = 0; r0 < nrows; r0 += UA) {
      static_for<UA>([&](auto uc) -> bool {
        constexpr int u = decltype(uc)::value;
        const int r = r0 + u;
        if (r >= nrows) return false;                        // uniform
        const f32x2 x = ahead[u % PA];
        ahead[u % PA] = load_row(r + PA);
        // volatile asm, products and adds alike: left to the compiler the adds sink to the end of the iteration and all
        // 2N+1 products stay live (see sg_2d_dense.hip)
        f32x2 done;
        if constexpr (FMA) {
            static_for<R::WS>([&](auto ic) -> bool {
                constexpr int a = R::WS - 1 - decltype(ic)::value;   // slot = tap index, 2N down to 0
                // fast form: slot a+1 = tap a * x + slot a in ONE instruction (the chain of an output stays a single chain)
                if constexpr (a == 0) {
                    acc[1] = pk_mul_sgpr<0>(taps.w[0], x);
                } else if constexpr (a == R::WS - 1) {
                    done = acc[a];
                    pk_fma_sgpr<(a & 1)>(done, taps.w[a >> 1], x);
                } else {
                    // acc[a + 1] = fma(w[a], x, acc[a]); three-address form so that the walk from the top down needs no copy
                    if constexpr ((a & 1) == 0) asm volatile("v_pk_fma_f32 %0, %1, %2, %3 op_sel_hi:[0,1,1]" : "=v"(acc[a + 1]) : "s"(taps.w[a >> 1]), "v"(x), "v"(acc[a]));
                    else                        asm volatile("v_pk_fma_f32 %0, %1, %2, %3 op_sel:[1,0,0] op_sel_hi:[1,1,1]" : "=v"(acc[a + 1]) : "s"(taps.w[a >> 1]), "v"(x), "v"(acc[a]));
                }
                return true;
            });
        } else {
            done = ref_advance<N>(acc, taps, x);
        }
        const long long t = (long long)t0 + r - 2 * N;
        if (r >= 2 * N && has_output<R::WS>(job, (unsigned long long)t)) {                               // uniform
            const f32x2 y = FMA ? __builtin_elementwise_fma(done, f32x2{job.dt_inv, job.dt_inv}, backdt) : done * f32x2{job.dt_inv, job.dt_inv};
            float *orow = job.out + (size_t)t * job.streams;
            if constexpr (VEC) __builtin_nontemporal_store(__builtin_bit_cast(u32x2, y), reinterpret_cast<u32x2 *>(orow + s0));
            else { if (live0) orow[s0] = y.x; if (live1) orow[s0 + 1] = y.y; }
        }
        return true;
      });
    }
}

// ---- TILE form (round 4; half windows <= STREAM_RING_MAX_N, stream rows 16-byte aligned) ----
// The 2-D kernel's lesson (csrc/sg_2d_roll.hip, tools/membench_tile2d.hip): a walk down a strip -- a long-lived wave with a few rows in
// flight -- tops out at 0.63-0.71 of the roofline bare, short-lived waves that issue ALL their loads up front and exit reach 0.71-0.78.
// Here: a wave owns 256 adjacent streams (a lane 4 = one 16-byte load per tick row) and TR output ticks; it loads the TR + 2N rows
// (history from the ring, then this call's samples) back to back into registers, computes its TR rows with literal indices -- the same
// per-output arithmetic as bank_roll_item, bit for bit in both forms -- stores them and exits.  The 2N halo rows are read again by the
// tile of the next TR ticks: out of L2, because tiles are dealt so that blocks sharing an XCD walk down a GROUP of neighbouring strips
// band by band (a whole 256 KiB tick row of 65 536 streams would not stay in a 4 MiB L2 for the 256 tiles between two bands; a group of
// G strips x (TR + 2N) rows does).  Rows and stores go through range-checked buffer descriptors (streams beyond the bank read 0 and
// store nothing; a row without an output selects an empty descriptor), so there is no branch between the first load and the last store
// and hipcc's vmcnt waits stay counted.
// Tiles of 16 tick rows, 2 waves per block.
template <int N, bool FMA>
__global__ __launch_bounds__(64 * STREAM_TILE_WPB, 2) void sg_bank_tile_kernel(const BankJob job, const SRollTaps<N> taps, const TileGeom geo)
{
    typedef SRoll<N> R;
    constexpr int TR = STREAM_TILE_ROWS, ROWS = TR + 2 * N, NP = 2;        // NP: stream pairs of a lane's 16-byte quad
    const int lane = threadIdx.x & 63;
    const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const TileAt at = tile_of(geo, xcd_block(job.aligned & 2) * STREAM_TILE_WPB + (unsigned)wv);
    if (!at.ok) return;
    const unsigned band = at.band, strip = at.strip;
    const size_t t0 = (size_t)band * TR;
    const unsigned voff = (strip * 256u + 4u * (unsigned)lane) * 4u;      // byte offset of this lane's streams in a row
    const int row_bytes = (int)(job.streams * 4);

    struct Row { f32x2 p[NP]; };
    auto load_row = [&](int r) -> Row {
        const float *row = history_row<R::WS>(job, (long long)t0 - 2 * N + r);
        const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(const_cast<float *>(row), 0, row_bytes, 0x00020000);
        const f32x4 q = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rs, (int)voff, 0, 0));
        Row o;
        o.p[0] = f32x2{q.x, q.y}; o.p[1] = f32x2{q.z, q.w};
        return o;
    };
    Row win[ROWS];
#pragma unroll
    for (int r = 0; r < ROWS; ++r) win[r] = load_row(r);

    static_for<TR>([&](auto mc) -> bool {
        constexpr int m = decltype(mc)::value;
        f32x2 a[NP];
        if constexpr (FMA) {
            // two chains (even taps, odd taps), one v_pk_fma_f32 per tap and stream pair: bank_roll_item's fast form
            f32x2 o[NP];
#pragma unroll
            for (int c = 0; c < NP; ++c) { o[c] = pk_mul_sgpr<1>(taps.w[0], win[m + 1].p[c]); a[c] = pk_mul_sgpr<0>(taps.w[0], win[m].p[c]); }
            static_for(std::make_integer_sequence<int, R::WS - 2>{}, [&](auto kc) -> bool {
                constexpr int k = decltype(kc)::value + 2;
#pragma unroll
                for (int c = 0; c < NP; ++c) {
                    if constexpr (k & 1) pk_fma_sgpr<1>(o[c], taps.w[k >> 1], win[m + k].p[c]);
                    else                 pk_fma_sgpr<0>(a[c], taps.w[k >> 1], win[m + k].p[c]);
                }
                return true;
            });
#pragma unroll
            for (int c = 0; c < NP; ++c) a[c] = a[c] + o[c];
        } else {
            // the reference's order (src/savgol_stream.c:25-38): one accumulator from 0, taps ascending, multiply and add rounded separately
            f32x2 p[NP];
#pragma unroll
            for (int c = 0; c < NP; ++c) { a[c] = f32x2{0.0f, 0.0f}; p[c] = pk_mul_sgpr<0>(taps.w[0], win[m].p[c]); }
            static_for(std::make_integer_sequence<int, R::WS>{}, [&](auto kc) -> bool {
                constexpr int k = decltype(kc)::value;
#pragma unroll
                for (int c = 0; c < NP; ++c) {
                    f32x2 nx = p[c];
                    if constexpr (k + 1 < R::WS) nx = pk_mul_sgpr<((k + 1) & 1)>(taps.w[(k + 1) >> 1], win[m + k + 1].p[c]);
                    a[c] = a[c] + p[c];
                    p[c] = nx;
                }
                return true;
            });
        }
        const size_t tt = t0 + (size_t)m;
        const bool has_out = tt < job.ticks && has_output<R::WS>(job, tt);                               // uniform
        const f32x2 s = f32x2{job.dt_inv, job.dt_inv};
        float *orow = job.out + (tt < job.ticks ? tt : 0) * job.streams;
        const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(orow, 0, has_out ? row_bytes : 0, 0x00020000);
        const f32x2 y0 = a[0] * s, y1 = a[1] * s;
        __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, f32x4{y0.x, y0.y, y1.x, y1.y}), rs, (int)voff, 0, 0);
        return true;
    });
}

template <int N, bool FMA>
__global__ __launch_bounds__(256) void sg_bank_roll_kernel(const BankJob job, const SRollTaps<N> taps)
{
    const int lane = threadIdx.x & 63;
    const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    // persistent waves; the 4 waves of a block take adjacent strips (2 KB contiguous per tick row)
    const unsigned nblk = gridDim.x;
    const unsigned blk = xcd_block(job.aligned & 2);         // (launch_bank_roll always asks for launch order)
    const unsigned long long total = (unsigned long long)job.strips * job.bands;
    for (unsigned long long item = (unsigned long long)blk * 4u + (unsigned)wv; item < total; item += (unsigned long long)nblk * 4u) {
        const unsigned strip = (unsigned)(item % job.strips), band = (unsigned)(item / job.strips);
        const size_t s0 = (size_t)strip * 128 + 2 * (size_t)lane;
        const size_t t0 = (size_t)band * (size_t)job.band_ticks;
        const int nt = job.ticks - t0 < (size_t)job.band_ticks ? (int)(job.ticks - t0) : job.band_ticks;
        const bool vec = (job.aligned & 1) && (size_t)strip * 128 + 128 <= job.streams;
        if constexpr (N <= STREAM_RING_MAX_N) {
            if (vec) bank_roll_item<N, true, FMA>(job, taps, s0, t0, nt); else bank_roll_item<N, false, FMA>(job, taps, s0, t0, nt);
        } else {
            if (vec) bank_accroll_item<N, true, FMA>(job, taps, s0, t0, nt); else bank_accroll_item<N, false, FMA>(job, taps, s0, t0, nt);
        }
    }
}

// register tiles (half windows <= 12 of the bit-exact bank: block_form): groups of 64 strips -- (TR + 2N) rows x 64 KiB of a tick row stay well inside
// an XCD's 4 MiB L2 beside the rows in flight
template <int N>
static int dispatch_bank_tile(int n, const float *center, BankJob job, hipStream_t st)
{
    if (n == N) {
        SRollTaps<N> taps;
        memset(&taps, 0, sizeof(taps));
        pack_taps(center, SRoll<N>::WS, taps.w);
        TileGeom geo;
        const unsigned grid = tile_geom(job.streams, 256, job.ticks, STREAM_TILE_ROWS, 64, STREAM_TILE_WPB, &geo);
        if (!grid) return 1;
        job.aligned = 1;
        hipLaunchKernelGGL((sg_bank_tile_kernel<N, false>), dim3(grid), dim3(64 * STREAM_TILE_WPB), 0, st, job, taps, geo);
        return 0;
    }
    if constexpr (N < 12) return dispatch_bank_tile<N + 1>(n, center, job, st);
    else return 1;
}

template <int N, bool FMA>
static int launch_bank_roll(const float *center, BankJob job, int cu_count, hipStream_t st)
{
    SRollTaps<N> taps;
    memset(&taps, 0, sizeof(taps));
    pack_taps(center, SRoll<N>::WS, taps.w);
    static const int per_cu = [] {                           // resident blocks per CU of this instantiation
        int nb = 0;
        if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, sg_bank_roll_kernel<N, FMA>, 256, 0) != hipSuccess || nb < 1) nb = 2;
        if (nb > 4) nb = 4;
        if (FMA && N <= 16 && nb > 2) nb = 2;                // fewer waves, more rows in flight each (see SRoll::P)
        return nb;
    }();
    const unsigned nwaves = (unsigned)cu_count * (unsigned)per_cu * 4u;
    job.strips = (unsigned)((job.streams + 127) / 128);
    const size_t bands = walk_bands(job.ticks, job.strips, nwaves, N);
    job.band_ticks = (int)((job.ticks + bands - 1) / bands);
    job.bands = (unsigned)((job.ticks + (size_t)job.band_ticks - 1) / (size_t)job.band_ticks);
    const unsigned long long total = (unsigned long long)job.strips * job.bands;
    unsigned grid = (unsigned)cu_count * (unsigned)per_cu;
    if ((unsigned long long)grid * 4ull > total) grid = (unsigned)((total + 3) / 4);
    grid = (grid + 7u) & ~7u;
    job.aligned = (job.streams % 2 == 0 && ((reinterpret_cast<uintptr_t>(job.samples) | reinterpret_cast<uintptr_t>(job.out) |
                                              reinterpret_cast<uintptr_t>(job.ring)) & 7u) == 0) ? 1 : 0;
    job.aligned |= 2;                                        // the walk's items in launch order (the XCD order lost, R3)
    hipLaunchKernelGGL((sg_bank_roll_kernel<N, FMA>), dim3(grid), dim3(256), 0, st, job, taps);
    return 0;
}

template <int N>
static int dispatch_bank_roll(int n, int fma, const float *center, const BankJob &job, int cu_count, hipStream_t st)
{
    if (n == N) return fma ? launch_bank_roll<N, true>(center, job, cu_count, st) : launch_bank_roll<N, false>(center, job, cu_count, st);
    if constexpr (N < STREAM_ROLL_MAX_N) return dispatch_bank_roll<N + 1>(n, fma, center, job, cu_count, st);
    else return 1;
}

// 0 = launched, 1 = not covered (half window outside 1..32, ticks >= 2^31).  Builds the job, asks block_form (sg_stream_host.hpp) which form the call
// takes and launches it; a launcher that reports "not covered" hands the call to the next form.
int sg_bank_roll_launch(int n, const float *center_weights, const float *ring, const float *samples, float *out, size_t streams,
                        int wp0, unsigned long long received0, size_t ticks, float dt_inv, int fma, int cu_count, hipStream_t st)
{
    if (n < 1 || n > STREAM_ROLL_MAX_N || ticks == 0 || ticks > (size_t)0x7fffffff) return 1;
    BankJob job;
    memset(&job, 0, sizeof(job));
    job.ring = ring; job.samples = samples; job.out = out;
    job.streams = streams; job.ticks = ticks; job.received0 = received0; job.wp0 = wp0; job.dt_inv = dt_inv;
    {
        double wsum = 0.0, wabs = 0.0;
        for (int k = 0; k <= 2 * n; ++k) { wsum += (double)center_weights[k]; wabs += std::fabs((double)center_weights[k]); }
        job.centre_sum = (float)wsum;
        job.centre = (fma && std::fabs(wsum) < 1e-3 * wabs) ? 1 : 0;       // smoothing filters (sum 1) gain nothing and a zero-mean stream would lose
    }
    static const int dma_env = [] { const char *e = getenv("SAVGOL_HIP_STREAM_DMA"); return e ? atoi(e) : 1; }();
    static const int moment_env = [] { const char *e = getenv("SAVGOL_HIP_STREAM_MOMENT"); return e ? atoi(e) : 1; }();
    const unsigned misaligned = (unsigned)((reinterpret_cast<uintptr_t>(samples) | reinterpret_cast<uintptr_t>(out) | reinterpret_cast<uintptr_t>(ring)) & 15u);
    StreamMomentFit fit;
    for (int first = MOMENT_TILES;; ++first) {
        const BlockForm form = block_form(n, fma != 0, streams, ticks, misaligned, job.centre != 0, dma_env != 0, moment_env != 0,
                                          [&] { return stream_moment_fit(n, center_weights, &fit); }, first);
        switch (form) {
        case MOMENT_TILES:   if (sg_bank_dma_launch_mom(n, fit, center_weights, job, st) == 0) return 0; break;
        case DMA_TILES:      if ((n <= 16 ? sg_bank_dma_launch_lo : sg_bank_dma_launch_hi)(n, fma, center_weights, job, st) == 0) return 0; break;
        case REGISTER_TILES: if (dispatch_bank_tile<1>(n, center_weights, job, st) == 0) return 0; break;
        case WALK:           return dispatch_bank_roll<1>(n, fma, center_weights, job, cu_count, st);
        }
        first = form;                                        // not covered: the next form in the order
    }
}

}  // namespace sg
