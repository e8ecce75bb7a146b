// sg_stream_roll.hpp -- types and device pieces shared by the block-push kernels (sg_stream_roll.hip: walk and register tiles; sg_stream_dma.hip: LDS-DMA tiles)
#pragma once

#include <hip/hip_runtime.h>

#include <cstddef>

#include "sg_pk.hpp"
#include "sg_stream.hpp"
#include "sg_stream_host.hpp"

namespace sg {

template <int N>
struct SRoll {
    static constexpr int WS = 2 * N + 1;
    // rows loaded ahead of the arithmetic.  Round 3, after the counters had said that a walk is short of
    // requests in flight rather than of memory (profiles/r03_strip_walk_counters.txt): the sample-ring kernels (n <= 16) with 7 rows
    // ahead -- and, for the fused-multiply-add bank, at most TWO resident blocks per CU (8 waves; launch_bank_roll) -- run config 3's
    // block push in 0.389 ms instead of 0.404-0.417 (0.69 of the roofline; n = 4: 0.378 vs 0.407), the reference-order bank 0.451-0.460
    // instead of 0.467-0.469 at its full occupancy (it is bound by its two instructions per tap and needs the waves).  The
    // accumulator-ring kernels (n > 16) have their own ring of rows in flight (bank_accroll_item) and keep 4 blocks per CU.
    static constexpr int P = N <= 16 ? 7 : 3;
    static constexpr int U = WS + P;                         // ring slots = unroll factor of the tick loop
    static constexpr int NP = N + 1;                         // SGPR pairs holding taps 0..2N
};

template <int N>
struct SRollTaps { f32x2 w[SRoll<N>::NP]; };

struct BankJob {
    const float *ring;               // [WS][streams], slot (wp0 - k) mod WS = sample -k of the history
    const float *samples;            // [ticks][streams]
    float       *out;                // [ticks][streams]
    size_t       streams, ticks;
    unsigned long long received0;    // samples per stream before this call
    int          wp0;
    float        dt_inv;
    unsigned     strips, bands;
    int          band_ticks;
    int          aligned;            // bit 0: rows of samples / ring / out start 8-byte aligned (streams even, bases aligned); bit 1: blocks in launch order (xcd_block)
    float        centre_sum;         // fused bank, LDS-DMA tiles: the sum of the reference's centre weights ...
    int          centre;             // ... and 1 when that sum is (nearly) zero -- a derivative filter: the tiles then run on centred samples (sg_stream_dma.hip)
};

// ---- pieces every block-push kernel is built from: each rule the forms must agree on, once ----
// History index h -> its row: h >= 0 is row h of this call's samples (h >= ticks: clamped -- past the call, loaded and never used), h < 0 is
// sample h of the history, ring slot (wp0 + h) mod WS
template <int WS>
__device__ __forceinline__ const float *history_row(const BankJob &job, long long h)
{
    if (h >= (long long)job.ticks) h = (long long)job.ticks - 1;
    int slot = job.wp0 + (int)(h < 0 ? h : 0);
    slot = slot < 0 ? slot + WS : slot;
    return h >= 0 ? job.samples + (size_t)h * job.streams : job.ring + (size_t)slot * job.streams;
}

// tick t of this call has an output: the windows are full (reference :166-170)
template <int WS>
__device__ __forceinline__ bool has_output(const BankJob &job, unsigned long long t) { return job.received0 + t + 1 >= (unsigned long long)WS; }

// the block whose share of the work this one takes: in launch order, or so that the blocks of one XCD (every eighth) take neighbouring shares
__device__ __forceinline__ unsigned xcd_block(bool launch_order)
{
    return launch_order ? blockIdx.x : (blockIdx.x & 7u) * (gridDim.x >> 3) + (blockIdx.x >> 3);
}

// tile t of the order tile_geom (sg_stream_host.hpp) lays out: groups of `group` neighbouring strips; inside a group band after band, strips fastest
// (32-bit scalar divisions: the launch keeps the tile count below 2^31).  !ok: beyond the last tile, or in the tail the narrower last group leaves empty
struct TileAt { unsigned band, strip; bool ok; };
__device__ __forceinline__ TileAt tile_of(const TileGeom &geo, unsigned t)
{
    if (t >= (unsigned)geo.total) return TileAt{0u, 0u, false};
    const unsigned per_group = geo.group * geo.bands;
    const unsigned grp = t / per_group;
    const unsigned rem = t - grp * per_group;
    const unsigned gs = geo.strips - grp * geo.group < geo.group ? geo.strips - grp * geo.group : geo.group;     // strips in this (last) group
    const unsigned band = rem / gs;
    return TileAt{band, grp * geo.group + (rem - band * gs), band < geo.bands};
}

// Fused bank, derivative filters (job.centre; R6.16, the reasons are in sg_stream_dma.hip): what an item's or tile's rows are centred on is the mean of
// EIGHT real samples of each stream, spread from the oldest real one at or after h_first to h_last (or the call's last row).  load(row) reads the lane's pair.
template <int WS, class Load>
__device__ __forceinline__ f32x2 spread_centre(const BankJob &job, long long h_first, long long h_last, Load load)
{
    const long long h0 = h_first < -(long long)job.received0 ? -(long long)job.received0 : h_first;
    const long long h1 = h_last > (long long)job.ticks - 1 ? (long long)job.ticks - 1 : h_last;
    const long long span = h1 - h0;
    f32x2 sum = f32x2{0.0f, 0.0f};
#pragma unroll
    for (int i = 0; i < 8; ++i) sum = sum + load(history_row<WS>(job, h0 + (span * i) / 7));
    return sum;
}
// the sum of eight -> the centre; an Inf / NaN among the eight: that stream stays as it is
__device__ __forceinline__ f32x2 centre_guard(const f32x2 sum)
{
    f32x2 cen = sum * f32x2{0.125f, 0.125f};
    if (!(cen.x - cen.x == 0.0f)) cen.x = 0.0f;
    if (!(cen.y - cen.y == 0.0f)) cen.y = 0.0f;
    return cen;
}

// Reference order (src/savgol_stream.c:25-38), one step: tap K times the sample pair, rounded on its own.  Volatile, like the adds beside it: left to
// the compiler the products of a row are hoisted in front of the sums and all stay live (256 registers and scratch; see sg_2d_dense.hip)
template <int K, int N>
__device__ __forceinline__ f32x2 pk_mul_tap(const SRollTaps<N> &taps, const f32x2 x)
{
    f32x2 p;
    if constexpr ((K & 1) == 0) asm volatile("v_pk_mul_f32 %0, %1, %2 op_sel_hi:[0,1]" : "=v"(p) : "s"(taps.w[K >> 1]), "v"(x));
    else                        asm volatile("v_pk_mul_f32 %0, %1, %2 op_sel:[1,0] op_sel_hi:[1,1]" : "=v"(p) : "s"(taps.w[K >> 1]), "v"(x));
    return p;
}
// Accumulator stationary: every in-flight output one tap further with sample pair x.  Slot a holds the output that has seen a samples; w[a] * x is
// added and the sum moves to slot a + 1 (walked from the top down, so that slot is already drained): every output adds its taps in ascending order
// onto 0, with separate roundings.  Returns the output that has just seen its last tap.
template <int N>
__device__ __forceinline__ f32x2 ref_advance(f32x2 (&acc)[2 * N + 1], const SRollTaps<N> &taps, const f32x2 x)
{
    constexpr int WS = 2 * N + 1;
    f32x2 done;
    static_for<WS>([&](auto ic) -> bool {
        constexpr int a = WS - 1 - decltype(ic)::value;      // slot = tap index, 2N down to 0
        const f32x2 p = pk_mul_tap<a>(taps, x);
        if constexpr (a == WS - 1)  asm volatile("v_pk_add_f32 %0, %1, %2" : "=v"(done) : "v"(acc[a]), "v"(p));
        else if constexpr (a == 0)  asm volatile("v_pk_add_f32 %0, %1, 0 op_sel_hi:[1,0]" : "=v"(acc[1]) : "v"(p));       // 0 + p: a product of -0 sums to +0, as in the reference
        else                        asm volatile("v_pk_add_f32 %0, %1, %2" : "=v"(acc[a + 1]) : "v"(acc[a]), "v"(p));
        return true;
    });
    return done;
}

// ---- the launchers of the forms block_form (sg_stream_host.hpp) chooses among.  0 = launched, 1 = not covered: a refused launch, a tile count beyond
// 32 bits -- sg_bank_roll_launch goes on to the next form ----
int sg_bank_dma_launch_mom(int n, const StreamMomentFit &fit, const float *center, const BankJob &job, hipStream_t st);    // sg_stream_dma.hip, half windows 12..20
int sg_bank_dma_launch_lo(int n, int fma, const float *center, const BankJob &job, hipStream_t st);                        // sg_stream_dma.hip, half windows 1..16
int sg_bank_dma_launch_hi(int n, int fma, const float *center, const BankJob &job, hipStream_t st);                        // 17..32

}  // namespace sg
