// sg_k1d_multi.hpp -- the fused multi-output 1-D kernel (savgol_apply_multi_batch_f32): K filters of one half window and one boundary mode
// (smoothing, d/dt, d^2/dt^2, ...) on ONE read of the input.  Bytes per input sample: 4 + 4 K instead of K (4 + 4).
//
// The tile algorithm of sg1d_tile_body, built from the same pieces (sg_k1d.hpp: sg1d_tile_of_wave, tile_channel, stage_tile, centre_slab, finish_acc,
// put_results, store_tile) on the narrow tile (64 lanes x 8 vectors), with the same inner product (Conv<float, N, VPL_NARROW>: three interleaved
// chains) once per output with that output's taps -- so output k carries the bits of the single call with SAVGOL_BATCH_PLAIN_SUMMATION.  Order is
// what keeps those bits:
//   1. the outputs that are not centred (derivative 0; the host puts them first, nraw of them) on the RAW slab;
//   2. then the slab is centred (the single kernel's JOB_CENTRE: the mean of the tile's body, the same Inf / NaN guard), if any output needs it;
//   3. the centred outputs on the centred slab, each adding back centre * sum(w) and scaling by its own dt_inv.
// Results leave through a second LDS region of the wave (8 KiB, the swizzled result layout of the single kernel), never through the slab, so the
// slab holds the samples until the last output's window reads are done, and output k's stores overlap output k+1's inner product.
// LDS: 9.5 + 8 KiB per wave, 70 KB per 4-wave block: two blocks per CU, 2 waves per SIMD (the wide single tiles run at that occupancy too).
// POLYNOMIAL edge rows ride as 2 K items per channel behind the tiles, each with its own output's edge table, dt_inv and leading-edge sign.
#pragma once

#include "sg_k1d.hpp"

namespace sg {

// edge item `it` of a multi-output job: channel it / (2K), output (it % 2K) / 2, end it % 2 (0 leading, 1 trailing)
template <int N, int K>
__device__ __forceinline__ void sg1d_multi_edge_item(const JobMulti1D &job, unsigned it, int lane)
{
    const unsigned c = it / (2u * K), r = it % (2u * K), k = r >> 1;
    const bool trailing = (r & 1u) != 0;
    const float *__restrict__ row = static_cast<const float *>(job.base.in) + (long long)c * job.base.in_ld;
    float *__restrict__ orow = static_cast<float *>(job.out[k]) + (long long)c * job.base.out_ld;
    sg1d_edge_rows<float, N>(job.edges[k], job.flags[k], job.dt_inv[k], trailing, (long long)job.base.length, lane,
                             [&](long long i) { return row[i]; }, [&](long long i, float v) { orow[i] = v; });
}

template <int N, int K>
__device__ __forceinline__ void sg1d_multi_body(const JobMulti1D &jm, const TapsMulti &taps)
{
    typedef K1D<float, N, VPL_NARROW> KT;
    constexpr int VPL = KT::VPL;
    static_assert(VPL == 8, "the result region uses the swizzled layout of 8 vectors per lane (result_vec_off8)");
    constexpr int RES = 64 * VPL * 16;                                   // bytes of one tile's results
    const Job1D &job = jm.base;

    __shared__ __attribute__((aligned(16))) char smem[KT::WAVES * (KT::SLAB + RES)];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    char *slab = smem + wave * (KT::SLAB + RES);
    char *res = slab + KT::SLAB;

    const unsigned tile = sg1d_tile_of_wave<KT::WAVES>(job, wave);
    if (tile >= job.total_tiles) {
        if (tile - job.total_tiles < job.edge_items) sg1d_multi_edge_item<N, K>(jm, tile - job.total_tiles, lane);
        return;
    }

    const unsigned c = tile_channel(job, tile);
    const int ts = (int)(tile - c * job.tiles_per_channel) * KT::TW;
    const float *__restrict__ row = static_cast<const float *>(job.in) + (long long)c * job.in_ld;
    const SlabRows<KT> row_vec(slab, lane);

    stage_tile<KT, SameStorage<float>>(row_vec, row, ts, (int)job.length, job.flags, lane);
    wave_lds_sync();

    const char *const win = slab + 16 * (lane * (KT::VPL + 1));
    float centre = 0.0f;
    static_for<K>([&](auto kc) {
        constexpr int k = decltype(kc)::value;
        if (k == (int)jm.nraw) {
            // the first centred output: centre the slab, after the raw outputs' window reads
            wave_lds_sync();
            centre = centre_slab(row_vec, lane);
            wave_lds_sync();
        }
        // ---- output k: the inner product, the centre added back, dt_inv ----
        float acc[KT::R];
        Conv<float, N, VPL_NARROW>::run(win, taps.t[k], acc);
        finish_acc(acc, jm.flags[k], centre, jm.centre_sum[k], jm.dt_inv[k]);
        // ---- through the result region (the previous output's reads of it are done: one wave's LDS operations run in order) ----
        put_results<KT>(res, lane, acc);
        wave_lds_sync();
        float *__restrict__ orow = static_cast<float *>(jm.out[k]) + (long long)c * job.out_ld - (long long)job.out_shift;
        store_tile<KT, SameStorage<float>>(res, orow, ts, (int)job.store_lo, (int)job.store_hi, jm.flags[k], lane);
        wave_lds_sync();
        return true;
    });
}

// K = 2 or 3 outputs; 2 waves per SIMD (LDS allows two 4-wave blocks per CU)
template <int N, int K>
__global__ __launch_bounds__(256, 2) void sg1d_multi_kernel(const JobMulti1D job, const TapsMulti taps)
{
    static_assert(K >= 2 && K <= MULTI_MAX_K, "2 or 3 outputs per launch");
    sg1d_multi_body<N, K>(job, taps);
}

}  // namespace sg
