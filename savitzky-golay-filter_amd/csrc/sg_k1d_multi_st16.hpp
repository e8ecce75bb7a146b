// sg_k1d_multi_st16.hpp -- the fused multi-output 1-D kernel on 16-bit STORAGE (savgol_apply[_valid]_multi_batch_h16 and _i16): K filters of one half
// window and one boundary mode on ONE read of 16-bit rows, fp32 arithmetic inside; ONE body for the two storage families of sg_k1d_st16.hpp (h16: fp16 /
// bf16 rows, outputs of the same type or fp32; i16: int16 rows, outputs int16 or fp32).  Bytes per input sample: 2 + 2 K (16 -> 16 bit) instead of
// K (2 + 2).
//
// The order of sg1d_multi_body (sg_k1d_multi.hpp) on the storage policies of sg1d_st16_body, written in the shared pieces of sg_k1d.hpp: stage_tile
// with the family's storage policy widens the rows into the fp32 slab (one dwordx2 load per slab vector, all loads issued before the first convert), which ends up exactly as the
// fp32 kernel's; the raw outputs, then centre_slab once, then the centred outputs, each Conv<float, N, VPL_NARROW>::run + finish_acc with its own taps,
// centre_sum and dt_inv; put_results into the wave's second LDS region; store_tile with the output's storage policy, which converts once on
// the way out (fp16 / bf16: nearest even; int16: nearest even, saturated, NaN -> 0).  So output k carries the bits of the family's single call with
// SAVGOL_BATCH_PLAIN_SUMMATION, and of the fp32 fused call on the widened input, converted once.
// The storage types are wave-uniform job fields (scalar branches, where sg_k1d_st16.hpp says): one kernel per (half window, K) serves every type pair
// of its family.  LDS, launch bounds and occupancy are sg1d_multi_kernel's: 9.5 + 8 KiB per wave, two 4-wave blocks per CU.
// POLYNOMIAL edge rows ride as 2 K items per channel behind the tiles, each a 16-bit load and a store of the output type (as sg1d_st16_edge_item's).
#pragma once

#include "sg_k1d_st16.hpp"

namespace sg {

// edge item `it`: channel it / (2K), output (it % 2K) / 2, end it % 2 (0 leading, 1 trailing)
template <int N, int K, typename F>
__device__ __forceinline__ void sg1d_multi_st16_edge_item(const JobMultiSt16<typename F::Types> &js, unsigned it, int lane)
{
    const JobMulti1D &job = js.multi;
    const unsigned c = it / (2u * K), r = it % (2u * K), k = r >> 1;
    const bool trailing = (r & 1u) != 0;
    const typename F::Elem *__restrict__ row = static_cast<const typename F::Elem *>(job.base.in) + (long long)c * job.base.in_ld;
    const bool ibf = F::in_bf(js), obf = F::out_bf(js), of32 = F::out_f32(js);
    float *__restrict__ orow32 = static_cast<float *>(job.out[k]) + (long long)c * job.base.out_ld;
    typename F::Elem *__restrict__ orow16 = static_cast<typename F::Elem *>(job.out[k]) + (long long)c * job.base.out_ld;
    sg1d_edge_rows<float, N>(job.edges[k], job.flags[k], job.dt_inv[k], trailing, (long long)job.base.length, lane,
                             [&](long long i) { return F::widen1(row[i], ibf); },
                             [&](long long i, float v) { if (of32) orow32[i] = v; else orow16[i] = F::narrow1(v, obf); });
}

template <int N, int K, typename F>
__device__ __forceinline__ void sg1d_multi_st16_body(const JobMultiSt16<typename F::Types> &js, const TapsMulti &taps)
{
    typedef K1D<float, N, VPL_NARROW> KT;
    constexpr int VPL = KT::VPL;
    static_assert(VPL == 8 && KT::E == 4, "the narrow fp32 tile: four samples per slab vector, the swizzled result layout (result_vec_off8)");
    constexpr int RES = 64 * VPL * 16;                                   // bytes of one tile's results
    const JobMulti1D &jm = js.multi;
    const Job1D &job = jm.base;

    __shared__ __attribute__((aligned(16))) char smem[KT::WAVES * (KT::SLAB + RES)];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    char *slab = smem + wave * (KT::SLAB + RES);
    char *res = slab + KT::SLAB;

    const unsigned tile = sg1d_tile_of_wave<KT::WAVES>(job, wave);
    if (tile >= job.total_tiles) {                                        // wave-uniform: past the tiles come the edge items, if any
        if (tile - job.total_tiles < job.edge_items) sg1d_multi_st16_edge_item<N, K, F>(js, tile - job.total_tiles, lane);
        return;
    }

    const unsigned c = tile_channel(job, tile);
    const int ts = (int)(tile - c * job.tiles_per_channel) * KT::TW;
    const typename F::Elem *__restrict__ row = static_cast<const typename F::Elem *>(job.in) + (long long)c * job.in_ld;
    const SlabRows<KT> row_vec(slab, lane);

    // ---- stage tile + halo into the slab, widened on the way ----
    if (F::HAS_BF && F::in_bf(js)) stage_tile<KT, typename F::template Storage<true>>(row_vec, row, ts, (int)job.length, job.flags, lane);
    else stage_tile<KT, typename F::template Storage<false>>(row_vec, row, ts, (int)job.length, job.flags, lane);
    wave_lds_sync();

    const char *const win = slab + 16 * (lane * (KT::VPL + 1));
    const int lo = (int)job.store_lo, hi = (int)job.store_hi;
    const long long o0 = (long long)c * job.out_ld - (long long)job.out_shift;
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
        if (F::out_f32(js)) store_tile<KT, SameStorage<float>>(res, static_cast<float *>(jm.out[k]) + o0, ts, lo, hi, jm.flags[k], lane);
        else if (F::HAS_BF && F::out_bf(js)) store_tile<KT, typename F::template Storage<true>>(res, static_cast<typename F::Elem *>(jm.out[k]) + o0, ts, lo, hi, jm.flags[k], lane);
        else store_tile<KT, typename F::template Storage<false>>(res, static_cast<typename F::Elem *>(jm.out[k]) + o0, ts, lo, hi, jm.flags[k], lane);
        wave_lds_sync();
        return true;
    });
}

// K = 2 or 3 outputs; 2 waves per SIMD (LDS allows two 4-wave blocks per CU), as sg1d_multi_kernel.  One entry point per family.
template <int N, int K>
__global__ __launch_bounds__(256, 2) void sg1d_multi_h16_kernel(const JobMultiH16 job, const TapsMulti taps)
{
    static_assert(K >= 2 && K <= MULTI_MAX_K, "2 or 3 outputs per launch");
    sg1d_multi_st16_body<N, K, H16Family>(job, taps);
}
template <int N, int K>
__global__ __launch_bounds__(256, 2) void sg1d_multi_i16_kernel(const JobMultiI16 job, const TapsMulti taps)
{
    static_assert(K >= 2 && K <= MULTI_MAX_K, "2 or 3 outputs per launch");
    sg1d_multi_st16_body<N, K, I16Family>(job, taps);
}

}  // namespace sg
