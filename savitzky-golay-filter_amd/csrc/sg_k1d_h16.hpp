// sg_k1d_h16.hpp -- the 1-D tile kernel on 16-bit STORAGE (savgol_apply[_valid]_batch_h16): fp16 or bf16 rows in, the same type or fp32 out,
// fp32 arithmetic inside.  4 B (16 -> 16) or 6 B (16 -> fp32) per sample instead of the fp32 call's 8.
//
// The tile algorithm of sg1d_tile_body, built from the same pieces (sg_k1d.hpp: sg1d_tile_of_wave, tile_channel, stage_tile, centre_slab, finish_acc,
// put_results, store_tile) on the narrow tile (64 lanes x 8 vectors of four samples), with the same inner product (the policy CV:
// DirectConv<float, N, 8> or MomentHConv<N, M1>) and the POLYNOMIAL edge rows as items of the same launch.
// Only the first and the last hop know the storage type (H16Storage below, the policy stage_tile and store_tile take), so the output is the fp32 narrow-tile call's on the widened input, bit for bit, rounded
// ONCE to nearest even into the output type just before it is stored (contract: include/savgol_hip.h).
//
// Staging.  A slab vector is four fp32 samples = four 16-bit elements = 8 bytes of the row, and both the halo (NA, a multiple of 4 samples) and the
// tile start (a multiple of 2048) are 8-byte granular.  So lane l loads the 8 bytes of slab vector l + 64 s with one dwordx2 load -- the fp32
// kernel's lane <-> vector mapping, a wave's load is one coalesced 512-byte row -- widens them in registers (v_cvt_f32_f16; a shift / mask for
// bf16) and writes the fp32 kernel's own ds_write_b128 to the fp32 kernel's own address: the slab ends up exactly as the fp32 kernel's, with its
// conflict-free bank pattern.  (16-byte loads would carry two slab vectors per lane: either the LDS writes leave the row-wise pattern, or the halo
// -- 8-byte granular for every NA that is not a multiple of 8 -- splits the load.  The tile is bound by HBM bytes, not by load instructions.)
// All loads are issued before the first conversion.  Store: the results come back row-wise through the result layout (the fp32 kernel's
// ds_read_b128), four per lane, are packed two per dword with the hardware converts (v_cvt_pk_f16_f32 / v_cvt_pk_bf16_f32, round to nearest even)
// and leave as coalesced 8-byte rows; fp32 output keeps the fp32 kernel's 16-byte store.
// The storage types are wave-uniform fields of the job (sg_k1d_h16_host.hpp): scalar branches, one kernel per half window for all four type pairs.
#pragma once

#include "sg_k1d.hpp"
#include "sg_k1d_h16_host.hpp"

namespace sg {

typedef _Float16 f16x4 __attribute__((ext_vector_type(4)));
typedef __bf16   bf16x4 __attribute__((ext_vector_type(4)));

// four 16-bit elements as loaded (element 0 in the low half of .x) -> fp32, exactly
__device__ __forceinline__ float4 widen4_f16(const u32x2 raw)
{
    const f16x4 h = __builtin_bit_cast(f16x4, raw);
    return float4{(float)h.x, (float)h.y, (float)h.z, (float)h.w};
}
__device__ __forceinline__ float4 widen4_bf16(const u32x2 raw)
{
    return float4{__uint_as_float(raw.x << 16), __uint_as_float(raw.x & 0xffff0000u), __uint_as_float(raw.y << 16), __uint_as_float(raw.y & 0xffff0000u)};
}
__device__ __forceinline__ float widen1(const unsigned short raw, const bool bf)
{
    if (bf) return __uint_as_float((unsigned)raw << 16);
    return (float)__builtin_bit_cast(_Float16, raw);
}
// fp32 -> the 16-bit type, round to nearest even (NaN stays NaN, overflow gives +-Inf)
__device__ __forceinline__ u32x2 narrow4_f16(const float4 v)
{
    const f32x4 f = {v.x, v.y, v.z, v.w};
    return __builtin_bit_cast(u32x2, __builtin_convertvector(f, f16x4));
}
__device__ __forceinline__ u32x2 narrow4_bf16(const float4 v)
{
    const f32x4 f = {v.x, v.y, v.z, v.w};
    return __builtin_bit_cast(u32x2, __builtin_convertvector(f, bf16x4));
}
__device__ __forceinline__ unsigned short narrow1(const float v, const bool bf)
{
    if (bf) return __builtin_bit_cast(unsigned short, (__bf16)v);
    return __builtin_bit_cast(unsigned short, (_Float16)v);
}

// 16-bit rows for stage_tile / store_tile (SameStorage's counterpart): a slab vector's four samples are 8 bytes of the row
template <bool BF>
struct H16Storage {
    typedef unsigned short Elem;
    typedef u32x2 Raw;
    static __device__ __forceinline__ Raw ld_stream(const Raw *p) { return __builtin_nontemporal_load(p); }
    static __device__ __forceinline__ void st_stream(Raw *p, const float4 &v) { __builtin_nontemporal_store(narrow(v), p); }
    static __device__ __forceinline__ float4 widen(const Raw &r) { if constexpr (BF) return widen4_bf16(r); else return widen4_f16(r); }
    static __device__ __forceinline__ float widen1(Elem x) { return sg::widen1(x, BF); }
    static __device__ __forceinline__ Raw narrow(const float4 &v) { if constexpr (BF) return narrow4_bf16(v); else return narrow4_f16(v); }
    static __device__ __forceinline__ Elem narrow1(float x) { return sg::narrow1(x, BF); }
};

// edge item 2c = leading end of channel c, 2c + 1 = its trailing end (sg1d_edge_item with a 16-bit Load and a Store of the output type: the row's
// fp32 result -- the fp32 call's own -- is rounded once more into the output type)
template <int N>
__device__ __forceinline__ void sg1d_h16_edge_item(const JobH16 &jh, unsigned item, int lane)
{
    const Job1D &job = jh.base;
    const long long c = item >> 1;
    const unsigned short *__restrict__ row = static_cast<const unsigned short *>(job.in) + c * job.in_ld;
    const bool ibf = jh.in_type == STORE_BF16, obf = jh.out_type == STORE_BF16, of32 = jh.out_type == STORE_F32;
    float *__restrict__ orow32 = static_cast<float *>(job.out) + c * job.out_ld;
    unsigned short *__restrict__ orow16 = static_cast<unsigned short *>(job.out) + c * job.out_ld;
    sg1d_edge_rows<float, N>(job.edges, job.flags, job.dt_inv, (item & 1u) != 0, (long long)job.length, lane,
                             [&](long long i) { return widen1(row[i], ibf); },
                             [&](long long i, float v) { if (of32) orow32[i] = v; else orow16[i] = narrow1(v, obf); });
}

template <int N, typename CV>
__device__ __forceinline__ void sg1d_h16_body(const JobH16 &jh, const typename CV::Args &taps)
{
    typedef typename CV::K K;
    constexpr int VPL = K::VPL;
    static_assert(VPL == VPL_NARROW && VPL == 8 && K::E == 4, "the narrow fp32 tile: four samples per slab vector, the swizzled result layout (result_vec_off8)");
    const Job1D &job = jh.base;

    __shared__ __attribute__((aligned(16))) char smem[K::WAVES * K::SLAB];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    char *slab = smem + wave * K::SLAB;

    const unsigned tile = sg1d_tile_of_wave<K::WAVES>(job, wave);
    if (tile >= job.total_tiles) {                                        // wave-uniform: past the tiles come the edge items, if any
        if (tile - job.total_tiles < job.edge_items) sg1d_h16_edge_item<N>(jh, tile - job.total_tiles, lane);
        return;
    }

    const unsigned c = tile_channel(job, tile);
    const int ts = (int)(tile - c * job.tiles_per_channel) * K::TW;
    const unsigned short *__restrict__ row = static_cast<const unsigned short *>(job.in) + (long long)c * job.in_ld;
    const SlabRows<K> row_vec(slab, lane);

    // ---- stage tile + halo into the slab, widened on the way (the storage types are wave-uniform kernel arguments: scalar branches) ----
    if (jh.in_type == STORE_BF16) stage_tile<K, H16Storage<true>>(row_vec, row, ts, (int)job.length, job.flags, lane);
    else stage_tile<K, H16Storage<false>>(row_vec, row, ts, (int)job.length, job.flags, lane);
    wave_lds_sync();

    float centre = 0.0f;
    if (job.flags & JOB_CENTRE) {                          // uniform
        centre = centre_slab(row_vec, lane);
        wave_lds_sync();
    }

    // ---- the convolution: lane owns outputs [lane*R, lane*R + R) of the tile ----
    float acc[K::R];
    CV::run(slab + 16 * (lane * (VPL + 1)), taps, acc, job.flags);
    finish_acc(acc, job.flags, centre, job.centre_sum, job.dt_inv);
    wave_lds_sync();                                   // all window reads done before overwrite

    // ---- results back through the slab, then coalesced rows to HBM in the output type, rounded once on the way ----
    put_results<K>(slab, lane, acc);
    wave_lds_sync();
    const int lo = (int)job.store_lo, hi = (int)job.store_hi;
    const long long o0 = (long long)c * job.out_ld - (long long)job.out_shift;
    if (jh.out_type == STORE_F32) store_tile<K, SameStorage<float>>(slab, static_cast<float *>(job.out) + o0, ts, lo, hi, job.flags, lane);
    else if (jh.out_type == STORE_BF16) store_tile<K, H16Storage<true>>(slab, static_cast<unsigned short *>(job.out) + o0, ts, lo, hi, job.flags, lane);
    else store_tile<K, H16Storage<false>>(slab, static_cast<unsigned short *>(job.out) + o0, ts, lo, hi, job.flags, lane);
}

// the plain sliding dot product on the narrow tile (sg1d_center_kernel<float, N, 8>'s arithmetic)
template <int N>
__global__ __launch_bounds__(64 * SG_K1D_WAVES, (K1D<float, N, VPL_NARROW>::MIN_WAVES)) void sg1d_h16_kernel(const JobH16 job, const Taps taps)
{
    sg1d_h16_body<N, DirectConv<float, N, VPL_NARROW>>(job, taps);
}

}  // namespace sg
