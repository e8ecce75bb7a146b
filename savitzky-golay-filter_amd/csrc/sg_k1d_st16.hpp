// sg_k1d_st16.hpp -- the 1-D tile kernel on 16-bit STORAGE, fp32 arithmetic inside: ONE body for two storage families,
//   h16  fp16 or bf16 rows in, the same type or fp32 out   (savgol_apply[_valid]_batch_h16)
//   i16  int16 rows in, int16 or fp32 out                   (savgol_apply[_valid]_batch_i16)
// 4 B (16 -> 16 bit) or 6 B (16 bit -> fp32) per sample instead of the fp32 call's 8.
//
// The tile algorithm of sg1d_tile_body, built from the same pieces (sg_k1d.hpp: sg1d_tile_of_wave, tile_channel, stage_tile, centre_slab, finish_acc,
// put_results, store_tile) on the narrow tile (64 lanes x 8 vectors of four samples), with the same inner product (the policy CV:
// DirectConv<float, N, 8> or MomentHConv<N, M1>) and the POLYNOMIAL edge rows as items of the same launch.
// Only the first and the last hop know the storage type (H16Storage / I16Storage below, the policies stage_tile and store_tile take), so the output is
// the fp32 narrow-tile call's on the widened input, bit for bit, converted ONCE into the output type just before it is stored (contract:
// include/savgol_hip.h): fp16 / bf16 round to nearest even; int16 rounds to nearest even, saturates, NaN -> 0.
//
// Staging.  A slab vector is four fp32 samples = four 16-bit elements = 8 bytes of the row, and both the halo (NA, a multiple of 4 samples) and the
// tile start (a multiple of 2048) are 8-byte granular.  So lane l loads the 8 bytes of slab vector l + 64 s with one nontemporal dwordx2 load -- the
// fp32 kernel's lane <-> vector mapping, a wave's load is one coalesced 512-byte row -- widens them in registers (v_cvt_f32_f16; a shift / mask for
// bf16; one sign-extending v_cvt_f32_i32 per int16 element, exact) and writes the fp32 kernel's own ds_write_b128 to the fp32 kernel's own address:
// the slab ends up exactly as the fp32 kernel's, with its conflict-free bank pattern.  (16-byte loads would carry two slab vectors per lane: either
// the LDS writes leave the row-wise pattern, or the halo -- 8-byte granular for every NA that is not a multiple of 8 -- splits the load.  The tile is
// bound by HBM bytes, not by load instructions.)  All loads are issued before the first conversion.  Store: the results come back row-wise through
// the result layout (the fp32 kernel's ds_read_b128), four per lane, are packed two per dword (v_cvt_pk_f16_f32 / v_cvt_pk_bf16_f32; v_rndne_f32,
// v_cvt_i32_f32 and v_cvt_pk_i16_i32 for int16) and leave as coalesced 8-byte rows; fp32 output keeps the fp32 kernel's 16-byte store.
//
// What the two families differ in is their policy (H16Family, I16Family): the element type, the storage fields of the job, the storage policies and
// converts, and where scalar branches on those wave-uniform fields sit -- h16 branches on in_type at staging and on out_type at the store, i16 on
// out_type at the store alone.
// One kernel per half window serves every type pair of its family.
#pragma once

#include "sg_family.hpp"
#include "sg_h16.hpp"
#include "sg_i16.hpp"
#include "sg_k1d.hpp"
#include "sg_k1d_st16_host.hpp"

namespace sg {

// 16-bit rows for stage_tile / store_tile (SameStorage's counterparts): a slab vector's four samples are 8 bytes of the row.  The converts: sg_h16.hpp
// and sg_i16.hpp, shared with the stream kernels.
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
struct I16Storage {
    typedef short Elem;
    typedef u32x2 Raw;
    static __device__ __forceinline__ Raw ld_stream(const Raw *p) { return __builtin_nontemporal_load(p); }
    static __device__ __forceinline__ void st_stream(Raw *p, const float4 &v) { __builtin_nontemporal_store(narrow(v), p); }
    static __device__ __forceinline__ float4 widen(const Raw &r) { return widen4_i16(r); }
    static __device__ __forceinline__ float widen1(Elem x) { return (float)x; }
    static __device__ __forceinline__ Raw narrow(const float4 &v) { return narrow4_i16(v); }
    static __device__ __forceinline__ Elem narrow1(float x) { return narrow1_i16(x); }
};

// ---- the storage families: what the shared bodies (sg1d_st16_body below, sg1d_multi_st16_body in sg_k1d_multi_st16.hpp) ask of a family ----
//   Elem, Types              the rows' element type; the job's storage fields (sg_k1d_st16_host.hpp)
//   Storage<BF>              the policy stage_tile / store_tile take for 16-bit rows; HAS_BF: the family has two element types, fp16 and bf16, and
//                            BF picks between them (where it has one, the bodies' branch on BF folds away at compile time)
//   in_bf, out_bf, out_f32   which types the job names: a bf16 input, a bf16 output, an fp32 output (wave-uniform: scalar branches)
//   widen1, narrow1          one element to fp32 and back, for the edge items' scalar loads and stores
// The bodies branch on these themselves and call stage_tile / store_tile directly: a family function around either call changes the generated code.
struct H16Family {
    typedef unsigned short Elem;
    typedef H16Types Types;
    template <bool BF> using Storage = H16Storage<BF>;
    static constexpr bool HAS_BF = true;
    static __device__ __forceinline__ bool in_bf(const Types &st) { return st.in_type == STORE_BF16; }
    static __device__ __forceinline__ bool out_bf(const Types &st) { return st.out_type == STORE_BF16; }
    static __device__ __forceinline__ bool out_f32(const Types &st) { return st.out_type == STORE_F32; }
    static __device__ __forceinline__ float widen1(Elem x, bool bf) { return sg::widen1(x, bf); }
    static __device__ __forceinline__ Elem narrow1(float v, bool bf) { return sg::narrow1(v, bf); }
};
struct I16Family {
    typedef short Elem;
    typedef I16Types Types;
    template <bool BF> using Storage = I16Storage;
    static constexpr bool HAS_BF = false;
    static __device__ __forceinline__ bool in_bf(const Types &) { return false; }
    static __device__ __forceinline__ bool out_bf(const Types &) { return false; }
    static __device__ __forceinline__ bool out_f32(const Types &st) { return st.out_type == STORE_I16_F32; }
    static __device__ __forceinline__ float widen1(Elem x, bool) { return (float)x; }
    static __device__ __forceinline__ Elem narrow1(float v, bool) { return narrow1_i16(v); }
};

// edge item 2c = leading end of channel c, 2c + 1 = its trailing end (sg1d_edge_item with a 16-bit Load and a Store of the output type: the row's
// fp32 result -- the fp32 call's own -- is converted once more into the output type)
template <int N, typename F>
__device__ __forceinline__ void sg1d_st16_edge_item(const JobSt16<typename F::Types> &js, unsigned item, int lane)
{
    const Job1D &job = js.base;
    const long long c = item >> 1;
    const typename F::Elem *__restrict__ row = static_cast<const typename F::Elem *>(job.in) + c * job.in_ld;
    const bool ibf = F::in_bf(js), obf = F::out_bf(js), of32 = F::out_f32(js);
    float *__restrict__ orow32 = static_cast<float *>(job.out) + c * job.out_ld;
    typename F::Elem *__restrict__ orow16 = static_cast<typename F::Elem *>(job.out) + c * job.out_ld;
    sg1d_edge_rows<float, N>(job.edges, job.flags, job.dt_inv, (item & 1u) != 0, (long long)job.length, lane,
                             [&](long long i) { return F::widen1(row[i], ibf); },
                             [&](long long i, float v) { if (of32) orow32[i] = v; else orow16[i] = F::narrow1(v, obf); });
}

template <int N, typename CV, typename F>
__device__ __forceinline__ void sg1d_st16_body(const JobSt16<typename F::Types> &js, const typename CV::Args &taps)
{
    typedef typename CV::K K;
    constexpr int VPL = K::VPL;
    static_assert(VPL == VPL_NARROW && VPL == 8 && K::E == 4, "the narrow fp32 tile: four samples per slab vector, the swizzled result layout (result_vec_off8)");
    const Job1D &job = js.base;

    __shared__ __attribute__((aligned(16))) char smem[K::WAVES * K::SLAB];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    char *slab = smem + wave * K::SLAB;

    const unsigned tile = sg1d_tile_of_wave<K::WAVES>(job, wave);
    if (tile >= job.total_tiles) {                                        // wave-uniform: past the tiles come the edge items, if any
        if (tile - job.total_tiles < job.edge_items) sg1d_st16_edge_item<N, F>(js, tile - job.total_tiles, lane);
        return;
    }

    const unsigned c = tile_channel(job, tile);
    const int ts = (int)(tile - c * job.tiles_per_channel) * K::TW;
    const typename F::Elem *__restrict__ row = static_cast<const typename F::Elem *>(job.in) + (long long)c * job.in_ld;
    const SlabRows<K> row_vec(slab, lane);

    // ---- stage tile + halo into the slab, widened on the way (the storage types are wave-uniform kernel arguments: scalar branches) ----
    if (F::HAS_BF && F::in_bf(js)) stage_tile<K, typename F::template Storage<true>>(row_vec, row, ts, (int)job.length, job.flags, lane);
    else stage_tile<K, typename F::template Storage<false>>(row_vec, row, ts, (int)job.length, job.flags, lane);
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

    // ---- results back through the slab, then coalesced rows to HBM in the output type, converted once on the way ----
    put_results<K>(slab, lane, acc);
    wave_lds_sync();
    const int lo = (int)job.store_lo, hi = (int)job.store_hi;
    const long long o0 = (long long)c * job.out_ld - (long long)job.out_shift;
    if (F::out_f32(js)) store_tile<K, SameStorage<float>>(slab, static_cast<float *>(job.out) + o0, ts, lo, hi, job.flags, lane);
    else if (F::HAS_BF && F::out_bf(js)) store_tile<K, typename F::template Storage<true>>(slab, static_cast<typename F::Elem *>(job.out) + o0, ts, lo, hi, job.flags, lane);
    else store_tile<K, typename F::template Storage<false>>(slab, static_cast<typename F::Elem *>(job.out) + o0, ts, lo, hi, job.flags, lane);
}

// the plain sliding dot product on the narrow tile (sg1d_center_kernel<float, N, 8>'s arithmetic), one entry point per family
template <int N>
__global__ __launch_bounds__(64 * SG_K1D_WAVES, (K1D<float, N, VPL_NARROW>::MIN_WAVES)) void sg1d_h16_kernel(const JobH16 job, const Taps taps)
{
    sg1d_st16_body<N, DirectConv<float, N, VPL_NARROW>, H16Family>(job, taps);
}
template <int N>
__global__ __launch_bounds__(64 * SG_K1D_WAVES, (K1D<float, N, VPL_NARROW>::MIN_WAVES)) void sg1d_i16_kernel(const JobI16 job, const Taps taps)
{
    sg1d_st16_body<N, DirectConv<float, N, VPL_NARROW>, I16Family>(job, taps);
}

// The instantiation files (sg_k1d_st16.hip, sg_k1d_st16_momenth.hip, sg_k1d_multi_st16.hip) are compiled once per family, -DSG_FAMILY=h16|i16:
// `Family` is that family's policy, SG_FAMILY_NAME(sg1d_, _kernel) (sg_family.hpp) its entry point sg1d_h16_kernel / sg1d_i16_kernel.
#ifdef SG_FAMILY
struct Families { typedef H16Family h16; typedef I16Family i16; };
typedef Families::SG_FAMILY Family;
#endif

}  // namespace sg
