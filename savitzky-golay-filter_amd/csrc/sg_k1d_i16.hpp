// sg_k1d_i16.hpp -- the 1-D tile kernel on int16 STORAGE (savgol_apply[_valid]_batch_i16): int16 rows in, int16 or fp32 out, fp32 arithmetic
// inside.  4 B (int16 -> int16) or 6 B (int16 -> fp32) per sample instead of the fp32 call's 8.
//
// sg1d_h16_body (sg_k1d_h16.hpp) step for step, built from the same pieces (sg_k1d.hpp: sg1d_tile_of_wave, tile_channel, stage_tile, centre_slab,
// finish_acc, put_results, store_tile) on the narrow tile (64 lanes x 8 vectors of four samples), with the same inner product (the policy CV:
// DirectConv<float, N, 8> or MomentHConv<N, M1>) and the POLYNOMIAL edge rows as items of the same launch.  Only the first and the last hop know
// the storage type (I16Storage below), so the output is the fp32 narrow-tile call's on the widened input, bit for bit; for int16 output it is
// converted ONCE just before it is stored (contract: include/savgol_hip.h).
//
// Staging.  A slab vector is four fp32 samples = four int16 elements = 8 bytes of the row, and both the halo (NA, a multiple of 4 samples) and the
// tile start (a multiple of 2048) are 8-byte granular.  So lane l loads the 8 bytes of slab vector l + 64 s with one nontemporal dwordx2 load --
// the fp32 kernel's lane <-> vector mapping, a wave's load is one coalesced 512-byte row -- widens them in registers (one sign-extending
// v_cvt_f32_i32 per element, exact) and writes the fp32 kernel's own ds_write_b128 to the fp32 kernel's own address.  All loads are issued before
// the first conversion.  Store: the results come back row-wise through the result layout (the fp32 kernel's ds_read_b128), four per lane; int16
// output is rounded (v_rndne_f32), converted (v_cvt_i32_f32), packed two per dword (v_cvt_pk_i16_i32) and leaves as coalesced 8-byte rows; fp32
// output keeps the fp32 kernel's 16-byte store.  The output type is a wave-uniform field of the job (sg_k1d_i16_host.hpp): a scalar branch, one
// kernel per half window for both outputs.
#pragma once

#include "sg_i16.hpp"
#include "sg_k1d.hpp"
#include "sg_k1d_i16_host.hpp"

namespace sg {

// the converts (widen4_i16, narrow4_i16, narrow1_i16 and what they are made of): sg_i16.hpp, shared with the stream kernels on int16 storage

// int16 rows for stage_tile / store_tile (SameStorage's counterpart): a slab vector's four samples are 8 bytes of the row
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

// edge item 2c = leading end of channel c, 2c + 1 = its trailing end (sg1d_edge_item with an int16 Load and a Store of the output type: the row's
// fp32 result -- the fp32 call's own -- is converted once into the output type)
template <int N>
__device__ __forceinline__ void sg1d_i16_edge_item(const JobI16 &ji, unsigned item, int lane)
{
    const Job1D &job = ji.base;
    const long long c = item >> 1;
    const short *__restrict__ row = static_cast<const short *>(job.in) + c * job.in_ld;
    const bool of32 = ji.out_type == STORE_I16_F32;
    float *__restrict__ orow32 = static_cast<float *>(job.out) + c * job.out_ld;
    short *__restrict__ orow16 = static_cast<short *>(job.out) + c * job.out_ld;
    sg1d_edge_rows<float, N>(job.edges, job.flags, job.dt_inv, (item & 1u) != 0, (long long)job.length, lane,
                             [&](long long i) { return (float)row[i]; },
                             [&](long long i, float v) { if (of32) orow32[i] = v; else orow16[i] = narrow1_i16(v); });
}

template <int N, typename CV>
__device__ __forceinline__ void sg1d_i16_body(const JobI16 &ji, const typename CV::Args &taps)
{
    typedef typename CV::K K;
    constexpr int VPL = K::VPL;
    static_assert(VPL == VPL_NARROW && VPL == 8 && K::E == 4, "the narrow fp32 tile: four samples per slab vector, the swizzled result layout (result_vec_off8)");
    const Job1D &job = ji.base;

    __shared__ __attribute__((aligned(16))) char smem[K::WAVES * K::SLAB];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    char *slab = smem + wave * K::SLAB;

    const unsigned tile = sg1d_tile_of_wave<K::WAVES>(job, wave);
    if (tile >= job.total_tiles) {                                        // wave-uniform: past the tiles come the edge items, if any
        if (tile - job.total_tiles < job.edge_items) sg1d_i16_edge_item<N>(ji, tile - job.total_tiles, lane);
        return;
    }

    const unsigned c = tile_channel(job, tile);
    const int ts = (int)(tile - c * job.tiles_per_channel) * K::TW;
    const short *__restrict__ row = static_cast<const short *>(job.in) + (long long)c * job.in_ld;
    const SlabRows<K> row_vec(slab, lane);

    // ---- stage tile + halo into the slab, widened on the way ----
    stage_tile<K, I16Storage>(row_vec, row, ts, (int)job.length, job.flags, lane);
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

    // ---- results back through the slab, then coalesced rows to HBM in the output type (the type is a wave-uniform kernel argument: a scalar branch) ----
    put_results<K>(slab, lane, acc);
    wave_lds_sync();
    const int lo = (int)job.store_lo, hi = (int)job.store_hi;
    const long long o0 = (long long)c * job.out_ld - (long long)job.out_shift;
    if (ji.out_type == STORE_I16_F32) store_tile<K, SameStorage<float>>(slab, static_cast<float *>(job.out) + o0, ts, lo, hi, job.flags, lane);
    else store_tile<K, I16Storage>(slab, static_cast<short *>(job.out) + o0, ts, lo, hi, job.flags, lane);
}

// the plain sliding dot product on the narrow tile (sg1d_center_kernel<float, N, 8>'s arithmetic)
template <int N>
__global__ __launch_bounds__(64 * SG_K1D_WAVES, (K1D<float, N, VPL_NARROW>::MIN_WAVES)) void sg1d_i16_kernel(const JobI16 job, const Taps taps)
{
    sg1d_i16_body<N, DirectConv<float, N, VPL_NARROW>>(job, taps);
}

}  // namespace sg
