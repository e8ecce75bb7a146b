// sg_k1d_h16.hpp -- the 1-D tile kernel on 16-bit STORAGE (savgol_apply[_valid]_batch_h16): fp16 or bf16 rows in, the same type or fp32 out,
// fp32 arithmetic inside.  4 B (16 -> 16) or 6 B (16 -> fp32) per sample instead of the fp32 call's 8.
//
// A variant of sg1d_tile_body (sg_k1d.hpp), written beside it so that no existing kernel changes: the same narrow tile (64 lanes x 8 vectors of four
// samples), the same XCD tile order, the same fp32 slab with the same remaps, the same centring (JOB_CENTRE), the same inner product (the policy CV:
// DirectConv<float, N, 8> or MomentHConv<N, M1>), JOB_SCALE, the same swizzled result layout, the POLYNOMIAL edge rows as items of the same launch.
// Only the first and the last hop know the storage type, so the output is the fp32 narrow-tile call's on the widened input, bit for bit, rounded
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
    typedef float4 VT;
    constexpr int E = K::E, R = K::R, TW = K::TW, NA = K::NA, HV = K::HV, VPL = K::VPL, TV = K::TV;
    static_assert(VPL == VPL_NARROW && VPL == 8 && E == 4, "the narrow fp32 tile: four samples per slab vector, the swizzled result layout (result_vec_off8)");
    const Job1D &job = jh.base;

    __shared__ __attribute__((aligned(16))) char smem[K::WAVES * K::SLAB];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    char *slab = smem + wave * K::SLAB;

    // tile order: sg1d_tile_body's (the host counts chunks in blocks of four tiles)
    const unsigned nb8 = gridDim.x >> 3;
    unsigned blk = blockIdx.x;
    if (blk < nb8 * 8u) {
        const unsigned cs = job.xcd_chunk_log2 == 0 || job.xcd_chunk_log2 >= 32u ? job.xcd_chunk_log2 : job.xcd_chunk_log2 + (K::WAVES == 4 ? 0u : K::WAVES == 2 ? 1u : 2u);
        if (cs == 0) blk = (blk & 7u) * nb8 + (blk >> 3);
        else if (cs < 32u) {
            const unsigned span = 8u << cs, q = blk >> (cs + 3u);
            if ((q + 1u) * span <= nb8 * 8u) { const unsigned r = blk & (span - 1u); blk = (((q << 3) + (r & 7u)) << cs) + (r >> 3); }
        }
    }
    const unsigned tile = blk * K::WAVES + wave;
    if (tile >= job.total_tiles) {                                        // wave-uniform: past the tiles come the edge items, if any
        if (tile - job.total_tiles < job.edge_items) sg1d_h16_edge_item<N>(jh, tile - job.total_tiles, lane);
        return;
    }

    const bool ibf = jh.in_type == STORE_BF16;                            // wave-uniform (kernel argument)
    const int L = (int)job.length;
    const int mode = (int)(job.flags & JOB_MODE_MASK);
    const unsigned c = job.tpc_shift >= 32 ? tile : (__umulhi(tile, job.tpc_magic) >> job.tpc_shift);
    const int ts = (int)(tile - c * job.tiles_per_channel) * TW;
    const unsigned short *__restrict__ row = static_cast<const unsigned short *>(job.in) + (long long)c * job.in_ld;
    char *const slab_row = slab + slab_vec_off<VPL>(lane);
    auto row_vec = [&](int s) -> VT * { return reinterpret_cast<VT *>(slab_row + s * (16 * (64 + 64 / VPL))); };

    // ---- stage tile + halo into the slab: sg1d_tile_body's out-of-place staging, sample for sample, widened on the way ----
    if ((job.flags & JOB_VEC_IN) && ts - NA >= 0 && ts + TW + NA <= L) {
        const u32x2 *src = reinterpret_cast<const u32x2 *>(row + (ts - NA));  // slab vector v <-> the 8 bytes of samples ts - NA + 4 v ..
        u32x2 p[VPL + 1];
#pragma unroll
        for (int s = 0; s < VPL; ++s) p[s] = __builtin_nontemporal_load(src + lane + 64 * s);
        if (lane < 2 * HV) p[VPL] = src[TV + lane];                       // halo: re-read by the neighbour tile, keep it cached
        if (ibf) {
#pragma unroll
            for (int s = 0; s < VPL; ++s) *row_vec(s) = widen4_bf16(p[s]);
            if (lane < 2 * HV) *row_vec(VPL) = widen4_bf16(p[VPL]);
        } else {
#pragma unroll
            for (int s = 0; s < VPL; ++s) *row_vec(s) = widen4_f16(p[s]);
            if (lane < 2 * HV) *row_vec(VPL) = widen4_f16(p[VPL]);
        }
    } else {
        // channel ends, short rows, rows without 8-byte alignment: vectors that lie wholly inside the row are still moved as vectors; the rest (the part
        // of the halo that sticks out of the row, remapped per boundary mode; everything if the row is unaligned) goes element by element
        const bool vec = (job.flags & JOB_VEC_IN) != 0;
        const int lim = L + NA;
#pragma unroll
        for (int s = 0; s < VPL + 1; ++s) {
            const int v = lane + 64 * s;
            const int g0 = ts - NA + v * E;
            if (v < K::SV && vec && g0 >= 0 && g0 + E <= L) {
                const u32x2 raw = *reinterpret_cast<const u32x2 *>(row + g0);
                *reinterpret_cast<VT *>(slab + slab_vec_off<VPL>(v)) = ibf ? widen4_bf16(raw) : widen4_f16(raw);
            }
        }
#pragma unroll 4
        for (int e = lane; e < K::SL; e += 64) {
            int g = ts - NA + e;
            const int g0 = g - (e % E);
            const bool direct = vec && g0 >= 0 && g0 + E <= L;
            if (!direct) {
                float x = 0.0f;                                          // beyond L + NA: zero-filled, as in sg1d_tile_body
                if (g < lim) {
                    bool zero = false;
                    if (g < 0 || g >= L) g = remap_index(g, L, mode, zero);
                    if (!zero) x = widen1(row[g], ibf);
                }
                *reinterpret_cast<float *>(slab + slab_vec_off<VPL>(e / E) + (e % E) * (int)sizeof(float)) = x;
            }
        }
    }
    wave_lds_sync();

    // ---- derivative filters (JOB_CENTRE): centre the tile on the mean of its body, sg1d_tile_body's code ----
    float centre = 0.0f;
    if (job.flags & JOB_CENTRE) {                          // uniform
        VT p[VPL + 1];
        float part = 0.0f;
#pragma unroll
        for (int s = 0; s < VPL + 1; ++s) {
            if (s < VPL || lane < 2 * HV) {
                p[s] = *row_vec(s);
                const int v = lane + 64 * s;
                if (v >= HV && v < HV + TV) {
#pragma unroll
                    for (int e = 0; e < E; ++e) part += vget(p[s], e);
                }
            }
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) part += __shfl_xor(part, o);
        centre = part * (1.0f / float(TW));
        if (!(centre - centre == 0.0f)) centre = 0.0f;     // Inf / NaN in the tile: leave it as it is
#pragma unroll
        for (int s = 0; s < VPL + 1; ++s) {
            if (s < VPL || lane < 2 * HV) {
#pragma unroll
                for (int e = 0; e < E; ++e) vset(p[s], e, vget(p[s], e) - centre);
                *row_vec(s) = p[s];
            }
        }
        wave_lds_sync();
    }

    // ---- the convolution: lane owns outputs [lane*R, lane*R + R) of the tile ----
    float acc[R];
    CV::run(slab + 16 * (lane * (VPL + 1)), taps, acc, job.flags);
    if (job.flags & JOB_CENTRE) {
        const float back = centre * job.centre_sum;
#pragma unroll
        for (int r = 0; r < R; ++r) acc[r] += back;
    }
    if (job.flags & JOB_SCALE) {
        const float s = job.dt_inv;
#pragma unroll
        for (int r = 0; r < R; ++r) acc[r] *= s;
    }
    wave_lds_sync();                                   // all window reads done before overwrite

    // ---- results back through the slab (the swizzled result layout), then coalesced rows to HBM in the output type ----
    {
        const int wbase = 128 * lane + 16 * (lane & 7);
#pragma unroll
        for (int s = 0; s < VPL; ++s) *reinterpret_cast<VT *>(slab + (wbase ^ (16 * s))) = float4{acc[4 * s], acc[4 * s + 1], acc[4 * s + 2], acc[4 * s + 3]};
    }
    wave_lds_sync();
    const int lo = (int)job.store_lo, hi = (int)job.store_hi;
    const bool whole = (job.flags & JOB_VEC_OUT) && ts >= lo && ts + TW <= hi;
    const bool vec = (job.flags & JOB_VEC_OUT) != 0;
    if (jh.out_type == STORE_F32) {
        // fp32 output: sg1d_tile_body's store
        float *__restrict__ orow = static_cast<float *>(job.out) + (long long)c * job.out_ld - (long long)job.out_shift;
        if (whole) {
            const char *const rbase = slab + result_vec_off8(lane);
#pragma unroll
            for (int s = 0; s < VPL; ++s) st_stream(reinterpret_cast<VT *>(orow + ts) + lane + 64 * s, *reinterpret_cast<const VT *>(rbase + 1024 * s));
        } else {
#pragma unroll
            for (int s = 0; s < VPL; ++s) {
                const int p = lane + 64 * s;
                const int g0 = ts + p * E;
                const VT o = *reinterpret_cast<const VT *>(slab + result_vec_off8(p));
                if (vec && g0 >= lo && g0 + E <= hi) {
                    *reinterpret_cast<VT *>(orow + g0) = o;
                } else {
#pragma unroll
                    for (int e = 0; e < E; ++e)
                        if (g0 + e >= lo && g0 + e < hi) orow[g0 + e] = vget(o, e);
                }
            }
        }
    } else {
        const bool obf = jh.out_type == STORE_BF16;
        unsigned short *__restrict__ orow = static_cast<unsigned short *>(job.out) + (long long)c * job.out_ld - (long long)job.out_shift;
        if (whole) {
            const char *const rbase = slab + result_vec_off8(lane);
            u32x2 *dst = reinterpret_cast<u32x2 *>(orow + ts) + lane;     // result vector lane + 64 s -> the 8 bytes of outputs ts + 4 (lane + 64 s) ..
            if (obf) {
#pragma unroll
                for (int s = 0; s < VPL; ++s) __builtin_nontemporal_store(narrow4_bf16(*reinterpret_cast<const VT *>(rbase + 1024 * s)), dst + 64 * s);
            } else {
#pragma unroll
                for (int s = 0; s < VPL; ++s) __builtin_nontemporal_store(narrow4_f16(*reinterpret_cast<const VT *>(rbase + 1024 * s)), dst + 64 * s);
            }
        } else {
            // first / last tile of a channel (the stored range ends inside it) or output rows without 8-byte alignment
#pragma unroll
            for (int s = 0; s < VPL; ++s) {
                const int p = lane + 64 * s;
                const int g0 = ts + p * E;
                const VT o = *reinterpret_cast<const VT *>(slab + result_vec_off8(p));
                if (vec && g0 >= lo && g0 + E <= hi) {
                    *reinterpret_cast<u32x2 *>(orow + g0) = obf ? narrow4_bf16(o) : narrow4_f16(o);
                } else {
#pragma unroll
                    for (int e = 0; e < E; ++e)
                        if (g0 + e >= lo && g0 + e < hi) orow[g0 + e] = narrow1(vget(o, e), obf);
                }
            }
        }
    }
}

// the plain sliding dot product on the narrow tile (sg1d_center_kernel<float, N, 8>'s arithmetic)
template <int N>
__global__ __launch_bounds__(64 * SG_K1D_WAVES, (K1D<float, N, VPL_NARROW>::MIN_WAVES)) void sg1d_h16_kernel(const JobH16 job, const Taps taps)
{
    sg1d_h16_body<N, DirectConv<float, N, VPL_NARROW>>(job, taps);
}

}  // namespace sg
