// sg_k1d_multi.hpp -- the fused multi-output 1-D kernel (savgol_apply_multi_batch_f32): K filters of one half window and one boundary mode
// (smoothing, d/dt, d^2/dt^2, ...) on ONE read of the input.  Bytes per input sample: 4 + 4 K instead of K (4 + 4).
//
// A variant of sg1d_tile_body (sg_k1d.hpp), written beside it so that no existing kernel changes: the same narrow tile (64 lanes x 8 vectors),
// the same XCD tile order, the same staging of tile + halo into the wave's slab with the same remaps, the same inner product
// (Conv<float, N, VPL_NARROW>: three interleaved chains) once per output with that output's taps -- so output k carries the bits of the single
// call with SAVGOL_BATCH_PLAIN_SUMMATION.  Order is what keeps those bits:
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
    typedef float4 VT;
    constexpr int E = KT::E, R = KT::R, TW = KT::TW, NA = KT::NA, HV = KT::HV, VPL = KT::VPL, TV = KT::TV;
    static_assert(VPL == 8, "the result region uses the swizzled layout of 8 vectors per lane (result_vec_off8)");
    constexpr int RES = 64 * VPL * 16;                                   // bytes of one tile's results
    const Job1D &job = jm.base;

    __shared__ __attribute__((aligned(16))) char smem[KT::WAVES * (KT::SLAB + RES)];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    char *slab = smem + wave * (KT::SLAB + RES);
    char *res = slab + KT::SLAB;

    // tile order: sg1d_tile_body's (4 waves per block)
    const unsigned nb8 = gridDim.x >> 3;
    unsigned blk = blockIdx.x;
    if (blk < nb8 * 8u) {
        const unsigned cs = job.xcd_chunk_log2;
        if (cs == 0) blk = (blk & 7u) * nb8 + (blk >> 3);
        else if (cs < 32u) {
            const unsigned span = 8u << cs, q = blk >> (cs + 3u);
            if ((q + 1u) * span <= nb8 * 8u) { const unsigned r = blk & (span - 1u); blk = (((q << 3) + (r & 7u)) << cs) + (r >> 3); }
        }
    }
    const unsigned tile = blk * KT::WAVES + wave;
    if (tile >= job.total_tiles) {
        if (tile - job.total_tiles < job.edge_items) sg1d_multi_edge_item<N, K>(jm, tile - job.total_tiles, lane);
        return;
    }

    const float *__restrict__ gin = static_cast<const float *>(job.in);
    const int L = (int)job.length;
    const int mode = (int)(job.flags & JOB_MODE_MASK);
    const unsigned c = job.tpc_shift >= 32 ? tile : (__umulhi(tile, job.tpc_magic) >> job.tpc_shift);
    const int ts = (int)(tile - c * job.tiles_per_channel) * TW;
    const float *__restrict__ row = gin + (long long)c * job.in_ld;
    char *const slab_row = slab + slab_vec_off<VPL>(lane);
    auto row_vec = [&](int s) -> VT * { return reinterpret_cast<VT *>(slab_row + s * (16 * (64 + 64 / VPL))); };

    // ---- stage tile + halo into the slab: sg1d_tile_body's out-of-place staging, sample for sample ----
    if ((job.flags & JOB_VEC_IN) && ts - NA >= 0 && ts + TW + NA <= L) {
        const VT *src = reinterpret_cast<const VT *>(row + (ts - NA));
        VT p[VPL + 1];
#pragma unroll
        for (int s = 0; s < VPL; ++s) p[s] = ld_stream(src + lane + 64 * s);
        if (lane < 2 * HV) p[VPL] = src[TV + lane];                       // halo: re-read by the neighbour tile, keep it cached
#pragma unroll
        for (int s = 0; s < VPL; ++s) *row_vec(s) = p[s];
        if (lane < 2 * HV) *row_vec(VPL) = p[VPL];
    } else {
        const bool vec = (job.flags & JOB_VEC_IN) != 0;
        const int lim = L + NA;
#pragma unroll
        for (int s = 0; s < VPL + 1; ++s) {
            const int v = lane + 64 * s;
            const int g0 = ts - NA + v * E;
            if (v < KT::SV && vec && g0 >= 0 && g0 + E <= L)
                *reinterpret_cast<VT *>(slab + slab_vec_off<VPL>(v)) = *reinterpret_cast<const VT *>(row + g0);
        }
#pragma unroll 4
        for (int e = lane; e < KT::SL; e += 64) {
            int g = ts - NA + e;
            const int g0 = g - (e % E);
            const bool direct = vec && g0 >= 0 && g0 + E <= L;
            if (!direct) {
                float x = 0.0f;
                if (g < lim) {
                    bool zero = false;
                    if (g < 0 || g >= L) g = remap_index(g, L, mode, zero);
                    if (!zero) x = row[g];
                }
                *reinterpret_cast<float *>(slab + slab_vec_off<VPL>(e / E) + (e % E) * (int)sizeof(float)) = x;
            }
        }
    }
    wave_lds_sync();

    const int lo = (int)job.store_lo, hi = (int)job.store_hi;
    const char *const win = slab + 16 * (lane * (VPL + 1));
    float centre = 0.0f;
    static_for<K>([&](auto kc) {
        constexpr int k = decltype(kc)::value;
        if (k == (int)jm.nraw) {
            // ---- the first centred output: centre the slab as sg1d_tile_body does under JOB_CENTRE (after the raw outputs' window reads) ----
            wave_lds_sync();
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
            if (!(centre - centre == 0.0f)) centre = 0.0f;
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
        // ---- output k: the inner product, the centre added back, dt_inv ----
        const unsigned fk = jm.flags[k];
        float acc[R];
        Conv<float, N, VPL_NARROW>::run(win, taps.t[k], acc);
        if (fk & JOB_CENTRE) {
            const float back = centre * jm.centre_sum[k];
#pragma unroll
            for (int r = 0; r < R; ++r) acc[r] += back;
        }
        if (fk & JOB_SCALE) {
            const float s = jm.dt_inv[k];
#pragma unroll
            for (int r = 0; r < R; ++r) acc[r] *= s;
        }
        // ---- through the result region (the previous output's reads of it are done: one wave's LDS operations run in order) ----
        {
            const int wbase = 128 * lane + 16 * (lane & 7);
#pragma unroll
            for (int s = 0; s < VPL; ++s) *reinterpret_cast<VT *>(res + (wbase ^ (16 * s))) = float4{acc[4 * s], acc[4 * s + 1], acc[4 * s + 2], acc[4 * s + 3]};
        }
        wave_lds_sync();
        float *__restrict__ orow = static_cast<float *>(jm.out[k]) + (long long)c * job.out_ld - (long long)job.out_shift;
        if ((fk & JOB_VEC_OUT) && ts >= lo && ts + TW <= hi) {
            const char *const rbase = res + result_vec_off8(lane);
#pragma unroll
            for (int s = 0; s < VPL; ++s) st_stream(reinterpret_cast<VT *>(orow + ts) + lane + 64 * s, *reinterpret_cast<const VT *>(rbase + 1024 * s));
        } else {
            const bool vec = (fk & JOB_VEC_OUT) != 0;
#pragma unroll
            for (int s = 0; s < VPL; ++s) {
                const int p = lane + 64 * s;
                const int g0 = ts + p * E;
                const VT o = *reinterpret_cast<const VT *>(res + result_vec_off8(p));
                if (vec && g0 >= lo && g0 + E <= hi) {
                    *reinterpret_cast<VT *>(orow + g0) = o;
                } else {
#pragma unroll
                    for (int e = 0; e < E; ++e)
                        if (g0 + e >= lo && g0 + e < hi) orow[g0 + e] = vget(o, e);
                }
            }
        }
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
