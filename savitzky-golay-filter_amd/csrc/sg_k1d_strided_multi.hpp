// sg_k1d_strided_multi.hpp -- sg1d_strided_multi_kernel<N>: several fields of an array of structs filtered in ONE pass over the records
// (savgol_apply_strided_multi_batch_f32).  The single kernel (sg1d_strided_kernel, sg_k1d.hpp) gathers one 4-byte field per call, so F fields pull the
// whole records through HBM F times; here a record line crosses HBM once per launch.
//
// A tile (2048 records + halo) is far larger than L1, and the resident tiles of an XCD are several times its L2 at 32-byte records, so "gather field 0,
// convolve, scatter, gather field 1, ..." inside a wave would re-read from beyond L2.  Instead the wave STAGES ALL ITS FIELDS FIRST, chunk by chunk
// (64 records): the dword loads of fields 0 .. K-1 of a chunk are issued back to back -- they touch the same lines, so all but the first hit in L1 or
// merge with the miss in flight -- several chunks in flight, into K slabs of the dense kernel's layout (one per job, the single kernel's `mine` / KSTEP
// addressing).  Then, per job, the single kernel's sequence word for word -- Conv<float, N, VPL_NARROW> on job k's slab with job k's taps, JOB_SCALE
// with its dt_inv, the results back into the slab -- and the scatter, again chunk by chunk with the K dword stores of a record back to back.
// Every output is the single call's bit for bit: same staging values, same inner product, same scale, same stored range.
//
// The job count is a run-time argument: the inner product is compiled once per half window (a loop over jobs, taps fetched from the kernel arguments
// by job index), only the small staging / scatter loops exist per job count.  One wave per block; its LDS is njobs slabs, sized per launch
// (19 / 28.5 / 38 KB for 2 / 3 / 4 jobs: 8 / 5 / 4 waves per CU).
#pragma once

#include "sg_k1d.hpp"
#include "sg_k1d_strided_multi_launch.hpp"

namespace sg {

template <int N>
struct StridedMulti {
    typedef K1D<float, N, VPL_NARROW> K;
    static_assert(K::VPL == 8, "the element <-> slab offset split is written for 8 vectors per lane (sg1d_strided_kernel)");
    static constexpr int KSTEP = 16 * 18;                                 // 16 vectors + 2 pads per 64 elements
    static constexpr int NK = (K::SL + 63) / 64;                          // chunks of tile + halo
    static constexpr int CG = 17;                                         // chunks in flight: CG * KJ loads per lane before the first LDS write (two rounds per tile)
    // waves per SIMD the registers must allow: the slabs hold 8 waves per CU at two jobs and fewer beyond, so two is all the LDS ever admits
    static constexpr int MIN_WAVES = 2;

    // ---- stage a tile whose halo lies inside the row: element i = lane + 64 k of tile + halo, fields 0 .. KJ-1 of its record back to back ----
    template <int KJ>
    static __device__ __forceinline__ void stage_full(const JobStridedMulti &job, const char *p, char *mine, int lane)
    {
        const long long stride = job.grid.in_stride;
#pragma unroll
        for (int k0 = 0; k0 < NK; k0 += CG) {
            float x[CG][KJ];
#pragma unroll
            for (int kk = 0; kk < CG; ++kk) {
                const int k = k0 + kk;
                if (k < NK && lane + 64 * k < K::SL) {
#pragma unroll
                    for (int f = 0; f < KJ; ++f) x[kk][f] = *reinterpret_cast<const float *>(p + job.in_off[f] + (long long)(64 * k) * stride);
                }
            }
#pragma unroll
            for (int kk = 0; kk < CG; ++kk) {
                const int k = k0 + kk;
                if (k < NK && lane + 64 * k < K::SL) {
#pragma unroll
                    for (int f = 0; f < KJ; ++f) *reinterpret_cast<float *>(mine + f * K::SLAB + k * KSTEP) = x[kk][f];
                }
            }
        }
    }

    // ---- results out of the slabs: element lane + 64 k of the tile -> fields 0 .. KJ-1 of its record back to back ----
    template <int KJ>
    static __device__ __forceinline__ void scatter(const JobStridedMulti &job, char *q, const char *mine, int ts, int lane)
    {
        const long long stride = job.grid.out_stride;
        const int lo = (int)job.grid.store_lo, hi = (int)job.grid.store_hi;
        if (ts >= lo && ts + K::TW <= hi) {
#pragma unroll 8
            for (int k = 0; k < K::TW / 64; ++k) {
#pragma unroll
                for (int f = 0; f < KJ; ++f)
                    *reinterpret_cast<float *>(q + job.out_off[f] + (long long)(64 * k) * stride) = *reinterpret_cast<const float *>(mine + f * K::SLAB + k * KSTEP);
            }
        } else {
#pragma unroll 4
            for (int k = 0; k < K::TW / 64; ++k) {
                const int g = ts + lane + 64 * k;
                if (g >= lo && g < hi) {
#pragma unroll
                    for (int f = 0; f < KJ; ++f)
                        *reinterpret_cast<float *>(q + job.out_off[f] + (long long)(64 * k) * stride) = *reinterpret_cast<const float *>(mine + f * K::SLAB + k * KSTEP);
                }
            }
        }
    }
};

template <int N>
__global__ __launch_bounds__(64, (StridedMulti<N>::MIN_WAVES)) void sg1d_strided_multi_kernel(const JobStridedMulti job, const TapsStridedMulti taps)
{
    typedef K1D<float, N, VPL_NARROW> K;
    typedef StridedMulti<N> M;
    constexpr int R = K::R, TW = K::TW, NA = K::NA, VPL = K::VPL;
    extern __shared__ __attribute__((aligned(16))) char smem[];            // njobs slabs of K::SLAB bytes (a multiple of 16)
    const int lane = threadIdx.x & 63;
    const JobStrided &grid = job.grid;
    const int nj = (int)job.njobs;

    const unsigned nb8 = gridDim.x >> 3;
    unsigned tile = blockIdx.x;                                           // one wave per block: block = tile
    if (tile < nb8 * 8u) tile = (tile & 7u) * nb8 + (tile >> 3);
    if (tile >= grid.total_tiles) {                                       // wave-uniform: past the tiles come the edge items, end e of job k at e * njobs + k
        const unsigned item = tile - grid.total_tiles;
        if (item < grid.edge_items) {
            const unsigned e = nj == 2 ? item >> 1 : nj == 3 ? item / 3u : item >> 2, k = item - e * (unsigned)nj;
            JobStrided view = grid;                                       // job k's single call on these channels
            view.in = grid.in + job.in_off[k];
            view.out = grid.out + job.out_off[k];
            view.dt_inv = job.dt_inv[k];
            view.flags = job.flags[k];
            view.edges = job.edges[k];
            sg1d_edge_item<N>(view, e, lane);
        }
        return;
    }
    const int L = (int)grid.length;
    const unsigned c = tile_channel(grid, tile);
    const int ts = (int)(tile - c * grid.tiles_per_channel) * TW;
    const char *__restrict__ row = grid.in + (long long)c * grid.in_pitch;
    char *__restrict__ orow = grid.out + (long long)c * grid.out_pitch;
    char *const mine = smem + 16 * ((lane >> 2) + (lane >> 5)) + 4 * (lane & 3);       // slab 0's; job f's is K::SLAB * f further

    // ---- stage tile + halo of every job's field: sample g = ts - NA + i of this channel ----
    if (ts - NA >= 0 && ts + TW + NA <= L) {
        const char *p = row + (long long)(ts - NA + lane) * grid.in_stride;
        if (nj == 2) M::template stage_full<2>(job, p, mine, lane);
        else if (nj == 3) M::template stage_full<3>(job, p, mine, lane);
        else M::template stage_full<4>(job, p, mine, lane);
    } else {
        // channel ends: the single kernel's remap path, job by job with job f's mode
#pragma unroll 1
        for (int f = 0; f < nj; ++f) {
            const int mode = (int)(job.flags[f] & JOB_MODE_MASK);
            const char *frow = row + job.in_off[f];
            char *fmine = mine + f * K::SLAB;
#pragma unroll 4
            for (int k = 0; k < M::NK; ++k) {
                const int i = lane + 64 * k;
                int g = ts - NA + i;
                if (i < K::SL && g < L + NA) {
                    bool zero = false;
                    if (g < 0 || g >= L) g = remap_index(g, L, mode, zero);
                    const float x = zero ? 0.0f : *reinterpret_cast<const float *>(frow + (long long)g * grid.in_stride);
                    *reinterpret_cast<float *>(fmine + k * M::KSTEP) = x;
                }
            }
        }
    }
    wave_lds_sync();

    // ---- per job: the single kernel's inner product, scale and results back into the job's slab ----
#pragma unroll 1
    for (int f = 0; f < nj; ++f) {
        char *slab = smem + f * K::SLAB;
        float acc[R];
        Conv<float, N, VPL_NARROW>::run(slab + 16 * (lane * (VPL + 1)), taps.t[f], acc);
        if (job.flags[f] & JOB_SCALE) {
            const float dt_inv = job.dt_inv[f];
#pragma unroll
            for (int r = 0; r < R; ++r) acc[r] *= dt_inv;
        }
        wave_lds_sync();                               // all window reads done before overwrite
#pragma unroll
        for (int s = 0; s < VPL; ++s)
            *reinterpret_cast<float4 *>(slab + 16 * (lane * (VPL + 1) + s)) = float4{acc[4 * s], acc[4 * s + 1], acc[4 * s + 2], acc[4 * s + 3]};
        wave_lds_sync();
    }

    char *q = orow + (long long)(ts + lane) * grid.out_stride;
    if (nj == 2) M::template scatter<2>(job, q, mine, ts, lane);
    else if (nj == 3) M::template scatter<3>(job, q, mine, ts, lane);
    else M::template scatter<4>(job, q, mine, ts, lane);
}

}  // namespace sg
