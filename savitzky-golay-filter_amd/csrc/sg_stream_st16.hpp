// sg_stream_st16.hpp -- the stream block push on 16-bit STORAGE, fp32 arithmetic inside, for two storage families:
//   h16  fp16 or bf16 rows in, the same type or fp32 out   (savgol_streambank_push_block_h16, savgol_streambank_push_block_multi_h16)
//   i16  int16 rows in, int16 or fp32 out                   (savgol_streambank_push_block_i16, savgol_streambank_push_block_multi_i16)
// The by-value jobs of the body tile (sg_stream_dma_body.inc) -- one pair for both families: the samples are 16-bit words either way --, the family
// policies the tile files are compiled with (sg_stream_dma_st16.hip, sg_stream_dma_multi_st16.hip) and the launchers their objects export.  Jobs of
// their own: BankJob and BankJobMulti are the fp32 block kernels' arguments and stay as they are.
#pragma once

#include <hip/hip_runtime.h>

#include <cstddef>

#include "sg_family.hpp"
#include "sg_h16.hpp"
#include "sg_i16.hpp"
#include "sg_stream_host.hpp"
#include "sg_stream_multi.hpp"

namespace sg {

// storage types of a device buffer: the values of SAVGOL_HIP_F32 / _F16 / _BF16 (include/savgol_hip.h).  On int16 storage in_type is SAVGOL_HIP_I16
// and out_type SAVGOL_HIP_I16 or SAVGOL_HIP_F32 (= H16_STORE_F32, the one value the body tile compares out_type with there).
enum : unsigned { H16_STORE_F32 = 0, H16_STORE_F16 = 1, H16_STORE_BF16 = 2 };

// The body of a tile-route call: ticks band0 * 32 .. ticks - 1 of the call.  Every row a body tile reads is a 16-bit row of this call (band0 * 32 >=
// 2n) and every tick has an output, so neither the ring nor the counters appear.  The types are wave-uniform: scalar branches at the widen and the store.
// The per-output fields are arrays of one: the body tile (sg_stream_dma_body.inc) reads this job and BankJobMultiH16 with the same text.
struct BankJobH16 {
    const unsigned short *samples;   // [ticks][streams], 16-bit words: fp16, bf16 or int16
    void                 *out[1];    // [ticks][streams] of out_type elements
    size_t                streams, ticks;          // of the whole call
    unsigned              band0;     // the twin's band of the body's first tile (2: the head is two bands)
    float                 dt_inv[1];
    float                 centre_sum[1];           // as BankJob's
    int                   centre[1];
    unsigned              in_type;   // H16_STORE_F16 or H16_STORE_BF16; SAVGOL_HIP_I16
    unsigned              out_type;  // the input's type, or H16_STORE_F32
};

// The body of a fused call: ticks band0 * 32 .. ticks - 1 of the call, for `outputs` banks that share the 16-bit samples.  Every row a body tile reads
// is a 16-bit row of this call (band0 * 32 >= 2n) and every tick has an output, so neither the rings nor the counters appear.  One input type and one
// output type serve every output; both are wave-uniform: scalar branches at the widen and at the stores.
struct BankJobMultiH16 {
    const unsigned short *samples;                           // [ticks][streams], 16-bit words: fp16, bf16 or int16
    void                 *out[STREAM_MULTI_PER_LAUNCH];      // [ticks][streams] of out_type elements each
    size_t                streams, ticks;                    // of the whole call
    unsigned              band0;                             // the twins' band of the body's first tile (2: the head is two bands)
    float                 dt_inv[STREAM_MULTI_PER_LAUNCH];
    float                 centre_sum[STREAM_MULTI_PER_LAUNCH];   // as BankJob's, per bank
    int                   centre[STREAM_MULTI_PER_LAUNCH];
    unsigned              in_type;                           // H16_STORE_F16 or H16_STORE_BF16; SAVGOL_HIP_I16
    unsigned              out_type;                          // the input's type, or H16_STORE_F32
};

// ---- the storage families: what differs between the two, for the body tile, its two instantiation files and the host route (sg_stream.hip) ----
//   Sample                       the rows' element type
//   widen2, narrow2              a dword's two elements to fp32 and back (sg_h16.hpp, sg_i16.hpp); `bf` picks bf16 where the family has two element types
//   STORE16_FIRST                the body tile's output step asks for the 16-bit store first (the same two stores either way)
//   tile_min_waves, multi_tile_min_waves   waves per SIMD the registers of the single and of the fused tile are allocated for (the second
//                                __launch_bounds__ argument); (wpb + 3) / 4 is what a block of wpb waves implies by itself
//   multi_max_n, multi_tile_shape   the fused call's bound and shape tables (sg_stream_host.hpp: a table of its own per family)
struct H16StreamFamily {
    typedef unsigned short Sample;
    static __device__ __forceinline__ f32x2 widen2(unsigned raw, bool bf) { return sg::widen2(raw, bf); }
    static __device__ __forceinline__ unsigned narrow2(f32x2 v, bool bf) { return sg::narrow2(v, bf); }
    static constexpr bool STORE16_FIRST = false;
    static constexpr int tile_min_waves(int, int, int wpb) { return (wpb + 3) / 4; }
    static constexpr int multi_tile_min_waves(int, bool, int, int wpb) { return (wpb + 3) / 4; }
    static constexpr int multi_max_n(bool fma, int outputs) { return stream_multi_h16_max_n(fma, outputs); }
    static constexpr MultiH16TileShape multi_tile_shape(int n, bool fma, int outputs) { return multi_h16_tile_shape(n, fma, outputs); }
};
struct I16StreamFamily {
    typedef short Sample;
    static __device__ __forceinline__ f32x2 widen2(unsigned raw, bool) { return widen2_i16(raw); }
    static __device__ __forceinline__ unsigned narrow2(f32x2 v, bool) { return narrow2_i16(v); }
    // in that order the int16 narrow (two temporaries where the bf16 convert needs one) does not sit at the tile's register peak
    static constexpr bool STORE16_FIRST = true;
    // The block-moment tiles up to half window 15 are held to five, the step their 16-bit float twins compile to (at most 96 VGPRs); left alone, the
    // three-moment tile at n = 15 comes out at 98.  Every other tile keeps what a block of wpb waves implies by itself.
    static constexpr int tile_min_waves(int n, int mom, int wpb) { return mom > 0 && n <= 15 ? 5 : (wpb + 3) / 4; }
    // One tile is held to the step its 16-bit float twin compiles to: the bit-exact bank's three-output tile at n = 4, 64 VGPRs = eight waves on the
    // twin; left alone it comes out at 66, the int16 narrow's second temporary.
    static constexpr int multi_tile_min_waves(int n, bool fma, int k, int wpb) { return !fma && n == 4 && k == 3 ? 8 : (wpb + 3) / 4; }
    static constexpr int multi_max_n(bool fma, int outputs) { return stream_multi_i16_max_n(fma, outputs); }
    static constexpr MultiH16TileShape multi_tile_shape(int n, bool fma, int outputs) { return multi_i16_tile_shape(n, fma, outputs); }
};

// The launchers the ten objects export, per family f: 0 = launched, 1 = not covered (a refused launch; a half window, or an output count, outside the
// object's range).  `geo` / `grid`: block_plan_h16's, for the body.  center[k]: bank k's centre taps; `plan`: block_plan_multi_h16's or _i16's (geometry,
// grid, waves per block and ring of the body's launches).
#define SG_STREAM_ST16_LAUNCHERS(f)                                                                                                                                             \
    int sg_bank_dma_##f##_launch_mom(int n, const StreamMomentFit &fit, const float *center, const BankJobH16 &job, const TileGeom &geo, unsigned grid, hipStream_t st); /* 12..20 */ \
    int sg_bank_dma_##f##_launch_lo(int n, int fma, const float *center, const BankJobH16 &job, const TileGeom &geo, unsigned grid, hipStream_t st);                     /* 1..16 */  \
    int sg_bank_dma_##f##_launch_hi(int n, int fma, const float *center, const BankJobH16 &job, const TileGeom &geo, unsigned grid, hipStream_t st);                     /* 17..32 */ \
    int sg_bank_dma_multi_##f##_launch_fma(int n, int outputs, const float *const *center, const BankJobMultiH16 &job, const MultiPlan &plan, hipStream_t st);                  \
    int sg_bank_dma_multi_##f##_launch_ref(int n, int outputs, const float *const *center, const BankJobMultiH16 &job, const MultiPlan &plan, hipStream_t st);
SG_STREAM_ST16_LAUNCHERS(h16)
SG_STREAM_ST16_LAUNCHERS(i16)
#undef SG_STREAM_ST16_LAUNCHERS

// The tile files are compiled once per family, -DSG_FAMILY=h16|i16: `StreamFamily` is that family's policy
#ifdef SG_FAMILY
struct StreamFamilies { typedef H16StreamFamily h16; typedef I16StreamFamily i16; };
typedef StreamFamilies::SG_FAMILY StreamFamily;
#endif

}  // namespace sg
