// sg_stream_dma_body.inc -- the BODY tile of the stream block push, once: the LDS-DMA tile of bands >= 2 of a call on 16-bit rows, with K >= 1 outputs
// from one trip of each row through the wave's LDS ring.  A FRAGMENT, as sg_stream_dma_feed.hpp is: the statements of a kernel, included as the whole body
// of sg_bank_dma_{h16,i16}_kernel (K = 1; sg_stream_dma_st16.hip) and of sg_bank_dma_multi_{h16,i16}_kernel (K = 2, 3; sg_stream_dma_multi_st16.hip).  Not a function
// template: hipcc optimises a __device__ function on its own before it inlines it, with the job behind a pointer, and the kernels then come out with
// commuted address arithmetic and other registers (745 of 5177 instructions at n = 2, three outputs); included, every kernel compiles the tokens it
// always did (profiles/stream_body_isa_diff.txt: every kernel reads `same`).  The including scope provides
//   constexpr int N, K, TRT, WPB, DP, FCH, MOM; constexpr bool FMA; F (the storage family: H16StreamFamily or I16StreamFamily, sg_stream_st16.hpp);
//   job (BankJobH16 or BankJobMultiH16: the same fields, the per-output ones arrays), all (the taps: body_taps, sg_stream_dma_body.hpp), geo (TileGeom).
// DP: the ring, in DMAs = KiB = four rows each.
//
// A body tile is the twin's tile of the same band and strip -- 128 streams x 32 ticks, the fp32 call's tile order.  What sets it apart from
// sg_bank_dma_kernel (sg_stream_dma.hip), and why that kernel is not built from this file: every row it reads is one of the call's own rows (the head, two
// bands, covers the 2n <= 64 rows a body tile reaches back to: no ring history, no spread centre) and every tick has an output (no counters).
//   * rows: a row is 256 bytes, one global_load_lds_dwordx4 moves FOUR rows (lane l: row l >> 4, 16-byte chunk l & 15); a lane takes its two streams out
//     of the slab with ONE 4-byte LDS read and widens them exactly (bf16: a shift and a mask; fp16: the hardware convert), ONCE per row for every output;
//   * ROWS = 32 + 2n is rounded up to whole DMAs (odd n: two pad rows, loaded from a clamped, valid address and never fed); rows past the call's last
//     tick (the last band) take the last row's address and finish no output;
//   * the widened pair goes into output k's accumulators with output k's taps through the fragment every stream tile's `feed` is made of
//     (sg_stream_dma_feed.hpp, included once per output): output k's fp32 value is its twin's by construction;
//   * centred tiles (block moments, the fused bank): the sum of the tile's first eight widened rows is taken once out of LDS; output k runs on x - cen_k,
//     cen_k = that centre where output k's filter is a derivative (job.centre[k]), else 0 -- a smoothing bank and a derivative bank share a launch;
//   * a finished output row issues K stores (DmaQueue<N, 32, DP, 4, K>, sg_stream_host.hpp; tests/mock/dma_queue_multi_h16.cpp): 16 -> 16 bit rounds the
//     pair once to nearest even into one dword, 16 bit -> fp32 keeps the fp32 store; range-checked descriptors, nontemporal like the fp32 tile's.
// The block-moment form (MOM > 0) is the single call's (K = 1) alone.
// STORAGE is the family F's: its widen2 and narrow2 are the converts of the three places below that know the element type.  h16 (sg_h16.hpp): fp16 /
// bf16 by the job's wave-uniform types.  i16 (sg_i16.hpp): the widen is the exact sign-extending convert of the dword's two halves and a 16-bit output
// row is rounded to nearest even, saturated and packed once (NaN gives 0); in_type / out_type then only tell a 16-bit output row from an fp32 one, and
// the output step asks for the 16-bit store first (F::STORE16_FIRST: the same two stores, one per output row).
    typedef DmaQueue<N, TRT, DP, 4, K> Q;
    constexpr int TR = TRT, ROWS = TR + 2 * N, NI = Q::NI, RB = 256, RING = DP * 1024;
    static_assert(DP >= 2 && DP <= NI, "ring of row quads; the first eight rows are in it together");
    static_assert(2 * N <= 64, "the head (two bands) covers every row a body tile reaches back to");
    static_assert(K >= 1, "outputs per launch");
    static_assert(MOM == 0 || K == 1, "the block moments are the single call's");
    extern __shared__ __attribute__((aligned(1024))) char lds[];
    const int lane = threadIdx.x & 63;
    const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const TileAt at = tile_of(geo, xcd_block(false) * WPB + (unsigned)wv);
    if (!at.ok) return;
    const unsigned strip = at.strip;
    const long long t0 = (long long)(at.band + job.band0) * TR;                                   // >= 2N: row 0 of the slab is tick t0 - 2N >= 0 of this call
    const unsigned ring = (unsigned)(uintptr_t)((__attribute__((address_space(3))) char *)lds) + (unsigned)wv * (unsigned)RING;   // LDS byte address, wave-uniform
    const int sub = lane >> 4, chunk = lane & 15;                                                 // row of the quad, 16-byte chunk (8 streams) of the row
    const size_t col = (size_t)strip * 128 + (size_t)chunk * 8;
    const bool ibf = job.in_type == H16_STORE_BF16, obf = job.out_type == H16_STORE_BF16, of32 = job.out_type == H16_STORE_F32;   // uniform

    // source of row quad i: slab row r = tick t0 - 2N + r; rows past the call's last tick (the last band, pad rows) take the last row's address
    const long long last = (long long)job.ticks - 1;
    const bool inside = t0 - 2 * N + 4 * NI <= (long long)job.ticks;                              // uniform
    const unsigned short *const p0 = job.samples + (size_t)(t0 - 2 * N + (inside ? sub : 0)) * job.streams + col;
    const size_t pstep = 4 * job.streams;
    auto issue = [&](auto ic) {
        constexpr int i = decltype(ic)::value;
        const unsigned short *src;
        if (inside) {
            src = p0 + (size_t)i * pstep;
        } else {
            long long h = t0 - 2 * N + 4 * i + sub;
            h = h > last ? last : h;
            src = job.samples + (size_t)h * job.streams + col;
        }
        dma16(reinterpret_cast<const float *>(src), ring + (unsigned)(i % DP) * 1024u);
    };
    static_for<DP>([&](auto ic) -> bool { issue(ic); return true; });

    // ---- consume the rows in arrival order ----
    const char *mine = lds + (size_t)wv * RING + lane * 4;
    const unsigned voff = strip * 128u + 2u * (unsigned)lane;                                     // this lane's first stream
    constexpr int CH = MOM ? 1 : (FMA ? FCH : 1);
    f32x2 accs[K][CH][TR];
    f32x2 mom[MOM > 0 ? MOM : 1];
    f32x2 cens[K], backdts[K];
    static_for<K>([&](auto kc) -> bool { cens[decltype(kc)::value] = f32x2{0.0f, 0.0f}; backdts[decltype(kc)::value] = f32x2{0.0f, 0.0f}; return true; });
    auto row_in = [&](auto rc) -> unsigned {
        constexpr int r = decltype(rc)::value;
        return *reinterpret_cast<const unsigned *>(mine + ((r / 4) % DP) * 1024 + (r & 3) * RB);
    };
    // one arriving row into output k: the tiles' `feed`, bound to output k's accumulators, taps and (centred) sample pair
    auto feed = [&](auto kc, auto rc, const f32x2 x) {
        constexpr int k = decltype(kc)::value, r = decltype(rc)::value;
        f32x2 (&acc)[CH][TR] = accs[k];
        const auto &taps = body_taps<k>(all);
#include "sg_stream_dma_feed.hpp"
        if constexpr (r >= 2 * N && r - 2 * N < TR) {                                             // output m = r - 2N has seen its last row
            constexpr int m = r - 2 * N;
            const long long tt = t0 + m;
            const bool has_out = tt <= last;                                                      // uniform
            // the fp32 tile's output step: the chains' sum; centred tiles: (a + c * sum_k w_k) * dt_inv in one multiply-add
            f32x2 a = acc[0][m];
            if constexpr (CH == 2) a = a + acc[1][m];
            const f32x2 y = (MOM > 0 || FMA) ? __builtin_elementwise_fma(a, f32x2{job.dt_inv[k], job.dt_inv[k]}, backdts[k]) : a * f32x2{job.dt_inv[k], job.dt_inv[k]};
            const size_t orow = (size_t)(has_out ? tt : 0) * job.streams;
            // one store per output and output row whatever the type (the queue arithmetic is static); a row past the call stores into an empty descriptor
            // (the family's order: with STORE16_FIRST the 16-bit store is asked for first -- the same two stores, written out: behind a lambda they schedule differently)
            if constexpr (F::STORE16_FIRST) {
                if (!of32) {
                    const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(static_cast<unsigned short *>(job.out[k]) + orow, 0, has_out ? (int)(job.streams * 2) : 0, 0x00020000);
                    __builtin_amdgcn_raw_buffer_store_b32(F::narrow2(y, obf), rs, (int)(voff * 2u), 0, 2);
                } else {
                    const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(static_cast<float *>(job.out[k]) + orow, 0, has_out ? (int)(job.streams * 4) : 0, 0x00020000);
                    __builtin_amdgcn_raw_buffer_store_b64(__builtin_bit_cast(u32x2, y), rs, (int)(voff * 4u), 0, 2);
                }
            } else {
                if (of32) {
                    const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(static_cast<float *>(job.out[k]) + orow, 0, has_out ? (int)(job.streams * 4) : 0, 0x00020000);
                    __builtin_amdgcn_raw_buffer_store_b64(__builtin_bit_cast(u32x2, y), rs, (int)(voff * 4u), 0, 2);
                } else {
                    const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(static_cast<unsigned short *>(job.out[k]) + orow, 0, has_out ? (int)(job.streams * 2) : 0, 0x00020000);
                    __builtin_amdgcn_raw_buffer_store_b32(F::narrow2(y, obf), rs, (int)(voff * 2u), 0, 2);
                }
            }
        }
    };
    // the centre of the centred outputs: the sum of the tile's first eight widened rows (all real samples here), once, out of LDS after two DMAs have landed
    if constexpr (MOM > 0 || FMA) {
        bool any = false;                                    // uniform
        static_for<K>([&](auto kc) -> bool { any = any || job.centre[decltype(kc)::value] != 0; return true; });
        if (any) {
            f32x2 sum = f32x2{0.0f, 0.0f};
            wait_vm<(Q::younger(1, 0) > 63 ? 63 : Q::younger(1, 0))>();
            static_for<8>([&](auto rc) -> bool { sum = sum + F::widen2(row_in(rc), ibf); return true; });
            const f32x2 cen = centre_guard(sum);
            static_for<K>([&](auto kc) -> bool {
                constexpr int k = decltype(kc)::value;
                if (job.centre[k]) {                         // uniform; smoothing filters keep cen_k = 0
                    cens[k] = cen;
                    backdts[k] = cen * f32x2{job.centre_sum[k] * job.dt_inv[k], job.centre_sum[k] * job.dt_inv[k]};
                }
                return true;
            });
        }
    }
    wait_vm<(Q::younger(0, 0) > 63 ? 63 : Q::younger(0, 0))>();
    unsigned x0 = row_in(std::integral_constant<int, 0>{}), x1 = row_in(std::integral_constant<int, 1>{}),
             x2 = row_in(std::integral_constant<int, 2>{}), x3 = row_in(std::integral_constant<int, 3>{});
    // Step g consumes quad g (already in x0..x3, still packed) for every output, after it has waited for quad g + 1 and issued its LDS reads, and ends by
    // issuing DMA g + DP into the ring slot quad g has just left.  A row without an output still issues its K stores (into empty descriptors): the queue
    // is static.
    static_for<NI>([&](auto gc) -> bool {
        constexpr int g = decltype(gc)::value;
        unsigned n0 = x0, n1 = x1, n2 = x2, n3 = x3;
        if constexpr (g + 1 < NI) {
            wait_vm<(Q::younger(g + 1, g) > 63 ? 63 : Q::younger(g + 1, g))>();
            n0 = row_in(std::integral_constant<int, 4 * g + 4>{});
            n1 = row_in(std::integral_constant<int, 4 * g + 5>{});
            n2 = row_in(std::integral_constant<int, 4 * g + 6>{});
            n3 = row_in(std::integral_constant<int, 4 * g + 7>{});
            __builtin_amdgcn_sched_barrier(0);                                                    // keep these reads AHEAD of quad g's arithmetic
        }
        auto take = [&](auto rc, const unsigned raw) {
            constexpr int r = decltype(rc)::value;
            if constexpr (r < ROWS) {                                                             // pad rows are never fed
                const f32x2 wide = F::widen2(raw, ibf);                                           // once per row, for every output
                static_for<K>([&](auto kc) -> bool {
                    if constexpr (MOM > 0 || FMA) feed(kc, rc, wide - cens[decltype(kc)::value]);
                    else feed(kc, rc, wide);
                    return true;
                });
            }
        };
        take(std::integral_constant<int, 4 * g>{}, x0);
        take(std::integral_constant<int, 4 * g + 1>{}, x1);
        take(std::integral_constant<int, 4 * g + 2>{}, x2);
        take(std::integral_constant<int, 4 * g + 3>{}, x3);
        if constexpr (g + DP < NI) {
            // quad g's slot is free once its LDS reads have returned: drain the LDS queue before the DMA may overwrite the slot
            __builtin_amdgcn_sched_barrier(0);
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            issue(std::integral_constant<int, g + DP>{});
        }
        x0 = n0; x1 = n1; x2 = n2; x3 = n3;
        return true;
    });
