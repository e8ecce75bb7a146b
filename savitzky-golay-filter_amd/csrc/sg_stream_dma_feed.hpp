// sg_stream_dma_feed.hpp -- ONE arriving row of an LDS-DMA stream tile goes into every accumulator it touches: the three summation forms (block moments,
// the fused bank's chains, the reference's order) of sg_bank_dma_kernel (sg_stream_dma.hip) and the body tile (sg_stream_dma_body.inc).
// A FRAGMENT, not a header of declarations: it is included inside the body of each kernel's `feed` lambda, so both kernels compile the same tokens and
// the fp32 kernel compiles the tokens it always did (profiles/stream_h16_isa_diff.txt: every existing kernel reads `same`).  The including scope provides
//   constexpr int N, TR, CH, MOM; constexpr bool FMA; constexpr int r (the slab row: tap r - m of output m);
//   taps (SRollTaps<N> or MomTaps<N, MOM>), f32x2 acc[CH][TR], f32x2 mom[MOM > 0 ? MOM : 1], const f32x2 x (the lane's sample pair, centred where the tile is).
        constexpr int mlo = r - 2 * N > 0 ? r - 2 * N : 0, mhi = r < TR - 1 ? r : TR - 1;
        if constexpr (MOM > 0) {
            typedef MomGeom<N> G;
            static_assert(N >= 8, "head taps (k <= 6) and tail taps (k >= 2N - 6) must not meet");
            constexpr int j = r / G::BK, t = r % G::BK;
            // the block's moments (tap-free: shared by every output that takes this block whole)
            if constexpr (t == 0) {
                mom[0] = x;
                static_for<MOM - 1>([&](auto sc) -> bool { constexpr int sm = decltype(sc)::value; mom[sm + 1] = pk_mul_sgpr<(t & 1)>(taps.q[sm][t >> 1], x); return true; });
            } else {
                mom[0] = mom[0] + x;
                static_for<MOM - 1>([&](auto sc) -> bool { constexpr int sm = decltype(sc)::value; pk_fma_sgpr<(t & 1)>(mom[sm + 1], taps.q[sm][t >> 1], x); return true; });
            }
            // rows before an output's first / after its last whole block: tap by tap
            static_for<mhi - mlo + 1>([&](auto ic) -> bool {
                constexpr int m = mlo + decltype(ic)::value, k = r - m;
                if constexpr (G::direct(m, r)) {
                    constexpr bool is_head = k < G::BK;
                    constexpr int kk = is_head ? k : k - (2 * N - (G::BK - 1));
                    static_assert(kk >= 0 && kk < 8, "direct taps sit within 7 of either end of the window");
                    if constexpr (k == 0) acc[0][m] = pk_mul_sgpr<(kk & 1)>(taps.head[kk >> 1], x);                    // m % 8 != 0: the output's first term
                    else if constexpr (is_head) pk_fma_sgpr<(kk & 1)>(acc[0][m], taps.head[kk >> 1], x);
                    else pk_fma_sgpr<(kk & 1)>(acc[0][m], taps.tail[kk >> 1], x);
                }
                return true;
            });
            // a block is complete: its share of every output that takes it whole
            if constexpr (t == G::BK - 1) {
                static_for<mhi - mlo + 1>([&](auto ic) -> bool {
                    constexpr int m = mlo + decltype(ic)::value;
                    if constexpr (G::whole(m, r)) {
                        constexpr int off = G::BK * j - m;
                        static_assert(off >= 0 && off < G::NOFF, "block offset");
                        static_for<MOM>([&](auto sc) -> bool {
                            constexpr int sm = decltype(sc)::value;
                            if constexpr (sm == 0 && off == 0) acc[0][m] = pk_mul_sgpr<(off & 1)>(taps.c[0][off >> 1], mom[0]);  // m % 8 == 0: the output's first term
                            else pk_fma_sgpr<(off & 1)>(acc[0][m], taps.c[sm][off >> 1], mom[sm]);
                            return true;
                        });
                    }
                    return true;
                });
            }
        } else if constexpr (FMA) {
            static_for<mhi - mlo + 1>([&](auto ic) -> bool {
                constexpr int m = mlo + decltype(ic)::value, k = r - m;
                // two chains (even taps, odd taps), one v_pk_fma_f32 per tap: bank_roll_item's fast form, bit for bit -- or ONE chain in the
                // reference's order (taller tiles fit the registers; each term rounds once where the reference rounds twice)
                if constexpr (k < CH) acc[k][m] = pk_mul_sgpr<k>(taps.w[0], x);
                else pk_fma_sgpr<(k & 1)>(acc[(k & 1) % CH][m], taps.w[k >> 1], x);
                return true;
            });
        } else {
            // the reference's order (src/savgol_stream.c:25-38): sum = 0; sum += w[k] * x[k], k ascending, product and sum rounded separately.
            // Volatile asm for products and sums alike, each product issued one output ahead of its sum: left to the compiler, all the
            // products of a row are hoisted in front of the sums and stay live (256 registers and scratch; see bank_accroll_item)
            f32x2 p = pk_mul_tap<r - mlo>(taps, x);
            static_for<mhi - mlo + 1>([&](auto ic) -> bool {
                constexpr int m = mlo + decltype(ic)::value, k = r - m;
                f32x2 pn = p;
                if constexpr (m < mhi) pn = pk_mul_tap<k - 1>(taps, x);
                if constexpr (k == 0) asm volatile("v_pk_add_f32 %0, %1, 0 op_sel_hi:[1,0]" : "=v"(acc[0][m]) : "v"(p));       // 0 + p: a product of -0 sums to +0, as in the reference
                else                  asm volatile("v_pk_add_f32 %0, %0, %1" : "+v"(acc[0][m]) : "v"(p));
                p = pn;
                return true;
            });
        }
