// sg_2d_roll_st16.inc -- the additive tile form of sg_2d_roll.hip on 16-bit rows, for both storage families (sg_2d_st16.hpp): fp16 / bf16 rows
// (savgol2d_apply_batch_h16, route TILES) and int16 rows (savgol2d_apply_batch_i16, route TILES).  Not a header: an include file of one translation unit --
// sg_2d_roll.hip includes it, inside namespace sg, in its SG_ROLL_H16 and its SG_ROLL_I16 build, where it stands in for the fp32 entry points.
//
// Both kernels are sg2d_rolling_kernel<N, 2, 1, true, false, TR> with 16-bit rows at one or both ends: the same strips of Roll<N>::SW stored columns, the
// same TR-row tiles in the same XCD chunk order, 2 waves per block, the same LDS rows, and roll_item's fp32 text between its load and its store -- which
// is why their outputs are the fp32 tile's bits, rounded / converted once.
//   sg2d_rolling_h16_kernel<N, TR>           the storage types are wave-uniform fields of the job: one kernel per half window serves all four type pairs.
//   sg2d_rolling_i16_kernel<N, TR, OUT_F32>  the storage types are the kernel's own (roll_item is entered with TIN = short, TOUT = short or float): one
//                                            convert per loaded element, ONE store per row, and no finiteness vote -- an int16 frame holds nothing
//                                            non-finite (see roll_item).  16 half windows x 2 output types = 32 kernels.
//
// Waves per SIMD: the fp32 tile's (roll_tile_waves) except from F::TWO_WAVES_FROM up to n = 9, where the kernels are built for two: occupancy changes, TR,
// the strip width and the bits do not.  The fp32 tile sits at 166-168 of the 170 registers that three waves per SIMD allow there.
//   h16, n = 7, 8, 9: the 16-bit rows' raw dwords and converts do not fit beside it: 7-register spills at n = 7, 6 at n = 8, 2 at n = 9 (12-20 bytes of
//        scratch); 171 registers at n = 7 with two waves.
//   i16, n = 9 only: THREE waves at n = 7 and 8 (167 / 167-168 registers) -- without the vote, the cold paths and the second store the raw dwords fit.
//        At n = 9 three waves spill (168 registers + 2 spilled with int16 rows out, + 4 with fp32 rows out: 12 bytes of scratch).
// No kernel carries scratch (tools/kernel_resources.py lists them all; tests/test_kernel_resources.py and tests/test_i16_2d_host.py hold the library to it).
//
// The kernels' body is one text, the fragment sg_2d_roll_st16_tile.inc, included into each with its family F and its TOUT.
template <class F>
constexpr int roll_st16_waves(int n) { return (n >= F::TWO_WAVES_FROM && n <= 9) ? 2 : roll_tile_waves(n); }

template <int N, int TR>
__global__ __launch_bounds__(64 * roll_wpb(N, TR), roll_st16_waves<H16Family2D>(N)) void sg2d_rolling_h16_kernel(const Job2DH16 job, const RollTaps<N, 2, 1> taps, unsigned strips,
                                                                                                                unsigned bands, unsigned total_items, int aligned)
{
    typedef H16Family2D F;
    typedef unsigned char TOUT;
    constexpr int NT = 2;
    constexpr bool BOX = true;
#include "sg_2d_roll_st16_tile.inc"
}
template <int N, int TR, bool OUT_F32>
__global__ __launch_bounds__(64 * roll_wpb(N, TR), roll_st16_waves<I16Family2D>(N)) void sg2d_rolling_i16_kernel(const Job2DI16 job, const RollTaps<N, 2, 1> taps, unsigned strips,
                                                                                                                unsigned bands, unsigned total_items, int aligned)
{
    typedef I16Family2D F;
    typedef typename std::conditional<OUT_F32, float, short>::type TOUT;
    constexpr int NT = 2;
    constexpr bool BOX = true;
#include "sg_2d_roll_st16_tile.inc"
}
#ifdef SG_ROLL_I16_GEN
// The GENERAL one- and two-term tile on int16 rows (the y frame of savgol2d_gradient_batch_i16): sg2d_rolling_kernel<N, NT, 1, false, false, 20> with int16
// rows at one or both ends -- roll_item<N, NT, 1, MODE, false, false, 20> entered with TIN = short, at the fp32 form's waves per SIMD (roll_tile_waves(n, nt,
// false): three, two for two terms from n = 6) except the one-term tile at n = 7, which is built for two: at three it spills (168 registers + 4 spilled with
// int16 rows out, + 2 with fp32 rows out: 20 / 12 bytes of scratch); occupancy changes, the tile, the strip width and the bits do not.  7 half windows x 2
// term counts x 2 output types = 28 kernels, in objects of their own (Makefile, ROLL_GEN16_RULE).  The name matches neither the additive tiles' nor the
// staged kernels'.
constexpr int ROLL_GEN16_MAX_N = 7;
constexpr int roll_gen16_waves(int n, int nt) { return (n == 7 && nt == 1) ? 2 : roll_tile_waves(n, nt, false); }
template <int N, int NT, bool OUT_F32>
__global__ __launch_bounds__(64 * roll_wpb(N, ROLL_TILE_ROWS), roll_gen16_waves(N, NT)) void sg2d_rolling_gen_i16_kernel(const Job2DI16 job, const RollTaps<N, NT, 1> taps,
                                                                                                                   unsigned strips, unsigned bands, unsigned total_items, int aligned)
{
    typedef I16Family2D F;
    typedef typename std::conditional<OUT_F32, float, short>::type TOUT;
    constexpr int TR = roll_tile_rows(N, NT, 1, false);
    constexpr bool BOX = false;
    static_assert(TR == ROLL_TILE_ROWS && N <= ROLL_GEN16_MAX_N, "the general form's 20-row tile");
#include "sg_2d_roll_st16_tile.inc"
}
#endif
// a family's kernel for one half window (OUT_F32: which of the int16 family's two); a further family names its kernel here
template <class F, int N, int TR, bool OUT_F32>
constexpr auto roll_st16_kernel()
{
    static_assert(std::is_same<F, H16Family2D>::value || std::is_same<F, I16Family2D>::value, "no tile kernel for this storage family");
    if constexpr (std::is_same<F, I16Family2D>::value) return &sg2d_rolling_i16_kernel<N, TR, OUT_F32>;
    else return &sg2d_rolling_h16_kernel<N, TR>;
}

// launch_roll_kernel's tile geometry (TR > 0): TR rows per band whatever the batch, whole frames per launch, the XCD chunk of whole frames with at
// least 128 bands of every strip.  The caller has checked what launch_roll_kernel checks before it takes tiles (frame_plan_h16).
// (kernel: the instance to launch -- an additive tile of roll_st16_kernel, or a general tile on int16 rows)
template <int N, int TR, class F, bool OUT_F32, int NT, class KERNEL>
static int launch_roll_st16_kernel(KERNEL kernel, const Job2DSt16<F> &job, const RollTaps<N, NT, 1> &taps, unsigned images, hipStream_t st)
{
    typedef Roll<N> R;
    const unsigned strips = (unsigned)((job.cols + R::SW - 1) / R::SW);
    constexpr unsigned WPB = (unsigned)roll_wpb(N, TR);
    const size_t lds = sizeof(float) * WPB * 2 * NT * R::BUFW;
    const unsigned bands = (unsigned)((job.rows + TR - 1) / TR);
    const unsigned long long per_image = (unsigned long long)strips * bands;
    const unsigned long long max_items = ((1ull << 32) - 4096) / 64;           // a launch indexes < 2^32 threads: split over images
    unsigned long long img_step = max_items / per_image;
    if (img_step == 0) { sg_set_error("2-D frame too large for one launch (%llu items)", per_image); return -1; }
    if (img_step > images) img_step = images;
    const size_t out_elem = job.st.out_f32 ? 4 : 2;
    for (unsigned long long i0 = 0; i0 < images; i0 += img_step) {
        const unsigned long long ni = images - i0 < img_step ? images - i0 : img_step;
        const unsigned long long total = ni * per_image;
        unsigned grid = (unsigned)((total + WPB - 1) / WPB);
        grid = (grid + 7u) & ~7u;
        Job2DSt16<F> part = job;
        part.in = job.in + (long long)i0 * job.in_pitch;
        part.out = static_cast<unsigned char *>(job.out) + (size_t)i0 * (size_t)job.out_pitch * out_elem;
        int aligned_launch = 7;
        const int chunk_bands = (int)(bands * ((128u + bands - 1u) / bands));
        const unsigned long long chunk_items = (unsigned long long)chunk_bands * strips;
        if (chunk_items % WPB == 0 && chunk_items / WPB < (1u << 22) && chunk_items / WPB * 8u <= grid) aligned_launch |= (int)((unsigned)(chunk_items / WPB) << 8);
        hipLaunchKernelGGL(kernel, dim3(grid), dim3(64 * WPB), lds, st, part, taps, strips, bands, (unsigned)total, aligned_launch);
    }
    return 0;
}

// job == NULL: only whether the fp32 call takes its additive tile form for these factors (sg_2d_st16.hpp)
template <int N, class F>
static int dispatch_roll_st16(int n, const Job2DSt16<F> *job, const float *factors, float scale, unsigned images, hipStream_t st)
{
    if (n == N) {
        constexpr int TR = roll_tile_rows(N, 2, 1, true);
        if constexpr (TR > 0) {
            RollTaps<N, 2, 1> box;
            memset(&box, 0, sizeof(box));
            if (!fill_box_taps<N>(box, factors, scale) || !roll_tiles_on()) return 1;
            if (!job) return 0;
            if constexpr (F::TYPED_OUT) { if (job->st.out_f32) return launch_roll_st16_kernel<N, TR, F, true>(roll_st16_kernel<F, N, TR, true>(), *job, box, images, st); }
            return launch_roll_st16_kernel<N, TR, F, false>(roll_st16_kernel<F, N, TR, false>(), *job, box, images, st);
        } else return 1;
    }
    if constexpr (N < SEP_ROLL_MAX_N) return dispatch_roll_st16<N + 1>(n, job, factors, scale, images, st);
    else return 1;
}

#ifdef SG_ROLL_I16_GEN
// The fp32 launcher's own decisions for one output frame of `terms` terms (launch_roll): two terms that fill_box_taps accepts are the additive form's, not
// this tile's; the taps are fill_taps' (RollTaps<N, NT, 1>); tiles must be on.  job == NULL: the answer alone, nothing launched.  The caller has checked what launch_roll_kernel checks before it takes tiles.
template <int N, int NT>
static int dispatch_roll_gen16(int n, int terms, const Job2DI16 *job, const float *factors, float scale, unsigned images, hipStream_t st)
{
    if (n == N && terms == NT) {
        constexpr int TR = roll_tile_rows(N, NT, 1, false);
        if (!roll_tiles_on()) return 1;
        if constexpr (NT == 2) {
            RollTaps<N, 2, 1> box;
            memset(&box, 0, sizeof(box));
            if (fill_box_taps<N>(box, factors, scale)) return 1;
        }
        RollTaps<N, NT, 1> taps;
        memset(&taps, 0, sizeof(taps));
        if (!fill_taps<N, NT, 1>(taps, 0, factors, scale)) return 1;
        if (!job) return 0;
        if (job->st.out_f32) return launch_roll_st16_kernel<N, TR, I16Family2D, true>(&sg2d_rolling_gen_i16_kernel<N, NT, true>, *job, taps, images, st);
        return launch_roll_st16_kernel<N, TR, I16Family2D, false>(&sg2d_rolling_gen_i16_kernel<N, NT, false>, *job, taps, images, st);
    }
    if constexpr (NT < 2) return dispatch_roll_gen16<N, NT + 1>(n, terms, job, factors, scale, images, st);
    else if constexpr (N < SEP_ROLL_MAX_N) return dispatch_roll_gen16<N + 1, 1>(n, terms, job, factors, scale, images, st);
    else return 1;
}

// see sg_2d_st16.hpp (RollGen16Launch)
int SEP_ROLL_FN(int n, int terms, const Job2DI16 *job, const float *factors, float scale, unsigned images, hipStream_t st)
{
    static_assert(SEP_ROLL_MAX_N <= ROLL_GEN16_MAX_N, "built for the half windows whose general form is a 20-row tile");
    if (n < SEP_ROLL_MIN_N || n > SEP_ROLL_MAX_N || terms < 1 || terms > 2) return 1;
    return dispatch_roll_gen16<SEP_ROLL_MIN_N, 1>(n, terms, job, factors, scale, images, st);
}
#else
// see sg_2d_st16.hpp
int SEP_ROLL_FN(int n, int terms, const Job2DSt16<Roll16Family> *job, const float *factors, float scale, unsigned images, hipStream_t st)
{
    if (n < SEP_ROLL_MIN_N || n > SEP_ROLL_MAX_N || terms != 2) return 1;
    return dispatch_roll_st16<SEP_ROLL_MIN_N>(n, job, factors, scale, images, st);
}
#endif
