// sg_2d_roll_i16.inc -- the additive tile form of sg_2d_roll.hip on int16 rows (savgol2d_apply_batch_i16, route TILES).  Not a header: an include file of one translation unit --
// sg_2d_roll.hip includes it, inside namespace sg, in its SG_ROLL_I16 build, where it stands in for the fp32 entry points.
//
// sg2d_rolling_i16_kernel<N, TR, OUT_F32> is sg2d_rolling_kernel<N, 2, 1, true, false, TR> with int16 rows in and int16 (OUT_F32 = false) or fp32 rows out:
// the same strips of Roll<N>::SW stored columns, the same TR-row tiles in the same XCD chunk order, 2 waves per block, the same LDS rows, and roll_item's
// fp32 text between its load and its store -- which is why its outputs are the fp32 tile's bits, converted once.  Unlike sg2d_rolling_h16_kernel the storage
// types are the kernel's own (roll_item is entered with TIN = short, TOUT = short or float): one convert per loaded element, ONE store per row, and no
// finiteness vote -- an int16 frame holds nothing non-finite (see roll_item).  16 half windows x 2 output types = 32 kernels.
//
// Waves per SIMD: the fp32 tile's (roll_tile_waves) except at n = 9.  THREE at n = 7 and 8 (167 / 167-168 registers of the 170 three waves allow), where the
// 16-bit float tile had to fall back to two: without the vote, the cold paths and the second store the raw dwords fit beside the fp32 tile's registers.  At
// n = 9 three waves spill (168 registers + 2 spilled with int16 rows out, + 4 with fp32 rows out: 12 bytes of scratch), so both n = 9 kernels are built for two,
// as roll_h16_waves has them.  No kernel carries scratch (tools/kernel_resources.py lists them all; tests/test_kernel_resources.py and
// tests/test_i16_2d_host.py hold the library to it).
constexpr int roll_i16_waves(int n) { return n == 9 ? 2 : roll_tile_waves(n); }

template <int N, int TR, bool OUT_F32>
__global__ __launch_bounds__(64 * roll_wpb(N, TR), roll_i16_waves(N)) void sg2d_rolling_i16_kernel(const Job2DI16 job, const RollTaps<N, 2, 1> taps, unsigned strips, unsigned bands,
                                                                                                   unsigned total_items, int aligned)
{
    typedef Roll<N> R;
    typedef typename std::conditional<OUT_F32, float, short>::type TOUT;
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int lane = threadIdx.x & 63;
    const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    float *mine = lds + wv * (2 * 2 * R::BUFW);              // two LDS rows per term, private to this wave

    // the fp32 tile's block order: bits 8.. of `aligned` = blocks per XCD chunk, 0 = every XCD sweeps one contiguous eighth of the launch
    const unsigned nblk = gridDim.x;
    unsigned blk = blockIdx.x;
    const unsigned chunk = (unsigned)aligned >> 8;
    if (chunk == 0) blk = (blk & 7u) * (nblk >> 3) + (blk >> 3);
    else {
        const unsigned span = 8u * chunk, q = blk / span;
        if ((q + 1u) * span <= nblk) { const unsigned r = blk - q * span; blk = (q * 8u + (r & 7u)) * chunk + (r >> 3); }    // the last, partial span keeps launch order
    }
    constexpr unsigned WPB = (unsigned)roll_wpb(N, TR);
    const unsigned item = blk * WPB + (unsigned)wv;          // one tile per wave
    if (item >= total_items) return;

    const bool valid = job.boundary == SAVGOL2D_BOUNDARY_VALID;
    const int xlo = valid ? job.nx : 0, xhi = valid ? job.cols - job.nx : job.cols;
    const int ylo = valid ? job.ny : 0, yhi = valid ? job.rows - job.ny : job.rows;
    const unsigned strip = item % strips, ib = item / strips;
    const unsigned band = ib % bands, img = ib / bands;
    const int yb = (int)band * TR;
    const int nout = job.rows - yb < TR ? job.rows - yb : TR;
    const short *in = job.in + (long long)img * job.in_pitch;
    TOUT *outs[1];
    outs[0] = static_cast<TOUT *>(job.out) + (long long)img * job.out_pitch;
    const int sx = (int)strip * R::SW;
    // interior strips: all 256 input columns inside the frame, all SW output columns stored.  The host sends only frames whose every strip can run on
    // vector loads (frame_plan_h16), so the edge strips take the remapped quads: MODE 2 (padded modes) or 3 (VALID: partial quads).
    if (sx - 4 * R::HL >= 0 && sx - 4 * R::HL + 256 <= job.cols && sx >= xlo && sx + R::SW <= xhi)
        roll_item<N, 2, 1, 1, true, false, TR>(job, taps, mine, in, outs, sx - 4 * R::HL, yb, nout, lane, xlo, xhi, ylo, yhi);
    else if (valid) roll_item<N, 2, 1, 3, true, false, TR>(job, taps, mine, in, outs, sx - 4 * R::HL, yb, nout, lane, xlo, xhi, ylo, yhi);
    else roll_item<N, 2, 1, 2, true, false, TR>(job, taps, mine, in, outs, sx - 4 * R::HL, yb, nout, lane, xlo, xhi, ylo, yhi);
}

// launch_roll_kernel's tile geometry (TR > 0), as launch_roll_h16_kernel has it: TR rows per band whatever the batch, whole frames per launch, the XCD
// chunk of whole frames with at least 128 bands of every strip.  The caller has checked what launch_roll_kernel checks before it takes tiles (frame_plan_h16).
template <int N, int TR, bool OUT_F32>
static int launch_roll_i16_kernel(const Job2DI16 &job, const RollTaps<N, 2, 1> &taps, unsigned images, hipStream_t st)
{
    typedef Roll<N> R;
    const unsigned strips = (unsigned)((job.cols + R::SW - 1) / R::SW);
    constexpr unsigned WPB = (unsigned)roll_wpb(N, TR);
    const size_t lds = sizeof(float) * WPB * 2 * 2 * R::BUFW;
    const unsigned bands = (unsigned)((job.rows + TR - 1) / TR);
    const unsigned long long per_image = (unsigned long long)strips * bands;
    const unsigned long long max_items = ((1ull << 32) - 4096) / 64;           // a launch indexes < 2^32 threads: split over images
    unsigned long long img_step = max_items / per_image;
    if (img_step == 0) { sg_set_error("2-D frame too large for one launch (%llu items)", per_image); return -1; }
    if (img_step > images) img_step = images;
    constexpr size_t out_elem = OUT_F32 ? 4 : 2;
    for (unsigned long long i0 = 0; i0 < images; i0 += img_step) {
        const unsigned long long ni = images - i0 < img_step ? images - i0 : img_step;
        const unsigned long long total = ni * per_image;
        unsigned grid = (unsigned)((total + WPB - 1) / WPB);
        grid = (grid + 7u) & ~7u;
        Job2DI16 part = job;
        part.in = job.in + (long long)i0 * job.in_pitch;
        part.out = static_cast<unsigned char *>(job.out) + (size_t)i0 * (size_t)job.out_pitch * out_elem;
        int aligned_launch = 7;
        const int chunk_bands = (int)(bands * ((128u + bands - 1u) / bands));
        const unsigned long long chunk_items = (unsigned long long)chunk_bands * strips;
        if (chunk_items % WPB == 0 && chunk_items / WPB < (1u << 22) && chunk_items / WPB * 8u <= grid) aligned_launch |= (int)((unsigned)(chunk_items / WPB) << 8);
        hipLaunchKernelGGL((sg2d_rolling_i16_kernel<N, TR, OUT_F32>), dim3(grid), dim3(64 * WPB), lds, st, part, taps, strips, bands, (unsigned)total, aligned_launch);
    }
    return 0;
}

template <int N>
static int dispatch_roll_i16(int n, const Job2DI16 &job, const float *factors, float scale, unsigned images, hipStream_t st)
{
    if (n == N) {
        constexpr int TR = roll_tile_rows(N, 2, 1, true);
        if constexpr (TR > 0) {
            RollTaps<N, 2, 1> box;
            memset(&box, 0, sizeof(box));
            if (!fill_box_taps<N>(box, factors, scale) || !roll_tiles_on()) return 1;
            return job.out_f32 ? launch_roll_i16_kernel<N, TR, true>(job, box, images, st) : launch_roll_i16_kernel<N, TR, false>(job, box, images, st);
        } else return 1;
    }
    if constexpr (N < SEP_ROLL_MAX_N) return dispatch_roll_i16<N + 1>(n, job, factors, scale, images, st);
    else return 1;
}

// see sg_2d_i16.hpp
int SEP_ROLL_FN(int n, int terms, const Job2DI16 &job, const float *factors, float scale, unsigned images, hipStream_t st)
{
    if (n < SEP_ROLL_MIN_N || n > SEP_ROLL_MAX_N || terms != 2) return 1;
    return dispatch_roll_i16<SEP_ROLL_MIN_N>(n, job, factors, scale, images, st);
}
