// sg_2d_roll_st16_tile.inc -- one tile of the additive form on 16-bit rows, once: the fp32 tile's prologue (LDS carve-up, XCD block order, item ->
// strip, band, image), the family's pointers, and roll_item in the strip's MODE.  A FRAGMENT, as sg_stream_dma_body.inc is: the statements of a kernel,
// included as the whole body of sg2d_rolling_h16_kernel and of sg2d_rolling_i16_kernel (sg_2d_roll_st16.inc).  Not a function template: as a
// __device__ __forceinline__ function over the family the kernels came out with other registers (job and taps by reference) or, the int16 ones, with the
// operands of the stores' row-offset multiply commuted (by value); included, every kernel compiles the tokens it always did
// (profiles/2d_st16_isa_diff.txt).  The including scope provides
//   constexpr int N, TR, NT; constexpr bool BOX (the additive form: NT = 2, BOX = true; the general form on int16 rows: NT = 1 or 2, BOX = false);
//   the family F (sg_2d_st16.hpp) and TOUT, what roll_item stores through (h16: bytes; i16: short or float);
//   job (Job2DSt16<F>), taps, strips, bands, total_items, aligned: the kernel's arguments.
    typedef Roll<N> R;
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int lane = threadIdx.x & 63;
    const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    float *mine = lds + wv * (2 * NT * R::BUFW);             // two LDS rows per term, private to this wave

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
    const typename F::Elem *in = job.in + (long long)img * job.in_pitch;
    TOUT *outs[1];
    outs[0] = F::template image_out<TOUT>(job, img);
    const int sx = (int)strip * R::SW;
    // interior strips: all 256 input columns inside the frame, all SW output columns stored.  The host sends only frames whose every strip can run on
    // vector loads (frame_plan_h16), so the edge strips take the remapped quads: MODE 2 (padded modes) or 3 (VALID: partial quads).
    if (sx - 4 * R::HL >= 0 && sx - 4 * R::HL + 256 <= job.cols && sx >= xlo && sx + R::SW <= xhi)
        roll_item<N, NT, 1, 1, BOX, false, TR>(job, taps, mine, in, outs, sx - 4 * R::HL, yb, nout, lane, xlo, xhi, ylo, yhi);
    else if (valid) roll_item<N, NT, 1, 3, BOX, false, TR>(job, taps, mine, in, outs, sx - 4 * R::HL, yb, nout, lane, xlo, xhi, ylo, yhi);
    else roll_item<N, NT, 1, 2, BOX, false, TR>(job, taps, mine, in, outs, sx - 4 * R::HL, yb, nout, lane, xlo, xhi, ylo, yhi);
