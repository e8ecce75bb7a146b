// sg_2d_hf_body.inc -- one item of the horizontal-first kernel, once: the LDS row, the XCD block order, item -> strip, band, image, the frame's pointers and
// hf_item in the strip's MODE.  A FRAGMENT, as sg_2d_roll_st16_tile.inc is: the statements of a kernel, included as the whole body of sg2d_rolling_hf_kernel
// (fp32 rows) and of sg2d_rolling_hf_i16_kernel (int16 rows in, int16 or fp32 rows out) in sg_2d_hf.hip; included, the fp32 kernels compile the tokens
// they always did.  The including scope provides
//   constexpr int N, NT; constexpr bool ACC; the rows' types TIN and TOUT;
//   job (Job2D or Job2DI16), taps, strips, bands, band_rows, total_items, aligned: the kernel's arguments.
    typedef Hf<N> R;
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int lane = threadIdx.x & 63;
    const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    float *mine = lds + wv * R::BUFW;
    // blocks that share an XCD (blockIdx % 8, observed placement; speed only) take neighbouring items
    const unsigned nblk = gridDim.x;
    const unsigned blk = (blockIdx.x & 7u) * (nblk >> 3) + (blockIdx.x >> 3);
    const unsigned item = blk * R::WPB + (unsigned)wv;
    if (item >= total_items) return;
    const bool valid = job.boundary == SAVGOL2D_BOUNDARY_VALID;
    const int xlo = valid ? job.nx : 0, xhi = valid ? job.cols - job.nx : job.cols;
    const int ylo = valid ? job.ny : 0, yhi = valid ? job.rows - job.ny : job.rows;
    const unsigned strip = item % strips, ib = item / strips;
    const unsigned band = ib % bands, img = ib / bands;
    const int yb = (int)band * band_rows;
    const int nout = job.rows - yb < band_rows ? job.rows - yb : band_rows;
    const TIN *in = job.in + (long long)img * job.in_pitch;
    TOUT *out = static_cast<TOUT *>(job.out) + (long long)img * job.out_pitch;
    const int sx = (int)strip * R::SW;
    if (aligned == 3 && sx - 4 * R::HL >= 0 && sx - 4 * R::HL + 256 <= job.cols && sx >= xlo && sx + R::SW <= xhi)
        hf_item<N, 1, ACC, NT>(job, taps, mine, in, out, sx - 4 * R::HL, yb, nout, lane, xlo, xhi, ylo, yhi);
    else
        hf_item<N, 0, ACC, NT>(job, taps, mine, in, out, sx - 4 * R::HL, yb, nout, lane, xlo, xhi, ylo, yhi);
