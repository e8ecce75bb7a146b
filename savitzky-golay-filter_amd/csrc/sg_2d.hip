// sg_2d.hip -- 2-D path: the drop-in entry points of savgol2d.h and savgol2d_apply_batch_f32.
//
// Reference arithmetic (src/savgol2d.c): out[oy,ox] = scale * sum_{wy} sum_{wx} W[wy][wx] * in[fix(oy+wy-ny)][fix(ox+wx-nx)]
// with a single fp32 accumulator walked row-major over W, separate multiply and add
// (savgol2d_apply_valid :374-393, savgol2d_apply :417-453), `fix` = clamp (CONSTANT) or half-sample
// mirror then clamp (REFLECT) (:428-445); VALID writes only the interior of a same-size frame (:410-414).
//
// Method 1 = the dense window in the SAME summation order and rounding as the reference -> bit-identical outputs:
// sg_2d_dense.hip (packed math, input-row stationary; square and, since round 6, rectangular windows -- the one-pixel-per-lane
// kernel that used to serve those is gone; sg2d_direct2_kernel below keeps its tile form for the rectangular Laplacian).
// Kernels 2 and 3 (method 2 / auto): W is exactly low rank, W(x,y) = sum_t G_t(y) Q_t(x) with r <= 4 terms, so the
// frame is filtered as r column passes and r row passes: 2 r (2n+1) FMAs per pixel instead of (2n+1)^2, back in
// HBM-bound territory; fp32 rounding only (1e-7 level) against the reference.  enqueue_frame picks the kernel for one output
// frame: sg_2d_hf.hip (x-dominant derivative frames, horizontal pass first), sg_2d_roll.hip (rolling column windows in
// registers) or sg_2d_sep.hip (the tile kernel: square windows, any half window).
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <vector>

#include "sg_2d.hpp"
#include "sg_2d_grad16_host.hpp"
#include "sg_2d_st16.hpp"
#include "sg_runtime.hpp"

namespace sg {

constexpr int T2_W = 64, T2_H = 16;                 // outputs per block: 64 wide, 16 tall (4 per thread)
constexpr int SEP_FACTOR_FLOATS = SEP_MAX_TERMS * 2 * (2 * SAVGOL2D_MAX_HALF_WINDOW + 2);   // one frame's factors at the widest half window

// Two dense windows over one read of the tile, each summed in the reference's order and scaled, then added: the reference's Laplacian
// (savgol2d_laplacian, src/savgol2d.c:560-618: output = xx frame, temp = yy frame, output += temp) bit for bit, with no temporary frame
// and no add pass.  Rectangular windows (the square ones have the fast kernels).  LDS: W1, W2 (each padded to a multiple of 4), the tile.
__global__ __launch_bounds__(256) void sg2d_direct2_kernel(const Job2D job, const float *__restrict__ W1, const float *__restrict__ W2, float scale2)
{
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int nx = job.nx, ny = job.ny, ww = 2 * nx + 1, wh = 2 * ny + 1;
    const int wpad = (ww * wh + 3) & ~3;
    float *wl1 = lds, *wl2 = lds + wpad;
    float *tile = lds + 2 * wpad;
    const int tw = T2_W + 2 * nx, th = T2_H + 2 * ny;
    const int tid = threadIdx.x;
    const int bx = blockIdx.x % job.tiles_x, by = blockIdx.x / job.tiles_x;
    const long long img = blockIdx.y;
    const float *in = job.in + img * job.in_pitch;
    float *out = job.out + img * job.out_pitch;
    const int x0 = bx * T2_W, y0 = by * T2_H;
    for (int i = tid; i < ww * wh; i += 256) { wl1[i] = W1[i]; wl2[i] = W2[i]; }
    for (int i = tid; i < tw * th; i += 256) {
        const int r = i / tw, c = i - r * tw;
        const int iy = fix_index(y0 + r - ny, job.rows, job.boundary);
        const int ix = fix_index(x0 + c - nx, job.cols, job.boundary);
        tile[i] = in[(long long)iy * job.in_stride + ix];
    }
    __syncthreads();
    const int lx = tid & 63, ly = tid >> 6;
    float a1[4] = {0.0f, 0.0f, 0.0f, 0.0f}, a2[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    for (int wy = 0; wy < wh; ++wy) {
        const float *t0 = tile + (ly + wy) * tw + lx;
        for (int wx = 0; wx < ww; ++wx) {
            const float w1 = wl1[wy * ww + wx], w2 = wl2[wy * ww + wx];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const float v = t0[(4 * k) * tw + wx];
                a1[k] = __fadd_rn(a1[k], __fmul_rn(w1, v));
                a2[k] = __fadd_rn(a2[k], __fmul_rn(w2, v));
            }
        }
    }
    const int ox = x0 + lx;
    const bool valid = job.boundary == SAVGOL2D_BOUNDARY_VALID;
    const int xlo = valid ? nx : 0, xhi = valid ? job.cols - nx : job.cols;
    const int ylo = valid ? ny : 0, yhi = valid ? job.rows - ny : job.rows;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int oy = y0 + ly + 4 * k;
        if (ox >= xlo && ox < xhi && oy >= ylo && oy < yhi)
            out[(long long)oy * job.out_stride + ox] = __fadd_rn(__fmul_rn(a1[k], job.scale), __fmul_rn(a2[k], scale2));
    }
}

// out += other over a rows x cols region (savgol2d_laplacian, reference :609-613)
__global__ __launch_bounds__(256) void sg2d_add_kernel(float *__restrict__ out, const float *__restrict__ other, int rows,
                                                       int cols, int stride)
{
    const int x = blockIdx.x * 256 + threadIdx.x, y = blockIdx.y;
    if (x < cols && y < rows) out[(long long)y * stride + x] = __fadd_rn(out[(long long)y * stride + x], other[(long long)y * stride + x]);
}

// separable factors per config, computed once (host least-squares solve + orthogonalisation)
static int sep_factors_cached(const Savgol2DConfig *cfg, float *factors)
{
    struct Entry { Savgol2DConfig cfg; int terms; float f[SEP_FACTOR_FLOATS]; };
    static std::mutex mu;
    static Entry cache[32];
    static int used = 0, next = 0;
    std::lock_guard<std::mutex> lock(mu);
    for (int i = 0; i < used; ++i)
        if (memcmp(&cache[i].cfg, cfg, sizeof(*cfg)) == 0) { memcpy(factors, cache[i].f, sizeof(cache[i].f)); return cache[i].terms; }
    Entry &e = cache[next];
    next = (next + 1) % 32;
    if (used < 32) ++used;
    memset(&e, 0, sizeof(e));
    memcpy(&e.cfg, cfg, sizeof(*cfg));
    e.terms = sg2d_separable_factors(cfg, e.f, SEP_MAX_TERMS);
    memcpy(factors, e.f, sizeof(e.f));
    return e.terms;
}

// The derivative entry points take a configuration, not a filter object: without these two caches every call repeated the host
// least-squares solve (75 us at n = 7, 0.4-2.7 ms at n = 16 per gradient / Hessian call: tools/time_2d_host_overhead.py).
// (a) the summed Laplacian kernel's factors per (n, order, deltas); (b) dense weight tables of rectangular windows per full config.
struct SummedKey { int n, order; float dx, dy; };
static int summed_factors_cached(const SummedKey &key, const double *Wsum, float *factors)
{
    struct Entry { SummedKey key; int terms; float f[SEP_FACTOR_FLOATS]; };
    static std::mutex mu;
    static Entry cache[16];
    static int used = 0, next = 0;
    std::lock_guard<std::mutex> lock(mu);
    for (int i = 0; i < used; ++i)
        if (memcmp(&cache[i].key, &key, sizeof(key)) == 0) {
            if (factors) memcpy(factors, cache[i].f, sizeof(cache[i].f));
            return cache[i].terms;
        }
    if (!Wsum) return -1;                                    // lookup only
    Entry &e = cache[next];
    next = (next + 1) % 16;
    if (used < 16) ++used;
    memset(&e, 0, sizeof(e));
    e.key = key;
    e.terms = sg2d_factors_from_kernel(Wsum, key.n, key.order, e.f, SEP_MAX_TERMS);
    memcpy(factors, e.f, sizeof(e.f));
    return e.terms;
}

// a filter object per distinct rectangular configuration, kept for the life of the process (a few KB each, at most 64)
static const Savgol2DFilter *rect_filter_cached(const Savgol2DConfig *cfg, bool *owned)
{
    static std::mutex mu;
    static std::vector<Savgol2DFilter *> cache;
    std::lock_guard<std::mutex> lock(mu);
    for (const Savgol2DFilter *f : cache)
        if (memcmp(&f->config, cfg, sizeof(*cfg)) == 0) { *owned = false; return f; }
    Savgol2DFilter *f = savgol2d_create(cfg);
    if (!f) return nullptr;
    if (cache.size() < 64) { cache.push_back(f); *owned = false; }
    else *owned = true;                                      // cache full: the caller destroys it
    return f;
}

// rect_filter_cached's answer for the length of one call: a filter the full cache did not keep is destroyed with the holder
struct CachedFilter {
    bool owned = false;
    const Savgol2DFilter *f = nullptr;
    const Savgol2DFilter *get(const Savgol2DConfig *cfg) { if (!f) f = rect_filter_cached(cfg, &owned); return f; }
    CachedFilter() = default;
    CachedFilter(const CachedFilter &) = delete;
    CachedFilter &operator=(const CachedFilter &) = delete;
    ~CachedFilter() { if (owned) savgol2d_destroy(const_cast<Savgol2DFilter *>(f)); }
};

// Do two fp32 frame batches share a byte?  The exact test for strided layouts lives in sg_2d_h16_host.hpp (plain C++, so that a host program can hold it
// to its cases), generalised over the element sizes for the call on 16-bit storage; two fp32 stacks get the answers they always got.
static bool frames_overlap(const float *a, long long a_pitch, int a_stride, const float *b, long long b_pitch, int b_stride, int rows, int cols, size_t images)
{
    return frames_overlap(reinterpret_cast<uintptr_t>(a), sizeof(float), a_pitch, a_stride, reinterpret_cast<uintptr_t>(b), sizeof(float), b_pitch, b_stride, rows, cols, images);
}

// the geometry every 2-D device entry point refuses, with its texts
static bool geometry_ok(const char *who, int nx, int ny, int rows, int cols, int in_stride, int out_stride, int boundary)
{
    if (rows <= 0 || cols <= 0 || in_stride < cols || out_stride < cols) { sg_set_error("%s: bad image geometry", who); return false; }
    if (boundary == SAVGOL2D_BOUNDARY_VALID && (rows - 2 * ny <= 0 || cols - 2 * nx <= 0)) {
        sg_set_error("%s: image smaller than the window", who);
        return false;
    }
    return true;
}

// What every 2-D device entry point checks once its kernel is known to be valid, and the Job2D it starts from: job.in = d_in, the
// caller sets out, scale and the tile counts.  0 = go on, 1 = nothing to do (no images), -1 = error.
static int make_job(const char *who, int nx, int ny, const float *d_in, float *const *outs, int nout, int rows, int cols, int in_stride,
                    long long in_pitch, int out_stride, long long out_pitch, size_t images, int boundary, Job2D &job)
{
    bool null = !d_in;
    for (int i = 0; i < nout; ++i) null = null || !outs[i];
    if (null) { sg_set_error("%s: NULL pointer", who); return -1; }
    if (!geometry_ok(who, nx, ny, rows, cols, in_stride, out_stride, boundary)) return -1;
    if (images == 0) return 1;
    // No 2-D kernel may run in place: every output reads its neighbours' inputs, tiles of one frame run in any order, and the
    // two-pass form of wide windows re-reads the input after the output has been written.  The reference's loop is no different
    // (src/savgol2d.c:374-393 reads input rows it has long overwritten).  Refuse instead of returning garbage.
    for (int i = 0; i < nout; ++i)
        if (frames_overlap(d_in, in_pitch, in_stride, outs[i], out_pitch, out_stride, rows, cols, images)) {
            sg_set_error("%s: input and output frames overlap (2-D filtering cannot run in place)", who);
            return -1;
        }
    memset(&job, 0, sizeof(job));
    job.in = d_in;
    job.rows = rows; job.cols = cols; job.in_stride = in_stride; job.out_stride = out_stride;
    job.in_pitch = in_pitch; job.out_pitch = out_pitch;
    job.nx = nx; job.ny = ny;
    job.boundary = (boundary == SAVGOL2D_BOUNDARY_VALID || boundary == SAVGOL2D_BOUNDARY_REFLECT) ? boundary : SAVGOL2D_BOUNDARY_CONSTANT;
    return 0;
}

// What each term's x factor must SUM to (sg_2d_hf.hip, convert()): the horizontal-first kernel applies its taps to centred samples, s_k - c, and adds
// c * sigma_t back -- with sigma_t taken from the REFERENCE's dense fp32 table instead of the rounded factor taps: least squares over the window rows y of
//      scale * sum_x W[y][x]  ~=  sum_t sigma_t G_t(y)          (G_t = the fp32 column factors as the kernel mirrors them)
// so that a constant (or slowly varying) part of the input comes out as the reference's own table maps it.  A failed solve gives zeros (the centred pass alone).
// columns = true: the transposed roles (the tile kernel on y-dominant kernels, whose FIRST pass runs down the columns): what each term's y factor must sum
// to, fitted to the table's column sums in the basis of the x factors.
// tile = true: the tile kernel (sg_2d_sep.hip) -- taps as stored, not mirrored, and the scale left to its store.  false = no fit (sigma zeroed).
static bool hf_term_sums(int n, int terms, const float *factors, const Savgol2DFilter *dense, float *sigma, bool columns = false, bool tile = false)
{
    const int ws = 2 * n + 1, nx = dense->config.half_window_x, ny = dense->config.half_window_y, ww = 2 * nx + 1;
    double rs[2 * SAVGOL2D_MAX_HALF_WINDOW + 1] = {0.0}, G[SEP_MAX_TERMS][2 * SAVGOL2D_MAX_HALF_WINDOW + 1];
    for (int t = 0; t < terms; ++t) sigma[t] = 0.0f;
    if (terms < 1 || terms > SEP_MAX_TERMS || ny > n || nx > n) return false;
    const double sc = tile ? 1.0 : (double)dense->scale;
    if (!columns) {
        for (int y = 0; y <= 2 * ny; ++y) {
            double acc = 0.0;
            for (int x = 0; x < ww; ++x) acc += (double)dense->weights[y * ww + x];
            rs[(n - ny) + y] = acc * sc;
        }
    } else {
        for (int x = 0; x < ww; ++x) {
            double acc = 0.0;
            for (int y = 0; y <= 2 * ny; ++y) acc += (double)dense->weights[y * ww + x];
            rs[(n - nx) + x] = acc * sc;
        }
    }
    for (int t = 0; t < terms; ++t) {
        const float *g = factors + (size_t)t * 2 * (ws + 1) + (columns ? 0 : (ws + 1));          // the basis: G_t (rows) or Q_t (columns)
        float sy = 1.0f;
        if (tile) { for (int y = 0; y < ws; ++y) G[t][y] = (double)g[y]; continue; }
        if (!vector_parity(g, n, &sy)) return false;
        for (int y = 0; y < ws; ++y) G[t][y] = y <= n ? (double)((y == n && sy < 0.0f) ? 0.0f : g[y]) : (double)sy * (double)g[2 * n - y];
    }
    double A[SEP_MAX_TERMS][SEP_MAX_TERMS + 1];
    for (int t = 0; t < terms; ++t) {
        for (int u = 0; u < terms; ++u) { double d = 0.0; for (int y = 0; y < ws; ++y) d += G[t][y] * G[u][y]; A[t][u] = d; }
        double d = 0.0;
        for (int y = 0; y < ws; ++y) d += G[t][y] * rs[y];
        A[t][terms] = d;
    }
    for (int c = 0; c < terms; ++c) {                                  // Gaussian elimination with partial pivoting (<= 4 x 4)
        int piv = c;
        for (int r = c + 1; r < terms; ++r) if (std::fabs(A[r][c]) > std::fabs(A[piv][c])) piv = r;
        if (std::fabs(A[piv][c]) < 1e-300) return false;
        if (piv != c) for (int j = 0; j <= terms; ++j) { const double tmp = A[c][j]; A[c][j] = A[piv][j]; A[piv][j] = tmp; }
        for (int r = c + 1; r < terms; ++r) { const double fct = A[r][c] / A[c][c]; for (int j = c; j <= terms; ++j) A[r][j] -= fct * A[c][j]; }
    }
    double sol[SEP_MAX_TERMS];
    for (int i = terms - 1; i >= 0; --i) {
        double v = A[i][terms];
        for (int j = i + 1; j < terms; ++j) v -= A[i][j] * sol[j];
        sol[i] = v / A[i][i];
    }
    for (int t = 0; t < terms; ++t) sigma[t] = (float)sol[t];
    return true;
}

// One output frame of a separable kernel: `terms` terms laid out for the half window it is filtered with (a rectangular window's
// factors zero-padded to its larger half window), output = scale * their sum.
struct SepFrame {
    const float *factors;
    int terms;
    float scale;
    Savgol2DConfig cfg;                 // deriv_x / deriv_y set the pass order ((0, 0): the summed Laplacian); the dense table's configuration
    const Savgol2DFilter *dense;        // that table if the caller holds it, else NULL: looked up when a pass needs it
    float *out;
};

// Kernels whose x factor cancels harder than their y factor (sg2d_x_dominant: d/dx, d^2/dx^2, ...) run the HORIZONTAL pass first
// (sg_2d_hf.hip): one launch per term, the later ones accumulating (the first two share one where the kernel has that form); the term
// sums are fitted to `dense`, the frame's table (hf_term_sums).  0 = launched, 1 = not covered (no definite parity: nothing has been
// launched), -1 = error.
static int roll_passes_hf(int n, const Job2D &job, const SepFrame &fr, const Savgol2DFilter *dense, unsigned images, int cu_count, hipStream_t st)
{
    const size_t tstride = (size_t)2 * (2 * n + 2);
    for (int t = 0; t < fr.terms; ++t) {
        float s;
        if (!vector_parity(fr.factors + t * tstride, n, &s) || !vector_parity(fr.factors + t * tstride + (2 * n + 2), n, &s)) return 1;
    }
    float sigma[SEP_MAX_TERMS] = {0.0f, 0.0f, 0.0f, 0.0f};
    hf_term_sums(n, fr.terms, fr.factors, dense, sigma);
    Job2D j = job;
    int t = 0;
    if (fr.terms >= 2) {                                     // two terms from one trip of every row through LDS
        const int rc = sg2d_launch_rolling_hf(n, j, fr.factors, fr.scale, sigma[0], fr.factors + tstride, sigma[1], images, cu_count, st);
        if (rc < 0) return rc;
        if (rc == 0) { t = 2; j.accumulate = 1; }
    }
    for (; t < fr.terms; ++t) {
        const int rc = sg2d_launch_rolling_hf(n, j, fr.factors + t * tstride, fr.scale, sigma[t], nullptr, 0.0f, images, cu_count, st);
        if (rc != 0) return t == 0 ? rc : -1;
        j.accumulate = 1;
    }
    return 0;
}

// The rolling kernel on one frame, in one launch where its taps fit the scalar registers (4 terms up to n = 8, 3 up to n = 12, 2
// beyond), else in TWO: the first half of the terms, then the rest with job.accumulate (out += ...).  The second pass re-reads the
// input and read-modify-writes the output -- 20 B per pixel instead of 8 -- which these arithmetic-bound shapes can afford: order 6
// at n = 9 / 12 / 16: 1.83 / 2.25 / 3.15 ms per 16 frames on the tile kernel, two rolling passes 1.5-2 x faster (profiles/
// r03_sweep_2d_orders.txt).  0 = launched, 1 = not covered, -1 = error.
static int roll_passes(int n, const Job2D &job, const SepFrame &fr, unsigned images, int cu_count, hipStream_t st)
{
    int rc = sg2d_launch_rolling(n, fr.terms, job, fr.factors, fr.scale, images, cu_count, st);
    if (rc != 1 || n < 9 || fr.terms < 3 || fr.terms > 4) return rc;      // split only what is "not covered" (1), never an error (-1)
    // 2 + 2 (or 2 + 1) rather than 3 + 1 where three terms fit: the accumulating pass moves 12 B per pixel and takes ~0.9 ms per 16
    // frames at n = 9 whether it carries one term or two, so it may as well carry two (3 + 1: 1.05 + 0.89 ms, 2 + 2: 0.75 + 0.93)
    const int first = 2;
    Job2D rest = job;
    rest.accumulate = 1;
    // try the second pass's instantiation first?  Both exist for every n >= 9 (NT <= 2), so the first failing means neither ran.
    rc = sg2d_launch_rolling(n, first, job, fr.factors, fr.scale, images, cu_count, st);
    if (rc != 0) return rc;
    return sg2d_launch_rolling(n, fr.terms - first, rest, fr.factors + (size_t)first * 2 * (2 * n + 2), fr.scale, images, cu_count, st);
}

// One output frame through the first kernel in this order that takes it: horizontal pass first (x-dominant frames), the rolling
// kernel (in two passes where its terms do not fit one), the tile kernel (square windows, every half window).  Method 3 on a square
// window goes straight to the tile kernel, whose first pass runs down the columns for y-dominant frames and on centred samples for x-
// and y-dominant ones.  job: all but the output; n: the half window the factors are laid out for.  0 = launched, 1 = not covered
// (nothing launched: a rectangular window beyond the rolling kernel's ranks), -1 = error.
static int enqueue_frame(const char *who, DeviceCtx *ctx, const Job2D &job, int n, bool square, int method, const SepFrame &fr,
                         size_t images, hipStream_t st)
{
    const bool xdom = sg2d_x_dominant(fr.cfg.deriv_x, fr.cfg.deriv_y), ydom = sg2d_y_dominant(fr.cfg.deriv_x, fr.cfg.deriv_y);
    CachedFilter held;
    const Savgol2DFilter *dense = fr.dense;
    auto have_dense = [&] {                                  // on first use: most frames of a derivative call never need the table
        if (!dense) dense = held.get(&fr.cfg);
        if (!dense) sg_set_error("%s: weight computation failed", who);
        return dense != nullptr;
    };
    const float *d_f = nullptr;
    // chunks of images so that a launch indexes < 2^31 tiles
    const size_t max_img = ((size_t)1 << 30) / ((size_t)((job.cols + 63) / 64) * (size_t)(job.rows + 1)) + 1;
    for (size_t i0 = 0; i0 < images; i0 += max_img) {
        const unsigned ni = (unsigned)(images - i0 < max_img ? images - i0 : max_img);
        Job2D j = job;
        j.in = job.in + (long long)i0 * job.in_pitch;
        j.out = fr.out + (long long)i0 * job.out_pitch;
        int rc = 1;
        if (method != 3 || !square) {
            if (xdom) rc = have_dense() ? roll_passes_hf(n, j, fr, dense, ni, ctx->cu_count, st) : -1;
            if (rc == 1) rc = roll_passes(n, j, fr, ni, ctx->cu_count, st);
        }
        if (rc == 1 && square) {
            if (!d_f) d_f = ctx_table(ctx, fr.factors, sizeof(float) * (size_t)fr.terms * 2 * (2 * n + 2), 0x5e000000u + (unsigned)n);
            if (!d_f) return -1;
            SepPlan plan;
            memset(&plan, 0, sizeof(plan));
            plan.outputs = 1; plan.terms[0] = fr.terms; plan.scale[0] = fr.scale; plan.out[0] = j.out;
            plan.transposed = ydom ? 1 : 0;
            if (xdom || ydom) {
                if (!have_dense()) return -1;
                plan.centre = hf_term_sums(n, fr.terms, fr.factors, dense, plan.first_sum, ydom, true) ? 1 : 0;
            }
            if (sg2d_launch_separable(n, j, plan, d_f, ni, ctx->cu_count, st) != 0) { sg_set_error("%s: no separable kernel for n=%d", who, n); return -1; }
            rc = 0;
        }
        if (rc != 0) return rc;
    }
    return 0;
}

static bool filter_ok(const char *who, const Savgol2DFilter *f)
{
    const int nx = f->config.half_window_x, ny = f->config.half_window_y;
    if (nx < 1 || nx > SAVGOL2D_MAX_HALF_WINDOW || ny < 1 || ny > SAVGOL2D_MAX_HALF_WINDOW || !f->weights ||
        f->window_width != 2 * nx + 1 || f->window_height != 2 * ny + 1) {
        sg_set_error("%s: filter struct is not a valid Savgol2DFilter", who);
        return false;
    }
    return true;
}

static int enqueue_2d(const char *who, const Savgol2DFilter *f, const float *d_in, int rows, int cols, int in_stride,
                      long long in_pitch, float *d_out, int out_stride, long long out_pitch, size_t images, int boundary,
                      int method, hipStream_t st)
{
    if (!f) { sg_set_error("%s: NULL pointer", who); return -1; }
    if (!filter_ok(who, f)) return -1;
    const int nx = f->config.half_window_x, ny = f->config.half_window_y;
    Job2D job;
    int rc = make_job(who, nx, ny, d_in, &d_out, 1, rows, cols, in_stride, in_pitch, out_stride, out_pitch, images, boundary, job);
    if (rc != 0) return rc > 0 ? 0 : -1;
    DeviceCtx *ctx = ctx_get();
    if (!ctx) return -1;
    job.scale = f->scale;
    // method: 1 = dense window (bit-identical to the reference), 2 = separable passes (3 = its tile kernel only), 0 = separable when available
    if (method != 1) {
        float factors[SEP_FACTOR_FLOATS];
        const int terms = sep_factors_cached(&f->config, factors);
        if (terms > 0) {
            const SepFrame fr = {factors, terms, f->scale, f->config, f, d_out};
            rc = enqueue_frame(who, ctx, job, nx > ny ? nx : ny, nx == ny, method, fr, images, st);
            if (rc == 0) return hip_ok(hipGetLastError(), who) ? 0 : -1;
            if (rc < 0) return -1;
        }
        if (method >= 2) { sg_set_error("%s: no separable kernel for this %dx%d window (rank > %d, or a rectangular window beyond the rolling kernel's ranks)", who, 2 * nx + 1, 2 * ny + 1, SEP_MAX_TERMS); return -1; }
    }
    for (size_t i0 = 0; i0 < images; i0 += 65535) {
        const size_t ni = images - i0 < 65535 ? images - i0 : 65535;
        job.in = d_in + (long long)i0 * in_pitch;
        job.out = d_out + (long long)i0 * out_pitch;
        rc = sg2d_launch_dense_rolling(job, f->weights, ctx, (unsigned)ni, st);
        if (rc != 0) {
            if (rc > 0) sg_set_error("%s: no dense kernel for a %dx%d window", who, 2 * nx + 1, 2 * ny + 1);
            return -1;
        }
    }
    return hip_ok(hipGetLastError(), who) ? 0 : -1;
}

// host frame -> arena -> kernel -> host region [r0,r1) x [c0,c1) of the output frame
static int host_apply(const char *who, const Savgol2DFilter *f, const float *input, int rows, int cols, int in_stride,
                      float *output, int out_stride, int boundary, bool compact_valid)
{
    DeviceCtx *ctx = ctx_get();
    if (!ctx) { fprintf(stderr, "%s: %s\n", who, savgol_hip_last_error()); return -1; }
    std::lock_guard<std::recursive_mutex> lock(ctx->mu);
    const int nx = f->config.half_window_x, ny = f->config.half_window_y;
    const int dstride = (cols + 3) & ~3;
    float *d_in = static_cast<float *>(ctx_arena(ctx, 2 * sizeof(float) * (size_t)rows * dstride));
    if (!d_in) { fprintf(stderr, "%s: %s\n", who, savgol_hip_last_error()); return -1; }
    float *d_out = d_in + (size_t)rows * dstride;
    bool ok = hip_ok(hipMemcpy2D(d_in, sizeof(float) * dstride, input, sizeof(float) * in_stride, sizeof(float) * cols, rows,
                                 hipMemcpyHostToDevice), "H2D copy");
    // host-pointer calls are PCIe bound anyway: use the dense kernel, whose output is bit-identical to the reference's
    ok = ok && enqueue_2d(who, f, d_in, rows, cols, dstride, 0, d_out, dstride, 0, 1, boundary, 1, nullptr) == 0;
    if (ok) {
        const bool valid = boundary == SAVGOL2D_BOUNDARY_VALID;
        const int r0 = valid ? ny : 0, c0 = valid ? nx : 0;
        const int nr = valid ? rows - 2 * ny : rows, nc = valid ? cols - 2 * nx : cols;
        float *dst = compact_valid ? output : output + (size_t)r0 * out_stride + c0;
        ok = hip_ok(hipMemcpy2D(dst, sizeof(float) * out_stride, d_out + (size_t)r0 * dstride + c0, sizeof(float) * dstride,
                                sizeof(float) * nc, nr, hipMemcpyDeviceToHost), "D2H copy");
    }
    if (!ok) { fprintf(stderr, "%s: %s\n", who, savgol_hip_last_error()); return -1; }
    return 0;
}

// ---- what the two 2-D batch calls on 2-byte storage share (savgol2d_apply_batch_h16, savgol2d_apply_batch_i16; the entry points are further down) ----
// The staged route: the twin itself.  Whole frames per piece, widened into aligned fp32 scratch, savgol2d_apply_batch_f32's own path (enqueue_2d)
// scratch to scratch, and the pixels it wrote rounded out.  Pieces of whole frames do not change bits: the additive tile's re-seed phase is the
// tile, the strip walk's the frame row (launch_roll_kernel), and every other 2-D kernel computes its outputs independently.
// (shared with savgol2d_apply_batch_i16: `widen(first frame, scratch, frames)` and `convert(scratch, first output byte, frames, xlo, xhi, ylo, yhi)` are the
//  storage family's two small kernels; the element sizes, and with them the pieces, are the same)
template <class Widen, class Convert>
static int staged16_2d(const char *who, DeviceCtx *ctx, const Savgol2DFilter *f, int rows, int cols, void *d_out, size_t out_elem, long long out_pitch, size_t images,
                       int boundary, int method, hipStream_t st, Widen widen, Convert convert)
{
    const FrameStageH16 g = frame_stage_h16(rows, cols, images);
    const size_t side = (g.frames * g.frame * sizeof(float) + 255) & ~(size_t)255;
    char *scratch = static_cast<char *>(scratch_alloc(ctx, 2 * side, st, who));
    if (!scratch) return -1;
    float *sin = reinterpret_cast<float *>(scratch), *sout = reinterpret_cast<float *>(scratch + side);
    const bool valid = boundary == SAVGOL2D_BOUNDARY_VALID;
    const int nx = f->config.half_window_x, ny = f->config.half_window_y;
    const int xlo = valid ? nx : 0, xhi = valid ? cols - nx : cols, ylo = valid ? ny : 0, yhi = valid ? rows - ny : rows;
    int rc = 0;
    for (size_t i0 = 0; i0 < images && rc == 0; i0 += g.frames) {
        const size_t ni = images - i0 < g.frames ? images - i0 : g.frames;
        widen(i0, sin, ni);
        rc = enqueue_2d(who, f, sin, rows, cols, g.stride, (long long)g.frame, sout, g.stride, (long long)g.frame, ni, boundary, method, st);
        if (rc != 0) break;
        convert(sout, static_cast<char *>(d_out) + i0 * (size_t)out_pitch * out_elem, ni, xlo, xhi, ylo, yhi);
    }
    const bool freed = scratch_free(scratch, st, who);
    if (rc != 0 || !freed) return -1;
    return hip_ok(hipGetLastError(), who) ? 0 : -1;
}

// The two calls on 2-byte storage share one route (apply16_2d, route16_2d below); what they differ in is their host-side description, the 2-D
// counterpart of the 1-D calls' H16Host / I16Host (sg_api_1d.cpp):
//   Family         the device-side policy (sg_2d_st16.hpp): element type, job, tile objects, staged kernels
//   WHO, FORM      the call's name; the storage's name in the method-1 refusal
//   TILES_ENV      the call's own switch
//   types_served   the refusal of a type pair (h16) or an output type (i16) the call does not serve; in_type is ignored where the input has one type
//   fill           how in_type / out_type map onto the job's storage fields
struct H16Host2D {
    typedef H16Family2D Family;
    static constexpr const char *WHO = "savgol2d_apply_batch_h16", *FORM = "16-bit", *TILES_ENV = "SAVGOL_HIP_2D_H16_TILES";
    static const char *type_name(int t) { return t == SAVGOL_HIP_F32 ? "f32" : t == SAVGOL_HIP_F16 ? "f16" : t == SAVGOL_HIP_BF16 ? "bf16" : "unknown"; }
    static bool types_served(int in_type, int out_type)
    {
        if ((in_type != SAVGOL_HIP_F16 && in_type != SAVGOL_HIP_BF16) || (out_type != in_type && out_type != SAVGOL_HIP_F32)) {
            sg_set_error("%s: type pair %s -> %s (%d -> %d) is not served: f16 -> f16, bf16 -> bf16, f16 -> f32, bf16 -> f32 are", WHO, type_name(in_type), type_name(out_type),
                         in_type, out_type);
            return false;
        }
        return true;
    }
    static void fill(Family::Fields &st, int in_type, int out_type)
    {
        st.in_bf = in_type == SAVGOL_HIP_BF16 ? 1 : 0; st.out_bf = out_type == SAVGOL_HIP_BF16 ? 1 : 0; st.out_f32 = out_type == SAVGOL_HIP_F32 ? 1 : 0;
    }
};
struct I16Host2D {
    typedef I16Family2D Family;
    static constexpr const char *WHO = "savgol2d_apply_batch_i16", *FORM = "int16", *TILES_ENV = "SAVGOL_HIP_2D_I16_TILES";
    static bool types_served(int, int out_type)
    {
        if (out_type != SAVGOL_HIP_I16 && out_type != SAVGOL_HIP_F32) {
            sg_set_error("%s: out_type %d is not served: SAVGOL_HIP_I16 (%d) and SAVGOL_HIP_F32 (%d) are", WHO, out_type, SAVGOL_HIP_I16, SAVGOL_HIP_F32);
            return false;
        }
        return true;
    }
    static void fill(Family::Fields &st, int, int out_type) { st.out_f32 = out_type == SAVGOL_HIP_F32 ? 1 : 0; }
};

static bool method_ok_16(const char *who, int method, const char *form)
{
    if (method == 1) { sg_set_error("%s: method 1 (the dense kernel in the reference's summation order) is not served: the reference has no %s form to be identical to", who, form); return false; }
    if (method < 0 || method > 3) { sg_set_error("%s: method %d is not one of 0, 2, 3", who, method); return false; }
    return true;
}
// Everything after a call's method and type checks: the remaining refusals in the header's order, then the route: -1 = refused (text set), 0 = nothing to do
// (no images) or STAGED, 1 = TILES.  Touches no device.  `factors` / `terms`: the filter's separable factors, for the launch that follows.
static int plan16_2d(const char *who, const char *tiles_env, const Savgol2DFilter *filter, const void *d_in, int rows, int cols, int in_stride, long long in_pitch,
                     const void *d_out, int out_type, int out_stride, long long out_pitch, size_t images, int boundary, int method, float *factors, int *terms)
{
    if (!filter || !d_in || !d_out) { sg_set_error("%s: NULL pointer", who); return -1; }
    if (!filter_ok(who, filter)) return -1;
    const int nx = filter->config.half_window_x, ny = filter->config.half_window_y;
    if (!geometry_ok(who, nx, ny, rows, cols, in_stride, out_stride, boundary)) return -1;
    if (images == 0) return 0;
    const int out_elem = out_type == SAVGOL_HIP_F32 ? 4 : 2;
    const uintptr_t in0 = reinterpret_cast<uintptr_t>(d_in), out0 = reinterpret_cast<uintptr_t>(d_out);
    if (frames_overlap(in0, 2, in_pitch, in_stride, out0, (size_t)out_elem, out_pitch, out_stride, rows, cols, images)) {
        sg_set_error("%s: input and output frames overlap (2-D filtering cannot run in place; compared byte-wise)", who);
        return -1;
    }
    // the route (sg_2d_h16_host.hpp).  The call's switch (SAVGOL_HIP_2D_H16_TILES / SAVGOL_HIP_2D_I16_TILES) is read at every call, not once: tools/time_2d_h16.py times both routes interleaved in
    // one process (single-threaded; the header says so).  SAVGOL_HIP_ROLL_TILE is read once, where the fp32 launcher reads it (roll_tiles_on, inside
    // the predicate); the rule names it as a condition of its own, so the shape carries it too.
    const char *const tiles_text = getenv(tiles_env);
    static const bool roll_tile_env = [] { const char *e = getenv("SAVGOL_HIP_ROLL_TILE"); return !e || atoi(e) != 0; }();
    *terms = sep_factors_cached(&filter->config, factors);
    FrameShapeH16 shape;
    shape.rows = rows; shape.cols = cols;
    shape.in_stride = in_stride; shape.in_pitch = in_pitch; shape.out_stride = out_stride; shape.out_pitch = out_pitch;
    shape.in_base = in0; shape.out_base = out0; shape.out_elem = out_elem;
    shape.method = method;
    shape.x_dominant = sg2d_x_dominant(filter->config.deriv_x, filter->config.deriv_y);
    shape.additive_tile = *terms > 0 && roll16_fp32_takes_tiles(nx > ny ? nx : ny, *terms, factors, filter->scale);
    shape.roll_tile_switch = roll_tile_env;
    shape.tiles_switch = !tiles_text || atoi(tiles_text) != 0;
    return frame_plan_h16(shape) == FRAME_H16_TILES ? 1 : 0;
}

// A call's refusals in the header's order (method, type pair, then plan16_2d's), then its route.  Serves the _route exports as it stands.
template <class H>
static int route16_2d(const Savgol2DFilter *filter, const void *d_in, int in_type, int rows, int cols, int in_stride, long long in_pitch, const void *d_out, int out_type,
                      int out_stride, long long out_pitch, size_t images, int boundary, int method, float *factors, int *terms)
{
    if (!method_ok_16(H::WHO, method, H::FORM) || !H::types_served(in_type, out_type)) return -1;
    return plan16_2d(H::WHO, H::TILES_ENV, filter, d_in, rows, cols, in_stride, in_pitch, d_out, out_type, out_stride, out_pitch, images, boundary, method, factors, terms);
}

// The call: fp16 / bf16 or int16 frames in, the same type or fp32 out, the fp32 call's arithmetic in between (contract: savgol_hip.h).
template <class H>
static int apply16_2d(const Savgol2DFilter *filter, const void *d_in, int in_type, int rows, int cols, int in_stride, long long in_pitch, void *d_out, int out_type,
                      int out_stride, long long out_pitch, size_t images, int boundary, int method, hipStream_t st)
{
    typedef typename H::Family F;
    const char *who = H::WHO;
    float factors[SEP_FACTOR_FLOATS];
    int terms = 0;
    // the refusals, in the order the header gives, and the route: decided before anything touches the device
    const int route = route16_2d<H>(filter, d_in, in_type, rows, cols, in_stride, in_pitch, d_out, out_type, out_stride, out_pitch, images, boundary, method, factors, &terms);
    if (route < 0) return -1;
    if (images == 0) return 0;
    DeviceCtx *ctx = ctx_get();                               // both routes: the context binds the thread to the library's device, as in the fp32 call
    if (!ctx) return -1;
    const typename F::Elem *in = static_cast<const typename F::Elem *>(d_in);
    const size_t out_elem = out_type == SAVGOL_HIP_F32 ? 4 : 2;
    if (route == 1) {
        Job2DSt16<F> job;
        memset(&job, 0, sizeof(job));
        job.rows = rows; job.cols = cols; job.in_stride = in_stride; job.out_stride = out_stride;
        job.in_pitch = in_pitch; job.out_pitch = out_pitch;
        job.nx = filter->config.half_window_x; job.ny = filter->config.half_window_y;
        job.boundary = (boundary == SAVGOL2D_BOUNDARY_VALID || boundary == SAVGOL2D_BOUNDARY_REFLECT) ? boundary : SAVGOL2D_BOUNDARY_CONSTANT;
        H::fill(job.st, in_type, out_type);
        // chunks of images as enqueue_frame cuts them for the twin
        const size_t max_img = ((size_t)1 << 30) / ((size_t)((cols + 63) / 64) * (size_t)(rows + 1)) + 1;
        int rc = 0;
        for (size_t i0 = 0; i0 < images && rc == 0; i0 += max_img) {
            const unsigned ni = (unsigned)(images - i0 < max_img ? images - i0 : max_img);
            job.in = in + (long long)i0 * in_pitch;
            job.out = static_cast<unsigned char *>(d_out) + i0 * (size_t)out_pitch * out_elem;
            rc = sg2d_launch_rolling_st16<F>(job.nx > job.ny ? job.nx : job.ny, terms, &job, factors, filter->scale, ni, st);
            if (rc == 1 && i0 > 0) rc = -1;                  // cannot happen: the first chunk's answer holds for all
        }
        if (rc == 0) return hip_ok(hipGetLastError(), who) ? 0 : -1;
        if (rc < 0) return -1;
        // "not covered": nothing has been enqueued -- the staged route
    }
    return staged16_2d(who, ctx, filter, rows, cols, d_out, out_elem, out_pitch, images, boundary, method, st,
                       [&](size_t i0, float *sin, size_t ni) {
                           sg2d_st16_widen_frames<F>(in + (long long)i0 * in_pitch, in_type, in_stride, in_pitch, sin, rows, cols, ni, st);
                       },
                       [&](const float *sout, void *out, size_t ni, int xlo, int xhi, int ylo, int yhi) {
                           sg2d_st16_out_frames<F>(sout, out, out_type, out_stride, out_pitch, rows, cols, xlo, xhi, ylo, yhi, ni, st);
                       });
}

}  // namespace sg

extern "C" {

bool savgol2d_config_valid(const Savgol2DConfig *config) { return sg2d_config_ok(config) != 0; }

Savgol2DFilter *savgol2d_create(const Savgol2DConfig *config)
{
    if (!sg2d_config_ok(config)) {
        fprintf(stderr, "savgol2d_create: invalid configuration\n");
        return nullptr;
    }
    Savgol2DFilter *f = static_cast<Savgol2DFilter *>(malloc(sizeof(Savgol2DFilter)));
    if (!f) return nullptr;
    f->config = *config;
    f->window_width = 2 * config->half_window_x + 1;
    f->window_height = 2 * config->half_window_y + 1;
    f->window_area = f->window_width * f->window_height;
    f->num_terms = savgol2d_num_terms(config->poly_order);
    f->scale = sg2d_scale(config);
    f->weights = static_cast<float *>(malloc(sizeof(float) * (size_t)f->window_area));
    double coef[SAVGOL2D_MAX_TERMS];
    if (!f->weights || sg2d_weights_fill(config, f->weights, coef) != 0) {
        if (f->weights) fprintf(stderr, "savgol2d_create: weight computation failed\n");
        free(f->weights);
        free(f);
        return nullptr;
    }
    return f;
}

void savgol2d_destroy(Savgol2DFilter *filter)
{
    if (!filter) return;
    free(filter->weights);
    free(filter);
}

int savgol2d_apply_valid(const Savgol2DFilter *filter, const float *input, int rows, int cols, int in_stride, float *output,
                         int out_stride)
{
    if (!filter || !input || !output) return -1;
    if (rows - 2 * filter->config.half_window_y <= 0 || cols - 2 * filter->config.half_window_x <= 0) return -1;
    return sg::host_apply("savgol2d_apply_valid", filter, input, rows, cols, in_stride, output, out_stride,
                          SAVGOL2D_BOUNDARY_VALID, true);
}

int savgol2d_apply(const Savgol2DFilter *filter, const float *input, int rows, int cols, int in_stride, float *output,
                   int out_stride, Savgol2DBoundary boundary)
{
    if (!filter || !input || !output) return -1;
    if (boundary == SAVGOL2D_BOUNDARY_VALID &&
        (rows - 2 * filter->config.half_window_y <= 0 || cols - 2 * filter->config.half_window_x <= 0)) return -1;
    return sg::host_apply("savgol2d_apply", filter, input, rows, cols, in_stride, output, out_stride, (int)boundary, false);
}

int savgol2d_apply_batch_f32(const Savgol2DFilter *filter, const float *d_in, int rows, int cols, int in_stride,
                             size_t in_image_pitch, float *d_out, int out_stride, size_t out_image_pitch, size_t images,
                             Savgol2DBoundary boundary, int method, void *stream)
{
    return sg::enqueue_2d("savgol2d_apply_batch_f32", filter, d_in, rows, cols, in_stride, (long long)in_image_pitch, d_out,
                          out_stride, (long long)out_image_pitch, images, (int)boundary, method, static_cast<hipStream_t>(stream));
}

// ---- the 2-D batch calls on 16-bit storage (contract: savgol_hip.h): apply16_2d / route16_2d above with the call's description.  The int16 call's
//      input has one type: its in_type is not looked at ----
int savgol2d_apply_batch_h16_route(const Savgol2DFilter *filter, const void *d_in, int in_type, int rows, int cols, int in_stride, size_t in_image_pitch,
                                   const void *d_out, int out_type, int out_stride, size_t out_image_pitch, size_t images, Savgol2DBoundary boundary, int method)
{
    float factors[sg::SEP_FACTOR_FLOATS];
    int terms = 0;
    return sg::route16_2d<sg::H16Host2D>(filter, d_in, in_type, rows, cols, in_stride, (long long)in_image_pitch, d_out, out_type, out_stride, (long long)out_image_pitch,
                                         images, (int)boundary, method, factors, &terms);
}

int savgol2d_apply_batch_h16(const Savgol2DFilter *filter, const void *d_in, int in_type, int rows, int cols, int in_stride, size_t in_image_pitch,
                             void *d_out, int out_type, int out_stride, size_t out_image_pitch, size_t images, Savgol2DBoundary boundary, int method,
                             void *stream)
{
    return sg::apply16_2d<sg::H16Host2D>(filter, d_in, in_type, rows, cols, in_stride, (long long)in_image_pitch, d_out, out_type, out_stride, (long long)out_image_pitch,
                                         images, (int)boundary, method, static_cast<hipStream_t>(stream));
}

int savgol2d_apply_batch_i16_route(const Savgol2DFilter *filter, const int16_t *d_in, int rows, int cols, int in_stride, size_t in_image_pitch, const void *d_out,
                                   int out_type, int out_stride, size_t out_image_pitch, size_t images, Savgol2DBoundary boundary, int method)
{
    float factors[sg::SEP_FACTOR_FLOATS];
    int terms = 0;
    return sg::route16_2d<sg::I16Host2D>(filter, d_in, SAVGOL_HIP_I16, rows, cols, in_stride, (long long)in_image_pitch, d_out, out_type, out_stride,
                                         (long long)out_image_pitch, images, (int)boundary, method, factors, &terms);
}

int savgol2d_apply_batch_i16(const Savgol2DFilter *filter, const int16_t *d_in, int rows, int cols, int in_stride, size_t in_image_pitch, void *d_out, int out_type,
                             int out_stride, size_t out_image_pitch, size_t images, Savgol2DBoundary boundary, int method, void *stream)
{
    return sg::apply16_2d<sg::I16Host2D>(filter, d_in, SAVGOL_HIP_I16, rows, cols, in_stride, (long long)in_image_pitch, d_out, out_type, out_stride,
                                         (long long)out_image_pitch, images, (int)boundary, method, static_cast<hipStream_t>(stream));
}

// ---- device entry points of the derivative frames.  Square windows: a separable frame per output, each through enqueue_frame --
//      x-dominant frames first, then the rest, two of them with the same number of terms (the Hessian's xy and yy) in ONE walk over
//      the input; the Laplacian is one frame of the summed kernel (no temporary frame, no add pass).  Other window shapes: one pass per
//      output through enqueue_2d; the Laplacian both dense sums over one read of each tile. ----
namespace sg {

struct DerivSpec { int dx, dy; float *out; };

static int enqueue_derivatives(const char *who, int nx, int ny, int order, const float *d_in, int rows, int cols, int in_stride,
                               size_t in_pitch, const DerivSpec *specs, int nspec, bool sum_into_one, int out_stride,
                               size_t out_pitch, size_t images, float delta_x, float delta_y, int boundary, hipStream_t st)
{
    Savgol2DConfig cfg;
    memset(&cfg, 0, sizeof(cfg));
    cfg.half_window_x = (uint8_t)nx; cfg.half_window_y = (uint8_t)ny; cfg.poly_order = (uint8_t)order;
    cfg.delta_x = delta_x; cfg.delta_y = delta_y;
    if (nx < 0 || nx > 255 || ny < 0 || ny > 255 || order < 0 || order > 255) { sg_set_error("%s: invalid configuration", who); return -1; }
    float *outs[SEP_MAX_OUTPUTS];
    for (int i = 0; i < nspec; ++i) {
        cfg.deriv_x = (uint8_t)specs[i].dx; cfg.deriv_y = (uint8_t)specs[i].dy;
        if (!sg2d_config_ok(&cfg)) { sg_set_error("%s: invalid configuration", who); return -1; }
        outs[i] = specs[i].out;
    }
    Job2D job;
    int rc = make_job(who, nx, ny, d_in, outs, nspec, rows, cols, in_stride, (long long)in_pitch, out_stride, (long long)out_pitch, images,
                      boundary, job);
    if (rc != 0) return rc > 0 ? 0 : -1;
    DeviceCtx *ctx = ctx_get();
    if (!ctx) return -1;

    if (nx != ny) {
        CachedFilter fs[SEP_MAX_OUTPUTS];
        for (int i = 0; i < nspec; ++i) {
            cfg.deriv_x = (uint8_t)specs[i].dx; cfg.deriv_y = (uint8_t)specs[i].dy;
            if (!fs[i].get(&cfg)) return -1;
        }
        if (!sum_into_one) {
            for (int i = 0; i < nspec; ++i)                  // the rolling kernel on zero-padded factors where it is built for the rank, else dense
                if (enqueue_2d(who, fs[i].f, d_in, rows, cols, in_stride, (long long)in_pitch, specs[i].out, out_stride, (long long)out_pitch,
                               images, boundary, 0, st) != 0) return -1;
            return 0;
        }
        // the Laplacian of a rectangular window: BOTH dense sums from one read of the tile, added as the reference adds its two frames
        // (bit-identical to savgol2d_laplacian; round 5 summed the two kernels into one table, whose re-rounded taps put the result
        // 1.38e-6 from the oracle where the reference's xx + yy is at 1.22e-6).  Nothing but launches: capturable into a hipGraph.
        const Savgol2DFilter *fxx = fs[0].f, *fyy = fs[1].f;
        const float *d_w1 = ctx_table(ctx, fxx->weights, sizeof(float) * (size_t)fxx->window_area, 0x2d000000u + (unsigned)(nx * 64 + ny));
        const float *d_w2 = d_w1 ? ctx_table(ctx, fyy->weights, sizeof(float) * (size_t)fyy->window_area, 0x2d000000u + (unsigned)(nx * 64 + ny)) : nullptr;
        if (!d_w1 || !d_w2) return -1;
        job.scale = fxx->scale;
        job.tiles_x = (cols + T2_W - 1) / T2_W;
        job.tiles_y = (rows + T2_H - 1) / T2_H;
        const size_t lds = sizeof(float) * (size_t)(2 * ((fxx->window_area + 3) & ~3) + (T2_W + 2 * nx) * (T2_H + 2 * ny));
        for (size_t i0 = 0; i0 < images; i0 += 65535) {
            const size_t ni = images - i0 < 65535 ? images - i0 : 65535;
            job.in = d_in + (long long)i0 * (long long)in_pitch;
            job.out = specs[0].out + (long long)i0 * (long long)out_pitch;
            hipLaunchKernelGGL(sg2d_direct2_kernel, dim3((unsigned)(job.tiles_x * job.tiles_y), (unsigned)ni), dim3(256), lds, st, job, d_w1, d_w2, fyy->scale);
        }
        return hip_ok(hipGetLastError(), who) ? 0 : -1;
    }

    const int n = nx;
    float factors[SEP_MAX_OUTPUTS][SEP_FACTOR_FLOATS];
    SepFrame frames[SEP_MAX_OUTPUTS];
    int nframes = 0;
    if (sum_into_one) {
        // the Laplacian: ONE frame of the summed kernel sxx*Wxx + syy*Wyy (the only summed form: d = (2,0) + (0,2), which the key takes for granted)
        static thread_local double Wd[33 * 33], Wsum[33 * 33];
        const int ws = 2 * n + 1;
        const SummedKey key = {n, order, delta_x, delta_y};
        int t = summed_factors_cached(key, nullptr, factors[0]);
        if (t < 0) {
            for (int i = 0; i < ws * ws; ++i) Wsum[i] = 0.0;
            for (int i = 0; i < nspec; ++i) {
                cfg.deriv_x = (uint8_t)specs[i].dx; cfg.deriv_y = (uint8_t)specs[i].dy;
                if (sg2d_kernel_double(&cfg, Wd) != 0) { sg_set_error("%s: weight computation failed", who); return -1; }
                const double sc = (double)sg2d_scale(&cfg);
                for (int k = 0; k < ws * ws; ++k) Wsum[k] += sc * Wd[k];
            }
            t = summed_factors_cached(key, Wsum, factors[0]);
        }
        if (t <= 0) { sg_set_error("%s: kernel is not separable with <= %d terms", who, SEP_MAX_TERMS); return -1; }
        cfg.deriv_x = 0; cfg.deriv_y = 0;
        frames[nframes++] = SepFrame{factors[0], t, 1.0f, cfg, nullptr, specs[0].out};
    } else {
        for (int i = 0; i < nspec; ++i) {
            cfg.deriv_x = (uint8_t)specs[i].dx; cfg.deriv_y = (uint8_t)specs[i].dy;
            const int t = sep_factors_cached(&cfg, factors[i]);
            if (t <= 0) { sg_set_error("%s: kernel is not separable with <= %d terms", who, SEP_MAX_TERMS); return -1; }
            frames[nframes++] = SepFrame{factors[i], t, sg2d_scale(&cfg), cfg, nullptr, specs[i].out};
        }
    }
    // x-dominant frames first, each on its own (horizontal pass first: the order that keeps them inside the parity rule); of the frames
    // left, two with the same number of terms share one launch -- the input read once, the vertical ring shared (12 B per pixel of HBM
    // traffic instead of 16)
    int left[SEP_MAX_OUTPUTS], nleft = 0;
    for (int i = 0; i < nframes; ++i) {
        if (!sg2d_x_dominant(frames[i].cfg.deriv_x, frames[i].cfg.deriv_y)) left[nleft++] = i;
        else if (enqueue_frame(who, ctx, job, n, true, 0, frames[i], images, st) != 0) return -1;
    }
    if (nleft == 2 && frames[left[0]].terms == frames[left[1]].terms) {
        const SepFrame &a = frames[left[0]], &b = frames[left[1]];
        Job2D j = job;
        j.out = a.out;
        rc = sg2d_launch_rolling2(n, a.terms, j, a.factors, a.scale, b.factors, b.scale, b.out, (unsigned)images, ctx->cu_count, st);
        if (rc < 0) return -1;
        if (rc == 0) nleft = 0;
    }
    for (int i = 0; i < nleft; ++i)
        if (enqueue_frame(who, ctx, job, n, true, 0, frames[left[i]], images, st) != 0) return -1;
    return hip_ok(hipGetLastError(), who) ? 0 : -1;
}

// ---- savgol2d_gradient_batch_i16 (contract: savgol_hip.h): the gradient on int16 frames, the counterpart of apply16_2d above for the fp32 gradient call.
//      It stands here because its staged route IS enqueue_derivatives.  The route rule is sg_2d_grad16_host.hpp's, asked by the call and by _route alike. ----
static const char *const GRAD16_WHO = "savgol2d_gradient_batch_i16";

// what the route decision has prepared for the launches that follow: frame 0 = gx (d/dx), 1 = gy (d/dy); a frame that is not requested is left alone
struct Grad16Frames {
    bool want[2];
    Savgol2DConfig cfg[2];
    float factors[2][SEP_FACTOR_FLOATS];
    int terms[2];
};

// The call's refusals in the header's order, then its route: -1 = refused (text set), 0 = nothing to do (no images) or STAGED, 1 = DIRECT.  Touches no device.
static int plan_grad16(int nx, int ny, int order, const int16_t *d_in, int rows, int cols, int in_stride, long long in_pitch, const void *d_gx, const void *d_gy, int out_type,
                       int out_stride, long long out_pitch, size_t images, float delta_x, float delta_y, int boundary, Grad16Frames &fr)
{
    const char *who = GRAD16_WHO;
    if (out_type != SAVGOL_HIP_I16 && out_type != SAVGOL_HIP_F32) {
        sg_set_error("%s: out_type %d is not served: SAVGOL_HIP_I16 (%d) and SAVGOL_HIP_F32 (%d) are", who, out_type, SAVGOL_HIP_I16, SAVGOL_HIP_F32);
        return -1;
    }
    if (!d_in) { sg_set_error("%s: NULL pointer", who); return -1; }
    // the configuration and geometry texts of the fp32 gradient call (enqueue_derivatives, make_job)
    if (nx < 0 || nx > 255 || ny < 0 || ny > 255 || order < 0 || order > 255) { sg_set_error("%s: invalid configuration", who); return -1; }
    const void *outs[2] = {d_gx, d_gy};
    for (int i = 0; i < 2; ++i) {
        fr.want[i] = outs[i] != nullptr;
        fr.terms[i] = 0;
        memset(&fr.cfg[i], 0, sizeof(fr.cfg[i]));
        fr.cfg[i].half_window_x = (uint8_t)nx; fr.cfg[i].half_window_y = (uint8_t)ny; fr.cfg[i].poly_order = (uint8_t)order;
        fr.cfg[i].deriv_x = i == 0 ? 1 : 0; fr.cfg[i].deriv_y = i == 0 ? 0 : 1;
        fr.cfg[i].delta_x = delta_x; fr.cfg[i].delta_y = delta_y;
        if (fr.want[i] && !sg2d_config_ok(&fr.cfg[i])) { sg_set_error("%s: invalid configuration", who); return -1; }
    }
    if (!geometry_ok(who, nx, ny, rows, cols, in_stride, out_stride, boundary)) return -1;
    if (images == 0) return 0;
    const size_t out_elem = out_type == SAVGOL_HIP_F32 ? 4 : 2;
    const uintptr_t in0 = reinterpret_cast<uintptr_t>(d_in), gx0 = reinterpret_cast<uintptr_t>(d_gx), gy0 = reinterpret_cast<uintptr_t>(d_gy);
    for (int i = 0; i < 2; ++i)
        if (fr.want[i] && frames_overlap(in0, 2, in_pitch, in_stride, i == 0 ? gx0 : gy0, out_elem, out_pitch, out_stride, rows, cols, images)) {
            sg_set_error("%s: input and output frames overlap (2-D filtering cannot run in place; compared byte-wise)", who);
            return -1;
        }
    if (fr.want[0] && fr.want[1] && frames_overlap(gx0, out_elem, out_pitch, out_stride, gy0, out_elem, out_pitch, out_stride, rows, cols, images)) {
        sg_set_error("%s: the two output frames overlap (compared byte-wise)", who);
        return -1;
    }
    // the route.  SAVGOL_HIP_2D_GRAD_I16_DIRECT is read at every call (tools/time_2d_grad_i16.py times both routes interleaved in one process);
    // SAVGOL_HIP_ROLL_TILE once, as the fp32 launcher reads it
    const char *const direct_text = getenv("SAVGOL_HIP_2D_GRAD_I16_DIRECT");
    static const bool roll_tile_env = [] { const char *e = getenv("SAVGOL_HIP_ROLL_TILE"); return !e || atoi(e) != 0; }();
    GradShapeI16 shape;
    memset(&shape, 0, sizeof(shape));
    shape.nx = nx; shape.ny = ny; shape.rows = rows; shape.cols = cols;
    shape.in_stride = in_stride; shape.in_pitch = in_pitch; shape.out_stride = out_stride; shape.out_pitch = out_pitch;
    shape.in_base = in0; shape.want_gx = fr.want[0]; shape.want_gy = fr.want[1]; shape.gx_base = gx0; shape.gy_base = gy0;
    shape.out_elem = (int)out_elem;
    shape.roll_tile_switch = roll_tile_env;
    shape.direct_switch = !direct_text || atoi(direct_text) != 0;
    if (nx == ny && nx >= 1 && nx <= GRAD_I16_DIRECT_MAX_N) {
        // what the twin's launchers ask of each requested frame's factors: gx -- hf_dispatch's one-launch forms (one term, or two whose x factors share a
        // parity; every vector of definite parity); gy -- launch_roll's general tile, asked of the launcher itself (nothing is launched)
        const int n = nx;
        const size_t tstride = (size_t)2 * (2 * n + 2);
        for (int i = 0; i < 2; ++i)
            if (fr.want[i]) fr.terms[i] = sep_factors_cached(&fr.cfg[i], fr.factors[i]);
        if (fr.want[0] && (fr.terms[0] == 1 || fr.terms[0] == 2)) {
            bool ok = true;
            float sx[2] = {0.0f, 0.0f}, sy;
            for (int t = 0; t < fr.terms[0]; ++t)
                ok = ok && vector_parity(fr.factors[0] + t * tstride, n, &sx[t]) && vector_parity(fr.factors[0] + t * tstride + (2 * n + 2), n, &sy);
            shape.gx_direct = ok && (fr.terms[0] == 1 || sx[0] == sx[1]);
        }
        if (fr.want[1] && (fr.terms[1] == 1 || fr.terms[1] == 2))
            shape.gy_direct = sg2d_launch_rolling_gen_i16(n, fr.terms[1], nullptr, fr.factors[1], sg2d_scale(&fr.cfg[1]), 0, nullptr) == 0;
    }
    return grad_plan_i16(shape) == GRAD_I16_DIRECT ? 1 : 0;
}

// STAGED: the twin itself.  Whole frames per piece (grad_stage_i16) widened ONCE, enqueue_derivatives scratch to scratch for the requested frames, each
// converted out; one stream-ordered allocate / free pair per call.  Pieces of whole frames do not change bits: neither the horizontal-first kernel nor the
// general tile carries anything from row to row, and every other 2-D kernel computes its outputs independently.
static int staged_grad16(DeviceCtx *ctx, int nx, int ny, int order, const int16_t *d_in, int rows, int cols, int in_stride, long long in_pitch, void *const (&outs)[2],
                         int out_type, int out_stride, long long out_pitch, size_t images, float delta_x, float delta_y, int boundary, hipStream_t st)
{
    const char *who = GRAD16_WHO;
    const FrameStageH16 g = grad_stage_i16(rows, cols, images);
    const size_t side = (g.frames * g.frame * sizeof(float) + 255) & ~(size_t)255;
    const int nspec = (outs[0] ? 1 : 0) + (outs[1] ? 1 : 0);
    char *scratch = static_cast<char *>(scratch_alloc(ctx, (size_t)(1 + nspec) * side, st, who));
    if (!scratch) return -1;
    float *sin = reinterpret_cast<float *>(scratch);
    DerivSpec specs[2];
    void *dst[2];
    int k = 0;
    for (int i = 0; i < 2; ++i)
        if (outs[i]) { specs[k] = DerivSpec{i == 0 ? 1 : 0, i == 0 ? 0 : 1, reinterpret_cast<float *>(scratch + (size_t)(1 + k) * side)}; dst[k] = outs[i]; ++k; }
    const bool valid = boundary == SAVGOL2D_BOUNDARY_VALID;
    const int xlo = valid ? nx : 0, xhi = valid ? cols - nx : cols, ylo = valid ? ny : 0, yhi = valid ? rows - ny : rows;
    const size_t out_elem = out_type == SAVGOL_HIP_F32 ? 4 : 2;
    int rc = 0;
    for (size_t i0 = 0; i0 < images && rc == 0; i0 += g.frames) {
        const size_t ni = images - i0 < g.frames ? images - i0 : g.frames;
        sg2d_st16_widen_frames<I16Family2D>(d_in + (long long)i0 * in_pitch, SAVGOL_HIP_I16, in_stride, in_pitch, sin, rows, cols, ni, st);
        rc = enqueue_derivatives(who, nx, ny, order, sin, rows, cols, g.stride, g.frame, specs, nspec, false, g.stride, g.frame, ni, delta_x, delta_y, boundary, st);
        if (rc != 0) break;
        for (int s = 0; s < nspec; ++s)
            sg2d_st16_out_frames<I16Family2D>(specs[s].out, static_cast<char *>(dst[s]) + i0 * (size_t)out_pitch * out_elem, out_type, out_stride, out_pitch, rows, cols,
                                              xlo, xhi, ylo, yhi, ni, st);
    }
    const bool freed = scratch_free(scratch, st, who);
    if (rc != 0 || !freed) return -1;
    return hip_ok(hipGetLastError(), who) ? 0 : -1;
}

static int gradient16_2d(int nx, int ny, int order, const int16_t *d_in, int rows, int cols, int in_stride, long long in_pitch, void *d_gx, void *d_gy, int out_type,
                         int out_stride, long long out_pitch, size_t images, float delta_x, float delta_y, int boundary, hipStream_t st)
{
    const char *who = GRAD16_WHO;
    if (!d_gx && !d_gy) return 0;                            // as the twin: no frame requested, nothing looked at
    static thread_local Grad16Frames fr;
    const int route = plan_grad16(nx, ny, order, d_in, rows, cols, in_stride, in_pitch, d_gx, d_gy, out_type, out_stride, out_pitch, images, delta_x, delta_y, boundary, fr);
    if (route < 0) return -1;
    if (images == 0) return 0;
    DeviceCtx *ctx = ctx_get();
    if (!ctx) return -1;
    void *const outs[2] = {d_gx, d_gy};
    const size_t out_elem = out_type == SAVGOL_HIP_F32 ? 4 : 2;
    bool launched = false;
    if (route == 1) {
        // DIRECT: enqueue_derivatives' own preparation -- the factors of sep_factors_cached (plan_grad16), sg2d_scale, the term sums fitted to the frame's
        // dense table (roll_passes_hf), enqueue_frame's image chunks -- so the taps and sigma are the twin's by construction.  gx first, then gy.
        const int n = nx;
        Job2DI16 job;
        memset(&job, 0, sizeof(job));
        job.rows = rows; job.cols = cols; job.in_stride = in_stride; job.out_stride = out_stride;
        job.in_pitch = in_pitch; job.out_pitch = out_pitch;
        job.nx = nx; job.ny = ny;
        job.boundary = (boundary == SAVGOL2D_BOUNDARY_VALID || boundary == SAVGOL2D_BOUNDARY_REFLECT) ? boundary : SAVGOL2D_BOUNDARY_CONSTANT;
        job.st.out_f32 = out_type == SAVGOL_HIP_F32 ? 1 : 0;
        const size_t tstride = (size_t)2 * (2 * n + 2);
        float sigma[SEP_MAX_TERMS] = {0.0f, 0.0f, 0.0f, 0.0f};
        CachedFilter held;
        if (fr.want[0]) {
            const Savgol2DFilter *dense = held.get(&fr.cfg[0]);
            if (!dense) { sg_set_error("%s: weight computation failed", who); return -1; }
            hf_term_sums(n, fr.terms[0], fr.factors[0], dense, sigma);
        }
        const size_t max_img = ((size_t)1 << 30) / ((size_t)((cols + 63) / 64) * (size_t)(rows + 1)) + 1;
        int rc = 0;
        for (int i = 0; i < 2 && rc == 0; ++i) {
            if (!fr.want[i]) continue;
            const float scale = sg2d_scale(&fr.cfg[i]);
            for (size_t i0 = 0; i0 < images && rc == 0; i0 += max_img) {
                const unsigned ni = (unsigned)(images - i0 < max_img ? images - i0 : max_img);
                job.in = d_in + (long long)i0 * in_pitch;
                job.out = static_cast<char *>(outs[i]) + i0 * (size_t)out_pitch * out_elem;
                if (i == 0) rc = sg2d_launch_rolling_hf_i16(n, job, fr.factors[0], scale, sigma[0], fr.terms[0] == 2 ? fr.factors[0] + tstride : nullptr, sigma[1], ni,
                                                            ctx->cu_count, st);
                else rc = sg2d_launch_rolling_gen_i16(n, fr.terms[1], &job, fr.factors[1], scale, ni, st);
                if (rc == 0) launched = true;
            }
        }
        if (rc == 0) return hip_ok(hipGetLastError(), who) ? 0 : -1;
        if (rc < 0) return -1;
        // "not covered": before anything has been enqueued it is the staged route's; after a launch it is an error
        if (launched) { sg_set_error("%s: a kernel of the direct route refused its frame after another had been enqueued", who); return -1; }
    }
    return staged_grad16(ctx, nx, ny, order, d_in, rows, cols, in_stride, in_pitch, outs, out_type, out_stride, out_pitch, images, delta_x, delta_y, boundary, st);
}

}  // namespace sg

int savgol2d_gradient_batch_i16_route(int half_win_x, int half_win_y, int poly_order, const int16_t *d_in, int rows, int cols, int in_stride, size_t in_image_pitch,
                                      const void *d_grad_x, const void *d_grad_y, int out_type, int out_stride, size_t out_image_pitch, size_t images, float delta_x,
                                      float delta_y, Savgol2DBoundary boundary)
{
    if (!d_grad_x && !d_grad_y) return 0;
    static thread_local sg::Grad16Frames fr;
    return sg::plan_grad16(half_win_x, half_win_y, poly_order, d_in, rows, cols, in_stride, (long long)in_image_pitch, d_grad_x, d_grad_y, out_type, out_stride,
                           (long long)out_image_pitch, images, delta_x, delta_y, (int)boundary, fr);
}

int savgol2d_gradient_batch_i16(int half_win_x, int half_win_y, int poly_order, const int16_t *d_in, int rows, int cols, int in_stride, size_t in_image_pitch,
                                void *d_grad_x, void *d_grad_y, int out_type, int out_stride, size_t out_image_pitch, size_t images, float delta_x, float delta_y,
                                Savgol2DBoundary boundary, void *stream)
{
    return sg::gradient16_2d(half_win_x, half_win_y, poly_order, d_in, rows, cols, in_stride, (long long)in_image_pitch, d_grad_x, d_grad_y, out_type, out_stride,
                             (long long)out_image_pitch, images, delta_x, delta_y, (int)boundary, static_cast<hipStream_t>(stream));
}

int savgol2d_gradient_batch_f32(int half_win_x, int half_win_y, int poly_order, const float *d_in, int rows, int cols, int in_stride,
                                size_t in_image_pitch, float *d_grad_x, float *d_grad_y, int out_stride, size_t out_image_pitch,
                                size_t images, float delta_x, float delta_y, Savgol2DBoundary boundary, void *stream)
{
    sg::DerivSpec specs[2];
    int n = 0;
    if (d_grad_x) specs[n++] = sg::DerivSpec{1, 0, d_grad_x};
    if (d_grad_y) specs[n++] = sg::DerivSpec{0, 1, d_grad_y};
    if (n == 0) return 0;
    return sg::enqueue_derivatives("savgol2d_gradient_batch_f32", half_win_x, half_win_y, poly_order, d_in, rows, cols, in_stride,
                                   in_image_pitch, specs, n, false, out_stride, out_image_pitch, images, delta_x, delta_y, (int)boundary,
                                   static_cast<hipStream_t>(stream));
}

int savgol2d_hessian_batch_f32(int half_win_x, int half_win_y, int poly_order, const float *d_in, int rows, int cols, int in_stride,
                               size_t in_image_pitch, float *d_xx, float *d_xy, float *d_yy, int out_stride, size_t out_image_pitch,
                               size_t images, float delta_x, float delta_y, Savgol2DBoundary boundary, void *stream)
{
    if (poly_order < 2) { sg_set_error("savgol2d_hessian_batch_f32: poly_order must be >= 2"); return -1; }
    sg::DerivSpec specs[3];
    int n = 0;
    if (d_xx) specs[n++] = sg::DerivSpec{2, 0, d_xx};
    if (d_xy) specs[n++] = sg::DerivSpec{1, 1, d_xy};
    if (d_yy) specs[n++] = sg::DerivSpec{0, 2, d_yy};
    if (n == 0) return 0;
    return sg::enqueue_derivatives("savgol2d_hessian_batch_f32", half_win_x, half_win_y, poly_order, d_in, rows, cols, in_stride,
                                   in_image_pitch, specs, n, false, out_stride, out_image_pitch, images, delta_x, delta_y, (int)boundary,
                                   static_cast<hipStream_t>(stream));
}

int savgol2d_laplacian_batch_f32(int half_win_x, int half_win_y, int poly_order, const float *d_in, int rows, int cols, int in_stride,
                                 size_t in_image_pitch, float *d_out, int out_stride, size_t out_image_pitch, size_t images,
                                 float delta_x, float delta_y, Savgol2DBoundary boundary, void *stream)
{
    if (poly_order < 2) { sg_set_error("savgol2d_laplacian_batch_f32: poly_order must be >= 2"); return -1; }
    if (!d_out) { sg_set_error("savgol2d_laplacian_batch_f32: NULL pointer"); return -1; }
    const sg::DerivSpec specs[2] = {sg::DerivSpec{2, 0, d_out}, sg::DerivSpec{0, 2, d_out}};
    return sg::enqueue_derivatives("savgol2d_laplacian_batch_f32", half_win_x, half_win_y, poly_order, d_in, rows, cols, in_stride,
                                   in_image_pitch, specs, 2, true, out_stride, out_image_pitch, images, delta_x, delta_y, (int)boundary,
                                   static_cast<hipStream_t>(stream));
}

// ---- helper wrappers (reference :462-618: one create / apply / destroy per requested output, each reading the input again) ----
// Same outputs bit for bit -- the dense kernel per output, the Laplacian's fp32 add over the whole frame -- but the frame crosses
// the host link once: one upload, one dense launch per output, one download per output.  The filters (host least squares) come
// from the per-configuration cache the device entry points use.
}  // extern "C"

namespace sg {

struct HostDeriv { int dx, dy; float *out; };

static int host_derivatives(const char *who, int nx, int ny, int order, const HostDeriv *specs, int nspec, const float *input, int rows,
                            int cols, int stride, float delta_x, float delta_y, int boundary, bool laplacian)
{
    if (nspec == 0) return 0;
    CachedFilter fs[SEP_MAX_OUTPUTS];
    for (int i = 0; i < nspec; ++i) {
        Savgol2DConfig cfg;
        memset(&cfg, 0, sizeof(cfg));
        cfg.half_window_x = (uint8_t)nx; cfg.half_window_y = (uint8_t)ny; cfg.poly_order = (uint8_t)order;
        cfg.deriv_x = (uint8_t)specs[i].dx; cfg.deriv_y = (uint8_t)specs[i].dy; cfg.delta_x = delta_x; cfg.delta_y = delta_y;
        if (nx < 0 || nx > 255 || ny < 0 || ny > 255 || order < 0 || order > 255) { fprintf(stderr, "savgol2d_create: invalid configuration\n"); return -1; }
        if (!fs[i].get(&cfg)) return -1;
    }
    const bool valid = boundary == SAVGOL2D_BOUNDARY_VALID;
    if (!input || rows <= 0 || cols <= 0 || (valid && (rows - 2 * ny <= 0 || cols - 2 * nx <= 0))) return -1;
    DeviceCtx *ctx = ctx_get();
    if (!ctx) { fprintf(stderr, "%s: %s\n", who, savgol_hip_last_error()); return -1; }
    std::lock_guard<std::recursive_mutex> lock(ctx->mu);
    const int dstride = (cols + 3) & ~3;
    const size_t frame = (size_t)rows * dstride;
    float *d_in = static_cast<float *>(ctx_arena(ctx, sizeof(float) * frame * (size_t)(1 + nspec)));
    if (!d_in) { fprintf(stderr, "%s: %s\n", who, savgol_hip_last_error()); return -1; }
    bool ok = hip_ok(hipMemcpy2D(d_in, sizeof(float) * dstride, input, sizeof(float) * stride, sizeof(float) * cols, rows, hipMemcpyHostToDevice),
                     "H2D copy");
    for (int i = 0; i < nspec && ok; ++i) {
        float *d_out = d_in + frame * (size_t)(1 + i);
        if (laplacian && valid) {
            // reference :598-613: d2/dx2 lands inside the caller's frame, d2/dy2 inside a temporary (zeros here), then the WHOLE frame is
            // added: the caller's border values pass through that add, so they have to be on the device too
            if (i == 0) ok = hip_ok(hipMemcpy2D(d_out, sizeof(float) * dstride, specs[0].out, sizeof(float) * stride, sizeof(float) * cols, rows,
                                                hipMemcpyHostToDevice), "H2D copy");
            else ok = hip_ok(hipMemsetAsync(d_out, 0, sizeof(float) * frame, nullptr), "hipMemsetAsync");
        }
        ok = ok && enqueue_2d(who, fs[i].f, d_in, rows, cols, dstride, 0, d_out, dstride, 0, 1, boundary, 1, nullptr) == 0;
    }
    if (ok && laplacian) {
        float *d_a = d_in + frame, *d_b = d_in + 2 * frame;
        hipLaunchKernelGGL(sg2d_add_kernel, dim3((cols + 255) / 256, rows), dim3(256), 0, nullptr, d_a, d_b, rows, cols, dstride);
        ok = hip_ok(hipGetLastError(), "add kernel") &&
             hip_ok(hipMemcpy2D(specs[0].out, sizeof(float) * stride, d_a, sizeof(float) * dstride, sizeof(float) * cols, rows, hipMemcpyDeviceToHost),
                    "D2H copy");
    } else if (ok) {
        const int r0 = valid ? ny : 0, c0 = valid ? nx : 0;
        const int nr = valid ? rows - 2 * ny : rows, nc = valid ? cols - 2 * nx : cols;
        for (int i = 0; i < nspec && ok; ++i)
            ok = hip_ok(hipMemcpy2D(specs[i].out + (size_t)r0 * stride + c0, sizeof(float) * stride,
                                    d_in + frame * (size_t)(1 + i) + (size_t)r0 * dstride + c0, sizeof(float) * dstride, sizeof(float) * nc, nr,
                                    hipMemcpyDeviceToHost), "D2H copy");
    }
    if (!ok) { fprintf(stderr, "%s: %s\n", who, savgol_hip_last_error()); return -1; }
    return 0;
}

}  // namespace sg

extern "C" {

int savgol2d_gradient(int half_win_x, int half_win_y, int poly_order, const float *input, int rows, int cols, int stride,
                      float *grad_x, float *grad_y, float delta_x, float delta_y, Savgol2DBoundary boundary)
{
    sg::HostDeriv specs[2];
    int n = 0;
    if (grad_x) specs[n++] = {1, 0, grad_x};
    if (grad_y) specs[n++] = {0, 1, grad_y};
    return sg::host_derivatives("savgol2d_gradient", half_win_x, half_win_y, poly_order, specs, n, input, rows, cols, stride, delta_x, delta_y,
                                (int)boundary, false);
}

int savgol2d_hessian(int half_win_x, int half_win_y, int poly_order, const float *input, int rows, int cols, int stride,
                     float *hess_xx, float *hess_xy, float *hess_yy, float delta_x, float delta_y, Savgol2DBoundary boundary)
{
    if (poly_order < 2) {
        fprintf(stderr, "savgol2d_hessian: poly_order must be >= 2\n");
        return -1;
    }
    sg::HostDeriv specs[3];
    int n = 0;
    if (hess_xx) specs[n++] = {2, 0, hess_xx};
    if (hess_xy) specs[n++] = {1, 1, hess_xy};
    if (hess_yy) specs[n++] = {0, 2, hess_yy};
    return sg::host_derivatives("savgol2d_hessian", half_win_x, half_win_y, poly_order, specs, n, input, rows, cols, stride, delta_x, delta_y,
                                (int)boundary, false);
}

int savgol2d_laplacian(int half_win_x, int half_win_y, int poly_order, const float *input, int rows, int cols, int stride,
                       float *output, float delta_x, float delta_y, Savgol2DBoundary boundary)
{
    if (poly_order < 2) {
        fprintf(stderr, "savgol2d_laplacian: poly_order must be >= 2\n");
        return -1;
    }
    if (!input || !output) return -1;
    const sg::HostDeriv specs[2] = {{2, 0, output}, {0, 2, nullptr}};
    return sg::host_derivatives("savgol2d_laplacian", half_win_x, half_win_y, poly_order, specs, 2, input, rows, cols, stride, delta_x, delta_y,
                                (int)boundary, true);
}

}  // extern "C"
