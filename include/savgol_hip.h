/*
 * savgol_hip.h -- device-side C ABI of the MI355X Savitzky-Golay library (libsavgol_hip.so).
 *
 * The reference API (savgolFilter.h, savgol_stream.h, savgol2d.h) is one signal / one stream /
 * one image at a time, fp32, host pointers.  The workloads this library is built for -- thousands
 * of channels resident in HBM, tens of thousands of concurrent streams, image stacks, fp64 --
 * cannot be expressed through it, so this header ADDS entry points next to the drop-in ones.
 * Everything here is plain C: raw device pointers, sizes, an opaque `void *stream`
 * (a hipStream_t; NULL = the default stream).  No torch / C++ types cross this boundary.
 *
 * Each function names the reference routine whose arithmetic it performs.  All of them return
 * 0 on success and -1 on error unless stated otherwise; savgol_hip_last_error() has the text.
 * Launches are asynchronous on `stream`.  What "enqueue only" means, entry point by entry point:
 *   - savgol_apply[_valid]_batch_f32/f64, savgol_apply[_valid]_multi_batch_f32, savgol2d_apply_batch_f32, savgol2d_gradient/hessian/laplacian_batch_f32 (square and
 *     rectangular windows), savgol_streambank_push/_push_full/_push_block/_push_block_multi/_flush/_flush_leading/_reset: launches only --
 *     capturable into a hipGraph AFTER one warm-up call with the same filter: the FIRST call with a new filter content
 *     uploads its tables (hipMalloc + a synchronous hipMemcpy, then cached for the life of the process; tables are never
 *     freed or moved, so captured graphs and queued launches stay valid) and, for the derivative frames, solves the
 *     least-squares problem on the host (cached per configuration);
 *   - savgol_apply_strided_batch_f32[_ex]: launches only when the fields are 4-byte aligned and disjoint (the fused kernel);
 *     otherwise (reference summation order, unaligned or overlapping fields) launches plus a stream-ordered allocation /
 *     free pair for its two dense frames, from the library's own retained memory pool (no shared scratch, no lock, no
 *     synchronise); savgol2d_apply_rowband_f32 and channels longer than 2^30 samples use the same pool for their scratch;
 *   - savgol_apply_strided_multi_batch_f32: a fused call (savgol_apply_strided_multi_batch_f32_route > 0) makes launches only and allocates nothing --
 *     capturable after one warm-up call with the same filters; a call that falls back is `njobs` savgol_apply_strided_batch_f32_ex calls;
 *   - savgol_streambank_push_block_h16: launches plus ONE stream-ordered allocation / free pair from the same pool (the fp32 frames of its head, or
 *     of the staged route's chunk); capturable after one warm-up call like savgol_streambank_push_block;
 *   - savgol_streambank_push_block_multi_h16: a fused call makes launches plus ONE such pair (the two fp32 frames of its head, shared by the banks);
 *     a call that falls back is `count` savgol_streambank_push_block_h16 calls; capturable after one warm-up call;
 *   - savgol_streambank_push_block_multi_i16: the same on int16 samples -- a fused call makes launches plus ONE such pair; a call that falls back is
 *     `count` savgol_streambank_push_block_i16 calls; capturable after one warm-up call;
 *   - savgol_streambank_save/_load, savgol_hip_synchronize and every host-pointer drop-in call of savgolFilter.h /
 *     savgol_stream.h / savgol2d.h: synchronous by nature (they return host data).
 * Short host-pointer calls (savgol_apply / _valid / _strided on <= 4096 samples and <= 64 K multiply-adds, every savgol_stream_* call
 * on one SavgolStream) do not launch: one workgroup stays resident behind a doorbell (csrc/sg_k1d_misc.hip) and answers in 6-8 us
 * with the reference's bits.  It leaves by itself after 60 us without a call -- a device-wide synchronise issued by the caller
 * waits at most that long for it -- is told to leave before the library's own hipFree / hipMalloc, is restarted by the next short
 * call, and after an unanswered call stays away for 1 s, doubling to 64 s.  Environment: SAVGOL_HIP_SMALL_SERVICE=0 disables it
 * (every call then launches), SAVGOL_HIP_SMALL_SERVICE_IDLE_US sets the idle time (50 ... 5 000 000).  The library installs no
 * signal handlers unless SAVGOL_HIP_BAR_DOORBELL=1 asks for doorbells in BAR-mapped device memory (probed with a guarded store).
 * Accuracy of the default fp32 device kernels against the double-accumulation oracle (normwise, max|err| / max|ref|): ONE rule, everywhere --
 * <= max(1e-6, 1.1 x the error of the reference's OWN fp32 arithmetic on the same samples), i.e. 1e-6 outright wherever the reference itself
 * meets 1e-6 (smoothing filters that pass the signal: always).  1-D: three interleaved partial sums per output, block moments from half window
 * 20; 2-D: the pass whose taps cancel harder runs first (derivative frames included: no wider constant since round 6).  tests/_util.py holds the
 * rule, tools/parity_margins.py prints every comparison's margin.  Bit-identical-to-the-reference results:
 * SAVGOL_HIP_OPT_REFERENCE_SUMMATION (1-D), method 1 (2-D), and every host-pointer drop-in call.
 */
#ifndef SAVGOL_HIP_H
#define SAVGOL_HIP_H

#include <stdbool.h>
#include <stddef.h>
#include <stdint.h>
#include "savgolFilter.h"
#include "savgol2d.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---------------------------------------------------------------- runtime ------------- */
int         savgol_hip_device_count(void);          /* usable HIP devices (0 = none)       */
int         savgol_hip_set_device(int ordinal);     /* device used by THIS thread's calls  */
int         savgol_hip_get_device(void);
int         savgol_hip_synchronize(void *stream);       /* hipStreamSynchronize; the scratch pool keeps its threshold (savgol_hip_trim_scratch hands it back) */
/* Calls that need a temporary frame (staged strided path, reference-order batches, channel ends of very long channels, row-band strips)
 * take it from the library's own stream-ordered pool, which keeps up to 256 MiB of freed blocks for the next call
 * (SAVGOL_HIP_SCRATCH_KEEP_MB).  This returns every unused byte of it to the driver now.  0 / -1. */
int         savgol_hip_trim_scratch(void);
size_t      savgol_hip_scratch_reserved(void);          /* bytes the pool holds right now (hipMemPoolAttrReservedMemCurrent) */
/* Multi-GPU: the path shards by independent units (channels, streams, images) with no data-path collective, so the whole
 * "context" is: one process (or thread) per GPU calls savgol_hip_set_device(local_rank) and filters its own contiguous slice.
 * This returns that slice [*lo, *hi) of `total` units for `rank` of `world_size` (the first total % world_size ranks take
 * one unit more); -1 on bad arguments.  bench.py and the Python mirror use the same arithmetic.                        */
int         savgol_hip_shard_range(size_t total, int world_size, int rank, size_t *lo, size_t *hi);
const char *savgol_hip_last_error(void);            /* thread-local, never NULL            */
const char *savgol_hip_version(void);
/* Process-wide switches; defaults reproduce the reference bit for bit in behaviour, quirks included.
 * SAVGOL_HIP_OPT_CORRECT_LEADING_EDGE = 1: in POLYNOMIAL mode the first n outputs of an ODD derivative get the
 * mathematically correct sign.  (The reference applies the trailing-edge rows to reversed data, which negates odd
 * derivatives on the leading edge -- src/savgolFilter.c:773-777)  Affects the 1-D batch / apply
 * entry points only; the streaming path keeps the reference behaviour.                                           */
enum { SAVGOL_HIP_OPT_CORRECT_LEADING_EDGE = 1, SAVGOL_HIP_OPT_REFERENCE_SUMMATION = 2, SAVGOL_HIP_OPT_PLAIN_SUMMATION = 3,
       SAVGOL_HIP_OPT_BOUNDARY_AWARE = 4, SAVGOL_HIP_OPT_TILE_WIDTH = 5 };
/* SAVGOL_HIP_OPT_REFERENCE_SUMMATION = 1: the fp32 1-D batch / valid / strided DEVICE entry points sum each output in
 * the reference's own order (convolve_ilp, src/savgolFilter.c:547-580: four chains, separate multiply and add) and are
 * then bit-identical to the reference's savgol_apply; 1.5x (n=5) to 2.1x (n=32) slower than the default FMA kernel, which
 * agrees with it to 1e-6.  The host-pointer drop-in calls of savgolFilter.h always use that order.
 * SAVGOL_HIP_OPT_PLAIN_SUMMATION = 1: the fp32 batch kernels apply all 2n+1 taps one by one at every half window.  By default, from half
 * window 20 up (poly_order >= 2, derivative <= 1), a lane treats its 32 outputs as two groups of 16 and replaces the taps that fall on the
 * samples common to a group's windows by block moments (the taps are a polynomial of degree <= poly_order in the tap index;
 * csrc/sg_k1d_momenth.hpp): 19 instead of 33 packed multiply-adds per output pair at half_window 32, the same 1e-6 agreement with the fp64
 * oracle, different last bits.  Filters whose table is not such a polynomial (hand-edited center_weights), poly_order > 6, poly_order < 2,
 * second derivatives and half windows below 20 always use the plain sum.
 * SAVGOL_HIP_OPT_BOUNDARY_AWARE = 1: the paths that IGNORE config.boundary in the reference honour it:
 *   - savgol_apply_strided / savgol_apply_strided_batch_f32 (reference src/savgolFilter.c:877-934 always uses the polynomial
 *     edge rows) apply the configured mode, like savgol_apply;
 *   - savgol_stream_* and savgol_streambank_* (reference src/savgol_stream.c:43-74 likewise) emit REFLECT / CONSTANT edges in
 *     push_full / flush / flush_leading: the first and last n outputs are the centre taps on the index-remapped window
 *     (get_padded_sample, :442-482), so push_full... + flush equals savgol_apply in that mode.  PERIODIC needs samples from the
 *     other end of the signal and keeps the polynomial rows.  Read when a stream or bank is created / a stream call is made;
 *     set it before.  Default 0: the reference's behaviour.
 * SAVGOL_HIP_OPT_TILE_WIDTH: which of the two tile widths the 1-D batch kernels run with where both are built (fp32 half windows
 *   <= 18, fp64 <= 24).  0 (default): by job size -- the 12 / 16 KiB tile from 16384 tiles up, the 8 KiB tile below; 1: always the
 *   8 KiB tile; 2: always the wide one.  A tuning and test knob: smoothing filters give the same bits either way; derivative
 *   filters run on tiles centred on their own mean, so their last bits depend on the tile width.                              */
int         savgol_hip_set_option(int option, int value);
/* The same switches PER CALL: the *_ex forms of the 1-D device entry points take them as flags, so two threads (or two
 * calls) can run different summation orders or tile widths at the same time; the options above are only the DEFAULTS the
 * non-_ex entry points use (savgol_hip_default_flags() returns them as flags).  A flag word is complete: an _ex call
 * ignores the process-wide options.  TILE_NARROW and TILE_WIDE exclude each other; neither = by job size.               */
enum { SAVGOL_BATCH_REFERENCE_SUMMATION = 1u, SAVGOL_BATCH_PLAIN_SUMMATION = 2u, SAVGOL_BATCH_TILE_NARROW = 4u, SAVGOL_BATCH_TILE_WIDE = 8u,
       SAVGOL_BATCH_CORRECT_LEADING_EDGE = 16u, SAVGOL_BATCH_BOUNDARY_AWARE = 32u /* strided calls only */,
       SAVGOL_BATCH_MOMENT_F64 = 64u /* fp64 calls, half_window 24..32: block moments replace the taps on the lanes' common block (~36 multiply-adds
                                        per output instead of 65).  The block's share is a least-squares projection of the block's own promoted taps,
                                        so the result is within ~1e-7 (bar: 1e-6) of the default fp64 path instead of its 1e-12 -- on zero-mean data
                                        and equally on data riding on an offset, a ramp or a parabola (the projection keeps the taps' moments of
                                        order < 3 exactly; tested to offsets of 1e3 and slopes of 0.5 per sample).  Opt-in for that reason. */ };
unsigned    savgol_hip_default_flags(void);
/* Diagnostic (host only, no device needed): the constant table the half-lane block-moment kernel (fp32 batch calls, half windows 20..32:
 * csrc/sg_k1d_momenth.hpp; layout in csrc/sg_k1d_host.hpp, at most SAVGOL_HIP_MOMENT_TABLE_FLOATS floats).  Returns the number of block
 * moments the kernel will use (3, 5 or 7), 0 when the filter keeps the plain 2n+1-tap sum (half windows below 20, poly_order > 6, tables that
 * are not a polynomial), -1 on NULL.                                                                                                       */
#define SAVGOL_HIP_MOMENT_TABLE_FLOATS 400
int         savgol_hip_momenth_table(const SavgolFilter *filter, float *table);
/* The same for the fp64 block-moment kernel (savgol_apply[_valid]_batch_f64_tol / SAVGOL_BATCH_MOMENT_F64, half windows 24..32:
 * csrc/sg_k1d_moment64.hpp; layout MOMENT64_OFF_W / _PHI / _C in csrc/sg_k1d_host.hpp, SAVGOL_HIP_MOMENT64_TABLE_DOUBLES doubles).  Same return
 * convention: 3, 5 or 7 block moments, 0 when the filter keeps the tap-by-tap kernel (half windows outside 24..32, poly_order > 6, tables that
 * are not a polynomial), -1 on NULL.                                                                                                        */
#define SAVGOL_HIP_MOMENT64_TABLE_DOUBLES 278
int         savgol_hip_moment64_table(const SavgolFilter *filter, double *table);
/* Diagnostic (host only): the fit behind the fused stream bank's block-moment tiles (csrc/sg_stream_dma.hip, half windows 12..20).  `center_weights`:
 * the 2n+1 fp32 taps a bank applies; `coefficients`: 3 x SAVGOL_HIP_STREAM_MOMENT_OFFSETS floats, [s][off] = weight of moment s (basis 1, t - 3.5,
 * (t - 3.5)^2 - 5.25 on t = 0..7) of the 8-tick block that starts `off` taps into a window.  Returns the number of moments (1..3), 0 when the
 * table is not a polynomial of degree <= 2 to 3e-7 of its largest tap (the bank then runs tap by tap), -1 on NULL.                              */
#define SAVGOL_HIP_STREAM_MOMENT_OFFSETS 34
int         savgol_hip_stream_moment_table(int half_window, const float *center_weights, float *coefficients);

/* ---------------------------------------------------------------- table export ------- *
 * The reference's on-disk format for a filter's tables: the C header its savgol_export tool writes
 * (src/savgol_export.c:145-282 -- `%+.10ef` values four per line, CENTER_WEIGHTS[2n+1], EDGE_WEIGHTS[n][2n+1], a naive
 * inline apply).  Host only.  `prefix` NULL = "SAVGOL"; `timestamp` NULL = now ("%Y-%m-%d %H:%M:%S", the tool's
 * "Generated by" line).  Writes at most capacity-1 bytes + NUL into buf (buf may be NULL) and returns the full length
 * of the text, -1 on a bad filter.  Byte-identical to the tool's output for the same filter, prefix and timestamp.   */
long savgol_export_header(const SavgolFilter *filter, const char *prefix, const char *timestamp, char *buf, size_t capacity);

/* ---------------------------------------------------------------- 1-D batch ----------- *
 * channels independent signals, row-major: sample i of channel c at base[c*ld + i].
 * Arithmetic of savgol_apply (reference src/savgolFilter.c:743-804): centre taps on the
 * interior, filter->config.boundary on the first/last n samples (POLYNOMIAL rows incl. the
 * reference's reversed leading edge; REFLECT / PERIODIC / CONSTANT by index remap).
 * No row of d_in may share a byte with a row of d_out (checked: -1); interleaved layouts whose rows stay apart are fine
 * (in = buf[:, 0, :], out = buf[:, 1, :] with equal pitches).  IN PLACE is the one exception, and its contract is exact: d_out == d_in AND
 * out_ld == in_ld, the full-length entry points only (not the _valid ones), channels of at most 2^30 samples.  The call then returns the
 * OUT-OF-PLACE answer (bit-identical to it; the reference's own in-place loop reads samples it has already overwritten -- a documented
 * divergence, as for the host-pointer call): the even tiles of every channel run first and hand their first / last samples to their odd
 * neighbours through a stream-ordered stash of 2n samples per tile, then the odd tiles, then the edge rows (+3-6 % over out of place).  length >= 2n+1, and any size_t beyond that, like the
 * reference's: a channel longer than 2^30 samples is enqueued as sub-rows of 2^29 outputs plus its two
 * ends (same arithmetic per output; a little stream-ordered scratch for the ends).
 * f32: fp32 tables, fp32 FMA accumulation (within 1e-6 normwise of the fp64 oracle).
 * f64: the same fp32 tables promoted exactly to double, double accumulation, the reference's
 *      float 1/dt_scale promoted -- there is no fp64 path in the reference.
 *      The centre taps must be (anti)symmetric bit for bit, as savgol_create builds them
 *      (tap[k] == +-tap[2n-k]); a hand-edited table that is not returns -1.
 * NaN / Inf.  A non-finite input sample makes non-finite exactly the outputs whose window, after the boundary remap, contains it (the reference's loops skip
 * no tap: src/savgolFilter.c:547-580, :763-800; a POLYNOMIAL edge row uses all 2n+1 samples of its end, so a special among them reaches all n outputs of that
 * end), and nothing else; a NaN makes them NaN.  The kernels that apply the taps one by one -- fp32 below half_window 20, second derivatives and poly_order < 2,
 * PLAIN_SUMMATION, the default fp64 calls, the multi-output and the strided calls -- have the fp64 oracle's NaN / +Inf / -Inf at its positions;
 * REFERENCE_SUMMATION has the reference's, bit for bit.  The block-moment kernels (fp32 from half_window 20 by default, fp64 under rel_tol >= 1e-6 /
 * SAVGOL_BATCH_MOMENT_F64 at 24..32, the 16-bit and int16 calls on the same half windows) may give NaN where the reference gives +-Inf: an Inf inside the
 * samples common to a group's windows makes every moment of that block +-Inf, and their sum mixes signs (Inf - Inf).  In place, VALID and every layout keep
 * the same rule (tests/test_gpu_1d_nonfinite.py).                                                                                                         */
int savgol_apply_batch_f32(const SavgolFilter *filter, const float *d_in, float *d_out,
                           size_t channels, size_t length, size_t in_ld, size_t out_ld,
                           void *stream);
int savgol_apply_batch_f64(const SavgolFilter *filter, const double *d_in, double *d_out,
                           size_t channels, size_t length, size_t in_ld, size_t out_ld,
                           void *stream);
int savgol_apply_batch_f32_ex(const SavgolFilter *filter, const float *d_in, float *d_out,
                              size_t channels, size_t length, size_t in_ld, size_t out_ld,
                              unsigned flags, void *stream);
int savgol_apply_batch_f64_ex(const SavgolFilter *filter, const double *d_in, double *d_out,
                              size_t channels, size_t length, size_t in_ld, size_t out_ld,
                              unsigned flags, void *stream);
/* fp64 with the tolerance stated in the call: `rel_tol` is the normwise distance from the fp64 oracle (promoted fp32 tables, double accumulation)
 * the caller accepts, and it picks the kernel.  rel_tol >= 1e-6 -- the bar BASELINE's fp64 configs state -- runs the block-moment kernel at half
 * windows 24..32 when the filter's table is the polynomial savgol_create builds (measured <= 1.5e-7 of the oracle, 0.78-0.84 of the HBM roofline at
 * n = 32 against the default's 0.66-0.70); a tighter rel_tol, other half windows and hand-edited tables run the tap-by-tap kernel (1e-12).  Same
 * process-wide defaults as the plain entry points otherwise.  The _ex flag SAVGOL_BATCH_MOMENT_F64 is the same choice as a flag.
 * What the 1.5e-7 holds for: poly_order <= 6, derivatives 0..2, every boundary mode and VALID, on the synthetic workload (zero-mean tones plus
 * noise) AND on signals of unit variation riding on an offset up to 1e3, a ramp up to 0.5 per sample or a parabola (tests/test_gpu_1d.py,
 * test_f64_tolerance_call_on_offsets_and_ramps): the kernel's replacement taps keep the table's moments of order 0, 1, 2 to rounding, so what
 * lies under the signal meets no error beyond double rounding at its own size.  savgol_hip_moment64_table returns the table for inspection.  */
int savgol_apply_batch_f64_tol(const SavgolFilter *filter, const double *d_in, double *d_out,
                               size_t channels, size_t length, size_t in_ld, size_t out_ld,
                               double rel_tol, void *stream);
int savgol_apply_valid_batch_f64_tol(const SavgolFilter *filter, const double *d_in, double *d_out,
                                     size_t channels, size_t length, size_t in_ld, size_t out_ld,
                                     double rel_tol, void *stream);
/* savgol_apply_valid (:821-850) per channel: writes length-2n samples at d_out[c*out_ld + 0..] */
int savgol_apply_valid_batch_f32(const SavgolFilter *filter, const float *d_in, float *d_out,
                                 size_t channels, size_t length, size_t in_ld, size_t out_ld,
                                 void *stream);
int savgol_apply_valid_batch_f64(const SavgolFilter *filter, const double *d_in, double *d_out,
                                 size_t channels, size_t length, size_t in_ld, size_t out_ld,
                                 void *stream);
int savgol_apply_valid_batch_f32_ex(const SavgolFilter *filter, const float *d_in, float *d_out,
                                    size_t channels, size_t length, size_t in_ld, size_t out_ld,
                                    unsigned flags, void *stream);
int savgol_apply_valid_batch_f64_ex(const SavgolFilter *filter, const double *d_in, double *d_out,
                                    size_t channels, size_t length, size_t in_ld, size_t out_ld,
                                    unsigned flags, void *stream);
/* savgol_apply_strided (:877-934) on device memory: element i of channel c is the float at
 * (char*)base + c*channel_pitch + i*stride + offset (bytes).  Edges are always POLYNOMIAL.     */
int savgol_apply_strided_batch_f32(const SavgolFilter *filter,
                                   const void *d_in, size_t in_stride, size_t in_offset, size_t in_channel_pitch,
                                   void *d_out, size_t out_stride, size_t out_offset, size_t out_channel_pitch,
                                   size_t channels, size_t count, void *stream);
int savgol_apply_strided_batch_f32_ex(const SavgolFilter *filter,
                                      const void *d_in, size_t in_stride, size_t in_offset, size_t in_channel_pitch,
                                      void *d_out, size_t out_stride, size_t out_offset, size_t out_channel_pitch,
                                      size_t channels, size_t count, unsigned flags, void *stream);
/* Several FIELDS of the records from one pass: job k applies jobs[k].filter to the field at in_offset of every record of the input grid
 * (d_in, in_stride, in_channel_pitch) and writes the field at out_offset of the output grid (d_out, out_stride, out_channel_pitch); offsets are bytes
 * inside a record.  Jobs may share an input field (value, velocity and acceleration of one field); d_out may be d_in (the in-place array-of-structs
 * case).  `flags` is a complete SAVGOL_BATCH_* word, those of savgol_apply_strided_batch_f32_ex.
 * CONTRACT: the call leaves memory as `njobs` calls of savgol_apply_strided_batch_f32_ex(jobs[k].filter, d_in, in_stride, jobs[k].in_offset, ..., flags)
 * in the caller's order would leave it, BIT FOR BIT: NaN positions coincide, and bytes no job writes (other fields, the slack between `count` records
 * and the channel pitch, anything outside the grids) stay as they were.
 * Refusals, -1 with a text naming this call, before any device call and with nothing written, in this order: 1. unknown flags, or TILE_NARROW with
 * TILE_WIDE;  2. NULL jobs, d_in or d_out;  3. njobs outside 1..SAVGOL_STRIDED_MULTI_MAX_JOBS;  4. a NULL jobs[k].filter (k ascending);  5. a
 * filter struct that is not a valid SavgolFilter (k ascending);  6. count below a job's window size (k ascending).  channels == 0 returns 0.
 * FUSED (one pass over the records per launch, sg1d_strided_multi_kernel) needs all of: njobs >= 2; every filter the same half_window; under
 * SAVGOL_BATCH_BOUNDARY_AWARE the same config.boundary; no SAVGOL_BATCH_REFERENCE_SUMMATION; every field address, both strides and both channel pitches
 * multiples of 4 and both strides >= 4; count <= 2^30; no output field sharing a byte with any job's input field or another job's output field (one
 * record grid with offsets at least 4 bytes apart cyclically, or two grids that do not overlap at all); record sizes inside the measured table (equal
 * strides of 8, 12, 16, 20, 32 or 64 bytes: DESIGN.md 4.1f).  A fused call runs the jobs in order in launches of at most 4 jobs, a last group of one
 * job as a single call.  Every other call IS the `njobs` single calls in order -- which is also what gives a job that reads an earlier job's output
 * its sequential meaning.
 * _route: what the call would do, enqueuing nothing and needing no device: the number of fused launches, 0 = njobs single calls (or channels == 0),
 * -1 = refused with the same text.                                                                                                              */
enum { SAVGOL_STRIDED_MULTI_MAX_JOBS = 16 };
typedef struct { const SavgolFilter *filter; size_t in_offset, out_offset; } SavgolFieldJob;   /* byte offsets inside a record */
int savgol_apply_strided_multi_batch_f32(const SavgolFieldJob *jobs, int njobs,
                                         const void *d_in, size_t in_stride, size_t in_channel_pitch,
                                         void *d_out, size_t out_stride, size_t out_channel_pitch,
                                         size_t channels, size_t count, unsigned flags, void *stream);
int savgol_apply_strided_multi_batch_f32_route(const SavgolFieldJob *jobs, int njobs,
                                               const void *d_in, size_t in_stride, size_t in_channel_pitch,
                                               void *d_out, size_t out_stride, size_t out_channel_pitch,
                                               size_t channels, size_t count, unsigned flags);
/* Several filters on ONE batch in one pass: smoothing and derivatives (d = 0 / 1 / 2 ...) of the same signals read the input once.
 * `filters` and `d_outs` are host arrays of `count` entries, 1 <= count <= SAVGOL_MULTI_MAX_FILTERS; d_outs[k] is a device pointer and every
 * output has the pitch out_ld.  All filters share config.half_window and config.boundary (poly_order, derivative and time_step may differ;
 * a mismatch returns -1 naming the field).  `flags` is a complete SAVGOL_BATCH_* word, as in the _ex calls.
 * Output k is bit-identical to savgol_apply[_valid]_batch_f32_ex(filters[k], d_in, d_outs[k], ..., flags | SAVGOL_BATCH_PLAIN_SUMMATION, stream).
 * Fused: 2 or 3 outputs per launch, 4 + 4 count bytes per input sample instead of count x 8; count = 4 is two launches of two (the input is
 * read twice); count = 1 is the single call.  These routes stay count single calls (same contract, not fused):
 *   - SAVGOL_BATCH_REFERENCE_SUMMATION;
 *   - channels longer than 2^30 samples (the single calls' sub-row route);
 *   - derivative filters where the single call takes the wide tile (half_window <= 18 with SAVGOL_BATCH_TILE_WIDE, or without a tile flag on
 *     batches of 16384 wide tiles and more): a derivative filter's tiles are centred on their mean, so its bits depend on the tile width.
 *     Pass SAVGOL_BATCH_TILE_NARROW to fuse them as well.  Smoothing filters fuse either way.
 * Returns -1 before any device call on: a NULL filter / input / output pointer, count outside 1..4, mismatched half_window or boundary,
 * length < window, pitches smaller than the row, and any d_outs[k] that shares a byte with d_in or another output (in place is not supported).
 * Like the single calls it only enqueues (after one warm-up call with the same filters), so it can be captured into a graph.
 * fp32 only: the fp64 kernel is issue-bound (65 fp64 FMAs per output), so three fused outputs triple its FMAs to save a third of its bytes. */
#define SAVGOL_MULTI_MAX_FILTERS 4
int savgol_apply_multi_batch_f32(const SavgolFilter *const *filters, int count,
                                 const float *d_in, float *const *d_outs,
                                 size_t channels, size_t length, size_t in_ld, size_t out_ld,
                                 unsigned flags, void *stream);
/* the same with savgol_apply_valid's outputs: length - 2n samples at d_outs[k][c*out_ld + 0..] */
int savgol_apply_valid_multi_batch_f32(const SavgolFilter *const *filters, int count,
                                       const float *d_in, float *const *d_outs,
                                       size_t channels, size_t length, size_t in_ld, size_t out_ld,
                                       unsigned flags, void *stream);

/* 16-bit STORAGE for the 1-D batch call: fp16 or bf16 rows in device memory, fp32 arithmetic inside.  4 bytes per sample (16 -> 16 bit) or 6
 * (16 bit -> fp32) instead of the fp32 call's 8; every kernel behind the batch call is bound by HBM bytes.
 * d_in / d_out are device pointers to rows of `in_type` / `out_type` elements (SAVGOL_HIP_F16: IEEE binary16, SAVGOL_HIP_BF16: bfloat16);
 * in_ld and out_ld count elements of their own buffer's type.  Type pairs (in -> out): f16 -> f16, bf16 -> bf16, f16 -> f32, bf16 -> f32.
 * Every other pair returns -1 naming the pair -- f32 -> f32 included: that is savgol_apply[_valid]_batch_f32[_ex].
 * Arithmetic is exactly the fp32 call's: every input element is widened exactly to fp32 while its tile is staged, the tile runs the fp32 path
 * unchanged (three-chain sum; block moments from half window 20 where the fp32 call takes them; centred tiles for derivative filters; dt
 * scaling; POLYNOMIAL edge rows in the same launch) on the narrow tile, and a result is rounded to the output type ONCE, to nearest even, just
 * before it is stored (NaN stays NaN; overflow to fp16 gives +-Inf as IEEE rounding does).
 * CONTRACT: the output equals, bit for bit, savgol_apply[_valid]_batch_f32_ex(filter, widen(d_in), ..., flags | SAVGOL_BATCH_TILE_NARROW)
 * rounded to nearest even into out_type; for out_type f32 it is that call's output itself.  NaN positions coincide; NaN payloads are free.
 * `flags` is a complete SAVGOL_BATCH_* word, as in the _ex calls: SAVGOL_BATCH_PLAIN_SUMMATION, SAVGOL_BATCH_TILE_NARROW (implied) and
 * SAVGOL_BATCH_CORRECT_LEADING_EDGE are served.  Returns -1 with a text, before any device call, on: SAVGOL_BATCH_REFERENCE_SUMMATION (the
 * reference has no 16-bit form to be identical to), SAVGOL_BATCH_TILE_WIDE, flags of other calls (BOUNDARY_AWARE, MOMENT_F64) or unknown bits, an
 * unserved type pair, a NULL pointer, length < window, a pitch smaller than the row, channels longer than 2^30 samples, and input and output rows
 * that share a byte (in place included: a 16-bit row cannot hold its fp32 halo stash; use separate buffers).
 * Rows whose base and pitch keep every group of four elements naturally aligned (8 bytes for 16-bit rows, 16 for fp32 output) move as vectors; any
 * other base or pitch is served element by element.  Like the single calls it only enqueues (after one warm-up call with the same filter), so it
 * can be captured into a graph.  Several filters on one read of 16-bit rows: savgol_apply[_valid]_multi_batch_h16 below.  Not served in 16 bit: the strided path,
 * the 2-D derivative-frame and row-band calls, fp32 -> 16-bit pairs (int16 samples: savgol_apply[_valid]_batch_i16 below).  The stream bank's block push on 16-bit rows:
 * savgol_streambank_push_block_h16 below; the 2-D batch call on 16-bit frames: savgol2d_apply_batch_h16 below. */
enum { SAVGOL_HIP_F32 = 0, SAVGOL_HIP_F16 = 1, SAVGOL_HIP_BF16 = 2 };   /* storage type of a device buffer */
int savgol_apply_batch_h16(const SavgolFilter *filter, const void *d_in, int in_type, void *d_out, int out_type,
                           size_t channels, size_t length, size_t in_ld, size_t out_ld, unsigned flags, void *stream);
/* the same with savgol_apply_valid's outputs: length - 2n elements at d_out[c*out_ld + 0..] */
int savgol_apply_valid_batch_h16(const SavgolFilter *filter, const void *d_in, int in_type, void *d_out, int out_type,
                                 size_t channels, size_t length, size_t in_ld, size_t out_ld, unsigned flags, void *stream);

/* int16 STORAGE for the 1-D batch call: int16 samples (ADC / DAQ / audio counts) in device memory, fp32 arithmetic inside.  4 bytes per sample
 * (int16 -> int16) or 6 (int16 -> fp32) instead of a widening pass plus the fp32 call's 8.
 * d_in points to rows of int16 elements, d_out to rows of `out_type` elements: SAVGOL_HIP_I16 or SAVGOL_HIP_F32.  in_ld and out_ld count elements
 * of their own buffer.  Every input element is widened exactly to fp32 while its tile is staged and the tile runs the fp32 path unchanged
 * (three-chain sum; block moments from half window 20 where the fp32 call takes them; centred tiles for derivative filters; dt scaling;
 * POLYNOMIAL edge rows in the same launch) on the narrow tile.
 * CONTRACT: the output equals, bit for bit, savgol_apply[_valid]_batch_f32_ex(filter, widen(d_in), ..., flags | SAVGOL_BATCH_TILE_NARROW), where
 * widen is the exact int16 -> fp32 conversion.  For out_type F32 it is that call's output itself (NaN positions coincide; NaN payloads are free).
 * For out_type I16 each fp32 result is converted ONCE, just before it is stored: rounded to nearest, ties to even; saturated to
 * [-32768, 32767], so +-Inf saturate; NaN gives 0.
 * `flags` is a complete SAVGOL_BATCH_* word, as in the _ex calls: SAVGOL_BATCH_PLAIN_SUMMATION, SAVGOL_BATCH_TILE_NARROW (implied) and
 * SAVGOL_BATCH_CORRECT_LEADING_EDGE are served.
 * Returns -1 with a text naming the call, before any device call; the checks run in this order and the first fault wins:
 *   1. flags: SAVGOL_BATCH_REFERENCE_SUMMATION, then SAVGOL_BATCH_TILE_WIDE, then flags of other calls (BOUNDARY_AWARE, MOMENT_F64), then unknown bits;
 *   2. an out_type other than SAVGOL_HIP_I16 / SAVGOL_HIP_F32;
 *   3. a NULL pointer, then length < window, then channels longer than 2^30 samples, then a pitch smaller than the row;
 *   4. input and output rows that share a byte (compared byte-wise: the element sizes may differ; in place is not served).
 * channels == 0 returns 0.  Rows whose base and pitch keep every group of four elements naturally aligned (8 bytes for int16 rows, 16 for fp32
 * output) move as vectors; any other base or pitch is served element by element.  Like its siblings it only enqueues (after one warm-up call with
 * the same filter), so it can be captured into a graph.  Several filters on one read of int16 rows: savgol_apply[_valid]_multi_batch_i16 below.
 * Not served on int16: uint16 samples, a gain or offset per call or channel, int16 -> fp16 / bf16 outputs, the strided and 2-D calls, in place.
 * The stream bank's block push on int16: savgol_streambank_push_block_i16 below. */
enum { SAVGOL_HIP_I16 = 3 };   /* joins SAVGOL_HIP_F32 / _F16 / _BF16 */
int savgol_apply_batch_i16(const SavgolFilter *filter, const int16_t *d_in, void *d_out, int out_type,
                           size_t channels, size_t length, size_t in_ld, size_t out_ld, unsigned flags, void *stream);
/* the same with savgol_apply_valid's outputs: length - 2n elements at d_out[c*out_ld + 0..] */
int savgol_apply_valid_batch_i16(const SavgolFilter *filter, const int16_t *d_in, void *d_out, int out_type,
                                 size_t channels, size_t length, size_t in_ld, size_t out_ld, unsigned flags, void *stream);

/* Several filters on ONE batch of 16-bit rows in one pass: the multi-output call on 16-bit storage.  2 + 2 count bytes per input sample
 * (16 -> 16 bit) instead of count x 4 for count single calls; 8 bytes for a smoothed trace and two derivatives.
 * `filters` and `d_outs` are host arrays of `count` entries, 1 <= count <= SAVGOL_MULTI_MAX_FILTERS, as in savgol_apply_multi_batch_f32; all filters
 * share config.half_window and config.boundary.  d_in holds rows of `in_type` elements; EVERY output holds rows of `out_type` elements with the one
 * pitch out_ld; in_ld and out_ld count elements of their own buffer's type.  Type pairs are those of savgol_apply_batch_h16: f16 -> f16,
 * bf16 -> bf16, f16 -> f32, bf16 -> f32.
 * CONTRACT: output k equals, bit for bit,
 *   savgol_apply[_valid]_batch_h16(filters[k], d_in, in_type, d_outs[k], out_type, ..., flags | SAVGOL_BATCH_PLAIN_SUMMATION, stream)
 * and, equivalently, output k of savgol_apply[_valid]_multi_batch_f32(filters, widen(d_in), ..., flags | SAVGOL_BATCH_TILE_NARROW) rounded ONCE to
 * nearest even into out_type (for out_type f32: that output itself).  NaN positions coincide; NaN payloads are free.
 * `flags` is a complete SAVGOL_BATCH_* word: SAVGOL_BATCH_PLAIN_SUMMATION (implied), SAVGOL_BATCH_TILE_NARROW (implied) and
 * SAVGOL_BATCH_CORRECT_LEADING_EDGE are served.  The narrow tile is implied, so the fp32 call's wide-tile exception does not exist here: every
 * output fuses.  2 or 3 outputs are one launch, 4 are two launches of two (the input is read twice), 1 is the single 16-bit call with
 * SAVGOL_BATCH_PLAIN_SUMMATION.  Outputs land in the caller's order.
 * Returns -1 with a text naming the call, before any device call; the checks run in this order and the first fault wins:
 *   1. flags: SAVGOL_BATCH_REFERENCE_SUMMATION, then SAVGOL_BATCH_TILE_WIDE, then flags of other calls (BOUNDARY_AWARE, MOMENT_F64), then unknown bits;
 *   2. an unserved type pair;
 *   3. a NULL `filters`, `d_outs` or `d_in`;   4. count outside 1..4;   5. a NULL or malformed filters[k] / a NULL d_outs[k], k ascending;
 *   6. filters[k] with another half_window, then another boundary, than filters[0], k ascending;
 *   7. length < window, then channels longer than 2^30 samples, then a pitch smaller than the row;
 *   8. for k ascending: d_outs[k] sharing a byte with the input rows, then with the rows of d_outs[j], j < k (compared byte-wise: the element
 *      sizes may differ; in place is not served).
 * Like its siblings it only enqueues (after one warm-up call with the same filters), so it can be captured into a graph. */
int savgol_apply_multi_batch_h16(const SavgolFilter *const *filters, int count,
                                 const void *d_in, int in_type, void *const *d_outs, int out_type,
                                 size_t channels, size_t length, size_t in_ld, size_t out_ld,
                                 unsigned flags, void *stream);
/* the same with savgol_apply_valid's outputs: length - 2n elements at d_outs[k][c*out_ld + 0..] */
int savgol_apply_valid_multi_batch_h16(const SavgolFilter *const *filters, int count,
                                       const void *d_in, int in_type, void *const *d_outs, int out_type,
                                       size_t channels, size_t length, size_t in_ld, size_t out_ld,
                                       unsigned flags, void *stream);

/* Several filters on ONE batch of int16 rows in one pass: the multi-output call on int16 storage.  2 + 2 count bytes per input sample
 * (int16 -> int16) instead of count x 4 for count single calls; 8 bytes for a smoothed trace and two derivatives.
 * `filters` and `d_outs` are host arrays of `count` entries, 1 <= count <= SAVGOL_MULTI_MAX_FILTERS, as in savgol_apply_multi_batch_f32; all filters
 * share config.half_window and config.boundary.  d_in holds rows of int16 elements; EVERY output holds rows of `out_type` elements, SAVGOL_HIP_I16
 * or SAVGOL_HIP_F32, with the one pitch out_ld; in_ld and out_ld count elements of their own buffer.
 * CONTRACT: output k equals, bit for bit,
 *   savgol_apply[_valid]_batch_i16(filters[k], d_in, d_outs[k], out_type, ..., flags | SAVGOL_BATCH_PLAIN_SUMMATION, stream)
 * and, equivalently, output k of savgol_apply[_valid]_multi_batch_f32(filters, widen(d_in), ..., flags | SAVGOL_BATCH_TILE_NARROW), where widen is
 * the exact int16 -> fp32 conversion.  For out_type F32 it is that output itself (NaN positions coincide; NaN payloads are free).  For out_type I16
 * each fp32 result is converted ONCE, just before it is stored: rounded to nearest, ties to even; saturated to [-32768, 32767], so +-Inf saturate;
 * NaN gives 0.
 * `flags` is a complete SAVGOL_BATCH_* word: SAVGOL_BATCH_PLAIN_SUMMATION (implied), SAVGOL_BATCH_TILE_NARROW (implied) and
 * SAVGOL_BATCH_CORRECT_LEADING_EDGE are served.  The narrow tile is implied, so the fp32 call's wide-tile exception does not exist here: every
 * output fuses.  2 or 3 outputs are one launch, 4 are two launches of two (the input is read twice), 1 is the single int16 call with
 * SAVGOL_BATCH_PLAIN_SUMMATION.  Outputs land in the caller's order.
 * Returns -1 with a text naming the call, before any device call; the checks run in this order and the first fault wins:
 *   1. flags: SAVGOL_BATCH_REFERENCE_SUMMATION, then SAVGOL_BATCH_TILE_WIDE, then flags of other calls (BOUNDARY_AWARE, MOMENT_F64), then unknown bits;
 *   2. an out_type other than SAVGOL_HIP_I16 / SAVGOL_HIP_F32;
 *   3. a NULL `filters`, `d_outs` or `d_in`;   4. count outside 1..4;   5. a NULL or malformed filters[k] / a NULL d_outs[k], k ascending;
 *   6. filters[k] with another half_window, then another boundary, than filters[0], k ascending;
 *   7. length < window, then channels longer than 2^30 samples, then a pitch smaller than the row;
 *   8. for k ascending: d_outs[k] sharing a byte with the input rows, then with the rows of d_outs[j], j < k (compared byte-wise: the element
 *      sizes may differ; in place is not served).
 * channels == 0 returns 0.  Like its siblings it only enqueues (after one warm-up call with the same filters), so it can be captured into a graph.
 * Not served: uint16 samples, int16 -> fp16 / bf16 outputs, a gain or offset per channel, in place. */
int savgol_apply_multi_batch_i16(const SavgolFilter *const *filters, int count,
                                 const int16_t *d_in, void *const *d_outs, int out_type,
                                 size_t channels, size_t length, size_t in_ld, size_t out_ld,
                                 unsigned flags, void *stream);
/* the same with savgol_apply_valid's outputs: length - 2n elements at d_outs[k][c*out_ld + 0..] */
int savgol_apply_valid_multi_batch_i16(const SavgolFilter *const *filters, int count,
                                       const int16_t *d_in, void *const *d_outs, int out_type,
                                       size_t channels, size_t length, size_t in_ld, size_t out_ld,
                                       unsigned flags, void *stream);

/* ---------------------------------------------------------------- stream bank --------- *
 * `streams` independent SavgolStream-equivalents advancing in lock step, state in HBM as a
 * structure of arrays (ring[slot][stream]).  Arithmetic of src/savgol_stream.c: single fp32
 * accumulator, taps in order, separate multiply and add -- outputs are bit-identical to the
 * reference's savgol_stream_push / _push_full / _flush / _flush_leading for every stream.
 * Output rows are [row][stream] with pitch `streams`.                                        */
typedef struct SavgolStreamBank SavgolStreamBank;

SavgolStreamBank *savgol_streambank_create(const SavgolConfig *config, size_t streams);
/* Per-bank choice of the summation, fixed at create (the stream analogue of the 1-D batch path's fast default):
 * SAVGOL_STREAMBANK_FMA: centre outputs of _push / _push_block / _push_full (after the filling tick) are fused multiply-adds --
 *   one v_pk_fma_f32 per tap and stream pair instead of a multiply and an add (reference loop src/savgol_stream.c:25-38), half
 *   the vector instructions of the block push.  NOT the reference's bits: <= 1e-6 (smoothing) / 1.5e-6 (derivatives) normwise of
 *   the fp64 oracle, like the default 1-D batch kernels.  Edge rows (leading burst, _flush, _flush_leading), the resident
 *   tick service and calls of >= 2^31 ticks keep the reference's order.  Half windows <= 16 sum in two interleaved chains in _push
 *   and _push_block alike; above 16 the block push keeps ONE chain per output (its accumulators live in registers) while the
 *   per-tick kernel uses two, so the two calls agree to fp32 rounding there, not bit for bit.
 *   _push at half window 1 sums its three taps in ONE chain: the even / odd split would add x0 + x2 before -2 x1 on a second-derivative bank,
 *   a rounding at twice the streams' offset that the reference's order does not have.  flags 0 == savgol_streambank_create. */
enum { SAVGOL_STREAMBANK_FMA = 1 };
SavgolStreamBank *savgol_streambank_create_ex(const SavgolConfig *config, size_t streams, unsigned flags);
void   savgol_streambank_destroy(SavgolStreamBank *bank);
int    savgol_streambank_reset(SavgolStreamBank *bank, void *stream);
/* one tick = one sample per stream.  Returns 1 when d_out[0..streams) holds centre outputs,
 * 0 while the windows are still filling (d_out untouched), -1 on error.                       */
int    savgol_streambank_push(SavgolStreamBank *bank, const float *d_samples, float *d_out, void *stream);
/* The same tick, and d_out is complete (in memory: write-through stores) when the call returns: the tick kernel's last block writes a sequence
 * number into a word of pinned host memory and the host spins on it -- no hipStreamSynchronize.  The lowest-latency way to take one tick's
 * outputs.  Needs a multiple of 64 streams; otherwise it is push + hipStreamSynchronize.  Same return value as savgol_streambank_push. */
int    savgol_streambank_push_wait(SavgolStreamBank *bank, const float *d_samples, float *d_out, void *stream);
/* with edges: returns the number of output rows written (0, 1, or up to n+1 on the tick that
 * fills the windows, truncated to max_rows), -1 on error.                                     */
int    savgol_streambank_push_full(SavgolStreamBank *bank, const float *d_samples,
                                   float *d_out, int max_rows, void *stream);
/* `ticks` pushes in one launch (ring kept on chip in between): d_samples[t*streams + s],
 * d_out[t*streams + s] is written for every tick t that has a centre output.  Returns the
 * number of ticks that produced output (they are the last ones), -1 on error.
 * Not in place: when [d_samples, d_samples + ticks*streams) and [d_out, d_out + ticks*streams)
 * share a byte the call returns -1 ("overlap" in savgol_hip_last_error()) before any launch,
 * with the bank's counters and ring untouched.  Buffers that touch end to start are fine.     */
int    savgol_streambank_push_block(SavgolStreamBank *bank, const float *d_samples, size_t ticks,
                                    float *d_out, void *stream);
/* The block push on 16-bit STORAGE: fp16 or bf16 samples in, the same type or fp32 out, fp32 arithmetic inside -- 4 bytes per stream-tick
 * (16 -> 16 bit) or 6 (16 bit -> fp32) instead of the fp32 call's 8, and no widened copy of the samples on the caller's side.
 * Rows are [tick][stream] with pitch `streams`, in elements of the buffer's own type.  in_type / out_type: SAVGOL_HIP_F16 or SAVGOL_HIP_BF16,
 * out_type also SAVGOL_HIP_F32; served pairs are savgol_apply_batch_h16's (f16 -> f16, bf16 -> bf16, f16 -> f32, bf16 -> f32).
 * The bank is an ordinary bank (savgol_streambank_create or _create_ex): its ring stays fp32 and holds the samples widened exactly, so this call
 * mixes freely with _push, _push_full, the fp32 _push_block, both flushes, _save / _load and the tick service.
 * CONTRACT.  Let the twin be a bank of the same configuration, flags and history that takes savgol_streambank_push_block on the samples widened
 * exactly to fp32, in 16-byte aligned fp32 buffers.  Every output row equals the twin's row bit for bit, rounded ONCE to nearest even into out_type
 * (out_type f32: the twin's row itself; NaN positions coincide, NaN payloads are free; overflow into fp16 gives +-Inf).  Rows of ticks without an
 * output are not written.  Afterwards counters, write position and ring are the twin's: the savgol_streambank_save blobs are equal byte for byte.
 * The return value is savgol_streambank_push_block's.  None of this depends on the alignment of the 16-bit buffers.
 * Two routes, chosen before anything is enqueued.  TILES -- streams % 128 == 0, ticks >= 64, both bases 16-byte aligned, and the twin takes its
 * LDS-DMA tiles: the first 64 ticks (two bands of tiles) are widened into fp32 scratch and go through the fp32 block push, the rest through the
 * same tiles reading 16-bit rows and storing out_type rows (csrc/sg_stream_dma_h16.hip).  STAGED -- every other call (odd stream counts, unaligned
 * pointers, fewer than 64 ticks, banks whose fp32 call walks or takes register tiles): the samples are widened into aligned fp32 scratch, pushed
 * through the fp32 block push and the outputs rounded out; up to 2^24 stream-ticks (128 MiB of scratch) in one piece, longer calls in chunks of
 * max(64, (2^24 / streams) & ~63) ticks.  ONE EXCEPTION to the contract follows from the chunks: the twin of a chunked call is the same sequence
 * of fp32 block pushes, chunk by chunk.  That changes bits only for a SAVGOL_STREAMBANK_FMA bank with a derivative filter whose fp32 call walks:
 * the walk's items are centred on their own extent, which a chunk boundary cuts.
 * Returns -1 with a text naming the call, before any launch or scratch allocation, counters and ring untouched: a NULL pointer; an unserved
 * type pair (named); input and output ranges that share a byte (compared byte-wise); more than 2^30 ticks (split the call); the bank on another
 * device; the tick service running.  ticks == 0 returns 0. */
int    savgol_streambank_push_block_h16(SavgolStreamBank *bank, const void *d_samples, int in_type, size_t ticks,
                                        void *d_out, int out_type, void *stream);
/* The block push on int16 STORAGE: int16 samples (ADC / DAQ counts) in, int16 or fp32 out, fp32 arithmetic inside -- 4 bytes per stream-tick
 * (int16 -> int16) or 6 (int16 -> fp32) instead of a widening pass, the fp32 call's 8 and a rounding pass on the caller's side.
 * out_type is SAVGOL_HIP_I16 or SAVGOL_HIP_F32.  Rows are [tick][stream] with pitch `streams`, in elements of the buffer's own type.
 * The bank is an ordinary bank: its ring stays fp32 and holds the samples widened exactly, so this call mixes freely with _push, _push_full, the
 * fp32 and 16-bit float block pushes, both flushes, _save / _load and the tick service.
 * CONTRACT: savgol_streambank_push_block_h16's with the int16 conversions of savgol_apply_batch_i16.  Let the twin be a bank of the same
 * configuration, flags and history that takes savgol_streambank_push_block on the samples widened exactly to fp32, in 16-byte aligned fp32 buffers.
 * For out_type F32 every output row is the twin's row bit for bit (NaN positions coincide, NaN payloads are free).  For out_type I16 every output
 * row is the twin's row converted ONCE: rounded to nearest, ties to even; saturated to [-32768, 32767], so +-Inf saturate; NaN gives 0 (a NaN or an
 * Inf can only come out of ring history that fp32 pushes put there).  Rows of ticks without an output are not written.  Afterwards counters, write
 * position and ring are the twin's: the savgol_streambank_save blobs are equal byte for byte.  The return value is savgol_streambank_push_block's.
 * None of this depends on the alignment of the int16 buffers.  The 16-bit float call's one exception carries over unchanged: the twin of a chunked
 * staged call is the same sequence of fp32 block pushes, chunk by chunk.
 * The two routes are savgol_streambank_push_block_h16's, chosen by the same plan before anything is enqueued.  TILES -- streams % 128 == 0,
 * ticks >= 64, both bases 16-byte aligned, and the twin takes its LDS-DMA or block-moment tiles: the first 64 ticks are widened into fp32 scratch,
 * go through the fp32 tiles and are converted out, the rest goes through the same tiles reading int16 rows (csrc/sg_stream_dma_i16.hip).
 * STAGED -- every other call, in the same chunks: one piece up to 2^24 stream-ticks, else max(64, (2^24 / streams) & ~63) ticks.
 * Returns -1 with a text naming the call, before any launch or scratch allocation, counters and ring untouched; the checks run in this order and
 * the first fault wins:
 *   1. a NULL pointer;   2. an out_type other than SAVGOL_HIP_I16 / SAVGOL_HIP_F32 (named);   3. the tick service running, or the bank on another
 *   device;   4. ticks == 0 returns 0;   5. more than 2^30 ticks (split the call);   6. input and output ranges that share a byte (compared
 *   byte-wise: the element sizes may differ; in place is not served).
 * Not served on int16 here: uint16 samples, a gain or offset per call or stream, int16 -> fp16 / bf16 outputs, int16 in _push, _push_full, the
 * flushes and the tick service.  The fused multi-output push on int16 is savgol_streambank_push_block_multi_i16 below
 * (savgol_streambank_push_block_multi_h16 keeps refusing SAVGOL_HIP_I16). */
int    savgol_streambank_push_block_i16(SavgolStreamBank *bank, const int16_t *d_samples, size_t ticks,
                                        void *d_out, int out_type, void *stream);
/* The FUSED MULTI-OUTPUT block push: `count` banks (1..4) take the same block of samples, which is read from memory once -- value, velocity and
 * acceleration of the same sensor streams move 4 + 4 * count bytes per stream-tick instead of 8 * count.
 * `banks` and `d_outs` are host arrays of `count` entries; the banks are ordinary banks (savgol_streambank_create / _create_ex), each with its own
 * filter, ring and counters, all with the same `streams`.  d_samples is one block [ticks][streams]; d_outs[k] is bank k's output block, same pitch.
 * The banks need not share a history, a filter order, a derivative or a time_step.
 * CONTRACT.  Let bank k's twin be a bank of the same configuration, flags and history that takes savgol_streambank_push_block(twin, d_samples, ticks,
 * d_outs[k], stream).  Output k equals the twin's output bit for bit (NaN positions coincide, NaN payloads are free); rows of ticks without an output
 * are not written; bank k's counters, write position and ring are the twin's (the savgol_streambank_save blobs are byte-equal); produced[k] is the
 * twin's return value (`produced` may be NULL).  No tolerance anywhere.  Returns the smallest produced[k], -1 on error; ticks == 0 returns 0.
 * Two routes, chosen before anything is enqueued (csrc/sg_stream_host.hpp, block_plan_multi).  FUSED needs all of: count >= 2; every bank the same
 * half window n and the same SAVGOL_STREAMBANK_FMA flag; n <= 8 (both bank kinds, two and three outputs per launch); streams % 128 == 0; the
 * samples and every output 16-byte aligned; more than 64 ticks; every bank's own block push takes its tap-by-tap LDS-DMA tiles.  Then every bank's
 * first 64 ticks go through its own tiles on its own ring, the rest of the block through one launch that reads each row once and feeds every output
 * (two or three outputs: one launch; four: two launches of two; csrc/sg_stream_dma_multi.hip), and every ring takes its newest samples.  Every other
 * call is `count` single block pushes in the caller's order.  The call only enqueues and allocates nothing: capturable after one warm-up call.
 * Returns -1 with a text naming the call, before any launch, every bank untouched; checked in this order: NULL banks / d_outs / d_samples; count
 * outside 1..4; a NULL banks[k] or d_outs[k]; a bank listed twice; a bank with another `streams` than banks[0]; a bank on another device or with
 * the tick service running; more than 2^30 ticks; d_outs[k] sharing a byte with the samples or with an earlier d_outs[j].
 * _route enqueues nothing and changes nothing: -1 on the refusals above, else the number of fused launches the call would make (0: the call is
 * `count` single block pushes). */
#define SAVGOL_STREAM_MULTI_MAX_BANKS 4
int    savgol_streambank_push_block_multi(SavgolStreamBank *const *banks, int count, const float *d_samples, size_t ticks,
                                          float *const *d_outs, int *produced, void *stream);
int    savgol_streambank_push_block_multi_route(SavgolStreamBank *const *banks, int count, const float *d_samples, size_t ticks,
                                                float *const *d_outs);
/* The FUSED MULTI-OUTPUT block push on 16-bit STORAGE: both of the above at once -- `count` banks (1..4) take the same block of fp16 or bf16 samples,
 * which is read from memory once, and write outputs of the same type or fp32: value, velocity and acceleration of the same sensor streams move
 * 2 + 2 * count bytes per stream-tick (16 -> 16 bit) instead of 4 * count, or 2 + 4 * count (16 bit -> fp32) instead of 6 * count.
 * `banks` and `d_outs` are host arrays of `count` entries; the banks are ordinary banks (fp32 rings), all with the same `streams`.  ONE in_type and ONE
 * out_type serve every output, as in savgol_apply_multi_batch_h16; the served pairs are savgol_streambank_push_block_h16's (f16 -> f16, bf16 -> bf16,
 * f16 -> f32, bf16 -> f32).  d_samples is one block [ticks][streams] of in_type; d_outs[k] is bank k's output block of out_type, same pitch in elements.
 * The banks need not share a history, a filter order, a derivative or a time_step.
 * CONTRACT.  Let bank k's twin be a bank of the same configuration, flags and history that takes the single savgol_streambank_push_block_h16(twin,
 * d_samples, in_type, ticks, d_outs[k], out_type, stream).  Output k equals the twin's output bit for bit, byte for byte (NaN positions coincide, NaN
 * payloads are free); rows of ticks without an output are not written; bank k's counters, write position and ring are the twin's (the
 * savgol_streambank_save blobs are byte-equal); produced[k] is the twin's return value (`produced` may be NULL).  By the single call's own contract
 * every output is therefore also savgol_streambank_push_block_multi's output on the samples widened exactly to fp32, rounded ONCE to nearest even.
 * No tolerance anywhere.  Returns the smallest produced[k], -1 on error; ticks == 0 returns 0.
 * Two routes, chosen before anything is enqueued (csrc/sg_stream_host.hpp, block_plan_multi_h16).  FUSED needs all of: count >= 2; every bank the same
 * half window n and the same SAVGOL_STREAMBANK_FMA flag; n <= 8 (both bank kinds, two and three outputs per launch); streams % 128 == 0; the samples,
 * every output and every ring 16-byte aligned; more than 64 ticks; every bank's twin takes its tap-by-tap LDS-DMA tiles.  Then the first 64 ticks are
 * widened once into fp32 scratch and go, bank after bank, through the bank's own fp32 tiles on its own ring and are rounded out (the twin's own head);
 * the rest of the block goes through one launch that reads each 16-bit row once and feeds every output (two or three outputs: one launch; four: two
 * launches of two; csrc/sg_stream_dma_multi_h16.hip); every ring takes its newest samples.  Every other call is `count` single
 * savgol_streambank_push_block_h16 calls in the caller's order.  A fused call makes launches plus ONE stream-ordered allocation / free pair from the
 * library's pool, like the single 16-bit call: capturable after one warm-up call.
 * Returns -1 with a text naming the call, before any launch or scratch allocation, every bank untouched; checked in this order: NULL banks / d_outs /
 * d_samples; count outside 1..4; a NULL banks[k] or d_outs[k]; an unserved type pair (named; f32 -> anything included); a bank listed twice; a bank
 * with another `streams` than banks[0]; a bank on another device or with the tick service running; more than 2^30 ticks; d_outs[k] sharing a byte with
 * the samples or with an earlier d_outs[j] (compared byte-wise, each buffer with its own element size).
 * _route enqueues nothing and changes nothing: -1 on the refusals above, else the number of fused launches the call would make (0: the call is
 * `count` single 16-bit block pushes). */
int    savgol_streambank_push_block_multi_h16(SavgolStreamBank *const *banks, int count, const void *d_samples, int in_type, size_t ticks,
                                              void *const *d_outs, int out_type, int *produced, void *stream);
int    savgol_streambank_push_block_multi_h16_route(SavgolStreamBank *const *banks, int count, const void *d_samples, int in_type, size_t ticks,
                                                    void *const *d_outs, int out_type);
/* The FUSED MULTI-OUTPUT block push on int16 STORAGE: `count` banks (1..4) take the same block of int16 samples (ADC / DAQ counts), which is read
 * from memory once, and write int16 or fp32 outputs: value, velocity and acceleration of the same sensor streams move 2 + 2 * count bytes per
 * stream-tick (int16 -> int16) instead of 4 * count, or 2 + 4 * count (int16 -> fp32) instead of 6 * count.
 * `banks` and `d_outs` are host arrays of `count` entries; the banks are ordinary banks (fp32 rings), all with the same `streams`.  out_type is
 * SAVGOL_HIP_I16 or SAVGOL_HIP_F32, ONE output type for every output.  d_samples is one block [ticks][streams] of int16; d_outs[k] is bank k's output
 * block of out_type, same pitch in elements.  The banks need not share a history, a filter order, a derivative or a time_step.
 * CONTRACT.  Let bank k's twin be a bank of the same configuration, flags and history that takes the single savgol_streambank_push_block_i16(twin,
 * d_samples, ticks, d_outs[k], out_type, stream).  Output k equals the twin's output byte for byte (fp32 outputs: NaN positions coincide, NaN payloads
 * are free); rows of ticks without an output are not written; bank k's counters, write position and ring are the twin's (the savgol_streambank_save
 * blobs are byte-equal); produced[k] is the twin's return value (`produced` may be NULL).  By the single call's own contract every output is therefore
 * also savgol_streambank_push_block_multi's output on the samples widened exactly to fp32; int16 outputs are that output converted ONCE: rounded to
 * nearest, ties to even; saturated to [-32768, 32767], so +-Inf saturate; NaN gives 0.  No tolerance anywhere.  Returns the smallest produced[k], -1 on
 * error; ticks == 0 returns 0.
 * Two routes, chosen before anything is enqueued (csrc/sg_stream_host.hpp, block_plan_multi_i16).  FUSED needs all of: count >= 2; every bank the same
 * half window n and the same SAVGOL_STREAMBANK_FMA flag; n <= 8 (both bank kinds, two and three outputs per launch); streams % 128 == 0; the samples,
 * every output and every ring 16-byte aligned; more than 64 ticks; every bank's twin takes its tap-by-tap LDS-DMA tiles.  Then the first 64 ticks are
 * widened once into fp32 scratch and go, bank after bank, through the bank's own fp32 tiles on its own ring and are converted out (the twin's own
 * head); the rest of the block goes through one launch that reads each int16 row once and feeds every output (two or three outputs: one launch; four:
 * two launches of two; csrc/sg_stream_dma_multi_i16.hip); every ring takes its newest samples.  Every other call is `count` single
 * savgol_streambank_push_block_i16 calls in the caller's order.  A fused call makes launches plus ONE stream-ordered allocation / free pair from the
 * library's pool, like the single int16 call: capturable after one warm-up call.
 * Returns -1 with a text naming the call, before any launch or scratch allocation, every bank untouched; checked in this order: NULL banks / d_outs /
 * d_samples; count outside 1..4; a NULL banks[k] or d_outs[k]; an out_type other than SAVGOL_HIP_I16 / SAVGOL_HIP_F32 (named); a bank listed twice; a
 * bank with another `streams` than banks[0]; a bank on another device or with the tick service running; more than 2^30 ticks; d_outs[k] sharing a
 * byte with the samples or with an earlier d_outs[j] (compared byte-wise, each buffer with its own element size).
 * _route enqueues nothing and changes nothing: -1 on the refusals above, else the number of fused launches the call would make (0: the call is
 * `count` single int16 block pushes).
 * Not served here: what savgol_streambank_push_block_i16 does not serve (uint16 samples, a gain or offset, int16 -> fp16 / bf16 outputs). */
int    savgol_streambank_push_block_multi_i16(SavgolStreamBank *const *banks, int count, const int16_t *d_samples, size_t ticks,
                                              void *const *d_outs, int out_type, int *produced, void *stream);
int    savgol_streambank_push_block_multi_i16_route(SavgolStreamBank *const *banks, int count, const int16_t *d_samples, size_t ticks,
                                                    void *const *d_outs, int out_type);
/* trailing / leading edge rows, up to n of them; -1 on bad arguments, 0 if never filled       */
int    savgol_streambank_flush(SavgolStreamBank *bank, float *d_out, int max_rows, void *stream);
int    savgol_streambank_flush_leading(SavgolStreamBank *bank, float *d_out, int max_rows, void *stream);
bool   savgol_streambank_ready(const SavgolStreamBank *bank);
size_t savgol_streambank_latency(const SavgolStreamBank *bank);
size_t savgol_streambank_streams(const SavgolStreamBank *bank);
size_t savgol_streambank_samples_received(const SavgolStreamBank *bank);   /* per stream */
size_t savgol_streambank_samples_output(const SavgolStreamBank *bank);     /* per stream */
/* Resident tick service: ONE kernel stays on the device (one wave per 256 streams, accumulators in registers) and every tick
 * is a doorbell write + a spin on a completion array instead of a launch + a synchronise (csrc/sg_stream_service.hip).
 * service_tick is SYNCHRONOUS: it returns 1 when d_out[0..streams) holds this tick's centre outputs (complete in device
 * memory), 0 while the windows are still filling (d_out untouched), -1 on error; results are bit-identical to
 * savgol_streambank_push / the reference's savgol_stream_push.  Needs streams % 4 == 0, streams <= 262144, 16-byte aligned
 * d_samples / d_out.  While the service runs, the other savgol_streambank_* calls on this bank return -1 (stop first; the
 * ring, write position and counters carry over in both directions).  The kernel leaves by itself after idle_ms (0 = 1000)
 * without a tick and is restarted by the next one; until then a DEVICE-wide synchronise waits for it -- synchronise
 * streams, or stop the service.                                                                                     */
int    savgol_streambank_service_start(SavgolStreamBank *bank, unsigned idle_ms);
int    savgol_streambank_service_tick(SavgolStreamBank *bank, const float *d_samples, float *d_out);
int    savgol_streambank_service_stop(SavgolStreamBank *bank);
int    savgol_streambank_service_running(const SavgolStreamBank *bank);
/* checkpoint / resume: the whole state as one blob (synchronous) */
size_t savgol_streambank_state_bytes(const SavgolStreamBank *bank);
int    savgol_streambank_save(const SavgolStreamBank *bank, void *host_blob, void *stream);
int    savgol_streambank_load(SavgolStreamBank *bank, const void *host_blob, void *stream);

/* ---------------------------------------------------------------- 2-D batch ----------- *
 * `images` frames, image k at base + k*image_pitch (elements), row pitch in elements.
 * Arithmetic of savgol2d_apply / savgol2d_apply_valid (src/savgol2d.c:356-456).
 * method: 0 = auto, 1 = direct dense window (bit-identical to the reference), 2 = exact low-rank
 * separable passes (rolling-window kernel for every half window: one launch holds 4 terms to n = 8, 3 to n = 12, 2 to
 * n = 16; kernels with more -- orders 4 to 6 on wide windows -- take two launches, the second adding to the output frame,
 * which therefore must not overlap the input), 3 = the separable tile kernel for any half window (diagnostic).
 * Rectangular windows (half_window_x != half_window_y): methods 0 / 2 run the rolling kernel of the LARGER half window on
 * factors zero-padded to it (same results to fp32 rounding).  Caveat of the padding: a zero tap times a non-finite sample is NaN, so in
 * this method NaN / Inf input spreads over the padded (square) window instead of the rectangular one; method 1 does not.
 * NaN / Inf.  A non-finite input pixel makes non-finite exactly the outputs whose window, after the border remap, contains it (the reference's dense loop skips
 * no tap: src/savgol2d.c:374-393), and nothing else; a NaN makes them NaN.  Method 1 has the reference's NaN / +Inf / -Inf at the reference's positions;
 * the separable methods (0, 2, 3) may give NaN where the reference gives +-Inf (two terms can meet as Inf - Inf).  The one exception is the caveat above:
 * a rectangular window on methods 0 / 2 spreads a special over the square window of its larger half.  The derivative calls and savgol2d_apply_batch_h16
 * below keep the same rule (the 16-bit call on the frames widened to fp32).
 * The input and output frame stacks must not share a byte (no 2-D kernel can run in place: every output reads its neighbours'
 * inputs): an overlapping call returns -1 with "overlap" in savgol_hip_last_error(); the derivative calls below alike.        */
int savgol2d_apply_batch_f32(const Savgol2DFilter *filter,
                             const float *d_in, int rows, int cols, int in_stride, size_t in_image_pitch,
                             float *d_out, int out_stride, size_t out_image_pitch,
                             size_t images, Savgol2DBoundary boundary, int method, void *stream);

/* The 2-D batch call on 16-bit STORAGE: fp16 or bf16 frames in, the same type or fp32 out, fp32 arithmetic inside -- 4 bytes per pixel (16 -> 16 bit)
 * or 6 (16 bit -> fp32) instead of the fp32 call's 8, and no widened copy of the frames on the caller's side.
 * in_type / out_type: SAVGOL_HIP_F16 / _BF16, out_type also SAVGOL_HIP_F32; served pairs are savgol_apply_batch_h16's (f16 -> f16, bf16 -> bf16,
 * f16 -> f32, bf16 -> f32).  Strides and image pitches count elements of their own buffer's type.
 * CONTRACT.  The twin is savgol2d_apply_batch_f32 with the same filter, boundary and method on the frames widened exactly to fp32, in buffers with
 * 16-byte aligned bases, stride = cols rounded up to a multiple of 4 (input and output alike) and image pitch rows x stride.  Every output pixel
 * equals the twin's pixel bit for bit, rounded ONCE to nearest even into out_type (out_type f32: the twin's pixel itself; NaN positions coincide,
 * NaN payloads are free; overflow into fp16 gives +-Inf; a non-finite input pixel reaches what it reaches in the twin: savgol2d_apply_batch_f32's NaN / Inf
 * rule).  Pixels the twin does not write are not written: the VALID border, and every byte between
 * cols and the stride and between frames.  None of this depends on the alignment of the caller's buffers.  (The twin's alignment is part of the
 * contract because the fp32 call's additive form re-seeds its rolling column sums at a tile's first row on its tile form and at multiples of U frame
 * rows on its strip walk, which unaligned fp32 buffers take: the two are not the same bits.)
 * method: 0, 2 and 3 mean what they mean for the twin.  Method 1 (the dense kernel, whose point is the reference's bits) returns -1: the reference
 * has no 16-bit form to be identical to -- as savgol_apply_batch_h16 refuses SAVGOL_BATCH_REFERENCE_SUMMATION.
 * Two routes, chosen by one host rule before anything is enqueued (csrc/sg_2d_h16_host.hpp, frame_plan_h16).  TILES -- the twin launches the rolling
 * kernel's additive tile form (every smoothing filter of order <= 3 on a square window, half windows 1..16; a rectangular window runs on zero-padded
 * factors, which are not the additive form, and is staged; not an x-dominant derivative filter,
 * method 0 or 2), cols % 4 == 0 and cols >= 32, every base, stride and pitch keeps quads naturally aligned (16-bit side: 8-byte base, stride and pitch
 * multiples of 4; fp32 output: 16-byte base), rows x out_stride x element size and the twin's rows x cols x 4 are under 0x7fffff00, and neither
 * SAVGOL_HIP_ROLL_TILE nor SAVGOL_HIP_2D_H16_TILES is 0: the same tiles reading 16-bit rows and storing out_type rows (csrc/sg_2d_roll_st16.inc).
 * STAGED -- every other call runs the twin itself: whole frames (max(1, 2^24 / (rows x stride)) per piece: 64 MiB per side of stream-ordered
 * scratch unless one frame alone is larger) are widened into aligned fp32 scratch, filtered scratch to scratch and the pixels the twin wrote
 * rounded out.  Pieces of whole frames do not change bits.
 * SAVGOL_HIP_2D_H16_TILES is read with getenv at every call (SAVGOL_HIP_ROLL_TILE once per process): a process that rewrites its environment
 * while other threads are inside the call races with getenv, as with any environment variable; set it before the threads start.
 * Returns -1 with a text naming the call, before any launch or scratch allocation; the checks run in this order and the first fault wins:
 *   1. method 1, or a method outside 0..3;   2. an unserved type pair (named);   3. a NULL pointer;   4. an invalid filter struct;
 *   5. the geometry savgol2d_apply_batch_f32 refuses, with its texts (bad image geometry, image smaller than the window);
 *   6. input and output stacks that share a byte (compared byte-wise: the element sizes may differ).
 * One refusal is the twin's own and comes later, on the staged route after its scratch has been allocated and the widen pass enqueued (the scratch is
 * freed in stream order, d_out is untouched): method 2 or 3 on a filter for which the fp32 call has no separable kernel ("no separable kernel ...").
 * images == 0 returns 0.  Like its siblings it only enqueues (after one warm-up call with the same filter), so it can be captured into a graph.
 * Not served in 16 bit: the derivative-frame calls below (a Savgol2DFilter created with deriv_x / deriv_y goes through this call like any other
 * filter), the row-band calls, uint16 pixels (int16 pixels: savgol2d_apply_batch_i16 below; this call keeps refusing SAVGOL_HIP_I16), fp32 -> 16-bit pairs. */
int savgol2d_apply_batch_h16(const Savgol2DFilter *filter,
                             const void *d_in, int in_type, int rows, int cols, int in_stride, size_t in_image_pitch,
                             void *d_out, int out_type, int out_stride, size_t out_image_pitch,
                             size_t images, Savgol2DBoundary boundary, int method, void *stream);
/* Which route the call above would take for these arguments, decided by the same code and touching no device: 1 = TILES, 0 = STAGED (or no images),
 * -1 = the call would be refused before any launch (same order, same texts). */
int savgol2d_apply_batch_h16_route(const Savgol2DFilter *filter,
                                   const void *d_in, int in_type, int rows, int cols, int in_stride, size_t in_image_pitch,
                                   const void *d_out, int out_type, int out_stride, size_t out_image_pitch,
                                   size_t images, Savgol2DBoundary boundary, int method);

/* The 2-D batch call on INT16 STORAGE: int16 frames in (detector and camera frames, CT slices, depth and SAR rasters), int16 or fp32 out, fp32
 * arithmetic inside -- 4 bytes per pixel (int16 -> int16) or 6 (int16 -> fp32) instead of the 12-20 that widening, filtering and converting on the
 * caller's side keep resident.  out_type: SAVGOL_HIP_I16 or SAVGOL_HIP_F32.  Strides and image pitches count elements of their own buffer's type.
 * CONTRACT (savgol2d_apply_batch_h16's).  The twin is savgol2d_apply_batch_f32 with the same filter, boundary and method on the frames widened exactly to
 * fp32, in buffers with 16-byte aligned bases, stride = cols rounded up to a multiple of 4 (input and output alike) and image pitch rows x stride.
 * An fp32 output pixel is the twin's pixel bit for bit.  An int16 output pixel is the twin's pixel converted ONCE by the rule of the other int16 calls
 * (csrc/sg_i16.hpp): round to nearest, ties to even; saturate to [-32768, 32767]; NaN -> 0 (stated for uniformity: an int16 frame holds no NaN or Inf,
 * so a NaN is reachable only through a filter whose scale overflows).  Pixels the twin does not write are not written: the VALID border, and every byte
 * between cols and the stride and between frames.  None of this depends on the alignment of the caller's buffers.
 * method: 0, 2 and 3 mean what they mean for the twin.  Method 1 returns -1: the reference has no int16 form to be identical to.
 * Two routes, chosen by one host rule before anything is enqueued -- the 16-bit call's rule unchanged (csrc/sg_2d_h16_host.hpp, frame_plan_h16: the
 * element sizes are the same).  TILES -- the twin launches the rolling kernel's additive tile form (a smoothing filter of order <= 3 on a square window,
 * half windows 1..16; not an x-dominant filter; method 0 or 2), cols % 4 == 0 and cols >= 32, quads are naturally aligned (int16 side: 8-byte base,
 * stride and pitch multiples of 4; fp32 output: 16-byte base), rows x out_stride x element size and the twin's rows x cols x 4 are under 0x7fffff00,
 * and neither SAVGOL_HIP_ROLL_TILE nor SAVGOL_HIP_2D_I16_TILES is 0: sg2d_rolling_i16_kernel (csrc/sg_2d_roll_st16.inc), the same tiles reading int16 rows
 * and storing out_type rows, the storage types fixed when the kernel is compiled.  STAGED -- every other call (the general, two-output,
 * horizontal-first and accumulating tile forms included) runs the twin itself: whole frames in the 16-bit call's pieces are widened into aligned fp32
 * scratch (sg2d_i16_widen_kernel), filtered scratch to scratch, and the pixels the twin wrote converted out (sg2d_i16_convert_kernel).  Pieces of whole
 * frames do not change bits.  SAVGOL_HIP_2D_I16_TILES is read with getenv at every call (SAVGOL_HIP_ROLL_TILE once per process); set it before
 * threads start.
 * Returns -1 with a text naming savgol2d_apply_batch_i16, before any launch or scratch allocation; the checks run in this order and the first fault wins:
 *   1. method 1, or a method outside 0..3;   2. an out_type other than SAVGOL_HIP_I16 / SAVGOL_HIP_F32 (named);   3. a NULL pointer;
 *   4. an invalid filter struct;   5. the geometry savgol2d_apply_batch_f32 refuses, with its texts;
 *   6. input and output stacks that share a byte (compared byte-wise: element sizes 2 and 2 or 4; d_in == d_out is an overlap).
 * The twin's own late refusal is kept as the 16-bit call has it: "no separable kernel ..." on the staged route with method 2 or 3 (d_out untouched).
 * images == 0 returns 0.  Like its siblings it only enqueues (after one warm-up call with the same filter), so it can be captured into a graph.
 * Not served: uint16 pixels (12- and 14-bit unsigned data, everything below 32768, can be passed as int16 as it is); a gain or offset per call;
 * int16 -> fp16 / bf16 pairs; the Hessian, Laplacian and row-band calls (the gradient on int16 frames: savgol2d_gradient_batch_i16 below); in place; the
 * general, two-output, horizontal-first and accumulating tile forms on int16 rows through THIS call (they take the staged route); bench.py (the flagship workload stays fp32).  savgol2d_apply_batch_h16 keeps refusing SAVGOL_HIP_I16. */
int savgol2d_apply_batch_i16(const Savgol2DFilter *filter,
                             const int16_t *d_in, int rows, int cols, int in_stride, size_t in_image_pitch,
                             void *d_out, int out_type, int out_stride, size_t out_image_pitch,
                             size_t images, Savgol2DBoundary boundary, int method, void *stream);
/* Which route the call above would take for these arguments, decided by the same code and touching no device: 1 = TILES, 0 = STAGED (or no images),
 * -1 = the call would be refused before any launch (same order, same texts). */
int savgol2d_apply_batch_i16_route(const Savgol2DFilter *filter,
                                   const int16_t *d_in, int rows, int cols, int in_stride, size_t in_image_pitch,
                                   const void *d_out, int out_type, int out_stride, size_t out_image_pitch,
                                   size_t images, Savgol2DBoundary boundary, int method);

/* The GRADIENT on INT16 STORAGE: int16 frames in, gx = d/dx and gy = d/dy out as int16 or fp32 frames (out_type: SAVGOL_HIP_I16 or SAVGOL_HIP_F32, both
 * frames the same type), fp32 arithmetic inside, no fp32 copy of the stack on the caller's side.  Strides and image pitches count elements of their own
 * buffer; the two outputs share out_stride and out_image_pitch.  Either output pointer may be NULL: that frame is not computed.  With both NULL the call
 * returns 0 and looks at nothing else, as savgol2d_gradient_batch_f32 does.
 * CONTRACT (savgol2d_apply_batch_i16's).  The twin is savgol2d_gradient_batch_f32 (declared below) with the same half windows, order, deltas and boundary
 * on the frames widened exactly to fp32, in buffers with 16-byte aligned bases, stride = cols rounded up to a multiple of 4 and image pitch rows x stride.
 * An fp32 output pixel is the twin's pixel bit for bit.  An int16 output pixel is the twin's pixel converted ONCE by csrc/sg_i16.hpp's rule: round to
 * nearest, ties to even; saturate to [-32768, 32767]; NaN -> 0 (reachable only through deltas whose scale overflows).  Pixels the twin does not write are
 * not written: the VALID border, every byte between cols and the stride and between frames.  None of this depends on the alignment of the caller's buffers.
 * Two routes, chosen by one host rule before anything is enqueued (csrc/sg_2d_grad16_host.hpp, grad_plan_i16).  DIRECT, for both requested frames, needs all
 * of: a square window with 1 <= n <= 7; every requested frame's separable factors have one or two terms of definite parity (poly_order <= 4 in practice;
 * the rule asks the factors), gx's two x factors of one parity; cols % 4 == 0 and cols >= 32; the int16 sides on 8-byte bases with stride and pitch
 * multiples of 4, an fp32 output on a 16-byte base; rows x out_stride x element size and the twin's rows x cols x 4 under 0x7fffff00 (frame_plan_h16's
 * layout conditions, asked of frame_plan_h16); neither SAVGOL_HIP_ROLL_TILE nor SAVGOL_HIP_2D_GRAD_I16_DIRECT is 0.  Then the twin itself runs the
 * horizontal-first kernel for gx and the general 20-row tile for gy, and this call runs the same two on int16 rows: sg2d_rolling_hf_i16_kernel
 * (csrc/sg_2d_hf.hip) and sg2d_rolling_gen_i16_kernel (csrc/sg_2d_roll_st16.inc), gx first, with the twin's taps and term sums.  STAGED -- every other call
 * (half windows above 7, rectangular windows, order >= 5, odd layouts) runs the twin itself: whole frames in pieces (three fp32 sides within 128 MiB:
 * grad_stage_i16) are widened ONCE into aligned fp32 scratch (sg2d_i16_widen_kernel), savgol2d_gradient_batch_f32's own path runs scratch to scratch for
 * the requested frames, and each is converted out (sg2d_i16_convert_kernel); one stream-ordered allocate / free pair per call.  Pieces of whole frames do
 * not change bits.  SAVGOL_HIP_2D_GRAD_I16_DIRECT is read with getenv at every call (SAVGOL_HIP_ROLL_TILE once per process); set it before threads start.
 * Returns -1 with a text naming savgol2d_gradient_batch_i16, before any launch or scratch allocation; the checks run in this order and the first fault wins:
 *   1. an out_type other than SAVGOL_HIP_I16 / SAVGOL_HIP_F32 (named);   2. a NULL d_in;
 *   3. the configuration and the geometry savgol2d_gradient_batch_f32 refuses, with its texts (invalid configuration, bad image geometry, image smaller
 *      than the window);
 *   4. stacks that share a byte (compared byte-wise: element sizes 2 and 2 or 4): the input against each output, then the two outputs against each other.
 * images == 0 returns 0 once 1-3 have passed.  Like its siblings it only enqueues (after one warm-up call with the same arguments), so it can be captured
 * into a graph.
 * Not served: Hessian and Laplacian on int16; fp16 / bf16 frames; half windows above 7, rectangular windows and order >= 5 on the direct route (they are
 * staged); accumulating passes with 16-bit outputs; a one-read gradient (each frame reads the input once); mixed output types; uint16 pixels; in place;
 * bench.py.  The route and bits of savgol2d_apply_batch_i16 are unchanged. */
int savgol2d_gradient_batch_i16(int half_win_x, int half_win_y, int poly_order,
                                const int16_t *d_in, int rows, int cols, int in_stride, size_t in_image_pitch,
                                void *d_grad_x, void *d_grad_y, int out_type, int out_stride, size_t out_image_pitch,
                                size_t images, float delta_x, float delta_y, Savgol2DBoundary boundary, void *stream);
/* Which route the call above would take for these arguments, decided by the same code and touching no device: 1 = DIRECT, 0 = STAGED (or nothing to do:
 * no images, both outputs NULL), -1 = the call would be refused before any launch (same order, same texts). */
int savgol2d_gradient_batch_i16_route(int half_win_x, int half_win_y, int poly_order,
                                      const int16_t *d_in, int rows, int cols, int in_stride, size_t in_image_pitch,
                                      const void *d_grad_x, const void *d_grad_y, int out_type, int out_stride, size_t out_image_pitch,
                                      size_t images, float delta_x, float delta_y, Savgol2DBoundary boundary);

/* Derivative frames (arithmetic of savgol2d_gradient / _hessian / _laplacian, src/savgol2d.c:462-618).  The Laplacian
 * writes one frame, with no temporary frame and no add pass.  Outputs may be NULL (skipped), like the reference.
 * Square windows use the separable kernels (fp32 rounding only vs the reference), one frame after the other: frames
 * whose x derivative is the higher (gradient x, Hessian xx) run the horizontal pass first; the Hessian's xy and yy share
 * one rolling-window launch where they have as many terms; the Laplacian is one frame of the summed kernel
 * scale_xx*Wxx + scale_yy*Wyy.  Other window
 * shapes: one pass per output as savgol2d_apply_batch_f32 method 0 runs it; the Laplacian computes both dense sums from
 * one read of each input tile and adds them as the reference adds its two frames (bit-identical).  See DESIGN.md.
 * NaN / Inf: the rule of savgol2d_apply_batch_f32, every frame under its own (deriv_x, deriv_y) filter; the Laplacian's xx and yy share one window.    */
int savgol2d_gradient_batch_f32(int half_win_x, int half_win_y, int poly_order,
                                const float *d_in, int rows, int cols, int in_stride, size_t in_image_pitch,
                                float *d_grad_x, float *d_grad_y, int out_stride, size_t out_image_pitch,
                                size_t images, float delta_x, float delta_y, Savgol2DBoundary boundary, void *stream);
int savgol2d_hessian_batch_f32(int half_win_x, int half_win_y, int poly_order,
                               const float *d_in, int rows, int cols, int in_stride, size_t in_image_pitch,
                               float *d_xx, float *d_xy, float *d_yy, int out_stride, size_t out_image_pitch,
                               size_t images, float delta_x, float delta_y, Savgol2DBoundary boundary, void *stream);
int savgol2d_laplacian_batch_f32(int half_win_x, int half_win_y, int poly_order,
                                 const float *d_in, int rows, int cols, int in_stride, size_t in_image_pitch,
                                 float *d_out, int out_stride, size_t out_image_pitch,
                                 size_t images, float delta_x, float delta_y, Savgol2DBoundary boundary, void *stream);

/* ---------------------------------------------------------------- 2-D row bands (multi-GPU) --- *
 * Frames too large for one GPU, or fewer frames than GPUs: every rank owns a horizontal band of rows of every frame and needs
 * the half_window_y rows next to its band from the ranks above and below -- the only exchange step on the hot path (the
 * reference filters whole frames: src/savgol2d.c:398-456; a band's rows must be the rows that call would have produced).
 * savgol2d_rowband_plan: rank's rows [*row_lo, *row_hi) of a `rows`-row frame (savgol_hip_shard_range) and how many halo rows it
 *   needs from above / below (half_window_y, or 0 at the frame's real top / bottom).  -1 when the bands would be thinner than
 *   2 x half_window_y.
 * savgol2d_apply_rowband_f32: filters one band, d_band = its band_rows x cols rows per image.  d_halo_up / d_halo_down: the
 *   half_window_y rows just above / below the band (row 0 = the farthest-up row; halo_stride elements between rows,
 *   halo_image_pitch between images), NULL where the band ends at the frame's real edge -- the boundary mode applies there
 *   exactly as in savgol2d_apply_batch_f32.  All band_rows output rows are written (VALID: not the frame's own first / last
 *   half_window_y rows, not the half_window_x border columns).  Enqueue-only plus a stream-ordered scratch allocation; the
 *   FIRST launch (the band itself) does not read the halos.  Method 1 gives the whole-frame call's bits; method 2 its bits for
 *   kernels of order > 3 or derivative kernels, and fp32 rounding (<= 2.5e-7 of the input's maximum) for the additive smoothing
 *   kernels, whose rolling column sums are re-seeded on a phase tied to the frame's row 0.
 * The halo buffers are the caller's to fill: a device-to-device copy on one GPU, ncclSend / ncclRecv across GPUs --
 * savgol2d_rowband_exchange_rccl in the optional lib/libsavgol_hip_rccl.so (csrc/sg_rowband_rccl.cpp; comm = an ncclComm_t,
 * d_send_scratch = 2 * images * half_window_y * cols floats, halos received with halo_stride = cols and halo_image_pitch =
 * half_window_y * cols; one message per neighbour and direction for the whole stack).                                   */
int savgol2d_rowband_plan(int rows, int half_win_y, int rank, int world_size, int *row_lo, int *row_hi, int *halo_up, int *halo_down);
int savgol2d_apply_rowband_f32(const Savgol2DFilter *filter,
                               const float *d_band, int band_rows, int cols, int in_stride, size_t in_image_pitch,
                               const float *d_halo_up, const float *d_halo_down, int halo_stride, size_t halo_image_pitch,
                               float *d_out, int out_stride, size_t out_image_pitch,
                               size_t images, Savgol2DBoundary boundary, int method, void *stream);
/* Step (2) of the call above on its own -- the half_window_y output rows next to each artificial edge -- for callers that overlap
 * the halo exchange with the band: enqueue savgol2d_apply_batch_f32 on the band (it reads no halo) while the exchange runs on
 * another stream, make the compute stream wait for the exchange, then call this.  Same arguments, same result as the one call. */
int savgol2d_apply_rowband_edges_f32(const Savgol2DFilter *filter,
                                     const float *d_band, int band_rows, int cols, int in_stride, size_t in_image_pitch,
                                     const float *d_halo_up, const float *d_halo_down, int halo_stride, size_t halo_image_pitch,
                                     float *d_out, int out_stride, size_t out_image_pitch,
                                     size_t images, Savgol2DBoundary boundary, int method, void *stream);
/* The same on two streams (round 6): the strips are gathered and filtered on `halo_stream` -- the stream the halos arrive on; call this after
 * enqueueing the exchange there.  They read the band and the halos and write library scratch only, so they run BESIDE the band launch still
 * going on `stream`; only the copy of the finished half_window_y rows per edge into d_out is ordered behind everything enqueued on `stream`
 * so far (the band launch), through an event the call records itself.  No wait between the two streams is needed from the caller.
 * halo_stream == stream is savgol2d_apply_rowband_edges_f32. */
int savgol2d_apply_rowband_edges_streams_f32(const Savgol2DFilter *filter,
                                             const float *d_band, int band_rows, int cols, int in_stride, size_t in_image_pitch,
                                             const float *d_halo_up, const float *d_halo_down, int halo_stride, size_t halo_image_pitch,
                                             float *d_out, int out_stride, size_t out_image_pitch,
                                             size_t images, Savgol2DBoundary boundary, int method, void *halo_stream, void *stream);
/* (savgol2d_rowband_exchange_rccl is declared in savgol_hip_rccl.h -- that library is the only part that links librccl) */

/* ---------------------------------------------------------------- bench utilities ----- *
 * Synthetic workload of SURVEY.md section 8(d), generated in HBM (never crosses PCIe):
 * x[c][i] = sin(2 pi f_c i) + 0.5 sin(2 pi 7.3 f_c i + phi_c) + 0.1 u(c,i).                  */
int savgol_hip_synth_f32(float *d_dst, size_t channel0, size_t channels, size_t length, size_t ld,
                         uint64_t seed, void *stream);
int savgol_hip_synth_f64(double *d_dst, size_t channel0, size_t channels, size_t length, size_t ld,
                         uint64_t seed, void *stream);

/* What the memory system gives a plain stream of the same buffers, for the bench line's roofline.copy_frac / read_only_frac (SURVEY.md 8d:
 * "a device copy timed in the same harness"): one 16-byte nontemporal vector per thread.  bytes and both addresses multiples of 16.
 * _read stores nothing (d_sink4 may be NULL; 4 bytes that are never written in practice).  Enqueue only.  0 / -1. */
int savgol_hip_stream_copy(const void *d_in, void *d_out, size_t bytes, void *stream);
int savgol_hip_stream_read(const void *d_in, size_t bytes, void *d_sink4, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* SAVGOL_HIP_H */
