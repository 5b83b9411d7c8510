/* thzgpu.h — C ABI of libthzgpu.so, the MI355X (gfx950) engine for the
 * data_thread recompute path of unibe-icelab/thz-image-explorer.
 *
 * This is the drop-in boundary: plain pointers and sizes, no
 * C++/torch types.  Each entry point names the reference interface it
 * replaces (paths relative to the reference checkout).  A Rust maintainer
 * binds these with an `extern "C"` block (INTEGRATION.md shows the stub); the
 * tests bind them with ctypes; the C++ host mirror (thz_image_explorer_amd/host)
 * sits on top of them.
 *
 * Conventions
 *  - One context per process per GPU; calls on one context are made from one
 *    thread at a time (the reference's single data thread, data_thread.rs:162).
 *  - Every function returns THZ_OK (0) or a negative thz_status; it never
 *    throws or aborts.  thz_last_error() gives the text.  On error device
 *    buffers named as outputs are unspecified but inputs are untouched, so a
 *    caller can do what the reference does on failure: keep `input.clone()`.
 *  - Pointers named d_* are DEVICE pointers (from thz_malloc or any other HIP
 *    allocation on the context's device); all others are host pointers.
 *  - Layout is the reference's: cubes are C-order (x, y, t|f) with the last
 *    axis contiguous (data_container.rs:136-151); complex = interleaved
 *    {re, im} f32 (num_complex::Complex32).  `npix` = nx*ny traces.
 *  - Kernels are enqueued on the context's stream; thz_sync() / any D2H copy
 *    waits for them.
 */
#ifndef THZGPU_H
#define THZGPU_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define THZGPU_ABI_VERSION 2

typedef struct thz_ctx thz_ctx;

typedef enum thz_status {
    THZ_OK = 0,
    THZ_ERR_INVALID = -1,      /* bad argument / shape */
    THZ_ERR_UNSUPPORTED = -2,  /* transform length not supported */
    THZ_ERR_HIP = -3,          /* HIP runtime failure (no GPU, OOM, fault) */
    THZ_ERR_NOT_READY = -4,    /* geometry / cube not set */
    THZ_ERR_ABORTED = -5,      /* abort flag observed between kernel batches */
    THZ_SKIPPED = 1            /* not an error: a guard of the reference applied, output = input */
} thz_status;

/* FftWindowType, math_tools.rs:35-46 (same order) */
typedef enum thz_window_type {
    THZ_WIN_ADAPTED_BLACKMAN = 0,
    THZ_WIN_BLACKMAN = 1,
    THZ_WIN_HANNING = 2,
    THZ_WIN_HAMMING = 3,
    THZ_WIN_FLAT_TOP = 4
} thz_window_type;

/* ConfigContainer.fft_window / fft_window_type, config.rs:171-213 */
typedef struct thz_window_cfg {
    int32_t type;   /* thz_window_type */
    float lower;    /* fft_window[0], ps; default 1.0 */
    float upper;    /* fft_window[1], ps; default 7.0 */
} thz_window_cfg;

/* ------------------------------------------------------------------ */
/* lifecycle                                                           */
/* ------------------------------------------------------------------ */

/* Creates a context on HIP device `device`.  Fails with THZ_ERR_HIP when no
 * GPU is present — there is no CPU fallback. */
int thz_create(int device, thz_ctx **out);
void thz_destroy(thz_ctx *ctx);
/* Frees the device scratch the context keeps between calls (the pixel-sum workspace, the blocks of the last
 * thz_deconvolve — see there); the next call that needs them allocates again.  Waits for the context's stream.
 * Not in the reference (its buffers die with each filter call): a host under memory pressure calls this after a
 * Deconvolution, the way it would drop a cache. */
int thz_release_scratch(thz_ctx *ctx);
const char *thz_last_error(const thz_ctx *ctx);
int thz_abi_version(void);
/* hipStream_t of the context as an opaque pointer (for callers that want to
 * order their own HIP work, e.g. torch.cuda.ExternalStream). */
void *thz_stream(thz_ctx *ctx);
int thz_sync(thz_ctx *ctx);

/* device memory helpers so that a non-HIP caller can own buffers */
int thz_malloc(thz_ctx *ctx, void **d_ptr, size_t bytes);
int thz_free(thz_ctx *ctx, void *d_ptr);
int thz_memcpy_h2d(thz_ctx *ctx, void *d_dst, const void *src, size_t bytes);
int thz_memcpy_d2h(thz_ctx *ctx, void *dst, const void *d_src, size_t bytes);
int thz_memcpy_d2d(thz_ctx *ctx, void *d_dst, const void *d_src, size_t bytes);
int thz_memset(thz_ctx *ctx, void *d_dst, int value, size_t bytes);

/* ------------------------------------------------------------------ */
/* geometry / plan                                                     */
/* ------------------------------------------------------------------ */

/* Sets trace length and time axis; builds the transform tables ("plans").
 * Replaces RealFftPlanner::plan_fft_forward/inverse + the frequency-axis rule
 * at io.rs:614-621, data_thread.rs:1194-1207, tilt_compensation.rs:206-217:
 * frequency[i] = i / (time[nt-1] - time[0]), i = 0..nt/2.
 * Supported nt: any length 2..65536, as realfft plans any length.  Lengths whose transform buffers do not fit a
 * CU's LDS — not a power of two above 8191 (4096 with thz_set_kernel_family(1)), powers of two above 16384 — run
 * with those buffers in global scratch (up to 1 GiB, allocated here): correct, two orders of magnitude slower per
 * sample than the lengths with a kernel of their own. */
int thz_set_time_axis(thz_ctx *ctx, const float *time, size_t nt);
/* Kernel family selection: 0 = automatic (register-resident three-pass "F"
 * kernels for nt = 1024/2048/4096; mixed-radix "P" kernels for the lengths that
 * factor into three small radices — nt = 1001 = 7 x 11 x 13, the length of the
 * reference's real scans, and 1000 / 1200 / 1500 / 2000; half-length mixed-radix "PH" kernels for
 * 2002 / 2400 / 3000 / 4000 (twice a P length); chirp-z over the mixed-radix core — "FBP"
 * kernels, convolution length 2304 / 2560 — for the other lengths in 1025 ... 1280, where a tilted
 * 1001-sample scan lands; chirp-z over the F core — "FB" kernels —
 * for the remaining lengths that are not a power of two; LDS Stockham "G" kernels
 * for the remaining powers of two), 1 = G kernels (Stockham / Bluestein in LDS)
 * for every length, 2 = automatic without the P, PH and FBP kernels (A/B measurements, tests).
 * Re-plans if a time axis is already set. */
int thz_set_kernel_family(thz_ctx *ctx, int family);
size_t thz_nt(const thz_ctx *ctx);
size_t thz_nf(const thz_ctx *ctx);
int thz_get_frequency(const thz_ctx *ctx, float *frequency /* nf */);

/* ------------------------------------------------------------------ */
/* host-side multiplier vectors (O(nt) work, no GPU involved)          */
/* ------------------------------------------------------------------ */
/* The reference re-evaluates its window formulas for every trace inside the
 * pixel loops; they only depend on the axis, so the engine evaluates them once
 * per call on the host, in the reference's f32 operation order, and the
 * kernels multiply by the resulting vector.  These need no context. */

/* frequency[i] = i / (time[nt-1] - time[0]), i = 0..nt/2 (io.rs:614-621). */
int thz_host_frequency_axis(const float *time, size_t nt, float *frequency /* nt/2+1 */);

/* Window multiplier of the fft stage, math_tools.rs:102-198, 356-371:
 * out[i] = w(time[i]) such that windowed = data * out. */
int thz_host_fft_window(const float *time, size_t nt, const thz_window_cfg *cfg,
                        float *out /* nt */);

/* apply_adapted_blackman_window on ones (math_tools.rs:102-122) over an
 * arbitrary axis slice; tilt compensation's tail taper is (lower 0, upper 7),
 * tilt_compensation.rs:186-188. */
int thz_host_adapted_blackman(const float *axis, size_t len, float lower, float upper,
                              float *out /* len */);

/* "Time Band Pass" multiplier, band_pass_td_before_fft.rs:124-182 (and
 * _after_fft.rs): 0 outside [lower,upper), adapted-Blackman taper inside.
 * The low / high values are clamped in place exactly as the filter clamps its
 * own fields (:137-138).  lower/upper indices are returned when non-NULL. */
int thz_host_td_bandpass(const float *time, size_t nt, double *low, double *high,
                         double window_width, float *out /* nt */, int64_t *lower,
                         int64_t *upper);

/* "Frequency Band Pass" multiplier, band_pass_fd.rs:135-168 + zero padding
 * :194-212: 0 outside [lower,upper), taper inside. */
int thz_host_fd_bandpass(const float *frequency, size_t nf, double low, double high,
                         double window_width, float *out /* nf */, int64_t *lower,
                         int64_t *upper);

/* Build-defined frequency-domain filters (the reference has neither; it only
 * draws the water lines, gui/center_panel.rs:477-485).  Both
 * produce per-bin multipliers for thz_apply_fd_mask / thz_apply_fd_cmask.
 *   water lines (K14): out[k] = prod_i (1 - exp(-((f_k - line_i)/sigma)^2))
 *   Wiener (K13): out[k] = conj(R[k]) / (|R[k]|^2 + eps_rel * max_j |R[j]|^2),
 *                 R = spectrum of the reference pulse (interleaved, nf bins) */
int thz_host_water_line_mask(const float *frequency, size_t nf, const float *lines_thz,
                             size_t n_lines, float sigma_thz, float *out /* nf */);
int thz_host_wiener_filter(const float *ref_fft, size_t nf, float eps_rel,
                           float *out_cmask /* nf interleaved complex */);

/* TiltCompensation::filter geometry, tilt_compensation.rs:104-175 (K11): the
 * time extension (floor((|cx*tx| + |cy*ty|)/c/0.05)*0.05 with the reference's
 * hard-coded dt = 0.05 ps), the extended time axis (front/back linspaces) and,
 * per pixel, the index at which the tapered trace is inserted.  Returns
 * num_steps; the new length is nt + 2*num_steps.  new_time / insert_index may
 * be NULL (sizing call). */
size_t thz_host_tilt_plan(const float *time, size_t nt, size_t nx, size_t ny, double tilt_x_deg,
                          double tilt_y_deg, float dx, float dy,
                          float *new_time /* nt + 2*num_steps */,
                          int32_t *insert_index /* nx*ny */);

/* ------------------------------------------------------------------ */
/* stage kernels (device pointers)                                     */
/* ------------------------------------------------------------------ */

/* math_tools::fft, math_tools.rs:330-398 (K1+K2+K3), optionally fused with
 * the Frequency Band Pass multiply, band_pass_fd.rs:184-187 (K4).
 *   d_in        (npix, nt) f32
 *   d_win_a/b   (nt) f32 multipliers applied in that order, each may be NULL
 *   d_data_out  (npix, nt) windowed trace (the stage's `data` output), or NULL
 *   d_fft       (npix, nf) complex, or NULL
 *   d_amp       (npix, nf) = |X| (Complex::norm, :384), or NULL
 *   d_phase     (npix, nf) = numpy_unwrap(arg X, 2*pi) (:387-388), or NULL
 *   d_fd_mask   (nf) f32 or NULL: when given, d_fft and d_amp are multiplied
 *               by it (phases are not — band_pass_fd.rs leaves them) */
int thz_fft(thz_ctx *ctx, size_t npix, const float *d_in, const float *d_win_a,
            const float *d_win_b, float *d_data_out, float *d_fft, float *d_amp, float *d_phase,
            const float *d_fd_mask);

/* FrequencyDomainBandPass::filter per-pixel part, band_pass_fd.rs:175-212,
 * in place: fft *= mask, amp *= mask.  Either array may be NULL. */
int thz_apply_fd_mask(thz_ctx *ctx, size_t npix, float *d_fft, float *d_amp, const float *d_mask);

/* Same with a complex per-bin multiplier (interleaved, nf entries): the
 * build-defined reference-pulse (Wiener) deconvolution K13.  Bin 0 and, for
 * even nt, the last bin have their imaginary part forced to 0 so the result
 * stays a valid C2R input (SURVEY a'-4).  amp *= |mask|. */
int thz_apply_fd_cmask(thz_ctx *ctx, size_t npix, float *d_fft, float *d_amp,
                       const float *d_cmask);

/* math_tools::ifft per-pixel part, math_tools.rs:545-568 (K5: C2R then /nt),
 * optionally fused with a time multiplier (K6, band_pass_td_after_fft.rs) and
 * the intensity image (K7, data_thread.rs:1288-1307).
 *   d_fft      (npix, nf) complex
 *   d_td_win   (nt) or NULL
 *   d_data_out (npix, nt)
 *   d_img      (npix) or NULL: sum_t out^2 */
int thz_ifft(thz_ctx *ctx, size_t npix, const float *d_fft, const float *d_td_win,
             float *d_data_out, float *d_img);

/* The avg_in_fourier_space branch of math_tools::ifft (math_tools.rs:442-470) and
 * its per-ROI twin (:496-529): spectrum[k] = from_polar(amp[k], phase[k]) of an
 * AVERAGED amplitude / unwrapped-phase pair, C2R, / nt — one trace, so host
 * vectors in and out (amp, phase: nf; out: nt).  zero_dc_imag: the ROI branch
 * clears Im(spectrum[0]) by hand (:510-512).  The transform ignores the
 * imaginary parts of bin 0 and (even nt) the last bin, as realfft's does. */
int thz_polar_ifft(thz_ctx *ctx, const float *amp, const float *phase, int zero_dc_imag, float *out);

/* Whole default chain for one cube tile in ONE launch (the hot path):
 * raw -> *pre window -> R2C -> amp/phase/unwrap -> *fd mask -> store
 *     -> C2R /nt -> *post window -> store + intensity.
 * d_pre_win is the composition of every time-domain multiplier in front of
 * the transform (tilt taper, Time Band Pass, fft window); d_post_win the Time
 * Band Pass after the inverse.  Output pointers other than d_data_out may be
 * NULL (not materialised). */
int thz_pipeline(thz_ctx *ctx, size_t npix, const float *d_raw, const float *d_pre_win,
                 const float *d_fd_mask, const float *d_post_win, float *d_fft, float *d_amp,
                 float *d_phase, float *d_data_out, float *d_img);

/* The same launch with every optional input and output of the fused chain:
 *   d_fd_cmask  (nf) interleaved complex per-bin multiplier or NULL — the build-defined
 *               reference-pulse (Wiener) filter K13 (thz_host_wiener_filter) inside the
 *               ONE pass over HBM: spectrum = X * (cmask * mask), imaginary parts of bin 0 and (even
 *               nt) of the last bin forced to 0 (math_tools.rs:510-512), amplitudes = |X cmask mask|,
 *               phases those of X (band_pass_fd.rs:184-212 does not touch them either).  Fused for nt = 1024 / 2048 /
 *               4096, 1001 / 1000 / 1200 / 1500 / 2000, 2002 / 2400 / 3000 / 4000 and the chirp-z lengths
 *               1025 ... 1280 (the F, P, PH and FBP kernel families); trace lengths without a fused kernel for it run fft -> thz_apply_fd_cmask ->
 *               ifft internally.
 *   d_sums      (2 nf) or NULL: sum over the npix traces of the stored amplitudes [0, nf) and of the
 *               unwrapped phases [nf, 2 nf) — the numerators of the pixel means of the ifft stage
 *               (math_tools.rs:427-440; divide by nx ny, or all-reduce the sums of the tiles first).  For
 *               nt = 1024 / 2048 / 4096, 1001 / 1000 / 1200 / 1500 / 2000 and 2002 / 2400 / 3000 / 4000 they are taken INSIDE the launch (every block adds its
 *               traces' values to accumulators in LDS, wave by wave in a fixed order; a small pass adds the
 *               blocks' rows), and so for 1025 ... 1280 (FBP kernels: every wave keeps its traces' sums in
 *               registers and leaves one row), for other lengths by thz_pixel_sum passes over d_amp / d_phase
 *               behind it.
 *               Deterministic; the summation order differs from the reference's sequential one (<= 2e-6
 *               relative); thz_pixel_mean is the bit-exact form.
 * d_fft, d_amp, d_phase and d_data_out are required here. */
typedef struct thz_pipeline_io {
    const float *d_raw;      /* (npix, nt) */
    const float *d_pre_win;  /* (nt) or NULL */
    const float *d_fd_mask;  /* (nf) real or NULL */
    const float *d_fd_cmask; /* (nf) complex or NULL */
    const float *d_post_win; /* (nt) or NULL */
    float *d_fft;            /* (npix, nf) complex */
    float *d_amp;            /* (npix, nf) */
    float *d_phase;          /* (npix, nf) */
    float *d_data_out;       /* (npix, nt) */
    float *d_img;            /* (npix) or NULL */
    float *d_sums;           /* (2 nf) or NULL */
    /* Optional: the caller's word that d_fd_mask is ZERO at every bin outside [band_lo, band_hi) — the index range
     * thz_host_fd_bandpass hands back (lower, upper).  0, 0: unknown.  With d_fd_cmask and d_sums at nt = 4096 the fused
     * kernel then stages only the band's bins of the complex multiplier (half the table at the default 0.2-5 THz) and
     * keeps its eighth wave per block; results are the same bit for bit.  A wrong range gives wrong spectra. */
    size_t band_lo, band_hi;
} thz_pipeline_io;
int thz_pipeline_ex(thz_ctx *ctx, size_t npix, const thz_pipeline_io *io);

/* thz_pipeline_ex on traces that are re-laid on the context's (extended) time axis while they are read: the Tilt
 * Compensation's per-pixel copy (thz_tilt_apply) without the extended cube.  Sample n of pixel p is d_src[p][0] in
 * front of the pixel's insert index, d_src[p][n - ins] * d_taper[n - ins] behind it and 0 behind the trace; io->d_raw
 * is ignored, every output is what thz_tilt_apply + thz_pipeline_ex give, bit for bit.  With an FBP plan (the
 * context's nt in 1025 ... 1280) this is ONE launch from the untilted cube — gather, optional complex multiplier and
 * pixel sums included; with any other plan the traces are re-laid into scratch of the context first and the chain
 * runs on that, so the results do not depend on the length.
 *   d_src_sum  (nt) or NULL: sum over the npix traces of the re-laid, tapered samples (before d_pre_win) — with the
 *              pixel count it gives the mean spectrum by linearity, mask * FFT(pre * mean trace).
 * THZ_ERR_INVALID for nt_in == 0 or nt_in > nt.  The insert indices live on the device and are the caller's word:
 * each in [0, nt - 1], as thz_host_tilt_plan makes them (an index outside reads no memory out of bounds, it yields
 * the first sample or zeros). */
typedef struct thz_tilt_src {
    const float *d_src;            /* (npix, nt_in) untilted traces */
    size_t nt_in;
    const float *d_taper;          /* (nt_in) thz_host_adapted_blackman(time, 0, 7) */
    const int32_t *d_insert_index; /* (npix), thz_host_tilt_plan */
    float *d_src_sum;              /* (nt) or NULL */
} thz_tilt_src;
int thz_pipeline_tilted(thz_ctx *ctx, size_t npix, const thz_pipeline_io *io, const thz_tilt_src *src);

/* Time multiplier alone (K6): out = in * win; in place allowed. */
int thz_apply_td_window(thz_ctx *ctx, size_t npix, const float *d_in, const float *d_win,
                        float *d_out);

/* Intensity image (K7), data_thread.rs:1288-1307 / io.rs:588-594. */
int thz_intensity(thz_ctx *ctx, size_t npix, const float *d_data, float *d_img);

/* Load-time preprocessing, io.rs:578-596: per-trace subtract data[x,y,0],
 * then intensity.  In place; d_img may be NULL. */
int thz_subtract_bias(thz_ctx *ctx, size_t npix, float *d_data, float *d_img);

/* Pixel means (K8), math_tools.rs:421-440: mean over x then over y of an
 * (nx, ny, len*ncomp) f32 array -> len*ncomp values.  ncomp = 2 for complex.
 * Also used for avg_data (data_thread.rs:1423-1429).
 * d_out holds *sums* scaled as the reference does: (sum_x / nx) summed over y
 * / ny.  For multi-GPU tiles use thz_pixel_sum and divide after the
 * all-reduce. */
int thz_pixel_mean(thz_ctx *ctx, size_t nx, size_t ny, size_t len, int ncomp, const float *d_arr,
                   float *d_out);
int thz_pixel_sum(thz_ctx *ctx, size_t npix, size_t len, int ncomp, const float *d_arr,
                  float *d_out);

/* ROI (K9), math_tools.rs:574-661.  Polygon vertices are (x, y) pairs of
 * u64 as the reference's Vec<(usize, usize)>; arithmetic is u64 with
 * release-mode wrapping, bit-exact.  mask is (shape0, shape1) u8 indexed
 * [y * shape1 + x] in the function's own (swapped) coordinates. */
int thz_roi_mask(thz_ctx *ctx, const uint64_t *poly_xy, size_t n_vertices, uint64_t scaling,
                 size_t shape0, size_t shape1, uint8_t *d_mask);
/* mean over masked pixels of data[shape0 - y - 1, x, :] (:647); zeros when
 * the mask is empty (:656-658).  d_count (u32, may be NULL) gets the pixel
 * count; with sum_only != 0 the division is skipped (multi-GPU partials). */
int thz_roi_mean(thz_ctx *ctx, const float *d_arr, size_t shape0, size_t shape1, size_t len,
                 const uint8_t *d_mask, float *d_out, uint32_t *d_count, int sum_only);

/* math_tools::scaling scale_3d helper, math_tools.rs:273-301 (K10). */
int thz_scale3d(thz_ctx *ctx, const float *d_arr, size_t nx, size_t ny, size_t len, int ncomp,
                size_t s, float *d_out);

/* TiltCompensation::filter per-pixel copy, tilt_compensation.rs:171-201 (K11):
 * out[p, :ins] = in[p, 0]; out[p, ins:ins+nt_in] = in[p, :] * taper (clipped at
 * nt_out); zeros behind.  d_taper = thz_host_adapted_blackman(time, 0, 7).
 * The caller then re-plans with thz_set_time_axis(new_time) exactly as the
 * reference re-plans after a length change (data_thread.rs:1194-1227). */
int thz_tilt_apply(thz_ctx *ctx, size_t npix, const float *d_in, size_t nt_in, const float *d_taper,
                   const int32_t *d_insert_index, size_t nt_out, float *d_out);

/* ------------------------------------------------------------------ */
/* Deconvolution (K12), src/filters/deconvolution.rs + src/filters/psf.rs */
/* ------------------------------------------------------------------ */

/* CubicSplineCoeffs, psf.rs:7-14 (arrays as loaded from psf.npz, io.rs:146-166) */
typedef struct thz_spline {
    const float *knots;    /* n_knots   */
    const float *values;   /* n_knots   */
    const float *coeff_a;  /* n_knots-1 */
    const float *coeff_b;
    const float *coeff_c;
    const float *coeff_d;
    size_t n_knots;
} thz_spline;

/* HybridFit, psf.rs:17-22: a/f + b + spline correction */
typedef struct thz_hybrid_fit {
    float base_a, base_b;
    thz_spline correction;
} thz_hybrid_fit;

/* PSF, psf.rs:201-207 */
typedef struct thz_psf {
    thz_hybrid_fit wx_fit, wy_fit;
    thz_spline x0_spline, y0_spline;
} thz_psf;

/* Deconvolution fields, deconvolution.rs:239-253 (defaults 500 / 25 / 0.1 / 10 / 0.5) */
typedef struct thz_deconv_cfg {
    uint32_t n_iterations;
    uint32_t n_filters;
    float start_freq, end_freq, win_width;
    /* Band-parallel execution across GPUs: this call only sums
     * bands [band_begin, band_end) of the n_filters-band bank; 0, 0 = all bands;
     * band_begin == band_end > 0 = none (more ranks than bands).  The per-rank
     * d_out add up to the full result (all-reduce them) on every path: when a guard
     * or an abort makes the stage pass its input through, the rank that owns band 0
     * writes the input and every other rank zeros, so the all-reduce yields the
     * input once; every rank returns the same status for a guard.  d_img of a band
     * subset is the energy of a partial sum: take the image after the all-reduce.
     * The iteration schedule uses the beam widths of the whole bank. */
    uint32_t band_begin, band_end;
} thz_deconv_cfg;

/* host pieces, exported for tests and for hosts that want to show them:
 * HybridFit::eval_single / eval_single_const_extrap (psf.rs:83-131),
 * create_filter_bank (deconvolution.rs:160-211; filters n_filters x 499),
 * the per-band 2-D PSF (deconvolution.rs:906-960 + psf.rs:228-313; call with
 * out = NULL to get rows/cols). */
int thz_host_psf_eval(const thz_psf *psf, const float *freqs, size_t n, float *wx, float *wy,
                      float *x0, float *y0);
int thz_host_filter_bank(const float *time, size_t nt, const thz_deconv_cfg *cfg, float *filters,
                         float *centers);
int thz_host_band_psf(const thz_psf *psf, float center_freq, float dx, float dy, size_t img_rows,
                      size_t img_cols, float *out, size_t *rows, size_t *cols);

/* Deconvolution::filter, deconvolution.rs:766-1041, on the cube (nx, ny, nt) with
 * nt of the current time axis: FIR bank -> per band energy image ->
 * Richardson–Lucy against the band's Gaussian PSF -> gain sqrt(max(u,0)/d) ->
 * sum over bands of gain x filtered trace; d_img (may be NULL) = sum_t out^2.
 * d_gains_out (may be NULL) receives the (n_filters, nx, ny) gains.
 * abort_flag (may be NULL) is polled between iteration batches like the
 * reference's cancellable loops; *progress (may be NULL) is updated in [0,1].
 * Returns THZ_SKIPPED with out = in when one of the reference's guards applies
 * (empty PSF, image < 16x16, PSF wider than the image), THZ_ERR_ABORTED (out =
 * in) when aborted, THZ_ERR_UNSUPPORTED for traces of more than 7694 samples
 * (the FIR transform's padded length is at most 8192).  Blocking.  The call's device scratch (one padded spectrum
 * per pixel, the bands' images: ~0.6 KB x nt/1000 per pixel and band) and the
 * iteration graphs stay with the context for the next call of the same geometry and is released by a call of
 * another geometry or by thz_destroy.
 * Arithmetic against the reference's: fp32 FIR (the reference's is Complex<f64>); band energies as
 * Parseval's sum minus the two 249-sample edges of the full convolution; every band PSF as two 1-D passes over its
 * profiles — the same sums in another order, also for kernels of <= 256 taps, which the reference sums directly
 * (environment variable THZ_RL_NARROW_EXACT=1: those in the reference's own order, bit for bit).  Cube, gains and image
 * within 1e-5 of the reference's at its defaults (500 iterations, 25 bands). */
int thz_deconvolve(thz_ctx *ctx, const thz_psf *psf, const thz_deconv_cfg *cfg, size_t nx, size_t ny,
                   float dx, float dy, const float *d_in, float *d_out, float *d_img,
                   float *d_gains_out, volatile const int *abort_flag, float *progress);

/* ------------------------------------------------------------------ */
/* Pulse arrival times and the tilt they imply (K16)    */
/* ------------------------------------------------------------------ */
/* Not a reference function: the reference's Tilt Compensation takes two angles typed in by hand
 * (tilt_compensation.rs:27-32) and nothing says what they should be.  The quantity they describe is when the pulse
 * arrives at each pixel — also the time-of-flight image of a scan (thickness / depth contrast).
 *
 * thz_peak_map: per trace x[0 .. nt) of a (npix, nt) f32 cube, with key = |x| (mode 0), x (mode 1) or -x (mode 2):
 *   d_index  (npix) int32  position of the largest key.  Of equal keys the lowest index; a NaN never wins; a trace
 *                          of NaNs gives 0.
 *   d_value  (npix) f32    x[index], signed, exact
 *   d_offset (npix) f32    sub-sample vertex of the parabola through x[k-1], x[k], x[k+1]:
 *                          0.5 (y- - y+) / (y- - 2 y0 + y+) in f32, clamped to [-0.5, 0.5]; exactly 0 for k == 0,
 *                          k == nt - 1, a zero denominator or a non-finite value among the three
 * Any output may be NULL.  One streaming read of the cube, the traffic of thz_intensity; d_data needs 4-byte
 * alignment only.  nt <= 2^30.  Time under THZ_STAGE_PEAK. */
int thz_peak_map(thz_ctx *ctx, size_t npix, size_t nt, const float *d_data, int mode, int32_t *d_index,
                 float *d_offset, float *d_value);

/* The ten sums of the least-squares plane tau(u, v) = t0 + a u + b v over an (nx, ny) grid of the three images:
 * with vmax the largest finite |value|, a pixel takes part iff |value| is finite and >= rel_threshold * vmax (f32);
 *   u = (i - nx / 2) dx, v = (j - ny / 2) dy   (the centre rule of tilt_compensation.rs:159-164),
 *   tau = (index + offset) dt_ps               (ps from the axis' first sample)
 * moments = { S 1, S u, S v, S uu, S uv, S vv, S tau, S u tau, S v tau, S tau tau }, host, added in double in a fixed
 * order on a fixed launch geometry: the same images give the same ten doubles on every run and every device. */
int thz_arrival_plane_moments(thz_ctx *ctx, size_t nx, size_t ny, float dx, float dy, double dt_ps,
                              const int32_t *d_index, const float *d_offset, const float *d_value,
                              float rel_threshold, double *moments /* 10 */);

/* The plane and the angles that flatten it under the reference's rule delta = (u tilt_x + v tilt_y) / c
 * (tilt_compensation.rs:171-175, c = 0.299792458 mm / ps): tilt = -slope c radians, reported in degrees. */
typedef struct thz_tilt_fit {
    double tilt_x_deg, tilt_y_deg;
    double slope_x_ps_per_mm, slope_y_ps_per_mm;
    double t0_ps;   /* the plane at u = v = 0, from the axis' first sample */
    double rms_ps;  /* root mean square residual of the pixels that took part */
    uint64_t n_used;
} thz_tilt_fit;
/* Solves the plane's normal equations in double from the ten moments; no GPU involved.  THZ_SKIPPED with every field
 * zero when fewer than 3 pixels took part or the pixels do not span a plane (one row, one column, one line). */
int thz_host_arrival_plane_fit(const double *moments /* 10 */, thz_tilt_fit *out);

/* ------------------------------------------------------------------ */
/* Optical-property maps (K17)                          */
/* ------------------------------------------------------------------ */
/* calculate_optical_properties (math_tools.rs:663-701; thz_host_optical_properties) for every pixel of a scan, as means
 * over bands of bins.  The reference computes one vector (the selected pixel or a region's mean, data_thread.rs:1489-1559)
 * from absolute unwrapped phases.  Per pixel that is not enough: numpy_unwrap starts at bin 0, in the noise, so each
 * pixel's phase reaches the band with its own multiple of 2 pi.  The anchor removes it: over the bins [anchor_k0,
 * anchor_k1) the least-squares line delta_k = b + s k through delta_k = phase[p, k] - ref_phase[k] is fitted in double;
 * m = rint(b / 2 pi) (b: the line at bin 0; m = 0 when b is not finite) and the pixel's phases enter the formula as
 * fl32(phase - w), w = (float)(m 2 pi).  anchor_k0 == anchor_k1: no anchor, m = 0, w = +0 — the reference's own
 * absolute phases.  Per bin k of a band the values are the reference's f32 formula in its operation order (IEEE division
 * and fmaxf; no special case for a thickness <= 0, zero amplitudes or NaN):
 *   d_n, d_alpha, d_kappa  (n_bands, npix) f32, band-major: the mean over the band's bins [band_k0, band_k1), added in
 *                          f32 in an order that depends on the arguments alone (same inputs, same bits)
 *   d_wraps                (npix) int32: m
 *   d_slope                (npix) f32: (float)s, rad per bin — the group delay of the pixel against the reference: the
 *                          pixel's pulse arrives -s nt / (2 pi) samples after the reference's
 * Any output may be NULL.  d_amp, d_phase: (npix, nf) f32 on the device, 4-byte alignment; ref_amp, ref_phase, freq
 * (THz): nf host floats; d_thickness: one thickness per pixel (device, npix) or NULL for cfg->thickness everywhere.
 * One launch; only the anchor's and the bands' bins of each row are read.  THZ_ERR_INVALID before any launch unless
 * n_bands <= THZ_OPTICAL_MAX_BANDS, every band has 1 <= k0 < k1 <= nf (bin 0 has omega = 0) and the anchor has at least
 * two bins or none, and ends at nf or before.  npix == 0 is a no-op.  Time under THZ_STAGE_OPTICAL. */
#define THZ_OPTICAL_MAX_BANDS 8
typedef struct thz_optical_cfg {
    float thickness;               /* sample_thickness as the reference passes it; unused where a thickness image is given */
    uint32_t anchor_k0, anchor_k1; /* [a0, a1); equal = off */
    uint32_t n_bands;
    uint32_t band_k0[8], band_k1[8];
} thz_optical_cfg;
int thz_optical_maps(thz_ctx *ctx, size_t npix, size_t nf, const float *d_amp, const float *d_phase,
                     const float *ref_amp, const float *ref_phase, const float *freq, const thz_optical_cfg *cfg,
                     const float *d_thickness, float *d_n, float *d_alpha, float *d_kappa, int32_t *d_wraps,
                     float *d_slope);

/* ------------------------------------------------------------------ */
/* Echoes and layer thickness (K18)                     */
/* ------------------------------------------------------------------ */
/* Not a reference function.  A thickness is the delay between two pulses of one trace (front and back surface, coating
 * layers: time-of-flight tomography) or of the pulse against the reference pulse (transmission); thz_peak_map finds one
 * pulse only.  thz_echo_map is its multi-pulse form: the K strongest separated pulses of every trace.
 *
 * Per trace x[0 .. nt), with key as in thz_peak_map (mode 0 |x|, 1 x, 2 -x) and a NaN key ordered as -Inf:
 *   rank 0      thz_peak_map's result by definition: the same index, offset and value, bit for bit, in every corner that
 *               function defines (ties, NaNs, traces of -Inf).
 *   candidates  for the ranks j >= 1: sample i is a candidate when its key is not NaN, i == 0 || key[i] > key[i-1], and
 *               i == nt-1 || key[i] >= key[i+1].  A plateau gives its lowest index once; the shoulder of a pulse is
 *               never a candidate, wherever the guard window ends.
 *   threshold   thr = rel_threshold * key[index_0], one f32 product.  A candidate is admitted iff key >= thr (false when
 *               thr is NaN).
 *   rank j      (j = 1 .. K-1) the admitted candidate with the largest key among those with |i - index_m| >= guard for
 *               every earlier rank m < j; of equal keys the lowest index.  If there is none, this rank and every later
 *               one are absent: index -1, offset 0.0f, value 0.0f.
 *   offset, value of a found rank follow thz_peak_map's rules around that index: the same f32 parabola through x, the
 *               same clamp, the same exact-zero cases.
 *   d_count     (npix) int32: the number of ranks found, at least 1.
 * d_index (int32), d_offset, d_value (f32) are (K, npix), rank-major, in the way the optical maps are band-major.  Any
 * output may be NULL.  One wave per trace and one read of the cube from HBM: the rounds behind the first work on what
 * the wave holds in registers (traces of up to 4099 samples) or read the trace again through the cache; d_data needs
 * 4-byte alignment only.  THZ_ERR_INVALID before any launch for a mode outside 0..2, K outside 1..THZ_ECHO_MAX,
 * guard < 1, a threshold that is negative or not finite, nt == 0 or nt > 2^30.  npix == 0 is a no-op.  Time under
 * THZ_STAGE_ECHO. */
#define THZ_ECHO_MAX 4
typedef struct thz_echo_cfg {
    int32_t mode;         /* thz_peak_map's key: 0 |x|, 1 x, 2 -x */
    int32_t n_echoes;     /* K, 1 .. THZ_ECHO_MAX */
    int32_t guard;        /* >= 1: two reported pulses are at least this many samples apart */
    float rel_threshold;  /* finite, >= 0 */
} thz_echo_cfg;
int thz_echo_map(thz_ctx *ctx, size_t npix, size_t nt, const float *d_data, const thz_echo_cfg *cfg,
                 int32_t *d_index, float *d_offset, float *d_value, int32_t *d_count);

/* Delays and thicknesses from the (n_echoes, npix) index and offset maps of thz_echo_map.
 *   mode 0  per pixel the found ranks (index >= 0) are put in ascending index order; for l = 0 .. K-2
 *             delay[l] = (float)(i_{l+1} - i_l) + (o_{l+1} - o_l)   (int32 and f32 subtractions as written)
 *             thickness[l] = scale[l] * delay[l]
 *           and a layer whose later pulse is absent gets NaN in both.  Outputs (K-1, npix); K = 1 is THZ_ERR_INVALID.
 *   mode 1  one row: delay = (float)(i_0 - ref_index) + (o_0 - ref_offset), thickness = scale[0] * delay.
 * Either output may be NULL.  npix == 0 is a no-op.  Time under THZ_STAGE_ECHO. */
typedef struct thz_layer_cfg {
    int32_t mode;       /* 0: between consecutive pulses in TIME order; 1: rank 0 against a fixed arrival */
    float scale[4];     /* mm per sample of delay, per layer: reflection c dt / (2 n_l), transmission c dt / (n - 1) */
    int32_t ref_index;  /* mode 1: where the reference pulse peaks ... */
    float ref_offset;   /* ... and its sub-sample offset (thz_host_echo_trace on the reference pulse) */
} thz_layer_cfg;
int thz_layer_map(thz_ctx *ctx, size_t npix, int n_echoes, const int32_t *d_index, const float *d_offset,
                  const thz_layer_cfg *cfg, float *d_thickness, float *d_delay);

/* thz_echo_map's selection for one host vector: index, offset, value hold cfg->n_echoes entries each, count one.  No
 * GPU and no context: what gives ref_index / ref_offset from the reference pulse (thz_reference_spectrum's
 * reference_out).  THZ_ERR_INVALID for the configurations thz_echo_map refuses. */
int thz_host_echo_trace(const float *x, size_t nt, const thz_echo_cfg *cfg, int32_t *index, float *offset,
                        float *value, int32_t *count);

/* ------------------------------------------------------------------ */
/* Principal components of a scan (K19)                 */
/* ------------------------------------------------------------------ */
/* Not a reference function.  "Which pixels have a different spectrum at all?" is principal component analysis of the
 * spectra: the mean spectrum, the covariance of the columns over the pixels, its leading eigenvectors (the components)
 * and one score image per component.  Four calls that compose; the outputs of the first two are plain sums, so the
 * slabs of a group are added on the host.
 *
 * Every device call sees an (npix x L) f32 matrix X[p, j] = d_x[p * row_stride + j * col_step] (both in floats,
 * col_step >= 1, 4-byte alignment only: rows of the resident cubes are never 16-byte aligned), 1 <= L <=
 * THZ_PCA_MAX_LEN, and an optional d_mask: npix uint8 in the cube's own pixel order (not thz_roi_mask's swapped
 * coordinates), NULL for none.  A pixel with mask 0 is left out of the sums and of the Gram matrix; it still gets
 * scores.  Anything outside these limits, or a required pointer that is NULL, is THZ_ERR_INVALID before any launch or
 * allocation; npix == 0 is a no-op that returns zeros.  NaN and Inf get no special case: they propagate.
 *
 *   thz_pca_sums    sum[j] = sum over the unmasked pixels of X[p, j], added in f64 in a fixed order; *count their number.
 *   thz_pca_gram    gram[i * L + j] = sum_p a[p, i] * a[p, j] with a[p, j] = X[p, j] - mu[j], ONE f32 subtraction made when
 *                   the element is loaded (a = X when mu is NULL; a masked pixel enters as a = 0).  32 x 32 tiles of the
 *                   upper triangle over chunks of pixels on the exact-f32 matrix instruction (v_mfma_f32_32x32x2_f32, the
 *                   pixel index is its k; a diagonal tile's two operands are the same registers), whose result is a
 *                   k-ordered fmaf chain: one f32 accumulator takes at most THZ_PCA_CHAIN products before it is added
 *                   into f64, and a second kernel adds the slabs' f64 partial tiles in slab order and writes the lower
 *                   triangle as the mirror.  No floating-point atomics: the same inputs give the same bits on every
 *                   run, gram is exactly symmetric, and |gram_ij - exact| <= (THZ_PCA_CHAIN + 2) 2^-24 sum_p |a_pi a_pj|.
 *   thz_host_pca_components   plain C++ in f64, no GPU and no context (Householder tridiagonalisation + implicit QL):
 *                   C = gram / (count - 1); the K largest eigenvalues in descending order; each eigenvector with unit
 *                   2-norm, its sign chosen so that its entry of largest magnitude is positive (the lowest index wins a
 *                   tie), then rounded to f32 into components (K x L); *total_variance = trace(C).  THZ_ERR_INVALID for
 *                   count < 2, K outside 1 .. min(L, THZ_PCA_MAX_COMPONENTS), L outside 1 .. THZ_PCA_MAX_LEN, a
 *                   non-finite entry, or an iteration that does not converge (it is bounded: the call always returns).
 *   thz_pca_scores  d_scores[c * npix + p] = sum_j a[p, j] * components[c * L + j] in f32 for EVERY pixel, one wave per
 *                   pixel: lane l adds j = l, l + 64, ... in ascending order, then the lanes as a fixed tree — the order
 *                   depends on L alone.  mu (L host floats or NULL) and components (K x L host floats) go up once per call.
 * Time of the gram and score launches under THZ_STAGE_PCA. */
#define THZ_PCA_MAX_LEN 512
#define THZ_PCA_MAX_COMPONENTS 8
#define THZ_PCA_CHAIN 1024
int thz_pca_sums(thz_ctx *ctx, size_t npix, size_t L, const float *d_x, size_t row_stride, size_t col_step,
                 const uint8_t *d_mask, double *sum /* L, host */, uint64_t *count);
int thz_pca_gram(thz_ctx *ctx, size_t npix, size_t L, const float *d_x, size_t row_stride, size_t col_step,
                 const uint8_t *d_mask, const float *mu /* L host floats or NULL */, double *gram /* L x L, host */);
int thz_host_pca_components(const double *gram, size_t L, uint64_t count, int K, float *components /* K x L */,
                            double *eigenvalues /* K */, double *total_variance);
int thz_pca_scores(thz_ctx *ctx, size_t npix, size_t L, const float *d_x, size_t row_stride, size_t col_step,
                   const float *mu, const float *components, int K, float *d_scores /* (K, npix) */);

/* ------------------------------------------------------------------ */
/* Segmenting a scan into materials: k-means (K20)     */
/* ------------------------------------------------------------------ */
/* Not a reference function.  "Which pixels belong together?" is k-means of the pixels' rows: one label image and one
 * mean row (the mean spectrum of a material) per cluster.  One device call is one step of Lloyd's algorithm; the
 * centroid update is plain C++, so the slabs of a group are added on the host between the two.
 *
 * thz_cluster_step sees the matrix of the PCA calls above — X[p, j] = d_x[p * row_stride + j * col_step], 1 <= L <=
 * THZ_PCA_MAX_LEN, 4-byte alignment only, the optional d_mask of npix uint8 — and K x L host floats `centroids`,
 * 1 <= K <= THZ_CLUSTER_MAX, which go up once per call.
 *   assignment   for EVERY pixel, masked ones included, one wave per pixel with the centroids in LDS:
 *                dist2[c] = sum_j (X[p, j] - m[c, j])^2 in f32, d = x - m ONE f32 subtraction, lane l adding
 *                fmaf(d, d, acc) over j = l, l + 64, ... in ascending order, then the lanes as the fixed tree of
 *                thz_pca_scores — the order depends on L alone, and |dist2 - exact| <= (ceil(L / 64) + 9) 2^-24 exact.
 *                d_label[p] = the lowest c with the smallest dist2[c]; a NaN never wins; when all K are NaN the label
 *                is -1 and d_dist2[p] NaN, otherwise d_dist2[p] is the winner's.  *changed counts the pixels whose
 *                label differs from the one d_label held BEFORE the call (it is read, then overwritten; an integer
 *                count): a caller starts a run with d_label filled with -1.
 *   sums         over the unmasked pixels with label >= 0, all in f64 over fixed slabs of pixels whose partials a
 *                second kernel adds in slab order (no floating-point atomics: the same bits on every run):
 *                sums[c * L + j] = sum of X[p, j] over the pixels of cluster c (sums may be NULL: not returned),
 *                counts[c] their number, *inertia = sum of d_dist2[p], *farthest = the index of the pixel with the
 *                largest finite d_dist2, the lowest index winning a tie, npix when there is none.
 * THZ_ERR_INVALID, before any launch or allocation, for anything outside these limits or a required pointer that is
 * NULL (all but d_mask and sums); npix == 0 is a no-op that returns zeros.  NaN and Inf get no special case beyond the
 * label rule.  Time of the launches under THZ_STAGE_PCA.
 *
 * thz_host_cluster_update is plain C++, no GPU and no context: centroids[c, j] = (float)(sums[c, j] / counts[c]) in
 * f64; a cluster with counts[c] == 0 keeps previous[c, :] bit for bit (previous and centroids may be the same array).
 * THZ_ERR_INVALID for K outside 1 .. THZ_CLUSTER_MAX, L outside 1 .. THZ_PCA_MAX_LEN, a NULL pointer, or a non-finite
 * sum. */
#define THZ_CLUSTER_MAX 16
int thz_cluster_step(thz_ctx *ctx, size_t npix, size_t L, const float *d_x, size_t row_stride, size_t col_step,
                     const uint8_t *d_mask, const float *centroids /* K x L host */, int K,
                     int32_t *d_label, float *d_dist2 /* device, npix; d_label is read AND written */,
                     double *sums /* K x L host or NULL */, uint64_t *counts /* K */, double *inertia,
                     uint64_t *changed, uint64_t *farthest);
int thz_host_cluster_update(const double *sums, const uint64_t *counts, int K, size_t L,
                            const float *previous /* K x L */, float *centroids /* K x L */);

/* ------------------------------------------------------------------ */
/* Sparse deconvolution: overlapping echoes (K21)      */
/* ------------------------------------------------------------------ */
/* Not a reference function.  thz_echo_map finds separated pulses; two surfaces closer than a pulse width give one
 * merged wavelet.  Here every trace is written as y = h * x + noise with h the reference pulse and x a sparse spike
 * train, and 1/2 |y - H x|^2 + lam |x|_1 is minimised by iterative shrinkage (ISTA, or FISTA with momentum): the spikes
 * of x are the echoes.  All arithmetic is f32.
 *
 * y is one trace x[0 .. nt), h[0 .. P) the taps, c the centre tap: a spike at sample m puts h[c] at sample m.  With
 * T[i][m] = h[i + c - m], zero outside 0 <= i + c - m < P:
 *   (H z)[i]   = sum over m = 0 .. nt-1 of T[i][m] z[m]
 *   (H^T r)[j] = sum over i = 0 .. nt-1 of T[i][j] r[i]
 * each ONE fmaf chain from +0.0f in ascending order of the index of the vector it reads, acc = fmaf(T, v, acc); terms
 * with T = 0 may be skipped or executed (for finite data the value is the same).
 *   threshold  g0 = H^T y, gmax = max_j |g0[j]|, lam = fmaxf(rel_lambda * gmax, min_lambda), th = step * lam (one f32
 *              product each)
 *   start      x = z = 0
 *   iteration n = 0 .. n_iter-1:  r = y - H z;  g = H^T r;  v = fmaf(step, g, z);  a = fabsf(v) - th;
 *              xn = a > 0 ? copysignf(a, v) : +0.0f;  z = xn (accelerate == 0) or fmaf(beta[n], xn - x, xn)
 *              (accelerate == 1);  x = xn
 *   momentum   on the host in double: t_0 = 1, t_{n+1} = (1 + sqrt(1 + 4 t_n^2)) / 2, beta[n] = (float)((t_n - 1) /
 *              t_{n+1}); one function makes the table for the device (uploaded once per call) and for the host twin.
 * d_out (npix, nt) f32 is x after n_iter iterations (all zeros for n_iter == 0); d_resid (npix) f32 or NULL is
 * sum_i (y - H x)[i]^2, in any order of summation; d_nnz (npix) int32 or NULL the number of x[i] != 0.  d_out == d_data
 * (in place) is allowed; any other overlap is undefined.  A trace with a non-finite sample has unspecified values in
 * its own row and affects no other row; subnormal values are outside the definition.
 * THZ_ERR_INVALID, before any launch or allocation, for anything outside the limits below, a non-finite tap, nt == 0 or
 * nt > THZ_SPARSE_MAX_NT, or a NULL required pointer (all but d_resid and d_nnz); npix == 0 is a no-op.  d_data needs
 * 4-byte alignment only.  The cube is read once and written once whatever n_iter: one wave per trace keeps y, z, r and
 * x in LDS.  Time under THZ_STAGE_ECHO.
 *
 * thz_host_sparse_trace is plain C++ with the same chains, no GPU and no context: for finite data it equals the device
 * bit for bit, -0 and +0 compared as numbers.  y and x may be the same vector.
 * thz_host_sparse_kernel cuts the taps out of a reference pulse: k0 = the index of the largest |ref|, the lowest index
 * on ties (thz_host_echo_trace with one rank in mode 0); taps[k] = ref[k0 - center + k], zero outside [0, nref);
 * *step = (float)(1 / (sum |taps|)^2) in double — (sum |h|)^2 >= |H|^2 by Young's inequality, so this step converges.
 * THZ_ERR_INVALID when every tap is zero or one is not finite. */
#define THZ_SPARSE_MAX_TAPS 256
#define THZ_SPARSE_MAX_NT   4608   /* a 4096-sample scan and its tilt; z, r, x, y of one trace with their halos fit a CU's LDS */
#define THZ_SPARSE_MAX_ITER 4096
typedef struct thz_sparse_cfg {
    int32_t n_taps, center;      /* P in 1..THZ_SPARSE_MAX_TAPS, c in 0..P-1 */
    int32_t n_iter, accelerate;  /* 0..THZ_SPARSE_MAX_ITER; 0 ISTA, 1 FISTA */
    float step;                  /* finite, > 0; converges for step <= 1/||H||^2 */
    float rel_lambda, min_lambda;/* finite, >= 0 */
} thz_sparse_cfg;
int thz_sparse_deconv(thz_ctx *ctx, size_t npix, size_t nt, const float *d_data, const float *taps /* P host */,
                      const thz_sparse_cfg *cfg, float *d_out, float *d_resid, int32_t *d_nnz);
int thz_host_sparse_trace(const float *y, size_t nt, const float *taps, const thz_sparse_cfg *cfg,
                          float *x, float *resid, int32_t *nnz);
int thz_host_sparse_kernel(const float *ref, size_t nref, int n_taps, int center, float *taps, float *step);

/* ------------------------------------------------------------------ */
/* Unmixing every pixel into its materials: NNLS (K22) */
/* ------------------------------------------------------------------ */
/* Not a reference function.  "How much of each material is in every pixel?": for a pixel's row x and K known spectra
 * (the endmembers E, K x L — from a library, from pixels picked by hand, or the k-means centroids) the abundances a
 * minimise |x - E^T a|^2 subject to a >= 0.  All device arithmetic is f32.
 *
 * thz_unmix sees the matrix of the PCA calls above — X[p, j] = d_x[p * row_stride + j * col_step], 1 <= L <=
 * THZ_PCA_MAX_LEN, col_step >= 1, 4-byte alignment only — and K x L host floats `endmembers`, 1 <= K <= THZ_UNMIX_MAX
 * (= THZ_CLUSTER_MAX: centroids feed it directly), which go up once per call.
 *   element      u[p, j] = X[p, j] when cfg->absorbance == 0; otherwise u = lref[j] - logf(X[p, j]) (ONE f32
 *                subtraction) with lref[j] = (float)log((double)ref[j]) made on the host: Beer-Lambert absorbance against
 *                the reference spectrum `ref` of L host floats, required, finite and > 0 when absorbance != 0 (not read
 *                otherwise).  The endmembers are then absorbance spectra too.
 *   projection   b[c] = sum_j u[p, j] E[c, j], one wave per pixel: lane l adds j = l, l + 64, ... in ascending order,
 *                acc = fmaf(u, E, acc), then the lanes as the fixed tree of thz_pca_scores — the order depends on L
 *                alone, and |b - exact| <= (ceil(L / 64) + 8) 2^-24 sum_j |u E|, exact the f64 sum over the f32 u.
 *                With absorbance u itself lies within 2 ulp of |log X| plus one rounding of the subtraction of the f64
 *                value (DESIGN.md §4.12 has what was measured).
 *   normal matrix  on the host, thz_host_unmix_prepare, plain C++ with no GPU and no context: G64[i][c] = sum_j
 *                (double)E[i, j] (double)E[c, j] with j ascending, G = (float)G64, rd[c] = (float)(1.0 / G64[c][c]).
 *                THZ_ERR_INVALID for a non-finite entry, a zero endmember (G64[c][c] == 0), a non-finite rd, K outside
 *                1 .. THZ_UNMIX_MAX, L outside 1 .. THZ_PCA_MAX_LEN or a NULL pointer.
 *   solve        cyclic coordinate descent on the normal equations, one pixel at a time, from b, G, rd alone:
 *                    a[c] = +0, g[c] = -b[c]
 *                    sweep s = 0 .. n_sweeps-1, c = 0 .. K-1 in order:
 *                        an = fmaxf(fmaf(-g[c], rd[c], a[c]), 0.0f);  d = an - a[c];
 *                        for i = 0 .. K-1: g[i] = fmaf(G[i][c], d, g[i]);   a[c] = an;
 *                    kkt = max over c of (a[c] > 0 ? fabsf(g[c]) : fmaxf(-g[c], 0))
 *                g is the running gradient, not recomputed.  n_sweeps in 0 .. THZ_UNMIX_MAX_SWEEPS.  The update for
 *                d == 0 may be skipped, and a pixel (or a whole wave) whose last full sweep changed nothing may stop:
 *                the remaining sweeps would repeat it.  thz_host_unmix_solve is the plain-C++ twin: for finite data
 *                it equals the device bit for bit from the device's own b, -0 and +0 compared as numbers.
 *   residual     resid[p] = sum_j (u[p, j] - m_j)^2 with m_j the fmaf(a[c], E[c, j], m) chain from +0 over ascending c,
 *                the squares summed in any order; computed directly in a second pass over the row, never as
 *                xx - 2 a.b + a G a, which cancels.
 * d_abund (K, npix), endmember-major, is required; d_proj (K, npix) takes the b's; d_resid and d_kkt are (npix).  Each of
 * d_proj, d_resid and d_kkt may be NULL, and the second read of the cube is skipped when d_resid is NULL.
 * A row with a non-finite element has unspecified values in its own outputs and affects no other pixel.  npix == 0 is a
 * no-op.  Anything outside these limits, or a NULL required pointer, is THZ_ERR_INVALID before any launch or
 * allocation.  No floating-point atomics: the same inputs give the same bits on every run.  Time of the three launches
 * under THZ_STAGE_PCA. */
#define THZ_UNMIX_MAX 16
#define THZ_UNMIX_MAX_SWEEPS 4096
typedef struct thz_unmix_cfg {
    int32_t n_endmembers;        /* K, 1 .. THZ_UNMIX_MAX */
    int32_t n_sweeps;            /* 0 .. THZ_UNMIX_MAX_SWEEPS */
    int32_t absorbance;          /* 0: u = X; otherwise u = log(ref) - log(X) */
} thz_unmix_cfg;
int thz_unmix(thz_ctx *ctx, size_t npix, size_t L, const float *d_x, size_t row_stride, size_t col_step,
              const float *endmembers /* K x L host */, const float *ref /* L host, or NULL when absorbance == 0 */,
              const thz_unmix_cfg *cfg, float *d_abund /* (K, npix) */, float *d_proj /* (K, npix) or NULL */,
              float *d_resid /* npix or NULL */, float *d_kkt /* npix or NULL */);
int thz_host_unmix_prepare(const float *endmembers, int K, size_t L, float *G /* K x K */, float *rd /* K */);
int thz_host_unmix_solve(const float *b, const float *G, const float *rd, int K, int n_sweeps, float *a /* K */, float *kkt);

/* ------------------------------------------------------------------ */
/* Denoising every trace: wavelet shrinkage (K23)      */
/* ------------------------------------------------------------------ */
/* Not a reference function.  The traces are noisy, and the Wiener multiplier (K13) amplifies whatever lies outside the
 * reference's band; the standard remedy for THz pulses is wavelet shrinkage of the trace ("Wiener multiplier, then
 * wavelet shrinkage" is frequency-wavelet domain deconvolution).  All device arithmetic is f32.
 *
 * The transform is the undecimated (stationary, a trous) wavelet transform with periodic extension: translation
 * invariant, and defined for every trace length N = nt >= 1.  The caller passes Lf analysis taps hn[0 .. Lf) and
 * gn[0 .. Lf) as host floats, 1 <= Lf <= THZ_WAVELET_MAX_TAPS.
 *   forward    a_0 = y; for level j = 1 .. J and s = 2^(j-1):
 *                  a_j[i] = chain over k = 0 .. Lf-1 ascending from +0.0f: acc = fmaf(hn[k], a_{j-1}[(i + s k) mod N], acc)
 *                  d_j[i] = the same chain with gn
 *              The mod is the mathematical one: s k may exceed N many times over, and N = 1 is legal.
 *   threshold  m = the lower median of |d_1[i]|: the element of rank (N - 1) / 2 (integer division, 0-based) in
 *              ascending order — an order statistic, whose value does not depend on how it is found.
 *              noise_mode 0: th_j = scale[j-1] * m (one f32 product); noise_mode 1: th_j = scale[j-1].
 *              scale: J host floats, finite and >= 0.
 *   shrink     shrink 0 (soft): t = fabsf(d) - th; d' = t > 0 ? copysignf(t, d) : +0.0f (the sparse stage's rule).
 *              shrink 1 (hard): d' = fabsf(d) > th ? d : +0.0f.  a_J is kept as it is.
 *   inverse    r_J = a_J; for j = J .. 1, s = 2^(j-1):
 *                  ch = chain over k ascending from +0.0f: fmaf(hn[k], r_j[(i - s k) mod N], acc)
 *                  cg = chain over k ascending from +0.0f: fmaf(gn[k], d'_j[(i - s k) mod N], acc)
 *                  r_{j-1}[i] = ch + cg   (one f32 addition)
 *              The output is r_0.  For an orthonormal h with hn = h / sqrt 2 and gn[k] = (-1)^k hn[Lf-1-k] this
 *              reconstructs y exactly in exact arithmetic, for every N.
 * d_out (npix, nt) f32 is r_0; d_out == d_data (in place) is allowed, any other overlap is undefined.  d_sigma (npix) f32
 * or NULL is m; d_kept (npix) int32 or NULL the number of d'_j[i] != 0 over all levels.
 * Limits: 1 <= J <= THZ_WAVELET_MAX_LEVELS, nt <= THZ_WAVELET_MAX_NT and (J + 2) nt <= THZ_WAVELET_MAX_WORDS (the
 * ping-pong pair of approximations and J detail planes of one trace in a CU's LDS: 144 KiB at J = 6, nt = 4608).
 * Everything inside them runs.  Anything outside them, a non-finite tap or scale, a negative scale, shrink or noise_mode
 * outside {0, 1}, nt == 0 or a NULL required pointer (all but d_sigma and d_kept) is THZ_ERR_INVALID before any launch
 * or allocation; npix == 0 is a no-op.  A trace with a non-finite sample has unspecified values in its own outputs and
 * affects no other row; subnormals are outside the definition; -0 and +0 compare as numbers.  d_data needs 4-byte
 * alignment only.  The cube is read once and written once whatever J.  No floating-point atomics: the same inputs give
 * the same bits on every run.  Time under THZ_STAGE_ECHO.
 *
 * thz_host_wavelet_trace is the plain-C++ twin, no GPU and no context: for finite data it equals the device bit for
 * bit.  y and x may be the same vector.
 * thz_host_wavelet_filter gives the Daubechies filter of order 1 .. 4 (Lf = 2, 4, 6, 8; order 1 is Haar) from the
 * orthonormal h held as double literals in minimum-phase order: hn[k] = (float)(h[k] / sqrt 2), gn[k] =
 * (float)((-1)^k h[Lf-1-k] / sqrt 2).  Any other order is THZ_ERR_INVALID.
 * thz_host_wavelet_universal gives the universal threshold under the MAD noise estimate, in double:
 * scale[j-1] = (float)((sqrt 2 / 0.6744897501960817) 2^(-j/2) sqrt(2 ln nt)) — under white noise of deviation sigma d_1
 * has deviation sigma / sqrt 2, so sigma^ = m sqrt 2 / 0.6745, and level j's details have deviation sigma^ 2^(-j/2).
 * THZ_ERR_INVALID for nt == 0, n_levels outside 1 .. THZ_WAVELET_MAX_LEVELS or a NULL pointer. */
#define THZ_WAVELET_MAX_TAPS   16
#define THZ_WAVELET_MAX_LEVELS 6
#define THZ_WAVELET_MAX_NT     4608
#define THZ_WAVELET_MAX_WORDS  36864  /* (J + 2) nt */
typedef struct thz_wavelet_cfg {
    int32_t n_taps, n_levels;    /* Lf in 1..THZ_WAVELET_MAX_TAPS, J in 1..THZ_WAVELET_MAX_LEVELS */
    int32_t shrink, noise_mode;  /* 0 soft, 1 hard; 0: th_j = scale[j-1] * m, 1: th_j = scale[j-1] */
} thz_wavelet_cfg;
int thz_wavelet_denoise(thz_ctx *ctx, size_t npix, size_t nt, const float *d_data, const float *hn /* Lf host */,
                        const float *gn /* Lf host */, const float *scale /* J host */, const thz_wavelet_cfg *cfg,
                        float *d_out, float *d_sigma, int32_t *d_kept);
int thz_host_wavelet_trace(const float *y, size_t nt, const float *hn, const float *gn, const float *scale,
                           const thz_wavelet_cfg *cfg, float *x, float *sigma, int32_t *kept);
int thz_host_wavelet_filter(int order, float *hn /* 2 order */, float *gn /* 2 order */, int *n_taps);
int thz_host_wavelet_universal(size_t nt, int n_levels, float *scale /* n_levels */);

/* Synthetic input generator for benchmarks and tests (not a reference
 * function): derivative-of-Gaussian pulse + echo + 1 % noise
 * per trace from counter-based Philox4x32-10, identical to tests/synth.py.
 * Trace ids first_trace .. first_trace+ntraces-1; d_time is the nt-sample
 * time axis on the device. */
int thz_synth_cube(thz_ctx *ctx, float *d_out, size_t ntraces, uint64_t first_trace,
                   const float *d_time, uint32_t seed, int subtract_bias);

/* Measurement aid (not a reference function): moves the bytes of thz_pipeline in its access
 * shape — per trace read nt floats, write 2 nf + nf + nf + nt floats to four arrays — with no
 * arithmetic, so that the roofline can be quoted against what the memory system gives this
 * traffic pattern as well as against the 8 TB/s spec.  nt % 8 == 0; time under THZ_STAGE_PROBE. */
int thz_traffic_probe(thz_ctx *ctx, size_t npix, size_t nt, const float *d_in, float *d_fft, float *d_amp,
                      float *d_phase, float *d_data_out);

/* ------------------------------------------------------------------ */
/* Resident cube + whole-chain recompute ("session")                    */
/* ------------------------------------------------------------------ */
/* What the data thread keeps per open file, on the device: the raw cube
 * (after the load-time bias subtraction) and ONE set of outputs — spectrum,
 * amplitudes, phases, final trace cube, image, pixel means — instead of the
 * reference's nine full containers (config.rs:270, main.rs:178-268).  Because
 * the whole default chain is one HBM pass (thz_pipeline), every
 * UpdateType::Filter(idx) (data_thread.rs:1023) is served by re-running it from
 * the raw cube: that is the partial-recompute policy — nothing but the raw cube
 * is cached.  A non-zero tilt changes the trace length: the session re-plans for the
 * new length.  A 1001-sample scan tilted onto 1025 ... 1280 samples (up to 4.8 degrees
 * across 50 mm) still runs the whole chain as ONE launch from the raw cube
 * (thz_pipeline_tilted: the re-laying is folded into the FBP kernel's loads, the
 * complex multiplier and the pixel sums ride in the same launch); the extended cube
 * is only built when a region of interest or a plot asks for the extended traces.
 * Other tilted lengths take the staged path (tilt kernel into an extended cube, then
 * the transforms of the new length; beyond 1280 samples the FB kernels' two launches). */
typedef struct thz_session thz_session;

typedef struct thz_chain_cfg {
    /* TiltCompensation (tilt_compensation.rs:27-32); active by default with 0/0 */
    int32_t tilt_active;
    double tilt_x_deg, tilt_y_deg;
    /* Time Band Pass before the FFT (band_pass_td_before_fft.rs:28-33, reset :66-72) */
    int32_t td_before_active;
    double td_before_low, td_before_high, td_before_width;
    /* ConfigContainer.fft_window(_type), config.rs:171-213 */
    thz_window_cfg fft_window;
    /* Frequency Band Pass (band_pass_fd.rs:30-37) */
    int32_t fd_active;
    double fd_low, fd_high, fd_width;
    /* Time Band Pass after the inverse FFT (band_pass_td_after_fft.rs) */
    int32_t td_after_active;
    double td_after_low, td_after_high, td_after_width;
    /* pixel means of the ifft stage (math_tools.rs:421-440): 0 none; 1 amplitude / phase sums taken
     * inside the fused launch and avg_fft by linearity from the mean trace (<= 1e-5 of the reference's
     * values, no extra pass over the outputs; on a tilted cube the mean trace is that of the re-laid traces:
     * one launch's sums for the lengths 1025 ... 1280, thz_pixel_sum passes behind the launch for the others);
     * 2 the reference's summation order bit for bit (three passes over the outputs) */
    int32_t want_means;
    /* ConfigContainer.scale_factor: the chain's first stage, math_tools::scaling
     * (math_tools.rs:242-310).  s > 1 replaces the raw cube by its s x s block
     * means (sum / s^2, also on ragged edges), every later stage and output then
     * lives on the (nx / s, ny / s) grid with dx * s, dy * s (thz_session_grid);
     * s <= 1, or a side shorter than s, leaves the grid alone. */
    int32_t scale_factor;
    /* ConfigContainer.avg_in_fourier_space (config.rs:171-213; default false): the ifft stage then also
     * rebuilds a time trace from the pixel-mean amplitudes and phases — avg_data = C2R(from_polar(avg_signal_fft,
     * avg_phase_fft)) / nt (math_tools.rs:442-470), needs want_means — and every region of interest's roi_data
     * from its own mean amplitudes and phases (:496-529) instead of from the traces (:477-483). */
    int32_t avg_in_fourier_space;
} thz_chain_cfg;

/* Defaults of the reference after OpenFile + reset(): every filter active, bounds
 * = ends of the time axis, widths 2.0 / 0.1 ps, 0.2-5 THz / 0.1 THz, window
 * AdaptedBlackman [1, 7] ps, no tilt. */
int thz_chain_cfg_default(const float *time, size_t nt, thz_chain_cfg *out);

enum {
    THZ_BUF_RAW = 0,        /* (nx, ny, nt) f32 */
    THZ_BUF_FFT = 1,        /* (nx, ny, nf) complex */
    THZ_BUF_AMPLITUDES = 2, /* (nx, ny, nf) */
    THZ_BUF_PHASES = 3,     /* (nx, ny, nf) */
    THZ_BUF_DATA = 4,       /* (nx, ny, nt_out) final trace cube */
    THZ_BUF_IMG = 5,        /* (nx, ny) */
    THZ_BUF_AVG_FFT = 6,    /* (nf) complex   — needs want_means */
    THZ_BUF_AVG_AMPLITUDES = 7, /* (nf) */
    THZ_BUF_AVG_PHASES = 8, /* (nf) */
    THZ_BUF_OPACITY = 9,    /* (nx, ny, nt_out) after thz_session_voxels */
    THZ_BUF_PEAK_INDEX = 10,  /* int32, one per pixel of the grid thz_session_peak_map last mapped */
    THZ_BUF_PEAK_OFFSET = 11, /* f32, likewise */
    THZ_BUF_PEAK_VALUE = 12,  /* f32, likewise */
    THZ_BUF_OPT_N = 13,       /* (n_bands, npix) f32 of the last thz_session_optical_maps, band-major */
    THZ_BUF_OPT_ALPHA = 14,   /* likewise */
    THZ_BUF_OPT_KAPPA = 15,   /* likewise */
    THZ_BUF_OPT_WRAPS = 16,   /* (npix) int32 */
    THZ_BUF_OPT_SLOPE = 17,   /* (npix) f32 */
    THZ_BUF_ECHO_INDEX = 18,  /* (n_echoes, npix) int32 of the last thz_session_echo_map, rank-major */
    THZ_BUF_ECHO_OFFSET = 19, /* (n_echoes, npix) f32 */
    THZ_BUF_ECHO_VALUE = 20,  /* (n_echoes, npix) f32 */
    THZ_BUF_ECHO_COUNT = 21,  /* (npix) int32 */
    THZ_BUF_LAYER_THICKNESS = 22, /* (rows, npix) f32 of the last thz_session_layer_map */
    THZ_BUF_LAYER_DELAY = 23, /* likewise */
    THZ_BUF_PCA_SCORES = 24,  /* (K, npix) f32 of the last thz_session_pca / _pca_project, component-major */
    THZ_BUF_PCA_COMPONENTS = 25, /* (K, L) f32 */
    THZ_BUF_PCA_MEAN = 26,    /* (L) f32; zeros when the call did not centre */
    THZ_BUF_CLUSTER_LABELS = 27, /* (npix) int32 of the last thz_session_cluster / _cluster_step; -1: every distance NaN */
    THZ_BUF_CLUSTER_DIST = 28,   /* (npix) f32: squared distance to the pixel's centroid */
    THZ_BUF_CLUSTER_CENTROIDS = 29, /* (K, L) f32: the centroids the labels belong to, one mean row per cluster */
    THZ_BUF_SPARSE = 30,       /* (npix, nt_src) f32: the spike trains of the last thz_session_sparse_deconv */
    THZ_BUF_SPARSE_RESID = 31, /* (npix) f32: sum of (y - H x)^2 per trace */
    THZ_BUF_SPARSE_NNZ = 32,   /* (npix) int32: spikes per trace */
    THZ_BUF_UNMIX_ABUNDANCE = 33, /* (K, npix) f32 of the last thz_session_unmix, endmember-major */
    THZ_BUF_UNMIX_PROJ = 34,   /* (K, npix) f32: the projections b the abundances were solved from */
    THZ_BUF_UNMIX_RESID = 35,  /* (npix) f32: sum of (u - E^T a)^2 per pixel */
    THZ_BUF_UNMIX_KKT = 36,    /* (npix) f32: the largest violation of the optimality conditions left */
    THZ_BUF_DENOISED = 37,     /* (npix, nt_src) f32: the denoised traces of the last thz_session_wavelet_denoise */
    THZ_BUF_DENOISE_SIGMA = 38, /* (npix) f32: the lower median of |d_1| per trace */
    THZ_BUF_DENOISE_KEPT = 39  /* (npix) int32: detail coefficients kept per trace */
};

int thz_session_create(thz_ctx *ctx, size_t nx, size_t ny, size_t nt, const float *time, float dx,
                       float dy, thz_session **out);
void thz_session_destroy(thz_session *s);
/* open_scan_from_thz's in-memory part (io.rs:576-628): H2D, per-trace bias
 * subtraction when asked, intensity image of the raw cube.  `cube` is host
 * memory (nx, ny, nt) C-order, or NULL when the caller fills the raw buffer
 * itself through thz_session_buffer(). */
int thz_session_upload(thz_session *s, const float *cube, int subtract_bias);
/* UpdateType::Filter(1) (ConfigCommand::UpdateFilters, SetDownScaling: data_thread.rs:836-838, 903-905):
 * recomputes every output. */
int thz_session_recompute(thz_session *s, const thz_chain_cfg *cfg);
/* UpdateType::Filter(start_idx), data_thread.rs:1090-1105: the stage walk starts at chain position
 * start_stage of the reference's filter_chain (main.rs:182-247; "initial" is 0):
 *   1 scaling  2 Tilt Compensation  3 Time Band Pass  4 fft  5 Frequency Band Pass (+ the plugins of
 *   thz_session_set_fd_filters)  6 ifft  7 Time Band Pass (after)  8 Deconvolution
 * (UpdateFilter(uuid) sends the filter's own position, :907-921; the fft window commands send fft_index =
 * 3, one in front of the fft stage, :813-836.)  Positions 1-5 run the one-pass chain from the raw cube:
 * the resident spectrum is the band-passed one, so nothing in front of position 6 can restart from an
 * intermediate.  Positions 6 and 7 re-run only C2R -> Time Band Pass -> image on the resident spectrum
 * (a third of the full chain's traffic) — provided the last full recompute used the same settings in
 * front of position 6, else they fall back to the full chain.  Position 8 is thz_session_deconvolve's;
 * here it is a no-op.
 * The unwrapped phases are those of the transform in front of the Frequency Band Pass and its plugins: they
 * depend on the source traces, the scale factor, the tilt and the multipliers in front of the transform
 * (tilt taper, Time Band Pass, fft window) alone.  A full recompute that changes none of these — a drag on
 * the Frequency Band Pass, a plugin, the Time Band Pass (after) — leaves THZ_BUF_PHASES and the phases'
 * pixel sums as they are instead of computing the same values again (nt = 4096, a band that ends at or
 * below bin 1152; every other recompute computes them).  The outputs are the same either way. */
int thz_session_recompute_from(thz_session *s, const thz_chain_cfg *cfg, int start_stage);
/* Further Frequency-domain plugins of the chain (FilterDomain::Frequency, behind "Frequency Band Pass"),
 * as per-bin multipliers for the chain's nf bins (host vectors, copied; NULL removes one): a real one —
 * the water-line notch K14, thz_host_water_line_mask — and a complex one — the reference-pulse Wiener
 * filter K13, thz_host_wiener_filter.  Both ride in the fused launch.  A later recompute whose spectra
 * have another length (tilted cube) returns THZ_ERR_INVALID. */
int thz_session_set_fd_filters(thz_session *s, const float *real_mask, const float *cmask, size_t nf);
/* Regions of interest — ScannedImageFilterData::rois (data_container.rs:109-162), edited by ConfigCommand::AddROI /
 * UpdateROI / DeleteROI (data_thread.rs:922-1000).  Replaces the session's whole set (n_rois = 0 removes it).
 * poly_xy: the polygons' vertices one after the other, (x, y) u64 pairs exactly as the reference keeps them
 * (f64 -> usize by truncation, :936-939: pixels of the RAW grid — average_polygon_roi divides them by the
 * scale factor itself, math_tools.rs:606-609); n_vertices[i] of them belong to region i.  From the next
 * recompute on, the ifft stage's per-region means (math_tools.rs:473-543) and the plot copy-out's
 * (data_thread.rs:1442-1482) are taken with every recompute and read with thz_session_roi. */
int thz_session_set_rois(thz_session *s, size_t n_rois, const size_t *n_vertices, const uint64_t *poly_xy);
size_t thz_session_roi_count(const thz_session *s);
/* One region's vectors after a recompute; host pointers, any may be NULL.  The masks follow the reference's
 * integer rule bit for bit (thz_roi_mask); the sampled pixel of mask position (x, y) is [shape0 - y - 1, x]
 * (math_tools.rs:647).  With want_means == 2 the pixels are added in the reference's order — y outer, x inner,
 * sequential f32 — and divided by the count: the means are those of the resident arrays bit for bit; otherwise
 * (0, 1) the sums are taken in parallel (<= 2e-6 of the largest value away). */
typedef struct thz_roi_out {
    float *signal_fft; /* nf_out  roi_signal_fft: mean amplitudes (:485, data_thread.rs:1453-1461) */
    float *phase_fft;  /* nf_out  roi_phase_fft: mean unwrapped phases (:486, :1464-1472) */
    float *signal;     /* nt_out  data.roi_signal of the plot copy-out: mean of the chain's FINAL traces
                                   (data_thread.rs:1445-1451) or, with avg_in_fourier_space, roi_data (:1476-1482) */
    float *roi_data;   /* nt_out  the ifft stage's roi_data: mean of the stage's input traces — the fft stage's
                                   windowed `data` — (math_tools.rs:477-483) or, with avg_in_fourier_space,
                                   C2R(from_polar(signal_fft, phase_fft), Im X[0] := 0) / nt (:496-529; where realfft
                                   would refuse the spectrum — Im of the last bin of an even length != 0 — the
                                   reference's fallback: the mean of the traces, :530-538) */
    uint32_t *count;   /* pixels inside the polygon */
} thz_roi_out;
int thz_session_roi(thz_session *s, size_t roi, const thz_roi_out *out);

/* Grid of the last recompute's outputs (the raw grid until then): every buffer
 * except THZ_BUF_RAW has nx * ny pixels of this grid.  Any pointer may be NULL. */
int thz_session_grid(const thz_session *s, size_t *nx, size_t *ny, float *dx, float *dy);
/* UpdateType::Filter(<Deconvolution>): the chain's last stage (FilterDomain::
 * TimeAfterFFTPrioLast, deconvolution.rs:751) — Deconvolution::filter
 * (deconvolution.rs:766-1041) on the "Time Band Pass" output of the last
 * recompute, with the session's dx / dy.  Its result is THZ_BUF_DATA /
 * THZ_BUF_IMG (and what thz_session_voxels / thz_session_plot read) until the
 * next thz_session_recompute: the reference does not re-run the deconvolution
 * when another filter is updated (data_thread.rs:1080, 1139-1149), the stage
 * then passes its input through (:1186-1188).  Calling it again deconvolves the
 * Time Band Pass output again, not the previous result.  Returns THZ_OK,
 * THZ_SKIPPED (a guard returned the input unchanged; the output is that copy)
 * or a negative code (THZ_ERR_ABORTED: the final output is the input again). */
int thz_session_deconvolve(thz_session *s, const thz_psf *psf, const thz_deconv_cfg *cfg,
                           volatile const int *abort_flag, float *progress);
/* trace length of the final cube (nt, or nt + 2*steps after a tilt) and its axis */
size_t thz_session_nt_out(const thz_session *s);
int thz_session_time_out(const thz_session *s, float *time /* nt_out */);
/* device pointer of a resident buffer; NULL if absent — every output buffer (everything but THZ_BUF_RAW
 * and THZ_BUF_IMG) is absent until a recompute has run after the latest upload.
 * THZ_BUF_FFT and THZ_BUF_AMPLITUDES: the session is the only writer of these two arrays and, between
 * recomputes, leaves in place the zeros that the Frequency Band Pass puts outside its range instead of
 * storing them again.  A caller may write through the pointer until the NEXT recompute: every call of this
 * function for one of the two makes that recompute store every bin.  Writing through a pointer obtained
 * earlier, after a later recompute, is outside the contract — bins outside the band would keep what was
 * written.  (The same holds for the sessions of a group, thz_group_session_member.)
 * THZ_BUF_PHASES likewise: the session is its only writer and leaves the phases in place while nothing
 * they depend on changes (thz_session_recompute_from); every call of this function for THZ_BUF_PHASES or
 * for THZ_BUF_RAW makes the next recompute compute and store them all.  A raw cube written through a held
 * pointer is followed by thz_session_upload(s, NULL, ...) as before. */
void *thz_session_buffer(thz_session *s, int which);
/* copies pixels [pix0, pix0+npix) of a per-pixel buffer (or the whole vector for
 * the AVG_* ones, pix0 = 0, npix = 1) to the host: the selected-pixel trace, a
 * tile, or everything.  THZ_ERR_NOT_READY for an absent buffer, THZ_ERR_INVALID for a
 * pixel range beyond the grid of the recompute that filled it. */
int thz_session_download(thz_session *s, int which, size_t pix0, size_t npix, void *dst);

/* thz_peak_map on a resident cube: `which` = THZ_BUF_RAW (the raw grid, nt samples) or THZ_BUF_DATA (the last
 * recompute's grid and final traces, nt_out samples; the deconvolved cube after thz_session_deconvolve).  Fills the
 * three resident images THZ_BUF_PEAK_INDEX / _OFFSET / _VALUE (thz_session_buffer, thz_session_download; absent until
 * the first call, and again after an upload).  THZ_ERR_NOT_READY when the cube is absent. */
int thz_session_peak_map(thz_session *s, int which, int mode);
/* The map, the moments and the fit in one call: the angles that flatten the arrival plane of `which`.  THZ_BUF_RAW
 * uses the raw grid's dx / dy and time axis, THZ_BUF_DATA thz_session_grid's and thz_session_time_out's; dt is the
 * axis' mean step.  Returns thz_host_arrival_plane_fit's code. */
int thz_session_estimate_tilt(thz_session *s, int which, int mode, float rel_threshold, thz_tilt_fit *out);

/* thz_optical_maps on the resident amplitudes and phases of the last recompute, on its grid (thz_session_grid) and with
 * the frequency axis of its time axis (thz_host_frequency_axis of thz_session_time_out).  ref_amp / ref_phase: nf host
 * floats, e.g. thz_reference_spectrum's; nf must be nt_out / 2 + 1 (THZ_ERR_INVALID).  THZ_ERR_NOT_READY when no
 * recompute has run since the last upload.  Reads the two arrays in place: the next recompute still knows their zeros.
 * Fills the five resident images THZ_BUF_OPT_N / _ALPHA / _KAPPA / _WRAPS / _SLOPE (thz_session_buffer,
 * thz_session_download; absent until the first call, and again after an upload).  For the three band-major ones the
 * pix0 / npix of thz_session_download count over the flattened (band, pixel) array of the last call.
 * A group has no form of its own: call this on thz_group_session_member(gs, i) with that slab's rows of the thickness
 * image; every pixel is independent, so the slabs' maps are the whole grid's rows.
 * A row of THZ_BUF_LAYER_THICKNESS (thz_session_layer_map below), taken through thz_session_buffer, is a valid
 * d_thickness when the echo map was taken on this grid: the thickness image never leaves the device. */
int thz_session_optical_maps(thz_session *s, const float *ref_amp, const float *ref_phase, size_t nf,
                             const thz_optical_cfg *cfg, const float *d_thickness);

/* thz_echo_map on a resident cube: `which` = THZ_BUF_RAW or THZ_BUF_DATA exactly as for thz_session_peak_map (the same
 * grids, the same THZ_ERR_NOT_READY and THZ_ERR_INVALID cases).  Fills the four resident images THZ_BUF_ECHO_INDEX /
 * _OFFSET / _VALUE / _COUNT (thz_session_buffer, thz_session_download; absent until the first call, and again after an
 * upload).  For the three rank-major ones the pix0 / npix of thz_session_download count over the flattened (rank, pixel)
 * array of the last call.
 * thz_session_layer_map runs thz_layer_map on the last echo map (THZ_ERR_NOT_READY when there is none) and fills
 * THZ_BUF_LAYER_THICKNESS / _DELAY, (K - 1, npix) in mode 0 and (1, npix) in mode 1, with the same download rule.
 * A group has no form of its own: call these on thz_group_session_member(gs, i); every pixel is independent, so the
 * slabs' maps are the whole grid's rows. */
int thz_session_echo_map(thz_session *s, int which, const thz_echo_cfg *cfg);
int thz_session_layer_map(thz_session *s, const thz_layer_cfg *cfg);

/* thz_sparse_deconv on a resident cube: `which` = THZ_BUF_RAW or THZ_BUF_DATA exactly as for thz_session_peak_map (the
 * same grids, the same THZ_ERR_NOT_READY and THZ_ERR_INVALID cases), or THZ_BUF_DENOISED: the denoised traces of the last
 * thz_session_wavelet_denoise, on the grid they were taken of (THZ_ERR_NOT_READY before a denoise call).  Fills the resident buffers THZ_BUF_SPARSE
 * (npix, nt of that cube) / _SPARSE_RESID (npix f32) / _SPARSE_NNZ (npix int32) (thz_session_buffer,
 * thz_session_download with pix0 / npix in pixels; absent until the first call, and again after an upload).  The
 * session remembers the grid and time axis they belong to: thz_session_peak_map, thz_session_echo_map,
 * thz_session_estimate_tilt and thz_group_session_estimate_tilt accept `which` = THZ_BUF_SPARSE and then run on the spike
 * trains (THZ_ERR_NOT_READY before a sparse call), so thz_session_layer_map turns a thin coating's two spikes into a
 * thickness image that reaches thz_session_optical_maps without leaving the device.
 * A group has no form of its own: call this on thz_group_session_member(gs, i); every pixel is independent, so the
 * slabs' spike trains are the whole grid's rows. */
int thz_session_sparse_deconv(thz_session *s, int which, const float *taps, const thz_sparse_cfg *cfg);

/* thz_wavelet_denoise on a resident cube: `which` = THZ_BUF_RAW or THZ_BUF_DATA exactly as for thz_session_sparse_deconv.
 * Fills the resident buffers THZ_BUF_DENOISED (npix, nt of that cube) / _DENOISE_SIGMA (npix f32) / _DENOISE_KEPT (npix
 * int32) (thz_session_buffer, thz_session_download with pix0 / npix in pixels; absent until the first call, and again
 * after an upload; a refused call leaves the last result resident).  The session remembers the grid and time axis they
 * belong to: thz_session_peak_map, thz_session_echo_map, thz_session_estimate_tilt, thz_group_session_estimate_tilt and
 * thz_session_sparse_deconv accept `which` = THZ_BUF_DENOISED and then run on the denoised traces (THZ_ERR_NOT_READY
 * before a denoise call).  A recompute with the Wiener multiplier followed by this call on THZ_BUF_DATA is
 * frequency-wavelet domain deconvolution on the device.
 * A group has no form of its own: call this on thz_group_session_member(gs, i); every pixel is independent, so the
 * slabs' traces are the whole grid's rows. */
int thz_session_wavelet_denoise(thz_session *s, int which, const float *hn, const float *gn, const float *scale,
                                const thz_wavelet_cfg *cfg);

/* Principal components of a resident cube.  `which` names the matrix: THZ_BUF_AMPLITUDES or THZ_BUF_PHASES (columns
 * are bins, nf = nt_out / 2 + 1 of them), THZ_BUF_DATA (samples, nt_out) — all three on the last recompute's grid, as
 * thz_session_peak_map and thz_session_optical_maps define it, THZ_ERR_NOT_READY before a recompute — or THZ_BUF_RAW
 * (samples, nt, the raw grid).  THZ_BUF_FFT and anything else is THZ_ERR_INVALID.  Column j of the matrix is column
 * first + j * step of the cube, j = 0 .. count-1: count in 1 .. THZ_PCA_MAX_LEN, step >= 1, the last one inside the
 * row (THZ_ERR_INVALID).  d_mask: optional, one uint8 per pixel of that grid, on the session's device.
 * The spectra are read in place through the session's own pointers: the next recompute still knows their zeros.
 *
 * thz_session_pca runs the four calls: thz_pca_sums; mu = (float)(sum / count) in f64 (center == 0: no mu is formed,
 * the Gram matrix is taken of X itself and THZ_BUF_PCA_MEAN holds zeros); thz_pca_gram; thz_host_pca_components with
 * that count; thz_pca_scores.  It fills *out and the three resident buffers THZ_BUF_PCA_SCORES (K, npix) /
 * _COMPONENTS (K, L) / _MEAN (L) (thz_session_buffer, thz_session_download; absent until the first call, and again
 * after an upload; for the first two the pix0 / npix of thz_session_download count over the flattened array, for the
 * mean over its L entries).
 * The covariance is NOT pixel-independent, so a group cannot call thz_session_pca slab by slab.  The three piece calls
 * are what a group's owner runs on every thz_group_session_member(gs, i): _pca_sums and _pca_gram per member, added on
 * the host in member order (f64), thz_host_pca_components once, then _pca_project per member with the common mu and
 * components, which fills that member's three buffers (mu NULL: not centred).  GpuEngine::pca does this for the
 * members of one process; a collective form for rank processes is not provided. */
typedef struct thz_pca_cfg {
    uint32_t first, count, step; /* the columns (bins or samples): first + j * step, j = 0 .. count-1 */
    int32_t n_components;        /* K, 1 .. min(count, THZ_PCA_MAX_COMPONENTS) */
    int32_t center;              /* 0: second moments of X itself; otherwise the covariance about the mean */
    const uint8_t *d_mask;       /* NULL, or one byte per pixel (device): 0 leaves the pixel out of mean and covariance */
} thz_pca_cfg;
typedef struct thz_pca_out {
    double eigenvalues[8];       /* the first n_components, descending; the rest 0 */
    double total_variance;       /* trace of the covariance */
    uint64_t count;              /* unmasked pixels */
} thz_pca_out;
int thz_session_pca(thz_session *s, int which, const thz_pca_cfg *cfg, thz_pca_out *out);
int thz_session_pca_sums(thz_session *s, int which, const thz_pca_cfg *cfg, double *sum /* count */, uint64_t *count);
int thz_session_pca_gram(thz_session *s, int which, const thz_pca_cfg *cfg, const float *mu, double *gram);
int thz_session_pca_project(thz_session *s, int which, const thz_pca_cfg *cfg, const float *mu,
                            const float *components);

/* k-means of the pixels of a resident cube.  `which` and the columns first / count / step name the matrix exactly as
 * for thz_session_pca (same grids, same THZ_ERR_NOT_READY / THZ_ERR_INVALID cases), read in place through the session's
 * own pointers; in addition THZ_BUF_PCA_SCORES names the score images of the last thz_session_pca / _pca_project: the
 * columns are then the components (first + j * step < K of that call), the pixels those of the score images, and the
 * call is THZ_ERR_NOT_READY before a PCA call.  n_clusters in 1 .. THZ_CLUSTER_MAX, init 0 or 1, max_iter in
 * 1 .. 1000, centroids not NULL when init == 0: anything else is THZ_ERR_INVALID.
 *
 * thz_session_cluster:
 *   seeds    init 0: cfg->centroids.  init 1, farthest-first: mu = (float)(sum / count) from thz_pca_sums
 *            (THZ_ERR_INVALID when no pixel is unmasked); c_0 = the row of the pixel farthest from mu (a step with
 *            K = 1; THZ_ERR_INVALID when no distance is finite); c_k = the row of the pixel farthest from its nearest
 *            of c_0 .. c_k-1 (a step with K = k); with no finite farthest pixel the remaining seeds repeat the last
 *            one — ties go to the lowest label, so the repeats stay empty.
 *   loop     the labels start at -1; a step, then thz_host_cluster_update, until a step reports changed == 0
 *            (converged = 1) or max_iter steps have run.  No update follows the last step: the centroids kept are the
 *            ones that step used, so labels, distances and centroids belong together.
 *   *out     inertia, counts and their sum of the last step, the steps run and whether the last one changed nothing.
 * It fills the resident buffers THZ_BUF_CLUSTER_LABELS (npix int32) / _DIST (npix f32) / _CENTROIDS (K, L f32)
 * (thz_session_buffer, thz_session_download, whose pix0 / npix count entries of the flattened array; absent until
 * the first call, and again after an upload).  The centroid rows are the mean spectra per material.
 *
 * Clustering is NOT pixel-independent, so a group cannot call thz_session_cluster slab by slab.  The two piece calls
 * are what a group's owner runs on every thz_group_session_member(gs, i):
 *   thz_session_cluster_step  one thz_cluster_step on the member's matrix and its resident labels and distances, with
 *            K = cfg->n_clusters rows in `centroids`, which become THZ_BUF_CLUSTER_CENTROIDS.  cfg->init != 0 fills
 *            the labels with -1 first (every seeding step and the first step of a loop); the buffers are also
 *            started afresh when the number of pixels has changed.  cfg->max_iter and cfg->centroids are not read.
 *            The owner adds sums, counts, inertia and changed in member order and takes the farthest pixel as the
 *            largest THZ_BUF_CLUSTER_DIST entry among the members' candidates, the lowest global index winning a tie.
 *   thz_session_cluster_row   the `count` values of row `pixel` of the member's matrix, to the host.
 * GpuEngine::cluster does this for the members of one process; a collective form for rank processes is not provided. */
typedef struct thz_cluster_cfg {
    uint32_t first, count, step;  /* the columns (bins, samples or components), exactly as thz_pca_cfg */
    int32_t n_clusters;           /* K, 1 .. THZ_CLUSTER_MAX */
    int32_t init;                 /* 0: cfg->centroids; 1: farthest-first */
    int32_t max_iter;             /* 1 .. 1000 */
    const uint8_t *d_mask;        /* NULL, or one byte per pixel (device): 0 leaves the pixel out of sums, seeds and inertia */
    const float *centroids;       /* init 0: K x count host floats */
} thz_cluster_cfg;
typedef struct thz_cluster_out {
    double inertia;               /* sum of the squared distances of the unmasked, labelled pixels */
    uint64_t count;               /* those pixels */
    uint64_t counts[16];          /* per cluster; the entries from n_clusters on are 0 */
    int32_t iterations, converged;
} thz_cluster_out;
int thz_session_cluster(thz_session *s, int which, const thz_cluster_cfg *cfg, thz_cluster_out *out);
int thz_session_cluster_step(thz_session *s, int which, const thz_cluster_cfg *cfg, const float *centroids,
                             double *sums, uint64_t *counts, double *inertia, uint64_t *changed, uint64_t *farthest);
int thz_session_cluster_row(thz_session *s, int which, const thz_cluster_cfg *cfg, uint64_t pixel, float *row /* count */);

/* thz_unmix on a resident cube.  `which` and the columns first / count / step name the matrix exactly as for
 * thz_session_pca: THZ_BUF_AMPLITUDES, _PHASES, _DATA or _RAW, the same grids and the same THZ_ERR_NOT_READY /
 * THZ_ERR_INVALID cases; anything else, THZ_BUF_PCA_SCORES included, is THZ_ERR_INVALID.  The spectra are read in place
 * through the session's own pointers: the next recompute still knows their zeros.
 * cfg->endmembers: n_endmembers x count host floats, or NULL for the resident THZ_BUF_CLUSTER_CENTROIDS — the
 * hard-labels-to-fractions path, with no trip to the host beyond the K x L copy: THZ_ERR_NOT_READY when there are none,
 * THZ_ERR_INVALID unless that plane holds exactly n_endmembers x count entries.  cfg->ref: count host floats when
 * absorbance != 0.
 * It fills the resident buffers THZ_BUF_UNMIX_ABUNDANCE (K, npix) / _PROJ (K, npix) / _RESID (npix) / _KKT (npix)
 * (thz_session_buffer, thz_session_download; absent until the first call, and again after an upload; for the first two
 * the pix0 / npix of thz_session_download count over the flattened array).
 * A group has no form of its own: call this on thz_group_session_member(gs, i); every pixel is independent, so the
 * slabs' maps are the whole grid's rows. */
typedef struct thz_unmix_session_cfg {
    uint32_t first, count, step;  /* the columns (bins or samples), exactly as thz_pca_cfg */
    int32_t n_endmembers;         /* K, 1 .. THZ_UNMIX_MAX */
    int32_t n_sweeps;             /* 0 .. THZ_UNMIX_MAX_SWEEPS */
    int32_t absorbance;           /* as thz_unmix_cfg */
    const float *endmembers;      /* K x count host floats; NULL: the resident k-means centroids */
    const float *ref;             /* count host floats when absorbance != 0 */
} thz_unmix_session_cfg;
int thz_session_unmix(thz_session *s, int which, const thz_unmix_session_cfg *cfg);

/* ------------------------------------------------------------------ */
/* Multi-GPU: x-slab tiles of one cube over the GPUs of a node          */
/* ------------------------------------------------------------------ */
/* Every (x, y) trace is independent, so a cube is split into contiguous slabs of x rows,
 * one per GPU — the split rayon makes over Axis(0) in the reference's pixel loops (math_tools.rs:333-339,
 * 545-568).  The data path needs no collective; per recompute there are two exchange steps, both RCCL calls
 * made by this library on the members' own streams (no host sync between kernels and collectives):
 *   C2  ncclAllReduce(sum) of the slabs' pixel-sum vectors (2 nf floats) -> pixel means on every member
 *   C1  grouped ncclSend / ncclRecv gather of per-pixel results to rank 0: the image always, the final
 *       trace cube / every output on request (thz_gather)
 * A group is either ONE process driving n devices — the shape of the reference, whose single data thread
 * (data_thread.rs:162-174) would own all of them — or one member of a one-process-per-GPU launch
 * (torchrun-style); the calls below are the same in both.  librccl is opened on first use of a group with
 * more than one device, not at library load. */
typedef struct thz_group thz_group;
#define THZ_GROUP_ID_BYTES 128 /* = NCCL_UNIQUE_ID_BYTES */

/* rows [*x0, *x0 + *n) of `rank`: nx / world rows each, the remainder spread over the first ranks */
int thz_host_slab(size_t nx, int world, int rank, size_t *x0, size_t *n);

/* one process, n devices (ncclCommInitAll).  Members that all name the SAME device form a group without a
 * fabric — collectives become device-local copies on that device — which is how a one-GPU box exercises
 * the slab logic; a mix of repeated and distinct devices is THZ_ERR_INVALID. */
int thz_group_create(const int *devices, int n, thz_group **out);
/* one process per GPU: rank 0 calls thz_group_unique_id and ships the THZ_GROUP_ID_BYTES to every other
 * rank by any means (a file, MPI, torch.distributed ...); every rank then calls thz_group_create_rank
 * (ncclCommInitRank; collective: returns when all `world` ranks have called it). */
int thz_group_unique_id(void *id);
int thz_group_create_rank(int device, int rank, int world, const void *id, thz_group **out);
void thz_group_destroy(thz_group *g);
const char *thz_group_last_error(const thz_group *g);
int thz_group_world(const thz_group *g);        /* ranks in the group */
int thz_group_local_count(const thz_group *g);  /* members this process drives */
int thz_group_rank(const thz_group *g, int i);  /* rank of local member i */
thz_ctx *thz_group_ctx(thz_group *g, int i);    /* context of local member i (owned by the group) */
/* C2 / C1 as stand-alone calls, for callers that drive the stage entry points themselves: d_bufs / d_send
 * hold one device pointer per LOCAL member (on that member's device); counts has one entry per RANK;
 * d_recv_root (on rank 0's device; ignored in processes that do not drive rank 0) receives the rows in
 * rank order.  Enqueued on the members' streams. */
int thz_group_all_reduce_sum(thz_group *g, float *const *d_bufs, size_t count);
int thz_group_all_reduce_u64(thz_group *g, uint64_t *const *d_bufs, size_t count);
int thz_group_gather(thz_group *g, const float *const *d_send, const size_t *counts, float *d_recv_root);
int thz_group_sync(thz_group *g); /* waits for every local member's stream */

/* what C1 brings to rank 0 (gathering everything is xGMI-bound — 6 GiB per peer at
 * 1024 x 1024 x 4096 against 14 ms of compute — the GUI reads only the small products) */
typedef enum thz_gather {
    THZ_GATHER_SMALL = 0, /* image + pixel means (what img_lock / PlotDataContainer readers need) */
    THZ_GATHER_TIME = 1,  /* + the final trace cube (the 3-D tab's input) */
    THZ_GATHER_ALL = 2    /* + spectrum, amplitudes, phases: a complete ScannedImageFilterData on rank 0 */
} thz_gather;

/* A session over a group: member i keeps slab i of the raw cube and of every output resident.  Everything a session
 * does shards (round 3): a non-zero tilt (the plan is made for the whole grid), scale_factor > 1 (a block of s x s
 * pixels whose rows lie in two slabs belongs to the slab that holds its LAST row: the slab in front hands over the
 * partial sums of its rows, the sum continues in the reference's order — THZ_ERR_UNSUPPORTED only when a slab has
 * fewer rows than the scale factor: nx / world < scale_factor while nx / scale_factor and ny / scale_factor are not 0;
 * every rank refuses before any exchange and the outputs stay those of the last recompute), want_means 2 (the
 * reference's sequential means, slab after slab on a carried running sum: bit for bit one session's, serial by
 * construction). */
typedef struct thz_group_session thz_group_session;
int thz_group_session_create(thz_group *g, size_t nx, size_t ny, size_t nt, const float *time, float dx, float dy,
                             thz_group_session **out);
void thz_group_session_destroy(thz_group_session *gs);
/* the slab session of local member i (its buffers, plot copy-out ...); rows via thz_host_slab.  Its
 * thz_session_voxels covers that slab only: the whole grid's 3-D view is thz_group_session_voxels. */
thz_session *thz_group_session_member(thz_group_session *gs, int i);
/* `cube`: the WHOLE (nx, ny, nt) host cube — each member uploads its rows — or NULL when the caller filled
 * the members' THZ_BUF_RAW itself.  Collective (C2 of the raw pixel sums). */
int thz_group_session_upload(thz_group_session *gs, const float *cube, int subtract_bias);
/* UpdateType::Filter(start_stage) on every slab + C2 + C1.  Collective; blocking. */
int thz_group_session_recompute(thz_group_session *gs, const thz_chain_cfg *cfg, int start_stage, int gather);
/* UpdateType::Filter(<Deconvolution>) over the group — BASELINE config 4's "1 -> 2 GPUs".  The stage's transform, band
 * energies and recombination are per PIXEL, its Richardson-Lucy iterations per BAND over the whole image: every member
 * runs the per-pixel parts for its own rows and the iterations for its own bands (contiguous ranges dealt out by a
 * fitted time model), and what crosses the fabric is two sets of 2-D images — n_filters x Nx x Ny energies out, as many
 * gains back (grouped ncclBroadcast) — not the cube (round 2's form gathered and all-reduced it).  The output slab stays
 * on its member; image (and the final cube, if the last recompute gathered it) are re-gathered to rank 0.  Members of
 * one process run on host threads.  A guard of the reference (the same on every rank) or an abort / error on any rank
 * (agreed by a one-float all-reduce after each part) makes every slab keep its input.  Same return codes as
 * thz_session_deconvolve.  DESIGN.md §5: expected times on 2 / 4 / 8 GPUs from measured phase times. */
int thz_group_session_deconvolve(thz_group_session *gs, const thz_psf *psf, const thz_deconv_cfg *cfg,
                                 volatile const int *abort_flag, float *progress);
/* thz_session_estimate_tilt over the whole grid of a group session, bit for bit one session's result on every rank.
 * Every member maps its own slab (its THZ_BUF_PEAK_* images); the three images go to rank 0 through the gather (the
 * int32 image as its bits); rank 0 runs the same moments kernels and the same fit on the whole-grid images; the
 * seven doubles and the count return to every rank as bit patterns through one thz_group_all_reduce_u64 to which the
 * other ranks add zeros.  Collective and blocking: every rank calls it with the same arguments. */
int thz_group_session_estimate_tilt(thz_group_session *gs, int which, int mode, float rel_threshold, thz_tilt_fit *out);
/* the gathered whole-grid maps of the last thz_group_session_estimate_tilt on rank 0's device (NULL elsewhere, or
 * before the first call): which = THZ_BUF_PEAK_INDEX / _OFFSET / _VALUE */
void *thz_group_session_peak_result(thz_group_session *gs, int which);
/* Regions of interest over the whole (nx, ny) grid (thz_session_set_rois): every slab sums its rows of the
 * whole grid's mask — the sampled row index shape0 - y - 1 (math_tools.rs:647) runs along the sharded axis —,
 * the recompute's C2 all-reduces the regions' sums with the pixel sums, and every member divides by the grid's
 * pixel count.  thz_group_session_roi reads local member 0's copy (identical on all).  Collective like the
 * recompute itself: every rank sets the same regions. */
int thz_group_session_set_rois(thz_group_session *gs, size_t n_rois, const size_t *n_vertices, const uint64_t *poly_xy);
int thz_group_session_roi(thz_group_session *gs, size_t roi, const thz_roi_out *out);
/* gathered results on rank 0's device after a recompute: THZ_BUF_IMG (nx, ny) always; THZ_BUF_DATA with
 * THZ_GATHER_TIME / ALL; THZ_BUF_FFT / AMPLITUDES / PHASES with ALL; THZ_BUF_AVG_* (on every member these
 * are also in its slab session).  NULL when absent or when this process does not drive rank 0. */
void *thz_group_session_result(thz_group_session *gs, int which);
/* the whole grid of the last recompute's outputs (thz_session_grid over all slabs): (nx, ny) of the raw grid, or
 * behind a scaling stage (nx / s, ny / s); what the gathered buffers and thz_group_session_download index */
int thz_group_session_grid(const thz_group_session *gs, size_t *nx, size_t *ny);
int thz_group_session_download(thz_group_session *gs, int which, size_t pix0, size_t npix, void *dst);

/* Plot copy-out of UpdateType::Plot (data_thread.rs:1337-1432): everything the
 * right-hand panel plots for the selected pixel, in one call.  Host pointers, any
 * may be NULL.  px, py index the (nx, ny) grid (pixel_selected / scaling). */
typedef struct thz_plot_out {
    float *signal;              /* nt      raw trace, filter_data.first()               :1344-1362 */
    float *signal_fft;          /* nf_out  amplitudes right after the fft stage         :1366-1380 */
    float *phase_fft;           /* nf_out  phases right after the fft stage                        */
    float *filtered_signal;     /* nt_out  final trace, filter_data.last()              :1384-1396 */
    float *filtered_signal_fft; /* nf_out  band-passed amplitudes                       :1398-1408 */
    float *filtered_phase_fft;  /* nf_out                                               :1409-1419 */
    float *avg_signal;          /* nt_out  pixel mean of the final cube, or — avg_in_fourier_space of the last
                                            recompute — the ifft stage's avg_data            :1422-1432 */
    float *avg_signal_fft;      /* nf_out  pixel mean of the amplitudes (needs want_means) :1434   */
    float *avg_phase_fft;       /* nf_out                                                  :1435   */
} thz_plot_out;
int thz_session_plot(thz_session *s, size_t px, size_t py, const thz_plot_out *out);

/* ConfigCommand::OpenRef (data_thread.rs:372-588): a reference pulse read from its own file
 * becomes a length-nt vector on the scan's time axis — zero-padded index shift by
 * round((scan_time[0] - ref_time[0]) / ref_dt) (:405-481) — is windowed with the *reference
 * file's* time axis (:490-515) and transformed with the scan's plan (:517-533).
 * thz_host_align_reference returns 0 (lengths and origin already match), 1 (shifted) or
 * 2 (naive pad / truncate for degenerate axes). */
int thz_host_align_reference(const float *scan_time, size_t nt, const float *ref_time, const float *ref_signal,
                             size_t nref, float *out /* nt */);
/* all host pointers; reference_out (nt) = aligned and windowed pulse (roi_data), amplitudes /
 * phases (nf) = |X| and numpy_unwrap(arg X) (roi_signal_fft / roi_phase_fft).  Plans for
 * scan_time if the context's axis differs.  THZ_ERR_INVALID where the reference panics: a
 * non-adapted window with nref != nt. */
int thz_reference_spectrum(thz_ctx *ctx, const float *scan_time, size_t nt, const float *ref_time,
                           const float *ref_signal, size_t nref, const thz_window_cfg *window,
                           float *reference_out, float *amplitudes, float *phases);

/* calculate_optical_properties (math_tools.rs:663-701): refractive index, absorption
 * coefficient and extinction coefficient per bin from sample and reference amplitude /
 * phase spectra (host vectors; f32 in the reference's operation order). */
int thz_host_optical_properties(const float *sample_amp, const float *sample_phase, const float *ref_amp,
                                const float *ref_phase, const float *freq, size_t nf, float thickness,
                                float *refractive_index, float *absorption_coeff, float *extinction_coeff);

/* ------------------------------------------------------------------ */
/* 3-D voxel envelope (gui/threed_plot.rs:80-276)                       */
/* ------------------------------------------------------------------ */
/* The data thread rebuilds the voxel instances of the 3-D tab after every
 * recompute (update_intensity_image, data_thread.rs:48-101): per trace
 * (v^2)^contrast -> 1-D Gaussian -> max / min rule; then the max_instances-th
 * largest opacity of the whole cube (select_nth_unstable_by, :205-214) becomes
 * the effective threshold and every voxel >= it becomes one instance. */
typedef struct thz_voxel_cfg {
    float opacity_threshold; /* gui_settings.opacity_threshold, application.rs:202 (0.1) */
    float contrast;          /* contrast_3d (2.0) */
    float sigma;             /* kernel_sigma (3.0) */
    int32_t radius;          /* kernel_radius (9); slider 1..50 */
} thz_voxel_cfg;

/* bevy_voxel_plot::InstanceData as filled at threed_plot.rs:260-264 */
typedef struct thz_voxel_instance {
    float position[3];
    float scale;
    float color[4]; /* linear RGB of the jet colour, alpha = opacity */
} thz_voxel_instance;

#define THZ_VOXEL_MAX_INSTANCES 2000000u /* threed_plot.rs:206 */

int thz_voxel_cfg_default(thz_voxel_cfg *out);
/* gaussian_kernel1d (:80-101); out has 2*radius+1 entries */
int thz_host_gaussian_kernel1d(float sigma, int radius, float *out);
/* d_data (npix, nt) -> d_opacity (npix, nt), nt <= 8192; the two may not alias */
int thz_voxel_opacity(thz_ctx *ctx, size_t npix, size_t nt, const float *d_data, const thz_voxel_cfg *cfg,
                      float *d_opacity);
/* Radix select, one level: d_hist (2048 u64, device) += histogram of the level's
 * bits among the n values whose higher bits equal `prefix` (level 0: 11 bits of
 * all values; level 1: next 11; level 2: last 10).  At level 0 `prefix` is a floor
 * bin instead: keys of lower bins are counted in it (0 = full histogram); if the
 * walk ends in a non-zero floor bin, level 0 is repeated with floor 0.
 * Histograms of the tiles of a cube add up, so ranks all-reduce d_hist between
 * levels. */
int thz_select_histogram(thz_ctx *ctx, const float *d_vals, size_t n, int level, uint32_t prefix,
                         uint64_t *d_hist);
/* host walk of one level: the bin holding the k-th largest (k >= 1) and its rank
 * inside the bin; nbins = 2048 (levels 0, 1) or 1024 (level 2) */
int thz_host_select_step(const uint64_t *hist, int nbins, uint64_t k, int *bin, uint64_t *k_rem);
/* value from the three bins of the levels */
float thz_host_select_value(int bin0, int bin1, int bin2);
/* the three levels on one GPU: k-th largest of n values (1 <= k <= n) */
int thz_kth_largest(thz_ctx *ctx, const float *d_vals, size_t n, uint64_t k, float *out);
/* effective threshold (:205-214): 0.0 when n <= max_instances */
int thz_voxel_threshold(thz_ctx *ctx, const float *d_opacity, size_t n, uint64_t max_instances, float *out);
/* Instance loop (:216-271) over a (gw, gh, gd) opacity cube, in x, y, z order.
 * x0 / gw_total place a tile of x-rows inside the whole grid (x0 = 0, gw_total =
 * gw for one GPU).  Writes at most `capacity` records to d_out and the number of
 * voxels >= threshold to *count; cube_dims = {cube_width, cube_height, cube_depth}. */
int thz_voxel_instances(thz_ctx *ctx, const float *d_opacity, size_t gw, size_t gh, size_t gd, size_t x0,
                        size_t gw_total, float threshold, float time_span, int scaling, size_t orig_w,
                        size_t orig_h, size_t orig_d, thz_voxel_instance *d_out, uint64_t capacity,
                        uint64_t *count, float *cube_dims);

/* update_intensity_image's 3-D part for a session (data_thread.rs:82-101): opacity cube of the
 * session's final trace cube, effective threshold, instance list — downloaded to `host_out`
 * (capacity records; NULL with capacity 0 to only count).  time_span = last - first sample of the
 * final time axis; scaling / orig_* as in thz_voxel_instances.  The opacity cube stays resident in
 * the session (THZ_BUF_OPACITY) until the next call. */
int thz_session_voxels(thz_session *s, const thz_voxel_cfg *cfg, uint64_t max_instances, int scaling,
                       size_t orig_w, size_t orig_h, size_t orig_d, thz_voxel_instance *host_out,
                       uint64_t capacity, uint64_t *count, float *threshold, float *cube_dims);
/* The same over the WHOLE grid of a group session (thz_group_session_grid), bit for bit what one session over the
 * same cube and chain gives: the same threshold, the same *count, the same first min(count, capacity) records.
 * thz_session_voxels on a group's member stays what it is: that slab alone, placed as though it were the whole grid.
 * Collective and blocking, like thz_group_session_recompute: every rank calls it with the same cfg, max_instances,
 * scaling and orig_*.  Every member computes the opacities of its slab of the final cube (the group's Deconvolution
 * stage included; resident as its THZ_BUF_OPACITY); the max_instances-th largest value of the whole grid is found
 * from all-reduced select histograms (thz_kth_largest's walk, on every rank); one all-reduce of the slabs' counts
 * places each slab's records in the whole list; the records that fit are gathered to rank 0 in rank order.
 * *count (the whole grid's), *threshold and cube_dims reach every rank; only the process that drives rank 0 receives
 * records — its `capacity` is the one that counts (NULL with 0: count only); elsewhere host_out and capacity are
 * ignored.  THZ_ERR_NOT_READY before the first recompute.  Every rank returns the same code: a failure on one rank
 * (capacity without a buffer on rank 0's process, an allocation, the opacity launch) is agreed on by an all-reduce. */
int thz_group_session_voxels(thz_group_session *gs, const thz_voxel_cfg *cfg, uint64_t max_instances, int scaling,
                             size_t orig_w, size_t orig_h, size_t orig_d, thz_voxel_instance *host_out,
                             uint64_t capacity, uint64_t *count, float *threshold, float *cube_dims);

/* Per-stage device time of the most recent call of each kind, the value the
 * reference shows next to each filter (filter.rs:607-621).  `stage` is one
 * of the THZ_STAGE_* ids. */
enum {
    THZ_STAGE_FFT = 0,
    THZ_STAGE_FD_MASK = 1,
    THZ_STAGE_IFFT = 2,
    THZ_STAGE_PIPELINE = 3,
    THZ_STAGE_TD_WINDOW = 4,
    THZ_STAGE_INTENSITY = 5,
    THZ_STAGE_MEAN = 6,
    THZ_STAGE_ROI = 7,
    THZ_STAGE_VOXEL_OPACITY = 8,
    THZ_STAGE_VOXEL_SELECT = 9,
    THZ_STAGE_VOXEL_EMIT = 10,
    THZ_STAGE_PROBE = 11,
    THZ_STAGE_PEAK = 12,
    THZ_STAGE_OPTICAL = 13,
    THZ_STAGE_ECHO = 14,
    THZ_STAGE_PCA = 15,
    THZ_STAGE_COUNT = 16
};
/* hipEvent bracketing of every stage call on the context's stream.
 *   0  off (default)
 *   1  immediate: the call waits for its kernel; thz_stage_time_ns() then
 *      returns the device time of the latest call of that stage
 *   2  deferred: events are recorded without any host wait;
 *      thz_timing_collect() later synchronises once and returns the summed
 *      device time and the number of calls of `stage` since the last collect */
int thz_enable_timing(thz_ctx *ctx, int mode);
int thz_stage_time_ns(thz_ctx *ctx, int stage, uint64_t *ns);
int thz_timing_collect(thz_ctx *ctx, int stage, uint64_t *total_ns, uint64_t *count);

/* Kernel variant actually used for the current nt ("stockham-lds-r2", …),
 * for logs and for the tests that assert the native path ran. */
const char *thz_kernel_variant(const thz_ctx *ctx);

#ifdef __cplusplus
}
#endif
#endif /* THZGPU_H */
