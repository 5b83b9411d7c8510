// optical.hip — K17: refractive index, absorption and extinction per pixel, as means over bands of bins, from the
// amplitudes and unwrapped phases a recompute leaves resident.
//
//   k_optical_map     one wave per pixel, one launch for everything:
//                     1. anchor: the least-squares line through (phase - reference phase) over the anchor's bins, in
//                        double; its intercept at bin 0 names the multiple of 2 pi this pixel's unwrap picked up in
//                        the noise below the band, which is taken off the phases again
//                     2. bands: calculate_optical_properties (math_tools.rs:663-701) per bin in the reference's f32
//                        operation order, added per band
//                     Only the anchor's and the bands' bins of a row are read; bins that both passes (or two bands)
//                     read come from the cache the second time, the wave has just had them.
//
// Built with -ffp-contract=off: every per-bin value is the f32 formula as written, one rounding per operation.
#include "optical.hpp"
#include "kernels.hpp"
#include "thz_device.hpp"

#include <math.h>

namespace thz {

namespace {

constexpr float kLightSpeed = 2.99792458e8f;
constexpr float kPiF = 3.14159274101257324219f;  // std::f32::consts::PI
constexpr double kTwoPi = 6.283185307179586476925;

// every lane the same sum: a + b = b + a at each step of the butterfly
__device__ __forceinline__ double wave_sum_f64(double v)
{
    for (int m = 1; m < kWave; m <<= 1) v += __shfl_xor(v, m, kWave);
    return v;
}

}  // namespace

// Lane l takes the bins k0 + l, k0 + l + 64, ... of a range as dword loads, in ascending order.  Measured against whole
// quads per lane (16-byte loads on 4-byte alignment; profiles/optical_map_timing.txt): the kernel is bound by the
// divisions and the logarithm, not by its loads, and a band of 35 bins keeps 35 lanes busy this way but only 9 as quads.
__global__ __launch_bounds__(256) void k_optical_map(size_t npix, int nf, const float *__restrict__ amp,
                                                     const float *__restrict__ phase, const float *__restrict__ tab,
                                                     OpticalGeom g, const float *__restrict__ thick,
                                                     float *__restrict__ out_n, float *__restrict__ out_alpha,
                                                     float *__restrict__ out_kappa, int *__restrict__ wraps,
                                                     float *__restrict__ slope)
{
    const int lane = lane_id();
    const int wib = (int)(threadIdx.x >> 6);
    const int wpb = (int)(blockDim.x >> 6);
    const float *t_pr = tab, *t_om = tab + nf, *t_ar = tab + 2 * (size_t)nf, *t_fp = tab + 3 * (size_t)nf;
    // the anchor's abscissae about their centre: sum (k - c) = 0 and sum (k - c)^2 = n (n^2 - 1) / 12
    const int a0 = (int)g.a0, a1 = (int)g.a1;
    const double na = (double)(a1 - a0);
    const double centre = (double)a0 + 0.5 * (na - 1.0);
    const double skk = na * (na * na - 1.0) / 12.0;
    const bool want_bands = out_n || out_alpha || out_kappa;
    for (size_t p = (size_t)blockIdx.x * wpb + wib; p < npix; p += (size_t)gridDim.x * wpb) {
        const float *A = amp + p * (size_t)nf, *P = phase + p * (size_t)nf;
        double m = 0.0, s = 0.0;
        if (a1 > a0) {
            double s0 = 0.0, s1 = 0.0;
            for (int k = a0 + lane; k < a1; k += kWave) {
                const double delta = (double)P[k] - (double)t_pr[k];
                s0 += delta;
                s1 += ((double)k - centre) * delta;
            }
            s0 = wave_sum_f64(s0);
            s1 = wave_sum_f64(s1);
            s = s1 / skk;
            const double b = s0 / na - s * centre;  // the line at bin 0
            m = isfinite(b) ? rint(b / kTwoPi) + 0.0 : 0.0;  // (an integer: -0 is 0, so that w is +0)
        }
        const float w = (float)(m * kTwoPi);
        if (lane == 0) {
            // (a count beyond int32 — phases of 1e10 rad — saturates)
            if (wraps) wraps[p] = m >= 2147483647.0 ? 2147483647 : (m <= -2147483648.0 ? (int)(-2147483647 - 1) : (int)m);
            if (slope) slope[p] = (float)s;
        }
        if (!want_bands) continue;
        const float d = thick ? thick[p] : g.thickness;
        const float m2d = -2.0f / d;
        for (int b = 0; b < (int)g.n_bands; ++b) {
            const int k0 = (int)g.k0[b], k1 = (int)g.k1[b];
            float sn = 0.0f, sa = 0.0f, sk = 0.0f;
            for (int k = k0 + lane; k < k1; k += kWave) {
                const float delta_phi = (P[k] - w) - t_pr[k];
                const float n = 1.0f + kLightSpeed * delta_phi / (t_om[k] * d);
                const float a = fmaxf(A[k], 1e-12f);
                const float n_safe = fmaxf(n, 1e-6f);
                const float np1 = n_safe + 1.0f;
                const float alpha = m2d * logf((np1 * np1) / (4.0f * n_safe) * a / t_ar[k]);
                const float kappa = alpha * kLightSpeed / t_fp[k];
                sn += n;
                sa += alpha;
                sk += kappa;
            }
            // lanes as a fixed tree, then the mean: the order depends on k0 and k1 alone
            sn = wave_reduce_add(sn);
            sa = wave_reduce_add(sa);
            sk = wave_reduce_add(sk);
            if (lane == 0) {
                const float nb = (float)(k1 - k0);
                const size_t o = (size_t)b * npix + p;
                if (out_n) out_n[o] = sn / nb;
                if (out_alpha) out_alpha[o] = sa / nb;
                if (out_kappa) out_kappa[o] = sk / nb;
            }
        }
    }
}

size_t optical_table_floats(size_t nf) { return 4 * nf; }

void optical_tables(const float *ref_amp, const float *ref_phase, const float *freq, size_t nf, float *tab)
{
    for (size_t k = 0; k < nf; ++k) {
        const float frequency_hz = freq[k] * 1.0e12f;
        tab[k] = ref_phase[k];
        tab[nf + k] = 2.0f * kPiF * frequency_hz;
        tab[2 * nf + k] = fmaxf(ref_amp[k], 1e-12f);
        tab[3 * nf + k] = 4.0f * kPiF * frequency_hz;
    }
}

void launch_optical_map(hipStream_t st, size_t npix, int nf, const float *amp, const float *phase, const float *d_tab,
                        const OpticalGeom &geom, const float *d_thickness, float *n, float *alpha, float *kappa,
                        int32_t *wraps, float *slope)
{
    const size_t blocks = (npix * kWave + 255) / 256;
    const unsigned grid = (unsigned)(blocks < 1 ? 1 : (blocks > (size_t)kNumCU * 8 ? (size_t)kNumCU * 8 : blocks));
    THZ_LAUNCH(k_optical_map, grid, 256, 0, st, npix, nf, amp, phase, d_tab, geom, d_thickness, n, alpha, kappa, wraps, slope);
}

}  // namespace thz
