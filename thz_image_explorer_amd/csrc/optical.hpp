// optical.hpp — K17 optical-property maps: the launch of optical.hip
#pragma once
#include <hip/hip_runtime.h>

#include <stddef.h>
#include <stdint.h>

namespace thz {

constexpr int kOpticalMaxBands = 8;  // THZ_OPTICAL_MAX_BANDS

// what the kernel needs of a thz_optical_cfg, by value
struct OpticalGeom {
    float thickness;
    uint32_t a0, a1;  // anchor [a0, a1); a0 == a1: off
    uint32_t n_bands;
    uint32_t k0[kOpticalMaxBands], k1[kOpticalMaxBands];
};

// The per-bin factors that do not depend on the pixel, nf floats each, in the reference's f32 operation order:
//   [ref_phase | omega = (2 pi_f) f_hz | amp_ref = fmax(ref_amp, 1e-12) | four_pi_f = (4 pi_f) f_hz],  f_hz = f 1e12
size_t optical_table_floats(size_t nf);
void optical_tables(const float *ref_amp, const float *ref_phase, const float *freq, size_t nf, float *tab);

// per pixel of (npix, nf) amplitudes / phases: anchor (wraps, slope) and the bands' means of n, alpha, kappa
// ((n_bands, npix) each); d_tab: optical_tables() on the device; d_thickness: npix floats or null (geom.thickness);
// any output may be null
void launch_optical_map(hipStream_t st, size_t npix, int nf, const float *amp, const float *phase, const float *d_tab,
                        const OpticalGeom &geom, const float *d_thickness, float *n, float *alpha, float *kappa,
                        int32_t *wraps, float *slope);

}  // namespace thz
