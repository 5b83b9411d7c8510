// tilt_fit_host.cpp — thz_host_arrival_plane_fit: the least-squares plane through the pulse arrival times, from the ten
// sums thz_arrival_plane_moments leaves (include/thzgpu.h, "Pulse arrival times").  Host only, O(1), double.
//
// The 3 x 3 normal equations
//     | S1  Su  Sv  | | t0 |   | St  |
//     | Su  Suu Suv | | a  | = | Sut |
//     | Sv  Suv Svv | | b  |   | Svt |
// are solved by eliminating t0 first (the Schur complement of S1: the moments about the participating pixels' centre),
// which leaves a 2 x 2 system in the slopes whose determinant says whether the pixels span a plane at all.
#include "../../include/thzgpu.h"

#include <cmath>
#include <cstring>

extern "C" int thz_host_arrival_plane_fit(const double *m, thz_tilt_fit *out)
{
    if (!m || !out) return THZ_ERR_INVALID;
    std::memset(out, 0, sizeof(*out));
    const double n = m[0];
    if (!(n >= 3.0)) return THZ_SKIPPED;
    for (int q = 0; q < 10; ++q)
        if (!std::isfinite(m[q])) return THZ_SKIPPED;
    const double ub = m[1] / n, vb = m[2] / n, tb = m[6] / n;
    const double cuu = m[3] - m[1] * ub, cuv = m[4] - m[1] * vb, cvv = m[5] - m[2] * vb;
    const double cut = m[7] - m[1] * tb, cvt = m[8] - m[2] * tb, ctt = m[9] - m[6] * tb;
    const double det = cuu * cvv - cuv * cuv;
    // Pixels on one line make the determinant zero in exact arithmetic; what the roundings of the sums leave of it is
    // some 1e-16 of the product of the two variances.  A grid of two rows by two columns keeps det = cuu cvv.
    if (!(cuu > 0.0 && cvv > 0.0 && det > 1e-10 * cuu * cvv)) return THZ_SKIPPED;
    const double a = (cut * cvv - cvt * cuv) / det, b = (cvt * cuu - cut * cuv) / det;
    const double rss = ctt - a * cut - b * cvt;
    constexpr double c_mm_per_ps = 0.299792458, deg = 180.0 / 3.14159265358979323846;
    out->slope_x_ps_per_mm = a;
    out->slope_y_ps_per_mm = b;
    out->tilt_x_deg = -a * c_mm_per_ps * deg;
    out->tilt_y_deg = -b * c_mm_per_ps * deg;
    out->t0_ps = tb - a * ub - b * vb;
    out->rms_ps = rss > 0.0 ? std::sqrt(rss / n) : 0.0;
    out->n_used = (uint64_t)n;
    return THZ_OK;
}
