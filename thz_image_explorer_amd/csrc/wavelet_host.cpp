// wavelet_host.cpp — wavelet shrinkage of ONE host vector (include/thzgpu.h, "Denoising every trace"): plain C++, no GPU
// and no context, with the chains of wavelet.hip — every sum one fmaf chain from +0 over ascending k.  Also the
// Daubechies filters and the universal thresholds.  Built with -ffp-contract=off.
#include "../../include/thzgpu.h"

#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

// declared in wavelet.hpp, which this unit leaves out: it builds without the HIP headers
const char *wavelet_cfg_error(const thz_wavelet_cfg *cfg, size_t nt, const float *hn, const float *gn, const float *scale);

const char *wavelet_cfg_error(const thz_wavelet_cfg *cfg, size_t nt, const float *hn, const float *gn, const float *scale)
{
    if (nt == 0 || nt > THZ_WAVELET_MAX_NT) return "1 <= nt <= THZ_WAVELET_MAX_NT";
    if (cfg->n_taps < 1 || cfg->n_taps > THZ_WAVELET_MAX_TAPS) return "1 <= n_taps <= THZ_WAVELET_MAX_TAPS";
    if (cfg->n_levels < 1 || cfg->n_levels > THZ_WAVELET_MAX_LEVELS) return "1 <= n_levels <= THZ_WAVELET_MAX_LEVELS";
    if ((size_t)(cfg->n_levels + 2) * nt > THZ_WAVELET_MAX_WORDS) return "(n_levels + 2) * nt <= THZ_WAVELET_MAX_WORDS";
    if (cfg->shrink != 0 && cfg->shrink != 1) return "shrink is 0 or 1";
    if (cfg->noise_mode != 0 && cfg->noise_mode != 1) return "noise_mode is 0 or 1";
    for (int k = 0; k < cfg->n_taps; ++k)
        if (!std::isfinite(hn[k]) || !std::isfinite(gn[k])) return "every tap is finite";
    for (int j = 0; j < cfg->n_levels; ++j)
        if (!(std::isfinite(scale[j]) && scale[j] >= 0.0f)) return "every scale is finite and >= 0";
    return nullptr;
}

namespace {

float shrink(float d, float th, int hard)
{
    if (hard) return std::fabs(d) > th ? d : 0.0f;
    const float t = std::fabs(d) - th;
    return t > 0.0f ? std::copysign(t, d) : 0.0f;
}

// The orthonormal Daubechies scaling filters, minimum phase (sum h = sqrt 2, sum h[k] h[k + 2m] = delta_m)
const double kDb1[2] = {0.7071067811865476, 0.7071067811865476};
const double kDb2[4] = {0.48296291314453416, 0.8365163037378078, 0.2241438680420134, -0.12940952255126037};
const double kDb3[6] = {0.3326705529500826, 0.8068915093110924, 0.4598775021184915, -0.1350110200102546,
                        -0.08544127388202669, 0.035226291885709526};
const double kDb4[8] = {0.23037781330889645, 0.7148465705529156, 0.630880767929859, -0.02798376941685959,
                        -0.18703481171909309, 0.03084138183556063, 0.03288301166688517, -0.010597401785069018};
const double *const kDb[4] = {kDb1, kDb2, kDb3, kDb4};

}  // namespace

extern "C" {

int thz_host_wavelet_trace(const float *y, size_t nt_, const float *hn, const float *gn, const float *scale,
                           const thz_wavelet_cfg *cfg, float *x, float *sigma, int32_t *kept)
{
    if (!y || !hn || !gn || !scale || !cfg || !x) return THZ_ERR_INVALID;
    if (wavelet_cfg_error(cfg, nt_, hn, gn, scale)) return THZ_ERR_INVALID;
    const int nt = (int)nt_, J = cfg->n_levels, Lf = cfg->n_taps;
    std::vector<float> a(y, y + nt), an((size_t)nt), d((size_t)J * (size_t)nt);
    float m = 0.0f;
    int32_t count = 0;
    for (int j = 1; j <= J; ++j) {
        float *dj = d.data() + (size_t)(j - 1) * (size_t)nt;
        const int step = (int)((1u << (j - 1)) % (unsigned)nt);
        for (int i = 0; i < nt; ++i) {
            float ah = 0.0f, ag = 0.0f;
            int idx = i;
            for (int k = 0; k < Lf; ++k) {
                ah = std::fmaf(hn[k], a[(size_t)idx], ah);
                ag = std::fmaf(gn[k], a[(size_t)idx], ag);
                idx += step;
                idx = idx >= nt ? idx - nt : idx;
            }
            an[(size_t)i] = ah;
            dj[i] = ag;
        }
        a.swap(an);
        if (j == 1) {
            // the order statistic on the bit patterns of |d_1|: the order of the values for everything that is not NaN,
            // and a total order for what is
            std::vector<uint32_t> bits((size_t)nt);
            for (int i = 0; i < nt; ++i) {
                std::memcpy(&bits[(size_t)i], &dj[i], sizeof(uint32_t));
                bits[(size_t)i] &= 0x7fffffffu;
            }
            std::nth_element(bits.begin(), bits.begin() + (nt - 1) / 2, bits.end());
            std::memcpy(&m, &bits[(size_t)((nt - 1) / 2)], sizeof(float));
        }
        const float th = cfg->noise_mode ? scale[j - 1] : scale[j - 1] * m;
        for (int i = 0; i < nt; ++i) {
            dj[i] = shrink(dj[i], th, cfg->shrink);
            count += dj[i] != 0.0f;
        }
    }
    for (int j = J; j >= 1; --j) {
        const float *dj = d.data() + (size_t)(j - 1) * (size_t)nt;
        const int step = (int)((1u << (j - 1)) % (unsigned)nt);
        for (int i = 0; i < nt; ++i) {
            float ch = 0.0f, cg = 0.0f;
            int idx = i;
            for (int k = 0; k < Lf; ++k) {
                ch = std::fmaf(hn[k], a[(size_t)idx], ch);
                cg = std::fmaf(gn[k], dj[idx], cg);
                idx -= step;
                idx = idx < 0 ? idx + nt : idx;
            }
            an[(size_t)i] = ch + cg;
        }
        a.swap(an);
    }
    for (int i = 0; i < nt; ++i) x[i] = a[(size_t)i];  // y and x may be the same vector
    if (sigma) *sigma = m;
    if (kept) *kept = count;
    return THZ_OK;
}

int thz_host_wavelet_filter(int order, float *hn, float *gn, int *n_taps)
{
    if (!hn || !gn || !n_taps || order < 1 || order > 4) return THZ_ERR_INVALID;
    const int Lf = 2 * order;
    const double *h = kDb[order - 1];
    const double root2 = std::sqrt(2.0);
    for (int k = 0; k < Lf; ++k) {
        hn[k] = (float)(h[k] / root2);
        gn[k] = (float)((k & 1 ? -1.0 : 1.0) * h[Lf - 1 - k] / root2);
    }
    *n_taps = Lf;
    return THZ_OK;
}

int thz_host_wavelet_universal(size_t nt, int n_levels, float *scale)
{
    if (!scale || nt == 0 || n_levels < 1 || n_levels > THZ_WAVELET_MAX_LEVELS) return THZ_ERR_INVALID;
    const double lead = std::sqrt(2.0) / 0.6744897501960817 * std::sqrt(2.0 * std::log((double)nt));
    for (int j = 1; j <= n_levels; ++j) scale[j - 1] = (float)(lead * std::pow(2.0, -0.5 * (double)j));
    return THZ_OK;
}

}  // extern "C"
