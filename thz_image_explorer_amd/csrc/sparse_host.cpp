// sparse_host.cpp — sparse deconvolution of ONE host vector (include/thzgpu.h, "Sparse deconvolution"): plain C++, no GPU
// and no context, with the chains of sparse.hip — every sum one fmaf chain from +0 in ascending order of the sample it
// reads, terms outside the taps or the trace skipped.  Also the taps and step a reference pulse gives, and the momentum
// table both sides use.  Built with -ffp-contract=off.
#include "sparse.hpp"
#include "../../include/thzgpu.h"

#include <cmath>
#include <vector>

namespace thz {

void sparse_momentum(int n_iter, float *beta)
{
    double t = 1.0;
    for (int n = 0; n < n_iter; ++n) {
        const double t1 = (1.0 + std::sqrt(1.0 + 4.0 * t * t)) / 2.0;
        beta[n] = (float)((t - 1.0) / t1);
        t = t1;
    }
}

}  // namespace thz

const char *sparse_cfg_error(const thz_sparse_cfg *cfg, size_t nt, const float *taps)
{
    if (nt == 0 || nt > THZ_SPARSE_MAX_NT) return "1 <= nt <= THZ_SPARSE_MAX_NT";
    if (cfg->n_taps < 1 || cfg->n_taps > THZ_SPARSE_MAX_TAPS) return "1 <= n_taps <= THZ_SPARSE_MAX_TAPS";
    if (cfg->center < 0 || cfg->center >= cfg->n_taps) return "0 <= center < n_taps";
    if (cfg->n_iter < 0 || cfg->n_iter > THZ_SPARSE_MAX_ITER) return "0 <= n_iter <= THZ_SPARSE_MAX_ITER";
    if (cfg->accelerate != 0 && cfg->accelerate != 1) return "accelerate is 0 or 1";
    if (!(std::isfinite(cfg->step) && cfg->step > 0.0f)) return "step is finite and > 0";
    if (!(std::isfinite(cfg->rel_lambda) && cfg->rel_lambda >= 0.0f)) return "rel_lambda is finite and >= 0";
    if (!(std::isfinite(cfg->min_lambda) && cfg->min_lambda >= 0.0f)) return "min_lambda is finite and >= 0";
    for (int k = 0; k < cfg->n_taps; ++k)
        if (!std::isfinite(taps[k])) return "every tap is finite";
    return nullptr;
}

namespace {

// out[i] = sum over m of h[i + c - m] v[m], ascending m
void apply_h(const float *h, int P, int c, const float *v, int nt, float *out)
{
    for (int i = 0; i < nt; ++i) {
        const int lo = i + c - (P - 1) > 0 ? i + c - (P - 1) : 0, hi = i + c < nt - 1 ? i + c : nt - 1;
        float acc = 0.0f;
        for (int m = lo; m <= hi; ++m) acc = std::fmaf(h[i + c - m], v[m], acc);
        out[i] = acc;
    }
}

// out[j] = sum over i of h[i + c - j] v[i], ascending i
void apply_ht(const float *h, int P, int c, const float *v, int nt, float *out)
{
    for (int j = 0; j < nt; ++j) {
        const int lo = j - c > 0 ? j - c : 0, hi = j - c + P - 1 < nt - 1 ? j - c + P - 1 : nt - 1;
        float acc = 0.0f;
        for (int i = lo; i <= hi; ++i) acc = std::fmaf(h[i + c - j], v[i], acc);
        out[j] = acc;
    }
}

}  // namespace

extern "C" {

int thz_host_sparse_trace(const float *y, size_t nt_, const float *taps, const thz_sparse_cfg *cfg, float *x, float *resid,
                          int32_t *nnz)
{
    if (!y || !taps || !cfg || !x) return THZ_ERR_INVALID;
    if (sparse_cfg_error(cfg, nt_, taps)) return THZ_ERR_INVALID;
    const int nt = (int)nt_, P = cfg->n_taps, c = cfg->center;
    std::vector<float> beta((size_t)cfg->n_iter + 1), z((size_t)nt, 0.0f), r((size_t)nt), g((size_t)nt), xs((size_t)nt, 0.0f);
    thz::sparse_momentum(cfg->n_iter, beta.data());
    apply_ht(taps, P, c, y, nt, g.data());
    float gmax = 0.0f;
    for (int j = 0; j < nt; ++j) gmax = std::fmax(gmax, std::fabs(g[(size_t)j]));
    const float lam = std::fmax(cfg->rel_lambda * gmax, cfg->min_lambda);
    const float th = cfg->step * lam;
    for (int n = 0; n < cfg->n_iter; ++n) {
        apply_h(taps, P, c, z.data(), nt, r.data());
        for (int i = 0; i < nt; ++i) r[(size_t)i] = y[i] - r[(size_t)i];
        apply_ht(taps, P, c, r.data(), nt, g.data());
        for (int j = 0; j < nt; ++j) {
            const float v = std::fmaf(cfg->step, g[(size_t)j], z[(size_t)j]);
            const float a = std::fabs(v) - th;
            const float xn = a > 0.0f ? std::copysign(a, v) : 0.0f;
            z[(size_t)j] = cfg->accelerate ? std::fmaf(beta[(size_t)n], xn - xs[(size_t)j], xn) : xn;
            xs[(size_t)j] = xn;
        }
    }
    if (resid) {
        apply_h(taps, P, c, xs.data(), nt, r.data());
        float s = 0.0f;
        for (int i = 0; i < nt; ++i) {
            const float d = y[i] - r[(size_t)i];
            s = std::fmaf(d, d, s);
        }
        *resid = s;
    }
    int32_t count = 0;
    for (int i = 0; i < nt; ++i) {
        x[i] = xs[(size_t)i];  // y and x may be the same vector
        count += xs[(size_t)i] != 0.0f;
    }
    if (nnz) *nnz = count;
    return THZ_OK;
}

int thz_host_sparse_kernel(const float *ref, size_t nref, int n_taps, int center, float *taps, float *step)
{
    if (!ref || !taps || !step || nref == 0 || n_taps < 1 || n_taps > THZ_SPARSE_MAX_TAPS || center < 0 || center >= n_taps)
        return THZ_ERR_INVALID;
    // the largest |ref|, the lowest index on ties: thz_host_echo_trace's rank 0 in mode 0
    size_t k0 = 0;
    float best = -INFINITY;
    for (size_t i = 0; i < nref; ++i) {
        const float key = std::fabs(ref[i]);
        if (key > best) {
            best = key;
            k0 = i;
        }
    }
    double sum = 0.0;
    bool finite = true;
    for (int k = 0; k < n_taps; ++k) {
        const long long at = (long long)k0 - center + k;
        const float v = (at >= 0 && at < (long long)nref) ? ref[at] : 0.0f;
        finite = finite && std::isfinite(v);
        sum += std::fabs((double)v);
    }
    if (!finite || !(sum > 0.0)) return THZ_ERR_INVALID;  // before anything is written
    for (int k = 0; k < n_taps; ++k) {
        const long long at = (long long)k0 - center + k;
        taps[k] = (at >= 0 && at < (long long)nref) ? ref[at] : 0.0f;
    }
    *step = (float)(1.0 / (sum * sum));
    return THZ_OK;
}

}  // extern "C"
