// unmix_host.cpp — the host side of the unmixing (include/thzgpu.h, "Unmixing every pixel into its materials"): the
// normal matrix in f64 and the twin of the device's solve, plain C++ with no GPU and no context.
#include "../../include/thzgpu.h"

#include <cmath>

extern "C" int thz_host_unmix_prepare(const float *endmembers, int K, size_t L, float *G, float *rd)
{
    if (!endmembers || !G || !rd) return THZ_ERR_INVALID;
    if (K < 1 || K > THZ_UNMIX_MAX || L < 1 || L > THZ_PCA_MAX_LEN) return THZ_ERR_INVALID;
    for (size_t i = 0; i < (size_t)K * L; ++i)
        if (!std::isfinite(endmembers[i])) return THZ_ERR_INVALID;  // before anything is written
    double g64[THZ_UNMIX_MAX][THZ_UNMIX_MAX];
    for (int i = 0; i < K; ++i)
        for (int c = 0; c < K; ++c) {
            const float *ei = endmembers + (size_t)i * L, *ec = endmembers + (size_t)c * L;
            double s = 0.0;
            for (size_t j = 0; j < L; ++j) s += (double)ei[j] * (double)ec[j];
            g64[i][c] = s;
        }
    for (int c = 0; c < K; ++c) {
        if (g64[c][c] == 0.0) return THZ_ERR_INVALID;  // a zero endmember
        if (!std::isfinite((float)(1.0 / g64[c][c]))) return THZ_ERR_INVALID;
        for (int i = 0; i < K; ++i)
            if (!std::isfinite((float)g64[i][c])) return THZ_ERR_INVALID;
    }
    for (int i = 0; i < K; ++i)
        for (int c = 0; c < K; ++c) G[i * K + c] = (float)g64[i][c];
    for (int c = 0; c < K; ++c) rd[c] = (float)(1.0 / g64[c][c]);
    return THZ_OK;
}

extern "C" int thz_host_unmix_solve(const float *b, const float *G, const float *rd, int K, int n_sweeps, float *a, float *kkt)
{
    if (!b || !G || !rd || !a) return THZ_ERR_INVALID;
    if (K < 1 || K > THZ_UNMIX_MAX || n_sweeps < 0 || n_sweeps > THZ_UNMIX_MAX_SWEEPS) return THZ_ERR_INVALID;
    float g[THZ_UNMIX_MAX];
    for (int c = 0; c < K; ++c) {
        a[c] = 0.0f;
        g[c] = -b[c];
    }
    for (int s = 0; s < n_sweeps; ++s) {
        bool moved = false;
        for (int c = 0; c < K; ++c) {
            const float an = std::fmax(std::fma(-g[c], rd[c], a[c]), 0.0f);
            const float d = an - a[c];
            moved = moved || d != 0.0f;
            for (int i = 0; i < K; ++i) g[i] = std::fma(G[i * K + c], d, g[i]);
            a[c] = an;
        }
        if (!moved) break;  // every further sweep would repeat this one
    }
    if (kkt) {
        float worst = 0.0f;
        for (int c = 0; c < K; ++c) worst = std::fmax(worst, a[c] > 0.0f ? std::fabs(g[c]) : std::fmax(-g[c], 0.0f));
        *kkt = worst;
    }
    return THZ_OK;
}
