// cluster_host.cpp — the centroid update of k-means (include/thzgpu.h, "Segmenting a scan into materials"): plain C++ in
// f64, no GPU and no context.
#include "../../include/thzgpu.h"

#include <cmath>
#include <cstring>

extern "C" int thz_host_cluster_update(const double *sums, const uint64_t *counts, int K, size_t L, const float *previous,
                                       float *centroids)
{
    if (!sums || !counts || !previous || !centroids) return THZ_ERR_INVALID;
    if (K < 1 || K > THZ_CLUSTER_MAX || L < 1 || L > THZ_PCA_MAX_LEN) return THZ_ERR_INVALID;
    for (int c = 0; c < K; ++c)
        for (size_t j = 0; j < L; ++j)
            if (!std::isfinite(sums[(size_t)c * L + j])) return THZ_ERR_INVALID;  // before anything is written
    for (int c = 0; c < K; ++c) {
        float *dst = centroids + (size_t)c * L;
        if (!counts[c]) {  // an empty cluster stays where it is
            if (dst != previous + (size_t)c * L) std::memmove(dst, previous + (size_t)c * L, L * sizeof(float));
            continue;
        }
        const double n = (double)counts[c];
        for (size_t j = 0; j < L; ++j) dst[j] = (float)(sums[(size_t)c * L + j] / n);
    }
    return THZ_OK;
}
