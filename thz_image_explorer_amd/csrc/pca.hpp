// pca.hpp — K19 principal components: the launches of pca.hip
#pragma once
#include <hip/hip_runtime.h>

#include <stddef.h>
#include <stdint.h>

namespace thz {

// the (npix x L) matrix every PCA kernel reads: X[p, j] = x[p * row_stride + j * col_step] (include/thzgpu.h,
// "Principal components of a scan"); mask: npix bytes or null
struct PcaView {
    const float *x;
    size_t npix;
    int L;
    size_t row_stride, col_step;
    const uint8_t *mask;
};

// Column sums over the unmasked pixels and their number, in f64.  ws (pca_sums_ws_bytes) comes back with the L sums
// and, as entry L, the count (a sum of ones: exact) in its first L + 1 doubles.
size_t pca_sums_ws_bytes(size_t npix, int L);
void launch_pca_sums(hipStream_t st, const PcaView &v, void *ws);

// Gram matrix of a = X - mu over the unmasked pixels.  ws (pca_gram_ws_bytes) = [G: L x L doubles | mu: 512 floats |
// the slabs' partial tiles]; the caller has put mu (zeros for none: x - 0 is x,
// bit for bit) at pca_gram_mu_offset before the launch, G is the result.
size_t pca_gram_ws_bytes(size_t npix, int L);
size_t pca_gram_mu_offset(int L);
void launch_pca_gram(hipStream_t st, const PcaView &v, void *ws);

// scores[c * npix + p] = sum_j (X[p, j] - mu[j]) V[c * L + j], c < K <= 8, for every pixel (the mask is not read).
// d_tab = [mu: L floats (zeros when there is none) | V: K x L floats] on the device
void launch_pca_scores(hipStream_t st, const PcaView &v, const float *d_tab, int K, float *scores);

}  // namespace thz
