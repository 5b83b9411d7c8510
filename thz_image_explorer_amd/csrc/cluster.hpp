// cluster.hpp — K20 k-means of the pixels of a scan: the launches of cluster.hip
#pragma once
#include "pca.hpp"

namespace thz {

// The workspace of one step.  `out` is what the host reads back in one copy: K rows of L + 1 doubles (the cluster's
// column sums, then its count — a sum of ones: exact), the inertia, the farthest pixel's index as a double (exact below
// 2^53; npix for none), and behind them `changed` as one 64-bit integer.  `cent` takes the K x L centroids before the
// launch; the caller sets *changed to zero.
struct ClusterWs {
    double *out;
    unsigned long long *changed;
    float *cent;
    double *psum, *pstat;  // the slabs' partials
    size_t bytes;
};
ClusterWs cluster_ws(void *ws, size_t npix, int L, int K);
inline size_t cluster_out_words(int L, int K) { return (size_t)K * (size_t)(L + 1) + 3; }

// One step on the view v (pca.hpp): every pixel's label (the lowest c with the smallest dist2, -1 when every distance
// is NaN) and dist2 — label is read before it is written, for the count of changes — then the per-cluster sums, counts,
// inertia and farthest pixel over the unmasked pixels with label >= 0, slab partials added in slab order.
void launch_cluster_step(hipStream_t st, const PcaView &v, int K, const ClusterWs &w, int32_t *label, float *dist2);

// out[j] = X[pixel, j], j < L
void launch_cluster_row(hipStream_t st, const PcaView &v, size_t pixel, float *out);

}  // namespace thz
