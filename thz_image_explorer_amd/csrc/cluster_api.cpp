// cluster_api.cpp — k-means of the pixels of a scan (include/thzgpu.h, "Segmenting a scan into materials"): the stage
// entry point over cluster.hip and the session forms.  The centroid update is cluster_host.cpp's.
#include "session.hpp"
#include "cluster.hpp"

#include <cstring>

using namespace thz;

namespace {

// what `which` and cfg name: the matrices of the PCA calls, and the score images of the last PCA call
int cluster_matrix(thz_session *s, int which, const thz_cluster_cfg *cfg, SessionMatrix *m)
{
    thz_ctx *ctx = s->ctx;
    if (which != THZ_BUF_PCA_SCORES) {
        thz_pca_cfg columns{};
        columns.first = cfg->first;
        columns.count = cfg->count;
        columns.step = cfg->step;
        return session_matrix(s, which, &columns, "k-means", m);
    }
    // the resident [scores: (K, npix) | components: (K, L) | mean: L]
    const ResidentMaps &pca = s->maps[kMapPca];
    const size_t L = pca.entries(2), K = L ? pca.entries(1) / L : 0, npix = K ? pca.entries(0) / K : 0;
    if (!npix) return fail(ctx, THZ_ERR_NOT_READY, "k-means: no principal components have been taken");
    if (cfg->count < 1 || cfg->count > THZ_PCA_MAX_LEN || cfg->step < 1
        || (uint64_t)cfg->first + (uint64_t)(cfg->count - 1) * (uint64_t)cfg->step >= (uint64_t)K)
        return fail(ctx, THZ_ERR_INVALID, "k-means: count >= 1, step >= 1, and the last component inside the " + std::to_string(K)
                                              + " of the last PCA call");
    // (component, pixel), component-major: a pixel's row has its values npix apart
    m->d = pca.ptr(0) + (size_t)cfg->first * npix;
    m->npix = npix;
    m->L = cfg->count;
    m->row_stride = 1;
    m->col_step = (size_t)cfg->step * npix;
    return THZ_OK;
}

bool bad_k(const thz_cluster_cfg *cfg) { return cfg->n_clusters < 1 || cfg->n_clusters > THZ_CLUSTER_MAX; }

// One step on the session's resident labels and distances; `centroids` (K x L) become the resident centroids.
// [labels: npix | dist2: npix | centroids: (K, L)], the block sized for THZ_CLUSTER_MAX x THZ_PCA_MAX_LEN centroids so that
// the steps of one run never move it
int session_step(thz_session *s, const SessionMatrix &m, const uint8_t *d_mask, const float *centroids, int K, bool reset, double *sums,
                 uint64_t *counts, double *inertia, uint64_t *changed, uint64_t *farthest)
{
    thz_ctx *ctx = s->ctx;
    ResidentMaps &r = s->maps[kMapCluster];
    if (r.entries(0) != m.npix) reset = true;  // no labels of this many pixels are resident
    if (int rc = maps_begin(ctx, &r, {{m.npix}, {m.npix}, {(size_t)K * m.L}}, 2 * m.npix + (size_t)THZ_CLUSTER_MAX * THZ_PCA_MAX_LEN))
        return rc;
    if (reset && m.npix) HIP_TRY(ctx, hipMemsetAsync(r.ptr(0), 0xff, m.npix * sizeof(int32_t), ctx->stream));
    if (int rc = thz_cluster_step(ctx, m.npix, m.L, m.d, m.row_stride, m.col_step, d_mask, centroids, K, r.ptr<int32_t>(0), r.ptr(1), sums,
                                  counts, inertia, changed, farthest))
        return rc;
    if (int rc = thz_memcpy_h2d(ctx, r.ptr(2), centroids, (size_t)K * m.L * sizeof(float))) return rc;
    return maps_commit(ctx, &r);
}

// a run that cannot go on after some of its steps: their labels are no result
int unfinished(thz_session *s, const char *why)
{
    s->maps[kMapCluster].resident = false;
    return fail(s->ctx, THZ_ERR_INVALID, why);
}

int fetch_row(thz_ctx *ctx, const SessionMatrix &m, size_t pixel, float *row)
{
    if (int rc = ensure_ws(ctx, m.L * sizeof(float))) return rc;
    launch_cluster_row(ctx->stream, PcaView{m.d, m.npix, (int)m.L, m.row_stride, m.col_step, nullptr}, pixel, ctx->ws.as<float>());
    if (int rc = check_launch(ctx)) return rc;
    return thz_memcpy_d2h(ctx, row, ctx->ws, m.L * sizeof(float));
}

}  // namespace

extern "C" {

int thz_cluster_step(thz_ctx *ctx, size_t npix, size_t L, const float *d_x, size_t row_stride, size_t col_step, const uint8_t *d_mask,
                     const float *centroids, int K, int32_t *d_label, float *d_dist2, double *sums, uint64_t *counts, double *inertia,
                     uint64_t *changed, uint64_t *farthest)
{
    if (!ctx) return THZ_ERR_INVALID;
    if (int rc = use_device(ctx)) return rc;
    if (!centroids || !d_label || !d_dist2 || !counts || !inertia || !changed || !farthest)
        return fail(ctx, THZ_ERR_INVALID, "thz_cluster_step: a required pointer is NULL");
    if (const char *why = pca_view_error(L, d_x, row_stride, col_step)) return fail(ctx, THZ_ERR_INVALID, std::string("thz_cluster_step: ") + why);
    if (K < 1 || K > THZ_CLUSTER_MAX) return fail(ctx, THZ_ERR_INVALID, "thz_cluster_step: 1 <= K <= THZ_CLUSTER_MAX");
    if (sums) std::memset(sums, 0, (size_t)K * L * sizeof(double));
    std::memset(counts, 0, (size_t)K * sizeof(uint64_t));
    *inertia = 0.0;
    *changed = 0;
    *farthest = npix;
    if (npix == 0) return THZ_OK;
    const PcaView v{d_x, npix, (int)L, row_stride, col_step, d_mask};
    if (int rc = ensure_ws(ctx, cluster_ws(nullptr, npix, (int)L, K).bytes)) return rc;
    const ClusterWs w = cluster_ws(ctx->ws, npix, (int)L, K);
    if (int rc = thz_memcpy_h2d(ctx, w.cent, centroids, (size_t)K * L * sizeof(float))) return rc;
    HIP_TRY(ctx, hipMemsetAsync(w.changed, 0, sizeof(unsigned long long), ctx->stream));
    {
        StageTimer t(ctx, THZ_STAGE_PCA);
        launch_cluster_step(ctx->stream, v, K, w, d_label, d_dist2);
    }
    if (int rc = check_launch(ctx)) return rc;
    std::vector<double> got(cluster_out_words((int)L, K));
    if (int rc = thz_memcpy_d2h(ctx, got.data(), w.out, got.size() * sizeof(double))) return rc;
    for (int c = 0; c < K; ++c) {
        const double *row = got.data() + (size_t)c * (L + 1);
        if (sums) std::memcpy(sums + (size_t)c * L, row, L * sizeof(double));
        counts[c] = (uint64_t)row[L];
    }
    const size_t n = (size_t)K * (L + 1);
    *inertia = got[n];
    *farthest = (uint64_t)got[n + 1];
    std::memcpy(changed, &got[n + 2], sizeof(uint64_t));
    return THZ_OK;
}

int thz_session_cluster_step(thz_session *s, int which, const thz_cluster_cfg *cfg, const float *centroids, double *sums, uint64_t *counts,
                             double *inertia, uint64_t *changed, uint64_t *farthest)
{
    if (!s) return THZ_ERR_INVALID;
    thz_ctx *ctx = s->ctx;
    if (int rc = use_device(ctx)) return rc;
    if (!cfg || !centroids || !counts || !inertia || !changed || !farthest)
        return fail(ctx, THZ_ERR_INVALID, "thz_session_cluster_step: a required pointer is NULL");
    SessionMatrix m;
    if (int rc = cluster_matrix(s, which, cfg, &m)) return rc;
    if (bad_k(cfg)) return fail(ctx, THZ_ERR_INVALID, "thz_session_cluster_step: 1 <= n_clusters <= THZ_CLUSTER_MAX");
    return session_step(s, m, cfg->d_mask, centroids, cfg->n_clusters, cfg->init != 0, sums, counts, inertia, changed, farthest);
}

int thz_session_cluster_row(thz_session *s, int which, const thz_cluster_cfg *cfg, uint64_t pixel, float *row)
{
    if (!s) return THZ_ERR_INVALID;
    thz_ctx *ctx = s->ctx;
    if (int rc = use_device(ctx)) return rc;
    if (!cfg || !row) return fail(ctx, THZ_ERR_INVALID, "thz_session_cluster_row: a required pointer is NULL");
    SessionMatrix m;
    if (int rc = cluster_matrix(s, which, cfg, &m)) return rc;
    if (pixel >= (uint64_t)m.npix) return fail(ctx, THZ_ERR_INVALID, "thz_session_cluster_row: the pixel is outside the grid");
    return fetch_row(ctx, m, (size_t)pixel, row);
}

int thz_session_cluster(thz_session *s, int which, const thz_cluster_cfg *cfg, thz_cluster_out *out)
{
    if (!s) return THZ_ERR_INVALID;
    thz_ctx *ctx = s->ctx;
    if (int rc = use_device(ctx)) return rc;
    if (!cfg || !out) return fail(ctx, THZ_ERR_INVALID, "thz_session_cluster: a required pointer is NULL");
    *out = thz_cluster_out{};
    SessionMatrix m;
    if (int rc = cluster_matrix(s, which, cfg, &m)) return rc;
    if (bad_k(cfg)) return fail(ctx, THZ_ERR_INVALID, "thz_session_cluster: 1 <= n_clusters <= THZ_CLUSTER_MAX");
    if (cfg->init != 0 && cfg->init != 1) return fail(ctx, THZ_ERR_INVALID, "thz_session_cluster: init is 0 or 1");
    if (cfg->max_iter < 1 || cfg->max_iter > 1000) return fail(ctx, THZ_ERR_INVALID, "thz_session_cluster: 1 <= max_iter <= 1000");
    if (cfg->init == 0 && !cfg->centroids) return fail(ctx, THZ_ERR_INVALID, "thz_session_cluster: init 0 takes cfg->centroids");
    const size_t L = m.L;
    const int K = cfg->n_clusters;
    std::vector<float> cent((size_t)K * L), next((size_t)K * L);
    std::vector<double> sums((size_t)K * L);
    uint64_t counts[THZ_CLUSTER_MAX] = {0}, changed = 0, farthest = 0;
    double inertia = 0.0;
    if (cfg->init == 0) {
        std::memcpy(cent.data(), cfg->centroids, cent.size() * sizeof(float));
    } else {
        // farthest-first: the pixel farthest from the mean, then each time the one farthest from its nearest seed
        uint64_t count = 0;
        if (int rc = thz_pca_sums(ctx, m.npix, L, m.d, m.row_stride, m.col_step, cfg->d_mask, sums.data(), &count)) return rc;
        if (!count) return fail(ctx, THZ_ERR_INVALID, "thz_session_cluster: no unmasked pixel");
        for (size_t j = 0; j < L; ++j) next[j] = (float)(sums[j] / (double)count);
        for (int k = 0; k < K; ++k) {
            const float *seen = k ? cent.data() : next.data();
            if (int rc = session_step(s, m, cfg->d_mask, seen, k ? k : 1, true, nullptr, counts, &inertia, &changed, &farthest)) return rc;
            if (farthest >= (uint64_t)m.npix) {
                if (!k) return unfinished(s, "thz_session_cluster: no pixel at a finite distance from the mean");
                std::memcpy(cent.data() + (size_t)k * L, cent.data() + (size_t)(k - 1) * L, L * sizeof(float));
            } else if (int rc = fetch_row(ctx, m, (size_t)farthest, cent.data() + (size_t)k * L)) {
                return rc;
            }
        }
    }
    for (int it = 1; it <= cfg->max_iter; ++it) {
        if (int rc = session_step(s, m, cfg->d_mask, cent.data(), K, it == 1, sums.data(), counts, &inertia, &changed, &farthest)) return rc;
        out->iterations = it;
        out->converged = changed == 0;
        if (out->converged || it == cfg->max_iter) break;
        if (thz_host_cluster_update(sums.data(), counts, K, L, cent.data(), next.data()) != THZ_OK)
            return unfinished(s, "thz_session_cluster: a cluster's sum is not finite");
        cent.swap(next);
    }
    out->inertia = inertia;
    for (int c = 0; c < K; ++c) {
        out->counts[c] = counts[c];
        out->count += counts[c];
    }
    return THZ_OK;
}

}  // extern "C"
