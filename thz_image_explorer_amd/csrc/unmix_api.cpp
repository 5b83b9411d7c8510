// unmix_api.cpp — non-negative least squares of every pixel against K endmembers (include/thzgpu.h, "Unmixing every
// pixel into its materials"): the stage entry point over unmix.hip and its session form.  The normal matrix and the
// solve's host twin are unmix_host.cpp's.
#include "session.hpp"
#include "unmix.hpp"

#include <cmath>
#include <cstring>

using namespace thz;

namespace {

// the argument rules of both entry points besides the matrix's own: the reason for THZ_ERR_INVALID, or null
const char *unmix_cfg_error(int K, int n_sweeps)
{
    if (K < 1 || K > THZ_UNMIX_MAX) return "1 <= n_endmembers <= THZ_UNMIX_MAX";
    if (n_sweeps < 0 || n_sweeps > THZ_UNMIX_MAX_SWEEPS) return "0 <= n_sweeps <= THZ_UNMIX_MAX_SWEEPS";
    return nullptr;
}

}  // namespace

extern "C" {

int thz_unmix(thz_ctx *ctx, size_t npix, size_t L, const float *d_x, size_t row_stride, size_t col_step, const float *endmembers,
              const float *ref, const thz_unmix_cfg *cfg, float *d_abund, float *d_proj, float *d_resid, float *d_kkt)
{
    if (!ctx) return THZ_ERR_INVALID;
    if (int rc = use_device(ctx)) return rc;
    if (!endmembers || !cfg || !d_abund) return fail(ctx, THZ_ERR_INVALID, "thz_unmix: a required pointer is NULL");
    if (const char *why = pca_view_error(L, d_x, row_stride, col_step)) return fail(ctx, THZ_ERR_INVALID, std::string("thz_unmix: ") + why);
    if (const char *why = unmix_cfg_error(cfg->n_endmembers, cfg->n_sweeps)) return fail(ctx, THZ_ERR_INVALID, std::string("thz_unmix: ") + why);
    const int K = cfg->n_endmembers;
    const bool absorbance = cfg->absorbance != 0;
    // [E | lref | Gt | rd] (unmix.hpp) go up once per call
    std::vector<float> tab(unmix_table_floats((int)L, K), 0.0f);
    std::memcpy(tab.data(), endmembers, (size_t)K * L * sizeof(float));
    float *lref = tab.data() + (size_t)K * L, *gt = lref + L, *rd = gt + (size_t)K * K;
    if (absorbance) {
        if (!ref) return fail(ctx, THZ_ERR_INVALID, "thz_unmix: absorbance takes a reference spectrum");
        for (size_t j = 0; j < L; ++j) {
            if (!std::isfinite(ref[j]) || !(ref[j] > 0.0f)) return fail(ctx, THZ_ERR_INVALID, "thz_unmix: the reference spectrum is finite and > 0");
            lref[j] = (float)std::log((double)ref[j]);
        }
    }
    float G[THZ_UNMIX_MAX * THZ_UNMIX_MAX];
    if (thz_host_unmix_prepare(endmembers, K, L, G, rd) != THZ_OK)
        return fail(ctx, THZ_ERR_INVALID, "thz_unmix: an endmember is zero or holds a non-finite value");
    for (int c = 0; c < K; ++c)
        for (int i = 0; i < K; ++i) gt[c * K + i] = G[i * K + c];
    if (npix == 0) return THZ_OK;
    // without d_proj the projections live behind the table for the length of the call
    const size_t tab_floats = (tab.size() + 3) & ~(size_t)3;
    if (int rc = ensure_ws(ctx, (tab_floats + (d_proj ? 0 : (size_t)K * npix)) * sizeof(float))) return rc;
    float *d_tab = ctx->ws.as<float>();
    if (!d_proj) d_proj = d_tab + tab_floats;
    if (int rc = thz_memcpy_h2d(ctx, d_tab, tab.data(), tab.size() * sizeof(float))) return rc;
    const UnmixTable t = unmix_table(d_tab, (int)L, K);
    const PcaView v{d_x, npix, (int)L, row_stride, col_step, nullptr};
    StageTimer timer(ctx, THZ_STAGE_PCA);
    launch_unmix_project(ctx->stream, v, t, K, absorbance, d_proj);
    launch_unmix_solve(ctx->stream, npix, t, K, cfg->n_sweeps, d_proj, d_abund, d_kkt);
    if (d_resid) launch_unmix_resid(ctx->stream, v, t, K, absorbance, d_abund, d_resid);
    return check_launch(ctx);
}

int thz_session_unmix(thz_session *s, int which, const thz_unmix_session_cfg *cfg)
{
    if (!s) return THZ_ERR_INVALID;
    thz_ctx *ctx = s->ctx;
    if (int rc = use_device(ctx)) return rc;
    if (!cfg) return fail(ctx, THZ_ERR_INVALID, "thz_session_unmix: cfg is NULL");
    thz_pca_cfg columns{};
    columns.first = cfg->first;
    columns.count = cfg->count;
    columns.step = cfg->step;
    SessionMatrix m;
    if (int rc = session_matrix(s, which, &columns, "unmixing", &m)) return rc;
    if (const char *why = unmix_cfg_error(cfg->n_endmembers, cfg->n_sweeps))
        return fail(ctx, THZ_ERR_INVALID, std::string("thz_session_unmix: ") + why);
    const size_t K = (size_t)cfg->n_endmembers;
    std::vector<float> centroids;
    const float *endmembers = cfg->endmembers;
    if (!endmembers) {
        // the mean spectra of the last segmentation: THZ_BUF_CLUSTER_CENTROIDS, (K, L)
        const ResidentMaps &cluster = s->maps[kMapCluster];
        if (!cluster.entries(2)) return fail(ctx, THZ_ERR_NOT_READY, "thz_session_unmix: no segmentation has run: there are no centroids");
        if (cluster.entries(2) != K * m.L)
            return fail(ctx, THZ_ERR_INVALID, "thz_session_unmix: the resident centroids are not n_endmembers x count");
        centroids.resize(K * m.L);
        if (int rc = thz_memcpy_d2h(ctx, centroids.data(), cluster.ptr(2), centroids.size() * sizeof(float))) return rc;
        endmembers = centroids.data();
    }
    thz_unmix_cfg call{};
    call.n_endmembers = cfg->n_endmembers;
    call.n_sweeps = cfg->n_sweeps;
    call.absorbance = cfg->absorbance;
    // what thz_unmix would refuse is refused before the resident maps are touched
    if (cfg->absorbance != 0) {
        if (!cfg->ref) return fail(ctx, THZ_ERR_INVALID, "thz_session_unmix: absorbance takes a reference spectrum");
        for (size_t j = 0; j < m.L; ++j)
            if (!std::isfinite(cfg->ref[j]) || !(cfg->ref[j] > 0.0f))
                return fail(ctx, THZ_ERR_INVALID, "thz_session_unmix: the reference spectrum is finite and > 0");
    }
    {
        float G[THZ_UNMIX_MAX * THZ_UNMIX_MAX], rd[THZ_UNMIX_MAX];
        if (thz_host_unmix_prepare(endmembers, (int)K, m.L, G, rd) != THZ_OK)
            return fail(ctx, THZ_ERR_INVALID, "thz_session_unmix: an endmember is zero or holds a non-finite value");
    }
    // [abundances: (K, npix), endmember-major | projections: (K, npix) | residual: npix | kkt: npix]
    ResidentMaps &r = s->maps[kMapUnmix];
    if (int rc = maps_begin(ctx, &r, {{K * m.npix}, {K * m.npix}, {m.npix}, {m.npix}})) return rc;
    if (int rc = thz_unmix(ctx, m.npix, m.L, m.d, m.row_stride, m.col_step, endmembers, cfg->ref, &call, r.ptr(0), r.ptr(1), r.ptr(2), r.ptr(3)))
        return rc;
    return maps_commit(ctx, &r);
}

}  // extern "C"
