// pca_api.cpp — principal components of a scan (include/thzgpu.h, "Principal components of a scan"): the stage entry
// points over pca.hip and their session forms.  The eigenvectors are pca_host.cpp's.
#include "session.hpp"
#include "pca.hpp"

#include <cstring>

using namespace thz;

// the argument rules every device call shares, checked before anything is launched or allocated
const char *pca_view_error(size_t L, const float *d_x, size_t row_stride, size_t col_step)
{
    if (!d_x) return "d_x is NULL";
    if (L < 1 || L > THZ_PCA_MAX_LEN) return "1 <= L <= THZ_PCA_MAX_LEN";
    if (col_step < 1) return "col_step >= 1";
    if (row_stride > ((size_t)1 << 40) || col_step > ((size_t)1 << 30)) return "row_stride <= 2^40, col_step <= 2^30";
    return nullptr;
}

namespace {

PcaView view_of(size_t npix, size_t L, const float *d_x, size_t row_stride, size_t col_step, const uint8_t *d_mask)
{
    return PcaView{d_x, npix, (int)L, row_stride, col_step, d_mask};
}

}  // namespace

// what `which` and the columns of cfg name in a session: the matrix, or the error (`what` starts its message)
int session_matrix(thz_session *s, int which, const thz_pca_cfg *cfg, const char *what, SessionMatrix *m)
{
    const std::string of = std::string(what) + ": ";
    thz_ctx *ctx = s->ctx;
    if (which != THZ_BUF_AMPLITUDES && which != THZ_BUF_PHASES && which != THZ_BUF_DATA && which != THZ_BUF_RAW)
        return fail(ctx, THZ_ERR_INVALID, of + "the matrix is THZ_BUF_AMPLITUDES, _PHASES, _DATA or _RAW");
    size_t len = 0;
    if (which == THZ_BUF_RAW) {
        m->d = s->d_raw;
        m->npix = s->nx * s->ny;
        len = s->nt;
    } else {
        if (!s->have_outputs) return fail(ctx, THZ_ERR_NOT_READY, of + "no recompute has run");
        const size_t grid = s->nx_cur * s->ny_cur;
        m->npix = s->out_pix < grid ? s->out_pix : grid;
        // the session's own pointers for the spectra: thz_session_buffer would make the next recompute store every
        // bin (session.hpp)
        m->d = which == THZ_BUF_AMPLITUDES ? s->d_amp
               : which == THZ_BUF_PHASES   ? s->d_ph
                                           : static_cast<const float *>(session_buffer_ro(s, THZ_BUF_DATA));
        len = which == THZ_BUF_DATA ? s->nt_out : s->nf_out;
    }
    if (!m->d) return fail(ctx, THZ_ERR_NOT_READY, of + "the cube is not available");
    if (cfg->count < 1 || cfg->count > THZ_PCA_MAX_LEN || cfg->step < 1
        || (uint64_t)cfg->first + (uint64_t)(cfg->count - 1) * (uint64_t)cfg->step >= (uint64_t)len)
        return fail(ctx, THZ_ERR_INVALID,
                    of + "1 <= count <= THZ_PCA_MAX_LEN, step >= 1, and the last column inside the row of " + std::to_string(len));
    m->d += cfg->first;
    m->L = cfg->count;
    m->row_stride = len;
    m->col_step = cfg->step;
    return THZ_OK;
}

namespace {

bool bad_k(const thz_pca_cfg *cfg)
{
    return cfg->n_components < 1 || cfg->n_components > THZ_PCA_MAX_COMPONENTS || (uint32_t)cfg->n_components > cfg->count;
}

}  // namespace

extern "C" {

int thz_pca_sums(thz_ctx *ctx, size_t npix, size_t L, const float *d_x, size_t row_stride, size_t col_step,
                 const uint8_t *d_mask, double *sum, uint64_t *count)
{
    if (!ctx) return THZ_ERR_INVALID;
    if (int rc = use_device(ctx)) return rc;
    if (!sum || !count) return fail(ctx, THZ_ERR_INVALID, "thz_pca_sums: a required pointer is NULL");
    if (const char *why = pca_view_error(L, d_x, row_stride, col_step)) return fail(ctx, THZ_ERR_INVALID, std::string("thz_pca_sums: ") + why);
    std::memset(sum, 0, L * sizeof(double));
    *count = 0;
    if (npix == 0) return THZ_OK;
    const PcaView v = view_of(npix, L, d_x, row_stride, col_step, d_mask);
    if (int rc = ensure_ws(ctx, pca_sums_ws_bytes(npix, (int)L))) return rc;
    launch_pca_sums(ctx->stream, v, ctx->ws);
    if (int rc = check_launch(ctx)) return rc;
    std::vector<double> got(L + 1);
    if (int rc = thz_memcpy_d2h(ctx, got.data(), ctx->ws, got.size() * sizeof(double))) return rc;
    std::memcpy(sum, got.data(), L * sizeof(double));
    *count = (uint64_t)got[L];
    return THZ_OK;
}

int thz_pca_gram(thz_ctx *ctx, size_t npix, size_t L, const float *d_x, size_t row_stride, size_t col_step,
                 const uint8_t *d_mask, const float *mu, double *gram)
{
    if (!ctx) return THZ_ERR_INVALID;
    if (int rc = use_device(ctx)) return rc;
    if (!gram) return fail(ctx, THZ_ERR_INVALID, "thz_pca_gram: gram is NULL");
    if (const char *why = pca_view_error(L, d_x, row_stride, col_step)) return fail(ctx, THZ_ERR_INVALID, std::string("thz_pca_gram: ") + why);
    std::memset(gram, 0, L * L * sizeof(double));
    if (npix == 0) return THZ_OK;
    const PcaView v = view_of(npix, L, d_x, row_stride, col_step, d_mask);
    if (int rc = ensure_ws(ctx, pca_gram_ws_bytes(npix, (int)L))) return rc;
    // no mu: zeros — x - 0 is x, bit for bit
    std::vector<float> m(L, 0.0f);
    if (mu) std::memcpy(m.data(), mu, L * sizeof(float));
    if (int rc = thz_memcpy_h2d(ctx, ctx->ws.as<unsigned char>() + pca_gram_mu_offset((int)L), m.data(), L * sizeof(float)))
        return rc;
    {
        StageTimer t(ctx, THZ_STAGE_PCA);
        launch_pca_gram(ctx->stream, v, ctx->ws);
    }
    if (int rc = check_launch(ctx)) return rc;
    return thz_memcpy_d2h(ctx, gram, ctx->ws, L * L * sizeof(double));
}

int thz_pca_scores(thz_ctx *ctx, size_t npix, size_t L, const float *d_x, size_t row_stride, size_t col_step,
                   const float *mu, const float *components, int K, float *d_scores)
{
    if (!ctx) return THZ_ERR_INVALID;
    if (int rc = use_device(ctx)) return rc;
    if (!components || !d_scores) return fail(ctx, THZ_ERR_INVALID, "thz_pca_scores: a required pointer is NULL");
    if (const char *why = pca_view_error(L, d_x, row_stride, col_step)) return fail(ctx, THZ_ERR_INVALID, std::string("thz_pca_scores: ") + why);
    if (K < 1 || K > THZ_PCA_MAX_COMPONENTS) return fail(ctx, THZ_ERR_INVALID, "thz_pca_scores: 1 <= K <= THZ_PCA_MAX_COMPONENTS");
    if (npix == 0) return THZ_OK;
    // [mu | components] go up once per call
    std::vector<float> tab((size_t)(K + 1) * L, 0.0f);
    if (mu) std::memcpy(tab.data(), mu, L * sizeof(float));
    std::memcpy(tab.data() + L, components, (size_t)K * L * sizeof(float));
    if (int rc = ensure_ws(ctx, tab.size() * sizeof(float))) return rc;
    if (int rc = thz_memcpy_h2d(ctx, ctx->ws, tab.data(), tab.size() * sizeof(float))) return rc;
    const PcaView v = view_of(npix, L, d_x, row_stride, col_step, nullptr);
    StageTimer t(ctx, THZ_STAGE_PCA);
    launch_pca_scores(ctx->stream, v, ctx->ws.as<const float>(), K, d_scores);
    return check_launch(ctx);
}

int thz_session_pca_sums(thz_session *s, int which, const thz_pca_cfg *cfg, double *sum, uint64_t *count)
{
    if (!s) return THZ_ERR_INVALID;
    thz_ctx *ctx = s->ctx;
    if (int rc = use_device(ctx)) return rc;
    if (!cfg) return fail(ctx, THZ_ERR_INVALID, "thz_session_pca_sums: cfg is NULL");
    SessionMatrix m;
    if (int rc = session_matrix(s, which, cfg, "principal components", &m)) return rc;
    return thz_pca_sums(ctx, m.npix, m.L, m.d, m.row_stride, m.col_step, cfg->d_mask, sum, count);
}

int thz_session_pca_gram(thz_session *s, int which, const thz_pca_cfg *cfg, const float *mu, double *gram)
{
    if (!s) return THZ_ERR_INVALID;
    thz_ctx *ctx = s->ctx;
    if (int rc = use_device(ctx)) return rc;
    if (!cfg) return fail(ctx, THZ_ERR_INVALID, "thz_session_pca_gram: cfg is NULL");
    SessionMatrix m;
    if (int rc = session_matrix(s, which, cfg, "principal components", &m)) return rc;
    return thz_pca_gram(ctx, m.npix, m.L, m.d, m.row_stride, m.col_step, cfg->d_mask, mu, gram);
}

int thz_session_pca_project(thz_session *s, int which, const thz_pca_cfg *cfg, const float *mu, const float *components)
{
    if (!s) return THZ_ERR_INVALID;
    thz_ctx *ctx = s->ctx;
    if (int rc = use_device(ctx)) return rc;
    if (!cfg || !components) return fail(ctx, THZ_ERR_INVALID, "thz_session_pca_project: a required pointer is NULL");
    SessionMatrix m;
    if (int rc = session_matrix(s, which, cfg, "principal components", &m)) return rc;
    if (bad_k(cfg)) return fail(ctx, THZ_ERR_INVALID, "thz_session_pca_project: 1 <= n_components <= min(count, THZ_PCA_MAX_COMPONENTS)");
    const size_t K = (size_t)cfg->n_components;
    // [scores: (K, npix), component-major | components: (K, L) | mean: L]
    ResidentMaps &r = s->maps[kMapPca];
    if (int rc = maps_begin(ctx, &r, {{K * m.npix}, {K * m.L}, {m.L}})) return rc;
    std::vector<float> tail((K + 1) * m.L, 0.0f);  // the two planes behind the scores, in one copy
    std::memcpy(tail.data(), components, K * m.L * sizeof(float));
    if (mu) std::memcpy(tail.data() + K * m.L, mu, m.L * sizeof(float));
    if (int rc = thz_memcpy_h2d(ctx, r.ptr(1), tail.data(), tail.size() * sizeof(float))) return rc;
    if (int rc = thz_pca_scores(ctx, m.npix, m.L, m.d, m.row_stride, m.col_step, mu, components, (int)K, r.ptr(0))) return rc;
    return maps_commit(ctx, &r);
}

int thz_session_pca(thz_session *s, int which, const thz_pca_cfg *cfg, thz_pca_out *out)
{
    if (!s) return THZ_ERR_INVALID;
    thz_ctx *ctx = s->ctx;
    if (int rc = use_device(ctx)) return rc;
    if (!cfg || !out) return fail(ctx, THZ_ERR_INVALID, "thz_session_pca: a required pointer is NULL");
    *out = thz_pca_out{};
    SessionMatrix m;
    if (int rc = session_matrix(s, which, cfg, "principal components", &m)) return rc;
    if (bad_k(cfg)) return fail(ctx, THZ_ERR_INVALID, "thz_session_pca: 1 <= n_components <= min(count, THZ_PCA_MAX_COMPONENTS)");
    const size_t L = m.L;
    const int K = cfg->n_components;
    std::vector<double> sum(L), gram(L * L);
    uint64_t count = 0;
    if (int rc = thz_session_pca_sums(s, which, cfg, sum.data(), &count)) return rc;
    out->count = count;
    if (count < 2) return fail(ctx, THZ_ERR_INVALID, "thz_session_pca: fewer than two unmasked pixels");
    std::vector<float> mu(L, 0.0f);
    if (cfg->center)
        for (size_t j = 0; j < L; ++j) mu[j] = (float)(sum[j] / (double)count);
    const float *mu_arg = cfg->center ? mu.data() : nullptr;
    if (int rc = thz_session_pca_gram(s, which, cfg, mu_arg, gram.data())) return rc;
    std::vector<float> comp((size_t)K * L);
    if (int rc = thz_host_pca_components(gram.data(), L, count, K, comp.data(), out->eigenvalues, &out->total_variance))
        return fail(ctx, rc, "thz_session_pca: the covariance has no eigenvectors (a non-finite entry)");
    return thz_session_pca_project(s, which, cfg, mu_arg, comp.data());
}

}  // extern "C"
