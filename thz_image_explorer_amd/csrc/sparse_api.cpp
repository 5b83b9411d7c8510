// sparse_api.cpp — sparse deconvolution of every trace (include/thzgpu.h, "Sparse deconvolution"): the stage entry
// point over sparse.hip and its session form.  The host twin and the argument rules are sparse_host.cpp's.
#include "session.hpp"
#include "sparse.hpp"

#include <vector>

using namespace thz;

extern "C" {

int thz_sparse_deconv(thz_ctx *ctx, size_t npix, size_t nt, const float *d_data, const float *taps, const thz_sparse_cfg *cfg,
                      float *d_out, float *d_resid, int32_t *d_nnz)
{
    if (!ctx) return THZ_ERR_INVALID;
    if (int rc = use_device(ctx)) return rc;
    if (!d_data || !taps || !cfg || !d_out) return fail(ctx, THZ_ERR_INVALID, "thz_sparse_deconv: a required pointer is NULL");
    if (const char *why = sparse_cfg_error(cfg, nt, taps)) return fail(ctx, THZ_ERR_INVALID, std::string("thz_sparse_deconv: ") + why);
    SparseGeom g{};
    if (!sparse_geom((int)nt, cfg->n_taps, cfg->center, cfg->n_iter, cfg->accelerate, cfg->step, cfg->rel_lambda, cfg->min_lambda, &g))
        return fail(ctx, THZ_ERR_INVALID, "thz_sparse_deconv: the trace and its taps do not fit the kernel's LDS image");
    if (npix == 0) return THZ_OK;
    // taps of both products and the momentum table go up once per call
    std::vector<float> table(sparse_table_floats(g));
    sparse_fill_table(g, taps, cfg->n_taps, cfg->center, table.data());
    if (int rc = ensure_ws(ctx, table.size() * sizeof(float))) return rc;
    if (int rc = thz_memcpy_h2d(ctx, ctx->ws, table.data(), table.size() * sizeof(float))) return rc;
    StageTimer t(ctx, THZ_STAGE_ECHO);
    const hipError_t e = launch_sparse_deconv(ctx->stream, npix, g, d_data, ctx->ws.as<const float>(), d_out, d_resid, d_nnz);
    if (e != hipSuccess) return fail(ctx, THZ_ERR_HIP, std::string("thz_sparse_deconv: ") + hipGetErrorString(e));
    return THZ_OK;
}

int thz_session_sparse_deconv(thz_session *s, int which, const float *taps, const thz_sparse_cfg *cfg)
{
    if (!s) return THZ_ERR_INVALID;
    thz_ctx *ctx = s->ctx;
    if (int rc = use_device(ctx)) return rc;
    if (!taps || !cfg) return fail(ctx, THZ_ERR_INVALID, "thz_session_sparse_deconv: a required pointer is NULL");
    if (which != THZ_BUF_RAW && which != THZ_BUF_DATA && which != THZ_BUF_DENOISED)
        return fail(ctx, THZ_ERR_INVALID, "thz_session_sparse_deconv: the traces are THZ_BUF_RAW, THZ_BUF_DATA or THZ_BUF_DENOISED");
    SessionCube c;
    if (int rc = session_cube(s, which, &c)) return rc;
    if (const char *why = sparse_cfg_error(cfg, c.nt, taps)) return fail(ctx, THZ_ERR_INVALID, std::string("thz_session_sparse_deconv: ") + why);
    const size_t npix = c.nx * c.ny;
    // [x: (npix, nt) | resid: npix | nnz: npix]
    ResidentMaps &m = s->maps[kMapSparse];
    if (int rc = maps_begin(ctx, &m, {{npix, c.nt}, {npix}, {npix}})) return rc;
    if (int rc = thz_sparse_deconv(ctx, npix, c.nt, c.d, taps, cfg, m.ptr(0), m.ptr(1), m.ptr<int32_t>(2))) return rc;
    // the spike trains as a cube for the per-trace maps: on the grid, pitch and time step of the cube they were taken of
    s->sparse_cube = c;
    s->sparse_cube.d = m.ptr(0);
    return maps_commit(ctx, &m);
}

}  // extern "C"
