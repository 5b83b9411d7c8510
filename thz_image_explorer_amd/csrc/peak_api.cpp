// peak_api.cpp — pulse arrival times and the tilt they imply (include/thzgpu.h, "Pulse arrival times"): the stage
// entry points over peak.hip and their session forms.
#include "session.hpp"
#include "peak.hpp"

using namespace thz;

extern "C" {

int thz_peak_map(thz_ctx *ctx, size_t npix, size_t nt, const float *d_data, int mode, int32_t *d_index, float *d_offset,
                 float *d_value)
{
    if (!ctx) return THZ_ERR_INVALID;
    if (int rc = use_device(ctx)) return rc;
    if (!d_data || nt == 0 || nt > ((size_t)1 << 30) || mode < 0 || mode > 2)
        return fail(ctx, THZ_ERR_INVALID, "thz_peak_map: bad argument (mode 0..2, 1 <= nt <= 2^30)");
    if (npix == 0 || (!d_index && !d_offset && !d_value)) return THZ_OK;
    StageTimer t(ctx, THZ_STAGE_PEAK);
    launch_peak_map(ctx->stream, npix, (int)nt, d_data, mode, d_index, d_offset, d_value);
    return check_launch(ctx);
}

int thz_arrival_plane_moments(thz_ctx *ctx, size_t nx, size_t ny, float dx, float dy, double dt_ps, const int32_t *d_index,
                              const float *d_offset, const float *d_value, float rel_threshold, double *moments)
{
    if (!ctx) return THZ_ERR_INVALID;
    if (int rc = use_device(ctx)) return rc;
    if (!d_index || !d_offset || !d_value || !moments || nx == 0 || ny == 0)
        return fail(ctx, THZ_ERR_INVALID, "thz_arrival_plane_moments: bad argument");
    if (int rc = ensure_ws(ctx, plane_moments_ws_bytes())) return rc;
    launch_plane_moments(ctx->stream, nx, ny, (double)dx, (double)dy, dt_ps, d_index, d_offset, d_value, rel_threshold, ctx->ws);
    if (int rc = check_launch(ctx)) return rc;
    return thz_memcpy_d2h(ctx, moments, ctx->ws, 10 * sizeof(double));
}

}  // extern "C"

int session_cube(thz_session *s, int which, SessionCube *out)
{
    thz_ctx *ctx = s->ctx;
    if (which != THZ_BUF_RAW && which != THZ_BUF_DATA && which != THZ_BUF_SPARSE && which != THZ_BUF_DENOISED)
        return fail(ctx, THZ_ERR_INVALID, "arrival times are taken of THZ_BUF_RAW, THZ_BUF_DATA, THZ_BUF_SPARSE or THZ_BUF_DENOISED");
    out->d = static_cast<const float *>(session_buffer_ro(s, which));
    if (which == THZ_BUF_SPARSE) {  // the spike trains, on the grid and axis of the cube they were taken of
        if (!out->d) return fail(ctx, THZ_ERR_NOT_READY, "arrival times: no spike trains are resident (thz_session_sparse_deconv)");
        *out = s->sparse_cube;
        return THZ_OK;
    }
    if (which == THZ_BUF_DENOISED) {  // likewise the denoised traces
        if (!out->d) return fail(ctx, THZ_ERR_NOT_READY, "arrival times: no denoised traces are resident (thz_session_wavelet_denoise)");
        *out = s->denoised_cube;
        return THZ_OK;
    }
    if (!out->d) return fail(ctx, THZ_ERR_NOT_READY, "arrival times: the cube is not available (no recompute has run)");
    const bool raw = which == THZ_BUF_RAW;
    const std::vector<float> &time = raw ? s->time : s->time_out;
    out->nx = raw ? s->nx : s->nx_cur;
    out->ny = raw ? s->ny : s->ny_cur;
    out->nt = raw ? s->nt : s->nt_out;
    out->dx = raw ? s->dx : s->dx_cur;
    out->dy = raw ? s->dy : s->dy_cur;
    out->dt_ps = time.size() > 1 ? ((double)time.back() - (double)time.front()) / (double)(time.size() - 1) : 0.0;
    return THZ_OK;
}

extern "C" {

int thz_session_peak_map(thz_session *s, int which, int mode)
{
    if (!s) return THZ_ERR_INVALID;
    thz_ctx *ctx = s->ctx;
    if (int rc = use_device(ctx)) return rc;
    if (mode < 0 || mode > 2) return fail(ctx, THZ_ERR_INVALID, "thz_session_peak_map: mode is 0, 1 or 2");
    SessionCube c;
    if (int rc = session_cube(s, which, &c)) return rc;
    const size_t npix = c.nx * c.ny;
    // [index | offset | value], one entry per pixel of the mapped grid (the kernel stores them an element at a time)
    ResidentMaps &m = s->maps[kMapPeak];
    if (int rc = maps_begin(ctx, &m, {{npix}, {npix}, {npix}})) return rc;
    if (int rc = thz_peak_map(ctx, npix, c.nt, c.d, mode, m.ptr<int32_t>(0), m.ptr(1), m.ptr(2))) return rc;
    return maps_commit(ctx, &m);
}

int thz_session_estimate_tilt(thz_session *s, int which, int mode, float rel_threshold, thz_tilt_fit *out)
{
    if (!s || !out) return THZ_ERR_INVALID;
    *out = thz_tilt_fit{};
    if (int rc = thz_session_peak_map(s, which, mode)) return rc;
    SessionCube c;
    if (int rc = session_cube(s, which, &c)) return rc;
    double m[10];
    const ResidentMaps &peak = s->maps[kMapPeak];
    if (int rc = thz_arrival_plane_moments(s->ctx, c.nx, c.ny, c.dx, c.dy, c.dt_ps, peak.ptr<int32_t>(0), peak.ptr(1), peak.ptr(2),
                                           rel_threshold, m))
        return rc;
    return thz_host_arrival_plane_fit(m, out);
}

}  // extern "C"
