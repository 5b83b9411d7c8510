// wavelet_api.cpp — wavelet shrinkage of every trace (include/thzgpu.h, "Denoising every trace"): the stage entry point
// over wavelet.hip and its session form.  The host twin and the argument rules are wavelet_host.cpp's.
#include "session.hpp"
#include "wavelet.hpp"

using namespace thz;

extern "C" {

int thz_wavelet_denoise(thz_ctx *ctx, size_t npix, size_t nt, const float *d_data, const float *hn, const float *gn,
                        const float *scale, const thz_wavelet_cfg *cfg, float *d_out, float *d_sigma, int32_t *d_kept)
{
    if (!ctx) return THZ_ERR_INVALID;
    if (int rc = use_device(ctx)) return rc;
    if (!d_data || !hn || !gn || !scale || !cfg || !d_out) return fail(ctx, THZ_ERR_INVALID, "thz_wavelet_denoise: a required pointer is NULL");
    if (const char *why = wavelet_cfg_error(cfg, nt, hn, gn, scale)) return fail(ctx, THZ_ERR_INVALID, std::string("thz_wavelet_denoise: ") + why);
    if (npix == 0) return THZ_OK;
    WaveletParams w{};
    w.nt = (int)nt;
    w.n_taps = cfg->n_taps;
    w.n_levels = cfg->n_levels;
    w.shrink = cfg->shrink;
    w.noise_mode = cfg->noise_mode;
    for (int k = 0; k < cfg->n_taps; ++k) {
        w.hn[k] = hn[k];
        w.gn[k] = gn[k];
    }
    for (int j = 0; j < cfg->n_levels; ++j) w.scale[j] = scale[j];
    StageTimer t(ctx, THZ_STAGE_ECHO);
    const hipError_t e = launch_wavelet_denoise(ctx->stream, npix, w, d_data, d_out, d_sigma, d_kept);
    if (e != hipSuccess) return fail(ctx, THZ_ERR_HIP, std::string("thz_wavelet_denoise: ") + hipGetErrorString(e));
    return THZ_OK;
}

int thz_session_wavelet_denoise(thz_session *s, int which, const float *hn, const float *gn, const float *scale,
                                const thz_wavelet_cfg *cfg)
{
    if (!s) return THZ_ERR_INVALID;
    thz_ctx *ctx = s->ctx;
    if (int rc = use_device(ctx)) return rc;
    if (!hn || !gn || !scale || !cfg) return fail(ctx, THZ_ERR_INVALID, "thz_session_wavelet_denoise: a required pointer is NULL");
    if (which != THZ_BUF_RAW && which != THZ_BUF_DATA)
        return fail(ctx, THZ_ERR_INVALID, "thz_session_wavelet_denoise: the traces are THZ_BUF_RAW or THZ_BUF_DATA");
    SessionCube c;
    if (int rc = session_cube(s, which, &c)) return rc;
    if (const char *why = wavelet_cfg_error(cfg, c.nt, hn, gn, scale))
        return fail(ctx, THZ_ERR_INVALID, std::string("thz_session_wavelet_denoise: ") + why);
    const size_t npix = c.nx * c.ny;
    // [x: (npix, nt) | sigma: npix | kept: npix]
    ResidentMaps &m = s->maps[kMapDenoise];
    if (int rc = maps_begin(ctx, &m, {{npix, c.nt}, {npix}, {npix}})) return rc;
    if (int rc = thz_wavelet_denoise(ctx, npix, c.nt, c.d, hn, gn, scale, cfg, m.ptr(0), m.ptr(1), m.ptr<int32_t>(2))) return rc;
    // the denoised traces as a cube for the per-trace maps: on the grid, pitch and time step of the cube they were taken of
    s->denoised_cube = c;
    s->denoised_cube.d = m.ptr(0);
    return maps_commit(ctx, &m);
}

}  // extern "C"
