// optical_api.cpp — optical-property maps (include/thzgpu.h, "Optical-property maps"): the stage entry point over
// optical.hip and its session form.
#include "session.hpp"
#include "optical.hpp"

using namespace thz;

namespace {

// the argument rules of thz_optical_maps, checked before anything is launched or allocated
const char *optical_cfg_error(const thz_optical_cfg *cfg, size_t nf)
{
    if (nf == 0 || nf > ((size_t)1 << 30)) return "1 <= nf <= 2^30";
    if (cfg->n_bands > THZ_OPTICAL_MAX_BANDS) return "at most THZ_OPTICAL_MAX_BANDS bands";
    for (uint32_t b = 0; b < cfg->n_bands; ++b)
        if (!(cfg->band_k0[b] >= 1 && cfg->band_k0[b] < cfg->band_k1[b] && cfg->band_k1[b] <= nf))
            return "every band needs 1 <= k0 < k1 <= nf (bin 0 has omega = 0)";
    if (cfg->anchor_k0 != cfg->anchor_k1 && !(cfg->anchor_k0 < cfg->anchor_k1 && cfg->anchor_k1 - cfg->anchor_k0 >= 2))
        return "the anchor needs at least two bins, or anchor_k0 == anchor_k1 for none";
    if (cfg->anchor_k1 > nf) return "the anchor ends beyond nf";
    return nullptr;
}

}  // namespace

extern "C" {

int thz_optical_maps(thz_ctx *ctx, size_t npix, size_t nf, const float *d_amp, const float *d_phase, const float *ref_amp,
                     const float *ref_phase, const float *freq, const thz_optical_cfg *cfg, const float *d_thickness,
                     float *d_n, float *d_alpha, float *d_kappa, int32_t *d_wraps, float *d_slope)
{
    if (!ctx) return THZ_ERR_INVALID;
    if (int rc = use_device(ctx)) return rc;
    if (!cfg || !d_amp || !d_phase || !ref_amp || !ref_phase || !freq)
        return fail(ctx, THZ_ERR_INVALID, "thz_optical_maps: a required pointer is NULL");
    if (const char *why = optical_cfg_error(cfg, nf)) return fail(ctx, THZ_ERR_INVALID, std::string("thz_optical_maps: ") + why);
    if (npix == 0 || (!d_n && !d_alpha && !d_kappa && !d_wraps && !d_slope)) return THZ_OK;
    // the per-bin factors go up once per call
    std::vector<float> tab(optical_table_floats(nf));
    optical_tables(ref_amp, ref_phase, freq, nf, tab.data());
    if (int rc = ensure_ws(ctx, tab.size() * sizeof(float))) return rc;
    if (int rc = thz_memcpy_h2d(ctx, ctx->ws, tab.data(), tab.size() * sizeof(float))) return rc;
    OpticalGeom g{};
    g.thickness = cfg->thickness;
    g.a0 = cfg->anchor_k0;
    g.a1 = cfg->anchor_k1;
    g.n_bands = cfg->n_bands;
    for (uint32_t b = 0; b < cfg->n_bands; ++b) {
        g.k0[b] = cfg->band_k0[b];
        g.k1[b] = cfg->band_k1[b];
    }
    StageTimer t(ctx, THZ_STAGE_OPTICAL);
    launch_optical_map(ctx->stream, npix, (int)nf, d_amp, d_phase, ctx->ws.as<const float>(), g, d_thickness, d_n, d_alpha,
                       d_kappa, d_wraps, d_slope);
    return check_launch(ctx);
}

int thz_session_optical_maps(thz_session *s, const float *ref_amp, const float *ref_phase, size_t nf, const thz_optical_cfg *cfg,
                             const float *d_thickness)
{
    if (!s) return THZ_ERR_INVALID;
    thz_ctx *ctx = s->ctx;
    if (int rc = use_device(ctx)) return rc;
    if (!cfg || !ref_amp || !ref_phase) return fail(ctx, THZ_ERR_INVALID, "thz_session_optical_maps: a required pointer is NULL");
    if (!s->have_outputs) return fail(ctx, THZ_ERR_NOT_READY, "thz_session_optical_maps: no spectra are resident (no recompute has run)");
    if (nf != s->nt_out / 2 + 1)
        return fail(ctx, THZ_ERR_INVALID, "thz_session_optical_maps: the reference has " + std::to_string(nf) + " bins, the resident spectra "
                                              + std::to_string(s->nt_out / 2 + 1));
    if (const char *why = optical_cfg_error(cfg, nf)) return fail(ctx, THZ_ERR_INVALID, std::string("thz_session_optical_maps: ") + why);
    const size_t npix = s->nx_cur * s->ny_cur, nb = cfg->n_bands;
    // the five images: [n | alpha | kappa] (n_bands, npix) each, band-major — empty planes without bands — then wraps and
    // slope (npix); the kernel stores them an element at a time
    ResidentMaps &m = s->maps[kMapOptical];
    if (int rc = maps_begin(ctx, &m, {{nb * npix}, {nb * npix}, {nb * npix}, {npix}, {npix}})) return rc;
    // the axis of the resident spectra, frequency[i] = i / (time[nt - 1] - time[0]) of the chain's final time axis
    std::vector<float> freq(nf);
    if (int rc = thz_host_frequency_axis(s->time_out.data(), s->nt_out, freq.data())) return rc;
    // the session's own pointers: thz_session_buffer would make the next recompute store every bin (session.hpp)
    if (int rc = thz_optical_maps(ctx, npix, nf, s->d_amp, s->d_ph, ref_amp, ref_phase, freq.data(), cfg, d_thickness, m.ptr(0),
                                  m.ptr(1), m.ptr(2), m.ptr<int32_t>(3), m.ptr(4)))
        return rc;
    return maps_commit(ctx, &m);
}

}  // extern "C"
