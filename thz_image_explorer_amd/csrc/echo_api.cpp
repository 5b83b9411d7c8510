// echo_api.cpp — echoes and layer thickness (include/thzgpu.h, "Echoes and layer thickness"): the stage entry points
// over echo.hip, their session forms, and the same selection for one host vector.
// Built with -ffp-contract=off: the host's offsets are the f32 formula as written, like the kernel's.
#include "session.hpp"
#include "echo.hpp"

#include <cmath>

using namespace thz;

namespace {

// the argument rules of thz_echo_map and thz_host_echo_trace, checked before anything is launched
const char *echo_cfg_error(const thz_echo_cfg *cfg, size_t nt)
{
    if (nt == 0 || nt > ((size_t)1 << 30)) return "1 <= nt <= 2^30";
    if (cfg->mode < 0 || cfg->mode > 2) return "mode is 0, 1 or 2";
    if (cfg->n_echoes < 1 || cfg->n_echoes > THZ_ECHO_MAX) return "1 <= n_echoes <= THZ_ECHO_MAX";
    if (cfg->guard < 1) return "guard >= 1";
    if (!(std::isfinite(cfg->rel_threshold) && cfg->rel_threshold >= 0.0f)) return "rel_threshold is finite and >= 0";
    return nullptr;
}

inline float host_key(float x, int mode) { return mode == 0 ? std::fabs(x) : (mode == 1 ? x : -x); }
inline float host_low(float key) { return key == key ? key : -INFINITY; }

// thz_peak_map's offset around sample k
float host_vertex(const float *x, size_t nt, size_t k)
{
    if (k == 0 || k + 1 >= nt) return 0.0f;
    const float ym = x[k - 1], y0 = x[k], yp = x[k + 1];
    const float den = ym - 2.0f * y0 + yp;
    if (!(std::isfinite(ym) && std::isfinite(y0) && std::isfinite(yp) && den != 0.0f)) return 0.0f;
    const float off = 0.5f * (ym - yp) / den;
    return std::isfinite(off) ? std::fmin(std::fmax(off, -0.5f), 0.5f) : 0.0f;
}

}  // namespace

extern "C" {

int thz_host_echo_trace(const float *x, size_t nt, const thz_echo_cfg *cfg, int32_t *index, float *offset, float *value,
                        int32_t *count)
{
    if (!x || !cfg || echo_cfg_error(cfg, nt)) return THZ_ERR_INVALID;
    const int mode = cfg->mode, K = cfg->n_echoes;
    int64_t found[THZ_ECHO_MAX];
    int n = 0;
    // rank 0: thz_peak_map's winner
    {
        float best = -INFINITY;
        int64_t best_i = -1;
        for (size_t i = 0; i < nt; ++i) {
            const float key = host_key(x[i], mode);
            if (key > best) { best = key; best_i = (int64_t)i; }
        }
        if (best_i < 0) {  // nothing above -Inf: the first number, or sample 0 in a trace of NaNs
            best_i = 0;
            for (size_t i = 0; i < nt; ++i)
                if (x[i] == x[i]) { best_i = (int64_t)i; break; }
        }
        found[n++] = best_i;
    }
    const float thr = cfg->rel_threshold * host_key(x[found[0]], mode);
    for (int j = 1; j < K; ++j) {
        float best = -INFINITY;
        int64_t best_i = -1;
        for (size_t i = 0; i < nt; ++i) {
            const float key = host_key(x[i], mode);
            if (!(key >= thr)) continue;  // also a NaN key, also a NaN threshold
            if (i > 0 && !(key > host_low(host_key(x[i - 1], mode)))) continue;
            if (i + 1 < nt && !(key >= host_low(host_key(x[i + 1], mode)))) continue;
            bool far = true;
            for (int m = 0; m < n; ++m) {
                const int64_t d = (int64_t)i - found[m];
                far = far && (d < 0 ? -d : d) >= (int64_t)cfg->guard;
            }
            if (far && (best_i < 0 || key > best)) { best = key; best_i = (int64_t)i; }
        }
        if (best_i < 0) break;
        found[n++] = best_i;
    }
    for (int j = 0; j < K; ++j) {
        const bool have = j < n;
        if (index) index[j] = have ? (int32_t)found[j] : -1;
        if (offset) offset[j] = have ? host_vertex(x, nt, (size_t)found[j]) : 0.0f;
        if (value) value[j] = have ? x[found[j]] : 0.0f;
    }
    if (count) *count = n;
    return THZ_OK;
}

int thz_echo_map(thz_ctx *ctx, size_t npix, size_t nt, const float *d_data, const thz_echo_cfg *cfg, int32_t *d_index,
                 float *d_offset, float *d_value, int32_t *d_count)
{
    if (!ctx) return THZ_ERR_INVALID;
    if (int rc = use_device(ctx)) return rc;
    if (!d_data || !cfg) return fail(ctx, THZ_ERR_INVALID, "thz_echo_map: a required pointer is NULL");
    if (const char *why = echo_cfg_error(cfg, nt)) return fail(ctx, THZ_ERR_INVALID, std::string("thz_echo_map: ") + why);
    if (npix == 0 || (!d_index && !d_offset && !d_value && !d_count)) return THZ_OK;
    StageTimer t(ctx, THZ_STAGE_ECHO);
    launch_echo_map(ctx->stream, npix, (int)nt, d_data, cfg->mode, cfg->n_echoes, cfg->guard, cfg->rel_threshold, d_index,
                    d_offset, d_value, d_count);
    return check_launch(ctx);
}

int thz_layer_map(thz_ctx *ctx, size_t npix, int n_echoes, const int32_t *d_index, const float *d_offset,
                  const thz_layer_cfg *cfg, float *d_thickness, float *d_delay)
{
    if (!ctx) return THZ_ERR_INVALID;
    if (int rc = use_device(ctx)) return rc;
    if (!d_index || !d_offset || !cfg) return fail(ctx, THZ_ERR_INVALID, "thz_layer_map: a required pointer is NULL");
    if (cfg->mode < 0 || cfg->mode > 1 || n_echoes < 1 || n_echoes > THZ_ECHO_MAX || (cfg->mode == 0 && n_echoes < 2))
        return fail(ctx, THZ_ERR_INVALID, "thz_layer_map: mode is 0 (two echoes or more) or 1, 1 <= n_echoes <= THZ_ECHO_MAX");
    if (npix == 0 || (!d_thickness && !d_delay)) return THZ_OK;
    LayerGeom g{};
    g.mode = cfg->mode;
    g.n_echoes = n_echoes;
    for (int l = 0; l < 4; ++l) g.scale[l] = cfg->scale[l];
    g.ref_index = cfg->ref_index;
    g.ref_offset = cfg->ref_offset;
    StageTimer t(ctx, THZ_STAGE_ECHO);
    launch_layer_map(ctx->stream, npix, g, d_index, d_offset, d_thickness, d_delay);
    return check_launch(ctx);
}

int thz_session_echo_map(thz_session *s, int which, const thz_echo_cfg *cfg)
{
    if (!s) return THZ_ERR_INVALID;
    thz_ctx *ctx = s->ctx;
    if (int rc = use_device(ctx)) return rc;
    if (!cfg) return fail(ctx, THZ_ERR_INVALID, "thz_session_echo_map: cfg is NULL");
    SessionCube c;
    if (int rc = session_cube(s, which, &c)) return rc;
    if (const char *why = echo_cfg_error(cfg, c.nt)) return fail(ctx, THZ_ERR_INVALID, std::string("thz_session_echo_map: ") + why);
    const size_t npix = c.nx * c.ny, K = (size_t)cfg->n_echoes;
    // [index | offset | value: (K, npix) each, rank-major | count: npix]
    ResidentMaps &m = s->maps[kMapEcho];
    if (int rc = maps_begin(ctx, &m, {{K * npix}, {K * npix}, {K * npix}, {npix}})) return rc;
    if (int rc = thz_echo_map(ctx, npix, c.nt, c.d, cfg, m.ptr<int32_t>(0), m.ptr(1), m.ptr(2), m.ptr<int32_t>(3))) return rc;
    return maps_commit(ctx, &m);
}

int thz_session_layer_map(thz_session *s, const thz_layer_cfg *cfg)
{
    if (!s) return THZ_ERR_INVALID;
    thz_ctx *ctx = s->ctx;
    if (int rc = use_device(ctx)) return rc;
    if (!cfg) return fail(ctx, THZ_ERR_INVALID, "thz_session_layer_map: cfg is NULL");
    // the resident echo maps: one count per pixel, K indices per pixel
    const ResidentMaps &echo = s->maps[kMapEcho];
    const size_t npix = echo.entries(3);
    if (!npix) return fail(ctx, THZ_ERR_NOT_READY, "thz_session_layer_map: no echo map is resident (thz_session_echo_map)");
    const size_t K = echo.entries(0) / npix;
    if (cfg->mode < 0 || cfg->mode > 1 || (cfg->mode == 0 && K < 2))
        return fail(ctx, THZ_ERR_INVALID, "thz_session_layer_map: mode is 0 (an echo map of two ranks or more) or 1");
    const size_t rows = cfg->mode == 0 ? K - 1 : 1;
    // [thickness | delay], (rows, npix) each
    ResidentMaps &m = s->maps[kMapLayer];
    if (int rc = maps_begin(ctx, &m, {{rows * npix}, {rows * npix}})) return rc;
    if (int rc = thz_layer_map(ctx, npix, (int)K, echo.ptr<const int32_t>(0), echo.ptr(1), cfg, m.ptr(0), m.ptr(1))) return rc;
    return maps_commit(ctx, &m);
}

}  // extern "C"
