// group_tilt.cpp — thz_group_session_estimate_tilt (group.hpp): the arrival plane of the whole grid of a group session
// (include/thzgpu.h).  Every member maps its own slab; what crosses the fabric is three 2-D images to rank 0 and nine
// words back.
#include "group.hpp"

#include <cstring>

using namespace thz;

extern "C" {

int thz_group_session_estimate_tilt(thz_group_session *gs, int which, int mode, float rel_threshold, thz_tilt_fit *out)
{
    // arguments and state every rank checks alike, before any collective
    if (!gs || !out) return THZ_ERR_INVALID;
    *out = thz_tilt_fit{};
    thz_group *g = gs->g;
    const size_t nl = gs->sess.size(), W = (size_t)g->world;
    if (mode < 0 || mode > 2) return gfail(g, THZ_ERR_INVALID, "thz_group_session_estimate_tilt: mode is 0, 1 or 2");
    SessionCube c0;
    for (size_t i = 0; i < nl; ++i) {
        SessionCube c;
        if (int rc = session_cube(gs->sess[i], which, &c))
            return gfail(g, rc, std::string("thz_group_session_estimate_tilt: ") + thz_last_error(g->m[i].ctx));
        if (i == 0) c0 = c;
    }
    // the whole grid the slabs' maps make up, in rank order
    // (the spike trains and the denoised traces lie on the grid of the cube they were taken of: the raw one when the first
    // local member's do)
    const bool taken = which == THZ_BUF_SPARSE || which == THZ_BUF_DENOISED;
    const bool raw_grid = which == THZ_BUF_RAW
                          || (taken && nl > 0 && c0.ny == gs->ny && c0.nx == gs->rows[(size_t)g->m[0].rank]);
    const std::vector<size_t> &rows = raw_grid ? gs->rows : gs->cur_rows;
    const size_t ny = raw_grid ? gs->ny : gs->cur_ny;
    for (size_t i = 0; taken && i < nl; ++i) {
        SessionCube c;
        (void)session_cube(gs->sess[i], which, &c);
        if (c.nx != rows[(size_t)g->m[i].rank] || c.ny != ny)
            return gfail(g, THZ_ERR_INVALID, "thz_group_session_estimate_tilt: the members' traces are not slabs of one grid");
    }
    size_t nx = 0;
    std::vector<size_t> counts(W);
    for (size_t q = 0; q < W; ++q) {
        nx += rows[q];
        counts[q] = rows[q] * ny;
    }
    const size_t npix = nx * ny;
    constexpr size_t kWords = 9;  // the fit's six doubles, its count and the code rank 0 returns
    std::vector<uint64_t *> d_scr(nl, nullptr);
    CallBufs bufs(g);
    for (size_t i = 0; i < nl; ++i) {
        GHIP_TRY(g, hipSetDevice(g->m[i].ctx->device));
        if (int rc = bufs.alloc(i, &d_scr[i], kWords * sizeof(uint64_t), "thz_group_session_estimate_tilt: scratch allocation failed")) return rc;
    }
    if (gs->root_local >= 0) {
        thz_ctx *ctx = g->m[(size_t)gs->root_local].ctx;
        GHIP_TRY(g, hipSetDevice(ctx->device));
        if (int rc = gs->d_peak.grow(ctx, 3 * npix)) return gfail(g, rc, std::string("thz_group_session_estimate_tilt: ") + thz_last_error(ctx));
    }
    gs->peak_pix = 0;
    if (int rc = each_member(g, "slab arrival times: ", [&](size_t i) { return thz_session_peak_map(gs->sess[i], which, mode); })) return rc;
    // C1: index (as its bits) | offset | value, each a whole-grid image on rank 0
    const int bufs_of[3] = {THZ_BUF_PEAK_INDEX, THZ_BUF_PEAK_OFFSET, THZ_BUF_PEAK_VALUE};
    for (int b = 0; b < 3; ++b) {
        std::vector<const float *> send;
        for (thz_session *s : gs->sess) send.push_back(static_cast<const float *>(session_buffer_ro(s, bufs_of[b])));
        if (int rc = thz_group_gather(g, send.data(), counts.data(), gs->d_peak ? gs->d_peak + (size_t)b * gs->peak_stride() : nullptr)) return rc;
    }
    // rank 0: the same moments kernels and the same fit a single session runs.  Whatever happens here, rank 0 goes on
    // to the all-reduce — its code travels with the result, so that no rank waits for one that has left.
    uint64_t words[kWords] = {0};
    if (gs->root_local >= 0) {
        thz_ctx *ctx = g->m[(size_t)gs->root_local].ctx;
        GHIP_TRY(g, hipSetDevice(ctx->device));
        double m[10];
        thz_tilt_fit fit{};
        int rc = thz_arrival_plane_moments(ctx, nx, ny, c0.dx, c0.dy, c0.dt_ps, gs->d_peak.as<const int32_t>(),
                                           gs->d_peak + gs->peak_stride(), gs->d_peak + 2 * gs->peak_stride(), rel_threshold, m);
        if (rc) gfail(g, rc, std::string("thz_group_session_estimate_tilt: ") + thz_last_error(ctx));
        else rc = thz_host_arrival_plane_fit(m, &fit);
        const double d[6] = {fit.tilt_x_deg, fit.tilt_y_deg, fit.slope_x_ps_per_mm, fit.slope_y_ps_per_mm, fit.t0_ps, fit.rms_ps};
        std::memcpy(words, d, 6 * sizeof(double));
        words[6] = fit.n_used;
        words[7] = (uint64_t)(uint32_t)(int32_t)rc;
        words[8] = 1;  // rank 0 spoke
    }
    for (size_t i = 0; i < nl; ++i) {
        thz_ctx *ctx = g->m[i].ctx;
        GHIP_TRY(g, hipSetDevice(ctx->device));
        if ((int)i == gs->root_local) GHIP_TRY(g, hipMemcpyAsync(d_scr[i], words, sizeof words, hipMemcpyHostToDevice, ctx->stream));
        else GHIP_TRY(g, hipMemsetAsync(d_scr[i], 0, sizeof words, ctx->stream));
    }
    if (int rc = thz_group_all_reduce_u64(g, d_scr.data(), kWords)) return rc;
    uint64_t got[kWords];
    GHIP_TRY(g, hipSetDevice(g->m[0].ctx->device));
    GHIP_TRY(g, hipMemcpyAsync(got, d_scr[0], sizeof got, hipMemcpyDeviceToHost, g->m[0].ctx->stream));
    if (int rc = thz_group_sync(g)) return rc;
    if (got[8] != 1) return gfail(g, THZ_ERR_HIP, "thz_group_session_estimate_tilt: rank 0's result did not arrive");
    const int code = (int)(int32_t)(uint32_t)got[7];
    if (code < 0) return gfail(g, code, g->err.empty() ? "thz_group_session_estimate_tilt: failed on rank 0" : g->err);
    std::memcpy(out, got, 6 * sizeof(double));  // the struct's six leading doubles
    out->n_used = got[6];
    gs->peak_pix = npix;
    return code;
}

void *thz_group_session_peak_result(thz_group_session *gs, int which)
{
    if (!gs || gs->root_local < 0 || !gs->peak_pix || !gs->d_peak) return nullptr;
    switch (which) {
    case THZ_BUF_PEAK_INDEX: return gs->d_peak;
    case THZ_BUF_PEAK_OFFSET: return gs->d_peak + gs->peak_stride();
    case THZ_BUF_PEAK_VALUE: return gs->d_peak + 2 * gs->peak_stride();
    default: return nullptr;
    }
}

}  // extern "C"
