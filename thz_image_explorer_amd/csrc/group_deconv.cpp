// group_deconv.cpp — thz_group_session_deconvolve (group.hpp): the Deconvolution stage over a group's slabs, its
// per-pixel parts on every member's own rows and its Richardson-Lucy iterations dealt out band by band.
#include "group.hpp"

#include <algorithm>
#include <cstring>

using namespace thz;

// The bands' iteration counts and tile counts (host arithmetic, identical on every rank) -> contiguous band ranges:
// rank q iterates the bands [band0[q], band0[q + 1]).  costs: per band {iterations, iterations x tiles}.
// A range's iterations run as chains of dependent launches: its time is about alpha x (its longest band's
// iterations) + beta x (sum of iterations x tiles) — alpha = 13.2 us per iteration (two launches end to end),
// beta = 20 ns per tile and iteration, fitted to the widest band alone at 128 x 128 and 512 x 512 pixels
// (profiles/r03_deconv_group_estimate.txt).  The ranges minimise the slowest rank's time (dynamic programme over
// the cut points; a rank may stay without a band when there are more ranks than bands).
std::vector<size_t> dc_band_ranges(const std::vector<double> &costs, int world)
{
    const size_t W = (size_t)world, nb = costs.size() / 2;
    const double alpha = 13.2, beta = 0.0204;
    auto range_cost = [&](size_t a, size_t b) {  // bands [a, b)
        double it = 0.0, w = 0.0;
        for (size_t k = a; k < b; ++k) {
            it = std::max(it, costs[2 * k]);
            w += costs[2 * k + 1];
        }
        return alpha * it + beta * w;
    };
    // best[q][b]: the smallest possible slowest-rank time when ranks 0 .. q-1 share the bands [0, b)
    std::vector<std::vector<double>> best(W + 1, std::vector<double>(nb + 1, 1e300));
    std::vector<std::vector<size_t>> cut(W + 1, std::vector<size_t>(nb + 1, 0));
    best[0][0] = 0.0;
    for (size_t q = 1; q <= W; ++q)
        for (size_t b = 0; b <= nb; ++b)
            for (size_t a = 0; a <= b; ++a) {
                if (best[q - 1][a] >= 1e300) continue;
                const double v = std::max(best[q - 1][a], range_cost(a, b));
                if (v < best[q][b]) { best[q][b] = v; cut[q][b] = a; }
            }
    std::vector<size_t> band0(W + 1, 0);
    size_t b = nb;
    for (size_t q = W; q >= 1; --q) {
        band0[q] = b;
        b = cut[q][b];
    }
    return band0;
}

// what a phase that failed somewhere in the group returns on this rank: a local member's own code (the last one;
// with abort_counts == false an abort does not count as one), or `otherwise` when the failure was another rank's
static int phase_status(const std::vector<int> &rcs, int otherwise, bool abort_counts)
{
    int status = otherwise;
    for (int rc : rcs)
        if (rc < 0 && (abort_counts || rc != THZ_ERR_ABORTED)) status = rc;
    return status;
}

// ---- several slabs (round 3).  The stage has three parts with two different independences: the transform, the band
// energies and the recombination are per PIXEL (every band), the Richardson-Lucy iterations are per BAND (the
// whole image).  So every member does the per-pixel parts for its own rows and the iterations for its own bands,
// and what crosses the fabric is two sets of 2-D images — n_filters x Nx x Ny energies out, as many gains back —
// instead of round 2's all-gather and all-reduce of the whole cube (2 x Nx Ny Nt floats per member, and two
// whole-cube buffers on every GPU): SURVEY 8e's alternative.
//   A  thz_dc_slab_energies      own rows, every band                      -> E_slab [nb][npix_slab]
//   X1 all-gather of the E_slab blocks; a member keeps its bands' images    -> E_mine [bands][npix]
//   B  thz_dc_band_gains          own bands (dealt out by cost), whole grid -> G_mine [bands][npix]
//   X2 all-gather of the G_mine blocks (rank order = band order); a member keeps its rows' columns -> G_slab
//   C  thz_dc_slab_combine        own rows, every band                      -> the slab of the stage's output
// A guard (the same on every rank) or an abort / error on any rank makes every slab keep its input.
// *status: what the call returns once the regions of interest have followed — THZ_OK, THZ_SKIPPED or, from the first
// phase that failed on any rank, this rank's code for it.  A non-zero return is a failure of the orchestration itself.
static int dc_slabs(thz_group_session *gs, const thz_psf *psf, const thz_deconv_cfg *cfg, volatile const int *abort_flag, float *progress, int *status)
{
    thz_group *g = gs->g;
    const size_t nl = gs->sess.size();
    std::vector<size_t> cur_x0((size_t)g->world, 0);
    for (int q = 1; q < g->world; ++q) cur_x0[(size_t)q] = cur_x0[(size_t)q - 1] + gs->cur_rows[(size_t)q - 1];
    const size_t grid_ny = gs->cur_ny, npix_all = gs->cur_pix(), grid_nx = npix_all / (grid_ny ? grid_ny : 1);
    const size_t nt = gs->nt_out;
    const size_t nb = cfg->n_filters;
    auto rank_pix = [&](size_t q) { return gs->cur_rows[q] * grid_ny; };
    auto pix_of = [&](size_t i) { return rank_pix((size_t)g->m[i].rank); };
    // the members' engines on the chain's current axis
    if (int rc = each_member(g, "", [&](size_t i) {
            thz_ctx *ctx = g->m[i].ctx;
            thz_session *s = gs->sess[i];
            const bool same = ctx->time.size() == nt && std::memcmp(ctx->time.data(), s->time_out.data(), nt * sizeof(float)) == 0;
            return same ? (int)THZ_OK : thz_set_time_axis(ctx, s->time_out.data(), nt);
        }))
        return rc;
    // ---- costs -> ranges (the reference's guards — no bands, a grid smaller than the widest PSF ... — are
    // rank-independent too)
    std::vector<double> costs;
    const int rc_costs = thz_dc_band_costs(g->m[0].ctx, psf, cfg, grid_nx, grid_ny, gs->sess[0]->dx_cur, gs->sess[0]->dy_cur, &costs);
    if (rc_costs < 0) return gfail(g, rc_costs, std::string("thz_group_session_deconvolve: ") + thz_last_error(g->m[0].ctx));
    const bool skipped = rc_costs == THZ_SKIPPED || costs.size() != 2 * nb;
    const std::vector<size_t> band0 = skipped ? std::vector<size_t>((size_t)g->world + 1, 0) : dc_band_ranges(costs, g->world);
    // per local member, freed however the call ends: A's energies, later X2's gains of the own rows [nb][npix_slab] |
    // what an all-gather delivers | the own bands' energies | the own bands' gains [bands][npix] | group_any_failed's float
    std::vector<float *> bufA(nl, nullptr), bufB(nl, nullptr), bufC(nl, nullptr), bufD(nl, nullptr), flag(nl, nullptr);
    CallBufs bufs(g);
    // every member's slab output buffers (the stage's result replaces the final cube / image until the next recompute)
    for (size_t i = 0; i < nl; ++i) {
        thz_session *s = gs->sess[i];
        GHIP_TRY(g, hipSetDevice(g->m[i].ctx->device));
        if (int rc = session_size_deconv(s)) return gfail(g, rc, std::string("thz_group_session_deconvolve: ") + thz_last_error(s->ctx));
        if (int rc = bufs.alloc(i, &flag[i], sizeof(float), "thz_group_session_deconvolve: allocation failed")) return rc;
    }
    std::vector<int> rcs;
    bool bad = false;
    *status = skipped ? THZ_SKIPPED : THZ_OK;
    if (!skipped) {
        const char *msg = "thz_group_session_deconvolve: allocation of the band images failed";
        for (size_t i = 0; i < nl; ++i) {
            GHIP_TRY(g, hipSetDevice(g->m[i].ctx->device));
            const size_t q = (size_t)g->m[i].rank, nbs = band0[q + 1] - band0[q];
            int rc = bufs.alloc(i, &bufA[i], std::max<size_t>(nb * rank_pix(q), 4) * sizeof(float), msg);
            if (!rc) rc = bufs.alloc(i, &bufB[i], std::max<size_t>(nb * npix_all, 4) * sizeof(float), msg);
            if (!rc) rc = bufs.alloc(i, &bufC[i], std::max<size_t>(nbs * npix_all, 4) * sizeof(float), msg);
            if (!rc) rc = bufs.alloc(i, &bufD[i], std::max<size_t>(nbs * npix_all, 4) * sizeof(float), msg);
            if (rc) return rc;
        }
        // ---- A: own rows, every band
        members_in_parallel(g, [&](size_t i) {
            thz_session *s = gs->sess[i];
            return thz_dc_slab_energies(g->m[i].ctx, psf, cfg, grid_nx, grid_ny, s->dx_cur, s->dy_cur, s->d_data, pix_of(i), bufA[i]);
        }, rcs);
        if (int rc = group_any_failed(g, rcs, flag.data(), &bad)) return rc;
        if (bad) *status = phase_status(rcs, THZ_ERR_HIP, true);
    }
    if (!skipped && !bad) {
        // ---- X1: every slab's [nb][npix_slab] block to everybody; a member re-tiles its bands' rows into whole images
        std::vector<size_t> counts((size_t)g->world);
        for (int q = 0; q < g->world; ++q) counts[(size_t)q] = nb * rank_pix((size_t)q);
        const std::vector<size_t> off = offsets(counts.data(), g->world);
        if (int rc = group_all_gather(g, bufA.data(), counts.data(), bufB.data())) return rc;
        for (size_t i = 0; i < nl; ++i) {
            GHIP_TRY(g, hipSetDevice(g->m[i].ctx->device));
            const size_t me = (size_t)g->m[i].rank, b_lo = band0[me], nbs = band0[me + 1] - b_lo;
            for (int q = 0; q < g->world && nbs; ++q) {
                const size_t pq = rank_pix((size_t)q);
                if (pq)
                    GHIP_TRY(g, hipMemcpy2DAsync(bufC[i] + cur_x0[(size_t)q] * grid_ny, npix_all * sizeof(float), bufB[i] + off[(size_t)q] + b_lo * pq,
                                                 pq * sizeof(float), pq * sizeof(float), nbs, hipMemcpyDeviceToDevice, g->m[i].ctx->stream));
            }
        }
        if (int rc = thz_group_sync(g)) return rc;
        // ---- B: own bands, whole grid
        members_in_parallel(g, [&](size_t i) {
            thz_session *s = gs->sess[i];
            const size_t me = (size_t)g->m[i].rank;
            thz_deconv_cfg c = *cfg;
            c.band_begin = (uint32_t)band0[me];
            c.band_end = (uint32_t)band0[me + 1];
            if (c.band_begin == c.band_end) return (int)THZ_OK;  // more ranks than bands
            return thz_dc_band_gains(g->m[i].ctx, psf, &c, grid_nx, grid_ny, s->dx_cur, s->dy_cur, bufC[i], bufD[i], abort_flag, i == 0 ? progress : nullptr);
        }, rcs);
        if (int rc = group_any_failed(g, rcs, flag.data(), &bad)) return rc;
        if (bad) *status = phase_status(rcs, THZ_ERR_ABORTED, false);
    }
    if (!skipped && !bad) {
        // ---- X2: the ranks' [bands][npix] gain blocks, in rank order = band order -> [nb][npix] on everybody; a member
        // keeps the columns of its own rows
        std::vector<size_t> counts((size_t)g->world);
        for (int q = 0; q < g->world; ++q) counts[(size_t)q] = (band0[(size_t)q + 1] - band0[(size_t)q]) * npix_all;
        if (int rc = group_all_gather(g, bufD.data(), counts.data(), bufB.data())) return rc;
        for (size_t i = 0; i < nl; ++i) {
            GHIP_TRY(g, hipSetDevice(g->m[i].ctx->device));
            const size_t me = (size_t)g->m[i].rank, pq = rank_pix(me);
            if (pq)
                GHIP_TRY(g, hipMemcpy2DAsync(bufA[i], pq * sizeof(float), bufB[i] + cur_x0[me] * grid_ny, npix_all * sizeof(float), pq * sizeof(float), nb,
                                             hipMemcpyDeviceToDevice, g->m[i].ctx->stream));
        }
        if (int rc = thz_group_sync(g)) return rc;
        // ---- C: own rows, every band
        members_in_parallel(g, [&](size_t i) {
            thz_session *s = gs->sess[i];
            return thz_dc_slab_combine(g->m[i].ctx, psf, cfg, grid_nx, grid_ny, s->dx_cur, s->dy_cur, pix_of(i), bufA[i], s->d_deconv, s->d_deconv_img);
        }, rcs);
        if (int rc = group_any_failed(g, rcs, flag.data(), &bad)) return rc;
        if (bad) *status = phase_status(rcs, THZ_ERR_HIP, true);
    }
    if (skipped || bad) {
        // the stage passes its input through: every slab keeps its own "Time Band Pass" output
        for (size_t i = 0; i < nl; ++i) {
            thz_session *s = gs->sess[i];
            thz_ctx *ctx = g->m[i].ctx;
            GHIP_TRY(g, hipSetDevice(ctx->device));
            const size_t pq = pix_of(i);
            GHIP_TRY(g, hipMemcpyAsync(s->d_deconv, s->d_data, pq * nt * sizeof(float), hipMemcpyDeviceToDevice, ctx->stream));
            if (int rc = thz_intensity(ctx, pq, s->d_deconv, s->d_deconv_img)) return gfail(g, rc, thz_last_error(ctx));
        }
    }
    for (thz_session *s : gs->sess) s->deconv_current = *status >= 0;
    // C1: the new image (and, if the last recompute gathered it, the new final cube) to rank 0
    std::vector<const float *> im, dat;
    std::vector<size_t> ic((size_t)g->world), dc((size_t)g->world);
    for (int q = 0; q < g->world; ++q) {
        ic[(size_t)q] = rank_pix((size_t)q);
        dc[(size_t)q] = rank_pix((size_t)q) * nt;
    }
    for (thz_session *s : gs->sess) {
        im.push_back(s->deconv_current ? s->d_deconv_img : s->d_img);
        dat.push_back(s->deconv_current ? s->d_deconv : s->d_data);
    }
    if (int rc = thz_group_gather(g, im.data(), ic.data(), gs->d_img)) return rc;
    if (gs->gathered >= THZ_GATHER_TIME && (gs->root_local < 0 || gs->d_data))
        if (int rc = thz_group_gather(g, dat.data(), dc.data(), gs->d_data)) return rc;
    return THZ_OK;
}

extern "C" int thz_group_session_deconvolve(thz_group_session *gs, const thz_psf *psf, const thz_deconv_cfg *cfg,
                                            volatile const int *abort_flag, float *progress)
{
    if (!gs || !psf || !cfg) return THZ_ERR_INVALID;
    thz_group *g = gs->g;
    for (thz_session *s : gs->sess)
        if (!s->have_outputs) return gfail(g, THZ_ERR_NOT_READY, "thz_group_session_deconvolve: no recompute has run");
    if (one_slab(g)) {
        // one slab = the whole grid: the session's own stage (no gather of the cube, no second copy of it), then C1
        const int rc = thz_session_deconvolve(gs->sess[0], psf, cfg, abort_flag, progress);
        if (rc < 0) return gfail(g, rc, std::string("thz_group_session_deconvolve: ") + thz_last_error(g->m[0].ctx));
        thz_session *s = gs->sess[0];
        const size_t npix = s->nx_cur * s->ny_cur;
        GHIP_TRY(g, hipSetDevice(g->m[0].ctx->device));
        GHIP_TRY(g, hipMemcpyAsync(gs->d_img, thz_session_buffer(s, THZ_BUF_IMG), npix * sizeof(float), hipMemcpyDeviceToDevice, g->m[0].ctx->stream));
        if (gs->gathered >= THZ_GATHER_TIME && gs->d_data)
            GHIP_TRY(g, hipMemcpyAsync(gs->d_data, thz_session_buffer(s, THZ_BUF_DATA), npix * gs->nt_out * sizeof(float), hipMemcpyDeviceToDevice,
                                       g->m[0].ctx->stream));
        if (int rc2 = thz_group_sync(g)) return rc2;
        return rc;
    }
    int status = THZ_OK;
    if (int rc = dc_slabs(gs, psf, cfg, abort_flag, progress, &status)) return rc;
    // the regions of interest's means of the FINAL traces follow the stage's output (data_thread.rs:1445-1451)
    if (!gs->sess[0]->rois.empty() && gs->sess[0]->have_last_cfg) {
        if (int rc = group_roi_tail(gs, nullptr, true)) return rc;
        if (int rc = thz_group_sync(g)) return rc;
    }
    if (status < 0) return gfail(g, status, "thz_group_session_deconvolve: aborted or failed on a rank; the stage passes its input through");
    return status;
}
