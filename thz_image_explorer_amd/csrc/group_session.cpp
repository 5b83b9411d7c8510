// group_session.cpp — the session behind thz_group_session* (group.hpp): one resident-cube session per x-slab,
// recomputed side by side on the members' streams, with the exchanges the chain needs between them (block sums over
// slab edges, the means, the regions of interest) and the gather of the results on rank 0.
#include "group.hpp"

#include <memory>

using namespace thz;

// want_means == 2 over several slabs: the reference's means are SEQUENTIAL sums over all x rows (ndarray mean_axis on
// axis 0, then on the next: math_tools.rs:421-440), so the slabs take turns in rank order — each continues the running
// sums of the slabs in front of it (k_sum_axis0's carry) and hands them on; the last one divides by nx, sums over y,
// divides by ny; the result reaches every member through an all-reduce in which all others add zeros.  Bit for bit
// one session's means; serial by construction — this mode is for comparing against the reference, not for speed.
static int group_means_reference_order(thz_group_session *gs)
{
    thz_group *g = gs->g;
    const size_t nl = gs->sess.size(), nt = gs->nt_out, nf = nt / 2 + 1, ny = gs->cur_ny;
    size_t nx_total = 0;
    for (size_t v : gs->cur_rows) nx_total += v;
    std::vector<float *> run(nl, nullptr), avg(nl, nullptr);
    CallBufs bufs(g);
    for (size_t i = 0; i < nl; ++i) {
        GHIP_TRY(g, hipSetDevice(g->m[i].ctx->device));
        if (int rc = bufs.alloc(i, &run[i], ny * 2 * nf * sizeof(float), "reference-order means: allocation failed")) return rc;
        avg[i] = gs->sess[i]->d_avg;
        if (hipMemsetAsync(avg[i], 0, 4 * nf * sizeof(float), g->m[i].ctx->stream) != hipSuccess) return gfail(g, THZ_ERR_HIP, "memset");
    }
    struct Arr { size_t L, off; int which; };
    const Arr arrs[3] = {{2 * nf, 0, 0}, {nf, 2 * nf, 1}, {nf, 3 * nf, 2}};
    int rc = THZ_OK;
    for (const Arr &a : arrs) {
        for (int q = 0; q < g->world && !rc; ++q) {
            if (q > 0) rc = group_p2p(g, q - 1, q, run.data(), run.data(), ny * a.L);
            for (size_t i = 0; i < nl && !rc; ++i) {
                if (g->m[i].rank != q) continue;
                thz_session *s = gs->sess[i];
                const float *arr = a.which == 0 ? s->d_fft : (a.which == 1 ? s->d_amp : s->d_ph);
                if (hipSetDevice(g->m[i].ctx->device) != hipSuccess) { rc = THZ_ERR_HIP; break; }
                const bool last = q == g->world - 1;
                launch_sum_axis0(g->m[i].ctx->stream, arr, gs->cur_rows[(size_t)q], ny * a.L, last ? (float)nx_total : 0.0f, run[i], q > 0 ? run[i] : nullptr);
                if (last) launch_sum_axis0(g->m[i].ctx->stream, run[i], ny, a.L, (float)ny, avg[i] + a.off);
                if (hipGetLastError() != hipSuccess) rc = THZ_ERR_HIP;
            }
        }
        if (rc) break;
    }
    if (!rc) rc = thz_group_all_reduce_sum(g, avg.data(), 4 * nf);  // everybody but the last rank holds zeros
    if (rc) return gfail(g, rc, "reference-order means over the slabs failed");
    for (thz_session *s : gs->sess) s->have_means = true;
    return THZ_OK;
}

// all-reduce of the members' region sums (session_roi.cpp's block layout: the final traces' block is the last
// R x nt floats — the only one a tail-only recompute or the Deconvolution stage renews)
static int group_roi_reduce(thz_group_session *gs, std::vector<float *> &bufs, bool data_only)
{
    thz_session *s0 = gs->sess[0];
    const size_t total = session_roi_floats(s0), fin = s0->rois.size() * s0->nt_out, spec = 2 * s0->rois.size() * s0->nf_out;
    std::vector<float *> tail(bufs);
    for (float *&b : tail) b += total - fin;
    if (data_only) return thz_group_all_reduce_sum(gs->g, tail.data(), fin);
    if (s0->roi_src_fresh) return thz_group_all_reduce_sum(gs->g, bufs.data(), total);
    // the source traces' block in the middle holds the grid's sums of an earlier recompute: left alone
    if (int rc = thz_group_all_reduce_sum(gs->g, bufs.data(), spec)) return rc;
    return thz_group_all_reduce_sum(gs->g, tail.data(), fin);
}

int group_roi_tail(thz_group_session *gs, const thz_chain_cfg *cfg, bool data_only)
{
    thz_group *g = gs->g;
    auto cfg_of = [&](size_t i) { return cfg ? cfg : &gs->sess[i]->last_cfg; };
    std::vector<float *> bufs;
    if (int rc = each_member(g, "slab regions of interest: ", [&](size_t i) { return session_roi_sums(gs->sess[i], cfg_of(i), &data_only); })) return rc;
    for (thz_session *s : gs->sess) bufs.push_back(s->d_roi_sum);
    if (int rc = group_roi_reduce(gs, bufs, data_only)) return rc;
    return each_member(g, "slab regions of interest: ", [&](size_t i) { return session_roi_finish(gs->sess[i], cfg_of(i), data_only); });
}

// C2: the slabs' undivided amplitude / phase sums -> the cube's, on every member
static int group_means(thz_group_session *gs, const thz_chain_cfg *cfg, bool single)
{
    thz_group *g = gs->g;
    thz_session *s0 = gs->sess[0];
    const size_t nt_out = gs->nt_out, nf = nt_out / 2 + 1;
    auto means_of = [&](size_t total_pix) {
        return each_member(g, "slab means: ", [&](size_t i) {
            const int rc = session_means(gs->sess[i], cfg, total_pix);
            return rc ? rc : session_avg_data(gs->sess[i], cfg);
        });
    };
    const bool additive = s0->msum_fast || s0->msum_passes;
    // the whole grid in one slab, means in the reference's order: nothing to exchange
    if (!additive && single) return means_of(s0->nx_cur * s0->ny_cur);
    if (!additive) {
        if (int rc = group_means_reference_order(gs)) return rc;
        return each_member(g, "slab means: ", [&](size_t i) { return session_avg_data(gs->sess[i], cfg); });
    }
    std::vector<float *> bufs;
    // amplitude / phase sums of the fused launch (2 nf), or — a tilted cube — spectrum, amplitude and phase sums
    // (4 nf).  The sum of the SOURCE traces in front of them (avg_fft follows from it by linearity) was all-reduced
    // at upload for the raw cube; a block-averaged or re-laid (tilted) source's is the slab's own and goes along.
    const bool src_too = s0->src_sum_own;
    for (thz_session *s : gs->sess) bufs.push_back(src_too ? s->d_msum : s->d_msum + nt_out);
    const size_t count = (s0->msum_passes ? 4 * nf : 2 * nf) + (src_too ? nt_out : 0);
    if (int rc = thz_group_all_reduce_sum(g, bufs.data(), count)) return rc;
    // Σ of the raw traces was all-reduced at upload; the copy in d_msum[0, nt) is already the cube's
    return means_of(gs->cur_pix());
}

// C1: one per-pixel result to rank 0, whose buffer grows when it is too small
static int gather_buf(thz_group_session *gs, int which, size_t per_pix, DevBuf<float> *d_dst)
{
    thz_group *g = gs->g;
    std::vector<const float *> send;
    std::vector<size_t> counts((size_t)g->world);
    for (int q = 0; q < g->world; ++q) counts[(size_t)q] = gs->cur_rows[(size_t)q] * gs->cur_ny * per_pix;
    for (thz_session *s : gs->sess) send.push_back(static_cast<const float *>(session_buffer_ro(s, which)));
    if (gs->root_local >= 0) {  // (a tilted cube's outputs are longer than the raw traces)
        thz_ctx *ctx = g->m[(size_t)gs->root_local].ctx;
        GHIP_TRY(g, hipSetDevice(ctx->device));
        if (int rc = d_dst->grow(ctx, gs->cur_pix() * per_pix)) return gfail(g, rc, std::string("gathered results: ") + thz_last_error(ctx));
    }
    return thz_group_gather(g, send.data(), counts.data(), *d_dst);
}

extern "C" {

void thz_group_session_destroy(thz_group_session *gs)
{
    if (!gs) return;
    for (thz_session *s : gs->sess) thz_session_destroy(s);
    if (gs->root_local >= 0) (void)hipSetDevice(gs->g->m[(size_t)gs->root_local].ctx->device);
    delete gs;
}

int thz_group_session_create(thz_group *g, size_t nx, size_t ny, size_t nt, const float *time, float dx, float dy,
                             thz_group_session **out)
{
    if (!g || !out || !time || ny == 0 || nt < 2) return THZ_ERR_INVALID;
    *out = nullptr;
    if (nx < (size_t)g->world) return gfail(g, THZ_ERR_INVALID, "fewer x rows than ranks: every slab needs at least one row");
    std::unique_ptr<thz_group_session, void (*)(thz_group_session *)> own(new thz_group_session(), thz_group_session_destroy);
    thz_group_session *gs = own.get();  // (destroyed again by whichever return comes before the release below)
    gs->g = g; gs->nx = nx; gs->ny = ny; gs->nt = nt; gs->nt_out = nt;
    gs->x0.resize((size_t)g->world);
    gs->rows.resize((size_t)g->world);
    for (int q = 0; q < g->world; ++q) (void)thz_host_slab(nx, g->world, q, &gs->x0[(size_t)q], &gs->rows[(size_t)q]);
    gs->root_local = local_of_rank(g, 0);
    if (int rc = each_member(g, "slab session: ", [&](size_t i) {
            thz_session *s = nullptr;
            if (int rc = thz_session_create(g->m[i].ctx, gs->rows[(size_t)g->m[i].rank], ny, nt, time, dx, dy, &s)) return rc;
            // where the slab sits in the whole grid: the Tilt plan, block means over slab edges and the regions of
            // interest depend on it (session_enqueue derives the current grid's placement from these)
            s->raw_grid_x0 = gs->x0[(size_t)g->m[i].rank];
            s->raw_grid_rows = nx;
            s->slab_rank = g->m[i].rank;
            s->slab_world = g->world;
            s->grid_x0 = s->raw_grid_x0;
            s->grid_rows = nx;
            gs->sess.push_back(s);
            return (int)THZ_OK;
        }))
        return rc;
    gs->cur_rows = gs->rows;
    gs->cur_ny = ny;
    if (gs->root_local >= 0) {
        thz_ctx *ctx = g->m[(size_t)gs->root_local].ctx;
        if (hipSetDevice(ctx->device) != hipSuccess || gs->d_img.grow(ctx, nx * ny))
            return gfail(g, THZ_ERR_HIP, "gathered image: allocation failed");
    }
    *out = own.release();
    return THZ_OK;
}

thz_session *thz_group_session_member(thz_group_session *gs, int i)
{
    return (gs && i >= 0 && i < (int)gs->sess.size()) ? gs->sess[(size_t)i] : nullptr;
}

int thz_group_session_upload(thz_group_session *gs, const float *cube, int subtract_bias)
{
    if (!gs) return THZ_ERR_INVALID;
    thz_group *g = gs->g;
    std::vector<float *> sums;
    auto slab_of = [&](size_t i) { return cube ? cube + gs->x0[(size_t)g->m[i].rank] * gs->ny * gs->nt : nullptr; };
    if (int rc = each_member(g, "slab upload: ", [&](size_t i) { return thz_session_upload(gs->sess[i], slab_of(i), subtract_bias); })) return rc;
    for (thz_session *s : gs->sess) sums.push_back(s->d_rawsum);
    // the slabs' raw pixel sums become the cube's: avg_fft of every later recompute follows from them
    if (int rc = thz_group_all_reduce_sum(g, sums.data(), gs->nt)) return rc;
    gs->gathered = -1;
    return thz_group_sync(g);
}

int thz_group_session_set_rois(thz_group_session *gs, size_t n_rois, const size_t *n_vertices, const uint64_t *poly_xy)
{
    if (!gs) return THZ_ERR_INVALID;
    return each_member(gs->g, "slab regions of interest: ", [&](size_t i) { return thz_session_set_rois(gs->sess[i], n_rois, n_vertices, poly_xy); });
}

int thz_group_session_roi(thz_group_session *gs, size_t roi, const thz_roi_out *out)
{
    if (!gs || gs->sess.empty()) return THZ_ERR_INVALID;
    const int rc = thz_session_roi(gs->sess[0], roi, out);
    if (rc) return gfail(gs->g, rc, std::string("thz_group_session_roi: ") + thz_last_error(gs->g->m[0].ctx));
    return rc;
}

int thz_group_session_recompute(thz_group_session *gs, const thz_chain_cfg *cfg, int start_stage, int gather)
{
    if (!gs || !cfg) return THZ_ERR_INVALID;
    thz_group *g = gs->g;
    if (gather < THZ_GATHER_SMALL || gather > THZ_GATHER_ALL || start_stage < 0 || start_stage > 8)
        return gfail(g, THZ_ERR_INVALID, "thz_group_session_recompute: bad gather level or chain position");
    const bool single = g->world == 1;  // one slab = the whole grid
    if (start_stage == 8) return THZ_OK;
    // Scaling over slab edges (round 3): a block's rows may lie in two slabs.  Every slab sums the first rows of the
    // block it cannot finish and hands the partial sums to the next slab, which continues the sequence — the block
    // belongs to the slab that holds its LAST row.  Needed only when the walk re-runs the scaling stage.
    const size_t sf = cfg->scale_factor > 1 ? (size_t)cfg->scale_factor : 1;
    // A slab shorter than the scale factor is refused by a rule of (nx, ny, world, sf) alone: every rank refuses
    // here, before any exchange and before any slab is touched, and the group keeps its last outputs
    if (slab_scale_refused(gs->nx, gs->ny, g->world, sf))
        return gfail(g, THZ_ERR_UNSUPPORTED, "scaling over slabs: a slab has fewer rows than the scale factor");
    if (!single && sf > 1 && gs->nx / sf > 0 && gs->ny / sf > 0) {
        std::vector<float *> out, in;
        if (int rc = each_member(g, "scaling over slabs: ", [&](size_t i) { return session_scale_tail(gs->sess[i], cfg); })) return rc;
        for (thz_session *s : gs->sess) {
            out.push_back(s->d_carry_out);
            in.push_back(s->d_carry_in);
        }
        const size_t count = (gs->ny / sf) * gs->nt;
        for (int q = 0; q + 1 < g->world; ++q)
            if (slab_scale(gs->nx, g->world, q, sf).tail)
                if (int rc = group_p2p(g, q, q + 1, out.data(), in.data(), count)) return rc;
    }
    // every slab's chain, enqueued side by side on the members' streams
    std::unique_ptr<bool[]> tail(new bool[gs->sess.size()]());  // per member: its chain's tail alone was walked
    if (int rc = each_member(g, "slab recompute: ", [&](size_t i) { return session_enqueue(gs->sess[i], cfg, start_stage, &tail[i]); })) return rc;
    const bool tail_only = tail[0];  // (the members agree: same regions, same history)
    thz_session *s0 = gs->sess[0];
    const size_t nt_out = s0->nt_out, nf = nt_out / 2 + 1;
    gs->nt_out = nt_out;
    // the outputs' grid: the raw one, or — one slab, scaled — the session's block grid
    gs->cur_rows = gs->rows;
    gs->cur_ny = gs->ny;
    if (s0->scale > 1) {
        gs->cur_ny = s0->ny_cur;
        for (int q = 0; q < g->world; ++q) gs->cur_rows[(size_t)q] = single ? s0->nx_cur : slab_scale(gs->nx, g->world, q, s0->scale).rows;
    }
    if (cfg->want_means && !tail_only)
        if (int rc = group_means(gs, cfg, single)) return rc;
    // C2, second part: the regions of interest's masked sums (every slab's rows of the whole grid's mask)
    if (!s0->rois.empty())
        if (int rc = group_roi_tail(gs, cfg, tail_only)) return rc;
    // C1: per-pixel results to rank 0
    if (int rc = gather_buf(gs, THZ_BUF_IMG, 1, &gs->d_img)) return rc;
    if (gather >= THZ_GATHER_TIME)
        if (int rc = gather_buf(gs, THZ_BUF_DATA, nt_out, &gs->d_data)) return rc;
    if (gather >= THZ_GATHER_ALL) {
        if (int rc = gather_buf(gs, THZ_BUF_FFT, 2 * nf, &gs->d_fft)) return rc;
        if (int rc = gather_buf(gs, THZ_BUF_AMPLITUDES, nf, &gs->d_amp)) return rc;
        if (int rc = gather_buf(gs, THZ_BUF_PHASES, nf, &gs->d_ph)) return rc;
    }
    gs->gathered = gather;
    return thz_group_sync(g);
}

int thz_group_session_grid(const thz_group_session *gs, size_t *nx, size_t *ny)
{
    if (!gs) return THZ_ERR_INVALID;
    if (nx) *nx = gs->cur_ny ? gs->cur_pix() / gs->cur_ny : 0;
    if (ny) *ny = gs->cur_ny;
    return THZ_OK;
}

void *thz_group_session_result(thz_group_session *gs, int which)
{
    if (!gs || gs->root_local < 0 || gs->gathered < 0) return nullptr;
    switch (which) {
    case THZ_BUF_IMG: return gs->d_img;
    case THZ_BUF_DATA: return gs->gathered >= THZ_GATHER_TIME ? gs->d_data : nullptr;
    case THZ_BUF_FFT: return gs->gathered >= THZ_GATHER_ALL ? gs->d_fft : nullptr;
    case THZ_BUF_AMPLITUDES: return gs->gathered >= THZ_GATHER_ALL ? gs->d_amp : nullptr;
    case THZ_BUF_PHASES: return gs->gathered >= THZ_GATHER_ALL ? gs->d_ph : nullptr;
    case THZ_BUF_AVG_FFT: case THZ_BUF_AVG_AMPLITUDES: case THZ_BUF_AVG_PHASES:
        return thz_session_buffer(gs->sess[(size_t)gs->root_local], which);
    default: return nullptr;
    }
}

int thz_group_session_download(thz_group_session *gs, int which, size_t pix0, size_t npix, void *dst)
{
    if (!gs || !dst) return THZ_ERR_INVALID;
    thz_group *g = gs->g;
    if (gs->root_local < 0) return gfail(g, THZ_ERR_NOT_READY, "this process does not drive rank 0");
    thz_session *rs = gs->sess[(size_t)gs->root_local];
    if (which == THZ_BUF_AVG_FFT || which == THZ_BUF_AVG_AMPLITUDES || which == THZ_BUF_AVG_PHASES)
        return thz_session_download(rs, which, 0, 1, dst);
    const float *base = static_cast<const float *>(thz_group_session_result(gs, which));
    if (!base) return gfail(g, THZ_ERR_NOT_READY, "buffer was not gathered by the last recompute");
    const size_t nf = gs->nt_out / 2 + 1;
    size_t per = 0;
    switch (which) {
    case THZ_BUF_IMG: per = 1; break;
    case THZ_BUF_DATA: per = gs->nt_out; break;
    case THZ_BUF_FFT: per = 2 * nf; break;
    case THZ_BUF_AMPLITUDES: case THZ_BUF_PHASES: per = nf; break;
    default: return THZ_ERR_INVALID;
    }
    if (pix0 > gs->cur_pix() || npix > gs->cur_pix() - pix0) return gfail(g, THZ_ERR_INVALID, "pixel range out of bounds");
    return thz_memcpy_d2h(g->m[(size_t)gs->root_local].ctx, dst, base + pix0 * per, npix * per * sizeof(float));
}

}  // extern "C"
