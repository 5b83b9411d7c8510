// group_voxels.cpp — thz_group_session_voxels (group.hpp): update_intensity_image's 3-D part over the whole grid
// (include/thzgpu.h).  Every member works on its own slab; what crosses the fabric is the select's histograms, one
// (world + 1)-vector of counts and the records to rank 0.
#include "group.hpp"

#include <algorithm>

using namespace thz;

// Where each rank's records go in the whole list and how many of them fit.  cnt[q]: rank q's records at the
// threshold; base[q]: where they start (base[W] = total); take[q]: rank q's records that fit into `capacity`;
// n_rec: the records the list gets = min(total, capacity).
struct VoxelRecordPlan {
    std::vector<uint64_t> base, take;
    uint64_t total, n_rec;
};
VoxelRecordPlan voxel_record_plan(const uint64_t *cnt, uint64_t capacity, size_t W)
{
    VoxelRecordPlan p{std::vector<uint64_t>(W + 1, 0), std::vector<uint64_t>(W, 0), 0, 0};
    for (size_t q = 0; q < W; ++q) {
        p.base[q + 1] = p.base[q] + cnt[q];
        p.take[q] = std::min<uint64_t>(cnt[q], capacity > p.base[q] ? capacity - p.base[q] : 0);
    }
    p.total = p.base[W];
    p.n_rec = std::min<uint64_t>(p.total, capacity);
    return p;
}

extern "C" int thz_group_session_voxels(thz_group_session *gs, const thz_voxel_cfg *cfg, uint64_t max_instances, int scaling,
                                        size_t orig_w, size_t orig_h, size_t orig_d, thz_voxel_instance *host_out,
                                        uint64_t capacity, uint64_t *count, float *threshold, float *cube_dims)
{
    // arguments every rank checks alike, before any collective
    if (!gs || !cfg || !count) return THZ_ERR_INVALID;
    thz_group *g = gs->g;
    const size_t nl = gs->sess.size(), W = (size_t)g->world;
    if (max_instances < 1) return gfail(g, THZ_ERR_INVALID, "thz_group_session_voxels: max_instances must be >= 1");
    for (thz_session *s : gs->sess)
        if (!s->have_outputs) return gfail(g, THZ_ERR_NOT_READY, "thz_group_session_voxels: no recompute has run");
    size_t gx = 0, gy = 0;
    (void)thz_group_session_grid(gs, &gx, &gy);
    const size_t nt = gs->nt_out, n_total = gx * gy * nt;
    const VoxelLayout L = voxel_layout(gs->sess[0]->time_out.back() - gs->sess[0]->time_out.front(), gx, gy, nt, orig_w, orig_h, orig_d);
    // per member, u64: select histogram [kSelBins] | counts per rank + rank 0's capacity [W + 1] | failure tally [5]
    const size_t off_cnt = kSelBins, off_flag = off_cnt + W + 1, scratch = off_flag + 5;
    std::vector<uint64_t *> d_scr(nl, nullptr), d_hist(nl), d_cnt(nl), d_flag(nl);
    std::vector<thz_voxel_instance *> d_rec(nl, nullptr);  // a member's own records (NULL: it writes into d_root)
    thz_voxel_instance *d_root = nullptr;                   // the gathered list, on rank 0's device
    const uint64_t h_capacity = capacity;                   // host source of a small upload, alive until the buffers are freed
    CallBufs bufs(g);
    // The scratch first: it is the one allocation no agreement can cover (a process without it cannot take part in
    // a collective); 16 KiB and a few words per member.
    for (size_t i = 0; i < nl; ++i) {
        GHIP_TRY(g, hipSetDevice(g->m[i].ctx->device));
        if (int rc = bufs.alloc(i, &d_scr[i], scratch * sizeof(uint64_t), "thz_group_session_voxels: scratch allocation failed")) return rc;
        d_hist[i] = d_scr[i];
        d_cnt[i] = d_scr[i] + off_cnt;
        d_flag[i] = d_scr[i] + off_flag;
    }
    // every rank returns the code the group agrees on (group_agree), with its own message if it has one
    auto agree_or_return = [&](const std::vector<int> &rcs) -> int {
        int agreed = THZ_OK;
        if (int rc = group_agree(g, rcs, d_flag.data(), &agreed)) return rc;
        if (agreed) return gfail(g, agreed, g->err.empty() ? "thz_group_session_voxels: failed on another rank" : g->err);
        return THZ_OK;
    };
    // ---- opacity of every slab, resident as the member's THZ_BUF_OPACITY; then the first agreement
    std::vector<int> rcs(nl, THZ_OK);
    for (size_t i = 0; i < nl; ++i) {
        thz_session *s = gs->sess[i];
        thz_ctx *ctx = g->m[i].ctx;
        if (gs->root_local == (int)i && capacity && !host_out) {
            rcs[i] = gfail(g, THZ_ERR_INVALID, "thz_group_session_voxels: capacity without a buffer");
            continue;
        }
        const size_t npix = s->nx_cur * s->ny_cur;
        GHIP_TRY(g, hipSetDevice(ctx->device));
        rcs[i] = session_size_opacity(s);
        if (!rcs[i]) rcs[i] = thz_voxel_opacity(ctx, npix, nt, static_cast<const float *>(thz_session_buffer(s, THZ_BUF_DATA)), cfg, s->d_opacity);
        if (rcs[i]) gfail(g, rcs[i], std::string("thz_group_session_voxels: ") + thz_last_error(ctx));
    }
    if (int rc = agree_or_return(rcs)) return rc;
    // ---- threshold: the max_instances-th largest opacity of the whole grid.  Every level's histograms are
    // all-reduced, and every rank walks the same sums with thz_kth_largest's walk: the ranks agree without a broadcast.
    float thr = 0.0f;
    if (n_total > max_instances) {
        bool too_few = false;
        const int rc = select_walk(
            max_instances,
            [&](int level, uint32_t prefix, uint64_t *hist) -> int {
                for (size_t i = 0; i < nl; ++i) {
                    thz_ctx *ctx = g->m[i].ctx;
                    thz_session *s = gs->sess[i];
                    GHIP_TRY(g, hipSetDevice(ctx->device));
                    GHIP_TRY(g, hipMemsetAsync(d_hist[i], 0, kSelBins * sizeof(uint64_t), ctx->stream));
                    if (int rc2 = thz_select_histogram(ctx, s->d_opacity, s->d_opacity.count(), level, prefix, d_hist[i]))
                        return gfail(g, rc2, std::string("thz_group_session_voxels: ") + thz_last_error(ctx));
                }
                if (int rc2 = thz_group_all_reduce_u64(g, d_hist.data(), kSelBins)) return rc2;
                GHIP_TRY(g, hipSetDevice(g->m[0].ctx->device));
                GHIP_TRY(g, hipMemcpyAsync(hist, d_hist[0], kSelBins * sizeof(uint64_t), hipMemcpyDeviceToHost, g->m[0].ctx->stream));
                GHIP_TRY(g, hipStreamSynchronize(g->m[0].ctx->stream));
                return THZ_OK;
            },
            &thr, &too_few);
        if (too_few) gfail(g, THZ_ERR_INVALID, "thz_group_session_voxels: the histograms hold fewer values than the grid");
        if (rc) return rc;
    }
    // ---- counts: member r's total into slot r, rank 0's capacity into slot W.  One all-reduce tells every rank where
    // each slab's records start in the whole list and how many of them fit.
    for (size_t i = 0; i < nl; ++i) {
        thz_ctx *ctx = g->m[i].ctx;
        thz_session *s = gs->sess[i];
        const size_t q = (size_t)g->m[i].rank, npix = s->nx_cur * s->ny_cur;
        GHIP_TRY(g, hipSetDevice(ctx->device));
        GHIP_TRY(g, hipMemsetAsync(d_cnt[i], 0, (W + 1) * sizeof(uint64_t), ctx->stream));
        if (npix) {
            uint64_t *d_total = nullptr;
            if (int rc = voxel_count_scan(ctx, s->d_opacity, npix, nt, thr, &d_total))
                return gfail(g, rc, std::string("thz_group_session_voxels: ") + thz_last_error(ctx));
            GHIP_TRY(g, hipMemcpyAsync(d_cnt[i] + q, d_total, sizeof(uint64_t), hipMemcpyDeviceToDevice, ctx->stream));
        }
        if (q == 0) GHIP_TRY(g, hipMemcpyAsync(d_cnt[i] + W, &h_capacity, sizeof(uint64_t), hipMemcpyHostToDevice, ctx->stream));
    }
    if (int rc = thz_group_all_reduce_u64(g, d_cnt.data(), W + 1)) return rc;
    std::vector<uint64_t> cnt(W + 1);
    GHIP_TRY(g, hipSetDevice(g->m[0].ctx->device));
    GHIP_TRY(g, hipMemcpyAsync(cnt.data(), d_cnt[0], (W + 1) * sizeof(uint64_t), hipMemcpyDeviceToHost, g->m[0].ctx->stream));
    GHIP_TRY(g, hipStreamSynchronize(g->m[0].ctx->stream));
    const VoxelRecordPlan plan = voxel_record_plan(cnt.data(), cnt[W], W);
    // ---- records: every member emits those of its records that fit.  A member on rank 0's device (rank 0 itself, or
    // any member of a same-device group) writes straight into its place in the gathered list, which the gather then
    // leaves alone; the others emit into a buffer of their own, sent to rank 0 in rank order.
    if (plan.n_rec) {
        const char *msg = "thz_group_session_voxels: allocation of the records failed";
        rcs.assign(nl, THZ_OK);
        if (gs->root_local >= 0) {
            GHIP_TRY(g, hipSetDevice(g->m[(size_t)gs->root_local].ctx->device));
            rcs[(size_t)gs->root_local] = bufs.alloc((size_t)gs->root_local, &d_root, plan.n_rec * sizeof(thz_voxel_instance), msg);
        }
        for (size_t i = 0; i < nl; ++i) {
            const size_t q = (size_t)g->m[i].rank;
            if (!plan.take[q] || q == 0 || g->same_device) continue;
            GHIP_TRY(g, hipSetDevice(g->m[i].ctx->device));
            rcs[i] = bufs.alloc(i, &d_rec[i], plan.take[q] * sizeof(thz_voxel_instance), msg);
        }
        if (int rc = agree_or_return(rcs)) return rc;
        std::vector<const float *> send(nl, nullptr);
        std::vector<size_t> counts(W);
        for (size_t q = 0; q < W; ++q) counts[q] = (size_t)plan.take[q] * (sizeof(thz_voxel_instance) / sizeof(float));
        if (int rc = each_member(g, "thz_group_session_voxels: ", [&](size_t i) {
                thz_session *s = gs->sess[i];
                const size_t q = (size_t)g->m[i].rank;
                if (!plan.take[q]) return (int)THZ_OK;
                thz_voxel_instance *dst = d_rec[i] ? d_rec[i] : d_root + plan.base[q];
                send[i] = reinterpret_cast<const float *>(dst);
                const VoxelGeom geom{L.spacing_w, L.spacing_h, L.spacing_d, L.half_w, L.half_h, L.half_d, (float)scaling, thr, s->grid_x0};
                return voxel_emit(g->m[i].ctx, s->d_opacity, s->nx_cur * s->ny_cur, s->ny_cur, nt, geom, dst, plan.take[q]);
            }))
            return rc;
        if (int rc = thz_group_gather(g, send.data(), counts.data(), reinterpret_cast<float *>(d_root))) return rc;
        if (gs->root_local >= 0) {
            thz_ctx *ctx = g->m[(size_t)gs->root_local].ctx;
            if (int rc = thz_memcpy_d2h(ctx, host_out, d_root, plan.n_rec * sizeof(thz_voxel_instance)))
                return gfail(g, rc, std::string("thz_group_session_voxels: ") + thz_last_error(ctx));
        }
    }
    *count = plan.total;
    if (threshold) *threshold = thr;
    if (cube_dims) {
        cube_dims[0] = L.cube_width;
        cube_dims[1] = L.cube_height;
        cube_dims[2] = L.cube_depth;
    }
    return THZ_OK;
}
