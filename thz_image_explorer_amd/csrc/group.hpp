// group.hpp — x-slab tiles of one cube over the GPUs of a node (include/thzgpu.h, "Multi-GPU" section): the group
// and its session behind thz_group* / thz_group_session*, and what the units of the layer share — group_comm.cpp
// (RCCL, the group object, the collectives), group_session.cpp (the slabs' chain), group_deconv.cpp (the band-parallel
// Deconvolution stage), group_voxels.cpp (the 3-D view).  Internal, like session.hpp.
#pragma once
#include "session.hpp"
#include "host_windows.hpp"

#include <rccl/rccl.h>

#include <functional>
#include <string>
#include <thread>
#include <vector>

struct thz_group {
    struct Member {
        thz_ctx *ctx = nullptr;
        int rank = 0;
        ncclComm_t comm = nullptr;
        hipEvent_t ev = nullptr;  // same-device groups: orders the members' streams around a collective
    };
    std::vector<Member> m;
    int world = 0;
    bool same_device = false;  // one process, every member on one device: no fabric, device-local copies
    std::string err;
};

struct thz_group_session {
    thz_group *g = nullptr;
    size_t nx = 0, ny = 0, nt = 0;
    std::vector<thz_session *> sess;   // one per local member
    std::vector<size_t> x0, rows;      // one per rank
    int root_local = -1;               // index of rank 0 among the local members, -1: another process has it
    // gathered copies on rank 0's device, allocated when first asked for (grow-only)
    DevBuf<float> d_img, d_data, d_fft, d_amp, d_ph;
    // gathered arrival-time maps of the last thz_group_session_estimate_tilt (group_tilt.cpp), on rank 0's device:
    // [index bits | offsets | values], peak_stride() entries each of which the first peak_pix are the grid's (grow-only)
    DevBuf<float> d_peak;
    size_t peak_pix = 0;
    size_t peak_stride() const { return d_peak.count() / 3; }
    std::vector<size_t> cur_rows;      // rows of the outputs' grid per rank (the block grid behind a scaling stage)
    size_t cur_ny = 0;
    size_t cur_pix() const
    {
        size_t r = 0;
        for (size_t v : cur_rows) r += v;
        return r * cur_ny;
    }
    size_t nt_out = 0;
    int gathered = -1;  // thz_gather level of the last recompute
};

inline int gfail(thz_group *g, int code, const std::string &msg)
{
    if (g) g->err = msg;
    return code;
}

#define GHIP_TRY(g, expr)                                                                            \
    do {                                                                                             \
        hipError_t e_ = (expr);                                                                      \
        if (e_ != hipSuccess) return gfail(g, THZ_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(e_)); \
    } while (0)

// one slab, no communicator: the group is one session and a collective has nothing to move
inline bool one_slab(const thz_group *g) { return g->world == 1 && !g->m[0].comm; }

// the local member that holds rank q, -1: another process has it
inline int local_of_rank(const thz_group *g, int q)
{
    for (size_t i = 0; i < g->m.size(); ++i)
        if (g->m[i].rank == q) return (int)i;
    return -1;
}

// where rank q's floats start when the ranks' counts lie one behind the other; [world]: all of them
inline std::vector<size_t> offsets(const size_t *counts, int world)
{
    std::vector<size_t> off((size_t)world + 1, 0);
    for (int q = 0; q < world; ++q) off[(size_t)q + 1] = off[(size_t)q] + counts[q];
    return off;
}

// The device buffers ONE call allocated on the members' devices.  However the call ends: per member, its device
// current, its stream synchronised once, its buffers freed.  Buffers that outlive the call (the gathered results, a
// session's d_deconv / d_opacity) do not belong here.
struct CallBufs {
    thz_group *g;
    std::vector<std::vector<void *>> held;  // per local member
    explicit CallBufs(thz_group *g_) : g(g_), held(g_->m.size()) {}
    CallBufs(const CallBufs &) = delete;
    ~CallBufs()
    {
        for (size_t i = 0; i < held.size(); ++i) {
            (void)hipSetDevice(g->m[i].ctx->device);
            (void)hipStreamSynchronize(g->m[i].ctx->stream);
            for (void *p : held[i]) (void)hipFree(p);
        }
    }
    // member i's device is current: `bytes` of its memory into *out, or THZ_ERR_HIP with msg as the group's error
    template <class T>
    int alloc(size_t i, T **out, size_t bytes, const char *msg)
    {
        *out = nullptr;
        if (hipMalloc((void **)out, bytes) != hipSuccess) return gfail(g, THZ_ERR_HIP, msg);
        held[i].push_back(*out);
        return THZ_OK;
    }
};

// fn(i) for every local member in turn, its device current; the first non-zero code ends the walk and becomes the
// group's, with the member's own message behind `prefix`
template <class F>
int each_member(thz_group *g, const char *prefix, F &&fn)
{
    for (size_t i = 0; i < g->m.size(); ++i) {
        (void)hipSetDevice(g->m[i].ctx->device);
        if (int rc = fn(i)) return gfail(g, rc, std::string(prefix) + thz_last_error(g->m[i].ctx));
    }
    return THZ_OK;
}

// fn(i) for every local member SIDE BY SIDE, its device current: one host thread per member, because the calls wait
// for their streams (the Deconvolution stage's phases).  rcs[i] is what member i returned; nothing is reported.
inline void members_in_parallel(thz_group *g, const std::function<int(size_t)> &fn, std::vector<int> &rcs)
{
    rcs.assign(g->m.size(), THZ_OK);
    auto one = [&](size_t i) {
        (void)hipSetDevice(g->m[i].ctx->device);
        rcs[i] = fn(i);
    };
    if (rcs.size() == 1) return one(0);
    std::vector<std::thread> th;
    for (size_t i = 0; i < rcs.size(); ++i) th.emplace_back(one, i);
    for (auto &t : th) t.join();
}

// ---- group_comm.cpp.  rank `from` -> rank `to`: src / dst are indexed by LOCAL member; only the members that hold the two ranks act
int group_p2p(thz_group *g, int from, int to, const float *const *d_src, float *const *d_dst, size_t count);
// every member ends with all ranks' rows: d_send[i] (counts[rank_i] floats) -> d_recv[i] + offset(rank), in rank order
int group_all_gather(thz_group *g, const float *const *d_send, const size_t *counts, float *const *d_recv);
// Failure agreement, two protocols over per-member device scratch of the caller (rcs[i]: member i's own code).
// group_any_failed — one float per member, summed over the group: did anybody fail?
int group_any_failed(thz_group *g, const std::vector<int> &rcs, float *const *flag, bool *bad);
// group_agree — every local member adds its code to the group's tally (5 x u64 per member, one slot per THZ_ERR_*
// code); *agreed is the first code any rank reported, in the order INVALID, UNSUPPORTED, HIP, NOT_READY, ABORTED.
int group_agree(thz_group *g, const std::vector<int> &rcs, uint64_t *const *d_flag, int *agreed);
// ---- group_session.cpp.  The regions of interest's masked sums of every slab -> all-reduce -> the means, on every member.  cfg == NULL:
// every slab's own last configuration (the Deconvolution stage).
int group_roi_tail(thz_group_session *gs, const thz_chain_cfg *cfg, bool data_only);
