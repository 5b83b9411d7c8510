// group_comm.cpp — the group object behind thz_group* (group.hpp): member contexts, and the exchange steps of the
// path as collectives on the members' own streams.  Every collective has two forms, chosen at its top: device-local
// copies ordered by events (one process, every member on one device) and RCCL calls.
//
// librccl is opened with dlopen when a group with more than one device is created, so the library
// has no load-time dependency on it (a single-GPU user never maps its 570 MB).  The function
// prototypes come from <rccl/rccl.h>; only the symbols are looked up at run time.
#include "group.hpp"

#include <dlfcn.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>

using namespace thz;

namespace {

// RCCL's entry points the group uses, named once: the table's fields, and what rccl_load looks up ("nccl" + name)
#define THZ_RCCL_SYMS(X) \
    X(GetUniqueId) X(CommInitRank) X(CommInitAll) X(CommDestroy) X(GetErrorString) X(AllReduce) X(Broadcast) X(Send) X(Recv) X(GroupStart) X(GroupEnd)
#define THZ_RCCL_FIELD(name) decltype(&nccl##name) name = nullptr;
#define THZ_RCCL_LOOKUP(name) &&rccl_sym(r, r.name, "nccl" #name)

struct Rccl {
    void *h = nullptr;
    THZ_RCCL_SYMS(THZ_RCCL_FIELD)
    std::string err;
};

Rccl &rccl()
{
    static Rccl r;
    return r;
}

template <class F>
bool rccl_sym(Rccl &r, F &field, const char *sym)
{
    field = reinterpret_cast<F>(dlsym(r.h, sym));
    if (field) return true;
    r.err = std::string("librccl lacks ") + sym;
    dlclose(r.h);
    r.h = nullptr;
    return false;
}

bool rccl_load()
{
    Rccl &r = rccl();
    if (r.h) return true;
    // THZ_RCCL_LIB: developer knob — the library to open in RCCL's place (tests/mock_rccl: several ranks on ONE GPU)
    if (const char *override_path = getenv("THZ_RCCL_LIB")) {
        // never silent: a release process whose collectives go through something else than librccl says so
        fprintf(stderr, "[thzgpu] THZ_RCCL_LIB is set: opening %s in place of librccl (test infrastructure)\n", override_path);
        r.h = dlopen(override_path, RTLD_NOW | RTLD_LOCAL);
    } else
        for (const char *name : {"librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1"}) {
            r.h = dlopen(name, RTLD_NOW | RTLD_LOCAL);
            if (r.h) break;
        }
    if (!r.h) {
        r.err = std::string("cannot open librccl: ") + dlerror();
        return false;
    }
    return true THZ_RCCL_SYMS(THZ_RCCL_LOOKUP);
}

// One RCCL group call: `enqueue(r)` puts the local members' operations between GroupStart and GroupEnd and yields
// the first result that is not ncclSuccess, which ends the group and is reported as "<what>: <RCCL's words>".
template <class F>
int rccl_group(thz_group *g, const char *what, F &&enqueue)
{
    Rccl &r = rccl();
    auto report = [&](const char *call, ncclResult_t rc) { return gfail(g, THZ_ERR_HIP, std::string(call) + ": " + r.GetErrorString(rc)); };
    if (const ncclResult_t rc = r.GroupStart()) return report("r.GroupStart()", rc);
    if (const ncclResult_t rc = enqueue(r)) {
        (void)r.GroupEnd();
        return report(what, rc);
    }
    if (const ncclResult_t rc = r.GroupEnd()) return report("r.GroupEnd()", rc);
    return THZ_OK;
}

// member i, its device made current: the communicator's device is current while its call is enqueued
thz_group::Member &current(thz_group *g, size_t i)
{
    (void)hipSetDevice(g->m[i].ctx->device);
    return g->m[i];
}

// same-device groups: stream 0 waits for everything the other members have enqueued ...
int join_on_first(thz_group *g)
{
    for (size_t i = 1; i < g->m.size(); ++i) {
        GHIP_TRY(g, hipEventRecord(g->m[i].ev, g->m[i].ctx->stream));
        GHIP_TRY(g, hipStreamWaitEvent(g->m[0].ctx->stream, g->m[i].ev, 0));
    }
    return THZ_OK;
}
// ... and the others wait for what stream 0 did meanwhile
int fan_out_from_first(thz_group *g)
{
    GHIP_TRY(g, hipEventRecord(g->m[0].ev, g->m[0].ctx->stream));
    for (size_t i = 1; i < g->m.size(); ++i) GHIP_TRY(g, hipStreamWaitEvent(g->m[i].ctx->stream, g->m[0].ev, 0));
    return THZ_OK;
}

template <class T>
int all_reduce(thz_group *g, T *const *d_bufs, size_t count, ncclDataType_t type)
{
    if (!g || !d_bufs) return THZ_ERR_INVALID;
    if (count == 0 || one_slab(g)) return THZ_OK;
    for (size_t i = 0; i < g->m.size(); ++i)
        if (!d_bufs[i]) return gfail(g, THZ_ERR_INVALID, "all-reduce: null buffer");
    if (g->same_device) {
        GHIP_TRY(g, hipSetDevice(g->m[0].ctx->device));
        if (int rc = join_on_first(g)) return rc;
        hipStream_t st = g->m[0].ctx->stream;
        for (size_t i = 1; i < g->m.size(); ++i) {
            if constexpr (sizeof(T) == 4) launch_add_vec(st, (float *)d_bufs[0], (const float *)d_bufs[i], count);
            else launch_add_u64(st, (unsigned long long *)d_bufs[0], (const unsigned long long *)d_bufs[i], count);
        }
        GHIP_TRY(g, hipGetLastError());
        for (size_t i = 1; i < g->m.size(); ++i)
            GHIP_TRY(g, hipMemcpyAsync(d_bufs[i], d_bufs[0], count * sizeof(T), hipMemcpyDeviceToDevice, st));
        return fan_out_from_first(g);
    }
    return rccl_group(g, "ncclAllReduce", [&](Rccl &r) {
        ncclResult_t rc = ncclSuccess;
        for (size_t i = 0; i < g->m.size() && rc == ncclSuccess; ++i) {
            thz_group::Member &mb = current(g, i);
            rc = r.AllReduce(d_bufs[i], d_bufs[i], count, type, ncclSum, mb.comm, mb.ctx->stream);
        }
        return rc;
    });
}

int make_member(thz_group *g, int device, int rank)
{
    thz_group::Member mb;
    if (int rc = thz_create(device, &mb.ctx)) return gfail(g, rc, "thz_create(" + std::to_string(device) + ") failed");
    mb.rank = rank;
    if (hipEventCreateWithFlags(&mb.ev, hipEventDisableTiming) != hipSuccess) {
        thz_destroy(mb.ctx);
        return gfail(g, THZ_ERR_HIP, "hipEventCreate failed");
    }
    g->m.push_back(mb);
    return THZ_OK;
}

using GroupPtr = std::unique_ptr<thz_group, void (*)(thz_group *)>;

}  // namespace

int group_p2p(thz_group *g, int from, int to, const float *const *d_src, float *const *d_dst, size_t count)
{
    if (count == 0 || from == to) return THZ_OK;
    const int lf = local_of_rank(g, from), lt = local_of_rank(g, to);
    if (lf < 0 && lt < 0) return THZ_OK;
    if (g->same_device || (lf >= 0 && lt >= 0 && !g->m[(size_t)lf].comm)) {
        // one process, no fabric: a device-local copy on the receiver's stream behind the sender's work
        GHIP_TRY(g, hipSetDevice(g->m[(size_t)lt].ctx->device));
        GHIP_TRY(g, hipEventRecord(g->m[(size_t)lf].ev, g->m[(size_t)lf].ctx->stream));
        GHIP_TRY(g, hipStreamWaitEvent(g->m[(size_t)lt].ctx->stream, g->m[(size_t)lf].ev, 0));
        GHIP_TRY(g, hipMemcpyAsync(d_dst[lt], d_src[lf], count * sizeof(float), hipMemcpyDeviceToDevice, g->m[(size_t)lt].ctx->stream));
        // ... and the sender's stream behind the copy, as a send on its own stream would be: the sender may write its
        // buffer again right away (the carried means reuse one running-sum buffer for all three arrays)
        GHIP_TRY(g, hipEventRecord(g->m[(size_t)lt].ev, g->m[(size_t)lt].ctx->stream));
        GHIP_TRY(g, hipStreamWaitEvent(g->m[(size_t)lf].ctx->stream, g->m[(size_t)lt].ev, 0));
        return THZ_OK;
    }
    return rccl_group(g, "ncclSend / ncclRecv", [&](Rccl &r) {
        ncclResult_t rc = ncclSuccess;
        if (lf >= 0) {
            thz_group::Member &mb = current(g, (size_t)lf);
            rc = r.Send(d_src[lf], count, ncclFloat, to, mb.comm, mb.ctx->stream);
        }
        if (lt >= 0 && rc == ncclSuccess) {
            thz_group::Member &mb = current(g, (size_t)lt);
            rc = r.Recv(d_dst[lt], count, ncclFloat, from, mb.comm, mb.ctx->stream);
        }
        return rc;
    });
}

int group_all_gather(thz_group *g, const float *const *d_send, const size_t *counts, float *const *d_recv)
{
    const std::vector<size_t> off = offsets(counts, g->world);
    if (g->same_device || one_slab(g)) {
        GHIP_TRY(g, hipSetDevice(g->m[0].ctx->device));
        if (g->world > 1)
            if (int rc = join_on_first(g)) return rc;
        for (size_t i = 0; i < g->m.size(); ++i)
            for (size_t k = 0; k < g->m.size(); ++k) {
                const size_t q = (size_t)g->m[k].rank;
                if (counts[q])
                    GHIP_TRY(g, hipMemcpyAsync(d_recv[i] + off[q], d_send[k], counts[q] * sizeof(float), hipMemcpyDeviceToDevice,
                                               g->m[0].ctx->stream));
            }
        return g->world > 1 ? fan_out_from_first(g) : THZ_OK;
    }
    return rccl_group(g, "ncclBroadcast", [&](Rccl &r) {
        ncclResult_t rc = ncclSuccess;
        for (size_t i = 0; i < g->m.size() && rc == ncclSuccess; ++i) {
            thz_group::Member &mb = current(g, i);
            for (int q = 0; q < g->world && rc == ncclSuccess; ++q)
                if (counts[q])
                    rc = r.Broadcast(mb.rank == q ? d_send[i] : d_recv[i] + off[(size_t)q], d_recv[i] + off[(size_t)q], counts[q], ncclFloat, q,
                                     mb.comm, mb.ctx->stream);
        }
        return rc;
    });
}

int group_any_failed(thz_group *g, const std::vector<int> &rcs, float *const *flag, bool *bad)
{
    for (size_t i = 0; i < g->m.size(); ++i) {
        GHIP_TRY(g, hipSetDevice(g->m[i].ctx->device));
        const float v = rcs[i] < 0 ? 1.0f : 0.0f;
        GHIP_TRY(g, hipMemcpyAsync(flag[i], &v, sizeof v, hipMemcpyHostToDevice, g->m[i].ctx->stream));
        GHIP_TRY(g, hipStreamSynchronize(g->m[i].ctx->stream));
    }
    if (int rc = thz_group_all_reduce_sum(g, flag, 1)) return rc;
    float v = 0.0f;
    GHIP_TRY(g, hipSetDevice(g->m[0].ctx->device));
    GHIP_TRY(g, hipMemcpyAsync(&v, flag[0], sizeof v, hipMemcpyDeviceToHost, g->m[0].ctx->stream));
    GHIP_TRY(g, hipStreamSynchronize(g->m[0].ctx->stream));
    *bad = v != 0.0f;
    return THZ_OK;
}

int group_agree(thz_group *g, const std::vector<int> &rcs, uint64_t *const *d_flag, int *agreed)
{
    static const uint64_t one = 1;  // host source of the small uploads: alive whenever a stream gets to them
    for (size_t i = 0; i < g->m.size(); ++i) {
        GHIP_TRY(g, hipSetDevice(g->m[i].ctx->device));
        GHIP_TRY(g, hipMemsetAsync(d_flag[i], 0, 5 * sizeof(uint64_t), g->m[i].ctx->stream));
        if (rcs[i] < 0) {
            const int slot = rcs[i] >= -5 ? -rcs[i] - 1 : 2;  // (an unknown code counts as a HIP failure)
            GHIP_TRY(g, hipMemcpyAsync(d_flag[i] + slot, &one, sizeof(uint64_t), hipMemcpyHostToDevice, g->m[i].ctx->stream));
        }
    }
    if (int rc = thz_group_all_reduce_u64(g, d_flag, 5)) return rc;
    uint64_t tally[5];
    GHIP_TRY(g, hipSetDevice(g->m[0].ctx->device));
    GHIP_TRY(g, hipMemcpyAsync(tally, d_flag[0], sizeof tally, hipMemcpyDeviceToHost, g->m[0].ctx->stream));
    GHIP_TRY(g, hipStreamSynchronize(g->m[0].ctx->stream));
    *agreed = THZ_OK;
    for (int c = 0; c < 5 && !*agreed; ++c)
        if (tally[c]) *agreed = -(c + 1);
    return THZ_OK;
}

extern "C" {

int thz_host_slab(size_t nx, int world, int rank, size_t *x0, size_t *n)
{
    if (world < 1 || rank < 0 || rank >= world) return THZ_ERR_INVALID;
    const size_t base = nx / (size_t)world, rem = nx % (size_t)world, r = (size_t)rank;
    if (n) *n = base + (r < rem ? 1 : 0);
    if (x0) *x0 = r * base + (r < rem ? r : rem);
    return THZ_OK;
}

// g == NULL: why the last thz_group_create* / thz_group_unique_id could not load RCCL (there is no group to ask then)
const char *thz_group_last_error(const thz_group *g) { return g ? g->err.c_str() : (rccl().err.empty() ? "null group" : rccl().err.c_str()); }
int thz_group_world(const thz_group *g) { return g ? g->world : 0; }
int thz_group_local_count(const thz_group *g) { return g ? (int)g->m.size() : 0; }
int thz_group_rank(const thz_group *g, int i) { return (g && i >= 0 && i < (int)g->m.size()) ? g->m[i].rank : -1; }
thz_ctx *thz_group_ctx(thz_group *g, int i) { return (g && i >= 0 && i < (int)g->m.size()) ? g->m[i].ctx : nullptr; }

void thz_group_destroy(thz_group *g)  // (also what ends a group whose creation fails half-way: GroupPtr)
{
    if (!g) return;
    for (auto &mb : g->m) {
        if (mb.ctx) {
            (void)hipSetDevice(mb.ctx->device);
            (void)hipStreamSynchronize(mb.ctx->stream);
        }
        if (mb.comm) (void)rccl().CommDestroy(mb.comm);
        if (mb.ev) (void)hipEventDestroy(mb.ev);
        if (mb.ctx) thz_destroy(mb.ctx);
    }
    delete g;
}

int thz_group_create(const int *devices, int n, thz_group **out)
{
    if (!out || !devices || n < 1) return THZ_ERR_INVALID;
    *out = nullptr;
    bool all_same = true, distinct = true;
    for (int i = 0; i < n; ++i)
        for (int j = i + 1; j < n; ++j) {
            if (devices[i] == devices[j]) distinct = false;
            else all_same = false;
        }
    if (n > 1 && !all_same && !distinct) return THZ_ERR_INVALID;
    GroupPtr g(new thz_group(), thz_group_destroy);
    g->world = n;
    g->same_device = n > 1 && all_same;
    for (int i = 0; i < n; ++i)
        if (int rc = make_member(g.get(), devices[i], i)) return rc;
    if (n > 1 && distinct) {
        if (!rccl_load()) return THZ_ERR_HIP;
        std::vector<ncclComm_t> comms((size_t)n);
        if (rccl().CommInitAll(comms.data(), n, devices) != ncclSuccess) return THZ_ERR_HIP;
        for (int i = 0; i < n; ++i) g->m[(size_t)i].comm = comms[(size_t)i];
    }
    *out = g.release();
    return THZ_OK;
}

int thz_group_unique_id(void *id)
{
    if (!id) return THZ_ERR_INVALID;
    static_assert(sizeof(ncclUniqueId) == THZ_GROUP_ID_BYTES, "THZ_GROUP_ID_BYTES");
    if (!rccl_load()) return THZ_ERR_HIP;
    ncclUniqueId u;
    if (rccl().GetUniqueId(&u) != ncclSuccess) return THZ_ERR_HIP;
    std::memcpy(id, &u, sizeof u);
    return THZ_OK;
}

int thz_group_create_rank(int device, int rank, int world, const void *id, thz_group **out)
{
    if (!out || world < 1 || rank < 0 || rank >= world || (world > 1 && !id)) return THZ_ERR_INVALID;
    *out = nullptr;
    GroupPtr g(new thz_group(), thz_group_destroy);
    g->world = world;
    if (int rc = make_member(g.get(), device, rank)) return rc;
    // THZ_GROUP_FORCE_RCCL: a single-rank group still opens librccl, builds its communicator and sends its
    // collectives through it — how the RCCL entry points are exercised on a one-GPU box (tests/test_gpu_group.py)
    if (world > 1 || (id && getenv("THZ_GROUP_FORCE_RCCL"))) {
        if (!rccl_load()) return THZ_ERR_HIP;
        ncclUniqueId u;
        std::memcpy(&u, id, sizeof u);
        if (hipSetDevice(device) != hipSuccess || rccl().CommInitRank(&g->m[0].comm, world, u, rank) != ncclSuccess) {
            g->m[0].comm = nullptr;
            return THZ_ERR_HIP;
        }
    }
    *out = g.release();
    return THZ_OK;
}

int thz_group_all_reduce_sum(thz_group *g, float *const *d_bufs, size_t count) { return all_reduce<float>(g, d_bufs, count, ncclFloat); }
int thz_group_all_reduce_u64(thz_group *g, uint64_t *const *d_bufs, size_t count) { return all_reduce<uint64_t>(g, d_bufs, count, ncclUint64); }

int thz_group_gather(thz_group *g, const float *const *d_send, const size_t *counts, float *d_recv_root)
{
    if (!g || !d_send || !counts) return THZ_ERR_INVALID;
    const std::vector<size_t> off = offsets(counts, g->world);
    const int root = local_of_rank(g, 0);
    if (root >= 0 && !d_recv_root) return gfail(g, THZ_ERR_INVALID, "gather: rank 0 needs a receive buffer");
    if (g->same_device) {
        GHIP_TRY(g, hipSetDevice(g->m[0].ctx->device));
        if (int rc = join_on_first(g)) return rc;
        for (size_t i = 0; i < g->m.size(); ++i) {
            const size_t q = (size_t)g->m[i].rank;
            if (counts[q] && d_recv_root + off[q] != d_send[i])
                GHIP_TRY(g, hipMemcpyAsync(d_recv_root + off[q], d_send[i], counts[q] * sizeof(float), hipMemcpyDeviceToDevice,
                                           g->m[0].ctx->stream));
        }
        return fan_out_from_first(g);
    }
    if (root >= 0 && counts[0] && d_recv_root != d_send[root]) {  // rank 0's own rows: a device-local copy
        GHIP_TRY(g, hipSetDevice(g->m[(size_t)root].ctx->device));
        GHIP_TRY(g, hipMemcpyAsync(d_recv_root, d_send[root], counts[0] * sizeof(float), hipMemcpyDeviceToDevice,
                                   g->m[(size_t)root].ctx->stream));
    }
    if (one_slab(g)) return THZ_OK;
    return rccl_group(g, "ncclSend / ncclRecv", [&](Rccl &r) {
        ncclResult_t rc = ncclSuccess;
        for (size_t i = 0; i < g->m.size() && rc == ncclSuccess; ++i) {
            const size_t q = (size_t)g->m[i].rank;
            thz_group::Member &mb = current(g, i);
            if (q != 0 && counts[q]) rc = r.Send(d_send[i], counts[q], ncclFloat, 0, mb.comm, mb.ctx->stream);
        }
        if (root >= 0) {
            thz_group::Member &mb = current(g, (size_t)root);
            for (int q = 1; q < g->world && rc == ncclSuccess; ++q)
                if (counts[q]) rc = r.Recv(d_recv_root + off[(size_t)q], counts[q], ncclFloat, q, mb.comm, mb.ctx->stream);
        }
        return rc;
    });
}

int thz_group_sync(thz_group *g)
{
    if (!g) return THZ_ERR_INVALID;
    for (auto &mb : g->m) {
        GHIP_TRY(g, hipSetDevice(mb.ctx->device));
        GHIP_TRY(g, hipStreamSynchronize(mb.ctx->stream));
    }
    return THZ_OK;
}

}  // extern "C"
