// dev_buf_driver.cpp — every transition of the device-buffer owner (csrc/dev_buf.hpp) on the host, under
// AddressSanitizer + UBSan (tests/test_dev_buf_host.py).  The six HIP calls the header uses are defined here over
// malloc / free, with a count of live blocks, a count of synchronisations and a switch that fails the next allocation.
// A block counts as in use by the stream from its allocation on: freeing it without a synchronisation in between is
// an error, so is every leak, double free or use of a freed block (the sanitizer's part).
#include "dev_buf.hpp"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <type_traits>
#include <utility>
#include <vector>

static int g_live = 0, g_syncs = 0, g_allocs = 0, g_unsynced_frees = 0;
static bool g_fail_next = false, g_busy = false;

static hipError_t fake_alloc(void **p, size_t bytes)
{
    if (g_fail_next) {
        g_fail_next = false;
        *p = nullptr;
        return hipErrorOutOfMemory;
    }
    *p = std::malloc(bytes);
    std::memset(*p, 0x5a, bytes);  // the whole block is writable
    ++g_live;
    ++g_allocs;
    g_busy = true;
    return hipSuccess;
}
static hipError_t fake_free(void *p)
{
    if (!p) return hipSuccess;
    if (g_busy) ++g_unsynced_frees;
    --g_live;
    std::free(p);
    return hipSuccess;
}
extern "C" {
hipError_t hipMalloc(void **p, size_t bytes) { return fake_alloc(p, bytes); }
hipError_t hipHostMalloc(void **p, size_t bytes, unsigned int) { return fake_alloc(p, bytes); }
hipError_t hipFree(void *p) { return fake_free(p); }
hipError_t hipHostFree(void *p) { return fake_free(p); }
hipError_t hipStreamSynchronize(hipStream_t)
{
    ++g_syncs;
    g_busy = false;
    return hipSuccess;
}
const char *hipGetErrorString(hipError_t) { return "out of memory (driver)"; }
}

struct Ctx {
    hipStream_t stream = nullptr;
    std::string err;
};

#define CHECK(cond)                                                              \
    do {                                                                         \
        if (!(cond)) {                                                           \
            std::printf("FAILED line %d: %s (live %d, syncs %d)\n", __LINE__, #cond, g_live, g_syncs); \
            return 1;                                                            \
        }                                                                        \
    } while (0)
// after every step: so many blocks alive, and no live block was ever freed without a synchronisation before it
#define STEP(live) CHECK(g_live == (live) && g_unsynced_frees == 0)

struct Roi {  // like SessionRoi: lives in a std::vector
    std::vector<int> poly;
    DevBuf<unsigned> list;
};
struct Tables {  // like DcSpectra: reset by assigning a fresh struct
    DevBuf<float> a, b;
    size_t M = 0;
};
static_assert(std::is_nothrow_move_constructible<DevBuf<float>>::value && std::is_nothrow_move_assignable<DevBuf<float>>::value, "");
static_assert(!std::is_copy_constructible<DevBuf<float>>::value && std::is_nothrow_move_constructible<Roi>::value, "");

static int scoped_early_return(Ctx *ctx, bool early)
{
    ScopedDevBuf<double, Ctx> t(ctx);
    if (t.alloc(9)) return -1;
    t[8] = 1.0;
    if (early) return 1;
    return 0;
}

int main()
{
    Ctx ctx;
    {
        DevBuf<float> b;
        CHECK(!b && b.count() == 0 && !b.holds(0));
        // ---- exact: first, same, smaller, larger
        CHECK(b.exact(&ctx, 10) == 0 && b && b.count() == 10);
        STEP(1);
        float *p = b;
        int syncs = g_syncs, allocs = g_allocs;
        b[9] = 1.0f;
        CHECK(b.exact(&ctx, 10) == 0 && b == p && g_syncs == syncs && g_allocs == allocs);  // steady state: nothing happens
        STEP(1);
        CHECK(b.exact(&ctx, 4) == 0 && b.count() == 4 && g_syncs == syncs + 1 && g_allocs == allocs + 1);
        STEP(1);
        CHECK(b.exact(&ctx, 100) == 0 && b.count() == 100);
        b[99] = 2.0f;
        STEP(1);
        // ---- grow: smaller keeps the block, larger replaces it
        p = b;
        syncs = g_syncs;
        CHECK(b.grow(&ctx, 7) == 0 && b == p && b.count() == 100 && g_syncs == syncs);
        CHECK(b.grow(&ctx, 100) == 0 && b == p && g_syncs == syncs);
        STEP(1);
        CHECK(b.grow(&ctx, 101) == 0 && b.count() == 101 && g_syncs == syncs + 1);
        b[100] = 3.0f;
        STEP(1);
        // ---- zero counts: exact allocates one element, grow of an empty owner allocates nothing
        CHECK(b.exact(&ctx, 0) == 0 && b && b.count() == 0 && b.holds(0));
        b[0] = 4.0f;
        STEP(1);
        p = b;
        CHECK(b.exact(&ctx, 0) == 0 && b == p);
        DevBuf<float> e;
        CHECK(e.grow(&ctx, 0) == 0 && !e);
        STEP(1);
        // ---- a failed allocation: on an empty owner, on a full one; then the next call succeeds
        g_fail_next = true;
        CHECK(e.exact(&ctx, 5) == kDevBufErrHip && !e && e.count() == 0 && !ctx.err.empty());
        STEP(1);
        ctx.err.clear();
        g_fail_next = true;
        CHECK(b.grow(&ctx, 50) == kDevBufErrHip && !b && b.count() == 0 && !ctx.err.empty());
        STEP(0);
        CHECK(b.grow(&ctx, 50) == 0 && b.count() == 50);
        b[49] = 5.0f;
        CHECK(e.exact(&ctx, 5) == 0 && e.count() == 5);
        STEP(2);
        // ---- drop, twice
        syncs = g_syncs;
        b.drop(&ctx);
        CHECK(!b && b.count() == 0 && g_syncs == syncs + 1);
        STEP(1);
        b.drop(&ctx);
        CHECK(!b && g_syncs == syncs + 1);
        STEP(1);
        // ---- move-construct; move-assign over a full owner (the caller has drained the stream, as for a destructor)
        p = e;
        DevBuf<float> m(std::move(e));
        CHECK(m == p && m.count() == 5 && !e && e.count() == 0);
        STEP(1);
        CHECK(b.exact(&ctx, 3) == 0);
        STEP(2);
        (void)hipStreamSynchronize(ctx.stream);
        p = m;
        b = std::move(m);
        CHECK(b == p && b.count() == 5 && !m);
        STEP(1);
        DevBuf<float> &self = b;
        b = std::move(self);  // self-assignment keeps the block
        CHECK(b == p && b.count() == 5);
        STEP(1);
        (void)hipStreamSynchronize(ctx.stream);
    }
    STEP(0);
    {
        // ---- the pinned form follows the same rules
        PinnedBuf<float> h;
        CHECK(h.exact(&ctx, 16) == 0 && h.count() == 16);
        h[15] = 1.0f;
        float *p = h;
        CHECK(h.exact(&ctx, 16) == 0 && h == p);
        CHECK(h.exact(&ctx, 32) == 0 && h.count() == 32);
        STEP(1);
        g_fail_next = true;
        CHECK(h.exact(&ctx, 8) == kDevBufErrHip && !h && ctx.err.find("hipHostMalloc") == 0);
        STEP(0);
    }
    {
        // ---- a vector of structs that hold an owner, pushed past its capacity and cleared
        std::vector<Roi> rois;
        std::vector<unsigned *> seen;
        for (int i = 0; i < 9; ++i) {
            Roi r;
            r.poly.assign(4, i);
            CHECK(r.list.grow(&ctx, (size_t)i + 1) == 0);
            seen.push_back(r.list);
            rois.push_back(std::move(r));
            STEP(i + 1);
        }
        for (int i = 0; i < 9; ++i) CHECK(rois[(size_t)i].list == seen[(size_t)i] && rois[(size_t)i].list.count() == (size_t)i + 1);
        (void)hipStreamSynchronize(ctx.stream);
        rois.clear();
        STEP(0);
    }
    {
        // ---- a fresh struct assigned over one that holds two owners
        Tables t;
        CHECK(t.a.exact(&ctx, 8) == 0 && t.b.exact(&ctx, 2) == 0);
        t.M = 8;
        STEP(2);
        t.a.drop(&ctx);
        t.b.drop(&ctx);
        t = Tables{};
        CHECK(!t.a && !t.b && t.M == 0);
        STEP(0);
        CHECK(t.a.exact(&ctx, 8) == 0 && t.b.exact(&ctx, 2) == 0);
        (void)hipStreamSynchronize(ctx.stream);
        t = Tables{};
        STEP(0);
    }
    {
        // ---- build beside the standing block, replace it on success only (thz_set_time_axis)
        DevBuf<float> standing;
        CHECK(standing.exact(&ctx, 6) == 0);
        float *p = standing;
        {
            DevBuf<float> next;
            g_fail_next = true;
            CHECK(next.exact(&ctx, 12) == kDevBufErrHip);
        }
        CHECK(standing == p && standing.count() == 6);
        STEP(1);
        {
            DevBuf<float> next;
            (void)hipStreamSynchronize(ctx.stream);
            CHECK(next.exact(&ctx, 12) == 0);
            STEP(2);
            (void)hipStreamSynchronize(ctx.stream);
            standing = std::move(next);
        }
        CHECK(standing.count() == 12);
        STEP(1);
        (void)hipStreamSynchronize(ctx.stream);
    }
    STEP(0);
    // ---- the scope-bound form: freed behind its own synchronisation, by an early return as by the last one
    int syncs = g_syncs;
    CHECK(scoped_early_return(&ctx, true) == 1 && g_syncs == syncs + 1);
    STEP(0);
    CHECK(scoped_early_return(&ctx, false) == 0 && g_syncs == syncs + 2);
    STEP(0);
    g_fail_next = true;
    CHECK(scoped_early_return(&ctx, false) == -1 && g_syncs == syncs + 2);
    STEP(0);
    std::printf("dev_buf done: %d allocations, %d synchronisations\n", g_allocs, g_syncs);
    return 0;
}
