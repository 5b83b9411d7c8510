// dev_buf.hpp — the owner of one persistent device block and of the element count it was asked for.  Every device
// buffer that outlives a call is a member of this type: sized by exact() or grow(), freed by nobody.  Stands alone: of
// HIP it needs the runtime API's allocation calls only, of the project nothing.
//
//   exact(ctx, n)   a block of exactly n elements: nothing if that is what is held, otherwise free, then allocate
//   grow(ctx, n)    a block of at least n elements: nothing if the one held is large enough, otherwise free, then allocate
//   drop(ctx)       free; no block, count 0
//
// The old block is freed BEFORE the new one is allocated (the two are never alive together), and a live block is
// freed only behind a synchronisation of ctx->stream — which therefore happens on a reallocation and never in a
// steady state.  A failed allocation leaves no block and count 0, puts the reason into ctx->err and returns
// kDevBufErrHip.  ctx is any object with a `stream` and a string `err` (the context); the owner stores neither, so it
// stays a plain movable struct member.  The destructor and a move-assignment over a held block free WITHOUT a
// synchronisation: whoever destroys or replaces an owner has drained the stream.
#pragma once
#include <hip/hip_runtime_api.h>

#include <cstddef>
#include <string>

constexpr int kDevBufErrHip = -3;  // THZ_ERR_HIP of the C ABI (ctx.hpp holds the two together)

template <class T, bool kPinnedHost = false>
class DevBuf {
    T *p_ = nullptr;
    size_t n_ = 0;

    void release()
    {
        if (p_) (void)(kPinnedHost ? hipHostFree(p_) : hipFree(p_));
        p_ = nullptr;
        n_ = 0;
    }
    template <class Ctx>
    int renew(Ctx *ctx, size_t n)
    {
        drop(ctx);
        const size_t bytes = (n ? n : 1) * sizeof(T);
        void *p = nullptr;
        const hipError_t e = kPinnedHost ? hipHostMalloc(&p, bytes, hipHostMallocDefault) : hipMalloc(&p, bytes);
        if (e != hipSuccess) {
            ctx->err = std::string(kPinnedHost ? "hipHostMalloc" : "hipMalloc") + " of " + std::to_string(bytes) + " bytes: " + hipGetErrorString(e);
            return kDevBufErrHip;
        }
        p_ = static_cast<T *>(p);
        n_ = n;
        return 0;
    }

public:
    DevBuf() = default;
    DevBuf(const DevBuf &) = delete;
    DevBuf &operator=(const DevBuf &) = delete;
    DevBuf(DevBuf &&o) noexcept : p_(o.p_), n_(o.n_)
    {
        o.p_ = nullptr;
        o.n_ = 0;
    }
    DevBuf &operator=(DevBuf &&o) noexcept
    {
        if (this != &o) {
            release();
            p_ = o.p_;
            n_ = o.n_;
            o.p_ = nullptr;
            o.n_ = 0;
        }
        return *this;
    }
    ~DevBuf() { release(); }

    operator T *() const { return p_; }
    template <class U>
    U *as() const { return reinterpret_cast<U *>(p_); }
    size_t count() const { return n_; }                       // elements asked for; 0 without a block
    bool holds(size_t n) const { return p_ && n_ == n; }      // a block of exactly n elements

    template <class Ctx>
    int exact(Ctx *ctx, size_t n) { return holds(n) ? 0 : renew(ctx, n); }
    template <class Ctx>
    int grow(Ctx *ctx, size_t n) { return n <= n_ ? 0 : renew(ctx, n); }
    template <class Ctx>
    void drop(Ctx *ctx)
    {
        if (p_) (void)hipStreamSynchronize(ctx->stream);
        release();
    }
};

template <class T>
using PinnedBuf = DevBuf<T, true>;

// A device block of ONE call: allocated when the call knows its size, freed behind a synchronisation of the stream
// however the call ends.
template <class T, class Ctx>
class ScopedDevBuf {
    Ctx *ctx_;
    DevBuf<T> b_;

public:
    explicit ScopedDevBuf(Ctx *ctx) : ctx_(ctx) {}
    ScopedDevBuf(const ScopedDevBuf &) = delete;
    ScopedDevBuf &operator=(const ScopedDevBuf &) = delete;
    ~ScopedDevBuf() { b_.drop(ctx_); }
    int alloc(size_t n) { return b_.exact(ctx_, n); }
    operator T *() const { return b_; }
};
