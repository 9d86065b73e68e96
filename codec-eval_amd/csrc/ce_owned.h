// Owners of what the host runtime takes from HIP: a device allocation, a page-locked host block, an event, a created stream.
// Each is move-only, releases in its destructor and is empty after reset() or after it was moved from, so a struct of them is
// all-or-nothing by construction: build it in a local, move it into place when every alloc() has succeeded, and a failure
// half-way releases what there was on the way out.  alloc() / create() return a CE_* status and write the context's error as
// "<what>: <HIP's words>" (ctx may be null: no error string is kept); a failed call leaves the owner empty and no HIP error
// pending.  This header includes no HIP header: it comes after <hip/hip_runtime.h> (ce_internal.h), or after a test's
// stand-ins for the few calls used here (tests/cpp/test_owned.cpp).
#pragma once

#include <cstddef>
#include <string>

template <class Ctx>
inline int ce_owned_status(Ctx *ctx, hipError_t e, const char *what)
{
    if (e == hipSuccess) return CE_OK;
    (void)hipGetLastError();
    if (ctx) ctx->err = std::string(what) + ": " + hipGetErrorString(e);
    return CE_ERR_BACKEND;
}

// `n` elements of T from hipMalloc (Pinned: from hipHostMalloc); converts to the plain pointer wherever one is wanted
template <class T, bool Pinned>
class ce_block {
    T *p = nullptr;
    size_t n = 0;

public:
    ce_block() = default;
    ce_block(ce_block &&o) noexcept : p(o.p), n(o.n) { o.p = nullptr, o.n = 0; }
    ce_block &operator=(ce_block &&o) noexcept
    {
        if (this != &o) {
            reset();
            p = o.p, n = o.n;
            o.p = nullptr, o.n = 0;
        }
        return *this;
    }
    ~ce_block() { reset(); }
    void reset()
    {
        if (p) (void)(Pinned ? hipHostFree(p) : hipFree(p));
        p = nullptr, n = 0;
    }
    // a new block of `count` elements in place of the old one, which is released first
    template <class Ctx>
    int alloc(Ctx *ctx, size_t count, const char *what = Pinned ? "hipHostMalloc" : "hipMalloc")
    {
        reset();
        void *q = nullptr;
        const hipError_t e = Pinned ? hipHostMalloc(&q, count * sizeof(T), hipHostMallocDefault) : hipMalloc(&q, count * sizeof(T));
        if (e != hipSuccess) return ce_owned_status(ctx, e, what);
        p = static_cast<T *>(q), n = count;
        return CE_OK;
    }
    // grow-only: the block is kept when it holds `count` elements already
    template <class Ctx>
    int reserve(Ctx *ctx, size_t count, const char *what = Pinned ? "hipHostMalloc" : "hipMalloc")
    {
        return count <= n ? CE_OK : alloc(ctx, count, what);
    }
    operator T *() const { return p; }
    T *get() const { return p; }
    size_t size() const { return n; }  // elements
};
template <class T>
using ce_dev = ce_block<T, false>;
template <class T>
using ce_pinned = ce_block<T, true>;

// an event without timing (every event of a batch orders streams, none is read as a time)
class ce_event {
    hipEvent_t e = nullptr;

public:
    ce_event() = default;
    ce_event(ce_event &&o) noexcept : e(o.e) { o.e = nullptr; }
    ce_event &operator=(ce_event &&o) noexcept
    {
        if (this != &o) {
            reset();
            e = o.e;
            o.e = nullptr;
        }
        return *this;
    }
    ~ce_event() { reset(); }
    void reset()
    {
        if (e) (void)hipEventDestroy(e);
        e = nullptr;
    }
    template <class Ctx>
    int create(Ctx *ctx, const char *what = "hipEventCreate")
    {
        reset();
        const hipError_t r = hipEventCreateWithFlags(&e, hipEventDisableTiming);
        if (r != hipSuccess) e = nullptr;
        return ce_owned_status(ctx, r, what);
    }
    operator hipEvent_t() const { return e; }
};

// a non-blocking stream this owner created; reset() destroys it without waiting (HIP lets queued work finish)
class ce_stream {
    hipStream_t s = nullptr;

public:
    ce_stream() = default;
    ce_stream(ce_stream &&o) noexcept : s(o.s) { o.s = nullptr; }
    ce_stream &operator=(ce_stream &&o) noexcept
    {
        if (this != &o) {
            reset();
            s = o.s;
            o.s = nullptr;
        }
        return *this;
    }
    ~ce_stream() { reset(); }
    void reset()
    {
        if (s) (void)hipStreamDestroy(s);
        s = nullptr;
    }
    template <class Ctx>
    int create(Ctx *ctx, const char *what = "hipStreamCreate")
    {
        reset();
        const hipError_t r = hipStreamCreateWithFlags(&s, hipStreamNonBlocking);
        if (r != hipSuccess) s = nullptr;
        return ce_owned_status(ctx, r, what);
    }
    operator hipStream_t() const { return s; }
};
