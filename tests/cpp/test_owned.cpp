// The owners of codec-eval_amd/csrc/ce_owned.h on the host, stand-alone under AddressSanitizer and
// UndefinedBehaviorSanitizer (tests/test_owned_cpu.py): counting stand-ins take the place of the few HIP calls the header
// uses, and can be told to fail their N-th allocation or creation.  Checked: a working set built in a local and moved into
// place is whole or empty whichever allocation fails, and a retry starts clean; moves transfer ownership (one release per
// allocation); reserve() is grow-only and never holds two blocks or leaks one; a lazy extra that fails half-way stays
// disengaged; the error string is "<what>: <HIP's words>".
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <set>
#include <string>
#include <utility>

#include "ce_metrics.h"

// ---- stand-ins for HIP -----------------------------------------------------------------------------------------------
enum hipError_t { hipSuccess = 0, hipErrorOutOfMemory = 2 };
typedef struct ev_tag *hipEvent_t;
typedef struct st_tag *hipStream_t;
enum { hipHostMallocDefault = 0, hipEventDisableTiming = 2, hipStreamNonBlocking = 1 };

static std::set<void *> g_dev, g_host, g_events, g_streams;  // what is live, by kind
static long g_calls = 0, g_fail_at = 0;                      // acquisitions so far; the one that fails (0: none)
static long g_acquired = 0, g_released = 0, g_last_error_reads = 0;

#define CHECK(c)                                                              \
    do {                                                                      \
        if (!(c)) {                                                           \
            std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c);        \
            std::exit(1);                                                     \
        }                                                                     \
    } while (0)

static bool failing() { return ++g_calls == g_fail_at; }
static size_t live() { return g_dev.size() + g_host.size() + g_events.size() + g_streams.size(); }

static hipError_t acquire(std::set<void *> &kind, void **out, size_t bytes)
{
    if (failing()) return hipErrorOutOfMemory;  // like HIP, leaves *out alone
    *out = std::malloc(bytes ? bytes : 1);
    kind.insert(*out);
    g_acquired++;
    return hipSuccess;
}
static hipError_t release(std::set<void *> &kind, void *p)
{
    CHECK(kind.erase(p) == 1);  // released once, by the call that matches its allocation
    std::free(p);
    g_released++;
    return hipSuccess;
}
static hipError_t hipMalloc(void **p, size_t bytes) { return acquire(g_dev, p, bytes); }
static hipError_t hipFree(void *p) { return release(g_dev, p); }
static hipError_t hipHostMalloc(void **p, size_t bytes, unsigned) { return acquire(g_host, p, bytes); }
static hipError_t hipHostFree(void *p) { return release(g_host, p); }
static hipError_t hipEventCreateWithFlags(hipEvent_t *e, unsigned flags)
{
    CHECK(flags == hipEventDisableTiming);
    return acquire(g_events, reinterpret_cast<void **>(e), 1);
}
static hipError_t hipEventDestroy(hipEvent_t e) { return release(g_events, e); }
static hipError_t hipStreamCreateWithFlags(hipStream_t *s, unsigned flags)
{
    CHECK(flags == hipStreamNonBlocking);
    return acquire(g_streams, reinterpret_cast<void **>(s), 1);
}
static hipError_t hipStreamDestroy(hipStream_t s) { return release(g_streams, s); }
static hipError_t hipGetLastError() { return g_last_error_reads++, hipSuccess; }
static const char *hipGetErrorString(hipError_t e) { return e == hipSuccess ? "no error" : "out of memory"; }

struct ce_ctx {
    std::string err;
};

#include "ce_owned.h"

// ---- a working set shaped like ce_ssim2_set / ce_ba_set (ce_internal.h) --------------------------------------------------
constexpr int kLevels = 3;
struct half_extra {  // like ce_ba_half: a borrowed stream, two events, three planes
    hipStream_t stream = nullptr;
    ce_event ev_fork, ev_join;
    ce_dev<float> s[3];
};
struct working_set {
    int levels = 0;
    ce_dev<float> planes[kLevels], rows[kLevels];
    ce_event ev[2];
    ce_dev<double> partials;
    ce_pinned<double> host;
    ce_stream own_stream;
    ce_dev<float> cells;  // grow-only
    half_extra half;      // lazily
    bool engaged() const { return partials != nullptr; }
};
constexpr long kSetAcquisitions = 2 * kLevels + 2 + 1 + 1 + 1;
constexpr long kHalfAcquisitions = 2 + 3;

struct batch {
    ce_ctx *ctx;
    working_set set;
};

static int prepare(batch *b)
{
    if (b->set.engaged()) return CE_OK;
    working_set S;
    S.levels = kLevels;
    int rc = CE_OK;
    for (int l = 0; l < kLevels && rc == CE_OK; l++) {
        rc = S.planes[l].alloc(b->ctx, 100u << l);
        if (rc == CE_OK) rc = S.rows[l].alloc(b->ctx, 10u << l, "hipMalloc rows");
    }
    for (auto &e : S.ev)
        if (rc == CE_OK) rc = e.create(b->ctx);
    if (rc == CE_OK) rc = S.own_stream.create(b->ctx);
    if (rc == CE_OK) rc = S.host.alloc(b->ctx, 7, "hipHostMalloc scores");
    if (rc == CE_OK) rc = S.partials.alloc(b->ctx, 64);
    if (rc != CE_OK) return rc;
    b->set = std::move(S);
    return CE_OK;
}

static hipStream_t const kBorrowed = reinterpret_cast<hipStream_t>(0x40);  // the context's stream: never destroyed by a set

static int prepare_half(batch *b)
{
    if (b->set.half.stream) return CE_OK;
    half_extra h;
    h.stream = kBorrowed;
    if (int rc = h.ev_fork.create(b->ctx)) return rc;
    if (int rc = h.ev_join.create(b->ctx)) return rc;
    for (auto &p : h.s)
        if (int rc = p.alloc(b->ctx, 50)) return rc;
    b->set.half = std::move(h);
    return CE_OK;
}

static void arm(long n) { g_calls = 0, g_fail_at = n; }

static void test_all_or_nothing()
{
    for (long n = 1; n <= kSetAcquisitions; n++) {
        ce_ctx ctx;
        batch b{&ctx, {}};
        arm(n);
        CHECK(prepare(&b) == CE_ERR_BACKEND);
        CHECK(live() == 0);
        CHECK(!b.set.engaged() && b.set.levels == 0 && !b.set.planes[0] && !b.set.host);
        CHECK(!ctx.err.empty());
        arm(0);
        CHECK(prepare(&b) == CE_OK);
        CHECK(b.set.engaged() && b.set.levels == kLevels);
        CHECK((long)live() == kSetAcquisitions);
        for (int l = 0; l < kLevels; l++) CHECK(b.set.planes[l] && b.set.rows[l] && b.set.planes[l].size() == (100u << l));
        CHECK(prepare(&b) == CE_OK && (long)live() == kSetAcquisitions);  // engaged: nothing is allocated again
    }
    CHECK(live() == 0 && g_acquired == g_released);
    arm(kSetAcquisitions + 1);  // past the last allocation: nothing fails
    {
        ce_ctx ctx;
        batch b{&ctx, {}};
        CHECK(prepare(&b) == CE_OK && g_calls == kSetAcquisitions);
    }
    CHECK(live() == 0);
}

static void test_lazy_extra()
{
    for (long n = 1; n <= kHalfAcquisitions; n++) {
        ce_ctx ctx;
        batch b{&ctx, {}};
        arm(0);
        CHECK(prepare(&b) == CE_OK);
        arm(n);
        CHECK(prepare_half(&b) == CE_ERR_BACKEND);
        CHECK(!b.set.half.stream && !b.set.half.ev_fork && !b.set.half.ev_join);  // the next launch does not take the fork
        for (auto &p : b.set.half.s) CHECK(!p);
        CHECK((long)live() == kSetAcquisitions);  // the set itself is untouched
        arm(0);
        CHECK(prepare_half(&b) == CE_OK);  // and the next attempt allocates again
        CHECK(b.set.half.stream == kBorrowed && b.set.half.ev_fork && b.set.half.ev_join);
        for (auto &p : b.set.half.s) CHECK(p && p.size() == 50);
        CHECK((long)live() == kSetAcquisitions + kHalfAcquisitions);
    }
    CHECK(live() == 0 && g_acquired == g_released);
}

static void test_moves()
{
    arm(0);
    ce_ctx ctx;
    const long before = g_released;
    {
        ce_dev<float> a;
        CHECK(a.alloc(&ctx, 8) == CE_OK);
        float *const p = a;
        ce_dev<float> b(std::move(a));  // move construction
        CHECK(!a && a.size() == 0 && b.get() == p && b.size() == 8);
        ce_dev<float> c;
        CHECK(c.alloc(&ctx, 4) == CE_OK);
        c = std::move(b);  // move assignment releases what c held, once
        CHECK(g_released == before + 1 && !b && c.get() == p && c.size() == 8);
        ce_dev<float> &self = c;
        c = std::move(self);  // onto itself: kept
        CHECK(c.get() == p && live() == 1);
        ce_pinned<uint8_t> h, h2;
        CHECK(h.alloc(&ctx, 3) == CE_OK);
        h2 = std::move(h);
        ce_event e, e2;
        CHECK(e.create(&ctx) == CE_OK);
        e2 = std::move(e);
        ce_event e3(std::move(e2));
        CHECK(!e && !e2 && e3);
        ce_stream s, s2;
        CHECK(s.create(&ctx) == CE_OK);
        s2 = std::move(s);
        CHECK(!s && s2 && live() == 4);
        s2.reset();
        s2.reset();  // twice: nothing to release the second time
        CHECK(live() == 3);
    }
    CHECK(live() == 0 && g_acquired == g_released);
    // a whole set: move construction and assignment, then one release per allocation
    {
        batch b{&ctx, {}};
        CHECK(prepare(&b) == CE_OK && prepare_half(&b) == CE_OK);
        const long held = (long)live(), released = g_released;
        working_set moved(std::move(b.set));
        CHECK(!b.set.engaged() && !b.set.half.ev_fork && moved.engaged() && (long)live() == held && g_released == released);
        batch other{&ctx, {}};
        CHECK(prepare(&other) == CE_OK);
        other.set = std::move(moved);  // what `other` held goes, what `moved` held stays
        CHECK(g_released == released + kSetAcquisitions && (long)live() == held && other.set.half.stream == kBorrowed);
    }
    CHECK(live() == 0 && g_acquired == g_released);
}

static void test_reserve()
{
    arm(0);
    ce_ctx ctx;
    {
        ce_dev<float> cells;
        CHECK(cells.reserve(&ctx, 10) == CE_OK && cells.size() == 10 && live() == 1);
        float *const p = cells;
        const long acquired = g_acquired;
        CHECK(cells.reserve(&ctx, 10) == CE_OK && cells.reserve(&ctx, 3) == CE_OK);  // fits: kept
        CHECK(cells.get() == p && cells.size() == 10 && g_acquired == acquired);
        CHECK(cells.reserve(&ctx, 11) == CE_OK && cells.size() == 11);  // grows: one block, the old one released
        CHECK(live() == 1 && g_acquired == acquired + 1 && g_released == g_acquired - 1);
        arm(1);
        CHECK(cells.reserve(&ctx, 100) == CE_ERR_BACKEND);  // fails: empty, nothing held, nothing leaked
        CHECK(!cells && cells.size() == 0 && live() == 0);
        arm(0);
        CHECK(cells.reserve(&ctx, 5) == CE_OK && cells.size() == 5 && live() == 1);  // and usable again
    }
    CHECK(live() == 0 && g_acquired == g_released);
}

static void test_error_string()
{
    ce_ctx ctx;
    ce_dev<float> d;
    ce_pinned<float> h;
    ce_event e;
    ce_stream s;
    const long reads = g_last_error_reads;
    arm(1);
    CHECK(d.alloc(&ctx, 4) == CE_ERR_BACKEND && ctx.err == "hipMalloc: out of memory");
    CHECK(g_last_error_reads == reads + 1);  // the failure does not stay pending for a later hipGetLastError
    arm(1);
    CHECK(d.alloc(&ctx, 4, "hipMalloc refs") == CE_ERR_BACKEND && ctx.err == "hipMalloc refs: out of memory");
    arm(1);
    CHECK(h.alloc(&ctx, 4) == CE_ERR_BACKEND && ctx.err == "hipHostMalloc: out of memory");
    arm(1);
    CHECK(e.create(&ctx) == CE_ERR_BACKEND && ctx.err == "hipEventCreate: out of memory" && !e);
    arm(1);
    CHECK(s.create(&ctx, "hipStreamCreate upload") == CE_ERR_BACKEND && ctx.err == "hipStreamCreate upload: out of memory" && !s);
    ctx.err = "kept";
    arm(1);
    CHECK(d.alloc((ce_ctx *)nullptr, 4) == CE_ERR_BACKEND && ctx.err == "kept");  // without a context: no string
    arm(0);
    CHECK(live() == 0);
}

int main()
{
    test_all_or_nothing();
    test_lazy_extra();
    test_moves();
    test_reserve();
    test_error_string();
    CHECK(live() == 0 && g_acquired == g_released && g_acquired > 0);
    std::printf("owned OK (%ld acquisitions, %ld releases)\n", g_acquired, g_released);
    return 0;
}
