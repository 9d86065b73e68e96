// Host runtime behind the C ABI (include/ce_metrics.h): errors, profiling hooks, the device copy of a host table, contexts,
// the HBM-resident pair grid (batch lifetime, launch, collect, the map read-outs, HDR fidelity and image heuristics of a
// batch's slabs), shape bucketing for mixed batches (ce_eval_batch), reference handles, the debug hooks.  Everything that
// writes a slot of a batch is in ce_ingest.cpp, every call that takes host images and returns a result through scratch the
// context owns in ce_leaf.cpp, resampling in ce_resample.cpp.  All device work is in the .hip files; there is no CPU compute
// path here — if HIP is unavailable every entry point fails with CE_ERR_BACKEND.
#include <algorithm>
#include <atomic>
#include <condition_variable>
#include <functional>
#include <mutex>
#include <thread>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <new>

#include "ce_internal.h"

static thread_local std::string g_err_noctx;

int ce_fail(ce_ctx *ctx, int code, const std::string &msg)
{
    if (ctx) ctx->err = msg; else g_err_noctx = msg;
    return code;
}

int ce_bad_length(ce_ctx *ctx, size_t want, size_t got)
{
    return ce_fail(ctx, CE_ERR_BAD_LENGTH, "Invalid image size: expected " + std::to_string(want) + " bytes, got " + std::to_string(got));
}

// validation order of calculate_ssimulacra2 / calculate_butteraugli
// (src/metrics/ssimulacra2.rs:65-82, src/metrics/butteraugli.rs:51-67)
int ce_validate_pair(ce_ctx *ctx, size_t ref_len, size_t test_len, size_t w, size_t h)
{
    if (ref_len != test_len)
        return ce_fail(ctx, CE_ERR_DIM_MISMATCH, "Dimension mismatch: reference " + std::to_string(ref_len) +
                                                   " bytes, test " + std::to_string(test_len) + " bytes");
    if (ref_len != w * h * 3) return ce_bad_length(ctx, w * h * 3, ref_len);
    return CE_OK;
}

// A new device copy of a host table (ce_internal.h).  The context's table maps all fill through here: find; else build on
// the host, copy, emplace.
int ce_device_table(ce_ctx *ctx, const void *host, size_t bytes, const char *what, void **out)
{
    void *d = nullptr;
    CE_HIP(ctx, hipMalloc(&d, bytes));
    if (hipMemcpy(d, host, bytes, hipMemcpyHostToDevice) != hipSuccess) {
        hipFree(d);
        return ce_fail(ctx, CE_ERR_BACKEND, std::string("H2D failed (") + what + ")");
    }
    *out = d;
    return CE_OK;
}

// the argument checks of every map readout (what = "diffmap" / "SSIM map"): pairs [first, first + count) of the `stored`
// ones of the last launch, block 1 or a power of two up to 64, and out_floats = count * ceil(w / B) * ceil(h / B) floats of
// a w x h map (0 when there is no map output)
static int check_map_readout(ce_ctx *ctx, const char *what, uint32_t stored, uint32_t first, uint32_t count, uint32_t block, uint32_t w,
                      uint32_t h, bool has_out, size_t out_floats)
{
    if (count == 0 || first > stored || count > stored - first)
        return ce_fail(ctx, CE_ERR_INVALID_ARG, std::string(what) + " pairs [" + std::to_string(first) + ", " + std::to_string((uint64_t)first + count) +
                                                 ") outside the " + std::to_string(stored) + " stored");
    if (block == 0 || block > 64 || (block & (block - 1)) != 0)
        return ce_fail(ctx, CE_ERR_INVALID_ARG, std::string(what) + " block must be 1 or a power of two up to 64");
    const size_t want = has_out ? (size_t)count * ((w + block - 1) / block) * ((h + block - 1) / block) : 0;
    if (out_floats != want)
        return ce_fail(ctx, CE_ERR_INVALID_ARG, std::string(what) + " readout needs " + std::to_string(want) + " floats, got " + std::to_string(out_floats));
    return CE_OK;
}

// the readouts of CE_FLAG_BUTTERAUGLI_DIFFMAP (also behind ce_ref_butteraugli_diffmap and ce_calculate_butteraugli_diffmap):
// checks, then the device readout (butteraugli.hip)
int ce_batch_butteraugli_diffmap(ce_batch *b, uint32_t first, uint32_t count, uint32_t block, float *out, size_t out_floats)
{
    if (!b || !out) return CE_ERR_INVALID_ARG;
    ce_ctx *ctx = b->ctx;
    if (b->ba_map_pairs == 0)
        return ce_fail(ctx, CE_ERR_INVALID_ARG, "no Butteraugli diffmaps: the last launch did not run Butteraugli with CE_FLAG_BUTTERAUGLI_DIFFMAP");
    if (int rc = check_map_readout(ctx, "diffmap", b->ba_map_pairs, first, count, block, b->w, b->h, true, out_floats)) return rc;
    CE_HIP(ctx, hipSetDevice(ctx->device));
    return ce_butteraugli_read_maps(b, first, count, block, out);
}

// the readouts of DSSIM's SsimMap (also behind ce_ref_dssim_ssim_maps and ce_calculate_dssim_ssim_maps): checks, then the
// device readout (dssim.hip)
int ce_batch_dssim_ssim_maps(ce_batch *b, uint32_t level, uint32_t first, uint32_t count, uint32_t block, float *maps,
                             size_t maps_floats, double *ssim)
{
    if (!b || (!maps && !ssim)) return CE_ERR_INVALID_ARG;
    ce_ctx *ctx = b->ctx;
    if (b->ds_map_pairs == 0) return ce_fail(ctx, CE_ERR_INVALID_ARG, "no DSSIM SSIM maps: the last launch did not run DSSIM");
    if (level >= (uint32_t)b->ds.levels)
        return ce_fail(ctx, CE_ERR_INVALID_ARG, "DSSIM level " + std::to_string(level) + " of " + std::to_string(b->ds.levels));
    const auto &d = b->ds.lvl[level];
    if (int rc = check_map_readout(ctx, "SSIM map", b->ds_map_pairs, first, count, block, d.w, d.h, maps != nullptr, maps_floats)) return rc;
    CE_HIP(ctx, hipSetDevice(ctx->device));
    return ce_dssim_read_maps(b, level, first, count, block, maps, ssim);
}

// the readouts of SSIMULACRA2's maps and their norms (also behind ce_ref_ssimulacra2_maps and ce_calculate_ssimulacra2_maps):
// checks, then the device readout (ssim2.hip).  Norms need a last launch with SSIMULACRA2, maps one with
// CE_FLAG_SSIMULACRA2_MAPS too.
int ce_batch_ssimulacra2_maps(ce_batch *b, uint32_t scale, uint32_t channel, uint32_t kind, uint32_t first, uint32_t count,
                              uint32_t block, float *maps, size_t maps_floats, double *norms)
{
    if (!b) return ce_fail(nullptr, CE_ERR_INVALID_ARG, "null handle");
    ce_ctx *ctx = b->ctx;
    if (!maps && !norms) return ce_fail(ctx, CE_ERR_INVALID_ARG, "SSIMULACRA2 maps readout without an output");
    if (b->s2_norm_pairs == 0)
        return ce_fail(ctx, CE_ERR_INVALID_ARG, "no SSIMULACRA2 maps or norms: the last launch did not run SSIMULACRA2");
    if (maps && b->s2_map_pairs == 0)
        return ce_fail(ctx, CE_ERR_INVALID_ARG, "no SSIMULACRA2 maps: the last launch did not run SSIMULACRA2 with CE_FLAG_SSIMULACRA2_MAPS");
    if (scale >= b->s2_scales_run)
        return ce_fail(ctx, CE_ERR_INVALID_ARG, "SSIMULACRA2 scale " + std::to_string(scale) + " of " + std::to_string(b->s2_scales_run) + " that ran");
    if (channel >= 3) return ce_fail(ctx, CE_ERR_INVALID_ARG, "SSIMULACRA2 channel " + std::to_string(channel) + " of 3");
    if (kind >= 3) return ce_fail(ctx, CE_ERR_INVALID_ARG, "SSIMULACRA2 map kind " + std::to_string(kind) + " of 3");
    const ce_plane_geom &d = b->s2.lvl[scale];
    if (int rc = check_map_readout(ctx, "SSIMULACRA2 map", maps ? b->s2_map_pairs : b->s2_norm_pairs, first, count, block, d.w, d.h,
                                   maps != nullptr, maps_floats))
        return rc;
    CE_HIP(ctx, hipSetDevice(ctx->device));
    return ce_ssim2_read_maps(b, scale, channel, kind, first, count, block, maps, norms);
}

static double psnr_from_sse(unsigned long long sse, size_t w, size_t h, double maxv = 255.0)
{
    // src/metrics/mod.rs:317,324-330 (a deep batch: 255 replaced by its 2^depth - 1)
    const double pixel_count = (double)(w * h * 3);
    const double mse = (double)sse / pixel_count;
    if (mse == 0.0) return INFINITY;
    return 10.0 * std::log10(maxv * maxv / mse);
}

// The sRGB -> linear table of a deep batch's side on the device: 2^depth entries by `rule` (0: ce_build_srgb_table_f64,
// 1: ce_build_srgb_table_powf), built once per context and kept (ce_ctx::deep_tables).
static int ce_deep_table(ce_ctx *ctx, uint32_t depth, int rule, const float **out)
{
    const auto key = std::make_pair(depth, rule);
    auto it = ctx->deep_tables.find(key);
    if (it == ctx->deep_tables.end()) {
        const uint32_t maxv = (1u << depth) - 1u;
        std::vector<float> host((size_t)maxv + 1);
        if (rule == 0) ce_build_srgb_table_f64(host.data(), maxv); else ce_build_srgb_table_powf(host.data(), maxv);
        void *d = nullptr;
        if (int rc = ce_device_table(ctx, host.data(), host.size() * sizeof(float), "deep sRGB table", &d)) return rc;
        it = ctx->deep_tables.emplace(key, static_cast<float *>(d)).first;
    }
    *out = it->second;
    return CE_OK;
}

// ---- profiling -----------------------------------------------------------------------------

int ce_prof_begin(ce_ctx *ctx, const char *name, hipStream_t stream)
{
    if (!ctx->prof_filter.empty()) {  // "=name": that kernel only; otherwise a substring
        const char *f = ctx->prof_filter.c_str();
        if (f[0] == '=' ? std::strcmp(name, f + 1) != 0 : !std::strstr(name, f)) return -1;
    }
    int idx = -1;
    for (size_t i = 0; i < ctx->stats.size(); i++)
        if (ctx->stats[i].name == name) { idx = (int)i; break; }
    if (idx < 0) {
        ctx->stats.push_back(ce_kernel_stat{name, 0, 0.0});
        idx = (int)ctx->stats.size() - 1;
    }
    ce_ctx::pending pd{idx, nullptr, nullptr};
    for (hipEvent_t *e : {&pd.e0, &pd.e1}) {
        if (!ctx->event_pool.empty()) {
            *e = ctx->event_pool.back();
            ctx->event_pool.pop_back();
        } else if (hipEventCreate(e) != hipSuccess) {
            return -1;
        }
    }
    hipEventRecord(pd.e0, stream);
    ctx->pend.push_back(pd);
    return (int)ctx->pend.size() - 1;
}

void ce_prof_end(ce_ctx *ctx, int token, hipStream_t stream) { hipEventRecord(ctx->pend[token].e1, stream); }

static void prof_drain(ce_ctx *ctx)
{
    if (ctx->pend.empty()) return;
    hipSetDevice(ctx->device);
    hipStreamSynchronize(ctx->stream);
    for (auto &pd : ctx->pend) {
        float ms = 0.f;
        if (hipEventElapsedTime(&ms, pd.e0, pd.e1) == hipSuccess) {
            ctx->stats[pd.stat].launches++;
            ctx->stats[pd.stat].total_ms += ms;
        }
        ctx->event_pool.push_back(pd.e0);
        ctx->event_pool.push_back(pd.e1);
    }
    ctx->pend.clear();
}

// The XCD-aware work list (ce_plan.h: ce_plan_xcd_list) of batch b's first n_pairs pairs, on the device.  Rebuilt only
// when one of its inputs changes: the pair -> reference table, the pair count or the keys.
int ce_build_xcd_list(ce_batch *b, uint32_t n_pairs, const ce_xcd_keys &keys, ce_xcd_list *L)
{
    static_assert(sizeof(ce_plan_entry) == sizeof(uint2) && alignof(ce_plan_entry) <= alignof(uint2), "entries are read as uint2");
    if (L->d && L->version == b->pair_ref_version && L->pairs == n_pairs && L->keys == keys) return CE_OK;
    ce_ctx *ctx = b->ctx;
    const std::vector<ce_plan_entry> flat = ce_plan_xcd_list(b->h_pair_ref.data(), n_pairs, b->max_refs, keys);
    if (int rc = L->d.reserve(ctx, flat.size())) return rc;
    if (int rc = ce_upload_table(b, L->d, flat.data(), flat.size() * sizeof(uint2))) return rc;  // `flat` is pageable and goes out of scope
    L->len = (uint32_t)flat.size();
    L->version = b->pair_ref_version;
    L->pairs = n_pairs;
    L->keys = keys;
    return CE_OK;
}

thread_local hipStream_t ce_tls_stream = nullptr;  // ce_internal.h: CE_STREAM

// Host table -> device memory of batch `b`, complete when this returns.  Work lists and the pair -> reference table are
// built in pageable vectors, so the host has to wait for the copy - but NOT for the context's stream: round 2 copied on
// that stream and drained it, which made every ce_eval_batch chunk whose pair count differs from the slot's previous one
// wait for the kernels of the chunk before it, and its uploads no longer overlapped them (profiles/r03_experiments.md
// section 17: 141 -> see there).  The copy runs on the batch's upload stream, behind the previous launch of THIS batch
// (which may still read the old table) and behind the image uploads already queued there.
int ce_upload_table(ce_batch *b, void *dst, const void *src, size_t bytes)
{
    ce_ctx *ctx = b->ctx;
    if (bytes == 0) return CE_OK;
    CE_HIP(ctx, hipStreamWaitEvent(b->up_stream, b->ev_run, 0));  // never recorded = no wait
    CE_HIP(ctx, hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, b->up_stream));
    CE_HIP(ctx, hipStreamSynchronize(b->up_stream));
    return CE_OK;
}

hipStream_t ce_ctx_aux_stream(ce_ctx *ctx, int which)
{
    if (which < 0 || which >= ce_ctx::AUX_COUNT) return nullptr;
    if (!ctx->aux_stream[which]) {
        const hipError_t e = hipStreamCreateWithFlags(&ctx->aux_stream[which], hipStreamNonBlocking);
        if (e != hipSuccess) {
            ctx->aux_stream[which] = nullptr;
            ctx->err = std::string("hipStreamCreateWithFlags (auxiliary stream): ") + hipGetErrorString(e);
        }
    }
    return ctx->aux_stream[which];
}

// a failed call may leave copies from the caller's page-locked buffers queued: drain them before the buffers can go away
void ce_drain_batch(ce_batch *b)
{
    hipStreamSynchronize(b->up_stream);
    if (b->ctx->up2_stream) hipStreamSynchronize(b->ctx->up2_stream);
    hipStreamSynchronize(b->ctx->stream);
}

// the device copies a table map of the context holds (ce_device_table made them), freed with the context
static void *table_of(float *p) { return p; }
static void *table_of(const ce_resample_axis &a) { return a.d; }
template <class Map>
static void free_tables(Map &m)
{
    for (auto &kv : m) hipFree(table_of(kv.second));
    m.clear();
}

static bool hdr_depth_ok(uint32_t d) { return d == 10 || d == 12 || d == 16; }

// HDR fidelity's two parameters, for ce_batch_hdr_fidelity and ce_eval_pair_hdr_fidelity (ce_leaf.cpp)
int ce_hdr_params_check(ce_ctx *ctx, uint32_t depth, float white_nits)
{
    if (!hdr_depth_ok(depth)) return ce_fail(ctx, CE_ERR_INVALID_ARG, "HDR fidelity: depth must be 10, 12 or 16, got " + std::to_string(depth));
    if (!(white_nits > 0.0f && std::isfinite(white_nits))) return ce_fail(ctx, CE_ERR_INVALID_ARG, "HDR fidelity: white_nits must be finite and > 0");
    return CE_OK;
}

extern "C" {

const char *ce_version(void) { return "codec-eval_amd 0.3.0 (gfx950)"; }

int ce_device_count(void)
{
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return -1;
    return n;
}

int ce_ctx_create_on_stream(int device, void *hip_stream, ce_ctx **out)
{
    if (!out) return CE_ERR_INVALID_ARG;
    *out = nullptr;
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0)
        return ce_fail(nullptr, CE_ERR_BACKEND, "no HIP device visible");
    if (device < 0 || device >= n) return ce_fail(nullptr, CE_ERR_INVALID_ARG, "device index out of range");
    ce_ctx *ctx = new (std::nothrow) ce_ctx();
    if (!ctx) return CE_ERR_BACKEND;
    ctx->device = device;
    auto bail = [&](const char *what, hipError_t e) {
        g_err_noctx = std::string(what) + ": " + hipGetErrorString(e);
        delete ctx;
        return CE_ERR_BACKEND;
    };
    hipError_t e;
    if ((e = hipSetDevice(device)) != hipSuccess) return bail("hipSetDevice", e);
    if (hip_stream) {
        ctx->stream = (hipStream_t)hip_stream;
        ctx->own_stream = false;
    } else {
        if ((e = hipStreamCreateWithFlags(&ctx->stream, hipStreamNonBlocking)) != hipSuccess)
            return bail("hipStreamCreate", e);
    }
    float lut[256];
    if ((e = hipMalloc(&ctx->d_lut_ssim2, sizeof(lut))) != hipSuccess) return bail("hipMalloc", e);
    if ((e = hipMalloc(&ctx->d_lut_powf, sizeof(lut))) != hipSuccess) return bail("hipMalloc", e);
    ce_build_srgb_lut_f64(lut);
    if ((e = hipMemcpy(ctx->d_lut_ssim2, lut, sizeof(lut), hipMemcpyHostToDevice)) != hipSuccess)
        return bail("hipMemcpy", e);
    ce_build_srgb_lut_powf(lut);
    if ((e = hipMemcpy(ctx->d_lut_powf, lut, sizeof(lut), hipMemcpyHostToDevice)) != hipSuccess)
        return bail("hipMemcpy", e);
    float thresh[256];
    if (!ce_build_xyb_srgb_thresholds(thresh)) {
        g_err_noctx = "host powf is not monotone around an sRGB code boundary; cannot build the XYB table";
        delete ctx;
        return CE_ERR_BACKEND;
    }
    if ((e = hipMalloc(&ctx->d_xyb_thresh, sizeof(thresh))) != hipSuccess) return bail("hipMalloc", e);
    if ((e = hipMemcpy(ctx->d_xyb_thresh, thresh, sizeof(thresh), hipMemcpyHostToDevice)) != hipSuccess)
        return bail("hipMemcpy", e);
    if ((e = hipEventCreate(&ctx->t0)) != hipSuccess) return bail("hipEventCreate", e);
    if ((e = hipEventCreate(&ctx->t1)) != hipSuccess) return bail("hipEventCreate", e);
    *out = ctx;
    return CE_OK;
}

int ce_ctx_create(int device, ce_ctx **out) { return ce_ctx_create_on_stream(device, nullptr, out); }

// Parked helper threads of a context.  Round 2 spawned a std::thread per chain and call: creating a thread and making its
// first HIP call cost ~50-100 us, more than the 0.2 ms of launches it was meant to overlap (a single 768x512 pair traced in
// round 3: 96 us between the upload and the first kernel, the third chain starting 190 us after the first).  A helper sets
// its device once and sleeps on a condition variable between jobs.
struct ce_fork_helpers {
    struct worker {
        std::thread th;
        std::mutex m;
        std::condition_variable cv;
        std::function<void()> job;
        bool has_job = false, done = true, stop = false;
    } w[2];
    explicit ce_fork_helpers(int device)
    {
        try {
            for (auto &x : w)
                x.th = std::thread([&x, device] {
                    (void)hipSetDevice(device);
                    std::unique_lock<std::mutex> lk(x.m);
                    for (;;) {
                        x.cv.wait(lk, [&] { return x.has_job || x.stop; });
                        if (x.stop) return;
                        x.has_job = false;
                        lk.unlock();
                        x.job();
                        lk.lock();
                        x.done = true;
                        x.cv.notify_all();
                    }
                });
        } catch (...) {  // a thread could not be created: stop and join the ones that were, then let the caller fall back
            stop_all();
            throw;
        }
    }
    void submit(int i, std::function<void()> f)
    {
        std::lock_guard<std::mutex> lk(w[i].m);
        w[i].job = std::move(f);
        w[i].has_job = true;
        w[i].done = false;
        w[i].cv.notify_all();
    }
    void wait(int i)
    {
        std::unique_lock<std::mutex> lk(w[i].m);
        w[i].cv.wait(lk, [&] { return w[i].done; });
    }
    ~ce_fork_helpers() { stop_all(); }
    void stop_all()
    {
        for (auto &x : w) {
            {
                std::lock_guard<std::mutex> lk(x.m);
                x.stop = true;
                x.cv.notify_all();
            }
            if (x.th.joinable()) x.th.join();
        }
    }
};

void ce_ctx_destroy(ce_ctx *ctx)
{
    if (!ctx) return;
    hipSetDevice(ctx->device);
    hipStreamSynchronize(ctx->stream);
    delete ctx->helpers;
    ctx->helpers = nullptr;

    prof_drain(ctx);
    for (auto &kv : ctx->shape_pool) ce_batch_destroy(kv.second);
    ctx->shape_pool.clear();
    for (ce_batch *&b : ctx->leaf_batch) ce_batch_destroy(b), b = nullptr;
    free_tables(ctx->deep_tables);
    free_tables(ctx->cicp_tables);
    free_tables(ctx->hdr_tables);
    free_tables(ctx->icc_thresholds);
    free_tables(ctx->alpha_tables);
    if (ctx->up2_stream) hipStreamSynchronize(ctx->up2_stream), hipStreamDestroy(ctx->up2_stream), hipEventDestroy(ctx->ev_up2);
    for (auto &st : ctx->aux_stream)  // after the last batch that may still drain them
        if (st) hipStreamSynchronize(st), hipStreamDestroy(st), st = nullptr;
    for (hipEvent_t ev : ctx->event_pool) hipEventDestroy(ev);
    if (ctx->t0) hipEventDestroy(ctx->t0);
    if (ctx->t1) hipEventDestroy(ctx->t1);
    hipFree(ctx->leaf_d_in);
    hipFree(ctx->leaf_d_out);
    if (ctx->leaf_h) hipHostFree(ctx->leaf_h);
    hipFree(ctx->heur_d);
    if (ctx->heur_h) hipHostFree(ctx->heur_h);
    hipFree(ctx->rs_mid);
    free_tables(ctx->rs_tables);
    hipFree(ctx->d_lut_ssim2);
    hipFree(ctx->d_lut_powf);
    hipFree(ctx->d_xyb_thresh);
    if (ctx->own_stream && ctx->stream) hipStreamDestroy(ctx->stream);
    delete ctx;
}

int ce_ctx_synchronize(ce_ctx *ctx)
{
    if (!ctx) return CE_ERR_INVALID_ARG;
    CE_HIP(ctx, hipSetDevice(ctx->device));
    CE_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return CE_OK;
}

void *ce_ctx_stream(ce_ctx *ctx) { return ctx ? (void *)ctx->stream : nullptr; }

// batches launched and not yet collected, per device, over all contexts of the process: ce_batch_launch forks a larger
// batch's metric chains only when nothing else is in flight beside it
static std::atomic<int> g_in_flight[64];
static std::atomic<int> &in_flight_of(const ce_ctx *ctx) { return g_in_flight[(unsigned)ctx->device % 64u]; }
static void leave_flight(ce_batch *b)
{
    if (b->counted_in_flight) {
        in_flight_of(b->ctx).fetch_sub(1, std::memory_order_relaxed);
        b->counted_in_flight = false;
    }
}

const char *ce_last_error(const ce_ctx *ctx) { return ctx ? ctx->err.c_str() : g_err_noctx.c_str(); }

// ---- resident batch ------------------------------------------------------------------------

// ref_depth = test_depth = 0: an RGB8 batch; otherwise a deep one (checked by the caller)
// linear: packed f32 RGB slabs (ce_batch_create_linear; depths 0 / 0)
static int batch_create(ce_ctx *ctx, uint32_t width, uint32_t height, uint32_t max_refs, uint32_t max_pairs, uint32_t ref_depth,
                        uint32_t test_depth, ce_batch **out, bool linear = false)
{
    if (!ctx || !out || width == 0 || height == 0 || max_refs == 0 || max_pairs == 0) return CE_ERR_INVALID_ARG;
    *out = nullptr;
    CE_HIP(ctx, hipSetDevice(ctx->device));
    const float *deep_lut[2][2] = {};
    if (ref_depth)
        for (int rule = 0; rule < 2; rule++)
            for (int side = 0; side < 2; side++)
                if (int rc = ce_deep_table(ctx, side ? test_depth : ref_depth, rule, &deep_lut[rule][side])) return rc;
    ce_batch *b = new (std::nothrow) ce_batch();
    if (!b) return CE_ERR_BACKEND;
    b->ctx = ctx;
    b->w = width;
    b->h = height;
    b->max_refs = max_refs;
    b->max_pairs = max_pairs;
    b->img_bytes = (size_t)width * height * (linear ? 12 : ref_depth ? 6 : 3);
    b->linear = linear;
    b->depth[0] = ref_depth, b->depth[1] = test_depth;
    std::memcpy(b->deep_lut, deep_lut, sizeof(deep_lut));
    b->h_pair_ref.assign(max_pairs, 0);
    // CE_KEEP_REFERENCE_STATE=0: an ordinary batch rebuilds its reference-side planes on every launch, for A/B runs
    static const bool keep_reference_state = [] { const char *e = std::getenv("CE_KEEP_REFERENCE_STATE"); return !(e && e[0] == '0'); }();
    b->refs.keep = keep_reference_state;
    // +16 bytes: the PSNR kernel reads whole 16-byte words
    int rc = b->d_refs.alloc(ctx, b->img_bytes * max_refs + 16, "hipMalloc refs");
    if (rc == CE_OK) rc = b->d_tests.alloc(ctx, b->img_bytes * max_pairs + 16, "hipMalloc tests");
    // [pair_ref (P) | pair_first (P) | ref_off (R + 1) | ref_idx (P)]
    if (rc == CE_OK) rc = b->d_pair_ref.alloc(ctx, 3 * (size_t)max_pairs + max_refs + 1, "hipMalloc pair_ref");
    if (rc == CE_OK) {
        b->d_pair_first = b->d_pair_ref + max_pairs;
        b->d_ref_off = b->d_pair_ref + 2 * (size_t)max_pairs;
        b->d_ref_idx = b->d_ref_off + max_refs + 1;
        rc = b->d_scores.alloc(ctx, max_pairs, "hipMalloc scores");
    }
    if (rc == CE_OK) rc = b->h_scores.alloc(ctx, max_pairs, "hipHostMalloc scores");
    if (rc == CE_OK) rc = b->up_stream.create(ctx, "hipStreamCreate upload");
    if (rc == CE_OK) rc = b->ev_up.create(ctx);
    if (rc == CE_OK) rc = b->ev_run.create(ctx);
    for (int k = 0; k < ce_batch::kStages && rc == CE_OK; k++) {
        rc = b->h_stage[k].alloc(ctx, b->img_bytes, "hipHostMalloc stage");
        if (rc == CE_OK) rc = b->ev_stage[k].create(ctx, "hipEventCreate stage");
    }
    if (rc == CE_OK) rc = ce_owned_status(ctx, hipMemsetAsync(b->d_scores, 0, sizeof(ce_dev_scores) * max_pairs, ctx->stream), "memset");
    if (rc != CE_OK) {
        ce_batch_destroy(b);
        return rc;
    }
    *out = b;
    return CE_OK;
}

int ce_batch_create(ce_ctx *ctx, uint32_t width, uint32_t height, uint32_t max_refs, uint32_t max_pairs, ce_batch **out)
{
    return batch_create(ctx, width, height, max_refs, max_pairs, 0, 0, out);
}

int ce_batch_create_deep(ce_ctx *ctx, uint32_t width, uint32_t height, uint32_t max_refs, uint32_t max_pairs, uint32_t ref_depth,
                         uint32_t test_depth, ce_batch **out)
{
    if (!ctx || !out) return CE_ERR_INVALID_ARG;
    *out = nullptr;
    if (!ce_deep_depth_ok(ref_depth) || !ce_deep_depth_ok(test_depth))
        return ce_fail(ctx, CE_ERR_INVALID_ARG, "a deep batch's depths must be 8, 10, 12 or 16 bits, got " + std::to_string(ref_depth) +
                                                 " / " + std::to_string(test_depth));
    return batch_create(ctx, width, height, max_refs, max_pairs, ref_depth, test_depth, out);
}

int ce_batch_create_linear(ce_ctx *ctx, uint32_t width, uint32_t height, uint32_t max_refs, uint32_t max_pairs, ce_batch **out)
{
    return batch_create(ctx, width, height, max_refs, max_pairs, 0, 0, out, true);
}

void ce_batch_destroy(ce_batch *b)
{
    if (!b) return;
    hipSetDevice(b->ctx->device);
    hipStreamSynchronize(b->ctx->stream);
    leave_flight(b);
    // what the batch queued elsewhere: its uploads, and the context's auxiliary streams it used (drained, never destroyed
    // here); then every owner in the batch releases itself
    if (b->up_stream) hipStreamSynchronize(b->up_stream);
    for (hipStream_t st : {b->fork[0].stream, b->fork[1].stream, b->fork[2].stream, b->s2.l0_stream, b->ba.half.stream})
        if (st) hipStreamSynchronize(st);
    delete b;
}

// the pair -> reference table of the batch on the device, as the last ce_batch_bind_pair left it
static int sync_pair_ref(ce_batch *b)
{
    if (!b->pair_ref_dirty) return CE_OK;
    // pair_first[p] = the lowest pair index bound to the same reference as p: that pair's row pass also produces
    // the two reference-only blur streams (a, a*a) which every pair of the reference then reads (ssim2.hip)
    // ... and the inverse table, reference -> its pairs in ascending pair order (kernels that walk a reference's
    // distorted images with the reference's planes held in registers: dssim.hip)
    const size_t P = b->max_pairs, R = b->max_refs;
    std::vector<uint32_t> table(3 * P + R + 1), first_of(R, ~0u), count(R + 1, 0);
    for (uint32_t i = 0; i < P; i++) {
        const uint32_t r = b->h_pair_ref[i];
        if (first_of[r] == ~0u) first_of[r] = i;
        table[i] = r;
        table[P + i] = first_of[r];
        count[r + 1]++;
    }
    for (size_t r = 0; r < R; r++) count[r + 1] += count[r];
    for (size_t r = 0; r <= R; r++) table[2 * P + r] = count[r];
    std::vector<uint32_t> fill(count.begin(), count.end() - 1);
    for (uint32_t i = 0; i < P; i++) table[2 * P + R + 1 + fill[b->h_pair_ref[i]]++] = i;
    if (int rc = ce_upload_table(b, b->d_pair_ref, table.data(), sizeof(uint32_t) * table.size())) return rc;  // `table` is pageable
    b->pair_ref_dirty = false;
    return CE_OK;
}

// What a launch of DSSIM, SSIMULACRA2 and Butteraugli takes (ce_plan.h): their front ends put the
// launch's image slots, or a plane's rows, into a grid's y or z.  The rule counts the references the pairs name whether or not
// the launch would find their state kept, so a launch is refused or runs whatever ran before it.  PSNR takes any n_pairs.
static_assert(ce_grid_yz_max == CE_LAUNCH_GRID_MAX && ce_launch_slots_max == CE_LAUNCH_MAX_SLOTS &&
                  ce_ba_height_max == CE_BUTTERAUGLI_MAX_HEIGHT && ce_ssim2_height_max == CE_SSIMULACRA2_MAX_HEIGHT,
              "ce_plan.h and ce_metrics.h state the same limits");
static int launch_fits(ce_ctx *ctx, uint32_t w, uint32_t h, uint32_t n_refs_used, uint32_t n_pairs, uint32_t metric_mask)
{
    const bool ssim2 = (metric_mask & CE_METRIC_SSIMULACRA2) && w >= 8 && h >= 8, ba = (metric_mask & CE_METRIC_BUTTERAUGLI) && w >= 8 && h >= 8;
    if (!ssim2 && !ba && !(metric_mask & CE_METRIC_DSSIM)) return CE_OK;
    if ((uint64_t)n_refs_used + n_pairs > ce_launch_slots_max)
        return ce_fail(ctx, CE_ERR_INVALID_ARG,
                       "launch too large: " + std::to_string(n_refs_used) + " references + " + std::to_string(n_pairs) + " pairs = " +
                           std::to_string((uint64_t)n_refs_used + n_pairs) + " image slots, DSSIM, SSIMULACRA2 and Butteraugli take at most " +
                           std::to_string(ce_launch_slots_max) + " slots in one launch");
    if (ba && h > ce_ba_height_max)
        return ce_fail(ctx, CE_ERR_INVALID_ARG,
                       "image too tall: height " + std::to_string(h) + ", Butteraugli takes at most " + std::to_string(ce_ba_height_max) + " rows");
    if (ssim2 && h > ce_ssim2_height_max)
        return ce_fail(ctx, CE_ERR_INVALID_ARG,
                       "image too tall: height " + std::to_string(h) + ", SSIMULACRA2 takes at most " + std::to_string(ce_ssim2_height_max) + " rows");
    return CE_OK;
}

int ce_batch_launch(ce_batch *b, uint32_t n_pairs, uint32_t metric_mask, uint32_t flags, float intensity_target)
{
    if (!b) return CE_ERR_INVALID_ARG;
    ce_ctx *ctx = b->ctx;
    if (n_pairs == 0 || n_pairs > b->max_pairs) return ce_fail(ctx, CE_ERR_INVALID_ARG, "n_pairs out of range");
    if (metric_mask & ~ce_known_metrics) return ce_fail(ctx, CE_ERR_INVALID_ARG, "unknown metric bit");
    if (b->depth[0] && (flags & CE_FLAG_XYB_ROUNDTRIP))
        return ce_fail(ctx, CE_ERR_INVALID_ARG, "CE_FLAG_XYB_ROUNDTRIP quantises to 8 bits by definition: not for a deep batch");
    if (b->linear && (flags & CE_FLAG_XYB_ROUNDTRIP))
        return ce_fail(ctx, CE_ERR_INVALID_ARG, "CE_FLAG_XYB_ROUNDTRIP quantises to 8 bits by definition: not for a linear batch");
    uint32_t n_refs_used = 0;
    for (uint32_t i = 0; i < n_pairs; i++) n_refs_used = std::max(n_refs_used, b->h_pair_ref[i] + 1);
    // a launch that does not fit a grid is refused here: nothing has run, and every record of reference state stands
    if (int rc = launch_fits(ctx, b->w, b->h, n_refs_used, n_pairs, metric_mask)) return rc;
    b->ba_map_pairs = b->ds_map_pairs = 0;  // whatever happens below, no readout returns the maps of an earlier launch
    b->s2_map_pairs = b->s2_norm_pairs = 0;
    CE_HIP(ctx, hipSetDevice(ctx->device));
    {
        int rc = ce_flush_uploads(b);
        if (rc != CE_OK) return rc;
    }
    if (int rc = sync_pair_ref(b)) return rc;

    const uint8_t *d_refs = b->d_refs;
    if (flags & CE_FLAG_XYB_ROUNDTRIP) {
        // MetricConfig::xyb_roundtrip: every metric sees the roundtripped reference (session.rs:447-456)
        if (!b->d_refs_rt)
            if (int rc = b->d_refs_rt.alloc(ctx, b->img_bytes * b->max_refs + 16, "hipMalloc roundtripped refs")) return rc;
        if (!b->refs.reuse(CE_REF_ROUNDTRIP, b->d_refs, n_refs_used, 0)) {
            int rc = ce_launch_xyb_roundtrip(ctx, b->d_refs, b->d_refs_rt, (size_t)n_refs_used * b->w * b->h);
            if (rc != CE_OK) return rc;
            b->refs.built(CE_REF_ROUNDTRIP, b->d_refs, n_refs_used, 0);
        }
        d_refs = b->d_refs_rt;
    }
    // The three perceptual metrics are independent chains over their own buffers (PSNR - two short launches on the
    // context's stream - is enqueued after them, so that forked chains do not wait behind it).
    const bool run_ssim2 = (metric_mask & CE_METRIC_SSIMULACRA2) && b->w >= 8 && b->h >= 8;
    const bool run_dssim = (metric_mask & CE_METRIC_DSSIM) != 0;
    const bool run_ba = (metric_mask & CE_METRIC_BUTTERAUGLI) && b->w >= 8 && b->h >= 8;
    const bool store_maps = run_ba && (flags & CE_FLAG_BUTTERAUGLI_DIFFMAP);
    const bool store_ssim2_maps = run_ssim2 && (flags & CE_FLAG_SSIMULACRA2_MAPS);
    // Side by side or back to back?  Measured (profiles/r02_experiments.md sections 1, 12, 15): a SMALL batch is bound by
    // the latency of its ~130 dependent launches, and three chains side by side hide each other's gaps (one Kodak pair
    // 0.76 -> 0.54 ms, eight 1.37 -> 1.23 ms, one 4K pair 3.65 -> 2.94 ms); a LARGE grid fills the GPU from one chain,
    // and with other batches in flight beside it (two shape buckets, two steps) forked chains evict each other's
    // reference planes from L2 and halve each other's resident workgroups (Kodak grid 6.55 -> 7.55 ms per step).  So the
    // chains fork when the batch holds at most CE_METRIC_FORK_BELOW_MP megapixels of pairs (default 4), or at most
    // CE_METRIC_FORK_ALONE_BELOW_MP (default 64) while no other batch of this device is launched and uncollected, and run
    // back to back on the context's stream otherwise (SSIMULACRA2 still overlaps its level-0 passes with its tail
    // levels).  Scores do not depend on the schedule.
    // fork mask: bit k = metric chain k (0 SSIMULACRA2, 1 DSSIM, 2 Butteraugli) runs on its own stream beside the others.
    // CE_METRIC_STREAMS = "fork" (all three, always), "fork:dssim", "fork:ssim2,ba", ... (those, always), "serial" (never);
    // unset / "auto" = by size.
    static const int fork_mask_env = [] {
        const char *e = std::getenv("CE_METRIC_STREAMS");
        if (!e || std::strcmp(e, "auto") == 0) return -1;
        if (std::strncmp(e, "fork", 4) != 0) return 0;
        if (e[4] != ':') return 7;
        int m = 0;
        if (std::strstr(e + 5, "ssim2")) m |= 1;
        if (std::strstr(e + 5, "dssim")) m |= 2;
        if (std::strstr(e + 5, "ba")) m |= 4;
        return m;
    }();
    static const double fork_below_mp = [] {
        const char *e = std::getenv("CE_METRIC_FORK_BELOW_MP");
        return e ? std::atof(e) : CE_DEFAULT_FORK_BELOW_MP;
    }();
    static const double fork_alone_below_mp = [] {
        const char *e = std::getenv("CE_METRIC_FORK_ALONE_BELOW_MP");
        return e ? std::atof(e) : CE_DEFAULT_FORK_ALONE_BELOW_MP;
    }();
    const double batch_mp = (double)n_pairs * b->w * b->h * 1e-6;
    const int others = in_flight_of(ctx).load(std::memory_order_relaxed) - (b->counted_in_flight ? 1 : 0);
    const bool by_size = batch_mp <= fork_below_mp || (others <= 0 && batch_mp <= fork_alone_below_mp);
    const unsigned fork_wanted = fork_mask_env >= 0 ? (unsigned)fork_mask_env : (by_size ? 7u : 0u);
    const unsigned fork_mask = (!ctx->prof_serial && (int)run_ssim2 + (int)run_dssim + (int)run_ba > 1) ? fork_wanted : 0u;
    hipStream_t base = ctx->stream;
    if (fork_mask) {
        if (!b->ev_fork)
            if (int rc = b->ev_fork.create(ctx)) return rc;
        CE_HIP(ctx, hipEventRecord(b->ev_fork, base));
    }
    unsigned joined = 0;
    auto prepare_fork = [&](int k) -> int {  // the chain's stream exists and waits for the fork point
        if (!b->fork[k].stream) {  // the stream is seen only with its event
            ce_batch::metric_fork f;
            if (!(f.stream = ce_ctx_aux_stream(ctx, ce_ctx::AUX_METRIC0 + k))) return CE_ERR_BACKEND;
            if (int rc = f.ev_join.create(ctx)) return rc;
            b->fork[k] = std::move(f);
        }
        CE_HIP(ctx, hipStreamWaitEvent(b->fork[k].stream, b->ev_fork, 0));
        return CE_OK;
    };
    auto launch_metric = [&](int k) -> int {
        return k == 0   ? ce_launch_ssim2(b, d_refs, n_refs_used, n_pairs, store_ssim2_maps)
               : k == 1 ? ce_launch_dssim(b, d_refs, n_refs_used, n_pairs)
                        : ce_launch_butteraugli(b, d_refs, n_refs_used, n_pairs, intensity_target, store_maps);
    };
    // the chains are enqueued in this order: SSIMULACRA2 first is the fastest start (profiles/r02_experiments.md section 19)
    const bool runs[3] = {run_ssim2, run_dssim, run_ba};
    // A forked SMALL batch is bound by the host: the ~50 launches of the three chains take ~0.2 ms to enqueue one after
    // the other, and a chain cannot start before its first launch is enqueued.  So the chains of a fully forked batch are
    // enqueued by one host thread each (the caller's + two helpers; CE_STREAM makes a launch function enqueue on its
    // thread's chain stream); CE_FORK_THREADS=0 keeps the single-threaded enqueue for A/B runs.  Per-kernel event timing
    // (ce_prof_*) keeps its bookkeeping on one thread.
    static const bool fork_threads = [] { const char *e = std::getenv("CE_FORK_THREADS"); return !(e && e[0] == '0'); }();
    if (fork_mask == 7u && fork_threads && !ctx->prof) {
        int rcs[3] = {CE_OK, CE_OK, CE_OK};
        std::string errs[3];
        int last = -1;
        for (int k = 0; k < 3; k++)
            if (runs[k]) {
                int rc = prepare_fork(k);
                if (rc != CE_OK) return rc;
                last = k;
            }
        auto body = [&](int k) {
            ce_tls_stream = b->fork[k].stream;
            rcs[k] = launch_metric(k);
            ce_tls_stream = nullptr;
            if (rcs[k] == CE_OK && hipEventRecord(b->fork[k].ev_join, b->fork[k].stream) != hipSuccess) rcs[k] = CE_ERR_BACKEND;
        };
        if (!ctx->helpers) {
            try {
                ctx->helpers = new ce_fork_helpers(ctx->device);
            } catch (...) {  // no threads to be had: every chain is enqueued here (nothing may be thrown across the C ABI)
                ctx->helpers = nullptr;
            }
        }
        int used = 0;
        for (int k = 0; k < 3; k++) {
            if (!runs[k] || k == last) continue;
            if (ctx->helpers && used < 2)
                ctx->helpers->submit(used++, [&body, k] { body(k); });
            else
                body(k);
        }
        body(last);  // the caller's thread takes the last chain that runs
        for (int i = 0; i < used; i++) ctx->helpers->wait(i);
        for (int k = 0; k < 3; k++) {
            if (!runs[k]) continue;
            if (rcs[k] != CE_OK) return rcs[k];
            joined |= 1u << k;
        }
    } else {
        for (int k = 0; k < 3; k++) {
            if (!runs[k]) continue;
            if (!(fork_mask & (1u << k))) {
                int rc = launch_metric(k);
                if (rc != CE_OK) return rc;
                continue;
            }
            int rc = prepare_fork(k);
            if (rc != CE_OK) return rc;
            ce_tls_stream = b->fork[k].stream;  // the chain's launches go to its own stream
            rc = launch_metric(k);
            ce_tls_stream = nullptr;
            if (rc != CE_OK) return rc;
            CE_HIP(ctx, hipEventRecord(b->fork[k].ev_join, b->fork[k].stream));
            joined |= 1u << k;  // the context's stream waits for it after every chain has been launched
        }
    }
    if ((metric_mask & CE_METRIC_PSNR) && b->depth[0] == b->depth[1] && !b->linear) {  // sides of two depths, or floats, share no integer grid: no PSNR
        int rc = ce_launch_psnr(b, d_refs, n_pairs);
        if (rc != CE_OK) return rc;
    }
    for (int k = 0; k < 3; k++)
        if (joined & (1u << k)) CE_HIP(ctx, hipStreamWaitEvent(base, b->fork[k].ev_join, 0));
    b->last_n_pairs = n_pairs;
    b->last_mask = metric_mask;
    b->ba_map_pairs = store_maps ? n_pairs : 0;
    b->ds_map_pairs = run_dssim ? n_pairs : 0;  // DSSIM writes its SSIM maps on every launch
    b->s2_norm_pairs = run_ssim2 ? n_pairs : 0;  // ... and SSIMULACRA2 its pooled norms (d_avg)
    b->s2_map_pairs = store_ssim2_maps ? n_pairs : 0;
    b->s2_scales_run = run_ssim2 ? (uint32_t)std::min(b->s2.n_scales, b->debug_max_scales) : 0;
    // the scores come back behind the last kernel of THIS launch and ev_run marks them: ce_batch_collect waits for the event,
    // not for the stream (round 2 copied at collect time and drained the context's stream, so collecting one batch waited
    // for every batch launched after it - in ce_eval_batch the next chunk's upload then started only when the device was idle)
    CE_HIP(ctx, hipMemcpyAsync(b->h_scores, b->d_scores, sizeof(ce_dev_scores) * n_pairs, hipMemcpyDeviceToHost, ctx->stream));
    CE_HIP(ctx, hipEventRecord(b->ev_run, ctx->stream));
    b->run_pending = true;
    b->inline_pending = false;  // the next write on up_stream waits for ev_run, which is behind every inline write
    if (!b->counted_in_flight) {
        in_flight_of(ctx).fetch_add(1, std::memory_order_relaxed);
        b->counted_in_flight = true;
    }
    return CE_OK;
}

int ce_batch_collect(ce_batch *b, uint32_t n_pairs, ce_scores *out)
{
    if (!b || !out) return CE_ERR_INVALID_ARG;
    ce_ctx *ctx = b->ctx;
    if (n_pairs == 0 || n_pairs > b->max_pairs) return ce_fail(ctx, CE_ERR_INVALID_ARG, "n_pairs out of range");
    CE_HIP(ctx, hipSetDevice(ctx->device));
    if (n_pairs > b->last_n_pairs) return ce_fail(ctx, CE_ERR_INVALID_ARG, "collect asks for more pairs than the last launch ran");
    CE_HIP(ctx, hipEventSynchronize(b->ev_run));  // the launch's kernels and the copy of its scores into h_scores (ce_batch_launch)
    b->run_pending = false;
    leave_flight(b);
    const uint32_t mask = b->last_mask;
    for (uint32_t i = 0; i < n_pairs; i++) {
        ce_scores s{};
        s.status = CE_OK;
        const ce_dev_scores &d = b->h_scores[i];
        if ((mask & CE_METRIC_PSNR) && b->depth[0] == b->depth[1] && !b->linear) {
            s.psnr = psnr_from_sse(d.sse, b->w, b->h, b->depth[0] ? (double)((1u << b->depth[0]) - 1u) : 255.0);
            s.valid |= CE_METRIC_PSNR;
        }
        if (mask & CE_METRIC_DSSIM) {
            s.dssim = d.dssim;
            s.valid |= CE_METRIC_DSSIM;
        }
        if (mask & CE_METRIC_BUTTERAUGLI) {
            if (b->w < 8 || b->h < 8) {  // "minimum 8x8 for butteraugli", src/eval/helpers.rs:89
                s.status = CE_ERR_TOO_SMALL;
            } else {
                s.butteraugli = d.butteraugli;
                s.valid |= CE_METRIC_BUTTERAUGLI;
            }
        }
        if (mask & CE_METRIC_SSIMULACRA2) {
            if (b->w < 8 || b->h < 8) {
                s.status = CE_ERR_TOO_SMALL;
            } else {
                s.ssimulacra2 = d.ssimulacra2;
                s.valid |= CE_METRIC_SSIMULACRA2;
            }
        }
        out[i] = s;
    }
    return CE_OK;
}

int ce_batch_butteraugli_pnorm3(ce_batch *b, uint32_t n_pairs, double *out)
{
    if (!b || !out || !b->ba.engaged() || n_pairs == 0 || n_pairs > b->max_pairs) return CE_ERR_INVALID_ARG;
    ce_ctx *ctx = b->ctx;
    CE_HIP(ctx, hipSetDevice(ctx->device));
    CE_HIP(ctx, hipStreamSynchronize(ctx->stream));
    CE_HIP(ctx, hipMemcpy(out, b->ba.pnorm, sizeof(double) * n_pairs, hipMemcpyDeviceToHost));
    return CE_OK;
}

int ce_batch_run(ce_batch *b, uint32_t n_pairs, uint32_t metric_mask, uint32_t flags, float intensity_target,
                 ce_scores *out)
{
    if (int rc = ce_batch_launch(b, n_pairs, metric_mask, flags, intensity_target)) return rc;
    return ce_batch_collect(b, n_pairs, out);
}

// ---- single pair / mixed batch ----------------------------------------------------------------

// Device bytes a batch of this shape needs once the metrics in `mask` have run (working sets are allocated lazily,
// per metric).  Mirrors ce_ssim2_prepare / dssim_prepare / ba_prepare, with the plane padding folded into one factor.
// ref_planes: with SSIMULACRA2's final reference planes, which a batch allocates when it first builds them (ssim2.hip:
// ssim2_ref_blur_allocate).  The ABI's estimate always counts them; ce_eval_batch, whose pooled batches never build, does not.
static size_t estimate_batch_bytes(uint32_t w, uint32_t h, uint32_t n_refs, uint32_t n_pairs, uint32_t metric_mask, bool ref_planes)
{
    const double px = (double)w * h, slots = (double)n_refs + n_pairs, pairs = n_pairs;
    double bytes = 3.0 * px * slots + 64.0 * pairs;  // u8 slabs, scores
    double allocations = 8;                          // each device allocation is rounded up; budget 256 KiB of slack apiece
    if (metric_mask & CE_METRIC_SSIMULACRA2) {  // linear pyramid (levels >= 1) 4, XYB pyramid 16 per slot; 15 row-blurred planes x 1.333 per pair;
        // a reference's final mu1 / s11: 6 planes x 1.333 per reference
        bytes += px * (20.0 * slots + 80.0 * pairs + (ref_planes ? 32.0 * n_refs : 0.0));
        allocations += ref_planes ? 30 : 24;
    }
    if (metric_mask & CE_METRIC_DSSIM) {  // linear ping-pong 6 per slot; img 12 + the SSIM maps of all levels 5.4 per pair; the references' per-level img / mu / sq 48
        bytes += px * (6.0 * slots + 48.0 * n_refs + 17.4 * pairs);
        allocations += 24;
    }
    if (metric_mask & CE_METRIC_BUTTERAUGLI) {  // PsychoImage 50, mask input 5, three 3-plane scratch sets 36 per slot; mask values 10 per reference; half-resolution diffmap 1 per pair
        bytes += px * (91.0 * slots + 10.0 * n_refs + 1.0 * pairs);
        allocations += 20;
    }
    if (metric_mask & CE_METRIC_PSNR) bytes += 8.0 * pairs;
    return (size_t)(bytes * 1.2) + (size_t)(allocations * (256u << 10)) + (8u << 20);  // row / pitch padding of the planar buffers
}

size_t ce_estimate_batch_bytes(uint32_t w, uint32_t h, uint32_t n_refs, uint32_t n_pairs, uint32_t metric_mask)
{
    return estimate_batch_bytes(w, h, n_refs, n_pairs, metric_mask, true);
}

// the u16 slabs hold 6 bytes per pixel instead of 3, and the tables 4 * 2^depth bytes per side and rule; the working sets
// behind the front ends are the same
size_t ce_estimate_batch_bytes_deep(uint32_t w, uint32_t h, uint32_t n_refs, uint32_t n_pairs, uint32_t metric_mask, uint32_t ref_depth,
                                    uint32_t test_depth)
{
    if (!ce_deep_depth_ok(ref_depth) || !ce_deep_depth_ok(test_depth)) return 0;
    const size_t slabs = (size_t)3 * w * h * ((size_t)n_refs + n_pairs);
    return ce_estimate_batch_bytes(w, h, n_refs, n_pairs, metric_mask) + slabs + (((size_t)8 << ref_depth) + ((size_t)8 << test_depth));
}

// the f32 slabs hold 12 bytes per pixel instead of 3; the working sets behind the front ends are the same
size_t ce_estimate_batch_bytes_linear(uint32_t w, uint32_t h, uint32_t n_refs, uint32_t n_pairs, uint32_t metric_mask)
{
    return ce_estimate_batch_bytes(w, h, n_refs, n_pairs, metric_mask) + (size_t)9 * w * h * ((size_t)n_refs + n_pairs);
}

int ce_ctx_memory_info(ce_ctx *ctx, size_t *free_bytes, size_t *total_bytes)
{
    if (!ctx || !free_bytes || !total_bytes) return CE_ERR_INVALID_ARG;
    CE_HIP(ctx, hipSetDevice(ctx->device));
    CE_HIP(ctx, hipMemGetInfo(free_bytes, total_bytes));
    return CE_OK;
}

int ce_host_alloc(ce_ctx *ctx, size_t bytes, void **out)
{
    if (!ctx || !out || bytes == 0) return CE_ERR_INVALID_ARG;
    *out = nullptr;
    CE_HIP(ctx, hipSetDevice(ctx->device));
    CE_HIP(ctx, hipHostMalloc(out, bytes, hipHostMallocDefault));
    return CE_OK;
}

int ce_host_free(ce_ctx *ctx, void *p)
{
    if (!p) return CE_OK;
    const hipError_t e = hipHostFree(p);
    if (e != hipSuccess) {
        if (ctx) ctx->err = std::string("hipHostFree: ") + hipGetErrorString(e);
        return CE_ERR_BACKEND;
    }
    return CE_OK;
}

// bytes one ce_eval_batch chunk may allocate: CE_EVAL_BATCH_BYTES if set (tests), else a share of what is free now
static size_t chunk_budget(ce_ctx *ctx)
{
    if (const char *e = std::getenv("CE_EVAL_BATCH_BYTES")) {
        const long long v = std::atoll(e);
        if (v > 0) return (size_t)v;
    }
    size_t free_b = 0, total_b = 0;
    if (hipMemGetInfo(&free_b, &total_b) != hipSuccess) return (size_t)8 << 30;
    // the pooled batches of this context are reused, so what they hold already counts as available
    size_t pooled = 0;
    for (auto &kv : ctx->shape_pool) {
        const ce_batch *pb = kv.second;
        const uint32_t held = (pb->s2.engaged() ? CE_METRIC_SSIMULACRA2 : 0u) | (pb->ds.engaged() ? CE_METRIC_DSSIM : 0u) |
                              (pb->ba.engaged() ? CE_METRIC_BUTTERAUGLI : 0u);
        pooled += estimate_batch_bytes(pb->w, pb->h, pb->max_refs, pb->max_pairs, held, pb->s2.ref_blur[0] != nullptr);
    }
    // ... and no chunk asks for more than kChunkBytesMax: on a 288 GB device a third of the free memory is a 70+ GB batch whose
    // hipMalloc calls alone take seconds (measured: 2000 pairs of 512x512, three metrics - first call 3.7 s + 6.5 s for the
    // second with 73 GB chunks, 0.19 s with 48 GiB ones; steady state 128 ms vs 139 ms; profiles/r03_experiments.md §17)
    const size_t share = (size_t)((double)(free_b + pooled) * 0.8 / ce_ctx::kPoolRing);
    return std::min(share, ce_ctx::kChunkBytesMax);
}

// free every pooled batch that has nothing in flight (called when a new one does not fit)
static void pool_evict_idle(ce_ctx *ctx)
{
    for (auto it = ctx->shape_pool.begin(); it != ctx->shape_pool.end();) {
        if (!it->second->run_pending && !it->second->uploads_pending) {
            ce_batch_destroy(it->second);
            it = ctx->shape_pool.erase(it);
        } else {
            ++it;
        }
    }
}

static int shape_batch(ce_ctx *ctx, uint32_t w, uint32_t h, uint32_t need_pairs, uint32_t ring_slot, ce_batch **out)
{
    auto key = std::make_tuple(w, h, ring_slot);
    auto it = ctx->shape_pool.find(key);
    if (it != ctx->shape_pool.end() && it->second->max_pairs >= need_pairs) {
        *out = it->second;
        return CE_OK;
    }
    if (it != ctx->shape_pool.end()) {
        ce_batch_destroy(it->second);
        ctx->shape_pool.erase(it);
    }
    ce_batch *b = nullptr;
    int rc = ce_batch_create(ctx, w, h, need_pairs, need_pairs, &b);
    if (rc == CE_ERR_BACKEND) {  // out of device memory: drop the idle pooled batches of other shapes / sizes and retry once
        pool_evict_idle(ctx);
        rc = ce_batch_create(ctx, w, h, need_pairs, need_pairs, &b);
    }
    if (rc != CE_OK) return rc;
    ctx->shape_pool[key] = b;
    *out = b;
    return CE_OK;
}

int ce_eval_batch(ce_ctx *ctx, size_t n, const ce_pair_desc *pairs, uint32_t metric_mask, uint32_t flags,
                  float intensity_target, ce_scores *out)
{
    return ce_eval_batch_lut(ctx, n, pairs, nullptr, metric_mask, flags, intensity_target, out);
}

// Each bucket streams through up to kPoolRing pooled batches in the chunks of its plan (ce_plan.h); chunks are collected in
// launch order, or before their ring slot's batch is filled again.
int ce_eval_batch_lut(ce_ctx *ctx, size_t n, const ce_pair_desc *pairs, const ce_lut *const *test_luts, uint32_t metric_mask,
                      uint32_t flags, float intensity_target, ce_scores *out)
{
    if (!ctx || (!pairs && n) || (!out && n)) return CE_ERR_INVALID_ARG;
    // the maps live in the pooled batches, which the next call reuses: they are read from a ce_batch or a ce_ref
    if (flags & CE_FLAG_BUTTERAUGLI_DIFFMAP)
        return ce_fail(ctx, CE_ERR_INVALID_ARG, "CE_FLAG_BUTTERAUGLI_DIFFMAP needs a ce_batch or a ce_ref: the pooled batches keep no maps");
    if (flags & CE_FLAG_SSIMULACRA2_MAPS)
        return ce_fail(ctx, CE_ERR_INVALID_ARG, "CE_FLAG_SSIMULACRA2_MAPS needs a ce_batch or a ce_ref: the pooled batches keep no maps");
    // bucket by shape (Kodak mixes 768x512 and 512x768); invalid items never reach the device
    std::map<std::pair<uint32_t, uint32_t>, std::vector<size_t>> buckets;
    for (size_t i = 0; i < n; i++) {
        out[i] = ce_scores{};
        const ce_pair_desc &d = pairs[i];
        int rc = (!d.reference || !d.test || d.width == 0 || d.height == 0)
                     ? CE_ERR_INVALID_ARG
                     : ce_validate_pair(ctx, d.reference_len, d.test_len, d.width, d.height);
        if (rc != CE_OK) {
            out[i].status = rc;
            continue;
        }
        if (test_luts && test_luts[i] && test_luts[i]->ctx->device != ctx->device)
            return ce_fail(ctx, CE_ERR_INVALID_ARG, "colour table and batch are on different devices");
        buckets[{d.width, d.height}].push_back(i);
    }
    if (buckets.empty()) return CE_OK;
    // what ce_batch_launch would reject is rejected before anything is uploaded
    if (metric_mask & ~ce_known_metrics) return ce_fail(ctx, CE_ERR_INVALID_ARG, "unknown metric bit");
    static const size_t forced_chunks = [] {  // CE_EVAL_BATCH_CHUNKS (1..3) forces the chunk count for A/B runs
        const char *e = std::getenv("CE_EVAL_BATCH_CHUNKS");
        const int v = e ? std::atoi(e) : 0;
        return (size_t)(v >= 1 && v <= (int)ce_ctx::kPoolRing ? v : 0);
    }();
    static const size_t ramp0 = [] {  // CE_EVAL_BATCH_RAMP: pairs of the call's first chunk (0 = every chunk at the target)
        const char *e = std::getenv("CE_EVAL_BATCH_RAMP");
        return (size_t)(e ? std::max(0, std::atoi(e)) : 64);  // 2000 pairs of 512x512: off 106.5 ms, 32 -> 102.1, 64 -> 100.0, 128 -> 101.1
    }();
    std::vector<ce_plan_chunk> plan;
    struct launched { ce_batch *b = nullptr; std::vector<size_t> items; };
    std::vector<launched> running;  // per chunk, while launched and not collected: its batch and items in pair order
    ce_batch *filling = nullptr;    // the batch of the chunk begun last
    int rc = CE_OK;
    auto collect = [&](size_t c) -> int {  // waits for the chunk's ev_run; its scores reach out[] only while the call succeeds
        const launched l = std::exchange(running[c], launched{});
        std::vector<ce_scores> tmp(l.items.size());
        const int r = ce_batch_collect(l.b, (uint32_t)tmp.size(), tmp.data());
        for (size_t k = 0; k < tmp.size() && r == CE_OK && rc == CE_OK; k++) out[l.items[k]] = tmp[k];
        return r;
    };
    auto run_chunk = [&](uint32_t w, uint32_t h, size_t c) -> int {
        const ce_plan_chunk &p = plan[c];
        if (p.collect_first != ce_plan_none)  // the ring slot's batch still runs an earlier chunk of this call
            if (int r = collect(p.collect_first)) return r;
        ce_batch *b = nullptr;
        if (int r = shape_batch(ctx, w, h, p.max_pairs, p.slot, &b)) return r;
        filling = b;
        std::vector<ce_upload_job> jobs;
        std::vector<size_t> items;
        for (uint32_t s = 0; s < p.refs.size(); s++) {
            jobs.push_back({b->d_refs + (size_t)s * b->img_bytes, pairs[p.refs[s][0]].reference});
            for (size_t i : p.refs[s]) {
                if (int r = ce_batch_bind_pair(b, (uint32_t)items.size(), s)) return r;
                jobs.push_back({b->d_tests + items.size() * b->img_bytes, pairs[i].test});
                items.push_back(i);
            }
        }
        ce_invalidate_reference_state(b);
        if (int r = ce_upload_many(b, jobs)) return r;
        if (test_luts)  // ICC -> sRGB of the decoded images, on the upload stream behind their copies (icc.rs:69-103)
            for (size_t k = 0; k < items.size(); k++)
                if (int r = ce_apply_lut(b, b->d_tests + k * b->img_bytes, test_luts[items[k]])) return r;
        if (int r = ce_batch_launch(b, (uint32_t)items.size(), metric_mask, flags, intensity_target)) return r;
        running[c] = {b, std::move(items)};
        return CE_OK;
    };
    uint32_t ring = 0;
    for (auto it = buckets.begin(); it != buckets.end() && rc == CE_OK; ++it) {
        const uint32_t w = it->first.first, h = it->first.second;
        std::vector<const void *> refs;
        for (size_t i : it->second) refs.push_back(pairs[i].reference);
        // without SSIMULACRA2's final reference planes: a pooled batch's references are written before every launch, so it never builds them
        const size_t per_pair = estimate_batch_bytes(w, h, 1, 2, metric_mask, false) - estimate_batch_bytes(w, h, 1, 1, metric_mask, false) +
                                estimate_batch_bytes(w, h, 2, 1, metric_mask, false) - estimate_batch_bytes(w, h, 1, 1, metric_mask, false);  // a pair with a reference of its own
        auto pooled = ctx->shape_pool.find(std::make_tuple(w, h, 0u));
        const ce_plan_inputs in{chunk_budget(ctx), per_pair, pooled != ctx->shape_pool.end() ? pooled->second->max_pairs : 0u, forced_chunks, ramp0,
                                 ce_launch_slots_max};
        const size_t first = plan.size();
        ce_plan_bucket(it->second, refs, in, ring, plan);
        running.resize(plan.size());
        for (size_t c = first; c < plan.size() && rc == CE_OK; c++) rc = run_chunk(w, h, c);
    }
    // the one exit: every launched chunk is waited for (its batch leaves the in-flight count), and a failed call drains the
    // batch it was filling before the caller's buffers can go away
    for (size_t c = 0; c < plan.size(); c++)
        if (running[c].b) {
            const int r = collect(c);
            if (rc == CE_OK) rc = r;
        }
    if (rc != CE_OK && filling) ce_drain_batch(filling);
    return rc;
}

// ---- image heuristics (heuristics.hip) ---------------------------------------------------------

int ce_batch_image_heuristics(ce_batch *b, uint32_t which, uint32_t first, uint32_t count, ce_image_heuristics *out)
{
    if (!b || !out) return CE_ERR_INVALID_ARG;
    ce_ctx *ctx = b->ctx;
    if (b->depth[0]) return ce_fail(ctx, CE_ERR_INVALID_ARG, "image heuristics are defined on u8 gray levels: not for a deep batch");
    if (b->linear) return ce_fail(ctx, CE_ERR_INVALID_ARG, "image heuristics are defined on u8 gray levels: not for a linear batch");
    if (which != CE_BATCH_REFERENCES && which != CE_BATCH_TESTS)
        return ce_fail(ctx, CE_ERR_INVALID_ARG, "image heuristics: unknown slab " + std::to_string(which));
    const uint32_t slots = which == CE_BATCH_TESTS ? b->max_pairs : b->max_refs;
    if (count == 0 || first > slots || count > slots - first)
        return ce_fail(ctx, CE_ERR_INVALID_ARG, "image heuristics: images [" + std::to_string(first) + ", " +
                                                 std::to_string((uint64_t)first + count) + ") outside the " + std::to_string(slots) +
                                                 " slots");
    if (b->w < 3 || b->h < 3)
        return ce_fail(ctx, CE_ERR_TOO_SMALL, "image heuristics need at least 3 x 3 pixels, got " + std::to_string(b->w) + " x " +
                                               std::to_string(b->h));
    CE_HIP(ctx, hipSetDevice(ctx->device));
    // the kernels run on the context's stream: behind the inline route's copies already, behind the upload stream's
    // copies, conversions and colour tables from here (the ordering of a launch, ce_order_write)
    if (int rc = ce_flush_uploads(b)) return rc;
    const uint8_t *slab = which == CE_BATCH_TESTS ? b->d_tests : b->d_refs;
    return ce_image_heuristics_run(ctx, slab + (size_t)first * b->img_bytes, b->img_bytes, b->w, b->h, count, out);
}

// ---- HDR fidelity of linear batches: PQ-PSNR and BT.2124 Delta E ITP (hdr_fidelity.hip) ----------

int ce_pq_code_thresholds(uint32_t depth, float white_nits, float *out, size_t n)
{
    if (!out || !hdr_depth_ok(depth) || n != ((size_t)1 << depth) - 1)
        return ce_fail(nullptr, CE_ERR_INVALID_ARG, "ce_pq_code_thresholds: depth 10, 12 or 16 and n = 2^depth - 1");
    if (!ce_build_pq_code_thresholds((1u << depth) - 1u, (double)white_nits, out))
        return ce_fail(nullptr, CE_ERR_INVALID_ARG, "ce_pq_code_thresholds: white_nits must be finite and > 0");
    return CE_OK;
}

int ce_hdr_fidelity_matrices(float a[9], float b[9])
{
    if (!a || !b) return ce_fail(nullptr, CE_ERR_INVALID_ARG, "ce_hdr_fidelity_matrices: null pointer");
    ce_build_hdr_fidelity_matrices(a, b);
    return CE_OK;
}

// the thresholds of (depth, white_nits) on the device, built once per context and kept: [table, padded to 16 floats | at
// depth 16 every 16th threshold]; *coarse is the level the kernel stages in LDS
static int hdr_table_dev(ce_ctx *ctx, uint32_t depth, float white_nits, const float **table, const float **coarse)
{
    uint32_t white_bits;
    std::memcpy(&white_bits, &white_nits, 4);
    const size_t n = ((size_t)1 << depth) - 1, padded = (n + 15) & ~(size_t)15, n_coarse = depth > 12 ? ((size_t)1 << 12) - 1 : 0;
    const auto key = std::make_pair(depth, white_bits);
    auto it = ctx->hdr_tables.find(key);
    if (it == ctx->hdr_tables.end()) {
        std::vector<float> host(padded + n_coarse, INFINITY);
        ce_build_pq_code_thresholds((uint32_t)n, (double)white_nits, host.data());
        const size_t stride = (size_t)1 << (depth > 12 ? depth - 12 : 0);
        for (size_t j = 0; j < n_coarse; j++) host[padded + j] = host[(j + 1) * stride - 1];
        void *d = nullptr;
        if (int rc = ce_device_table(ctx, host.data(), host.size() * sizeof(float), "PQ code thresholds", &d)) return rc;
        it = ctx->hdr_tables.emplace(key, static_cast<float *>(d)).first;
    }
    *table = it->second;
    *coarse = n_coarse ? it->second + padded : it->second;
    return CE_OK;
}

int ce_batch_hdr_fidelity(ce_batch *b, uint32_t n_pairs, uint32_t depth, float white_nits, ce_hdr_scores *out)
{
    if (!b) return CE_ERR_INVALID_ARG;
    ce_ctx *ctx = b->ctx;
    if (!out) return ce_fail(ctx, CE_ERR_INVALID_ARG, "HDR fidelity: null pointer");
    if (!b->linear)
        return ce_fail(ctx, CE_ERR_INVALID_ARG, "HDR fidelity reads linear light: it needs a linear batch (ce_batch_create_linear)");
    if (int rc = ce_hdr_params_check(ctx, depth, white_nits)) return rc;
    if (n_pairs == 0 || n_pairs > b->max_pairs) return ce_fail(ctx, CE_ERR_INVALID_ARG, "n_pairs out of range");
    CE_HIP(ctx, hipSetDevice(ctx->device));
    const float *d_table = nullptr, *d_coarse = nullptr;
    if (int rc = hdr_table_dev(ctx, depth, white_nits, &d_table, &d_coarse)) return rc;
    if (!b->hdr)
        if (int rc = b->hdr.alloc(ctx, (size_t)3 * b->max_pairs)) return rc;
    // on the context's stream, as a launch: behind the uploads queued so far, with the pair table of the last bind
    if (int rc = ce_flush_uploads(b)) return rc;
    if (int rc = sync_pair_ref(b)) return rc;
    float a[9], lms[9];
    ce_build_hdr_fidelity_matrices(a, lms);
    if (int rc = ce_launch_hdr_fidelity(b, n_pairs, depth, d_table, d_coarse, a, lms, b->hdr.d)) return rc;
    CE_HIP(ctx, hipMemcpyAsync(b->hdr.h, b->hdr.d, sizeof(unsigned long long) * 3 * n_pairs, hipMemcpyDeviceToHost, ctx->stream));
    CE_HIP(ctx, hipStreamSynchronize(ctx->stream));  // the slabs are free again: a later upload needs no fence against this
    const double maxv = (double)((1u << depth) - 1u), n_px = (double)((size_t)b->w * b->h);
    for (uint32_t i = 0; i < n_pairs; i++) {
        ce_hdr_scores s{};
        s.pq_sse = b->hdr.h[3 * i], s.itp_sum_q20 = b->hdr.h[3 * i + 1], s.itp_max_q20 = b->hdr.h[3 * i + 2];
        s.pq_psnr = psnr_from_sse(s.pq_sse, b->w, b->h, maxv);
        s.delta_e_itp_mean = (double)s.itp_sum_q20 / 1048576.0 / n_px;
        s.delta_e_itp_max = (double)s.itp_max_q20 / 1048576.0;
        out[i] = s;
    }
    return CE_OK;
}

// Delta E ITP per pixel, per cell and over thresholds (include/ce_metrics.h): ce_batch_hdr_fidelity's
// frame around the map kernel
int ce_batch_delta_e_itp_map(ce_batch *b, uint32_t first, uint32_t count, uint32_t depth, float white_nits, uint32_t block, uint32_t *map,
                             size_t map_len, const uint32_t *thresholds_q20, uint32_t n_thresholds, uint64_t *over)
{
    if (!b) return ce_fail(nullptr, CE_ERR_INVALID_ARG, "Delta E ITP map: null batch");
    ce_ctx *ctx = b->ctx;
    if (!b->linear)
        return ce_fail(ctx, CE_ERR_INVALID_ARG, "the Delta E ITP map reads linear light: it needs a linear batch (ce_batch_create_linear)");
    if (int rc = ce_hdr_params_check(ctx, depth, white_nits)) return rc;
    if (!map && !over) return ce_fail(ctx, CE_ERR_INVALID_ARG, "Delta E ITP map: neither a map nor counts asked for");
    if (count == 0 || first > b->max_pairs || count > b->max_pairs - first)
        return ce_fail(ctx, CE_ERR_INVALID_ARG, "Delta E ITP map: pairs [" + std::to_string(first) + ", " + std::to_string((uint64_t)first + count) +
                                                 ") outside the batch's " + std::to_string(b->max_pairs));
    if (int rc = check_map_readout(ctx, "Delta E ITP map", b->max_pairs, first, count, block, b->w, b->h, map != nullptr, map_len)) return rc;
    if (n_thresholds > CE_DELTA_E_ITP_MAX_THRESHOLDS)
        return ce_fail(ctx, CE_ERR_INVALID_ARG, "Delta E ITP map: at most " + std::to_string(CE_DELTA_E_ITP_MAX_THRESHOLDS) + " thresholds, got " +
                                                 std::to_string(n_thresholds));
    if (over && (n_thresholds == 0 || !thresholds_q20)) return ce_fail(ctx, CE_ERR_INVALID_ARG, "Delta E ITP map: counts asked for without thresholds");
    if (!over && (n_thresholds != 0 || thresholds_q20)) return ce_fail(ctx, CE_ERR_INVALID_ARG, "Delta E ITP map: thresholds given without a place for the counts");
    CE_HIP(ctx, hipSetDevice(ctx->device));
    const float *d_table = nullptr, *d_coarse = nullptr;
    if (int rc = hdr_table_dev(ctx, depth, white_nits, &d_table, &d_coarse)) return rc;
    if (map)
        if (int rc = b->d_itp_map.reserve(ctx, map_len)) return rc;
    const size_t over_bytes = sizeof(unsigned long long) * CE_DELTA_E_ITP_MAX_THRESHOLDS;  // per pair
    if (over && !b->itp_over)
        if (int rc = b->itp_over.alloc(ctx, (size_t)CE_DELTA_E_ITP_MAX_THRESHOLDS * b->max_pairs)) return rc;
    // on the context's stream, as a launch: behind the uploads queued so far, with the pair table of the last bind
    if (int rc = ce_flush_uploads(b)) return rc;
    if (int rc = sync_pair_ref(b)) return rc;
    float a[9], lms[9];
    ce_build_hdr_fidelity_matrices(a, lms);
    if (int rc = ce_launch_delta_e_itp_map(b, first, count, depth, d_table, d_coarse, a, lms, block, map ? b->d_itp_map.get() : nullptr, thresholds_q20,
                                           n_thresholds, over ? b->itp_over.d.get() : nullptr))
        return rc;
    if (map) CE_HIP(ctx, hipMemcpyAsync(map, b->d_itp_map, map_len * sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
    if (over) CE_HIP(ctx, hipMemcpyAsync(b->itp_over.h, b->itp_over.d, over_bytes * count, hipMemcpyDeviceToHost, ctx->stream));
    CE_HIP(ctx, hipStreamSynchronize(ctx->stream));  // the slabs are free again: a later upload needs no fence against this
    for (uint32_t i = 0; over && i < count; i++)
        for (uint32_t j = 0; j < n_thresholds; j++) over[(size_t)i * n_thresholds + j] = b->itp_over.h[(size_t)i * CE_DELTA_E_ITP_MAX_THRESHOLDS + j];
    return CE_OK;
}

// ---- SSIM and MS-SSIM of RGB8 and deep batches (msssim.hip) -------------------------------------------

// (ce_msssim_window is in msssim.hip, beside the literals the kernel filters with)

// the levels' geometry, or why there is none (the reason goes to ctx, or to the calling thread without one)
static int msssim_levels(ce_ctx *ctx, uint32_t w, uint32_t h, uint32_t levels, uint32_t *lw, uint32_t *lh)
{
    if (levels != 1 && levels != CE_MSSSIM_LEVELS)
        return ce_fail(ctx, CE_ERR_INVALID_ARG, "MS-SSIM: levels must be 1 (SSIM) or 5 (MS-SSIM), got " + std::to_string(levels));
    const uint32_t m = std::min(w, h);
    if (levels == 1 ? m < 11 : m <= 160)
        return ce_fail(ctx, CE_ERR_INVALID_ARG, std::string("MS-SSIM: ") + (levels == 1 ? "one level needs min(w, h) >= 11" : "five levels need min(w, h) > 160") +
                                                 ", got " + std::to_string(w) + " x " + std::to_string(h));
    for (uint32_t l = 0; l < levels; l++) {
        lw[l] = w, lh[l] = h;
        w = (w + (w & 1u)) / 2, h = (h + (h & 1u)) / 2;
    }
    return CE_OK;
}

int ce_msssim_levels(uint32_t w, uint32_t h, uint32_t levels, uint32_t *n_levels, uint32_t *level_w, uint32_t *level_h)
{
    if (!n_levels || !level_w || !level_h) return ce_fail(nullptr, CE_ERR_INVALID_ARG, "ce_msssim_levels: null pointer");
    if (int rc = msssim_levels(nullptr, w, h, levels, level_w, level_h)) return rc;
    *n_levels = levels;
    return CE_OK;
}

int ce_batch_msssim(ce_batch *b, uint32_t n_pairs, uint32_t levels, ce_msssim_scores *out)
{
    if (!b) return CE_ERR_INVALID_ARG;
    ce_ctx *ctx = b->ctx;
    if (!out) return ce_fail(ctx, CE_ERR_INVALID_ARG, "MS-SSIM: null pointer");
    if (b->linear) return ce_fail(ctx, CE_ERR_INVALID_ARG, "MS-SSIM reads encoded sample values: not for a linear batch");
    if (b->depth[0] != b->depth[1])
        return ce_fail(ctx, CE_ERR_INVALID_ARG, "MS-SSIM needs both sides at one depth, got " + std::to_string(b->depth[0]) + " / " +
                                                 std::to_string(b->depth[1]));
    uint32_t lw[CE_MSSSIM_LEVELS] = {}, lh[CE_MSSSIM_LEVELS] = {};
    if (int rc = msssim_levels(ctx, b->w, b->h, levels, lw, lh)) return rc;
    if (n_pairs == 0 || n_pairs > b->max_pairs) return ce_fail(ctx, CE_ERR_INVALID_ARG, "n_pairs out of range");
    CE_HIP(ctx, hipSetDevice(ctx->device));
    constexpr size_t per_pair = (size_t)CE_MSSSIM_LEVELS * 3 * 2;
    if (!b->msssim)
        if (int rc = b->msssim.alloc(ctx, per_pair * b->max_pairs)) return rc;
    size_t pyr = 0;
    for (uint32_t l = 1; l < levels; l++) pyr += ((size_t)b->max_refs + b->max_pairs) * 3 * lw[l] * lh[l];
    if (int rc = b->d_msssim_pyr.reserve(ctx, pyr)) return rc;
    // on the context's stream, as a launch: behind the uploads queued so far, with the pair table of the last bind
    if (int rc = ce_flush_uploads(b)) return rc;
    if (int rc = sync_pair_ref(b)) return rc;
    if (int rc = ce_launch_msssim(b, n_pairs, levels, lw, lh, b->d_msssim_pyr, b->msssim.d)) return rc;
    CE_HIP(ctx, hipMemcpyAsync(b->msssim.h, b->msssim.d, sizeof(unsigned long long) * per_pair * n_pairs, hipMemcpyDeviceToHost, ctx->stream));
    CE_HIP(ctx, hipStreamSynchronize(ctx->stream));  // the slabs are free again: a later upload needs no fence against this
    static const double wt[CE_MSSSIM_LEVELS] = {0.0448, 0.2856, 0.3001, 0.2363, 0.1333};
    for (uint32_t i = 0; i < n_pairs; i++) {
        ce_msssim_scores s{};
        s.n_levels = levels;
        double ms[CE_MSSSIM_LEVELS][3], mc[CE_MSSSIM_LEVELS][3];
        for (uint32_t l = 0; l < levels; l++) {
            s.n[l] = (uint64_t)(lw[l] - 10) * (lh[l] - 10);
            for (int c = 0; c < 3; c++) {
                const unsigned long long *q = b->msssim.h + (((size_t)i * CE_MSSSIM_LEVELS + l) * 3 + c) * 2;
                s.ssim_q[l][c] = (int64_t)q[0], s.cs_q[l][c] = (int64_t)q[1];
                ms[l][c] = ((double)s.ssim_q[l][c] / 4294967296.0) / (double)s.n[l];
                mc[l][c] = ((double)s.cs_q[l][c] / 4294967296.0) / (double)s.n[l];
            }
        }
        for (int c = 0; c < 3; c++) {
            s.ssim_rgb[c] = ms[0][c];
            s.ms_ssim_rgb[c] = NAN;
            if (levels == CE_MSSSIM_LEVELS) {
                double p = std::pow(std::max(mc[0][c], 0.0), wt[0]);
                for (int l = 1; l < 4; l++) p = p * std::pow(std::max(mc[l][c], 0.0), wt[l]);
                s.ms_ssim_rgb[c] = p * std::pow(std::max(ms[4][c], 0.0), wt[4]);
            }
        }
        s.ssim = ((s.ssim_rgb[0] + s.ssim_rgb[1]) + s.ssim_rgb[2]) / 3.0;
        s.ms_ssim = levels == CE_MSSSIM_LEVELS ? ((s.ms_ssim_rgb[0] + s.ms_ssim_rgb[1]) + s.ms_ssim_rgb[2]) / 3.0 : NAN;
        out[i] = s;
    }
    return CE_OK;
}

// SSIM / MS-SSIM per position, per cell and over thresholds (include/ce_metrics.h): ce_batch_msssim's frame
// around the map kernel, ce_batch_delta_e_itp_map's rules for the outputs
int ce_batch_msssim_map(ce_batch *b, uint32_t first, uint32_t count, uint32_t levels, uint32_t level, uint32_t what, uint32_t block,
                        uint32_t *map, size_t map_len, const uint32_t *thresholds_q32, uint32_t n_thresholds, uint64_t *over)
{
    if (!b) return ce_fail(nullptr, CE_ERR_INVALID_ARG, "MS-SSIM map: null batch");
    ce_ctx *ctx = b->ctx;
    if (b->linear) return ce_fail(ctx, CE_ERR_INVALID_ARG, "the MS-SSIM map reads encoded sample values: not for a linear batch");
    if (b->depth[0] != b->depth[1])
        return ce_fail(ctx, CE_ERR_INVALID_ARG, "the MS-SSIM map needs both sides at one depth, got " + std::to_string(b->depth[0]) + " / " +
                                                 std::to_string(b->depth[1]));
    uint32_t lw[CE_MSSSIM_LEVELS] = {}, lh[CE_MSSSIM_LEVELS] = {};
    if (int rc = msssim_levels(ctx, b->w, b->h, levels, lw, lh)) return rc;
    if (level >= levels)
        return ce_fail(ctx, CE_ERR_INVALID_ARG, "MS-SSIM map: level " + std::to_string(level) + " of " + std::to_string(levels));
    if (what > CE_MSSSIM_MAP_CS)
        return ce_fail(ctx, CE_ERR_INVALID_ARG, "MS-SSIM map: what must be CE_MSSSIM_MAP_SSIM or CE_MSSSIM_MAP_CS, got " + std::to_string(what));
    if (!map && !over) return ce_fail(ctx, CE_ERR_INVALID_ARG, "MS-SSIM map: neither a map nor counts asked for");
    if (count == 0 || first > b->max_pairs || count > b->max_pairs - first)
        return ce_fail(ctx, CE_ERR_INVALID_ARG, "MS-SSIM map: pairs [" + std::to_string(first) + ", " + std::to_string((uint64_t)first + count) +
                                                 ") outside the batch's " + std::to_string(b->max_pairs));
    if (block == 0 || block > 64 || (block & (block - 1)) != 0)
        return ce_fail(ctx, CE_ERR_INVALID_ARG, "MS-SSIM map: block must be 1 or a power of two up to 64");
    const uint32_t vw = lw[level] - 10, vh = lh[level] - 10;
    const size_t want = map ? (size_t)count * 3 * ((vw + block - 1) / block) * ((vh + block - 1) / block) : 0;
    if (map_len != want)
        return ce_fail(ctx, CE_ERR_INVALID_ARG, "MS-SSIM map: the map needs " + std::to_string(want) + " elements, got " + std::to_string(map_len));
    if (n_thresholds > CE_MSSSIM_MAP_MAX_THRESHOLDS)
        return ce_fail(ctx, CE_ERR_INVALID_ARG, "MS-SSIM map: at most " + std::to_string(CE_MSSSIM_MAP_MAX_THRESHOLDS) + " thresholds, got " +
                                                 std::to_string(n_thresholds));
    if (over && (n_thresholds == 0 || !thresholds_q32)) return ce_fail(ctx, CE_ERR_INVALID_ARG, "MS-SSIM map: counts asked for without thresholds");
    if (!over && (n_thresholds != 0 || thresholds_q32)) return ce_fail(ctx, CE_ERR_INVALID_ARG, "MS-SSIM map: thresholds given without a place for the counts");
    CE_HIP(ctx, hipSetDevice(ctx->device));
    if (map)
        if (int rc = b->d_msssim_map.reserve(ctx, map_len)) return rc;
    constexpr size_t per_pair = (size_t)3 * CE_MSSSIM_MAP_MAX_THRESHOLDS;
    if (over && !b->msssim_over)
        if (int rc = b->msssim_over.alloc(ctx, per_pair * b->max_pairs)) return rc;
    // the pyramid whole, as ce_batch_msssim makes it: the two calls share it, and its layout does not depend on the level asked for
    size_t pyr = 0;
    for (uint32_t l = 1; l < levels; l++) pyr += ((size_t)b->max_refs + b->max_pairs) * 3 * lw[l] * lh[l];
    if (level)
        if (int rc = b->d_msssim_pyr.reserve(ctx, pyr)) return rc;
    // on the context's stream, as a launch: behind the uploads queued so far, with the pair table of the last bind
    if (int rc = ce_flush_uploads(b)) return rc;
    if (int rc = sync_pair_ref(b)) return rc;
    if (int rc = ce_launch_msssim_map(b, first, count, level, lw, lh, b->d_msssim_pyr, what, block, map ? b->d_msssim_map.get() : nullptr,
                                      thresholds_q32, n_thresholds, over ? b->msssim_over.d.get() : nullptr))
        return rc;
    if (map) CE_HIP(ctx, hipMemcpyAsync(map, b->d_msssim_map, map_len * sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
    if (over)
        CE_HIP(ctx, hipMemcpyAsync(b->msssim_over.h, b->msssim_over.d, sizeof(unsigned long long) * per_pair * count, hipMemcpyDeviceToHost, ctx->stream));
    CE_HIP(ctx, hipStreamSynchronize(ctx->stream));  // the slabs are free again: a later upload needs no fence against this
    for (size_t i = 0; over && i < (size_t)count * 3; i++)
        for (uint32_t j = 0; j < n_thresholds; j++) over[i * n_thresholds + j] = b->msssim_over.h[i * CE_MSSSIM_MAP_MAX_THRESHOLDS + j];
    return CE_OK;
}

// ---- CIEDE2000 of RGB8 and deep batches (ciede2000.hip) ------------------------------------------------

int ce_batch_ciede2000(ce_batch *b, uint32_t n_pairs, const uint32_t *thresholds_q20, uint32_t n_thresholds, ce_ciede2000_scores *out)
{
    if (!b) return CE_ERR_INVALID_ARG;
    ce_ctx *ctx = b->ctx;
    if (!out || (n_thresholds && !thresholds_q20)) return ce_fail(ctx, CE_ERR_INVALID_ARG, "CIEDE2000: null pointer");
    if (b->linear)
        return ce_fail(ctx, CE_ERR_INVALID_ARG, "CIEDE2000 reads sRGB sample values: not for a linear batch, whose colour difference is Delta E ITP "
                                                "(ce_batch_hdr_fidelity)");
    if (n_thresholds > CE_CIEDE2000_MAX_THRESHOLDS)
        return ce_fail(ctx, CE_ERR_INVALID_ARG, "CIEDE2000: at most " + std::to_string(CE_CIEDE2000_MAX_THRESHOLDS) + " thresholds, got " +
                                                 std::to_string(n_thresholds));
    if (n_pairs == 0 || n_pairs > b->max_pairs) return ce_fail(ctx, CE_ERR_INVALID_ARG, "n_pairs out of range");
    CE_HIP(ctx, hipSetDevice(ctx->device));
    // the tables SSIMULACRA2 reads a deep batch through, per side; an RGB8 batch through the 8-bit one
    const float *d_tab[2] = {nullptr, nullptr};
    for (int s = 0; s < 2; s++)
        if (int rc = ce_deep_table(ctx, b->depth[s] ? b->depth[s] : 8, 0, &d_tab[s])) return rc;
    constexpr size_t per_pair = 2 + CE_CIEDE2000_MAX_THRESHOLDS;
    if (!b->ciede2000)
        if (int rc = b->ciede2000.alloc(ctx, per_pair * b->max_pairs)) return rc;
    // on the context's stream, as a launch: behind the uploads queued so far, with the pair table of the last bind
    if (int rc = ce_flush_uploads(b)) return rc;
    if (int rc = sync_pair_ref(b)) return rc;
    if (int rc = ce_launch_ciede2000(b, n_pairs, d_tab[0], d_tab[1], thresholds_q20, n_thresholds, b->ciede2000.d)) return rc;
    CE_HIP(ctx, hipMemcpyAsync(b->ciede2000.h, b->ciede2000.d, sizeof(unsigned long long) * per_pair * n_pairs, hipMemcpyDeviceToHost, ctx->stream));
    CE_HIP(ctx, hipStreamSynchronize(ctx->stream));  // the slabs are free again: a later upload needs no fence against this
    for (uint32_t i = 0; i < n_pairs; i++) {
        const unsigned long long *v = b->ciede2000.h + per_pair * i;
        ce_ciede2000_scores s{};
        s.sum_q20 = v[0], s.max_q20 = (uint32_t)v[1], s.n = (uint64_t)b->w * b->h, s.n_thresholds = n_thresholds;
        for (uint32_t j = 0; j < n_thresholds; j++) s.n_above[j] = v[2 + j];
        s.mean = ((double)s.sum_q20 / 1048576.0) / (double)s.n;
        s.max = (double)s.max_q20 / 1048576.0;
        s.ciede2000_db = s.sum_q20 ? 45.0 - 20.0 * std::log10(s.mean) : INFINITY;
        out[i] = s;
    }
    return CE_OK;
}

int ce_ciede2000_pixels(const uint16_t *ref_rgb, uint32_t ref_depth, const uint16_t *test_rgb, uint32_t test_depth, size_t n, uint32_t *out_q20)
{
    if (!ce_deep_depth_ok(ref_depth) || !ce_deep_depth_ok(test_depth))
        return ce_fail(nullptr, CE_ERR_INVALID_ARG, "ce_ciede2000_pixels: depths must be 8, 10, 12 or 16 bits, got " + std::to_string(ref_depth) +
                                                     " / " + std::to_string(test_depth));
    if (!ref_rgb || !test_rgb || !out_q20) return ce_fail(nullptr, CE_ERR_INVALID_ARG, "ce_ciede2000_pixels: null pointer");
    const uint32_t maxv[2] = {(1u << ref_depth) - 1u, (1u << test_depth) - 1u};
    std::vector<float> tab[2];
    for (int s = 0; s < (ref_depth == test_depth ? 1 : 2); s++) {
        tab[s].resize((size_t)maxv[s] + 1);
        ce_build_srgb_table_f64(tab[s].data(), maxv[s]);
    }
    ce_ciede2000_pixels_host(ref_rgb, tab[0].data(), maxv[0], test_rgb, tab[ref_depth == test_depth ? 0 : 1].data(), maxv[1], n, out_q20);
    return CE_OK;
}

// CIEDE2000 per pixel, per cell and over thresholds, for q or one of its terms (include/ce_metrics.h):
// ce_batch_ciede2000's frame around the map kernel, ce_batch_delta_e_itp_map's rules for the outputs
int ce_batch_ciede2000_map(ce_batch *b, uint32_t first, uint32_t count, uint32_t what, uint32_t block, uint32_t *map, size_t map_len,
                           const uint32_t *thresholds_q20, uint32_t n_thresholds, uint64_t *over)
{
    if (!b) return ce_fail(nullptr, CE_ERR_INVALID_ARG, "CIEDE2000 map: null batch");
    ce_ctx *ctx = b->ctx;
    if (b->linear)
        return ce_fail(ctx, CE_ERR_INVALID_ARG, "the CIEDE2000 map reads sRGB sample values: not for a linear batch, whose map is Delta E ITP's "
                                                "(ce_batch_delta_e_itp_map)");
    if (what > CE_CIEDE2000_MAP_DH)
        return ce_fail(ctx, CE_ERR_INVALID_ARG, "CIEDE2000 map: what must be CE_CIEDE2000_MAP_DE, _DL, _DC or _DH, got " + std::to_string(what));
    if (!map && !over) return ce_fail(ctx, CE_ERR_INVALID_ARG, "CIEDE2000 map: neither a map nor counts asked for");
    if (count == 0 || first > b->max_pairs || count > b->max_pairs - first)
        return ce_fail(ctx, CE_ERR_INVALID_ARG, "CIEDE2000 map: pairs [" + std::to_string(first) + ", " + std::to_string((uint64_t)first + count) +
                                                 ") outside the batch's " + std::to_string(b->max_pairs));
    if (int rc = check_map_readout(ctx, "CIEDE2000 map", b->max_pairs, first, count, block, b->w, b->h, map != nullptr, map_len)) return rc;
    if (n_thresholds > CE_CIEDE2000_MAX_THRESHOLDS)
        return ce_fail(ctx, CE_ERR_INVALID_ARG, "CIEDE2000 map: at most " + std::to_string(CE_CIEDE2000_MAX_THRESHOLDS) + " thresholds, got " +
                                                 std::to_string(n_thresholds));
    if (over && (n_thresholds == 0 || !thresholds_q20)) return ce_fail(ctx, CE_ERR_INVALID_ARG, "CIEDE2000 map: counts asked for without thresholds");
    if (!over && (n_thresholds != 0 || thresholds_q20)) return ce_fail(ctx, CE_ERR_INVALID_ARG, "CIEDE2000 map: thresholds given without a place for the counts");
    CE_HIP(ctx, hipSetDevice(ctx->device));
    const float *d_tab[2] = {nullptr, nullptr};
    for (int s = 0; s < 2; s++)
        if (int rc = ce_deep_table(ctx, b->depth[s] ? b->depth[s] : 8, 0, &d_tab[s])) return rc;
    if (map)
        if (int rc = b->d_ciede2000_map.reserve(ctx, map_len)) return rc;
    const size_t over_bytes = sizeof(unsigned long long) * CE_CIEDE2000_MAX_THRESHOLDS;  // per pair
    if (over && !b->ciede2000_over)
        if (int rc = b->ciede2000_over.alloc(ctx, (size_t)CE_CIEDE2000_MAX_THRESHOLDS * b->max_pairs)) return rc;
    // on the context's stream, as a launch: behind the uploads queued so far, with the pair table of the last bind
    if (int rc = ce_flush_uploads(b)) return rc;
    if (int rc = sync_pair_ref(b)) return rc;
    if (int rc = ce_launch_ciede2000_map(b, first, count, what, d_tab[0], d_tab[1], block, map ? b->d_ciede2000_map.get() : nullptr, thresholds_q20,
                                         n_thresholds, over ? b->ciede2000_over.d.get() : nullptr))
        return rc;
    if (map) CE_HIP(ctx, hipMemcpyAsync(map, b->d_ciede2000_map, map_len * sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
    if (over) CE_HIP(ctx, hipMemcpyAsync(b->ciede2000_over.h, b->ciede2000_over.d, over_bytes * count, hipMemcpyDeviceToHost, ctx->stream));
    CE_HIP(ctx, hipStreamSynchronize(ctx->stream));  // the slabs are free again: a later upload needs no fence against this
    for (uint32_t i = 0; over && i < count; i++)
        for (uint32_t j = 0; j < n_thresholds; j++) over[(size_t)i * n_thresholds + j] = b->ciede2000_over.h[(size_t)i * CE_CIEDE2000_MAX_THRESHOLDS + j];
    return CE_OK;
}

int ce_ciede2000_pixel_terms(const uint16_t *ref_rgb, uint32_t ref_depth, const uint16_t *test_rgb, uint32_t test_depth, size_t n, uint32_t *out)
{
    if (!ce_deep_depth_ok(ref_depth) || !ce_deep_depth_ok(test_depth))
        return ce_fail(nullptr, CE_ERR_INVALID_ARG, "ce_ciede2000_pixel_terms: depths must be 8, 10, 12 or 16 bits, got " + std::to_string(ref_depth) +
                                                     " / " + std::to_string(test_depth));
    if (!ref_rgb || !test_rgb || !out) return ce_fail(nullptr, CE_ERR_INVALID_ARG, "ce_ciede2000_pixel_terms: null pointer");
    const uint32_t maxv[2] = {(1u << ref_depth) - 1u, (1u << test_depth) - 1u};
    std::vector<float> tab[2];
    for (int s = 0; s < (ref_depth == test_depth ? 1 : 2); s++) {
        tab[s].resize((size_t)maxv[s] + 1);
        ce_build_srgb_table_f64(tab[s].data(), maxv[s]);
    }
    ce_ciede2000_pixel_terms_host(ref_rgb, tab[0].data(), maxv[0], test_rgb, tab[ref_depth == test_depth ? 0 : 1].data(), maxv[1], n, out);
    return CE_OK;
}

// ---- reference handle -------------------------------------------------------------------------

struct ce_ref {
    ce_ctx *ctx;
    ce_batch *batch;
    uint32_t flags;
};

int ce_ref_create(ce_ctx *ctx, const uint8_t *reference, size_t reference_len, uint32_t width, uint32_t height,
                  uint32_t flags, ce_ref **out)
{
    if (!ctx || !reference || !out) return CE_ERR_INVALID_ARG;
    *out = nullptr;
    if (reference_len != (size_t)width * height * 3) return ce_bad_length(ctx, (size_t)width * height * 3, reference_len);
    ce_batch *b = nullptr;
    int rc = ce_batch_create(ctx, width, height, 1, 1, &b);
    if (rc != CE_OK) return rc;
    rc = ce_batch_set_reference(b, 0, reference, reference_len);
    if (rc != CE_OK) {
        ce_batch_destroy(b);
        return rc;
    }
    b->refs.keep = true;  // whatever CE_KEEP_REFERENCE_STATE says: keeping the state is what a handle is
    b->ref_handle = true;
    *out = new ce_ref{ctx, b, flags};
    return CE_OK;
}

int ce_ref_compare_many(ce_ref *ref, const uint8_t *const *tests, const size_t *test_lens, uint32_t n_tests,
                        uint32_t metric_mask, float intensity_target, ce_scores *out)
{
    if (!ref || !tests || !test_lens || !out) return CE_ERR_INVALID_ARG;
    if (n_tests == 0) return CE_OK;
    ce_ctx *ctx = ref->ctx;
    ce_batch *b = ref->batch;
    CE_HIP(ctx, hipSetDevice(ctx->device));
    if (n_tests > b->max_pairs) {
        // grow the handle: a new batch of the same shape takes over the resident reference (device copy)
        ce_batch *nb = nullptr;
        int rc = ce_batch_create(ctx, b->w, b->h, 1, n_tests, &nb);
        if (rc != CE_OK) return rc;
        rc = ce_flush_uploads(b);
        if (rc != CE_OK) return rc;
        CE_HIP(ctx, hipMemcpyAsync(nb->d_refs, b->d_refs, b->img_bytes, hipMemcpyDeviceToDevice, ctx->stream));
        CE_HIP(ctx, hipStreamSynchronize(ctx->stream));
        ce_invalidate_reference_state(nb);  // a new slab: the first compare on it builds
        nb->refs.keep = true;
        nb->ref_handle = true;
        for (int k = 0; k < 3; k++) nb->refs.builds[k] = b->refs.builds[k];  // the handle's history (ce_ref_stats) carries over
        ce_batch_destroy(b);
        ref->batch = b = nb;
    }
    bool any_ok = false;
    for (uint32_t i = 0; i < n_tests; i++) {
        out[i] = ce_scores{};
        if (!tests[i]) return CE_ERR_INVALID_ARG;
        if (test_lens[i] != b->img_bytes) {
            out[i].status = ce_fail(ctx, CE_ERR_DIM_MISMATCH, "Dimension mismatch: reference " + std::to_string(b->img_bytes) +
                                                               " bytes, test " + std::to_string(test_lens[i]) + " bytes");
            continue;
        }
        any_ok = true;
    }
    if (!any_ok) return CE_OK;
    // Rejected items keep their slot (their scores are discarded); every valid test is uploaded to its own slot.
    std::vector<ce_scores> tmp(n_tests);
    b->caller_blocks = true;  // this call returns after its kernels: page-locked test images are read in place (upload())
    int rc = CE_OK;
    for (uint32_t i = 0; i < n_tests && rc == CE_OK; i++)
        rc = out[i].status != CE_OK ? ce_batch_bind_pair(b, i, 0) : ce_batch_set_test(b, i, 0, tests[i], test_lens[i]);
    if (rc == CE_OK) rc = ce_batch_run(b, n_tests, metric_mask, ref->flags, intensity_target, tmp.data());
    if (rc != CE_OK) ce_drain_batch(b);  // copies straight from the caller's memory may still be queued
    b->caller_blocks = false;
    if (rc != CE_OK) return rc;
    for (uint32_t i = 0; i < n_tests; i++)
        if (out[i].status == CE_OK) out[i] = tmp[i];
    return CE_OK;
}

int ce_ref_compare(ce_ref *ref, const uint8_t *test, size_t test_len, uint32_t metric_mask, float intensity_target,
                   ce_scores *out)
{
    if (!ref || !test || !out) return CE_ERR_INVALID_ARG;
    int rc = ce_ref_compare_many(ref, &test, &test_len, 1, metric_mask, intensity_target, out);
    if (rc != CE_OK) return rc;
    return out->status;
}

int ce_ref_butteraugli_diffmap(ce_ref *ref, uint32_t first, uint32_t count, uint32_t block, float *out, size_t out_floats)
{
    if (!ref) return CE_ERR_INVALID_ARG;
    return ce_batch_butteraugli_diffmap(ref->batch, first, count, block, out, out_floats);  // the handle's current batch (compare_many may replace it)
}

int ce_ref_dssim_ssim_maps(ce_ref *ref, uint32_t level, uint32_t first, uint32_t count, uint32_t block, float *maps,
                           size_t maps_floats, double *ssim)
{
    if (!ref) return CE_ERR_INVALID_ARG;
    return ce_batch_dssim_ssim_maps(ref->batch, level, first, count, block, maps, maps_floats, ssim);  // the handle's current batch
}

int ce_ref_ssimulacra2_maps(ce_ref *ref, uint32_t scale, uint32_t channel, uint32_t kind, uint32_t first, uint32_t count, uint32_t block,
                            float *maps, size_t maps_floats, double *norms)
{
    if (!ref) return ce_fail(nullptr, CE_ERR_INVALID_ARG, "null handle");
    return ce_batch_ssimulacra2_maps(ref->batch, scale, channel, kind, first, count, block, maps, maps_floats, norms);  // the handle's current batch
}

int ce_ref_image_heuristics(ce_ref *ref, ce_image_heuristics *out)
{
    if (!ref || !out) return CE_ERR_INVALID_ARG;
    return ce_batch_image_heuristics(ref->batch, CE_BATCH_REFERENCES, 0, 1, out);  // the handle's current batch holds its image
}

int ce_ssimulacra2_scales(uint32_t width, uint32_t height, uint32_t *n_scales, uint32_t *scale_w, uint32_t *scale_h)
{
    if (!n_scales || !scale_w || !scale_h) return ce_fail(nullptr, CE_ERR_INVALID_ARG, "null pointer");
    if (width == 0 || height == 0) return ce_fail(nullptr, CE_ERR_INVALID_ARG, "empty image");
    *n_scales = ce_plan_ssim2_scales(width, height, CE_SSIM2_MAX_SCALES, scale_w, scale_h);
    return CE_OK;
}

int ce_dssim_levels(uint32_t width, uint32_t height, uint32_t *n_levels, uint32_t *level_w, uint32_t *level_h)
{
    if (!n_levels || !level_w || !level_h) return ce_fail(nullptr, CE_ERR_INVALID_ARG, "null pointer");
    if (width == 0 || height == 0) return ce_fail(nullptr, CE_ERR_INVALID_ARG, "empty image");
    *n_levels = ce_plan_dssim_levels(width, height, CE_DSSIM_MAX_LEVELS, level_w, level_h);
    return CE_OK;
}

int ce_ref_stats(const ce_ref *ref, uint32_t builds[3])
{
    if (!ref || !builds) return CE_ERR_INVALID_ARG;
    return ce_batch_ref_stats(ref->batch, builds);
}

int ce_batch_ref_stats(const ce_batch *b, uint32_t builds[3])
{
    if (!b || !builds) return CE_ERR_INVALID_ARG;
    for (int k = 0; k < 3; k++) builds[k] = b->refs.builds[k];
    return CE_OK;
}

void ce_ref_destroy(ce_ref *ref)
{
    if (!ref) return;
    ce_batch_destroy(ref->batch);
    delete ref;
}

// ---- measurement hooks ----------------------------------------------------------------------

int ce_prof_enable(ce_ctx *ctx, int on)
{
    if (!ctx) return CE_ERR_INVALID_ARG;
    prof_drain(ctx);
    ctx->prof = on != 0;
    ctx->prof_serial = on == 1;
    return CE_OK;
}

int ce_prof_filter(ce_ctx *ctx, const char *substring)
{
    if (!ctx) return CE_ERR_INVALID_ARG;
    prof_drain(ctx);
    ctx->prof_filter = substring ? substring : "";
    return CE_OK;
}

int ce_prof_reset(ce_ctx *ctx)
{
    if (!ctx) return CE_ERR_INVALID_ARG;
    prof_drain(ctx);
    ctx->stats.clear();
    return CE_OK;
}

int ce_prof_count(ce_ctx *ctx)
{
    if (!ctx) return 0;
    prof_drain(ctx);
    return (int)ctx->stats.size();
}

int ce_prof_get(ce_ctx *ctx, int index, const char **name, uint64_t *launches, double *total_ms)
{
    if (!ctx || index < 0 || index >= (int)ctx->stats.size()) return CE_ERR_INVALID_ARG;
    prof_drain(ctx);
    if (name) *name = ctx->stats[index].name.c_str();
    if (launches) *launches = ctx->stats[index].launches;
    if (total_ms) *total_ms = ctx->stats[index].total_ms;
    return CE_OK;
}

int ce_timer_start(ce_ctx *ctx)
{
    if (!ctx) return CE_ERR_INVALID_ARG;
    CE_HIP(ctx, hipSetDevice(ctx->device));
    CE_HIP(ctx, hipEventRecord(ctx->t0, ctx->stream));
    return CE_OK;
}

int ce_timer_stop(ce_ctx *ctx, double *elapsed_ms)
{
    if (!ctx || !elapsed_ms) return CE_ERR_INVALID_ARG;
    CE_HIP(ctx, hipSetDevice(ctx->device));
    CE_HIP(ctx, hipEventRecord(ctx->t1, ctx->stream));
    CE_HIP(ctx, hipEventSynchronize(ctx->t1));
    float ms = 0.f;
    CE_HIP(ctx, hipEventElapsedTime(&ms, ctx->t0, ctx->t1));
    *elapsed_ms = ms;
    return CE_OK;
}

// ---- test hooks -------------------------------------------------------------------------------

int ce_debug_ssim2_planes(ce_batch *b, int scale, int which, int channel, float *out, size_t out_floats,
                          uint32_t *w_out, uint32_t *h_out)
{
    if (!b || !out || !b->s2.engaged() || scale < 0 || scale >= b->s2.n_scales) return CE_ERR_INVALID_ARG;
    ce_ctx *ctx = b->ctx;
    const ce_plane_geom &d = b->s2.lvl[scale];
    const int nplanes = which == 4 ? CE_SSIM2_STREAMS : 3;
    if (out_floats < (size_t)nplanes * d.w * d.h) return CE_ERR_INVALID_ARG;
    const uint32_t ref_slot = b->h_pair_ref[0], test_slot = b->max_refs;
    const float *src = nullptr;
    switch (which) {
        case 0:
        case 1:
            if (scale == 0) return CE_ERR_INVALID_ARG;  // level 0 has no linear plane (read from u8 on the fly)
            src = b->s2.lin[scale] + (size_t)(which == 0 ? ref_slot : test_slot) * 3 * d.plane;
            break;
        case 2: src = b->s2.xyb[scale] + (size_t)ref_slot * 3 * d.plane; break;
        case 3: src = b->s2.xyb[scale] + (size_t)test_slot * 3 * d.plane; break;
        case 4:
            if (channel < 0 || channel > 2) return CE_ERR_INVALID_ARG;
            src = b->s2.hbuf[scale] + (size_t)channel * CE_SSIM2_STREAMS * d.plane;
            // after a split-path launch the row-blurred a, a*a exist nowhere (they were scratch of the build)
            if (b->s2.split_last) return ce_fail(ctx, CE_ERR_INVALID_ARG, "the last launch took SSIMULACRA2's split path: it leaves no row-blurred reference streams to read");
            break;
        default: return CE_ERR_INVALID_ARG;
    }
    CE_HIP(ctx, hipSetDevice(ctx->device));
    CE_HIP(ctx, hipStreamSynchronize(ctx->stream));
    for (int p = 0; p < nplanes; p++)
        CE_HIP(ctx, hipMemcpy2D(out + (size_t)p * d.w * d.h, (size_t)d.w * sizeof(float), src + (size_t)p * d.plane,
                                d.pitch * sizeof(float), (size_t)d.w * sizeof(float), d.h, hipMemcpyDeviceToHost));
    if (w_out) *w_out = d.w;
    if (h_out) *h_out = d.h;
    return CE_OK;
}

int ce_debug_ssim2_limit_scales(ce_batch *b, int max_scales)
{
    if (!b || max_scales < 1 || max_scales > CE_MAX_SCALES) return CE_ERR_INVALID_ARG;
    b->debug_max_scales = max_scales;
    return CE_OK;
}

int ce_debug_dssim_walk_rows(ce_batch *b, uint32_t rows)
{
    // ds.part holds a strip's partial sums per 2-row tile (dssim.hip: ce_dssim_set::blocks), so every allowed walk fits
    if (!b || (rows != 0 && (rows < 2 || rows > 64 || (rows & (rows - 1)) != 0))) return CE_ERR_INVALID_ARG;
    b->debug_ds_rows = rows;
    b->refs.of[CE_REF_DSSIM].invalidate();  // the references' planes are walked at the new length too
    return CE_OK;
}

int ce_debug_ssim2_averages(ce_batch *b, uint32_t pair_index, double *avg, int *n_scales)
{
    if (!b || !avg || !b->s2.engaged() || pair_index >= b->max_pairs) return CE_ERR_INVALID_ARG;
    ce_ctx *ctx = b->ctx;
    CE_HIP(ctx, hipSetDevice(ctx->device));
    CE_HIP(ctx, hipStreamSynchronize(ctx->stream));
    CE_HIP(ctx, hipMemcpy(avg, b->s2.avg + (size_t)pair_index * CE_MAX_SCALES * 18, sizeof(double) * CE_MAX_SCALES * 18,
                          hipMemcpyDeviceToHost));
    if (n_scales) *n_scales = b->s2.n_scales;
    return CE_OK;
}

int ce_debug_ssim2_occupancy(int which) { return ce_ssim2_occupancy(which); }

int ce_debug_div_sweep(ce_ctx *ctx, uint64_t seed, uint64_t count, uint64_t *mismatches)
{
    if (!ctx || count == 0) return CE_ERR_INVALID_ARG;
    CE_HIP(ctx, hipSetDevice(ctx->device));
    return ce_butteraugli_div_sweep(ctx, seed, count, mismatches);
}

int ce_debug_calibrate_traffic(ce_ctx *ctx, size_t bytes)
{
    if (!ctx) return CE_ERR_INVALID_ARG;
    CE_HIP(ctx, hipSetDevice(ctx->device));
    return ce_calibrate_traffic(ctx, bytes);
}

int ce_debug_cbrt_sweep(ce_ctx *ctx, uint32_t first_bits, uint64_t count, uint64_t *mismatches, uint64_t *slow_path)
{
    if (!ctx || count == 0 || (uint64_t)first_bits + count > (1ull << 32)) return CE_ERR_INVALID_ARG;
    CE_HIP(ctx, hipSetDevice(ctx->device));
    return ce_ssim2_cbrt_sweep(ctx, first_bits, count, mismatches, slow_path);
}

}  // extern "C"
