// Everything that writes a slot of a resident batch (include/ce_metrics.h: ce_batch_set_*, ce_batch_bind_pair), the tables
// and the one-image leaves of the same conversions (ce_*_table, ce_*_to_linear, ce_yuv_to_rgb*, ce_tensor_to_*, ce_composite_*,
// ce_linear_over).  The handles some routes take (colour tables, ICC profiles) are made in ce_handles.cpp.
// Four things live here once and every route goes through them: the ordering rule of slot writes (ce_order_write), the
// wide staging pair (wide_send), the frame of a setter of one slot (set_slot) and of n consecutive slots (set_slots).  A
// route adds its check, which fills its plan, its fill of the staging pair and its launch.  All device work is in the .hip
// files.
#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <thread>

#include "ce_internal.h"

// ---- the upload path ------------------------------------------------------------------------------------------------------

// the reference slab is about to change: whatever was derived from it (XYB roundtrip, SSIMULACRA2 XYB pyramid, DSSIM
// img / mu / sq pyramid, Butteraugli PsychoImage) is rebuilt by the next launch
void ce_invalidate_reference_state(ce_batch *b) { b->refs.invalidate(); }

// kernels (context stream) must see everything uploaded so far
int ce_flush_uploads(ce_batch *b)
{
    if (!b->uploads_pending) return CE_OK;
    ce_ctx *ctx = b->ctx;
    CE_HIP(ctx, hipEventRecord(b->ev_up, b->up_stream));
    CE_HIP(ctx, hipStreamWaitEvent(ctx->stream, b->ev_up, 0));
    b->uploads_pending = false;
    return CE_OK;
}

// Called before every write into a slot; the one ordering rule of slot writes.  A slot is written either on the context's
// stream (the inline route of a small batch, upload(); a resample into the batch) or on the batch's upload stream (everything
// else).  A write on the context's stream while uploads are pending runs ce_flush_uploads first; a write on the upload stream
// waits for the batch's last launch, which may still read the slabs, and after an inline write that no launch has followed
// yet, for the context's stream.  A batch whose images all take one route never meets either fence.
int ce_order_write(ce_batch *b, bool on_ctx_stream)
{
    ce_ctx *ctx = b->ctx;
    if (on_ctx_stream) {
        b->inline_pending = true;  // cleared by the next launch, which runs behind it on the same stream
        return ce_flush_uploads(b);
    }
    if (b->run_pending) {
        CE_HIP(ctx, hipStreamWaitEvent(b->up_stream, b->ev_run, 0));
        b->run_pending = false;  // ordered from here on
    }
    if (b->inline_pending) {
        CE_HIP(ctx, hipEventRecord(b->ev_up, ctx->stream));
        CE_HIP(ctx, hipStreamWaitEvent(b->up_stream, b->ev_up, 0));
        b->inline_pending = false;
    }
    return CE_OK;
}

// true if the runtime knows `p` as page-locked host memory (hipHostMalloc / hipHostRegister): the DMA engine can
// read it directly
static bool is_pinned_host(const void *p)
{
    hipPointerAttribute_t a{};
    if (hipPointerGetAttributes(&a, p) != hipSuccess) {
        (void)hipGetLastError();  // an ordinary pageable pointer is reported as an error: clear it
        return false;
    }
    return a.type == hipMemoryTypeHost;
}

// One image into a device slot on stream `s`; returns the HIP error (no ctx->err), so that upload threads can call it.
// stage < 0: a page-locked source the DMA engine reads in place (the caller collects before it can go away); otherwise
// the source goes through pinned staging slot `stage` (once its previous DMA is done) and is consumed on return.
static hipError_t copy_in(ce_batch *b, int stage, uint8_t *dst, const uint8_t *src, hipStream_t s)
{
    if (stage < 0) return hipMemcpyAsync(dst, src, b->img_bytes, hipMemcpyHostToDevice, s);
    hipError_t e = b->stage_busy[stage] ? hipEventSynchronize(b->ev_stage[stage]) : hipSuccess;
    if (e == hipSuccess) {
        std::memcpy(b->h_stage[stage], src, b->img_bytes);
        e = hipMemcpyAsync(dst, b->h_stage[stage], b->img_bytes, hipMemcpyHostToDevice, s);
    }
    if (e == hipSuccess) e = hipEventRecord(b->ev_stage[stage], s);
    b->stage_busy[stage] = true;
    return e;
}

static int upload(ce_batch *b, uint8_t *dst, const uint8_t *src, bool allow_inline = true)
{
    ce_ctx *ctx = b->ctx;
    // pageable source -> pinned staging ring -> device on the batch's upload stream: the DMA of this slot overlaps the
    // host copy into the next one and the kernels of other batches
    CE_HIP(ctx, hipSetDevice(ctx->device));  // the calling thread's current device may be another one (multi-device hosts)
    // A small batch (the one-pair-per-call regime of a reference handle) uploads on the context's own stream: its launch
    // follows at once, and a cross-stream event between the copy and the first kernel costs ~25 us of its ~0.5 ms
    // (not for an image that a format conversion or a colour table follows on the upload stream: allow_inline = false)
    const bool inline_copy = allow_inline && (double)b->max_pairs * b->w * b->h <= 4e6;
    if (int rc = ce_order_write(b, inline_copy)) return rc;
    // A BLOCKING entry point (ce_ref_compare*, which collects before it returns) whose caller's image is page-locked
    // (ce_host_alloc) needs no staging copy: the DMA engine reads the caller's buffer, which outlives the call's kernels.
    const int stage = b->caller_blocks && is_pinned_host(src) ? -1 : b->next_stage;
    if (stage >= 0) b->next_stage = (stage + 1) % ce_batch::kStages;
    const hipError_t e = copy_in(b, stage, dst, src, inline_copy ? ctx->stream : b->up_stream);
    if (!inline_copy) b->uploads_pending = true;
    if (e != hipSuccess) return ce_fail(ctx, CE_ERR_BACKEND, std::string("upload: ") + hipGetErrorString(e));
    return CE_OK;
}

// Many images at once (ce_eval_batch): the host copies into the pinned ring are spread over a few threads, each
// with its own pair of ring slots, because one thread's memcpy (~12 GB/s) is slower than the PCIe link.
int ce_upload_many(ce_batch *b, const std::vector<ce_upload_job> &jobs)
{
    ce_ctx *ctx = b->ctx;
    if (jobs.empty()) return CE_OK;
    CE_HIP(ctx, hipSetDevice(ctx->device));
    // Page-locked sources skip the staging ring: one asynchronous copy per image straight from the caller's buffer.
    // Only ce_eval_batch comes through here, and it collects (synchronises) before it returns, so the buffers
    // outlive the copies.
    const bool all_pinned = std::all_of(jobs.begin(), jobs.end(), [](const ce_upload_job &j) { return is_pinned_host(j.src); });
    const int n_threads = (int)std::min<size_t>({(size_t)ce_batch::kStages / 2, jobs.size(),
                                                 (size_t)std::max(1u, std::thread::hardware_concurrency())});
    if (!all_pinned && (n_threads <= 1 || b->img_bytes < (64u << 10))) {
        for (const auto &j : jobs) {
            int rc = upload(b, j.dst, j.src, false);
            if (rc != CE_OK) return rc;
        }
        return CE_OK;
    }
    // One stream moves a 786 KB image in 38 us (20.6 GB/s): the 1.88 GB of the Kodak + CID22 sweep would take as long as its
    // kernels.  The copies of a chunk therefore alternate between the batch's upload stream and a second one of the context,
    // which is fenced on both sides so that everything else keeps seeing "the uploads are on up_stream".
    static const int n_up = [] {
        const char *e = std::getenv("CE_UPLOAD_STREAMS");
        return e ? std::max(1, std::min(2, std::atoi(e))) : 2;  // 2000 pairs of 512x512, page-locked: 99.9 -> 95.4 ms; pageable: see r03_experiments 17
    }();
    const bool two_up = n_up == 2 && jobs.size() >= 16;
    auto up2_begin = [&]() -> int {
        if (!ctx->up2_stream) {
            CE_HIP(ctx, hipStreamCreateWithFlags(&ctx->up2_stream, hipStreamNonBlocking));
            CE_HIP(ctx, hipEventCreateWithFlags(&ctx->ev_up2, hipEventDisableTiming));
        }
        CE_HIP(ctx, hipEventRecord(ctx->ev_up2, b->up_stream));  // behind whatever up_stream already waits for
        CE_HIP(ctx, hipStreamWaitEvent(ctx->up2_stream, ctx->ev_up2, 0));
        return CE_OK;
    };
    auto up2_end = [&]() -> int {
        CE_HIP(ctx, hipEventRecord(ctx->ev_up2, ctx->up2_stream));
        CE_HIP(ctx, hipStreamWaitEvent(b->up_stream, ctx->ev_up2, 0));
        return CE_OK;
    };
    if (int rc = ce_order_write(b, false)) return rc;
    if (two_up)
        if (int rc = up2_begin()) return rc;
    std::atomic<size_t> next{0};
    std::atomic<int> err{(int)hipSuccess};
    const int device = ctx->device;
    auto worker = [&](int t) {
        if (hipSetDevice(device) != hipSuccess) return;
        for (int flip = 0;; flip ^= 1) {
            const size_t i = next.fetch_add(1);
            if (i >= jobs.size()) break;
            // page-locked: one thread whose copies alternate between the streams; staged: a worker's two ring slots stay on its stream
            const hipStream_t us = (two_up && ((all_pinned ? i : (size_t)t) & 1)) ? ctx->up2_stream : b->up_stream;
            const hipError_t e = copy_in(b, all_pinned ? -1 : 2 * t + flip, jobs[i].dst, jobs[i].src, us);
            if (e != hipSuccess) {
                err.store((int)e);
                break;
            }
        }
    };
    std::vector<std::thread> pool;
    for (int t = 1; t < (all_pinned ? 1 : n_threads); t++) {
        try {
            pool.emplace_back(worker, t);
        } catch (...) {  // no thread to be had: the calling thread's loop below takes whatever is left (nothing may be thrown across the C ABI)
            break;
        }
    }
    worker(0);
    for (auto &th : pool) th.join();
    b->uploads_pending = true;
    if (two_up)
        if (int rc = up2_end()) return rc;
    if (err.load() != (int)hipSuccess)
        return ce_fail(ctx, CE_ERR_BACKEND, std::string("upload: ") + hipGetErrorString((hipError_t)err.load()));
    return CE_OK;
}

// the table runs on the batch's upload stream, behind the copy (and the format conversion) of the same image
int ce_apply_lut(ce_batch *b, uint8_t *slot, const ce_lut *lut)
{
    if (!lut) return CE_OK;
    if (lut->ctx->device != b->ctx->device) return ce_fail(b->ctx, CE_ERR_INVALID_ARG, "colour table and batch are on different devices");
    // the table was built on its context's stream and ce_lut_create synchronised: it is complete
    return ce_launch_lut_apply(b->ctx, b->up_stream, slot, lut->d_table, (size_t)b->w * b->h);
}

namespace {

// ---- the wide staging pair ------------------------------------------------------------------------------------------------

// Every image that a conversion kernel follows (a decoder's format, tagged code values, host Y'CbCr planes, RGBA over
// backgrounds) goes host -> h_wide[k] -> d_wide[k] -> kernel -> slot on the batch's upload stream.  There are two pairs, made
// on first use: while pair k's copy and conversion are in flight the host fills the other.  A pair holds 8 bytes per pixel,
// the widest decoder format (16 on a linear batch: packed f32 RGBA, which the linear-light composite takes).
struct wide_pair {
    uint8_t *h, *d;  // the pinned host buffer to fill and where its device copy will be
    int k;           // which of the two, for a route that keeps a pair of its own beside it (the gain map's side pair)
};

// One image through the next wide pair, and the only code that touches the pairs: the pair is taken ordered as a slot write
// and free of its previous image; fill(pair) writes `bytes` into pair.h (pair.d is for a route whose launch arguments point
// into the device copy); then the copy, launch(pair) on up_stream, and the event behind it that keeps the pair busy until
// up_stream gets there.  A fill or a launch that fails returns before the pair is closed.
template <class Fill, class Launch>
int wide_send(ce_batch *b, size_t bytes, Fill fill, Launch launch)
{
    ce_ctx *ctx = b->ctx;
    CE_HIP(ctx, hipSetDevice(ctx->device));  // the staging allocations and the launch go to the context's device
    const int k = b->next_wide;
    b->next_wide ^= 1;
    if (!b->ev_wide[k])
        if (int rc = b->ev_wide[k].create(ctx)) return rc;
    if (int rc = ce_order_write(b, false)) return rc;
    if (b->wide_busy[k]) CE_HIP(ctx, hipEventSynchronize(b->ev_wide[k]));  // this staging pair's previous image has been converted
    b->wide_busy[k] = false;
    if (!b->wide[k] || b->wide[k].h.size() < bytes) {
        // A tensor image takes up to 16 bytes per pixel in any batch (f32 RGBA; planar f32: 12): the pair grows for the call
        // that needs more, behind its event, so every other workload keeps the memory it had.
        b->wide[k].reset();
        if (int rc = b->wide[k].alloc(ctx, std::max((size_t)b->w * b->h * (b->linear ? 16 : 8), bytes))) return rc;
    }
    const wide_pair pair{b->wide[k].h, b->wide[k].d, k};
    if (int rc = fill(pair)) return rc;
    CE_HIP(ctx, hipMemcpyAsync(pair.d, pair.h, bytes, hipMemcpyHostToDevice, b->up_stream));
    if (int rc = launch(pair)) return rc;
    CE_HIP(ctx, hipEventRecord(b->ev_wide[k], b->up_stream));
    b->wide_busy[k] = true;
    b->uploads_pending = true;
    return CE_OK;
}

// the fill of a route whose image is packed already
auto packed_fill(const void *pixels, size_t len)
{
    return [=](const wide_pair &p) {
        std::memcpy(p.h, pixels, len);
        return CE_OK;
    };
}

// ---- the frame of a setter --------------------------------------------------------------------------------------------------

// the batches a route refuses - those whose `linear` is this one - and the text it refuses them with (no text: none)
struct kind_rule {
    bool linear = false;
    const char *text = nullptr;
};

// Every setter of one slot: reference `ref_index`, or with `test` the test image of `pair_index`, bound to `ref_index`.
// check() holds the route's own refusals and fills its plan; write(slot) queues the image into the slot.
template <class Check, class Write>
int set_slot(ce_batch *b, bool test, uint32_t pair_index, uint32_t ref_index, kind_rule refuses, Check check, Write write)
{
    if (!b) return CE_ERR_INVALID_ARG;
    if (refuses.text && b->linear == refuses.linear) return ce_fail(b->ctx, CE_ERR_INVALID_ARG, refuses.text);
    if (test && (pair_index >= b->max_pairs || ref_index >= b->max_refs)) return ce_fail(b->ctx, CE_ERR_INVALID_ARG, "pair/ref index out of range");
    if (!test && ref_index >= b->max_refs) return ce_fail(b->ctx, CE_ERR_INVALID_ARG, "ref_index out of range");
    if (int rc = check()) return rc;
    if (test) {
        if (int rc = ce_batch_bind_pair(b, pair_index, ref_index)) return rc;
    } else {
        ce_invalidate_reference_state(b);  // cached reference-side planes are stale
    }
    return write(test ? b->d_tests + (size_t)pair_index * b->img_bytes : b->d_refs + (size_t)ref_index * b->img_bytes);
}

// Every setter of n consecutive slots from `first` on, the test slots bound to ref_indices[]: set_slot's frame with `route`
// ("alpha compositing: ") in front of its own messages.  null_arg: one of the route's pointers is null; check() and
// write(first slot) as set_slot's.
template <class Check, class Write>
int set_slots(ce_batch *b, bool test, uint32_t first, uint32_t n, const uint32_t *ref_indices, const char *route, kind_rule refuses, bool null_arg,
              Check check, Write write)
{
    if (!b) return CE_ERR_INVALID_ARG;
    ce_ctx *ctx = b->ctx;
    if (refuses.text && b->linear == refuses.linear) return ce_fail(ctx, CE_ERR_INVALID_ARG, refuses.text);
    if ((test && !ref_indices) || null_arg) return ce_fail(ctx, CE_ERR_INVALID_ARG, std::string(route) + "null pointer");
    if (int rc = check()) return rc;
    const uint32_t slots = test ? b->max_pairs : b->max_refs;
    if (first > slots || n > slots - first)
        return ce_fail(ctx, CE_ERR_INVALID_ARG, std::string(route) + (test ? "test" : "reference") + " slots [" + std::to_string(first) + ", " +
                                                    std::to_string((uint64_t)first + n) + ") outside the " + std::to_string(slots) + " slots");
    for (uint32_t k = 0; test && k < n; k++)
        if (ref_indices[k] >= b->max_refs) return ce_fail(ctx, CE_ERR_INVALID_ARG, std::string(route) + "ref index " + std::to_string(ref_indices[k]) + " out of range");
    for (uint32_t k = 0; test && k < n; k++)
        if (int rc = ce_batch_bind_pair(b, first + k, ref_indices[k])) return rc;
    if (!test) ce_invalidate_reference_state(b);
    return write((test ? b->d_tests : b->d_refs) + (size_t)first * b->img_bytes);
}

// ---- RGB8, a decoder's formats, colour tables ---------------------------------------------------------------------------------

const char *const kLinearWants =
    "a linear batch takes CE_PIXEL_RGB_F32 through ce_batch_set_*_fmt and tagged code values through ce_batch_set_*_cicp";

int fmt_check(ce_batch *b, size_t len, int format, uint32_t depth)
{
    ce_ctx *ctx = b->ctx;
    const size_t bpp = ce_pixel_bytes(format), n_px = (size_t)b->w * b->h;
    if (bpp == 0) return ce_fail(ctx, CE_ERR_INVALID_ARG, "unknown pixel format");
    if (b->linear != (format == CE_PIXEL_RGB_F32))
        return ce_fail(ctx, CE_ERR_INVALID_ARG, b->linear ? kLinearWants : "CE_PIXEL_RGB_F32 needs a linear batch (ce_batch_create_linear)");
    const bool fmt16 = format == CE_PIXEL_RGB16 || format == CE_PIXEL_RGBA16, fmt8 = format == CE_PIXEL_RGB8 || format == CE_PIXEL_RGBA8;
    if (!depth && fmt16) return ce_fail(ctx, CE_ERR_INVALID_ARG, "CE_PIXEL_RGB16 / CE_PIXEL_RGBA16 need a deep batch (ce_batch_create_deep)");
    if (depth && !fmt16 && !fmt8)
        return ce_fail(ctx, CE_ERR_INVALID_ARG, "the *_10BIT formats round to 8 bits: a deep batch takes CE_PIXEL_RGB16 / CE_PIXEL_RGBA16");
    if (depth && fmt8 && depth != 8)
        return ce_fail(ctx, CE_ERR_INVALID_ARG, "an 8-bit image needs a side of depth 8, this one has " + std::to_string(depth));
    if (len != n_px * bpp) return ce_bad_length(ctx, n_px * bpp, len);
    return CE_OK;
}

// checked pixels in a decoder's format -> wide staging -> device -> ingest kernel writes the RGB8 slab slot
// (a deep batch: -> the ingest kernel that writes the u16 slab slot of that side, depth `depth`; 0 = an RGB8 batch)
int upload_fmt(ce_batch *b, uint8_t *dst, const void *pixels, size_t len, int format, uint32_t depth)
{
    ce_ctx *ctx = b->ctx;
    const size_t n_px = (size_t)b->w * b->h;
    if (format == CE_PIXEL_RGB8 && !depth) return upload(b, dst, static_cast<const uint8_t *>(pixels), false);
    return wide_send(b, len, packed_fill(pixels, len), [&](const wide_pair &p) {
        return b->linear ? ce_launch_linear_sanitise(ctx, b->up_stream, reinterpret_cast<const float *>(p.d), reinterpret_cast<float *>(dst), n_px * 3)
               : depth   ? ce_launch_ingest_deep(ctx, b->up_stream, format, depth, p.d, reinterpret_cast<uint16_t *>(dst), n_px)
                         : ce_launch_ingest(ctx, b->up_stream, format, p.d, dst, n_px);
    });
}

// ce_batch_set_*_fmt (lut = nullptr) and ce_batch_set_*_lut
int set_fmt(ce_batch *b, bool test, uint32_t pair_index, uint32_t ref_index, const void *pixels, size_t len, int format, const ce_lut *lut)
{
    if (b && lut && b->depth[0]) return ce_fail(b->ctx, CE_ERR_INVALID_ARG, "a colour table is 2^24 8-bit colours: not for a deep batch");
    if (b && lut && b->linear) return ce_fail(b->ctx, CE_ERR_INVALID_ARG, "a colour table is 2^24 8-bit colours: not for a linear batch");
    if (!b || !pixels) return CE_ERR_INVALID_ARG;
    return set_slot(
        b, test, pair_index, ref_index, kind_rule{}, [&] { return fmt_check(b, len, format, b->depth[test]); },
        [&](uint8_t *slot) {
            if (int rc = upload_fmt(b, slot, pixels, len, format, b->depth[test])) return rc;
            return ce_apply_lut(b, slot, lut);
        });
}

// ce_batch_set_reference / ce_batch_set_test: a deep batch widens RGB8 on the device.  (The reference setter has always
// tested its index before the batch kind and the test setter after: both keep their order.)
int set_rgb8(ce_batch *b, bool test, uint32_t pair_index, uint32_t ref_index, const uint8_t *rgb, size_t len)
{
    if (!b || !rgb) return CE_ERR_INVALID_ARG;
    if (b->depth[0]) return set_fmt(b, test, pair_index, ref_index, rgb, len, CE_PIXEL_RGB8, nullptr);
    return set_slot(
        b, test, pair_index, ref_index, test ? kind_rule{true, kLinearWants} : kind_rule{},
        [&]() -> int {
            if (b->linear) return ce_fail(b->ctx, CE_ERR_INVALID_ARG, kLinearWants);
            if (len != b->img_bytes) return ce_bad_length(b->ctx, b->img_bytes, len);
            return CE_OK;
        },
        [&](uint8_t *slot) { return upload(b, slot, rgb); });
}

// ---- tagged code values into a linear batch: CICP and HLG (cicp.hip; DESIGN.md sections 15, 18) -------------------

// The two descriptions share their checks and their entry points, written once below over `Desc`; what differs is here:
// the words of their messages, the check of the description alone (colour_check: fills maxv, the matrix and, for HLG, the
// five doubles) and the device table (table_dev).
struct route_words {
    const char *name, *depth_owner;
};
route_words words(const ce_colour *) { return {"CICP", "colour description's"}; }
route_words words(const ce_hlg *) { return {"HLG", "description's"}; }

// depth, transfer and primaries from the lists of the header
int colour_check(ce_ctx *ctx, const ce_colour *c, ce_linear_pixel *plan)
{
    if (!ce_deep_depth_ok(c->depth)) return ce_fail(ctx, CE_ERR_INVALID_ARG, "CICP ingest: depth must be 8, 10, 12 or 16, got " + std::to_string(c->depth));
    if (c->transfer != 13 && c->transfer != 8 && c->transfer != 16)
        return ce_fail(ctx, CE_ERR_INVALID_ARG, "CICP ingest: transfer must be 13 (sRGB), 8 (linear) or 16 (PQ), got " + std::to_string(c->transfer) +
                                                    (c->transfer == 18 ? " (HLG carries a display description: ce_batch_set_*_hlg)" : ""));
    if (c->transfer == 16 && !(c->white_nits > 0.0f && std::isfinite(c->white_nits)))
        return ce_fail(ctx, CE_ERR_INVALID_ARG, "CICP ingest: PQ needs white_nits > 0");
    if (!ce_build_colour_matrix(c->primaries, plan->m))
        return ce_fail(ctx, CE_ERR_INVALID_ARG, "CICP ingest: primaries must be 1 (BT.709), 9 (BT.2020) or 12 (Display P3), got " + std::to_string(c->primaries));
    plan->has_matrix = c->primaries != 1;
    plan->maxv = (1u << c->depth) - 1u;
    plan->d_table = nullptr;
    return CE_OK;
}

// primaries and depth from the header's lists, the two luminances finite and > 0, the system gamma - given, or BT.2100's
// rule from the peak - in [0.8, 1.6]; out = {kR, kG, kB, gamma - 1, A}
int hlg_describe(ce_ctx *ctx, const ce_hlg *h, double out[5])
{
    if (!ce_deep_depth_ok(h->depth)) return ce_fail(ctx, CE_ERR_INVALID_ARG, "HLG ingest: depth must be 8, 10, 12 or 16, got " + std::to_string(h->depth));
    if (!ce_build_luminance_row(h->primaries, out))
        return ce_fail(ctx, CE_ERR_INVALID_ARG, "HLG ingest: primaries must be 1 (BT.709), 9 (BT.2020) or 12 (Display P3), got " + std::to_string(h->primaries));
    if (!(h->peak_nits > 0.0f && std::isfinite(h->peak_nits))) return ce_fail(ctx, CE_ERR_INVALID_ARG, "HLG ingest: peak_nits must be finite and > 0");
    if (!(h->white_nits > 0.0f && std::isfinite(h->white_nits))) return ce_fail(ctx, CE_ERR_INVALID_ARG, "HLG ingest: white_nits must be finite and > 0");
    const double gamma = h->system_gamma != 0.0f ? (double)h->system_gamma : 1.2 + 0.42 * std::log10((double)h->peak_nits / 1000.0);
    if (!(gamma >= 0.8 && gamma <= 1.6))
        return ce_fail(ctx, CE_ERR_INVALID_ARG, "HLG ingest: the system gamma must lie in [0.8, 1.6], got " + std::to_string(gamma));
    out[3] = gamma - 1.0;
    out[4] = (double)h->peak_nits / (double)h->white_nits;
    return CE_OK;
}

int colour_check(ce_ctx *ctx, const ce_hlg *h, ce_linear_pixel *plan)
{
    if (int rc = hlg_describe(ctx, h, plan->hlg_params)) return rc;
    ce_build_colour_matrix(h->primaries, plan->m);
    plan->hlg = true;
    plan->has_matrix = h->primaries != 1;
    plan->maxv = (1u << h->depth) - 1u;
    plan->d_table = nullptr;
    return CE_OK;
}

// The device copy of an ingest's table (ce_ctx::cicp_tables): 2^depth floats, made by `build` on first use and kept until
// the context goes; `what` names it in an error
int ingest_table(ce_ctx *ctx, int transfer, uint32_t depth, uint32_t white_bits, const char *what, const std::function<void(float *)> &build,
                 const float **out)
{
    const auto key = std::make_tuple(transfer, depth, white_bits);
    auto it = ctx->cicp_tables.find(key);
    if (it == ctx->cicp_tables.end()) {
        std::vector<float> host((size_t)1 << depth);
        build(host.data());
        CE_HIP(ctx, hipSetDevice(ctx->device));
        void *d = nullptr;
        if (int rc = ce_device_table(ctx, host.data(), host.size() * sizeof(float), what, &d)) return rc;
        it = ctx->cicp_tables.emplace(key, static_cast<float *>(d)).first;
    }
    *out = it->second;
    return CE_OK;
}

// the transfer table of a checked description, keyed by (transfer, depth, white); white only matters to PQ
int table_dev(ce_ctx *ctx, const ce_colour *c, ce_linear_pixel *plan)
{
    const float white = c->transfer == 16 ? c->white_nits : 0.0f;
    uint32_t white_bits;
    std::memcpy(&white_bits, &white, 4);
    return ingest_table(
        ctx, c->transfer, c->depth, white_bits, "transfer table",
        [&](float *t) { ce_build_transfer_table(c->transfer, plan->maxv, (double)white, t); }, &plan->d_table);
}

// the inverse-OETF table of a checked description, one per depth, under H.273's code for HLG: (18, depth, 0)
int table_dev(ce_ctx *ctx, const ce_hlg *h, ce_linear_pixel *plan)
{
    return ingest_table(ctx, 18, h->depth, 0u, "HLG table", [&](float *t) { ce_build_hlg_table(plan->maxv, t); }, &plan->d_table);
}

// one image of code values with its description: everything refused about either, then the plan
template <class Desc>
int tagged_check(ce_ctx *ctx, const void *pixels, size_t len, int format, const Desc *d, size_t n_px, ce_linear_pixel *plan)
{
    const std::string route = std::string(words(d).name) + " ingest: ";
    if (!pixels || !d) return ce_fail(ctx, CE_ERR_INVALID_ARG, route + "null pointer");
    const bool fmt8 = format == CE_PIXEL_RGB8 || format == CE_PIXEL_RGBA8, fmt16 = format == CE_PIXEL_RGB16 || format == CE_PIXEL_RGBA16;
    if (!fmt8 && !fmt16) return ce_fail(ctx, CE_ERR_INVALID_ARG, route + "format must be CE_PIXEL_RGB8, RGBA8, RGB16 or RGBA16");
    if (fmt8 && ce_deep_depth_ok(d->depth) && d->depth != 8)
        return ce_fail(ctx, CE_ERR_INVALID_ARG, route + "an 8-bit format needs depth 8, got " + std::to_string(d->depth));
    if (int rc = colour_check(ctx, d, plan)) return rc;
    if (len != n_px * ce_pixel_bytes(format)) return ce_bad_length(ctx, n_px * ce_pixel_bytes(format), len);
    return table_dev(ctx, d, plan);
}

// one checked image through the wide staging pair into the slot at dst
int upload_cicp(ce_batch *b, uint8_t *dst, const void *pixels, size_t len, int format, const ce_linear_pixel &plan)
{
    return wide_send(b, len, packed_fill(pixels, len), [&](const wide_pair &p) {
        return ce_launch_tagged(b->ctx, b->up_stream, format, p.d, reinterpret_cast<float *>(dst), (size_t)b->w * b->h, plan);
    });
}

const char *const kCicpWantsLinear = "CICP ingest writes linear light: it needs a linear batch (ce_batch_create_linear)";
const char *const kHlgWantsLinear = "HLG ingest writes linear light: it needs a linear batch (ce_batch_create_linear)";

// ce_batch_set_*_cicp and ce_batch_set_*_hlg
template <class Desc>
int set_tagged(ce_batch *b, bool test, uint32_t pair_index, uint32_t ref_index, const void *pixels, size_t len, int format, const Desc *d,
               const char *wants_linear)
{
    ce_linear_pixel plan;
    return set_slot(
        b, test, pair_index, ref_index, kind_rule{false, wants_linear},
        [&] { return tagged_check(b->ctx, pixels, len, format, d, (size_t)b->w * b->h, &plan); },
        [&](uint8_t *slot) { return upload_cicp(b, slot, pixels, len, format, plan); });
}

// ce_cicp_to_linear and ce_hlg_to_linear: one image of code values -> packed f32 RGB in host memory
template <class Desc>
int tagged_to_linear(ce_ctx *ctx, const void *pixels, size_t len, int format, const Desc *d, uint32_t w, uint32_t h, float *out, size_t out_len)
{
    if (!ctx || !out) return CE_ERR_INVALID_ARG;
    const std::string route = std::string(words(d).name) + " ingest: ";
    if (w == 0 || h == 0) return ce_fail(ctx, CE_ERR_INVALID_ARG, route + "empty image");
    const size_t n_px = (size_t)w * h;
    ce_linear_pixel plan;
    if (int rc = tagged_check(ctx, pixels, len, format, d, n_px, &plan)) return rc;
    if (out_len != n_px * 3) return ce_fail(ctx, CE_ERR_BAD_LENGTH, route + "out_len must be " + std::to_string(n_px * 3) + " floats, got " + std::to_string(out_len));
    return ce_leaf_roundtrip(ctx, pixels, len, out, n_px * 12, [&](uint8_t *d_in, uint8_t *d_out) {
        return ce_launch_tagged(ctx, ctx->stream, format, d_in, reinterpret_cast<float *>(d_out), n_px, plan);
    });
}

// ---- gain-map images into a linear batch (gainmap.hip) ------------------------------------------------

// the three headrooms, which is all that W reads
int gainmap_headrooms_check(ce_ctx *ctx, const ce_gainmap *g)
{
    const struct {
        const char *name;
        float v;
    } rooms[3] = {{"base_headroom", g->base_headroom}, {"alternate_headroom", g->alternate_headroom}, {"display_headroom", g->display_headroom}};
    for (const auto &r : rooms)
        if (!std::isfinite(r.v) || std::fabs(r.v) > 16.0f)
            return ce_fail(ctx, CE_ERR_INVALID_ARG, std::string("gain-map ingest: ") + r.name + " must be finite and within [-16, 16]");
    if (g->alternate_headroom == g->base_headroom)
        return ce_fail(ctx, CE_ERR_INVALID_ARG, "gain-map ingest: alternate_headroom equals base_headroom, so no weight is defined");
    return CE_OK;
}

// the metadata that `channels` channels read
int gainmap_meta_check(ce_ctx *ctx, const ce_gainmap *g, uint32_t channels)
{
    if (channels != 1 && channels != 3) return ce_fail(ctx, CE_ERR_INVALID_ARG, "gain-map ingest: channels must be 1 or 3, got " + std::to_string(channels));
    if (int rc = gainmap_headrooms_check(ctx, g)) return rc;
    for (uint32_t c = 0; c < channels; c++) {
        const std::string at = " of channel " + std::to_string(c);
        for (float v : {g->gain_min[c], g->gain_max[c], g->gamma[c], g->base_offset[c], g->alternate_offset[c]})
            if (!std::isfinite(v)) return ce_fail(ctx, CE_ERR_INVALID_ARG, "gain-map ingest: a value that is not finite in the metadata" + at);
        if (!(g->gamma[c] > 0.0f)) return ce_fail(ctx, CE_ERR_INVALID_ARG, "gain-map ingest: gamma must be > 0" + at);
        if (g->gain_min[c] > g->gain_max[c]) return ce_fail(ctx, CE_ERR_INVALID_ARG, "gain-map ingest: gain_min is above gain_max" + at);
        if (std::fabs(g->gain_min[c]) > 16.0f || std::fabs(g->gain_max[c]) > 16.0f)
            return ce_fail(ctx, CE_ERR_INVALID_ARG, "gain-map ingest: the log2 gains must lie within [-16, 16]" + at);
        if (std::fabs(g->base_offset[c]) > 1.0f || std::fabs(g->alternate_offset[c]) > 1.0f)
            return ce_fail(ctx, CE_ERR_INVALID_ARG, "gain-map ingest: the offsets must lie within [-1, 1]" + at);
    }
    return CE_OK;
}

// one base image with its description, map and metadata: everything refused about any of them, then the plan
int gainmap_check(ce_ctx *ctx, const void *pixels, size_t len, int format, const ce_colour *c, const ce_gainmap_image *map, const ce_gainmap *g,
                  uint32_t w, uint32_t h, ce_gainmap_plan *plan)
{
    if (!pixels || !c || !map || !g || !map->samples) return ce_fail(ctx, CE_ERR_INVALID_ARG, "gain-map ingest: null pointer");
    if (int rc = gainmap_meta_check(ctx, g, map->channels)) return rc;
    if (map->width == 0 || map->height == 0 || map->width > w || map->height > h)
        return ce_fail(ctx, CE_ERR_INVALID_ARG, "gain-map ingest: a map of " + std::to_string(map->width) + " x " + std::to_string(map->height) +
                                                    " for a base of " + std::to_string(w) + " x " + std::to_string(h) + ": it must be 1 x 1 at least and the base's size at most");
    if (int rc = tagged_check(ctx, pixels, len, format, c, (size_t)w * h, &plan->base)) return rc;
    plan->gw = map->width, plan->gh = map->height, plan->channels = map->channels;
    for (int i = 0; i < 3; i++) {
        const int k = map->channels == 3 ? i : 0;
        plan->base_offset[i] = (double)g->base_offset[k], plan->alternate_offset[i] = (double)g->alternate_offset[k];
    }
    ce_build_gainmap_tables(g, map->channels, plan->ytab);
    return CE_OK;
}

// what travels beside the base image: the plan's tables, then the map's samples (ce_launch_gainmap's d_side)
size_t gainmap_side(const ce_gainmap_plan &plan, const ce_gainmap_image *map, uint8_t *h_side)
{
    std::memcpy(h_side, plan.ytab, plan.table_bytes());
    std::memcpy(h_side + plan.table_bytes(), map->samples, plan.map_bytes());
    return plan.table_bytes() + plan.map_bytes();
}

// One checked image into the slot at dst: the base through the wide staging pair, the tables and the map through a pair of
// their own beside it, made on first use for the largest map the batch's shape admits (three channels at the base's size) -
// a wide pair is w * h * 12 bytes, which a small RGBA16 base with such a map would overrun.  Both are busy until the launch
// is done, under the wide pair's event: the side pair is filled before the copies are queued, and its copy goes behind the base's.
int upload_gainmap(ce_batch *b, uint8_t *dst, const void *pixels, size_t len, int format, const ce_gainmap_image *map, const ce_gainmap_plan &plan)
{
    ce_ctx *ctx = b->ctx;
    size_t side = 0;
    return wide_send(
        b, len,
        [&](const wide_pair &p) -> int {
            if (!b->side[p.k])
                if (int rc = b->side[p.k].alloc(ctx, 3 * 256 * sizeof(double) + (size_t)b->w * b->h * 3)) return rc;
            std::memcpy(p.h, pixels, len);
            side = gainmap_side(plan, map, b->side[p.k].h);
            return CE_OK;
        },
        [&](const wide_pair &p) -> int {
            CE_HIP(ctx, hipMemcpyAsync(b->side[p.k].d, b->side[p.k].h, side, hipMemcpyHostToDevice, b->up_stream));
            return ce_launch_gainmap(ctx, b->up_stream, format, p.d, b->side[p.k].d, reinterpret_cast<float *>(dst), b->w, b->h, plan);
        });
}

const char *const kGainmapWantsLinear = "gain-map ingest writes linear light: it needs a linear batch (ce_batch_create_linear)";

// ce_batch_set_*_gainmap
int set_gainmap(ce_batch *b, bool test, uint32_t pair_index, uint32_t ref_index, const void *pixels, size_t len, int format, const ce_colour *c,
                const ce_gainmap_image *map, const ce_gainmap *g)
{
    ce_gainmap_plan plan;
    return set_slot(
        b, test, pair_index, ref_index, kind_rule{false, kGainmapWantsLinear},
        [&] { return gainmap_check(b->ctx, pixels, len, format, c, map, g, b->w, b->h, &plan); },
        [&](uint8_t *slot) { return upload_gainmap(b, slot, pixels, len, format, map, plan); });
}

// ce_gainmap_to_linear: through the leaf scratch on the context's stream, the tables and the map behind the base at the next
// 16-byte boundary
int gainmap_to_linear(ce_ctx *ctx, const void *pixels, size_t len, int format, const ce_colour *c, const ce_gainmap_image *map, const ce_gainmap *g,
                      uint32_t w, uint32_t h, float *out, size_t out_len)
{
    if (!ctx || !out) return CE_ERR_INVALID_ARG;
    if (w == 0 || h == 0) return ce_fail(ctx, CE_ERR_INVALID_ARG, "gain-map ingest: empty image");
    ce_gainmap_plan plan;
    if (int rc = gainmap_check(ctx, pixels, len, format, c, map, g, w, h, &plan)) return rc;
    const size_t n_px = (size_t)w * h, at = (len + 15) & ~(size_t)15, in_bytes = at + plan.table_bytes() + plan.map_bytes();
    if (out_len != n_px * 3)
        return ce_fail(ctx, CE_ERR_BAD_LENGTH, "gain-map ingest: out_len must be " + std::to_string(n_px * 3) + " floats, got " + std::to_string(out_len));
    return ce_leaf_roundtrip(
        ctx, in_bytes,
        [&](uint8_t *h_in, uint8_t *) {
            std::memcpy(h_in, pixels, len);
            gainmap_side(plan, map, h_in + at);
        },
        out, n_px * 12,
        [&](uint8_t *d_in, uint8_t *d_out) { return ce_launch_gainmap(ctx, ctx->stream, format, d_in, d_in + at, reinterpret_cast<float *>(d_out), w, h, plan); });
}

// ---- matrix/TRC ICC profiles into any batch (icc.hip) ---------------------------------------------------

// the device copy of the sRGB code thresholds of an integer slot of `depth` bits (ce_ctx::icc_thresholds)
int icc_thresholds_dev(ce_ctx *ctx, uint32_t depth, const float **out)
{
    auto it = ctx->icc_thresholds.find(depth);
    if (it == ctx->icc_thresholds.end()) {
        std::vector<float> host((size_t)1 << depth, 0.0f);  // entry 0 is not read
        ce_srgb_encode_thresholds(depth, host.data() + 1, host.size() - 1);
        CE_HIP(ctx, hipSetDevice(ctx->device));
        void *d = nullptr;
        if (int rc = ce_device_table(ctx, host.data(), host.size() * sizeof(float), "sRGB code thresholds", &d)) return rc;
        it = ctx->icc_thresholds.emplace(depth, static_cast<float *>(d)).first;
    }
    *out = it->second;
    return CE_OK;
}

// the slot an ICC ingest writes: depth_out bits (0: linear light), out16: u16 samples, wide_ok: it takes 16-bit sources
struct icc_slot {
    uint32_t depth_out;
    bool out16, wide_ok;
};

// the slot kind of a batch's side
icc_slot icc_slot_of(const ce_batch *b, bool test)
{
    const uint32_t side = b->depth[test];
    return {b->linear ? 0 : side ? side : 8, side != 0, b->linear || side != 0};
}

// the plan of a checked handle for sources of `depth` bits (one of the handle's four) into `slot`: the tables of that depth,
// the matrix, the LUT stages and, for an integer slot, the thresholds of its depth, made on demand
int icc_plan(ce_ctx *ctx, const ce_icc *icc, uint32_t depth, icc_slot slot, ce_icc_pixel *plan)
{
    plan->maxv = (1u << depth) - 1u;
    plan->has_matrix = icc->has_matrix;
    for (int i = 0; i < 9; i++) plan->m[i] = icc->m[i];
    plan->depth_out = slot.depth_out, plan->out16 = slot.out16;
    if (slot.depth_out)
        if (int rc = icc_thresholds_dev(ctx, slot.depth_out, &plan->d_thr)) return rc;
    plan->d_tables = icc->d_tables[ce_icc_depth_index(depth)];
    plan->lut = icc->lut;
    return CE_OK;
}

// One image of code values with its profile for `slot`: everything refused about either, then the plan
int icc_check(ce_ctx *ctx, const void *pixels, size_t len, int format, uint32_t depth, const ce_icc *icc, size_t n_px, icc_slot slot, ce_icc_pixel *plan)
{
    if (!pixels || !icc) return ce_fail(ctx, CE_ERR_INVALID_ARG, "ICC ingest: null pointer");
    if (icc->ctx->device != ctx->device) return ce_fail(ctx, CE_ERR_INVALID_ARG, "ICC ingest: the profile and the destination are on different devices");
    const bool fmt8 = format == CE_PIXEL_RGB8 || format == CE_PIXEL_RGBA8, fmt16 = format == CE_PIXEL_RGB16 || format == CE_PIXEL_RGBA16;
    if (!fmt8 && !fmt16) return ce_fail(ctx, CE_ERR_INVALID_ARG, "ICC ingest: format must be CE_PIXEL_RGB8, RGBA8, RGB16 or RGBA16");
    if (!ce_deep_depth_ok(depth)) return ce_fail(ctx, CE_ERR_INVALID_ARG, "ICC ingest: depth must be 8, 10, 12 or 16, got " + std::to_string(depth));
    if (fmt8 && depth != 8) return ce_fail(ctx, CE_ERR_INVALID_ARG, "ICC ingest: an 8-bit format needs depth 8, got " + std::to_string(depth));
    if (fmt16 && !slot.wide_ok)
        return ce_fail(ctx, CE_ERR_INVALID_ARG, "ICC ingest: an RGB8 batch takes CE_PIXEL_RGB8 / RGBA8; 16-bit samples need a deep or a linear batch");
    if (len != n_px * ce_pixel_bytes(format)) return ce_bad_length(ctx, n_px * ce_pixel_bytes(format), len);
    return icc_plan(ctx, icc, depth, slot, plan);
}

// ce_batch_set_*_icc
int set_icc(ce_batch *b, bool test, uint32_t pair_index, uint32_t ref_index, const void *pixels, size_t len, int format, uint32_t depth, const ce_icc *icc)
{
    if (!b) return CE_ERR_INVALID_ARG;
    ce_icc_pixel plan;
    return set_slot(
        b, test, pair_index, ref_index, kind_rule{},
        [&] { return icc_check(b->ctx, pixels, len, format, depth, icc, (size_t)b->w * b->h, icc_slot_of(b, test), &plan); },
        [&](uint8_t *slot) {
            return wide_send(b, len, packed_fill(pixels, len), [&](const wide_pair &p) {
                return ce_launch_icc(b->ctx, b->up_stream, format, p.d, slot, (size_t)b->w * b->h, plan);
            });
        });
}

// ce_icc_to_linear (depth_out = 0), ce_icc_to_srgb8 and ce_icc_to_srgb16: one image -> host memory through the leaf scratch
int icc_to_host(ce_ctx *ctx, const void *pixels, size_t len, int format, uint32_t depth, const ce_icc *icc, uint32_t w, uint32_t h, uint32_t depth_out,
                bool out16, void *out, size_t out_len)
{
    if (!ctx) return CE_ERR_INVALID_ARG;
    if (!out) return ce_fail(ctx, CE_ERR_INVALID_ARG, "ICC ingest: null output");
    if (w == 0 || h == 0) return ce_fail(ctx, CE_ERR_INVALID_ARG, "ICC ingest: empty image");
    if (out16 && !ce_deep_depth_ok(depth_out))
        return ce_fail(ctx, CE_ERR_INVALID_ARG, "ICC ingest: the output depth must be 8, 10, 12 or 16 bits, got " + std::to_string(depth_out));
    const size_t n_px = (size_t)w * h;
    ce_icc_pixel plan;
    if (int rc = icc_check(ctx, pixels, len, format, depth, icc, n_px, icc_slot{depth_out, out16, true}, &plan)) return rc;
    if (out_len != n_px * 3)
        return ce_fail(ctx, CE_ERR_BAD_LENGTH, "ICC ingest: out_len must be " + std::to_string(n_px * 3) + " samples, got " + std::to_string(out_len));
    const size_t sample = depth_out == 0 ? sizeof(float) : out16 ? 2 : 1;
    return ce_leaf_roundtrip(ctx, pixels, len, out, n_px * 3 * sample,
                             [&](uint8_t *d_in, uint8_t *d_out) { return ce_launch_icc(ctx, ctx->stream, format, d_in, d_out, n_px, plan); });
}

// ---- planar Y'CbCr (yuv.hip), and with a description into a linear batch (yuv_cicp.hip) -------------------

// a checked ce_yuv_image: what the kernel reads, and each plane's rows for the host copy
struct yuv_plan {
    ce_yuv_dev dev{};
    int n_planes = 0;
    size_t rows[3] = {}, row_bytes[3] = {};
    size_t offset[3] = {}, total = 0;  // the planes packed without pitch padding, each at an even offset
};

int yuv_check(ce_ctx *ctx, const ce_yuv_image *img, uint32_t w, uint32_t h, uint32_t depth_out, yuv_plan *plan)
{
    if (!img) return ce_fail(ctx, CE_ERR_INVALID_ARG, "Y'CbCr ingest: null image");
    if (img->subsampling < CE_YUV_444 || img->subsampling > CE_YUV_400)
        return ce_fail(ctx, CE_ERR_INVALID_ARG, "Y'CbCr ingest: unknown subsampling " + std::to_string(img->subsampling));
    if (img->layout != CE_YUV_PLANAR && img->layout != CE_YUV_SEMIPLANAR)
        return ce_fail(ctx, CE_ERR_INVALID_ARG, "Y'CbCr ingest: unknown layout " + std::to_string(img->layout));
    if (img->upsample != CE_CHROMA_NEAREST && img->upsample != CE_CHROMA_TRIANGLE)
        return ce_fail(ctx, CE_ERR_INVALID_ARG, "Y'CbCr ingest: unknown chroma upsampling " + std::to_string(img->upsample));
    if (img->memory != CE_MEM_HOST && img->memory != CE_MEM_DEVICE)
        return ce_fail(ctx, CE_ERR_INVALID_ARG, "Y'CbCr ingest: unknown memory kind " + std::to_string(img->memory));
    if (img->depth != 8 && img->depth != 10 && img->depth != 12)
        return ce_fail(ctx, CE_ERR_INVALID_ARG, "Y'CbCr ingest: depth must be 8, 10 or 12 bits, got " + std::to_string(img->depth));
    if (img->msb_aligned && img->depth == 8) return ce_fail(ctx, CE_ERR_INVALID_ARG, "Y'CbCr ingest: msb_aligned is for u16 samples, not depth 8");
    if (img->lut) return ce_fail(ctx, CE_ERR_INVALID_ARG, "Y'CbCr ingest: a colour table is 2^24 RGB colours and is not offered for YUV");
    ce_yuv_dev &d = plan->dev;
    if (ce_yuv_coefficients(img->matrix, img->range, (uint32_t)img->depth, depth_out, d.k) != CE_OK)
        return ce_fail(ctx, CE_ERR_INVALID_ARG, "Y'CbCr ingest: unknown matrix " + std::to_string(img->matrix) + " or range " + std::to_string(img->range));
    const size_t bps = img->depth == 8 ? 1 : 2;
    const size_t cw = img->subsampling == CE_YUV_444 ? w : ((size_t)w + 1) / 2, ch = img->subsampling == CE_YUV_420 ? ((size_t)h + 1) / 2 : h;
    const bool semi = img->layout == CE_YUV_SEMIPLANAR;
    plan->n_planes = img->subsampling == CE_YUV_400 ? 1 : semi ? 2 : 3;
    for (int p = 0; p < plan->n_planes; p++) {
        plan->rows[p] = p == 0 ? h : ch;
        plan->row_bytes[p] = (p == 0 ? (size_t)w : semi ? 2 * cw : cw) * bps;
        if (!img->plane[p]) return ce_fail(ctx, CE_ERR_INVALID_ARG, "Y'CbCr ingest: plane " + std::to_string(p) + " is missing");
        if (img->pitch[p] < plan->row_bytes[p])
            return ce_fail(ctx, CE_ERR_INVALID_ARG, "Y'CbCr ingest: pitch " + std::to_string(img->pitch[p]) + " of plane " + std::to_string(p) +
                                                        " is under its row's " + std::to_string(plan->row_bytes[p]) + " bytes");
        if (bps == 2 && ((reinterpret_cast<uintptr_t>(img->plane[p]) | img->pitch[p]) & 1))
            return ce_fail(ctx, CE_ERR_INVALID_ARG, "Y'CbCr ingest: the pointer and pitch of u16 plane " + std::to_string(p) + " must be 2-byte aligned");
        plan->offset[p] = plan->total;
        plan->total += (plan->rows[p] * plan->row_bytes[p] + 1) & ~(size_t)1;
        d.plane[p] = static_cast<const uint8_t *>(img->plane[p]);
        d.pitch[p] = img->pitch[p];
    }
    d.subsampling = img->subsampling, d.layout = img->layout, d.upsample = img->upsample;
    d.depth = (uint32_t)img->depth;
    d.shift = img->msb_aligned ? 16u - (uint32_t)img->depth : 0u;
    return CE_OK;
}

// everything *_yuv refuses about the image and *_cicp / *_hlg about the description, and their one joint rule: the integer
// RGB grid between the two halves (d->depth) is no coarser than the samples
template <class Desc>
int yuv_tagged_check(ce_ctx *ctx, const ce_yuv_image *img, const Desc *d, uint32_t w, uint32_t h, yuv_plan *plan, ce_linear_pixel *lin)
{
    const route_words rw = words(d);
    if (!img) return ce_fail(ctx, CE_ERR_INVALID_ARG, "Y'CbCr ingest: null image");
    if (!d) return ce_fail(ctx, CE_ERR_INVALID_ARG, std::string(rw.name) + " ingest: null pointer");
    if (int rc = colour_check(ctx, d, lin)) return rc;
    if (int rc = yuv_check(ctx, img, w, h, d->depth, plan)) return rc;
    if (d->depth < (uint32_t)img->depth)
        return ce_fail(ctx, CE_ERR_INVALID_ARG, std::string("Y'CbCr ") + rw.name + " ingest: the " + rw.depth_owner + " depth " + std::to_string(d->depth) +
                                                    " is under the samples' " + std::to_string(img->depth) + " bits");
    return table_dev(ctx, d, lin);
}

// host planes -> `h_stage` without their pitch padding; the device copy at d_stage is what the kernel then reads
void yuv_pack(const ce_yuv_image *img, yuv_plan *plan, uint8_t *h_stage, const uint8_t *d_stage)
{
    for (int p = 0; p < plan->n_planes; p++) {
        const uint8_t *src = static_cast<const uint8_t *>(img->plane[p]);
        uint8_t *dst = h_stage + plan->offset[p];
        for (size_t r = 0; r < plan->rows[p]; r++) std::memcpy(dst + r * plan->row_bytes[p], src + r * img->pitch[p], plan->row_bytes[p]);
        plan->dev.plane[p] = d_stage + plan->offset[p];
        plan->dev.pitch[p] = plan->row_bytes[p];
    }
}

// the conversion of one checked image into dst: integer RGB (u8, or u16 of `depth`), or with `lin` the fused linear-light
// ingest of a linear batch (yuv_cicp.hip: the CICP or the HLG pixel, as `lin` says), or with `icc` the fused ICC ingest into
// the slot its depth_out names (yuv_icc.hip); the integer grid of either is the one plan.dev.k was built for
int launch_yuv_into(ce_ctx *ctx, hipStream_t stream, const yuv_plan &plan, uint32_t w, uint32_t h, uint8_t *dst, uint32_t depth,
                    const ce_linear_pixel *lin, const ce_icc_pixel *icc = nullptr)
{
    if (icc) return ce_launch_yuv_icc(ctx, stream, plan.dev, w, h, dst, *icc);
    if (lin) return ce_launch_yuv_tagged(ctx, stream, plan.dev, w, h, reinterpret_cast<float *>(dst), *lin);
    return ce_launch_yuv(ctx, stream, plan.dev, w, h, dst, depth != 0, depth ? depth : 8);
}

// one Y'CbCr image into a slab slot on the batch's upload stream: device planes are read in place, host planes go
// through the wide staging pair (the packed planes are at most 6 bytes per pixel and a few bytes)
int upload_yuv(ce_batch *b, uint8_t *dst, const ce_yuv_image *img, yuv_plan &plan, uint32_t depth, const ce_linear_pixel *lin,
               const ce_icc_pixel *icc = nullptr)
{
    ce_ctx *ctx = b->ctx;
    auto launch = [&] { return launch_yuv_into(ctx, b->up_stream, plan, b->w, b->h, dst, depth, lin, icc); };
    if (img->memory == CE_MEM_DEVICE) {
        CE_HIP(ctx, hipSetDevice(ctx->device));
        if (int rc = ce_order_write(b, false)) return rc;
        if (int rc = launch()) return rc;
        b->uploads_pending = true;
        return CE_OK;
    }
    // 8 bytes per pixel on a linear batch too, whose pairs hold 16
    if (plan.total > (size_t)b->w * b->h * 8) return ce_fail(ctx, CE_ERR_INVALID_ARG, "Y'CbCr ingest: the packed planes do not fit the staging buffer");
    return wide_send(
        b, plan.total,
        [&](const wide_pair &p) {
            yuv_pack(img, &plan, p.h, p.d);
            return CE_OK;
        },
        [&](const wide_pair &) { return launch(); });
}

// one checked image -> host memory through the leaf scratch, on the context's stream; depth, lin and icc as launch_yuv_into's
int yuv_leaf(ce_ctx *ctx, const ce_yuv_image *image, yuv_plan &plan, uint32_t w, uint32_t h, uint32_t depth, const ce_linear_pixel *lin, void *out,
             size_t out_bytes, const ce_icc_pixel *icc = nullptr)
{
    const bool host = image->memory == CE_MEM_HOST;  // device planes are read in place: nothing goes in
    return ce_leaf_roundtrip(
        ctx, host ? plan.total : 0,
        [&](uint8_t *h_in, uint8_t *d_in) {
            if (host) yuv_pack(image, &plan, h_in, d_in);
        },
        out, out_bytes, [&](uint8_t *, uint8_t *d_out) { return launch_yuv_into(ctx, ctx->stream, plan, w, h, d_out, depth, lin, icc); });
}

// ce_yuv_to_rgb8 (out16 = false, depth_out = 8) and ce_yuv_to_rgb16
int yuv_to_host(ce_ctx *ctx, const ce_yuv_image *image, uint32_t w, uint32_t h, bool out16, uint32_t depth_out, void *out, size_t out_len)
{
    if (!ctx) return CE_ERR_INVALID_ARG;
    if (!out) return ce_fail(ctx, CE_ERR_INVALID_ARG, "Y'CbCr ingest: null output");
    if (w == 0 || h == 0) return ce_fail(ctx, CE_ERR_INVALID_ARG, "Y'CbCr ingest: empty image");
    if (out16 && !ce_deep_depth_ok(depth_out))
        return ce_fail(ctx, CE_ERR_INVALID_ARG, "Y'CbCr ingest: the output depth must be 8, 10, 12 or 16 bits, got " + std::to_string(depth_out));
    yuv_plan plan;
    if (int rc = yuv_check(ctx, image, w, h, depth_out, &plan)) return rc;
    const size_t samples = (size_t)w * h * 3;
    if (out_len != samples)
        return ce_fail(ctx, CE_ERR_BAD_LENGTH, "Invalid image size: expected " + std::to_string(samples) + " samples, got " + std::to_string(out_len));
    return yuv_leaf(ctx, image, plan, w, h, out16 ? depth_out : 0, nullptr, out, samples * (out16 ? 2 : 1));
}

// ce_yuv_to_linear and ce_yuv_hlg_to_linear
template <class Desc>
int yuv_to_linear(ce_ctx *ctx, const ce_yuv_image *image, const Desc *d, uint32_t w, uint32_t h, float *out, size_t out_len)
{
    if (!ctx) return CE_ERR_INVALID_ARG;
    if (!out) return ce_fail(ctx, CE_ERR_INVALID_ARG, "Y'CbCr ingest: null output");
    if (w == 0 || h == 0) return ce_fail(ctx, CE_ERR_INVALID_ARG, "Y'CbCr ingest: empty image");
    yuv_plan plan;
    ce_linear_pixel lin;
    if (int rc = yuv_tagged_check(ctx, image, d, w, h, &plan, &lin)) return rc;
    const size_t samples = (size_t)w * h * 3;
    if (out_len != samples)
        return ce_fail(ctx, CE_ERR_BAD_LENGTH, std::string("Y'CbCr ") + words(d).name + " ingest: out_len must be " + std::to_string(samples) +
                                                   " floats, got " + std::to_string(out_len));
    return yuv_leaf(ctx, image, plan, w, h, 0, &lin, out, samples * sizeof(float));
}

const char *const kYuvLinear = "Y'CbCr ingest writes integer RGB: a linear batch takes planes through ce_batch_set_*_yuv_cicp";
const char *const kYuvCicpWantsLinear =
    "Y'CbCr CICP ingest writes linear light: it needs a linear batch (ce_batch_create_linear); ce_batch_set_*_yuv serves the others";

// ce_batch_set_*_yuv
int set_yuv(ce_batch *b, bool test, uint32_t pair_index, uint32_t ref_index, const ce_yuv_image *image)
{
    yuv_plan plan;
    return set_slot(
        b, test, pair_index, ref_index, kind_rule{true, kYuvLinear},
        [&] { return yuv_check(b->ctx, image, b->w, b->h, b->depth[test] ? b->depth[test] : 8, &plan); },
        [&](uint8_t *slot) { return upload_yuv(b, slot, image, plan, b->depth[test], nullptr); });
}

// ce_batch_set_*_yuv_cicp and ce_batch_set_*_yuv_hlg
template <class Desc>
int set_yuv_tagged(ce_batch *b, bool test, uint32_t pair_index, uint32_t ref_index, const ce_yuv_image *image, const Desc *d, const char *wants_linear)
{
    yuv_plan plan;
    ce_linear_pixel lin;
    return set_slot(
        b, test, pair_index, ref_index, kind_rule{false, wants_linear},
        [&] { return yuv_tagged_check(b->ctx, image, d, b->w, b->h, &plan, &lin); },
        [&](uint8_t *slot) { return upload_yuv(b, slot, image, plan, 0, &lin); });
}

// ---- Y'CbCr planes with an ICC profile into any batch (yuv_icc.hip) ----------------------------------------

// everything *_yuv refuses about the image and *_icc about the handle, and their joint rule: the integer RGB grid between the
// two halves (rgb_depth) is one of the handle's four and no coarser than the samples
int yuv_icc_check(ce_ctx *ctx, const ce_yuv_image *img, uint32_t rgb_depth, const ce_icc *icc, uint32_t w, uint32_t h, icc_slot slot, yuv_plan *plan,
                  ce_icc_pixel *px)
{
    if (!img) return ce_fail(ctx, CE_ERR_INVALID_ARG, "Y'CbCr ingest: null image");
    if (!icc) return ce_fail(ctx, CE_ERR_INVALID_ARG, "ICC ingest: null pointer");
    if (icc->ctx->device != ctx->device) return ce_fail(ctx, CE_ERR_INVALID_ARG, "ICC ingest: the profile and the destination are on different devices");
    if (!ce_deep_depth_ok(rgb_depth))
        return ce_fail(ctx, CE_ERR_INVALID_ARG, "Y'CbCr ICC ingest: rgb_depth must be 8, 10, 12 or 16, got " + std::to_string(rgb_depth));
    if (int rc = yuv_check(ctx, img, w, h, rgb_depth, plan)) return rc;
    if (rgb_depth < (uint32_t)img->depth)
        return ce_fail(ctx, CE_ERR_INVALID_ARG, "Y'CbCr ICC ingest: rgb_depth " + std::to_string(rgb_depth) + " is under the samples' " +
                                                    std::to_string(img->depth) + " bits");
    return icc_plan(ctx, icc, rgb_depth, slot, px);
}

// ce_batch_set_*_yuv_icc: set_yuv's frame around the fused launch, into a linear, an RGB8 or a deep batch
int set_yuv_icc(ce_batch *b, bool test, uint32_t pair_index, uint32_t ref_index, const ce_yuv_image *image, uint32_t rgb_depth, const ce_icc *icc)
{
    if (!b) return CE_ERR_INVALID_ARG;
    yuv_plan plan;
    ce_icc_pixel px;
    return set_slot(
        b, test, pair_index, ref_index, kind_rule{},
        [&] { return yuv_icc_check(b->ctx, image, rgb_depth, icc, b->w, b->h, icc_slot_of(b, test), &plan, &px); },
        [&](uint8_t *slot) { return upload_yuv(b, slot, image, plan, 0, nullptr, &px); });
}

// ce_yuv_icc_to_linear (depth_out = 0), ce_yuv_icc_to_srgb8 and ce_yuv_icc_to_srgb16: one image -> host memory through the leaf scratch
int yuv_icc_to_host(ce_ctx *ctx, const ce_yuv_image *image, uint32_t rgb_depth, const ce_icc *icc, uint32_t w, uint32_t h, uint32_t depth_out, bool out16,
                    void *out, size_t out_len)
{
    if (!ctx) return CE_ERR_INVALID_ARG;
    if (!out) return ce_fail(ctx, CE_ERR_INVALID_ARG, "Y'CbCr ICC ingest: null output");
    if (w == 0 || h == 0) return ce_fail(ctx, CE_ERR_INVALID_ARG, "Y'CbCr ICC ingest: empty image");
    if (out16 && !ce_deep_depth_ok(depth_out))
        return ce_fail(ctx, CE_ERR_INVALID_ARG, "Y'CbCr ICC ingest: the output depth must be 8, 10, 12 or 16 bits, got " + std::to_string(depth_out));
    yuv_plan plan;
    ce_icc_pixel px;
    if (int rc = yuv_icc_check(ctx, image, rgb_depth, icc, w, h, icc_slot{depth_out, out16, true}, &plan, &px)) return rc;
    const size_t samples = (size_t)w * h * 3;
    if (out_len != samples)
        return ce_fail(ctx, CE_ERR_BAD_LENGTH, "Y'CbCr ICC ingest: out_len must be " + std::to_string(samples) + " samples, got " + std::to_string(out_len));
    return yuv_leaf(ctx, image, plan, w, h, 0, nullptr, out, samples * (depth_out == 0 ? sizeof(float) : out16 ? 2 : 1), &px);
}

// ---- strided tensors of a framework (tensor.hip) ---------------------------------------------------------

// the slot kinds of ce_launch_tensor
enum { kTensorSlotU8 = 0, kTensorSlotU16 = 1, kTensorSlotLin = 2 };

// the slot kind a batch's side gives a tensor, and its depth (read for u16 slots)
struct tensor_slot {
    int kind;
    uint32_t depth;
};
tensor_slot tensor_slot_of(const ce_batch *b, bool test)
{
    return b->linear ? tensor_slot{kTensorSlotLin, 0} : b->depth[test] ? tensor_slot{kTensorSlotU16, b->depth[test]} : tensor_slot{kTensorSlotU8, 8};
}

// a checked ce_tensor_image: what the kernel reads in place, and for a host source what one image takes in staging
struct tensor_plan {
    ce_tensor_dev dev{};
    size_t es = 0;           // bytes per element
    bool interleaved = false;  // host: rows are runs of whole pixels (stride_c = 1, stride_x 3 or 4), else of one plane's elements
    size_t stage_bytes = 0;  // host: one image in staging
};

int tensor_check(ce_ctx *ctx, const ce_tensor_image *t, uint32_t w, uint32_t h, uint32_t count, tensor_slot slot, tensor_plan *plan)
{
    const std::string route = "tensor ingest: ";
    if (!t || !t->data) return ce_fail(ctx, CE_ERR_INVALID_ARG, route + "null pointer");
    if (t->dtype < CE_DTYPE_U8 || t->dtype > CE_DTYPE_F32) return ce_fail(ctx, CE_ERR_INVALID_ARG, route + "unknown dtype " + std::to_string(t->dtype));
    if (t->memory != CE_MEM_HOST && t->memory != CE_MEM_DEVICE)
        return ce_fail(ctx, CE_ERR_INVALID_ARG, route + "unknown memory kind " + std::to_string(t->memory));
    if (t->quantise != CE_QUANT_NEAREST_EVEN && t->quantise != CE_QUANT_TRUNCATE)
        return ce_fail(ctx, CE_ERR_INVALID_ARG, route + "unknown quantise rule " + std::to_string(t->quantise));
    const bool integer = t->dtype == CE_DTYPE_U8 || t->dtype == CE_DTYPE_U16;
    if (t->quantise != 0 && (integer || slot.kind == kTensorSlotLin))
        return ce_fail(ctx, CE_ERR_INVALID_ARG, route + "quantise is for float dtypes into integer slots: it must be 0 here");
    if (t->stride_n < 0 || t->stride_c < 0 || t->stride_y < 0 || t->stride_x < 0) return ce_fail(ctx, CE_ERR_INVALID_ARG, route + "negative stride");
    if (t->stride_x < 1 || t->stride_y < 1) return ce_fail(ctx, CE_ERR_INVALID_ARG, route + "stride_x and stride_y must be at least 1");
    const size_t es = t->dtype == CE_DTYPE_U8 ? 1 : t->dtype == CE_DTYPE_F32 ? 4 : 2;
    if (reinterpret_cast<uintptr_t>(t->data) % es)
        return ce_fail(ctx, CE_ERR_INVALID_ARG, route + "the data pointer is not aligned to its " + std::to_string(es) + "-byte elements");
    const unsigned __int128 last = (unsigned __int128)(count ? count - 1 : 0) * (uint64_t)t->stride_n + (unsigned __int128)2 * (uint64_t)t->stride_c +
                                   (unsigned __int128)(h ? h - 1 : 0) * (uint64_t)t->stride_y + (unsigned __int128)(w ? w - 1 : 0) * (uint64_t)t->stride_x;
    if ((last + 1) * es > (unsigned __int128)INT64_MAX) return ce_fail(ctx, CE_ERR_INVALID_ARG, route + "the tensor's extent overflows size_t");
    if (t->dtype == CE_DTYPE_U8 && slot.kind == kTensorSlotU16 && slot.depth != 8)
        return ce_fail(ctx, CE_ERR_INVALID_ARG, route + "an 8-bit tensor needs a side of depth 8, this one has " + std::to_string(slot.depth));
    if (t->dtype == CE_DTYPE_U16 && slot.kind == kTensorSlotU8)
        return ce_fail(ctx, CE_ERR_INVALID_ARG, route + "CE_DTYPE_U16 needs a deep batch (ce_batch_create_deep)");
    if (integer && slot.kind == kTensorSlotLin)
        return ce_fail(ctx, CE_ERR_INVALID_ARG, route + "a linear batch takes float tensors, which are linear light; integer code values go through ce_batch_set_*_cicp");
    if (count == 0 || count > 65535u) return ce_fail(ctx, CE_ERR_INVALID_ARG, route + "count must be 1 to 65535, got " + std::to_string(count));
    plan->es = es;
    plan->dev = ce_tensor_dev{t->data, t->stride_n, t->stride_c, t->stride_y, t->stride_x, t->dtype, t->quantise};
    if (t->memory == CE_MEM_HOST) {
        plan->interleaved = t->stride_x != 1;
        if (plan->interleaved && !(t->stride_c == 1 && (t->stride_x == 3 || t->stride_x == 4)))
            return ce_fail(ctx, CE_ERR_INVALID_ARG, route + "a host tensor's rows must be contiguous runs (stride_x = 1, or stride_c = 1 with stride_x 3 or 4): "
                                                            "make it contiguous or pass device memory");
        plan->stage_bytes = (size_t)w * h * es * (plan->interleaved ? (size_t)t->stride_x : t->stride_c == 0 ? 1 : 3);
    }
    return CE_OK;
}

// image n of a checked host tensor -> `h_stage`, its rows as they are, one after another; what the kernel then reads at d_stage
ce_tensor_dev tensor_stage(const tensor_plan &plan, uint32_t n, uint32_t w, uint32_t h, uint8_t *h_stage, const uint8_t *d_stage)
{
    const ce_tensor_dev &s = plan.dev;
    const size_t es = plan.es;
    const uint8_t *img = static_cast<const uint8_t *>(s.data) + (size_t)n * (size_t)s.stride_n * es;
    ce_tensor_dev d = s;
    d.data = d_stage, d.stride_n = 0;
    if (plan.interleaved) {
        // the last pixel's run ends with its third channel: a fourth one behind it need not exist
        const size_t row = (size_t)w * (size_t)s.stride_x * es, run = ((size_t)(w - 1) * (size_t)s.stride_x + 3) * es;
        for (size_t y = 0; y < h; y++) std::memcpy(h_stage + y * row, img + y * (size_t)s.stride_y * es, run);
        d.stride_y = (int64_t)w * s.stride_x;
        return d;
    }
    const size_t row = (size_t)w * es;
    for (size_t c = 0; c < (s.stride_c == 0 ? 1u : 3u); c++)
        for (size_t y = 0; y < h; y++)
            std::memcpy(h_stage + (c * h + y) * row, img + (c * (size_t)s.stride_c + y * (size_t)s.stride_y) * es, row);
    d.stride_c = s.stride_c == 0 ? 0 : (int64_t)w * h, d.stride_y = w;
    return d;
}

// `count` checked images into consecutive slots from dst on, on the batch's upload stream.  A device tensor is read in place by
// one launch, ordered as every slot write and - this source alone - behind what the context's stream holds at this point, so
// that a model running on that stream needs no host synchronisation; host images go one by one through the wide staging pair.
int upload_tensor(ce_batch *b, uint8_t *dst, const ce_tensor_image *t, const tensor_plan &plan, uint32_t count, tensor_slot slot)
{
    ce_ctx *ctx = b->ctx;
    if (t->memory == CE_MEM_DEVICE) {
        CE_HIP(ctx, hipSetDevice(ctx->device));
        if (int rc = ce_order_write(b, false)) return rc;
        CE_HIP(ctx, hipEventRecord(b->ev_up, ctx->stream));
        CE_HIP(ctx, hipStreamWaitEvent(b->up_stream, b->ev_up, 0));
        if (int rc = ce_launch_tensor(ctx, b->up_stream, plan.dev, b->w, b->h, count, dst, b->img_bytes, slot.kind, slot.depth)) return rc;
        b->uploads_pending = true;
        return CE_OK;
    }
    for (uint32_t n = 0; n < count; n++) {
        ce_tensor_dev staged{};
        const int rc = wide_send(
            b, plan.stage_bytes,
            [&](const wide_pair &p) {
                staged = tensor_stage(plan, n, b->w, b->h, p.h, p.d);
                return CE_OK;
            },
            [&](const wide_pair &) {
                return ce_launch_tensor(ctx, b->up_stream, staged, b->w, b->h, 1, dst + (size_t)n * b->img_bytes, b->img_bytes, slot.kind, slot.depth);
            });
        if (rc != CE_OK) return rc;
    }
    return CE_OK;
}

// ce_batch_set_*_tensor
int set_tensor(ce_batch *b, bool test, uint32_t first, const uint32_t *ref_indices, uint32_t count, const ce_tensor_image *t)
{
    tensor_plan plan;
    return set_slots(
        b, test, first, count, ref_indices, "tensor ingest: ", kind_rule{}, !t || !t->data,
        [&] { return tensor_check(b->ctx, t, b->w, b->h, count, tensor_slot_of(b, test), &plan); },
        [&](uint8_t *dst) { return upload_tensor(b, dst, t, plan, count, tensor_slot_of(b, test)); });
}

// ce_tensor_to_rgb8 / _to_rgb16 / _to_linear: image 0 -> host memory through the leaf scratch, on the context's stream
int tensor_to_host(ce_ctx *ctx, const ce_tensor_image *t, uint32_t w, uint32_t h, tensor_slot slot, void *out, size_t out_len)
{
    if (!ctx) return CE_ERR_INVALID_ARG;
    if (!out) return ce_fail(ctx, CE_ERR_INVALID_ARG, "tensor ingest: null output");
    if (w == 0 || h == 0) return ce_fail(ctx, CE_ERR_INVALID_ARG, "tensor ingest: empty image");
    if (slot.kind == kTensorSlotU16 && !ce_deep_depth_ok(slot.depth))
        return ce_fail(ctx, CE_ERR_INVALID_ARG, "tensor ingest: the output depth must be 8, 10, 12 or 16 bits, got " + std::to_string(slot.depth));
    tensor_plan plan;
    if (int rc = tensor_check(ctx, t, w, h, 1, slot, &plan)) return rc;
    const size_t samples = (size_t)w * h * 3, out_bytes = samples * (slot.kind == kTensorSlotU8 ? 1 : slot.kind == kTensorSlotU16 ? 2 : 4);
    if (out_len != samples)
        return ce_fail(ctx, CE_ERR_BAD_LENGTH, "tensor ingest: out_len must be " + std::to_string(samples) + " samples, got " + std::to_string(out_len));
    const bool host = t->memory == CE_MEM_HOST;  // a device tensor is read in place: nothing goes in
    ce_tensor_dev src = plan.dev;
    return ce_leaf_roundtrip(
        ctx, host ? plan.stage_bytes : 0,
        [&](uint8_t *h_in, uint8_t *d_in) {
            if (host) src = tensor_stage(plan, 0, w, h, h_in, d_in);
        },
        out, out_bytes, [&](uint8_t *, uint8_t *d_out) { return ce_launch_tensor(ctx, ctx->stream, src, w, h, 1, d_out, out_bytes, slot.kind, slot.depth); });
}

// ---- alpha: composited over solid backgrounds (alpha.hip) -------------------------------------------------------------------

int alpha_backgrounds_ok(ce_ctx *ctx, uint32_t n_bg, const uint16_t *backgrounds, uint32_t depth)
{
    if (n_bg == 0 || n_bg > CE_MAX_BACKGROUNDS)
        return ce_fail(ctx, CE_ERR_INVALID_ARG, "alpha compositing: 1 to " + std::to_string(CE_MAX_BACKGROUNDS) + " backgrounds, got " + std::to_string(n_bg));
    const uint32_t m = (1u << depth) - 1u;
    for (uint32_t i = 0; i < 3 * n_bg; i++)
        if (backgrounds[i] > m)
            return ce_fail(ctx, CE_ERR_INVALID_ARG, "alpha compositing: background sample " + std::to_string(backgrounds[i]) + " is above " + std::to_string(m));
    return CE_OK;
}

// the checks of one ce_batch_set_*_over call that do not depend on the slots; depth = that side's (0: an RGB8 batch)
int alpha_check(ce_batch *b, size_t len, int format, uint32_t n_bg, const uint16_t *backgrounds, uint32_t depth)
{
    ce_ctx *ctx = b->ctx;
    if (b->linear) return ce_fail(ctx, CE_ERR_INVALID_ARG, "alpha compositing works on encoded integer samples: not for a linear batch");
    if (format != CE_PIXEL_RGBA8 && format != CE_PIXEL_RGBA16)
        return ce_fail(ctx, CE_ERR_INVALID_ARG, format == CE_PIXEL_RGBA16_10BIT ? "alpha compositing: CE_PIXEL_RGBA16_10BIT rounds to 8 bits; a deep batch takes 10-bit alpha as CE_PIXEL_RGBA16"
                                                                                 : "alpha compositing: the format must be CE_PIXEL_RGBA8 or CE_PIXEL_RGBA16");
    if (!depth && format == CE_PIXEL_RGBA16) return ce_fail(ctx, CE_ERR_INVALID_ARG, "alpha compositing: CE_PIXEL_RGBA16 needs a deep batch (ce_batch_create_deep)");
    if (depth && depth != 8 && format == CE_PIXEL_RGBA8)
        return ce_fail(ctx, CE_ERR_INVALID_ARG, "alpha compositing: an 8-bit image needs a side of depth 8, this one has " + std::to_string(depth));
    const size_t want = (size_t)b->w * b->h * ce_pixel_bytes(format);
    if (len != want)
        return ce_fail(ctx, CE_ERR_INVALID_ARG, "alpha compositing: expected " + std::to_string(want) + " bytes, got " + std::to_string(len));
    return alpha_backgrounds_ok(ctx, n_bg, backgrounds, depth ? depth : 8);
}

// one RGBA image through the wide staging pair into n_bg consecutive slots from dst on
int upload_over(ce_batch *b, uint8_t *dst, const void *pixels, size_t len, int format, uint32_t depth, uint32_t n_bg, const uint16_t *backgrounds)
{
    return wide_send(b, len, packed_fill(pixels, len), [&](const wide_pair &p) {
        return ce_launch_alpha(b->ctx, b->up_stream, p.d, format == CE_PIXEL_RGBA16, dst, depth != 0, depth ? depth : 8, (size_t)b->w * b->h, n_bg, backgrounds);
    });
}

// ce_batch_set_*_over (a linear batch is refused behind a null pointer, by alpha_check)
int set_over(ce_batch *b, bool test, uint32_t first, const uint32_t *ref_indices, const void *pixels, size_t len, int format, uint32_t n_bg,
             const uint16_t *backgrounds)
{
    return set_slots(
        b, test, first, n_bg, ref_indices, "alpha compositing: ", kind_rule{}, !pixels || !backgrounds,
        [&] { return alpha_check(b, len, format, n_bg, backgrounds, b->depth[test]); },
        [&](uint8_t *dst) { return upload_over(b, dst, pixels, len, format, b->depth[test], n_bg, backgrounds); });
}

// one image over one colour -> host memory through the leaf scratch, on the context's stream
int composite_to_host(ce_ctx *ctx, const void *rgba, size_t len, uint32_t w, uint32_t h, bool deep, uint32_t depth, const uint16_t bg[3], void *out,
                      size_t out_len)
{
    if (!ctx) return CE_ERR_INVALID_ARG;
    if (!rgba || !bg || !out) return ce_fail(ctx, CE_ERR_INVALID_ARG, "alpha compositing: null pointer");
    if (!ce_deep_depth_ok(depth)) return ce_fail(ctx, CE_ERR_INVALID_ARG, "alpha compositing: depth must be 8, 10, 12 or 16 bits, got " + std::to_string(depth));
    const size_t n_px = (size_t)w * h;
    if (len != n_px * 4 || out_len != n_px * 3)
        return ce_fail(ctx, CE_ERR_INVALID_ARG, "alpha compositing: expected " + std::to_string(n_px * 4) + " samples in and " + std::to_string(n_px * 3) +
                                                    " out, got " + std::to_string(len) + " and " + std::to_string(out_len));
    if (int rc = alpha_backgrounds_ok(ctx, 1, bg, depth)) return rc;
    if (n_px == 0) return CE_OK;
    const size_t bps = deep ? 2 : 1;
    return ce_leaf_roundtrip(ctx, rgba, len * bps, out, out_len * bps, [&](uint8_t *d_in, uint8_t *d_out) {
        return ce_launch_alpha(ctx, ctx->stream, d_in, deep, d_out, deep, depth, n_px, 1, bg);
    });
}

// ---- alpha in linear light: blended over solid backgrounds behind the pixel (over_linear_kernel.h) -------

// ce_alpha_table: atab[k] = float32(k) / float32(m), one correctly rounded f32 division each
void build_alpha_table(uint32_t depth, float *out)
{
    const uint32_t m = (1u << depth) - 1u;
    const float fm = (float)m;
    for (uint32_t k = 0; k <= m; k++) out[k] = (float)k / fm;
}

// the device copy of the alpha table of a source depth (ce_ctx::alpha_tables)
int alpha_table_dev(ce_ctx *ctx, uint32_t depth, const float **out)
{
    auto it = ctx->alpha_tables.find(depth);
    if (it == ctx->alpha_tables.end()) {
        std::vector<float> host((size_t)1 << depth);
        build_alpha_table(depth, host.data());
        CE_HIP(ctx, hipSetDevice(ctx->device));
        void *d = nullptr;
        if (int rc = ce_device_table(ctx, host.data(), host.size() * sizeof(float), "alpha table", &d)) return rc;
        it = ctx->alpha_tables.emplace(depth, static_cast<float *>(d)).first;
    }
    *out = it->second;
    return CE_OK;
}

// n_bg and the backgrounds of a linear-light composite, into the plan
int over_backgrounds(ce_ctx *ctx, uint32_t n_bg, const float *backgrounds, ce_over_plan *ov)
{
    if (!backgrounds) return ce_fail(ctx, CE_ERR_INVALID_ARG, "linear-light compositing: null pointer");
    if (n_bg == 0 || n_bg > CE_MAX_BACKGROUNDS)
        return ce_fail(ctx, CE_ERR_INVALID_ARG, "linear-light compositing: 1 to " + std::to_string(CE_MAX_BACKGROUNDS) + " backgrounds, got " + std::to_string(n_bg));
    for (uint32_t i = 0; i < 3 * n_bg; i++) {
        if (!std::isfinite(backgrounds[i]) || std::fabs(backgrounds[i]) > CE_LINEAR_MAX)
            return ce_fail(ctx, CE_ERR_INVALID_ARG, "linear-light compositing: a background must be finite and within +-" + std::to_string((int)CE_LINEAR_MAX));
        ov->bg[i / 3][i % 3] = backgrounds[i];
    }
    ov->n_bg = n_bg;
    return CE_OK;
}

const char *const kOverWantsLinear = "linear-light compositing writes linear light: it needs a linear batch (ce_batch_create_linear)";

int over_format_check(ce_ctx *ctx, int format)
{
    if (format != CE_PIXEL_RGBA8 && format != CE_PIXEL_RGBA16)
        return ce_fail(ctx, CE_ERR_INVALID_ARG, "linear-light compositing: the format must be CE_PIXEL_RGBA8 or CE_PIXEL_RGBA16");
    return CE_OK;
}

// Every ce_batch_set_*_*_over call: set_slots around a route's check(ov), which holds its own refusals and fills its plan and
// the alpha table, and its launch(d_src, d_dst, ov) behind the copy of the `len` bytes at `pixels` through the wide staging pair.
template <class Check, class Launch>
int set_over_linear(ce_batch *b, bool test, uint32_t first, const uint32_t *ref_indices, const void *pixels, size_t len, uint32_t n_bg,
                    const float *backgrounds, Check check, Launch launch)
{
    ce_over_plan ov;
    return set_slots(
        b, test, first, n_bg, ref_indices, "linear-light compositing: ", kind_rule{false, kOverWantsLinear}, !pixels || !backgrounds,
        [&]() -> int {
            if (int rc = check(&ov)) return rc;
            return over_backgrounds(b->ctx, n_bg, backgrounds, &ov);
        },
        [&](uint8_t *dst) {
            ov.slot_floats = (size_t)b->w * b->h * 3;
            return wide_send(b, len, packed_fill(pixels, len),
                             [&](const wide_pair &p) { return launch(b->up_stream, p.d, reinterpret_cast<float *>(dst), ov); });
        });
}

// One image over one background -> packed f32 RGB in host memory, through the leaf scratch on the context's stream
template <class Check, class Launch>
int over_to_linear(ce_ctx *ctx, const void *pixels, size_t len, uint32_t w, uint32_t h, const float bg[3], float *out, size_t out_len, Check check,
                   Launch launch)
{
    if (!ctx) return CE_ERR_INVALID_ARG;
    if (!pixels || !bg || !out) return ce_fail(ctx, CE_ERR_INVALID_ARG, "linear-light compositing: null pointer");
    if (w == 0 || h == 0) return ce_fail(ctx, CE_ERR_INVALID_ARG, "linear-light compositing: empty image");
    const size_t n_px = (size_t)w * h;
    ce_over_plan ov;
    if (int rc = check(&ov)) return rc;
    if (int rc = over_backgrounds(ctx, 1, bg, &ov)) return rc;
    if (out_len != n_px * 3)
        return ce_fail(ctx, CE_ERR_BAD_LENGTH, "linear-light compositing: out_len must be " + std::to_string(n_px * 3) + " floats, got " + std::to_string(out_len));
    ov.slot_floats = n_px * 3;
    return ce_leaf_roundtrip(ctx, pixels, len, out, n_px * 12,
                             [&](uint8_t *d_in, uint8_t *d_out) { return launch(ctx->stream, d_in, reinterpret_cast<float *>(d_out), ov); });
}

// what ce_batch_set_*_cicp_over / _hlg_over and their leaves check: the format, then everything the plain call refuses
template <class Desc>
int tagged_over_check(ce_ctx *ctx, const void *pixels, size_t len, int format, const Desc *d, size_t n_px, ce_linear_pixel *plan, ce_over_plan *ov)
{
    if (!d) return ce_fail(ctx, CE_ERR_INVALID_ARG, std::string(words(d).name) + " ingest: null pointer");
    if (int rc = over_format_check(ctx, format)) return rc;
    if (int rc = tagged_check(ctx, pixels, len, format, d, n_px, plan)) return rc;
    return alpha_table_dev(ctx, d->depth, &ov->d_atab);
}

template <class Desc>
int set_tagged_over(ce_batch *b, bool test, uint32_t first, const uint32_t *ref_indices, const void *pixels, size_t len, int format, const Desc *d,
                    uint32_t n_bg, const float *backgrounds)
{
    ce_linear_pixel plan;
    return set_over_linear(
        b, test, first, ref_indices, pixels, len, n_bg, backgrounds,
        [&](ce_over_plan *ov) { return tagged_over_check(b->ctx, pixels, len, format, d, (size_t)b->w * b->h, &plan, ov); },
        [&](hipStream_t s, const uint8_t *d_src, float *d_dst, const ce_over_plan &ov) {
            return ce_launch_tagged_over(b->ctx, s, format, d_src, d_dst, (size_t)b->w * b->h, plan, ov);
        });
}

template <class Desc>
int tagged_over_to_linear(ce_ctx *ctx, const void *pixels, size_t len, int format, const Desc *d, uint32_t w, uint32_t h, const float bg[3], float *out,
                          size_t out_len)
{
    ce_linear_pixel plan;
    const size_t n_px = (size_t)w * h;
    return over_to_linear(
        ctx, pixels, len, w, h, bg, out, out_len, [&](ce_over_plan *ov) { return tagged_over_check(ctx, pixels, len, format, d, n_px, &plan, ov); },
        [&](hipStream_t s, const uint8_t *d_src, float *d_dst, const ce_over_plan &ov) {
            return ce_launch_tagged_over(ctx, s, format, d_src, d_dst, n_px, plan, ov);
        });
}

// ... ce_batch_set_*_icc_over and its leaf: the format, then everything ce_batch_set_*_icc refuses of a linear slot
int icc_over_check(ce_ctx *ctx, const void *pixels, size_t len, int format, uint32_t depth, const ce_icc *icc, size_t n_px, ce_icc_pixel *plan,
                   ce_over_plan *ov)
{
    if (!icc) return ce_fail(ctx, CE_ERR_INVALID_ARG, "ICC ingest: null pointer");
    if (int rc = over_format_check(ctx, format)) return rc;
    if (int rc = icc_check(ctx, pixels, len, format, depth, icc, n_px, icc_slot{0, false, true}, plan)) return rc;
    return alpha_table_dev(ctx, depth, &ov->d_atab);
}

// ... ce_batch_set_*_linear_over and its leaf
int linear_over_check(ce_ctx *ctx, size_t len, int format, size_t n_px)
{
    if (format != CE_PIXEL_RGBA_F32) return ce_fail(ctx, CE_ERR_INVALID_ARG, "linear-light compositing: the format must be CE_PIXEL_RGBA_F32");
    if (len != n_px * 16) return ce_bad_length(ctx, n_px * 16, len);
    return CE_OK;
}

}  // namespace

// yuv_check for the plane-domain scores (plane_fidelity.hip): the matrix and range are validated for the image's own depth and
// not applied
int ce_yuv_planes_check(ce_ctx *ctx, const ce_yuv_image *img, uint32_t w, uint32_t h, ce_yuv_planes *out)
{
    yuv_plan plan;
    if (int rc = yuv_check(ctx, img, w, h, img ? (uint32_t)img->depth : 8u, &plan)) return rc;
    out->n_stored = plan.n_planes;
    for (int p = 0; p < plan.n_planes; p++) out->rows[p] = plan.rows[p], out->row_bytes[p] = plan.row_bytes[p];
    out->shift = plan.dev.shift;
    return CE_OK;
}

// ---- the entry points -------------------------------------------------------------------------------------------------------

extern "C" {

int ce_batch_bind_pair(ce_batch *b, uint32_t pair_index, uint32_t ref_index)
{
    if (!b) return CE_ERR_INVALID_ARG;
    if (pair_index >= b->max_pairs || ref_index >= b->max_refs)
        return ce_fail(b->ctx, CE_ERR_INVALID_ARG, "pair/ref index out of range");
    if (b->h_pair_ref[pair_index] != ref_index) {
        b->h_pair_ref[pair_index] = ref_index;
        b->pair_ref_dirty = true;
        b->pair_ref_version++;  // device-side tables derived from it (pair_ref, XCD work lists) are rebuilt at the next launch
    }
    return CE_OK;
}

void *ce_batch_reference_slab(ce_batch *b)
{
    if (!b) return nullptr;
    ce_invalidate_reference_state(b);  // the caller may overwrite references behind our back
    return b->d_refs;
}
int ce_batch_references_changed(ce_batch *b)
{
    if (!b) return CE_ERR_INVALID_ARG;
    ce_invalidate_reference_state(b);
    return CE_OK;
}
void *ce_batch_test_slab(ce_batch *b) { return b ? b->d_tests : nullptr; }

int ce_batch_set_reference(ce_batch *b, uint32_t ref_index, const uint8_t *rgb, size_t len) { return set_rgb8(b, false, 0, ref_index, rgb, len); }
int ce_batch_set_test(ce_batch *b, uint32_t pair_index, uint32_t ref_index, const uint8_t *rgb, size_t len)
{
    return set_rgb8(b, true, pair_index, ref_index, rgb, len);
}

int ce_batch_set_reference_fmt(ce_batch *b, uint32_t ref_index, const void *pixels, size_t len, int format)
{
    return set_fmt(b, false, 0, ref_index, pixels, len, format, nullptr);
}
int ce_batch_set_test_fmt(ce_batch *b, uint32_t pair_index, uint32_t ref_index, const void *pixels, size_t len, int format)
{
    return set_fmt(b, true, pair_index, ref_index, pixels, len, format, nullptr);
}

int ce_batch_set_reference_lut(ce_batch *b, uint32_t ref_index, const void *pixels, size_t len, int format, const ce_lut *lut)
{
    return set_fmt(b, false, 0, ref_index, pixels, len, format, lut);
}
int ce_batch_set_test_lut(ce_batch *b, uint32_t pair_index, uint32_t ref_index, const void *pixels, size_t len, int format, const ce_lut *lut)
{
    return set_fmt(b, true, pair_index, ref_index, pixels, len, format, lut);
}

// CICP
int ce_srgb_table(uint32_t depth, int rule, float *out, size_t n)
{
    if (!out || !ce_deep_depth_ok(depth) || (rule != 0 && rule != 1) || n != ((size_t)1 << depth))
        return ce_fail(nullptr, CE_ERR_INVALID_ARG, "ce_srgb_table: depth 8, 10, 12 or 16, rule 0 or 1, n = 2^depth");
    if (rule == 0) ce_build_srgb_table_f64(out, (1u << depth) - 1u); else ce_build_srgb_table_powf(out, (1u << depth) - 1u);
    return CE_OK;
}

int ce_transfer_table(int transfer, uint32_t depth, float white_nits, float *out, size_t n)
{
    if (!out || !ce_deep_depth_ok(depth) || n != ((size_t)1 << depth))
        return ce_fail(nullptr, CE_ERR_INVALID_ARG, "ce_transfer_table: depth 8, 10, 12 or 16 and n = 2^depth");
    if (!ce_build_transfer_table(transfer, (1u << depth) - 1u, (double)white_nits, out))
        return ce_fail(nullptr, CE_ERR_INVALID_ARG, "ce_transfer_table: transfer 13 (sRGB), 8 (linear) or 16 (PQ, white_nits > 0)");
    return CE_OK;
}

int ce_colour_matrix(int primaries, float out[9])
{
    if (!out || !ce_build_colour_matrix(primaries, out))
        return ce_fail(nullptr, CE_ERR_INVALID_ARG, "ce_colour_matrix: primaries 1 (BT.709), 9 (BT.2020) or 12 (Display P3)");
    return CE_OK;
}

int ce_batch_set_reference_cicp(ce_batch *b, uint32_t ref_index, const void *pixels, size_t len, int format, const ce_colour *c)
{
    return set_tagged(b, false, 0, ref_index, pixels, len, format, c, kCicpWantsLinear);
}
int ce_batch_set_test_cicp(ce_batch *b, uint32_t pair_index, uint32_t ref_index, const void *pixels, size_t len, int format, const ce_colour *c)
{
    return set_tagged(b, true, pair_index, ref_index, pixels, len, format, c, kCicpWantsLinear);
}
int ce_cicp_to_linear(ce_ctx *ctx, const void *pixels, size_t len, int format, const ce_colour *c, uint32_t w, uint32_t h, float *out, size_t out_len)
{
    return tagged_to_linear(ctx, pixels, len, format, c, w, h, out, out_len);
}

// HLG
int ce_hlg_table(uint32_t depth, float *out, size_t n)
{
    if (!out || !ce_deep_depth_ok(depth) || n != ((size_t)1 << depth))
        return ce_fail(nullptr, CE_ERR_INVALID_ARG, "ce_hlg_table: depth 8, 10, 12 or 16 and n = 2^depth");
    ce_build_hlg_table((1u << depth) - 1u, out);
    return CE_OK;
}

int ce_hlg_params(const ce_hlg *h, double out[5])
{
    if (!h || !out) return ce_fail(nullptr, CE_ERR_INVALID_ARG, "ce_hlg_params: null pointer");
    return hlg_describe(nullptr, h, out);
}

int ce_batch_set_reference_hlg(ce_batch *b, uint32_t ref_index, const void *pixels, size_t len, int format, const ce_hlg *h)
{
    return set_tagged(b, false, 0, ref_index, pixels, len, format, h, kHlgWantsLinear);
}
int ce_batch_set_test_hlg(ce_batch *b, uint32_t pair_index, uint32_t ref_index, const void *pixels, size_t len, int format, const ce_hlg *h)
{
    return set_tagged(b, true, pair_index, ref_index, pixels, len, format, h, kHlgWantsLinear);
}
int ce_hlg_to_linear(ce_ctx *ctx, const void *pixels, size_t len, int format, const ce_hlg *h, uint32_t w, uint32_t height, float *out, size_t out_len)
{
    return tagged_to_linear(ctx, pixels, len, format, h, w, height, out, out_len);
}

// gain maps
int ce_gainmap_weight(const ce_gainmap *g, double *w)
{
    if (!g || !w) return ce_fail(nullptr, CE_ERR_INVALID_ARG, "ce_gainmap_weight: null pointer");
    if (int rc = gainmap_headrooms_check(nullptr, g)) return rc;
    *w = ce_build_gainmap_weight(g);
    return CE_OK;
}

int ce_gainmap_tables(const ce_gainmap *g, uint32_t channels, double *out, size_t n)
{
    if (!g || !out) return ce_fail(nullptr, CE_ERR_INVALID_ARG, "ce_gainmap_tables: null pointer");
    if (int rc = gainmap_meta_check(nullptr, g, channels)) return rc;
    if (n != (size_t)256 * channels) return ce_fail(nullptr, CE_ERR_INVALID_ARG, "ce_gainmap_tables: n must be 256 * channels");
    ce_build_gainmap_tables(g, channels, out);
    return CE_OK;
}

int ce_batch_set_reference_gainmap(ce_batch *b, uint32_t ref_index, const void *pixels, size_t len, int format, const ce_colour *c,
                                   const ce_gainmap_image *map, const ce_gainmap *g)
{
    return set_gainmap(b, false, 0, ref_index, pixels, len, format, c, map, g);
}
int ce_batch_set_test_gainmap(ce_batch *b, uint32_t pair_index, uint32_t ref_index, const void *pixels, size_t len, int format, const ce_colour *c,
                              const ce_gainmap_image *map, const ce_gainmap *g)
{
    return set_gainmap(b, true, pair_index, ref_index, pixels, len, format, c, map, g);
}
int ce_gainmap_to_linear(ce_ctx *ctx, const void *pixels, size_t len, int format, const ce_colour *c, const ce_gainmap_image *map, const ce_gainmap *g,
                         uint32_t w, uint32_t h, float *out, size_t out_len)
{
    return gainmap_to_linear(ctx, pixels, len, format, c, map, g, w, h, out, out_len);
}

// ICC profiles of both flavours (DESIGN.md sections 22, 23); the handles are made in ce_handles.cpp
int ce_batch_set_reference_icc(ce_batch *b, uint32_t ref_index, const void *pixels, size_t len, int format, uint32_t depth, const ce_icc *icc)
{
    return set_icc(b, false, 0, ref_index, pixels, len, format, depth, icc);
}
int ce_batch_set_test_icc(ce_batch *b, uint32_t pair_index, uint32_t ref_index, const void *pixels, size_t len, int format, uint32_t depth,
                          const ce_icc *icc)
{
    return set_icc(b, true, pair_index, ref_index, pixels, len, format, depth, icc);
}
int ce_icc_to_linear(ce_ctx *ctx, const void *pixels, size_t len, int format, uint32_t depth, const ce_icc *icc, uint32_t w, uint32_t h, float *out,
                     size_t out_len)
{
    return icc_to_host(ctx, pixels, len, format, depth, icc, w, h, 0, false, out, out_len);
}
int ce_icc_to_srgb8(ce_ctx *ctx, const void *pixels, size_t len, int format, uint32_t depth, const ce_icc *icc, uint32_t w, uint32_t h, uint8_t *out,
                    size_t out_len)
{
    return icc_to_host(ctx, pixels, len, format, depth, icc, w, h, 8, false, out, out_len);
}
int ce_icc_to_srgb16(ce_ctx *ctx, const void *pixels, size_t len, int format, uint32_t depth, const ce_icc *icc, uint32_t w, uint32_t h,
                     uint32_t depth_out, uint16_t *out, size_t out_len)
{
    return icc_to_host(ctx, pixels, len, format, depth, icc, w, h, depth_out, true, out, out_len);
}

// planar Y'CbCr, alone and with either description (DESIGN.md sections 13, 16, 18)
int ce_batch_set_reference_yuv(ce_batch *b, uint32_t ref_index, const ce_yuv_image *image) { return set_yuv(b, false, 0, ref_index, image); }
int ce_batch_set_test_yuv(ce_batch *b, uint32_t pair_index, uint32_t ref_index, const ce_yuv_image *image)
{
    return set_yuv(b, true, pair_index, ref_index, image);
}
int ce_yuv_to_rgb8(ce_ctx *ctx, const ce_yuv_image *image, uint32_t width, uint32_t height, uint8_t *out, size_t out_len)
{
    return yuv_to_host(ctx, image, width, height, false, 8, out, out_len);
}
int ce_yuv_to_rgb16(ce_ctx *ctx, const ce_yuv_image *image, uint32_t width, uint32_t height, uint32_t depth_out, uint16_t *out, size_t out_len)
{
    return yuv_to_host(ctx, image, width, height, true, depth_out, out, out_len);
}

int ce_batch_set_reference_yuv_cicp(ce_batch *b, uint32_t ref_index, const ce_yuv_image *image, const ce_colour *c)
{
    return set_yuv_tagged(b, false, 0, ref_index, image, c, kYuvCicpWantsLinear);
}
int ce_batch_set_test_yuv_cicp(ce_batch *b, uint32_t pair_index, uint32_t ref_index, const ce_yuv_image *image, const ce_colour *c)
{
    return set_yuv_tagged(b, true, pair_index, ref_index, image, c, kYuvCicpWantsLinear);
}
int ce_yuv_to_linear(ce_ctx *ctx, const ce_yuv_image *image, const ce_colour *c, uint32_t w, uint32_t h, float *out, size_t out_len)
{
    return yuv_to_linear(ctx, image, c, w, h, out, out_len);
}

int ce_batch_set_reference_yuv_icc(ce_batch *b, uint32_t ref_index, const ce_yuv_image *image, uint32_t rgb_depth, const ce_icc *icc)
{
    return set_yuv_icc(b, false, 0, ref_index, image, rgb_depth, icc);
}
int ce_batch_set_test_yuv_icc(ce_batch *b, uint32_t pair_index, uint32_t ref_index, const ce_yuv_image *image, uint32_t rgb_depth, const ce_icc *icc)
{
    return set_yuv_icc(b, true, pair_index, ref_index, image, rgb_depth, icc);
}
int ce_yuv_icc_to_linear(ce_ctx *ctx, const ce_yuv_image *image, uint32_t rgb_depth, const ce_icc *icc, uint32_t w, uint32_t h, float *out, size_t out_len)
{
    return yuv_icc_to_host(ctx, image, rgb_depth, icc, w, h, 0, false, out, out_len);
}
int ce_yuv_icc_to_srgb8(ce_ctx *ctx, const ce_yuv_image *image, uint32_t rgb_depth, const ce_icc *icc, uint32_t w, uint32_t h, uint8_t *out, size_t out_len)
{
    return yuv_icc_to_host(ctx, image, rgb_depth, icc, w, h, 8, false, out, out_len);
}
int ce_yuv_icc_to_srgb16(ce_ctx *ctx, const ce_yuv_image *image, uint32_t rgb_depth, const ce_icc *icc, uint32_t w, uint32_t h, uint32_t depth_out,
                         uint16_t *out, size_t out_len)
{
    return yuv_icc_to_host(ctx, image, rgb_depth, icc, w, h, depth_out, true, out, out_len);
}

int ce_batch_set_reference_yuv_hlg(ce_batch *b, uint32_t ref_index, const ce_yuv_image *image, const ce_hlg *h)
{
    return set_yuv_tagged(b, false, 0, ref_index, image, h, kHlgWantsLinear);
}
int ce_batch_set_test_yuv_hlg(ce_batch *b, uint32_t pair_index, uint32_t ref_index, const ce_yuv_image *image, const ce_hlg *h)
{
    return set_yuv_tagged(b, true, pair_index, ref_index, image, h, kHlgWantsLinear);
}
int ce_yuv_hlg_to_linear(ce_ctx *ctx, const ce_yuv_image *image, const ce_hlg *hd, uint32_t w, uint32_t h, float *out, size_t out_len)
{
    return yuv_to_linear(ctx, image, hd, w, h, out, out_len);
}

// strided tensors
int ce_batch_set_reference_tensor(ce_batch *b, uint32_t first_ref, uint32_t count, const ce_tensor_image *t)
{
    return set_tensor(b, false, first_ref, nullptr, count, t);
}
int ce_batch_set_test_tensor(ce_batch *b, uint32_t first_pair, const uint32_t *ref_indices, uint32_t count, const ce_tensor_image *t)
{
    return set_tensor(b, true, first_pair, ref_indices, count, t);
}
int ce_tensor_to_rgb8(ce_ctx *ctx, const ce_tensor_image *t, uint32_t w, uint32_t h, uint8_t *out, size_t out_len)
{
    return tensor_to_host(ctx, t, w, h, tensor_slot{kTensorSlotU8, 8}, out, out_len);
}
int ce_tensor_to_rgb16(ce_ctx *ctx, const ce_tensor_image *t, uint32_t w, uint32_t h, uint32_t depth_out, uint16_t *out, size_t out_len)
{
    return tensor_to_host(ctx, t, w, h, tensor_slot{kTensorSlotU16, depth_out}, out, out_len);
}
int ce_tensor_to_linear(ce_ctx *ctx, const ce_tensor_image *t, uint32_t w, uint32_t h, float *out, size_t out_len)
{
    return tensor_to_host(ctx, t, w, h, tensor_slot{kTensorSlotLin, 0}, out, out_len);
}

// alpha
int ce_batch_set_reference_over(ce_batch *b, uint32_t first_ref, const void *pixels, size_t len, int format, uint32_t n_bg, const uint16_t *backgrounds)
{
    return set_over(b, false, first_ref, nullptr, pixels, len, format, n_bg, backgrounds);
}
int ce_batch_set_test_over(ce_batch *b, uint32_t first_pair, const uint32_t *ref_indices, const void *pixels, size_t len, int format, uint32_t n_bg,
                           const uint16_t *backgrounds)
{
    return set_over(b, true, first_pair, ref_indices, pixels, len, format, n_bg, backgrounds);
}

int ce_composite_rgba8(ce_ctx *ctx, const uint8_t *rgba, size_t len, uint32_t w, uint32_t h, const uint8_t bg[3], uint8_t *out, size_t out_len)
{
    uint16_t bg16[3] = {};
    for (int c = 0; bg && c < 3; c++) bg16[c] = bg[c];
    return composite_to_host(ctx, rgba, len, w, h, false, 8, bg ? bg16 : nullptr, out, out_len);
}

int ce_composite_rgba16(ce_ctx *ctx, const uint16_t *rgba, size_t len, uint32_t w, uint32_t h, uint32_t depth, const uint16_t bg[3], uint16_t *out,
                        size_t out_len)
{
    return composite_to_host(ctx, rgba, len, w, h, true, depth, bg, out, out_len);
}

// alpha in linear light
int ce_alpha_table(uint32_t depth, float *out, size_t n)
{
    if (!out || !ce_deep_depth_ok(depth) || n != ((size_t)1 << depth))
        return ce_fail(nullptr, CE_ERR_INVALID_ARG, "ce_alpha_table: depth 8, 10, 12 or 16 and n = 2^depth");
    build_alpha_table(depth, out);
    return CE_OK;
}

int ce_batch_set_reference_cicp_over(ce_batch *b, uint32_t first_ref, const void *pixels, size_t len, int format, const ce_colour *c, uint32_t n_bg,
                                     const float *backgrounds)
{
    return set_tagged_over(b, false, first_ref, nullptr, pixels, len, format, c, n_bg, backgrounds);
}
int ce_batch_set_test_cicp_over(ce_batch *b, uint32_t first_pair, const uint32_t *ref_indices, const void *pixels, size_t len, int format,
                                const ce_colour *c, uint32_t n_bg, const float *backgrounds)
{
    return set_tagged_over(b, true, first_pair, ref_indices, pixels, len, format, c, n_bg, backgrounds);
}
int ce_batch_set_reference_hlg_over(ce_batch *b, uint32_t first_ref, const void *pixels, size_t len, int format, const ce_hlg *h, uint32_t n_bg,
                                    const float *backgrounds)
{
    return set_tagged_over(b, false, first_ref, nullptr, pixels, len, format, h, n_bg, backgrounds);
}
int ce_batch_set_test_hlg_over(ce_batch *b, uint32_t first_pair, const uint32_t *ref_indices, const void *pixels, size_t len, int format,
                               const ce_hlg *h, uint32_t n_bg, const float *backgrounds)
{
    return set_tagged_over(b, true, first_pair, ref_indices, pixels, len, format, h, n_bg, backgrounds);
}

static int set_icc_over(ce_batch *b, bool test, uint32_t first, const uint32_t *ref_indices, const void *pixels, size_t len, int format, uint32_t depth,
                        const ce_icc *icc, uint32_t n_bg, const float *backgrounds)
{
    ce_icc_pixel plan;
    return set_over_linear(
        b, test, first, ref_indices, pixels, len, n_bg, backgrounds,
        [&](ce_over_plan *ov) { return icc_over_check(b->ctx, pixels, len, format, depth, icc, (size_t)b->w * b->h, &plan, ov); },
        [&](hipStream_t s, const uint8_t *d_src, float *d_dst, const ce_over_plan &ov) {
            return ce_launch_icc(b->ctx, s, format, d_src, d_dst, (size_t)b->w * b->h, plan, &ov);
        });
}
int ce_batch_set_reference_icc_over(ce_batch *b, uint32_t first_ref, const void *pixels, size_t len, int format, uint32_t depth, const ce_icc *icc,
                                    uint32_t n_bg, const float *backgrounds)
{
    return set_icc_over(b, false, first_ref, nullptr, pixels, len, format, depth, icc, n_bg, backgrounds);
}
int ce_batch_set_test_icc_over(ce_batch *b, uint32_t first_pair, const uint32_t *ref_indices, const void *pixels, size_t len, int format, uint32_t depth,
                               const ce_icc *icc, uint32_t n_bg, const float *backgrounds)
{
    return set_icc_over(b, true, first_pair, ref_indices, pixels, len, format, depth, icc, n_bg, backgrounds);
}

static int set_linear_over(ce_batch *b, bool test, uint32_t first, const uint32_t *ref_indices, const void *pixels, size_t len, int format,
                           int premultiplied, uint32_t n_bg, const float *backgrounds)
{
    return set_over_linear(
        b, test, first, ref_indices, pixels, len, n_bg, backgrounds,
        [&](ce_over_plan *) { return linear_over_check(b->ctx, len, format, (size_t)b->w * b->h); },
        [&](hipStream_t s, const uint8_t *d_src, float *d_dst, const ce_over_plan &ov) {
            return ce_launch_linear_over(b->ctx, s, reinterpret_cast<const float *>(d_src), d_dst, (size_t)b->w * b->h, premultiplied != 0, ov);
        });
}
int ce_batch_set_reference_linear_over(ce_batch *b, uint32_t first_ref, const void *pixels, size_t len, int format, int premultiplied, uint32_t n_bg,
                                       const float *backgrounds)
{
    return set_linear_over(b, false, first_ref, nullptr, pixels, len, format, premultiplied, n_bg, backgrounds);
}
int ce_batch_set_test_linear_over(ce_batch *b, uint32_t first_pair, const uint32_t *ref_indices, const void *pixels, size_t len, int format,
                                  int premultiplied, uint32_t n_bg, const float *backgrounds)
{
    return set_linear_over(b, true, first_pair, ref_indices, pixels, len, format, premultiplied, n_bg, backgrounds);
}

int ce_cicp_over_to_linear(ce_ctx *ctx, const void *pixels, size_t len, int format, const ce_colour *c, uint32_t w, uint32_t h, const float bg[3],
                           float *out, size_t out_len)
{
    return tagged_over_to_linear(ctx, pixels, len, format, c, w, h, bg, out, out_len);
}
int ce_hlg_over_to_linear(ce_ctx *ctx, const void *pixels, size_t len, int format, const ce_hlg *hd, uint32_t w, uint32_t h, const float bg[3],
                          float *out, size_t out_len)
{
    return tagged_over_to_linear(ctx, pixels, len, format, hd, w, h, bg, out, out_len);
}
int ce_icc_over_to_linear(ce_ctx *ctx, const void *pixels, size_t len, int format, uint32_t depth, const ce_icc *icc, uint32_t w, uint32_t h,
                          const float bg[3], float *out, size_t out_len)
{
    ce_icc_pixel plan;
    const size_t n_px = (size_t)w * h;
    return over_to_linear(
        ctx, pixels, len, w, h, bg, out, out_len, [&](ce_over_plan *ov) { return icc_over_check(ctx, pixels, len, format, depth, icc, n_px, &plan, ov); },
        [&](hipStream_t s, const uint8_t *d_src, float *d_dst, const ce_over_plan &ov) { return ce_launch_icc(ctx, s, format, d_src, d_dst, n_px, plan, &ov); });
}
int ce_linear_over(ce_ctx *ctx, const void *pixels, size_t len, int format, int premultiplied, uint32_t w, uint32_t h, const float bg[3], float *out,
                   size_t out_len)
{
    const size_t n_px = (size_t)w * h;
    return over_to_linear(
        ctx, pixels, len, w, h, bg, out, out_len, [&](ce_over_plan *) { return linear_over_check(ctx, len, format, n_px); },
        [&](hipStream_t s, const uint8_t *d_src, float *d_dst, const ce_over_plan &ov) {
            return ce_launch_linear_over(ctx, s, reinterpret_cast<const float *>(d_src), d_dst, n_px, premultiplied != 0, ov);
        });
}

}  // extern "C"
