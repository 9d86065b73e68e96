// Viewing simulation: resampling (include/ce_metrics.h: ce_resample_rgb8, ce_resample_linear, ce_batch_resample,
// ce_batch_resample_pairs; DESIGN.md sections 12 and 17).  One host half serves both resamplers - the fixed-point one over
// packed RGB8 (resample.hip) and the float one over packed f32 RGB (resample_f32.hip): the kept tap tables, the image between
// the passes, the checks.  `linear` selects the element size and the launcher.  All device work is in the .hip files.
#include <algorithm>

#include "ce_internal.h"

// the taps of one axis on the device, built on first use and kept with the context (ce_ctx::rs_tables); the fixed-point and
// the f64 table of one (n_in, n_out, filter) are two entries
static int resample_table(ce_ctx *ctx, uint32_t n_in, uint32_t n_out, int filter, bool f64, const ce_resample_axis **out)
{
    const auto key = std::make_tuple(n_in, n_out, filter, f64);
    auto it = ctx->rs_tables.find(key);
    if (it == ctx->rs_tables.end()) {
        std::vector<int32_t> fixed;
        std::vector<double> wide;
        ce_resample_axis a;
        a.n_in = n_in, a.n_out = n_out;
        if (!(f64 ? ce_build_resample_table_f64(n_in, n_out, filter, wide, &a.ksize) : ce_build_resample_table(n_in, n_out, filter, fixed, &a.ksize)))
            return ce_fail(ctx, CE_ERR_INVALID_ARG, "resample: bad axis");
        if (int rc = f64 ? ce_device_table(ctx, wide.data(), wide.size() * sizeof(double), "resample taps", &a.d)
                         : ce_device_table(ctx, fixed.data(), fixed.size() * sizeof(int32_t), "resample taps", &a.d))
            return rc;
        it = ctx->rs_tables.emplace(key, a).first;
    }
    *out = &it->second;
    return CE_OK;
}

static bool resample_filter_ok(int filter) { return filter >= CE_RESAMPLE_BOX && filter <= CE_RESAMPLE_LANCZOS3; }

// the image between the two passes: at least `need` bytes of ce_ctx::rs_mid
static int resample_mid(ce_ctx *ctx, size_t need)
{
    if (ctx->rs_mid_cap < need) {
        CE_HIP(ctx, hipStreamSynchronize(ctx->stream));  // an earlier resample may still be between its passes
        CE_HIP(ctx, hipFree(ctx->rs_mid));
        ctx->rs_mid = nullptr;
        ctx->rs_mid_cap = 0;
        CE_HIP(ctx, hipMalloc((void **)&ctx->rs_mid, need + need / 4));
        ctx->rs_mid_cap = need + need / 4;
    }
    return CE_OK;
}

// n images of w x h at d_src (src_stride bytes apart) to out_w x out_h at d_dst, queued on the context's stream: packed RGB8,
// or (linear) packed f32 RGB, whose strides are multiples of 4; equal sizes are a byte copy, unclamped
static int resample_images(ce_ctx *ctx, bool linear, const uint8_t *d_src, size_t src_stride, uint8_t *d_dst, size_t dst_stride, uint32_t w,
                           uint32_t h, uint32_t out_w, uint32_t out_h, uint32_t n, int filter)
{
    const size_t pixel = linear ? 12 : 3;
    if (w == out_w && h == out_h) {  // no pass changes a size: the bytes themselves
        const size_t img = (size_t)w * h * pixel;
        if (src_stride == img && dst_stride == img) {
            CE_HIP(ctx, hipMemcpyAsync(d_dst, d_src, img * n, hipMemcpyDeviceToDevice, ctx->stream));
        } else {
            for (uint32_t i = 0; i < n; i++)
                CE_HIP(ctx, hipMemcpyAsync(d_dst + i * dst_stride, d_src + i * src_stride, img, hipMemcpyDeviceToDevice, ctx->stream));
        }
        return CE_OK;
    }
    const ce_resample_axis *horiz = nullptr, *vert = nullptr;
    if (w != out_w)
        if (int rc = resample_table(ctx, w, out_w, filter, linear, &horiz)) return rc;
    if (h != out_h)
        if (int rc = resample_table(ctx, h, out_h, filter, linear, &vert)) return rc;
    if (horiz && vert)
        if (int rc = resample_mid(ctx, (size_t)n * h * out_w * pixel)) return rc;
    if (linear)
        return ce_launch_resample_f32(ctx, ctx->stream, reinterpret_cast<const float *>(d_src), src_stride / 4, reinterpret_cast<float *>(d_dst),
                                      dst_stride / 4, w, h, out_w, out_h, n, horiz, vert, reinterpret_cast<float *>(ctx->rs_mid));
    return ce_launch_resample(ctx, ctx->stream, d_src, src_stride, d_dst, dst_stride, w, h, out_w, out_h, n, horiz, vert, ctx->rs_mid);
}

// one host image through the leaf scratch: ce_resample_rgb8 and ce_resample_linear behind their element size
static int resample_leaf(ce_ctx *ctx, bool linear, const void *rgb, size_t len, uint32_t w, uint32_t h, uint32_t out_w, uint32_t out_h, int filter,
                         void *out, size_t out_len)
{
    if (!ctx || !rgb || !out) return ce_fail(ctx, CE_ERR_INVALID_ARG, "resample: null pointer");
    if (!resample_filter_ok(filter)) return ce_fail(ctx, CE_ERR_INVALID_ARG, "resample: unknown filter " + std::to_string(filter));
    if (w == 0 || h == 0 || out_w == 0 || out_h == 0)
        return ce_fail(ctx, CE_ERR_INVALID_ARG, "resample: " + std::to_string(w) + " x " + std::to_string(h) + " to " + std::to_string(out_w) +
                                                 " x " + std::to_string(out_h) + " has an empty side");
    const size_t pixel = linear ? 12 : 3, want_in = (size_t)w * h * pixel, want_out = (size_t)out_w * out_h * pixel;
    if (len != want_in) return ce_bad_length(ctx, want_in, len);
    if (out_len != want_out) return ce_bad_length(ctx, want_out, out_len);
    return ce_leaf_roundtrip(ctx, rgb, len, out, out_len, [&](uint8_t *d_in, uint8_t *d_out) {
        return resample_images(ctx, linear, d_in, want_in, d_out, want_out, w, h, out_w, out_h, 1, filter);
    });
}

extern "C" {

int ce_resample_rgb8(ce_ctx *ctx, const uint8_t *rgb, size_t len, uint32_t w, uint32_t h, uint32_t out_w, uint32_t out_h, int filter,
                     uint8_t *out, size_t out_len)
{
    return resample_leaf(ctx, false, rgb, len, w, h, out_w, out_h, filter, out, out_len);
}

int ce_resample_linear(ce_ctx *ctx, const float *rgb, size_t len, uint32_t w, uint32_t h, uint32_t out_w, uint32_t out_h, int filter, float *out,
                       size_t out_len)
{
    return resample_leaf(ctx, true, rgb, len, w, h, out_w, out_h, filter, out, out_len);
}

// the checks two batches must pass before anything moves between them
static int resample_check(ce_batch *src, ce_batch *dst, int filter)
{
    if (!src || !dst) return ce_fail(src ? src->ctx : dst ? dst->ctx : nullptr, CE_ERR_INVALID_ARG, "resample: null batch");
    ce_ctx *ctx = src->ctx;
    if (dst->ctx != ctx) return ce_fail(ctx, CE_ERR_INVALID_ARG, "resample: the two batches belong to different contexts");
    if (src == dst) return ce_fail(ctx, CE_ERR_INVALID_ARG, "resample: source and destination are the same batch");
    if (!resample_filter_ok(filter)) return ce_fail(ctx, CE_ERR_INVALID_ARG, "resample: unknown filter " + std::to_string(filter));
    if (src->depth[0] || dst->depth[0])
        return ce_fail(ctx, CE_ERR_INVALID_ARG, src->linear || dst->linear
                                                 ? "resample: a linear batch resamples into a linear batch only, and a deep batch is out of its scope"
                                                 : "resample works on RGB8 and linear batches: a deep batch is out of its scope");
    if (src->linear != dst->linear)
        return ce_fail(ctx, CE_ERR_INVALID_ARG, "resample: a linear batch resamples into a linear batch only, an RGB8 batch into an RGB8 one");
    return CE_OK;
}

static int resample_slab(ce_batch *src, ce_batch *dst, uint32_t which, uint32_t first, uint32_t count, int filter)
{
    ce_ctx *ctx = src->ctx;
    const bool tests = which == CE_BATCH_TESTS;
    CE_HIP(ctx, hipSetDevice(ctx->device));
    // the kernels run on the context's stream: behind src's uploads (the ordering of a launch), and as an inline write of
    // dst (ce_order_write: behind dst's own uploads, ahead of its next launch and of its later uploads)
    if (int rc = ce_flush_uploads(src)) return rc;
    if (int rc = ce_order_write(dst, true)) return rc;
    if (!tests) ce_invalidate_reference_state(dst);
    const uint8_t *s = (tests ? src->d_tests : src->d_refs) + (size_t)first * src->img_bytes;
    uint8_t *d = (tests ? dst->d_tests : dst->d_refs) + (size_t)first * dst->img_bytes;
    const int rc = resample_images(ctx, src->linear, s, src->img_bytes, d, dst->img_bytes, src->w, src->h, dst->w, dst->h, count, filter);
    src->inline_pending = true;  // a later upload into src waits for these reads (ce_order_write)
    return rc;
}

static int resample_range_check(ce_batch *src, ce_batch *dst, bool tests, uint32_t first, uint32_t count)
{
    const uint32_t slots = tests ? std::min(src->max_pairs, dst->max_pairs) : std::min(src->max_refs, dst->max_refs);
    if (count == 0 || first > slots || count > slots - first)
        return ce_fail(src->ctx, CE_ERR_INVALID_ARG, std::string("resample: ") + (tests ? "tests [" : "references [") + std::to_string(first) + ", " +
                                                      std::to_string((uint64_t)first + count) + ") outside the " + std::to_string(slots) +
                                                      " slots both batches have");
    return CE_OK;
}

int ce_batch_resample(ce_batch *src, ce_batch *dst, uint32_t which, uint32_t first, uint32_t count, int filter)
{
    if (int rc = resample_check(src, dst, filter)) return rc;
    if (which != CE_BATCH_REFERENCES && which != CE_BATCH_TESTS)
        return ce_fail(src->ctx, CE_ERR_INVALID_ARG, "resample: unknown slab " + std::to_string(which));
    if (int rc = resample_range_check(src, dst, which == CE_BATCH_TESTS, first, count)) return rc;
    return resample_slab(src, dst, which, first, count, filter);
}

int ce_batch_resample_pairs(ce_batch *src, ce_batch *dst, uint32_t n_refs, uint32_t n_pairs, int filter)
{
    if (int rc = resample_check(src, dst, filter)) return rc;
    if (int rc = resample_range_check(src, dst, false, 0, n_refs)) return rc;
    if (int rc = resample_range_check(src, dst, true, 0, n_pairs)) return rc;
    for (uint32_t i = 0; i < n_pairs; i++)
        if (src->h_pair_ref[i] >= n_refs)
            return ce_fail(src->ctx, CE_ERR_INVALID_ARG, "resample: pair " + std::to_string(i) + " is bound to reference " +
                                                          std::to_string(src->h_pair_ref[i]) + ", outside the " + std::to_string(n_refs) + " resampled");
    if (int rc = resample_slab(src, dst, CE_BATCH_REFERENCES, 0, n_refs, filter)) return rc;
    if (int rc = resample_slab(src, dst, CE_BATCH_TESTS, 0, n_pairs, filter)) return rc;
    for (uint32_t i = 0; i < n_pairs; i++)
        if (int rc = ce_batch_bind_pair(dst, i, src->h_pair_ref[i])) return rc;
    return CE_OK;
}

}  // extern "C"
