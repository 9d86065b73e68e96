// Every call that takes host images and returns a result through scratch the context owns (include/ce_metrics.h:
// ce_eval_pair*, ce_calculate_*, ce_xyb_roundtrip, ce_rgb8_to_dssim_image, ce_image_heuristics_rgb8).  Two things live here
// once: the grow-only leaf scratch of the one-image calls (ce_leaf_scratch, ce_leaf_roundtrip) and the frame of the kept
// one-pair batches (leaf_batch hands out the batch of a kind, leaf_pair runs a pair through it).  All device work is in the
// .hip files.
#include <algorithm>
#include <cmath>
#include <cstring>

#include "ce_internal.h"

// ---- the leaf scratch -----------------------------------------------------------------------------------------------------------

// leaf scratch (ce_internal.h): device buffers of at least in_bytes / out_bytes and a pinned staging buffer of the larger
int ce_leaf_scratch(ce_ctx *ctx, size_t in_bytes, size_t out_bytes)
{
    CE_HIP(ctx, hipSetDevice(ctx->device));
    auto grow = [&](uint8_t *&p, size_t &cap, size_t want, bool host) -> int {
        if (cap >= want) return CE_OK;
        if (p) CE_HIP(ctx, host ? hipHostFree(p) : hipFree(p));
        p = nullptr;
        cap = 0;
        const size_t sz = want + want / 4;  // a little head room: a sweep over nearby shapes does not reallocate each time
        CE_HIP(ctx, host ? hipHostMalloc((void **)&p, sz, hipHostMallocDefault) : hipMalloc((void **)&p, sz));
        cap = sz;
        return CE_OK;
    };
    int rc = grow(ctx->leaf_d_in, ctx->leaf_in_cap, in_bytes, false);
    if (rc == CE_OK) rc = grow(ctx->leaf_d_out, ctx->leaf_out_cap, out_bytes, false);
    if (rc == CE_OK) rc = grow(ctx->leaf_h, ctx->leaf_h_cap, std::max(in_bytes, out_bytes), true);
    return rc;
}

// fill(h_in, d_in) writes in_bytes of input into h_in (d_in is where its device copy will be; nothing with in_bytes = 0, for
// input that is on the device already) -> kernel -> host image out through the leaf scratch, everything on the context's stream
int ce_leaf_roundtrip(ce_ctx *ctx, size_t in_bytes, const std::function<void(uint8_t *, uint8_t *)> &fill, void *out, size_t out_bytes,
                      const std::function<int(uint8_t *, uint8_t *)> &launch)
{
    int rc = ce_leaf_scratch(ctx, in_bytes ? in_bytes : 1, out_bytes);
    if (rc != CE_OK) return rc;
    fill(ctx->leaf_h, ctx->leaf_d_in);
    if (in_bytes) CE_HIP(ctx, hipMemcpyAsync(ctx->leaf_d_in, ctx->leaf_h, in_bytes, hipMemcpyHostToDevice, ctx->stream));
    rc = launch(ctx->leaf_d_in, ctx->leaf_d_out);
    if (rc != CE_OK) return rc;
    CE_HIP(ctx, hipMemcpyAsync(ctx->leaf_h, ctx->leaf_d_out, out_bytes, hipMemcpyDeviceToHost, ctx->stream));
    CE_HIP(ctx, hipStreamSynchronize(ctx->stream));
    std::memcpy(out, ctx->leaf_h, out_bytes);
    return CE_OK;
}

// the same for a host image that is packed already
int ce_leaf_roundtrip(ce_ctx *ctx, const void *in, size_t in_bytes, void *out, size_t out_bytes,
                      const std::function<int(uint8_t *, uint8_t *)> &launch)
{
    return ce_leaf_roundtrip(ctx, in_bytes, [&](uint8_t *h_in, uint8_t *) { std::memcpy(h_in, in, in_bytes); }, out, out_bytes, launch);
}

// ---- the kept one-pair batches -----------------------------------------------------------------------------------------------

// The context's kept 1 x 1 batch of `kind` (ce_ctx::leaf_batch; not the pooled ce_eval_batch batches, whose next call reuses
// them) at this shape and, for the deep kind, these depths (0 / 0 otherwise): remade when one of them changes.  The caller
// has selected the device.
static int leaf_batch(ce_ctx *ctx, ce_leaf_kind kind, uint32_t width, uint32_t height, uint32_t ref_depth, uint32_t test_depth, ce_batch **out)
{
    ce_batch *&b = ctx->leaf_batch[kind];
    if (!b || b->w != width || b->h != height || b->depth[0] != ref_depth || b->depth[1] != test_depth) {
        ce_batch_destroy(b);
        b = nullptr;
        if (int rc = kind == CE_LEAF_DEEP     ? ce_batch_create_deep(ctx, width, height, 1, 1, ref_depth, test_depth, &b)
                     : kind == CE_LEAF_LINEAR ? ce_batch_create_linear(ctx, width, height, 1, 1, &b)
                                              : ce_batch_create(ctx, width, height, 1, 1, &b))
            return rc;
    }
    *out = b;
    return CE_OK;
}

// One pair of checked images, `len` bytes each, through that batch: set the reference, set the test, `run` (a launch and its
// collect, or a score); a failure drains what may still read the caller's buffers.  The RGB8 kind is collected before its
// callers return, so page-locked images are read in place (ce_ingest.cpp: upload()).
template <class Run>
static int leaf_pair(ce_batch *b, ce_leaf_kind kind, const void *reference, const void *test, size_t len, Run run)
{
    const int format = kind == CE_LEAF_DEEP ? CE_PIXEL_RGB16 : CE_PIXEL_RGB_F32;
    b->caller_blocks = kind == CE_LEAF_RGB8;
    int rc = kind == CE_LEAF_RGB8 ? ce_batch_set_reference(b, 0, static_cast<const uint8_t *>(reference), len)
                                  : ce_batch_set_reference_fmt(b, 0, reference, len, format);
    if (rc == CE_OK)
        rc = kind == CE_LEAF_RGB8 ? ce_batch_set_test(b, 0, 0, static_cast<const uint8_t *>(test), len)
                                  : ce_batch_set_test_fmt(b, 0, 0, test, len, format);
    if (rc == CE_OK) rc = run();
    if (rc != CE_OK) ce_drain_batch(b);
    b->caller_blocks = false;
    return rc;
}

// ce_eval_pair_deep (depths: the two of them, 6 bytes a pixel) and ce_eval_pair_linear (depths: nullptr, 12 bytes a pixel).
// Validation in ce_eval_pair's order: null pointers, (the depths,) empty image, length mismatch, wrong length; then the flags.
static int eval_pair_wide(ce_ctx *ctx, ce_leaf_kind kind, const uint32_t *depths, size_t bytes_per_pixel, const void *reference,
                          size_t reference_len, const void *test, size_t test_len, uint32_t width, uint32_t height, uint32_t metric_mask,
                          uint32_t flags, float intensity_target, ce_scores *out)
{
    if (!ctx || !out || !reference || !test) return CE_ERR_INVALID_ARG;
    *out = ce_scores{};
    if (depths && (!ce_deep_depth_ok(depths[0]) || !ce_deep_depth_ok(depths[1])))
        return out->status = ce_fail(ctx, CE_ERR_INVALID_ARG, "depths must be 8, 10, 12 or 16 bits, got " + std::to_string(depths[0]) + " / " +
                                                               std::to_string(depths[1]));
    if (width == 0 || height == 0) return out->status = CE_ERR_INVALID_ARG;
    if (reference_len != test_len)
        return out->status = ce_fail(ctx, CE_ERR_DIM_MISMATCH, "Dimension mismatch: reference " + std::to_string(reference_len) +
                                                                " bytes, test " + std::to_string(test_len) + " bytes");
    const size_t want = (size_t)width * height * bytes_per_pixel;
    if (reference_len != want) return out->status = ce_bad_length(ctx, want, reference_len);
    if (flags & (CE_FLAG_BUTTERAUGLI_DIFFMAP | CE_FLAG_SSIMULACRA2_MAPS))
        return out->status = ce_fail(ctx, CE_ERR_INVALID_ARG, "map flags need a ce_batch: this call's batch does not outlive it");
    if (metric_mask & ~ce_known_metrics) return out->status = ce_fail(ctx, CE_ERR_INVALID_ARG, "unknown metric bit");
    CE_HIP(ctx, hipSetDevice(ctx->device));
    ce_batch *b = nullptr;
    if (int rc = leaf_batch(ctx, kind, width, height, depths ? depths[0] : 0, depths ? depths[1] : 0, &b)) return out->status = rc;
    if (int rc = leaf_pair(b, kind, reference, test, reference_len, [&] { return ce_batch_run(b, 1, metric_mask, flags, intensity_target, out); }))
        return out->status = rc;
    return out->status;
}

extern "C" {

int ce_eval_pair(ce_ctx *ctx, const uint8_t *reference, size_t reference_len, const uint8_t *test, size_t test_len,
                 uint32_t width, uint32_t height, uint32_t metric_mask, uint32_t flags, float intensity_target,
                 ce_scores *out)
{
    if (!ctx || !out || !reference || !test) return CE_ERR_INVALID_ARG;
    ce_pair_desc d{reference, reference_len, test, test_len, width, height};
    int rc = ce_eval_batch(ctx, 1, &d, metric_mask, flags, intensity_target, out);
    if (rc != CE_OK) return rc;
    return out->status;
}

// One pair of packed u16 RGB through the context's one-pair deep batch (kept while shape and depths stay the same)
int ce_eval_pair_deep(ce_ctx *ctx, const uint16_t *reference, size_t reference_len, uint32_t ref_depth, const uint16_t *test,
                      size_t test_len, uint32_t test_depth, uint32_t width, uint32_t height, uint32_t metric_mask, uint32_t flags,
                      float intensity_target, ce_scores *out)
{
    const uint32_t depths[2] = {ref_depth, test_depth};
    return eval_pair_wide(ctx, CE_LEAF_DEEP, depths, 6, reference, reference_len, test, test_len, width, height, metric_mask, flags,
                          intensity_target, out);
}

// One pair of packed f32 RGB through the context's one-pair linear batch (kept while the shape stays the same)
int ce_eval_pair_linear(ce_ctx *ctx, const float *reference, size_t reference_len, const float *test, size_t test_len, uint32_t width,
                        uint32_t height, uint32_t metric_mask, uint32_t flags, float intensity_target, ce_scores *out)
{
    return eval_pair_wide(ctx, CE_LEAF_LINEAR, nullptr, 12, reference, reference_len, test, test_len, width, height, metric_mask, flags,
                          intensity_target, out);
}

static int leaf(ce_ctx *ctx, const uint8_t *reference, size_t reference_len, const uint8_t *test, size_t test_len,
                size_t width, size_t height, uint32_t metric, float intensity, double *out)
{
    if (!ctx || !out) return CE_ERR_INVALID_ARG;
    ce_scores s{};
    int rc = ce_eval_pair(ctx, reference, reference_len, test, test_len, (uint32_t)width, (uint32_t)height, metric, 0,
                          intensity, &s);
    if (rc != CE_OK) return rc;
    *out = metric == CE_METRIC_PSNR          ? s.psnr
           : metric == CE_METRIC_SSIMULACRA2 ? s.ssimulacra2
           : metric == CE_METRIC_DSSIM       ? s.dssim
                                             : s.butteraugli;
    return CE_OK;
}

int ce_calculate_psnr(ce_ctx *ctx, const uint8_t *reference, size_t reference_len, const uint8_t *test,
                      size_t test_len, size_t width, size_t height, double *out)
{
    return leaf(ctx, reference, reference_len, test, test_len, width, height, CE_METRIC_PSNR, 0.f, out);
}

int ce_calculate_ssimulacra2(ce_ctx *ctx, const uint8_t *reference, size_t reference_len, const uint8_t *test,
                             size_t test_len, size_t width, size_t height, double *out)
{
    return leaf(ctx, reference, reference_len, test, test_len, width, height, CE_METRIC_SSIMULACRA2, 0.f, out);
}

int ce_calculate_dssim(ce_ctx *ctx, const uint8_t *reference, size_t reference_len, const uint8_t *test,
                       size_t test_len, size_t width, size_t height, double *out)
{
    return leaf(ctx, reference, reference_len, test, test_len, width, height, CE_METRIC_DSSIM, 0.f, out);
}

int ce_calculate_butteraugli(ce_ctx *ctx, const uint8_t *reference, size_t reference_len, const uint8_t *test,
                             size_t test_len, size_t width, size_t height, float intensity_target, double *out)
{
    return leaf(ctx, reference, reference_len, test, test_len, width, height, CE_METRIC_BUTTERAUGLI, intensity_target,
                out);
}

// The one-pair map calls (ce_calculate_butteraugli_diffmap, ce_calculate_dssim_ssim_maps, ce_calculate_ssimulacra2_maps): the
// pair through the context's one-pair RGB8 batch; *out_b is that batch, with the maps of this run.  The caller has checked the
// arguments.
static int leaf_map_run(ce_ctx *ctx, const uint8_t *reference, size_t reference_len, const uint8_t *test, size_t width, size_t height,
                        uint32_t metric, uint32_t flags, float intensity_target, ce_scores *s, ce_batch **out_b)
{
    CE_HIP(ctx, hipSetDevice(ctx->device));
    if (int rc = leaf_batch(ctx, CE_LEAF_RGB8, (uint32_t)width, (uint32_t)height, 0, 0, out_b)) return rc;
    ce_batch *b = *out_b;
    if (int rc = leaf_pair(b, CE_LEAF_RGB8, reference, test, reference_len, [&] { return ce_batch_run(b, 1, metric, flags, intensity_target, s); }))
        return rc;
    return s->status;
}

int ce_calculate_butteraugli_diffmap(ce_ctx *ctx, const uint8_t *reference, size_t reference_len, const uint8_t *test,
                                     size_t test_len, size_t width, size_t height, float intensity_target, double *score,
                                     float *diffmap_out)
{
    if (!ctx || !reference || !test || !score || !diffmap_out) return CE_ERR_INVALID_ARG;
    if (int rc = ce_validate_pair(ctx, reference_len, test_len, width, height)) return rc;
    if (width < 8 || height < 8) return ce_fail(ctx, CE_ERR_TOO_SMALL, "minimum 8x8 for butteraugli");  // src/eval/helpers.rs:89
    if (width > UINT32_MAX || height > UINT32_MAX) return ce_fail(ctx, CE_ERR_INVALID_ARG, "image too large");
    ce_scores s{};
    ce_batch *b = nullptr;
    if (int rc = leaf_map_run(ctx, reference, reference_len, test, width, height, CE_METRIC_BUTTERAUGLI,
                              CE_FLAG_BUTTERAUGLI_DIFFMAP, intensity_target, &s, &b))
        return rc;
    if (int r = ce_batch_butteraugli_diffmap(b, 0, 1, 1, diffmap_out, width * height)) return r;
    *score = s.butteraugli;
    return CE_OK;
}

int ce_calculate_dssim_ssim_maps(ce_ctx *ctx, const uint8_t *reference, size_t reference_len, const uint8_t *test, size_t test_len,
                                 size_t width, size_t height, double *dssim, double *level_ssim, float *maps, size_t maps_floats)
{
    if (!ctx || !reference || !test || !dssim || !level_ssim || !maps) return CE_ERR_INVALID_ARG;
    if (width == 0 || height == 0) return ce_fail(ctx, CE_ERR_INVALID_ARG, "empty image");  // ce_calculate_dssim's order
    if (int rc = ce_validate_pair(ctx, reference_len, test_len, width, height)) return rc;
    if (width > UINT32_MAX || height > UINT32_MAX) return ce_fail(ctx, CE_ERR_INVALID_ARG, "image too large");
    uint32_t lw[CE_DSSIM_MAX_LEVELS], lh[CE_DSSIM_MAX_LEVELS];
    const uint32_t n = ce_plan_dssim_levels((uint32_t)width, (uint32_t)height, CE_DSSIM_MAX_LEVELS, lw, lh);
    size_t want = 0;
    for (uint32_t l = 0; l < n; l++) want += (size_t)lw[l] * lh[l];
    if (maps_floats != want)
        return ce_fail(ctx, CE_ERR_INVALID_ARG, "SSIM maps of every level need " + std::to_string(want) + " floats, got " + std::to_string(maps_floats));
    ce_scores s{};
    ce_batch *b = nullptr;
    if (int rc = leaf_map_run(ctx, reference, reference_len, test, width, height, CE_METRIC_DSSIM, 0, 0.0f, &s, &b))
        return rc;
    size_t off = 0;
    for (uint32_t l = 0; l < CE_DSSIM_MAX_LEVELS; l++) {
        level_ssim[l] = NAN;
        if (l >= n) continue;
        if (int r = ce_batch_dssim_ssim_maps(b, l, 0, 1, 1, maps + off, (size_t)lw[l] * lh[l], &level_ssim[l])) return r;
        off += (size_t)lw[l] * lh[l];
    }
    *dssim = s.dssim;
    return CE_OK;
}

int ce_calculate_ssimulacra2_maps(ce_ctx *ctx, const uint8_t *reference, size_t reference_len, const uint8_t *test, size_t test_len,
                                  size_t width, size_t height, double *score, double *features, float *maps, size_t maps_floats)
{
    if (!ctx || !reference || !test || !score || !features || !maps) return CE_ERR_INVALID_ARG;
    if (width == 0 || height == 0) return ce_fail(ctx, CE_ERR_INVALID_ARG, "empty image");  // ce_calculate_ssimulacra2's order
    if (int rc = ce_validate_pair(ctx, reference_len, test_len, width, height)) return rc;
    if (width > UINT32_MAX || height > UINT32_MAX) return ce_fail(ctx, CE_ERR_INVALID_ARG, "image too large");
    if (width < 8 || height < 8) return ce_fail(ctx, CE_ERR_TOO_SMALL, "minimum 8x8 for ssimulacra2");
    uint32_t sw[CE_SSIM2_MAX_SCALES], sh[CE_SSIM2_MAX_SCALES];
    const uint32_t n = ce_plan_ssim2_scales((uint32_t)width, (uint32_t)height, CE_SSIM2_MAX_SCALES, sw, sh);
    size_t want = 0;
    for (uint32_t s = 0; s < n; s++) want += 9 * (size_t)sw[s] * sh[s];
    if (maps_floats != want)
        return ce_fail(ctx, CE_ERR_INVALID_ARG, "SSIMULACRA2 maps of every scale need " + std::to_string(want) + " floats, got " + std::to_string(maps_floats));
    ce_scores s{};
    ce_batch *b = nullptr;
    if (int rc = leaf_map_run(ctx, reference, reference_len, test, width, height, CE_METRIC_SSIMULACRA2,
                              CE_FLAG_SSIMULACRA2_MAPS, 0.0f, &s, &b))
        return rc;
    double avg[CE_SSIM2_MAX_SCALES * 18];
    CE_HIP(ctx, hipMemcpyAsync(avg, b->s2.avg, sizeof(avg), hipMemcpyDeviceToHost, ctx->stream));
    CE_HIP(ctx, hipStreamSynchronize(ctx->stream));
    for (uint32_t i = 0; i < CE_SSIM2_MAX_SCALES * 18; i++) features[i] = i < b->s2_scales_run * 18 ? avg[i] : NAN;
    size_t off = 0;
    for (uint32_t sc = 0; sc < b->s2_scales_run; sc++)
        for (uint32_t c = 0; c < 3; c++)
            for (uint32_t k = 0; k < 3; k++) {
                const size_t np = (size_t)sw[sc] * sh[sc];
                if (int r = ce_batch_ssimulacra2_maps(b, sc, c, k, 0, 1, 1, maps + off, np, nullptr)) return r;
                off += np;
            }
    *score = s.ssimulacra2;
    return CE_OK;
}

int ce_xyb_roundtrip(ce_ctx *ctx, const uint8_t *rgb, size_t rgb_len, size_t width, size_t height, uint8_t *out)
{
    if (!ctx || !rgb || !out) return CE_ERR_INVALID_ARG;
    if (rgb_len != width * height * 3)
        return ce_fail(ctx, CE_ERR_BAD_LENGTH, "Buffer size mismatch");  // xyb.rs:227
    if (rgb_len == 0) return CE_OK;
    return ce_leaf_roundtrip(ctx, rgb, rgb_len, out, rgb_len,
                          [&](uint8_t *d_in, uint8_t *d_out) { return ce_launch_xyb_roundtrip(ctx, d_in, d_out, width * height); });
}

int ce_rgb8_to_dssim_image(ce_ctx *ctx, const uint8_t *rgb, size_t rgb_len, size_t width, size_t height,
                           float *rgba_out)
{
    if (!ctx || !rgb || !rgba_out) return CE_ERR_INVALID_ARG;
    if (rgb_len != width * height * 3) return ce_fail(ctx, CE_ERR_BAD_LENGTH, "Buffer size mismatch");
    const size_t n = width * height;
    if (n == 0) return CE_OK;
    return ce_leaf_roundtrip(ctx, rgb, rgb_len, rgba_out, n * 4 * sizeof(float), [&](uint8_t *d_in, uint8_t *d_out) {
        return ce_launch_rgb8_to_dssim_image(ctx, d_in, reinterpret_cast<float *>(d_out), n);
    });
}

int ce_image_heuristics_rgb8(ce_ctx *ctx, const uint8_t *rgb, size_t len, size_t width, size_t height, ce_image_heuristics *out)
{
    if (!ctx || !rgb || !out) return CE_ERR_INVALID_ARG;
    if (width > UINT32_MAX || height > UINT32_MAX || (height && width > SIZE_MAX / 3 / height))
        return ce_fail(ctx, CE_ERR_INVALID_ARG, "image heuristics: image dimensions out of range");
    if (len != width * height * 3) return ce_bad_length(ctx, width * height * 3, len);
    if (width < 3 || height < 3)
        return ce_fail(ctx, CE_ERR_TOO_SMALL, "image heuristics need at least 3 x 3 pixels, got " + std::to_string(width) + " x " +
                                               std::to_string(height));
    int rc = ce_leaf_scratch(ctx, len, 0);
    if (rc != CE_OK) return rc;
    std::memcpy(ctx->leaf_h, rgb, len);
    const hipError_t e = hipMemcpyAsync(ctx->leaf_d_in, ctx->leaf_h, len, hipMemcpyHostToDevice, ctx->stream);
    if (e != hipSuccess) return ce_fail(ctx, CE_ERR_BACKEND, std::string("image heuristics upload: ") + hipGetErrorString(e));
    return ce_image_heuristics_run(ctx, ctx->leaf_d_in, len, (uint32_t)width, (uint32_t)height, 1, out);
}

// One pair of packed f32 RGB through the context's one-pair linear batch, which ce_eval_pair_linear shares
int ce_eval_pair_hdr_fidelity(ce_ctx *ctx, const float *reference, size_t reference_len, const float *test, size_t test_len, uint32_t width,
                              uint32_t height, uint32_t depth, float white_nits, ce_hdr_scores *out)
{
    if (!ctx) return CE_ERR_INVALID_ARG;
    if (!out || !reference || !test) return ce_fail(ctx, CE_ERR_INVALID_ARG, "HDR fidelity: null pointer");
    *out = ce_hdr_scores{};
    if (width == 0 || height == 0) return ce_fail(ctx, CE_ERR_INVALID_ARG, "HDR fidelity: empty image");
    if (int rc = ce_hdr_params_check(ctx, depth, white_nits)) return rc;
    const size_t want = (size_t)width * height * 12;
    if (reference_len != want) return ce_bad_length(ctx, want, reference_len);
    if (test_len != want) return ce_bad_length(ctx, want, test_len);
    CE_HIP(ctx, hipSetDevice(ctx->device));
    ce_batch *b = nullptr;
    if (int rc = leaf_batch(ctx, CE_LEAF_LINEAR, width, height, 0, 0, &b)) return rc;
    return leaf_pair(b, CE_LEAF_LINEAR, reference, test, want, [&] { return ce_batch_hdr_fidelity(b, 1, depth, white_nits, out); });
}

// ... and its Delta E ITP map and exceedance counts through the same batch; what concerns the outputs is ce_batch_delta_e_itp_map's
// to refuse
int ce_eval_pair_delta_e_itp_map(ce_ctx *ctx, const float *reference, size_t reference_len, const float *test, size_t test_len, uint32_t width,
                                 uint32_t height, uint32_t depth, float white_nits, uint32_t block, uint32_t *map, size_t map_len,
                                 const uint32_t *thresholds_q20, uint32_t n_thresholds, uint64_t *over)
{
    if (!ctx) return CE_ERR_INVALID_ARG;
    if (!reference || !test) return ce_fail(ctx, CE_ERR_INVALID_ARG, "Delta E ITP map: null pointer");
    if (width == 0 || height == 0) return ce_fail(ctx, CE_ERR_INVALID_ARG, "Delta E ITP map: empty image");
    if (int rc = ce_hdr_params_check(ctx, depth, white_nits)) return rc;
    const size_t want = (size_t)width * height * 12;
    if (reference_len != want) return ce_bad_length(ctx, want, reference_len);
    if (test_len != want) return ce_bad_length(ctx, want, test_len);
    CE_HIP(ctx, hipSetDevice(ctx->device));
    ce_batch *b = nullptr;
    if (int rc = leaf_batch(ctx, CE_LEAF_LINEAR, width, height, 0, 0, &b)) return rc;
    return leaf_pair(b, CE_LEAF_LINEAR, reference, test, want, [&] {
        return ce_batch_delta_e_itp_map(b, 0, 1, depth, white_nits, block, map, map_len, thresholds_q20, n_thresholds, over);
    });
}

// One pair through the context's one-pair RGB8 batch (depth 0) or deep batch of depth / depth into ce_batch_msssim, which
// refuses what concerns levels and the image's size
static int leaf_msssim(ce_ctx *ctx, ce_leaf_kind kind, uint32_t depth, size_t bytes_per_pixel, const void *reference, size_t reference_len,
                       const void *test, size_t test_len, uint32_t width, uint32_t height, uint32_t levels, ce_msssim_scores *out)
{
    if (!ctx) return CE_ERR_INVALID_ARG;
    if (!out || !reference || !test) return ce_fail(ctx, CE_ERR_INVALID_ARG, "MS-SSIM: null pointer");
    *out = ce_msssim_scores{};
    if (kind == CE_LEAF_DEEP && !ce_deep_depth_ok(depth))
        return ce_fail(ctx, CE_ERR_INVALID_ARG, "MS-SSIM: depth must be 8, 10, 12 or 16 bits, got " + std::to_string(depth));
    if (width == 0 || height == 0) return ce_fail(ctx, CE_ERR_INVALID_ARG, "MS-SSIM: empty image");
    const size_t want = (size_t)width * height * bytes_per_pixel;
    if (reference_len != want) return ce_bad_length(ctx, want, reference_len);
    if (test_len != want) return ce_bad_length(ctx, want, test_len);
    uint32_t n = 0, lw[CE_MSSSIM_LEVELS], lh[CE_MSSSIM_LEVELS];
    if (int rc = ce_msssim_levels(width, height, levels, &n, lw, lh)) return ce_fail(ctx, rc, ce_last_error(nullptr));  // before a batch is made
    CE_HIP(ctx, hipSetDevice(ctx->device));
    ce_batch *b = nullptr;
    if (int rc = leaf_batch(ctx, kind, width, height, depth, depth, &b)) return rc;
    return leaf_pair(b, kind, reference, test, want, [&] { return ce_batch_msssim(b, 1, levels, out); });
}

int ce_eval_pair_msssim(ce_ctx *ctx, const uint8_t *reference, size_t reference_len, const uint8_t *test, size_t test_len, uint32_t width,
                        uint32_t height, uint32_t levels, ce_msssim_scores *out)
{
    return leaf_msssim(ctx, CE_LEAF_RGB8, 0, 3, reference, reference_len, test, test_len, width, height, levels, out);
}

int ce_eval_pair_msssim_deep(ce_ctx *ctx, const uint16_t *reference, size_t reference_len, const uint16_t *test, size_t test_len,
                             uint32_t depth, uint32_t width, uint32_t height, uint32_t levels, ce_msssim_scores *out)
{
    return leaf_msssim(ctx, CE_LEAF_DEEP, depth, 6, reference, reference_len, test, test_len, width, height, levels, out);
}

// One pair through the context's one-pair RGB8 batch (depths 0 / 0) or deep batch of ref_depth / test_depth into
// ce_batch_ciede2000, which refuses what concerns the thresholds
static int leaf_ciede2000(ce_ctx *ctx, ce_leaf_kind kind, uint32_t ref_depth, uint32_t test_depth, size_t bytes_per_pixel, const void *reference,
                          size_t reference_len, const void *test, size_t test_len, uint32_t width, uint32_t height,
                          const uint32_t *thresholds_q20, uint32_t n_thresholds, ce_ciede2000_scores *out)
{
    if (!ctx) return CE_ERR_INVALID_ARG;
    if (!out || !reference || !test) return ce_fail(ctx, CE_ERR_INVALID_ARG, "CIEDE2000: null pointer");
    *out = ce_ciede2000_scores{};
    if (kind == CE_LEAF_DEEP && (!ce_deep_depth_ok(ref_depth) || !ce_deep_depth_ok(test_depth)))
        return ce_fail(ctx, CE_ERR_INVALID_ARG, "CIEDE2000: depths must be 8, 10, 12 or 16 bits, got " + std::to_string(ref_depth) + " / " +
                                                 std::to_string(test_depth));
    if (width == 0 || height == 0) return ce_fail(ctx, CE_ERR_INVALID_ARG, "CIEDE2000: empty image");
    const size_t want = (size_t)width * height * bytes_per_pixel;
    if (reference_len != want) return ce_bad_length(ctx, want, reference_len);
    if (test_len != want) return ce_bad_length(ctx, want, test_len);
    CE_HIP(ctx, hipSetDevice(ctx->device));
    ce_batch *b = nullptr;
    if (int rc = leaf_batch(ctx, kind, width, height, ref_depth, test_depth, &b)) return rc;
    return leaf_pair(b, kind, reference, test, want, [&] { return ce_batch_ciede2000(b, 1, thresholds_q20, n_thresholds, out); });
}

int ce_eval_pair_ciede2000(ce_ctx *ctx, const uint8_t *reference, size_t reference_len, const uint8_t *test, size_t test_len, uint32_t width,
                           uint32_t height, const uint32_t *thresholds_q20, uint32_t n_thresholds, ce_ciede2000_scores *out)
{
    return leaf_ciede2000(ctx, CE_LEAF_RGB8, 0, 0, 3, reference, reference_len, test, test_len, width, height, thresholds_q20, n_thresholds, out);
}

int ce_eval_pair_ciede2000_deep(ce_ctx *ctx, const uint16_t *reference, size_t reference_len, const uint16_t *test, size_t test_len,
                                uint32_t ref_depth, uint32_t test_depth, uint32_t width, uint32_t height, const uint32_t *thresholds_q20,
                                uint32_t n_thresholds, ce_ciede2000_scores *out)
{
    return leaf_ciede2000(ctx, CE_LEAF_DEEP, ref_depth, test_depth, 6, reference, reference_len, test, test_len, width, height, thresholds_q20,
                          n_thresholds, out);
}

// ... and its CIEDE2000 map and exceedance counts through the same batches, as leaf_ciede2000; what concerns what, block and the
// outputs is ce_batch_ciede2000_map's to refuse
static int leaf_ciede2000_map(ce_ctx *ctx, ce_leaf_kind kind, uint32_t ref_depth, uint32_t test_depth, size_t bytes_per_pixel, const void *reference,
                              size_t reference_len, const void *test, size_t test_len, uint32_t width, uint32_t height, uint32_t what,
                              uint32_t block, uint32_t *map, size_t map_len, const uint32_t *thresholds_q20, uint32_t n_thresholds, uint64_t *over)
{
    if (!ctx) return CE_ERR_INVALID_ARG;
    if (!reference || !test) return ce_fail(ctx, CE_ERR_INVALID_ARG, "CIEDE2000 map: null pointer");
    if (kind == CE_LEAF_DEEP && (!ce_deep_depth_ok(ref_depth) || !ce_deep_depth_ok(test_depth)))
        return ce_fail(ctx, CE_ERR_INVALID_ARG, "CIEDE2000 map: depths must be 8, 10, 12 or 16 bits, got " + std::to_string(ref_depth) + " / " +
                                                 std::to_string(test_depth));
    if (width == 0 || height == 0) return ce_fail(ctx, CE_ERR_INVALID_ARG, "CIEDE2000 map: empty image");
    const size_t want = (size_t)width * height * bytes_per_pixel;
    if (reference_len != want) return ce_bad_length(ctx, want, reference_len);
    if (test_len != want) return ce_bad_length(ctx, want, test_len);
    CE_HIP(ctx, hipSetDevice(ctx->device));
    ce_batch *b = nullptr;
    if (int rc = leaf_batch(ctx, kind, width, height, ref_depth, test_depth, &b)) return rc;
    return leaf_pair(b, kind, reference, test, want, [&] {
        return ce_batch_ciede2000_map(b, 0, 1, what, block, map, map_len, thresholds_q20, n_thresholds, over);
    });
}

int ce_eval_pair_ciede2000_map(ce_ctx *ctx, const uint8_t *reference, size_t reference_len, const uint8_t *test, size_t test_len, uint32_t width,
                               uint32_t height, uint32_t what, uint32_t block, uint32_t *map, size_t map_len, const uint32_t *thresholds_q20,
                               uint32_t n_thresholds, uint64_t *over)
{
    return leaf_ciede2000_map(ctx, CE_LEAF_RGB8, 0, 0, 3, reference, reference_len, test, test_len, width, height, what, block, map, map_len,
                              thresholds_q20, n_thresholds, over);
}

int ce_eval_pair_ciede2000_map_deep(ce_ctx *ctx, const uint16_t *reference, size_t reference_len, const uint16_t *test, size_t test_len,
                                    uint32_t ref_depth, uint32_t test_depth, uint32_t width, uint32_t height, uint32_t what, uint32_t block,
                                    uint32_t *map, size_t map_len, const uint32_t *thresholds_q20, uint32_t n_thresholds, uint64_t *over)
{
    return leaf_ciede2000_map(ctx, CE_LEAF_DEEP, ref_depth, test_depth, 6, reference, reference_len, test, test_len, width, height, what, block,
                              map, map_len, thresholds_q20, n_thresholds, over);
}

// ... and its SSIM / MS-SSIM map and exceedance counts through the same batches, as leaf_msssim; what concerns level, what, block
// and the outputs is ce_batch_msssim_map's to refuse
static int leaf_msssim_map(ce_ctx *ctx, ce_leaf_kind kind, uint32_t depth, size_t bytes_per_pixel, const void *reference, size_t reference_len,
                           const void *test, size_t test_len, uint32_t width, uint32_t height, uint32_t levels, uint32_t level, uint32_t what,
                           uint32_t block, uint32_t *map, size_t map_len, const uint32_t *thresholds_q32, uint32_t n_thresholds, uint64_t *over)
{
    if (!ctx) return CE_ERR_INVALID_ARG;
    if (!reference || !test) return ce_fail(ctx, CE_ERR_INVALID_ARG, "MS-SSIM map: null pointer");
    if (kind == CE_LEAF_DEEP && !ce_deep_depth_ok(depth))
        return ce_fail(ctx, CE_ERR_INVALID_ARG, "MS-SSIM map: depth must be 8, 10, 12 or 16 bits, got " + std::to_string(depth));
    if (width == 0 || height == 0) return ce_fail(ctx, CE_ERR_INVALID_ARG, "MS-SSIM map: empty image");
    const size_t want = (size_t)width * height * bytes_per_pixel;
    if (reference_len != want) return ce_bad_length(ctx, want, reference_len);
    if (test_len != want) return ce_bad_length(ctx, want, test_len);
    uint32_t n = 0, lw[CE_MSSSIM_LEVELS], lh[CE_MSSSIM_LEVELS];
    if (int rc = ce_msssim_levels(width, height, levels, &n, lw, lh)) return ce_fail(ctx, rc, ce_last_error(nullptr));  // before a batch is made
    CE_HIP(ctx, hipSetDevice(ctx->device));
    ce_batch *b = nullptr;
    if (int rc = leaf_batch(ctx, kind, width, height, depth, depth, &b)) return rc;
    return leaf_pair(b, kind, reference, test, want, [&] {
        return ce_batch_msssim_map(b, 0, 1, levels, level, what, block, map, map_len, thresholds_q32, n_thresholds, over);
    });
}

int ce_eval_pair_msssim_map(ce_ctx *ctx, const uint8_t *reference, size_t reference_len, const uint8_t *test, size_t test_len, uint32_t width,
                            uint32_t height, uint32_t levels, uint32_t level, uint32_t what, uint32_t block, uint32_t *map, size_t map_len,
                            const uint32_t *thresholds_q32, uint32_t n_thresholds, uint64_t *over)
{
    return leaf_msssim_map(ctx, CE_LEAF_RGB8, 0, 3, reference, reference_len, test, test_len, width, height, levels, level, what, block, map,
                           map_len, thresholds_q32, n_thresholds, over);
}

int ce_eval_pair_msssim_map_deep(ce_ctx *ctx, const uint16_t *reference, size_t reference_len, const uint16_t *test, size_t test_len,
                                 uint32_t depth, uint32_t width, uint32_t height, uint32_t levels, uint32_t level, uint32_t what, uint32_t block,
                                 uint32_t *map, size_t map_len, const uint32_t *thresholds_q32, uint32_t n_thresholds, uint64_t *over)
{
    return leaf_msssim_map(ctx, CE_LEAF_DEEP, depth, 6, reference, reference_len, test, test_len, width, height, levels, level, what, block, map,
                           map_len, thresholds_q32, n_thresholds, over);
}

}  // extern "C"
