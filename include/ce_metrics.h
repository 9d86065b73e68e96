/*
 * ce_metrics.h — C ABI of libce_metrics_hip.so, the MI355X (gfx950) backend for the
 * perceptual-metric hot path of imazen/codec-eval.
 *
 * Every entry point replaces one reference interface; the citation after each
 * declaration is the Rust item (path relative to the reference checkout) whose
 * FFI binding would call it.  Conventions (reference: SURVEY.md §8b):
 *
 *   pixels     tightly packed interleaved RGB8, row-major, no stride
 *              (src/metrics/ssimulacra2.rs:41,72; src/eval/session.rs:98-117)
 *   ownership  every pointer is borrowed for the duration of the call only; the
 *              library copies what it needs and owns all device memory
 *   errors     integer status, never abort/panic; ce_last_error() gives the text.
 *              CE_ERR_DIM_MISMATCH  <-> Error::DimensionMismatch  (src/error.rs:31-38)
 *              CE_ERR_BAD_LENGTH    <-> Error::MetricCalculation{"Invalid image size"}
 *                                       (src/metrics/ssimulacra2.rs:73-82)
 *              CE_ERR_TOO_SMALL     <-> Error::MetricCalculation from the metric crate
 *                                       for images under 8x8 (src/eval/helpers.rs:89)
 *              CE_ERR_BACKEND       <-> Error::MetricCalculation{reason: backend text}
 *              PSNR in the reference asserts (src/metrics/mod.rs:313-314); here it
 *              returns the code and the Rust shim re-raises the panic.
 *   results    double, as MetricResult's Option<f64> (src/metrics/mod.rs:140-149)
 *   threading  one in-flight call per context (GpuSsim2::compute takes &mut self,
 *              crates/codec-iter/src/gpu.rs:83); any number of contexts per device.
 *              Process-wide state: one counter per device of launched-and-uncollected
 *              batches, read by ce_batch_launch to choose between running a batch's metric
 *              chains side by side or back to back (a scheduling hint: it never changes a
 *              score), and the environment knobs DESIGN.md lists, read once.
 *   no torch / no C++ types in any signature.
 */
#ifndef CE_METRICS_H
#define CE_METRICS_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct ce_ctx ce_ctx;     /* device + stream + scratch pool       */
typedef struct ce_batch ce_batch; /* HBM-resident grid of (ref, test) pairs of one shape */
typedef struct ce_ref ce_ref;     /* one reference image held on device   */
typedef struct ce_lut ce_lut;     /* one colour transform (ICC -> sRGB) held on device as a 2^24-entry table */

enum ce_status {
    CE_OK = 0,
    CE_ERR_DIM_MISMATCH = 1,
    CE_ERR_BAD_LENGTH = 2,
    CE_ERR_TOO_SMALL = 3,
    CE_ERR_BACKEND = 4,
    CE_ERR_INVALID_ARG = 5
};

/* MetricConfig (src/metrics/mod.rs:46-63) as a bit mask */
enum ce_metric {
    CE_METRIC_DSSIM = 1u << 0,
    CE_METRIC_SSIMULACRA2 = 1u << 1,
    CE_METRIC_BUTTERAUGLI = 1u << 2,
    CE_METRIC_PSNR = 1u << 3
};
enum ce_flag {
    CE_FLAG_XYB_ROUNDTRIP = 1u << 0, /* MetricConfig::xyb_roundtrip: reference side only (session.rs:447-456) */
    /* ButteraugliResult.diffmap (src/metrics/prelude.rs:64-65): with CE_METRIC_BUTTERAUGLI, ce_batch_launch / ce_batch_run
     * and the compares of a ce_ref created with it also keep every pair's full-resolution diffmap on the device (4 bytes per
     * pixel and pair, allocated by the first such launch; not counted by ce_estimate_batch_bytes), to be read with
     * ce_batch_butteraugli_diffmap / ce_ref_butteraugli_diffmap.  Scores are the same with and without it.
     * ce_eval_batch, ce_eval_batch_lut and ce_eval_pair return CE_ERR_INVALID_ARG for it: their batches do not outlive the
     * call. */
    CE_FLAG_BUTTERAUGLI_DIFFMAP = 1u << 1,
    /* The per-pixel terms SSIMULACRA2 pools (ssim_map / edge_diff_map of the lineage behind src/metrics/ssimulacra2.rs:96):
     * with CE_METRIC_SSIMULACRA2, ce_batch_launch / ce_batch_run and the compares of a ce_ref created with it also keep
     * every pair's nine maps per scale (ce_ssim2_map x 3 XYB channels) on the device (36 bytes per pixel of every scale and
     * pair, about 20 MB per 768x512 pair; allocated by the first such launch, not counted by ce_estimate_batch_bytes), to
     * be read with ce_batch_ssimulacra2_maps / ce_ref_ssimulacra2_maps.  Scores are the same with and without it.
     * ce_eval_batch, ce_eval_batch_lut and ce_eval_pair return CE_ERR_INVALID_ARG for it. */
    CE_FLAG_SSIMULACRA2_MAPS = 1u << 2
};

#define CE_DEFAULT_INTENSITY_TARGET 80.0f /* src/metrics/butteraugli.rs:94 */
#define CE_DSSIM_MAX_LEVELS 5 /* dssim-core's scale weights: at most this many SsimMap per compare */
#define CE_SSIM2_MAX_SCALES 6 /* Msssim's NUM_SCALES (lineage of src/metrics/ssimulacra2.rs:96) */

/* SSIMULACRA2's three per-pixel error terms of one XYB channel at one scale, each >= 0 (ssim_map and edge_diff_map of
 * the lineage).  The score pools each one's mean and 4-norm.
 *   SSIM         1 - SSIM of the blurred statistics, clamped at 0: structural error
 *   ARTIFACT     max((1 + |test - mu_test|) / (1 + |ref - mu_ref|) - 1, 0): edges or texture the test adds (ringing, blocking)
 *   DETAIL_LOST  max(1 - (1 + |test - mu_test|) / (1 + |ref - mu_ref|), 0): edges or texture the test lost (blur) */
enum ce_ssim2_map { CE_SSIM2_MAP_SSIM = 0, CE_SSIM2_MAP_ARTIFACT = 1, CE_SSIM2_MAP_DETAIL_LOST = 2 };

/* MetricResult (src/metrics/mod.rs:140-149): a score is meaningful iff its bit is
 * set in `valid`; `status` is the ce_status of this pair. */
typedef struct ce_scores {
    double dssim;
    double ssimulacra2;
    double butteraugli;
    double psnr;
    uint32_t valid;
    int32_t status;
} ce_scores;

/* one work item of the (image x codec x quality) grid */
typedef struct ce_pair_desc {
    const uint8_t *reference;
    size_t reference_len;
    const uint8_t *test;
    size_t test_len;
    uint32_t width;
    uint32_t height;
} ce_pair_desc;

/* ---- library / device -------------------------------------------------------- */
const char *ce_version(void);
int ce_device_count(void); /* number of visible HIP devices; <0 on runtime failure */

/* GpuSsim2::new (crates/codec-iter/src/gpu.rs:40-80) without the fixed-shape limit:
 * scratch is keyed by (w,h) and grows on demand. */
int ce_ctx_create(int device, ce_ctx **out);
/* same, launching on a caller-owned hipStream_t (passed as void*); NULL (0) = own stream, exactly ce_ctx_create: the
 * legacy default stream, whose handle is 0, cannot be adopted (nor can a framework's default stream that is it: pass a
 * stream the framework created, INTEGRATION.md "Stream order").  The context never
 * destroys a caller's stream; ce_ctx_destroy synchronises it.
 *
 * Stream order.  "The context's stream" is ce_ctx_stream(): the caller's, or the context's own - a caller may enqueue on
 * either.  The library fans a call out to further streams of its own (metric chains, upload streams, helper threads) and
 * fences them so that, seen from outside, every call behaves as if its device work ran on the context's stream at the
 * point of the call:
 *  - Work the caller enqueued on the context's stream BEFORE a call (a decoder's kernels or copies into the slabs of
 *    ce_batch_reference_slab / ce_batch_test_slab, followed by ce_batch_references_changed where references changed) is
 *    visible to that call's device work.  No host synchronisation is needed in between.
 *  - Work enqueued on the context's stream AFTER a call returns runs after that call's device work, a launch that has not
 *    been collected included.
 *  - No other stream is ever waited for.  What a call reads from device memory the caller wrote on another stream
 *    (slabs, CE_MEM_DEVICE planes) must be complete before the call, or that stream be made to precede the context's
 *    (hipStreamWaitEvent) before the call.  (HIP maps streams onto a few hardware queues and may run a stream behind
 *    another that shares its queue; the library adds no such dependency and none may be relied on.)
 *  - A ce_batch_set_*, ce_batch_bind_pair or ce_batch_resample into a batch issued after ce_batch_launch does not
 *    disturb that launch: it is ordered behind the launch's reads, whichever stream carries it, and the launch's scores
 *    and maps are those of the images it was launched on.
 *  - Host sources of ce_batch_set_* are consumed on return (copied to page-locked staging), whatever is still queued.
 * ce_batch_launch, the setters and ce_batch_resample* return without waiting for the stream (a launch waits, for the
 * batch's own previous launch only, when the pair bindings or the pair count changed since: it rebuilds its tables, and
 * a setter waits for a staging buffer it used a few images ago).  Calls that return results to the host
 * (ce_batch_run, ce_batch_collect, the leaves, ce_batch_image_heuristics, ce_batch_hdr_fidelity, map readouts) wait for what
 * they return. */
int ce_ctx_create_on_stream(int device, void *hip_stream, ce_ctx **out);
/* Drop for GpuSsim2 (gpu.rs:118-133): synchronises the stream, then frees */
void ce_ctx_destroy(ce_ctx *ctx);
int ce_ctx_synchronize(ce_ctx *ctx);
void *ce_ctx_stream(ce_ctx *ctx); /* the hipStream_t kernels are launched on */
const char *ce_last_error(const ce_ctx *ctx);

/* ---- leaf metric calls: one per reference leaf function ------------------------ */
/* calculate_psnr                       src/metrics/mod.rs:312 */
int ce_calculate_psnr(ce_ctx *ctx, const uint8_t *reference, size_t reference_len, const uint8_t *test,
                      size_t test_len, size_t width, size_t height, double *out);
/* calculate_ssimulacra2                src/metrics/ssimulacra2.rs:59 ; GpuSsim2::compute gpu.rs:83 */
int ce_calculate_ssimulacra2(ce_ctx *ctx, const uint8_t *reference, size_t reference_len,
                             const uint8_t *test, size_t test_len, size_t width, size_t height,
                             double *out);
/* rgb8_to_dssim_image x2 + calculate_dssim   src/metrics/dssim.rs:102,40 (session.rs:467-476) */
int ce_calculate_dssim(ce_ctx *ctx, const uint8_t *reference, size_t reference_len, const uint8_t *test,
                       size_t test_len, size_t width, size_t height, double *out);
/* calculate_butteraugli / _with_intensity    src/metrics/butteraugli.rs:45,99 */
int ce_calculate_butteraugli(ce_ctx *ctx, const uint8_t *reference, size_t reference_len,
                             const uint8_t *test, size_t test_len, size_t width, size_t height,
                             float intensity_target, double *out);
/* ButteraugliResult{score, diffmap}: src/metrics/prelude.rs:64-65; butteraugli.rs:45,99.  diffmap_out: w*h floats */
int ce_calculate_butteraugli_diffmap(ce_ctx *ctx, const uint8_t *reference, size_t reference_len, const uint8_t *test,
                                     size_t test_len, size_t width, size_t height, float intensity_target,
                                     double *score, float *diffmap_out);
/* DSSIM's SsimMap (dssim-core, re-exported at src/metrics/prelude.rs:45; Dssim::compare returns (Val, Vec<SsimMap>),
 * which src/metrics/dssim.rs:68 drops as _ssim_maps).  An SsimMap is one scale's per-pixel SSIM image of the channel-
 * averaged statistics (map) and that scale's pooled score (ssim).
 * Level geometry, the rule of Dssim::create_image: a level is halved (floor) only while it is at least 8 x 8, at most
 * CE_DSSIM_MAX_LEVELS levels; level_w / level_h have CE_DSSIM_MAX_LEVELS entries.  A pure host function (no context, works
 * without a device); CE_ERR_INVALID_ARG for width or height 0 or a null pointer. */
int ce_dssim_levels(uint32_t width, uint32_t height, uint32_t *n_levels, uint32_t *level_w, uint32_t *level_h);
/* The one-pair call: Dssim::compare with every scale's map kept (Dssim::set_save_ssim_maps).  dssim as ce_calculate_dssim;
 * level_ssim[CE_DSSIM_MAX_LEVELS] the levels' SsimMap.ssim (NaN past the image's level count); maps every level's full map,
 * level after level, row-major; maps_floats must be the sum of w_l * h_l over the levels (ce_dssim_levels).  Length and
 * dimension errors as ce_calculate_dssim. */
int ce_calculate_dssim_ssim_maps(ce_ctx *ctx, const uint8_t *reference, size_t reference_len, const uint8_t *test,
                                 size_t test_len, size_t width, size_t height, double *dssim, double *level_ssim,
                                 float *maps, size_t maps_floats);
/* SSIMULACRA2's scale geometry (Msssim's loop behind src/metrics/ssimulacra2.rs:96): scale 0 is the image; a scale exists
 * while its parent is at least 8 x 8 and is the parent halved with ceiling, at most CE_SSIM2_MAX_SCALES scales (0 below
 * 8 x 8).  scale_w / scale_h have CE_SSIM2_MAX_SCALES entries.  A pure host function (no context, works without a
 * device); CE_ERR_INVALID_ARG for width or height 0 or a null pointer. */
int ce_ssimulacra2_scales(uint32_t width, uint32_t height, uint32_t *n_scales, uint32_t *scale_w, uint32_t *scale_h);
/* The one-pair call: calculate_ssimulacra2 (src/metrics/ssimulacra2.rs:59) with everything it pools kept.  score as
 * ce_calculate_ssimulacra2; features = [CE_SSIM2_MAX_SCALES][3][6] doubles, the 108 pooled values the score weighs
 * ([scale][channel]{ssim mean, ssim 4-norm, artifact mean, artifact 4-norm, detail mean, detail 4-norm}; NaN past the
 * image's scales); maps = every scale's [channel][kind][h_s][w_s] floats, scale after scale; maps_floats must be
 * 9 * the sum of w_s * h_s (ce_ssimulacra2_scales).  Length and dimension errors as ce_calculate_ssimulacra2. */
int ce_calculate_ssimulacra2_maps(ce_ctx *ctx, const uint8_t *reference, size_t reference_len, const uint8_t *test,
                                  size_t test_len, size_t width, size_t height, double *score, double *features,
                                  float *maps, size_t maps_floats);
/* xyb_roundtrip                         src/metrics/xyb.rs:225 ; out has rgb_len bytes */
int ce_xyb_roundtrip(ce_ctx *ctx, const uint8_t *rgb, size_t rgb_len, size_t width, size_t height,
                     uint8_t *out);
/* rgb8_to_dssim_image                   src/metrics/dssim.rs:102 ; out has 4*w*h floats (a = 1.0) */
int ce_rgb8_to_dssim_image(ce_ctx *ctx, const uint8_t *rgb, size_t rgb_len, size_t width, size_t height,
                           float *rgba_out);

/* ---- dispatcher --------------------------------------------------------------- */
/* EvalSession::calculate_metrics        src/eval/session.rs:437-497
 * evaluate_single                       src/eval/helpers.rs:105-173 */
int ce_eval_pair(ce_ctx *ctx, const uint8_t *reference, size_t reference_len, const uint8_t *test,
                 size_t test_len, uint32_t width, uint32_t height, uint32_t metric_mask, uint32_t flags,
                 float intensity_target, ce_scores *out);

/* The (codec x quality) double loop of EvalSession::evaluate_image (session.rs:375-376)
 * and images.par_iter() of crates/codec-compare/src/full_comparison.rs:319-328, as one
 * call: n independent pairs, any mix of shapes (bucketed by shape internally).
 * Per-pair failures are reported in out[i].status; the return value is CE_OK unless the
 * call itself could not run. */
int ce_eval_batch(ce_ctx *ctx, size_t n, const ce_pair_desc *pairs, uint32_t metric_mask, uint32_t flags,
                  float intensity_target, ce_scores *out);
/* the same with a colour table per pair for the DISTORTED image (NULL entries / a NULL array: none): the decoded image's
 * ICC -> sRGB step of evaluate_image (session.rs:394, ImageData::to_rgb8_srgb) runs on the device - see ce_lut_create */
int ce_eval_batch_lut(ce_ctx *ctx, size_t n, const ce_pair_desc *pairs, const ce_lut *const *test_luts, uint32_t metric_mask,
                      uint32_t flags, float intensity_target, ce_scores *out);

/* Memory planning for callers that size their own batches (EvalSession::evaluate_corpus streams a corpus through
 * batches that fit the device): an upper estimate of the device bytes a batch of this shape holds once the metrics
 * in metric_mask have run, and the device's free / total memory.  ce_eval_batch uses the same estimate to split a
 * grid that does not fit into chunks (each at most a third of the free memory; CE_EVAL_BATCH_BYTES overrides). */
size_t ce_estimate_batch_bytes(uint32_t width, uint32_t height, uint32_t n_refs, uint32_t n_pairs, uint32_t metric_mask);
int ce_ctx_memory_info(ce_ctx *ctx, size_t *free_bytes, size_t *total_bytes);

/* Page-locked host memory for the images a caller hands to ce_eval_batch / ce_ref_compare*, which return only after their
 * kernels: buffers from here are copied by the DMA engines straight from the caller's memory (one asynchronous copy per
 * image, overlapped with the kernels of the previous chunk).  Any other host pointer, and every image given to
 * ce_batch_set_* (which return before the copy is done), first goes through the library's own page-locked staging ring.
 * A decoder writes its output into such a buffer and scores it in place - the role of the cudarse pinned buffers behind
 * GpuSsim2 (crates/codec-iter/src/gpu.rs:96-108).  Freed with ce_host_free (before or after the context is gone). */
int ce_host_alloc(ce_ctx *ctx, size_t bytes, void **out);
int ce_host_free(ce_ctx *ctx, void *p);

/* ---- HBM-resident grid (what bench.py times; inputs already on device) ---------- */
/* One shape, up to max_refs reference images and max_pairs (reference, test) items. */
int ce_batch_create(ce_ctx *ctx, uint32_t width, uint32_t height, uint32_t max_refs, uint32_t max_pairs,
                    ce_batch **out);
void ce_batch_destroy(ce_batch *b);
/* host -> device copies (pinned staging inside) */
int ce_batch_set_reference(ce_batch *b, uint32_t ref_index, const uint8_t *rgb, size_t len);
int ce_batch_set_test(ce_batch *b, uint32_t pair_index, uint32_t ref_index, const uint8_t *rgb, size_t len);
/* Decoded-image ingest: the same two calls for pixels as a decoder hands them over.  The conversion to the
 * packed RGB8 the metrics read happens on the device (no per-pixel pass on the host):
 *   CE_PIXEL_RGBA8         alpha dropped          ImageData::to_rgb8_vec, src/eval/session.rs:98-117
 *   CE_PIXEL_RGB16_10BIT   ((v*255+512)/1023).min(255) per sample, u16 little endian
 *   CE_PIXEL_RGBA16_10BIT  both                   to_8bit / pixel_data_to_rgb8, crates/codec-iter/src/avif_config.rs:122-170
 * len is in bytes and must be width * height * bytes-per-pixel of the format. */
enum {
    CE_PIXEL_RGB8 = 0,
    CE_PIXEL_RGBA8 = 1,
    CE_PIXEL_RGB16_10BIT = 2,
    CE_PIXEL_RGBA16_10BIT = 3
};
int ce_batch_set_reference_fmt(ce_batch *b, uint32_t ref_index, const void *pixels, size_t len, int format);
int ce_batch_set_test_fmt(ce_batch *b, uint32_t pair_index, uint32_t ref_index, const void *pixels, size_t len, int format);
/* ICC -> sRGB on the device, EXACTLY (transform_to_srgb, src/metrics/icc.rs:69-103, called on every decoded image at
 * src/eval/session.rs:394 through ImageData::to_rgb8_srgb).  The reference's transform (moxcms, 8-bit RGB -> 8-bit RGB)
 * is a pure function of a pixel's three bytes, so the table of its outputs on all 2^24 colours reproduces it bit for bit:
 * the host runs ITS colour management once per profile over the identity colour cube (50 MB, tens of milliseconds) and
 * the device applies the table to every decoded image of that profile - no per-pixel colour management on the host and
 * no interpolation error.  table[((r << 16) | (g << 8) | b) * 3 + c] = channel c of the transformed colour;
 * table_len must be 3 * 2^24.  A table belongs to its context's device and must be destroyed before the context. */
int ce_lut_create(ce_ctx *ctx, const uint8_t *table, size_t table_len, ce_lut **out);
void ce_lut_destroy(ce_lut *lut);
/* ce_batch_set_{reference,test}_fmt followed by the table, all on the device (lut == NULL: no transform) */
int ce_batch_set_reference_lut(ce_batch *b, uint32_t ref_index, const void *pixels, size_t len, int format, const ce_lut *lut);
int ce_batch_set_test_lut(ce_batch *b, uint32_t pair_index, uint32_t ref_index, const void *pixels, size_t len, int format,
                          const ce_lut *lut);
/* device pointers of the packed u8 slabs ([max_refs][h][w][3], [max_pairs][h][w][3]) so a caller that
 * already has pixels in HBM (e.g. a GPU decoder) can write them in place.
 * A batch keeps what its metrics derive from the references alone (the XYB roundtrip, SSIMULACRA2's XYB pyramid, DSSIM's
 * img / mu / sq pyramid, Butteraugli's PsychoImage and mask planes) from one launch to the next and rebuilds it only after
 * a reference has been written.  Every ce_batch_set_reference*, ce_batch_resample into the batch and ce_eval_batch says so
 * itself; a write through the slab pointer is invisible to the library.  ce_batch_reference_slab therefore drops that
 * state when it hands the pointer out, and a caller that KEEPS the pointer must, after writing references through it and
 * before the next launch, either fetch the pointer again or call ce_batch_references_changed (which drops the state and
 * does nothing else; CE_ERR_INVALID_ARG for a null batch) - otherwise that launch scores against the planes of the old
 * references.  The test slab has no such rule: nothing derived from a test image outlives a launch. */
void *ce_batch_reference_slab(ce_batch *b);
int ce_batch_references_changed(ce_batch *b);
void *ce_batch_test_slab(ce_batch *b);
/* builds[k] = launches of this batch so far that had to (re)build the reference-side state of SSIMULACRA2 (k = 0),
 * DSSIM (1), Butteraugli (2): what ce_ref_stats returns for a handle.  A launch rebuilds a metric's state when a reference
 * was written since it was built, when it uses more references than the state covers, when Butteraugli's intensity target
 * or the CE_FLAG_XYB_ROUNDTRIP flag differs from the launch that built it, or when the metric has not run on the batch
 * yet; rebinding pairs and replacing test images rebuild nothing.  CE_KEEP_REFERENCE_STATE=0 in the environment (read once
 * per process; a measurement switch, no score depends on it) makes every launch of an ordinary batch rebuild. */
int ce_batch_ref_stats(const ce_batch *b, uint32_t builds[3]);
int ce_batch_bind_pair(ce_batch *b, uint32_t pair_index, uint32_t ref_index);
/* run the hot path over pairs [0, n_pairs); blocks until scores are on the host */
int ce_batch_run(ce_batch *b, uint32_t n_pairs, uint32_t metric_mask, uint32_t flags, float intensity_target,
                 ce_scores *out);
/* same, without the final wait (for back-to-back timed steps and pipelines of several batches): the launch queues the
 * kernels and, behind them, the copy of the scores into the batch's page-locked buffer; ce_batch_collect waits for THAT
 * launch only (not for batches launched after it on the same context) and converts the first n_pairs scores
 * (n_pairs <= the launched count, CE_ERR_INVALID_ARG otherwise).
 *
 * What one launch takes.  ce_batch_create accepts any max_pairs, and the calls that are one kernel
 * over (blocks, pairs) - CE_METRIC_PSNR here, ce_batch_ciede2000, ce_batch_hdr_fidelity, ce_batch_delta_e_itp_map, and
 * ce_batch_msssim / ce_batch_msssim_map / ce_batch_plane_fidelity - score any n_pairs <= max_pairs: they CHUNK the pair
 * range into kernel launches of at most CE_LAUNCH_GRID_MAX pairs.  CE_METRIC_DSSIM, CE_METRIC_SSIMULACRA2 and
 * CE_METRIC_BUTTERAUGLI do not chunk; a launch that asks for any of them is REFUSED - CE_ERR_INVALID_ARG, the limit in
 * ce_last_error, before any kernel runs and with the batch, its kept reference state and its earlier results as they were -
 * when
 *   - the references the pairs [0, n_pairs) name (the highest bound index + 1) plus n_pairs exceed CE_LAUNCH_MAX_SLOTS image
 *     slots.  The count is the same whether or not the launch would find its references' state kept, so a launch is refused
 *     or runs whatever ran before it;
 *   - CE_METRIC_BUTTERAUGLI runs (an image of 8 x 8 or more) and height > CE_BUTTERAUGLI_MAX_HEIGHT;
 *   - CE_METRIC_SSIMULACRA2 runs and height > CE_SSIMULACRA2_MAX_HEIGHT.
 * A caller with more pairs launches them in parts (ce_batch_bind_pair and the test slab cost nothing to rearrange);
 * ce_eval_batch plans its own chunks under the same limit and takes any n.  No grid limits the width (a grid's x holds
 * 2^31 - 1 blocks); what SSIMULACRA2's work lists add (65535 blocks of 32 rows or 64 columns a launch) lies past 2 000 000 pixels a side
 * and is refused with CE_ERR_INVALID_ARG from inside the metric. */
#define CE_LAUNCH_GRID_MAX 65535u
#define CE_LAUNCH_MAX_SLOTS 65535u
#define CE_BUTTERAUGLI_MAX_HEIGHT 262140u
#define CE_SSIMULACRA2_MAX_HEIGHT 524280u
int ce_batch_launch(ce_batch *b, uint32_t n_pairs, uint32_t metric_mask, uint32_t flags,
                    float intensity_target);
int ce_batch_collect(ce_batch *b, uint32_t n_pairs, ce_scores *out);
/* libjxl's p-norm of the Butteraugli diffmap (mean of the 3-, 6- and 12-norms) for the pairs of the last run
 * that asked for CE_METRIC_BUTTERAUGLI.  The reference only ever reads `.score` (the max-norm,
 * src/metrics/butteraugli.rs:80); BASELINE.json's configs[2] also names the 3-norm. */
int ce_batch_butteraugli_pnorm3(ce_batch *b, uint32_t n_pairs, double *out);
/* ButteraugliResult.diffmap (src/metrics/prelude.rs:64-65) of a grid, as crates/codec-compare/src/find_outliers.rs:77-118
 * would look for where a pair is bad: maps of pairs [first, first+count) of the last launch that had
 * CE_FLAG_BUTTERAUGLI_DIFFMAP and Butteraugli; block = 1 (full map) or a power of two <= 64 (B x B cell maxima, edge cells
 * clipped to the image); out_floats must be count*ceil(w/B)*ceil(h/B); out is [count][ceil(h/B)][ceil(w/B)].  Waits for
 * that launch.  CE_ERR_INVALID_ARG for a null pointer, no stored maps, count = 0 or a range past the stored pairs, a bad
 * block or a wrong out_floats. */
int ce_batch_butteraugli_diffmap(ce_batch *b, uint32_t first, uint32_t count, uint32_t block, float *out, size_t out_floats);
/* DSSIM's SsimMap (see ce_dssim_levels) of pairs [first, first+count) at `level`, from the last launch of this batch that
 * ran CE_METRIC_DSSIM (every such launch keeps its maps on the device, no flag needed).  maps = [count][ceil(h_l/B)]
 * [ceil(w_l/B)] floats: block B = 1 is the full map, B = a power of two <= 64 the MINIMUM of each B x B cell (the worst
 * local similarity; edge cells clipped to the level); ssim = [count] doubles (SsimMap.ssim).  Either output may be NULL
 * (maps_floats then 0), not both.  Waits for that launch.  CE_ERR_INVALID_ARG for a null handle, no stored maps,
 * level >= the level count, count = 0 or a range past the stored pairs, a bad block or a wrong maps_floats. */
int ce_batch_dssim_ssim_maps(ce_batch *b, uint32_t level, uint32_t first, uint32_t count, uint32_t block,
                             float *maps, size_t maps_floats, double *ssim);
/* SSIMULACRA2's error maps (ce_ssim2_map) of pairs [first, first+count) of the last launch: map `kind` of XYB channel
 * `channel` at `scale` (see ce_ssimulacra2_scales).  maps = [count][ceil(h_s/B)][ceil(w_s/B)] floats: block B = 1 is the
 * full map, B = a power of two <= 64 the MAXIMUM of each B x B cell (the worst local error; edge cells clipped to the
 * scale); needs a last launch with CE_FLAG_SSIMULACRA2_MAPS.  norms = [count][2] doubles: that map's mean and 4-norm
 * exactly as the score pooled them; needs only a last launch with CE_METRIC_SSIMULACRA2.  Either output may be NULL
 * (maps_floats then 0), not both.  Waits for that launch.  CE_ERR_INVALID_ARG for a null handle, no stored maps or norms,
 * scale >= the scales that ran, channel or kind >= 3, count = 0 or a range past the stored pairs, a bad block or a
 * wrong maps_floats. */
int ce_batch_ssimulacra2_maps(ce_batch *b, uint32_t scale, uint32_t channel, uint32_t kind, uint32_t first,
                              uint32_t count, uint32_t block, float *maps, size_t maps_floats, double *norms);

/* ---- deep batches: 10-, 12- and 16-bit images at their own precision --------------------------
 * CE_PIXEL_RGB16_10BIT above restates to_8bit (crates/codec-iter/src/avif_config.rs:122-170): every 10-bit sample of a
 * decode is rounded to 8 bits before anything is measured.  A deep batch keeps the samples: its slabs are packed
 * interleaved RGB in uint16_t (little endian) with a declared depth d in {8, 10, 12, 16} per side; sample v (larger values
 * are clamped to 2^d - 1 on ingest, as to_8bit's .min does) means the sRGB-encoded value v / (2^d - 1), and each metric
 * turns it into linear light by its own 8-bit rule with 255 replaced by 2^d - 1 (SSIMULACRA2 and Butteraugli: the curve in
 * f64 rounded once to f32; DSSIM: f32 with powf, src/metrics/dssim.rs:78-85; PSNR: the exact integer sum of squared sample
 * differences, then calculate_psnr's expression, src/metrics/mod.rs:324-330, with 255 replaced by 2^d - 1).  The two sides
 * have their own depths - an 8-bit source against a 10-bit decode, neither rescaled; PSNR needs equal depths and with
 * unequal ones its bit stays clear in `valid` while the other metrics run.  A deep batch of depths 8 / 8 scores an image
 * bit for bit as an RGB8 batch does, and so does one of depth 16 holding v8 * 257.
 * Not part of this: deep ce_ref handles, deep ce_eval_batch (linear-f32 input, PQ and wide-gamut primaries: linear batches,
 * below; HLG: ce_batch_set_*_hlg on linear batches, further below).
 * Pixel formats of a deep batch only (their depth is that side's): packed u16 RGB / RGBA (alpha dropped). */
enum {
    CE_PIXEL_RGB16 = 4,
    CE_PIXEL_RGBA16 = 5
};
/* bytes per pixel of a CE_PIXEL_* format, 0 for an unknown one (pure host function) */
size_t ce_pixel_bytes(int format);
/* ce_batch_create with a depth per side; CE_ERR_INVALID_ARG for a depth outside {8, 10, 12, 16}.  On such a batch
 *   ce_batch_set_reference_fmt / ce_batch_set_test_fmt take CE_PIXEL_RGB16 and CE_PIXEL_RGBA16, and CE_PIXEL_RGB8 /
 *     CE_PIXEL_RGBA8 where that side's depth is 8 (the *_10BIT formats: CE_ERR_INVALID_ARG); ce_batch_set_reference /
 *     ce_batch_set_test are the CE_PIXEL_RGB8 form;
 *   ce_batch_reference_slab / ce_batch_test_slab are the u16 slabs ([max_refs][h][w][3], [max_pairs][h][w][3]; values
 *     written in place must not exceed 2^d - 1);
 *   ce_batch_bind_pair, ce_batch_run, ce_batch_launch, ce_batch_collect, ce_batch_butteraugli_pnorm3 and the three map
 *     readers work as on any batch;
 *   CE_ERR_INVALID_ARG, with the reason in ce_last_error: CE_FLAG_XYB_ROUNDTRIP (by definition an 8-bit quantisation,
 *     src/metrics/xyb.rs:185-199), ce_batch_image_heuristics (defined on u8 gray levels), ce_batch_set_*_lut with a table
 *     (the table is 2^24 8-bit colours).
 * (No reference item: the reference scores PixelData::Rgb16 only after to_8bit.) */
int ce_batch_create_deep(ce_ctx *ctx, uint32_t width, uint32_t height, uint32_t max_refs, uint32_t max_pairs,
                         uint32_t ref_depth, uint32_t test_depth, ce_batch **out);
/* ce_estimate_batch_bytes for a deep batch (0 for a depth outside {8, 10, 12, 16}) */
size_t ce_estimate_batch_bytes_deep(uint32_t width, uint32_t height, uint32_t n_refs, uint32_t n_pairs, uint32_t metric_mask,
                                    uint32_t ref_depth, uint32_t test_depth);
/* ce_eval_pair over packed u16 RGB of the given depths (lengths in bytes: width * height * 6; samples above 2^d - 1 are
 * clamped); the same error kinds in the same order, CE_ERR_INVALID_ARG for a bad depth, CE_FLAG_XYB_ROUNDTRIP or a map flag */
int ce_eval_pair_deep(ce_ctx *ctx, const uint16_t *reference, size_t reference_len, uint32_t ref_depth, const uint16_t *test,
                      size_t test_len, uint32_t test_depth, uint32_t width, uint32_t height, uint32_t metric_mask,
                      uint32_t flags, float intensity_target, ce_scores *out);

/* ---- reference handle: Ssimulacra2Reference::{new,compare} ------------------------
 * crates/codec-iter/src/eval.rs:138-149,83-89; crates/codec-compare/src/brute_force_sweep.rs:197-201,256
 * The handle keeps the reference resident in HBM together with its reference-side state for EVERY metric: the XYB
 * roundtrip (CE_FLAG_XYB_ROUNDTRIP), the SSIMULACRA2 XYB pyramid, DSSIM's img / mu / blur(img^2) pyramid
 * (Dssim::create_image of the reference) and Butteraugli's PsychoImage at both resolutions are built by the first
 * compare that needs them and reused by every later one (Butteraugli's also depends on intensity_target: a compare
 * with another target rebuilds it).  The row-blurred SSIMULACRA2 reference planes are NOT kept: the blur passes are
 * bound by HBM traffic and a compare would read a cached plane just as it reads a recomputed one. */
int ce_ref_create(ce_ctx *ctx, const uint8_t *reference, size_t reference_len, uint32_t width, uint32_t height,
                  uint32_t flags, ce_ref **out);
int ce_ref_compare(ce_ref *ref, const uint8_t *test, size_t test_len, uint32_t metric_mask,
                   float intensity_target, ce_scores *out);
/* The quality sweep of one reference in one launch: the loop
 *   for q in qualities { reference.compare(decoded[q]) }      (eval.rs:83-89, brute_force_sweep.rs:256)
 * as a single batch.  tests[i] / test_lens[i]: the i-th distorted image; out[i].status is per item
 * (CE_ERR_DIM_MISMATCH for a wrong length, the others still run); the return value reports call-level
 * failures only. */
int ce_ref_compare_many(ce_ref *ref, const uint8_t *const *tests, const size_t *test_lens, uint32_t n_tests,
                        uint32_t metric_mask, float intensity_target, ce_scores *out);
/* builds[k] = number of compares so far that had to (re)build the reference-side state of SSIMULACRA2 (k = 0),
 * DSSIM (1), Butteraugli (2): 1 each after any number of compares of one handle with one intensity target */
int ce_ref_stats(const ce_ref *ref, uint32_t builds[3]);
/* the same for a reference handle created with CE_FLAG_BUTTERAUGLI_DIFFMAP: the tests of its last compare / compare_many
 * (src/metrics/prelude.rs:64-65 per compare of eval.rs:83-89) */
int ce_ref_butteraugli_diffmap(ce_ref *ref, uint32_t first, uint32_t count, uint32_t block, float *out, size_t out_floats);
/* the same as ce_batch_dssim_ssim_maps for the tests of a reference handle's last compare / compare_many that ran DSSIM */
int ce_ref_dssim_ssim_maps(ce_ref *ref, uint32_t level, uint32_t first, uint32_t count, uint32_t block,
                           float *maps, size_t maps_floats, double *ssim);
/* the same as ce_batch_ssimulacra2_maps for the tests of a reference handle's last compare / compare_many (maps: a handle
 * created with CE_FLAG_SSIMULACRA2_MAPS; crates/codec-iter/src/eval.rs:83-89) */
int ce_ref_ssimulacra2_maps(ce_ref *ref, uint32_t scale, uint32_t channel, uint32_t kind, uint32_t first, uint32_t count,
                            uint32_t block, float *maps, size_t maps_floats, double *norms);
void ce_ref_destroy(ce_ref *ref);

/* ---- image heuristics: ImageHeuristics of crates/codec-compare/src/image_heuristics.rs:22-63 ----------------------
 * compute_heuristics (image_heuristics.rs:76-305), whose CSV (:358-400) build-predictor reads to pick an encoder
 * (crates/codec-compare/src/build_predictor.rs:75-100).  Same field names and order; the image name stays with the caller.
 * Every per-pixel and per-block value (gray, gradients, 3x3 contrast, saturation, adjacent differences, each 8x8 block's
 * sequential f32 mean and variance) is the reference's f32 arithmetic, so width .. pixels, edge_strength_max,
 * edge_density, the five *_block_pct, analyze_detail_block_pct, high/low_freq_energy and freq_ratio equal the
 * reference's bit for bit.  The whole-image sums behind the other fields (means, variances, standard deviations, the
 * complexities) take the reference's f32 terms (a variance's (v - mean)^2 with the f32 mean), add them in f64 in an
 * order fixed by the image's shape alone, round once to f32 and divide by the reference's f32 divisor: deterministic,
 * but not the reference's sequential f32 accumulation (DESIGN.md section 2 gives the measured gap).  Images under 8 x 8
 * have no blocks: their block fields are 0 (num_blocks.max(1), image_heuristics.rs:136).  Images under 3 x 3 return
 * CE_ERR_TOO_SMALL (the reference underflows width - 2 there). */
typedef struct ce_image_heuristics {
    uint64_t width;
    uint64_t height;
    uint64_t pixels;
    float mean_luminance;
    float luminance_variance;
    float luminance_std;
    float edge_strength_mean;
    float edge_strength_max;
    float edge_density;
    float flat_block_pct;
    float low_var_block_pct;
    float mid_var_block_pct;
    float high_var_block_pct;
    float detail_block_pct;
    float block_variance_mean;
    float block_variance_std;
    float color_variance;
    float saturation_mean;
    float saturation_std;
    float high_freq_energy;
    float low_freq_energy;
    float freq_ratio;
    float local_contrast_mean;
    float local_contrast_std;
    float horizontal_complexity;
    float vertical_complexity;
    float diagonal_complexity;
    /* analyze-image's detail_block_pct (crates/codec-compare/src/analyze_image.rs:94-96): blocks with variance > 1000,
     * over num_blocks.max(1) like the fields above (0, not analyze-image's NaN, without blocks) */
    float analyze_detail_block_pct;
} ce_image_heuristics;

/* which slab ce_batch_image_heuristics reads */
enum ce_batch_images { CE_BATCH_REFERENCES = 0, CE_BATCH_TESTS = 1 };

/* compute_heuristics (image_heuristics.rs:76) of one packed RGB8 image.  CE_ERR_BAD_LENGTH unless len = w * h * 3,
 * then CE_ERR_TOO_SMALL for a width or height under 3. */
int ce_image_heuristics_rgb8(ce_ctx *ctx, const uint8_t *rgb, size_t len, size_t width, size_t height, ce_image_heuristics *out);
/* compute_heuristics of images [first, first + count) already resident in a batch's references (which =
 * CE_BATCH_REFERENCES) or tests (CE_BATCH_TESTS) slab - the source images of a corpus sweep, with no second upload
 * (full_comparison.rs uploads every source image; image_heuristics.rs:334-345 decodes it again).  Sees every image
 * written by ce_batch_set_* / bind_pair before the call; launches nothing of the metrics and leaves the last launch's
 * scores and maps as they were.  out has count entries.  CE_ERR_INVALID_ARG for an unknown slab, count = 0 or a range
 * past the slab, CE_ERR_TOO_SMALL for a batch under 3 x 3. */
int ce_batch_image_heuristics(ce_batch *b, uint32_t which, uint32_t first, uint32_t count, ce_image_heuristics *out);
/* the same for the image of a reference handle (Ssimulacra2Reference::new, crates/codec-iter/src/eval.rs:138-149) */
int ce_ref_image_heuristics(ce_ref *ref, ce_image_heuristics *out);

/* ---- viewing simulation: the resampling ViewingCondition::simulation_params asks for (src/viewing.rs:244-301) -----------
 * SimulationParams (src/viewing.rs:308-331) says at which size an image has to be looked at under a ViewingCondition
 * ("simulate browser behavior exactly", src/viewing.rs:18-19, 33-53); the reference has no resampler and its metrics ignore
 * the condition (src/metrics/dssim.rs:43).  These calls change an image's size on the device.  The resampler is the
 * separable fixed-point convolution Pillow's Image.resize runs on 8-bit images, on the sRGB-encoded bytes as a browser
 * does, bit for bit: per axis with scale = in / out, fs = max(scale, 1) and support = S * fs, output
 * sample xx has center = (xx + 0.5) * scale, taps [xmin, xmax) = [max(0, (int)(center - support + 0.5)),
 * min(in, (int)(center + support + 0.5))), weights f((x + xmin - center + 0.5) / fs) normalised by their left-to-right f64
 * sum, each turned into (int)(+-0.5 + k * 2^22), and is clip_0_255((2^21 + sum k_i * sample_i) >> 22) in int32.  The
 * horizontal pass runs first and writes u8, the vertical pass runs on that; a pass whose size does not change is skipped
 * (equal sizes: a byte copy).  The weights are built on the host in f64.
 * A LINEAR batch (below) is resampled in linear light, where averaging light is physically right, by
 * the same convolution as Pillow runs it on mode "F" images, bit for bit: the same taps [xmin, xmax), ss = 1.0 / fs, weights
 * w_x = f((x + xmin - center + 0.5) * ss) divided by their left-to-right f64 sum when that is not zero and kept as doubles;
 * acc = 0.0, then acc = acc + (double)sample[xmin + x] * w_x for x ascending, the product and the sum each rounded to f64 (no
 * fused multiply-add); out = (float)acc.  Horizontal pass first, f32 between the passes, a pass whose size does not change
 * skipped, equal sizes a byte copy, the three channels independent.  The last pass that runs clamps what it stores to
 * [-CE_LINEAR_MAX, CE_LINEAR_MAX], the invariant of a linear slab (a filter with negative lobes overshoots); the byte copy
 * does not clamp.  tests/resample_linear_restatement.py restates this in numpy.
 *   BOX       f = 1 on (-0.5, 0.5], S = 0.5      BILINEAR  f = 1 - |x| on (-1, 1), S = 1
 *   BICUBIC   Keys' cubic with a = -0.5, S = 2    LANCZOS3  sinc(x) sinc(x / 3) on [-3, 3), S = 3 */
enum ce_resample_filter {
    CE_RESAMPLE_BOX = 0,
    CE_RESAMPLE_BILINEAR = 1,
    CE_RESAMPLE_BICUBIC = 2,
    CE_RESAMPLE_LANCZOS3 = 3
};
/* One packed RGB8 image of w x h to out_w x out_h (the image SimulationParams::target_width / target_height describe,
 * src/viewing.rs:312-316).  CE_ERR_INVALID_ARG for a null pointer, an unknown filter or a zero size; CE_ERR_BAD_LENGTH
 * unless len = w * h * 3 and out_len = out_w * out_h * 3. */
int ce_resample_rgb8(ce_ctx *ctx, const uint8_t *rgb, size_t len, uint32_t w, uint32_t h, uint32_t out_w, uint32_t out_h,
                     int filter, uint8_t *out, size_t out_len);
/* One packed float RGB image in linear light to another size, by the float resampler above.  Errors as ce_resample_rgb8, in
 * the same order, with the lengths in bytes: len = w * h * 12, out_len = out_w * out_h * 12.  The input is taken as it is
 * (a NaN spreads to the outputs whose taps cover it); the output is clamped as stated above. */
int ce_resample_linear(ce_ctx *ctx, const float *rgb, size_t len, uint32_t w, uint32_t h, uint32_t out_w, uint32_t out_h, int filter,
                       float *out, size_t out_len);
/* Images [first, first + count) of src's reference or test slab (which: enum ce_batch_images) resampled into the same
 * indices of dst, a batch of another (or the same) shape on the same context - the images of a resident sweep at the
 * size a condition displays them (src/viewing.rs:244-301), with no upload and no host pixel pass.  Runs behind every
 * ce_batch_set_* of src so far and before any later launch on dst; touches no metric buffer and no stored scores or maps
 * of either batch; returns without waiting.  CE_ERR_INVALID_ARG, with the reason in ce_last_error, for a null handle,
 * batches of different contexts, src = dst, an unknown slab or filter, count = 0, a range past either batch's slots, a
 * deep batch on either side (resampling u16 samples is not part of this: nothing outside the project defines its result,
 * DESIGN.md section 17), or a linear batch paired with one that is not.  RGB8 -> RGB8 runs the fixed-point resampler,
 * linear -> linear the float one; stream ordering and bindings are the same for both. */
int ce_batch_resample(ce_batch *src, ce_batch *dst, uint32_t which, uint32_t first, uint32_t count, int filter);
/* Both slabs - references [0, n_refs) and tests [0, n_pairs) - and src's pair -> reference bindings of those pairs, so
 * that ce_batch_run(dst, n_pairs, ...) follows directly (src/viewing.rs:244-301 applied to a whole grid).  Errors as
 * ce_batch_resample. */
int ce_batch_resample_pairs(ce_batch *src, ce_batch *dst, uint32_t n_refs, uint32_t n_pairs, int filter);

/* ---- planar Y'CbCr ingest: a decoder's planes straight into a slot of a resident batch ----------
 * A decoder works in Y'CbCr planes, usually 4:2:0 (a JPEG decoder in raw mode, dav1d / libavif, rocJPEG and rocDecode,
 * whose surfaces are already in device memory); crates/codec-iter/src/avif_config.rs:163-169 bails on every PixelData
 * variant that is not RGB.  These calls run the chroma upsampling and the colour matrix on the device, in integers, and
 * write packed RGB into the slot: u8 on an RGB8 batch (output depth D = 8), u16 of that side's depth D on a deep batch.
 *   samples   depth d in {8, 10, 12}: u8 at 8 bits, u16 little endian above, low-aligned (values above 2^d - 1 are
 *             clamped to it, as deep ingest does) or MSB-aligned (P010: v >> (16 - d)).  m = 2^D - 1, u = 2^(d - 8).
 *   chroma    planes are ceil(w / 2) wide for 4:2:0 and 4:2:2 and ceil(h / 2) tall for 4:2:0; they are upsampled to
 *             2 cw x 2 ch (4:2:0) or 2 cw x h (4:2:2) and cropped to w x h.
 *             CE_CHROMA_NEAREST   replication
 *             CE_CHROMA_TRIANGLE  libjpeg's "fancy" upsampling, centre-sited, in integers (>> is a floor):
 *               h2v2, chroma row r:  even output row  t[i] = 3 c[r][i] + c[max(r - 1, 0)][i]
 *                                    odd output row   t[i] = 3 c[r][i] + c[min(r + 1, ch - 1)][i]
 *                                    out[2i] = (3 t[i] + t[max(i - 1, 0)] + 8) >> 4
 *                                    out[2i + 1] = (3 t[i] + t[min(i + 1, cw - 1)] + 7) >> 4
 *               h2v1:                out[2i] = (3 c[i] + c[max(i - 1, 0)] + 1) >> 2
 *                                    out[2i + 1] = (3 c[i] + c[min(i + 1, cw - 1)] + 2) >> 2
 *   matrix    a (Cr -> R), b (Cb -> G), c (Cr -> G), e (Cb -> B).  BT601: the literals 1.40200, 0.34414, 0.71414, 1.77200
 *             (libjpeg's jdcolor.c).  BT709 (Kr = 0.2126, Kb = 0.0722) and BT2020 (Kr = 0.2627, Kb = 0.0593): in f64,
 *             a = 2 (1 - Kr), e = 2 (1 - Kb), b = Kb e / Kg, c = Kr a / Kg with Kg = 1 - Kr - Kb.
 *   range     FULL: y0 = 0, c0 = 2^(d - 1), sy = sc = m / (2^d - 1).  LIMITED: y0 = 16 u, c0 = 128 u, sy = m / (219 u),
 *             sc = m / (224 u).
 *   fixed point, built on the host in f64, int64 on the device:
 *             KY = rint(sy 2^16), KRV = rint(sc a 2^16), KGU = rint(sc b 2^16), KGV = rint(sc c 2^16), KBU = rint(sc e 2^16)
 *             R = clamp((KY (y - y0) + KRV (cr - c0) + 2^15) >> 16, 0, m)
 *             G = clamp((KY (y - y0) - KGU (cb - c0) - KGV (cr - c0) + 2^15) >> 16, 0, m)
 *             B = clamp((KY (y - y0) + KBU (cb - c0) + 2^15) >> 16, 0, m)
 *             BT601 / FULL / d = D = 8 gives 65536, 91881, 22554, 46802, 116130: libjpeg-turbo's decoder, bit for bit.
 *             4:0:0 (gray): R = G = B from the Y term alone.
 * Not part of this: left-cosited (MPEG-2 / H.264 default) and other chroma sitings, 4:1:1 / 4:4:0, packed YUYV, 16-bit
 * YUV (PQ: ce_batch_set_*_yuv_cicp below; HLG: ce_batch_set_*_yuv_hlg), identity / YCgCo matrices, YUV through ce_eval_batch, ce_ref_* and ce_batch_resample*, alpha planes. */
enum ce_yuv_subsampling { CE_YUV_444 = 0, CE_YUV_422 = 1, CE_YUV_420 = 2, CE_YUV_400 = 3 };
/* PLANAR: plane[0..2] = Y, Cb, Cr (I420 and its kin).  SEMIPLANAR: plane[0] = Y, plane[1] = interleaved Cb Cr pairs
 * (NV12 / NV16 / P010), plane[2] unused.  4:0:0 reads plane[0] only under either layout. */
enum ce_yuv_layout { CE_YUV_PLANAR = 0, CE_YUV_SEMIPLANAR = 1 };
enum ce_yuv_matrix { CE_YUV_BT601 = 0, CE_YUV_BT709 = 1, CE_YUV_BT2020 = 2 };
enum ce_yuv_range { CE_YUV_FULL = 0, CE_YUV_LIMITED = 1 };
enum ce_chroma_upsample { CE_CHROMA_NEAREST = 0, CE_CHROMA_TRIANGLE = 1 };
enum ce_mem { CE_MEM_HOST = 0, CE_MEM_DEVICE = 1 };
typedef struct ce_yuv_image {
    const void *plane[3];
    size_t pitch[3];      /* bytes from one row to the next; may exceed the row */
    int subsampling;      /* enum ce_yuv_subsampling */
    int layout;           /* enum ce_yuv_layout */
    int matrix;           /* enum ce_yuv_matrix */
    int range;            /* enum ce_yuv_range */
    int upsample;         /* enum ce_chroma_upsample */
    int depth;            /* 8, 10 or 12 */
    int msb_aligned;      /* u16 samples hold their value in the top bits (P010); depth 8: must be 0 */
    int memory;           /* enum ce_mem: where the planes are */
    const ce_lut *lut;    /* reserved, must be NULL: a colour table is 2^24 RGB colours and is not offered for YUV; a
                           * non-NULL value is refused with CE_ERR_INVALID_ARG rather than ignored */
} ce_yuv_image;
/* {KY, KRV, KGU, KGV, KBU, y0, c0} as defined above.  A pure host function (no context, works without a device);
 * CE_ERR_INVALID_ARG for an unknown matrix or range, depth_in outside {8, 10, 12}, depth_out outside {8, 10, 12, 16} or
 * a null pointer. */
int ce_yuv_coefficients(int matrix, int range, uint32_t depth_in, uint32_t depth_out, int64_t out[7]);
/* One image of the batch's shape into a reference / test slot, on an RGB8 or a deep batch, on the same stream and with
 * the same ordering as ce_batch_set_*_fmt.  CE_MEM_HOST planes are copied row by row (not the pitch padding) through the
 * batch's page-locked staging and are consumed on return.  CE_MEM_DEVICE planes are read in place by the kernel, on the
 * context's device: the caller must have finished writing them before the call and must keep them until the batch's next
 * launch has been collected; the call returns without waiting.  CE_ERR_INVALID_ARG, with the reason in ce_last_error and
 * the batch still usable, for a null struct, a missing plane of the layout, an unknown enum, a depth outside {8, 10, 12},
 * a pitch under the row's bytes, a u16 plane pointer or pitch that is not 2-byte aligned, msb_aligned with depth 8, or a
 * colour table. */
int ce_batch_set_reference_yuv(ce_batch *b, uint32_t ref_index, const ce_yuv_image *image);
int ce_batch_set_test_yuv(ce_batch *b, uint32_t pair_index, uint32_t ref_index, const ce_yuv_image *image);
/* One image of width x height to packed RGB8 (out_len = width * height * 3 bytes) or to packed u16 RGB of depth_out in
 * {8, 10, 12, 16} (out_len = width * height * 3 samples) in host memory.  Errors as above; CE_ERR_BAD_LENGTH for a
 * wrong out_len. */
int ce_yuv_to_rgb8(ce_ctx *ctx, const ce_yuv_image *image, uint32_t width, uint32_t height, uint8_t *out, size_t out_len);
int ce_yuv_to_rgb16(ce_ctx *ctx, const ce_yuv_image *image, uint32_t width, uint32_t height, uint32_t depth_out, uint16_t *out,
                    size_t out_len);

/* ---- alpha: a transparent image composited over solid backgrounds on the device -----------------
 * CE_PIXEL_RGBA8 / CE_PIXEL_RGBA16 above drop alpha (ImageData::to_rgb8_vec, src/eval/session.rs:98-117), so the colour an
 * encoder left under alpha = 0 is scored although nobody sees it, and damage to the alpha plane is not scored although it
 * shows over every background but one.  These calls composite instead: source-over of STRAIGHT (non-premultiplied) alpha
 * onto an opaque solid colour, on the ENCODED sample values (what a browser's compositor does with an sRGB page), in
 * unsigned 32-bit integers.  With m = 2^d - 1 (255 for 8-bit samples), per channel,
 *     out = (c * a + bg * (m - a) + (m >> 1)) / m        (integer division; c and a clamped to m first)
 * c * a + bg * (m - a) <= m * m, so with the rounding term the sum stays below 2^32 at every depth; the division is exact.
 * For m = 255 this is Pillow's Image.alpha_composite over an opaque background on all 2^24 (c, a, bg) triples.  a = m
 * gives c, a = 0 gives bg, and the result is monotone in c.
 * One upload of the image fills n_bg consecutive slots, slot k over backgrounds[k] (1 <= n_bg <= CE_MAX_BACKGROUNDS): the
 * pixel is read once on the device.  format: CE_PIXEL_RGBA8 on an RGB8 batch or on a side of depth 8 of a deep batch,
 * CE_PIXEL_RGBA16 on a deep batch (samples of that side's depth d).  backgrounds: [n_bg][3] samples at the destination
 * side's depth (an RGB8 batch: <= 255).
 * Not part of this: premultiplied alpha, linear-light blending (the convention of libjxl's command-line tools), patterned
 * (checkerboard) backgrounds, dssim-core's own alpha handling, CE_PIXEL_RGBA16_10BIT (refused; a deep batch is the route
 * for 10-bit alpha), device-resident sources, ce_ref_* handles, ce_eval_batch, ce_eval_batch_lut and ce_batch_resample*. */
#define CE_MAX_BACKGROUNDS 8
/* Reference slots first_ref .. first_ref + n_bg - 1 / test slots first_pair .. first_pair + n_bg - 1, pair first_pair + k
 * bound to reference ref_indices[k]; on the same stream and with the same ordering as ce_batch_set_*_fmt, the pixels
 * consumed on return.  CE_ERR_INVALID_ARG, with the reason in ce_last_error and the batch still usable, for a null handle
 * or pointer, a format without alpha or a *_10BIT format, CE_PIXEL_RGBA16 on an RGB8 batch, CE_PIXEL_RGBA8 on a deep side
 * whose depth is not 8, a wrong len, n_bg = 0 or n_bg > CE_MAX_BACKGROUNDS, a background sample above m, a slot range or a
 * ref_indices entry past the batch. */
int ce_batch_set_reference_over(ce_batch *b, uint32_t first_ref, const void *pixels, size_t len, int format, uint32_t n_bg,
                                const uint16_t *backgrounds);
int ce_batch_set_test_over(ce_batch *b, uint32_t first_pair, const uint32_t *ref_indices, const void *pixels, size_t len,
                           int format, uint32_t n_bg, const uint16_t *backgrounds);
/* One image over one colour to host memory: w x h RGBA8 (len = w * h * 4 bytes) -> packed RGB8 (out_len = w * h * 3
 * bytes); w x h u16 RGBA of `depth` bits in {8, 10, 12, 16} (len = w * h * 4 samples) -> packed u16 RGB (out_len =
 * w * h * 3 samples).  CE_ERR_INVALID_ARG for a null handle or pointer, a wrong len or out_len, a background sample above
 * m, or a depth outside {8, 10, 12, 16}. */
int ce_composite_rgba8(ce_ctx *ctx, const uint8_t *rgba, size_t len, uint32_t w, uint32_t h, const uint8_t bg[3], uint8_t *out,
                       size_t out_len);
int ce_composite_rgba16(ce_ctx *ctx, const uint16_t *rgba, size_t len, uint32_t w, uint32_t h, uint32_t depth, const uint16_t bg[3],
                        uint16_t *out, size_t out_len);

/* ---- linear batches and CICP ingest: HDR and wide-gamut images -----------------------------------
 * Every batch above reads its samples as sRGB-encoded values with BT.709 primaries.  A LINEAR batch holds linear light
 * instead: its slabs are packed interleaved RGB float, linear light with BT.709 / sRGB primaries and D65 white, 1.0 the
 * white an 8-bit 255 maps to; values below 0 (colours outside the sRGB gamut) and above 1 (highlights) are legal and are
 * scored.  On ingest NaN becomes 0 and every sample is clamped to [-CE_LINEAR_MAX, CE_LINEAR_MAX] (PQ's 10 000 nits at an
 * 80-nit white is 125).  Slot k of a slab starts at byte k * width * height * 12 (ce_batch_reference_slab /
 * ce_batch_test_slab; one copy of the image per slot, read by every metric).
 * SSIMULACRA2, DSSIM and Butteraugli take the sample as their level-0 linear value, with no table; everything behind that
 * - the diffmap, DSSIM's SSIM maps, CE_FLAG_SSIMULACRA2_MAPS included - is the code every batch runs, so a linear batch
 * loaded with ce_srgb_table(8, 0)[v] scores SSIMULACRA2 and Butteraugli bit for bit as the RGB8 batch of the bytes v does,
 * and one loaded with ce_srgb_table(8, 1)[v] DSSIM.  PSNR has no integer grid here: its bit stays clear in `valid` and the
 * other metrics run.  Butteraugli's intensity_target keeps its meaning: nits at 1.0.  It is not range-checked; the range
 * over which a linear batch is held to the oracle - every per-pixel map bit for bit, on samples from the smallest subnormal
 * to +-CE_LINEAR_MAX - is 80 .. 10 000 ("Operand ranges"; tests/test_gpu_wide_content.py).  The
 * oracle itself stays finite on such samples up to about 1e9 and not at 1e12.
 * On a linear batch
 *   ce_batch_set_reference_fmt / ce_batch_set_test_fmt take CE_PIXEL_RGB_F32 only (len = width * height * 12);
 *   ce_batch_set_reference_cicp / ce_batch_set_test_cicp take tagged integer code values (below);
 *   ce_batch_set_reference_yuv_cicp / ce_batch_set_test_yuv_cicp take Y'CbCr planes with such a tag (below);
 *   ce_batch_set_reference_hlg / ce_batch_set_test_hlg and their *_yuv_hlg forms take BT.2100 HLG (below);
 *   ce_batch_set_reference_gainmap / ce_batch_set_test_gainmap take an SDR base image with a gain map (below);
 *   ce_batch_set_*_cicp_over / _hlg_over / _icc_over / _linear_over take an image with alpha and blend it over solid
 *     backgrounds in linear light (the section "alpha in linear light" at the end of this header);
 *   ce_batch_bind_pair, ce_batch_run, ce_batch_launch, ce_batch_collect, ce_batch_butteraugli_pnorm3 and the three map
 *     readers work as on any batch;
 *   CE_ERR_INVALID_ARG, with the reason in ce_last_error and the batch still usable: CE_FLAG_XYB_ROUNDTRIP,
 *     ce_batch_image_heuristics, ce_batch_set_*_lut with a table, ce_batch_set_reference / ce_batch_set_test and every
 *     8- / 16-bit format (the *_10BIT ones included) through *_fmt, ce_batch_resample* between it and a batch that is not linear, *_over, *_yuv.
 *   ce_batch_resample / ce_batch_resample_pairs from a linear batch into a linear batch run the float resampler of the
 *     viewing-simulation section above.
 *   CE_PIXEL_RGB_F32 on a batch that is not linear is refused the same way.
 * Not part of this: the BT.709 / BT.1886 gamma transfers (HLG, whose OOTF couples the channels, has calls of its own below),
 * primaries with a non-D65 white, limited-range RGB, ce_ref_* handles on linear batches and the pooled ce_eval_batch on
 * them.
 * (No reference item: the reference scores every PixelData variant only after to_8bit / to_rgb8_vec.) */
enum {
    CE_PIXEL_RGB_F32 = 7 /* packed float RGB, 12 bytes per pixel: linear batches only (6 is not a format) */
};
#define CE_LINEAR_MAX 1024.0f
int ce_batch_create_linear(ce_ctx *ctx, uint32_t width, uint32_t height, uint32_t max_refs, uint32_t max_pairs, ce_batch **out);
/* ce_estimate_batch_bytes for a linear batch */
size_t ce_estimate_batch_bytes_linear(uint32_t width, uint32_t height, uint32_t n_refs, uint32_t n_pairs, uint32_t metric_mask);
/* ce_eval_pair over packed float RGB (lengths in bytes: width * height * 12); the same error kinds in the same order,
 * CE_ERR_INVALID_ARG for CE_FLAG_XYB_ROUNDTRIP or a map flag */
int ce_eval_pair_linear(ce_ctx *ctx, const float *reference, size_t reference_len, const float *test, size_t test_len, uint32_t width,
                        uint32_t height, uint32_t metric_mask, uint32_t flags, float intensity_target, ce_scores *out);
/* The library's own sRGB -> linear table of `depth` bits (8, 10, 12 or 16; n = 2^depth entries): rule 0 the f64 curve
 * rounded once to f32 (SSIMULACRA2, Butteraugli), rule 1 f32 powf (DSSIM, src/metrics/dssim.rs:78-85) - exactly the floats
 * the RGB8 and deep batches read.  A pure host function. */
int ce_srgb_table(uint32_t depth, int rule, float *out, size_t n);

/* CICP ingest: integer RGB code values tagged with ITU-T H.273 code points -> a slot of a linear batch, on the device.
 *   primaries  1 BT.709 (x, y: R 0.640 0.330, G 0.300 0.600, B 0.150 0.060), 9 BT.2020 (R 0.708 0.292, G 0.170 0.797,
 *              B 0.131 0.046), 12 Display P3 (R 0.680 0.320, G 0.265 0.690, B 0.150 0.060); white D65 (0.3127, 0.3290) each
 *   transfer   13 sRGB; 8 linear: v / maxv; 16 PQ (SMPTE ST 2084): nits / white_nits with white_nits > 0 (203 is the usual
 *              suggestion; pass Butteraugli's intensity target to keep absolute nits)
 *   depth      8, 10, 12 or 16; maxv = 2^depth - 1; 8-bit formats require depth 8
 * Definition, per pixel of a CE_PIXEL_RGB8 / RGBA8 / RGB16 / RGBA16 image (alpha dropped, as to_rgb8_vec drops it):
 *   1. t = table[min(v, maxv)] per channel.  The table is built on the host in f64 per code point e = v / maxv and rounded
 *      once to f32; the curve is never evaluated on the device.  sRGB: exactly ce_srgb_table(depth, 0).  PQ, with
 *      m1 = 2610/16384, m2 = 2523/4096 * 128, c1 = 3424/4096, c2 = 2413/4096 * 32, c3 = 2392/4096 * 32:
 *      p = e^(1/m2), nits = 10000 * (max(p - c1, 0) / (c2 - c3 p))^(1/m1), t = nits / white_nits.
 *   2. primaries 1: nothing further, the result is the table value bit for bit.
 *   3. otherwise o_i = (M[i][0] * r + M[i][1] * g) + M[i][2] * b in f32, every product and sum rounded separately (no
 *      fused multiply-add), with M = inv(XYZ <- sRGB) * (XYZ <- src) built on the host in f64 from the chromaticities above
 *      and rounded once to f32 (ce_colour_matrix, row-major).
 *   4. the clamp of a linear image: NaN -> 0, then [-CE_LINEAR_MAX, CE_LINEAR_MAX].
 * tests/cicp_restatement.py restates this in numpy; the device equals it bit for bit. */
typedef struct ce_colour {
    int primaries;     /* H.273 ColourPrimaries: 1, 9 or 12 */
    int transfer;      /* H.273 TransferCharacteristics: 13, 8 or 16 */
    uint32_t depth;    /* 8, 10, 12 or 16; samples above 2^depth - 1 are clamped */
    float white_nits;  /* PQ only: the luminance that becomes 1.0 */
} ce_colour;
/* One image of the batch's shape into a reference / test slot of a LINEAR batch, on the same stream and with the same
 * staging and ordering as ce_batch_set_*_fmt; the pixels are consumed on return.  CE_ERR_INVALID_ARG, with the reason in
 * ce_last_error and the batch still usable, for a batch that is not linear, a null pointer, another format, a depth,
 * primaries or transfer outside the lists above, an 8-bit format with depth != 8, PQ without white_nits > 0;
 * CE_ERR_BAD_LENGTH for a wrong len. */
int ce_batch_set_reference_cicp(ce_batch *b, uint32_t ref_index, const void *pixels, size_t len, int format, const ce_colour *c);
int ce_batch_set_test_cicp(ce_batch *b, uint32_t pair_index, uint32_t ref_index, const void *pixels, size_t len, int format,
                           const ce_colour *c);
/* One image of w x h to packed float RGB in host memory (out_len = w * h * 3 floats).  Errors as above. */
int ce_cicp_to_linear(ce_ctx *ctx, const void *pixels, size_t len, int format, const ce_colour *c, uint32_t w, uint32_t h, float *out,
                      size_t out_len);
/* The ingest's transfer table (n = 2^depth entries; white_nits is read for PQ only) and its primaries matrix (row-major;
 * primaries 1: the identity).  Pure host functions; CE_ERR_INVALID_ARG for a code point outside the lists above. */
int ce_transfer_table(int transfer, uint32_t depth, float white_nits, float *out, size_t n);
int ce_colour_matrix(int primaries, float out[9]);

/* Y'CbCr planes with a CICP description -> a slot of a linear batch, on the device, in one kernel:
 * what an HDR10 frame, an AVIF-HDR still from dav1d / libavif or a rocDecode / rocJPEG surface is.  The definition is the
 * composition of the two above and adds no arithmetic.  For an image img and a colour description c,
 *     rgb = the integer RGB that ce_yuv_to_rgb16(img, depth_out = c.depth) defines (samples, chroma upsampling, fixed-point
 *           matrix, clamp to 2^c.depth - 1)
 *     out = what ce_cicp_to_linear(rgb as CE_PIXEL_RGB16, c) defines (table gather, separately rounded f32 3 x 3 for
 *           primaries != 1, the clamp of a linear image)
 * img.depth (8, 10 or 12) is the depth of the Y'CbCr samples; c.depth (8, 10, 12 or 16) is the depth of the integer RGB
 * grid between the two steps and the size of the transfer table, and must not be under img.depth.  c.depth = 16 keeps what
 * the matrix produces between the samples' code points; c.depth = img.depth is what a decoder's own RGB output would have
 * been.  The composition of tests/yuv_restatement.py (yuv_to_rgb with D = c.depth) and tests/cicp_restatement.py (to_linear)
 * restates it in numpy; the device equals it bit for bit, on every float.
 * ce_batch_set_*_yuv_cicp: one image of the batch's shape into a reference / test slot of a LINEAR batch, with the staging,
 * the stream and the ordering of ce_batch_set_*_yuv; CE_MEM_HOST planes are consumed on return, CE_MEM_DEVICE planes are
 * read in place under the lifetime rule given there.  CE_ERR_INVALID_ARG, with the reason in ce_last_error and the batch
 * still usable, for everything ce_batch_set_*_yuv refuses about the image, everything ce_batch_set_*_cicp refuses about c,
 * c.depth < img.depth, a null pointer, and a batch that is not linear.  (ce_batch_set_*_yuv on a linear batch stays refused:
 * it has no colour description to go by.)
 * ce_yuv_to_linear: one image of width x height to packed float RGB in host memory (out_len = width * height * 3 floats);
 * errors as above, CE_ERR_BAD_LENGTH for a wrong out_len.
 * Not part of this: the BT.709 / BT.1886 transfers (HLG: ce_batch_set_*_yuv_hlg below), identity / YCgCo matrices, chroma sitings other than the centred
 * one, ce_ref_* handles and the pooled ce_eval_batch on linear batches. */
int ce_batch_set_reference_yuv_cicp(ce_batch *b, uint32_t ref_index, const ce_yuv_image *image, const ce_colour *c);
int ce_batch_set_test_yuv_cicp(ce_batch *b, uint32_t pair_index, uint32_t ref_index, const ce_yuv_image *image, const ce_colour *c);
int ce_yuv_to_linear(ce_ctx *ctx, const ce_yuv_image *image, const ce_colour *c, uint32_t width, uint32_t height, float *out, size_t out_len);

/* Y'CbCr planes with an ICC profile -> a slot of any batch, on the device, in one kernel: what a
 * phone's JPEG or HEIC is - planes with a Display P3 profile - and what a rocJPEG surface of one is.  The definition is the
 * composition of ce_yuv_to_rgb16 and the ICC section's (below) and adds no arithmetic.  For an image img, a profile handle
 * icc of either flavour (ce_icc_create: matrix/TRC; ce_icc_lut_create: LUT-based) and an integer grid depth rgb_depth,
 *     rgb = the integer RGB that ce_yuv_to_rgb16(img, depth_out = rgb_depth) defines (samples, chroma upsampling, fixed-point
 *           matrix, clamp to 2^rgb_depth - 1)
 *     a linear slot:  what ce_icc_to_linear(rgb as CE_PIXEL_RGB16, depth = rgb_depth, icc) defines
 *     an RGB8 slot (D = 8, stored as u8) / a deep side of depth D:
 *                     what ce_icc_to_srgb16(rgb as CE_PIXEL_RGB16, depth = rgb_depth, icc, depth_out = D) defines
 * img.depth (8, 10 or 12) is the depth of the Y'CbCr samples; rgb_depth (8, 10, 12 or 16) is the depth of the integer RGB
 * grid between the two steps and picks the handle's tone tables, and must not be under img.depth - what c.depth is to
 * ce_batch_set_*_yuv_cicp.  rgb_depth = img.depth is what the decoder's own RGB output handed to a CMS would have been;
 * rgb_depth = 16 keeps what the matrix produces between the samples' code points.  The composition of
 * tests/yuv_restatement.py (yuv_to_rgb with D = rgb_depth) and tests/icc_restatement.py / icc_lut_restatement.py (to_linear,
 * to_srgb) restates it in numpy (tests/yuv_icc_cases.py); the device equals it bit for bit.
 * ce_batch_set_*_yuv_icc: one image of the batch's shape into a reference / test slot of a linear, an RGB8 or a deep batch (a
 * deep side is written at its own depth), with the staging, the stream and the ordering of ce_batch_set_*_yuv; CE_MEM_HOST
 * planes are consumed on return, CE_MEM_DEVICE planes are read in place under the lifetime rule given there.
 * CE_ERR_INVALID_ARG, with the reason in ce_last_error and the batch still usable, for everything ce_batch_set_*_yuv refuses
 * about the image (the reserved lut field included), a null handle, a profile of another device, and rgb_depth outside {8,
 * 10, 12, 16} or under img.depth.  (ce_batch_set_*_yuv on a linear batch stays refused.)
 * ce_yuv_icc_to_linear / _to_srgb8 / _to_srgb16: one image of width x height to packed float RGB, u8 sRGB codes or u16 sRGB
 * codes of depth_out bits (8, 10, 12 or 16) in host memory (out_len = width * height * 3 samples); errors as above,
 * CE_ERR_BAD_LENGTH for a wrong out_len.
 * Not part of this: chroma sitings other than the centred one, alpha planes and the *_over calls with planes, Gray and CMYK
 * profiles, ce_ref_* handles and the pooled ce_eval_batch, gain maps on planes. */
struct ce_icc; /* the handle ce_icc_create / ce_icc_lut_create make: ce_icc, in the ICC section below */
int ce_batch_set_reference_yuv_icc(ce_batch *b, uint32_t ref_index, const ce_yuv_image *image, uint32_t rgb_depth, const struct ce_icc *icc);
int ce_batch_set_test_yuv_icc(ce_batch *b, uint32_t pair_index, uint32_t ref_index, const ce_yuv_image *image, uint32_t rgb_depth, const struct ce_icc *icc);
int ce_yuv_icc_to_linear(ce_ctx *ctx, const ce_yuv_image *image, uint32_t rgb_depth, const struct ce_icc *icc, uint32_t width, uint32_t height, float *out, size_t out_len);
int ce_yuv_icc_to_srgb8(ce_ctx *ctx, const ce_yuv_image *image, uint32_t rgb_depth, const struct ce_icc *icc, uint32_t width, uint32_t height, uint8_t *out, size_t out_len);
int ce_yuv_icc_to_srgb16(ce_ctx *ctx, const ce_yuv_image *image, uint32_t rgb_depth, const struct ce_icc *icc, uint32_t width, uint32_t height, uint32_t depth_out, uint16_t *out, size_t out_len);

/* HLG ingest: integer RGB code values, or Y'CbCr planes, in BT.2100 Hybrid Log-Gamma (H.273 transfer
 * 18) -> a slot of a linear batch, on the device.  HLG is scene-referred: the inverse OETF is per channel, but the OOTF that
 * turns scene light into display light scales all three channels by Ys^(gamma - 1), Ys the pixel's scene luminance and gamma
 * a function of the display's peak luminance.  So HLG is no per-channel table and ce_colour has no field for the display: it
 * has a description and calls of its own, and transfer 18 through ce_transfer_table and the *_cicp calls stays refused.
 * Definition, per pixel of a CE_PIXEL_RGB8 / RGBA8 / RGB16 / RGBA16 image (alpha dropped; 8-bit formats require depth 8;
 * maxv = 2^depth - 1):
 *   1. e_c = hlg_table[min(v_c, maxv)] per channel.  The table is built on the host in f64 per code point x = v / maxv and
 *      rounded once to f32: E = x^2 / 3 for x <= 1/2, E = (exp((x - c) / a) + b) / 12 otherwise, with BT.2100's a = 0.17883277,
 *      b = 0.28466892, c = 0.55991073 (ce_hlg_table).  hlg_table[0] = 0, hlg_table[maxv] = 1.0f exactly (the f64 value
 *      1.00000003 rounds there).  The curve is never evaluated on the device.
 *   2. ys = (kR * (double)e_r + kG * (double)e_g) + kB * (double)e_b in f64, every product and sum rounded separately; kR, kG,
 *      kB are the Y row of the f64 XYZ <- src matrix of the tagged primaries, the one ce_colour_matrix starts from (BT.2020:
 *      0.2627, 0.6780, 0.0593 at four decimals).
 *   3. s = ys > 0 ? hlg_pow(ys, gamma - 1) : 0;  k = (float)(A * s) with A = (double)peak_nits / (double)white_nits: one f64
 *      product, one rounding to f32.  Black level L_B = 0.
 *   4. d_c = k * e_c in f32, one product per channel: display light, 1.0 = white_nits.
 *   5. primaries other than 1: the separately rounded f32 3 x 3 of the CICP definition's step 3; then its step 4, the clamp of
 *      a linear image.
 * gamma = system_gamma if that is non-zero, else BT.2100's 1.2 + 0.42 * log10(peak_nits / 1000) evaluated on the host in f64
 * (1000 nits: 1.2); it must lie in [0.8, 1.6].  system_gamma = 1 with peak_nits = white_nits makes k exactly 1.0f: the output
 * for primaries 1 is then the table, bit for bit.
 * hlg_pow(x, g) is part of the definition, not a library call: no two libraries' pow agree to the last bit.  It is a fixed
 * sequence of IEEE f64 operations - add, multiply, divide, integer work on the exponent bits, one round-to-nearest-integer -
 * each correctly rounded on the device and on a host alike (codec-eval_amd/csrc/hlg_pixel.h; tests/hlg_restatement.py runs the
 * same sequence on numpy f64 arrays):
 *   x = m * 2^e with m in [sqrt(1/2), sqrt(2)) (bits; m >= 1.4142135623730951 is halved);  t = (m - 1) / (m + 1);
 *   ln m = (2 t) * P(t^2), P = 1 + t^2 (1/3 + t^2 (1/5 + ... + t^2 / 21)) in Horner form from 1/21 down;
 *   y = g * (ln m + e * ln2), ln2 = 0.6931471805599453;  n = rint(y / ln2);  f = y - n * ln2;
 *   exp f = 1 + f (1 + f (1/2 + f (1/6 + ... + f / 14!))) in Horner form from 1/14! down;  result = exp f * 2^n (bits).
 * It stays within 1e-13 relative of the real power (measured: 5e-15) for x in [2^-40, 2] and g in [-0.2, 0.6] - six orders
 * under an f32 half-ulp - and hlg_pow(x, 0) = 1 exactly.
 * tests/hlg_restatement.py restates all of this in numpy; the device equals it bit for bit, on every float.
 * ce_batch_set_*_hlg / ce_hlg_to_linear take exactly what ce_batch_set_*_cicp / ce_cicp_to_linear take, with their staging,
 * stream and ordering.  ce_batch_set_*_yuv_hlg / ce_yuv_hlg_to_linear take what ce_batch_set_*_yuv_cicp / ce_yuv_to_linear
 * take (CE_MEM_HOST planes consumed on return, CE_MEM_DEVICE planes read in place under the same lifetime rule); their
 * definition is the composition of ce_yuv_to_rgb16(img, depth_out = h.depth) and ce_hlg_to_linear(rgb as CE_PIXEL_RGB16, h) and
 * adds no arithmetic; h.depth must not be under img.depth.
 * CE_ERR_INVALID_ARG, with the reason in ce_last_error and the batch still usable: a batch that is not linear, a null
 * pointer, another format, an 8-bit format with depth != 8, primaries or depth outside the lists, peak_nits or white_nits
 * that is not finite and > 0, a gamma - given or derived - outside [0.8, 1.6] or NaN, h.depth < img.depth, everything *_yuv
 * refuses about the image, slot indices past the batch.  CE_ERR_BAD_LENGTH for a wrong len or out_len.
 * Not part of this: a non-zero black level L_B, BT.2390's extended gamma rule, HLG -> PQ transcoding, limited-range RGB,
 * non-D65 whites, ce_ref_* handles and the pooled ce_eval_batch on linear batches. */
typedef struct ce_hlg {
    int primaries;      /* H.273 ColourPrimaries: 1, 9 or 12 (BT.2100 itself: 9) */
    uint32_t depth;     /* 8, 10, 12 or 16; samples above 2^depth - 1 are clamped */
    float peak_nits;    /* L_W, the display's nominal peak luminance, > 0 */
    float system_gamma; /* 0: BT.2100's rule from peak_nits; otherwise used as given; the result must lie in [0.8, 1.6] */
    float white_nits;   /* the luminance that becomes 1.0, > 0 (203 is the usual suggestion) */
} ce_hlg;               /* 20 bytes */
int ce_batch_set_reference_hlg(ce_batch *b, uint32_t ref_index, const void *pixels, size_t len, int format, const ce_hlg *h);
int ce_batch_set_test_hlg(ce_batch *b, uint32_t pair_index, uint32_t ref_index, const void *pixels, size_t len, int format, const ce_hlg *h);
int ce_hlg_to_linear(ce_ctx *ctx, const void *pixels, size_t len, int format, const ce_hlg *h, uint32_t w, uint32_t height, float *out,
                     size_t out_len);
int ce_batch_set_reference_yuv_hlg(ce_batch *b, uint32_t ref_index, const ce_yuv_image *image, const ce_hlg *h);
int ce_batch_set_test_yuv_hlg(ce_batch *b, uint32_t pair_index, uint32_t ref_index, const ce_yuv_image *image, const ce_hlg *h);
int ce_yuv_hlg_to_linear(ce_ctx *ctx, const ce_yuv_image *image, const ce_hlg *h, uint32_t width, uint32_t height, float *out, size_t out_len);
/* Pure host functions: the inverse-OETF table (n = 2^depth entries), and kR, kG, kB, gamma - 1, A of a description - exactly
 * what the kernel is handed.  CE_ERR_INVALID_ARG for what the calls above refuse about depth and description. */
int ce_hlg_table(uint32_t depth, float *out, size_t n);
int ce_hlg_params(const ce_hlg *h, double out[5]);

/* Gain-map ingest: an SDR base image, a small 8-bit gain map and a few numbers of metadata - what an
 * Ultra HDR JPEG or a gain-map AVIF / HEIC / JPEG XL file carries, as ISO 21496-1 describes it - -> the HDR rendition in a
 * slot of a linear batch, on the device.  The formula below is the ISO 21496-1 / Adobe gain-map application as its authors
 * recalled it; it has not been checked against the text of the standard, so THIS text is the contract, not the standard.
 * The base is an image of the batch's shape w x h in CE_PIXEL_RGB8 / RGBA8 / RGB16 / RGBA16 (alpha dropped), read by a
 * ce_colour exactly as step 1 of the CICP definition reads it.  The map is gw x gh samples of `channels` (1 or 3) bytes,
 * tightly packed, with 1 <= gw <= w and 1 <= gh <= h, in host memory and consumed on return; it carries no length of its
 * own: gw * gh * channels bytes are read (the bindings check their containers).  Gains and headrooms are log2 values; with
 * channels == 1 only index 0 of each array of the metadata is read, and serves all three colour channels.
 * Per channel c of the map, on the host in f64 (ce_gainmap_weight, ce_gainmap_tables), every operation rounded separately:
 *   W      = clamp((display_headroom - base_headroom) / (alternate_headroom - base_headroom), 0, 1)
 *   Y_c[v] = W * (gain_min_c + (gain_max_c - gain_min_c) * (v / 255)^(1 / gamma_c))   for v = 0 .. 255
 * with the power the host libm's pow, and no power at all for gamma_c == 1, so that Y_c is then affine in v to the last bit.
 * W == 0 gives a table of zeros.
 * Per pixel (x, y) of the base, on the device, every f32 and f64 operation rounded separately (no fused multiply-add):
 *   1. t_c = table[min(v_c, maxv)] in f32, the CICP definition's step 1.
 *   2. The map is sampled with centres aligned and edges clamped, in integers:
 *        nx = clamp((2x + 1) * gw - w, 0, (gw - 1) * 2w);  i0 = nx / (2w);  i1 = min(i0 + 1, gw - 1);
 *        fx = (double)(nx - i0 * 2w) / (double)(2w);   the same in y with gh and h, giving j0, j1, fy.
 *      A map of the base's own size has fx = fy = 0 everywhere.
 *   3. lerp(a, b, f) = a + f * (b - a), three operations;  m_ji = the map's sample at column i of row j;
 *        y_c = lerp(lerp(Y_c[m_j0i0], Y_c[m_j0i1], fx), lerp(Y_c[m_j1i0], Y_c[m_j1i1], fx), fy).
 *      The table values - log2 gains - are interpolated; for gamma 1 that is the interpolation of the encoded map.  A
 *      constant map gives Y_c[v] exactly.
 *   4. g_c = gm_exp2(y_c):  n = rint(y), f = (y - n) * 0.6931471805599453, exp f = the degree-14 Taylor series in Horner form
 *      from 1/14! down that hlg_pow ends with, result = exp f * 2^n with 2^n built from bits.  gm_exp2 of an integer is exactly
 *      that power of two; on [-16, 16] it stays within 1e-15 relative of the real 2^y (measured: 2.3e-16 against numpy.exp2).
 *   5. o_c = (float)(((double)t_c + base_offset_c) * g_c - alternate_offset_c): one f64 sum, product and difference, one
 *      rounding to f32.  A single-channel map computes one y and one g per pixel.
 *   6. The CICP definition's steps 3 and 4 - the f32 matrix for primaries other than 1, the clamp of a linear image: the gain
 *      is applied in the base's primaries.
 * Exact anchors: W == 0 with zero offsets gives ce_cicp_to_linear(base) bit for bit; a constant map with gain_min = gain_max
 * = 1, W = 1 and zero offsets gives exactly twice that (before the clamp).
 * tests/gainmap_restatement.py restates all of this in numpy; the device equals it bit for bit, on every float.
 * ce_batch_set_*_gainmap: one image into a reference / test slot of a LINEAR batch with the staging, stream and ordering of
 * ce_batch_set_*_cicp.  ce_gainmap_to_linear: one w x h image to packed float RGB in host memory (out_len = w * h * 3).
 * CE_ERR_INVALID_ARG, with the reason in ce_last_error and the batch still usable: everything ce_batch_set_*_cicp refuses
 * about the base, a batch that is not linear, a null pointer, channels other than 1 or 3, a map dimension of 0 or above the
 * base's, and in the metadata that is read: a value that is not finite, gamma <= 0, gain_min > gain_max, |gain| or
 * |headroom| above 16, |offset| above 1, alternate_headroom == base_headroom.  CE_ERR_BAD_LENGTH for a wrong len or out_len.
 * Not part of this: gain application in the alternate image's primaries, Y'CbCr-plane bases and device-resident sources,
 * maps deeper than 8 bits, interpolation other than bilinear, parsing of the containers' metadata boxes (XMP / ISO box),
 * ce_ref_* handles and the pooled ce_eval_batch on linear batches. */
typedef struct ce_gainmap_image {
    const uint8_t *samples; /* height rows of width * channels bytes, no padding */
    uint32_t width, height, channels;
} ce_gainmap_image;
typedef struct ce_gainmap {
    float gain_min[3], gain_max[3]; /* log2 of the smallest and the largest gain the map encodes */
    float gamma[3];                 /* > 0: the map stores ((log2 gain - min) / (max - min))^gamma */
    float base_offset[3], alternate_offset[3];
    float base_headroom, alternate_headroom; /* log2 of the two renditions' HDR headroom */
    float display_headroom;                  /* log2 of the headroom to render for */
} ce_gainmap;                                /* 72 bytes */
int ce_batch_set_reference_gainmap(ce_batch *b, uint32_t ref_index, const void *pixels, size_t len, int format, const ce_colour *c,
                                   const ce_gainmap_image *map, const ce_gainmap *g);
int ce_batch_set_test_gainmap(ce_batch *b, uint32_t pair_index, uint32_t ref_index, const void *pixels, size_t len, int format,
                              const ce_colour *c, const ce_gainmap_image *map, const ce_gainmap *g);
int ce_gainmap_to_linear(ce_ctx *ctx, const void *pixels, size_t len, int format, const ce_colour *c, const ce_gainmap_image *map,
                         const ce_gainmap *g, uint32_t w, uint32_t h, float *out, size_t out_len);
/* Pure host functions: the log2-gain tables (n = 256 * channels doubles, channel by channel) and W - exactly what the kernel
 * is handed.  CE_ERR_INVALID_ARG for what the calls above refuse about channels and metadata. */
int ce_gainmap_tables(const ce_gainmap *g, uint32_t channels, double *out, size_t n);
int ce_gainmap_weight(const ce_gainmap *g, double *w);

/* ---- HDR fidelity of linear batches: PQ-PSNR and BT.2124 Delta E ITP ----------------------------------
 * The two plain fidelity numbers HDR encoders are compared by, next to the perceptual scores: PSNR of the PQ code values, and
 * the Delta E ITP of Rec. ITU-R BT.2124 as a mean and a maximum over the pixels.  A linear batch has no integer grid of its
 * own (which is why CE_METRIC_PSNR stays clear on it), so the call names one: `depth` (10, 12 or 16; maxv = 2^depth - 1) and
 * `white_nits`, the luminance of sample value 1.0, finite and > 0 - Butteraugli's intensity target, the PQ ingest's white_nits.
 * The definition is made of integers and correctly rounded IEEE operations only; everything that is summed is an integer, so
 * the results do not depend on the order of summation.
 * Thresholds.  T[c] = f32(PQ_EOTF((c - 0.5) / maxv) / white_nits) for c = 1 .. maxv, built on the host in f64 with ST 2084's
 *   constants and operation order exactly as ce_transfer_table's PQ branch has them (e = (c - 0.5) / maxv, p = e^(1/m2),
 *   nits = 10000 * (max(p - c1, 0) / (c2 - c3 p))^(1/m1), T = nits / white_nits) and rounded once to f32
 *   (ce_pq_code_thresholds; out[c - 1] = T[c]).  code(x) = the number of c with T[c] <= x, a binary search:
 *   numpy.searchsorted(T, x, side="right").  Negatives, zero and NaN give 0, anything at or above T[maxv] gives maxv.  The PQ
 *   curve is never evaluated on the device.  code(ce_transfer_table(16, depth, white_nits)[v]) = v for every v: the search
 *   inverts the PQ ingest exactly.
 * Per pixel of either image (linear light, sRGB primaries):
 *   1. q = A rgb, q_i = (A[i][0] * r + A[i][1] * g) + A[i][2] * b in f32, every product and sum rounded separately (no fused
 *      multiply-add: the form of the CICP definition's step 3).  A = the inverse of ce_colour_matrix(9) - of that f32 matrix,
 *      widened to f64, inverted by its adjugate in f64 and rounded once to f32: BT.2020 <- sRGB primaries.
 *   2. l = B q in the same form, B = BT.2100's [[1688, 2146, 262], [683, 2951, 462], [99, 309, 3688]] / 4096, exact in f32.
 *      (ce_hdr_fidelity_matrices returns A and B, row-major.)
 *   3. Rc, Gc, Bc = code(q);  Lc, Mc, Sc = code(l).
 *   4. in 64-bit integers, exactly: i = 2048 (Lc + Mc), ct = 6610 Lc - 13613 Mc + 7003 Sc, cp = 17933 Lc - 17390 Mc - 543 Sc:
 *      BT.2100's ICtCp times 4096 * maxv.  BT.2124's T is Ct / 2.
 * Per pair, d* = reference minus test:
 *   pq_sse       = the sum over the pixels of dRc^2 + dGc^2 + dBc^2, in u64.
 *   per pixel      s = (di * di + 0.25 * (dct * dct)) + dcp * dcp in f64, the integer differences converted first and every
 *                  operation rounded separately; e = 720 * sqrt(s) / (4096 * maxv) with a correctly rounded sqrt, the product
 *                  before the quotient; k = (u64) rint(e * 2^20), under 2^33.
 *   itp_sum_q20  = the sum of k;  itp_max_q20 = the maximum of k.
 *   pq_psnr          = 10 log10(maxv^2 / (pq_sse / (3 n))) in f64, n the pixels of an image; identical codes: what PSNR
 *                      returns for identical images, +infinity
 *   delta_e_itp_mean = itp_sum_q20 / 2^20 / n;  delta_e_itp_max = itp_max_q20 / 2^20.
 * tests/hdr_fidelity_restatement.py restates this in numpy; the device equals it bit for bit. */
typedef struct ce_hdr_scores {
    double pq_psnr;          /* dB; +infinity when no PQ code differs */
    double delta_e_itp_mean; /* BT.2124 Delta E ITP, mean over the pixels (1 is about one just noticeable difference) */
    double delta_e_itp_max;  /* ... and its maximum */
    uint64_t pq_sse;         /* the exact integers the three are finished from */
    uint64_t itp_sum_q20;
    uint64_t itp_max_q20;
} ce_hdr_scores;             /* 48 bytes */
/* Scores pairs [0, n_pairs) of a LINEAR batch into out[0 .. n_pairs): one kernel on the context's stream, ordered behind the
 * uploads queued so far as a launch is; blocks until the scores are on the host.  ce_scores, its `valid` bits and whatever
 * ce_batch_launch left to collect are untouched.  CE_ERR_INVALID_ARG, with the reason in ce_last_error and the batch still
 * usable, for a batch that is not linear, a depth other than 10, 12 or 16, a white_nits that is not finite and > 0, a null
 * pointer, n_pairs of 0 or past the batch. */
int ce_batch_hdr_fidelity(ce_batch *b, uint32_t n_pairs, uint32_t depth, float white_nits, ce_hdr_scores *out);
/* One pair of packed float RGB through the same kernel (lengths in bytes: width * height * 12; NaN -> 0 and the clamp of a
 * linear image apply, as in ce_eval_pair_linear).  CE_ERR_INVALID_ARG as above and for an empty image, CE_ERR_BAD_LENGTH for a
 * length that is not width * height * 12. */
int ce_eval_pair_hdr_fidelity(ce_ctx *ctx, const float *reference, size_t reference_len, const float *test, size_t test_len,
                              uint32_t width, uint32_t height, uint32_t depth, float white_nits, ce_hdr_scores *out);
/* Pure host functions: the thresholds (n = 2^depth - 1 entries, out[c - 1] = T[c]; CE_ERR_INVALID_ARG for another depth or n,
 * a null pointer, a white_nits that is not finite and > 0) and the two matrices, row-major - exactly what the kernel is
 * handed. */
int ce_pq_code_thresholds(uint32_t depth, float white_nits, float *out, size_t n);
int ce_hdr_fidelity_matrices(float a[9], float b[9]);

/* ---- Delta E ITP per pixel, per cell and over thresholds ----------------------------------------------
 * Where a pair is bad, and how much of it: for every pixel of a pair of a LINEAR batch, k exactly as defined above for `depth`
 * and `white_nits` - Delta E ITP in units of 2^-20 - and nothing new in arithmetic.
 * Map value.  m = min(k, 2^32 - 1) as uint32_t.  The saturation is real: k needs 33 bits for pairs of imaginary colours inside
 *   +-CE_LINEAR_MAX (about 6.9e9, a Delta E ITP of 6500, nine times black to peak), so a map value of 2^32 - 1 reads "4096 or
 *   more"; the scores above carry k in 64 bits and do not saturate.  map.sum() = itp_sum_q20 and map.max() = itp_max_q20 for
 *   every pair whose k stay under 2^32.
 * block.  1: the map itself, [h][w].  A power of two up to 64: the MAXIMUM of m over each block x block cell, edge cells clipped
 *   to the image, [ceil(h / block)][ceil(w / block)] - ce_batch_butteraugli_diffmap's rules.
 * Exceedance counts.  over[j] = the number of pixels of the pair with m > thresholds_q20[j] (same units; CE_DELTA_E_ITP_Q20
 *   is 1.0), for up to CE_DELTA_E_ITP_MAX_THRESHOLDS thresholds: exact integers over the pixels, never over cells, whatever
 *   `block` is.  A threshold of 2^32 - 1 counts nothing.
 * Everything is an integer maximum or an integer sum, so nothing depends on the grid or on the order.
 * The call scores pairs [first, first + count) in one kernel on the context's stream, ordered behind the uploads queued so far
 * as a launch is, with the pair table of the last bind; it blocks until the results are on the host.  ce_scores, stored maps,
 * the HDR fidelity scores and whatever ce_batch_launch left to collect are untouched.  `map` receives
 * [count][ceil(h / block)][ceil(w / block)] values and map_len is that number of ELEMENTS; `over` receives
 * [count][n_thresholds].  map may be NULL with map_len 0 (counts only: no map is stored and no map memory allocated), over may
 * be NULL with n_thresholds 0 and thresholds_q20 NULL, not both.  The device buffer of the maps of one call (map_len * 4
 * bytes; at block 1, count * w * h * 4) is a grow-only buffer of the batch, freed with it; it is outside
 * ce_estimate_batch_bytes.
 * CE_ERR_INVALID_ARG, with the reason in ce_last_error and the batch still usable: a null batch; a batch that is not linear; a
 * depth other than 10, 12 or 16; a white_nits that is not finite and > 0; both outputs NULL; count of 0 or a range past the
 * batch's max_pairs; a block that is not 1, 2, 4, 8, 16, 32 or 64; a map_len other than the above; n_thresholds above 8; over
 * without thresholds; thresholds without over. */
#define CE_DELTA_E_ITP_MAX_THRESHOLDS 8
#define CE_DELTA_E_ITP_Q20 1048576u
int ce_batch_delta_e_itp_map(ce_batch *b, uint32_t first, uint32_t count, uint32_t depth, float white_nits, uint32_t block,
                             uint32_t *map, size_t map_len, const uint32_t *thresholds_q20, uint32_t n_thresholds, uint64_t *over);
/* One pair of packed float RGB through the same kernel, as ce_eval_pair_hdr_fidelity: lengths in bytes (width * height * 12),
 * NaN -> 0 and the clamp of a linear image apply.  CE_ERR_INVALID_ARG as above and for a null image or an empty one,
 * CE_ERR_BAD_LENGTH for a length that is not width * height * 12. */
int ce_eval_pair_delta_e_itp_map(ce_ctx *ctx, const float *reference, size_t reference_len, const float *test, size_t test_len,
                                 uint32_t width, uint32_t height, uint32_t depth, float white_nits, uint32_t block, uint32_t *map,
                                 size_t map_len, const uint32_t *thresholds_q20, uint32_t n_thresholds, uint64_t *over);

/* ---- SSIM and MS-SSIM of RGB8 and deep batches, exactly -------------------------------------------------
 * The two numbers learned-codec papers tabulate beside PSNR, in the form they use (Wang et al. 2003 as the frameworks' MS-SSIM
 * packages compute it): an 11-tap Gaussian window of sigma 1.5, "valid" filtering, each of R, G and B on the encoded sample values, 2 x 2 mean
 * pooling between five scales.  A call of its own beside the launch, as HDR fidelity is.  Everything is pinned to f64
 * operations in a stated order and the per-pixel values are summed as integers, so no result depends on the grid or on the
 * order of summation.
 * Samples.  The integers in the slabs of an RGB8 batch, or of a deep batch whose two sides have EQUAL depth d; L = 2^d - 1
 *   (255 for RGB8).  Each channel c of R, G, B separately.
 * Window.  g[0 .. 10], symmetric, g[i] = g[10 - i]; g[0 .. 5] are the doubles 0.00102838008447911, 0.007598758135239185,
 *   0.03600077212843083, 0.10936068950970002, 0.2130055377112537, 0.26601172486179436: exp(-(i - 5)^2 / 4.5) divided by their
 *   sum in index order, as numpy gives them; literals in the library, not computed at run time (ce_msssim_window).
 * Filter F(p) of a plane p of h x w doubles, h, w >= 11.  First down the columns, v[y][x] = sum_i g[i] * p[y + i][x], (h - 10)
 *   x w; then along the rows, o[y][x] = sum_i g[i] * v[y][x + i], (h - 10) x (w - 10).  Each sum starts at +0.0 and adds the
 *   taps in order i = 0 .. 10; every product and every sum is rounded separately in f64 (no fused multiply-add); v stays f64.
 * Per level and channel, x the reference plane and y the test plane, both f64:
 *   mx = F(x), my = F(y);  sxx = F(x * x) - mx * mx, syy = F(y * y) - my * my, sxy = F(x * y) - mx * my;
 *   C1 = (0.01 * L) * (0.01 * L) and C2 = (0.03 * L) * (0.03 * L) in f64;
 *   cs = (2.0 * sxy + C2) / ((sxx + syy) + C2);  lum = (2.0 * (mx * my) + C1) / ((mx * mx + my * my) + C1);  s = lum * cs.
 *   The divisions are correctly rounded and the parentheses are as written, so identical images give exactly 1.0 everywhere.
 *   qs = (int64) rint(s * 2^32) and qc = (int64) rint(cs * 2^32), ties to even.  ssim_q[level][c] = the sum of qs over the
 *   (h - 10) x (w - 10) positions, cs_q[level][c] = the sum of qc: signed 64-bit, possibly negative.  n[level] = the number
 *   of positions.
 * Next level.  From level planes p of h x w, with ph = h & 1 and pw = w & 1: q = p with ph rows of zeros above and pw columns
 *   of zeros on the left; next[Y][X] = ((q[2Y][2X] + q[2Y][2X+1]) + (q[2Y+1][2X] + q[2Y+1][2X+1])) * 0.25, shape
 *   ((h + ph) / 2) x ((w + pw) / 2): avg_pool2d(2, padding = size % 2) with the pad counted in the divisor.  Every value is a
 *   dyadic rational of at most 16 + 8 bits, exact in f32 and f64 (the pyramid is stored in f32); x * x and x * y are exact in f64.
 * levels.  1 (SSIM; needs min(w, h) >= 11) or 5 (MS-SSIM; needs min(w, h) > 160: its last level is at least 11 x 11).
 * Finishing, on the host in f64.  ms[l][c] = ((double) ssim_q[l][c] / 4294967296.0) / n[l], mc[l][c] the same from cs_q;
 *   ssim_rgb[c] = ms[0][c];  ms_ssim_rgb[c] = the product over l = 0 .. 3 of pow(max(mc[l][c], 0), wt[l]), multiplied in level
 *   order, then multiplied by pow(max(ms[4][c], 0), wt[4]), wt = {0.0448, 0.2856, 0.3001, 0.2363, 0.1333};
 *   ssim = ((ssim_rgb[0] + ssim_rgb[1]) + ssim_rgb[2]) / 3.0, ms_ssim the same over ms_ssim_rgb.  With levels = 1 the MS-SSIM
 *   fields are NaN and n_levels is 1; the integers of levels that did not run are 0.
 * tests/msssim_restatement.py restates this in numpy; the device equals it on every integer. */
#define CE_MSSSIM_LEVELS 5
typedef struct ce_msssim_scores {
    double ms_ssim;         /* NaN with levels = 1 */
    double ssim;            /* level 0's mean SSIM over R, G, B */
    double ms_ssim_rgb[3];
    double ssim_rgb[3];
    int64_t ssim_q[5][3];   /* the exact integers the doubles are finished from: [level][channel] */
    int64_t cs_q[5][3];
    uint64_t n[5];          /* positions of a level: (h_l - 10) * (w_l - 10) */
    uint32_t n_levels;
    uint32_t reserved;      /* 0 */
} ce_msssim_scores;         /* 352 bytes */
/* Scores pairs [0, n_pairs) of an RGB8 or equal-depth deep batch into out[0 .. n_pairs): on the context's stream, ordered behind
 * the uploads queued so far as a launch is, with the pair table of the last bind; blocks until the scores are on the host.
 * ce_scores, the stored maps and whatever ce_batch_launch left to collect are untouched.  Each reference slot the pairs name is
 * pooled once.  The pyramid of levels 1 - 4 (f32, 4/3 bytes per sample of every slot of the batch) is a grow-only buffer of the
 * batch, made by the first call with levels = 5 and freed with the batch; it is outside ce_estimate_batch_bytes.
 * CE_ERR_INVALID_ARG, with the reason in ce_last_error and the batch still usable: a linear batch; a deep batch of unequal
 * depths; levels other than 1 or 5; an image too small for `levels`; a null pointer; n_pairs of 0 or past the batch. */
int ce_batch_msssim(ce_batch *b, uint32_t n_pairs, uint32_t levels, ce_msssim_scores *out);
/* One pair of packed RGB8 host images (lengths in bytes: width * height * 3), and one pair of packed u16 RGB of one `depth`
 * (8, 10, 12 or 16; width * height * 6 bytes), through the context's one-pair batches.  CE_ERR_INVALID_ARG as above and for an
 * empty image, CE_ERR_BAD_LENGTH for a length that is not the image's. */
int ce_eval_pair_msssim(ce_ctx *ctx, const uint8_t *reference, size_t reference_len, const uint8_t *test, size_t test_len,
                        uint32_t width, uint32_t height, uint32_t levels, ce_msssim_scores *out);
int ce_eval_pair_msssim_deep(ce_ctx *ctx, const uint16_t *reference, size_t reference_len, const uint16_t *test, size_t test_len,
                             uint32_t depth, uint32_t width, uint32_t height, uint32_t levels, ce_msssim_scores *out);
/* Pure host functions: the window's eleven literals, and the geometry of the levels of a w x h image - *n_levels = levels and
 * level_w / level_h [0 .. levels) - with CE_ERR_INVALID_ARG for a null pointer, levels other than 1 or 5 and an image too small. */
int ce_msssim_window(double out[11]);
int ce_msssim_levels(uint32_t w, uint32_t h, uint32_t levels, uint32_t *n_levels, uint32_t *level_w, uint32_t *level_h);

/* ---- SSIM and MS-SSIM per position, per cell and over thresholds ----------------------------------------
 * Where a pair is bad, and how much of it, at one level of the pyramid above: the very integers ce_batch_msssim sums, before
 * they are summed, and nothing new in arithmetic.
 * Position values.  For a pair, a level l of the pyramid defined above (samples, window, filter F, C1, C2, next level: all
 *   unchanged) and a channel c, at each of the vh x vw = (h_l - 10) x (w_l - 10) valid positions: qs = (int64) rint(s * 2^32)
 *   and qc = (int64) rint(cs * 2^32) exactly as defined above - the same filter order, parentheses and quotients.
 * Map value.  A dissimilarity in units of 2^-32 (CE_MSSSIM_Q32 is 1.0) as uint32_t: d = min(max(2^32 - q, 0), 2^32 - 1), q =
 *   qs with what = CE_MSSSIM_MAP_SSIM and qc with what = CE_MSSSIM_MAP_CS.  Identical images give 0 everywhere.  The
 *   saturation is real: s and cs can be zero or negative (a pattern against its inverse), so a map value of 2^32 - 1 reads
 *   "SSIM of 2^-32 or less, negatives included"; a q above 2^32, should rounding ever give one, reads 0.  The sums above
 *   carry q signed in 64 bits and do not saturate.  For every (pair, level, channel) none of whose q lies outside
 *   [1, 2^32]:  n[l] * 2^32 - map.sum() == ssim_q[l][c]  (cs_q[l][c] with CE_MSSSIM_MAP_CS), both from ce_batch_msssim on the
 *   same pair.
 * block.  1: the map itself, [vh][vw].  A power of two up to 64: the MAXIMUM of d over each block x block cell of the valid
 *   region, edge cells clipped to the region, [ceil(vh / block)][ceil(vw / block)] - ce_batch_delta_e_itp_map's rules.
 * Exceedance counts.  over[pair][c][j] = the number of valid positions with d > thresholds_q32[j] (same units), for up to
 *   CE_MSSSIM_MAP_MAX_THRESHOLDS thresholds: exact integers over the positions, never over cells, whatever `block` is.  A
 *   threshold of 2^32 - 1 counts nothing.
 * levels, level.  levels is 1 or 5 by ce_msssim_levels' rule, level in [0, levels): one level per call.  The pyramid is pooled
 *   only as far as `level`, for the reference slots that pairs [first, first + count) name - once each - and those pairs' test
 *   slots.
 * Everything is an integer maximum, an integer sum or a plain store, so nothing depends on the grid or on the order.
 * The call runs on the context's stream, ordered behind the uploads queued so far as a launch is, with the pair table of the
 * last bind; it blocks until the results are on the host.  ce_scores, stored maps, the integers ce_batch_msssim keeps and
 * whatever ce_batch_launch left to collect are untouched.  `map` receives [count][3][ceil(vh / block)][ceil(vw / block)] values
 * and map_len is that number of ELEMENTS; `over` receives [count][3][n_thresholds].  map may be NULL with map_len 0 (counts only:
 * no map is stored and no map memory allocated), over may be NULL with n_thresholds 0 and thresholds_q32 NULL, not both.  The
 * device buffer of the maps of one call (map_len * 4 bytes) and the counts are grow-only buffers of the batch, freed with it;
 * like the pyramid they are outside ce_estimate_batch_bytes.
 * CE_ERR_INVALID_ARG, with the reason in ce_last_error and the batch still usable: a null batch; a linear batch; a deep batch
 * of unequal depths; levels other than 1 or 5; an image too small for `levels`; level >= levels; what above 1; both outputs
 * NULL; count of 0 or a range past the batch's max_pairs; a block that is not 1, 2, 4, 8, 16, 32 or 64; a map_len other than
 * the above; n_thresholds above 8; over without thresholds; thresholds without over.
 * tests/msssim_map_restatement.py restates this in numpy; the device equals it on every element. */
#define CE_MSSSIM_MAP_MAX_THRESHOLDS 8
#define CE_MSSSIM_Q32 4294967296ull
enum { CE_MSSSIM_MAP_SSIM = 0, CE_MSSSIM_MAP_CS = 1 };
int ce_batch_msssim_map(ce_batch *b, uint32_t first, uint32_t count, uint32_t levels, uint32_t level, uint32_t what, uint32_t block,
                        uint32_t *map, size_t map_len, const uint32_t *thresholds_q32, uint32_t n_thresholds, uint64_t *over);
/* One pair of packed RGB8 host images (lengths in bytes: width * height * 3), and one pair of packed u16 RGB of one `depth`
 * (8, 10, 12 or 16; width * height * 6 bytes), through the context's one-pair batches as ce_eval_pair_msssim takes them.
 * CE_ERR_INVALID_ARG as above and for a null image or an empty one, CE_ERR_BAD_LENGTH for a length that is not the image's. */
int ce_eval_pair_msssim_map(ce_ctx *ctx, const uint8_t *reference, size_t reference_len, const uint8_t *test, size_t test_len,
                            uint32_t width, uint32_t height, uint32_t levels, uint32_t level, uint32_t what, uint32_t block,
                            uint32_t *map, size_t map_len, const uint32_t *thresholds_q32, uint32_t n_thresholds, uint64_t *over);
int ce_eval_pair_msssim_map_deep(ce_ctx *ctx, const uint16_t *reference, size_t reference_len, const uint16_t *test, size_t test_len,
                                 uint32_t depth, uint32_t width, uint32_t height, uint32_t levels, uint32_t level, uint32_t what,
                                 uint32_t block, uint32_t *map, size_t map_len, const uint32_t *thresholds_q32, uint32_t n_thresholds,
                                 uint64_t *over);

/* ---- CIEDE2000 of RGB8 and deep batches, exactly ----------------------------------------------------------
 * How far colour drifts, on average and at worst: the CIE's Delta E 2000 between the two sides of every pixel, read as sRGB.  A
 * call of its own beside the launch, as HDR fidelity and MS-SSIM are.  Every operation below is one IEEE f64 operation, rounded
 * separately (no fused multiply-add), in the order the parentheses give; the per-pixel value is quantised and everything after
 * it is an integer, so no result depends on the grid or on the order of summation.
 * Samples.  The integers in the slabs of an RGB8 batch (depth 8) or of a deep batch, each side at its own depth d (8, 10, 12 or
 *   16); the two depths may differ.  Per pixel and per side, channels R, G, B:
 * 1. Linear value.  e_c = (double) T_d[min(v_c, 2^d - 1)], T_d = ce_srgb_table(d, 0): the f32 values SSIMULACRA2 reads, widened
 *    exactly.
 * 2. XYZ (OpenCV's and scikit-image's matrix).  X = ((0.412453 * e_r) + (0.357580 * e_g)) + (0.180423 * e_b);
 *    Y = ((0.212671 * e_r) + (0.715160 * e_g)) + (0.072169 * e_b);  Z = ((0.019334 * e_r) + (0.119193 * e_g)) + (0.950227 * e_b).
 *    The white is the row sums: tx = X / 0.950456, ty = Y, tz = Z / 1.088754.
 * 3. Lab.  f(t) = cbrt(t) if t > 216.0 / 24389.0, else (((24389.0 / 27.0) * t) + 16.0) / 116.0;  fx = f(tx), fy = f(ty), fz = f(tz);
 *    L = (116.0 * fy) - 16.0;  a = 500.0 * (fx - fy);  b = 200.0 * (fy - fz).
 * 4. CIEDE2000 with kL = kC = kH = 1, in the form of Sharma, Wu and Dalal (2005); side 1 is the reference, side 2 the test:
 *    C_i = sqrt((a_i * a_i) + (b_i * b_i));  Cb = 0.5 * (C_1 + C_2);  p7(c) = (((c * c) * c) * ((c * c) * c)) * c;
 *    G = 0.5 * (1.0 - sqrt(p7(Cb) / (p7(Cb) + 6103515625.0)));  a'_i = (1.0 + G) * a_i;  C'_i = sqrt((a'_i * a'_i) + (b_i * b_i));
 *    h_i = hue(b_i, a'_i) in degrees in [0, 360), 0 when a'_i = b_i = 0;
 *    dL = L_2 - L_1;  dC = C'_2 - C'_1;  cc = C'_1 * C'_2;
 *    dh = h_2 - h_1, minus 360.0 if above 180.0, plus 360.0 if below -180.0, and 0.0 when cc == 0;
 *    dH = (2.0 * sqrt(cc)) * sin_deg(0.5 * dh);
 *    hs = h_1 + h_2;  hb = hs when cc == 0; else 0.5 * hs when |h_1 - h_2| <= 180.0; else 0.5 * (hs + 360.0) when hs < 360.0;
 *    else 0.5 * (hs - 360.0);
 *    Lb = 0.5 * (L_1 + L_2);  Cpb = 0.5 * (C'_1 + C'_2);
 *    T = (((1.0 - (0.17 * cos_deg(hb - 30.0))) + (0.24 * cos_deg(2.0 * hb))) + (0.32 * cos_deg((3.0 * hb) + 6.0)))
 *        - (0.20 * cos_deg((4.0 * hb) - 63.0));
 *    z = (hb - 275.0) / 25.0;  dtheta = 30.0 * exp(-(z * z));  R_C = 2.0 * sqrt(p7(Cpb) / (p7(Cpb) + 6103515625.0));
 *    l2 = (Lb - 50.0) * (Lb - 50.0);  S_L = 1.0 + ((0.015 * l2) / sqrt(20.0 + l2));  S_C = 1.0 + (0.045 * Cpb);
 *    S_H = 1.0 + ((0.015 * Cpb) * T);  R_T = (-sin_deg(2.0 * dtheta)) * R_C;
 *    tl = dL / S_L;  tc = dC / S_C;  th = dH / S_H;
 *    dE = sqrt(max((((tl * tl) + (tc * tc)) + (th * th)) + (R_T * (tc * th)), 0.0)) - the max because the form is positive
 *    definite only in exact arithmetic.
 * 5. q = rint(dE * 2^20), ties to even: an integer under 2^32 (dE stays under 120 for sRGB colours), the unit of
 *    ce_batch_delta_e_itp_map's values.
 * Elementary functions.  Fixed sequences of f64 + - * /, sqrt, one rint, comparisons and integer work on exponent bits; no libm
 *   and no device math library (codec-eval_amd/csrc/ciede2000_pixel.h holds them; hlg_pixel.h the exponential's series):
 *   cbrt(t), t = m * 2^e with m in [1, 2), e = 3 * k + r, r in {0, 1, 2}:  y = 0.7401 + (0.2599 * m); three times
 *     y3 = (y * y) * y, y = (y * (y3 + (m + m))) / ((y3 + y3) + m);  result ((y * c_r) * 2^k), c = {1, 1.2599210498948732,
 *     1.5874010519681994}.
 *   hue(b, a):  t = min(|a|, |b|) / max(|a|, |b|);  u = (t - 1.0) / (t + 1.0) when t > 0.41421356237309503, else t;  P = the
 *     polynomial in (u * u) with coefficients 1, -1/3, 1/5, ... 1/49 (each the correctly rounded quotient) in Horner form from
 *     1/49 down, p = (p * u2) + c;  d = (u * P) * 57.29577951308232, plus 45.0 in the first case;  d = 90.0 - d when |b| > |a|;
 *     d = 180.0 - d when a < 0;  d = 360.0 - d when b < 0;  d = d - 360.0 when d >= 360.0.
 *   sin_deg(x), cos_deg(x):  n = rint(x / 90.0);  r = x - (90.0 * n) (exact);  rr = r * 0.017453292519943295;  S = rr * the
 *     polynomial in (rr * rr) with coefficients 1, -1/3!, ... 1/17!, C = the one with 1, -1/2!, ... -1/18!, both in Horner form
 *     from the highest down;  n mod 4 = 0, 1, 2, 3 gives sin = S, C, -S, -C and cos = C, -S, -C, S.
 *   exp(y), y <= 0:  n = rint(y / 0.6931471805599453);  f = y - (n * 0.6931471805599453);  the Taylor series of exp f to degree 14
 *     in Horner form from 1/14! down, times 2^n built from bits (ce_batch_set_*_hlg's exp_times_pow2).
 * 6. Per pair, over its width * height pixels:  sum_q20 = the sum of q (64 bits);  max_q20 = the largest q;  n = the number of
 *    pixels;  n_above[k] = the number of pixels with q > thresholds_q20[k], k < n_thresholds <= CE_CIEDE2000_MAX_THRESHOLDS (the
 *    rest 0).  A threshold of 2^32 - 1 counts nothing.
 * 7. Finishing, on the host in f64:  mean = ((double) sum_q20 / 1048576.0) / (double) n;  max = (double) max_q20 / 1048576.0;
 *    ciede2000_db = 45.0 - 20.0 * log10(mean), +infinity when sum_q20 is 0.  The last is the PSNR-like form in which Daala's
 *    tools and libvmaf's feature report CIEDE2000, as remembered: it could not be verified against either where this was
 *    written, so treat the constant as this library's own.
 * Properties.  Identical samples at one depth give q = 0 exactly, and so does any pixel whose two sides hold the same table
 *   values - 8-bit v against 16-bit 257 * v.  Black against white gives q = 100 * 2^20 exactly.  The fixed sequences stay within
 *   1e-8 of the same formula through libm on 8-bit content, so q differs by at most one; of the 34 pairs of Sharma
 *   et al.'s table they reproduce 33 to the fourth decimal, and (50, -0.001, 2.49) against (50, 0.0010, -2.49), whose hues are
 *   180 degrees apart on the formula's own discontinuity, falls on the other side of it: 4.7461 for 4.8045.
 * tests/ciede2000_restatement.py restates this in numpy; the device and ce_ciede2000_pixels equal it on every integer. */
#define CE_CIEDE2000_MAX_THRESHOLDS 8
#define CE_CIEDE2000_Q20 1048576u
typedef struct ce_ciede2000_scores {
    uint64_t sum_q20;       /* the exact integers the doubles are finished from */
    uint64_t n;
    uint64_t n_above[8];    /* pixels with q > thresholds_q20[k]; 0 from n_thresholds on */
    double mean;            /* mean Delta E 2000 of the pair's pixels */
    double max;             /* the largest */
    double ciede2000_db;    /* 45 - 20 log10(mean); +infinity for a mean of 0 */
    uint32_t max_q20;
    uint32_t n_thresholds;
    uint32_t reserved[2];   /* 0 */
} ce_ciede2000_scores;      /* 120 bytes */
/* Scores pairs [0, n_pairs) of an RGB8 or deep batch into out[0 .. n_pairs): on the context's stream, ordered behind the uploads
 * queued so far as a launch is, with the pair table of the last bind; blocks until the scores are on the host.  ce_scores, the
 * stored maps and whatever ce_batch_launch left to collect are untouched.  thresholds_q20 may be NULL with n_thresholds 0.
 * CE_ERR_INVALID_ARG, with the reason in ce_last_error and the batch still usable: a linear batch (its colour difference is
 * ce_batch_hdr_fidelity's Delta E ITP); more than 8 thresholds; a null pointer (out; thresholds_q20 with n_thresholds > 0);
 * n_pairs of 0 or past the batch. */
int ce_batch_ciede2000(ce_batch *b, uint32_t n_pairs, const uint32_t *thresholds_q20, uint32_t n_thresholds, ce_ciede2000_scores *out);
/* One pair of packed RGB8 host images (lengths in bytes: width * height * 3), and one pair of packed u16 RGB at ref_depth /
 * test_depth (each 8, 10, 12 or 16; width * height * 6 bytes a side), through the context's one-pair batches.
 * CE_ERR_INVALID_ARG as above and for an empty image or a depth that is none of the four, CE_ERR_BAD_LENGTH for a length that is
 * not the image's. */
int ce_eval_pair_ciede2000(ce_ctx *ctx, const uint8_t *reference, size_t reference_len, const uint8_t *test, size_t test_len,
                           uint32_t width, uint32_t height, const uint32_t *thresholds_q20, uint32_t n_thresholds,
                           ce_ciede2000_scores *out);
int ce_eval_pair_ciede2000_deep(ce_ctx *ctx, const uint16_t *reference, size_t reference_len, const uint16_t *test, size_t test_len,
                                uint32_t ref_depth, uint32_t test_depth, uint32_t width, uint32_t height,
                                const uint32_t *thresholds_q20, uint32_t n_thresholds, ce_ciede2000_scores *out);
/* A pure host function, no GPU needed: q of n pixels, ref_rgb and test_rgb holding n * 3 samples of ref_depth / test_depth bits
 * (8, 10, 12 or 16) - the same pixel text as the kernel's, compiled for the host.  CE_ERR_INVALID_ARG for a null pointer or such
 * a depth. */
int ce_ciede2000_pixels(const uint16_t *ref_rgb, uint32_t ref_depth, const uint16_t *test_rgb, uint32_t test_depth, size_t n,
                        uint32_t *out_q20);

/* ---- CIEDE2000 per pixel, per cell and over thresholds, whole or term by term ---------------------------
 * Which pixels of a pair drift, and in which direction of colour space: for every pixel of a pair of an RGB8 or deep batch,
 * steps 1 to 4 above up to tl = dL / S_L, tc = dC / S_C, th = dH / S_H, R_T and dE, exactly as defined there - no operation is
 * new and none is reordered - and then one of four values, selected by `what`, each a uint32_t in the unit of step 5 (2^-20):
 *   CE_CIEDE2000_MAP_DE (0):  q = rint(dE * 2^20), step 5 itself: the very integer ce_batch_ciede2000 sums.
 *   CE_CIEDE2000_MAP_DL (1):  rint(|tl| * 2^20), the lightness term dL' / S_L.
 *   CE_CIEDE2000_MAP_DC (2):  rint(|tc| * 2^20), the chroma term dC' / S_C.
 *   CE_CIEDE2000_MAP_DH (3):  rint(|th| * 2^20), the hue term dH' / S_H.
 *   Magnitudes only: |x| clears the sign bit of the f64, so -0 gives 0; rint rounds ties to even.
 * Range.  No saturation rule is needed: over 400 000 random pairs of 8-bit colours and all 64 pairs of cube corners
 *   (tests/test_ciede2000_map_cpu.py) the largest values are dE 115.37 (other samples reach 116.84; step 5's bound of 120
 *   holds), |tl| 100 (black against white: the largest there is, L spanning 0 .. 100 with S_L >= 1), |tc| 33.36 and |th| 109.56,
 *   so every value stays under 2^27.
 * The terms are not bounded by dE.  dE^2 = tl^2 + tc^2 + th^2 + R_T * (tc * th), and the rotation term is negative where
 *   tc * th > 0 (R_T <= 0): of the 400 064 references above against themselves moved by up to +-3 codes, 3667 have |tc| > dE
 *   and 15 168 have |th| > dE.  Nothing promises "term <= dE"; a term map is read beside the DE map, not as a share of it.
 * Equal pixels.  A pixel whose two code triples and depths are equal has all four values 0 exactly: dL = 0, dC = 0, and dH is a
 *   multiple of sin_deg(0) = 0.  So has any pixel whose two sides hold the same table values.
 * block.  1: the map itself, [h][w].  A power of two up to 64: the MAXIMUM of the selected value over each block x block cell,
 *   edge cells clipped to the image, [ceil(h / block)][ceil(w / block)] - ce_batch_delta_e_itp_map's rules.
 * Exceedance counts.  over[j] = the number of pixels of the pair whose selected value is > thresholds_q20[j] (same unit;
 *   CE_CIEDE2000_Q20 is 1.0), for up to CE_CIEDE2000_MAX_THRESHOLDS thresholds: exact integers over the pixels, never over
 *   cells, whatever `block` is.  A threshold of 2^32 - 1 counts nothing.
 * For what = CE_CIEDE2000_MAP_DE and every pair: map.sum() == sum_q20, map.max() == max_q20 and over == n_above of
 *   ce_batch_ciede2000 with the same thresholds.
 * Everything is an integer maximum or an integer sum, so nothing depends on the grid or on the order.
 * The call works on pairs [first, first + count) on the context's stream, ordered behind the uploads queued so far as a launch
 * is, with the pair table of the last bind; it blocks until the results are on the host.  ce_scores, stored maps, the CIEDE2000
 * scores and whatever ce_batch_launch left to collect are untouched.  `map` receives [count][ceil(h / block)][ceil(w / block)]
 * values and map_len is that number of ELEMENTS; `over` receives [count][n_thresholds].  map may be NULL with map_len 0 (counts
 * only: no map is stored and no map memory allocated), over may be NULL with n_thresholds 0 and thresholds_q20 NULL, not both.
 * The device buffer of the maps of one call (map_len * 4 bytes; at block 1, count * w * h * 4) is a grow-only buffer of the
 * batch, freed with it; it is outside ce_estimate_batch_bytes, and where it cannot be had the call returns CE_ERR_BACKEND with
 * the batch still usable.
 * CE_ERR_INVALID_ARG, with the reason in ce_last_error and the batch still usable: a null batch; a linear batch (its map is
 * ce_batch_delta_e_itp_map's); a `what` above 3; both outputs NULL; count of 0 or a range past the batch's max_pairs; a block
 * that is not 1, 2, 4, 8, 16, 32 or 64; a map_len other than the above; n_thresholds above 8; over without thresholds;
 * thresholds without over.
 * tests/ciede2000_map_restatement.py restates the four values, the cells and the counts in numpy; the device and
 * ce_ciede2000_pixel_terms equal it on every integer. */
#define CE_CIEDE2000_MAP_DE 0u
#define CE_CIEDE2000_MAP_DL 1u
#define CE_CIEDE2000_MAP_DC 2u
#define CE_CIEDE2000_MAP_DH 3u
int ce_batch_ciede2000_map(ce_batch *b, uint32_t first, uint32_t count, uint32_t what, uint32_t block, uint32_t *map, size_t map_len,
                           const uint32_t *thresholds_q20, uint32_t n_thresholds, uint64_t *over);
/* One pair of packed RGB8 host images, and one pair of packed u16 RGB at ref_depth / test_depth, through the same kernel and
 * the context's one-pair batches, as ce_eval_pair_ciede2000{,_deep} take them (lengths in bytes).  CE_ERR_INVALID_ARG as above
 * and for a null image, an empty one or a depth that is none of 8, 10, 12 and 16; CE_ERR_BAD_LENGTH for a length that is not
 * the image's. */
int ce_eval_pair_ciede2000_map(ce_ctx *ctx, const uint8_t *reference, size_t reference_len, const uint8_t *test, size_t test_len,
                               uint32_t width, uint32_t height, uint32_t what, uint32_t block, uint32_t *map, size_t map_len,
                               const uint32_t *thresholds_q20, uint32_t n_thresholds, uint64_t *over);
int ce_eval_pair_ciede2000_map_deep(ce_ctx *ctx, const uint16_t *reference, size_t reference_len, const uint16_t *test, size_t test_len,
                                    uint32_t ref_depth, uint32_t test_depth, uint32_t width, uint32_t height, uint32_t what,
                                    uint32_t block, uint32_t *map, size_t map_len, const uint32_t *thresholds_q20,
                                    uint32_t n_thresholds, uint64_t *over);
/* A pure host function, no GPU needed, beside ce_ciede2000_pixels: the four values of n pixels, out[i * 4 + what] - the same
 * pixel text as the kernel's, compiled for the host; out[i * 4] is ce_ciede2000_pixels' q.  CE_ERR_INVALID_ARG for a null
 * pointer or a depth that is none of 8, 10, 12 and 16. */
int ce_ciede2000_pixel_terms(const uint16_t *ref_rgb, uint32_t ref_depth, const uint16_t *test_rgb, uint32_t test_depth, size_t n,
                             uint32_t *out);

/* ---- a decoder's Y'CbCr planes scored as planes: PSNR, SSIM and MS-SSIM per plane -----------------------
 * What codec test conditions (AOM, JVET, JPEG) tabulate: PSNR-Y, PSNR-Cb, PSNR-Cr on the planes the decoder wrote, each at its
 * own resolution - no chroma upsampling, no colour matrix, no RGB clamp - with the 6:1:1 weighted and the overall PSNR, and
 * SSIM / MS-SSIM per plane.  One call on the context, no batch.  Every value the device returns is an exact integer.
 * Images.  ce_yuv_image as the ingest takes it (above), with the ingest's own checks.  Every image of a call has the call's width
 *   x height and one subsampling and one depth d in {8, 10, 12}; layout, pitch, msb_aligned and memory are per image (an I420
 *   file on the host against a decoder's NV12 / P010 surface on the device).  matrix, range and upsample are validated and not
 *   applied; the two sides of a pair must agree in matrix and range, since their code values would not mean the same otherwise.
 * Planes.  p = 0, 1, 2 = Y, Cb, Cr; 4:0:0 has plane 0 only (n_planes = 1).  Plane 0 is w x h; planes 1 and 2 are cw x ch, cw =
 *   ceil(w / 2) for 4:2:0 and 4:2:2 (else w), ch = ceil(h / 2) for 4:2:0 (else h).  In a semiplanar image Cb and Cr are the even
 *   and odd samples of plane[1].
 * Samples.  min(v >> shift, L), L = 2^d - 1, shift = 16 - d for MSB-aligned samples and 0 otherwise, as the ingest reads them.
 * PSNR.  sse[p] = the sum over plane p's samples of (x - y)^2, x the reference's sample and y the test's, unsigned 64-bit;
 *   n[p] = the plane's sample count.  psnr[p]: mse = (double) sse[p] / (double) n[p]; +INFINITY when mse == 0, otherwise
 *   10.0 * log10(L * L / mse) with L * L formed in f64.  psnr_weighted = ((6.0 * psnr[0] + psnr[1]) + psnr[2]) / 8.0 (the 6:1:1
 *   figure of the HEVC / VVC literature).  psnr_overall = the same expression as psnr[p] on sse[0] + sse[1] + sse[2] and n[0] +
 *   n[1] + n[2] (aomenc's "overall").  4:0:0: the chroma integers are 0, the chroma doubles and psnr_weighted NaN, psnr_overall
 *   luma's.
 * SSIM / MS-SSIM.  The definition of ce_batch_msssim above, unchanged - the window literals, the filter first down the columns
 *   and then along the rows, separately rounded f64 operations, C1 and C2 from L, qs and qc = rint(. * 2^32) summed as int64,
 *   the padded 2 x 2 pooling, the finishing with wt - applied to each plane at its own size as it is applied there to a channel;
 *   planes are not averaged.  levels: 0 (PSNR only), 1 (SSIM) or 5 (MS-SSIM); luma must admit `levels` by ce_msssim_levels' rule.
 *   A chroma plane runs n_levels[p] levels: `levels` if the plane admits them by that rule, else 1 if levels >= 1 and
 *   min(cw, ch) >= 11, else 0.  ssim_q[p][l], cs_q[p][l] and n_pos[p][l] = (h_l - 10) * (w_l - 10) are level l of plane p;
 *   ssim[p] = ((double) ssim_q[p][0] / 4294967296.0) / n_pos[p][0]; ms_ssim[p] as ms_ssim_rgb[c] there, NaN unless
 *   n_levels[p] == 5.  Of levels that did not run the integers are 0 and the doubles NaN.
 * tests/plane_fidelity_restatement.py restates this in numpy; the device equals it on every integer.
 * Not part of this: ce_ref_* handles, ce_eval_batch, the session and the report wire formats, 16-bit planes, chroma sitings
 * (no sample is moved, so siting does not enter), and plane-domain Butteraugli / SSIMULACRA2 / DSSIM. */
typedef struct ce_plane_scores {
    uint64_t sse[3];
    uint64_t n[3];
    double psnr[3];
    double psnr_weighted;
    double psnr_overall;
    double ssim[3];
    double ms_ssim[3];
    int64_t ssim_q[3][5];   /* [plane][level] */
    int64_t cs_q[3][5];
    uint64_t n_pos[3][5];
    uint32_t n_levels[3];
    uint32_t n_planes;
} ce_plane_scores;          /* 512 bytes */
/* Scores n_pairs tests, tests[i] against refs[pair_ref[i]] - or against refs[i] with pair_ref NULL, which needs n_refs ==
 * n_pairs - into out[0 .. n_pairs).  Runs on the context's stream and blocks until the scores are on the host; touches no
 * batch, and a batch launch that is still to be collected is unaffected.  CE_MEM_HOST planes are copied row by row, without
 * their pitch padding, through page-locked staging into a grow-only scratch buffer of the context and are consumed on return.
 * CE_MEM_DEVICE planes are read in place by the kernels, on the context's device, and no full-resolution copy of them is made:
 * the caller must have finished writing them before the call and may reuse them when it returns.  The pyramid of levels 1 - 4,
 * the plane table and the result integers are grow-only scratch of the context too, freed with it and outside
 * ce_estimate_batch_bytes.  A reference that several pairs name is pooled once per call.
 * CE_ERR_INVALID_ARG, with the reason in ce_last_error and the context still usable: a null pointer; n_pairs or n_refs of 0;
 * pair_ref[i] >= n_refs; NULL pair_ref with n_refs != n_pairs; levels outside {0, 1, 5}; a luma plane too small for `levels`;
 * width or height of 0; images that disagree in subsampling or depth; a pair that disagrees in matrix or range; and whatever
 * the ingest refuses of an image (a missing plane of the layout, an unknown enum, a depth outside {8, 10, 12}, a pitch under
 * the row's bytes, a u16 plane pointer or pitch that is not 2-byte aligned, msb_aligned with depth 8, a colour table).  A
 * scratch allocation that fails returns CE_ERR_BACKEND and leaves the context usable. */
int ce_yuv_plane_fidelity(ce_ctx *ctx, uint32_t width, uint32_t height, const ce_yuv_image *refs, uint32_t n_refs,
                          const ce_yuv_image *tests, uint32_t n_pairs, const uint32_t *pair_ref, uint32_t levels,
                          ce_plane_scores *out);

/* ---- PSNR-HVS and PSNR-HVS-M of a decoder's Y'CbCr planes -------------------------------------------------
 * The DCT-domain, CSF-weighted PSNR of Egiazarian et al. (PSNR-HVS) and its contrast-masked form of Ponomarenko et al.
 * (PSNR-HVS-M), per plane, on the planes as the decoder wrote them: the fifth figure codec dashboards tabulate beside PSNR, SSIM,
 * MS-SSIM (above) and CIEDE2000.  This text and its numpy restatement, tests/plane_hvs_restatement.py, are the contract - not
 * the output of any tool: the device equals the restatement on every integer.  Every f64 operation named below is one
 * separately rounded IEEE operation (no contraction, no libm on the device); sqrt and division are correctly rounded.
 * Inputs.  The images, planes p = 0, 1, 2, plane sizes and samples min(v >> shift, L), L = 2^d - 1, d in {8, 10, 12}, of
 *   ce_yuv_plane_fidelity above, unchanged.  One `step` in [1, 8] a call: 8 is Ponomarenko's non-overlapping blocks, 7 the
 *   stride of Daala's and libaom's tools.  The blocks of a pw x ph plane are the 8 x 8 windows at (x, y) = (i step, j step) with
 *   x + 8 <= pw and y + 8 <= ph: n_blocks[p] = ((pw - 8) / step + 1) * ((ph - 8) / step + 1), or 0 if pw < 8 or ph < 8.  Luma
 *   must have a block.  A chroma plane with none has integers 0 and doubles NaN.  The same luma tables serve all three planes:
 *   that is this library's choice - Daala's per-plane chroma CSF tables and its mask normalisation are not part of it, so step 7
 *   is not claimed to reproduce Daala's or libaom's figures.
 * Tables.  Q[8][8] = JPEG (ITU-T T.81) Annex K's luminance table K.1 in natural order (16 11 10 16 24 40 51 61 / 12 12 14 19 26
 *   58 60 55 / 14 13 16 24 40 57 69 56 / 14 17 22 29 51 87 80 62 / 18 22 37 56 68 109 103 77 / 24 35 55 64 81 104 113 92 / 49 64
 *   78 87 103 121 120 101 / 72 92 95 98 112 100 103 99).  csf[k][l] = 25.73509 / (double) Q[k][l]; mc[k][l] = 100.0 / (double)
 *   (Q[k][l] * Q[k][l]): the published CSFCof and MaskCof to their printed decimals.
 * DCT.  Orthonormal 8-point DCT-II in the direct form.  g[0] = sqrt(1 / 8) and g[m] = cos(m pi / 16) / 2, m = 1 .. 7, each the
 *   nearest f64 (plane_hvs_kernel.h has them as hex-float literals).  T[0][j] = g[0]; T[k][j] = +-g[m] with a = (2j + 1) k mod
 *   32, a > 16 -> 32 - a, then a > 8 -> sign -, m = 16 - a, else m = a.  out[k] = ((((((T[k][0] x0 + T[k][1] x1) + T[k][2] x2) +
 *   ...) + T[k][7] x7: products separately rounded, sums left to right.  Along the rows of the block first, then down the columns:
 *   D[k][l], k the vertical frequency.
 * Per block and side, z its 64 samples and D its DCT.  m = sum over (k, l) != (0, 0) of (D[k][l] * D[k][l]) * mc[k][l]: per
 *   column l from k = 0 down without the DC term, the eight column sums as ((c0 + c1) + (c2 + c3)) + ((c4 + c5) + (c6 + c7)).
 *   I(z) = N sum z^2 - (sum z)^2 as an exact integer, N the sample count.  pop = 0 if I(block) == 0, else (63.0 * (double)
 *   (I(q00) + I(q01) + I(q10) + I(q11))) / (15.0 * (double) I(block)) over the four 4 x 4 quadrants.  mask = sqrt(m * pop) / 32.0.
 * Per block.  M = max(maskA, maskB).  Per coefficient u = |DA - DB|, t = M / mc[k][l]; um = u at DC, elsewhere 0 if u < t, else
 *   u - t.  q_hvs = rint(((u * csf[k][l]) * (u * csf[k][l])) * 2^(36 - 2d)), q_hvsm the same of um: the unit is 2^-20 of a
 *   squared 8-bit code at every depth.
 * Per pair and plane.  The exact sums of q_hvs and q_hvsm over all coefficients of all blocks, each as two integers: sum =
 *   x_q[p][0] + x_q[p][1] * 2^32, x_q[p][0] < 2^32.  S = (((double) x_q[p][1] * 4294967296.0 + (double) x_q[p][0]) / 2^(36 - 2d))
 *   / (64.0 * n_blocks[p]); the score is +INFINITY if the sum is 0 (the MATLAB tool prints 100000 there), else 10.0 * log10(L *
 *   L / S) with L * L formed in f64.
 * Not part of this: per-block maps, a plane batch kind, ce_ref_* handles and ce_eval_batch, a factorised DCT (another summation
 *   order would be another contract), chroma CSF tables, RGB batches. */
typedef struct ce_plane_hvs_scores {
    uint64_t hvs_q[3][2];   /* [plane][low 32 bits of the sum, the rest] */
    uint64_t hvsm_q[3][2];
    uint64_t n_blocks[3];
    double psnr_hvs[3];
    double psnr_hvsm[3];
    uint32_t n_planes;
    uint32_t step;
} ce_plane_hvs_scores;      /* 176 bytes */
/* Scores n_pairs tests, tests[i] against refs[pair_ref[i]] - or against refs[i] with pair_ref NULL, which needs n_refs ==
 * n_pairs - into out[0 .. n_pairs), with ce_yuv_plane_fidelity's semantics: on the context's stream, blocking until the scores
 * are on the host; no batch is touched and a batch launch that is still to be collected is unaffected; CE_MEM_HOST planes go
 * through the same page-locked staging and grow-only scratch and are consumed on return; CE_MEM_DEVICE planes are read in
 * place.  One launch covers every plane of up to 21845 pairs.
 * CE_ERR_INVALID_ARG, with the reason in ce_last_error and the context still usable: everything ce_yuv_plane_fidelity refuses
 * of the pointers, the counts, the pair table and the images; step outside [1, 8]; a luma plane under 8 x 8. */
int ce_yuv_plane_hvs(ce_ctx *ctx, uint32_t width, uint32_t height, const ce_yuv_image *refs, uint32_t n_refs,
                     const ce_yuv_image *tests, uint32_t n_pairs, const uint32_t *pair_ref, uint32_t step,
                     ce_plane_hvs_scores *out);

/* ---- pixel-domain VIF (VIFp) of a decoder's Y'CbCr planes ---------------------------------------------------
 * Sheikh & Bovik's visual information fidelity in the pixel domain (vifp_mscale), per plane, on the planes as the decoder wrote
 * them: the "VIF" of learned-codec papers and of the JPEG AI common test conditions; its per-scale ratios are the four VIF
 * features a VMAF model reads.  This text and its numpy restatement, tests/plane_vif_restatement.py, are the contract - not the
 * output of any tool: the device equals the restatement on every integer.  Every f64 operation named below is one separately
 * rounded IEEE operation (no contraction, no libm on the device); division is correctly rounded.
 * Inputs.  The images, planes p = 0, 1, 2, plane sizes and samples min(v >> shift, L), L = 2^d - 1, d in {8, 10, 12}, of
 *   ce_yuv_plane_fidelity above, unchanged.  A sample enters as x = (double) v * 2^(8 - d), which is exact: the constants 2.0
 *   and 1e-10 below keep their 8-bit meaning at every depth.
 * Windows.  Scale s = 1 .. 4 has N_s = 17, 9, 5, 3 taps: g_s[i] = exp(-(i - c)^2 / (2 sd^2)) over their sum, c = (N_s - 1) / 2,
 *   sd = N_s / 5, the f64 numbers numpy gives, literals in the library (ce_vif_window).
 * Filter F_s(p).  "Valid" filtering, first down the columns and then along the rows, each pass ((g[0] p0 + g[1] p1) + g[2] p2)
 *   + ...: products separately rounded, sums left to right.  A w x h plane gives (w - N_s + 1) x (h - N_s + 1).
 * Pyramid.  Scale 1 is the plane.  For s >= 2 both sides become F_s(previous)[0::2, 0::2] - the outputs at even rows and even
 *   columns - so w_s = (w_(s-1) - N_s + 2) / 2 in integers, h_s alike; the values stay f64.  A plane runs all four scales iff
 *   pw >= 41 and ph >= 41, the smallest size that leaves one position at scale 4.  Luma must run; a chroma plane that does not
 *   has integers 0, doubles NaN and ran[p] = 0.
 * Per scale and position, X the reference and Y the test at scale s: mu1 = F(X), mu2 = F(Y), s1 = F(X * X) - mu1 * mu1, s2 =
 *   F(Y * Y) - mu2 * mu2, s12 = F(X * Y) - mu1 * mu2, the products X * X, Y * Y, X * Y formed per sample before filtering.
 *   Then in this order: (1) s1 < 0 -> s1 = 0; s2 < 0 -> s2 = 0.  (2) g = s12 / (s1 + 1e-10); sv = s2 - g * s12.  (3) where
 *   s1 < 1e-10: g = 0, sv = s2, s1 = 0.  (4) where s2 < 1e-10: g = 0, sv = 0.  (5) where g < 0: sv = s2, g = 0.  (6) where
 *   sv <= 1e-10: sv = 1e-10.  (7) a = 1.0 + ((g * g) * s1) / (sv + 2.0); b = 1.0 + s1 / 2.0.
 * Logarithm.  ln_fixed(x) for a normal x >= 1: the exponent e and the mantissa m in [1, 2) split from the bits; m >=
 *   1.4142135623730951 -> m = m * 0.5, e = e + 1; t = (m - 1.0) / (m + 1.0); t2 = t * t; p = 1.0 / 21.0, then p = p * t2 + 1.0 /
 *   k for k = 19, 17, ... 3, 1 (the quotients of literals correctly rounded); ln_fixed = (2.0 * t) * p + (double) e *
 *   0.6931471805599453.  qa = (uint64) rint(ln_fixed(a) * 16777216.0), qb the same of b: the unit is 2^-24 nat, each q is
 *   under 2^28.
 * Per pair, plane and scale.  num_q[p][s-1] = sum qa, den_q[p][s-1] = sum qb, n_pos[p][s-1] = (w_s - N_s + 1) * (h_s - N_s +
 *   1): exact unsigned 64-bit integers, whatever the grid.
 * Finishing, on the host.  vif_scale[p][s-1] = (double) num_q / (double) den_q; vifp[p] the same of the sums over the four
 *   scales; a denominator of 0 (a reference with nothing to lose) gives 1.0 - libvmaf's convention, here this library's
 *   choice.  Planes are not averaged.
 * Not part of this: wavelet-domain VIF, VMAF's integer VIF and its model, per-position maps, RGB batches, ce_ref_* handles and
 *   ce_eval_batch, f32 pyramids (another rounding would be another contract). */
typedef struct ce_plane_vif_scores {
    uint64_t num_q[3][4];   /* [plane][scale - 1] */
    uint64_t den_q[3][4];
    uint64_t n_pos[3][4];
    double vif_scale[3][4];
    double vifp[3];
    uint32_t ran[3];        /* 1: the plane ran its four scales */
    uint32_t n_planes;
} ce_plane_vif_scores;      /* 424 bytes */
/* Scores n_pairs tests, tests[i] against refs[pair_ref[i]] - or against refs[i] with pair_ref NULL, which needs n_refs ==
 * n_pairs - into out[0 .. n_pairs), with ce_yuv_plane_hvs's semantics: on the context's stream, blocking until the scores are
 * on the host; no batch is touched and a batch launch that is still to be collected is unaffected; CE_MEM_HOST planes go
 * through the same page-locked staging and grow-only scratch and are consumed on return; CE_MEM_DEVICE planes are read in
 * place.  The f64 pyramid of scales 2 - 4 and the result integers are grow-only scratch of the context too, freed with it and
 * outside ce_estimate_batch_bytes; a scratch allocation that fails returns CE_ERR_BACKEND and leaves the context usable.  A
 * reference that several pairs name is reduced once per call.
 * CE_ERR_INVALID_ARG, with the reason in ce_last_error and the context still usable: everything ce_yuv_plane_fidelity refuses
 * of the pointers, the counts, the pair table and the images; a luma plane under 41 x 41. */
int ce_yuv_plane_vif(ce_ctx *ctx, uint32_t width, uint32_t height, const ce_yuv_image *refs, uint32_t n_refs,
                     const ce_yuv_image *tests, uint32_t n_pairs, const uint32_t *pair_ref, ce_plane_vif_scores *out);
/* The N_s literals of scale 1 .. 4's window (17, 9, 5, 3) into out[0 .. N_s); a pure host function.  CE_ERR_INVALID_ARG for a
 * null pointer or another scale. */
int ce_vif_window(uint32_t scale, double *out);

/* ---- GMSD of a decoder's Y'CbCr planes -----------------------------------------------------------------------
 * Gradient magnitude similarity deviation (Xue, Zhang, Mou and Bovik 2014), per plane, on the planes as the decoder wrote them,
 * with its mean (GMSM) beside it.  The paper's MATLAB code is restated here as remembered; nothing available while this was
 * written could confirm it against that code.  This text and its numpy restatement, tests/plane_gmsd_restatement.py, are the
 * contract - not the output of any tool: the device equals the restatement on every integer.  Every f64 operation named below is
 * one separately rounded IEEE operation (no contraction, no libm on the device); sqrt and division are correctly rounded.
 * Inputs.  The images, planes p = 0, 1, 2, plane sizes pw x ph and samples v = min(raw >> shift, L), L = 2^d - 1, d in {8, 10,
 *   12}, of ce_yuv_plane_fidelity above, unchanged.  Every plane of the subsampling is scored; a plane of any size >= 1 x 1
 *   runs.  Planes are not averaged.
 * Downsample.  W2 = (pw + 1) / 2, H2 = (ph + 1) / 2 in integers.  S[j][i] = v[2j][2i] + v[2j][2i+1] + v[2j+1][2i] + v[2j+1][2i+1],
 *   a sample outside the plane counting 0: conv2(Y, ones(2) / 4, 'same') taken at 1:2:end, times 4, so an odd last row or column
 *   gets the half sum the MATLAB code gives it.  S is an exact integer <= 4 L.
 * Gradients, at each of the n_pos = W2 * H2 positions, S outside the grid counting 0 (conv2(.., 'same')): Gx = (S[j-1][i-1] +
 *   S[j][i-1] + S[j+1][i-1]) - (S[j-1][i+1] + S[j][i+1] + S[j+1][i+1]); Gy its transpose, row j - 1 less row j + 1.  A = Gx * Gx +
 *   Gy * Gy, an exact integer <= 2 (12 L)^2 < 2^33: 144 * 4^(d - 8) times the squared Prewitt (/ 3) gradient magnitude of the
 *   2 x 2 mean of the image scaled to 8 bits.
 * Similarity.  K = 24480 * 4^(d - 8) = 144 * 170 at the depth's scale: the paper's constant keeps its 8-bit meaning.  Per side m
 *   = sqrt((double) A).  Per position num = (2.0 * (m_ref * m_test)) + (double) K; den = (double) (A_ref + A_test + K), the sum
 *   formed in integers and converted once, exactly; g = num / den; q = (uint64) rint(g * 4294967296.0).  1 <= q <= 2^32, q =
 *   2^32 where both sides are flat; 2^32 - q fits a uint32.
 * Per pair and plane, exact integers whatever the grid: sum_q = sum q (< 2^64); sum_q2 = sum q * q as a 128-bit integer, [low
 *   64 bits, high 64 bits]; max_dis = max (2^32 - q); n_pos.
 * Finishing, on the host.  V = n_pos * sum_q2 - sum_q * sum_q as an exact integer (it fits 128 bits since n_pos < 2^32); gmsd =
 *   sqrt((double) V) / ((double) n_pos * 4294967296.0) with (double) V the nearest double; gmsm = (double) sum_q / ((double)
 *   n_pos * 4294967296.0).  The deviation divides by N as the paper's formula does - this library's choice; MATLAB's std2
 *   divides by N - 1, and the integers let a caller form either.
 * Not part of this: per-position maps and cell maxima, RGB batches, ce_ref_* handles and ce_eval_batch, keeping a reference's
 *   A between pairs. */
typedef struct ce_plane_gmsd_scores {
    uint64_t sum_q[3];
    uint64_t sum_q2[3][2];   /* [plane][low 64 bits, high 64 bits] */
    uint64_t n_pos[3];
    double gmsd[3];
    double gmsm[3];
    uint32_t max_dis[3];
    uint32_t n_planes;
} ce_plane_gmsd_scores;      /* 160 bytes */
/* Scores n_pairs tests, tests[i] against refs[pair_ref[i]] - or against refs[i] with pair_ref NULL, which needs n_refs ==
 * n_pairs - into out[0 .. n_pairs), with ce_yuv_plane_hvs's semantics: on the context's stream, blocking until the scores are
 * on the host; no batch is touched and a batch launch that is still to be collected is unaffected; CE_MEM_HOST planes go
 * through the same page-locked staging and grow-only scratch and are consumed on return; CE_MEM_DEVICE planes are read in
 * place.  One launch covers every plane of up to 21845 pairs.  Planes beyond n_planes have integers 0 and doubles NaN.
 * CE_ERR_INVALID_ARG, with a reason that starts "plane gmsd: " in ce_last_error and the context still usable: everything
 * ce_yuv_plane_fidelity refuses of the pointers, the counts, the pair table and the images; a luma plane with W2 * H2 >= 2^32. */
int ce_yuv_plane_gmsd(ce_ctx *ctx, uint32_t width, uint32_t height, const ce_yuv_image *refs, uint32_t n_refs,
                      const ce_yuv_image *tests, uint32_t n_pairs, const uint32_t *pair_ref, ce_plane_gmsd_scores *out);

/* ---- matrix/TRC ICC profiles applied on the device ------------------------------------------------
 * transform_to_srgb (src/metrics/icc.rs:69-103) for the profiles photographs carry - three colorant tags and three tone
 * curves - without a CMS on the host.  ce_lut_* above stays the route for every other profile.
 * Accepted: ICC v2 and v4; `acsp`; data colour space `RGB `, PCS `XYZ `; class `mntr`, `scnr` or `spac`; rXYZ / gXYZ / bXYZ
 * of type `XYZ `; rTRC / gTRC / bTRC of type `curv` or `para`.  A profile with an A2B0, A2B1 or A2B2 tag is LUT-based and not
 * accepted (a CMS would use the LUT).  PCS white, wtpt and chad are not read: the colorants are D50-adapted by the format's
 * own rule.  Every length, offset and count is checked against the buffer before use; a profile is at most
 * CE_ICC_MAX_PROFILE_BYTES long (its header's size field must lie within the buffer) and a curv at most
 * CE_ICC_MAX_CURVE_POINTS samples.
 * Curves, in f64 at e = v / maxv, the result clipped to [0, 1] (NaN -> 0) and rounded once to f32:
 *   curv n = 0: e.  n = 1: e^g, g the u8Fixed8 number.  n >= 2: samples s = u16 / 65535 interpolated at p = e * (n - 1):
 *     i = min(floor(p), n - 2), s[i] + (s[i + 1] - s[i]) * (p - i).
 *   para (parameters s15Fixed16 / 65536; a negative base of the power is taken as 0):
 *     0: X^g.  1: (aX + b)^g for X >= -b / a, else 0.  2: (aX + b)^g + c for X >= -b / a, else c.  A profile whose type 1 or 2
 *     curve has a = 0 has no breakpoint and is malformed.
 *     3: (aX + b)^g for X >= d, else cX.  4: (aX + b)^g + e for X >= d, else cX + f.
 * Matrix: M = inv(A) * P in f64 rounded once to f32, row-major; P has the profile's colorants as columns (the s15Fixed16
 * integers / 65536, exactly), A those of the canonical sRGB profile - rXYZ (0x6FA2, 0x38F5, 0x0390), gXYZ (0x6299, 0xB785,
 * 0x18DA), bXYZ (0x24A0, 0x0F84, 0xB6CF) - inverted by ce_colour_matrix's adjugate / determinant sequence and multiplied as
 * (ai0 * p0 + ai1 * p1) + ai2 * p2.  A profile whose nine integers are A's has M = I exactly and is not multiplied.
 * Definition, per pixel of a CE_PIXEL_RGB8 / RGBA8 / RGB16 / RGBA16 image (alpha dropped) of source depth d in {8, 10, 12,
 * 16}, maxv = 2^d - 1:
 *   1. t_c = table_c[min(v_c, maxv)], one table per channel (ce_icc_build_tables).
 *   2. unless M = I: o_i = (M[i][0] * t_r + M[i][1] * t_g) + M[i][2] * t_b in f32, each product and sum rounded separately.
 *   3. the clamp of a linear image (NaN -> 0, [-CE_LINEAR_MAX, CE_LINEAR_MAX]).  This is the value a linear batch stores.
 *   4. an RGB8 batch (D = 8) or a side of depth D of a deep batch stores, for each of the three values x,
 *        code = #{ k in 1 .. 2^D - 1 : x >= T[k] },  T[k] = f32(srgb_eotf_f64((k - 0.5) / (2^D - 1)))
 *      with srgb_eotf_f64 the curve of ce_srgb_table's rule 0: a search in a strictly increasing table (ce_srgb_encode_thresholds),
 *      NaN -> 0, out-of-gamut values clip.  The integer routes are the encode of the linear route and add no other arithmetic.
 * tests/icc_restatement.py restates this in numpy; the device equals it bit for bit.
 * Not part of this: LUT-based profiles (mAB, lut8, lut16: ce_icc_lut_create below takes those), Gray and CMYK profiles,
 * rendering intents, black-point compensation, alpha compositing with a profile, ce_ref_* handles and the pooled
 * ce_eval_batch.  (Y'CbCr planes with a profile: ce_batch_set_*_yuv_icc, next to the other plane routes above.) */
#define CE_ICC_MAX_PROFILE_BYTES 4194304u
#define CE_ICC_MAX_CURVE_POINTS 65536u
enum { CE_ICC_SUPPORTED = 0, CE_ICC_LUT_BASED = 1, CE_ICC_NOT_RGB_XYZ = 2, CE_ICC_MALFORMED = 3 };
enum { CE_ICC_CURVE_CURV = 0, CE_ICC_CURVE_PARA = 1, CE_ICC_CURVE_TABLE8 = 2 /* ce_icc_lut_describe only: count u8 samples at offset (mft1) */ };
typedef struct ce_icc_curve {
    int type;          /* CE_ICC_CURVE_CURV or CE_ICC_CURVE_PARA */
    uint32_t count;    /* curv: the number of samples (0: identity, 1: a gamma); para: the function type 0 .. 4 */
    int32_t params[7]; /* para: g a b c d e f as s15Fixed16 (those the type has; the rest 0); curv n = 1: params[0] = u8Fixed8 */
    uint32_t offset;   /* curv n >= 2: where the first u16 sample lies in the profile */
} ce_icc_curve;
typedef struct ce_icc_description {
    int kind;               /* CE_ICC_SUPPORTED, _LUT_BASED, _NOT_RGB_XYZ or _MALFORMED; the fields below are filled as far as parsing got */
    uint32_t version;       /* header bytes 8 .. 11, e.g. 0x04300000 */
    uint32_t profile_class; /* the signature as a big-endian number: 'mntr' = 0x6d6e7472 */
    int32_t colorants[9];   /* P row-major as s15Fixed16: rows X Y Z, columns r g b */
    ce_icc_curve curves[3]; /* rTRC, gTRC, bTRC */
    char reason[96];        /* kind != 0: why, NUL-terminated */
} ce_icc_description;
/* Pure host functions.  ce_icc_describe returns CE_OK whenever `out` is filled, whatever the kind.  The builders return
 * CE_ERR_INVALID_ARG for a profile whose kind != 0 (ce_icc_describe has the reason), a depth outside {8, 10, 12, 16} or a
 * wrong n.  ce_icc_build_tables: out = [3][2^depth] floats, n = 3 << depth.  ce_srgb_encode_thresholds: out[k - 1] = T[k],
 * n = 2^depth - 1. */
int ce_icc_describe(const uint8_t *bytes, size_t len, ce_icc_description *out);
int ce_icc_build_matrix(const uint8_t *bytes, size_t len, float out[9]);
int ce_icc_build_tables(const uint8_t *bytes, size_t len, uint32_t depth, float *out, size_t n);
int ce_srgb_encode_thresholds(uint32_t depth, float *out, size_t n);
/* A parsed profile on a context's device, with its tone tables of all four source depths (0.85 MB of device memory), built
 * by ce_icc_create; the handle does not change afterwards.  It belongs to its context and follows the context's threading
 * rule: one in-flight call per context, the calls that take the handle included (the thresholds of a slot depth are made on
 * the context by the first ingest that needs them).  CE_ERR_INVALID_ARG with the reason in ce_last_error for a profile whose
 * kind != 0.  Destroy it after the last batch that was given it has been collected. */
typedef struct ce_icc ce_icc;
int ce_icc_create(ce_ctx *ctx, const uint8_t *bytes, size_t len, ce_icc **out);
void ce_icc_destroy(ce_icc *icc);
/* One image of the batch's shape into a reference / test slot of a linear, an RGB8 or a deep batch, with the staging, stream
 * and ordering of ce_batch_set_*_cicp; the pixels are consumed on return.  `depth` is the source's.  An RGB8 batch takes
 * CE_PIXEL_RGB8 / RGBA8 only; a deep side is written at its own depth from any of the four formats.  CE_ERR_INVALID_ARG, with
 * the reason in ce_last_error and the batch still usable, for a null pointer, a profile of another device, another format, a
 * depth outside {8, 10, 12, 16}, an 8-bit format with depth != 8, a 16-bit format on an RGB8 batch; CE_ERR_BAD_LENGTH for a
 * wrong len. */
int ce_batch_set_reference_icc(ce_batch *b, uint32_t ref_index, const void *pixels, size_t len, int format, uint32_t depth,
                               const ce_icc *icc);
int ce_batch_set_test_icc(ce_batch *b, uint32_t pair_index, uint32_t ref_index, const void *pixels, size_t len, int format,
                          uint32_t depth, const ce_icc *icc);
/* One image of w x h to host memory: packed float RGB (out_len = w * h * 3 floats), packed sRGB8 (out_len = w * h * 3
 * bytes) or packed u16 sRGB of depth_out in {8, 10, 12, 16} (out_len = w * h * 3 samples).  Errors as above, and
 * CE_ERR_BAD_LENGTH for a wrong out_len. */
int ce_icc_to_linear(ce_ctx *ctx, const void *pixels, size_t len, int format, uint32_t depth, const ce_icc *icc, uint32_t w,
                     uint32_t h, float *out, size_t out_len);
int ce_icc_to_srgb8(ce_ctx *ctx, const void *pixels, size_t len, int format, uint32_t depth, const ce_icc *icc, uint32_t w,
                    uint32_t h, uint8_t *out, size_t out_len);
int ce_icc_to_srgb16(ce_ctx *ctx, const void *pixels, size_t len, int format, uint32_t depth, const ce_icc *icc, uint32_t w,
                     uint32_t h, uint32_t depth_out, uint16_t *out, size_t out_len);

/* ---- LUT-based ICC profiles applied on the device ----------------------------------------------------
 * transform_to_srgb (src/metrics/icc.rs:69-103) for the profiles whose transform is a table: an A2B tag of type `mAB `
 * (lutAToBType), `mft2` (lut16) or `mft1` (lut8) - the jpegli XYB profile is one - evaluated from the profile itself, with
 * no CMS on the host and no 2^24-entry table.  ce_icc_describe / ce_icc_create above keep answering CE_ICC_LUT_BASED for them.
 * Accepted: ICC v2 and v4; `acsp`; data colour space `RGB `; PCS `XYZ ` or `Lab `; class `mntr`, `scnr` or `spac`; the tag
 * A2B0, or with intent 1 / 2 the tag A2B1 / A2B2 where the profile has it and A2B0 otherwise; 3 input and 3 output channels.
 *   mAB : B curves alone; M curves, the 3 x 4 matrix and B; A curves, the CLUT and B; or A, CLUT, M, matrix and B - what its
 *         five offsets name must be one of these four, each curve sequence three `curv` / `para` elements padded to 4 bytes,
 *         the CLUT of 1 or 2 bytes per sample with its own grid size per axis.
 *   mft2, mft1: input tables (2 .. 4096 u16 entries; 256 u8 entries), the CLUT, output tables.  Their 3 x 3 matrix is read
 *         and not applied: the format applies it to XYZ input only.  mft1 with PCS XYZ is refused: the format has no such.
 * Every grid size lies in [2, 255] and the nodes number at most CE_ICC_MAX_CLUT_NODES; curves follow the rules of the
 * matrix/TRC section (a = 0 in a type 1 or 2 para is malformed; a curv has at most CE_ICC_MAX_CURVE_POINTS samples); the
 * profile is at most CE_ICC_MAX_PROFILE_BYTES long.  Every offset, count and size is checked in size_t against the tag, and
 * the tag against the profile, before anything is read.
 * Definition, per pixel of a CE_PIXEL_RGB8 / RGBA8 / RGB16 / RGBA16 image (alpha dropped) of source depth d, maxv = 2^d - 1.
 * f32 unless stated, every product and sum rounded separately (no contraction), in the order written:
 *   1. a_c = table_c[min(v_c, maxv)] (ce_icc_lut_build_input_tables): the A curve (mAB) or the input table (mft*, its samples
 *      u16 / 65535 or u8 / 255 interpolated by the `curv n >= 2` rule above) in f64 at v / maxv, clipped to [0, 1], rounded once
 *      to f32; v / maxv itself where the stage is absent.
 *   2. With a CLUT of grid (g0, g1, g2), nodes N[i0][i1][i2][k] = f32(u16 / 65535) or f32(u8 / 255), the first channel's index
 *      slowest: per axis p = a * f32(g - 1), i = min(floor(p), g - 2), f = p - f32(i), so the last node is reached with f = 1.
 *      With cxyz the node at (i0 + x, i1 + y, i2 + z) and (fx, fy, fz) the three fractions, per output channel:
 *      CE_ICC_CLUT_TRILINEAR: c00 = c000 + (c001 - c000) * fz, c01 = c010 + (c011 - c010) * fz, c10 and c11 likewise from
 *        c100, c101 and c110, c111; c0 = c00 + (c01 - c00) * fy, c1 = c10 + (c11 - c10) * fy; v = c0 + (c1 - c0) * fx.
 *      CE_ICC_CLUT_TETRAHEDRAL: v = ((c000 + (ca - c000) * hi) + (cb - ca) * mid) + (c111 - cb) * lo, where
 *        fx >= fy: fy >= fz: (hi, mid, lo) = (fx, fy, fz), ca = c100, cb = c110;  else fx >= fz: (fx, fz, fy), c100, c101;
 *                  else (fz, fx, fy), c001, c101;
 *        fx <  fy: fx >= fz: (fy, fx, fz), c010, c110;  else fy >= fz: (fy, fz, fx), c010, c011;  else (fz, fy, fx), c001, c011.
 *        A tie therefore goes to the earlier axis: fx = fy = fz walks c100, c110.  Where an output channel depends on one axis
 *        alone both interpolations give c000 + (c1 - c000) * f of that axis, bit for bit; on an affine CLUT they agree
 *        within rounding only.
 *      Without a CLUT v = a.
 *   3. mAB: the M curves, the matrix, the B curves; mft*: the output tables (as B).  A curve on x:
 *        curv n = 0: x, unchanged and unclipped.  Every other curve first clips x to [0, 1] (NaN -> 0).
 *        curv n >= 2, output table: samples s = f32(u16 / 65535) (f32(u8 / 255)), p = x * f32(n - 1), i = min(floor(p), n - 2),
 *          s[i] + (s[i + 1] - s[i]) * (p - f32(i)).
 *        curv n = 1, para: the formulas above in f64 on X = (double)x, the result clipped to [0, 1] (NaN -> 0) and rounded once
 *          to f32.  The power B^g: B <= 0 or B < 2^-1022 is taken as 0, and 0^g is +inf for g < 0, 1 for g = 0, else 0.  With E
 *          the unbiased binary exponent of B, |g| * (|E| + 1) > 1000 is not evaluated: the power is +inf where g * (E + 0.5) > 0
 *          and 0 otherwise (exact to the clip for |g| <= 500; beyond that a base in [1/2, 2) is misjudged - no profile known
 *          to us has such a curve).  Otherwise it is the fixed sequence of IEEE f64 operations the HLG and gain-map ingests
 *          use (csrc/hlg_pixel.h: hlg_pow; tests/hlg_restatement.py), the same on the device and in the restatement.  Measured
 *          against the host libm's pow over bases in [2^-40, 2] and twelve exponents from 1/3 to 3 (1e6 seeded bases and the
 *          curves' own breakpoints): 2.2e-14 relative at most; bounded by 2.4e-14 (|g ln B| <= 83.2 there, one rounding of
 *          which is 1.85e-14 of the result, on top of hlg_pow's own 5e-15).
 *        matrix: m = f32(s15Fixed16 / 65536), y_i = ((m[i][0] * x0 + m[i][1] * x1) + m[i][2] * x2) + m[i][3].
 *   4. PCS decode.  XYZ: X = v * f32(1 + 32767 / 32768).  Lab in mAB and mft1: L = 100 * v, a = 255 * v - 128, b likewise.
 *      Lab in mft2, in a v2 and in a v4 profile alike (the legacy 16-bit encoding, which is what lcms2 decodes in both):
 *      L = v * f32(65535 / 652.8), a = v * f32(65535 / 256) - 128.  Lab -> XYZ: fy = (L + 16) / 116, fx = fy + a / 500,
 *      fz = fy - b / 200; t(f) = (f * f) * f for f > f32(6 / 29), else (f - f32(4 / 29)) * f32(108 / 841); X = f32(0xF6D6 / 65536)
 *      * t(fx), Y = t(fy), Z = f32(0xD32D / 65536) * t(fz).
 *   5. o_i = (M[i][0] * X + M[i][1] * Y) + M[i][2] * Z with M = f32(inv(A)), A and the inversion as in the matrix/TRC section
 *      (ce_icc_lut_build_pcs_matrix).
 *   6. the clamp of a linear image: the value a linear batch stores.  An RGB8 batch or a deep side stores its code by step 4 of
 *      the matrix/TRC definition, unchanged.
 * tests/icc_lut_restatement.py restates this in numpy; the device equals it bit for bit.
 * Not part of this: Gray and CMYK profiles, mBA / B2A tags, multiProcessElements (D2B*), black-point compensation, alpha
 * with a profile in one kernel, ce_ref_* handles and the pooled ce_eval_batch.  (Y'CbCr planes with a profile of either
 * flavour: ce_batch_set_*_yuv_icc above.) */
#define CE_ICC_MAX_CLUT_NODES 274625u /* 65^3: 4.4 MB on the device, a node being 16 bytes there */
enum { CE_ICC_LUT_SUPPORTED = 0, CE_ICC_LUT_NOT_LUT = 1, CE_ICC_LUT_UNSUPPORTED = 2, CE_ICC_LUT_MALFORMED = 3 };
enum { CE_ICC_CLUT_TRILINEAR = 0, CE_ICC_CLUT_TETRAHEDRAL = 1 };
enum { CE_ICC_STAGE_A = 1, CE_ICC_STAGE_CLUT = 2, CE_ICC_STAGE_M = 4, CE_ICC_STAGE_MATRIX = 8, CE_ICC_STAGE_B = 16 };
typedef struct ce_icc_lut_description {
    int kind;               /* CE_ICC_LUT_SUPPORTED, _NOT_LUT (no A2B tag), _UNSUPPORTED (not RGB, a PCS other than XYZ / Lab, a
                               class or a channel count not taken) or _MALFORMED; the fields below as far as parsing got */
    uint32_t version;       /* header bytes 8 .. 11 */
    uint32_t profile_class; /* signatures as big-endian numbers */
    uint32_t pcs;           /* 'XYZ ' or 'Lab ' */
    uint32_t tag;           /* the tag used: 'A2B0', 'A2B1' or 'A2B2' */
    uint32_t tag_type;      /* 'mAB ', 'mft2' or 'mft1' */
    uint32_t tag_offset, tag_size;
    uint32_t stages;        /* CE_ICC_STAGE_* present; mft*: A (input tables), CLUT and B (output tables) */
    uint32_t grid[3];       /* nodes per axis, the first input channel's first */
    uint32_t precision;     /* bytes per CLUT sample: 1 or 2 */
    uint32_t clut_offset;   /* where the first sample lies in the profile */
    int32_t matrix[12];     /* mAB: e1 .. e12 as s15Fixed16 (3 x 3 row-major, then the three offsets); mft*: e1 .. e9, not applied */
    ce_icc_curve a[3];      /* A curves / input tables (mft2: CURV with count entries at offset; mft1: TABLE8) */
    ce_icc_curve m[3];      /* M curves */
    ce_icc_curve b[3];      /* B curves / output tables */
    char reason[96];        /* kind != 0: why, NUL-terminated */
} ce_icc_lut_description;
/* A post-CLUT curve as the kernel takes it (ce_icc_lut_build_curves) */
enum { CE_ICC_LUT_CURVE_IDENTITY = 0, CE_ICC_LUT_CURVE_SAMPLED = 1, CE_ICC_LUT_CURVE_POWER = 2 };
typedef struct ce_icc_lut_curve {
    int kind;              /* CE_ICC_LUT_CURVE_* */
    uint32_t ftype;        /* POWER: the para function type 0 .. 4 (curv n = 1: 0) */
    uint32_t count;        /* SAMPLED: the number of samples */
    uint32_t first_sample; /* SAMPLED: where they start in the samples array */
    double q[7];           /* POWER: g a b c d e f */
} ce_icc_lut_curve;
/* Pure host functions; `intent` 0, 1 or 2 chooses the tag as above.  ce_icc_lut_describe returns CE_OK whenever `out` is filled
 * (CE_ERR_INVALID_ARG for a null pointer or another intent).  The builders return CE_ERR_INVALID_ARG for a profile whose kind
 * != 0, a bad depth or a wrong n, and give exactly what the kernel is handed:
 *   input_tables: [3][2^depth] floats, n = 3 << depth.
 *   clut: nodes padded to four floats, [g0 * g1 * g2][4] with the fourth 0, n = 4 * the node count; n = 0 and nothing written
 *     for a profile without a CLUT.
 *   matrix: the 12 floats of step 3 (3 x 3 row-major, then the offsets); the identity and 0 without the stage.
 *   curves: out[0 .. 2] the M curves, out[3 .. 5] the B curves / output tables (IDENTITY where the stage is absent); the
 *     samples of SAMPLED curves one after another in `samples`, n_samples floats of room; *needed = the floats they take
 *     (call with samples = NULL, n_samples = 0 to learn it; CE_ERR_BAD_LENGTH when the room is less).
 *   pcs_matrix: the 9 floats of step 5. */
int ce_icc_lut_describe(const uint8_t *bytes, size_t len, int intent, ce_icc_lut_description *out);
int ce_icc_lut_build_input_tables(const uint8_t *bytes, size_t len, int intent, uint32_t depth, float *out, size_t n);
int ce_icc_lut_build_clut(const uint8_t *bytes, size_t len, int intent, float *out, size_t n);
int ce_icc_lut_build_matrix(const uint8_t *bytes, size_t len, int intent, float out[12]);
int ce_icc_lut_build_curves(const uint8_t *bytes, size_t len, int intent, ce_icc_lut_curve out[6], float *samples, size_t n_samples,
                            size_t *needed);
int ce_icc_lut_build_pcs_matrix(float out[9]);
/* The same handle type as ce_icc_create's, for a LUT-based profile: the input tables of all four source depths, the CLUT and
 * the sampled curves on the device, immutable afterwards; `interpolation` is CE_ICC_CLUT_TRILINEAR or _TETRAHEDRAL.  Every call
 * that takes a ce_icc takes this one, with the same staging, stream, ordering, formats, depths and refusals.
 * CE_ERR_INVALID_ARG with the reason in ce_last_error for a profile whose kind != 0, another intent or interpolation. */
int ce_icc_lut_create(ce_ctx *ctx, const uint8_t *bytes, size_t len, int intent, int interpolation, ce_icc **out);

/* ---- alpha in linear light: transparent HDR and wide-gamut images over solid backgrounds ------------
 * Every route into a linear batch above drops alpha, which brings back for transparent images the two faults that the alpha
 * section removed for SDR: colour left under a = 0 is scored, damage to the alpha plane is not.  These calls blend instead,
 * AFTER the pixel has been turned into linear light - the "linear-light blending" that the alpha section leaves out.  There
 * the blend is physically meaningful and does not depend on the transfer the file happened to use: a 0 / 1 edge at half
 * coverage gives 0.5 of the light, not code 128.  (Blending the encoded samples first is ce_composite_rgba* followed by the
 * plain ingest.)
 * Definition, per pixel of a CE_PIXEL_RGBA8 / CE_PIXEL_RGBA16 image of source depth d, m = 2^d - 1, STRAIGHT alpha; every
 * product and sum is a separately rounded f32 operation (no fused multiply-add):
 *   1. v[3] = the pixel of the plain call of the same kind on the three colour samples, its final clamp included: the CICP
 *      definition, the HLG definition, the matrix/TRC or the LUT definition above, unchanged.
 *   2. t = atab[min(a, m)] with atab[k] = float32(k) / float32(m), one correctly rounded f32 division, built on the host per
 *      depth (ce_alpha_table); the device only gathers.  u = 1.0f - t, one f32 subtraction on the device.
 *   3. over background k with linear colour bg[k][3], per channel: o = (t == 1) ? v : (t == 0) ? bg : (v * t) + (bg * u).
 *      The two selects make an opaque pixel equal to the plain ingest on every bit, -0.0 included, and a hidden pixel equal
 *      to the background on every bit.
 *   4. the clamp of a linear image on o: NaN -> 0, then [-CE_LINEAR_MAX, CE_LINEAR_MAX].
 * CE_PIXEL_RGBA_F32 is float RGBA, 16 bytes per pixel, linear light with sRGB primaries; only the *_linear_over calls below
 * accept it (ce_batch_set_*_fmt refuses it).  v = the clamp of a linear image on each colour sample; t = alpha with NaN -> 0,
 * then clamped to [0, 1]; u, the blend and the clamp as above.  With premultiplied != 0 the colour samples already hold
 * colour * coverage and step 3 is o = (u == 0) ? v : v + (bg * u).
 * backgrounds: float [n_bg][3], linear light with sRGB primaries, 1 <= n_bg <= CE_MAX_BACKGROUNDS, every value finite and
 * within +-CE_LINEAR_MAX.  As in the alpha section one upload fills n_bg consecutive slots, slot k over backgrounds[k]; the
 * pixel is read and converted once.  tests/alpha_linear_restatement.py restates this in numpy; the device equals it bit for
 * bit.
 * Not part of this: premultiplied integer formats, gain-map images with alpha, Y'CbCr planes with a separate alpha plane, ICC
 * with alpha into RGB8 / deep slots, patterned backgrounds, device-resident sources, ce_ref_* handles and ce_eval_batch. */
enum {
    CE_PIXEL_RGBA_F32 = 8 /* packed float RGBA, 16 bytes per pixel, linear light: the *_linear_over calls only */
};
/* atab of `depth` bits (8, 10, 12 or 16; n = 2^depth entries).  A pure host function. */
int ce_alpha_table(uint32_t depth, float *out, size_t n);
/* ce_batch_set_*_cicp (the description, its formats with alpha, staging, upload stream and ordering) with ce_batch_set_*_over's
 * slots: reference slots first_ref .. first_ref + n_bg - 1 / test slots first_pair .. first_pair + n_bg - 1, pair
 * first_pair + k bound to reference ref_indices[k]; the pixels are consumed on return.  CE_ERR_INVALID_ARG, with the reason in
 * ce_last_error and the batch still usable, for a batch that is not linear, a null handle or pointer, a format without alpha,
 * every refusal of ce_batch_set_*_cicp, n_bg = 0 or n_bg > CE_MAX_BACKGROUNDS, a background that is not finite or beyond
 * +-CE_LINEAR_MAX, a slot range or a ref_indices entry past the batch; CE_ERR_BAD_LENGTH for a wrong len. */
int ce_batch_set_reference_cicp_over(ce_batch *b, uint32_t first_ref, const void *pixels, size_t len, int format, const ce_colour *c,
                                     uint32_t n_bg, const float *backgrounds);
int ce_batch_set_test_cicp_over(ce_batch *b, uint32_t first_pair, const uint32_t *ref_indices, const void *pixels, size_t len, int format,
                                const ce_colour *c, uint32_t n_bg, const float *backgrounds);
/* the same around ce_batch_set_*_hlg and its refusals */
int ce_batch_set_reference_hlg_over(ce_batch *b, uint32_t first_ref, const void *pixels, size_t len, int format, const ce_hlg *h,
                                    uint32_t n_bg, const float *backgrounds);
int ce_batch_set_test_hlg_over(ce_batch *b, uint32_t first_pair, const uint32_t *ref_indices, const void *pixels, size_t len, int format,
                               const ce_hlg *h, uint32_t n_bg, const float *backgrounds);
/* the same around ce_batch_set_*_icc and its refusals, either flavour of handle; a linear batch only */
int ce_batch_set_reference_icc_over(ce_batch *b, uint32_t first_ref, const void *pixels, size_t len, int format, uint32_t depth,
                                    const ce_icc *icc, uint32_t n_bg, const float *backgrounds);
int ce_batch_set_test_icc_over(ce_batch *b, uint32_t first_pair, const uint32_t *ref_indices, const void *pixels, size_t len, int format,
                               uint32_t depth, const ce_icc *icc, uint32_t n_bg, const float *backgrounds);
/* CE_PIXEL_RGBA_F32 (len = width * height * 16), straight or premultiplied; extends ce_batch_set_*_fmt(CE_PIXEL_RGB_F32) */
int ce_batch_set_reference_linear_over(ce_batch *b, uint32_t first_ref, const void *pixels, size_t len, int format, int premultiplied,
                                       uint32_t n_bg, const float *backgrounds);
int ce_batch_set_test_linear_over(ce_batch *b, uint32_t first_pair, const uint32_t *ref_indices, const void *pixels, size_t len, int format,
                                  int premultiplied, uint32_t n_bg, const float *backgrounds);
/* One image of w x h over one background to packed float RGB in host memory (out_len = w * h * 3 floats): ce_cicp_to_linear,
 * ce_hlg_to_linear, ce_icc_to_linear and the float upload with the blend.  Errors as above. */
int ce_cicp_over_to_linear(ce_ctx *ctx, const void *pixels, size_t len, int format, const ce_colour *c, uint32_t w, uint32_t h,
                           const float bg[3], float *out, size_t out_len);
int ce_hlg_over_to_linear(ce_ctx *ctx, const void *pixels, size_t len, int format, const ce_hlg *hd, uint32_t w, uint32_t h,
                          const float bg[3], float *out, size_t out_len);
int ce_icc_over_to_linear(ce_ctx *ctx, const void *pixels, size_t len, int format, uint32_t depth, const ce_icc *icc, uint32_t w,
                          uint32_t h, const float bg[3], float *out, size_t out_len);
int ce_linear_over(ce_ctx *ctx, const void *pixels, size_t len, int format, int premultiplied, uint32_t w, uint32_t h, const float bg[3],
                   float *out, size_t out_len);

/* ---- tensors: a framework's strided image tensors into slots of a resident batch -------------------
 * A learned codec returns its decoded images as an N x 3 x H x W tensor of float32, float16 or bfloat16 in [0, 1] on the
 * device; a GPU decoder (a framework's JPEG decoder on a device, rocJPEG's RGB outputs) returns 3 x H x W or pitched H x W x 3
 * uint8 there.  These calls read such a tensor through its strides and write the slots in one kernel: nothing crosses the bus
 * for a device tensor, and the rounding from float to the integer grid is the definition below, not whatever the glue did.
 * Channel c in {0, 1, 2} of pixel (y, x) of image n is the element at n * stride_n + c * stride_c + y * stride_y + x * stride_x
 * (strides in ELEMENTS, not bytes): CHW / NCHW (stride_x = 1), HWC / NHWC and channels_last (stride_c = 1, stride_x = 3),
 * RGBA (stride_x = 4; the fourth channel is never read), cropped views and pitched surfaces (stride_y above the row), a gray
 * tensor expanded to three channels (stride_c = 0).
 * Definition, per sample, with m = 2^D - 1 for the slot's depth D (8 on an RGB8 batch, that side's depth on a deep batch):
 *   a float dtype into an integer slot:
 *     v = f32(x), an exact widening (bf16: the 16 bits shifted left by 16)
 *     c = (v > 0) ? min(v, 1.0f) : 0.0f             NaN and -0 become +0
 *     p = c * f32(m)                                one f32 multiply
 *     q = rint(p), ties to even, under CE_QUANT_NEAREST_EVEN; floor(p) under CE_QUANT_TRUNCATE
 *     NEAREST_EVEN is a framework's round(clamp(float32(x), 0, 1) * m), ties to even, on every input that is not NaN; TRUNCATE is the
 *     mul(255).byte() idiom on in-range input.
 *   a float dtype into a slot of a linear batch: the sample is linear light, f32(x), then the clamp of a linear image (NaN ->
 *     0, then [-CE_LINEAR_MAX, CE_LINEAR_MAX]); quantise must be 0.
 *   CE_DTYPE_U8 into an RGB8 batch or a deep side of depth 8: as it is (widened to u16 on the deep side).
 *   CE_DTYPE_U16 into a deep side: min(v, m), as deep ingest clamps.  Integer dtypes: quantise must be 0.
 * tests/tensor_restatement.py restates this in numpy; the device equals it bit for bit.
 * ce_batch_set_reference_tensor / ce_batch_set_test_tensor: images n = 0 .. count - 1 of the batch's shape into reference slots
 * first_ref + n / test slots first_pair + n, pair first_pair + n bound to reference ref_indices[n].
 *   CE_MEM_HOST: one staged copy and one launch per image on the batch's upload stream, with the ordering of
 *     ce_batch_set_*_fmt; the rows are copied as they are and the tensor is consumed on return.  Only layouts whose rows are
 *     contiguous runs are taken: stride_x = 1 (planar, or gray with stride_c = 0), or stride_c = 1 with stride_x 3 or 4.
 *   CE_MEM_DEVICE: read in place on the context's device, ONE launch for all count images, on the batch's upload stream,
 *     ordered as every slot write and, for this source alone, behind everything the caller has enqueued on the context's stream
 *     (ce_ctx_stream) before the call: a model that runs on the stream the context was created on (ce_ctx_create_on_stream)
 *     needs no host synchronisation between its last kernel and this call.  A tensor written on any other stream must be
 *     complete before the call, as device planes must.  The caller keeps the tensor alive and unchanged until the batch's next
 *     launch has been collected.  The call returns without waiting.
 * CE_ERR_INVALID_ARG, with the reason in ce_last_error and the batch still usable, for a null struct or data pointer, an unknown
 * dtype, memory or quantise value, quantise != 0 where it has no meaning (integer dtypes, linear slots), a negative stride,
 * stride_x < 1 or stride_y < 1 (stride_c = 0 and stride_n = 0 are allowed), a data pointer not aligned to its element size, an
 * extent in bytes that overflows size_t, CE_DTYPE_U8 onto a deep side whose depth is not 8, CE_DTYPE_U16 into an RGB8 batch, an
 * integer dtype into a linear batch, count = 0 or above 65535, a slot range or a ref_indices entry past the batch, and a host
 * layout other than the three above ("make it contiguous or pass device memory").
 * ce_tensor_to_rgb8 / _to_rgb16 / _to_linear: image n = 0 of width x height through the same kernel into host memory, as an
 * RGB8 slot, a deep side of depth_out in {8, 10, 12, 16} or a linear slot would hold it (out_len = width * height * 3
 * samples); errors as above, CE_ERR_BAD_LENGTH for a wrong out_len.
 * Not part of this: tensors through ce_eval_batch, ce_ref_* and the *_over / ICC / CICP routes (a tensor is sRGB-encoded, or
 * linear light with sRGB primaries on a linear batch); signed or 64-bit dtypes; negative strides; float tensors scaled to
 * anything but [0, 1]. */
enum ce_dtype { CE_DTYPE_U8 = 0, CE_DTYPE_U16 = 1, CE_DTYPE_F16 = 2, CE_DTYPE_BF16 = 3, CE_DTYPE_F32 = 4 };
enum ce_quantise { CE_QUANT_NEAREST_EVEN = 0, CE_QUANT_TRUNCATE = 1 };
typedef struct ce_tensor_image {
    const void *data;   /* element (n = 0, c = 0, y = 0, x = 0) */
    int64_t stride_n, stride_c, stride_y, stride_x;   /* in ELEMENTS, not bytes */
    int dtype;          /* enum ce_dtype */
    int memory;         /* enum ce_mem */
    int quantise;       /* enum ce_quantise; float dtypes into integer slots only, otherwise must be 0 */
} ce_tensor_image;
int ce_batch_set_reference_tensor(ce_batch *b, uint32_t first_ref, uint32_t count, const ce_tensor_image *t);
int ce_batch_set_test_tensor(ce_batch *b, uint32_t first_pair, const uint32_t *ref_indices, uint32_t count, const ce_tensor_image *t);
int ce_tensor_to_rgb8(ce_ctx *ctx, const ce_tensor_image *t, uint32_t w, uint32_t h, uint8_t *out, size_t out_len);
int ce_tensor_to_rgb16(ce_ctx *ctx, const ce_tensor_image *t, uint32_t w, uint32_t h, uint32_t depth_out, uint16_t *out, size_t out_len);
int ce_tensor_to_linear(ce_ctx *ctx, const ce_tensor_image *t, uint32_t w, uint32_t h, float *out, size_t out_len);

/* ---- measurement hooks (bench.py) ------------------------------------------------ */
/* Bracket every kernel launch with a HIP event pair, recorded on the stream the kernel is launched on,
 * and accumulate per-kernel time.  on = 0: off (default).  on = 2: events only; the batch keeps its
 * multi-stream schedule, so a kernel's time includes whatever it shares the GPU with (what rocprofv3's
 * kernel trace sees).  on = 1: additionally keep all launches on the context's stream, one kernel at a
 * time ("solo" times). */
int ce_prof_enable(ce_ctx *ctx, int on);
/* restrict the events to kernels whose name contains `substring` (NULL or "" = all kernels; "=name" = exactly that kernel) */
int ce_prof_filter(ce_ctx *ctx, const char *substring);
int ce_prof_reset(ce_ctx *ctx);
/* number of distinct kernels seen; then per index: name, launches, total ms */
int ce_prof_count(ce_ctx *ctx);
int ce_prof_get(ce_ctx *ctx, int index, const char **name, uint64_t *launches, double *total_ms);
/* plain HIP-event stopwatch on the context's stream */
int ce_timer_start(ce_ctx *ctx);
int ce_timer_stop(ce_ctx *ctx, double *elapsed_ms);

/* Test hooks (plane-level parity, arithmetic sweeps, counter calibration) are declared in ce_metrics_debug.h: they are
 * exported by the same library but are not part of the boundary a host binds. */

#ifdef __cplusplus
}
#endif
#endif
