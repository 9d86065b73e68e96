// Internal declarations shared by the host runtime (ce_api.cpp, ce_ingest.cpp, ce_handles.cpp, ce_leaf.cpp, ce_resample.cpp) and the
// gfx950 kernels.
// Nothing here is part of the ABI; the ABI is include/ce_metrics.h.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdio>
#include <functional>
#include <map>
#include <string>
#include <tuple>
#include <utility>
#include <vector>

#include "ce_metrics.h"
#include "ce_metrics_debug.h"
#include "ce_plan.h"
#include "ce_ref_state.h"
#include "ce_owned.h"

#define CE_MAX_SCALES 6      // SSIMULACRA2 pyramid depth
#define CE_SSIM2_STREAMS 5   // blur(a), blur(b), blur(a*a), blur(b*b), blur(a*b)
#define CE_DSSIM_SCALES 5    // dssim-core DEFAULT_WEIGHTS.len()
// where a front end's level 0 comes from: the linear planes of the level below (levels above 0), packed RGB8, or the packed
// u16 RGB of a deep batch (ce_batch_create_deep), or the packed f32 RGB of a linear batch (ce_batch_create_linear: the sample
// is the linear value, no table)
enum { CE_SRC_F32 = 0, CE_SRC_U8 = 1, CE_SRC_U16 = 2, CE_SRC_LIN = 3 };
static_assert(CE_MAX_SCALES == CE_SSIM2_MAX_SCALES, "the ABI's scale count is the pyramid's");

// per-pair device results; PSNR leaves the device as the exact integer SSE and is
// finished on the host with the host libm (bit-identical to the reference's f64 log10).
struct ce_dev_scores {
    double dssim;
    double ssimulacra2;
    double butteraugli;
    unsigned long long sse;
};

struct ce_kernel_stat {
    std::string name;
    uint64_t launches = 0;
    double total_ms = 0.0;
};

// metric chains of a batch run side by side when the batch holds at most this many megapixels of pairs (ce_api.cpp,
// ce_batch_launch; measured in profiles/r02_experiments.md section 15); CE_METRIC_FORK_BELOW_MP overrides it
#ifndef CE_DEFAULT_FORK_BELOW_MP
#define CE_DEFAULT_FORK_BELOW_MP 4.0
#endif
#ifndef CE_DEFAULT_FORK_ALONE_BELOW_MP
#define CE_DEFAULT_FORK_ALONE_BELOW_MP 64.0
#endif

// One axis of a resample on the device.  resample.hip reads d as int32: [n_out] first tap | [n_out] tap count | [n_out][ksize]
// weights (22-bit fixed point).  The float resampler (resample_f32.hip) reads it as n_out * (1 + ksize) doubles, the first
// n_out of them holding, as int32, [n_out] first tap | [n_out] tap count; then [n_out][ksize] f64 weights.
struct ce_resample_axis {
    void *d = nullptr;
    uint32_t n_in = 0, n_out = 0, ksize = 0;
};

// the kinds of one-pair batch a context keeps for its host-image calls (ce_ctx::leaf_batch)
enum ce_leaf_kind { CE_LEAF_RGB8 = 0, CE_LEAF_DEEP = 1, CE_LEAF_LINEAR = 2, CE_LEAF_KINDS = 3 };

struct ce_ctx {
    int device = 0;
    hipStream_t stream = nullptr;
    bool own_stream = true;
    std::string err;

    // device constant tables (built on the host at context creation)
    float *d_lut_ssim2 = nullptr;  // sRGB->linear, f64 formula rounded to f32 (SSIMULACRA2 front end)
    float *d_lut_powf = nullptr;   // sRGB->linear via f32 powf(2.4) (dssim.rs:78-85, xyb.rs:60-66)
    float *d_xyb_thresh = nullptr; // linear->sRGB u8 decision thresholds (xyb.rs:86-88)
    // sRGB->linear tables of the deep batches, 2^depth entries each, keyed by (depth, rule: 0 = the f64 curve, 1 = f32 powf);
    // built by the first deep batch that needs one and kept until the context goes (ce_api.cpp: ce_deep_table)
    std::map<std::pair<uint32_t, int>, float *> deep_tables;
    // the kept one-pair batches (ce_leaf.cpp: leaf_batch), remade when the shape or, deep, a depth changes: RGB8 for
    // ce_calculate_butteraugli_diffmap, ce_calculate_dssim_ssim_maps and ce_calculate_ssimulacra2_maps, deep for
    // ce_eval_pair_deep, linear for ce_eval_pair_linear and ce_eval_pair_hdr_fidelity
    struct ce_batch *leaf_batch[CE_LEAF_KINDS] = {};
    // transfer tables of the CICP ingest (cicp.hip), 2^depth entries each, keyed by (transfer, depth, bits of white_nits);
    // built by the first ingest that needs one and kept until the context goes (ce_ingest.cpp: ingest_table).  The HLG ingest's
    // inverse-OETF tables (cicp.hip) live here too, one per depth, under H.273's code for HLG: (18, depth, 0)
    std::map<std::tuple<int, uint32_t, uint32_t>, float *> cicp_tables;
    // threshold tables of the HDR fidelity scores (hdr_fidelity.hip), keyed by (depth, bits of white_nits), built by the first
    // call that needs one and kept until the context goes (ce_api.cpp: hdr_table_dev): T[1 .. maxv], padded to a multiple of
    // 16 floats, then at depth 16 the coarse level a block stages in LDS (every 16th threshold)
    std::map<std::pair<uint32_t, uint32_t>, float *> hdr_tables;
    // sRGB code thresholds of the ICC ingest into integer slots (icc.hip), keyed by the slot's depth D: 2^D floats with
    // entry k = T[k] for k >= 1 (entry 0 is not read); built by the first such ingest and kept until the context goes
    // (ce_ingest.cpp: icc_thresholds_dev)
    std::map<uint32_t, float *> icc_thresholds;
    // alpha tables of the linear-light composite (over_linear_kernel.h), keyed by the source depth: ce_alpha_table's 2^depth
    // floats; built by the first such composite and kept until the context goes (ce_ingest.cpp: alpha_table_dev)
    std::map<uint32_t, float *> alpha_tables;

    // profiling
    bool prof = false;         // record a HIP event pair around every launch (on the launch's own stream)
    bool prof_serial = false;  // ...and keep everything on the context's stream so kernel times do not overlap
    std::string prof_filter;   // non-empty: only kernels whose name contains this get events
    std::vector<ce_kernel_stat> stats;
    struct pending { int stat; hipEvent_t e0, e1; };
    std::vector<pending> pend;
    std::vector<hipEvent_t> event_pool;
    hipEvent_t t0 = nullptr, t1 = nullptr;

    // scratch batches for the single-pair / mixed-shape entry points, keyed by shape
    // scratch pool for the host-buffer entry points: up to kPoolRing batches per shape (ce_eval_batch streams a large
    // bucket through them in chunks so that the upload of one chunk overlaps the kernels of the previous one)
    static constexpr uint32_t kPoolRing = ce_plan_ring_slots;
    // largest device footprint one ce_eval_batch chunk is sized for (ce_api.cpp: chunk_budget)
    static constexpr size_t kChunkBytesMax = (size_t)48 << 30;
    std::map<std::tuple<uint32_t, uint32_t, uint32_t>, ce_batch *> shape_pool;

    // grow-only scratch of the leaf entry points that take one host image and return one (ce_xyb_roundtrip,
    // ce_rgb8_to_dssim_image): device in / out and a page-locked staging buffer, kept between calls
    uint8_t *leaf_d_in = nullptr, *leaf_d_out = nullptr, *leaf_h = nullptr;
    size_t leaf_in_cap = 0, leaf_out_cap = 0, leaf_h_cap = 0;
    // grow-only device scratch of the image heuristics (heuristics.hip: per-tile partial sums, per-image means and results)
    // and the page-locked buffer their results come back through
    uint8_t *heur_d = nullptr, *heur_h = nullptr;
    size_t heur_d_cap = 0, heur_h_cap = 0;
    // grow-only device scratch of the resamplers (resample.hip, resample_f32.hip): the image between the two passes - u8, or
    // f32 for a linear batch; both resamplers run on the context's stream, so one buffer serves them - and the tap tables of
    // the (in, out, filter, f64 weights?) axes used so far, keyed by them and kept until the context goes (ce_resample.cpp:
    // resample_table)
    uint8_t *rs_mid = nullptr;
    size_t rs_mid_cap = 0;
    std::map<std::tuple<uint32_t, uint32_t, int, bool>, ce_resample_axis> rs_tables;
    // grow-only scratch of the plane-domain scores (plane_fidelity.hip), outside ce_estimate_batch_bytes as the heuristics'
    // is: the host planes of a call without their pitch padding, page-locked and on the device; the plane table with the pair
    // table behind it; the f32 pyramid of levels 1 - 4, [plane][level][image][h][w]; the result integers, [pair][33]
    ce_dev<uint8_t> pf_planes_d, pf_tables_d;
    ce_pinned<uint8_t> pf_planes_h, pf_tables_h;
    ce_dev<float> pf_pyr;
    ce_dev<unsigned long long> pf_out_d;
    ce_pinned<unsigned long long> pf_out_h;
    // ... and of VIFp on the same planes (plane_vif.hip): the f64 pyramid of scales 2 - 4, [plane][scale][image][h][w]; its
    // result integers, [pair][24], go through pf_out_d / pf_out_h
    ce_dev<double> pf_vif_pyr;

    // Auxiliary streams of the context, shared by all its batches (made on first use, destroyed with the context): the
    // three metric chains of a forked batch, SSIMULACRA2's level-0 passes, Butteraugli's half-resolution chain.  Rounds
    // 1-2 made them per BATCH: a context with a scratch batch and a reference handle then held 13 streams, HIP maps streams onto GPU_MAX_HW_QUEUES hardware queues in creation order, and two
    // chains of one call could land on one queue - the same call took 0.45 or 0.8 ms depending on what had been created
    // before it (profiles/r03_experiments.md section 15).
    enum { AUX_METRIC0 = 0, AUX_SSIM2_L0 = 3, AUX_BA_HALF = 4, AUX_COUNT = 5 };
    hipStream_t aux_stream[AUX_COUNT] = {};
    hipStream_t up2_stream = nullptr;  // second DMA stream of ce_eval_batch's page-locked uploads (CE_UPLOAD_STREAMS=2)
    hipEvent_t ev_up2 = nullptr;

    // two parked host threads that enqueue the other metric chains of a forked batch (ce_api.cpp: ce_fork_helpers); made on
    // the first forked launch, joined by ce_ctx_destroy
    struct ce_fork_helpers *helpers = nullptr;
};

// XCD-aware 1-D launch order of a per-pair tile kernel on the device (ce_plan.h, ce_build_xcd_list in ce_api.cpp):
// entry = (tile, pair), with the inputs it was built from; the device list is grow-only
struct ce_xcd_list {
    ce_dev<uint2> d;
    uint32_t len = 0, version = ~0u, pairs = 0;
    ce_xcd_keys keys{};
};

// a device buffer and the page-locked block it is copied from or into, `n` elements each: made together or not at all
template <class T>
struct ce_mirror {
    ce_dev<T> d;
    ce_pinned<T> h;
    int alloc(ce_ctx *ctx, size_t n)
    {
        ce_mirror m;
        if (int rc = m.d.alloc(ctx, n)) return rc;
        if (int rc = m.h.alloc(ctx, n)) return rc;
        *this = std::move(m);
        return CE_OK;
    }
    void reset() { d.reset(), h.reset(); }
    explicit operator bool() const { return d != nullptr; }
};

// A metric's device working set is a value: its *_prepare builds one in a local and moves it into the batch when every
// allocation has succeeded, so a set is whole or empty (engaged()), and it releases itself with the batch.  What a later
// launch adds on first use (the members marked "lazily") is committed the same way, whole or not at all.  Streams in a set
// are the context's auxiliary streams: used and drained (ce_batch_destroy), never destroyed here.

// SSIMULACRA2 working set (ssim2.hip).  Image slots: [0, max_refs) references, then tests.
struct ce_ssim2_set {
    int n_scales = 0;
    ce_plane_geom lvl[CE_MAX_SCALES] = {};  // pitch a multiple of 32 floats (128-byte rows), rows padded to the row pass's block
    ce_dev<float> lin[CE_MAX_SCALES];   // [slots][3][plane_s] linear RGB pyramid (levels 1..: level 0 is read from the slabs)
    ce_dev<float> xyb[CE_MAX_SCALES];   // [slots][3][plane_s] positive XYB, one buffer per level
    ce_dev<float> hbuf[CE_MAX_SCALES];  // [pairs][3][5][plane_s] row-blurred streams, one buffer per level
    // The references' final planes mu1 = blur(a), s11 = blur(a*a), per level [max_refs][3][2][plane_s], which the pair column
    // pass of the split path reads (ssim2.hip: ce_launch_ssim2; record CE_REF_SSIM2_BLUR); lazily, every level or none.
    // split_last: the last launch took the split path, so hbuf holds no streams 0 and 2 (ce_debug_ssim2_planes).
    ce_dev<float> ref_blur[CE_MAX_SCALES];
    bool split_last = false;
    // level 0's row/column pass runs on l0_stream, fenced by ev_prep[0] / ev_done[0] against the front end and the final
    // reduction; the other levels follow the front end on the launching stream ([1]: if they ever leave it)
    hipStream_t l0_stream = nullptr;
    ce_event ev_prep[2], ev_done[2];
    ce_dev<double> partials;  // [pairs][scales][3][max_vblocks][6]
    uint32_t max_vblocks = 0;
    ce_dev<double> avg;       // [pairs][6][3][6]
    // CE_FLAG_SSIMULACRA2_MAPS: per scale s, [max_pairs][channel 3][kind 3][plane_s] per-pixel error maps (d, artifact, detail
    // lost) in one allocation, lazily; map_lvl[s] = scale s's part.  cells: the block-max readouts' device buffer (grow-only)
    ce_dev<float> map;
    float *map_lvl[CE_MAX_SCALES] = {};
    ce_dev<float> cells;
    // XCD-aware work lists of the row / column pass: launch id -> (block, channel, pair)
    ce_xcd_list work_h, work_v;    // level 0
    ce_xcd_list work_ht, work_vt;  // the merged launch of levels 1..
    bool engaged() const { return avg != nullptr; }
};

// DSSIM working set (dssim.hip); planes are [slot][3][plane] with the level's own geometry
struct ce_dssim_set {
    int levels = 0;
    ce_plane_geom lvl[CE_DSSIM_SCALES] = {};
    ce_dev<float> lin[2];  // linear RGB of the current and the next level
    ce_dev<float> img;     // [max_pairs][3][plane_0]: L, a', b' (chroma pre-blurred) of the distorted images, one level at a time
    ce_dev<float> rimg[CE_DSSIM_SCALES], rmu[CE_DSSIM_SCALES], rsq[CE_DSSIM_SCALES];  // the references' planes, per level: [max_refs][3][plane_l]
    ce_dev<float> map;     // [level][max_pairs][plane_l] channel-averaged SSIM maps (SsimMap.map)
    ce_dev<double> part;   // [pairs][levels][2][blocks] partial sums (sum, abs-dev)
    ce_dev<double> level_scores;  // [pairs][CE_DSSIM_SCALES]: after a launch, every level's score (SsimMap.ssim)
    ce_dev<float> cells;   // the block-min readouts' device buffer (grow-only)
    uint32_t blocks = 0;
    ce_xcd_list gwork[CE_DSSIM_SCALES];  // k_dssim_compare_stream's launch order, per level
    bool engaged() const { return level_scores != nullptr; }
};

// a small batch runs Butteraugli's half-resolution chain on a stream of its own, beside the full-resolution one, with its
// own scratch (butteraugli.hip: ce_launch_butteraugli)
struct ce_ba_half {
    hipStream_t stream = nullptr;
    ce_event ev_fork, ev_join;
    ce_dev<float> s[3];
};

// Butteraugli working set (butteraugli.hip): level 0 = full resolution, 1 = 2x-subsampled
struct ce_ba_set {
    ce_plane_geom lvl[2] = {};
    int levels = 0;
    ce_dev<float> psy[2];   // [slot][10][plane_l]  PsychoImage
    ce_dev<float> diff[2];  // [pair][plane_1]      the half-resolution diffmap ([1]; the full-resolution one is reduced in registers)
    ce_dev<float> mask[2];  // [slot][plane_l]      blurred mask input (DiffPrecompute of HF + UHF, sigma 2.7)
    ce_dev<float> s[3];     // per-slot scratch, 3 planes each
    ce_ba_half half;        // lazily
    ce_dev<float> mask_vals[2];  // [ref][2][plane_l]    maskval / dc_maskval of the references (FuzzyErosion + mask curves)
    // CE_FLAG_BUTTERAUGLI_DIFFMAP: [pair][plane_0] full-resolution diffmaps, lazily; cells: the block-max readouts' device
    // buffer (grow-only)
    ce_dev<float> map, cells;
    ce_dev<float> blk_max;
    ce_dev<double> blk_sums;
    ce_dev<double> pnorm;  // [pair] libjxl 3-norm of the last run
    uint32_t blocks = 0;
    ce_xcd_list work[2];  // Malta's launch order, per resolution level
    ce_xcd_list work_lf[2];  // the LF column blur's launch order when it forms the LF term (EPI_LF_TERM), lazily
    bool engaged() const { return pnorm != nullptr; }
};

struct ce_batch {
    ce_ctx *ctx = nullptr;
    uint32_t w = 0, h = 0, max_refs = 0, max_pairs = 0;
    size_t img_bytes = 0;  // w*h*3; w*h*6 in a deep batch; w*h*12 in a linear batch
    bool linear = false;   // a linear batch (ce_batch_create_linear): the slabs hold packed f32 RGB, linear light; depth = 0 / 0
    // A deep batch (ce_batch_create_deep): depth[0] / depth[1] = bits per sample of the reference / test side (8, 10, 12 or
    // 16), the slabs hold packed u16 RGB and the front ends read them through deep_lut[rule][side] (ce_ctx::deep_tables).
    // 0 / 0: an RGB8 batch.
    uint32_t depth[2] = {0, 0};
    const float *deep_lut[2][2] = {};

    ce_dev<uint8_t> d_refs;     // [max_refs][h][w][3]
    ce_dev<uint8_t> d_refs_rt;  // XYB-roundtripped references (lazily)
    ce_dev<uint8_t> d_tests;    // [max_pairs][h][w][3]
    ce_dev<uint32_t> d_pair_ref;
    uint32_t *d_pair_first = nullptr;  // second part of the d_pair_ref allocation
    uint32_t *d_ref_off = nullptr, *d_ref_idx = nullptr;  // ... then reference -> its pairs (CSR: [max_refs + 1] offsets, [max_pairs] pair indices)
    std::vector<uint32_t> h_pair_ref;
    bool pair_ref_dirty = true;
    uint32_t pair_ref_version = 0;  // bumped whenever the pair -> reference table changes
    // pinned staging ring for host -> device uploads: the host copy into slot k overlaps the DMA of slot k-1
    static constexpr int kStages = 8;  // two per upload worker (ce_eval_batch fills a bucket with 4 host threads)
    ce_pinned<uint8_t> h_stage[kStages];
    ce_event ev_stage[kStages];
    bool stage_busy[kStages] = {};
    int next_stage = 0;
    // uploads run on their own stream so that filling one batch overlaps another batch's kernels
    ce_stream up_stream;
    ce_event ev_up, ev_run;  // uploads done / last launch done
    bool uploads_pending = false, run_pending = false;
    bool inline_pending = false;  // a slot was written on the context's stream since the last launch (ce_ingest.cpp: ce_order_write)
    bool counted_in_flight = false;  // this batch is in the device's launched-and-not-collected count (ce_api.cpp: g_in_flight)
    // the wide staging pairs of every image a conversion kernel follows: one pinned + one device staging image each, made
    // on first use and handed out in turn (ce_ingest.cpp: wide_send, which states their size - more once a tensor image needed
    // more - and alone touches them)
    ce_mirror<uint8_t> wide[2];
    ce_event ev_wide[2];
    bool wide_busy[2] = {};
    int next_wide = 0;
    // what a gain-map ingest stages beside its base image, which takes wide pair k: the log2-gain tables and the map's samples
    // in a pinned + device pair of their own (ce_ingest.cpp: upload_gainmap, which states their size), busy with wide pair k
    ce_mirror<uint8_t> side[2];

    // one stream per metric chain when a launch runs several of them (SSIMULACRA2, DSSIM, Butteraugli side by side): the
    // context's auxiliary stream and the event that joins it back, lazily
    struct metric_fork {
        hipStream_t stream = nullptr;
        ce_event ev_join;
    } fork[3];
    ce_event ev_fork;

    // The metrics' working sets, and what the LAST launch left in them: how many pairs stored their SSIMULACRA2 maps (0 after
    // a launch without the flag or without SSIMULACRA2) and left their pooled norms in s2.avg (every launch with SSIMULACRA2),
    // the scales it ran; how many left their SSIM maps in ds.map (every launch with DSSIM does) and their diffmaps in ba.map
    // (CE_FLAG_BUTTERAUGLI_DIFFMAP).  ref_handle: a reference handle's batch.
    ce_ssim2_set s2;
    ce_dssim_set ds;
    ce_ba_set ba;
    uint32_t s2_map_pairs = 0, s2_norm_pairs = 0, s2_scales_run = 0, ds_map_pairs = 0, ba_map_pairs = 0;
    bool ref_handle = false;
    ce_dev<ce_dev_scores> d_scores;
    ce_pinned<ce_dev_scores> h_scores;
    // What the planes derived from the references were built from, per metric and for d_refs_rt (ce_ref_state.h): they stay
    // valid until a reference is written, so later launches only build the distorted side.  Each metric's launch function
    // touches its own record only (the chains of a forked batch are enqueued by three host threads).
    ce_ref_states refs;
    int debug_max_scales = CE_MAX_SCALES;  // test hook: stop the pyramid early
    uint32_t debug_ds_rows = 0;  // test hook (ce_debug_dssim_walk_rows): forced walk length of DSSIM's streaming kernels, 0 = automatic

    // HDR fidelity (hdr_fidelity.hip): [max_pairs][3] exact integers on the device and page-locked, lazily
    ce_mirror<unsigned long long> hdr;
    // Delta E ITP maps (hdr_fidelity.hip: k_delta_e_itp_map): the device buffer of the maps or cell maxima of one call, grow-only;
    // [max_pairs][8] exceedance counts on the device and page-locked, made by the first call that asks for counts
    ce_dev<uint32_t> d_itp_map;
    ce_mirror<unsigned long long> itp_over;
    // SSIM / MS-SSIM (msssim.hip): [max_pairs][5][3][2] exact integers on the device and page-locked, lazily; the f32 pyramid
    // of levels 1 - 4 of every slot (references, then tests), level by level [slot][3][h_l][w_l], made by the first call with
    // five levels and kept
    ce_mirror<unsigned long long> msssim;
    ce_dev<float> d_msssim_pyr;
    // SSIM / MS-SSIM maps (msssim_map.hip): the device buffer of the maps or cell maxima of one call, grow-only; [max_pairs][3][8]
    // exceedance counts on the device and page-locked, made by the first call that asks for counts
    ce_dev<uint32_t> d_msssim_map;
    ce_mirror<unsigned long long> msssim_over;
    // CIEDE2000 (ciede2000.hip): [max_pairs][10] exact integers on the device and page-locked, lazily
    ce_mirror<unsigned long long> ciede2000;
    // CIEDE2000 maps (ciede2000_map.hip: k_ciede2000_map): the device buffer of the maps or cell maxima of one call, grow-only;
    // [max_pairs][8] exceedance counts on the device and page-locked, made by the first call that asks for counts
    ce_dev<uint32_t> d_ciede2000_map;
    ce_mirror<unsigned long long> ciede2000_over;

    uint32_t last_n_pairs = 0;
    bool caller_blocks = false;  // set by entry points that collect before returning: page-locked sources need no staging copy
    uint32_t last_mask = 0;
};

#define CE_HIP(ctx_, expr)                                                                         \
    do {                                                                                           \
        hipError_t e__ = (expr);                                                                   \
        if (e__ != hipSuccess) {                                                                   \
            (ctx_)->err = std::string(#expr) + ": " + hipGetErrorString(e__);                      \
            return CE_ERR_BACKEND;                                                                 \
        }                                                                                          \
    } while (0)

// ---- what the parts of the host runtime share: ce_api.cpp (errors, profiling, contexts, batch lifetime, launch, collect,
// the map read-outs, the calls on a batch's slabs, the pooled ce_eval_batch, reference handles, hooks), ce_ingest.cpp
// (everything that writes a slot), ce_leaf.cpp (host images in, a result out through scratch the context owns) and
// ce_resample.cpp (resampling) -------------------------------------------------------------------------------------------------

// record `msg` as the context's last error (the calling thread's, without a context) and return `code` (ce_api.cpp)
int ce_fail(ce_ctx *ctx, int code, const std::string &msg);
int ce_bad_length(ce_ctx *ctx, size_t want, size_t got);  // CE_ERR_BAD_LENGTH, "Invalid image size: expected ... bytes, got ..."
inline bool ce_deep_depth_ok(uint32_t d) { return d == 8 || d == 10 || d == 12 || d == 16; }

// an ICC -> sRGB colour table on the device (ce_lut_create)
struct ce_lut {
    ce_ctx *ctx;
    uint32_t *d_table;  // [2^24] r | g << 8 | b << 16
};
// a matrix/TRC ICC profile on the device (ce_icc_create; ce_handles.cpp): its matrix and the device copies of
// ce_icc_build_tables for the four source depths 8, 10, 12 and 16, all made by ce_icc_create - nothing in the handle changes
// after that - and kept until the handle goes
struct ce_icc_lut;
struct ce_icc {
    ce_ctx *ctx;
    float m[9];
    bool has_matrix;
    float *d_tables[4];  // [3][2^depth] floats each, by ce_icc_depth_index
    ce_icc_lut *lut = nullptr;  // ce_icc_lut_create's handles: the rest of a LUT-based profile; m is then f32(inv(A))
};
// what a LUT-based profile adds to its input tables (ce_icc_lut_create), immutable like the rest
struct ce_icc_lut {
    bool tetra;              // CE_ICC_CLUT_TETRAHEDRAL
    float *d_clut;           // [g0 * g1 * g2][4] floats, null without a CLUT
    uint32_t grid[3];
    float *d_samples;        // the samples of the SAMPLED curves, null without one
    ce_icc_lut_curve curves[6];  // M then B, as ce_icc_lut_build_curves gives them
    float mat[12];
    bool has_matrix;
    uint32_t pcs;            // 0 XYZ, 1 Lab, 2 Lab in the legacy 16-bit encoding
};
inline int ce_icc_depth_index(uint32_t depth) { return depth == 8 ? 0 : depth == 10 ? 1 : depth == 12 ? 2 : 3; }
// one image of ce_upload_many
struct ce_upload_job {
    uint8_t *dst;
    const uint8_t *src;
};

// The slot-write ordering (ce_ingest.cpp).  ce_order_write comes before every write into a slot, on the context's stream
// or on the batch's upload stream; ce_flush_uploads before every kernel that reads one on the context's stream; a new
// reference slab drops what was derived from the old one.
int ce_order_write(ce_batch *b, bool on_ctx_stream);
int ce_flush_uploads(ce_batch *b);
void ce_invalidate_reference_state(ce_batch *b);
// jobs.size() packed images of b->img_bytes into their slots, from a few host threads (ce_eval_batch; ce_ingest.cpp)
int ce_upload_many(ce_batch *b, const std::vector<ce_upload_job> &jobs);
// `lut` (nullptr: nothing) over the RGB8 image at `slot`, on the batch's upload stream behind its copy (ce_ingest.cpp)
int ce_apply_lut(ce_batch *b, uint8_t *slot, const ce_lut *lut);
// the context's leaf scratch grown to in_bytes / out_bytes, and one host image through it and `launch(d_in, d_out)` on the
// context's stream, complete on return (ce_leaf.cpp): the `in_bytes` at `in`, or what fill(h_in, d_in) writes into the pinned
// h_in, whose device copy will be at d_in (in_bytes = 0: nothing is copied in)
int ce_leaf_scratch(ce_ctx *ctx, size_t in_bytes, size_t out_bytes);
int ce_leaf_roundtrip(ce_ctx *ctx, const void *in, size_t in_bytes, void *out, size_t out_bytes,
                      const std::function<int(uint8_t *, uint8_t *)> &launch);
int ce_leaf_roundtrip(ce_ctx *ctx, size_t in_bytes, const std::function<void(uint8_t *, uint8_t *)> &fill, void *out, size_t out_bytes,
                      const std::function<int(uint8_t *, uint8_t *)> &launch);

// host table -> device memory of `b`, complete on return, without draining the context's stream (ce_api.cpp)
int ce_upload_table(ce_batch *b, void *dst, const void *src, size_t bytes);
// a new device copy of the `bytes` at `host`, complete on return, for the table maps a context keeps; a failed copy frees
// the allocation and fails with "H2D failed (<what>)" (ce_api.cpp)
int ce_device_table(ce_ctx *ctx, const void *host, size_t bytes, const char *what, void **out);
// the metric bits a launch knows
constexpr uint32_t ce_known_metrics = CE_METRIC_DSSIM | CE_METRIC_SSIMULACRA2 | CE_METRIC_BUTTERAUGLI | CE_METRIC_PSNR;
// the length checks of a packed RGB8 pair in the reference's order: mismatch, then wrong length (ce_api.cpp)
int ce_validate_pair(ce_ctx *ctx, size_t ref_len, size_t test_len, size_t w, size_t h);
// a failed call drains the copies that may still read the caller's buffers (ce_api.cpp)
void ce_drain_batch(ce_batch *b);
// HDR fidelity's depth (10, 12 or 16) and white_nits (finite, > 0), refused in that order (ce_api.cpp)
int ce_hdr_params_check(ce_ctx *ctx, uint32_t depth, float white_nits);

// the context's auxiliary stream `which` (ce_ctx::AUX_*), made on first use; nullptr + ctx->err on failure (ce_api.cpp)
hipStream_t ce_ctx_aux_stream(ce_ctx *ctx, int which);

// profiling hooks around a launch (ce_api.cpp)
int ce_prof_begin(ce_ctx *ctx, const char *name, hipStream_t stream);
void ce_prof_end(ce_ctx *ctx, int token, hipStream_t stream);

// The stream a metric's launch function enqueues on: the context's stream, unless the calling thread is one of the helper
// threads that enqueue a forked batch's chains side by side (ce_api.cpp: ce_batch_launch) - those set the override.
extern thread_local hipStream_t ce_tls_stream;
#define CE_STREAM(ctx_) (ce_tls_stream ? ce_tls_stream : (ctx_)->stream)

#define CE_LAUNCH_ON(ctx_, stream_, name_, kern_, grid_, block_, shmem_, ...)                      \
    do {                                                                                           \
        int tok__ = (ctx_)->prof ? ce_prof_begin((ctx_), name_, (stream_)) : -1;                   \
        hipLaunchKernelGGL(kern_, grid_, block_, shmem_, (stream_), __VA_ARGS__);                  \
        if (tok__ >= 0) ce_prof_end((ctx_), tok__, (stream_));                                     \
    } while (0)
#define CE_LAUNCH(ctx_, name_, kern_, grid_, block_, shmem_, ...)                                  \
    CE_LAUNCH_ON(ctx_, CE_STREAM(ctx_), name_, kern_, grid_, block_, shmem_, __VA_ARGS__)

#if defined(__HIPCC__)
// Correctly rounded f32 quotients without the range-scaling steps of the compiler's expansion.  hipcc turns a / b into
// v_div_scale x2, v_rcp, two fused steps refining the reciprocal, a product, two fused quotient corrections, v_div_fmas
// and v_div_fixup (11 instructions).  When neither operand is zero-denominator / infinite / NaN / denormal and the
// quotient is far from overflow and underflow, v_div_scale returns its operands unchanged, v_div_fmas is a plain fma and
// v_div_fixup returns the quotient, so the same arithmetic is 8 instructions, bit for bit.  Measured per call site with
// the oracle's probe ("Operand ranges"; tests/test_wide_content_cpu.py): RGB8 and deep batches keep
// operands and quotients between 2^-22 and 2^27; a LINEAR batch (samples to +-1024, intensity targets to 10 000) takes
// operands from 2^-20 to 2^92, of either sign, and quotients from 2^-42 to 2^23 - still no zero, subnormal or infinite
// operand and no quotient near the ends of the format.  ce_debug_div_sweep checks both forms against operator/ on the
// device over [2^-40, 2^92) with either sign.  A zero denominator would give NaN here where operator/ gives an infinity:
// no site has one (cbrt_poly's denominators step over zero without touching it, every float32 around each crossing is
// in tests/wide_content.py: lab_crossing).
__device__ __forceinline__ float ce_div_refined(float a, float b, float r)  // r = refined reciprocal of b
{
    float q = a * r;
    q = __builtin_fmaf(__builtin_fmaf(-b, q, a), r, q);
    return __builtin_fmaf(__builtin_fmaf(-b, q, a), r, q);
}
__device__ __forceinline__ float ce_rcp_refined(float b)
{
    const float r0 = __builtin_amdgcn_rcpf(b);
    return __builtin_fmaf(__builtin_fmaf(-b, r0, 1.0f), r0, r0);
}
__device__ __forceinline__ float ce_div_noscale(float a, float b) { return ce_div_refined(a, b, ce_rcp_refined(b)); }
#endif

// ---- kernel launchers (one .hip file per metric) ---------------------------------------
int ce_launch_psnr(ce_batch *b, const uint8_t *d_refs, uint32_t n_pairs);
int ce_launch_ingest(ce_ctx *ctx, hipStream_t stream, int format, const void *d_src, uint8_t *d_dst, size_t n_pixels);
int ce_launch_ingest_deep(ce_ctx *ctx, hipStream_t stream, int format, uint32_t depth, const void *d_src, uint16_t *d_dst, size_t n_pixels);
int ce_launch_lut_expand(ce_ctx *ctx, hipStream_t stream, const uint8_t *d_packed, uint32_t *d_table);
int ce_launch_lut_apply(ce_ctx *ctx, hipStream_t stream, uint8_t *d_rgb, const uint32_t *d_table, size_t n_pixels);
int ce_ssim2_prepare(ce_batch *b);
int ce_launch_ssim2(ce_batch *b, const uint8_t *d_refs, uint32_t n_refs_used, uint32_t n_pairs, bool store_maps);
int ce_ssim2_read_maps(ce_batch *b, uint32_t scale, uint32_t channel, uint32_t kind, uint32_t first, uint32_t count,
                       uint32_t block, float *maps, double *norms);
int ce_ssim2_occupancy(int which);
int ce_ssim2_cbrt_sweep(ce_ctx *ctx, uint32_t first_bits, uint64_t count, uint64_t *mismatches, uint64_t *slow_path);
int ce_launch_xyb_roundtrip(ce_ctx *ctx, const uint8_t *d_in, uint8_t *d_out, size_t n_pixels);
int ce_launch_dssim(ce_batch *b, const uint8_t *d_refs, uint32_t n_refs_used, uint32_t n_pairs);
int ce_launch_butteraugli(ce_batch *b, const uint8_t *d_refs, uint32_t n_refs_used, uint32_t n_pairs, float intensity_target,
                          bool store_map);
int ce_butteraugli_read_maps(ce_batch *b, uint32_t first, uint32_t count, uint32_t block, float *out);
int ce_dssim_read_maps(ce_batch *b, uint32_t level, uint32_t first, uint32_t count, uint32_t block, float *maps, double *ssim);
// a readout of pitched per-pair maps, g.plane floats from one pair's to the next's, through the grow-only `cells` (maps.hip)
int ce_read_map_cells(ce_batch *b, const char *name, const float *map, ce_plane_geom g, uint32_t first, uint32_t count, uint32_t block,
                      bool take_min, ce_dev<float> &cells, float *out);
int ce_butteraugli_div_sweep(ce_ctx *ctx, uint64_t seed, uint64_t count, uint64_t *mismatches);
int ce_calibrate_traffic(ce_ctx *ctx, size_t bytes);
int ce_build_xcd_list(ce_batch *b, uint32_t n_pairs, const ce_xcd_keys &keys, ce_xcd_list *list);
int ce_launch_rgb8_to_dssim_image(ce_ctx *ctx, const uint8_t *d_rgb, float *d_rgba, size_t n_pixels);
// compute_heuristics of n packed RGB8 images of one shape, img_stride bytes apart on the device, on the context's stream;
// returns after the results are in out (heuristics.hip)
int ce_image_heuristics_run(ce_ctx *ctx, const uint8_t *d_imgs, size_t img_stride, uint32_t w, uint32_t h, uint32_t n,
                            ce_image_heuristics *out);

// n images of w x h packed RGB8, src_stride bytes apart, to out_w x out_h, dst_stride apart, on `stream` (resample.hip):
// `horiz` / `vert` are the axes whose size changes (nullptr: that pass is skipped; both nullptr is the caller's byte copy),
// `mid` holds the n x h x out_w x 3 bytes between the passes when both run
int ce_launch_resample(ce_ctx *ctx, hipStream_t stream, const uint8_t *d_src, size_t src_stride, uint8_t *d_dst, size_t dst_stride,
                       uint32_t w, uint32_t h, uint32_t out_w, uint32_t out_h, uint32_t n, const ce_resample_axis *horiz,
                       const ce_resample_axis *vert, uint8_t *mid);
// what both resample launchers end with: the launches' error, if any, as "resample: <HIP's words>"
inline int ce_resample_launched(ce_ctx *ctx)
{
    const hipError_t e = hipGetLastError();
    if (e == hipSuccess) return CE_OK;
    ctx->err = std::string("resample: ") + hipGetErrorString(e);
    return CE_ERR_BACKEND;
}

// The same for packed f32 RGB (a linear batch's slabs; resample_f32.hip): strides in floats, `mid` the n x h x out_w x 3 floats
// between the passes; the last pass that runs clamps its store to +-CE_LINEAR_MAX
int ce_launch_resample_f32(ce_ctx *ctx, hipStream_t stream, const float *d_src, size_t src_stride, float *d_dst, size_t dst_stride,
                           uint32_t w, uint32_t h, uint32_t out_w, uint32_t out_h, uint32_t n, const ce_resample_axis *horiz,
                           const ce_resample_axis *vert, float *mid);

// One Y'CbCr image on the device as yuv.hip reads it: checked by ce_ingest.cpp (yuv_check), planes in device memory
struct ce_yuv_dev {
    const uint8_t *plane[3];
    size_t pitch[3];         // bytes
    int subsampling, layout, upsample;
    uint32_t depth, shift;   // bits per sample; right shift of an MSB-aligned u16 sample (0: low-aligned)
    int64_t k[7];            // ce_yuv_coefficients for (matrix, range, depth, depth_out)
};
// w x h pixels of `src` -> packed RGB at d_dst: u8 (depth_out = 8, out16 = false) or u16 of depth_out, one launch (yuv.hip)
int ce_launch_yuv(ce_ctx *ctx, hipStream_t stream, const ce_yuv_dev &src, uint32_t w, uint32_t h, void *d_dst, bool out16, uint32_t depth_out);
// what the two launchers of Y'CbCr planes put into yuv_kernel.h's yuv_args: `src` at w x h, the integer RGB clamped to m
template <class YuvArgs>
inline void ce_fill_yuv_args(YuvArgs &a, const ce_yuv_dev &src, uint32_t w, uint32_t h, int64_t m)
{
    a.p0 = src.plane[0], a.p1 = src.plane[1], a.p2 = src.plane[2];
    a.pitch0 = src.pitch[0], a.pitch1 = src.pitch[1], a.pitch2 = src.pitch[2];
    a.w = w, a.h = h;
    a.cw = src.subsampling == CE_YUV_444 ? w : (w + 1) / 2;
    a.ch = src.subsampling == CE_YUV_420 ? (h + 1) / 2 : h;
    a.shift = src.shift, a.maxv = (1u << src.depth) - 1u;
    a.triangle = src.upsample == CE_CHROMA_TRIANGLE;
    a.ky = src.k[0], a.krv = src.k[1], a.kgu = src.k[2], a.kgv = src.k[3], a.kbu = src.k[4], a.y0 = src.k[5], a.c0 = src.k[6];
    a.m = m;
}

// n_pixels RGBA pixels at d_src (u8, or u16 of `depth` bits: src16) source-over onto each of n_bg solid colours
// (backgrounds[n_bg][3], <= 2^depth - 1) -> n_bg consecutive packed RGB images from d_dst on, u8 or u16 (dst16; u8
// samples: depth 8), one launch (alpha.hip)
int ce_launch_alpha(ce_ctx *ctx, hipStream_t stream, const void *d_src, bool src16, void *d_dst, bool dst16, uint32_t depth,
                    size_t n_pixels, uint32_t n_bg, const uint16_t *backgrounds);

// `count` images of a strided tensor on the device as tensor.hip reads them: checked by ce_ingest.cpp (tensor_check), the
// strides in elements, data in device memory
struct ce_tensor_dev {
    const void *data;
    int64_t stride_n, stride_c, stride_y, stride_x;
    int dtype;     // enum ce_dtype
    int quantise;  // enum ce_quantise
};
// w x h pixels of each of `count` images of `src` -> packed RGB in `count` slots slot_bytes apart from d_dst on, one launch
// (tensor.hip).  slot: 0 u8, 1 u16 of `depth` bits, 2 f32 linear light (depth unused); the (dtype, slot) pairs the header
// admits, anything else is CE_ERR_INVALID_ARG
int ce_launch_tensor(ce_ctx *ctx, hipStream_t stream, const ce_tensor_dev &src, uint32_t w, uint32_t h, uint32_t count, void *d_dst,
                     size_t slot_bytes, int slot, uint32_t depth);

// n_samples floats at d_src (16-byte aligned staging) -> d_dst with NaN -> 0 and the clamp to +-CE_LINEAR_MAX (cicp.hip)
int ce_launch_linear_sanitise(ce_ctx *ctx, hipStream_t stream, const float *d_src, float *d_dst, size_t n_samples);
// What one ingest into a linear batch converts a pixel's three code values with (checked and filled by ce_ingest.cpp): the
// device table of maxv + 1 floats - a CICP transfer's, or with `hlg` the inverse OETF's - the primaries matrix (has_matrix:
// primaries other than 1) and, for HLG, ce_hlg_params' five doubles {kR, kG, kB, gamma - 1, A}
struct ce_linear_pixel {
    const float *d_table;
    uint32_t maxv;
    bool has_matrix;
    float m[9];
    bool hlg = false;
    double hlg_params[5];
};
// what the two launchers below put into hlg_pixel.h's hlg_args, whose `c` alone is the CICP pixel's cicp_args: the slot, the
// table, the matrix (without one m is not read) and, for HLG, the five doubles
template <class HlgArgs>
inline void ce_fill_pixel_args(HlgArgs &a, float *d_dst, const ce_linear_pixel &px)
{
    a.c.dst = d_dst, a.c.table = px.d_table, a.c.maxv = px.maxv;
    if (px.has_matrix)
        for (int i = 0; i < 9; i++) a.c.m[i] = px.m[i];
    if (px.hlg) a.kr = px.hlg_params[0], a.kg = px.hlg_params[1], a.kb = px.hlg_params[2], a.gm1 = px.hlg_params[3], a.a = px.hlg_params[4];
}
// n_pixels RGB(A) pixels of u8 / u16 samples at d_src (16-byte aligned staging; format: CE_PIXEL_RGB8 / RGBA8 / RGB16 /
// RGBA16) -> packed f32 RGB at d_dst, one launch (cicp.hip).  CICP: table[min(v, maxv)] per channel, then, with a matrix, the
// 3 x 3 product in separately rounded f32 operations, then the clamp of a linear image.  HLG: between the gather and the
// matrix, k = (float)(A * hlg_pow(ys, gamma - 1)) scales the three.
int ce_launch_tagged(ce_ctx *ctx, hipStream_t stream, int format, const void *d_src, float *d_dst, size_t n_pixels, const ce_linear_pixel &px);
// w x h pixels of `src`, whose k was built for depth_out = log2(px.maxv + 1), -> packed f32 RGB at d_dst: ce_launch_yuv's
// integer RGB in [0, maxv] handed pixel by pixel to ce_launch_tagged's pixel, one launch (yuv_cicp.hip)
int ce_launch_yuv_tagged(ce_ctx *ctx, hipStream_t stream, const ce_yuv_dev &src, uint32_t w, uint32_t h, float *d_dst, const ce_linear_pixel &px);
// What one gain-map ingest applies (checked and filled by ce_ingest.cpp: gainmap_check): the base's CICP pixel, the map's
// shape, the offsets per output channel as doubles and the log2-gain tables ce_gainmap_tables returns, 256 per map channel
struct ce_gainmap_plan {
    ce_linear_pixel base;
    uint32_t gw, gh, channels;
    double base_offset[3], alternate_offset[3];
    double ytab[3 * 256];
    size_t table_bytes() const { return (size_t)channels * 256 * sizeof(double); }
    size_t map_bytes() const { return (size_t)gw * gh * channels; }
};
// w x h RGB(A) pixels of u8 / u16 samples at d_src (16-byte aligned staging; the four formats of ce_launch_tagged) with the
// gain map applied -> packed f32 RGB at d_dst, one launch (gainmap.hip).  d_side holds the plan's tables (8-byte aligned) and
// behind them the map's samples, as ce_ingest.cpp's gainmap_side packs them.
int ce_launch_gainmap(ce_ctx *ctx, hipStream_t stream, int format, const void *d_src, const uint8_t *d_side, float *d_dst, uint32_t w, uint32_t h,
                      const ce_gainmap_plan &plan);

// What one ICC ingest converts a pixel with (checked by ce_ingest.cpp: icc_check, filled by its icc_plan): the profile's three device
// tables of the source depth, [3][maxv + 1] floats, its matrix (has_matrix: colorants other than the canonical sRGB profile's)
// and, for an integer slot of depth_out bits (0: a linear slot; out16: u16 samples), the sRGB code thresholds of that depth
// with d_thr[k] = T[k] for k = 1 .. 2^depth_out - 1
struct ce_icc_pixel {
    const float *d_tables = nullptr;
    uint32_t maxv = 0;
    bool has_matrix = false;
    float m[9] = {};
    uint32_t depth_out = 0;
    bool out16 = false;
    const float *d_thr = nullptr;
    const ce_icc_lut *lut = nullptr;  // a LUT-based profile: m is f32(inv(A)) and icc_lut.hip's launch takes the image
};
// n_pixels RGB(A) pixels of u8 / u16 samples at d_src (16-byte aligned staging; the four formats of ce_launch_tagged) ->
// packed f32 RGB, or packed u8 / u16 sRGB code values, at d_dst, one launch (icc.hip).  With `ov` (a linear slot, RGBA8 /
// RGBA16 only): blended over ov->n_bg backgrounds into as many consecutive slots from d_dst on (ce_over_plan, below)
struct ce_over_plan;
int ce_launch_icc(ce_ctx *ctx, hipStream_t stream, int format, const void *d_src, void *d_dst, size_t n_pixels, const ce_icc_pixel &px,
                  const ce_over_plan *ov = nullptr);
// the same for px.lut != nullptr, which ce_launch_icc hands on (icc_lut.hip)
int ce_launch_icc_lut(ce_ctx *ctx, hipStream_t stream, int format, const void *d_src, void *d_dst, size_t n_pixels, const ce_icc_pixel &px,
                      const ce_over_plan *ov = nullptr);
// what the launchers of a matrix/TRC profile put into icc_pixel.h's icc_args beside the frame's own src, dst and n_pixels:
// the three tables of maxv + 1 floats and the matrix (without one m is not read)
template <class IccArgs>
inline void ce_fill_icc_args(IccArgs &a, const ce_icc_pixel &px)
{
    a.c.maxv = px.maxv;
    a.c.table = px.d_tables, a.table_g = px.d_tables + (size_t)px.maxv + 1, a.table_b = px.d_tables + 2 * ((size_t)px.maxv + 1);
    if (px.has_matrix)
        for (int i = 0; i < 9; i++) a.c.m[i] = px.m[i];
}
// the same for a LUT-based profile (px.lut != nullptr) and icc_lut_pixel.h's icc_lut_args: the tables, f32(inv(A)), the CLUT's
// geometry, the 3 x 4 matrix, the PCS and the six post-CLUT curves
template <class IccLutArgs>
inline void ce_fill_icc_lut_args(IccLutArgs &a, const ce_icc_pixel &px)
{
    const ce_icc_lut *lut = px.lut;
    a.c.maxv = px.maxv;
    a.c.table = px.d_tables, a.table_g = px.d_tables + (size_t)px.maxv + 1, a.table_b = px.d_tables + 2 * ((size_t)px.maxv + 1);
    for (int i = 0; i < 9; i++) a.c.m[i] = px.m[i];
    a.clut = reinterpret_cast<decltype(a.clut)>(lut->d_clut);
    if (lut->d_clut) {
        a.s0 = lut->grid[1] * lut->grid[2], a.s1 = lut->grid[2];
        a.i0 = lut->grid[0] - 2, a.i1 = lut->grid[1] - 2, a.i2 = lut->grid[2] - 2;
        a.g0 = (float)(lut->grid[0] - 1), a.g1 = (float)(lut->grid[1] - 1), a.g2 = (float)(lut->grid[2] - 1);
    }
    a.has_matrix = lut->has_matrix, a.pcs = lut->pcs;
    for (int i = 0; i < 12; i++) a.mat[i] = lut->mat[i];
    for (int k = 0; k < 6; k++) {
        const ce_icc_lut_curve &c = lut->curves[k];
        auto &o = k < 3 ? a.mc[k] : a.bc[k - 3];
        o.kind = (uint32_t)c.kind;
        o.n = c.kind == CE_ICC_LUT_CURVE_SAMPLED ? c.count : c.ftype;
        o.s = c.kind == CE_ICC_LUT_CURVE_SAMPLED ? lut->d_samples + c.first_sample : nullptr;
        for (int i = 0; i < 7; i++) o.q[i] = c.q[i];
        (k < 3 ? a.has_m : a.has_b) |= c.kind != CE_ICC_LUT_CURVE_IDENTITY;
    }
}
// w x h pixels of `src`, whose k was built for depth_out = log2(px.maxv + 1) (the call's rgb_depth), -> what ce_launch_icc
// makes of ce_launch_yuv's integer RGB: packed f32 RGB, or packed u8 / u16 sRGB code values of px.depth_out bits, at d_dst,
// one launch and no integer RGB image between the halves (yuv_icc.hip); either flavour of profile
int ce_launch_yuv_icc(ce_ctx *ctx, hipStream_t stream, const ce_yuv_dev &src, uint32_t w, uint32_t h, void *d_dst, const ce_icc_pixel &px);
// its three halves, one per slot kind (0 f32, 1 u8, 2 u16) and per object that yuv_icc.hip is compiled into: the launch alone,
// the arguments checked by ce_launch_yuv_icc
int ce_launch_yuv_icc_0(ce_ctx *ctx, hipStream_t stream, const ce_yuv_dev &src, uint32_t w, uint32_t h, void *d_dst, const ce_icc_pixel &px);
int ce_launch_yuv_icc_1(ce_ctx *ctx, hipStream_t stream, const ce_yuv_dev &src, uint32_t w, uint32_t h, void *d_dst, const ce_icc_pixel &px);
int ce_launch_yuv_icc_2(ce_ctx *ctx, hipStream_t stream, const ce_yuv_dev &src, uint32_t w, uint32_t h, void *d_dst, const ce_icc_pixel &px);

// What a linear-light composite blends with (checked and filled by ce_ingest.cpp: over_check): the
// device alpha table of the source depth (ce_alpha_table; nullptr for CE_PIXEL_RGBA_F32, whose alpha is the coverage), the
// checked backgrounds in linear light and the distance from one slot to the next in floats
struct ce_over_plan {
    const float *d_atab = nullptr;
    uint32_t n_bg = 0;
    float bg[CE_MAX_BACKGROUNDS][3] = {};
    size_t slot_floats = 0;
};
// ce_launch_tagged's pixel on an RGBA8 / RGBA16 image, blended over ov.n_bg backgrounds into as many consecutive slots from
// d_dst on, one launch (cicp.hip: over_linear_kernel.h's k_tagged_over)
int ce_launch_tagged_over(ce_ctx *ctx, hipStream_t stream, int format, const void *d_src, float *d_dst, size_t n_pixels, const ce_linear_pixel &px,
                          const ce_over_plan &ov);
// (ce_launch_icc and ce_launch_icc_lut take the plan as their last argument: the ICC pixel of a linear slot in the same frame)
// n_pixels CE_PIXEL_RGBA_F32 pixels at d_src (16-byte aligned staging), straight or premultiplied, over ov.n_bg backgrounds
// (cicp.hip: k_linear_over)
int ce_launch_linear_over(ce_ctx *ctx, hipStream_t stream, const float *d_src, float *d_dst, size_t n_pixels, bool premultiplied,
                          const ce_over_plan &ov);
// what the launchers put into over_linear_kernel.h's over_args
template <class OverArgs>
inline void ce_fill_over_args(OverArgs &o, const ce_over_plan &ov)
{
    o.atab = ov.d_atab, o.n_bg = ov.n_bg, o.slot_floats = ov.slot_floats;
    for (uint32_t k = 0; k < CE_MAX_BACKGROUNDS; k++)
        for (int c = 0; c < 3; c++) o.bg[k][c] = ov.bg[k][c];
}

// pairs [0, n_pairs) of a linear batch -> d_out[pair][3] = pq_sse, itp_sum_q20, itp_max_q20, cleared and filled on the
// launching stream (hdr_fidelity.hip): d_table = T[1 .. maxv], 64-byte aligned, d_coarse the level staged in LDS (the table
// itself at depths 10 and 12, every 16th threshold at 16), a / lms = ce_build_hdr_fidelity_matrices
int ce_launch_hdr_fidelity(ce_batch *b, uint32_t n_pairs, uint32_t depth, const float *d_table, const float *d_coarse, const float a[9],
                           const float lms[9], unsigned long long *d_out);

// pairs [first, first + count) of a linear batch, same tables and matrices: every pixel's Delta E ITP in units of 2^-20,
// saturated to 32 bits, into d_map - [count][h][w] at block 1, else the maxima of block x block cells, [count][ceil(h / block)]
// [ceil(w / block)], cleared here; nullptr: no map - and into d_over[count][8] how many pixels exceed thresholds[j],
// j < n_thresholds <= 8, cleared here (nullptr: no counts)
int ce_launch_delta_e_itp_map(ce_batch *b, uint32_t first, uint32_t count, uint32_t depth, const float *d_table, const float *d_coarse,
                              const float a[9], const float lms[9], uint32_t block, uint32_t *d_map, const uint32_t *thresholds,
                              uint32_t n_thresholds, unsigned long long *d_over);

// pairs [0, n_pairs) of an RGB8 or deep batch -> d_out[pair][10] = sum_q20, max_q20, n_above[8], cleared and filled on the
// launching stream (ciede2000.hip): d_table_ref / d_table_test = ce_srgb_table(depth, 0) of the two sides (depth 8 for an RGB8
// batch), thresholds[j], j < n_thresholds <= 8, what n_above[j] counts the pixels above
int ce_launch_ciede2000(ce_batch *b, uint32_t n_pairs, const float *d_table_ref, const float *d_table_test, const uint32_t *thresholds,
                        uint32_t n_thresholds, unsigned long long *d_out);
// ce_ciede2000_pixels' loop (ce_ciede2000_host.cpp: ciede2000_pixel.h compiled for the host): n pixels of packed u16 RGB a side,
// read through the sides' tables of maxv + 1 floats
void ce_ciede2000_pixels_host(const uint16_t *ref_rgb, const float *ref_table, uint32_t ref_maxv, const uint16_t *test_rgb,
                              const float *test_table, uint32_t test_maxv, size_t n, uint32_t *out_q20);
// ce_ciede2000_pixel_terms' loop, beside it: out[n][4] = q and the magnitudes of the lightness, chroma and hue terms
void ce_ciede2000_pixel_terms_host(const uint16_t *ref_rgb, const float *ref_table, uint32_t ref_maxv, const uint16_t *test_rgb,
                                   const float *test_table, uint32_t test_maxv, size_t n, uint32_t *out);
// pairs [first, first + count) of an RGB8 or deep batch (ciede2000_map.hip): value `what` (CE_CIEDE2000_MAP_*) of every pixel into
// d_map[count][h][w] (block 1) or its maximum over block x block cells into d_map[count][ch][cw], which is cleared first (nullptr:
// no map); d_over[count][8] (nullptr: no counts) = how many pixels exceed thresholds[j], j < n_thresholds <= 8, cleared first.
// The tables are ce_launch_ciede2000's.
int ce_launch_ciede2000_map(ce_batch *b, uint32_t first, uint32_t count, uint32_t what, const float *d_table_ref, const float *d_table_test,
                            uint32_t block, uint32_t *d_map, const uint32_t *thresholds, uint32_t n_thresholds, unsigned long long *d_over);

// pairs [0, n_pairs) of an RGB8 or equal-depth deep batch, whose level l is lw[l] x lh[l] (ce_msssim_levels) -> d_out[pair][5]
// [3][2] = ssim_q, cs_q, cleared and filled on the launching stream (msssim.hip): with five levels, every reference slot the
// pairs name and the pairs' test slots are pooled level by level into d_pyr (ce_batch::d_msssim_pyr's layout), and each level
// is one launch of the fused kernel
int ce_launch_msssim(ce_batch *b, uint32_t n_pairs, uint32_t levels, const uint32_t *lw, const uint32_t *lh, float *d_pyr,
                     unsigned long long *d_out);

// Level l of the two sides of such a batch as the level kernels read it (msssim.hip): slot 0 of the references and of the tests -
// the slabs at level 0 (packed RGB: px = 3, chan = 1), the planar f32 pyramid above (px = 1, chan = w * h) - with the elements
// from a slot to the next; kind: 0 u8 slabs, 1 u16 slabs, 2 the pyramid
struct ce_msssim_planes {
    const void *refs, *tests;
    size_t slot, chan, px;
    int kind;
};
ce_msssim_planes ce_msssim_level_planes(const ce_batch *b, uint32_t l, const uint32_t *lw, const uint32_t *lh, float *d_pyr);
// Levels from + 1 .. last of d_pyr from level `from`, on the launching stream: every reference slot that pairs [first, first +
// count) name, once each, and those pairs' test slots.  from == last: nothing.
int ce_msssim_pool(ce_batch *b, uint32_t first, uint32_t count, uint32_t from, uint32_t last, const uint32_t *lw, const uint32_t *lh,
                   float *d_pyr);

// Pairs [first, first + count) of such a batch at `level` (msssim_map.hip; include/ce_metrics.h: ce_batch_msssim_map): the
// pyramid pooled as far as `level`, then every valid position's 2^32 - qs (what = 0) or 2^32 - qc (1), saturated to 32 bits,
// into d_map - [count][3][vh][vw] at block 1, else the maxima of block x block cells, [count][3][ceil(vh / block)]
// [ceil(vw / block)]; nullptr: no map - and into d_over[count][3][8] how many positions exceed thresholds[j], j <
// n_thresholds <= 8, cleared here (nullptr: no counts)
int ce_launch_msssim_map(ce_batch *b, uint32_t first, uint32_t count, uint32_t level, const uint32_t *lw, const uint32_t *lh, float *d_pyr,
                         uint32_t what, uint32_t block, uint32_t *d_map, const uint32_t *thresholds, uint32_t n_thresholds,
                         unsigned long long *d_over);

// What the plane-domain scores (plane_fidelity.hip) take from the Y'CbCr ingest's own check of an image (ce_ingest.cpp:
// yuv_check, with every refusal of it): the planes as the layout stores them - 1, or 2 (semiplanar), or 3 - with their rows
// and their rows' bytes, and the shift of MSB-aligned samples
struct ce_yuv_planes {
    int n_stored = 0;
    size_t rows[3] = {}, row_bytes[3] = {};
    uint32_t shift = 0;
};
int ce_yuv_planes_check(ce_ctx *ctx, const ce_yuv_image *img, uint32_t w, uint32_t h, ce_yuv_planes *out);

// host-side constant builders (ce_tables.cpp)
// HDR fidelity's PQ code thresholds (include/ce_metrics.h: ce_pq_code_thresholds; maxv entries; false unless white_nits is
// finite and > 0) and its two matrices (ce_hdr_fidelity_matrices)
bool ce_build_pq_code_thresholds(uint32_t maxv, double white_nits, float *out);
void ce_build_hdr_fidelity_matrices(float a[9], float b[9]);
// the HLG ingest's inverse-OETF table (include/ce_metrics.h: ce_hlg_table) and the Y row of the f64 XYZ <- src matrix of
// `primaries` (ce_hlg_params' kR, kG, kB); false for primaries that are not offered
void ce_build_hlg_table(uint32_t maxv, float *lut);
// the gain-map ingest's weight W (include/ce_metrics.h: ce_gainmap_weight) and its log2-gain tables, 256 doubles for each of
// `channels` channels with W folded in (ce_gainmap_tables), of checked metadata
double ce_build_gainmap_weight(const ce_gainmap *g);
void ce_build_gainmap_tables(const ce_gainmap *g, uint32_t channels, double *out);
bool ce_build_luminance_row(int primaries, double k[3]);
// the CICP ingest's transfer table (include/ce_metrics.h: ce_transfer_table) and primaries matrix (ce_colour_matrix); false
// for a code point that is not offered
bool ce_build_transfer_table(int transfer, uint32_t maxv, double white_nits, float *lut);
bool ce_build_colour_matrix(int primaries, float m[9]);
// the resampler's taps of one axis, n_in -> n_out samples (include/ce_metrics.h, enum ce_resample_filter): table = [n_out]
// first tap | [n_out] tap count | [n_out][ksize] weights; false for an unknown filter or an empty axis
bool ce_build_resample_table(uint32_t n_in, uint32_t n_out, int filter, std::vector<int32_t> &table, uint32_t *ksize);
// the float resampler's: the same geometry with the normalised f64 weights themselves, in the layout ce_resample_axis gives for resample_f32.hip
bool ce_build_resample_table_f64(uint32_t n_in, uint32_t n_out, int filter, std::vector<double> &table, uint32_t *ksize);
void ce_build_srgb_lut_f64(float lut[256]);
void ce_build_srgb_lut_powf(float lut[256]);
// the same two rules for samples 0 .. maxv meaning v / maxv: lut has maxv + 1 entries
void ce_build_srgb_table_f64(float *lut, uint32_t maxv);
void ce_build_srgb_table_powf(float *lut, uint32_t maxv);
void ce_ssim2_recursive_gaussian(float mul_in[3], float mul_prev[3]);
bool ce_build_xyb_srgb_thresholds(float thresh[256]);
