// Host-side launch planning, plain C++ without device calls, checked on the host by tests/cpp/test_eval_plan.cpp: how
// ce_eval_batch cuts a shape bucket into chunks, and the XCD-aware work lists of the per-pair tile kernels.  The callers
// (ce_api.cpp and the metrics' launch functions) read the inputs from their context and put the result on the device.
#pragma once

#include <algorithm>
#include <cstdint>
#include <map>
#include <vector>

// one pitched float plane of every metric's working set and of the per-pixel maps: w x h samples, rows `pitch` floats apart,
// the next plane `plane` floats on.  Kernels take it by value.
struct ce_plane_geom {
    uint32_t w, h, pitch;
    size_t plane;
};

// What one launch takes.  A grid's y and z hold at most 65535 blocks, and the main metrics' front ends
// put the launch's image slots - the references it uses plus its pairs - or a plane's rows into one of them.
inline constexpr uint32_t ce_grid_yz_max = 65535;
inline constexpr uint32_t ce_launch_slots_max = ce_grid_yz_max;    // references + pairs of a launch with DSSIM, SSIMULACRA2 or Butteraugli
inline constexpr uint32_t ce_ba_height_max = 4 * ce_grid_yz_max;     // Butteraugli: k_ba_mask_vals, 4 rows to a block of y
inline constexpr uint32_t ce_ssim2_height_max = 8 * ce_grid_yz_max;  // SSIMULACRA2: k_ssim2_prep, 4 rows of 2 x 2 quads to a block of y

inline constexpr uint32_t ce_plan_ring_slots = 3;  // pooled batches per shape a bucket streams through (ce_ctx::kPoolRing)
inline constexpr size_t ce_plan_none = ~(size_t)0;

struct ce_plan_inputs {
    size_t budget;          // bytes one chunk may allocate (chunk_budget, read once per bucket)
    size_t per_pair;        // estimated device bytes of one pair with a reference of its own
    uint32_t pooled_pairs;  // max_pairs of this shape's pooled batch on ring slot 0, 0 if there is none
    size_t forced_chunks;   // CE_EVAL_BATCH_CHUNKS, 0 = by size
    size_t ramp;            // CE_EVAL_BATCH_RAMP: pairs of the call's first chunk, 0 = every chunk at the target
    size_t max_slots = ce_launch_slots_max;  // references plus pairs one launch takes, at least 2; a caller that names none gets the launch's own
};

struct ce_plan_chunk {
    uint32_t slot;                          // ring slot: the pooled batch (w, h, slot) the chunk runs on
    uint32_t max_pairs;                     // pairs that batch is allocated for
    size_t collect_first;                   // the earlier chunk on the same batch, collected before this one is filled
    std::vector<std::vector<size_t>> refs;  // per reference slot, its items (indices into the call's pairs)
};

// Appends the chunks of one bucket to `plan`.  refs[j] is the reference pointer of items[j]; ring counts the call's
// chunks so far (0: the next one is the call's first).
inline void ce_plan_bucket(const std::vector<size_t> &items, const std::vector<const void *> &refs, const ce_plan_inputs &in,
                           uint32_t &ring, std::vector<ce_plan_chunk> &plan)
{
    // all pairs of a reference stay together, identical reference pointers share one device slot (first-appearance order)
    std::map<const void *, size_t> group_of;
    std::vector<std::vector<size_t>> groups;
    for (size_t j = 0; j < items.size(); j++) {
        const size_t g = group_of.emplace(refs[j], groups.size()).first->second;
        if (g == groups.size()) groups.emplace_back();
        groups[g].push_back(items[j]);
    }
    // A bucket that fits is cut into chunks (the upload of one overlaps the kernels of the one before) only once it holds
    // 64 pairs per chunk: on the 54-pair Kodak bucket with three metrics one chunk took 9.1 ms per grid, two 12.7, three
    // 10.1 (round 2).  Buckets of different shapes still overlap: each has its own batch and upload stream.
    const size_t n = items.size();
    const size_t n_chunks = in.forced_chunks ? std::min<size_t>(in.forced_chunks, std::max<size_t>(1, n))
                                             : std::min<size_t>(ce_plan_ring_slots, std::max<size_t>(1, n / 64));
    // ... and fits the budget (a larger grid streams through the ring in more chunks; a reference with more tests than
    // that is split and uploaded once per part)
    size_t target = std::min((n + n_chunks - 1) / n_chunks, std::max<size_t>(1, in.budget / std::max<size_t>(in.per_pair, 1)));
    // ... and a launch: a chunk holds its references beside its pairs, the smallest one reference beside `target` pairs
    target = std::min(target, std::max<size_t>(in.max_slots, 2) - 1);
    // a pooled batch a little smaller than that (estimate and free memory move by a few per cent) is used as it is
    if (in.pooled_pairs < target && (size_t)in.pooled_pairs * 4 >= target * 3) target = in.pooled_pairs;
    std::vector<std::vector<size_t>> split;
    for (auto &g : groups)
        for (size_t o = 0; o < g.size(); o += target) split.emplace_back(g.begin() + o, g.begin() + std::min(g.size(), o + target));
    // The call's FIRST upload overlaps nothing, so its chunks start small and double up to the target (an upload costs
    // about half of the same pairs' kernels, so each chunk's kernels still cover the next one's upload).
    const bool several = n > target;
    size_t limit = (several && in.ramp && ring == 0) ? std::min(in.ramp, target) : target;
    const size_t bucket_begin = plan.size();
    for (size_t g0 = 0, g1 = 0; g0 < split.size(); g0 = g1) {
        size_t count = 0;
        // (g1 - g0 references so far; a part is at most `target` pairs, so the chunk's first part always fits the launch)
        while (g1 < split.size() && (count == 0 || (count + split[g1].size() <= limit &&
                                                    count + split[g1].size() + (g1 - g0) + 1 <= in.max_slots)))
            count += split[g1++].size();
        limit = std::min(target, limit * 2);
        // several chunks: every ring slot is sized for the target, so that a later, larger chunk does not reallocate it
        ce_plan_chunk c{ring++ % ce_plan_ring_slots, (uint32_t)(several ? std::max(count, target) : count), ce_plan_none,
                        std::vector<std::vector<size_t>>(split.begin() + g0, split.begin() + g1)};
        for (size_t p = bucket_begin; p < plan.size(); p++)
            if (plan[p].slot == c.slot) c.collect_first = p;  // the latest one; the earlier ones it collected itself
        plan.push_back(std::move(c));
    }
}

// XCD-aware 1-D launch order for per-pair tile kernels.  Workgroups reach the 8 XCDs round-robin by launch id and every
// XCD has its own L2, so the workgroups that read the same part of one REFERENCE for its different distorted images
// should carry ids that are congruent mod 8 and adjacent: the reference's data is then fetched into one XCD's L2 once and
// hit there by the reference's other pairs.  The keys of each reference that has pairs are dealt to the 8 classes in
// turn; a key is followed by its tiles and each tile by all pairs of its reference.  Entry id = slot * 8 + class; every
// class is padded to one length, a multiple of round_to, with (~0u, 0) entries (the kernel returns at once).
struct ce_plan_entry {  // (tile, pair): the layout of HIP's uint2, which the kernels read
    uint32_t tile, pair;
};

struct ce_xcd_keys {
    uint32_t channels;          // a reference has channels * keys_per_channel keys, channel-major
    uint32_t keys_per_channel;
    uint32_t tiles_per_key;     // key j of channel c covers the tiles (j * tiles_per_key + sub) | c << 16
    uint32_t round_to = 1;      // a block takes round_to consecutive entries of one class
};

inline bool operator==(const ce_xcd_keys &a, const ce_xcd_keys &b)
{
    return a.channels == b.channels && a.keys_per_channel == b.keys_per_channel && a.tiles_per_key == b.tiles_per_key &&
           a.round_to == b.round_to;
}

// The list of pairs [0, n_pairs); pair_ref[p] < n_refs is the reference of pair p.
inline std::vector<ce_plan_entry> ce_plan_xcd_list(const uint32_t *pair_ref, uint32_t n_pairs, uint32_t n_refs, const ce_xcd_keys &k)
{
    std::vector<std::vector<uint32_t>> pairs_of(n_refs);
    for (uint32_t p = 0; p < n_pairs; p++) pairs_of[pair_ref[p]].push_back(p);
    std::vector<ce_plan_entry> cls[8];
    uint32_t key = 0;
    for (const auto &pairs : pairs_of) {
        if (pairs.empty()) continue;
        for (uint32_t c = 0; c < k.channels; c++)
            for (uint32_t j = 0; j < k.keys_per_channel; j++, key++)
                for (uint32_t sub = 0; sub < k.tiles_per_key; sub++)
                    for (uint32_t p : pairs) cls[key & 7].push_back({(j * k.tiles_per_key + sub) | c << 16, p});
    }
    size_t len = 0;
    for (const auto &v : cls) len = std::max(len, v.size());
    len = (len + k.round_to - 1) / k.round_to * k.round_to;
    std::vector<ce_plan_entry> list(len * 8, ce_plan_entry{~0u, 0u});
    for (uint32_t x = 0; x < 8; x++)
        for (size_t i = 0; i < cls[x].size(); i++) list[i * 8 + x] = cls[x][i];
    return list;
}

// Which blur passes an SSIMULACRA2 launch runs.  A reference's own streams mu1 = blur(a), s11 = blur(a*a) do not depend on
// the distorted image: the split path keeps them as final planes per reference and the pair passes filter only the three
// streams that involve the distorted image.  It runs when the planes' record covers the launch's references, or when they
// can be built and amortised.  Building costs about four launches' worth of what a launch then saves, so it must be
// followed by launches that reuse the planes: the batch keeps reference state, the launch has more pairs than references,
// and the launch itself REUSED the references' XYB pyramid (`reused`) - the references have outlived a launch, the one
// sign a batch gives that they stay.  A batch's first launch, and every launch of a batch whose references are written
// before each one (ce_eval_batch's pooled batches), therefore run the passes as they always were.  A reference handle's
// batch builds without waiting: staying is what a handle is.  A launch with one pair per reference and nothing to reuse -
// ce_eval_pair, the one-pair leaves - also keeps the passes as they were: the build would put four dependent launches in
// front of its own.  enabled = false (CE_SSIM2_REF_BLUR=0): always those.
enum { CE_SSIM2_BLUR_TODAY = 0, CE_SSIM2_BLUR_SPLIT = 1, CE_SSIM2_BLUR_SPLIT_BUILD = 2 };

inline int ce_plan_ssim2_ref_blur(bool enabled, bool keeps_state, bool handle, bool reused, bool covered, uint32_t n_pairs,
                                  uint32_t n_refs)
{
    if (!enabled || !keeps_state) return CE_SSIM2_BLUR_TODAY;  // a batch that keeps nothing has no record to be covered by
    if (covered) return CE_SSIM2_BLUR_SPLIT;
    if (handle) return CE_SSIM2_BLUR_SPLIT_BUILD;
    return (reused && n_pairs > n_refs) ? CE_SSIM2_BLUR_SPLIT_BUILD : CE_SSIM2_BLUR_TODAY;
}

// Where a Butteraugli launch forms the LF term of CombineChannelsToDiffmap, mc_dc = sum over c of (lf_ref[c] - lf_dist[c])^2 *
// w[c] * dc_maskval.  Both of its reference operands - the reference's LF planes and dc_maskval - are state that a launch
// which found its references kept (`cached`) has in place before its first kernel: there the LF column blur forms the term
// where the distorted LF is still in registers and writes one plane per distorted slot instead of three, and Malta's epilogue
// reads that plane.  A batch's first launch, ce_eval_batch's pooled batches and everything else that rebuilds its references
// makes the mask values AFTER the blurs, so it keeps the term in Malta's epilogue.  enabled = false (CE_BA_LF_TERM=0):
// always there.
inline bool ce_plan_ba_lf_term_in_blur(bool enabled, bool cached) { return enabled && cached; }

// DSSIM's scale pyramid (Dssim::create_image, make_scales_recursive): level 0 is the image, and a level is halved (floor)
// into the next only while it is at least 8 x 8, up to max_levels levels.  Writes the level sizes, returns their count (0
// for an empty image).  The one rule of dssim.hip's working set and of ce_dssim_levels.
inline uint32_t ce_plan_dssim_levels(uint32_t w, uint32_t h, uint32_t max_levels, uint32_t *level_w, uint32_t *level_h)
{
    if (w == 0 || h == 0) return 0;
    uint32_t n = 0;
    while (n < max_levels) {
        level_w[n] = w;
        level_h[n] = h;
        n++;
        if (w < 8 || h < 8) break;
        w /= 2;
        h /= 2;
    }
    return n;
}

// SSIMULACRA2's scale pyramid (Msssim's loop in the lineage): `if w < 8 || h < 8 {break}; if scale > 0 {downscale}` - the
// size is tested BEFORE halving (with ceiling), so a scale smaller than 8 px exists whenever its parent was >= 8; at most
// max_scales scales.  Writes the scale sizes, returns their count (0 below 8 x 8).  The one rule of ssim2.hip's working set
// and of ce_ssimulacra2_scales.
inline uint32_t ce_plan_ssim2_scales(uint32_t w, uint32_t h, uint32_t max_scales, uint32_t *scale_w, uint32_t *scale_h)
{
    uint32_t n = 0;
    for (uint32_t s = 0; s < max_scales; s++) {
        if (w < 8 || h < 8) break;
        if (s > 0) {
            w = w / 2 + (w & 1);
            h = h / 2 + (h & 1);
        }
        scale_w[n] = w;
        scale_h[n] = h;
        n++;
    }
    return n;
}
