// What the calls that score a decoder's planes where they lie share on the host (plane_fidelity.hip: ce_yuv_plane_fidelity;
// plane_hvs.hip: ce_yuv_plane_hvs): the checks of the pair table and of the images, the planes' sizes, and the upload - host
// planes without their pitch padding through the context's page-locked staging into its grow-only scratch, the plane table
// with the pair table and whatever constants the call adds behind it.  `what` opens every reason ("plane fidelity", "plane
// hvs").  Included after the kernel header that defines pf_plane.
#pragma once

#include <cstring>
#include <string>
#include <vector>

#include "ce_internal.h"

namespace {

struct pf_images {
    uint32_t n_refs = 0, n_pairs = 0, n_planes = 0, depth = 8, bps = 1, maxv = 255;
    uint32_t pw[3] = {}, ph[3] = {};  // the planes' sizes
    std::vector<ce_yuv_planes> plans;  // the references', then the tests'
    std::vector<uint32_t> ref_of;      // pair -> reference
    // after pf_upload
    const pf_plane *d_tab = nullptr;
    const uint32_t *d_pair_ref = nullptr;
    const uint8_t *d_extra = nullptr;
};

inline size_t pf_round_up(size_t v, size_t to) { return (v + to - 1) / to * to; }

// the pointers, the counts and the pair table
inline int pf_check_pairs(ce_ctx *ctx, const char *what, const ce_yuv_image *refs, uint32_t n_refs, const ce_yuv_image *tests, uint32_t n_pairs,
                          const uint32_t *pair_ref, const void *out)
{
    const auto bad = [&](const std::string &why) { return ce_fail(ctx, CE_ERR_INVALID_ARG, std::string(what) + ": " + why); };
    if (!refs || !tests || !out) return bad("null pointer");
    if (n_refs == 0 || n_pairs == 0) return bad("no references or no pairs");
    if (!pair_ref && n_refs != n_pairs)
        return bad("without a pair table pair i scores against reference i: " + std::to_string(n_refs) + " references for " + std::to_string(n_pairs) + " pairs");
    for (uint32_t i = 0; pair_ref && i < n_pairs; i++)
        if (pair_ref[i] >= n_refs)
            return bad("pair " + std::to_string(i) + " names reference " + std::to_string(pair_ref[i]) + " of " + std::to_string(n_refs));
    return CE_OK;
}

// the images: the ingest's checks, one subsampling and one depth a call, one matrix and one range a pair
inline int pf_check_images(ce_ctx *ctx, const char *what, uint32_t width, uint32_t height, const ce_yuv_image *refs, uint32_t n_refs,
                           const ce_yuv_image *tests, uint32_t n_pairs, const uint32_t *pair_ref, pf_images *out)
{
    const auto bad = [&](const std::string &why) { return ce_fail(ctx, CE_ERR_INVALID_ARG, std::string(what) + ": " + why); };
    if (width == 0 || height == 0) return bad("empty image");
    const size_t n_img = (size_t)n_refs + n_pairs;
    const auto image = [&](size_t i) -> const ce_yuv_image & { return i < n_refs ? refs[i] : tests[i - n_refs]; };
    out->plans.resize(n_img);
    for (size_t i = 0; i < n_img; i++) {
        if (int rc = ce_yuv_planes_check(ctx, &image(i), width, height, &out->plans[i])) return rc;
        if (image(i).subsampling != refs[0].subsampling || image(i).depth != refs[0].depth)
            return bad(std::string(i < n_refs ? "reference " : "test ") + std::to_string(i < n_refs ? i : i - n_refs) +
                       " differs from reference 0 in subsampling or depth: every image of a call has one of each");
    }
    out->ref_of.resize(n_pairs);
    for (uint32_t i = 0; i < n_pairs; i++) {
        out->ref_of[i] = pair_ref ? pair_ref[i] : i;
        if (tests[i].matrix != refs[out->ref_of[i]].matrix || tests[i].range != refs[out->ref_of[i]].range)
            return bad("pair " + std::to_string(i) + ": the two sides differ in matrix or range, their code values do not mean the same");
    }
    out->n_refs = n_refs, out->n_pairs = n_pairs;
    const int sub = refs[0].subsampling;
    out->n_planes = sub == CE_YUV_400 ? 1 : 3;
    out->depth = refs[0].depth, out->bps = refs[0].depth == 8 ? 1 : 2, out->maxv = (1u << refs[0].depth) - 1u;
    const uint32_t cw = sub == CE_YUV_444 ? width : (uint32_t)(((size_t)width + 1) / 2), ch = sub == CE_YUV_420 ? (uint32_t)(((size_t)height + 1) / 2) : height;
    for (uint32_t p = 0; p < out->n_planes; p++) out->pw[p] = p ? cw : width, out->ph[p] = p ? ch : height;
    return CE_OK;
}

// Queues the call's inputs on the context's stream: host planes without their pitch padding (rows 16 bytes apart at least, so
// that a wide path reads them), then the plane table - device planes where they lie, host planes where their copy will be -
// with the pair table and `extra` (16-byte aligned) behind it.  The caller has set the device.
inline int pf_upload(ce_ctx *ctx, pf_images &j, const ce_yuv_image *refs, const ce_yuv_image *tests, const void *extra = nullptr, size_t extra_bytes = 0)
{
    const size_t n_img = (size_t)j.n_refs + j.n_pairs;
    const auto image = [&](size_t i) -> const ce_yuv_image & { return i < j.n_refs ? refs[i] : tests[i - j.n_refs]; };
    size_t stage = 0;
    for (size_t i = 0; i < n_img; i++)
        if (image(i).memory == CE_MEM_HOST)
            for (int s = 0; s < j.plans[i].n_stored; s++) stage += pf_round_up(pf_round_up(j.plans[i].row_bytes[s], 16) * j.plans[i].rows[s], 256);
    const size_t tab_bytes = pf_round_up(n_img * 3 * sizeof(pf_plane), 16), pairs_bytes = sizeof(uint32_t) * j.n_pairs;
    const size_t extra_at = pf_round_up(tab_bytes + pairs_bytes, 16), tables = extra_bytes ? extra_at + extra_bytes : tab_bytes + pairs_bytes;
    if (int rc = ctx->pf_planes_h.reserve(ctx, stage)) return rc;
    if (int rc = ctx->pf_planes_d.reserve(ctx, stage)) return rc;
    if (int rc = ctx->pf_tables_h.reserve(ctx, tables)) return rc;
    if (int rc = ctx->pf_tables_d.reserve(ctx, tables)) return rc;
    pf_plane *tab = reinterpret_cast<pf_plane *>(ctx->pf_tables_h.get());
    size_t at = 0;
    for (size_t i = 0; i < n_img; i++) {
        const ce_yuv_image &img = image(i);
        const uint8_t *base[3] = {};
        size_t pitch[3] = {};
        for (int s = 0; s < j.plans[i].n_stored; s++) {
            base[s] = static_cast<const uint8_t *>(img.plane[s]), pitch[s] = img.pitch[s];
            if (img.memory != CE_MEM_HOST) continue;
            const size_t row = j.plans[i].row_bytes[s], to = pf_round_up(row, 16);
            uint8_t *dst = ctx->pf_planes_h.get() + at;
            for (size_t r = 0; r < j.plans[i].rows[s]; r++) std::memcpy(dst + r * to, base[s] + r * pitch[s], row);
            base[s] = ctx->pf_planes_d.get() + at, pitch[s] = to;
            at += pf_round_up(to * j.plans[i].rows[s], 256);
        }
        const bool semi = img.layout == CE_YUV_SEMIPLANAR;
        for (uint32_t p = 0; p < 3; p++) {
            pf_plane e{};
            if (p < j.n_planes) {
                const int s = semi && p == 2 ? 1 : (int)p;
                e.base = base[s] + (semi && p == 2 ? j.bps : 0), e.pitch = pitch[s], e.step = semi && p ? 2 : 1, e.shift = j.plans[i].shift;
            }
            tab[i * 3 + p] = e;
        }
    }
    std::memcpy(ctx->pf_tables_h.get() + tab_bytes, j.ref_of.data(), pairs_bytes);
    if (extra_bytes) std::memcpy(ctx->pf_tables_h.get() + extra_at, extra, extra_bytes);
    if (stage) CE_HIP(ctx, hipMemcpyAsync(ctx->pf_planes_d.get(), ctx->pf_planes_h.get(), stage, hipMemcpyHostToDevice, ctx->stream));
    CE_HIP(ctx, hipMemcpyAsync(ctx->pf_tables_d.get(), ctx->pf_tables_h.get(), tables, hipMemcpyHostToDevice, ctx->stream));
    j.d_tab = reinterpret_cast<const pf_plane *>(ctx->pf_tables_d.get());
    j.d_pair_ref = reinterpret_cast<const uint32_t *>(ctx->pf_tables_d.get() + tab_bytes);
    j.d_extra = extra_bytes ? ctx->pf_tables_d.get() + extra_at : nullptr;
    return CE_OK;
}

}  // namespace
