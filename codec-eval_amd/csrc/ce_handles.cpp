// The handles a slot write takes beside its pixels (include/ce_metrics.h: ce_lut_*, ce_icc_create, ce_icc_lut_create,
// ce_icc_destroy): their device tables are built here once and are read-only from then on, so ce_ingest.cpp only reads them.
// The parsers are pure host code in ce_icc.cpp and ce_icc_lut.cpp; all device work is in the .hip files.
#include <string>
#include <vector>

#include "ce_internal.h"

extern "C" {

// ICC -> sRGB colour tables: [2^24] r | g << 8 | b << 16 on the device (struct ce_lut, ce_internal.h)
int ce_lut_create(ce_ctx *ctx, const uint8_t *table, size_t table_len, ce_lut **out)
{
    if (!ctx || !table || !out) return CE_ERR_INVALID_ARG;
    *out = nullptr;
    const size_t want = (size_t)3 << 24;
    if (table_len != want)
        return ce_fail(ctx, CE_ERR_BAD_LENGTH, "Invalid colour table size: expected " + std::to_string(want) + " bytes, got " + std::to_string(table_len));
    CE_HIP(ctx, hipSetDevice(ctx->device));
    uint8_t *d_packed = nullptr;
    uint32_t *d_table = nullptr;
    CE_HIP(ctx, hipMalloc(&d_packed, want));
    if (hipMalloc(&d_table, sizeof(uint32_t) << 24) != hipSuccess) {
        hipFree(d_packed);
        return ce_fail(ctx, CE_ERR_BACKEND, "hipMalloc failed (colour table)");
    }
    int rc = CE_OK;
    if (hipMemcpyAsync(d_packed, table, want, hipMemcpyHostToDevice, ctx->stream) != hipSuccess) rc = ce_fail(ctx, CE_ERR_BACKEND, "H2D failed (colour table)");
    if (rc == CE_OK) rc = ce_launch_lut_expand(ctx, ctx->stream, d_packed, d_table);
    if (rc == CE_OK && hipStreamSynchronize(ctx->stream) != hipSuccess) rc = ce_fail(ctx, CE_ERR_BACKEND, "sync failed (colour table)");
    hipFree(d_packed);
    if (rc != CE_OK) {
        hipFree(d_table);
        return rc;
    }
    *out = new ce_lut{ctx, d_table};
    return CE_OK;
}

void ce_lut_destroy(ce_lut *lut)
{
    if (!lut) return;
    hipSetDevice(lut->ctx->device);
    hipStreamSynchronize(lut->ctx->stream);
    hipFree(lut->d_table);
    delete lut;
}

// matrix/TRC ICC profiles; the pure host functions are in ce_icc.cpp
int ce_icc_create(ce_ctx *ctx, const uint8_t *bytes, size_t len, ce_icc **out)
{
    if (!ctx || !out) return CE_ERR_INVALID_ARG;
    *out = nullptr;
    if (!bytes) return ce_fail(ctx, CE_ERR_INVALID_ARG, "ICC profile: null pointer");
    ce_icc_description d;
    ce_icc_describe(bytes, len, &d);
    if (d.kind != CE_ICC_SUPPORTED) {
        static const char *const kKinds[4] = {"", "a LUT-based profile", "not an RGB profile with an XYZ connection space", "a malformed profile"};
        return ce_fail(ctx, CE_ERR_INVALID_ARG, std::string("ICC profile: ") + kKinds[d.kind & 3] + " (" + d.reason + ")");
    }
    ce_icc *icc = new ce_icc{ctx, {}, false, {}};
    ce_icc_build_matrix(bytes, len, icc->m);
    for (int i = 0; i < 9; i++) icc->has_matrix |= icc->m[i] != ((i % 4 == 0) ? 1.0f : 0.0f);
    // the tone tables of all four source depths now (0.85 MB of device memory in all): the handle is read-only from here on
    int rc = hipSetDevice(ctx->device) == hipSuccess ? CE_OK : ce_fail(ctx, CE_ERR_BACKEND, "hipSetDevice failed (ICC profile)");
    for (uint32_t depth : {8u, 10u, 12u, 16u}) {
        if (rc != CE_OK) break;
        std::vector<float> host((size_t)3 << depth);
        ce_icc_build_tables(bytes, len, depth, host.data(), host.size());
        void *d = nullptr;
        rc = ce_device_table(ctx, host.data(), host.size() * sizeof(float), "ICC tone tables", &d);
        icc->d_tables[ce_icc_depth_index(depth)] = static_cast<float *>(d);
    }
    if (rc != CE_OK) {
        for (float *t : icc->d_tables) hipFree(t);
        delete icc;
        return rc;
    }
    *out = icc;
    return CE_OK;
}

// what both flavours of handle own
static void icc_free(ce_icc *icc)
{
    for (float *t : icc->d_tables) hipFree(t);
    if (icc->lut) {
        hipFree(icc->lut->d_clut);
        hipFree(icc->lut->d_samples);
        delete icc->lut;
    }
    delete icc;
}

void ce_icc_destroy(ce_icc *icc)
{
    if (!icc) return;
    hipSetDevice(icc->ctx->device);
    hipDeviceSynchronize();  // the batches' upload streams may still gather from the tables
    icc_free(icc);
}

// LUT-based ICC profiles; the pure host functions are in ce_icc_lut.cpp
int ce_icc_lut_create(ce_ctx *ctx, const uint8_t *bytes, size_t len, int intent, int interpolation, ce_icc **out)
{
    if (!ctx || !out) return CE_ERR_INVALID_ARG;
    *out = nullptr;
    if (!bytes) return ce_fail(ctx, CE_ERR_INVALID_ARG, "ICC profile: null pointer");
    if (intent < 0 || intent > 2) return ce_fail(ctx, CE_ERR_INVALID_ARG, "ICC profile: intent must be 0, 1 or 2, got " + std::to_string(intent));
    if (interpolation != CE_ICC_CLUT_TRILINEAR && interpolation != CE_ICC_CLUT_TETRAHEDRAL)
        return ce_fail(ctx, CE_ERR_INVALID_ARG, "ICC profile: interpolation must be CE_ICC_CLUT_TRILINEAR or CE_ICC_CLUT_TETRAHEDRAL");
    ce_icc_lut_description d;
    ce_icc_lut_describe(bytes, len, intent, &d);
    if (d.kind != CE_ICC_LUT_SUPPORTED) {
        static const char *const kKinds[4] = {"", "not a LUT-based profile", "a LUT-based profile of a kind not taken", "a malformed profile"};
        return ce_fail(ctx, CE_ERR_INVALID_ARG, std::string("ICC profile: ") + kKinds[d.kind & 3] + " (" + d.reason + ")");
    }
    ce_icc *icc = new ce_icc{ctx, {}, true, {}};
    ce_icc_lut *lut = icc->lut = new ce_icc_lut{};
    ce_icc_lut_build_pcs_matrix(icc->m);
    lut->tetra = interpolation == CE_ICC_CLUT_TETRAHEDRAL;
    lut->has_matrix = (d.stages & CE_ICC_STAGE_MATRIX) != 0;
    ce_icc_lut_build_matrix(bytes, len, intent, lut->mat);
    constexpr uint32_t kLab = 0x4c616220u, kMft2 = 0x6d667432u;  // 'Lab ', 'mft2'
    lut->pcs = d.pcs != kLab ? 0u : d.tag_type == kMft2 ? 2u : 1u;
    for (int k = 0; k < 3; k++) lut->grid[k] = d.grid[k];
    // everything the kernel gathers from now (the input tables of all four depths, 0.85 MB; the CLUT, 16 bytes a node; the
    // sampled curves): the handle is read-only from here on
    int rc = hipSetDevice(ctx->device) == hipSuccess ? CE_OK : ce_fail(ctx, CE_ERR_BACKEND, "hipSetDevice failed (ICC profile)");
    for (uint32_t depth : {8u, 10u, 12u, 16u}) {
        if (rc != CE_OK) break;
        std::vector<float> host((size_t)3 << depth);
        ce_icc_lut_build_input_tables(bytes, len, intent, depth, host.data(), host.size());
        void *p = nullptr;
        rc = ce_device_table(ctx, host.data(), host.size() * sizeof(float), "ICC input tables", &p);
        icc->d_tables[ce_icc_depth_index(depth)] = static_cast<float *>(p);
    }
    if (rc == CE_OK && (d.stages & CE_ICC_STAGE_CLUT)) {
        std::vector<float> host((size_t)d.grid[0] * d.grid[1] * d.grid[2] * 4);
        ce_icc_lut_build_clut(bytes, len, intent, host.data(), host.size());
        void *p = nullptr;
        rc = ce_device_table(ctx, host.data(), host.size() * sizeof(float), "ICC CLUT", &p);
        lut->d_clut = static_cast<float *>(p);
    }
    if (rc == CE_OK) {
        size_t needed = 0;
        ce_icc_lut_build_curves(bytes, len, intent, lut->curves, nullptr, 0, &needed);
        std::vector<float> host(needed);
        ce_icc_lut_build_curves(bytes, len, intent, lut->curves, host.data(), host.size(), &needed);
        if (needed) {
            void *p = nullptr;
            rc = ce_device_table(ctx, host.data(), host.size() * sizeof(float), "ICC curve samples", &p);
            lut->d_samples = static_cast<float *>(p);
        }
    }
    if (rc != CE_OK) {
        icc_free(icc);
        return rc;
    }
    *out = icc;
    return CE_OK;
}

}  // extern "C"
