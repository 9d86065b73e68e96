// What a batch keeps of its references between launches, plain C++ without device calls, checked on the host by
// tests/cpp/test_ref_state.cpp.  Every metric builds planes that depend on the references alone (SSIMULACRA2's XYB pyramid,
// DSSIM's img / mu / sq pyramid, Butteraugli's PsychoImage, mask input and mask values; the XYB roundtrip of the slab
// itself); a launch that finds them covering what it needs skips the reference slots of its per-slot kernels (their z0
// argument).  The record says what the planes on the device were built from; the planes themselves are the batch's.
#pragma once

#include <cstdint>
#include <cstring>

// the records of a batch: the three metric chains in ce_batch_launch's order, then the roundtripped slab (d_refs_rt), then
// SSIMULACRA2's final reference planes mu1 / s11 (marked and invalidated like CE_REF_SSIM2: same slab, count and scale count;
// not a chain of its own, so it does not count in builds[])
enum { CE_REF_SSIM2 = 0, CE_REF_DSSIM = 1, CE_REF_BUTTERAUGLI = 2, CE_REF_ROUNDTRIP = 3, CE_REF_SSIM2_BLUR = 4, CE_REF_KINDS = 5 };

// the bits of a float parameter (Butteraugli's intensity target): equal bits, equal planes
inline uint64_t ce_ref_param_f32(float v)
{
    uint32_t u;
    std::memcpy(&u, &v, sizeof(u));
    return u;
}

struct ce_ref_state {
    const void *src = nullptr;  // the reference slab the planes were built from (d_refs or d_refs_rt); nullptr: nothing valid
    uint32_t count = 0;         // references [0, count) are covered
    uint64_t param = 0;         // what else the planes depend on: SSIMULACRA2's scale count, the bits of the intensity target
    bool covers(const void *slab, uint32_t n_refs, uint64_t p) const { return src && src == slab && n_refs <= count && param == p; }
    void invalidate() { src = nullptr, count = 0, param = 0; }
    void mark(const void *slab, uint32_t n_refs, uint64_t p) { src = slab, count = n_refs, param = p; }
};

struct ce_ref_states {
    // reuse at all?  Every batch does unless CE_KEEP_REFERENCE_STATE=0 (then only a reference handle's batch does)
    bool keep = true;
    ce_ref_state of[CE_REF_KINDS];
    // launches in which the reference-side state of [SSIMULACRA2, DSSIM, Butteraugli] was (re)built (ce_batch_ref_stats)
    uint32_t builds[3] = {0, 0, 0};

    // The first thing a launch asks: true - record k covers references [0, n_refs) of `slab` at `p`, skip their slots.
    // false - they are rebuilt: the build is counted and the record dropped, so a launch that fails half way leaves nothing
    // valid; built() follows once the whole chain has been enqueued without error.
    bool reuse(int k, const void *slab, uint32_t n_refs, uint64_t p)
    {
        if (keep && of[k].covers(slab, n_refs, p)) return true;
        of[k].invalidate();
        if (k < 3) builds[k]++;
        return false;
    }
    void built(int k, const void *slab, uint32_t n_refs, uint64_t p) { of[k].mark(slab, n_refs, p); }
    // a reference was, or may have been, written: everything derived from the slab goes
    void invalidate()
    {
        for (auto &s : of) s.invalidate();
    }
};
