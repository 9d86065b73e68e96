// The reference-state records of codec-eval_amd/csrc/ce_ref_state.h on the rules a launch relies on.  No device.
#include <cstdio>
#include <cstdlib>

#include "ce_ref_state.h"

#define CHECK(cond)                                                         \
    do {                                                                    \
        if (!(cond)) {                                                      \
            std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond); \
            std::exit(1);                                                   \
        }                                                                   \
    } while (0)

int main()
{
    unsigned char slab[4], roundtripped[4];
    const uint64_t t80 = ce_ref_param_f32(80.0f), t250 = ce_ref_param_f32(250.0f);
    CHECK(t80 != t250 && ce_ref_param_f32(80.0f) == t80);

    // one record: nothing is covered before a build, a build covers its slab, its count and fewer, at its parameter only
    ce_ref_state s;
    CHECK(!s.covers(slab, 0, 0) && !s.covers(slab, 1, 0) && !s.covers(nullptr, 0, 0));
    s.mark(slab, 3, 6);
    CHECK(s.covers(slab, 3, 6) && s.covers(slab, 2, 6) && s.covers(slab, 1, 6));
    CHECK(!s.covers(slab, 4, 6));          // more references than were built
    CHECK(!s.covers(slab, 3, 5));          // another scale count
    CHECK(!s.covers(roundtripped, 3, 6));  // another source slab
    s.invalidate();
    CHECK(!s.covers(slab, 1, 6) && s.src == nullptr && s.count == 0 && s.param == 0);

    // a batch: a metric that has not run builds on its first launch; the same launch again reuses
    ce_ref_states r;
    CHECK(r.keep);
    for (int k = 0; k < 3; k++) {
        const uint64_t p = k == CE_REF_SSIM2 ? 6 : k == CE_REF_BUTTERAUGLI ? t80 : 0;
        CHECK(!r.reuse(k, slab, 3, p));
        CHECK(r.builds[k] == 1);
        CHECK(!r.of[k].covers(slab, 3, p));  // not valid before the chain is enqueued: a failed launch leaves nothing behind
        r.built(k, slab, 3, p);
        CHECK(r.reuse(k, slab, 3, p) && r.builds[k] == 1);
    }
    // a launch that failed half way: reuse() said rebuild, built() never came
    CHECK(!r.reuse(CE_REF_DSSIM, slab, 4, 0) && r.builds[1] == 2);
    CHECK(!r.reuse(CE_REF_DSSIM, slab, 3, 0) && r.builds[1] == 3);  // ... so even what was covered before is rebuilt
    r.built(CE_REF_DSSIM, slab, 3, 0);
    // shrinking reuses, growing rebuilds and then covers the larger count
    CHECK(r.reuse(CE_REF_SSIM2, slab, 2, 6) && r.builds[0] == 1);
    CHECK(!r.reuse(CE_REF_SSIM2, slab, 4, 6) && r.builds[0] == 2);
    r.built(CE_REF_SSIM2, slab, 4, 6);
    CHECK(r.reuse(CE_REF_SSIM2, slab, 3, 6) && r.reuse(CE_REF_SSIM2, slab, 4, 6) && r.builds[0] == 2);
    // another intensity target rebuilds Butteraugli only, and going back rebuilds again (one record, one target)
    CHECK(!r.reuse(CE_REF_BUTTERAUGLI, slab, 3, t250) && r.builds[2] == 2);
    r.built(CE_REF_BUTTERAUGLI, slab, 3, t250);
    CHECK(r.reuse(CE_REF_DSSIM, slab, 3, 0) && r.reuse(CE_REF_SSIM2, slab, 3, 6) && r.builds[0] == 2 && r.builds[1] == 3);
    CHECK(!r.reuse(CE_REF_BUTTERAUGLI, slab, 3, t80) && r.builds[2] == 3);
    r.built(CE_REF_BUTTERAUGLI, slab, 3, t80);
    // another scale limit rebuilds SSIMULACRA2 only
    CHECK(!r.reuse(CE_REF_SSIM2, slab, 3, 1) && r.builds[0] == 3 && r.reuse(CE_REF_DSSIM, slab, 3, 0));
    r.built(CE_REF_SSIM2, slab, 3, 1);
    // the roundtrip flag: the roundtripped slab is built (not counted: it is no metric), the metrics see another source
    CHECK(!r.reuse(CE_REF_ROUNDTRIP, slab, 3, 0));
    r.built(CE_REF_ROUNDTRIP, slab, 3, 0);
    CHECK(r.builds[0] == 3 && r.builds[1] == 3 && r.builds[2] == 3);
    CHECK(!r.reuse(CE_REF_DSSIM, roundtripped, 3, 0) && r.builds[1] == 4);
    r.built(CE_REF_DSSIM, roundtripped, 3, 0);
    CHECK(r.reuse(CE_REF_ROUNDTRIP, slab, 3, 0) && r.reuse(CE_REF_DSSIM, roundtripped, 3, 0));
    CHECK(!r.reuse(CE_REF_DSSIM, slab, 3, 0) && r.builds[1] == 5);  // flag off again
    r.built(CE_REF_DSSIM, slab, 3, 0);
    CHECK(r.reuse(CE_REF_ROUNDTRIP, slab, 3, 0));                   // the roundtripped slab itself is still good
    // writing a reference drops everything, the counters stay
    r.invalidate();
    for (int k = 0; k < CE_REF_KINDS; k++) CHECK(!r.of[k].covers(slab, 0, 0) && !r.of[k].covers(roundtripped, 0, 0));
    CHECK(r.builds[0] == 3 && r.builds[1] == 5 && r.builds[2] == 3);
    CHECK(!r.reuse(CE_REF_SSIM2, slab, 3, 1) && r.builds[0] == 4);
    r.built(CE_REF_SSIM2, slab, 3, 1);

    // keep = false (CE_KEEP_REFERENCE_STATE=0): every launch rebuilds and counts, whatever built() recorded
    ce_ref_states off;
    off.keep = false;
    for (uint32_t n = 1; n <= 3; n++) {
        CHECK(!off.reuse(CE_REF_DSSIM, slab, 2, 0) && off.builds[1] == n);
        off.built(CE_REF_DSSIM, slab, 2, 0);
    }
    std::puts("ref state OK");
    return 0;
}
