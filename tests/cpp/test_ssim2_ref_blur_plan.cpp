// Which blur passes an SSIMULACRA2 launch runs (codec-eval_amd/csrc/ce_plan.h: ce_plan_ssim2_ref_blur) over a grid of
// (keeps state, handle, reused, covered, pairs, references), and the record of the references' final planes
// (ce_ref_state.h: CE_REF_SSIM2_BLUR) beside the chains' records.  No device.
#include <cstdio>
#include <cstdlib>

#include "ce_plan.h"
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
    // The rule in words, written down apart from the implementation: the split path runs when the planes are there
    // (covered), or when they can be built and amortised; everything else keeps the unsplit passes.  "Built and amortised":
    // a handle always; any other batch only if it keeps state, the launch found its references kept from an earlier launch
    // (reused) and it has more pairs than references.  Nothing of this holds with the knob off or for a batch that keeps
    // nothing.  The grid counts, per outcome, the combinations that must give it.
    const uint32_t counts[] = {1, 2, 3, 6, 8, 54, 432};
    int n_today = 0, n_split = 0, n_build = 0;
    for (int keeps = 0; keeps < 2; keeps++)
        for (int handle = 0; handle < 2; handle++)
            for (int reused = 0; reused < 2; reused++)
                for (int covered = 0; covered < 2; covered++)
                    for (uint32_t pairs : counts)
                        for (uint32_t refs : counts) {
                            if (refs > pairs) continue;  // every used reference has a pair
                            CHECK(ce_plan_ssim2_ref_blur(false, keeps, handle, reused, covered, pairs, refs) == CE_SSIM2_BLUR_TODAY);
                            const int got = ce_plan_ssim2_ref_blur(true, keeps, handle, reused, covered, pairs, refs);
                            const bool planes_there = keeps && covered;
                            const bool amortised = keeps && (handle || (reused && pairs > refs));
                            const bool runs_split = planes_there || amortised;
                            CHECK((got != CE_SSIM2_BLUR_TODAY) == runs_split);
                            CHECK((got == CE_SSIM2_BLUR_SPLIT_BUILD) == (runs_split && !planes_there));  // builds exactly what is missing
                            if (!keeps) CHECK(got == CE_SSIM2_BLUR_TODAY);
                            if (pairs == refs && !handle && !covered) CHECK(got == CE_SSIM2_BLUR_TODAY);  // one pair per reference, nothing to reuse
                            if (!reused && !handle && !covered) CHECK(got == CE_SSIM2_BLUR_TODAY);        // a first launch, a pooled batch
                            n_today += got == CE_SSIM2_BLUR_TODAY, n_split += got == CE_SSIM2_BLUR_SPLIT, n_build += got == CE_SSIM2_BLUR_SPLIT_BUILD;
                        }
    CHECK(n_today > 0 && n_split > 0 && n_build > 0);
    // the cases by name (enabled, keeps, handle, reused, covered, pairs, references)
    CHECK(ce_plan_ssim2_ref_blur(true, true, false, false, false, 1, 1) == CE_SSIM2_BLUR_TODAY);          // ce_eval_pair, the one-pair leaves
    CHECK(ce_plan_ssim2_ref_blur(true, true, false, true, false, 54, 54) == CE_SSIM2_BLUR_TODAY);         // one pair per reference, relaunched
    CHECK(ce_plan_ssim2_ref_blur(true, true, false, false, false, 432, 54) == CE_SSIM2_BLUR_TODAY);       // the sweep's first launch; ce_eval_batch's pooled batch, every launch
    CHECK(ce_plan_ssim2_ref_blur(true, true, false, true, false, 432, 54) == CE_SSIM2_BLUR_SPLIT_BUILD);  // ... its second launch on the same references
    CHECK(ce_plan_ssim2_ref_blur(true, true, false, true, true, 432, 54) == CE_SSIM2_BLUR_SPLIT);         // ... and every later one
    CHECK(ce_plan_ssim2_ref_blur(true, true, false, true, true, 2, 2) == CE_SSIM2_BLUR_SPLIT);            // a prefix launch of a covered batch
    CHECK(ce_plan_ssim2_ref_blur(true, true, true, false, false, 1, 1) == CE_SSIM2_BLUR_SPLIT_BUILD);     // a handle's first compare
    CHECK(ce_plan_ssim2_ref_blur(true, true, true, true, true, 1, 1) == CE_SSIM2_BLUR_SPLIT);             // ... and its later ones
    CHECK(ce_plan_ssim2_ref_blur(true, false, false, true, false, 432, 54) == CE_SSIM2_BLUR_TODAY);       // CE_KEEP_REFERENCE_STATE=0

    // the record: marked and invalidated like CE_REF_SSIM2 (slab, count, scale count), never counted in builds[]
    unsigned char slab[4], roundtripped[4];
    ce_ref_states r;
    static_assert(CE_REF_SSIM2_BLUR >= 3 && CE_REF_SSIM2_BLUR < CE_REF_KINDS, "no chain of its own");
    CHECK(!r.reuse(CE_REF_SSIM2, slab, 3, 6) && r.builds[0] == 1);
    CHECK(!r.of[CE_REF_SSIM2_BLUR].covers(slab, 1, 6));
    CHECK(!r.reuse(CE_REF_SSIM2_BLUR, slab, 3, 6));
    CHECK(r.builds[0] == 1 && r.builds[1] == 0 && r.builds[2] == 0);
    r.built(CE_REF_SSIM2, slab, 3, 6);
    r.built(CE_REF_SSIM2_BLUR, slab, 3, 6);
    CHECK(r.builds[0] == 1 && r.builds[1] == 0 && r.builds[2] == 0);
    CHECK(r.of[CE_REF_SSIM2_BLUR].covers(slab, 3, 6) && r.of[CE_REF_SSIM2_BLUR].covers(slab, 2, 6));
    CHECK(!r.of[CE_REF_SSIM2_BLUR].covers(slab, 4, 6));          // more references than were built
    CHECK(!r.of[CE_REF_SSIM2_BLUR].covers(slab, 3, 5));          // another scale count
    CHECK(!r.of[CE_REF_SSIM2_BLUR].covers(roundtripped, 3, 6));  // the roundtrip's slab
    CHECK(r.reuse(CE_REF_SSIM2_BLUR, slab, 3, 6) && r.builds[0] == 1);
    CHECK(!r.reuse(CE_REF_SSIM2_BLUR, slab, 4, 6));              // drops the record, counts nothing
    CHECK(!r.of[CE_REF_SSIM2_BLUR].covers(slab, 1, 6) && r.builds[0] == 1 && r.builds[1] == 0 && r.builds[2] == 0);
    CHECK(r.of[CE_REF_SSIM2].covers(slab, 3, 6));                // each record on its own
    r.built(CE_REF_SSIM2_BLUR, slab, 4, 6);
    r.invalidate();  // a reference was written: both go
    CHECK(!r.of[CE_REF_SSIM2_BLUR].covers(slab, 1, 6) && !r.of[CE_REF_SSIM2].covers(slab, 1, 6));
    CHECK(r.builds[0] == 1 && r.builds[1] == 0 && r.builds[2] == 0);

    std::printf("ssim2 ref blur plan OK\n");
    return 0;
}
