// Where a Butteraugli launch forms the LF term (codec-eval_amd/csrc/ce_plan.h: ce_plan_ba_lf_term_in_blur), beside the record
// that decides `cached` (ce_ref_state.h: CE_REF_BUTTERAUGLI).  No device.
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
    // the rule: in the blur exactly when the references' LF planes and mask values are in place before the launch
    CHECK(!ce_plan_ba_lf_term_in_blur(true, false));   // a batch's first launch, a pooled batch, a rewritten reference
    CHECK(ce_plan_ba_lf_term_in_blur(true, true));     // a steady launch
    CHECK(!ce_plan_ba_lf_term_in_blur(false, true));   // CE_BA_LF_TERM=0
    CHECK(!ce_plan_ba_lf_term_in_blur(false, false));

    // ... as a batch's launches reach it: the launch that builds the state never, the ones that find it always
    unsigned char slab[4];
    ce_ref_states r;
    const uint64_t target = 80;
    CHECK(!ce_plan_ba_lf_term_in_blur(true, r.reuse(CE_REF_BUTTERAUGLI, slab, 3, target)));
    r.built(CE_REF_BUTTERAUGLI, slab, 3, target);
    CHECK(ce_plan_ba_lf_term_in_blur(true, r.reuse(CE_REF_BUTTERAUGLI, slab, 3, target)));
    CHECK(ce_plan_ba_lf_term_in_blur(true, r.reuse(CE_REF_BUTTERAUGLI, slab, 2, target)));    // a prefix of the references
    CHECK(!ce_plan_ba_lf_term_in_blur(true, r.reuse(CE_REF_BUTTERAUGLI, slab, 3, target + 1)));  // another intensity target
    r.built(CE_REF_BUTTERAUGLI, slab, 3, target + 1);
    r.invalidate();  // a reference was written
    CHECK(!ce_plan_ba_lf_term_in_blur(true, r.reuse(CE_REF_BUTTERAUGLI, slab, 3, target + 1)));

    std::printf("ba lf term plan OK\n");
    return 0;
}
