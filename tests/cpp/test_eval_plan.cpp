// The chunk plan of ce_eval_batch (codec-eval_amd/csrc/ce_plan.h) on hand-derived cases: budget cap with ring reuse, the
// first-chunk ramp, two buckets, a split reference, the pooled-batch hint.  No device.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "ce_plan.h"

static int g_fail = 0;
#define CHECK(c)                                                        \
    do {                                                                \
        if (!(c)) {                                                     \
            std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #c);    \
            g_fail++;                                                   \
        }                                                               \
    } while (0)

static const size_t kNone = ce_plan_none;
static const size_t kPerPair = 1000;

static ce_plan_inputs inputs(size_t cap_pairs, size_t ramp, uint32_t pooled = 0, size_t forced = 0)
{
    return ce_plan_inputs{cap_pairs * kPerPair, kPerPair, pooled, forced, ramp};
}

// n_refs references with n_tests tests each; the items are listed test-major (item t * n_refs + r belongs to reference r),
// so that grouping by reference pointer has to gather them
struct bucket {
    std::vector<size_t> items;
    std::vector<const void *> refs;
    bucket(size_t n_refs, size_t n_tests, size_t first_item = 0, uintptr_t ref_base = 0x1000)
    {
        for (size_t t = 0; t < n_tests; t++)
            for (size_t r = 0; r < n_refs; r++) {
                items.push_back(first_item + t * n_refs + r);
                refs.push_back(reinterpret_cast<const void *>(ref_base + 16 * r));
            }
    }
};

static size_t pairs_of(const ce_plan_chunk &c)
{
    size_t k = 0;
    for (auto &g : c.refs) k += g.size();
    return k;
}

static void check_chunks(const std::vector<ce_plan_chunk> &plan, size_t first, const std::vector<size_t> &counts,
                         const std::vector<uint32_t> &slots, const std::vector<size_t> &collect_first, uint32_t max_pairs)
{
    CHECK(plan.size() == first + counts.size());
    if (plan.size() != first + counts.size()) return;
    for (size_t i = 0; i < counts.size(); i++) {
        const ce_plan_chunk &c = plan[first + i];
        if (pairs_of(c) != counts[i]) std::printf("chunk %zu: %zu pairs, want %zu\n", first + i, pairs_of(c), counts[i]);
        CHECK(pairs_of(c) == counts[i]);
        CHECK(c.slot == slots[i]);
        CHECK(c.collect_first == collect_first[i]);
        CHECK(c.max_pairs == max_pairs);
    }
}

int main()
{
    {  // 12 refs x 4 tests, cap 8 pairs, ramp 64: six chunks of two whole references on slots 0,1,2,0,1,2
        bucket b(12, 4);
        std::vector<ce_plan_chunk> plan;
        uint32_t ring = 0;
        ce_plan_bucket(b.items, b.refs, inputs(8, 64), ring, plan);
        check_chunks(plan, 0, {8, 8, 8, 8, 8, 8}, {0, 1, 2, 0, 1, 2}, {kNone, kNone, kNone, 0, 1, 2}, 8);
        CHECK(ring == 6);
        CHECK(plan[0].refs.size() == 2);
        CHECK((plan[0].refs[0] == std::vector<size_t>{0, 12, 24, 36}));
        CHECK((plan[0].refs[1] == std::vector<size_t>{1, 13, 25, 37}));
        CHECK((plan[5].refs[1] == std::vector<size_t>{11, 23, 35, 47}));
    }
    {  // 250 refs x 8 tests, no cap, ramp 64: target 667, chunks 64, 128, 256, 512, 664 (83 refs), 376
        bucket b(250, 8);
        std::vector<ce_plan_chunk> plan;
        uint32_t ring = 0;
        ce_plan_bucket(b.items, b.refs, inputs(1u << 20, 64), ring, plan);
        check_chunks(plan, 0, {64, 128, 256, 512, 664, 376}, {0, 1, 2, 0, 1, 2}, {kNone, kNone, kNone, 0, 1, 2}, 667);
        // ... and without the ramp: 664, 664, 664, 8
        plan.clear();
        ring = 0;
        ce_plan_bucket(b.items, b.refs, inputs(1u << 20, 0), ring, plan);
        check_chunks(plan, 0, {664, 664, 664, 8}, {0, 1, 2, 0}, {kNone, kNone, kNone, 0}, 667);
    }
    {  // two buckets: the ring counter continues, the ramp only applies to the call's first bucket, and a chunk only
       // collects earlier chunks of its own bucket (shape)
        bucket a(128, 1), b(200, 1, 128, 0x100000);
        std::vector<ce_plan_chunk> plan;
        uint32_t ring = 0;
        ce_plan_bucket(a.items, a.refs, inputs(1u << 20, 64), ring, plan);  // 2 chunks of target 64
        check_chunks(plan, 0, {64, 64}, {0, 1}, {kNone, kNone}, 64);
        ce_plan_bucket(b.items, b.refs, inputs(1u << 20, 64), ring, plan);  // 3 chunks of target 67, no ramp
        check_chunks(plan, 2, {67, 67, 66}, {2, 0, 1}, {kNone, kNone, kNone}, 67);
        CHECK(ring == 5);
        CHECK(plan[2].refs.front().front() == 128);
        // the same second bucket as the call's first one ramps: 64, 67, 67, 2
        std::vector<ce_plan_chunk> alone;
        uint32_t ring2 = 0;
        ce_plan_bucket(b.items, b.refs, inputs(1u << 20, 64), ring2, alone);
        check_chunks(alone, 0, {64, 67, 67, 2}, {0, 1, 2, 0}, {kNone, kNone, kNone, 0}, 67);
    }
    {  // a reference with more tests than the cap is split, its reference uploaded once per part
        bucket one(1, 20);
        std::vector<ce_plan_chunk> plan;
        uint32_t ring = 0;
        ce_plan_bucket(one.items, one.refs, inputs(8, 64), ring, plan);
        check_chunks(plan, 0, {8, 8, 4}, {0, 1, 2}, {kNone, kNone, kNone}, 8);
        for (auto &c : plan) CHECK(c.refs.size() == 1);
        CHECK((plan[2].refs[0] == std::vector<size_t>{16, 17, 18, 19}));
        // reference A with 10 tests and B with 3, cap 8: A's first 8; then A's last 2 and B share a chunk
        std::vector<size_t> items;
        std::vector<const void *> refs;
        for (size_t i = 0; i < 13; i++) {
            items.push_back(i);
            refs.push_back(reinterpret_cast<const void *>(uintptr_t(i < 10 ? 0x10 : 0x20)));
        }
        plan.clear();
        ring = 0;
        ce_plan_bucket(items, refs, inputs(8, 64), ring, plan);
        check_chunks(plan, 0, {8, 5}, {0, 1}, {kNone, kNone}, 8);
        CHECK(plan[1].refs.size() == 2);
        CHECK((plan[1].refs[0] == std::vector<size_t>{8, 9}));
        CHECK((plan[1].refs[1] == std::vector<size_t>{10, 11, 12}));
    }
    {  // pooled-batch hint: a pooled slot-0 batch of >= 3/4 of the target (and below it) becomes the target
        bucket b(100, 1);
        std::vector<ce_plan_chunk> plan;
        uint32_t ring = 0;
        ce_plan_bucket(b.items, b.refs, inputs(1u << 20, 64, 80), ring, plan);  // target 100 -> 80: several, ramp 64
        check_chunks(plan, 0, {64, 36}, {0, 1}, {kNone, kNone}, 80);
        plan.clear();
        ring = 0;
        ce_plan_bucket(b.items, b.refs, inputs(1u << 20, 64, 74), ring, plan);  // 74 * 4 < 300: target stays 100
        check_chunks(plan, 0, {100}, {0}, {kNone}, 100);
        plan.clear();
        ring = 0;
        ce_plan_bucket(b.items, b.refs, inputs(1u << 20, 64, 120), ring, plan);  // large enough already
        check_chunks(plan, 0, {100}, {0}, {kNone}, 100);
    }
    {  // CE_EVAL_BATCH_CHUNKS=2 on 10 pairs: two chunks of 5
        bucket b(10, 1);
        std::vector<ce_plan_chunk> plan;
        uint32_t ring = 0;
        ce_plan_bucket(b.items, b.refs, inputs(1u << 20, 64, 0, 2), ring, plan);
        check_chunks(plan, 0, {5, 5}, {0, 1}, {kNone, kNone}, 5);
    }
    if (g_fail) std::printf("%d check(s) failed\n", g_fail);
    else std::printf("eval plan: all checks passed\n");
    return g_fail ? 1 : 0;
}
