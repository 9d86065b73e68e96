// The host-side launch plans of codec-eval_amd/csrc/ce_plan.h on hand-derived cases.  No device.
// - The chunk plan of ce_eval_batch: budget cap with ring reuse, the first-chunk ramp, two buckets, a split reference, the
//   pooled-batch hint.
// - The XCD-aware work lists: one list per tile encoding (Butteraugli's Malta tiles, SSIMULACRA2's channel blocks, DSSIM's
//   strips with a rounded class length), and properties over a sweep of bindings.
#include <cstdint>
#include <cstdio>
#include <set>
#include <utility>
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

static ce_plan_inputs inputs(size_t cap_pairs, size_t ramp, uint32_t pooled = 0, size_t forced = 0, size_t max_slots = (size_t)1 << 40)
{
    return ce_plan_inputs{cap_pairs * kPerPair, kPerPair, pooled, forced, ramp, max_slots};
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

// what a launch counts: the chunk's references beside its pairs
static size_t slots_of(const ce_plan_chunk &c) { return c.refs.size() + pairs_of(c); }

// every item of the bucket in exactly one chunk, no chunk past max_slots, every part of a chunk non-empty
static void check_cap(const std::vector<ce_plan_chunk> &plan, size_t n_items, size_t max_slots)
{
    std::vector<int> seen(n_items, 0);
    for (const ce_plan_chunk &c : plan) {
        CHECK(slots_of(c) <= max_slots);
        CHECK(c.max_pairs >= pairs_of(c));
        for (auto &g : c.refs) {
            CHECK(!g.empty());
            for (size_t i : g)
                if (i < n_items) seen[i]++;
        }
    }
    size_t once = 0;
    for (int s : seen) once += s == 1;
    CHECK(once == n_items);
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

static const ce_plan_entry kPad{~0u, 0u};

static bool operator==(const ce_plan_entry &a, const ce_plan_entry &b) { return a.tile == b.tile && a.pair == b.pair; }

static void check_list(const std::vector<ce_plan_entry> &got, const std::vector<ce_plan_entry> &want)
{
    CHECK(got.size() == want.size());
    for (size_t i = 0; i < got.size() && i < want.size(); i++)
        if (!(got[i] == want[i])) {
            std::printf("entry %zu: (%x, %u), want (%x, %u)\n", i, got[i].tile, got[i].pair, want[i].tile, want[i].pair);
            g_fail++;
        }
}

// the list whose class x holds cls[x] (entry id = slot * 8 + class), padded to `len` slots
static std::vector<ce_plan_entry> from_classes(const std::vector<std::vector<ce_plan_entry>> &cls, size_t len)
{
    std::vector<ce_plan_entry> v(len * 8, kPad);
    for (size_t x = 0; x < cls.size(); x++)
        for (size_t i = 0; i < cls[x].size(); i++) v[i * 8 + x] = cls[x][i];
    return v;
}

// Properties of any list: every (tile, pair) of a pair below n_pairs appears exactly once; all other entries are padding;
// key i of the bound references (in reference order) sits in class i % 8; the length is 8 x round_to x k, with no padding
// group of round_to slots at the end.
static void check_list_properties(const std::vector<uint32_t> &pair_ref, uint32_t n_pairs, uint32_t n_refs, const ce_xcd_keys &k)
{
    const std::vector<ce_plan_entry> list = ce_plan_xcd_list(pair_ref.data(), n_pairs, n_refs, k);
    std::vector<uint32_t> first_key(n_refs, ~0u);  // global index of each bound reference's first key
    uint32_t keys = 0;
    for (uint32_t r = 0; r < n_refs; r++)
        for (uint32_t p = 0; p < n_pairs; p++)
            if (pair_ref[p] == r) {
                first_key[r] = keys;
                keys += k.channels * k.keys_per_channel;
                break;
            }
    std::set<std::pair<uint32_t, uint32_t>> want, seen;
    for (uint32_t p = 0; p < n_pairs; p++)
        for (uint32_t c = 0; c < k.channels; c++)
            for (uint32_t t = 0; t < k.keys_per_channel * k.tiles_per_key; t++) want.insert({t | c << 16, p});
    size_t last_used = 0;
    for (size_t i = 0; i < list.size(); i++) {
        const ce_plan_entry e = list[i];
        if (e == kPad) continue;
        last_used = i / 8 + 1;
        CHECK(e.pair < n_pairs);
        if (e.pair >= n_pairs) continue;
        CHECK(seen.insert({e.tile, e.pair}).second);
        const uint32_t c = e.tile >> 16, j = (e.tile & 0xffffu) / k.tiles_per_key;
        CHECK(first_key[pair_ref[e.pair]] != ~0u);
        CHECK((first_key[pair_ref[e.pair]] + c * k.keys_per_channel + j) % 8 == i % 8);
    }
    CHECK(seen == want);
    CHECK(list.size() % (8 * k.round_to) == 0);
    CHECK(list.size() / 8 - last_used < k.round_to);
}

static void xcd_lists()
{
    {  // the worked example: references 0 (pairs 0, 2) and 1 (pair 1), three keys each, one tile per key
        const std::vector<uint32_t> pair_ref{0, 1, 0};
        check_list(ce_plan_xcd_list(pair_ref.data(), 3, 2, ce_xcd_keys{1, 3, 1}),
                   {{0, 0}, {1, 0}, {2, 0}, {0, 1}, {1, 1}, {2, 1}, kPad, kPad,  //
                    {0, 2}, {1, 2}, {2, 2}, kPad, kPad, kPad, kPad, kPad});
    }
    {  // SSIMULACRA2 (3 channels x 2 blocks, entry block | channel << 16): pairs bound out of order (reference 2 holds
       // pairs 0 and 2, reference 0 pair 1), reference 1 unbound, pair 3 past n_pairs.  Reference 0's six keys take
       // classes 0-5, reference 2's classes 6, 7, 0, 1, 2, 3.
        const std::vector<uint32_t> pair_ref{2, 0, 2, 1};
        const uint32_t C1 = 1u << 16, C2 = 2u << 16;
        check_list(ce_plan_xcd_list(pair_ref.data(), 3, 3, ce_xcd_keys{3, 2, 1}),
                   from_classes({{{0, 1}, {C1, 0}, {C1, 2}},
                                 {{1, 1}, {C1 | 1, 0}, {C1 | 1, 2}},
                                 {{C1, 1}, {C2, 0}, {C2, 2}},
                                 {{C1 | 1, 1}, {C2 | 1, 0}, {C2 | 1, 2}},
                                 {{C2, 1}},
                                 {{C2 | 1, 1}},
                                 {{0, 0}, {0, 2}},
                                 {{1, 0}, {1, 2}}},
                                3));
    }
    {  // DSSIM (one key per row block covering its 3 strips, entry row block * 3 + strip; classes rounded to 4 slots):
       // one reference with pairs 0 and 1, two row blocks
        const std::vector<uint32_t> pair_ref{0, 0};
        check_list(ce_plan_xcd_list(pair_ref.data(), 2, 1, ce_xcd_keys{1, 2, 3, 4}),
                   from_classes({{{0, 0}, {0, 1}, {1, 0}, {1, 1}, {2, 0}, {2, 1}},  //
                                 {{3, 0}, {3, 1}, {4, 0}, {4, 1}, {5, 0}, {5, 1}}},
                                8));
    }
    {  // no pair: an empty list
        const std::vector<uint32_t> pair_ref{0};
        CHECK(ce_plan_xcd_list(pair_ref.data(), 0, 1, ce_xcd_keys{3, 5, 1}).empty());
    }
    // properties over a sweep: up to 20 references (some unbound), pairs bound in a scrambled order, n_pairs below the
    // table's length, key counts that are and are not multiples of 8, round_to 1 and 4
    uint32_t seed = 1;
    auto next = [&seed](uint32_t n) {
        seed = seed * 1664525u + 1013904223u;
        return (seed >> 8) % n;
    };
    for (int it = 0; it < 300; it++) {
        const uint32_t n_refs = 1 + next(20), max_pairs = 1 + next(40), n_pairs = next(max_pairs + 1);
        std::vector<uint32_t> pair_ref(max_pairs);
        for (auto &r : pair_ref) r = next(n_refs) & ~1u;  // odd references stay unbound
        const ce_xcd_keys k{1 + next(3), 1 + next(24), 1 + next(5), next(2) ? 4u : 1u};
        check_list_properties(pair_ref, n_pairs, n_refs, k);
    }
}

int main()
{
    xcd_lists();
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
    {  // the launch cap: 3 references x 100 000 tests, no budget cap, a launch of 65535 slots.  By bytes alone: three chunks
       // of 100 001 slots.  Target 65534 (one reference beside it), each reference split 65534 + 34466, no two parts share a chunk
        bucket b(3, 100000);
        std::vector<ce_plan_chunk> plan;
        uint32_t ring = 0;
        ce_plan_bucket(b.items, b.refs, inputs((size_t)1 << 30, 0), ring, plan);
        check_chunks(plan, 0, {100000, 100000, 100000}, {0, 1, 2}, {kNone, kNone, kNone}, 100000);
        plan.clear();
        ring = 0;
        ce_plan_bucket(b.items, b.refs, inputs((size_t)1 << 30, 0, 0, 0, ce_launch_slots_max), ring, plan);
        check_chunks(plan, 0, {65534, 34466, 65534, 34466, 65534, 34466}, {0, 1, 2, 0, 1, 2}, {kNone, kNone, kNone, 0, 1, 2}, 65534);
        check_cap(plan, b.items.size(), ce_launch_slots_max);
        CHECK(slots_of(plan[0]) == ce_launch_slots_max);
        // ... which is what inputs that name no limit plan under
        plan.clear();
        ring = 0;
        ce_plan_bucket(b.items, b.refs, ce_plan_inputs{((size_t)1 << 30) * kPerPair, kPerPair, 0, 0, 0}, ring, plan);
        check_cap(plan, b.items.size(), ce_launch_slots_max);
        CHECK(plan.size() == 6);
        // ... and with the ramp: a chunk's first part is taken whole, so the same chunks
        plan.clear();
        ring = 0;
        ce_plan_bucket(b.items, b.refs, inputs((size_t)1 << 30, 64, 0, 0, ce_launch_slots_max), ring, plan);
        check_chunks(plan, 0, {65534, 34466, 65534, 34466, 65534, 34466}, {0, 1, 2, 0, 1, 2}, {kNone, kNone, kNone, 0, 1, 2}, 65534);
    }
    {  // every pair with a reference of its own counts two slots: 10 such pairs, a launch of 7 slots -> target 6, but three
       // references and their three pairs fill a chunk (a fourth pair would make 8 slots)
        bucket b(10, 1);
        std::vector<ce_plan_chunk> plan;
        uint32_t ring = 0;
        ce_plan_bucket(b.items, b.refs, inputs(1u << 20, 0, 0, 0, 7), ring, plan);
        check_chunks(plan, 0, {3, 3, 3, 1}, {0, 1, 2, 0}, {kNone, kNone, kNone, 0}, 6);
        check_cap(plan, 10, 7);
        // one reference with 20 tests, a launch of 5 slots: five chunks of the reference and 4 tests
        bucket one(1, 20);
        plan.clear();
        ring = 0;
        ce_plan_bucket(one.items, one.refs, inputs(1u << 20, 64, 0, 0, 5), ring, plan);
        check_chunks(plan, 0, {4, 4, 4, 4, 4}, {0, 1, 2, 0, 1}, {kNone, kNone, kNone, 0, 1}, 4);
        check_cap(plan, 20, 5);
        // a budget below the launch cap still rules: cap 8 pairs, a launch of 100 slots
        plan.clear();
        ring = 0;
        ce_plan_bucket(one.items, one.refs, inputs(8, 64, 0, 0, 100), ring, plan);
        check_chunks(plan, 0, {8, 8, 4}, {0, 1, 2}, {kNone, kNone, kNone}, 8);
    }
    {  // a sweep: references with 1 .. 9 tests, launches of 2 .. 40 slots, with and without the ramp
        for (size_t max_slots = 2; max_slots <= 40; max_slots += 3)
            for (size_t n_tests = 1; n_tests <= 9; n_tests += 4)
                for (size_t ramp : {(size_t)0, (size_t)4}) {
                    bucket b(17, n_tests);
                    std::vector<ce_plan_chunk> plan;
                    uint32_t ring = 0;
                    ce_plan_bucket(b.items, b.refs, inputs(1u << 20, ramp, 0, 0, max_slots), ring, plan);
                    check_cap(plan, b.items.size(), max_slots);
                }
    }
    if (g_fail) std::printf("%d check(s) failed\n", g_fail);
    else std::printf("eval plan: all checks passed\n");
    return g_fail ? 1 : 0;
}
