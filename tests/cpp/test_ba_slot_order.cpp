// The launch-id decode of Butteraugli's per-slot kernels (codec-eval_amd/csrc/ba_slot_order.h).  No device.
//   1. both orders, every grid: the ids 0 .. blocks - 1 hit every (tile, plane, slot in z0 .. z0 + n_slots - 1) exactly once;
//      every other id is a padding id and maps to nothing; ids past the grid are never produced by a launch
//   2. slot order: all items of a slot carry one id % 8, the slots of one class are walked one after the other (a slot's
//      items are consecutive among the ids of its class, tiles row-major), and there are fewer than 8 slots of padding
//   3. tile order: the id is the linear id of a (tiles_x, tiles_y, slots x planes) grid, x fastest - the launch order of the
//      3-D grids the kernels had
//   4. the rule that picks the order: slot order from ba_slot_order_min slots on, while the padding is at most n / 16
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "ba_slot_order.h"

#define CHECK(cond)                                                         \
    do {                                                                    \
        if (!(cond)) {                                                      \
            std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond); \
            std::exit(1);                                                   \
        }                                                                   \
    } while (0)

namespace {

long ids_checked = 0, padding_ids = 0;

void check_grid(uint32_t tx, uint32_t ty, uint32_t planes, uint32_t n_slots, uint32_t z0, bool by_xcd)
{
    ba_slot_grid s = ba_slot_grid_make(tx, ty, planes, n_slots, z0, ~0u);
    CHECK(s.by_xcd == 0);
    s.by_xcd = by_xcd ? 1u : 0u;  // either order at every slot count, whatever the rule would pick
    const uint64_t per_slot = (uint64_t)tx * ty * planes, blocks = ba_slot_blocks(s);
    CHECK(ba_slot_items(s) == per_slot);
    CHECK(blocks >= per_slot * n_slots && blocks < per_slot * (n_slots + (by_xcd ? ba_slot_xcds : 1u)));
    if (!by_xcd) CHECK(blocks == per_slot * n_slots);
    std::vector<uint8_t> hit(per_slot * n_slots, 0);
    std::vector<int> cls(n_slots, -1);                 // id % 8 of a slot's items
    std::vector<long> last_slot(ba_slot_xcds, -1);     // per class: the slot its latest id worked on (z0 excluded)
    std::vector<uint64_t> next_item(n_slots, 0);       // per slot: the item its next id must carry
    uint64_t live = 0;
    for (uint64_t id = 0; id < blocks; id++, ids_checked++) {
        const ba_slot_item it = ba_slot_decode(s, id);
        if (!it.live) {
            CHECK(by_xcd);  // tile order has no padding
            padding_ids++;
            continue;
        }
        live++;
        CHECK(it.x < tx && it.y < ty && it.plane < planes && it.z >= z0 && it.z - z0 < n_slots);
        const uint32_t slot = it.z - z0;
        const uint64_t item = ((uint64_t)it.plane * ty + it.y) * tx + it.x;
        CHECK(!hit[slot * per_slot + item]);
        hit[slot * per_slot + item] = 1;
        if (by_xcd) {
            const uint32_t c = (uint32_t)(id % ba_slot_xcds);
            CHECK(cls[slot] == -1 || cls[slot] == (int)c);
            cls[slot] = (int)c;
            CHECK(slot % ba_slot_xcds == c);
            CHECK(item == next_item[slot]++);  // row-major, nothing of another slot of the class in between:
            if (last_slot[c] < 0)              // the class starts with slot c and never returns to an earlier slot
                CHECK(slot == c);
            else if (slot != (uint32_t)last_slot[c])
                CHECK(slot == (uint32_t)last_slot[c] + ba_slot_xcds && next_item[(size_t)last_slot[c]] == per_slot);
            last_slot[c] = slot;
        } else {
            CHECK(id == it.x + (uint64_t)tx * (it.y + (uint64_t)ty * ((uint64_t)slot * planes + it.plane)));
        }
    }
    CHECK(live == per_slot * n_slots);
    for (uint8_t h : hit) CHECK(h == 1);
}

}  // namespace

int main()
{
    const uint32_t slot_counts[] = {1, 7, 8, 9, 63, 64, 65, 576}, z0s[] = {0, 1, 8};
    for (uint32_t tx = 1; tx <= 13; tx++)
        for (uint32_t ty = 1; ty <= 17; ty++)
            for (uint32_t n : slot_counts)
                for (uint32_t z0 : z0s)
                    for (int by_xcd = 0; by_xcd < 2; by_xcd++) {
                        check_grid(tx, ty, 1, n, z0, by_xcd != 0);
                        if (tx <= 3) check_grid(tx, ty, 3, n, z0, by_xcd != 0);  // the row blur: 256-wide tiles, three planes
                    }
    // the rule: from ba_slot_order_min slots on, while the last group's padding is at most a sixteenth of the slots
    for (uint32_t n = 1; n <= 600; n++) {
        const uint32_t pad = (8 - n % 8) % 8, want = n >= ba_slot_order_min && 16 * pad <= n ? 1u : 0u;
        CHECK(ba_slot_grid_make(8, 16, 1, n, 0).by_xcd == want);
        CHECK(ba_slot_grid_make(8, 16, 1, n, 16).by_xcd == want);  // the slots past z0 count, not z0
        if (n % 8 == 0) CHECK(want == (n >= ba_slot_order_min ? 1u : 0u));
    }
    CHECK(ba_slot_order_min == 64);
    CHECK(!ba_slot_grid_make(8, 16, 1, 63, 0).by_xcd && ba_slot_grid_make(8, 16, 1, 64, 0).by_xcd && !ba_slot_grid_make(8, 16, 1, 65, 0).by_xcd);
    CHECK(ba_slot_grid_make(8, 16, 1, 71, 0).by_xcd && ba_slot_grid_make(8, 16, 1, 72, 0).by_xcd && !ba_slot_grid_make(8, 16, 1, 73, 0).by_xcd);
    CHECK(ba_slot_grid_make(8, 16, 1, 121, 0).by_xcd && ba_slot_grid_make(8, 16, 1, 576, 0).by_xcd);
    CHECK(!ba_slot_grid_make(8, 70000, 1, 576, 0).by_xcd);  // too tall for the y of a slot-order grid
    // a large grid stays inside 32 bits where the launch code admits it
    {
        const ba_slot_grid s = ba_slot_grid_make(240, 135, 1, 4096, 0);
        CHECK(ba_slot_blocks(s) == (uint64_t)240 * 135 * 4096);
        const ba_slot_item it = ba_slot_decode(s, ba_slot_blocks(s) - 1);
        CHECK(it.live && it.x == 239 && it.y == 134 && it.z == 4095);
    }
    std::printf("ba slot order OK: %ld ids, %ld padding ids\n", ids_checked, padding_ids);
    return 0;
}
