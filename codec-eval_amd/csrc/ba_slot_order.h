// Launch order of Butteraugli's per-slot kernels (k_ba_front, k_ba_blur_h, k_ba_blur_v_split; butteraugli.hip), plain C++
// without device calls, checked on the host by tests/cpp/test_ba_slot_order.cpp.  The functions are constexpr so that the
// kernels can call them as they stand.
//
// A launch covers the image slots z0 .. z0 + n_slots - 1; a slot's work items are its planes x tiles_y x tiles_x tiles.
// Workgroups reach the 8 XCDs round-robin by launch id (the linear block index, x fastest), and every XCD has its own L2.
// A kernel decodes its item from the launch id in one of two orders:
//   tile order (by_xcd = 0)  x fastest, then y, then (slot, plane): a slot's tiles are spread over all XCDs - by column strip
//                            where tiles_x = 8 - and a tile's neighbours sit behind other L2s.
//   slot order (by_xcd = 1)  id % 8 names a class, id / 8 = k; the ids of a class walk one slot's items (plane, y, x: x fastest)
//                            and then go on with the slot 8 further along:
//                                slot = z0 + 8 (k / items_per_slot) + id % 8,   item = k % items_per_slot
//                            A slot stays on one XCD, whose L2 then serves the halo a tile shares with its neighbours.  The
//                            last group of 8 slots is padded: ids that land past the last slot map to nothing.
// Both orders hit every item exactly once, so the choice changes no result: it is made for speed alone (ba_slot_order_min).
//
// No division on the device: the grid's three dimensions are chosen so that the hardware's block index IS the decode
// (ba_slot_dims, ba_slot_decode3) - tile order (tiles_x, tiles_y, slots x planes), slot order (8 tiles_x, planes x tiles_y,
// groups of 8 slots), whose linear id is x + 8 tiles_x (y' + planes tiles_y group) with x = class + 8 tile_x.  Decoding a
// 1-D id with divisions by the tile counts in every workgroup cost 0.45 ms of a 79 ms step (profiles/r06_slot_xcd.md).
#pragma once

#include <cstdint>

inline constexpr uint32_t ba_slot_xcds = 8;
// Slot order when the launch loads all XCDs evenly: from this many slots on, and only while the padding of the last group
// of 8 is at most a sixteenth of the slots.  A one-pair call (1 - 2 slots) would run on one or two XCDs, 9 slots would make
// one XCD work twice as long as the others; measured alone, a launch of 8 n slots gains 1 - 2 % from n = 3 on and a launch of
// 8 n + 1 slots loses 2 - 9 % up to 65 slots, and in the sweep a crossover of 48 (the 54-slot Kodak bucket in slot order)
// is 0.35 ms slower than 64.  DESIGN.md section 4, profiles/r06_slot_xcd.md.
inline constexpr uint32_t ba_slot_order_min = 64;
constexpr bool ba_slot_order_even(uint32_t n_slots, uint32_t min_slots)
{
    const uint64_t padded = ((uint64_t)n_slots + ba_slot_xcds - 1) / ba_slot_xcds * ba_slot_xcds;
    return n_slots >= min_slots && 16 * (padded - n_slots) <= n_slots;
}
inline constexpr uint32_t ba_slot_grid_yz_max = 65535;  // HIP's limit of a grid's y and z

struct ba_slot_grid {
    uint32_t tiles_x, tiles_y, planes;  // of one slot
    uint32_t n_slots, z0;               // the launch's slots: z0 .. z0 + n_slots - 1
    uint32_t by_xcd;                    // slot order
};

struct ba_slot_dims3 {
    uint32_t x, y, z;
};

struct ba_slot_item {
    uint32_t x, y, plane;  // the tile and the plane
    uint32_t z;            // the slot, z0 included
    bool live;             // false: a padding id, nothing to do
};

constexpr ba_slot_grid ba_slot_grid_make(uint32_t tiles_x, uint32_t tiles_y, uint32_t planes, uint32_t n_slots, uint32_t z0,
                                         uint32_t min_slots = ba_slot_order_min)
{
    // (a level too tall for the y of a slot-order grid - 65535 tile rows - keeps tile order)
    return ba_slot_grid{tiles_x, tiles_y, planes, n_slots, z0,
                        ba_slot_order_even(n_slots, min_slots) && (uint64_t)tiles_y * planes <= ba_slot_grid_yz_max ? 1u : 0u};
}

constexpr uint64_t ba_slot_items(const ba_slot_grid &s) { return (uint64_t)s.tiles_x * s.tiles_y * s.planes; }

// the launch's grid (the caller checks y and z against ba_slot_grid_yz_max)
constexpr ba_slot_dims3 ba_slot_dims(const ba_slot_grid &s)
{
    return s.by_xcd ? ba_slot_dims3{ba_slot_xcds * s.tiles_x, s.tiles_y * s.planes, (s.n_slots + ba_slot_xcds - 1) / ba_slot_xcds}
                    : ba_slot_dims3{s.tiles_x, s.tiles_y, s.n_slots * s.planes};
}

constexpr uint64_t ba_slot_blocks(const ba_slot_grid &s)
{
    const ba_slot_dims3 d = ba_slot_dims(s);
    return (uint64_t)d.x * d.y * d.z;
}

// a kernel's decode: b = its block index in the grid of ba_slot_dims; planes = s.planes (a kernel of one plane per slot
// passes the literal, and its decode is shifts and adds)
constexpr ba_slot_item ba_slot_decode3(const ba_slot_grid &s, uint32_t planes, uint32_t bx, uint32_t by, uint32_t bz)
{
    if (s.by_xcd) {
        const uint32_t slot = ba_slot_xcds * bz + bx % ba_slot_xcds, plane = planes == 1 ? 0 : by / s.tiles_y;
        return ba_slot_item{bx / ba_slot_xcds, by - plane * s.tiles_y, plane, s.z0 + slot, slot < s.n_slots};
    }
    const uint32_t slot = planes == 1 ? bz : bz / planes;
    return ba_slot_item{bx, by, bz - slot * planes, s.z0 + slot, true};
}

// the same from the launch id (the linear block index of that grid), as the host checks it
constexpr ba_slot_item ba_slot_decode(const ba_slot_grid &s, uint64_t id)
{
    const ba_slot_dims3 d = ba_slot_dims(s);
    return ba_slot_decode3(s, s.planes, (uint32_t)(id % d.x), (uint32_t)(id / d.x % d.y), (uint32_t)(id / ((uint64_t)d.x * d.y)));
}
