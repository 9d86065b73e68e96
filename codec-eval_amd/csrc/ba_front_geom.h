// Region and rim index logic of Butteraugli's front end (k_ba_front, butteraugli.hip), plain C++ without device calls, checked
// on the host by tests/cpp/test_ba_front_geom.cpp.  The functions are constexpr so that the kernel can call them as they stand.
//
// A block owns a 32 x 32 tile of a level and holds its 36 x 36 region (the tile and the 5-tap blur's halo of 2) in LDS, the
// region's cell (lx, ly) being the level's element (gx0 + lx, gy0 + ly), gx0 = x0 - 2.  The load phase fills the in-image
// cells: a task is a region row and a group of consecutive elements, loaded either from aligned dwords (the fast route) or
// element by element.  An edge tile then fills its rim - the out-of-image cells a tap can reach - from the cells the blur's
// mirroring names, after which the blur indexes the region plainly, as it does on an interior tile.
#pragma once

#include <cstddef>
#include <cstdint>

inline constexpr int ba_front_tile = 32, ba_front_halo = 2, ba_front_region = ba_front_tile + 2 * ba_front_halo;
// tasks of a region row: groups of four elements at full resolution, of two elements (2 x 4 source pixels) at half resolution
inline constexpr int ba_front_groups4 = ba_front_region / 4, ba_front_groups2 = ba_front_region / 2;

// ConvolutionWithTranspose's border rule: reflect about the edge, as often as a line shorter than the reach asks for
constexpr int ba_mirror(int x, int n)
{
    while (x < 0 || x >= n) x = x < 0 ? -x - 1 : 2 * n - 1 - x;
    return x;
}

// Full resolution, a task = a region row and one of nine groups g of four cells.  A tile whose region crosses the image's
// left or right edge shifts its groups by the halo (shift = 2): groups 0 .. 7 then start on element x0 + 4 g, so that an image
// whose width is a multiple of four has no group across either edge, and group 8 is the row's four end cells (0, 1, 34, 35:
// halo cells, loaded one by one where they are inside the image).  Every other tile has shift = 0 and nine plain groups.
constexpr int ba_front_shift4(int gx0, int w) { return (gx0 < 0 || gx0 + ba_front_region > w) ? ba_front_halo : 0; }
constexpr bool ba_front_group4_contiguous(int g, int shift) { return shift == 0 || g < ba_front_groups4 - 1; }
// cell k (0 .. 3) of group g
constexpr int ba_front_group4_cell(int g, int k, int shift)
{
    return ba_front_group4_contiguous(g, shift) ? shift + 4 * g + k : (k < 2 ? k : ba_front_region - 4 + k);
}
// Half resolution, task i -> the first of its two cells (2 x 4 source pixels); an even width has no group across an edge
constexpr void ba_front_task2(int i, int &lx, int &ly) { ly = i / ba_front_groups2, lx = 2 * (i % ba_front_groups2); }

// The fast route reads the 16 bytes from the aligned dword at or below a group's 12.  An image's bytes are
// [mis, mis + bytes) counted from an aligned address (mis = the image's address & 3: images are packed in their slab); the
// group's 12 start `off` bytes into the image.  True: the 16 lie inside the image's own bytes.
constexpr bool ba_front_window_inside(size_t off, uint32_t mis, size_t bytes)
{
    const size_t first = (mis + off) & ~(size_t)3;
    return first >= mis && first + 16 <= mis + bytes;
}

// Full resolution: may the task of row Y and elements X0 .. X0 + 3 of a w x h image take the fast route?  The row is inside
// the image, the group wholly inside the row, the window inside the image's bytes.
constexpr bool ba_front_fast4(int X0, int Y, int w, int h, uint32_t mis)
{
    if (Y < 0 || Y >= h || X0 < 0 || X0 + 4 > w) return false;
    return ba_front_window_inside(((size_t)Y * w + X0) * 3, mis, (size_t)w * h * 3);
}

// Half resolution: elements X0 and X0 + 1 of row Y are the 2 x 2 averages of source pixels 2 X0 .. 2 X0 + 3 of source rows
// 2 Y and 2 Y + 1 of the W8 x H8 image.  The fast route needs all eight inside it, which also keeps the doubled last
// element of an odd width or height (it has one source column or row only) on the per-element route.
constexpr bool ba_front_fast2_half(int X0, int Y, int W8, int H8, uint32_t mis)
{
    if (Y < 0 || 2 * Y + 1 >= H8 || X0 < 0 || 2 * X0 + 3 >= W8) return false;
    const size_t off = ((size_t)(2 * Y) * W8 + 2 * X0) * 3, bytes = (size_t)W8 * H8 * 3;
    return ba_front_window_inside(off, mis, bytes) && ba_front_window_inside(off + (size_t)W8 * 3, mis, bytes);
}

// Block-uniform shortcuts: every task of the tile takes the fast route.  The first task being fast puts the region's first
// row and column inside the image, the last one its last row and column, and a window's place grows with the task.
constexpr bool ba_front_all_fast4(int gx0, int gy0, int w, int h, uint32_t mis)
{
    return ba_front_fast4(gx0, gy0, w, h, mis) && ba_front_fast4(gx0 + ba_front_region - 4, gy0 + ba_front_region - 1, w, h, mis);
}
constexpr bool ba_front_all_fast2_half(int gx0, int gy0, int W8, int H8, uint32_t mis)
{
    return ba_front_fast2_half(gx0, gy0, W8, H8, mis) &&
           ba_front_fast2_half(gx0 + ba_front_region - 2, gy0 + ba_front_region - 1, W8, H8, mis);
}

// The out-of-image lines (columns or rows) of a region that starts at element g0 of an axis n long: the first `lo` lines (the
// halo before the image: 0 or 2) and the lines from `hi` on (the first one behind the image); [lo, hi) are inside.  The rim
// fill walks the out-of-image columns whole, then the out-of-image rows over the in-image columns: every out-of-image cell once.
constexpr int ba_front_out_lo(int g0) { return g0 < 0 ? -g0 : 0; }
constexpr int ba_front_out_hi(int g0, int n) { return n - g0 < ba_front_region ? n - g0 : ba_front_region; }
constexpr int ba_front_out_line(int k, int lo, int hi) { return k < lo ? k : hi + (k - lo); }  // the k-th of them

// What the rim fill does with the region cell of element (X, Y) of a w x h level:
//   BA_RIM_IMAGE  inside the image: loaded, left alone
//   BA_RIM_COPY   within two columns and rows of the image: takes the value of region cell `src`, the cell of
//                 (mirror(X, w), mirror(Y, h)) - both coordinates at once, from an in-image cell, so a corner waits for nobody
//   BA_RIM_ZERO   farther out: no tap of a stored output reaches it; set to zero so that nothing in LDS is undefined
// The source is always inside the region.  It is an element of [0, w).  A left rim cell (X = -1 or -2) exists only in the
// tile at x0 = 0, whose region holds elements -2 .. 33; its source is element 0 or 1, or some element of a w < 3, all in
// there.  A right rim cell (X = w or w + 1) has its source in w - 2 .. w - 1 (element 0 when w = 1), and a tile owns a column
// of the image, x0 <= w - 1, so gx0 = x0 - 2 <= w - 3 lies to the source's left and the rim cell itself to its right.  The
// same holds for rows.  tests/cpp/test_ba_front_geom.cpp checks it for every size up to 70 x 70.
enum { BA_RIM_IMAGE = 0, BA_RIM_COPY = 1, BA_RIM_ZERO = 2 };
constexpr int ba_front_rim(int X, int Y, int w, int h, int gx0, int gy0, int &src)
{
    if (X >= 0 && X < w && Y >= 0 && Y < h) return BA_RIM_IMAGE;
    if (X < -ba_front_halo || X >= w + ba_front_halo || Y < -ba_front_halo || Y >= h + ba_front_halo) return BA_RIM_ZERO;
    src = (ba_mirror(Y, h) - gy0) * ba_front_region + (ba_mirror(X, w) - gx0);
    return BA_RIM_COPY;
}
