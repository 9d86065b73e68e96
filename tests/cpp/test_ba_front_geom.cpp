// The region and rim index logic of Butteraugli's front end (codec-eval_amd/csrc/ba_front_geom.h) against what the kernel's
// earlier form did: it mirrored every tap of both blur passes in image coordinates.  No device.
//   1. rim: for every level size up to 70 x 70 and every tile, every tap of every stored output - read with plain indices
//      from the region after the rim fill - is the element the mirrored tap named; a copy's source is an in-image cell of
//      the region
//   2. loads, full resolution (sizes up to 70 x 70) and half resolution (source sizes up to 70 x 70 and some up to 140, odd ones
//      included), at every alignment of the image in its slab: every in-image cell is loaded exactly once, no other cell is
//      loaded, and no packed load's 16-byte window leaves the image's bytes; the kernel's walk of the rim visits every
//      out-of-image cell once
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "ba_front_geom.h"

#define CHECK(cond)                                                         \
    do {                                                                    \
        if (!(cond)) {                                                      \
            std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond); \
            std::exit(1);                                                   \
        }                                                                   \
    } while (0)

namespace {

constexpr int FT = ba_front_tile, FR = ba_front_region;

// the mirroring of the earlier stages, restated
int old_mirror(int x, int n)
{
    while (x < 0 || x >= n) x = x < 0 ? -x - 1 : 2 * n - 1 - x;
    return x;
}

long taps_checked = 0, copies = 0, zeroed = 0, fast_tasks = 0, slow_cells = 0;

void check_rim(int w, int h)
{
    for (int y0 = 0; y0 < h; y0 += FT)
        for (int x0 = 0; x0 < w; x0 += FT) {
            const int gx0 = x0 - 2, gy0 = y0 - 2;
            // the element each region cell holds after the load phase and the rim fill: y * w + x, -1 = zero
            std::vector<int> elem(FR * FR, -2);
            for (int i = 0; i < FR * FR; i++) {
                const int X = gx0 + i % FR, Y = gy0 + i / FR;
                if (X >= 0 && X < w && Y >= 0 && Y < h) elem[i] = Y * w + X;
            }
            const std::vector<int> loaded = elem;
            // the kernel's walk: the out-of-image columns whole, then the out-of-image rows over the in-image columns
            std::vector<int> visits(FR * FR, 0);
            auto fill = [&](int lx, int ly) {
                CHECK(lx >= 0 && lx < FR && ly >= 0 && ly < FR);
                const int i = ly * FR + lx;
                int src = -1;
                const int kind = ba_front_rim(gx0 + lx, gy0 + ly, w, h, gx0, gy0, src);
                CHECK(kind != BA_RIM_IMAGE && loaded[i] < 0);
                visits[i]++;
                if (kind == BA_RIM_COPY) {
                    CHECK(src >= 0 && src < FR * FR);
                    CHECK(loaded[src] >= 0);  // an in-image cell: nothing waits for another copy
                    elem[i] = loaded[src];
                    copies++;
                } else {
                    elem[i] = -1;
                    zeroed++;
                }
            };
            const int xlo = ba_front_out_lo(gx0), xhi = ba_front_out_hi(gx0, w), ylo = ba_front_out_lo(gy0), yhi = ba_front_out_hi(gy0, h);
            for (int t = 0; t < (xlo + FR - xhi) * FR; t++) fill(ba_front_out_line(t / FR, xlo, xhi), t % FR);
            for (int t = 0; t < (ylo + FR - yhi) * FR; t++) {
                const int lx = t % FR;
                if (lx >= xlo && lx < xhi) fill(lx, ba_front_out_line(t / FR, ylo, yhi));
            }
            for (int i = 0; i < FR * FR; i++) {
                int src = -1;
                const bool in_image = ba_front_rim(gx0 + i % FR, gy0 + i / FR, w, h, gx0, gy0, src) == BA_RIM_IMAGE;
                CHECK(in_image == (loaded[i] >= 0));
                CHECK(visits[i] == (in_image ? 0 : 1));  // every out-of-image cell once, no other
            }
            for (int i = 0; i < FR * FR; i++) CHECK(elem[i] >= -1);  // every cell is defined
            // the two passes with plain indices: output (X, Y) takes rows r0 + e of H, whose cell (tx, ly) takes cells
            // c0 + d of row ly of L; the earlier form took H row mirror(Y + e) formed from elements mirror(X + d) of it
            for (int ty = 0; ty < FT; ty++)
                for (int tx = 0; tx < FT; tx++) {
                    const int X = x0 + tx, Y = y0 + ty;
                    if (X >= w || Y >= h) continue;  // not stored
                    for (int e = -2; e <= 2; e++)
                        for (int d = -2; d <= 2; d++) {
                            const int cell = (ty + 2 + e) * FR + (tx + 2 + d);
                            CHECK(elem[cell] == old_mirror(Y + e, h) * w + old_mirror(X + d, w));
                            taps_checked++;
                        }
                }
        }
}

// [first, first + 16) of a packed load of the 12 bytes at `off`, counted from the aligned address the image starts mis
// bytes after: inside the image's bytes?
void check_window(size_t off, uint32_t mis, size_t bytes)
{
    const size_t first = (mis + off) / 4 * 4;
    CHECK(first >= mis && first + 16 <= mis + bytes);
    CHECK(first <= mis + off && mis + off + 12 <= first + 16);  // and it holds the 12
}

// W8 x H8: the source image; w x h: the level (the same at full resolution)
void check_loads(bool half, int W8, int H8)
{
    const int w = half ? (W8 + 1) / 2 : W8, h = half ? (H8 + 1) / 2 : H8;
    const size_t bytes = (size_t)W8 * H8 * 3;
    for (uint32_t mis = 0; mis < 4; mis++)
        for (int y0 = 0; y0 < h; y0 += FT)
            for (int x0 = 0; x0 < w; x0 += FT) {
                const int gx0 = x0 - 2, gy0 = y0 - 2;
                std::vector<int> count(FR * FR, 0), fast_cell(FR * FR, 0);
                auto load_cell = [&](int lx, int ly) {  // the per-element route loads in-image cells only
                    const int X = gx0 + lx, Y = gy0 + ly;
                    CHECK(lx >= 0 && lx < FR && ly >= 0 && ly < FR);
                    if (X >= 0 && X < w && Y >= 0 && Y < h) count[ly * FR + lx]++, slow_cells++;
                };
                const int per_row = half ? ba_front_groups2 : ba_front_groups4, n = half ? 2 : 4;
                // the block-uniform shortcut runs plain groups through the packed route without asking task by task
                const bool all_fast = half ? ba_front_all_fast2_half(gx0, gy0, W8, H8, mis) : ba_front_all_fast4(gx0, gy0, w, h, mis);
                const int shift = half || all_fast ? 0 : ba_front_shift4(gx0, w);
                CHECK(shift == 0 || shift == 2);
                for (int i = 0; i < FR * per_row; i++) {
                    const int g = i % per_row, ly = i / per_row;
                    int cell[4] = {-1, -1, -1, -1};
                    bool contiguous = true;
                    if (half) {
                        int lx2 = -1, ly2 = -1;
                        ba_front_task2(i, lx2, ly2);
                        CHECK(ly2 == ly);
                        cell[0] = lx2, cell[1] = lx2 + 1;
                    } else {
                        contiguous = ba_front_group4_contiguous(g, shift);
                        for (int k = 0; k < 4; k++) cell[k] = ba_front_group4_cell(g, k, shift);
                    }
                    for (int k = 0; k < n; k++) CHECK(cell[k] >= 0 && cell[k] < FR && (!contiguous || cell[k] == cell[0] + k));
                    const int lx = cell[0], X0 = gx0 + lx, Y = gy0 + ly;
                    const bool fast = contiguous && (half ? ba_front_fast2_half(X0, Y, W8, H8, mis) : ba_front_fast4(X0, Y, w, h, mis));
                    CHECK(fast || !all_fast);
                    if (!fast) {
                        for (int k = 0; k < n; k++) load_cell(cell[k], ly);
                        continue;
                    }
                    fast_tasks++;
                    CHECK(Y >= 0 && Y < h && X0 >= 0 && X0 + n <= w);
                    if (half) {
                        // all eight source pixels exist, so neither element is the doubled last one of an odd size
                        CHECK(2 * X0 + 3 < W8 && 2 * Y + 1 < H8);
                        check_window(((size_t)(2 * Y) * W8 + 2 * X0) * 3, mis, bytes);
                        check_window(((size_t)(2 * Y + 1) * W8 + 2 * X0) * 3, mis, bytes);
                    } else {
                        check_window(((size_t)Y * w + X0) * 3, mis, bytes);
                    }
                    for (int k = 0; k < n; k++) count[ly * FR + lx + k]++, fast_cell[ly * FR + lx + k] = 1;
                }
                // an image whose width is a multiple of four has no group across its left or right edge: in an aligned slab
                // only the image's very last group (its window would end behind the image) goes element by element
                if (!half && w % 4 == 0 && mis == 0)
                    for (int i = 0; i < FR * FR; i++) {
                        const int X = gx0 + i % FR, Y = gy0 + i / FR;
                        if (X >= 0 && X < w && Y >= 0 && Y < h && !(Y == h - 1 && X >= w - 4)) CHECK(fast_cell[i] || i % FR < 2 || i % FR >= FR - 2);
                    }
                for (int i = 0; i < FR * FR; i++) {
                    const int X = gx0 + i % FR, Y = gy0 + i / FR;
                    CHECK(count[i] == ((X >= 0 && X < w && Y >= 0 && Y < h) ? 1 : 0));
                }
            }
}

}  // namespace

int main()
{
    CHECK(ba_mirror(-1, 5) == 0 && ba_mirror(-2, 5) == 1 && ba_mirror(5, 5) == 4 && ba_mirror(6, 5) == 3);
    CHECK(ba_mirror(-2, 1) == 0 && ba_mirror(2, 1) == 0 && ba_mirror(3, 2) == 0 && ba_mirror(-2, 2) == 1);
    for (int h = 1; h <= 70; h++)
        for (int w = 1; w <= 70; w++) {
            check_rim(w, h);
            check_loads(false, w, h);
        }
    // source sizes 1 .. 70 and, for levels of two and three tiles with an interior one, a few around 128 and 140
    std::vector<int> sizes;
    for (int n = 1; n <= 70; n++) sizes.push_back(n);
    for (int n : {127, 128, 129, 130, 139, 140}) sizes.push_back(n);
    for (int H8 : sizes)
        for (int W8 : sizes) check_loads(true, W8, H8);
    // the packed route is taken where it can be: a 70 x 70 image's second row of its first tile, aligned slab
    CHECK(ba_front_fast4(0, 1, 70, 70, 0) && ba_front_fast4(28, 1, 70, 70, 0) && !ba_front_fast4(-2, 1, 70, 70, 0));
    CHECK(!ba_front_fast4(0, 0, 70, 70, 1));      // its window would start before the image
    CHECK(!ba_front_fast4(66, 69, 70, 70, 0));    // its window would end after it
    CHECK(ba_front_fast2_half(0, 0, 70, 70, 0) && !ba_front_fast2_half(34, 0, 71, 70, 0) && ba_front_fast2_half(32, 0, 71, 70, 0));
    CHECK(taps_checked > 0 && copies > 0 && zeroed > 0 && fast_tasks > 0 && slow_cells > 0);
    std::printf("ba front geometry OK: %ld taps, %ld rim copies, %ld zeroed cells, %ld packed tasks, %ld single cells\n", taps_checked,
                copies, zeroed, fast_tasks, slow_cells);
    return 0;
}
