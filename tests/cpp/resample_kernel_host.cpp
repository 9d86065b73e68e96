// The device code of the resampler (codec-eval_amd/csrc/resample_kernel.h) compiled for the host: the HIP keywords are
// defined away, blockIdx / threadIdx are plain variables that a loop sets, and every thread of every block of the grids
// that plan_resample - the launcher's own geometry - returns runs in turn: resample_h_stage for all 256 threads, then
// resample_h_body for all 256, as the barrier between them orders a block on the device.  Built with
// -fsanitize=address,undefined by tests/test_resample_kernel_host_cpu.py.  Everything is a heap block of exactly its size:
// the source, the image between the passes, the tap tables (built by the product's ce_build_resample_table, ce_tables.cpp
// linked in), the LDS stand-in (the dynamic LDS the launch would ask for, refilled with a sentinel before every block so
// that taps a previous block staged cannot stand in for ones this block did not; a null pointer on the global-table route)
// and the destination, `off` bytes after a 16-byte boundary behind guard bytes.  A load or store outside any of them
// stops the run.
//
// usage: resample_kernel_host CONFIGS IN OUT.  CONFIGS holds one job per line:
//   table n_in n_out filter              OUT receives ksize (u32) and the table, n_out * (2 + ksize) ints
//   case w h out_w out_h n off filter    IN holds the n source images; OUT receives the horizontal table (as above) if
//                                        out_w != w, the vertical one if out_h != h, then the n output images
// and stdout one line per pass that ran: "pass JOB h|v tiles grid lds_bytes lds empty", `lds` 1 when the taps were staged
// and `empty` the number of blocks whose tile holds no byte of its row.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "hip_on_host.h"

#include "resample_kernel.h"

bool ce_build_resample_table(uint32_t n_in, uint32_t n_out, int filter, std::vector<int32_t> &table, uint32_t *ksize);  // ce_tables.cpp

static const int32_t kLdsSentinel = 0x5a5a5a5a;  // as a first tap or a tap count: far outside any source row

// the table of one axis in a block of exactly its size, and into OUT
static int32_t *build_table(uint32_t n_in, uint32_t n_out, int filter, uint32_t *ksize, FILE *out)
{
    std::vector<int32_t> t;
    if (!ce_build_resample_table(n_in, n_out, filter, t, ksize)) return nullptr;
    if (t.size() != (size_t)n_out * (2 + *ksize)) return nullptr;
    int32_t *tab = static_cast<int32_t *>(malloc(t.size() * sizeof(int32_t)));
    if (!tab) return nullptr;
    memcpy(tab, t.data(), t.size() * sizeof(int32_t));
    fwrite(ksize, 4, 1, out);
    fwrite(tab, sizeof(int32_t), t.size(), out);
    return tab;
}

static void run_h(const pass_launch &p, const int32_t *tab, uint32_t n_out, uint32_t ksize, unsigned *empty)
{
    int32_t *lds = p.lds ? static_cast<int32_t *>(malloc(p.lds_bytes)) : nullptr;
    if (p.lds && !lds) exit(70);
    for (uint32_t b = 0; b < p.grid; b++) {
        blockIdx.x = b, threadIdx.x = 0;
        const place first = find_place(p.g);
        if (first.b1 <= first.b0) ++*empty;
        if (p.lds) {
            for (size_t i = 0; i < p.lds_bytes / sizeof(int32_t); i++) lds[i] = kLdsSentinel;
            for (unsigned t = 0; t < kThreads; t++) {
                threadIdx.x = t;
                resample_h_stage(find_place(p.g), tab, n_out, ksize, lds);
            }
        }
        for (unsigned t = 0; t < kThreads; t++) {
            threadIdx.x = t;
            if (p.lds) resample_h_body<true>(p.g, find_place(p.g), tab, n_out, ksize, lds);
            else resample_h_body<false>(p.g, find_place(p.g), tab, n_out, ksize, nullptr);
        }
    }
    free(lds);
}

static void run_v(const pass_launch &p, const int32_t *tab, uint32_t n_out, uint32_t ksize, unsigned *empty)
{
    for (uint32_t b = 0; b < p.grid; b++) {
        blockIdx.x = b, threadIdx.x = 0;
        const place first = find_place(p.g);
        if (first.b1 <= first.b0) ++*empty;
        for (unsigned t = 0; t < kThreads; t++) {
            threadIdx.x = t;
            resample_v_body(p.g, tab, n_out, ksize);
        }
    }
}

int main(int argc, char **argv)
{
    if (argc != 4) return 64;
    FILE *cfg = fopen(argv[1], "r"), *in = fopen(argv[2], "rb"), *out = fopen(argv[3], "wb");
    if (!cfg || !in || !out) return 65;
    char kind[16];
    int jobs = 0;
    for (; fscanf(cfg, "%15s", kind) == 1; jobs++) {
        if (!strcmp(kind, "table")) {
            unsigned n_in, n_out, ksize;
            int filter;
            if (fscanf(cfg, "%u %u %d", &n_in, &n_out, &filter) != 3) return 66;
            int32_t *tab = build_table(n_in, n_out, filter, &ksize, out);
            if (!tab) return 67;
            free(tab);
            continue;
        }
        if (strcmp(kind, "case")) return 66;
        unsigned w, h, ow, oh, n, off;
        int filter;
        if (fscanf(cfg, "%u %u %u %u %u %u %d", &w, &h, &ow, &oh, &n, &off, &filter) != 7 || off > 15) return 66;
        const bool horiz = ow != w, vert = oh != h;
        if (!horiz && !vert) return 66;  // a byte copy: the caller's, no kernel runs
        const size_t src_img = (size_t)w * h * 3, mid_img = (size_t)ow * h * 3, dst_img = (size_t)ow * oh * 3;
        uint8_t *src = static_cast<uint8_t *>(malloc(n * src_img));
        if (!src || fread(src, 1, n * src_img, in) != n * src_img) return 68;
        uint8_t *mid = horiz && vert ? static_cast<uint8_t *>(malloc(n * mid_img)) : nullptr;
        if (mid) memset(mid, 0xEE, n * mid_img);
        const size_t guard = 16 + off;
        uint8_t *slab = static_cast<uint8_t *>(malloc(guard + n * dst_img));  // malloc: 16-byte aligned
        if (!slab || (reinterpret_cast<uintptr_t>(slab) & 15) || (horiz && vert && !mid)) return 69;
        memset(slab, 0xEE, guard + n * dst_img);
        uint32_t ksize_h = 0, ksize_v = 0;
        int32_t *tab_h = horiz ? build_table(w, ow, filter, &ksize_h, out) : nullptr;
        int32_t *tab_v = vert ? build_table(h, oh, filter, &ksize_v, out) : nullptr;
        if ((horiz && !tab_h) || (vert && !tab_v)) return 67;
        resample_launch r;
        if (!plan_resample(src, src_img, slab + guard, dst_img, w, h, ow, oh, n, horiz, vert, ksize_h, mid, &r)) return 71;
        if (horiz) {
            unsigned empty = 0;
            run_h(r.h, tab_h, ow, ksize_h, &empty);
            printf("pass %d h %u %u %zu %d %u\n", jobs, r.h.g.tiles, r.h.grid, r.h.lds_bytes, (int)r.h.lds, empty);
        }
        if (vert) {
            unsigned empty = 0;
            run_v(r.v, tab_v, oh, ksize_v, &empty);
            printf("pass %d v %u %u %zu %d %u\n", jobs, r.v.g.tiles, r.v.grid, r.v.lds_bytes, (int)r.v.lds, empty);
        }
        for (size_t i = 0; i < guard; i++)
            if (slab[i] != 0xEE) {
                fprintf(stderr, "job %d wrote in front of its destination\n", jobs);
                return 2;
            }
        fwrite(slab + guard, 1, n * dst_img, out);
        free(tab_h), free(tab_v), free(slab), free(mid), free(src);
    }
    fclose(cfg), fclose(in), fclose(out);
    printf("done %d\n", jobs);
    return 0;
}
