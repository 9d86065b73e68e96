// The device code of the tensor ingest (codec-eval_amd/csrc/tensor_kernel.h) compiled for the host: the HIP keywords are
// defined away, blockIdx / threadIdx are plain variables that a loop sets, and every thread of every block of a launch runs
// in turn, with the arguments and the grid ce_launch_tensor makes (tensor_ladder.h).  Built with -fsanitize=address,undefined
// by tests/test_tensor_kernel_host_cpu.py: the source is allocated at exactly its extent, `src_off` elements after a 16-byte
// boundary, and the slots at exactly theirs, `dst_off` bytes after one with a guard in front, so a load outside the source or
// a store outside the slots stops the run, and so does a wide access to an address that is not a multiple of its width.
//
// usage: tensor_kernel_host CONFIGS SOURCES OUT.  CONFIGS holds one case per line:
//   dtype slot depth quantise stride_n stride_c stride_y stride_x w h count dst_off src_off extent
// (strides, src_off and extent in elements; slot 0 u8, 1 u16 of `depth`, 2 f32).  SOURCES holds the cases' sources one after
// another, `extent` elements each; OUT receives, per case, its `count` slots.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "hip_on_host.h"

#include "tensor_kernel.h"
#include "tensor_ladder.h"

template <int DT, int SLOT>
static void run(const tensor_args &a, unsigned count)
{
    const size_t blocks = tensor_blocks(a);
    for (unsigned n = 0; n < count; n++)
        for (size_t b = 0; b < blocks; b++)
            for (unsigned t = 0; t < (unsigned)kTensorBlock; t++) {
                blockIdx.x = (unsigned)b, blockIdx.y = n, threadIdx.x = t;
                k_tensor<DT, SLOT>(a);
            }
}

int main(int argc, char **argv)
{
    if (argc != 4) return 64;
    FILE *in = fopen(argv[1], "r"), *srcs = fopen(argv[2], "rb"), *out = fopen(argv[3], "wb");
    if (!in || !srcs || !out) return 65;
    int dtype, slot, depth, quantise;
    long long sn, sc, sy, sx;
    unsigned w, h, count, dst_off, src_off;
    unsigned long long extent;
    int cases = 0;
    while (fscanf(in, "%d %d %d %d %lld %lld %lld %lld %u %u %u %u %u %llu", &dtype, &slot, &depth, &quantise, &sn, &sc, &sy, &sx, &w, &h, &count, &dst_off,
                  &src_off, &extent) == 14) {
        const size_t es = (size_t)tensor_elem_bytes(dtype), src_bytes = (size_t)extent * es, front = (size_t)src_off * es;
        uint8_t *src = static_cast<uint8_t *>(malloc(front + src_bytes));  // malloc: 16-byte aligned
        if (!src || (reinterpret_cast<uintptr_t>(src) & 15)) return 67;
        if (fread(src + front, 1, src_bytes, srcs) != src_bytes) return 66;
        const size_t slot_bytes = (size_t)w * h * 3 * (size_t)tensor_out_bytes(slot);
        uint8_t *slab = static_cast<uint8_t *>(malloc(count * slot_bytes + dst_off));
        if (!slab || (reinterpret_cast<uintptr_t>(slab) & 15)) return 68;
        memset(slab, 0xEE, count * slot_bytes + dst_off);
        const tensor_args a = tensor_make_args(dtype, quantise, src + front, sn, sc, sy, sx, w, h, count, slab + dst_off, slot_bytes, slot, (uint32_t)depth);
        const bool known = tensor_ladder(dtype, slot, [&](auto dt, auto sl) { run<decltype(dt)::value, decltype(sl)::value>(a, count); });
        if (!known) return 69;
        for (unsigned i = 0; i < dst_off; i++)
            if (slab[i] != 0xEE) {
                fprintf(stderr, "case %d wrote in front of its slots\n", cases);
                return 2;
            }
        fwrite(slab + dst_off, 1, count * slot_bytes, out);
        free(slab);
        free(src);
        cases++;
    }
    fclose(in);
    fclose(srcs);
    fclose(out);
    printf("%d\n", cases);
    return 0;
}
