// The device code of the fused Y'CbCr + HLG ingest (yuv_hlg.hip): k_yuv_cicp's frame - yuv_kernel.h's block (loads,
// integer upsampling, int64 matrix), store24 with its four residues, the cropped-group path and the odd-height last row -
// with hlg_pixel.h's pixel in cicp_pixel's place.  Kept, like the headers it builds on, free of anything but the HIP
// keywords, min / max, float2 / float4 and blockIdx / threadIdx, so that tests/cpp/hlg_kernel_host.cpp can compile the same
// text for the host and run it under the host sanitizers.  Compiled with -ffp-contract=off on the device and on the host.
#pragma once

#include "hlg_pixel.h"
#include "yuv_cicp_kernel.h"

namespace {

struct yuv_hlg_args {
    yuv_args y;  // y.m = h.c.maxv = 2^(the HLG description's depth) - 1: the integer RGB grid between the two halves
    hlg_args h;  // table, maxv, m, dst (the slot) and the five doubles; c.src and c.n_pixels are not read
};

// BPS: bytes per input sample; SUB: enum ce_yuv_subsampling; SEMI: interleaved CbCr; MATRIX: primaries other than 1.
// The grid and the thread's 8 x 2 block are k_yuv's.  A cropped group (x0 + 8 > w) stores sample by sample; the second
// row of an odd height's last pair repeats the first's loads (yuv_block) and is neither converted nor stored.
template <int BPS, int SUB, bool SEMI, bool MATRIX>
__global__ __launch_bounds__(64) void k_yuv_hlg(const yuv_hlg_args a)
{
    const uint32_t gw = (a.y.w + 7) / 8, gh = (a.y.h + 1) / 2;
    const size_t tid = (size_t)blockIdx.x * 64 + threadIdx.x;
    if (tid >= (size_t)gw * gh) return;
    const uint32_t gy = (uint32_t)(tid / gw), gx = (uint32_t)(tid - (size_t)gy * gw);
    const uint32_t x0 = gx * 8, y0 = gy * 2;

    int Y[2][8], CB[2][8], CR[2][8];
    yuv_block<BPS, SUB, SEMI>(a.y, gx, gy, Y, CB, CR);

    const bool full = x0 + 8 <= a.y.w;
#pragma unroll
    for (int j = 0; j < 2; j++) {
        const uint32_t y = y0 + j;
        if (y >= a.y.h) break;
        uint32_t smp[24];
#pragma unroll
        for (int k = 0; k < 8; k++) yuv_matrix_px(a.y, Y[j][k], CB[j][k], CR[j][k], smp[3 * k], smp[3 * k + 1], smp[3 * k + 2]);
        float o[24];
#pragma unroll
        for (int k = 0; k < 8; k++) {
            float px[3];
            hlg_pixel<MATRIX>(a.h, smp[3 * k], smp[3 * k + 1], smp[3 * k + 2], px);
            o[3 * k] = px[0], o[3 * k + 1] = px[1], o[3 * k + 2] = px[2];
        }
        float *p = a.h.c.dst + ((size_t)y * a.y.w + x0) * 3;
        if (full) {
            store24(p, o);
        } else {
#pragma unroll
            for (int k = 0; k < 8; k++) {
                if (x0 + k < a.y.w) {
#pragma unroll
                    for (int c = 0; c < 3; c++) p[3 * k + c] = o[3 * k + c];
                }
            }
        }
    }
}

}  // namespace
