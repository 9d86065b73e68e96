// The device code of the fused ingest of Y'CbCr planes with an ICC profile (yuv_icc.hip): yuv_kernel.h's
// block (loads, integer upsampling, int64 matrix) followed by an ICC pixel - icc_pixel.h's icc_px or icc_lut_pixel.h's
// icc_lut_px - and the store of the slot's kind.  A linear slot is yuv_cicp_kernel.h's k_yuv_tagged with that pixel, unchanged.
// An integer slot is the frame below, k_yuv_icc_encode: k_yuv's grid and stores around the pixel and icc_kernel.h's search of
// the sRGB code thresholds.  Kept, like the headers it builds on, free of anything but the HIP keywords, min / max, uint2 /
// uint4 and blockIdx / threadIdx, so that tests/cpp/yuv_icc_kernel_host.cpp can compile the same text for the host and run it
// under the host sanitizers.  Compiled with -ffp-contract=off on the device and on the host.
#pragma once

#include "icc_kernel.h"
#include "icc_lut_pixel.h"
#include "yuv_cicp_kernel.h"

namespace {

// What k_yuv_icc_encode is launched with: the planes and the pixel as k_yuv_tagged takes them (y.m = the pixel's maxv =
// 2^rgb_depth - 1 is the integer RGB grid between the two halves; nothing of the pixel's frame() is read), then the slot -
// packed u8 RGB, or with OUT16 packed u16 RGB - and the thresholds of the slot's depth D: thr[1 .. 2^D - 1], top = 2^(D - 1).
template <class Pixel>
struct yuv_icc_args {
    yuv_args y;
    Pixel px;
    uint8_t *dst;
    const float *thr;
    uint32_t top;
};

// How many pixels' searches run side by side: 4 pixels are twelve searches, k_icc_encode's count, so that a step's gathers do
// not wait for each other.  A row of a block is two such batches.  A whole row at once (24 searches) was measured and is
// slower in every integer instantiation but one.
constexpr int kYuvIccBatch = 4;

// BPS: bytes per input sample; OUT16: u16 output (a deep side); SUB: enum ce_yuv_subsampling; SEMI: interleaved CbCr; Pixel:
// icc_px<MATRIX> or icc_lut_px<TETRA>.  The grid, the thread's 8 x 2 block and the stores are k_yuv's: a full group's row goes
// out as 16-byte (u16) or 8-byte (u8) stores where its address allows, else as dwords; a cropped group (x0 + 8 > w) or a row
// that is not 4-byte aligned goes sample by sample.  The second row of an odd height's last pair repeats the first's loads
// (yuv_block) and is neither converted nor stored.  thr[0] is never read: every gather is at pos + step >= 1.
//
// The two rows and a row's two batches are loops that stay rolled, so a kernel holds the pixel four times and not sixteen:
// the LUT pixel with its six curves is large, sixteen copies of it are past what the compiler will unroll, and what it then
// leaves indexed by the loop counter goes to scratch.  Nothing here is indexed by a loop counter: the batch at work is
// always elements 0 .. 3 of the row at work, and the rest moves down behind it (the codes found so far likewise), which is
// a few register moves per batch.
template <int BPS, bool OUT16, int SUB, bool SEMI, class Pixel>
__global__ __launch_bounds__(64) void k_yuv_icc_encode(const yuv_icc_args<Pixel> k)
{
    const yuv_args &a = k.y;
    const Pixel &px = k.px;
    const float *__restrict__ thr = k.thr;
    const uint32_t gw = (a.w + 7) / 8, gh = (a.h + 1) / 2;
    const size_t tid = (size_t)blockIdx.x * 64 + threadIdx.x;
    if (tid >= (size_t)gw * gh) return;
    const uint32_t gy = (uint32_t)(tid / gw), gx = (uint32_t)(tid - (size_t)gy * gw);
    const uint32_t x0 = gx * 8, y0 = gy * 2;

    int Y[2][8], CB[2][8], CR[2][8];
    yuv_block<BPS, SUB, SEMI>(a, gx, gy, Y, CB, CR);

    constexpr int OB = OUT16 ? 2 : 1;  // bytes per output sample
    constexpr int NW = 24 * OB / 4;    // dwords per block row
    constexpr int NP = kYuvIccBatch, NS = 3 * NP;
    static_assert(2 * NP == 8, "a row is two batches");
    const bool full = x0 + 8 <= a.w;
    const uint32_t rows = y0 + 1 < a.h ? 2u : 1u;
#pragma unroll 1
    for (uint32_t j = 0; j < rows; j++) {
        const uint32_t y = y0 + j;
        uint32_t smp[24] = {};
#pragma unroll 1
        for (int g = 0; g < 2; g++) {
            float x[NS];
#pragma unroll
            for (int p = 0; p < NP; p++) {
                uint32_t r, gr, b;
                yuv_matrix_px(a, Y[0][p], CB[0][p], CR[0][p], r, gr, b);
                float v[3];
                px(r, gr, b, v);
                x[3 * p] = v[0], x[3 * p + 1] = v[1], x[3 * p + 2] = v[2];
            }
            // icc_encode on the batch's values side by side
            uint32_t c[NS] = {};
            for (uint32_t step = k.top; step != 0; step >>= 1) {
#pragma unroll
                for (int i = 0; i < NS; i++) c[i] += x[i] >= thr[c[i] + step] ? step : 0u;
            }
#pragma unroll
            for (int i = 0; i < NS; i++) smp[i] = smp[NS + i], smp[NS + i] = c[i];
#pragma unroll
            for (int p = 0; p < NP; p++) Y[0][p] = Y[0][NP + p], CB[0][p] = CB[0][NP + p], CR[0][p] = CR[0][NP + p];
        }
#pragma unroll
        for (int i = 0; i < 8; i++) Y[0][i] = Y[1][i], CB[0][i] = CB[1][i], CR[0][i] = CR[1][i];
        uint8_t *p = k.dst + ((size_t)y * a.w + x0) * (3 * OB);
        const uintptr_t addr = reinterpret_cast<uintptr_t>(p);
        if (full && (addr & 3) == 0) {
            uint32_t o[NW];
#pragma unroll
            for (int i = 0; i < NW; i++)
                o[i] = OUT16 ? smp[2 * i] | (smp[2 * i + 1] << 16)
                             : smp[4 * i] | (smp[4 * i + 1] << 8) | (smp[4 * i + 2] << 16) | (smp[4 * i + 3] << 24);
            if (OUT16 && (addr & 15) == 0) {
#pragma unroll
                for (int i = 0; i < 3; i++) reinterpret_cast<uint4 *>(p)[i] = make_uint4(o[4 * i], o[4 * i + 1], o[4 * i + 2], o[4 * i + 3]);
            } else if (!OUT16 && (addr & 7) == 0) {
#pragma unroll
                for (int i = 0; i < 3; i++) reinterpret_cast<uint2 *>(p)[i] = make_uint2(o[2 * i], o[2 * i + 1]);
            } else {
#pragma unroll
                for (int i = 0; i < NW; i++) reinterpret_cast<uint32_t *>(p)[i] = o[i];
            }
        } else {
#pragma unroll
            for (int s = 0; s < 8; s++) {
                if (x0 + s < a.w) {
#pragma unroll
                    for (int ch = 0; ch < 3; ch++) {
                        if (OUT16) reinterpret_cast<uint16_t *>(p)[3 * s + ch] = (uint16_t)smp[3 * s + ch];
                        else p[3 * s + ch] = (uint8_t)smp[3 * s + ch];
                    }
                }
            }
        }
    }
}

}  // namespace
