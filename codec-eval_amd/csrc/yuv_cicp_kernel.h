// The device code of the fused ingest of Y'CbCr planes into a linear batch, CICP and HLG (yuv_cicp.hip): yuv_kernel.h's block
// (loads, integer upsampling, int64 matrix) followed by a pixel - cicp_pixel.h's cicp_px (table gather, separately rounded
// f32 matrix, clamp of a linear image) or hlg_pixel.h's hlg_px (the same around the f64 OOTF) - with nothing but the stores
// of its own.  One frame, k_yuv_tagged, with the pixel as a parameter.  Kept, like the headers it builds on, free of anything
// but the HIP keywords, min / max, float2 / float4 and blockIdx / threadIdx, so that tests/cpp/yuv_cicp_kernel_host.cpp and
// hlg_kernel_host.cpp can compile the same text for the host and run it under the host sanitizers.  Compiled with
// -ffp-contract=off on the device and on the host.
#pragma once

#include "cicp_pixel.h"
#include "yuv_kernel.h"

namespace {

// One row of a full block, 24 floats, to p (4-byte aligned).  p is a multiple of 32 bytes past the row's start, and the
// row's start moves through all four residues mod 16 with the slot, y * w and the image's size, so the choice is made per
// row: six 16-byte stores at residue 0; at 8 an 8-byte store on either side of five 16-byte ones; at 4 and 12 the 4- and
// 8-byte stores that reach the next 16-byte boundary, five 16-byte stores and the rest.  Every store is aligned to its width.
__device__ __forceinline__ void store24(float *p, const float (&o)[24])
{
    const uint32_t r = (uint32_t)(reinterpret_cast<uintptr_t>(p) & 15);
    if (r == 0) {
#pragma unroll
        for (int i = 0; i < 6; i++) reinterpret_cast<float4 *>(p)[i] = make_float4(o[4 * i], o[4 * i + 1], o[4 * i + 2], o[4 * i + 3]);
    } else if (r == 8) {
        *reinterpret_cast<float2 *>(p) = make_float2(o[0], o[1]);
#pragma unroll
        for (int i = 0; i < 5; i++)
            reinterpret_cast<float4 *>(p + 2)[i] = make_float4(o[4 * i + 2], o[4 * i + 3], o[4 * i + 4], o[4 * i + 5]);
        *reinterpret_cast<float2 *>(p + 22) = make_float2(o[22], o[23]);
    } else if (r == 4) {
        p[0] = o[0];
        *reinterpret_cast<float2 *>(p + 1) = make_float2(o[1], o[2]);
#pragma unroll
        for (int i = 0; i < 5; i++)
            reinterpret_cast<float4 *>(p + 3)[i] = make_float4(o[4 * i + 3], o[4 * i + 4], o[4 * i + 5], o[4 * i + 6]);
        p[23] = o[23];
    } else {  // 12
        p[0] = o[0];
#pragma unroll
        for (int i = 0; i < 5; i++)
            reinterpret_cast<float4 *>(p + 1)[i] = make_float4(o[4 * i + 1], o[4 * i + 2], o[4 * i + 3], o[4 * i + 4]);
        *reinterpret_cast<float2 *>(p + 21) = make_float2(o[21], o[22]);
        p[23] = o[23];
    }
}

// What the frame is launched with: the planes and the pixel in one argument, laid out as the two structs behind each other.
// y.m = the pixel's maxv = 2^(the description's depth) - 1 is the integer RGB grid between the two halves; of the pixel's
// frame() only dst (the slot: packed f32 RGB, 4-byte aligned) is read, src and n_pixels are not.
template <class Pixel>
struct yuv_px_args {
    yuv_args y;
    Pixel px;
};

// BPS: bytes per input sample; SUB: enum ce_yuv_subsampling; SEMI: interleaved CbCr; Pixel: cicp_px<MATRIX> or
// hlg_px<MATRIX>.  The grid and the thread's 8 x 2 block are k_yuv's.  A cropped group (x0 + 8 > w) stores sample by sample;
// the second row of an odd height's last pair repeats the first's loads (yuv_block) and is neither converted nor stored.
template <int BPS, int SUB, bool SEMI, class Pixel>
__global__ __launch_bounds__(64) void k_yuv_tagged(const yuv_px_args<Pixel> k)
{
    const yuv_args &a = k.y;
    const Pixel &px = k.px;
    const uint32_t gw = (a.w + 7) / 8, gh = (a.h + 1) / 2;
    const size_t tid = (size_t)blockIdx.x * 64 + threadIdx.x;
    if (tid >= (size_t)gw * gh) return;
    const uint32_t gy = (uint32_t)(tid / gw), gx = (uint32_t)(tid - (size_t)gy * gw);
    const uint32_t x0 = gx * 8, y0 = gy * 2;

    int Y[2][8], CB[2][8], CR[2][8];
    yuv_block<BPS, SUB, SEMI>(a, gx, gy, Y, CB, CR);

    const bool full = x0 + 8 <= a.w;
#pragma unroll
    for (int j = 0; j < 2; j++) {
        const uint32_t y = y0 + j;
        if (y >= a.h) break;
        uint32_t smp[24];
#pragma unroll
        for (int k = 0; k < 8; k++) yuv_matrix_px(a, Y[j][k], CB[j][k], CR[j][k], smp[3 * k], smp[3 * k + 1], smp[3 * k + 2]);
        float o[24];
#pragma unroll
        for (int k = 0; k < 8; k++) {
            float v[3];
            px(smp[3 * k], smp[3 * k + 1], smp[3 * k + 2], v);
            o[3 * k] = v[0], o[3 * k + 1] = v[1], o[3 * k + 2] = v[2];
        }
        float *p = px.frame().dst + ((size_t)y * a.w + x0) * 3;
        if (full) {
            store24(p, o);
        } else {
#pragma unroll
            for (int k = 0; k < 8; k++) {
                if (x0 + k < a.w) {
#pragma unroll
                    for (int c = 0; c < 3; c++) p[3 * k + c] = o[3 * k + c];
                }
            }
        }
    }
}

}  // namespace
