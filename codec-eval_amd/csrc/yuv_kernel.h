// The device code of the Y'CbCr ingest (yuv.hip), kept free of anything but the HIP keywords, min / max, uint2 / uint4 and
// blockIdx / threadIdx, so that tests/cpp/yuv_kernel_host.cpp can compile the same text for the host - thread and block
// indices as loop variables - and run it under the host sanitizers against planes allocated at exactly their size.  Its
// loads, upsampling and matrix (yuv_block, yuv_matrix_px) also serve the fused linear-light ingest, yuv_cicp_kernel.h.
#pragma once

#include <cstddef>
#include <cstdint>

#include "ce_metrics.h"

namespace {

struct yuv_args {
    const uint8_t *p0, *p1, *p2;
    size_t pitch0, pitch1, pitch2;
    uint32_t w, h, cw, ch;  // chroma plane size in samples (4:4:4: w x h)
    uint32_t shift, maxv;   // a sample is min(v >> shift, maxv)
    int triangle;
    int64_t ky, krv, kgu, kgv, kbu, y0, c0, m;
};

template <int BPS>
__device__ __forceinline__ uint32_t ld_sample(const uint8_t *row, uint32_t i)
{
    if (BPS == 1) return row[i];
    return reinterpret_cast<const uint16_t *>(row)[i];
}

// NR x NC chroma samples at rows r[] and columns clamp(col0 + k, 0, cw - 1)
template <int BPS, bool SEMI, int NR, int NC>
__device__ __forceinline__ void ld_chroma(const yuv_args &a, const uint32_t (&r)[NR], int col0, int (&cb)[NR][NC], int (&cr)[NR][NC])
{
#pragma unroll
    for (int j = 0; j < NR; j++) {
#pragma unroll
        for (int k = 0; k < NC; k++) {
            const uint32_t i = (uint32_t)min(max(col0 + k, 0), (int)a.cw - 1);
            uint32_t u, v;
            if (SEMI) {
                const uint8_t *p = a.p1 + (size_t)r[j] * a.pitch1 + (size_t)i * (2 * BPS);
                if (BPS == 1) {  // the pitch may be odd: no alignment is promised
                    uint16_t pair;
                    __builtin_memcpy(&pair, p, 2);
                    u = pair & 255u, v = pair >> 8;
                } else {  // 2-byte aligned
                    const uint16_t *q = reinterpret_cast<const uint16_t *>(p);
                    uint32_t pair;
                    __builtin_memcpy(&pair, q, 4);
                    u = pair & 0xffffu, v = pair >> 16;
                }
            } else {
                u = ld_sample<BPS>(a.p1 + (size_t)r[j] * a.pitch1, i);
                v = ld_sample<BPS>(a.p2 + (size_t)r[j] * a.pitch2, i);
            }
            cb[j][k] = (int)min(u >> a.shift, a.maxv);
            cr[j][k] = (int)min(v >> a.shift, a.maxv);
        }
    }
}

// the 8 luma samples of row y from column x0 on (zeros past the row's end)
template <int BPS>
__device__ __forceinline__ void ld_luma(const yuv_args &a, uint32_t y, uint32_t x0, int (&out)[8])
{
    const uint8_t *row = a.p0 + (size_t)y * a.pitch0;
    if (a.w >= 8) {  // the same for every thread: one wide load at a start clamped into the row, then a per-lane shift
        const uint32_t xs = min(x0, a.w - 8u), sh = x0 - xs;
        if (BPS == 1) {
            uint64_t v;
            __builtin_memcpy(&v, row + xs, 8);
            v >>= 8 * sh;
#pragma unroll
            for (int k = 0; k < 8; k++) out[k] = (int)((v >> (8 * k)) & 255u);
        } else {
            uint64_t lo, hi;
            const uint16_t *p = reinterpret_cast<const uint16_t *>(row) + xs;
            __builtin_memcpy(&lo, p, 8);
            __builtin_memcpy(&hi, p + 4, 8);
            const uint32_t s = 16 * sh;  // 0 .. 112
            const uint64_t lo1 = s == 0 ? lo : s < 64 ? (lo >> s) | (hi << (64 - s)) : hi >> (s - 64);
            const uint64_t hi1 = s < 64 ? hi >> s : 0;
#pragma unroll
            for (int k = 0; k < 4; k++) {
                out[k] = (int)((lo1 >> (16 * k)) & 0xffffu);
                out[4 + k] = (int)((hi1 >> (16 * k)) & 0xffffu);
            }
        }
    } else {
#pragma unroll
        for (int k = 0; k < 8; k++) out[k] = (int)ld_sample<BPS>(row, min(x0 + k, a.w - 1u));
    }
#pragma unroll
    for (int k = 0; k < 8; k++) out[k] = (int)min((uint32_t)out[k] >> a.shift, a.maxv);
}

__device__ __forceinline__ uint32_t clamp_m(int64_t v, int64_t m) { return (uint32_t)(v < 0 ? 0 : v > m ? m : v); }

// The block of group (gx, gy) before the matrix: its 2 x 8 luma samples and its chroma at full resolution (the upsampling of
// include/ce_metrics.h).  Every load goes through ld_luma / ld_chroma, whose clamped indices keep it inside the planes.
// Shared by k_yuv and k_yuv_tagged (yuv_cicp_kernel.h).
template <int BPS, int SUB, bool SEMI>
__device__ __forceinline__ void yuv_block(const yuv_args &a, uint32_t gx, uint32_t gy, int (&Y)[2][8], int (&CB)[2][8], int (&CR)[2][8])
{
    const uint32_t x0 = gx * 8, y0 = gy * 2;
    const uint32_t y1 = min(y0 + 1, a.h - 1);  // odd height: the second row repeats the first's loads and is not stored
    ld_luma<BPS>(a, y0, x0, Y[0]);
    ld_luma<BPS>(a, y1, x0, Y[1]);

    if (SUB == CE_YUV_400) {
#pragma unroll
        for (int j = 0; j < 2; j++)
#pragma unroll
            for (int k = 0; k < 8; k++) CB[j][k] = CR[j][k] = (int)a.c0;
    } else if (SUB == CE_YUV_444) {
        const uint32_t r[2] = {y0, y1};
        ld_chroma<BPS, SEMI, 2, 8>(a, r, (int)x0, CB, CR);
    } else {
        // columns 4 gx - 1 .. 4 gx + 4; rows: 4:2:0 the pair's chroma row and its two neighbours, 4:2:2 the two output rows
        constexpr int NR = SUB == CE_YUV_420 ? 3 : 2;
        int cb[NR][6], cr[NR][6];
        uint32_t r[NR];
        if (SUB == CE_YUV_420) {
            r[0] = a.triangle ? (gy > 0 ? gy - 1 : 0) : gy;
            r[1] = gy;
            r[NR - 1] = a.triangle ? min(gy + 1, a.ch - 1) : gy;
        } else {
            r[0] = y0, r[1] = y1;
        }
        ld_chroma<BPS, SEMI, NR, 6>(a, r, (int)(4 * gx) - 1, cb, cr);
#pragma unroll
        for (int j = 0; j < 2; j++) {
            int tb[6], tr[6];
#pragma unroll
            for (int k = 0; k < 6; k++) {
                if (SUB == CE_YUV_420) {
                    tb[k] = 3 * cb[1][k] + cb[j == 0 ? 0 : NR - 1][k];
                    tr[k] = 3 * cr[1][k] + cr[j == 0 ? 0 : NR - 1][k];
                } else {
                    tb[k] = cb[j][k], tr[k] = cr[j][k];
                }
            }
            constexpr int even_add = SUB == CE_YUV_420 ? 8 : 1, odd_add = SUB == CE_YUV_420 ? 7 : 2, sh = SUB == CE_YUV_420 ? 4 : 2;
#pragma unroll
            for (int k = 0; k < 4; k++) {
                const int c_b = tb[k + 1], c_r = tr[k + 1];
                const int lb = a.triangle ? tb[k] : c_b, rb = a.triangle ? tb[k + 2] : c_b;
                const int lr = a.triangle ? tr[k] : c_r, rr = a.triangle ? tr[k + 2] : c_r;
                CB[j][2 * k] = (3 * c_b + lb + even_add) >> sh;
                CB[j][2 * k + 1] = (3 * c_b + rb + odd_add) >> sh;
                CR[j][2 * k] = (3 * c_r + lr + even_add) >> sh;
                CR[j][2 * k + 1] = (3 * c_r + rr + odd_add) >> sh;
            }
        }
    }
}

// one pixel through the fixed-point matrix: R, G, B in [0, a.m]
__device__ __forceinline__ void yuv_matrix_px(const yuv_args &a, int y, int cb, int cr, uint32_t &r, uint32_t &g, uint32_t &b)
{
    const int64_t yy = a.ky * ((int64_t)y - a.y0) + 32768;
    const int64_t u = (int64_t)cb - a.c0, v = (int64_t)cr - a.c0;
    r = clamp_m((yy + a.krv * v) >> 16, a.m);
    g = clamp_m((yy - a.kgu * u - a.kgv * v) >> 16, a.m);
    b = clamp_m((yy + a.kbu * u) >> 16, a.m);
}

// BPS: bytes per input sample; OUT16: u16 output (a deep batch); SUB: enum ce_yuv_subsampling; SEMI: interleaved CbCr
template <int BPS, bool OUT16, int SUB, bool SEMI>
__global__ __launch_bounds__(64) void k_yuv(const yuv_args a, uint8_t *__restrict__ dst)
{
    const uint32_t gw = (a.w + 7) / 8, gh = (a.h + 1) / 2;
    const size_t tid = (size_t)blockIdx.x * 64 + threadIdx.x;
    if (tid >= (size_t)gw * gh) return;
    const uint32_t gy = (uint32_t)(tid / gw), gx = (uint32_t)(tid - (size_t)gy * gw);
    const uint32_t x0 = gx * 8, y0 = gy * 2;

    int Y[2][8], CB[2][8], CR[2][8];
    yuv_block<BPS, SUB, SEMI>(a, gx, gy, Y, CB, CR);

    constexpr int OB = OUT16 ? 2 : 1;        // bytes per output sample
    constexpr int NW = 24 * OB / 4;          // dwords per block row
    const bool full = x0 + 8 <= a.w;
#pragma unroll
    for (int j = 0; j < 2; j++) {
        uint32_t smp[24];
#pragma unroll
        for (int k = 0; k < 8; k++) yuv_matrix_px(a, Y[j][k], CB[j][k], CR[j][k], smp[3 * k], smp[3 * k + 1], smp[3 * k + 2]);
        const uint32_t y = y0 + j;
        if (y >= a.h) break;
        uint8_t *p = dst + ((size_t)y * a.w + x0) * (3 * OB);
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
            for (int k = 0; k < 8; k++) {
                if (x0 + k < a.w) {
#pragma unroll
                    for (int c = 0; c < 3; c++) {
                        if (OUT16) reinterpret_cast<uint16_t *>(p)[3 * k + c] = (uint16_t)smp[3 * k + c];
                        else p[3 * k + c] = (uint8_t)smp[3 * k + c];
                    }
                }
            }
        }
    }
}

}  // namespace
