// The device code of the alpha compositor (alpha.hip), kept free of anything but the HIP keywords, min, uint2 / uint4 and
// blockIdx / threadIdx, so that tests/cpp/alpha_kernel_host.cpp can compile the same text for the host - thread and block
// indices as loop variables - and run it under the host sanitizers against a source and slots allocated at exactly their
// size.
#pragma once

#include <cstddef>
#include <cstdint>

#include "ce_metrics.h"

namespace {

constexpr int kAlphaBlock = 64;  // threads per block: a 768 x 512 image is 384 (u8 slots) or 768 (u16 slots) waves

struct alpha_args {
    const void *src;      // packed RGBA, u8 or u16 samples, 16-byte aligned
    uint8_t *dst;         // slot 0; slot k starts slot_bytes further on
    size_t slot_bytes;    // n_pixels * 3 * bytes per output sample
    size_t n_pixels;
    uint32_t n_bg;        // 1 .. CE_MAX_BACKGROUNDS
    uint32_t bg[CE_MAX_BACKGROUNDS][3];  // <= 2^DEPTH - 1, checked by the host
};

// (c a + bg (m - a) + (m >> 1)) / m with c, a <= m: at most m * m + (m >> 1) < 2^32.  M is a constant of the
// instantiation, so the division is the compiler's exact multiply-high sequence, not a reciprocal in floating point.
template <uint32_t M>
__device__ __forceinline__ uint32_t over(uint32_t c, uint32_t a, uint32_t na_bg_plus_half)
{
    return (c * a + na_bg_plus_half) / M;
}

// 48 bytes (12 dwords) to p in the widest stores its address allows; the same choice for every thread of a launch and
// slot, since a group starts a multiple of 48 bytes into its slot
template <bool DST16>
__device__ __forceinline__ void store48(uint8_t *p, const uint32_t (&o)[12])
{
    const uintptr_t addr = reinterpret_cast<uintptr_t>(p);
    if ((addr & 15) == 0) {
#pragma unroll
        for (int i = 0; i < 3; i++) reinterpret_cast<uint4 *>(p)[i] = make_uint4(o[4 * i], o[4 * i + 1], o[4 * i + 2], o[4 * i + 3]);
    } else if ((addr & 7) == 0) {
#pragma unroll
        for (int i = 0; i < 6; i++) reinterpret_cast<uint2 *>(p)[i] = make_uint2(o[2 * i], o[2 * i + 1]);
    } else if ((addr & 3) == 0) {
#pragma unroll
        for (int i = 0; i < 12; i++) reinterpret_cast<uint32_t *>(p)[i] = o[i];
    } else if (DST16 || (addr & 1) == 0) {  // a u16 slot is 2-byte aligned by its type
#pragma unroll
        for (int i = 0; i < 12; i++) {
            reinterpret_cast<uint16_t *>(p)[2 * i] = (uint16_t)o[i];
            reinterpret_cast<uint16_t *>(p)[2 * i + 1] = (uint16_t)(o[i] >> 16);
        }
    } else {
#pragma unroll
        for (int i = 0; i < 12; i++) {
            p[4 * i] = (uint8_t)o[i], p[4 * i + 1] = (uint8_t)(o[i] >> 8);
            p[4 * i + 2] = (uint8_t)(o[i] >> 16), p[4 * i + 3] = (uint8_t)(o[i] >> 24);
        }
    }
}

// SRC16: u16 RGBA samples of DEPTH bits (larger values clamped, as deep ingest does), else u8; DST16: u16 slots, else u8
// (SRC16 implies DST16; !SRC16 implies DEPTH = 8).  A thread composites one group of G pixels - 48 bytes of every slot -
// over each background in turn from the registers its 16-byte loads filled; the last n_pixels % G pixels go sample by
// sample, one pixel to a thread of block 0.
template <bool SRC16, bool DST16, int DEPTH>
__global__ __launch_bounds__(kAlphaBlock) void k_alpha(const alpha_args a)
{
    static_assert(DST16 || !SRC16, "u16 samples need a u16 slot");
    static_assert(SRC16 || DEPTH == 8, "u8 samples are depth 8");
    constexpr uint32_t M = (1u << DEPTH) - 1u, HALF = M >> 1;
    constexpr int G = DST16 ? 8 : 16;       // pixels per group: 48 bytes of output
    constexpr int NL = SRC16 ? 4 : G / 4;   // 16-byte loads per group
    constexpr int OB = DST16 ? 2 : 1;       // bytes per output sample
    const size_t n_groups = a.n_pixels / G;
    const size_t tid = (size_t)blockIdx.x * kAlphaBlock + threadIdx.x;

    if (tid < n_groups) {
        uint32_t s[4 * NL];
        const uint4 *s4 = reinterpret_cast<const uint4 *>(a.src) + (size_t)NL * tid;
#pragma unroll
        for (int i = 0; i < NL; i++) {
            const uint4 v = s4[i];
            s[4 * i] = v.x, s[4 * i + 1] = v.y, s[4 * i + 2] = v.z, s[4 * i + 3] = v.w;
        }
        uint32_t c[G][3], al[G];
#pragma unroll
        for (int j = 0; j < G; j++) {
            if (SRC16) {
                c[j][0] = min(s[2 * j] & 0xffffu, M), c[j][1] = min(s[2 * j] >> 16, M);
                c[j][2] = min(s[2 * j + 1] & 0xffffu, M), al[j] = min(s[2 * j + 1] >> 16, M);
            } else {
                c[j][0] = s[j] & 255u, c[j][1] = (s[j] >> 8) & 255u, c[j][2] = (s[j] >> 16) & 255u, al[j] = s[j] >> 24;
            }
        }
        for (uint32_t k = 0; k < a.n_bg; k++) {
            const uint32_t bg0 = a.bg[k][0], bg1 = a.bg[k][1], bg2 = a.bg[k][2];
            uint32_t smp[3 * G];
#pragma unroll
            for (int j = 0; j < G; j++) {
                const uint32_t na = M - al[j];
                smp[3 * j] = over<M>(c[j][0], al[j], bg0 * na + HALF);
                smp[3 * j + 1] = over<M>(c[j][1], al[j], bg1 * na + HALF);
                smp[3 * j + 2] = over<M>(c[j][2], al[j], bg2 * na + HALF);
            }
            uint32_t o[12];
#pragma unroll
            for (int i = 0; i < 12; i++)
                o[i] = DST16 ? smp[2 * i] | (smp[2 * i + 1] << 16)
                             : smp[4 * i] | (smp[4 * i + 1] << 8) | (smp[4 * i + 2] << 16) | (smp[4 * i + 3] << 24);
            store48<DST16>(a.dst + (size_t)k * a.slot_bytes + tid * 48, o);
        }
    }

    const size_t i = n_groups * G + tid;  // tid < G <= kAlphaBlock: block 0 only
    if (tid < (size_t)G && i < a.n_pixels) {
        uint32_t c[3], al;
        if (SRC16) {
            const uint16_t *p = reinterpret_cast<const uint16_t *>(a.src) + 4 * i;
            c[0] = min((uint32_t)p[0], M), c[1] = min((uint32_t)p[1], M), c[2] = min((uint32_t)p[2], M), al = min((uint32_t)p[3], M);
        } else {
            const uint8_t *p = reinterpret_cast<const uint8_t *>(a.src) + 4 * i;
            c[0] = p[0], c[1] = p[1], c[2] = p[2], al = p[3];
        }
        const uint32_t na = M - al;
        for (uint32_t k = 0; k < a.n_bg; k++) {
            uint8_t *p = a.dst + (size_t)k * a.slot_bytes + i * (3 * OB);
#pragma unroll
            for (int ch = 0; ch < 3; ch++) {
                const uint32_t v = over<M>(c[ch], al, a.bg[k][ch] * na + HALF);
                if (DST16) reinterpret_cast<uint16_t *>(p)[ch] = (uint16_t)v;
                else p[ch] = (uint8_t)v;
            }
        }
    }
}

}  // namespace
