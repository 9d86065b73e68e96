// The device code of the tensor ingest (tensor.hip), kept free of anything but the HIP keywords, min, uint2 / uint4 and
// blockIdx / threadIdx, so that tests/cpp/tensor_kernel_host.cpp can compile the same text for the host - thread and block
// indices as loop variables - and run it under the host sanitizers against sources and slots allocated at exactly their
// extent.
#pragma once

#include <cstddef>
#include <cstdint>

#include "ce_metrics.h"

namespace {

constexpr int kTensorBlock = 64;  // threads per block: a 768 x 512 image is 384 (u8 slots), 768 (u16) or 1536 (f32) waves

enum { TENSOR_SLOT_U8 = 0, TENSOR_SLOT_U16 = 1, TENSOR_SLOT_LIN = 2 };
// how a full group reads its pixels, one choice per launch made on the host (tensor_ladder.h: tensor_pick_path)
enum { TENSOR_PATH_GENERAL = 0, TENSOR_PATH_PLANAR = 1, TENSOR_PATH_INTERLEAVED = 2 };

constexpr int tensor_elem_bytes(int dtype) { return dtype == CE_DTYPE_U8 ? 1 : dtype == CE_DTYPE_F32 ? 4 : 2; }
constexpr int tensor_out_bytes(int slot) { return slot == TENSOR_SLOT_U8 ? 1 : slot == TENSOR_SLOT_U16 ? 2 : 4; }
// pixels of one row a thread owns: 48 bytes of its slot
constexpr int tensor_group(int slot) { return 16 / tensor_out_bytes(slot); }
// bytes per load of the two fast paths: a group's elements of one plane are 8 (u8 -> u16, half -> f32), 16, 32 or 64 bytes
constexpr int tensor_load_bytes(int dtype, int slot) { return tensor_group(slot) * tensor_elem_bytes(dtype) >= 16 ? 16 : 8; }

struct tensor_args {
    const uint8_t *src;      // element (n = 0, c = 0, y = 0, x = 0), aligned to its element size
    int64_t sn, sc, sy, sx;  // strides in elements, all >= 0, sy and sx >= 1
    uint8_t *dst;            // slot of image 0; image n's starts n * slot_bytes further on
    size_t slot_bytes;
    uint32_t w, h;
    uint32_t gpr;            // groups per row: ceil(w / G)
    uint32_t m;              // integer slots: 2^D - 1
    float fm;                // f32(m)
    uint32_t truncate;       // CE_QUANT_TRUNCATE
    uint32_t path;           // TENSOR_PATH_*
};

__device__ __forceinline__ float tensor_bits_to_float(uint32_t u)
{
    float f;
    __builtin_memcpy(&f, &u, 4);
    return f;
}
__device__ __forceinline__ uint32_t tensor_float_to_bits(float f)
{
    uint32_t u;
    __builtin_memcpy(&u, &f, 4);
    return u;
}

// the element's bits, zero-extended -> f32, exactly
template <int DT>
__device__ __forceinline__ float tensor_widen(uint32_t r)
{
    if constexpr (DT == CE_DTYPE_F32) {
        return tensor_bits_to_float(r);
    } else if constexpr (DT == CE_DTYPE_BF16) {
        return tensor_bits_to_float(r << 16);
    } else {
#if defined(__HIPCC__)
        const uint16_t b = (uint16_t)r;  // the hardware conversion
        _Float16 hv;
        __builtin_memcpy(&hv, &b, 2);
        return (float)hv;
#else
        const uint32_t s = (r & 0x8000u) << 16, e = (r >> 10) & 31u, f = r & 1023u;
        if (e == 0) return tensor_bits_to_float(s | tensor_float_to_bits((float)f * 5.9604644775390625e-08f));  // f * 2^-24
        if (e == 31) return tensor_bits_to_float(s | 0x7f800000u | (f << 13));
        return tensor_bits_to_float(s | ((e + 112u) << 23) | (f << 13));
#endif
    }
}

// the header's per-sample rule: the element's bits -> the slot's sample (a linear slot: the float's bits)
template <int DT, int SLOT>
__device__ __forceinline__ uint32_t tensor_sample(uint32_t r, const tensor_args &a)
{
    if constexpr (DT == CE_DTYPE_U8) {
        return r;
    } else if constexpr (DT == CE_DTYPE_U16) {
        return min(r, a.m);
    } else {
        const float v = tensor_widen<DT>(r);
        if constexpr (SLOT == TENSOR_SLOT_LIN) {
            if (v != v) return 0u;
            return tensor_float_to_bits(v > CE_LINEAR_MAX ? CE_LINEAR_MAX : (v < -CE_LINEAR_MAX ? -CE_LINEAR_MAX : v));
        } else {
            const float c = v > 0.0f ? (v < 1.0f ? v : 1.0f) : 0.0f;
            const float p = c * a.fm;
            return (uint32_t)(a.truncate ? __builtin_floorf(p) : __builtin_rintf(p));
        }
    }
}

// N dwords from p, which is a multiple of LW bytes, in loads of LW bytes
template <int LW, int N>
__device__ __forceinline__ void tensor_load_run(const uint8_t *p, uint32_t (&wd)[N])
{
    static_assert(N % (LW / 4) == 0, "a run is whole loads");
    if constexpr (LW == 16) {
#pragma unroll
        for (int i = 0; i < N / 4; i++) {
            const uint4 v = reinterpret_cast<const uint4 *>(p)[i];
            wd[4 * i] = v.x, wd[4 * i + 1] = v.y, wd[4 * i + 2] = v.z, wd[4 * i + 3] = v.w;
        }
    } else {
#pragma unroll
        for (int i = 0; i < N / 2; i++) {
            const uint2 v = reinterpret_cast<const uint2 *>(p)[i];
            wd[2 * i] = v.x, wd[2 * i + 1] = v.y;
        }
    }
}

// element i of a run of little-endian dwords
template <int ES, int N>
__device__ __forceinline__ uint32_t tensor_run_elem(const uint32_t (&wd)[N], int i)
{
    if constexpr (ES == 1) return (wd[i >> 2] >> (8 * (i & 3))) & 255u;
    else if constexpr (ES == 2) return (wd[i >> 1] >> (16 * (i & 1))) & 0xffffu;
    else return wd[i];
}

template <int ES>
__device__ __forceinline__ uint32_t tensor_load_elem(const uint8_t *p)
{
    if constexpr (ES == 1) return *p;
    else if constexpr (ES == 2) return *reinterpret_cast<const uint16_t *>(p);
    else return *reinterpret_cast<const uint32_t *>(p);
}

// 48 bytes (12 dwords) to p, which is a multiple of OB bytes, in the widest stores its address allows; a launch's slots and
// rows differ in alignment (slot k of an RGB8 slab starts at k * w * h * 3 bytes and a row at y * w * 3), a wave's lanes of one
// row do not
template <int OB>
__device__ __forceinline__ void tensor_store48(uint8_t *p, const uint32_t (&o)[12])
{
    const uintptr_t addr = reinterpret_cast<uintptr_t>(p);
    if ((addr & 15) == 0) {
#pragma unroll
        for (int i = 0; i < 3; i++) reinterpret_cast<uint4 *>(p)[i] = make_uint4(o[4 * i], o[4 * i + 1], o[4 * i + 2], o[4 * i + 3]);
    } else if ((addr & 7) == 0) {
#pragma unroll
        for (int i = 0; i < 6; i++) reinterpret_cast<uint2 *>(p)[i] = make_uint2(o[2 * i], o[2 * i + 1]);
    } else if (OB == 4 || (addr & 3) == 0) {
#pragma unroll
        for (int i = 0; i < 12; i++) reinterpret_cast<uint32_t *>(p)[i] = o[i];
    } else if (OB == 2 || (addr & 1) == 0) {
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

// DT: enum ce_dtype; SLOT: TENSOR_SLOT_*.  A thread owns G consecutive pixels of one row of image blockIdx.y - 48 bytes of
// that image's slot.  A full group reads them as the launch's path says: PLANAR (stride_x = 1, every plane row a multiple of
// the load width) G elements of each of the three planes in 16-byte loads (8 where the G elements are 8 bytes); INTERLEAVED
// (stride_c = 1, stride_x 3 or 4, every row a multiple of the load width) its G whole pixels as one run, the channels picked
// from the registers; GENERAL element by element at any strides.  It then converts and stores 12 dwords in the widest stores
// the address allows.  The last w % G pixels of a row go element by element and sample by sample, and so does the last group
// of an image's last row with stride_x = 4, whose run would end one element behind the last one the tensor has to own.  All
// address arithmetic is 64-bit.
template <int DT, int SLOT>
__global__ __launch_bounds__(kTensorBlock) void k_tensor(const tensor_args a)
{
    constexpr int ES = tensor_elem_bytes(DT), OB = tensor_out_bytes(SLOT), G = tensor_group(SLOT);
    constexpr int LW = tensor_load_bytes(DT, SLOT), NW = G * ES / 4;  // dwords of a group's elements of one plane
    static_assert(DT != CE_DTYPE_U8 || SLOT != TENSOR_SLOT_LIN, "integer dtypes do not enter a linear slot");
    static_assert(DT != CE_DTYPE_U16 || SLOT == TENSOR_SLOT_U16, "u16 elements need a u16 slot");
    const uint32_t t = blockIdx.x * (uint32_t)kTensorBlock + threadIdx.x;
    const uint32_t y = t / a.gpr;
    if (y >= a.h) return;
    const uint32_t x0 = (t - y * a.gpr) * (uint32_t)G;
    const int64_t n = (int64_t)blockIdx.y;
    const uint8_t *row = a.src + (n * a.sn + (int64_t)y * a.sy) * ES;
    const bool full = x0 + (uint32_t)G <= a.w;

    uint32_t raw[G][3];
    if (full && a.path == TENSOR_PATH_PLANAR) {
#pragma unroll
        for (int c = 0; c < 3; c++) {
            uint32_t wd[NW];
            tensor_load_run<LW, NW>(row + ((int64_t)c * a.sc + (int64_t)x0) * ES, wd);
#pragma unroll
            for (int j = 0; j < G; j++) raw[j][c] = tensor_run_elem<ES, NW>(wd, j);
        }
    } else if (full && a.path == TENSOR_PATH_INTERLEAVED && a.sx == 3) {
        uint32_t wd[3 * NW];
        tensor_load_run<LW, 3 * NW>(row + (int64_t)x0 * 3 * ES, wd);
#pragma unroll
        for (int j = 0; j < G; j++)
#pragma unroll
            for (int c = 0; c < 3; c++) raw[j][c] = tensor_run_elem<ES, 3 * NW>(wd, 3 * j + c);
    } else if (full && a.path == TENSOR_PATH_INTERLEAVED && !(y == a.h - 1 && x0 + (uint32_t)G == a.w)) {
        uint32_t wd[4 * NW];
        tensor_load_run<LW, 4 * NW>(row + (int64_t)x0 * 4 * ES, wd);
#pragma unroll
        for (int j = 0; j < G; j++)
#pragma unroll
            for (int c = 0; c < 3; c++) raw[j][c] = tensor_run_elem<ES, 4 * NW>(wd, 4 * j + c);
    } else {
#pragma unroll
        for (int j = 0; j < G; j++)
#pragma unroll
            for (int c = 0; c < 3; c++)
                raw[j][c] = x0 + (uint32_t)j < a.w ? tensor_load_elem<ES>(row + ((int64_t)c * a.sc + (int64_t)(x0 + (uint32_t)j) * a.sx) * ES) : 0u;
    }

    uint32_t smp[3 * G];
#pragma unroll
    for (int j = 0; j < G; j++)
#pragma unroll
        for (int c = 0; c < 3; c++) smp[3 * j + c] = tensor_sample<DT, SLOT>(raw[j][c], a);

    uint8_t *p = a.dst + (size_t)n * a.slot_bytes + ((size_t)y * a.w + x0) * (3 * OB);
    if (full) {
        uint32_t o[12];
#pragma unroll
        for (int i = 0; i < 12; i++)
            o[i] = OB == 4   ? smp[i]
                   : OB == 2 ? smp[(2 * i) % (3 * G)] | (smp[(2 * i + 1) % (3 * G)] << 16)
                             : smp[(4 * i) % (3 * G)] | (smp[(4 * i + 1) % (3 * G)] << 8) | (smp[(4 * i + 2) % (3 * G)] << 16) | (smp[(4 * i + 3) % (3 * G)] << 24);
        tensor_store48<OB>(p, o);
    } else {
#pragma unroll
        for (int j = 0; j < G; j++)
            if (x0 + (uint32_t)j < a.w) {
#pragma unroll
                for (int c = 0; c < 3; c++) {
                    const uint32_t v = smp[3 * j + c];
                    if (OB == 4) reinterpret_cast<uint32_t *>(p)[3 * j + c] = v;
                    else if (OB == 2) reinterpret_cast<uint16_t *>(p)[3 * j + c] = (uint16_t)v;
                    else p[3 * j + c] = (uint8_t)v;
                }
            }
    }
}

}  // namespace
