// What a launch of a strided tensor picks at run time and its kernel wants at compile time, in one place for tensor.hip and
// the host harness (tests/cpp/tensor_kernel_host.cpp), beside packed_ladder.h and yuv_ladder.h: (dtype, slot kind) -> DT and
// SLOT of tensor_kernel.h's k_tensor, the launch-uniform choice of how full groups read, and the profile name that says what a
// dispatch moved.  Include it behind tensor_kernel.h.  Host-compilable with plain g++ -std=c++17.
#pragma once

#include <cstdio>
#include <type_traits>

#include "ce_metrics.h"

// f(dt, slot) is called once, with two std::integral_constant: the enum ce_dtype and TENSOR_SLOT_*; false, and no call, for a
// pair the header does not admit (an unknown dtype or slot, u8 or u16 into a linear slot, u16 into a u8 slot)
template <class F>
inline bool tensor_ladder(int dtype, int slot, F &&f)
{
    auto with_slot = [&](auto dt) {
        constexpr int DT = decltype(dt)::value;
        constexpr bool is_float = DT != CE_DTYPE_U8 && DT != CE_DTYPE_U16;
        switch (slot) {
            case TENSOR_SLOT_U8:
                if constexpr (DT != CE_DTYPE_U16) return f(dt, std::integral_constant<int, TENSOR_SLOT_U8>{}), true;
                return false;
            case TENSOR_SLOT_U16: return f(dt, std::integral_constant<int, TENSOR_SLOT_U16>{}), true;
            case TENSOR_SLOT_LIN:
                if constexpr (is_float) return f(dt, std::integral_constant<int, TENSOR_SLOT_LIN>{}), true;
                return false;
            default: return false;
        }
    };
    switch (dtype) {
        case CE_DTYPE_U8: return with_slot(std::integral_constant<int, CE_DTYPE_U8>{});
        case CE_DTYPE_U16: return with_slot(std::integral_constant<int, CE_DTYPE_U16>{});
        case CE_DTYPE_F16: return with_slot(std::integral_constant<int, CE_DTYPE_F16>{});
        case CE_DTYPE_BF16: return with_slot(std::integral_constant<int, CE_DTYPE_BF16>{});
        case CE_DTYPE_F32: return with_slot(std::integral_constant<int, CE_DTYPE_F32>{});
        default: return false;
    }
}

// How the full groups of a launch read, the same for every thread: a fast path needs contiguous rows and every row base - of
// every plane and image the launch covers - at a multiple of the load width; the slot's alignment is the store's own test.
inline uint32_t tensor_pick_path(int dtype, int slot, const void *data, int64_t sn, int64_t sc, int64_t sy, int64_t sx, uint32_t count)
{
    const int64_t es = tensor_elem_bytes(dtype), lw = tensor_load_bytes(dtype, slot);
    auto aligned = [&](int64_t stride) { return (stride * es) % lw == 0; };
    if (reinterpret_cast<uintptr_t>(data) % (uintptr_t)lw != 0 || !aligned(sy) || (count > 1 && !aligned(sn))) return TENSOR_PATH_GENERAL;
    if (sx == 1 && aligned(sc)) return TENSOR_PATH_PLANAR;
    if (sc == 1 && (sx == 3 || sx == 4)) return TENSOR_PATH_INTERLEAVED;
    return TENSOR_PATH_GENERAL;
}

// What ce_launch_tensor hands the kernel: `count` images of w x h at `data` with their strides in elements into slots slot_bytes
// apart from dst on; depth is read for TENSOR_SLOT_U16 only
inline tensor_args tensor_make_args(int dtype, int quantise, const void *data, int64_t sn, int64_t sc, int64_t sy, int64_t sx, uint32_t w, uint32_t h,
                                    uint32_t count, void *dst, size_t slot_bytes, int slot, uint32_t depth)
{
    const uint32_t G = (uint32_t)tensor_group(slot);
    tensor_args a{};
    a.src = static_cast<const uint8_t *>(data);
    a.sn = sn, a.sc = sc, a.sy = sy, a.sx = sx;
    a.dst = static_cast<uint8_t *>(dst), a.slot_bytes = slot_bytes;
    a.w = w, a.h = h, a.gpr = (w + G - 1) / G;
    a.m = slot == TENSOR_SLOT_U8 ? 255u : slot == TENSOR_SLOT_U16 ? (1u << depth) - 1u : 0u;
    a.fm = (float)a.m;
    a.truncate = quantise == CE_QUANT_TRUNCATE;
    a.path = tensor_pick_path(dtype, slot, data, sn, sc, sy, sx, count);
    return a;
}
// its grid's x: the blocks that cover an image's groups
inline size_t tensor_blocks(const tensor_args &a) { return ((size_t)a.gpr * a.h + kTensorBlock - 1) / kTensorBlock; }

// "tensor_<dtype>_<u8|u16|lin>[_m]": tensor_f32_u8, tensor_bf16_lin, tensor_u8_u16_m; _m for a launch that covers more than
// one image.  A value, not a pointer to keep: the profiler copies a name it has not seen and compares the others.
struct tensor_profile_name {
    char s[24];
    tensor_profile_name(int dtype, int slot, bool many)
    {
        std::snprintf(s, sizeof s, "tensor_%s_%s%s",
                      dtype == CE_DTYPE_U8 ? "u8" : dtype == CE_DTYPE_U16 ? "u16" : dtype == CE_DTYPE_F16 ? "f16" : dtype == CE_DTYPE_BF16 ? "bf16" : "f32",
                      slot == TENSOR_SLOT_U8 ? "u8" : slot == TENSOR_SLOT_U16 ? "u16" : "lin", many ? "_m" : "");
    }
};
