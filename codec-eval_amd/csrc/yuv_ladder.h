// What a launch of Y'CbCr planes picks at run time and its kernel wants at compile time, in one place for yuv.hip,
// yuv_cicp.hip and the host harnesses (tests/cpp/yuv_kernel_host.cpp, yuv_cicp_kernel_host.cpp, hlg_kernel_host.cpp):
// (8-bit samples, subsampling, semiplanar) -> BPS, SUB and SEMI of yuv_kernel.h's yuv_block, and the profile name that says
// what a dispatch moved.  Host-compilable with plain g++ -std=c++17.
#pragma once

#include <cstdio>
#include <type_traits>

#include "ce_metrics.h"

// f(bps, sub, semi) is called once, with three std::integral_constant: bytes per sample (1: depth 8, 2 otherwise), the
// enum ce_yuv_subsampling (anything but 4:4:4, 4:2:2 and 4:2:0 is 4:0:0) and whether CbCr is interleaved, which 4:0:0, having no
// chroma, never is
template <class F>
inline void yuv_ladder(bool depth8, int subsampling, bool semiplanar, F &&f)
{
    auto layout = [&](auto bps, auto sub) {
        if constexpr (decltype(sub)::value != CE_YUV_400) {
            if (semiplanar) return f(bps, sub, std::true_type{});
        }
        return f(bps, sub, std::false_type{});
    };
    auto sub = [&](auto bps) {
        switch (subsampling) {
            case CE_YUV_444: return layout(bps, std::integral_constant<int, CE_YUV_444>{});
            case CE_YUV_422: return layout(bps, std::integral_constant<int, CE_YUV_422>{});
            case CE_YUV_420: return layout(bps, std::integral_constant<int, CE_YUV_420>{});
            default: return layout(bps, std::integral_constant<int, CE_YUV_400>{});
        }
    };
    if (depth8) sub(std::integral_constant<int, 1>{});
    else sub(std::integral_constant<int, 2>{});
}

// "yuv<subsampling>_<bits of an input sample><suffix>": yuv420_8, yuv444_16_deep, yuv422_8_lin_m, yuv400_16_hlg.  A value, not
// a pointer to keep: the profiler copies a name it has not seen and compares the others (ce_api.cpp: ce_prof_begin).
struct yuv_profile_name {
    char s[24];
    yuv_profile_name(int sub, int bps, const char *suffix)
    {
        std::snprintf(s, sizeof s, "yuv%s_%d%s", sub == CE_YUV_444 ? "444" : sub == CE_YUV_422 ? "422" : sub == CE_YUV_420 ? "420" : "400",
                      8 * bps, suffix);
    }
};
