// What a launch of packed RGB(A) code values picks at run time and its kernel wants at compile time, in one place for
// cicp.hip, icc.hip, icc_lut.hip and gainmap.hip, beside yuv_ladder.h: the format -> FMT of cicp_kernel.h's frames, and the
// profile name that says what a dispatch moved.  Host-compilable with plain g++ -std=c++17.
#pragma once

#include <cstdio>
#include <type_traits>

#include "ce_metrics.h"

// f(fmt) is called once, with the std::integral_constant of CE_PIXEL_RGB8, RGBA8, RGB16 or RGBA16; false, and no call, for any
// other format.  An `_over` launcher, which has refused everything but RGBA8 / RGBA16, launches under
// `if constexpr (packed_has_alpha(FMT))`: the ladder instantiates f for all four.
template <class F>
inline bool packed_ladder(int format, F &&f)
{
    switch (format) {
        case CE_PIXEL_RGB8: f(std::integral_constant<int, CE_PIXEL_RGB8>{}); return true;
        case CE_PIXEL_RGBA8: f(std::integral_constant<int, CE_PIXEL_RGBA8>{}); return true;
        case CE_PIXEL_RGB16: f(std::integral_constant<int, CE_PIXEL_RGB16>{}); return true;
        case CE_PIXEL_RGBA16: f(std::integral_constant<int, CE_PIXEL_RGBA16>{}); return true;
        default: return false;
    }
}

constexpr bool packed_has_alpha(int format) { return format == CE_PIXEL_RGBA8 || format == CE_PIXEL_RGBA16; }

// "<stem><slot>_<format><suffix>": cicp_rgb8_m, hlg_over_rgba16, icc_u16_rgb8_m, icc_lut_tet_lin_rgba16, gainmap_rgb16_3_m.
// `slot` is "", "_over" or an ICC slot kind ("_lin", "_u8", "_u16").  A value, not a pointer to keep: the profiler copies a
// name it has not seen and compares the others (ce_api.cpp: ce_prof_begin).
struct packed_profile_name {
    char s[32];
    packed_profile_name(const char *stem, const char *slot, int format, const char *suffix)
    {
        std::snprintf(s, sizeof s, "%s%s_%s%s", stem, slot,
                      format == CE_PIXEL_RGB8 ? "rgb8" : format == CE_PIXEL_RGBA8 ? "rgba8" : format == CE_PIXEL_RGB16 ? "rgb16" : "rgba16", suffix);
    }
};
