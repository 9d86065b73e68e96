// Which pixel a ce_linear_pixel means, in one place for the launchers of a colour description: cicp.hip's ce_launch_tagged and
// ce_launch_tagged_over, yuv_cicp.hip's ce_launch_yuv_tagged.
#pragma once

#include "ce_internal.h"

#include "cicp_pixel.h"
#include "hlg_pixel.h"

// f(pixel, stem, m) is called once, with cicp_pixel.h's cicp_px<MATRIX> or hlg_pixel.h's hlg_px<MATRIX> filled from the plan
// and the frame's d_src (nullptr for planes), n_pixels and d_dst, and with what the profile name of a packed launch begins
// ("cicp", "hlg") and ends with ("_m" with the primaries matrix, "" without)
template <class F>
inline void tagged_pick(const ce_linear_pixel &px, const void *d_src, size_t n_pixels, float *d_dst, F &&f)
{
    hlg_args a{};  // the CICP pixel takes its `c` alone
    a.c.src = d_src, a.c.n_pixels = n_pixels;
    ce_fill_pixel_args(a, d_dst, px);
    if (px.hlg) {
        if (px.has_matrix) f(hlg_px<true>{a}, "hlg", "_m");
        else f(hlg_px<false>{a}, "hlg", "");
    } else {
        if (px.has_matrix) f(cicp_px<true>{a.c}, "cicp", "_m");
        else f(cicp_px<false>{a.c}, "cicp", "");
    }
}
