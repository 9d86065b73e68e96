// One pixel of the ICC ingest (include/ce_metrics.h: the matrix/TRC definition, steps 1 to 3): cicp_pixel.h's arguments with
// a table per channel - `c.table` is the red one - its separately rounded f32 matrix and its clamp.  icc_px is the pixel the
// frames take (cicp_kernel.h: k_tagged for linear slots; icc_kernel.h: k_icc_encode for u8 and u16 slots).  Host-compilable
// like the headers that include it, and compiled with -ffp-contract=off.
#pragma once

#include "cicp_pixel.h"

namespace {

struct icc_args {
    cicp_args c;            // table: the red channel's, maxv + 1 entries
    const float *table_g;   // maxv + 1 entries each
    const float *table_b;
};

// MATRIX: a profile whose colorants are not the canonical sRGB profile's
template <bool MATRIX>
struct icc_px {
    icc_args a;
    __device__ __forceinline__ const cicp_args &frame() const { return a.c; }
    __device__ __forceinline__ void operator()(uint32_t r, uint32_t g, uint32_t b, float (&o)[3]) const
    {
        const uint32_t m = a.c.maxv;
        const float tr = a.c.table[r < m ? r : m], tg = a.table_g[g < m ? g : m], tb = a.table_b[b < m ? b : m];
        cicp_matrix_clamp<MATRIX>(a.c, tr, tg, tb, o);
    }
};

}  // namespace
