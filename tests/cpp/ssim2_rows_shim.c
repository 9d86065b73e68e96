/*
 * Test shim: the two passes of the CPU oracle's SSIMULACRA2 blur (oracle/ssimulacra2.c, blur mode 1: the recursive
 * Gaussian rg_line_iir) one at a time, which ceo_ssim2_blur_plane runs back to back without exporting the row pass.
 * Compiled at test time with the oracle Makefile's flags and -I oracle; the oracle itself stays as it is.
 *
 * shim_ssim2_row_streams forms the five streams of one XYB channel in the order of the device's row kernel
 * (ssim2.hip, k_ssim2_hblur_lds: {a, b, a*a, b*b, a*b}, a = the reference's plane, b = the distorted image's) with the
 * f32 products of ceo_ssimulacra2_detail, and runs the row pass over each.
 */
#include "ce_oracle.h"

int ceo_variant[CEO_V_COUNT]; /* the switches of this copy (libce_oracle.so keeps its own), all 0 */

#include "ssimulacra2.c"

#define SHIM_STREAMS 5

/* a, b: w * h floats, row-major; out: 5 * w * h floats, stream-major */
int shim_ssim2_row_streams(const float *a, const float *b, size_t w, size_t h, float *out)
{
    if (w == 0 || h == 0) return CEO_TOO_SMALL;
    const size_t n = w * h;
    rg_coeffs rg;
    rg_create(1.5, &rg);
    float *in = (float *)malloc(sizeof(float) * n);
    for (int s = 0; s < SHIM_STREAMS; s++) {
        for (size_t i = 0; i < n; i++) {
            switch (s) {
                case 0: in[i] = a[i]; break;
                case 1: in[i] = b[i]; break;
                case 2: in[i] = a[i] * a[i]; break;
                case 3: in[i] = b[i] * b[i]; break;
                default: in[i] = a[i] * b[i]; break;
            }
        }
        for (size_t y = 0; y < h; y++) rg_line_iir(&rg, in + y * w, out + (size_t)s * n + y * w, (ptrdiff_t)w, 1);
    }
    free(in);
    return CEO_OK;
}

/* the column pass of ceo_ssim2_blur_plane (blur mode 1) over a row-blurred plane of w * h floats */
int shim_ssim2_col_pass(const float *in, size_t w, size_t h, float *out)
{
    if (w == 0 || h == 0) return CEO_TOO_SMALL;
    rg_coeffs rg;
    rg_create(1.5, &rg);
    for (size_t x = 0; x < w; x++) rg_line_iir(&rg, in + x, out + x, (ptrdiff_t)h, (ptrdiff_t)w);
    return CEO_OK;
}
