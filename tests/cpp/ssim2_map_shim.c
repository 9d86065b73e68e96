/*
 * Test shim: the CPU oracle's SSIMULACRA2 per-pixel error maps (oracle/ssimulacra2.c), which the oracle pools into means
 * and 4-norms without exporting the maps.  Compiled at test time with the oracle Makefile's flags and -I oracle; the
 * oracle itself stays as it is.
 *
 * shim_ssim2_maps repeats ceo_ssimulacra2_detail (blur mode 1, the recursive Gaussian the device runs) and keeps every
 * scale's nine maps instead of pooling them:
 *   d            the SSIM error of ssim_map in the form of its CEO_V_SSIM2_F32_POOL switch, which is the device's: the f32
 *                1 - (num_m * num_s) / denom_s, clamped at 0 (f32)
 *   artifact,    edge_diff_map's terms with the oracle's default switches: (1 + |img2 - mu2|) / (1 + |img1 - mu1|) - 1
 *   detail_lost  in f64, then max(d1, 0) and max(-d1, 0) (f64)
 * shim_ssim2_scales repeats the scale loop's size rule without building the planes.
 */
#include "ce_oracle.h"

int ceo_variant[CEO_V_COUNT]; /* the switches of this copy (libce_oracle.so keeps its own), all 0 */

#include "ssimulacra2.c"

/* the loop control of ceo_ssimulacra2_detail: the sizes of its scales */
int shim_ssim2_scales(size_t w, size_t h, size_t *scale_w, size_t *scale_h)
{
    int n = 0;
    for (int scale = 0; scale < NUM_SCALES; scale++) {
        if (w < 8 || h < 8) break;
        if (scale > 0) {
            w = (w + 1) / 2;
            h = (h + 1) / 2;
        }
        scale_w[n] = w;
        scale_h[n] = h;
        n++;
    }
    return n;
}

/* Scale after scale (sizes of shim_ssim2_scales): d_maps gets [3][h_s][w_s] floats, edge_maps [3][2][h_s][w_s] doubles
 * (artifact, detail_lost). */
int shim_ssim2_maps(const uint8_t *ref, const uint8_t *test, size_t width, size_t height, int *n_scales_out, float *d_maps,
                    double *edge_maps)
{
    if (width < 8 || height < 8) return CEO_TOO_SMALL;
    size_t w = width, h = height, n = w * h;
    float *lin1 = (float *)malloc(sizeof(float) * 3 * n), *lin2 = (float *)malloc(sizeof(float) * 3 * n);
    float *tmp = (float *)malloc(sizeof(float) * 3 * n);
    float *x1 = (float *)malloc(sizeof(float) * 3 * n), *x2 = (float *)malloc(sizeof(float) * 3 * n);
    float *mul = (float *)malloc(sizeof(float) * 3 * n);
    float *s11 = (float *)malloc(sizeof(float) * 3 * n), *s22 = (float *)malloc(sizeof(float) * 3 * n);
    float *s12 = (float *)malloc(sizeof(float) * 3 * n);
    float *mu1 = (float *)malloc(sizeof(float) * 3 * n), *mu2 = (float *)malloc(sizeof(float) * 3 * n);
    ceo_ssim2_linear_planar(ref, n, lin1);
    ceo_ssim2_linear_planar(test, n, lin2);
    const float C2 = 0.0009f;
    int ns = 0;
    size_t doff = 0, eoff = 0;
    for (int scale = 0; scale < NUM_SCALES; scale++) {
        if (w < 8 || h < 8) break;
        if (scale > 0) {
            ceo_ssim2_downscale(lin1, w, h, tmp);
            size_t ow = (w + 1) / 2, oh = (h + 1) / 2;
            memcpy(lin1, tmp, sizeof(float) * 3 * ow * oh);
            ceo_ssim2_downscale(lin2, w, h, tmp);
            memcpy(lin2, tmp, sizeof(float) * 3 * ow * oh);
            w = ow;
            h = oh;
            n = w * h;
        }
        ceo_ssim2_xyb_positive(lin1, n, x1);
        ceo_ssim2_xyb_positive(lin2, n, x2);
        for (int c = 0; c < 3; c++) {
            const size_t o = (size_t)c * n;
            for (size_t i = 0; i < n; i++) mul[o + i] = x1[o + i] * x1[o + i];
            ceo_ssim2_blur_plane(mul + o, w, h, 1, s11 + o);
            for (size_t i = 0; i < n; i++) mul[o + i] = x2[o + i] * x2[o + i];
            ceo_ssim2_blur_plane(mul + o, w, h, 1, s22 + o);
            for (size_t i = 0; i < n; i++) mul[o + i] = x1[o + i] * x2[o + i];
            ceo_ssim2_blur_plane(mul + o, w, h, 1, s12 + o);
            ceo_ssim2_blur_plane(x1 + o, w, h, 1, mu1 + o);
            ceo_ssim2_blur_plane(x2 + o, w, h, 1, mu2 + o);
        }
        for (int c = 0; c < 3; c++) {
            const size_t o = (size_t)c * n;
            float *dm = d_maps + doff + o;
            double *am = edge_maps + eoff + 2 * o, *lm = am + n;
            for (size_t i = 0; i < n; i++) {
                /* ssim_map */
                float m1 = mu1[o + i], m2 = mu2[o + i];
                float mu11 = m1 * m1, mu22 = m2 * m2, mu12 = m1 * m2;
                float mu_diff = m1 - m2;
                float num_m = fmaf(mu_diff, -mu_diff, 1.0f);
                float num_s = fmaf(2.0f, s12[o + i] - mu12, C2);
                float denom_s = (s11[o + i] - mu11) + (s22[o + i] - mu22) + C2;
                float d = 1.0f - (num_m * num_s) / denom_s;
                dm[i] = d > 0.0f ? d : 0.0f;
                /* edge_diff_map */
                double d1 = (1.0 + (double)fabsf(x2[o + i] - m2)) / (1.0 + (double)fabsf(x1[o + i] - m1)) - 1.0;
                am[i] = d1 > 0.0 ? d1 : 0.0;
                lm[i] = -d1 > 0.0 ? -d1 : 0.0;
            }
        }
        doff += 3 * n;
        eoff += 6 * n;
        ns++;
    }
    free(lin1); free(lin2); free(tmp); free(x1); free(x2); free(mul);
    free(s11); free(s22); free(s12); free(mu1); free(mu2);
    *n_scales_out = ns;
    return CEO_OK;
}
