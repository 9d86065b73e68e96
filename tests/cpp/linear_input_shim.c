/*
 * Test shim: the CPU oracle's three perceptual metrics on linear input (packed float RGB, linear light with sRGB primaries,
 * any range), for the linear-input tests.  Compiled at test time with the oracle Makefile's flags and -I oracle; the oracle
 * itself stays as it is.
 *
 * Only the first lines of the oracle's three drivers are replaced - samples -> linear planes is a copy here, with no table.
 * Everything after that is the oracle's own code: ceo_ssim2_downscale .. ceo_ssimulacra2_score (the body of
 * ceo_ssimulacra2_detail), ceo_dssim_rgbaf, and diffmap_level / subsample2x with the max / p-norm tail of ceo_butteraugli.
 */
#include "ce_oracle.h"

int ceo_variant[CEO_V_COUNT]; /* the switches of this copy (libce_oracle.so keeps its own), all 0 */

#include "psnr_xyb.c" /* ceo_srgb_u8_to_linear, which dssim.c's u8 driver calls */
#include "ssimulacra2.c"
#include "dssim.c"
#include "butteraugli.c"

/* packed samples -> three linear planes */
static void lin_planar(const float *rgb, size_t npix, float *planes)
{
    for (size_t i = 0; i < npix; i++)
        for (int c = 0; c < 3; c++) planes[(size_t)c * npix + i] = rgb[3 * i + c];
}

/* ceo_ssimulacra2_detail after its first two lines */
int shim_linear_ssimulacra2(const float *ref, const float *test, size_t width,
                          size_t height, int blur_mode, double *score)
{
    if (width < 8 || height < 8) return CEO_TOO_SMALL;
    size_t w = width, h = height, n = w * h;
    double avg[NUM_SCALES * 18];
    float *lin1 = (float *)malloc(sizeof(float) * 3 * n), *lin2 = (float *)malloc(sizeof(float) * 3 * n);
    float *tmp = (float *)malloc(sizeof(float) * 3 * n);
    float *x1 = (float *)malloc(sizeof(float) * 3 * n), *x2 = (float *)malloc(sizeof(float) * 3 * n);
    float *mul = (float *)malloc(sizeof(float) * 3 * n);
    float *s11 = (float *)malloc(sizeof(float) * 3 * n), *s22 = (float *)malloc(sizeof(float) * 3 * n);
    float *s12 = (float *)malloc(sizeof(float) * 3 * n);
    float *mu1 = (float *)malloc(sizeof(float) * 3 * n), *mu2 = (float *)malloc(sizeof(float) * 3 * n);
    lin_planar(ref, n, lin1);
    lin_planar(test, n, lin2);
    int ns = 0;
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
            ceo_ssim2_blur_plane(mul + o, w, h, blur_mode, s11 + o);
            for (size_t i = 0; i < n; i++) mul[o + i] = x2[o + i] * x2[o + i];
            ceo_ssim2_blur_plane(mul + o, w, h, blur_mode, s22 + o);
            for (size_t i = 0; i < n; i++) mul[o + i] = x1[o + i] * x2[o + i];
            ceo_ssim2_blur_plane(mul + o, w, h, blur_mode, s12 + o);
            ceo_ssim2_blur_plane(x1 + o, w, h, blur_mode, mu1 + o);
            ceo_ssim2_blur_plane(x2 + o, w, h, blur_mode, mu2 + o);
        }
        double *a = avg + (size_t)scale * 18;
        ssim_map(w, h, mu1, mu2, s11, s22, s12, a);
        edge_diff_map(w, h, x1, mu1, x2, mu2, a);
        ns++;
    }
    free(lin1); free(lin2); free(tmp); free(x1); free(x2); free(mul);
    free(s11); free(s22); free(s12); free(mu1); free(mu2);
    *score = ceo_ssimulacra2_score(avg, ns);
    return CEO_OK;
}

/* both sides into RGBA<f32>, then the oracle's float-in DSSIM */
int shim_linear_dssim(const float *ref, const float *test, size_t width, size_t height,
                    double *out)
{
    const size_t n = width * height;
    float *p = (float *)malloc(sizeof(float) * 3 * n);
    float *ra = (float *)malloc(sizeof(float) * 4 * n), *ta = (float *)malloc(sizeof(float) * 4 * n);
    lin_planar(ref, n, p);
    for (size_t i = 0; i < n; i++) {
        for (int c = 0; c < 3; c++) ra[4 * i + c] = p[(size_t)c * n + i];
        ra[4 * i + 3] = 1.0f;
    }
    lin_planar(test, n, p);
    for (size_t i = 0; i < n; i++) {
        for (int c = 0; c < 3; c++) ta[4 * i + c] = p[(size_t)c * n + i];
        ta[4 * i + 3] = 1.0f;
    }
    int rc = ceo_dssim_rgbaf(ra, width, height, ta, width, height, out);
    free(p); free(ra); free(ta);
    return rc;
}

/* ceo_butteraugli after its table and sample loop */
int shim_linear_butteraugli(const float *ref, const float *test, size_t width,
                          size_t height, float intensity_target, double *score, double *pnorm3)
{
    if (width < 8 || height < 8) return CEO_TOO_SMALL;
    const size_t w = width, h = height, n = w * h;
    img rgb0[3], rgb1[3];
    for (int c = 0; c < 3; c++) {
        rgb0[c] = img_new(w, h);
        rgb1[c] = img_new(w, h);
    }
    float *p = (float *)malloc(sizeof(float) * 3 * n);
    lin_planar(ref, n, p);
    for (int c = 0; c < 3; c++) memcpy(rgb0[c].p, p + (size_t)c * n, sizeof(float) * n);
    lin_planar(test, n, p);
    for (int c = 0; c < 3; c++) memcpy(rgb1[c].p, p + (size_t)c * n, sizeof(float) * n);
    free(p);
    img diffmap = img_new(w, h);
    diffmap_level(rgb0, rgb1, intensity_target, &diffmap);
    img s0[3], s1[3];
    subsample2x(rgb0, s0);
    subsample2x(rgb1, s1);
    if (s0[0].w >= 8 && s0[0].h >= 8) {
        img sub = img_new(s0[0].w, s0[0].h);
        diffmap_level(s0, s1, intensity_target, &sub);
        const float kHeuristicMixingValue = 0.3f, wgt = 0.5f;
        for (size_t y = 0; y < h; y++)
            for (size_t x = 0; x < w; x++) {
                float *d = &diffmap.p[y * w + x];
                *d *= 1.0f - kHeuristicMixingValue * wgt;
                *d += wgt * sub.p[(y / 2) * sub.w + x / 2];
            }
        img_free(&sub);
    }
    float mx = 0.0f;
    double sum1[3] = {0, 0, 0};
    for (size_t i = 0; i < n; i++) {
        const float d = diffmap.p[i];
        if (d > mx) mx = d;
        const double dd = d, d3 = dd * dd * dd, d6 = d3 * d3;
        sum1[0] += d3;
        sum1[1] += d6;
        sum1[2] += d6 * d6;
    }
    *score = (double)mx;
    if (pnorm3) {
        const double one_per_pixels = 1.0 / (double)n;
        double v = pow(one_per_pixels * sum1[0], 1.0 / 3.0) + pow(one_per_pixels * sum1[1], 1.0 / 6.0) +
                   pow(one_per_pixels * sum1[2], 1.0 / 12.0);
        *pnorm3 = v / 3.0;
    }
    img_free(&diffmap);
    for (int c = 0; c < 3; c++) {
        img_free(&rgb0[c]); img_free(&rgb1[c]); img_free(&s0[c]); img_free(&s1[c]);
    }
    return CEO_OK;
}
