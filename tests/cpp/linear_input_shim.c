/*
 * Test shim: the CPU oracle's three perceptual metrics on linear input (packed float RGB, linear light with sRGB primaries,
 * any range), for the linear-input and wide-content tests.  Compiled at test time with the oracle Makefile's flags and
 * -I oracle; the oracle itself stays as it is.
 *
 * Only the first lines of the oracle's three drivers are replaced - samples -> linear planes is a copy here, with no table.
 * Everything after that is the oracle's own code: ceo_ssim2_downscale .. ceo_ssimulacra2_score (the body of
 * ceo_ssimulacra2_detail), ceo_dssim_rgbaf, and diffmap_level / subsample2x with the max / p-norm tail of ceo_butteraugli.
 * The *_maps entry points keep what the drivers pool away, in the way of ba_diffmap_shim.c, dssim_map_shim.c and
 * ssim2_map_shim.c.
 *
 * This copy also records the operands of the oracle's hand-expandable divisions: CEO_DIV (ce_oracle.h) is defined here as
 * a call that computes the same a / b and keeps per-site extremes (shim_probe_read / shim_probe_reset).
 */
#include <math.h>
#include <stdint.h>
#include <string.h>

static float shim_div(int site, float a, float b);
#define CEO_DIV(site, a, b) shim_div((site), (a), (b))

#include "ce_oracle.h"

int ceo_variant[CEO_V_COUNT]; /* the switches of this copy (libce_oracle.so keeps its own), all 0 */

void shim_set_variant(int key, int value)
{
    if (key >= 0 && key < CEO_V_COUNT) ceo_variant[key] = value;
}

/* per site: [0..5] min / max of |numerator|, |denominator|, |quotient| over the finite non-zero values; [6] the signs seen
 * (bit 0 numerator > 0, 1 numerator < 0, 2 denominator > 0, 3 denominator < 0); [7] zero numerators, [8] zero
 * denominators, [9] subnormal numerators, [10] subnormal denominators, [11] subnormal quotients, [12] non-finite
 * quotients, [13] divisions */
#define PROBE_FIELDS 14
static double probe[CEO_DIV_SITES][PROBE_FIELDS];
static float probe_last_den[CEO_DIV_SITES];

void shim_probe_reset(void)
{
    for (int s = 0; s < CEO_DIV_SITES; s++) {
        for (int k = 0; k < PROBE_FIELDS; k++) probe[s][k] = 0.0;
        probe[s][0] = probe[s][2] = probe[s][4] = INFINITY;
    }
}

void shim_probe_read(double *out /* [CEO_DIV_SITES][PROBE_FIELDS] */)
{
    memcpy(out, probe, sizeof(probe));
}

static void probe_extreme(double *lohi, float v)
{
    const double m = fabs((double)v);
    if (m == 0.0 || !isfinite(m)) return;
    if (m < lohi[0]) lohi[0] = m;
    if (m > lohi[1]) lohi[1] = m;
}

static float shim_div(int site, float a, float b)
{
    const float q = a / b;
    double *p = probe[site];
    if (p[13] == 0.0 && p[0] == 0.0) shim_probe_reset(); /* first use */
    probe_extreme(p + 0, a);
    probe_extreme(p + 2, b);
    probe_extreme(p + 4, q);
    p[6] = (double)((int)p[6] | (a > 0) | (a < 0) << 1 | (b > 0) << 2 | (b < 0) << 3);
    p[7] += a == 0.0f;
    p[8] += b == 0.0f;
    p[9] += a != 0.0f && fabsf(a) < 1.17549435e-38f;
    p[10] += b != 0.0f && fabsf(b) < 1.17549435e-38f;
    p[11] += q != 0.0f && fabsf(q) < 1.17549435e-38f;
    p[12] += !isfinite(q);
    p[13] += 1.0;
    probe_last_den[site] = b;
    return q;
}

#include "psnr_xyb.c" /* ceo_srgb_u8_to_linear, which dssim.c's u8 driver calls */
#include "ssimulacra2.c"
#include "dssim.c"
#include "butteraugli.c"

/* the denominator of cbrt_poly's Halley step `step` (1 or 2) at x - 2 y^3 + x with y the seed polynomial, or the first
 * step's result - through the oracle's own cbrt_poly; leaves the probe's extremes as they were */
float shim_probe_cbrt_den(float x, int step)
{
    double keep[CEO_DIV_SITES][PROBE_FIELDS];
    memcpy(keep, probe, sizeof(probe));
    (void)cbrt_poly(x);
    memcpy(probe, keep, sizeof(probe));
    return probe_last_den[step == 2 ? CEO_DIV_CBRT_2 : CEO_DIV_CBRT_1];
}

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
static int linear_butteraugli(const float *ref, const float *test, size_t width, size_t height, float intensity_target,
                              double *score, double *pnorm3, float *map_out)
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
    if (map_out) memcpy(map_out, diffmap.p, n * sizeof(float));
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

int shim_linear_butteraugli(const float *ref, const float *test, size_t width,
                          size_t height, float intensity_target, double *score, double *pnorm3)
{
    return linear_butteraugli(ref, test, width, height, intensity_target, score, pnorm3, NULL);
}

/* the same with the finished diffmap: out is width * height floats, row-major */
int shim_linear_butteraugli_map(const float *ref, const float *test, size_t width, size_t height, float intensity_target,
                                double *score, double *pnorm3, float *out)
{
    return linear_butteraugli(ref, test, width, height, intensity_target, score, pnorm3, out);
}

/* dssim_map_shim.c's shim_dssim_maps from float planes on: every scale's map (w_l * h_l floats, scale after scale), its score
 * and the weighted result.  The per-pixel expression and the pooling are compare()'s, operation for operation. */
int shim_linear_dssim_maps(const float *ref, const float *test, size_t width, size_t height, int *n_scales, float *maps,
                           double *scores, double *out)
{
    const size_t npix = width * height;
    if (npix == 0) return CEO_BACKEND;
    float *p1 = (float *)malloc(sizeof(float) * 3 * npix), *p2 = (float *)malloc(sizeof(float) * 3 * npix);
    lin_planar(ref, npix, p1);
    lin_planar(test, npix, p2);
    dssim_image o, m;
    create_image(p1, width, height, &o);
    create_image(p2, width, height, &m);
    free(p1);
    free(p2);
    const float c1 = 0.01f * 0.01f, c2 = 0.03f * 0.03f;
    int ns = o.n < m.n ? o.n : m.n;
    double ssim_sum = 0.0, weight_sum = 0.0;
    size_t map_off = 0;
    for (int k = 0; k < ns; k++) {
        const dssim_scale *a = &o.s[k], *b = &m.s[k];
        const size_t w = a->w, h = a->h, n = w * h;
        float *i12[3];
        float *tmp = (float *)malloc(sizeof(float) * n);
        float *mul = (float *)malloc(sizeof(float) * n);
        for (int c = 0; c < 3; c++) {
            i12[c] = (float *)malloc(sizeof(float) * n);
            for (size_t i = 0; i < n; i++) mul[i] = a->img[c][i] * b->img[c][i];
            blur2(mul, i12[c], tmp, w, h);
        }
        float *map = maps + map_off;
        const float third = 1.0f / 3.0f;
        for (size_t i = 0; i < n; i++) {
            float mu1mu1[3], mu1mu2[3], mu2mu2[3], s1[3], s2[3], s12[3];
            for (int c = 0; c < 3; c++) {
                float u1 = a->mu[c][i], u2 = b->mu[c][i];
                mu1mu1[c] = u1 * u1;
                mu1mu2[c] = u1 * u2;
                mu2mu2[c] = u2 * u2;
                s1[c] = a->sq[c][i] - mu1mu1[c];
                s2[c] = b->sq[c][i] - mu2mu2[c];
                s12[c] = i12[c][i] - mu1mu2[c];
            }
#define AVG3(v) (((v)[0] + (v)[1] + (v)[2]) * third)
            float mu1_sq = AVG3(mu1mu1), mu2_sq = AVG3(mu2mu2), mu1_mu2 = AVG3(mu1mu2);
            float sigma1_sq = AVG3(s1), sigma2_sq = AVG3(s2), sigma12 = AVG3(s12);
#undef AVG3
            map[i] = (2.0f * mu1_mu2 + c1) * (2.0f * sigma12 + c2) /
                     ((mu1_sq + mu2_sq + c1) * (sigma1_sq + sigma2_sq + c2));
        }
        double sum = 0.0;
        for (size_t i = 0; i < n; i++) sum += (double)map[i];
        double len = (double)n;
        double avg = sum / len;
        if (!(avg > 0.0)) avg = 0.0;
        avg = pow(avg, pow(0.5, (double)k));
        double dev = 0.0;
        for (size_t i = 0; i < n; i++) dev += fabs(avg - (double)map[i]);
        double score = 1.0 - dev / len;
        scores[k] = score;
        ssim_sum += score * DEFAULT_WEIGHTS[k];
        weight_sum += DEFAULT_WEIGHTS[k];
        for (int c = 0; c < 3; c++) free(i12[c]);
        free(tmp);
        free(mul);
        map_off += n;
    }
    free_image(&o);
    free_image(&m);
    *n_scales = ns;
    double ssim = ssim_sum / weight_sum;
    if (!(ssim > DBL_EPSILON)) ssim = DBL_EPSILON;
    *out = 1.0 / ssim - 1.0;
    return CEO_OK;
}

/* ssim2_map_shim.c's shim_ssim2_maps from float planes on (blur mode 1).  Scale after scale: d_maps gets [3][h_s][w_s]
 * floats (ssim_map's error in the f32 form of CEO_V_SSIM2_F32_POOL, the device's), edge_maps [3][2][h_s][w_s] doubles
 * (edge_diff_map's artifact and detail_lost in f64) and, when edge_f32 is given, the same two expressions evaluated in
 * f32 - the spread between the two is the reference's own, which bounds what an f32 device can be asked to match. */
int shim_linear_ssim2_maps(const float *ref, const float *test, size_t width, size_t height, int *n_scales_out, float *d_maps,
                           double *edge_maps, float *edge_f32)
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
    lin_planar(ref, n, lin1);
    lin_planar(test, n, lin2);
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
            float *af = edge_f32 ? edge_f32 + eoff + 2 * o : NULL, *lf = af ? af + n : NULL;
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
                if (af) {
                    float f1 = (1.0f + fabsf(x2[o + i] - m2)) / (1.0f + fabsf(x1[o + i] - m1)) - 1.0f;
                    af[i] = f1 > 0.0f ? f1 : 0.0f;
                    lf[i] = -f1 > 0.0f ? -f1 : 0.0f;
                }
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
