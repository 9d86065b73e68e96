/*
 * Test shim: the CPU oracle's DSSIM SSIM maps (oracle/dssim.c), which the oracle reduces to per-scale scores and a
 * score without exporting the maps.  Compiled at test time with the oracle Makefile's flags and -I oracle; the oracle
 * itself stays as it is.  shim_dssim_maps repeats ceo_dssim_detail and the body of compare up to each scale's map[]
 * (the same f32 operations in the same order) and keeps every scale's map, its score and the weighted result;
 * shim_dssim_levels repeats the size rule of create_image without building the planes.
 */
#include "psnr_xyb.c" /* ceo_srgb_u8_to_linear and this copy's ceo_variant */
#include "dssim.c"

/* create_image's loop control: the sizes of its scales */
int shim_dssim_levels(size_t w, size_t h, size_t *level_w, size_t *level_h)
{
    int n = 0;
    if (w == 0 || h == 0) return 0;
    for (int scale = 0; scale < DSSIM_MAX_SCALES; scale++) {
        level_w[n] = w;
        level_h[n] = h;
        n++;
        if (scale + 1 >= DSSIM_MAX_SCALES) break;
        if (w < 8 || h < 8) break;
        w /= 2;
        h /= 2;
    }
    return n;
}

/* maps: every scale's w_l * h_l floats, scale after scale, row-major; scores: DSSIM_MAX_SCALES doubles */
int shim_dssim_maps(const uint8_t *ref, const uint8_t *test, size_t width, size_t height, int *n_scales, float *maps,
                    double *scores, double *out)
{
    const size_t npix = width * height;
    if (npix == 0) return CEO_BACKEND;
    float *p1 = (float *)malloc(sizeof(float) * 3 * npix), *p2 = (float *)malloc(sizeof(float) * 3 * npix);
    for (size_t i = 0; i < npix; i++)
        for (int c = 0; c < 3; c++) {
            p1[(size_t)c * npix + i] = ceo_srgb_u8_to_linear(ref[3 * i + c]);
            p2[(size_t)c * npix + i] = ceo_srgb_u8_to_linear(test[3 * i + c]);
        }
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
