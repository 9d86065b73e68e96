/*
 * Test shim: the CPU oracle's Butteraugli diffmap (oracle/butteraugli.c), which the oracle reduces to a score and a
 * p-norm without exporting the map.  Compiled at test time with the oracle Makefile's flags and -I oracle; the oracle
 * itself stays as it is.  shim_butteraugli_diffmap repeats the steps of ceo_butteraugli up to the finished map: the sRGB
 * table, diffmap_level at full resolution, subsample2x and, when the half level is at least 8 x 8, the supersampled mix.
 */
#include "ce_oracle.h"

int ceo_variant[CEO_V_COUNT]; /* the switches of this copy (libce_oracle.so keeps its own) */

#include "butteraugli.c"

void shim_set_variant(int key, int value)
{
    if (key >= 0 && key < CEO_V_COUNT) ceo_variant[key] = value;
}

/* out: width * height floats, row-major */
int shim_butteraugli_diffmap(const uint8_t *ref, const uint8_t *test, size_t width, size_t height, float intensity_target, float *out)
{
    if (width < 8 || height < 8) return CEO_TOO_SMALL;
    const size_t w = width, h = height, n = w * h;
    img rgb0[3], rgb1[3];
    for (int c = 0; c < 3; c++) {
        rgb0[c] = img_new(w, h);
        rgb1[c] = img_new(w, h);
    }
    float lut[256];
    for (int i = 0; i < 256; i++) {
        double v = (double)i / 255.0;
        lut[i] = (float)(v <= 0.04045 ? v / 12.92 : pow((v + 0.055) / 1.055, 2.4));
    }
    for (size_t i = 0; i < n; i++)
        for (int c = 0; c < 3; c++) {
            rgb0[c].p[i] = lut[ref[3 * i + c]];
            rgb1[c].p[i] = lut[test[3 * i + c]];
        }
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
    memcpy(out, diffmap.p, n * sizeof(float));
    img_free(&diffmap);
    for (int c = 0; c < 3; c++) {
        img_free(&rgb0[c]); img_free(&rgb1[c]); img_free(&s0[c]); img_free(&s1[c]);
    }
    return CEO_OK;
}
