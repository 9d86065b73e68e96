// ce_ciede2000_pixels' arithmetic (include/ce_metrics.h): ciede2000_pixel.h - the text ciede2000.hip
// compiles for the device - compiled for the host.  The Makefile builds this one file as plain C++ (no HIP, so the keywords of
// the pixel headers are defined away here, as the *_kernel_host.cpp test programs do) with -ffp-contract=off: every operation
// of the pixel is then the same separately rounded IEEE f64 operation on the host as on the device, and the integers agree.
// The checks of the arguments and the tables are ce_api.cpp's.
#define __device__
#define __forceinline__ inline

#include "ciede2000_pixel.h"

void ce_ciede2000_pixels_host(const uint16_t *ref_rgb, const float *ref_table, uint32_t ref_maxv, const uint16_t *test_rgb,
                              const float *test_table, uint32_t test_maxv, size_t n, uint32_t *out_q20)
{
    for (size_t i = 0; i < n; i++) {
        float er[3], et[3];
        for (int c = 0; c < 3; c++) {
            const uint32_t r = ref_rgb[i * 3 + c], t = test_rgb[i * 3 + c];
            er[c] = ref_table[r < ref_maxv ? r : ref_maxv], et[c] = test_table[t < test_maxv ? t : test_maxv];
        }
        out_q20[i] = cie_pixel_q20(er, et);
    }
}

// ce_ciede2000_pixel_terms' loop: the four values of a pixel as ciede2000_map_kernel.h's cie_map_pixel
// forms them - q and rint(|term| 2^20) of the lightness, chroma and hue terms - without its skip of equal triples, which
// changes no value
void ce_ciede2000_pixel_terms_host(const uint16_t *ref_rgb, const float *ref_table, uint32_t ref_maxv, const uint16_t *test_rgb,
                                   const float *test_table, uint32_t test_maxv, size_t n, uint32_t *out)
{
    for (size_t i = 0; i < n; i++) {
        float er[3], et[3];
        for (int c = 0; c < 3; c++) {
            const uint32_t r = ref_rgb[i * 3 + c], t = test_rgb[i * 3 + c];
            er[c] = ref_table[r < ref_maxv ? r : ref_maxv], et[c] = test_table[t < test_maxv ? t : test_maxv];
        }
        const cie_terms e = cie_de2000_terms(cie_lab_of(er[0], er[1], er[2]), cie_lab_of(et[0], et[1], et[2]));
        const double term[3] = {e.tl, e.tc, e.th};
        out[i * 4] = cie_terms_q20(e);
        for (int k = 0; k < 3; k++) out[i * 4 + 1 + k] = (uint32_t)(unsigned long long)__builtin_rint(__builtin_fabs(term[k]) * 1048576.0);
    }
}
