// Host-built constant tables for the device kernels.  Built once per context with the host
// libm, because the reference computes the same quantities with the host libm
// (Rust f32::powf -> powf, f64::powf -> pow).
#include <cmath>
#include <cstring>

#include "ce_internal.h"

// sRGB u8 -> linear, evaluated in f64 per code point and rounded once to f32: the front end
// of SSIMULACRA2.
void ce_build_srgb_lut_f64(float lut[256])
{
    for (int i = 0; i < 256; i++) {
        const double v = (double)i / 255.0;
        lut[i] = (float)(v <= 0.04045 ? v / 12.92 : std::pow((v + 0.055) / 1.055, 2.4));
    }
}

// sRGB u8 -> linear exactly as /root/reference/src/metrics/dssim.rs:78-85 and
// src/metrics/xyb.rs:60-66,80-82 write it: f32 arithmetic, f32 powf(2.4).
void ce_build_srgb_lut_powf(float lut[256])
{
    for (int i = 0; i < 256; i++) {
        const float s = (float)i / 255.0f;
        lut[i] = s <= 0.04045f ? s / 12.92f : powf((s + 0.055f) / 1.055f, 2.4f);
    }
}

// The same two rules with 255 replaced by maxv = 2^depth - 1 (deep batches): sample v means the sRGB
// value v / maxv.  With maxv = 255 these are the two tables above, entry for entry; with maxv = 65535 entry 257 * i is entry
// i of them (257 i / 65535 and i / 255 are the same real number and the division is correctly rounded).
void ce_build_srgb_table_f64(float *lut, uint32_t maxv)
{
    for (uint32_t i = 0; i <= maxv; i++) {
        const double v = (double)i / (double)maxv;
        lut[i] = (float)(v <= 0.04045 ? v / 12.92 : std::pow((v + 0.055) / 1.055, 2.4));
    }
}

void ce_build_srgb_table_powf(float *lut, uint32_t maxv)
{
    for (uint32_t i = 0; i <= maxv; i++) {
        const float s = (float)i / (float)maxv;
        lut[i] = s <= 0.04045f ? s / 12.92f : powf((s + 0.055f) / 1.055f, 2.4f);
    }
}

// Coefficients of the sigma = 1.5 recursive Gaussian (Charalampidis 2016 truncated-cosine
// form as derived in libjxl's CreateRecursiveGaussian):
// three second-order sections k = 1,3,5 with   out_k[n] = n2_k (in[n-N-1] + in[n+N-1])
//                                                          - d1_k out_k[n-1] - out_k[n-2].
// mul_in = n2, mul_prev = -d1, both rounded to f32.
void ce_ssim2_recursive_gaussian(float mul_in[3], float mul_prev[3])
{
    const double sigma = 1.5;
    const double radius = std::round(3.2795 * sigma + 0.2546);
    const double pi_div_2r = M_PI / (2.0 * radius);
    const double omega[3] = {pi_div_2r, 3.0 * pi_div_2r, 5.0 * pi_div_2r};
    const double p1 = +1.0 / std::tan(0.5 * omega[0]);
    const double p3 = -1.0 / std::tan(0.5 * omega[1]);
    const double p5 = +1.0 / std::tan(0.5 * omega[2]);
    const double r1 = +p1 * p1 / std::sin(omega[0]);
    const double r3 = -p3 * p3 / std::sin(omega[1]);
    const double r5 = +p5 * p5 / std::sin(omega[2]);
    const double neg_half_sigma2 = -0.5 * sigma * sigma;
    const double recip_radius = 1.0 / radius;
    double rho[3];
    for (int i = 0; i < 3; i++) rho[i] = std::exp(neg_half_sigma2 * omega[i] * omega[i]) * recip_radius;
    const double D13 = p1 * r3 - r1 * p3;
    const double D35 = p3 * r5 - r3 * p5;
    const double D51 = p5 * r1 - r5 * p1;
    const double recip_d13 = 1.0 / D13;
    const double zeta15 = D35 * recip_d13;
    const double zeta35 = D51 * recip_d13;
    // beta = A^-1 gamma with A = [[p1 p3 p5][r1 r3 r5][zeta15 zeta35 1]]
    const double a = p1, b = p3, c = p5, d = r1, e = r3, f = r5, g = zeta15, h = zeta35, i = 1.0;
    const double det = a * (e * i - f * h) - b * (d * i - f * g) + c * (d * h - e * g);
    const double id = 1.0 / det;
    const double inv[9] = {(e * i - f * h) * id, (c * h - b * i) * id, (b * f - c * e) * id,
                           (f * g - d * i) * id, (a * i - c * g) * id, (c * d - a * f) * id,
                           (d * h - e * g) * id, (b * g - a * h) * id, (a * e - b * d) * id};
    const double gamma[3] = {1.0, radius * radius - sigma * sigma, zeta15 * rho[0] + zeta35 * rho[1] + rho[2]};
    for (int k = 0; k < 3; k++) {
        const double beta = inv[3 * k] * gamma[0] + inv[3 * k + 1] * gamma[1] + inv[3 * k + 2] * gamma[2];
        mul_in[k] = (float)(-beta * std::cos(omega[k] * (radius + 1.0)));
        mul_prev[k] = (float)(2.0 * std::cos(omega[k]));
    }
}

// linear -> sRGB u8 exactly as /root/reference/src/metrics/xyb.rs:70-76,86-88 for an already
// clamped input c in [0,1]
static int xyb_linear_to_srgb_u8_host(float c)
{
    const float e = c <= 0.0031308f ? c * 12.92f : 1.055f * powf(c, 1.0f / 2.4f) - 0.055f;
    const float r = roundf(e * 255.0f);
    if (!(r > 0.0f)) return 0;
    if (r > 255.0f) return 255;
    return (int)r;
}

// thresh[k] (k = 1..255) = the smallest f32 c in [0,1] whose u8 code is >= k under the host's
// powf; thresh[0] = -inf.  The code is a monotone step function of c, so
// code(c) = #{k : thresh[k] <= c}.  Returns false if monotonicity fails in the +-256 ulp
// neighbourhood of any threshold (then the table cannot represent the host function).
bool ce_build_xyb_srgb_thresholds(float thresh[256])
{
    auto f = [](uint32_t bits) {
        float c;
        memcpy(&c, &bits, 4);
        return xyb_linear_to_srgb_u8_host(c);
    };
    const uint32_t one = 0x3f800000u;
    thresh[0] = -INFINITY;
    bool ok = true;
    for (int k = 1; k <= 255; k++) {
        if (f(one) < k) {
            thresh[k] = INFINITY;
            continue;
        }
        uint32_t lo = 0, hi = one;  // f(lo) < k <= f(hi); non-negative floats order like their bits
        if (f(lo) >= k) {
            hi = 0;
        } else {
            while (hi - lo > 1) {
                const uint32_t mid = lo + (hi - lo) / 2;
                if (f(mid) >= k) hi = mid; else lo = mid;
            }
        }
        memcpy(&thresh[k], &hi, 4);
        const uint32_t a = hi > 256 ? hi - 256 : 0, b = hi + 256 < one ? hi + 256 : one;
        for (uint32_t u = a; u <= b; u++) {
            const bool above = f(u) >= k;
            if (above != (u >= hi)) ok = false;
        }
    }
    return ok;
}

// The taps of one axis of the resampler (include/ce_metrics.h, enum ce_resample_filter), all in f64
// with the host libm as the sRGB tables above: Pillow's precompute_coeffs + normalize_coeffs_8bpc.
static double resample_sinc(double x)
{
    if (x == 0.0) return 1.0;
    x *= M_PI;
    return std::sin(x) / x;
}

static double resample_weight(int filter, double x)
{
    switch (filter) {
    case CE_RESAMPLE_BOX: return x > -0.5 && x <= 0.5 ? 1.0 : 0.0;
    case CE_RESAMPLE_BILINEAR:
        if (x < 0.0) x = -x;
        return x < 1.0 ? 1.0 - x : 0.0;
    case CE_RESAMPLE_BICUBIC: {
        const double a = -0.5;
        if (x < 0.0) x = -x;
        if (x < 1.0) return ((a + 2.0) * x - (a + 3.0)) * x * x + 1;
        if (x < 2.0) return (((x - 5) * x + 8) * x - 4) * a;
        return 0.0;
    }
    default: return -3.0 <= x && x < 3.0 ? resample_sinc(x) * resample_sinc(x / 3) : 0.0;
    }
}

bool ce_build_resample_table(uint32_t n_in, uint32_t n_out, int filter, std::vector<int32_t> &table, uint32_t *ksize_out)
{
    static const double supports[4] = {0.5, 1.0, 2.0, 3.0};
    if (filter < 0 || filter > 3 || n_in == 0 || n_out == 0) return false;
    const double scale = (double)n_in / (double)n_out;
    const double fs = scale < 1.0 ? 1.0 : scale;
    const double support = supports[filter] * fs;
    const uint32_t ksize = (uint32_t)std::ceil(support) * 2 + 1;
    table.assign((size_t)n_out * (2 + (size_t)ksize), 0);
    std::vector<double> k(ksize);
    for (uint32_t xx = 0; xx < n_out; xx++) {
        const double center = (xx + 0.5) * scale;
        int64_t xmin = (int64_t)(center - support + 0.5);
        if (xmin < 0) xmin = 0;
        int64_t xmax = (int64_t)(center + support + 0.5);
        if (xmax > (int64_t)n_in) xmax = n_in;
        const int64_t n = xmax - xmin;
        double ww = 0.0;
        for (int64_t x = 0; x < n; x++) {
            k[x] = resample_weight(filter, (x + xmin - center + 0.5) / fs);
            ww += k[x];
        }
        table[xx] = (int32_t)xmin;
        table[(size_t)n_out + xx] = (int32_t)n;
        int32_t *out = &table[2 * (size_t)n_out + (size_t)xx * ksize];
        for (int64_t x = 0; x < n; x++) {
            const double v = ww != 0.0 ? k[x] / ww : k[x];
            out[x] = v < 0 ? (int32_t)(-0.5 + v * (double)(1 << 22)) : (int32_t)(0.5 + v * (double)(1 << 22));
        }
    }
    *ksize_out = ksize;
    return true;
}

// The taps of one axis of the float resampler (ce_resample_linear): Pillow's precompute_coeffs alone,
// the weights kept as the normalised doubles.  Same geometry and ksize as above; the filter's argument is scaled by the
// reciprocal 1.0 / fs as Pillow writes it, which differs from the division above in the last bits of some bilinear taps -
// invisible after the rounding to 22 bits there, visible here.  table = n_out * (1 + ksize) doubles: the first n_out hold,
// as 2 * n_out int32, [n_out] first tap | [n_out] tap count; then [n_out][ksize] weights, zero past a sample's count.
bool ce_build_resample_table_f64(uint32_t n_in, uint32_t n_out, int filter, std::vector<double> &table, uint32_t *ksize_out)
{
    static const double supports[4] = {0.5, 1.0, 2.0, 3.0};
    if (filter < 0 || filter > 3 || n_in == 0 || n_out == 0) return false;
    const double scale = (double)n_in / (double)n_out;
    const double fs = scale < 1.0 ? 1.0 : scale;
    const double support = supports[filter] * fs;
    const double ss = 1.0 / fs;
    const uint32_t ksize = (uint32_t)std::ceil(support) * 2 + 1;
    table.assign((size_t)n_out * (1 + (size_t)ksize), 0.0);
    std::vector<int32_t> head(2 * (size_t)n_out);
    for (uint32_t xx = 0; xx < n_out; xx++) {
        const double center = (xx + 0.5) * scale;
        int64_t xmin = (int64_t)(center - support + 0.5);
        if (xmin < 0) xmin = 0;
        int64_t xmax = (int64_t)(center + support + 0.5);
        if (xmax > (int64_t)n_in) xmax = n_in;
        const int64_t n = xmax - xmin;
        double *k = &table[(size_t)n_out + (size_t)xx * ksize];
        double ww = 0.0;
        for (int64_t x = 0; x < n; x++) {
            k[x] = resample_weight(filter, (x + xmin - center + 0.5) * ss);
            ww += k[x];
        }
        if (ww != 0.0)
            for (int64_t x = 0; x < n; x++) k[x] /= ww;
        head[xx] = (int32_t)xmin;
        head[(size_t)n_out + xx] = (int32_t)n;
    }
    memcpy(table.data(), head.data(), head.size() * sizeof(int32_t));
    *ksize_out = ksize;
    return true;
}

// ---- Y'CbCr -> RGB fixed-point coefficients (include/ce_metrics.h: ce_yuv_coefficients; yuv.hip) ------------------------
// {KY, KRV, KGU, KGV, KBU, y0, c0}, every product in f64 and rounded once with rint.  BT601 uses libjpeg's literals
// (jdcolor.c), which are not the Kr / Kb quotients to the last digit: they are what makes d = D = 8 full range its table.
int ce_yuv_coefficients(int matrix, int range, uint32_t depth_in, uint32_t depth_out, int64_t out[7])
{
    if (!out) return CE_ERR_INVALID_ARG;
    if (depth_in != 8 && depth_in != 10 && depth_in != 12) return CE_ERR_INVALID_ARG;
    if (depth_out != 8 && depth_out != 10 && depth_out != 12 && depth_out != 16) return CE_ERR_INVALID_ARG;
    double a, b, c, e;
    if (matrix == CE_YUV_BT601) {
        a = 1.40200, b = 0.34414, c = 0.71414, e = 1.77200;
    } else if (matrix == CE_YUV_BT709 || matrix == CE_YUV_BT2020) {
        const double kr = matrix == CE_YUV_BT709 ? 0.2126 : 0.2627, kb = matrix == CE_YUV_BT709 ? 0.0722 : 0.0593;
        const double kg = 1.0 - kr - kb;
        a = 2.0 * (1.0 - kr), e = 2.0 * (1.0 - kb);
        b = kb * e / kg, c = kr * a / kg;
    } else {
        return CE_ERR_INVALID_ARG;
    }
    const double m = (double)((1u << depth_out) - 1u), u = (double)(1u << (depth_in - 8));
    double sy, sc;
    int64_t y0, c0;
    if (range == CE_YUV_FULL) {
        y0 = 0, c0 = (int64_t)1 << (depth_in - 1);
        sy = sc = m / (double)((1u << depth_in) - 1u);
    } else if (range == CE_YUV_LIMITED) {
        y0 = 16 << (depth_in - 8), c0 = 128 << (depth_in - 8);
        sy = m / (219.0 * u), sc = m / (224.0 * u);
    } else {
        return CE_ERR_INVALID_ARG;
    }
    out[0] = (int64_t)std::rint(sy * 65536.0);
    out[1] = (int64_t)std::rint(sc * a * 65536.0);
    out[2] = (int64_t)std::rint(sc * b * 65536.0);
    out[3] = (int64_t)std::rint(sc * c * 65536.0);
    out[4] = (int64_t)std::rint(sc * e * 65536.0);
    out[5] = y0, out[6] = c0;
    return CE_OK;
}

// ---- CICP ingest (include/ce_metrics.h: ce_transfer_table, ce_colour_matrix) --------------------------
// Transfer characteristics 13 (sRGB: the rule-0 table above), 8 (linear: v / maxv) and 16 (PQ, SMPTE ST 2084 with its
// rational constants: nits / white_nits), each in f64 per code point and rounded once to f32.
bool ce_build_transfer_table(int transfer, uint32_t maxv, double white_nits, float *lut)
{
    if (transfer == 13) {
        ce_build_srgb_table_f64(lut, maxv);
        return true;
    }
    if (transfer == 8) {
        for (uint32_t i = 0; i <= maxv; i++) lut[i] = (float)((double)i / (double)maxv);
        return true;
    }
    if (transfer == 16) {
        if (!(white_nits > 0.0) || !std::isfinite(white_nits)) return false;
        const double m1 = 2610.0 / 16384.0, m2 = 2523.0 / 4096.0 * 128.0;
        const double c1 = 3424.0 / 4096.0, c2 = 2413.0 / 4096.0 * 32.0, c3 = 2392.0 / 4096.0 * 32.0;
        for (uint32_t i = 0; i <= maxv; i++) {
            const double e = (double)i / (double)maxv;
            const double p = std::pow(e, 1.0 / m2);
            const double num = std::fmax(p - c1, 0.0), den = c2 - c3 * p;
            const double y = std::pow(num / den, 1.0 / m1);
            lut[i] = (float)(10000.0 * y / white_nits);
        }
        return true;
    }
    return false;
}

// ---- HDR fidelity (include/ce_metrics.h: ce_pq_code_thresholds, ce_hdr_fidelity_matrices) ------------
// The decision thresholds of PQ code values on linear light: T[c] = PQ_EOTF((c - 0.5) / maxv) / white_nits for c = 1 .. maxv,
// at out[c - 1], with the constants and the operation order of the PQ branch above, in f64 and rounded once to f32.
bool ce_build_pq_code_thresholds(uint32_t maxv, double white_nits, float *out)
{
    if (!(white_nits > 0.0) || !std::isfinite(white_nits)) return false;
    const double m1 = 2610.0 / 16384.0, m2 = 2523.0 / 4096.0 * 128.0;
    const double c1 = 3424.0 / 4096.0, c2 = 2413.0 / 4096.0 * 32.0, c3 = 2392.0 / 4096.0 * 32.0;
    for (uint32_t c = 1; c <= maxv; c++) {
        const double e = ((double)c - 0.5) / (double)maxv;
        const double p = std::pow(e, 1.0 / m2);
        const double num = std::fmax(p - c1, 0.0), den = c2 - c3 * p;
        const double y = std::pow(num / den, 1.0 / m1);
        out[c - 1] = (float)(10000.0 * y / white_nits);
    }
    return true;
}

namespace {
// inverse of a 3 x 3 matrix by its adjugate, every operation written out (the restatement in tests/cicp_restatement.py
// performs the same f64 operations in the same order)
void inv3(const double a[9], double o[9])
{
    const double c00 = a[4] * a[8] - a[5] * a[7], c01 = a[5] * a[6] - a[3] * a[8], c02 = a[3] * a[7] - a[4] * a[6];
    const double det = (a[0] * c00 + a[1] * c01) + a[2] * c02;
    o[0] = c00 / det;
    o[1] = (a[2] * a[7] - a[1] * a[8]) / det;
    o[2] = (a[1] * a[5] - a[2] * a[4]) / det;
    o[3] = c01 / det;
    o[4] = (a[0] * a[8] - a[2] * a[6]) / det;
    o[5] = (a[2] * a[3] - a[0] * a[5]) / det;
    o[6] = c02 / det;
    o[7] = (a[1] * a[6] - a[0] * a[7]) / det;
    o[8] = (a[0] * a[4] - a[1] * a[3]) / det;
}

// XYZ <- RGB of a set of chromaticities (x, y of red, green, blue, white): columns (x / y, 1, (1 - x - y) / y) scaled so
// that RGB = (1, 1, 1) gives the white point with Y = 1
void rgb_to_xyz(const double xy[8], double m[9])
{
    double p[9], pi[9];
    for (int c = 0; c < 3; c++) {
        const double x = xy[2 * c], y = xy[2 * c + 1];
        p[c] = x / y, p[3 + c] = 1.0, p[6 + c] = ((1.0 - x) - y) / y;
    }
    const double wx = xy[6] / xy[7], wy = 1.0, wz = ((1.0 - xy[6]) - xy[7]) / xy[7];
    inv3(p, pi);
    for (int c = 0; c < 3; c++) {
        const double s = (pi[3 * c] * wx + pi[3 * c + 1] * wy) + pi[3 * c + 2] * wz;
        for (int r = 0; r < 3; r++) m[3 * r + c] = p[3 * r + c] * s;
    }
}
}  // namespace

// Colour primaries 1 (BT.709), 9 (BT.2020) and 12 (Display P3, D65), H.273's chromaticities: M = inv(XYZ <- sRGB) * (XYZ <-
// src) in f64, rounded once to f32; primaries 1 gives the identity (the ingest does not multiply then).
static const double k709[8] = {0.640, 0.330, 0.300, 0.600, 0.150, 0.060, 0.3127, 0.3290};
static const double k2020[8] = {0.708, 0.292, 0.170, 0.797, 0.131, 0.046, 0.3127, 0.3290};
static const double kP3[8] = {0.680, 0.320, 0.265, 0.690, 0.150, 0.060, 0.3127, 0.3290};

bool ce_build_colour_matrix(int primaries, float m[9])
{
    if (primaries == 1) {
        for (int i = 0; i < 9; i++) m[i] = (i % 4 == 0) ? 1.0f : 0.0f;
        return true;
    }
    const double *src = primaries == 9 ? k2020 : primaries == 12 ? kP3 : nullptr;
    if (!src) return false;
    double a[9], ai[9], s[9];
    rgb_to_xyz(k709, a);
    inv3(a, ai);
    rgb_to_xyz(src, s);
    for (int r = 0; r < 3; r++)
        for (int c = 0; c < 3; c++) m[3 * r + c] = (float)((ai[3 * r] * s[c] + ai[3 * r + 1] * s[3 + c]) + ai[3 * r + 2] * s[6 + c]);
    return true;
}

// HDR fidelity's two matrices, row-major: a = the inverse of ce_build_colour_matrix(9) - of the f32 matrix the ingest multiplies
// by - taken in f64 by inv3 and rounded once to f32 (BT.2020 <- sRGB primaries); b = BT.2100's LMS <- BT.2020, n / 4096 each,
// exact in f32.
void ce_build_hdr_fidelity_matrices(float a[9], float b[9])
{
    static const int lms[9] = {1688, 2146, 262, 683, 2951, 462, 99, 309, 3688};
    float m[9];
    double md[9], inv[9];
    ce_build_colour_matrix(9, m);
    for (int i = 0; i < 9; i++) md[i] = (double)m[i];
    inv3(md, inv);
    for (int i = 0; i < 9; i++) a[i] = (float)inv[i], b[i] = (float)((double)lms[i] / 4096.0);
}

// ---- HLG ingest (include/ce_metrics.h: ce_hlg_table, ce_hlg_params) --------------------------------
// BT.2100's HLG inverse OETF with its published constants, in f64 per code point x = v / maxv and rounded once to f32:
// scene light in [0, 1].  The f64 value at x = 1 is 1.00000003, which rounds to 1.0f.
void ce_build_hlg_table(uint32_t maxv, float *lut)
{
    const double a = 0.17883277, b = 0.28466892, c = 0.55991073;
    for (uint32_t i = 0; i <= maxv; i++) {
        const double x = (double)i / (double)maxv;
        lut[i] = (float)(x <= 0.5 ? x * x / 3.0 : (std::exp((x - c) / a) + b) / 12.0);
    }
}

// The luminance coefficients of the tagged primaries: the Y row of the f64 XYZ <- src matrix ce_build_colour_matrix starts
// from (BT.2020: 0.2627, 0.6780, 0.0593 at four decimals).
bool ce_build_luminance_row(int primaries, double k[3])
{
    const double *src = primaries == 1 ? k709 : primaries == 9 ? k2020 : primaries == 12 ? kP3 : nullptr;
    if (!src) return false;
    double m[9];
    rgb_to_xyz(src, m);
    k[0] = m[3], k[1] = m[4], k[2] = m[5];
    return true;
}

// ---- gain-map ingest (include/ce_metrics.h: ce_gainmap_weight, ce_gainmap_tables) ------------------
// W = clamp((display - base) / (alternate - base), 0, 1) over the three log2 headrooms, in f64; alternate != base was checked
double ce_build_gainmap_weight(const ce_gainmap *g)
{
    const double w = ((double)g->display_headroom - (double)g->base_headroom) / ((double)g->alternate_headroom - (double)g->base_headroom);
    return w < 0.0 ? 0.0 : (w > 1.0 ? 1.0 : w);
}

// Y_c[v] = W * (gain_min_c + (gain_max_c - gain_min_c) * (v / 255)^(1 / gamma_c)) in f64, every operation rounded separately;
// gamma_c == 1 takes no power, so that Y_c is affine in v to the last bit
void ce_build_gainmap_tables(const ce_gainmap *g, uint32_t channels, double *out)
{
    const double w = ce_build_gainmap_weight(g);
    for (uint32_t c = 0; c < channels; c++) {
        const double lo = (double)g->gain_min[c], span = (double)g->gain_max[c] - lo, inv_gamma = 1.0 / (double)g->gamma[c];
        for (int v = 0; v < 256; v++) {
            const double x = (double)v / 255.0;
            const double e = g->gamma[c] == 1.0f ? x : std::pow(x, inv_gamma);
            const double scaled = span * e;
            out[256 * c + v] = w * (lo + scaled);
        }
    }
}
