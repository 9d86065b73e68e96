// Matrix/TRC ICC profiles on the host (include/ce_metrics.h: ce_icc_describe, ce_icc_build_matrix, ce_icc_build_tables,
// ce_srgb_encode_thresholds): the parser and the builders of what the device gathers from.  Nothing here
// touches the GPU or the rest of the runtime - the file includes the public header alone - so tests/cpp/icc_parse_host.cpp
// builds it into a stand-alone program under the host sanitizers.  Every read of the profile goes through be16 / be32 behind
// a check of its offset against `end`, the header's size field once that is known to lie within the buffer.
#include <cmath>
#include <cstdio>
#include <cstring>

#include "ce_metrics.h"

namespace {

uint32_t be32(const uint8_t *p) { return ((uint32_t)p[0] << 24) | ((uint32_t)p[1] << 16) | ((uint32_t)p[2] << 8) | (uint32_t)p[3]; }
uint32_t be16(const uint8_t *p) { return ((uint32_t)p[0] << 8) | (uint32_t)p[1]; }
int32_t s15f16(const uint8_t *p)
{
    const uint32_t u = be32(p);
    int32_t v;
    std::memcpy(&v, &u, 4);
    return v;
}
constexpr uint32_t sig(char a, char b, char c, char d)
{
    return ((uint32_t)(uint8_t)a << 24) | ((uint32_t)(uint8_t)b << 16) | ((uint32_t)(uint8_t)c << 8) | (uint32_t)(uint8_t)d;
}

// the canonical sRGB profile's colorants, row-major (rows X Y Z, columns r g b)
constexpr int32_t kSrgbColorants[9] = {0x6FA2, 0x6299, 0x24A0, 0x38F5, 0xB785, 0x0F84, 0x0390, 0x18DA, 0xB6CF};

int refuse(ce_icc_description *d, int kind, const char *why)
{
    d->kind = kind;
    std::snprintf(d->reason, sizeof d->reason, "%s", why);
    return kind;
}

// one tag of the table: where its data lies, checked against the profile
struct tag_at {
    uint32_t offset = 0, size = 0;
    bool found = false;
};

// rTRC / gTRC / bTRC at t: `curv` or `para`, its numbers into c
const char *parse_curve(const uint8_t *bytes, tag_at t, ce_icc_curve *c)
{
    if (t.size < 12) return "a TRC tag is under 12 bytes";
    const uint8_t *p = bytes + t.offset;
    const uint32_t type = be32(p);
    if (type == sig('c', 'u', 'r', 'v')) {
        const uint32_t n = be32(p + 8);
        if (n > CE_ICC_MAX_CURVE_POINTS) return "a curv tag has more samples than CE_ICC_MAX_CURVE_POINTS";
        if ((size_t)n * 2 > (size_t)t.size - 12) return "a curv tag's samples run past the tag";
        c->type = CE_ICC_CURVE_CURV, c->count = n;
        if (n == 1) c->params[0] = (int32_t)be16(p + 12);
        if (n >= 2) c->offset = t.offset + 12;
        return nullptr;
    }
    if (type == sig('p', 'a', 'r', 'a')) {
        const uint32_t f = be16(p + 8);
        if (f > 4) return "a para tag's function type is above 4";
        static const uint32_t kCount[5] = {1, 3, 4, 5, 7};
        if ((size_t)kCount[f] * 4 > (size_t)t.size - 12) return "a para tag's parameters run past the tag";
        c->type = CE_ICC_CURVE_PARA, c->count = f;
        for (uint32_t i = 0; i < kCount[f]; i++) c->params[i] = s15f16(p + 12 + 4 * i);
        if ((f == 1 || f == 2) && c->params[1] == 0) return "a para tag of type 1 or 2 has a = 0: its breakpoint -b / a is not defined";
        return nullptr;
    }
    return "a TRC tag is neither curv nor para";
}

// the whole of ce_icc_describe; returns the kind
int describe(const uint8_t *bytes, size_t len, ce_icc_description *d)
{
    std::memset(d, 0, sizeof *d);
    if (len < 132) return refuse(d, CE_ICC_MALFORMED, "shorter than a header and a tag count");
    if (len > CE_ICC_MAX_PROFILE_BYTES) return refuse(d, CE_ICC_MALFORMED, "longer than CE_ICC_MAX_PROFILE_BYTES");
    const uint32_t end = be32(bytes);
    if (end < 132 || end > len) return refuse(d, CE_ICC_MALFORMED, "the header's size field does not lie within the buffer");
    if (be32(bytes + 36) != sig('a', 'c', 's', 'p')) return refuse(d, CE_ICC_MALFORMED, "no acsp signature");
    d->version = be32(bytes + 8);
    d->profile_class = be32(bytes + 12);
    if ((d->version >> 24) != 2 && (d->version >> 24) != 4) return refuse(d, CE_ICC_MALFORMED, "the version is neither 2 nor 4");
    if (be32(bytes + 16) != sig('R', 'G', 'B', ' ')) return refuse(d, CE_ICC_NOT_RGB_XYZ, "the data colour space is not RGB");
    if (be32(bytes + 20) != sig('X', 'Y', 'Z', ' ')) return refuse(d, CE_ICC_NOT_RGB_XYZ, "the PCS is not XYZ");
    if (d->profile_class != sig('m', 'n', 't', 'r') && d->profile_class != sig('s', 'c', 'n', 'r') && d->profile_class != sig('s', 'p', 'a', 'c'))
        return refuse(d, CE_ICC_NOT_RGB_XYZ, "the class is not mntr, scnr or spac");
    const uint32_t n_tags = be32(bytes + 128);
    if (n_tags > (end - 132) / 12) return refuse(d, CE_ICC_MALFORMED, "the tag table runs past the profile");
    static const uint32_t kWanted[6] = {sig('r', 'X', 'Y', 'Z'), sig('g', 'X', 'Y', 'Z'), sig('b', 'X', 'Y', 'Z'),
                                        sig('r', 'T', 'R', 'C'), sig('g', 'T', 'R', 'C'), sig('b', 'T', 'R', 'C')};
    tag_at tags[6];
    bool lut = false;
    for (uint32_t i = 0; i < n_tags; i++) {
        const uint8_t *e = bytes + 132 + (size_t)12 * i;
        const uint32_t s = be32(e), off = be32(e + 4), size = be32(e + 8);
        if (off > end || size > end - off) return refuse(d, CE_ICC_MALFORMED, "a tag lies outside the profile");
        if (s == sig('A', '2', 'B', '0') || s == sig('A', '2', 'B', '1') || s == sig('A', '2', 'B', '2')) lut = true;
        for (int k = 0; k < 6; k++)
            if (s == kWanted[k] && !tags[k].found) tags[k] = tag_at{off, size, true};
    }
    if (lut) return refuse(d, CE_ICC_LUT_BASED, "the profile carries an A2B tag: it is LUT-based");
    for (int k = 0; k < 6; k++)
        if (!tags[k].found) return refuse(d, CE_ICC_MALFORMED, "a colorant or TRC tag is missing");
    for (int c = 0; c < 3; c++) {
        if (tags[c].size < 20 || be32(bytes + tags[c].offset) != sig('X', 'Y', 'Z', ' '))
            return refuse(d, CE_ICC_MALFORMED, "a colorant tag is not an XYZ of 20 bytes");
        for (int r = 0; r < 3; r++) d->colorants[3 * r + c] = s15f16(bytes + tags[c].offset + 8 + 4 * r);
    }
    for (int c = 0; c < 3; c++)
        if (const char *why = parse_curve(bytes, tags[3 + c], &d->curves[c])) return refuse(d, CE_ICC_MALFORMED, why);
    d->kind = CE_ICC_SUPPORTED;
    return CE_ICC_SUPPORTED;
}

double clip01(double y) { return !(y > 0.0) ? 0.0 : (y > 1.0 ? 1.0 : y); }
double power(double base, double g) { return std::pow(base > 0.0 ? base : 0.0, g); }

// a checked curve at e, before the clip
double curve_at(const uint8_t *bytes, const ce_icc_curve &c, double e)
{
    if (c.type == CE_ICC_CURVE_CURV) {
        if (c.count == 0) return e;
        if (c.count == 1) return power(e, (double)c.params[0] / 256.0);
        const double p = e * (double)(c.count - 1);
        size_t i = (size_t)p;  // e in [0, 1]: p in [0, n - 1]
        if (i > c.count - 2) i = c.count - 2;
        const double s0 = (double)be16(bytes + c.offset + 2 * i) / 65535.0, s1 = (double)be16(bytes + c.offset + 2 * i + 2) / 65535.0;
        return s0 + (s1 - s0) * (p - (double)i);
    }
    double q[7];
    for (int i = 0; i < 7; i++) q[i] = (double)c.params[i] / 65536.0;
    const double g = q[0], a = q[1], b = q[2], cc = q[3], dd = q[4], ee = q[5], ff = q[6];
    switch (c.count) {
        case 0: return power(e, g);
        case 1: return e >= -b / a ? power(a * e + b, g) : 0.0;
        case 2: return e >= -b / a ? power(a * e + b, g) + cc : cc;
        case 3: return e >= dd ? power(a * e + b, g) : cc * e;
        default: return e >= dd ? power(a * e + b, g) + ee : cc * e + ff;
    }
}

// ce_colour_matrix's inverse: the adjugate over the determinant, every operation written out
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

bool depth_ok(uint32_t d) { return d == 8 || d == 10 || d == 12 || d == 16; }

}  // namespace

extern "C" {

int ce_icc_describe(const uint8_t *bytes, size_t len, ce_icc_description *out)
{
    if (!bytes || !out) return CE_ERR_INVALID_ARG;
    describe(bytes, len, out);
    return CE_OK;
}

int ce_icc_build_matrix(const uint8_t *bytes, size_t len, float out[9])
{
    ce_icc_description d;
    if (!bytes || !out || describe(bytes, len, &d) != CE_ICC_SUPPORTED) return CE_ERR_INVALID_ARG;
    if (std::memcmp(d.colorants, kSrgbColorants, sizeof kSrgbColorants) == 0) {
        for (int i = 0; i < 9; i++) out[i] = (i % 4 == 0) ? 1.0f : 0.0f;
        return CE_OK;
    }
    double a[9], ai[9], p[9];
    for (int i = 0; i < 9; i++) a[i] = (double)kSrgbColorants[i] / 65536.0, p[i] = (double)d.colorants[i] / 65536.0;
    inv3(a, ai);
    for (int r = 0; r < 3; r++)
        for (int c = 0; c < 3; c++) out[3 * r + c] = (float)((ai[3 * r] * p[c] + ai[3 * r + 1] * p[3 + c]) + ai[3 * r + 2] * p[6 + c]);
    return CE_OK;
}

int ce_icc_build_tables(const uint8_t *bytes, size_t len, uint32_t depth, float *out, size_t n)
{
    ce_icc_description d;
    if (!bytes || !out || !depth_ok(depth) || n != ((size_t)3 << depth) || describe(bytes, len, &d) != CE_ICC_SUPPORTED) return CE_ERR_INVALID_ARG;
    const uint32_t maxv = (1u << depth) - 1u;
    for (int c = 0; c < 3; c++)
        for (uint32_t v = 0; v <= maxv; v++)
            out[((size_t)c << depth) + v] = (float)clip01(curve_at(bytes, d.curves[c], (double)v / (double)maxv));
    return CE_OK;
}

int ce_srgb_encode_thresholds(uint32_t depth, float *out, size_t n)
{
    if (!out || !depth_ok(depth) || n != ((size_t)1 << depth) - 1) return CE_ERR_INVALID_ARG;
    const uint32_t maxv = (1u << depth) - 1u;
    for (uint32_t k = 1; k <= maxv; k++) {
        const double v = ((double)k - 0.5) / (double)maxv;
        out[k - 1] = (float)(v <= 0.04045 ? v / 12.92 : std::pow((v + 0.055) / 1.055, 2.4));
    }
    return CE_OK;
}

}  // extern "C"
