// LUT-based ICC profiles on the host (include/ce_metrics.h: ce_icc_lut_describe and the ce_icc_lut_build_* functions; DESIGN.md
// section 23): the parser of A2B tags of type mAB, mft2 and mft1 and the builders of exactly what the device is handed.  Like
// ce_icc.cpp nothing here touches the GPU or the rest of the runtime - the file includes the public header alone - so
// tests/cpp/icc_lut_parse_host.cpp builds it into a stand-alone program under the host sanitizers.  Every read of the profile
// goes through be16 / be32 / u8 behind a check of its offset: a tag-table entry against `end`, the header's size field once
// that is known to lie within the buffer, and everything inside the tag against the tag's own size, counts compared in size_t
// before they are multiplied.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <initializer_list>

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

// the canonical sRGB profile's colorants, row-major (rows X Y Z, columns r g b): ce_icc.cpp's
constexpr int32_t kSrgbColorants[9] = {0x6FA2, 0x6299, 0x24A0, 0x38F5, 0xB785, 0x0F84, 0x0390, 0x18DA, 0xB6CF};

int refuse(ce_icc_lut_description *d, int kind, const char *why)
{
    d->kind = kind;
    std::snprintf(d->reason, sizeof d->reason, "%s", why);
    return kind;
}

// One element of a curve sequence at `at` inside the tag [t, t + size): `curv` or `para`, its numbers into c (offsets are the
// profile's), *used = the element's bytes before padding.  The rules of ce_icc.cpp's parse_curve.
const char *parse_curve(const uint8_t *bytes, uint32_t t, size_t size, size_t at, ce_icc_curve *c, size_t *used)
{
    if (at > size || size - at < 12) return "a curve element runs past the tag";
    const uint8_t *p = bytes + t + at;
    const size_t room = size - at - 12;
    const uint32_t type = be32(p);
    if (type == sig('c', 'u', 'r', 'v')) {
        const uint32_t n = be32(p + 8);
        if (n > CE_ICC_MAX_CURVE_POINTS) return "a curv element has more samples than CE_ICC_MAX_CURVE_POINTS";
        if ((size_t)n * 2 > room) return "a curv element's samples run past the tag";
        c->type = CE_ICC_CURVE_CURV, c->count = n;
        if (n == 1) c->params[0] = (int32_t)be16(p + 12);
        if (n >= 2) c->offset = t + (uint32_t)at + 12;
        *used = 12 + (size_t)n * 2;
        return nullptr;
    }
    if (type == sig('p', 'a', 'r', 'a')) {
        const uint32_t f = be16(p + 8);
        if (f > 4) return "a para element's function type is above 4";
        static const uint32_t kCount[5] = {1, 3, 4, 5, 7};
        if ((size_t)kCount[f] * 4 > room) return "a para element's parameters run past the tag";
        c->type = CE_ICC_CURVE_PARA, c->count = f;
        for (uint32_t i = 0; i < kCount[f]; i++) c->params[i] = s15f16(p + 12 + 4 * i);
        if ((f == 1 || f == 2) && c->params[1] == 0) return "a para element of type 1 or 2 has a = 0: its breakpoint -b / a is not defined";
        *used = 12 + (size_t)kCount[f] * 4;
        return nullptr;
    }
    return "a curve element is neither curv nor para";
}

// three elements from `at` on, each padded to a multiple of 4 bytes
const char *parse_curves(const uint8_t *bytes, uint32_t t, size_t size, size_t at, ce_icc_curve (&c)[3])
{
    for (int k = 0; k < 3; k++) {
        size_t used = 0;
        if (const char *why = parse_curve(bytes, t, size, at, &c[k], &used)) return why;
        at += (used + 3) & ~(size_t)3;  // a padded end past the tag is caught by the next element's check; the last needs no padding
    }
    return nullptr;
}

// grid sizes checked, the node count (at most CE_ICC_MAX_CLUT_NODES) into *nodes
const char *check_grid(const uint32_t (&g)[3], size_t *nodes)
{
    for (int k = 0; k < 3; k++)
        if (g[k] < 2 || g[k] > 255) return "a CLUT grid size is outside [2, 255]";
    const size_t n = (size_t)g[0] * g[1] * g[2];  // at most 255^3
    if (n > CE_ICC_MAX_CLUT_NODES) return "the CLUT has more nodes than CE_ICC_MAX_CLUT_NODES";
    *nodes = n;
    return nullptr;
}

int parse_mab(const uint8_t *bytes, uint32_t t, size_t size, ce_icc_lut_description *d)
{
    if (size < 32) return refuse(d, CE_ICC_LUT_MALFORMED, "an mAB tag is under 32 bytes");
    const uint8_t *p = bytes + t;
    if (p[8] != 3 || p[9] != 3) return refuse(d, CE_ICC_LUT_UNSUPPORTED, "the tag does not have 3 input and 3 output channels");
    const size_t off_b = be32(p + 12), off_mat = be32(p + 16), off_m = be32(p + 20), off_clut = be32(p + 24), off_a = be32(p + 28);
    if (!off_b) return refuse(d, CE_ICC_LUT_MALFORMED, "an mAB tag has no B curves");
    if ((off_m != 0) != (off_mat != 0)) return refuse(d, CE_ICC_LUT_MALFORMED, "an mAB tag has M curves without a matrix or a matrix without M curves");
    if ((off_a != 0) != (off_clut != 0)) return refuse(d, CE_ICC_LUT_MALFORMED, "an mAB tag has A curves without a CLUT or a CLUT without A curves");
    for (size_t off : {off_b, off_mat, off_m, off_clut, off_a})
        if (off != 0 && (off < 32 || off > size)) return refuse(d, CE_ICC_LUT_MALFORMED, "an mAB offset points outside the tag");
    d->stages = CE_ICC_STAGE_B;
    if (const char *why = parse_curves(bytes, t, size, off_b, d->b)) return refuse(d, CE_ICC_LUT_MALFORMED, why);
    if (off_m) {
        d->stages |= CE_ICC_STAGE_M | CE_ICC_STAGE_MATRIX;
        if (const char *why = parse_curves(bytes, t, size, off_m, d->m)) return refuse(d, CE_ICC_LUT_MALFORMED, why);
        if (size - off_mat < 48) return refuse(d, CE_ICC_LUT_MALFORMED, "the mAB matrix runs past the tag");
        for (int i = 0; i < 12; i++) d->matrix[i] = s15f16(p + off_mat + 4 * i);
    }
    if (off_a) {
        d->stages |= CE_ICC_STAGE_A | CE_ICC_STAGE_CLUT;
        if (const char *why = parse_curves(bytes, t, size, off_a, d->a)) return refuse(d, CE_ICC_LUT_MALFORMED, why);
        if (size - off_clut < 20) return refuse(d, CE_ICC_LUT_MALFORMED, "the mAB CLUT header runs past the tag");
        for (int k = 0; k < 3; k++) d->grid[k] = p[off_clut + k];
        d->precision = p[off_clut + 16];
        if (d->precision != 1 && d->precision != 2) return refuse(d, CE_ICC_LUT_MALFORMED, "the CLUT precision is neither 1 nor 2");
        size_t nodes = 0;
        if (const char *why = check_grid(d->grid, &nodes)) return refuse(d, CE_ICC_LUT_MALFORMED, why);
        if (nodes * 3 * d->precision > size - off_clut - 20) return refuse(d, CE_ICC_LUT_MALFORMED, "the CLUT runs past the tag");
        d->clut_offset = t + (uint32_t)off_clut + 20;
    }
    return CE_ICC_LUT_SUPPORTED;
}

int parse_mft(const uint8_t *bytes, uint32_t t, size_t size, bool wide, ce_icc_lut_description *d)
{
    const size_t head = wide ? 52 : 48;
    if (size < head) return refuse(d, CE_ICC_LUT_MALFORMED, "an mft tag is shorter than its header");
    const uint8_t *p = bytes + t;
    if (p[8] != 3 || p[9] != 3) return refuse(d, CE_ICC_LUT_UNSUPPORTED, "the tag does not have 3 input and 3 output channels");
    if (!wide && d->pcs == sig('X', 'Y', 'Z', ' ')) return refuse(d, CE_ICC_LUT_UNSUPPORTED, "an mft1 tag with PCS XYZ: the format has no 8-bit XYZ encoding");
    d->grid[0] = d->grid[1] = d->grid[2] = p[10];
    d->precision = wide ? 2 : 1;
    for (int i = 0; i < 9; i++) d->matrix[i] = s15f16(p + 12 + 4 * i);
    const size_t n_in = wide ? be16(p + 48) : 256, n_out = wide ? be16(p + 50) : 256;
    if (n_in < 2 || n_in > 4096 || n_out < 2 || n_out > 4096) return refuse(d, CE_ICC_LUT_MALFORMED, "an mft2 table count is outside [2, 4096]");
    size_t nodes = 0;
    if (const char *why = check_grid(d->grid, &nodes)) return refuse(d, CE_ICC_LUT_MALFORMED, why);
    const size_t sample = d->precision, room = size - head;
    if (3 * n_in * sample > room) return refuse(d, CE_ICC_LUT_MALFORMED, "the input tables run past the tag");
    if (nodes * 3 * sample > room - 3 * n_in * sample) return refuse(d, CE_ICC_LUT_MALFORMED, "the CLUT runs past the tag");
    if (3 * n_out * sample > room - 3 * n_in * sample - nodes * 3 * sample) return refuse(d, CE_ICC_LUT_MALFORMED, "the output tables run past the tag");
    d->stages = CE_ICC_STAGE_A | CE_ICC_STAGE_CLUT | CE_ICC_STAGE_B;
    const uint32_t in_at = t + (uint32_t)head;
    d->clut_offset = in_at + (uint32_t)(3 * n_in * sample);
    const uint32_t out_at = d->clut_offset + (uint32_t)(nodes * 3 * sample);
    for (uint32_t c = 0; c < 3; c++) {
        d->a[c].type = d->b[c].type = wide ? CE_ICC_CURVE_CURV : CE_ICC_CURVE_TABLE8;
        d->a[c].count = (uint32_t)n_in, d->a[c].offset = in_at + c * (uint32_t)(n_in * sample);
        d->b[c].count = (uint32_t)n_out, d->b[c].offset = out_at + c * (uint32_t)(n_out * sample);
    }
    return CE_ICC_LUT_SUPPORTED;
}

// the whole of ce_icc_lut_describe; returns the kind
int describe(const uint8_t *bytes, size_t len, int intent, ce_icc_lut_description *d)
{
    std::memset(d, 0, sizeof *d);
    if (len < 132) return refuse(d, CE_ICC_LUT_MALFORMED, "shorter than a header and a tag count");
    if (len > CE_ICC_MAX_PROFILE_BYTES) return refuse(d, CE_ICC_LUT_MALFORMED, "longer than CE_ICC_MAX_PROFILE_BYTES");
    const uint32_t end = be32(bytes);
    if (end < 132 || end > len) return refuse(d, CE_ICC_LUT_MALFORMED, "the header's size field does not lie within the buffer");
    if (be32(bytes + 36) != sig('a', 'c', 's', 'p')) return refuse(d, CE_ICC_LUT_MALFORMED, "no acsp signature");
    d->version = be32(bytes + 8);
    d->profile_class = be32(bytes + 12);
    d->pcs = be32(bytes + 20);
    if ((d->version >> 24) != 2 && (d->version >> 24) != 4) return refuse(d, CE_ICC_LUT_MALFORMED, "the version is neither 2 nor 4");
    const uint32_t n_tags = be32(bytes + 128);
    if (n_tags > (end - 132) / 12) return refuse(d, CE_ICC_LUT_MALFORMED, "the tag table runs past the profile");
    uint32_t at[3] = {}, size[3] = {};
    bool found[3] = {};
    for (uint32_t i = 0; i < n_tags; i++) {
        const uint8_t *e = bytes + 132 + (size_t)12 * i;
        const uint32_t s = be32(e), off = be32(e + 4), sz = be32(e + 8);
        if (off > end || sz > end - off) return refuse(d, CE_ICC_LUT_MALFORMED, "a tag lies outside the profile");
        for (uint32_t k = 0; k < 3; k++)
            if (s == sig('A', '2', 'B', (char)('0' + k)) && !found[k]) at[k] = off, size[k] = sz, found[k] = true;
    }
    if (!found[0] && !found[1] && !found[2]) return refuse(d, CE_ICC_LUT_NOT_LUT, "the profile has no A2B tag: it is not LUT-based");
    if (be32(bytes + 16) != sig('R', 'G', 'B', ' ')) return refuse(d, CE_ICC_LUT_UNSUPPORTED, "the data colour space is not RGB");
    if (d->pcs != sig('X', 'Y', 'Z', ' ') && d->pcs != sig('L', 'a', 'b', ' ')) return refuse(d, CE_ICC_LUT_UNSUPPORTED, "the PCS is neither XYZ nor Lab");
    if (d->profile_class != sig('m', 'n', 't', 'r') && d->profile_class != sig('s', 'c', 'n', 'r') && d->profile_class != sig('s', 'p', 'a', 'c'))
        return refuse(d, CE_ICC_LUT_UNSUPPORTED, "the class is not mntr, scnr or spac");
    const int k = found[intent] ? intent : 0;
    if (!found[k]) return refuse(d, CE_ICC_LUT_MALFORMED, "the profile has an A2B1 or A2B2 tag and no A2B0");
    d->tag = sig('A', '2', 'B', (char)('0' + k)), d->tag_offset = at[k], d->tag_size = size[k];
    if (size[k] < 12) return refuse(d, CE_ICC_LUT_MALFORMED, "the A2B tag is under 12 bytes");
    d->tag_type = be32(bytes + at[k]);
    if (d->tag_type == sig('m', 'A', 'B', ' ')) return d->kind = parse_mab(bytes, at[k], size[k], d);
    if (d->tag_type == sig('m', 'f', 't', '2')) return d->kind = parse_mft(bytes, at[k], size[k], true, d);
    if (d->tag_type == sig('m', 'f', 't', '1')) return d->kind = parse_mft(bytes, at[k], size[k], false, d);
    return refuse(d, CE_ICC_LUT_MALFORMED, "the A2B tag is not of type mAB, mft2 or mft1");
}

double clip01(double y) { return !(y > 0.0) ? 0.0 : (y > 1.0 ? 1.0 : y); }
double power(double base, double g) { return std::pow(base > 0.0 ? base : 0.0, g); }

// sample i of a checked sampled curve, in f64
double sample_at(const uint8_t *bytes, const ce_icc_curve &c, size_t i)
{
    return c.type == CE_ICC_CURVE_TABLE8 ? (double)bytes[c.offset + i] / 255.0 : (double)be16(bytes + c.offset + 2 * i) / 65535.0;
}

// a checked input-side curve at e in [0, 1], before the clip: ce_icc.cpp's curve_at with the u8 tables of mft1
double curve_at(const uint8_t *bytes, const ce_icc_curve &c, double e)
{
    if (c.type != CE_ICC_CURVE_PARA) {
        if (c.count == 0) return e;
        if (c.count == 1) return power(e, (double)c.params[0] / 256.0);
        const double p = e * (double)(c.count - 1);
        size_t i = (size_t)p;
        if (i > c.count - 2) i = c.count - 2;
        const double s0 = sample_at(bytes, c, i), s1 = sample_at(bytes, c, i + 1);
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

// ce_colour_matrix's inverse: the adjugate over the determinant, every operation written out (ce_icc.cpp's)
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
bool supported(const uint8_t *bytes, size_t len, int intent, ce_icc_lut_description *d)
{
    return bytes && intent >= 0 && intent <= 2 && describe(bytes, len, intent, d) == CE_ICC_LUT_SUPPORTED;
}

}  // namespace

extern "C" {

int ce_icc_lut_describe(const uint8_t *bytes, size_t len, int intent, ce_icc_lut_description *out)
{
    if (!bytes || !out || intent < 0 || intent > 2) return CE_ERR_INVALID_ARG;
    describe(bytes, len, intent, out);
    return CE_OK;
}

int ce_icc_lut_build_input_tables(const uint8_t *bytes, size_t len, int intent, uint32_t depth, float *out, size_t n)
{
    ce_icc_lut_description d;
    if (!out || !depth_ok(depth) || n != ((size_t)3 << depth) || !supported(bytes, len, intent, &d)) return CE_ERR_INVALID_ARG;
    const uint32_t maxv = (1u << depth) - 1u;
    for (int c = 0; c < 3; c++)
        for (uint32_t v = 0; v <= maxv; v++) {
            const double e = (double)v / (double)maxv;
            out[((size_t)c << depth) + v] = (float)clip01((d.stages & CE_ICC_STAGE_A) ? curve_at(bytes, d.a[c], e) : e);
        }
    return CE_OK;
}

int ce_icc_lut_build_clut(const uint8_t *bytes, size_t len, int intent, float *out, size_t n)
{
    ce_icc_lut_description d;
    if (!supported(bytes, len, intent, &d)) return CE_ERR_INVALID_ARG;
    const size_t nodes = (d.stages & CE_ICC_STAGE_CLUT) ? (size_t)d.grid[0] * d.grid[1] * d.grid[2] : 0;
    if (n != nodes * 4 || (nodes && !out)) return CE_ERR_INVALID_ARG;
    for (size_t i = 0; i < nodes; i++) {
        for (size_t k = 0; k < 3; k++)
            out[4 * i + k] = d.precision == 1 ? (float)((double)bytes[d.clut_offset + 3 * i + k] / 255.0)
                                              : (float)((double)be16(bytes + d.clut_offset + 2 * (3 * i + k)) / 65535.0);
        out[4 * i + 3] = 0.0f;
    }
    return CE_OK;
}

int ce_icc_lut_build_matrix(const uint8_t *bytes, size_t len, int intent, float out[12])
{
    ce_icc_lut_description d;
    if (!out || !supported(bytes, len, intent, &d)) return CE_ERR_INVALID_ARG;
    for (int i = 0; i < 12; i++)
        out[i] = (d.stages & CE_ICC_STAGE_MATRIX) ? (float)((double)d.matrix[i] / 65536.0) : ((i < 9 && i % 4 == 0) ? 1.0f : 0.0f);
    return CE_OK;
}

int ce_icc_lut_build_curves(const uint8_t *bytes, size_t len, int intent, ce_icc_lut_curve out[6], float *samples, size_t n_samples, size_t *needed)
{
    ce_icc_lut_description d;
    if (!out || !needed || !supported(bytes, len, intent, &d)) return CE_ERR_INVALID_ARG;
    size_t total = 0;
    for (int k = 0; k < 6; k++) {
        const bool present = k < 3 ? (d.stages & CE_ICC_STAGE_M) != 0 : (d.stages & CE_ICC_STAGE_B) != 0;
        const ce_icc_curve &c = k < 3 ? d.m[k] : d.b[k - 3];
        if (present && c.type != CE_ICC_CURVE_PARA && c.count >= 2) total += c.count;
    }
    *needed = total;
    if (total > n_samples || (total && !samples)) return CE_ERR_BAD_LENGTH;
    size_t at = 0;
    for (int k = 0; k < 6; k++) {
        const bool present = k < 3 ? (d.stages & CE_ICC_STAGE_M) != 0 : (d.stages & CE_ICC_STAGE_B) != 0;
        const ce_icc_curve &c = k < 3 ? d.m[k] : d.b[k - 3];
        ce_icc_lut_curve &o = out[k];
        std::memset(&o, 0, sizeof o);
        if (!present || (c.type == CE_ICC_CURVE_CURV && c.count == 0)) continue;  // CE_ICC_LUT_CURVE_IDENTITY
        if (c.type == CE_ICC_CURVE_PARA) {
            o.kind = CE_ICC_LUT_CURVE_POWER, o.ftype = c.count;
            for (int i = 0; i < 7; i++) o.q[i] = (double)c.params[i] / 65536.0;
        } else if (c.count == 1) {
            o.kind = CE_ICC_LUT_CURVE_POWER, o.ftype = 0, o.q[0] = (double)c.params[0] / 256.0;
        } else {
            o.kind = CE_ICC_LUT_CURVE_SAMPLED, o.count = c.count, o.first_sample = (uint32_t)at;
            for (size_t i = 0; i < c.count; i++) samples[at + i] = (float)sample_at(bytes, c, i);
            at += c.count;
        }
    }
    return CE_OK;
}

int ce_icc_lut_build_pcs_matrix(float out[9])
{
    if (!out) return CE_ERR_INVALID_ARG;
    double a[9], ai[9];
    for (int i = 0; i < 9; i++) a[i] = (double)kSrgbColorants[i] / 65536.0;
    inv3(a, ai);
    for (int i = 0; i < 9; i++) out[i] = (float)ai[i];
    return CE_OK;
}

}  // extern "C"
