// Butteraugli on gfx950 — replaces butteraugli::butteraugli(..).score behind
// /root/reference/src/metrics/butteraugli.rs:72-80,127-135 (and compute_butteraugli(..).score in the
// codec-compare bins).  Restates libjxl's butteraugli.cc pipeline stage by stage, in the same f32
// operation order as the CPU restatement (oracle/butteraugli.c):
//
//   per image slot and resolution level (2x-subsampled first, then full) — the "PsychoImage", built once per
//   reference, not once per pair:
//     sRGB u8 -> linear (the half-resolution level: 2x2 average, formed in the same kernel) -> blur sigma 1.2 (5-tap,
//     mirrored) -> OpsinDynamicsImage -> XYB                                                          [k_ba_front]
//     -> LF = blur 7.156 ; MF = blur 3.225 of (XYB - LF) ; HF = blur 1.564 of the rest ; UHF = rest, with the range
//        shaping of SeparateFrequencies -> 10 planes; the mask input (DiffPrecompute of HF + UHF) falls out of the HF
//        stage and is blurred with sigma 2.7                                           [k_ba_blur_h<33>, k_ba_blur_v_split]
//   per reference and level: the mask values (fuzzy erosion + the two mask curves)                  [k_ba_mask_vals]
//   per pair and level, ONE kernel:                                                                [k_ba_malta_l2_xy]
//     Malta line filters (UHF, HF, MF; X and Y), asymmetric L2 (HF), L2 (MF), L2 (LF), CombineChannelsToDiffmap; the
//     full-resolution level then forms diffmap = 0.85 * full + 0.5 * upsampled(half) in registers and reduces it
//   score = max ; p-norm = mean of 3-, 6-, 12-norms.                                                    [k_ba_score]
//
// The 33-tap blur is a row kernel + a column kernel; the 15-, 13- and 7-tap blurs run row and column pass in one kernel
// (LDS-tiled, borders re-normalised).  Build with -ffp-contract=off.
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <type_traits>

#include "ba_front_geom.h"
#include "ba_slot_order.h"
#include "ce_internal.h"

namespace {

constexpr int TPB = 256;
constexpr int PSY = 10;  // uhf0 uhf1 hf0 hf1 mf0 mf1 mf2 lf0 lf1 lf2
enum { UHF0 = 0, UHF1, HF0, HF1, MF0, MF1, MF2, LF0, LF1, LF2 };

struct blur_kernel {
    int len;
    float k[40];
    // 1 / (sum of the valid weights) for an output d pixels from the low / high border of a line that is at least
    // `len` long, summed on the host in the order the pixel loop would sum them (low border: taps off-d .. len-1,
    // high border: taps 0 .. off+d)
    float lo[16], hi[16];
};

#define BA_XY                                                           \
    const uint32_t x = blockIdx.x * 64 + (threadIdx.x & 63);            \
    const uint32_t y = blockIdx.y * 4 + (threadIdx.x >> 6);             \
    if (x >= g.w || y >= g.h) return;                                   \
    const size_t o = (size_t)y * g.pitch + x

__device__ __forceinline__ uint32_t slot_of(uint32_t z, uint32_t n_refs_used, uint32_t max_refs)
{
    return z < n_refs_used ? z : max_refs + (z - n_refs_used);
}

// ---- separable blurs ------------------------------------------------------------------------------------
// unit stride `us` planes per unit; planes [first, first+n) of each unit are processed; z = unit * n + k
struct plane_sel {
    uint32_t per_unit, first, n;
};

// Long separable blurs, LDS-tiled with a register window: a thread produces 8 consecutive outputs
// from 8 + LEN - 1 inputs held in registers (5 LDS reads per output at LEN = 33 instead of 33), each
// output summing its taps in ascending order exactly like ConvolutionWithTranspose.  Taps outside the
// image are zero in the tile (x + 0.0f == x, so the sum over the valid taps is unchanged) and border
// outputs are scaled by 1 / (sum of their valid weights).
constexpr int BW_OUT = 8;

// A tap of the long blurs: sum + v * k with the lineage's two roundings (bit-identical planes).  -DCE_BA_BLUR_FMA=1 builds
// the taps as ONE fused multiply-add - the oracle's switch "ba_blur_fma" bit for bit - for A/B runs: measured in round 3
// at +3 % of the headline (the five blur kernels 1.86 -> 1.70 ms per Kodak step) for a score that moves by up to 6e-5
// relative on small shapes (profiles/r03_experiments.md section 3): too close to the 1e-4 contract, not adopted.
#ifndef CE_BA_BLUR_FMA
#define CE_BA_BLUR_FMA 0
#endif
__device__ __forceinline__ float blur_tap(float sum, float v, float k)
{
#if CE_BA_BLUR_FMA
    return __builtin_fmaf(v, k, sum);
#else
    return sum + v * k;
#endif
}

template <int LEN>
__device__ __forceinline__ float border_scale(const blur_kernel &bk, int pos, int n, float inv_wsum)
{
    constexpr int off = LEN / 2;
    if (pos - off >= 0 && pos + off <= n - 1) return inv_wsum;
    if (n >= LEN) {
        // one border only: pick the host-built scale with compile-time indices (a dynamic index into the kernel
        // arguments would be a serialised global load per tap - it used to cost the x-border blocks ~100 us each)
        const int d = pos < off ? pos : n - 1 - pos;
        float s = 0.0f;
#pragma unroll
        for (int i = 0; i < off; i++) s = d == i ? (pos < off ? bk.lo[i] : bk.hi[i]) : s;
        return s;
    }
    float weight = 0.0f;
    for (int j = max(pos - off, 0); j <= min(pos + off, n - 1); j++) weight += bk.k[j - pos + off];
    return 1.0f / weight;
}

// horizontal: block = 8 rows x 256 columns.  The tile starts 16 columns left of the block whatever LEN is, so rows
// load as aligned float4 (72 per row); LDS rows are padded one float per 8 so that lanes reading with a stride of
// 8 floats hit distinct banks.  A thread produces 8 consecutive outputs as 4 PAIRS: its 8+LEN-1 inputs are held
// as even-aligned pairs (v[2i], v[2i+1]) and odd-aligned pairs (v[2i+1], v[2i+2]), so every tap of an output pair
// is one v_pk_mul_f32 + one v_pk_add_f32 (two IEEE multiplies / adds: bit-identical to the scalar tap loop, taps
// still summed in ascending order).
typedef float ba_f2 __attribute__((ext_vector_type(2)));
#ifndef CE_BH_TILES
#define CE_BH_TILES 4
#endif
constexpr int BH_TILES = CE_BH_TILES;  // 8-row tiles per block of the row blur

template <int LEN>
__global__ __launch_bounds__(TPB) void k_ba_blur_h(const float *__restrict__ in, float *__restrict__ out, ce_plane_geom g, plane_sel si,
                                                   plane_sel so, blur_kernel bk, float inv_wsum, uint32_t n_refs_used,
                                                   uint32_t max_refs, int by_slot, ba_slot_grid sg)
{
    const ba_slot_item it = ba_slot_decode3(sg, sg.planes, blockIdx.x, blockIdx.y, blockIdx.z);  // (tile, plane, slot): ba_slot_order.h
    if (!it.live) return;
    constexpr int off = LEN / 2, TW = 256, TR = 8, LEFT = 16, RAW = TW + 2 * LEFT, ROWF = RAW + RAW / 8 + 1, SH = LEFT - off;
    static_assert(off <= LEFT, "tile halo");
    __shared__ float tile[TR * ROWF];
    const uint32_t u = it.z, k = it.plane;
    const uint32_t unit = by_slot ? slot_of(u, n_refs_used, max_refs) : u;
    const float *p = in + ((size_t)unit * si.per_unit + si.first + k) * g.plane;
    const int x0 = it.x * TW;
    // A block walks BH_TILES consecutive 8-row tiles; the next tile's float4 pieces are fetched into registers while
    // the current one is filtered out of LDS.
    constexpr int NF = (TR * (RAW / 4) + TPB - 1) / TPB;
    float4 pf[NF];
    auto fetch = [&](int y0) {
#pragma unroll
        for (int m = 0; m < NF; m++) {
            const int i = m * TPB + (int)threadIdx.x, r = i / (RAW / 4), c = 4 * (i % (RAW / 4)), gx = x0 - LEFT + c, gy = y0 + r;
            float4 v = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            if (r < TR && gx >= 0 && gx < (int)g.pitch && gy < (int)g.h) {  // 16-byte aligned, whole float4 inside the padded row
                v = *reinterpret_cast<const float4 *>(p + (size_t)gy * g.pitch + gx);
                if (gx + 3 >= (int)g.w) {  // the row's padding is not part of the image
                    if (gx + 0 >= (int)g.w) v.x = 0.0f;
                    if (gx + 1 >= (int)g.w) v.y = 0.0f;
                    if (gx + 2 >= (int)g.w) v.z = 0.0f;
                    v.w = 0.0f;
                }
            }
            pf[m] = v;
        }
    };
    const int r = threadIdx.x >> 5, cx = threadIdx.x & 31, gx0 = x0 + 8 * cx;
    // The border scale of a column is the same for every row: each thread forms ONE column's scale (the select chain of
    // border_scale is ~50 instructions) and the block shares the 256 of them through LDS, instead of every thread forming
    // the eight of its own outputs (~700 of the ~3 300 instructions a thread executed per block: profiles/r03_experiments.md 22).
    __shared__ __attribute__((aligned(16))) float s_scale[TW];
    {
        const int gx = x0 + (int)threadIdx.x;
        s_scale[threadIdx.x] = gx < (int)g.w ? border_scale<LEN>(bk, gx, (int)g.w, inv_wsum) : 0.0f;
    }
    constexpr int NV = BW_OUT + LEN - 1, NP = (NV + 1) / 2;
    const float *row = &tile[r * ROWF + 9 * cx];  // element j of the window sits at j + SH + ((j + SH) >> 3)
    auto at = [&](int j) { return row[(j + SH) + ((j + SH) >> 3)]; };
    const int y_first = it.y * (TR * BH_TILES);
    fetch(y_first);
#pragma unroll 1
    for (int t = 0; t < BH_TILES; t++) {
        const int y0 = y_first + t * TR;
        if (y0 >= (int)g.h) break;  // block-uniform
        if (t) __syncthreads();     // the previous tile has been read
#pragma unroll
        for (int m = 0; m < NF; m++) {
            const int i = m * TPB + (int)threadIdx.x, rr = i / (RAW / 4), c = 4 * (i % (RAW / 4));
            if (rr < TR) {
                float *tp = &tile[rr * ROWF + c + (c >> 3)];  // c is a multiple of 4: the four floats stay inside one group of 8
                tp[0] = pf[m].x, tp[1] = pf[m].y, tp[2] = pf[m].z, tp[3] = pf[m].w;
            }
        }
        if (t + 1 < BH_TILES && y0 + TR < (int)g.h) fetch(y0 + TR);
        __syncthreads();
        const int gy = y0 + r;
        if (gy >= (int)g.h || gx0 >= (int)g.w) continue;
        ba_f2 pe[NP], po[NP];
#pragma unroll
        for (int i = 0; i < NP; i++) {
            pe[i] = ba_f2{at(2 * i), 2 * i + 1 < NV ? at(2 * i + 1) : 0.0f};
            po[i] = ba_f2{2 * i + 1 < NV ? at(2 * i + 1) : 0.0f, 2 * i + 2 < NV ? at(2 * i + 2) : 0.0f};
        }
        float *dst = out + ((size_t)unit * so.per_unit + so.first + k) * g.plane + (size_t)gy * g.pitch + gx0;
        float res[BW_OUT];
#pragma unroll
        for (int op = 0; op < BW_OUT / 2; op++) {
            ba_f2 sum = {0.0f, 0.0f};
#pragma unroll
            for (int j = 0; j < LEN; j++) {
                const int idx = 2 * op + j;
                const ba_f2 src = (idx & 1) ? po[idx >> 1] : pe[idx >> 1];
#if CE_BA_BLUR_FMA
                sum = __builtin_elementwise_fma(src, ba_f2{bk.k[j], bk.k[j]}, sum);
#else
                const ba_f2 prod = src * ba_f2{bk.k[j], bk.k[j]};
                sum = sum + prod;
#endif
            }
            res[2 * op] = sum.x * s_scale[8 * cx + 2 * op];  // written before the tile's first barrier
            res[2 * op + 1] = sum.y * s_scale[8 * cx + 2 * op + 1];
        }
        if (gx0 + BW_OUT <= (int)g.w) {  // rows are 128-byte aligned and gx0 is a multiple of 8
            *reinterpret_cast<float4 *>(dst) = make_float4(res[0], res[1], res[2], res[3]);
            *reinterpret_cast<float4 *>(dst + 4) = make_float4(res[4], res[5], res[6], res[7]);
        } else {
#pragma unroll
            for (int o = 0; o < BW_OUT; o++)
                if (gx0 + o < (int)g.w) dst[o] = res[o];
        }
    }
}

// ---- OpsinDynamicsImage (pointwise part) ---------------------------------------------------------------
__device__ __forceinline__ void opsin_absorbance(float in0, float in1, float in2, float &o0, float &o1, float &o2)
{
    const float mixi0 = 0.29956550340058319f, mixi1 = 0.63373087833825936f, mixi2 = 0.077705617820981968f, mixi3 = 1.7557483643287353f;
    const float mixi4 = 0.22158691104574774f, mixi5 = 0.69391388044116142f, mixi6 = 0.0987313588422f, mixi7 = 1.7557483643287353f;
    const float mixi8 = 0.02f, mixi9 = 0.02f, mixi10 = 0.20480129041026129f, mixi11 = 12.226454707163354f;
    o0 = __builtin_fmaf(mixi0, in0, __builtin_fmaf(mixi1, in1, __builtin_fmaf(mixi2, in2, mixi3)));
    o1 = __builtin_fmaf(mixi4, in0, __builtin_fmaf(mixi5, in1, __builtin_fmaf(mixi6, in2, mixi7)));
    o2 = __builtin_fmaf(mixi8, in0, __builtin_fmaf(mixi9, in1, __builtin_fmaf(mixi10, in2, mixi11)));
}

// FastLog2f of the lineage (libjxl lib/jxl/base/fast_math-inl.h): mantissa reduced to [-1/3, 1/3] by integer
// arithmetic on the bits, (2,2) rational polynomial of log2(1 + t) in Horner form with fused multiply-adds, one
// IEEE division.  IEEE basic operations only: bit-identical to oracle/butteraugli.c (a libm log2f is not, and on a
// flat image one ulp of the logarithm moves the score by up to 4e-3 relative).
__device__ __forceinline__ float fast_log2f(float x)
{
    const float p0 = -1.8503833400518310E-06f, p1 = 1.4287160470083755E+00f, p2 = 7.4245873327820566E-01f;
    const float q0 = 9.9032814277590719E-01f, q1 = 1.0096718572241148E+00f, q2 = 1.7409343003366853E-01f;
    const int32_t xb = (int32_t)__float_as_uint(x);
    const int32_t es = (xb - 0x3f2aaaab) >> 23;  // arithmetic shift
    const float m = __uint_as_float((uint32_t)xb - ((uint32_t)es << 23));
    const float t = m - 1.0f;
    const float yp = __builtin_fmaf(__builtin_fmaf(p2, t, p1), t, p0);
    const float yq = __builtin_fmaf(__builtin_fmaf(q2, t, q1), t, q0);
    return ce_div_noscale(yp, yq) + (float)es;  // yq in [0.67, 1.35], |yp| < 0.6 (ce_internal.h: the IEEE quotient, 8 instructions)
}

__device__ __forceinline__ float gamma_f(float v)
{
    const float kRetMul = 19.245013259874995f * 0.693147180559945f, kRetAdd = -23.16046239805755f;
    if (v < 0.0f) v = 0.0f;
    const float biased = v + 9.9710635769299145f;
    return __builtin_fmaf(kRetMul, fast_log2f(biased), kRetAdd);
}

// Front end, fused: linear RGB tile (level 0: sRGB u8 through the table; level 1: the subsampled planes) with a
// 2-pixel halo in LDS -> the 5-tap sigma-1.2 blur (mirrored at the image border, both passes in LDS) ->
// OpsinDynamicsImage -> XYB planes.  Only XYB is written (12 B/px); nothing else of this stage touches HBM.
constexpr int FT = 32, FR = FT + 4;
// HALF: the half-resolution level - its linear RGB is the 2x2 average of the full-resolution image's (Subsample2x: the
// four quarter-weighted samples added in row-major order, the last odd row / column doubled), formed here from the u8
// source instead of in a pass of its own; gi = the full-resolution geometry.
// T: the sample type - uint8_t (the 256-entry table in LDS, packed loads wherever a group of pixels lies inside its row) or
// the uint16_t of a deep batch (2^depth entries per side in global memory, lut for the references and lut_test for the
// distorted images; every cell takes the per-sample loads) or the float of a linear batch (the sample
// is the linear value: no table, the same per-sample loads).
// Every tile runs the same two blur passes with plain indices: a tile that touches the image's edge first writes the
// mirrored values into the out-of-image cells of its region (ba_front_geom.h), once, instead of mirroring at every tap.
template <typename T>
__device__ __forceinline__ float ba_linear_of(const float *tab, T v) { return tab[v]; }
template <>
__device__ __forceinline__ float ba_linear_of<float>(const float *, float v) { return v; }

template <bool HALF, typename T>
__global__ __launch_bounds__(TPB) void k_ba_front(const uint8_t *__restrict__ refs, const uint8_t *__restrict__ tests,
                                                  const float *__restrict__ lut, const float *__restrict__ lut_test, ce_plane_geom gi,
                                                  float *__restrict__ xyb, ce_plane_geom g, float w0, float w1, float w2,
                                                  float intensity_target, size_t img_bytes, uint32_t n_refs_used, uint32_t max_refs,
                                                  ba_slot_grid sg)
{
    const ba_slot_item it = ba_slot_decode3(sg, 1, blockIdx.x, blockIdx.y, blockIdx.z);  // (tile, slot): ba_slot_order.h
    if (!it.live) return;
    __shared__ float L[3][FR * FR];   // linear, region = tile + 2
    __shared__ float H[3][FR * FT];   // row-blurred: FR rows x FT columns
    constexpr bool U8 = sizeof(T) == 1;
    __shared__ float s_lut[256];
    if (U8) s_lut[threadIdx.x] = lut[threadIdx.x];
    const uint32_t z = it.z, slot = slot_of(z, n_refs_used, max_refs);
    const int w = (int)g.w, h = (int)g.h, x0 = it.x * FT, y0 = it.y * FT, gx0 = x0 - 2, gy0 = y0 - 2;
    const uint8_t *src8 = z < n_refs_used ? refs + (size_t)z * img_bytes : tests + (size_t)(z - n_refs_used) * img_bytes;
    const T *srcT = reinterpret_cast<const T *>(src8);
    const float *tab = U8 ? s_lut : (z < n_refs_used ? lut : lut_test);
    const int W8 = HALF ? (int)gi.w : w, H8 = HALF ? (int)gi.h : h;  // the u8 image
    __syncthreads();
    // block-uniform: the whole 36x36 region lies inside the image, so there is no rim to fill
    const bool interior = gx0 >= 0 && gy0 >= 0 && gx0 + FR <= w && gy0 + FR <= h;
    const uint32_t mis = (uint32_t)(reinterpret_cast<uintptr_t>(src8) & 3);
    // four u8 pixels (12 bytes, any alignment) from four aligned dwords
    auto load12 = [&](const uint8_t *p, uint32_t &v0, uint32_t &v1, uint32_t &v2) {
        const uintptr_t a = reinterpret_cast<uintptr_t>(p);
        const uint32_t *q = reinterpret_cast<const uint32_t *>(a & ~(uintptr_t)3);
        const uint32_t d0 = q[0], d1 = q[1], d2 = q[2], d3 = q[3], sh = (uint32_t)(a & 3);
        v0 = __builtin_amdgcn_alignbyte(d1, d0, sh), v1 = __builtin_amdgcn_alignbyte(d2, d1, sh), v2 = __builtin_amdgcn_alignbyte(d3, d2, sh);
    };
    // the per-element route: one region cell, sample by sample; a cell outside the image loads nothing
    auto load_cell = [&](int lx, int ly) {
        const int i = ly * FR + lx, X = gx0 + lx, Y = gy0 + ly;
        if (X >= 0 && X < w && Y >= 0 && Y < h) {
            if (!HALF) {
                const T *px = srcT + ((size_t)Y * w + X) * 3;
                L[0][i] = ba_linear_of<T>(tab, px[0]);
                L[1][i] = ba_linear_of<T>(tab, px[1]);
                L[2][i] = ba_linear_of<T>(tab, px[2]);
            } else {
                float acc[3] = {0.0f, 0.0f, 0.0f};
#pragma unroll
                for (int dy = 0; dy < 2; dy++)
#pragma unroll
                    for (int dx = 0; dx < 2; dx++) {
                        const int ix = 2 * X + dx, iy = 2 * Y + dy;
                        if (ix < W8 && iy < H8) {
                            const T *px = srcT + ((size_t)iy * W8 + ix) * 3;
#pragma unroll
                            for (int c = 0; c < 3; c++) acc[c] += 0.25f * ba_linear_of<T>(tab, px[c]);
                        }
                    }
#pragma unroll
                for (int c = 0; c < 3; c++) {
                    float v = acc[c];
                    if ((W8 & 1) && X == w - 1) v *= 2.0f;
                    if ((H8 & 1) && Y == h - 1) v *= 2.0f;
                    L[c][i] = v;
                }
            }
        }
    };
    // Load phase (ba_front_geom.h): a u8 task takes the packed route wherever its row is inside the image and its group inside
    // the row, on every tile; only the groups across the left or right edge go element by element
    if (U8 && !HALF) {
        // four pixels per task; nine tasks per row of the region
        auto packed4 = [&](int lx, int ly) {
            uint32_t v0, v1, v2;
            load12(src8 + ((size_t)(gy0 + ly) * w + gx0 + lx) * 3, v0, v1, v2);
            const int o = ly * FR + lx;
            L[0][o] = s_lut[v0 & 255u], L[1][o] = s_lut[(v0 >> 8) & 255u], L[2][o] = s_lut[(v0 >> 16) & 255u];
            L[0][o + 1] = s_lut[v0 >> 24], L[1][o + 1] = s_lut[v1 & 255u], L[2][o + 1] = s_lut[(v1 >> 8) & 255u];
            L[0][o + 2] = s_lut[(v1 >> 16) & 255u], L[1][o + 2] = s_lut[v1 >> 24], L[2][o + 2] = s_lut[v2 & 255u];
            L[0][o + 3] = s_lut[(v2 >> 8) & 255u], L[1][o + 3] = s_lut[(v2 >> 16) & 255u], L[2][o + 3] = s_lut[v2 >> 24];
        };
        if (ba_front_all_fast4(gx0, gy0, w, h, mis)) {  // block-uniform
            for (int i = threadIdx.x; i < FR * ba_front_groups4; i += TPB) packed4(4 * (i % ba_front_groups4), i / ba_front_groups4);
        } else {
            const int shift = ba_front_shift4(gx0, w);
            for (int i = threadIdx.x; i < FR * ba_front_groups4; i += TPB) {
                const int g = i % ba_front_groups4, ly = i / ba_front_groups4, lx = ba_front_group4_cell(g, 0, shift);
                if (ba_front_group4_contiguous(g, shift) && ba_front_fast4(gx0 + lx, gy0 + ly, w, h, mis))
                    packed4(lx, ly);
                else
                    for (int k = 0; k < 4; k++) load_cell(ba_front_group4_cell(g, k, shift), ly);
            }
        }
    } else if (U8 && HALF) {
        // two half-resolution elements (2 x 4 u8 pixels) per task: ((0 + q00) + q01) + q10) + q11, q = 0.25 * linear
        auto packed2 = [&](int lx, int ly) {
            uint32_t a0, a1, a2, b0, b1, b2;
            const uint8_t *p = src8 + ((size_t)(2 * (gy0 + ly)) * W8 + 2 * (gx0 + lx)) * 3;
            load12(p, a0, a1, a2);
            load12(p + (size_t)W8 * 3, b0, b1, b2);
            const int o = ly * FR + lx;
            // row pixels: p0 = (v0.b0, v0.b1, v0.b2), p1 = (v0.b3, v1.b0, v1.b1), p2 = (v1.b2, v1.b3, v2.b0), p3 = (v2.b1, v2.b2, v2.b3)
#define CE_Q(v) (0.25f * s_lut[(v)])
            L[0][o] = ((0.0f + CE_Q(a0 & 255u)) + CE_Q(a0 >> 24)) + CE_Q(b0 & 255u) + CE_Q(b0 >> 24);
            L[1][o] = ((0.0f + CE_Q((a0 >> 8) & 255u)) + CE_Q(a1 & 255u)) + CE_Q((b0 >> 8) & 255u) + CE_Q(b1 & 255u);
            L[2][o] = ((0.0f + CE_Q((a0 >> 16) & 255u)) + CE_Q((a1 >> 8) & 255u)) + CE_Q((b0 >> 16) & 255u) + CE_Q((b1 >> 8) & 255u);
            L[0][o + 1] = ((0.0f + CE_Q((a1 >> 16) & 255u)) + CE_Q((a2 >> 8) & 255u)) + CE_Q((b1 >> 16) & 255u) + CE_Q((b2 >> 8) & 255u);
            L[1][o + 1] = ((0.0f + CE_Q(a1 >> 24)) + CE_Q((a2 >> 16) & 255u)) + CE_Q(b1 >> 24) + CE_Q((b2 >> 16) & 255u);
            L[2][o + 1] = ((0.0f + CE_Q(a2 & 255u)) + CE_Q(a2 >> 24)) + CE_Q(b2 & 255u) + CE_Q(b2 >> 24);
#undef CE_Q
        };
        if (ba_front_all_fast2_half(gx0, gy0, W8, H8, mis)) {  // block-uniform
            for (int i = threadIdx.x; i < FR * ba_front_groups2; i += TPB) packed2(2 * (i % ba_front_groups2), i / ba_front_groups2);
        } else {
            for (int i = threadIdx.x; i < FR * ba_front_groups2; i += TPB) {
                int lx, ly;
                ba_front_task2(i, lx, ly);
                if (ba_front_fast2_half(gx0 + lx, gy0 + ly, W8, H8, mis)) {
                    packed2(lx, ly);
                } else {
                    load_cell(lx, ly);
                    load_cell(lx + 1, ly);
                }
            }
        }
    } else {
        for (int i = threadIdx.x; i < FR * FR; i += TPB) load_cell(i % FR, i / FR);
    }
    __syncthreads();
    // Rim fill, edge tiles only: every out-of-image cell a tap can reach takes the value of the cell the blur's mirroring
    // names (an in-image cell: written before the barrier above, read-only here), every other out-of-image cell is zeroed.
    // The out-of-image columns first, then the out-of-image rows over the in-image columns: few cells, each visited once
    if (!interior) {
        auto fill = [&](int lx, int ly) {
            const int i = ly * FR + lx;
            int src = 0;
            if (ba_front_rim(gx0 + lx, gy0 + ly, w, h, gx0, gy0, src) == BA_RIM_COPY)
                L[0][i] = L[0][src], L[1][i] = L[1][src], L[2][i] = L[2][src];
            else
                L[0][i] = 0.0f, L[1][i] = 0.0f, L[2][i] = 0.0f;
        };
        const int xlo = ba_front_out_lo(gx0), xhi = ba_front_out_hi(gx0, w), ylo = ba_front_out_lo(gy0), yhi = ba_front_out_hi(gy0, h);
        for (int t = threadIdx.x; t < (xlo + FR - xhi) * FR; t += TPB) fill(ba_front_out_line(t / FR, xlo, xhi), t % FR);
        for (int t = threadIdx.x; t < (ylo + FR - yhi) * FR; t += TPB) {
            const int lx = t % FR;
            if (lx >= xlo && lx < xhi) fill(lx, ba_front_out_line(t / FR, ylo, yhi));
        }
        __syncthreads();
    }
    // Row pass on every row of the region, tile columns only, with plain indices: a rim row holds its mirror source's cells,
    // so its H row is that row's, from the same inputs and the same expression.  Columns right of the image blur zeros and
    // are not stored.
    for (int i = threadIdx.x; i < FR * FT; i += TPB) {
        const int tx = i % FT, ly = i / FT, c0 = tx + 2;
#pragma unroll
        for (int c = 0; c < 3; c++) {
            const float *r = &L[c][ly * FR];
            H[c][i] = r[c0] * w0 + (r[c0 - 1] + r[c0 + 1]) * w1 + (r[c0 - 2] + r[c0 + 2]) * w2;
        }
    }
    __syncthreads();
    for (int i = threadIdx.x; i < FT * FT; i += TPB) {
        const int tx = i % FT, ty = i / FT, X = x0 + tx, Y = y0 + ty;
        if (X >= w || Y >= h) continue;
        const int r0 = ty + 2;
        float bl[3], ln[3];
#pragma unroll
        for (int c = 0; c < 3; c++) {
            const float *col = &H[c][tx];
            bl[c] = col[r0 * FT] * w0 + (col[(r0 - 1) * FT] + col[(r0 + 1) * FT]) * w1 + (col[(r0 - 2) * FT] + col[(r0 + 2) * FT]) * w2;
            ln[c] = L[c][(ty + 2) * FR + tx + 2];
        }
        const float mn = 1e-4f;
        float p0, p1v, p2v;
        opsin_absorbance(bl[0] * intensity_target, bl[1] * intensity_target, bl[2] * intensity_target, p0, p1v, p2v);
        p0 = p0 > mn ? p0 : mn;
        p1v = p1v > mn ? p1v : mn;
        p2v = p2v > mn ? p2v : mn;
        // IEEE quotients without the range-scaling steps (ce_internal.h).  Measured ("Operand
        // ranges"): RGB8 / deep batches p in [1.76, 7.2e3] (the opsin bias keeps p off its clamp), gamma in [24, 148];
        // linear batches p in [1e-4 (the clamp above), 1.04e7], gamma in [21, 288], quotients in [2.8e-5, 2.1e5]
        float s0 = ce_div_noscale(gamma_f(p0), p0), s1 = ce_div_noscale(gamma_f(p1v), p1v), s2 = ce_div_noscale(gamma_f(p2v), p2v);
        s0 = s0 > mn ? s0 : mn;
        s1 = s1 > mn ? s1 : mn;
        s2 = s2 > mn ? s2 : mn;
        float c0, c1, c2;
        opsin_absorbance(ln[0] * intensity_target, ln[1] * intensity_target, ln[2] * intensity_target, c0, c1, c2);
        c0 *= s0;
        c1 *= s1;
        c2 *= s2;
        const float min01 = 1.7557483643287353f, min2 = 12.226454707163354f;
        c0 = c0 > min01 ? c0 : min01;
        c1 = c1 > min01 ? c1 : min01;
        c2 = c2 > min2 ? c2 : min2;
        const size_t o = (size_t)slot * 3 * g.plane + (size_t)Y * g.pitch + X;
        xyb[o] = c0 - c1;
        xyb[o + g.plane] = c0 + c1;
        xyb[o + 2 * g.plane] = c2;
    }
}

// ---- SeparateFrequencies pointwise stages ------------------------------------------------------------------
__device__ __forceinline__ float remove_range(float w, float x) { return x > w ? x - w : (x < -w ? x + w : 0.0f); }
__device__ __forceinline__ float amplify_range(float w, float x) { return x > w ? x + w : (x < -w ? x - w : x + x); }
__device__ __forceinline__ float maximum_clamp(float v, float maxval)
{
    const float kMul = 0.724216145665f;
    if (v >= maxval) return __builtin_fmaf(v - maxval, kMul, maxval);
    if (v < -maxval) return __builtin_fmaf(v + maxval, kMul, -maxval);
    return v;
}

// ---- column blur of all planes of one image slot + the pointwise stage that consumes them, fused ---------------
// SeparateFrequencies alternates a blur with a pointwise split; as separate kernels every split re-reads the blur's
// output and the band it splits.  Here a block blurs the NP planes of its 64 x 32 tile one after the other (same
// LDS tile, results kept in registers) and then runs the split on registers, reading only the raw band:
//   EPI_LF (3 planes, sigma 7.156): lf = blur(xyb);  mf_raw = xyb - lf -> psy MF;  XybLowFreqToVals(lf) -> psy LF
//   EPI_MF (3 planes, sigma 3.225): mf = blur(mf_raw);  hf_raw = mf_raw - mf (X suppressed by Y) -> psy HF;
//                                   range-shaped mf -> psy MF
//   EPI_HF (2 planes, sigma 1.564): hf = blur(hf_raw);  uhf = hf_raw - hf, clamps / ranges -> psy UHF, HF
// Arithmetic per element is exactly that of k_ba_blur_v followed by the old pointwise kernels.
//
// HV (the MF and HF stages, 15 and 7 taps): the ROW blur runs in the same kernel - the raw band's tile (64 + LEN - 1 rows,
// 64 + 16 columns, zero outside the image) is staged in LDS, every tile row is filtered into the column pass's tile
// (taps in ascending order, border scale of k_ba_blur_h: the same sums), so the row-blurred planes never travel through
// HBM.  A fused stage reads its raw band with a halo, so no stage may overwrite its own input: the raw bands live in
// scratch planes (`aux`): LF stage -> raw MF -> aux_out;  MF stage: aux_in -> MF (psy), raw HF -> aux_out;  HF stage:
// aux_in -> HF, UHF (psy), mask input.  (The 33-tap LF stage keeps its separate row pass: its halo would be half a tile.)
//   EPI_MASK (1 plane per slot, sigma 2.7, HV): the mask input's blur, no pointwise stage: tmp[slot] -> aux_out[slot]
//   EPI_LF_TERM: EPI_LF for a launch whose references' state is kept (ce_plan.h: ce_plan_ba_lf_term_in_blur).  A distorted
//     slot's psy LF has one reader, the LF term of CombineChannelsToDiffmap in Malta's epilogue, and that term's other operands -
//     the reference's psy LF and dc_maskval - are in place before the launch: the term is formed here, on the registers that
//     hold the distorted LF, with the epilogue's expressions in its order (the same float), and stored to the slot's LF0 plane;
//     LF1 and LF2 of a distorted slot are not written.  Such a launch skips the reference slots (their state is kept), so
//     every slot the instance sees is a distorted one.
enum { EPI_LF = 0, EPI_MF = 1, EPI_HF = 2, EPI_MASK = 3, EPI_LF_TERM = 4 };

// SetL2Diff's weights of the three LF channels (wmul[6 .. 8] of the Malta kernel)
__device__ constexpr float BA_LF_WMUL[3] = {29.2353797994f, 0.844626970982f, 0.703646627719f};

// MaskPsychoImage's input at one pixel: DiffPrecompute of (UHF + HF) of X and Y (pointwise on the FINAL band values)
__device__ __forceinline__ float mask_pre_one(float uhf0, float hf0, float uhf1, float hf1)
{
    const float muls[3] = {2.5f, 0.4f, 0.4f};
    const float xdiff = (uhf0 + hf0) * muls[0];
    const float ydiff = uhf1 * muls[1] + hf1 * muls[2];
    const float m = sqrtf(xdiff * xdiff + ydiff * ydiff);
    const float kMul = 6.19424080439f, kBias = 12.61050594197f;
    const float bias = kMul * kBias;
    const float sqrt_bias = sqrtf(bias);
    return sqrtf(kMul * fabsf(m) + bias) - sqrt_bias;
}

template <int LEN, int EPI, bool HV, int TR>
__global__ __launch_bounds__(TPB) void k_ba_blur_v_split(const float *__restrict__ tmp, const float *__restrict__ xyb,
                                                         float *__restrict__ psy, ce_plane_geom g, blur_kernel bk, float inv_wsum,
                                                         uint32_t n_refs_used, uint32_t max_refs, ba_slot_grid sg,
                                                         float *__restrict__ mask_in, float *__restrict__ aux_out,
                                                         const uint32_t *__restrict__ pair_ref, const float *__restrict__ ref_psy,
                                                         const float *__restrict__ mask_vals, const uint2 *__restrict__ lf_work)
{
    // (pair_ref, ref_psy, mask_vals, lf_work: EPI_LF_TERM only.  ref_psy is psy again, for the references' planes, which this
    // launch only reads: through a pointer of their own the loads need not wait for the stores of the pixel before.)
    // (tile, slot): ba_slot_order.h - or, lf_work given, a 1-D launch over that list (ce_plan_xcd_list with one key per tile
    // column: tile = row | column << 16, pair), which keeps a column's tiles of all pairs of one reference on one XCD - a tile
    // is followed by the same tile of the reference's other pairs, whose L2 then serves the reference's lines to all of them,
    // and by the tile below, which shares its halo rows
    auto decode = [&]() {
        if (EPI == EPI_LF_TERM && lf_work) {
            const uint2 wi = lf_work[blockIdx.x];
            return ba_slot_item{wi.x >> 16, wi.x & 0xffffu, 0, n_refs_used + wi.y, wi.x != ~0u};
        }
        return ba_slot_decode3(sg, 1, blockIdx.x, blockIdx.y, blockIdx.z);
    };
    const ba_slot_item it = decode();
    if (!it.live) return;
    constexpr int NP = EPI == EPI_HF ? 2 : EPI == EPI_MASK ? 1 : 3;
    // 64 columns x 64 rows per block (two 8-row groups per thread): the halo of LEN - 1 rows is read once per 64 rows
    constexpr int off = LEN / 2, TW = 64, PARTS = TR / 32, RAW = TR + LEN - 1;
    static_assert(TR % 32 == 0, "four waves x 8 rows per part");
    // HV: the staged input is 4 or 8 columns wider on each side (>= off, and its rows load as aligned float4)
    constexpr int LEFT = off <= 4 ? 4 : 8, IW = HV ? TW + 2 * LEFT : TW;
    static_assert(!HV || off <= LEFT, "row-pass halo");
    __shared__ __attribute__((aligned(16))) float tile[RAW * TW];
    __shared__ __attribute__((aligned(16))) float in_t[HV ? RAW * IW : 4];
    const uint32_t slot = slot_of(it.z, n_refs_used, max_refs);
    const int x0 = it.x * TW, y0 = it.y * TR;
    const int c = threadIdx.x & 63, wv = threadIdx.x >> 6, gx = x0 + c;
    const bool col_live = gx < (int)g.w;
    float res[NP][PARTS][BW_OUT];
    // The (input) tile of plane q+1 is fetched (aligned float4 pieces of the rows, zero outside the image) into registers
    // while plane q is filtered: NF float4 per thread.
    constexpr int NF = (RAW * (IW / 4) + TPB - 1) / TPB;
    float4 pf[NF];
    auto fetch = [&](int q) {
        // the row-blurred planes (HV: the raw band) of this slot; the mask input is one plane per slot
        const float *p = tmp + (EPI == EPI_MASK ? (size_t)slot : (size_t)slot * 3 + q) * g.plane;
#pragma unroll
        for (int m = 0; m < NF; m++) {
            const int i = m * TPB + (int)threadIdx.x, r = i / (IW / 4), X = x0 - (HV ? LEFT : 0) + 4 * (i % (IW / 4)), Y = y0 - off + r;
            float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
            if (r < RAW && Y >= 0 && Y < (int)g.h && X >= 0 && X < (int)g.pitch) v = *reinterpret_cast<const float4 *>(p + (size_t)Y * g.pitch + X);
            v.x = X < (int)g.w ? v.x : 0.0f;
            v.y = X + 1 < (int)g.w ? v.y : 0.0f;
            v.z = X + 2 < (int)g.w ? v.z : 0.0f;
            v.w = X + 3 < (int)g.w ? v.w : 0.0f;
            pf[m] = v;
        }
    };
    auto stash = [&]() {  // the fetched pieces -> LDS (HV: the input tile, else the column pass's tile)
#pragma unroll
        for (int m = 0; m < NF; m++) {
            const int i = m * TPB + (int)threadIdx.x;
            if (i < RAW * (IW / 4)) *reinterpret_cast<float4 *>((HV ? in_t : tile) + 4 * i) = pf[m];
        }
    };
    // HV row pass: a thread filters four adjacent columns of a row from one aligned window of the input tile (NW float4 LDS
    // reads for four outputs); its column group is the same in every row it visits (TPB is a multiple of TW / 4)
    constexpr int S0 = LEFT - off, NW = (S0 + 3 + LEN + 3) / 4;
    const int rc4 = 4 * ((int)threadIdx.x % (TW / 4));
    // the row pass's border scale of a column: one thread per column forms it, the block shares the 64 through LDS (k_ba_blur_h)
    __shared__ __attribute__((aligned(16))) float s_sx[HV ? TW : 4];
    if (HV && threadIdx.x < TW)
        s_sx[threadIdx.x] = x0 + (int)threadIdx.x < (int)g.w ? border_scale<LEN>(bk, x0 + (int)threadIdx.x, (int)g.w, inv_wsum) : 0.0f;
    float scale_x[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    fetch(0);
    if (HV) {
        stash();
        __syncthreads();
#pragma unroll
        for (int k = 0; k < 4; k++) scale_x[k] = s_sx[rc4 + k];
    }
#pragma unroll
    for (int q = 0; q < NP; q++) {
        if (HV) {
            // row pass of every tile row: taps in ascending order, zero outside the image (x + 0.0f == x), border scale
#pragma unroll 1
            for (int u = threadIdx.x; u < RAW * (TW / 4); u += TPB) {
                const int r = u / (TW / 4);
                const float4 *src = reinterpret_cast<const float4 *>(in_t + r * IW + rc4);
                float wnd[4 * NW];
#pragma unroll
                for (int m = 0; m < NW; m++) {
                    const float4 v = src[m];
                    wnd[4 * m] = v.x, wnd[4 * m + 1] = v.y, wnd[4 * m + 2] = v.z, wnd[4 * m + 3] = v.w;
                }
                float out[4];
#pragma unroll
                for (int k = 0; k < 4; k++) {
                    float sum = 0.0f;
#pragma unroll
                    for (int j = 0; j < LEN; j++) sum = blur_tap(sum, wnd[S0 + k + j], bk.k[j]);
                    out[k] = sum * scale_x[k];  // scale 0 right of the image: the column pass sees zeros there
                }
                *reinterpret_cast<float4 *>(tile + r * TW + rc4) = make_float4(out[0], out[1], out[2], out[3]);
            }
            __syncthreads();  // the tile is complete; the input tile may be overwritten
            if (q + 1 < NP) fetch(q + 1);
        } else {
            if (q) __syncthreads();
            stash();
            if (q + 1 < NP) fetch(q + 1);
            __syncthreads();
        }
#pragma unroll
        for (int part = 0; part < PARTS; part++) {
            const int ly = 32 * part + 8 * wv, gy0 = y0 + ly;
            if (col_live && gy0 < (int)g.h) {
                float v[BW_OUT + LEN - 1];
#pragma unroll
                for (int j = 0; j < BW_OUT + LEN - 1; j++) v[j] = tile[(ly + j) * TW + c];
#pragma unroll
                for (int o = 0; o < BW_OUT; o++) {
                    float sum = 0.0f;
#pragma unroll
                    for (int j = 0; j < LEN; j++) sum = blur_tap(sum, v[o + j], bk.k[j]);
                    res[q][part][o] = sum * border_scale<LEN>(bk, gy0 + o, (int)g.h, inv_wsum);
                }
            }
        }
        if (HV && q + 1 < NP) {
            stash();
            __syncthreads();  // the next input tile is complete; this plane's tile has been read
        }
    }
    if (!col_live) return;
    const size_t pl = g.plane;
    if constexpr (EPI == EPI_LF_TERM) {
        // Every slot of such a launch is a distorted one: pair it.z - n_refs_used, whose reference is the same for the whole
        // block.  Two rows at a time: their 14 loads (raw XYB, the reference's LF, dc_maskval) are requested together, from
        // addresses that no branch guards - a row past the image reads the last row instead and stores nothing.  (Behind a
        // branch per row the kernel made two dependent round trips for every row and lost 0.87 ms per step; four rows at a
        // time take 113 VGPRs and the fifth block of a CU: profiles/r09_ba_lf_term.md.)
        const size_t rslot = (uint32_t)__builtin_amdgcn_readfirstlane((int)pair_ref[it.z - n_refs_used]);
        const float *xs = xyb + (size_t)slot * 3 * pl + gx, *a = ref_psy + (rslot * PSY + LF0) * pl + gx;
        const float *dcm = mask_vals + (rslot * 2 + 1) * pl + gx;
        float *raw = aux_out + (size_t)slot * 3 * pl + gx, *term = psy + ((size_t)slot * PSY + LF0) * pl + gx;
        constexpr int ROWS = 2;
#pragma unroll
        for (int part = 0; part < PARTS; part++) {
            const int gy0 = y0 + 32 * part + 8 * wv;
            if (gy0 >= (int)g.h) break;
#pragma unroll
            for (int o0 = 0; o0 < BW_OUT; o0 += ROWS) {
                float vx[ROWS][3], va[ROWS][3], vm[ROWS];
#pragma unroll
                for (int k = 0; k < ROWS; k++) {
                    const size_t px = (size_t)min(gy0 + o0 + k, (int)g.h - 1) * g.pitch;
#pragma unroll
                    for (int c = 0; c < 3; c++) vx[k][c] = xs[c * pl + px], va[k][c] = a[c * pl + px];
                    vm[k] = dcm[px];
                }
                // (the empty asm keeps the compiler from moving each row's loads down to the row's stores, behind its branch)
#pragma unroll
                for (int k = 0; k < ROWS; k++) {
#pragma unroll
                    for (int c = 0; c < 3; c++) asm volatile("" : "+v"(vx[k][c]), "+v"(va[k][c]));
                    asm volatile("" : "+v"(vm[k]));
                }
#pragma unroll
                for (int k = 0; k < ROWS; k++) {
                    const int o = o0 + k;
                    if (gy0 + o >= (int)g.h) break;
                    const size_t px = (size_t)(gy0 + o) * g.pitch;
                    const float lx = res[0][part][o], ly = res[1][part][o], lb = res[2][part][o];
                    raw[px] = vx[k][0] - lx;  // raw MF, as EPI_LF
                    raw[px + pl] = vx[k][1] - ly;
                    raw[px + 2 * pl] = vx[k][2] - lb;
                    // XybLowFreqToVals, as EPI_LF
                    const float xmul = 33.832837186260f, ymul = 14.458268100570f, bmul = 49.87984651440f, y_to_b_mul = -0.362267051518f;
                    const float bb = __builtin_fmaf(y_to_b_mul, ly, lb);
                    const float lf[3] = {lx * xmul, ly * ymul, bb * bmul};
                    // the LF term of Malta's epilogue (k_ba_malta_l2_xy: dcv, mc_dc), expression for expression
                    float dcv[3];
#pragma unroll
                    for (int c = 0; c < 3; c++) {
                        const float diff = va[k][c] - lf[c];
                        dcv[c] = (diff * diff) * BA_LF_WMUL[c];
                    }
                    const float dc_maskval = vm[k];
                    float dc0 = dcv[0], dc1 = dcv[1], dc2 = dcv[2];
                    const float one = 1.0f;
                    dc0 *= one;
                    term[px] = dc0 * dc_maskval + dc1 * dc_maskval + dc2 * dc_maskval;
                }
            }
        }
        return;
    }
#pragma unroll
    for (int part = 0; part < PARTS; part++) {
        const int gy0 = y0 + 32 * part + 8 * wv;
        if (gy0 >= (int)g.h) break;
        float *ps = psy + (size_t)slot * PSY * g.plane + (size_t)gy0 * g.pitch + gx;
#pragma unroll
        for (int o = 0; o < BW_OUT; o++) {
            if (gy0 + o >= (int)g.h) break;
            float *q = ps + (size_t)o * g.pitch;
            // this pixel in the 3-plane scratch sets (raw bands in / out)
            const size_t ao = (size_t)slot * 3 * pl + (size_t)(gy0 + o) * g.pitch + gx;
            if (EPI == EPI_LF) {
                const float *xs = xyb + (size_t)slot * 3 * pl + (size_t)(gy0 + o) * g.pitch + gx;
                const float lx = res[0][part][o], ly = res[1][part][o], lb = res[2][part][o];
                aux_out[ao] = xs[0] - lx;  // raw MF: the MF stage reads it with a halo, so it cannot live where MF is written
                aux_out[ao + pl] = xs[pl] - ly;
                aux_out[ao + 2 * pl] = xs[2 * pl] - lb;
                // XybLowFreqToVals
                const float xmul = 33.832837186260f, ymul = 14.458268100570f, bmul = 49.87984651440f, y_to_b_mul = -0.362267051518f;
                const float bb = __builtin_fmaf(y_to_b_mul, ly, lb);
                q[LF2 * pl] = bb * bmul;
                q[LF0 * pl] = lx * xmul;
                q[LF1 * pl] = ly * ymul;
            } else if (EPI == EPI_MF) {
                const float kRemoveMfRange = 0.29f, kAddMfRange = 0.1f;
                const float mf0 = res[0][part][o], mf1 = res[1][part][o];
                const float hf0 = tmp[ao] - mf0, hf1 = tmp[ao + pl] - mf1;
                q[MF0 * pl] = remove_range(kRemoveMfRange, mf0);
                q[MF1 * pl] = amplify_range(kAddMfRange, mf1);
                q[MF2 * pl] = res[2][part][o];
                // SuppressXByY(hf[1], &hf[0])
                const float suppress = 46.0f, sv = 0.653020556257f, one_minus_s = 1.0f - 0.653020556257f;
                const float scaler = __builtin_fmaf(suppress / __builtin_fmaf(hf1, hf1, suppress), one_minus_s, sv);
                aux_out[ao] = scaler * hf0;  // raw HF, for the HF stage
                aux_out[ao + pl] = hf1;
            } else if (EPI == EPI_MASK) {
                aux_out[(size_t)slot * pl + (size_t)(gy0 + o) * g.pitch + gx] = res[0][part][o];
            } else {
                const float kRemoveHfRange = 1.5f, kAddHfRange = 0.132f, kRemoveUhfRange = 0.04f;
                const float kMaxclampHf = 28.4691806922f, kMaxclampUhf = 5.19175294647f, kMulYHf = 2.155f, kMulYUhf = 2.69313763794f;
                float hf0_out, uhf0_out, hf1_out, uhf1_out;
                {
                    const float hf = res[0][part][o];
                    const float uhf = tmp[ao] - hf;
                    hf0_out = remove_range(kRemoveHfRange, hf);
                    uhf0_out = remove_range(kRemoveUhfRange, uhf);
                    q[HF0 * pl] = hf0_out;
                    q[UHF0 * pl] = uhf0_out;
                }
                {
                    float hf = maximum_clamp(res[1][part][o], kMaxclampHf);
                    float uhf = tmp[ao + pl] - hf;
                    uhf = maximum_clamp(uhf, kMaxclampUhf);
                    uhf *= kMulYUhf;
                    uhf1_out = uhf;
                    q[UHF1 * pl] = uhf;
                    hf *= kMulYHf;
                    hf1_out = amplify_range(kAddHfRange, hf);
                    q[HF1 * pl] = hf1_out;
                }
                // the four band values are final here: the mask input of this pixel (one plane per image slot) costs no
                // extra pass over the PsychoImage
                mask_in[(size_t)slot * pl + (size_t)(gy0 + o) * g.pitch + gx] = mask_pre_one(uhf0_out, hf0_out, uhf1_out, hf1_out);
            }
        }
    }
}

// ---- per pair: Malta ----------------------------------------------------------------------------------------
struct malta_params {
    float norm2_0gt1, norm2_0lt1, norm1;
};

struct mline {
    int n;
    signed char d[9][2];
};

__device__ constexpr mline MALTA_HF[16] = {
    {9, {{-4, 0}, {-3, 0}, {-2, 0}, {-1, 0}, {0, 0}, {1, 0}, {2, 0}, {3, 0}, {4, 0}}},
    {9, {{0, -4}, {0, -3}, {0, -2}, {0, -1}, {0, 0}, {0, 1}, {0, 2}, {0, 3}, {0, 4}}},
    {7, {{-3, -3}, {-2, -2}, {-1, -1}, {0, 0}, {1, 1}, {2, 2}, {3, 3}}},
    {7, {{3, -3}, {2, -2}, {1, -1}, {0, 0}, {-1, 1}, {-2, 2}, {-3, 3}}},
    {9, {{1, -4}, {1, -3}, {1, -2}, {0, -1}, {0, 0}, {0, 1}, {-1, 2}, {-1, 3}, {-1, 4}}},
    {9, {{-1, -4}, {-1, -3}, {-1, -2}, {0, -1}, {0, 0}, {0, 1}, {1, 2}, {1, 3}, {1, 4}}},
    {9, {{-4, -1}, {-3, -1}, {-2, -1}, {-1, 0}, {0, 0}, {1, 0}, {2, 1}, {3, 1}, {4, 1}}},
    {9, {{-4, 1}, {-3, 1}, {-2, 1}, {-1, 0}, {0, 0}, {1, 0}, {2, -1}, {3, -1}, {4, -1}}},
    {7, {{-2, -3}, {-1, -2}, {-1, -1}, {0, 0}, {1, 1}, {1, 2}, {2, 3}}},
    {7, {{2, -3}, {1, -2}, {1, -1}, {0, 0}, {-1, 1}, {-1, 2}, {-2, 3}}},
    {7, {{-3, -2}, {-2, -1}, {-1, -1}, {0, 0}, {1, 1}, {2, 1}, {3, 2}}},
    {7, {{3, -2}, {2, -1}, {1, -1}, {0, 0}, {-1, 1}, {-2, 1}, {-3, 2}}},
    {8, {{-4, 2}, {-3, 2}, {-2, 1}, {-1, 1}, {0, 0}, {1, 0}, {2, -1}, {3, -1}}},
    {8, {{-4, -2}, {-3, -2}, {-2, -1}, {-1, -1}, {0, 0}, {1, 0}, {2, 1}, {3, 1}}},
    {8, {{-2, -4}, {-2, -3}, {-1, -2}, {-1, -1}, {0, 0}, {0, 1}, {1, 2}, {1, 3}}},
    {8, {{2, -4}, {2, -3}, {1, -2}, {1, -1}, {0, 0}, {0, 1}, {-1, 2}, {-1, 3}}},
};
__device__ constexpr mline MALTA_LF[16] = {
    {5, {{-4, 0}, {-2, 0}, {0, 0}, {2, 0}, {4, 0}}},
    {5, {{0, -4}, {0, -2}, {0, 0}, {0, 2}, {0, 4}}},
    {5, {{-3, -3}, {-2, -2}, {0, 0}, {2, 2}, {3, 3}}},
    {5, {{3, -3}, {2, -2}, {0, 0}, {-2, 2}, {-3, 3}}},
    {5, {{1, -4}, {1, -2}, {0, 0}, {-1, 2}, {-1, 4}}},
    {5, {{-1, -4}, {-1, -2}, {0, 0}, {1, 2}, {1, 4}}},
    {5, {{-4, -1}, {-2, -1}, {0, 0}, {2, 1}, {4, 1}}},
    {5, {{-4, 1}, {-2, 1}, {0, 0}, {2, -1}, {4, -1}}},
    {5, {{-2, -3}, {-1, -2}, {0, 0}, {1, 2}, {2, 3}}},
    {5, {{2, -3}, {1, -2}, {0, 0}, {-1, 2}, {-2, 3}}},
    {5, {{-3, -2}, {-2, -1}, {0, 0}, {2, 1}, {3, 2}}},
    {5, {{3, -2}, {2, -1}, {0, 0}, {-2, 1}, {-3, 2}}},
    {5, {{-4, 2}, {-2, 1}, {0, 0}, {2, -1}, {4, -2}}},
    {5, {{-4, -2}, {-2, -1}, {0, 0}, {2, 1}, {4, 2}}},
    {5, {{-2, -4}, {-1, -2}, {0, 0}, {1, 2}, {2, 4}}},
    {5, {{2, -4}, {1, -2}, {0, 0}, {-1, 2}, {-2, 4}}},
};

// 64 x 32 outputs per block from a zero-padded 72 x 40 LDS tile of (x, y) pairs (1.41x halo)
constexpr int MT = 64, MH = 4, ML = MT + 2 * MH;

// a Malta line whose taps run from the bottom row to the top one (every other line runs top to bottom)
__device__ constexpr bool malta_line_descends(const mline &ln)
{
    for (int j = 1; j < ln.n; j++)
        if (ln.d[j][1] > ln.d[j - 1][1]) return false;
    return ln.d[0][1] != ln.d[ln.n - 1][1];
}
__device__ constexpr bool malta_line_monotone(const mline &ln)
{
    bool up = true, down = true;
    for (int j = 1; j < ln.n; j++) {
        if (ln.d[j][1] < ln.d[j - 1][1]) up = false;
        if (ln.d[j][1] > ln.d[j - 1][1]) down = false;
    }
    return up || down;
}
__device__ constexpr bool malta_tables_monotone()
{
    for (int k = 0; k < 16; k++)
        if (!malta_line_monotone(MALTA_HF[k]) || !malta_line_monotone(MALTA_LF[k])) return false;
    return true;
}
static_assert(malta_tables_monotone(), "the row-streaming Malta unit needs every line's rows to be visited in one direction");

// ---- per pair, fused: the three Malta bands of channels X and Y + every channel's L2 terms -----------------------
// For channel c in {X, Y}: UHF (9-sample lines), HF and MF (5-sample lines).  Per band the two images' 72x72
// regions are read once, the asymmetric pre-scaled difference (MaltaDiffMap's first loop) goes to LDS (zero outside
// the image, as PaddedMaltaUnit does) and the 16 line sums are squared and accumulated.  Then the
// L2DiffAsymmetric (HF), L2Diff (MF) and SetL2Diff (LF) terms of the channel are added and ac[c] / dc[c] are written
// once.  Channel B has no Malta term: only L2Diff (MF) and SetL2Diff (LF).
// A band's constants as (X, Y) pairs: the kernel's arguments arrive in scalar registers, and a pair that is adjacent here is
// an aligned register pair there, which is what a packed instruction takes as one operand.
struct malta_params_xy {
    ba_f2 norm2_0gt1, norm2_0lt1, norm1;
};
struct malta_bands {
    malta_params_xy p[3];  // [band: uhf, hf, mf]
};
__host__ inline malta_params_xy malta_pair(const malta_params &x, const malta_params &y)
{
    return malta_params_xy{ba_f2{x.norm2_0gt1, y.norm2_0gt1}, ba_f2{x.norm2_0lt1, y.norm2_0lt1}, ba_f2{x.norm1, y.norm1}};
}

// Two correctly rounded f32 quotients a0 / b and a1 / b with ONE reciprocal.  hipcc expands every IEEE division into
// v_div_scale x2, v_rcp, two fused steps that refine the reciprocal, a product, two fused quotient corrections, v_div_fmas
// and v_div_fixup (11 instructions) and does not share anything between two divisions by the same denominator.  For
// operands whose quotient cannot overflow, underflow or involve a denormal, v_div_scale returns its operand unchanged,
// v_div_fmas is a plain fma and v_div_fixup returns the quotient, so the same arithmetic is 3 shared + 5 per numerator =
// 13 instructions instead of 22, bit for bit (ce_debug_div_sweep checks it against operator/ on the device).  Here the
// numerators are positive constants in [1.7, 4.1e7] and b = norm1 + |..| is positive; measured (DESIGN.md section 15,
// "Operand ranges"): b in [5, 1.3e8] on RGB8 / deep batches, [5, 7.5e12 < 2^43] on linear batches (a +-1024 checker at
// intensity target 10 000), quotients down to 2.7e-13 = 2^-42.
// Written on (X, Y) pairs - ce_rcp_refined / ce_div_refined (ce_internal.h) on both halves at once, the same IEEE
// operations per half in the same order.  v_rcp_f32 has no packed form: two scalar instructions.
__device__ __forceinline__ ba_f2 rcp_refined_xy(ba_f2 b)
{
    const ba_f2 r0 = {__builtin_amdgcn_rcpf(b.x), __builtin_amdgcn_rcpf(b.y)};
    return __builtin_elementwise_fma(__builtin_elementwise_fma(-b, r0, ba_f2{1.0f, 1.0f}), r0, r0);
}
__device__ __forceinline__ ba_f2 div_refined_xy(ba_f2 a, ba_f2 b, ba_f2 r)  // r = refined reciprocal of b
{
    ba_f2 q = a * r;
    q = __builtin_elementwise_fma(__builtin_elementwise_fma(-b, q, a), r, q);
    return __builtin_elementwise_fma(__builtin_elementwise_fma(-b, q, a), r, q);
}

// MaltaDiffMap's pre-scaled difference of one position for channels X and Y together: v0 / v1 are the (X, Y) samples of the
// two images, the result is the pair the LDS tile stores.  Each half is the scalar chain; its fused steps, products, sums
// and differences run on v_pk_fma_f32 / v_pk_mul_f32 / v_pk_add_f32, the reciprocal, the comparisons and the selects per
// half.  |x| is formed explicitly: a packed instruction has no |.| source modifier.
__device__ __forceinline__ ba_f2 malta_pre_diff_xy(ba_f2 v0, ba_f2 v1, const malta_params_xy &mp)
{
    const ba_f2 fabs0 = __builtin_elementwise_abs(v0);
    const ba_f2 absval = ba_f2{0.5f, 0.5f} * (fabs0 + __builtin_elementwise_abs(v1));
    const ba_f2 diff = v0 - v1;
    const ba_f2 den = mp.norm1 + absval, rden = rcp_refined_xy(den);
    const ba_f2 scaler = div_refined_xy(mp.norm2_0gt1, den, rden), scaler2 = div_refined_xy(mp.norm2_0lt1, den, rden);
    const ba_f2 r = scaler * diff;
    // The four branches of MaltaDiffMap's asymmetry term, without divergence, in f32 (the lineage forms it in f64: worth
    // 9e-8 of the score, tests/golden/sensitivity.json "ba_malta_f32" - the oracle's switch of that name is this arithmetic
    // bit for bit; round 2 paid ten f64-rate instructions per sample for it).  Mirror v1 for a negative v0:
    //   v0 <  0: v1 > -too_small  <=>  u < too_small   r - scaler2 (v1 + too_small) = r - scaler2 (too_small - u)
    //            v1 < -too_big    <=>  u > too_big     r + scaler2 (-v1 - too_big)  = r + scaler2 (u - too_big)
    //   v0 >= 0: v1 <  too_small  <=>  u < too_small   r + scaler2 (too_small - v1)
    //            v1 >  too_big    <=>  u > too_big     r - scaler2 (v1 - too_big)
    // with u = v0 < 0 ? -v1 : v1.
    const ba_f2 too_small = ba_f2{0.55f, 0.55f} * fabs0, too_big = ba_f2{1.05f, 1.05f} * fabs0;
    const bool negx = v0.x < 0, negy = v0.y < 0;
    const ba_f2 u = {negx ? -v1.x : v1.x, negy ? -v1.y : v1.y};
    const bool lox = u.x < too_small.x, loy = u.y < too_small.y, hix = u.x > too_big.x, hiy = u.y > too_big.y;
    const ba_f2 below = too_small - u, above = u - too_big;
    const ba_f2 impact = scaler2 * ba_f2{lox ? below.x : above.x, loy ? below.y : above.y};
    const ba_f2 rn = r + ba_f2{(negx == lox) ? -impact.x : impact.x, (negy == loy) ? -impact.y : impact.y};
    return ba_f2{(lox || hix) ? rn.x : r.x, (loy || hiy) ? rn.y : r.y};
}

// L2DiffAsymmetric's in-place accumulation for one sample of hf[c] (libjxl / oracle l2_diff_asymmetric)
__device__ __forceinline__ float l2_asym_acc(float total, float val0, float val1, float vw_0gt1, float vw_0lt1)
{
    const float diff = val0 - val1;
    total = __builtin_fmaf(diff * diff, vw_0gt1, total);
    const float fabs0 = fabsf(val0);
    const float too_small = 0.4f * fabs0, too_big = fabs0;
    const float if_neg = val1 > -too_small ? val1 + too_small : (val1 < -too_big ? -val1 - too_big : 0.0f);
    const float if_pos = val1 < too_small ? too_small - val1 : (val1 > too_big ? val1 - too_big : 0.0f);
    const float v = val0 < 0.0f ? if_neg : if_pos;
    return __builtin_fmaf(vw_0lt1, v * v, total);
}

// Channels X and Y are PACKED: the LDS tile holds (x-diff, y-diff) pairs and a thread forms the 16 line sums of MaltaUnit
// for two horizontally adjacent centres and both channels at once on v_pk_add_f32 / v_pk_fma_f32 (two IEEE operations
// each, so every channel's sums are exactly those of a scalar loop).  The 9 x 10 window of pairs is STREAMED row by
// row (five 16-byte LDS reads per row) into 32 running line sums instead of being held whole (180 registers, two waves
// per SIMD, VALU busy 59 %): a line's taps are added in the lineage's order - fourteen of the sixteen lines run top
// to bottom, so their running sum simply follows the rows; lines 7 and 12 run bottom to top, so their taps are parked
// until the row of their FIRST tap arrives and are then added in order.  Bit-identical sums, ~150 registers, and with
// a 64 x 32 tile (72 x 40 pairs + 64 x 32 running sums = 39 KB) three to four blocks per CU.
template <bool LF>
__device__ __forceinline__ void malta_rows_xy(const ba_f2 *__restrict__ base, ba_f2 (&acc)[2])
{
    ba_f2 sum[2][16];
    ba_f2 parked[2][16][9];  // only the entries of the two bottom-up lines are ever touched (all indices are static)
#pragma unroll
    for (int r = 0; r < 9; r++) {
        ba_f2 v[10];
        const float4 *row = reinterpret_cast<const float4 *>(base + r * ML);
#pragma unroll
        for (int q = 0; q < 5; q++) {
            const float4 t = row[q];
            v[2 * q] = ba_f2{t.x, t.y};
            v[2 * q + 1] = ba_f2{t.z, t.w};
        }
        const int dy = r - 4;
#pragma unroll
        for (int o = 0; o < 2; o++) {
#pragma unroll
            for (int k = 0; k < 16; k++) {
                const mline &ln = LF ? MALTA_LF[k] : MALTA_HF[k];
                if (!malta_line_descends(ln)) {
#pragma unroll
                    for (int j = 0; j < 9; j++)
                        if (j < ln.n && ln.d[j][1] == dy) {
                            const ba_f2 t = v[4 + o + ln.d[j][0]];
                            sum[o][k] = j == 0 ? t : sum[o][k] + t;  // 0 + t == t: the lineage's sum starts at zero
                        }
                } else if (dy == ln.d[0][1]) {  // the row of the line's first tap: everything below it is parked
                    ba_f2 acc_k = {0.0f, 0.0f};
#pragma unroll
                    for (int j = 0; j < 9; j++)
                        if (j < ln.n) {
                            const ba_f2 t = ln.d[j][1] == dy ? v[4 + o + ln.d[j][0]] : parked[o][k][j];
                            acc_k = j == 0 ? t : acc_k + t;
                        }
                    sum[o][k] = acc_k;
                } else {
#pragma unroll
                    for (int j = 0; j < 9; j++)
                        if (j < ln.n && ln.d[j][1] == dy) parked[o][k][j] = v[4 + o + ln.d[j][0]];
                }
            }
        }
    }
#pragma unroll
    for (int o = 0; o < 2; o++) {
        ba_f2 ret = {0.0f, 0.0f};
#pragma unroll
        for (int k = 0; k < 16; k++) ret = __builtin_elementwise_fma(sum[o][k], sum[o][k], ret);
        acc[o] = acc[o] + ret;
    }
}

// MR rows of outputs per block, NT threads (32 threads per output row pair-column, NT / 32 rows per step):
//   <32, 256> (the one launched): 72 x 40 tile (1.41x halo), 39 KB LDS, four blocks per CU.  <64, 512> - a 72 x 72 tile,
//   10 % fewer pre-scalings, 73 KB LDS, two blocks of eight waves per CU - was slower (profiles/r02_experiments.md section 6)
// FINAL (the full-resolution level, launched after the half-resolution one): the pixel's diffmap value takes the
// half-resolution diffmap (AddSupersampled2x, weight 0.5) and goes straight into the score reductions - max, sum d^3, d^6,
// d^12 per tile - instead of to memory; !FINAL (the half-resolution level) writes its diffmap.
// FINAL && STORE (CE_FLAG_BUTTERAUGLI_DIFFMAP): the same reductions, and the final value of every pixel is also written
// to `diffmap` ([pair][h][pitch] of the full resolution), one float2 per thread and row - the thread's two columns (0 past
// the image's right edge, inside the pitch padding).
// The tile fill of a band (profiles/r08_malta_fill.md): a thread's three quads of the 72 x 40 region are laid out and their
// twelve float4 loads requested before any arithmetic; a position's X and Y samples are pre-scaled as one pair
// (malta_pre_diff_xy); nothing is loaded or computed behind a branch - a position outside the image is computed on
// whatever stands at the plane's start and 0 is selected for it at the end.  A block whose whole region lies inside the
// image (decided once, uniformly) takes the same body without the flags and selects.
template <int MR, int NT, bool FINAL, bool STORE>
__global__ __launch_bounds__(NT, NT == 256 ? 3 : 4) void k_ba_malta_l2_xy(const float *__restrict__ psy, const uint32_t *__restrict__ pair_ref,
                                                           const float *__restrict__ blurred, const float *__restrict__ mask_vals,
                                                           float *__restrict__ diffmap, ce_plane_geom g, uint32_t max_refs,
                                                           malta_bands mb, const uint2 *__restrict__ work, uint32_t tiles_x,
                                                           const float *__restrict__ sub_map, ce_plane_geom gs, int has_sub,
                                                           float *__restrict__ blk_max, double *__restrict__ blk_sums, uint32_t n_blocks,
                                                           int lf_term)
{
    constexpr int MLR = MR + 2 * MH, RSTEP = NT / 32;  // tile rows; output rows per step of the whole block
    __shared__ __attribute__((aligned(16))) ba_f2 s[MLR * ML];
    __shared__ __attribute__((aligned(16))) ba_f2 s_acc[MR * MT];  // the block's running sums; each thread owns its entries
    // XCD-aware 1-D launch (ce_build_xcd_list): the work list says which (tile, pair) this workgroup is
    const uint2 wi = work[blockIdx.x];
    if (wi.x == ~0u) return;  // padding entry
    const uint32_t p = wi.y, bx = wi.x % tiles_x, by = wi.x / tiles_x;
    const int x0 = (int)bx * MT - MH, y0 = (int)by * MR - MH;
    const float *a = psy + (size_t)pair_ref[p] * PSY * g.plane;
    const float *b = psy + (size_t)(max_refs + p) * PSY * g.plane;
    // thread -> two adjacent outputs (columns 2*tq, 2*tq+1 of row 8*sub + ty), four row groups per tile
    const int tq = threadIdx.x & 31, ty = threadIdx.x >> 5;
    const float wmul[9] = {400.0f, 1.50815703118f, 0.0f, 2150.0f, 10.6195433239f, 16.2176043152f, 29.2353797994f, 0.844626970982f, 0.703646627719f};
    const float hf_asymmetry = 1.0f;
    // The tile fill.  Per band a thread fills NI quads (four adjacent positions of one tile row): quads threadIdx.x + k NT of
    // the tile's MLR x ML / 4.  NQ is no multiple of NT: the threads past the last quad fill it once more - the same values to
    // the same addresses, and it lies in the halo, so no L2 term is added twice - so that no quad stands behind a branch,
    // which would keep its loads behind it too.
    constexpr int NQ = MLR * (ML / 4), NI = (NQ + NT - 1) / NT;
    static_assert(MH > 0, "the tile's last quad must hold no own pixel");
    // A quad's word: bits 0 .. 3 - sample j lies inside the image (gx + j < w: the pitch padding is outside); FQ_LOAD - its 16
    // bytes lie inside the plane's rows; FQ_OWN - it holds own pixels of the tile, whose L2 terms this block adds; the tile
    // row from bit 8, the quad of the row from bit 16.
    constexpr uint32_t FQ_LOAD = 16, FQ_OWN = 32;
    // A block whose whole region lies inside the image (84 of the 128 tiles of a 512 x 512 image) has every flag of every quad
    // set: it fills without predicates and selects.  Uniform - bx, by and g are scalars.
    const bool interior = x0 >= 0 && y0 >= 0 && x0 + ML <= (int)g.w && y0 + MLR <= (int)g.h;
#pragma unroll
    for (int band = 0; band < 3; band++) {
        const malta_params_xy mp = mb.p[band];
        const uint32_t plane0 = band == 0 ? UHF0 : band == 1 ? HF0 : MF0;  // channel X's plane; channel Y's is the next one
        const float *pax = a + (size_t)plane0 * g.plane, *pbx = b + (size_t)plane0 * g.plane;
        const float *pay = pax + g.plane, *pby = pbx + g.plane;
        // The quads' words are formed ahead of the band's arithmetic, once per band and not once per block: they are the same
        // for the three bands, but kept across the line sums - which take the whole register budget of four waves per SIMD -
        // they cost the kernel a wave (168 VGPRs, 5 - 9 of them spilled; profiles/r08_malta_fill.md).  The empty asm keeps
        // the compiler from keeping them by itself.
        uint32_t fq[NI];
        int tid = threadIdx.x;
        asm volatile("" : "+v"(tid));
#pragma unroll
        for (int k = 0; k < NI; k++) {
            const int i = min(tid + k * NT, NQ - 1), ly = i / (ML / 4), lq = i % (ML / 4), gx = x0 + 4 * lq, gy = y0 + ly;
            const bool in = gx >= 0 && gy >= 0 && gx < (int)g.pitch && gy < (int)g.h;
            const bool own = ly >= MH && ly < MH + MR && lq >= MH / 4 && lq < (MH + MT) / 4 && gy < (int)g.h;
            uint32_t m = (uint32_t)ly << 8 | (uint32_t)lq << 16 | (own ? FQ_OWN : 0u) | (in ? FQ_LOAD : 0u);
#pragma unroll
            for (int j = 0; j < 4; j++) m |= (in && gx + j < (int)g.w) ? 1u << j : 0u;
            fq[k] = m;
        }
        auto fill = [&](auto interior_c) {
            constexpr bool INTERIOR = decltype(interior_c)::value;
            // the band's loads of all the thread's quads are requested together, ahead of the first pre-scaling: the first
            // quad waits for its own 64 bytes only, the others' round trips pass behind its arithmetic.  No branch stands
            // between the quads (band 0) or only the L2 terms' (bands 1, 2), so their chains are scheduled into each other.
            float4 vax[NI], vbx[NI], vay[NI], vby[NI];
            auto load = [&](int k) {
                // no branch around a load: a quad with nothing to load reads the plane's first 16 bytes instead, and what it
                // makes of them is never used (0 is selected for a position outside the image, the L2 terms look at the flags)
                const bool in = INTERIOR || (fq[k] & FQ_LOAD);
                const int gy = in ? y0 + (int)(fq[k] >> 8 & 0xff) : 0, gx = in ? x0 + 4 * (int)(fq[k] >> 16) : 0;
                const size_t o = (size_t)gy * g.pitch + gx;
                vax[k] = *reinterpret_cast<const float4 *>(pax + o);
                vbx[k] = *reinterpret_cast<const float4 *>(pbx + o);
                vay[k] = *reinterpret_cast<const float4 *>(pay + o);
                vby[k] = *reinterpret_cast<const float4 *>(pby + o);
            };
            auto scale = [&](int k) {
                const int ly = fq[k] >> 8 & 0xff, lq = fq[k] >> 16;
                const bool i0 = INTERIOR || (fq[k] & 1), i1 = INTERIOR || (fq[k] & 2), i2 = INTERIOR || (fq[k] & 4), i3 = INTERIOR || (fq[k] & 8);
                // computed on whatever was loaded (the denominator is norm1 + |..| > 0); outside the image and in the pitch
                // padding the tile holds 0, selected afterwards
                const ba_f2 zero = {0.0f, 0.0f};
                const ba_f2 d0 = malta_pre_diff_xy(ba_f2{vax[k].x, vay[k].x}, ba_f2{vbx[k].x, vby[k].x}, mp);
                const ba_f2 d1 = malta_pre_diff_xy(ba_f2{vax[k].y, vay[k].y}, ba_f2{vbx[k].y, vby[k].y}, mp);
                const ba_f2 d2 = malta_pre_diff_xy(ba_f2{vax[k].z, vay[k].z}, ba_f2{vbx[k].z, vby[k].z}, mp);
                const ba_f2 d3 = malta_pre_diff_xy(ba_f2{vax[k].w, vay[k].w}, ba_f2{vbx[k].w, vby[k].w}, mp);
                const ba_f2 e0 = i0 ? d0 : zero, e1 = i1 ? d1 : zero, e2 = i2 ? d2 : zero, e3 = i3 ? d3 : zero;
                float4 *dst = reinterpret_cast<float4 *>(s + ly * ML + 4 * lq);
                dst[0] = make_float4(e0.x, e0.y, e1.x, e1.y);
                dst[1] = make_float4(e2.x, e2.y, e3.x, e3.y);
                // The HF / MF samples of the tile's OWN pixels are in registers here: their L2DiffAsymmetric (hf) / L2Diff (mf)
                // terms join the running block_diff_ac sums now (after the previous band's Malta sums, before this band's),
                // instead of being loaded again - 32 B per pixel - by the epilogue.  The same in-place accumulations as the
                // lineage's, in another order: the oracle's switch "ba_l2_early" is this order bit for bit.
                if (band >= 1 && (fq[k] & FQ_OWN)) {
                    const float4 ax = vax[k], bx_ = vbx[k], ay = vay[k], by_ = vby[k];
                    float4 *pa = reinterpret_cast<float4 *>(s_acc + (ly - MH) * MT + 4 * lq - MH);
                    float4 t01 = pa[0], t23 = pa[1];  // (x0, y0, x1, y1), (x2, y2, x3, y3)
                    if (band == 1) {
                        const float gx_ = wmul[0] * hf_asymmetry * 0.8f, lx_ = wmul[0] / hf_asymmetry * 0.8f;
                        const float gy_ = wmul[1] * hf_asymmetry * 0.8f, ly_ = wmul[1] / hf_asymmetry * 0.8f;
                        if (i0) t01.x = l2_asym_acc(t01.x, ax.x, bx_.x, gx_, lx_), t01.y = l2_asym_acc(t01.y, ay.x, by_.x, gy_, ly_);
                        if (i1) t01.z = l2_asym_acc(t01.z, ax.y, bx_.y, gx_, lx_), t01.w = l2_asym_acc(t01.w, ay.y, by_.y, gy_, ly_);
                        if (i2) t23.x = l2_asym_acc(t23.x, ax.z, bx_.z, gx_, lx_), t23.y = l2_asym_acc(t23.y, ay.z, by_.z, gy_, ly_);
                        if (i3) t23.z = l2_asym_acc(t23.z, ax.w, bx_.w, gx_, lx_), t23.w = l2_asym_acc(t23.w, ay.w, by_.w, gy_, ly_);
                    } else {
                        auto l2 = [](float total, float v0, float v1, float w) {
                            const float diff = v0 - v1;
                            return __builtin_fmaf(diff * diff, w, total);
                        };
                        if (i0) t01.x = l2(t01.x, ax.x, bx_.x, wmul[3]), t01.y = l2(t01.y, ay.x, by_.x, wmul[4]);
                        if (i1) t01.z = l2(t01.z, ax.y, bx_.y, wmul[3]), t01.w = l2(t01.w, ay.y, by_.y, wmul[4]);
                        if (i2) t23.x = l2(t23.x, ax.z, bx_.z, wmul[3]), t23.y = l2(t23.y, ay.z, by_.z, wmul[4]);
                        if (i3) t23.z = l2(t23.z, ax.w, bx_.w, wmul[3]), t23.w = l2(t23.w, ay.w, by_.w, wmul[4]);
                    }
                    pa[0] = t01;
                    pa[1] = t23;
                }
            };
#pragma unroll
            for (int k = 0; k < NI; k++) load(k);
#pragma unroll
            for (int k = 0; k < NI; k++) scale(k);
        };
        if (interior)
            fill(std::true_type{});
        else
            fill(std::false_type{});
        __syncthreads();
#pragma unroll 1
        for (int sub = 0; sub < MR / RSTEP; sub++) {
            ba_f2 acc[2] = {{0.f, 0.f}, {0.f, 0.f}};  // this band's sums; 0 + ret is exact, so adding them afterwards is the same sum
            const ba_f2 *base = s + (RSTEP * sub + ty) * ML + 2 * tq;
            // block_diff_ac accumulates band by band in the lineage: same order here
            if (band == 0)
                malta_rows_xy<false>(base, acc);
            else
                malta_rows_xy<true>(base, acc);
            float4 *pacc = reinterpret_cast<float4 *>(s_acc + (RSTEP * sub + ty) * MT + 2 * tq);
            float4 t = make_float4(0.f, 0.f, 0.f, 0.f);
            if (band != 0) t = *pacc;
            *pacc = make_float4(t.x + acc[0].x, t.y + acc[0].y, t.z + acc[1].x, t.w + acc[1].y);
        }
        __syncthreads();
    }
    float red_m = 0.0f;  // the diffmap is non-negative
    double red_s3 = 0.0, red_s6 = 0.0, red_s12 = 0.0;
#pragma unroll 1
    for (int sub = 0; sub < MR / RSTEP; sub++) {
    float dmap[2] = {0.0f, 0.0f};  // STORE: the row's two final values of this thread
#pragma unroll
    for (int r = 0; r < 2; r++) {
        const uint32_t x = bx * MT + 2 * tq + r, y = by * MR + RSTEP * sub + ty;
        if (x >= g.w || y >= g.h) continue;
        const size_t o = (size_t)y * g.pitch + x;
        const ba_f2 sums = s_acc[(RSTEP * sub + ty) * MT + 2 * tq + r];
        float acv[3], dcv[3];
#pragma unroll
        for (uint32_t c = 0; c < 3; c++) {
            // channels X and Y: the Malta sums of the three bands and the hf / mf L2 terms are all in `sums` (see the tile
            // fill); channel B has no Malta term and no hf: L2Diff on mf[2] only
            float total = c == 0 ? sums.x : c == 1 ? sums.y : 0.0f;
            if (c == 2) {
                const float diff = a[(MF0 + c) * g.plane + o] - b[(MF0 + c) * g.plane + o];
                total = __builtin_fmaf(diff * diff, wmul[3 + c], total);
            }
            acv[c] = total;
        }
        // CombineChannelsToDiffmap for this pixel (the mask values come from k_ba_mask_vals, once per reference): the
        // block_diff_ac / block_diff_dc triples never leave registers
        const size_t rslot = pair_ref[p];
        const float maskval = mask_vals[(rslot * 2 + 0) * g.plane + o];
        const float mdiff = blurred[rslot * g.plane + o] - blurred[((size_t)max_refs + p) * g.plane + o];
        float ac0 = acv[0], ac1 = acv[1], ac2 = acv[2];
        ac1 += 10.0f * mdiff * mdiff;  // kMaskToErrorMul
        const float xmul = 1.0f;
        ac0 *= xmul;
        float mc_dc;
        if (lf_term) {  // uniform: the LF column blur formed the term (EPI_LF_TERM) into the distorted slot's LF0 plane
            mc_dc = b[LF0 * g.plane + o];
        } else {
            const float dc_maskval = mask_vals[(rslot * 2 + 1) * g.plane + o];
#pragma unroll
            for (uint32_t c = 0; c < 3; c++) {  // SetL2Diff on lf[c]
                const float diff = a[(LF0 + c) * g.plane + o] - b[(LF0 + c) * g.plane + o];
                dcv[c] = (diff * diff) * wmul[6 + c];
            }
            float dc0 = dcv[0], dc1 = dcv[1], dc2 = dcv[2];
            dc0 *= xmul;
            mc_dc = dc0 * dc_maskval + dc1 * dc_maskval + dc2 * dc_maskval;
        }
        const float mc_ac = ac0 * maskval + ac1 * maskval + ac2 * maskval;
        float d = sqrtf(mc_dc + mc_ac);
        if (!FINAL) {
            diffmap[(size_t)p * g.plane + o] = d;
            continue;
        }
        if (has_sub) {  // AddSupersampled2x
            const float kHeuristicMixingValue = 0.3f, wgt = 0.5f;
            d *= 1.0f - kHeuristicMixingValue * wgt;
            d += wgt * sub_map[(size_t)p * gs.plane + (size_t)(y / 2) * gs.pitch + x / 2];
        }
        const double dd = d, d3 = dd * dd * dd, d6 = d3 * d3;
        red_s3 += d3;
        red_s6 += d6;
        red_s12 += d6 * d6;
        red_m = fmaxf(red_m, d);
        if (STORE) dmap[r] = d;
    }
    if constexpr (FINAL && STORE) {  // x is even and the pitch a multiple of 32: x < w puts x + 1 inside the row's pitch
        const uint32_t x = bx * MT + 2 * tq, y = by * MR + RSTEP * sub + ty;
        if (x < g.w && y < g.h)
            *reinterpret_cast<float2 *>(diffmap + (size_t)p * g.plane + (size_t)y * g.pitch + x) = make_float2(dmap[0], dmap[1]);
    }
    }
    if (FINAL) {  // one partial per (pair, tile): thread order, then wave order - fixed, so the sums are reproducible
        __shared__ float s_max[NT / 64];
        __shared__ double s_sum[3][NT / 64];
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            red_m = fmaxf(red_m, __shfl_down(red_m, off, 64));
            red_s3 += __shfl_down(red_s3, off, 64);
            red_s6 += __shfl_down(red_s6, off, 64);
            red_s12 += __shfl_down(red_s12, off, 64);
        }
        const int wv = threadIdx.x >> 6;
        if ((threadIdx.x & 63) == 0) {
            s_max[wv] = red_m;
            s_sum[0][wv] = red_s3;
            s_sum[1][wv] = red_s6;
            s_sum[2][wv] = red_s12;
        }
        __syncthreads();
        if (threadIdx.x == 0) {
            float mm = s_max[0];
            double sa = 0, sb = 0, sc = 0;
            for (int k = 0; k < NT / 64; k++) {
                mm = fmaxf(mm, s_max[k]);
                sa += s_sum[0][k];
                sb += s_sum[1][k];
                sc += s_sum[2][k];
            }
            const size_t bi = (size_t)p * n_blocks + wi.x;
            blk_max[bi] = mm;
            blk_sums[bi * 3] = sa;
            blk_sums[bi * 3 + 1] = sb;
            blk_sums[bi * 3 + 2] = sc;
        }
    }
}

// ---- per pair: mask -----------------------------------------------------------------------------------------------
// DiffPrecompute(sqrt(xdiff^2 + ydiff^2)) of the reference (m0) and the test image (m1) of a pair

// StoreMin3: keep the three smallest values seen, sorted.  The state (min0 <= min1 <= min2) starts sorted for the
// non-negative inputs of the mask, so the insertion is a min/max network - no branches, no indexed temporaries
// (the branchy form was compiled into a scratch-memory array).
__device__ __forceinline__ void store_min3(float v, float &min0, float &min1, float &min2)
{
    const float a = fminf(min0, v), t = fmaxf(min0, v);
    const float b = fminf(min1, t), u = fmaxf(min1, t);
    min2 = fminf(min2, u);
    min1 = b;
    min0 = a;
}

// mask = FuzzyErosion(blurred0); ac[1] += 10 (blurred0 - blurred1)^2; then CombineChannelsToDiffmap — one pass
// MaskPsychoImage's per-pixel mask values depend on the REFERENCE's blurred mask input only (FuzzyErosion, then the two
// f64 rational curves of MaskY / MaskDcY): formed once per reference slot - not once per pair - into two planes that a
// batch keeps with the PsychoImage between launches; the pair part of CombineChannelsToDiffmap is the Malta kernel's epilogue.
__global__ __launch_bounds__(TPB) void k_ba_mask_vals(const float *__restrict__ blurred, float *__restrict__ vals, ce_plane_geom g)
{
    const uint32_t z = blockIdx.z;  // reference slot
    BA_XY;
    const float *from = blurred + (size_t)z * g.plane;
    const int X = (int)x, Y = (int)y, W = (int)g.w, H = (int)g.h, S = 3;
    const uint32_t pitch = g.pitch;
#define at(yy, xx) from[(size_t)(yy) * pitch + (xx)]
    // FuzzyErosion: the three smallest of the centre and its eight neighbours at distance 3 that exist.  All nine
    // loads are issued unconditionally at clamped coordinates (independent, so they overlap); a neighbour that does
    // not exist enters as +inf, which store_min3 ignores.
    const int xl = max(X - S, 0), xr = min(X + S, W - 1), yu = max(Y - S, 0), yd = min(Y + S, H - 1);
    const float c0 = at(Y, X);
    const float v_l = at(Y, xl), v_lu = at(yu, xl), v_ld = at(yd, xl), v_r = at(Y, xr), v_ru = at(yu, xr), v_rd = at(yd, xr),
                v_u = at(yu, X), v_d = at(yd, X);
    const bool hl = X >= S, hr = X < W - S, hu = Y >= S, hd = Y < H - S;
    const float INF = __builtin_inff();
    float min0 = c0, min1 = 2 * min0, min2 = min1;
    store_min3(hl ? v_l : INF, min0, min1, min2);
    store_min3(hl && hu ? v_lu : INF, min0, min1, min2);
    store_min3(hl && hd ? v_ld : INF, min0, min1, min2);
    store_min3(hr ? v_r : INF, min0, min1, min2);
    store_min3(hr && hu ? v_ru : INF, min0, min1, min2);
    store_min3(hr && hd ? v_rd : INF, min0, min1, min2);
    store_min3(hu ? v_u : INF, min0, min1, min2);
    store_min3(hd ? v_d : INF, min0, min1, min2);
    const float mask = 0.45f * min0 + 0.3f * min1 + 0.25f * min2;
#undef at
    const double kGlobalScale = 1.0 / (17.83 * 0.790799174);
    const double val = (double)mask;
    double c = 2.5485944793 / ((0.451936922203 * val) + 0.829591754942);
    double rv = kGlobalScale * (1.0 + c);
    vals[((size_t)z * 2 + 0) * g.plane + o] = (float)(rv * rv);  // maskval
    c = 0.505054525019 / ((3.87449418804 * val) + 0.20025578522);
    rv = kGlobalScale * (1.0 + c);
    vals[((size_t)z * 2 + 1) * g.plane + o] = (float)(rv * rv);  // dc_maskval
}

// one block per pair: max and the three power sums over the block partials (fixed order), then the norms
__global__ __launch_bounds__(TPB) void k_ba_score(const float *__restrict__ blk_max, const double *__restrict__ blk_sums,
                                                  ce_dev_scores *__restrict__ scores, double *__restrict__ pnorm,
                                                  uint32_t n_blocks, uint32_t used_blocks, double npix)
{
    __shared__ float s_max[TPB];
    __shared__ double s_sum[3][TPB];
    const uint32_t p = blockIdx.x, t = threadIdx.x;
    float mx = 0.0f;
    double s[3] = {0, 0, 0};
    for (uint32_t k = t; k < used_blocks; k += TPB) {
        mx = fmaxf(mx, blk_max[(size_t)p * n_blocks + k]);
        for (int q = 0; q < 3; q++) s[q] += blk_sums[((size_t)p * n_blocks + k) * 3 + q];
    }
    s_max[t] = mx;
    for (int q = 0; q < 3; q++) s_sum[q][t] = s[q];
    __syncthreads();
    for (int off = TPB / 2; off > 0; off >>= 1) {
        if ((int)t < off) {
            s_max[t] = fmaxf(s_max[t], s_max[t + off]);
            for (int q = 0; q < 3; q++) s_sum[q][t] += s_sum[q][t + off];
        }
        __syncthreads();
    }
    if (t == 0) {
        scores[p].butteraugli = (double)s_max[0];
        const double opp = 1.0 / npix;
        pnorm[p] = (pow(opp * s_sum[0][0], 1.0 / 3.0) + pow(opp * s_sum[1][0], 1.0 / 6.0) + pow(opp * s_sum[2][0], 1.0 / 12.0)) / 3.0;
    }
}

// debug: rcp_refined_xy / div_refined_xy (two numerators over one denominator) and ce_div_noscale against operator/ on pseudo-random operands of the ranges their call sites
// use.  The range is the union over the batch kinds of what the oracle's probe records per site ("Operand ranges",
// tests/test_wide_content_cpu.py), rounded outward to whole binades: [2^-40, 2^92) - RGB8 and deep batches stay inside
// [2^-40, 2^40), a linear batch reaches 2^91.2 (cbrt_poly's second numerator at x = 1024) and 2^-20 (its first denominator
// stepping over zero near x = 3.764).  Exponents are drawn independently, so quotients run from 2^-132 (subnormal) to 2^132
// (overflow) - further than any site's: where a / b is subnormal, zero or infinite the two forms may round differently
// and the sample is not counted, as no site produces one.
constexpr uint32_t DIV_SWEEP_EXP_FIRST = 87u, DIV_SWEEP_EXP_SPAN = 132u;  // biased exponents 87 .. 218
__global__ __launch_bounds__(256) void k_div_sweep(uint64_t seed, uint64_t count, unsigned long long *out)
{
    unsigned long long bad = 0;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < count; i += (uint64_t)gridDim.x * blockDim.x) {
        uint64_t x = (i + seed) * 0x9E3779B97F4A7C15ull;  // splitmix64
        x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
        x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
        x ^= x >> 31;
        // random mantissas, exponents from the hash; either sign for the first numerator and - cbrt_poly's denominators are
        // negative beyond the crossing - for the denominator; a zero numerator now and then
        const uint32_t mb = (uint32_t)x & 0x7fffffu, ma = (uint32_t)(x >> 23) & 0x7fffffu, m2 = (uint32_t)(x >> 41) & 0x7fffffu;
        const uint32_t eb = DIV_SWEEP_EXP_FIRST + (uint32_t)((x >> 17) % DIV_SWEEP_EXP_SPAN),
                       ea = DIV_SWEEP_EXP_FIRST + (uint32_t)((x >> 7) % DIV_SWEEP_EXP_SPAN),
                       e2 = DIV_SWEEP_EXP_FIRST + (uint32_t)((x >> 3) % DIV_SWEEP_EXP_SPAN);
        const float b = __uint_as_float((eb << 23) | mb | ((uint32_t)(x >> 61) & 1u) << 31);
        float a0 = __uint_as_float((ea << 23) | ma | ((uint32_t)(x >> 60) & 1u) << 31), a1 = __uint_as_float((e2 << 23) | m2);
        if ((x >> 50 & 1023u) == 0) a0 = 0.0f;
        // the Malta fill's form: both numerators as one pair over the denominator twice
        const ba_f2 bb = {b, b}, q01 = div_refined_xy(ba_f2{a0, a1}, bb, rcp_refined_xy(bb));
        const float q0 = q01.x, q1 = q01.y;
        const float w0 = a0 / b, w1 = a1 / b;
        const bool in0 = a0 == 0.0f || (fabsf(w0) >= 1.17549435e-38f && fabsf(w0) <= 3.40282347e+38f);
        const bool in1 = fabsf(w1) >= 1.17549435e-38f && fabsf(w1) <= 3.40282347e+38f;
        bad += (in0 && __float_as_uint(q0) != __float_as_uint(w0)) + (in1 && __float_as_uint(q1) != __float_as_uint(w1));
        bad += in1 && __float_as_uint(ce_div_noscale(a1, b)) != __float_as_uint(w1);
    }
    if (bad) atomicAdd(out, bad);
}

blur_kernel make_kernel(float sigma)
{
    blur_kernel bk{};
    const float m = 2.25f;
    const double scaler = -1.0 / (2.0 * (double)sigma * (double)sigma);
    int diff = (int)(m * std::fabs(sigma));
    if (diff < 1) diff = 1;
    for (int i = -diff; i <= diff; i++) bk.k[i + diff] = (float)std::exp(scaler * i * i);
    bk.len = 2 * diff + 1;
    for (int d = 0; d < diff && d < 16; d++) {
        float lo = 0.0f, hi = 0.0f;
        for (int j = diff - d; j < bk.len; j++) lo += bk.k[j];
        for (int j = 0; j <= diff + d; j++) hi += bk.k[j];
        bk.lo[d] = 1.0f / lo;
        bk.hi[d] = 1.0f / hi;
    }
    return bk;
}

float inv_weight_sum(const blur_kernel &bk)
{
    float wsum = 0.0f;
    for (int j = 0; j < bk.len; j++) wsum += bk.k[j];
    return 1.0f / wsum;
}

malta_params make_malta(double w_0gt1, double w_0lt1, double norm1, bool lf)
{
    const double len = 3.75, mulli = lf ? 0.611612573796 : 0.39905817637;
    const float kWeight0 = 0.5f, kWeight1 = 0.33f;
    const double w_pre0gt1 = mulli * std::sqrt(kWeight0 * w_0gt1) / (len * 2 + 1);
    const double w_pre0lt1 = mulli * std::sqrt(kWeight1 * w_0lt1) / (len * 2 + 1);
    return malta_params{(float)(w_pre0gt1 * norm1), (float)(w_pre0lt1 * norm1), (float)norm1};
}

}  // namespace

int ce_butteraugli_div_sweep(ce_ctx *ctx, uint64_t seed, uint64_t count, uint64_t *mismatches)
{
    unsigned long long *d = nullptr, h = 0;
    CE_HIP(ctx, hipMalloc(&d, sizeof(h)));
    CE_HIP(ctx, hipMemsetAsync(d, 0, sizeof(h), ctx->stream));
    CE_LAUNCH(ctx, "div_sweep", k_div_sweep, dim3(4096), dim3(256), 0, seed, count, d);
    CE_HIP(ctx, hipMemcpyAsync(&h, d, sizeof(h), hipMemcpyDeviceToHost, ctx->stream));
    CE_HIP(ctx, hipStreamSynchronize(ctx->stream));
    CE_HIP(ctx, hipFree(d));
    if (mismatches) *mismatches = h;
    return CE_OK;
}

static int ba_prepare(ce_batch *b)
{
    if (b->ba.engaged()) return CE_OK;
    ce_ctx *ctx = b->ctx;
    ce_ba_set B;
    auto set = [](ce_plane_geom &d, uint32_t w, uint32_t h) {
        d.w = w;
        d.h = h;
        d.pitch = (w + 31u) & ~31u;
        d.plane = (size_t)d.pitch * h;
    };
    set(B.lvl[0], b->w, b->h);
    set(B.lvl[1], (b->w + 1) / 2, (b->h + 1) / 2);
    B.levels = (B.lvl[1].w >= 8 && B.lvl[1].h >= 8) ? 2 : 1;
    const size_t slots = (size_t)b->max_refs + b->max_pairs, P = b->max_pairs, p0 = B.lvl[0].plane;
    int rc = CE_OK;
    for (int l = 0; l < B.levels && rc == CE_OK; l++) {
        rc = B.psy[l].alloc(ctx, slots * PSY * B.lvl[l].plane);
        if (l == 1 && rc == CE_OK) rc = B.diff[l].alloc(ctx, P * B.lvl[l].plane);  // the full-resolution diffmap: map, on request
    }
    for (auto &p : B.s)
        if (rc == CE_OK) rc = p.alloc(ctx, slots * 3 * p0);
    // blurred mask input per image slot and level, the references' two mask-value planes per level (both persist like the
    // PsychoImage)
    for (int l = 0; l < B.levels && rc == CE_OK; l++) {
        rc = B.mask[l].alloc(ctx, slots * B.lvl[l].plane);
        if (rc == CE_OK) rc = B.mask_vals[l].alloc(ctx, (size_t)b->max_refs * 2 * B.lvl[l].plane);
    }
    B.blocks = ((B.lvl[0].w + 63) / 64) * ((B.lvl[0].h + 3) / 4);
    if (rc == CE_OK) rc = B.blk_max.alloc(ctx, P * B.blocks);
    if (rc == CE_OK) rc = B.blk_sums.alloc(ctx, P * B.blocks * 3);
    if (rc == CE_OK) rc = B.pnorm.alloc(ctx, P);
    if (rc != CE_OK) return rc;  // all or nothing: B releases what it got
    b->ba = std::move(B);
    return CE_OK;
}

int ce_launch_butteraugli(ce_batch *b, const uint8_t *d_refs, uint32_t n_refs_used, uint32_t n_pairs, float intensity_target,
                          bool store_map)
{
    ce_ctx *ctx = b->ctx;
    int rc = ba_prepare(b);
    if (rc != CE_OK) return rc;
    // CE_FLAG_BUTTERAUGLI_DIFFMAP: the full-resolution diffmaps of all pairs, allocated by the first launch that asks for
    // them (one allocation: there is nothing to undo if it fails) and kept with the working set
    if (store_map && !b->ba.map && b->ba.map.alloc((ce_ctx *)nullptr, (size_t)b->max_pairs * b->ba.lvl[0].plane) != CE_OK) {
        ctx->err = "out of device memory for the Butteraugli diffmaps";
        return CE_ERR_BACKEND;
    }
    const uint32_t n_slots = n_refs_used + n_pairs, mr = b->max_refs;
    // the references' PsychoImage, mask input and mask values (both resolutions) of an earlier launch with the same
    // intensity target are still in place?  Then only the distorted slots go through the per-image chain
    const bool cached = b->refs.reuse(CE_REF_BUTTERAUGLI, d_refs, n_refs_used, ce_ref_param_f32(intensity_target));
    const uint32_t z0 = cached ? n_refs_used : 0, nz = n_slots - z0;
    // Where the LF term of CombineChannelsToDiffmap is formed (ce_plan.h: ce_plan_ba_lf_term_in_blur): in the LF column blur
    // when the references' LF planes and mask values are already in place, else in Malta's epilogue as always.
    // CE_BA_LF_TERM=0 forces the latter, for A/B runs; 2 forms the term in the blur but keeps the blur's launches in slot
    // order, where 1 (the default) walks the reference-ordered list (k_ba_blur_v_split: lf_work).
    static const int lf_term_mode = [] { const char *e = std::getenv("CE_BA_LF_TERM"); return e && e[0] >= '0' && e[0] <= '2' ? e[0] - '0' : 1; }();
    const bool lf_term = ce_plan_ba_lf_term_in_blur(lf_term_mode != 0, cached);
// the arguments of k_ba_blur_v_split that only EPI_LF_TERM reads
#define BA_NO_LF_TERM (const uint32_t *)nullptr, (const float *)nullptr, (const float *)nullptr, (const uint2 *)nullptr
    const blur_kernel k12 = make_kernel(1.2f), kLf = make_kernel(7.15593339443f), kHf = make_kernel(3.22489901262f),
                      kUhf = make_kernel(1.56416327805f), kMask = make_kernel(2.7f);
    float sw = 0.0f;
    for (int j = 0; j < 5; j++) sw += k12.k[j];
    const float sc = 1.0f / sw, w0 = k12.k[2] * sc, w1 = k12.k[3] * sc, w2 = k12.k[4] * sc;
    const double hf_asymmetry = 1.0;
    const malta_params mUhfY = make_malta(1.10039032555 * hf_asymmetry, 1.10039032555 / hf_asymmetry, 71.7800275169, false);
    const malta_params mUhfX = make_malta(173.5 * hf_asymmetry, 173.5 / hf_asymmetry, 5.0, false);
    const malta_params mHfY = make_malta(18.7237414387 * std::sqrt(hf_asymmetry), 18.7237414387 / std::sqrt(hf_asymmetry), 4498534.45232, true);
    const malta_params mHfX = make_malta(6923.99476109 * std::sqrt(hf_asymmetry), 6923.99476109 / std::sqrt(hf_asymmetry), 8051.15833247, true);
    const malta_params mMfY = make_malta(37.0819870399, 37.0819870399, 130262059.556, true);
    const malta_params mMfX = make_malta(8246.75321353, 8246.75321353, 1009002.70582, true);

    // half resolution first: the full-resolution level's Malta kernel folds that diffmap into its own values and reduces
    // them to the score partials.
    // A small batch (the one-pair-per-call regime) is a chain of 16 dependent launches of a few workgroups each; the two
    // resolution levels are independent until the full-resolution Malta kernel, so the half-resolution chain runs on a stream
    // of its own (with its own scratch planes) beside the full-resolution one: two cross-stream events instead of seven
    // launches on the critical path (profiles/r03_experiments.md section 14).
    const bool two_streams = b->ba.levels == 2 && !ctx->prof_serial && (double)n_pairs * b->w * b->h <= 4e6;
    hipStream_t s_main = CE_STREAM(ctx), s_half = s_main;
    if (two_streams) {
        if (!b->ba.half.stream) {  // whole or not at all: a failure leaves no stream behind for the next launch to trust
            ce_ba_half half;
            if (!(half.stream = ce_ctx_aux_stream(ctx, ce_ctx::AUX_BA_HALF))) return CE_ERR_BACKEND;
            if ((rc = half.ev_fork.create(ctx)) != CE_OK || (rc = half.ev_join.create(ctx)) != CE_OK) return rc;
            const size_t slots = (size_t)b->max_refs + b->max_pairs;
            for (auto &p : half.s)
                if ((rc = p.alloc(ctx, slots * 3 * b->ba.lvl[1].plane)) != CE_OK) return rc;
            b->ba.half = std::move(half);
        }
        s_half = b->ba.half.stream;
        CE_HIP(ctx, hipEventRecord(b->ba.half.ev_fork, s_main));
        CE_HIP(ctx, hipStreamWaitEvent(s_half, b->ba.half.ev_fork, 0));
    }
    // The per-slot kernels' launch order (ba_slot_order.h).  A/B knobs: CE_BA_SLOT_ORDER_MIN = slots per launch from which a
    // slot's tiles stay on one XCD, CE_BA_SLOT_ORDER_KERNELS = the kernels that follow it (bits: 1 front, 2 h33, 4 v_lf,
    // 8 hv_mf, 16 hv_hf, 32 hv_mask; the others keep tile order at every size)
    static const uint32_t order_min = [] {
        const char *e = std::getenv("CE_BA_SLOT_ORDER_MIN");
        return e ? (uint32_t)std::atol(e) : ba_slot_order_min;
    }();
    static const uint32_t order_kernels = [] {
        const char *e = std::getenv("CE_BA_SLOT_ORDER_KERNELS");
        return e ? (uint32_t)std::atol(e) : 63u;
    }();
    uint32_t final_tiles = 0;
    for (int l = b->ba.levels - 1; l >= 0; l--) {
        const ce_plane_geom &d = b->ba.lvl[l], &g = d;
        const dim3 gx((d.w + 63) / 64, (d.h + 3) / 4, 1);
        auto G = [&](uint32_t z) { return dim3(gx.x, gx.y, z); };
        hipStream_t st = l == 1 ? s_half : s_main;
        const ce_dev<float> *scr = (two_streams && l == 1) ? b->ba.half.s : b->ba.s;
        float *psy = b->ba.psy[l], *sA = scr[0], *sC = scr[2];
        // ---- per image slot: PsychoImage ----
        const plane_sel s3{3, 0, 3};
        // the launch order (ba_slot_order.h): a slot's tiles on one XCD when the launch has enough slots
        auto SG = [&](uint32_t tile_w, uint32_t tile_h, uint32_t planes, uint32_t kernel_bit) {
            return ba_slot_grid_make((d.w + tile_w - 1) / tile_w, (d.h + tile_h - 1) / tile_h, planes, nz, z0,
                                     (order_kernels & kernel_bit) ? order_min : ~0u);
        };
        auto SB = [](const ba_slot_grid &s) {
            const ba_slot_dims3 dims = ba_slot_dims(s);
            return dim3(dims.x, dims.y, dims.z);
        };
        const ba_slot_grid sg_front = SG(FT, FT, 1, 1), sg_h33 = SG(256, 8 * BH_TILES, 3, 2), sg_vlf = SG(64, 32, 1, 4),
                           sg_mf = SG(64, 32, 1, 8), sg_hf = SG(64, 32, 1, 16), sg_mask = SG(64, 32, 1, 32);
        for (const ba_slot_grid &s : {sg_front, sg_h33, sg_vlf, sg_mf, sg_hf, sg_mask})
            if (ba_slot_dims(s).y > ba_slot_grid_yz_max || ba_slot_dims(s).z > ba_slot_grid_yz_max) {
                ctx->err = "Butteraugli batch too large for one launch";
                return CE_ERR_BACKEND;
            }
        const dim3 ft = SB(sg_front);
        const ce_plane_geom &gfull = b->ba.lvl[0];
        if (b->linear) {  // a linear batch: f32 samples, no table
            const float *none = nullptr;
            if (l == 0)
                CE_LAUNCH_ON(ctx, st, "ba_front_lin", (k_ba_front<false, float>), ft, dim3(TPB), 0, d_refs, b->d_tests, none, none, g, sC, g,
                             w0, w1, w2, intensity_target, b->img_bytes, n_refs_used, mr, sg_front);
            else
                CE_LAUNCH_ON(ctx, st, "ba_front_half_lin", (k_ba_front<true, float>), ft, dim3(TPB), 0, d_refs, b->d_tests, none, none, gfull,
                             sC, g, w0, w1, w2, intensity_target, b->img_bytes, n_refs_used, mr, sg_front);
        } else if (b->depth[0]) {  // a deep batch: u16 samples, one table per side (rule 0, the f64 curve)
            const float *lr = b->deep_lut[0][0], *lt = b->deep_lut[0][1];
            if (l == 0)
                CE_LAUNCH_ON(ctx, st, "ba_front_u16", (k_ba_front<false, uint16_t>), ft, dim3(TPB), 0, d_refs, b->d_tests, lr, lt, g, sC, g,
                             w0, w1, w2, intensity_target, b->img_bytes, n_refs_used, mr, sg_front);
            else
                CE_LAUNCH_ON(ctx, st, "ba_front_half_u16", (k_ba_front<true, uint16_t>), ft, dim3(TPB), 0, d_refs, b->d_tests, lr, lt, gfull,
                             sC, g, w0, w1, w2, intensity_target, b->img_bytes, n_refs_used, mr, sg_front);
        } else if (l == 0) {
            CE_LAUNCH_ON(ctx, st, "ba_front_u8", (k_ba_front<false, uint8_t>), ft, dim3(TPB), 0, d_refs, b->d_tests, ctx->d_lut_ssim2,
                         ctx->d_lut_ssim2, g, sC, g, w0, w1, w2, intensity_target, b->img_bytes, n_refs_used, mr, sg_front);
        } else {
            CE_LAUNCH_ON(ctx, st, "ba_front_half", (k_ba_front<true, uint8_t>), ft, dim3(TPB), 0, d_refs, b->d_tests, ctx->d_lut_ssim2,
                         ctx->d_lut_ssim2, gfull, sC, g, w0, w1, w2, intensity_target, b->img_bytes, n_refs_used, mr, sg_front);
        }
        // LF = blur(xyb, 7.156) -> psy[LF0..2]
        // SeparateFrequencies: row blur of a band, then column blur fused with the pointwise split (k_ba_blur_v_split)
        {
            if (kLf.len != 33 || kHf.len != 15 || kUhf.len != 7) {
                ctx->err = "unexpected blur kernel length";
                return CE_ERR_BACKEND;
            }
            float *sB = scr[1];
            // LF: row pass sC -> sA, column pass + split: LF -> psy, raw MF -> sB
            CE_LAUNCH_ON(ctx, st, "ba_blur_h33", k_ba_blur_h<33>, SB(sg_h33), dim3(TPB), 0, (const float *)sC, sA, g, s3, s3, kLf, inv_weight_sum(kLf),
                      n_refs_used, mr, 1, sg_h33);
            // 32 rows per block of the column / fused stages (26 / 21 KB of LDS and ~100 / 56 registers: five blocks per
            // CU).  64 rows (smaller halo, 45 / 38 KB, three or four blocks) measured equal or slower
            // (profiles/r02_experiments.md section 18, r03_experiments.md section 12).
            // (lf_term: the distorted slots' LF term instead of their three LF planes, see EPI_LF_TERM)
            if (lf_term) {
                // A launch large enough for the slot order spreads a reference's distorted slots over the XCDs, and every
                // XCD's L2 then fetches the reference's lines for itself (16 B per pixel: profiles/r09_ba_lf_term.md).  It
                // walks a list instead that keeps the pairs of a reference, tile by tile, on one XCD (one key per tile column:
                // a tile's lower neighbour follows it on the same XCD, as in slot order).  Smaller launches keep their grid.
                const uint2 *lf_work = nullptr;
                dim3 grid = SB(sg_vlf);
                if (sg_vlf.by_xcd && lf_term_mode == 1 && sg_vlf.tiles_x <= 0xffffu && sg_vlf.tiles_y <= 0xffffu) {
                    if ((rc = ce_build_xcd_list(b, n_pairs, ce_xcd_keys{sg_vlf.tiles_x, 1, sg_vlf.tiles_y}, &b->ba.work_lf[l])) != CE_OK) return rc;
                    lf_work = b->ba.work_lf[l].d;
                    grid = dim3(b->ba.work_lf[l].len);
                }
                CE_LAUNCH_ON(ctx, st, "ba_blur_v_lf", (k_ba_blur_v_split<33, EPI_LF_TERM, false, 32>), grid, dim3(TPB), 0,
                             (const float *)sA, (const float *)sC, psy, g, kLf, inv_weight_sum(kLf), n_refs_used, mr, sg_vlf, (float *)nullptr,
                             sB, (const uint32_t *)b->d_pair_ref, (const float *)psy, (const float *)b->ba.mask_vals[l], lf_work);
            } else
                CE_LAUNCH_ON(ctx, st, "ba_blur_v_lf", (k_ba_blur_v_split<33, EPI_LF, false, 32>), SB(sg_vlf), dim3(TPB), 0, (const float *)sA,
                             (const float *)sC, psy, g, kLf, inv_weight_sum(kLf), n_refs_used, mr, sg_vlf, (float *)nullptr, sB, BA_NO_LF_TERM);
            // MF: row + column pass of raw MF (sB) + split: MF -> psy, raw HF -> sA (its old contents are dead)
            CE_LAUNCH_ON(ctx, st, "ba_blur_hv_mf", (k_ba_blur_v_split<15, EPI_MF, true, 32>), SB(sg_mf), dim3(TPB), 0, (const float *)sB,
                         (const float *)nullptr, psy, g, kHf, inv_weight_sum(kHf), n_refs_used, mr, sg_mf, (float *)nullptr, sA, BA_NO_LF_TERM);
            // HF: row + column pass of raw HF (sA) + split: HF, UHF -> psy, the mask input -> sB (raw MF is dead)
            CE_LAUNCH_ON(ctx, st, "ba_blur_hv_hf", (k_ba_blur_v_split<7, EPI_HF, true, 32>), SB(sg_hf), dim3(TPB), 0, (const float *)sA,
                         (const float *)nullptr, psy, g, kUhf, inv_weight_sum(kUhf), n_refs_used, mr, sg_hf, sB, (float *)nullptr, BA_NO_LF_TERM);
        }

        // mask input: DiffPrecompute of HF + UHF (written by the HF split's epilogue into scratch plane 1), blurred with sigma 2.7 -
        // per image slot (the references' once per reference; kept with the PsychoImage between launches), into
        // the level's own per-slot planes; then the
        // references' mask values (FuzzyErosion + the two mask curves), also once per reference
        {
            if (kMask.len != 13) {
                ctx->err = "unexpected blur kernel length";
                return CE_ERR_BACKEND;
            }
            CE_LAUNCH_ON(ctx, st, "ba_blur_hv_mask", (k_ba_blur_v_split<13, EPI_MASK, true, 32>), SB(sg_mask), dim3(TPB), 0, (const float *)scr[1],
                      (const float *)nullptr, psy, g, kMask, inv_weight_sum(kMask), n_refs_used, mr, sg_mask, (float *)nullptr, b->ba.mask[l], BA_NO_LF_TERM);
        }
        if (!cached)
            CE_LAUNCH_ON(ctx, st, "ba_mask_vals", k_ba_mask_vals, G(n_refs_used), dim3(TPB), 0, (const float *)b->ba.mask[l], b->ba.mask_vals[l], g);

        // ---- per pair: Malta + L2 terms + CombineChannelsToDiffmap -> the level's diffmap ----
        // 32-row tiles, 256 threads: the 64-row / 512-thread tile was slower (profiles/r02_experiments.md section 6,
        // r03_experiments.md section 12)
        malta_bands mb;
        mb.p[0] = malta_pair(mUhfX, mUhfY); mb.p[1] = malta_pair(mHfX, mHfY); mb.p[2] = malta_pair(mMfX, mMfY);
        const uint32_t tiles_x = (d.w + MT - 1) / MT, tiles_y = (d.h + 31) / 32;
        if ((rc = ce_build_xcd_list(b, n_pairs, ce_xcd_keys{1, tiles_x * tiles_y, 1}, &b->ba.work[l])) != CE_OK) return rc;
        const bool has_sub = b->ba.levels == 2;
        const ce_plane_geom &gsub = b->ba.lvl[has_sub ? 1 : 0];
#define CE_MALTA_ARGS(FINAL, STORE)                                                                                                \
    psy, b->d_pair_ref, (const float *)b->ba.mask[l], (const float *)b->ba.mask_vals[l],                                               \
        STORE ? b->ba.map : FINAL ? (float *)nullptr : b->ba.diff[1], g, mr, mb, (const uint2 *)b->ba.work[l].d, tiles_x,             \
        FINAL ? (const float *)b->ba.diff[1] : (const float *)nullptr, gsub, has_sub ? 1 : 0, b->ba.blk_max, b->ba.blk_sums, b->ba.blocks, lf_term ? 1 : 0
        const dim3 gmalta(b->ba.work[l].len);
        if (l == 0) {
            final_tiles = tiles_x * tiles_y;
            if (two_streams) CE_HIP(ctx, hipStreamWaitEvent(s_main, b->ba.half.ev_join, 0));  // the half-resolution diffmap
            if (store_map)  // the same kernel, also writing the diffmap: a profiler name of its own
                CE_LAUNCH_ON(ctx, st, "ba_malta_l2_map", (k_ba_malta_l2_xy<32, 256, true, true>), gmalta, dim3(256), 0, CE_MALTA_ARGS(true, true));
            else
                CE_LAUNCH_ON(ctx, st, "ba_malta_l2", (k_ba_malta_l2_xy<32, 256, true, false>), gmalta, dim3(256), 0, CE_MALTA_ARGS(true, false));
        } else {
            CE_LAUNCH_ON(ctx, st, "ba_malta_l2", (k_ba_malta_l2_xy<32, 256, false, false>), gmalta, dim3(256), 0, CE_MALTA_ARGS(false, false));
            if (two_streams) CE_HIP(ctx, hipEventRecord(b->ba.half.ev_join, s_half));
        }
#undef CE_MALTA_ARGS
    }
#undef BA_NO_LF_TERM
    const auto &d0 = b->ba.lvl[0];
    CE_LAUNCH(ctx, "ba_score", k_ba_score, dim3(n_pairs), dim3(TPB), 0, b->ba.blk_max, b->ba.blk_sums, b->d_scores, b->ba.pnorm,
              b->ba.blocks, final_tiles, (double)d0.w * (double)d0.h);
    CE_HIP(ctx, hipGetLastError());
    if (!cached) b->refs.built(CE_REF_BUTTERAUGLI, d_refs, n_refs_used, ce_ref_param_f32(intensity_target));
    return CE_OK;
}

// B x B cell maxima (B = 1: the packed map itself) of the stored diffmaps of pairs [first, first + count) into `out` (host,
// count * ceil(h / B) * ceil(w / B) floats); the caller has checked the range and B.  maps.hip: ce_read_map_cells.
int ce_butteraugli_read_maps(ce_batch *b, uint32_t first, uint32_t count, uint32_t block, float *out)
{
    return ce_read_map_cells(b, "ba_block_max", b->ba.map, b->ba.lvl[0], first, count, block, false, b->ba.cells, out);
}
