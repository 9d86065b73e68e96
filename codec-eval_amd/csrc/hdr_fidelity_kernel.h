// The device code of the HDR fidelity scores (hdr_fidelity.hip), kept like resample_f32_kernel.h free of anything but the HIP
// keywords, float4 and blockIdx / threadIdx / gridDim, so that tests/cpp/hdr_fidelity_kernel_host.cpp can compile the same
// text for the host and run it under the host sanitizers.  k_hdr_fidelity is split at its barrier for that: hdrf_stage fills
// the LDS, hdrf_lane reads it and returns the lane's three integers; the reduction across lanes stays in hdr_fidelity.hip.
//
// The arithmetic (include/ce_metrics.h: ce_batch_hdr_fidelity): two 3 x 3 products in f32 and one Delta E in f64 whose
// products, sums, quotient and square root are each rounded separately - this text is compiled with -ffp-contract=off on the
// device and on the host - six table searches per pixel, and integers from there on.  The PQ curve is never evaluated here.
#pragma once

#include <cstddef>
#include <cstdint>

namespace {

constexpr uint32_t kHdrfThreads = 256;
constexpr int kHdrfCoarseBits = 12;  // the level of the table a block keeps in LDS: at most 2^12 - 1 thresholds, 16 KB

// coarse level of a table of `depth` bits: 2^min(depth, 12) - 1 thresholds, every 2^(depth - 12)-th of a deeper table
constexpr int hdrf_coarse_bits(int depth) { return depth > kHdrfCoarseBits ? kHdrfCoarseBits : depth; }
constexpr uint32_t hdrf_coarse_len(int depth) { return (1u << hdrf_coarse_bits(depth)) - 1u; }

struct hdrf_args {
    const float *refs, *tests;     // the batch's slabs: n_pixels * 3 floats per slot
    const uint32_t *pair_ref;      // pair -> reference slot
    const float *table;            // T[1 .. maxv] at [0, maxv), 64-byte aligned; read at depths above 12 only
    const float *coarse;           // coarse[j] = table[(j + 1) * 2^(depth - 12) - 1], hdrf_coarse_len entries (depth <= 12: the table)
    size_t n_pixels;
    float a[9], b[9];              // BT.2020 <- sRGB primaries; BT.2100's LMS <- BT.2020
    double denom;                  // 4096 * maxv
    uint32_t first;                // the launch's pairs are [first, first + gridDim.y) of those that tests and pair_ref start at
};

// the pair of this block
__device__ __forceinline__ uint32_t hdrf_pair(const hdrf_args &a) { return a.first + blockIdx.y; }

// The blocks a pair gets in a launch of n_pairs: a lane's unit of work is four pixels on the wide path and one on the other; a
// block has up to 16 KB of table to stage, so at most 64 blocks a pair, or what keeps a launch of few pairs near 1024 blocks.
inline uint32_t hdrf_blocks(size_t n_pixels, uint32_t n_pairs)
{
    const size_t work = (n_pixels & 3) ? n_pixels : n_pixels / 4;
    const size_t want = (work + kHdrfThreads - 1) / kHdrfThreads, cap = 1024 / n_pairs > 64 ? 1024 / n_pairs : 64;
    return (uint32_t)(want > cap ? cap : want ? want : 1);
}

// Before the barrier: the coarse level into s_tab.
template <int DEPTH>
__device__ __forceinline__ void hdrf_stage(const hdrf_args &a, float *s_tab)
{
    for (uint32_t i = threadIdx.x; i < hdrf_coarse_len(DEPTH); i += kHdrfThreads) s_tab[i] = a.coarse[i];
}

// code(x): how many thresholds are <= x (numpy.searchsorted(T, x, side="right")).  A table of 2^d - 1 sorted entries is
// searched in d steps without a branch: pos counts the entries known to be <= x, and entry pos + step - 1 decides whether
// `step` more are.  NaN and everything under T[1] fail every comparison: 0.  The first min(DEPTH, 12) steps probe only entries
// of the coarse level, in LDS; at depth 16 the last four walk the 15 thresholds between two coarse ones, entries
// [16 * pos, 16 * pos + 14] of the global table: one 64-byte line.
template <int DEPTH>
__device__ __forceinline__ int32_t hdrf_code(const float *__restrict__ table, const float *s_tab, float x)
{
    constexpr int CB = hdrf_coarse_bits(DEPTH);
    uint32_t pos = 0;
#pragma unroll
    for (int k = CB - 1; k >= 0; k--) {
        const uint32_t step = 1u << k;
        pos += s_tab[pos + step - 1] <= x ? step : 0u;
    }
    if (DEPTH > CB) {
        pos <<= (DEPTH - CB);
#pragma unroll
        for (int k = DEPTH - CB - 1; k >= 0; k--) {
            const uint32_t step = 1u << k;
            pos += table[pos + step - 1] <= x ? step : 0u;
        }
    }
    return (int32_t)pos;
}

// one image's pixel: c = Rc Gc Bc Lc Mc Sc
template <int DEPTH>
__device__ __forceinline__ void hdrf_codes(const hdrf_args &a, const float *s_tab, float r, float g, float b, int32_t c[6])
{
    float q[3], l[3];
#pragma unroll
    for (int i = 0; i < 3; i++) q[i] = (a.a[3 * i] * r + a.a[3 * i + 1] * g) + a.a[3 * i + 2] * b;
#pragma unroll
    for (int i = 0; i < 3; i++) l[i] = (a.b[3 * i] * q[0] + a.b[3 * i + 1] * q[1]) + a.b[3 * i + 2] * q[2];
#pragma unroll
    for (int i = 0; i < 3; i++) c[i] = hdrf_code<DEPTH>(a.table, s_tab, q[i]), c[3 + i] = hdrf_code<DEPTH>(a.table, s_tab, l[i]);
}

// the code differences of a pixel of a pair, reference minus test: d = dRc dGc dBc dLc dMc dSc
template <int DEPTH>
__device__ __forceinline__ void hdrf_diffs(const hdrf_args &a, const float *s_tab, const float ref[3], const float test[3], long long d[6])
{
    int32_t cr[6], ct[6];
    hdrf_codes<DEPTH>(a, s_tab, ref[0], ref[1], ref[2], cr);
    hdrf_codes<DEPTH>(a, s_tab, test[0], test[1], test[2], ct);
#pragma unroll
    for (int i = 0; i < 6; i++) d[i] = (long long)cr[i] - (long long)ct[i];
}

// ... -> k, the pixel's Delta E ITP in units of 2^-20 (under 2^33): what the scores sum and the maps (hdr_fidelity_map_kernel.h) store
__device__ __forceinline__ unsigned long long hdrf_itp_q20(const hdrf_args &a, const long long d[6])
{
    // the differences of BT.2100's ICtCp times 4096 * maxv, exact
    const long long di = 2048 * (d[3] + d[4]);
    const long long dct = 6610 * d[3] - 13613 * d[4] + 7003 * d[5];
    const long long dcp = 17933 * d[3] - 17390 * d[4] - 543 * d[5];
    const double fi = (double)di, fct = (double)dct, fcp = (double)dcp;
    const double s = (fi * fi + 0.25 * (fct * fct)) + fcp * fcp;  // BT.2124: T = Ct / 2
    const double e = 720.0 * __builtin_sqrt(s) / a.denom;
    return (unsigned long long)__builtin_rint(e * 1048576.0);
}

// one pixel of a pair into the lane's integers: acc = pq_sse, itp_sum_q20, itp_max_q20
template <int DEPTH>
__device__ __forceinline__ void hdrf_pixel(const hdrf_args &a, const float *s_tab, const float ref[3], const float test[3],
                                           unsigned long long acc[3])
{
    long long d[6];
    hdrf_diffs<DEPTH>(a, s_tab, ref, test, d);
    acc[0] += (unsigned long long)(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]);
    const unsigned long long k = hdrf_itp_q20(a, d);
    acc[1] += k;
    acc[2] = k > acc[2] ? k : acc[2];
}

// After the barrier: this lane's share of pair first + blockIdx.y, in k_psnr_sse's frame.  An image whose byte size is a multiple of
// 16 - a multiple of four pixels; every image of a slab then starts 16-byte aligned - is read as groups of four pixels, three
// 16-byte loads a side; any other pixel by pixel.
template <int DEPTH>
__device__ __forceinline__ void hdrf_lane(const hdrf_args &a, const float *s_tab, unsigned long long acc[3])
{
    const uint32_t p = hdrf_pair(a);
    const size_t img = a.n_pixels * 3;
    const float *ref = a.refs + (size_t)a.pair_ref[p] * img;
    const float *test = a.tests + (size_t)p * img;
    const size_t tid = (size_t)blockIdx.x * kHdrfThreads + threadIdx.x;
    const size_t nthreads = (size_t)gridDim.x * kHdrfThreads;
    acc[0] = acc[1] = acc[2] = 0;
    if ((a.n_pixels & 3) == 0) {
        const float4 *r4 = reinterpret_cast<const float4 *>(ref);
        const float4 *t4 = reinterpret_cast<const float4 *>(test);
        for (size_t i = tid; i < a.n_pixels / 4; i += nthreads) {
            const float4 r0 = r4[i * 3], r1 = r4[i * 3 + 1], r2 = r4[i * 3 + 2];
            const float4 t0 = t4[i * 3], t1 = t4[i * 3 + 1], t2 = t4[i * 3 + 2];
            const float r[12] = {r0.x, r0.y, r0.z, r0.w, r1.x, r1.y, r1.z, r1.w, r2.x, r2.y, r2.z, r2.w};
            const float t[12] = {t0.x, t0.y, t0.z, t0.w, t1.x, t1.y, t1.z, t1.w, t2.x, t2.y, t2.z, t2.w};
#pragma unroll
            for (int k = 0; k < 4; k++) hdrf_pixel<DEPTH>(a, s_tab, r + 3 * k, t + 3 * k, acc);
        }
    } else {
        for (size_t i = tid; i < a.n_pixels; i += nthreads) {
            const float r[3] = {ref[i * 3], ref[i * 3 + 1], ref[i * 3 + 2]};
            const float t[3] = {test[i * 3], test[i * 3 + 1], test[i * 3 + 2]};
            hdrf_pixel<DEPTH>(a, s_tab, r, t, acc);
        }
    }
}

}  // namespace
