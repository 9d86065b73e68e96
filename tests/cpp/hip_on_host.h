// What the *_kernel_host.cpp programs put in HIP's place to compile a kernel header of codec-eval_amd/csrc for the host: the
// keywords defined away, blockIdx / threadIdx / gridDim as plain variables that the program's loops set - every thread of
// every block of a launch runs in turn - and the vector types the kernels load and store through, with the alignment the
// device asks of them where a kernel's own address test is what keeps an access legal, so that UBSan stops a wide access to
// an address that is not a multiple of its width.  Include it before the kernel header.
#pragma once

#include <algorithm>
#include <cstdint>

#define __device__
#define __global__
#define __forceinline__ inline
#define __restrict__
#define __launch_bounds__(x)
struct idx3 {
    unsigned x, y;
};
[[maybe_unused]] static idx3 blockIdx, threadIdx, gridDim;
using std::max;
using std::min;
struct alignas(16) uint4 {
    uint32_t x, y, z, w;
};
struct uint2 {
    uint32_t x, y;
};
static inline uint4 make_uint4(uint32_t a, uint32_t b, uint32_t c, uint32_t d) { return {a, b, c, d}; }
static inline uint2 make_uint2(uint32_t a, uint32_t b) { return {a, b}; }
struct alignas(16) float4 {
    float x, y, z, w;
};
struct alignas(8) float2 {
    float x, y;
};
static inline float4 make_float4(float a, float b, float c, float d) { return {a, b, c, d}; }
static inline float2 make_float2(float a, float b) { return {a, b}; }
