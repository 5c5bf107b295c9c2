// What the two segmented sorters share (rank.hip: Spearman ranks from (key, index) pairs; distribution.hip: sorted values from
// keys alone): the order-preserving key of a float, binary search in sorted keys, and the pieces of the 8-bit LSD radix pass
// that do not depend on a payload.
#pragma once
#include "common.h"

namespace {

constexpr int RK_RADIX = 256;

__device__ __forceinline__ uint32_t rank_key(float v) {
    uint32_t u = __float_as_uint(v);
    if (u == 0x80000000u) u = 0u;                      // -0.0 == +0.0
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

// the float a key was made from (-0.0 comes back as +0.0)
__device__ __forceinline__ float key_value(uint32_t k) {
    return __uint_as_float((k & 0x80000000u) ? (k & 0x7FFFFFFFu) : ~k);
}

// first position in sorted k[0, n) whose key is >= x (LB) or > x (!LB)
template <bool LB, typename P>
__device__ __forceinline__ uint32_t bound(P k, uint32_t n, uint32_t x) {
    uint32_t lo = 0, hi = n;
    while (lo < hi) {
        const uint32_t mid = (lo + hi) >> 1;
        const uint32_t v = k[mid];
        if (LB ? (v < x) : (v <= x)) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// the 64-bit mask of the lanes of this wave that are valid and carry the same 8-bit digit as this one
__device__ __forceinline__ uint64_t match_digit(uint32_t d, bool valid) {
    uint64_t m = __ballot(valid);
#pragma unroll
    for (int bit = 0; bit < 8; ++bit) {
        const uint64_t bl = __ballot((d >> bit) & 1u);
        m &= ((d >> bit) & 1u) ? bl : ~bl;
    }
    return m;
}

// per segment (blockIdx.x, RK_RADIX threads): hist[tile][digit] counts -> exclusive scatter offsets, digit-major then tile:
// off[t][d] = sum_{d' < d} total[d'] + sum_{t' < t} hist[t'][d]
__global__ void __launch_bounds__(RK_RADIX) radix_scan_kernel(uint32_t* __restrict__ hist, int ntiles) {
    __shared__ uint32_t tot[RK_RADIX];
    const int d = threadIdx.x;
    uint32_t* h = hist + (size_t)blockIdx.x * ntiles * RK_RADIX + d;
    uint32_t run = 0;
    for (int t = 0; t < ntiles; ++t) {
        const uint32_t v = h[(size_t)t * RK_RADIX];
        h[(size_t)t * RK_RADIX] = run;
        run += v;
    }
    tot[d] = run;
    __syncthreads();
    for (int s = 1; s < RK_RADIX; s <<= 1) {           // inclusive Hillis-Steele scan of the digit totals
        const uint32_t x = d >= s ? tot[d - s] : 0u;
        __syncthreads();
        tot[d] += x;
        __syncthreads();
    }
    const uint32_t base = tot[d] - run;
    for (int t = 0; t < ntiles; ++t) h[(size_t)t * RK_RADIX] += base;
}

inline size_t al256(size_t b) { return (b + 255) & ~size_t(255); }

}  // namespace
