// Trend per grid cell over the periods: the Mann-Kendall statistic with its tie term, and Sen's slope.
// The reference has no counterpart.
//
// v is fp64 [P][per], one value per period and cell in period order (annual prcptot, rx1day or a mean from climate_indices, say),
// 1 <= P <= 128.  Time is the period index 0..P-1; a value is VALID iff finite, so gaps keep their true spacing.  Comparisons are
// made on fp64.  Per cell c (each output may be null, not all):
//   valid [per]     int32: n, the number of valid values
//   mk    [2][per]  int64: row 0 S = sum over i < j, both valid, of sign(v_j - v_i); row 1 the tie term, the sum over the groups
//                   of equal values of g(g - 1)(2g + 5), formed without a sort as sum_i (c_i - 1)(2 c_i + 5) with c_i the number
//                   of valid values equal to v_i.  Both are exact integers
//   sen   [per]     fp64: with the M = n(n - 1)/2 slopes s = (v_j - v_i) / (double)(j - i), i < j both valid, sorted ascending:
//                   s[(M-1)/2] for odd M, (s[M/2 - 1] + s[M/2]) * 0.5 for even M.  The subtraction, the division and the addition
//                   are each rounded on their own, the division correctly.  A zero is written as +0.0; NaN when n < 2
//
// Kernel: one workgroup of TRD_THREADS threads per cell; parallelism is the cells alone.  Thread i < P counts, in one pass over j,
// c_i and its share of S; the TRD_THREADS shares are folded by a fixed tree (integers: any order gives the same).  All threads
// form the P(P - 1)/2 slopes as order-preserving 64-bit keys in LDS, pair (i, j) at its place in the upper triangle, a pair with
// an invalid end as the all-ones key, which no slope has and which sorts last.  bitonic_rows<> of sort_keys.h sorts them, padded
// to 512 (P <= 32), 2048 (P <= 64) or 8192 keys; the M slopes are then the first M keys.
#include "common.h"
#include "ops.h"
#include "prof.h"
#include "sort_keys.h"

namespace {

constexpr int TRD_THREADS = 256;
constexpr uint64_t TRD_PAD = ~uint64_t(0);

// ascending keys are ascending doubles; -0.0 and +0.0 share the key of +0.0
__device__ __forceinline__ uint64_t trend_key(double v) {
    uint64_t u = (uint64_t)__double_as_longlong(v);
    if (u == 0x8000000000000000ull) u = 0ull;
    return (u >> 63) ? ~u : (u | 0x8000000000000000ull);
}
__device__ __forceinline__ double trend_value(uint64_t k) {
    return __longlong_as_double((long long)((k >> 63) ? (k & 0x7FFFFFFFFFFFFFFFull) : ~k));
}
__device__ __forceinline__ bool trend_finite(double v) { return __builtin_fabs(v) < __builtin_inf(); }     // false for NaN

template <int PAD>
__global__ void __launch_bounds__(TRD_THREADS) trend_kernel(const double* __restrict__ v, int P, size_t per, int* __restrict__ valid,
                                                            long long* __restrict__ mk, double* __restrict__ sen) {
    __shared__ uint64_t key[PAD];
    __shared__ double val[TRD_MAX_PERIODS];
    __shared__ long long red_s[TRD_THREADS], red_t[TRD_THREADS];
    __shared__ int red_n[TRD_THREADS];
    const int tid = threadIdx.x;
    const size_t c = blockIdx.x;
    if (tid < P) val[tid] = v[(size_t)tid * per + c];
    for (int k = tid; k < PAD; k += TRD_THREADS) key[k] = TRD_PAD;
    __syncthreads();
    long long s = 0, tie = 0;
    int n = 0;
    if (tid < P && trend_finite(val[tid])) {
        const double vi = val[tid];
        int same = 0;
        for (int j = 0; j < P; ++j) {
            const double vj = val[j];
            if (!trend_finite(vj)) continue;
            same += vj == vi ? 1 : 0;
            if (j > tid) s += (vj > vi ? 1 : 0) - (vj < vi ? 1 : 0);
        }
        tie = (long long)(same - 1) * (2 * same + 5);
        n = 1;
    }
    red_s[tid] = s;
    red_t[tid] = tie;
    red_n[tid] = n;
    if (sen) {
        for (int q = tid; q < P * P; q += TRD_THREADS) {
            const int i = q / P, j = q - i * P;
            if (i < j && trend_finite(val[i]) && trend_finite(val[j])) {
                const double slope = (val[j] - val[i]) / (double)(j - i);
                key[i * P - i * (i + 1) / 2 + (j - i - 1)] = trend_key(slope);
            }
        }
    }
    group_tree<TRD_THREADS>(tid, [&](int i, int j) {
        red_s[i] += red_s[j];
        red_t[i] += red_t[j];
        red_n[i] += red_n[j];
    });
    const int nv = red_n[0];
    if (sen && nv >= 2) bitonic_rows<PAD, 1, PAD, TRD_THREADS, false, uint64_t>(key, nullptr);          // (nv is uniform)
    if (tid != 0) return;
    if (valid) valid[c] = nv;
    if (mk) {
        mk[c] = red_s[0];
        mk[per + c] = red_t[0];
    }
    if (sen) {
        double r = __builtin_nan("");
        if (nv >= 2) {
            const int M = nv * (nv - 1) / 2;
            r = (M & 1) ? trend_value(key[(M - 1) / 2]) : (trend_value(key[M / 2 - 1]) + trend_value(key[M / 2])) * 0.5;
            r = r == 0.0 ? 0.0 : r;
        }
        sen[c] = r;
    }
}

}  // namespace

void trend(hipStream_t s, const double* v, int P, size_t per, int* valid, long long* mk, double* sen) {
    DL4DS_REQUIRE(P >= 1 && P <= TRD_MAX_PERIODS, "trend: 1 <= P <= 128 periods");
    DL4DS_REQUIRE(per > 0, "trend: empty array");
    DL4DS_REQUIRE(per < (size_t(1) << 31), "trend: too many cells for one launch");
    DL4DS_REQUIRE(v, "trend: null array");
    DL4DS_REQUIRE(valid || mk || sen, "trend: all three outputs are null");
    const int M = P * (P - 1) / 2;
    const dim3 g((unsigned)per), b(TRD_THREADS);
    ProfScope ps(s, "trend", 0.0, (double)per * (8.0 * P + (valid ? 4.0 : 0.0) + (mk ? 16.0 : 0.0) + (sen ? 8.0 : 0.0)));
    if (M <= 512) DL4DS_LAUNCH(trend_kernel<512>, g, b, 0, s, v, P, per, valid, mk, sen);
    else if (M <= 2048) DL4DS_LAUNCH(trend_kernel<2048>, g, b, 0, s, v, P, per, valid, mk, sen);
    else DL4DS_LAUNCH(trend_kernel<8192>, g, b, 0, s, v, P, per, valid, mk, sen);
    HIP_CHECK(hipGetLastError());
}
