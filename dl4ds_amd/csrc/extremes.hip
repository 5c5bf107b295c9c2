// Extreme-value verification: the sorted probability-weighted moments of a cell's samples (lmoments) and
// the declustered peaks over a threshold (pot_peaks).  The fits (GEV, Gumbel, GPD) and the return levels are host work on these
// per-cell numbers (dl4ds_amd/extremes.py).  The reference has no counterpart.
//
// lmoments.  Sample n of cell c lives at x[n*stride + c], stride >= per (row 0 of climate_indices' ext output, stride 2*per, and the
// peaks of pot_peaks are read in place).  The valid samples of a cell are the finite ones of sign*x (NaN is the mask, -0.0 is +0.0).
// With n their number and x_0 <= ... <= x_{n-1} their ascending values in fp64, for r = 0..3
//   S_r = sum_{j = r}^{n-1} w_r(j) * x_j in ascending j from its first term,   w_0 = 1,  w_r(j) = w_{r-1}(j) * ((j-r+1) / (n-r))
// every quotient correctly rounded, every product and sum rounded on its own (no fused multiply-add), and
//   pwm[r*per + c] = S_r / n  (NaN when n <= r),   valid[c] = n:
// Hosking's unbiased b_0..b_3.  Equal values have equal bits, so the order inside a tie does not matter.  The cells' ascending keys
// come from the per-cell engine of cell_sort.h (sign < 0: the keys of -x).  N <= SORT_STRIDED_MAX: the lane that owns a cell walks
// its LDS row in rank order.  Longer: a wave walks 64 cells of the chunk: tiles of 64 cells x 64 ranks come through LDS (read with
// lanes along the ranks, walked with lanes along the cells).
// Both walks are the same function on the same sequence of values: the same bits.  No atomics.
//
// pot_peaks.  x as in climate_indices (stride per), periods from period_starts, one threshold [1] or [per].  v = sign*x and
// u = sign*thr on fp32; a valid sample is an exceedance iff v > u.  A cluster opens at an exceedance and closes after `run`
// consecutive valid non-exceedances, at an invalid sample, at a period boundary and at the end of the series.  Its peak is the
// largest v (first occurrence), written as x with a zero as +0.0, in order of occurrence: peak[k*per + c], pos[k*per + c] for
// k < min(count, K); rows from count on hold NaN / -1; count[c] is the true number of clusters.  A threshold that is not finite
// gives count -1 and K rows of NaN / -1.  A lane owns a cell and walks the whole series in order (the peaks of a cell are numbered
// across the periods, so the parallelism is the cells alone); POT_DEPTH samples are loaded at once and consumed in order.
#include "common.h"
#include "ops.h"
#include "prof.h"
#include "cell_sort.h"
#include "periods.h"

// every product and sum of the S_r walk is rounded on its own
#pragma clang fp contract(off)

namespace {

constexpr int POT_CELLS = 64;                          // pot_peaks: cells (threads) per workgroup, one wave
constexpr int POT_DEPTH = 16;                          // pot_peaks: samples a lane has in flight

// the four running sums of one cell; add() takes the values in rank order j = 0, 1, ..., n-1
struct PwmWalk {
    double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0;
    __device__ __forceinline__ void add(uint32_t j, uint32_t n, double x) {
        s0 = j == 0 ? x : s0 + x;
        if (j < 1) return;
        double w = (double)j / (double)(n - 1);
        const double t1 = w * x;
        s1 = j == 1 ? t1 : s1 + t1;
        if (j < 2) return;
        w = w * ((double)(j - 1) / (double)(n - 2));
        const double t2 = w * x;
        s2 = j == 2 ? t2 : s2 + t2;
        if (j < 3) return;
        w = w * ((double)(j - 2) / (double)(n - 3));
        const double t3 = w * x;
        s3 = j == 3 ? t3 : s3 + t3;
    }
    __device__ __forceinline__ void store(uint32_t n, size_t c, size_t per, int* __restrict__ valid, double* __restrict__ pwm) const {
        if (valid) valid[c] = (int)n;
        if (!pwm) return;
        const double nan64 = __builtin_nan(""), dn = (double)n;
        pwm[c] = n > 0 ? s0 / dn : nan64;
        pwm[per + c] = n > 1 ? s1 / dn : nan64;
        pwm[2 * per + c] = n > 2 ? s2 / dn : nan64;
        pwm[3 * per + c] = n > 3 ? s3 / dn : nan64;
    }
};

// strided LDS engine: G cells of N <= P samples per workgroup
template <int P>
__global__ void __launch_bounds__(CELL_THREADS) lmom_lds_kernel(const float* __restrict__ x, size_t N, size_t per, size_t stride, int neg,
                                                               int* __restrict__ valid, double* __restrict__ pwm) {
    constexpr int G = cell_group<P>(), PITCH = P + 1;
    static_assert(G <= CELL_THREADS, "lmom_lds_kernel: one lane per cell");
    extern __shared__ __attribute__((aligned(16))) unsigned char lmom_lds[];
    uint32_t* key = reinterpret_cast<uint32_t*>(lmom_lds);                // [G][PITCH]
    const int t = threadIdx.x;
    const size_t c0 = (size_t)blockIdx.x * G;
    const int cells = (int)(per - c0 < (size_t)G ? per - c0 : (size_t)G);
    sorted_cell_rows<P>(x, N, stride, neg, c0, cells, key);
    if (t >= cells) return;
    const uint32_t* row = key + t * PITCH;
    const uint32_t n = bound<true>(row, (uint32_t)P, SORT_INVALID);
    PwmWalk acc;
    for (uint32_t j = 0; j < n; ++j) acc.add(j, n, (double)key_value(row[j]));
    acc.store(n, c0 + t, per, valid, pwm);
}

// global engine, step 3: one wave per 64 cells of the chunk, from their sorted keys
__global__ void __launch_bounds__(CELL_TR) lmom_walk_kernel(const uint32_t* __restrict__ k, size_t ncell, size_t N, size_t per,
                                                         size_t cell0, int* __restrict__ valid, double* __restrict__ pwm) {
    __shared__ uint32_t tk[CELL_TR][CELL_TR + 1];
    const int lane = threadIdx.x;
    const size_t c0 = (size_t)blockIdx.x * CELL_TR;
    const int cells = (int)(ncell - c0 < (size_t)CELL_TR ? ncell - c0 : (size_t)CELL_TR);
    const bool live = lane < cells;
    const uint32_t n = live ? bound<true>(k + (c0 + lane) * N, (uint32_t)N, SORT_INVALID) : 0u;
    uint32_t nmax = n;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) nmax = max(nmax, (uint32_t)__shfl_xor((int)nmax, o, 64));
    PwmWalk acc;
    for (uint32_t p0 = 0; p0 < nmax; p0 += CELL_TR) {                       // (uniform)
        __syncthreads();
        const size_t pos = (size_t)p0 + lane;
        for (int g = 0; g < cells; ++g) tk[g][lane] = pos < N ? k[(c0 + g) * N + pos] : SORT_INVALID;
        __syncthreads();
        if (live)
            for (int e = 0; e < CELL_TR && p0 + e < n; ++e) acc.add(p0 + e, n, (double)key_value(tk[lane][e]));
    }
    if (live) acc.store(n, cell0 + c0 + lane, per, valid, pwm);
}

// ------------------------------------------------------------------------------------------------------------------ pot_peaks
struct PotArgs {
    const float* x;
    size_t N, per;
    const long long* starts;                           // [P + 1], device
    const float* thr;
    int thr_per_cell, neg, run, K;
    int* count;
    float* peak;
    int* pos;
};

__global__ void __launch_bounds__(POT_CELLS) pot_peaks_kernel(const PotArgs a) {
    const size_t per = a.per, c = (size_t)blockIdx.x * POT_CELLS + threadIdx.x;
    const bool live = c < per;
    const size_t cc = live ? c : per - 1;                                 // an idle lane walks the last cell and stores nothing
    const bool neg = a.neg != 0;
    const float t0 = a.thr_per_cell ? a.thr[cc] : a.thr[0];
    const bool thr_ok = finite_f32(t0);
    const float u = neg ? -t0 : t0;
    const int K = a.K, run = a.run;
    const float nan32 = __builtin_nanf("");

    bool open = false;
    int gap = 0, count = 0, ppos = -1;
    float pk = 0.f;
    auto close = [&]() {
        if (open && live && count < K) {
            const float o = neg ? -pk : pk;
            if (a.peak) a.peak[(size_t)count * per + c] = o == 0.f ? 0.f : o;
            if (a.pos) a.pos[(size_t)count * per + c] = ppos;
        }
        count += open ? 1 : 0;
        open = false;
        gap = 0;
    };

    const float* col = a.x + cc;                                          // sample n at col[n*per]
    const size_t N = a.N;
    unsigned p = 0;
    size_t nb = (size_t)a.starts[1];                                      // the next period's first sample; N, never met, in the last
    for (size_t n0 = 0; n0 < N; n0 += POT_DEPTH) {
        float blk[POT_DEPTH];
#pragma unroll
        for (int k = 0; k < POT_DEPTH; ++k) {
            const size_t n = n0 + k < N ? n0 + k : N - 1;
            blk[k] = col[n * per];
        }
#pragma unroll
        for (int k = 0; k < POT_DEPTH; ++k) {
            const size_t n = n0 + k;
            if (n >= N) break;                                            // (uniform)
            if (n == nb) {                                                // (uniform) a period boundary cuts the cluster
                close();
                nb = (size_t)a.starts[++p + 1];                           // n < N = starts[P]: p + 1 <= P
            }
            const bool ok = finite_f32(blk[k]);
            const float x = blk[k] == 0.f ? 0.f : blk[k];                 // -0.0 counts as +0.0
            const float v = neg ? -x : x;
            if (!ok) {
                close();
            } else if (thr_ok && v > u) {
                if (!open || v > pk) { pk = v; ppos = (int)n; }
                open = true;
                gap = 0;
            } else if (open) {
                if (++gap >= run) close();
            }
        }
    }
    close();
    if (!live) return;
    a.count[c] = thr_ok ? count : -1;
    for (int k = thr_ok ? (count < K ? count : K) : 0; k < K; ++k) {
        if (a.peak) a.peak[(size_t)k * per + c] = nan32;
        if (a.pos) a.pos[(size_t)k * per + c] = -1;
    }
}

}  // namespace

size_t lmoments_workspace_bytes(size_t N, size_t per, size_t stride, int sign) {
    DL4DS_REQUIRE(N > 0 && per > 0, "lmoments: empty array");
    DL4DS_REQUIRE(N < (size_t(1) << 31), "lmoments: 2^31 or more samples are not supported");
    DL4DS_REQUIRE(per < (size_t(1) << 36), "lmoments: too many cells");
    DL4DS_REQUIRE(stride >= per, "lmoments: the stride between samples must be at least the number of cells");
    DL4DS_REQUIRE(sign == 1 || sign == -1, "lmoments: sign must be +1 or -1");
    return cell_sort_workspace_bytes(N, per);
}

void lmoments(hipStream_t s, const float* x, size_t N, size_t per, size_t stride, int sign, int* valid, double* pwm, void* workspace,
              size_t workspace_bytes) {
    const size_t need = lmoments_workspace_bytes(N, per, stride, sign);   // (refuses a bad request)
    DL4DS_REQUIRE(x, "lmoments: null array");
    DL4DS_REQUIRE(valid || pwm, "lmoments: both outputs are null");
    if (need) DL4DS_REQUIRE(workspace && workspace_bytes >= need, "lmoments workspace too small");
    const int neg = sign < 0;
    cell_sort(
        s, "lmoments", x, N, per, stride, neg, workspace,
        [&](auto P) { launch_cell_lds<P(), lmom_lds_kernel<P()>>(s, per, x, N, per, stride, neg, valid, pwm); },
        [&](const uint32_t* keys, size_t nc, size_t c0) {
            DL4DS_LAUNCH(lmom_walk_kernel, dim3((unsigned)cdivz(nc, CELL_TR)), dim3(CELL_TR), 0, s, keys, nc, N, per, c0, valid, pwm);
        });
}

size_t pot_peaks_workspace_bytes(size_t N, size_t per, const long long* period_starts, int P, int sign, int run, int K) {
    DL4DS_REQUIRE(N > 0 && per > 0, "pot_peaks: empty array");
    DL4DS_REQUIRE(N < (size_t(1) << 31), "pot_peaks: 2^31 or more samples are not supported");
    DL4DS_REQUIRE(P >= 1, "pot_peaks: at least one period is needed");
    DL4DS_REQUIRE(sign == 1 || sign == -1, "pot_peaks: sign must be +1 or -1");
    DL4DS_REQUIRE(run >= 1 && run <= POT_MAX_RUN, "pot_peaks: 1 <= run <= 32");
    DL4DS_REQUIRE(K >= 0, "pot_peaks: K must not be negative");
    check_period_starts("pot_peaks", period_starts, P, N);
    DL4DS_REQUIRE(cdivz(per, POT_CELLS) < (size_t(1) << 31), "pot_peaks: too many cells for one launch");
    return period_starts_bytes(P);
}

void pot_peaks(hipStream_t s, const float* x, size_t N, size_t per, const long long* period_starts, int P, const float* thr,
               int thr_per_cell, int sign, int run, int K, int* count, float* peak, int* pos, void* workspace, size_t workspace_bytes) {
    const size_t need = pot_peaks_workspace_bytes(N, per, period_starts, P, sign, run, K);                  // (refuses a bad request)
    DL4DS_REQUIRE(x && thr, "pot_peaks: null array or threshold");
    DL4DS_REQUIRE(count, "pot_peaks: null count output");
    DL4DS_REQUIRE(K == 0 || peak || pos, "pot_peaks: K > 0 with both the peak and the position output null");
    DL4DS_REQUIRE(workspace && workspace_bytes >= need, "pot_peaks workspace too small");
    const long long* starts = upload_period_starts(s, period_starts, P, workspace);
    const PotArgs a{x, N, per, starts, thr, thr_per_cell, sign < 0, run, K, count, peak, pos};
    ProfScope ps(s, "pot_peaks", 0.0, 4.0 * (double)N * (double)per + (double)per * (4.0 + (peak ? 4.0 * K : 0.0) + (pos ? 4.0 * K : 0.0)));
    DL4DS_LAUNCH(pot_peaks_kernel, dim3((unsigned)cdivz(per, POT_CELLS)), dim3(POT_CELLS), 0, s, a);
    HIP_CHECK(hipGetLastError());
}
