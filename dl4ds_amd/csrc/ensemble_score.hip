// Verification of an MC-dropout ensemble against an observation (the MCDropout / MCGaussianDropout / MCSpatialDropout layers of
// blocks.py:658-676 give the members; the reference leaves their verification to the user): CRPS, squared error of the ensemble mean,
// ensemble variance, rank of the observation among the members and coverage of the ensemble's quantiles, from ONE read of the
// member stack members[K][n] plus the observation row obs[n].  DESIGN.md section 13.
//
// Stage 1 (ensemble_score_reg / ensemble_score_staged), per element, the register / LDS-column budgeting of ensemble.hip:
//   valid   iff obs[e] and all K members are finite and, with a scale, scale[e % per] is finite and > 0.  An invalid element gets
//           NaN / rank -1 / no covered bit and takes no part in any fold.
//   d_k = x_k - y in fp64 (exact for fp32 inputs of comparable magnitude), then
//   crps    = (1/K) sum_k |d_k|  -  c * sum_i (2 i - K + 1) d_(i),  d_(i) the sorted differences (0-based), which is
//             sum_{i<j} |x_i - x_j|; c = 1 / K^2, or 1 / (K (K - 1)) for the fair CRPS (K = 1: the pair term is 0).  Times scale.
//             Evaluated as sum / K - pair / (1 / c), two divisions: equal real quotients round equally, so a fair CRPS whose
//             parts cancel (members (0, 0, a), y = 0) is exactly 0.
//   sqerr   = (mean - y)^2, var = sum_k (x_k - mean)^2 / (K - 1) (K = 1: 0), mean = (sum_k x_k) / K: sequential fp64 sums in member
//             order as in ensemble.hip.  Times scale^2.
//   rank    = #{k : x_k < y} + tie(seed, g, #{k : x_k == y}), g = elem_offset + e the element's global index and
//             tie(seed, g, m): z = seed + 0x9E3779B97F4A7C15 * (g + 1);  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9;
//                              z = (z ^ (z >> 27)) * 0x94D049BB133111EB;  z = z ^ (z >> 31)        (splitmix64, all mod 2^64)
//                              tie = ((z >> 32) * (m + 1)) >> 32                                   (one of 0 ... m; 0 when m = 0)
//   covered bit j = [y <= Q_j], Q_j the fp32 'linear' quantile of ensemble.hip (same positions, same ens_lerp, rounded to fp32).
//   Every float is evaluated in fp64 on the fp32 inputs and rounded to fp32 once.
// Hand-over: five 4-byte words per element (crps, sqerr, var, rank, covered bits), in the caller's arrays where given, else in the
// workspace.
// Stage 2 (ens_score_fold, ens_score_sample_sum): a lane owns one cell (position inside a sample) and walks the B samples in
//   ascending order: the cell's fp64 sums are ADDED ONTO the accumulators in memory (so the order of additions over several calls
//   is the order of the samples, whatever the batch size), a wave's 64 values of sample b are summed by a shuffle tree and written
//   as one partial, ranks and covered bits go to an LDS histogram and from there with one 64-bit integer atomic per non-empty bin
//   to memory.  ens_score_sample_sum adds a sample's partials in a fixed order.  No floating-point atomics: same bits every call.
#include "ensemble_common.h"
#include "prof.h"

#pragma clang fp contract(off)

namespace {

struct EnsScoreIn {
    const float* obs;
    const float* scale;          // [per] or null
    size_t per;
    unsigned long long elem_offset, seed;
    double pair_div;             // 1 / c above: K^2 or K (K - 1) (K = 1: 1, the pair term is 0 there)
};
struct EnsScoreOut {
    float *crps, *sqerr, *var;
    int* rank;
    unsigned* cov;
};

__device__ __forceinline__ int ens_tie(unsigned long long seed, unsigned long long g, int equal) {
    unsigned long long z = seed + 0x9E3779B97F4A7C15ull * (g + 1ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    z = z ^ (z >> 31);
    return (int)(((z >> 32) * (unsigned long long)(equal + 1)) >> 32);
}

// what stage 1 knows of an element once its K values have been walked in member order
struct EnsElem {
    double y, sum_abs, mean, m2;
    int below, equal;
    bool valid;
};

__device__ __forceinline__ void ens_finish(const EnsElem& el, double pair, unsigned cov, int K, const EnsScoreIn& in, size_t e,
                                           size_t cell, float& crps, float& sqerr, float& var, int& rank, unsigned& covbits) {
    bool ok = el.valid;
    double sc = 1.0;
    if (in.scale) {
        const float s = in.scale[cell];
        ok = ok && ens_finite(s) && s > 0.f;
        sc = (double)s;
    }
    const double err = el.mean - el.y;
    const double c = (el.sum_abs / (double)K - pair / in.pair_div) * sc;       // (a division: sum / K == pair / pairs stays exactly 0)
    const double v = K > 1 ? el.m2 / (double)(K - 1) : 0.0;
    crps = ok ? (float)c : ens_nan();
    sqerr = ok ? (float)(err * err * (sc * sc)) : ens_nan();
    var = ok ? (float)(v * (sc * sc)) : ens_nan();
    rank = ok ? el.below + ens_tie(in.seed, in.elem_offset + e, el.equal) : -1;
    covbits = ok ? cov : 0u;
}

// ------------------------------------------------------------------------------------------------ K <= 64: registers
template <int KP, int VEC, bool FULL>
__global__ void __launch_bounds__(ENS_THREADS) ensemble_score_reg(const float* __restrict__ members, int K, size_t n, size_t stride,
                                                                  EnsScoreIn in, EnsQ q, int nq, EnsScoreOut out) {
    const size_t blk = (size_t)blockIdx.x * (ENS_THREADS * VEC);
    const unsigned off = threadIdx.x * VEC;
    if (blk + off >= n) return;
    float v[KP][VEC];
    ens_load<KP, VEC, FULL>(members + blk, off, K, stride, v);
    const size_t e0 = blk + off;
    float y[VEC];
    ens_load_vec<VEC>(in.obs + e0, y);

    EnsElem el[VEC];
#pragma unroll
    for (int c = 0; c < VEC; ++c) {
        const float yf = y[c];
        const double yd = (double)yf;
        double s = 0.0, sa = 0.0;
        int below = 0, equal = 0;
        bool fin = ens_finite(yf);
#pragma unroll
        for (int k = 0; k < KP; ++k) {          // (uniform selects, no control flow: the values stay in registers)
            const bool inr = FULL || k < K;
            const float x = v[k][c];
            const double s1 = s + (double)x;
            const double a1 = sa + __builtin_fabs((double)x - yd);
            s = inr ? s1 : s;
            sa = inr ? a1 : sa;
            below += (inr && x < yf) ? 1 : 0;
            equal += (inr && x == yf) ? 1 : 0;
            fin = fin && (!inr || ens_finite(x));
        }
        const double mean = s / (double)K;
        double m2 = 0.0;
#pragma unroll
        for (int k = 0; k < KP; ++k) m2 = ens_m2_add(m2, v[k][c], mean, FULL || k < K);
        el[c] = EnsElem{yd, sa, mean, m2, below, equal, fin};
    }

    ens_sort_reg<KP, VEC>(v);
    size_t cell = in.scale ? e0 % in.per : 0;
    float r_crps[VEC], r_sq[VEC], r_var[VEC];
    int r_rank[VEC];
    unsigned r_cov[VEC];
#pragma unroll
    for (int c = 0; c < VEC; ++c) {
        double pair = 0.0;
#pragma unroll
        for (int k = 0; k < KP; ++k) {            // the padding (+inf) sits behind the K real values and is never added
            const double p1 = pair + (double)(2 * k - K + 1) * ((double)v[k][c] - el[c].y);
            pair = (FULL || k < K) ? p1 : pair;
        }
        unsigned cov = 0u;
        for (int j = 0; j < nq; ++j) {
            float a, b;
            ens_pick<KP, VEC>(v, c, q.lo[j], q.hi[j], a, b);
            const float Q = (float)ens_lerp(a, b, q.t[j]);
            cov |= (y[c] <= Q) ? (1u << j) : 0u;
        }
        ens_finish(el[c], pair, cov, K, in, e0 + c, cell, r_crps[c], r_sq[c], r_var[c], r_rank[c], r_cov[c]);
        cell = cell + 1 >= in.per ? 0 : cell + 1;
    }
    ens_store<VEC, float>(out.crps + e0, r_crps);
    ens_store<VEC, float>(out.sqerr + e0, r_sq);
    ens_store<VEC, float>(out.var + e0, r_var);
    ens_store<VEC, int>(out.rank + e0, r_rank);
    ens_store<VEC, unsigned>(out.cov + e0, r_cov);
}

// ------------------------------------------------------------------------------------------------ 64 < K <= 256: LDS columns
__global__ void __launch_bounds__(ENS_STAGED_THREADS) ensemble_score_staged(const float* __restrict__ members, int K, int KP, size_t n,
                                                                            size_t stride, EnsScoreIn in, EnsQ q, int nq,
                                                                            EnsScoreOut out) {
    extern __shared__ float col[];            // [KP][64]
    const int lane = threadIdx.x;
    const size_t e = (size_t)blockIdx.x * ENS_STAGED_THREADS + lane;
    if (e >= n) return;                       // (no barrier below: a lane only ever touches its own column)
    float* s = col + lane;
    const float yf = in.obs[e];
    EnsElem el{(double)yf, 0.0, 0.0, 0.0, 0, 0, ens_finite(yf)};
    double sum = 0.0;
    for (int k = 0; k < K; ++k) {
        const float x = members[(size_t)k * stride + e];
        s[k * ENS_STAGED_THREADS] = x;
        sum += (double)x;
        el.sum_abs += __builtin_fabs((double)x - el.y);
        el.below += x < yf ? 1 : 0;
        el.equal += x == yf ? 1 : 0;
        el.valid = el.valid && ens_finite(x);
    }
    for (int k = K; k < KP; ++k) s[k * ENS_STAGED_THREADS] = __builtin_inff();
    el.mean = sum / (double)K;
    el.m2 = ens_m2_column(s, K, el.mean);
    ens_sort_column(s, KP);
    double pair = 0.0;
    for (int k = 0; k < K; ++k) pair += (double)(2 * k - K + 1) * ((double)s[k * ENS_STAGED_THREADS] - el.y);
    unsigned cov = 0u;
    for (int j = 0; j < nq; ++j) {
        const float Q = (float)ens_lerp(s[q.lo[j] * ENS_STAGED_THREADS], s[q.hi[j] * ENS_STAGED_THREADS], q.t[j]);
        cov |= (yf <= Q) ? (1u << j) : 0u;
    }
    ens_finish(el, pair, cov, K, in, e, in.scale ? e % in.per : 0, out.crps[e], out.sqerr[e], out.var[e], out.rank[e], out.cov[e]);
}

// ------------------------------------------------------------------------------------------------ stage 2
constexpr int FOLD_THREADS = 256, FOLD_WAVES = FOLD_THREADS / 64;

__global__ void __launch_bounds__(FOLD_THREADS) ens_score_fold(EnsScoreOut f, size_t per, int B, int K, int nq, double* cell_acc,
                                                               double* partial, size_t n_part, unsigned long long* rank_hist,
                                                               unsigned long long* covered) {
    __shared__ unsigned hist[ENS_MAX_MEMBERS + 1 + ENS_MAX_QUANTILES];
    const int bins = K + 1 + nq;
    for (int i = threadIdx.x; i < bins; i += FOLD_THREADS) hist[i] = 0u;
    __syncthreads();
    const size_t c = (size_t)blockIdx.x * FOLD_THREADS + threadIdx.x;
    const bool act = c < per;
    const size_t part = (size_t)blockIdx.x * FOLD_WAVES + threadIdx.x / 64;        // < n_part (the host sized it so)
    double a[4] = {0.0, 0.0, 0.0, 0.0};
    if (act && cell_acc) {
#pragma unroll
        for (int i = 0; i < 4; ++i) a[i] = cell_acc[(size_t)i * per + c];
    }
    for (int b = 0; b < B; ++b) {
        double p[4] = {0.0, 0.0, 0.0, 0.0};
        if (act) {
            const size_t e = (size_t)b * per + c;
            const int r = f.rank[e];
            if (r >= 0) {
                p[0] = (double)f.crps[e];
                p[1] = (double)f.sqerr[e];
                p[2] = (double)f.var[e];
                p[3] = 1.0;
                if (rank_hist) atomicAdd(&hist[r], 1u);
                if (covered)
                    for (unsigned cv = f.cov[e]; cv; cv &= cv - 1u) atomicAdd(&hist[K + 1 + (__ffs((int)cv) - 1)], 1u);
            }
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            a[i] += p[i];                       // (+ 0.0 for an invalid element: the sum's bits do not change)
            if (partial) {
                const double w = wave_sum(p[i]);
                if ((threadIdx.x & 63) == 0) partial[((size_t)b * n_part + part) * 4 + i] = w;
            }
        }
    }
    if (act && cell_acc) {
#pragma unroll
        for (int i = 0; i < 4; ++i) cell_acc[(size_t)i * per + c] = a[i];
    }
    __syncthreads();
    for (int i = threadIdx.x; i < bins; i += FOLD_THREADS) {
        const unsigned h = hist[i];
        if (!h) continue;
        if (i <= K) {
            if (rank_hist) atomicAdd(&rank_hist[i], (unsigned long long)h);
        } else if (covered) {
            atomicAdd(&covered[i - K - 1], (unsigned long long)h);
        }
    }
}

// sample_out[b][i] = sum of the sample's n_part partials: strided per thread, then a fixed tree through LDS
__global__ void __launch_bounds__(FOLD_THREADS) ens_score_sample_sum(const double* __restrict__ partial, size_t n_part,
                                                                     double* __restrict__ sample_out) {
    __shared__ double red[FOLD_THREADS][4];
    const size_t b = blockIdx.x;
    double a[4] = {0.0, 0.0, 0.0, 0.0};
    for (size_t w = threadIdx.x; w < n_part; w += FOLD_THREADS) {
#pragma unroll
        for (int i = 0; i < 4; ++i) a[i] += partial[(b * n_part + w) * 4 + i];
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) red[threadIdx.x][i] = a[i];
    __syncthreads();
    for (int d = FOLD_THREADS / 2; d > 0; d >>= 1) {
        if ((int)threadIdx.x < d) {
#pragma unroll
            for (int i = 0; i < 4; ++i) red[threadIdx.x][i] += red[threadIdx.x + d][i];
        }
        __syncthreads();
    }
    if (threadIdx.x < 4) sample_out[b * 4 + threadIdx.x] = red[0][threadIdx.x];
}

size_t padded(size_t n) { return (n + 3) / 4 * 4; }                 // every field of the workspace starts 16-byte aligned
size_t n_partials(size_t per) { return cdivz(per, FOLD_THREADS) * FOLD_WAVES; }

}  // namespace

size_t ensemble_score_workspace_bytes(size_t n, size_t B) {
    if (n == 0 || B == 0) return 0;
    return 5 * padded(n) * sizeof(float) + B * n_partials(n / B) * 4 * sizeof(double);
}

void ensemble_score(hipStream_t s, const float* members, size_t K, size_t n, size_t member_stride, const float* obs, size_t B,
                    unsigned long long elem_offset, const float* scale, int fair, unsigned long long seed, const float* q_host, int nq,
                    float* crps, float* sqerr, float* var, int* rank, double* sample_out, double* cell_acc,
                    unsigned long long* rank_hist, unsigned long long* covered, void* workspace, size_t workspace_bytes) {
    DL4DS_REQUIRE(K >= 1 && K <= ENS_MAX_MEMBERS, "ensemble_score: 1 <= K <= 256 members");
    DL4DS_REQUIRE(nq >= 0 && nq <= ENS_MAX_QUANTILES, "ensemble_score: at most 32 quantiles per call");
    DL4DS_REQUIRE(nq == 0 || q_host, "ensemble_score: nq > 0 without probabilities");
    DL4DS_REQUIRE(nq == 0 || covered, "ensemble_score: nq > 0 without covered counts");
    const EnsQ q = ens_positions("ensemble_score", K, q_host, nq);
    if (n == 0) return;
    DL4DS_REQUIRE(B >= 1 && n % B == 0, "ensemble_score: n must be B whole samples");
    DL4DS_REQUIRE(B <= 0x7fffffffull, "ensemble_score: too many samples for one call");
    const size_t per = n / B;
    DL4DS_REQUIRE(elem_offset % per == 0, "ensemble_score: elem_offset must be a whole number of samples");
    DL4DS_REQUIRE(members && obs, "ensemble_score: null member stack or observation");
    DL4DS_REQUIRE(member_stride >= n, "ensemble_score: member stride smaller than the member");
    DL4DS_REQUIRE(workspace && workspace_bytes >= ensemble_score_workspace_bytes(n, B), "ensemble_score: workspace too small");
    float* ws = static_cast<float*>(workspace);
    const size_t np = padded(n);
    const EnsScoreOut out{crps ? crps : ws, sqerr ? sqerr : ws + np, var ? var : ws + 2 * np,
                          rank ? rank : reinterpret_cast<int*>(ws + 3 * np), reinterpret_cast<unsigned*>(ws + 4 * np)};
    double* partial = reinterpret_cast<double*>(ws + 5 * np);
    const int k = (int)K;
    const double pairs = fair ? (double)K * (double)(K - 1) : (double)K * (double)K;
    const EnsScoreIn in{obs, scale, per, elem_offset, seed, K > 1 ? pairs : 1.0};
    ProfScope ps(s, "ensemble_score", (double)n * (6.0 * K), (double)n * 4.0 * (double)(K + 1 + 5 + 5));
    ens_launch(
        "ensemble_score", k, n, member_stride, {members, obs, out.crps, out.sqerr, out.var, out.rank, out.cov},
        [&](auto KP, auto VEC, auto FULL, dim3 grid) {
            DL4DS_LAUNCH((ensemble_score_reg<decltype(KP)::value, decltype(VEC)::value, decltype(FULL)::value>), grid,
                         dim3(ENS_THREADS), 0, s, members, k, n, member_stride, in, q, nq, out);
        },
        [&](int kp, dim3 grid, size_t lds) {
            DL4DS_LAUNCH(ensemble_score_staged, grid, dim3(ENS_STAGED_THREADS), lds, s, members, k, kp, n,
                         member_stride, in, q, nq, out);
        });
    HIP_CHECK(hipGetLastError());
    if (!sample_out && !cell_acc && !rank_hist && !covered) return;
    const size_t n_part = n_partials(per);
    DL4DS_REQUIRE(cdivz(per, FOLD_THREADS) <= 0x7fffffffull, "ensemble_score: too many cells for one launch");
    DL4DS_LAUNCH(ens_score_fold, dim3((unsigned)cdivz(per, FOLD_THREADS)), dim3(FOLD_THREADS), 0, s, out, per, (int)B, k,
                 covered ? nq : 0, cell_acc, sample_out ? partial : nullptr, n_part, rank_hist, covered);
    if (sample_out)
        DL4DS_LAUNCH(ens_score_sample_sum, dim3((unsigned)B), dim3(FOLD_THREADS), 0, s, partial, n_part, sample_out);
    HIP_CHECK(hipGetLastError());
}
