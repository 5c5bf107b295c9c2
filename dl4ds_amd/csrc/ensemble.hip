// Member statistics of an MC-dropout ensemble (the MCDropout / MCGaussianDropout / MCSpatialDropout layers of blocks.py:658-676 stay
// active at inference so that K forward passes form an ensemble): ONE read of the member stack members[K][n] gives, per element,
// mean, population std, min, max and nq linearly interpolated quantiles.  DESIGN.md section 12.
//
// A thread owns VEC consecutive elements and holds all K values of each in registers: KP * VEC floats, KP = K rounded up to a power
// of two (missing rows are +inf, which a sort leaves behind the K real values).  VEC shrinks as K grows so that the live set stays at
// 64 data registers: K <= 16: 4 elements (16-byte loads per member row), K <= 32: 2, K <= 64: 1, and every load of a thread (up to
// 64) is issued before the first use.
// K in 65 ... 256 takes the staged kernel: a wave keeps the K values of 64 elements in LDS (one column per lane: conflict-free),
// each lane sorts its own column in place with a looped bitonic network.  Only correctness is asked of that path.
//
// Arithmetic (what numpy does on the fp64 copy of the stack, np.mean / np.std / np.min / np.max / np.quantile along axis 0):
//   mean  = (sum_k x_k) / K, std = sqrt((sum_k (x_k - mean)^2) / K): sequential fp64 sums in member order, product and sum rounded
//           separately, ONE rounding to fp32 at the end.  No state in memory, no atomics: a repeated call gives the same bits.
//   quantile q: pos = (K - 1) q.  pos >= K - 1: a = b = the largest value, t = pos + 1; else a, b = order statistics floor(pos) and
//           floor(pos) + 1, t = pos - floor(pos).  d = b - a; result = t >= 0.5 ? b - d (1 - t) : a + d t, in fp64 on the two fp32
//           values, rounded once.  (numpy's _lerp: the second form is what decides between inf and NaN next to an infinite value.)
//   A NaN among the K values makes every output of that element NaN; infinities give what the formulas give (std NaN).
#include "ensemble_common.h"
#include "prof.h"

// numpy rounds (x - mean)^2 and the running sum separately, and d * t and the sum of the interpolation too
#pragma clang fp contract(off)

namespace {

struct EnsOut { float *mean, *std, *mn, *mx, *quant; };

// ------------------------------------------------------------------------------------------------ K <= 64: registers
// (KP, VEC, FULL) and what the host guarantees for VEC > 1: ens_launch.
template <int KP, int VEC, bool FULL>
__global__ void __launch_bounds__(ENS_THREADS) ensemble_reduce_reg(const float* __restrict__ members, int K, size_t n, size_t stride,
                                                                   EnsQ q, int nq, EnsOut out) {
    const size_t blk = (size_t)blockIdx.x * (ENS_THREADS * VEC);       // uniform: the row pointers stay scalar,
    const unsigned off = threadIdx.x * VEC;                             // the lane's part is one 32-bit offset
    if (blk + off >= n) return;
    float v[KP][VEC];
    // branch-free: every row's load is issued before anything is used (ens_load)
    ens_load<KP, VEC, FULL>(members + blk, off, K, stride, v);

    float r_mean[VEC], r_std[VEC], r_mn[VEC], r_mx[VEC];
    bool isnan_[VEC];
#pragma unroll
    for (int c = 0; c < VEC; ++c) {
        double s = 0.0;
        float mn = v[0][c], mx = v[0][c];
        bool bad = false;
#pragma unroll
        for (int k = 0; k < KP; ++k) {          // (uniform selects, no control flow: the values stay in registers)
            const bool in = FULL || k < K;
            const float x = v[k][c];
            const double s1 = s + (double)x;
            s = in ? s1 : s;
            mn = (in && x < mn) ? x : mn;
            mx = (in && x > mx) ? x : mx;
            bad = bad || (x != x);                // (the padding is +inf, never NaN)
        }
        const double mean = s / (double)K;
        double m2 = 0.0;
#pragma unroll
        for (int k = 0; k < KP; ++k) m2 = ens_m2_add(m2, v[k][c], mean, FULL || k < K);
        isnan_[c] = bad;
        r_mean[c] = bad ? ens_nan() : (float)mean;
        r_std[c] = bad ? ens_nan() : (float)sqrt(m2 / (double)K);
        r_mn[c] = bad ? ens_nan() : mn;
        r_mx[c] = bad ? ens_nan() : mx;
    }
    const size_t e0 = blk + off;
    ens_store<VEC, float>(out.mean ? out.mean + e0 : nullptr, r_mean);
    ens_store<VEC, float>(out.std ? out.std + e0 : nullptr, r_std);
    ens_store<VEC, float>(out.mn ? out.mn + e0 : nullptr, r_mn);
    ens_store<VEC, float>(out.mx ? out.mx + e0 : nullptr, r_mx);

    if (nq <= 0) return;
    ens_sort_reg<KP, VEC>(v);
    for (int j = 0; j < nq; ++j) {
        const int lo = q.lo[j], hi = q.hi[j];
        const double t = q.t[j];
        float r[VEC];
#pragma unroll
        for (int c = 0; c < VEC; ++c) {
            float a, b;
            ens_pick<KP, VEC>(v, c, lo, hi, a, b);
            r[c] = isnan_[c] ? ens_nan() : (float)ens_lerp(a, b, t);
        }
        ens_store<VEC, float>(out.quant + (size_t)j * n + e0, r);
    }
}

// ------------------------------------------------------------------------------------------------ 64 < K <= 256: LDS columns
__global__ void __launch_bounds__(ENS_STAGED_THREADS) ensemble_reduce_staged(const float* __restrict__ members, int K, int KP, size_t n,
                                                                             size_t stride, EnsQ q, int nq, EnsOut out) {
    extern __shared__ float col[];            // [KP][64]
    const int lane = threadIdx.x;
    const size_t e = (size_t)blockIdx.x * ENS_STAGED_THREADS + lane;
    if (e >= n) return;                       // (no barrier below: a lane only ever touches its own column)
    float* s = col + lane;
    double sum = 0.0;
    float mn = __builtin_inff(), mx = -__builtin_inff();
    bool bad = false;
    for (int k = 0; k < K; ++k) {
        const float x = members[(size_t)k * stride + e];
        s[k * ENS_STAGED_THREADS] = x;
        sum += (double)x;
        mn = x < mn ? x : mn;
        mx = x > mx ? x : mx;
        bad = bad || (x != x);
    }
    for (int k = K; k < KP; ++k) s[k * ENS_STAGED_THREADS] = __builtin_inff();
    const double mean = sum / (double)K;
    const double m2 = ens_m2_column(s, K, mean);
    if (out.mean) out.mean[e] = bad ? ens_nan() : (float)mean;
    if (out.std) out.std[e] = bad ? ens_nan() : (float)sqrt(m2 / (double)K);
    if (out.mn) out.mn[e] = bad ? ens_nan() : mn;
    if (out.mx) out.mx[e] = bad ? ens_nan() : mx;
    if (nq <= 0 || !out.quant) return;
    ens_sort_column(s, KP);
    for (int j = 0; j < nq; ++j) {
        const float a = s[q.lo[j] * ENS_STAGED_THREADS], b = s[q.hi[j] * ENS_STAGED_THREADS];
        out.quant[(size_t)j * n + e] = bad ? ens_nan() : (float)ens_lerp(a, b, q.t[j]);
    }
}

}  // namespace

void ensemble_reduce(hipStream_t s, const float* members, size_t K, size_t n, size_t member_stride, const float* q_host, int nq,
                     float* mean, float* std_, float* mn, float* mx, float* quant) {
    DL4DS_REQUIRE(K >= 1 && K <= ENS_MAX_MEMBERS, "ensemble_reduce: 1 <= K <= 256 members");
    DL4DS_REQUIRE(nq >= 0 && nq <= ENS_MAX_QUANTILES, "ensemble_reduce: at most 32 quantiles per call");
    DL4DS_REQUIRE(nq == 0 || q_host, "ensemble_reduce: nq > 0 without probabilities");
    if (n == 0) return;
    DL4DS_REQUIRE(members, "ensemble_reduce: null member stack");
    DL4DS_REQUIRE(member_stride >= n, "ensemble_reduce: member stride smaller than the member");
    const EnsQ q = ens_positions("ensemble_reduce", K, q_host, nq);
    if (!quant) nq = 0;
    const EnsOut out{mean, std_, mn, mx, quant};
    const int k = (int)K;
    ProfScope ps(s, "ensemble_reduce", (double)n * (4.0 * K), (double)n * 4.0 * (double)(K + 4 + nq));
    ens_launch(
        "ensemble_reduce", k, n, member_stride, {members, mean, std_, mn, mx, quant},
        [&](auto KP, auto VEC, auto FULL, dim3 grid) {
            DL4DS_LAUNCH((ensemble_reduce_reg<decltype(KP)::value, decltype(VEC)::value, decltype(FULL)::value>), grid,
                         dim3(ENS_THREADS), 0, s, members, k, n, member_stride, q, nq, out);
        },
        [&](int kp, dim3 grid, size_t lds) {
            DL4DS_LAUNCH(ensemble_reduce_staged, grid, dim3(ENS_STAGED_THREADS), lds, s, members, k, kp, n,
                         member_stride, q, nq, out);
        });
    HIP_CHECK(hipGetLastError());
}
