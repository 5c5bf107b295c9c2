// The optimiser's extensions on the flat fp32 arenas: clipping by the global gradient norm (Keras global_clipnorm =
// tf.clip_by_global_norm), decoupled weight decay (Keras weight_decay / AdamW: _apply_weight_decay, before the gradient update) and
// an exponential moving average of the weights (Keras use_ema / ema_momentum).  adam.hip stays what it was; trainer_apply_adam comes
// here only when one of the three is on.  At most two launches per optimiser step, no host synchronisation, no atomics:
//   1. sqnorm_partials_kernel (clipping on only): reads g once, squares and accumulates in fp64 (the product of two fp32 values is
//      exact in fp64), one fp64 partial per block.  The block count depends on n alone (sqnorm_blocks), never on the device, and every
//      sum runs in a fixed order: the norm is bit-reproducible from run to run and the same on every rank of a data-parallel job.
//   2. adam_ext_kernel: every block sums the partials (at most SQNORM_BLOCK_CAP, from L2) in the same fixed order, forms
//      norm = fl32(grad_scale * sqrt(sum)) and c = clip / max(norm, clip) (== 1.0f exactly whenever norm <= clip), then per element
//        [decayed]  w <- w - (lr * wd) * w                      (the plain scheduled lr, not the bias-corrected one)
//                   adam.hip's expressions on gr = g * fl32(grad_scale * c)
//        [EMA]      ema <- mu * ema + (1 - mu) * w_new
//      and block 0 leaves norm, c and the running count of skipped steps in three device words.
// A norm that is not finite SKIPS the step: every block leaves w, m, v and ema untouched and block 0 counts it (TensorFlow would turn
// every gradient, and with it every weight, into NaN).  The sticky device error word is honoured as in adam_kernel, in both launches.
//
// The decayed set is a sorted table of element bounds b0 < e0 < b1 < e1 < ... (ranges [b_k, e_k), merged where they touch; any
// element may start or end one).  Element i is decayed iff the number of bounds <= i is odd: one binary search of the table (16 B per
// range, L1/L2-resident) per float4, then a walk over its four elements.
// Bytes per parameter: norm 4 read; update 16 read + 12 written as plain Adam, + 4 read + 4 written with the average.
#include "ops.h"
#include "prof.h"
#include <algorithm>
#include <vector>

namespace {
constexpr int SQNORM_THREADS = 256;
constexpr int SQNORM_BLOCK_CAP = 1024;

__global__ void __launch_bounds__(SQNORM_THREADS) sqnorm_partials_kernel(const float* __restrict__ g, size_t n,
                                                                         double* __restrict__ partials, const unsigned* err) {
    if (err && __builtin_nontemporal_load(err) != 0u) return;
    __shared__ double ws[SQNORM_THREADS / 64];
    const size_t n4 = n >> 2;
    const float4* g4 = reinterpret_cast<const float4*>(g);
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    double acc = 0.0;
    for (size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x; e < n4; e += stride) {
        const float4 gg = g4[e];
        const double x = gg.x, y = gg.y, z = gg.z, w = gg.w;
        acc += x * x; acc += y * y; acc += z * z; acc += w * w;
    }
    for (size_t e = (n4 << 2) + (size_t)blockIdx.x * blockDim.x + threadIdx.x; e < n; e += stride) {
        const double x = g[e];
        acc += x * x;
    }
    acc = wave_sum(acc);
    if ((threadIdx.x & 63) == 0) ws[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) {
        double s = ws[0];
        for (int k = 1; k < SQNORM_THREADS / 64; ++k) s += ws[k];
        partials[blockIdx.x] = s;
    }
}

// number of table bounds <= i
__device__ inline int bounds_le(const size_t* __restrict__ tab, int nb, size_t i) {
    int lo = 0, hi = nb;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (tab[mid] <= i) lo = mid + 1; else hi = mid;
    }
    return lo;
}

struct AdamExtArgs {
    float lr_t, b1, b2, eps, gs;
    float clip;                    // 0: no clipping (no partials are read, c = 1)
    float lr_wd;                   // lr * weight_decay; the table decides where it applies
    float mu;                      // read only where ema != nullptr
    int n_partials;
    int n_bounds;                  // 0: nothing is decayed
};

__global__ void __launch_bounds__(256) adam_ext_kernel(float* __restrict__ w, const float* __restrict__ g, float* __restrict__ m,
                                                       float* __restrict__ v, float* __restrict__ ema, size_t n, AdamExtArgs a,
                                                       const double* __restrict__ partials, const size_t* __restrict__ tab,
                                                       float* __restrict__ stats, const unsigned* err) {
    // Contraction is spelled out here, not left to the compiler: with everything off (and with c == 1) the results must be
    // adam_kernel's bit for bit, and what hipcc makes of adam_kernel's expressions is m' = fma(1 - b1, gr, b1 m) and
    // v' = fma(gr, (1 - b2) gr, b2 v) in the float4 body, and separate multiplications and additions in the scalar tail (its packed
    // tail code has no fused form).  tests/test_gpu_optimizer.py compares the two kernels at every size.
#pragma clang fp contract(off)
    if (err && __builtin_nontemporal_load(err) != 0u) return;
    __shared__ float s_norm;
    float norm = 0.f, c = 1.f;
    if (a.clip > 0.f) {
        // the same fixed order in every block: lane l takes partials l, l + 64, ... in turn, then the wave tree
        if (threadIdx.x < 64) {
            double s = 0.0;
            for (int k = threadIdx.x; k < a.n_partials; k += 64) s += partials[k];
            s = wave_sum(s);
            if (threadIdx.x == 0) s_norm = (float)((double)a.gs * sqrt(s));
        }
        __syncthreads();
        norm = s_norm;
        const bool finite = fabsf(norm) <= 3.402823466e+38f;          // false for Inf and NaN
        if (!finite) {
            if (blockIdx.x == 0 && threadIdx.x == 0) {
                stats[0] = norm; stats[1] = 0.f;
                reinterpret_cast<unsigned*>(stats)[2] += 1u;
            }
            return;
        }
        c = a.clip / fmaxf(norm, a.clip);
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) { stats[0] = norm; stats[1] = c; }
    // grad_scale and c reach the gradient as ONE fp32 factor: gr = g * fl32(grad_scale * c) is a single rounding per element, and with
    // c == 1 the expressions below are adam_kernel's, operand for operand (the results are then the same bits)
    const float lr_t = a.lr_t, b1 = a.b1, b2 = a.b2, eps = a.eps, gs = a.gs * c, lr_wd = a.lr_wd, mu = a.mu;
    const size_t n4 = n >> 2;
    float4* w4 = reinterpret_cast<float4*>(w);
    const float4* g4 = reinterpret_cast<const float4*>(g);
    float4* m4 = reinterpret_cast<float4*>(m);
    float4* v4 = reinterpret_cast<float4*>(v);
    float4* e4 = reinterpret_cast<float4*>(ema);
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    for (size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x; e < n4; e += stride) {
        float4 ww = w4[e], gg = g4[e], mm = m4[e], vv = v4[e];
        int nb = a.n_bounds ? bounds_le(tab, a.n_bounds, e << 2) : 0;
#define ADAM1(c_, k_)                                                          \
    {                                                                          \
        while (nb < a.n_bounds && tab[nb] <= (e << 2) + k_) ++nb;              \
        if (nb & 1) ww.c_ -= lr_wd * ww.c_;                                    \
        const float gr = gg.c_ * gs;                                           \
        mm.c_ = __builtin_fmaf(1.f - b1, gr, b1 * mm.c_);                      \
        vv.c_ = __builtin_fmaf(gr, (1.f - b2) * gr, b2 * vv.c_);               \
        ww.c_ -= lr_t * mm.c_ / (sqrtf(vv.c_) + eps);                          \
    }
        ADAM1(x, 0) ADAM1(y, 1) ADAM1(z, 2) ADAM1(w, 3)
#undef ADAM1
        w4[e] = ww; m4[e] = mm; v4[e] = vv;
        if (ema) {
            float4 ee = e4[e];
            ee.x = mu * ee.x + (1.f - mu) * ww.x;
            ee.y = mu * ee.y + (1.f - mu) * ww.y;
            ee.z = mu * ee.z + (1.f - mu) * ww.z;
            ee.w = mu * ee.w + (1.f - mu) * ww.w;
            e4[e] = ee;
        }
    }
    for (size_t e = (n4 << 2) + (size_t)blockIdx.x * blockDim.x + threadIdx.x; e < n; e += stride) {
        float ww = w[e];
        if (a.n_bounds && (bounds_le(tab, a.n_bounds, e) & 1)) ww -= lr_wd * ww;
        const float gr = g[e] * gs;
        const float mm = b1 * m[e] + (1.f - b1) * gr;
        const float vv = b2 * v[e] + (1.f - b2) * gr * gr;
        m[e] = mm; v[e] = vv;
        ww -= lr_t * mm / (sqrtf(vv) + eps);
        w[e] = ww;
        if (ema) ema[e] = mu * ema[e] + (1.f - mu) * ww;
    }
}

__global__ void __launch_bounds__(256) arena_swap_kernel(float* __restrict__ a, float* __restrict__ b, size_t n) {
    const size_t n4 = n >> 2;
    float4* a4 = reinterpret_cast<float4*>(a);
    float4* b4 = reinterpret_cast<float4*>(b);
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    for (size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x; e < n4; e += stride) {
        const float4 x = a4[e], y = b4[e];
        a4[e] = y; b4[e] = x;
    }
    for (size_t e = (n4 << 2) + (size_t)blockIdx.x * blockDim.x + threadIdx.x; e < n; e += stride) {
        const float x = a[e], y = b[e];
        a[e] = y; b[e] = x;
    }
}
}  // namespace

int sqnorm_blocks(size_t n) { return (int)std::max<size_t>(1, std::min<size_t>(cdivz(n / 4 + 1, 256), 1024)); }
static_assert(SQNORM_THREADS == 256 && SQNORM_BLOCK_CAP == 1024, "sqnorm_blocks restates these figures");

std::vector<size_t> decay_bounds(const size_t* ranges, int n_ranges, size_t n) {
    std::vector<std::pair<size_t, size_t>> r;
    for (int k = 0; k < n_ranges; ++k) {
        const size_t b = ranges[2 * k], e = ranges[2 * k + 1];
        DL4DS_REQUIRE(b <= e && e <= n, "decay range outside the arena (or begin > end)");
        if (b < e) r.push_back({b, e});
    }
    std::sort(r.begin(), r.end());
    std::vector<size_t> out;
    for (const auto& p : r) {
        if (!out.empty() && p.first <= out.back()) out.back() = std::max(out.back(), p.second);     // touching or overlapping
        else { out.push_back(p.first); out.push_back(p.second); }
    }
    return out;
}

void adam_ext_update(hipStream_t s, float* w, const float* g, float* m, float* v, float* ema, size_t n, float lr_t, float beta1,
                     float beta2, float eps, float grad_scale, float clipnorm, float lr, float weight_decay, const size_t* bounds_dev,
                     int n_bounds, float ema_momentum, double* partials_dev, float* stats_dev, const unsigned* err_word) {
    if (n == 0) return;
    DL4DS_REQUIRE(stats_dev, "adam_ext: the three statistics words are required");
    DL4DS_REQUIRE(!(clipnorm > 0.f) || partials_dev, "adam_ext: clipping needs the partial-sum buffer");
    AdamExtArgs a;
    a.lr_t = lr_t; a.b1 = beta1; a.b2 = beta2; a.eps = eps; a.gs = grad_scale;
    a.clip = clipnorm > 0.f ? clipnorm : 0.f;
    a.lr_wd = lr * weight_decay;
    a.mu = ema_momentum;
    a.n_partials = 0;
    a.n_bounds = (weight_decay > 0.f && bounds_dev) ? n_bounds : 0;
    if (a.clip > 0.f) {
        a.n_partials = sqnorm_blocks(n);
        ProfScope ps(s, "adam_norm", 0.0, 4.0 * (double)n);
        DL4DS_LAUNCH(sqnorm_partials_kernel, dim3(a.n_partials), dim3(SQNORM_THREADS), 0, s, g, n, partials_dev, err_word);
        HIP_CHECK(hipGetLastError());
    }
    ProfScope ps(s, "adam_ext", 0.0, (ema ? 36.0 : 28.0) * (double)n);
    const int blocks = (int)std::max<size_t>(1, std::min<size_t>(cdivz(n / 4 + 1, 256), 2048));
    DL4DS_LAUNCH(adam_ext_kernel, dim3(blocks), dim3(256), 0, s, w, g, m, v, ema, n, a, (const double*)partials_dev, bounds_dev,
                 stats_dev, err_word);
    HIP_CHECK(hipGetLastError());
}

void arena_swap(hipStream_t s, float* a, float* b, size_t n) {
    if (n == 0) return;
    ProfScope ps(s, "ema_swap", 0.0, 16.0 * (double)n);
    const int blocks = (int)std::max<size_t>(1, std::min<size_t>(cdivz(n / 4 + 1, 256), 2048));
    DL4DS_LAUNCH(arena_swap_kernel, dim3(blocks), dim3(256), 0, s, a, b, n);
    HIP_CHECK(hipGetLastError());
}
