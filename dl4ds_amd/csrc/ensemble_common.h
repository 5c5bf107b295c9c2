// Pieces shared by the per-element kernels over an ensemble's member stack: the member statistics (ensemble.hip) and the
// verification scores (ensemble_score.hip).  Both hold the K values of an element in registers (K <= 64) or in an LDS column
// (K <= 256), sort them with a bitonic network and interpolate np.quantile's 'linear' quantiles between two order statistics.
#pragma once
#include "common.h"
#include "ops.h"
#include <cmath>
#include <cstdint>

constexpr int ENS_THREADS = 256;
constexpr int ENS_STAGED_THREADS = 64;      // one wave: a lane's column is private, no barrier anywhere

// quantile j lies between the order statistics lo[j] and hi[j], at fraction t[j] (ens_positions / ens_lerp)
struct EnsQ {
    int lo[ENS_MAX_QUANTILES], hi[ENS_MAX_QUANTILES];
    double t[ENS_MAX_QUANTILES];
};

// numpy's positions for method='linear': pos = (K - 1) q.  pos >= K - 1: a = b = the largest value, t = pos + 1 (numpy: previous
// index -1, the last element, gamma = pos - (-1)); else the order statistics floor(pos) and floor(pos) + 1, t = pos - floor(pos).
inline EnsQ ens_positions(const char* who, size_t K, const float* q_host, int nq) {
    EnsQ q{};
    for (int j = 0; j < nq; ++j) {
        const double p = (double)q_host[j];
        if (!(p >= 0.0 && p <= 1.0)) throw Dl4dsError(std::string("dl4ds: ") + who + ": quantile probabilities must be in [0, 1]");
        const double pos = (double)(K - 1) * p;
        if (pos >= (double)(K - 1)) {
            q.lo[j] = q.hi[j] = (int)K - 1;
            q.t[j] = pos + 1.0;
        } else {
            const double f = std::floor(pos);
            q.lo[j] = (int)f;
            q.hi[j] = (int)f + 1;
            q.t[j] = pos - f;
        }
    }
    return q;
}

__device__ __forceinline__ float ens_nan() { return __builtin_nanf(""); }

// numpy's _lerp in fp64 on the two fp32 order statistics: the second form is what decides between inf and NaN next to an infinity
__device__ __forceinline__ double ens_lerp(float a, float b, double t) {
    const double da = (double)a, db = (double)b;
    const double d = db - da;
    return t >= 0.5 ? db - d * (1.0 - t) : da + d * t;
}

// VEC results -> p[e0 .. e0 + VEC) as one 4 / 8 / 16-byte store (the host checked alignment and n % VEC == 0); null: skipped
template <int VEC, typename T>
__device__ __forceinline__ void ens_store(T* p, const T (&r)[VEC]) {
    static_assert(sizeof(T) == 4, "4-byte elements");
    if (!p) return;
    if constexpr (VEC == 4) {
        uint4 w;
        __builtin_memcpy(&w, r, 16);
        *reinterpret_cast<uint4*>(p) = w;
    } else if constexpr (VEC == 2) {
        uint2 w;
        __builtin_memcpy(&w, r, 8);
        *reinterpret_cast<uint2*>(p) = w;
    } else {
        p[0] = r[0];
    }
}

// VEC consecutive values of each of the KP rows (row k at row0 + k * stride; rows k >= K re-read row K - 1: a cache hit, no HBM
// traffic, none when FULL) into v, every load issued before anything is used; then rows k >= K become +inf, which a sort leaves
// behind the K real values.
template <int KP, int VEC, bool FULL>
__device__ __forceinline__ void ens_load(const float* row, unsigned off, int K, size_t stride, float (&v)[KP][VEC]) {
#pragma unroll
    for (int k = 0; k < KP; ++k) {
        if constexpr (VEC == 4) {
            const float4 x = *reinterpret_cast<const float4*>(row + off);
            v[k][0] = x.x; v[k][1] = x.y; v[k][2] = x.z; v[k][3] = x.w;
        } else if constexpr (VEC == 2) {
            const float2 x = *reinterpret_cast<const float2*>(row + off);
            v[k][0] = x.x; v[k][1] = x.y;
        } else {
            v[k][0] = row[off];
        }
        row += (FULL || k + 1 < K) ? stride : 0;
    }
    if constexpr (!FULL) {
#pragma unroll
        for (int k = 1; k < KP; ++k) {
#pragma unroll
            for (int c = 0; c < VEC; ++c) v[k][c] = k < K ? v[k][c] : __builtin_inff();
        }
    }
}

// bitonic network on the KP register values of each element: every index is a compile-time constant after unrolling
template <int KP, int VEC>
__device__ __forceinline__ void ens_sort_reg(float (&v)[KP][VEC]) {
#pragma unroll
    for (int size = 2; size <= KP; size <<= 1) {
#pragma unroll
        for (int j = size >> 1; j > 0; j >>= 1) {
#pragma unroll
            for (int i = 0; i < KP; ++i) {
                const int l = i ^ j;
                if (l > i) {
                    const bool up = (i & size) == 0;
#pragma unroll
                    for (int c = 0; c < VEC; ++c) {
                        const float a = v[i][c], b = v[l][c];
                        const float lo = fminf(a, b), hi = fmaxf(a, b);
                        v[i][c] = up ? lo : hi;
                        v[l][c] = up ? hi : lo;
                    }
                }
            }
        }
    }
}

// the two order statistics of quantile (lo, hi) out of the sorted register values (lo, hi are uniform: selects on a scalar
// condition, no indexed register file)
template <int KP, int VEC>
__device__ __forceinline__ void ens_pick(const float (&v)[KP][VEC], int c, int lo, int hi, float& a, float& b) {
    a = v[0][c];
    b = v[0][c];
#pragma unroll
    for (int k = 1; k < KP; ++k) {
        a = k == lo ? v[k][c] : a;
        b = k == hi ? v[k][c] : b;
    }
}

// the looped network of the LDS path: a lane sorts its own column s[k * ENS_STAGED_THREADS], k < KP, in place
__device__ __forceinline__ void ens_sort_column(float* s, int KP) {
    for (int size = 2; size <= KP; size <<= 1)
        for (int j = size >> 1; j > 0; j >>= 1)
            for (int i = 0; i < KP; ++i) {
                const int l = i ^ j;
                if (l > i) {
                    const float a = s[i * ENS_STAGED_THREADS], b = s[l * ENS_STAGED_THREADS];
                    const float lo = fminf(a, b), hi = fmaxf(a, b);
                    const bool up = (i & size) == 0;
                    s[i * ENS_STAGED_THREADS] = up ? lo : hi;
                    s[l * ENS_STAGED_THREADS] = up ? hi : lo;
                }
            }
}
