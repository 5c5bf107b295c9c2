// What the kernels over an ensemble's member stack members[K][n] (row k at members + k * stride) agree on, stated once.
//   ensemble.hip        member statistics: all of it
//   ensemble_score.hip  verification scores: all of it
//   exceedance.hip      exceedance counts: ens_finite, ens_load_vec, ens_store (it sorts nothing and has its own launch shapes)
//   ensemble_multi.hip  energy and variogram scores: ens_finite
// ensemble.hip and ensemble_score.hip hold the K values of an element in registers (K <= 64) or in an LDS column (K <= 256), sort
// them with a bitonic network and interpolate np.quantile's 'linear' quantiles between two order statistics; ens_launch picks the
// instance for both.  (The fp64 wave sum of their folds is common.h's wave_sum, beside wave_sum_u64.)
#pragma once
#include "common.h"
#include "ops.h"
#include <cmath>
#include <cstdint>
#include <initializer_list>
#include <type_traits>

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

__device__ __forceinline__ bool ens_finite(float x) { return __builtin_fabsf(x) < __builtin_inff(); }      // false for NaN

// VEC consecutive floats as one 4 / 8 / 16-byte load (the host checked alignment and n % VEC == 0)
template <int VEC>
__device__ __forceinline__ void ens_load_vec(const float* p, float (&v)[VEC]) {
    if constexpr (VEC == 4) {
        const float4 x = *reinterpret_cast<const float4*>(p);
        v[0] = x.x; v[1] = x.y; v[2] = x.z; v[3] = x.w;
    } else if constexpr (VEC == 2) {
        const float2 x = *reinterpret_cast<const float2*>(p);
        v[0] = x.x; v[1] = x.y;
    } else {
        v[0] = p[0];
    }
}

// VEC results of 2 or 4 bytes each -> p[0 .. VEC) as one store of VEC * sizeof(T) bytes (alignment as above); null: skipped
template <int VEC, typename T>
__device__ __forceinline__ void ens_store(T* p, const T (&r)[VEC]) {
    static_assert(sizeof(T) == 4 || sizeof(T) == 2, "2- or 4-byte elements");
    if (!p) return;
    if constexpr (VEC == 1) {
        p[0] = r[0];
    } else if constexpr (VEC * sizeof(T) == 16) {
        uint4 w;
        __builtin_memcpy(&w, r, 16);
        *reinterpret_cast<uint4*>(p) = w;
    } else if constexpr (VEC * sizeof(T) == 8) {
        uint2 w;
        __builtin_memcpy(&w, r, 8);
        *reinterpret_cast<uint2*>(p) = w;
    } else {
        unsigned w;
        __builtin_memcpy(&w, r, 4);
        *reinterpret_cast<unsigned*>(p) = w;
    }
}

// VEC consecutive values of each of the KP rows (row k at row0 + k * stride; rows k >= K re-read row K - 1: a cache hit, no HBM
// traffic, none when FULL) into v, every load issued before anything is used; then rows k >= K become +inf, which a sort leaves
// behind the K real values.
template <int KP, int VEC, bool FULL>
__device__ __forceinline__ void ens_load(const float* row, unsigned off, int K, size_t stride, float (&v)[KP][VEC]) {
#pragma unroll
    for (int k = 0; k < KP; ++k) {
        ens_load_vec<VEC>(row + off, v[k]);
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

// One member of the second pass of the two-pass variance: m2 + (x - mean)^2 where `in`, else m2; the register kernels call it for
// k = 0 .. KP - 1 in member order with in = FULL || k < K.  numpy rounds the square and the running sum separately.  x is converted
// to fp64 AGAIN, behind an empty asm that keeps the compiler from reusing the first pass's conversion: 2 K live fp64 registers
// would halve the occupancy.  (The step, not the loop: with the loop in here the VEC = 1 instances come out differently.)
__device__ __forceinline__ double ens_m2_add(double m2, float x, double mean, bool in) {
#pragma clang fp contract(off)
    asm("" : "+v"(x));
    const double d = (double)x - mean;
    const double m1 = m2 + d * d;
    return in ? m1 : m2;
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

// the same sum over a lane's LDS column (the K real values lie in member order until ens_sort_column runs)
__device__ __forceinline__ double ens_m2_column(const float* s, int K, double mean) {
#pragma clang fp contract(off)
    double m2 = 0.0;
    for (int k = 0; k < K; ++k) {
        const double d = (double)s[k * ENS_STAGED_THREADS] - mean;
        m2 += d * d;
    }
    return m2;
}

// ------------------------------------------------------------------------------------------------ host: which instance serves K
// K <= 64, registers: KP = K rounded up to 2, 4, ... 64 and VEC elements per lane so that KP * VEC stays at 64 data registers
// (KP <= 16: 4, 32: 2, 64: 1).  FULL = (K == KP): no padding rows, no predication.  Vector loads / stores need whole, aligned
// groups in every row: with n or stride no multiple of VEC, or one of ptrs (the stack and every per-element array; all hold
// 4-byte elements, null counts as aligned) not aligned to VEC of them, the VEC = 1 instance runs instead -- never an
// intermediate width -- one element per lane, still coalesced.  reg(KP, VEC, FULL, grid) gets the three as integral constants.
// 64 < K <= 256, LDS columns: staged(KP, grid, lds_bytes) with KP = 128 or 256.
// `who` names the entry in the message of the grid-size guard.
template <int KP, int VEC, class Reg>
void ens_launch_reg(const char* who, int K, size_t n, size_t stride, std::initializer_list<const void*> ptrs, Reg& reg) {
    if constexpr (VEC > 1) {
        bool whole = n % VEC == 0 && stride % VEC == 0;
        for (const void* p : ptrs) whole = whole && (uintptr_t)p % (sizeof(float) * VEC) == 0;
        if (!whole) return ens_launch_reg<KP, 1>(who, K, n, stride, ptrs, reg);
    }
    const size_t blocks = cdivz(n, (size_t)ENS_THREADS * VEC);
    DL4DS_REQUIRE(blocks <= 0x7fffffffull, std::string(who) + ": too many elements for one launch");
    const std::integral_constant<int, KP> kp;
    const std::integral_constant<int, VEC> vec;
    if (K == KP) reg(kp, vec, std::true_type{}, dim3((unsigned)blocks));
    else reg(kp, vec, std::false_type{}, dim3((unsigned)blocks));
}

template <class Reg, class Staged>
void ens_launch(const char* who, int K, size_t n, size_t stride, std::initializer_list<const void*> ptrs, Reg reg, Staged staged) {
    if (K <= 2) ens_launch_reg<2, 4>(who, K, n, stride, ptrs, reg);
    else if (K <= 4) ens_launch_reg<4, 4>(who, K, n, stride, ptrs, reg);
    else if (K <= 8) ens_launch_reg<8, 4>(who, K, n, stride, ptrs, reg);
    else if (K <= 16) ens_launch_reg<16, 4>(who, K, n, stride, ptrs, reg);
    else if (K <= 32) ens_launch_reg<32, 2>(who, K, n, stride, ptrs, reg);
    else if (K <= 64) ens_launch_reg<64, 1>(who, K, n, stride, ptrs, reg);
    else {
        const int kp = K <= 128 ? 128 : 256;
        const size_t blocks = cdivz(n, ENS_STAGED_THREADS);
        DL4DS_REQUIRE(blocks <= 0x7fffffffull, std::string(who) + ": too many elements for one launch");
        staged(kp, dim3((unsigned)blocks), (size_t)kp * ENS_STAGED_THREADS * sizeof(float));        // 32 KB / 64 KB of LDS
    }
}
