// MinMaxScaler / StandardScaler of dl4ds/preprocessing.py on the device: the NaN-skipping statistics of `partial_fit`
// (np.nanmin / nanmax / nanmean / nanstd over a set of axes, keepdims) in ONE read of X, and the element-wise passes of
// `transform` / `inverse_transform` as one streaming rewrite.  float and double data, size_t indexing.  DESIGN.md section 11.
//
// Shape handling (host, make_plan): size-1 axes dropped, adjacent axes of one kind merged -> an alternating kept / reduced shape
// of at most five groups.  The two innermost groups decide the memory shape, the remaining (at most four) "outer" groups only
// enumerate rows:
//  * ROWS, period P: the array is n_outer rows of row_len contiguous elements; element f of a row belongs to inner cell f mod P.
//      P = 1  : innermost group reduced (axis=None: one row; axis=(1,2) on (N,H,W): one row per sample)
//      P <= 64: innermost group KEPT and small (axis=(0,1,2) on channels-last (N,H,W,C)): the row is the reduced group times P,
//               read flat; a workgroup advances by L = the largest multiple of lcm(P, VEC) that fits its slots, so the channel of
//               every lane's register is fixed for the whole pass and nothing is strided by C.
//    Every row is split over S workgroups; a workgroup leaves P partial states.
//  * COLS: innermost group kept and wide (axis=0: per grid point over time).  Lanes along the kept index (VEC columns each), the
//    reduced index walked with stride K, split over S workgroups when there are few column tiles.
// A state is (n, mean, M2, min, max) in fp64.  Per lane the sums are taken about a pivot (the lane's first non-NaN value):
// s1 = sum(x - p), s2 = sum((x - p)^2), which is free of the cancellation of plain sum / sum-of-squares (kelvin temperatures),
// and costs three fp64 operations per element instead of Welford's division.  Lanes, workgroups and splits are then combined with
// Chan's merge in a fixed order: an LDS tree in the workgroup, partials in the workspace, one finishing kernel.  No floating-point
// atomics anywhere, so a repeated call gives the same bits.  The NaN mask is a bit per element (bit e%32 of word e/32), built
// from the same loads with integer atomicOr of the non-zero words into a cleared buffer (order-independent).
#include "common.h"
#include "ops.h"
#include "prof.h"
#include <algorithm>
#include <cmath>

// numpy performs `X *= a; X += b` as two separately rounded operations in the array's dtype: no fused multiply-add here
#pragma clang fp contract(off)

namespace {

constexpr int SC_THREADS = 256;
constexpr int SC_MAX_OUTER = 4;
constexpr int SC_UNROLL = 4;              // loads in flight per lane in the statistics kernels
constexpr size_t SC_PERIOD_MAX = 64;        // kept innermost extents up to this are read flat (ROWS, period P)
constexpr size_t SC_TARGET_BLOCKS = 2048;   // 256 CUs x 8

struct Outer { size_t d[SC_MAX_OUTER]; int kept[SC_MAX_OUTER]; int n; };

struct Plan {
    Outer outer;
    size_t R = 1, K = 1;          // the two innermost groups: reduced extent, kept extent (1 when the innermost group is reduced)
    size_t n_outer = 1, n_outer_red = 1, n_outer_kept = 1;
    size_t n = 0, ncells = 1, per_cell = 1;
    bool cols = false;
    size_t row_len = 1;
};

Plan make_plan(const size_t* shape, int ndim, const int* reduce) {
    DL4DS_REQUIRE(ndim >= 0 && ndim <= 8, "scaler: at most 8 axes");
    size_t md[8];
    int mk[8];          // 1 = kept
    int m = 0;
    size_t n = 1;
    for (int i = 0; i < ndim; ++i) {
        DL4DS_REQUIRE(shape[i] > 0, "scaler: empty array");
        n *= shape[i];
        if (shape[i] == 1) continue;
        const int kept = reduce[i] ? 0 : 1;
        if (m && mk[m - 1] == kept) md[m - 1] *= shape[i];
        else { md[m] = shape[i]; mk[m] = kept; ++m; }
    }
    DL4DS_REQUIRE(m <= 5, "scaler: more than five alternating kept / reduced axis groups");
    Plan p;
    p.n = n;
    int no = m;
    if (m == 0) { p.R = 1; p.K = 1; }
    else if (!mk[m - 1]) { p.R = md[m - 1]; p.K = 1; no = m - 1; }
    else {
        p.K = md[m - 1];
        if (m >= 2) { p.R = md[m - 2]; no = m - 2; } else { p.R = 1; no = 0; }
    }
    p.outer.n = no;
    for (int i = 0; i < SC_MAX_OUTER; ++i) { p.outer.d[i] = 1; p.outer.kept[i] = 0; }
    for (int i = 0; i < no; ++i) {
        p.outer.d[i] = md[i];
        p.outer.kept[i] = mk[i];
        p.n_outer *= md[i];
        if (mk[i]) p.n_outer_kept *= md[i]; else p.n_outer_red *= md[i];
    }
    p.ncells = p.n_outer_kept * p.K;
    p.per_cell = p.n_outer_red * p.R;
    p.cols = p.K > SC_PERIOD_MAX;
    p.row_len = p.R * p.K;
    return p;
}

size_t gcdz(size_t a, size_t b) { while (b) { const size_t t = a % b; a = b; b = t; } return a; }

// ---------------------------------------------------------------------------------------------------------------- device helpers
template <typename T, int VEC> struct alignas(sizeof(T) * VEC) Pack { T v[VEC]; };

struct State { double n, mean, m2, mn, mx; };

__device__ __forceinline__ State state_empty() { return State{0.0, 0.0, 0.0, __builtin_inf(), -__builtin_inf()}; }

// Chan et al.: b merged into a
__device__ __forceinline__ State state_merge(const State& a, const State& b) {
    if (b.n == 0.0) return a;
    if (a.n == 0.0) return b;
    State r;
    r.n = a.n + b.n;
    const double delta = b.mean - a.mean;
    r.mean = a.mean + delta * (b.n / r.n);
    r.m2 = a.m2 + b.m2 + delta * delta * (a.n * b.n / r.n);
    r.mn = fmin(a.mn, b.mn);
    r.mx = fmax(a.mx, b.mx);
    return r;
}

template <typename T> struct Acc {
    double s1, s2, piv;
    unsigned long long n;
    T mn, mx;
};
template <typename T> __device__ __forceinline__ void acc_init(Acc<T>& a) {
    a.s1 = 0.0; a.s2 = 0.0; a.piv = 0.0; a.n = 0ull;
    a.mn = (T)__builtin_inf(); a.mx = (T)-__builtin_inf();
}
template <typename T> __device__ __forceinline__ void acc_add(Acc<T>& a, T x) {
    if (x == x) {
        if (a.n == 0ull) a.piv = (double)x;
        const double d = (double)x - a.piv;
        a.s1 += d;
        a.s2 = fma(d, d, a.s2);
        a.n += 1ull;
        a.mn = x < a.mn ? x : a.mn;
        a.mx = x > a.mx ? x : a.mx;
    }
}
template <typename T> __device__ __forceinline__ State acc_state(const Acc<T>& a) {
    if (a.n == 0ull) return state_empty();
    State s;
    s.n = (double)a.n;
    s.mean = a.piv + a.s1 / s.n;
    const double m2 = a.s2 - a.s1 * a.s1 / s.n;
    s.m2 = m2 > 0.0 ? m2 : 0.0;
    s.mn = (double)a.mn;
    s.mx = (double)a.mx;
    return s;
}

__device__ __forceinline__ State state_load(const double* ws, size_t nstates, size_t i) {
    return State{ws[i], ws[nstates + i], ws[2 * nstates + i], ws[3 * nstates + i], ws[4 * nstates + i]};
}
__device__ __forceinline__ void state_store(double* ws, size_t nstates, size_t i, const State& s) {
    ws[i] = s.n; ws[nstates + i] = s.mean; ws[2 * nstates + i] = s.m2; ws[3 * nstates + i] = s.mn; ws[4 * nstates + i] = s.mx;
}
// out [5][ncells] = count, min, max, mean, population std; an empty cell gives count 0 and NaN
__device__ __forceinline__ void state_finish(double* out, size_t ncells, size_t cell, const State& s, double per_cell,
                                             unsigned* nan_flag) {
    const double nan = __builtin_nan("");
    const bool empty = s.n == 0.0;
    out[cell] = s.n;
    out[ncells + cell] = empty ? nan : s.mn;
    out[2 * ncells + cell] = empty ? nan : s.mx;
    out[3 * ncells + cell] = empty ? nan : s.mean;
    out[4 * ncells + cell] = empty ? nan : sqrt(s.m2 / s.n);
    if (s.n < per_cell) atomicOr(nan_flag, 1u);
}

// VEC consecutive elements at x; only the first nv (<= VEC) exist
template <typename T, int VEC> __device__ __forceinline__ void load_elems(const T* x, unsigned nv, T (&v)[VEC]) {
    if (VEC > 1 && nv == VEC) {
        const Pack<T, VEC> q = *reinterpret_cast<const Pack<T, VEC>*>(x);
#pragma unroll
        for (int j = 0; j < VEC; ++j) v[j] = q.v[j];
    } else {
#pragma unroll
        for (int j = 0; j < VEC; ++j) v[j] = (unsigned)j < nv ? x[j] : T(0);
    }
}

// The NaN bits of a wave's elements into the bit mask.  Every lane of the wave calls this (shuffles); `bits` holds the lane's VEC
// flags, e0 the flat index of the lane's first element.  32 / VEC neighbouring lanes cover 32 consecutive elements.
template <int VEC> __device__ __forceinline__ void mask_emit(unsigned* mask, unsigned bits, size_t e0) {
    if (!__any(bits != 0u)) return;
    constexpr int G = 32 / VEC;
    const int gl = (threadIdx.x & 63) % G;
    unsigned v = bits << (VEC * gl);
#pragma unroll
    for (int m = 1; m < G; m <<= 1) v |= (unsigned)__shfl_xor((int)v, m);
    if (gl == 0 && v) {
        const unsigned long long w = (unsigned long long)v << (unsigned)(e0 & 31);
        if ((unsigned)w) atomicOr(mask + (e0 >> 5), (unsigned)w);
        if ((unsigned)(w >> 32)) atomicOr(mask + (e0 >> 5) + 1, (unsigned)(w >> 32));
    }
}

// flat index over the outer groups -> flat index over the KEPT outer groups
__device__ __forceinline__ size_t outer_kept_index(const Outer& o, size_t idx) {
    size_t kc = 0, stride = 1;
    for (int i = o.n - 1; i >= 0; --i) {
        const size_t c = idx % o.d[i];
        idx /= o.d[i];
        if (o.kept[i]) { kc += c * stride; stride *= o.d[i]; }
    }
    return kc;
}
// (kept index, reduced index) over the outer groups -> flat index over all of them
__device__ __forceinline__ size_t outer_index(const Outer& o, size_t kc, size_t jr) {
    size_t idx = 0, stride = 1;
    for (int i = o.n - 1; i >= 0; --i) {
        size_t c;
        if (o.kept[i]) { c = kc % o.d[i]; kc /= o.d[i]; } else { c = jr % o.d[i]; jr /= o.d[i]; }
        idx += c * stride;
        stride *= o.d[i];
    }
    return idx;
}

// ---------------------------------------------------------------------------------------------------------------- statistics
struct RowsArgs {
    const void* x;
    size_t row_len, S, seg;       // S workgroups per row, each seg elements (a multiple of L)
    unsigned L, P;                // elements per workgroup iteration (multiple of P and VEC), period
    double* ws;
    size_t nstates;
    unsigned* mask;
};

template <typename T, int VEC>
__global__ __launch_bounds__(SC_THREADS) void scaler_stats_rows_kernel(RowsArgs p) {
    constexpr int SLOTS = SC_THREADS * VEC;
    __shared__ double sm[5][SLOTS];
    const size_t b = blockIdx.x;
    const size_t o = b / p.S, sp = b % p.S;
    const size_t seg0 = sp * p.seg;
    const size_t seglen = p.row_len - seg0 < p.seg ? p.row_len - seg0 : p.seg;
    const size_t base = o * p.row_len + seg0;
    const T* x = static_cast<const T*>(p.x) + base;
    const unsigned s0 = threadIdx.x * VEC;
    Acc<T> acc[VEC];
#pragma unroll
    for (int j = 0; j < VEC; ++j) acc_init(acc[j]);
    // SC_UNROLL iterations' loads are issued before the first is consumed (memory-level parallelism)
    for (size_t off0 = 0; off0 < seglen; off0 += (size_t)SC_UNROLL * p.L) {
        T v[SC_UNROLL][VEC];
        unsigned nv[SC_UNROLL];
#pragma unroll
        for (int u = 0; u < SC_UNROLL; ++u) {
            const size_t off = off0 + (size_t)u * p.L;
            const size_t rem = off < seglen ? seglen - off : 0;
            const unsigned lim = rem < p.L ? (unsigned)rem : p.L;
            nv[u] = s0 < lim ? (lim - s0 < (unsigned)VEC ? lim - s0 : (unsigned)VEC) : 0u;
            if (nv[u]) load_elems<T, VEC>(x + off + s0, nv[u], v[u]);
        }
#pragma unroll
        for (int u = 0; u < SC_UNROLL; ++u) {
            unsigned bits = 0u;
#pragma unroll
            for (int j = 0; j < VEC; ++j)
                if ((unsigned)j < nv[u]) {
                    if (v[u][j] != v[u][j]) bits |= 1u << j;
                    acc_add(acc[j], v[u][j]);
                }
            if (p.mask) mask_emit<VEC>(p.mask, bits, base + off0 + (size_t)u * p.L + s0);
        }
    }
#pragma unroll
    for (int j = 0; j < VEC; ++j) {
        const State s = acc_state(acc[j]);
        sm[0][s0 + j] = s.n; sm[1][s0 + j] = s.mean; sm[2][s0 + j] = s.m2; sm[3][s0 + j] = s.mn; sm[4][s0 + j] = s.mx;
    }
    __syncthreads();
    // slots s and s + m*P hold the same inner cell: fixed-order tree over m
    const unsigned groups = (p.L + p.P - 1) / p.P;
    unsigned h = 1;
    while (h < groups) h <<= 1;
    for (h >>= 1; h >= 1; h >>= 1) {
        const unsigned span = h * p.P;
        for (unsigned s = threadIdx.x; s < span; s += SC_THREADS) {
            const unsigned q = s + span;
            if (q < p.L) {
                const State a{sm[0][s], sm[1][s], sm[2][s], sm[3][s], sm[4][s]};
                const State c{sm[0][q], sm[1][q], sm[2][q], sm[3][q], sm[4][q]};
                const State r = state_merge(a, c);
                sm[0][s] = r.n; sm[1][s] = r.mean; sm[2][s] = r.m2; sm[3][s] = r.mn; sm[4][s] = r.mx;
            }
        }
        __syncthreads();
    }
    if (threadIdx.x < p.P) {
        const unsigned s = threadIdx.x;
        state_store(p.ws, p.nstates, b * p.P + s, State{sm[0][s], sm[1][s], sm[2][s], sm[3][s], sm[4][s]});
    }
}

struct ColsArgs {
    const void* x;
    size_t R, K, S, rseg, ktiles;
    double* ws;                   // [5][n_outer*S*K] partial states, or
    size_t nstates;
    double* out;                  // (direct) the final statistics when every cell has exactly one partial
    size_t ncells;
    double per_cell;
    unsigned* nan_flag;
    unsigned* mask;
};

template <typename T, int VEC>
__global__ __launch_bounds__(SC_THREADS) void scaler_stats_cols_kernel(ColsArgs p) {
    constexpr int SLOTS = SC_THREADS * VEC;
    const size_t b = blockIdx.x;
    const size_t kt = b % p.ktiles, q = b / p.ktiles;
    const size_t sp = q % p.S, o = q / p.S;
    const size_t k0 = kt * SLOTS + (size_t)threadIdx.x * VEC;
    const unsigned nv = k0 < p.K ? (p.K - k0 < (size_t)VEC ? (unsigned)(p.K - k0) : (unsigned)VEC) : 0u;
    const size_t r0 = sp * p.rseg;
    const size_t r1 = p.R - r0 < p.rseg ? p.R : r0 + p.rseg;
    const T* x = static_cast<const T*>(p.x);
    Acc<T> acc[VEC];
#pragma unroll
    for (int j = 0; j < VEC; ++j) acc_init(acc[j]);
    for (size_t ra = r0; ra < r1; ra += SC_UNROLL) {
        T v[SC_UNROLL][VEC];
#pragma unroll
        for (int u = 0; u < SC_UNROLL; ++u)
            if (nv && ra + u < r1) load_elems<T, VEC>(x + (o * p.R + ra + u) * p.K + k0, nv, v[u]);
#pragma unroll
        for (int u = 0; u < SC_UNROLL; ++u) {
            const bool live = ra + u < r1;
            unsigned bits = 0u;
#pragma unroll
            for (int j = 0; j < VEC; ++j)
                if (live && (unsigned)j < nv) {
                    if (v[u][j] != v[u][j]) bits |= 1u << j;
                    acc_add(acc[j], v[u][j]);
                }
            if (p.mask) mask_emit<VEC>(p.mask, bits, (o * p.R + ra + u) * p.K + k0);
        }
    }
#pragma unroll
    for (int j = 0; j < VEC; ++j)
        if ((unsigned)j < nv) {
            const State s = acc_state(acc[j]);
            if (p.out) state_finish(p.out, p.ncells, o * p.K + k0 + j, s, p.per_cell, p.nan_flag);
            else state_store(p.ws, p.nstates, (o * p.S + sp) * p.K + k0 + j, s);
        }
}

struct FinishArgs {
    Outer outer;
    const double* ws;
    size_t nstates, S, Pn, nj, ncells;     // partial (o, sp, pp) lives at (o*S + sp)*Pn + pp; nj = n_outer_red * S per cell
    unsigned G;                            // threads per cell (power of two <= 256)
    double per_cell;
    double* out;
    unsigned* nan_flag;
};

__global__ __launch_bounds__(SC_THREADS) void scaler_stats_finish_kernel(FinishArgs p) {
    __shared__ double sm[5][SC_THREADS];
    const unsigned t = threadIdx.x;
    const unsigned cpb = SC_THREADS / p.G;
    const unsigned cl = t % cpb, jl = t / cpb;
    const size_t cell = (size_t)blockIdx.x * cpb + cl;
    State acc = state_empty();
    if (cell < p.ncells) {
        const size_t kc = cell / p.Pn, pp = cell % p.Pn;
        for (size_t j = jl; j < p.nj; j += p.G) {
            const size_t jr = j / p.S, sp = j % p.S;
            const size_t o = outer_index(p.outer, kc, jr);
            acc = state_merge(acc, state_load(p.ws, p.nstates, (o * p.S + sp) * p.Pn + pp));
        }
    }
    if (p.G > 1) {
        sm[0][t] = acc.n; sm[1][t] = acc.mean; sm[2][t] = acc.m2; sm[3][t] = acc.mn; sm[4][t] = acc.mx;
        __syncthreads();
        for (unsigned h = p.G >> 1; h >= 1; h >>= 1) {
            if (jl < h) {
                const unsigned q = t + h * cpb;
                const State a{sm[0][t], sm[1][t], sm[2][t], sm[3][t], sm[4][t]};
                const State c{sm[0][q], sm[1][q], sm[2][q], sm[3][q], sm[4][q]};
                const State r = state_merge(a, c);
                sm[0][t] = r.n; sm[1][t] = r.mean; sm[2][t] = r.m2; sm[3][t] = r.mn; sm[4][t] = r.mx;
            }
            __syncthreads();
        }
        acc = State{sm[0][t], sm[1][t], sm[2][t], sm[3][t], sm[4][t]};
    }
    if (jl == 0 && cell < p.ncells) state_finish(p.out, p.ncells, cell, acc, p.per_cell, p.nan_flag);
}

// how the statistics pass of a plan is launched (shared by the workspace query and the launch)
struct StatsLaunch {
    int vec;
    unsigned L;
    size_t S, seg, ktiles, Pn, nstates, blocks;
    bool direct;
};

StatsLaunch stats_launch(const Plan& p, int elem_bytes, bool aligned) {
    StatsLaunch l{};
    const size_t vmax = 16 / elem_bytes;
    if (p.cols) {
        l.vec = (aligned && p.K % vmax == 0) ? (int)vmax : 1;
        const size_t slots = (size_t)SC_THREADS * l.vec;
        l.ktiles = cdivz(p.K, slots);
        const size_t base = p.n_outer * l.ktiles;
        size_t S = base >= SC_TARGET_BLOCKS ? 1 : SC_TARGET_BLOCKS / base;
        S = std::max<size_t>(1, std::min(S, p.R / 16));          // at least 16 rows per split
        l.seg = cdivz(p.R, S);
        l.S = cdivz(p.R, l.seg);
        l.Pn = p.K;
        l.direct = l.S == 1 && p.n_outer_red == 1;
        l.blocks = base * l.S;
    } else {
        l.vec = (aligned && (p.row_len % vmax == 0 || p.n_outer == 1)) ? (int)vmax : 1;
        const size_t slots = (size_t)SC_THREADS * l.vec;
        const size_t unit = p.K / gcdz(p.K, (size_t)l.vec) * l.vec;      // lcm(P, VEC) <= 64 * VEC <= slots
        l.L = (unsigned)(slots / unit * unit);
        size_t S = p.n_outer >= SC_TARGET_BLOCKS ? 1 : SC_TARGET_BLOCKS / p.n_outer;
        S = std::max<size_t>(1, std::min(S, p.row_len / (4 * (size_t)l.L)));   // at least four iterations per split
        l.seg = cdivz(cdivz(p.row_len, S), (size_t)l.L) * l.L;
        l.S = cdivz(p.row_len, l.seg);
        l.Pn = p.K;
        l.direct = false;
        l.blocks = p.n_outer * l.S;
    }
    l.nstates = l.direct ? 0 : p.n_outer * l.S * l.Pn;
    return l;
}

template <typename T>
void stats_typed(hipStream_t s, const Plan& p, const StatsLaunch& l, const void* x, double* out, unsigned* nan_flag, unsigned* mask,
                 double* ws) {
    constexpr int VMAX = 16 / (int)sizeof(T);
    DL4DS_REQUIRE(l.blocks < (size_t(1) << 31), "scaler: too many rows for one launch");
    if (p.cols) {
        ColsArgs a{x, p.R, p.K, l.S, l.seg, l.ktiles, ws, l.nstates, l.direct ? out : nullptr, p.ncells, (double)p.per_cell,
                   nan_flag, mask};
        auto kv = scaler_stats_cols_kernel<T, VMAX>;
        auto k1 = scaler_stats_cols_kernel<T, 1>;
        if (l.vec > 1) DL4DS_LAUNCH(kv, dim3((unsigned)l.blocks), dim3(SC_THREADS), 0, s, a);
        else DL4DS_LAUNCH(k1, dim3((unsigned)l.blocks), dim3(SC_THREADS), 0, s, a);
    } else {
        RowsArgs a{x, p.row_len, l.S, l.seg, l.L, (unsigned)p.K, ws, l.nstates, mask};
        auto kv = scaler_stats_rows_kernel<T, VMAX>;
        auto k1 = scaler_stats_rows_kernel<T, 1>;
        if (l.vec > 1) DL4DS_LAUNCH(kv, dim3((unsigned)l.blocks), dim3(SC_THREADS), 0, s, a);
        else DL4DS_LAUNCH(k1, dim3((unsigned)l.blocks), dim3(SC_THREADS), 0, s, a);
    }
    if (l.direct) return;
    FinishArgs f{};
    f.outer = p.outer;
    f.ws = ws; f.nstates = l.nstates; f.S = l.S; f.Pn = l.Pn;
    f.nj = p.n_outer_red * l.S;
    f.ncells = p.ncells;
    unsigned G = 1;
    while (G < SC_THREADS && (size_t)G * 8 < f.nj) G <<= 1;          // up to eight partials per thread before the tree
    f.G = G;
    f.per_cell = (double)p.per_cell;
    f.out = out; f.nan_flag = nan_flag;
    const size_t fb = cdivz(p.ncells, (size_t)(SC_THREADS / G));
    DL4DS_REQUIRE(fb < (size_t(1) << 31), "scaler: too many cells for one launch");
    DL4DS_LAUNCH(scaler_stats_finish_kernel, dim3((unsigned)fb), dim3(SC_THREADS), 0, s, f);
}

// ---------------------------------------------------------------------------------------------------------------- apply
struct ApplyArgs {
    Outer outer;
    const void* x;
    void* out;
    size_t row_len, K, chunks, chunk;     // chunk: elements per workgroup (a multiple of L)
    unsigned L;
    int periodic;                         // K <= SC_PERIOD_MAX: a lane's cells are fixed, operands live in registers
    int op1, op2, nan_mode;
    const void* a;
    const void* b;
    double fill;
    const unsigned* mask;
};

template <typename T> __device__ __forceinline__ T apply_op(int op, T y, T c) {
    switch (op) {
        case SCALER_OP_MUL: return y * c;
        case SCALER_OP_ADD: return y + c;
        case SCALER_OP_SUB: return y - c;
        case SCALER_OP_DIV: return y / c;
        default: return y;
    }
}

template <typename T, int VEC>
__global__ __launch_bounds__(SC_THREADS) void scaler_apply_kernel(ApplyArgs p) {
    const size_t blk = blockIdx.x;
    const size_t o = blk / p.chunks, ch = blk % p.chunks;
    const size_t f0 = ch * p.chunk;
    const size_t flen = p.row_len - f0 < p.chunk ? p.row_len - f0 : p.chunk;
    const size_t base = o * p.row_len + f0;
    const size_t cellbase = outer_kept_index(p.outer, o) * p.K;
    const T* x = static_cast<const T*>(p.x) + base;
    T* out = static_cast<T*>(p.out) + base;
    const T* A = static_cast<const T*>(p.a) + cellbase;
    const T* B = static_cast<const T*>(p.b) + cellbase;
    const unsigned s0 = threadIdx.x * VEC;
    const T fill = (T)p.fill;
    T av[VEC], bv[VEC];
    size_t c = 0, cstep = 0;
    if (p.periodic) {
#pragma unroll
        for (int j = 0; j < VEC; ++j) {
            const unsigned cj = (s0 + j) % (unsigned)p.K;          // f0 and L are multiples of K
            av[j] = p.op1 ? A[cj] : T(0);
            bv[j] = p.op2 ? B[cj] : T(0);
        }
    } else {
        c = (f0 + s0) % p.K;
        cstep = p.L % p.K;
    }
    for (size_t off = 0; off < flen; off += p.L) {
        const size_t rem = flen - off;
        const unsigned lim = rem < p.L ? (unsigned)rem : p.L;
        const unsigned nv = s0 < lim ? (lim - s0 < (unsigned)VEC ? lim - s0 : (unsigned)VEC) : 0u;
        if (nv) {
            T v[VEC];
            load_elems<T, VEC>(x + off + s0, nv, v);
            if (!p.periodic) {
#pragma unroll
                for (int j = 0; j < VEC; ++j) {
                    size_t cj = c + j;
                    if (cj >= p.K) cj -= p.K;
                    av[j] = p.op1 ? A[cj] : T(0);
                    bv[j] = p.op2 ? B[cj] : T(0);
                }
            }
            unsigned mbits = 0u;
            if (p.nan_mode == SCALER_NAN_MASK && p.mask) {
                const size_t e0 = base + off + s0;
                unsigned long long w = p.mask[e0 >> 5];
                if (((e0 & 31) + VEC) > 32) w |= (unsigned long long)p.mask[(e0 >> 5) + 1] << 32;
                mbits = (unsigned)(w >> (e0 & 31));
            }
#pragma unroll
            for (int j = 0; j < VEC; ++j) {
                T y = apply_op<T>(p.op1, v[j], av[j]);
                y = apply_op<T>(p.op2, y, bv[j]);
                if (p.nan_mode == SCALER_NAN_FILL) y = (y != y) ? fill : y;
                else if ((mbits >> j) & 1u) y = (T)__builtin_nan("");
                v[j] = y;
            }
            if (VEC > 1 && nv == VEC) {
                Pack<T, VEC> q;
#pragma unroll
                for (int j = 0; j < VEC; ++j) q.v[j] = v[j];
                *reinterpret_cast<Pack<T, VEC>*>(out + off + s0) = q;
            } else {
#pragma unroll
                for (int j = 0; j < VEC; ++j)
                    if ((unsigned)j < nv) out[off + s0 + j] = v[j];
            }
        }
        if (!p.periodic) { c += cstep; if (c >= p.K) c -= p.K; }
    }
}

template <typename T>
void apply_typed(hipStream_t s, const Plan& p, const void* x, void* out, int op1, const void* a, int op2, const void* b, int nan_mode,
                 double fill, const unsigned* mask) {
    constexpr size_t VMAX = 16 / sizeof(T);
    const bool aligned = ((uintptr_t)x % 16 == 0) && ((uintptr_t)out % 16 == 0);
    const bool periodic = !p.cols;
    size_t vec;
    if (periodic) vec = (aligned && (p.row_len % VMAX == 0 || p.n_outer == 1)) ? VMAX : 1;
    else vec = (aligned && p.K % VMAX == 0) ? VMAX : 1;
    const size_t slots = (size_t)SC_THREADS * vec;
    size_t L = slots;
    if (periodic) {
        const size_t unit = p.K / gcdz(p.K, vec) * vec;
        L = slots / unit * unit;
    }
    ApplyArgs g{};
    g.outer = p.outer;
    g.x = x; g.out = out;
    g.row_len = p.row_len; g.K = p.K;
    g.L = (unsigned)L;
    g.chunk = L * 8;
    g.chunks = cdivz(p.row_len, g.chunk);
    g.periodic = periodic ? 1 : 0;
    g.op1 = op1; g.op2 = op2; g.nan_mode = nan_mode;
    g.a = a ? a : b; g.b = b ? b : a;
    g.fill = fill; g.mask = mask;
    const size_t blocks = p.n_outer * g.chunks;
    DL4DS_REQUIRE(blocks < (size_t(1) << 31), "scaler: too many rows for one launch");
    auto kv = scaler_apply_kernel<T, (int)VMAX>;
    auto k1 = scaler_apply_kernel<T, 1>;
    if (vec > 1) DL4DS_LAUNCH(kv, dim3((unsigned)blocks), dim3(SC_THREADS), 0, s, g);
    else DL4DS_LAUNCH(k1, dim3((unsigned)blocks), dim3(SC_THREADS), 0, s, g);
}

}  // namespace

size_t scaler_cells(const size_t* shape, int ndim, const int* reduce) { return make_plan(shape, ndim, reduce).ncells; }

size_t scaler_stats_workspace_bytes(const size_t* shape, int ndim, const int* reduce, int is_double) {
    const Plan p = make_plan(shape, ndim, reduce);
    // the vector width changes how rows are split: cover both
    const StatsLaunch a = stats_launch(p, is_double ? 8 : 4, true), b = stats_launch(p, is_double ? 8 : 4, false);
    return 5 * sizeof(double) * std::max(a.nstates, b.nstates);
}

void scaler_stats(hipStream_t s, const void* x, int is_double, const size_t* shape, int ndim, const int* reduce, double* out,
                  unsigned* nan_flag, unsigned* mask_bits, void* workspace, size_t workspace_bytes) {
    const Plan p = make_plan(shape, ndim, reduce);
    const StatsLaunch l = stats_launch(p, is_double ? 8 : 4, (uintptr_t)x % 16 == 0);
    DL4DS_REQUIRE(workspace_bytes >= 5 * sizeof(double) * l.nstates, "scaler_stats workspace too small");
    ProfScope ps(s, "scaler_stats", 0.0, (double)p.n * (is_double ? 8.0 : 4.0));
    HIP_CHECK(hipMemsetAsync(nan_flag, 0, sizeof(unsigned), s));
    if (mask_bits) HIP_CHECK(hipMemsetAsync(mask_bits, 0, cdivz(p.n, 32) * sizeof(unsigned), s));
    if (is_double) stats_typed<double>(s, p, l, x, out, nan_flag, mask_bits, static_cast<double*>(workspace));
    else stats_typed<float>(s, p, l, x, out, nan_flag, mask_bits, static_cast<double*>(workspace));
}

void scaler_apply(hipStream_t s, const void* x, void* out, int is_double, const size_t* shape, int ndim, const int* reduce, int op1,
                  const void* a, int op2, const void* b, int nan_mode, double fill, const unsigned* mask_bits) {
    const Plan p = make_plan(shape, ndim, reduce);
    DL4DS_REQUIRE(op1 >= SCALER_OP_NONE && op1 <= SCALER_OP_DIV && op2 >= SCALER_OP_NONE && op2 <= SCALER_OP_DIV,
                  "scaler_apply: unknown operation");
    DL4DS_REQUIRE((!op1 || a) && (!op2 || b), "scaler_apply: an operation without its operand array");
    DL4DS_REQUIRE(nan_mode == SCALER_NAN_FILL || nan_mode == SCALER_NAN_MASK, "scaler_apply: unknown nan_mode");
    ProfScope ps(s, "scaler_apply", 0.0, 2.0 * (double)p.n * (is_double ? 8.0 : 4.0));
    if (is_double) apply_typed<double>(s, p, x, out, op1, a, op2, b, nan_mode, fill, mask_bits);
    else apply_typed<float>(s, p, x, out, op1, a, op2, b, nan_mode, fill, mask_bits);
}
