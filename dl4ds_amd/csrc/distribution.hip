// Distribution verification of S pairs of float segments (observation y, prediction p): per segment the sample quantiles of
// either side, the 1-Wasserstein distance, the two-sample Kolmogorov-Smirnov statistic times n, a histogram of either side over
// common bin edges and the number of valid elements.  Element k of segment s lives at base[s*seg_stride + k*elem_stride], as in
// rank.hip: per sample over its H*W*C values (contiguous) or per grid cell over the N samples (strided by the number of cells).
//
// An element is VALID iff y and p are both finite there (NaN in y is the masking mechanism); invalid elements leave both sides,
// so both samples have n <= L values.  Keys are the order-preserving uint32 of rank.hip (sort_keys.h; -0.0 is +0.0); an invalid
// element and the padding get the key 0xFFFFFFFF, which no finite float has, and sort last: n is its lower bound in the sorted
// keys.  Only keys are sorted, the values come back by inverting the key.  With a, b the ascending valid values:
//   quantile q: h = q*(n-1), j = floor(h), x[j] + (x[min(j+1, n-1)] - x[j]) * (h - j) in fp64, not contracted (numpy 'linear')
//   W1 = (1/n) sum |a[i] - b[i]| in fp64: per-thread sums over i = r, r + R, ..., then a fixed tree: the same bits every call
//   KS*n = max over v of |#{a <= v} - #{b <= v}|: evaluated at the last element of every tie run of either side (there
//          #{x <= v} of the own side is its position + 1, of the other side an upper bound by binary search): exact integers
//   histogram bin [e_b, e_b+1): difference of two lower bounds; the last bin ends at the upper bound of e_E-1 (right-closed)
//
// Three engines:
//  * LDS, one segment (elem_stride == 1, seg_stride != 1, L <= DS_LDS_MAX): a workgroup loads both sides of its segment as keys into LDS, sorts
//    both with one bitonic network and computes the results from LDS.
//  * LDS, strided (seg_stride == 1, L <= DS_STRIDED_MAX): a workgroup takes G consecutive segments and loads them row by row --
//    adjacent lanes read element k of adjacent segments, G*4 contiguous bytes -- into LDS rows of pitch P + 1 (the transpose:
//    a lane's store goes to bank (g*(P+1) + k) % 32, conflict-free), then the same network sorts the 2*G rows independently.
//    Both are one kernel template <P, G> (P = padded length, G = 1 for the first).
//  * global (everything else): a gather kernel writes both sides' keys into the contiguous workspace (strided input through a
//    64 x 64 LDS transpose, so reads and writes are both coalesced), the key-only radix sort of sort_keys.h per side, a kernel
//    with the W1 / KS partials per tile of sorted positions and a finish kernel per segment.  Segments go through in chunks
//    sized by a fixed workspace budget.
#include "common.h"
#include "ops.h"
#include "prof.h"
#include "sort_keys.h"
#include <algorithm>
#include <cmath>

namespace {

constexpr int DS_LDS_MAX = 8192;                       // longest segment whose two sides one workgroup sorts in LDS (64 KiB of keys)
constexpr int DS_STRIDED_MAX = SORT_STRIDED_MAX;       // longest segment of the strided LDS engine (16 segments of pitch 513)
constexpr int DS_ROW = 16;                             // fewest segments per strided workgroup: rows of 64 contiguous bytes
constexpr size_t DS_LDS_BUDGET = size_t(72) << 10;     // LDS of a workgroup, keys + reduction buffers: two workgroups per 160 KiB CU
constexpr int DS_MAX_Q = 64, DS_MAX_E = 257;           // (the C header states both)
constexpr uint32_t DS_INVALID = SORT_INVALID;          // key of an invalid element and of the padding
constexpr int DS_TR = 64;                              // gather kernel: 64 segments x 64 elements per transposed tile

struct DistParams {
    double q[DS_MAX_Q];
    float edges[DS_MAX_E];
    int Q, E;
};

struct DistOut {
    double* quant;
    double* w1;
    long long* ks;
    long long* hist;
    long long* valid;
};

__device__ __forceinline__ void make_keys(float yv, float pv, uint32_t& a, uint32_t& b) {
    const bool ok = finite_bits(yv) && finite_bits(pv);
    a = ok ? rank_key(yv) : DS_INVALID;
    b = ok ? rank_key(pv) : DS_INVALID;
}

__device__ __forceinline__ uint32_t absdiff(uint32_t x, uint32_t y) { return x > y ? x - y : y - x; }

// what sorted position j < n adds to the W1 sum and to the KS maximum
template <typename P>
__device__ __forceinline__ void position_terms(P ka, P kb, uint32_t n, uint32_t j, double& w1, uint32_t& ks) {
    const uint32_t a = ka[j], b = kb[j];
    w1 += fabs((double)key_value(a) - (double)key_value(b));
    if (a == b) return;                                // v = a[j] = b[j]: the run that ends later decides, at its own end
    if (j + 1 == n || ka[j + 1] != a) ks = max(ks, absdiff(j + 1, bound<false>(kb, n, a)));
    if (j + 1 == n || kb[j + 1] != b) ks = max(ks, absdiff(j + 1, bound<false>(ka, n, b)));
}

// quantiles and histogram of one segment by the R threads r = 0 .. R-1 that share it
template <typename P>
__device__ __forceinline__ void segment_tables(const DistParams& prm, P ka, P kb, uint32_t n, size_t seg, int r, int R,
                                               const DistOut& out) {
    for (int i = r; i < 2 * prm.Q; i += R) {
        const int side = i >= prm.Q, qi = side ? i - prm.Q : i;
        out.quant[(seg * 2 + side) * prm.Q + qi] = quantile_of(side ? kb : ka, n, prm.q[qi]);
    }
    const int B = prm.E - 1;
    for (int i = r; i < 2 * B; i += R) {
        const int side = i >= B, b = side ? i - B : i;
        P k = side ? kb : ka;
        const uint32_t lo = bound<true>(k, n, rank_key(prm.edges[b]));
        const uint32_t hi = b + 1 == B ? bound<false>(k, n, rank_key(prm.edges[B])) : bound<true>(k, n, rank_key(prm.edges[b + 1]));
        out.hist[(seg * 2 + side) * B + b] = (long long)(hi - lo);
    }
}

// fixed-order tree (sum, maximum) over groups of R consecutive threads; the results land in the group's first slot
template <int R>
__device__ __forceinline__ void group_reduce(double* redd, uint32_t* redu, int t, double w, uint32_t ks) {
    redd[t] = w; redu[t] = ks;
    group_tree<R>(t, [&](int i, int j) { redd[i] += redd[j]; redu[i] = max(redu[i], redu[j]); });
}

__device__ __forceinline__ void write_scalars(const DistOut& out, size_t seg, uint32_t n, double w1sum, uint32_t ks) {
    out.w1[seg] = n ? w1sum / (double)n : __builtin_nan("");
    out.ks[seg] = (long long)ks;
    out.valid[seg] = (long long)n;
}

// --------------------------------------------------------------------------------------------------------------- LDS engines
template <int P, int G>
constexpr int lds_threads() { return G * P >= 4096 ? 512 : 256; }
template <int P, int G>
constexpr int lds_pitch() { return G > 1 ? P + 1 : P; }
template <int P, int G>
constexpr size_t lds_bytes() { return (size_t)lds_threads<P, G>() * 12 + (size_t)2 * G * lds_pitch<P, G>() * 4; }

template <int P, int G>
__global__ void __launch_bounds__((lds_threads<P, G>())) dist_lds_kernel(const float* __restrict__ y, const float* __restrict__ p,
                                                                       size_t S, size_t L, size_t ss, size_t es,
                                                                       const DistParams prm, const DistOut out) {
    constexpr int T = lds_threads<P, G>(), PITCH = lds_pitch<P, G>();
    constexpr int R = G == 1 ? T : (P < T ? P : T);    // threads that share a segment in the results phase
    constexpr int GROUPS = T / R;                      // segments worked on at a time
    static_assert(G % GROUPS == 0 && (P & (P - 1)) == 0 && (G & (G - 1)) == 0, "dist_lds_kernel: shape");
    static_assert(lds_bytes<P, G>() <= DS_LDS_BUDGET, "dist_lds_kernel: LDS budget");
    extern __shared__ __attribute__((aligned(16))) unsigned char dist_lds[];
    double* redd = reinterpret_cast<double*>(dist_lds);                   // [T]
    uint32_t* redu = reinterpret_cast<uint32_t*>(redd + T);               // [T]
    uint32_t* ka = redu + T;                                              // [G][PITCH]
    uint32_t* kb = ka + G * PITCH;
    const int t = threadIdx.x;
    const size_t s0 = (size_t)blockIdx.x * G;
    if (G == 1) {
        const size_t base = s0 * ss;
        for (int i = t; i < P; i += T) {
            uint32_t a = DS_INVALID, b = DS_INVALID;
            if ((size_t)i < L) make_keys(y[base + (size_t)i * es], p[base + (size_t)i * es], a, b);
            ka[i] = a; kb[i] = b;
        }
    } else {
        for (int i = t; i < G * P; i += T) {                              // row k of the G segments: adjacent lanes, adjacent floats
            const int k = i / G, g = i % G;
            uint32_t a = DS_INVALID, b = DS_INVALID;
            if ((size_t)k < L && s0 + g < S) {
                const size_t o = (s0 + g) * ss + (size_t)k * es;
                make_keys(y[o], p[o], a, b);
            }
            ka[g * PITCH + k] = a; kb[g * PITCH + k] = b;
        }
    }
    __syncthreads();
    bitonic_rows<P, 2 * G, PITCH, T, false>(ka, nullptr);              // ka and kb are contiguous: 2*G rows
    for (int g0 = 0; g0 < G; g0 += GROUPS) {
        const int g = g0 + t / R, r = t % R;
        const size_t seg = s0 + g;
        const uint32_t* a = ka + g * PITCH;
        const uint32_t* b = kb + g * PITCH;
        const uint32_t n = bound<true>(a, (uint32_t)P, DS_INVALID);
        double w = 0.0;
        uint32_t ks = 0;
        for (uint32_t j = r; j < n; j += R) position_terms(a, b, n, j, w, ks);
        group_reduce<R>(redd, redu, t, w, ks);
        if (seg < S) {
            if (r == 0) write_scalars(out, seg, n, redd[t], redu[t]);
            segment_tables(prm, a, b, n, seg, r, R, out);
        }
        __syncthreads();                                                  // the reduction buffers are written again
    }
}

// ------------------------------------------------------------------------------------------------------------- global engine
// Chunk-local layout and grid convention: sort_keys.h (blockIdx.x = segment of the chunk * ntiles + tile).

// both sides' keys of a chunk, contiguous per segment; lanes run along the elements
__global__ void __launch_bounds__(SORT_THREADS) dist_gather_kernel(const float* __restrict__ y, const float* __restrict__ p, size_t L,
                                                                 size_t ss, size_t es, const TileGrid grid, uint32_t* __restrict__ ka,
                                                                 uint32_t* __restrict__ kb) {
    size_t seg, tile;
    grid.split(seg, tile);
    for (int i = threadIdx.x; i < SORT_TILE; i += SORT_THREADS) {
        const size_t pos = tile * SORT_TILE + i;
        if (pos < L) {
            const size_t o = seg * ss + pos * es;
            uint32_t a, b;
            make_keys(y[o], p[o], a, b);
            ka[seg * L + pos] = a; kb[seg * L + pos] = b;
        }
    }
}

// the same for seg_stride == 1: a tile of 64 segments x 64 elements is read with lanes along the segments and written with lanes
// along the elements, transposed through LDS.  blockIdx.x = segment block * etiles + element block.
__global__ void __launch_bounds__(SORT_THREADS) dist_gather_tr_kernel(const float* __restrict__ y, const float* __restrict__ p,
                                                                    size_t nseg, size_t L, size_t es, unsigned etiles,
                                                                    uint32_t* __restrict__ ka, uint32_t* __restrict__ kb) {
    __shared__ uint32_t ta[DS_TR][DS_TR + 1], tb[DS_TR][DS_TR + 1];
    const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
    const size_t sg0 = (size_t)(blockIdx.x / etiles) * DS_TR, p0 = (size_t)(blockIdx.x % etiles) * DS_TR;
    for (int e = ty; e < DS_TR; e += SORT_WAVES) {
        const size_t seg = sg0 + tx, pos = p0 + e;
        uint32_t a = DS_INVALID, b = DS_INVALID;
        if (seg < nseg && pos < L) make_keys(y[seg + pos * es], p[seg + pos * es], a, b);
        ta[e][tx] = a; tb[e][tx] = b;
    }
    __syncthreads();
    for (int g = ty; g < DS_TR; g += SORT_WAVES) {
        const size_t seg = sg0 + g, pos = p0 + tx;
        if (seg < nseg && pos < L) {
            ka[seg * L + pos] = ta[tx][g]; kb[seg * L + pos] = tb[tx][g];
        }
    }
}

// W1 sum and KS maximum of one tile of sorted positions -> pw / pk[segment*ntiles + tile]
__global__ void __launch_bounds__(SORT_THREADS) dist_terms_kernel(const uint32_t* __restrict__ ka, const uint32_t* __restrict__ kb, size_t L,
                                                                const TileGrid grid, double* __restrict__ pw, uint32_t* __restrict__ pk) {
    __shared__ double redd[SORT_THREADS];
    __shared__ uint32_t redu[SORT_THREADS];
    __shared__ uint32_t n_sh;
    const int t = threadIdx.x;
    size_t seg, tile;
    grid.split(seg, tile);
    const size_t t0 = tile * SORT_TILE;
    const uint32_t* a = ka + seg * L;
    const uint32_t* b = kb + seg * L;
    if (t == 0) n_sh = bound<true>(a, (uint32_t)L, DS_INVALID);
    __syncthreads();
    const uint32_t n = n_sh;
    double w = 0.0;
    uint32_t ks = 0;
    for (int i = t; i < SORT_TILE; i += SORT_THREADS) {
        const size_t j = t0 + i;
        if (j < n) position_terms(a, b, n, (uint32_t)j, w, ks);
    }
    group_reduce<SORT_THREADS>(redd, redu, t, w, ks);
    if (t == 0) { pw[blockIdx.x] = redd[0]; pk[blockIdx.x] = redu[0]; }
}

// per segment of the chunk: the tiles' partials in a fixed order, then the quantiles and the histogram from the sorted keys
__global__ void __launch_bounds__(SORT_THREADS) dist_finish_kernel(const uint32_t* __restrict__ ka, const uint32_t* __restrict__ kb, size_t L,
                                                                 unsigned ntiles, const double* __restrict__ pw,
                                                                 const uint32_t* __restrict__ pk, size_t seg0, const DistParams prm,
                                                                 const DistOut out) {
    __shared__ double redd[SORT_THREADS];
    __shared__ uint32_t redu[SORT_THREADS];
    __shared__ uint32_t n_sh;
    const int t = threadIdx.x;
    const size_t seg = blockIdx.x;
    const uint32_t* a = ka + seg * L;
    const uint32_t* b = kb + seg * L;
    if (t == 0) n_sh = bound<true>(a, (uint32_t)L, DS_INVALID);
    __syncthreads();
    const uint32_t n = n_sh;
    double w = 0.0;
    uint32_t ks = 0;
    for (size_t i = t; i < ntiles; i += SORT_THREADS) {
        w += pw[seg * ntiles + i];
        ks = max(ks, pk[seg * ntiles + i]);
    }
    group_reduce<SORT_THREADS>(redd, redu, t, w, ks);
    if (t == 0) write_scalars(out, seg0 + seg, n, redd[0], redu[0]);
    segment_tables(prm, a, b, n, seg0 + seg, t, SORT_THREADS, out);
}

// workspace of `segs` segments: both sides' keys and the sort's second buffer; per tile the digit counts and the W1 / KS partials
struct Workspace {
    uint32_t *ka, *kb, *tmp, *hist;
    double* pw;
    uint32_t* pk;
    Workspace(Carver& w, size_t segs, size_t ntiles, size_t L)
        : ka(w.take<uint32_t>(segs * L)), kb(w.take<uint32_t>(segs * L)), tmp(w.take<uint32_t>(segs * L)),
          hist(w.take<uint32_t>(segs * ntiles * SORT_RADIX)), pw(w.take<double>(segs * ntiles)), pk(w.take<uint32_t>(segs * ntiles)) {}
};

enum Engine { ENGINE_LDS, ENGINE_STRIDED, ENGINE_GLOBAL };

// seg_stride == 1 is the per-grid-cell layout whatever the number of cells (one cell: elem_stride == 1 as well), so that the
// engine, and with it the order of the W1 sum, depends on L alone when a caller cuts the cells into bands
Engine engine_of(size_t L, size_t ss, size_t es) {
    if (ss == 1) return L <= (size_t)DS_STRIDED_MAX ? ENGINE_STRIDED : ENGINE_GLOBAL;
    return es == 1 && L <= (size_t)DS_LDS_MAX ? ENGINE_LDS : ENGINE_GLOBAL;
}

template <int P, int G>
void launch_lds(hipStream_t s, const float* y, const float* p, size_t S, size_t L, size_t ss, size_t es, const DistParams& prm,
                const DistOut& out) {
    auto kern = dist_lds_kernel<P, G>;
    static bool once = false;
    if (!once) {
        HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize,
                                      (int)lds_bytes<P, G>()));
        once = true;
    }
    const dim3 grid((unsigned)cdivz(S, G)), block(lds_threads<P, G>());
    const size_t lds = lds_bytes<P, G>();
    DL4DS_LAUNCH(kern, grid, block, lds, s, y, p, S, L, ss, es, prm, out);
    HIP_CHECK(hipGetLastError());
}

// G per padded length P of the strided engine: 4096 / P segments, at least DS_ROW -- 64 segments (256-byte rows) at P = 64 down to
// 16 (64-byte rows) from P = 256 on; 2 * G * (P + 1) keys stay within DS_LDS_BUDGET up to P = DS_STRIDED_MAX
void launch_strided(hipStream_t s, const float* y, const float* p, size_t S, size_t L, size_t ss, size_t es, const DistParams& prm,
                    const DistOut& out) {
    if (L <= 64) launch_lds<64, 64>(s, y, p, S, L, ss, es, prm, out);
    else if (L <= 128) launch_lds<128, 32>(s, y, p, S, L, ss, es, prm, out);
    else if (L <= 256) launch_lds<256, DS_ROW>(s, y, p, S, L, ss, es, prm, out);
    else launch_lds<DS_STRIDED_MAX, DS_ROW>(s, y, p, S, L, ss, es, prm, out);
}

void launch_one(hipStream_t s, const float* y, const float* p, size_t S, size_t L, size_t ss, size_t es, const DistParams& prm,
                const DistOut& out) {
    if (L <= 64) launch_lds<64, 1>(s, y, p, S, L, ss, es, prm, out);
    else if (L <= 128) launch_lds<128, 1>(s, y, p, S, L, ss, es, prm, out);
    else if (L <= 256) launch_lds<256, 1>(s, y, p, S, L, ss, es, prm, out);
    else if (L <= 512) launch_lds<512, 1>(s, y, p, S, L, ss, es, prm, out);
    else if (L <= 1024) launch_lds<1024, 1>(s, y, p, S, L, ss, es, prm, out);
    else if (L <= 2048) launch_lds<2048, 1>(s, y, p, S, L, ss, es, prm, out);
    else if (L <= 4096) launch_lds<4096, 1>(s, y, p, S, L, ss, es, prm, out);
    else launch_lds<DS_LDS_MAX, 1>(s, y, p, S, L, ss, es, prm, out);
}

}  // namespace

void distribution_check_args(size_t S, size_t L, const double* q, int Q, const float* edges, int E) {
    DL4DS_REQUIRE(L < (size_t(1) << 31), "distribution: segments of 2^31 or more elements are not supported");
    DL4DS_REQUIRE(S < (size_t(1) << 31), "distribution: too many segments");
    DL4DS_REQUIRE(Q >= 0 && Q <= DS_MAX_Q && (Q == 0 || q), "distribution: between 0 and 64 quantiles are supported");
    for (int i = 0; i < Q; ++i) DL4DS_REQUIRE(q[i] >= 0.0 && q[i] <= 1.0, "distribution: quantiles must lie in [0, 1]");
    DL4DS_REQUIRE(E == 0 || (E >= 2 && E <= DS_MAX_E && edges), "distribution: 0 or between 2 and 257 bin edges are supported");
    for (int i = 0; i < E; ++i) {
        DL4DS_REQUIRE(std::isfinite(edges[i]), "distribution: bin edges must be finite");
        DL4DS_REQUIRE(i == 0 || edges[i] > edges[i - 1], "distribution: bin edges must be strictly increasing");
    }
}

size_t distribution_workspace_bytes(size_t S, size_t L, size_t seg_stride, size_t elem_stride) {
    if (S == 0 || engine_of(L, seg_stride, elem_stride) != ENGINE_GLOBAL) return 0;
    return plan_chunks<Workspace>(S, L).bytes();
}

void distribution(hipStream_t s, const float* y, const float* p, size_t S, size_t L, size_t seg_stride, size_t elem_stride,
                  const double* q, int Q, const float* edges, int E, double* quant, double* w1, long long* ks, long long* hist,
                  long long* valid, void* workspace, size_t workspace_bytes) {
    distribution_check_args(S, L, q, Q, edges, E);
    DL4DS_REQUIRE(E == 0 || hist, "distribution: bin edges without a histogram output");
    if (S == 0) return;
    DistParams prm = {};
    for (int i = 0; i < Q; ++i) prm.q[i] = q[i];
    for (int i = 0; i < E; ++i) prm.edges[i] = edges[i];
    prm.Q = Q; prm.E = E;
    const DistOut out{quant, w1, ks, hist, valid};
    const Engine e = engine_of(L, seg_stride, elem_stride);
    ProfScope ps(s, e == ENGINE_LDS ? "distribution_lds" : e == ENGINE_STRIDED ? "distribution_strided" : "distribution_global", 0.0,
                 8.0 * (double)S * (double)L);
    if (e == ENGINE_LDS) return launch_one(s, y, p, S, L, seg_stride, elem_stride, prm, out);
    if (e == ENGINE_STRIDED) return launch_strided(s, y, p, S, L, seg_stride, elem_stride, prm, out);
    DL4DS_REQUIRE(workspace_bytes >= distribution_workspace_bytes(S, L, seg_stride, elem_stride), "distribution workspace too small");
    const Chunk c = plan_chunks<Workspace>(S, L);
    Carver carver{static_cast<char*>(workspace)};
    const Workspace w(carver, c.segs, c.ntiles, L);
    const unsigned nt = (unsigned)c.ntiles;
    const bool transposed = seg_stride == 1 && elem_stride != 1;
    for (size_t s0 = 0; s0 < S; s0 += c.segs) {
        const size_t ns = std::min(c.segs, S - s0);
        const dim3 grid((unsigned)(ns * nt)), block(SORT_THREADS);
        const float* ys = y + s0 * seg_stride;
        const float* psrc = p + s0 * seg_stride;
        if (transposed) {
            const unsigned etiles = (unsigned)cdivz(L, DS_TR);
            DL4DS_LAUNCH(dist_gather_tr_kernel, dim3((unsigned)(cdivz(ns, DS_TR) * etiles)), block, 0, s, ys, psrc, ns, L, elem_stride,
                         etiles, w.ka, w.kb);
        } else {
            DL4DS_LAUNCH(dist_gather_kernel, grid, block, 0, s, ys, psrc, L, seg_stride, elem_stride, tile_grid(nt), w.ka, w.kb);
        }
        for (uint32_t* k : {w.ka, w.kb}) segmented_sort<false>(s, KeyBuffer{k}, k, nullptr, w.tmp, nullptr, ns, L, nt, w.hist);
        DL4DS_LAUNCH(dist_terms_kernel, grid, block, 0, s, (const uint32_t*)w.ka, (const uint32_t*)w.kb, L, tile_grid(nt), w.pw, w.pk);
        DL4DS_LAUNCH(dist_finish_kernel, dim3((unsigned)ns), block, 0, s, (const uint32_t*)w.ka, (const uint32_t*)w.kb, L, nt,
                     (const double*)w.pw, (const uint32_t*)w.pk, s0, prm, out);
    }
    HIP_CHECK(hipGetLastError());
}
