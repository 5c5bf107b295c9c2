// Spearman rank correlation of S pairs of float sequences (compute_correlation, dl4ds/metrics.py:51-97, with
// scipy.stats.spearmanr on 1-D inputs): rho = Pearson correlation of the AVERAGE ranks, NaN when either sequence holds a NaN
// (nan_policy='propagate'), is constant, or is shorter than two.  Element k of sequence s lives at base[s*seg_stride +
// k*elem_stride], which covers both uses of compute_metrics: per test pair (S = N, L = H*W*C, contiguous) and per grid point
// (S = H*W, L = N, strided by H*W*C).
//
// Keys: the float's bits mapped to an order-preserving uint32 (negatives inverted, positives with the top bit set), -0.0 first
// canonicalised to +0.0 so the two zeros form one tie group as numpy's comparison has them.
// Ranks: after sorting, equal keys are adjacent; the run at sorted positions [lo, hi) has average rank (lo + hi + 1) / 2, kept
// exactly as the integer 2*rank = lo + hi + 1 (lo / hi by binary search in the sorted keys).  With d = 2*rank - (L + 1)
// (twice the distance from the mean rank (L + 1) / 2) rho = sum(da*db) / sqrt(sum(da^2) * sum(db^2)); the products are
// integers, summed exactly in int64 per thread and in fp64 in a fixed order above that -- no float atomics, so a repeated
// call gives bitwise the same result.
//
// Two engines:
//  * L <= RK_LDS_MAX: one workgroup per pair sorts (key, index) of one side in LDS (bitonic), writes the 2*rank of every
//    element back in original order into LDS, sorts the other side and walks it in sorted order, gathering the first side's
//    ranks through the sorted indices.  12 B of LDS per element (54 KiB at 4096 with the fp64 reduction buffer: two
//    workgroups per 160 KiB CU).
//  * longer: the stable LSD radix sort of sort_keys.h in global memory, four 8-bit passes over (key, index) pairs ping-ponged
//    through the workspace; every pass = per-(pair, tile) digit histogram, a scan per pair, a stable scatter.  Then a ranks kernel per side
//    (side a scatters its 2*rank to original order, side b gathers and reduces to per-tile partial sums) and a finish kernel.
//    Pairs go through in chunks sized by a fixed workspace budget, so the workspace is bounded whatever S is.
#include "common.h"
#include "ops.h"
#include "prof.h"
#include "sort_keys.h"
#include <algorithm>

namespace {

constexpr int RK_LDS_MAX = 4096;                       // longest segment sorted in LDS by one workgroup

__device__ __forceinline__ double rho_from(double sab, double saa, double sbb, bool nan, size_t L) {
    if (nan || L < 2) return __builtin_nan("");
    return sab / sqrt(saa * sbb);                      // constant side: 0 / 0 = NaN
}

// fixed-order tree over the block's per-thread partial sums (three at a time); the result lands in red[*][0]
template <int T>
__device__ __forceinline__ void block_sum3(double (*red)[T], double a, double b, double c) {
    const int t = threadIdx.x;
    red[0][t] = a; red[1][t] = b; red[2][t] = c;
    group_tree<T>(t, [&](int i, int j) { red[0][i] += red[0][j]; red[1][i] += red[1][j]; red[2][i] += red[2][j]; });
}

// ---------------------------------------------------------------------------------------------------------------- LDS engine
template <int P>
constexpr int lds_threads() { return P / 2 < 64 ? 64 : (P / 2 > 256 ? 256 : P / 2); }

template <int P, int T>
__device__ __forceinline__ void lds_load_sort(const float* __restrict__ src, size_t L, size_t es, uint32_t* key, uint32_t* idx,
                                              int* nan) {
    const int t = threadIdx.x;
    for (int i = t; i < P; i += T) {
        uint32_t k = 0xFFFFFFFFu;                      // padding sorts last (a real key this large is a NaN: result NaN anyway)
        if ((size_t)i < L) {
            const float v = src[(size_t)i * es];
            if (v != v) *nan = 1;
            k = rank_key(v);
        }
        key[i] = k;
        idx[i] = (uint32_t)i;
    }
    __syncthreads();
    bitonic_rows<P, 1, P, T, true>(key, idx);
}

template <int P>
__global__ void __launch_bounds__(lds_threads<P>()) spearman_lds_kernel(const float* __restrict__ a, const float* __restrict__ b,
                                                                        size_t L, size_t ss, size_t es, double* __restrict__ out) {
    constexpr int T = lds_threads<P>();
    __shared__ uint32_t key[P], idx[P], ra[P];
    __shared__ double red[3][T];
    __shared__ int nan_seen;
    const size_t seg = blockIdx.x;
    const int t = threadIdx.x;
    const uint32_t n = (uint32_t)L;
    if (t == 0) nan_seen = 0;
    __syncthreads();
    lds_load_sort<P, T>(a + seg * ss, L, es, key, idx, &nan_seen);
    for (uint32_t j = t; j < n; j += T) {
        const uint32_t k = key[j];
        ra[idx[j]] = bound<true>(key, n, k) + bound<false>(key, n, k) + 1u;
    }
    __syncthreads();
    lds_load_sort<P, T>(b + seg * ss, L, es, key, idx, &nan_seen);
    const int64_t c = (int64_t)L + 1;
    int64_t sab = 0, saa = 0, sbb = 0;
    for (uint32_t j = t; j < n; j += T) {
        const uint32_t k = key[j];
        const int64_t db = (int64_t)(bound<true>(key, n, k) + bound<false>(key, n, k) + 1u) - c;
        const int64_t da = (int64_t)ra[idx[j]] - c;
        sab += da * db; saa += da * da; sbb += db * db;
    }
    block_sum3<T>(red, (double)sab, (double)saa, (double)sbb);
    if (t == 0) out[seg] = rho_from(red[0][0], red[1][0], red[2][0], nan_seen != 0, L);
}

// ------------------------------------------------------------------------------------------------------------- global engine
// The sort is the shared one of sort_keys.h (chunk-local layout and grid convention there): pass 0 reads the floats, makes the
// keys on the fly and flags NaNs per tile; the (key, index) pairs end in (k0, i0).

// 2*rank of every sorted position of one tile.  Side a (!REDUCE): R[original index] = 2*rank.  Side b (REDUCE): gathers side a's
// 2*rank through the sorted indices and writes the tile's three partial sums.  A tie run may reach beyond the tile: its ends come
// from a binary search of the whole sorted pair for the tile's first and last key.
template <bool REDUCE>
__global__ void __launch_bounds__(SORT_THREADS) spearman_ranks_kernel(const uint32_t* __restrict__ ks, const uint32_t* __restrict__ is,
                                                                    size_t L, const TileGrid grid, uint32_t* __restrict__ R,
                                                                    double* __restrict__ part) {
    __shared__ uint32_t tk[SORT_TILE];
    __shared__ uint32_t g_lo, g_hi;
    __shared__ double red[3][SORT_THREADS];
    const int t = threadIdx.x;
    size_t seg, tile;
    grid.split(seg, tile);
    const size_t t0 = tile * SORT_TILE;
    const uint32_t n = (uint32_t)(L - t0 < (size_t)SORT_TILE ? L - t0 : (size_t)SORT_TILE);
    const uint32_t* k = ks + seg * L;
    for (uint32_t i = t; i < n; i += SORT_THREADS) tk[i] = k[t0 + i];
    __syncthreads();
    if (t == 0) g_lo = bound<true>(k, (uint32_t)L, tk[0]);
    if (t == 64) g_hi = bound<false>(k, (uint32_t)L, tk[n - 1]);
    __syncthreads();
    const int64_t c = (int64_t)L + 1;
    int64_t sab = 0, saa = 0, sbb = 0;
    for (uint32_t i = t; i < n; i += SORT_THREADS) {
        const uint32_t x = tk[i];
        const uint32_t lo = bound<true>(tk, n, x), hi = bound<false>(tk, n, x);
        const uint32_t r2 = (lo == 0 ? g_lo : (uint32_t)t0 + lo) + (hi == n ? g_hi : (uint32_t)t0 + hi) + 1u;
        const size_t o = seg * L + is[seg * L + t0 + i];
        if (!REDUCE) {
            R[o] = r2;
        } else {
            const int64_t da = (int64_t)R[o] - c, db = (int64_t)r2 - c;
            sab += da * db; saa += da * da; sbb += db * db;
        }
    }
    if (REDUCE) {
        block_sum3<SORT_THREADS>(red, (double)sab, (double)saa, (double)sbb);
        if (t == 0) {
            double* p = part + (size_t)blockIdx.x * 3;
            p[0] = red[0][0]; p[1] = red[1][0]; p[2] = red[2][0];
        }
    }
}

__global__ void spearman_finish_kernel(const double* __restrict__ part, const uint32_t* __restrict__ nanflag, size_t S, int ntiles,
                                       size_t L, double* __restrict__ out) {
    const size_t seg = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (seg >= S) return;
    double sab = 0.0, saa = 0.0, sbb = 0.0;
    bool nan = false;
    for (int t = 0; t < ntiles; ++t) {                 // fixed order
        const double* p = part + (seg * ntiles + t) * 3;
        sab += p[0]; saa += p[1]; sbb += p[2];
        nan |= nanflag[seg * ntiles + t] != 0u;
    }
    out[seg] = rho_from(sab, saa, sbb, nan, L);
}

// workspace of `pairs` pairs: (key, index) twice, side a's 2*rank; per tile the digit counts, the NaN flag, three partial sums
struct Workspace {
    uint32_t *k0, *i0, *k1, *i1, *R, *hist, *nanflag;
    double* part;
    Workspace(Carver& w, size_t pairs, size_t ntiles, size_t L)
        : k0(w.take<uint32_t>(pairs * L)), i0(w.take<uint32_t>(pairs * L)), k1(w.take<uint32_t>(pairs * L)),
          i1(w.take<uint32_t>(pairs * L)), R(w.take<uint32_t>(pairs * L)), hist(w.take<uint32_t>(pairs * ntiles * SORT_RADIX)),
          nanflag(w.take<uint32_t>(pairs * ntiles)), part(w.take<double>(pairs * ntiles * 3)) {}
};

template <int P>
void launch_lds(hipStream_t s, const float* a, const float* b, size_t S, size_t L, size_t ss, size_t es, double* out) {
    DL4DS_LAUNCH(spearman_lds_kernel<P>, dim3((unsigned)S), dim3(lds_threads<P>()), 0, s, a, b, L, ss, es, out);
}

}  // namespace

size_t spearman_workspace_bytes(size_t S, size_t L) {
    if (L <= (size_t)RK_LDS_MAX || S == 0) return 0;
    return plan_chunks<Workspace>(S, L).bytes();
}

void spearman(hipStream_t s, const float* a, const float* b, size_t S, size_t L, size_t seg_stride, size_t elem_stride, double* out,
              void* workspace, size_t workspace_bytes) {
    DL4DS_REQUIRE(L < (size_t(1) << 28), "spearman: sequences of 2^28 or more elements are not supported");
    DL4DS_REQUIRE(S < (size_t(1) << 31), "spearman: too many pairs");
    if (S == 0) return;
    ProfScope ps(s, "spearman", 0.0, 8.0 * (double)S * (double)L + 8.0 * (double)S);
    if (L <= (size_t)RK_LDS_MAX) {
        if (L <= 64) launch_lds<64>(s, a, b, S, L, seg_stride, elem_stride, out);
        else if (L <= 128) launch_lds<128>(s, a, b, S, L, seg_stride, elem_stride, out);
        else if (L <= 256) launch_lds<256>(s, a, b, S, L, seg_stride, elem_stride, out);
        else if (L <= 512) launch_lds<512>(s, a, b, S, L, seg_stride, elem_stride, out);
        else if (L <= 1024) launch_lds<1024>(s, a, b, S, L, seg_stride, elem_stride, out);
        else if (L <= 2048) launch_lds<2048>(s, a, b, S, L, seg_stride, elem_stride, out);
        else launch_lds<4096>(s, a, b, S, L, seg_stride, elem_stride, out);
        return;
    }
    DL4DS_REQUIRE(workspace_bytes >= spearman_workspace_bytes(S, L), "spearman workspace too small");
    const Chunk c = plan_chunks<Workspace>(S, L);
    Carver carver{static_cast<char*>(workspace)};
    const Workspace w(carver, c.segs, c.ntiles, L);
    const unsigned nt = (unsigned)c.ntiles;
    for (size_t s0 = 0; s0 < S; s0 += c.segs) {
        const size_t np = std::min(c.segs, S - s0);
        const dim3 grid((unsigned)(np * nt)), block(SORT_THREADS);
        for (int side = 0; side < 2; ++side) {
            // pass 0 reads the floats (keys made on the fly, index = position); side a stores the tiles' NaN flags, side b adds to them
            const FloatInput src{(side ? b : a) + s0 * seg_stride, seg_stride, elem_stride, w.nanflag, side};
            segmented_sort<true>(s, src, w.k0, w.i0, w.k1, w.i1, np, L, nt, w.hist);
            if (side == 0) DL4DS_LAUNCH(spearman_ranks_kernel<false>, grid, block, 0, s, w.k0, w.i0, L, tile_grid(nt), w.R, w.part);
            else DL4DS_LAUNCH(spearman_ranks_kernel<true>, grid, block, 0, s, w.k0, w.i0, L, tile_grid(nt), w.R, w.part);
        }
        DL4DS_LAUNCH(spearman_finish_kernel, dim3((unsigned)cdivz(np, 256)), dim3(256), 0, s, w.part, w.nanflag, np, (int)nt, L,
                     out + s0);
    }
}
