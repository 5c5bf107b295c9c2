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
//  * longer: a stable LSD radix sort in global memory, four 8-bit passes over (key, index) pairs ping-ponged through the
//    workspace; every pass = per-(pair, tile) digit histogram, a scan per pair, a stable scatter.  Then a ranks kernel per side
//    (side a scatters its 2*rank to original order, side b gathers and reduces to per-tile partial sums) and a finish kernel.
//    Pairs go through in chunks sized by a fixed workspace budget, so the workspace is bounded whatever S is.
#include "common.h"
#include "ops.h"
#include "prof.h"
#include "sort_keys.h"
#include <algorithm>

namespace {

constexpr int RK_LDS_MAX = 4096;                       // longest segment sorted in LDS by one workgroup
constexpr int RK_THREADS = 256;                        // global engine: threads per workgroup (4 waves)
constexpr int RK_TILE = 4096;                          // global engine: elements per tile
constexpr int RK_WAVES = RK_THREADS / 64;
constexpr int RK_WAVE_SPAN = RK_TILE / RK_WAVES;       // 1024 consecutive elements per wave, 16 chunks of 64
constexpr size_t RK_WS_BUDGET = size_t(128) << 20;     // workspace of the global engine (one chunk of pairs)

__device__ __forceinline__ double rho_from(double sab, double saa, double sbb, bool nan, size_t L) {
    if (nan || L < 2) return __builtin_nan("");
    return sab / sqrt(saa * sbb);                      // constant side: 0 / 0 = NaN
}

// fixed-order tree over the block's per-thread partial sums (three at a time); the result lands in red[*][0]
template <int T>
__device__ __forceinline__ void block_sum3(double (*red)[T], double a, double b, double c) {
    const int t = threadIdx.x;
    red[0][t] = a; red[1][t] = b; red[2][t] = c;
    __syncthreads();
#pragma unroll
    for (int s = T / 2; s > 0; s >>= 1) {
        if (t < s) {
            red[0][t] += red[0][t + s];
            red[1][t] += red[1][t + s];
            red[2][t] += red[2][t + s];
        }
        __syncthreads();
    }
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
    for (int k = 2; k <= P; k <<= 1) {
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int q = t; q < P / 2; q += T) {
                const int i = 2 * j * (q / j) + (q % j), o = i + j;
                const bool up = (i & k) == 0;
                const uint32_t a = key[i], b = key[o];
                if ((a > b) == up) {
                    key[i] = b; key[o] = a;
                    const uint32_t x = idx[i]; idx[i] = idx[o]; idx[o] = x;
                }
            }
            __syncthreads();
        }
    }
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
// Chunk-local layout: pair i of the chunk owns elements [i*L, (i+1)*L) of every per-element buffer and tiles
// [i*ntiles, (i+1)*ntiles) of every per-tile buffer.  blockIdx.x = tile, blockIdx.y = pair of the chunk.

template <bool FROM_INPUT>
__device__ __forceinline__ uint32_t load_key(const float* __restrict__ src, const uint32_t* __restrict__ kin, size_t seg, size_t L,
                                             size_t ss, size_t es, size_t pos, int& nan) {
    if (FROM_INPUT) {
        const float v = src[seg * ss + pos * es];
        nan |= (v != v);
        return rank_key(v);
    }
    return kin[seg * L + pos];
}

// per-(pair, tile) digit counts -> hist[(pair*ntiles + tile)*256 + digit]; the input pass of side a also records a NaN flag per
// tile, the one of side b adds its own
template <bool FROM_INPUT>
__global__ void __launch_bounds__(RK_THREADS) spearman_hist_kernel(const float* __restrict__ src, const uint32_t* __restrict__ kin,
                                                                   size_t L, size_t ss, size_t es, int shift, int side_b,
                                                                   uint32_t* __restrict__ hist, uint32_t* __restrict__ nanflag) {
    __shared__ uint32_t cnt[RK_RADIX];
    __shared__ int nan_any;
    const int t = threadIdx.x, lane = t & 63;
    const size_t seg = blockIdx.y, tile = blockIdx.x, ntiles = gridDim.x;
    const size_t t0 = tile * RK_TILE;
    cnt[t] = 0u;
    if (t == 0) nan_any = 0;
    __syncthreads();
    int nan = 0;
    for (int i = t; i < RK_TILE; i += RK_THREADS) {
        const size_t pos = t0 + i;
        const bool valid = pos < L;
        const uint32_t d = valid ? (load_key<FROM_INPUT>(src, kin, seg, L, ss, es, pos, nan) >> shift) & 255u : 0u;
        const uint64_t m = match_digit(d, valid);
        if (valid && (m & ((1ull << lane) - 1ull)) == 0ull) atomicAdd(&cnt[d], (uint32_t)__popcll(m));
    }
    if (FROM_INPUT && nan) nan_any = 1;
    __syncthreads();
    hist[(seg * ntiles + tile) * RK_RADIX + t] = cnt[t];
    if (FROM_INPUT && t == 0) {
        if (!side_b) nanflag[seg * ntiles + tile] = (uint32_t)nan_any;
        else if (nan_any) nanflag[seg * ntiles + tile] = 1u;
    }
}

// stable scatter of one pass: wave w ranks its 1024 consecutive elements per digit in order (chunks of 64, lanes in order by the
// match mask), the waves' counts are scanned in wave order, the pair's offsets of this tile come from the scan kernel
template <bool FROM_INPUT>
__global__ void __launch_bounds__(RK_THREADS) spearman_scatter_kernel(const float* __restrict__ src, const uint32_t* __restrict__ kin,
                                                                      const uint32_t* __restrict__ iin, size_t L, size_t ss, size_t es,
                                                                      int shift, const uint32_t* __restrict__ off,
                                                                      uint32_t* __restrict__ kout, uint32_t* __restrict__ iout) {
    constexpr int CH = RK_WAVE_SPAN / 64;
    __shared__ uint32_t wcnt[RK_WAVES][RK_RADIX];
    __shared__ uint32_t gofs[RK_RADIX];
    const int t = threadIdx.x, lane = t & 63, w = t >> 6;
    const size_t seg = blockIdx.y, tile = blockIdx.x, ntiles = gridDim.x;
    for (int i = t; i < RK_WAVES * RK_RADIX; i += RK_THREADS) wcnt[i / RK_RADIX][i % RK_RADIX] = 0u;
    gofs[t] = off[(seg * ntiles + tile) * RK_RADIX + t];
    __syncthreads();
    const uint64_t lt = (1ull << lane) - 1ull;
    const size_t p0 = tile * RK_TILE + (size_t)w * RK_WAVE_SPAN + lane;
    uint32_t key[CH], id[CH], r[CH];
    int nan = 0;
#pragma unroll
    for (int c = 0; c < CH; ++c) {
        const size_t pos = p0 + (size_t)c * 64;
        const bool valid = pos < L;
        key[c] = valid ? load_key<FROM_INPUT>(src, kin, seg, L, ss, es, pos, nan) : 0u;
        id[c] = valid ? (FROM_INPUT ? (uint32_t)pos : iin[seg * L + pos]) : 0u;
        const uint32_t d = (key[c] >> shift) & 255u;
        const uint64_t m = match_digit(d, valid);
        const uint32_t before = valid ? wcnt[w][d] : 0u;
        r[c] = before + (uint32_t)__popcll(m & lt);
        if (valid && (m & lt) == 0ull) wcnt[w][d] = before + (uint32_t)__popcll(m);
    }
    __syncthreads();
    {                                                  // exclusive scan of the four waves' counts, per digit
        uint32_t run = 0;
#pragma unroll
        for (int v = 0; v < RK_WAVES; ++v) {
            const uint32_t x = wcnt[v][t];
            wcnt[v][t] = run;
            run += x;
        }
    }
    __syncthreads();
#pragma unroll
    for (int c = 0; c < CH; ++c) {
        const size_t pos = p0 + (size_t)c * 64;
        if (pos < L) {
            const uint32_t d = (key[c] >> shift) & 255u;
            const size_t dst = seg * L + gofs[d] + wcnt[w][d] + r[c];
            kout[dst] = key[c];
            iout[dst] = id[c];
        }
    }
}

// 2*rank of every sorted position of one tile.  Side a (!REDUCE): R[original index] = 2*rank.  Side b (REDUCE): gathers side a's
// 2*rank through the sorted indices and writes the tile's three partial sums.  A tie run may reach beyond the tile: its ends come
// from a binary search of the whole sorted pair for the tile's first and last key.
template <bool REDUCE>
__global__ void __launch_bounds__(RK_THREADS) spearman_ranks_kernel(const uint32_t* __restrict__ ks, const uint32_t* __restrict__ is,
                                                                    size_t L, uint32_t* __restrict__ R, double* __restrict__ part) {
    __shared__ uint32_t tk[RK_TILE];
    __shared__ uint32_t g_lo, g_hi;
    __shared__ double red[3][RK_THREADS];
    const int t = threadIdx.x;
    const size_t seg = blockIdx.y, tile = blockIdx.x, ntiles = gridDim.x;
    const size_t t0 = tile * RK_TILE;
    const uint32_t n = (uint32_t)(L - t0 < (size_t)RK_TILE ? L - t0 : (size_t)RK_TILE);
    const uint32_t* k = ks + seg * L;
    for (uint32_t i = t; i < n; i += RK_THREADS) tk[i] = k[t0 + i];
    __syncthreads();
    if (t == 0) g_lo = bound<true>(k, (uint32_t)L, tk[0]);
    if (t == 64) g_hi = bound<false>(k, (uint32_t)L, tk[n - 1]);
    __syncthreads();
    const int64_t c = (int64_t)L + 1;
    int64_t sab = 0, saa = 0, sbb = 0;
    for (uint32_t i = t; i < n; i += RK_THREADS) {
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
        block_sum3<RK_THREADS>(red, (double)sab, (double)saa, (double)sbb);
        if (t == 0) {
            double* p = part + (seg * ntiles + tile) * 3;
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

struct Chunk {
    size_t pairs, ntiles, elems;                       // pairs per chunk, tiles per pair, elements per pair
    size_t bytes_per_pair() const {
        return 5 * al256(elems * 4) + al256(ntiles * RK_RADIX * 4) + al256(ntiles * 4) + al256(ntiles * 24);
    }
};

Chunk plan(size_t S, size_t L) {
    Chunk c{0, cdivz(L, RK_TILE), L};
    c.pairs = std::max<size_t>(1, std::min(S, RK_WS_BUDGET / c.bytes_per_pair()));
    return c;
}

template <int P>
void launch_lds(hipStream_t s, const float* a, const float* b, size_t S, size_t L, size_t ss, size_t es, double* out) {
    DL4DS_LAUNCH(spearman_lds_kernel<P>, dim3((unsigned)S), dim3(lds_threads<P>()), 0, s, a, b, L, ss, es, out);
}

}  // namespace

size_t spearman_workspace_bytes(size_t S, size_t L) {
    if (L <= (size_t)RK_LDS_MAX || S == 0) return 0;
    const Chunk c = plan(S, L);
    return c.pairs * c.bytes_per_pair();
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
    const Chunk c = plan(S, L);
    char* ws = static_cast<char*>(workspace);
    const size_t eb = al256(c.pairs * c.elems * 4);
    uint32_t* k0 = reinterpret_cast<uint32_t*>(ws);
    uint32_t* i0 = reinterpret_cast<uint32_t*>(ws + eb);
    uint32_t* k1 = reinterpret_cast<uint32_t*>(ws + 2 * eb);
    uint32_t* i1 = reinterpret_cast<uint32_t*>(ws + 3 * eb);
    uint32_t* R = reinterpret_cast<uint32_t*>(ws + 4 * eb);
    char* q = ws + 5 * eb;
    uint32_t* hist = reinterpret_cast<uint32_t*>(q);
    q += al256(c.pairs * c.ntiles * RK_RADIX * 4);
    uint32_t* nanflag = reinterpret_cast<uint32_t*>(q);
    q += al256(c.pairs * c.ntiles * 4);
    double* part = reinterpret_cast<double*>(q);
    const int nt = (int)c.ntiles;
    for (size_t s0 = 0; s0 < S; s0 += c.pairs) {
        const size_t np = std::min(c.pairs, S - s0);
        const dim3 grid((unsigned)nt, (unsigned)np);
        for (int side = 0; side < 2; ++side) {
            const float* src = (side ? b : a) + s0 * seg_stride;
            // pass 0 reads the floats (keys made on the fly, index = position) -> (k1, i1); then k1 -> k0 -> k1 -> k0
            DL4DS_LAUNCH(spearman_hist_kernel<true>, grid, dim3(RK_THREADS), 0, s, src, nullptr, L, seg_stride, elem_stride, 0, side,
                         hist, nanflag);
            DL4DS_LAUNCH(radix_scan_kernel, dim3((unsigned)np), dim3(RK_THREADS), 0, s, hist, nt);
            DL4DS_LAUNCH(spearman_scatter_kernel<true>, grid, dim3(RK_THREADS), 0, s, src, nullptr, nullptr, L, seg_stride, elem_stride,
                         0, hist, k1, i1);
            for (int pass = 1; pass < 4; ++pass) {
                const uint32_t* kin = (pass & 1) ? k1 : k0;
                const uint32_t* iin = (pass & 1) ? i1 : i0;
                uint32_t* kout = (pass & 1) ? k0 : k1;
                uint32_t* iout = (pass & 1) ? i0 : i1;
                DL4DS_LAUNCH(spearman_hist_kernel<false>, grid, dim3(RK_THREADS), 0, s, nullptr, kin, L, size_t(0), size_t(0),
                             8 * pass, side, hist, nanflag);
                DL4DS_LAUNCH(radix_scan_kernel, dim3((unsigned)np), dim3(RK_THREADS), 0, s, hist, nt);
                DL4DS_LAUNCH(spearman_scatter_kernel<false>, grid, dim3(RK_THREADS), 0, s, nullptr, kin, iin, L, size_t(0), size_t(0),
                             8 * pass, hist, kout, iout);
            }
            if (side == 0) DL4DS_LAUNCH(spearman_ranks_kernel<false>, grid, dim3(RK_THREADS), 0, s, k0, i0, L, R, part);
            else DL4DS_LAUNCH(spearman_ranks_kernel<true>, grid, dim3(RK_THREADS), 0, s, k0, i0, L, R, part);
        }
        DL4DS_LAUNCH(spearman_finish_kernel, dim3((unsigned)cdivz(np, 256)), dim3(256), 0, s, part, nanflag, np, nt, L, out + s0);
    }
}
