// The segmented sorter of rank.hip (Spearman ranks from (key, index) pairs) and distribution.hip (sorted values from keys alone),
// DESIGN.md section 10a.  Many float segments are sorted at once, element k of segment s at base[s*seg_stride + k*elem_stride]:
//  * the order-preserving key of a float and binary search in sorted keys;
//  * in LDS: one bitonic network over independent rows of keys, with or without an index payload;
//  * in global memory: a stable 8-bit LSD radix sort, four passes of (per-tile digit histogram, scan per segment, stable
//    scatter) ping-ponged between two buffers, the first pass reading either keys or the floats themselves;
//  * a fixed-order reduction tree, and the chunk planner and workspace carving of the clients' global engines;
//  * what distribution.hip and qmap.hip share on top: the key of an invalid element, the longest segment of the strided LDS
//    engine, and the 'linear' sample quantile read from sorted keys.
// Chunk-local layout of the global engine: segment i of a chunk owns elements [i*L, (i+1)*L) of every per-element buffer and tiles
// [i*ntiles, (i+1)*ntiles) of every per-tile buffer; every per-tile kernel runs with blockIdx.x = i*ntiles + tile (TileGrid).
#pragma once
#include "common.h"
#include "prof.h"
#include <algorithm>

namespace {

constexpr int SORT_RADIX = 256;
constexpr int SORT_THREADS = 256;                      // global engine: threads per workgroup (4 waves)
constexpr int SORT_TILE = 4096;                        // global engine: elements per tile
constexpr int SORT_WAVES = SORT_THREADS / 64;
constexpr int SORT_WAVE_SPAN = SORT_TILE / SORT_WAVES; // 1024 consecutive elements per wave, 16 chunks of 64
constexpr size_t SORT_WS_BUDGET = size_t(128) << 20;   // workspace of a global engine (one chunk of segments)
constexpr size_t SORT_MAX_GRID = size_t(1) << 30;      // most (segment, tile) workgroups of one launch
constexpr uint32_t SORT_INVALID = 0xFFFFFFFFu;         // key of an invalid element and of the padding: no finite float has it, sorts last
constexpr int SORT_STRIDED_MAX = 512;                  // longest segment of the strided (seg_stride == 1) LDS engines

// The grid convention of every per-tile kernel: blockIdx.x = segment*ntiles + tile.  A workgroup splits its index without a
// division: magic = floor((2^64 - 1) / ntiles) + 1 = (2^64 + e) / ntiles with 0 <= e <= ntiles, so the high half of b*magic is
// floor(b / ntiles) for every b < 2^32 (b*e < 2^64); magic 0 stands for ntiles == 1
struct TileGrid {
    unsigned ntiles;
    uint64_t magic;
    __device__ __forceinline__ void split(size_t& seg, size_t& tile) const {
        const uint32_t b = blockIdx.x, q = (uint32_t)__umul64hi((uint64_t)b, magic) + (magic ? 0u : b);   // (no branch)
        seg = q;
        tile = b - q * ntiles;
    }
};

inline TileGrid tile_grid(size_t ntiles) { return {(unsigned)ntiles, ntiles > 1 ? ~uint64_t(0) / ntiles + 1 : 0}; }

__device__ __forceinline__ uint32_t rank_key(float v) {
    uint32_t u = __float_as_uint(v);
    if (u == 0x80000000u) u = 0u;                      // -0.0 == +0.0
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

// the float a key was made from (-0.0 comes back as +0.0)
__device__ __forceinline__ float key_value(uint32_t k) {
    return __uint_as_float((k & 0x80000000u) ? (k & 0x7FFFFFFFu) : ~k);
}

// first position in sorted k[0, n) whose key is >= x (LB) or > x (!LB)
template <bool LB, typename P>
__device__ __forceinline__ uint32_t bound(P k, uint32_t n, uint32_t x) {
    uint32_t lo = 0, hi = n;
    while (lo < hi) {
        const uint32_t mid = (lo + hi) >> 1;
        const uint32_t v = k[mid];
        if (LB ? (v < x) : (v <= x)) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// numpy's 'linear' quantile q of the n ascending values behind the sorted keys k[0, n), in fp64; NaN when n == 0
template <typename P>
__device__ __forceinline__ double quantile_of(P k, uint32_t n, double q) {
#pragma clang fp contract(off)                         // h - floor(h) and the interpolation as written: every product is rounded
    if (n == 0) return __builtin_nan("");
    const double h = q * (double)(n - 1), fl = floor(h), g = h - fl;
    const uint32_t j = (uint32_t)fl;
    const double x0 = (double)key_value(k[j]), x1 = (double)key_value(k[min(j + 1, n - 1)]);
    return x0 + (x1 - x0) * g;
}

// fixed-order tree over groups of R consecutive threads whose partials the caller has stored in LDS: combine(i, j) folds slot j
// into slot i (buf[i] = buf[i] op buf[j], this operand order), the stride halves from R/2, the result lands in the group's first slot
template <int R, typename F>
__device__ __forceinline__ void group_tree(int t, F combine) {
    const int r = t % R;
    __syncthreads();
#pragma unroll
    for (int s = R / 2; s > 0; s >>= 1) {
        if (r < s) combine(t, t + s);
        __syncthreads();
    }
}

// bitonic network over ROWS independent rows of P keys (a power of two) at pitch PITCH in LDS, worked by the T threads of the
// workgroup; with PAYLOAD idx is swapped alongside.  Compare-exchange c works on row c / (P/2); the direction comes from the index
// within the row.  The caller synchronises before; every stage ends in a barrier.  K: the key type (uint32_t, or uint64_t in trend.hip).
template <int P, int ROWS, int PITCH, int T, bool PAYLOAD, typename K = uint32_t>
__device__ __forceinline__ void bitonic_rows(K* key, uint32_t* idx) {
    constexpr int LOGP = __builtin_ctz(P);
    static_assert((P & (P - 1)) == 0 && P >= 2, "bitonic_rows: P");
    for (int lk = 1; lk <= LOGP; ++lk) {
        for (int lj = lk - 1; lj >= 0; --lj) {
            for (int c = threadIdx.x; c < ROWS * (P / 2); c += T) {
                const int g = c >> (LOGP - 1), q = c & (P / 2 - 1);
                const int i = ((q >> lj) << (lj + 1)) | (q & ((1 << lj) - 1)), o = i + (1 << lj);
                const bool up = ((i >> lk) & 1) == 0;
                K* row = key + g * PITCH;
                const K a = row[i], b = row[o];
                if ((a > b) == up) {
                    row[i] = b; row[o] = a;
                    if constexpr (PAYLOAD) {
                        uint32_t* ri = idx + g * PITCH;
                        const uint32_t x = ri[i]; ri[i] = ri[o]; ri[o] = x;
                    }
                }
            }
            __syncthreads();
        }
    }
}

// ------------------------------------------------------------------------------------------------------------- radix passes
// Where a pass reads its keys: a buffer an earlier pass (or a gather kernel) wrote, or the float input with keys made on the fly,
// which is also where the index payload starts as the position and where a NaN is flagged: one flag per (segment, tile), stored
// (!nan_or: the first side of a pair) or only ever set (nan_or: the second side adds its own).
struct KeyBuffer {
    static constexpr bool FROM_INPUT = false;
    const uint32_t* k;
    __device__ __forceinline__ uint32_t key(size_t seg, size_t L, size_t pos, int&) const { return k[seg * L + pos]; }
};

struct FloatInput {
    static constexpr bool FROM_INPUT = true;
    const float* src;
    size_t ss, es;
    uint32_t* nanflag;
    int nan_or;
    __device__ __forceinline__ uint32_t key(size_t seg, size_t, size_t pos, int& nan) const {
        const float v = src[seg * ss + pos * es];
        nan |= (v != v);
        return rank_key(v);
    }
};

// the 64-bit mask of the lanes of this wave that are valid and carry the same 8-bit digit as this one
__device__ __forceinline__ uint64_t match_digit(uint32_t d, bool valid) {
    uint64_t m = __ballot(valid);
#pragma unroll
    for (int bit = 0; bit < 8; ++bit) {
        const uint64_t bl = __ballot((d >> bit) & 1u);
        m &= ((d >> bit) & 1u) ? bl : ~bl;
    }
    return m;
}

// per-(segment, tile) digit counts -> hist[(segment*ntiles + tile)*256 + digit]; from the float input also the tile's NaN flag
template <typename Src>
__global__ void __launch_bounds__(SORT_THREADS) radix_hist_kernel(const Src in, size_t L, const TileGrid grid, int shift,
                                                                  uint32_t* __restrict__ hist) {
    __shared__ uint32_t cnt[SORT_RADIX];
    __shared__ int nan_any;
    const int t = threadIdx.x, lane = t & 63;
    size_t seg, tile;
    grid.split(seg, tile);
    const size_t t0 = tile * SORT_TILE;
    cnt[t] = 0u;
    if constexpr (Src::FROM_INPUT) { if (t == 0) nan_any = 0; }
    __syncthreads();
    int nan = 0;
    for (int i = t; i < SORT_TILE; i += SORT_THREADS) {
        const size_t pos = t0 + i;
        const bool valid = pos < L;
        const uint32_t d = valid ? (in.key(seg, L, pos, nan) >> shift) & 255u : 0u;
        const uint64_t m = match_digit(d, valid);
        if (valid && (m & ((1ull << lane) - 1ull)) == 0ull) atomicAdd(&cnt[d], (uint32_t)__popcll(m));
    }
    if constexpr (Src::FROM_INPUT) { if (nan) nan_any = 1; }
    __syncthreads();
    hist[(size_t)blockIdx.x * SORT_RADIX + t] = cnt[t];
    if constexpr (Src::FROM_INPUT) {
        if (t == 0) {
            if (!in.nan_or) in.nanflag[blockIdx.x] = (uint32_t)nan_any;
            else if (nan_any) in.nanflag[blockIdx.x] = 1u;
        }
    }
}

// per segment (blockIdx.x, SORT_RADIX threads): hist[tile][digit] counts -> exclusive scatter offsets, digit-major then tile:
// off[t][d] = sum_{d' < d} total[d'] + sum_{t' < t} hist[t'][d]
__global__ void __launch_bounds__(SORT_RADIX) radix_scan_kernel(uint32_t* __restrict__ hist, int ntiles) {
    __shared__ uint32_t tot[SORT_RADIX];
    const int d = threadIdx.x;
    uint32_t* h = hist + (size_t)blockIdx.x * ntiles * SORT_RADIX + d;
    uint32_t run = 0;
    for (int t = 0; t < ntiles; ++t) {
        const uint32_t v = h[(size_t)t * SORT_RADIX];
        h[(size_t)t * SORT_RADIX] = run;
        run += v;
    }
    tot[d] = run;
    __syncthreads();
    for (int s = 1; s < SORT_RADIX; s <<= 1) {         // inclusive Hillis-Steele scan of the digit totals
        const uint32_t x = d >= s ? tot[d - s] : 0u;
        __syncthreads();
        tot[d] += x;
        __syncthreads();
    }
    const uint32_t base = tot[d] - run;
    for (int t = 0; t < ntiles; ++t) h[(size_t)t * SORT_RADIX] += base;
}

// stable scatter of one pass: wave w ranks its SORT_WAVE_SPAN consecutive elements per digit in order (chunks of 64, lanes in order
// by the match mask), the waves' counts are scanned in wave order, the segment's offsets of this tile come from the scan kernel.
// With PAYLOAD an index travels with every key (from the float input: its position)
template <typename Src, bool PAYLOAD>
__global__ void __launch_bounds__(SORT_THREADS) radix_scatter_kernel(const Src in, const uint32_t* __restrict__ iin, size_t L,
                                                                     const TileGrid grid, int shift, const uint32_t* __restrict__ off,
                                                                     uint32_t* __restrict__ kout, uint32_t* __restrict__ iout) {
    constexpr int CH = SORT_WAVE_SPAN / 64;
    __shared__ uint32_t wcnt[SORT_WAVES][SORT_RADIX];
    __shared__ uint32_t gofs[SORT_RADIX];
    const int t = threadIdx.x, lane = t & 63, w = t >> 6;
    size_t seg, tile;
    grid.split(seg, tile);
    for (int i = t; i < SORT_WAVES * SORT_RADIX; i += SORT_THREADS) wcnt[i / SORT_RADIX][i % SORT_RADIX] = 0u;
    gofs[t] = off[(size_t)blockIdx.x * SORT_RADIX + t];
    __syncthreads();
    const uint64_t lt = (1ull << lane) - 1ull;
    const size_t p0 = tile * SORT_TILE + (size_t)w * SORT_WAVE_SPAN + lane;
    uint32_t key[CH], id[PAYLOAD ? CH : 1], r[CH];
    int nan = 0;
#pragma unroll
    for (int c = 0; c < CH; ++c) {
        const size_t pos = p0 + (size_t)c * 64;
        const bool valid = pos < L;
        key[c] = valid ? in.key(seg, L, pos, nan) : 0u;
        if constexpr (PAYLOAD) id[c] = valid ? (Src::FROM_INPUT ? (uint32_t)pos : iin[seg * L + pos]) : 0u;
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
        for (int v = 0; v < SORT_WAVES; ++v) {
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
            if constexpr (PAYLOAD) iout[dst] = id[c];
        }
    }
}

template <typename Src, bool PAYLOAD>
void radix_pass(hipStream_t s, const Src& in, const uint32_t* iin, size_t ns, size_t L, unsigned nt, int shift, uint32_t* hist,
                uint32_t* kout, uint32_t* iout) {
    const dim3 grid((unsigned)(ns * nt)), block(SORT_THREADS);
    const TileGrid tg = tile_grid(nt);
    DL4DS_LAUNCH(radix_hist_kernel<Src>, grid, block, 0, s, in, L, tg, shift, hist);
    DL4DS_LAUNCH(radix_scan_kernel, dim3((unsigned)ns), dim3(SORT_RADIX), 0, s, hist, (int)nt);
    DL4DS_LAUNCH((radix_scatter_kernel<Src, PAYLOAD>), grid, block, 0, s, in, iin, L, tg, shift, (const uint32_t*)hist, kout, iout);
}

// sorts the ns segments of a chunk (L elements, nt tiles each) in four passes: `first` -> (k1, i1) -> (k0, i0) -> (k1, i1) ->
// (k0, i0), so the sorted keys end in k0 (which `first` may be: sorted in place through k1).  i0 / i1 are used with PAYLOAD only
template <bool PAYLOAD, typename Src>
void segmented_sort(hipStream_t s, const Src& first, uint32_t* k0, uint32_t* i0, uint32_t* k1, uint32_t* i1, size_t ns, size_t L,
                    unsigned nt, uint32_t* hist) {
    radix_pass<Src, PAYLOAD>(s, first, nullptr, ns, L, nt, 0, hist, k1, i1);
    for (int pass = 1; pass < 4; ++pass) {
        const bool odd = pass & 1;
        radix_pass<KeyBuffer, PAYLOAD>(s, KeyBuffer{odd ? k1 : k0}, odd ? i1 : i0, ns, L, nt, 8 * pass, hist, odd ? k0 : k1,
                                       odd ? i0 : i1);
    }
}

// ------------------------------------------------------------------------------------------------- chunks and the workspace
inline size_t al256(size_t b) { return (b + 255) & ~size_t(255); }

// Bump pointer that hands out 256-byte-aligned typed buffers.  A client describes its workspace once, as a struct W whose
// constructor W(carver, nseg, ntiles, L) takes its buffers of `nseg` segments: from a null base with nseg = 1 that gives the bytes
// per segment (`used`), from the workspace with the chunk's segments the pointers -- one description, so size and pointers cannot
// drift apart.
struct Carver {
    char* base;
    size_t used = 0;
    template <typename T>
    T* take(size_t n) {
        T* p = reinterpret_cast<T*>(reinterpret_cast<uintptr_t>(base) + used);
        used += al256(n * sizeof(T));
        return p;
    }
};

struct Chunk {
    size_t segs, ntiles, bytes_per_seg;                // segments per chunk, tiles per segment
    size_t bytes() const { return segs * bytes_per_seg; }
};

// as many segments of workspace W per chunk as the budget and the grid hold, at least one.  The grid cap never binds for a segment
// of more than SORT_TILE elements (rank.hip): bytes_per_seg >= 4*L > 2^13 * ntiles, so segs*ntiles <= 2^27 / 2^13 (and a segment
// beyond the budget runs alone with ntiles < 2^31 / SORT_TILE); it is there for short segments with a small footprint
template <typename W>
Chunk plan_chunks(size_t S, size_t L) {
    const size_t ntiles = std::max<size_t>(1, cdivz(L, SORT_TILE));
    Carver one{nullptr};
    const W measured(one, 1, ntiles, L);
    (void)measured;
    return {std::max<size_t>(1, std::min({S, SORT_WS_BUDGET / one.used, SORT_MAX_GRID / ntiles})), ntiles, one.used};
}

}  // namespace
