// What the two neighbourhood scores share (fss.hip, ensemble_fss.hip): the launch constants, the layout of
// the row prefixes and of the outputs that a prefix kernel and the window walk agree on, the window walk itself, the chunk planner
// and the host driver over chunks of fields x groups of thresholds x window sizes, the argument rules and the entry prologue.
// Each score keeps its own prefix kernel and a thin __global__ wrapper around the walk.  fss is the K = 1 case throughout.
#pragma once
#include "common.h"
#include "prof.h"
#include <algorithm>
#include <cmath>

namespace {

constexpr int NB_TG = 8;                               // thresholds per group (their carries and counts live in registers)
constexpr int NB_THREADS = 256;                        // every kernel: 4 waves
constexpr int NB_WAVES = NB_THREADS / 64;
constexpr int NB_PREFIX_ROWS = 32;                     // rows per workgroup of a prefix kernel (8 per wave)
constexpr int NB_BAND_MIN = 32;                        // window walk: fewest rows of a band
constexpr size_t NB_TARGET_BLOCKS = 2048;              // window walk: bands are made until the grid has about this many blocks
constexpr size_t NB_WS_BUDGET = size_t(128) << 20;     // workspace of one chunk of fields
constexpr size_t NB_MAX_CHUNK_FIELDS = 32768;
constexpr size_t NB_NARROW_MAX = 65535;                // largest K * W with 16-bit prefixes, largest K * m squared in 32 bits

struct NbThresholds {
    float t[NB_TG];                                    // an unused slot holds +inf: no finite value reaches it, its counters are never read
    int count;
};

// ---------------------------------------------------------------------------------------------------------------------- layout
// first cell of field g of the call (sample g / C, channel g % C) in an (N, H, W, C) array; its cells are C apart
__device__ __forceinline__ size_t nb_field_base(size_t g, int H, int W, int C) {
    return (g / (size_t)C) * ((size_t)H * W * C) + g % (size_t)C;
}

// prefix[((fl * tcount + k) * 2 + side) * H + r][0 .. W]: row r of field fl of the chunk, threshold k of the group; side 0 (.o) is
// the observation, side 1 (.f) the forecast, H rows further on
template <typename P>
struct NbRows {
    P* o;
    P* f;
};
template <typename P>
__device__ __forceinline__ NbRows<P> nb_prefix_rows(P* prefix, size_t fl, int tcount, int k, int H, int W, size_t r) {
    const size_t rs = (size_t)W + 1;
    P* po = prefix + (((fl * tcount + k) * 2) * (size_t)H + r) * rs;
    return {po, po + (size_t)H * rs};
}

// cont[g][t][0 .. per) and sums[g][t][s][0 .. per) of field g of the call, threshold t of the call, window s
__device__ __forceinline__ size_t nb_cont_at(size_t g, int T, int t, int per) { return (g * (size_t)T + (size_t)t) * per; }
__device__ __forceinline__ size_t nb_sums_at(size_t g, int T, int t, int S, int s, int per) {
    return ((g * (size_t)T + (size_t)t) * S + s) * per;
}

// ------------------------------------------------------------------------------------------------------------- the window walk
// One window size.  blockIdx.x = ((f * tcount + k) * nbands + band) * colblocks + column block; half = n / 2 of the (clamped) window
// size n.  A thread per column j holds the two column ends c0, c1 of its window and walks down the rows of its band with running
// sums so / sf of the two sides: the entering row adds P[c1] - P[c0], the leaving row subtracts it; a band starts by summing its
// first window (at most n rows).  The sums are modulo 2^32 (a 32-bit prefix may wrap): every window sum is < 2^31, so exact.
// Per cell D += (sf - K so)^2, F += sf^2, O += so^2; WIDE: K * m > 65535, the squares need 64-bit multiplies.  ENSEMBLE adds
// Fv += sf^2 at valid centre cells (bit j & 63 of vbits[(fl * H + i) * words + j / 64]) and X += sf at centre cells whose
// o = P[j + 1] - P[j] is 1; without it K = 1, vbits is not read and only three sums exist.  64-bit sums per thread, a wave
// reduction, one atomic per workgroup and sum.
template <typename PT, bool WIDE, bool ENSEMBLE>
__device__ __forceinline__ void nb_window_walk(const PT* __restrict__ prefix, const unsigned long long* __restrict__ vbits, uint32_t K,
                                               int H, int W, int tcount, long long n, long long half, int band_rows, int nbands,
                                               size_t field0, int T, int t0, int S, int s, unsigned long long* __restrict__ sums) {
    constexpr int NSUMS = ENSEMBLE ? 5 : 3;
    __shared__ unsigned long long red[NB_WAVES][NSUMS];
    const unsigned colblocks = (unsigned)((W + NB_THREADS - 1) / NB_THREADS);
    unsigned b = blockIdx.x;
    const int j = (int)(b % colblocks) * NB_THREADS + (int)threadIdx.x;
    b /= colblocks;
    const int band = (int)(b % (unsigned)nbands);
    b /= (unsigned)nbands;
    const int k = (int)(b % (unsigned)tcount);
    const size_t fl = b / (unsigned)tcount;
    const size_t rs = (size_t)W + 1;
    const NbRows<const PT> rows = nb_prefix_rows(prefix, fl, tcount, k, H, W, 0);
    const PT* po = rows.o;
    const PT* pf = rows.f;
    const size_t words = ((size_t)W + 63) / 64;
    const unsigned long long* vb = nullptr;
    if constexpr (ENSEMBLE) vb = vbits + fl * (size_t)H * words + (size_t)(j >> 6);
    unsigned long long d2 = 0, f2 = 0, o2 = 0, fv = 0, xs = 0;
    if (j < W) {
        const int c0 = (int)max((long long)j - half, 0ll), c1 = (int)min((long long)j - half + n, (long long)W);
        const int r0 = band * band_rows, r1 = min(r0 + band_rows, H);
        const int lo = (int)max((long long)r0 - half, 0ll), hi = (int)min((long long)r0 - half + n, (long long)H);
        uint32_t so = 0, sf = 0;                                          // window sums of the current row
        for (int r = lo; r < hi; ++r) {
            so += (uint32_t)po[r * rs + c1] - (uint32_t)po[r * rs + c0];
            sf += (uint32_t)pf[r * rs + c1] - (uint32_t)pf[r * rs + c0];
        }
        // !WIDE: counts <= 65535, the squares fit 32 bits
        const auto sq = [](uint32_t v) { if constexpr (WIDE) return (unsigned long long)v * v; else return v * v; };
        for (int i = r0; i < r1; ++i) {
            uint32_t ko = so;
            if constexpr (ENSEMBLE) ko = K * so;                          // <= K m < 2^31
            const uint32_t ad = sf > ko ? sf - ko : ko - sf;
            bool ov = false, vc = false;
            if constexpr (ENSEMBLE) {
                ov = (uint32_t)po[(size_t)i * rs + j + 1] != (uint32_t)po[(size_t)i * rs + j];             // the centre cell's o
                vc = (vb[(size_t)i * words] >> (j & 63)) & 1ull;                                           // and its validity
            }
            d2 += sq(ad);
            const auto q = sq(sf);
            f2 += q; o2 += sq(so);
            fv += vc ? q : 0;
            xs += ov ? sf : 0u;
            const long long enter = (long long)i - half + n, leave = (long long)i - half;
            if (enter < H) {
                so += (uint32_t)po[(size_t)enter * rs + c1] - (uint32_t)po[(size_t)enter * rs + c0];
                sf += (uint32_t)pf[(size_t)enter * rs + c1] - (uint32_t)pf[(size_t)enter * rs + c0];
            }
            if (leave >= 0) {
                so -= (uint32_t)po[(size_t)leave * rs + c1] - (uint32_t)po[(size_t)leave * rs + c0];
                sf -= (uint32_t)pf[(size_t)leave * rs + c1] - (uint32_t)pf[(size_t)leave * rs + c0];
            }
        }
    }
    d2 = wave_sum_u64(d2); f2 = wave_sum_u64(f2); o2 = wave_sum_u64(o2);
    if constexpr (ENSEMBLE) { fv = wave_sum_u64(fv); xs = wave_sum_u64(xs); }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) {
        red[wave][0] = d2; red[wave][1] = f2; red[wave][2] = o2;
        if constexpr (ENSEMBLE) { red[wave][3] = fv; red[wave][4] = xs; }
    }
    __syncthreads();
    if (threadIdx.x < NSUMS) {
        unsigned long long v = 0;
        for (int w = 0; w < NB_WAVES; ++w) v += red[w][threadIdx.x];
        if (v) atomicAdd(sums + nb_sums_at(field0 + fl, T, t0 + k, S, s, NSUMS) + threadIdx.x, v);
    }
}

// ------------------------------------------------------------------------------------------------------------------- the host
struct NbPlan {
    size_t bytes_per_field;                            // one threshold group of one field: prefixes and the caller's extra bytes
    size_t fields;                                     // fields per chunk
    size_t bytes() const { return fields * bytes_per_field; }
};

inline size_t nb_esize(size_t K, int W) { return K * (size_t)W <= NB_NARROW_MAX ? 2 : 4; }

inline NbPlan nb_plan(size_t fields, int H, int W, int T, size_t esize, size_t extra_bytes_per_field) {
    NbPlan pl;
    pl.bytes_per_field = (size_t)std::min(T, NB_TG) * 2 * (size_t)H * ((size_t)W + 1) * esize + extra_bytes_per_field;
    pl.fields = std::max<size_t>(1, std::min({fields, NB_WS_BUDGET / pl.bytes_per_field, NB_MAX_CHUNK_FIELDS}));
    return pl;
}

// what the driver hands to the caller's launches: a chunk of fields with a group of thresholds, and one window size on it
struct NbGroup {
    size_t f0, nf;                                     // fields [f0, f0 + nf) of the call
    NbThresholds thr;                                  // thresholds [t0, t0 + thr.count) of the call
    int t0;
    unsigned prefix_grid;                              // nf * ceil(H / NB_PREFIX_ROWS)
};
struct NbWindow {
    long long n, half;                                 // the clamped window size and n / 2
    int band_rows, nbands, s;
    unsigned grid;
    bool wide;                                         // K * min(n, H) * min(n, W) > 65535
};

// Walks chunks of `chunk_fields` fields x groups of NB_TG thresholds x the S window sizes: per group launch_prefix(group), then
// per window launch_window(group, window), each inside its profiler scope `who`_prefix / `who`_window.  PT is the prefix type,
// window_reads the prefix entries the window kernel reads per cell and threshold (8 of the walk, 2 more for the centre cell).
template <typename PT, typename Prefix, typename Window>
void nb_run(hipStream_t st, const char* who, size_t K, size_t fields, int H, int W, const float* thresholds, int T,
            const int* windows, int S, size_t chunk_fields, double window_reads, Prefix launch_prefix, Window launch_window) {
    const std::string name(who);
    const size_t pbands = cdivz(H, NB_PREFIX_ROWS), colblocks = cdivz(W, NB_THREADS);
    const long long cover = 2ll * std::max(H, W);      // a window this large holds the whole field from every cell
    const double cells = (double)H * W;
    for (size_t f0 = 0; f0 < fields; f0 += chunk_fields) {
        const size_t nf = std::min(chunk_fields, fields - f0);
        DL4DS_REQUIRE(nf * pbands < (size_t(1) << 31), name + ": grid too large");
        for (int t0 = 0; t0 < T; t0 += NB_TG) {
            NbGroup g{f0, nf, {}, t0, (unsigned)(nf * pbands)};
            g.thr.count = std::min(NB_TG, T - t0);
            for (int k = 0; k < NB_TG; ++k) g.thr.t[k] = k < g.thr.count ? thresholds[t0 + k] : INFINITY;
            {
                ProfScope ps(st, name + "_prefix", 0.0, cells * nf * (4.0 * (double)(K + 1) + 2.0 * g.thr.count * sizeof(PT)));
                launch_prefix(g);
            }
            for (int s = 0; s < S; ++s) {
                NbWindow w;
                w.n = std::min<long long>(windows[s], cover);
                w.half = w.n / 2;
                w.s = s;
                const unsigned long long m = (unsigned long long)std::min<long long>(w.n, H) * std::min<long long>(w.n, W);
                w.wide = K * m > NB_NARROW_MAX;
                // bands of rows when the grid would be small; at least n rows each, so a band's start-up reads stay below its own
                const size_t base_blocks = nf * g.thr.count * colblocks;
                const size_t want = std::max<size_t>(1, NB_TARGET_BLOCKS / base_blocks);
                w.band_rows = (int)std::min<long long>(H, std::max<long long>({(long long)cdivz(H, want), w.n, NB_BAND_MIN}));
                w.nbands = (int)cdivz(H, w.band_rows);
                const size_t grid = base_blocks * w.nbands;
                DL4DS_REQUIRE(grid < (size_t(1) << 31), name + ": grid too large");
                w.grid = (unsigned)grid;
                ProfScope ps(st, name + "_window", 0.0, cells * nf * g.thr.count * window_reads * sizeof(PT));
                launch_window(g, w);
            }
        }
    }
}

// the rules both entries share, for K members (fss: 1) and `fields` fields of H x W cells; sum_bound names the bounded product
inline void nb_check_args(const char* entry, const char* sum_bound, size_t K, unsigned __int128 fields, int H, int W,
                          const float* thresholds, int T, const int* windows, int S) {
    const std::string who(entry);
    DL4DS_REQUIRE((long long)H * W < (1ll << 31), who + ": fields of 2^31 or more cells are not supported");
    DL4DS_REQUIRE(fields < ((unsigned __int128)1 << 31), who + ": too many fields");
    for (int k = 0; k < T; ++k) DL4DS_REQUIRE(std::isfinite(thresholds[k]), who + ": thresholds must be finite");
    for (int s = 0; s < S; ++s) {
        DL4DS_REQUIRE(windows[s] >= 1, who + ": window sizes must be positive");
        const unsigned __int128 km = (unsigned __int128)K * (unsigned)std::min(windows[s], H) * (unsigned)std::min(windows[s], W);
        DL4DS_REQUIRE((unsigned __int128)H * (unsigned)W * km * km < ((unsigned __int128)1 << 62),
                      who + ": " + sum_bound + " with m = min(n, H)*min(n, W) must stay below 2^62 for the exact 64-bit sums");
    }
}

// Zeroes the outputs (nsums sums per field, threshold and window; ncont counts per field and threshold; the valid count per
// field) and calls run(PT(), sums, cont, valid) with the unsigned views and the prefix type: uint16 while K * W <= 65535
template <typename Run>
void nb_enter(hipStream_t st, size_t K, size_t fields, int W, int T, int S, int nsums, int ncont, long long* sums, long long* cont,
              long long* valid, Run run) {
    HIP_CHECK(hipMemsetAsync(sums, 0, fields * T * S * nsums * sizeof(long long), st));
    HIP_CHECK(hipMemsetAsync(cont, 0, fields * T * ncont * sizeof(long long), st));
    HIP_CHECK(hipMemsetAsync(valid, 0, fields * sizeof(long long), st));
    auto* us = reinterpret_cast<unsigned long long*>(sums);
    auto* uc = reinterpret_cast<unsigned long long*>(cont);
    auto* uv = reinterpret_cast<unsigned long long*>(valid);
    if (nb_esize(K, W) == 2) run(uint16_t(), us, uc, uv);
    else run(uint32_t(), us, uc, uv);
}

}  // namespace
