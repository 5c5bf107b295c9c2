// Neighbourhood verification of N*C fields (planes of two (N, H, W, C) arrays): per field, exceedance threshold and window size the
// three integer sums of the Fractions Skill Score (Roberts & Lean 2008), per field and threshold the 2 x 2 contingency table.
//
// A cell is VALID iff y and p are both finite there (NaN in y is the masking mechanism).  Indicators bo = valid & (y >= t),
// bf = valid & (p >= t).  The window of size n at cell (i, j) is rows [i - n/2, i - n/2 + n), columns likewise, clipped to the
// field; co / cf are the counts of bo / bf in it.  D = sum (cf - co)^2, F = sum cf^2, O = sum co^2 over ALL H*W cells, the
// contingency counts over the valid cells.  FSS = 1 - D / (F + O) follows on the host.  Everything here is integer arithmetic:
// integer sums are associative, so the 64-bit atomics below give the same bits in any order and the result EQUALS a reference.
//
// Two kernels per chunk of fields and group of at most FSS_TG thresholds:
//  * fss_prefix_kernel: a wave per row reads y and p once, 64 cells at a time.  For every threshold of the group the two
//    indicators are one __ballot each; the exclusive row prefix of lane l is popcount(mask below l) + the carry of the earlier
//    segments (a wave-uniform count), stored as uint16 (W <= 65535) or uint32 in rows of W + 1 entries.  The contingency
//    counts are popcounts of the same masks: wave-uniform, summed over the block's rows, one atomic per block and count.
//  * fss_window_kernel, per window size: a thread per column j holds the two column ends c0, c1 of its window and walks down the
//    rows with running sums: the entering row adds P[c1] - P[c0], the leaving row subtracts it.  Reads are coalesced along j, the
//    work per cell does not depend on n, no 2-D table exists.  Squares are 32-bit while min(n, H) * min(n, W) <= 65535 and 64-bit
//    beyond; per-thread 64-bit sums, a wave reduction, one atomic per workgroup and sum.  Tall fields are cut into bands of rows
//    when the grid would otherwise be small; a band starts by summing its first window (at most n rows).
// Fields go through in chunks sized by a fixed workspace budget; a threshold group of one field larger than it runs alone.
#include "common.h"
#include "ops.h"
#include "prof.h"
#include <algorithm>
#include <cmath>

namespace {

constexpr int FSS_TG = 8;                              // thresholds per group (their carries and counts live in registers)
constexpr int FSS_THREADS = 256;                       // both kernels: 4 waves
constexpr int FSS_WAVES = FSS_THREADS / 64;
constexpr int FSS_PREFIX_ROWS = 32;                    // rows per workgroup of the prefix kernel (8 per wave)
constexpr int FSS_BAND_MIN = 32;                       // window kernel: fewest rows of a band
constexpr size_t FSS_TARGET_BLOCKS = 2048;             // window kernel: bands are made until the grid has about this many blocks
constexpr size_t FSS_WS_BUDGET = size_t(128) << 20;    // workspace of one chunk of fields
constexpr size_t FSS_MAX_CHUNK_FIELDS = 32768;
constexpr int FSS_NCNT = 3 * FSS_TG + 1;               // per threshold: hits, observed events, forecast events; + the valid count

struct FssThresholds {
    float t[FSS_TG];
    int count;
};

__device__ __forceinline__ bool finite_bits(float v) { return (__float_as_uint(v) & 0x7f800000u) != 0x7f800000u; }

// prefix[((f * tcount + k) * 2 + side) * H + row][0 .. W] for field f of the chunk, threshold k of the group, side 0 = observation
template <typename PT>
__global__ void __launch_bounds__(FSS_THREADS) fss_prefix_kernel(const float* __restrict__ y, const float* __restrict__ p, int H,
                                                                 int W, int C, size_t field0, FssThresholds thr, int T, int t0,
                                                                 PT* __restrict__ prefix, unsigned long long* __restrict__ cont,
                                                                 unsigned long long* __restrict__ valid_out) {
    __shared__ unsigned long long cnt[FSS_WAVES][FSS_NCNT];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int bands = (H + FSS_PREFIX_ROWS - 1) / FSS_PREFIX_ROWS;
    const size_t fl = blockIdx.x / (unsigned)bands;                        // field of the chunk
    const int band = (int)(blockIdx.x % (unsigned)bands);
    const size_t g = field0 + fl;                                         // field of the call: sample g / C, channel g % C
    const size_t base = (g / (size_t)C) * ((size_t)H * W * C) + g % (size_t)C;
    const size_t rs = (size_t)W + 1;                                      // entries per prefix row
    const uint64_t below = (1ull << lane) - 1ull;
    const int r1 = min((band + 1) * FSS_PREFIX_ROWS, H);
    unsigned long long hits[FSS_TG] = {}, nobs[FSS_TG] = {}, nfc[FSS_TG] = {}, nvalid = 0;
    for (int r = band * FSS_PREFIX_ROWS + wave; r < r1; r += FSS_WAVES) {
        uint32_t co[FSS_TG] = {}, cf[FSS_TG] = {};
        const size_t rowbase = base + (size_t)r * W * C;
        for (int j0 = 0; j0 < W; j0 += 64) {
            const int j = j0 + lane;
            const bool in = j < W;
            const size_t o = rowbase + (size_t)(in ? j : 0) * C;
            const float yv = y[o], pv = p[o];
            const bool ok = in && finite_bits(yv) && finite_bits(pv);
            nvalid += (unsigned)__popcll(__ballot(ok));
#pragma unroll
            for (int k = 0; k < FSS_TG; ++k) {
                if (k < thr.count) {                                      // uniform
                    const uint64_t mo = __ballot(ok && yv >= thr.t[k]), mf = __ballot(ok && pv >= thr.t[k]);
                    if (in) {
                        PT* po = prefix + (((fl * thr.count + k) * 2) * (size_t)H + r) * rs;
                        PT* pf = po + (size_t)H * rs;
                        if (j == 0) { po[0] = (PT)0; pf[0] = (PT)0; }
                        const uint64_t upto = below | (1ull << lane);
                        po[j + 1] = (PT)(co[k] + (uint32_t)__popcll(mo & upto));
                        pf[j + 1] = (PT)(cf[k] + (uint32_t)__popcll(mf & upto));
                    }
                    const uint32_t no = (uint32_t)__popcll(mo), nf = (uint32_t)__popcll(mf);
                    co[k] += no; cf[k] += nf;
                    nobs[k] += no; nfc[k] += nf;
                    hits[k] += (unsigned)__popcll(mo & mf);
                }
            }
        }
    }
    if (lane == 0) {
#pragma unroll
        for (int k = 0; k < FSS_TG; ++k) {
            cnt[wave][3 * k] = hits[k]; cnt[wave][3 * k + 1] = nobs[k]; cnt[wave][3 * k + 2] = nfc[k];
        }
        cnt[wave][3 * FSS_TG] = nvalid;
    }
    __syncthreads();
    const int k = threadIdx.x;
    if (k <= thr.count) {
        unsigned long long v = 0;
        for (int w = 0; w < FSS_WAVES; ++w) v += cnt[w][3 * FSS_TG];
        if (k == thr.count) {
            if (valid_out) atomicAdd(valid_out + g, v);
        } else {
            unsigned long long h = 0, ob = 0, fc = 0;
            for (int w = 0; w < FSS_WAVES; ++w) { h += cnt[w][3 * k]; ob += cnt[w][3 * k + 1]; fc += cnt[w][3 * k + 2]; }
            unsigned long long* c = cont + (g * (size_t)T + (size_t)(t0 + k)) * 4;
            atomicAdd(c + 0, h);                                          // hits
            atomicAdd(c + 1, ob - h);                                     // misses
            atomicAdd(c + 2, fc - h);                                     // false alarms
            atomicAdd(c + 3, v + h - ob - fc);                            // correct negatives (valid, neither)
        }
    }
}

__device__ __forceinline__ unsigned long long wave_sum_u64(unsigned long long v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
    return v;
}

// blockIdx.x = ((f * tcount + k) * nbands + band) * colblocks + column block.  half = n / 2 of the (clamped) window size n.
template <typename PT, bool WIDE>
__global__ void __launch_bounds__(FSS_THREADS) fss_window_kernel(const PT* __restrict__ prefix, int H, int W, int tcount,
                                                                 long long n, long long half, int band_rows, int nbands,
                                                                 size_t field0, int T, int t0, int S, int s,
                                                                 unsigned long long* __restrict__ sums) {
    __shared__ unsigned long long red[FSS_WAVES][3];
    const unsigned colblocks = (unsigned)((W + FSS_THREADS - 1) / FSS_THREADS);
    unsigned b = blockIdx.x;
    const int j = (int)(b % colblocks) * FSS_THREADS + (int)threadIdx.x;
    b /= colblocks;
    const int band = (int)(b % (unsigned)nbands);
    b /= (unsigned)nbands;
    const int k = (int)(b % (unsigned)tcount);
    const size_t fl = b / (unsigned)tcount;
    const size_t rs = (size_t)W + 1;
    const PT* po = prefix + ((fl * tcount + k) * 2) * (size_t)H * rs;
    const PT* pf = po + (size_t)H * rs;
    unsigned long long d2 = 0, f2 = 0, o2 = 0;
    if (j < W) {
        const int c0 = (int)max((long long)j - half, 0ll), c1 = (int)min((long long)j - half + n, (long long)W);
        const int r0 = band * band_rows, r1 = min(r0 + band_rows, H);
        const int lo = (int)max((long long)r0 - half, 0ll), hi = (int)min((long long)r0 - half + n, (long long)H);
        uint32_t so = 0, sf = 0;                                          // window counts of the current row
        for (int r = lo; r < hi; ++r) {
            so += (uint32_t)po[r * rs + c1] - (uint32_t)po[r * rs + c0];
            sf += (uint32_t)pf[r * rs + c1] - (uint32_t)pf[r * rs + c0];
        }
        for (int i = r0; i < r1; ++i) {
            const uint32_t ad = sf > so ? sf - so : so - sf;
            if (WIDE) {
                d2 += (unsigned long long)ad * ad; f2 += (unsigned long long)sf * sf; o2 += (unsigned long long)so * so;
            } else {
                d2 += ad * ad; f2 += sf * sf; o2 += so * so;              // counts <= 65535: the squares fit 32 bits
            }
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
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) { red[wave][0] = d2; red[wave][1] = f2; red[wave][2] = o2; }
    __syncthreads();
    if (threadIdx.x < 3) {
        unsigned long long v = 0;
        for (int w = 0; w < FSS_WAVES; ++w) v += red[w][threadIdx.x];
        if (v) atomicAdd(sums + (((field0 + fl) * (size_t)T + (size_t)(t0 + k)) * S + s) * 3 + threadIdx.x, v);
    }
}

struct Plan {
    size_t esize;                                      // bytes of a prefix entry
    size_t bytes_per_field;                            // one threshold group of one field
    size_t fields;                                     // fields per chunk
};

Plan plan(size_t fields, int H, int W, int T) {
    Plan pl;
    pl.esize = W <= 65535 ? 2 : 4;
    pl.bytes_per_field = (size_t)std::min(T, FSS_TG) * 2 * (size_t)H * ((size_t)W + 1) * pl.esize;
    pl.fields = std::max<size_t>(1, std::min({fields, FSS_WS_BUDGET / pl.bytes_per_field, FSS_MAX_CHUNK_FIELDS}));
    return pl;
}

template <typename PT>
void run(hipStream_t st, const float* y, const float* p, int N, int H, int W, int C, const float* thresholds, int T,
         const int* windows, int S, unsigned long long* sums, unsigned long long* cont, unsigned long long* valid, void* workspace) {
    const size_t fields = (size_t)N * C;
    const Plan pl = plan(fields, H, W, T);
    PT* prefix = static_cast<PT*>(workspace);
    const size_t pbands = cdivz(H, FSS_PREFIX_ROWS), colblocks = cdivz(W, FSS_THREADS);
    const long long cover = 2ll * std::max(H, W);      // a window this large holds the whole field from every cell
    const double cells = (double)fields * H * W;
    for (size_t f0 = 0; f0 < fields; f0 += pl.fields) {
        const size_t nf = std::min(pl.fields, fields - f0);
        for (int t0 = 0; t0 < T; t0 += FSS_TG) {
            FssThresholds thr;
            thr.count = std::min(FSS_TG, T - t0);
            for (int k = 0; k < FSS_TG; ++k) thr.t[k] = k < thr.count ? thresholds[t0 + k] : 0.f;
            {
                ProfScope ps(st, "fss_prefix", 0.0, cells / fields * nf * (8.0 + 2.0 * thr.count * sizeof(PT)));
                DL4DS_LAUNCH(fss_prefix_kernel<PT>, dim3((unsigned)(nf * pbands)), dim3(FSS_THREADS), 0, st, y, p, H, W, C, f0, thr, T,
                             t0, prefix, cont, t0 == 0 ? valid : nullptr);
            }
            for (int s = 0; s < S; ++s) {
                const long long n = std::min<long long>(windows[s], cover), half = n / 2;
                const unsigned long long m = (unsigned long long)std::min<long long>(n, H) * std::min<long long>(n, W);
                // bands of rows when the grid would be small; at least n rows each, so a band's start-up reads stay below its own
                const size_t base_blocks = nf * thr.count * colblocks;
                const size_t want = std::max<size_t>(1, FSS_TARGET_BLOCKS / base_blocks);
                const long long rows = std::min<long long>(H, std::max<long long>({(long long)cdivz(H, want), n, FSS_BAND_MIN}));
                const int band_rows = (int)rows, nbands = (int)cdivz(H, band_rows);
                const size_t grid = base_blocks * nbands;
                DL4DS_REQUIRE(grid < (size_t(1) << 31), "fss: grid too large");
                ProfScope ps(st, "fss_window", 0.0, cells / fields * nf * thr.count * 8.0 * sizeof(PT));
                const auto kern = m <= 65535ull ? fss_window_kernel<PT, false> : fss_window_kernel<PT, true>;
                DL4DS_LAUNCH(kern, dim3((unsigned)grid), dim3(FSS_THREADS), 0, st, (const PT*)prefix, H, W, thr.count, n, half,
                             band_rows, nbands, f0, T, t0, S, s, sums);
            }
        }
    }
}

}  // namespace

size_t fss_workspace_bytes(int N, int H, int W, int C, int T) {
    if (N <= 0 || H <= 0 || W <= 0 || C <= 0 || T <= 0) return 0;
    const Plan pl = plan((size_t)N * C, H, W, T);
    return pl.fields * pl.bytes_per_field;
}

void fss_check_args(int N, int H, int W, int C, const float* thresholds, int T, const int* windows, int S) {
    DL4DS_REQUIRE(N >= 0 && H >= 1 && W >= 1 && C >= 1, "fss: expected N >= 0 and H, W, C >= 1");
    DL4DS_REQUIRE(T >= 1 && S >= 1 && thresholds && windows, "fss: at least one threshold and one window are needed");
    DL4DS_REQUIRE((long long)H * W < (1ll << 31), "fss: fields of 2^31 or more cells are not supported");
    DL4DS_REQUIRE((long long)N * C < (1ll << 31), "fss: too many fields");
    for (int k = 0; k < T; ++k) DL4DS_REQUIRE(std::isfinite(thresholds[k]), "fss: thresholds must be finite");
    for (int s = 0; s < S; ++s) {
        DL4DS_REQUIRE(windows[s] >= 1, "fss: window sizes must be positive");
        const unsigned __int128 m = (unsigned __int128)std::min(windows[s], H) * (unsigned)std::min(windows[s], W);
        DL4DS_REQUIRE((unsigned __int128)H * (unsigned)W * m * m < ((unsigned __int128)1 << 62),
                      "fss: H*W*m^2 with m = min(n, H)*min(n, W) must stay below 2^62 for the exact 64-bit sums");
    }
}

void fss(hipStream_t st, const float* y, const float* p, int N, int H, int W, int C, const float* thresholds, int T,
         const int* windows, int S, long long* sums, long long* cont, long long* valid, void* workspace, size_t workspace_bytes) {
    fss_check_args(N, H, W, C, thresholds, T, windows, S);
    if (N == 0) return;
    DL4DS_REQUIRE(workspace_bytes >= fss_workspace_bytes(N, H, W, C, T), "fss workspace too small");
    const size_t fields = (size_t)N * C;
    HIP_CHECK(hipMemsetAsync(sums, 0, fields * T * S * 3 * sizeof(long long), st));
    HIP_CHECK(hipMemsetAsync(cont, 0, fields * T * 4 * sizeof(long long), st));
    HIP_CHECK(hipMemsetAsync(valid, 0, fields * sizeof(long long), st));
    auto* us = reinterpret_cast<unsigned long long*>(sums);
    auto* uc = reinterpret_cast<unsigned long long*>(cont);
    auto* uv = reinterpret_cast<unsigned long long*>(valid);
    if (W <= 65535) run<uint16_t>(st, y, p, N, H, W, C, thresholds, T, windows, S, us, uc, uv, workspace);
    else run<uint32_t>(st, y, p, N, H, W, C, thresholds, T, windows, S, us, uc, uv, workspace);
}
