// Neighbourhood verification of an MC-dropout ensemble as a PROBABILITY forecast: the member stack
// members[K][n] and the observation obs[n] are B whole samples of shape (H, W, C), each of the B*C planes is a field.  Per field,
// threshold and window size the five integer sums behind the Fractions Skill Score of the neighbourhood ensemble probability and
// the neighbourhood Brier score, per field and threshold the event counts of either side.
//
// A cell is VALID iff its observation and all K members are finite (NaN in obs is the masking mechanism).  Per valid cell and
// threshold t, on float32: o = [obs >= t], c = #{k : x_k >= t} (0 ... K); invalid cells have o = c = 0.  The window of size n at
// cell (i, j) is exactly fss.hip's: rows [i - n/2, i - n/2 + n), columns likewise, clipped to the field.  co / cf are the sums of
// o / c over it, co <= m = min(n, H) * min(n, W), cf <= K m.  Over ALL H*W cells D = sum (cf - K co)^2, F = sum cf^2, O = sum co^2;
// over the valid centre cells Fv = sum cf^2; over the centre cells with o = 1 X = sum cf.  E = sum o, Cs = sum c.  Integer
// arithmetic only: the 64-bit atomics give the same bits in any order and the result EQUALS an integer reference.
//
// Two kernels per chunk of fields and group of at most EFSS_TG thresholds (the shape of fss.hip's pair):
//  * efss_prefix_kernel: a wave per row, 64 cells per step, one lane per cell (stride C inside a plane).  The lane reads its
//    observation and walks the K member rows (adjacent lanes read adjacent cells of every row: coalesced), with up to EFSS_TG
//    threshold counters in registers; a non-finite value zeroes them.  MORE THAN EFSS_TG THRESHOLDS MEAN ANOTHER PASS OVER THE
//    STACK per further group (T = 9 ... 16: two reads of (K + 1) * 4 B per cell).  No per-cell count array goes to memory: the
//    observed indicator becomes a __ballot / popcount prefix as in fss.hip, the member count a wave-inclusive scan (__shfl_up, six
//    steps) whose lane 63 carries the wave-uniform total into the next segment.  Exclusive row prefixes P[0 .. W] of both sides
//    are stored as uint16 while K * W <= 65535 and as uint32 beyond; 32-bit prefixes may wrap (K * W can pass 2^32 on a single
//    long row): every difference the window kernel takes is a window count < 2^31, exact modulo 2^32.  The validity of the row
//    is one ballot word per segment (a bit-plane).  E, Cs and n_valid are wave-uniform: one atomic per workgroup and counter.
//  * efss_window_kernel, per window size: the walk of fss_window_kernel (a thread per column, two running sums per side, bands
//    of rows when the grid would be small), plus per row the centre cell's o = P[j + 1] - P[j] and its validity bit.  Squares
//    are 32-bit multiplies while K * m <= 65535 and 64-bit beyond.
// Fields go through in chunks sized by the same fixed workspace budget as fss.hip; the result does not depend on the chunking.
#include "common.h"
#include "ops.h"
#include "prof.h"
#include <algorithm>
#include <cmath>

namespace {

constexpr int EFSS_TG = 8;                             // thresholds per pass over the stack (their counters live in registers)
constexpr int EFSS_THREADS = 256;                      // both kernels: 4 waves
constexpr int EFSS_WAVES = EFSS_THREADS / 64;
constexpr int EFSS_PREFIX_ROWS = 32;                   // rows per workgroup of the prefix kernel (8 per wave)
constexpr int EFSS_BAND_MIN = 32;                      // window kernel: fewest rows of a band
constexpr size_t EFSS_TARGET_BLOCKS = 2048;            // window kernel: bands are made until the grid has about this many blocks
constexpr size_t EFSS_WS_BUDGET = size_t(128) << 20;   // workspace of one chunk of fields
constexpr size_t EFSS_MAX_CHUNK_FIELDS = 32768;
constexpr int EFSS_NCNT = 2 * EFSS_TG + 1;             // per threshold: observed events, member events; + the valid count

struct EfssThresholds {
    float t[EFSS_TG];
    int count;
};

__device__ __forceinline__ bool efss_finite(float v) { return (__float_as_uint(v) & 0x7f800000u) != 0x7f800000u; }

// prefix[((f * tcount + k) * 2 + side) * H + row][0 .. W] for field f of the chunk, threshold k of the group, side 0 = observation;
// vbits[(f * H + row) * words + segment]: bit l = validity of cell 64 * segment + l
template <typename PT>
__global__ void __launch_bounds__(EFSS_THREADS) efss_prefix_kernel(const float* __restrict__ members, size_t stride, int K,
                                                                   const float* __restrict__ obs, int H, int W, int C, size_t field0,
                                                                   EfssThresholds thr, int T, int t0, PT* __restrict__ prefix,
                                                                   unsigned long long* __restrict__ vbits,
                                                                   unsigned long long* __restrict__ cont,
                                                                   unsigned long long* __restrict__ valid_out) {
    __shared__ unsigned long long cnt[EFSS_WAVES][EFSS_NCNT];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int bands = (H + EFSS_PREFIX_ROWS - 1) / EFSS_PREFIX_ROWS;
    const size_t fl = blockIdx.x / (unsigned)bands;                       // field of the chunk
    const int band = (int)(blockIdx.x % (unsigned)bands);
    const size_t g = field0 + fl;                                         // field of the call: sample g / C, channel g % C
    const size_t base = (g / (size_t)C) * ((size_t)H * W * C) + g % (size_t)C;
    const size_t rs = (size_t)W + 1;                                      // entries per prefix row
    const size_t words = ((size_t)W + 63) / 64;                           // validity words per row
    const uint64_t upto = (2ull << lane) - 1ull;                          // lanes 0 ... lane
    const int r1 = min((band + 1) * EFSS_PREFIX_ROWS, H);
    unsigned long long nobs[EFSS_TG] = {}, nfc[EFSS_TG] = {}, nvalid = 0;
    for (int r = band * EFSS_PREFIX_ROWS + wave; r < r1; r += EFSS_WAVES) {
        uint32_t co[EFSS_TG] = {}, cf[EFSS_TG] = {};                      // carries of the earlier segments (wave-uniform)
        const size_t rowbase = base + (size_t)r * W * C;
        for (int j0 = 0; j0 < W; j0 += 64) {
            const int j = j0 + lane;
            const bool in = j < W;
            const size_t o = rowbase + (size_t)(in ? j : 0) * C;          // an idle lane reads the row's first cell and counts nothing
            const float yv = obs[o];
            bool fin = efss_finite(yv);
            uint32_t c[EFSS_TG] = {};
            const float* x = members + o;
#pragma unroll 4
            for (int m = 0; m < K; ++m) {
                const float xv = *x;
                x += stride;
                fin = fin && efss_finite(xv);
#pragma unroll
                for (int k = 0; k < EFSS_TG; ++k) c[k] += xv >= thr.t[k] ? 1u : 0u;
            }
            const bool ok = in && fin;
            const uint64_t mv = __ballot(ok);
            nvalid += (unsigned)__popcll(mv);
            if (lane == 0) vbits[(fl * (size_t)H + r) * words + (size_t)(j0 >> 6)] = mv;
#pragma unroll
            for (int k = 0; k < EFSS_TG; ++k) {
                if (k < thr.count) {                                      // uniform
                    const uint64_t mo = __ballot(ok && yv >= thr.t[k]);
                    uint32_t s = ok ? c[k] : 0u;                          // -> the inclusive scan of the wave
#pragma unroll
                    for (int d = 1; d < 64; d <<= 1) {
                        const uint32_t u = __shfl_up(s, d, 64);
                        if (lane >= d) s += u;
                    }
                    const uint32_t nf = (uint32_t)__builtin_amdgcn_readlane((int)s, 63);
                    if (in) {
                        PT* po = prefix + (((fl * thr.count + k) * 2) * (size_t)H + r) * rs;
                        PT* pf = po + (size_t)H * rs;
                        if (j == 0) { po[0] = (PT)0; pf[0] = (PT)0; }
                        po[j + 1] = (PT)(co[k] + (uint32_t)__popcll(mo & upto));
                        pf[j + 1] = (PT)(cf[k] + s);
                    }
                    const uint32_t no = (uint32_t)__popcll(mo);
                    co[k] += no; cf[k] += nf;
                    nobs[k] += no; nfc[k] += nf;
                }
            }
        }
    }
    if (lane == 0) {
#pragma unroll
        for (int k = 0; k < EFSS_TG; ++k) { cnt[wave][2 * k] = nobs[k]; cnt[wave][2 * k + 1] = nfc[k]; }
        cnt[wave][2 * EFSS_TG] = nvalid;
    }
    __syncthreads();
    const int k = threadIdx.x;
    if (k <= thr.count) {
        if (k == thr.count) {
            unsigned long long v = 0;
            for (int w = 0; w < EFSS_WAVES; ++w) v += cnt[w][2 * EFSS_TG];
            if (valid_out && v) atomicAdd(valid_out + g, v);
        } else {
            unsigned long long ob = 0, fc = 0;
            for (int w = 0; w < EFSS_WAVES; ++w) { ob += cnt[w][2 * k]; fc += cnt[w][2 * k + 1]; }
            unsigned long long* c = cont + (g * (size_t)T + (size_t)(t0 + k)) * 2;
            if (ob) atomicAdd(c + 0, ob);                                 // E
            if (fc) atomicAdd(c + 1, fc);                                 // Cs
        }
    }
}

__device__ __forceinline__ unsigned long long efss_wave_sum(unsigned long long v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
    return v;
}

// blockIdx.x = ((f * tcount + k) * nbands + band) * colblocks + column block.  half = n / 2 of the (clamped) window size n.
// WIDE: K * m > 65535, the squares need 64-bit multiplies.
template <typename PT, bool WIDE>
__global__ void __launch_bounds__(EFSS_THREADS) efss_window_kernel(const PT* __restrict__ prefix,
                                                                   const unsigned long long* __restrict__ vbits, uint32_t K, int H,
                                                                   int W, int tcount, long long n, long long half, int band_rows,
                                                                   int nbands, size_t field0, int T, int t0, int S, int s,
                                                                   unsigned long long* __restrict__ sums) {
    __shared__ unsigned long long red[EFSS_WAVES][5];
    const unsigned colblocks = (unsigned)((W + EFSS_THREADS - 1) / EFSS_THREADS);
    unsigned b = blockIdx.x;
    const int j = (int)(b % colblocks) * EFSS_THREADS + (int)threadIdx.x;
    b /= colblocks;
    const int band = (int)(b % (unsigned)nbands);
    b /= (unsigned)nbands;
    const int k = (int)(b % (unsigned)tcount);
    const size_t fl = b / (unsigned)tcount;
    const size_t rs = (size_t)W + 1;
    const size_t words = ((size_t)W + 63) / 64;
    const PT* po = prefix + ((fl * tcount + k) * 2) * (size_t)H * rs;
    const PT* pf = po + (size_t)H * rs;
    const unsigned long long* vb = vbits + fl * (size_t)H * words + (size_t)(j >> 6);
    unsigned long long d2 = 0, f2 = 0, o2 = 0, fv = 0, xs = 0;
    if (j < W) {
        const int c0 = (int)max((long long)j - half, 0ll), c1 = (int)min((long long)j - half + n, (long long)W);
        const int r0 = band * band_rows, r1 = min(r0 + band_rows, H);
        const int lo = (int)max((long long)r0 - half, 0ll), hi = (int)min((long long)r0 - half + n, (long long)H);
        uint32_t so = 0, sf = 0;                                          // window sums of the current row (modulo 2^32: exact, < 2^31)
        for (int r = lo; r < hi; ++r) {
            so += (uint32_t)po[r * rs + c1] - (uint32_t)po[r * rs + c0];
            sf += (uint32_t)pf[r * rs + c1] - (uint32_t)pf[r * rs + c0];
        }
        for (int i = r0; i < r1; ++i) {
            const uint32_t ko = K * so;                                   // <= K m < 2^31
            const uint32_t ad = sf > ko ? sf - ko : ko - sf;
            const bool ov = (uint32_t)po[(size_t)i * rs + j + 1] != (uint32_t)po[(size_t)i * rs + j];      // the centre cell's o
            const bool vc = (vb[(size_t)i * words] >> (j & 63)) & 1ull;                                    // and its validity
            if (WIDE) {
                const unsigned long long q = (unsigned long long)sf * sf;
                d2 += (unsigned long long)ad * ad; f2 += q; o2 += (unsigned long long)so * so;
                fv += vc ? q : 0ull;
            } else {
                const uint32_t q = sf * sf;                               // counts <= 65535: the squares fit 32 bits
                d2 += ad * ad; f2 += q; o2 += so * so;
                fv += vc ? q : 0u;
            }
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
    d2 = efss_wave_sum(d2); f2 = efss_wave_sum(f2); o2 = efss_wave_sum(o2); fv = efss_wave_sum(fv); xs = efss_wave_sum(xs);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) { red[wave][0] = d2; red[wave][1] = f2; red[wave][2] = o2; red[wave][3] = fv; red[wave][4] = xs; }
    __syncthreads();
    if (threadIdx.x < 5) {
        unsigned long long v = 0;
        for (int w = 0; w < EFSS_WAVES; ++w) v += red[w][threadIdx.x];
        if (v) atomicAdd(sums + (((field0 + fl) * (size_t)T + (size_t)(t0 + k)) * S + s) * 5 + threadIdx.x, v);
    }
}

struct Plan {
    size_t esize;                                      // bytes of a prefix entry
    size_t bits_per_field;                             // bytes of one field's validity bit-plane
    size_t bytes_per_field;                            // one threshold group of one field: prefixes and bit-plane
    size_t fields;                                     // fields per chunk
};

Plan plan(size_t K, size_t fields, int H, int W, int T) {
    Plan pl;
    pl.esize = K * (size_t)W <= 65535 ? 2 : 4;
    pl.bits_per_field = (size_t)H * (((size_t)W + 63) / 64) * sizeof(unsigned long long);
    pl.bytes_per_field = (size_t)std::min(T, EFSS_TG) * 2 * (size_t)H * ((size_t)W + 1) * pl.esize + pl.bits_per_field;
    pl.fields = std::max<size_t>(1, std::min({fields, EFSS_WS_BUDGET / pl.bytes_per_field, EFSS_MAX_CHUNK_FIELDS}));
    return pl;
}

template <typename PT>
void run(hipStream_t st, const float* members, size_t K, size_t stride, const float* obs, size_t B, int H, int W, int C,
         const float* thresholds, int T, const int* windows, int S, unsigned long long* sums, unsigned long long* cont,
         unsigned long long* valid, void* workspace) {
    const size_t fields = B * (size_t)C;
    const Plan pl = plan(K, fields, H, W, T);
    auto* vbits = static_cast<unsigned long long*>(workspace);            // the chunk's bit-planes first (8-byte aligned), then the prefixes
    PT* prefix = reinterpret_cast<PT*>(static_cast<char*>(workspace) + pl.fields * pl.bits_per_field);
    const size_t pbands = cdivz(H, EFSS_PREFIX_ROWS), colblocks = cdivz(W, EFSS_THREADS);
    const long long cover = 2ll * std::max(H, W);      // a window this large holds the whole field from every cell
    const double cells = (double)H * W;
    for (size_t f0 = 0; f0 < fields; f0 += pl.fields) {
        const size_t nf = std::min(pl.fields, fields - f0);
        for (int t0 = 0; t0 < T; t0 += EFSS_TG) {
            EfssThresholds thr;
            thr.count = std::min(EFSS_TG, T - t0);
            // an unused slot holds +inf: no finite member reaches it, and its counter is never read
            for (int k = 0; k < EFSS_TG; ++k) thr.t[k] = k < thr.count ? thresholds[t0 + k] : INFINITY;
            {
                DL4DS_REQUIRE(nf * pbands < (size_t(1) << 31), "ensemble_fss: grid too large");
                ProfScope ps(st, "ensemble_fss_prefix", 0.0, cells * nf * (4.0 * (double)(K + 1) + 2.0 * thr.count * sizeof(PT)));
                DL4DS_LAUNCH(efss_prefix_kernel<PT>, dim3((unsigned)(nf * pbands)), dim3(EFSS_THREADS), 0, st, members, stride, (int)K,
                             obs, H, W, C, f0, thr, T, t0, prefix, vbits, cont, t0 == 0 ? valid : nullptr);
            }
            for (int s = 0; s < S; ++s) {
                const long long n = std::min<long long>(windows[s], cover), half = n / 2;
                const unsigned long long m = (unsigned long long)std::min<long long>(n, H) * std::min<long long>(n, W);
                // bands of rows when the grid would be small; at least n rows each, so a band's start-up reads stay below its own
                const size_t base_blocks = nf * thr.count * colblocks;
                const size_t want = std::max<size_t>(1, EFSS_TARGET_BLOCKS / base_blocks);
                const long long rows = std::min<long long>(H, std::max<long long>({(long long)cdivz(H, want), n, EFSS_BAND_MIN}));
                const int band_rows = (int)rows, nbands = (int)cdivz(H, band_rows);
                const size_t grid = base_blocks * nbands;
                DL4DS_REQUIRE(grid < (size_t(1) << 31), "ensemble_fss: grid too large");
                ProfScope ps(st, "ensemble_fss_window", 0.0, cells * nf * thr.count * 10.0 * sizeof(PT));
                const auto kern = K * m <= 65535ull ? efss_window_kernel<PT, false> : efss_window_kernel<PT, true>;
                DL4DS_LAUNCH(kern, dim3((unsigned)grid), dim3(EFSS_THREADS), 0, st, (const PT*)prefix,
                             (const unsigned long long*)vbits, (uint32_t)K, H, W, thr.count, n, half, band_rows, nbands, f0, T, t0, S,
                             s, sums);
            }
        }
    }
}

}  // namespace

size_t ensemble_fss_workspace_bytes(size_t K, size_t B, int H, int W, int C, int T) {
    if (K == 0 || B == 0 || H <= 0 || W <= 0 || C <= 0 || T <= 0) return 0;
    const Plan pl = plan(K, B * (size_t)C, H, W, T);
    return pl.fields * pl.bytes_per_field;
}

void ensemble_fss_check_args(const float* members, size_t K, size_t n, size_t member_stride, const float* obs, size_t B, int H,
                             int W, int C, const float* thresholds, int T, const int* windows, int S, const long long* sums,
                             const long long* cont, const long long* valid) {
    DL4DS_REQUIRE(K >= 1 && K <= ENS_MAX_MEMBERS, "ensemble_fss: 1 <= K <= 256 members");
    DL4DS_REQUIRE(T >= 1 && T <= EXC_MAX_THRESHOLDS, "ensemble_fss: 1 <= T <= 16 thresholds");
    DL4DS_REQUIRE(S >= 1, "ensemble_fss: at least one window is needed");
    DL4DS_REQUIRE(H >= 1 && W >= 1 && C >= 1, "ensemble_fss: expected H, W, C >= 1");
    DL4DS_REQUIRE(members && obs && thresholds && windows && sums && cont && valid,
                  "ensemble_fss: null member stack, observation, thresholds, windows or output");
    DL4DS_REQUIRE((long long)H * W < (1ll << 31), "ensemble_fss: fields of 2^31 or more cells are not supported");
    DL4DS_REQUIRE((unsigned __int128)B * (unsigned)C < ((unsigned __int128)1 << 31), "ensemble_fss: too many fields");
    DL4DS_REQUIRE((unsigned __int128)B * (unsigned)H * (unsigned)W * (unsigned)C == (unsigned __int128)n,
                  "ensemble_fss: n must be B whole samples of H * W * C cells");
    DL4DS_REQUIRE(member_stride >= n, "ensemble_fss: member stride smaller than the member");
    for (int k = 0; k < T; ++k) DL4DS_REQUIRE(std::isfinite(thresholds[k]), "ensemble_fss: thresholds must be finite");
    for (int s = 0; s < S; ++s) {
        DL4DS_REQUIRE(windows[s] >= 1, "ensemble_fss: window sizes must be positive");
        const unsigned __int128 km = (unsigned __int128)K * (unsigned)std::min(windows[s], H) * (unsigned)std::min(windows[s], W);
        DL4DS_REQUIRE((unsigned __int128)H * (unsigned)W * km * km < ((unsigned __int128)1 << 62),
                      "ensemble_fss: H*W*(K*m)^2 with m = min(n, H)*min(n, W) must stay below 2^62 for the exact 64-bit sums");
    }
}

void ensemble_fss(hipStream_t st, const float* members, size_t K, size_t n, size_t member_stride, const float* obs, size_t B, int H,
                  int W, int C, const float* thresholds, int T, const int* windows, int S, long long* sums, long long* cont,
                  long long* valid, void* workspace, size_t workspace_bytes) {
    ensemble_fss_check_args(members, K, n, member_stride, obs, B, H, W, C, thresholds, T, windows, S, sums, cont, valid);
    if (B == 0) return;
    DL4DS_REQUIRE(workspace && workspace_bytes >= ensemble_fss_workspace_bytes(K, B, H, W, C, T), "ensemble_fss workspace too small");
    const size_t fields = B * (size_t)C;
    HIP_CHECK(hipMemsetAsync(sums, 0, fields * T * S * 5 * sizeof(long long), st));
    HIP_CHECK(hipMemsetAsync(cont, 0, fields * T * 2 * sizeof(long long), st));
    HIP_CHECK(hipMemsetAsync(valid, 0, fields * sizeof(long long), st));
    auto* us = reinterpret_cast<unsigned long long*>(sums);
    auto* uc = reinterpret_cast<unsigned long long*>(cont);
    auto* uv = reinterpret_cast<unsigned long long*>(valid);
    if (K * (size_t)W <= 65535)
        run<uint16_t>(st, members, K, member_stride, obs, B, H, W, C, thresholds, T, windows, S, us, uc, uv, workspace);
    else
        run<uint32_t>(st, members, K, member_stride, obs, B, H, W, C, thresholds, T, windows, S, us, uc, uv, workspace);
}
