// Neighbourhood verification of N*C fields (planes of two (N, H, W, C) arrays): per field, exceedance threshold and window size the
// three integer sums of the Fractions Skill Score (Roberts & Lean 2008), per field and threshold the 2 x 2 contingency table.
//
// A cell is VALID iff y and p are both finite there (NaN in y is the masking mechanism).  Indicators bo = valid & (y >= t),
// bf = valid & (p >= t).  The window of size n at cell (i, j) is rows [i - n/2, i - n/2 + n), columns likewise, clipped to the
// field; co / cf are the counts of bo / bf in it.  D = sum (cf - co)^2, F = sum cf^2, O = sum co^2 over ALL H*W cells, the
// contingency counts over the valid cells.  FSS = 1 - D / (F + O) follows on the host.  Everything here is integer arithmetic:
// integer sums are associative, so the 64-bit atomics below give the same bits in any order and the result EQUALS a reference.
//
// Two kernels per chunk of fields and group of at most NB_TG thresholds.  This file owns the first and the
// contingency table; the window walk, the chunk planner, the driver and the argument rules are neighbourhood.h's, shared with
// ensemble_fss.hip (section 14a), of which this entry is the K = 1 case:
//  * fss_prefix_kernel: a wave per row reads y and p once, 64 cells at a time.  For every threshold of the group the two
//    indicators are one __ballot each; the exclusive row prefix of lane l is popcount(mask below l) + the carry of the earlier
//    segments (a wave-uniform count), stored as uint16 (W <= 65535) or uint32 in rows of W + 1 entries.  The contingency
//    counts are popcounts of the same masks: wave-uniform, summed over the block's rows, one atomic per block and count.
//  * fss_window_kernel, per window size: nb_window_walk without the ensemble's centre-cell sums.  Reads are coalesced along the
//    columns, the work per cell does not depend on n, no 2-D table exists.
// Fields go through in chunks sized by a fixed workspace budget; a threshold group of one field larger than it runs alone.
#include "neighbourhood.h"
#include "ops.h"

namespace {

constexpr int FSS_NCNT = 3 * NB_TG + 1;                // per threshold: hits, observed events, forecast events; + the valid count

template <typename PT>
__global__ void __launch_bounds__(NB_THREADS) fss_prefix_kernel(const float* __restrict__ y, const float* __restrict__ p, int H,
                                                                int W, int C, size_t field0, NbThresholds thr, int T, int t0,
                                                                PT* __restrict__ prefix, unsigned long long* __restrict__ cont,
                                                                unsigned long long* __restrict__ valid_out) {
    __shared__ unsigned long long cnt[NB_WAVES][FSS_NCNT];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int bands = (H + NB_PREFIX_ROWS - 1) / NB_PREFIX_ROWS;
    const size_t fl = blockIdx.x / (unsigned)bands;                        // field of the chunk
    const int band = (int)(blockIdx.x % (unsigned)bands);
    const size_t g = field0 + fl;                                         // field of the call
    const size_t base = nb_field_base(g, H, W, C);
    const uint64_t below = (1ull << lane) - 1ull;
    const int r1 = min((band + 1) * NB_PREFIX_ROWS, H);
    unsigned long long hits[NB_TG] = {}, nobs[NB_TG] = {}, nfc[NB_TG] = {}, nvalid = 0;
    for (int r = band * NB_PREFIX_ROWS + wave; r < r1; r += NB_WAVES) {
        uint32_t co[NB_TG] = {}, cf[NB_TG] = {};
        const size_t rowbase = base + (size_t)r * W * C;
        for (int j0 = 0; j0 < W; j0 += 64) {
            const int j = j0 + lane;
            const bool in = j < W;
            const size_t o = rowbase + (size_t)(in ? j : 0) * C;
            const float yv = y[o], pv = p[o];
            const bool ok = in && finite_bits(yv) && finite_bits(pv);
            nvalid += (unsigned)__popcll(__ballot(ok));
#pragma unroll
            for (int k = 0; k < NB_TG; ++k) {
                if (k < thr.count) {                                      // uniform
                    const uint64_t mo = __ballot(ok && yv >= thr.t[k]), mf = __ballot(ok && pv >= thr.t[k]);
                    if (in) {
                        const NbRows<PT> row = nb_prefix_rows(prefix, fl, thr.count, k, H, W, r);
                        if (j == 0) { row.o[0] = (PT)0; row.f[0] = (PT)0; }
                        const uint64_t upto = below | (1ull << lane);
                        row.o[j + 1] = (PT)(co[k] + (uint32_t)__popcll(mo & upto));
                        row.f[j + 1] = (PT)(cf[k] + (uint32_t)__popcll(mf & upto));
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
        for (int k = 0; k < NB_TG; ++k) {
            cnt[wave][3 * k] = hits[k]; cnt[wave][3 * k + 1] = nobs[k]; cnt[wave][3 * k + 2] = nfc[k];
        }
        cnt[wave][3 * NB_TG] = nvalid;
    }
    __syncthreads();
    const int k = threadIdx.x;
    if (k <= thr.count) {
        unsigned long long v = 0;
        for (int w = 0; w < NB_WAVES; ++w) v += cnt[w][3 * NB_TG];
        if (k == thr.count) {
            if (valid_out) atomicAdd(valid_out + g, v);
        } else {
            unsigned long long h = 0, ob = 0, fc = 0;
            for (int w = 0; w < NB_WAVES; ++w) { h += cnt[w][3 * k]; ob += cnt[w][3 * k + 1]; fc += cnt[w][3 * k + 2]; }
            unsigned long long* c = cont + nb_cont_at(g, T, t0 + k, 4);
            atomicAdd(c + 0, h);                                          // hits
            atomicAdd(c + 1, ob - h);                                     // misses
            atomicAdd(c + 2, fc - h);                                     // false alarms
            atomicAdd(c + 3, v + h - ob - fc);                            // correct negatives (valid, neither)
        }
    }
}

template <typename PT, bool WIDE>
__global__ void __launch_bounds__(NB_THREADS) fss_window_kernel(const PT* __restrict__ prefix, int H, int W, int tcount, long long n,
                                                                long long half, int band_rows, int nbands, size_t field0, int T,
                                                                int t0, int S, int s, unsigned long long* __restrict__ sums) {
    nb_window_walk<PT, WIDE, false>(prefix, nullptr, 1u, H, W, tcount, n, half, band_rows, nbands, field0, T, t0, S, s, sums);
}

NbPlan plan(size_t fields, int H, int W, int T) { return nb_plan(fields, H, W, T, nb_esize(1, W), 0); }

}  // namespace

size_t fss_workspace_bytes(int N, int H, int W, int C, int T) {
    if (N <= 0 || H <= 0 || W <= 0 || C <= 0 || T <= 0) return 0;
    return plan((size_t)N * C, H, W, T).bytes();
}

void fss_check_args(int N, int H, int W, int C, const float* thresholds, int T, const int* windows, int S) {
    DL4DS_REQUIRE(N >= 0 && H >= 1 && W >= 1 && C >= 1, "fss: expected N >= 0 and H, W, C >= 1");
    DL4DS_REQUIRE(T >= 1 && S >= 1 && thresholds && windows, "fss: at least one threshold and one window are needed");
    nb_check_args("fss", "H*W*m^2", 1, (unsigned __int128)N * (unsigned)C, H, W, thresholds, T, windows, S);
}

void fss(hipStream_t st, const float* y, const float* p, int N, int H, int W, int C, const float* thresholds, int T,
         const int* windows, int S, long long* sums, long long* cont, long long* valid, void* workspace, size_t workspace_bytes) {
    fss_check_args(N, H, W, C, thresholds, T, windows, S);
    if (N == 0) return;
    DL4DS_REQUIRE(workspace_bytes >= fss_workspace_bytes(N, H, W, C, T), "fss workspace too small");
    const size_t fields = (size_t)N * C;
    nb_enter(st, 1, fields, W, T, S, 3, 4, sums, cont, valid, [&](auto pt, auto* us, auto* uc, auto* uv) {
        using PT = decltype(pt);
        PT* prefix = static_cast<PT*>(workspace);
        nb_run<PT>(
            st, "fss", 1, fields, H, W, thresholds, T, windows, S, plan(fields, H, W, T).fields, 8.0,
            [&](const NbGroup& g) {
                DL4DS_LAUNCH(fss_prefix_kernel<PT>, dim3(g.prefix_grid), dim3(NB_THREADS), 0, st, y, p, H, W, C, g.f0, g.thr, T, g.t0,
                             prefix, uc, g.t0 == 0 ? uv : nullptr);
            },
            [&](const NbGroup& g, const NbWindow& w) {
                const auto kern = w.wide ? fss_window_kernel<PT, true> : fss_window_kernel<PT, false>;
                DL4DS_LAUNCH(kern, dim3(w.grid), dim3(NB_THREADS), 0, st, (const PT*)prefix, H, W, g.thr.count, w.n, w.half,
                             w.band_rows, w.nbands, g.f0, T, g.t0, S, w.s, us);
            });
    });
}
