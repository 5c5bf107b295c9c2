// Temporal verification along the time axis: the raw sums of the lag-k autocorrelation, the event
// transition counts and the histogram of spell lengths per grid cell and period, of one series or of two on common validity.
// The reference has no counterpart.
//
// y, p are fp32 (N, H, W, C) in time order; a cell is one (h, w, c), per = H*W*C, cell c of sample n lives at x[n*per + c].  p may
// be null: S = 1 with y alone, S = 2 with both; series 0 is y, series 1 is p.  The P periods are given by period_starts with P + 1
// entries (int64, strictly increasing, first 0, last N), as in indices.hip; nothing carries across a boundary.  A sample is VALID
// in a cell iff it is finite in every series supplied (common validity, as in distribution.hip); -0.0 counts as +0.0.
// 0 <= L <= 4 lags, strictly increasing, each in 1..32.  0 <= T <= 4 thresholds in a DEVICE array, thr [T] or with thr_per_cell
// [T][per]; one comparison op for all of them (0 >=, 1 >, 2 <, 3 <=), made on fp32.  A valid sample of a series is an EVENT for
// threshold t iff x op thr(t, c), a non-event otherwise; an event run is a maximal stretch of consecutive samples of the period
// that are all events, a non-event run the same over valid non-events; an invalid sample ends both kinds of run.  1 <= B <= 32
// spell bins.  Where thr(t, c) is not finite every integer output of (t, c) is -1 in every period.  Per period p and cell c (each
// output may be null; all are overwritten):
//   valid  [P][per]              int32: the number of valid samples
//   moment [P][S][2][per]        fp64: sum x and sum x^2 over the valid samples, each added one term at a time in ascending sample
//                                order from 0.0; x^2 is formed in fp64 from the fp32 value (exact)
//   pair   [P][L][per]           int32: the number of pairs (n, n + lag) with both samples inside the period and both valid
//   lag    [P][S][L][3][per]     fp64: over exactly those pairs in ascending n, a = x_n, b = x_{n+lag}: sum a, sum b, sum a*b; the
//                                product is formed in fp64 from two fp32 values and is exact, so a fused multiply-add gives the
//                                same bits as a product and an addition
//   trans  [P][S][T][4][per]     int32: over consecutive samples (n, n + 1) both inside the period and both valid: n00, n01, n10,
//                                n11 (first digit the state at n, second at n + 1; 1 is an event)
//   spell  [P][S][T][2][B][per]  int32: kind 0 event runs, kind 1 non-event runs; bin k - 1 the number of runs of length k for
//                                k < B, the last bin the runs of length >= B.  Every maximal run counts, also one cut by a period
//                                boundary or ended by an invalid sample
// No floating-point atomics, no sum whose order could vary: a repeated call gives the same bits.
//
// Kernel: as in indices.hip a lane owns one cell and walks one period's samples in order; a workgroup is TMP_CELLS consecutive
// cells of one period (blockIdx.x = cell group * P + period).  TMP_DEPTH samples of every series are loaded at once and consumed
// in order.  The last 32 values of a lane and series live in an LDS ring at word k*TMP_CELLS + thread; the pair (n - lag, n) is
// formed when n arrives, from the ring (read before n is written: lag 32 reads the slot n takes).  Whether n - lag was valid, and
// inside the period, is one bit of a 32-bit history of the lane's validity that starts empty with the period.  The current run of
// a (series, threshold) is one signed counter (> 0 an event run, < 0 a non-event run), which is also the state at n - 1 for the
// transition counts.  One kernel per (S, T, L): nothing is indexed at run time.  The histogram is the lane's own column of the
// output: the lane zeroes bins 1.. before the walk, counts the runs of length 1 (bin 0) in registers and adds one to a longer
// run's bin with a plain load and store of its own word; no atomics.  A period is not split over time, which would change the
// order of the fp64 sums: parallelism is cells x periods.
#include "common.h"
#include "ops.h"
#include "periods.h"
#include "prof.h"

namespace {

constexpr int TMP_CELLS = 256;                         // cells (threads) per workgroup
constexpr int TMP_DEPTH = 8;                           // samples of each series a lane has in flight
constexpr int TMP_RING = 32;                           // ring slots per lane and series = the largest lag
struct TmpArgs {
    const float* x[2];                                 // y, p (null with S = 1)
    size_t per;
    const long long* starts;                           // [P + 1], device
    const int* lags;                                   // [TMP_MAX_LAGS], device
    unsigned P;
    const float* thr;
    int thr_per_cell, op, bins;
    int* valid;
    double* moment;
    int* pair;
    double* lag;
    int* trans;
    int* spell;
};

template <int S, int T, int L>
__global__ void __launch_bounds__(TMP_CELLS) temporal_kernel(const TmpArgs a) {
    constexpr int T1 = T ? T : 1, L1 = L ? L : 1;
    __shared__ float ring[L ? S * TMP_RING * TMP_CELLS : 1];
    const int tid = threadIdx.x;
    const unsigned p = blockIdx.x % a.P;
    const size_t per = a.per, c = (size_t)(blockIdx.x / a.P) * TMP_CELLS + tid;
    const bool live = c < per;
    const size_t cc = live ? c : per - 1;                                 // an idle lane walks the last cell and stores nothing
    const size_t s0 = (size_t)a.starts[p], s1 = (size_t)a.starts[p + 1];
    const int len = (int)(s1 - s0), B = a.bins;
    const auto [neg, strict] = decode_op(a.op);

    int lags[L1];
#pragma unroll
    for (int l = 0; l < L; ++l) lags[l] = a.lags[l];
    float thr[T1];
    bool thr_ok[T1];
#pragma unroll
    for (int t = 0; t < T; ++t) {
        const float v = a.thr_per_cell ? a.thr[(size_t)t * per + cc] : a.thr[t];
        thr_ok[t] = finite_f32(v);
        thr[t] = neg ? -v : v;
    }
    int n_valid = 0, n_pair[L1];
    unsigned hist = 0;                                                    // bit k: the sample k + 1 before this one was valid
    double sum[S], sq[S], la[S][L1], lb[S][L1], lab[S][L1];
    int run[S][T1], tr[S][T1][4], one_e[S][T1], one_n[S][T1];             // current run (signed), transitions, runs of length 1
#pragma unroll
    for (int l = 0; l < L1; ++l) n_pair[l] = 0;
#pragma unroll
    for (int s = 0; s < S; ++s) {
        sum[s] = sq[s] = 0.0;
#pragma unroll
        for (int l = 0; l < L1; ++l) la[s][l] = lb[s][l] = lab[s][l] = 0.0;
#pragma unroll
        for (int t = 0; t < T1; ++t) run[s][t] = tr[s][t][0] = tr[s][t][1] = tr[s][t][2] = tr[s][t][3] = one_e[s][t] = one_n[s][t] = 0;
    }
    // the lane's histogram column: spell[((((p*S + s)*T + t)*2 + kind)*B + k)*per + c]
    const bool do_spell = T > 0 && a.spell != nullptr && live;
    int* const hcol = do_spell ? a.spell + (size_t)p * S * T * 2 * B * per + c : nullptr;
    if (do_spell) {
#pragma unroll
        for (int s = 0; s < S; ++s)
#pragma unroll
            for (int t = 0; t < T; ++t)
                for (int k = 0; k < 2 * B; ++k)                           // (bin 0 of either kind is stored again after the walk)
                    hcol[((size_t)(s * T + t) * 2 * B + k) * per] = thr_ok[t] ? 0 : -1;
    }
    // a run of `r` samples (r > 0 events, r < 0 non-events) of (s, t) has ended
    auto ended = [&](int s, int t, int r) {
        const int n = r > 0 ? r : -r, k = (n < B ? n : B) - 1;
        one_e[s][t] += (k == 0 && r > 0) ? 1 : 0;
        one_n[s][t] += (k == 0 && r < 0) ? 1 : 0;
        if (k > 0 && do_spell && thr_ok[t]) {
            int* w = hcol + ((size_t)((s * T + t) * 2 + (r > 0 ? 0 : 1)) * B + k) * per;
            *w = *w + 1;
        }
    };

    const float* col[S];
#pragma unroll
    for (int s = 0; s < S; ++s) col[s] = a.x[s] + s0 * per + cc;          // sample i of the period at col[s][i*per]
    for (int i0 = 0; i0 < len; i0 += TMP_DEPTH) {
        float blk[S][TMP_DEPTH];
#pragma unroll
        for (int u = 0; u < TMP_DEPTH; ++u) {
            const int i = i0 + u < len ? i0 + u : len - 1;
#pragma unroll
            for (int s = 0; s < S; ++s) blk[s][u] = col[s][(size_t)i * per];
        }
#pragma unroll
        for (int u = 0; u < TMP_DEPTH; ++u) {
            const int i = i0 + u;
            if (i >= len) break;                                          // (uniform)
            bool ok = true;
            float v[S];
#pragma unroll
            for (int s = 0; s < S; ++s) {
                ok = ok && finite_f32(blk[s][u]);
                v[s] = blk[s][u] == 0.f ? 0.f : blk[s][u];                // -0.0 counts as +0.0
            }
            n_valid += ok ? 1 : 0;
            if constexpr (L > 0) {
                bool both[L];
#pragma unroll
                for (int l = 0; l < L; ++l) {
                    both[l] = ok && ((hist >> (lags[l] - 1)) & 1u);
                    n_pair[l] += both[l] ? 1 : 0;
                }
#pragma unroll
                for (int s = 0; s < S; ++s) {
                    float* r = ring + s * TMP_RING * TMP_CELLS + tid;
                    const double d = (double)v[s];
#pragma unroll
                    for (int l = 0; l < L; ++l) {                         // (a slot no sample has written yet is read and dropped)
                        const double e = (double)r[((i - lags[l]) & (TMP_RING - 1)) * TMP_CELLS];
                        if (both[l]) {
                            la[s][l] += e;
                            lb[s][l] += d;
                            lab[s][l] += e * d;
                        }
                    }
                    r[(i & (TMP_RING - 1)) * TMP_CELLS] = v[s];
                }
            }
            hist = (hist << 1) | (ok ? 1u : 0u);
#pragma unroll
            for (int s = 0; s < S; ++s) {
                const double d = (double)v[s];
                if (ok) {
                    sum[s] += d;
                    sq[s] += d * d;
                }
                const float cv = neg ? -v[s] : v[s];
#pragma unroll
                for (int t = 0; t < T; ++t) {
                    const bool ev = ok && (strict ? cv > thr[t] : cv >= thr[t]);
                    const int cur = ev ? 1 : (ok ? -1 : 0), r = run[s][t];
                    tr[s][t][0] += (r < 0 && cur < 0) ? 1 : 0;
                    tr[s][t][1] += (r < 0 && cur > 0) ? 1 : 0;
                    tr[s][t][2] += (r > 0 && cur < 0) ? 1 : 0;
                    tr[s][t][3] += (r > 0 && cur > 0) ? 1 : 0;
                    const bool same = (r > 0 && cur > 0) || (r < 0 && cur < 0);
                    if (r != 0 && !same) ended(s, t, r);
                    run[s][t] = same ? r + cur : cur;
                }
            }
        }
    }
#pragma unroll
    for (int s = 0; s < S; ++s)
#pragma unroll
        for (int t = 0; t < T; ++t)
            if (run[s][t] != 0) ended(s, t, run[s][t]);                   // the period's end cuts the run
    if (!live) return;
    if (a.valid) a.valid[(size_t)p * per + c] = n_valid;
    if (a.moment) {
#pragma unroll
        for (int s = 0; s < S; ++s) {
            double* o = a.moment + ((size_t)p * S + s) * 2 * per + c;
            o[0] = sum[s];
            o[per] = sq[s];
        }
    }
    if constexpr (L > 0) {
        if (a.pair) {
#pragma unroll
            for (int l = 0; l < L; ++l) a.pair[((size_t)p * L + l) * per + c] = n_pair[l];
        }
        if (a.lag) {
#pragma unroll
            for (int s = 0; s < S; ++s)
#pragma unroll
                for (int l = 0; l < L; ++l) {
                    double* o = a.lag + (((size_t)p * S + s) * L + l) * 3 * per + c;
                    o[0] = la[s][l];
                    o[per] = lb[s][l];
                    o[2 * per] = lab[s][l];
                }
        }
    }
    if constexpr (T > 0) {
        if (a.trans) {
#pragma unroll
            for (int s = 0; s < S; ++s)
#pragma unroll
                for (int t = 0; t < T; ++t) {
                    int* o = a.trans + (((size_t)p * S + s) * T + t) * 4 * per + c;
#pragma unroll
                    for (int j = 0; j < 4; ++j) o[(size_t)j * per] = thr_ok[t] ? tr[s][t][j] : -1;
                }
        }
        if (do_spell) {
#pragma unroll
            for (int s = 0; s < S; ++s)
#pragma unroll
                for (int t = 0; t < T; ++t) {
                    int* o = hcol + (size_t)(s * T + t) * 2 * B * per;
                    o[0] = thr_ok[t] ? one_e[s][t] : -1;
                    o[(size_t)B * per] = thr_ok[t] ? one_n[s][t] : -1;
                }
        }
    }
}

template <int S, int T>
void tmp_launch(hipStream_t s, const TmpArgs& a, unsigned blocks, int L) {
    const dim3 g(blocks), b(TMP_CELLS);
    switch (L) {
        case 0: DL4DS_LAUNCH((temporal_kernel<S, T, 0>), g, b, 0, s, a); break;
        case 1: DL4DS_LAUNCH((temporal_kernel<S, T, 1>), g, b, 0, s, a); break;
        case 2: DL4DS_LAUNCH((temporal_kernel<S, T, 2>), g, b, 0, s, a); break;
        case 3: DL4DS_LAUNCH((temporal_kernel<S, T, 3>), g, b, 0, s, a); break;
        default: DL4DS_LAUNCH((temporal_kernel<S, T, 4>), g, b, 0, s, a); break;
    }
}

template <int S>
void tmp_launch_s(hipStream_t s, const TmpArgs& a, unsigned blocks, int T, int L) {
    switch (T) {
        case 0: tmp_launch<S, 0>(s, a, blocks, L); break;
        case 1: tmp_launch<S, 1>(s, a, blocks, L); break;
        case 2: tmp_launch<S, 2>(s, a, blocks, L); break;
        case 3: tmp_launch<S, 3>(s, a, blocks, L); break;
        default: tmp_launch<S, 4>(s, a, blocks, L); break;
    }
}

size_t tmp_lags_offset(int P) { return (period_starts_bytes(P) + 15) & ~size_t(15); }

}  // namespace

size_t temporal_workspace_bytes(size_t N, size_t per, const long long* period_starts, int P, const int* lags, int L, int T, int op,
                                int spell_bins) {
    DL4DS_REQUIRE(N > 0 && per > 0, "temporal: empty array");
    DL4DS_REQUIRE(N < (size_t(1) << 31), "temporal: 2^31 or more samples are not supported");
    DL4DS_REQUIRE(P >= 1, "temporal: at least one period is needed");
    DL4DS_REQUIRE(L >= 0 && L <= TMP_MAX_LAGS, "temporal: 0 <= L <= 4 lags");
    DL4DS_REQUIRE(T >= 0 && T <= TMP_MAX_THRESHOLDS, "temporal: 0 <= T <= 4 thresholds");
    DL4DS_REQUIRE(spell_bins >= 1 && spell_bins <= TMP_MAX_BINS, "temporal: 1 <= spell_bins <= 32");
    DL4DS_REQUIRE(op >= 0 && op <= 3, "temporal: op must be 0 (>=), 1 (>), 2 (<) or 3 (<=)");
    DL4DS_REQUIRE(period_starts, "temporal: null period starts");       // (before the lags, as it has always been)
    DL4DS_REQUIRE(L == 0 || lags, "temporal: null lags");
    for (int l = 0; l < L; ++l)
        DL4DS_REQUIRE(lags[l] >= 1 && lags[l] <= TMP_RING && (l == 0 || lags[l] > lags[l - 1]),
                      "temporal: lags must be strictly increasing, each in 1..32");
    check_period_starts("temporal", period_starts, P, N);
    DL4DS_REQUIRE(cdivz(per, TMP_CELLS) * (size_t)P < (size_t(1) << 31), "temporal: too many cells x periods for one launch");
    return tmp_lags_offset(P) + TMP_MAX_LAGS * sizeof(int);
}

void temporal(hipStream_t s, const float* y, const float* p, size_t N, size_t per, const long long* period_starts, int P,
              const int* lags, int L, const float* thr, int T, int thr_per_cell, int op, int spell_bins, int* valid, double* moment,
              int* pair, double* lag, int* trans, int* spell, void* workspace, size_t workspace_bytes) {
    const size_t need = temporal_workspace_bytes(N, per, period_starts, P, lags, L, T, op, spell_bins);      // (refuses a bad request)
    DL4DS_REQUIRE(y, "temporal: null array");
    DL4DS_REQUIRE(T == 0 || thr, "temporal: null thresholds");
    DL4DS_REQUIRE(L > 0 || (!pair && !lag), "temporal: pair and lag outputs need at least one lag");
    DL4DS_REQUIRE(T > 0 || (!trans && !spell), "temporal: transition and spell outputs need at least one threshold");
    DL4DS_REQUIRE(valid || moment || pair || lag || trans || spell, "temporal: all six outputs are null");
    DL4DS_REQUIRE(workspace && workspace_bytes >= need, "temporal workspace too small");
    int* dlags = reinterpret_cast<int*>(static_cast<char*>(workspace) + tmp_lags_offset(P));
    int hl[TMP_MAX_LAGS] = {1, 1, 1, 1};
    for (int l = 0; l < L; ++l) hl[l] = lags[l];
    HIP_CHECK(hipMemcpyAsync(dlags, hl, sizeof(hl), hipMemcpyHostToDevice, s));
    const long long* starts = upload_period_starts(s, period_starts, P, workspace);      // (waits for the lags too: hl may go away)
    const int S = p ? 2 : 1;
    const TmpArgs a{{y, p}, per, starts, dlags, (unsigned)P, thr, thr_per_cell, op, spell_bins, valid, moment, pair, lag, trans, spell};
    const unsigned blocks = (unsigned)(cdivz(per, TMP_CELLS) * (size_t)P);
    const double cells = (double)per * P;
    ProfScope ps(s, "temporal", 0.0,
                 4.0 * S * (double)N * (double)per +
                     cells * ((valid ? 4.0 : 0.0) + (moment ? 16.0 * S : 0.0) + (pair ? 4.0 * L : 0.0) + (lag ? 24.0 * S * L : 0.0) +
                              (trans ? 16.0 * S * T : 0.0) + (spell ? 8.0 * S * T * spell_bins : 0.0)));
    if (S == 1) tmp_launch_s<1>(s, a, blocks, T, L);
    else tmp_launch_s<2>(s, a, blocks, T, L);
    HIP_CHECK(hipGetLastError());
}
