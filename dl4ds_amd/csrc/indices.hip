// Climate indices along the time axis: spells, extremes, threshold days and sums per grid cell and period,
// the raw material of the ETCCDI indices (CDD / CWD, Rx1day / Rx5day, R1mm / R10mm / R20mm, SDII, PRCPTOT, TXx / TNn, FD / SU,
// R95pTOT, start and end of a season).  The reference has no counterpart.
//
// x is fp32 (N, H, W, C); a cell is one (h, w, c), per = H*W*C, cell c of sample n lives at x[n*per + c].  The samples are in time
// order.  The P periods are given by period_starts with P + 1 entries (int64, strictly increasing, first 0, last N): period p is
// the samples start_p <= n < start_{p+1}.  Periods are independent, nothing carries across a boundary: a run is cut there and a
// window lies inside one period.  A sample is VALID in a cell iff its value is finite (NaN is the masking mechanism); -0.0 counts
// as +0.0.  1 <= T <= 4 thresholds in a DEVICE array, used as in ensemble_exceedance: thr [T], or with thr_per_cell [T][per]; one
// comparison op for all of them (0 >=, 1 >, 2 <, 3 <=), made on fp32.  A valid sample is an EVENT for threshold t iff
// x op thr(t, c), a non-event otherwise.  An event run is a maximal stretch of consecutive samples of the period that are all
// events, a non-event run the same over valid non-events; an invalid sample ends both kinds of run.  Where thr(t, c) is not finite
// the per-threshold outputs of (t, c) are -1 (integers) and NaN (sum) in every period.  Per period p and cell c (each output may be
// null; all are overwritten):
//   valid [P][per]        int32: the number of valid samples
//   event [P][T][6][per]  int32: number of events; longest event run; longest non-event run; number of event runs; offset from the
//                         period's first sample of the first event (-1: none); offset of the last event (-1: none)
//   ext   [P][2][per]     fp32: the largest and the smallest valid value, NaN without one; a zero is +0.0
//   sum   [P][2 + T][per] fp64: row 0 the sum of the valid values, added one by one in ascending sample order from the first
//                         valid value (NaN without one); row 1 the largest window sum over all windows of `window` (1..32)
//                         consecutive samples that lie wholly inside the period and are all valid, each window sum formed afresh
//                         from its values in ascending sample order (no sliding add and subtract; NaN without such a window);
//                         row 2 + t the sum of the event values of threshold t in the order of row 0 (0.0 without an event)
// No floating-point atomics, no sum whose order could vary: a repeated call gives the same bits.
//
// Kernel: a lane owns one cell and walks one period's samples in order; a workgroup is IDX_CELLS consecutive cells of one period
// (blockIdx.x = cell group * P + period), so every wave-instruction reads 256 contiguous bytes.  The walk is sequential, the
// loads are not: IDX_DEPTH samples are loaded at once and then consumed in order.  The state of a threshold is ten registers; one
// kernel per T keeps it out of scratch.  The last 32 values of a lane live in an LDS ring at word k*IDX_CELLS + thread (a lane
// reads its own bank, whatever k): a window sum re-adds `window` of them.  (Re-reading the window from global memory was measured
// and dropped; the variant stays behind exp_env.)  A period is not split over time, which would change the
// order of the fp64 sums: parallelism is cells x periods.
#include "common.h"
#include "ops.h"
#include "periods.h"
#include "prof.h"
#include <vector>

namespace {

constexpr int IDX_CELLS = 256;                         // cells (threads) per workgroup
constexpr int IDX_DEPTH = 8;                           // samples a lane has in flight
constexpr int IDX_RING = 32;                           // ring slots per lane = the largest window
struct IdxArgs {
    const float* x;
    size_t per;
    const long long* starts;                           // [P + 1], device
    unsigned P;
    const float* thr;
    int thr_per_cell, op, window;
    int* valid;
    int* event;
    float* ext;
    double* sum;
};

// GLOBAL_WINDOW: the window's values are read again from global memory (L2) instead of the LDS ring
template <int T, bool GLOBAL_WINDOW>
__global__ void __launch_bounds__(IDX_CELLS) climate_indices_kernel(const IdxArgs a) {
    __shared__ float ring[GLOBAL_WINDOW ? 1 : IDX_RING * IDX_CELLS];
    const int tid = threadIdx.x;
    const unsigned p = blockIdx.x % a.P;
    const size_t per = a.per, c = (size_t)(blockIdx.x / a.P) * IDX_CELLS + tid;
    const bool live = c < per;
    const size_t cc = live ? c : per - 1;                                 // an idle lane walks the last cell and stores nothing
    const size_t s0 = (size_t)a.starts[p], s1 = (size_t)a.starts[p + 1];
    const int len = (int)(s1 - s0), w = a.window;
    const auto [neg, strict] = decode_op(a.op);

    float thr[T];
    bool thr_ok[T];
    int n_event[T], run_e[T], run_n[T], long_e[T], long_n[T], n_runs[T], first[T], last[T];
    double esum[T];
#pragma unroll
    for (int t = 0; t < T; ++t) {
        const float v = a.thr_per_cell ? a.thr[(size_t)t * per + cc] : a.thr[t];
        thr_ok[t] = finite_f32(v);
        thr[t] = neg ? -v : v;
        n_event[t] = run_e[t] = run_n[t] = long_e[t] = long_n[t] = n_runs[t] = 0;
        first[t] = last[t] = -1;
        esum[t] = 0.0;
    }
    int n_valid = 0, run_v = 0;
    float vmax = -__builtin_inff(), vmin = __builtin_inff();
    double total = 0.0, wmax = -__builtin_inf();                          // a window sum is finite: -inf stands for "no window yet"

    const float* col = a.x + s0 * per + cc;                               // sample i of the period at col[i*per]
    for (int i0 = 0; i0 < len; i0 += IDX_DEPTH) {
        float blk[IDX_DEPTH];
#pragma unroll
        for (int u = 0; u < IDX_DEPTH; ++u) {
            const int i = i0 + u < len ? i0 + u : len - 1;
            blk[u] = col[(size_t)i * per];
        }
#pragma unroll
        for (int u = 0; u < IDX_DEPTH; ++u) {
            const int i = i0 + u;
            if (i >= len) break;                                          // (uniform)
            const bool ok = finite_f32(blk[u]);
            const float v = blk[u] == 0.f ? 0.f : blk[u];                 // -0.0 counts as +0.0
            if (!GLOBAL_WINDOW) ring[(i & (IDX_RING - 1)) * IDX_CELLS + tid] = v;
            const double d = (double)v;
            n_valid += ok ? 1 : 0;
            run_v = ok ? run_v + 1 : 0;
            if (ok) {
                total += d;
                vmax = v > vmax ? v : vmax;
                vmin = v < vmin ? v : vmin;
            }
            if (run_v >= w) {                                             // the window that ends at sample i, formed afresh
                double s = 0.0;
                for (int k = i - w + 1; k <= i; ++k)
                    s += (double)(GLOBAL_WINDOW ? (col[(size_t)k * per] == 0.f ? 0.f : col[(size_t)k * per])
                                                : ring[(k & (IDX_RING - 1)) * IDX_CELLS + tid]);
                wmax = s > wmax ? s : wmax;
            }
            const float cv = neg ? -v : v;
#pragma unroll
            for (int t = 0; t < T; ++t) {
                const bool ev = ok && (strict ? cv > thr[t] : cv >= thr[t]);
                const bool ne = ok && !ev;
                n_runs[t] += (ev && run_e[t] == 0) ? 1 : 0;
                run_e[t] = ev ? run_e[t] + 1 : 0;
                run_n[t] = ne ? run_n[t] + 1 : 0;
                long_e[t] = run_e[t] > long_e[t] ? run_e[t] : long_e[t];
                long_n[t] = run_n[t] > long_n[t] ? run_n[t] : long_n[t];
                n_event[t] += ev ? 1 : 0;
                first[t] = (ev && first[t] < 0) ? i : first[t];
                last[t] = ev ? i : last[t];
                if (ev) esum[t] += d;
            }
        }
    }
    if (!live) return;
    const double nan64 = __builtin_nan("");
    const float nan32 = __builtin_nanf("");
    if (a.valid) a.valid[(size_t)p * per + c] = n_valid;
    if (a.ext) {
        a.ext[((size_t)p * 2 + 0) * per + c] = n_valid ? vmax : nan32;
        a.ext[((size_t)p * 2 + 1) * per + c] = n_valid ? vmin : nan32;
    }
    if (a.sum) {
        double* o = a.sum + (size_t)p * (2 + T) * per + c;
        o[0] = n_valid ? total : nan64;
        o[per] = wmax == -__builtin_inf() ? nan64 : wmax;
#pragma unroll
        for (int t = 0; t < T; ++t) o[(size_t)(2 + t) * per] = thr_ok[t] ? esum[t] : nan64;
    }
    if (a.event) {
#pragma unroll
        for (int t = 0; t < T; ++t) {
            int* o = a.event + ((size_t)p * T + t) * 6 * per + c;
            const bool k = thr_ok[t];
            o[0] = k ? n_event[t] : -1;
            o[per] = k ? long_e[t] : -1;
            o[2 * per] = k ? long_n[t] : -1;
            o[3 * per] = k ? n_runs[t] : -1;
            o[4 * per] = k ? first[t] : -1;
            o[5 * per] = k ? last[t] : -1;
        }
    }
}

template <int T>
void idx_launch(hipStream_t s, const IdxArgs& a, unsigned blocks) {
    if (exp_env("DL4DS_INDICES_WINDOW_GLOBAL"))
        DL4DS_LAUNCH((climate_indices_kernel<T, true>), dim3(blocks), dim3(IDX_CELLS), 0, s, a);
    else
        DL4DS_LAUNCH((climate_indices_kernel<T, false>), dim3(blocks), dim3(IDX_CELLS), 0, s, a);
}

}  // namespace

size_t climate_indices_workspace_bytes(size_t N, size_t per, const long long* period_starts, int P, int T, int op, int window) {
    DL4DS_REQUIRE(N > 0 && per > 0, "climate_indices: empty array");
    DL4DS_REQUIRE(N < (size_t(1) << 31), "climate_indices: 2^31 or more samples are not supported");
    DL4DS_REQUIRE(P >= 1, "climate_indices: at least one period is needed");
    DL4DS_REQUIRE(T >= 1 && T <= IDX_MAX_THRESHOLDS, "climate_indices: 1 <= T <= 4 thresholds");
    DL4DS_REQUIRE(window >= 1 && window <= IDX_RING, "climate_indices: 1 <= window <= 32");
    DL4DS_REQUIRE(op >= 0 && op <= 3, "climate_indices: op must be 0 (>=), 1 (>), 2 (<) or 3 (<=)");
    check_period_starts("climate_indices", period_starts, P, N);
    DL4DS_REQUIRE(cdivz(per, IDX_CELLS) * (size_t)P < (size_t(1) << 31), "climate_indices: too many cells x periods for one launch");
    return period_starts_bytes(P);
}

void climate_indices(hipStream_t s, const float* x, size_t N, size_t per, const long long* period_starts, int P, const float* thr,
                     int T, int thr_per_cell, int op, int window, int* valid, int* event, float* ext, double* sum, void* workspace,
                     size_t workspace_bytes) {
    const size_t need = climate_indices_workspace_bytes(N, per, period_starts, P, T, op, window);          // (refuses a bad request)
    DL4DS_REQUIRE(x && thr, "climate_indices: null array or thresholds");
    DL4DS_REQUIRE(valid || event || ext || sum, "climate_indices: all four outputs are null");
    DL4DS_REQUIRE(workspace && workspace_bytes >= need, "climate_indices workspace too small");
    const long long* starts = upload_period_starts(s, period_starts, P, workspace);
    const IdxArgs a{x, per, starts, (unsigned)P, thr, thr_per_cell, op, window, valid, event, ext, sum};
    const unsigned blocks = (unsigned)(cdivz(per, IDX_CELLS) * (size_t)P);
    const double cells = (double)per * P;
    ProfScope ps(s, "climate_indices", 0.0,
                 4.0 * (double)N * (double)per + cells * ((valid ? 4.0 : 0.0) + (event ? 24.0 * T : 0.0) + (ext ? 8.0 : 0.0) +
                                                         (sum ? 8.0 * (2 + T) : 0.0)));
    switch (T) {
        case 1: idx_launch<1>(s, a, blocks); break;
        case 2: idx_launch<2>(s, a, blocks); break;
        case 3: idx_launch<3>(s, a, blocks); break;
        default: idx_launch<4>(s, a, blocks); break;
    }
    HIP_CHECK(hipGetLastError());
}
