// Quantile-mapping bias correction: the quantile table of one array per grid cell (fit) and the map that
// carries a value from the model's distribution onto the observed one (apply).  Arrays are fp32 (N, H, W, C); a cell is one
// (h, w, c), per = H*W*C, cell c of sample n lives at x[n*per + c].
//
// Table (quantile_table): the valid values of a cell are the finite ones among its N samples (NaN and +-inf are dropped, -0.0 is
// +0.0); with x_0 <= ... <= x_{n-1} the ascending valid values and q_i the Q probabilities (fp64, strictly increasing, in [0, 1]):
//   h = q_i*(n-1), j = floor(h), g = h - j, val = x_j + (x_{min(j+1, n-1)} - x_j) * g      in fp64, not contracted (numpy 'linear')
// rounded once to fp32 into table[i*per + c] ([Q][per]: neighbouring lanes of the map read neighbouring addresses); n = 0 gives NaN
// in all Q entries; valid[c] = n.  The cells' ascending keys come from the per-cell engine of cell_sort.h (stride per, no
// negation); 64 (or G) cells' Q values are then written by threads that run along the cells.  No floating-point atomics, no sum
// whose order could vary: a repeated call gives the same bits.
//
// Map (qmap_apply), m the model's historical table, o the observed one, f the table of the period being corrected (QDM only); the
// search table s is m for EQM and f for QDM.  Every operation is on fp32 and rounded on its own (no fused multiply-add, division
// correctly rounded).  For element value v in cell c:
//   1. v not finite: out = v                                                                              (n_nonfinite)
//   2. row 0 of a table in use is NaN at c (the cell is unfitted): out = NaN, or v with keep_unfitted      (n_unfitted)
//   3. v <  s[0]:   j = 0,   t = 0                                                                         (n_below)
//      v >= s[Q-1]: j = Q-1, t = 0                                                                         (n_above)
//      otherwise j = the largest index with s[j] <= v (so s[j+1] > v), t = (v - s[j]) / (s[j+1] - s[j])
//   4. o_t = o[j] at the two ends, else o[j] + (o[j+1] - o[j]) * t; m_t likewise from m
//   5. EQM in the interior: out = o_t.  QDM everywhere and EQM at the two ends: kind 0: out = v + (o_t - m_t); kind 1:
//      out = v * (o_t / m_t), and out = o_t where m_t == 0.
// A thread owns one cell and walks samples; a workgroup is 64 consecutive cells x 4 waves, wave w taking every fourth sample of
// the workgroup's share, so x, out and every table row are read 256 contiguous bytes per wave-instruction.  The tables of the 64
// cells are staged in LDS as [q][64]: a lane reads word q*64 + lane, its own bank whatever q it is at.  All tables in use are
// staged while they fit QM_LDS_BUDGET (two workgroups per CU); beyond that only the search table is, and the o / m rows at j and
// j + 1 come from global memory (L2).  The samples are split over workgroups when the cells alone would leave CUs idle.  Counts:
// per-thread integers, summed per wave, then in LDS (where the tables were), then one integer atomic per workgroup and counter.
#include "common.h"
#include "ops.h"
#include "prof.h"
#include "cell_sort.h"
#include <algorithm>
#include <cmath>

// every product, sum and quotient of the map is rounded on its own, like the numpy float32 restatement
#pragma clang fp contract(off)

namespace {

constexpr int QM_MAX_Q = 256;                          // (the C header states it)
constexpr int QM_CELLS = 64;                           // map: cells per workgroup, one per lane
constexpr int QM_THREADS = 256;                        // map: 4 waves, each on its own samples
constexpr int QM_WAVES = QM_THREADS / 64;
constexpr int QM_UNROLL = 4;                           // map: samples a lane has in flight
constexpr size_t QM_LDS_BUDGET = size_t(80) << 10;     // map: staged tables of a workgroup, two workgroups per 160 KiB CU
constexpr size_t QM_TARGET_BLOCKS = 2048;              // map: 256 CUs x 8
constexpr size_t QM_MIN_WALK = 16;                     // map: fewest samples of a workgroup when the samples are split
constexpr size_t QM_MAX_WALK = size_t(1) << 30;        // map: most samples of a workgroup (32-bit counts per lane)

struct QuantParams {
    double q[QM_MAX_Q];
    int Q;
};

// ------------------------------------------------------------------------------------------------------------------- the fit
// Q values of `cells` cells (the first is cell c0) whose sorted keys are row(g) and whose valid counts are n[g]: threads along g
template <typename Row>
__device__ __forceinline__ void write_tables(const QuantParams& prm, Row row, const uint32_t* n, int cells, size_t c0, size_t per,
                                             int t, int T, float* __restrict__ table) {
    for (int i = t; i < prm.Q * cells; i += T) {
        const int qi = i / cells, g = i % cells;
        table[(size_t)qi * per + c0 + g] = (float)quantile_of(row(g), n[g], prm.q[qi]);
    }
}

// strided LDS engine: G cells of N <= P samples per workgroup
template <int P>
__global__ void __launch_bounds__(CELL_THREADS) qtab_lds_kernel(const float* __restrict__ x, size_t N, size_t per, const QuantParams prm,
                                                               float* __restrict__ table, long long* __restrict__ valid) {
    constexpr int T = CELL_THREADS, G = cell_group<P>(), PITCH = P + 1;
    extern __shared__ __attribute__((aligned(16))) unsigned char qtab_lds[];
    uint32_t* key = reinterpret_cast<uint32_t*>(qtab_lds);                // [G][PITCH]
    __shared__ uint32_t nn[G];
    const int t = threadIdx.x;
    const size_t c0 = (size_t)blockIdx.x * G;
    const int cells = (int)(per - c0 < (size_t)G ? per - c0 : (size_t)G);
    sorted_cell_rows<P>(x, N, per, false, c0, cells, key);
    if (t < G) nn[t] = bound<true>(key + t * PITCH, (uint32_t)P, SORT_INVALID);
    __syncthreads();
    if (valid && t < cells) valid[c0 + t] = (long long)nn[t];
    write_tables(prm, [&](int g) { return (const uint32_t*)(key + g * PITCH); }, nn, cells, c0, per, t, T, table);
}

// global engine, step 3: 64 cells of the chunk per workgroup, from their sorted keys
__global__ void __launch_bounds__(SORT_THREADS) qtab_finish_kernel(const uint32_t* __restrict__ k, size_t ncell, size_t N, size_t per,
                                                                 size_t cell0, const QuantParams prm, float* __restrict__ table,
                                                                 long long* __restrict__ valid) {
    __shared__ uint32_t nn[CELL_TR];
    const int t = threadIdx.x;
    const size_t c0 = (size_t)blockIdx.x * CELL_TR;
    const int cells = (int)(ncell - c0 < (size_t)CELL_TR ? ncell - c0 : (size_t)CELL_TR);
    if (t < cells) {
        nn[t] = bound<true>(k + (c0 + t) * N, (uint32_t)N, SORT_INVALID);
        if (valid) valid[cell0 + c0 + t] = (long long)nn[t];
    }
    __syncthreads();
    write_tables(prm, [&](int g) { return k + (c0 + g) * N; }, nn, cells, cell0 + c0, per, t, SORT_THREADS, table);
}

// --------------------------------------------------------------------------------------------------------------------- the map
struct MapArgs {
    const float* x;
    float* out;
    size_t B, per, walk;                               // walk: samples per workgroup (blockIdx.y)
    const float *s, *o, *m;                            // search table (m or f), observed, model
    int Q, iters, kind, keep_unfitted;                 // iters: steps of the binary search over Q knots
    unsigned long long* counts;
};

struct Tab {                                           // a table of the workgroup's cells as one lane reads it: knot q at p[q*pitch]
    const float* p;
    size_t pitch;
    __device__ __forceinline__ float operator[](int q) const { return p[(size_t)q * pitch]; }
};

__device__ __forceinline__ float lerp_knots(const Tab& a, int j, float t, bool end) {
    const float a0 = a[j];
    if (end) return a0;
    return a0 + (a[j + 1] - a0) * t;
}

// QDM: s = f, m and o are separate tables; EQM: s is m.  ALL: o (and m for QDM) are staged in LDS next to s
template <bool QDM, bool ALL>
__global__ void __launch_bounds__(QM_THREADS) qmap_apply_kernel(const MapArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char qmap_lds[];
    float* lds = reinterpret_cast<float*>(qmap_lds);                      // [tables][Q][QM_CELLS]
    const int t = threadIdx.x, lane = t & 63, w = t >> 6, Q = a.Q;
    const size_t c0 = (size_t)blockIdx.x * QM_CELLS, c = c0 + lane;
    const bool live = c < a.per;
    constexpr int STAGED = ALL ? (QDM ? 3 : 2) : 1;
    const float* src[3] = {a.s, a.o, a.m};
    for (int k = 0; k < STAGED; ++k)
        for (int i = t; i < Q * QM_CELLS; i += QM_THREADS) {
            const size_t cell = c0 + (i & 63);
            lds[k * Q * QM_CELLS + i] = cell < a.per ? src[k][(size_t)(i >> 6) * a.per + cell] : 0.f;
        }
    __syncthreads();
    const size_t cc = live ? c : 0;                                       // a dead lane reads cell 0 of global tables and stores nothing
    const Tab S{lds + lane, QM_CELLS};
    const Tab O = ALL ? Tab{lds + Q * QM_CELLS + lane, QM_CELLS} : Tab{a.o + cc, a.per};
    const Tab M = !QDM ? S : ALL ? Tab{lds + 2 * Q * QM_CELLS + lane, QM_CELLS} : Tab{a.m + cc, a.per};
    const float s_lo = S[0], s_hi = S[Q - 1];
    const float o0 = O[0], m0 = M[0];
    const bool unfitted = (s_lo != s_lo) || (o0 != o0) || (m0 != m0);
    uint32_t n_nonfinite = 0, n_unfitted = 0, n_below = 0, n_above = 0;
    const size_t b0 = (size_t)blockIdx.y * a.walk, b1 = b0 + a.walk < a.B ? b0 + a.walk : a.B;
    for (size_t b = b0 + w; b < b1 && live; b += (size_t)QM_WAVES * QM_UNROLL) {
        float v[QM_UNROLL];
#pragma unroll
        for (int u = 0; u < QM_UNROLL; ++u) {
            const size_t bu = b + (size_t)u * QM_WAVES;
            v[u] = a.x[(bu < b1 ? bu : b) * a.per + c];
        }
#pragma unroll
        for (int u = 0; u < QM_UNROLL; ++u) {
            const size_t bu = b + (size_t)u * QM_WAVES;
            if (bu >= b1) break;
            const float x = v[u];
            float r;
            if (!finite_bits(x)) {
                r = x;
                ++n_nonfinite;
            } else if (unfitted) {
                r = a.keep_unfitted ? x : __builtin_nanf("");
                ++n_unfitted;
            } else {
                const bool below = x < s_lo, above = x >= s_hi, end = below || above;
                int lo = 0, hi = Q - 1;                                   // s[lo] <= x < s[hi] in the interior
                for (int it = 0; it < a.iters; ++it) {
                    const int mid = (lo + hi) >> 1;                       // lo <= mid < hi: every read stays inside [0, Q - 2]
                    const bool le = S[mid] <= x;
                    lo = le ? mid : lo;
                    hi = le ? hi : mid;
                }
                const int j = below ? 0 : above ? Q - 1 : lo;
                float tt = 0.f;
                if (!end) {
                    const float sj = S[j];
                    tt = (x - sj) / (S[j + 1] - sj);
                }
                n_below += below;
                n_above += above;
                const float ot = lerp_knots(O, j, tt, end);
                if (!QDM && !end) {
                    r = ot;
                } else {
                    const float mt = lerp_knots(M, j, tt, end);
                    if (a.kind == 0) r = x + (ot - mt);
                    else r = mt == 0.f ? ot : x * (ot / mt);
                }
            }
            a.out[bu * a.per + c] = r;
        }
    }
    if (a.counts) {
        // the workgroup's totals take the place of the staged tables, which every wave has finished with: no LDS of their own, so
        // that two workgroups of QM_LDS_BUDGET fit a CU
        unsigned long long* tot = reinterpret_cast<unsigned long long*>(qmap_lds);
        __syncthreads();
        if (t < 4) tot[t] = 0ull;
        __syncthreads();
        unsigned long long cnt[4] = {n_nonfinite, n_unfitted, n_below, n_above};
#pragma unroll
        for (int k = 0; k < 4; ++k) {
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) cnt[k] += __shfl_down(cnt[k], o, 64);
            if (lane == 0 && cnt[k]) atomicAdd(&tot[k], cnt[k]);
        }
        __syncthreads();
        if (t < 4 && tot[t]) atomicAdd(&a.counts[t], tot[t]);
    }
}

template <bool QDM, bool ALL>
void launch_map(hipStream_t s, const MapArgs& a, dim3 grid, size_t lds) {
    auto kern = qmap_apply_kernel<QDM, ALL>;
    static bool once = false;
    if (!once) {
        HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize,
                                      (int)QM_LDS_BUDGET));
        once = true;
    }
    DL4DS_LAUNCH(kern, grid, dim3(QM_THREADS), lds, s, a);
    HIP_CHECK(hipGetLastError());
}

QuantParams checked_probabilities(const double* q, int Q) {
    DL4DS_REQUIRE(Q >= 2 && Q <= QM_MAX_Q, "quantile mapping: between 2 and 256 probabilities are supported");
    DL4DS_REQUIRE(q, "quantile mapping: null probabilities");
    QuantParams prm = {};
    for (int i = 0; i < Q; ++i) {
        DL4DS_REQUIRE(q[i] >= 0.0 && q[i] <= 1.0, "quantile mapping: probabilities must lie in [0, 1]");
        DL4DS_REQUIRE(i == 0 || q[i] > q[i - 1], "quantile mapping: probabilities must be strictly increasing");
        prm.q[i] = q[i];
    }
    prm.Q = Q;
    return prm;
}

}  // namespace

size_t quantile_table_workspace_bytes(size_t N, size_t per) {
    DL4DS_REQUIRE(N > 0 && per > 0, "quantile_table: empty array");
    DL4DS_REQUIRE(N < (size_t(1) << 31), "quantile_table: 2^31 or more samples are not supported");
    DL4DS_REQUIRE(per < (size_t(1) << 36), "quantile_table: too many cells");
    return cell_sort_workspace_bytes(N, per);
}

void quantile_table(hipStream_t s, const float* x, size_t N, size_t per, const double* q, int Q, float* table, long long* valid,
                    void* workspace, size_t workspace_bytes) {
    const QuantParams prm = checked_probabilities(q, Q);
    const size_t need = quantile_table_workspace_bytes(N, per);           // (refuses an empty or oversized array)
    DL4DS_REQUIRE(x && table, "quantile_table: null array or table");
    if (need) DL4DS_REQUIRE(workspace_bytes >= need, "quantile_table workspace too small");
    cell_sort(
        s, "quantile_table", x, N, per, per, 0, workspace,
        [&](auto P) { launch_cell_lds<P(), qtab_lds_kernel<P()>>(s, per, x, N, per, prm, table, valid); },
        [&](const uint32_t* keys, size_t nc, size_t c0) {
            DL4DS_LAUNCH(qtab_finish_kernel, dim3((unsigned)cdivz(nc, CELL_TR)), dim3(SORT_THREADS), 0, s, keys, nc, N, per, c0, prm, table,
                         valid);
        });
}

void qmap_apply(hipStream_t s, const float* x, float* out, size_t B, size_t per, const float* model_tab, const float* obs_tab,
                const float* target_tab, int Q, int kind, int keep_unfitted, unsigned long long* counts) {
    DL4DS_REQUIRE(Q >= 2 && Q <= QM_MAX_Q, "qmap_apply: between 2 and 256 probabilities are supported");
    DL4DS_REQUIRE(kind == 0 || kind == 1, "qmap_apply: kind must be 0 (additive) or 1 (multiplicative)");
    DL4DS_REQUIRE(x && out && model_tab && obs_tab, "qmap_apply: null array or table");
    DL4DS_REQUIRE(per > 0, "qmap_apply: empty cells");
    const size_t groups = cdivz(per, QM_CELLS);
    DL4DS_REQUIRE(groups < (size_t(1) << 31), "qmap_apply: too many cells");
    if (B == 0) return;
    const bool qdm = target_tab != nullptr;
    // the samples are split until the grid fills the device, a workgroup keeping enough of them to pay for staging its tables
    size_t splits = std::max<size_t>(1, std::min(cdivz(QM_TARGET_BLOCKS, groups), B / QM_MIN_WALK));
    splits = std::max(splits, cdivz(B, QM_MAX_WALK));
    const size_t walk = cdivz(B, splits);
    splits = cdivz(B, walk);
    DL4DS_REQUIRE(splits <= 65535, "qmap_apply: too many samples for one launch");
    const size_t one = (size_t)Q * QM_CELLS * sizeof(float);
    const bool all = one * (qdm ? 3 : 2) <= QM_LDS_BUDGET;
    const size_t lds = all ? one * (qdm ? 3 : 2) : one;
    int iters = 0;
    while ((1 << iters) < Q - 1) ++iters;                                 // the bracket [lo, hi] starts Q - 1 knots wide
    const MapArgs a{x, out, B, per, walk, qdm ? target_tab : model_tab, obs_tab, model_tab, Q, iters, kind, keep_unfitted, counts};
    ProfScope ps(s, qdm ? "qmap_apply_qdm" : "qmap_apply_eqm", 0.0, 8.0 * (double)B * (double)per);
    const dim3 grid((unsigned)groups, (unsigned)splits);
    if (qdm) { if (all) launch_map<true, true>(s, a, grid, lds); else launch_map<true, false>(s, a, grid, lds); }
    else { if (all) launch_map<false, true>(s, a, grid, lds); else launch_map<false, false>(s, a, grid, lds); }
}
