// Distance-map verification of the N*C fields (planes) of two (N, H, W, C) arrays: per field and threshold the exact squared
// Euclidean distance transform of the observed and of the predicted event set, and on top of the two maps the sums of the Hausdorff
// distance, the mean error distances, Baddeley's Delta and Pratt's figure of merit.
//
// A cell is VALID iff y and p are both finite there; A = valid & (y >= t), B = valid & (p >= t) on float32.  d2(x, S) = min over
// s in S of the squared cell distance, DC_DIST_EMPTY = 2^31 - 1 for an empty S.  Distances pass through invalid cells; sums do not.
//
// Plain launches on one stream, no workgroup waits for another, every loop is bounded by H, W or the number of segments.  Every
// index, distance, early exit and score term is distance_core.h's, which tools/distance_host_check.cpp runs cell by cell with
// checked accesses.  Per chunk of fields and group of at most DC_TG thresholds:
//   col    one lane per column walks the H rows down and up again: g = the vertical distance to the column's nearest event, for
//          both sides and every threshold of the group from one read of y and p (lanes along j: the stride-C reads coalesce as far
//          as C allows).  g is stored in 16 bits: the size rule keeps H below 46342.
//   row    one wave per row (a workgroup of 64): the row of g^2 of both sides goes into LDS a segment at a time; lane j scans the
//          columns outward from j and stops once o^2 + (the segment's smallest g^2) >= its best; segments are visited outward from
//          the lane's own and skipped once no lane can gain from them.  The two maps stay in registers: the lane adds its cells'
//          terms in ascending j, one fixed shuffle tree joins the 64 lanes, lane 0 writes the row's 8 integers and 7 doubles.
//   final  one workgroup per (field, threshold): thread t joins the rows t, t + 256, ... in ascending order, a fixed tree joins the
//          256 partial results.
// No atomics at all: integers and maps are pure functions of the input, the fp64 sums have one summation order that depends on
// (H, W) alone, so a repeated call gives the same bits and nothing depends on N, on the chunking or on the threshold grouping.
#include "distance_core.h"
#include "ops.h"
#include "prof.h"
#include "runtime.h"
#include <algorithm>
#include <cmath>

namespace {

constexpr int DIST_FINAL_THREADS = 256;
constexpr size_t DIST_WS_BUDGET = size_t(128) << 20;      // workspace of one chunk of fields
constexpr size_t DIST_MAX_GRID_Y = 65535;

struct DistThresholds {
    float t[DC_TG];                                       // an unused slot holds +inf and is never looked at
    int count;
};

typedef uint16_t GT;                                      // a stored g: H <= 46341 by the size rule, so 16 bits hold it

__global__ void __launch_bounds__(64) dist_col_kernel(const float* __restrict__ y, const float* __restrict__ p, int H, int W, int C,
                                                      size_t field0, DistThresholds thr, GT* __restrict__ g) {
    const size_t fl = blockIdx.y, f = field0 + fl;
    const int lane = threadIdx.x;
    const int j = (int)blockIdx.x * 64 + lane;
    if (j >= W) return;
    {
        int since[2][DC_TG];
#pragma unroll
        for (int k = 0; k < DC_TG; ++k) since[0][k] = since[1][k] = DC_G_NONE;
        for (int i = 0; i < H; ++i) {
            const size_t o = dc_x_index(f, i, j, H, W, C);
            const float yv = y[o], pv = p[o];
            const bool ok = dc_valid(yv, pv);
#pragma unroll
            for (int k = 0; k < DC_TG; ++k) {
                if (k < thr.count) {                                      // uniform
                    since[0][k] = dc_col_step(since[0][k], dc_event(ok, yv, thr.t[k]));
                    since[1][k] = dc_col_step(since[1][k], dc_event(ok, pv, thr.t[k]));
                    g[dc_g_index(fl, thr.count, k, 0, H, W, i, j)] = dc_g_pack(since[0][k]);
                    g[dc_g_index(fl, thr.count, k, 1, H, W, i, j)] = dc_g_pack(since[1][k]);
                }
            }
        }
#pragma unroll
        for (int k = 0; k < DC_TG; ++k) since[0][k] = since[1][k] = DC_G_NONE;
        for (int i = H - 1; i >= 0; --i) {
#pragma unroll
            for (int k = 0; k < DC_TG; ++k) {
                if (k < thr.count) {
#pragma unroll
                    for (int side = 0; side < 2; ++side) {
                        GT* at = g + dc_g_index(fl, thr.count, k, side, H, W, i, j);
                        const int down = dc_g_unpack(*at);
                        since[side][k] = dc_col_step(since[side][k], down == 0);
                        const int m = dc_col_join(down, since[side][k]);
                        if (m != down) *at = dc_g_pack(m);
                    }
                }
            }
        }
    }
}

__device__ __forceinline__ int wave_min_all(int v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = min(v, __shfl_xor(v, o, 64));
    return v;
}

__global__ void __launch_bounds__(64) dist_row_kernel(const float* __restrict__ y, const float* __restrict__ p, int H, int W, int C,
                                                      size_t field0, int tcount, int T, int t0, int seg, const GT* __restrict__ g,
                                                      double cutoff, double alpha, long long* __restrict__ pc, double* __restrict__ ps,
                                                      int* __restrict__ d2_obs, int* __restrict__ d2_pred) {
    __shared__ int row2[2][DC_SEG_MAX];
    const int lane = threadIdx.x;
    const size_t fl = blockIdx.y / (unsigned)tcount, f = field0 + fl;
    const int k = (int)(blockIdx.y % (unsigned)tcount);
    const int nseg = dc_segments(W, seg);
    const int i = (int)blockIdx.x;
    {
        const GT* ga = g + dc_g_index(fl, tcount, k, 0, H, W, i, 0);
        const GT* gb = g + dc_g_index(fl, tcount, k, 1, H, W, i, 0);
        DcTerms acc;
        dc_zero(&acc);
        int staged = -1, mina = DC_DIST_EMPTY, minb = DC_DIST_EMPTY;
        for (int j0 = 0; j0 < W; j0 += 64) {
            const bool in = j0 + lane < W;
            const int j = in ? j0 + lane : W - 1;
            const int own = j0 / seg;
            int da = DC_DIST_EMPTY, db = DC_DIST_EMPTY;
            for (int step = 0; step < 2 * nseg - 1; ++step) {
                const int s = dc_seg_visit(own, step);
                if (s < 0 || s >= nseg) continue;                          // (uniform)
                const int a = s * seg, b = min(a + seg, W);
                const int o0 = dc_seg_offset(j, a, b);
                if (!__any(in && dc_seg_needed(o0, max(da, db)))) continue; // (uniform) no lane of the wave can gain from it
                if (staged != s) {
                    __syncthreads();                                       // the scans of the segment before are done
                    int ma = DC_DIST_EMPTY, mb = DC_DIST_EMPTY;
                    for (int c = lane; c < b - a; c += 64) {
                        const int va = dc_g2(dc_g_unpack(ga[a + c])), vb = dc_g2(dc_g_unpack(gb[a + c]));
                        row2[0][c] = va; row2[1][c] = vb;
                        ma = min(ma, va); mb = min(mb, vb);
                    }
                    mina = wave_min_all(ma); minb = wave_min_all(mb);
                    staged = s;
                    __syncthreads();
                }
                da = dc_row_scan(row2[0], a, b, mina, j, da);
                db = dc_row_scan(row2[1], a, b, minb, j, db);
            }
            if (in) {
                const size_t o = dc_x_index(f, i, j, H, W, C);
                DcTerms t;
                dc_cell_terms(dc_valid(y[o], p[o]), da, db, cutoff, alpha, &t);
                dc_join(&acc, &t);
                const size_t m = (dc_out_index(f, T, t0 + k) * (size_t)H + (size_t)i) * (size_t)W + (size_t)j;
                if (d2_obs) d2_obs[m] = da;
                if (d2_pred) d2_pred[m] = db;
            }
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {                                 // the fixed tree over the 64 lanes; lane 0 holds the row
            DcTerms t;
#pragma unroll
            for (int q = 0; q < DC_NCOUNT; ++q) t.c[q] = __shfl_down(acc.c[q], o, 64);
#pragma unroll
            for (int q = 0; q < DC_NSUM; ++q) t.s[q] = __shfl_down(acc.s[q], o, 64);
            dc_join(&acc, &t);
        }
        if (lane == 0) {
            long long* c = pc + dc_partial_index(fl, tcount, k, H, i, DC_NCOUNT);
            double* s = ps + dc_partial_index(fl, tcount, k, H, i, DC_NSUM);
#pragma unroll
            for (int q = 0; q < DC_NCOUNT; ++q) c[q] = acc.c[q];
#pragma unroll
            for (int q = 0; q < DC_NSUM; ++q) s[q] = acc.s[q];
        }
    }
}

// One workgroup per (field of the chunk, threshold of the group).
__global__ void __launch_bounds__(DIST_FINAL_THREADS) dist_final_kernel(int H, size_t field0, int tcount, int T, int t0,
                                                                        const long long* __restrict__ pc, const double* __restrict__ ps,
                                                                        long long* __restrict__ counts, double* __restrict__ sums) {
    __shared__ DcTerms red[DIST_FINAL_THREADS];
    const int t = threadIdx.x;
    const size_t fl = blockIdx.x / (unsigned)tcount;
    const int k = (int)(blockIdx.x % (unsigned)tcount);
    DcTerms acc;
    dc_zero(&acc);
    for (int i = t; i < H; i += DIST_FINAL_THREADS) {
        const long long* c = pc + dc_partial_index(fl, tcount, k, H, i, DC_NCOUNT);
        const double* s = ps + dc_partial_index(fl, tcount, k, H, i, DC_NSUM);
        DcTerms r;
#pragma unroll
        for (int q = 0; q < DC_NCOUNT; ++q) r.c[q] = c[q];
#pragma unroll
        for (int q = 0; q < DC_NSUM; ++q) r.s[q] = s[q];
        dc_join(&acc, &r);
    }
    red[t] = acc;
    __syncthreads();
    for (int o = DIST_FINAL_THREADS / 2; o > 0; o >>= 1) {
        if (t < o) dc_join(&red[t], &red[t + o]);
        __syncthreads();
    }
    if (t < DC_NCOUNT) counts[dc_out_index(field0 + fl, T, t0 + k) * DC_NCOUNT + t] = red[0].c[t];
    if (t < DC_NSUM) sums[dc_out_index(field0 + fl, T, t0 + k) * DC_NSUM + t] = red[0].s[t];
}

struct DistPlan {
    int tcount;                                            // thresholds of a full group
    size_t gsize, cells, fields;                           // bytes of a g entry; cells per field; fields of one chunk
    size_t partial_bytes(size_t n) const { return n * (size_t)tcount * rows * (DC_NCOUNT + DC_NSUM) * 8; }
    size_t rows;
    size_t bytes() const { return partial_bytes(fields) + fields * (size_t)tcount * 2 * cells * gsize; }
};
DistPlan plan(size_t fields, int H, int W, int T) {
    DistPlan p;
    p.tcount = std::min(T, DC_TG);
    p.gsize = sizeof(GT);
    p.cells = (size_t)H * W;
    p.rows = (size_t)H;
    const size_t per = (size_t)p.tcount * (2 * p.cells * p.gsize + p.rows * (DC_NCOUNT + DC_NSUM) * 8);
    p.fields = std::max<size_t>(1, std::min({fields, DIST_WS_BUDGET / per, DIST_MAX_GRID_Y / (size_t)p.tcount}));
    return p;
}

// the columns of a row segment: DC_SEG_MAX, lowered by the tests so that small fields cross a segment
int segment_columns() {
    int seg = DC_SEG_MAX;
    if (const char* e = test_env("DL4DS_EDT_SEG")) { const int n = atoi(e); if (n >= 1) seg = std::min(seg, n); }
    return seg;
}

void run(hipStream_t st, const float* y, const float* p, int H, int W, int C, size_t F, const float* thresholds, int T, double cutoff,
         double alpha, long long* counts, double* sums, int* d2_obs, int* d2_pred, void* workspace, const DistPlan& pl) {
    long long* pc = static_cast<long long*>(workspace);                    // [fields][tcount][H][8]
    double* ps = reinterpret_cast<double*>(pc + pl.fields * (size_t)pl.tcount * pl.rows * DC_NCOUNT);
    GT* g = reinterpret_cast<GT*>(ps + pl.fields * (size_t)pl.tcount * pl.rows * DC_NSUM);
    const int seg = segment_columns();
    const unsigned col_x = (unsigned)((W + 63) / 64), row_x = (unsigned)H;   // H, W <= 46341 by the size rule
    const double maps = (d2_obs ? 4.0 : 0.0) + (d2_pred ? 4.0 : 0.0);
    for (size_t f0 = 0; f0 < F; f0 += pl.fields) {
        const size_t fc = std::min(pl.fields, F - f0);
        for (int t0 = 0; t0 < T; t0 += DC_TG) {
            DistThresholds thr;
            thr.count = std::min(DC_TG, T - t0);
            for (int k = 0; k < DC_TG; ++k) thr.t[k] = k < thr.count ? thresholds[t0 + k] : INFINITY;
            const double nc = (double)fc * (double)pl.cells, gb = 2.0 * thr.count * sizeof(GT);
            {   // (profiler tags distance_col, distance_row, distance_final: kernel time per step, bytes = its algorithmic traffic)
                ProfScope scope(st, "distance_col", 0.0, nc * (8.0 + 2.0 * gb));
                DL4DS_LAUNCH(dist_col_kernel, dim3(col_x, (unsigned)fc), dim3(64), 0, st, y, p, H, W, C, f0, thr, g);
            }
            {
                ProfScope scope(st, "distance_row", 0.0, nc * (gb + thr.count * (8.0 + maps)));
                DL4DS_LAUNCH(dist_row_kernel, dim3(row_x, (unsigned)(fc * thr.count)), dim3(64), 0, st, y, p, H, W, C, f0, thr.count,
                             T, t0, seg, (const GT*)g, cutoff, alpha, pc, ps, d2_obs, d2_pred);
            }
            {
                ProfScope scope(st, "distance_final", 0.0, (double)fc * thr.count * (double)H * (DC_NCOUNT + DC_NSUM) * 8.0);
                DL4DS_LAUNCH(dist_final_kernel, dim3((unsigned)(fc * thr.count)), dim3(DIST_FINAL_THREADS), 0, st, H, f0, thr.count, T,
                             t0, (const long long*)pc, (const double*)ps, counts, sums);
            }
        }
    }
    HIP_CHECK(hipGetLastError());
}

}  // namespace

void distance_check_args(const float* y, const float* p, int N, int H, int W, int C, const float* thresholds, int T, double cutoff,
                         double alpha, const long long* counts, const double* sums) {
    DL4DS_REQUIRE(N >= 1 && H >= 1 && W >= 1 && C >= 1 && T >= 1, "distance_scores: expected N, H, W, C, T >= 1");
    DL4DS_REQUIRE(dc_sizes_ok(H, W), "distance_scores: (H-1)^2 + (W-1)^2 must stay below 2^31 - 1 and H*W below 2^31");
    DL4DS_REQUIRE(y && p && thresholds && counts && sums, "distance_scores: both arrays, the thresholds, counts and sums are needed");
    for (int t = 0; t < T; ++t) DL4DS_REQUIRE(std::isfinite(thresholds[t]), "distance_scores: thresholds must be finite");
    DL4DS_REQUIRE(cutoff > 0, "distance_scores: cutoff must be > 0 (it may be +inf)");
    DL4DS_REQUIRE(alpha > 0 && std::isfinite(alpha), "distance_scores: alpha must be positive and finite");
}

size_t distance_workspace_bytes(int N, int H, int W, int C, int T) {
    if (N <= 0 || H <= 0 || W <= 0 || C <= 0 || T <= 0 || !dc_sizes_ok(H, W)) return 0;
    return plan((size_t)N * C, H, W, T).bytes();
}

void distance_scores(hipStream_t st, const float* y, const float* p, int N, int H, int W, int C, const float* thresholds, int T,
                     double cutoff, double alpha, long long* counts, double* sums, int* d2_obs, int* d2_pred, void* workspace,
                     size_t workspace_bytes) {
    distance_check_args(y, p, N, H, W, C, thresholds, T, cutoff, alpha, counts, sums);
    const size_t F = (size_t)N * C;
    const DistPlan pl = plan(F, H, W, T);
    DL4DS_REQUIRE(workspace && workspace_bytes >= pl.bytes(), "distance_scores workspace too small");
    run(st, y, p, H, W, C, F, thresholds, T, cutoff, alpha, counts, sums, d2_obs, d2_pred, workspace, pl);
}
