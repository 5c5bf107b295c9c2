// Regridding between rectilinear grids and the consistency sums of a regridded field.
//
// x [N][H][W][C] fp32 -> out [N][H'][W'][C] fp32 through two axis tables (CSR: ptr, idx, w in fp64; regrid_core.h), uploaded once
// per plan.  One thread owns one output element (the 4-byte form) or four consecutive channels of one output cell (the 16-byte
// form: C a multiple of 4, both pointers 16-byte aligned) and walks the y-taps of its row in table order and, inside each, the
// x-taps of its column in table order, accumulating in fp64 with every operation rounded on its own (rg_walk, rg_finish).  No
// atomics: an element is a pure function of the input and the tables, whatever N and however the samples are split into calls.
//
// A workgroup is one slab of RG_THREADS lanes of ONE output row: the row's y-taps are wave-uniform (scalar loads), the x-taps of
// the columns the slab spans are staged into LDS once (idx and w, at most RG_LDS_TAPS of them; a longer list, a heavy coarsening
// of a short row, is read from the table in global memory, which every workgroup of the row shares in cache).  Lanes run along
// (j', c), so the loads of x coalesce over c and, where the x-taps of neighbouring columns are neighbours, over j.
//
// Traffic.  Coarsening by r reads every input element about once (the taps of neighbouring outputs tile the input; the lines a
// wave touches are finished by its next tap) and writes the output once: 4 * N * C * (H W + H' W') bytes.  Refining re-reads each
// input line from cache about r^2 times; HBM sees the same two terms.  The tables are a few KiB.
//
// Consistency (regrid_consistency): r = the value apply stores, y = ref[n, i', j', c]; per (n, c) the six sums and two counts of
// regrid_core.h in its ONE order: a workgroup per (n, i') row, lane t joins the cells j' = t, t + 256, ... ascending for one channel
// at a time, an LDS tree joins the lanes, the row partials are joined in ascending i' by one thread per (n, c).  Nothing of r is
// stored unless the residual is asked for.
#include "ops.h"
#include "prof.h"
#include "regrid_core.h"
#include <algorithm>

namespace {

struct RegridTables {
    const int* yptr; const int* yidx; const double* yw;      // [H' + 1], [nnz_y], [nnz_y]
    const int* xptr; const int* xidx; const double* xw;      // [W' + 1], [nnz_x], [nnz_x]
    const double* ay; const double* ax;                      // [H'], [W']
    int H, W, Ho, Wo;
};

struct XTable {
    int lds_idx[RG_LDS_TAPS];
    double lds_w[RG_LDS_TAPS];
};

// the x-taps of the columns [j0, j1) -> LDS (when they fit); -> the first tap
__device__ inline int stage_x(const RegridTables& t, int j0, int j1, XTable& xt, bool* in_lds) {
    const int p0 = t.xptr[j0], p1 = t.xptr[j1];
    *in_lds = rg_taps_in_lds(p1 - p0);
    if (*in_lds) {
        for (int k = threadIdx.x; k < p1 - p0; k += RG_THREADS) {
            xt.lds_idx[k] = t.xidx[p0 + k];
            xt.lds_w[k] = t.xw[p0 + k];
        }
    }
    __syncthreads();
    return p0;
}

template <int V>
__device__ inline void cell_value(const RegridTables& t, const XTable& xt, bool in_lds, int p0, const float* xs, int C, int i, int j,
                                  int c, bool skipna, double min_valid, float* r) {
    RgAcc acc[V];
    const int ya = t.yptr[i], yb = t.yptr[i + 1];
    const int xa = t.xptr[j], xb = t.xptr[j + 1];
    if (in_lds) rg_walk<V>(xs, t.W, C, t.yidx, t.yw, ya, yb, xt.lds_idx, xt.lds_w, xa - p0, xb - p0, c, skipna, acc);
    else rg_walk<V>(xs, t.W, C, t.yidx, t.yw, ya, yb, t.xidx, t.xw, xa, xb, c, skipna, acc);
#pragma unroll
    for (int k = 0; k < V; ++k) r[k] = rg_finish(acc + k, min_valid);
}

// grid: x = (row slab, output row), y = sample
template <int V>
__global__ void __launch_bounds__(RG_THREADS) regrid_apply_kernel(const RegridTables t, const float* __restrict__ x, float* __restrict__ out,
                                                                  int C, int skipna, double min_valid) {
    __shared__ XTable xt;
    const int nb = rg_row_blocks((rg_i64)t.Wo * C, V);
    const int i = blockIdx.x / nb, b = blockIdx.x - i * nb;
    const size_t n = blockIdx.y;
    int j0, j1;
    rg_block_cols(b, V, t.Wo, C, &j0, &j1);
    bool in_lds;
    const int p0 = stage_x(t, j0, j1, xt, &in_lds);
    const rg_i64 e = ((rg_i64)b * RG_THREADS + threadIdx.x) * V;
    if (e >= (rg_i64)t.Wo * C) return;
    const int j = (int)(e / C), c = (int)(e - (rg_i64)j * C);
    const float* xs = x + n * (size_t)t.H * (size_t)t.W * (size_t)C;
    float r[V];
    cell_value<V>(t, xt, in_lds, p0, xs, C, i, j, c, skipna != 0, min_valid, r);
    float* o = out + rg_index(n, i, j, c, t.Ho, t.Wo, C);
    if (V == RG_VEC) *reinterpret_cast<float4*>(o) = make_float4(r[0], r[1 % V], r[2 % V], r[3 % V]);
    else o[0] = r[0];
}

// grid: x = output row, y = sample.  part_s [N][C][H'][6], part_c [N][C][H'][2]
__global__ void __launch_bounds__(RG_THREADS) regrid_cons_rows_kernel(const RegridTables t, const float* __restrict__ x,
                                                                      const float* __restrict__ ref, float* __restrict__ resid, int C,
                                                                      int skipna, double min_valid, double* __restrict__ part_s,
                                                                      rg_i64* __restrict__ part_c) {
    __shared__ XTable xt;
    __shared__ RgCons red[RG_THREADS];
    const int i = blockIdx.x;
    const size_t n = blockIdx.y;
    bool in_lds;
    const int p0 = stage_x(t, 0, t.Wo, xt, &in_lds);
    const float* xs = x + n * (size_t)t.H * (size_t)t.W * (size_t)C;
    const double ayv = t.ay[i];
    for (int c = 0; c < C; ++c) {
        RgCons acc;
        rg_cons_zero(&acc);
        for (int j = threadIdx.x; j < t.Wo; j += RG_THREADS) {
            float r;
            cell_value<1>(t, xt, in_lds, p0, xs, C, i, j, c, skipna != 0, min_valid, &r);
            const size_t o = rg_index(n, i, j, c, t.Ho, t.Wo, C);
            const float d = rg_cons_cell(&acc, r, ref[o], rg_area(ayv, t.ax[j]));
            if (resid) resid[o] = d;
        }
        red[threadIdx.x] = acc;
        __syncthreads();
        for (int o = RG_THREADS / 2; o > 0; o >>= 1) {
            if ((int)threadIdx.x < o) rg_cons_join(&red[threadIdx.x], &red[threadIdx.x + o]);
            __syncthreads();
        }
        if (threadIdx.x == 0) {
            double* ps = part_s + rg_partial_index(n, c, i, C, t.Ho, RG_NSUM);
            rg_i64* pc = part_c + rg_partial_index(n, c, i, C, t.Ho, RG_NCOUNT);
            for (int k = 0; k < RG_NSUM; ++k) ps[k] = red[0].s[k];
            for (int k = 0; k < RG_NCOUNT; ++k) pc[k] = red[0].c[k];
        }
        __syncthreads();
    }
}

// one thread per (n, c): the rows in ascending i'
__global__ void __launch_bounds__(RG_THREADS) regrid_cons_finish_kernel(const double* __restrict__ part_s, const rg_i64* __restrict__ part_c,
                                                                        size_t fields, int Ho, double* __restrict__ sums,
                                                                        rg_i64* __restrict__ counts) {
    const size_t f = (size_t)blockIdx.x * RG_THREADS + threadIdx.x;
    if (f >= fields) return;
    RgCons acc;
    rg_cons_zero(&acc);
    for (int i = 0; i < Ho; ++i) {
        RgCons r;
        for (int k = 0; k < RG_NSUM; ++k) r.s[k] = part_s[(f * (size_t)Ho + (size_t)i) * RG_NSUM + k];
        for (int k = 0; k < RG_NCOUNT; ++k) r.c[k] = part_c[(f * (size_t)Ho + (size_t)i) * RG_NCOUNT + k];
        rg_cons_join(&acc, &r);
    }
    for (int k = 0; k < RG_NSUM; ++k) sums[f * RG_NSUM + k] = acc.s[k];
    for (int k = 0; k < RG_NCOUNT; ++k) counts[f * RG_NCOUNT + k] = acc.c[k];
}

constexpr int MAX_GRID_Y = 65535;

}  // namespace

struct RegridPlan {
    RegridTables t{};
    void* mem = nullptr;           // one allocation behind every table
    size_t nnz_y = 0, nnz_x = 0;
};

static void check_axis(const char* axis, const int* ptr, const int* idx, const double* w, int src, int dst) {
    DL4DS_REQUIRE(ptr && ptr[0] == 0, std::string("regrid_plan_create: the ") + axis + " table's ptr must start at 0");
    for (int d = 0; d < dst; ++d)
        DL4DS_REQUIRE(ptr[d + 1] >= ptr[d], std::string("regrid_plan_create: the ") + axis + " table's ptr must not decrease");
    const int nnz = ptr[dst];
    DL4DS_REQUIRE(nnz == 0 || (idx && w), std::string("regrid_plan_create: the ") + axis + " table has taps but no idx / w");
    for (int k = 0; k < nnz; ++k) {
        DL4DS_REQUIRE(idx[k] >= 0 && idx[k] < src, std::string("regrid_plan_create: a source index of the ") + axis + " table is out of range");
        DL4DS_REQUIRE(w[k] >= 0.0 && w[k] <= 1.7976931348623157e308, std::string("regrid_plan_create: a weight of the ") + axis +
                                                                         " table is negative or not finite");
    }
}

// Everything is validated before the first allocation; the tables go up in one synchronous copy.
RegridPlan* regrid_plan_create(hipStream_t s, int H, int W, int Ho, int Wo, const int* yptr, const int* yidx, const double* yw,
                               const int* xptr, const int* xidx, const double* xw, const double* ay, const double* ax) {
    DL4DS_REQUIRE(H >= 1 && W >= 1 && Ho >= 1 && Wo >= 1, "regrid_plan_create: every extent must be at least 1");
    DL4DS_REQUIRE(rg_sizes_ok(H, W) && rg_sizes_ok(Ho, Wo), "regrid_plan_create: H*W and H'*W' must stay below 2^31");
    DL4DS_REQUIRE(ay && ax, "regrid_plan_create: null destination cell measures");
    check_axis("y", yptr, yidx, yw, H, Ho);
    check_axis("x", xptr, xidx, xw, W, Wo);
    for (int i = 0; i < Ho; ++i) DL4DS_REQUIRE(ay[i] >= 0.0 && ay[i] <= 1.7976931348623157e308, "regrid_plan_create: a cell measure of ay is negative or not finite");
    for (int j = 0; j < Wo; ++j) DL4DS_REQUIRE(ax[j] >= 0.0 && ax[j] <= 1.7976931348623157e308, "regrid_plan_create: a cell measure of ax is negative or not finite");
    const size_t ny = (size_t)yptr[Ho], nx = (size_t)xptr[Wo];
    // doubles first (8-byte aligned), then the ints
    const size_t nd = ny + nx + (size_t)Ho + (size_t)Wo, ni = (size_t)Ho + 1 + (size_t)Wo + 1 + ny + nx;
    std::vector<char> host(nd * sizeof(double) + ni * sizeof(int));
    double* hd = reinterpret_cast<double*>(host.data());
    int* hi = reinterpret_cast<int*>(host.data() + nd * sizeof(double));
    std::copy(yw, yw + ny, hd);
    std::copy(xw, xw + nx, hd + ny);
    std::copy(ay, ay + Ho, hd + ny + nx);
    std::copy(ax, ax + Wo, hd + ny + nx + Ho);
    std::copy(yptr, yptr + Ho + 1, hi);
    std::copy(xptr, xptr + Wo + 1, hi + Ho + 1);
    std::copy(yidx, yidx + ny, hi + Ho + 1 + Wo + 1);
    std::copy(xidx, xidx + nx, hi + Ho + 1 + Wo + 1 + ny);
    RegridPlan* p = new RegridPlan;
    if (hipMalloc(&p->mem, host.size()) != hipSuccess) {
        (void)hipGetLastError();
        delete p;
        throw Dl4dsError("regrid_plan_create: out of device memory for the tables");
    }
    try {
        HIP_CHECK(hipMemcpyAsync(p->mem, host.data(), host.size(), hipMemcpyHostToDevice, s));
        HIP_CHECK(hipStreamSynchronize(s));
    } catch (...) {
        (void)hipFree(p->mem);
        delete p;
        throw;
    }
    const double* dd = reinterpret_cast<const double*>(p->mem);
    const int* di = reinterpret_cast<const int*>(reinterpret_cast<const char*>(p->mem) + nd * sizeof(double));
    RegridTables& t = p->t;
    t.yw = dd; t.xw = dd + ny; t.ay = dd + ny + nx; t.ax = dd + ny + nx + Ho;
    t.yptr = di; t.xptr = di + Ho + 1; t.yidx = di + Ho + 1 + Wo + 1; t.xidx = di + Ho + 1 + Wo + 1 + ny;
    t.H = H; t.W = W; t.Ho = Ho; t.Wo = Wo;
    p->nnz_y = ny; p->nnz_x = nx;
    return p;
}

void regrid_plan_destroy(hipStream_t s, RegridPlan* p) {
    if (!p) return;
    HIP_CHECK(hipStreamSynchronize(s));                      // (a launch that reads the tables may still be in flight)
    if (p->mem) HIP_CHECK(hipFree(p->mem));
    delete p;
}

void regrid_check_call(const char* what, const RegridPlan* p, const float* x, int N, int C, double min_valid) {
    DL4DS_REQUIRE(p, std::string(what) + ": null or destroyed plan");
    DL4DS_REQUIRE(x, std::string(what) + ": null input pointer");
    DL4DS_REQUIRE(N >= 1 && C >= 1, std::string(what) + ": N and C must be at least 1");
    DL4DS_REQUIRE(min_valid >= 0.0 && min_valid <= 1.0, std::string(what) + ": min_valid must lie in [0, 1]");
    DL4DS_REQUIRE((rg_i64)p->t.W * C < RG_CELL_BOUND && (rg_i64)p->t.Wo * C < RG_CELL_BOUND, std::string(what) + ": a row of more than 2^31 floats");
}

size_t regrid_consistency_workspace_bytes(const RegridPlan* p, int N, int C) {
    return (size_t)N * C * p->t.Ho * (RG_NSUM * sizeof(double) + RG_NCOUNT * sizeof(rg_i64));
}

// Everything is checked by the caller (capi.cpp: dl4ds_regrid_apply).
void regrid_apply(hipStream_t s, const RegridPlan* p, const float* x, int N, int C, bool skipna, double min_valid, float* out) {
    const RegridTables& t = p->t;
    const bool vec = rg_vec_ok(C, (uintptr_t)x, (uintptr_t)out);
    const int V = vec ? RG_VEC : 1;
    const rg_i64 blocks = (rg_i64)rg_row_blocks((rg_i64)t.Wo * C, V) * t.Ho;
    DL4DS_REQUIRE(blocks < RG_CELL_BOUND, "regrid_apply: too many workgroups per sample");
    const double bytes = 4.0 * N * C * ((double)t.H * t.W + (double)t.Ho * t.Wo);
    ProfScope ps(s, vec ? "regrid_apply_v4" : "regrid_apply_v1", 0.0, bytes);
    const size_t in_per = (size_t)t.H * t.W * C, out_per = (size_t)t.Ho * t.Wo * C;
    for (int n0 = 0; n0 < N; n0 += MAX_GRID_Y) {             // (samples are independent: the split changes no bit)
        const int nb = std::min(MAX_GRID_Y, N - n0);
        const dim3 grid((unsigned)blocks, nb);
        if (vec) DL4DS_LAUNCH(regrid_apply_kernel<RG_VEC>, grid, dim3(RG_THREADS), 0, s, t, x + n0 * in_per, out + n0 * out_per, C, (int)skipna, min_valid);
        else DL4DS_LAUNCH(regrid_apply_kernel<1>, grid, dim3(RG_THREADS), 0, s, t, x + n0 * in_per, out + n0 * out_per, C, (int)skipna, min_valid);
        HIP_CHECK(hipGetLastError());
    }
}

// Everything is checked by the caller (capi.cpp: dl4ds_regrid_consistency).  ws: regrid_consistency_workspace_bytes.
void regrid_consistency(hipStream_t s, const RegridPlan* p, const float* x, const float* ref, int N, int C, bool skipna, double min_valid,
                        double* sums, long long* counts, float* resid, void* ws) {
    const RegridTables& t = p->t;
    const size_t fields = (size_t)N * C;
    double* part_s = reinterpret_cast<double*>(ws);
    rg_i64* part_c = reinterpret_cast<rg_i64*>(part_s + fields * t.Ho * RG_NSUM);
    const double bytes = 4.0 * N * C * ((double)t.H * t.W + (resid ? 2.0 : 1.0) * (double)t.Ho * t.Wo);
    ProfScope ps(s, "regrid_consistency", 0.0, bytes);
    const size_t in_per = (size_t)t.H * t.W * C, out_per = (size_t)t.Ho * t.Wo * C;
    for (int n0 = 0; n0 < N; n0 += MAX_GRID_Y) {
        const int nb = std::min(MAX_GRID_Y, N - n0);
        DL4DS_LAUNCH(regrid_cons_rows_kernel, dim3(t.Ho, nb), dim3(RG_THREADS), 0, s, t, x + n0 * in_per, ref + n0 * out_per,
                     resid ? resid + n0 * out_per : nullptr, C, (int)skipna, min_valid, part_s + (size_t)n0 * C * t.Ho * RG_NSUM,
                     part_c + (size_t)n0 * C * t.Ho * RG_NCOUNT);
        HIP_CHECK(hipGetLastError());
    }
    DL4DS_LAUNCH(regrid_cons_finish_kernel, dim3((unsigned)((fields + RG_THREADS - 1) / RG_THREADS)), dim3(RG_THREADS), 0, s, part_s, part_c,
                 fields, t.Ho, sums, reinterpret_cast<rg_i64*>(counts));
    HIP_CHECK(hipGetLastError());
}
