// Index arithmetic, tap walk and summation order of the regridding kernels (regrid.hip), compiled twice: by
// hipcc into the kernels and by a plain C++ compiler into tools/regrid_host_check.cpp, which runs the same steps lane by lane on
// the CPU with every array access checked.  The kernels add the launches, the staging of the x-table into LDS and the LDS tree.
//
// Tables.  An axis table is CSR: the taps of destination index d are ptr[d] ... ptr[d + 1] - 1, tap t reads source index idx[t]
// with weight w[t] >= 0 (fp64).  A destination without taps is legal (its outputs are NaN).
//
// The value of one output element (n, i', j', c), rg_walk + rg_finish: the y-taps of i' in table order, inside each of them the
// x-taps of j' in table order, every operation rounded on its own (FMA contraction is off in every function here):
//     w = wy[a] * wx[b];   tot = tot + w
//     skipna and x not finite:  continue
//     num = num + w * (double)x[n, iy[a], ix[b], c];   den = den + w
//     out = (den > 0 and den >= min_valid * tot) ? (float)(num / den) : NaN
// Every NaN that is stored is the canonical quiet NaN 0x7fc00000.
//
// Forms.  A lane owns RG_VEC = 4 consecutive channels of one (i', j') where C is a multiple of 4 and both pointers are 16-byte
// aligned (rg_vec_ok): one 16-byte load per tap, one 16-byte store; otherwise one element, 4-byte accesses.  A workgroup of
// RG_THREADS lanes owns the elements [e0, e0 + RG_THREADS * V) of one output row; the x-taps of the columns it spans
// (rg_block_cols, rg_block_taps) are staged into LDS when they are at most RG_LDS_TAPS and read from the table in global memory
// otherwise (rg_taps_in_lds): the same taps in the same order either way.
//
// Consistency sums (rg_cons_*): per (n, c) six fp64 sums and two counts over the cells (i', j').  ONE order: lane t of the
// RG_THREADS lanes of a row joins its cells j' = t, t + RG_THREADS, ... in ascending j' (rg_cons_cell); the tree
// (rg_cons_tree_partner: o = RG_THREADS / 2 ... 1, lane t < o joins lane t + o) joins the lanes into the row's partial; the rows
// are joined in ascending i', starting from zero (rg_cons_join).  Sums add, max|d| takes the larger, counts add.
#pragma once
#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define RG_HD __host__ __device__ inline
#else
#define RG_HD inline
#endif
#if defined(__clang__)
#define RG_NO_CONTRACT _Pragma("clang fp contract(off)")
#else
#define RG_NO_CONTRACT                                      // (a host build passes -ffp-contract=off)
#endif

// the host program checks every load of x: it defines RG_CHECK_X(pointer, floats) before it includes this file
#ifndef RG_CHECK_X
#define RG_CHECK_X(p, n)
#endif

typedef long long rg_i64;

constexpr int RG_THREADS = 256;                             // lanes of a workgroup, of the apply and of the consistency kernel
constexpr int RG_VEC = 4;                                   // floats of a 16-byte access
constexpr int RG_LDS_TAPS = 2048;                           // x-taps a workgroup stages: 2048 * (4 + 8) B = 24 KiB of LDS
constexpr int RG_NSUM = 6;                                  // sum A, sum A d, sum A d^2, sum A y, sum A r, max |d|
constexpr int RG_NCOUNT = 2;                                // valid cells, cells where exactly one side is finite
constexpr rg_i64 RG_CELL_BOUND = 2147483648ll;              // H*W and H'*W' stay below it

// ---- sizes and forms
RG_HD bool rg_sizes_ok(rg_i64 H, rg_i64 W) { return H >= 1 && W >= 1 && H < RG_CELL_BOUND && W < RG_CELL_BOUND && H * W < RG_CELL_BOUND; }
RG_HD bool rg_vec_ok(int C, uintptr_t x, uintptr_t out) { return C % RG_VEC == 0 && ((x | out) & 15u) == 0; }
// element of the (N, H, W, C) array, 64-bit
RG_HD size_t rg_index(size_t n, int i, int j, int c, int H, int W, int C) {
    return ((n * (size_t)H + (size_t)i) * (size_t)W + (size_t)j) * (size_t)C + (size_t)c;
}
// workgroups along a row of `row` = W' * C floats, V floats per lane
RG_HD int rg_row_blocks(rg_i64 row, int V) { return (int)((row + (rg_i64)RG_THREADS * V - 1) / ((rg_i64)RG_THREADS * V)); }
// the output columns [j0, j1) that workgroup `b` of a row spans
RG_HD void rg_block_cols(int b, int V, int Wo, int C, int* j0, int* j1) {
    const rg_i64 row = (rg_i64)Wo * C, e0 = (rg_i64)b * RG_THREADS * V;
    rg_i64 e1 = e0 + (rg_i64)RG_THREADS * V;
    if (e1 > row) e1 = row;
    *j0 = (int)(e0 / C);
    *j1 = (int)((e1 + C - 1) / C);
}
RG_HD bool rg_taps_in_lds(int taps) { return taps <= RG_LDS_TAPS; }
RG_HD bool rg_finite(float v) {
    union { float f; uint32_t u; } c;
    c.f = v;
    return (c.u & 0x7f800000u) != 0x7f800000u;
}
RG_HD float rg_nan() { return __builtin_nanf(""); }

// ---- the value of an output element
struct RgAcc { double num, den, tot; };
RG_HD void rg_acc_zero(RgAcc* a) { a->num = 0.0; a->den = 0.0; a->tot = 0.0; }
RG_HD void rg_tap(RgAcc* a, double w, float v, bool skipna) {
    RG_NO_CONTRACT
    a->tot = a->tot + w;
    if (skipna && !rg_finite(v)) return;
    const double p = w * (double)v;
    a->num = a->num + p;
    a->den = a->den + w;
}
RG_HD double rg_weight(double wy, double wx) {
    RG_NO_CONTRACT
    return wy * wx;
}
RG_HD float rg_finish(const RgAcc* a, double min_valid) {
    RG_NO_CONTRACT
    const double need = min_valid * a->tot;
    if (a->den > 0.0 && a->den >= need) {
        const double q = a->num / a->den;
        const float r = (float)q;
        return r != r ? rg_nan() : r;                       // ONE NaN: the sign and payload an invalid operation leaves differ by machine
    }
    return rg_nan();
}
// V consecutive channels c ... c + V - 1 of column j', row i' of sample `xs` (H x W x C floats): y-taps [ya, yb) of (iy, wy),
// x-taps [xa, xb) of (ix, wx).  TI / TW: the x-table where the caller keeps it (LDS, global memory, a checked host array).
template <int V, class TI, class TW>
RG_HD void rg_walk(const float* xs, int W, int C, const int* iy, const double* wy, int ya, int yb, TI ix, TW wx, int xa, int xb, int c,
                   bool skipna, RgAcc* acc) {
    for (int k = 0; k < V; ++k) rg_acc_zero(acc + k);
    for (int a = ya; a < yb; ++a) {
        const float* row = xs + (size_t)iy[a] * (size_t)W * (size_t)C;
        const double wa = wy[a];
        for (int b = xa; b < xb; ++b) {
            const double w = rg_weight(wa, wx[b]);
            const float* p = row + (size_t)ix[b] * (size_t)C + (size_t)c;
            RG_CHECK_X(p, V);
            if (V == RG_VEC) {
#if defined(__HIP_DEVICE_COMPILE__)
                const float4 q = *reinterpret_cast<const float4*>(p);
                const float v[4] = {q.x, q.y, q.z, q.w};
#else
                const float v[4] = {p[0], p[1], p[2], p[3]};
#endif
                for (int k = 0; k < V; ++k) rg_tap(acc + k, w, v[k], skipna);
            } else {
                rg_tap(acc, w, p[0], skipna);
            }
        }
    }
}

// ---- the consistency sums
struct RgCons {
    double s[RG_NSUM];
    rg_i64 c[RG_NCOUNT];
};
RG_HD void rg_cons_zero(RgCons* t) {
    for (int k = 0; k < RG_NSUM; ++k) t->s[k] = 0.0;
    for (int k = 0; k < RG_NCOUNT; ++k) t->c[k] = 0;
}
RG_HD double rg_area(double ay, double ax) {
    RG_NO_CONTRACT
    return ay * ax;
}
// what the cell with regridded value r (as stored: fp32), reference y and measure A adds; -> the residual r - y (fp32), NaN where
// the cell is not valid
RG_HD float rg_cons_cell(RgCons* t, float r, float y, double A) {
    RG_NO_CONTRACT
    const bool fr = rg_finite(r), fy = rg_finite(y);
    if (!(fr && fy)) {
        if (fr != fy) t->c[1] += 1;
        return rg_nan();
    }
    const double rd = (double)r, yd = (double)y;
    const double d = rd - yd;
    const double ad = A * d;
    const double d2 = d * d;
    const double ad2 = A * d2;
    const double ay = A * yd;
    const double ar = A * rd;
    const double m = __builtin_fabs(d);
    t->s[0] = t->s[0] + A;
    t->s[1] = t->s[1] + ad;
    t->s[2] = t->s[2] + ad2;
    t->s[3] = t->s[3] + ay;
    t->s[4] = t->s[4] + ar;
    t->s[5] = m > t->s[5] ? m : t->s[5];
    t->c[0] += 1;
    return r - y;
}
RG_HD void rg_cons_join(RgCons* acc, const RgCons* t) {
    RG_NO_CONTRACT
    for (int k = 0; k < RG_NSUM - 1; ++k) acc->s[k] = acc->s[k] + t->s[k];
    acc->s[RG_NSUM - 1] = t->s[RG_NSUM - 1] > acc->s[RG_NSUM - 1] ? t->s[RG_NSUM - 1] : acc->s[RG_NSUM - 1];
    for (int k = 0; k < RG_NCOUNT; ++k) acc->c[k] += t->c[k];
}
// row partials [N][C][H'][RG_NSUM] (fp64) and [N][C][H'][RG_NCOUNT] (int64)
RG_HD size_t rg_partial_index(size_t n, int c, int i, int C, int Ho, int per) {
    return ((n * (size_t)C + (size_t)c) * (size_t)Ho + (size_t)i) * (size_t)per;
}
