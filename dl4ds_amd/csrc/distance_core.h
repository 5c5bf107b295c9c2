// Index arithmetic, distances, early-exit conditions and score terms of the distance-map verification (distance.hip; DESIGN.md
// section 29), compiled twice: by hipcc into the kernels and by a plain C++ compiler into tools/distance_host_check.cpp, which runs
// the same steps cell by cell on the CPU with every array access checked.  The kernels add the launches, the staging of a row into
// LDS, the wave shuffles and the final tree.
//
// Geometry.  A field is H x W cells with (H-1)^2 + (W-1)^2 < 2^31 - 1 and H*W < 2^31: every squared distance between two cells is an
// int32 below DC_DIST_EMPTY, the value a distance to an EMPTY set takes.  The exact Euclidean distance transform is separable:
//   column pass  g(i, j)  = the vertical distance from (i, j) to the nearest event of column j, DC_G_NONE when the column has none;
//   row pass     D(i, j)  = min over k of (j - k)^2 + g(i, k)^2.
// The row pass sees the row of g^2 one SEGMENT of at most DC_SEG_MAX columns at a time (the LDS stage of the kernel).
//
// Termination.  dc_row_scan walks the offsets o = o0, o0 + 1, ... of one segment [a, b) and ends after at most b - a of them: the
// loop counts them.  It stops earlier once o^2 + (the smallest g^2 of the segment) >= best: every term still to come is at least
// that large, so the stop is exact.  The column pass is two loops over the H rows, the segment walk one loop over the segments.
//
// Term arithmetic.  Every fp64 term is built from sqrt, +, -, *, /, min and abs, one operation per statement, in functions that
// switch FMA contraction off: a term has the bits numpy gives for the same expression.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define DC_HD __host__ __device__ inline
#else
#define DC_HD inline
#endif
#if defined(__clang__)
#define DC_NO_CONTRACT _Pragma("clang fp contract(off)")
#else
#define DC_NO_CONTRACT                                      // (a host build passes -ffp-contract=off)
#endif

typedef long long dc_i64;

// the host program checks every access the scans make: it defines DC_CHECK_ACCESS(pointer) before it includes this file
#ifndef DC_CHECK_ACCESS
#define DC_CHECK_ACCESS(p)
#endif

constexpr int DC_DIST_EMPTY = 2147483647;                   // d^2 to an empty set; reads as +inf
constexpr int DC_G_NONE = 2147483647;                       // a column without an event
constexpr int DC_TG = 8;                                    // thresholds per group: one read of y and p serves them all
constexpr int DC_SEG_MAX = 1024;                            // columns of a segment: 2 sides x 4 B x 1024 = 8 KiB of LDS per wave
constexpr int DC_NCOUNT = 8;                                // n_valid, n_A, n_B, n_AB, max_d2_AB, max_d2_BA, sum_d2_AB, sum_d2_BA
constexpr int DC_NSUM = 7;                                  // sum_d_AB, sum_d_BA, pratt_AB, pratt_BA, bad1, bad2, badmax

// ---- sizes, the strided input, the workspace
DC_HD bool dc_sizes_ok(dc_i64 H, dc_i64 W) {
    if (H < 1 || W < 1 || H > 2147483647ll || W > 2147483647ll) return false;
    const unsigned long long a = (unsigned long long)(H - 1), b = (unsigned long long)(W - 1);
    return a * a + b * b < 2147483647ull && (unsigned long long)H * (unsigned long long)W < 2147483648ull;
}
// element of the (N, H, W, C) array that holds cell (i, j) of field f = n*C + c
DC_HD size_t dc_x_index(size_t f, int i, int j, int H, int W, int C) {
    const size_t n = f / (size_t)C, c = f % (size_t)C;
    return ((n * (size_t)H + (size_t)i) * (size_t)W + (size_t)j) * (size_t)C + c;
}
// g[field of the chunk][threshold of the group][side][H][W]; side 0 is the observation (A), side 1 the prediction (B)
DC_HD size_t dc_g_index(size_t fl, int tcount, int k, int side, int H, int W, int i, int j) {
    return ((((fl * (size_t)tcount + (size_t)k) * 2 + (size_t)side) * (size_t)H + (size_t)i) * (size_t)W) + (size_t)j;
}
// row partials [field of the chunk][threshold of the group][H][DC_NCOUNT or DC_NSUM]
DC_HD size_t dc_partial_index(size_t fl, int tcount, int k, int H, int i, int n) {
    return ((fl * (size_t)tcount + (size_t)k) * (size_t)H + (size_t)i) * (size_t)n;
}
// outputs [F][T][...]
DC_HD size_t dc_out_index(size_t f, int T, int t) { return f * (size_t)T + (size_t)t; }

// ---- values
DC_HD uint32_t dc_bits(float v) { union { float f; uint32_t u; } c; c.f = v; return c.u; }
DC_HD bool dc_finite(float v) { return (dc_bits(v) & 0x7f800000u) != 0x7f800000u; }
DC_HD bool dc_valid(float y, float p) { return dc_finite(y) && dc_finite(p); }
// an event: a valid cell at or above the threshold, compared on float32 (-0.0 >= 0.0 holds)
DC_HD bool dc_event(bool valid, float v, float thr) { return valid && v >= thr; }

// ---- the column pass
// rows since the last event of the column, walking away from it: 0 on an event, DC_G_NONE before the first one
DC_HD int dc_col_step(int since, bool event) { return event ? 0 : (since == DC_G_NONE ? DC_G_NONE : since + 1); }
DC_HD int dc_col_join(int down, int up) { return down < up ? down : up; }
// g is stored in 16 bits: the size rule gives H <= 46341, so g <= H - 1 < 0xffff
DC_HD uint16_t dc_g_pack(int g) { return g == DC_G_NONE ? (uint16_t)0xffffu : (uint16_t)g; }
DC_HD int dc_g_unpack(uint16_t v) { return v == 0xffffu ? DC_G_NONE : (int)v; }
DC_HD int dc_g2(int g) { return g == DC_G_NONE ? DC_DIST_EMPTY : g * g; }              // g <= H - 1: g^2 < 2^31 - 1

// ---- the row pass
// o^2 + g^2 of one candidate: below 2^31 - 1 for a real one by the size rule; DC_DIST_EMPTY when the column has no event
DC_HD int dc_term(unsigned o2, int g2) {
    const unsigned s = o2 + (unsigned)g2;                                              // < 2^32: both are below 2^31
    return s < (unsigned)DC_DIST_EMPTY ? (int)s : DC_DIST_EMPTY;
}
DC_HD int dc_segments(int W, int seg) { return (W + seg - 1) / seg; }
// smallest |j - k| over the columns k of [a, b)
DC_HD int dc_seg_offset(int j, int a, int b) { return j < a ? a - j : (j >= b ? j - (b - 1) : 0); }
// can a segment at offset o0 still lower `best`?
DC_HD bool dc_seg_needed(int o0, int best) { return (unsigned)o0 * (unsigned)o0 < (unsigned)best; }
// the s-th segment to visit from the segment `own`: own, own - 1, own + 1, own - 2, ... (may lie outside [0, segments))
DC_HD int dc_seg_visit(int own, int step) { return (step & 1) ? own - (step + 1) / 2 : own + step / 2; }
DC_HD int dc_load(const int* p) {
    DC_CHECK_ACCESS(p);
    return *p;
}
// min(best, min over the columns k of [a, b) of (j - k)^2 + g2[k - a]); segmin = the smallest g2 of the segment
DC_HD int dc_row_scan(const int* g2, int a, int b, int segmin, int j, int best) {
    if (segmin == DC_DIST_EMPTY) return best;
    int o = dc_seg_offset(j, a, b);
    for (int n = a; n < b; ++n, ++o) {                                                 // at most b - a offsets reach into [a, b)
        const unsigned o2 = (unsigned)o * (unsigned)o;
        if (dc_term(o2, segmin) >= best) break;                                        // every term from here on is at least that
        const int l = j - o, r = j + o;
        const bool left = l >= a && l < b, right = o > 0 && r >= a && r < b;
        if (left) { const int t = dc_term(o2, dc_load(g2 + (l - a))); best = t < best ? t : best; }
        if (right) { const int t = dc_term(o2, dc_load(g2 + (r - a))); best = t < best ? t : best; }
        if (l < a && r >= b) break;
    }
    return best;
}

// ---- the score terms of one cell
DC_HD double dc_inf() { return __builtin_inf(); }
DC_HD double dc_dist(int d2) { return d2 == DC_DIST_EMPTY ? dc_inf() : __builtin_sqrt((double)d2); }
DC_HD double dc_d2f(int d2) { return d2 == DC_DIST_EMPTY ? dc_inf() : (double)d2; }
DC_HD double dc_min(double a, double b) { return a < b ? a : b; }
DC_HD double dc_add(double a, double b) {
    DC_NO_CONTRACT
    return a + b;
}
// NaN from either side stays
DC_HD double dc_max(double a, double b) { return (b > a || b != b) ? b : a; }
// 1 / (1 + alpha * d2)
DC_HD double dc_pratt(double alpha, int d2) {
    DC_NO_CONTRACT
    const double m = alpha * dc_d2f(d2);
    const double s = 1.0 + m;
    return 1.0 / s;
}
// | min(d(x, A), c) - min(d(x, B), c) |
DC_HD double dc_baddeley(int d2a, int d2b, double cutoff) {
    DC_NO_CONTRACT
    const double a = dc_min(dc_dist(d2a), cutoff), b = dc_min(dc_dist(d2b), cutoff);
    const double d = a - b;
    return __builtin_fabs(d);
}
DC_HD double dc_square(double w) {
    DC_NO_CONTRACT
    return w * w;
}

struct DcTerms {
    dc_i64 c[DC_NCOUNT];
    double s[DC_NSUM];
};
DC_HD void dc_zero(DcTerms* t) {
    for (int k = 0; k < DC_NCOUNT; ++k) t->c[k] = 0;
    for (int k = 0; k < DC_NSUM; ++k) t->s[k] = 0.0;
}
// what cell x with d2a = d^2(x, A), d2b = d^2(x, B) adds; an invalid cell adds nothing (it is never an event either)
DC_HD void dc_cell_terms(bool valid, int d2a, int d2b, double cutoff, double alpha, DcTerms* t) {
    dc_zero(t);
    if (!valid) return;
    const bool in_a = d2a == 0, in_b = d2b == 0;
    t->c[0] = 1; t->c[1] = in_a; t->c[2] = in_b; t->c[3] = in_a && in_b;
    if (in_a) { t->c[4] = d2b; t->c[6] = d2b; t->s[0] = dc_dist(d2b); t->s[2] = dc_pratt(alpha, d2b); }
    if (in_b) { t->c[5] = d2a; t->c[7] = d2a; t->s[1] = dc_dist(d2a); t->s[3] = dc_pratt(alpha, d2a); }
    const double w = dc_baddeley(d2a, d2b, cutoff);
    t->s[4] = w; t->s[5] = dc_square(w); t->s[6] = w;
}
// the two ways partial results join: counts 4 and 5 and sum 6 are maxima, everything else is a sum
DC_HD dc_i64 dc_join_count(int k, dc_i64 a, dc_i64 b) { return (k == 4 || k == 5) ? (a > b ? a : b) : a + b; }
DC_HD double dc_join_sum(int k, double a, double b) { return k == 6 ? dc_max(a, b) : dc_add(a, b); }
DC_HD void dc_join(DcTerms* acc, const DcTerms* t) {
    for (int k = 0; k < DC_NCOUNT; ++k) acc->c[k] = dc_join_count(k, acc->c[k], t->c[k]);
    for (int k = 0; k < DC_NSUM; ++k) acc->s[k] = dc_join_sum(k, acc->s[k], t->s[k]);
}
