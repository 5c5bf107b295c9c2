// Index arithmetic and parent walks of the object labelling (objects.hip), compiled twice: by hipcc into the
// kernels and by a plain C++ compiler into tools/objects_host_check.cpp, which runs the same steps cell by cell on the CPU with
// every array access checked.  Everything that computes a cell index or follows `parent` is here; the kernels add the launches,
// the wave ballots and the atomics on the output tables.
//
// Geometry.  A field is H x W cells, cell (i, j) at index i*W + j < 2^31 - 1.  A UNIT is one row segment of 64 columns (one wave):
// unit u = i * segments(W) + s holds the cells (i, 64 s + lane), so units in ascending order hold the cells in raster order.
// parent[idx] is -1 for a background cell and otherwise the index of an event cell of the same object with parent[idx] <= idx:
// the links form a forest whose roots (parent[idx] == idx) end up as the smallest index of each object, its `first` cell.
//
// Termination.  Every walk moves to a strictly smaller index or stops, so `find` takes at most H*W steps and a `unite` -- whose
// every round either ends or replaces one of its two indices by a smaller one -- at most 2 H*W steps in all.  Each loop carries
// that bound as an explicit budget; a value outside [0, H*W) read from `parent` ends the walk as well.  Both report failure
// instead of going on, and a correct labelling never reaches either.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define OC_HD __host__ __device__ inline
#else
#define OC_HD inline
#endif

typedef long long oc_i64;

// the host program checks every access the walks make: it defines OC_CHECK_ACCESS(pointer) before it includes this file
#ifndef OC_CHECK_ACCESS
#define OC_CHECK_ACCESS(p)
#endif

constexpr int OC_SEG = 64;                                  // columns of a unit: one wave

// ---- cells, units, the strided input
OC_HD int oc_cell(int i, int j, int W) { return i * W + j; }
OC_HD int oc_segments(int W) { return (W + OC_SEG - 1) / OC_SEG; }
OC_HD oc_i64 oc_units(int H, int W) { return (oc_i64)H * oc_segments(W); }
OC_HD void oc_unit_pos(oc_i64 u, int W, int* i, int* j0) {
    const int ns = oc_segments(W);
    *i = (int)(u / ns);
    *j0 = (int)(u % ns) * OC_SEG;
}
// element of the (N, H, W, C) array that holds cell (i, j) of field f = n*C + c
OC_HD size_t oc_x_index(size_t f, int i, int j, int H, int W, int C) {
    const size_t n = f / (size_t)C, c = f % (size_t)C;
    return ((n * (size_t)H + (size_t)i) * (size_t)W + (size_t)j) * (size_t)C + c;
}
// index of the neighbour (i + di, j + dj), or -1 beyond the edge of the field (fields do not wrap)
OC_HD int oc_neighbour(int i, int j, int H, int W, int di, int dj) {
    const int a = i + di, b = j + dj;
    return (a < 0 || a >= H || b < 0 || b >= W) ? -1 : oc_cell(a, b, W);
}

// ---- values
OC_HD uint32_t oc_bits(float v) { union { float f; uint32_t u; } c; c.f = v; return c.u; }
OC_HD float oc_float(uint32_t b) { union { float f; uint32_t u; } c; c.u = b; return c.f; }
OC_HD bool oc_finite(float v) { return (oc_bits(v) & 0x7f800000u) != 0x7f800000u; }
// an event cell: valid (finite) and at or above a finite threshold, compared on float32 (-0.0 >= 0.0 holds)
OC_HD bool oc_event(float v, float thr) { return oc_finite(v) && oc_finite(thr) && v >= thr; }
// total order of float32 as unsigned integers, +0.0 above -0.0; every finite value and both infinities map above 0
OC_HD uint32_t oc_key(float v) {
    const uint32_t b = oc_bits(v);
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
OC_HD float oc_unkey(uint32_t k) { return oc_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k); }

// ---- runs of consecutive event lanes in a unit's 64-bit event mask
OC_HD int oc_ctz64(uint64_t m) { return m ? __builtin_ctzll(m) : 64; }
OC_HD int oc_clz64(uint64_t m) { return m ? __builtin_clzll(m) : 64; }
// cells of lane's run from `lane` to its end, `lane` included (lane is set in mask)
OC_HD int oc_run_len(uint64_t mask, int lane) { return oc_ctz64(~(mask >> lane)); }
// first lane of lane's run (lane is set in mask)
OC_HD int oc_run_first(uint64_t mask, int lane) {
    const uint64_t below = lane ? (~mask) << (64 - lane) : 0;          // lanes lane-1 ... 0 that are NOT events, from the top bit down
    const int ones = oc_clz64(below);                                  // consecutive events just below lane (64: all of them)
    return ones >= lane ? 0 : lane - ones;
}
// exact integer sums of the run of `len` cells (i, j ... j + len - 1): area, sum i, sum j, sum ii, sum jj, sum ij
OC_HD void oc_run_sums(int i, int j, int len, oc_i64 out[6]) {
    const oc_i64 n = len, a = j, I = i;
    const oc_i64 s1 = n * (n - 1) / 2, s2 = (n - 1) * n * (2 * n - 1) / 6;                 // sum k, sum k^2 for k < n <= 64
    const oc_i64 sj = n * a + s1;
    // sum (a + k)^2 = n a^2 + 2 a s1 + s2: every term is positive and part of the sum itself, which the size rules keep below 2^62
    out[0] = n; out[1] = n * I; out[2] = sj; out[3] = n * I * I; out[4] = n * a * a + 2 * a * s1 + s2; out[5] = I * sj;
}

// ---- the two wrappers around what is atomic on the device and a plain operation on the host
OC_HD int oc_load(const int* p) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#else
    OC_CHECK_ACCESS(p);
    return *p;
#endif
}
// *p = min(*p, v) -> the value before
OC_HD int oc_fetch_min(int* p, int v) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __hip_atomic_fetch_min(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#else
    OC_CHECK_ACCESS(p);
    const int old = *p;
    if (v < old) *p = v;
    return old;
#endif
}

// ---- walks.  `budget` is the number of steps left; a walk that runs out of it, or reads an index outside [0, cells), returns -1.
OC_HD int oc_find(const int* parent, int cells, int x, oc_i64* budget) {
    while (true) {
        if (x < 0 || x >= cells || *budget <= 0) return -1;
        --*budget;
        const int p = oc_load(parent + x);
        if (p == x) return x;
        if (p > x) return -1;                                           // links only ever point downwards
        x = p;
    }
}
// lock-free union towards the smaller index: find both roots; while they differ hang the larger below the smaller with a
// fetch-min; if the larger was no root any more, go on from what it pointed to.  -> false when the budget ran out.
OC_HD bool oc_unite(int* parent, int cells, int a, int b, oc_i64* budget) {
    while (true) {
        a = oc_find(parent, cells, a, budget);
        b = oc_find(parent, cells, b, budget);
        if (a < 0 || b < 0) return false;
        if (a == b) return true;
        if (a > b) { const int t = a; a = b; b = t; }                    // a < b
        const int old = oc_fetch_min(parent + b, a);
        if (old == b) return true;
        if (old < 0 || old > b) return false;
        b = old;                                                        // old < b: the pair got smaller
    }
}
OC_HD oc_i64 oc_find_budget(int cells) { return (oc_i64)cells + 2; }
OC_HD oc_i64 oc_unite_budget(int cells) { return 2 * (oc_i64)cells + 8; }

// ---- the steps per cell
// init: the cell's first link, to the first cell of its run inside its unit (mask: the unit's event mask)
OC_HD int oc_init_parent(uint64_t mask, int lane, int i, int j0, int W) {
    return ((mask >> lane) & 1) ? oc_cell(i, j0 + oc_run_first(mask, lane), W) : -1;
}
// merge: the unions event cell (i, j) owes, one per pair of its run and a run that touches it from the left or from above:
//   left   across a unit boundary (inside a unit `init` has linked the run already);
//   up     where this run or the run above begins (left neighbour or upper-left neighbour no event);
//   upper-left / upper-right (connectivity 2) at this run's first / last cell, where the cell above is no event -- if it is one,
//   it belongs to the same upper run and `up` has made the union.
// -> false when a walk gave up.
OC_HD bool oc_merge_cell(int* parent, int H, int W, int connectivity, int i, int j) {
    const int cells = H * W, idx = oc_cell(i, j, W);
    if (oc_load(parent + idx) < 0) return true;
    const int l = oc_neighbour(i, j, H, W, 0, -1), u = oc_neighbour(i, j, H, W, -1, 0);
    const bool L = l >= 0 && oc_load(parent + l) >= 0, U = u >= 0 && oc_load(parent + u) >= 0;
    bool ok = true;
    if (L && (j % OC_SEG) == 0) { oc_i64 b = oc_unite_budget(cells); ok = oc_unite(parent, cells, idx, l, &b) && ok; }
    const int ul = oc_neighbour(i, j, H, W, -1, -1);
    const bool UL = ul >= 0 && oc_load(parent + ul) >= 0;
    if (U && (!L || !UL)) { oc_i64 b = oc_unite_budget(cells); ok = oc_unite(parent, cells, idx, u, &b) && ok; }
    if (connectivity == 2 && !U) {
        if (UL && !L) { oc_i64 b = oc_unite_budget(cells); ok = oc_unite(parent, cells, idx, ul, &b) && ok; }
        const int r = oc_neighbour(i, j, H, W, 0, 1), ur = oc_neighbour(i, j, H, W, -1, 1);
        const bool R = r >= 0 && oc_load(parent + r) >= 0, UR = ur >= 0 && oc_load(parent + ur) >= 0;
        if (UR && !R) { oc_i64 b = oc_unite_budget(cells); ok = oc_unite(parent, cells, idx, ur, &b) && ok; }
    }
    return ok;
}
// flatten: the root of cell idx (-1: background), -2 when the walk gave up
OC_HD int oc_root(const int* parent, int cells, int idx) {
    if (oc_load(parent + idx) < 0) return -1;
    oc_i64 b = oc_find_budget(cells);
    const int r = oc_find(parent, cells, idx, &b);
    return r < 0 ? -2 : r;
}
// gather: the label of a cell whose flattened parent is `root`; 0 for background, -1 for a root outside the field
OC_HD int oc_label(const int* rootlabel, int cells, int root) {
    if (root < 0) return 0;
    if (root >= cells) return -1;
    OC_CHECK_ACCESS(rootlabel + root);
    return rootlabel[root];
}
// row of label `lab` in tables of `cap` rows per field, or -1 when the object is left out
OC_HD oc_i64 oc_table_row(size_t f, int lab, int cap) { return (lab >= 1 && lab <= cap) ? (oc_i64)(f * (size_t)cap + (size_t)(lab - 1)) : -1; }
