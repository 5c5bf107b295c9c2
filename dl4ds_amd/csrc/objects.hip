// Object labelling of the N*C fields (planes) of an (N, H, W, C) array: connected components of the cells at or above a per-field
// threshold, numbered in raster order of their first cell, with per-object sums.
//
// A cell is VALID iff finite, an EVENT iff valid and x >= thr on float32 with a finite thr (-0.0 >= 0.0 holds).  Connectivity 1
// (4 neighbours) or 2 (8 neighbours); fields do not wrap.  labels: 0 background, 1 ... count in raster order of each object's
// first cell = scipy.ndimage.label's numbering.  Tables of cap rows per field, rows count ... cap zero, objects beyond cap left out.
//
// Plain launches on one stream, no workgroup ever waits for another, every loop has a bound taken from the field size.  All index
// arithmetic and every walk over `parent` is objects_core.h's, which a host program runs cell by cell with checked accesses
// (tools/objects_host_check.cpp).  One wave per UNIT, a row segment of 64 columns; per chunk of fields:
//   init     parent = first cell of the cell's run inside its unit (one ballot), -1 for background; per unit nvalid and the three
//            field sums by a fixed shuffle tree.
//   merge    objects_core.h's oc_merge_cell: lock-free minimum-index unions, one per pair of touching runs.
//   flatten  parent = root; per unit the number of roots (ballot + popcount).
//   field    one workgroup per field: the unit sums in a fixed order -> nvalid, field_sums; the exclusive scan of the root
//            counts -> the first label of each unit, count.
//   number   rootlabel[root] = the unit's base + the root's rank in the unit + 1.
//   gather   labels = rootlabel[parent]; per run of consecutive event lanes one set of atomics on the table rows: closed-form
//            integer sums (64-bit adds), bbox (32-bit min / max), vmax (max of the ordered key), the three fp64 masses (a fixed
//            segmented shuffle tree inside the run, then an fp64 atomic add); `first` is written by the root cell.
//   finish   decodes vmax, zeroes the rows from count on.
// What is reproducible: labels, every integer output and vmax are pure functions of the input; field_sums have one summation
// order and give the same bits every call; the masses are sums of exact fp64 terms whose order across runs is the order in which
// the atomics arrive: they may differ in the last bits between calls, within gamma_(n-1) * sum |term| of the exact sum.
// The workspace is 8 B per cell (parent, rootlabel) and 32 B per unit; fields go through in chunks sized by a fixed budget.
#include "objects_core.h"
#include "ops.h"
#include "prof.h"
#include "runtime.h"
#include <algorithm>
#include <climits>

namespace {

constexpr int OBJ_THREADS = 256, OBJ_WAVES = OBJ_THREADS / 64;
constexpr size_t OBJ_WS_BUDGET = size_t(128) << 20;       // workspace of one chunk of fields
constexpr long long OBJ_MAX_CHUNK_UNITS = 1ll << 30;      // units of one launch: the grid stays below 2^31 blocks

__device__ __forceinline__ void raise(unsigned* err) {
    __hip_atomic_fetch_or(err, (unsigned)DEV_ERR_OBJECTS_WALK, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}

// the unit of this wave: field of the chunk, row, first column; false beyond the chunk's last unit (wave-uniform)
struct Unit { size_t fl; oc_i64 u; int i, j0; };
__device__ __forceinline__ bool this_unit(oc_i64 units, oc_i64 total, int W, Unit& t) {
    const oc_i64 gid = (oc_i64)blockIdx.x * OBJ_WAVES + (threadIdx.x >> 6);
    if (gid >= total) return false;
    t.fl = (size_t)(gid / units);
    t.u = gid % units;
    oc_unit_pos(t.u, W, &t.i, &t.j0);
    return true;
}

__global__ void __launch_bounds__(OBJ_THREADS) obj_init_kernel(const float* __restrict__ x, const float* __restrict__ thr, int H,
                                                               int W, int C, size_t field0, oc_i64 units, oc_i64 total,
                                                               int* __restrict__ parent, double* __restrict__ usum,
                                                               int* __restrict__ uvalid) {
    Unit t;
    if (!this_unit(units, total, W, t)) return;
    const int lane = threadIdx.x & 63, j = t.j0 + lane;
    const bool in = j < W;
    const size_t f = field0 + t.fl;
    const float v = x[oc_x_index(f, t.i, in ? j : t.j0, H, W, C)];
    const bool valid = in && oc_finite(v), ev = in && oc_event(v, thr[f]);
    const uint64_t mask = __ballot(ev);
    if (in) parent[t.fl * ((size_t)H * W) + oc_cell(t.i, j, W)] = oc_init_parent(mask, lane, t.i, t.j0, W);
    const double d = valid ? (double)v : 0.0;
    const double s0 = wave_sum(d), s1 = wave_sum(d * (double)t.i), s2 = wave_sum(d * (double)j);
    const int nv = __popcll(__ballot(valid));
    if (lane == 0) {
        const size_t o = t.fl * (size_t)units + (size_t)t.u;
        usum[3 * o] = s0; usum[3 * o + 1] = s1; usum[3 * o + 2] = s2;
        uvalid[o] = nv;
    }
}

__global__ void __launch_bounds__(OBJ_THREADS) obj_merge_kernel(int H, int W, int connectivity, oc_i64 units, oc_i64 total,
                                                                int* parent, unsigned* err) {
    Unit t;
    if (!this_unit(units, total, W, t)) return;
    const int j = t.j0 + (int)(threadIdx.x & 63);
    if (j < W && !oc_merge_cell(parent + t.fl * ((size_t)H * W), H, W, connectivity, t.i, j)) raise(err);
}

__global__ void __launch_bounds__(OBJ_THREADS) obj_flatten_kernel(int H, int W, oc_i64 units, oc_i64 total, int* parent,
                                                                  int* __restrict__ ucount, unsigned* err) {
    Unit t;
    if (!this_unit(units, total, W, t)) return;
    const int lane = threadIdx.x & 63, j = t.j0 + lane, cells = H * W;
    const bool in = j < W;
    int* pf = parent + t.fl * (size_t)cells;
    const int idx = oc_cell(t.i, in ? j : t.j0, W);
    const int r = in ? oc_root(pf, cells, idx) : -1;
    if (r == -2) raise(err);
    if (r >= 0) pf[idx] = r;
    const int n = __popcll(__ballot(r == idx));
    if (lane == 0) ucount[t.fl * (size_t)units + (size_t)t.u] = n;
}

// One workgroup per field of the chunk.  Thread t sums the units t, t + 256, ... in ascending order, a fixed tree joins the 256
// partial sums: one summation order, whatever the launch.  Then the root counts become exclusive prefixes, 256 units at a time.
__global__ void __launch_bounds__(OBJ_THREADS) obj_field_kernel(oc_i64 units, size_t field0, const double* __restrict__ usum,
                                                                const int* __restrict__ uvalid, int* __restrict__ ucount,
                                                                int* __restrict__ count, long long* __restrict__ nvalid,
                                                                double* __restrict__ field_sums) {
    __shared__ double sd[3][OBJ_THREADS];
    __shared__ long long sv[OBJ_THREADS];
    __shared__ int sc[2][OBJ_THREADS];
    const int t = threadIdx.x;
    const size_t fl = blockIdx.x, f = field0 + fl, base = fl * (size_t)units;
    double a0 = 0, a1 = 0, a2 = 0;
    long long nv = 0;
    for (oc_i64 u = t; u < units; u += OBJ_THREADS) {
        const size_t o = base + (size_t)u;
        a0 += usum[3 * o]; a1 += usum[3 * o + 1]; a2 += usum[3 * o + 2];
        nv += uvalid[o];
    }
    sd[0][t] = a0; sd[1][t] = a1; sd[2][t] = a2; sv[t] = nv;
    __syncthreads();
    for (int o = OBJ_THREADS / 2; o > 0; o >>= 1) {
        if (t < o) { sd[0][t] += sd[0][t + o]; sd[1][t] += sd[1][t + o]; sd[2][t] += sd[2][t + o]; sv[t] += sv[t + o]; }
        __syncthreads();
    }
    if (t == 0) {
        if (nvalid) nvalid[f] = sv[0];
        if (field_sums) { field_sums[3 * f] = sd[0][0]; field_sums[3 * f + 1] = sd[1][0]; field_sums[3 * f + 2] = sd[2][0]; }
    }
    int running = 0;
    for (oc_i64 u0 = 0; u0 < units; u0 += OBJ_THREADS) {
        const bool there = u0 + t < units;
        const int c = there ? ucount[base + (size_t)(u0 + t)] : 0;
        int cur = 0;
        sc[0][t] = c;
        __syncthreads();
        for (int o = 1; o < OBJ_THREADS; o <<= 1) {                      // inclusive scan, ping-pong between the two rows
            const int v = sc[cur][t] + (t >= o ? sc[cur][t - o] : 0);
            sc[cur ^ 1][t] = v;
            cur ^= 1;
            __syncthreads();
        }
        if (there) ucount[base + (size_t)(u0 + t)] = running + sc[cur][t] - c;
        running += sc[cur][OBJ_THREADS - 1];
        __syncthreads();
    }
    if (t == 0) count[f] = running;
}

__global__ void __launch_bounds__(OBJ_THREADS) obj_number_kernel(int H, int W, oc_i64 units, oc_i64 total,
                                                                 const int* __restrict__ parent, const int* __restrict__ ucount,
                                                                 int* __restrict__ rootlabel) {
    Unit t;
    if (!this_unit(units, total, W, t)) return;
    const int lane = threadIdx.x & 63, j = t.j0 + lane;
    const bool in = j < W;
    const size_t off = t.fl * ((size_t)H * W);
    const int idx = oc_cell(t.i, in ? j : t.j0, W);
    const bool root = in && parent[off + idx] == idx;
    const uint64_t m = __ballot(root);
    if (root) rootlabel[off + idx] = ucount[t.fl * (size_t)units + (size_t)t.u] + __popcll(m & ((1ull << lane) - 1ull)) + 1;
}

__global__ void __launch_bounds__(OBJ_THREADS) obj_gather_kernel(const float* __restrict__ x, int H, int W, int C, size_t field0,
                                                                 oc_i64 units, oc_i64 total, const int* __restrict__ parent,
                                                                 const int* __restrict__ rootlabel, int cap, int* __restrict__ labels,
                                                                 unsigned long long* __restrict__ sums, int* __restrict__ bbox,
                                                                 int* __restrict__ first, unsigned* __restrict__ vkey,
                                                                 double* __restrict__ mass, unsigned* err) {
    Unit t;
    if (!this_unit(units, total, W, t)) return;
    const int lane = threadIdx.x & 63, j = t.j0 + lane, cells = H * W;
    const bool in = j < W;
    const size_t f = field0 + t.fl, off = t.fl * (size_t)cells;
    const int idx = oc_cell(t.i, in ? j : t.j0, W);
    const int root = in ? parent[off + idx] : -1;
    int lab = oc_label(rootlabel + off, cells, root);
    if (lab < 0) { raise(err); lab = 0; }
    if (labels && in) labels[f * (size_t)cells + idx] = lab;
    if (cap == 0) return;                                                // (uniform)
    const float v = x[oc_x_index(f, t.i, in ? j : t.j0, H, W, C)];
    const bool ev = lab > 0;
    const uint64_t mask = __ballot(ev);
    const int len = ev ? oc_run_len(mask, lane) : 1;
    const int end = lane + len - 1;
    double m0 = ev ? (double)v : 0.0, m1 = m0 * (double)t.i, m2 = m0 * (double)j;       // exact products: |i|, |j| < 2^29
    unsigned key = ev ? oc_key(v) : 0u;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {                                   // suffix sums inside the run: lane l gets lanes l ... end
        const double t0 = __shfl_down(m0, o, 64), t1 = __shfl_down(m1, o, 64), t2 = __shfl_down(m2, o, 64);
        const unsigned tk = __shfl_down(key, o, 64);
        if (lane + o <= end) { m0 += t0; m1 += t1; m2 += t2; key = max(key, tk); }
    }
    const oc_i64 row = oc_table_row(f, lab, cap);
    if (row < 0) return;
    if (root == idx) first[row] = idx;
    if (oc_run_first(mask, lane) != lane) return;                        // one lane per run goes on
    oc_i64 s[6];
    oc_run_sums(t.i, j, len, s);
#pragma unroll
    for (int k = 0; k < 6; ++k) atomicAdd(sums + 6 * row + k, (unsigned long long)s[k]);
    atomicMin(bbox + 4 * row, t.i);
    atomicMax(bbox + 4 * row + 1, t.i);
    atomicMin(bbox + 4 * row + 2, j);
    atomicMax(bbox + 4 * row + 3, j + len - 1);
    atomicMax(vkey + row, key);
    atomicAdd(mass + 3 * row, m0);
    atomicAdd(mass + 3 * row + 1, m1);
    atomicAdd(mass + 3 * row + 2, m2);
}

// before gather: the bbox rows of the chunk's fields start at (max, min, max, min) so that the atomic min / max find them
__global__ void __launch_bounds__(OBJ_THREADS) obj_preset_kernel(size_t rows, int* __restrict__ bbox) {
    const size_t r = (size_t)blockIdx.x * OBJ_THREADS + threadIdx.x;
    if (r >= rows) return;
    bbox[4 * r] = INT_MAX; bbox[4 * r + 1] = INT_MIN; bbox[4 * r + 2] = INT_MAX; bbox[4 * r + 3] = INT_MIN;
}
// after gather: vmax from its key; the rows from count on are zero
__global__ void __launch_bounds__(OBJ_THREADS) obj_finish_kernel(size_t fields, int cap, const int* __restrict__ count,
                                                                 int* __restrict__ bbox, unsigned* __restrict__ vkey) {
    const size_t r = (size_t)blockIdx.x * OBJ_THREADS + threadIdx.x;
    if (r >= fields * (size_t)cap) return;
    const size_t f = r / (size_t)cap;
    if ((int)(r % (size_t)cap) < count[f]) {
        vkey[r] = oc_bits(oc_unkey(vkey[r]));
    } else {
        vkey[r] = 0u;
        bbox[4 * r] = 0; bbox[4 * r + 1] = 0; bbox[4 * r + 2] = 0; bbox[4 * r + 3] = 0;
    }
}

// SAL's thresholds: the largest key of a field's finite cells (0: none) ...
__global__ void __launch_bounds__(OBJ_THREADS) obj_maxkey_kernel(const float* __restrict__ x, int H, int W, int C, size_t field0,
                                                                 oc_i64 units, oc_i64 total, unsigned* __restrict__ keys) {
    Unit t;
    if (!this_unit(units, total, W, t)) return;
    const int lane = threadIdx.x & 63, j = t.j0 + lane;
    const bool in = j < W;
    const size_t f = field0 + t.fl;
    const float v = x[oc_x_index(f, t.i, in ? j : t.j0, H, W, C)];
    unsigned key = (in && oc_finite(v)) ? oc_key(v) : 0u;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) key = max(key, (unsigned)__shfl_down(key, o, 64));
    if (lane == 0 && key) atomicMax(keys + f, key);
}
// ... and thr = float32(factor * max), the product in fp64 and rounded once; 0 without a finite cell or a finite product
__global__ void __launch_bounds__(OBJ_THREADS) obj_threshold_kernel(size_t fields, double factor, const unsigned* __restrict__ keys,
                                                                    float* __restrict__ thr) {
    const size_t f = (size_t)blockIdx.x * OBJ_THREADS + threadIdx.x;
    if (f >= fields) return;
    float t = 0.f;
    if (keys[f]) {
        t = (float)(factor * (double)oc_unkey(keys[f]));
        if (!oc_finite(t)) t = 0.f;
    }
    thr[f] = t;
}

struct ObjPlan {
    size_t cells, units, fields;                                         // per field; fields of one chunk
    size_t bytes() const { return fields * (units * 32 + cells * 8); }
};
ObjPlan plan(size_t fields, int H, int W) {
    ObjPlan p;
    p.cells = (size_t)H * W;
    p.units = (size_t)oc_units(H, W);
    const size_t per = p.units * 32 + p.cells * 8;
    p.fields = std::max<size_t>(1, std::min({fields, OBJ_WS_BUDGET / per, (size_t)OBJ_MAX_CHUNK_UNITS / p.units}));
    return p;
}
void check_sizes(const char* who, int N, int H, int W, int C) {
    const std::string w(who);
    DL4DS_REQUIRE(N >= 1 && H >= 1 && W >= 1 && C >= 1, w + ": expected N, H, W, C >= 1");
    const unsigned __int128 cells = (unsigned __int128)H * (unsigned)W, side = (unsigned)std::max(H, W);
    DL4DS_REQUIRE(cells < (((unsigned __int128)1 << 31) - 1), w + ": H*W must stay below 2^31 - 1");
    DL4DS_REQUIRE(side < ((unsigned __int128)1 << 29), w + ": max(H, W) must stay below 2^29");
    DL4DS_REQUIRE(cells * side * side < ((unsigned __int128)1 << 62), w + ": H*W*max(H, W)^2 must stay below 2^62");
}
unsigned grid_for(size_t n, size_t per_block) { return (unsigned)((n + per_block - 1) / per_block); }

}  // namespace

size_t objects_workspace_bytes(int N, int H, int W, int C) {
    if (N <= 0 || H <= 0 || W <= 0 || C <= 0) return 0;
    return plan((size_t)N * C, H, W).bytes();
}

void objects_check_args(const float* x, int N, int H, int W, int C, const float* thr, int connectivity, int cap, const int* count,
                        const long long* sums, const int* bbox, const int* first, const float* vmax, const double* mass) {
    check_sizes("label_objects", N, H, W, C);
    DL4DS_REQUIRE(connectivity == 1 || connectivity == 2, "label_objects: connectivity must be 1 (4 neighbours) or 2 (8 neighbours)");
    DL4DS_REQUIRE(cap >= 0, "label_objects: cap must not be negative");
    DL4DS_REQUIRE(x && thr && count, "label_objects: the array, the thresholds and count are needed");
    DL4DS_REQUIRE(cap == 0 || (sums && bbox && first && vmax && mass), "label_objects: cap > 0 needs all five tables");
}

void label_objects(hipStream_t st, const float* x, int N, int H, int W, int C, const float* thr, int connectivity, int cap, int* labels,
                   int* count, long long* nvalid, double* field_sums, long long* sums, int* bbox, int* first, float* vmax,
                   double* mass, void* workspace, size_t workspace_bytes, unsigned* err) {
    objects_check_args(x, N, H, W, C, thr, connectivity, cap, count, sums, bbox, first, vmax, mass);
    const size_t F = (size_t)N * C;
    const ObjPlan pl = plan(F, H, W);
    DL4DS_REQUIRE(workspace && workspace_bytes >= pl.bytes() && err, "label_objects workspace too small");
    double* usum = static_cast<double*>(workspace);                      // [fields][units][3]
    int* parent = reinterpret_cast<int*>(usum + pl.fields * pl.units * 3);
    int* rootlabel = parent + pl.fields * pl.cells;
    int* ucount = rootlabel + pl.fields * pl.cells;                      // [fields][units]
    int* uvalid = ucount + pl.fields * pl.units;
    unsigned* vkey = reinterpret_cast<unsigned*>(vmax);
    // (profiler tags objects_init ... objects_finish: kernel time per step, bytes = the step's algorithmic traffic)
#define OBJ_STEP(tag, bytes, ...)                                  \
    do {                                                           \
        ProfScope ps(st, "objects_" tag, 0.0, (double)(bytes));    \
        DL4DS_LAUNCH(__VA_ARGS__);                                 \
    } while (0)
    if (cap > 0) {
        const size_t rows = F * (size_t)cap;
        HIP_CHECK(hipMemsetAsync(sums, 0, rows * 6 * sizeof(long long), st));
        HIP_CHECK(hipMemsetAsync(first, 0, rows * sizeof(int), st));
        HIP_CHECK(hipMemsetAsync(vmax, 0, rows * sizeof(float), st));
        HIP_CHECK(hipMemsetAsync(mass, 0, rows * 3 * sizeof(double), st));
        OBJ_STEP("finish", rows * 16, obj_preset_kernel, dim3(grid_for(rows, OBJ_THREADS)), dim3(OBJ_THREADS), 0, st, rows, bbox);
    }
    const oc_i64 units = (oc_i64)pl.units;
    for (size_t f0 = 0; f0 < F; f0 += pl.fields) {
        const size_t fc = std::min(pl.fields, F - f0);
        const oc_i64 total = (oc_i64)fc * units;
        const size_t nc = fc * pl.cells, nu = fc * pl.units;
        const dim3 grid(grid_for((size_t)total, OBJ_WAVES)), block(OBJ_THREADS);
        OBJ_STEP("init", nc * 8 + nu * 28, obj_init_kernel, grid, block, 0, st, x, thr, H, W, C, f0, units, total, parent, usum, uvalid);
        OBJ_STEP("merge", nc * 4, obj_merge_kernel, grid, block, 0, st, H, W, connectivity, units, total, parent, err);
        OBJ_STEP("flatten", nc * 8 + nu * 4, obj_flatten_kernel, grid, block, 0, st, H, W, units, total, parent, ucount, err);
        OBJ_STEP("field", nu * 36, obj_field_kernel, dim3((unsigned)fc), block, 0, st, units, f0, (const double*)usum,
                 (const int*)uvalid, ucount, count, nvalid, field_sums);
        OBJ_STEP("number", nc * 4 + nu * 4, obj_number_kernel, grid, block, 0, st, H, W, units, total, (const int*)parent,
                 (const int*)ucount, rootlabel);
        if (labels || cap > 0)
            OBJ_STEP("gather", nc * (4 + (cap > 0 ? 4 : 0) + (labels ? 4 : 0)), obj_gather_kernel, grid, block, 0, st, x, H, W, C, f0,
                     units, total, (const int*)parent, (const int*)rootlabel, cap, labels,
                     reinterpret_cast<unsigned long long*>(sums), bbox, first, vkey, mass, err);
    }
    if (cap > 0)
        OBJ_STEP("finish", F * (size_t)cap * 24, obj_finish_kernel, dim3(grid_for(F * (size_t)cap, OBJ_THREADS)), dim3(OBJ_THREADS), 0,
                 st, F, cap, (const int*)count, bbox, vkey);
#undef OBJ_STEP
    HIP_CHECK(hipGetLastError());
}

size_t object_thresholds_workspace_bytes(int N, int H, int W, int C) {
    if (N <= 0 || H <= 0 || W <= 0 || C <= 0) return 0;
    return (size_t)N * C * sizeof(unsigned);
}

void object_thresholds(hipStream_t st, const float* x, int N, int H, int W, int C, double factor, float* thr, void* workspace,
                       size_t workspace_bytes) {
    check_sizes("object_thresholds", N, H, W, C);
    DL4DS_REQUIRE(x && thr, "object_thresholds: the array and the thresholds are needed");
    DL4DS_REQUIRE(factor > 0 && factor <= 1.7976931348623157e308, "object_thresholds: factor must be positive and finite");
    const size_t F = (size_t)N * C;
    DL4DS_REQUIRE(workspace && workspace_bytes >= F * sizeof(unsigned), "object_thresholds workspace too small");
    unsigned* keys = static_cast<unsigned*>(workspace);
    HIP_CHECK(hipMemsetAsync(keys, 0, F * sizeof(unsigned), st));
    const oc_i64 units = oc_units(H, W);
    const size_t chunk = std::max<size_t>(1, std::min(F, (size_t)(OBJ_MAX_CHUNK_UNITS / units)));
    for (size_t f0 = 0; f0 < F; f0 += chunk) {
        const oc_i64 total = (oc_i64)std::min(chunk, F - f0) * units;
        DL4DS_LAUNCH(obj_maxkey_kernel, dim3(grid_for((size_t)total, OBJ_WAVES)), dim3(OBJ_THREADS), 0, st, x, H, W, C, f0, units,
                     total, keys);
    }
    DL4DS_LAUNCH(obj_threshold_kernel, dim3(grid_for(F, OBJ_THREADS)), dim3(OBJ_THREADS), 0, st, F, factor, (const unsigned*)keys, thr);
    HIP_CHECK(hipGetLastError());
}
