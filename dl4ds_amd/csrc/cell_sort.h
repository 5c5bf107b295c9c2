// The per-cell sorted-series engine of qmap.hip (quantile_table) and extremes.hip (lmoments), DESIGN.md section 10a: the finite
// values of +x or -x of every grid cell along the time axis, as ascending keys.  Sample n of cell c lives at x[n*stride + c],
// stride >= per; an element that is not finite gets the key SORT_INVALID, which sorts last, so a cell's valid count is the lower
// bound of SORT_INVALID in its sorted keys.  Two engines, one host driver (cell_sort); a client keeps only its consumer:
//  * N <= SORT_STRIDED_MAX: the client's kernel for the row length P, a workgroup of CELL_THREADS on G consecutive cells, calls
//    sorted_cell_rows: sample k of the G cells is loaded by adjacent lanes into LDS rows of pitch P + 1 (the lane that owns a row
//    then walks it at bank (g*(P+1) + j) % 32: conflict-free), and the bitonic network sorts the G rows.  G is twice
//    distribution.hip's, whose network sorts two sides.
//  * longer: the 64 x 64 transposing gather writes the keys contiguous per cell into the workspace, the key-only radix sort sorts
//    them, and the client's finish launch reads the chunk's sorted keys.  Cells go through in chunks sized by the workspace budget.
#pragma once
#include "sort_keys.h"
#include <string>
#include <type_traits>

namespace {

constexpr int CELL_TR = 64;                            // gather and finish kernels: 64 cells x 64 samples per transposed tile
constexpr int CELL_THREADS = 512;                      // LDS engine: threads per workgroup

__device__ __forceinline__ uint32_t cell_key(float v, bool neg) {
    v = neg ? -v : v;
    return finite_bits(v) ? rank_key(v) : SORT_INVALID;
}

template <int P>
constexpr int cell_group() { return 2 * (4096 / P > 16 ? 4096 / P : 16); }
template <int P>
constexpr size_t cell_lds_bytes() { return (size_t)cell_group<P>() * (P + 1) * 4; }

// strided LDS engine: sample k of the workgroup's `cells` <= G cells from cell c0 on, N <= P samples each, is loaded into
// key[g*(P + 1) + k] and the G rows are sorted; rows beyond `cells` and samples beyond N are SORT_INVALID.  key: the workgroup's
// dynamic LDS, cell_lds_bytes<P>()
template <int P>
__device__ __forceinline__ void sorted_cell_rows(const float* __restrict__ x, size_t N, size_t stride, bool neg, size_t c0, int cells,
                                                 uint32_t* key) {
    constexpr int T = CELL_THREADS, G = cell_group<P>(), PITCH = P + 1;
    for (int i = threadIdx.x; i < G * P; i += T) {                        // sample k of the G cells: adjacent lanes, adjacent floats
        const int k = i / G, g = i % G;
        key[g * PITCH + k] = ((size_t)k < N && g < cells) ? cell_key(x[(size_t)k * stride + c0 + g], neg) : SORT_INVALID;
    }
    __syncthreads();
    bitonic_rows<P, G, PITCH, T, false>(key, nullptr);
}

// global engine, step 1: the keys of a chunk of `ncell` cells (the first at x), contiguous per cell: a tile of 64 cells x 64
// samples is read with lanes along the cells and written with lanes along the samples.  blockIdx.x = cell block * etiles + sample block
__global__ void __launch_bounds__(SORT_THREADS) cell_gather_kernel(const float* __restrict__ x, size_t ncell, size_t N, size_t stride,
                                                                 int neg, unsigned etiles, uint32_t* __restrict__ k) {
    __shared__ uint32_t tk[CELL_TR][CELL_TR + 1];
    const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
    const size_t c0 = (size_t)(blockIdx.x / etiles) * CELL_TR, p0 = (size_t)(blockIdx.x % etiles) * CELL_TR;
    for (int e = ty; e < CELL_TR; e += SORT_WAVES) {
        const size_t cell = c0 + tx, pos = p0 + e;
        tk[e][tx] = (cell < ncell && pos < N) ? cell_key(x[pos * stride + cell], neg) : SORT_INVALID;
    }
    __syncthreads();
    for (int g = ty; g < CELL_TR; g += SORT_WAVES) {
        const size_t cell = c0 + g, pos = p0 + tx;
        if (cell < ncell && pos < N) k[cell * N + pos] = tk[tx][g];
    }
}

// workspace of `segs` cells: their keys, the sort's second buffer, the digit counts per tile
struct CellWorkspace {
    uint32_t *k, *tmp, *hist;
    CellWorkspace(Carver& w, size_t segs, size_t ntiles, size_t L)
        : k(w.take<uint32_t>(segs * L)), tmp(w.take<uint32_t>(segs * L)), hist(w.take<uint32_t>(segs * ntiles * SORT_RADIX)) {}
};

inline size_t cell_sort_workspace_bytes(size_t N, size_t per) {
    return N <= (size_t)SORT_STRIDED_MAX ? 0 : plan_chunks<CellWorkspace>(per, N).bytes();
}

// launches the client's LDS kernel Kern for row length P over `per` cells
template <int P, auto Kern, typename... Args>
void launch_cell_lds(hipStream_t s, size_t per, Args... args) {
    static bool once = false;
    if (!once) {
        HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(Kern), hipFuncAttributeMaxDynamicSharedMemorySize,
                                      (int)cell_lds_bytes<P>()));
        once = true;
    }
    DL4DS_LAUNCH(Kern, dim3((unsigned)cdivz(per, cell_group<P>())), dim3(CELL_THREADS), cell_lds_bytes<P>(), s, args...);
    HIP_CHECK(hipGetLastError());
}

// The host driver of both engines, under the profiler tag name_strided or name_global.  N <= SORT_STRIDED_MAX: lds(P) with P a
// std::integral_constant, the row length for N, launches the client's kernel through launch_cell_lds.  Longer: per chunk the gather
// and the sort, then finish(keys, ncell, cell0) launches the client's kernel over the chunk's sorted keys, cell i of the chunk at
// keys[i*N]; `workspace` holds cell_sort_workspace_bytes(N, per) (the client has checked it).
template <typename Lds, typename Finish>
void cell_sort(hipStream_t s, const char* name, const float* x, size_t N, size_t per, size_t stride, int neg, void* workspace, Lds lds,
               Finish finish) {
    const bool strided = N <= (size_t)SORT_STRIDED_MAX;
    ProfScope ps(s, std::string(name) + (strided ? "_strided" : "_global"), 0.0, 4.0 * (double)N * (double)per);
    if (strided) {
        if (N <= 64) return lds(std::integral_constant<int, 64>());
        if (N <= 128) return lds(std::integral_constant<int, 128>());
        if (N <= 256) return lds(std::integral_constant<int, 256>());
        return lds(std::integral_constant<int, SORT_STRIDED_MAX>());
    }
    const Chunk c = plan_chunks<CellWorkspace>(per, N);
    Carver carver{static_cast<char*>(workspace)};
    const CellWorkspace w(carver, c.segs, c.ntiles, N);
    const unsigned nt = (unsigned)c.ntiles, etiles = (unsigned)cdivz(N, CELL_TR);
    for (size_t c0 = 0; c0 < per; c0 += c.segs) {
        const size_t nc = std::min(c.segs, per - c0);
        const size_t cblocks = cdivz(nc, CELL_TR);
        DL4DS_REQUIRE(cblocks * etiles < (size_t(1) << 31), std::string(name) + ": too many tiles for one launch");
        DL4DS_LAUNCH(cell_gather_kernel, dim3((unsigned)(cblocks * etiles)), dim3(SORT_THREADS), 0, s, x + c0, nc, N, stride, neg, etiles,
                     w.k);
        segmented_sort<false>(s, KeyBuffer{w.k}, w.k, nullptr, w.tmp, nullptr, nc, N, nt, w.hist);
        finish((const uint32_t*)w.k, nc, c0);
    }
    HIP_CHECK(hipGetLastError());
}

}  // namespace
