// Tiled prediction: the merge of a batch of tile outputs into the output field.
//
// The reference predicts the whole field in one call (inference.py:238, `model.predict(x_test_lr)`); Model.predict_tiled runs the
// network tile by tile on a sibling graph planned for the tile and this kernel stitches the tile outputs on the device:
//   out[s_t][oy_t + y][ox_t + x][c] += wy[ry_t][y] * wx[rx_t][x] * tile[t][y][x][c]       for every tile t of the batch
// tiles [n][th][tw][C], out [N][H][W][C], wy [wy_rows][th], wx [wx_rows][tw] (fp32, device); origin (oy_t, ox_t), sample s_t and the
// table rows (ry_t, rx_t) of each tile are host ints.
//
// SUMMATION ORDER.  An output element is owned by ONE thread per launch: the thread of the lowest-numbered tile of the batch that
// covers it.  The owner loads the stored value once, walks the covering tiles of the batch in ascending tile number, applies one
//   acc = fmaf(w, v, acc),   w = wy * wx rounded to fp32
// per tap and stores once.  Launches are ordered on the library stream, so over a whole plan an element receives its taps in
// ascending tile number whatever the split into batches: the result is bit-for-bit independent of the batch size.  There are no
// floating-point atomics.  A tap whose wy or wx is exactly 0 is SKIPPED, not multiplied: a NaN / inf in a discarded halo never reaches
// the output, and with 0/1 weights ('crop') the stored value is fmaf(1, v, 0) = v (a tile value of -0.0 lands as +0.0 on the zeroed
// output; nothing else changes a bit).
//
// Cost beyond the streaming: per workgroup (one row of one tile) the first wave scans the n tiles of the launch once, 64 per step, and
// leaves those that share the row in LDS; a lane then tests only these (a 2-D plan: the tile's row of the origin grid) for coverage.
// n is limited to 256 per launch (the LDS list); dl4ds_tile_merge enforces it and the caller splits longer batches.
// Memory: streaming; LDS holds the candidate list only.  A workgroup is one row of one tile (blockIdx.y = row, blockIdx.z = tile), so everything that decides
// which tiles cover the row is wave-uniform (scalar registers, scalar branches); lanes run along the row's tw * C floats, 16 bytes per
// lane where tw * C, W * C and every ox * C of the batch are multiples of 4 and the pointers are 16-byte aligned (a 4-float group
// is then wholly inside or outside any tile of the batch), one float per lane otherwise.  One read of the tile batch (less what the
// zero weights skip), one read-modify-write of the covered output.
#include "ops.h"
#include "prof.h"
#include <algorithm>

namespace {

struct MergeParams {
    const float* tiles;
    const float* wy;
    const float* wx;
    float* out;
    const int* oy;          // [n] device copies of the host lists
    const int* ox;
    const int* smp;
    const int* ry;
    const int* rx;
    int n, th, tw, C, H, W;
};

constexpr int MERGE_MAX_TILES = 256;     // tiles per launch: the candidate list of a row lives in LDS (dl4ds_tile_merge enforces it)

template <int V>
__global__ void __launch_bounds__(256) tile_merge_kernel(const MergeParams a) {
    // the tiles of the launch that share this output row with tile t, in ascending tile number: found once per workgroup by its first
    // wave (64 tiles per step, ordered by ballot + popcount), then read from LDS by every lane
    __shared__ int c_j[MERGE_MAX_TILES], c_ox[MERGE_MAX_TILES], c_dy[MERGE_MAX_TILES], c_rx[MERGE_MAX_TILES];
    __shared__ float c_wy[MERGE_MAX_TILES];
    __shared__ int c_n;
    const int t = blockIdx.z, y = blockIdx.y;
    const int row = a.tw * a.C;                    // floats per tile row
    const int oy = a.oy[t], oxc = a.ox[t] * a.C, sm = a.smp[t];
    const int Y = oy + y;                          // output row
    if (threadIdx.x < 64) {                        // (blockDim.x is a multiple of 64: the whole first wave)
        int count = 0;
        for (int base = 0; base < a.n; base += 64) {
            const int j = base + (int)threadIdx.x;
            bool ok = false;
            int dy = 0;
            if (j < a.n) {
                dy = Y - a.oy[j];
                ok = a.smp[j] == sm && (unsigned)dy < (unsigned)a.th;
            }
            const unsigned long long m = __ballot(ok);
            if (ok) {
                const int pos = count + __popcll(m & ((1ull << threadIdx.x) - 1ull));        // < n <= MERGE_MAX_TILES
                c_j[pos] = j; c_ox[pos] = a.ox[j] * a.C; c_dy[pos] = dy; c_rx[pos] = a.rx[j];
                c_wy[pos] = a.wy[(size_t)a.ry[j] * a.th + dy];
            }
            count += __popcll(m);
        }
        if (threadIdx.x == 0) c_n = count;
    }
    __syncthreads();
    const int nc = c_n;
    float* orow = a.out + ((size_t)sm * a.H + Y) * a.W * a.C;
    for (int e = (blockIdx.x * blockDim.x + threadIdx.x) * V; e < row; e += gridDim.x * blockDim.x * V) {
        const int E = oxc + e;                     // float offset in the output row
        float acc[V];
        bool owned = true, loaded = false;
        for (int k = 0; k < nc; ++k) {
            const int d = E - c_ox[k];             // float offset in that tile's row
            if ((unsigned)d >= (unsigned)row) continue;
            const int j = c_j[k];
            if (j < t) { owned = false; break; }   // a lower-numbered tile covers this element: its thread owns it (no tap applied yet:
                                                   // the list is ascending)
            const float wyv = c_wy[k];
            if (wyv == 0.f) continue;
            const float* wxr = a.wx + (size_t)c_rx[k] * a.tw;
            float wxv[V];
            bool any = false;
#pragma unroll
            for (int i = 0; i < V; ++i) {
                wxv[i] = wxr[a.C == 1 ? d + i : (d + i) / a.C];
                any = any || wxv[i] != 0.f;
            }
            if (!any) continue;
            if (!loaded) {
                if (V == 4) {
                    const float4 o = *reinterpret_cast<const float4*>(orow + E);
                    acc[0] = o.x; acc[1] = o.y; acc[2 % V] = o.z; acc[3 % V] = o.w;
                } else {
                    acc[0] = orow[E];
                }
                loaded = true;
            }
            const float* tp = a.tiles + ((size_t)j * a.th + c_dy[k]) * row + d;
            float v[V];
            if (V == 4) {
                const float4 q = *reinterpret_cast<const float4*>(tp);
                v[0] = q.x; v[1] = q.y; v[2 % V] = q.z; v[3 % V] = q.w;
            } else {
                v[0] = tp[0];
            }
#pragma unroll
            for (int i = 0; i < V; ++i)
                if (wxv[i] != 0.f) acc[i] = fmaf(__fmul_rn(wyv, wxv[i]), v[i], acc[i]);
        }
        if (!owned || !loaded) continue;           // not this thread's element, or every tap had weight 0: the stored value stays
        if (V == 4) *reinterpret_cast<float4*>(orow + E) = make_float4(acc[0], acc[1], acc[2 % V], acc[3 % V]);
        else orow[E] = acc[0];
    }
}

// ---- field sums of a tensor that exists tile by tile (the mean ChannelAttention2D needs):
//   sums[smp[t]][c] += sum over y, x of wy[ry[t]][y] * wx[rx[t]][x] * tiles[t][y][x][c]         (fp64; 'crop' weights: every pixel once)
// Fixed order, no floating-point atomics: a workgroup sums one (tile, channel) with a fixed stride and a fixed LDS tree into
// partial[t][c]; one workgroup then adds the partials to the sums in ascending t.  The strided channel read touches every line C
// times; the tensor is one layer of one tile batch, small next to the forward pass that produced it.
__global__ void __launch_bounds__(256) tile_pool_kernel(const MergeParams a, double* __restrict__ partial) {
    const int t = blockIdx.y, c = blockIdx.x;
    const float* wyr = a.wy + (size_t)a.ry[t] * a.th;
    const float* wxr = a.wx + (size_t)a.rx[t] * a.tw;
    const float* tp = a.tiles + (size_t)t * a.th * a.tw * a.C + c;
    double acc = 0.0;
    for (int p = threadIdx.x; p < a.th * a.tw; p += 256) {
        const int y = p / a.tw, x = p - y * a.tw;
        const float w = __fmul_rn(wyr[y], wxr[x]);
        if (w != 0.f) acc += (double)w * (double)tp[(size_t)p * a.C];
    }
    __shared__ double red[256];
    red[threadIdx.x] = acc;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
        __syncthreads();
    }
    if (threadIdx.x == 0) partial[(size_t)t * a.C + c] = red[0];
}

__global__ void __launch_bounds__(256) tile_pool_finish_kernel(const double* __restrict__ partial, const int* __restrict__ smp,
                                                               double* __restrict__ sums, int n, int C) {
    for (int c = threadIdx.x; c < C; c += 256)
        for (int t = 0; t < n; ++t) sums[(size_t)smp[t] * C + c] += partial[(size_t)t * C + c];
}

}  // namespace

// partial: [n][C] doubles of scratch.  Checked by the caller (capi.cpp: dl4ds_tile_pool).
void tile_pool(hipStream_t s, const float* tiles, const float* wy, const float* wx, const int* smp, const int* ry, const int* rx,
               int n, int th, int tw, int C, double* partial, double* sums) {
    MergeParams a{};
    a.tiles = tiles; a.wy = wy; a.wx = wx; a.smp = smp; a.ry = ry; a.rx = rx; a.n = n; a.th = th; a.tw = tw; a.C = C;
    ProfScope ps(s, "tile_pool", 0.0, 4.0 * n * (double)th * tw * C);
    DL4DS_LAUNCH(tile_pool_kernel, dim3(C, n), dim3(256), 0, s, a, partial);
    HIP_CHECK(hipGetLastError());
    DL4DS_LAUNCH(tile_pool_finish_kernel, dim3(1), dim3(256), 0, s, partial, smp, sums, n, C);
    HIP_CHECK(hipGetLastError());
}

// Everything is checked by the caller (capi.cpp: dl4ds_tile_merge); `vec`: the 16-byte form is legal for this batch.
void tile_merge(hipStream_t s, const float* tiles, const float* wy, const float* wx, float* out, const int* oy, const int* ox,
                const int* smp, const int* ry, const int* rx, int n, int th, int tw, int C, int H, int W, bool vec) {
    DL4DS_REQUIRE(n <= MERGE_MAX_TILES, "tile_merge: more tiles than the kernel's candidate list holds");
    MergeParams a;
    a.tiles = tiles; a.wy = wy; a.wx = wx; a.out = out; a.oy = oy; a.ox = ox; a.smp = smp; a.ry = ry; a.rx = rx;
    a.n = n; a.th = th; a.tw = tw; a.C = C; a.H = H; a.W = W;
    const int lanes = cdiv(tw * C, vec ? 4 : 1);
    const int threads = std::min(256, cdiv(lanes, 64) * 64);
    const dim3 grid(std::min(cdiv(lanes, threads), 1024), th, n);
    const double bytes = 4.0 * n * (double)th * tw * C;
    ProfScope ps(s, vec ? "tile_merge_v4" : "tile_merge_v1", 2.0 * bytes / 4.0, 3.0 * bytes);
    if (vec) DL4DS_LAUNCH(tile_merge_kernel<4>, grid, dim3(threads), 0, s, a);
    else DL4DS_LAUNCH(tile_merge_kernel<1>, grid, dim3(threads), 0, s, a);
    HIP_CHECK(hipGetLastError());
}
