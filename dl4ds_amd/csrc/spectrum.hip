// Spectral verification of the F = N*C fields of an observation y and a prediction p, both (N, H, W, C) fp32: per field the
// unnormalised two-dimensional DFT of either side in fp64, folded over caller-defined bins of the half plane kx = 0 .. W/2 into
//   power[f][0..3][b] = sum mult |Y|^2, sum mult |P|^2, Re sum mult Y conj(P), Im sum mult Y conj(P)
// (the definitions are in include/dl4ds_hip.h).  A cell is KEPT iff y and p are both finite there; with
// detrend each side loses its own mean over the kept cells; excluded cells are 0; with window the cell (i, j) is multiplied by the
// periodic Hann weights wy[i] * wx[j].  The transform is a direct DFT as two matrix products -- climate grids are rarely powers of
// two -- with twiddle factors from host-made fp64 tables indexed by (k * i) mod n, an exact integer.
//
// Four kernels per call, LDS-tiled fp64 FMA (no MFMA yet, DESIGN.md section 16 "Next"):
//  (a) prepare, one workgroup per field: kept count and both means, per-thread sums over cells t, t + 256, ... then a fixed tree.
//  (b) rows: Z[side][field][y][kx] = sum_j v[y][j] tw_W[(kx j) mod W], a real x complex GEMM over all rows of a chunk of fields.
//      Rows are ordered [sample][y][channel], so a tile's loads walk the contiguous W*C run of a grid row with adjacent lanes on
//      adjacent floats also for C > 1; detrend, zero-fill and window are applied as the values are loaded.
//  (c) columns: X[ky][kx] = sum_y tw_H[(ky y) mod H] Z[y][kx], complex x complex per field with both sides' tiles of one (ky, kx)
//      block in one workgroup; the epilogue forms the four products per coefficient in registers and stores them.  X is not stored.
//  (d) bins: the host sorts the bin map by bin (counting sort, index order within a bin) once per call; one workgroup per
//      (field, bin) gathers its coefficients, per-thread sums over list entries t, t + 256, ... then the same fixed tree.
// No floating-point atomics and no order that depends on the launch: a repeated call gives the same bits, and a field's result does
// not depend on which other fields share the call.  Fields go through in chunks sized by the workspace budget of sort_keys.h.
#include "common.h"
#include "ops.h"
#include "prof.h"
#include "sort_keys.h"
#include <cmath>
#include <vector>

namespace {

constexpr int SP_MAX_DIM = 16384, SP_MAX_BINS = 16384;    // (the C header states both)
constexpr int SP_THREADS = 256;                           // every kernel: 16 x 16 threads in the two GEMMs
constexpr int SP_BK = 16;                                 // K step of both GEMMs: 64-byte runs of a grid row per tile row
constexpr int SP_RM = 128, SP_RN = 64;                    // row transform: tile of 128 rows x 64 kx, 8 x 4 per thread
constexpr int SP_CM = 64, SP_CN = 64;                     // column transform: tile of 64 ky x 64 kx, 4 x 4 per thread and side
constexpr size_t SP_MAX_FIELDS = size_t(1) << 20;         // most fields of a chunk; fields * bins also stays below 2^30 (grid of (d))
constexpr double SP_TWO_PI = 6.283185307179586476925286766559;

struct SpShape { int H, W, C, Wh; };
// samples [n0, n0 + ns) x channels [c0, c0 + nc): whole samples (nc == C), or some channels of one sample when a sample is over budget
struct SpChunk { size_t n0; int ns, c0, nc; };

// ------------------------------------------------------------------------------------------------------------------ (a) prepare
__global__ void __launch_bounds__(SP_THREADS) spec_prepare_kernel(const float* __restrict__ y, const float* __restrict__ p, const SpShape sh,
                                                                 int detrend, long long* __restrict__ valid, double* __restrict__ mean) {
    __shared__ double sy[SP_THREADS], sp[SP_THREADS];
    __shared__ unsigned cnt[SP_THREADS];
    const int t = threadIdx.x;
    const size_t f = blockIdx.x, n = f / (size_t)sh.C, c = f % (size_t)sh.C;
    const size_t cells = (size_t)sh.H * sh.W, base = n * cells * sh.C + c;
    double a = 0.0, b = 0.0;
    unsigned k = 0;
    for (size_t i = t; i < cells; i += SP_THREADS) {
        const float yv = y[base + i * sh.C], pv = p ? p[base + i * sh.C] : 0.f;
        if (finite_bits(yv) && finite_bits(pv)) { a += (double)yv; b += (double)pv; ++k; }
    }
    sy[t] = a; sp[t] = b; cnt[t] = k;
    group_tree<SP_THREADS>(t, [&](int i, int j) { sy[i] += sy[j]; sp[i] += sp[j]; cnt[i] += cnt[j]; });
    if (t == 0) {
        const unsigned nv = cnt[0];
        const bool sub = detrend && nv;
        valid[f] = (long long)nv;
        mean[f * 2] = sub ? sy[0] / (double)nv : 0.0;
        mean[f * 2 + 1] = sub && p ? sp[0] / (double)nv : 0.0;
    }
}

// --------------------------------------------------------------------------------------------------------------------- (b) rows
// Row r of the chunk is (pixel row q = r / nc, channel c0 + r % nc) with q = sample * H + y.  blockIdx = (row tile, kx tile, side).
template <bool C1>
__global__ void __launch_bounds__(SP_THREADS) spec_rows_kernel(const float* __restrict__ y, const float* __restrict__ p, const SpShape sh,
                                                              const SpChunk ch, const double* __restrict__ mean,
                                                              const double2* __restrict__ twx, const double* __restrict__ wx,
                                                              const double* __restrict__ wy, double* __restrict__ Zr,
                                                              double* __restrict__ Zi) {
    __shared__ double As[SP_BK][SP_RM + 1];
    __shared__ double Bc[SP_BK][SP_RN], Bs[SP_BK][SP_RN];
    const int t = threadIdx.x, tx = t & 15, ty = t >> 4;
    const int side = blockIdx.z, H = sh.H, W = sh.W, Wh = sh.Wh;
    const int C = C1 ? 1 : sh.C, nc = C1 ? 1 : ch.nc, c0 = C1 ? 0 : ch.c0;
    const size_t r0 = (size_t)blockIdx.x * SP_RM;
    const int kx0 = blockIdx.y * SP_RN;
    const size_t nq = (size_t)ch.ns * H, rows = nq * nc;
    const size_t qa = r0 / nc, qe = (r0 + SP_RM - 1) / nc, qb = qe < nq ? qe : nq - 1;
    const unsigned span = SP_BK * C;                       // floats of one pixel row that a K step covers
    const size_t total = (qb - qa + 1) * span;
    for (int i = t; i < SP_BK * (SP_RM + 1); i += SP_THREADS) (&As[0][0])[i] = 0.0;   // tile rows past the chunk stay 0
    double accr[8][4] = {}, acci[8][4] = {};
    for (int j0 = 0; j0 < W; j0 += SP_BK) {
        __syncthreads();
        for (size_t idx = t; idx < total; idx += SP_THREADS) {             // adjacent lanes, adjacent floats of a grid row
            const size_t q = qa + idx / span;
            const unsigned e = (unsigned)(idx % span);
            const int jj = C1 ? (int)e : (int)(e / C), c = C1 ? 0 : (int)(e % C), cl = c - c0;
            if (cl < 0 || cl >= nc) continue;
            const size_t r = q * nc + cl;
            if (r < r0 || r >= r0 + SP_RM) continue;
            const int j = j0 + jj;
            double v = 0.0;
            if (j < W) {
                const size_t n = ch.n0 + q / H;
                const int yy = (int)(q % H);
                const size_t o = ((n * H + yy) * W + j) * C + c;
                const float a = y[o], b = p ? p[o] : 0.f;
                if (finite_bits(a) && finite_bits(b))
                    v = ((double)(side ? b : a) - mean[(n * C + c) * 2 + side]) * (wy[yy] * wx[j]);
            }
            As[jj][r - r0] = v;
        }
        for (int idx = t; idx < SP_BK * SP_RN; idx += SP_THREADS) {
            const int kk = idx / SP_RN, col = idx % SP_RN, kx = kx0 + col, j = j0 + kk;
            double cs = 0.0, sn = 0.0;
            if (kx < Wh && j < W) {
                const double2 tw = twx[(unsigned)(kx * j) % (unsigned)W];   // kx * j < 2^28: exact
                cs = tw.x; sn = -tw.y;
            }
            Bc[kk][col] = cs; Bs[kk][col] = sn;
        }
        __syncthreads();
#pragma unroll 4
        for (int kk = 0; kk < SP_BK; ++kk) {
            double a[8], bc[4], bs[4];
#pragma unroll
            for (int i = 0; i < 8; ++i) a[i] = As[kk][ty + 16 * i];
#pragma unroll
            for (int n = 0; n < 4; ++n) { bc[n] = Bc[kk][tx + 16 * n]; bs[n] = Bs[kk][tx + 16 * n]; }
#pragma unroll
            for (int i = 0; i < 8; ++i)
#pragma unroll
                for (int n = 0; n < 4; ++n) {
                    accr[i][n] = fma(a[i], bc[n], accr[i][n]);
                    acci[i][n] = fma(a[i], bs[n], acci[i][n]);
                }
        }
    }
    const size_t nfc = (size_t)ch.ns * nc;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const size_t r = r0 + ty + 16 * i;
        if (r >= rows) continue;
        const size_t q = r / nc, fl = (q / H) * nc + r % nc;
        const size_t base = ((side * nfc + fl) * H + q % H) * Wh;
#pragma unroll
        for (int n = 0; n < 4; ++n) {
            const int kx = kx0 + tx + 16 * n;
            if (kx < Wh) { Zr[base + kx] = accr[i][n]; Zi[base + kx] = acci[i][n]; }
        }
    }
}

// ------------------------------------------------------------------------------------------------------------------ (c) columns
// blockIdx = (field of the chunk, ky tile, kx tile).  T[field][comp][ky * Wh + kx], COMPS = 4 with two sides, 1 with one.
template <int SIDES>
__global__ void __launch_bounds__(SP_THREADS) spec_cols_kernel(const SpShape sh, size_t nfc, const double2* __restrict__ twy,
                                                              const double* __restrict__ Zr, const double* __restrict__ Zi,
                                                              double* __restrict__ T) {
    __shared__ double Ac[SP_BK][SP_CM], As[SP_BK][SP_CM];
    __shared__ double Br[SIDES][SP_BK][SP_CN], Bi[SIDES][SP_BK][SP_CN];
    const int t = threadIdx.x, tx = t & 15, ty = t >> 4;
    const int H = sh.H, Wh = sh.Wh;
    const size_t fl = blockIdx.x;
    const int ky0 = blockIdx.y * SP_CM, kx0 = blockIdx.z * SP_CN;
    double xr[SIDES][4][4] = {}, xi[SIDES][4][4] = {};
    for (int y0 = 0; y0 < H; y0 += SP_BK) {
        __syncthreads();
        for (int idx = t; idx < SP_BK * SP_CM; idx += SP_THREADS) {
            const int kk = idx / SP_CM, row = idx % SP_CM, ky = ky0 + row, yy = y0 + kk;
            double cs = 0.0, sn = 0.0;
            if (ky < H && yy < H) {
                const double2 tw = twy[(unsigned)(ky * yy) % (unsigned)H];
                cs = tw.x; sn = tw.y;
            }
            Ac[kk][row] = cs; As[kk][row] = sn;
        }
#pragma unroll
        for (int s = 0; s < SIDES; ++s)
            for (int idx = t; idx < SP_BK * SP_CN; idx += SP_THREADS) {
                const int kk = idx / SP_CN, col = idx % SP_CN, yy = y0 + kk, kx = kx0 + col;
                double re = 0.0, im = 0.0;
                if (yy < H && kx < Wh) {
                    const size_t o = ((s * nfc + fl) * H + yy) * Wh + kx;
                    re = Zr[o]; im = Zi[o];
                }
                Br[s][kk][col] = re; Bi[s][kk][col] = im;
            }
        __syncthreads();
#pragma unroll 2
        for (int kk = 0; kk < SP_BK; ++kk) {
            double cs[4], sn[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) { cs[i] = Ac[kk][ty + 16 * i]; sn[i] = As[kk][ty + 16 * i]; }
#pragma unroll
            for (int s = 0; s < SIDES; ++s) {
                double zr[4], zi[4];
#pragma unroll
                for (int n = 0; n < 4; ++n) { zr[n] = Br[s][kk][tx + 16 * n]; zi[n] = Bi[s][kk][tx + 16 * n]; }
#pragma unroll
                for (int i = 0; i < 4; ++i)
#pragma unroll
                    for (int n = 0; n < 4; ++n) {                          // (cs - i sn) (zr + i zi)
                        xr[s][i][n] = fma(cs[i], zr[n], fma(sn[i], zi[n], xr[s][i][n]));
                        xi[s][i][n] = fma(cs[i], zi[n], fma(-sn[i], zr[n], xi[s][i][n]));
                    }
            }
        }
    }
    const size_t cells = (size_t)H * Wh;
    double* Tf = T + fl * (SIDES == 2 ? 4 : 1) * cells;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int ky = ky0 + ty + 16 * i;
        if (ky >= H) continue;
#pragma unroll
        for (int n = 0; n < 4; ++n) {
            const int kx = kx0 + tx + 16 * n;
            if (kx >= Wh) continue;
            const size_t o = (size_t)ky * Wh + kx;
            const double yr = xr[0][i][n], yi = xi[0][i][n];
            Tf[o] = fma(yr, yr, yi * yi);                                  // (written as fma: the same rounding in every instance)
            if constexpr (SIDES == 2) {
                const double pr = xr[1][i][n], pi = xi[1][i][n];
                Tf[cells + o] = fma(pr, pr, pi * pi);
                Tf[2 * cells + o] = fma(yr, pr, yi * pi);                  // Y conj(P)
                Tf[3 * cells + o] = fma(yi, pr, -(yr * pi));
            }
        }
    }
}

// --------------------------------------------------------------------------------------------------------------------- (d) bins
// blockIdx.x = field of the chunk * B + bin.  list[off[b] .. off[b + 1]) are the half-plane coefficients of bin b, ascending.
template <int COMPS>
__global__ void __launch_bounds__(SP_THREADS) spec_bins_kernel(const SpShape sh, const SpChunk ch, int B, const int* __restrict__ off,
                                                              const int* __restrict__ list, const double* __restrict__ T,
                                                              double* __restrict__ power) {
    __shared__ double red[COMPS][SP_THREADS];
    const int t = threadIdx.x;
    const size_t fl = blockIdx.x / (unsigned)B;
    const int b = (int)(blockIdx.x % (unsigned)B);
    const size_t cells = (size_t)sh.H * sh.Wh;
    const double* Tf = T + fl * COMPS * cells;
    double acc[COMPS] = {};
    for (int i = off[b] + t; i < off[b + 1]; i += SP_THREADS) {
        const int idx = list[i], kx = idx % sh.Wh;
        const double m = (kx == 0 || 2 * kx == sh.W) ? 1.0 : 2.0;
#pragma unroll
        for (int c = 0; c < COMPS; ++c) acc[c] += m * Tf[c * cells + idx];
    }
#pragma unroll
    for (int c = 0; c < COMPS; ++c) red[c][t] = acc[c];
    group_tree<SP_THREADS>(t, [&](int i, int j) {
#pragma unroll
        for (int c = 0; c < COMPS; ++c) red[c][i] += red[c][j];
    });
    if (t < 4) {
        const size_t f = (ch.n0 + fl / ch.nc) * sh.C + ch.c0 + fl % ch.nc;
        power[(f * 4 + t) * B + b] = t < COMPS ? red[t < COMPS ? t : 0][0] : 0.0;
    }
}

// ------------------------------------------------------------------------------------------------------ workspace and the chunks
struct SpBuffers {                                         // of `fields` fields
    double *zr, *zi, *t;
    SpBuffers(Carver& w, size_t fields, size_t cells, int sides)
        : zr(w.take<double>(fields * sides * cells)), zi(w.take<double>(fields * sides * cells)),
          t(w.take<double>(fields * (sides == 2 ? 4 : 1) * cells)) {}
};

struct SpTables {                                          // of one call
    double2 *twx, *twy;
    double *wx, *wy;
    int *off, *list;
    SpTables(Carver& w, int H, int W, int B, size_t cells)
        : twx(w.take<double2>(W)), twy(w.take<double2>(H)), wx(w.take<double>(W)), wy(w.take<double>(H)), off(w.take<int>(B + 1)),
          list(w.take<int>(cells)) {}
};

struct SpPlan { int ns, nc; size_t buffer_bytes, table_bytes; };

// as many fields per chunk as the budget holds, in whole samples; a sample over the budget goes by channels, a field over it alone
SpPlan sp_plan(int N, int H, int W, int C, int sides, int B) {
    const size_t cells = (size_t)H * (W / 2 + 1);
    const size_t per_field = (size_t)(2 * sides + (sides == 2 ? 4 : 1)) * 8 * cells;
    const size_t room = (SORT_WS_BUDGET - 3 * 256) / per_field;           // (three buffers, each rounded up to 256 bytes)
    const size_t cap = std::max<size_t>(1, std::min({room, SP_MAX_FIELDS, (size_t(1) << 30) / (size_t)B}));
    SpPlan pl;
    if (cap >= (size_t)C) { pl.ns = (int)std::min<size_t>((size_t)N, cap / C); pl.nc = C; }
    else { pl.ns = 1; pl.nc = (int)cap; }
    Carver one{nullptr}, two{nullptr};
    const SpBuffers b(one, (size_t)pl.ns * pl.nc, cells, sides);
    const SpTables tb(two, H, W, B, cells);
    (void)b; (void)tb;
    pl.buffer_bytes = one.used; pl.table_bytes = two.used;
    return pl;
}

void fill_axis(double2* tw, double* win, int n, int window) {
    for (int k = 0; k < n; ++k) {
        const double ang = SP_TWO_PI * (double)k / (double)n;
        tw[k] = double2{std::cos(ang), std::sin(ang)};
        win[k] = window ? 0.5 - 0.5 * std::cos(ang) : 1.0;
    }
}

}  // namespace

void spectrum_check_args(int N, int H, int W, int C, const int* bin_host, int B) {
    DL4DS_REQUIRE(H >= 1 && H <= SP_MAX_DIM && W >= 1 && W <= SP_MAX_DIM, "spectrum: H and W must lie in [1, 16384]");
    DL4DS_REQUIRE(B >= 1 && B <= SP_MAX_BINS, "spectrum: between 1 and 16384 bins are supported");
    DL4DS_REQUIRE(N >= 0 && C >= 0, "spectrum: negative shape");
    DL4DS_REQUIRE((size_t)N * (size_t)C < (size_t(1) << 31), "spectrum: N*C must stay below 2^31");
    DL4DS_REQUIRE(bin_host, "spectrum: bin map missing");
    const size_t cells = (size_t)H * (W / 2 + 1);
    for (size_t i = 0; i < cells; ++i)
        DL4DS_REQUIRE(bin_host[i] >= -1 && bin_host[i] < B, "spectrum: bin map entries must lie in [-1, B)");
}

size_t spectrum_workspace_bytes(int N, int H, int W, int C, int sides, int B) {
    if ((size_t)N * (size_t)C == 0) return 0;
    const SpPlan pl = sp_plan(N, H, W, C, sides, B);
    return pl.buffer_bytes + pl.table_bytes;
}

void spectrum(hipStream_t s, const float* y, const float* p, int N, int H, int W, int C, int detrend, int window, const int* bin_host,
              int B, double* power, long long* valid, double* mean, void* workspace, size_t workspace_bytes) {
    spectrum_check_args(N, H, W, C, bin_host, B);
    const size_t F = (size_t)N * (size_t)C;
    if (F == 0) return;
    DL4DS_REQUIRE(y && power && valid && mean, "spectrum: null array");
    const int sides = p ? 2 : 1, Wh = W / 2 + 1;
    const size_t cells = (size_t)H * Wh;
    const SpPlan pl = sp_plan(N, H, W, C, sides, B);
    DL4DS_REQUIRE(workspace && workspace_bytes >= pl.buffer_bytes + pl.table_bytes, "spectrum workspace too small");
    Carver carver{static_cast<char*>(workspace)};
    const SpBuffers buf(carver, (size_t)pl.ns * pl.nc, cells, sides);
    char* table_base = static_cast<char*>(workspace) + carver.used;
    Carver dev_tables{table_base};
    const SpTables tb(dev_tables, H, W, B, cells);
    {   // the call's tables, laid out on the host as on the device and uploaded in one copy
        std::vector<char> host(pl.table_bytes);
        Carver hc{host.data()};
        const SpTables ht(hc, H, W, B, cells);
        fill_axis(ht.twx, ht.wx, W, window);
        fill_axis(ht.twy, ht.wy, H, window);
        for (int b = 0; b <= B; ++b) ht.off[b] = 0;
        for (size_t i = 0; i < cells; ++i) if (bin_host[i] >= 0) ++ht.off[bin_host[i] + 1];
        for (int b = 0; b < B; ++b) ht.off[b + 1] += ht.off[b];
        std::vector<int> at(ht.off, ht.off + B);
        for (size_t i = 0; i < cells; ++i) if (bin_host[i] >= 0) ht.list[at[bin_host[i]]++] = (int)i;
        HIP_CHECK(hipMemcpyAsync(table_base, host.data(), pl.table_bytes, hipMemcpyHostToDevice, s));
        HIP_CHECK(hipStreamSynchronize(s));                                // `host` goes out of scope
    }
    const SpShape sh{H, W, C, Wh};
    const dim3 block(SP_THREADS);
    {
        ProfScope ps(s, "spectrum_prepare", 0.0, 4.0 * sides * (double)F * H * W);
        DL4DS_LAUNCH(spec_prepare_kernel, dim3((unsigned)F), block, 0, s, y, p, sh, detrend, valid, mean);
    }
    for (size_t n0 = 0; n0 < (size_t)N; n0 += pl.ns) {
        for (int c0 = 0; c0 < C; c0 += pl.nc) {
            const SpChunk ch{n0, (int)std::min<size_t>(pl.ns, (size_t)N - n0), c0, std::min(pl.nc, C - c0)};
            const size_t nfc = (size_t)ch.ns * ch.nc, rows = nfc * H;
            {
                ProfScope ps(s, "spectrum_rows", 4.0 * sides * (double)rows * W * Wh, 16.0 * sides * (double)rows * Wh);
                const dim3 grid((unsigned)cdivz(rows, SP_RM), (unsigned)cdivz(Wh, SP_RN), sides);
                if (C == 1) DL4DS_LAUNCH(spec_rows_kernel<true>, grid, block, 0, s, y, p, sh, ch, (const double*)mean,
                                         (const double2*)tb.twx, (const double*)tb.wx, (const double*)tb.wy, buf.zr, buf.zi);
                else DL4DS_LAUNCH(spec_rows_kernel<false>, grid, block, 0, s, y, p, sh, ch, (const double*)mean, (const double2*)tb.twx,
                                  (const double*)tb.wx, (const double*)tb.wy, buf.zr, buf.zi);
            }
            {
                ProfScope ps(s, "spectrum_cols", 8.0 * sides * (double)nfc * H * H * Wh, (16.0 * sides + 8.0 * (p ? 4 : 1)) * nfc * cells);
                const dim3 grid((unsigned)nfc, (unsigned)cdivz(H, SP_CM), (unsigned)cdivz(Wh, SP_CN));
                if (p) DL4DS_LAUNCH(spec_cols_kernel<2>, grid, block, 0, s, sh, nfc, (const double2*)tb.twy, (const double*)buf.zr,
                                    (const double*)buf.zi, buf.t);
                else DL4DS_LAUNCH(spec_cols_kernel<1>, grid, block, 0, s, sh, nfc, (const double2*)tb.twy, (const double*)buf.zr,
                                  (const double*)buf.zi, buf.t);
            }
            {
                ProfScope ps(s, "spectrum_bins", 0.0, 8.0 * (p ? 4 : 1) * nfc * cells);
                const dim3 grid((unsigned)(nfc * B));
                if (p) DL4DS_LAUNCH(spec_bins_kernel<4>, grid, block, 0, s, sh, ch, B, (const int*)tb.off, (const int*)tb.list,
                                    (const double*)buf.t, power);
                else DL4DS_LAUNCH(spec_bins_kernel<1>, grid, block, 0, s, sh, ch, B, (const int*)tb.off, (const int*)tb.list,
                                  (const double*)buf.t, power);
            }
        }
    }
    HIP_CHECK(hipGetLastError());
}
