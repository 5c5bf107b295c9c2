// DSSIM loss of dl4ds/losses.py:23-55 fused with its gradient w.r.t. the prediction:
//   drange = max(max y, max p) - min(min y, min p)   (whole batch; differentiated through, like TF does)
//   x = y - min(y) if min(y) < 0 else y ;  q = p - min(p) if min(p) < 0 else p
//   ssim   = tf.image.ssim(x, q, max_val=drange, 11x11 gaussian sigma 1.5, VALID, k1=.01, k2=.03)
//   dssim  = mean_n((1 - ssim_n)/2)
// Pivot: float32 moments of the values themselves lose sigma^2 = E[x^2] - mu^2 and sigma_xy to rounding as soon as the mean is large
// against the range (Kelvin, Pascal, a nearly constant field: c2 = (0.03 drange)^2 is all that is left).  Every tile kernel below
// therefore stages t - pivT and p - pivP, the batch-wide means of the two arrays (Stats; the min/max pass sums them in double, fixed
// order, so they are wave-uniform scalars and exact for a constant array), and takes all second moments of those.  Only the luminance
// term needs the means themselves: mu = (piv - shift) + mu', where shift is the negative minimum that the loss takes off.  The
// backward combines the same pivoted pixels with the transposed maps (x' T(va) + 2 q' T(vb) + T(vmu)): with raw pixels its three terms
// would cancel at the size of the offset.  Average pooling preserves a constant, so the multi-scale pyramid is built of pivoted images.
// Kernels: (1) min/max(+arg) reduction, (2) 16x16-tile SSIM map from an LDS halo tile -- the 11x11 Gaussian is applied
// separably (row pass over the 26 halo rows into LDS, then the column pass per output: 2 x 11 taps instead of 121) to the
// four moments -- emitting the three per-map derivatives, (3) the transposed (again separable) filter of those
// derivatives per input pixel, (4) scalar fix-ups (drange and shift terms routed to arg-max / arg-min).
// The loss, the multi-scale loss and image_metrics are built of one toolkit, each piece standing once: minmax_tree (both min/max
// kernels), tile_of / stage_pair / sep_moments (forward tiles), stage_maps3 / sep_transposed3 (the one backward tile kernel,
// ssim_bwd_kernel<WEIGHTED, REDUCE>), SsimPoint (the SSIM arithmetic of a window; ssim_fwd_kernel and ms_ssim_kernel differ in their
// epilogues only), route_range_and_shift (both finishing kernels), block_tree_sum of common.h (every block reduction), and on the
// host carve_stats / run_minmax / map_geom over one Bump carving, which the workspace-size functions and the launches share.
//
// Weighted form (dssim_forward_backward_weighted; contract in losses.hip): window weights omega = G * w over the VALID windows,
// term = sum omega (1 - s)/2 / sum omega, windows with omega == 0 excluded by selection.  omega_kernel WRITES the omega map once per
// call (w_batch x w_channels planes of Ho x Wo, the separable filter of the moments applied to w) together with per-tile sums, whose
// fixed-order double sum leaves 1 / sum omega in a device scalar; the WEIGHTED instantiations of the tile kernels multiply S, the three
// derivative maps and the c1 / c2 partials by omega at the window, and the backward and finishing kernels take their coefficient
// from that scalar -- so the drange and min-shift fix-ups carry the weights.  minmax_kernel is the unweighted one: dynamic range and
// positivity shift are those of the whole arrays, hence y_true must be finite everywhere.
#include "ops.h"
#include "prof.h"
#include <algorithm>

namespace {

constexpr int KF = 11, KH = 5, TS = 16, TL = TS + KF - 1;    // filter, half, tile, tile+halo
constexpr int PT = 48;      // LDS pitch of the halo tiles: consecutive rows start 16 banks apart, so the 2 rows x 16 columns
                            // a 32-lane LDS pass touches are conflict-free (the row-filtered tiles use pitch TS = 16 likewise)

struct Gauss { float g[KF]; };
Gauss make_gauss() {
    Gauss k;
    double s = 0;
    for (int i = 0; i < KF; ++i) { double c = i - (KF - 1) / 2.0; k.g[i] = (float)std::exp(-c * c / (2.0 * 1.5 * 1.5)); s += k.g[i]; }
    for (int i = 0; i < KF; ++i) k.g[i] = (float)(k.g[i] / s);   // outer(g,g)/sum == outer(g/s, g/s)
    return k;
}

struct Stats {            // device-resident scalars
    float minT, maxT, minP, maxP;
    unsigned long long argminP, argmaxP;
    float sumS, gc1, gc2, sumdy;
    float pivT, pivP;     // means of y_true, y_pred: the pivots of the window moments
};
// what a tile kernel takes off its pixels (pT, pP) and what the luminance term adds back to the pivoted means (oT, oP); `shift`:
// the loss's min-shift is in force (it is not for image_metrics)
struct Pivot { float pT, pP, oT, oP; };
__device__ __forceinline__ Pivot pivot_of(const Stats* __restrict__ st, bool shift) {
    const float shT = (shift && st->minT < 0.f) ? st->minT : 0.f, shP = (shift && st->minP < 0.f) ? st->minP : 0.f;
    return Pivot{st->pivT, st->pivP, st->pivT - shT, st->pivP - shP};
}

// Block result of the min/max pass: min / max of t, min / max of p with their flat indices, and the double sums of both.  Every
// thread hands in its own; ties of p's extremes go to the smallest flat index, as a serial scan would pick.  Row [.][0] holds the result
struct MinMaxRed { float s[4][256]; unsigned long long si[2][256]; double sd[2][256]; };
__device__ __forceinline__ void minmax_tree(MinMaxRed& r, int i, float mnT, float mxT, float mnP, float mxP, unsigned long long amn,
                                            unsigned long long amx, double sT, double sP) {
    r.s[0][i] = mnT; r.s[1][i] = mxT; r.s[2][i] = mnP; r.s[3][i] = mxP; r.si[0][i] = amn; r.si[1][i] = amx;
    r.sd[0][i] = sT; r.sd[1][i] = sP;
    block_tree(i, [&](int i, int j) {      // i keeps, j = i + o is folded in
        r.sd[0][i] += r.sd[0][j]; r.sd[1][i] += r.sd[1][j];
        r.s[0][i] = fminf(r.s[0][i], r.s[0][j]);
        r.s[1][i] = fmaxf(r.s[1][i], r.s[1][j]);
        if (r.s[2][j] < r.s[2][i] || (r.s[2][j] == r.s[2][i] && r.si[0][j] < r.si[0][i])) { r.s[2][i] = r.s[2][j]; r.si[0][i] = r.si[0][j]; }
        if (r.s[3][j] > r.s[3][i] || (r.s[3][j] == r.s[3][i] && r.si[1][j] < r.si[1][i])) { r.s[3][i] = r.s[3][j]; r.si[1][i] = r.si[1][j]; }
    });
}

__global__ void __launch_bounds__(256) minmax_kernel(const float* __restrict__ t, const float* __restrict__ p, size_t n,
                                                     float* __restrict__ pf, unsigned long long* __restrict__ pi,
                                                     double* __restrict__ ps) {
    __shared__ MinMaxRed r;
    float mnT = 3.4e38f, mxT = -3.4e38f, mnP = 3.4e38f, mxP = -3.4e38f;
    unsigned long long amn = 0, amx = 0;
    double sT = 0.0, sP = 0.0;
    for (size_t e = (size_t)blockIdx.x * 256 + threadIdx.x; e < n; e += (size_t)gridDim.x * 256) {
        const float a = t[e], b = p[e];
        mnT = fminf(mnT, a); mxT = fmaxf(mxT, a);
        if (b < mnP) { mnP = b; amn = e; }
        if (b > mxP) { mxP = b; amx = e; }
        sT += (double)a; sP += (double)b;
    }
    minmax_tree(r, threadIdx.x, mnT, mxT, mnP, mxP, amn, amx, sT, sP);
    if (threadIdx.x == 0) {
        for (int k = 0; k < 4; ++k) pf[blockIdx.x * 4 + k] = r.s[k][0];
        pi[blockIdx.x * 2] = r.si[0][0];
        pi[blockIdx.x * 2 + 1] = r.si[1][0];
        ps[blockIdx.x * 2] = r.sd[0][0];
        ps[blockIdx.x * 2 + 1] = r.sd[1][0];
    }
}
__global__ void __launch_bounds__(256) minmax_finish_kernel(const float* __restrict__ pf, const unsigned long long* __restrict__ pi,
                                                            const double* __restrict__ ps, double inv_n, int nb, Stats* st) {
    __shared__ MinMaxRed r;
    const int i = threadIdx.x;
    float mnT = 3.4e38f, mxT = -3.4e38f, mnP = 3.4e38f, mxP = -3.4e38f;
    unsigned long long amn = ~0ull, amx = ~0ull;
    double sT = 0.0, sP = 0.0;
    for (int k = i; k < nb; k += 256) {
        mnT = fminf(mnT, pf[4 * k]); mxT = fmaxf(mxT, pf[4 * k + 1]);
        if (pf[4 * k + 2] < mnP || (pf[4 * k + 2] == mnP && pi[2 * k] < amn)) { mnP = pf[4 * k + 2]; amn = pi[2 * k]; }
        if (pf[4 * k + 3] > mxP || (pf[4 * k + 3] == mxP && pi[2 * k + 1] < amx)) { mxP = pf[4 * k + 3]; amx = pi[2 * k + 1]; }
        sT += ps[2 * k]; sP += ps[2 * k + 1];
    }
    minmax_tree(r, i, mnT, mxT, mnP, mxP, amn, amx, sT, sP);
    if (i) return;
    st->minT = r.s[0][0]; st->maxT = r.s[1][0]; st->minP = r.s[2][0]; st->maxP = r.s[3][0]; st->argminP = r.si[0][0]; st->argmaxP = r.si[1][0];
    st->sumS = 0.f; st->gc1 = 0.f; st->gc2 = 0.f; st->sumdy = 0.f;
    st->pivT = (float)(r.sd[0][0] * inv_n); st->pivP = (float)(r.sd[1][0] * inv_n);
}

// block -> 16x16 tile (origin y0, x0) of plane (n, c) of a stack of C-channel planes, and this thread's pixel (ly, lx) of the tile
struct Tile { int c, n, y0, x0, ly, lx; };
__device__ __forceinline__ Tile tile_of(int tiles_x, int tiles_y, int C) {
    int b = blockIdx.x;
    const int tx = b % tiles_x; b /= tiles_x;
    const int ty = b % tiles_y; b /= tiles_y;
    return Tile{b % C, b / C, ty * TS, tx * TS, (int)threadIdx.x / TS, (int)threadIdx.x % TS};
}
// halo tile (TL x TL from the tile's origin) of the pixel pair of an NHWC array less (pT, pP), zero outside the image; ends in a barrier
__device__ __forceinline__ void stage_pair(float (*sx)[PT], float (*sq)[PT], const float* __restrict__ t, const float* __restrict__ p,
                                           float pT, float pP, const Tile& tl, int H, int W, int C) {
    for (int i = threadIdx.x; i < TL * TL; i += 256) {
        const int r = i / TL, cc = i % TL;
        const int y = tl.y0 + r, x = tl.x0 + cc;
        float a = 0.f, q = 0.f;
        if (y < H && x < W) {
            const size_t o = (((size_t)tl.n * H + y) * W + x) * C + tl.c;
            a = t[o] - pT; q = p[o] - pP;
        }
        sx[r][cc] = a; sq[r][cc] = q;
    }
    __syncthreads();
}
// halo tiles of the three derivative maps (planes of Ho x Wo) for a tile of INPUT pixels: input pixel (y,x) is covered by outputs
// (y-i, x-j), i,j in [0,10], so the halo tile starts at (y0-10, x0-10); zero outside the map; ends in a barrier
__device__ __forceinline__ void stage_maps3(float (*s1)[PT], float (*s2)[PT], float (*s3)[PT], const float* __restrict__ dmu,
                                            const float* __restrict__ da, const float* __restrict__ db, const Tile& tl, int Ho, int Wo,
                                            int C) {
    for (int i = threadIdx.x; i < TL * TL; i += 256) {
        const int r = i / TL, cc = i % TL;
        const int oy = tl.y0 - (KF - 1) + r, ox = tl.x0 - (KF - 1) + cc;
        float a = 0.f, bb = 0.f, d = 0.f;
        if (oy >= 0 && oy < Ho && ox >= 0 && ox < Wo) {
            const size_t o = (((size_t)tl.n * C + tl.c) * Ho + oy) * Wo + ox;
            a = dmu[o]; bb = da[o]; d = db[o];
        }
        s1[r][cc] = a; s2[r][cc] = bb; s3[r][cc] = d;
    }
    __syncthreads();
}

// Gaussian-filtered moments (mean x, mean q, E[xq], E[x^2 + q^2]) of this thread's output pixel of the tile: row pass of
// all TL halo rows into h (all 256 threads; contains a barrier), then the column pass.  sx, sq hold pivoted pixels.
struct MsMoments { float mx, my, A, Bq; };
__device__ __forceinline__ MsMoments sep_moments(const float (*sx)[PT], const float (*sq)[PT], float (*h)[TL][TS], const Gauss& gk) {
    for (int it = threadIdx.x; it < TL * TS; it += 256) {
        const int r = it / TS, cx = it % TS;
        float rx = 0.f, ry = 0.f, ra = 0.f, rb = 0.f;
#pragma unroll
        for (int j = 0; j < KF; ++j) {
            const float a = sx[r][cx + j], q = sq[r][cx + j], w = gk.g[j];
            rx += w * a; ry += w * q; ra += w * a * q; rb += w * (a * a + q * q);
        }
        h[0][r][cx] = rx; h[1][r][cx] = ry; h[2][r][cx] = ra; h[3][r][cx] = rb;
    }
    __syncthreads();
    const int ly = threadIdx.x / TS, lx = threadIdx.x % TS;
    MsMoments m{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int i = 0; i < KF; ++i) {
        const float w = gk.g[i];
        m.mx += w * h[0][ly + i][lx]; m.my += w * h[1][ly + i][lx]; m.A += w * h[2][ly + i][lx]; m.Bq += w * h[3][ly + i][lx];
    }
    return m;
}
// transposed filter of three derivative maps held as halo tiles starting (KF-1) pixels before the tile:
// T_k = sum_{i,j} g[i] g[j] s_k[ly + KF-1 - i][lx + KF-1 - j]
__device__ __forceinline__ void sep_transposed3(const float (*s1)[PT], const float (*s2)[PT], const float (*s3)[PT],
                                                float (*h)[TL][TS], const Gauss& gk, float& T1, float& T2, float& T3) {
    for (int it = threadIdx.x; it < TL * TS; it += 256) {
        const int r = it / TS, cx = it % TS;
        float r1 = 0.f, r2 = 0.f, r3 = 0.f;
#pragma unroll
        for (int j = 0; j < KF; ++j) {
            const float w = gk.g[j];
            r1 += w * s1[r][cx + (KF - 1) - j]; r2 += w * s2[r][cx + (KF - 1) - j]; r3 += w * s3[r][cx + (KF - 1) - j];
        }
        h[0][r][cx] = r1; h[1][r][cx] = r2; h[2][r][cx] = r3;
    }
    __syncthreads();
    const int ly = threadIdx.x / TS, lx = threadIdx.x % TS;
    T1 = T2 = T3 = 0.f;
#pragma unroll
    for (int i = 0; i < KF; ++i) {
        const float w = gk.g[i];
        T1 += w * h[0][ly + (KF - 1) - i][lx]; T2 += w * h[1][ly + (KF - 1) - i][lx]; T3 += w * h[2][ly + (KF - 1) - i][lx];
    }
}

// The SSIM of one window from its moments.  m holds moments of the pivoted pixels: the contrast-structure term cs = N2 / D2 is made of
// them alone, the luminance term lum = N1 / D1 of the means of the shifted arrays, mx = pv.oT + m.mx, my = pv.oP + m.my.  The
// derivatives are those of any f(lum, cs), given v = df/dlum and u = df/dcs (S = lum cs: v = cs, u = lum), w.r.t. the prediction's
// mean (dlum_dmy, dcs_dmy), the moments A = E[xq] and Bq = E[x^2 + q^2], and the constants c1, c2
__device__ __forceinline__ float drange_of(const Stats* __restrict__ st) { return fmaxf(st->maxT, st->maxP) - fminf(st->minT, st->minP); }
struct SsimConsts { float c1, c2; };
__device__ __forceinline__ SsimConsts ssim_consts(const Stats* __restrict__ st) {
    const float drange = drange_of(st);
    return SsimConsts{(0.01f * drange) * (0.01f * drange), (0.03f * drange) * (0.03f * drange)};
}
// d/ddrange through c1 = (k1 L)^2, c2 = (k2 L)^2, given the sums g1, g2 of the windows' d/dc1, d/dc2
__device__ __forceinline__ float drange_grad(const Stats* __restrict__ st, float g1, float g2) {
    const float drange = drange_of(st);
    return g1 * 2.f * 0.01f * 0.01f * drange + g2 * 2.f * 0.03f * 0.03f * drange;
}
struct SsimPoint {
    float mxs, mys, mx, my, N1, D1, N2, D2, lum, cs;
    __device__ __forceinline__ SsimPoint(MsMoments m, Pivot pv, SsimConsts k) {
        mxs = m.mx; mys = m.my;
        mx = pv.oT + m.mx; my = pv.oP + m.my;
        N1 = 2.f * mx * my + k.c1; D1 = mx * mx + my * my + k.c1;
        N2 = 2.f * m.A - 2.f * m.mx * m.my + k.c2; D2 = m.Bq - m.mx * m.mx - m.my * m.my + k.c2;
        lum = N1 / D1; cs = N2 / D2;
    }
    __device__ __forceinline__ float dlum_dmy() const { return 2.f * mx / D1 - N1 * 2.f * my / (D1 * D1); }
    __device__ __forceinline__ float dcs_dmy() const { return -2.f * mxs / D2 + N2 * 2.f * mys / (D2 * D2); }
    __device__ __forceinline__ float dS_dA(float u) const { return u * 2.f / D2; }
    __device__ __forceinline__ float dS_dB(float u) const { return -u * N2 / (D2 * D2); }
    __device__ __forceinline__ float dS_dc1(float v) const { return v * (D1 - N1) / (D1 * D1); }
    __device__ __forceinline__ float dS_dc2(float u) const { return u * (D2 - N2) / (D2 * D2); }
};

// omega[(m, c), oy, ox] = sum_ij g[i] g[j] w[m, oy + i, ox + j, c]; one block = one 16x16 tile of plane (m, c) of the w_batch x cw
// weight planes; partial[block] = the tile's sum of omega.  All taps and weights are >= 0: omega == 0 iff the whole window is masked.
__global__ void __launch_bounds__(256) omega_kernel(const float* __restrict__ w, int H, int W, int cw, int Ho, int Wo, int tiles_x,
                                                    int tiles_y, Gauss gk, float* __restrict__ omega, float* __restrict__ partial) {
    __shared__ float sw[TL][PT], h[TL][TS];
    __shared__ float red[256];
    const Tile tl = tile_of(tiles_x, tiles_y, cw);          // n: the map m
    for (int i = threadIdx.x; i < TL * TL; i += 256) {
        const int r = i / TL, cc = i % TL;
        const int y = tl.y0 + r, x = tl.x0 + cc;
        sw[r][cc] = (y < H && x < W) ? w[(((size_t)tl.n * H + y) * W + x) * cw + tl.c] : 0.f;
    }
    __syncthreads();
    for (int it = threadIdx.x; it < TL * TS; it += 256) {
        const int r = it / TS, cx = it % TS;
        float a = 0.f;
#pragma unroll
        for (int j = 0; j < KF; ++j) a += gk.g[j] * sw[r][cx + j];
        h[r][cx] = a;
    }
    __syncthreads();
    const int oy = tl.y0 + tl.ly, ox = tl.x0 + tl.lx;
    float om = 0.f;
    if (oy < Ho && ox < Wo) {
#pragma unroll
        for (int i = 0; i < KF; ++i) om += gk.g[i] * h[tl.ly + i][tl.lx];
        omega[(((size_t)tl.n * cw + tl.c) * Ho + oy) * Wo + ox] = om;
    }
    red[threadIdx.x] = om;
    block_tree_sum(red, threadIdx.x);
    if (threadIdx.x == 0) partial[blockIdx.x] = red[0];
}

// one block = one 16x16 tile of the (Ho,Wo) SSIM map of plane (n,c).  WEIGHTED: S, the derivative maps and the c1 / c2 partials are
// multiplied by omega[(n / wrep, cw == C ? c : 0), oy, ox]; a window with omega == 0 contributes exact zeros whatever it holds
template <bool WEIGHTED>
__global__ void __launch_bounds__(256) ssim_fwd_kernel(const float* __restrict__ t, const float* __restrict__ p, int H, int W,
                                                       int C, int Ho, int Wo, int tiles_x, int tiles_y, Gauss gk,
                                                       const Stats* __restrict__ st, float* __restrict__ dmu,
                                                       float* __restrict__ da, float* __restrict__ db,
                                                       float* __restrict__ partial, const float* __restrict__ omega, int wrep,
                                                       int cw) {
    __shared__ float sx[TL][PT], sq[TL][PT], hrow[4][TL][TS];
    __shared__ float red[3][256];
    const Tile tl = tile_of(tiles_x, tiles_y, C);
    const int c = tl.c, n = tl.n;
    const Pivot pv = pivot_of(st, true);
    const SsimConsts kc = ssim_consts(st);
    stage_pair(sx, sq, t, p, pv.pT, pv.pP, tl, H, W, C);
    const int oy = tl.y0 + tl.ly, ox = tl.x0 + tl.lx;
    float S = 0.f, g1 = 0.f, g2 = 0.f;
    const MsMoments mom = sep_moments(sx, sq, hrow, gk);
    if (oy < Ho && ox < Wo) {
        // SsimPoint's arithmetic, written out: through the struct the compiler packs the column pass of the WEIGHTED instantiation
        // in pairs and fuses fewer of its multiply-adds, which moves the last bits of the loss
        const float c1 = kc.c1, c2 = kc.c2;
        const float mxs = mom.mx, mys = mom.my, A = mom.A, Bq = mom.Bq;      // moments of the pivoted pixels
        const float mx = pv.oT + mxs, my = pv.oP + mys;                      // means of the shifted arrays: luminance only
        const float N1 = 2.f * mx * my + c1, D1 = mx * mx + my * my + c1;
        const float N2 = 2.f * A - 2.f * mxs * mys + c2, D2 = Bq - mxs * mxs - mys * mys + c2;
        const float lum = N1 / D1, cs = N2 / D2;
        S = lum * cs;
        const size_t o = (((size_t)n * C + c) * Ho + oy) * Wo + ox;
        float vmu = cs * (2.f * mx / D1 - N1 * 2.f * my / (D1 * D1)) + lum * (-2.f * mxs / D2 + N2 * 2.f * mys / (D2 * D2));
        float va = lum * 2.f / D2;
        float vb = -lum * N2 / (D2 * D2);
        g1 = cs * (D1 - N1) / (D1 * D1);
        g2 = lum * (D2 - N2) / (D2 * D2);
        if (WEIGHTED) {
            const float om = omega[(((size_t)(n / wrep) * cw + (cw == C ? c : 0)) * Ho + oy) * Wo + ox];
            if (om > 0.f) { S *= om; vmu *= om; va *= om; vb *= om; g1 *= om; g2 *= om; }
            else { S = 0.f; vmu = 0.f; va = 0.f; vb = 0.f; g1 = 0.f; g2 = 0.f; }
        }
        dmu[o] = vmu;
        da[o] = va;
        db[o] = vb;
    }
    red[0][threadIdx.x] = S; red[1][threadIdx.x] = g1; red[2][threadIdx.x] = g2;
    block_tree_sum(red, threadIdx.x);
    if (threadIdx.x == 0)
        for (int k = 0; k < 3; ++k) partial[(size_t)blockIdx.x * 3 + k] = red[k][0];
}

// First stage of the long partial-sum reductions: out[g][k] = sum of in[r][k] over the g-th slice of the nb rows (fixed
// order, double accumulation), so the single-block finishing kernels read COMPACT_G rows instead of one per tile.
constexpr int COMPACT_G = 64;
template <int K>
__global__ void __launch_bounds__(256) compact_partials_kernel(const float* __restrict__ in, int nb, float* __restrict__ out) {
    __shared__ double red[K][256];
    const int chunk = (nb + (int)gridDim.x - 1) / (int)gridDim.x;
    const int r0 = blockIdx.x * chunk, r1 = min(r0 + chunk, nb);
    double a[K];
#pragma unroll
    for (int k = 0; k < K; ++k) a[k] = 0.0;
    for (int r = r0 + threadIdx.x; r < r1; r += 256)
#pragma unroll
        for (int k = 0; k < K; ++k) a[k] += (double)in[(size_t)r * K + k];
#pragma unroll
    for (int k = 0; k < K; ++k) red[k][threadIdx.x] = a[k];
    block_tree_sum(red, threadIdx.x);
    if (threadIdx.x == 0)
#pragma unroll
        for (int k = 0; k < K; ++k) out[(size_t)blockIdx.x * K + k] = (float)red[k][0];
}

__global__ void sum3_kernel(const float* __restrict__ partial, int nb, Stats* st) {
    __shared__ double red[3][256];
    double a[3] = {0, 0, 0};
    for (int k = threadIdx.x; k < nb; k += 256)
        for (int j = 0; j < 3; ++j) a[j] += partial[(size_t)k * 3 + j];
    for (int j = 0; j < 3; ++j) red[j][threadIdx.x] = a[j];
    block_tree_sum(red, threadIdx.x);
    if (threadIdx.x == 0) { st->sumS = (float)red[0][0]; st->gc1 = (float)red[1][0]; st->gc2 = (float)red[2][0]; }
}

// one block = one 16x16 tile of INPUT pixels of plane (n,c): transposed 11x11 filter of the derivative maps, combined with the pivoted
// pixels the moments were taken of (raw: t, p are y_true / y_pred themselves, pivoted here; else images of the pivoted pyramid);
// dpred (+)= coef * that.  WEIGHTED: the maps already carry omega; coef (-weight / 2 here) is completed by 1 / sum omega from the
// device scalar.  REDUCE: partial[block] = the tile's sum (for the min-shift term); the pyramid levels of the multi-scale loss run
// without it, with coef = 1 and accumulate = 0 (both exact)
template <bool WEIGHTED, bool REDUCE>
__global__ void __launch_bounds__(256) ssim_bwd_kernel(const float* __restrict__ t, const float* __restrict__ p, int raw, int H, int W,
                                                       int C, int Ho, int Wo, int tiles_x, int tiles_y, Gauss gk,
                                                       const Stats* __restrict__ st, const float* __restrict__ dmu,
                                                       const float* __restrict__ da, const float* __restrict__ db,
                                                       float coef, float* __restrict__ dpred, int accumulate,
                                                       float* __restrict__ partial, const float* __restrict__ inv_so) {
    __shared__ float s1[TL][PT], s2[TL][PT], s3[TL][PT], hrow[3][TL][TS];
    if (WEIGHTED) coef *= inv_so[0];
    const Tile tl = tile_of(tiles_x, tiles_y, C);
    const float pT = raw ? st->pivT : 0.f, pP = raw ? st->pivP : 0.f;
    stage_maps3(s1, s2, s3, dmu, da, db, tl, Ho, Wo, C);
    const int y = tl.y0 + tl.ly, x = tl.x0 + tl.lx;
    float g = 0.f;
    float T1, T2, T3;
    sep_transposed3(s1, s2, s3, hrow, gk, T1, T2, T3);
    if (y < H && x < W) {
        const size_t o = (((size_t)tl.n * H + y) * W + x) * C + tl.c;
        const float xv = t[o] - pT, qv = p[o] - pP;
        g = coef * (T1 + xv * T2 + 2.f * qv * T3);
        dpred[o] = accumulate ? dpred[o] + g : g;
    }
    if constexpr (REDUCE) {
        __shared__ float red[256];
        red[threadIdx.x] = g;
        block_tree_sum(red, threadIdx.x);
        if (threadIdx.x == 0) partial[blockIdx.x] = red[0];
    }
}

// the scalar terms of the gradient, each added to one element of dpred: ddr (the range, through c1 and c2 of every window) where the
// prediction sets that end of the range, sumdy (the min-shift q = p - min(p)) at the prediction's minimum
__device__ __forceinline__ void route_range_and_shift(const Stats* __restrict__ st, float ddr, float sumdy, float* __restrict__ dpred) {
    if (st->maxP > st->maxT) dpred[st->argmaxP] += ddr;      // tf.maximum routes ties to its first argument (y_true)
    if (st->minP < st->minT) dpred[st->argminP] -= ddr;
    if (st->minP < 0.f) dpred[st->argminP] -= sumdy;
}

// WEIGHTED: inv_m and the completion of coef (-weight / 2 here) are 1 / sum omega from the device scalar; a zero sum gives loss 0
template <bool WEIGHTED>
__global__ void dssim_finish_kernel(const float* __restrict__ partial, int nb, Stats* st, float weight, float inv_m,
                                    float coef, float* __restrict__ dpred, float* __restrict__ loss_out, int accumulate_loss,
                                    const float* __restrict__ inv_so) {
    __shared__ double red[256];
    double a = 0;
    for (int k = threadIdx.x; k < nb; k += 256) a += partial[k];
    red[threadIdx.x] = a;
    block_tree_sum(red, threadIdx.x);
    if (threadIdx.x != 0) return;
    const float sumdy = (float)red[0];
    if (WEIGHTED) { inv_m = inv_so[0]; coef *= inv_m; }
    const float v = (WEIGHTED && inv_m == 0.f) ? 0.f : weight * (0.5f - 0.5f * st->sumS * inv_m);
    loss_out[0] = accumulate_loss ? loss_out[0] + v : v;
    if (!dpred) return;
    route_range_and_shift(st, coef * drange_grad(st, st->gc1, st->gc2), sumdy, dpred);
}

// ---- host: the workspace.  Bump carves 256-byte-aligned arrays off a base in order; the size functions run the same carving on a
// null base and read the end offset, so a size and its carving cannot disagree
struct Bump {
    uintptr_t base;
    size_t o = 0;
    explicit Bump(void* ws) : base(reinterpret_cast<uintptr_t>(ws)) {}
    template <class T> T* take(size_t count) {
        T* r = reinterpret_cast<T*>(base + o);
        o += (count * sizeof(T) + 255) & ~(size_t)255;
        return r;
    }
};
// head of every workspace here: the Stats and the nb_mm per-block results of the min/max pass
struct StatsScratch { Stats* st; float* pf; unsigned long long* pi; double* ps; int nb_mm; };
StatsScratch carve_stats(Bump& b) {
    StatsScratch h;
    h.nb_mm = 512;
    h.st = b.take<Stats>(1);
    h.pf = b.take<float>((size_t)h.nb_mm * 4);
    h.pi = b.take<unsigned long long>((size_t)h.nb_mm * 2);
    h.ps = b.take<double>((size_t)h.nb_mm * 2);
    return h;
}
// Stats of the n elements of (t, p): extremes, the prediction's arg-extremes, the pivots; the loss sums zeroed
void run_minmax(hipStream_t s, const float* t, const float* p, size_t n, const StatsScratch& h) {
    const int nb = (int)std::min<size_t>(h.nb_mm, cdivz(n, 256));
    DL4DS_LAUNCH(minmax_kernel, dim3(nb), dim3(256), 0, s, t, p, n, h.pf, h.pi, h.ps);
    DL4DS_LAUNCH(minmax_finish_kernel, dim3(1), dim3(256), 0, s, h.pf, h.pi, h.ps, 1.0 / (double)n, nb, h.st);
}
// the VALID map of an (H, W) image and its tiles
struct MapGeom { int Ho, Wo, txo, tyo; };
MapGeom map_geom(int H, int W) {
    const int Ho = H - KF + 1, Wo = W - KF + 1;
    return MapGeom{Ho, Wo, cdiv(Wo, TS), cdiv(Ho, TS)};
}

struct Layout { StatsScratch hdr; MapGeom g; float *maps, *part, *part2; size_t total; };
Layout layout(void* ws, int N, int H, int W, int C) {
    Bump b(ws);
    Layout l;
    l.g = map_geom(H, W);
    l.hdr = carve_stats(b);
    l.maps = b.take<float>(3 * (size_t)N * C * l.g.Ho * l.g.Wo);
    l.part = b.take<float>((size_t)N * C * cdiv(H, TS) * cdiv(W, TS) * 3);
    l.part2 = b.take<float>((size_t)COMPACT_G * 3);
    l.total = b.o;
    return l;
}

// ============================================================================================ multi-scale DSSIM
// msdssim of dl4ds/losses.py:92-130 (+ the mixes :133-149): tf.image.ssim_multiscale with four scales.  Scale k is the
// shifted image pair halved k times (2x2 average, odd sizes SYMMETRIC-padded = edge row/column repeated).  Per scale and
// per (n, c): cs_k = mean contrast-structure, and on the last scale ssim_3 = mean luminance*cs; relu'd,
//     ms[n,c] = cs_0^w0 * cs_1^w1 * cs_2^w2 * ssim_3^w3 ,  loss = weight * mean_n (1 - mean_c ms) / 2 .
// Passes: pooled pyramids -> per-tile (ssim, cs) sums per scale -> per-(n,c) means -> one block combines them into the
// loss and the upstream weights G -> per scale: derivative maps (moments recomputed, weighted by G) -> transposed filter
// into a per-scale image gradient -> coarse-to-fine accumulation through the pooling adjoint -> dpred, plus the same
// drange / min-shift fix-ups as the single-scale loss.  All reductions have a fixed order (deterministic).
constexpr int MS_SCALES = 4;
struct MsDims { int H[MS_SCALES], W[MS_SCALES]; };

// dst (Hd, Wd) = 2x2 average of src (Hs, Ws) less its pivot (scale 0 -> 1 reads the raw array; the coarser images are pivoted
// already), edge repeated.  The pivot comes off each source, not off the sum: the sum of four raw values rounds at the size of the mean
__global__ void ms_pool_kernel(const float* __restrict__ src, float* __restrict__ dst, int N, int Hs, int Ws, int Hd, int Wd,
                               int C, const Stats* __restrict__ st, int which) {      // which: 0 none, 1 y_true, 2 y_pred
    const float pv = which == 1 ? st->pivT : which == 2 ? st->pivP : 0.f;
    const size_t total = (size_t)N * Hd * Wd * C;
    for (size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (size_t)gridDim.x * blockDim.x) {
        const int c = (int)(e % C);
        size_t r = e / C;
        const int x = (int)(r % Wd); r /= Wd;
        const int y = (int)(r % Hd);
        const int n = (int)(r / Hd);
        const int y0 = 2 * y, y1 = min(2 * y + 1, Hs - 1), x0 = 2 * x, x1 = min(2 * x + 1, Ws - 1);
        const float* b = src + (size_t)n * Hs * Ws * C + c;
        const float v = (b[((size_t)y0 * Ws + x0) * C] - pv) + (b[((size_t)y0 * Ws + x1) * C] - pv) +
                        (b[((size_t)y1 * Ws + x0) * C] - pv) + (b[((size_t)y1 * Ws + x1) * C] - pv);
        dst[e] = 0.25f * v;
    }
}

// fine (Hs, Ws) += pooling adjoint of coarse (Hd, Wd): each of the four (possibly repeated) sources gets 1/4
__global__ void ms_unpool_add_kernel(float* __restrict__ fine, const float* __restrict__ coarse, int N, int Hs, int Ws, int Hd,
                                     int Wd, int C) {
    const size_t total = (size_t)N * Hs * Ws * C;
    for (size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (size_t)gridDim.x * blockDim.x) {
        const int c = (int)(e % C);
        size_t r = e / C;
        const int x = (int)(r % Ws); r /= Ws;
        const int y = (int)(r % Hs);
        const int n = (int)(r / Hs);
        const float wy = ((Hs & 1) && y == Hs - 1) ? 2.f : 1.f;      // the repeated edge row counts twice
        const float wx = ((Ws & 1) && x == Ws - 1) ? 2.f : 1.f;
        fine[e] += 0.25f * wy * wx * coarse[(((size_t)n * Hd + y / 2) * Wd + x / 2) * C + c];
    }
}

// MODE 0: partial[block] = (sum ssim, sum cs) of the tile.  MODE 1: derivative maps weighted by gs[n,c] (ssim) and gc[n,c]
// (cs), partial[block] = (d/dc1, d/dc2).  x / q: scale images (raw: y_true / y_pred themselves, pivoted here; else images of the
// pivoted pyramid).  shift: the loss's min-shift enters the luminance means (0 for image_metrics).
template <int MODE>
__global__ void __launch_bounds__(256) ms_ssim_kernel(const float* __restrict__ x, const float* __restrict__ q, int raw, int shift, int H, int W,
                                                      int C, int Ho, int Wo, int tiles_x, int tiles_y, Gauss gk,
                                                      const Stats* __restrict__ st, const float* __restrict__ gs,
                                                      const float* __restrict__ gc, float* __restrict__ dmu, float* __restrict__ da,
                                                      float* __restrict__ db, float* __restrict__ partial) {
    __shared__ float sx[TL][PT], sq[TL][PT], hrow[4][TL][TS];
    __shared__ float red[2][256];
    const Tile tl = tile_of(tiles_x, tiles_y, C);
    const int c = tl.c, n = tl.n;
    const Pivot pv = pivot_of(st, shift != 0);
    const SsimConsts kc = ssim_consts(st);
    stage_pair(sx, sq, x, q, raw ? pv.pT : 0.f, raw ? pv.pP : 0.f, tl, H, W, C);
    const int oy = tl.y0 + tl.ly, ox = tl.x0 + tl.lx;
    float r0 = 0.f, r1 = 0.f;
    const MsMoments m = sep_moments(sx, sq, hrow, gk);
    if (oy < Ho && ox < Wo) {
        const SsimPoint s(m, pv, kc);
        if (MODE == 0) {
            r0 = s.lum * s.cs; r1 = s.cs;
        } else {
            const float inv_m = 1.f / ((float)Ho * (float)Wo);
            const float ws = gs[n * C + c] * inv_m, wc = gc[n * C + c] * inv_m;
            const float dcs_dmy = s.dcs_dmy(), dlum_dmy = s.dlum_dmy();
            const size_t o = (((size_t)n * C + c) * Ho + oy) * Wo + ox;
            const float v = ws * s.cs, u = ws * s.lum + wc;              // d/dlum, d/dcs of ws lum cs + wc cs
            dmu[o] = ws * (s.cs * dlum_dmy + s.lum * dcs_dmy) + wc * dcs_dmy;
            da[o] = s.dS_dA(u);
            db[o] = s.dS_dB(u);
            r0 = s.dS_dc1(v);
            r1 = s.dS_dc2(u);
        }
    }
    red[0][threadIdx.x] = r0; red[1][threadIdx.x] = r1;
    block_tree_sum(red, threadIdx.x);
    if (threadIdx.x == 0) { partial[(size_t)blockIdx.x * 2] = red[0][0]; partial[(size_t)blockIdx.x * 2 + 1] = red[1][0]; }
}

// mean_ssim[nc], mean_cs[nc] of one scale from its per-tile sums (tiles of a plane are consecutive blocks); one wavefront
// per plane: lane-strided loads, fixed shuffle tree
__global__ void __launch_bounds__(64) ms_means_kernel(const float* __restrict__ partial, int tiles, int NC, float inv_m,
                                                      float* __restrict__ mean_ssim, float* __restrict__ mean_cs) {
    const int nc = blockIdx.x;
    double a = 0, b = 0;
    for (int k = threadIdx.x; k < tiles; k += 64) { a += partial[((size_t)nc * tiles + k) * 2]; b += partial[((size_t)nc * tiles + k) * 2 + 1]; }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { a += __shfl_xor(a, o, 64); b += __shfl_xor(b, o, 64); }
    if (threadIdx.x == 0) {
        mean_ssim[nc] = (float)(a * inv_m);
        mean_cs[nc] = (float)(b * inv_m);
    }
}

// one block: loss value and the upstream weights gs[k][nc] (only the last scale), gc[k][nc] (the other scales)
__global__ void __launch_bounds__(256) ms_combine_kernel(const float* __restrict__ mean_ssim, const float* __restrict__ mean_cs, int NC,
                                                         float weight, float* __restrict__ gs, float* __restrict__ gc,
                                                         float* __restrict__ loss_out, int accumulate_loss) {
    const float pw[MS_SCALES] = {0.0448f, 0.2856f, 0.3001f, 0.2363f};
    __shared__ double red[256];
    double acc = 0;
    for (int nc = threadIdx.x; nc < NC; nc += 256) {
        float v[MS_SCALES], ms = 1.f;
#pragma unroll
        for (int k = 0; k < MS_SCALES; ++k) {
            v[k] = fmaxf(k == MS_SCALES - 1 ? mean_ssim[k * NC + nc] : mean_cs[k * NC + nc], 0.f);
            ms *= powf(v[k], pw[k]);
        }
        acc += ms;
        const float up = -0.5f * weight / (float)NC;                       // dL/dms[n,c]
#pragma unroll
        for (int k = 0; k < MS_SCALES; ++k) {
            const float g = v[k] > 0.f ? up * pw[k] * ms / v[k] : 0.f;
            gs[k * NC + nc] = (k == MS_SCALES - 1) ? g : 0.f;
            gc[k * NC + nc] = (k == MS_SCALES - 1) ? 0.f : g;
        }
    }
    red[threadIdx.x] = acc;
    block_tree_sum(red, threadIdx.x);
    if (threadIdx.x == 0) {
        const float v = weight * (0.5f - 0.5f * (float)(red[0] / NC));
        loss_out[0] = accumulate_loss ? loss_out[0] + v : v;
    }
}

// dpred (+)= g0 ; partial[block] = sum of g0 over the block's elements (for the min-shift term)
__global__ void __launch_bounds__(256) ms_apply_kernel(const float* __restrict__ g0, float* __restrict__ dpred, size_t n, int accumulate,
                                                       float* __restrict__ partial) {
    __shared__ float red[256];
    float s = 0.f;
    for (size_t e = (size_t)blockIdx.x * 256 + threadIdx.x; e < n; e += (size_t)gridDim.x * 256) {
        const float g = g0[e];
        dpred[e] = accumulate ? dpred[e] + g : g;
        s += g;
    }
    red[threadIdx.x] = s;
    block_tree_sum(red, threadIdx.x);
    if (threadIdx.x == 0) partial[blockIdx.x] = red[0];
}

// scalar fix-ups: drange enters every scale's c1, c2; the prediction's minimum shifts the whole image
__global__ void __launch_bounds__(256) ms_finish_kernel(const float* __restrict__ sum_partial, int nb_sum, const float* __restrict__ gcp,
                                                        int ng, const Stats* __restrict__ st, float* __restrict__ dpred) {
    __shared__ double red[3][256];
    double a = 0, g1 = 0, g2 = 0;
    for (int k = threadIdx.x; k < nb_sum; k += 256) a += sum_partial[k];
    for (int k = threadIdx.x; k < ng; k += 256) { g1 += gcp[(size_t)k * 2]; g2 += gcp[(size_t)k * 2 + 1]; }
    red[0][threadIdx.x] = a; red[1][threadIdx.x] = g1; red[2][threadIdx.x] = g2;
    block_tree_sum(red, threadIdx.x);
    if (threadIdx.x != 0) return;
    route_range_and_shift(st, drange_grad(st, (float)red[1][0], (float)red[2][0]), (float)red[0][0], dpred);
}

struct MsLayout {
    StatsScratch hdr;
    float *imgs, *grads, *maps, *part, *part2, *gcp, *means, *gw;
    size_t total, img_off[MS_SCALES], grad_off[MS_SCALES], gcp_off[MS_SCALES];      // offsets in floats
    MsDims d;
    MapGeom g[MS_SCALES];
};
MsLayout ms_layout(void* ws, int N, int H, int W, int C) {
    Bump b(ws);
    MsLayout l;
    l.d.H[0] = H; l.d.W[0] = W;
    for (int k = 1; k < MS_SCALES; ++k) { l.d.H[k] = (l.d.H[k - 1] + 1) / 2; l.d.W[k] = (l.d.W[k - 1] + 1) / 2; }
    l.hdr = carve_stats(b);
    size_t img = 0, grad = 0, gcp = 0;
    for (int k = 0; k < MS_SCALES; ++k) {
        const size_t n = (size_t)N * l.d.H[k] * l.d.W[k] * C;
        if (k > 0) { l.img_off[k] = img; img += 2 * n; } else l.img_off[k] = 0;      // x_k then q_k (k >= 1)
        l.grad_off[k] = grad; grad += n;
        l.gcp_off[k] = gcp;
        l.g[k] = map_geom(l.d.H[k], l.d.W[k]);
        gcp += (size_t)N * C * l.g[k].tyo * l.g[k].txo;
    }
    l.imgs = b.take<float>(img);
    l.grads = b.take<float>(grad);
    l.maps = b.take<float>(3 * (size_t)N * C * l.g[0].Ho * l.g[0].Wo);
    l.part = b.take<float>(std::max<size_t>((size_t)N * C * l.g[0].tyo * l.g[0].txo * 2, 4096));
    l.part2 = b.take<float>((size_t)COMPACT_G * 2);
    l.gcp = b.take<float>(gcp * 2);
    l.means = b.take<float>((size_t)2 * MS_SCALES * N * C);      // [ssim: scales x NC][cs: scales x NC]
    l.gw = b.take<float>((size_t)2 * MS_SCALES * N * C);         // [gs: scales x NC][gc: scales x NC]
    l.total = b.o;
    return l;
}
}  // namespace

size_t dssim_workspace_bytes(int N, int H, int W, int C) { return layout(nullptr, N, H, W, C).total; }

void weight_sum_finish(hipStream_t s, const float* partial, int nb, double mult, float* inv_out);     // losses.hip

namespace {
// the weight side of one weighted call: maps, their batch / channel counts, the device scalar 1 / sum omega, and the extra workspace
struct DssimWeights { const float* w; int wb, cw; float* inv_so; float* ext; };
size_t omega_floats(const MapGeom& g, int wb, int cw) { return ((size_t)wb * cw * g.Ho * g.Wo + 63) & ~(size_t)63; }
size_t omega_tiles(const MapGeom& g, int wb, int cw) { return (size_t)wb * cw * g.tyo * g.txo; }

template <bool WEIGHTED>
void dssim_run(hipStream_t s, const float* y_true, const float* y_pred, float* dpred, int N, int H, int W, int C, float weight,
               float* loss_out, int accumulate_loss, float* workspace, size_t workspace_bytes, const DssimWeights& dw) {
    DL4DS_REQUIRE(H >= KF && W >= KF, "dssim needs grids of at least 11x11");
    const Layout l = layout(workspace, N, H, W, C);
    DL4DS_REQUIRE(workspace_bytes >= l.total, "dssim workspace too small");
    Stats* st = l.hdr.st;
    const int Ho = l.g.Ho, Wo = l.g.Wo, txo = l.g.txo, tyo = l.g.tyo;
    const size_t msz = (size_t)N * C * Ho * Wo;
    float* dmu = l.maps;
    float* da = dmu + msz;
    float* db = da + msz;
    float* part = l.part;
    float* part2 = l.part2;
    const size_t n = (size_t)N * H * W * C;
    static const Gauss gk = make_gauss();
    ProfScope ps(s, "dssim", 0.0, 4.0 * (double)n * 8);
    run_minmax(s, y_true, y_pred, n, l.hdr);
    const int nbf = N * C * txo * tyo;
    const float* omega = nullptr;
    const float* inv_so = nullptr;
    int wrep = 1, cw = 1;
    if (WEIGHTED) {
        float* om = dw.ext;
        float* opart = dw.ext + omega_floats(l.g, dw.wb, dw.cw);
        const int nbo = (int)omega_tiles(l.g, dw.wb, dw.cw);
        DL4DS_LAUNCH(omega_kernel, dim3(nbo), dim3(256), 0, s, dw.w, H, W, dw.cw, Ho, Wo, txo, tyo, gk, om, opart);
        // sum over samples, windows and channels = the planes' sum times how often each plane is used
        weight_sum_finish(s, opart, nbo, (double)(N / dw.wb) * (double)(C / dw.cw), dw.inv_so);
        omega = om; inv_so = dw.inv_so; wrep = N / dw.wb; cw = dw.cw;
    }
    DL4DS_LAUNCH(ssim_fwd_kernel<WEIGHTED>, dim3(nbf), dim3(256), 0, s, y_true, y_pred, H, W, C, Ho, Wo, txo, tyo, gk, st, dmu, da,
                       db, part, omega, wrep, cw);
    DL4DS_LAUNCH(compact_partials_kernel<3>, dim3(COMPACT_G), dim3(256), 0, s, part, nbf, part2);
    DL4DS_LAUNCH(sum3_kernel, dim3(1), dim3(256), 0, s, part2, COMPACT_G, st);
    const float inv_m = 1.f / (float)msz;
    const float coef = WEIGHTED ? -0.5f * weight : -0.5f * weight * inv_m;      // WEIGHTED: completed on the device by 1 / sum omega
    int nbb = 0;
    if (dpred) {
        const int txi = cdiv(W, TS), tyi = cdiv(H, TS);
        nbb = N * C * txi * tyi;
        DL4DS_LAUNCH((ssim_bwd_kernel<WEIGHTED, true>), dim3(nbb), dim3(256), 0, s, y_true, y_pred, 1, H, W, C, Ho, Wo, txi, tyi, gk, st,
                           dmu, da, db, coef, dpred, 1, part, inv_so);
    }
    if (nbb) DL4DS_LAUNCH(compact_partials_kernel<1>, dim3(COMPACT_G), dim3(256), 0, s, part, nbb, part2);
    DL4DS_LAUNCH(dssim_finish_kernel<WEIGHTED>, dim3(1), dim3(256), 0, s, part2, nbb ? COMPACT_G : 0, st, weight, inv_m, coef, dpred,
                       loss_out, accumulate_loss, inv_so);
    HIP_CHECK(hipGetLastError());
}
}  // namespace

void dssim_forward_backward(hipStream_t s, const float* y_true, const float* y_pred, float* dpred, int N, int H, int W, int C,
                            float weight, float* loss_out, int accumulate_loss, float* workspace, size_t workspace_bytes) {
    dssim_run<false>(s, y_true, y_pred, dpred, N, H, W, C, weight, loss_out, accumulate_loss, workspace, workspace_bytes,
                     DssimWeights{nullptr, 1, 1, nullptr, nullptr});
}

size_t dssim_weighted_workspace_bytes(int N, int H, int W, int C, int w_batch, int w_channels) {
    (void)N; (void)C;
    if (H < KF || W < KF) return 0;
    const MapGeom g = map_geom(H, W);
    return (omega_floats(g, w_batch, w_channels) + omega_tiles(g, w_batch, w_channels)) * sizeof(float);
}

// w: w_batch maps (H, W, w_channels) (contract in losses.hip); inv_so_dev: one device float that receives 1 / sum omega; ext: the
// omega map and its per-tile sums (dssim_weighted_workspace_bytes)
void dssim_forward_backward_weighted(hipStream_t s, const float* y_true, const float* y_pred, float* dpred, int N, int H, int W,
                                     int C, float weight, float* loss_out, int accumulate_loss, const float* w, int w_batch,
                                     int w_channels, float* inv_so_dev, float* workspace, size_t workspace_bytes, float* ext,
                                     size_t ext_bytes) {
    DL4DS_REQUIRE(H >= KF && W >= KF, "dssim needs grids of at least 11x11");
    DL4DS_REQUIRE(ext_bytes >= dssim_weighted_workspace_bytes(N, H, W, C, w_batch, w_channels), "weighted dssim workspace too small");
    dssim_run<true>(s, y_true, y_pred, dpred, N, H, W, C, weight, loss_out, accumulate_loss, workspace, workspace_bytes,
                    DssimWeights{w, w_batch, w_channels, inv_so_dev, ext});
}

size_t msdssim_workspace_bytes(int N, int H, int W, int C) { return ms_layout(nullptr, N, H, W, C).total; }

void msdssim_forward_backward(hipStream_t s, const float* y_true, const float* y_pred, float* dpred, int N, int H, int W, int C,
                              float weight, float* loss_out, int accumulate_loss, float* workspace, size_t workspace_bytes) {
    DL4DS_REQUIRE(((H + 7) / 8) >= KF && ((W + 7) / 8) >= KF,
                  "msdssim needs grids of at least 81x81 (four scales, 11-tap filter on the coarsest)");
    const MsLayout l = ms_layout(workspace, N, H, W, C);
    DL4DS_REQUIRE(workspace_bytes >= l.total, "msdssim workspace too small");
    Stats* st = l.hdr.st;
    float *imgs = l.imgs, *grads = l.grads, *part = l.part, *part2 = l.part2, *gcp = l.gcp, *means = l.means, *gw = l.gw;
    const int NC = N * C;
    const size_t n0 = (size_t)N * H * W * C;
    static const Gauss gk = make_gauss();
    ProfScope ps(s, "msdssim", 0.0, 4.0 * (double)n0 * 12);
    run_minmax(s, y_true, y_pred, n0, l.hdr);
    auto ew = [](size_t n) { return (int)std::max<size_t>(1, std::min<size_t>(cdivz(n, 256), 8192)); };
    const float* xk[MS_SCALES];
    const float* qk[MS_SCALES];
    xk[0] = y_true; qk[0] = y_pred;
    // ---- pyramids
    for (int k = 1; k < MS_SCALES; ++k) {
        const size_t n = (size_t)N * l.d.H[k] * l.d.W[k] * C;
        float* xd = imgs + l.img_off[k];
        float* qd = xd + n;
        DL4DS_LAUNCH(ms_pool_kernel, dim3(ew(n)), dim3(256), 0, s, xk[k - 1], xd, N, l.d.H[k - 1], l.d.W[k - 1], l.d.H[k],
                           l.d.W[k], C, st, k == 1 ? 1 : 0);
        DL4DS_LAUNCH(ms_pool_kernel, dim3(ew(n)), dim3(256), 0, s, qk[k - 1], qd, N, l.d.H[k - 1], l.d.W[k - 1], l.d.H[k],
                           l.d.W[k], C, st, k == 1 ? 2 : 0);
        xk[k] = xd; qk[k] = qd;
    }
    // ---- per-scale (ssim, cs) means
    for (int k = 0; k < MS_SCALES; ++k) {
        const int Ho = l.g[k].Ho, Wo = l.g[k].Wo, txo = l.g[k].txo, tyo = l.g[k].tyo;
        DL4DS_LAUNCH(ms_ssim_kernel<0>, dim3(NC * txo * tyo), dim3(256), 0, s, xk[k], qk[k], k == 0 ? 1 : 0, 1, l.d.H[k], l.d.W[k],
                           C, Ho, Wo, txo, tyo, gk, st, nullptr, nullptr, nullptr, nullptr, nullptr, part);
        DL4DS_LAUNCH(ms_means_kernel, dim3(NC), dim3(64), 0, s, part, txo * tyo, NC, 1.f / ((float)Ho * (float)Wo),
                           means + (size_t)k * NC, means + (size_t)(MS_SCALES + k) * NC);
    }
    DL4DS_LAUNCH(ms_combine_kernel, dim3(1), dim3(256), 0, s, means, means + (size_t)MS_SCALES * NC, NC, weight, gw,
                       gw + (size_t)MS_SCALES * NC, loss_out, accumulate_loss);
    HIP_CHECK(hipGetLastError());
    if (!dpred) return;
    // ---- per-scale gradients (coarse to fine), pooled scales folded into the finer one
    float* dmu = l.maps;
    size_t gcp_total = 0;
    for (int k = MS_SCALES - 1; k >= 0; --k) {
        const int Hk = l.d.H[k], Wk = l.d.W[k], Ho = l.g[k].Ho, Wo = l.g[k].Wo, txo = l.g[k].txo, tyo = l.g[k].tyo;
        const size_t msz = (size_t)NC * Ho * Wo;
        float* da = dmu + msz;
        float* db = da + msz;
        DL4DS_LAUNCH(ms_ssim_kernel<1>, dim3(NC * txo * tyo), dim3(256), 0, s, xk[k], qk[k], k == 0 ? 1 : 0, 1, Hk, Wk, C, Ho, Wo,
                           txo, tyo, gk, st, gw + (size_t)k * NC, gw + (size_t)(MS_SCALES + k) * NC, dmu, da, db,
                           gcp + l.gcp_off[k] * 2);
        gcp_total = std::max(gcp_total, l.gcp_off[k] + (size_t)NC * txo * tyo);
        const int txi = cdiv(Wk, TS), tyi = cdiv(Hk, TS);
        float* gk_img = grads + l.grad_off[k];
        DL4DS_LAUNCH((ssim_bwd_kernel<false, false>), dim3(NC * txi * tyi), dim3(256), 0, s, xk[k], qk[k], k == 0 ? 1 : 0, Hk, Wk, C, Ho,
                           Wo, txi, tyi, gk, st, dmu, da, db, 1.f, gk_img, 0, nullptr, nullptr);
        if (k < MS_SCALES - 1) {
            const size_t n = (size_t)N * Hk * Wk * C;
            DL4DS_LAUNCH(ms_unpool_add_kernel, dim3(ew(n)), dim3(256), 0, s, gk_img, grads + l.grad_off[k + 1], N, Hk, Wk,
                               l.d.H[k + 1], l.d.W[k + 1], C);
        }
    }
    const int nba = (int)std::min<size_t>(cdivz(n0, 256), 2048);
    DL4DS_LAUNCH(ms_apply_kernel, dim3(nba), dim3(256), 0, s, grads + l.grad_off[0], dpred, n0, 1, part);
    DL4DS_LAUNCH(compact_partials_kernel<2>, dim3(COMPACT_G), dim3(256), 0, s, gcp, (int)gcp_total, part2);
    DL4DS_LAUNCH(ms_finish_kernel, dim3(1), dim3(256), 0, s, part, nba, part2, COMPACT_G, st, dpred);
    HIP_CHECK(hipGetLastError());
}

// ============================================================================================ post-hoc image metrics
// dl4ds/metrics.py:166-185,196-262 (compute_metrics) without the plotting: per test pair PSNR (tf.image.psnr with the
// joint dynamic range), SSIM (tf.image.ssim, no min-shift here), MAE, RMSE and Pearson correlation over the grid; per grid
// point RMSE, mean bias and Pearson correlation over the pairs.  Everything is a streaming pass over the two arrays:
//   pair sums   : blocks of one pair reduce (|d|, d^2, x, y, xy, x^2, y^2) -> fixed-order partials -> one thread per pair;
//   grid points : one thread per (pixel, channel) walks the pairs (coalesced across pixels);
//   SSIM        : the tile kernel of the multi-scale loss at scale 0 (separable Gaussian moments of the pivoted pixels, no min-shift)
//                 + its per-plane means.
namespace {
constexpr int MET_CHUNKS = 64, MET_K = 7;

__global__ void __launch_bounds__(256) met_pair_partial_kernel(const float* __restrict__ t, const float* __restrict__ p, size_t per,
                                                               float* __restrict__ partial) {
    __shared__ double red[MET_K][256];
    const int n = blockIdx.y;
    const size_t chunk = (per + gridDim.x - 1) / gridDim.x;
    const size_t e0 = (size_t)blockIdx.x * chunk, e1 = min(e0 + chunk, per);
    const float* a = t + (size_t)n * per;
    const float* b = p + (size_t)n * per;
    // the moments are those of (x - x0, y - y0), the pair's first elements (exact in double): Pearson does not see the shift, and the
    // float partials of data with a large mean (Kelvin, Pascal) would otherwise lose the covariance in cov = E[xy] - E[x] E[y]
    const double x0 = a[0], y0 = b[0];
    double s[MET_K] = {0, 0, 0, 0, 0, 0, 0};
    for (size_t e = e0 + threadIdx.x; e < e1; e += 256) {
        const double x = (double)a[e] - x0, y = (double)b[e] - y0, d = (double)b[e] - (double)a[e];
        s[0] += fabs(d); s[1] += d * d; s[2] += x; s[3] += y; s[4] += x * y; s[5] += x * x; s[6] += y * y;
    }
    for (int k = 0; k < MET_K; ++k) red[k][threadIdx.x] = s[k];
    block_tree_sum(red, threadIdx.x);
    if (threadIdx.x < MET_K) partial[((size_t)n * gridDim.x + blockIdx.x) * MET_K + threadIdx.x] = (float)red[threadIdx.x][0];
}
// out[n] = (mae, mse, pearson over the grid); a pair with a constant side has exact zero moments on that side (the shift above) and
// reports a correlation of 0
__global__ void met_pair_finish_kernel(const float* __restrict__ partial, int nchunks, int N, double per, float* __restrict__ out) {
    const int n = blockIdx.x * blockDim.x + threadIdx.x;
    if (n >= N) return;
    double s[MET_K] = {0, 0, 0, 0, 0, 0, 0};
    for (int c = 0; c < nchunks; ++c)
        for (int k = 0; k < MET_K; ++k) s[k] += (double)partial[((size_t)n * nchunks + c) * MET_K + k];
    const double mx = s[2] / per, my = s[3] / per;
    const double cov = s[4] / per - mx * my, vx = s[5] / per - mx * mx, vy = s[6] / per - my * my;
    out[n * 3 + 0] = (float)(s[0] / per);
    out[n * 3 + 1] = (float)(s[1] / per);
    out[n * 3 + 2] = (float)(cov / sqrt(fmax(vx * vy, 1e-300)));
}
// maps[0][e] = sqrt(mean_n d^2), maps[1][e] = mean_n d, maps[2][e] = pearson over the pairs
__global__ void met_grid_kernel(const float* __restrict__ t, const float* __restrict__ p, int N, size_t per, float* __restrict__ maps) {
    for (size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x; e < per; e += (size_t)gridDim.x * blockDim.x) {
        double sd = 0, sdd = 0, sx = 0, sy = 0, sxy = 0, sxx = 0, syy = 0;
        for (int n = 0; n < N; ++n) {
            const double x = t[(size_t)n * per + e], y = p[(size_t)n * per + e], d = y - x;
            sd += d; sdd += d * d; sx += x; sy += y; sxy += x * y; sxx += x * x; syy += y * y;
        }
        const double nn = (double)N, mx = sx / nn, my = sy / nn;
        const double cov = sxy / nn - mx * my, vx = sxx / nn - mx * mx, vy = syy / nn - my * my;
        maps[e] = (float)sqrt(sdd / nn);
        maps[per + e] = (float)(sd / nn);
        maps[2 * per + e] = (vx > 0 && vy > 0) ? (float)(cov / sqrt(vx * vy)) : NAN;
    }
}
__global__ void met_assemble_kernel(const float* __restrict__ pair3, const float* __restrict__ means, int N, int C, int has_ssim,
                                    const Stats* __restrict__ st, float* __restrict__ out, float* __restrict__ range) {
    const int n = blockIdx.x * blockDim.x + threadIdx.x;
    if (n == 0) {
        range[0] = fminf(st->minT, st->minP);
        range[1] = fmaxf(st->maxT, st->maxP);
    }
    if (n >= N) return;
    float sm = 0.f;
    for (int c = 0; c < C; ++c) sm += has_ssim ? means[n * C + c] : NAN;
    out[n * 4 + 0] = pair3[n * 3 + 0];
    out[n * 4 + 1] = pair3[n * 3 + 1];
    out[n * 4 + 2] = pair3[n * 3 + 2];
    out[n * 4 + 3] = sm / (float)C;
}

// has_ssim: the grid holds an 11x11 window
struct MetLayout { StatsScratch hdr; MapGeom g; bool has_ssim; float *partial, *pair3, *tile_part, *means; size_t total; };
MetLayout met_layout(void* ws, int N, int H, int W, int C) {
    Bump b(ws);
    MetLayout l;
    l.g = map_geom(H, W);
    l.has_ssim = l.g.Ho > 0 && l.g.Wo > 0;
    l.hdr = carve_stats(b);
    l.partial = b.take<float>((size_t)N * MET_CHUNKS * MET_K);
    l.pair3 = b.take<float>((size_t)N * 3);
    l.tile_part = b.take<float>(l.has_ssim ? (size_t)N * C * l.g.tyo * l.g.txo * 2 : 0);
    l.means = b.take<float>((size_t)2 * N * C);
    b.take<float>(3 * (size_t)H * W * C);      // unused: the size has always counted the three grid maps, which go to grid_out_dev
    l.total = b.o;
    return l;
}
}  // namespace

size_t metrics_workspace_bytes(int N, int H, int W, int C) { return met_layout(nullptr, N, H, W, C).total; }

// pair_out: [N][4] = (mae, mse, pearson, ssim)   grid_out: [3][H*W*C] = (rmse, mean bias, pearson)   stats_out: Stats
void image_metrics(hipStream_t s, const float* y_true, const float* y_pred, int N, int H, int W, int C, float* pair_out_dev,
                   float* grid_out_dev, float* range_out_dev, float* workspace, size_t workspace_bytes) {
    const MetLayout l = met_layout(workspace, N, H, W, C);
    DL4DS_REQUIRE(workspace_bytes >= l.total, "metrics workspace too small");
    const size_t per = (size_t)H * W * C, n0 = per * N;
    Stats* st = l.hdr.st;
    float *partial = l.partial, *pair3 = l.pair3, *tile_part = l.tile_part, *means = l.means;
    static const Gauss gk = make_gauss();
    ProfScope ps(s, "image_metrics", 0.0, 4.0 * (double)n0 * 6);
    run_minmax(s, y_true, y_pred, n0, l.hdr);
    DL4DS_LAUNCH(met_pair_partial_kernel, dim3(MET_CHUNKS, N), dim3(256), 0, s, y_true, y_pred, per, partial);
    DL4DS_LAUNCH(met_pair_finish_kernel, dim3(cdiv(N, 64)), dim3(64), 0, s, partial, MET_CHUNKS, N, (double)per, pair3);
    DL4DS_LAUNCH(met_grid_kernel, dim3((unsigned)std::min<size_t>(cdivz(per, 256), 4096)), dim3(256), 0, s, y_true, y_pred, N,
                       per, grid_out_dev);
    // SSIM per pair = mean over channels of the per-plane mean SSIM (needs an 11x11 window)
    const int NC = N * C;
    if (l.has_ssim) {
        const int Ho = l.g.Ho, Wo = l.g.Wo, txo = l.g.txo, tyo = l.g.tyo;
        DL4DS_LAUNCH(ms_ssim_kernel<0>, dim3(NC * txo * tyo), dim3(256), 0, s, y_true, y_pred, 1, 0, H, W, C, Ho, Wo, txo, tyo, gk, st,
                           nullptr, nullptr, nullptr, nullptr, nullptr, tile_part);
        DL4DS_LAUNCH(ms_means_kernel, dim3(NC), dim3(64), 0, s, tile_part, txo * tyo, NC, 1.f / ((float)Ho * (float)Wo), means,
                           means + NC);
    }
    HIP_CHECK(hipGetLastError());
    // assemble [N][4] and the range on the device (tiny)
    DL4DS_LAUNCH(met_assemble_kernel, dim3(cdiv(N, 64)), dim3(64), 0, s, pair3, means, N, C, l.has_ssim ? 1 : 0, st, pair_out_dev,
                       range_out_dev);
    HIP_CHECK(hipGetLastError());
}
