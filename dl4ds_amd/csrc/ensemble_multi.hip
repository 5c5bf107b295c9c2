// Multivariate verification of an MC-dropout ensemble against an observation: the energy score (Gneiting et al. 2008) and the
// variogram score (Scheuerer & Hamill 2015).  Both need all K members of a sample at once -- the member stack members[K][n]
// (row k at members + k * stride) that the ensemble entries hold on the device -- and both are sums of NON-NEGATIVE terms, reduced
// without floating-point atomics in an order that depends only on (K, sample shape, max_lag).  DESIGN.md section 25.
//
// An element is VALID iff its observation and all K members are finite and, with weights, its cell weight is > 0.
//
// Energy (ensemble_energy): the observation is row K of an (K + 1)-row matrix, and every output is the weighted squared distance
// of two rows: D_k = pair (k, K), G_kj = pair (k, j).  A workgroup owns one chunk of one sample; per tile of TE elements it
//   stages the K + 1 rows into LDS as tile[e][row] (invalid elements and elements past the chunk become all-zero with weight 0),
//   and every lane adds, for its element slice of the tile, the 4 x 4 block of pairs (rows 4 bi .. 4 bi + 3) x (rows 4 bj .. 4 bj + 3)
//   it owns onto 16 fp64 registers: two 16-byte LDS reads and 48 fp64 operations per element and block.
// K + 1 <= 129 rows make at most 33 row groups and 561 blocks (bi <= bj): up to three blocks per lane (NT); with fewer blocks than
// lanes the lanes of a block split the tile's elements (S slices) and are summed in slice order through LDS at the end.  The
// workgroup writes its sums to a workspace [B][chunks][K (K + 1) / 2]; a second launch adds the chunks in ascending order.
//
// Variogram (ensemble_variogram): a field is one H x W plane (fixed leading index and channel).  A workgroup owns a band of 8 rows
// of one field and walks its 32 x 8 tiles; a lane owns one base cell.  Per tile the observation and a validity mask are staged
// with a halo of max_lag cells left, right and below; the lags are taken in passes of up to 25, whose fp64 member sums live in
// registers; members are staged eight at a time and added in member order.  Per pass and lag the lanes' (o - e)^2, o, e are
// reduced by a fixed shuffle tree, the four waves in order, onto LDS accumulators of the band; a second launch adds fields and
// bands in ascending order.
#include "ensemble_common.h"
#include "prof.h"
#include <algorithm>

namespace {

// ------------------------------------------------------------------------------------------------------------------ energy
constexpr int EM_THREADS = 256;
constexpr int EM_RED_BYTES = EM_THREADS * 16 * 8;          // the slice reduction: 16 fp64 per lane

struct EnergyPlan {
    int M, MB, ntiles, NT, S, MS, TE;
    size_t npo, chunk, nchunks, lds;
};

// everything here is a function of (K, per) alone: the split of a sample never depends on B or on the sample's position
EnergyPlan energy_plan(size_t K, size_t per) {
    EnergyPlan p;
    p.M = (int)K + 1;
    p.MB = (p.M + 3) / 4;
    p.ntiles = p.MB * (p.MB + 1) / 2;
    p.NT = p.ntiles > EM_THREADS ? (p.ntiles + EM_THREADS - 1) / EM_THREADS : 1;
    p.S = p.ntiles >= EM_THREADS ? 1 : EM_THREADS / p.ntiles;
    p.MS = 4 * p.MB + ((4 * p.MB) % 8 == 0 ? 4 : 0);       // row stride of tile[e][.]: a multiple of 4 (16-byte reads), 4 mod 8
    p.TE = p.MS <= 48 ? 256 : p.MS <= 96 ? 128 : 64;
    p.npo = K * (K + 1) / 2;
    const size_t cap = p.M <= 33 ? 128 : p.M <= 65 ? 64 : 32;
    const size_t nt = cdivz(std::max<size_t>(per, 1), (size_t)p.TE);
    const size_t tiles_per = cdivz(nt, std::min(nt, cap));
    p.chunk = tiles_per * (size_t)p.TE;
    p.nchunks = cdivz(std::max<size_t>(per, 1), p.chunk);
    const size_t tile_bytes = (size_t)p.TE * p.MS * 4 + (size_t)p.TE * 8;
    p.lds = std::max<size_t>(tile_bytes, EM_RED_BYTES) + EM_THREADS * sizeof(long long);
    return p;
}

struct EnergyArgs {
    const float* members;
    const float* obs;
    const float* weight;
    size_t stride, per, chunk, npo;
    int K, M, MB, ntiles, S, MS, TE;
    double* part;                            // [B][nchunks][npo]
    long long* pcnt;                         // [B][nchunks]
};

// block t of the upper triangle (bi <= bj), rows of blocks in ascending bi
__device__ __forceinline__ void em_decode(int t, int MB, int& bi, int& bj) {
    bi = 0;
    int row = MB;
    while (t >= row) {
        t -= row;
        --row;
        ++bi;
    }
    bj = bi + t;
}

// rows r < c <= K -> position in [D_0 .. D_{K-1}, G_01, G_02, ..., G_{K-2,K-1}]
__device__ __forceinline__ size_t em_slot(int r, int c, int K) {
    return c == K ? (size_t)r : (size_t)K + (size_t)r * (size_t)(2 * K - r - 1) / 2 + (size_t)(c - r - 1);
}

__device__ __forceinline__ void em_write_block(double* out, const double (&acc)[16], int bi, int bj, int K) {
#pragma unroll
    for (int q = 0; q < 16; ++q) {
        const int r = 4 * bi + q / 4, c = 4 * bj + q % 4;
        if (r < c && c <= K) out[em_slot(r, c, K)] = acc[q];
    }
}

template <int NT>
__global__ void __launch_bounds__(EM_THREADS) ensemble_energy_kernel(EnergyArgs a) {
    extern __shared__ __align__(16) unsigned char em_lds[];
    const int TE = a.TE, MS = a.MS, M = a.M, K = a.K;
    float* tile = reinterpret_cast<float*>(em_lds);                          // [TE][MS]
    float* wl = tile + (size_t)TE * MS;                                      // [TE]
    int* flag = reinterpret_cast<int*>(wl + TE);                             // [TE]
    const int tid = threadIdx.x;
    const size_t b = blockIdx.y;
    const size_t e_begin = (size_t)blockIdx.x * a.chunk;
    const size_t e_end = min(a.per, e_begin + a.chunk);
    const float* obs = a.obs + b * a.per;
    const float* mem = a.members + b * a.per;

    // the lane's blocks and its element slice
    const int S = NT == 1 ? a.S : 1;
    const int s = NT == 1 ? tid % S : 0;
    int bi[NT], bj[NT];
    bool own[NT];
#pragma unroll
    for (int i = 0; i < NT; ++i) {
        const int t = NT == 1 ? tid / S : tid + i * EM_THREADS;
        own[i] = t < a.ntiles;
        em_decode(own[i] ? t : 0, a.MB, bi[i], bj[i]);
    }
    double acc[NT][16];
#pragma unroll
    for (int i = 0; i < NT; ++i) {
#pragma unroll
        for (int q = 0; q < 16; ++q) acc[i][q] = 0.0;
    }
    long long cnt = 0;

    for (int i = tid; i < TE * MS; i += EM_THREADS) tile[i] = 0.f;            // (the padding rows M .. 4 MB - 1 stay zero)
    const int te_shift = TE == 256 ? 8 : TE == 128 ? 7 : 6;

    for (size_t e0 = e_begin; e0 < e_end; e0 += (size_t)TE) {
        for (int e = tid; e < TE; e += EM_THREADS) {
            const size_t ge = e0 + e;
            float wv = 0.f;
            if (ge < e_end) wv = a.weight ? a.weight[ge] : 1.f;
            const bool ok = wv > 0.f;                                        // (false for NaN and past the chunk)
            wl[e] = ok ? wv : 0.f;
            flag[e] = ok ? 1 : 0;
        }
        __syncthreads();
        for (int i = tid; i < M * TE; i += EM_THREADS) {
            const int k = i >> te_shift, e = i & (TE - 1);
            const size_t ge = e0 + e;
            float v = 0.f;
            if (ge < e_end) v = k < K ? mem[(size_t)k * a.stride + ge] : obs[ge];
            if (!ens_finite(v)) {
                flag[e] = 0;                                                 // (every writer writes 0)
                v = 0.f;
            }
            tile[e * MS + k] = v;
        }
        __syncthreads();
        for (int i = tid; i < M * TE; i += EM_THREADS) {                      // an invalid element: all rows 0, weight 0
            const int k = i >> te_shift, e = i & (TE - 1);
            if (!flag[e]) tile[e * MS + k] = 0.f;
        }
        for (int e = tid; e < TE; e += EM_THREADS) {
            if (flag[e]) ++cnt;
            else wl[e] = 0.f;
        }
        __syncthreads();
        for (int e = s; e < TE; e += S) {
            const double w = (double)wl[e];
            const float* row = tile + e * MS;
#pragma unroll
            for (int i = 0; i < NT; ++i) {
                const float4 ra = *reinterpret_cast<const float4*>(row + 4 * bi[i]);
                const float4 rb = *reinterpret_cast<const float4*>(row + 4 * bj[i]);
                const double x[4] = {(double)ra.x, (double)ra.y, (double)ra.z, (double)ra.w};
                const double y[4] = {(double)rb.x, (double)rb.y, (double)rb.z, (double)rb.w};
#pragma unroll
                for (int q = 0; q < 16; ++q) {
                    const double d = x[q / 4] - y[q % 4];
                    acc[i][q] += d * d * w;
                }
            }
        }
        __syncthreads();
    }

    double* out = a.part + (b * gridDim.x + blockIdx.x) * a.npo;
    double* red = reinterpret_cast<double*>(em_lds);                          // [EM_THREADS][16] (the tile is done)
    long long* cred = reinterpret_cast<long long*>(em_lds + (a.TE * a.MS * 4 + a.TE * 8 > EM_RED_BYTES
                                                                 ? (size_t)a.TE * a.MS * 4 + (size_t)a.TE * 8
                                                                 : (size_t)EM_RED_BYTES));
    if constexpr (NT == 1) {
#pragma unroll
        for (int q = 0; q < 16; ++q) red[tid * 16 + q] = acc[0][q];
        cred[tid] = cnt;
        __syncthreads();
        for (int j = tid; j < a.ntiles * 16; j += EM_THREADS) {               // slices in ascending order
            const int t = j >> 4, q = j & 15;
            double sum = 0.0;
            for (int ss = 0; ss < S; ++ss) sum += red[(t * S + ss) * 16 + q];
            int tbi, tbj;
            em_decode(t, a.MB, tbi, tbj);
            const int r = 4 * tbi + q / 4, c = 4 * tbj + q % 4;
            if (r < c && c <= K) out[em_slot(r, c, K)] = sum;
        }
    } else {
        cred[tid] = cnt;
        __syncthreads();
#pragma unroll
        for (int i = 0; i < NT; ++i) {
            if (own[i]) em_write_block(out, acc[i], bi[i], bj[i], K);
        }
    }
    if (tid == 0) {
        long long total = 0;
        for (int i = 0; i < EM_THREADS; ++i) total += cred[i];
        a.pcnt[b * gridDim.x + blockIdx.x] = total;
    }
}

// dist[b][slot] = sum over the chunks of sample b, ascending;  nvalid[b] likewise
__global__ void __launch_bounds__(256) ensemble_energy_fold(const double* __restrict__ part, const long long* __restrict__ pcnt,
                                                            size_t B, size_t nchunks, size_t npo, double* __restrict__ dist,
                                                            long long* __restrict__ nvalid) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i < B * npo) {
        const size_t b = i / npo, slot = i % npo;
        double sum = 0.0;
        for (size_t c = 0; c < nchunks; ++c) sum += part[(b * nchunks + c) * npo + slot];
        dist[i] = sum;
    }
    if (nvalid && i < B) {
        long long total = 0;
        for (size_t c = 0; c < nchunks; ++c) total += pcnt[i * nchunks + c];
        nvalid[i] = total;
    }
}

// --------------------------------------------------------------------------------------------------------------- variogram
constexpr int VG_THREADS = 256, VG_TW = 32, VG_TH = 8;
constexpr int VG_MAX_LAG = 8, VG_MAX_LAGS = 98;
constexpr int VG_LC = 25;                                  // lags per pass: their member sums are 25 fp64 registers of the lane
constexpr int VG_MG = 8;                                   // members staged per barrier pair
constexpr int VG_MAX_CELLS = (VG_TW + 2 * VG_MAX_LAG) * (VG_TH + VG_MAX_LAG);      // 768: three per lane
constexpr int VG_CPL = VG_MAX_CELLS / VG_THREADS;
static_assert(VG_CPL * VG_THREADS == VG_MAX_CELLS, "whole cells per lane");

struct VarioArgs {
    const float* members;
    const float* obs;
    const float* weight;
    size_t stride, per;
    int K, H, W, C, Lm, nl, pitch, cells;
    double* psum;                            // [B][fields][bands][nl][3]
    long long* pcnt;                         // [B][fields][bands][nl]
    unsigned short lag[VG_MAX_LAGS];         // dy << 8 | (dx + 8)
};

// |d|^p for the three orders, each a single correctly rounded fp32 operation on |d|
template <int ORDER>
__device__ __forceinline__ float vg_pow(float d) {
    const float m = __builtin_fabsf(d);
    if constexpr (ORDER == 0) return __builtin_sqrtf(m);
    else if constexpr (ORDER == 1) return m;
    else return m * m;
}

template <int ORDER>
__global__ void __launch_bounds__(VG_THREADS) ensemble_variogram_kernel(VarioArgs a) {
    __shared__ float mt[VG_MG * VG_MAX_CELLS];               // the staged members' tiles
    __shared__ float ot[VG_MAX_CELLS];                       // the observation's tile
    __shared__ int mk[VG_MAX_CELLS];                         // 1: the cell lies in the field and is valid
    __shared__ double wred[4 * VG_LC * 3];
    __shared__ int wcnt[4 * VG_LC];
    __shared__ double accl[VG_MAX_LAGS * 3];                 // the band's sums
    __shared__ long long cntl[VG_MAX_LAGS];

    const int tid = threadIdx.x, wave = tid >> 6;
    const int K = a.K, H = a.H, W = a.W, C = a.C, Lm = a.Lm, nl = a.nl, pitch = a.pitch, cells = a.cells;
    const int band = blockIdx.x, field = blockIdx.y;
    const size_t b = blockIdx.z;
    const int pl = field / C, ch = field - pl * C;
    const int y0 = band * VG_TH;
    const float* obs = a.obs + b * a.per;
    const float* mem = a.members + b * a.per;
    const int base = (tid / VG_TW) * pitch + (tid % VG_TW) + Lm;
    const double dK = (double)K;

    for (int i = tid; i < nl * 3; i += VG_THREADS) accl[i] = 0.0;
    for (int i = tid; i < nl; i += VG_THREADS) cntl[i] = 0;

    for (int x0 = 0; x0 < W; x0 += VG_TW) {
        __syncthreads();                                    // the previous tile is done with ot, mk and mt
        long long coff[VG_CPL];                             // the lane's cells: element offset inside the sample, -1 outside the field
#pragma unroll
        for (int i = 0; i < VG_CPL; ++i) {
            const int c = tid + i * VG_THREADS;
            coff[i] = -1;
            if (c < cells) {
                const int cy = c / pitch, cx = c - cy * pitch;
                const int gy = y0 + cy, gx = x0 + cx - Lm;
                if (gy < H && gx >= 0 && gx < W) coff[i] = (long long)((((size_t)pl * H + gy) * W + gx) * C + ch);
                float ov = 0.f;
                bool ok = false;
                if (coff[i] >= 0) {
                    ov = obs[coff[i]];
                    ok = ens_finite(ov) && (!a.weight || a.weight[coff[i]] > 0.f);
                }
                ot[c] = ov;
                mk[c] = ok ? 1 : 0;
            }
        }
        for (int l0 = 0; l0 < nl; l0 += VG_LC) {
            double acc[VG_LC];
#pragma unroll
            for (int l = 0; l < VG_LC; ++l) acc[l] = 0.0;
            for (int g0 = 0; g0 < K; g0 += VG_MG) {
                __syncthreads();                            // mt is free (and, first time round, ot / mk are written)
                const int gm = min(VG_MG, K - g0);
#pragma unroll
                for (int i = 0; i < VG_CPL; ++i) {
                    const int c = tid + i * VG_THREADS;
                    if (c < cells) {
                        for (int m = 0; m < gm; ++m) {
                            float v = 0.f;
                            if (coff[i] >= 0) v = mem[(size_t)(g0 + m) * a.stride + coff[i]];
                            if (l0 == 0 && !ens_finite(v)) mk[c] = 0;         // (every writer writes 0; read after the passes' barrier)
                            mt[m * VG_MAX_CELLS + c] = v;
                        }
                    }
                }
                __syncthreads();
                for (int m = 0; m < gm; ++m) {              // member order
                    const float* t = mt + m * VG_MAX_CELLS + base;
                    const float vi = t[0];
#pragma unroll
                    for (int l = 0; l < VG_LC; ++l) {
                        if (l0 + l < nl) {                  // (uniform)
                            const int lg = a.lag[l0 + l];
                            const int off = (lg >> 8) * pitch + (lg & 255) - 8;
                            acc[l] += (double)vg_pow<ORDER>(vi - t[off]);
                        }
                    }
                }
            }
            // the pass's lags: per valid pair (o - e)^2, o, e; lanes by a fixed tree, then the waves in order
            const int mi = mk[base];
            const float oi = ot[base];
#pragma unroll
            for (int l = 0; l < VG_LC; ++l) {
                if (l0 + l < nl) {
                    const int lg = a.lag[l0 + l];
                    const int off = (lg >> 8) * pitch + (lg & 255) - 8;
                    const bool valid = mi && mk[base + off];
                    const float o = vg_pow<ORDER>(oi - ot[base + off]);
                    const double e = acc[l] / dK;
                    const double d = (double)o - e;
                    const double s0 = wave_sum(valid ? d * d : 0.0);
                    const double s1 = wave_sum(valid ? (double)o : 0.0);
                    const double s2 = wave_sum(valid ? e : 0.0);
                    const int n = (int)__popcll(__ballot(valid));
                    if ((tid & 63) == 0) {
                        double* w = wred + (wave * VG_LC + l) * 3;
                        w[0] = s0;
                        w[1] = s1;
                        w[2] = s2;
                        wcnt[wave * VG_LC + l] = n;
                    }
                }
            }
            __syncthreads();
            if (tid < VG_LC && l0 + tid < nl) {             // one lane per lag: nobody else touches its accumulators
                const int l = tid;
#pragma unroll
                for (int q = 0; q < 3; ++q) {
                    const double t = ((wred[(0 * VG_LC + l) * 3 + q] + wred[(1 * VG_LC + l) * 3 + q]) + wred[(2 * VG_LC + l) * 3 + q]) +
                                     wred[(3 * VG_LC + l) * 3 + q];
                    accl[(l0 + l) * 3 + q] += t;
                }
                cntl[l0 + l] += wcnt[l] + wcnt[VG_LC + l] + wcnt[2 * VG_LC + l] + wcnt[3 * VG_LC + l];
            }
            // (wred / wcnt are written again only after the next pass's barriers)
        }
    }
    __syncthreads();
    const size_t slot = (b * gridDim.y + field) * gridDim.x + band;
    for (int i = tid; i < nl * 3; i += VG_THREADS) a.psum[slot * nl * 3 + i] = accl[i];
    for (int i = tid; i < nl; i += VG_THREADS) a.pcnt[slot * nl + i] = cntl[i];
}

// per (sample, lag): the partial sums of its fields and bands, ascending
__global__ void __launch_bounds__(256) ensemble_variogram_fold(const double* __restrict__ psum, const long long* __restrict__ pcnt,
                                                               size_t B, size_t parts, size_t nl, long long* __restrict__ npairs,
                                                               double* __restrict__ sums) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= B * nl * 4) return;
    const size_t q = i & 3, l = (i >> 2) % nl, b = (i >> 2) / nl;
    if (q == 3) {
        long long total = 0;
        for (size_t p = 0; p < parts; ++p) total += pcnt[(b * parts + p) * nl + l];
        npairs[b * nl + l] = total;
    } else {
        double sum = 0.0;
        for (size_t p = 0; p < parts; ++p) sum += psum[((b * parts + p) * nl + l) * 3 + q];
        sums[(b * nl + l) * 3 + q] = sum;
    }
}

size_t align256(size_t v) { return (v + 255) / 256 * 256; }

}  // namespace

// ------------------------------------------------------------------------------------------------------------------ host
int variogram_lags(int max_lag, int* dydx, int* count) {
    DL4DS_REQUIRE(max_lag >= 1 && max_lag <= VG_MAX_LAG, "variogram_lags: 1 <= max_lag <= 8");
    int n = 0;
    for (int dy = 0; dy <= max_lag; ++dy) {
        for (int dx = dy == 0 ? 1 : -max_lag; dx <= max_lag; ++dx) {
            if (dy * dy + dx * dx > max_lag * max_lag) continue;
            if (dydx) {
                dydx[2 * n] = dy;
                dydx[2 * n + 1] = dx;
            }
            ++n;
        }
    }
    if (count) *count = n;
    return n;
}

void ensemble_energy_check(const float* members, size_t K, size_t n, size_t member_stride, const float* obs, size_t B,
                           const double* dist_out, const long long* nvalid_out) {
    DL4DS_REQUIRE(K >= 2 && K <= ENS_MULTI_MAX_MEMBERS, "ensemble_energy: 2 <= K <= 128 members");
    DL4DS_REQUIRE(B >= 1 && n % B == 0, "ensemble_energy: n must be B whole samples");
    DL4DS_REQUIRE(B <= 65535, "ensemble_energy: too many samples for one call");
    DL4DS_REQUIRE(members && obs && dist_out && nvalid_out, "ensemble_energy: null member stack, observation or output");
    DL4DS_REQUIRE(member_stride >= n, "ensemble_energy: member stride smaller than the member");
}

size_t ensemble_energy_workspace_bytes(size_t K, size_t n, size_t B) {
    const EnergyPlan p = energy_plan(K, n / B);
    return align256(B * p.nchunks * p.npo * sizeof(double)) + align256(B * p.nchunks * sizeof(long long));
}

void ensemble_energy(hipStream_t s, const float* members, size_t K, size_t n, size_t member_stride, const float* obs, size_t B,
                     const float* weight, double* dist_out, long long* nvalid_out, void* workspace, size_t workspace_bytes) {
    ensemble_energy_check(members, K, n, member_stride, obs, B, dist_out, nvalid_out);
    const size_t per = n / B;
    const EnergyPlan p = energy_plan(K, per);
    if (n == 0) {
        HIP_CHECK(hipMemsetAsync(dist_out, 0, B * p.npo * sizeof(double), s));
        HIP_CHECK(hipMemsetAsync(nvalid_out, 0, B * sizeof(long long), s));
        return;
    }
    DL4DS_REQUIRE(workspace && workspace_bytes >= ensemble_energy_workspace_bytes(K, n, B), "ensemble_energy: workspace too small");
    DL4DS_REQUIRE(p.nchunks <= 0x7fffffffull, "ensemble_energy: too many chunks for one launch");
    double* part = static_cast<double*>(workspace);
    long long* pcnt = reinterpret_cast<long long*>(static_cast<char*>(workspace) + align256(B * p.nchunks * p.npo * sizeof(double)));
    const EnergyArgs a{members, obs, weight, member_stride, per, p.chunk, p.npo, (int)K, p.M, p.MB, p.ntiles, p.S, p.MS, p.TE, part, pcnt};
    // 3 fp64 operations per pair and element (the padded blocks included in neither figure), one read of the stack
    ProfScope ps(s, "ensemble_energy", (double)n * 3.0 * (double)p.npo, (double)n * 4.0 * (double)(K + 1));
    const dim3 grid((unsigned)p.nchunks, (unsigned)B);
    if (p.NT == 1) DL4DS_LAUNCH((ensemble_energy_kernel<1>), grid, dim3(EM_THREADS), p.lds, s, a);
    else if (p.NT == 2) DL4DS_LAUNCH((ensemble_energy_kernel<2>), grid, dim3(EM_THREADS), p.lds, s, a);
    else DL4DS_LAUNCH((ensemble_energy_kernel<3>), grid, dim3(EM_THREADS), p.lds, s, a);
    const size_t items = std::max(B * p.npo, B);
    DL4DS_LAUNCH(ensemble_energy_fold, dim3((unsigned)cdivz(items, 256)), dim3(256), 0, s, part, pcnt, B, p.nchunks, p.npo, dist_out,
                 nvalid_out);
    HIP_CHECK(hipGetLastError());
}

void ensemble_variogram_check(const float* members, size_t K, size_t n, size_t member_stride, const float* obs, size_t B,
                              size_t planes, size_t H, size_t W, size_t C, int max_lag, int order_code, const long long* npairs_out,
                              const double* sums_out) {
    DL4DS_REQUIRE(K >= 2 && K <= ENS_MULTI_MAX_MEMBERS, "ensemble_variogram: 2 <= K <= 128 members");
    DL4DS_REQUIRE(max_lag >= 1 && max_lag <= VG_MAX_LAG, "ensemble_variogram: 1 <= max_lag <= 8");
    DL4DS_REQUIRE(order_code >= 0 && order_code <= 2, "ensemble_variogram: order code must be 0 (0.5), 1 (1) or 2 (2)");
    DL4DS_REQUIRE(B >= 1 && n % B == 0, "ensemble_variogram: n must be B whole samples");
    DL4DS_REQUIRE(B <= 65535, "ensemble_variogram: too many samples for one call");
    DL4DS_REQUIRE(H <= 0x3fffffffull && W <= 0x3fffffffull && C <= 0x3fffffffull && planes <= 0x3fffffffull,
                  "ensemble_variogram: a dimension of the sample is too large");
    DL4DS_REQUIRE(planes * H * W * C == n / B, "ensemble_variogram: planes * H * W * C must be one sample (n / B)");
    DL4DS_REQUIRE(members && obs && npairs_out && sums_out, "ensemble_variogram: null member stack, observation or output");
    DL4DS_REQUIRE(member_stride >= n, "ensemble_variogram: member stride smaller than the member");
    DL4DS_REQUIRE(n == 0 || planes * C <= 65535, "ensemble_variogram: too many fields (planes * C) for one launch");
}

size_t ensemble_variogram_workspace_bytes(size_t B, size_t planes, size_t H, size_t C, int max_lag) {
    const size_t nl = (size_t)variogram_lags(max_lag, nullptr, nullptr);
    const size_t parts = planes * C * cdivz(H, VG_TH);
    return align256(B * parts * nl * 3 * sizeof(double)) + align256(B * parts * nl * sizeof(long long));
}

void ensemble_variogram(hipStream_t s, const float* members, size_t K, size_t n, size_t member_stride, const float* obs, size_t B,
                        const float* weight, size_t planes, size_t H, size_t W, size_t C, int max_lag, int order_code,
                        long long* npairs_out, double* sums_out, void* workspace, size_t workspace_bytes) {
    ensemble_variogram_check(members, K, n, member_stride, obs, B, planes, H, W, C, max_lag, order_code, npairs_out, sums_out);
    int dydx[2 * VG_MAX_LAGS];
    const size_t nl = (size_t)variogram_lags(max_lag, dydx, nullptr);
    if (n == 0) {
        HIP_CHECK(hipMemsetAsync(npairs_out, 0, B * nl * sizeof(long long), s));
        HIP_CHECK(hipMemsetAsync(sums_out, 0, B * nl * 3 * sizeof(double), s));
        return;
    }
    DL4DS_REQUIRE(workspace && workspace_bytes >= ensemble_variogram_workspace_bytes(B, planes, H, C, max_lag),
                  "ensemble_variogram: workspace too small");
    const size_t bands = cdivz(H, VG_TH), fields = planes * C, parts = fields * bands;
    DL4DS_REQUIRE(bands <= 0x7fffffffull, "ensemble_variogram: too many rows for one launch");
    VarioArgs a{};
    a.members = members; a.obs = obs; a.weight = weight;
    a.stride = member_stride; a.per = n / B;
    a.K = (int)K; a.H = (int)H; a.W = (int)W; a.C = (int)C; a.Lm = max_lag; a.nl = (int)nl;
    a.pitch = VG_TW + 2 * max_lag;
    a.cells = a.pitch * (VG_TH + max_lag);
    a.psum = static_cast<double*>(workspace);
    a.pcnt = reinterpret_cast<long long*>(static_cast<char*>(workspace) + align256(B * parts * nl * 3 * sizeof(double)));
    for (size_t l = 0; l < nl; ++l) a.lag[l] = (unsigned short)((dydx[2 * l] << 8) | (dydx[2 * l + 1] + 8));
    // per pair and member a subtraction, the power and an fp64 addition; the stack once (the halo and the passes re-read it from cache)
    ProfScope ps(s, "ensemble_variogram", (double)n * (double)nl * 3.0 * (double)(K + 1), (double)n * 4.0 * (double)(K + 1));
    const dim3 grid((unsigned)bands, (unsigned)fields, (unsigned)B);
    if (order_code == 0) DL4DS_LAUNCH((ensemble_variogram_kernel<0>), grid, dim3(VG_THREADS), 0, s, a);
    else if (order_code == 1) DL4DS_LAUNCH((ensemble_variogram_kernel<1>), grid, dim3(VG_THREADS), 0, s, a);
    else DL4DS_LAUNCH((ensemble_variogram_kernel<2>), grid, dim3(VG_THREADS), 0, s, a);
    DL4DS_LAUNCH(ensemble_variogram_fold, dim3((unsigned)cdivz(B * nl * 4, 256)), dim3(256), 0, s, a.psum, a.pcnt, B, parts, nl,
                 npairs_out, sums_out);
    HIP_CHECK(hipGetLastError());
}
