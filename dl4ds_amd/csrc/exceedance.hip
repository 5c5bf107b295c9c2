// Exceedance-probability verification of an MC-dropout ensemble against an observation (the MCDropout / MCGaussianDropout /
// MCSpatialDropout layers of blocks.py:658-676 give the members; the reference leaves their verification to the user): at each of T
// thresholds the forecast probability of an element is c / K with c = #{k : x_k >= thr}, so the Brier score, its decomposition,
// the reliability diagram and the ROC curve are all functions of INTEGER sums.  One streaming read of the member stack
// members[K][n] plus the observation row obs[n], nothing sorted.  DESIGN.md section 17.
//
// Per (threshold t, element e), thr = thr[t] or, per cell, thr[t][e % per]:
//   valid iff obs[e], all K members and thr are finite;  o = [obs[e] >= thr], c = #{k : x_k >= thr} (fp32 comparisons, -0.0 == +0.0)
//   count[t][e] = c, or -1 where invalid (int16, overwritten)
//   sample_out[b][t][4] = n_valid, sum o, sum c, sum (c - K o)^2 over sample b (int64, overwritten)
//   cell_acc[t][4][per] += the same four per cell;  table[t][c][o] += 1   (64-bit integer atomics)
//
// Kernel: a lane owns VEC consecutive cells and walks `walk` consecutive samples (blockIdx.y picks the group of samples), for each
// sample the K rows: adjacent lanes read adjacent addresses of every row.  Thresholds and counters live in registers.
//   cell sums     32-bit registers of the lane for the whole walk, added onto memory once at its end
//   sample sums   the four sums of a wave packed into one 64-bit word, one shuffle tree per threshold, lane 0 adds them onto a
//                 32-bit LDS slot of the sample; every EXC_SB samples the workgroup flushes its slots with one atomic each
//   table         the two corner bins (c = 0, o = 0) and (c = K, o = 1), where a sharp forecast puts nearly every element, are
//                 counted by a ballot per wave (64 lanes on one LDS address would serialise); everything else is an LDS atomic on
//                 the workgroup's 32-bit histogram, flushed at the end with one 64-bit atomic per non-empty bin
// OVERFLOW RULE of the narrow partial sums (the host enforces it by bounding `walk`, exc_walk_limit):
//   lane, per cell:   n_valid and sum o share one register (16 bits each): walk <= 65535;  sum c <= 256 walk;
//                     sum (c - K o)^2 <= K^2 walk, which must stay below 2^32: walk <= (2^32 - 1) / K^2
//   wave, per sample: 64 VEC <= 256 elements: sum (c - K o)^2 <= 2^24 (25 bits), sum c <= 2^16 (17 bits), the counts <= 256 (10 bits)
//   workgroup:        a sample's LDS slot <= 1024 * 65536 = 2^26;  a histogram bin <= 1024 walk < 2^26
// Integer arithmetic only: the result does not depend on the order of the atomics, the grouping of samples or the batch size.
#include "ensemble_common.h"
#include "prof.h"
#include <algorithm>

namespace {

constexpr int EXC_THREADS = 256;
constexpr int EXC_SB = 8;                  // samples between two flushes of the per-sample LDS slots
constexpr size_t EXC_TARGET_BLOCKS = 1024; // samples are split over workgroups until the grid has about this many

struct ExcArgs {
    const float* members;
    const float* obs;
    const float* thr;
    size_t stride, per;
    int K, T;
    unsigned B, walk;
    short* count;                          // [T][n]
    unsigned long long* sample_out;        // [B][T][4]
    unsigned long long* cell_acc;          // [T][4][per]
    unsigned long long* table;             // [T][K + 1][2]
};

// TP: thresholds held in registers (T <= TP), VEC: consecutive cells per lane, CELL: thresholds per cell ([T][per]) or one per t
template <int TP, int VEC, bool CELL>
__global__ void __launch_bounds__(EXC_THREADS) ensemble_exceedance_kernel(ExcArgs a) {
    extern __shared__ unsigned exc_lds[];                       // hist [T][K + 1][2], then slots [EXC_SB][T][4]
    const int K = a.K, T = a.T, K1 = K + 1;
    const int bins = T * K1 * 2, nslots = EXC_SB * T * 4;
    unsigned* hist = exc_lds;
    unsigned* slots = exc_lds + bins;
    for (int i = threadIdx.x; i < bins + nslots; i += EXC_THREADS) exc_lds[i] = 0u;
    __syncthreads();

    const size_t per = a.per;
    const size_t cell0 = ((size_t)blockIdx.x * EXC_THREADS + threadIdx.x) * VEC;
    const bool act = cell0 < per;                               // (per % VEC == 0: all VEC cells or none)
    const size_t cc = act ? cell0 : 0;                          // an idle lane reads the first cells and counts nothing
    const unsigned b0 = blockIdx.y * a.walk;
    const unsigned b1 = min(a.B, b0 + a.walk);
    const size_t n = (size_t)a.B * per;

    float thr[TP][VEC];                                         // NaN: no threshold here (t >= T, or not finite)
#pragma unroll
    for (int t = 0; t < TP; ++t) {
#pragma unroll
        for (int c = 0; c < VEC; ++c) {
            float v = __builtin_nanf("");
            if (t < T) v = CELL ? a.thr[(size_t)t * per + cc + c] : a.thr[t];
            thr[t][c] = ens_finite(v) ? v : __builtin_nanf("");
        }
    }
    unsigned s_no[TP][VEC], s_c[TP][VEC], s_q[TP][VEC];         // n_valid | sum o << 16, sum c, sum (c - K o)^2 of the lane's cells
    unsigned corner0[TP], corner1[TP];                          // the wave's counts of the bins (0, 0) and (K, 1)
#pragma unroll
    for (int t = 0; t < TP; ++t) {
        corner0[t] = corner1[t] = 0u;
#pragma unroll
        for (int c = 0; c < VEC; ++c) s_no[t][c] = s_c[t][c] = s_q[t][c] = 0u;
    }

    for (unsigned b = b0; b < b1; ++b) {
        const size_t e0 = (size_t)b * per + cc;
        float y[VEC];
        ens_load_vec<VEC>(a.obs + e0, y);
        bool fin[VEC];
        int cnt[TP][VEC];
#pragma unroll
        for (int c = 0; c < VEC; ++c) fin[c] = ens_finite(y[c]);
#pragma unroll
        for (int t = 0; t < TP; ++t) {
#pragma unroll
            for (int c = 0; c < VEC; ++c) cnt[t][c] = 0;
        }
        const float* row = a.members + e0;
#pragma unroll 4
        for (int k = 0; k < K; ++k) {
            float x[VEC];
            ens_load_vec<VEC>(row, x);
            row += a.stride;
#pragma unroll
            for (int c = 0; c < VEC; ++c) {
                fin[c] = fin[c] && ens_finite(x[c]);
#pragma unroll
                for (int t = 0; t < TP; ++t) cnt[t][c] += x[c] >= thr[t][c] ? 1 : 0;
            }
        }
        const unsigned slot = ((b - b0) % EXC_SB) * (unsigned)T * 4u;
#pragma unroll
        for (int t = 0; t < TP; ++t) {
            if (t < T) {                                        // (uniform)
                unsigned long long pk = 0ull;
                short res[VEC];
#pragma unroll
                for (int c = 0; c < VEC; ++c) {
                    const bool valid = act && fin[c] && thr[t][c] == thr[t][c];
                    const int o = y[c] >= thr[t][c] ? 1 : 0;
                    const int cn = cnt[t][c];
                    const int d = cn - K * o;
                    const unsigned q = (unsigned)(d * d);
                    res[c] = valid ? (short)cn : (short)-1;
                    if (valid) {
                        s_no[t][c] += 1u | ((unsigned)o << 16);
                        s_c[t][c] += (unsigned)cn;
                        s_q[t][c] += q;
                        pk += (unsigned long long)q | ((unsigned long long)cn << 25) | ((unsigned long long)o << 42) | (1ull << 52);
                    }
                    if (a.table) {
                        const bool z0 = valid && cn == 0 && o == 0, z1 = valid && cn == K && o == 1;
                        corner0[t] += (unsigned)__popcll(__ballot(z0));
                        corner1[t] += (unsigned)__popcll(__ballot(z1));
                        if (valid && !z0 && !z1) atomicAdd(&hist[(t * K1 + cn) * 2 + o], 1u);
                    }
                }
                if (a.count && act) ens_store<VEC, short>(a.count + (size_t)t * n + e0, res);
                if (a.sample_out) {
                    pk = wave_sum_u64(pk);
                    if ((threadIdx.x & 63) == 0 && pk) {
                        atomicAdd(&slots[slot + t * 4 + 0], (unsigned)(pk >> 52));
                        atomicAdd(&slots[slot + t * 4 + 1], (unsigned)(pk >> 42) & 0x3ffu);
                        atomicAdd(&slots[slot + t * 4 + 2], (unsigned)(pk >> 25) & 0x1ffffu);
                        atomicAdd(&slots[slot + t * 4 + 3], (unsigned)pk & 0x1ffffffu);
                    }
                }
            }
        }
        if (a.sample_out && ((b - b0 + 1) % EXC_SB == 0 || b + 1 == b1)) {        // (uniform: every lane walks the same samples)
            __syncthreads();
            const unsigned first = b - (b - b0) % EXC_SB;                          // the sample of slot 0
            const int used = (int)(b - first + 1) * T * 4;
            for (int i = threadIdx.x; i < used; i += EXC_THREADS) {
                const unsigned v = slots[i];
                if (v) atomicAdd(&a.sample_out[(size_t)first * T * 4 + i], (unsigned long long)v);
                slots[i] = 0u;
            }
            __syncthreads();
        }
    }

    if (a.table) {
        if ((threadIdx.x & 63) == 0) {
#pragma unroll
            for (int t = 0; t < TP; ++t) {
                if (t < T) {
                    if (corner0[t]) atomicAdd(&hist[(t * K1) * 2], corner0[t]);
                    if (corner1[t]) atomicAdd(&hist[(t * K1 + K) * 2 + 1], corner1[t]);
                }
            }
        }
        __syncthreads();
        for (int i = threadIdx.x; i < bins; i += EXC_THREADS) {
            const unsigned h = hist[i];
            if (h) atomicAdd(&a.table[i], (unsigned long long)h);
        }
    }
    if (a.cell_acc && act) {
#pragma unroll
        for (int t = 0; t < TP; ++t) {
            if (t < T) {
#pragma unroll
                for (int c = 0; c < VEC; ++c) {
                    const unsigned no = s_no[t][c];
                    if (!no) continue;                          // no valid sample of this cell in this walk: all four are 0
                    unsigned long long* p = a.cell_acc + (size_t)t * 4 * per + cell0 + c;
                    atomicAdd(p, (unsigned long long)(no & 0xffffu));
                    atomicAdd(p + per, (unsigned long long)(no >> 16));
                    atomicAdd(p + 2 * per, (unsigned long long)s_c[t][c]);
                    atomicAdd(p + 3 * per, (unsigned long long)s_q[t][c]);
                }
            }
        }
    }
}

template <int TP, int VEC, bool CELL>
void exc_launch(hipStream_t s, const ExcArgs& a) {
    if constexpr (VEC > 1) {
        // vector loads / stores need whole, aligned groups in every row and sample; otherwise one cell per lane (still coalesced)
        auto aligned = [](const void* p, size_t bytes) { return ((uintptr_t)p % bytes) == 0; };
        // (thresholds are read one value at a time: their alignment does not matter)
        if (a.per % VEC || a.stride % VEC || !aligned(a.members, 4 * VEC) || !aligned(a.obs, 4 * VEC) ||
            (a.count && !aligned(a.count, 2 * VEC)))
            return exc_launch<TP, 1, CELL>(s, a);
    }
    const size_t bx = cdivz(a.per, (size_t)EXC_THREADS * VEC);
    DL4DS_REQUIRE(bx <= 0x7fffffffull, "ensemble_exceedance: too many cells for one launch");
    // samples per workgroup: all of them when the cells alone fill the chip, fewer for small fields; never more than the
    // overflow rule allows
    const size_t limit = exc_walk_limit((size_t)a.K);
    size_t groups = std::min<size_t>(a.B, std::max<size_t>(1, EXC_TARGET_BLOCKS / bx));
    size_t walk = std::min(cdivz(a.B, groups), limit);
    groups = cdivz(a.B, walk);
    DL4DS_REQUIRE(groups <= 65535, "ensemble_exceedance: too many samples for one call");
    ExcArgs k = a;
    k.walk = (unsigned)walk;
    const size_t lds = ((size_t)a.T * (a.K + 1) * 2 + (size_t)EXC_SB * a.T * 4) * sizeof(unsigned);      // <= 34.9 KB
    DL4DS_LAUNCH((ensemble_exceedance_kernel<TP, VEC, CELL>), dim3((unsigned)bx, (unsigned)groups), dim3(EXC_THREADS), lds, s, k);
}

template <bool CELL>
void exc_dispatch(hipStream_t s, const ExcArgs& a) {
    // the member loop compares against all TP thresholds: TP stays close to T (at most T + 3), the cells per lane follow the registers
    if (a.T <= 1) exc_launch<1, 4, CELL>(s, a);
    else if (a.T <= 2) exc_launch<2, 4, CELL>(s, a);
    else if (a.T <= 4) exc_launch<4, 4, CELL>(s, a);
    else if (a.T <= 6) exc_launch<6, 2, CELL>(s, a);
    else if (a.T <= 8) exc_launch<8, 2, CELL>(s, a);
    else if (a.T <= 12) exc_launch<12, 1, CELL>(s, a);
    else exc_launch<16, 1, CELL>(s, a);
}

}  // namespace

size_t exc_walk_limit(size_t K) {
    const size_t k2 = std::max<size_t>(K, 1) * std::max<size_t>(K, 1);
    return std::min<size_t>(65535, 0xffffffffull / k2);
}

void ensemble_exceedance(hipStream_t s, const float* members, size_t K, size_t n, size_t member_stride, const float* obs, size_t B,
                         const float* thr, int T, int thr_per_cell, short* count, long long* sample_out, long long* cell_acc,
                         unsigned long long* table) {
    DL4DS_REQUIRE(K >= 1 && K <= ENS_MAX_MEMBERS, "ensemble_exceedance: 1 <= K <= 256 members");
    DL4DS_REQUIRE(T >= 1 && T <= EXC_MAX_THRESHOLDS, "ensemble_exceedance: 1 <= T <= 16 thresholds");
    if (n == 0) return;
    DL4DS_REQUIRE(B >= 1 && n % B == 0, "ensemble_exceedance: n must be B whole samples");
    DL4DS_REQUIRE(B <= 0x7fffffffull, "ensemble_exceedance: too many samples for one call");
    DL4DS_REQUIRE(members && obs && thr, "ensemble_exceedance: null member stack, observation or thresholds");
    DL4DS_REQUIRE(member_stride >= n, "ensemble_exceedance: member stride smaller than the member");
    if (sample_out) HIP_CHECK(hipMemsetAsync(sample_out, 0, B * (size_t)T * 4 * sizeof(long long), s));
    const ExcArgs a{members, obs, thr, member_stride, n / B, (int)K, T, (unsigned)B, 0u, count,
                    reinterpret_cast<unsigned long long*>(sample_out), reinterpret_cast<unsigned long long*>(cell_acc), table};
    ProfScope ps(s, "ensemble_exceedance", (double)n * K * (2.0 * T + 1.0), (double)n * (4.0 * (double)(K + 1) + (count ? 2.0 * T : 0.0)));
    if (thr_per_cell) exc_dispatch<true>(s, a);
    else exc_dispatch<false>(s, a);
    HIP_CHECK(hipGetLastError());
}
