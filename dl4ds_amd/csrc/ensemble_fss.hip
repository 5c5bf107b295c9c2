// Neighbourhood verification of an MC-dropout ensemble as a PROBABILITY forecast: the member stack
// members[K][n] and the observation obs[n] are B whole samples of shape (H, W, C), each of the B*C planes is a field.  Per field,
// threshold and window size the five integer sums behind the Fractions Skill Score of the neighbourhood ensemble probability and
// the neighbourhood Brier score, per field and threshold the event counts of either side.
//
// A cell is VALID iff its observation and all K members are finite (NaN in obs is the masking mechanism).  Per valid cell and
// threshold t, on float32: o = [obs >= t], c = #{k : x_k >= t} (0 ... K); invalid cells have o = c = 0.  The window of size n at
// cell (i, j) is exactly fss.hip's: rows [i - n/2, i - n/2 + n), columns likewise, clipped to the field.  co / cf are the sums of
// o / c over it, co <= m = min(n, H) * min(n, W), cf <= K m.  Over ALL H*W cells D = sum (cf - K co)^2, F = sum cf^2, O = sum co^2;
// over the valid centre cells Fv = sum cf^2; over the centre cells with o = 1 X = sum cf.  E = sum o, Cs = sum c.  Integer
// arithmetic only: the 64-bit atomics give the same bits in any order and the result EQUALS an integer reference.
//
// Two kernels per chunk of fields and group of at most NB_TG thresholds.  This file owns the first, the validity bit-plane and
// the ensemble-only argument rules; the window walk, the chunk planner, the driver and the shared rules are neighbourhood.h's
// (DESIGN.md section 14a), of which fss.hip is the K = 1 case:
//  * efss_prefix_kernel: a wave per row, 64 cells per step, one lane per cell (stride C inside a plane).  The lane reads its
//    observation and walks the K member rows (adjacent lanes read adjacent cells of every row: coalesced), with up to NB_TG
//    threshold counters in registers; a non-finite value zeroes them.  MORE THAN NB_TG THRESHOLDS MEAN ANOTHER PASS OVER THE
//    STACK per further group (T = 9 ... 16: two reads of (K + 1) * 4 B per cell).  No per-cell count array goes to memory: the
//    observed indicator becomes a __ballot / popcount prefix as in fss.hip, the member count a wave-inclusive scan (__shfl_up, six
//    steps) whose lane 63 carries the wave-uniform total into the next segment.  Exclusive row prefixes P[0 .. W] of both sides
//    are stored as uint16 while K * W <= 65535 and as uint32 beyond; 32-bit prefixes may wrap (K * W can pass 2^32 on a single
//    long row): every difference the window walk takes is a window count < 2^31, exact modulo 2^32.  The validity of the row
//    is one ballot word per segment (a bit-plane).  E, Cs and n_valid are wave-uniform: one atomic per workgroup and counter.
//  * efss_window_kernel, per window size: nb_window_walk with the centre cell's o = P[j + 1] - P[j] and its validity bit, five sums.
// Fields go through in chunks sized by the same fixed workspace budget as fss.hip; the result does not depend on the chunking.
#include "neighbourhood.h"
#include "ops.h"

namespace {

constexpr int EFSS_NCNT = 2 * NB_TG + 1;               // per threshold: observed events, member events; + the valid count

// vbits[(f * H + row) * words + segment]: bit l = validity of cell 64 * segment + l
template <typename PT>
__global__ void __launch_bounds__(NB_THREADS) efss_prefix_kernel(const float* __restrict__ members, size_t stride, int K,
                                                                 const float* __restrict__ obs, int H, int W, int C, size_t field0,
                                                                 NbThresholds thr, int T, int t0, PT* __restrict__ prefix,
                                                                 unsigned long long* __restrict__ vbits,
                                                                 unsigned long long* __restrict__ cont,
                                                                 unsigned long long* __restrict__ valid_out) {
    __shared__ unsigned long long cnt[NB_WAVES][EFSS_NCNT];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int bands = (H + NB_PREFIX_ROWS - 1) / NB_PREFIX_ROWS;
    const size_t fl = blockIdx.x / (unsigned)bands;                       // field of the chunk
    const int band = (int)(blockIdx.x % (unsigned)bands);
    const size_t g = field0 + fl;                                         // field of the call
    const size_t base = nb_field_base(g, H, W, C);
    const size_t words = ((size_t)W + 63) / 64;                           // validity words per row
    const uint64_t upto = (2ull << lane) - 1ull;                          // lanes 0 ... lane
    const int r1 = min((band + 1) * NB_PREFIX_ROWS, H);
    unsigned long long nobs[NB_TG] = {}, nfc[NB_TG] = {}, nvalid = 0;
    for (int r = band * NB_PREFIX_ROWS + wave; r < r1; r += NB_WAVES) {
        uint32_t co[NB_TG] = {}, cf[NB_TG] = {};                      // carries of the earlier segments (wave-uniform)
        const size_t rowbase = base + (size_t)r * W * C;
        for (int j0 = 0; j0 < W; j0 += 64) {
            const int j = j0 + lane;
            const bool in = j < W;
            const size_t o = rowbase + (size_t)(in ? j : 0) * C;          // an idle lane reads the row's first cell and counts nothing
            const float yv = obs[o];
            bool fin = finite_bits(yv);
            uint32_t c[NB_TG] = {};
            const float* x = members + o;
#pragma unroll 4
            for (int m = 0; m < K; ++m) {
                const float xv = *x;
                x += stride;
                fin = fin && finite_bits(xv);
#pragma unroll
                for (int k = 0; k < NB_TG; ++k) c[k] += xv >= thr.t[k] ? 1u : 0u;
            }
            const bool ok = in && fin;
            const uint64_t mv = __ballot(ok);
            nvalid += (unsigned)__popcll(mv);
            if (lane == 0) vbits[(fl * (size_t)H + r) * words + (size_t)(j0 >> 6)] = mv;
#pragma unroll
            for (int k = 0; k < NB_TG; ++k) {
                if (k < thr.count) {                                      // uniform
                    const uint64_t mo = __ballot(ok && yv >= thr.t[k]);
                    uint32_t s = ok ? c[k] : 0u;                          // -> the inclusive scan of the wave
#pragma unroll
                    for (int d = 1; d < 64; d <<= 1) {
                        const uint32_t u = __shfl_up(s, d, 64);
                        if (lane >= d) s += u;
                    }
                    const uint32_t nf = (uint32_t)__builtin_amdgcn_readlane((int)s, 63);
                    if (in) {
                        const NbRows<PT> row = nb_prefix_rows(prefix, fl, thr.count, k, H, W, r);
                        if (j == 0) { row.o[0] = (PT)0; row.f[0] = (PT)0; }
                        row.o[j + 1] = (PT)(co[k] + (uint32_t)__popcll(mo & upto));
                        row.f[j + 1] = (PT)(cf[k] + s);
                    }
                    const uint32_t no = (uint32_t)__popcll(mo);
                    co[k] += no; cf[k] += nf;
                    nobs[k] += no; nfc[k] += nf;
                }
            }
        }
    }
    if (lane == 0) {
#pragma unroll
        for (int k = 0; k < NB_TG; ++k) { cnt[wave][2 * k] = nobs[k]; cnt[wave][2 * k + 1] = nfc[k]; }
        cnt[wave][2 * NB_TG] = nvalid;
    }
    __syncthreads();
    const int k = threadIdx.x;
    if (k <= thr.count) {
        if (k == thr.count) {
            unsigned long long v = 0;
            for (int w = 0; w < NB_WAVES; ++w) v += cnt[w][2 * NB_TG];
            if (valid_out && v) atomicAdd(valid_out + g, v);
        } else {
            unsigned long long ob = 0, fc = 0;
            for (int w = 0; w < NB_WAVES; ++w) { ob += cnt[w][2 * k]; fc += cnt[w][2 * k + 1]; }
            unsigned long long* c = cont + nb_cont_at(g, T, t0 + k, 2);
            if (ob) atomicAdd(c + 0, ob);                                 // E
            if (fc) atomicAdd(c + 1, fc);                                 // Cs
        }
    }
}

template <typename PT, bool WIDE>
__global__ void __launch_bounds__(NB_THREADS) efss_window_kernel(const PT* __restrict__ prefix,
                                                                 const unsigned long long* __restrict__ vbits, uint32_t K, int H,
                                                                 int W, int tcount, long long n, long long half, int band_rows,
                                                                 int nbands, size_t field0, int T, int t0, int S, int s,
                                                                 unsigned long long* __restrict__ sums) {
    nb_window_walk<PT, WIDE, true>(prefix, vbits, K, H, W, tcount, n, half, band_rows, nbands, field0, T, t0, S, s, sums);
}

// bytes of one field's validity bit-plane
size_t bits_per_field(int H, int W) { return (size_t)H * (((size_t)W + 63) / 64) * sizeof(unsigned long long); }

NbPlan plan(size_t K, size_t fields, int H, int W, int T) { return nb_plan(fields, H, W, T, nb_esize(K, W), bits_per_field(H, W)); }

}  // namespace

size_t ensemble_fss_workspace_bytes(size_t K, size_t B, int H, int W, int C, int T) {
    if (K == 0 || B == 0 || H <= 0 || W <= 0 || C <= 0 || T <= 0) return 0;
    return plan(K, B * (size_t)C, H, W, T).bytes();
}

void ensemble_fss_check_args(const float* members, size_t K, size_t n, size_t member_stride, const float* obs, size_t B, int H,
                             int W, int C, const float* thresholds, int T, const int* windows, int S, const long long* sums,
                             const long long* cont, const long long* valid) {
    DL4DS_REQUIRE(K >= 1 && K <= ENS_MAX_MEMBERS, "ensemble_fss: 1 <= K <= 256 members");
    DL4DS_REQUIRE(T >= 1 && T <= EXC_MAX_THRESHOLDS, "ensemble_fss: 1 <= T <= 16 thresholds");
    DL4DS_REQUIRE(S >= 1, "ensemble_fss: at least one window is needed");
    DL4DS_REQUIRE(H >= 1 && W >= 1 && C >= 1, "ensemble_fss: expected H, W, C >= 1");
    DL4DS_REQUIRE(members && obs && thresholds && windows && sums && cont && valid,
                  "ensemble_fss: null member stack, observation, thresholds, windows or output");
    DL4DS_REQUIRE((unsigned __int128)B * (unsigned)H * (unsigned)W * (unsigned)C == (unsigned __int128)n,
                  "ensemble_fss: n must be B whole samples of H * W * C cells");
    DL4DS_REQUIRE(member_stride >= n, "ensemble_fss: member stride smaller than the member");
    nb_check_args("ensemble_fss", "H*W*(K*m)^2", K, (unsigned __int128)B * (unsigned)C, H, W, thresholds, T, windows, S);
}

void ensemble_fss(hipStream_t st, const float* members, size_t K, size_t n, size_t member_stride, const float* obs, size_t B, int H,
                  int W, int C, const float* thresholds, int T, const int* windows, int S, long long* sums, long long* cont,
                  long long* valid, void* workspace, size_t workspace_bytes) {
    ensemble_fss_check_args(members, K, n, member_stride, obs, B, H, W, C, thresholds, T, windows, S, sums, cont, valid);
    if (B == 0) return;
    DL4DS_REQUIRE(workspace && workspace_bytes >= ensemble_fss_workspace_bytes(K, B, H, W, C, T), "ensemble_fss workspace too small");
    const size_t fields = B * (size_t)C;
    nb_enter(st, K, fields, W, T, S, 5, 2, sums, cont, valid, [&](auto pt, auto* us, auto* uc, auto* uv) {
        using PT = decltype(pt);
        const size_t chunk = plan(K, fields, H, W, T).fields;
        auto* vbits = static_cast<unsigned long long*>(workspace);        // the chunk's bit-planes first (8-byte aligned), then the prefixes
        PT* prefix = reinterpret_cast<PT*>(static_cast<char*>(workspace) + chunk * bits_per_field(H, W));
        nb_run<PT>(
            st, "ensemble_fss", K, fields, H, W, thresholds, T, windows, S, chunk, 10.0,
            [&](const NbGroup& g) {
                DL4DS_LAUNCH(efss_prefix_kernel<PT>, dim3(g.prefix_grid), dim3(NB_THREADS), 0, st, members, member_stride, (int)K, obs,
                             H, W, C, g.f0, g.thr, T, g.t0, prefix, vbits, uc, g.t0 == 0 ? uv : nullptr);
            },
            [&](const NbGroup& g, const NbWindow& w) {
                const auto kern = w.wide ? efss_window_kernel<PT, true> : efss_window_kernel<PT, false>;
                DL4DS_LAUNCH(kern, dim3(w.grid), dim3(NB_THREADS), 0, st, (const PT*)prefix, (const unsigned long long*)vbits,
                             (uint32_t)K, H, W, g.thr.count, w.n, w.half, w.band_rows, w.nbands, g.f0, T, g.t0, S, w.s, us);
            });
    });
}
