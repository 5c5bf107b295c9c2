// Pixel losses of dl4ds/losses.py (mae :5-11, mse :14-20, dssim :23-55 and the 0.8/0.2, 0.6/0.2/0.2
// mixes :58-89) and Keras BinaryCrossentropy(from_logits=False) (cgan.py:546-549,567-571), each fused
// with its gradient w.r.t. the prediction.  Wave reductions -> one partial per block -> finish kernel.
//
// Per-grid-cell loss weights (masks, area weights): loss_forward_backward_weighted.  The contract:
//   * w is float32, finite, >= 0, on the output grid: w_batch maps of (H, W, w_channels), w_channels in {1, C}; w_batch divides N
//     and sample row r of the (N, H, W, C) batch uses map r / (N / w_batch) -- w_batch == 1: one shared map, w_batch == N: one
//     map per sample (patch training), w_batch == N / nmul: one map per sample of a spatio-temporal output of nmul frames.
//   * with d = p - t and sums over ALL N*H*W*C entries (w broadcast):  mae_w = sum w|d| / sum w,  mse_w = sum w d^2 / sum w,
//     gradients accordingly (0 at d == 0, as in the unweighted kernel); w == const > 0 reproduces the unweighted loss.
//   * exclusion: an entry with w == 0 is left out by SELECTION, not multiplied by 0 -- neither t nor p there enters a sum and its
//     gradient is exactly +0.0, also where t is NaN or Inf.  This holds for the MAE and MSE terms of every kind.
//   * sum w == 0 (a patch entirely over masked cells): loss 0, dpred all zeros, no NaN.
//   * dssim kinds: the SSIM map over the VALID 11x11 windows gets window weights omega = G * w (G: the Gaussian of the moments, so
//     omega == 1 where w == 1); term = sum omega (1 - s)/2 / sum omega over samples, windows and channels; windows with
//     omega == 0 are excluded by selection.  Dynamic range and positivity shift stay those of the WHOLE arrays (minmax_kernel is
//     unchanged), so y_true must be finite everywhere for these kinds.  The mixes keep 0.8/0.2 and 0.6/0.2/0.2 over the weighted terms.
//   * msdssim kinds with weights are refused.
// Passes: weight_sum_kernel + finish (fixed order, double in the finish) leave 1 / sum w in a device scalar that the pixel kernel and
// its finish read -- no host read-back, no synchronisation; all reductions have a fixed order (same inputs, same bits).
#include "ops.h"
#include "prof.h"
#include <algorithm>

namespace {

__device__ __forceinline__ float block_sum(float v, float* red) {
    v = wave_sum(v);
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    if (lane == 0) red[wv] = v;
    __syncthreads();
    float s = 0.f;
    if (threadIdx.x == 0) for (int k = 0; k < (int)(blockDim.x >> 6); ++k) s += red[k];
    __syncthreads();
    return s;   // valid in thread 0
}

// partial[2*b] = sum |d| ; partial[2*b+1] = sum d^2 ; dpred (+)= ga*sign(d) + gs*2*d
__global__ void __launch_bounds__(256) pixel_loss_kernel(const float* __restrict__ t, const float* __restrict__ p,
                                                         float* __restrict__ dp, size_t n, float ga, float gs,
                                                         int accumulate, float* __restrict__ partial) {
    __shared__ float red[4];
    float sa = 0.f, ss = 0.f;
    for (size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x; e < n; e += (size_t)gridDim.x * blockDim.x) {
        const float d = p[e] - t[e];
        sa += fabsf(d);
        ss += d * d;
        if (dp) {
            const float sg = (d > 0.f) ? 1.f : ((d < 0.f) ? -1.f : 0.f);
            const float g = ga * sg + gs * 2.f * d;
            dp[e] = accumulate ? dp[e] + g : g;
        }
    }
    const float a = block_sum(sa, red);
    const float b = block_sum(ss, red);
    if (threadIdx.x == 0) { partial[2 * blockIdx.x] = a; partial[2 * blockIdx.x + 1] = b; }
}

// loss_out[0] (+)= wa*mean|d| + ws*mean d^2
__global__ void pixel_loss_finish_kernel(const float* __restrict__ partial, int nb, float wa, float ws, float inv_n,
                                         float* loss_out, int accumulate) {
    // one wave: lane-strided partial sums, then a fixed butterfly (deterministic; the single-thread chain took 53 us)
    float a = 0.f, b = 0.f;
    for (int k = threadIdx.x; k < nb; k += 64) { a += partial[2 * k]; b += partial[2 * k + 1]; }
    a = wave_sum(a);
    b = wave_sum(b);
    if (threadIdx.x == 0 && blockIdx.x == 0) {
        const float v = wa * a * inv_n + ws * b * inv_n;
        loss_out[0] = accumulate ? loss_out[0] + v : v;
    }
}

// ---- weighted forms
// How an element index maps to its weight: element e = (n, r) with r < per = H*W*C; weight = w[(n / rep) * wper + (cw == C ? r : r / C)]
struct WIndex {
    unsigned per, wper, C, cw;      // elements per sample, weights per map, channels of the batch / of the map
    unsigned wb, rep;               // maps, samples per map (N / wb)
    unsigned stride_n, stride_r;    // one grid stride (gridDim.x * 256 elements) = stride_n samples + stride_r elements
};

// partial[b] = sum of this block's share of the weight array (or of any float array)
__global__ void __launch_bounds__(256) weight_sum_kernel(const float* __restrict__ w, size_t n, float* __restrict__ partial) {
    __shared__ float red[4];
    float s = 0.f;
    for (size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x; e < n; e += (size_t)gridDim.x * blockDim.x) s += w[e];
    const float a = block_sum(s, red);
    if (threadIdx.x == 0) partial[blockIdx.x] = a;
}
// inv_out[0] = 1 / (mult * sum partial), or 0 when the sum is 0 (every later kernel then yields 0); double, fixed tree
__global__ void __launch_bounds__(256) weight_sum_finish_kernel(const float* __restrict__ partial, int nb, double mult,
                                                                float* __restrict__ inv_out) {
    __shared__ double red[256];
    double a = 0.0;
    for (int k = threadIdx.x; k < nb; k += 256) a += (double)partial[k];
    red[threadIdx.x] = a;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        const double tot = red[0] * mult;
        inv_out[0] = tot > 0.0 ? (float)(1.0 / tot) : 0.f;
    }
}

// partial[2*b] = sum w|d| ; partial[2*b+1] = sum w d^2 over the entries with w > 0 ; dpred (+)= w / sum w * (ga*sign(d) + gs*2*d), +0.0 where
// w == 0.  The sample / in-sample position of a block's 256 elements is carried along the grid-stride loop (one 64-bit division per
// block, none per element); a division by C (32-bit) remains only for a one-channel map over a multi-channel batch.
__global__ void __launch_bounds__(256) pixel_loss_w_kernel(const float* __restrict__ t, const float* __restrict__ p,
                                                           const float* __restrict__ w, float* __restrict__ dp, size_t n,
                                                           WIndex ix, float ga, float gs, const float* __restrict__ inv_sw_dev,
                                                           int accumulate, float* __restrict__ partial) {
    __shared__ float red[4];
    const float inv_sw = inv_sw_dev[0];
    size_t e0 = (size_t)blockIdx.x * 256;
    unsigned n0 = (unsigned)(e0 / ix.per);
    unsigned r0 = (unsigned)(e0 - (size_t)n0 * ix.per);
    float sa = 0.f, ss = 0.f;
    for (; e0 < n; e0 += (size_t)gridDim.x * 256) {
        const size_t e = e0 + threadIdx.x;
        unsigned r = r0 + threadIdx.x, sn = n0;
        if (ix.per >= 256u) {
            if (r >= ix.per) { r -= ix.per; ++sn; }
        } else {
            sn += r / ix.per; r %= ix.per;
        }
        if (e < n) {
            const unsigned m = ix.wb == 1u ? 0u : (ix.rep == 1u ? sn : sn / ix.rep);
            const unsigned q = ix.cw == ix.C ? r : r / ix.C;
            // all three loads are issued together (a masked t may be NaN: it is read but never used)
            const float wv = w[(size_t)m * ix.wper + q], pv = p[e], tv = t[e];
            float g = 0.f;
            if (wv > 0.f) {
                const float d = pv - tv;
                sa += wv * fabsf(d);
                ss += wv * d * d;
                const float sg = (d > 0.f) ? 1.f : ((d < 0.f) ? -1.f : 0.f);
                g = (wv * inv_sw) * (ga * sg + gs * 2.f * d);
            }
            if (dp) dp[e] = accumulate ? dp[e] + g : g;
        }
        n0 += ix.stride_n; r0 += ix.stride_r;
        if (r0 >= ix.per) { r0 -= ix.per; ++n0; }
    }
    const float a = block_sum(sa, red);
    const float b = block_sum(ss, red);
    if (threadIdx.x == 0) { partial[2 * blockIdx.x] = a; partial[2 * blockIdx.x + 1] = b; }
}

// loss_out[0] = (wa * sum w|d| + ws * sum w d^2) / sum w
__global__ void pixel_loss_w_finish_kernel(const float* __restrict__ partial, int nb, float wa, float ws,
                                           const float* __restrict__ inv_sw_dev, float* loss_out) {
    float a = 0.f, b = 0.f;
    for (int k = threadIdx.x; k < nb; k += 64) { a += partial[2 * k]; b += partial[2 * k + 1]; }
    a = wave_sum(a);
    b = wave_sum(b);
    if (threadIdx.x == 0 && blockIdx.x == 0) {
        const float inv_sw = inv_sw_dev[0];
        loss_out[0] = wa * a * inv_sw + ws * b * inv_sw;
    }
}

__global__ void __launch_bounds__(256) bce_kernel(const float* __restrict__ p, float label, int n, float scale,
                                                  float* loss_out, float* __restrict__ dp, int accumulate_loss) {
    __shared__ float red[4];
    const float eps = 1e-7f;
    float s = 0.f;
    for (int e = threadIdx.x; e < n; e += blockDim.x) {
        const float pr = p[e];
        const float pc = fminf(fmaxf(pr, eps), 1.f - eps);
        s += -(label * logf(pc) + (1.f - label) * logf(1.f - pc));
        if (dp) {
            // d/dp of the clipped form: zero outside [eps, 1-eps]
            float g = 0.f;
            if (pr >= eps && pr <= 1.f - eps) g = -(label / pc - (1.f - label) / (1.f - pc));
            dp[e] = scale * g / (float)n;
        }
    }
    const float tot = block_sum(s, red);
    if (threadIdx.x == 0) {
        const float v = scale * tot / (float)n;
        loss_out[0] = accumulate_loss ? loss_out[0] + v : v;
    }
}

int loss_blocks(size_t n) { return (int)std::max<size_t>(1, std::min<size_t>(cdivz(n, 256 * 8), 1024)); }

}  // namespace

void dssim_forward_backward(hipStream_t s, const float* y_true, const float* y_pred, float* dpred, int N, int H, int W,
                            int C, float weight, float* loss_out, int accumulate_loss, float* workspace,
                            size_t workspace_bytes);
size_t dssim_workspace_bytes(int N, int H, int W, int C);
void msdssim_forward_backward(hipStream_t s, const float* y_true, const float* y_pred, float* dpred, int N, int H, int W,
                              int C, float weight, float* loss_out, int accumulate_loss, float* workspace,
                              size_t workspace_bytes);
size_t msdssim_workspace_bytes(int N, int H, int W, int C);

static void loss_weights(int kind, float& wd, float& wa, float& ws, float& wm) {
    wd = wa = ws = wm = 0.f;
    switch (kind) {
        case LOSS_MAE: wa = 1.f; break;
        case LOSS_MSE: ws = 1.f; break;
        case LOSS_DSSIM: wd = 1.f; break;
        case LOSS_DSSIM_MAE: wd = 0.8f; wa = 0.2f; break;
        case LOSS_DSSIM_MSE: wd = 0.8f; ws = 0.2f; break;
        case LOSS_DSSIM_MAE_MSE: wd = 0.6f; wa = 0.2f; ws = 0.2f; break;
        case LOSS_MSDSSIM: wm = 1.f; break;                                   // losses.py:92-130
        case LOSS_MSDSSIM_MAE: wm = 0.8f; wa = 0.2f; break;                   // :133-139
        case LOSS_MSDSSIM_MAE_MSE: wm = 0.6f; wa = 0.2f; ws = 0.2f; break;    // :142-149
        default: throw Dl4dsError("unknown loss kind " + std::to_string(kind));
    }
}

size_t loss_workspace_bytes(int kind, int N, int H, int W, int C) {
    float wd, wa, ws, wm;
    loss_weights(kind, wd, wa, ws, wm);
    size_t b = 2 * 1024 * sizeof(float);
    if (wd != 0.f) b += dssim_workspace_bytes(N, H, W, C);
    if (wm != 0.f) b += msdssim_workspace_bytes(N, H, W, C);
    return b;
}

void loss_forward_backward(hipStream_t s, int kind, const float* y_true, const float* y_pred, float* dpred, int N,
                           int H, int W, int C, float scale, float* loss_out, int accumulate, float* workspace,
                           size_t workspace_bytes) {
    float wd, wa, ws, wm;
    loss_weights(kind, wd, wa, ws, wm);
    const size_t n = (size_t)N * H * W * C;
    DL4DS_REQUIRE(workspace_bytes >= loss_workspace_bytes(kind, N, H, W, C), "loss workspace too small");
    const int nb = loss_blocks(n);
    const float inv_n = 1.f / (float)n;
    ProfScope ps(s, "pixel_loss", 0.0, 12.0 * (double)n);
    DL4DS_LAUNCH(pixel_loss_kernel, dim3(nb), dim3(256), 0, s, y_true, y_pred, dpred, n, scale * wa * inv_n,
                       scale * ws * inv_n, accumulate, workspace);
    HIP_CHECK(hipGetLastError());
    DL4DS_LAUNCH(pixel_loss_finish_kernel, dim3(1), dim3(64), 0, s, workspace, nb, scale * wa, scale * ws, inv_n,
                       loss_out, 0);
    HIP_CHECK(hipGetLastError());
    if (wd != 0.f) {
        dssim_forward_backward(s, y_true, y_pred, dpred, N, H, W, C, scale * wd, loss_out, 1, workspace + 2 * 1024,
                               workspace_bytes - 2 * 1024 * sizeof(float));
    }
    if (wm != 0.f) {
        msdssim_forward_backward(s, y_true, y_pred, dpred, N, H, W, C, scale * wm, loss_out, 1, workspace + 2 * 1024,
                                 workspace_bytes - 2 * 1024 * sizeof(float));
    }
}

// ---- weighted
void dssim_forward_backward_weighted(hipStream_t s, const float* y_true, const float* y_pred, float* dpred, int N, int H, int W,
                                     int C, float weight, float* loss_out, int accumulate_loss, const float* w, int w_batch,
                                     int w_channels, float* inv_so_dev, float* workspace, size_t workspace_bytes, float* ext,
                                     size_t ext_bytes);      // ext: the omega map and its partial sums
size_t dssim_weighted_workspace_bytes(int N, int H, int W, int C, int w_batch, int w_channels);

// inv_out[0] = 1 / (mult * sum x[0..n)), 0 for a zero sum; partial: at least 1024 floats
void weight_sum(hipStream_t s, const float* x, size_t n, double mult, float* partial, float* inv_out) {
    const int nb = loss_blocks(n);
    DL4DS_LAUNCH(weight_sum_kernel, dim3(nb), dim3(256), 0, s, x, n, partial);
    DL4DS_LAUNCH(weight_sum_finish_kernel, dim3(1), dim3(256), 0, s, partial, nb, mult, inv_out);
    HIP_CHECK(hipGetLastError());
}
void weight_sum_finish(hipStream_t s, const float* partial, int nb, double mult, float* inv_out) {
    DL4DS_LAUNCH(weight_sum_finish_kernel, dim3(1), dim3(256), 0, s, partial, nb, mult, inv_out);
    HIP_CHECK(hipGetLastError());
}

static const char* loss_kind_name(int kind) {
    static const char* names[] = {"mae", "mse", "dssim", "dssim_mae", "dssim_mse", "dssim_mae_mse", "msdssim", "msdssim_mae",
                                  "msdssim_mae_mse"};
    return (kind >= 0 && kind < 9) ? names[kind] : "?";
}

// layout: [unweighted workspace of the kind][64 floats: 1/sum w, 1/sum omega][1024 floats: weight partials][dssim: omega map + partials]
static constexpr size_t W_SCALARS = 64, W_PARTIALS = 1024;
size_t loss_workspace_bytes_weighted(int kind, int N, int H, int W, int C, int w_batch, int w_channels) {
    float wd, wa, ws, wm;
    loss_weights(kind, wd, wa, ws, wm);
    size_t b = ((loss_workspace_bytes(kind, N, H, W, C) + 255) & ~(size_t)255) + (W_SCALARS + W_PARTIALS) * sizeof(float);
    if (wd != 0.f) b += dssim_weighted_workspace_bytes(N, H, W, C, w_batch, w_channels);
    return b;
}

void loss_forward_backward_weighted(hipStream_t s, int kind, const float* y_true, const float* y_pred, float* dpred, int N,
                                    int H, int W, int C, float scale, float* loss_out, int accumulate, const float* w,
                                    int w_batch, int w_channels, float* workspace, size_t workspace_bytes) {
    float wd, wa, ws, wm;
    loss_weights(kind, wd, wa, ws, wm);
    DL4DS_REQUIRE(wm == 0.f, std::string("loss weights are not available for the multi-scale kinds: ") + loss_kind_name(kind));
    DL4DS_REQUIRE(w != nullptr && N > 0 && H > 0 && W > 0 && C > 0, "weighted loss: null weights / empty batch");
    DL4DS_REQUIRE(w_batch >= 1 && N % w_batch == 0, "weighted loss: w_batch must divide N (1: shared map, N: one map per sample)");
    DL4DS_REQUIRE(w_channels == 1 || w_channels == C, "weighted loss: w_channels must be 1 or C");
    DL4DS_REQUIRE((size_t)H * W * C < ((size_t)1 << 31) - 256, "weighted loss: one sample must hold fewer than 2^31 entries");
    DL4DS_REQUIRE(workspace_bytes >= loss_workspace_bytes_weighted(kind, N, H, W, C, w_batch, w_channels),
                  "weighted loss workspace too small");
    const size_t n = (size_t)N * H * W * C;
    const size_t base_bytes = (loss_workspace_bytes(kind, N, H, W, C) + 255) & ~(size_t)255;
    float* inv = reinterpret_cast<float*>(reinterpret_cast<char*>(workspace) + base_bytes);     // [0] 1/sum w  [1] 1/sum omega
    float* wpart = inv + W_SCALARS;
    float* dssim_ext = wpart + W_PARTIALS;
    const int nb = loss_blocks(n);
    WIndex ix;
    ix.per = (unsigned)((size_t)H * W * C); ix.wper = (unsigned)((size_t)H * W * w_channels);
    ix.C = (unsigned)C; ix.cw = (unsigned)w_channels; ix.wb = (unsigned)w_batch; ix.rep = (unsigned)(N / w_batch);
    const size_t stride = (size_t)nb * 256;
    ix.stride_n = (unsigned)(stride / ix.per); ix.stride_r = (unsigned)(stride % ix.per);
    const size_t nw = (size_t)w_batch * ix.wper;
    ProfScope ps(s, "pixel_loss_w", 0.0, 12.0 * (double)n + 4.0 * (double)nw * (1.0 + (double)ix.rep * (C / w_channels)));
    // sum over all entries of the batch = sum of the maps times how often each weight is used
    weight_sum(s, w, nw, (double)ix.rep * (double)(C / w_channels), wpart, inv);
    DL4DS_LAUNCH(pixel_loss_w_kernel, dim3(nb), dim3(256), 0, s, y_true, y_pred, w, dpred, n, ix, scale * wa, scale * ws, inv,
                 accumulate, workspace);
    HIP_CHECK(hipGetLastError());
    DL4DS_LAUNCH(pixel_loss_w_finish_kernel, dim3(1), dim3(64), 0, s, workspace, nb, scale * wa, scale * ws, inv, loss_out);
    HIP_CHECK(hipGetLastError());
    if (wd != 0.f) {
        dssim_forward_backward_weighted(s, y_true, y_pred, dpred, N, H, W, C, scale * wd, loss_out, 1, w, w_batch, w_channels,
                                        inv + 1, workspace + 2 * 1024, base_bytes - 2 * 1024 * sizeof(float), dssim_ext,
                                        dssim_weighted_workspace_bytes(N, H, W, C, w_batch, w_channels));
    }
}

void bce_forward_backward(hipStream_t s, const float* p, float label, int n, float scale, float* loss_out, float* dp,
                          int accumulate_loss) {
    DL4DS_LAUNCH(bce_kernel, dim3(1), dim3(256), 0, s, p, label, n, scale, loss_out, dp, accumulate_loss);
    HIP_CHECK(hipGetLastError());
}
