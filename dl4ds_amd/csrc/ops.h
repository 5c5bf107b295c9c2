// Internal C++ launch API of the gfx950 kernels (one stream argument everywhere; no hidden syncs).
#pragma once
#include "common.h"
#include <vector>

// ----------------------------------------------------------------------------- conv (conv.hip)
// y = epilogue(conv_same_stride1(x, w)) ; w is HWIO flattened [KS*KS][Cin][Cout]
struct ConvEpilogue {
    const float* bias = nullptr;   // [Cout] or null
    TView add{nullptr, 0, 0, 0, 0, 0, 0, 0};    // optional residual added before the activation
    TView mask{nullptr, 0, 0, 0, 0, 0, 0, 0};   // optional: result zeroed where mask <= 0 (ReLU backward)
    int relu = 0;
    int accumulate = 0;            // out += result (gradient accumulation)
    // optional [tiles][8] per-tile channel sums of the stored values (tiles of one image contiguous, see
    // conv2d_narrow_pair_tiles_per_image): the pooling of a ChannelAttention2D that consumes this output.  Only the
    // narrow pair kernel emits it (conv2d_forward_route(..).family == NarrowPair, conv_route.h), every other path rejects it.
    float* pool = nullptr;
    // Second output pairs (both with the output's shape and layout; conv2d_forward_fused only, see there):
    //   sum_out = v + sum_add, v the value stored to `out` (AFTER the activation -- not `add`, which comes before it): an Add that
    //   consumes this layer's output, written by the layer;
    //   out2 = the value `out` receives before ITS mask, zeroed where mask2 <= 0 (needs mask): the backward of an Add of two ReLU
    //   outputs, written by the dgrad that produces the Add's output gradient.  With more than one pass over the input channels the
    //   raw partial sums accumulate in `partial` (then required: the Add's output-gradient buffer), not in `out`.
    TView sum_add{nullptr, 0, 0, 0, 0, 0, 0, 0}, sum_out{nullptr, 0, 0, 0, 0, 0, 0, 0};
    TView mask2{nullptr, 0, 0, 0, 0, 0, 0, 0}, out2{nullptr, 0, 0, 0, 0, 0, 0, 0}, partial{nullptr, 0, 0, 0, 0, 0, 0, 0};
};
void conv2d_forward(hipStream_t s, const TView& in, const float* w, int KS, const TView& out,
                    const ConvEpilogue& ep);
// The same convolution with an epilogue that carries sum_out or out2, on the kernel conv2d_forward picks for the call without
// them -- if that kernel has the form (conv_split: sum_out; conv_wino<3,3>: both).  false: nothing was launched, the caller runs
// the plain convolution and the stand-alone element-wise pass (conv2d_forward itself refuses such an epilogue).
bool conv2d_forward_fused(hipStream_t s, const TView& in, const float* w, int KS, const TView& out, const ConvEpilogue& ep);
// wt[(KS*KS-1-tap)][co][ci] = w[tap][ci][co] : conv2d_forward(dz, wt) == dgrad
void conv2d_dgrad_weights(hipStream_t s, const float* w, float* wt, int KS, int Cin, int Cout);
// several of them in one launch: jobs_dev = nj x DgradWeightsJob on the device, blocks = sum of their block counts
struct DgradWeightsJob { const float* src; float* dst; int KK, Cin, Cout, block0; };
int dgrad_weights_job_blocks(int KK, int Cin, int Cout);
void conv2d_dgrad_weights_batched(hipStream_t s, const DgradWeightsJob* jobs_dev, int nj, int blocks);
// dw[tap][ci][co] (+)= sum_{n,y,x} x[n,y+ky-p,x+kx-p,ci] * dz[n,y,x,co] ; db[co] (+)= sum dz[n,y,x,co] (db may be null)
size_t conv2d_wgrad_workspace_bytes(const TView& x, const TView& dz, int KS);
void conv2d_wgrad(hipStream_t s, const TView& x, const TView& dz, int KS, float* dw, int accumulate, float* db,
                  int accumulate_db, float* workspace, size_t workspace_bytes);
// Which family takes a layer is stated once, by conv2d_forward_route / conv2d_wgrad_route (conv_route.h): conv2d_forward / conv2d_wgrad
// follow them, a caller that plans around a family (pooling partials, a channel-affine view) asks them; the entry points below only launch.
// Stencil (VALU) path for 3x3 layers with pad2(Cin)*pad2(Cout) <= 8 (conv_direct.hip)
void conv2d_direct_forward(hipStream_t s, const TView& in, const float* w, const TView& out, const ConvEpilogue& ep);
// 3x3, Cin <= 16, Cout <= 16: register-resident filter, persistent MFMA kernel (conv_narrow.hip); pair_ok: the route is NarrowPair
void conv2d_narrow_forward(hipStream_t s, const TView& in, const float* w, const TView& out, const ConvEpilogue& ep, bool pair_ok);
// 1x1 layers with channel counts that are multiples of four, up to 48, on flat views (conv_pointwise.hip): register-direct loads,
// MFMA, float4 stores, no LDS; the route is Pointwise
void conv2d_pointwise_forward(hipStream_t s, const TView& in, const float* w, const TView& out, const ConvEpilogue& ep);
// 1x1 layers whose channel counts are not multiples of four (conv_point.hip): contiguous staging + MFMA + contiguous store
bool conv2d_point_forward(hipStream_t s, const TView& in, const float* w, int KS, const TView& out, const ConvEpilogue& ep);
int conv2d_narrow_pair_tiles_per_image(int H, int W);
// weight gradient of a stencil convolution behind a ChannelAttention2D scale + the attention's d(loss)/d(scale), both from
// per-image raw weight gradients (conv_direct.hip); false: not eligible, nothing was launched
bool conv2d_direct_wgrad_attention(hipStream_t s, const TView& x_raw, const TView& dz, int KS, const float* scale, const float* w,
                                   float* dw, int accumulate, float* db, int accumulate_db, float* ds, float* workspace,
                                   size_t workspace_bytes);
size_t conv2d_direct_wgrad_attention_workspace_bytes(const TView& x_raw, const TView& dz, int KS);      // (what it asks of `workspace`)
// 3x3 wgrad with Cin <= 8, Cout <= 16 (two taps per MFMA tile); same slab protocol as the direct path
int conv2d_narrow_wgrad(hipStream_t s, const TView& x, const TView& dz, int KS, float* partial, int max_slabs);
// 3x3, Cin >= 16: filter streamed from L2 into the MFMA operands, no barriers in the K loop (conv_stream.hip)
// small grids (H W <= max_hw) with many channels as a GEMM over flattened pixels (conv_gemm.hip); false = not eligible
bool conv2d_gemm_forward(hipStream_t s, const TView& in, const float* w, int KS, const TView& out, const ConvEpilogue& ep, int max_hw);
// Winograd F(2x2, 3x3) form of the MFMA-bound 3x3 layers (conv_wino.hip); false = not eligible
bool conv2d_wino_forward(hipStream_t s, const TView& in, const float* w, const TView& out, const ConvEpilogue& ep,
                         bool* form_refused = nullptr);
// (form_refused, both kernels: set when the layer is the kernel's but ep's sum_out / out2 form is not built -- conv2d_forward_fused)
// the 40 / 48-channel 3x3 layers with their fp32 products as six bf16 MFMA terms (conv_split.hip); false = not eligible / DL4DS_NO_SPLIT
bool conv2d_split_forward(hipStream_t s, const TView& in, const float* w, const TView& out, const ConvEpilogue& ep,
                          bool* form_refused = nullptr);
// The operands derived from the filters of a graph's layers -- the Winograd layers' transformed filters (conv_wino.hip), then the
// six-term kernel's bf16 fragments (conv_split.hip) -- one batched launch each per pass instead of one per layer (conv_cache.h; a pass
// of a graph holds a GraphPassGuard): _invalidate marks every registered filter inside [lo, hi) stale, _refresh rebuilds the stale
// ones of that pass kind (0 = forward, 1 = backward) on s, _release frees them (graph destruction).
void derived_filters_invalidate(const float* lo, const float* hi);
void derived_filters_refresh(hipStream_t s, const float* lo, const float* hi, int kind);
void derived_filters_release(const float* lo, const float* hi);
// conv_split.hip: its share of the three (called by the derived_filters_* functions)
void split_filters_invalidate(const float* lo, const float* hi);
void split_filters_refresh(hipStream_t s, const float* lo, const float* hi, int kind);
void split_filters_release(const float* lo, const float* hi);
// ... and of their weight gradient (conv_wino_wgrad.hip): dw [3][3][Cin][Cout], db [Cout] or null
bool conv2d_wino_wgrad(hipStream_t s, const TView& x, const TView& dy, float* dw, int accumulate, float* db, int accumulate_db);
bool conv2d_stream_forward(hipStream_t s, const TView& in, const float* w, int KS, const TView& out,
                           const ConvEpilogue& ep);
// writes at most `slabs` partial slabs (the workspace bound); returns how many it wrote
int conv2d_direct_wgrad(hipStream_t s, const TView& x, const TView& dz, int KS, float* partial, int slabs);
// Conv2DTranspose(k, stride s, 'same', no bias), kernel HWOI [k*k][Cout][Cin] (blocks.py:508-516)
void conv2d_transpose_forward(hipStream_t s, const TView& in, const float* w, int KS, int stride,
                              const TView& out, int relu, float* workspace, size_t workspace_bytes);
// `relu_mask` (may be null): the layer's INPUT activation; its gradient is zeroed where that activation is <= 0 (the ReLU
// backward of the producing layer folded into this store)
void conv2d_transpose_dgrad(hipStream_t s, const TView& dz, const float* w, int KS, int stride,
                            const TView& dx, int accumulate, float* workspace, size_t workspace_bytes,
                            const TView* relu_mask = nullptr);
void conv2d_transpose_wgrad(hipStream_t s, const TView& x, const TView& dz, int KS, int stride,
                            float* dw, int accumulate, float* workspace, size_t workspace_bytes);
size_t conv2d_transpose_workspace_bytes(const TView& in, const TView& out, int KS, int stride);

// ------------------------------------------------------------------- elementwise (elementwise.hip)
// dz = dy * (y > 0 ? 1 : 0) (if y.p) written to dz (may alias dy); db[c] (+)= sum dz[...,c] (if db)
size_t bias_grad_workspace_bytes(const TView& dy);
void bias_act_backward(hipStream_t s, const TView& dy, const TView& y, const TView& dz, float* db,
                       int accumulate_db, float* workspace, size_t workspace_bytes);
// dst (+)= alpha * src  (same logical shape; either side may be a strided / d2s view)
void view_axpy(hipStream_t s, const TView& src, const TView& dst, float alpha, int accumulate);
// dst (+)= src * [mask > 0] (mask.p == nullptr: plain copy): Concatenate backward of a ReLU output whose mask the consumers apply
void view_axpy_masked(hipStream_t s, const TView& src, const TView& mask, const TView& dst, int accumulate);
// Concatenate backward in one pass over the wide gradient (elementwise.hip): slice k = channels [off, off + C) -> dense dst (+ mask)
struct ConcatSlice { float* dst; const float* mask; int off, C, accumulate; };
void concat_split(hipStream_t s, const float* src, int ld, size_t npx, const ConcatSlice* slices, int n);
// the mirror, Concatenate forward in one pass: slices[k].dst is read as the dense input k (mask / accumulate unused)
void concat_join(hipStream_t s, float* dst, int ld, size_t npx, const ConcatSlice* slices, int n);
// dst (+)= dy * [y > 0]  (flat, contiguous)
void masked_axpy(hipStream_t s, const float* dy, const float* y, float* dst, size_t n, int accumulate);
// ... for both operands of an Add at once (false: not applicable, call masked_axpy twice)
bool masked_axpy_pair(hipStream_t s, const float* dy, const float* ya, float* da, int acc_a, const float* yb, float* db, int acc_b, size_t n);
// out = act(a + b)
void add_act(hipStream_t s, const float* a, const float* b, float* out, size_t n, int relu);
// in-place / out-of-place activation forward y = f(x) and backward dx (+)= dy * f'(x)
enum ActKind { ACT_NONE = 0, ACT_RELU = 1, ACT_SIGMOID = 2, ACT_TANH = 3, ACT_ELU = 4,
               ACT_LEAKY_RELU = 5, ACT_SELU = 6, ACT_GELU = 7 };
void act_forward(hipStream_t s, const float* x, float* y, size_t n, int kind);
void act_backward(hipStream_t s, const float* x, const float* dy, float* dx, size_t n, int kind,
                  int accumulate);
void fill(hipStream_t s, float* p, size_t n, float v);
// DepthwiseConv2D(7, 'same') of ConvNextBlock (dwconv.hip).  flip != 0: mirrored taps = the input gradient.
void dwconv_forward(hipStream_t s, const float* x, const float* k, const float* bias, float* y, int N, int H, int W, int C,
                    int KS, int flip, int accumulate);
size_t dwconv_wgrad_workspace_bytes(int C, int KS);
void dwconv_wgrad(hipStream_t s, const float* x, const float* dy, float* dk, float* db, int accumulate, int N, int H, int W, int C,
                  int KS, float* ws, size_t ws_bytes);
// post-hoc test metrics of dl4ds/metrics.py:166-262 (dssim.hip): pair_out [N][4] = (mae, mse, pearson over the grid, ssim),
// grid_out [3][H*W*C] = (rmse, mean bias, pearson over the pairs), range_out [2] = joint (min, max)
size_t metrics_workspace_bytes(int N, int H, int W, int C);
void image_metrics(hipStream_t s, const float* y_true, const float* y_pred, int N, int H, int W, int C, float* pair_out_dev,
                   float* grid_out_dev, float* range_out_dev, float* workspace, size_t workspace_bytes);
// Spearman rank correlation (rank.hip) of S pairs of length-L sequences, element k of pair s at [s*seg_stride + k*elem_stride]:
// out[s] = scipy.stats.spearmanr(a_s, b_s)[0] in fp64 (average ranks of ties; NaN for a NaN, a constant side or L < 2)
size_t spearman_workspace_bytes(size_t S, size_t L);
void spearman(hipStream_t s, const float* a, const float* b, size_t S, size_t L, size_t seg_stride, size_t elem_stride, double* out,
              void* workspace, size_t workspace_bytes);
// MinMaxScaler / StandardScaler of preprocessing.py (scaler.hip).  shape / reduce describe a C-contiguous array of ndim axes and
// which of them are reduced (reduce[i] != 0); float or double data.  scaler_stats: out [5][cells] fp64 = count, min, max, mean,
// population std per kept cell, NaNs skipped (an empty cell: count 0, NaN); *nan_flag = 1 if any NaN was seen; mask_bits (optional)
// = the NaN mask, bit e%32 of word e/32 for flat element e ((n + 31) / 32 words).  Bitwise reproducible.
// scaler_apply: out[e] = op2(op1(x[e], a[cell(e)]), b[cell(e)]), each operation rounded on its own in the array's type, then
// NaN -> fill (SCALER_NAN_FILL) or NaN where the mask bit is set (SCALER_NAN_MASK, mask_bits may be null); out may be x.
enum ScalerOp { SCALER_OP_NONE = 0, SCALER_OP_MUL = 1, SCALER_OP_ADD = 2, SCALER_OP_SUB = 3, SCALER_OP_DIV = 4 };
enum ScalerNan { SCALER_NAN_FILL = 0, SCALER_NAN_MASK = 1 };
size_t scaler_cells(const size_t* shape, int ndim, const int* reduce);
size_t scaler_stats_workspace_bytes(const size_t* shape, int ndim, const int* reduce, int is_double);
void scaler_stats(hipStream_t s, const void* x, int is_double, const size_t* shape, int ndim, const int* reduce, double* out,
                  unsigned* nan_flag, unsigned* mask_bits, void* workspace, size_t workspace_bytes);
void scaler_apply(hipStream_t s, const void* x, void* out, int is_double, const size_t* shape, int ndim, const int* reduce, int op1,
                  const void* a, int op2, const void* b, int nan_mode, double fill, const unsigned* mask_bits);
// Member statistics of an MC-dropout ensemble (ensemble.hip): one read of members[K][n] (row k at members + k * member_stride) ->
// per element mean, population std, min, max and quant[j][e] = np.quantile(q[j], method='linear') over the K values, evaluated as
// numpy does on the fp64 copy of the stack and rounded to fp32 once.  Any output may be null.  Bitwise reproducible.
constexpr int ENS_MAX_MEMBERS = 256, ENS_MAX_QUANTILES = 32;
void ensemble_reduce(hipStream_t s, const float* members, size_t K, size_t n, size_t member_stride, const float* q_host, int nq,
                     float* mean, float* std_, float* mn, float* mx, float* quant);
// Verification of the ensemble members[K][n] against obs[n] (ensemble_score.hip): per element CRPS (fair != 0: the fair form),
// squared error of the ensemble mean, unbiased variance, rank of the observation with hashed tie-breaking, coverage of nq quantiles;
// folded per sample (sample_out[B][4]: sums of crps, sqerr, var and the valid count), per cell (cell_acc[4][n / B], +=) and into
// rank_hist[K + 1] / covered[nq] (+=).  Elements next to a non-finite value or a scale cell that is not finite and > 0 are invalid:
// NaN / rank -1, in no fold.  Per-element outputs and folds may be null.  No floating-point atomics: bitwise reproducible.
size_t ensemble_score_workspace_bytes(size_t n, size_t B);
void ensemble_score(hipStream_t s, const float* members, size_t K, size_t n, size_t member_stride, const float* obs, size_t B,
                    unsigned long long elem_offset, const float* scale, int fair, unsigned long long seed, const float* q_host, int nq,
                    float* crps, float* sqerr, float* var, int* rank, double* sample_out, double* cell_acc,
                    unsigned long long* rank_hist, unsigned long long* covered, void* workspace, size_t workspace_bytes);
// Exceedance verification of the ensemble members[K][n] against obs[n] at T thresholds (exceedance.hip): thr [T], or
// [T][n / B] with thr_per_cell; per valid (t, e): o = [obs >= thr], c = #{k : x_k >= thr}.  count [T][n] = c or -1 (overwritten),
// sample_out [B][T][4] = n_valid, sum o, sum c, sum (c - K o)^2 per sample (overwritten), cell_acc [T][4][n / B] the same per cell
// (+=), table [T][K + 1][2] the number of valid elements with (c, o) (+=).  Outputs may be null.  Integer arithmetic only.
// exc_walk_limit: the samples one lane may walk before its 32-bit partial sums could overflow (the launch splits a call by it).
constexpr int EXC_MAX_THRESHOLDS = 16;
size_t exc_walk_limit(size_t K);
void ensemble_exceedance(hipStream_t s, const float* members, size_t K, size_t n, size_t member_stride, const float* obs, size_t B,
                         const float* thr, int T, int thr_per_cell, short* count, long long* sample_out, long long* cell_acc,
                         unsigned long long* table);
// Multivariate verification of the ensemble members[K][n] against obs[n] (ensemble_multi.hip), 2 <= K <= 128, B whole samples of
// n / B elements, weight [n / B] or null; an element is valid iff obs and all K members are finite and its weight (if any) is > 0.
// ensemble_energy: dist_out [B][K (K + 1) / 2] = D_k = sum w (x_k - y)^2 (k < K), then G_kj = sum w (x_k - x_j)^2 row-major over
// k < j, each term and sum in fp64 from the differences themselves; nvalid_out [B].  ensemble_variogram: a sample is planes x H x W
// x C; per sample and lag of variogram_lags(max_lag) (ordered (dy, dx) in the upper half-plane, at most 98) npairs_out [B][L] and
// sums_out [B][L][3] = sum (o - e)^2, sum o, sum e over the valid pairs of one H x W plane, o = |y_i - y_j|^p and e_k in fp32,
// e = (sum_k e_k in fp64, member order) / K; order_code 0 / 1 / 2: p = 0.5 / 1 / 2.  Outputs are overwritten.  No floating-point
// atomics; how a sample is split over workgroups depends on (K, sample shape, max_lag) alone: the sums of a sample have the same
// bits for every B and every position in the call.  The *_check functions throw on a bad request (before a workspace is sized).
constexpr int ENS_MULTI_MAX_MEMBERS = 128;
int variogram_lags(int max_lag, int* dydx, int* count);
void ensemble_energy_check(const float* members, size_t K, size_t n, size_t member_stride, const float* obs, size_t B,
                           const double* dist_out, const long long* nvalid_out);
size_t ensemble_energy_workspace_bytes(size_t K, size_t n, size_t B);
void ensemble_energy(hipStream_t s, const float* members, size_t K, size_t n, size_t member_stride, const float* obs, size_t B,
                     const float* weight, double* dist_out, long long* nvalid_out, void* workspace, size_t workspace_bytes);
void ensemble_variogram_check(const float* members, size_t K, size_t n, size_t member_stride, const float* obs, size_t B,
                              size_t planes, size_t H, size_t W, size_t C, int max_lag, int order_code, const long long* npairs_out,
                              const double* sums_out);
size_t ensemble_variogram_workspace_bytes(size_t B, size_t planes, size_t H, size_t C, int max_lag);
void ensemble_variogram(hipStream_t s, const float* members, size_t K, size_t n, size_t member_stride, const float* obs, size_t B,
                        const float* weight, size_t planes, size_t H, size_t W, size_t C, int max_lag, int order_code,
                        long long* npairs_out, double* sums_out, void* workspace, size_t workspace_bytes);
// Neighbourhood verification (fss.hip) of the N*C fields of y, p (N, H, W, C) at T thresholds and S window sizes (host arrays):
// sums [N][C][T][S][3] = the exact integer sums D, F, O of the Fractions Skill Score, cont [N][C][T][4] = hits, misses, false
// alarms, correct negatives over the valid (both finite) cells, valid [N][C] their count.  Outputs are overwritten.  Integer
// arithmetic only: equal to a reference, whatever the order of the atomics.  fss_check_args throws on a bad or overflowing request.
size_t fss_workspace_bytes(int N, int H, int W, int C, int T);
void fss_check_args(int N, int H, int W, int C, const float* thresholds, int T, const int* windows, int S);
void fss(hipStream_t s, const float* y, const float* p, int N, int H, int W, int C, const float* thresholds, int T,
         const int* windows, int S, long long* sums, long long* cont, long long* valid, void* workspace, size_t workspace_bytes);
// Neighbourhood verification of the ensemble members[K][n] against obs[n] (ensemble_fss.hip): the n elements are B samples of
// (H, W, C), each of the B*C planes a field; per valid cell (obs and all members finite) and threshold o = [obs >= t], c = #{k :
// x_k >= t}; co, cf their sums over fss.hip's window.  sums [B][C][T][S][5] = D = sum (cf - K co)^2, F = sum cf^2, O = sum co^2
// over all cells, Fv = sum cf^2 over the valid centre cells, X = sum cf over the centre cells with o = 1; cont [B][C][T][2] = sum o,
// sum c; valid [B][C].  Thresholds and windows are host arrays.  Outputs are overwritten.  Integer arithmetic only.
// ensemble_fss_check_args throws on a bad or overflowing request (before the workspace is sized).
size_t ensemble_fss_workspace_bytes(size_t K, size_t B, int H, int W, int C, int T);
void ensemble_fss_check_args(const float* members, size_t K, size_t n, size_t member_stride, const float* obs, size_t B, int H,
                             int W, int C, const float* thresholds, int T, const int* windows, int S, const long long* sums,
                             const long long* cont, const long long* valid);
void ensemble_fss(hipStream_t s, const float* members, size_t K, size_t n, size_t member_stride, const float* obs, size_t B, int H,
                  int W, int C, const float* thresholds, int T, const int* windows, int S, long long* sums, long long* cont,
                  long long* valid, void* workspace, size_t workspace_bytes);
// Object labelling (objects.hip) of the N*C fields of x (N, H, W, C) at one device threshold per field:
// labels [F][H][W] (or null), count [F], nvalid [F], field_sums [F][3], and tables of cap rows per field: sums [F][cap][6], bbox
// [F][cap][4], first [F][cap], vmax [F][cap], mass [F][cap][3] (null when cap == 0).  Outputs are overwritten.  err: the sticky
// device error word (runtime.h), raised if a parent walk passes its bound.  objects_check_args throws on a request the entry
// refuses (before the workspace is sized).  object_thresholds: thr [F] = float32(factor * max of the finite cells), 0 without one.
size_t objects_workspace_bytes(int N, int H, int W, int C);
void objects_check_args(const float* x, int N, int H, int W, int C, const float* thr, int connectivity, int cap, const int* count,
                        const long long* sums, const int* bbox, const int* first, const float* vmax, const double* mass);
void label_objects(hipStream_t s, const float* x, int N, int H, int W, int C, const float* thr, int connectivity, int cap, int* labels,
                   int* count, long long* nvalid, double* field_sums, long long* sums, int* bbox, int* first, float* vmax,
                   double* mass, void* workspace, size_t workspace_bytes, unsigned* err);
size_t object_thresholds_workspace_bytes(int N, int H, int W, int C);
void object_thresholds(hipStream_t s, const float* x, int N, int H, int W, int C, double factor, float* thr, void* workspace,
                       size_t workspace_bytes);
// Distance-map verification (distance.hip) of the N*C fields of y, p (N, H, W, C) at T host thresholds: per
// field and threshold counts [F][T][8] (n_valid, n_A, n_B, n_AB, max and sum of d2 from A to B and from B to A) and sums [F][T][7]
// (sum d both ways, Pratt sums both ways, Baddeley sum w, sum w^2, max w); d2_obs / d2_pred [F][T][H][W] (or null): the squared
// distance maps of A and B.  Outputs are overwritten.  distance_check_args throws on a request the entry refuses (before the
// workspace is sized).
size_t distance_workspace_bytes(int N, int H, int W, int C, int T);
void distance_check_args(const float* y, const float* p, int N, int H, int W, int C, const float* thresholds, int T, double cutoff,
                         double alpha, const long long* counts, const double* sums);
void distance_scores(hipStream_t s, const float* y, const float* p, int N, int H, int W, int C, const float* thresholds, int T,
                     double cutoff, double alpha, long long* counts, double* sums, int* d2_obs, int* d2_pred, void* workspace,
                     size_t workspace_bytes);
// Regridding between rectilinear grids (regrid.hip).  A plan holds the two axis tables (CSR, fp64 weights) and
// the destination cell measures on the device; plan_create validates the host tables and throws before anything is allocated.
// apply: x (N, H, W, C) -> out (N, H', W', C).  consistency: sums [N][C][6], counts [N][C][2] of the regridded x against ref
// (N, H', W', C), resid (or null) the fp32 residual; workspace: regrid_consistency_workspace_bytes.  regrid_check_call throws on a
// call the entries refuse.
struct RegridPlan;
RegridPlan* regrid_plan_create(hipStream_t s, int H, int W, int Ho, int Wo, const int* yptr, const int* yidx, const double* yw,
                               const int* xptr, const int* xidx, const double* xw, const double* ay, const double* ax);
void regrid_plan_destroy(hipStream_t s, RegridPlan* p);
void regrid_check_call(const char* what, const RegridPlan* p, const float* x, int N, int C, double min_valid);
size_t regrid_consistency_workspace_bytes(const RegridPlan* p, int N, int C);
void regrid_apply(hipStream_t s, const RegridPlan* p, const float* x, int N, int C, bool skipna, double min_valid, float* out);
void regrid_consistency(hipStream_t s, const RegridPlan* p, const float* x, const float* ref, int N, int C, bool skipna,
                        double min_valid, double* sums, long long* counts, float* resid, void* workspace);
// Distribution verification (distribution.hip) of S pairs of length-L segments, element k of segment s at [s*seg_stride +
// k*elem_stride]: per segment quant [S][2][Q] (numpy 'linear' quantiles of the valid values of y, p), w1 [S] (1-Wasserstein), ks [S]
// (n times the two-sample KS statistic), hist [S][2][E-1] (np.histogram over the E edges; may be null when E == 0), valid [S] (n).
// q / edges are host arrays.  Outputs are overwritten.  distribution_check_args throws on a request the entry refuses.
size_t distribution_workspace_bytes(size_t S, size_t L, size_t seg_stride, size_t elem_stride);
void distribution_check_args(size_t S, size_t L, const double* q, int Q, const float* edges, int E);
void distribution(hipStream_t s, const float* y, const float* p, size_t S, size_t L, size_t seg_stride, size_t elem_stride,
                  const double* q, int Q, const float* edges, int E, double* quant, double* w1, long long* ks, long long* hist,
                  long long* valid, void* workspace, size_t workspace_bytes);
// Quantile-mapping bias correction (qmap.hip).  quantile_table: per cell c < per the Q 'linear' sample quantiles
// of the finite values among x[n*per + c], n < N, rounded to fp32 into table [Q][per], and their number into valid [per] (may be
// null); q is a host array.  qmap_apply: B samples of per cells through the tables of the model's history, the observation and
// (QDM; null: EQM) the period being corrected; kind 0 additive, 1 multiplicative; counts [4] (nonfinite, unfitted, below, above;
// may be null) are added to; out may be x.  quantile_table_workspace_bytes throws on an empty array or N >= 2^31 (before anything
// is sized); quantile_table checks the probabilities, once.
size_t quantile_table_workspace_bytes(size_t N, size_t per);
void quantile_table(hipStream_t s, const float* x, size_t N, size_t per, const double* q, int Q, float* table, long long* valid,
                    void* workspace, size_t workspace_bytes);
void qmap_apply(hipStream_t s, const float* x, float* out, size_t B, size_t per, const float* model_tab, const float* obs_tab,
                const float* target_tab, int Q, int kind, int keep_unfitted, unsigned long long* counts);
// Climate indices along the time axis (indices.hip) of x (N samples of per cells) over the P periods of the
// HOST array period_starts [P + 1] at T <= 4 thresholds (thr [T] or, thr_per_cell, [T][per]; DEVICE) under one comparison op:
// valid [P][per], event [P][T][6][per] (events, longest event / non-event run, event runs, first / last event offset), ext
// [P][2][per] (max, min), sum [P][2 + T][per] (sum, largest window sum, event sums; fp64 in sample order).  Outputs may be null
// (not all) and are overwritten.  climate_indices_workspace_bytes throws on a request the entry refuses, before anything is sized;
// the workspace takes the period starts.  Synchronises the stream once, after their upload.
constexpr int IDX_MAX_THRESHOLDS = 4;
size_t climate_indices_workspace_bytes(size_t N, size_t per, const long long* period_starts, int P, int T, int op, int window);
void climate_indices(hipStream_t s, const float* x, size_t N, size_t per, const long long* period_starts, int P, const float* thr,
                     int T, int thr_per_cell, int op, int window, int* valid, int* event, float* ext, double* sum, void* workspace,
                     size_t workspace_bytes);
// Extreme-value verification (extremes.hip).  lmoments: per cell c < per Hosking's unbiased probability-weighted
// moments b_0..b_3 of the finite values among sign * x[n*stride + c], n < N (stride >= per), summed in rank order in fp64 into
// pwm [4][per] (NaN where n <= r), their number into valid [per]; either may be null.  pot_peaks: the declustered peaks of x (N
// samples of per cells) over the threshold thr ([1] or, thr_per_cell, [per]; DEVICE) within the P periods of the HOST array
// period_starts [P + 1]: count [per] the clusters, peak / pos [K][per] the first K peaks and their sample indices in order of
// occurrence, NaN / -1 beyond the count (either may be null; K == 0 only counts).  Both *_workspace_bytes throw on a request
// the entry refuses, before anything is sized; pot_peaks' workspace takes the period starts and it synchronises the stream once.
constexpr int POT_MAX_RUN = 32;
size_t lmoments_workspace_bytes(size_t N, size_t per, size_t stride, int sign);
void lmoments(hipStream_t s, const float* x, size_t N, size_t per, size_t stride, int sign, int* valid, double* pwm, void* workspace,
              size_t workspace_bytes);
size_t pot_peaks_workspace_bytes(size_t N, size_t per, const long long* period_starts, int P, int sign, int run, int K);
void pot_peaks(hipStream_t s, const float* x, size_t N, size_t per, const long long* period_starts, int P, const float* thr,
               int thr_per_cell, int sign, int run, int K, int* count, float* peak, int* pos, void* workspace, size_t workspace_bytes);
// Temporal verification (temporal.hip) of y and, when p is not null, of p on common validity (N samples of per
// cells, S = 1 or 2 series) over the P periods of the HOST array period_starts [P + 1], at the L <= 4 lags of the HOST array lags
// (strictly increasing, 1..32) and at T <= 4 thresholds (thr [T] or, thr_per_cell, [T][per]; DEVICE) under one comparison op:
// valid [P][per], moment [P][S][2][per] (sum x, sum x^2), pair [P][L][per], lag [P][S][L][3][per] (sum a, sum b, sum a*b over the
// pairs), trans [P][S][T][4][per] (n00, n01, n10, n11), spell [P][S][T][2][B][per] (run-length histograms of event and non-event
// runs, B = spell_bins in 1..32).  Outputs may be null (not all; pair / lag need L > 0, trans / spell T > 0) and are overwritten;
// fp64 sums in sample order.  temporal_workspace_bytes throws on a request the entry refuses, before anything is sized; the
// workspace takes the period starts and the lags.  Synchronises the stream once, after their upload.
constexpr int TMP_MAX_LAGS = 4, TMP_MAX_THRESHOLDS = 4, TMP_MAX_BINS = 32;
size_t temporal_workspace_bytes(size_t N, size_t per, const long long* period_starts, int P, const int* lags, int L, int T, int op,
                                int spell_bins);
void temporal(hipStream_t s, const float* y, const float* p, size_t N, size_t per, const long long* period_starts, int P,
              const int* lags, int L, const float* thr, int T, int thr_per_cell, int op, int spell_bins, int* valid, double* moment,
              int* pair, double* lag, int* trans, int* spell, void* workspace, size_t workspace_bytes);
// Trend per cell over the P <= 128 periods of v [P][per] (fp64, DEVICE; trend.hip): valid [per] the number of
// finite values, mk [2][per] the Mann-Kendall S and its tie term, sen [per] Sen's slope.  Outputs may be null (not all).
constexpr int TRD_MAX_PERIODS = 128;
void trend(hipStream_t s, const double* v, int P, size_t per, int* valid, long long* mk, double* sen);
// Spectral verification (spectrum.hip) of the N*C fields of y, p (N, H, W, C; p may be null): the unnormalised 2-D DFT of either
// side in fp64 (kept cells, optional detrending and periodic Hann window), folded over the bins of the HOST map bin [H][W/2 + 1]
// (values in [-1, B)) into power [N][C][4][B]; valid [N][C] kept cells, mean [N][C][2] the subtracted means.  Outputs are
// overwritten.  Fixed-order reductions: bitwise reproducible.  `sides`: 2 with a prediction, 1 without.  Synchronises the stream
// once, after the upload of the call's tables.  spectrum_check_args throws on a request the entry refuses.
size_t spectrum_workspace_bytes(int N, int H, int W, int C, int sides, int B);
void spectrum_check_args(int N, int H, int W, int C, const int* bin_host, int B);
void spectrum(hipStream_t s, const float* y, const float* p, int N, int H, int W, int C, int detrend, int window, const int* bin_host,
              int B, double* power, long long* valid, double* mean, void* workspace, size_t workspace_bytes);
// Merge of a batch of tile outputs into the output field (tiles.hip): out[smp[t]][oy[t] + y][ox[t] + x][c] +=
// wy[ry[t]][y] * wx[rx[t]][x] * tiles[t][y][x][c], taps in ascending t, zero weights skipped.  The five lists are DEVICE ints; nothing
// is checked here (capi.cpp does); `vec`: 16-byte accesses are legal for this batch.
void tile_merge(hipStream_t s, const float* tiles, const float* wy, const float* wx, float* out, const int* oy, const int* ox,
                const int* smp, const int* ry, const int* rx, int n, int th, int tw, int C, int H, int W, bool vec);
// sums[smp[t]][c] += sum_yx wy * wx * tiles[t][y][x][c] in fp64, fixed order (tiles.hip); partial: [n][C] doubles of scratch
void tile_pool(hipStream_t s, const float* tiles, const float* wy, const float* wx, const int* smp, const int* ry, const int* rx,
               int n, int th, int tw, int C, double* partial, double* sums);
// LayerNormalization / BatchNormalization over the channel axis of [npix][C] (norm.hip), optional fused ReLU
size_t norm_workspace_bytes(int C);
void layernorm_forward(hipStream_t s, const float* x, const float* gamma, const float* beta, float* y, size_t npix, int C,
                       float eps, int relu);
void layernorm_backward(hipStream_t s, const float* x, const float* y, const float* dy, const float* gamma, float* dx, int acc_dx,
                        float* dgamma, float* dbeta, int acc_dw, size_t npix, int C, float eps, int relu, float* ws,
                        size_t ws_bytes);
void batchnorm_forward(hipStream_t s, const float* x, const float* gamma, const float* beta, float* mov_mean, float* mov_var,
                       float* y, float* saved, size_t npix, int C, float eps, float momentum, int training, int relu, float* ws,
                       size_t ws_bytes);
void batchnorm_backward(hipStream_t s, const float* x, const float* y, const float* dy, const float* gamma, const float* saved,
                        float* dx, int acc_dx, float* dgamma, float* dbeta, int acc_dw, size_t npix, int C, int relu, float* ws,
                        size_t ws_bytes);
// depth_to_space standalone (used by tests and unfused fallbacks)
void depth_to_space(hipStream_t s, const float* x, float* y, int N, int H, int W, int C, int r);
void space_to_depth(hipStream_t s, const float* y, float* x, int N, int H, int W, int C, int r);
// MaxPooling2D(2,2) valid
void maxpool2_forward(hipStream_t s, const TView& x, const TView& y);
// relu_mask != 0: x is a ReLU output whose backward rides on this store (gradient zeroed where x <= 0)
void maxpool2_backward(hipStream_t s, const TView& x, const TView& y, const TView& dy, const TView& dx,
                       int accumulate, int relu_mask = 0);
// bilinear resize (half-pixel centres)
void resize_bilinear_forward(hipStream_t s, const TView& x, const TView& y);
void resize_nearest_forward(hipStream_t s, const TView& x, const TView& y);
void resize_nearest_backward(hipStream_t s, const TView& dy, const TView& dx, int accumulate);
void resize_bilinear_backward(hipStream_t s, const TView& dy, const TView& dx, int accumulate);
// LocallyConnected2D 1x1: y[n,h,w,f] = b[h,w,f] + sum_c x[n,h,w,c] W[h,w,c,f]
void localconv_forward(hipStream_t s, const TView& x, const float* w, const float* b, const TView& y);
void localconv_backward(hipStream_t s, const TView& x, const float* w, const TView& dy, const TView& dx,
                        int accumulate_dx, float* dw, float* db, int accumulate_dw);

// --------------------------------------------------------- channel attention (attention.hip)
// x viewed as [G][R][Q]: mean over R, MLP over the last C channels of Q=(P*C), scale.
struct AttShape { int G, R, P, C, Cr; };
// pool_partial (optional): [G][pool_tiles][8] per-tile channel sums emitted by the producing convolution (ConvEpilogue::pool)
// -> no pooling pass over x.  y == nullptr: the scale is not applied here (the consumer reads x through TView::sc = scale).
void chatt_forward(hipStream_t s, const float* x, float* y, const AttShape& sh, const float* w1,
                   const float* b1, const float* w2, const float* b2, float* mean, float* hidden,
                   float* scale, float* workspace, const float* pool_partial = nullptr, int pool_tiles = 0,
                   const float* given_mean = nullptr);      // given_mean [G][C] (P == 1): used instead of the pooled mean (tiles.hip)
// dx == nullptr: dX = dY * scale + dmean is not materialised; dmean is left in dmean_out ([G*P*C], caller-owned) for the
// producer's lazy dY view (TView::sc = scale, TView::sh = dmean)
void chatt_backward(hipStream_t s, const float* x, const float* dy, float* dx, int accumulate_dx,
                    const AttShape& sh, const float* w1, const float* w2, const float* mean,
                    const float* hidden, const float* scale, float* dw1, float* db1, float* dw2,
                    float* db2, int accumulate_dw, float* workspace, float* dmean_out = nullptr,
                    const float* ds_given = nullptr);     // ds_given ([G*P*C]): sum_r(dy * x) already known -> no pass over dy, x
size_t chatt_workspace_bytes(const AttShape& sh);

// ----------------------------------------------------------------------- losses (losses.hip)
enum LossKind { LOSS_MAE = 0, LOSS_MSE = 1, LOSS_DSSIM = 2, LOSS_DSSIM_MAE = 3, LOSS_DSSIM_MSE = 4,
                LOSS_DSSIM_MAE_MSE = 5, LOSS_MSDSSIM = 6, LOSS_MSDSSIM_MAE = 7, LOSS_MSDSSIM_MAE_MSE = 8 };
// loss_out[0] = scale * loss ; dpred (+)= scale * dloss/dpred.  y_true,y_pred: (N,H,W,C) contiguous.
size_t loss_workspace_bytes(int kind, int N, int H, int W, int C);
void loss_forward_backward(hipStream_t s, int kind, const float* y_true, const float* y_pred,
                           float* dpred, int N, int H, int W, int C, float scale, float* loss_out,
                           int accumulate, float* workspace, size_t workspace_bytes);
// The same with per-grid-cell weights w (contract at the top of losses.hip): w_batch maps of (H, W, w_channels), w_batch divides N
// (sample row r uses map r / (N / w_batch)), w_channels in {1, C}.  The msdssim kinds are refused.  The unweighted workspace figure
// is unchanged; the weighted call needs loss_workspace_bytes_weighted.
size_t loss_workspace_bytes_weighted(int kind, int N, int H, int W, int C, int w_batch, int w_channels);
void loss_forward_backward_weighted(hipStream_t s, int kind, const float* y_true, const float* y_pred, float* dpred, int N,
                                    int H, int W, int C, float scale, float* loss_out, int accumulate, const float* w,
                                    int w_batch, int w_channels, float* workspace, size_t workspace_bytes);
// BCE on probabilities p[n] vs constant label; loss_out[0] (+)= scale*mean ; dp = scale*dL/dp
void bce_forward_backward(hipStream_t s, const float* p, float label, int n, float scale,
                          float* loss_out, float* dp, int accumulate_loss);

// -------------------------------------------------------------------------- optimiser (adam.hip)
// Keras Adam on a flat arena. lr_t = lr*sqrt(1-b2^t)/(1-b1^t) computed by the caller.
void adam_update(hipStream_t s, float* w, const float* g, float* m, float* v, size_t n, float lr_t,
                 float beta1, float beta2, float eps, float grad_scale, const unsigned* err_word = nullptr);   // err_word: see runtime.h
// The same step with global-norm clipping, decoupled weight decay and a weight average (adam_ext.hip; at most two launches).
//   clipnorm 0: no clipping (no norm launch, factor 1);  weight_decay applies inside the table `bounds_dev` (decay_bounds, uploaded by
//   the caller; null or n_bounds 0: nowhere) with the plain scheduled `lr`;  ema null: no average.
//   partials_dev: sqnorm_blocks(n) doubles (clipping only);  stats_dev: [0] fl32 norm (0 without clipping) [1] clip factor
//   [2] count of steps skipped for a non-finite norm, a 32-bit unsigned integer that the kernel increments in place.
void adam_ext_update(hipStream_t s, float* w, const float* g, float* m, float* v, float* ema, size_t n, float lr_t, float beta1,
                     float beta2, float eps, float grad_scale, float clipnorm, float lr, float weight_decay, const size_t* bounds_dev,
                     int n_bounds, float ema_momentum, double* partials_dev, float* stats_dev, const unsigned* err_word = nullptr);
int sqnorm_blocks(size_t n);                  // blocks (= fp64 partials) of the norm launch: a function of n alone, at most 1024
// [begin, end) element ranges of an arena of n (any order, may touch or overlap) -> the sorted bounds b0 < e0 < b1 < e1 < ...
std::vector<size_t> decay_bounds(const size_t* ranges, int n_ranges, size_t n);
void arena_swap(hipStream_t s, float* a, float* b, size_t n);         // exchanges two arenas element by element (exact)

// ------------------------------------------------------------- batch preparation (batchprep.hip), "next" row f1
// Gathers one training batch from a device-resident dataset: block-mean coarsening (cv2 INTER_AREA at an integer
// ratio), pixel replication back to the HR grid for 'pin', crops, predictor / static-variable channel stacking.
// idx / cy / cx are DEVICE int arrays of length B (first frame, crop corner in HR pixels).
void batch_prepare(hipStream_t s, const float* hr, const float* pred, const float* stat, const int* idx, const int* cy,
                   const int* cx, float* out_lr, float* out_hr, float* out_stat, int H, int W, int C, int P, int S, int T,
                   int B, int scale, int psy, int psx, int pin, int static_in_lr);
// One axis of a separable cv2.resize: k (source index, weight) taps per output row / column, device arrays [n_out][k].
struct TapAxis { const int* idx; const float* wt; int k; };
// The same for any interpolation (see batchprep.hip): each table argument is {y axis, x axis}.
void batch_prepare_taps(hipStream_t s, const float* hr, const float* pred, const float* stat, const int* idx, const int* cy,
                        const int* cx, float* out_lr, float* out_hr, float* out_stat, float* scratch, int H, int W, int C,
                        int P, int S, int T, int B, int scale, int psy, int psx, int pin, int static_in_lr,
                        const TapAxis* dn_patch, const TapAxis* dn_field, const TapAxis* up_field);
// one gather pass over up to three channel groups (raw crops or separable tap tables): the primitive behind both of the above
struct GatherGroup { const float* src; int channels, frames, src_h, src_w, raw, origin_from_crop, row_div; TapAxis taps[2]; };
void batch_gather(hipStream_t s, const GatherGroup* groups, int n_groups, const int* idx, const int* cy, const int* cx, float* out,
                  int out_h, int out_w, int T, int B);
void repeat_time_forward(hipStream_t s, const float* in, float* out, int B, int T, size_t ps);
void repeat_time_forward_view(hipStream_t s, const float* in, const TView& out, int B, int T);     // out: (B*T, H, W, C) view, any pixel pitch
void repeat_time_backward(hipStream_t s, const float* dout, float* din, int B, int T, size_t ps, int accumulate);
void repeat_time_backward_view(hipStream_t s, const TView& dout, float* din, int B, int T, int accumulate);   // dout: slice view
void resize_table_forward(hipStream_t s, const TView& x, const TView& y, const int* iy, const float* wy, const int* ix, const float* wx,
                          int ky, int kx);   // [out][k] taps per axis
void resize_table_backward(hipStream_t s, const TView& dy, const TView& dx, const int* py, const int* oy, const float* vy,
                           const int* px, const int* ox, const float* vx, int accumulate, int max_taps_x = 0);
