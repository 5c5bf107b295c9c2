/* dl4ds_hip.h -- C ABI of libdl4ds_hip.so: the MI355X (gfx950) native replacement for the
 * TensorFlow/Keras + Horovod arithmetic behind dl4ds's conv-SR train step.
 *
 * The reference (carlos-gg/dl4ds 1.8.0) has NO plugin / FFI interface: its hot path sits behind plain
 * Python (`dl4ds.models.*` builders returning tf.keras.Model; `SupervisedTrainer.run`, `CGANTrainer.run`,
 * `Predictor.run`).  The entry points below are what a ctypes binding for that path needs; each names the
 * reference code it replaces (paths relative to the reference repo).  The Python mirror that binds them is
 * dl4ds_amd/ (same builder / trainer signatures as the reference).
 *
 * Conventions: every function returns 0 on success, <0 on error (message: dl4ds_last_error()); no C++
 * exception crosses the boundary; all tensors are fp32 NHWC ("channels_last"), conv kernels HWIO,
 * transposed-conv kernels HWOI, dense kernels [in][out]; pointers named *_dev are device (HBM) pointers,
 * *_host are host pointers; sizes are element counts unless called bytes.  One library-wide HIP stream;
 * calls are asynchronous unless documented otherwise.  ONE HOST THREAD per process drives the library (one process per GPU): the profiler and a few run-time statics are unsynchronised.
 */
#ifndef DL4DS_HIP_H
#define DL4DS_HIP_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct dl4ds_graph dl4ds_graph;
typedef struct dl4ds_trainer dl4ds_trainer;

/* ---------------------------------------------------------------- runtime / memory (plumbing)
 * replaces: tf.config device selection, dl4ds/utils.py:174-203; training/base.py:97-122 */
const char* dl4ds_last_error(void);
int dl4ds_init(int device);                       /* hipSetDevice + create the library stream */
int dl4ds_device_count(int* n);
int dl4ds_device_name(char* buf, int buflen);
int dl4ds_malloc(void** p_dev, size_t bytes);
int dl4ds_free(void* p_dev);
int dl4ds_memcpy_h2d(void* dst_dev, const void* src_host, size_t bytes);   /* synchronous */
int dl4ds_memcpy_d2h(void* dst_host, const void* src_dev, size_t bytes);   /* synchronous */
int dl4ds_memcpy_d2d(void* dst_dev, const void* src_dev, size_t bytes);    /* async on the stream */
/* Page-lock a host buffer the caller owns for the duration of a run of host <-> device copies (hipHostRegister / hipHostUnregister):
 * copies to / from it then go at the link's rate instead of through the runtime's staging of pageable memory.  Used by
 * Model.predict for the array it returns (inference.py:238-249 hands numpy arrays in and out).  register returns non-zero when the
 * range cannot be pinned (the caller simply goes on with pageable copies). */
int dl4ds_host_register(void* p_host, size_t bytes);
int dl4ds_host_unregister(void* p_host);
int dl4ds_memset(void* p_dev, int value, size_t bytes);
int dl4ds_sync(void);                             /* hipStreamSynchronize(library stream); fails if a kernel raised the
                                                   * sticky device-side error word since the last wait (e.g. the persistent
                                                   * ConvLSTM kernel gave up waiting for a neighbouring tile: that step is invalid) */
/* diagnostic: a one-thread kernel on the library stream raises the device-side error word with `code` exactly as a kernel
 * would; the next host-side wait (dl4ds_sync, a loss read-back ...) must fail once and clear it.  No reference counterpart
 * (TensorFlow reports device-side failures through its own status plumbing). */
int dl4ds_debug_raise_device_error(int code);
int dl4ds_event_timer_start(void);                /* hipEventRecord on the library stream */
int dl4ds_event_timer_stop(float* ms);            /* record + synchronize + elapsed ms */
/* per-launch HIP-event timing on the library stream (off by default).  report: JSON
 * {"<kernel tag>": {"n": launches, "ms": total, "flops": algorithmic, "bytes": algorithmic}, ...};
 * synchronises and clears the log. */
int dl4ds_profile_enable(int on);
/* restrict the timing to launches whose tag starts with `tag_prefix` (NULL / "" = all): lets a benchmark time its
 * dominant kernel inside the measured region without paying two events for every other launch */
int dl4ds_profile_filter(const char* tag_prefix);
int dl4ds_profile_report(char* json_buf, size_t buflen);

/* ---------------------------------------------------------------- single-op entry points
 * (unit-testable against the oracle; contiguous NHWC device tensors) */

/* y = [relu](conv_same_s1(x,w) + b + add), optionally stored through depth_to_space(d2s_r).
 * replaces tf.keras.layers.Conv2D (blocks.py:49-61,208,249-259,299,414-416,479; sp_postups.py:134,156)
 * fused with Add (blocks.py:228), Activation (blocks.py:75) and tf.nn.depth_to_space (blocks.py:427). */
int dl4ds_op_conv2d_fwd(const float* x_dev, const float* w_dev, const float* b_dev, const float* add_dev,
                        float* y_dev, int N, int H, int W, int Cin, int Cout, int KS, int relu, int d2s_r);
/* The same convolution with EVERY operand of the fused epilogue, in the order the train step applies them:
 * y = [y_old +] mask_gt0( [relu]( conv_same_s1(x,w) + b + add ), mask ) -- residual Add (blocks.py:228), Activation
 * (blocks.py:75), the ReLU backward of the layer below riding on a dgrad store (mask = that layer's activation) and gradient
 * accumulation.  The narrow kernels compile one form per operand combination (csrc/conv_narrow.hip); this entry point lets a
 * test reach all of them.  b, add, mask may be NULL; accumulate != 0 adds the result to what y holds. */
int dl4ds_op_conv2d_epilogue(const float* x_dev, const float* w_dev, const float* b_dev, const float* add_dev,
                             const float* mask_dev, float* y_dev, int N, int H, int W, int Cin, int Cout, int KS, int relu,
                             int accumulate);
/* The convolution with a second output pair, as the graph uses it around the long skip `s + relu(conv)` of the residual backbone
 * (sp_postups.py:154-158), on the kernel dl4ds_op_conv2d_epilogue picks for the same call without the pair:
 *   sum_add, sum_out:      y = act(conv(x, w) + b) and sum_out = sum_add + y (the Add that follows the layer);
 *   mask, mask2, y2:       y = conv * [mask > 0], y2 = conv * [mask2 > 0] (the backward of that Add over two ReLU outputs, from the
 *                          dgrad that makes its output gradient); `partial` (N*H*W*Cout floats) takes the raw partial sums when the
 *                          kernel makes more than one pass over the input channels.
 * One pair per call; all arrays (N,H,W,Cout).  *launched = 0: that kernel has no such form and nothing was written. */
int dl4ds_op_conv2d_second_output(const float* x_dev, const float* w_dev, const float* b_dev, const float* sum_add_dev,
                                  float* sum_out_dev, const float* mask_dev, const float* mask2_dev, float* y2_dev,
                                  float* partial_dev, float* y_dev, int N, int H, int W, int Cin, int Cout, int KS, int relu,
                                  int* launched);
/* out = [relu](a + b) over n floats -- tf.keras.layers.Add (sp_postups.py:158), the stand-alone pass */
int dl4ds_op_add_act(const float* a_dev, const float* b_dev, float* out_dev, size_t n, int relu);
/* da = dy * [ya > 0], db = dy * [yb > 0] over n floats: the backward of an Add of two ReLU outputs, the stand-alone pass.
 * *launched = 0: n % 4 != 0 or an operand is not 16-byte aligned, nothing was written. */
int dl4ds_op_masked_axpy_pair(const float* dy_dev, const float* ya_dev, float* da_dev, const float* yb_dev, float* db_dev,
                              size_t n, int* launched);
/* dx (+)= dgrad(dz, w); dz may be given in depth_to_space(d2s_r) layout (gradient of a fused-d2s conv) */
int dl4ds_op_conv2d_dgrad(const float* dz_dev, const float* w_dev, float* dx_dev, int N, int H, int W,
                          int Cin, int Cout, int KS, int d2s_r, int accumulate);
/* dw (+)= wgrad(x, dz) */
int dl4ds_op_conv2d_wgrad(const float* x_dev, const float* dz_dev, float* dw_dev, int N, int H, int W,
                          int Cin, int Cout, int KS, int d2s_r, int accumulate);
/* One operand of a convolution as the train graph passes it (csrc/common.h: TView): `C` logical channels at a pitch of `ld` floats
 * per pixel (0: dense, ld = C; > C: a channel slice of a wider buffer, p already at the slice's first channel -- the outputs and
 * inputs that live inside a Concatenate's buffer, blocks.py:228 / sp_preups.py:262-285), images `nstride` floats apart (0:
 * contiguous; T*H*W*C: frame t of every sample of a (B,T,H,W,C) buffer, p already at frame t -- the TimeDistributed layers of
 * spt_postups.py:152-157), d2s > 1: the memory holds tf.nn.depth_to_space(d2s) of the logical tensor (blocks.py:427), sc / sh
 * (read operands only, may be NULL; sh needs sc): per-image channel affine, logical value = mem * sc[n*C + c] + sh[n*C + c] inside
 * the image, zero padding outside -- ChannelAttention2D's broadcast scale (blocks.py:585-593) and its backward carried in the
 * neighbouring convolution's loads.  float4 access is decided by the same rule as for the graph's own views. */
typedef struct dl4ds_view {
    const float* p;
    int C, ld, d2s;
    size_t nstride;
    const float* sc;
    const float* sh;
} dl4ds_view;
/* dl4ds_op_conv2d_epilogue on such views: y = [y_old +] mask_gt0( [relu]( conv_same_s1(x,w) + b + add ), mask ) with x, add, mask
 * read and y written through their descriptors (Conv2D + Add + Activation, blocks.py:49-75,228).  dgrad != 0: w is the FORWARD
 * layer's [KS][KS][y.C][x.C] filter and the call is that layer's input gradient (x = dz).  A view form the kernels cannot take
 * (a channel affine outside the stencil / narrow-pair kernels) is an error, never ignored. */
int dl4ds_op_conv2d_views(const dl4ds_view* x, const float* w_dev, const float* b_dev, const dl4ds_view* add, const dl4ds_view* mask,
                          const dl4ds_view* y, int N, int H, int W, int KS, int relu, int accumulate, int dgrad);
/* dw (+)= wgrad(x, dz) and, with db_dev, db (+)= sum_pixels dz (the bias gradient of Conv2D(use_bias=True), blocks.py:49-61, which
 * every weight-gradient kernel family produces on the side); accumulate and accumulate_db are independent. */
int dl4ds_op_conv2d_wgrad_views(const dl4ds_view* x, const dl4ds_view* dz, float* dw_dev, int N, int H, int W, int KS, int accumulate,
                                float* db_dev, int accumulate_db);
/* Weight gradient of a stencil convolution that reads its input through ChannelAttention2D's scale, y = conv(x * scale[n, ci])
 * (blocks.py:585-593), together with the attention's d(loss)/d(scale): dw (+)= wgrad(x * scale, dz), db (+)= sum dz (db_dev may be
 * NULL), ds[n, ci] = sum_p x[n,p,ci] * dgrad(dz, w)[n,p,ci].  x is the RAW input.  *launched = 0: the layer is not one the stencil
 * kernels take, nothing was written. */
int dl4ds_op_conv2d_wgrad_attention(const dl4ds_view* x, const dl4ds_view* dz, const float* scale_dev, const float* w_dev, float* dw_dev,
                                    int N, int H, int W, int KS, int accumulate, float* db_dev, int accumulate_db, float* ds_dev,
                                    int* launched);
/* dz = dy * [y>0] (if y_dev) in place over dy; db = sum_pixels dz (if db_dev) */
int dl4ds_op_bias_act_bwd(float* dy_dev, const float* y_dev, float* db_dev, int N, int H, int W, int C);
/* Conv2DTranspose(k=KS, stride, 'same', use_bias=False) -- blocks.py:508-516; kernel HWOI */
int dl4ds_op_conv2d_transpose_fwd(const float* x_dev, const float* w_dev, float* y_dev, int N, int H, int W,
                                  int Cin, int Cout, int KS, int stride, int relu);
int dl4ds_op_conv2d_transpose_dgrad(const float* dz_dev, const float* w_dev, float* dx_dev, int N, int H,
                                    int W, int Cin, int Cout, int KS, int stride, int accumulate);
int dl4ds_op_conv2d_transpose_wgrad(const float* x_dev, const float* dz_dev, float* dw_dev, int N, int H,
                                    int W, int Cin, int Cout, int KS, int stride, int accumulate);
/* tf.nn.depth_to_space / its adjoint -- blocks.py:427 */
int dl4ds_op_depth_to_space(const float* x_dev, float* y_dev, int N, int H, int W, int C, int r);
int dl4ds_op_space_to_depth(const float* y_dev, float* x_dev, int N, int H, int W, int C, int r);
/* MaxPooling2D((2,2)) -- blocks.py:613 */
int dl4ds_op_maxpool2_fwd(const float* x_dev, float* y_dev, int N, int H, int W, int C);
int dl4ds_op_maxpool2_bwd(const float* x_dev, const float* y_dev, const float* dy_dev, float* dx_dev, int N,
                          int H, int W, int C);
/* DepthwiseConv2D(kernel_size=7, padding='same', depth_multiplier=1) -- ConvNextBlock.dwconv, blocks.py:143-144.
 * k: (7,7,C) taps (Keras (7,7,C,1)), bias (C) or NULL.  bwd: dx / dk (+ db) may be NULL; accumulate adds into them. */
int dl4ds_op_dwconv_fwd(const float* x_dev, const float* k_dev, const float* bias_dev, float* y_dev, int N, int H, int W, int C,
                        int KS);
int dl4ds_op_dwconv_bwd(const float* x_dev, const float* k_dev, const float* dy_dev, float* dx_dev, float* dk_dev, float* db_dev,
                        int N, int H, int W, int C, int KS, int accumulate);
/* LayerNormalization(axis=-1) / BatchNormalization(axis=-1) over [npix][C] -- blocks.py:63-71,151-159,293-296.
 * relu: fuse the activation that follows.  bwd: y is only read when relu != 0; dx / dgamma / dbeta may be NULL;
 * accumulate != 0 adds into dx, dgamma, dbeta.  batchnorm: `saved` (2*C floats: batch mean, 1/std) is written by a
 * training-mode forward and read by the backward; moving statistics are updated in place when training. */
int dl4ds_op_layernorm_fwd(const float* x_dev, const float* gamma_dev, const float* beta_dev, float* y_dev, size_t npix, int C,
                           float eps, int relu);
int dl4ds_op_layernorm_bwd(const float* x_dev, const float* y_dev, const float* dy_dev, const float* gamma_dev, float* dx_dev,
                           float* dgamma_dev, float* dbeta_dev, size_t npix, int C, float eps, int relu, int accumulate);
int dl4ds_op_batchnorm_fwd(const float* x_dev, const float* gamma_dev, const float* beta_dev, float* moving_mean_dev,
                           float* moving_var_dev, float* y_dev, float* saved_dev, size_t npix, int C, float eps,
                           float momentum, int training, int relu);
int dl4ds_op_batchnorm_bwd(const float* x_dev, const float* y_dev, const float* dy_dev, const float* gamma_dev,
                           const float* saved_dev, float* dx_dev, float* dgamma_dev, float* dbeta_dev, size_t npix, int C,
                           int relu, int accumulate);
/* Resizing(..., 'bilinear') -- blocks.py:489; discriminator.py:62-63 */
int dl4ds_op_resize_bilinear_fwd(const float* x_dev, float* y_dev, int N, int H, int W, int C, int Ho, int Wo);
int dl4ds_op_resize_bilinear_bwd(const float* dy_dev, float* dx_dev, int N, int H, int W, int C, int Ho, int Wo);
/* LocallyConnected2D(F,(1,1),implementation=3) -- blocks.py:322-328 */
int dl4ds_op_localconv_fwd(const float* x_dev, const float* w_dev, const float* b_dev, float* y_dev, int N,
                           int H, int W, int C, int F);
int dl4ds_op_localconv_bwd(const float* x_dev, const float* w_dev, const float* dy_dev, float* dx_dev,
                           float* dw_dev, float* db_dev, int N, int H, int W, int C, int F);
/* ChannelAttention2D -- blocks.py:585-593.  x is [G][R][P*C] (4-D: G=B,R=H*W,P=1; 5-D: G=B,R=T*H,P=W).
 * saved_dev: G*P*(2C+Cr) floats written by fwd and consumed by bwd. */
int dl4ds_op_chatt_fwd(const float* x_dev, float* y_dev, int G, int R, int P, int C, int Cr, const float* w1_dev,
                       const float* b1_dev, const float* w2_dev, const float* b2_dev, float* saved_dev);
int dl4ds_op_chatt_bwd(const float* x_dev, const float* dy_dev, float* dx_dev, int G, int R, int P, int C, int Cr,
                       const float* w1_dev, const float* w2_dev, const float* saved_dev, float* dw1_dev,
                       float* db1_dev, float* dw2_dev, float* db2_dev);
/* dl4ds/losses.py:5-149.  kind: 0 mae 1 mse 2 dssim 3 dssim_mae 4 dssim_mse 5 dssim_mae_mse
 * 6 msdssim 7 msdssim_mae 8 msdssim_mae_mse (tf.image.ssim_multiscale, four scales: grids of at least 81x81).
 * loss_dev[0] = loss ; dpred_dev = dloss/dpred (may be NULL). */
int dl4ds_op_loss(int kind, const float* y_true_dev, const float* y_pred_dev, float* dpred_dev, int N, int H,
                  int W, int C, float* loss_dev);
/* The same as the trainers call it: loss_dev[0] = scale * loss (the cGAN's lambda); dpred_dev = scale * dloss/dpred, ADDED to what
 * dpred_dev holds when accumulate != 0 (the drange and min-shift terms of the SSIM kinds included).  scale = 1, accumulate = 0 is
 * dl4ds_op_loss bit for bit. */
int dl4ds_op_loss_scaled(int kind, const float* y_true_dev, const float* y_pred_dev, float* dpred_dev, int N, int H,
                         int W, int C, float scale, int accumulate, float* loss_dev);
/* dl4ds_op_loss with per-grid-cell weights (masks, cos(latitude) area weights).  w_dev: float32, finite, >= 0, w_batch maps of
 * (H, W, w_channels); w_batch must DIVIDE N and sample row r of the (N, H, W, C) batch uses map r / (N / w_batch) -- 1: one map shared by
 * all samples, N: one map per sample (patch training), N / nmul: one map per sample of a spatio-temporal output of nmul frames;
 * w_channels is 1 (the map serves every channel) or C.  With d = p - t and sums over all N*H*W*C entries (w broadcast):
 *   mae_w = sum w|d| / sum w,  mse_w = sum w d^2 / sum w  (gradient 0 at d == 0; w == const > 0 reproduces the unweighted loss).
 * An entry with w == 0 is excluded by selection: neither y_true nor y_pred there enters any sum and its gradient is exactly +0.0,
 * also where y_true is NaN or Inf (MAE and MSE terms of every kind).  sum w == 0: loss 0 and dpred all zeros, never NaN.
 * dssim kinds (2..5): window weights omega = G * w (G: the 11x11 Gaussian of the moments) over the VALID windows,
 * term = sum omega (1 - ssim)/2 / sum omega over samples, windows and channels, windows with omega == 0 excluded; the dynamic range and
 * positivity shift are those of the whole arrays as in the unweighted loss, so y_true must be finite everywhere for these kinds; the
 * mixes keep 0.8/0.2 and 0.6/0.2/0.2 over the weighted terms.  The multi-scale kinds (6..8) are refused.  Bitwise reproducible. */
int dl4ds_op_loss_weighted(int kind, const float* y_true_dev, const float* y_pred_dev, float* dpred_dev, int N, int H,
                           int W, int C, const float* w_dev, int w_batch, int w_channels, float* loss_dev);
/* compute_metrics (metrics.py:166-262) without the plots, on device-resident test arrays (N,H,W,C):
 *   pair_out_dev  [N][4]       per test pair: MAE, MSE, Pearson correlation over the grid, SSIM (tf.image.ssim with the
 *                              joint dynamic range; NaN when the grid is smaller than the 11x11 window).
 *                              PSNR = 10 log10(range^2 / MSE) follows on the host (tf.image.psnr, metrics.py:168-169)
 *   grid_out_dev  [3][H*W*C]   per grid point over the pairs: RMSE (metrics.py:188), mean bias (:219), Pearson (:247)
 *   range_out_dev [2]          joint (min, max) of both arrays (metrics.py:166) */
int dl4ds_metrics(const float* y_true_dev, const float* y_pred_dev, int N, int H, int W, int C, float* pair_out_dev,
                  float* grid_out_dev, float* range_out_dev);
/* Spearman rank correlation of compute_correlation (metrics.py:51-97), scipy.stats.spearmanr semantics on 1-D inputs: for every
 * pair s < S, out_dev[s] (fp64) = Pearson correlation of the average ranks (ties share the mean of their positions; -0.0 ties
 * with +0.0) of the two length-L sequences whose element k lives at a_dev / b_dev [s*seg_stride + k*elem_stride]; NaN when
 * either sequence holds a NaN (nan_policy='propagate'), is constant, or L < 2.  Per test pair: S = N, L = H*W*C,
 * seg_stride = L, elem_stride = 1; per grid point of channel 0: S = H*W, L = N, seg_stride = C, elem_stride = H*W*C.
 * Bitwise reproducible.  L < 2^28. */
int dl4ds_spearman(const float* a_dev, const float* b_dev, size_t S, size_t L, size_t seg_stride, size_t elem_stride,
                   double* out_dev);
/* MinMaxScaler / StandardScaler -- preprocessing.py:78-117 (MinMaxScaler.partial_fit: nan mask, np.nanmin / np.nanmax),
 * :247-283 (StandardScaler.partial_fit: np.nanmean / np.nanstd), :120-167 and :285-334 (transform / inverse_transform).
 * x_dev: a C-contiguous device array of ndim <= 8 axes (host arrays shape[ndim], reduce[ndim]; reduce[i] != 0: axis i is
 * reduced), float (is_double = 0) or double; after dropping size-1 axes and merging neighbours of one kind at most five groups.
 * dl4ds_scaler_stats: ONE read of x.  out_dev [5][cells] fp64, cells = product of the kept extents in C order (keepdims layout):
 *   count of non-NaN values, min, max, mean, population standard deviation (ddof 0) of every kept cell with NaNs skipped; an
 *   all-NaN cell gives count 0 and NaN.  nan_flag_dev [1]: 1 if any element was NaN.  mask_bits_dev (or null): the NaN mask,
 *   bit e%32 of word e/32 for flat element e, (n + 31) / 32 words.  fp64 accumulation, no floating-point atomics: bitwise
 *   reproducible.
 * dl4ds_scaler_apply: out[e] = op2(op1(x[e], a[cell(e)]), b[cell(e)]) in the array's own type, every operation rounded on its own
 *   like numpy's in-place `*=`, `+=`, `-=`, `/=` (op: 0 none, 1 multiply, 2 add, 3 subtract, 4 divide; a_dev / b_dev [cells] in
 *   the array's type, null for op 0); then nan_mode 0: NaN -> fill (np.nan_to_num(nan=fillnanto)), nan_mode 1: NaN where the bit
 *   of mask_bits_dev (or null) is set (X[nan_mask] = np.nan).  out_dev may be x_dev. */
int dl4ds_scaler_cells(const size_t* shape, int ndim, const int* reduce, size_t* cells_out);
int dl4ds_scaler_stats_workspace_bytes(const size_t* shape, int ndim, const int* reduce, int is_double, size_t* bytes_out);
int dl4ds_scaler_stats(const void* x_dev, int is_double, const size_t* shape, int ndim, const int* reduce, double* out_dev,
                       unsigned* nan_flag_dev, unsigned* mask_bits_dev);
int dl4ds_scaler_apply(const void* x_dev, void* out_dev, int is_double, const size_t* shape, int ndim, const int* reduce, int op1,
                       const void* a_dev, int op2, const void* b_dev, int nan_mode, double fill, const unsigned* mask_bits_dev);
/* Member statistics of an MC-dropout ensemble.  Serves the MCDropout / MCGaussianDropout / MCSpatialDropout layers of
 * blocks.py:658-676, which stay active at inference so that K forward passes of one input form an ensemble (the reference leaves
 * the loop and the reduction to the user).  members_dev: K rows of n fp32 values, row k at members_dev + k * member_stride
 * (member_stride >= n, in elements), 1 <= K <= 256.  ONE read of the stack writes, per element e < n (any output may be null and
 * is then skipped): mean_dev[e], std_dev[e] (population, ddof 0), min_dev[e], max_dev[e], and quant_dev[j * n + e] for the nq <= 32
 * probabilities q_host[j] in [0, 1]: np.quantile's default 'linear' method on the sorted K values.  Everything is evaluated as
 * numpy does on the fp64 copy of the stack (sequential fp64 two-pass mean / std in member order, fp64 interpolation between the two
 * fp32 order statistics) and rounded to fp32 once; a NaN among the K values makes every output of that element NaN, infinities
 * give what those formulas give.  No atomics: bitwise reproducible.  Algorithmic traffic (K + 4 + nq) * 4 * n bytes. */
int dl4ds_ensemble_reduce(const float* members_dev, size_t K, size_t n, size_t member_stride, const float* q_host, int nq,
                          float* mean_dev, float* std_dev, float* min_dev, float* max_dev, float* quant_dev);
/* Verification of an MC-dropout ensemble against an observation.  Serves the same MC* layers of blocks.py:658-676: the reference
 * defines them and leaves both the ensemble loop and its verification to the user.  members_dev as for dl4ds_ensemble_reduce
 * (K rows of n fp32 values, row k at members_dev + k * member_stride, 1 <= K <= 256); obs_dev [n]: the observation; the n
 * elements are B whole samples of per = n / B cells (n % B == 0), the first of them element elem_offset of the whole data set
 * (elem_offset % per == 0); scale_dev (or null) [per]: a positive factor per cell that carries the scores into physical units.
 * An element e is VALID iff obs[e] and its K members are finite (no NaN, no infinity) and, with a scale, scale[e % per] is finite
 * and > 0.  An invalid element gets NaN (rank -1) in the per-element outputs and takes no part in any sum, count or histogram: NaN
 * in obs_dev is the masking mechanism.  ONE read of the stack computes per element, each value in fp64 on the fp32 inputs, rounded
 * to fp32 once:
 *   crps_dev[e]  = (1/K) sum_k |x_k - y| - c sum_{i<j} |x_i - x_j|, c = 1/K^2 (CRPS of the empirical distribution) or, fair != 0,
 *                  c = 1/(K (K - 1)) (fair CRPS); K = 1: |x_0 - y|.  The pair term is evaluated from the sorted differences
 *                  d_k = x_k - y as sum_i (2 i - K + 1) d_(i), so cancellation scales with the ensemble's distance from the
 *                  observation, not with the field's magnitude.  Times scale.
 *   sqerr_dev[e] = (mean_k x_k - y)^2, var_dev[e] = sum_k (x_k - mean)^2 / (K - 1) (K = 1: 0); times scale^2.
 *   rank_dev[e]  = #{k : x_k < y} + tie(seed, g, m), m = #{k : x_k == y} (-0.0 == +0.0), g = elem_offset + e, and with all
 *                  arithmetic on unsigned 64-bit integers (mod 2^64):
 *                    z = seed + 0x9E3779B97F4A7C15 * (g + 1);  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9;
 *                    z = (z ^ (z >> 27)) * 0x94D049BB133111EB;  z = z ^ (z >> 31);  tie = ((z >> 32) * (m + 1)) >> 32
 *                  (splitmix64 of (seed, g); one of 0 ... m, 0 when m = 0): random tie-breaking that is a pure function of
 *                  (seed, g, m) and so does not depend on how the samples were split into calls.
 *   covered_j[e] = [y <= Q_j] for the nq <= 32 probabilities q_host[j] in [0, 1], Q_j the fp32 'linear' quantile that
 *                  dl4ds_ensemble_reduce writes.
 * Folds over the valid elements (each may be null; the per-element outputs too):
 *   sample_out_dev [B][4]: fp64 sums of crps, sqerr, var over sample b and its valid count, overwritten;
 *   cell_acc_dev [4][per]: the same four per cell, ADDED ONTO the accumulators, samples in ascending order, so that the result
 *                  after all calls does not depend on the number of samples per call;
 *   rank_hist_dev [K + 1], covered_dev [nq] (required when nq > 0): 64-bit counts, ADDED (integer atomics).
 * The accumulators are zeroed by the caller (dl4ds_memset).  No floating-point atomics: a repeated call gives the same bits.
 * Algorithmic traffic (K + 1) * 4 * n bytes read plus a hand-over of five 4-byte words per element written and read once. */
int dl4ds_ensemble_score(const float* members_dev, size_t K, size_t n, size_t member_stride, const float* obs_dev, size_t B,
                         unsigned long long elem_offset, const float* scale_dev, int fair, unsigned long long seed,
                         const float* q_host, int nq, float* crps_dev, float* sqerr_dev, float* var_dev, int* rank_dev,
                         double* sample_out_dev, double* cell_acc_dev, unsigned long long* rank_hist_dev,
                         unsigned long long* covered_dev);
/* Exceedance-probability verification of an MC-dropout ensemble against an observation at T thresholds.  Serves the same MC*
 * layers of blocks.py:658-676: the reference defines them and leaves both the ensemble loop and its verification to the user; the
 * definitions are DESIGN.md section 17.  members_dev, K, n, member_stride, obs_dev and B as for dl4ds_ensemble_score: K rows of n
 * fp32 values (row k at members_dev + k * member_stride, 1 <= K <= 256), the observation obs_dev [n], the n elements being B whole
 * samples of per = n / B cells.  thr_dev: the 1 <= T <= 16 thresholds, a DEVICE array; thr_per_cell == 0: [T] values, thr(t, e) =
 * thr_dev[t]; otherwise [T][per], a threshold field per cell (a local climatological percentile), thr(t, e) = thr_dev[t * per +
 * e % per].  Thresholds may come in any order and may repeat.
 * Element e is VALID for threshold t iff obs[e] and all K members are finite (no NaN, no infinity) and thr(t, e) is finite: NaN in
 * obs_dev is the masking mechanism, a NaN threshold excludes its cell for that threshold only.  Per valid (t, e), every comparison on
 * float32 (-0.0 equals +0.0):
 *   o = [obs[e] >= thr(t, e)]            the event was observed
 *   c = #{k : x_k[e] >= thr(t, e)}       0 ... K members forecast it: the forecast probability is c / K
 * Outputs (each may be null and is then skipped):
 *   count_dev      [T][n]        int16: c, or -1 where invalid; overwritten
 *   sample_out_dev [B][T][4]     int64: per sample n_valid, sum o, sum c, sum (c - K o)^2 (K^2 n_valid times its Brier score);
 *                                overwritten
 *   cell_acc_dev   [T][4][per]   int64: the same four per cell, ADDED onto accumulators that the caller has zeroed
 *   table_dev      [T][K + 1][2] uint64: the number of valid elements with c = i and o = 0 / 1, ADDED
 * Integer arithmetic only (integer atomics, no floating-point accumulation anywhere): the sums equal an integer reference and do
 * not depend on the order of the atomics, on how the samples are grouped into calls, or on B.  Partial sums narrower than 64 bits
 * are flushed before they can overflow: a lane walks at most dl4ds_ensemble_exceedance_walk_limit(K) = min(65535, (2^32 - 1) /
 * K^2) samples ((c - K o)^2 reaches K^2 per element), a call with more samples is split across workgroups.
 * Refused (non-zero return, dl4ds_last_error): K or T out of range, n % B != 0, member_stride < n, null members_dev, obs_dev or
 * thr_dev.  Algorithmic traffic (K + 1) * 4 * n bytes read once, plus 2 T n bytes written with count_dev. */
int dl4ds_ensemble_exceedance(const float* members_dev, size_t K, size_t n, size_t member_stride, const float* obs_dev, size_t B,
                              const float* thr_dev, int T, int thr_per_cell, short* count_dev, long long* sample_out_dev,
                              long long* cell_acc_dev, unsigned long long* table_dev);
int dl4ds_ensemble_exceedance_walk_limit(size_t K, size_t* samples_out);
/* Multivariate verification of an MC-dropout ensemble against an observation: the energy score (Gneiting et al. 2008) and the
 * variogram score (Scheuerer & Hamill 2015), the scores that see the members' SPATIAL structure (every score above looks at one
 * cell at a time).  The reference has neither; the definitions are DESIGN.md section 25.  members_dev, n, member_stride, obs_dev
 * and B as for dl4ds_ensemble_score: K rows of n fp32 values (row k at members_dev + k * member_stride), here 2 <= K <= 128, the
 * observation obs_dev [n], the n elements being B whole samples of P = n / B elements.  weight_dev (or null) [P]: a weight >= 0
 * per cell of one sample.  An element is VALID iff its observation and all K members are finite (no NaN, no infinity) and, with
 * weights, its cell weight is > 0: NaN in obs_dev is the masking mechanism.
 * dl4ds_ensemble_energy, per sample b, over its valid elements i, w_i = 1 without weights:
 *   D_k  = sum_i w_i (x_ki - y_i)^2,  k = 0 .. K - 1          G_kj = sum_i w_i (x_ki - x_kj)^2,  k < j
 *   dist_out_dev [B][K (K + 1) / 2] fp64: the K values D_k, then G_kj row-major over k < j;  nvalid_out_dev [B] int64
 *   (the host takes ES = (1/K) sum_k sqrt(D_k) - c sum_{k<j} sqrt(G_kj), c = 1 / K^2 or, fair, 1 / (K (K - 1)))
 *   Every term is computed and accumulated in fp64: (double)x - (double)y, squared, times (double)w.  The pair terms come from
 *   the differences themselves, never from a Gram matrix S_kk + S_jj - 2 S_kj, which cancels where members are close: every sum is
 *   a sum of non-negative terms.  One read of the stack; K (K + 1) / 2 fp64 multiply-adds per element against 4 (K + 1) bytes.
 * dl4ds_ensemble_variogram: a sample is planes x H x W x C (C innermost; planes: the product of its leading dimensions), a FIELD
 * one H x W plane of it (fixed leading index and channel).  The lags are the offsets (dy, dx) with 0 < dy^2 + dx^2 <= max_lag^2
 * and dy > 0 or (dy == 0 and dx > 0), ordered by (dy, dx) ascending: L <= 98 for 1 <= max_lag <= 8; dl4ds_variogram_lags writes
 * them as L (dy, dx) pairs into the HOST array dydx_out (or null) and L into count_out (or null).  A pair (i, i + lag) is valid
 * iff both elements are valid and lie in the same field.  Per valid pair, order p = 0.5 / 1 / 2 for order_code 0 / 1 / 2:
 *   o = |y_i - y_j|^p, e_k = |x_ki - x_kj|^p: difference and power are float32 IEEE operations (sqrtf, fabsf, one multiply)
 *   e = (sum_k (double)e_k) / K, summed in fp64 in member order k = 0, 1, ...
 *   npairs_out_dev [B][L] int64;  sums_out_dev [B][L][3] fp64: sum (o - e)^2, sum o, sum e over the valid pairs
 *   Weights only decide validity here (weight 0 excludes the element).
 * All outputs are overwritten.  No floating-point atomics: a repeated call gives the same bits.  How a sample's elements are split
 * over workgroups depends on (K, sample shape, max_lag) alone, and the partial sums are added in a fixed order: the sums of a
 * sample have the same bits for every B and for every position of the sample inside a call.
 * Refused (non-zero return, dl4ds_last_error): K or max_lag out of range, an unknown order code, n % B != 0, planes * H * W * C !=
 * n / B, member_stride < n, a null member stack, observation or output. */
int dl4ds_ensemble_energy(const float* members_dev, size_t K, size_t n, size_t member_stride, const float* obs_dev, size_t B,
                          const float* weight_dev, double* dist_out_dev, long long* nvalid_out_dev);
int dl4ds_ensemble_variogram(const float* members_dev, size_t K, size_t n, size_t member_stride, const float* obs_dev, size_t B,
                             const float* weight_dev, size_t planes, size_t H, size_t W, size_t C, int max_lag, int order_code,
                             long long* npairs_out_dev, double* sums_out_dev);
int dl4ds_variogram_lags(int max_lag, int* dydx_out, int* count_out);
/* Neighbourhood (scale- and threshold-dependent) verification of a prediction against an observation: the Fractions Skill Score
 * of Roberts & Lean (2008) and the 2 x 2 contingency table.  The reference has no such metric; the definitions are DESIGN.md
 * section 14.  y_dev / p_dev: observation and prediction, (N, H, W, C) fp32; each of the N*C planes is one field.
 * thresholds_host [T] (finite), windows_host [S] (>= 1): HOST arrays.  A cell is VALID iff y and p are both finite there: NaN in
 * y_dev is the masking mechanism.  bo = valid & (y >= t), bf = valid & (p >= t).  The window of size n at cell (i, j) is rows
 * [i - n/2, i - n/2 + n), columns likewise, clipped to the field (scipy.ndimage.uniform_filter(mode='constant') * n^2, even n
 * included; windows larger than the field are legal); co, cf are the counts of bo, bf in it.  All outputs are overwritten:
 *   sums_dev  [N][C][T][S][3]  D = sum (cf - co)^2, F = sum cf^2, O = sum co^2 over all H*W cells; FSS = 1 - D / (F + O)
 *   cont_dev  [N][C][T][4]     hits, misses, false alarms, correct negatives over the valid cells
 *   valid_dev [N][C]           number of valid cells
 * Integer arithmetic only (64-bit sums, integer atomics): the result equals an integer reference and a repeated call gives the
 * same bits.  Refused (non-zero return, dl4ds_last_error) unless H*W < 2^31 and, for every window, H*W*m^2 < 2^62 with
 * m = min(n, H) * min(n, W).  Algorithmic traffic: 8 B per cell read once, then 2-byte row prefixes (4-byte when W > 65535):
 * 4 T per cell written once, 16 T per cell and window read, mostly from cache. */
int dl4ds_fss(const float* y_dev, const float* p_dev, int N, int H, int W, int C, const float* thresholds_host, int T,
              const int* windows_host, int S, long long* sums_dev, long long* cont_dev, long long* valid_dev);
/* Neighbourhood verification of an MC-dropout ensemble as a PROBABILITY forecast: the Fractions Skill Score of the neighbourhood
 * ensemble probability (Schwartz et al. 2010) and the neighbourhood Brier score, for the sharp, slightly displaced members that
 * every per-cell score punishes twice.  The reference has no such metric; the definitions are DESIGN.md section 28.
 * members_dev, K, n, member_stride and obs_dev as for dl4ds_ensemble_exceedance: K rows of n fp32 values (row k at members_dev +
 * k * member_stride, 1 <= K <= 256) and the observation obs_dev [n].  The n elements are B whole samples of shape (H, W, C); each
 * of the B*C planes is one field.  thresholds_host [T] (1 <= T <= 16, finite) and windows_host [S] (S >= 1, each >= 1): HOST
 * arrays, as for dl4ds_fss.  A cell is VALID iff its observation and all K members are finite: NaN in obs_dev is the masking
 * mechanism.  Per valid cell and threshold t, every comparison on float32 (-0.0 >= 0.0 holds):
 *   o = [obs >= t],  c = #{k : x_k >= t} in 0 ... K;  an invalid cell has o = c = 0.
 * The window of size n at cell (i, j) is dl4ds_fss's: rows [i - n/2, i - n/2 + n), columns likewise, clipped to the field (even n
 * included, windows larger than the field are legal).  co = sum of o, cf = sum of c over the window; with m = min(n, H) * min(n, W),
 * co <= m and cf <= K m.  All outputs are overwritten:
 *   sums_dev  [B][C][T][S][5]  D = sum (cf - K co)^2, F = sum cf^2, O = sum co^2 over all H*W cells; Fv = sum cf^2 over the valid
 *                              centre cells; X = sum cf over the valid centre cells with o = 1
 *   cont_dev  [B][C][T][2]     E = sum o, Cs = sum c
 *   valid_dev [B][C]           number of valid cells
 * On the host: pFSS = 1 - D / (F + K^2 O), the FSS of the probability cf / (K n^2) against the observed fraction co / n^2; the
 * neighbourhood Brier score of that probability against the point observation is (Fv - 2 K n^2 X + K^2 n^4 E) / (K^2 n^4 n_valid)
 * with the REQUESTED n.  With n = 1 it is dl4ds_ensemble_exceedance's Brier score; with K = 1, D, F and O are dl4ds_fss's.
 * Integer arithmetic only (64-bit sums, integer atomics): the result equals an integer reference, a repeated call gives the same
 * bits, and nothing depends on B or on how the samples are grouped into calls.  More than 8 thresholds mean a second pass over
 * the stack.  Refused (non-zero return, dl4ds_last_error): K or T out of range, S < 1, n != B*H*W*C, member_stride < n, a null
 * pointer, a threshold that is not finite, a window < 1, H*W >= 2^31, or a window with H*W*(K m)^2 >= 2^62.
 * Algorithmic traffic: (K + 1) * 4 B per cell read once per group of 8 thresholds, then 2-byte row prefixes (4-byte when
 * K*W > 65535): 4 T per cell written once, 20 T per cell and window read, mostly from cache. */
int dl4ds_ensemble_fss(const float* members_dev, size_t K, size_t n, size_t member_stride, const float* obs_dev, size_t B, int H,
                       int W, int C, const float* thresholds_host, int T, const int* windows_host, int S, long long* sums_dev,
                       long long* cont_dev, long long* valid_dev);
/* Object labelling for object-based verification (SAL, object attributes): every field is cut into the connected objects of its
 * cells at or above a threshold.  The reference has no such metric; the definitions are DESIGN.md section 27.  x_dev: (N, H, W, C)
 * fp32, each of the F = N*C planes one field (f = n*C + c), read in place with stride C.  thr_dev [F]: one DEVICE threshold per
 * field.  A cell is VALID iff finite, an EVENT iff valid and x >= thr on float32 (-0.0 >= 0.0 holds); a field whose threshold is
 * not finite has no event.  connectivity 1 (4 neighbours) or 2 (8 neighbours), fields do not wrap.  Every output given is
 * overwritten; labels_dev, nvalid_dev and field_sums_dev may be null, the five tables may be null when cap == 0:
 *   labels_dev     [F][H][W]    0 background, objects 1 ... count in raster order of their first cell (scipy.ndimage.label)
 *   count_dev      [F]          number of objects, also when it exceeds cap
 *   nvalid_dev     [F]          number of valid cells;  field_sums_dev [F][3]  fp64 sum v, sum v*i, sum v*j over the valid cells
 *   sums_dev       [F][cap][6]  area, sum i, sum j, sum i*i, sum j*j, sum i*j of object r + 1 (exact 64-bit integers)
 *   bbox_dev       [F][cap][4]  min i, max i, min j, max j;  first_dev [F][cap]  the object's smallest cell index i*W + j
 *   vmax_dev       [F][cap]     the object's largest value (exact, +0.0 above -0.0)
 *   mass_dev       [F][cap][3]  fp64 sum v, sum v*i, sum v*j over the object's cells, every term exact
 * Rows count ... cap are zero; objects beyond cap are left out of the tables and keep their labels.  Labels, every integer output
 * and vmax are pure functions of the input; field_sums_dev has one fixed summation order (no float atomics) and gives the same
 * bits every call; mass_dev is accumulated with fp64 atomic adds and may differ in the last bits between calls, within
 * gamma_(n-1) * sum |term| of the exact sum of the object's n terms.  No workgroup waits for another and every loop is bounded by
 * the field size; a parent walk that passed its bound would raise the sticky device error that dl4ds_sync reports.
 * Refused (non-zero return, dl4ds_last_error) before any launch: N, H, W or C < 1, H*W >= 2^31 - 1, max(H, W) >= 2^29,
 * H*W*max(H, W)^2 >= 2^62, connectivity not 1 or 2, cap < 0, a null x_dev, thr_dev or count_dev, cap > 0 with a null table.
 * dl4ds_object_thresholds: SAL's thr_dev [F] = float32(factor * the largest finite value of the field), the product taken in fp64
 * and rounded once; 0 for a field without a finite cell or with a product that is not finite; factor positive and finite.
 * Algorithmic traffic: 4 B per cell read (twice when tables are wanted), an 8 B per cell workspace (parent links, root labels)
 * written once and read a small number of times, 4 B per cell of labels written when wanted.  Fields go through in chunks of a
 * fixed workspace budget. */
int dl4ds_label_objects(const float* x_dev, int N, int H, int W, int C, const float* thr_dev, int connectivity, int cap,
                        int* labels_dev, int* count_dev, long long* nvalid_dev, double* field_sums_dev, long long* sums_dev,
                        int* bbox_dev, int* first_dev, float* vmax_dev, double* mass_dev);
int dl4ds_object_thresholds(const float* x_dev, int N, int H, int W, int C, double factor, float* thr_dev);
/* Distance and displacement measures on binary event fields: the exact Euclidean distance transform of the observed and of the
 * predicted event set and, on top of the two maps, the sums of the Hausdorff distance, the mean error distances, Baddeley's Delta
 * and Pratt's figure of merit.  The reference has no such metric; the definitions are DESIGN.md section 29.  y_dev / p_dev:
 * observation and prediction, (N, H, W, C) fp32, read in place with stride C; each of the F = N*C planes is one field (f = n*C + c).
 * p_dev may equal y_dev (a single-field distance transform).  thresholds_host [T] (finite): a HOST array.  A cell is VALID iff y and
 * p are both finite there: NaN in y_dev is the masking mechanism.  A = valid & (y >= t), B = valid & (p >= t) on float32 (-0.0 >=
 * 0.0 holds); fields do not wrap.  d2(x, S) = min over s in S of di^2 + dj^2 as int32, 2^31 - 1 when S is empty (it reads as +inf);
 * distances pass through invalid cells, sums leave them out.  With d = sqrt(d2) in fp64, cutoff c > 0 (may be +inf), alpha
 * positive and finite, w(x) = |min(d(x, A), c) - min(d(x, B), c)|, every output given is overwritten:
 *   counts_dev  [F][T][8] int64  n_valid, n_A, n_B, n_AB, max over A of d2(a, B), max over B of d2(b, A), sum over A of d2(a, B),
 *                                sum over B of d2(b, A)  (0 over an empty set; the 2^31 - 1 of an empty other side is taken as it is)
 *   sums_dev    [F][T][7] fp64   sum over A of d(a, B), sum over B of d(b, A), sum over A of 1 / (1 + alpha d2(a, B)), sum over B of
 *                                1 / (1 + alpha d2(b, A)), and over the valid cells sum w, sum w^2, max w
 *   d2_obs_dev, d2_pred_dev [F][T][H][W] int32, or null: d2(x, A) and d2(x, B) at every cell
 * Every fp64 term is built from sqrt, +, -, *, /, min and abs without FMA contraction; non-finite results are left as IEEE
 * arithmetic gives them.  The integers and the maps are pure functions of the input.  No atomics: the fp64 sums have one summation
 * order (a lane's cells in ascending j, a fixed tree over the lanes, the rows in a fixed order), so a repeated call gives the same
 * bits and nothing depends on N or on how the fields go through in chunks of a fixed workspace budget.  Plain launches on one
 * stream; every loop is bounded by H, W or the number of row segments.
 * Refused (non-zero return, dl4ds_last_error) before any launch: a null y_dev, p_dev, thresholds_host, counts_dev or sums_dev;
 * N, H, W, C or T < 1; (H-1)^2 + (W-1)^2 >= 2^31 - 1 or H*W >= 2^31; a threshold that is not finite; cutoff not > 0 (NaN included);
 * alpha not positive and finite.
 * Algorithmic traffic: 8 B per cell read once per group of 8 thresholds; per threshold and cell 2 vertical distances (2 B each)
 * written, read and mostly rewritten by the column pass and read once by the row pass, which also reads the 8 B of
 * y and p again (from cache) and writes 4 B per map wanted. */
int dl4ds_distance_scores(const float* y_dev, const float* p_dev, int N, int H, int W, int C, const float* thresholds_host, int T,
                          double cutoff, double alpha, long long* counts_dev, double* sums_dev, int* d2_obs_dev, int* d2_pred_dev);
/* Distribution verification of a prediction against an observation: per segment the sample quantiles of either side, the
 * 1-Wasserstein distance, the two-sample Kolmogorov-Smirnov statistic, a histogram of either side and the valid count.  The
 * reference has no such metric; the definitions are DESIGN.md section 15.  Element k of segment s of either array lives at
 * base[s*seg_stride + k*elem_stride] (as dl4ds_spearman): per sample over its values (S = N, L = H*W*C, contiguous) or per grid
 * cell over the samples (S = H*W*C, L = N, seg_stride 1, elem_stride H*W*C).  q_host [Q] (0 <= Q <= 64, each in [0, 1]) and
 * edges_host [E] (E = 0, or 2 <= E <= 257 finite, strictly increasing) are HOST arrays.  Per segment:
 *   an element is VALID iff y and p are both finite there (NaN in y_dev is the masking mechanism); invalid elements are dropped
 *   from both sides, so both samples have n <= L values; -0.0 counts as +0.0.  With a, b the ascending valid values of y, p:
 *   quant_dev [S][2][Q]   (obs, pred) numpy method='linear': h = q*(n-1), j = floor(h), x[j] + (x[min(j+1, n-1)] - x[j]) * (h - j)
 *                         in fp64 on the float32 values, multiply and add not fused; NaN when n = 0
 *   w1_dev    [S]         (1/n) sum |a[i] - b[i]| in fp64: the 1-Wasserstein distance of two equal-size samples; NaN when n = 0
 *   ks_dev    [S]         max over every valid value v of either side of |#{a <= v} - #{b <= v}|: n times the two-sample
 *                         Kolmogorov-Smirnov statistic, an exact integer; 0 when n = 0
 *   hist_dev  [S][2][E-1] number of valid values in [e_b, e_b+1), the last bin closed on the right (np.histogram); values outside
 *                         the edges are counted nowhere; may be null when E == 0
 *   valid_dev [S]         n
 * All outputs are overwritten.  No float atomics, reductions in a fixed order: a repeated call gives the same bits.  Refused
 * (non-zero return, dl4ds_last_error): L >= 2^31, S >= 2^31, Q < 0 or Q > 64, a q outside [0, 1], E = 1 or E > 257, edges that
 * are not finite or not strictly increasing.  Segments of up to 8192 contiguous elements, and of up to 512 elements when
 * seg_stride == 1, are sorted in LDS (8 B read per element, nothing else); longer ones by a key-only radix sort in a
 * workspace of at most 128 MiB per chunk of segments: 8 B read and 8 B written per element, then per side four passes of
 * 8 B read (twice) and 4 B written per element. */
int dl4ds_distribution(const float* y_dev, const float* p_dev, size_t S, size_t L, size_t seg_stride, size_t elem_stride,
                       const double* q_host, int Q, const float* edges_host, int E, double* quant_dev, double* w1_dev,
                       long long* ks_dev, long long* hist_dev, long long* valid_dev);
/* Quantile-mapping bias correction: empirical quantile mapping (EQM) and quantile delta mapping (QDM; Cannon et al. 2015).  The
 * reference has no counterpart; DESIGN.md section 18 carries the same definitions.  Arrays are fp32 (N, H, W, C); a cell is one
 * (h, w, c), per = H*W*C, cell c of sample n lives at x[n*per + c].
 * dl4ds_quantile_table (the fit).  The valid values of a cell are the finite ones among its N samples: NaN and +-inf are dropped
 *   (NaN is the masking mechanism), -0.0 counts as +0.0.  With x_0 <= ... <= x_{n-1} the ascending valid values, for each of the Q
 *   probabilities q_host[i] (HOST array, fp64, strictly increasing, in [0, 1]), in fp64 with every operation rounded on its own:
 *     h = q_i*(n-1), j = floor(h), g = h - j, val = x_j + (x_{min(j+1, n-1)} - x_j) * g
 *   (numpy's method='linear'), rounded once to fp32 into table_dev[i*per + c] (layout [Q][per]); with n = 0 all Q entries are NaN.
 *   valid_dev [per] (may be null) = n.  Segments of up to 512 samples are sorted in LDS, longer ones by the key-only radix sort of
 *   dl4ds_distribution in a workspace of at most 128 MiB per chunk of cells.  No floating-point atomics: a repeated call gives
 *   the same bits.
 * dl4ds_qmap_apply (the map), B samples of per cells; m = model_tab_dev (the model's historical table), o = obs_tab_dev, f =
 *   target_tab_dev (the table of the period being corrected; null selects EQM, non-null QDM), all [Q][per]; the search table s is m
 *   for EQM and f for QDM.  Every operation is on fp32 and rounded on its own (no fused multiply-add, division correctly rounded).
 *   For element value v in cell c:
 *     1. v not finite: out = v; counted in counts[0] (n_nonfinite).
 *     2. the cell is UNFITTED iff row 0 of any table in use is NaN there: out = NaN, or v with keep_unfitted != 0; counts[1].
 *     3. v < s[0]: j = 0, t = 0 (counts[2], n_below); v >= s[Q-1]: j = Q-1, t = 0 (counts[3], n_above); otherwise j is the largest
 *        index with s[j] <= v (so s[j+1] > v) and t = (v - s[j]) / (s[j+1] - s[j]).
 *     4. o_t = o[j] at the two ends, otherwise o[j] + (o[j+1] - o[j]) * t; m_t likewise from m.
 *     5. EQM in the interior: out = o_t.  QDM everywhere and EQM at the two ends: kind 0 (additive): out = v + (o_t - m_t); kind 1
 *        (multiplicative): out = v * (o_t / m_t), and out = o_t where m_t == 0.
 *   Tables are non-decreasing by construction; ties are legal (rule 3 never divides by zero).  out_dev may be x_dev.  counts_dev
 *   [4] (may be null): 64-bit counts ADDED onto what the caller has zeroed (integer atomics, one per workgroup and counter).
 *   Algorithmic traffic 8 B per element plus the tables once, 4*Q B per cell and table.
 * Refused (non-zero return, dl4ds_last_error): Q < 2 or Q > 256, a q outside [0, 1] or q not strictly increasing, N == 0,
 * per == 0, N >= 2^31, a null required pointer, kind not 0 or 1. */
int dl4ds_quantile_table(const float* x_dev, size_t N, size_t per, const double* q_host, int Q, float* table_dev,
                         long long* valid_dev);
int dl4ds_qmap_apply(const float* x_dev, float* out_dev, size_t B, size_t per, const float* model_tab_dev, const float* obs_tab_dev,
                     const float* target_tab_dev, int Q, int kind, int keep_unfitted, unsigned long long* counts_dev);
/* Climate indices along the time axis: spells, extremes, threshold days and sums per grid cell and period, the raw material of the
 * ETCCDI indices (CDD / CWD, Rx1day / Rx5day, R1mm / R10mm / R20mm, SDII, PRCPTOT, TXx / TNn, FD / SU, R95pTOT, start and end of a
 * season).  The reference has no counterpart; DESIGN.md section 19 carries the same definitions.
 * x is fp32 with shape (N, H, W, C).  A cell is one (h, w, c), and per = H*W*C.  Cell c of sample n lives at x[n*per + c].
 * The samples are in time order.  The P periods are given by period_starts_host with P + 1 entries: a HOST array of int64, strictly
 * increasing, first 0, last N.  Period p is the set of samples with start_p <= n < start_{p+1}.  Periods are independent.  Nothing
 * carries across a boundary: a run is cut there, and a window lies inside one period.
 * A sample is VALID in a cell iff its value is finite.  NaN is the masking mechanism.  -0.0 counts as +0.0.
 * There are 1 <= T <= 4 thresholds in the DEVICE array thr_dev, used as in dl4ds_ensemble_exceedance: thr_per_cell == 0 means [T]
 * values, otherwise [T][per] is a threshold field per cell (a local wet-day percentile, say).  One comparison op applies to all of
 * them: 0 is >=, 1 is >, 2 is <, 3 is <=.  Comparisons are made on float32.
 * A valid sample is an EVENT for threshold t iff x op thr(t, c) holds, and is a non-event otherwise.  An event run is a maximal
 * stretch of consecutive samples of the period that are all events.  A non-event run is the same over valid non-events.  An
 * invalid sample ends both kinds of run.
 * If thr(t, c) is not finite, the per-threshold outputs of that (t, c) are -1 for the integers and NaN for the sum, in every period.
 * Per period p and cell c, each output may be null and is then skipped.  All outputs are overwritten.
 *   valid_dev int32 [P][per]         the number of valid samples
 *   event_dev int32 [P][T][6][per]   in this order: the number of events; the longest event run; the longest non-event run; the
 *                                    number of event runs; the offset from the period's first sample of the first event, -1 if
 *                                    none; the offset of the last event, -1 if none
 *   ext_dev   fp32  [P][2][per]      the largest and smallest valid value, NaN if there is none; a zero is always written as +0.0
 *   sum_dev   fp64  [P][2 + T][per]  row 0: the sum of the valid values, added one by one in ascending sample order, in fp64,
 *                                    starting from the first valid value; NaN if there is none.
 *                                    row 1: the largest window sum, over all windows of `window` consecutive samples
 *                                    (1 <= window <= 32) that lie wholly inside the period and are all valid.  Each window sum is
 *                                    formed afresh: its `window` values are added in ascending sample order in fp64 (no sliding add
 *                                    and subtract, which gives other bits).  NaN if no such window exists.
 *                                    row 2 + t: the sum of the event values for threshold t, in the same order as row 0; 0.0 if
 *                                    the threshold is finite and there is no event.
 * There are no floating-point atomics and no sum whose order can vary.  A repeated call gives the same bits.
 * Refused (non-zero return, dl4ds_last_error): P < 1; starts that are not strictly increasing from 0 to N; N == 0, per == 0 or
 * N >= 2^31; T or window out of range; an op outside 0..3; a null x_dev, thr_dev or period_starts_host; all four outputs null.
 * A lane owns one cell and walks one period in order, so parallelism is cells x periods; a period is never split over time, which
 * would change the order of the fp64 sums.  Algorithmic traffic: 4 B per element read once, the outputs written once. */
int dl4ds_climate_indices(const float* x_dev, size_t N, size_t per, const long long* period_starts_host, int P,
                          const float* thr_dev, int T, int thr_per_cell, int op, int window, int* valid_dev, int* event_dev,
                          float* ext_dev, double* sum_dev);
/* Extreme-value verification: sorted probability-weighted moments per cell and declustered peaks over a threshold, the device
 * side of L-moment fits (GEV, Gumbel, GPD) and N-year return levels.  The reference has no counterpart; DESIGN.md section 26
 * carries the same definitions.
 * dl4ds_lmoments.  Sample n of cell c lives at x_dev[n*stride + c] with stride >= per, so row 0 of dl4ds_climate_indices' ext_dev
 *   (stride 2*per) and the peaks of dl4ds_pot_peaks are read in place.  sign is +1 or -1 and the sample is sign * x, so -1 serves
 *   the lower tail and minima.  The valid samples of a cell are the finite ones (NaN is the masking mechanism); -0.0 counts as
 *   +0.0.  Let n be their number and x_0 <= ... <= x_{n-1} their values in ascending order, widened exactly to fp64.  For r = 0..3:
 *     S_r = the sum of w_r(j) * x_j over j = r..n-1, in ascending j, starting from its first term
 *     w_0 = 1,  w_r(j) = w_{r-1}(j) * ((double)(j-r+1) / (double)(n-r))
 *   Every division is correctly rounded.  Every multiplication and addition is rounded on its own (no fused multiply-add).
 *     pwm_dev fp64 [4][per]   pwm_dev[r*per + c] = S_r / (double)n, NaN when n <= r: Hosking's unbiased b_0..b_3
 *     valid_dev int32 [per]   n
 *   Either output may be null, not both.  With ties the order of equal values does not matter.  Segments of up to 512 samples are
 *   sorted in LDS, longer ones by the key-only radix sort of dl4ds_distribution in a workspace of at most 128 MiB per chunk of
 *   cells; the lane that owns a cell then adds its values in rank order, so both engines give the same bits.  No atomics.
 *   Refused (non-zero return, dl4ds_last_error): N == 0, per == 0, N >= 2^31, stride < per, sign not +-1, a null x_dev, both
 *   outputs null.
 * dl4ds_pot_peaks.  x, per, period_starts_host and P as in dl4ds_climate_indices (stride per; validity and -0.0 as there).  One
 *   threshold in the DEVICE array thr_dev: thr_per_cell == 0 means [1], otherwise [per].  sign is +1 or -1, run is in 1..32.
 *   With v = sign*x and u = sign*thr(c), compared on fp32, a valid sample is an EXCEEDANCE iff v > u.  A cluster opens at an
 *   exceedance.  It closes after `run` consecutive valid non-exceedances, at an invalid sample, at a period boundary and at the end
 *   of the series; run = 1 makes every maximal run of exceedances a cluster.  The peak of a cluster is its largest v, written as x
 *   (not v) with a zero as +0.0, and its position is the sample index of the first occurrence of that value in the cluster.
 *     count_dev int32 [per]     the number of clusters of the cell, also beyond K; -1 where the threshold is not finite
 *     peak_dev  fp32  [K][per]  the peaks in order of occurrence, row k < min(count, K); NaN in the rows from count on (so
 *                               dl4ds_lmoments reads the buffer as it is); all K rows NaN where the threshold is not finite
 *     pos_dev   int32 [K][per]  their sample indices; -1 where peak_dev holds NaN
 *   peak_dev and pos_dev may be null.  K == 0 only counts.  All outputs are overwritten.
 *   Refused: what dl4ds_climate_indices refuses of N, per, P and the starts; a null x_dev, thr_dev, period_starts_host or
 *   count_dev; sign not +-1; run outside 1..32; K < 0; K > 0 with peak_dev and pos_dev both null.
 *   A lane owns one cell and walks the series in order.  Algorithmic traffic: 4 B per element read once. */
int dl4ds_lmoments(const float* x_dev, size_t N, size_t per, size_t stride, int sign, int* valid_dev, double* pwm_dev);
int dl4ds_pot_peaks(const float* x_dev, size_t N, size_t per, const long long* period_starts_host, int P, const float* thr_dev,
                    int thr_per_cell, int sign, int run, int K, int* count_dev, float* peak_dev, int* pos_dev);
/* Temporal verification along the time axis: the raw sums of the lag-k autocorrelation, the event transition counts and the
 * histogram of spell lengths per grid cell and period, of one series or of two on common validity.  The reference has no
 * counterpart; DESIGN.md section 24 carries the same definitions.
 * y and p are fp32 with shape (N, H, W, C), in time order.  A cell is one (h, w, c), and per = H*W*C.  Cell c of sample n lives at
 * x[n*per + c].  p_dev may be null.  S = 1 with y alone and S = 2 with both; series 0 is y, series 1 is p.
 * The P periods are given by period_starts_host exactly as in dl4ds_climate_indices: a HOST array of int64 with P + 1 entries,
 * strictly increasing, first 0, last N.  Nothing carries across a period boundary.
 * A sample is VALID in a cell iff it is finite in every series supplied.  This is common validity, as in dl4ds_distribution, so
 * the two series are compared on the same days.  -0.0 counts as +0.0.
 * lags_host is a HOST array of 0 <= L <= 4 lags, strictly increasing, each in 1..32.
 * There are 0 <= T <= 4 thresholds.  thr_dev, thr_per_cell and op mean exactly what they mean in dl4ds_climate_indices: [T] or
 * [T][per] in a DEVICE array, op 0 is >=, 1 is >, 2 is <, 3 is <=, compared on float32.  Events, non-events, event runs and
 * non-event runs are defined as there: an invalid sample ends both kinds of run.  spell_bins is B in 1..32.
 * If thr(t, c) is not finite, every integer output of that (t, c) is -1 in every period.
 * Per period p and cell c, each output may be null and is then skipped.  All outputs are overwritten.
 *   valid_dev  int32 [P][per]              the number of valid samples
 *   moment_dev fp64  [P][S][2][per]        sum x and sum x^2 over the valid samples of the period, each added one term at a time
 *                                          in ascending sample order, starting from 0.0.  x^2 is formed in fp64 from the fp32
 *                                          value, which is exact.
 *   pair_dev   int32 [P][L][per]           the number of pairs (n, n + lag) with both samples inside the period and both valid
 *   lag_dev    fp64  [P][S][L][3][per]     over exactly those pairs, in ascending n, with a = x_n and b = x_{n+lag}: sum a, sum b,
 *                                          sum a*b.  The product is formed in fp64 from two fp32 values and is exact, so fused
 *                                          and unfused evaluation give the same bits.
 *   trans_dev  int32 [P][S][T][4][per]     over consecutive samples (n, n + 1) both inside the period and both valid: the counts
 *                                          n00, n01, n10, n11.  The first digit is the state at n, the second at n + 1; 1 means
 *                                          event.
 *   spell_dev  int32 [P][S][T][2][B][per]  kind 0 is event runs, kind 1 is non-event runs.  Bin k - 1 holds the number of runs of
 *                                          length k for k < B; the last bin holds the runs of length >= B.  Every maximal run
 *                                          counts, including one cut by a period boundary or ended by an invalid sample.
 * There are no floating-point atomics and no sum whose order can vary.  A repeated call gives the same bits.
 * Refused (non-zero return, dl4ds_last_error): P < 1; starts that are not strictly increasing from 0 to N; N == 0, per == 0 or
 * N >= 2^31; L, T or B out of range; a lag out of range or not increasing; an op outside 0..3; a null y_dev or period_starts_host;
 * lags_host null with L > 0; thr_dev null with T > 0; pair_dev or lag_dev non-null with L == 0; trans_dev or spell_dev non-null
 * with T == 0; all six outputs null.
 * A lane owns one cell and walks one period in order, so parallelism is cells x periods.  Algorithmic traffic: 4*S B per element
 * read once, the outputs written once. */
int dl4ds_temporal(const float* y_dev, const float* p_dev, size_t N, size_t per, const long long* period_starts_host, int P,
                   const int* lags_host, int L, const float* thr_dev, int T, int thr_per_cell, int op, int spell_bins,
                   int* valid_dev, double* moment_dev, int* pair_dev, double* lag_dev, int* trans_dev, int* spell_dev);
/* Trend per grid cell over the periods: Mann-Kendall and Sen's slope.  The reference has no counterpart; DESIGN.md section 24
 * carries the same definitions.
 * v_dev is fp64 [P][per]: one value per period and cell, in period order (annual prcptot, rx1day or a mean from
 * dl4ds_climate_indices, say).  Time is the period index 0..P-1.  A value is valid iff finite, so gaps keep their true spacing.
 * Comparisons are made on fp64.  Each output may be null; at least one must be non-null.
 *   valid_dev int32 [per]     n, the number of valid values
 *   mk_dev    int64 [2][per]  row 0: S = the sum over i < j, both valid, of sign(v_j - v_i).  row 1: the tie term, the sum over the
 *                             groups of equal values of g(g - 1)(2g + 5).  Both are exact integers.
 *   sen_dev   fp64  [per]     with the M = n(n - 1)/2 slopes s = (v_j - v_i) / (double)(j - i) for i < j both valid, sorted
 *                             ascending: s[(M-1)/2] for odd M and (s[M/2 - 1] + s[M/2]) * 0.5 for even M.  The subtraction, the
 *                             division and the addition are each rounded on their own; the division is correctly rounded.  A zero
 *                             is written as +0.0.  NaN when n < 2.
 * Refused: P < 1 or P > 128; per == 0; a null v_dev; all outputs null. */
int dl4ds_trend(const double* v_dev, int P, size_t per, int* valid_dev, long long* mk_dev, double* sen_dev);
/* Spectral verification of a prediction against an observation: binned power and cross spectra per field.  The reference has no
 * such metric; DESIGN.md section 16 carries the same definitions.  y, p are observation and prediction, fp32, shaped (N, H, W, C).
 * Each of the F = N*C planes is one field.  Fields are ordered [n][c].
 * 1. Kept cells and detrending.  A cell is kept iff y and p are both finite there.  NaN in y is the masking mechanism.
 *    n_valid[f] is the number of kept cells.  detrend = 1: each side has its own mean over its kept cells subtracted.  The mean is
 *    an fp64 sum in a fixed order, and is returned in mean_dev[f][2].  detrend = 0: nothing is subtracted.  The means are written
 *    as 0.  Excluded cells become 0 after that step.
 * 2. Window.  window = 1 multiplies cell (i, j) by wy[i]*wx[j].  w[i] = 0.5 - 0.5*cos(2 pi i / n) is the periodic Hann window.  It
 *    is computed on the host in fp64.  window = 0: no window.
 * 3. Transform.  X(ky, kx) = sum_i sum_j v[i][j] * exp(-2 pi i (ky*i/H + kx*j/W)).  This is numpy's unnormalised fft2, evaluated in
 *    fp64.  Twiddle factors come from host-made fp64 tables of H and W entries.  They are indexed by (k*i) mod n, an exact
 *    integer, so no angle is ever reduced in floating point.
 * 4. Bins.  The caller passes a HOST map bin_host[H][W/2+1] of int32 for the half plane kx = 0 .. floor(W/2).  Values lie in
 *    [0, B), or -1 for a coefficient counted nowhere.  The library never computes a radius.  A half-plane coefficient counts
 *    mult(kx) times.  mult is 1 for kx = 0 and for kx = W/2 when W is even, else 2.  The caller's map is symmetric under
 *    (ky, kx) -> (-ky, -kx), so this equals the full-plane sum.
 * 5. Outputs.  All are overwritten.
 *      power_dev [F][4][B]  fp64: sum mult*|Y|^2, sum mult*|P|^2, Re sum mult*Y*conj(P), Im sum mult*Y*conj(P) over the half-plane
 *                           coefficients of the bin
 *      valid_dev [F]        int64
 *      mean_dev  [F][2]     fp64
 *    p_dev may be null.  Then only component 0 and column 0 of mean_dev carry values and the rest is written as 0.  A field with
 *    n_valid = 0 gives zeros.  There are no floating-point atomics and every reduction has a fixed order.  A repeated call gives
 *    the same bits, and the result does not depend on how fields are grouped into calls.
 * 6. Refusals.  A non-zero return with dl4ds_last_error, for any of: H or W < 1 or > 16384; B < 1 or B > 16384; a map entry
 *    outside [-1, B); N*C >= 2^31.
 * The transform is a direct DFT as two fp64 matrix products (about 2 H W^2 + 4 H^2 W flops per field and side), tiled through LDS;
 * the row transform's complex output and the four products per coefficient live in a workspace of at most 128 MiB per chunk of
 * fields (64 bytes per half-plane coefficient and field), a field larger than that runs alone. */
int dl4ds_spectrum(const float* y_dev, const float* p_dev, int N, int H, int W, int C, int detrend, int window,
                   const int* bin_host, int B, double* power_dev, long long* valid_dev, double* mean_dev);
/* Keras BinaryCrossentropy(from_logits=False) vs a constant label -- cgan.py:546-549,567-571 */
int dl4ds_op_bce(const float* p_dev, float label, int n, float* loss_dev, float* dp_dev);
/* tf.keras.optimizers.Adam step t (1-based) -- supervised.py:353; cgan.py:277-278 */
int dl4ds_op_adam(float* w_dev, const float* g_dev, float* m_dev, float* v_dev, size_t n, int t, float lr,
                  float beta1, float beta2, float eps, float grad_scale);
/* dl4ds_op_adam with clipping by the global gradient norm (Keras global_clipnorm = tf.clip_by_global_norm; 0: off), decoupled weight
 * decay (Keras weight_decay / AdamW: w <- w - lr * weight_decay * w with the plain lr, before the gradient update) on the n_ranges
 * [begin, end) element ranges decay_ranges_host[2 * n_ranges] (any order, any element boundaries; merged where they touch) and an
 * exponential moving average ema <- ema_momentum * ema + (1 - ema_momentum) * w_new (ema_dev NULL: none).  At most two launches.
 * norm = fl32(grad_scale * sqrt(sum g^2)) with the sum in fp64 in a fixed order (bit-reproducible); the gradient is scaled by
 * c = clip / max(norm, clip), exactly 1 when norm <= clip.  A NON-FINITE norm skips the step: w, m, v, ema stay untouched.
 * stats_out_dev[3] (device, kept by the caller across calls): [0] norm (0 without clipping) [1] c [2] the count of skipped steps,
 * a 32-bit UNSIGNED INTEGER in that word, incremented in place.  With everything off the results equal dl4ds_op_adam's bit for bit. */
int dl4ds_op_adam_ext(float* w_dev, const float* g_dev, float* m_dev, float* v_dev, float* ema_dev, size_t n, int t, float lr,
                      float beta1, float beta2, float eps, float grad_scale, float global_clipnorm, float weight_decay,
                      const size_t* decay_ranges_host, int n_ranges, float ema_momentum, float* stats_out_dev);
/* exchanges two device arrays element by element in one kernel (what dl4ds_trainer_ema_swap runs) */
int dl4ds_op_arena_swap(float* a_dev, float* b_dev, size_t n);

/* ---------------------------------------------------------------- model graph
 * replaces the tf.keras functional graphs assembled by dl4ds/models/{sp_postups,sp_preups,spt_postups,
 * spt_preups,discriminator}.py.  The Python builders add tensors / parameters / ops in call order. */
int dl4ds_graph_create(dl4ds_graph** g);
int dl4ds_graph_destroy(dl4ds_graph* g);
/* nmul: batch multiplier of the tensor (1, or time_window for (B,T,H,W,C) tensors) */
int dl4ds_graph_input(dl4ds_graph* g, int H, int W, int C, int nmul, int* tensor_id);
/* allocate a gradient buffer for an input (the discriminator's HR input: the generator's adversarial
 * gradient flows through it -- cgan.py:600-613) */
int dl4ds_graph_input_requires_grad(dl4ds_graph* g, int tensor_id);
int dl4ds_graph_param(dl4ds_graph* g, size_t n, int* param_id);
int dl4ds_graph_conv2d(dl4ds_graph* g, int in, int w, int b, int add, int KS, int Cout, int relu, int d2s_r, int* out);
int dl4ds_graph_conv2d_transpose(dl4ds_graph* g, int in, int w, int KS, int stride, int Cout, int relu, int* out);
int dl4ds_graph_chatt(dl4ds_graph* g, int in, int w1, int b1, int w2, int b2, int Cr, int time_window_5d, int* out);
int dl4ds_graph_concat(dl4ds_graph* g, const int* ins, int n, int* out);
int dl4ds_graph_add(dl4ds_graph* g, int a, int b, int relu, int* out);
int dl4ds_graph_act(dl4ds_graph* g, int in, int kind, int* out);   /* 1 relu 2 sigmoid 3 tanh 4 elu 5 leaky 6 selu 7 gelu */
int dl4ds_graph_maxpool2(dl4ds_graph* g, int in, int* out);
int dl4ds_graph_resize(dl4ds_graph* g, int in, int Ho, int Wo, int* out);
/* Resizing(Ho, Wo, interpolation='nearest') (half-pixel centres) -- ResizeConvolutionBlock(interpolation='nearest'), blocks.py:473-489 */
int dl4ds_graph_resize_nearest(dl4ds_graph* g, int in, int Ho, int Wo, int* out);
/* Resizing(interpolation='bicubic') = tf.image.resize(method='bicubic'): ResizeBicubic with half-pixel centres (Keys cubic,
 * A = -0.5, 1024-step weight table, out-of-image taps dropped and the rest renormalised) -- blocks.py:473-489 */
int dl4ds_graph_resize_bicubic(dl4ds_graph* g, int in, int Ho, int Wo, int* out);
/* Resizing(interpolation=...) by number: 0 bilinear, 1 nearest, 2 bicubic, and tf.image.resize's ScaleAndTranslate family
 * (antialias=False: scale = out / in, kernel scale 1, spans clamped into the image and normalised): 3 lanczos3, 4 lanczos5,
 * 5 gaussian (radius 1.5, sigma 0.5), 6 mitchellcubic -- blocks.py:473-489.  ('area' has no gradient in TensorFlow, so a
 * ResizeConvolutionBlock built with it cannot be trained by the reference either; it is rejected.) */
int dl4ds_graph_resize_method(dl4ds_graph* g, int in, int Ho, int Wo, int method, int* out);
int dl4ds_graph_localconv(dl4ds_graph* g, int in, int w, int b, int F, int* out);
int dl4ds_graph_repeat_time(dl4ds_graph* g, int in, int T, int* out);
/* The recurrent nets' tail as ONE op -- spt_postups.py:133-151 / spt_preups.py:114-132, blocks.py:301-333:
 *   y = TransitionLast(Concatenate([x24, LocalizedConvBlock(x24)])),  x24 = Concatenate([x, repeat(expand_dims(s, 1), T)])
 * x: (B,T,H,W,CX), s: (B,H,W,CS) = ConvBlock_aux's output, y: (B,T,H,W,CO), ReLU after both 1x1 convolutions.  Parameters = the
 * reference layers' own variables: wt / bt = LocalizedConvBlock's TransitionBlock(2) kernel [1,1,CX+CS,2] / bias, wl / bl =
 * its LocallyConnected2D kernel [H,W,2,2] / bias [H,W,2], w / b = TransitionLast's kernel [1,1,CX+CS+2,CO] / bias.  No
 * concatenation and no time repeat is materialised (csrc/graph_ops4.hip).  dl4ds_rec_tail_supported says whether the channel
 * combination is built (and DL4DS_NO_REC_TAIL_FUSION is unset); otherwise the caller builds the separate layers. */
int dl4ds_rec_tail_supported(int CX, int CS, int CO, int* yes);
int dl4ds_graph_rec_tail(dl4ds_graph* g, int x, int s, int wt, int bt, int wl, int bl, int w, int b, int T, int CO, int* out);
int dl4ds_graph_convlstm(dl4ds_graph* g, int in, int wk, int wr, int b, int KS, int F, int T, int relu, int* out);
int dl4ds_graph_gap(dl4ds_graph* g, int in, int* out);
/* DepthwiseConv2D(7, 'same') + bias -- blocks.py:143-144 */
int dl4ds_graph_dwconv(dl4ds_graph* g, int in, int w, int b, int KS, int* out);
/* GlobalAveragePooling3D over the (time, H, W) axes of a time-distributed tensor -- discriminator.py:73-74 */
int dl4ds_graph_gap3d(dl4ds_graph* g, int in, int* out);
/* y[:, i, j, :] = x[:, oy + i*step, ox + j*step, :] (i < Ho, j < Wo): the sub-sampling half of Conv2D(strides=2)
 * (the stride-1 convolution runs on the MFMA kernels) and Cropping2D -- discriminator.py:53-60 */
int dl4ds_graph_slice(dl4ds_graph* g, int in, int oy, int ox, int step, int Ho, int Wo, int* out);
/* Conv2D(KSxKS, d2s*d2s*Cmid filters) [+ depth_to_space(d2s)] immediately followed by Conv2D(1x1, Cout) (+ optional ReLU)
 * evaluated as one convolution with the composed filter; parameters and their gradients stay those of the two layers
 * (w1 (KS,KS,Cin,d2s^2*Cmid), b1, w2 (Cmid,Cout), b2; biases may be -1).  SubpixelConvolutionBlock / ResizeConvolutionBlock
 * + TransitionBlock 'TransitionLast' -- sp_postups.py:172-177,203. */
int dl4ds_graph_conv2d_folded(dl4ds_graph* g, int in, int w1, int b1, int w2, int b2, int KS, int Cmid, int Cout, int relu,
                              int d2s, int* out);
/* ... with the HR auxiliary branch of the model: TransitionLast reads Concatenate([upsampled x, s]) (sp_postups.py:184-203), i.e.
 * w2 has Cmid + C(aux) rows; out = act(composed conv(x) + conv1x1(aux; rows Cmid..) + bias).  `aux` lives on the output grid. */
int dl4ds_graph_conv2d_folded_aux(dl4ds_graph* g, int in, int aux, int w1, int b1, int w2, int b2, int KS, int Cmid, int Cout,
                                  int relu, int d2s, int* out);
/* ZeroPadding2D(((0, Ho - H), (0, Wo - W))) -- PadConcat, blocks.py:639-647 */
int dl4ds_graph_pad(dl4ds_graph* g, int in, int Ho, int Wo, int* out);
int dl4ds_graph_dense(dl4ds_graph* g, int in, int w, int b, int F, int act, int* out);
int dl4ds_graph_dropout(dl4ds_graph* g, int in, float rate, int* out);
/* get_dropout_layer (blocks.py:679-706).  variant: 0 Dropout, 1 GaussianDropout, 2 SpatialDropout2D/3D (spatial_dim);
 * mc != 0: the MC* layers of blocks.py:658-676, active at inference too. */
int dl4ds_graph_dropout_variant(dl4ds_graph* g, int in, float rate, int variant, int mc, int spatial_dim, int* out);
/* noise of dropout op `index` (creation order) for a batch of B samples: the keep mask (variants 0, 2; one entry per
 * element resp. per (frame|sample, channel)) or the multiplicative Gaussian noise (variant 1).  get: the one the last
 * forward pass used; set: used by the NEXT training-mode forward instead of drawing a new one. */
int dl4ds_graph_dropout_count(dl4ds_graph* g, int* n);
int dl4ds_graph_dropout_mask_size(dl4ds_graph* g, int index, int B, size_t* n);
int dl4ds_graph_dropout_get_mask(dl4ds_graph* g, int index, int B, float* dst_host);
int dl4ds_graph_dropout_set_mask(dl4ds_graph* g, int index, int B, const float* src_host);
/* reseed: every dropout op gets the seed mix(seed, op index) and its draw counter goes back to 0, so the masks drawn by the
 * forward passes that follow (fixed batch size) are a pure function of `seed`: a reproducible MC ensemble (blocks.py:658-676).
 * The scheme, all mod 2^64 with G = 0x9E3779B97F4A7C15 and splitmix64 the finaliser z ^= z >> 30, z *= 0xBF58476D1CE4E5B9,
 * z ^= z >> 27, z *= 0x94D049BB133111EB, z ^= z >> 31:  op i (creation order) has the seed s_i = splitmix64(seed + G * (i + 1));
 * element e of its k-th drawing forward pass (k = 1, 2, ...) takes z = splitmix64(s_i + k * 0x1000003 + G * (e + 1)),
 * u = (z >> 40) / 2^24 and u2 = ((z >> 16) & 0xFFFFFF) / 2^24; the keep mask is 1 iff u >= rate (in fp32), the Gaussian noise
 * 1 + sqrt(rate / (1 - rate)) * sqrt(-2 ln(1 - u)) * cos(2 pi u2).
 * A graph that was never reseeded draws as if reseeded with the built-in seed 0x5DEECE66D: its ops' seeds are hashed the same
 * way (they used to be 0x5DEECE66D + G * (i + 1) un-hashed, which made the mask of op i + 1 the mask of op i shifted by one
 * element).  mc_count: dropout ops that are active at inference (mc != 0, rate > 0). */
int dl4ds_graph_dropout_reseed(dl4ds_graph* g, unsigned long long seed);
int dl4ds_graph_dropout_mc_count(dl4ds_graph* g, int* n);
/* LayerNormalization(axis=-1) (batch == 0; mov_* ignored) / BatchNormalization(axis=-1, momentum=0.99) (batch != 0)
 * as instantiated by blocks.py:63-71,151-159,293-296; relu != 0 fuses the activation that follows the layer. */
int dl4ds_graph_norm(dl4ds_graph* g, int in, int gamma, int beta, int mov_mean, int mov_var, int batch, float eps, int relu,
                     int* out);
int dl4ds_graph_output(dl4ds_graph* g, int tensor_id);
int dl4ds_graph_finalize(dl4ds_graph* g);
int dl4ds_graph_tensor_shape(dl4ds_graph* g, int tensor_id, int shape4[4]);   /* nmul,H,W,C */
/* parameters: flat fp32 arena; param_id -> (offset, n).  model.get_weights()/set_weights() analogue */
int dl4ds_graph_param_count(dl4ds_graph* g, size_t* n_arena, int* n_params);
int dl4ds_graph_param_info(dl4ds_graph* g, int param_id, size_t* offset, size_t* n);
int dl4ds_graph_set_param(dl4ds_graph* g, int param_id, const float* src_host);
int dl4ds_graph_get_param(dl4ds_graph* g, int param_id, float* dst_host);
int dl4ds_graph_get_grad(dl4ds_graph* g, int param_id, float* dst_host);
int dl4ds_graph_arena_ptrs(dl4ds_graph* g, float** w_dev, float** g_dev);
/* model(inputs, training=...) / model.predict -- inference.py:238; cgan.py:597-600.
 * inputs: n_inputs pointers in graph-input order; is_host selects host or device pointers.
 * out: output tensor 0 copied to out (host or device per is_host); synchronous if is_host. */
int dl4ds_graph_forward(dl4ds_graph* g, const float* const* inputs, int n_inputs, int B, int training, int is_host,
                        float* out);
int dl4ds_graph_tensor_ptr(dl4ds_graph* g, int tensor_id, int grad, float** p_dev);
/* which passes of ChannelAttention2D (blocks.py:585-593) the neighbouring convolutions took over for batch size B
 * (pooling from the producer's epilogue, scale in the consumer's loads, dX in the producer's backward loads): a JSON list,
 * one object per attention layer.  Diagnostics / tests; DL4DS_NO_TAIL_FUSION=1 turns the hand-over off. */
int dl4ds_graph_fusion_report(dl4ds_graph* g, int B, char* json_buf, size_t buflen);
/* weight-gradient calls this graph has issued on the second stream since it was created (read-only; DL4DS_AUX_STREAM=1 at
 * dl4ds_graph_create, profiler off); 0 for a graph created without the switch.  Diagnostics / tests. */
int dl4ds_graph_aux_launches(dl4ds_graph* g, long* n);
/* the gradient buckets of the data-parallel all-reduce (hvd.DistributedOptimizer's fusion buffer, supervised.py:363-365;
 * hvd.DistributedGradientTape, cgan.py:608-611) in LAUNCH order: a JSON list of {bytes, offset, params,
 * final_after_backward_of_op, of_ops} -- bucket k's ncclAllReduce is queued on the communication stream as soon as the
 * backward pass has run forward op number `final_after_backward_of_op` (the tail of the network goes first). */
int dl4ds_graph_bucket_plan(dl4ds_graph* g, char* json_buf, size_t buflen);

/* ---------------------------------------------------------------- training
 * replaces the Keras fit inner step configured by SupervisedTrainer.run (supervised.py:336-353,396-406):
 * forward -> loss -> backward -> [RCCL all-reduce] -> Adam(PiecewiseConstantDecay). */
int dl4ds_trainer_create(dl4ds_graph* g, int loss_kind, float lr0, float lr1, double lr_boundary, float beta1,
                         float beta2, float eps, dl4ds_trainer** tr);
int dl4ds_trainer_destroy(dl4ds_trainer* tr);
/* one optimisation step.  inputs in graph-input order; y_true (B*nmul,H,W,C) of output 0.
 * loss_host: NULL -> fully asynchronous step; else the loss value (forces a stream sync). */
int dl4ds_trainer_step(dl4ds_trainer* tr, const float* const* inputs, int n_inputs, const float* y_true, int B,
                       int is_host, float* loss_host);
/* loss/gradients without the optimiser update (tests; model.evaluate analogue) */
int dl4ds_trainer_loss_and_grads(dl4ds_trainer* tr, const float* const* inputs, int n_inputs, const float* y_true,
                                 int B, int is_host, float* loss_host);
/* model.evaluate (supervised.py:396-409 validation / test loss): inference-mode forward + loss, no gradients, no
 * BatchNormalization moving-average update, dropout inactive unless it is an MC variant */
int dl4ds_trainer_evaluate(dl4ds_trainer* tr, const float* const* inputs, int n_inputs, const float* y_true, int B,
                           int is_host, float* loss_host);
/* per-grid-cell weights of the trainer's loss (semantics: dl4ds_op_loss_weighted).  w: w_batch maps of (H, W, w_channels), host
 * (is_host) or device; copied into a trainer-owned buffer asynchronously on the library stream (a host array must stay alive until the
 * next synchronising call) and in force for dl4ds_trainer_step / _loss_and_grads / _evaluate until replaced; w == NULL clears them and
 * the unweighted kernels run again.  H, W must be those of output 0 and w_channels 1 or its channel count.  w_batch is 1 (shared map)
 * or the batch size B of the following steps (one map per sample, every frame of a spatio-temporal sample uses its sample's map); a
 * step whose B differs from a per-sample w_batch fails.  Trainers of a msdssim loss fail at the step. */
int dl4ds_trainer_set_loss_weights(dl4ds_trainer* tr, const float* w, int w_batch, int H, int W, int w_channels, int is_host);
int dl4ds_trainer_get_state(dl4ds_trainer* tr, float* m_host, float* v_host, long* step);
/* restore the Adam slots (arena-sized host arrays) and optimizer.iterations -- resume from a checkpoint
 * (the reference resumes through tf.train.Checkpoint, cgan.py:288-292; supervised.py:322-325 re-uses a trained model) */
int dl4ds_trainer_set_state(dl4ds_trainer* tr, const float* m_host, const float* v_host, long step);
int dl4ds_trainer_last_loss(dl4ds_trainer* tr, float* loss_host);   /* synchronises */
/* Optimiser extensions (semantics: dl4ds_op_adam_ext), between steps, any number of times.  global_clipnorm 0: no clipping.
 * weight_decay applies to the parameters decay_param_ids[n_ids] (dl4ds_graph_param ids).  ema_momentum in [0, 1) switches the weight
 * average on -- the first time it allocates a shadow arena initialised as a copy of the current weights (the Keras optimiser's
 * `average` slots), later calls keep it -- and a negative value switches it off and frees the arena.  With all three off the step is
 * the plain Adam launch.  The step counter counts attempted steps: a step skipped for a non-finite gradient norm still advances the
 * learning-rate schedule and the bias correction.  Data parallel: the norm is taken on the all-reduced arena, 1/world folded in. */
int dl4ds_trainer_set_optimizer_ext(dl4ds_trainer* tr, float global_clipnorm, float weight_decay, const int* decay_param_ids,
                                    int n_ids, float ema_momentum);
/* the last step's gradient norm (0 without clipping) and clip factor, and the count of skipped steps; synchronises */
int dl4ds_trainer_optimizer_stats(dl4ds_trainer* tr, float* norm, float* factor, long* skipped);
/* exchanges the weights and their averages in one kernel (exact; twice = identity); the average must be on */
int dl4ds_trainer_ema_swap(dl4ds_trainer* tr);
/* the averages as one arena-sized host array (layout: dl4ds_graph_param_info) -- checkpoints; synchronise */
int dl4ds_trainer_ema_get(dl4ds_trainer* tr, float* ema_host);
int dl4ds_trainer_ema_set(dl4ds_trainer* tr, const float* ema_host);

/* CGAN step -- cgan.py:575-639 with generator_loss (:525-553, lambda) and discriminator_loss (:556-572).
 * gen: generator graph (inputs: lr[, static]); disc: discriminator graph (inputs: lr, hr/generated).
 * losses_host[4] = gen_total, gen_gan, gen_px, disc (NULL -> asynchronous).
 * dropout_keep_host: optional 2*B*C keep-mask (real rows first) for the discriminator's Dropout(0.4). */
int dl4ds_cgan_create(dl4ds_graph* gen, dl4ds_graph* disc, int px_loss_kind, float lr, float beta1, float lam,
                      dl4ds_trainer** tr);
/* genlr, dislr = learning_rates (cgan.py:271-278): one Adam(beta_1=0.5) per model, each with its own rate */
int dl4ds_cgan_set_learning_rates(dl4ds_trainer* tr, float gen_lr, float disc_lr);
/* dl4ds_trainer_set_loss_weights for the CGAN step's pixel loss (gen_px and its gradient) only: the adversarial terms are untouched */
int dl4ds_cgan_set_loss_weights(dl4ds_trainer* tr, const float* w, int w_batch, int H, int W, int w_channels, int is_host);
int dl4ds_cgan_step(dl4ds_trainer* tr, const float* const* gen_inputs, int n_gen_inputs, const float* hr, int B,
                    int is_host, const float* dropout_keep_host, int apply_update, float* losses_host);
/* Adam slots + optimizer.iterations of the generator (which = 0) / discriminator (which = 1) optimiser -- the contents of
 * the reference's tf.train.Checkpoint(generator_optimizer, discriminator_optimizer, generator, discriminator)
 * (cgan.py:288-292) and what load_checkpoint restores (cgan.py:447-522) */
int dl4ds_cgan_get_state(dl4ds_trainer* tr, int which, float* m_host, float* v_host, long* step);
int dl4ds_cgan_set_state(dl4ds_trainer* tr, int which, const float* m_host, const float* v_host, long step);
/* the optimiser extensions of the generator (which = 0) / discriminator (which = 1) optimiser; the weight average exists for the
 * generator only (ema_momentum must be negative for which = 1) and dl4ds_cgan_ema_* act on it */
int dl4ds_cgan_set_optimizer_ext(dl4ds_trainer* tr, int which, float global_clipnorm, float weight_decay, const int* decay_param_ids,
                                 int n_ids, float ema_momentum);
int dl4ds_cgan_optimizer_stats(dl4ds_trainer* tr, int which, float* norm, float* factor, long* skipped);
int dl4ds_cgan_ema_swap(dl4ds_trainer* tr);
int dl4ds_cgan_ema_get(dl4ds_trainer* tr, float* ema_host);
int dl4ds_cgan_ema_set(dl4ds_trainer* tr, const float* ema_host);
int dl4ds_cgan_get_disc_grad(dl4ds_trainer* tr, int param_id, float* dst_host);

/* ---------------------------------------------------------------- batch preparation (SURVEY section 8 "next" row f1)
 * One training batch gathered from a DEVICE-resident dataset; replaces the per-sample numpy/cv2 loop of
 * create_batch_hr_lr / create_pair_hr_lr (dataloader.py:297-360, 11-294) and crop_array / resize_array
 * (utils.py:251-401) for interpolation='inter_area' (integer ratio: block mean; re-expansion for 'pin': replication)
 * and no external LR array.
 *   hr_dev [N][H][W][C], pred_dev [N][H][W][P] or NULL, static_dev [H][W][S] or NULL (all float32, device)
 *   idx_host / cy_host / cx_host [B]: first frame of each sample and its crop corner in HR pixels (host ints; the
 *   caller draws them with the RNG calls of the reference's loop so both paths produce the same batch)
 *   T frames per sample (time_window, 1 for spatial models); patch psy x psx HR pixels (== H x W when not cropping)
 *   pin = 0: out_lr [B][T][psy/scale][psx/scale][C+P(+S)]     pin = 1: out_lr [B][T][psy][psx][C+P(+S)]
 *   static_in_lr: append the (block-mean / raw) static variables to lr (spatial models, dataloader.py:261-289)
 *   out_hr [B][T][psy][psx][C], out_static [B][psy][psx][S] (NULL when S == 0).  Asynchronous on the library stream. */
int dl4ds_batch_prepare(const float* hr_dev, const float* pred_dev, const float* static_dev, const int* idx_host,
                        const int* cy_host, const int* cx_host, float* out_lr_dev, float* out_hr_dev,
                        float* out_static_dev, int H, int W, int C, int P, int S, int T, int B, int scale, int psy,
                        int psx, int pin, int static_in_lr);

/* The same for every interpolation of resize_array (utils.py:369-381: cv2 INTER_NEAREST / INTER_CUBIC / INTER_LINEAR /
 * INTER_AREA / INTER_LANCZOS4).  cv2.resize is separable; one axis of it is a device table of k (source index, weight)
 * taps per output row / column, [n_out][k], built once by the caller from cv2's coefficients.  Each table argument points
 * at two axes {y, x}:
 *   dn_patch : resize of a psy x psx PATCH to (psy/scale) x (psx/scale), indices relative to the patch  (post-upsampling:
 *              the HR crop and the cropped static variables, dataloader.py:141-205,261-289)
 *   dn_field : resize of the whole H x W field to (H/scale) x (W/scale)  (predictors, dataloader.py:150-160; 'pin')
 *   up_field : resize of the (H/scale) x (W/scale) field back to H x W   ('pin', dataloader.py:94-112)
 * scratch_dev: 'pin' only, [B][T][H/scale][W/scale][C+P] floats.  Unused tables may be NULL. */
typedef struct dl4ds_tap_axis { const int* idx; const float* wt; int k; } dl4ds_tap_axis;
int dl4ds_batch_prepare_taps(const float* hr_dev, const float* pred_dev, const float* static_dev, const int* idx_host,
                             const int* cy_host, const int* cx_host, float* out_lr_dev, float* out_hr_dev,
                             float* out_static_dev, float* scratch_dev, int H, int W, int C, int P, int S, int T, int B,
                             int scale, int psy, int psx, int pin, int static_in_lr, const dl4ds_tap_axis* dn_patch,
                             const dl4ds_tap_axis* dn_field, const dl4ds_tap_axis* up_field);

/* The gather pass of the two entries above as a primitive, for the input forms of create_pair_hr_lr they do not cover
 * (dataloader.py:72-73,92-96,149-163,193-200: a caller-supplied LR array, predictors already on the LR grid; utils.py:369-381:
 * cv2.INTER_AREA between grids whose ratio is not an integer):
 *   out[b][t][oy][ox][:] = concat over the groups g of
 *     raw              : src_g[frame][cy_b / row_div + oy][cx_b / row_div + ox][:]      (row_div 0: the corner as given)
 *     origin_from_crop : sum_k wy[oy][ky] wx[ox][kx] src_g[frame][cy_b + iy[oy][ky]][cx_b + ix[ox][kx]][:]  (a PATCH was resized)
 *     row_div > 0      : the same with table rows oy + cy_b / row_div, ox + cx_b / row_div and no origin (the FIELD was resized,
 *                        then cropped on the output grid);   otherwise rows oy, ox, no crop
 *   frame = idx[b] + t (frames 0: dataset), b T + t (frames 1: a batch-local scratch of an earlier pass) or 0 (frames 2: one image).
 * <= 3 groups; idx / cy / cx are host lists of B ints (cy / cx NULL: no crop; idx NULL only without dataset-indexed groups).
 * Asynchronous on the library stream. */
typedef struct dl4ds_gather_group {
    const float* src_dev; int channels; int frames; int src_h; int src_w; int raw; int origin_from_crop; int row_div;
    dl4ds_tap_axis taps[2];
} dl4ds_gather_group;
int dl4ds_batch_gather(const dl4ds_gather_group* groups, int n_groups, const int* idx_host, const int* cy_host,
                       const int* cx_host, float* out_dev, int out_h, int out_w, int T, int B);

/* ---------------------------------------------------------------- tiled prediction
 * The reference predicts a whole field in one call (inference.py:238, `model.predict(x_test_lr)`), with every activation of the full
 * grid alive; Model.predict_tiled runs the network on overlapping tiles (dl4ds_batch_gather -> dl4ds_graph_forward with device
 * pointers) and this entry merges a batch of tile outputs into the output field on the device:
 *   out[sample[t]][oy[t] + y][ox[t] + x][c] += wy[wy_row[t]][y] * wx[wx_row[t]][x] * tiles[t][y][x][c]      t < n, y < th, x < tw
 *   tiles_dev [n][th][tw][C], out_dev [N][H][W][C], wy_dev [wy_rows][th], wx_dev [wx_rows][tw] (fp32, device); the five lists are
 *   host arrays of n ints: output origin of each tile, the sample it belongs to, its row in either weight table.
 * Summation order: an output element is owned by one thread per call, which walks the covering tiles of the call in ascending t
 * and applies acc = fmaf(w, v, acc) with w = wy * wx rounded to fp32, starting from the stored value; calls are ordered on the
 * library stream.  Tiles handed over in ascending order therefore give the same bits however they are split into calls.  No
 * floating-point atomics.  A tap whose wy or wx is exactly 0 is skipped (not multiplied): non-finite values under a zero weight
 * never reach the output, and 0/1 weights copy the tile value.  16-byte accesses where tw * C, W * C and every ox * C are
 * multiples of 4 and both pointers are 16-byte aligned, 4-byte accesses otherwise.  Cost beyond the streaming: each workgroup (one row
 * of one tile) scans the n tiles of the call once and keeps those that share its row in LDS, which is why n is limited to 256; a
 * longer batch is split into calls, which does not change a bit.  Refused before anything is launched: null
 * pointers, sizes < 1, n > 256 or th > 65535, a tile that leaves the output, a sample or table row out of range, and a call made while
 * the device error word is set (it stays set for dl4ds_sync to report).  Asynchronous on the library stream. */
int dl4ds_tile_merge(const float* tiles_dev, int n, int th, int tw, int C, const int* oy_host, const int* ox_host,
                     const int* sample_host, const int* wy_row_host, const int* wx_row_host, const float* wy_dev, int wy_rows,
                     const float* wx_dev, int wx_rows, float* out_dev, int N, int H, int W);

/* The field mean that ChannelAttention2D (blocks.py:585-593) needs when its input exists only tile by tile.  tile_pool adds, in fp64 and
 * in a fixed order (no floating-point atomics), sum_yx wy[wy_row[t]][y] * wx[wx_row[t]][x] * tiles[t][y][x][c] to
 * sums_dev[sample[t]][c] ([N][C] doubles): with the 0/1 weights of a 'crop' plan every pixel of the field counts once.  chatt_info:
 * the graph's channel-attention ops in op order (an index past the last one is an error), the tensor each one pools (dl4ds_graph_tensor_ptr gives its data after a
 * forward pass), its channel count, and whether that tensor is a plain contiguous [B][H][W][C] array of a 4-D model.  chatt_set_mean:
 * the forward passes that follow use mean_dev [B][C] (device, read at each pass) instead of pooling over the op's input; NULL
 * restores the pooling.  Inference only. */
int dl4ds_tile_pool(const float* tiles_dev, int n, int th, int tw, int C, const int* sample_host, const int* wy_row_host,
                    const int* wx_row_host, const float* wy_dev, int wy_rows, const float* wx_dev, int wx_rows, double* sums_dev,
                    int N);
int dl4ds_graph_chatt_info(dl4ds_graph* g, int index, int* tensor_in, int* channels, int* contiguous);
int dl4ds_graph_chatt_set_mean(dl4ds_graph* g, int index, const float* mean_dev);

/* ---------------------------------------------------------------- regridding between rectilinear grids
 * No counterpart in the reference, whose one route between a coarse and a fine grid is the index-space resize of create_pair_hr_lr
 * (dl4ds_batch_gather).  x [N][H][W][C] fp32 -> out [N][H'][W'][C] fp32 through one table per axis.  A table is CSR: the taps of
 * destination index d are ptr[d] ... ptr[d + 1] - 1 (int), tap t reads source index idx[t] (int) with weight w[t] >= 0 (fp64);
 * conservative, bilinear and nearest regridding on rectilinear grids all have this form (dl4ds_amd/regrid.py builds them).
 *
 * plan_create: host tables of both axes (y: H' + 1 ptr entries over sources 0 ... H - 1; x: W' + 1 over 0 ... W - 1) and the
 * destination cell measures ay_host [H'], ax_host [W'] (fp64; the area of cell (i', j') is ay[i'] * ax[j'], used by the consistency
 * sums only) -> a handle.  Refused before anything is allocated or uploaded: an extent < 1, H*W or H'*W' >= 2^31, a null table, a
 * ptr that does not start at 0 or decreases, a source index out of range, a weight or measure that is negative or not finite.  The
 * tables are uploaded once, synchronously.  plan_destroy waits for the library stream and frees them; the handle is dead afterwards.
 *
 * apply: one thread per output element (n, i', j', c) walks the y-taps a of i' in table order and inside each the x-taps b of j' in
 * table order, in fp64 with every operation rounded on its own (no FMA contraction):
 *     w = wy[a] * wx[b];   tot = tot + w
 *     skipna and x not finite:  continue
 *     num = num + w * (double)x[n, iy[a], ix[b], c];   den = den + w
 *     out = (den > 0 and den >= min_valid * tot) ? (float)(num / den) : NaN
 * Without skipna every tap is taken (den == tot; non-finite inputs propagate by IEEE rules); with it NaN and +-inf are dropped (the
 * masking convention of dl4ds_quantile_table) and min_valid in [0, 1] is the share of the weight that must remain.  An output
 * without taps is NaN; every NaN stored is the canonical quiet NaN 0x7fc00000.  No atomics: the result is a pure function of the input and the tables, the same bits for any N and any
 * split of the samples into calls.  64-bit offsets.  16-byte accesses where C is a multiple of 4 and both pointers are 16-byte
 * aligned (then W*C and W'*C are multiples of 4 too), 4-byte accesses otherwise.  The x-taps of a workgroup's columns sit in LDS
 * (up to 2048 of them; beyond that they are read from the table in global memory), the y-taps of its row in scalar registers.
 * Algorithmic traffic: 4 * N * C * (H W + H' W') bytes, one read of the input and one write of the output; when refining, the taps
 * of neighbouring outputs overlap and the re-reads come from cache.  Asynchronous on the library stream; out_dev must not alias x_dev.
 *
 * consistency: r = the value apply stores (rounded to fp32), y = ref_dev[n, i', j', c] ([N][H'][W'][C] fp32).  A cell is valid where
 * both are finite; there d = (double)r - (double)y and A = ay[i'] * ax[j'].  sums_dev [N][C][6] fp64: sum A, sum A*d, sum A*(d*d),
 * sum A*y, sum A*r, max |d|;  counts_dev [N][C][2] int64: valid cells, cells where exactly one side is finite;  resid_dev (or NULL)
 * [N][H'][W'][C] fp32: r - y, NaN where the cell is not valid.  ONE summation order (regrid_core.h): lane t of 256 joins the cells
 * j' = t, t + 256, ... of a row in ascending j'; a fixed tree (o = 128 ... 1: lane t < o joins lane t + o) joins the lanes; the rows are
 * joined in ascending i' from zero.  A repeated call, any N and any split of the samples give the same bits.  Outputs are
 * overwritten.  Algorithmic traffic: 4 * N * C * (H W + H' W') bytes read (+ the residual written).  Asynchronous on the library stream.
 *
 * apply and consistency refuse, before anything is launched: a null or destroyed plan, null required pointers, N or C < 1, min_valid
 * outside [0, 1] or NaN, and a call made while the device error word is set (it stays set for dl4ds_sync to report). */
typedef struct dl4ds_regrid_plan dl4ds_regrid_plan;
int dl4ds_regrid_plan_create(int H, int W, int Ho, int Wo, const int* yptr_host, const int* yidx_host, const double* yw_host,
                             const int* xptr_host, const int* xidx_host, const double* xw_host, const double* ay_host,
                             const double* ax_host, dl4ds_regrid_plan** plan);
int dl4ds_regrid_plan_destroy(dl4ds_regrid_plan* plan);
int dl4ds_regrid_apply(const dl4ds_regrid_plan* plan, const float* x_dev, int N, int C, int skipna, double min_valid, float* out_dev);
int dl4ds_regrid_consistency(const dl4ds_regrid_plan* plan, const float* x_dev, const float* ref_dev, int N, int C, int skipna,
                             double min_valid, double* sums_dev, long long* counts_dev, float* resid_dev);

/* ---------------------------------------------------------------- data parallelism (RCCL over xGMI)
 * replaces Horovod: hvd.init/rank/size (base.py:97-107), DistributedOptimizer / DistributedGradientTape
 * gradient averaging (supervised.py:365; cgan.py:608-611), broadcast of variables + optimiser slots from
 * rank 0 (supervised.py:369; cgan.py:633-637). */
int dl4ds_dist_unique_id(char id128[128]);                       /* rank 0: ncclGetUniqueId */
int dl4ds_dist_init(int rank, int world, const char id128[128]); /* ncclCommInitRank on the current device */
int dl4ds_dist_world(int* rank, int* world);
int dl4ds_dist_broadcast_trainer(dl4ds_trainer* tr, int root);   /* params + Adam m,v + step */
int dl4ds_dist_allreduce_sum(float* buf_dev, size_t n);          /* on the library stream */
int dl4ds_dist_finalize(void);
/* Fail-safe: the launcher's WORLD_SIZE (1 when unset or DL4DS_ALLOW_UNSYNCED=1).  dl4ds_trainer_step, dl4ds_cgan_step and
 * dl4ds_dist_broadcast_trainer return an error -- they do NOT fall back to local training -- when it is > 1 and no
 * communicator of that size exists (hvd.init() is unconditional in the reference, base.py:97-107). */
int dl4ds_dist_expected_world(int* world);
/* what RCCL reports for the communicator: ncclCommCount / ncclCommUserRank / ncclCommCuDevice (nranks 0: none) */
int dl4ds_dist_comm_info(int* nranks, int* rank, int* device);
/* in-place reduction of n <= 1024 host floats across the ranks; op: 0 sum, 1 max, 2 min; synchronous; identity without a
 * communicator.  Validation / test losses and the early-stopping decision (hvd.callbacks.MetricAverageCallback,
 * supervised.py:366-368), max-over-ranks timing. */
int dl4ds_dist_allreduce_host(float* values_host, int n, int op);
int dl4ds_dist_barrier(void);                                    /* stream sync + a 1-float all-reduce */

#ifdef __cplusplus
}
#endif
#endif /* DL4DS_HIP_H */
