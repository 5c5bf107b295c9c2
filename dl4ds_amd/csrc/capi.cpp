// extern "C" boundary of libdl4ds_hip.so -- see include/dl4ds_hip.h for the contract of every symbol.
#include "../../include/dl4ds_hip.h"
#include "graph.h"
#include "runtime.h"
#include "dist.h"
#include "prof.h"
#include <algorithm>
#include <cmath>
#include <cstring>
#include <cstdlib>
#include <mutex>
#include <set>
#include <vector>

// ---- internal functions defined in other translation units
Trainer* trainer_create(Graph* g, int loss_kind, const AdamCfg& cfg);
void graph_load_inputs(Graph& g, const float* const* inputs, int n_inputs, int B, bool is_host);
void trainer_evaluate(Trainer& t, const float* const* inputs, int n_inputs, const float* y_true, int B, bool is_host);
void trainer_loss_and_grads(Trainer& t, const float* const* inputs, int n_inputs, const float* y_true, int B, bool is_host,
                            bool reduce_across_ranks);
void trainer_step(Trainer& t, const float* const* inputs, int n_inputs, const float* y_true, int B, bool is_host, float* loss_host);
void trainer_set_optimizer_ext(Trainer& t, float clipnorm, float weight_decay, const int* decay_param_ids, int n_ids, float ema_momentum);
void trainer_optimizer_stats(Trainer& t, float* norm, float* factor, long* skipped);
void trainer_ema_swap(Trainer& t);
void trainer_ema_get(Trainer& t, float* host);
void trainer_ema_set(Trainer& t, const float* host);
struct CganTrainer;
CganTrainer* cgan_create(Graph* gen, Graph* disc, int px_loss_kind, float lr, float beta1, float lam);
void cgan_destroy(CganTrainer* t);
void cgan_step(CganTrainer& t, const float* const* gen_inputs, int n_gen_inputs, const float* hr, int B, bool is_host,
               const float* dropout_keep_host, bool apply_update, float* losses_host);
Trainer* cgan_disc_trainer(CganTrainer* t);
Trainer* cgan_gen_trainer(CganTrainer* t);
void cgan_set_learning_rates(CganTrainer* t, float gen_lr, float disc_lr);
void cgan_set_loss_weights(CganTrainer* t, const float* w, int w_batch, int H, int W, int w_channels, bool is_host);

namespace {
thread_local std::string g_last_error;
Runtime g_rt;
std::mutex g_rt_mu;
}  // namespace

Runtime& rt() { return g_rt; }
void set_last_error(const std::string& s) { g_last_error = s; }

// ---- sticky device-side error word (runtime.h)
namespace {
unsigned* g_err_host = nullptr;       // pinned, mapped
unsigned* g_err_dev = nullptr;
}  // namespace
unsigned* device_error_word() {
    if (!g_err_dev) {
        HIP_CHECK(hipHostMalloc((void**)&g_err_host, sizeof(unsigned), hipHostMallocMapped));
        *g_err_host = 0u;
        HIP_CHECK(hipHostGetDevicePointer((void**)&g_err_dev, g_err_host, 0));
    }
    return g_err_dev;
}
unsigned* device_error_word_if_any() { return g_err_dev; }
void device_error_check(const char* what) {
    if (!g_err_host) return;
    const unsigned code = *reinterpret_cast<volatile unsigned*>(g_err_host);
    if (!code) return;
    *g_err_host = 0u;                  // reported once; the step that raised it is lost either way
    std::string msg = std::string(what) + ": a kernel reported a device-side error (code " + std::to_string(code) + ")";
    if (code & DEV_ERR_CONVLSTM_SEQ_TIMEOUT)
        msg += ": the persistent ConvLSTM kernel gave up waiting for a neighbouring tile (its workgroups were not all resident, "
               "e.g. behind kernels of another stream or an RCCL collective held up by a late rank); the activations and "
               "gradients of that step are INVALID.  DL4DS_NO_CONVLSTM_SEQ=1 runs the recurrence step by step";
    if (code & DEV_ERR_OBJECTS_WALK)
        msg += ": a parent walk of the object labelling passed the bound its field size sets (a link that points upwards or out "
               "of the field); the outputs of that call are INVALID";
    throw Dl4dsError(msg);
}

void rt_ensure_init() {
    std::lock_guard<std::mutex> lk(g_rt_mu);
    if (g_rt.inited) return;
    int dev = 0;
    HIP_CHECK(hipGetDevice(&dev));
    g_rt.device = dev;
    HIP_CHECK(hipStreamCreateWithFlags(&g_rt.stream, hipStreamNonBlocking));
    HIP_CHECK(hipStreamCreateWithFlags(&g_rt.comm_stream, hipStreamNonBlocking));
    HIP_CHECK(hipStreamCreateWithFlags(&g_rt.aux_stream, hipStreamNonBlocking));
    HIP_CHECK(hipEventCreate(&g_rt.ev0));
    HIP_CHECK(hipEventCreate(&g_rt.ev1));
    g_rt.inited = true;
}

#define API_BEGIN try {
#define API_END                                   \
    }                                             \
    catch (const std::exception& e) {             \
        set_last_error(e.what());                 \
        return -1;                                \
    }                                             \
    catch (...) {                                 \
        set_last_error("unknown C++ exception");  \
        return -1;                                \
    }                                             \
    return 0;

struct dl4ds_graph { Graph g; };
struct dl4ds_trainer {
    Trainer* t = nullptr;          // supervised trainer
    CganTrainer* c = nullptr;      // or a CGAN trainer
};

static hipStream_t S() { rt_ensure_init(); return rt().stream; }
static float* scratch(size_t bytes) {       // grow-only scratch for the single-op entry points
    static float* p = nullptr;
    static size_t cap = 0;
    if (bytes > cap) {
        HIP_CHECK(hipStreamSynchronize(S()));
        if (p) HIP_CHECK(hipFree(p));
        HIP_CHECK(hipMalloc((void**)&p, bytes));
        cap = bytes;
    }
    return p;
}
static float* nc(const float* p) { return const_cast<float*>(p); }
// The three B-element index lists of a batch (first frame, crop corner; a null list: zeros) travel in one small upload into a
// persistent device buffer, grown on demand -> [idx | cy | cx].  The upload is ordered on the library stream behind the previous
// batch's kernels, which read the old contents.
static const int* upload_index_lists(const int* idx_host, const int* cy_host, const int* cx_host, int B) {
    static int* d_idx = nullptr;
    static int cap = 0;
    static std::vector<int> h_idx;
    if (3 * B > cap) {
        if (d_idx) HIP_CHECK(hipFree(d_idx));
        cap = std::max(3 * B, 3 * 256);
        HIP_CHECK(hipMalloc((void**)&d_idx, (size_t)cap * sizeof(int)));
    }
    h_idx.assign(3 * (size_t)B, 0);
    for (int b = 0; b < B; ++b) {
        if (idx_host) h_idx[b] = idx_host[b];
        if (cy_host) h_idx[B + b] = cy_host[b];
        if (cx_host) h_idx[2 * B + b] = cx_host[b];
    }
    HIP_CHECK(hipMemcpyAsync(d_idx, h_idx.data(), 3 * (size_t)B * sizeof(int), hipMemcpyHostToDevice, S()));
    return d_idx;
}

extern "C" {

const char* dl4ds_last_error(void) { return g_last_error.c_str(); }

int dl4ds_init(int device) {
    API_BEGIN
    {
        std::lock_guard<std::mutex> lk(g_rt_mu);
        DL4DS_REQUIRE(!g_rt.inited || g_rt.device == device, "dl4ds_init: already initialised on another device");
        HIP_CHECK(hipSetDevice(device));
    }
    rt_ensure_init();
    API_END
}
int dl4ds_device_count(int* n) {
    API_BEGIN
    HIP_CHECK(hipGetDeviceCount(n));
    API_END
}
int dl4ds_device_name(char* buf, int buflen) {
    API_BEGIN
    rt_ensure_init();
    hipDeviceProp_t prop;
    HIP_CHECK(hipGetDeviceProperties(&prop, rt().device));
    std::snprintf(buf, buflen, "%s (%s, %d CUs)", prop.name, prop.gcnArchName, prop.multiProcessorCount);
    API_END
}
int dl4ds_malloc(void** p, size_t bytes) {
    API_BEGIN
    rt_ensure_init();
    const hipError_t e = hipMalloc(p, bytes > 0 ? bytes : 4);
    if (e != hipSuccess) {
        // a refused allocation is reported here and nowhere else: the runtime also keeps it as the thread's "last error", where
        // the hipGetLastError() after the next kernel launch would find it and blame that launch
        (void)hipGetLastError();
        throw Dl4dsError(std::string("HIP error: ") + hipGetErrorString(e) + " (hipMalloc of " + std::to_string(bytes) + " bytes)");
    }
    API_END
}
int dl4ds_free(void* p) {
    API_BEGIN
    if (p) { HIP_CHECK(hipStreamSynchronize(S())); HIP_CHECK(hipFree(p)); }
    API_END
}
int dl4ds_memcpy_h2d(void* dst, const void* src, size_t bytes) {
    API_BEGIN
    HIP_CHECK(hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, S()));
    HIP_CHECK(hipStreamSynchronize(S()));
    API_END
}
int dl4ds_memcpy_d2h(void* dst, const void* src, size_t bytes) {
    API_BEGIN
    HIP_CHECK(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, S()));
    HIP_CHECK(hipStreamSynchronize(S()));
    API_END
}
int dl4ds_host_register(void* p, size_t bytes) {
    API_BEGIN
    DL4DS_REQUIRE(p && bytes, "host_register: empty range");
    const hipError_t e = hipHostRegister(p, bytes, hipHostRegisterDefault);
    if (e != hipSuccess) {
        (void)hipGetLastError();           // (callers go on with pageable copies: the refusal must not surface at the next launch)
        throw Dl4dsError(std::string("HIP error: ") + hipGetErrorString(e) + " (hipHostRegister)");
    }
    API_END
}
int dl4ds_host_unregister(void* p) {
    API_BEGIN
    HIP_CHECK(hipHostUnregister(p));
    API_END
}
int dl4ds_memcpy_d2d(void* dst, const void* src, size_t bytes) {
    API_BEGIN
    HIP_CHECK(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToDevice, S()));
    API_END
}
int dl4ds_memset(void* p, int value, size_t bytes) {
    API_BEGIN
    HIP_CHECK(hipMemsetAsync(p, value, bytes, S()));
    API_END
}
int dl4ds_sync(void) {
    API_BEGIN
    dist_stream_sync(S(), "dl4ds_sync");          // (plain hipStreamSynchronize unless several ranks take part)
    API_END
}
namespace {
__global__ void raise_device_error_kernel(unsigned* word, unsigned code) {
    __hip_atomic_fetch_or(word, code, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}
}  // namespace
int dl4ds_debug_raise_device_error(int code) {
    API_BEGIN
    hipLaunchKernelGGL(raise_device_error_kernel, dim3(1), dim3(1), 0, S(), device_error_word(), (unsigned)code);
    HIP_CHECK(hipGetLastError());
    API_END
}
int dl4ds_event_timer_start(void) {
    API_BEGIN
    HIP_CHECK(hipEventRecord(rt().ev0, S()));
    API_END
}
int dl4ds_event_timer_stop(float* ms) {
    API_BEGIN
    HIP_CHECK(hipEventRecord(rt().ev1, S()));
    HIP_CHECK(hipEventSynchronize(rt().ev1));
    HIP_CHECK(hipEventElapsedTime(ms, rt().ev0, rt().ev1));
    API_END
}

int dl4ds_profile_enable(int on) {
    API_BEGIN
    HIP_CHECK(hipStreamSynchronize(S()));
    prof().reset();
    prof().on = (on != 0);
    API_END
}
int dl4ds_profile_filter(const char* tag_prefix) {
    API_BEGIN
    prof().filter = tag_prefix ? tag_prefix : "";
    API_END
}
int dl4ds_profile_report(char* buf, size_t buflen) {
    API_BEGIN
    const std::string r = prof().report_json(S());
    DL4DS_REQUIRE(r.size() + 1 <= buflen, "profile report buffer too small");
    std::memcpy(buf, r.c_str(), r.size() + 1);
    API_END
}

// ------------------------------------------------------------------------------------------------ ops
int dl4ds_op_conv2d_fwd(const float* x, const float* w, const float* b, const float* add, float* y, int N, int H, int W,
                        int Cin, int Cout, int KS, int relu, int d2s_r) {
    API_BEGIN
    TView in = make_view(nc(x), N, H, W, Cin);
    TView out = (d2s_r > 1) ? make_view_d2s(y, N, H, W, Cout, d2s_r) : make_view(y, N, H, W, Cout);
    ConvEpilogue ep;
    ep.bias = b;
    if (add) ep.add = make_view(nc(add), N, H, W, Cout);
    ep.relu = relu;
    conv2d_forward(S(), in, w, KS, out, ep);
    API_END
}
int dl4ds_op_conv2d_epilogue(const float* x, const float* w, const float* b, const float* add, const float* mask, float* y, int N,
                             int H, int W, int Cin, int Cout, int KS, int relu, int accumulate) {
    API_BEGIN
    ConvEpilogue ep;
    ep.bias = b;
    if (add) ep.add = make_view(nc(add), N, H, W, Cout);
    if (mask) ep.mask = make_view(nc(mask), N, H, W, Cout);
    ep.relu = relu;
    ep.accumulate = accumulate;
    conv2d_forward(S(), make_view(nc(x), N, H, W, Cin), w, KS, make_view(y, N, H, W, Cout), ep);
    API_END
}
int dl4ds_op_conv2d_second_output(const float* x, const float* w, const float* b, const float* sum_add, float* sum_out, const float* mask,
                                  const float* mask2, float* y2, float* partial, float* y, int N, int H, int W, int Cin, int Cout, int KS,
                                  int relu, int* launched) {
    API_BEGIN
    DL4DS_REQUIRE(launched != nullptr, "conv2d_second_output: launched is null");
    ConvEpilogue ep;
    ep.bias = b;
    ep.relu = relu;
    if (sum_add) ep.sum_add = make_view(nc(sum_add), N, H, W, Cout);
    if (sum_out) ep.sum_out = make_view(sum_out, N, H, W, Cout);
    if (mask) ep.mask = make_view(nc(mask), N, H, W, Cout);
    if (mask2) ep.mask2 = make_view(nc(mask2), N, H, W, Cout);
    if (y2) ep.out2 = make_view(y2, N, H, W, Cout);
    if (partial) ep.partial = make_view(partial, N, H, W, Cout);
    *launched = conv2d_forward_fused(S(), make_view(nc(x), N, H, W, Cin), w, KS, make_view(y, N, H, W, Cout), ep) ? 1 : 0;
    API_END
}
int dl4ds_op_add_act(const float* a, const float* b, float* out, size_t n, int relu) {
    API_BEGIN
    add_act(S(), a, b, out, n, relu);
    API_END
}
int dl4ds_op_masked_axpy_pair(const float* dy, const float* ya, float* da, const float* yb, float* db, size_t n, int* launched) {
    API_BEGIN
    DL4DS_REQUIRE(launched != nullptr, "masked_axpy_pair: launched is null");
    *launched = masked_axpy_pair(S(), dy, ya, da, 0, yb, db, 0, n) ? 1 : 0;
    API_END
}
int dl4ds_op_conv2d_dgrad(const float* dz, const float* w, float* dx, int N, int H, int W, int Cin, int Cout, int KS,
                          int d2s_r, int accumulate) {
    API_BEGIN
    const size_t nw = (size_t)KS * KS * Cin * Cout;
    float* wt = scratch(nw * sizeof(float));
    conv2d_dgrad_weights(S(), w, wt, KS, Cin, Cout);
    TView dzv = (d2s_r > 1) ? make_view_d2s(nc(dz), N, H, W, Cout, d2s_r) : make_view(nc(dz), N, H, W, Cout);
    ConvEpilogue ep;
    ep.accumulate = accumulate;
    conv2d_forward(S(), dzv, wt, KS, make_view(dx, N, H, W, Cin), ep);
    API_END
}
int dl4ds_op_conv2d_wgrad(const float* x, const float* dz, float* dw, int N, int H, int W, int Cin, int Cout, int KS,
                          int d2s_r, int accumulate) {
    API_BEGIN
    TView xv = make_view(nc(x), N, H, W, Cin);
    TView dzv = (d2s_r > 1) ? make_view_d2s(nc(dz), N, H, W, Cout, d2s_r) : make_view(nc(dz), N, H, W, Cout);
    const size_t ws = conv2d_wgrad_workspace_bytes(xv, dzv, KS);
    conv2d_wgrad(S(), xv, dzv, KS, dw, accumulate, nullptr, 0, scratch(ws), ws);
    API_END
}
// ---- the same convolutions on the operand forms the graph passes: channel slices, frame views, channel-affine read views
static TView desc_view(const dl4ds_view* d, int N, int H, int W, bool affine_allowed, const char* what) {
    DL4DS_REQUIRE(d && d->p, std::string(what) + ": view without a base pointer");
    DL4DS_REQUIRE(d->C >= 1 && (d->ld == 0 || d->ld >= (d->d2s > 1 ? d->C / (d->d2s * d->d2s) : d->C)), std::string(what) + ": pitch below the channel count");
    DL4DS_REQUIRE(affine_allowed || (!d->sc && !d->sh), std::string(what) + ": only a read operand (x; dz of a weight gradient) takes a channel affine");
    DL4DS_REQUIRE(d->sc || !d->sh, std::string(what) + ": a shift needs a scale");
    TView v;
    if (d->d2s > 1) {
        DL4DS_REQUIRE(d->C % (d->d2s * d->d2s) == 0, std::string(what) + ": depth_to_space needs C % r^2 == 0");
        v = make_view_d2s(nc(d->p), N, H, W, d->C, d->d2s);
        if (d->ld) { v.ld = d->ld; v.vec = v.vec && (d->ld & 3) == 0; }
        v.nstride = d->nstride ? d->nstride : (size_t)H * d->d2s * W * d->d2s * v.ld;
    } else {
        const int ld = d->ld ? d->ld : d->C;
        v = make_pitched_view(nc(d->p), N, H, W, d->C, ld, d->nstride ? d->nstride : (size_t)H * W * ld);
    }
    v.sc = d->sc; v.sh = d->sh;
    return v;
}
int dl4ds_op_conv2d_views(const dl4ds_view* x, const float* w, const float* b, const dl4ds_view* add, const dl4ds_view* mask,
                          const dl4ds_view* y, int N, int H, int W, int KS, int relu, int accumulate, int dgrad) {
    API_BEGIN
    const TView in = desc_view(x, N, H, W, true, "conv2d_views x");
    const TView out = desc_view(y, N, H, W, false, "conv2d_views y");
    ConvEpilogue ep;
    ep.bias = b;
    if (add) ep.add = desc_view(add, N, H, W, false, "conv2d_views add");
    if (mask) ep.mask = desc_view(mask, N, H, W, false, "conv2d_views mask");
    DL4DS_REQUIRE((!add || add->C == y->C) && (!mask || mask->C == y->C), "conv2d_views: add / mask have the output's channels");
    ep.relu = relu;
    ep.accumulate = accumulate;
    const float* filt = w;
    if (dgrad) {                 // w: the forward layer's [KS][KS][y.C][x.C] filter; the dgrad runs on its flipped transpose
        float* wt = scratch((size_t)KS * KS * in.C * out.C * sizeof(float));
        conv2d_dgrad_weights(S(), w, wt, KS, out.C, in.C);
        filt = wt;
    }
    conv2d_forward(S(), in, filt, KS, out, ep);
    API_END
}
int dl4ds_op_conv2d_wgrad_views(const dl4ds_view* x, const dl4ds_view* dz, float* dw, int N, int H, int W, int KS, int accumulate,
                                float* db, int accumulate_db) {
    API_BEGIN
    const TView xv = desc_view(x, N, H, W, true, "conv2d_wgrad_views x");
    const TView dzv = desc_view(dz, N, H, W, true, "conv2d_wgrad_views dz");
    const size_t ws = conv2d_wgrad_workspace_bytes(xv, dzv, KS);
    conv2d_wgrad(S(), xv, dzv, KS, dw, accumulate, db, accumulate_db, scratch(ws), ws);
    API_END
}
int dl4ds_op_conv2d_wgrad_attention(const dl4ds_view* x, const dl4ds_view* dz, const float* scale, const float* w, float* dw, int N, int H,
                                    int W, int KS, int accumulate, float* db, int accumulate_db, float* ds, int* launched) {
    API_BEGIN
    DL4DS_REQUIRE(launched != nullptr && scale && w && dw && ds, "conv2d_wgrad_attention: null operand");
    const TView xv = desc_view(x, N, H, W, false, "conv2d_wgrad_attention x");
    const TView dzv = desc_view(dz, N, H, W, false, "conv2d_wgrad_attention dz");
    const size_t ws = conv2d_direct_wgrad_attention_workspace_bytes(xv, dzv, KS);
    *launched = conv2d_direct_wgrad_attention(S(), xv, dzv, KS, scale, w, dw, accumulate, db, accumulate_db, ds, scratch(ws), ws) ? 1 : 0;
    API_END
}
int dl4ds_op_bias_act_bwd(float* dy, const float* y, float* db, int N, int H, int W, int C) {
    API_BEGIN
    TView dyv = make_view(dy, N, H, W, C);
    TView none{nullptr, 0, 0, 0, 0, 0, 0, 0};
    const size_t ws = bias_grad_workspace_bytes(dyv);
    bias_act_backward(S(), dyv, y ? make_view(nc(y), N, H, W, C) : none, y ? dyv : none, db, 0, scratch(ws), ws);
    API_END
}
int dl4ds_op_conv2d_transpose_fwd(const float* x, const float* w, float* y, int N, int H, int W, int Cin, int Cout,
                                  int KS, int stride, int relu) {
    API_BEGIN
    TView in = make_view(nc(x), N, H, W, Cin);
    TView out = make_view(y, N, H * stride, W * stride, Cout);
    const size_t ws = conv2d_transpose_workspace_bytes(in, out, KS, stride);
    conv2d_transpose_forward(S(), in, w, KS, stride, out, relu, scratch(ws), ws);
    API_END
}
int dl4ds_op_conv2d_transpose_dgrad(const float* dz, const float* w, float* dx, int N, int H, int W, int Cin, int Cout,
                                    int KS, int stride, int accumulate) {
    API_BEGIN
    TView dxv = make_view(dx, N, H, W, Cin);
    TView dzv = make_view(nc(dz), N, H * stride, W * stride, Cout);
    const size_t ws = conv2d_transpose_workspace_bytes(dxv, dzv, KS, stride);
    conv2d_transpose_dgrad(S(), dzv, w, KS, stride, dxv, accumulate, scratch(ws), ws);
    API_END
}
int dl4ds_op_conv2d_transpose_wgrad(const float* x, const float* dz, float* dw, int N, int H, int W, int Cin, int Cout,
                                    int KS, int stride, int accumulate) {
    API_BEGIN
    TView xv = make_view(nc(x), N, H, W, Cin);
    TView dzv = make_view(nc(dz), N, H * stride, W * stride, Cout);
    const size_t ws = conv2d_transpose_workspace_bytes(xv, dzv, KS, stride);
    conv2d_transpose_wgrad(S(), xv, dzv, KS, stride, dw, accumulate, scratch(ws), ws);
    API_END
}
int dl4ds_batch_prepare(const float* hr, const float* pred, const float* stat, const int* idx_host, const int* cy_host,
                        const int* cx_host, float* out_lr, float* out_hr, float* out_stat, int H, int W, int C, int P, int S_,
                        int T, int B, int scale, int psy, int psx, int pin, int static_in_lr) {
    API_BEGIN
    DL4DS_REQUIRE(B > 0 && idx_host && cy_host && cx_host, "batch_prepare: index lists missing");
    const int* d_idx = upload_index_lists(idx_host, cy_host, cx_host, B);
    batch_prepare(S(), hr, pred, stat, d_idx, d_idx + B, d_idx + 2 * B, out_lr, out_hr, out_stat, H, W, C, P, S_, T, B, scale,
                  psy, psx, pin, static_in_lr);
    API_END
}
int dl4ds_batch_prepare_taps(const float* hr, const float* pred, const float* stat, const int* idx_host, const int* cy_host,
                             const int* cx_host, float* out_lr, float* out_hr, float* out_stat, float* scratch_dev, int H, int W,
                             int C, int P, int S_, int T, int B, int scale, int psy, int psx, int pin, int static_in_lr,
                             const dl4ds_tap_axis* dn_patch, const dl4ds_tap_axis* dn_field, const dl4ds_tap_axis* up_field) {
    API_BEGIN
    DL4DS_REQUIRE(B > 0 && idx_host && cy_host && cx_host, "batch_prepare_taps: index lists missing");
    const int* d_idx = upload_index_lists(idx_host, cy_host, cx_host, B);
    auto axes = [](const dl4ds_tap_axis* t, TapAxis* o) -> const TapAxis* {
        if (!t) return nullptr;
        for (int i = 0; i < 2; ++i) { o[i].idx = t[i].idx; o[i].wt = t[i].wt; o[i].k = t[i].k; }
        return o;
    };
    TapAxis a0[2], a1[2], a2[2];
    batch_prepare_taps(S(), hr, pred, stat, d_idx, d_idx + B, d_idx + 2 * B, out_lr, out_hr, out_stat, scratch_dev, H, W, C, P,
                       S_, T, B, scale, psy, psx, pin, static_in_lr, axes(dn_patch, a0), axes(dn_field, a1), axes(up_field, a2));
    API_END
}
int dl4ds_batch_gather(const dl4ds_gather_group* groups, int n_groups, const int* idx_host, const int* cy_host, const int* cx_host,
                       float* out_dev, int out_h, int out_w, int T, int B) {
    API_BEGIN
    DL4DS_REQUIRE(groups && n_groups >= 1 && n_groups <= 3 && B > 0, "batch_gather: groups / batch size");
    DL4DS_REQUIRE((cy_host == nullptr) == (cx_host == nullptr), "batch_gather: crop corner lists");
    const int* d_idx = upload_index_lists(idx_host, cy_host, cx_host, B);
    GatherGroup g[3];
    for (int i = 0; i < n_groups; ++i) {
        const dl4ds_gather_group& q = groups[i];
        DL4DS_REQUIRE(q.src_dev && q.channels > 0 && q.src_h > 0 && q.src_w > 0 && q.row_div >= 0, "batch_gather: group");
        // the kernel does not clamp: every crop has to stay inside its source (raw groups: the corner + the output extent; a patch that
        // was resized: the corner inside the field -- its tap indices are the caller's table, relative to the corner)
        for (int b = 0; b < B && (q.raw || q.origin_from_crop); ++b) {
            const int cy = cy_host ? cy_host[b] : 0, cx = cx_host ? cx_host[b] : 0;
            const int sy = q.row_div ? cy / q.row_div : cy, sx = q.row_div ? cx / q.row_div : cx;
            DL4DS_REQUIRE(cy >= 0 && cx >= 0 && sy < q.src_h && sx < q.src_w, "batch_gather: crop corner outside the source");
            if (q.raw) DL4DS_REQUIRE(sy + out_h <= q.src_h && sx + out_w <= q.src_w, "batch_gather: crop leaves the source");
        }
        g[i].src = q.src_dev; g[i].channels = q.channels; g[i].frames = q.frames; g[i].src_h = q.src_h; g[i].src_w = q.src_w;
        g[i].raw = q.raw; g[i].origin_from_crop = q.origin_from_crop; g[i].row_div = q.row_div;
        for (int k = 0; k < 2; ++k) { g[i].taps[k].idx = q.taps[k].idx; g[i].taps[k].wt = q.taps[k].wt; g[i].taps[k].k = q.taps[k].k; }
    }
    batch_gather(S(), g, n_groups, idx_host ? d_idx : nullptr, cy_host ? d_idx + B : nullptr, cy_host ? d_idx + 2 * B : nullptr, out_dev,
                 out_h, out_w, T, B);
    API_END
}
// k lists of n host ints -> one persistent device buffer [k][n], grown on demand; ordered on the library stream like
// upload_index_lists
static const int* upload_tile_lists(const int* const* src, int k, int n) {
    static int* d_lists = nullptr;
    static size_t cap = 0;
    static std::vector<int> h_lists;
    const size_t need = (size_t)k * n;
    if (need > cap) {
        if (d_lists) HIP_CHECK(hipFree(d_lists));
        d_lists = nullptr;
        cap = std::max<size_t>(need, 5 * 256);
        HIP_CHECK(hipMalloc((void**)&d_lists, cap * sizeof(int)));
    }
    h_lists.resize(need);
    for (int i = 0; i < k; ++i) std::copy(src[i], src[i] + n, h_lists.begin() + (size_t)i * n);
    HIP_CHECK(hipMemcpyAsync(d_lists, h_lists.data(), need * sizeof(int), hipMemcpyHostToDevice, S()));
    return d_lists;
}
int dl4ds_tile_pool(const float* tiles_dev, int n, int th, int tw, int C, const int* sample_host, const int* wy_row_host,
                    const int* wx_row_host, const float* wy_dev, int wy_rows, const float* wx_dev, int wx_rows, double* sums_dev,
                    int N) {
    API_BEGIN
    DL4DS_REQUIRE(tiles_dev && wy_dev && wx_dev && sums_dev, "tile_pool: null device pointer");
    DL4DS_REQUIRE(sample_host && wy_row_host && wx_row_host, "tile_pool: null host list");
    DL4DS_REQUIRE(n > 0 && th > 0 && tw > 0 && C > 0 && N > 0 && wy_rows > 0 && wx_rows > 0, "tile_pool: bad sizes");
    DL4DS_REQUIRE(n <= 65535 && (long long)th * tw < (1ll << 31), "tile_pool: at most 65535 tiles per call, 2^31 pixels per tile");
    for (int t = 0; t < n; ++t) {
        DL4DS_REQUIRE(sample_host[t] >= 0 && sample_host[t] < N, "tile_pool: sample index outside the sums");
        DL4DS_REQUIRE(wy_row_host[t] >= 0 && wy_row_host[t] < wy_rows && wx_row_host[t] >= 0 && wx_row_host[t] < wx_rows,
                      "tile_pool: weight-table row outside the table");
    }
    DL4DS_REQUIRE(!g_err_host || *reinterpret_cast<volatile unsigned*>(g_err_host) == 0u,
                  "tile_pool: device error word set (dl4ds_sync reports and clears it)");
    const int* src[3] = {sample_host, wy_row_host, wx_row_host};
    const int* d = upload_tile_lists(src, 3, n);
    double* partial = reinterpret_cast<double*>(scratch((size_t)n * C * sizeof(double)));
    tile_pool(S(), tiles_dev, wy_dev, wx_dev, d, d + n, d + 2 * n, n, th, tw, C, partial, sums_dev);
    API_END
}
int dl4ds_tile_merge(const float* tiles_dev, int n, int th, int tw, int C, const int* oy_host, const int* ox_host,
                     const int* sample_host, const int* wy_row_host, const int* wx_row_host, const float* wy_dev, int wy_rows,
                     const float* wx_dev, int wx_rows, float* out_dev, int N, int H, int W) {
    API_BEGIN
    DL4DS_REQUIRE(tiles_dev && wy_dev && wx_dev && out_dev, "tile_merge: null device pointer");
    DL4DS_REQUIRE(oy_host && ox_host && sample_host && wy_row_host && wx_row_host, "tile_merge: null host list");
    DL4DS_REQUIRE(n > 0 && th > 0 && tw > 0 && C > 0 && N > 0 && H > 0 && W > 0 && wy_rows > 0 && wx_rows > 0, "tile_merge: bad sizes");
    // the kernel keeps the tiles that share a row in an LDS list of 256 entries (tiles.hip)
    DL4DS_REQUIRE(n <= 256 && th <= 65535, "tile_merge: at most 256 tiles per call (split the batch: the result does not depend on it) and 65535 rows per tile");
    DL4DS_REQUIRE((long long)W * C < (1ll << 31) && (long long)tw * C < (1ll << 31), "tile_merge: a row of more than 2^31 floats");
    DL4DS_REQUIRE(th <= H && tw <= W, "tile_merge: tile larger than the output");
    bool vec = (tw * C) % 4 == 0 && ((long long)W * C) % 4 == 0 && (((uintptr_t)tiles_dev | (uintptr_t)out_dev) & 15) == 0;
    for (int t = 0; t < n; ++t) {
        DL4DS_REQUIRE(sample_host[t] >= 0 && sample_host[t] < N, "tile_merge: sample index outside the output");
        DL4DS_REQUIRE(oy_host[t] >= 0 && ox_host[t] >= 0 && oy_host[t] <= H - th && ox_host[t] <= W - tw,
                      "tile_merge: tile outside the output");
        DL4DS_REQUIRE(wy_row_host[t] >= 0 && wy_row_host[t] < wy_rows && wx_row_host[t] >= 0 && wx_row_host[t] < wx_rows,
                      "tile_merge: weight-table row outside the table");
        vec = vec && ((long long)ox_host[t] * C) % 4 == 0;
    }
    // a kernel of an earlier call raised the device error word: what this merge would read is invalid.  The word stays set; the next
    // host-side wait (dl4ds_sync) reports and clears it.
    DL4DS_REQUIRE(!g_err_host || *reinterpret_cast<volatile unsigned*>(g_err_host) == 0u,
                  "tile_merge: device error word set (dl4ds_sync reports and clears it)");
    const int* src[5] = {oy_host, ox_host, sample_host, wy_row_host, wx_row_host};
    const int* d_lists = upload_tile_lists(src, 5, n);
    tile_merge(S(), tiles_dev, wy_dev, wx_dev, out_dev, d_lists, d_lists + n, d_lists + 2 * n, d_lists + 3 * n, d_lists + 4 * n, n, th,
               tw, C, H, W, vec);
    API_END
}
// ---- regridding (regrid.hip).  A handle is valid from plan_create to plan_destroy: the live ones are kept here, so that a null, a
// destroyed or a foreign handle is refused rather than followed.
static std::set<const void*>& regrid_plans() {
    static std::set<const void*> live;
    return live;
}
static RegridPlan* regrid_plan_of(const char* what, const dl4ds_regrid_plan* plan) {
    DL4DS_REQUIRE(plan && regrid_plans().count(plan), std::string(what) + ": null or destroyed plan");
    return reinterpret_cast<RegridPlan*>(const_cast<dl4ds_regrid_plan*>(plan));
}
int dl4ds_regrid_plan_create(int H, int W, int Ho, int Wo, const int* yptr_host, const int* yidx_host, const double* yw_host,
                             const int* xptr_host, const int* xidx_host, const double* xw_host, const double* ay_host,
                             const double* ax_host, dl4ds_regrid_plan** plan) {
    API_BEGIN
    DL4DS_REQUIRE(plan, "regrid_plan_create: null handle pointer");
    *plan = nullptr;
    RegridPlan* p = regrid_plan_create(S(), H, W, Ho, Wo, yptr_host, yidx_host, yw_host, xptr_host, xidx_host, xw_host, ay_host, ax_host);
    regrid_plans().insert(p);
    *plan = reinterpret_cast<dl4ds_regrid_plan*>(p);
    API_END
}
int dl4ds_regrid_plan_destroy(dl4ds_regrid_plan* plan) {
    API_BEGIN
    RegridPlan* p = regrid_plan_of("regrid_plan_destroy", plan);
    regrid_plans().erase(plan);
    regrid_plan_destroy(S(), p);
    API_END
}
int dl4ds_regrid_apply(const dl4ds_regrid_plan* plan, const float* x_dev, int N, int C, int skipna, double min_valid, float* out_dev) {
    API_BEGIN
    const RegridPlan* p = regrid_plan_of("regrid_apply", plan);
    regrid_check_call("regrid_apply", p, x_dev, N, C, min_valid);
    DL4DS_REQUIRE(out_dev, "regrid_apply: null output pointer");
    DL4DS_REQUIRE(out_dev != x_dev, "regrid_apply: the output must not alias the input");
    // a kernel of an earlier call raised the device error word: what this call would read is invalid.  The word stays set; the next
    // host-side wait (dl4ds_sync) reports and clears it.
    DL4DS_REQUIRE(!g_err_host || *reinterpret_cast<volatile unsigned*>(g_err_host) == 0u,
                  "regrid_apply: device error word set (dl4ds_sync reports and clears it)");
    regrid_apply(S(), p, x_dev, N, C, skipna != 0, min_valid, out_dev);
    API_END
}
int dl4ds_regrid_consistency(const dl4ds_regrid_plan* plan, const float* x_dev, const float* ref_dev, int N, int C, int skipna,
                             double min_valid, double* sums_dev, long long* counts_dev, float* resid_dev) {
    API_BEGIN
    const RegridPlan* p = regrid_plan_of("regrid_consistency", plan);
    regrid_check_call("regrid_consistency", p, x_dev, N, C, min_valid);
    DL4DS_REQUIRE(ref_dev && sums_dev && counts_dev, "regrid_consistency: null pointer");
    DL4DS_REQUIRE(!g_err_host || *reinterpret_cast<volatile unsigned*>(g_err_host) == 0u,
                  "regrid_consistency: device error word set (dl4ds_sync reports and clears it)");
    const size_t ws = regrid_consistency_workspace_bytes(p, N, C);
    regrid_consistency(S(), p, x_dev, ref_dev, N, C, skipna != 0, min_valid, sums_dev, counts_dev, resid_dev, scratch(ws));
    API_END
}
int dl4ds_op_depth_to_space(const float* x, float* y, int N, int H, int W, int C, int r) {
    API_BEGIN
    depth_to_space(S(), x, y, N, H, W, C, r);
    API_END
}
int dl4ds_op_space_to_depth(const float* y, float* x, int N, int H, int W, int C, int r) {
    API_BEGIN
    space_to_depth(S(), y, x, N, H, W, C, r);
    API_END
}
int dl4ds_op_maxpool2_fwd(const float* x, float* y, int N, int H, int W, int C) {
    API_BEGIN
    maxpool2_forward(S(), make_view(nc(x), N, H, W, C), make_view(y, N, H / 2, W / 2, C));
    API_END
}
int dl4ds_op_maxpool2_bwd(const float* x, const float* y, const float* dy, float* dx, int N, int H, int W, int C) {
    API_BEGIN
    int acc = 0;
    if ((H | W) & 1) { fill(S(), dx, (size_t)N * H * W * C, 0.f); acc = 1; }
    maxpool2_backward(S(), make_view(nc(x), N, H, W, C), make_view(nc(y), N, H / 2, W / 2, C),
                      make_view(nc(dy), N, H / 2, W / 2, C), make_view(dx, N, H, W, C), acc);
    API_END
}
int dl4ds_op_dwconv_fwd(const float* x, const float* k, const float* bias, float* y, int N, int H, int W, int C, int KS) {
    API_BEGIN
    dwconv_forward(S(), x, k, bias, y, N, H, W, C, KS, 0, 0);
    API_END
}
int dl4ds_op_dwconv_bwd(const float* x, const float* k, const float* dy, float* dx, float* dk, float* db, int N, int H, int W, int C,
                        int KS, int accumulate) {
    API_BEGIN
    if (dx) dwconv_forward(S(), dy, k, nullptr, dx, N, H, W, C, KS, 1, accumulate);
    if (dk) {
        const size_t ws = dwconv_wgrad_workspace_bytes(C, KS);
        dwconv_wgrad(S(), x, dy, dk, db, accumulate, N, H, W, C, KS, scratch(ws), ws);
    }
    API_END
}
int dl4ds_op_layernorm_fwd(const float* x, const float* gamma, const float* beta, float* y, size_t npix, int C, float eps,
                           int relu) {
    API_BEGIN
    layernorm_forward(S(), x, gamma, beta, y, npix, C, eps, relu);
    API_END
}
int dl4ds_op_layernorm_bwd(const float* x, const float* y, const float* dy, const float* gamma, float* dx, float* dgamma,
                           float* dbeta, size_t npix, int C, float eps, int relu, int accumulate) {
    API_BEGIN
    const size_t ws = norm_workspace_bytes(C);
    layernorm_backward(S(), x, y, dy, gamma, dx, accumulate, dgamma, dbeta, accumulate, npix, C, eps, relu, scratch(ws), ws);
    API_END
}
int dl4ds_op_batchnorm_fwd(const float* x, const float* gamma, const float* beta, float* moving_mean, float* moving_var,
                           float* y, float* saved, size_t npix, int C, float eps, float momentum, int training, int relu) {
    API_BEGIN
    const size_t ws = norm_workspace_bytes(C);
    batchnorm_forward(S(), x, gamma, beta, moving_mean, moving_var, y, saved, npix, C, eps, momentum, training, relu,
                      scratch(ws), ws);
    API_END
}
int dl4ds_op_batchnorm_bwd(const float* x, const float* y, const float* dy, const float* gamma, const float* saved, float* dx,
                           float* dgamma, float* dbeta, size_t npix, int C, int relu, int accumulate) {
    API_BEGIN
    const size_t ws = norm_workspace_bytes(C);
    batchnorm_backward(S(), x, y, dy, gamma, saved, dx, accumulate, dgamma, dbeta, accumulate, npix, C, relu, scratch(ws), ws);
    API_END
}
int dl4ds_op_resize_bilinear_fwd(const float* x, float* y, int N, int H, int W, int C, int Ho, int Wo) {
    API_BEGIN
    resize_bilinear_forward(S(), make_view(nc(x), N, H, W, C), make_view(y, N, Ho, Wo, C));
    API_END
}
int dl4ds_op_resize_bilinear_bwd(const float* dy, float* dx, int N, int H, int W, int C, int Ho, int Wo) {
    API_BEGIN
    resize_bilinear_backward(S(), make_view(nc(dy), N, Ho, Wo, C), make_view(dx, N, H, W, C), 0);
    API_END
}
int dl4ds_op_localconv_fwd(const float* x, const float* w, const float* b, float* y, int N, int H, int W, int C, int F) {
    API_BEGIN
    localconv_forward(S(), make_view(nc(x), N, H, W, C), w, b, make_view(y, N, H, W, F));
    API_END
}
int dl4ds_op_localconv_bwd(const float* x, const float* w, const float* dy, float* dx, float* dw, float* db, int N,
                           int H, int W, int C, int F) {
    API_BEGIN
    TView dxv{nullptr, 0, 0, 0, 0, 0, 0, 0};
    if (dx) dxv = make_view(dx, N, H, W, C);
    localconv_backward(S(), make_view(nc(x), N, H, W, C), w, make_view(nc(dy), N, H, W, F), dxv, 0, dw, db, 0);
    API_END
}
int dl4ds_op_chatt_fwd(const float* x, float* y, int G, int R, int P, int C, int Cr, const float* w1, const float* b1,
                       const float* w2, const float* b2, float* saved) {
    API_BEGIN
    AttShape sh{G, R, P, C, Cr};
    const size_t inst = (size_t)G * P;
    float* mean = saved;
    float* scale = mean + inst * C;
    float* hidden = scale + inst * C;
    chatt_forward(S(), x, y, sh, w1, b1, w2, b2, mean, hidden, scale, scratch(chatt_workspace_bytes(sh)));
    API_END
}
int dl4ds_op_chatt_bwd(const float* x, const float* dy, float* dx, int G, int R, int P, int C, int Cr, const float* w1,
                       const float* w2, const float* saved, float* dw1, float* db1, float* dw2, float* db2) {
    API_BEGIN
    AttShape sh{G, R, P, C, Cr};
    const size_t inst = (size_t)G * P;
    const float* mean = saved;
    const float* scale = mean + inst * C;
    const float* hidden = scale + inst * C;
    chatt_backward(S(), x, dy, dx, 0, sh, w1, w2, mean, hidden, scale, dw1, db1, dw2, db2, 0,
                   scratch(chatt_workspace_bytes(sh)));
    API_END
}
int dl4ds_op_loss(int kind, const float* yt, const float* yp, float* dpred, int N, int H, int W, int C, float* loss_dev) {
    API_BEGIN
    const size_t ws = loss_workspace_bytes(kind, N, H, W, C);
    loss_forward_backward(S(), kind, yt, yp, dpred, N, H, W, C, 1.f, loss_dev, 0, scratch(ws), ws);
    API_END
}
int dl4ds_op_loss_scaled(int kind, const float* yt, const float* yp, float* dpred, int N, int H, int W, int C, float scale,
                         int accumulate, float* loss_dev) {
    API_BEGIN
    const size_t ws = loss_workspace_bytes(kind, N, H, W, C);
    loss_forward_backward(S(), kind, yt, yp, dpred, N, H, W, C, scale, loss_dev, accumulate, scratch(ws), ws);
    API_END
}
int dl4ds_op_loss_weighted(int kind, const float* yt, const float* yp, float* dpred, int N, int H, int W, int C, const float* w,
                           int w_batch, int w_channels, float* loss_dev) {
    API_BEGIN
    DL4DS_REQUIRE(w && w_batch >= 1 && N > 0 && N % w_batch == 0 && (w_channels == 1 || w_channels == C),
                  "op_loss_weighted: w_batch must divide N and w_channels must be 1 or C");
    const size_t ws = loss_workspace_bytes_weighted(kind, N, H, W, C, w_batch, w_channels);
    loss_forward_backward_weighted(S(), kind, yt, yp, dpred, N, H, W, C, 1.f, loss_dev, 0, w, w_batch, w_channels, scratch(ws), ws);
    API_END
}
int dl4ds_metrics(const float* yt, const float* yp, int N, int H, int W, int C, float* pair_out_dev, float* grid_out_dev,
                  float* range_out_dev) {
    API_BEGIN
    const size_t ws = metrics_workspace_bytes(N, H, W, C);
    image_metrics(S(), yt, yp, N, H, W, C, pair_out_dev, grid_out_dev, range_out_dev, scratch(ws), ws);
    API_END
}
int dl4ds_spearman(const float* a, const float* b, size_t n_pairs, size_t L, size_t seg_stride, size_t elem_stride, double* out_dev) {
    API_BEGIN
    const size_t ws = spearman_workspace_bytes(n_pairs, L);
    spearman(S(), a, b, n_pairs, L, seg_stride, elem_stride, out_dev, ws ? scratch(ws) : nullptr, ws);
    API_END
}
int dl4ds_scaler_cells(const size_t* shape, int ndim, const int* reduce, size_t* cells_out) {
    API_BEGIN
    *cells_out = scaler_cells(shape, ndim, reduce);
    API_END
}
int dl4ds_scaler_stats_workspace_bytes(const size_t* shape, int ndim, const int* reduce, int is_double, size_t* bytes_out) {
    API_BEGIN
    *bytes_out = scaler_stats_workspace_bytes(shape, ndim, reduce, is_double);
    API_END
}
int dl4ds_scaler_stats(const void* x, int is_double, const size_t* shape, int ndim, const int* reduce, double* out_dev,
                       unsigned* nan_flag_dev, unsigned* mask_bits_dev) {
    API_BEGIN
    const size_t ws = scaler_stats_workspace_bytes(shape, ndim, reduce, is_double);
    scaler_stats(S(), x, is_double, shape, ndim, reduce, out_dev, nan_flag_dev, mask_bits_dev, ws ? scratch(ws) : nullptr, ws);
    API_END
}
int dl4ds_scaler_apply(const void* x, void* out, int is_double, const size_t* shape, int ndim, const int* reduce, int op1,
                       const void* a_dev, int op2, const void* b_dev, int nan_mode, double fill, const unsigned* mask_bits_dev) {
    API_BEGIN
    scaler_apply(S(), x, out, is_double, shape, ndim, reduce, op1, a_dev, op2, b_dev, nan_mode, fill, mask_bits_dev);
    API_END
}
int dl4ds_ensemble_reduce(const float* members_dev, size_t K, size_t n, size_t member_stride, const float* q_host, int nq,
                          float* mean_dev, float* std_dev, float* min_dev, float* max_dev, float* quant_dev) {
    API_BEGIN
    ensemble_reduce(S(), members_dev, K, n, member_stride, q_host, nq, mean_dev, std_dev, min_dev, max_dev, quant_dev);
    API_END
}
int dl4ds_ensemble_score(const float* members_dev, size_t K, size_t n, size_t member_stride, const float* obs_dev, size_t B,
                         unsigned long long elem_offset, const float* scale_dev, int fair, unsigned long long seed,
                         const float* q_host, int nq, float* crps_dev, float* sqerr_dev, float* var_dev, int* rank_dev,
                         double* sample_out_dev, double* cell_acc_dev, unsigned long long* rank_hist_dev,
                         unsigned long long* covered_dev) {
    API_BEGIN
    const size_t ws = ensemble_score_workspace_bytes(n, B ? B : 1);
    ensemble_score(S(), members_dev, K, n, member_stride, obs_dev, B, elem_offset, scale_dev, fair, seed, q_host, nq, crps_dev,
                   sqerr_dev, var_dev, rank_dev, sample_out_dev, cell_acc_dev, rank_hist_dev, covered_dev, ws ? scratch(ws) : nullptr,
                   ws);
    API_END
}
int dl4ds_ensemble_exceedance(const float* members_dev, size_t K, size_t n, size_t member_stride, const float* obs_dev, size_t B,
                              const float* thr_dev, int T, int thr_per_cell, short* count_dev, long long* sample_out_dev,
                              long long* cell_acc_dev, unsigned long long* table_dev) {
    API_BEGIN
    ensemble_exceedance(S(), members_dev, K, n, member_stride, obs_dev, B, thr_dev, T, thr_per_cell, count_dev, sample_out_dev,
                        cell_acc_dev, table_dev);
    API_END
}
int dl4ds_ensemble_exceedance_walk_limit(size_t K, size_t* samples_out) {
    API_BEGIN
    DL4DS_REQUIRE(K >= 1 && K <= ENS_MAX_MEMBERS, "ensemble_exceedance: 1 <= K <= 256 members");
    *samples_out = exc_walk_limit(K);
    API_END
}
int dl4ds_ensemble_energy(const float* members_dev, size_t K, size_t n, size_t member_stride, const float* obs_dev, size_t B,
                          const float* weight_dev, double* dist_out_dev, long long* nvalid_out_dev) {
    API_BEGIN
    ensemble_energy_check(members_dev, K, n, member_stride, obs_dev, B, dist_out_dev, nvalid_out_dev);    // before the workspace is sized
    const size_t ws = ensemble_energy_workspace_bytes(K, n, B);
    ensemble_energy(S(), members_dev, K, n, member_stride, obs_dev, B, weight_dev, dist_out_dev, nvalid_out_dev,
                    ws ? scratch(ws) : nullptr, ws);
    API_END
}
int dl4ds_ensemble_variogram(const float* members_dev, size_t K, size_t n, size_t member_stride, const float* obs_dev, size_t B,
                             const float* weight_dev, size_t planes, size_t H, size_t W, size_t C, int max_lag, int order_code,
                             long long* npairs_out_dev, double* sums_out_dev) {
    API_BEGIN
    ensemble_variogram_check(members_dev, K, n, member_stride, obs_dev, B, planes, H, W, C, max_lag, order_code, npairs_out_dev,
                             sums_out_dev);
    const size_t ws = ensemble_variogram_workspace_bytes(B, planes, H, C, max_lag);
    ensemble_variogram(S(), members_dev, K, n, member_stride, obs_dev, B, weight_dev, planes, H, W, C, max_lag, order_code,
                       npairs_out_dev, sums_out_dev, ws ? scratch(ws) : nullptr, ws);
    API_END
}
int dl4ds_variogram_lags(int max_lag, int* dydx_out, int* count_out) {
    API_BEGIN
    variogram_lags(max_lag, dydx_out, count_out);
    API_END
}
int dl4ds_fss(const float* y_dev, const float* p_dev, int N, int H, int W, int C, const float* thresholds_host, int T,
              const int* windows_host, int n_windows, long long* sums_dev, long long* cont_dev, long long* valid_dev) {
    API_BEGIN
    fss_check_args(N, H, W, C, thresholds_host, T, windows_host, n_windows);        // before the workspace is sized
    const size_t ws = fss_workspace_bytes(N, H, W, C, T);
    fss(S(), y_dev, p_dev, N, H, W, C, thresholds_host, T, windows_host, n_windows, sums_dev, cont_dev, valid_dev,
        ws ? scratch(ws) : nullptr, ws);
    API_END
}
int dl4ds_ensemble_fss(const float* members_dev, size_t K, size_t n, size_t member_stride, const float* obs_dev, size_t B, int H,
                       int W, int C, const float* thresholds_host, int T, const int* windows_host, int n_windows, long long* sums_dev,
                       long long* cont_dev, long long* valid_dev) {
    API_BEGIN
    ensemble_fss_check_args(members_dev, K, n, member_stride, obs_dev, B, H, W, C, thresholds_host, T, windows_host, n_windows, sums_dev,
                            cont_dev, valid_dev);                                    // before the workspace is sized
    const size_t ws = ensemble_fss_workspace_bytes(K, B, H, W, C, T);
    ensemble_fss(S(), members_dev, K, n, member_stride, obs_dev, B, H, W, C, thresholds_host, T, windows_host, n_windows, sums_dev, cont_dev,
                 valid_dev, ws ? scratch(ws) : nullptr, ws);
    API_END
}
int dl4ds_label_objects(const float* x_dev, int N, int H, int W, int C, const float* thr_dev, int connectivity, int cap,
                        int* labels_dev, int* count_dev, long long* nvalid_dev, double* field_sums_dev, long long* sums_dev,
                        int* bbox_dev, int* first_dev, float* vmax_dev, double* mass_dev) {
    API_BEGIN
    objects_check_args(x_dev, N, H, W, C, thr_dev, connectivity, cap, count_dev, sums_dev, bbox_dev, first_dev, vmax_dev,
                       mass_dev);                                                    // before the workspace is sized
    const size_t ws = objects_workspace_bytes(N, H, W, C);
    label_objects(S(), x_dev, N, H, W, C, thr_dev, connectivity, cap, labels_dev, count_dev, nvalid_dev, field_sums_dev, sums_dev,
                  bbox_dev, first_dev, vmax_dev, mass_dev, scratch(ws), ws, device_error_word());
    API_END
}
int dl4ds_object_thresholds(const float* x_dev, int N, int H, int W, int C, double factor, float* thr_dev) {
    API_BEGIN
    const size_t ws = object_thresholds_workspace_bytes(N, H, W, C);
    object_thresholds(S(), x_dev, N, H, W, C, factor, thr_dev, ws ? scratch(ws) : nullptr, ws);
    API_END
}
int dl4ds_distance_scores(const float* y_dev, const float* p_dev, int N, int H, int W, int C, const float* thresholds_host, int T,
                          double cutoff, double alpha, long long* counts_dev, double* sums_dev, int* d2_obs_dev, int* d2_pred_dev) {
    API_BEGIN
    distance_check_args(y_dev, p_dev, N, H, W, C, thresholds_host, T, cutoff, alpha, counts_dev, sums_dev);   // before the workspace is sized
    const size_t ws = distance_workspace_bytes(N, H, W, C, T);
    distance_scores(S(), y_dev, p_dev, N, H, W, C, thresholds_host, T, cutoff, alpha, counts_dev, sums_dev, d2_obs_dev, d2_pred_dev,
                    scratch(ws), ws);
    API_END
}
int dl4ds_distribution(const float* y_dev, const float* p_dev, size_t n_seg, size_t L, size_t seg_stride, size_t elem_stride,
                       const double* q_host, int Q, const float* edges_host, int E, double* quant_dev, double* w1_dev,
                       long long* ks_dev, long long* hist_dev, long long* valid_dev) {
    API_BEGIN
    distribution_check_args(n_seg, L, q_host, Q, edges_host, E);                     // before the workspace is sized
    const size_t ws = distribution_workspace_bytes(n_seg, L, seg_stride, elem_stride);
    distribution(S(), y_dev, p_dev, n_seg, L, seg_stride, elem_stride, q_host, Q, edges_host, E, quant_dev, w1_dev, ks_dev, hist_dev,
                 valid_dev, ws ? scratch(ws) : nullptr, ws);
    API_END
}
int dl4ds_quantile_table(const float* x_dev, size_t N, size_t per, const double* q_host, int Q, float* table_dev,
                         long long* valid_dev) {
    API_BEGIN
    const size_t ws = quantile_table_workspace_bytes(N, per);                        // (refuses sizes the entry does not take)
    quantile_table(S(), x_dev, N, per, q_host, Q, table_dev, valid_dev, ws ? scratch(ws) : nullptr, ws);
    API_END
}
int dl4ds_qmap_apply(const float* x_dev, float* out_dev, size_t B, size_t per, const float* model_tab_dev, const float* obs_tab_dev,
                     const float* target_tab_dev, int Q, int kind, int keep_unfitted, unsigned long long* counts_dev) {
    API_BEGIN
    qmap_apply(S(), x_dev, out_dev, B, per, model_tab_dev, obs_tab_dev, target_tab_dev, Q, kind, keep_unfitted, counts_dev);
    API_END
}
int dl4ds_climate_indices(const float* x_dev, size_t N, size_t per, const long long* period_starts_host, int P,
                          const float* thr_dev, int T, int thr_per_cell, int op, int window, int* valid_dev, int* event_dev,
                          float* ext_dev, double* sum_dev) {
    API_BEGIN
    const size_t ws = climate_indices_workspace_bytes(N, per, period_starts_host, P, T, op, window);      // (refuses a bad request)
    climate_indices(S(), x_dev, N, per, period_starts_host, P, thr_dev, T, thr_per_cell, op, window, valid_dev, event_dev, ext_dev,
                    sum_dev, scratch(ws), ws);
    API_END
}
int dl4ds_lmoments(const float* x_dev, size_t N, size_t per, size_t stride, int sign, int* valid_dev, double* pwm_dev) {
    API_BEGIN
    const size_t ws = lmoments_workspace_bytes(N, per, stride, sign);                // (refuses a bad request)
    lmoments(S(), x_dev, N, per, stride, sign, valid_dev, pwm_dev, ws ? scratch(ws) : nullptr, ws);
    API_END
}
int dl4ds_pot_peaks(const float* x_dev, size_t N, size_t per, const long long* period_starts_host, int P, const float* thr_dev,
                    int thr_per_cell, int sign, int run, int K, int* count_dev, float* peak_dev, int* pos_dev) {
    API_BEGIN
    const size_t ws = pot_peaks_workspace_bytes(N, per, period_starts_host, P, sign, run, K);              // (refuses a bad request)
    pot_peaks(S(), x_dev, N, per, period_starts_host, P, thr_dev, thr_per_cell, sign, run, K, count_dev, peak_dev, pos_dev,
              scratch(ws), ws);
    API_END
}
int dl4ds_temporal(const float* y_dev, const float* p_dev, size_t N, size_t per, const long long* period_starts_host, int P,
                   const int* lags_host, int L, const float* thr_dev, int T, int thr_per_cell, int op, int spell_bins,
                   int* valid_dev, double* moment_dev, int* pair_dev, double* lag_dev, int* trans_dev, int* spell_dev) {
    API_BEGIN
    const size_t ws = temporal_workspace_bytes(N, per, period_starts_host, P, lags_host, L, T, op, spell_bins);   // (refuses a bad request)
    temporal(S(), y_dev, p_dev, N, per, period_starts_host, P, lags_host, L, thr_dev, T, thr_per_cell, op, spell_bins, valid_dev,
             moment_dev, pair_dev, lag_dev, trans_dev, spell_dev, scratch(ws), ws);
    API_END
}
int dl4ds_trend(const double* v_dev, int P, size_t per, int* valid_dev, long long* mk_dev, double* sen_dev) {
    API_BEGIN
    trend(S(), v_dev, P, per, valid_dev, mk_dev, sen_dev);
    API_END
}
int dl4ds_spectrum(const float* y_dev, const float* p_dev, int N, int H, int W, int C, int detrend, int window, const int* bin_host,
                   int B, double* power_dev, long long* valid_dev, double* mean_dev) {
    API_BEGIN
    spectrum_check_args(N, H, W, C, bin_host, B);                                    // before the workspace is sized
    const size_t ws = spectrum_workspace_bytes(N, H, W, C, p_dev ? 2 : 1, B);
    spectrum(S(), y_dev, p_dev, N, H, W, C, detrend, window, bin_host, B, power_dev, valid_dev, mean_dev, ws ? scratch(ws) : nullptr,
             ws);
    API_END
}
int dl4ds_op_bce(const float* p, float label, int n, float* loss_dev, float* dp) {
    API_BEGIN
    bce_forward_backward(S(), p, label, n, 1.f, loss_dev, dp, 0);
    API_END
}
int dl4ds_op_adam(float* w, const float* g, float* m, float* v, size_t n, int t, float lr, float beta1, float beta2,
                  float eps, float grad_scale) {
    API_BEGIN
    const float lr_t = (float)((double)lr * std::sqrt(1.0 - std::pow((double)beta2, (double)t)) /
                               (1.0 - std::pow((double)beta1, (double)t)));
    adam_update(S(), w, g, m, v, n, lr_t, beta1, beta2, eps, grad_scale, device_error_word_if_any());       // (skips the update once the sticky word is set)
    API_END
}
int dl4ds_op_adam_ext(float* w, const float* g, float* m, float* v, float* ema, size_t n, int t, float lr, float beta1, float beta2,
                      float eps, float grad_scale, float global_clipnorm, float weight_decay, const size_t* decay_ranges_host,
                      int n_ranges, float ema_momentum, float* stats_out_dev) {
    API_BEGIN
    DL4DS_REQUIRE(global_clipnorm >= 0.f && std::isfinite(global_clipnorm), "global_clipnorm must be finite and > 0 (0: off)");
    DL4DS_REQUIRE(weight_decay >= 0.f && std::isfinite(weight_decay), "weight_decay must be finite and >= 0");
    DL4DS_REQUIRE(!ema || (ema_momentum >= 0.f && ema_momentum < 1.f), "ema_momentum must be in [0, 1)");
    DL4DS_REQUIRE(stats_out_dev, "stats_out_dev is required");
    DL4DS_REQUIRE(n_ranges >= 0 && (n_ranges == 0 || decay_ranges_host), "decay_ranges_host missing");
    const float lr_t = (float)((double)lr * std::sqrt(1.0 - std::pow((double)beta2, (double)t)) /
                               (1.0 - std::pow((double)beta1, (double)t)));
    static std::vector<size_t> b;              // (static: the upload below is asynchronous, as in upload_index_lists)
    b = decay_bounds(decay_ranges_host, n_ranges, n);
    // one scratch carve: the norm's fp64 partials, then the table
    const size_t part_bytes = (size_t)sqnorm_blocks(n) * sizeof(double);
    char* base = reinterpret_cast<char*>(scratch(part_bytes + std::max<size_t>(b.size(), 1) * sizeof(size_t)));
    size_t* bounds_dev = reinterpret_cast<size_t*>(base + part_bytes);
    if (!b.empty()) HIP_CHECK(hipMemcpyAsync(bounds_dev, b.data(), b.size() * sizeof(size_t), hipMemcpyHostToDevice, S()));
    adam_ext_update(S(), w, g, m, v, ema, n, lr_t, beta1, beta2, eps, grad_scale, global_clipnorm, lr, weight_decay,
                    b.empty() ? nullptr : bounds_dev, (int)b.size(), ema_momentum, reinterpret_cast<double*>(base), stats_out_dev,
                    device_error_word_if_any());
    API_END
}
int dl4ds_op_arena_swap(float* a, float* b, size_t n) {
    API_BEGIN
    arena_swap(S(), a, b, n);
    API_END
}

// ------------------------------------------------------------------------------------------------ graph
int dl4ds_graph_create(dl4ds_graph** g) {
    API_BEGIN
    *g = new dl4ds_graph();
    (*g)->g.stream = S();
    // Weight-gradient kernels on a second stream (concurrent with the dgrad chain) paid off with the LDS-staged conv
    // kernels (+2-3 %); with the streamed-filter / row-walking kernels two co-resident MFMA kernels only take matrix-core
    // and L1 bandwidth from each other (-2 % measured), so the single-stream order is the default now.
    if (getenv("DL4DS_AUX_STREAM")) (*g)->g.aux_stream = rt().aux_stream;
    API_END
}
int dl4ds_graph_destroy(dl4ds_graph* g) {
    API_BEGIN
    if (g) { HIP_CHECK(hipStreamSynchronize(S())); delete g; }
    API_END
}
int dl4ds_graph_input(dl4ds_graph* g, int H, int W, int C, int nmul, int* tid) {
    API_BEGIN
    *tid = g->g.add_tensor(H, W, C, nmul, false, true);
    API_END
}
int dl4ds_graph_input_requires_grad(dl4ds_graph* g, int tid) {
    API_BEGIN
    DL4DS_REQUIRE(!g->g.finalized, "graph already finalized");
    GTensor& t = g->g.tensors.at(tid);
    DL4DS_REQUIRE(t.is_input, "not an input tensor");
    t.requires_grad = true;
    t.dep_grad_input = true;
    API_END
}
int dl4ds_graph_param(dl4ds_graph* g, size_t n, int* pid) {
    API_BEGIN
    *pid = g->g.add_param(n);
    API_END
}
int dl4ds_graph_conv2d(dl4ds_graph* g, int in, int w, int b, int add, int KS, int Cout, int relu, int d2s_r, int* out) {
    API_BEGIN
    *out = g_conv2d(g->g, in, w, b, add, KS, Cout, relu, d2s_r);
    API_END
}
int dl4ds_graph_conv2d_transpose(dl4ds_graph* g, int in, int w, int KS, int stride, int Cout, int relu, int* out) {
    API_BEGIN
    *out = g_conv2d_transpose(g->g, in, w, KS, stride, Cout, relu);
    API_END
}
int dl4ds_graph_chatt_info(dl4ds_graph* g, int index, int* tensor_in, int* channels, int* contiguous) {
    API_BEGIN
    DL4DS_REQUIRE(g && tensor_in && channels && contiguous, "graph_chatt_info: null argument");
    g_chatt_info(g->g, index, tensor_in, channels, contiguous);
    API_END
}
int dl4ds_graph_chatt_set_mean(dl4ds_graph* g, int index, const float* mean_dev) {
    API_BEGIN
    DL4DS_REQUIRE(g, "graph_chatt_set_mean: null graph");
    g_chatt_set_mean(g->g, index, mean_dev);
    API_END
}
int dl4ds_graph_chatt(dl4ds_graph* g, int in, int w1, int b1, int w2, int b2, int Cr, int T5, int* out) {
    API_BEGIN
    *out = g_chatt(g->g, in, w1, b1, w2, b2, Cr, T5);
    API_END
}
int dl4ds_graph_concat(dl4ds_graph* g, const int* ins, int n, int* out) {
    API_BEGIN
    *out = g_concat(g->g, ins, n);
    API_END
}
int dl4ds_graph_add(dl4ds_graph* g, int a, int b, int relu, int* out) {
    API_BEGIN
    *out = g_add(g->g, a, b, relu);
    API_END
}
int dl4ds_graph_act(dl4ds_graph* g, int in, int kind, int* out) {
    API_BEGIN
    *out = g_act(g->g, in, kind);
    API_END
}
int dl4ds_graph_maxpool2(dl4ds_graph* g, int in, int* out) {
    API_BEGIN
    *out = g_maxpool2(g->g, in);
    API_END
}
int dl4ds_graph_resize(dl4ds_graph* g, int in, int Ho, int Wo, int* out) {
    API_BEGIN
    *out = g_resize(g->g, in, Ho, Wo);
    API_END
}
int dl4ds_graph_resize_nearest(dl4ds_graph* g, int in, int Ho, int Wo, int* out) {
    API_BEGIN
    *out = g_resize(g->g, in, Ho, Wo, 1);
    API_END
}
int dl4ds_graph_resize_bicubic(dl4ds_graph* g, int in, int Ho, int Wo, int* out) {
    API_BEGIN
    *out = g_resize(g->g, in, Ho, Wo, 2);
    API_END
}
int dl4ds_graph_resize_method(dl4ds_graph* g, int in, int Ho, int Wo, int method, int* out) {
    API_BEGIN
    *out = g_resize(g->g, in, Ho, Wo, method);
    API_END
}
int dl4ds_graph_localconv(dl4ds_graph* g, int in, int w, int b, int F, int* out) {
    API_BEGIN
    *out = g_localconv(g->g, in, w, b, F);
    API_END
}
int dl4ds_rec_tail_supported(int CX, int CS, int CO, int* yes) {
    API_BEGIN
    *yes = rec_tail_supported(CX, CS, CO) ? 1 : 0;
    API_END
}
int dl4ds_graph_rec_tail(dl4ds_graph* g, int x, int s, int wt, int bt, int wl, int bl, int w, int b, int T, int CO, int* out) {
    API_BEGIN
    *out = g_rec_tail(g->g, x, s, wt, bt, wl, bl, w, b, T, CO);
    API_END
}
int dl4ds_graph_repeat_time(dl4ds_graph* g, int in, int T, int* out) {
    API_BEGIN
    *out = g_repeat_time(g->g, in, T);
    API_END
}
int dl4ds_graph_convlstm(dl4ds_graph* g, int in, int wk, int wr, int b, int KS, int F, int T, int relu, int* out) {
    API_BEGIN
    *out = g_convlstm(g->g, in, wk, wr, b, KS, F, T, relu);
    API_END
}
int dl4ds_graph_gap(dl4ds_graph* g, int in, int* out) {
    API_BEGIN
    *out = g_gap(g->g, in, 0);
    API_END
}
int dl4ds_graph_dwconv(dl4ds_graph* g, int in, int w, int b, int KS, int* out) {
    API_BEGIN
    *out = g_dwconv(g->g, in, w, b, KS);
    API_END
}
int dl4ds_graph_gap3d(dl4ds_graph* g, int in, int* out) {
    API_BEGIN
    *out = g_gap(g->g, in, 1);
    API_END
}
int dl4ds_graph_conv2d_folded(dl4ds_graph* g, int in, int w1, int b1, int w2, int b2, int KS, int Cmid, int Cout, int relu, int d2s,
                              int* out) {
    API_BEGIN
    *out = g_conv2d_folded(g->g, in, w1, b1, w2, b2, KS, Cmid, Cout, relu, d2s);
    API_END
}
int dl4ds_graph_conv2d_folded_aux(dl4ds_graph* g, int in, int aux, int w1, int b1, int w2, int b2, int KS, int Cmid, int Cout,
                                  int relu, int d2s, int* out) {
    API_BEGIN
    *out = g_conv2d_folded(g->g, in, w1, b1, w2, b2, KS, Cmid, Cout, relu, d2s, aux);
    API_END
}
int dl4ds_graph_pad(dl4ds_graph* g, int in, int Ho, int Wo, int* out) {
    API_BEGIN
    *out = g_pad(g->g, in, Ho, Wo);
    API_END
}
int dl4ds_graph_slice(dl4ds_graph* g, int in, int oy, int ox, int step, int Ho, int Wo, int* out) {
    API_BEGIN
    *out = g_slice(g->g, in, oy, ox, step, Ho, Wo);
    API_END
}
int dl4ds_graph_dense(dl4ds_graph* g, int in, int w, int b, int F, int act, int* out) {
    API_BEGIN
    *out = g_dense(g->g, in, w, b, F, act);
    API_END
}
int dl4ds_graph_dropout(dl4ds_graph* g, int in, float rate, int* out) {
    API_BEGIN
    *out = g_dropout(g->g, in, rate);
    API_END
}
int dl4ds_graph_dropout_variant(dl4ds_graph* g, int in, float rate, int variant, int mc, int spatial_dim, int* out) {
    API_BEGIN
    *out = g_dropout(g->g, in, rate, variant, mc, spatial_dim);
    API_END
}
int dl4ds_graph_dropout_count(dl4ds_graph* g, int* n) {
    API_BEGIN
    *n = (int)g->g.dropout_ops.size();
    API_END
}
int dl4ds_graph_dropout_reseed(dl4ds_graph* g, unsigned long long seed) {
    API_BEGIN
    // splitmix64 of (seed, op index): neighbouring seeds and neighbouring ops get unrelated streams
    for (size_t i = 0; i < g->g.dropout_ops.size(); ++i) g->g.dropout_ops[i]->reseed(dropout_op_seed(seed, i));
    API_END
}
int dl4ds_graph_dropout_mc_count(dl4ds_graph* g, int* n) {
    API_BEGIN
    int c = 0;
    for (GOp* op : g->g.dropout_ops) c += op->mc_active() ? 1 : 0;
    *n = c;
    API_END
}
static GOp* dropout_op(dl4ds_graph* g, int index, int B) {
    DL4DS_REQUIRE(index >= 0 && index < (int)g->g.dropout_ops.size(), "dropout op index out of range");
    DL4DS_REQUIRE(g->g.finalized && B > 0 && B <= g->g.maxB, "dropout mask: graph not prepared for this batch size");
    return g->g.dropout_ops[index];
}
int dl4ds_graph_dropout_mask_size(dl4ds_graph* g, int index, int B, size_t* n) {
    API_BEGIN
    DL4DS_REQUIRE(index >= 0 && index < (int)g->g.dropout_ops.size(), "dropout op index out of range");
    *n = g->g.dropout_ops[index]->mask_floats(g->g, B);
    API_END
}
int dl4ds_graph_dropout_get_mask(dl4ds_graph* g, int index, int B, float* dst_host) {
    API_BEGIN
    GOp* op = dropout_op(g, index, B);
    HIP_CHECK(hipMemcpyAsync(dst_host, op->saved, op->mask_floats(g->g, B) * sizeof(float), hipMemcpyDeviceToHost, g->g.stream));
    HIP_CHECK(hipStreamSynchronize(g->g.stream));
    API_END
}
int dl4ds_graph_dropout_set_mask(dl4ds_graph* g, int index, int B, const float* src_host) {
    API_BEGIN
    GOp* op = dropout_op(g, index, B);
    op->set_mask(g->g, src_host, op->mask_floats(g->g, B));
    HIP_CHECK(hipStreamSynchronize(g->g.stream));
    API_END
}
int dl4ds_graph_norm(dl4ds_graph* g, int in, int gamma, int beta, int mov_mean, int mov_var, int batch, float eps, int relu,
                     int* out) {
    API_BEGIN
    *out = g_norm(g->g, in, gamma, beta, mov_mean, mov_var, batch, eps, relu);
    API_END
}
int dl4ds_graph_output(dl4ds_graph* g, int tid) {
    API_BEGIN
    DL4DS_REQUIRE(tid >= 0 && tid < (int)g->g.tensors.size(), "bad tensor id");
    g->g.outputs.push_back(tid);
    API_END
}
int dl4ds_graph_finalize(dl4ds_graph* g) {
    API_BEGIN
    g->g.finalize();
    API_END
}
int dl4ds_graph_tensor_shape(dl4ds_graph* g, int tid, int shape4[4]) {
    API_BEGIN
    const GTensor& t = g->g.tensors.at(tid);
    shape4[0] = t.nmul; shape4[1] = t.H; shape4[2] = t.W; shape4[3] = t.C;
    API_END
}
int dl4ds_graph_param_count(dl4ds_graph* g, size_t* n_arena, int* n_params) {
    API_BEGIN
    *n_arena = g->g.n_params;
    *n_params = (int)g->g.params.size();
    API_END
}
int dl4ds_graph_param_info(dl4ds_graph* g, int pid, size_t* offset, size_t* n) {
    API_BEGIN
    *offset = g->g.params.at(pid).offset;
    *n = g->g.params.at(pid).n;
    API_END
}
int dl4ds_graph_set_param(dl4ds_graph* g, int pid, const float* src) {
    API_BEGIN
    DL4DS_REQUIRE(g->g.finalized, "graph not finalized");
    const GParam& p = g->g.params.at(pid);
    HIP_CHECK(hipMemcpyAsync(g->g.W + p.offset, src, p.n * sizeof(float), hipMemcpyHostToDevice, S()));
    HIP_CHECK(hipStreamSynchronize(S()));
    API_END
}
int dl4ds_graph_get_param(dl4ds_graph* g, int pid, float* dst) {
    API_BEGIN
    const GParam& p = g->g.params.at(pid);
    HIP_CHECK(hipMemcpyAsync(dst, g->g.W + p.offset, p.n * sizeof(float), hipMemcpyDeviceToHost, S()));
    HIP_CHECK(hipStreamSynchronize(S()));
    API_END
}
int dl4ds_graph_get_grad(dl4ds_graph* g, int pid, float* dst) {
    API_BEGIN
    const GParam& p = g->g.params.at(pid);
    HIP_CHECK(hipMemcpyAsync(dst, g->g.G + p.offset, p.n * sizeof(float), hipMemcpyDeviceToHost, S()));
    HIP_CHECK(hipStreamSynchronize(S()));
    API_END
}
int dl4ds_graph_arena_ptrs(dl4ds_graph* g, float** w, float** gr) {
    API_BEGIN
    *w = g->g.W;
    *gr = g->g.G;
    API_END
}
int dl4ds_graph_forward(dl4ds_graph* g, const float* const* inputs, int n_inputs, int B, int training, int is_host,
                        float* out) {
    API_BEGIN
    Graph& G = g->g;
    DL4DS_REQUIRE(!G.outputs.empty(), "graph has no output");
    graph_load_inputs(G, inputs, n_inputs, B, is_host != 0);
    G.forward(B, training != 0);
    if (out) {
        const GTensor& o = G.tensors[G.outputs[0]];
        HIP_CHECK(hipMemcpyAsync(out, o.data, o.per_sample() * B * sizeof(float),
                                 is_host ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice, S()));
        if (is_host) HIP_CHECK(hipStreamSynchronize(S()));
    }
    API_END
}
int dl4ds_graph_fusion_report(dl4ds_graph* g, int B, char* json_buf, size_t buflen) {
    API_BEGIN
    g->g.prepare(B);                       // fusion decisions need the allocated buffers (alignment of the real views)
    std::string out = "[";
    for (auto& op : g->g.ops) {
        const std::string d = op->describe_fusion(g->g);
        if (d.empty()) continue;
        if (out.size() > 1) out += ",";
        out += d;
    }
    out += "]";
    DL4DS_REQUIRE(out.size() + 1 <= buflen, "fusion_report: buffer too small");
    std::memcpy(json_buf, out.c_str(), out.size() + 1);
    API_END
}
int dl4ds_graph_aux_launches(dl4ds_graph* g, long* n) {
    API_BEGIN
    DL4DS_REQUIRE(g && n, "graph / result pointer missing");
    *n = g->g.aux_wgrad_launches;
    API_END
}
int dl4ds_graph_bucket_plan(dl4ds_graph* g, char* buf, size_t buflen) {
    API_BEGIN
    DL4DS_REQUIRE(g && g->g.finalized, "graph not finalized");
    // launch order = the order in which the backward pass completes the buckets (largest ready_op first)
    std::vector<int> order(g->g.buckets.size());
    for (size_t i = 0; i < order.size(); ++i) order[i] = (int)i;
    std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return g->g.buckets[a].ready_op > g->g.buckets[b].ready_op; });
    std::string r = "[";
    for (size_t i = 0; i < order.size(); ++i) {
        const auto& b = g->g.buckets[order[i]];
        if (i) r += ",";
        r += "{\"bytes\":" + std::to_string(b.n * sizeof(float)) + ",\"offset\":" + std::to_string(b.off * sizeof(float)) +
             ",\"params\":" + std::to_string(b.p_hi - b.p_lo) + ",\"final_after_backward_of_op\":" + std::to_string(b.ready_op) +
             ",\"of_ops\":" + std::to_string(g->g.ops.size()) + "}";
    }
    r += "]";
    DL4DS_REQUIRE(r.size() + 1 <= buflen, "bucket plan buffer too small");
    std::memcpy(buf, r.c_str(), r.size() + 1);
    API_END
}
int dl4ds_graph_tensor_ptr(dl4ds_graph* g, int tid, int grad, float** p) {
    API_BEGIN
    const GTensor& t = g->g.tensors.at(tid);
    *p = grad ? t.grad : t.data;
    API_END
}

// ------------------------------------------------------------------------------------------------ training
int dl4ds_trainer_create(dl4ds_graph* g, int loss_kind, float lr0, float lr1, double lr_boundary, float beta1,
                         float beta2, float eps, dl4ds_trainer** tr) {
    API_BEGIN
    AdamCfg c;
    c.lr0 = lr0; c.lr1 = lr1; c.boundary = lr_boundary; c.beta1 = beta1; c.beta2 = beta2; c.eps = eps;
    dl4ds_trainer* h = new dl4ds_trainer();
    h->t = trainer_create(&g->g, loss_kind, c);
    *tr = h;
    API_END
}
int dl4ds_trainer_destroy(dl4ds_trainer* tr) {
    API_BEGIN
    if (tr) {
        HIP_CHECK(hipStreamSynchronize(S()));
        if (tr->t) delete tr->t;
        if (tr->c) cgan_destroy(tr->c);
        delete tr;
    }
    API_END
}
int dl4ds_trainer_step(dl4ds_trainer* tr, const float* const* inputs, int n_inputs, const float* y_true, int B,
                       int is_host, float* loss_host) {
    API_BEGIN
    DL4DS_REQUIRE(tr && tr->t, "not a supervised trainer");
    trainer_step(*tr->t, inputs, n_inputs, y_true, B, is_host != 0, loss_host);
    API_END
}
int dl4ds_trainer_loss_and_grads(dl4ds_trainer* tr, const float* const* inputs, int n_inputs, const float* y_true,
                                 int B, int is_host, float* loss_host) {
    API_BEGIN
    DL4DS_REQUIRE(tr && tr->t, "not a supervised trainer");
    trainer_loss_and_grads(*tr->t, inputs, n_inputs, y_true, B, is_host != 0, false);    // this rank's gradients
    if (loss_host) {
        HIP_CHECK(hipMemcpyAsync(loss_host, tr->t->d_loss, sizeof(float), hipMemcpyDeviceToHost, S()));
        HIP_CHECK(hipStreamSynchronize(S()));
    }
    API_END
}
int dl4ds_trainer_evaluate(dl4ds_trainer* tr, const float* const* inputs, int n_inputs, const float* y_true, int B,
                           int is_host, float* loss_host) {
    API_BEGIN
    DL4DS_REQUIRE(tr && tr->t, "not a supervised trainer");
    DL4DS_REQUIRE(loss_host, "evaluate: loss_host is required");
    trainer_evaluate(*tr->t, inputs, n_inputs, y_true, B, is_host != 0);
    HIP_CHECK(hipMemcpyAsync(loss_host, tr->t->d_loss, sizeof(float), hipMemcpyDeviceToHost, S()));
    dist_stream_sync(S(), "dl4ds_trainer_evaluate");
    API_END
}
int dl4ds_trainer_set_loss_weights(dl4ds_trainer* tr, const float* w, int w_batch, int H, int W, int w_channels, int is_host) {
    API_BEGIN
    DL4DS_REQUIRE(tr && tr->t, "not a supervised trainer");
    Graph& g = *tr->t->g;
    loss_weight_map_set(tr->t->lw, g.stream, w, w_batch, H, W, w_channels, is_host != 0, g.tensors[g.outputs[0]]);
    API_END
}
int dl4ds_cgan_set_loss_weights(dl4ds_trainer* tr, const float* w, int w_batch, int H, int W, int w_channels, int is_host) {
    API_BEGIN
    DL4DS_REQUIRE(tr && tr->c, "not a CGAN trainer");
    cgan_set_loss_weights(tr->c, w, w_batch, H, W, w_channels, is_host != 0);
    API_END
}
int dl4ds_trainer_get_state(dl4ds_trainer* tr, float* m_host, float* v_host, long* step) {
    API_BEGIN
    DL4DS_REQUIRE(tr && tr->t, "not a supervised trainer");
    Trainer& t = *tr->t;
    const size_t bytes = t.g->n_params * sizeof(float);
    if (m_host) HIP_CHECK(hipMemcpyAsync(m_host, t.m, bytes, hipMemcpyDeviceToHost, S()));
    if (v_host) HIP_CHECK(hipMemcpyAsync(v_host, t.v, bytes, hipMemcpyDeviceToHost, S()));
    HIP_CHECK(hipStreamSynchronize(S()));
    if (step) *step = t.step;
    API_END
}
int dl4ds_trainer_set_state(dl4ds_trainer* tr, const float* m_host, const float* v_host, long step) {
    API_BEGIN
    DL4DS_REQUIRE(tr && tr->t, "not a supervised trainer");
    DL4DS_REQUIRE(m_host && v_host && step >= 0, "set_state: missing arrays / negative step");
    Trainer& t = *tr->t;
    const size_t bytes = t.g->n_params * sizeof(float);
    HIP_CHECK(hipMemcpyAsync(t.m, m_host, bytes, hipMemcpyHostToDevice, S()));
    HIP_CHECK(hipMemcpyAsync(t.v, v_host, bytes, hipMemcpyHostToDevice, S()));
    HIP_CHECK(hipStreamSynchronize(S()));
    t.step = step;
    API_END
}
static Trainer& cgan_side(dl4ds_trainer* tr, int which) {
    DL4DS_REQUIRE(tr && tr->c, "not a CGAN trainer");
    DL4DS_REQUIRE(which == 0 || which == 1, "which: 0 generator, 1 discriminator");
    return which == 0 ? *cgan_gen_trainer(tr->c) : *cgan_disc_trainer(tr->c);
}
int dl4ds_cgan_get_state(dl4ds_trainer* tr, int which, float* m_host, float* v_host, long* step) {
    API_BEGIN
    Trainer& t = cgan_side(tr, which);
    const size_t bytes = t.g->n_params * sizeof(float);
    if (m_host) HIP_CHECK(hipMemcpyAsync(m_host, t.m, bytes, hipMemcpyDeviceToHost, S()));
    if (v_host) HIP_CHECK(hipMemcpyAsync(v_host, t.v, bytes, hipMemcpyDeviceToHost, S()));
    HIP_CHECK(hipStreamSynchronize(S()));
    if (step) *step = t.step;
    API_END
}
int dl4ds_cgan_set_state(dl4ds_trainer* tr, int which, const float* m_host, const float* v_host, long step) {
    API_BEGIN
    Trainer& t = cgan_side(tr, which);
    DL4DS_REQUIRE(m_host && v_host && step >= 0, "set_state: missing arrays / negative step");
    const size_t bytes = t.g->n_params * sizeof(float);
    HIP_CHECK(hipMemcpyAsync(t.m, m_host, bytes, hipMemcpyHostToDevice, S()));
    HIP_CHECK(hipMemcpyAsync(t.v, v_host, bytes, hipMemcpyHostToDevice, S()));
    HIP_CHECK(hipStreamSynchronize(S()));
    t.step = step;
    API_END
}
int dl4ds_trainer_set_optimizer_ext(dl4ds_trainer* tr, float global_clipnorm, float weight_decay, const int* decay_param_ids, int n_ids,
                                    float ema_momentum) {
    API_BEGIN
    DL4DS_REQUIRE(tr && tr->t, "not a supervised trainer");
    trainer_set_optimizer_ext(*tr->t, global_clipnorm, weight_decay, decay_param_ids, n_ids, ema_momentum);
    API_END
}
int dl4ds_trainer_optimizer_stats(dl4ds_trainer* tr, float* norm, float* factor, long* skipped) {
    API_BEGIN
    DL4DS_REQUIRE(tr && tr->t, "not a supervised trainer");
    trainer_optimizer_stats(*tr->t, norm, factor, skipped);
    API_END
}
int dl4ds_trainer_ema_swap(dl4ds_trainer* tr) {
    API_BEGIN
    DL4DS_REQUIRE(tr && tr->t, "not a supervised trainer");
    trainer_ema_swap(*tr->t);
    API_END
}
int dl4ds_trainer_ema_get(dl4ds_trainer* tr, float* host) {
    API_BEGIN
    DL4DS_REQUIRE(tr && tr->t, "not a supervised trainer");
    trainer_ema_get(*tr->t, host);
    API_END
}
int dl4ds_trainer_ema_set(dl4ds_trainer* tr, const float* host) {
    API_BEGIN
    DL4DS_REQUIRE(tr && tr->t, "not a supervised trainer");
    trainer_ema_set(*tr->t, host);
    API_END
}
int dl4ds_cgan_set_optimizer_ext(dl4ds_trainer* tr, int which, float global_clipnorm, float weight_decay, const int* decay_param_ids,
                                 int n_ids, float ema_momentum) {
    API_BEGIN
    Trainer& t = cgan_side(tr, which);
    DL4DS_REQUIRE(which == 0 || ema_momentum < 0.f, "the weight average belongs to the generator: pass a negative ema_momentum for the discriminator");
    trainer_set_optimizer_ext(t, global_clipnorm, weight_decay, decay_param_ids, n_ids, ema_momentum);
    API_END
}
int dl4ds_cgan_optimizer_stats(dl4ds_trainer* tr, int which, float* norm, float* factor, long* skipped) {
    API_BEGIN
    trainer_optimizer_stats(cgan_side(tr, which), norm, factor, skipped);
    API_END
}
int dl4ds_cgan_ema_swap(dl4ds_trainer* tr) {
    API_BEGIN
    trainer_ema_swap(cgan_side(tr, 0));
    API_END
}
int dl4ds_cgan_ema_get(dl4ds_trainer* tr, float* host) {
    API_BEGIN
    trainer_ema_get(cgan_side(tr, 0), host);
    API_END
}
int dl4ds_cgan_ema_set(dl4ds_trainer* tr, const float* host) {
    API_BEGIN
    trainer_ema_set(cgan_side(tr, 0), host);
    API_END
}
int dl4ds_trainer_last_loss(dl4ds_trainer* tr, float* loss_host) {
    API_BEGIN
    DL4DS_REQUIRE(tr && tr->t, "not a supervised trainer");
    HIP_CHECK(hipMemcpyAsync(loss_host, tr->t->d_loss, sizeof(float), hipMemcpyDeviceToHost, S()));
    dist_stream_sync(S(), "dl4ds_trainer_last_loss");
    API_END
}

int dl4ds_cgan_create(dl4ds_graph* gen, dl4ds_graph* disc, int px_loss_kind, float lr, float beta1, float lam,
                      dl4ds_trainer** tr) {
    API_BEGIN
    dl4ds_trainer* h = new dl4ds_trainer();
    h->c = cgan_create(&gen->g, &disc->g, px_loss_kind, lr, beta1, lam);
    *tr = h;
    API_END
}
int dl4ds_cgan_set_learning_rates(dl4ds_trainer* tr, float gen_lr, float disc_lr) {
    API_BEGIN
    DL4DS_REQUIRE(tr && tr->c, "not a CGAN trainer");
    DL4DS_REQUIRE(gen_lr > 0.f && disc_lr > 0.f, "learning rates must be positive");
    cgan_set_learning_rates(tr->c, gen_lr, disc_lr);
    API_END
}
int dl4ds_cgan_step(dl4ds_trainer* tr, const float* const* gen_inputs, int n_gen_inputs, const float* hr, int B,
                    int is_host, const float* dropout_keep_host, int apply_update, float* losses_host) {
    API_BEGIN
    DL4DS_REQUIRE(tr && tr->c, "not a CGAN trainer");
    cgan_step(*tr->c, gen_inputs, n_gen_inputs, hr, B, is_host != 0, dropout_keep_host, apply_update != 0, losses_host);
    API_END
}
int dl4ds_cgan_get_disc_grad(dl4ds_trainer* tr, int pid, float* dst) {
    API_BEGIN
    DL4DS_REQUIRE(tr && tr->c, "not a CGAN trainer");
    Graph* g = cgan_disc_trainer(tr->c)->g;
    const GParam& p = g->params.at(pid);
    HIP_CHECK(hipMemcpyAsync(dst, g->G + p.offset, p.n * sizeof(float), hipMemcpyDeviceToHost, S()));
    HIP_CHECK(hipStreamSynchronize(S()));
    API_END
}

// ------------------------------------------------------------------------------------------------ dist
int dl4ds_dist_unique_id(char id128[128]) {
    API_BEGIN
    dist_unique_id(id128);
    API_END
}
int dl4ds_dist_init(int rank, int world, const char id128[128]) {
    API_BEGIN
    dist_init(rank, world, id128);
    API_END
}
int dl4ds_dist_world(int* rank, int* world) {
    API_BEGIN
    dist_world(*rank, *world);
    API_END
}
int dl4ds_dist_broadcast_trainer(dl4ds_trainer* tr, int root) {
    API_BEGIN
    DL4DS_REQUIRE(tr, "broadcast_trainer: null trainer");
    dist_require_ready("dl4ds_dist_broadcast_trainer");
    std::vector<Trainer*> ts;
    if (tr->t) ts.push_back(tr->t);
    if (tr->c) { ts.push_back(cgan_gen_trainer(tr->c)); ts.push_back(cgan_disc_trainer(tr->c)); }
    for (Trainer* t : ts) {
        dist_broadcast(t->g->W, t->g->n_params, root, S());
        dist_broadcast(t->m, t->g->n_params, root, S());
        dist_broadcast(t->v, t->g->n_params, root, S());
        if (t->ext.ema_on) dist_broadcast(t->ext.ema, t->g->n_params, root, S());
    }
    HIP_CHECK(hipStreamSynchronize(S()));
    for (Trainer* t : ts) dist_broadcast_i64(&t->step, root);     // optimizer.iterations (a resumed rank 0)
    API_END
}
int dl4ds_dist_expected_world(int* world) {
    API_BEGIN
    *world = dist_expected_world();
    API_END
}
int dl4ds_dist_comm_info(int* nranks, int* rank, int* device) {
    API_BEGIN
    dist_comm_info(*nranks, *rank, *device);
    API_END
}
int dl4ds_dist_allreduce_host(float* values_host, int n, int op) {
    API_BEGIN
    rt_ensure_init();
    dist_allreduce_host(values_host, n, op);
    API_END
}
int dl4ds_dist_barrier(void) {
    API_BEGIN
    rt_ensure_init();
    dist_barrier();
    API_END
}
int dl4ds_dist_allreduce_sum(float* buf, size_t n) {
    API_BEGIN
    dist_allreduce_grads(buf, n, S());
    API_END
}
int dl4ds_dist_finalize(void) {
    API_BEGIN
    dist_finalize();
    API_END
}

}  // extern "C"
