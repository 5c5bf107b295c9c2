// Per-step training arithmetic: forward -> loss(+grad) -> backward -> [RCCL gradient all-reduce] -> Keras Adam.
// Replaces the Keras `fit` inner step configured by SupervisedTrainer.run (dl4ds/training/supervised.py:336-353,
// 396-406) and train_step of the CGAN trainer (dl4ds/training/cgan.py:575-639).
#include "graph.h"
#include "runtime.h"
#include "dist.h"
#include <cmath>
#include <cstring>
#include <vector>

Trainer::~Trainer() {
    if (m) (void)hipFree(m);
    if (v) (void)hipFree(v);
    if (d_loss) (void)hipFree(d_loss);
    if (loss_ws) (void)hipFree(loss_ws);
    if (y_true) (void)hipFree(y_true);
}

OptExt::~OptExt() {
    if (ema) (void)hipFree(ema);
    if (bounds) (void)hipFree(bounds);
    if (partials) (void)hipFree(partials);
    if (stats) (void)hipFree(stats);
}

LossWeightMap::~LossWeightMap() {
    if (w) (void)hipFree(w);
}

void loss_weight_map_set(LossWeightMap& m, hipStream_t s, const float* w, int w_batch, int H, int W, int ch, bool is_host,
                         const GTensor& out) {
    if (!w) { m.set = false; return; }
    DL4DS_REQUIRE(w_batch >= 1, "loss weights: w_batch must be 1 (one shared map) or the batch size of the steps to come");
    DL4DS_REQUIRE(H == out.H && W == out.W, "loss weights: H, W must be those of output 0");
    DL4DS_REQUIRE(ch == 1 || ch == out.C, "loss weights: w_channels must be 1 or the channels of output 0");
    const size_t n = (size_t)w_batch * H * W * ch;
    if (n > m.cap) {
        HIP_CHECK(hipStreamSynchronize(s));
        if (m.w) HIP_CHECK(hipFree(m.w));
        m.w = nullptr; m.cap = 0; m.set = false;
        HIP_CHECK(hipMalloc((void**)&m.w, n * sizeof(float)));
        m.cap = n;
    }
    HIP_CHECK(hipMemcpyAsync(m.w, w, n * sizeof(float), is_host ? hipMemcpyHostToDevice : hipMemcpyDeviceToDevice, s));
    m.batch = w_batch; m.H = H; m.W = W; m.ch = ch; m.set = true;
}

// the trainer's loss on output 0: the weighted kernels while a weight map is in force, else exactly the unweighted call
static void trainer_loss(Trainer& t, const float* yt, int B) {
    Graph& g = *t.g;
    const GTensor& o = g.tensors[g.outputs[0]];
    if (!t.lw.set) {
        loss_forward_backward(g.stream, t.loss_kind, yt, o.data, o.grad, B * o.nmul, o.H, o.W, o.C, 1.f, t.d_loss, 0,
                              t.loss_ws, t.loss_ws_bytes);
        return;
    }
    loss_forward_backward_weighted(g.stream, t.loss_kind, yt, o.data, o.grad, B * o.nmul, o.H, o.W, o.C, 1.f, t.d_loss, 0,
                                   t.lw.w, t.lw.batch, t.lw.ch, t.loss_ws, t.loss_ws_bytes);
}

Trainer* trainer_create(Graph* g, int loss_kind, const AdamCfg& cfg) {
    DL4DS_REQUIRE(g->finalized, "trainer: graph not finalized");
    DL4DS_REQUIRE(g->outputs.size() >= 1, "trainer: graph has no output");
    Trainer* t = new Trainer();
    t->g = g;
    t->cfg = cfg;
    t->loss_kind = loss_kind;
    const size_t bytes = std::max<size_t>(g->n_params, 4) * sizeof(float);
    HIP_CHECK(hipMalloc((void**)&t->m, bytes));
    HIP_CHECK(hipMalloc((void**)&t->v, bytes));
    HIP_CHECK(hipMemset(t->m, 0, bytes));
    HIP_CHECK(hipMemset(t->v, 0, bytes));
    HIP_CHECK(hipMalloc((void**)&t->d_loss, 8 * sizeof(float)));
    HIP_CHECK(hipMemset(t->d_loss, 0, 8 * sizeof(float)));
    return t;
}

void graph_load_inputs(Graph& g, const float* const* inputs, int n_inputs, int B, bool is_host) {
    DL4DS_REQUIRE(n_inputs == (int)g.inputs.size(), "wrong number of model inputs");
    g.prepare(B);
    for (int i = 0; i < n_inputs; ++i) {
        GTensor& t = g.tensors[g.inputs[i]];
        const size_t bytes = t.per_sample() * B * sizeof(float);
        if (inputs[i] == t.data) continue;       // already in place
        HIP_CHECK(hipMemcpyAsync(t.data, inputs[i], bytes, is_host ? hipMemcpyHostToDevice : hipMemcpyDeviceToDevice,
                                 g.stream));
    }
}

static void ensure_loss_buffers(Trainer& t, int B) {
    Graph& g = *t.g;
    const GTensor& o = g.tensors[g.outputs[0]];
    const size_t need = o.per_sample() * B;
    if (need > t.y_true_floats) {
        HIP_CHECK(hipStreamSynchronize(g.stream));
        if (t.y_true) HIP_CHECK(hipFree(t.y_true));
        HIP_CHECK(hipMalloc((void**)&t.y_true, need * sizeof(float)));
        t.y_true_floats = need;
    }
    if (t.lw.set)
        DL4DS_REQUIRE(t.lw.batch == 1 || t.lw.batch == B, "per-sample loss weights were set for another batch size than this step's");
    const size_t ws = t.lw.set ? loss_workspace_bytes_weighted(t.loss_kind, B * o.nmul, o.H, o.W, o.C, t.lw.batch, t.lw.ch)
                               : loss_workspace_bytes(t.loss_kind, B * o.nmul, o.H, o.W, o.C);
    if (ws > t.loss_ws_bytes) {
        HIP_CHECK(hipStreamSynchronize(g.stream));
        if (t.loss_ws) HIP_CHECK(hipFree(t.loss_ws));
        HIP_CHECK(hipMalloc((void**)&t.loss_ws, ws));
        t.loss_ws_bytes = ws;
    }
}

// forward + loss + backward; gradients land in g->G (un-averaged, this rank only)
void trainer_loss_and_grads(Trainer& t, const float* const* inputs, int n_inputs, const float* y_true, int B,
                            bool is_host, bool reduce_across_ranks) {
    Graph& g = *t.g;
    graph_load_inputs(g, inputs, n_inputs, B, is_host);
    ensure_loss_buffers(t, B);
    const GTensor& o = g.tensors[g.outputs[0]];
    const float* yt = y_true;
    if (is_host) {
        HIP_CHECK(hipMemcpyAsync(t.y_true, y_true, o.per_sample() * B * sizeof(float), hipMemcpyHostToDevice, g.stream));
        yt = t.y_true;
    }
    g.forward(B, true);
    g.zero_grad_flags();
    trainer_loss(t, yt, B);
    // (inputs created with dl4ds_graph_input_requires_grad get their gradient too: dl4ds_graph_tensor_ptr(id, grad = 1))
    bool input_grads = false;
    for (int i : g.inputs) input_grads = input_grads || g.tensors[i].requires_grad;
    BwdCtx c{B, 0, B, true, input_grads};
    // data parallel: buckets of the gradient arena are all-reduced on the communication stream as the backward pass
    // finishes them; trainer_step waits for the last one before Adam
    if (reduce_across_ranks && dist_active()) {
        g.grad_ready = [](void*, float* grads, size_t n, hipStream_t st, hipStream_t aux) {
            dist_allreduce_bucket_async(grads, n, st, aux);
        };
    } else {
        g.grad_ready = nullptr;
    }
    g.backward(c);
}

// model.evaluate: inference-mode forward (dropout off unless MC, BatchNormalization on its moving statistics, which are
// left untouched) + the loss value; no backward pass
void trainer_evaluate(Trainer& t, const float* const* inputs, int n_inputs, const float* y_true, int B, bool is_host) {
    Graph& g = *t.g;
    graph_load_inputs(g, inputs, n_inputs, B, is_host);
    ensure_loss_buffers(t, B);
    const GTensor& o = g.tensors[g.outputs[0]];
    const float* yt = y_true;
    if (is_host) {
        HIP_CHECK(hipMemcpyAsync(t.y_true, y_true, o.per_sample() * B * sizeof(float), hipMemcpyHostToDevice, g.stream));
        yt = t.y_true;
    }
    g.forward(B, false);
    // the fused loss kernels always emit dL/dpred; it lands in the output's gradient buffer and is never read
    trainer_loss(t, yt, B);
}

static float current_lr(const Trainer& t) {
    // PiecewiseConstantDecay: lr0 while iterations <= boundary, else lr1 (supervised.py:340-346)
    return ((double)t.step <= t.cfg.boundary) ? t.cfg.lr0 : t.cfg.lr1;
}

// The sticky device error word (runtime.h) ENDS the process's training: the optimiser kernel leaves parameters and moments untouched
// once it is set, every later host-side wait throws, and nothing clears it -- a caller that catches the exception and goes on would
// only advance the step counter here (and, in a multi-rank job, diverge from ranks that did not raise).  SupervisedEngine / CGANEngine
// do not catch it; the C header says the same (dl4ds_last_error: "device error word set").
void trainer_apply_adam(Trainer& t) {
    Graph& g = *t.g;
    const float lr = current_lr(t);
    t.step += 1;
    const double tt = (double)t.step;
    const float lr_t = (float)((double)lr * std::sqrt(1.0 - std::pow((double)t.cfg.beta2, tt)) /
                               (1.0 - std::pow((double)t.cfg.beta1, tt)));
    int rank = 0, world = 1;
    dist_world(rank, world);
    if (!t.ext.any()) {
        adam_update(g.stream, g.W, g.G, t.m, t.v, g.n_params, lr_t, t.cfg.beta1, t.cfg.beta2, t.cfg.eps,
                    1.f / (float)world, device_error_word_if_any());
        return;
    }
    // clipping / weight decay / weight average (adam_ext.hip).  Data parallel: this runs behind dist_allreduce_wait, so the norm is
    // that of the SUMMED arena, the same bits on every rank, and 1/world reaches it through grad_scale.  t.step above counts
    // ATTEMPTED steps: a step the kernel skips for a non-finite norm still advances the schedule and the bias correction.
    OptExt& x = t.ext;
    adam_ext_update(g.stream, g.W, g.G, t.m, t.v, x.ema_on ? x.ema : nullptr, g.n_params, lr_t, t.cfg.beta1, t.cfg.beta2, t.cfg.eps,
                    1.f / (float)world, x.clipnorm, lr, x.weight_decay, x.bounds, x.n_bounds, x.ema_momentum, x.partials, x.stats,
                    device_error_word_if_any());
}

// dl4ds_trainer_set_optimizer_ext / dl4ds_cgan_set_optimizer_ext: between steps, any number of times.  ema_momentum < 0: no average.
void trainer_set_optimizer_ext(Trainer& t, float clipnorm, float weight_decay, const int* decay_param_ids, int n_ids,
                               float ema_momentum) {
    Graph& g = *t.g;
    OptExt& x = t.ext;
    DL4DS_REQUIRE(clipnorm >= 0.f && std::isfinite(clipnorm), "global_clipnorm must be finite and > 0 (0: off)");
    DL4DS_REQUIRE(weight_decay >= 0.f && std::isfinite(weight_decay), "weight_decay must be finite and >= 0");
    DL4DS_REQUIRE(ema_momentum < 1.f, "ema_momentum must be in [0, 1) (negative: no average)");
    DL4DS_REQUIRE(n_ids >= 0 && (n_ids == 0 || decay_param_ids), "decay_param_ids missing");
    std::vector<size_t> ranges;
    for (int k = 0; k < n_ids; ++k) {
        const GParam& p = g.params.at(decay_param_ids[k]);
        ranges.push_back(p.offset);
        ranges.push_back(p.offset + p.n);
    }
    const std::vector<size_t> b = decay_bounds(ranges.data(), n_ids, g.n_params);
    HIP_CHECK(hipStreamSynchronize(g.stream));               // a step in flight still reads the old table / average
    if (x.bounds) { HIP_CHECK(hipFree(x.bounds)); x.bounds = nullptr; }
    x.n_bounds = 0;
    if (!b.empty()) {
        HIP_CHECK(hipMalloc((void**)&x.bounds, b.size() * sizeof(size_t)));
        HIP_CHECK(hipMemcpy(x.bounds, b.data(), b.size() * sizeof(size_t), hipMemcpyHostToDevice));
        x.n_bounds = (int)b.size();
    }
    if (!x.partials) HIP_CHECK(hipMalloc((void**)&x.partials, (size_t)sqnorm_blocks(g.n_params) * sizeof(double)));
    if (!x.stats) {
        const float init[4] = {0.f, 1.f, 0.f, 0.f};          // norm, factor, skipped (the integer 0), spare
        HIP_CHECK(hipMalloc((void**)&x.stats, sizeof(init)));
        HIP_CHECK(hipMemcpy(x.stats, init, sizeof(init), hipMemcpyHostToDevice));
    }
    x.clipnorm = clipnorm;
    x.weight_decay = weight_decay;
    const bool want_ema = ema_momentum >= 0.f;
    const size_t bytes = std::max<size_t>(g.n_params, 4) * sizeof(float);
    if (want_ema && !x.ema_on) {
        // the Keras optimiser's `average` slots start as copies of the variables
        HIP_CHECK(hipMalloc((void**)&x.ema, bytes));
        HIP_CHECK(hipMemcpy(x.ema, g.W, bytes, hipMemcpyDeviceToDevice));
    } else if (!want_ema && x.ema_on) {
        HIP_CHECK(hipFree(x.ema));
        x.ema = nullptr;
    }
    x.ema_on = want_ema;
    x.ema_momentum = want_ema ? ema_momentum : 0.f;
}

void trainer_optimizer_stats(Trainer& t, float* norm, float* factor, long* skipped) {
    float h[3] = {0.f, 1.f, 0.f};
    if (t.ext.stats) {
        HIP_CHECK(hipMemcpyAsync(h, t.ext.stats, sizeof(h), hipMemcpyDeviceToHost, t.g->stream));
        dist_stream_sync(t.g->stream, "optimizer_stats");
    }
    unsigned k = 0;
    std::memcpy(&k, &h[2], sizeof(k));
    if (norm) *norm = h[0];
    if (factor) *factor = h[1];
    if (skipped) *skipped = (long)k;
}

void trainer_ema_swap(Trainer& t) {
    DL4DS_REQUIRE(t.ext.ema_on, "the weight average is off (set ema_momentum first)");
    arena_swap(t.g->stream, t.g->W, t.ext.ema, t.g->n_params);
}
void trainer_ema_get(Trainer& t, float* host) {
    DL4DS_REQUIRE(t.ext.ema_on && host, "the weight average is off (set ema_momentum first)");
    HIP_CHECK(hipMemcpyAsync(host, t.ext.ema, t.g->n_params * sizeof(float), hipMemcpyDeviceToHost, t.g->stream));
    HIP_CHECK(hipStreamSynchronize(t.g->stream));
}
void trainer_ema_set(Trainer& t, const float* host) {
    DL4DS_REQUIRE(t.ext.ema_on && host, "the weight average is off (set ema_momentum first)");
    HIP_CHECK(hipMemcpyAsync(t.ext.ema, host, t.g->n_params * sizeof(float), hipMemcpyHostToDevice, t.g->stream));
    HIP_CHECK(hipStreamSynchronize(t.g->stream));
}

void trainer_step(Trainer& t, const float* const* inputs, int n_inputs, const float* y_true, int B, bool is_host,
                  float* loss_host) {
    Graph& g = *t.g;
    dist_require_ready("dl4ds_trainer_step");               // WORLD_SIZE > 1 without a communicator is an error, not a no-op
    trainer_loss_and_grads(t, inputs, n_inputs, y_true, B, is_host, true);
    dist_allreduce_wait(g.stream);                          // buckets were launched during the backward pass
    trainer_apply_adam(t);
    if (loss_host) {
        HIP_CHECK(hipMemcpyAsync(loss_host, t.d_loss, sizeof(float), hipMemcpyDeviceToHost, g.stream));
        dist_stream_sync(g.stream, "dl4ds_trainer_step (loss read-back)");
    }
}
