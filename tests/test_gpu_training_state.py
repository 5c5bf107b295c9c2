"""State that lives BETWEEN optimiser steps (csrc/trainer.hip, csrc/graph.hip, training/engine.py) on MI355X, against references
that do not share it.

1. Every single update of a 6-step run across the learning-rate boundary is one Keras-Adam step in float64
   (tests/training_state_ref.py) from the device's own state before it and the gradient the device reported for that batch:
   schedule (updates 0, 1, 2 at lr0, then lr1), bias correction from the right t, moments carried.  Nothing accumulates.  The same
   for both optimisers of the CGAN engine (own rates, beta_1 = 0.5; gradients from step(apply_update=False), which leaves them
   readable) and for an engine with global_clipnorm, weight_decay and ema_momentum (tests/optimizer_ref.py fixes lr at 1e-3 and
   cannot cross the boundary, so the float64 restatement of the three extensions is the one in training_state_ref).
2. Batch sizes 4, 1, 3, 4, 2 on one engine give, at every step, the bytes a fresh model + engine gives that was loaded with the
   state before that step and ran that step only.
3. evaluate() between steps changes nothing a step depends on, and equals the oracle's inference-mode forward + loss.
4. DL4DS_AUX_STREAM=1 (weight gradients on a second stream) gives the bytes of the single-stream order with the same kernel
   selection, matches the fp64 oracle, and provably used the second stream (dl4ds_graph_aux_launches).

Measured on MI355X (worst over all tensors and steps; m / v in ulp of the larger term, bound 4; w as |dw - dw_ref| / lr, bound
2e-3 + 2^-23 |w| / lr):
    resnet_spc (net_postupsampling)      m 1.49 ulp   v 2.23 ulp   w 2.9e-4 lr
    pin_bn_dropout (net_pin)             m 1.46 ulp   v 1.89 ulp   w 5.9e-4 lr
    recnet_tw2 (recnet_postupsampling)   m 1.48 ulp   v 1.99 ulp   w 2.6e-4 lr
    CGAN generator / discriminator       m 1.00 / 1.00 ulp   v 2.09 / 1.87 ulp   w 2.5e-4 / 1.5e-4 lr
    clipping + decay + average           m 2.10 ulp   v 2.91 ulp   w 5.5e-4 lr
(the worst w figures come from the updates at lr = 1e-4, where the rounding of the subtraction at the size of w weighs ten times more.)
Oracle fall-backs in parts 2 and 4: none -- every tensor of every model is identical bytes.
Wall time of the module: 3.8 s for its 15 tests (each under 0.3 s)."""
import numpy as np
import pytest

from oracle import np_ops as N
from oracle import models as M
from tests import training_state_ref as R
from tests.parity import assert_matches_reference, first_quiet, oracle_reference, targets_clear_of_the_kink
from tests.test_gpu_models import _cgan_banded, build_pair, tie_free_inputs

pytestmark = pytest.mark.gpu

LR0, LR1, BOUNDARY = 1e-3, 1e-4, 2
STATS = ('moving_mean', 'moving_variance')

# kind, builder arguments, normalization / dropout arguments, per-sample input shape, per-sample auxiliary shape
PLAIN = ('net_postupsampling', dict(backbone_block='resnet', upsampling='spc', scale=2, n_blocks=2, n_filters=8), {}, (8, 8, 1), None)
BN_DROP = ('net_pin', dict(backbone_block='convnet', n_blocks=1, n_filters=6), dict(normalization='bn', dropout_rate=0.2),
           (12, 12, 2), None)
REC = ('recnet_postupsampling', dict(backbone_block='resnet', upsampling='spc', scale=2, time_window=2, n_filters=4, n_blocks=1), {},
       (2, 8, 6, 2), None)
MODELS = [PLAIN, BN_DROP, REC]
IDS = ['resnet_spc', 'pin_bn_dropout', 'recnet_tw2']


def make(case, B=4):
    """-> (model, oracle params, oracle cfg); the graph is prepared for B and its dropout ops know their mask sizes."""
    kind, cfg, var, xs, ss = case
    model, P, ocfg = build_pair(kind, cfg, (B,) + xs, None if ss is None else (B,) + ss, ctx_kw=var or None)
    if model.graph.dropout_count():
        w = model.get_weights()
        model([np.zeros((B,) + xs, np.float32)], training=True)          # (mask sizes are known once a batch of B has run)
        model.set_weights(w)                                             # (that pass moved the BatchNormalization averages)
    return model, P, ocfg


def sample_pool(case, model, n, seed):
    """n seeded samples: inputs (list of arrays) and targets."""
    kind, cfg, var, xs, ss = case
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((n,) + xs).astype(np.float32)
    y = rng.standard_normal((n,) + tuple(model.output_shape)).astype(np.float32)
    return x, y


def inject(model, B, seed, rate=0.2):
    """A seeded keep mask for every dropout op, used by the next training-mode forward of a batch of B."""
    g = model.graph
    rng = np.random.default_rng(seed)
    for i in range(g.dropout_count()):
        n = g.dropout_mask(i, B).size
        g.set_dropout_mask(i, B, (rng.random(n) >= rate).astype(np.float32))


def same_bytes(a, b, what):
    assert set(a) == set(b), what
    for k in a:
        assert np.array_equal(a[k], b[k]), (what, k, float(np.abs(a[k].astype(np.float64) - b[k]).max()))


def state(model, eng):
    m, v, step = eng.optimizer_state()
    return model.get_weights(), m, v, step


class Worst:
    def __init__(self):
        self.m = self.v = self.w = 0.0

    def take(self, c):
        self.m, self.v, self.w = max(self.m, c['m_ulps']), max(self.v, c['v_ulps']), max(self.w, c['w_over_lr'])

    def __str__(self):
        return f'm {self.m:.2f} ulp, v {self.v:.2f} ulp, w {self.w:.2e} lr'


def check_update(before, grads, after, it, lr, worst, what, beta_1=0.9, factor=1.0, decay=None, wd=0.0):
    """Every trainable tensor of one device update against R.adam_step; -> the rate the update used, read off its own result."""
    w0, m0, v0, s0 = before
    w1, m1, v1, s1 = after
    assert s0 == it and s1 == it + 1, (what, s0, s1)
    bw, am, av, aw = [], [], [], []
    for k in w0:
        if k.endswith(STATS):                       # never trained: no gradient, no moments
            assert not grads[k].any() and not m1[k].any() and not v1[k].any(), (what, k)
            continue
        c = R.check_step((w0[k], m0[k], v0[k]), grads[k], (w1[k], m1[k], v1[k]), it, lr, beta_1=beta_1, grad_factor=factor,
                         decay=wd if (decay and k in decay) else 0.0)
        worst.take(c)
        for name in ('m', 'v', 'w'):
            bad = c[name + '_bad']
            assert not bad.any(), (what, k, 'step', it, name, int(bad.sum()), bad.size, c['m_ulps'], c['v_ulps'], c['w_over_lr'])
        if not (decay and k in decay):
            bw.append(w0[k].ravel()); aw.append(w1[k].ravel()); am.append(m1[k].ravel()); av.append(v1[k].ravel())
    return R.implied_lr(np.concatenate(bw), (np.concatenate(aw), np.concatenate(am), np.concatenate(av)), it, beta_1=beta_1)


# ================================================================================================ 1. step-local Adam and schedule
@pytest.mark.parametrize('case', MODELS, ids=IDS)
def test_every_update_is_one_keras_adam_step_under_the_schedule(case):
    from dl4ds_amd.training import SupervisedEngine
    model, _, _ = make(case)
    eng = SupervisedEngine(model, loss='mse', learning_rate=(LR0, LR1), lr_decay_after=BOUNDARY)
    worst, rates = Worst(), []
    for it in range(6):
        x, y = sample_pool(case, model, 4, 100 + it)                   # a different batch per step: g_t differs
        before = state(model, eng)
        inject(model, 4, 7 * it)
        l1, g1 = eng.loss_and_grads([x], y)
        inject(model, 4, 7 * it)
        l2, g2 = eng.loss_and_grads([x], y)
        assert l1 == l2                                                  # precondition: the gradient of this batch is reproducible
        same_bytes(g1, g2, 'two loss_and_grads calls')
        stats = {k: v for k, v in model.get_weights().items() if k.endswith(STATS)}
        before[0].update(stats)                                          # (training-mode passes move the BN averages, Adam does not)
        inject(model, 4, 7 * it)
        assert eng.step([x], y) == l1
        after = state(model, eng)
        lr = R.scheduled_lr(it, LR0, LR1, BOUNDARY)
        rates.append(check_update(before, g1, after, it, lr, worst, case[0]))
    print('training-state figures', case[0], case[2], worst)
    for it, r in enumerate(rates):                                       # updates 0, 1, 2 at 1e-3; 3, 4, 5 at 1e-4
        assert abs(r / (LR0 if it <= 2 else LR1) - 1) < 1e-3, (it, rates)


def test_cgan_optimisers_each_take_keras_adam_steps_at_their_own_rate():
    """Generator at 2e-4, discriminator at 1e-4, beta_1 = 0.5, three steps on different batches.  The gradients come from
    step(apply_update=False) on the same batch and dropout mask, which leaves both gradient arenas readable (two such calls give
    identical bytes), so w, m and v are all checked per step, not only the moments' recursion."""
    import dl4ds_amd.models as PM
    from dl4ds_amd.training import CGANEngine
    B, h, w, nf = 2, 8, 7, 4
    gen = PM.net_postupsampling(n_channels=2, n_aux_channels=1, lr_size=(h, w), seed=3, backbone_block='resnet', upsampling='spc',
                                scale=2, n_blocks=1, n_filters=nf)
    disc = PM.residual_discriminator(2, 'spc', False, 2, (h, w), hr_size=(2 * h, 2 * w), time_window=None, seed=4, n_filters=nf,
                                     n_res_blocks=1)
    eng = CGANEngine(gen, disc, loss='mae', learning_rate=(2e-4, 1e-4), beta_1=0.5)
    worst = {'generator': Worst(), 'discriminator': Worst()}
    for it in range(3):
        r = np.random.default_rng(40 + it)
        lr = r.random((B, h, w, 2)).astype(np.float32)
        st = r.random((B, 2 * h, 2 * w, 1)).astype(np.float32)
        hr = r.random((B, 2 * h, 2 * w, 1)).astype(np.float32)
        mask = (r.random((2 * B, 2 * nf)) > 0.4).astype(np.float32)
        before = {wh: (mdl.get_weights(),) + eng.optimizer_state(wh) for wh, mdl in (('generator', gen), ('discriminator', disc))}
        o1 = eng.step([lr, st], hr, dropout_keep=mask, apply_update=False)
        grads = {'generator': gen.get_gradients(), 'discriminator': disc.get_gradients()}
        o2 = eng.step([lr, st], hr, dropout_keep=mask, apply_update=False)
        assert o1 == o2
        same_bytes(grads['generator'], gen.get_gradients(), 'generator gradients, two calls')
        same_bytes(grads['discriminator'], disc.get_gradients(), 'discriminator gradients, two calls')
        same_bytes(before['generator'][0], gen.get_weights(), 'apply_update=False moved the generator')
        assert eng.optimizer_state('generator')[2] == it and eng.optimizer_state('discriminator')[2] == it
        assert eng.step([lr, st], hr, dropout_keep=mask) == o1
        for wh, mdl, rate in (('generator', gen, 2e-4), ('discriminator', disc, 1e-4)):
            after = (mdl.get_weights(),) + eng.optimizer_state(wh)
            used = check_update(before[wh], grads[wh], after, it, rate, worst[wh], wh, beta_1=0.5)
            assert abs(used / rate - 1) < 1e-3, (wh, it, used)
    print('training-state figures cgan', {k: str(v) for k, v in worst.items()})


def test_clipping_decay_and_average_across_the_boundary():
    """global_clipnorm + weight_decay + ema_momentum over 4 steps across the boundary: the clipping factor the device reports is
    clip / max(||g||, clip) of its own gradients (three float32 roundings: 2^-22) and below 1 at least once, the decay uses the
    PLAIN scheduled lr (at t = 1 lr_t is 3.2 x lr: the w bound tells them apart on every decayed entry of size > 0.02), and the
    average follows ema_momentum from the weights the device returned."""
    from dl4ds_amd.training import SupervisedEngine
    case = PLAIN
    wd, mu = 0.1, 0.9
    model, _, _ = make(case)
    eng = SupervisedEngine(model, loss='mse', learning_rate=(LR0, LR1), lr_decay_after=BOUNDARY)
    x, y = sample_pool(case, model, 4, 100)
    _, g = eng.loss_and_grads([x], y)
    clip = 0.5 * R.clip_factor(g, 1.0)[1]                                # half the first batch's norm: that step is clipped
    eng.set_optimizer_ext(global_clipnorm=clip, weight_decay=wd, ema_momentum=mu)
    assert eng.decayed and len(eng.decayed) < len(g)
    worst, clipped = Worst(), 0
    for it in range(4):
        x, y = sample_pool(case, model, 4, 100 + it)
        before, ema0 = state(model, eng), eng.ema_state()
        _, g = eng.loss_and_grads([x], y)
        eng.step([x], y)
        after, ema1, st = state(model, eng), eng.ema_state(), eng.optimizer_stats()
        c64, norm = R.clip_factor(g, clip)
        assert st['skipped_steps'] == 0
        assert abs(st['grad_norm'] / norm - 1) <= 2.0 ** -22 and abs(st['clip_factor'] / c64 - 1) <= 2.0 ** -22, (it, st, norm, c64)
        clipped += st['clip_factor'] < 1
        lr = R.scheduled_lr(it, LR0, LR1, BOUNDARY)
        check_update(before, g, after, it, lr, worst, 'extended step', factor=st['clip_factor'], decay=set(eng.decayed), wd=wd)
        for k in ema0:
            ref, bound = R.ema_step(ema0[k], after[0][k], mu)
            assert (np.abs(ema1[k] - ref) <= bound).all(), (k, it)
    assert clipped >= 1
    print('training-state figures extended', worst)


# ================================================================================================ 2. batch-size sequence
@pytest.mark.parametrize('case', MODELS, ids=IDS)
def test_batch_size_sequence_equals_fresh_engines_step_by_step(case, tmp_path):
    """B = 4, 1, 3, 4, 2 from a fixed pool on ONE engine (grow-only buffers, saved activations, partial-tile scratch and gradient
    flags of the larger batches behind it) against a fresh model + engine per step that was loaded with the state before that step
    (weights with the BatchNormalization averages, m, v, iterations): loss, weights, moments, averages identical bytes."""
    from dl4ds_amd.training import SupervisedEngine
    sizes, starts = [4, 1, 3, 4, 2], [0, 4, 2, 1, 3]
    a, _, _ = make(case)
    x, y = sample_pool(case, a, 6, 55)
    ea = SupervisedEngine(a, loss='mae', learning_rate=(LR0, LR1), lr_decay_after=BOUNDARY)
    for k, (B, s0) in enumerate(zip(sizes, starts)):
        xb, yb = x[s0:s0 + B], y[s0:s0 + B]
        path = str(tmp_path / f'before{k}.npz')
        ea.save_checkpoint(path)
        inject(a, B, 300 + k)
        la = ea.step([xb], yb)
        b, _, _ = make(case, B)
        eb = SupervisedEngine(b, loss='mae', learning_rate=(LR0, LR1), lr_decay_after=BOUNDARY)
        assert eb.load_checkpoint(path) == k
        inject(b, B, 300 + k)
        lb = eb.step([xb], yb)
        assert la == lb, (k, B, la, lb)
        sa, sb = state(a, ea), state(b, eb)
        assert sa[3] == sb[3] == k + 1
        for name, da, db in zip(('weights', 'm', 'v'), sa[:3], sb[:3]):
            same_bytes(da, db, (name, 'step', k, 'B', B))


# ================================================================================================ 3. evaluate between steps
@pytest.mark.parametrize('case', MODELS, ids=IDS)
def test_evaluate_between_steps_changes_nothing_and_equals_the_oracle(case):
    """Run A evaluates after every step on other batches of other sizes (5: larger than any training batch, so the buffers are laid
    out again; 2; 1), run B never: losses, weights, moments and BatchNormalization averages identical bytes -- the dL/dpred the
    loss kernel leaves in the output's gradient buffer is never read, the averages and the dropout state are left alone.  Each
    evaluate equals the oracle's inference-mode forward (moving statistics, no dropout mask) + MAE to 1e-4."""
    from dl4ds_amd.training import SupervisedEngine
    kind, cfg, var, xs, ss = case
    a, _, ocfg = make(case)
    b, _, _ = make(case)
    ea = SupervisedEngine(a, loss='mae', learning_rate=(LR0, LR1), lr_decay_after=BOUNDARY)
    eb = SupervisedEngine(b, loss='mae', learning_rate=(LR0, LR1), lr_decay_after=BOUNDARY)
    xe, ye = sample_pool(case, a, 5, 77)
    moved = False
    for it, Be in enumerate([5, 2, 1, 5]):
        x, y = sample_pool(case, a, 3, 200 + it)
        inject(a, 3, 11 * it); inject(b, 3, 11 * it)
        assert ea.step([x], y) == eb.step([x], y), it
        w = a.get_weights()
        got = ea.evaluate([xe[:Be]], ye[:Be])
        P = M.Params()
        for k, v in w.items():
            P[k] = v.astype(np.float64)
        ref = M.MODELS[kind](N, P, xe[:Be].astype(np.float64), None, ctx=M.Ctx(training=False, **var), **ocfg)
        assert got == pytest.approx(float(np.abs(ref - ye[:Be]).mean()), rel=1e-4), (it, Be)
        same_bytes(w, a.get_weights(), ('evaluate moved a variable', it))
        sa, sb = state(a, ea), state(b, eb)
        assert sa[3] == sb[3] == it + 1
        for name, da, db in zip(('weights', 'm', 'v'), sa[:3], sb[:3]):
            same_bytes(da, db, (name, 'after step', it))
        moved = moved or any(k.endswith('moving_mean') and v.any() for k, v in w.items())
    if var.get('normalization') == 'bn':
        assert moved                 # (the averages the oracle was given had left their initial values: evaluate used THEM)


# ================================================================================================ 4. DL4DS_AUX_STREAM=1
AUX_MODELS = [
    ('net_postupsampling', dict(backbone_block='densenet', upsampling='spc', scale=2, n_blocks=2, n_filters=8), (2, 8, 8, 1)),
    ('unet_pin', dict(n_filters=4, n_blocks=2, decoder_upsampling='dc'), (2, 16, 16, 2)),
    ('recnet_postupsampling', dict(backbone_block='resnet', upsampling='spc', scale=2, time_window=2, n_filters=4, n_blocks=1),
     (2, 2, 8, 6, 2)),
]


def _env(monkeypatch, aux):
    """aux: the switch under test.  Otherwise the single-stream order with the kernel selection the switch forces: ConvLSTM step by
    step, no copy-free gradient for two fused adds."""
    for k in ('DL4DS_AUX_STREAM', 'DL4DS_NO_CONVLSTM_SEQ', 'DL4DS_NO_TWO_ADD_INPLACE'):
        monkeypatch.delenv(k, raising=False)
    if aux:
        monkeypatch.setenv('DL4DS_AUX_STREAM', '1')
    else:
        monkeypatch.setenv('DL4DS_NO_CONVLSTM_SEQ', '1')
        monkeypatch.setenv('DL4DS_NO_TWO_ADD_INPLACE', '1')


@pytest.mark.parametrize('kind,cfg,xs', AUX_MODELS, ids=['densenet', 'unet_dc', 'recnet'])
def test_aux_stream_equals_single_stream_and_the_oracle(monkeypatch, kind, cfg, xs):
    from dl4ds_amd.training import SupervisedEngine
    runs, ref = [], None
    for aux in (True, False):
        _env(monkeypatch, aux)
        model, P, ocfg = build_pair(kind, cfg, xs, None)
        rng, x, _, pred = tie_free_inputs(kind, P, ocfg, xs, None)
        y = targets_clear_of_the_kink(pred, rng)
        w0 = model.get_weights()
        eng = SupervisedEngine(model, loss='mae', learning_rate=1e-3)
        rec = []
        for it in range(3):
            if it:
                r = np.random.default_rng(900 + it)
                x, y = r.standard_normal(xs).astype(np.float32), r.standard_normal(y.shape).astype(np.float32)
            loss, g = eng.loss_and_grads([x], y)
            if aux and it == 0:
                ref = (g, oracle_reference('supervised', kind, ocfg, w0, x, None, y, loss='mae'))
            rec.append((loss, g, eng.step([x], y), model.get_weights()))
        n = model.graph.aux_launches()
        assert (n > 0) if aux else (n == 0), (aux, n)           # the second stream was really used / really not
        runs.append(rec)
        del eng, model
    for it, ((la, ga, sa, wa), (lb, gb, sb, wb)) in enumerate(zip(*runs)):
        assert la == lb and sa == sb, it
        same_bytes(ga, gb, ('gradients, step', it))
        same_bytes(wa, wb, ('weights after step', it))
    assert_matches_reference(ref[0], ref[1], what=('aux stream', kind))


def test_aux_stream_cgan_step_equals_single_stream_and_the_oracle(monkeypatch):
    import dl4ds_amd.models as PM
    from dl4ds_amd.training import CGANEngine
    B, H = 2, 16
    gcfg = dict(n_filters=4, n_blocks=2, decoder_upsampling='dc')
    dcfg = dict(upsampling='pin', scale=8, n_filters=4, n_res_blocks=2)
    picked, runs = None, []
    for aux in (True, False):
        _env(monkeypatch, aux)
        gen = PM.unet_pin('unet', 3, 1, hr_size=(H, H), seed=3, **gcfg)
        disc = PM.residual_discriminator(3, 'pin', False, 8, (H // 8, H // 8), n_filters=4, n_res_blocks=2, hr_size=(H, H), seed=4)
        g0, d0 = gen.get_weights(), disc.get_weights()
        if picked is None:
            def draw(seed):
                r = np.random.default_rng(seed)
                lr = r.random((B, H, H, 3)).astype(np.float32)
                st = r.random((B, H, H, 1)).astype(np.float32)
                hr = r.random((B, H, H, 1)).astype(np.float32)
                mask = (r.random((2 * B, 8)) > 0.4).astype(np.float32)
                return lr, st, hr, mask, _cgan_banded('unet_pin', gcfg, g0, dcfg, d0, lr, hr, st, mask)
            picked = first_quiet(draw, 90)
        lr, st, hr, mask, bref = picked
        eng = CGANEngine(gen, disc, loss='mae', learning_rate=2e-4, beta_1=0.5)
        out = eng.step([lr, st], hr, dropout_keep=mask)
        grads = {'G:' + k: v for k, v in gen.get_gradients().items()} | {'D:' + k: v for k, v in disc.get_gradients().items()}
        n = gen.graph.aux_launches() + disc.graph.aux_launches()
        assert (n > 0) if aux else (n == 0), (aux, n)
        runs.append((out, grads, gen.get_weights(), disc.get_weights()))
        del eng, gen, disc
    (oa, ga, wga, wda), (ob, gb, wgb, wdb) = runs
    assert oa == ob
    same_bytes(ga, gb, 'cgan gradients')
    same_bytes(wga, wgb, 'generator after the step')
    same_bytes(wda, wdb, 'discriminator after the step')
    assert_matches_reference(ga, bref, what='aux stream cgan')
