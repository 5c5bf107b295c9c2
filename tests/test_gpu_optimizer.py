"""The extended optimiser step on the device (csrc/adam_ext.hip): clipping by the global gradient norm,
decoupled weight decay and the weight average, op by op through dl4ds_op_adam_ext / dl4ds_op_arena_swap and through the engines.
Sizes, ranges and inputs: tests/optimizer_cases.py; float64 reference and bounds: tests/optimizer_ref.py.

Measured on an MI355X (largest error / bound over the cases; a record, nothing reads it): norm 3.2e-8 relative against the 1.19e-7
bound; op level m' 0.48, v' 0.56, w' 0.57, ema' 0.50; through the supervised engine m' 0.43, v' 0.89, w' 0.60, ema' 0.46."""
import numpy as np
import pytest

from tests import optimizer_cases as C
from tests import optimizer_ref as R
from tests import step_kernels_cases as S

pytestmark = pytest.mark.gpu

F32, F64 = np.float32, np.float64
ADAM = dict(lr=S.ADAM_LR, beta1=S.ADAM_B1, beta2=S.ADAM_B2, eps=S.ADAM_EPS)


@pytest.fixture(scope='module')
def ops():
    import dl4ds_amd.ops as o
    return o


def _same(a, b):
    return np.asarray(a).tobytes() == np.asarray(b).tobytes()


# ---------------------------------------------------------------------------------------------------------------- 1: off = adam
@pytest.mark.parametrize('n', C.SIZES)
def test_everything_off_is_the_old_kernel(ops, n):
    """dl4ds_op_adam_ext with clipping off, decay 0 and no average, and again with clipping on at a limit far above the gradient's
    norm (c == 1 exactly), returns w', m', v' bit-identical to dl4ds_op_adam, for grad_scale 1 and 1 / 3."""
    w, g, m, v, _ = C.inputs(n)
    for gs in C.SCALES:
        for t in C.STEPS:
            want = ops.adam(w, g, m, v, t, grad_scale=gs, **ADAM)
            off = ops.adam_ext(w, g, m, v, t, grad_scale=gs, **ADAM)
            far = ops.adam_ext(w, g, m, v, t, grad_scale=gs, global_clipnorm=1e30, **ADAM)
            for got in (off, far):
                assert all(_same(a, b) for a, b in zip(got[:3], want)), (n, gs, t)
                assert got[3] is None
            assert off[4] == dict(grad_norm=0.0, clip_factor=1.0, skipped_steps=0)
            assert far[4]['clip_factor'] == 1.0 and far[4]['grad_norm'] > 0 and far[4]['skipped_steps'] == 0


# ---------------------------------------------------------------------------------------------------------------- 2: the norm
@pytest.mark.parametrize('n', C.SIZES)
def test_reported_norm(ops, n):
    """norm within 2^-23 relative of grad_scale * ||g||_2 in float64 (one float32 rounding, 2^-24, dominates; the float64
    accumulation of exact squares is at the 2^-53 level per addition), the same bits on a second call, and
    c == fl32(clip / max(norm, clip)) of the reported norm for a clip below and above it."""
    w, g, m, v, _ = C.inputs(n)
    worst = 0.0
    for gs in C.SCALES:
        ref = R.global_norm64(g, gs)
        for clip in (0.25 * ref, 4.0 * ref):
            a = ops.adam_ext(w, g, m, v, 1, grad_scale=gs, global_clipnorm=clip, **ADAM)[4]
            b = ops.adam_ext(w, g, m, v, 1, grad_scale=gs, global_clipnorm=clip, **ADAM)[4]
            rel = abs(F64(a['grad_norm']) - ref) / ref
            worst = max(worst, rel)
            assert rel <= 2.0 ** -23, (n, gs, rel)
            assert _same(a['grad_norm'], b['grad_norm']) and _same(a['clip_factor'], b['clip_factor'])
            assert _same(a['clip_factor'], R.clip_factor32(a['grad_norm'], clip)), (n, gs, clip)
            assert (a['clip_factor'] == 1.0) == (clip > ref)
    print(f'norm n={n}: relative error {worst:.3e} (bound {2.0 ** -23:.3e})')


# ---------------------------------------------------------------------------------------------------------------- 3: the update
def _run_case(ops, n, t, gs, clip, wd, ranges, use_ema):
    w, g, m, v, ema = C.inputs(n)
    got = ops.adam_ext(w, g, m, v, t, grad_scale=gs, global_clipnorm=clip, weight_decay=wd, decay_ranges=ranges,
                       ema=ema if use_ema else None, ema_momentum=C.EMA_MOMENTUM, **ADAM)
    w1, m1, v1, e1, st = got
    if clip is None:
        assert st['grad_norm'] == 0.0 and st['clip_factor'] == 1.0
    else:
        assert _same(st['clip_factor'], R.clip_factor32(st['grad_norm'], clip))
    mask = R.decay_mask(n, ranges) if wd else None
    ref = R.step_ref(w, g, m, v, ema if use_ema else None, t, gs, st['clip_factor'], wd, mask, C.EMA_MOMENTUM, m1=m1, v1=v1, w1=w1)
    out = dict(w=w1, m=m1, v=v1)
    if use_ema:
        out['ema'] = e1
    r = R.ratios(out, ref)
    assert max(r.values()) <= 1.0, (n, t, gs, clip, wd, ranges, use_ema, r)
    return got, r


@pytest.mark.parametrize('n', C.SIZES)
def test_clipped_decayed_averaged_update(ops, n):
    """Against tests/optimizer_ref.py fed the device's reported c: every element of w', m', v', ema' within the reference's bound,
    for a clip below, at and above the norm, all eight on / off combinations of the three features, steps 1 and 7 and every decayed
    range set of the size; elements outside the decayed ranges are bit-identical to a run with decay 0."""
    w, g, m, v, ema = C.inputs(n)
    large = n == C.NORM_LARGEST
    worst = {}
    for gs in ((1.0 / 3.0,) if large else C.SCALES):
        norm32 = ops.adam_ext(w, g, m, v, 1, grad_scale=gs, global_clipnorm=1.0, **ADAM)[4]['grad_norm']
        sets = [s for s in C.decay_range_sets(n) if s]
        for t in C.STEPS:
            # clip below / at / above the norm, everything on (at the norm: c == 1 exactly)
            for clip, c_is_one in ((0.5 * float(norm32), False), (float(norm32), True), (2.0 * float(norm32), True)):
                got, r = _run_case(ops, n, t, gs, clip, C.WEIGHT_DECAY, sets[-1], True)
                assert (got[4]['clip_factor'] == 1.0) == c_is_one
                worst = {k: max(worst.get(k, 0.0), x) for k, x in r.items()}
            for on_clip, on_decay, on_ema in C.FEATURES:
                clip = 0.5 * float(norm32) if on_clip else None
                plain = None
                for ranges in (sets[-1:] if large or not on_decay else sets):
                    wd = C.WEIGHT_DECAY if on_decay else 0.0
                    got, r = _run_case(ops, n, t, gs, clip, wd, ranges if on_decay else [], on_ema)
                    worst = {k: max(worst.get(k, 0.0), x) for k, x in r.items()}
                    if on_decay:
                        if plain is None:
                            plain, _ = _run_case(ops, n, t, gs, clip, 0.0, [], on_ema)
                        out = ~R.decay_mask(n, ranges)
                        for a, b in zip(got[:4], plain[:4]):
                            assert (a is None and b is None) or _same(a[out], b[out]), (n, t, ranges)
                        inside = ~out
                        assert not np.array_equal(got[0][inside], plain[0][inside])
    print(f'adam_ext n={n}: error / bound ' + ', '.join(f'{k} {x:.3e}' for k, x in sorted(worst.items())))


# ---------------------------------------------------------------------------------------------------------------- 4: non-finite
@pytest.mark.parametrize('bad', [np.inf, np.nan])
@pytest.mark.parametrize('n', [5, 2051])
def test_non_finite_gradient_skips_the_step(ops, n, bad):
    """One Inf or NaN in g at the first, a middle and the last element: w, m, v and ema come back bit-identical to the inputs,
    skipped rises by one, and a following clean step applies its update."""
    w, g, m, v, ema = C.inputs(n)
    kw = dict(global_clipnorm=1.0, weight_decay=C.WEIGHT_DECAY, decay_ranges=[(0, n)], ema_momentum=C.EMA_MOMENTUM, **ADAM)
    for pos in (0, n // 2, n - 1):
        gb = g.copy()
        gb[pos] = bad
        w1, m1, v1, e1, st = ops.adam_ext(w, gb, m, v, 3, ema=ema, skipped=4, **kw)
        assert _same(w1, w) and _same(m1, m) and _same(v1, v) and _same(e1, ema), (n, pos)
        assert st['skipped_steps'] == 5 and not np.isfinite(st['grad_norm'])
    w2, m2, v2, e2, st2 = ops.adam_ext(w, g, m, v, 4, ema=ema, skipped=5, **kw)
    assert st2['skipped_steps'] == 5 and np.isfinite(st2['grad_norm'])
    assert not np.array_equal(w2, w) and not np.array_equal(m2, m) and not np.array_equal(e2, ema)
    mask = R.decay_mask(n, [(0, n)])
    ref = R.step_ref(w, g, m, v, ema, 4, 1.0, st2['clip_factor'], C.WEIGHT_DECAY, mask, C.EMA_MOMENTUM, m1=m2, v1=v2, w1=w2)
    assert max(R.ratios(dict(w=w2, m=m2, v=v2, ema=e2), ref).values()) <= 1.0


# ---------------------------------------------------------------------------------------------------------------- 5: the swap
@pytest.mark.parametrize('n', C.SIZES)
def test_arena_swap_is_exact_and_an_involution(ops, n):
    w, _, _, _, ema = C.inputs(n)
    a1, b1 = ops.arena_swap(w, ema)
    assert _same(a1, ema) and _same(b1, w)
    a2, b2 = ops.arena_swap(a1, b1)
    assert _same(a2, w) and _same(b2, ema)


# ---------------------------------------------------------------------------------------------------------------- engines
def _sup_model(seed=5):
    import dl4ds_amd.models as PM
    return PM.net_postupsampling('resnet', 'spc', 4, 1, 0, (16, 16), n_blocks=2, seed=seed)


def _sup_batch():
    rng = np.random.default_rng(0)
    return rng.standard_normal((2, 16, 16, 1)).astype(F32), rng.standard_normal((2, 64, 64, 1)).astype(F32)


EXT = dict(global_clipnorm=1e-3, weight_decay=C.WEIGHT_DECAY, ema_momentum=0.9)


def test_supervised_engine_three_steps_follow_the_reference():
    """Three steps of the smallest net_postupsampling model of tests/test_gpu_trainers.py with all three features on.  After each
    step the gradients are read back (the update leaves the arena in place) and the host reference advances from the previous
    weights, moments and averages with exactly those gradients and the reported c: everything stays within the bound."""
    from dl4ds_amd.training import SupervisedEngine
    x, y = _sup_batch()
    model = _sup_model()
    eng = SupervisedEngine(model, loss='mae', learning_rate=S.ADAM_LR, **EXT)
    assert eng.decayed and all(len(model.graph.params[k]['shape']) >= 2 for k in eng.decayed)
    assert eng.optimizer_stats() == {'grad_norm': 0.0, 'clip_factor': 1.0, 'skipped_steps': 0}
    worst = {}
    for t in (1, 2, 3):
        w0, e0 = model.get_weights(), eng.ema_state()
        m0, v0, _ = eng.optimizer_state()
        if t == 1:
            assert all(_same(w0[k], e0[k]) for k in w0)                  # the averages start as copies of the weights
        eng.step([x], y)
        st = eng.optimizer_stats()
        grads = model.get_gradients()
        norm = np.sqrt(sum(float(np.sum(a.astype(F64) ** 2)) for a in grads.values()))
        assert abs(st['grad_norm'] - norm) <= 2.0 ** -23 * norm
        assert _same(F32(st['clip_factor']), R.clip_factor32(st['grad_norm'], EXT['global_clipnorm'])) and st['skipped_steps'] == 0
        if t == 1:
            assert st['clip_factor'] < 1.0                               # the case is one where clipping acts
        w1, e1 = model.get_weights(), eng.ema_state()
        m1, v1, step = eng.optimizer_state()
        assert step == t
        for k in w0:
            mask = np.full(w0[k].shape, k in eng.decayed)
            ref = R.step_ref(w0[k], grads[k], m0[k], v0[k], e0[k], t, 1.0, F32(st['clip_factor']), EXT['weight_decay'], mask,
                             EXT['ema_momentum'], m1=m1[k], v1=v1[k], w1=w1[k])
            r = R.ratios(dict(w=w1[k], m=m1[k], v=v1[k], ema=e1[k]), ref)
            assert max(r.values()) <= 1.0, (t, k, r)
            worst = {q: max(worst.get(q, 0.0), z) for q, z in r.items()}
    print('supervised engine: error / bound ' + ', '.join(f'{k} {z:.3e}' for k, z in sorted(worst.items())))


def test_cgan_engine_pair_of_clip_values_and_generator_average():
    """One CGAN step on the smallest CGAN test model with a (generator, discriminator) pair of clip values: each optimiser reports
    the norm of its own gradient arena and the factor of its own limit, the generator's average moves by the rule, and the
    discriminator has (and accepts) no average."""
    import dl4ds_amd.models as PM
    from dl4ds_amd import _lib
    from dl4ds_amd.training import CGANEngine
    rng = np.random.default_rng(0)
    B, H = 2, 16
    lr, st, hr = (rng.random((B, H, H, c)).astype(F32) for c in (2, 1, 1))
    keep = (rng.random((2 * B, 8)) > 0.4).astype(F32)
    gen = PM.unet_pin('unet', 2, 1, hr_size=(H, H), n_filters=4, n_blocks=2, decoder_upsampling='dc', seed=3)
    disc = PM.residual_discriminator(2, 'pin', False, 8, (H // 8, H // 8), n_filters=4, n_res_blocks=1, hr_size=(H, H), seed=4)
    clips = (1e-3, 1e6)
    eng = CGANEngine(gen, disc, loss='mae', global_clipnorm=clips, weight_decay=(C.WEIGHT_DECAY, None), ema_momentum=0.9)
    assert eng.decayed[0] and not eng.decayed[1]
    w0, e0 = gen.get_weights(), eng.ema_state()
    assert all(_same(w0[k], e0[k]) for k in w0)
    eng.step([lr, st], hr, dropout_keep=keep)
    for which, model, clip in (('generator', gen, clips[0]), ('discriminator', disc, clips[1])):
        s = eng.optimizer_stats(which)
        norm = np.sqrt(sum(float(np.sum(a.astype(F64) ** 2)) for a in model.get_gradients().values()))
        assert norm > 0 and abs(s['grad_norm'] - norm) <= 2.0 ** -23 * norm, (which, s, norm)
        assert _same(F32(s['clip_factor']), R.clip_factor32(s['grad_norm'], clip)) and s['skipped_steps'] == 0
        assert (s['clip_factor'] == 1.0) == (which == 'discriminator')
    w1, e1 = gen.get_weights(), eng.ema_state()
    moved = False
    for k in w0:
        val, bound = R.ema_ref(e0[k], w1[k], 0.9)
        assert (np.abs(e1[k].astype(F64) - val) <= bound).all(), k
        moved = moved or not np.array_equal(e1[k], e0[k])
    assert moved
    with pytest.raises(_lib.Dl4dsHipError):
        _lib.check(eng._l.dl4ds_cgan_set_optimizer_ext(eng.h, 1, 0.0, 0.0, None, 0, 0.9))
    before = gen.get_weights()
    eng.swap_ema()
    assert all(_same(gen.get_weights()[k], e1[k]) for k in e1)
    eng.swap_ema()
    assert all(_same(gen.get_weights()[k], before[k]) for k in before)


def test_ema_weights_context_manager():
    """evaluate inside ema_weights() equals evaluate of a second model that was loaded with the averages; leaving the block restores
    the training weights bit for bit, also when the body raises."""
    from dl4ds_amd.training import SupervisedEngine
    x, y = _sup_batch()
    model = _sup_model()
    eng = SupervisedEngine(model, loss='mae', learning_rate=S.ADAM_LR, **EXT)
    for _ in range(2):
        eng.step([x], y)
    train_w, avg = model.get_weights(), eng.ema_state()
    assert any(not np.array_equal(train_w[k], avg[k]) for k in avg)
    with eng.ema_weights():
        inside = eng.evaluate([x], y)
        assert all(_same(model.get_weights()[k], avg[k]) for k in avg)
    assert all(_same(model.get_weights()[k], train_w[k]) for k in train_w)
    other = _sup_model(seed=9)
    other.set_weights(avg)
    assert SupervisedEngine(other, loss='mae').evaluate([x], y) == inside
    assert eng.evaluate([x], y) != inside
    with pytest.raises(RuntimeError, match='body failed'):
        with eng.ema_weights():
            raise RuntimeError('body failed')
    assert all(_same(model.get_weights()[k], train_w[k]) for k in train_w)
    assert all(_same(eng.ema_state()[k], avg[k]) for k in avg)


def test_checkpoint_round_trip_with_the_average(tmp_path):
    """A checkpoint written with the average on, loaded into a fresh engine, reproduces the next step bit for bit (loss, weights,
    averages); a checkpoint without ema/ entries loads into an averaging engine by re-initialising the averages from the weights."""
    from dl4ds_amd.training import SupervisedEngine
    x, y = _sup_batch()
    m_a = _sup_model()
    e_a = SupervisedEngine(m_a, loss='mae', learning_rate=S.ADAM_LR, **EXT)
    for _ in range(2):
        e_a.step([x], y)
    e_a.save_checkpoint(tmp_path / 'ck.npz')
    assert any(k.startswith('ema/') for k in np.load(tmp_path / 'ck.npz').keys())
    m_b = _sup_model(seed=11)
    e_b = SupervisedEngine(m_b, loss='mae', learning_rate=S.ADAM_LR, **EXT)
    assert e_b.load_checkpoint(tmp_path / 'ck.npz') == 2
    assert e_a.step([x], y) == e_b.step([x], y)
    for got, want in ((m_b.get_weights(), m_a.get_weights()), (e_b.ema_state(), e_a.ema_state())):
        assert all(_same(got[k], want[k]) for k in want)
    assert e_a.optimizer_stats() == e_b.optimizer_stats()
    plain = SupervisedEngine(_sup_model(seed=12), loss='mae')
    plain.step([x], y)
    plain.save_checkpoint(tmp_path / 'plain.npz')
    assert not any(k.startswith('ema/') for k in np.load(tmp_path / 'plain.npz').keys())
    m_c = _sup_model(seed=13)
    e_c = SupervisedEngine(m_c, loss='mae', ema_momentum=0.9)
    e_c.load_checkpoint(tmp_path / 'plain.npz')
    w, avg = m_c.get_weights(), e_c.ema_state()
    assert all(_same(w[k], avg[k]) for k in w) and all(_same(w[k], plain.model.get_weights()[k]) for k in w)


# ---------------------------------------------------------------------------------------------------------------- trainers
def _fields(n, hw, seed):
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:hw, 0:hw] / hw
    base = np.sin(6 * xx)[None] * np.cos(4 * yy)[None]
    return (base + 0.3 * rng.random((n, 1, 1)) + 0.05 * rng.random((n, hw, hw)))[..., None].astype(F32)


def test_supervised_trainer_with_the_extensions(capsys):
    """SupervisedTrainer.run() with all three on: the epoch line shows the gradient norm and the skipped steps, and when run()
    returns the model holds the averages (the engine's shadow arena then holds the training weights)."""
    from dl4ds_amd.training import SupervisedTrainer
    tr, va, te = _fields(16, 32, 0), _fields(8, 32, 1), _fields(8, 32, 2)
    t = SupervisedTrainer('resnet', 'spc', tr, va, te, scale=4, batch_size=4, loss='mae', epochs=2, learning_rate=1e-3,
                          verbose=2, n_blocks=2, n_filters=4, save=False, global_clipnorm=0.5, weight_decay=1e-3, ema_momentum=0.9)
    t.run()
    out = capsys.readouterr().out
    assert 'grad_norm:' in out and 'skipped_steps: 0' in out
    st = t.engine.optimizer_stats()
    assert st['grad_norm'] > 0 and 0 < st['clip_factor'] <= 1 and st['skipped_steps'] == 0
    avg, train = t.model.get_weights(), t.engine.ema_state()
    assert all(np.isfinite(a).all() for a in avg.values())
    assert any(not np.array_equal(avg[k], train[k]) for k in avg)
    # the averages lag the training weights: one more averaging step from them lands between the two
    k = t.engine.decayed[0]
    assert np.isfinite(t.test_loss) and len(t.fithist['val_loss']) == 2
    with t.engine.ema_weights():
        assert all(_same(t.model.get_weights()[q], train[q]) for q in train)
    assert _same(t.model.get_weights()[k], avg[k])


def test_cgan_trainer_with_the_extensions(tmp_path):
    """CGANTrainer.run() with a pair of clip values, decay and the generator's average: checkpoints carry generator/ema/ entries
    and the training weights, the generator-weight files and the generator after run() hold the averages."""
    from dl4ds_amd.training import CGANTrainer
    tr, te = _fields(8, 32, 0), _fields(4, 32, 1)
    topo = np.random.default_rng(3).random((32, 32)).astype(F32)
    t = CGANTrainer('unet', 'pin', tr, te, static_vars=[topo], scale=4, batch_size=4, epochs=2, verbose=False,
                    checkpoints_frequency=1, save_path=str(tmp_path) + '/',
                    generator_params=dict(n_filters=4, n_blocks=2, decoder_upsampling='dc'),
                    discriminator_params=dict(n_filters=4, n_res_blocks=1),
                    global_clipnorm=(1.0, 5.0), weight_decay=1e-3, ema_momentum=0.9)
    t.run()
    ck = np.load(tmp_path / 'checkpoints' / 'checkpoint_epoch-2.npz')
    saved = np.load(tmp_path / 'checkpoints' / 'save_epoch2_generator_weights.npz')
    avg = t.generator.get_weights()
    for k in avg:
        assert _same(avg[k], saved[k]) and _same(avg[k], ck['generator/ema/' + k]), k
        assert _same(t.engine.ema_state()[k], ck['generator/w/' + k]), k
    assert any(not np.array_equal(avg[k], ck['generator/w/' + k]) for k in avg)
    for which in ('generator', 'discriminator'):
        s = t.engine.optimizer_stats(which)
        assert s['grad_norm'] > 0 and s['skipped_steps'] == 0
    assert np.isfinite(t.test_loss)
