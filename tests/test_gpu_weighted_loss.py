"""Per-grid-cell loss weights on the MI355X: the weighted loss op (csrc/losses.hip, csrc/dssim.hip) against the fp64 reference of
tests/weighted_loss_ref.py, exclusion of zero-weight entries, degenerate sums, determinism, and the wiring through the supervised
and CGAN engines, the patch generator and SupervisedTrainer.

Tolerances are the loss op's own (tests/test_gpu_ops.py::test_dssim_losses): value rel 2e-4 / abs 1e-6, gradient within 1e-3 of the
reference gradient's largest magnitude."""
import numpy as np
import pytest

from tests import weighted_loss_cases as K
from tests import weighted_loss_ref as R

pytestmark = pytest.mark.gpu

PIXEL_KINDS = ['mae', 'mse']
DSSIM_KINDS = ['dssim', 'dssim_mae', 'dssim_mse', 'dssim_mae_mse']


@pytest.fixture(scope='module')
def ops():
    import dl4ds_amd.ops as o
    return o


def close(a, ref, tol=1e-3):
    ref = np.asarray(ref, np.float64)
    a = np.asarray(a, np.float64)
    assert a.shape == ref.shape, (a.shape, ref.shape)
    scale = max(np.abs(ref).max(), 1e-6)
    err = np.abs(a - ref).max() / scale
    assert err < tol, f'max rel err {err:.3e}'


def value_close(a, ref):
    assert a == pytest.approx(ref, rel=2e-4, abs=1e-6)


# ---------------------------------------------------------------------------------------------- 1. pixel kinds against the reference
@pytest.mark.parametrize('form', K.PIXEL_FORMS)
@pytest.mark.parametrize('shape', K.PIXEL_SHAPES, ids=str)
def test_pixel_kinds_against_the_reference(ops, shape, form):
    t, p, w = K.pixel_case(shape, form)
    assert (np.abs(p - t) >= K.MIN_RESIDUAL).all()          # the MAE sign is never in question: the reference alone decides
    for kind in PIXEL_KINDS:
        v, g = ops.loss(kind, t, p, weights=w)
        rv, rg = R.value_and_grad(kind, t, p, w)
        print(kind, shape, form, v, rv)
        value_close(v, rv)
        close(g, rg)


# ---------------------------------------------------------------------------------------------- 2. exclusion
@pytest.mark.parametrize('fill', [np.nan, np.inf], ids=['nan', 'inf'])
@pytest.mark.parametrize('form', K.PIXEL_FORMS)
@pytest.mark.parametrize('shape', K.PIXEL_SHAPES, ids=str)
def test_zero_weight_entries_are_excluded_by_selection(ops, shape, form, fill):
    t, p, w = K.pixel_case(shape, form)
    tm, masked = K.with_masked_truth(t, w, fill)
    assert masked.any() and not np.isfinite(tm[masked]).any()
    for kind in PIXEL_KINDS:
        v0, g0 = ops.loss(kind, t, p, weights=w)
        v1, g1 = ops.loss(kind, tm, p, weights=w)
        assert np.float32(v1).tobytes() == np.float32(v0).tobytes()
        assert g1.tobytes() == g0.tobytes()
        assert np.isfinite(v1) and np.isfinite(g1).all()
        assert (g1[masked] == 0).all() and not np.signbit(g1[masked]).any()


# ---------------------------------------------------------------------------------------------- 3. degenerate sums
@pytest.mark.parametrize('kind', PIXEL_KINDS + DSSIM_KINDS)
def test_all_zero_weights_give_zero_loss_and_gradient(ops, kind):
    rng = np.random.default_rng(3)
    t, p = rng.standard_normal((2, 13, 12, 2)).astype(np.float32), rng.standard_normal((2, 13, 12, 2)).astype(np.float32)
    for w in (np.zeros((13, 12), np.float32), np.zeros((2, 13, 12, 2), np.float32)):
        v, g = ops.loss(kind, t, p, weights=w)
        assert v == 0.0 and not np.isnan(g).any() and not g.any()


@pytest.mark.parametrize('kind', PIXEL_KINDS + DSSIM_KINDS)
def test_unit_weights_reproduce_the_unweighted_op(ops, kind):
    rng = np.random.default_rng(4)
    t = rng.random((2, 19, 23, 2)).astype(np.float32)
    p = (t + 0.1 * rng.standard_normal(t.shape) - 0.2).astype(np.float32)
    v0, g0 = ops.loss(kind, t, p)
    for w in (np.ones((19, 23), np.float32), np.ones((2, 19, 23, 2), np.float32)):
        v, g = ops.loss(kind, t, p, weights=w)
        value_close(v, v0)
        close(g, g0)


# ---------------------------------------------------------------------------------------------- 4. DSSIM kinds against the reference
@pytest.mark.parametrize('data', K.DSSIM_DATA)
@pytest.mark.parametrize('form', K.DSSIM_FORMS)
@pytest.mark.parametrize('shape', K.DSSIM_SHAPES, ids=str)
def test_dssim_kinds_against_the_reference(ops, shape, form, data):
    t, p, w = K.dssim_case(shape, form, data)
    if form == 'left_zero' and shape[2] > 15:
        om = R.window_weights(R.broadcast_weights(w, t.shape)).numpy()
        assert not om[:, :, :5].any() and (om[:, :, 5:] > 0).all()           # windows with ox <= 4 are the excluded ones
    for kind in DSSIM_KINDS:
        v, g = ops.loss(kind, t, p, weights=w)
        rv, rg = R.value_and_grad(kind, t, p, w)
        print(kind, shape, form, data, v, rv)
        value_close(v, rv)
        close(g, rg)


def test_dssim_mae_on_kelvin_fields_with_a_block_of_windows_masked(ops):
    """The weighted tile kernels take the same pivoted moments as the unweighted ones: data with a mean of 7 dynamic ranges
    (tests/ssim_cases.py: the kelvin class), a mask that removes 7 x 10 whole windows per sample."""
    from tests import ssim_cases as S
    case = S.FIELD_WEIGHTED_CASE
    t, p = S.loss_inputs(case)
    w = np.ones(case.shape[1:3], np.float32)
    w[S.FIELD_MASK_BLOCK] = 0.0
    om = R.window_weights(R.broadcast_weights(w, t.shape)).numpy()
    assert (om == 0).sum() == case.shape[0] * 7 * 10
    v, g = ops.loss(case.kind, t, p, weights=w)
    rv, rg = R.value_and_grad(case.kind, t, p, w)
    print(case.id, v, rv, np.abs(g - rg).max() / np.abs(rg).max())
    assert np.isfinite(v) and np.isfinite(g).all()
    value_close(v, rv)
    close(g, rg)


# ---------------------------------------------------------------------------------------------- 5. refusal
@pytest.mark.parametrize('kind', ['msdssim', 'msdssim_mae', 'msdssim_mae_mse'])
def test_multiscale_kinds_with_weights_are_refused(ops, kind):
    import ctypes
    from dl4ds_amd import _lib
    from dl4ds_amd.device import DeviceArray
    t = np.random.default_rng(0).random((1, 96, 96, 1)).astype(np.float32)
    w = np.ones((96, 96), np.float32)
    with pytest.raises(ValueError, match=kind):
        ops.loss(kind, t, t, weights=w)
    # ... and at the C ABI, not silently unweighted
    dt, dw, lv = DeviceArray.from_numpy(t), DeviceArray.from_numpy(w), DeviceArray.zeros((8,))
    st = _lib.lib().dl4ds_op_loss_weighted(ops.LOSS_KINDS[kind], dt.ptr, dt.ptr, None, 1, 96, 96, 1, dw.ptr, 1, 1, lv.ptr)
    assert st != 0
    msg = _lib.lib().dl4ds_last_error().decode()
    assert 'multi-scale' in msg and msg.rstrip().split(' [')[0].endswith(kind), msg
    assert ops.loss(kind, t, t)[0] == pytest.approx(0.0, abs=1e-6)             # the unweighted call still works


# ---------------------------------------------------------------------------------------------- 6. determinism
def test_same_inputs_same_bits(ops):
    t, p, w = K.pixel_case((2, 40, 40, 1), 'per_sample')
    runs = [ops.loss('mae', t, p, weights=w) for _ in range(2)]
    assert np.float32(runs[0][0]).tobytes() == np.float32(runs[1][0]).tobytes() and runs[0][1].tobytes() == runs[1][1].tobytes()
    t, p, w = K.dssim_case((1, 27, 30, 2), 'random', 'fixups')
    runs = [ops.loss('dssim_mae_mse', t, p, weights=w) for _ in range(2)]
    assert np.float32(runs[0][0]).tobytes() == np.float32(runs[1][0]).tobytes() and runs[0][1].tobytes() == runs[1][1].tobytes()


# ---------------------------------------------------------------------------------------------- 7. trainer wiring
def _small_net(seed=1):
    import dl4ds_amd.models as PM
    return PM.net_postupsampling('resnet', 'spc', 2, 1, 0, (8, 8), n_blocks=1, n_filters=4, seed=seed)


def _batch(seed=0):
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((2, 8, 8, 1)).astype(np.float32)
    y = rng.standard_normal((2, 16, 16, 1)).astype(np.float32)
    return rng, x, y


def test_engine_loss_is_the_weighted_op_on_the_model_output(ops):
    from dl4ds_amd.training import SupervisedEngine
    rng, x, y = _batch()
    for kind, w in (('mae', K.random_weights(rng, (16, 16))), ('dssim_mse', K.random_weights(rng, (2, 16, 16, 1)))):
        m = _small_net()
        eng = SupervisedEngine(m, loss=kind, learning_rate=1e-3)
        eng.set_loss_weights(w)
        lv, _ = eng.loss_and_grads([x], y)
        value_close(lv, ops.loss(kind, y, m([x]), want_grad=False, weights=w)[0])
        # d. evaluate uses the map (inference forward = training forward here: no dropout, no normalisation)
        value_close(eng.evaluate([x], y), lv)
        assert abs(lv - ops.loss(kind, y, m([x]), want_grad=False)[0]) > 1e-3 * abs(lv)        # ... and the map matters


def test_engine_unit_weights_equal_the_unweighted_engine():
    from dl4ds_amd.training import SupervisedEngine
    _, x, y = _batch(1)
    m0, m1 = _small_net(), _small_net()
    l0, g0 = SupervisedEngine(m0, loss='mae', learning_rate=1e-3).loss_and_grads([x], y)
    e1 = SupervisedEngine(m1, loss='mae', learning_rate=1e-3)
    e1.set_loss_weights(np.ones((16, 16, 1), np.float32))
    l1, g1 = e1.loss_and_grads([x], y)
    value_close(l1, l0)
    assert set(g0) == set(g1)
    for k in g0:
        close(g1[k], g0[k], 1e-3)


def test_engine_backpropagates_the_weighted_gradient():
    """mse with a 0/1 mask: sum m d^2 / sum m has (n / sum m) times the parameter gradients of the unweighted mse whose y_true is
    the model's own output on the masked cells (d == 0 there) -- so the weighted dpred really is what is back-propagated."""
    from dl4ds_amd.training import SupervisedEngine
    rng, x, y = _batch(2)
    mask = (rng.random((16, 16)) < 0.6).astype(np.float32)
    m0, m1 = _small_net(), _small_net()
    out = m0([x])
    y_fill = np.where(mask[None, :, :, None] > 0, y, out).astype(np.float32)
    _, g0 = SupervisedEngine(m0, loss='mse', learning_rate=1e-3).loss_and_grads([x], y_fill)
    e1 = SupervisedEngine(m1, loss='mse', learning_rate=1e-3)
    e1.set_loss_weights(mask)
    _, g1 = e1.loss_and_grads([x], y)
    ratio = mask.size / mask.sum()
    for k in g0:
        assert np.abs(g0[k]).max() > 0
        close(g1[k], ratio * g0[k].astype(np.float64), 1e-3)


def test_clearing_the_weights_restores_the_unweighted_bits():
    from dl4ds_amd.training import SupervisedEngine
    rng, x, y = _batch(3)
    m = _small_net()
    eng = SupervisedEngine(m, loss='dssim_mae', learning_rate=1e-3)
    l0, g0 = eng.loss_and_grads([x], y)
    eng.set_loss_weights(K.random_weights(rng, (2, 16, 16, 1)))
    l1, _ = eng.loss_and_grads([x], y)
    assert l1 != l0
    eng.set_loss_weights(None)
    l2, g2 = eng.loss_and_grads([x], y)
    assert np.float32(l2).tobytes() == np.float32(l0).tobytes()
    for k in g0:
        assert g2[k].tobytes() == g0[k].tobytes(), k


def test_per_sample_weights_for_another_batch_size_fail_at_the_step():
    from dl4ds_amd._lib import Dl4dsHipError
    from dl4ds_amd.training import SupervisedEngine
    _, x, y = _batch(4)
    eng = SupervisedEngine(_small_net(), loss='mae', learning_rate=1e-3)
    eng.set_loss_weights(np.ones((3, 16, 16, 1), np.float32))
    with pytest.raises(Dl4dsHipError, match='batch size'):
        eng.loss_and_grads([x], y)
    with pytest.raises(ValueError):
        eng.set_loss_weights(np.ones((8, 8), np.float32))
    with pytest.raises(ValueError, match='msdssim'):
        SupervisedEngine(_small_net(), loss='msdssim', learning_rate=1e-3).set_loss_weights(np.ones((16, 16), np.float32))


# ---------------------------------------------------------------------------------------------- 8. patches
def test_crop_field_cuts_at_the_stored_corners():
    from dl4ds_amd.dataloader import DeviceDataGenerator
    from dl4ds_amd.device import DeviceArray
    data = np.random.default_rng(0).random((6, 16, 16, 1)).astype(np.float32)
    gen = DeviceDataGenerator(data, None, 'resnet', 'spc', 2, batch_size=3, patch_size=8, seed=5)
    yy, xx = np.mgrid[0:16, 0:16]
    ramp = (1000 * yy + xx).astype(np.float32)
    ramp2 = np.stack([ramp, -ramp], axis=-1)
    d1, d2 = DeviceArray.from_numpy(ramp), DeviceArray.from_numpy(ramp2)
    seen = set()
    for i in range(2):
        (lr,), (hr,) = gen[i]
        idx, cy, cx = gen.last_draw
        assert len(idx) == 3 and lr.shape == (3, 4, 4, 1) and hr.shape == (3, 8, 8, 1)
        c1, c2 = gen.crop_field(d1).numpy(), gen.crop_field(d2).numpy()
        assert c1.shape == (3, 8, 8, 1) and c2.shape == (3, 8, 8, 2)
        for b in range(3):
            np.testing.assert_array_equal(c1[b, :, :, 0], ramp[cy[b]:cy[b] + 8, cx[b]:cx[b] + 8])
            np.testing.assert_array_equal(c2[b], ramp2[cy[b]:cy[b] + 8, cx[b]:cx[b] + 8])
            np.testing.assert_array_equal(hr.numpy()[b], data[idx[b], cy[b]:cy[b] + 8, cx[b]:cx[b] + 8])
            seen.add((int(cy[b]), int(cx[b])))
    assert len(seen) > 1
    with pytest.raises(ValueError):
        gen.crop_field(DeviceArray.from_numpy(np.zeros((8, 8), np.float32)))


def test_supervised_trainer_runs_on_patches_with_a_weight_map(capsys):
    import re
    from dl4ds_amd.training import SupervisedTrainer
    rng = np.random.default_rng(0)
    yy, xx = np.mgrid[0:16, 0:16] / 16

    def fields(n):      # a fixed pattern far from the initial output: every Adam step lowers the loss by more than the patches differ
        return (5.0 + 0.2 * np.sin(6 * xx)[None] + 0.01 * rng.random((n, 16, 16)))[..., None].astype(np.float32)
    w = K.random_weights(rng, (16, 16))
    w[:4] = 0.0
    t = SupervisedTrainer('resnet', 'spc', fields(8), fields(4), fields(4), scale=2, batch_size=2, patch_size=8, epochs=2,
                          steps_per_epoch=2, learning_rate=1e-2, loss='mae', loss_weights=w, verbose=True, save=False,
                          n_blocks=1, n_filters=4)
    t.run()
    printed = [float(v) for v in re.findall(r'Epoch \d+/2 - 2 steps - loss: ([0-9.eE+-]+|nan|inf)', capsys.readouterr().out)]
    assert len(printed) == 2 and np.isfinite(printed).all() and printed[1] <= printed[0], printed
    assert np.isfinite(t.fithist['val_loss']).all() and np.isfinite(t.test_loss)


# ---------------------------------------------------------------------------------------------- 9. CGAN
def test_cgan_pixel_loss_takes_the_weights_and_the_adversarial_terms_do_not(ops):
    import dl4ds_amd.models as PM
    from dl4ds_amd.training import CGANEngine
    rng = np.random.default_rng(0)
    B, H, lam = 2, 16, 100.0
    lr, st, hr = (rng.random((B, H, H, c)).astype(np.float32) for c in (2, 1, 1))
    mask = (rng.random((2 * B, 8)) > 0.4).astype(np.float32)
    w = K.random_weights(rng, (H, H))

    def engine():
        gen = PM.net_pin('resnet', 2, 1, hr_size=(H, H), n_filters=4, n_blocks=1, seed=3)           # no dropout, no normalisation
        disc = PM.residual_discriminator(2, 'pin', False, 8, (H // 8, H // 8), n_filters=4, n_res_blocks=1, hr_size=(H, H), seed=4)
        return gen, CGANEngine(gen, disc, loss='mae', lambda_scaling_factor=lam)
    gen0, e0 = engine()
    tot0, gan0, px0, disc0 = e0.step([lr, st], hr, dropout_keep=mask, apply_update=False)
    gen1, e1 = engine()
    e1.set_loss_weights(w)
    tot1, gan1, px1, disc1 = e1.step([lr, st], hr, dropout_keep=mask, apply_update=False)
    want = ops.loss('mae', hr, gen1([lr, st]), want_grad=False, weights=w)[0]
    value_close(px1, want)
    value_close(tot1 - gan1, lam * want)                      # the generator's total carries lambda times the weighted term
    assert abs(px1 - px0) > 1e-3 * px0
    assert np.float32(gan1).tobytes() == np.float32(gan0).tobytes() and np.float32(disc1).tobytes() == np.float32(disc0).tobytes()
    e1.set_loss_weights(None)
    assert e1.step([lr, st], hr, dropout_keep=mask, apply_update=False) == (tot0, gan0, px0, disc0)
