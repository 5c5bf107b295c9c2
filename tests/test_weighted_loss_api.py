"""CPU checks of the per-grid-cell loss weights: the Python-side validation (losses.check_loss_weights, latitude_weights), the
trainers' `loss_weights` keyword, and the identities of the fp64 reference (tests/weighted_loss_ref.py) that the GPU tests are
measured against."""
import numpy as np
import pytest
import torch

from oracle import torch_ops as T
from tests import weighted_loss_cases as K
from tests import weighted_loss_ref as R


def _fields(n, hw, seed=0):
    return np.random.default_rng(seed).random((n, hw, hw, 1)).astype(np.float32)


def test_check_loss_weights_accepts_the_valid_forms():
    from dl4ds_amd.losses import check_loss_weights
    rng = np.random.default_rng(0)
    for shape in [(6, 8), (6, 8, 1), (6, 8, 3)]:
        w = rng.random(shape)
        out = check_loss_weights(w, (6, 8, 3), 'mae')
        assert out.dtype == np.float32 and out.shape == shape and out.flags.c_contiguous
        np.testing.assert_array_equal(out, w.astype(np.float32))
    assert check_loss_weights(np.eye(5), (5, 5), 'dssim_mae').shape == (5, 5)              # (H, W) grid shape, zeros allowed
    assert check_loss_weights(np.ones((5, 5), bool), (9, 5, 5, 1), 'mse').dtype == np.float32


@pytest.mark.parametrize('bad,match', [
    (np.ones((6, 7)), 'do not fit'),
    (np.ones((6, 8, 2)), 'do not fit'),
    (np.ones((2, 6, 8, 1)), 'do not fit'),               # a full-field map has no batch axis
    (np.where(np.arange(48).reshape(6, 8) == 5, -1e-3, 1.0), '>= 0'),
    (np.where(np.arange(48).reshape(6, 8) == 7, np.nan, 1.0), 'finite'),
    (np.where(np.arange(48).reshape(6, 8) == 7, np.inf, 1.0), 'finite'),
    (np.zeros((6, 8)), 'zero everywhere'),
])
def test_check_loss_weights_rejects(bad, match):
    from dl4ds_amd.losses import check_loss_weights
    with pytest.raises(ValueError, match=match):
        check_loss_weights(bad, (6, 8, 3), 'mae')


@pytest.mark.parametrize('kind', ['msdssim', 'msdssim_mae', 'msdssim_mae_mse'])
def test_check_loss_weights_refuses_the_multiscale_kinds(kind):
    from dl4ds_amd.losses import check_loss_weights
    with pytest.raises(ValueError, match=kind):
        check_loss_weights(np.ones((96, 96)), (96, 96, 1), kind)


def test_weight_form():
    from dl4ds_amd.ops import weight_form
    b = (6, 5, 7, 3)
    assert weight_form((5, 7), b) == (1, 1) and weight_form((5, 7, 1), b) == (1, 1) and weight_form((5, 7, 3), b) == (1, 3)
    assert weight_form((6, 5, 7, 1), b) == (6, 1) and weight_form((3, 5, 7, 3), b) == (3, 3) and weight_form((1, 5, 7, 3), b) == (1, 3)
    for bad in [(5, 7, 2), (4, 5, 7, 1), (7, 5), (6, 5, 7, 2), (6,)]:
        with pytest.raises(ValueError):
            weight_form(bad, b)


def test_latitude_weights():
    from dl4ds_amd.losses import latitude_weights
    lat = np.array([-90.0, -60.0, -12.5, 0.0, 33.0, 89.0, 95.0])
    w = latitude_weights(lat, 5)
    assert w.shape == (7, 5) and w.dtype == np.float32
    ref = np.clip(np.cos(np.deg2rad(lat)), 0.0, None).astype(np.float32)
    for x in range(5):
        np.testing.assert_array_equal(w[:, x], ref)
    assert w[-1, 0] == 0.0 and (w >= 0).all()                  # beyond the pole: clipped


@pytest.mark.parametrize('kind', R.KINDS)
@pytest.mark.parametrize('const', [1.0, 3.5])
def test_reference_constant_weights_equal_the_unweighted_oracle(kind, const):
    rng = np.random.default_rng(5)
    t = torch.tensor(rng.random((2, 14, 17, 2)))
    p = torch.tensor(rng.random((2, 14, 17, 2)) - 0.2)
    for w in (np.full((14, 17), const), np.full((2, 14, 17, 2), const)):
        a = R.loss_w(kind, t, p, R.broadcast_weights(w, tuple(t.shape)))
        assert abs(float(a) - float(getattr(T, kind)(t, p))) < 1e-12


@pytest.mark.parametrize('kind', ['mae', 'mse'])
def test_reference_mask_is_the_mean_over_the_kept_entries(kind):
    rng = np.random.default_rng(6)
    t, p = rng.standard_normal((3, 9, 8, 2)), rng.standard_normal((3, 9, 8, 2))
    m = rng.random((3, 9, 8, 1)) < 0.6
    full = np.broadcast_to(m, t.shape)
    d = (p - t)[full]
    want = np.abs(d).mean() if kind == 'mae' else (d ** 2).mean()
    v, g = R.value_and_grad(kind, t, p, m.astype(np.float64))
    assert abs(v - want) < 1e-12
    assert (g[~full] == 0).all()
    tn = np.where(full, t, np.nan)                                 # exclusion: a NaN under the mask reaches nothing
    v2, g2 = R.value_and_grad(kind, tn, p, m.astype(np.float64))
    assert v2 == v and np.array_equal(g2, g)


def test_reference_zero_weights_give_zero():
    rng = np.random.default_rng(7)
    t, p = rng.random((1, 12, 12, 1)), rng.random((1, 12, 12, 1))
    for kind in R.KINDS:
        v, g = R.value_and_grad(kind, t, p, np.zeros((12, 12)))
        assert v == 0.0 and not g.any()


def test_cases_keep_the_residuals_clear_of_zero():
    for shape in K.PIXEL_SHAPES:
        for form in K.PIXEL_FORMS:
            t, p, w = K.pixel_case(shape, form)
            assert (np.abs(p - t) >= K.MIN_RESIDUAL).all()
            zeros = float((w == 0).mean())
            assert 0.05 < zeros < 0.6, (shape, form, zeros)
            R.broadcast_weights(w, t.shape)


def test_trainers_accept_the_keyword_and_refuse_host_patches():
    from dl4ds_amd.training import SupervisedTrainer, CGANTrainer
    tr, va, te = _fields(6, 16), _fields(4, 16, 1), _fields(4, 16, 2)
    w = np.random.default_rng(1).random((16, 16)).astype(np.float32)
    t = SupervisedTrainer('resnet', 'spc', tr, va, te, scale=2, batch_size=2, epochs=1, loss_weights=w, verbose=False)
    np.testing.assert_array_equal(t.loss_weights, w)
    assert SupervisedTrainer('resnet', 'spc', tr, va, te, scale=2, batch_size=2, epochs=1, verbose=False).loss_weights is None
    # patches on the host generator: no crop corners to cut the map at
    with pytest.raises(ValueError, match='device_data=False'):
        SupervisedTrainer('resnet', 'spc', tr, va, te, scale=2, batch_size=2, epochs=1, patch_size=8, device_data=False,
                          loss_weights=w, verbose=False)
    # ... without patches the host path takes the map
    t = SupervisedTrainer('resnet', 'spc', tr, va, te, scale=2, batch_size=2, epochs=1, device_data=False, loss_weights=w,
                          verbose=False)
    assert t.loss_weights.shape == (16, 16)
    SupervisedTrainer('resnet', 'spc', tr, va, te, scale=2, batch_size=2, epochs=1, patch_size=8, loss_weights=w, verbose=False)
    with pytest.raises(ValueError, match='do not fit'):
        SupervisedTrainer('resnet', 'spc', tr, va, te, scale=2, batch_size=2, epochs=1, loss_weights=w[:8], verbose=False)
    with pytest.raises(ValueError, match='msdssim'):
        SupervisedTrainer('resnet', 'spc', tr, va, te, scale=2, batch_size=2, epochs=1, loss='msdssim', loss_weights=w,
                          verbose=False)
    topo = np.random.default_rng(3).random((16, 16)).astype(np.float32)
    c = CGANTrainer('resnet', 'spc', tr, te, static_vars=[topo], scale=2, batch_size=2, epochs=1, loss_weights=w, verbose=False)
    np.testing.assert_array_equal(c.loss_weights, w)
    with pytest.raises(ValueError, match='zero everywhere'):
        CGANTrainer('resnet', 'spc', tr, te, static_vars=[topo], scale=2, batch_size=2, epochs=1, loss_weights=0 * w, verbose=False)
