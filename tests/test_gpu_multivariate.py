"""Multivariate ensemble verification on the device: csrc/ensemble_multi.hip through metrics.multivariate_scores on synthetic
member stacks, both entries called directly, and Model.score_multivariate / dl4ds_amd.verify_multivariate through a small
MC-dropout model, against the numpy restatement tests/multivariate_ref.py.

Bounds (tests/multivariate_ref.assert_same): n_pairs, n_valid, lags and every NaN position are EQUAL; a device sum of m
non-negative terms is within (m + 4) 2^-53 relative of the exactly rounded sum, m taken from each case; derived scores get that
bound plus 2 ulp per square root or quotient; the energy score, a difference of two non-negative parts, relative to their sum.  No
element is left out.  The per-sample raw sums are BIT-IDENTICAL for every batch size."""
import ctypes
import math

import numpy as np
import pytest

from tests import multivariate_cases as C
from tests import multivariate_ref as R

pytestmark = pytest.mark.gpu

RAW = ('dist_sums', 'variogram_sums', 'n_pairs', 'n_valid_per_sample')


def same_bits(a, b, what):
    assert set(a) == set(b)
    for k in a:
        assert np.asarray(a[k]).tobytes() == np.asarray(b[k]).tobytes(), (what, k)


@pytest.mark.parametrize('shape', C.SHAPES, ids=str)
@pytest.mark.parametrize('K', C.KS)
def test_kernel_against_the_restatement(K, shape):
    from dl4ds_amd.metrics import multivariate_scores
    m, y = C.data(100 * K + len(shape) + shape[-2], K, shape)
    energy = R.energy_sums_ref(m, y)                                        # once per stack
    for case in C.kernel_cases(K, shape):
        what = f'K={K} {shape} {case}'
        got = multivariate_scores(y, m, **case)
        R.assert_same(got, R.scores_ref(m, y, energy=energy, **case), what)
        assert got['lags'].shape[0] == {1: 2, 3: 14, 8: 98}[case['max_lag']]
        H, W = shape[-3], shape[-2]
        for l, (dy, dx) in enumerate(got['lags'].tolist()):                 # fields smaller than the lag: no pair, NaN variograms
            planes = int(np.prod(shape[:-3])) * shape[-1]
            assert (got['n_pairs'][:, l] == planes * max(H - dy, 0) * max(W - abs(dx), 0)).all(), (what, dy, dx)
            assert np.isnan(got['variogram_obs'][l]) == (dy >= H or abs(dx) >= W)
        for batch in (1, 2):
            other = multivariate_scores(y, m, batch_size=batch, **case)
            for k in RAW:
                assert got[k].tobytes() == other[k].tobytes(), (what, batch, k)
            same_bits(got, other, (what, batch))


def test_invalid_elements_are_excluded_everywhere():
    from dl4ds_amd.metrics import multivariate_scores
    K, shape = 5, (9, 40, 2)
    m, y = C.data(7, K, shape, n=4)
    y[0, 2, 3, 0], y[0, 8, 39, 1], y[1, 0, 0, 0] = np.nan, np.inf, -np.inf
    m[3, 0, 4, 31, 1], m[0, 1, 5, 32, 0], m[4, 1, 8, 0, 1] = np.nan, np.inf, -np.inf
    y[2] = np.nan                                                           # a sample with no valid element
    mask = np.ones(shape[:2])
    mask[4, 10:20] = 0
    w = np.ones(shape, np.float32)
    w[:, 5] = 0                                                             # zero weights exclude as well
    ym = y.copy()
    ym[:, 4, 10:20] = np.nan
    kw = dict(max_lag=3, order=0.5, weights=w)
    ref = R.scores_ref(m, ym, **kw)
    for mk in (mask, mask[..., None]):
        got = multivariate_scores(y, m, mask=mk, batch_size=3, **kw)
        R.assert_same(got, ref, 'invalid')
    assert got['n_valid_per_sample'].tolist() == [9 * 39 * 2 - 20 - 3, 9 * 39 * 2 - 20 - 3, 0, 9 * 39 * 2 - 20]
    assert np.isnan(got['energy_score_per_sample'][2]) and np.isnan(got['variogram_score_per_sample'][2])
    assert not got['dist_sums'][2].any() and not got['n_pairs'][2].any() and np.isfinite(got['energy_score'])
    keep = [0, 1, 3]
    assert got['energy_score'] == math.fsum(got['energy_score_per_sample'][keep].tolist()) / 3
    assert np.isnan(y[2]).all() and y[0, 4, 10, 0] == y[0, 4, 10, 0], 'the caller\'s observation was written'
    empty = multivariate_scores(np.full_like(y, np.nan), m, max_lag=2)
    R.assert_same(empty, R.scores_ref(m, np.full_like(y, np.nan), max_lag=2), 'all invalid')
    assert np.isnan(empty['energy_score']) and np.isnan(empty['variogram_score']) and np.isnan(empty['variogram_ens']).all()


def test_latitude_weights_weight_the_energy_score():
    from dl4ds_amd.losses import latitude_weights
    from dl4ds_amd.metrics import multivariate_scores
    K, shape = 6, (12, 37, 1)
    m, y = C.data(11, K, shape)
    w = latitude_weights(np.linspace(-100.0, 65.0, 12), 37)                 # a row past the pole has weight 0: excluded
    assert w.shape == (12, 37) and not w[0].any()
    for fair in (False, True):
        got = multivariate_scores(y, m, max_lag=2, order=1, fair=fair, weights=w)
        ref = R.scores_ref(m, y, max_lag=2, order=1, fair=fair, weights=w[..., None])
        R.assert_same(got, ref, f'latitude weights, fair={fair}')
        assert got['n_valid_per_sample'].tolist() == [11 * 37] * 3
    plain = multivariate_scores(y, m, max_lag=2, order=1)
    assert (plain['dist_sums'] > got['dist_sums']).all()


@pytest.mark.parametrize('fair', [False, True])
def test_one_cell_energy_score_is_the_crps_kernel(fair):
    """P = 1 on the device: the energy score of a one-cell sample is its CRPS.  ``ensemble_scores`` documents its accuracy in
    DESIGN.md section 13: per element within 1 ulp of float32, folds within 2^-22."""
    from dl4ds_amd.metrics import ensemble_scores, multivariate_scores
    rng = np.random.default_rng(3)
    for K in (2, 7, 40):
        m = rng.standard_normal((K, 50, 1, 1, 1)).astype(np.float32)
        y = rng.standard_normal((50, 1, 1, 1)).astype(np.float32)
        got = multivariate_scores(y, m, max_lag=1, fair=fair)
        ref = R.scores_ref(m, y, max_lag=1, fair=fair)
        R.assert_same(got, ref, f'P = 1, K={K}')
        assert not got['n_pairs'].any() and np.isnan(got['variogram_score'])
        crps = ensemble_scores(y, m, fair=fair)['crps_per_sample']
        bound = (5 * R.EPS + 6 * R.ULP) * ref['_parts'].sum(axis=1) + (2.0 ** -23 + 2.0 ** -22) * np.abs(crps)
        err = np.abs(got['energy_score_per_sample'] - crps)
        print(f'K={K} fair={fair}: worst |ES - CRPS| / bound {(err / bound).max():.3f}')
        assert (err <= bound).all(), (K, float((err / bound).max()))


def test_the_variogram_score_sees_structure_the_per_cell_scores_cannot():
    from dl4ds_amd.metrics import ensemble_scores, multivariate_scores
    y, smooth, shuffled = C.structure_case()
    a, b = ensemble_scores(y, smooth), ensemble_scores(y, shuffled)
    assert a['crps'] == b['crps'] and a['crps_per_sample'].tobytes() == b['crps_per_sample'].tobytes()
    assert np.array_equal(a['rank_histogram'], b['rank_histogram'])
    va, vb = multivariate_scores(y, smooth, max_lag=4, order=0.5), multivariate_scores(y, shuffled, max_lag=4, order=0.5)
    R.assert_same(va, R.scores_ref(smooth, y, max_lag=4, order=0.5), 'smooth')
    R.assert_same(vb, R.scores_ref(shuffled, y, max_lag=4, order=0.5), 'shuffled')
    assert vb['variogram_score'] > va['variogram_score'] and (vb['variogram_score_per_sample'] > va['variogram_score_per_sample']).all()


def direct(lib, which, m, y, B, K=None, n=None, stride=None, null=(), dims=None, max_lag=2, order=0, w=None):
    """dl4ds_ensemble_energy / dl4ds_ensemble_variogram called directly -> (status, first output, second output)"""
    from dl4ds_amd.device import DeviceArray
    K0, n0 = m.shape[0], (m.shape[1] if n is None else n)
    K, stride = (K0 if K is None else K), (m.shape[1] if stride is None else stride)
    rows = max(B, 1)
    dm, dy = DeviceArray.from_numpy(m), DeviceArray.from_numpy(y)
    dw = DeviceArray.from_numpy(w) if w is not None else None
    ptr = lambda k, d: None if k in null or d is None else d.ptr               # noqa: E731
    if which == 'energy':
        a, b = DeviceArray.from_numpy(np.full((rows, K0 * (K0 + 1) // 2), -7.0)), DeviceArray.from_numpy(np.full(rows, -7, np.int64))
        st = lib.dl4ds_ensemble_energy(ptr('members', dm), K, n0, stride, ptr('obs', dy), B, ptr('w', dw), ptr('out0', a), ptr('out1', b))
    else:
        L = len(R.lags_ref(max_lag)) if 1 <= max_lag <= 8 else 1
        a, b = DeviceArray.from_numpy(np.full((rows, L), -7, np.int64)), DeviceArray.from_numpy(np.full((rows, L, 3), -7.0))
        st = lib.dl4ds_ensemble_variogram(ptr('members', dm), K, n0, stride, ptr('obs', dy), B, ptr('w', dw), *dims, max_lag, order,
                                          ptr('out0', a), ptr('out1', b))
    out = (st, a.numpy(), b.numpy())
    for d in (dm, dy, a, b) + ((dw,) if dw is not None else ()):
        d.free()
    return out


def test_entries_called_directly():
    import dl4ds_amd._lib as L
    lib = L.lib()
    B, shape, K = 3, (2, 6, 5, 3), 4
    per = int(np.prod(shape))
    m, y = C.data(5, K, shape, n=B)
    pad = 5                                                                 # a member stride wider than n, and so misaligned rows
    wide = np.zeros((K, B * per + pad), np.float32)
    wide[:, :B * per] = m.reshape(K, -1)
    dims = (2, 6, 5, 3)
    dist_ref, nvalid_ref = R.energy_sums_ref(m, y)
    np_ref, sums_ref = R.variogram_sums_ref(m, y, 2, 0.5)
    runs = [direct(lib, 'energy', wide, y.reshape(-1), B, n=B * per) for _ in range(2)]
    L.check(runs[0][0])
    assert runs[0][1].tobytes() == runs[1][1].tobytes() and runs[0][2].tolist() == nvalid_ref.tolist()          # overwritten, same bits
    R.close(runs[0][1], dist_ref, (per + 4) * R.EPS, what='direct energy')
    runs = [direct(lib, 'variogram', wide, y.reshape(-1), B, n=B * per, dims=dims) for _ in range(2)]
    L.check(runs[0][0])
    assert runs[0][1].tobytes() == runs[1][1].tobytes() and runs[0][2].tobytes() == runs[1][2].tobytes()
    assert runs[0][1].tolist() == np_ref.tolist()
    R.close(runs[0][2], sums_ref, (np_ref[:, :, None] + 4) * R.EPS, what='direct variogram')
    flat, obs = m.reshape(K, -1), y.reshape(-1)
    for which, name in (('energy', 'ensemble_energy'), ('variogram', 'ensemble_variogram')):
        for kw in (dict(K=1), dict(K=129), dict(B=7), dict(B=0), dict(stride=B * per - 1), dict(null=('members',)),
                   dict(null=('obs',)), dict(null=('out0',)), dict(null=('out1',))):
            kw = dict(dict(B=B, dims=dims), **kw)
            with pytest.raises(L.Dl4dsHipError, match=name):
                L.check(direct(lib, which, flat, obs, **kw)[0])
    for kw in (dict(max_lag=0), dict(max_lag=9), dict(order=3), dict(order=-1), dict(dims=(2, 6, 5, 2)), dict(dims=(1, 6, 5, 3))):
        kw = dict(dict(B=B, dims=dims), **kw)
        with pytest.raises(L.Dl4dsHipError, match='ensemble_variogram'):
            L.check(direct(lib, 'variogram', flat, obs, **kw)[0])


# ------------------------------------------------------------------------------------------------ through the model
LR, SCALE = (16, 20), 2
HR = (LR[0] * SCALE, LR[1] * SCALE)


def mc_model():                                             # (the builder and size of tests/test_gpu_exceedance.py)
    import dl4ds_amd.models as PM
    return PM.net_postupsampling('resnet', 'spc', SCALE, 1, 0, LR, n_filters=8, n_blocks=2, dropout_rate=0.3, dropout_variant='mcdrop',
                                 seed=1)


def fields(n, seed=0, grid=LR, c=1):
    return np.random.default_rng(seed).standard_normal((n,) + tuple(grid) + (c,)).astype(np.float32)


def test_score_multivariate_is_predict_ensemble_plus_multivariate_scores():
    from dl4ds_amd.losses import latitude_weights
    from dl4ds_amd.metrics import multivariate_scores
    m = mc_model()
    x = fields(7, 1)
    y = m.predict(x) + 0.05 * fields(7, 2, HR)
    y[2, 3, 4, 0] = np.nan
    w = latitude_weights(np.linspace(30.0, 60.0, HR[0]), HR[1])
    kw = dict(max_lag=3, order=1, lag_weights='uniform', fair=True, weights=w)
    res = m.score_multivariate(x, y, 6, seed=77, batch_size=3, **kw)
    plain = m.predict_ensemble(x, 6, seed=77, batch_size=3, return_members=True)
    for k in ('mean', 'std', 'min', 'max', 'quantiles'):
        assert res[k].tobytes() == plain[k].tobytes(), k
    assert 'members' not in res and 'scores' not in res
    same_bits(res['multivariate'], multivariate_scores(y, plain['members'], **kw), 'score_multivariate')
    R.assert_same(res['multivariate'], R.scores_ref(plain['members'], y, **dict(kw, weights=w[..., None])), 'score_multivariate')
    assert res['multivariate']['n_valid_per_sample'].tolist() == [HR[0] * HR[1] - (i == 2) for i in range(7)]
    with pytest.raises(ValueError, match='y_true'):
        m.score_multivariate(x, y[:, :-1], 4)
    with pytest.raises(ValueError, match='members'):
        m.score_multivariate(x, y, 1)


@pytest.mark.parametrize('kind', [None, 'standard'])
def test_verify_multivariate(kind, tmp_path):
    """The scores are taken in the model's units: equal to ``multivariate_scores`` on the raw members and the transformed,
    masked observation."""
    import dl4ds_amd
    from dl4ds_amd.metrics import multivariate_scores
    from dl4ds_amd.preprocessing import StandardScaler
    m = mc_model()
    rng = np.random.default_rng(12)
    kelvin = (281.0 + 12.0 * rng.standard_normal((5,) + HR + (1,))).astype(np.float32)
    mask = np.ones(HR)
    mask[:3] = 0
    if kind is None:
        sc, arr = None, fields(5, 14, HR)
        y_true, y_model = arr, arr.copy()
    else:
        sc = StandardScaler(axis=None).fit(kelvin)
        arr = np.asarray(sc.transform(kelvin), np.float32).reshape(kelvin.shape)
        y_true = kelvin
        y_model = np.asarray(sc.transform(kelvin.copy()), np.float32).reshape(kelvin.shape)
    y_model[:, :3] = np.nan
    kw = dict(seed=21, batch_size=2, scaler=sc)
    mv = dict(max_lag=2, order=2, fair=False)
    res, lr = dl4ds_amd.verify_multivariate(m, arr, SCALE, 6, y_true=None if kind is None else y_true, mask=mask,
                                            save_path=str(tmp_path), return_lr=True, **kw, **mv)
    ens = dl4ds_amd.predict_ensemble(m, arr, SCALE, 6, **kw)
    for k in ('mean', 'std', 'min', 'max', 'quantiles'):
        assert res[k].tobytes() == ens[k].tobytes(), k
    assert lr.shape == (5,) + LR + (1,)
    raw = dl4ds_amd.predict_ensemble(m, arr, SCALE, 6, return_members=True, seed=21, batch_size=2)['members']
    got = res['multivariate']
    same_bits(got, multivariate_scores(y_model, raw, **mv), f'verify_multivariate {kind}')
    R.assert_same(got, R.scores_ref(raw, y_model, **mv), f'verify_multivariate {kind}')
    assert got['n_valid_per_sample'].tolist() == [(HR[0] - 3) * HR[1]] * 5
    saved = np.load(tmp_path / 'y_hat_multivariate.npz')
    assert set(saved.files) == {k for k in res if k != 'multivariate'} | {'multivariate_' + k for k in got}
    assert saved['multivariate_dist_sums'].tobytes() == got['dist_sums'].tobytes() and saved['mean'].tobytes() == res['mean'].tobytes()
    again = dl4ds_amd.MultivariateVerifier(m, arr, SCALE, 6, y_true=None if kind is None else y_true, mask=mask, array_in_hr=True,
                                           **kw, **mv).run()
    same_bits(got, again['multivariate'], 'verifier')
    with pytest.raises(ValueError, match='time_window'):
        dl4ds_amd.verify_multivariate(m, arr, SCALE, 6, y_true=y_true, time_window=2, scaler=sc)


def test_verify_multivariate_on_another_grid_than_the_model_was_built_for():
    """A model built for 16 x 20 inputs applied to 12 x 24 ones runs on its re-planned sibling: the weights have the shape of THAT
    output."""
    import dl4ds_amd
    from dl4ds_amd.losses import latitude_weights
    from dl4ds_amd.metrics import multivariate_scores
    m = mc_model()
    grid = (12 * SCALE, 24 * SCALE)
    arr = fields(4, 31, grid)
    y = arr + 0.1 * fields(4, 32, grid)
    w = latitude_weights(np.linspace(-20.0, 20.0, grid[0]), grid[1])
    res = dl4ds_amd.verify_multivariate(m, arr, SCALE, 5, y_true=y, seed=4, batch_size=3, weights=w)
    raw = dl4ds_amd.predict_ensemble(m, arr, SCALE, 5, return_members=True, seed=4, batch_size=3)['members']
    same_bits(res['multivariate'], multivariate_scores(y, raw, weights=w), 'other grid')
    R.assert_same(res['multivariate'], R.scores_ref(raw, y, weights=w[..., None]), 'other grid')
    with pytest.raises(ValueError, match='weights'):
        dl4ds_amd.verify_multivariate(m, arr, SCALE, 5, y_true=y, weights=np.ones(HR + (1,)))      # a map for the BUILD grid
