"""Multivariate ensemble verification (dl4ds_amd/ensemble_score.py) without a GPU: the argument checks, the
lag list of the library against its definition, the host arithmetic on hand-made sums, and the numpy restatement
tests/multivariate_ref.py, which is the expected side of tests/test_gpu_multivariate.py, against by-hand values."""
import inspect
import math

import numpy as np
import pytest

from tests import multivariate_cases as C
from tests import multivariate_ref as R


def test_exports_and_signatures():
    import dl4ds_amd
    import dl4ds_amd._lib as L
    from dl4ds_amd.graph import Model
    protos = L.parse_header()
    assert len(protos['dl4ds_ensemble_energy'][1]) == 9 and len(protos['dl4ds_ensemble_variogram'][1]) == 15
    assert len(protos['dl4ds_variogram_lags'][1]) == 3
    for name in ('multivariate_scores', 'verify_multivariate', 'MultivariateVerifier'):
        assert callable(getattr(dl4ds_amd, name))
    p = inspect.signature(dl4ds_amd.multivariate_scores).parameters
    assert list(p) == ['y_true', 'members', 'max_lag', 'order', 'lag_weights', 'fair', 'weights', 'mask', 'batch_size']
    assert (p['max_lag'].default, p['order'].default, p['lag_weights'].default, p['fair'].default) == (4, 0.5, 'inverse', False)
    p = inspect.signature(Model.score_multivariate).parameters
    assert list(p) == ['self', 'inputs', 'y_true', 'n_members', 'batch_size', 'seed', 'max_lag', 'order', 'lag_weights', 'fair',
                       'weights']
    v, e = inspect.signature(dl4ds_amd.verify_multivariate).parameters, inspect.signature(dl4ds_amd.verify_exceedance).parameters
    assert set(e) - {'thresholds'} <= set(v) and {'mask', 'time_window', 'save_path', 'scaler', 'weights'} <= set(v)


def test_argument_checks():
    from dl4ds_amd.ensemble_score import check_multivariate_args as check
    from dl4ds_amd.losses import latitude_weights
    from dl4ds_amd.metrics import multivariate_scores
    shape = (6, 5, 1)
    assert check(4, 0.5, 'inverse', False, None, shape) == (4, 0, None)
    assert check(np.int64(8), 2, 'uniform', np.bool_(True), None, None)[:2] == (8, 2) and check(1, 1.0, 'uniform', True, None, shape)[1] == 1
    lag, code, w = check(3, 1, 'inverse', False, latitude_weights(np.linspace(40.0, 50.0, 6), 5), shape)
    assert w.shape == shape and w.dtype == np.float32 and (w > 0).all() and w[2, 0, 0] == np.float32(np.cos(np.deg2rad(44.0)))
    for bad in (dict(order=0.7), dict(order='1'), dict(order=True), dict(max_lag=0), dict(max_lag=9), dict(max_lag=2.0),
                dict(max_lag=True), dict(lag_weights='gauss'), dict(lag_weights=None), dict(fair=1), dict(fair='no'),
                dict(weights=-np.ones(shape)), dict(weights=np.full(shape, np.nan)), dict(weights=np.full(shape, np.inf)),
                dict(weights=np.ones((6, 4, 1))), dict(weights='heavy'), dict(sample_shape=(6, 5)), dict(n_members=1),
                dict(n_members=129)):
        kw = dict(dict(max_lag=4, order=0.5, lag_weights='inverse', fair=False, weights=None, sample_shape=shape), **bad)
        with pytest.raises(ValueError):
            check(**kw)
    y = np.zeros((2,) + shape, np.float32)                                  # refused before the library is touched
    for K in (1, 129):
        with pytest.raises(ValueError, match='members'):
            multivariate_scores(y, np.zeros((K,) + y.shape, np.float32))
    with pytest.raises(ValueError):
        multivariate_scores(y, np.zeros((4, 2, 6, 4, 1), np.float32))
    with pytest.raises(ValueError, match='order'):
        multivariate_scores(y, np.zeros((4,) + y.shape, np.float32), order=0.7)
    with pytest.raises(ValueError, match='batch_size'):
        multivariate_scores(y, np.zeros((4,) + y.shape, np.float32), batch_size=0)


def test_the_lag_list():
    from dl4ds_amd.ensemble_score import variogram_lags
    import dl4ds_amd._lib as L
    counts = {1: 2, 2: 6, 4: 24, 8: 98}
    for lag in range(1, 9):
        got = variogram_lags(lag)
        assert got.dtype == np.int64 and got.tolist() == [list(p) for p in R.lags_ref(lag)], lag
        if lag in counts:
            assert len(got) == counts[lag]
        pairs = [tuple(p) for p in got.tolist()]
        assert pairs == sorted(pairs) and len(set(pairs)) == len(pairs)
        # every unordered offset within the radius appears once: the list and its mirror image tile the punctured disc
        disc = {(dy, dx) for dy in range(-lag, lag + 1) for dx in range(-lag, lag + 1) if 0 < dy * dy + dx * dx <= lag * lag}
        mirror = {(-dy, -dx) for dy, dx in pairs}
        assert set(pairs) | mirror == disc and not set(pairs) & mirror
    for bad in (0, 9, -1):
        with pytest.raises(L.Dl4dsHipError, match='max_lag'):
            variogram_lags(bad)


def test_from_sums_on_hand_made_sums():
    from dl4ds_amd.ensemble_score import multivariate_from_sums
    lags = np.asarray([[0, 1], [1, 0], [1, 1]])
    dist = np.asarray([[9.0, 16.0, 25.0], [4.0, 4.0, 0.0], [0.0, 0.0, 0.0]])       # K = 2: D_0, D_1, G_01
    nvalid = np.asarray([5, 3, 0])
    npairs = np.asarray([[4, 2, 0], [1, 1, 1], [0, 0, 0]])
    sums = np.zeros((3, 3, 3))
    sums[0, :, 0], sums[0, :, 1], sums[0, :, 2] = (2.0, 1.0, 0.0), (4.0, 2.0, 0.0), (8.0, 1.0, 0.0)
    sums[1, :, 0], sums[1, :, 1], sums[1, :, 2] = (1.0, 3.0, 5.0), (1.0, 1.0, 1.0), (2.0, 2.0, 2.0)
    r = multivariate_from_sums(dist, nvalid, npairs, sums, 2, lags, 'uniform', False)
    assert r['energy_score_per_sample'][:2].tolist() == [(3 + 4) / 2 - 5 / 4, 2.0] and np.isnan(r['energy_score_per_sample'][2])
    assert r['energy_score'] == ((3 + 4) / 2 - 5 / 4 + 2.0) / 2
    assert r['member_distance'].tolist() == [[3, 4], [2, 2], [0, 0]] and r['pair_distance'].tolist() == [[5], [0], [0]]
    assert r['variogram_score_per_sample'][:2].tolist() == [3.0 / 6, 9.0 / 3] and np.isnan(r['variogram_score_per_sample'][2])
    assert r['variogram_score'] == 12.0 / 9
    assert r['variogram_error'].tolist() == [3 / 5, 4 / 3, 5.0] and r['variogram_obs'].tolist() == [1.0, 1.0, 1.0]
    assert r['variogram_ens'].tolist() == [2.0, 1.0, 2.0]
    assert r['lag_distance'].tolist() == [1.0, 1.0, math.sqrt(2)] and r['lag_weight'].tolist() == [1, 1, 1]
    assert r['n_members'] == 2 and r['fair'] is False and r['n_pairs'].dtype == np.int64
    f = multivariate_from_sums(dist, nvalid, npairs, sums, 2, lags, 'inverse', True)
    w = 1 / math.sqrt(2)
    assert f['energy_score_per_sample'][0] == (3 + 4) / 2 - 5 / 2
    assert f['variogram_score_per_sample'][1] == math.fsum([1.0, 3.0, w * 5.0]) / math.fsum([1.0, 1.0, w])
    # a lag nobody has a pair for: its variograms are NaN, the scores do not see it
    none = multivariate_from_sums(dist, nvalid, npairs * [1, 1, 0], sums * np.asarray([1, 1, 0])[None, :, None], 2, lags, 'inverse', False)
    assert np.isnan(none['variogram_obs'][2]) and np.isnan(none['variogram_error'][2]) and none['variogram_score'] == 7.0 / 8
    with pytest.raises(ValueError):
        multivariate_from_sums(dist[:, :2], nvalid, npairs, sums, 2, lags, 'uniform', False)


def test_restatement_by_hand():
    # two members, three cells in a row, one sample
    y = np.asarray([1.0, 2.0, 4.0], np.float32).reshape(1, 1, 3, 1)
    m = np.asarray([[1.0, 3.0, 4.0], [2.0, 2.0, 8.0]], np.float32).reshape(2, 1, 1, 3, 1)
    r = R.scores_ref(m, y, max_lag=2, order=1, lag_weights='uniform')
    assert r['dist_sums'].tolist() == [[1.0, 17.0, 18.0]] and r['n_valid_per_sample'].tolist() == [3]
    assert r['energy_score_per_sample'][0] == (1.0 + math.sqrt(17.0)) / 2 - math.sqrt(18.0) / 4
    assert r['lags'].tolist() == [[0, 1], [0, 2], [1, -1], [1, 0], [1, 1], [2, 0]]
    assert r['n_pairs'].tolist() == [[2, 1, 0, 0, 0, 0]]
    # lag (0, 1): o = 1, 2; e = (2 + 0) / 2, (1 + 6) / 2 -> (o - e)^2 = 0, 2.25; lag (0, 2): o = 3, e = (3 + 6) / 2
    assert r['variogram_sums'][0, 0].tolist() == [2.25, 3.0, 4.5] and r['variogram_sums'][0, 1].tolist() == [2.25, 3.0, 4.5]
    assert r['variogram_score'] == 4.5 / 3 and np.isnan(r['variogram_obs'][2:]).all()
    half = R.scores_ref(m, y, max_lag=1, order=0.5)
    e = (np.float64(np.sqrt(np.float32(2.0))) + 0.0) / 2
    assert half['variogram_sums'][0, 0, 2] == math.fsum([e, (1.0 + np.float64(np.sqrt(np.float32(6.0)))) / 2])
    # weight 0 and a NaN exclude their cell, and with it every pair it belongs to
    r = R.scores_ref(m, y, max_lag=2, order=2, weights=np.asarray([1.0, 0.0, 2.0]).reshape(1, 3, 1))
    assert r['n_valid_per_sample'].tolist() == [2] and r['n_pairs'].tolist() == [[0, 1, 0, 0, 0, 0]]
    assert r['dist_sums'].tolist() == [[0.0, 1.0 + 2 * 16.0, 1.0 + 2 * 16.0]]
    y2 = y.copy()
    y2[0, 0, 2, 0] = np.nan
    assert R.scores_ref(m, y2, max_lag=2)['n_pairs'].tolist() == [[1, 0, 0, 0, 0, 0]]


def test_restatement_identities():
    rng = np.random.default_rng(5)
    y = rng.standard_normal((2, 4, 5, 2)).astype(np.float32)
    same = R.scores_ref(np.repeat(y[None], 5, axis=0), y, max_lag=3, order=0.5)               # all members equal the observation
    assert same['energy_score'] == 0 and same['variogram_score'] == 0 and not same['dist_sums'].any()
    x = rng.standard_normal(y.shape).astype(np.float32)
    ident = R.scores_ref(np.repeat(x[None], 4, axis=0), y, max_lag=2, order=1)                 # all members identical: ES = ||x - y||
    norm = [math.sqrt(math.fsum(((x[n].astype(np.float64) - y[n].astype(np.float64)) ** 2).ravel().tolist())) for n in range(2)]
    np.testing.assert_allclose(ident['energy_score_per_sample'], norm, rtol=4 * R.ULP, atol=0)
    assert not ident['pair_distance'].any()


@pytest.mark.parametrize('fair', [False, True])
def test_one_cell_energy_score_is_the_crps(fair):
    """P = 1: sqrt((x - y)^2) = |x - y|, so the energy score of a sample is the CRPS of its one element: the pairwise formula of
    the ensemble restatement (tests/ensemble_score_ref.py), evaluated here."""
    from tests.ensemble_score_ref import crps_pairwise
    rng = np.random.default_rng(9)
    for K in (2, 5, 16):
        m = rng.standard_normal((K, 7, 1, 1, 1)).astype(np.float32)
        y = rng.standard_normal((7, 1, 1, 1)).astype(np.float32)
        es = R.scores_ref(m, y, max_lag=1, fair=fair)['energy_score_per_sample']
        crps = crps_pairwise(m.reshape(K, 7).astype(np.float64), y.reshape(7).astype(np.float64), fair=fair)
        scale = np.abs(m.reshape(K, 7)).max(axis=0) + np.abs(y.reshape(7))
        assert (np.abs(es - crps) <= 8 * K * R.ULP * scale).all(), (K, np.abs(es - crps).max())


def test_the_seeded_structure_case_shows_what_the_variogram_score_is_for():
    """The inputs of the GPU structure test, with the restatement: the smooth and the per-cell shuffled ensemble have the same
    member SET in every cell (so every per-cell score is equal), and the variogram score tells them apart."""
    y, smooth, shuffled = C.structure_case()
    assert np.array_equal(np.sort(smooth, axis=0), np.sort(shuffled, axis=0)) and not np.array_equal(smooth, shuffled)
    a, b = R.scores_ref(smooth, y, max_lag=4, order=0.5), R.scores_ref(shuffled, y, max_lag=4, order=0.5)
    assert b['variogram_score'] > 1.5 * a['variogram_score'] and (b['variogram_score_per_sample'] > a['variogram_score_per_sample']).all()
    assert (b['variogram_ens'] > a['variogram_ens']).all()
