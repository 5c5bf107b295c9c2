"""Ensemble verification on the device: csrc/ensemble_score.hip through metrics.ensemble_scores on synthetic member stacks, and
Model.score_ensemble / dl4ds_amd.verify_ensemble through small models, against the fp64 numpy restatement
tests/ensemble_score_ref.py (CRPS by the O(K^2) pairwise definition).

Bounds (derived, not tuned):
* integer outputs (ranks, rank histogram, covered counts) are EQUAL to the restatement's.  One exclusion: where a quantile is
  genuinely interpolated (non-integer position AND its two order statistics differ) the existing ensemble tests allow it 1 ulp of
  float32, so an element with |y - Q_j| <= 1 ulp(Q_j) is left out of the covered comparison (the count may then lie anywhere
  between the restatement's count without and with those elements); at most 1 % of the elements of any (case, quantile).
* per-element floats: |got - ref| <= 1 ulp_fp32(ref) + K 2^-50 max_k |x_k - y| for crps (the second term bounds the fp64
  evaluation on the differences), the same with max_k |x_k - mean| for sqerr and var.  NaN positions coincide.
* folds: each term at most 1 ulp off, one final rounding: |got - ref| <= 2^-22 sum |terms| (the relative 2^-22 of a sum of
  non-negative terms); counts exact. The fair CRPS is not a sum of non-negative terms: its two parts can cancel to exactly 0
  (members (0, 0, a) against y = 0: a / 3 - 2 a / 6), where the bound is 0 too; the kernel divides by K and by K (K - 1) like
  the definition, so that such an element is exactly 0 there as well, and the bound holds for both forms as stated.
"""
import warnings

import numpy as np
import pytest

from tests import ensemble_score_ref as R

pytestmark = pytest.mark.gpu

KS = [1, 2, 3, 5, 8, 16, 17, 31, 32, 33, 64, 65, 128, 256]
Q3 = [0.05, 0.5, 0.95]
KINDS = ('normal', 'kelvin', 'relu')


def case(rng, kind, K, shape):
    """-> (members (K,) + shape, obs shape) float32"""
    z = rng.standard_normal((K + 1,) + tuple(shape))
    if kind == 'kelvin':
        z = 300.0 + 0.1 * z                                   # a temperature field: 300 K with a spread of 0.1 K
    elif kind == 'relu':
        z = np.maximum(z, 0.0)                                # ReLU-ended: many members and observations exactly 0 -> ties
    z = z.astype(np.float32)
    return z[:K], z[K]


def check_scores(got, members, obs, q=(), fair=False, seed=0, scale=None, label='', ref=None, fields=True):
    """``fields=False``: a result without the per-element fields (verify_ensemble): everything but those is checked"""
    K = members.shape[0]
    ref = R.score_ref(members, obs, q, fair=fair, seed=seed, scale=scale) if ref is None else ref
    v = ref['valid']
    # integers: exact
    if fields:
        np.testing.assert_array_equal(got['rank_field'], ref['rank'], err_msg=f'{label}: ranks')
    np.testing.assert_array_equal(got['rank_histogram'], np.bincount(ref['rank'][v], minlength=K + 1), err_msg=f'{label}: histogram')
    assert got['n_valid'] == int(v.sum()) and got['rank_histogram'].dtype == np.int64
    shares = []
    for j in range(len(q)):
        with np.errstate(invalid='ignore'):
            near = np.abs(ref['Q'][j].astype(np.float64) - np.asarray(obs, np.float64)) <= R.ulp32(ref['Q'][j])
        excl = ref['interp'][j] & near & v
        lo = int((ref['covered'][j] & ~excl).sum())
        share = float(excl.sum()) / max(v.size, 1)
        shares.append(share)
        assert share <= 0.01, f'{label}: quantile {j}: {share:.2e} of the covered flags excluded'
        assert lo <= got['covered'][j] <= lo + int(excl.sum()), (label, j, lo, int(got['covered'][j]), int(excl.sum()))
    # per-element floats
    worst = {}
    for k, extra in (('crps', 'dmax'), ('sqerr', 'mmax'), ('var', 'mmax')) if fields else ():
        g = got[k + '_field']
        assert g.dtype == np.float32 and g.shape == ref[k].shape
        np.testing.assert_array_equal(np.isnan(g), ~v, err_msg=f'{label} {k}: NaN positions')
        if v.any():
            err = np.abs(g.astype(np.float64) - ref[k])[v]
            bound = (R.ulp32(ref[k]) + K * 2.0**-50 * ref[extra])[v]
            worst[k] = float((err / R.ulp32(ref[k])[v]).max())
            assert (err <= bound).all(), (label, k, worst[k])
    # folds
    ps, pc = R.folds(ref)
    mag_s, mag_c = R.folds(dict(ref, **{k: np.abs(ref[k]) for k in ('crps', 'sqerr', 'var')}))
    np.testing.assert_array_equal(got['sample_sums'][:, 3], ps[:, 3])
    np.testing.assert_array_equal(got['cell_sums'][3], pc[3])
    worst['sample sums (2^-22)'] = float((np.abs(got['sample_sums'] - ps) / np.maximum(2.0**-22 * mag_s, 1e-300)).max())
    worst['cell sums (2^-22)'] = float((np.abs(got['cell_sums'] - pc) / np.maximum(2.0**-22 * mag_c, 1e-300)).max())
    print(f'{label}: folds, error over 2^-22 sum |terms|: ' + ', '.join(f'{k} {x:.3g}' for k, x in list(worst.items())[-2:]))
    assert (np.abs(got['sample_sums'] - ps) <= 2.0**-22 * mag_s).all(), f'{label}: per-sample sums'
    assert (np.abs(got['cell_sums'] - pc) <= 2.0**-22 * mag_c).all(), f'{label}: per-cell sums'
    if v.any():
        s = R.summary(ref, K)
        assert abs(got['crps'] - s['crps']) <= 2.0**-21 * np.abs(ref['crps'][v]).mean()
        np.testing.assert_allclose([got['rmse'], got['spread']], [s['rmse'], s['spread']], rtol=2.0**-21)
        np.testing.assert_allclose(got['coverage'], got['covered'] / v.sum(), rtol=1e-15)
    print(f'{label}: worst ulp ' + ', '.join(f'{k} {x:.2f}' for k, x in worst.items() if k in ('crps', 'sqerr', 'var')) +
          ('; excluded covered flags ' + ', '.join(f'{x:.1e}' for x in shares) if shares else ''))
    return worst


@pytest.mark.parametrize('K', KS)
def test_score_kernel_against_the_pairwise_restatement(K):
    from dl4ds_amd.metrics import ensemble_scores
    rng = np.random.default_rng(2000 + K)
    # (shape, batch): one element; 5 samples of 207 cells in chunks of 2 (tails, elem_offset > 0); whole 16-byte groups
    shapes = [((1, 1), None), ((5, 207), 2), ((4, 1024), None)] if K <= 64 else [((1, 1), None), ((5, 207), 2), ((2, 256), None)]
    for shape, batch in shapes:
        for kind in KINDS:
            m, y = case(rng, kind, K, shape)
            for fair in (False, True):
                got = ensemble_scores(y, m, Q3, fair=fair, seed=K, batch_size=batch, return_fields=True)
                check_scores(got, m, y, Q3, fair=fair, seed=K, label=f'K={K} {shape} {kind} fair={fair}')
            if kind == 'relu' and shape[1] > 1:
                ref = R.score_ref(m, y, Q3, seed=K)
                assert (ref['equal'] > 0).mean() > 0.2, 'the ReLU-ed kind exercises ties'
                if K > 1:
                    assert (ref['rank'] != ref['below']).any(), 'tie draws other than 0 occur'


def test_invalid_elements_are_excluded_everywhere():
    from dl4ds_amd.metrics import ensemble_scores
    rng = np.random.default_rng(5)
    for K in (4, 20, 100):
        m, y = case(rng, 'normal', K, (6, 8, 9, 1))
        y[0, 0, 0, 0] = np.nan
        y[1, 1, 1, 0] = -np.inf
        m[K - 1, 2, 2, 2, 0] = np.nan
        m[0, 3, 3, 3, 0] = np.inf
        m[:, 4, 7, 8, 0] = np.nan
        mask = np.ones((8, 9))
        mask[5] = 0
        scale = np.full((8, 9, 1), 1.5, np.float32)
        scale[0, 1], scale[0, 2], scale[0, 3] = 0.0, -2.0, np.nan
        got = ensemble_scores(y, m, Q3, seed=9, mask=mask, batch_size=4, scale=scale, return_fields=True)
        ym = y.copy()
        ym[:, 5] = np.nan
        ref = R.score_ref(m, ym, Q3, seed=9, scale=scale)
        assert got['n_cells_excluded'] == 3 and got['n_valid'] == 6 * 72 - 6 * 9 - 6 * 3 - 5
        check_scores(got, m, ym, Q3, seed=9, scale=scale, label=f'K={K} invalid', ref=ref)
        assert np.isnan(got['crps_map'][5]).all() and np.isnan(got['crps_map'][0, 1:4]).all()
        assert np.isfinite(got['crps_map'][0, 0]) and got['n_valid_map'][0, 0, 0] == 5
        assert (got['rank_field'][:, 5] == -1).all() and got['rank_histogram'].sum() == got['n_valid']
        assert y[0, 5, 0, 0] == y[0, 5, 0, 0], 'the caller\'s observation was written'


def test_calls_are_reproducible_and_independent_of_the_batch_size():
    from dl4ds_amd.metrics import ensemble_scores
    rng = np.random.default_rng(6)
    for K in (7, 16, 40, 70):
        m, y = case(rng, 'relu', K, (11, 13, 10))
        y[3, 4, 5] = np.nan
        a = ensemble_scores(y, m, Q3, seed=4, batch_size=3, return_fields=True)
        b = ensemble_scores(y, m, Q3, seed=4, batch_size=3, return_fields=True)
        c = ensemble_scores(y, m, Q3, seed=4, batch_size=8, return_fields=True)
        d = ensemble_scores(y, m, Q3, seed=4, return_fields=True)
        for other in (b, c, d):
            assert set(other) == set(a)
            for k in a:
                assert np.asarray(a[k]).tobytes() == np.asarray(other[k]).tobytes(), (K, k)
        e = ensemble_scores(y, m, Q3, seed=5, return_fields=True)
        assert (e['rank_field'] != a['rank_field']).any() and e['crps_field'].tobytes() == a['crps_field'].tobytes()


def test_bad_arguments_are_errors():
    import ctypes
    import dl4ds_amd._lib as L
    from dl4ds_amd.device import DeviceArray
    lib = L.lib()
    m, y = DeviceArray.zeros((4, 12)), DeviceArray.zeros((12,))
    hist, cov, cell = DeviceArray.zeros((5,), np.uint64), DeviceArray.zeros((2,), np.uint64), DeviceArray.zeros((4, 4), np.float64)

    def call(K=4, n=12, stride=12, B=3, off=0, q=(0.5,), covered=True):
        qc = (ctypes.c_float * max(len(q), 1))(*q)
        return lib.dl4ds_ensemble_score(m.ptr, K, n, stride, y.ptr, B, off, None, 0, 0, qc, len(q), None, None, None, None, None,
                                        cell.ptr, hist.ptr, cov.ptr if covered else None)
    L.check(call())
    for kw in (dict(K=0), dict(K=257), dict(B=5), dict(B=0), dict(stride=8), dict(off=2), dict(q=(1.5,)), dict(q=(0.1,) * 33),
               dict(covered=False)):
        with pytest.raises(L.Dl4dsHipError):
            L.check(call(**kw))
    L.check(call(off=8))
    assert hist.numpy().sum() == 24


# ------------------------------------------------------------------------------------------------ through the model
LR, SCALE = (16, 20), 2
HR = (LR[0] * SCALE, LR[1] * SCALE)


def mc_model(variant='mcdrop', rate=0.3, seed=1, **kw):
    import dl4ds_amd.models as PM
    cfg = dict(n_filters=8, n_blocks=2, dropout_rate=rate, dropout_variant=variant, seed=seed)
    cfg.update(kw)
    return PM.net_postupsampling('resnet', 'spc', SCALE, 1, cfg.pop('n_aux', 0), LR, **cfg)


def fields(n, seed=0, grid=LR, c=1):
    return np.random.default_rng(seed).standard_normal((n,) + tuple(grid) + (c,)).astype(np.float32)


def same_scores(a, b):
    assert set(a) == set(b), set(a) ^ set(b)
    for k in a:
        assert np.asarray(a[k]).tobytes() == np.asarray(b[k]).tobytes(), k


def against_predict_ensemble(m, inputs, y, K, batch, seed, q=Q3, fair=False, label=''):
    """score_ensemble == predict_ensemble's statistics + ensemble_scores on its members (same seed and batch size): every score
    identical; and the scores agree with the restatement"""
    from dl4ds_amd.metrics import ensemble_scores
    res = m.score_ensemble(inputs, y, K, batch_size=batch, quantiles=q, seed=seed, fair=fair, return_fields=True)
    plain = m.predict_ensemble(inputs, K, batch_size=batch, quantiles=q, seed=seed, return_members=True)
    for k in ('mean', 'std', 'min', 'max', 'quantiles'):
        assert res[k].tobytes() == plain[k].tobytes(), k
    assert 'members' not in res
    host = ensemble_scores(y, plain['members'], q, fair=fair, seed=seed, batch_size=batch, return_fields=True)
    same_scores(res['scores'], host)
    check_scores(res['scores'], plain['members'], y, q, fair=fair, seed=seed, label=label)
    return res, plain


@pytest.mark.parametrize('variant', ['mcdrop', 'mcgaussiandrop', 'mcspatialdrop'])
def test_score_ensemble_is_predict_ensemble_plus_scores(variant):
    m = mc_model(variant)
    x = fields(7, 1)
    y = m.predict(x) + 0.05 * fields(7, 2, HR)
    res, _ = against_predict_ensemble(m, x, y, 6, 3, 77, fair=(variant == 'mcdrop'), label=f'{variant} N=7 batch=3')
    sc = res['scores']
    assert sc['crps_map'].shape == m.output_shape and sc['crps_per_sample'].shape == (7,) and sc['spread'] > 0
    assert sc['rank_histogram'].shape == (7,) and sc['rank_histogram'].sum() == sc['n_valid'] == y.size
    assert np.isclose(sc['spread_skill'], sc['spread'] / sc['rmse'], rtol=1e-15)


def test_model_without_mc_dropout_degenerates():
    m = mc_model(None, rate=0)
    x = fields(4, 3)
    p = m.predict(x)
    y = p + 0.1 * fields(4, 4, HR)
    y[0, :4] = p[0, :4]                                                    # observation == every member: rank is the tie draw
    with pytest.warns(UserWarning, match='mcdrop'):
        res = m.score_ensemble(x, y, 5, seed=3, return_fields=True)
    sc = res['scores']
    want = np.abs(p.astype(np.float64) - y)
    off = np.abs(sc['crps_field'] - want) / R.ulp32(want)
    print(f'identical members: CRPS against |x - y|: worst {off.max():.2f} ulp')
    assert (off <= 1).all(), 'CRPS of identical members is the absolute error'
    assert (sc['var_field'] == 0).all() and sc['spread'] == 0
    r = sc['rank_field']
    ties = y == p
    assert ((r[~ties] == 0) | (r[~ties] == 5)).all()
    g = np.flatnonzero(ties.reshape(-1))
    assert r.reshape(-1)[g].tolist() == [R.tie(3, int(i), 5) for i in g] and len(g) >= 4 * HR[1]


def test_two_inputs_and_another_grid():
    m = mc_model(n_aux=2)
    x = fields(3, 5)
    st = np.random.default_rng(6).standard_normal((3,) + tuple(m.input_shapes[1])).astype(np.float32)
    against_predict_ensemble(m, [x, st], fields(3, 7, HR), 4, 2, 5, label='two inputs')
    m = mc_model()
    grid = (12, 24)
    x = fields(3, 8, grid)
    y = fields(3, 9, (grid[0] * SCALE, grid[1] * SCALE))
    res, _ = against_predict_ensemble(m, x, y, 4, 32, 3, label='other grid')
    assert res['scores']['crps_map'].shape == (grid[0] * SCALE, grid[1] * SCALE, 1)
    with pytest.raises(ValueError, match='y_true'):
        m.score_ensemble(x, y[:, :-1], 4)


@pytest.mark.parametrize('kind', ['standard', 'minmax'])
def test_verify_ensemble_through_a_scaler(kind, tmp_path):
    """The observation is transformed into the model's units and the scaler's slope carries the scores back: they equal the scores
    of the inverse-transformed members against the physical observation.  Those members (and the transformed observation) are
    rounded to float32 at the field's magnitude, which the bounds of check_scores do not know about: CRPS moves by at most the
    perturbation of the observation plus twice that of the members (first term 1-Lipschitz in y and in the members, pair term
    bounded by the members' perturbation again), i.e. 4 ulp_fp32(max |value|) with every rounding at most one ulp; RMSE and
    spread likewise (both are 1-Lipschitz in a uniform perturbation of their inputs)."""
    import dl4ds_amd
    from dl4ds_amd.metrics import ensemble_scores
    from dl4ds_amd.preprocessing import MinMaxScaler, StandardScaler
    m = mc_model()
    rng = np.random.default_rng(12)
    kelvin = (281.0 + 12.0 * rng.standard_normal((5,) + HR + (1,))).astype(np.float32)
    sc = (StandardScaler(axis=None) if kind == 'standard' else MinMaxScaler(axis=None)).fit(kelvin)
    arr = np.asarray(sc.transform(kelvin), np.float32).reshape(kelvin.shape)
    mask = np.ones(HR)
    mask[:3] = 0
    kw = dict(quantiles=Q3, seed=21, batch_size=2, scaler=sc)
    res = dl4ds_amd.verify_ensemble(m, arr, SCALE, 6, y_true=kelvin, mask=mask, save_path=str(tmp_path), **kw)
    ens = dl4ds_amd.predict_ensemble(m, arr, SCALE, 6, return_members=True, **kw)
    for k in ('mean', 'std', 'min', 'max', 'quantiles'):
        assert res[k].tobytes() == ens[k].tobytes(), k
    got = res['scores']
    members = ens['members'].reshape((6,) + kelvin.shape)                   # (the scalers drop size-1 axes)
    host = ensemble_scores(kelvin, members, Q3, seed=21, mask=mask)
    tol = 4 * float(np.spacing(np.float32(np.abs(members).max())))
    print(f'{kind}: crps {got["crps"]:.6f} vs {host["crps"]:.6f}, spread {got["spread"]:.6f} vs {host["spread"]:.6f}, tol {tol:.2e}')
    assert got['n_valid'] == host['n_valid'] == 5 * (HR[0] - 3) * HR[1] and got['n_cells_excluded'] == 0
    for k in ('crps', 'spread', 'rmse'):
        assert abs(got[k] - host[k]) <= tol, (k, got[k], host[k])
        assert np.nanmax(np.abs(got[k + '_map'] - host[k + '_map'])) <= tol, k
    assert np.isnan(got['crps_map'][:3]).all()
    # ranks do not change under an increasing affine map, except where a member lies within a rounding (3e-5 K) of the observation:
    # about 5e-6 per (element, member) for differences spread over kelvins, 0.2 expected among 6 x 5800, each moving two bins
    assert np.abs(got['rank_histogram'] - host['rank_histogram']).sum() <= 4
    # the same plumbing (transform of the observation, the scaler's slope as scale) with the tight bounds: the members in the
    # model's units against the test's own transform of the observation, scaled by the slope
    raw = dl4ds_amd.predict_ensemble(m, arr, SCALE, 6, return_members=True, quantiles=Q3, seed=21, batch_size=2)['members']
    y_model = arr.copy()
    y_model[:, :3] = np.nan
    two = (2,) + kelvin.shape[1:]
    slope = (np.asarray(sc.inverse_transform(np.ones(two)), np.float64) - np.asarray(sc.inverse_transform(np.zeros(two)), np.float64))
    slope = np.full(kelvin.shape[1:], np.float32(slope.reshape(-1)[0]))
    check_scores(got, raw, y_model, Q3, seed=21, scale=slope, label=f'{kind} scaler, model units', fields=False)
    saved = np.load(tmp_path / 'y_hat_ensemble_scores.npz')
    assert set(saved.files) == {k for k in res if k != 'scores'} | {'scores_' + k for k in got}
    assert saved['scores_rank_histogram'].tobytes() == got['rank_histogram'].tobytes() and saved['mean'].tobytes() == res['mean'].tobytes()


@pytest.mark.parametrize('kind', ['standard', 'minmax'])
def test_nan_observations_stay_invalid_through_a_scaler(kind):
    """The scalers' transform fills NaN with a finite value: the observation's gaps must be invalid all the same, and the caller's
    array must not be written, not even by a scaler built with copy=False."""
    import dl4ds_amd
    from dl4ds_amd.preprocessing import MinMaxScaler, StandardScaler
    Scaler = StandardScaler if kind == 'standard' else MinMaxScaler
    m = mc_model()
    rng = np.random.default_rng(15)
    kelvin = (281.0 + 12.0 * rng.standard_normal((5,) + HR + (1,))).astype(np.float32)
    arr = np.asarray(Scaler(axis=None).fit(kelvin).transform(kelvin), np.float32).reshape(kelvin.shape)
    y = kelvin.copy()
    y[0, 4:7, 5:9] = np.nan
    y[:, 10, 11] = np.nan                                                  # a cell that is missing in every sample
    y[3, 20, 2] = np.inf
    before = y.copy()
    bad = ~np.isfinite(y)
    full = dl4ds_amd.verify_ensemble(m, arr, SCALE, 5, y_true=kelvin, scaler=Scaler(axis=None).fit(kelvin), quantiles=[0.5], seed=3)
    for copy in (True, False):
        sc = Scaler(axis=None, copy=copy).fit(kelvin.copy())
        got = dl4ds_amd.verify_ensemble(m, arr, SCALE, 5, y_true=y, scaler=sc, quantiles=[0.5], seed=3)['scores']
        assert y.tobytes() == before.tobytes(), 'the caller\'s observation was written'
        assert got['n_valid'] == y.size - int(bad.sum()) == 5 * HR[0] * HR[1] - 12 - 5 - 1
        np.testing.assert_array_equal(got['n_valid_map'], (~bad).sum(axis=0))
        np.testing.assert_array_equal(got['n_valid_per_sample'], (~bad).reshape(5, -1).sum(axis=1))
        assert got['rank_histogram'].sum() == got['n_valid']
        for k in ('crps_map', 'rmse_map', 'spread_map'):
            np.testing.assert_array_equal(np.isnan(got[k]), bad.all(axis=0), err_msg=k)
            assert np.isnan(got[k][10, 11, 0]) and np.isfinite(got[k][5, 6, 0])
        # cells without a gap score exactly as with the complete observation (same seed: same members)
        whole = ~bad.any(axis=0)
        assert (got['crps_map'][whole] == full['scores']['crps_map'][whole]).all()


def test_verify_ensemble_defaults_to_the_hr_array_and_mirrors_predict_ensemble():
    import dl4ds_amd
    m = mc_model()
    arr = fields(5, 14, HR)
    res, lr = dl4ds_amd.verify_ensemble(m, arr, SCALE, 5, quantiles=[0.5], seed=8, batch_size=4, return_lr=True)
    ens = dl4ds_amd.predict_ensemble(m, arr, SCALE, 5, quantiles=[0.5], seed=8, batch_size=4, return_members=True)
    assert res['mean'].tobytes() == ens['mean'].tobytes() and lr.shape == (5,) + LR + (1,)
    again = dl4ds_amd.EnsembleVerifier(m, arr, SCALE, 5, quantiles=[0.5], seed=8, batch_size=4, array_in_hr=True).run()
    same_scores(res['scores'], again['scores'])
    ref = R.score_ref(ens['members'], arr, [0.5], seed=8)
    s = R.summary(ref, 5)
    np.testing.assert_array_equal(res['scores']['rank_histogram'], s['rank_histogram'])
    np.testing.assert_allclose(res['scores']['crps'], s['crps'], rtol=2.0**-21)
    with pytest.raises(ValueError, match='time_window'):
        dl4ds_amd.verify_ensemble(m, arr, SCALE, 5, time_window=2)
    with warnings.catch_warnings():
        warnings.simplefilter('error')
        dl4ds_amd.verify_ensemble(m, arr[:2], SCALE, 3)


def test_stack_that_does_not_fit_is_a_memory_error():
    import dl4ds_amd.models as PM
    m = PM.net_postupsampling('resnet', 'spc', 4, 1, 0, (128, 128), n_filters=8, n_blocks=1, dropout_rate=0.2,
                              dropout_variant='mcdrop', seed=1)
    x = np.zeros((1200, 128, 128, 1), np.float32)                           # (untouched zero pages: no host memory is committed)
    y = np.zeros((1200, 512, 512, 1), np.float32)
    with pytest.raises(MemoryError, match='batch_size'):                    # 256 x 1200 x 512^2 x 4 B = 300 GiB
        m.score_ensemble(x, y, 256, batch_size=1200)
    res = m.score_ensemble(x[:2], y[:2], 3, seed=1)                         # the refused allocation is over with the exception
    assert np.isfinite(res['scores']['crps']) and res['scores']['n_valid'] == 2 * 512 * 512
