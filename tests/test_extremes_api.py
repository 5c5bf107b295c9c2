"""The host side of the extreme-value verification (dl4ds_amd/extremes.py) and the restatement the device is
held to (tests/extremes_ref.py), without a GPU: the restatement against scipy and hand-written series, the fits against analytic
L-moments and scipy's quantile functions, the argument checks."""
import math

import numpy as np
import pytest

from dl4ds_amd import extremes as ex
from tests import extremes_cases as cases
from tests import extremes_ref as ref


def rel(got, want):
    return abs(got - want) / abs(want)


# ------------------------------------------------------------------------------------------------------------ the restatement
def test_vectorised_restatement_has_the_bits_of_the_plain_one():
    for pattern in ('spoiled', 'ties', 'wide'):
        for sign in (1, -1):
            x = cases.sample(41, 9, pattern, seed=3)
            n, pwm = ref.pwm(x, sign)
            for c in range(x.shape[1]):
                nc, pc = ref.pwm_cell(x[:, c], sign)
                assert nc == n[c]
                np.testing.assert_array_equal(np.array(pc).view(np.uint64), pwm[:, c].view(np.uint64), err_msg=f'{pattern} {sign} {c}')


@pytest.mark.parametrize('n', [4, 5, 37, 512, 1000])
def test_restatement_against_scipy_lmoment(n):
    """absolute tolerance 64 * n * 2^-53 * max|x|: the worst-case rounding of an n-term fp64 sum times the largest L-moment
    coefficient, 30, rounded up"""
    stats = pytest.importorskip('scipy.stats')
    if not hasattr(stats, 'lmoment'):
        pytest.skip('scipy.stats.lmoment is missing')
    rng = np.random.default_rng(n)
    x = rng.gamma(2.0, 5.0, (n, 3)).astype(np.float32) + np.float32(0.5)
    assert (x > 0).all()
    _, pwm = ref.pwm(x)
    m = ex.lmoments_from_pwm(pwm)
    tol = 64 * n * 2.0 ** -53 * float(x.max())
    for c in range(3):
        want = stats.lmoment(x[:, c].astype(np.float64), order=[1, 2, 3, 4], standardize=False)
        got = [m['l1'][c], m['l2'][c], m['t3'][c] * m['l2'][c], m['t4'][c] * m['l2'][c]]
        for g, w in zip(got, want):
            assert abs(g - w) <= tol, (n, c, g, w, tol)


def test_pwm_edge_cases():
    x = np.array([[np.nan, 1.0, 2.0, 4.0, 7.0],
                  [np.nan, np.nan, 2.0, 1.0, 7.0],
                  [np.nan, np.nan, np.nan, 3.0, 7.0],
                  [np.nan, np.inf, -np.inf, np.nan, 7.0]], np.float32)
    n, pwm = ref.pwm(x)
    np.testing.assert_array_equal(n, [0, 1, 2, 3, 4])
    for c in range(5):
        for r in range(4):
            assert np.isnan(pwm[r, c]) == (n[c] <= r), (r, c)
    assert pwm[0, 3] == 8.0 / 3 and pwm[1, 3] == (0.5 * 3.0 + 1.0 * 4.0) / 3
    m = ex.lmoments_from_pwm(pwm)
    assert np.isnan(m['t3'][4]) and m['l2'][4] == 0 and m['l1'][4] == 7.0       # a constant sample: l2 = 0 -> NaN
    assert np.isnan(m['t3'][:3]).all() and np.isfinite(m['t3'][3])
    lower = ref.pwm(x, -1)[1]
    assert lower[0, 3] == -8.0 / 3 and lower[1, 3] == (0.5 * -3.0 + 1.0 * -1.0) / 3
    z = ref.pwm(np.array([[0.0], [-0.0]], np.float32), -1)[1]
    assert not np.signbit(z[:2]).any()


# ---------------------------------------------------------------------------------------------------------------- clusters
def clusters(values, thr=10.0, run=1, starts=None, sign=1):
    return ref.clusters_cell(np.asarray(values, np.float32), [0, len(values)] if starts is None else starts, np.float32(thr), sign, run)


def test_cluster_state_machine_on_hand_written_series():
    s = [0, 12, 15, 3, 11, 0, 0, 20, 0, 0, 0, 13]
    assert clusters(s, run=1) == [(15.0, 2), (11.0, 4), (20.0, 7), (13.0, 11)]          # the last sample is an exceedance
    assert clusters(s, run=2) == [(15.0, 2), (20.0, 7), (13.0, 11)]
    assert clusters(s, run=3) == [(20.0, 7), (13.0, 11)]
    assert clusters(s, run=4) == [(20.0, 7)]
    n = np.nan
    assert clusters([12, n, 15, 0, 11], run=3) == [(12.0, 0), (15.0, 2)]                # a NaN inside a cluster cuts it
    assert clusters([12, np.inf, 15], run=3) == [(12.0, 0), (15.0, 2)]
    assert clusters([0, 12, 15, 14, 0], run=2, starts=[0, 2, 5]) == [(12.0, 1), (15.0, 2)]   # a period boundary inside a cluster
    assert clusters([0, 12, 15, 14, 0], run=2, starts=[0, 4, 5]) == [(15.0, 2)]
    assert clusters([15, 12, 15, 0, 15], run=2) == [(15.0, 0)]                          # a tie at the peak: the first position
    assert clusters([10, 10, 10]) == [] and clusters([10, 10.5, 10]) == [(10.5, 1)]     # strictly above
    assert clusters([1, 2], thr=np.nan) is None
    assert clusters([5, -3, -4, 0, -1], thr=-2.0, sign=-1) == [(-4.0, 2)]               # the lower tail: below -2, the smallest
    assert clusters([0.0, -0.0, 1.0], thr=-1.0) == [(1.0, 2)]
    assert clusters([-0.0, -0.0], thr=-1.0) == [(0.0, 0)] and not math.copysign(1, clusters([-0.0], thr=-1.0)[0][0]) < 0
    count, peak, pos = ref.pot_peaks(np.array([s, s], np.float32).T, [0, 12], np.array([10.0, np.nan], np.float32), K=2)
    np.testing.assert_array_equal(count, [4, -1])
    np.testing.assert_array_equal(peak[:, 0], [15.0, 11.0])
    np.testing.assert_array_equal(pos, [[2, -1], [4, -1]])
    assert np.isnan(peak[:, 1]).all()


def test_block_maxima_restatement():
    x = np.array([[1.0, np.nan], [3.0, np.nan], [-0.0, 2.0], [-5.0, np.inf]], np.float32)
    got = ref.block_maxima(x, [0, 2, 4])
    np.testing.assert_array_equal(got, np.array([[3.0, np.nan], [0.0, 2.0]], np.float32))
    np.testing.assert_array_equal(ref.block_maxima(x, [0, 2, 4], -1), np.array([[1.0, np.nan], [-5.0, 2.0]], np.float32))
    assert np.isnan(ref.block_maxima(x, [0, 2, 4], min_valid=2)[1, 1])


# -------------------------------------------------------------------------------------------------------------------- fits
@pytest.mark.parametrize('shape', [-0.3, -0.15, 0.1, 0.3, 0.15])
def test_gev_from_analytic_lmoments(shape):
    loc, scale = 31.5, 7.25
    fit = ex.gev_from_lmoments(*cases.gev_lmoments(loc, scale, shape))
    assert fit['n_not_converged'] == 0
    assert rel(fit['location'], loc) < 1e-10 and rel(fit['scale'], scale) < 1e-10 and rel(fit['shape'], shape) < 1e-10


def test_gev_on_a_gumbel_and_on_fields():
    loc, scale = 31.5, 7.25
    l1, l2, t3 = loc + ex.EULER_GAMMA * scale, scale * math.log(2.0), math.log(9.0 / 8.0) / math.log(2.0)
    fit = ex.gev_from_lmoments(l1, l2, t3)
    assert fit['n_not_converged'] == 0 and abs(fit['shape']) < 1e-10
    assert rel(fit['location'], loc) < 1e-10 and rel(fit['scale'], scale) < 1e-10
    g = ex.gumbel_from_lmoments(l1, l2)
    assert rel(g['location'], loc) < 1e-14 and rel(g['scale'], scale) < 1e-14 and g['shape'] == 0
    shapes = np.array([[-0.3, 0.1], [0.3, -0.15]])
    lm = np.vectorize(lambda s: cases.gev_lmoments(2.0, 3.0, s))(shapes)
    l1f, l2f, t3f = (np.array(a) for a in lm)
    l2f[0, 1] = 0.0                                                              # a constant sample
    t3f[1, 0] = np.nan                                                           # too few values
    fit = ex.gev_from_lmoments(l1f, l2f, t3f)
    assert fit['shape'].shape == (2, 2) and fit['n_not_converged'] == 0
    assert np.isnan(fit['shape'][0, 1]) and np.isnan(fit['scale'][1, 0]) and np.isnan(fit['location'][0, 1])
    assert rel(fit['shape'][0, 0], -0.3) < 1e-10 and rel(fit['shape'][1, 1], -0.15) < 1e-10


def test_gpd_and_gumbel_closed_forms():
    # GPD excesses with scale a and Hosking's k: l1 = a / (1 + k), l2 = a / ((1 + k)(2 + k))
    for a, k in ((3.0, 0.2), (5.5, -0.25), (1.0, 0.0)):
        fit = ex.gpd_from_lmoments(a / (1 + k), a / ((1 + k) * (2 + k)))
        assert rel(fit['scale'], a) < 1e-13 and abs(fit['shape'] + k) < 1e-13
    assert np.isnan(ex.gpd_from_lmoments(1.0, 0.0)['shape']) and np.isnan(ex.gumbel_from_lmoments(1.0, -1.0)['scale'])
    # PWMs of peaks -> those of the excesses: b_r - u / (r + 1)
    pwm = np.array([[14.0], [9.0], [7.0], [6.0]])
    fit = ex.gpd_fit_from_pwm(pwm, np.array([12]), 10.0, 4)
    want = ex.gpd_from_lmoments(4.0, 2.0 * (9.0 - 5.0) - 4.0)
    assert fit['scale'][0] == want['scale'] and fit['shape'][0] == want['shape'] and fit['rate'][0] == 3.0 and fit['threshold'][0] == 10.0


def test_return_levels_against_closed_forms_and_scipy():
    stats = pytest.importorskip('scipy.stats')
    T = np.array([2.0, 5.0, 10.0, 20.0, 50.0, 1000.0])
    p = 1.0 - 1.0 / T
    for shape in (-0.3, 0.1, 0.3, 0.0):
        fit = {'kind': 'gev', 'location': np.array(30.0), 'scale': np.array(7.0), 'shape': np.array(shape)}
        got = ex.return_levels(fit, T)
        np.testing.assert_allclose(got, stats.genextreme.ppf(p, c=-shape, loc=30.0, scale=7.0), rtol=1e-12, atol=0)
        if shape:
            np.testing.assert_allclose(got, 30.0 + 7.0 * (1.0 - (-np.log(p)) ** -shape) / -shape, rtol=1e-12, atol=0)
    gum = {'kind': 'gumbel', 'location': np.array(30.0), 'scale': np.array(7.0), 'shape': np.array(0.0)}
    np.testing.assert_allclose(ex.return_levels(gum, T), 30.0 - 7.0 * np.log(-np.log(p)), rtol=1e-12, atol=0)
    np.testing.assert_allclose(ex.return_levels(gum, T), stats.gumbel_r.ppf(p, loc=30.0, scale=7.0), rtol=1e-12, atol=0)
    for shape in (-0.25, 0.2, 0.0):
        rate = 2.5
        fit = {'kind': 'gpd', 'threshold': np.array(10.0), 'scale': np.array(4.0), 'shape': np.array(shape), 'rate': np.array(rate)}
        got = ex.return_levels(fit, T)
        np.testing.assert_allclose(got, stats.genpareto.ppf(1.0 - 1.0 / (rate * T), c=shape, loc=10.0, scale=4.0), rtol=1e-12, atol=0)
        if shape:
            np.testing.assert_allclose(got, 10.0 + 4.0 / -shape * (1.0 - (rate * T) ** shape), rtol=1e-12, atol=0)
        else:
            np.testing.assert_allclose(got, 10.0 + 4.0 * np.log(rate * T), rtol=1e-12, atol=0)
        np.testing.assert_array_equal(ex.return_levels(fit, T, rate=1.0), ex.return_levels(dict(fit, rate=np.array(1.0)), T))
    # a field of cells, and the lower tail: the fit describes -x, the levels come back negated
    field = {'kind': 'gev', 'location': np.full((2, 3, 1), 30.0), 'scale': np.full((2, 3, 1), 7.0), 'shape': np.full((2, 3, 1), 0.1),
             'sign': -1}
    got = ex.return_levels(field, (5, 20))
    assert got.shape == (2, 2, 3, 1)
    np.testing.assert_array_equal(got[:, 0, 0, 0], -ex.return_levels(dict(field, sign=1), (5, 20))[:, 0, 0, 0])
    with pytest.raises(ValueError):
        ex.return_levels(gum, (1.0, 5.0))


# -------------------------------------------------------------------------------------------------------- argument checks
def test_public_names_and_check_extreme_args():
    import dl4ds_amd
    for name in ('l_moments', 'block_maxima', 'peaks_over_threshold', 'lmoments_from_pwm', 'gev_from_lmoments', 'gumbel_from_lmoments',
                 'gpd_from_lmoments', 'return_levels', 'fit_gev', 'fit_gumbel', 'fit_gpd', 'extreme_scores', 'check_extreme_args'):
        assert getattr(dl4ds_amd, name) is getattr(ex, name)
    shape = (40, 9, 11, 2)
    sign, thr, T = ex.check_extreme_args(shape)
    assert sign == 1 and thr is None and T.tolist() == [5.0, 10.0, 20.0, 50.0]
    sign, thr, _ = ex.check_extreme_args(shape, 'lower', 32, (2,), 'pot', 10)
    assert sign == -1 and thr.dtype == np.float32 and thr.shape == (1,)
    assert ex.check_extreme_args(shape, threshold=np.zeros(shape[1:]))[1].shape == shape[1:]
    assert ex.check_extreme_args(shape, threshold=np.zeros((1,) + shape[1:]))[1].shape == shape[1:]
    assert ex.check_extreme_args((40, 9, 11, 1), threshold=np.zeros((9, 11)))[1].shape == (9, 11, 1)
    bad = [dict(tail='both'), dict(tail=None), dict(run=0), dict(run=33), dict(run=1.0), dict(run=True),
           dict(return_periods=(1.0, 5.0)), dict(return_periods=(0.5,)), dict(return_periods=()), dict(return_periods=(np.nan,)),
           dict(return_periods='often'), dict(method='mle'), dict(method='pot'), dict(method='pot', threshold=None),
           dict(threshold=np.zeros((9, 11))), dict(threshold=np.zeros((9, 11, 3))), dict(threshold=np.zeros((2, 9, 11, 2))),
           dict(threshold='high'), dict(batch_size=0)]
    for kw in bad:
        with pytest.raises(ValueError):
            ex.check_extreme_args(shape, **kw)
    with pytest.raises(ValueError):
        ex.check_extreme_args((40, 9, 11))
    # the device-backed functions refuse before any device call (no GPU here)
    x = np.zeros(shape, np.float32)
    for call in (lambda: ex.l_moments(x, tail='both'), lambda: ex.block_maxima(x, tail='both'),
                 lambda: ex.block_maxima(x, min_valid=0), lambda: ex.peaks_over_threshold(x, 1.0, run=0),
                 lambda: ex.peaks_over_threshold(x, np.zeros((3, 3, 3))), lambda: ex.extreme_scores(x, x, method='pot'),
                 lambda: ex.extreme_scores(x, x[:, :3]), lambda: ex.extreme_scores(x, x, return_periods=(1,)),
                 lambda: ex.fit_gpd(x, 1.0, 0)):
        with pytest.raises(ValueError):
            call()
