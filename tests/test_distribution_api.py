"""CPU-side checks of the distribution verification (dl4ds_amd.metrics.distribution_scores / quantile_maps, csrc/distribution.hip):
the numpy restatement tests/distribution_ref.py against np.quantile, scipy.stats and np.histogram on tie-heavy samples and against
answers worked by hand, the host arithmetic of the product on hand-made device outputs, the argument validation (no library
call), the exports and the C declaration."""
import inspect
import os

import numpy as np
import pytest

from tests import distribution_ref as ref
from tests.distribution_cases import CASES, MAX_E, MAX_Q, precip

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
Q9 = np.array([0.0, 0.01, 0.05, 0.25, 0.5, 0.75, 0.95, 0.99, 1.0])
EDGES = np.array([0.0, 0.1, 1.0, 2.0, 5.0, 10.0, 20.0, 50.0], np.float32)


def _tie_heavy_samples():
    """300 pairs: precipitation-like with 60 % zeros, integer-rounded normals, n from 1 upward"""
    rng = np.random.default_rng(2024)
    sizes = list(range(1, 41)) + [int(v) for v in rng.integers(41, 401, 260)]
    for i, n in enumerate(sizes):
        if i % 2:
            yield precip(rng, n), precip(rng, n)
        else:
            yield (np.round(3.0 * rng.standard_normal(n)).astype(np.float32) + np.float32(0.0),
                   np.round(3.0 * rng.standard_normal(n) + 1.0).astype(np.float32) + np.float32(0.0))


def test_restatement_against_numpy_and_scipy():
    """KS * n and the histograms agree exactly; quantiles within 2^-50 * max(|x_j|, |x_j+1|) (np.quantile interpolates from the
    upper neighbour when g >= 0.5: other roundings of the same magnitude); W1 within n * 2^-52 relative (non-negative terms: any
    summation order is within (n - 1) * 2^-53 of the exact sum)"""
    stats = pytest.importorskip('scipy.stats')
    count = 0
    for y, p in _tie_heavy_samples():
        n = len(y)
        quant, w1, ks, hist, nv, qmag = ref.segment_scores(y, p, Q9, EDGES)
        assert nv == n and np.isfinite(quant).all() and np.isfinite(w1)
        for side, x in enumerate((y, p)):
            want = np.quantile(x.astype(np.float64), Q9, method='linear')
            assert (np.abs(quant[side] - want) <= 2.0 ** -50 * qmag[side]).all(), (n, side)
            np.testing.assert_array_equal(hist[side], np.histogram(x, bins=EDGES)[0])
        want_w1 = stats.wasserstein_distance(y.astype(np.float64), p.astype(np.float64))
        assert abs(w1 - want_w1) <= n * 2.0 ** -52 * abs(want_w1), n
        d = stats.ks_2samp(y, p).statistic
        assert ks == round(d * n) and abs(ks / n - d) <= 1e-12, n
        count += 1
    assert count == 300


def _seg(y, p, q=(0.0, 0.5, 1.0), edges=None):
    return ref.segment_scores(np.asarray(y, np.float32), np.asarray(p, np.float32), q, edges)


def test_identical_disjoint_and_constant_samples_by_hand():
    """Identical samples: W1 = 0, KS = 0.  Disjoint samples a = 0..4, b = 10..14: every a lies below every b, so at v = 4 the
    counts are 5 against 0: KS * n = 5 = n; W1 = the shift 10.  A constant sample against itself shifted by 1: all quantiles equal
    the constant, W1 = 1, KS * n = n."""
    a = np.arange(5.0)
    quant, w1, ks, _, n, _ = _seg(a[::-1], a)
    assert (w1, ks, n) == (0.0, 0, 5) and quant.tolist() == [[0.0, 2.0, 4.0]] * 2
    quant, w1, ks, _, n, _ = _seg(a, a + 10.0)
    assert (w1, ks, n) == (10.0, 5, 5) and quant[1].tolist() == [10.0, 12.0, 14.0]
    quant, w1, ks, _, n, _ = _seg(np.full(7, 3.0), np.full(7, 4.0))
    assert (w1, ks, n) == (1.0, 7, 7) and quant.tolist() == [[3.0] * 3, [4.0] * 3]


def test_quantile_formula_by_hand():
    """x = 1, 2, 4, 8 (n = 4): q = 0.5: h = 1.5, j = 1, g = 0.5: 2 + (4 - 2) * 0.5 = 3.  q = 0.25: h = 0.75, j = 0: 1 + 1 * 0.75 =
    1.75.  q = 0 and q = 1 are the minimum and the maximum (j = n - 1, the upper neighbour clamped).  n = 1: every quantile is the
    value.  KS of (1, 2, 4, 8) against (2, 2, 8, 9): at v = 1: 1 - 0; v = 2: 2 - 2; v = 4: 3 - 2; v = 8: 4 - 3; v = 9: 0: KS * n = 1;
    W1 = (1 + 0 + 4 + 1) / 4 = 1.5."""
    quant, w1, ks, _, n, _ = _seg([8, 1, 4, 2], [9, 2, 8, 2], q=(0.5, 0.25, 0.0, 1.0))
    assert quant[0].tolist() == [3.0, 1.75, 1.0, 8.0] and quant[1].tolist() == [5.0, 2.0, 2.0, 9.0]
    assert (w1, ks, n) == (1.5, 1, 4)
    quant, w1, ks, _, n, _ = _seg([5.0], [7.0], q=(0.0, 0.3, 1.0))
    assert quant.tolist() == [[5.0] * 3, [7.0] * 3] and (w1, ks, n) == (2.0, 1, 1)


def test_invalid_elements_leave_both_sides():
    """y = (1, NaN, 3, 4), p = (2, 5, Inf, 6): the elements 1 and 2 are invalid: a = (1, 4), b = (2, 6)"""
    quant, w1, ks, hist, n, _ = _seg([1, np.nan, 3, 4], [2, 5, np.inf, 6], q=(0.0, 1.0), edges=(0.0, 3.5, 7.0))
    assert n == 2 and quant.tolist() == [[1.0, 4.0], [2.0, 6.0]] and w1 == 1.5 and ks == 1
    assert hist.tolist() == [[1, 1], [1, 1]]
    quant, w1, ks, hist, n, _ = _seg([np.nan, 1.0], [1.0, -np.inf], edges=(0.0, 1.0))
    assert n == 0 and np.isnan(quant).all() and np.isnan(w1) and ks == 0 and hist.tolist() == [[0], [0]]


def test_bin_edges_by_hand():
    """Edges 0, 1, 2: a value equal to an inner edge (1.0) goes to the bin it opens, the last edge (2.0) closes the last bin, values
    outside (-0.5, 2.5) are counted nowhere; -0.0 is 0.0 and lands in the first bin."""
    y = [-0.5, -0.0, 0.0, 0.5, 1.0, 1.0, 1.5, 2.0, 2.5]
    _, _, _, hist, n, _ = _seg(y, y, edges=(0.0, 1.0, 2.0))
    assert n == 9 and hist[0].tolist() == [3, 4] and hist[0].tolist() == np.histogram(y, bins=[0.0, 1.0, 2.0])[0].tolist()


def test_dict_of_the_restatement_and_perkins_by_hand():
    """two cells over four times.  Cell 0: obs (0, 0, 1, 3), pred (0, 1, 1, 1) on edges 0, 0.5, 2, 4: hist_obs = (2, 1, 1), hist_pred =
    (1, 3, 0): common = 1 + 1 + 0 = 2: Perkins 2/4.  Cell 1: masked: n = 0, NaN.  Pooled = cell 0."""
    y = np.array([[0, 9], [0, 9], [1, 9], [3, 9]], np.float32).reshape(4, 1, 2, 1)
    p = np.array([[0, 9], [1, 9], [1, 9], [1, 9]], np.float32).reshape(4, 1, 2, 1)
    r = ref.distribution_scores(y, p, (0.5,), bins=(0.0, 0.5, 2.0, 4.0), mask=np.array([[1, 0]]))
    assert r['n_valid'].tolist() == [[[4], [0]]] and r['hist_obs'][0, 0, 0].tolist() == [2, 1, 1]
    assert r['hist_pred'][0, 0, 0].tolist() == [1, 3, 0] and r['perkins'][0, 0, 0] == 0.5 and np.isnan(r['perkins'][0, 1, 0])
    assert r['perkins_pooled'] == 0.5 and r['hist_obs_pooled'].tolist() == [2, 1, 1]
    assert r['q_obs'][0, 0, 0, 0] == 0.5 and r['q_pred'][0, 0, 0, 0] == 1.0 and r['q_bias'][0, 0, 0, 0] == 0.5
    assert np.isnan(r['q_obs'][0, 1, 0, 0]) and np.isnan(r['ks'][0, 1, 0]) and r['ks_count'][0, 1, 0] == 0
    # KS: v = 0: 2 - 1; v = 1: 3 - 4; v = 3: 4 - 4: KS * n = 1.  W1 = (0 + 1 + 0 + 2) / 4
    assert r['ks_count'][0, 0, 0] == 1 and r['ks'][0, 0, 0] == 0.25 and r['wasserstein'][0, 0, 0] == 0.75
    s = ref.distribution_scores(y, p, (0.5,), bins=(0.0, 0.5, 2.0, 4.0), over='space')
    assert s['n_valid'].shape == (4,) and s['q_obs'].shape == (4, 1) and s['hist_obs'].shape == (4, 3)


def test_product_host_arithmetic_on_hand_outputs():
    """distribution_from_counts (what distribution_scores does with the device's outputs): ratios, NaN at n = 0, pooled sums beyond
    2^53 as Python integers"""
    from dl4ds_amd.metrics import distribution_from_counts
    quant = np.array([[[0.5], [1.0]], [[np.nan], [np.nan]]])
    hist = np.array([[[2, 1, 1], [1, 3, 0]], [[0, 0, 0], [0, 0, 0]]], np.int64)
    r = distribution_from_counts(quant, np.array([0.75, np.nan]), np.array([1, 0]), hist, np.array([4, 0]), (0.5,),
                                 np.array([0.0, 0.5, 2.0, 4.0], np.float32))
    assert r['q_bias'].tolist()[0] == [0.5] and np.isnan(r['q_bias'][1, 0])
    assert r['ks'][0] == 0.25 and np.isnan(r['ks'][1]) and r['perkins'][0] == 0.5 and np.isnan(r['perkins'][1])
    assert r['perkins_pooled'] == 0.5 and r['hist_obs_pooled'].tolist() == [2, 1, 1] and r['hist_pred_pooled'].tolist() == [1, 3, 0]
    assert r['n_valid'].dtype == np.int64 and r['ks_count'].dtype == np.int64 and r['hist_obs'].dtype == np.int64
    assert r['hist_obs_pooled'].dtype == np.int64 and r['q_obs'].dtype == np.float64 and r['bins'].dtype == np.float32
    assert r['quantiles'].dtype == np.float64 and isinstance(r['perkins_pooled'], np.float64)
    r = distribution_from_counts(quant, np.array([0.75, np.nan]), np.array([1, 0]), None, np.array([4, 0]), (0.5,), None)
    assert r['bins'] is None and 'hist_obs' not in r and 'perkins' not in r
    big = 2 ** 61                                                          # three segments of 2^61 values in one bin each
    hist = np.array([[[big, 0], [0, big]], [[big, 0], [big, 0]], [[0, big], [0, big]]], np.int64)
    r = distribution_from_counts(np.zeros((3, 2, 0)), np.zeros(3), np.zeros(3, np.int64), hist, np.full(3, big), (),
                                 np.array([0.0, 1.0, 2.0], np.float32))
    assert r['perkins'].tolist() == [0.0, 1.0, 1.0] and r['perkins_pooled'] == 2.0 / 3.0       # (min(2, 1) + min(1, 2)) / 3
    empty = distribution_from_counts(np.full((1, 2, 1), np.nan), [np.nan], [0], np.zeros((1, 2, 2), np.int64), [0], (0.5,),
                                     np.array([0.0, 1.0, 2.0], np.float32))
    assert np.isnan(empty['perkins_pooled']) and np.isnan(empty['ks'][0])


def _no_library(monkeypatch):
    import dl4ds_amd._lib as L

    def boom(*a, **k):
        raise AssertionError('the library was touched')
    monkeypatch.setattr(L, 'lib', boom)
    monkeypatch.setattr(L, 'load', boom)


@pytest.mark.parametrize('kw', [dict(quantiles=(-0.1,)), dict(quantiles=(0.5, 1.0 + 1e-12)), dict(quantiles=(np.nan,)),
                                dict(quantiles=((0.1, 0.2),)), dict(quantiles=np.linspace(0, 1, MAX_Q + 1)),
                                dict(bins=(1.0,)), dict(bins=()), dict(bins=(0.0, np.nan)), dict(bins=(0.0, np.inf)),
                                dict(bins=(1.0, 1.0)), dict(bins=(1.0, 0.5)), dict(bins=(0.3, 0.3 + 1e-12)), dict(bins=(0.0, 1e39)),
                                dict(bins=(-0.0, 0.0)), dict(bins=((0.0, 1.0),)), dict(bins=np.linspace(0, 1, MAX_E + 1)),
                                dict(bins=3), dict(over='pixels'), dict(over=None), dict(batch_size=0), dict(batch_size=1.5)])
def test_argument_validation_without_a_library_call(monkeypatch, kw):
    from dl4ds_amd.metrics import distribution_scores
    _no_library(monkeypatch)
    y = np.zeros((2, 6, 5, 1), np.float32)
    with pytest.raises(ValueError):
        distribution_scores(y, y, **kw)


def test_shape_validation_and_accepted_arguments_without_a_library_call(monkeypatch):
    from dl4ds_amd.metrics import check_distribution_args, distribution_scores, quantile_maps
    _no_library(monkeypatch)
    y = np.zeros((2, 6, 5, 1), np.float32)
    for a, b in [(y, y[:1]), (y, y[:, :, :4]), (y[0, 0, :, 0], y[0, 0, :, 0]), (y[:0], y[:0])]:
        with pytest.raises(ValueError):
            distribution_scores(a, b)
    with pytest.raises(ValueError):
        quantile_maps(y, y, (2.0,))
    with pytest.raises(ValueError, match='mask'):
        distribution_scores(y, y, mask=np.ones((3, 3)))
    with pytest.raises(ValueError, match=r'2\^31'):
        check_distribution_args((2 ** 31, 1, 1, 1), (0.5,))
    with pytest.raises(ValueError, match=r'2\^31'):
        check_distribution_args((1, 2 ** 16, 2 ** 15, 1), (0.5,), over='space')
    check_distribution_args((1, 2 ** 16, 2 ** 15, 1), (0.5,), over='time')
    q, e = check_distribution_args(y.shape, np.linspace(0, 1, MAX_Q), np.linspace(0, 1, MAX_E), 'space', 3)
    assert q.dtype == np.float64 and len(q) == MAX_Q and e.dtype == np.float32 and len(e) == MAX_E
    q, e = check_distribution_args(y.shape, 0.5, None)
    assert q.tolist() == [0.5] and e is None
    q, e = check_distribution_args(y.shape, (), (0.25, np.float64(0.3)))
    assert len(q) == 0 and e.tolist() == [0.25, float(np.float32(0.3))]


def test_exports_and_signatures():
    import dl4ds_amd as dds
    from dl4ds_amd import metrics
    assert dds.distribution_scores is metrics.distribution_scores and dds.quantile_maps is metrics.quantile_maps
    sig = inspect.signature(metrics.distribution_scores)
    assert list(sig.parameters) == ['y_test', 'y_test_hat', 'quantiles', 'bins', 'over', 'scaler', 'mask', 'batch_size']
    assert sig.parameters['quantiles'].default == (0.01, 0.05, 0.25, 0.5, 0.75, 0.95, 0.99)
    assert sig.parameters['over'].default == 'time'
    assert all(sig.parameters[k].default is None for k in ('bins', 'scaler', 'mask', 'batch_size'))
    sig = inspect.signature(metrics.quantile_maps)
    assert list(sig.parameters) == ['y', 'y_hat', 'quantiles', 'over', 'scaler', 'mask'] and sig.parameters['over'].default == 'time'


def test_c_entry_is_declared():
    import dl4ds_amd._lib as L
    protos = L.parse_header()
    assert 'dl4ds_distribution' in protos                     # tests/test_abi.py then checks that the library exports it
    assert len(protos['dl4ds_distribution'][1]) == 15
    assert os.path.exists(os.path.join(ROOT, 'dl4ds_amd', 'csrc', 'distribution.hip'))


@pytest.mark.parametrize('name', sorted(CASES))
def test_reference_is_finite_on_the_gpu_cases_except_by_construction(name):
    """the NaNs of the expected arrays of tests/test_gpu_distribution.py are exactly the segments built to have no valid element"""
    if name == 'workspace_chunks':
        c = CASES[name]()
        c['y'], c['p'] = c['y'][:, :2], c['p'][:, :2]         # (the property is per segment: two rows of it stand for all)
    else:
        c = CASES[name]()
    r = ref.distribution_scores(c['y'], c['p'], c['quantiles'], c['bins'], c['over'], c['mask'])
    empty = r['n_valid'] == 0
    assert int(empty.sum()) == c['empty']
    for k in ('wasserstein', 'ks') + (('perkins',) if c['bins'] is not None else ()):
        np.testing.assert_array_equal(np.isnan(r[k]), empty, err_msg=k)
        assert np.isfinite(r[k][~empty]).all(), k
    for k in ('q_obs', 'q_pred', 'q_bias'):
        np.testing.assert_array_equal(np.isnan(r[k]), np.broadcast_to(empty[..., None], r[k].shape), err_msg=k)
        assert np.isfinite(r[k][~empty]).all(), k
    assert (r['ks_count'][empty] == 0).all() and (r['ks_count'] <= r['n_valid']).all()
    if c['bins'] is not None:
        assert np.isfinite(r['perkins_pooled']) and (r['hist_obs'].sum(-1) <= r['n_valid']).all()
        assert (np.diff(np.asarray(c['bins'], np.float32)) > 0).all()
    q = np.asarray(c['quantiles'])
    assert ((q >= 0) & (q <= 1)).all()
