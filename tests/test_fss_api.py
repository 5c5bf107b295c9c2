"""CPU-side checks of the neighbourhood verification (dl4ds_amd.metrics.neighbourhood_scores / fss, csrc/fss.hip): the numpy
restatement tests/fss_ref.py against scipy.ndimage.uniform_filter and against answers worked by hand, the host arithmetic of the
product on hand-made counts, the argument validation (no library call), the exports and the C declaration."""
import inspect
import os

import numpy as np
import pytest

from tests import fss_ref
from tests.fss_cases import CASES

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize('shape', [(65, 63), (9, 8), (1, 40), (40, 1), (17, 30)])
def test_window_counts_match_uniform_filter(shape):
    """odd, even and larger-than-field windows on non-square fields: window_counts == uniform_filter(mode='constant') * n^2"""
    ndimage = pytest.importorskip('scipy.ndimage')
    b = (np.random.default_rng(sum(shape)).random(shape) > 0.6)
    for n in (1, 2, 3, 4, 5, 8, 9, 17, 64, 65, 129):
        want = ndimage.uniform_filter(b.astype(np.float64), size=n, mode='constant', cval=0.0) * n * n
        got = fss_ref.window_counts(b, n)
        assert got.dtype == np.int64
        assert np.abs(got - want).max() <= 1e-9 * n * n, n


def test_window_counts_by_brute_force():
    b = np.random.default_rng(3).random((7, 6)) > 0.5
    for n in (1, 2, 3, 4, 6, 7, 8, 20):
        for i in range(7):
            for j in range(6):
                r0, c0 = max(i - n // 2, 0), max(j - n // 2, 0)
                assert fss_ref.window_counts(b, n)[i, j] == b[r0:max(i - n // 2 + n, 0), c0:max(j - n // 2 + n, 0)].sum()


def _single(h, w, cells):
    a = np.zeros((1, h, w, 1), np.float32)
    for i, j in cells:
        a[0, i, j, 0] = 1.0
    return a


def test_displaced_event_by_hand():
    """One observed event at (10, 10), one forecast event at (10, 13): displacement d = 3 on a 21 x 21 field, threshold 0.5.

    n = 1: co and cf are the indicators.  D = 1 + 1, F = 1, O = 1: FSS = 1 - 2/2 = 0.
    n = 3: the window of (i, j) is rows i-1 .. i+1, columns j-1 .. j+1; a cell sees the observed event iff |i-10| <= 1 and
      |j-10| <= 1 (9 cells), the forecast one iff |j-13| <= 1 (9 cells), never both (columns 9-11 against 12-14): D = 18, F = O = 9,
      FSS = 0.  The same for n = 2 (columns j-1 .. j: 10-11 against 13-14) and n = 4 (columns j-2 .. j+1: the observed event is
      seen from j = 9 .. 12, the forecast one from j = 12 .. 15: column 12 sees BOTH): n = 4 is the first window that contains both.
      There co, cf in {0, 1}: 16 cells each (4 rows x 4 columns), 4 of them shared (column 12, 4 rows): D = 12 + 12 = 24,
      F = O = 16, FSS = 1 - 24/32 = 0.25.
    n = 5: columns j-2 .. j+2: observed from j = 8 .. 12, forecast from j = 11 .. 15, shared j = 11, 12 over 5 rows = 10 cells of
      25 each: D = 30, F = O = 25, FSS = 1 - 30/50 = 0.4."""
    y, p = _single(21, 21, [(10, 10)]), _single(21, 21, [(10, 13)])
    r = fss_ref.neighbourhood_scores(y, p, (0.5,), (1, 2, 3, 4, 5))
    assert r['sums'][0, 0, 0].tolist() == [[2, 1, 1], [8, 4, 4], [18, 9, 9], [24, 16, 16], [30, 25, 25]]
    assert r['fss'][0, 0, 0].tolist() == [0.0, 0.0, 0.0, 0.25, 0.4]
    assert r['fss_pooled'][0].tolist() == [0.0, 0.0, 0.0, 0.25, 0.4]
    # base rate 1/441: useful = 0.5 + 1/882 is not reached by 0.4
    assert r['useful_window'].tolist() == [-1]
    assert (r['hits'][0, 0, 0], r['misses'][0, 0, 0], r['false_alarms'][0, 0, 0], r['correct_negatives'][0, 0, 0]) == (0, 1, 1, 439)


def test_perfect_all_and_no_event_by_hand():
    """A perfect forecast has cf == co: D = 0 and FSS exactly 1 at every window.  An all-event 4 x 5 field at n = 3 has the counts
    (rows 2 3 3 2) x (columns 2 3 3 3 2) = row sum 13, column sum 10: F = O = (4+9+9+4) * (4+9+9+9+4) = 26 * 35 = 910.  A field
    without events has F + O = 0: NaN."""
    rng = np.random.default_rng(0)
    y = rng.random((2, 12, 10, 1)).astype(np.float32)
    r = fss_ref.neighbourhood_scores(y, y.copy(), (0.3, 0.6), (1, 2, 5, 40))
    assert (r['sums'][..., 0] == 0).all() and (r['sums'][..., 1] == r['sums'][..., 2]).all() and (r['sums'][..., 1] > 0).all()
    assert (r['fss'] == 1.0).all() and (r['fss_pooled'] == 1.0).all() and (r['fss_pooled_per_channel'] == 1.0).all()
    assert r['useful_window'].tolist() == [1, 1]
    ones = np.ones((1, 4, 5, 1), np.float32)
    r = fss_ref.neighbourhood_scores(ones, ones, (0.5, 2.0), (3,))
    assert r['sums'][0, 0, 0, 0].tolist() == [0, 910, 910] and r['fss'][0, 0, 0, 0] == 1.0
    assert r['sums'][0, 0, 1, 0].tolist() == [0, 0, 0] and np.isnan(r['fss'][0, 0, 1, 0]) and np.isnan(r['fss_pooled'][1, 0])
    assert r['hits'][0, 0].tolist() == [20, 0] and r['correct_negatives'][0, 0].tolist() == [0, 20]
    assert r['useful_window'].tolist() == [3, -1] and r['base_rate'].tolist() == [1.0, 0.0]
    for k in ('pod', 'far', 'csi', 'bias', 'ets'):            # threshold 2.0: every denominator is zero; ETS at 0.5: 20 - 20 = 0
        assert np.isnan(r[k][0, 0, 1]), k
    assert r['pod'][0, 0, 0] == 1.0 and r['far'][0, 0, 0] == 0.0 and r['bias'][0, 0, 0] == 1.0 and np.isnan(r['ets'][0, 0, 0])


HAND = dict(hits=3, misses=1, false_alarms=2, correct_negatives=6)


def _hand_fields():
    """12 valid cells (3 x 4) + 0 invalid: 3 hits, 1 miss, 2 false alarms, 6 correct negatives"""
    y = np.array([[1, 1, 1, 1], [0, 0, 0, 0], [0, 0, 0, 0]], np.float32).reshape(1, 3, 4, 1)
    p = np.array([[1, 1, 1, 0], [1, 1, 0, 0], [0, 0, 0, 0]], np.float32).reshape(1, 3, 4, 1)
    return y, p


def _check_hand_scores(r, sfx=''):
    """a = 3 hits, c = 1 miss, b = 2 false alarms, d = 6, n = 12: POD = a/(a+c) = 3/4, FAR = b/(a+b) = 2/5, CSI = a/(a+b+c) =
    3/6, bias = (a+b)/(a+c) = 5/4, hits_random = (a+c)(a+b)/n = 4*5/12 = 5/3, ETS = (3 - 5/3)/(6 - 5/3) = (4/3)/(13/3) = 4/13"""
    want = dict(pod=0.75, far=0.4, csi=0.5, bias=1.25, ets=4.0 / 13.0)
    for k, v in want.items():
        assert abs(float(np.ravel(r[k + sfx])[0]) - v) <= 1e-15, (k, r[k + sfx])


def test_contingency_by_hand():
    y, p = _hand_fields()
    r = fss_ref.neighbourhood_scores(y, p, (0.5,), (1,))
    for k, v in HAND.items():
        assert r[k][0, 0, 0] == v
    assert r['n_valid'][0, 0] == 12 and r['base_rate'][0] == 4 / 12 and r['fss_useful'][0] == 0.5 + 2 / 12
    _check_hand_scores(r)
    _check_hand_scores(r, '_pooled')
    y[0, 2, 3, 0] = np.nan                                   # an invalid cell leaves the table: one correct negative fewer
    p[0, 2, 2, 0] = np.inf
    r = fss_ref.neighbourhood_scores(y, p, (0.5,), (1,))
    assert r['n_valid'][0, 0] == 10 and r['correct_negatives'][0, 0, 0] == 4 and r['hits'][0, 0, 0] == 3
    r = fss_ref.neighbourhood_scores(*_hand_fields(), (0.5,), (1,), mask=np.array([[0, 1, 1, 1]] * 3))
    assert (r['hits'][0, 0, 0], r['misses'][0, 0, 0], r['false_alarms'][0, 0, 0], r['n_valid'][0, 0]) == (2, 1, 1, 9)


def test_product_host_arithmetic_on_hand_counts():
    """scores_from_counts (what neighbourhood_scores does with the device's integers) on the two hand-worked examples, and pooled
    sums beyond int64"""
    from dl4ds_amd.metrics import scores_from_counts
    sums = np.array([[2, 1, 1], [8, 4, 4], [18, 9, 9], [24, 16, 16], [30, 25, 25]], np.int64).reshape(1, 1, 1, 5, 3)
    cont = np.array([3, 1, 2, 6], np.int64).reshape(1, 1, 1, 4)
    r = scores_from_counts(sums, cont, np.array([[12]]), (0.5,), (1, 2, 3, 4, 5))
    assert r['fss'][0, 0, 0].tolist() == [0.0, 0.0, 0.0, 0.25, 0.4] and r['fss_pooled'][0].tolist() == [0.0, 0.0, 0.0, 0.25, 0.4]
    assert r['fss'].dtype == np.float64 and r['sums'].dtype == np.int64 and r['thresholds'].dtype == np.float32
    _check_hand_scores(r)
    _check_hand_scores(r, '_pooled')
    assert r['base_rate'][0] == 4 / 12 and r['fss_random'][0] == 4 / 12 and r['fss_useful'][0] == 0.5 + 2 / 12
    assert r['useful_window'].tolist() == [-1]
    big = 2 ** 61
    sums = np.array([[[[[big, big, big]]]], [[[[0, big, big]]]], [[[[0, big, big]]]]], np.int64)          # (3, 1, 1, 1, 3)
    r = scores_from_counts(sums, np.zeros((3, 1, 1, 4), np.int64), np.zeros((3, 1), np.int64), (0.0,), (1,))
    assert r['fss_pooled'][0, 0] == 1.0 - 1.0 / 6.0 and r['fss_pooled_per_channel'][0, 0, 0] == 1.0 - 1.0 / 6.0
    assert r['fss'][:, 0, 0, 0].tolist() == [0.5, 1.0, 1.0] and np.isnan(r['pod']).all() and np.isnan(r['base_rate']).all()


def _no_library(monkeypatch):
    import dl4ds_amd._lib as L

    def boom(*a, **k):
        raise AssertionError('the library was touched')
    monkeypatch.setattr(L, 'lib', boom)
    monkeypatch.setattr(L, 'load', boom)


@pytest.mark.parametrize('kw', [dict(thresholds=()), dict(thresholds=(0.0, np.nan)), dict(thresholds=(0.0, np.inf)),
                                dict(thresholds=(1.0, 1.0)), dict(thresholds=(1.0, 0.5)), dict(thresholds=(0.3, 0.3 + 1e-12)),
                                dict(thresholds=(1e39,)), dict(thresholds=((0.0, 1.0),)),
                                dict(windows=()), dict(windows=(0, 3)), dict(windows=(-1,)), dict(windows=(3, 3)),
                                dict(windows=(5, 3)), dict(windows=(1.5,)), dict(windows=(3.0,)), dict(windows=(True,)),
                                dict(windows=(2 ** 31,)), dict(batch_size=0), dict(batch_size=1.5)])
def test_argument_validation_without_a_library_call(monkeypatch, kw):
    from dl4ds_amd.metrics import neighbourhood_scores
    _no_library(monkeypatch)
    y = np.zeros((2, 6, 5, 1), np.float32)
    args = dict(thresholds=(0.0, 1.0), windows=(1, 3))
    args.update(kw)
    with pytest.raises(ValueError):
        neighbourhood_scores(y, y, **args)


def test_shape_validation_without_a_library_call(monkeypatch):
    from dl4ds_amd.metrics import neighbourhood_scores, fss
    _no_library(monkeypatch)
    y = np.zeros((2, 6, 5, 1), np.float32)
    for a, b in [(y, y[:1]), (y, y[:, :, :4]), (y[0, 0, :, 0], y[0, 0, :, 0]), (y[:0], y[:0])]:
        with pytest.raises(ValueError):
            neighbourhood_scores(a, b, (0.0,))
    with pytest.raises(ValueError):
        fss(y, y, ())
    with pytest.raises(ValueError, match='mask'):
        neighbourhood_scores(y, y, (0.0,), mask=np.ones((3, 3)))


def test_overflow_rule_without_a_library_call(monkeypatch):
    """H*W*m^2 >= 2^62 with m = min(n, H)*min(n, W) is refused: on 1500 x 1500 cells a window of 1100 gives 2.25e6 * (1.21e6)^2 =
    3.3e18 < 2^62 = 4.6e18, one of 1400 gives 8.6e18"""
    from dl4ds_amd.metrics import check_neighbourhood_args, neighbourhood_scores, FSS_SUM_BOUND
    _no_library(monkeypatch)
    assert FSS_SUM_BOUND == 2 ** 62
    y = np.zeros((1, 1500, 1500, 1), np.float32)
    for n in (1400, 1500, 10 ** 6):
        with pytest.raises(ValueError, match=r'2\^62'):
            neighbourhood_scores(y, y, (0.0,), windows=(1, n))
    check_neighbourhood_args(y.shape, (0.0,), (1, 1100))
    h, w = 1500, 1500
    edge = next(n for n in range(1, 1501) if h * w * (n * n) ** 2 >= 2 ** 62)      # the first refused window: exactly at the bound
    check_neighbourhood_args(y.shape, (0.0,), (edge - 1,))
    with pytest.raises(ValueError, match=r'2\^62'):
        check_neighbourhood_args(y.shape, (0.0,), (edge,))
    with pytest.raises(ValueError, match=r'2\^31'):
        check_neighbourhood_args((1, 2 ** 16, 2 ** 15, 1), (0.0,), (1,))
    thr, win = check_neighbourhood_args((1, 2 ** 15, 2 ** 15, 1), (0.25, np.float64(0.3)), [1, np.int64(3)])
    assert thr.dtype == np.float32 and thr.tolist() == [0.25, float(np.float32(0.3))] and win.dtype == np.int32


def test_exports_and_signatures():
    import dl4ds_amd as dds
    from dl4ds_amd import metrics
    assert dds.neighbourhood_scores is metrics.neighbourhood_scores and dds.fss is metrics.fss
    sig = inspect.signature(metrics.neighbourhood_scores)
    assert list(sig.parameters) == ['y_test', 'y_test_hat', 'thresholds', 'windows', 'scaler', 'mask', 'batch_size']
    assert sig.parameters['windows'].default == (1, 3, 5, 9, 17, 33, 65)
    assert all(sig.parameters[k].default is None for k in ('scaler', 'mask', 'batch_size'))
    assert list(inspect.signature(metrics.fss).parameters)[:4] == ['y', 'y_hat', 'thresholds', 'windows']


def test_c_entry_is_declared():
    import dl4ds_amd._lib as L
    protos = L.parse_header()
    assert 'dl4ds_fss' in protos                              # tests/test_abi.py then checks that the library exports it
    assert len(protos['dl4ds_fss'][1]) == 13
    assert os.path.exists(os.path.join(ROOT, 'dl4ds_amd', 'csrc', 'fss.hip'))


@pytest.mark.parametrize('name', sorted(CASES))
def test_reference_is_finite_on_the_gpu_cases_except_by_construction(name):
    """the NaNs of the expected arrays of tests/test_gpu_fss.py are exactly the thresholds built to have no event"""
    c = CASES[name]()
    r = fss_ref.neighbourhood_scores(c['y'], c['p'], c['thresholds'], c['windows'], mask=c['mask'])
    T = len(c['thresholds'])
    want_nan = np.zeros(r['fss'].shape, bool)
    want_nan[:, :, list(c['nan_thresholds'])] = True
    np.testing.assert_array_equal(np.isnan(r['fss']), want_nan)
    np.testing.assert_array_equal(np.isnan(r['fss_pooled']), want_nan[0, 0])
    np.testing.assert_array_equal(np.isnan(r['fss_pooled_per_channel']), want_nan[0])
    assert np.isfinite(r['base_rate']).all() and (r['n_valid'] > 0).all()
    ok = [k for k in range(T) if k not in c['nan_thresholds']]
    assert (r['hits'][:, :, ok] + r['misses'][:, :, ok] > 0).all() and (r['hits'][:, :, ok] + r['false_alarms'][:, :, ok] > 0).all()
    assert (np.diff(np.asarray(c['windows'])) > 0).all()
    assert (np.diff(np.asarray(c['thresholds'], np.float32)) > 0).all()
