"""Neighbourhood verification on the device (dl4ds_fss, csrc/fss.hip) through dl4ds_amd.metrics.neighbourhood_scores against the
integer restatement tests/fss_ref.py (itself checked against scipy.ndimage.uniform_filter and hand-worked answers in
tests/test_fss_api.py).  The device works in integers: sums, contingency counts and n_valid are compared with assert_array_equal;
the scores are one fp64 division of equal integers on either side and are compared at 1e-12 absolute.  The only NaNs in the
expected arrays are the ones the cases are built to give (tests/test_fss_api.py pins that down)."""
import ctypes

import numpy as np
import pytest

from tests import fss_ref
from tests.fss_cases import CASES, NARROW_MAX, THRESHOLD_GROUP, WS_BUDGET

pytestmark = pytest.mark.gpu

ATOL = 1e-12
INTEGERS = ('sums', 'hits', 'misses', 'false_alarms', 'correct_negatives', 'n_valid', 'useful_window', 'windows')
SCORES = ('fss', 'fss_pooled', 'fss_pooled_per_channel', 'pod', 'far', 'csi', 'ets', 'bias', 'pod_pooled', 'far_pooled',
          'csi_pooled', 'ets_pooled', 'bias_pooled', 'base_rate', 'fss_random', 'fss_useful')


def check(got, want):
    assert set(got) == set(want) == set(INTEGERS) | set(SCORES) | {'thresholds'}
    for k in INTEGERS:
        assert got[k].dtype == np.int64 and got[k].shape == want[k].shape, k
        np.testing.assert_array_equal(got[k], want[k], err_msg=k)
    assert got['thresholds'].dtype == np.float32
    np.testing.assert_array_equal(got['thresholds'], want['thresholds'])
    for k in SCORES:
        assert got[k].dtype == np.float64 and got[k].shape == want[k].shape, k
        np.testing.assert_array_equal(np.isnan(got[k]), np.isnan(want[k]), err_msg=k)
        np.testing.assert_allclose(got[k], want[k], rtol=0, atol=ATOL, equal_nan=True, err_msg=k)


@pytest.mark.parametrize('name', sorted(CASES))
def test_against_the_integer_reference(name):
    from dl4ds_amd.metrics import neighbourhood_scores
    c = CASES[name]()
    got = neighbourhood_scores(c['y'], c['p'], c['thresholds'], c['windows'], mask=c['mask'])
    want = fss_ref.neighbourhood_scores(c['y'], c['p'], c['thresholds'], c['windows'], mask=c['mask'])
    N, H, W, C = c['y'].shape
    T, S = len(c['thresholds']), len(c['windows'])
    assert got['sums'].shape == (N, C, T, S, 3) and got['fss'].shape == (N, C, T, S) and got['hits'].shape == (N, C, T)
    assert got['fss_pooled'].shape == (T, S) and got['fss_pooled_per_channel'].shape == (C, T, S) and got['n_valid'].shape == (N, C)
    check(got, want)
    nan = np.zeros((N, C, T, S), bool)
    nan[:, :, list(c['nan_thresholds'])] = True
    np.testing.assert_array_equal(np.isnan(got['fss']), nan)              # NaN where F + O = 0 by construction, nowhere else
    if name == 'extremes':
        assert (got['hits'][:, :, 0] == got['n_valid']).all()            # below the minimum: every valid cell an event
        assert (got['sums'][:, :, 3] == 0).all() and (got['hits'][:, :, 3] + got['false_alarms'][:, :, 3] == 0).all()
    if name == 'precip512':
        assert (np.diff(got['fss_pooled'][:, :4], axis=1) > 0).all()     # a displaced forecast gains skill with the scale
        m = np.minimum(np.array(c['windows']), 512) ** 2
        assert (m[:5] <= NARROW_MAX).all() and (m[5:] > NARROW_MAX).all()
    if name == 'workspace_chunks':
        assert N * min(T, THRESHOLD_GROUP) * 2 * H * (W + 1) * 2 > WS_BUDGET


def test_wrapper_scaler_and_5d_input():
    from dl4ds_amd.metrics import fss, neighbourhood_scores

    class Scaler:
        def inverse_transform(self, a):
            return a * 2.0 + 1.0

    c = CASES['two_channels']()
    want = fss_ref.neighbourhood_scores(c['y'] * 2.0 + 1.0, c['p'] * 2.0 + 1.0, c['thresholds'], (1, 4, 9))
    f, fp = fss(c['y'][..., None], c['p'][..., None], c['thresholds'], (1, 4, 9), scaler=Scaler())
    np.testing.assert_allclose(f, want['fss'], rtol=0, atol=ATOL)
    np.testing.assert_allclose(fp, want['fss_pooled'], rtol=0, atol=ATOL)
    got = neighbourhood_scores(c['y'].astype(np.float64), c['p'].astype(np.float64), c['thresholds'])    # the default windows
    assert got['windows'].tolist() == [1, 3, 5, 9, 17, 33, 65]
    check(got, fss_ref.neighbourhood_scores(c['y'], c['p'], c['thresholds'], (1, 3, 5, 9, 17, 33, 65)))


def test_result_does_not_depend_on_batch_size_and_is_reproducible():
    from dl4ds_amd.metrics import neighbourhood_scores
    c = CASES['nonfinite_mask2d']()
    y, p = np.concatenate([c['y'], c['y'][:2, ::-1]]), np.concatenate([c['p'], c['p'][:2, ::-1]])      # N = 5
    args = (y, p, c['thresholds'], c['windows'])
    ref = neighbourhood_scores(*args, mask=c['mask'])
    check(ref, fss_ref.neighbourhood_scores(*args, mask=c['mask']))
    for bs in (1, 2, 5, None, 64):                                        # one, a non-divisor of N, N, the default, more than N
        got = neighbourhood_scores(*args, mask=c['mask'], batch_size=bs)
        for k in ref:
            assert got[k].tobytes() == ref[k].tobytes(), (bs, k)


def _direct(y, p, thresholds, windows):
    """dl4ds_fss called directly -> (status, sums, cont, valid)"""
    import dl4ds_amd._lib as L
    from dl4ds_amd.device import DeviceArray
    N, H, W, C = y.shape
    thr, win = np.asarray(thresholds, np.float32), np.asarray(windows, np.int32)
    dy, dp = DeviceArray.from_numpy(y), DeviceArray.from_numpy(p)
    outs = [DeviceArray.zeros(s, np.int64) for s in ((N, C, len(thr), len(win), 3), (N, C, len(thr), 4), (N, C))]
    st = L.lib().dl4ds_fss(dy.ptr, dp.ptr, N, H, W, C, thr.ctypes.data, len(thr), win.ctypes.data, len(win), *(o.ptr for o in outs))
    return (st,) + tuple(o.numpy() for o in outs)


def test_overflow_rule():
    """1500 x 1500 cells: a window of 1400 has H*W*m^2 = 8.6e18 >= 2^62 and is refused by the Python layer and by the C entry;
    one of 1100 (3.3e18) is legal and, on an all-event field, drives the 64-bit sums to within a factor of two of the bound"""
    import dl4ds_amd._lib as L
    from dl4ds_amd.metrics import neighbourhood_scores
    y = np.ones((1, 1500, 1500, 1), np.float32)
    with pytest.raises(ValueError, match=r'2\^62'):
        neighbourhood_scores(y, y, (0.5,), windows=(1, 1400))
    st, sums, _, _ = _direct(y, y, (0.5,), (1, 1400))
    assert st != 0 and '2^62' in L.load().dl4ds_last_error().decode()
    assert (sums == 0).all()                                              # nothing was written
    for bad in [dict(thresholds=(np.nan,)), dict(windows=(0,)), dict(thresholds=())]:
        args = dict(thresholds=(0.5,), windows=(1,))
        args.update(bad)
        assert _direct(y[:, :8, :8], y[:, :8, :8], args['thresholds'], args['windows'])[0] != 0
    p = y.copy()
    p[0, :700] = 0.0
    got = neighbourhood_scores(y, p, (0.5,), windows=(1, 1100))
    want = fss_ref.neighbourhood_scores(y, p, (0.5,), (1, 1100))
    check(got, want)
    assert got['sums'][0, 0, 0, 1, 2] > 2 ** 60


def test_direct_call_overwrites_its_outputs():
    c = CASES['tiny']()
    a = _direct(c['y'], c['p'], c['thresholds'], c['windows'])
    want = fss_ref.neighbourhood_scores(c['y'], c['p'], c['thresholds'], c['windows'])
    assert a[0] == 0
    np.testing.assert_array_equal(a[1], want['sums'])
    np.testing.assert_array_equal(a[2][..., 0], want['hits'])
    np.testing.assert_array_equal(a[3], want['n_valid'])
    import dl4ds_amd._lib as L
    from dl4ds_amd.device import DeviceArray
    N, H, W, C = c['y'].shape
    thr, win = np.asarray(c['thresholds'], np.float32), np.asarray(c['windows'], np.int32)
    dy, dp = DeviceArray.from_numpy(c['y']), DeviceArray.from_numpy(c['p'])
    outs = [DeviceArray.from_numpy(np.full(x.shape, 7, np.int64)) for x in a[1:]]          # garbage in the outputs
    for _ in range(2):                                                                       # and a second call on top of the first
        L.check(L.lib().dl4ds_fss(dy.ptr, dp.ptr, N, H, W, C, thr.ctypes.data, len(thr), win.ctypes.data, len(win),
                                  *(o.ptr for o in outs)))
    for o, x in zip(outs, a[1:]):
        np.testing.assert_array_equal(o.numpy(), x)
