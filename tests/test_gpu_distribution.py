"""Distribution verification on the device (dl4ds_distribution, csrc/distribution.hip) through
dl4ds_amd.metrics.distribution_scores against the numpy restatement tests/distribution_ref.py (itself checked against np.quantile,
scipy.stats, np.histogram and hand-worked answers in tests/test_distribution_api.py).  Counts (n_valid, KS * n, histograms) are
compared with assert_array_equal.  Quantiles: both sides evaluate x_j + (x_j+1 - x_j) * g in fp64 on the same float32 order
statistics; the bound is 2^-50 * max(|x_j|, |x_j+1|), three roundings of at most 2^-52 of that magnitude on either side.  W1: a sum
of n non-negative fp64 terms in another order, each order within (n - 1) * 2^-53 relative of the exact sum, and one division:
n * 2^-52 relative.  The only NaNs in the expected arrays are the ones the cases are built to give
(tests/test_distribution_api.py pins that down)."""
import functools

import numpy as np
import pytest

from tests import distribution_ref as ref
from tests.distribution_cases import (CASES, LDS_MAX, MAX_E, MAX_Q, STRIDED_MAX, TILE, WS_BUDGET, global_bytes_per_segment,
                                      strided_group)

pytestmark = pytest.mark.gpu

INTEGERS = ('n_valid', 'ks_count')
HIST = ('hist_obs', 'hist_pred', 'hist_obs_pooled', 'hist_pred_pooled')
RATIOS = ('ks',)                                   # one fp64 division of equal integers on either side


@functools.lru_cache(maxsize=None)
def case(name):
    """(case, expected dict, quantile bounds), computed once per session and left unchanged"""
    c = CASES[name]()
    want, bounds = ref.distribution_scores(c['y'], c['p'], c['quantiles'], c['bins'], c['over'], c['mask'], return_bounds=True)
    return c, want, bounds


def check(got, want, bounds):
    keys = set(INTEGERS) | set(RATIOS) | {'q_obs', 'q_pred', 'q_bias', 'wasserstein', 'quantiles', 'bins'}
    if want['bins'] is not None:
        keys |= set(HIST) | {'perkins', 'perkins_pooled'}
    assert set(got) == set(want) == keys
    for k in INTEGERS + (HIST if want['bins'] is not None else ()):
        assert got[k].dtype == np.int64 and got[k].shape == want[k].shape, k
        np.testing.assert_array_equal(got[k], want[k], err_msg=k)
    for k in RATIOS + (('perkins', 'perkins_pooled') if want['bins'] is not None else ()):
        assert got[k].dtype == np.float64 and np.shape(got[k]) == np.shape(want[k]), k
        np.testing.assert_array_equal(got[k], want[k], err_msg=k)             # (NaN positions included)
    for k, b in (('q_obs', bounds[0]), ('q_pred', bounds[1]), ('q_bias', bounds[0] + bounds[1])):
        assert got[k].dtype == np.float64 and got[k].shape == want[k].shape, k
        np.testing.assert_array_equal(np.isnan(got[k]), np.isnan(want[k]), err_msg=k)
        ok = ~np.isnan(want[k])
        err = np.abs(got[k][ok] - want[k][ok])
        assert (err <= b[ok]).all(), (k, float(err.max()), float((err / np.maximum(b[ok], 1e-300)).max()))
    w, g = want['wasserstein'], got['wasserstein']
    assert g.dtype == np.float64 and g.shape == w.shape
    np.testing.assert_array_equal(np.isnan(g), np.isnan(w))
    ok = ~np.isnan(w)
    assert (np.abs(g[ok] - w[ok]) <= want['n_valid'][ok] * 2.0 ** -52 * np.abs(w[ok])).all()
    np.testing.assert_array_equal(got['quantiles'], want['quantiles'])
    if want['bins'] is None:
        assert got['bins'] is None
    else:
        assert got['bins'].dtype == np.float32
        np.testing.assert_array_equal(got['bins'], want['bins'])


@pytest.mark.parametrize('name', sorted(CASES))
def test_against_the_restatement(name):
    from dl4ds_amd.metrics import distribution_scores
    c, want, bounds = case(name)
    got = distribution_scores(c['y'], c['p'], c['quantiles'], c['bins'], over=c['over'], mask=c['mask'])
    N, H, W, C = c['y'].shape
    lead = (H, W, C) if c['over'] == 'time' else (N,)
    assert got['n_valid'].shape == lead and got['q_obs'].shape == lead + (len(c['quantiles']),)
    check(got, want, bounds)
    assert int((got['n_valid'] == 0).sum()) == c['empty']
    np.testing.assert_array_equal(np.isnan(got['wasserstein']), got['n_valid'] == 0)     # NaN where n = 0 by construction only
    length, cells = (N, H * W * C) if c['over'] == 'time' else (H * W * C, N)
    if name == 'workspace_chunks':
        assert length > STRIDED_MAX and cells * global_bytes_per_segment(length) > WS_BUDGET
    if name == f'space{3 * TILE + 5}':
        assert length == 3 * TILE + 5 > LDS_MAX
    if name.startswith('time') and 'x105' not in name and 'x6' not in name:
        assert cells == strided_group(length) + 1
    if name == 'caps':
        assert len(c['quantiles']) == MAX_Q and len(c['bins']) == MAX_E
    if name == 'quantiles_0_and_1':
        v = ~np.isnan(c['y'])
        assert v.all()
        np.testing.assert_array_equal(got['q_obs'][..., 0], c['y'].min(0))
        np.testing.assert_array_equal(got['q_obs'][..., 1], c['y'].max(0))
    if name == 'single_valid_element':
        assert got['n_valid'][0, 0, 0] == 1 and (got['q_obs'][0, 0, 0] == 1.25).all()
        assert got['ks_count'][0, 0, 0] == (0 if c['p'][7, 0, 0, 0] == np.float32(1.25) else 1)
    if name == 'all_equal':
        assert (got['q_obs'] == 2.5).all() and (got['q_pred'] == 3.0).all() and (got['wasserstein'] == 0.5).all()
        assert (got['ks_count'] == N).all() and (got['hist_obs'] == [0, N]).all() and (got['hist_pred'] == [0, N]).all()


def test_wrapper_scaler_and_5d_input():
    from dl4ds_amd.metrics import distribution_scores, quantile_maps

    class Scaler:
        def inverse_transform(self, a):
            return a * 2.0 + 1.0

    c = CASES['time37x105']()
    y2, p2 = c['y'] * 2.0 + 1.0, c['p'] * 2.0 + 1.0
    bins = (1.0, 1.5, 3.0, 9.0, 50.0)
    want, bounds = ref.distribution_scores(y2, p2, c['quantiles'], bins, return_bounds=True)
    got = distribution_scores(c['y'][..., None], c['p'][..., None], c['quantiles'], bins, scaler=Scaler())
    check(got, want, bounds)
    direct = distribution_scores(y2, p2, c['quantiles'], bins)
    for k in want:
        assert np.asarray(got[k]).tobytes() == np.asarray(direct[k]).tobytes(), k
    qo, qp = quantile_maps(c['y'].astype(np.float64)[..., None], c['p'][..., None], c['quantiles'], scaler=Scaler())
    assert qo.tobytes() == got['q_obs'].tobytes() and qp.tobytes() == got['q_pred'].tobytes()
    dflt = distribution_scores(c['y'], c['p'])                              # the default quantiles, no bins
    assert dflt['quantiles'].tolist() == [0.01, 0.05, 0.25, 0.5, 0.75, 0.95, 0.99] and dflt['bins'] is None
    qs, _ = quantile_maps(c['y'], c['p'], (0.5,), over='space')
    assert qs.shape == (37, 1)


@pytest.mark.parametrize('name', ['nonfinite_time', 'nonfinite_space', f'time{STRIDED_MAX + 1}x6', 'single_column_grid'])
def test_result_does_not_depend_on_batch_size_and_is_reproducible(name):
    """rows ('time') or samples ('space') per upload: 1, 3 (a non-divisor), more than there are; and the same call twice"""
    from dl4ds_amd.metrics import distribution_scores
    c, want, bounds = case(name)
    args = (c['y'], c['p'], c['quantiles'], c['bins'])
    first = distribution_scores(*args, over=c['over'], mask=c['mask'])
    check(first, want, bounds)
    for bs in (None, 1, 3, 1000):
        got = distribution_scores(*args, over=c['over'], mask=c['mask'], batch_size=bs)
        for k in first:
            assert np.asarray(got[k]).tobytes() == np.asarray(first[k]).tobytes(), (bs, k)


def _direct(y, p, S, L, ss, es, q, edges, fill=0):
    """dl4ds_distribution called directly -> (status, quant, w1, ks, hist, valid)"""
    import dl4ds_amd._lib as L_
    from dl4ds_amd.device import DeviceArray
    q, edges = np.asarray(q, np.float64), np.asarray(edges, np.float32)
    Q, E = len(q), len(edges)
    dy, dp = DeviceArray.from_numpy(y), DeviceArray.from_numpy(p)
    shapes = (((S, 2, max(Q, 1)), np.float64), ((S,), np.float64), ((S,), np.int64), ((S, 2, max(E - 1, 1)), np.int64), ((S,), np.int64))
    outs = [DeviceArray.from_numpy(np.full(s, fill, d)) for s, d in shapes]
    st = L_.lib().dl4ds_distribution(dy.ptr, dp.ptr, S, L, ss, es, q.ctypes.data if Q else None, Q,
                                     edges.ctypes.data if E else None, E, *(o.ptr for o in outs))
    res = (st,) + tuple(o.numpy() for o in outs)
    for d in [dy, dp] + outs:
        d.free()
    return res


def test_refusals_of_the_c_entry():
    import dl4ds_amd._lib as L_
    y = np.zeros((4, 8), np.float32)
    ok = dict(S=4, L=8, ss=8, es=1, q=(0.5,), edges=(0.0, 1.0))
    for bad, word in [(dict(L=2 ** 31), '2^31'), (dict(q=(1.5,)), '[0, 1]'), (dict(q=(-0.1,)), '[0, 1]'), (dict(q=(np.nan,)), '[0, 1]'),
                      (dict(q=np.linspace(0, 1, MAX_Q + 1)), '64'), (dict(edges=np.linspace(0, 1, MAX_E + 1)), '257'),
                      (dict(edges=(0.0, np.inf)), 'finite'), (dict(edges=(0.0, np.nan)), 'finite'),
                      (dict(edges=(1.0, 1.0)), 'increasing'), (dict(edges=(1.0, 0.0)), 'increasing'), (dict(edges=(1.0,)), '257')]:
        args = dict(ok)
        args.update(bad)
        res = _direct(y, y, fill=7, **args)
        assert res[0] != 0, bad
        assert word in L_.load().dl4ds_last_error().decode(), (bad, L_.load().dl4ds_last_error().decode())
        assert all((o == 7).all() for o in res[1:]), bad                   # nothing was written
    lib = L_.lib()
    neg = lib.dl4ds_distribution(None, None, 1, 1, 1, 1, None, -1, None, 0, None, None, None, None, None)
    assert neg != 0 and '64' in L_.load().dl4ds_last_error().decode()


def test_direct_call_overwrites_its_outputs_on_every_engine():
    """garbage in the outputs, general strides: contiguous rows (LDS engine), columns of a row-major matrix (strided engine, global
    engine beyond STRIDED_MAX), and Q = 0 with E = 0"""
    rng = np.random.default_rng(77)
    for shape, by_column in [((5, 300), False), ((300, 21), True), ((STRIDED_MAX + 3, 5), True), ((2, LDS_MAX + 7), False)]:
        y = np.round(rng.standard_normal(shape), 1).astype(np.float32)
        p = np.round(rng.standard_normal(shape), 1).astype(np.float32)
        y[0, 0] = np.nan
        S, L, ss, es = (shape[1], shape[0], 1, shape[1]) if by_column else (shape[0], shape[1], shape[1], 1)
        q, edges = (0.0, 0.3, 1.0), (-1.0, 0.0, 0.05, 1.0)
        st, quant, w1, ks, hist, valid = _direct(y, p, S, L, ss, es, q, edges, fill=7)
        assert st == 0
        for s in range(S):
            ys, ps = (y[:, s], p[:, s]) if by_column else (y[s], p[s])
            wq, ww, wk, wh, wn, mag = ref.segment_scores(ys, ps, q, edges)
            assert valid[s] == wn and ks[s] == wk
            np.testing.assert_array_equal(hist[s], wh)
            assert (np.abs(quant[s] - wq) <= 2.0 ** -50 * mag).all() and abs(w1[s] - ww) <= wn * 2.0 ** -52 * abs(ww)
        st, quant, w1b, ksb, hist, validb = _direct(y, p, S, L, ss, es, (), (), fill=7)
        assert st == 0 and (quant == 7).all() and (hist == 7).all()           # no quantile, no histogram: those stay untouched
        assert w1b.tobytes() == w1.tobytes() and (ksb == ks).all() and (validb == valid).all()
