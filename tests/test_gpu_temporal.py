"""Temporal verification on the device (dl4ds_temporal, csrc/temporal.hip; dl4ds_trend, csrc/trend.hip)
against the numpy restatement tests/temporal_ref.py (itself checked against itertools.groupby, plain Python loops, np.median,
scipy and hand-worked answers in tests/test_temporal_api.py).  Everything is compared bit for bit: the integers as integers, fp64
on its unsigned view, NaN included."""
import functools

import numpy as np
import pytest

from tests import temporal_cases as cases
from tests import temporal_ref as ref

pytestmark = pytest.mark.gpu

OUTPUTS = ('valid', 'moment', 'pair', 'lag', 'trans', 'spell')


def same_bits(g, w, what):
    assert g.dtype == w.dtype and g.shape == w.shape, (what, g.dtype, g.shape, w.dtype, w.shape)
    if w.dtype.kind == 'f':
        g, w = g.view(np.uint64), w.view(np.uint64)
    np.testing.assert_array_equal(g, w, err_msg=str(what))


def assert_same(got, want, what=''):
    assert len(got) == len(want)
    for name, g, w in zip(OUTPUTS, got, want):
        if w is None or w.size == 0:
            assert g is None, (what, name)
            continue
        same_bits(g, w, (what, name))


def device_temporal(y, p, st, lags=(), thr=(), op=0, bins=16, want=(True,) * 6):
    """dl4ds_temporal on the (N, cells) host arrays -> the six outputs, None where the output pointer was null (an output of no
    elements, L = 0 or T = 0, is always passed as null)"""
    from dl4ds_amd import _lib
    from dl4ds_amd.device import Buffers
    N, per = y.shape
    st, thr, lags = np.ascontiguousarray(st, np.int64), np.ascontiguousarray(thr, np.float32), np.ascontiguousarray(lags, np.int32)
    P, T, L, S = len(st) - 1, thr.shape[0], len(lags), 1 if p is None else 2
    shapes = (((P, per), np.int32), ((P, S, 2, per), np.float64), ((P, L, per), np.int32), ((P, S, L, 3, per), np.float64),
              ((P, S, T, 4, per), np.int32), ((P, S, T, 2, bins, per), np.int32))
    with Buffers() as buf:
        dy = buf.alloc(y.shape)
        dy.upload(np.ascontiguousarray(y, np.float32))
        dp = None
        if p is not None:
            dp = buf.alloc(p.shape)
            dp.upload(np.ascontiguousarray(p, np.float32))
        dthr = None
        if T:
            dthr = buf.alloc(thr.shape)
            dthr.upload(thr)
        devs = [buf.alloc(s, d) if w and int(np.prod(s)) else None for (s, d), w in zip(shapes, want)]
        for d in devs:                                          # every output is overwritten: start from a pattern
            if d is not None:
                _lib.check(_lib.lib().dl4ds_memset(d.ptr, 0x5a, d.nbytes))
        _lib.check(_lib.lib().dl4ds_temporal(dy.ptr, dp.ptr if dp is not None else None, N, per, st.ctypes.data, P,
                                             lags.ctypes.data if L else None, L, dthr.ptr if T else None, T, int(thr.ndim == 2), op,
                                             bins, *(d.ptr if d is not None else None for d in devs)))
        return tuple(d.numpy() if d is not None else None for d in devs)


@functools.lru_cache(maxsize=None)
def expected(n, cells, kind, S, lags, T, op, bins, per_cell, seed=0):
    """(y, p, starts, thr, the restatement's six outputs): computed once and left unchanged"""
    y = cases.series(n, cells, seed)
    p = cases.second(n, cells, seed) if S == 2 else None
    st = cases.starts(n, kind)
    thr = cases.cell_thresholds(T, cells, seed) if per_cell and T else np.asarray(cases.SCALARS[:T], np.float32)
    return y, p, st, thr, ref.temporal(y, p, st, lags, thr, op, bins)


def check(n, cells, kind, S, lags, T, op, bins=16, per_cell=False, seed=0):
    y, p, st, thr, want = expected(n, cells, kind, S, lags, T, op, bins, per_cell, seed)
    assert_same(device_temporal(y, p, st, lags, thr, op, bins), want, (n, cells, kind, S, lags, T, op, bins, per_cell))
    return y, p, st, thr, want


@pytest.mark.parametrize('n', cases.LENGTHS)
@pytest.mark.parametrize('cells', cases.CELLS)
def test_temporal_sizes(cells, n):
    """one cell, a partial wave, a whole one, one lane more, one cell more than a workgroup takes; one and two samples, the load
    block +- 1, lag 32 and the ring at their edge (33, 34), many blocks; one period, three uneven ones with a one-sample period,
    every sample a period; S = 1 and 2; L = 0..4; T = 0..4, every op, scalar and per-cell thresholds with a NaN threshold in one
    cell of one t; every B"""
    assert cells <= cases.GROUP + 1 and n in (1, 2, 4, 5, 9, 33, 34, 97) and cases.DEPTH == 8 and cases.RING == 32
    for k, kind in enumerate(cases.PERIOD_KINDS):
        for T in (0, 1, 2, 3, 4):
            j = T + k
            check(n, cells, kind, 1 + j % 2, cases.LAG_SETS[j % len(cases.LAG_SETS)], T, j % 4, cases.BINS[j % 4], j % 2 == 1,
                  seed=n + cells)


@pytest.mark.parametrize('S', [1, 2])
@pytest.mark.parametrize('T', [0, 1, 2, 3, 4])
def test_every_kernel_form(T, S):
    """every (S, T, L) the library compiles, every op, scalar and per-cell thresholds"""
    for L, lags in enumerate(((), (32,), (1, 32), (1, 2, 5), (1, 2, 5, 32))):
        assert len(lags) == L
        for op in range(4) if T else (0,):
            check(97, 65, 'uneven', S, lags, T, op, 16, per_cell=(op + L) % 2 == 1)


@pytest.mark.parametrize('bins', cases.BINS)
def test_spell_bins(bins):
    for S in (1, 2):
        *_, want = check(97, 70, 'uneven', S, (1,), 2, 0, bins, seed=bins)
        spell = want[5]
        assert spell.shape[4] == bins and spell[:, :, 0].max() > 0


def test_the_case_reaches_the_walks_branches():
    """a case cannot pass by never reaching a branch: an event run longer than one load block, a lag pair that spans two load
    blocks, a run that overflows into the last bin, an all-NaN cell, NaN in one series only, the 1e30 spike"""
    lags, bins = (1, 2, 5, 32), 4
    y, p, st, thr, (valid, moment, pair, lag, trans, spell) = check(97, 65, 'uneven', 2, lags, 2, 0, bins)
    longest, spans, overflows, all_nan = cases.reaches(y, st, lags, thr[0], bins)
    assert longest > cases.DEPTH and spans and overflows and all_nan
    assert spell[:, 0, 0, 0, bins - 1].max() > 0 and (valid[:, 3] == 0).all() and (moment[:, :, :, 3] == 0).all()
    only_y, only_p = np.isfinite(y) & ~np.isfinite(p), ~np.isfinite(y) & np.isfinite(p)
    assert only_y.any() and only_p.any()                                        # common validity matters
    alone = ref.temporal(y, None, st, lags, thr, 0, bins)
    assert (alone[0] >= valid).all() and (alone[0] > valid).any()
    assert (y[:, 2] == np.float32(1e30)).any() and moment[:, 0, 1, 2].max() > 1e59
    lens = np.diff(st)
    assert (spell[:, 0, 0, 0, :, 0].sum(axis=1) == 1).all() and (trans[:, 0, 0, 3, 0] == lens - 1).all()   # cell 0: one run per period
    assert pair[0, 3].max() > 0 and (pair[1] == 0).all()                         # lag 32 has pairs; the one-sample period none


def test_each_output_may_be_null_and_a_repeated_call_gives_the_same_bits():
    y, p, st, thr, want = expected(97, 65, 'uneven', 2, (1, 2, 5, 32), 3, 0, 16, True)
    first = device_temporal(y, p, st, (1, 2, 5, 32), thr, 0, 16)
    assert_same(first, want)
    assert_same(device_temporal(y, p, st, (1, 2, 5, 32), thr, 0, 16), first, 'repeat')
    for k in range(6):
        keep = tuple(j != k for j in range(6))
        got = device_temporal(y, p, st, (1, 2, 5, 32), thr, 0, 16, want=keep)
        assert_same(got, tuple(w if j != k else None for j, w in enumerate(want)), f'null {k}')
        only = tuple(j == k for j in range(6))
        got = device_temporal(y, p, st, (1, 2, 5, 32), thr, 0, 16, want=only)
        assert_same(got, tuple(w if j == k else None for j, w in enumerate(want)), f'only {k}')


def test_signed_zeros_against_zero_thresholds():
    z = np.where(np.arange(30)[:, None] % 3 == 0, np.float32(-0.0), np.float32(0.0)) * np.ones((1, 66), np.float32)
    st = cases.starts(30, 'uneven')
    for op in range(4):
        for t0 in (0.0, -0.0):
            thr = np.array([t0], np.float32)
            got = device_temporal(z, None, st, (1,), thr, op, 4)
            assert_same(got, ref.temporal(z, None, st, (1,), thr, op, 4))
            assert not np.signbit(got[1]).any() and not np.signbit(got[3]).any()
            assert (got[4][[0, 2], 0, 0, 3 if op in (0, 3) else 0] > 0).all()    # all events under >= and <=, none under > and <


# ------------------------------------------------------------------------------------------------------------------------ trend
def device_trend(v, want=(True, True, True)):
    from dl4ds_amd import _lib
    from dl4ds_amd.device import Buffers
    P, per = v.shape
    shapes = (((per,), np.int32), ((2, per), np.int64), ((per,), np.float64))
    with Buffers() as buf:
        dv = buf.alloc(v.shape, np.float64)
        dv.upload(np.ascontiguousarray(v, np.float64))
        devs = [buf.alloc(s, d) if w else None for (s, d), w in zip(shapes, want)]
        for d in devs:
            if d is not None:
                _lib.check(_lib.lib().dl4ds_memset(d.ptr, 0x5a, d.nbytes))
        _lib.check(_lib.lib().dl4ds_trend(dv.ptr, P, per, *(d.ptr if d is not None else None for d in devs)))
        return tuple(d.numpy() if d is not None else None for d in devs)


@functools.lru_cache(maxsize=None)
def expected_trend(P, cells):
    v = cases.trend_values(P, cells, seed=P + cells)
    return v, ref.trend(v)


def assert_trend(got, want, what=''):
    for name, g, w in zip(('valid', 'mk', 'sen'), got, want):
        if w is None:
            assert g is None, (what, name)
        else:
            same_bits(g, w, (what, name))


@pytest.mark.parametrize('P', cases.TREND_PERIODS)
@pytest.mark.parametrize('cells', cases.CELLS)
def test_trend_sizes(cells, P):
    """32 -> 33 periods cross the 512-slope network, 64 -> 65 the 2048-slope one; heavy ties, NaN gaps, n = 0 / 1 / 2, signed
    zeros, even and odd numbers of slopes"""
    v, want = expected_trend(P, cells)
    assert_trend(device_trend(v), want, (P, cells))
    n, (s, ties), sen = want
    if cells > 6 and P >= 4:
        M = n.astype(np.int64) * (n - 1) // 2
        assert (M % 2 == 0).any() and (M % 2 == 1).any() and n[1] == 0 and n[2] == 1 and n[3] == 2
        assert np.isnan(sen[1]) and np.isnan(sen[2]) and sen[3] == -3.0 / (P - 1) and s[3] == -1
        assert s[4] == 0 and ties[4] == n[4] * (n[4] - 1) * (2 * n[4] + 5) and sen[4] == 0 and not np.signbit(sen[4])
        assert s[6] == n[6] * (n[6] - 1) // 2 and ties[6] == 0 and sen[6] == 0.5
        assert (P < 32 or (ties[::4] > 0).all()) and not np.signbit(sen[sen == 0]).any()


def test_trend_outputs_may_be_null_and_a_repeated_call_gives_the_same_bits():
    v, want = expected_trend(65, 65)
    first = device_trend(v)
    assert_trend(first, want)
    assert_trend(device_trend(v), first, 'repeat')
    for k in range(3):
        keep = tuple(j != k for j in range(3))
        assert_trend(device_trend(v, keep), tuple(w if j != k else None for j, w in enumerate(want)), f'null {k}')
        only = tuple(j == k for j in range(3))
        assert_trend(device_trend(v, only), tuple(w if j == k else None for j, w in enumerate(want)), f'only {k}')


# ---------------------------------------------------------------------------------------------------------------- the host layer
GRID = (6, 7, 2)
LAGS = (1, 3)


@functools.lru_cache(maxsize=None)
def host_case():
    y = cases.series(60, 84, seed=9).reshape((60,) + GRID)
    p = cases.second(60, 84, seed=9).reshape((60,) + GRID)
    years = np.repeat([2001, 2002, 2004], [25, 1, 34])
    thr = cases.cell_thresholds(2, 84, seed=9).reshape((2,) + GRID)
    return y, p, years, thr


def named_ref(y, p, st, lags, thr, op, bins, s):
    """what `temporal_statistics` / one side of `temporal_scores` must return: the restatement's raw outputs and the statistics of
    dl4ds_amd.temporal.temporal_from_sums (checked on its own in tests/test_temporal_api.py) of them"""
    from dl4ds_amd.temporal import temporal_from_sums
    grid = y.shape[1:]
    thr = np.asarray(thr, np.float32)
    flat = ref.temporal(y.reshape(len(y), -1), None if p is None else p.reshape(len(p), -1), st, lags,
                        thr.reshape(thr.shape[0], -1) if thr.ndim > 1 else thr, op, bins)
    out = ref.named(flat, s, grid)
    out.update(temporal_from_sums(out))
    out['period_starts'] = np.asarray(st, np.int64)
    return out


def assert_named(got, want):
    assert set(got) == set(want)
    for name, w in want.items():
        same_bits(got[name], w, name)


def test_temporal_statistics_from_host_arrays():
    from dl4ds_amd.temporal import temporal_statistics
    y, _, years, thr = host_case()
    st = [0, 25, 26, 60]
    for thresholds, op in (((1.0, 3.0, 0.0), '>='), (thr, '<'), ((), '>=')):
        want = named_ref(y, None, st, LAGS, thresholds, ('>=', '>', '<', '<=').index(op), 8, 0)
        for batch_size in (None, 1, 3):
            assert_named(temporal_statistics(y, years, LAGS, thresholds, op, 8, batch_size=batch_size), want)
        assert_named(temporal_statistics(y.astype(np.float64), period_starts=st, lags=list(LAGS), thresholds=thresholds, op=op,
                                         spell_bins=8), want)
    assert want['transitions'].shape == (3, 0, 4) + GRID and want['acf'].shape == (3, 2) + GRID
    assert np.isfinite(want['acf']).any() and np.isnan(want['acf']).any()


def test_temporal_statistics_on_a_device_array_3d_input_and_mask():
    from dl4ds_amd.device import DeviceArray
    from dl4ds_amd.temporal import temporal_statistics
    y, _, years, thr = host_case()
    st = cases.starts(60, 'uneven')
    d_y = DeviceArray.from_numpy(y)
    assert_named(temporal_statistics(d_y, period_starts=st, lags=LAGS, thresholds=thr, spell_bins=5), named_ref(y, None, st, LAGS, thr, 0, 5, 0))
    np.testing.assert_array_equal(d_y.numpy().view(np.uint32), y.view(np.uint32))            # the input is left as it was
    flat = temporal_statistics(y[..., 0], years, thresholds=(1.0,))
    assert flat['sum'].shape == (3,) + GRID[:2] + (1,)
    assert_named(flat, named_ref(y[..., :1], None, [0, 25, 26, 60], (1,), (1.0,), 0, 16, 0))
    assert_named(temporal_statistics(DeviceArray.from_numpy(y[..., 0]), years, thresholds=(1.0,)), flat)
    mask = np.ones(GRID[:2], np.float32)
    mask[2:4, 1:5] = 0
    masked = y.copy()
    masked[:, 2:4, 1:5] = np.nan
    got = temporal_statistics(y, years, thresholds=(1.0,), mask=mask, batch_size=4)
    assert_named(got, named_ref(masked, None, [0, 25, 26, 60], (1,), (1.0,), 0, 16, 0))
    assert (got['n_valid'][:, 2:4, 1:5] == 0).all() and np.isfinite(y[:, 2, 2, 0]).any()
    with pytest.raises(ValueError):
        temporal_statistics(d_y, mask=mask)


def test_temporal_scores_end_to_end():
    from dl4ds_amd.device import DeviceArray
    from dl4ds_amd.temporal import temporal_scores
    y, p, years, thr = host_case()
    st = [0, 25, 26, 60]
    want_o, want_p = (named_ref(y, p, st, LAGS, thr, 1, 6, s) for s in (0, 1))
    for batch_size in (None, 1, 3):
        got = temporal_scores(y, p, years, LAGS, thr, '>', 6, batch_size=batch_size)
        assert set(got) == {'obs', 'pred', 'bias', 'mean_bias'}
        assert_named(got['obs'], want_o)
        assert_named(got['pred'], want_p)
    same_bits(got['obs']['n_valid'], got['pred']['n_valid'], 'common validity')
    assert set(got['bias']) == {'acf', 'p_event_given_event', 'p_event_given_nonevent', 'mean_event_spell', 'mean_nonevent_spell'}
    for name, b in got['bias'].items():
        same_bits(b, want_p[name] - want_o[name], name)
        same_bits(got['mean_bias'][name], b.mean(axis=0), name)
    dev = temporal_scores(DeviceArray.from_numpy(y), DeviceArray.from_numpy(p), years, LAGS, thr, '>', 6)
    assert_named(dev['obs'], want_o)
    assert_named(dev['pred'], want_p)
    with pytest.raises(ValueError):
        temporal_scores(y, p[:, :5])


def test_mann_kendall_and_trend_scores_end_to_end():
    from dl4ds_amd.device import DeviceArray
    from dl4ds_amd.temporal import mann_kendall, mann_kendall_from_counts, trend_scores
    v = cases.trend_values(33, 84, seed=4)
    n, (s, ties), sen = ref.trend(v)
    want = mann_kendall_from_counts(n.reshape(GRID), s.reshape(GRID), ties.reshape(GRID), sen.reshape(GRID))
    v4 = v.reshape((33,) + GRID)
    for batch_size in (None, 1, 3):
        assert_named(mann_kendall(v4, batch_size=batch_size), want)
    assert_named(mann_kendall(DeviceArray.from_numpy(v4)), want)
    flat = mann_kendall(v4[..., 0])
    assert flat['s'].shape == GRID[:2] + (1,)
    same_bits(flat['sen_slope'][..., 0], want['sen_slope'][..., 0], '3-D input')
    mask = np.ones(GRID[:2], np.float32)
    mask[1:3, 2:4] = 0
    got = mann_kendall(v4, mask=mask)
    assert (got['n'][1:3, 2:4] == 0).all() and np.isnan(got['sen_slope'][1:3, 2:4]).all() and np.isnan(got['z'][1:3, 2:4]).all()
    same_bits(got['sen_slope'][0], want['sen_slope'][0], 'outside the mask')
    scores = trend_scores(v4, v4 + np.arange(33).reshape(33, 1, 1, 1) * 0.5)
    assert_named(scores['obs'], want)
    np.testing.assert_allclose(scores['slope_bias'][np.isfinite(want['sen_slope'])], 0.5, rtol=0, atol=1e-12)
    assert 0.0 < scores['sign_agreement'] < 1.0


# ------------------------------------------------------------------------------------------------------------------ refusals
def test_abi_refusals():
    from dl4ds_amd import _lib
    from dl4ds_amd.device import Buffers
    lib = _lib.lib()

    def refused(status, word):
        assert status != 0
        message = lib.dl4ds_last_error().decode()
        assert word in message, message

    with Buffers() as buf:
        x, thr = buf.zeros((8, 6)), buf.zeros((4,))
        outs = (buf.alloc((8, 6), np.int32), buf.alloc((8, 2, 2, 6), np.float64), buf.alloc((8, 4, 6), np.int32),
                buf.alloc((8, 2, 4, 3, 6), np.float64), buf.alloc((8, 2, 4, 4, 6), np.int32), buf.alloc((8, 2, 4, 2, 32, 6), np.int32))
        ptrs = tuple(o.ptr for o in outs)

        def call(N=8, per=6, st=(0, 3, 8), P=None, lags=(1, 2), L=None, T=2, op=0, bins=16, yp=x.ptr, pp=x.ptr, tp=thr.ptr,
                 null_starts=False, null_lags=False, outs=ptrs):
            keep, kl = np.ascontiguousarray(st, np.int64), np.ascontiguousarray(lags, np.int32)
            return lib.dl4ds_temporal(yp, pp, N, per, None if null_starts else keep.ctypes.data, len(keep) - 1 if P is None else P,
                                      None if null_lags else kl.ctypes.data, len(kl) if L is None else L, tp, T, 0, op, bins, *outs)
        no_lag, no_thr = ptrs[:2] + (None, None) + ptrs[4:], ptrs[:4] + (None, None)
        assert call() == 0
        assert call(st=np.arange(9), pp=None) == 0
        assert call(lags=(), null_lags=True, outs=no_lag) == 0
        assert call(T=0, tp=None, outs=no_thr) == 0
        refused(call(P=0), 'at least one period')
        refused(call(P=-1), 'at least one period')
        refused(call(st=(1, 3, 8)), 'strictly increasing')
        refused(call(st=(0, 3, 7)), 'strictly increasing')
        refused(call(st=(0, 3, 3, 8)), 'strictly increasing')
        refused(call(st=(0, 5, 3, 8)), 'strictly increasing')
        refused(call(st=np.arange(10), N=8), 'strictly increasing')
        refused(call(N=0, st=(0, 0)), 'empty')
        refused(call(per=0), 'empty')
        refused(call(N=1 << 31, st=(0, 1 << 31)), '2^31')
        refused(call(L=-1), 'lags')
        refused(call(lags=(1, 2, 3, 4, 5)), 'lags')
        refused(call(lags=(0, 2)), 'lags must be')
        refused(call(lags=(1, 33)), 'lags must be')
        refused(call(lags=(2, 2)), 'lags must be')
        refused(call(lags=(3, 2)), 'lags must be')
        refused(call(T=-1), 'thresholds')
        refused(call(T=5), 'thresholds')
        refused(call(bins=0), 'spell_bins')
        refused(call(bins=33), 'spell_bins')
        refused(call(op=-1), 'op must be')
        refused(call(op=4), 'op must be')
        refused(call(yp=None), 'null')
        refused(call(null_starts=True), 'null')
        refused(call(null_lags=True), 'null lags')
        refused(call(tp=None), 'null thresholds')
        refused(call(lags=(), null_lags=True), 'at least one lag')
        refused(call(lags=(), null_lags=True, outs=ptrs[:2] + (ptrs[2], None) + ptrs[4:]), 'at least one lag')
        refused(call(T=0, tp=None), 'at least one threshold')
        refused(call(T=0, tp=None, outs=ptrs[:4] + (None, ptrs[5])), 'at least one threshold')
        refused(call(outs=(None,) * 6), 'all six outputs')

        v = buf.zeros((4, 6), np.float64)
        n, mk, sen = buf.alloc((6,), np.int32), buf.alloc((2, 6), np.int64), buf.alloc((6,), np.float64)
        assert lib.dl4ds_trend(v.ptr, 4, 6, n.ptr, mk.ptr, sen.ptr) == 0
        refused(lib.dl4ds_trend(v.ptr, 0, 6, n.ptr, mk.ptr, sen.ptr), '128 periods')
        refused(lib.dl4ds_trend(v.ptr, 129, 6, n.ptr, mk.ptr, sen.ptr), '128 periods')
        refused(lib.dl4ds_trend(v.ptr, 4, 0, n.ptr, mk.ptr, sen.ptr), 'empty')
        refused(lib.dl4ds_trend(None, 4, 6, n.ptr, mk.ptr, sen.ptr), 'null')
        refused(lib.dl4ds_trend(v.ptr, 4, 6, None, None, None), 'all three outputs')
