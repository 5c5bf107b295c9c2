"""Climate indices (dl4ds_amd/indices.py) without a GPU: the numpy restatement tests/indices_ref.py, which
the device is compared with bit for bit in tests/test_gpu_indices.py, against independent statements (itertools.groupby run
lengths, a plain Python float loop for the sums, np.nanmax / np.nanmin) and hand-worked sequences; the argument checks, the
conversion of labels to period starts, the wrappers' arithmetic and the lazy exports."""
import itertools

import numpy as np
import pytest

from tests import indices_cases as cases
from tests import indices_ref as ref

PY_OPS = (lambda v, t: v >= t, lambda v, t: v > t, lambda v, t: v < t, lambda v, t: v <= t)


def plain(col, thr, op, window):
    """one cell of one period in plain Python: -> (n_valid, the six event integers, max, min, sum, largest window sum, event sum)"""
    col = [float(np.float32(0) if v == 0 else v) for v in col]
    ok = [np.isfinite(v) for v in col]
    state = ['x' if not k else ('e' if PY_OPS[op](np.float32(v), np.float32(thr)) else 'n') for v, k in zip(col, ok)]
    runs = [(key, len(list(g))) for key, g in itertools.groupby(state)]
    events = [i for i, s in enumerate(state) if s == 'e']
    six = [len(events), max([n for k, n in runs if k == 'e'], default=0), max([n for k, n in runs if k == 'n'], default=0),
           sum(1 for k, _ in runs if k == 'e'), events[0] if events else -1, events[-1] if events else -1]
    if not np.isfinite(thr):
        six = [-1] * 6
    vals = [v for v, k in zip(col, ok) if k]
    total = float('nan')
    for j, v in enumerate(vals):
        total = v if j == 0 else total + v
    esum = 0.0
    for i in events:
        esum = esum + col[i]
    best = float('nan')
    for i in range(len(col) - window + 1):
        if all(ok[i:i + window]):
            s = col[i]
            for v in col[i + 1:i + window]:
                s = s + v
            best = s if not best == best or s > best else best
    return (len(vals), six, np.nanmax(np.where(ok, col, np.nan)) if vals else np.nan,
            np.nanmin(np.where(ok, col, np.nan)) if vals else np.nan, total, best, esum if np.isfinite(thr) else float('nan'))


def same(a, b):
    a, b = np.float64(a), np.float64(b)
    return a.view(np.uint64) == b.view(np.uint64) or (np.isnan(a) and np.isnan(b))


@pytest.mark.parametrize('op', [0, 1, 2, 3])
@pytest.mark.parametrize('kind', cases.PERIOD_KINDS)
def test_restatement_against_plain_python(kind, op):
    n, cells, window = 23, 9, 3
    x = cases.spoiled(n, cells, seed=op)
    st = cases.starts(n, kind)
    thr = cases.cell_thresholds(2, cells, seed=op)
    valid, event, ext, sums = ref.climate_indices(x, st, thr, op, window)
    assert valid.dtype == np.int32 and event.dtype == np.int32 and ext.dtype == np.float32 and sums.dtype == np.float64
    assert event.shape == (len(st) - 1, 2, 6, cells) and sums.shape == (len(st) - 1, 4, cells)
    for p in range(len(st) - 1):
        for c in range(cells):
            for t in range(2):
                nv, six, mx, mn, total, best, esum = plain(x[st[p]:st[p + 1], c], thr[t, c], op, window)
                assert valid[p, c] == nv
                assert list(event[p, t, :, c]) == six, (p, c, t)
                assert same(ext[p, 0, c], mx) and same(ext[p, 1, c], mn)
                assert same(sums[p, 0, c], total) and same(sums[p, 1, c], best) and same(sums[p, 2 + t, c], esum), (p, c, t)


def one_cell(values, starts=None, thr=(1.0,), op=0, window=2):
    x = np.asarray(values, np.float32)[:, None]
    return ref.climate_indices(x, np.array([0, len(values)] if starts is None else starts, np.int64), np.asarray(thr, np.float32),
                               op, window)


def test_hand_worked_all_events_and_no_event():
    valid, event, ext, sums = one_cell([2, 3, 4, 5])
    assert valid[0, 0] == 4 and list(event[0, 0, :, 0]) == [4, 4, 0, 1, 0, 3]
    assert ext[0, 0, 0] == 5 and ext[0, 1, 0] == 2 and list(sums[0, :, 0]) == [14.0, 9.0, 14.0]
    valid, event, ext, sums = one_cell([0.5, 0, 0.25])
    assert list(event[0, 0, :, 0]) == [0, 0, 3, 0, -1, -1] and list(sums[0, :, 0]) == [0.75, 0.5, 0.0]


def test_hand_worked_run_cut_by_a_period_boundary():
    _, event, _, sums = one_cell([0, 2, 2, 2, 2, 0], starts=[0, 3, 6], window=3)
    assert list(event[0, 0, :, 0]) == [2, 2, 1, 1, 1, 2] and list(event[1, 0, :, 0]) == [2, 2, 1, 1, 0, 1]
    assert list(sums[:, 1, 0]) == [4.0, 4.0]                       # windows lie inside one period: never 2 + 2 + 2
    _, whole, _, wsum = one_cell([0, 2, 2, 2, 2, 0], window=3)
    assert list(whole[0, 0, :, 0]) == [4, 4, 1, 1, 1, 4] and wsum[0, 1, 0] == 6.0


def test_hand_worked_run_ended_by_nan():
    valid, event, ext, sums = one_cell([3, 3, np.nan, 3, 0, 0, np.inf, 0], window=2)
    assert valid[0, 0] == 6 and list(event[0, 0, :, 0]) == [3, 2, 2, 2, 0, 3]
    assert list(sums[0, :, 0]) == [9.0, 6.0, 9.0] and ext[0, 0, 0] == 3 and ext[0, 1, 0] == 0


def test_hand_worked_short_periods_and_wide_windows():
    valid, event, ext, sums = one_cell([7], window=1)
    assert list(event[0, 0, :, 0]) == [1, 1, 0, 1, 0, 0] and list(sums[0, :, 0]) == [7.0, 7.0, 7.0]
    valid, event, ext, sums = one_cell([7, 8, 9], window=4)        # `window` larger than the period: no window sum
    assert np.isnan(sums[0, 1, 0]) and sums[0, 0, 0] == 24.0
    valid, event, ext, sums = one_cell([np.nan, np.nan], window=1)
    assert valid[0, 0] == 0 and np.isnan(ext[0, :, 0]).all() and np.isnan(sums[0, :2, 0]).all() and sums[0, 2, 0] == 0.0
    assert list(event[0, 0, :, 0]) == [0, 0, 0, 0, -1, -1]
    _, event, _, sums = one_cell([1, 2], thr=(np.nan,))            # no threshold here
    assert list(event[0, 0, :, 0]) == [-1] * 6 and np.isnan(sums[0, 2, 0]) and sums[0, 0, 0] == 3.0


@pytest.mark.parametrize('op, is_event', [(0, True), (1, False), (2, False), (3, True)])
@pytest.mark.parametrize('thr', [0.0, -0.0])
def test_negative_zero_against_a_threshold_of_zero(op, is_event, thr):
    valid, event, ext, sums = one_cell([-0.0, 0.0, -0.0], thr=(thr,), op=op, window=2)
    assert event[0, 0, 0, 0] == (3 if is_event else 0) and event[0, 0, 2, 0] == (0 if is_event else 3)
    for v in (ext[0, 0, 0], ext[0, 1, 0]):
        assert v == 0 and not np.signbit(v)                        # a zero is written as +0.0
    for v in sums[0, :, 0]:
        assert v == 0 and not np.signbit(v)


# --------------------------------------------------------------------------------------------------------------- the host layer
def test_lazy_exports():
    import dl4ds_amd
    from dl4ds_amd import indices
    for name in ('climate_indices', 'precipitation_indices', 'temperature_indices', 'percentile_threshold', 'index_scores',
                 'check_index_args'):
        assert getattr(dl4ds_amd, name) is getattr(indices, name)
    assert indices.INDEX_OPS == ('>=', '>', '<', '<=') and indices.EVENT_NAMES == ref.EVENT_ROWS


def test_labels_to_period_starts():
    from dl4ds_amd.indices import period_starts_from_labels
    years = np.array([1990, 1990, 1990, 1991, 1993, 1993])
    np.testing.assert_array_equal(period_starts_from_labels(years), [0, 3, 4, 6])
    np.testing.assert_array_equal(period_starts_from_labels(np.array([7])), [0, 1])
    np.testing.assert_array_equal(period_starts_from_labels(np.arange(4)), [0, 1, 2, 3, 4])
    assert period_starts_from_labels(years).dtype == np.int64
    for bad in (np.array([2, 1]), np.array([1.0, 2.0]), np.zeros((2, 2), int), np.array([], int)):
        with pytest.raises(ValueError):
            period_starts_from_labels(bad)


def test_check_index_args_accepts():
    from dl4ds_amd.indices import check_index_args
    shape = (6, 3, 4, 2)
    st, thr, op = check_index_args(shape)
    assert list(st) == [0, 6] and st.dtype == np.int64 and thr.dtype == np.float32 and list(thr) == [1.0] and op == 0
    st, thr, op = check_index_args(shape, periods=[1, 1, 2, 2, 2, 5], thresholds=(20, 1, 1, np.nan), op='<=', window=32, batch_size=2)
    assert list(st) == [0, 2, 5, 6] and thr.shape == (4,) and op == 3
    st, thr, op = check_index_args(shape, period_starts=[0, 1, 6], thresholds=np.ones((2, 3, 4, 2)), op='<', window=1)
    assert list(st) == [0, 1, 6] and thr.shape == (2, 3, 4, 2) and op == 2
    assert check_index_args(shape, thresholds=2.5)[1].shape == (1,)
    assert check_index_args((6, 3, 4, 1), thresholds=np.ones((2, 3, 4)))[1].shape == (2, 3, 4, 1)


@pytest.mark.parametrize('kw, message', [
    (dict(shape=(6, 3, 4)), 'non-empty'),
    (dict(shape=(0, 3, 4, 2)), 'non-empty'),
    (dict(shape=(6, 3, 0, 2)), 'non-empty'),
    (dict(shape=(1 << 31, 1, 1, 1)), '2^31'),
    (dict(op='=='), '`op`'),
    (dict(op=0), '`op`'),
    (dict(window=0), '`window`'),
    (dict(window=33), '`window`'),
    (dict(window=2.0), '`window`'),
    (dict(window=True), '`window`'),
    (dict(batch_size=0), '`batch_size`'),
    (dict(periods=[0] * 6, period_starts=[0, 6]), 'not both'),
    (dict(periods=[0] * 5), 'labels for 6'),
    (dict(periods=[0, 1, 0, 1, 2, 3]), 'non-decreasing'),
    (dict(periods=[0.0] * 6), 'integer'),
    (dict(period_starts=[0]), 'P + 1'),
    (dict(period_starts=[0.0, 6.0]), 'P + 1'),
    (dict(period_starts=[[0, 6]]), 'P + 1'),
    (dict(period_starts=[1, 6]), 'strictly increasing'),
    (dict(period_starts=[0, 5]), 'strictly increasing'),
    (dict(period_starts=[0, 3, 3, 6]), 'strictly increasing'),
    (dict(period_starts=[0, 4, 2, 6]), 'strictly increasing'),
    (dict(thresholds=()), 'between 1 and 4'),
    (dict(thresholds=(1, 2, 3, 4, 5)), 'between 1 and 4'),
    (dict(thresholds=np.ones((2, 3, 4, 1))), '(T, H, W, C)'),
    (dict(thresholds=np.ones((2, 2))), '(T, H, W, C)'),
    (dict(thresholds=np.ones((5, 3, 4, 2))), 'between 1 and 4'),
    (dict(thresholds=('a',)), 'numbers'),
])
def test_check_index_args_refuses(kw, message):
    from dl4ds_amd.indices import check_index_args
    kw = dict(dict(shape=(6, 3, 4, 2)), **kw)
    with pytest.raises(ValueError) as e:
        check_index_args(**kw)
    assert message in str(e.value), str(e.value)


def fake_result():
    """a `climate_indices` result of P = 2 periods on a (1, 2, 1) grid at three thresholds, written by hand"""
    g = (2, 1, 2, 1)
    r = {'n_valid': np.array([10, 10, 9, 0], np.int32).reshape(g),
         'max': np.array([30, 12, 4, np.nan], np.float32).reshape(g), 'min': np.array([0, 0, 0, np.nan], np.float32).reshape(g),
         'sum': np.array([60.0, 20.0, 4.5, np.nan]).reshape(g), 'max_window_sum': np.array([45.0, 15.0, 4.5, np.nan]).reshape(g),
         'period_starts': np.array([0, 10, 20], np.int64)}
    per_t = {'n_event': [[4, 3, 2, 0], [2, 1, 0, 0], [1, 0, 0, 0]], 'longest_event_run': [[3, 2, 1, 0], [2, 1, 0, 0], [1, 0, 0, 0]],
             'longest_nonevent_run': [[5, 4, 6, 0], [7, 9, 9, 0], [9, 10, 9, 0]], 'event_sum': [[58.0, 18.0, 4.0, 0.0], [50.0, 12.0, 0, 0],
                                                                                                 [30.0, 0, 0, 0]]}
    for name, rows in per_t.items():
        a = np.array(rows, np.float64 if name == 'event_sum' else np.int32)             # [T][P * cells]
        r[name] = np.ascontiguousarray(a.reshape(3, 2, 1, 2, 1).transpose(1, 0, 2, 3, 4))
    return r


def test_precipitation_names_on_a_fake_result():
    from dl4ds_amd.indices import _precipitation_from
    out = _precipitation_from(fake_result(), 5)
    flat = {k: np.asarray(v).reshape(-1) for k, v in out.items() if k != 'period_starts'}
    np.testing.assert_array_equal(flat['rx1day'], np.array([30, 12, 4, np.nan], np.float32))
    np.testing.assert_array_equal(flat['rx5day'], [45.0, 15.0, 4.5, np.nan])
    np.testing.assert_array_equal(flat['prcptot'], [60.0, 20.0, 4.5, np.nan])
    np.testing.assert_array_equal(flat['sdii'], [58.0 / 4, 18.0 / 3, 4.0 / 2, np.nan])          # NaN without wet days
    np.testing.assert_array_equal(flat['r1mm'], [4, 3, 2, 0])
    np.testing.assert_array_equal(flat['r10mm'], [2, 1, 0, 0])
    np.testing.assert_array_equal(flat['r20mm'], [1, 0, 0, 0])
    np.testing.assert_array_equal(flat['cwd'], [3, 2, 1, 0])
    np.testing.assert_array_equal(flat['cdd'], [5, 4, 6, 0])
    assert out['sdii'].shape == (2, 1, 2, 1) and out['sdii'].dtype == np.float64 and 'rx3day' in _precipitation_from(fake_result(), 3)


def test_temperature_names_and_bias_on_fake_results():
    from dl4ds_amd.indices import _bias, _temperature_from
    lo, hi = fake_result(), fake_result()
    hi['n_event'] = hi['n_event'] + 1
    out = _temperature_from(lo, hi)
    np.testing.assert_array_equal(out['mean'].reshape(-1), [6.0, 2.0, 0.5, np.nan])
    np.testing.assert_array_equal(out['days_below'].reshape(-1), [4, 3, 2, 0])
    np.testing.assert_array_equal(out['days_above'].reshape(-1), [5, 4, 3, 1])
    np.testing.assert_array_equal(out['txx'].reshape(-1), np.array([30, 12, 4, np.nan], np.float32))
    np.testing.assert_array_equal(out['longest_run_below'].reshape(-1), [3, 2, 1, 0])
    pred = {k: (v + 2 if k != 'period_starts' else v) for k, v in out.items()}
    scores = _bias(out, pred)
    assert 'period_starts' not in scores and set(scores['mean']) == {'obs', 'pred', 'bias', 'mean_bias'}
    assert scores['mean']['bias'].dtype == np.float64 and scores['days_below']['bias'].dtype == np.float64
    np.testing.assert_array_equal(scores['mean']['bias'].reshape(-1), [2.0, 2.0, 2.0, np.nan])
    np.testing.assert_array_equal(scores['mean']['mean_bias'].reshape(-1), [2.0, np.nan])       # NaN stays NaN
    np.testing.assert_array_equal(scores['days_above']['mean_bias'].reshape(-1), [2.0, 2.0])


def test_refusals_before_the_device():
    from dl4ds_amd.indices import climate_indices, index_scores, percentile_threshold, precipitation_indices
    x = np.zeros((4, 2, 2, 1), np.float32)
    with pytest.raises(ValueError):
        climate_indices(x, window=40)
    with pytest.raises(ValueError):
        precipitation_indices(x, heavy=(10.0,))
    with pytest.raises(ValueError):
        index_scores(x, x, kind='wind')
    with pytest.raises(ValueError):
        percentile_threshold(x, 101)
