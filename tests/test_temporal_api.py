"""Temporal verification (dl4ds_amd/temporal.py) without a GPU: the numpy restatement
tests/temporal_ref.py, which the device is compared with bit for bit in tests/test_gpu_temporal.py, against independent statements
(itertools.groupby run lengths for histograms and transitions, a plain Python float loop for every sum, a brute-force double loop
with np.median and scipy.stats.theilslopes for the trend) and hand-worked sequences; `temporal_from_sums` against the two-pass
centred formulas; the argument checks, the wrappers' arithmetic on a made-up device result and the lazy exports."""
import itertools
import math

import numpy as np
import pytest

from tests import temporal_cases as cases
from tests import temporal_ref as ref

PY_OPS = (lambda v, t: v >= t, lambda v, t: v > t, lambda v, t: v < t, lambda v, t: v <= t)


def plain(cols, thr, op, lags, bins):
    """one cell of one period in plain Python.  cols: the S columns -> (n_valid, per series (sum, sum_sq), per lag the pair count,
    per series and lag (sum a, sum b, sum ab), per series the four transition counts, per series the two histograms)"""
    cols = [[float(np.float32(0) if v == 0 else v) for v in col] for col in cols]
    n = len(cols[0])
    ok = [all(math.isfinite(col[i]) for col in cols) for i in range(n)]
    moments, lag_sums, transitions, hists = [], [], [], []
    pairs = [sum(1 for i in range(n - k) if ok[i] and ok[i + k]) for k in lags]
    for col in cols:
        s = q = 0.0
        for v, k in zip(col, ok):
            if k:
                s, q = s + v, q + v * v
        moments.append((s, q))
        per_lag = []
        for k in lags:
            a = b = ab = 0.0
            for i in range(n - k):
                if ok[i] and ok[i + k]:
                    a, b, ab = a + col[i], b + col[i + k], ab + col[i] * col[i + k]
            per_lag.append((a, b, ab))
        lag_sums.append(per_lag)
        state = ['x' if not k else ('e' if PY_OPS[op](np.float32(v), np.float32(thr)) else 'n') for v, k in zip(col, ok)]
        tr = [sum(1 for u, w in zip(state, state[1:]) if (u, w) == pair) for pair in (('n', 'n'), ('n', 'e'), ('e', 'n'), ('e', 'e'))]
        hist = [[0] * bins, [0] * bins]
        for key, g in itertools.groupby(state):
            if key != 'x':
                hist['en'.index(key)][min(len(list(g)), bins) - 1] += 1
        if not np.isfinite(thr):
            tr, hist = [-1] * 4, [[-1] * bins, [-1] * bins]
        transitions.append(tr)
        hists.append(hist)
    return sum(ok), moments, pairs, lag_sums, transitions, hists


def bits(a):
    return np.float64(a).view(np.uint64)


@pytest.mark.parametrize('op', [0, 1, 2, 3])
@pytest.mark.parametrize('kind', cases.PERIOD_KINDS)
@pytest.mark.parametrize('S', [1, 2])
def test_restatement_against_plain_python(S, kind, op):
    n, cells, lags, bins = 41, 9, (1, 3, 32), 3
    y, p = cases.series(n, cells, seed=op), cases.second(n, cells, seed=op) if S == 2 else None
    st = cases.starts(n, kind)
    thr = cases.cell_thresholds(2, cells, seed=op)
    valid, moment, pair, lag, trans, spell = ref.temporal(y, p, st, lags, thr, op, bins)
    assert valid.dtype == pair.dtype == trans.dtype == spell.dtype == np.int32 and moment.dtype == lag.dtype == np.float64
    P = len(st) - 1
    assert moment.shape == (P, S, 2, cells) and lag.shape == (P, S, 3, 3, cells) and spell.shape == (P, S, 2, 2, bins, cells)
    for q in range(P):
        for c in range(cells):
            cols = [a[st[q]:st[q + 1], c] for a in ((y,) if p is None else (y, p))]
            for t in range(2):
                nv, moments, pairs, lag_sums, transitions, hists = plain(cols, thr[t, c], op, lags, bins)
                assert valid[q, c] == nv and list(pair[q, :, c]) == pairs
                for s in range(S):
                    assert bits(moment[q, s, 0, c]) == bits(moments[s][0]) and bits(moment[q, s, 1, c]) == bits(moments[s][1])
                    for li in range(len(lags)):
                        assert [bits(v) for v in lag[q, s, li, :, c]] == [bits(v) for v in lag_sums[s][li]], (q, c, s, li)
                    assert list(trans[q, s, t, :, c]) == transitions[s], (q, c, s, t)
                    assert spell[q, s, t, :, :, c].tolist() == hists[s], (q, c, s, t)


def test_the_spike_shows_a_wrong_summation_order():
    """cell 2: 1e30 swallows what is added to it and is taken away again, so the ordered sum is the sum of what follows; a sorted
    or pairwise sum gives something else"""
    y = cases.series(97, 9, seed=0)
    moment = ref.temporal(y, None, [0, 97])[1]
    col = y[:, 2].astype(np.float64)
    big = float(np.float32(1e30))
    assert col[32] == big and col[64] == -big and np.isfinite(col[:64]).sum() > 40
    after = [v for v in col[65:] if math.isfinite(v)]
    assert moment[0, 0, 0, 2] == sum(after) > 0 and moment[0, 0, 0, 2] != np.sum(np.sort(col[np.isfinite(col)]))


def one_cell(values, starts=None, lags=(1,), thr=(1.0,), op=0, bins=4, second=None):
    y = np.asarray(values, np.float32)[:, None]
    p = None if second is None else np.asarray(second, np.float32)[:, None]
    return ref.temporal(y, p, np.array([0, len(values)] if starts is None else starts, np.int64), lags, np.asarray(thr, np.float32),
                        op, bins)


def test_hand_worked_all_events_and_no_event():
    valid, moment, pair, lag, trans, spell = one_cell([2, 3, 4, 5])
    assert valid[0, 0] == 4 and list(moment[0, 0, :, 0]) == [14.0, 54.0] and pair[0, 0, 0] == 3
    assert list(lag[0, 0, 0, :, 0]) == [9.0, 12.0, 6.0 + 12.0 + 20.0]
    assert list(trans[0, 0, 0, :, 0]) == [0, 0, 0, 3] and spell[0, 0, 0, :, :, 0].tolist() == [[0, 0, 0, 1], [0, 0, 0, 0]]
    valid, moment, pair, lag, trans, spell = one_cell([0.5, 0, 0.25])
    assert list(trans[0, 0, 0, :, 0]) == [2, 0, 0, 0] and spell[0, 0, 0, :, :, 0].tolist() == [[0, 0, 0, 0], [0, 0, 1, 0]]


def test_hand_worked_run_cut_by_a_period_boundary_and_run_ended_by_nan():
    *_, pair, lag, trans, spell = one_cell([0, 2, 2, 2, 2, 0], starts=[0, 3, 6])
    assert spell[:, 0, 0, 0, :, 0].tolist() == [[0, 1, 0, 0], [0, 1, 0, 0]]      # never one run of four
    assert list(trans[0, 0, 0, :, 0]) == [0, 1, 0, 1] and list(trans[1, 0, 0, :, 0]) == [0, 0, 1, 1] and list(pair[:, 0, 0]) == [2, 2]
    *_, whole = one_cell([0, 2, 2, 2, 2, 0])
    assert whole[0, 0, 0, 0, :, 0].tolist() == [0, 0, 0, 1] and whole[0, 0, 0, 1, :, 0].tolist() == [2, 0, 0, 0]
    valid, moment, pair, lag, trans, spell = one_cell([3, 3, np.nan, 3, 0, 0, np.inf, 0])
    assert valid[0, 0] == 6 and pair[0, 0, 0] == 3 and list(trans[0, 0, 0, :, 0]) == [1, 0, 1, 1]
    assert spell[0, 0, 0, :, :, 0].tolist() == [[1, 1, 0, 0], [1, 1, 0, 0]]
    assert list(lag[0, 0, 0, :, 0]) == [6.0, 3.0, 9.0]


def test_hand_worked_period_of_length_one_and_lag_beyond_the_period():
    valid, moment, pair, lag, trans, spell = one_cell([7], lags=(1, 32))
    assert valid[0, 0] == 1 and list(moment[0, 0, :, 0]) == [7.0, 49.0] and list(pair[0, :, 0]) == [0, 0]
    assert (lag == 0).all() and (trans == 0).all() and spell[0, 0, 0, :, :, 0].tolist() == [[1, 0, 0, 0], [0, 0, 0, 0]]
    valid, moment, pair, lag, trans, spell = one_cell([1, 2, 3], lags=(2, 3))
    assert list(pair[0, :, 0]) == [1, 0] and list(lag[0, 0, 0, :, 0]) == [1.0, 3.0, 3.0] and (lag[0, 0, 1] == 0).all()
    *_, trans, spell = one_cell([1, 2], thr=(np.nan,))
    assert (trans == -1).all() and (spell == -1).all()


@pytest.mark.parametrize('length', [3, 4, 5])
def test_hand_worked_runs_around_the_last_bin(length):
    """B = 4: a run of length B - 1, B and B + 1"""
    *_, spell = one_cell([0] + [2] * length + [0], bins=4)
    assert spell[0, 0, 0, 0, :, 0].tolist() == [0, 0, int(length == 3), int(length >= 4)]
    assert spell[0, 0, 0, 1, :, 0].tolist() == [2, 0, 0, 0]


@pytest.mark.parametrize('op, is_event', [(0, True), (1, False), (2, False), (3, True)])
@pytest.mark.parametrize('thr', [0.0, -0.0])
def test_negative_zero_against_a_threshold_of_zero(op, is_event, thr):
    valid, moment, pair, lag, trans, spell = one_cell([-0.0, 0.0, -0.0], thr=(thr,), op=op)
    assert list(trans[0, 0, 0, :, 0]) == ([0, 0, 0, 2] if is_event else [2, 0, 0, 0])
    assert spell[0, 0, 0, 0 if is_event else 1, 2, 0] == 1 and spell.sum() == 1
    for v in list(moment.ravel()) + list(lag.ravel()):
        assert v == 0 and not np.signbit(v)


def test_common_validity():
    valid, moment, pair, lag, trans, spell = one_cell([1, 2, np.nan, 4, 5], second=[1, np.inf, 3, 4, 5])
    assert valid[0, 0] == 3 and list(moment[0, :, 0, 0]) == [10.0, 10.0] and pair[0, 0, 0] == 1
    assert list(lag[0, 0, 0, :, 0]) == [4.0, 5.0, 20.0] and spell[0, :, 0, 0, :, 0].tolist() == [[1, 1, 0, 0]] * 2


# ------------------------------------------------------------------------------------------------------------------------ trend
def brute_trend(col):
    """one cell: (n, S, the tie term, Sen's slope) by a double loop, collections of equal values and np.median"""
    col = [float(v) for v in col]
    idx = [i for i, v in enumerate(col) if math.isfinite(v)]
    s, slopes = 0, []
    for a, i in enumerate(idx):
        for j in idx[a + 1:]:
            s += (col[j] > col[i]) - (col[j] < col[i])
            slopes.append((col[j] - col[i]) / (j - i))
    groups = [len(list(g)) for _, g in itertools.groupby(sorted(col[i] + 0.0 for i in idx))]
    ties = sum(g * (g - 1) * (2 * g + 5) for g in groups)
    return len(idx), s, ties, float(np.median(slopes)) + 0.0 if slopes else float('nan')


@pytest.mark.parametrize('P', [1, 2, 3, 4, 5, 12, 33])
def test_trend_restatement_against_brute_force(P):
    v = cases.trend_values(P, 29, seed=P)
    n, (s, ties), sen = ref.trend(v)
    assert n.dtype == np.int32 and s.dtype == np.int64 and sen.dtype == np.float64
    for c in range(29):
        bn, bs, bt, bsen = brute_trend(list(v[:, c]))
        assert (n[c], s[c], ties[c]) == (bn, bs, bt), c
        assert bits(sen[c]) == bits(bsen) or (np.isnan(sen[c]) and np.isnan(bsen)), (c, sen[c], bsen)


def test_trend_against_scipy_on_gap_free_series():
    stats = pytest.importorskip('scipy.stats')
    rng = np.random.default_rng(3)
    v = np.round(rng.normal(0, 3, (30, 11)) + 0.1 * np.arange(30)[:, None], 1)
    sen = ref.trend(v)[2]
    for c in range(11):
        assert sen[c] == stats.theilslopes(v[:, c], np.arange(30.0))[0]


def test_trend_hand_worked():
    nan = np.nan
    v = np.array([[2.5, nan, nan, 1.0, 0.0, -0.0, 1.0],
                  [2.5, nan, 4.0, nan, 1.0, 0.0, 3.0],
                  [2.5, nan, nan, nan, 2.0, -0.0, 2.0],
                  [2.5, nan, nan, 4.0, 3.0, 0.0, 2.0]])
    n, (s, ties), sen = ref.trend(v)
    assert list(n) == [4, 0, 1, 2, 4, 4, 4]
    assert list(s) == [0, 0, 0, 1, 6, 0, 1]                                     # monotone: n(n-1)/2
    assert list(ties) == [4 * 3 * 13, 0, 0, 0, 0, 4 * 3 * 13, 2 * 1 * 9]
    assert sen[0] == 0 and not np.signbit(sen[0]) and np.isnan(sen[1]) and np.isnan(sen[2])
    assert sen[3] == 1.0 and sen[4] == 1.0 and sen[5] == 0 and not np.signbit(sen[5])        # the gap keeps its spacing: 3 / 3
    assert sen[6] == (0 + 1 / 3) * 0.5                                          # slopes -1, -.5, 0, 1/3, .5, 2: even M
    from dl4ds_amd.temporal import mann_kendall_from_counts
    r = mann_kendall_from_counts(n, s, ties, sen)
    assert r['var_s'][0] == 0 and np.isnan(r['z'][0]) and np.isnan(r['p_value'][0])           # all tied
    assert r['z'][4] == 5 / math.sqrt(4 * 3 * 13 / 18) and r['p_value'][4] == math.erfc(r['z'][4] / math.sqrt(2))
    assert r['z'][3] == 0 and r['p_value'][3] == 1.0 and r['var_s'][3] == 1.0                 # s = 1: the correction takes it to 0
    assert r['var_s'][6] == (4 * 3 * 13 - 18) / 18


# --------------------------------------------------------------------------------------------------------------- the host layer
def test_lazy_exports():
    import dl4ds_amd
    from dl4ds_amd import temporal
    for name in ('temporal_statistics', 'temporal_scores', 'temporal_from_sums', 'mann_kendall', 'trend_scores', 'check_temporal_args'):
        assert getattr(dl4ds_amd, name) is getattr(temporal, name)
    assert temporal.RAW_NAMES == ref.RAW_NAMES and temporal.TEMPORAL_MAX_LAG == cases.RING


def test_check_temporal_args():
    from dl4ds_amd.temporal import check_temporal_args
    shape = (10, 3, 4, 1)
    starts, lags, thr, op = check_temporal_args(shape)
    assert list(starts) == [0, 10] and list(lags) == [1] and lags.dtype == np.int32 and thr.shape == (0,) and op == 0
    starts, lags, thr, op = check_temporal_args(shape, np.repeat([1, 2], 5), [1, 2, 5, 32], (1.0, 2.0), '<', 32, 2)
    assert list(starts) == [0, 5, 10] and list(lags) == [1, 2, 5, 32] and thr.dtype == np.float32 and list(thr) == [1, 2] and op == 2
    assert check_temporal_args(shape, lags=())[1].shape == (0,) and check_temporal_args(shape, lags=3)[1].tolist() == [3]
    assert check_temporal_args(shape, thresholds=np.ones((2, 3, 4)))[2].shape == (2, 3, 4, 1)
    for bad in (dict(lags=(0,)), dict(lags=(33,)), dict(lags=(2, 2)), dict(lags=(3, 1)), dict(lags=(1, 2, 3, 4, 5)), dict(lags=(1.0,)),
                dict(lags='a'), dict(lags=(True,)), dict(spell_bins=0), dict(spell_bins=33), dict(spell_bins=4.0), dict(op='=='),
                dict(thresholds=(1, 2, 3, 4, 5)), dict(thresholds=np.ones((1, 2, 2, 1))), dict(thresholds=('a',)),
                dict(batch_size=0), dict(periods=np.zeros(9, int)), dict(periods=np.array([2, 1] * 5)),
                dict(period_starts=[0, 5, 5, 10]), dict(period_starts=[0, 11]),
                dict(periods=np.zeros(10, int), period_starts=[0, 10])):
        with pytest.raises(ValueError):
            check_temporal_args(shape, **bad)
    for bad_shape in ((10, 3, 4), (0, 3, 4, 1), (1 << 31, 1, 1, 1)):
        with pytest.raises(ValueError):
            check_temporal_args(bad_shape)


def centred(col, lags):
    """one cell in two passes, centred, float64: (mean, variance, acf per lag)"""
    col = np.asarray(col, np.float64)
    m = col.mean()
    d = col - m
    den = (d * d).sum()
    return m, den / len(col), [(d[:-k] * d[k:]).sum() / den for k in lags]


def test_temporal_from_sums_against_the_two_pass_formula():
    """N = 3650 days, |mean| <= sigma: the data are halves drawn from -8 .. 8 with a small offset (mean about 0.5, sigma about
    4.9), persistent in time, so the raw-moment forms lose N * 2^-53 * (m^2 + sigma^2) / sigma^2, about 8e-13; the bound is 1e-10
    relative"""
    from dl4ds_amd.temporal import temporal_from_sums
    rng = np.random.default_rng(11)
    N, cells, lags = 3650, 6, (1, 2, 5, 32)
    x = (rng.integers(-16, 17, (N, cells)) / 2 + 0.5).astype(np.float32)
    keep = rng.random((N, cells)) < 0.5
    for i in range(1, N):
        x[i] = np.where(keep[i], x[i - 1], x[i])
    assert (np.abs(x.mean(axis=0)) <= x.std(axis=0)).all()
    flat = ref.temporal(x, None, [0, N], lags, (1.0,), 0, 8)
    got = temporal_from_sums(ref.named(flat, 0, (cells,)))
    for c in range(cells):
        m, var, acf = centred(x[:, c], lags)
        assert abs(got['mean'][0, c] - m) <= 1e-10 * abs(m) and abs(got['variance'][0, c] - var) <= 1e-10 * var
        for li in range(len(lags)):
            assert abs(got['acf'][0, li, c] - acf[li]) <= 1e-10 * abs(acf[li]), (c, li)
    assert (got['acf'][0, 0] > 0.3).all()


def fake_result():
    """raw outputs of P = 2 periods on a (1, 2, 1) grid, L = 1, T = 2, B = 3, written by hand"""
    g = (1, 2, 1)
    raw = {'n_valid': np.array([[4, 0], [3, 2]], np.int32).reshape((2,) + g),
           'sum': np.array([[8.0, 0.0], [6.0, 2.0]]).reshape((2,) + g),
           'sum_sq': np.array([[20.0, 0.0], [12.0, 2.0]]).reshape((2,) + g),
           'n_pairs': np.array([[3, 0], [2, 0]], np.int32).reshape((2, 1) + g),
           'lag_sums': np.array([[[5.0, 0.0], [7.0, 0.0], [9.0, 0.0]], [[4.0, 0.0], [4.0, 0.0], [8.0, 0.0]]]).reshape((2, 1, 3) + g),
           'transitions': np.array([[[[1, 0], [0, 0], [1, 0], [1, 0]], [[-1, 0], [-1, 0], [-1, 0], [-1, 0]]],
                                    [[[0, 1], [0, 0], [0, 0], [2, 0]], [[-1, 1], [-1, 0], [-1, 0], [-1, 0]]]], np.int32).reshape((2, 2, 4) + g),
           'spell_hist': np.zeros((2, 2, 2, 3) + g, np.int32)}
    h = raw['spell_hist']
    h[0, 0, 0, 1, 0, 0, 0], h[0, 0, 1, 1, 0, 0, 0] = 1, 1                       # period 0, cell 0, t 0: runs e e | n n
    h[1, 0, 0, 2, 0, 0, 0] = 1                                                  # period 1, cell 0, t 0: e e e
    h[1, :, 1, 1, 0, 1, 0] = 1                                                  # period 1, cell 1: n n under both t
    h[:, 1, :, :, 0, 0, 0] = -1                                                 # t 1 has no threshold in cell 0
    return raw


def test_temporal_from_sums_on_a_made_up_result():
    from dl4ds_amd.temporal import temporal_from_sums
    d = temporal_from_sums(fake_result())
    assert d['mean'].shape == (2, 1, 2, 1) and d['acf'].shape == (2, 1, 1, 2, 1) and d['p_event_given_event'].shape == (2, 2, 1, 2, 1)
    assert d['mean'][0, 0, 0, 0] == 2.0 and d['variance'][0, 0, 0, 0] == 1.0 and np.isnan(d['mean'][0, 0, 1, 0])
    assert d['acf'][0, 0, 0, 0, 0] == (9.0 - 2.0 * 12.0 + 3 * 4.0) / (20.0 - 16.0)
    assert np.isnan(d['acf'][1, 0, 0, 0, 0]) and np.isnan(d['acf'][0, 0, 0, 1, 0])            # denominator 0; no valid sample
    assert d['p_event_given_event'][0, 0, 0, 0, 0] == 0.5 and np.isnan(d['p_event_given_nonevent'][1, 0, 0, 0, 0])
    assert d['p_event_given_nonevent'][0, 0, 0, 0, 0] == 0.0 and d['p_event_given_event'][1, 0, 0, 0, 0] == 1.0
    assert d['mean_event_spell'][0, 0, 0, 0, 0] == 2.0 and d['mean_nonevent_spell'][0, 0, 0, 0, 0] == 2.0
    assert d['mean_event_spell'][1, 0, 0, 0, 0] == 3.0 and np.isnan(d['mean_nonevent_spell'][1, 0, 0, 0, 0])
    assert d['mean_nonevent_spell'][1, 0, 0, 1, 0] == 2.0 and np.isnan(d['mean_event_spell'][1, 0, 0, 1, 0])
    for name in ('p_event_given_event', 'p_event_given_nonevent', 'mean_event_spell', 'mean_nonevent_spell'):
        assert np.isnan(d[name][:, 1, 0, 0, 0]).all()                          # the device wrote -1


def test_scores_arithmetic_on_a_made_up_device_result(monkeypatch):
    from dl4ds_amd import temporal
    raw = fake_result()
    flat = [raw['n_valid'].reshape(2, 2), np.stack([np.stack([raw['sum'].reshape(2, 2), raw['sum_sq'].reshape(2, 2)], 1)] * 2, 1),
            raw['n_pairs'].reshape(2, 1, 2), np.stack([raw['lag_sums'].reshape(2, 1, 3, 2)] * 2, 1),
            np.stack([raw['transitions'].reshape(2, 2, 4, 2)] * 2, 1), np.stack([raw['spell_hist'].reshape(2, 2, 2, 3, 2)] * 2, 1)]
    flat[4] = flat[4].copy()
    flat[4][0, 1, 0, :, 0] = [0, 1, 1, 1]                                        # the prediction's transitions differ in one place
    seen = {}

    def fake(y, p, shape, starts, lags, thr, opn, bins, batch_size):
        seen.update(shape=shape, lags=list(lags), T=thr.shape[0], op=opn, bins=bins, two=p is not None)
        return flat
    monkeypatch.setattr(temporal, '_device_temporal', fake)
    x = np.zeros((5, 1, 2, 1), np.float32)
    r = temporal.temporal_scores(x, x, period_starts=[0, 2, 5], lags=(1,), thresholds=(1.0, 2.0), op='<=', spell_bins=3)
    assert seen == dict(shape=(5, 1, 2, 1), lags=[1], T=2, op=3, bins=3, two=True)
    assert set(r) == {'obs', 'pred', 'bias', 'mean_bias'} and set(r['bias']) == set(temporal.BIAS_NAMES)
    assert r['obs']['p_event_given_event'][0, 0, 0, 0, 0] == 0.5 and r['pred']['p_event_given_event'][0, 0, 0, 0, 0] == 0.5
    assert r['bias']['p_event_given_nonevent'][0, 0, 0, 0, 0] == 1.0 and r['bias']['acf'][0, 0, 0, 0, 0] == 0.0
    assert r['mean_bias']['p_event_given_nonevent'].shape == (2, 1, 2, 1) and np.isnan(r['mean_bias']['p_event_given_nonevent']).all()
    np.testing.assert_array_equal(r['obs']['period_starts'], [0, 2, 5])
    s = temporal.temporal_statistics(x[..., 0], lags=(1,), thresholds=(1.0, 2.0), spell_bins=3, period_starts=[0, 2, 5])
    assert seen['two'] is False and s['sum'].shape == (2, 1, 2, 1) and set(temporal.RAW_NAMES) < set(s)


def test_trend_scores_arithmetic(monkeypatch):
    from dl4ds_amd import temporal
    with pytest.raises(ValueError):
        temporal.mann_kendall(np.zeros((129, 2, 2)))
    with pytest.raises(ValueError):
        temporal.mann_kendall(np.zeros((4, 2, 2)), batch_size=0)
    slopes = iter([np.array([1.0, -1.0, np.nan, 0.0]), np.array([2.0, 1.0, 1.0, 0.0])])
    monkeypatch.setattr(temporal, 'mann_kendall', lambda v, mask=None: {'sen_slope': next(slopes)})
    r = temporal.trend_scores(None, None)
    assert r['sign_agreement'] == 0.5 and list(r['slope_bias'][[0, 1, 3]]) == [1.0, 2.0, 0.0] and np.isnan(r['slope_bias'][2])
    with pytest.raises(ValueError):
        temporal._trend_values(np.zeros((4, 2)))
    with pytest.raises(ValueError):
        temporal._trend_values(np.zeros((4, 2, 2)), mask=np.ones((3, 3)))
    v, shape = temporal._trend_values(np.ones((4, 2, 2)), mask=np.array([[1, 0], [1, 1]]))
    assert shape == (4, 2, 2, 1) and np.isnan(v[:, 0, 1, 0]).all() and np.isfinite(v[:, 1, 1, 0]).all()
