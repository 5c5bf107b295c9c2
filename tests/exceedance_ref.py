"""numpy restatement of the exceedance-probability verification of an ensemble (csrc/exceedance.hip, Model.score_exceedance,
metrics.exceedance_scores): broadcast float32 comparisons, np.add.at for the table, and every derived score from its textbook
definition in fractions.Fraction, rounded to float once.  Shared by tests/test_exceedance_api.py (CPU) and
tests/test_gpu_exceedance.py; imports nothing of the product."""
from fractions import Fraction

import numpy as np

NAN = float('nan')


def counts_ref(members, obs, thr):
    """members (K, N) + s, obs (N,) + s, thr (T,) or (T,) + s, all taken as float32 -> dict of
    valid, o (bool) and c (int64), each (N, T) + s;  count int16 (c, -1 where invalid);  table (T, K + 1, 2),
    cell (T, 4) + s and sample (N, T, 4) int64: n_valid, sum o, sum c, sum (c - K o)^2."""
    members, obs, thr = np.asarray(members, np.float32), np.asarray(obs, np.float32), np.asarray(thr, np.float32)
    K, N, s = members.shape[0], obs.shape[0], obs.shape[1:]
    T = thr.shape[0]
    tb = thr.reshape((1, T) + ((1,) * len(s) if thr.ndim == 1 else s))                        # (1, T) + s or ones
    fin = np.isfinite(obs) & np.isfinite(members).all(axis=0)                                 # (N,) + s
    valid = np.broadcast_to(fin[:, None] & np.isfinite(tb), (N, T) + s)
    with np.errstate(invalid='ignore'):
        o = np.broadcast_to(obs[:, None] >= tb, (N, T) + s)
        c = np.zeros((N, T) + s, np.int64)
        for k in range(K):
            c += members[k][:, None] >= tb
    table = np.zeros((T, K + 1, 2), np.int64)
    for t in range(T):
        v = valid[:, t]
        np.add.at(table[t], (c[:, t][v], o[:, t][v].astype(np.int64)), 1)
    oi = o.astype(np.int64)
    four = np.stack([valid.astype(np.int64), oi, c, (c - K * oi) ** 2], axis=2) * valid[:, :, None]      # (N, T, 4) + s
    cell = four.sum(axis=0)
    sample = four.reshape(N, T, 4, -1).sum(axis=3)
    count = np.where(valid, c, -1).astype(np.int16)
    return dict(valid=valid, o=o, c=c, count=count, table=table, cell=cell, sample=sample, K=K)


def _f(x):
    return NAN if x is None else float(x)


def _div(a, b):
    return None if b == 0 else Fraction(int(a), int(b))


def table_scores(table_t, K):
    """One threshold's (K + 1, 2) table -> dict of Fractions (None on a zero denominator), each from its definition."""
    m = [int(v) for v in table_t[:, 0]]
    a = [int(v) for v in table_t[:, 1]]
    ni = [x + y for x, y in zip(m, a)]
    n, N1 = sum(ni), sum(a)
    N0 = n - N1
    r = dict(n_valid=n, n_events=N1)
    p = [Fraction(i, K) for i in range(K + 1)]
    ob = _div(N1, n)
    oi = [_div(a[i], ni[i]) for i in range(K + 1)]
    r['base_rate'] = ob
    r['observed_frequency'] = oi
    r['forecast_count'] = ni
    if n:
        r['brier'] = sum(m[i] * p[i] ** 2 + a[i] * (1 - p[i]) ** 2 for i in range(K + 1)) / n
        r['reliability'] = sum(ni[i] * (p[i] - oi[i]) ** 2 for i in range(K + 1) if ni[i]) / n
        r['resolution'] = sum(ni[i] * (oi[i] - ob) ** 2 for i in range(K + 1) if ni[i]) / n
        r['uncertainty'] = ob * (1 - ob)
        r['brier_fair'] = None if K == 1 else \
            r['brier'] - Fraction(sum(ni[i] * i * (K - i) for i in range(K + 1)), K * K * (K - 1) * n)
        r['bss'] = None if r['uncertainty'] == 0 else 1 - r['brier'] / r['uncertainty']
    else:
        for k in ('brier', 'reliability', 'resolution', 'uncertainty', 'brier_fair', 'bss'):
            r[k] = None
    # ROC: point j warns iff c >= K + 1 - j
    pod, pofd = [], []
    for j in range(K + 2):
        pod.append(_div(sum(a[K + 1 - j:]), N1))
        pofd.append(_div(sum(m[K + 1 - j:]), N0))
    r['roc_pod'], r['roc_pofd'] = pod, pofd
    if N1 and N0:
        r['roc_auc'] = sum(a[i] * (sum(m[:i]) + Fraction(m[i], 2)) for i in range(K + 1)) / (N1 * N0)
    else:
        r['roc_auc'] = None
    return r


SCALARS = ('base_rate', 'brier', 'brier_fair', 'reliability', 'resolution', 'uncertainty', 'bss', 'roc_auc')


def from_counts_ref(table, cell, sample, K, thr):
    """The result dict of the product's ``exceedance_from_counts`` restated: Fractions rounded once, NaN on a zero denominator."""
    table, cell, sample = (np.asarray(x, np.int64) for x in (table, cell, sample))
    T = table.shape[0]
    per_t = [table_scores(table[t], K) for t in range(T)]
    res = dict(thresholds=np.asarray(thr, np.float32), n_members=K, table=table)
    res['n_valid'] = np.array([r['n_valid'] for r in per_t], np.int64)
    res['n_events'] = np.array([r['n_events'] for r in per_t], np.int64)
    for k in SCALARS:
        res[k] = np.array([_f(r[k]) for r in per_t], np.float64)
    res['forecast_probability'] = np.array([float(Fraction(i, K)) for i in range(K + 1)])
    res['observed_frequency'] = np.array([[_f(x) for x in r['observed_frequency']] for r in per_t], np.float64)
    res['forecast_count'] = np.array([r['forecast_count'] for r in per_t], np.int64)
    res['roc_pod'] = np.array([[_f(x) for x in r['roc_pod']] for r in per_t], np.float64)
    res['roc_pofd'] = np.array([[_f(x) for x in r['roc_pofd']] for r in per_t], np.float64)

    def each(fn, *arrays):                                  # Python integers in, one correctly rounded quotient out
        out = np.full(arrays[0].shape, NAN)
        for idx in np.ndindex(arrays[0].shape):
            num, den = fn(*(int(x[idx]) for x in arrays))
            if den != 0:
                out[idx] = num / den
        return out

    res.update(sample_sums=sample, n_valid_per_sample=sample[..., 0].copy(),
               brier_per_sample=each(lambda nv, q: (q, K * K * nv), sample[..., 0], sample[..., 3]))
    nv, so, sc, sq = (cell[:, i] for i in range(4))
    res.update(cell_sums=cell, n_valid_map=nv.copy(), brier_map=each(lambda n, q: (q, K * K * n), nv, sq),
               base_rate_map=each(lambda n, s: (s, n), nv, so), forecast_rate_map=each(lambda n, c: (c, K * n), nv, sc),
               bss_map=each(lambda n, s, q: (K * K * s * (n - s) - q * n, K * K * s * (n - s)), nv, so, sq))
    return res


def scores_ref(members, obs, thr, fields=True):
    """What metrics.exceedance_scores(obs, members, thr, return_fields=fields) returns, restated."""
    cr = counts_ref(members, obs, thr)
    res = from_counts_ref(cr['table'], cr['cell'], cr['sample'], cr['K'], thr)
    if fields:
        res['count_field'] = cr['count']
        res['probability_field'] = np.where(cr['valid'], cr['c'].astype(np.float32) / np.float32(cr['K']), np.float32(np.nan))
    return res


INT_KEYS = ('table', 'n_valid', 'n_events', 'forecast_count', 'sample_sums', 'n_valid_per_sample', 'cell_sums', 'n_valid_map')
FLOAT_KEYS = SCALARS + ('forecast_probability', 'observed_frequency', 'roc_pod', 'roc_pofd', 'brier_per_sample', 'brier_map',
                        'base_rate_map', 'forecast_rate_map', 'bss_map')


def assert_same(got, ref, label='', fields=True, rtol=1e-15):
    """Integers equal, no element left out; derived floats within ``rtol`` relative, NaN in the same places."""
    assert set(ref) <= set(got), (label, set(ref) - set(got))
    assert got['n_members'] == ref['n_members']
    np.testing.assert_array_equal(got['thresholds'], ref['thresholds'], err_msg=f'{label}: thresholds')
    for k in INT_KEYS + (('count_field',) if fields else ()):
        g = np.asarray(got[k])
        assert g.dtype == (np.int16 if k == 'count_field' else np.int64), (label, k, g.dtype)
        np.testing.assert_array_equal(g, ref[k], err_msg=f'{label}: {k}')
    for k in FLOAT_KEYS + (('probability_field',) if fields else ()):
        g, r = np.asarray(got[k]), np.asarray(ref[k])
        assert g.shape == r.shape, (label, k, g.shape, r.shape)
        np.testing.assert_array_equal(np.isnan(g), np.isnan(r), err_msg=f'{label}: NaN positions of {k}')
        np.testing.assert_allclose(g, r, rtol=rtol, atol=0, equal_nan=True, err_msg=f'{label}: {k}')
