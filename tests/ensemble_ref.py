"""fp64 numpy restatement of the ensemble statistics (csrc/ensemble.hip, Model.predict_ensemble): np.mean / np.std / np.min / np.max /
np.quantile(method='linear') along axis 0 of ``members.astype(float64)``, each rounded to float32.  Warnings are silenced: NaN and
infinite members give whatever numpy gives.  Shared by tests/test_ensemble_api.py (CPU) and tests/test_gpu_ensemble.py; imports
nothing of the package under test."""
import warnings

import numpy as np


def ensemble_ref(members, quantiles=()):
    """members (K, ...) float32 -> dict(mean, std, min, max: (...), quantiles: (len(quantiles), ...)), all float32.  ``quantiles`` are
    taken as given (pass the float32-rounded probabilities to restate a device call)."""
    m = np.asarray(members).astype(np.float64)
    q = np.asarray(quantiles, np.float64).reshape(-1)
    with warnings.catch_warnings(), np.errstate(all='ignore'):
        warnings.simplefilter('ignore')
        out = dict(mean=np.mean(m, axis=0), std=np.std(m, axis=0), min=np.min(m, axis=0), max=np.max(m, axis=0))
        out['quantiles'] = np.quantile(m, q, axis=0, method='linear') if q.size else np.empty((0,) + m.shape[1:])
        return {k: np.asarray(v).astype(np.float32) for k, v in out.items()}


def integer_position(K, q):
    """True where (K - 1) q is an integer: the quantile is an order statistic and has to be reproduced exactly."""
    pos = (K - 1) * np.asarray(q, np.float64)
    return pos == np.floor(pos)


def ulp_diff(a, b):
    """distance in units in the last place of float32 (NaN against NaN and equal values, infinities included, count 0; NaN against
    a number inf)"""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    assert a.shape == b.shape, (a.shape, b.shape)
    with np.errstate(all='ignore'):
        ulp = np.spacing(np.maximum(np.abs(a), np.abs(b))).astype(np.float64)
        d = np.abs(a.astype(np.float64) - b.astype(np.float64)) / ulp
    d = np.where(a == b, 0.0, d)
    d = np.where(np.isnan(a) & np.isnan(b), 0.0, d)
    d = np.where(np.isnan(a) != np.isnan(b), np.inf, d)
    return np.where(np.isnan(d), np.inf, d)


def check_stats(got, members, q32, label=''):
    """The bounds of the ensemble tests: min, max and quantiles at integer positions equal; mean, std and interpolated quantiles
    within 1 ulp of float32 (fp64 evaluation leaves an error of order K 2^-53, what remains is the final rounding plus a possible
    double rounding).  NaN positions must coincide.  Prints the worst distance per statistic."""
    K = members.shape[0]
    ref = ensemble_ref(members, np.asarray(q32, np.float32).astype(np.float64))
    worst = {}
    for k in ('mean', 'std', 'min', 'max'):
        assert got[k].dtype == np.float32 and got[k].shape == ref[k].shape, (k, got[k].dtype, got[k].shape, ref[k].shape)
        np.testing.assert_array_equal(np.isnan(got[k]), np.isnan(ref[k]), err_msg=f'{label} {k}: NaN positions')
        worst[k] = float(ulp_diff(got[k], ref[k]).max(initial=0.0))
    assert got['quantiles'].dtype == np.float32 and got['quantiles'].shape == ref['quantiles'].shape, \
        (got['quantiles'].shape, ref['quantiles'].shape)
    exact = integer_position(K, np.asarray(q32, np.float32).astype(np.float64))
    for j in range(len(exact)):
        g, r = got['quantiles'][j], ref['quantiles'][j]
        np.testing.assert_array_equal(np.isnan(g), np.isnan(r), err_msg=f'{label} quantile {j}: NaN positions')
        key = 'q_exact' if exact[j] else 'q_interp'
        worst[key] = max(worst.get(key, 0.0), float(ulp_diff(g, r).max(initial=0.0)))
    print(f'{label}: worst ulp ' + ', '.join(f'{k} {v:.2f}' for k, v in worst.items()))
    assert worst['min'] == 0 and worst['max'] == 0 and worst.get('q_exact', 0.0) == 0, (label, worst)
    assert worst['mean'] <= 1 and worst['std'] <= 1 and worst.get('q_interp', 0.0) <= 1, (label, worst)
    return worst
