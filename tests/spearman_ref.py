"""numpy fp64 restatement of scipy.stats.spearmanr on 1-D inputs, row by row over a (S, L) array: Pearson correlation of the
average ranks (a tie run at sorted positions [a, b) gets rank (a + b + 1) / 2, -0.0 ties with +0.0), NaN for a row holding a
NaN, a constant row, or L < 2.  The GPU tests compare dl4ds_spearman with it; tests/test_metrics_api.py checks it against scipy."""
import numpy as np


def average_ranks(x):
    """(S, L) -> (S, L) fp64 average ranks (1-based) along each row."""
    x = np.asarray(x, np.float64)
    s, n = x.shape
    order = np.argsort(x, axis=1, kind='stable')
    xs = np.take_along_axis(x, order, 1)
    head = np.ones((s, n), bool)
    head[:, 1:] = xs[:, 1:] != xs[:, :-1]                 # -0.0 != +0.0 is False: one run
    j = np.arange(n)
    start = np.maximum.accumulate(np.where(head, j, 0), axis=1)
    last = np.ones((s, n), bool)
    last[:, :-1] = head[:, 1:]
    end = np.minimum.accumulate(np.where(last, j + 1, n)[:, ::-1], axis=1)[:, ::-1]
    r = np.empty((s, n))
    np.put_along_axis(r, order, (start + end + 1) / 2.0, 1)
    return r


def spearman_rows(a, b):
    """rho of every row pair of two (S, L) arrays, fp64 (S,)."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    s, n = a.shape
    out = np.full(s, np.nan)
    if n < 2:
        return out
    m = (n + 1) / 2.0
    da, db = average_ranks(a) - m, average_ranks(b) - m
    den = np.sqrt((da * da).sum(1) * (db * db).sum(1))
    ok = (den > 0) & ~np.isnan(a).any(1) & ~np.isnan(b).any(1)
    out[ok] = (da * db).sum(1)[ok] / den[ok]
    return out


def spearman_space(y, p):
    """per test pair of (N, H, W, C) arrays, over all H*W*C values"""
    n = y.shape[0]
    return spearman_rows(np.reshape(y, (n, -1)), np.reshape(p, (n, -1)))


def spearman_time(y, p):
    """per grid point of channel 0 of (N, H, W, C) arrays, over the N pairs -> (H, W)"""
    n, h, w = y.shape[:3]
    t = lambda x: np.reshape(np.asarray(x)[..., 0], (n, h * w)).T
    return spearman_rows(t(y), t(p)).reshape(h, w)
