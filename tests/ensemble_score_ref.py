"""fp64 numpy restatement of the ensemble verification scores (csrc/ensemble_score.hip, Model.score_ensemble,
metrics.ensemble_scores).  CRPS by the O(K^2) pairwise definition (NOT the sorted form the kernel evaluates), variance by
np.var(ddof=1), ranks by counting plus the tie hash restated in integer arithmetic, coverage through np.quantile(method='linear')
rounded to float32 as the device's quantile is.  Shared by tests/test_ensemble_score_api.py (CPU) and tests/test_gpu_ensemble_score.py;
imports nothing of the package under test."""
import warnings

import numpy as np

M64 = (1 << 64) - 1


def tie(seed, g, equal):
    """The tie draw of include/dl4ds_hip.h in Python integers: one of 0 ... equal, a pure function of (seed, g, equal)."""
    z = (seed + 0x9E3779B97F4A7C15 * (g + 1)) & M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    z = z ^ (z >> 31)
    return ((z >> 32) * (equal + 1)) >> 32


def tie_array(seed, g, equal):
    """``tie`` on arrays (uint64 arithmetic wraps mod 2^64)."""
    g = np.asarray(g, np.uint64)
    with np.errstate(over='ignore'):
        z = np.uint64(seed & M64) + np.uint64(0x9E3779B97F4A7C15) * (g + np.uint64(1))
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        z = z ^ (z >> np.uint64(31))
        return (((z >> np.uint64(32)) * (np.asarray(equal, np.uint64) + np.uint64(1))) >> np.uint64(32)).astype(np.int64)


def crps_pairwise(x, y, fair=False):
    """x (K, n) and y (n,) float64 -> (1/K) sum_k |x_k - y| - c sum_{i<j} |x_i - x_j|, c = 1/K^2 or (fair) 1/(K (K - 1))"""
    K = x.shape[0]
    first = np.abs(x - y).sum(axis=0) / K
    pair = np.zeros(x.shape[1:], np.float64)
    for i in range(K):
        if i + 1 < K:
            pair += np.abs(x[i + 1:] - x[i]).sum(axis=0)
    if K == 1:
        return first
    return first - pair / (K * (K - 1) if fair else K * K)


def score_ref(members, obs, quantiles=(), fair=False, seed=0, scale=None):
    """members (K, N, ...) float32, obs (N, ...) float32, ``scale`` None or broadcastable to one sample -> dict of per-element
    arrays shaped like obs: 'valid' (bool), 'crps', 'sqerr', 'var' (float64, NaN where invalid), 'rank' (int64, -1 where invalid),
    'below', 'equal' (int64), 'covered' (nq, ...) bool (False where invalid), 'Q' (nq, ...) the float32 quantile, 'interp' (nq, ...)
    bool: the quantile is genuinely interpolated there (non-integer position AND its two order statistics differ), 'dmax' / 'mmax':
    max_k |x_k - y| and max_k |x_k - mean| (the terms of the error bounds).  The element index of the tie hash is the flat index
    into obs."""
    m32 = np.asarray(members, np.float32)
    y32 = np.asarray(obs, np.float32)
    K = m32.shape[0]
    assert m32.shape[1:] == y32.shape, (m32.shape, y32.shape)
    q = np.asarray(quantiles, np.float32).astype(np.float64).reshape(-1)
    x = m32.reshape(K, -1).astype(np.float64)
    y = y32.reshape(-1).astype(np.float64)
    n = y.size
    valid = np.isfinite(y) & np.isfinite(x).all(axis=0)
    sc = np.ones(n)
    if scale is not None:
        s1 = np.broadcast_to(np.asarray(scale, np.float32), y32.shape[1:]).astype(np.float64)
        sc = np.broadcast_to(s1, y32.shape).reshape(-1).copy()
        with np.errstate(invalid='ignore'):
            valid &= np.isfinite(sc) & (sc > 0)
    xs, ys = np.where(valid, x, 0.0), np.where(valid, y, 0.0)
    with warnings.catch_warnings(), np.errstate(all='ignore'):
        warnings.simplefilter('ignore')
        crps = crps_pairwise(xs, ys, fair) * sc
        mean = xs.mean(axis=0)
        sqerr = (mean - ys) ** 2 * sc * sc
        var = (np.var(xs, axis=0, ddof=1) if K > 1 else np.zeros(n)) * sc * sc
        below = (xs < ys).sum(axis=0).astype(np.int64)
        equal = (xs == ys).sum(axis=0).astype(np.int64)
        rank = below + tie_array(seed, np.arange(n, dtype=np.uint64), equal)
        srt = np.sort(xs, axis=0)
        Q = np.empty((len(q), n), np.float32)
        interp = np.zeros((len(q), n), bool)
        for j, p in enumerate(q):
            Q[j] = np.quantile(xs, p, axis=0, method='linear').astype(np.float32)
            pos = (K - 1) * p
            if pos != np.floor(pos):
                lo = int(np.floor(pos))
                interp[j] = srt[lo] != srt[min(lo + 1, K - 1)]
        covered = (ys.astype(np.float32)[None] <= Q) & valid[None]
        dmax, mmax = np.abs(xs - ys).max(axis=0) * sc, np.abs(xs - mean).max(axis=0) * sc
    nan = lambda a: np.where(valid, a, np.nan).reshape(y32.shape)                         # noqa: E731
    shp = y32.shape
    return dict(valid=valid.reshape(shp), crps=nan(crps), sqerr=nan(sqerr), var=nan(var),
                rank=np.where(valid, rank, -1).reshape(shp), below=below.reshape(shp), equal=equal.reshape(shp),
                covered=covered.reshape((len(q),) + shp), Q=Q.reshape((len(q),) + shp), interp=interp.reshape((len(q),) + shp),
                dmax=dmax.reshape(shp), mmax=mmax.reshape(shp))


def ulp32(a):
    """one unit in the last place of float32 at |a| (a in float64, taken at its float32 rounding; at least the smallest subnormal)"""
    with np.errstate(all='ignore'):
        return np.spacing(np.abs(np.asarray(a, np.float64)).astype(np.float32)).astype(np.float64)


def folds(ref):
    """fp64 sums of the restatement's float32-rounded fields: per sample (N, 4) and per cell (4, ...) as crps, sqerr, var, count;
    the rank histogram needs K: ``np.bincount(rank[valid], minlength=K + 1)``."""
    v = ref['valid']
    f = [np.where(v, ref[k].astype(np.float32).astype(np.float64), 0.0) for k in ('crps', 'sqerr', 'var')] + [v.astype(np.float64)]
    N = v.shape[0]
    per_sample = np.stack([a.reshape(N, -1).sum(axis=1) for a in f], axis=1)
    per_cell = np.stack([a.sum(axis=0) for a in f])
    return per_sample, per_cell


def summary(ref, K):
    """The scalars and histograms of the result dict from the restatement (means in fp64 over the valid elements)."""
    v = ref['valid']
    n_valid = int(v.sum())
    return dict(n_valid=n_valid, crps=float(ref['crps'][v].mean()), rmse=float(np.sqrt(ref['sqerr'][v].mean())),
                spread=float(np.sqrt(ref['var'][v].mean())), rank_histogram=np.bincount(ref['rank'][v], minlength=K + 1),
                covered=ref['covered'].reshape(ref['covered'].shape[0], -1).sum(axis=1))
