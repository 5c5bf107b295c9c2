"""numpy restatement of the distribution verification of dl4ds_amd.metrics.distribution_scores: per segment
the sample quantiles of observation and prediction, their 1-Wasserstein distance, the two-sample Kolmogorov-Smirnov statistic
times n, both histograms and the Perkins skill score, from np.sort and np.searchsorted.  Imports nothing from the product.

Definitions.  y (observation) and p (prediction) are (N, H, W, C), read as float32.  over='time': one segment per grid cell and
channel over the N samples, results shaped (H, W, C) + ...; over='space': one segment per sample, results shaped (N,) + ....  An
element is valid when y and p are finite there and the mask (2-D or with a channel axis, 0 = excluded) keeps it; invalid elements
leave both sides.  With a, b the ascending valid values (n each, as float64; -0.0 is +0.0):
  quantile q   h = q*(n-1), j = floor(h), x[j] + (x[min(j+1, n-1)] - x[j]) * (h - j); NaN when n = 0
  W1           sum |a[i] - b[i]| / n; NaN when n = 0
  KS * n       max over every value v of either side of |#{a <= v} - #{b <= v}|; 0 when n = 0
  histogram    bins [e_b, e_b+1) of float32 edges, the last one closed on the right; values outside are counted nowhere"""
import numpy as np


def segment_scores(y, p, q, edges=None):
    """-> (quant (2, Q), w1, ks_count, hist (2, B) or None, n, qmag (2, Q)) of two 1-D float32 samples; qmag = max(|x_j|, |x_j+1|)
    of the two order statistics a quantile is interpolated between (the scale of its rounding error)"""
    y, p = np.asarray(y, np.float32).ravel(), np.asarray(p, np.float32).ravel()
    ok = np.isfinite(y) & np.isfinite(p)
    a, b = np.sort(y[ok].astype(np.float64)) + 0.0, np.sort(p[ok].astype(np.float64)) + 0.0
    n = int(ok.sum())
    q = np.asarray(q, np.float64)
    quant, qmag = np.full((2, len(q)), np.nan), np.zeros((2, len(q)))
    hist = None
    if edges is not None:
        edges = np.asarray(edges, np.float32).astype(np.float64)
        hist = np.zeros((2, len(edges) - 1), np.int64)
    if n == 0:
        return quant, np.nan, 0, hist, 0, qmag
    h = q * (n - 1)
    j = np.floor(h).astype(np.int64)
    g = h - j
    for side, x in enumerate((a, b)):
        quant[side] = x[j] + (x[np.minimum(j + 1, n - 1)] - x[j]) * g
        qmag[side] = np.maximum(np.abs(x[j]), np.abs(x[np.minimum(j + 1, n - 1)]))
        if edges is not None:
            c = np.searchsorted(x, edges, 'left')
            c[-1] = np.searchsorted(x, edges[-1], 'right')
            hist[side] = np.diff(c)
    v = np.concatenate([a, b])
    ks = int(np.abs(np.searchsorted(a, v, 'right') - np.searchsorted(b, v, 'right')).max())
    return quant, float(np.abs(a - b).sum() / n), ks, hist, n, qmag


def prepare(y, p, mask=None):
    """-> (y, p): float32 (N, H, W, C) arrays, y with NaN where the mask excludes"""
    y, p = np.array(y, np.float32), np.asarray(p, np.float32)
    assert y.shape == p.shape and y.ndim == 4
    if mask is not None:
        mask = np.asarray(mask)
        if mask.ndim == 2:
            mask = mask[..., None]
        y[np.broadcast_to(mask == 0, y.shape)] = np.nan
    return y, p


def _div(num, den):
    return float('nan') if den == 0 else num / den


def distribution_scores(y, p, quantiles, bins=None, over='time', mask=None, return_bounds=False):
    """The dict dl4ds_amd.metrics.distribution_scores returns, computed segment by segment.  ``return_bounds``: also
    (bound_obs, bound_pred) shaped like q_obs = 2^-50 * max(|x_j|, |x_j+1|): three roundings of at most 2^-52 of that magnitude on
    either side of a comparison of two evaluations of the quantile formula."""
    y, p = prepare(y, p, mask)
    q = np.asarray(quantiles, np.float64).reshape(-1)
    edges = None if bins is None else np.asarray(bins, np.float32)
    N, H, W, C = y.shape
    if over == 'time':
        lead = (H, W, C)
        ys, ps = y.reshape(N, -1).T, p.reshape(N, -1).T
    else:
        assert over == 'space'
        lead = (N,)
        ys, ps = y.reshape(N, -1), p.reshape(N, -1)
    S, Q = len(ys), len(q)
    quant, w1, qmag = np.empty((S, 2, Q)), np.empty(S), np.empty((S, 2, Q))
    ks, nv = np.empty(S, np.int64), np.empty(S, np.int64)
    hist = None if edges is None else np.empty((S, 2, len(edges) - 1), np.int64)
    for s in range(S):
        r = segment_scores(ys[s], ps[s], q, edges)
        quant[s], w1[s], ks[s], nv[s], qmag[s] = r[0], r[1], r[2], r[4], r[5]
        if hist is not None:
            hist[s] = r[3]
    with np.errstate(invalid='ignore', divide='ignore'):
        ratio = lambda num: np.where(nv == 0, np.nan, num.astype(np.float64) / np.where(nv == 0, 1, nv).astype(np.float64))
        res = dict(n_valid=nv.reshape(lead), q_obs=quant[:, 0].reshape(lead + (Q,)), q_pred=quant[:, 1].reshape(lead + (Q,)),
                   q_bias=(quant[:, 1] - quant[:, 0]).reshape(lead + (Q,)), wasserstein=w1.reshape(lead),
                   ks_count=ks.reshape(lead), ks=ratio(ks).reshape(lead), quantiles=q, bins=None)
        if hist is not None:
            B = hist.shape[-1]
            po = [sum(int(v) for v in hist[:, 0, b]) for b in range(B)]
            pp = [sum(int(v) for v in hist[:, 1, b]) for b in range(B)]
            total = sum(int(v) for v in nv)
            res.update(hist_obs=hist[:, 0].reshape(lead + (B,)), hist_pred=hist[:, 1].reshape(lead + (B,)),
                       perkins=ratio(np.minimum(hist[:, 0], hist[:, 1]).sum(-1)).reshape(lead),
                       hist_obs_pooled=np.asarray(po, np.int64), hist_pred_pooled=np.asarray(pp, np.int64),
                       perkins_pooled=np.float64(_div(sum(min(a, b) for a, b in zip(po, pp)), total)), bins=edges)
    if return_bounds:
        return res, tuple((qmag[:, k] * 2.0 ** -50).reshape(lead + (Q,)) for k in range(2))
    return res
