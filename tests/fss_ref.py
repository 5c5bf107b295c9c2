"""numpy restatement of the neighbourhood verification of dl4ds_amd.metrics.neighbourhood_scores: the
Fractions Skill Score of Roberts & Lean (2008) and the 2 x 2 contingency scores, from integral images in int64 and Python integers
for the pooled sums.  Imports nothing from the product.

Definitions.  y (observation) and p (prediction) are (N, H, W, C), read as float32; each of the N*C planes is a field.  Thresholds
are cast to float32.  A cell is valid when y and p are finite there and the mask (2-D or with a channel axis, 0 = excluded) keeps
it.  bo = valid & (y >= t), bf = valid & (p >= t).  The window of size n >= 1 at (i, j) is rows [i - n//2, i - n//2 + n), columns
likewise, clipped to the field.  co, cf = window counts.  D = sum (cf - co)^2, F = sum cf^2, O = sum co^2 over all cells;
FSS = 1 - D / (F + O), NaN when F + O = 0; pooled: 1 - sum D / sum (F + O)."""
import numpy as np


def window_counts(b, n):
    """int64 (H, W): the number of set cells of the 2-D boolean / 0-1 array ``b`` in the window of size ``n`` around every cell."""
    b = np.asarray(b).astype(np.int64)
    h, w = b.shape
    sat = np.zeros((h + 1, w + 1), np.int64)
    sat[1:, 1:] = b.cumsum(0).cumsum(1)
    n = int(n)
    r0 = np.clip(np.arange(h) - n // 2, 0, h)
    r1 = np.clip(np.arange(h) - n // 2 + n, 0, h)
    c0 = np.clip(np.arange(w) - n // 2, 0, w)
    c1 = np.clip(np.arange(w) - n // 2 + n, 0, w)
    return sat[r1][:, c1] - sat[r0][:, c1] - sat[r1][:, c0] + sat[r0][:, c0]


def prepare(y, p, mask=None):
    """-> (y, p, valid): float32 (N, H, W, C) arrays and the boolean validity of every cell."""
    y, p = np.asarray(y, np.float32), np.asarray(p, np.float32)
    assert y.shape == p.shape and y.ndim == 4
    valid = np.isfinite(y) & np.isfinite(p)
    if mask is not None:
        mask = np.asarray(mask)
        if mask.ndim == 2:
            mask = mask[..., None]
        valid = valid & np.broadcast_to(mask != 0, y.shape)
    return y, p, valid


def field_sums(bo, bf, n):
    """(D, F, O) as Python integers for one field's indicator arrays and one window size."""
    co, cf = window_counts(bo, n), window_counts(bf, n)
    h, w = co.shape
    m = min(n, h) * min(n, w)
    assert h * w * m * m < 2 ** 62                                      # the int64 sums below are exact
    d = cf - co
    return int((d * d).sum()), int((cf * cf).sum()), int((co * co).sum())


def _div(num, den):
    return float('nan') if den == 0 else num / den


def contingency_scores(hits, misses, fa, nvalid):
    """POD, FAR, CSI, ETS, frequency bias from Python integers; NaN on a zero denominator."""
    obs, fc = hits + misses, hits + fa
    hr = _div(obs * fc, nvalid)
    ets = float('nan')
    if nvalid != 0 and (hits + misses + fa) - hr != 0:
        ets = (hits - hr) / ((hits + misses + fa) - hr)
    return dict(pod=_div(hits, obs), far=_div(fa, fc), csi=_div(hits, hits + misses + fa), ets=ets, bias=_div(fc, obs))


def neighbourhood_scores(y, p, thresholds, windows, mask=None):
    """The dict dl4ds_amd.metrics.neighbourhood_scores returns, computed field by field."""
    y, p, valid = prepare(y, p, mask)
    thr = np.asarray(thresholds, np.float32).reshape(-1)
    win = [int(v) for v in np.asarray(windows).reshape(-1)]
    N, H, W, C = y.shape
    T, S = len(thr), len(win)
    sums = np.zeros((N, C, T, S, 3), np.int64)
    cont = np.zeros((N, C, T, 4), np.int64)
    nvalid = valid.sum(axis=(1, 2)).astype(np.int64)                    # (N, C)
    names = ('pod', 'far', 'csi', 'ets', 'bias')
    per_field = {k: np.full((N, C, T), np.nan) for k in names}
    for i in range(N):
        for c in range(C):
            v = valid[i, :, :, c]
            for k, t in enumerate(thr):
                bo, bf = v & (y[i, :, :, c] >= t), v & (p[i, :, :, c] >= t)
                cont[i, c, k] = [(bo & bf).sum(), (bo & ~bf).sum(), (bf & ~bo).sum(), (v & ~bo & ~bf).sum()]
                for name, val in contingency_scores(*(int(x) for x in cont[i, c, k, :3]), int(nvalid[i, c])).items():
                    per_field[name][i, c, k] = val
                for s, n in enumerate(win):
                    sums[i, c, k, s] = field_sums(bo, bf, n)
    fss = np.full((N, C, T, S), np.nan)
    pooled = np.full((T, S), np.nan)
    pooled_c = np.full((C, T, S), np.nan)
    for k in range(T):
        for s in range(S):
            for i in range(N):
                for c in range(C):
                    d, f, o = (int(x) for x in sums[i, c, k, s])
                    fss[i, c, k, s] = 1.0 - _div(d, f + o)
            for c in range(C):
                d = sum(int(x) for x in sums[:, c, k, s, 0])
                fo = sum(int(x) for x in sums[:, c, k, s, 1]) + sum(int(x) for x in sums[:, c, k, s, 2])
                pooled_c[c, k, s] = 1.0 - _div(d, fo)
            d = sum(int(x) for x in sums[:, :, k, s, 0].ravel())
            fo = sum(int(x) for x in sums[:, :, k, s, 1].ravel()) + sum(int(x) for x in sums[:, :, k, s, 2].ravel())
            pooled[k, s] = 1.0 - _div(d, fo)
    res = dict(sums=sums, fss=fss, fss_pooled=pooled, fss_pooled_per_channel=pooled_c, hits=cont[..., 0], misses=cont[..., 1],
               false_alarms=cont[..., 2], correct_negatives=cont[..., 3], n_valid=nvalid, thresholds=thr,
               windows=np.asarray(win, np.int64), **per_field)
    nv = sum(int(x) for x in nvalid.ravel())
    pooled_scores = {k: np.full((T,), np.nan) for k in names}
    base = np.full((T,), np.nan)
    for k in range(T):
        h, m, f = (sum(int(x) for x in cont[:, :, k, q].ravel()) for q in range(3))
        for name, val in contingency_scores(h, m, f, nv).items():
            pooled_scores[name][k] = val
        base[k] = _div(h + m, nv)
    res.update({k + '_pooled': v for k, v in pooled_scores.items()})
    useful = 0.5 + base / 2.0
    uw = np.full((T,), -1, np.int64)
    for k in range(T):
        for s in range(S):
            if pooled[k, s] >= useful[k]:
                uw[k] = win[s]
                break
    res.update(base_rate=base, fss_random=base.copy(), fss_useful=useful, useful_window=uw)
    return res
