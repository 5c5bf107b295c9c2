"""Numpy restatement of the distance-map verification (dl4ds_amd/csrc/distance.hip): event sets, the exact
squared Euclidean distance transform twice over (separable in int64, and a plain minimum over all event cells), the eight integers
and the seven fp64 sums per field and threshold.  Every fp64 sum comes as `math.fsum` of its term list, next to the number of terms
and the sum of their magnitudes, from which `bound` derives what any summation order may differ by."""
import math

import numpy as np

DIST_EMPTY = 2 ** 31 - 1
COUNTS = ('n_valid', 'n_A', 'n_B', 'n_AB', 'max_d2_AB', 'max_d2_BA', 'sum_d2_AB', 'sum_d2_BA')
SUMS = ('sum_d_AB', 'sum_d_BA', 'pratt_AB', 'pratt_BA', 'bad1', 'bad2', 'badmax')


def event_sets(y, p, thresholds):
    """y, p (N, H, W, C) -> valid (F, H, W), A and B (F, T, H, W), fields f = n*C + c, compared on float32"""
    y, p = np.asarray(y, np.float32), np.asarray(p, np.float32)
    N, H, W, C = y.shape
    fy, fp = (a.transpose(0, 3, 1, 2).reshape(N * C, H, W) for a in (y, p))
    valid = np.isfinite(fy) & np.isfinite(fp)
    thr = np.asarray(thresholds, np.float32).reshape(-1)
    with np.errstate(invalid='ignore'):
        A = valid[:, None] & (fy[:, None] >= thr[None, :, None, None])
        B = valid[:, None] & (fp[:, None] >= thr[None, :, None, None])
    return valid, A, B


def edt_separable(ev):
    """squared distance of every cell of the (H, W) boolean field to its nearest event: the vertical distance g to the nearest
    event of the cell's column, then min over k of (j - k)^2 + g(i, k)^2, all in int64; DIST_EMPTY without an event"""
    H, W = ev.shape
    big = 1 << 40
    i = np.arange(H, dtype=np.int64)[:, None]
    last = np.maximum.accumulate(np.where(ev, i, -big), axis=0)                      # nearest event at or above
    nxt = np.minimum.accumulate(np.where(ev, i, big)[::-1], axis=0)[::-1]            # nearest event at or below
    g = np.minimum(i - last, nxt - i)
    g2 = np.where(g >= big // 2, big, g * g)
    j = np.arange(W, dtype=np.int64)
    d = ((j[:, None] - j[None, :]) ** 2)[None] + g2[:, None, :]                     # [i][j][k]
    d = d.min(axis=2)
    return np.where(d >= big, DIST_EMPTY, d)


def edt_brute(ev):
    """the same by the definition: the minimum over all event cells"""
    H, W = ev.shape
    ei, ej = (a.astype(np.int64) for a in np.nonzero(ev))
    out = np.full((H, W), DIST_EMPTY, np.int64)
    if not len(ei):
        return out
    j = np.arange(W, dtype=np.int64)
    for i in range(H):
        out[i] = ((i - ei) ** 2 + (j[:, None] - ej[None, :]) ** 2).min(axis=1)
    return out


def _fsum(terms):
    """-> (math.fsum of the terms, their number, the sum of their magnitudes)"""
    t = [float(v) for v in np.asarray(terms, np.float64).reshape(-1)]
    if any(math.isnan(v) for v in t):
        return float('nan'), len(t), float('nan')
    return math.fsum(t), len(t), math.fsum(abs(v) for v in t)


def field_sums(valid, A, B, dA, dB, cutoff, alpha):
    """the integers and sums of one field at one threshold from its two squared maps (int64) -> (counts [8] as Python integers,
    sums [7], number of terms [7], sum of the terms' magnitudes [7])"""
    a2, b2 = dB[A], dA[B]                                                            # d2(a, B) over A, d2(b, A) over B
    counts = [int(valid.sum()), int(A.sum()), int(B.sum()), int((A & B).sum()), int(a2.max()) if a2.size else 0,
              int(b2.max()) if b2.size else 0, int(a2.sum()), int(b2.sum())]
    inf = lambda d2: np.where(d2 == DIST_EMPTY, np.inf, d2.astype(np.float64))       # noqa: E731
    dist = lambda d2: np.sqrt(inf(d2))                                               # noqa: E731
    with np.errstate(invalid='ignore'):
        w = np.abs(np.minimum(dist(dA[valid]), cutoff) - np.minimum(dist(dB[valid]), cutoff))
        lists = [dist(a2), dist(b2), 1.0 / (1.0 + alpha * inf(a2)), 1.0 / (1.0 + alpha * inf(b2)), w, w * w]
    sums, n, mag = zip(*(_fsum(t) for t in lists))
    top = float(np.max(w)) if w.size else 0.0                                        # (np.max hands a NaN on)
    return counts, list(sums) + [top], list(n) + [1], list(mag) + [0.0]


def distance(y, p, thresholds, cutoff, alpha, edt=edt_separable):
    """everything dl4ds_distance_scores returns -> dict: counts (F, T, 8) int64, sums (F, T, 7), d2_obs / d2_pred (F, T, H, W) int32,
    and per sum n_terms and magnitude (F, T, 7)"""
    valid, A, B = event_sets(y, p, thresholds)
    F, T, H, W = A.shape
    out = dict(counts=np.zeros((F, T, 8), np.int64), sums=np.zeros((F, T, 7)), n_terms=np.zeros((F, T, 7), np.int64),
               magnitude=np.zeros((F, T, 7)), d2_obs=np.zeros((F, T, H, W), np.int32), d2_pred=np.zeros((F, T, H, W), np.int32))
    for f in range(F):
        for t in range(T):
            dA, dB = edt(A[f, t]), edt(B[f, t])
            out['d2_obs'][f, t], out['d2_pred'][f, t] = dA, dB
            c, s, n, m = field_sums(valid[f], A[f, t], B[f, t], dA, dB, cutoff, alpha)
            out['counts'][f, t], out['sums'][f, t], out['n_terms'][f, t], out['magnitude'][f, t] = c, s, n, m
    return out


def bound(n_terms, magnitude):
    """what a sum of n exact terms taken in any order may differ from math.fsum by: gamma_(n-1) * sum |term|, gamma_k = k u / (1 -
    k u), u = 2^-53; 0 for at most one term"""
    k = np.maximum(np.asarray(n_terms, np.float64) - 1.0, 0.0)
    u = 2.0 ** -53
    with np.errstate(invalid='ignore'):
        return np.where(k == 0, 0.0, k * u / (1.0 - k * u) * np.asarray(magnitude, np.float64))


def same(got, ref, maps=True):
    """`got` against distance(): integers and maps equal, fp64 sums within `bound`, bit-equal where the bound is 0 (badmax, sums of
    at most one term); a sum that is not finite in the restatement must be the same infinity, or NaN, in `got`"""
    np.testing.assert_array_equal(np.asarray(got['counts']).reshape(ref['counts'].shape), ref['counts'])
    if maps:
        for k in ('d2_obs', 'd2_pred'):
            assert got[k].dtype == np.int32
            np.testing.assert_array_equal(got[k].reshape(ref[k].shape), ref[k], err_msg=k)
    g, w = np.asarray(got['sums'], np.float64).reshape(ref['sums'].shape), ref['sums']
    fin = np.isfinite(w)
    np.testing.assert_array_equal(g[~fin], w[~fin])                                  # (NaN equals NaN here, inf its own sign)
    lim = bound(ref['n_terms'], ref['magnitude'])
    err = np.abs(g[fin] - w[fin])
    assert (err <= lim[fin]).all(), (np.argwhere(fin & ~(np.abs(g - np.where(fin, w, 0)) <= lim)).tolist(), err.max())
    exact = fin & (lim == 0)
    assert g[exact].tobytes() == w[exact].tobytes()
