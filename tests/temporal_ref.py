"""numpy restatement of dl4ds_temporal and dl4ds_trend (include/dl4ds_hip.h).  `temporal` walks the samples
of a period one by one, in order, and is vectorised over the cells only: every fp64 addition happens in the order the definition
gives, so the device is compared with it bit for bit.  `trend` loops over the pairs of periods and is vectorised over the cells.
tests/test_temporal_api.py checks both against independent statements (itertools.groupby, a plain Python float loop, a
brute-force double loop with np.median, scipy.stats.theilslopes) and hand-worked sequences."""
import numpy as np

OPS = (np.greater_equal, np.greater, np.less, np.less_equal)       # op 0..3
RAW_NAMES = ('n_valid', 'sum', 'sum_sq', 'n_pairs', 'lag_sums', 'transitions', 'spell_hist')


def canonical(row):
    """float32 with -0.0 as +0.0"""
    row = np.asarray(row, np.float32)
    return np.where(row == 0, np.float32(0), row)


def temporal(y, p, starts, lags=(), thr=(), op=0, bins=16):
    """y, p (N, per) float32 (p may be None); starts (P + 1,); lags (L,); thr (T,) or (T, per) -> valid int32 (P, per), moment
    float64 (P, S, 2, per), pair int32 (P, L, per), lag float64 (P, S, L, 3, per), trans int32 (P, S, T, 4, per), spell int32
    (P, S, T, 2, bins, per)"""
    xs = [np.asarray(a, np.float32) for a in ((y,) if p is None else (y, p))]
    S, (N, per) = len(xs), xs[0].shape
    lags = [int(v) for v in lags]
    L = len(lags)
    thr = np.asarray(thr, np.float32)
    T = thr.shape[0]
    thr = np.broadcast_to(thr.reshape(T, -1), (T, per)) if T else np.zeros((0, per), np.float32)
    thr_ok = np.isfinite(thr)
    P = len(starts) - 1
    cells = np.arange(per)
    valid, moment = np.zeros((P, per), np.int32), np.zeros((P, S, 2, per), np.float64)
    pair, lag = np.zeros((P, L, per), np.int32), np.zeros((P, S, L, 3, per), np.float64)
    trans, spell = np.zeros((P, S, T, 4, per), np.int32), np.zeros((P, S, T, 2, bins, per), np.int32)

    def ended(hist, run, mask):
        """the runs `run` (> 0 events, < 0 non-events) of the cells `mask` have ended: one more in their bin"""
        for kind, m in ((0, mask & (run > 0)), (1, mask & (run < 0))):
            k = np.minimum(np.abs(run[m]), bins) - 1
            np.add.at(hist[kind], (k, cells[m]), 1)

    with np.errstate(invalid='ignore', over='ignore'):
        for q in range(P):
            s0, s1 = int(starts[q]), int(starts[q + 1])
            ok = np.ones((s1 - s0, per), bool)
            for x in xs:
                ok &= np.isfinite(x[s0:s1])
            vs = [canonical(x[s0:s1]).astype(np.float64) for x in xs]
            run = np.zeros((S, T, per), np.int64)
            for i in range(s1 - s0):
                valid[q] += ok[i]
                for li, k in enumerate(lags):
                    if i - k < 0:
                        continue
                    both = ok[i] & ok[i - k]
                    pair[q, li] += both
                    for s in range(S):
                        a, b = vs[s][i - k], vs[s][i]
                        lag[q, s, li, 0] = np.where(both, lag[q, s, li, 0] + a, lag[q, s, li, 0])
                        lag[q, s, li, 1] = np.where(both, lag[q, s, li, 1] + b, lag[q, s, li, 1])
                        lag[q, s, li, 2] = np.where(both, lag[q, s, li, 2] + a * b, lag[q, s, li, 2])
                for s in range(S):
                    d = vs[s][i]
                    moment[q, s, 0] = np.where(ok[i], moment[q, s, 0] + d, moment[q, s, 0])
                    moment[q, s, 1] = np.where(ok[i], moment[q, s, 1] + d * d, moment[q, s, 1])
                    v32 = d.astype(np.float32)
                    for t in range(T):
                        ev = ok[i] & OPS[op](v32, thr[t])
                        cur = np.where(ev, 1, np.where(ok[i], -1, 0))
                        r = run[s, t]
                        trans[q, s, t, 0] += (r < 0) & (cur < 0)
                        trans[q, s, t, 1] += (r < 0) & (cur > 0)
                        trans[q, s, t, 2] += (r > 0) & (cur < 0)
                        trans[q, s, t, 3] += (r > 0) & (cur > 0)
                        same = ((r > 0) & (cur > 0)) | ((r < 0) & (cur < 0))
                        ended(spell[q, s, t], r, (r != 0) & ~same)
                        run[s, t] = np.where(same, r + cur, cur)
            for s in range(S):
                for t in range(T):
                    ended(spell[q, s, t], run[s, t], run[s, t] != 0)          # the period's end cuts the run
    for t in range(T):
        trans[:, :, t][..., ~thr_ok[t]] = -1
        spell[:, :, t][..., ~thr_ok[t]] = -1
    return valid, moment, pair, lag, trans, spell


def named(flat, s, grid):
    """series `s` of `temporal`'s outputs under the raw names of dl4ds_amd.temporal.temporal_statistics, cells as `grid`"""
    valid, moment, pair, lag, trans, spell = flat

    def g(a):
        return np.ascontiguousarray(a).reshape(a.shape[:-1] + tuple(grid))
    return dict(zip(RAW_NAMES, (g(valid), g(moment[:, s, 0]), g(moment[:, s, 1]), g(pair), g(lag[:, s]), g(trans[:, s]), g(spell[:, s]))))


def trend(v):
    """v (P, per) float64 -> valid int32 (per,), mk int64 (2, per) (S, the tie term), sen float64 (per,)"""
    v = np.asarray(v, np.float64)
    P, per = v.shape
    ok = np.isfinite(v)
    n = ok.sum(axis=0).astype(np.int32)
    s, ties = np.zeros(per, np.int64), np.zeros(per, np.int64)
    slopes = np.full((max(P * (P - 1) // 2, 1), per), np.nan)
    k = 0
    with np.errstate(invalid='ignore', over='ignore'):
        for i in range(P):
            same = np.zeros(per, np.int64)
            for j in range(P):
                both = ok[i] & ok[j]
                same += both & (v[j] == v[i])
                if j > i:
                    s += np.where(both, (v[j] > v[i]).astype(np.int64) - (v[j] < v[i]), 0)
                    q = (v[j] - v[i]) / np.float64(j - i)
                    slopes[k] = np.where(both, np.where(q == 0, 0.0, q), np.nan)
                    k += 1
            ties += np.where(ok[i], (same - 1) * (2 * same + 5), 0)
        slopes.sort(axis=0)                                         # NaN (a pair with an invalid end) sorts last
        M = n.astype(np.int64) * (n - 1) // 2
        lo, hi = np.maximum((M - 1) // 2, 0), np.maximum(M // 2, 0)
        cells = np.arange(per)
        mid = np.where(M % 2 == 1, slopes[lo, cells], (slopes[lo, cells] + slopes[hi, cells]) * 0.5)
        sen = np.where(M > 0, np.where(mid == 0, 0.0, mid), np.nan)
    return n, np.stack([s, ties]), sen
