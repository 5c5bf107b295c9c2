"""numpy restatement of the multivariate ensemble verification (include/dl4ds_hip.h): the energy score and
the variogram score, each term computed exactly as defined -- fp64 terms for the energy score; float32 difference and power, then
the fp64 mean over the members in member order, for the variogram score -- and every sum taken with math.fsum, which is exactly
rounded.  Written independently of dl4ds_amd/ensemble_score.py.

Bound of a comparison (assert_same).  The integers (n_pairs, n_valid, lags) and every NaN position are EQUAL.  e per pair is
bit-reproducible and all summands are non-negative, so a device sum of m terms is within (m + 4) 2^-53 relative of the exactly
rounded sum: one rounding per addition, plus the term's own roundings and a possible FMA contraction.  m is the number of valid
elements of the sample (energy sums) or the number of valid pairs of (sample, lag) (variogram sums); the bound is computed from each
case's m.  Derived scores get that bound plus 2 ulp (2^-52 relative each) per square root or quotient.  The energy score is a
DIFFERENCE of two such non-negative parts A = (1/K) sum sqrt(D_k) and B = c sum sqrt(G_kj): its bound is the relative bound times
(A + B)."""
import math

import numpy as np

EPS = 2.0 ** -53
ULP = 2.0 ** -52


def lags_ref(max_lag):
    """(dy, dx) with 0 < dy^2 + dx^2 <= max_lag^2 in the half-plane dy > 0 or (dy == 0 and dx > 0), ordered by (dy, dx)"""
    out = [(dy, dx) for dy in range(0, max_lag + 1) for dx in range(-max_lag, max_lag + 1)
           if 0 < dy * dy + dx * dx <= max_lag * max_lag and (dy > 0 or dx > 0)]
    return sorted(out)


def power(d, order):
    """|d|^order on float32, one correctly rounded operation after the absolute value"""
    m = np.abs(d).astype(np.float32)
    if order == 0.5:
        return np.sqrt(m)
    if order == 1:
        return m
    assert order == 2
    return m * m


def valid_ref(members, y, weights=None):
    """-> bool array shaped like y: observation and all members finite, weight > 0"""
    v = np.isfinite(y) & np.isfinite(members).all(axis=0)
    if weights is not None:
        v &= np.broadcast_to(np.asarray(weights, np.float32), y.shape[1:]) > 0
    return v


def energy_sums_ref(members, y, weights=None):
    """-> dist (N, K (K + 1) / 2) float64: D_k, then G_kj row-major over k < j; n_valid (N,) int64"""
    K, N = members.shape[0], y.shape[0]
    v = valid_ref(members, y, weights)
    w_all = np.ones(y.shape[1:], np.float64) if weights is None else \
        np.broadcast_to(np.asarray(weights, np.float32), y.shape[1:]).astype(np.float64)
    dist = np.zeros((N, K * (K + 1) // 2), np.float64)
    nvalid = np.zeros(N, np.int64)
    for n in range(N):
        keep = v[n].reshape(-1)
        nvalid[n] = int(keep.sum())
        x = members[:, n].reshape(K, -1)[:, keep].astype(np.float64)
        yy = y[n].reshape(-1)[keep].astype(np.float64)
        w = w_all.reshape(-1)[keep]
        for k in range(K):
            d = x[k] - yy
            dist[n, k] = math.fsum((d * d * w).tolist())
        s = K
        for k in range(K):
            for j in range(k + 1, K):
                d = x[k] - x[j]
                dist[n, s] = math.fsum((d * d * w).tolist())
                s += 1
    return dist, nvalid


def variogram_sums_ref(members, y, max_lag, order, weights=None):
    """-> n_pairs (N, L) int64, sums (N, L, 3) float64: sum (o - e)^2, sum o, sum e over the valid pairs of each lag"""
    K, N = members.shape[0], y.shape[0]
    shape = y.shape[1:]
    H, W, C = shape[-3:]
    planes = int(np.prod(shape[:-3], dtype=np.int64))
    lags = lags_ref(max_lag)
    v = valid_ref(members, y, weights).reshape(N, planes, H, W, C)
    yf = np.asarray(y, np.float32).reshape(N, planes, H, W, C)
    mf = np.asarray(members, np.float32).reshape(K, N, planes, H, W, C)
    npairs = np.zeros((N, len(lags)), np.int64)
    sums = np.zeros((N, len(lags), 3), np.float64)
    with np.errstate(invalid='ignore', over='ignore'):
        for li, (dy, dx) in enumerate(lags):
            if dy >= H or abs(dx) >= W:
                continue
            ya, yb = slice(0, H - dy), slice(dy, H)
            xa, xb = (slice(0, W - dx), slice(dx, W)) if dx >= 0 else (slice(-dx, W), slice(0, W + dx))
            for n in range(N):
                ok = v[n][:, ya, xa] & v[n][:, yb, xb]
                o = power(yf[n][:, ya, xa] - yf[n][:, yb, xb], order)
                acc = np.zeros(o.shape, np.float64)
                for k in range(K):                                          # member order
                    acc = acc + power(mf[k, n][:, ya, xa] - mf[k, n][:, yb, xb], order).astype(np.float64)
                e = acc / K
                o64 = o.astype(np.float64)
                d = o64 - e
                npairs[n, li] = int(ok.sum())
                sums[n, li, 0] = math.fsum((d * d)[ok].tolist())
                sums[n, li, 1] = math.fsum(o64[ok].tolist())
                sums[n, li, 2] = math.fsum(e[ok].tolist())
    return npairs, sums


def scores_ref(members, y, max_lag=4, order=0.5, lag_weights='inverse', fair=False, weights=None, energy=None):
    """The dict of ``metrics.multivariate_scores`` from the definitions, plus '_parts' (N, 2): the two non-negative parts A, B of
    each sample's energy score (for the bound).  ``energy``: what ``energy_sums_ref`` returned for the same members, observation
    and weights (it does not depend on the other arguments; computed once per stack by the tests, and left unchanged)."""
    members, y = np.asarray(members, np.float32), np.asarray(y, np.float32)
    K, N = members.shape[0], y.shape[0]
    dist, nvalid = energy_sums_ref(members, y, weights) if energy is None else (energy[0].copy(), energy[1].copy())
    npairs, sums = variogram_sums_ref(members, y, max_lag, order, weights)
    lags = np.asarray(lags_ref(max_lag), np.int64).reshape(-1, 2)
    L = len(lags)
    c = 1.0 / (K * (K - 1)) if fair else 1.0 / (K * K)
    member, pair = np.sqrt(dist[:, :K]), np.sqrt(dist[:, K:])
    parts = np.zeros((N, 2))
    es = np.full(N, np.nan)
    for n in range(N):
        parts[n] = math.fsum(member[n].tolist()) / K, c * math.fsum(pair[n].tolist())
        if nvalid[n] > 0:
            es[n] = parts[n, 0] - parts[n, 1]
    scored = [float(es[n]) for n in range(N) if nvalid[n] > 0]
    distance = np.asarray([math.sqrt(dy * dy + dx * dx) for dy, dx in lags.tolist()])
    omega = 1.0 / distance if lag_weights == 'inverse' else np.ones(L)

    def quotient(s, m):
        den = math.fsum((omega * np.asarray(m, np.float64)).tolist())
        return math.fsum((omega * np.asarray(s, np.float64)).tolist()) / den if den > 0 else float('nan')

    tot_n = npairs.sum(axis=0)
    tot = np.asarray([[math.fsum(sums[:, l, q].tolist()) for q in range(3)] for l in range(L)], np.float64).reshape(L, 3)
    with np.errstate(invalid='ignore', divide='ignore'):
        per_lag = np.where(tot_n[:, None] > 0, tot / tot_n[:, None], np.nan)
    return dict(energy_score=math.fsum(scored) / len(scored) if scored else float('nan'), energy_score_per_sample=es,
                member_distance=member, pair_distance=pair,
                variogram_score=quotient(tot[:, 0], tot_n),
                variogram_score_per_sample=np.asarray([quotient(sums[n, :, 0], npairs[n]) for n in range(N)], np.float64).reshape(N),
                lags=lags, lag_distance=distance, lag_weight=omega,
                variogram_obs=per_lag[:, 1], variogram_ens=per_lag[:, 2], variogram_error=per_lag[:, 0],
                n_pairs=npairs, n_valid_per_sample=nvalid, n_members=K, order=float(order), fair=bool(fair),
                dist_sums=dist, variogram_sums=sums, _parts=parts)


def close(got, ref, rel, scale=None, what=''):
    """every element: NaN in the same places, |got - ref| <= rel * scale (scale: |ref| by default); returns the worst error / bound"""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    rel = np.broadcast_to(np.asarray(rel, np.float64), ref.shape)
    scale = np.abs(ref) if scale is None else np.broadcast_to(np.asarray(scale, np.float64), ref.shape)
    nan = np.isnan(ref)
    assert np.array_equal(np.isnan(got), nan), (what, 'NaN positions differ')
    err, bound = np.abs(got - ref)[~nan], (rel * scale)[~nan]
    bad = err > bound
    assert not bad.any(), (what, f'{int(bad.sum())} of {bad.size} outside the bound', float(err[bad].max()), float(bound[bad].min()))
    with np.errstate(invalid='ignore', divide='ignore'):
        r = np.where(bound > 0, err / bound, 0.0)
    return float(r.max()) if r.size else 0.0


def assert_same(got, ref, what=''):
    """``metrics.multivariate_scores``'s dict against ``scores_ref``'s: every key, no element left out; prints the worst error over
    its bound per group of keys before anything derived is asserted."""
    assert set(got) == set(ref) - {'_parts'}, (what, set(got) ^ (set(ref) - {'_parts'}))
    for k in ('n_pairs', 'n_valid_per_sample', 'lags'):
        assert np.asarray(got[k]).dtype == np.int64 and np.array_equal(got[k], ref[k]), (what, k)
    for k in ('n_members', 'order', 'fair'):
        assert got[k] == ref[k], (what, k)
    for k in ('lag_distance', 'lag_weight'):
        close(got[k], ref[k], 2 * ULP, what=(what, k))
    m_e = ref['n_valid_per_sample'].astype(np.float64)                      # terms of every energy sum of the sample
    m_v = ref['n_pairs'].astype(np.float64)                                 # terms of every variogram sum of (sample, lag)
    rel_e, rel_v = (m_e + 4) * EPS, (m_v + 4) * EPS
    worst = dict(dist=close(got['dist_sums'], ref['dist_sums'], rel_e[:, None], what=(what, 'dist_sums')),
                 vsums=close(got['variogram_sums'], ref['variogram_sums'], rel_v[:, :, None], what=(what, 'variogram_sums')))
    for k in ('member_distance', 'pair_distance'):
        worst[k] = close(got[k], ref[k], rel_e[:, None] + 2 * ULP, what=(what, k))
    parts = ref['_parts'].sum(axis=1)
    rel_es = rel_e + 6 * ULP                                               # the sum's bound, a square root, the fsum, quotient and product
    worst['es'] = close(got['energy_score_per_sample'], ref['energy_score_per_sample'], rel_es, parts, what=(what, 'es per sample'))
    scored = m_e > 0
    if scored.any():
        bound = math.fsum((rel_es * parts)[scored].tolist()) / int(scored.sum()) + 2 * ULP * float(parts[scored].mean())
        worst['es_mean'] = close(got['energy_score'], ref['energy_score'], bound, 1.0, what=(what, 'energy_score'))
    else:
        assert np.isnan(got['energy_score']) and np.isnan(ref['energy_score']), what
    rel_vs = rel_v.max(axis=1) + 6 * ULP if m_v.shape[1] else np.zeros(len(m_e))
    worst['vs'] = close(got['variogram_score_per_sample'], ref['variogram_score_per_sample'], rel_vs, what=(what, 'vs per sample'))
    top = (float(m_v.max()) + 4) * EPS + 8 * ULP if m_v.size else 0.0      # (each sample's sums within its own bound, then the fsum)
    worst['vs_mean'] = close(got['variogram_score'], ref['variogram_score'], top, what=(what, 'variogram_score'))
    for k in ('variogram_obs', 'variogram_ens', 'variogram_error'):
        worst[k] = close(got[k], ref[k], top, what=(what, k))
    print(f'{what}: worst error / bound ' + ', '.join(f'{k} {v:.3f}' for k, v in worst.items()))
    return worst
