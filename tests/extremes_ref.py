"""numpy / Python restatement of dl4ds_lmoments and dl4ds_pot_peaks (include/dl4ds_hip.h).

`pwm_cell` and `clusters_cell` are the definitions in plain Python, one cell at a time: np.sort, Python floats added one by one, an
explicit state machine.  `pwm` is the same arithmetic vectorised over the cells (one numpy fp64 operation per Python operation, in
the same order), which the device is compared with bit for bit; tests/test_extremes_api.py holds the two to the same bits and
checks them against scipy and hand-written series."""
import numpy as np


def canonical(row):
    """float32 with -0.0 as +0.0"""
    row = np.asarray(row, np.float32)
    return np.where(row == 0, np.float32(0), row)


def sorted_valid(col, sign=1):
    """the finite values of sign * col, ascending, float32, -0.0 as +0.0"""
    v = canonical(np.float32(sign) * np.asarray(col, np.float32))
    return np.sort(v[np.isfinite(v)])


def pwm_cell(col, sign=1):
    """one cell: (n, [b_0..b_3]) by the definition, in Python floats"""
    xs = [float(v) for v in sorted_valid(col, sign)]
    n = len(xs)
    out = []
    for r in range(4):
        if n <= r:
            out.append(float('nan'))
            continue
        s = None
        for j in range(r, n):
            w = 1.0
            for q in range(1, r + 1):
                w = w * (float(j - q + 1) / float(n - q))
            term = w * xs[j]
            s = term if s is None else s + term
        out.append(s / float(n))
    return n, out


def pwm(x, sign=1):
    """x (N, per) float32 -> valid int32 (per,), pwm float64 (4, per): `pwm_cell` of every column, vectorised over the columns"""
    x = np.asarray(x, np.float32)
    N, per = x.shape
    v = canonical(np.float32(sign) * x)
    ok = np.isfinite(v)
    n = ok.sum(axis=0).astype(np.int64)
    xs = np.sort(np.where(ok, v, np.float32(np.inf)), axis=0).astype(np.float64)      # the invalid ones last
    s = np.zeros((4, per), np.float64)
    with np.errstate(invalid='ignore', divide='ignore', over='ignore'):
        for j in range(N):
            live = j < n
            w = np.ones(per, np.float64)
            for r in range(4):
                if r:
                    w = w * (np.float64(j - r + 1) / (n - r).astype(np.float64))
                term = w * xs[j]
                use = live & (j >= r)
                s[r] = np.where(use, np.where(j == r, term, s[r] + term), s[r])
        out = s / n.astype(np.float64)
    out[np.arange(4)[:, None] >= n[None, :]] = np.nan
    return n.astype(np.int32), out


def clusters_cell(col, starts, thr, sign=1, run=1):
    """one cell: the list of (peak as x, position) of its clusters in order of occurrence, or None where thr is not finite"""
    if not np.isfinite(thr):
        return None
    sgn = np.float32(sign)
    u = float(sgn * np.float32(thr))
    col = np.asarray(col, np.float32)
    # float32 values as Python floats: exact, so every comparison below is the float32 comparison
    oks, vs = np.isfinite(col).tolist(), (sgn * canonical(col)).astype(np.float32).tolist()
    cuts = set(int(s) for s in starts[1:-1])
    found = []
    state = {'open': False, 'gap': 0, 'peak': None, 'pos': -1}

    def close():
        if state['open']:
            found.append((float(canonical(sgn * np.float32(state['peak']))), state['pos']))
        state['open'], state['gap'] = False, 0

    for n, (ok, v) in enumerate(zip(oks, vs)):
        if n in cuts:
            close()
        if not ok:
            close()
            continue
        if v > u:
            if not state['open'] or v > state['peak']:
                state['peak'], state['pos'] = v, n
            state['open'], state['gap'] = True, 0
        elif state['open']:
            state['gap'] += 1
            if state['gap'] >= run:
                close()
    close()
    return found


def pot_peaks(x, starts, thr, sign=1, run=1, K=None):
    """x (N, per) float32; thr (1,) or (per,) -> count int32 (per,), peak float32 (K, per), pos int32 (K, per); K None: the largest
    count"""
    x = np.asarray(x, np.float32)
    per = x.shape[1]
    thr = np.broadcast_to(np.asarray(thr, np.float32).reshape(-1), (per,))
    found = [clusters_cell(x[:, c], starts, thr[c], sign, run) for c in range(per)]
    count = np.array([-1 if f is None else len(f) for f in found], np.int32)
    if K is None:
        K = max(int(count.max()), 0)
    peak, pos = np.full((K, per), np.nan, np.float32), np.full((K, per), -1, np.int32)
    for c, f in enumerate(found):
        for k, (v, n) in enumerate((f or [])[:K]):
            peak[k, c], pos[k, c] = v, n
    return count, peak, pos


def block_maxima(x, starts, sign=1, min_valid=1):
    """x (N, per) -> float32 (P, per): the largest (sign +1) or smallest (-1) finite value per period, NaN below min_valid"""
    x = np.asarray(x, np.float32)
    out = np.full((len(starts) - 1, x.shape[1]), np.nan, np.float32)
    for p in range(len(starts) - 1):
        blk = canonical(x[starts[p]:starts[p + 1]])
        ok = np.isfinite(blk)
        with np.errstate(invalid='ignore'):
            m = np.where(ok, blk, -np.inf if sign > 0 else np.inf)
            m = m.max(axis=0) if sign > 0 else m.min(axis=0)
        out[p] = np.where(ok.sum(axis=0) >= max(min_valid, 1), m, np.nan)
    return out
