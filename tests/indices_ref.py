"""numpy restatement of dl4ds_climate_indices (include/dl4ds_hip.h).  It walks the samples of a period one by
one, in order, and is vectorised over the cells only: every fp64 addition happens in the order the definition gives, so the device
is compared with it bit for bit.  tests/test_indices_api.py checks it against independent statements (itertools.groupby, a plain
Python float loop, np.nanmax / np.nanmin) and hand-worked sequences."""
import numpy as np

OPS = (np.greater_equal, np.greater, np.less, np.less_equal)       # op 0..3
EVENT_ROWS = ('n_event', 'longest_event_run', 'longest_nonevent_run', 'n_event_runs', 'first_event', 'last_event')


def canonical(row):
    """float32 with -0.0 as +0.0"""
    row = np.asarray(row, np.float32)
    return np.where(row == 0, np.float32(0), row)


def climate_indices(x, starts, thr, op=0, window=5):
    """x (N, per) float32; starts (P + 1,); thr (T,) or (T, per) -> valid int32 (P, per), event int32 (P, T, 6, per), ext float32
    (P, 2, per), sums float64 (P, 2 + T, per)"""
    x = np.asarray(x, np.float32)
    N, per = x.shape
    thr = np.asarray(thr, np.float32)
    T = thr.shape[0]
    thr = np.broadcast_to(thr.reshape(T, -1), (T, per))
    thr_ok = np.isfinite(thr)
    P = len(starts) - 1
    valid, event = np.zeros((P, per), np.int32), np.zeros((P, T, 6, per), np.int32)
    ext, sums = np.zeros((P, 2, per), np.float32), np.zeros((P, 2 + T, per), np.float64)
    with np.errstate(invalid='ignore', over='ignore'):
        for p in range(P):
            s0, s1 = int(starts[p]), int(starts[p + 1])
            n_valid, run_v = np.zeros(per, np.int32), np.zeros(per, np.int32)
            vmax, vmin = np.full(per, -np.inf, np.float32), np.full(per, np.inf, np.float32)
            total, wmax = np.zeros(per, np.float64), np.full(per, -np.inf, np.float64)
            n_event, run_e, run_n, long_e, long_n, n_runs = (np.zeros((T, per), np.int32) for _ in range(6))
            first, last = np.full((T, per), -1, np.int32), np.full((T, per), -1, np.int32)
            esum = np.zeros((T, per), np.float64)
            for i in range(s1 - s0):
                ok = np.isfinite(x[s0 + i])
                v = canonical(x[s0 + i])
                d = v.astype(np.float64)
                n_valid += ok
                run_v = np.where(ok, run_v + 1, 0).astype(np.int32)
                total = np.where(ok, total + d, total)
                vmax = np.where(ok & (v > vmax), v, vmax)
                vmin = np.where(ok & (v < vmin), v, vmin)
                has = run_v >= window
                if has.any():                                   # the window that ends at sample i, formed afresh
                    s = np.zeros(per, np.float64)
                    for k in range(i - window + 1, i + 1):
                        s = s + canonical(x[s0 + k]).astype(np.float64)
                    wmax = np.where(has & (s > wmax), s, wmax)
                for t in range(T):
                    ev = ok & OPS[op](v, thr[t])
                    ne = ok & ~ev
                    n_runs[t] += ev & (run_e[t] == 0)
                    run_e[t] = np.where(ev, run_e[t] + 1, 0)
                    run_n[t] = np.where(ne, run_n[t] + 1, 0)
                    long_e[t] = np.maximum(long_e[t], run_e[t])
                    long_n[t] = np.maximum(long_n[t], run_n[t])
                    n_event[t] += ev
                    first[t] = np.where(ev & (first[t] < 0), i, first[t])
                    last[t] = np.where(ev, i, last[t])
                    esum[t] = np.where(ev, esum[t] + d, esum[t])
            valid[p] = n_valid
            ext[p, 0], ext[p, 1] = np.where(n_valid > 0, vmax, np.nan), np.where(n_valid > 0, vmin, np.nan)
            sums[p, 0] = np.where(n_valid > 0, total, np.nan)
            sums[p, 1] = np.where(wmax == -np.inf, np.nan, wmax)
            sums[p, 2:] = np.where(thr_ok, esum, np.nan)
            for j, a in enumerate((n_event, long_e, long_n, n_runs, first, last)):
                event[p, :, j] = np.where(thr_ok, a, -1)
    return valid, event, ext, sums


def named(x4, starts, thr, op=0, window=5):
    """`climate_indices` of an (N, H, W, C) array (thr (T,) or (T, H, W, C)) under the names of dl4ds_amd.indices.climate_indices"""
    x4 = np.asarray(x4, np.float32)
    grid = x4.shape[1:]
    thr = np.asarray(thr, np.float32)
    T = thr.shape[0]
    valid, event, ext, sums = climate_indices(x4.reshape(x4.shape[0], -1), starts, thr.reshape(T, -1) if thr.ndim > 1 else thr, op,
                                              window)
    P = valid.shape[0]
    out = {'n_valid': valid.reshape((P,) + grid)}
    for j, name in enumerate(EVENT_ROWS):
        out[name] = np.ascontiguousarray(event[:, :, j]).reshape((P, T) + grid)
    out['max'], out['min'] = ext[:, 0].reshape((P,) + grid), ext[:, 1].reshape((P,) + grid)
    out['sum'], out['max_window_sum'] = sums[:, 0].reshape((P,) + grid), sums[:, 1].reshape((P,) + grid)
    out['event_sum'] = np.ascontiguousarray(sums[:, 2:]).reshape((P, T) + grid)
    out['period_starts'] = np.asarray(starts, np.int64)
    return out
