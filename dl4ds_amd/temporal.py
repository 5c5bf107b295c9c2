"""Temporal verification on the MI355X (csrc/temporal.hip, csrc/trend.hip): day-to-day persistence (lag-k
autocorrelation, event transition probabilities), the distribution of spell lengths, and the trend per grid cell (Mann-Kendall,
Sen's slope).

The reference has no counterpart.  ``temporal_statistics`` is one streaming read of the array on the device, ``temporal_scores``
one read of an observation and a prediction together, on the days both have; the samples are in time order, the periods (years,
seasons) are independent, and a sample counts in a cell iff it is finite there (NaN is the mask).  The device returns raw sums
and counts, as defined for ``dl4ds_temporal`` and ``dl4ds_trend`` in include/dl4ds_hip.h; the statistics are formed from them in
float64 numpy by ``temporal_from_sums`` and ``mann_kendall``.  numpy in / numpy out; a ``dl4ds_amd.device.DeviceArray`` is used
where it lies.
"""
import math

import numpy as np

from ._chunks import as_4d as _as_4d, cell_bands, check_batch_size, is_device as _is_device, is_int, masked
from .indices import check_index_args

__all__ = ['temporal_statistics', 'temporal_scores', 'temporal_from_sums', 'mann_kendall', 'trend_scores', 'check_temporal_args',
           'TEMPORAL_MAX_LAGS', 'TEMPORAL_MAX_LAG', 'TEMPORAL_MAX_THRESHOLDS', 'TEMPORAL_MAX_BINS', 'TREND_MAX_PERIODS']

TEMPORAL_MAX_LAGS, TEMPORAL_MAX_LAG, TEMPORAL_MAX_THRESHOLDS, TEMPORAL_MAX_BINS = 4, 32, 4, 32      # the caps of dl4ds_temporal
TREND_MAX_PERIODS = 128                                                                            # the cap of dl4ds_trend
RAW_NAMES = ('n_valid', 'sum', 'sum_sq', 'n_pairs', 'lag_sums', 'transitions', 'spell_hist')
BIAS_NAMES = ('acf', 'p_event_given_event', 'p_event_given_nonevent', 'mean_event_spell', 'mean_nonevent_spell')


def check_temporal_args(shape, periods=None, lags=(1,), thresholds=(), op='>=', spell_bins=16, batch_size=None, period_starts=None):
    """Validation of `temporal_statistics` from the arguments alone (no library call).  ``shape``: the array's (N, H, W, C).
    -> (period starts int64 (P + 1,), lags int32 (L,), thresholds float32 (T,) or (T, H, W, C), the number of ``op``)."""
    thr = np.asarray(getattr(thresholds, 'values', () if thresholds is None else thresholds))
    none = thr.size == 0 and thr.ndim <= 1
    starts, thr, opn = check_index_args(shape, periods, (0.0,) if none else thresholds, op, 1, batch_size, period_starts)
    if none:
        thr = np.zeros((0,), np.float32)
    try:
        lags = [lags] if is_int(lags) else list(lags)
    except TypeError:
        raise ValueError(f'`lags` must be integers, got {lags!r}') from None
    if not all(is_int(v) for v in lags):
        raise ValueError(f'`lags` must be integers, got {lags!r}')
    if len(lags) > TEMPORAL_MAX_LAGS:
        raise ValueError(f'at most {TEMPORAL_MAX_LAGS} lags are supported, got {len(lags)}')
    if any(not 1 <= v <= TEMPORAL_MAX_LAG for v in lags) or any(b <= a for a, b in zip(lags, lags[1:])):
        raise ValueError(f'`lags` must be strictly increasing, each between 1 and {TEMPORAL_MAX_LAG}, got {lags!r}')
    if not is_int(spell_bins) or not 1 <= spell_bins <= TEMPORAL_MAX_BINS:
        raise ValueError(f'`spell_bins` must be an integer between 1 and {TEMPORAL_MAX_BINS}, got {spell_bins!r}')
    return starts, np.asarray(lags, np.int32).reshape(-1), thr, opn


def _ratio(num, den, ok=True):
    """num / den in float64, NaN where den <= 0 or ``ok`` does not hold"""
    num, den = np.asarray(num, np.float64), np.asarray(den, np.float64)
    good = (den > 0) & ok
    return np.where(good, num / np.where(good, den, 1.0), np.nan)


def temporal_from_sums(raw):
    """The statistics of one series from the raw device outputs ``raw`` (the entries ``n_valid``, ``sum``, ``sum_sq``, ``n_pairs``,
    ``lag_sums``, ``transitions``, ``spell_hist`` of `temporal_statistics`, period axis first), in float64:

    * ``mean`` = sum / n and ``variance`` = sum_sq / n - mean^2 (P, ...);
    * ``acf`` (P, L, ...) = [sum ab - m (sum a + sum b) + n_l m^2] / [sum_sq - n m^2], the usual estimator with the period's own
      mean m; NaN where the denominator is <= 0 or there is no pair;
    * ``p_event_given_event`` = n11 / (n10 + n11) and ``p_event_given_nonevent`` = n01 / (n00 + n01) (P, T, ...);
    * ``mean_event_spell`` = (n11 + runs) / runs with ``runs`` the histogram's total of event runs: every event is either the first
      of its run or the second sample of a 1 -> 1 transition; ``mean_nonevent_spell`` likewise from n00 (P, T, ...).

    Wherever the device wrote -1 (no finite threshold) or a count is 0 the value is NaN."""
    n = np.asarray(raw['n_valid'], np.float64)
    s, q = np.asarray(raw['sum'], np.float64), np.asarray(raw['sum_sq'], np.float64)
    with np.errstate(invalid='ignore', divide='ignore', over='ignore'):
        mean = _ratio(s, n)
        out = {'mean': mean, 'variance': _ratio(q, n) - mean * mean}
        pairs, ls = np.asarray(raw['n_pairs'], np.float64), np.asarray(raw['lag_sums'], np.float64)
        m = mean[:, None]
        num = ls[:, :, 2] - m * (ls[:, :, 0] + ls[:, :, 1]) + pairs * (m * m)
        den = np.broadcast_to((q - n * (mean * mean))[:, None], num.shape)
        out['acf'] = _ratio(num, den, pairs > 0)
        tr = np.asarray(raw['transitions'], np.float64)
        n00, n01, n10, n11 = tr[:, :, 0], tr[:, :, 1], tr[:, :, 2], tr[:, :, 3]
        out['p_event_given_event'] = _ratio(n11, n10 + n11, n11 >= 0)
        out['p_event_given_nonevent'] = _ratio(n01, n00 + n01, n01 >= 0)
        runs = np.asarray(raw['spell_hist'], np.float64).sum(axis=3)                     # (P, T, 2, ...)
        out['mean_event_spell'] = _ratio(n11 + runs[:, :, 0], runs[:, :, 0], n11 >= 0)
        out['mean_nonevent_spell'] = _ratio(n00 + runs[:, :, 1], runs[:, :, 1], n00 >= 0)
    return out


def _named(flat, s, starts, grid):
    """Series ``s`` of the six flat outputs [P][...][per] -> the dict of raw (P, ..., H, W, C) arrays with the derived statistics"""
    valid, moment, pair, lag, trans, spell = flat
    P = valid.shape[0]

    def grid_of(a):
        return np.ascontiguousarray(a).reshape(a.shape[:-1] + grid)
    out = {'n_valid': grid_of(valid), 'sum': grid_of(moment[:, s, 0]), 'sum_sq': grid_of(moment[:, s, 1]), 'n_pairs': grid_of(pair),
           'lag_sums': grid_of(lag[:, s]), 'transitions': grid_of(trans[:, s]), 'spell_hist': grid_of(spell[:, s])}
    assert out['n_valid'].shape[0] == P
    out.update(temporal_from_sums(out))
    out['period_starts'] = starts
    return out


def _device_temporal(y, p, shape, starts, lags, thr, opn, bins, batch_size):
    """One `dl4ds_temporal` call per band of grid rows (or one on DeviceArrays) -> the six flat host outputs [P][...][per]"""
    from . import _lib
    lib = _lib.lib()
    N, H, W, C = shape
    per, P, S, L, T, cell = H * W * C, len(starts) - 1, 1 if p is None else 2, len(lags), thr.shape[0], thr.ndim == 4
    hosts = (np.empty((P, per), np.int32), np.empty((P, S, 2, per), np.float64), np.empty((P, L, per), np.int32),
             np.empty((P, S, L, 3, per), np.float64), np.empty((P, S, T, 4, per), np.int32), np.empty((P, S, T, 2, bins, per), np.int32))

    def call(band):
        _lib.check(lib.dl4ds_temporal(band.x, band.pred, N, band.cells, starts.ctypes.data, P, lags.ctypes.data if L else None, L,
                                      band.fields[0], T, int(cell), opn, int(bins), *band.outs))
    cell_bands(y, p, shape, [h if h.size else None for h in hosts], call, batch_size, fields=(thr,))
    return hosts


def _series(x, p, periods, lags, thresholds, op, spell_bins, mask, batch_size, period_starts):
    """The shared front of `temporal_statistics` (p None) and `temporal_scores` -> (flat outputs, starts, grid)"""
    x, shape = _as_4d(x)
    if p is not None:
        p, pshape = _as_4d(p, 'pred')
        if pshape != shape or _is_device(p) != _is_device(x):
            raise ValueError(f'expected two arrays of one shape and kind, got {shape} and {pshape}')
    starts, lags, thr, opn = check_temporal_args(shape, periods, lags, thresholds, op, spell_bins, batch_size, period_starts)
    return _device_temporal(masked(x, mask), p, shape, starts, lags, thr, opn, spell_bins, batch_size), starts, tuple(shape[1:])


def temporal_statistics(x, periods=None, lags=(1,), thresholds=(), op='>=', spell_bins=16, mask=None, batch_size=None,
                        period_starts=None):
    """Per grid cell and period of ``x`` (N, H, W, C; samples in time order), in one pass on the device.

    * ``periods`` / ``period_starts``, ``thresholds`` (T <= 4 scalars or a (T, H, W, C) field; none: no event statistics), ``op``,
      ``mask`` and ``batch_size`` as in `dl4ds_amd.indices.climate_indices`; nothing carries across a period boundary.
    * ``lags``: up to 4 strictly increasing lags between 1 and 32.
    * ``spell_bins`` B (1..32): bin k - 1 of a spell histogram counts the runs of length k, the last bin those of length >= B.

    -> dict of the raw device outputs ``n_valid`` int32 (P, H, W, C); ``sum``, ``sum_sq`` float64 (P, H, W, C); ``n_pairs`` int32
    (P, L, H, W, C); ``lag_sums`` float64 (P, L, 3, H, W, C) (sum a, sum b, sum ab over the pairs (n, n + lag)); ``transitions``
    int32 (P, T, 4, H, W, C) (n00, n01, n10, n11); ``spell_hist`` int32 (P, T, 2, B, H, W, C) (event runs, non-event runs), -1 where
    the threshold is not finite; ``period_starts``; and of the statistics `temporal_from_sums` forms from them."""
    flat, starts, grid = _series(x, None, periods, lags, thresholds, op, spell_bins, mask, batch_size, period_starts)
    return _named(flat, 0, starts, grid)


def temporal_scores(obs, pred, periods=None, lags=(1,), thresholds=(), op='>=', spell_bins=16, mask=None, batch_size=None,
                    period_starts=None):
    """`temporal_statistics` of an observation and of a prediction in one device call, on common validity: a sample counts in a
    cell iff both are finite there, so the two sides describe the same days.  -> ``{'obs', 'pred'}`` (the two dicts), ``'bias'``
    (pred - obs of ``acf``, ``p_event_given_event``, ``p_event_given_nonevent``, ``mean_event_spell``, ``mean_nonevent_spell``
    per period) and ``'mean_bias'`` (its mean over the periods; NaN stays NaN)."""
    flat, starts, grid = _series(obs, pred, periods, lags, thresholds, op, spell_bins, mask, batch_size, period_starts)
    o, p = _named(flat, 0, starts, grid), _named(flat, 1, starts, grid)
    bias = {name: p[name] - o[name] for name in BIAS_NAMES}
    return {'obs': o, 'pred': p, 'bias': bias, 'mean_bias': {name: b.mean(axis=0) for name, b in bias.items()}}


# ------------------------------------------------------------------------------------------------------------------------ trend
def _trend_values(values, mask=None):
    """-> (float64 (P, H, W, C) host array or the float64 DeviceArray, its shape as (P, H, W, C))"""
    if _is_device(values):
        if values.dtype != np.float64:
            raise TypeError(f'`values`: a DeviceArray must hold float64, got {values.dtype}')
        masked(values, mask)                                                             # (refuses a mask)
        shape = tuple(values.shape) + ((1,) if len(values.shape) == 3 else ())
    else:
        values = np.array(getattr(values, 'values', values), np.float64)                 # (a copy: the mask is written into it)
        if values.ndim == 3:
            values = values[..., None]
        shape = values.shape
        if mask is not None:
            mask = np.asarray(getattr(mask, 'values', mask))
            if mask.ndim == 2:
                mask = mask[..., None]
            try:
                values[np.broadcast_to(mask == 0, shape)] = np.nan
            except ValueError:
                raise ValueError(f'`mask` of shape {mask.shape} does not broadcast to the values {shape}') from None
    if len(shape) != 4 or min(shape) < 1:
        raise ValueError(f'expected a non-empty (P, H, W[, C]) array, got shape {shape}')
    if shape[0] > TREND_MAX_PERIODS:
        raise ValueError(f'at most {TREND_MAX_PERIODS} periods are supported, got {shape[0]}')
    return values, tuple(int(v) for v in shape)


def mann_kendall_from_counts(n, s, ties, sen_slope):
    """The Mann-Kendall test from the device's counts, in float64: ``var_s`` = [n(n-1)(2n+5) - ties] / 18; ``z`` = (s -+ 1) /
    sqrt(var_s) with the continuity correction towards zero, 0 when s = 0, NaN when var_s <= 0; ``p_value`` = erfc(|z| / sqrt 2)."""
    nf, sf = np.asarray(n, np.float64), np.asarray(s, np.float64)
    var_s = (nf * (nf - 1.0) * (2.0 * nf + 5.0) - np.asarray(ties, np.float64)) / 18.0
    with np.errstate(invalid='ignore', divide='ignore'):
        z = np.where(var_s > 0, (sf - np.sign(sf)) / np.sqrt(np.where(var_s > 0, var_s, 1.0)), np.nan)
    p_value = np.vectorize(math.erfc, otypes=[np.float64])(np.abs(z) / math.sqrt(2.0))
    return {'n': n, 's': s, 'var_s': var_s, 'z': z, 'p_value': p_value, 'sen_slope': sen_slope}


def mann_kendall(values, mask=None, batch_size=None):
    """Trend per grid cell of ``values`` (P, H, W[, C]), one value per period in period order (an annual index from
    `climate_indices`, say; P <= 128).  Time is the period index; a non-finite value is a gap and keeps its place in time.
    -> dict of (H, W, C) arrays: ``n`` int32 valid values; ``s`` int64, the Mann-Kendall statistic; ``var_s``, ``z``, ``p_value``
    (two-sided) float64 as in `mann_kendall_from_counts`; ``sen_slope`` float64, the median of the pairwise slopes per period step
    (NaN with fewer than two values).  Host arrays go up in bands of ``batch_size`` grid rows; the result does not depend on it."""
    from . import _lib
    check_batch_size(batch_size)
    values, shape = _trend_values(values, mask)
    lib = _lib.lib()
    P, H, W, C = shape
    per = H * W * C
    n, mk, sen = np.empty(per, np.int32), np.empty((2, per), np.int64), np.empty(per, np.float64)
    cell_bands(values, None, shape, (n, mk, sen), lambda band: _lib.check(lib.dl4ds_trend(band.x, P, band.cells, *band.outs)),
               batch_size, dtype=np.float64)
    grid = (H, W, C)
    return mann_kendall_from_counts(n.reshape(grid), mk[0].reshape(grid), mk[1].reshape(grid), sen.reshape(grid))


def trend_scores(obs, pred, mask=None):
    """`mann_kendall` of an observation and of a prediction -> ``{'obs', 'pred'}`` (the two dicts), ``'slope_bias'`` = pred - obs of
    ``sen_slope`` per cell, and ``'sign_agreement'``: the fraction of all cells where both slopes are finite and have the same
    sign."""
    o, p = mann_kendall(obs, mask), mann_kendall(pred, mask)
    a, b = o['sen_slope'], p['sen_slope']
    agree = np.isfinite(a) & np.isfinite(b) & (np.sign(a) == np.sign(b))
    return {'obs': o, 'pred': p, 'slope_bias': b - a, 'sign_agreement': float(agree.mean())}
