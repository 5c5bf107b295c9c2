"""Climate indices along the time axis on the MI355X (csrc/indices.hip): spells, extremes, threshold days
and sums per grid cell and period, and the ETCCDI names built from them.

The reference has no counterpart: a user who has run ``predict`` over thirty years of days takes the field back to numpy or xarray
for CDD, Rx5day or the frost days.  ``climate_indices`` is one streaming read of the array on the device; the samples are in time
order, the periods (years, seasons) are independent, and a sample counts in a cell iff it is finite there (NaN is the mask).  The
definitions are those of ``dl4ds_climate_indices`` in include/dl4ds_hip.h.  numpy in / numpy out; a
``dl4ds_amd.device.DeviceArray`` is used where it lies.
"""
import numpy as np

from ._chunks import as_4d as _as_4d, cell_bands, check_4d_shape, check_batch_size, is_device as _is_device, is_int, masked, numeric_array

__all__ = ['climate_indices', 'precipitation_indices', 'temperature_indices', 'percentile_threshold', 'index_scores',
           'check_index_args', 'period_starts_from_labels', 'INDEX_OPS', 'INDEX_MAX_THRESHOLDS', 'INDEX_MAX_WINDOW']

INDEX_OPS = ('>=', '>', '<', '<=')                     # the `op` numbers of dl4ds_climate_indices
INDEX_MAX_THRESHOLDS, INDEX_MAX_WINDOW = 4, 32         # its caps
INDEX_LENGTH_BOUND = 1 << 31
EVENT_NAMES = ('n_event', 'longest_event_run', 'longest_nonevent_run', 'n_event_runs', 'first_event', 'last_event')


def period_starts_from_labels(labels):
    """(N,) non-decreasing integer labels (years, say; equal labels form a period) -> int64 (P + 1,) starts, first 0, last N."""
    labels = np.asarray(getattr(labels, 'values', labels))
    if labels.ndim != 1 or labels.size < 1 or not np.issubdtype(labels.dtype, np.integer):
        raise ValueError('`periods` must be a non-empty 1-D array of integer labels, one per sample')
    step = np.diff(labels.astype(np.int64))
    if (step < 0).any():
        raise ValueError('`periods` must be non-decreasing: the samples are in time order')
    return np.concatenate(([0], np.flatnonzero(step) + 1, [labels.size])).astype(np.int64)


def check_index_args(shape, periods=None, thresholds=(1.0,), op='>=', window=5, batch_size=None, period_starts=None):
    """Validation of `climate_indices` from the arguments alone (no library call).  ``shape``: the array's (N, H, W, C).
    -> (period starts int64 (P + 1,), thresholds float32 (T,) or (T, H, W, C), the number of ``op``)."""
    shape = check_4d_shape(shape)
    N = shape[0]
    if N >= INDEX_LENGTH_BOUND:
        raise ValueError(f'the array has {N} samples: the number must stay below 2^31')
    if op not in INDEX_OPS:
        raise ValueError(f"`op` must be one of {INDEX_OPS}, got {op!r}")
    if not is_int(window) or not 1 <= window <= INDEX_MAX_WINDOW:
        raise ValueError(f'`window` must be an integer between 1 and {INDEX_MAX_WINDOW}, got {window!r}')
    check_batch_size(batch_size)
    if periods is not None and period_starts is not None:
        raise ValueError('give `periods` (labels) or `period_starts`, not both')
    if period_starts is not None:
        starts = np.asarray(period_starts)
        if starts.ndim != 1 or starts.size < 2 or not np.issubdtype(starts.dtype, np.integer):
            raise ValueError('`period_starts` must be a 1-D integer array of P + 1 >= 2 entries')
        starts = starts.astype(np.int64)
        if starts[0] != 0 or starts[-1] != N or not (np.diff(starts) > 0).all():
            raise ValueError(f'`period_starts` must be strictly increasing from 0 to N = {N}')
    elif periods is not None:
        starts = period_starts_from_labels(periods)
        if starts[-1] != N:
            raise ValueError(f'`periods` has {starts[-1]} labels for {N} samples')
    else:
        starts = np.array([0, N], np.int64)
    thr = numeric_array(thresholds, '`thresholds` must be numbers')
    if thr.ndim == 0:
        thr = thr.reshape(1)
    if thr.ndim == 3 and shape[3] == 1:
        thr = thr[..., None]
    if thr.ndim not in (1, 4) or (thr.ndim == 4 and thr.shape[1:] != shape[1:]):
        raise ValueError(f'`thresholds` must be T scalars or a (T, H, W, C) field on the grid {shape[1:]}, got shape {thr.shape}')
    if not 1 <= thr.shape[0] <= INDEX_MAX_THRESHOLDS:
        raise ValueError(f'between 1 and {INDEX_MAX_THRESHOLDS} thresholds are supported, got {thr.shape[0]}')
    return np.ascontiguousarray(starts), np.ascontiguousarray(thr, np.float32), INDEX_OPS.index(op)


def _named(valid, event, ext, sums, starts, grid):
    """The four flat outputs [P][...][per] -> the dict of (P, H, W, C) / (P, T, H, W, C) arrays."""
    P, T = event.shape[:2]
    out = {'n_valid': valid.reshape((P,) + grid)}
    for j, name in enumerate(EVENT_NAMES):
        out[name] = np.ascontiguousarray(event[:, :, j]).reshape((P, T) + grid)
    out['max'], out['min'] = ext[:, 0].reshape((P,) + grid), ext[:, 1].reshape((P,) + grid)
    out['sum'], out['max_window_sum'] = sums[:, 0].reshape((P,) + grid), sums[:, 1].reshape((P,) + grid)
    out['event_sum'] = np.ascontiguousarray(sums[:, 2:]).reshape((P, T) + grid)
    out['period_starts'] = starts
    return out


def climate_indices(x, periods=None, thresholds=(1.0,), op='>=', window=5, mask=None, batch_size=None, period_starts=None):
    """Per grid cell and period of ``x`` (N, H, W, C; samples in time order), in one pass on the device.

    * ``periods``: None (one period), or (N,) non-decreasing integer labels such as years (equal labels form a period); or
      ``period_starts=`` directly, P + 1 strictly increasing integers from 0 to N.  Periods are independent: a run is cut at a
      boundary and a window lies inside one period.
    * ``thresholds``: T <= 4 scalars or a (T, H, W, C) field (NaN: no threshold in that cell); a valid sample is an event of
      threshold t iff ``x op threshold`` (``op``: '>=', '>', '<', '<=', compared on float32).
    * ``mask`` (2-D, or with a channel axis; 0 = excluded) and non-finite values exclude samples; an excluded sample ends a run.
    * Host arrays are uploaded in bands of grid rows with the whole time axis (``batch_size`` rows per band, by default at most
      256 MiB); the result does not depend on it.

    -> dict of ``n_valid`` int32 (P, H, W, C); ``n_event``, ``longest_event_run``, ``longest_nonevent_run``, ``n_event_runs``,
    ``first_event``, ``last_event`` (offsets from the period's first sample, -1 without an event) int32 (P, T, H, W, C), all -1
    where the threshold is not finite; ``max``, ``min`` float32 (NaN without a valid sample); ``sum``, ``max_window_sum`` (the
    largest sum of ``window`` consecutive valid samples; NaN without one) float64; ``event_sum`` float64 (P, T, H, W, C);
    ``period_starts`` int64 (P + 1,)."""
    from . import _lib
    x, shape = _as_4d(x)
    starts, thr, opn = check_index_args(shape, periods, thresholds, op, window, batch_size, period_starts)
    x = masked(x, mask)
    lib = _lib.lib()
    N, H, W, C = shape
    per, P, T, cell = H * W * C, len(starts) - 1, thr.shape[0], thr.ndim == 4
    valid, event = np.empty((P, per), np.int32), np.empty((P, T, 6, per), np.int32)
    ext, sums = np.empty((P, 2, per), np.float32), np.empty((P, 2 + T, per), np.float64)

    def call(band):
        _lib.check(lib.dl4ds_climate_indices(band.x, N, band.cells, starts.ctypes.data, P, band.fields[0], T, int(cell), opn,
                                             int(window), *band.outs))
    cell_bands(x, None, shape, (valid, event, ext, sums), call, batch_size, fields=(thr,))
    return _named(valid, event, ext, sums, starts, (H, W, C))


def _precipitation_from(r, window):
    """The ETCCDI names of a `climate_indices` result at the thresholds (wet, heavy[0], heavy[1]) under '>='."""
    wet_days, wet_sum = r['n_event'][:, 0], r['event_sum'][:, 0]
    with np.errstate(invalid='ignore', divide='ignore'):
        sdii = np.where(wet_days > 0, wet_sum / np.where(wet_days > 0, wet_days, 1), np.nan)
    out = {'rx1day': r['max'], f'rx{window}day': r['max_window_sum'], 'prcptot': r['sum'], 'sdii': sdii, 'r1mm': wet_days,
           'cwd': r['longest_event_run'][:, 0], 'cdd': r['longest_nonevent_run'][:, 0], 'n_valid': r['n_valid'],
           'period_starts': r['period_starts']}
    for t in range(1, r['n_event'].shape[1]):
        out[('r10mm', 'r20mm')[t - 1]] = r['n_event'][:, t]
    return out


def precipitation_indices(pr, periods=None, wet=1.0, heavy=(10.0, 20.0), window=5, mask=None, batch_size=None, period_starts=None):
    """ETCCDI precipitation indices per cell and period, one device call (T = 3, '>='): ``rx1day``, ``rx{window}day`` (``rx5day``),
    ``prcptot`` (the sum of all valid days), ``sdii`` (the wet-day sum over ``r1mm``; NaN without wet days), ``r1mm`` / ``r10mm`` /
    ``r20mm`` (days at or above ``wet`` / ``heavy``), ``cwd`` / ``cdd`` (the longest run of wet / of valid dry days), ``n_valid``."""
    heavy = tuple(np.atleast_1d(heavy))
    if len(heavy) != 2:
        raise ValueError('`heavy` must be two thresholds (R10mm and R20mm)')
    r = climate_indices(pr, periods, (wet,) + heavy, '>=', window, mask, batch_size, period_starts)
    return _precipitation_from(r, window)


def _temperature_from(lo, hi):
    """The names of two `climate_indices` results, under '<' ``below`` and under '>' ``above``."""
    n = lo['n_valid']
    with np.errstate(invalid='ignore', divide='ignore'):
        mean = np.where(n > 0, lo['sum'] / np.where(n > 0, n, 1), np.nan)
    return {'txx': lo['max'], 'tnn': lo['min'], 'mean': mean, 'days_below': lo['n_event'][:, 0], 'days_above': hi['n_event'][:, 0],
            'longest_run_below': lo['longest_event_run'][:, 0], 'longest_run_above': hi['longest_event_run'][:, 0], 'n_valid': n,
            'period_starts': lo['period_starts']}


def temperature_indices(t, periods=None, below=0.0, above=25.0, mask=None, batch_size=None, period_starts=None):
    """Temperature indices per cell and period, two device calls ('<' ``below``: frost days for daily minima in degrees Celsius; '>'
    ``above``: summer days for daily maxima): ``txx``, ``tnn``, ``mean``, ``days_below``, ``days_above``, ``longest_run_below``,
    ``longest_run_above``, ``n_valid``."""
    lo = climate_indices(t, periods, (below,), '<', 1, mask, batch_size, period_starts)
    hi = climate_indices(t, periods, (above,), '>', 1, mask, batch_size, period_starts)
    return _temperature_from(lo, hi)


def percentile_threshold(x, q, wet=None, mask=None):
    """Per-cell float32 (1, H, W, C) threshold field for indices such as R95pTOT: the ``q``-th percentile (0..100) over all samples
    of the host array ``x``, values below ``wet`` dropped first (set to NaN), from `dl4ds_quantile_table`.  NaN in a cell without a
    value left."""
    from .metrics import _masked_observation
    from .postprocessing import _device_table
    if _is_device(x):
        raise TypeError('`percentile_threshold` takes host arrays only')
    if not 0.0 <= float(q) <= 100.0:
        raise ValueError(f'`q` must be a percentile in [0, 100], got {q!r}')
    x, shape = _as_4d(x)
    x = _masked_observation(x, mask)                                    # (a float32 copy)
    if wet is not None:
        with np.errstate(invalid='ignore'):
            x[x < np.float32(wet)] = np.nan
    # two knots: the table entry takes at least two probabilities
    p = float(q) / 100.0
    probs = np.array([p, 1.0] if p < 1.0 else [0.0, 1.0], np.float64)
    table = _device_table(x, shape, probs)[0]
    return np.ascontiguousarray(table[0 if p < 1.0 else 1][None])


def _bias(obs, pred):
    skip = ('period_starts',)
    out = {}
    for name in obs:
        if name in skip:
            continue
        o, p = np.asarray(obs[name], np.float64), np.asarray(pred[name], np.float64)
        bias = p - o
        out[name] = {'obs': o, 'pred': p, 'bias': bias, 'mean_bias': bias.mean(axis=0)}
    return out


def index_scores(obs, pred, kind='precipitation', mask=None, **kw):
    """The indices of an observation and of a prediction side by side -> per index ``{'obs', 'pred', 'bias', 'mean_bias'}`` in float64:
    the two maps (P, H, W, C), ``bias = pred - obs`` per period and its mean over the periods (NaN stays NaN: a cell with a NaN in
    one period has a NaN mean).  ``kind``: 'precipitation' or 'temperature'; ``kw`` goes to that function."""
    fns = {'precipitation': precipitation_indices, 'temperature': temperature_indices}
    if kind not in fns:
        raise ValueError(f"`kind` must be 'precipitation' or 'temperature', got {kind!r}")
    return _bias(fns[kind](obs, mask=mask, **kw), fns[kind](pred, mask=mask, **kw))
