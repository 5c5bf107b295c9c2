"""Distance and displacement measures on binary event fields (no counterpart in the reference): how far, in
grid cells, the predicted event area lies from the observed one.  Everything rests on the exact Euclidean distance transform of a
binary field, which runs on the device together with the sums of the scores (`dl4ds_distance_scores`, csrc/distance.hip;
tests/distance_ref.py is its restatement): `distance_transform` for one array, `distance_scores` for an observation and a
prediction (Hausdorff distance, mean error and RMS distances, Baddeley's Delta, Pratt's figure of merit), and the host parts
`check_distance_args` (the argument rules) and `distance_from_sums` (the arithmetic on the device's sums)."""
import math

import numpy as np

from . import _exact
from ._chunks import as_4d, check_4d_shape, check_batch_size, is_device, masked, paired_chunks

DIST_EMPTY = (1 << 31) - 1                         # the squared distance to an empty set; reads as +inf
DIST_CELL_BOUND = 1 << 31                          # H*W must stay below it
PRATT_DEFAULT_ALPHA = 1.0 / 9.0
COUNT_NAMES = ('n_valid', 'n_obs', 'n_pred', 'n_both', 'max_d2_obs_to_pred', 'max_d2_pred_to_obs', 'sum_d2_obs_to_pred',
               'sum_d2_pred_to_obs')
SUM_NAMES = ('sum_d_obs_to_pred', 'sum_d_pred_to_obs', 'pratt_obs_to_pred', 'pratt_pred_to_obs', 'baddeley_sum', 'baddeley_sum2',
             'baddeley_max')
SCORE_NAMES = ('hausdorff', 'med_obs_to_pred', 'med_pred_to_obs', 'rms_obs_to_pred', 'rms_pred_to_obs', 'baddeley1', 'baddeley2',
               'baddeley_max', 'pratt')


def _number(v, name):
    if isinstance(v, (bool, np.bool_)) or not isinstance(v, (int, float, np.integer, np.floating)):
        raise ValueError(f'`{name}` must be a number, got {v!r}')
    return float(v)


def check_distance_args(shape, thresholds, cutoff=None, alpha=PRATT_DEFAULT_ALPHA, batch_size=None):
    """The argument rules of a distance request on (N, H, W, C) = ``shape`` arrays (no library call) -> (thresholds as float32
    (T,), cutoff, alpha as floats).  ``cutoff`` None: the field diagonal sqrt((H-1)^2 + (W-1)^2), 1 on a field of one cell."""
    _, h, w, _ = check_4d_shape(shape)
    if (h - 1) ** 2 + (w - 1) ** 2 >= DIST_EMPTY:
        raise ValueError(f'fields of {h} x {w} cells are not supported: (H-1)^2 + (W-1)^2 must stay below 2^31 - 1')
    if h * w >= DIST_CELL_BOUND:
        raise ValueError(f'fields of H*W = {h * w} cells are not supported: H*W must stay below 2^31')
    t = np.asarray(getattr(thresholds, 'values', thresholds))
    if t.dtype == object or t.dtype == bool or not (np.issubdtype(t.dtype, np.floating) or np.issubdtype(t.dtype, np.integer)):
        raise ValueError('`thresholds` must be a number or a 1-D sequence of numbers')
    thr = _exact.finite_float32(np.atleast_1d(t), '`thresholds`')
    if len(thr) >= 1 << 31:
        raise ValueError('too many `thresholds`')
    if cutoff is None:
        cutoff = math.sqrt((h - 1) ** 2 + (w - 1) ** 2) or 1.0
    cutoff = _number(cutoff, 'cutoff')
    if not cutoff > 0:
        raise ValueError(f'`cutoff` must be > 0 (it may be inf), got {cutoff!r}')
    alpha = _number(alpha, 'alpha')
    if not (alpha > 0 and math.isfinite(alpha)):
        raise ValueError(f'`alpha` must be positive and finite, got {alpha!r}')
    check_batch_size(batch_size)
    return thr, cutoff, alpha


def _finite(a):
    return np.where(np.isfinite(a), a, np.nan)


def _mean(a):
    """mean over the fields (the two leading axes) that are not NaN, NaN when there is none -> (T,)"""
    ok = ~np.isnan(a)
    n = ok.sum(axis=(0, 1))
    return _exact.ratio(np.where(ok, a, 0.0).sum(axis=(0, 1)), n)


def distance_from_sums(counts, sums, shape, thresholds):
    """The scores from the sums of `dl4ds_distance_scores` on (N, H, W, C) = ``shape`` arrays (host arithmetic only): ``counts``
    (N*C, T, 8) int64 and ``sums`` (N*C, T, 7) fp64 in the entry's order.  With A the observed and B the
    predicted event set -> a dict of (N, C, T) arrays: ``hausdorff`` = sqrt(max(max d2(a, B), max d2(b, A))), ``med_obs_to_pred``
    = sum d(a, B) / n_A and ``med_pred_to_obs``, ``rms_obs_to_pred`` = sqrt(sum d2(a, B) / n_A) and ``rms_pred_to_obs``, ``pratt``
    = sum over B of 1 / (1 + alpha d2(b, A)) / max(n_A, n_B): all NaN where A or B is empty; ``baddeley1`` = sum w / n_valid,
    ``baddeley2`` = sqrt(sum w^2 / n_valid), ``baddeley_max`` = max w: NaN without a valid cell or where the sum is not finite (both
    sets empty under an infinite cutoff); ``n_obs``, ``n_pred``, ``n_both``, ``n_valid`` int64; each score's mean over the fields
    that are not NaN as ``hausdorff_mean`` ... (T,); ``thresholds``; the sums themselves under ``counts`` and ``sums``."""
    N, H, W, C = check_4d_shape(shape)
    thr = np.asarray(thresholds, np.float32).reshape(-1)
    T = len(thr)
    counts = np.asarray(counts, np.int64).reshape(N, C, T, 8)
    sums = np.asarray(sums, np.float64).reshape(N, C, T, 7)
    nv, na, nb, nab, mab, mba, s2ab, s2ba = (counts[..., k] for k in range(8))
    both = (na > 0) & (nb > 0)
    some = nv > 0
    pick = lambda ok, a: np.where(ok, a, np.nan)                        # noqa: E731
    with np.errstate(invalid='ignore', divide='ignore', over='ignore'):
        res = dict(hausdorff=pick(both, np.sqrt(np.maximum(mab, mba).astype(np.float64))),
                   med_obs_to_pred=pick(both, _exact.ratio(sums[..., 0], na)), med_pred_to_obs=pick(both, _exact.ratio(sums[..., 1], nb)),
                   rms_obs_to_pred=pick(both, np.sqrt(_exact.ratio(s2ab, na))), rms_pred_to_obs=pick(both, np.sqrt(_exact.ratio(s2ba, nb))),
                   baddeley1=_exact.ratio(sums[..., 4], nv), baddeley2=np.sqrt(_exact.ratio(sums[..., 5], nv)),
                   baddeley_max=pick(some, sums[..., 6]), pratt=pick(both, _exact.ratio(sums[..., 3], np.maximum(na, nb))))
    res = {k: _finite(v) for k, v in res.items()}
    res.update({k + '_mean': _mean(v) for k, v in list(res.items())})
    res.update(n_obs=na, n_pred=nb, n_both=nab, n_valid=nv, thresholds=thr, counts=counts, sums=sums)
    return res


def _run(obs, pred, shape, thr, cutoff, alpha, batch_size, maps):
    """The library calls: ``obs`` / ``pred`` float32 DeviceArrays, used where they lie, or host arrays, which go up in chunks of
    whole samples; ``pred`` None: the observation serves as both sides.  ``maps``: which of the two squared maps are wanted.
    -> (counts (F, T, 8), sums (F, T, 7), [d2_obs, d2_pred] as (F, T, H, W) int32 or None)."""
    from . import _lib
    from .device import Buffers, sync
    N, H, W, C = shape
    F, T = N * C, len(thr)
    lib = _lib.lib()
    thr = np.ascontiguousarray(thr, np.float32)
    counts, sums = np.zeros((F, T, 8), np.int64), np.zeros((F, T, 7), np.float64)
    d2 = [np.zeros((F, T, H, W), np.int32) if m else None for m in maps]

    def call(b, dy, dp, dcounts, dsums, dmaps):
        _lib.check(lib.dl4ds_distance_scores(dy, dp if dp is not None else dy, b, H, W, C, thr.ctypes.data, T, cutoff, alpha, dcounts,
                                             dsums, dmaps[0], dmaps[1]))
        sync()

    if is_device(obs):
        with Buffers() as buf:
            dc, ds = buf.alloc(counts.shape, counts.dtype), buf.alloc(sums.shape, sums.dtype)
            dm = [buf.alloc(m.shape, m.dtype) if m is not None else None for m in d2]
            call(N, obs.ptr, pred.ptr if pred is not None else None, dc.ptr, ds.ptr, [d.ptr if d is not None else None for d in dm])
            for h, d in zip([counts, sums] + d2, [dc, ds] + dm):
                if h is not None:
                    d.download(h)
    else:
        def chunk(b, dy, dp, dcounts, dsums, *dmaps):
            given = iter(dmaps)
            call(b, dy, dp, dcounts, dsums, [next(given) if m is not None else None for m in d2])
        paired_chunks(obs, pred, [counts, sums] + [m for m in d2 if m is not None], chunk, batch_size)
    return counts, sums, d2


def distance_transform(x, threshold, squared=True, batch_size=None, mask=None):
    """The exact Euclidean distance transform of every field of ``x`` (N, H, W, C) on the device: for every
    cell the squared distance, in grid cells, to the nearest event, a finite cell at or above ``threshold`` (one number, compared on
    float32).  ``x``: a host array of any dtype, read as float32 and uploaded in chunks of ``batch_size`` whole samples, or a float32
    DeviceArray, used where it lies.  ``mask`` (host arrays only; 0 = excluded) sets cells to NaN: they are no events, distances
    pass through them.  -> int32 (N, C, H, W), 2^31 - 1 everywhere on a field without an event; with ``squared=False`` the
    distances themselves as float64, inf on such a field."""
    x, shape = as_4d(x, 'x')
    if mask is not None and is_device(x):
        masked(x, mask)                                                   # (raises: a DeviceArray cannot take one)
    t = np.asarray(getattr(threshold, 'values', threshold))
    if t.size != 1:
        raise ValueError('`threshold` must be one number')
    thr, cutoff, alpha = check_distance_args(shape, t.reshape(()), None, PRATT_DEFAULT_ALPHA, batch_size)
    shape = check_4d_shape(shape)
    N, H, W, C = shape
    _, _, (d2, _) = _run(masked(x, mask), None, shape, thr, cutoff, alpha, batch_size, (True, False))
    d2 = d2.reshape(N, C, H, W)
    if squared:
        return d2
    return np.where(d2 == DIST_EMPTY, np.inf, np.sqrt(d2.astype(np.float64)))


def distance_scores(obs, pred, thresholds, cutoff=None, alpha=PRATT_DEFAULT_ALPHA, scaler=None, mask=None, batch_size=None,
                    return_maps=False):
    """Distance measures of a prediction against an observation, both (N, H, W, C), on the device.  Per
    field (each of the N*C planes) and threshold, A is the set of valid cells with obs >= threshold, B the same for the
    prediction; a cell is valid when both arrays are finite there and ``mask`` keeps it; d(x, S) is the Euclidean distance in
    grid cells from x to the nearest cell of S.  Host arrays of any dtype are prepared as in `neighbourhood_scores` (5-D squeezed,
    optional ``scaler.inverse_transform``, ``mask`` 2-D or with a channel axis, 0 = excluded), read as float32 and uploaded in
    chunks of ``batch_size`` whole samples; float32 DeviceArrays are used where they lie (no ``mask``, no ``scaler``: mark excluded
    cells with NaN).  ``cutoff`` (> 0, may be inf; None: the field diagonal, so that an empty side stays finite) caps the
    distances of Baddeley's Delta, ``alpha`` (default 1/9) scales Pratt's figure of merit.  -> the dict of `distance_from_sums`
    (``hausdorff``, ``med_obs_to_pred``, ``med_pred_to_obs``, ``rms_obs_to_pred``, ``rms_pred_to_obs``, ``baddeley1``,
    ``baddeley2``, ``baddeley_max``, ``pratt`` per (N, C, T) and as ``..._mean`` per threshold, ``n_obs``, ``n_pred``, ``n_both``,
    ``n_valid``), ``cutoff`` and ``alpha`` as used and, with ``return_maps``, ``d2_obs`` and ``d2_pred`` (N, C, T, H, W) int32: the
    squared distance maps of A and B (2^31 - 1 for an empty set).  The integers and the maps equal an integer reference; the fp64
    sums have one summation order, so the result has the same bits every call and for every ``batch_size``."""
    if is_device(obs) or is_device(pred):
        if not (is_device(obs) and is_device(pred)):
            raise ValueError('`obs` and `pred` must both be host arrays or both be DeviceArrays')
        obs, shape = as_4d(obs, 'obs')
        pred, pshape = as_4d(pred, 'pred')
        if tuple(shape) != tuple(pshape):
            raise ValueError(f'`obs` and `pred` must have one shape, got {tuple(shape)} and {tuple(pshape)}')
        if mask is not None:
            masked(obs, mask)                                             # (raises: a DeviceArray cannot take one)
        if scaler is not None:
            raise ValueError('`scaler` needs host arrays: transform a DeviceArray before it is scored')
        thr, cutoff, alpha = check_distance_args(shape, thresholds, cutoff, alpha, batch_size)
    else:
        from .metrics import _prepared
        obs, pred, (thr, cutoff, alpha) = _prepared(obs, pred, scaler, mask,
                                                    lambda s: check_distance_args(s, thresholds, cutoff, alpha, batch_size))
        shape = obs.shape
    shape = check_4d_shape(shape)
    N, H, W, C = shape
    counts, sums, d2 = _run(obs, None if pred is obs else pred, shape, thr, cutoff, alpha, batch_size, (bool(return_maps),) * 2)
    res = distance_from_sums(counts, sums, shape, thr)
    res.update(cutoff=cutoff, alpha=alpha)
    if return_maps:
        res.update(d2_obs=d2[0].reshape(N, C, len(thr), H, W), d2_pred=d2[1].reshape(N, C, len(thr), H, W))
    return res
