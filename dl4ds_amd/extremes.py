"""Extreme-value verification on the MI355X (csrc/extremes.hip): L-moments of block maxima or of declustered
peaks over a threshold, the GEV / Gumbel / GPD fits made from them and N-year return levels.

The reference has no counterpart: after ``climate_indices(...)['max']`` a user sorts every cell's series in numpy.  Here the device
produces the exact per-cell numbers -- the sorted probability-weighted moments b_0..b_3 of ``dl4ds_lmoments`` and the peaks of
``dl4ds_pot_peaks``, both defined in include/dl4ds_hip.h -- and the host turns them into fits and scores in float64 numpy
(`lmoments_from_pwm`, `gev_from_lmoments`, `gpd_from_lmoments`, `return_levels`: the ``*_from_sums`` of this module, usable without
a GPU).  A sample counts in a cell iff it is finite there (NaN is the mask).  ``tail='lower'`` works on -x throughout (minima, peaks
under a threshold) and gives the return levels back on the scale of x.  numpy in / numpy out; a ``dl4ds_amd.device.DeviceArray`` is
used where it lies.
"""
import math

import numpy as np

from ._chunks import as_4d as _as_4d, cell_bands, check_4d_shape, check_batch_size, is_int, masked as _masked, numeric_array
from .indices import check_index_args, climate_indices

__all__ = ['l_moments', 'block_maxima', 'peaks_over_threshold', 'lmoments_from_pwm', 'gev_from_lmoments', 'gumbel_from_lmoments',
           'gpd_from_lmoments', 'return_levels', 'fit_gev', 'fit_gumbel', 'fit_gpd', 'extreme_scores', 'check_extreme_args',
           'EXTREME_TAILS', 'EXTREME_METHODS', 'EXTREME_MAX_RUN']

EXTREME_TAILS = ('upper', 'lower')
EXTREME_METHODS = ('gev', 'gumbel', 'pot')
EXTREME_MAX_RUN = 32                                    # the cap of dl4ds_pot_peaks
EULER_GAMMA = 0.5772156649015329
LN2, LN3 = float(np.log(2.0)), float(np.log(3.0))
_gamma = np.vectorize(math.gamma, otypes=[np.float64])


def check_extreme_args(shape, tail='upper', run=1, return_periods=(5, 10, 20, 50), method='gev', threshold=None, batch_size=None):
    """Validation from the arguments alone (no library call).  ``shape``: the array's (N, H, W, C).
    -> (sign +1 / -1, threshold float32 (1,) or (H, W, C) or None, return periods float64 (R,))."""
    shape = check_4d_shape(shape)
    if tail not in EXTREME_TAILS:
        raise ValueError(f'`tail` must be one of {EXTREME_TAILS}, got {tail!r}')
    if not is_int(run) or not 1 <= run <= EXTREME_MAX_RUN:
        raise ValueError(f'`run` must be an integer between 1 and {EXTREME_MAX_RUN}, got {run!r}')
    if method not in EXTREME_METHODS:
        raise ValueError(f'`method` must be one of {EXTREME_METHODS}, got {method!r}')
    try:
        periods = np.atleast_1d(np.asarray(return_periods, np.float64))
    except (TypeError, ValueError):
        raise ValueError('`return_periods` must be numbers') from None
    if periods.ndim != 1 or periods.size < 1 or not (periods > 1.0).all():               # (a NaN fails the comparison)
        raise ValueError(f'`return_periods` must be numbers above 1 (blocks), got {return_periods!r}')
    check_batch_size(batch_size)
    if method == 'pot' and threshold is None:
        raise ValueError("method='pot' needs a `threshold`")
    thr = None
    if threshold is not None:
        thr = numeric_array(threshold, '`threshold` must be a number or a field of numbers')
        if thr.ndim == 4 and thr.shape[0] == 1:                                          # what percentile_threshold returns
            thr = thr[0]
        if thr.ndim == 2 and shape[3] == 1:
            thr = thr[..., None]
        if thr.ndim == 0:
            thr = thr.reshape(1)
        elif thr.shape != shape[1:]:
            raise ValueError(f'`threshold` must be a scalar or an (H, W, C) field on the grid {shape[1:]}, got shape {thr.shape}')
        thr = np.ascontiguousarray(thr, np.float32)
    return (1 if tail == 'upper' else -1), thr, periods


# ------------------------------------------------------------------------------------------------------------ device-backed
def l_moments(x, tail='upper', mask=None, batch_size=None):
    """Sample L-moments per grid cell over the samples of ``x`` (N, H, W, C), from the sorted probability-weighted moments of
    ``dl4ds_lmoments`` (of -x for ``tail='lower'``).  Host arrays are uploaded in bands of grid rows (``batch_size`` rows per band);
    the result does not depend on it.

    -> dict of ``n_valid`` int32 (H, W, C); ``pwm`` float64 (4, H, W, C) (b_r is NaN where n_valid <= r); ``l1``, ``l2``, ``t3``,
    ``t4`` float64 (H, W, C) as `lmoments_from_pwm` gives them."""
    from . import _lib
    x, shape = _as_4d(x)
    sign, _, _ = check_extreme_args(shape, tail, batch_size=batch_size)
    x = _masked(x, mask)
    lib = _lib.lib()
    N, H, W, C = shape
    per = H * W * C
    valid, pwm = np.empty((per,), np.int32), np.empty((4, per), np.float64)
    cell_bands(x, None, shape, (valid, pwm),
               lambda band: _lib.check(lib.dl4ds_lmoments(band.x, N, band.cells, band.cells, sign, *band.outs)), batch_size)
    out = {'n_valid': valid.reshape(H, W, C), 'pwm': pwm.reshape(4, H, W, C)}
    out.update(lmoments_from_pwm(out['pwm']))
    return out


def block_maxima(x, periods=None, period_starts=None, tail='upper', min_valid=1, mask=None, batch_size=None):
    """The largest (``tail='lower'``: the smallest) valid value per grid cell and period, `climate_indices`' ``max`` / ``min``;
    NaN where the period has fewer than ``min_valid`` valid samples.  ``periods`` / ``period_starts`` as there.
    -> float32 (P, H, W, C)."""
    _, shape = _as_4d(x)
    check_extreme_args(shape, tail, batch_size=batch_size)
    if not is_int(min_valid) or min_valid < 1:
        raise ValueError(f'`min_valid` must be a positive integer, got {min_valid!r}')
    r = climate_indices(x, periods, (0.0,), '>=', 1, mask, batch_size, period_starts)
    ext = r['max' if tail == 'upper' else 'min']
    return np.where(r['n_valid'] >= min_valid, ext, np.float32(np.nan)).astype(np.float32)


def peaks_over_threshold(x, threshold, run=1, tail='upper', periods=None, period_starts=None, mask=None, batch_size=None):
    """Declustered peaks over (``tail='lower'``: under) ``threshold`` per grid cell, ``dl4ds_pot_peaks``.  ``threshold`` is a scalar or
    an (H, W, C) field such as `percentile_threshold` gives (NaN: no threshold in that cell).  A cluster opens at an exceedance and
    closes after ``run`` consecutive valid non-exceedances, at an excluded sample, at a period boundary and at the end; its peak is
    its most extreme value.  A counting call sizes K to the largest number of clusters, so no peak is dropped.

    -> dict of ``n_peaks`` int32 (H, W, C) (-1 without a threshold); ``peaks`` float32 (K, H, W, C) in order of occurrence, NaN
    beyond a cell's count; ``positions`` int32 (K, H, W, C), their sample indices, -1 beyond the count; ``period_starts``."""
    from . import _lib
    x, shape = _as_4d(x)
    sign, thr, _ = check_extreme_args(shape, tail, run, method='pot', threshold=threshold, batch_size=batch_size)
    starts, _, _ = check_index_args(shape, periods, (0.0,), '>=', 1, batch_size, period_starts)
    x = _masked(x, mask)
    lib = _lib.lib()
    N, H, W, C = shape
    per, P, cell = H * W * C, len(starts) - 1, thr.ndim == 3
    count = np.empty((per,), np.int32)
    parts = []                                                          # (first cell, peaks (k, cells), positions (k, cells))

    def call(band):
        cells, c0 = band.cells, band.c0
        dc = band.buf.alloc((cells,), np.int32)
        args = (band.x, N, cells, starts.ctypes.data, P, band.fields[0], int(cell), sign, int(run))
        _lib.check(lib.dl4ds_pot_peaks(*args, 0, dc.ptr, None, None))
        n = count[c0:c0 + cells]
        dc.download(n)
        k = max(int(n.max()), 0)
        pk, ps = np.empty((k, cells), np.float32), np.empty((k, cells), np.int32)
        if k:
            dpk, dps = band.buf.alloc(pk.shape), band.buf.alloc(ps.shape, np.int32)
            _lib.check(lib.dl4ds_pot_peaks(*args, k, dc.ptr, dpk.ptr, dps.ptr))
            dpk.download(pk)
            dps.download(ps)
        parts.append((c0, pk, ps))
    cell_bands(x, None, shape, (), call, batch_size, fields=(thr,))
    K = max(pk.shape[0] for _, pk, _ in parts)
    peaks, pos = np.full((K, per), np.nan, np.float32), np.full((K, per), -1, np.int32)
    for c0, pk, ps in parts:
        peaks[:pk.shape[0], c0:c0 + pk.shape[1]] = pk
        pos[:ps.shape[0], c0:c0 + ps.shape[1]] = ps
    return {'n_peaks': count.reshape(H, W, C), 'peaks': peaks.reshape(K, H, W, C), 'positions': pos.reshape(K, H, W, C),
            'period_starts': starts}


# ---------------------------------------------------------------------------------------------------------------- host, fp64
def lmoments_from_pwm(pwm):
    """Hosking's b_0..b_3 (4, ...) -> dict of ``l1`` = b0, ``l2`` = 2 b1 - b0, ``t3`` = (6 b2 - 6 b1 + b0) / l2 and
    ``t4`` = (20 b3 - 30 b2 + 12 b1 - b0) / l2; t3 and t4 are NaN where l2 <= 0 (a constant sample) or a moment is missing."""
    b0, b1, b2, b3 = np.asarray(pwm, np.float64)
    l1, l2 = b0, 2.0 * b1 - b0
    l3, l4 = 6.0 * b2 - 6.0 * b1 + b0, 20.0 * b3 - 30.0 * b2 + 12.0 * b1 - b0
    with np.errstate(invalid='ignore', divide='ignore'):
        ok = l2 > 0
        safe = np.where(ok, l2, 1.0)
        t3, t4 = np.where(ok, l3 / safe, np.nan), np.where(ok, l4 / safe, np.nan)
    return {'l1': l1, 'l2': l2, 't3': t3, 't4': t4}


def _tau3_of_k(k):
    """(2 (1 - 3^-k) / (1 - 2^-k) - 3, its derivative) for k != 0"""
    a, b = -np.expm1(-k * LN3), -np.expm1(-k * LN2)                      # 1 - 3^-k, 1 - 2^-k
    g = 2.0 * a / b
    dg = 2.0 * ((1.0 - a) * LN3 * b - a * (1.0 - b) * LN2) / (b * b)
    return g - 3.0, dg


def gumbel_from_lmoments(l1, l2):
    """-> dict of ``location`` = l1 - gamma * scale and ``scale`` = l2 / ln 2 (``shape`` 0); NaN where l2 <= 0."""
    l1, l2 = np.asarray(l1, np.float64), np.asarray(l2, np.float64)
    with np.errstate(invalid='ignore'):
        scale = np.where(l2 > 0, l2 / LN2, np.nan)
    return {'kind': 'gumbel', 'location': l1 - EULER_GAMMA * scale, 'scale': scale, 'shape': np.zeros_like(scale) + 0.0 * scale}


def gev_from_lmoments(l1, l2, t3):
    """GEV by the method of L-moments (Hosking 1990): the start value k = 7.8590 c + 2.9554 c^2, c = 2 / (3 + t3) - ln 2 / ln 3, then
    Newton on 2 (1 - 3^-k) / (1 - 2^-k) - 3 = t3 (at most 30 steps, until |dk| < 1e-13; the Gumbel limit where |k| < 1e-8),
    scale = l2 k / ((1 - 2^-k) Gamma(1 + k)), location = l1 - scale (1 - Gamma(1 + k)) / k.

    -> dict of ``location``, ``scale``, ``shape`` and ``n_not_converged``.  ``shape`` is -k: POSITIVE MEANS A HEAVY (Frechet) TAIL,
    negative a bounded (Weibull) one, the sign of the climate literature and the opposite of Hosking's k and of scipy's ``c``.
    NaN where l2 <= 0, where a moment is missing, and where Newton did not converge (counted in ``n_not_converged``)."""
    l1, l2, t3 = np.broadcast_arrays(np.asarray(l1, np.float64), np.asarray(l2, np.float64), np.asarray(t3, np.float64))
    with np.errstate(invalid='ignore', divide='ignore', over='ignore'):
        ok = np.isfinite(l1) & np.isfinite(t3) & (l2 > 0) & (np.abs(t3) < 1)
        tau = np.where(ok, t3, 0.0)
        c = 2.0 / (3.0 + tau) - LN2 / LN3
        k = 7.8590 * c + 2.9554 * c * c
        done = ~ok
        for _ in range(30):
            small = np.abs(k) < 1e-8
            f, df = _tau3_of_k(np.where(small, 1.0, k))
            step = np.where(small | done, 0.0, (f - tau) / df)
            k = k - step
            done = done | small | (np.abs(step) < 1e-13)
            if done.all():
                break
        failed = ok & ~(done & np.isfinite(k))
        good = ok & ~failed
        small = np.abs(k) < 1e-8
        ks = np.where(good & ~small, k, 1.0)
        g = _gamma(1.0 + ks)
        scale = np.where(small, l2 / LN2, l2 * ks / (-np.expm1(-ks * LN2) * g))
        loc = np.where(small, l1 - EULER_GAMMA * scale, l1 - scale * (1.0 - g) / ks)
        nan = np.where(good, 0.0, np.nan)
    return {'kind': 'gev', 'location': loc + nan, 'scale': scale + nan, 'shape': -k + nan, 'n_not_converged': int(failed.sum())}


def gpd_from_lmoments(l1, l2):
    """Generalised Pareto of EXCESSES over a threshold by L-moments (Hosking & Wallis 1987): k = l1 / l2 - 2, scale = (1 + k) l1.
    -> dict of ``scale`` and ``shape`` = -k (positive: heavy tail); NaN where l2 <= 0."""
    l1, l2 = np.asarray(l1, np.float64), np.asarray(l2, np.float64)
    with np.errstate(invalid='ignore', divide='ignore'):
        ok = l2 > 0
        k = np.where(ok, l1 / np.where(ok, l2, 1.0) - 2.0, np.nan)
    return {'kind': 'gpd', 'scale': (1.0 + k) * l1, 'shape': -k}


def return_levels(fit, return_periods, rate=None):
    """Return levels of a fit for ``return_periods`` T > 1, in blocks (years).  GEV / Gumbel: the quantile at 1 - 1/T per block,
    location + scale (1 - (-ln(1 - 1/T))^k) / k, k = -shape (location - scale ln(-ln(1 - 1/T)) at k = 0).  GPD (a fit with
    ``threshold``): threshold + scale (1 - (rate T)^-k) / k, scale ln(rate T) at k = 0, ``rate`` = peaks per block (default: the
    fit's own).  A fit of the lower tail (``sign`` -1) describes -x; the levels come back on the scale of x.
    -> float64 (R,) + the fit's cell shape."""
    T = np.atleast_1d(np.asarray(return_periods, np.float64))
    if T.ndim != 1 or not (T > 1.0).all():
        raise ValueError(f'`return_periods` must be numbers above 1, got {return_periods!r}')
    scale, shape = np.asarray(fit['scale'], np.float64), np.asarray(fit['shape'], np.float64)
    k = -shape
    T = T.reshape((-1,) + (1,) * scale.ndim)
    with np.errstate(invalid='ignore', divide='ignore', over='ignore'):
        if fit.get('kind') == 'gpd' or 'threshold' in fit:
            rate = np.asarray(fit['rate'] if rate is None else rate, np.float64)
            base, y = np.asarray(fit['threshold'], np.float64), np.log(rate * T)         # 1 - (rate T)^-k = -expm1(-k y)
        else:
            base, y = np.asarray(fit['location'], np.float64), -np.log(-np.log1p(-1.0 / T))   # 1 - (-ln p)^k = -expm1(-k y)
        zero = k == 0
        ks = np.where(zero, 1.0, k)
        level = base + scale * np.where(zero, y, -np.expm1(-ks * y) / ks)
    return float(fit.get('sign', 1)) * level


def fit_gev(sample, tail='upper', mask=None, batch_size=None):
    """GEV per grid cell of ``sample`` (N, H, W, C), block maxima say: `l_moments` then `gev_from_lmoments`.
    -> the fit (``location``, ``scale``, ``shape``, ``n_not_converged``) with ``n_valid``, ``sign`` and the L-moments ``l1``, ``l2``,
    ``t3``, ``t4``.  With ``tail='lower'`` the fit describes -sample (``sign`` -1); `return_levels` undoes it."""
    m = l_moments(sample, tail, mask, batch_size)
    fit = gev_from_lmoments(m['l1'], m['l2'], m['t3'])
    fit.update(n_valid=m['n_valid'], sign=1 if tail == 'upper' else -1, l1=m['l1'], l2=m['l2'], t3=m['t3'], t4=m['t4'])
    return fit


def fit_gumbel(sample, tail='upper', mask=None, batch_size=None):
    """Gumbel per grid cell of ``sample``: `l_moments` then `gumbel_from_lmoments`; the other entries as in `fit_gev`."""
    m = l_moments(sample, tail, mask, batch_size)
    fit = gumbel_from_lmoments(m['l1'], m['l2'])
    fit.update(n_valid=m['n_valid'], sign=1 if tail == 'upper' else -1, l1=m['l1'], l2=m['l2'], t3=m['t3'], t4=m['t4'])
    return fit


def gpd_fit_from_pwm(pwm, n_peaks, threshold, n_blocks, sign=1):
    """The GPD fit from the PWMs of the PEAKS (of sign * x): those of the excesses are b_r - u / (r + 1), u = sign * threshold."""
    pwm = np.asarray(pwm, np.float64)
    u = float(sign) * np.broadcast_to(np.asarray(threshold, np.float64), pwm.shape[1:])
    e0, e1 = pwm[0] - u, pwm[1] - u / 2.0
    fit = gpd_from_lmoments(e0, 2.0 * e1 - e0)
    n = np.asarray(n_peaks)
    fit.update(threshold=u, rate=np.where(n >= 0, n, 0) / float(n_blocks), n_valid=n, sign=int(sign))
    return fit


def fit_gpd(peaks, threshold, n_blocks, tail='upper', mask=None, batch_size=None):
    """GPD per grid cell from the ``peaks`` (K, H, W, C) of `peaks_over_threshold` (NaN beyond a cell's count) over ``threshold``
    (scalar or (H, W, C)) in a record of ``n_blocks`` blocks (years): `l_moments` of the peaks, `gpd_from_lmoments` of their excesses.
    -> ``scale``, ``shape``, ``threshold`` (of sign * x), ``rate`` (peaks per block), ``n_valid``, ``sign``."""
    if not n_blocks > 0:
        raise ValueError(f'`n_blocks` must be positive, got {n_blocks!r}')
    _, shape = _as_4d(peaks)
    sign, thr, _ = check_extreme_args(shape, tail, method='pot', threshold=threshold, batch_size=batch_size)
    m = l_moments(peaks, tail, mask, batch_size)
    return gpd_fit_from_pwm(m['pwm'], m['n_valid'], thr if thr.ndim == 3 else thr.reshape(()), n_blocks, sign)


def extreme_scores(obs, pred, periods=None, return_periods=(5, 10, 20, 50), method='gev', threshold=None, run=1, tail='upper',
                   mask=None, period_starts=None, batch_size=None):
    """Return levels of an observation and of a prediction side by side.  ``method``: 'gev' / 'gumbel' fit the block extremes of the
    ``periods`` (`block_maxima`), 'pot' the declustered peaks over ``threshold`` (`peaks_over_threshold`, one block per period).

    -> dict of ``obs`` and ``pred`` (each ``{'fit', 'return_levels' (R, H, W, C), 'n_valid'}``), ``bias`` = pred - obs of the return
    levels, ``relative_bias`` = bias / |obs level| (NaN where that is 0), ``shape_difference`` = pred shape - obs shape (zero for
    'gumbel') and ``return_periods``."""
    _, shape = _as_4d(obs)
    _, pshape = _as_4d(pred)
    if shape != pshape:
        raise ValueError(f'`obs` {shape} and `pred` {pshape} must have the same shape')
    _, _, T = check_extreme_args(shape, tail, run, return_periods, method, threshold, batch_size)
    starts = check_index_args(shape, periods, (0.0,), '>=', 1, batch_size, period_starts)[0]

    def side(x):
        if method == 'pot':
            r = peaks_over_threshold(x, threshold, run, tail, None, starts, mask, batch_size)
            if r['peaks'].shape[0] == 0:
                r['peaks'] = np.full((1,) + shape[1:], np.nan, np.float32)
            fit = fit_gpd(r['peaks'], threshold, len(starts) - 1, tail, None, batch_size)
            fit['n_valid'] = r['n_peaks']
        else:
            bm = block_maxima(x, None, starts, tail, 1, mask, batch_size)
            fit = (fit_gev if method == 'gev' else fit_gumbel)(bm, tail, None, batch_size)
        return {'fit': fit, 'return_levels': return_levels(fit, T), 'n_valid': fit['n_valid']}
    o, p = side(obs), side(pred)
    bias = p['return_levels'] - o['return_levels']
    with np.errstate(invalid='ignore', divide='ignore'):
        mag = np.abs(o['return_levels'])
        rel = np.where(mag > 0, bias / np.where(mag > 0, mag, 1.0), np.nan)
    return {'obs': o, 'pred': p, 'bias': bias, 'relative_bias': rel,
            'shape_difference': np.asarray(p['fit']['shape']) - np.asarray(o['fit']['shape']), 'return_periods': T}
