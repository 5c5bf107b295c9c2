"""Object-based (feature-based) verification, host side (no counterpart in the reference): a field is cut
into the connected objects of its cells at or above a threshold, and the objects' number, size, shape, mass and position are
compared.  This module holds what follows from a labelling's per-object sums: `object_attributes` (area, centroid, mass, maximum,
bounding box, orientation, aspect), `sal_from_objects` (Structure, Amplitude, Location of Wernli et al. 2008),
`object_scores_from_objects` (attribute summary), SAL's `factor_thresholds` and the argument rules `check_object_args`.  The
labelling itself runs on the device (`dl4ds_label_objects`, csrc/objects.hip; tests/objects_ref.py is its sequential restatement):
`label_objects`, and on top of it `sal_scores` and `object_scores` for an observation and a prediction.  Matching of observed and
predicted objects is not done here."""
import ctypes

import numpy as np

from . import _exact
from ._chunks import as_4d, check_4d_shape, check_batch_size, is_device, is_int, masked, paired_chunks

OBJECTS_DEFAULT_CAP = 4096
OBJECTS_CELL_BOUND = (1 << 31) - 1                 # H*W must stay below it (int32 cell indices, -1 is background)
OBJECTS_SIDE_BOUND = 1 << 29                       # max(H, W) must stay below it (v*i is exact in fp64)
OBJECTS_SUM_BOUND = 1 << 62                        # H*W*max(H, W)^2 must stay below it (exact 64-bit second moments)
SAL_DEFAULT_FACTOR = 1.0 / 15.0


def check_object_args(shape, threshold, connectivity, cap, batch_size):
    """The argument rules of a labelling request (no library call) -> (thresholds as float32 (N*C,), or None when ``threshold`` is None;
    ``cap`` as int, None -> 4096)."""
    n, h, w, c = check_4d_shape(shape)
    if h * w >= OBJECTS_CELL_BOUND:
        raise ValueError(f'fields of H*W = {h * w} cells are not supported: H*W must stay below 2^31 - 1')
    if max(h, w) >= OBJECTS_SIDE_BOUND:
        raise ValueError(f'max(H, W) = {max(h, w)} must stay below 2^29')
    if h * w * max(h, w) ** 2 >= OBJECTS_SUM_BOUND:
        raise ValueError(f'H*W*max(H, W)^2 = {h * w * max(h, w) ** 2} must stay below 2^62 for the exact 64-bit sums')
    if not is_int(connectivity) or connectivity not in (1, 2):
        raise ValueError(f'`connectivity` must be 1 (4 neighbours) or 2 (8 neighbours), got {connectivity!r}')
    if cap is None:
        cap = OBJECTS_DEFAULT_CAP
    if not is_int(cap) or cap < 0 or cap >= 1 << 31:
        raise ValueError(f'`cap` must be a non-negative integer, got {cap!r}')
    check_batch_size(batch_size)
    thr = None
    if threshold is not None:
        t = np.asarray(getattr(threshold, 'values', threshold))
        if t.dtype == object or t.dtype == bool or not (np.issubdtype(t.dtype, np.floating) or np.issubdtype(t.dtype, np.integer)):
            raise ValueError('`threshold` must be a number or one number per field')
        if t.size == 1:                                                  # a scalar in any wrapping, broadcast to the fields
            t = np.broadcast_to(t.reshape(()), (n * c,))
        elif t.size != n * c or (t.ndim > 1 and t.shape != (n, c)):
            raise ValueError(f'`threshold` must be a scalar or hold one value per field (N*C = {n * c}), got shape {t.shape}')
        thr = _exact.finite_float32(t.reshape(-1), '`threshold`')
    return thr, int(cap)


def _check_factor(factor):
    if isinstance(factor, (bool, np.bool_)) or not isinstance(factor, (int, float, np.integer, np.floating)) \
            or not np.isfinite(factor) or factor <= 0:
        raise ValueError(f'`factor` must be a positive finite number, got {factor!r}')
    return float(factor)


def factor_thresholds(x, factor):
    """SAL's thresholds: per field of the host array ``x`` (N, H, W, C) ``factor`` times the largest finite float32 value, as
    float32 (N*C,); 0 for a field without a finite cell."""
    factor = _check_factor(factor)
    x = np.asarray(x)
    n, h, w, c = x.shape
    thr = np.zeros((n, c), np.float32)
    for i in range(n):                                                   # (sample by sample: no float32 copy of the whole array)
        with np.errstate(over='ignore'):
            f = np.asarray(x[i], np.float32).reshape(h * w, c)
        m = np.where(np.isfinite(f), f, -np.inf).max(axis=0).astype(np.float64)
        with np.errstate(over='ignore', invalid='ignore'):
            t = (factor * m).astype(np.float32)
        thr[i] = np.where(np.isfinite(m) & np.isfinite(t), t, np.float32(0))
    return thr.reshape(-1)


def object_attributes(raw, shape, thr, connectivity):
    """Per-object attributes from the sums of a labelling of the N*C fields of an (N, H, W, C) = ``shape`` array, fields on the
    leading axis (f = n*C + c), tables of at least max(count) rows (the layout of tests/objects_ref.py and DESIGN.md section 27):
    ``count`` (F,), ``nvalid`` (F,), ``field_sums`` (F, 3) = sum v, sum v*i, sum v*j over the valid cells, ``sums`` (F, K, 6) int64
    = area, sum i, sum j, sum i*i, sum j*j, sum i*j, ``bbox`` (F, K, 4), ``first`` (F, K), ``vmax`` (F, K) float32, ``mass``
    (F, K, 3) fp64 = sum v, sum v*i, sum v*j over the object's cells, optionally ``labels`` (F, H, W).  Returns a dict of arrays
    shaped (N, C, ...), K = the largest count, NaN (0 for the integers) beyond a field's count: ``count``, ``nvalid``,
    ``field_sums``, ``thresholds``, ``area`` int64, ``centroid`` (.., 2) = (i, j) from the integer sums, ``mass``,
    ``mass_centroid`` (.., 2), ``vmax``, ``bbox``, ``first``, ``orientation`` and ``aspect`` (`orientation_aspect` of the integer
    second moments), the sums themselves under ``raw``, and ``labels`` (N, C, H, W) when given."""
    N, H, W, C = shape
    count = raw['count'].reshape(N, C)
    K = int(count.max()) if count.size else 0
    cut = lambda a: a[:, :K].reshape((N, C, K) + a.shape[2:])
    sums, mass, vmax = cut(raw['sums']), cut(raw['mass']), cut(raw['vmax'])
    there = np.arange(K)[None, None, :] < count[..., None]
    nan = lambda a: np.where(there if a.ndim == 3 else there[..., None], a, np.nan)
    area = sums[..., 0]
    A = np.where(there, area, 1).astype(np.float64)
    centroid = nan(np.stack([sums[..., 1] / A, sums[..., 2] / A], -1))
    with np.errstate(divide='ignore', invalid='ignore'):
        mc = nan(np.stack([mass[..., 1] / mass[..., 0], mass[..., 2] / mass[..., 0]], -1))
    # central second moments from the integers, (A * sum ii - (sum i)^2) / A^2: numerator and denominator as Python integers (they
    # pass 2^64), each quotient correctly rounded; NaN beyond a field's count (A = 0 there)
    so = np.where(there[..., None], sums, 0).astype(object)
    a2 = so[..., 0] * so[..., 0]
    cii = _exact.ratio_exact(so[..., 0] * so[..., 3] - so[..., 1] * so[..., 1], a2)
    cjj = _exact.ratio_exact(so[..., 0] * so[..., 4] - so[..., 2] * so[..., 2], a2)
    cij = _exact.ratio_exact(so[..., 0] * so[..., 5] - so[..., 1] * so[..., 2], a2)
    orientation, aspect = orientation_aspect(cii, cjj, cij)
    res = dict(count=count, nvalid=raw['nvalid'].reshape(N, C), field_sums=raw['field_sums'].reshape(N, C, 3),
               thresholds=np.asarray(thr, np.float32).reshape(N, C), connectivity=int(connectivity),
               area=area, centroid=centroid, mass=nan(mass[..., 0]), mass_centroid=mc, vmax=nan(vmax.astype(np.float64)),
               bbox=cut(raw['bbox']), first=cut(raw['first']), orientation=nan(orientation), aspect=nan(aspect),
               raw=dict(sums=sums, mass=mass, vmax=vmax))
    if 'labels' in raw:
        res['labels'] = raw['labels'].reshape(N, C, H, W)
    return res


def orientation_aspect(cii, cjj, cij):
    """Closed-form eigen-decomposition of the 2 x 2 covariance [[cjj, cij], [cij, cii]] of an object's cells in (j, i) = (x, y):
    -> (angle of the major axis from the +j axis towards +i, in (-pi/2, pi/2]; sqrt(minor / major eigenvalue) in [0, 1], NaN for
    an object without extent along its major axis)."""
    half, dev = (cii + cjj) / 2.0, np.hypot((cjj - cii) / 2.0, cij)
    major, minor = half + dev, np.maximum(half - dev, 0.0)
    with np.errstate(divide='ignore', invalid='ignore'):
        aspect = np.where(major > 0, np.sqrt(minor / np.where(major > 0, major, 1.0)), np.nan)
    return 0.5 * np.arctan2(2.0 * cij, cjj - cii), aspect


def _mean(a):
    a = np.asarray(a, np.float64)
    ok = ~np.isnan(a)
    return float(a[ok].mean()) if ok.any() else float('nan')


def sal_from_objects(obs_objs, pred_objs, hw):
    """SAL (Wernli et al. 2008) per field pair from two `object_attributes` results on (H, W) = ``hw`` fields (host arithmetic only).
    With D the domain mean over the valid cells, R_n the mass of object n, x_n its mass centroid, x the centre of mass of the
    whole field and d = sqrt((H-1)^2 + (W-1)^2):

        A = (D_p - D_o) / (0.5 (D_p + D_o))
        S = (V_p - V_o) / (0.5 (V_p + V_o)),   V = sum_n R_n (R_n / vmax_n) / sum_n R_n
        L = L1 + L2,   L1 = |x_p - x_o| / d,   L2 = 2 |r_p - r_o| / d,   r = sum_n R_n |x - x_n| / sum_n R_n

    -> dict of (N, C) arrays S, A, L, L1, L2: NaN where a side has no object or a denominator (a field sum, a
    mass total, D_p + D_o, V_p + V_o) is zero; and
    their means over the fields that are not NaN as ``S_mean`` ... (NaN when there is none)."""
    H, W = hw
    d = float(np.hypot(H - 1, W - 1))

    def side(o):
        count = np.asarray(o['count'])
        fs = np.asarray(o['field_sums'], np.float64)
        D = _exact.ratio(fs[..., 0], np.asarray(o['nvalid']))
        com = np.stack([_exact.ratio(fs[..., 1], fs[..., 0]), _exact.ratio(fs[..., 2], fs[..., 0])], -1)    # NaN on a zero field sum
        R = np.asarray(o['mass'], np.float64)
        vmax = np.asarray(o['vmax'], np.float64)
        there = (np.arange(R.shape[-1])[None, None, :] < count[..., None]) & (R != 0)      # a massless object has no weight
        tot = np.where(there, R, 0.0).sum(-1)
        with np.errstate(divide='ignore', invalid='ignore', over='ignore'):
            V = _exact.ratio(np.where(there, R * (R / np.where(there, vmax, 1.0)), 0.0).sum(-1), tot)
            dist = np.sqrt(((np.asarray(o['mass_centroid'], np.float64) - com[..., None, :]) ** 2).sum(-1))
            r = _exact.ratio(np.where(there, R * dist, 0.0).sum(-1), tot)                    # NaN on a zero mass total
        none = count == 0
        return D, np.where(none, np.nan, V), np.where(none[..., None], np.nan, com), np.where(none, np.nan, r)

    Do, Vo, xo, ro = side(obs_objs)
    Dp, Vp, xp, rp = side(pred_objs)
    with np.errstate(divide='ignore', invalid='ignore'):
        A = np.where(Dp + Do == 0, np.nan, (Dp - Do) / (0.5 * (Dp + Do)))
        S = np.where(Vp + Vo == 0, np.nan, (Vp - Vo) / (0.5 * (Vp + Vo)))
        if d > 0:
            L1 = np.sqrt(((xp - xo) ** 2).sum(-1)) / d
            L2 = 2.0 * np.abs(rp - ro) / d
        else:
            L1 = L2 = np.full(A.shape, np.nan)
    either = np.isnan(Vo) | np.isnan(Vp)
    A = np.where(either, np.nan, A)
    res = dict(S=S, A=A, L=L1 + L2, L1=L1, L2=L2)
    res = {k: np.where(np.isfinite(v), v, np.nan) for k, v in res.items()}              # (a zero vmax, an overflow: NaN as well)
    res.update({k + '_mean': _mean(v) for k, v in list(res.items())})
    return res


def _area_summary(o, sfx):
    count, area = o['count'], o['area']
    total = area.sum(-1)
    return {'n_objects' + sfx: count, 'event_area' + sfx: total, 'mean_area' + sfx: _exact.ratio(total, count),
            'max_area' + sfx: area.max(-1) if area.shape[-1] else np.zeros(count.shape, np.int64)}


def object_scores_from_objects(obs_objs, pred_objs, hw):
    """Attribute summary of two `object_attributes` results on (H, W) = ``hw`` fields: ``count_ratio`` (N, C) = predicted /
    observed number of objects, ``largest_area_ratio``, ``mean_vmax_ratio`` (NaN on a zero denominator), ``area_bins`` (B + 1,)
    = 1, 2, 4, ... and ``area_hist_obs`` / ``area_hist_pred`` (B,) int64: objects of all fields with 2^b <= area < 2^(b+1), and
    per side (``_obs`` / ``_pred``) ``n_objects``, ``mean_area``, ``max_area`` and ``event_area`` (N, C)."""
    H, W = hw
    o, p = obs_objs, pred_objs
    res = {}
    res.update(_area_summary(o, '_obs'))
    res.update(_area_summary(p, '_pred'))
    B = max(int(H * W).bit_length(), 1)
    res['area_bins'] = 1 << np.arange(B + 1, dtype=np.int64)
    for sfx, s in (('_obs', o), ('_pred', p)):
        a = s['area'][s['area'] > 0]
        res['area_hist' + sfx] = np.bincount(np.floor(np.log2(a)).astype(np.int64), minlength=B)[:B].astype(np.int64) \
            if a.size else np.zeros(B, np.int64)
    res['count_ratio'] = _exact.ratio(p['count'], o['count'])
    res['largest_area_ratio'] = _exact.ratio(res['max_area_pred'], res['max_area_obs'])
    with np.errstate(invalid='ignore'):
        mv = lambda s: np.where(s['count'] > 0, np.nansum(s['vmax'], -1) / np.maximum(s['count'], 1), np.nan)
        vo, vp = mv(o), mv(p)
        res['mean_vmax_ratio'] = np.where(vo == 0, np.nan, vp / np.where(vo == 0, 1.0, vo))
    return res


def _raw_tables(F, cap, hw, labels):
    """host arrays of a labelling's outputs in the order of the library call, `labels` first (None when not wanted)"""
    H, W = hw
    return [np.zeros((F, H, W), np.int32) if labels else None, np.zeros(F, np.int32), np.zeros(F, np.int64), np.zeros((F, 3)),
            np.zeros((F, cap, 6), np.int64), np.zeros((F, cap, 4), np.int32), np.zeros((F, cap), np.int32),
            np.zeros((F, cap), np.float32), np.zeros((F, cap, 3))]


def _label(x, shape, thr, factor, connectivity, cap, batch_size, labels):
    """The library calls of one labelling: ``x`` a float32 DeviceArray, used where it lies, or a host array, which goes up in
    chunks of whole samples.  ``thr``: float32 (N*C,), or None for ``factor`` times each field's largest finite value, taken on the
    device.  -> (the outputs under `object_attributes`' names, the thresholds)."""
    from . import _lib
    from .device import Buffers, sync
    N, H, W, C = shape
    F = N * C
    lib = _lib.lib()
    host = _raw_tables(F, cap, (H, W), labels)
    thr_out = np.zeros(F, np.float32)
    if thr is not None:
        thr = np.ascontiguousarray(thr, np.float32)

    def call(b, dx, dthr, outs):
        if thr is None:
            _lib.check(lib.dl4ds_object_thresholds(dx, b, H, W, C, ctypes.c_double(factor), dthr))
        _lib.check(lib.dl4ds_label_objects(dx, b, H, W, C, dthr, connectivity, cap, *outs))
        sync()                                                             # (reports a device-side error of the call)

    if is_device(x):
        with Buffers() as buf:
            dthr = buf.alloc((F,))
            if thr is not None:
                dthr.upload(thr)
            devs = [buf.alloc(h.shape, h.dtype) if h is not None else None for h in host]
            call(N, x.ptr, dthr.ptr, [d.ptr if d is not None else None for d in devs])
            for h, d in zip(host + [thr_out], devs + [dthr]):
                if h is not None and h.nbytes:
                    d.download(h)
    else:
        done = [0]                                                         # samples labelled so far: chunks run in ascending order
        outputs = [thr_out] + [h for h in host if h is not None]

        def chunk(b, dx, _, dthr, *outs):
            if thr is not None:
                _lib.check(lib.dl4ds_memcpy_h2d(dthr, thr[done[0] * C:(done[0] + b) * C].ctypes.data, 4 * b * C))
            call(b, dx, dthr, ([] if labels else [None]) + list(outs))
            done[0] += b
        paired_chunks(x, None, outputs, chunk, batch_size)
    names = ('labels', 'count', 'nvalid', 'field_sums', 'sums', 'bbox', 'first', 'vmax', 'mass')
    return {k: h for k, h in zip(names, host) if h is not None}, thr_out


def _checked(x, name, threshold, factor, connectivity, cap, batch_size, mask):
    """every refusal of a labelling request, without a library call -> (x as it goes to `_label`, shape, thr or None, factor, cap)"""
    x, shape = as_4d(x, name)
    if mask is not None and is_device(x):
        masked(x, mask)                                                   # (raises: a DeviceArray cannot take one)
    if (threshold is None) == (factor is None):
        raise ValueError('exactly one of `threshold` and `factor` must be given')
    thr, cap = check_object_args(shape, threshold, connectivity, cap, batch_size)
    if factor is not None:
        factor = _check_factor(factor)
    return masked(x, mask), check_4d_shape(shape), thr, factor, cap


def _attributes(raw, shape, thr, connectivity, cap):
    """`object_attributes` of tables of ``cap`` rows: objects beyond ``cap`` are left out, ``count`` stays true, ``truncated`` says
    whether any field had more"""
    count = raw['count']
    res = object_attributes(dict(raw, count=np.minimum(count, cap)), shape, thr, connectivity)
    res['count'] = count.reshape(shape[0], shape[3])
    res['truncated'] = bool((count > cap).any())
    return res


def label_objects(x, threshold=None, factor=None, connectivity=1, cap=None, batch_size=None, mask=None, return_labels=True):
    """Labels the objects of every field of ``x`` (N, H, W, C) on the device: the connected sets (``connectivity``
    1: 4 neighbours, 2: 8) of finite cells at or above ``threshold`` (a scalar or one value per field) or, with ``factor``, above
    ``factor`` times the field's largest finite value.  ``x``: a host array of any dtype, read as float32 and uploaded in chunks of
    ``batch_size`` whole samples, or a float32 DeviceArray, used where it lies.  ``mask`` (host arrays only; 0 = excluded) sets
    cells to NaN.  ``cap``: rows of the per-object tables (default 4096); objects beyond it are left out of the attributes and keep
    their labels.  -> the dict of `object_attributes`, with ``labels`` (N, C, H, W) unless ``return_labels`` is False, ``count``
    true also beyond ``cap`` and ``truncated`` = whether any field's count exceeds ``cap``."""
    x, shape, thr, factor, cap = _checked(x, 'x', threshold, factor, connectivity, cap, batch_size, mask)
    raw, thr = _label(x, shape, thr, factor, int(connectivity), cap, batch_size, bool(return_labels))
    return _attributes(raw, shape, thr, int(connectivity), cap)


def _both_sides(obs, pred, threshold, factor, connectivity, cap, batch_size, mask):
    obs, shape = as_4d(obs, 'obs')
    pred, pshape = as_4d(pred, 'pred')
    if tuple(shape) != tuple(pshape):
        raise ValueError(f'`obs` and `pred` must have one shape, got {tuple(shape)} and {tuple(pshape)}')
    sides = [_checked(a, name, threshold, factor, connectivity, cap, batch_size, mask) for a, name in ((obs, 'obs'), (pred, 'pred'))]
    out = []
    for a, shape, thr, factor, cap in sides:                               # (both sides checked before the first library call)
        raw, thr = _label(a, shape, thr, factor, int(connectivity), cap, batch_size, False)
        out.append(_attributes(raw, shape, thr, int(connectivity), cap))
    return out[0], out[1], shape


def sal_scores(obs, pred, threshold=None, factor=SAL_DEFAULT_FACTOR, connectivity=1, cap=None, batch_size=None, mask=None):
    """SAL (`sal_from_objects`) of a prediction against an observation, both (N, H, W, C), host arrays or float32 DeviceArrays,
    labelled on the device as by `label_objects` (labels are not downloaded).  With ``factor`` (the default, 1/15: Wernli et al.
    2008) each side gets its own thresholds, ``factor`` times each field's largest finite value; pass ``threshold`` and
    ``factor=None`` for fixed ones.  ``mask`` applies to both sides.  Also in the result: ``n_objects_obs`` / ``n_objects_pred``
    (N, C), ``thresholds_obs`` / ``thresholds_pred`` (N, C) and ``truncated`` (a side had more than ``cap`` objects in a field)."""
    if threshold is not None and factor == SAL_DEFAULT_FACTOR:
        factor = None                                                      # (a threshold replaces the default factor)
    o, p, shape = _both_sides(obs, pred, threshold, factor, connectivity, cap, batch_size, mask)
    res = sal_from_objects(o, p, shape[1:3])
    res.update(n_objects_obs=o['count'], n_objects_pred=p['count'], thresholds_obs=o['thresholds'], thresholds_pred=p['thresholds'],
               truncated=o['truncated'] or p['truncated'])
    return res


def object_scores(obs, pred, threshold, connectivity=1, cap=None, batch_size=None, mask=None):
    """The attribute summary (`object_scores_from_objects`) of a prediction against an observation at one ``threshold`` (a scalar
    or one value per field) for both sides, labelled on the device as by `label_objects`; ``truncated`` as in `sal_scores`."""
    o, p, shape = _both_sides(obs, pred, threshold, None, connectivity, cap, batch_size, mask)
    res = object_scores_from_objects(o, p, shape[1:3])
    res['truncated'] = o['truncated'] or p['truncated']
    return res
