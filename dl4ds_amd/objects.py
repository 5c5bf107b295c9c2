"""Object-based (feature-based) verification, host side (no counterpart in the reference): a field is cut
into the connected objects of its cells at or above a threshold, and the objects' number, size, shape, mass and position are
compared.  This module holds what follows from a labelling's per-object sums: `object_attributes` (area, centroid, mass, maximum,
bounding box, orientation, aspect), `sal_from_objects` (Structure, Amplitude, Location of Wernli et al. 2008),
`object_scores_from_objects` (attribute summary), SAL's `factor_thresholds` and the argument rules `check_object_args`.  The
labelling itself is not in the library yet: tests/objects_ref.py is its sequential restatement.  Matching of observed and
predicted objects is not done here."""
import numpy as np

from . import _exact
from ._chunks import check_4d_shape, check_batch_size, is_int

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
