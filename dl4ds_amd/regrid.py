"""Regridding between rectilinear latitude / longitude grids on the device, and the consistency of a downscaled field with its
coarse input (no counterpart in the reference, whose one route between the grids is the index-space resize of `create_pair_hr_lr`;
DESIGN.md section 30).  On a rectilinear grid conservative, bilinear and nearest-neighbour regridding factorise into one table per
axis (`axis_table`: host arithmetic in fp64, no library call); the device applies both tables in one pass (`dl4ds_regrid_apply`,
csrc/regrid.hip; tests/regrid_ref.py is its restatement).  `Regridder` holds the tables of a pair of grids, `regrid` is the one-call
form, `consistency_scores` regrids a prediction onto the grid of its coarse input and scores the difference on the device
(`dl4ds_regrid_consistency`), `consistency_from_sums` is the host arithmetic on the device's sums and `check_regrid_args` the
argument rules."""
import math
import sys
import types
from collections import namedtuple

import numpy as np

from ._chunks import as_4d, check_4d_shape, check_batch_size, is_device, masked, paired_chunks, upload_batch

METHODS = ('conservative', 'bilinear', 'nearest')
GEOMETRIES = ('spherical', 'planar')
EXTRAPOLATE = ('nearest', 'nan')
CELL_BOUND = 1 << 31                                # H*W and H'*W' must stay below it
PERIOD_TOLERANCE = 1e-9
SUM_NAMES = ('sum_area', 'sum_area_d', 'sum_area_d2', 'sum_area_ref', 'sum_area_regridded', 'max_abs')
COUNT_NAMES = ('n_valid', 'n_mismatch')

AxisTable = namedtuple('AxisTable', 'ptr idx w dst_measure src_measure coverage')
AxisTable.__doc__ = """The taps of one axis, CSR: destination d reads the sources ``idx[ptr[d]:ptr[d + 1]]`` with the weights ``w``
(fp64, > 0); ``dst_measure`` / ``src_measure``: the measure of every destination / source cell (its width; with spherical latitudes
the difference of the sines of its bounds); ``coverage``: per destination the share of its measure that its taps cover (the sum of
the weights for the point methods)."""


def _coords(v, name, count=None):
    a = np.asarray(getattr(v, 'values', v))
    if a.dtype == object or a.dtype == bool or not (np.issubdtype(a.dtype, np.floating) or np.issubdtype(a.dtype, np.integer)):
        raise ValueError(f'`{name}` must be a 1-D sequence of numbers')
    a = a.astype(np.float64)
    if a.ndim != 1 or a.size < 1:
        raise ValueError(f'`{name}` must be a 1-D sequence of at least 1 value, got shape {a.shape}')
    if count is not None and a.size != count:
        raise ValueError(f'`{name}` must hold {count} values (one more than the cells), got {a.size}')
    if not np.isfinite(a).all():
        raise ValueError(f'`{name}` must be finite')
    d = np.diff(a)
    if a.size > 1 and not ((d > 0).all() or (d < 0).all()):
        raise ValueError(f'`{name}` must be strictly increasing or strictly decreasing')
    return a


def cell_bounds(centres, bounds=None, name='centres', spherical=False):
    """The n + 1 bounds of n cells: ``bounds`` where given, else the midpoints of the centres, the two end bounds continuing the end
    spacing by half a step.  ``spherical`` (latitudes in degrees): nothing may lie beyond +-90 as given, and the bounds derived from
    centres are clipped to +-90."""
    c = _coords(centres, name)
    if spherical and (np.abs(c) > 90).any():
        raise ValueError(f'`{name}`: latitudes beyond +-90 degrees with spherical geometry')
    if bounds is not None:
        b = _coords(bounds, name + '_bounds', c.size + 1)
        if spherical and (np.abs(b) > 90).any():
            raise ValueError(f'`{name}_bounds`: latitudes beyond +-90 degrees with spherical geometry')
        return c, b
    if c.size < 2:
        return c, None                               # (one cell without bounds: only the point methods can use it)
    b = np.empty(c.size + 1)
    b[1:-1] = (c[:-1] + c[1:]) / 2
    b[0] = c[0] - (c[1] - c[0]) / 2
    b[-1] = c[-1] + (c[-1] - c[-2]) / 2
    if spherical:
        b = np.clip(b, -90.0, 90.0)
    return c, b


def _g(b, spherical):
    """the measure coordinate of the bounds: sin(phi * pi / 180) for spherical latitudes, the bound itself otherwise"""
    if not spherical:
        return b.copy()
    return np.array([math.sin(float(v) * math.pi / 180.0) for v in b])


def _cells(b, spherical):
    """-> (lower, upper) measure coordinate of every cell"""
    g = _g(b, spherical)
    return np.minimum(g[:-1], g[1:]), np.maximum(g[:-1], g[1:])


def _overlap(lo_s, hi_s, lo_d, hi_d):
    return np.maximum(0.0, np.minimum(hi_s, hi_d) - np.maximum(lo_s, lo_d))


def _conservative(sb, db, spherical, periodic, period):
    slo, shi = _cells(sb, spherical)
    dlo, dhi = _cells(db, spherical)
    order = np.arange(slo.size) if slo.size < 2 or slo[1] > slo[0] else np.arange(slo.size)[::-1]      # ascending position
    lo_sorted, hi_sorted = slo[order], shi[order]
    taps = []
    for d in range(dlo.size):
        if periodic:
            shifts = range(int(math.floor((dlo[d] - shi.max()) / period)), int(math.ceil((dhi[d] - slo.min()) / period)) + 1)
        else:
            shifts = (0,)
        row = []
        for k in shifts:
            off = float(k) * period if periodic else 0.0
            lo_k, hi_k = (lo_sorted + off, hi_sorted + off) if periodic else (lo_sorted, hi_sorted)
            first = int(np.searchsorted(hi_k, dlo[d], 'right'))
            last = int(np.searchsorted(lo_k, dhi[d], 'left'))
            for q in range(first, last):
                w = float(_overlap(lo_k[q], hi_k[q], dlo[d], dhi[d]))
                if w > 0:
                    row.append((int(order[q]), w))
        if not periodic:
            row.sort(key=lambda t: t[0])              # ascending source index
        taps.append(row)                              # (periodic: ascending unwrapped position, as found)
    return taps, dhi - dlo, shi - slo


def _ascending(c):
    """-> (the centres ascending, the source index of each)"""
    if c.size < 2 or c[1] > c[0]:
        return c, np.arange(c.size)
    return c[::-1], np.arange(c.size)[::-1]


def _reduced(v, c0, period):
    """v brought into [c0, c0 + period]"""
    r = v - math.floor((v - c0) / period) * period
    return min(max(r, c0), c0 + period)


def _point_taps(sc, dc, method, periodic, period, extrapolate):
    ca, src = _ascending(sc)
    n = ca.size
    if periodic:
        ext = np.append(ca, ca[0] + period)
        src = np.append(src, src[0])
    else:
        ext = ca
    taps = []
    for v in dc:
        v = float(v)
        if periodic:
            v = _reduced(v, float(ca[0]), period)
        elif v < ext[0] or v > ext[-1]:
            edge = int(src[0] if v < ext[0] else src[-1])
            taps.append([(edge, 1.0)] if (method == 'nearest' or extrapolate == 'nearest') else [])
            continue
        k = min(int(np.searchsorted(ext, v, 'right')) - 1, ext.size - 2) if ext.size > 1 else 0
        if ext.size == 1:
            taps.append([(int(src[0]), 1.0)])
            continue
        if method == 'nearest':
            dl, dr = v - ext[k], ext[k + 1] - v
            a, b = int(src[k]), int(src[k + 1])
            pick = a if dl < dr else (b if dr < dl else min(a, b))
            taps.append([(pick, 1.0)])
            continue
        t = (v - ext[k]) / (ext[k + 1] - ext[k])
        row = [(int(src[k]), 1.0 - t), (int(src[k + 1]), t)]
        row = [(s, float(w)) for s, w in row if w > 0]
        if not periodic:
            row.sort(key=lambda q: q[0])
        taps.append(row)
    return taps


def axis_table(src, dst, method='conservative', spherical=False, periodic=False, period=360.0, src_bounds=None, dst_bounds=None,
               extrapolate='nearest'):
    """The taps of one axis from the ``src`` to the ``dst`` cell centres (host arithmetic in fp64, no library call) -> `AxisTable`.

    * ``'conservative'``: from cell bounds (``src_bounds`` / ``dst_bounds``, or `cell_bounds` of the centres).  With g(v) = v, or
      g(phi) = sin(phi pi / 180) for ``spherical`` latitudes, a cell is [min, max] of g at its two bounds and the weight of source s
      in destination d is max(0, min(hi_s, hi_d) - max(lo_s, lo_d)); taps of weight 0 are dropped.
    * ``'bilinear'``: from centres; for c[k] <= v < c[k + 1] (centres in ascending order) t = (v - c[k]) / (c[k + 1] - c[k]) and the
      taps are (k, 1 - t), (k + 1, t), a zero weight dropped; outside the centres ``extrapolate='nearest'`` gives the edge centre
      with weight 1, ``'nan'`` no tap.
    * ``'nearest'``: the nearest centre with weight 1, a tie going to the lower source index.

    Either side may ascend or descend.  Taps are listed in ascending source index.  ``periodic`` (a longitude axis): the source is
    repeated every ``period``; its bounds must span one period within 1e-9; the taps are listed in ascending unwrapped position
    along the destination cell, and a source cell cut by the seam may appear twice."""
    if method not in METHODS:
        raise ValueError(f'`method` must be one of {METHODS}, got {method!r}')
    if extrapolate not in EXTRAPOLATE:
        raise ValueError(f'`extrapolate` must be one of {EXTRAPOLATE}, got {extrapolate!r}')
    if periodic and spherical:
        raise ValueError('`periodic` applies to the longitude axis only')
    period = float(period)
    if periodic and not (period > 0 and math.isfinite(period)):
        raise ValueError(f'`period` must be positive and finite, got {period!r}')
    sc, sb = cell_bounds(src, src_bounds, 'src', spherical)
    dc, db = cell_bounds(dst, dst_bounds, 'dst', spherical)
    if periodic:
        if sb is None:
            raise ValueError('a periodic source of one cell needs `src_bounds`')
        if abs(abs(sb[-1] - sb[0]) - period) > PERIOD_TOLERANCE:
            raise ValueError(f'a periodic source must span exactly one period ({period}), its bounds span {abs(sb[-1] - sb[0])}')
    if method == 'conservative':
        if sb is None or db is None:
            raise ValueError('conservative regridding of a one-cell axis needs its bounds')
        taps, dm, sm = _conservative(sb, db, spherical, periodic, period)
    else:
        taps = _point_taps(sc, dc, method, periodic, period, extrapolate)
        dm = np.subtract(*_cells(db, spherical)[::-1]) if db is not None else np.ones(dc.size)
        sm = np.subtract(*_cells(sb, spherical)[::-1]) if sb is not None else np.ones(sc.size)
    ptr = np.zeros(len(taps) + 1, np.int64)
    ptr[1:] = np.cumsum([len(r) for r in taps])
    if ptr[-1] >= CELL_BOUND:
        raise ValueError('too many taps')
    idx = np.array([s for r in taps for s, _ in r], np.int32).reshape(-1)
    w = np.array([v for r in taps for _, v in r], np.float64).reshape(-1)
    total = np.array([math.fsum(v for _, v in r) for r in taps])
    if method == 'conservative':
        with np.errstate(divide='ignore', invalid='ignore'):
            cover = np.where(dm > 0, total / np.where(dm > 0, dm, 1.0), 0.0)
    else:
        cover = total
    return AxisTable(ptr.astype(np.int32), idx, w, np.asarray(dm, np.float64), np.asarray(sm, np.float64), cover)


def check_regrid_args(src_lat, src_lon, dst_lat, dst_lon, method='conservative', geometry='spherical', periodic=False, period=360.0,
                      src_lat_bounds=None, src_lon_bounds=None, dst_lat_bounds=None, dst_lon_bounds=None, extrapolate='nearest',
                      skipna=False, min_valid=0.5, batch_size=None):
    """The argument rules of a regridding request (no library call) -> (the latitude table, the longitude table), both `AxisTable`.
    Raises ValueError for: an unknown ``method`` / ``geometry`` / ``extrapolate``; coordinates that are not finite or not strictly
    monotone; an axis of fewer than 1 cell; bounds whose length is not one more than the cells; latitudes beyond +-90 with spherical
    geometry; a periodic source that does not span one ``period`` within 1e-9; ``min_valid`` outside [0, 1]; a ``batch_size`` that
    is not a positive integer; grids of 2^31 cells or more."""
    if method not in METHODS:
        raise ValueError(f'`method` must be one of {METHODS}, got {method!r}')
    if geometry not in GEOMETRIES:
        raise ValueError(f'`geometry` must be one of {GEOMETRIES}, got {geometry!r}')
    if extrapolate not in EXTRAPOLATE:
        raise ValueError(f'`extrapolate` must be one of {EXTRAPOLATE}, got {extrapolate!r}')
    if isinstance(min_valid, (bool, np.bool_)) or not isinstance(min_valid, (int, float, np.integer, np.floating)) or \
            not 0.0 <= float(min_valid) <= 1.0:
        raise ValueError(f'`min_valid` must be a number in [0, 1], got {min_valid!r}')
    check_batch_size(batch_size)
    ty = axis_table(src_lat, dst_lat, method, geometry == 'spherical', False, period, src_lat_bounds, dst_lat_bounds, extrapolate)
    tx = axis_table(src_lon, dst_lon, method, False, bool(periodic), period, src_lon_bounds, dst_lon_bounds, extrapolate)
    if ty.src_measure.size * tx.src_measure.size >= CELL_BOUND or ty.dst_measure.size * tx.dst_measure.size >= CELL_BOUND:
        raise ValueError('grids of H*W >= 2^31 cells are not supported')
    return ty, tx


def consistency_from_sums(sums, counts):
    """The scores from the sums of `dl4ds_regrid_consistency` (host arithmetic only): ``sums`` (N, C, 6) fp64 = sum A, sum A d,
    sum A d^2, sum A y, sum A r, max |d| over the valid cells (d = r - y: the regridded prediction minus the reference, A the cell
    area), ``counts`` (N, C, 2) int64 = valid cells, cells where exactly one side is finite.  -> a dict of (N, C) arrays ``bias`` =
    sum A d / sum A, ``rmse`` = sqrt(sum A d^2 / sum A), ``max_abs``, ``relative_mass_error`` = (sum A r - sum A y) / sum A y (NaN on
    a zero denominator or without a valid cell), ``n_valid``, ``n_mismatch``; the same scores pooled over the samples as
    ``..._pooled`` (C,), from the `math.fsum` of each sum over the samples; and ``sums`` and ``counts`` themselves."""
    from . import _exact
    from .metrics import _fsum_axis0
    sums, counts = np.asarray(sums, np.float64), np.asarray(counts, np.int64)
    if sums.ndim != 3 or sums.shape[2] != 6 or counts.shape != sums.shape[:2] + (2,):
        raise ValueError(f'expected sums (N, C, 6) and counts (N, C, 2), got {sums.shape} and {counts.shape}')

    def scores(s, nv):
        some = nv > 0
        with np.errstate(invalid='ignore', divide='ignore', over='ignore'):
            return dict(bias=np.where(some, _exact.ratio(s[..., 1], s[..., 0]), np.nan),
                        rmse=np.where(some, np.sqrt(_exact.ratio(s[..., 2], s[..., 0])), np.nan),
                        max_abs=np.where(some, s[..., 5], np.nan),
                        relative_mass_error=np.where(some, _exact.ratio(s[..., 4] - s[..., 3], s[..., 3]), np.nan))
    res = scores(sums, counts[..., 0])
    res.update(n_valid=counts[..., 0], n_mismatch=counts[..., 1])
    pooled = _fsum_axis0(sums[..., :5], np.ones(sums.shape[:2], bool))
    pooled = np.concatenate([pooled, sums[..., 5].max(axis=0)[:, None]], axis=1)
    pc = counts.sum(axis=0)
    res.update({k + '_pooled': v for k, v in scores(pooled, pc[..., 0]).items()})
    res.update(n_valid_pooled=pc[..., 0], n_mismatch_pooled=pc[..., 1], sums=sums, counts=counts)
    return res


class Regridder:
    """Regrids (N, H, W, C) fields from the grid (``src_lat``, ``src_lon``) to (``dst_lat``, ``dst_lon``): cell centres in degrees,
    ascending or descending; ``method`` 'conservative' (area-weighted means over the overlaps of the cells; bounds from
    ``*_bounds`` or from the centres), 'bilinear' or 'nearest'; ``geometry`` 'spherical' (latitude weights are differences of sines,
    i.e. cell areas) or 'planar'; ``periodic``: the longitudes wrap with ``period``.  ``skipna``: NaN and +-inf inputs are left out
    and an output needs ``min_valid`` of its weight to remain; without it non-finite inputs propagate.  `check_regrid_args` lists
    the refusals.  The tables are built on the host; the device plan is made at the first use and freed by `close` (or with the
    object).  Attributes: ``lat_table_``, ``lon_table_`` (`AxisTable`), ``shape_in`` (H, W), ``shape_out`` (H', W'), ``coverage_``
    (H', W'): the share of each destination cell's measure that the source covers, ``dst_area_`` (H', W')."""

    def __init__(self, src_lat, src_lon, dst_lat, dst_lon, method='conservative', geometry='spherical', periodic=False,
                 src_lat_bounds=None, src_lon_bounds=None, dst_lat_bounds=None, dst_lon_bounds=None, period=360.0,
                 extrapolate='nearest', skipna=False, min_valid=0.5, batch_size=None):
        self.lat_table_, self.lon_table_ = check_regrid_args(src_lat, src_lon, dst_lat, dst_lon, method, geometry, periodic, period,
                                                             src_lat_bounds, src_lon_bounds, dst_lat_bounds, dst_lon_bounds,
                                                             extrapolate, skipna, min_valid, batch_size)
        self.method, self.geometry, self.periodic, self.extrapolate = method, geometry, bool(periodic), extrapolate
        self.skipna, self.min_valid, self.batch_size = bool(skipna), float(min_valid), batch_size
        ty, tx = self.lat_table_, self.lon_table_
        self.shape_in = (ty.src_measure.size, tx.src_measure.size)
        self.shape_out = (ty.dst_measure.size, tx.dst_measure.size)
        self.coverage_ = np.outer(ty.coverage, tx.coverage)
        self.dst_area_ = np.outer(ty.dst_measure, tx.dst_measure)
        self._plan = None

    @classmethod
    def from_scale(cls, hr_shape, scale, method='conservative', refine=False, **kw):
        """The planar index grids of the dl4ds case: the (H, W) = ``hr_shape`` cells of the fine grid have unit width, the coarse
        grid has int(H / scale) x int(W / scale) equal cells over the same domain (``scale`` an integer or not).  -> the regridder
        from the fine to the coarse grid, or with ``refine`` from the coarse to the fine one."""
        if isinstance(scale, (bool, np.bool_)) or not isinstance(scale, (int, float, np.integer, np.floating)) or \
                not (math.isfinite(scale) and scale >= 1):
            raise ValueError(f'`scale` must be a finite number >= 1, got {scale!r}')
        try:
            H, W = (int(v) for v in hr_shape)
        except (TypeError, ValueError):
            raise ValueError(f'`hr_shape` must be (H, W), got {hr_shape!r}') from None
        h, w = int(H / scale), int(W / scale)
        if H < 1 or W < 1 or h < 1 or w < 1:
            raise ValueError(f'`hr_shape` {(H, W)} leaves no coarse cell at scale {scale}')
        fine = [np.arange(n + 1, dtype=np.float64) for n in (H, W)]
        coarse = [np.arange(m + 1, dtype=np.float64) * n / m for n, m in ((H, h), (W, w))]
        src, dst = (coarse, fine) if refine else (fine, coarse)
        mid = lambda b: (b[:-1] + b[1:]) / 2                        # noqa: E731
        return cls(mid(src[0]), mid(src[1]), mid(dst[0]), mid(dst[1]), method=method, geometry='planar', periodic=False,
                   src_lat_bounds=src[0], src_lon_bounds=src[1], dst_lat_bounds=dst[0], dst_lon_bounds=dst[1], **kw)

    # ---- the device plan
    def _handle(self):
        if self._plan is None:
            import ctypes
            from . import _lib
            ty, tx = self.lat_table_, self.lon_table_
            keep = [np.ascontiguousarray(a) for a in (ty.ptr, ty.idx, ty.w, tx.ptr, tx.idx, tx.w, ty.dst_measure, tx.dst_measure)]
            h = ctypes.c_void_p()
            _lib.check(_lib.lib().dl4ds_regrid_plan_create(self.shape_in[0], self.shape_in[1], self.shape_out[0], self.shape_out[1],
                                                           *(a.ctypes.data for a in keep), ctypes.byref(h)))
            self._plan = h.value
        return self._plan

    def close(self):
        """frees the device plan (it is made again at the next use)"""
        if getattr(self, '_plan', None):
            from . import _lib
            plan, self._plan = self._plan, None
            _lib.check(_lib.lib().dl4ds_regrid_plan_destroy(plan))

    free = close

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _checked(self, x, name, grid):
        x, shape = as_4d(x, name)
        shape = check_4d_shape(shape, name)
        if shape[1:3] != tuple(grid):
            raise ValueError(f'`{name}` must be (N, {grid[0]}, {grid[1]}, C), got {shape}')
        return x, shape

    def transform(self, x, batch_size=None):
        """``x`` (N, H, W, C) -> (N, H', W', C) float32.  A host array (any dtype, or anything with ``.values``) is read as float32,
        uploaded in chunks of ``batch_size`` whole samples and comes back as a numpy array; a float32 DeviceArray is used where it
        lies and a DeviceArray comes back.  The result does not depend on ``batch_size``."""
        from . import _lib
        from .device import DeviceArray, sync
        batch_size = self.batch_size if batch_size is None else batch_size
        check_batch_size(batch_size)
        x, (N, H, W, C) = self._checked(x, 'x', self.shape_in)
        Ho, Wo = self.shape_out
        lib, plan = _lib.lib(), self._handle()

        def call(b, dx, _, dout):
            _lib.check(lib.dl4ds_regrid_apply(plan, dx, b, C, int(self.skipna), self.min_valid, dout))
        if is_device(x):
            out = DeviceArray((N, Ho, Wo, C), np.float32)
            call(N, x.ptr, None, out.ptr)
            sync()
            return out
        out = np.empty((N, Ho, Wo, C), np.float32)
        paired_chunks(x, None, [out], call, batch_size)
        return out

    __call__ = transform

    def consistency_sums(self, x, ref, return_residual=False, batch_size=None):
        """The sums of `dl4ds_regrid_consistency` of ``x`` (N, H, W, C), regridded, against ``ref`` (N, H', W', C): both host arrays
        (uploaded in chunks of whole samples) or both float32 DeviceArrays -> (sums (N, C, 6) fp64, counts (N, C, 2) int64, the
        residual (N, H', W', C) float32 or None)."""
        from . import _lib
        from .device import Buffers, sync
        batch_size = self.batch_size if batch_size is None else batch_size
        check_batch_size(batch_size)
        if is_device(x) != is_device(ref):
            raise ValueError('`x` and `ref` must both be host arrays or both be DeviceArrays')
        x, (N, H, W, C) = self._checked(x, 'x', self.shape_in)
        ref, rshape = self._checked(ref, 'ref', self.shape_out)
        if rshape != (N,) + tuple(self.shape_out) + (C,):
            raise ValueError(f'`ref` must be {(N,) + tuple(self.shape_out) + (C,)}, got {rshape}')
        Ho, Wo = self.shape_out
        lib, plan = _lib.lib(), self._handle()
        sums, counts = np.zeros((N, C, 6), np.float64), np.zeros((N, C, 2), np.int64)
        resid = np.empty((N, Ho, Wo, C), np.float32) if return_residual else None
        device = is_device(x)
        bmax = N if device else upload_batch(batch_size, max(H * W, Ho * Wo) * C, N)
        with Buffers() as buf:
            ds, dc = buf.alloc((bmax, C, 6), np.float64), buf.alloc((bmax, C, 2), np.int64)
            dr = buf.alloc((bmax, Ho, Wo, C), np.float32) if return_residual else None
            dx = x if device else buf.alloc((bmax, H, W, C), np.float32)
            dy = ref if device else buf.alloc((bmax, Ho, Wo, C), np.float32)
            for i in range(0, N, bmax):
                b = min(bmax, N - i)
                if not device:
                    dx.upload(np.ascontiguousarray(x[i:i + b], np.float32))
                    dy.upload(np.ascontiguousarray(ref[i:i + b], np.float32))
                _lib.check(lib.dl4ds_regrid_consistency(plan, dx.ptr, dy.ptr, b, C, int(self.skipna), self.min_valid, ds.ptr, dc.ptr,
                                                        dr.ptr if dr is not None else None))
                sync()
                ds.download(sums[i:i + b])
                dc.download(counts[i:i + b])
                if dr is not None:
                    dr.download(resid[i:i + b])
        return sums, counts, resid


def regrid(x, src_lat, src_lon, dst_lat, dst_lon, **kw):
    """``Regridder(src_lat, src_lon, dst_lat, dst_lon, **kw).transform(x)`` in one call; the plan is freed on the way out."""
    r = Regridder(src_lat, src_lon, dst_lat, dst_lon, **kw)
    try:
        return r.transform(x)
    finally:
        r.close()


def consistency_scores(lr, hr_pred, regridder=None, scale=None, mask=None, batch_size=None, return_residual=False):
    """Does the downscaled field ``hr_pred`` (N, H, W, C) give back its coarse input ``lr`` (N, H', W', C) when it is regridded onto
    the coarse grid?  ``regridder`` maps the fine to the coarse grid; without one, ``scale`` gives
    ``Regridder.from_scale((H, W), scale)``: conservative means over the planar index grids.  Both arrays are host arrays (any
    dtype; ``mask`` on the coarse grid, 2-D or with a channel axis, 0 = excluded, sets cells of ``lr`` to NaN) or both float32
    DeviceArrays (no ``mask``: mark excluded cells with NaN).  The regridded prediction, rounded to float32 as `Regridder.transform`
    stores it, is compared with ``lr`` on the device where both are finite, with the destination cell areas as weights.  -> the dict
    of `consistency_from_sums` (``bias``, ``rmse``, ``max_abs``, ``relative_mass_error``, ``n_valid``, ``n_mismatch`` per (N, C)
    and ``..._pooled`` per channel) and, with ``return_residual``, ``residual`` (N, H', W', C) float32, NaN where not valid.  One
    summation order: the same bits every call and for every ``batch_size``."""
    check_batch_size(batch_size)
    if is_device(lr) != is_device(hr_pred):
        raise ValueError('`lr` and `hr_pred` must both be host arrays or both be DeviceArrays')
    hr_pred, hshape = as_4d(hr_pred, 'hr_pred')
    hshape = check_4d_shape(hshape, 'hr_pred')
    if mask is not None and is_device(lr):
        masked(lr, mask)                                                  # (raises: a DeviceArray cannot take one)
    own = regridder is None
    if own:
        if scale is None:
            raise ValueError('give a `regridder` or a `scale`')
        regridder = Regridder.from_scale(hshape[1:3], scale)
    elif scale is not None:
        raise ValueError('give a `regridder` or a `scale`, not both')
    try:
        if not is_device(lr):
            lr = masked(as_4d(lr, 'lr')[0], mask)
        sums, counts, resid = regridder.consistency_sums(hr_pred, lr, return_residual, batch_size)
    finally:
        if own:
            regridder.close()
    res = consistency_from_sums(sums, counts)
    if return_residual:
        res['residual'] = resid
    return res


class _CallableModule(types.ModuleType):
    """``dl4ds_amd.regrid`` names this module as soon as it is imported, and the one-call form has the same name: calling the module
    is calling `regrid`, so ``dl4ds_amd.regrid(x, ...)`` works whichever of the two the attribute holds."""

    def __call__(self, *args, **kw):
        return regrid(*args, **kw)


sys.modules[__name__].__class__ = _CallableModule
