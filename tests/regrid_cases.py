"""The seeded cases the CPU and GPU tests of the regridding share (tests/test_regrid_device_api.py, tests/test_gpu_regrid.py), and
their reference from tests/regrid_ref.py, computed once per process.

A case: the four coordinate arrays with their bounds, the arguments of `Regridder`, x (N, H, W, C) and a reference field on the
destination grid for the consistency sums (the regridded x plus noise, with a few non-finite cells).  Shapes: 7x9 -> 3x4 and
8x8 -> 2x2 (coarsening, fractional and whole overlaps), 3x4 -> 7x9 (refining; destinations outside the source centres), 64x96 ->
17x23 and its transpose (several rows and workgroup slabs; C = 3 gives an odd W'C = 69, C = 4 the 16-byte form), a 520-wide
destination (three slabs per row, lanes with three cells), a 1 x 2400 -> 1 x 4 coarsening whose 2400 x-taps exceed the LDS stage."""
import functools

import numpy as np

from tests import regrid_ref


def cells(lo, hi, n, descending=False):
    """n equal cells over [lo, hi] -> (centres, bounds)"""
    b = lo + (hi - lo) * np.arange(n + 1, dtype=np.float64) / n
    if descending:
        b = b[::-1].copy()
    return (b[:-1] + b[1:]) / 2, b


def _case(seed, src, dst, N=1, C=1, method='conservative', geometry='spherical', periodic=False, extrapolate='nearest', skipna=False,
          min_valid=0.5, lat=(-60.0, 75.0), lon=(10.0, 100.0), lat_desc=(False, False), lon_dst=None, spoil=None):
    rng = np.random.default_rng(seed)
    (H, W), (Ho, Wo) = src, dst
    slat, slatb = cells(lat[0], lat[1], H, lat_desc[0])
    dlat, dlatb = cells(lat[0], lat[1], Ho, lat_desc[1])
    slon, slonb = cells(lon[0], lon[1], W)
    dlon, dlonb = cells(*(lon_dst or lon), Wo)
    x = (rng.standard_normal((N, H, W, C)) * 3 + 280).astype(np.float32)
    if spoil:
        spoil(x)
    return dict(src_lat=slat, src_lon=slon, dst_lat=dlat, dst_lon=dlon,
                kw=dict(method=method, geometry=geometry, periodic=periodic, extrapolate=extrapolate, skipna=skipna, min_valid=min_valid,
                        src_lat_bounds=slatb, src_lon_bounds=slonb, dst_lat_bounds=dlatb, dst_lon_bounds=dlonb),
                x=x, seed=seed)


def _nan_block(x):
    x[:, 8:24, 10:40] = np.nan                        # covers whole destination cells and parts of others
    x[0, 40, 50, 0] = np.inf
    x[0, 50, 70, 0] = -np.inf


def _one_nan(x):
    x[0, 3, 4, 0] = np.nan


BUILDERS = {
    'cons_7x9_3x4': lambda: _case(1, (7, 9), (3, 4)),
    'cons_8x8_2x2_planar': lambda: _case(2, (8, 8), (2, 2), geometry='planar', lat=(0.0, 8.0), lon=(0.0, 8.0)),
    'bilinear_3x4_7x9': lambda: _case(3, (3, 4), (7, 9), method='bilinear'),
    'bilinear_3x4_7x9_nan_outside': lambda: _case(4, (3, 4), (7, 9), method='bilinear', extrapolate='nan', N=3, C=3),
    'nearest_3x4_7x9': lambda: _case(5, (3, 4), (7, 9), method='nearest', C=4),
    'cons_64x96_17x23_c3': lambda: _case(6, (64, 96), (17, 23), N=3, C=3),
    'cons_96x64_23x17_c4': lambda: _case(7, (96, 64), (23, 17), C=4),
    'cons_descending_lat': lambda: _case(8, (7, 9), (3, 4), N=3, C=4, lat_desc=(True, False)),
    'cons_descending_both': lambda: _case(9, (7, 9), (3, 4), lat_desc=(True, True)),
    'bilinear_descending_dst': lambda: _case(10, (7, 9), (5, 6), method='bilinear', lat_desc=(False, True), C=3),
    'periodic_seam_6_4': lambda: _case(11, (5, 6), (3, 4), periodic=True, lon=(0.0, 360.0), lon_dst=(-45.0, 315.0)),
    'periodic_24_10_bilinear': lambda: _case(12, (5, 24), (4, 10), method='bilinear', periodic=True, lon=(0.0, 360.0),
                                             lon_dst=(-200.0, 160.0), C=3),
    'periodic_24_10_nearest': lambda: _case(13, (5, 24), (4, 10), method='nearest', periodic=True, lon=(0.0, 360.0),
                                            lon_dst=(170.0, 530.0)),
    'skipna_min0': lambda: _case(14, (64, 96), (17, 23), skipna=True, min_valid=0.0, spoil=_nan_block),
    'skipna_min_half': lambda: _case(14, (64, 96), (17, 23), skipna=True, min_valid=0.5, spoil=_nan_block),
    'skipna_min1': lambda: _case(14, (64, 96), (17, 23), skipna=True, min_valid=1.0, spoil=_nan_block),
    'nan_propagates': lambda: _case(15, (7, 9), (3, 4), spoil=_one_nan),
    'wide_bilinear_520': lambda: _case(16, (2, 300), (3, 520), method='bilinear', N=3),
    'long_taps_2400_4': lambda: _case(17, (1, 2400), (1, 4), geometry='planar', lat=(0.0, 1.0), lon=(0.0, 2400.0)),
}
CASES = tuple(BUILDERS)


def tables(case):
    """the restatement's tables of a case -> ((ptr, idx, w) of the latitudes, of the longitudes, ay, ax)"""
    kw = case['kw']
    sph = kw['geometry'] == 'spherical'
    ry = regrid_ref.axis_rows(case['src_lat'], case['dst_lat'], kw['method'], sph, False, 360.0, kw['src_lat_bounds'],
                              kw['dst_lat_bounds'], kw['extrapolate'])
    rx = regrid_ref.axis_rows(case['src_lon'], case['dst_lon'], kw['method'], False, kw['periodic'], 360.0, kw['src_lon_bounds'],
                              kw['dst_lon_bounds'], kw['extrapolate'])
    ay = np.subtract(*regrid_ref.cell_ranges(kw['dst_lat_bounds'], sph)[::-1])
    ax = np.subtract(*regrid_ref.cell_ranges(kw['dst_lon_bounds'], False)[::-1])
    return regrid_ref.csr(ry), regrid_ref.csr(rx), ay, ax


@functools.lru_cache(maxsize=None)
def reference(name):
    """-> (the case, with its reference field under 'ref' and its tables under 'tables'; the restatement's results).  Computed once
    and shared: nobody writes into it."""
    case = BUILDERS[name]()
    ty, tx, ay, ax = tables(case)
    kw = case['kw']
    out = regrid_ref.apply(case['x'], ty, tx, kw['skipna'], kw['min_valid'])
    rng = np.random.default_rng(1000 + case['seed'])
    ref = (np.where(np.isfinite(out), out, 280.0) + rng.standard_normal(out.shape) * 0.5).astype(np.float32)
    flat = ref.reshape(-1)
    flat[::7] = out.reshape(-1)[::7]                  # exact agreement (and the regridded field's NaN) in places
    flat[3::11] = np.nan                              # finite on one side only, or on neither
    case.update(ref=ref, tables=(ty, tx, ay, ax))
    res = regrid_ref.consistency(case['x'], ref, ty, tx, ay, ax, kw['skipna'], kw['min_valid'])
    for a in [case['x'], ref] + list(res.values()):
        a.setflags(write=False)
    return case, res
