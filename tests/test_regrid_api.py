"""CPU checks of the regridding's host side (dl4ds_amd/regrid.py): the axis tables against hand-worked answers
and against the dense overlap matrices of tests/regrid_ref.py, the restatement against an independent dense evaluation, the
conservation of the area integral, `consistency_from_sums` against direct numpy, every refusal, the exports and the header."""
import inspect
import math
import os

import numpy as np
import pytest

from tests import regrid_ref
from tests.regrid_cases import CASES, cells, reference

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U24, U53 = 2.0 ** -24, 2.0 ** -53


def rows(t):
    return [list(zip(t.idx[t.ptr[d]:t.ptr[d + 1]].tolist(), t.w[t.ptr[d]:t.ptr[d + 1]].tolist())) for d in range(len(t.ptr) - 1)]


def test_planar_8_to_2_and_7_to_3_by_hand():
    from dl4ds_amd.regrid import axis_table
    (sc, sb), (dc, db) = cells(0.0, 8.0, 8), cells(0.0, 8.0, 2)
    t = axis_table(sc, dc, 'conservative', src_bounds=sb, dst_bounds=db)
    assert rows(t) == [[(0, 1.0), (1, 1.0), (2, 1.0), (3, 1.0)], [(4, 1.0), (5, 1.0), (6, 1.0), (7, 1.0)]]
    assert t.ptr.dtype == np.int32 and t.idx.dtype == np.int32 and t.w.dtype == np.float64
    assert t.dst_measure.tolist() == [4.0, 4.0] and t.coverage.tolist() == [1.0, 1.0]
    t2 = axis_table(sc, dc, 'conservative')                             # bounds from the centres: the same cells
    assert rows(t2) == rows(t)
    # 7 -> 3 over [0, 21]: sources 3 wide, destinations 7 wide: 3 + 3 + 1 | 2 + 3 + 2 | 1 + 3 + 3
    (sc, sb), (dc, db) = cells(0.0, 21.0, 7), cells(0.0, 21.0, 3)
    t = axis_table(sc, dc, 'conservative', src_bounds=sb, dst_bounds=db)
    assert rows(t) == [[(0, 3.0), (1, 3.0), (2, 1.0)], [(2, 2.0), (3, 3.0), (4, 2.0)], [(4, 1.0), (5, 3.0), (6, 3.0)]]
    assert [math.fsum(w for _, w in r) for r in rows(t)] == t.dst_measure.tolist() == [7.0, 7.0, 7.0]
    # a non-integer ratio with bounds that are no binary fractions: every destination still sums to its width within rounding
    (sc, sb), (dc, db) = cells(0.1, 7.3, 7), cells(0.1, 7.3, 3)
    t = axis_table(sc, dc, 'conservative', src_bounds=sb, dst_bounds=db)
    for r, m in zip(rows(t), t.dst_measure):
        assert abs(math.fsum(w for _, w in r) - m) <= 4 * np.spacing(m)


def test_spherical_weights_are_areas():
    from dl4ds_amd.regrid import axis_table
    (sc, sb), (dc, db) = cells(-60.0, 75.0, 7), cells(-60.0, 75.0, 3)
    t = axis_table(sc, dc, 'conservative', spherical=True, src_bounds=sb, dst_bounds=db)
    want = math.sin(75.0 * math.pi / 180.0) - math.sin(-60.0 * math.pi / 180.0)
    assert abs(math.fsum(t.w) - want) <= 4 * np.spacing(want)
    assert abs(math.fsum(t.dst_measure) - want) <= 4 * np.spacing(want)
    # bounds from centres are clipped at the poles
    t = axis_table([-67.5, -22.5, 22.5, 67.5], [-45.0, 45.0], 'conservative', spherical=True)
    assert math.fsum(t.w) == 2.0 and t.dst_measure.tolist() == [1.0, 1.0]


@pytest.mark.parametrize('sdesc,ddesc', [(True, False), (False, True), (True, True)])
def test_descending_axes(sdesc, ddesc):
    from dl4ds_amd.regrid import axis_table
    (sc, sb), (dc, db) = cells(0.0, 21.0, 7, sdesc), cells(0.0, 21.0, 3, ddesc)
    t = axis_table(sc, dc, 'conservative', src_bounds=sb, dst_bounds=db)
    asc = [[(0, 3.0), (1, 3.0), (2, 1.0)], [(2, 2.0), (3, 3.0), (4, 2.0)], [(4, 1.0), (5, 3.0), (6, 3.0)]]
    want = [sorted((6 - s if sdesc else s, w) for s, w in r) for r in (asc[::-1] if ddesc else asc)]
    assert rows(t) == want                                               # ascending source index whatever the directions


def test_periodic_seam_inside_a_destination_cell():
    from dl4ds_amd.regrid import axis_table
    (sc, sb), (dc, db) = cells(0.0, 360.0, 6), cells(-45.0, 315.0, 4)
    t = axis_table(sc, dc, 'conservative', periodic=True, src_bounds=sb, dst_bounds=db)
    # destination 0 = [-45, 45]: the last source cell, moved one period back, then the first: ascending unwrapped position
    assert rows(t) == [[(5, 45.0), (0, 45.0)], [(0, 15.0), (1, 60.0), (2, 15.0)], [(2, 45.0), (3, 45.0)], [(3, 15.0), (4, 60.0), (5, 15.0)]]
    assert t.coverage.tolist() == [1.0] * 4
    per_source = np.zeros(6)
    np.add.at(per_source, t.idx, t.w)
    assert per_source.tolist() == t.src_measure.tolist() == [60.0] * 6
    # any offset, also several periods away; a source cell cut by the seam appears at both ends of a destination that spans it
    for off in (-725.0, 0.0, 3601.25):
        (dc, db) = cells(off, off + 360.0, 1)
        t = axis_table(sc, dc, 'conservative', periodic=True, src_bounds=sb, dst_bounds=db)
        assert abs(math.fsum(t.w) - 360.0) < 1e-9 and t.coverage[0] == pytest.approx(1.0, abs=1e-12)
    t = axis_table(sc, [200.0], 'conservative', periodic=True, src_bounds=sb, dst_bounds=[20.0, 380.0])
    assert rows(t) == [[(0, 40.0), (1, 60.0), (2, 60.0), (3, 60.0), (4, 60.0), (5, 60.0), (0, 20.0)]]


def test_bilinear_and_nearest_by_hand():
    from dl4ds_amd.regrid import axis_table
    src = [0.0, 1.0, 3.0]
    t = axis_table(src, [0.0, 0.25, 1.0, 2.5, 3.0], 'bilinear')
    assert rows(t) == [[(0, 1.0)], [(0, 0.75), (1, 0.25)], [(1, 1.0)], [(1, 0.25), (2, 0.75)], [(2, 1.0)]]      # coinciding: one tap
    t = axis_table(src, [-1.0, 2.0, 4.0], 'bilinear', extrapolate='nearest')
    assert rows(t) == [[(0, 1.0)], [(1, 0.5), (2, 0.5)], [(2, 1.0)]] and t.coverage.tolist() == [1.0, 1.0, 1.0]
    t = axis_table(src, [-1.0, 2.0, 4.0], 'bilinear', extrapolate='nan')
    assert rows(t) == [[], [(1, 0.5), (2, 0.5)], []] and t.coverage.tolist() == [0.0, 1.0, 0.0] and t.ptr.tolist() == [0, 0, 2, 2]
    t = axis_table(src[::-1], [0.25], 'bilinear')                        # a descending source: ascending source index
    assert rows(t) == [[(1, 0.25), (2, 0.75)]]
    t = axis_table(src, [-9.0, 0.4, 0.5, 2.0, 2.1, 9.0], 'nearest')      # ties go to the lower source index
    assert rows(t) == [[(0, 1.0)], [(0, 1.0)], [(0, 1.0)], [(1, 1.0)], [(2, 1.0)], [(2, 1.0)]]
    t = axis_table(src[::-1], [0.5, 2.0], 'nearest')
    assert rows(t) == [[(1, 1.0)], [(0, 1.0)]]
    lon = [0.0, 90.0, 180.0, 270.0]
    t = axis_table(lon, [-45.0, 315.0, 360.0, 725.0], 'bilinear', periodic=True)
    assert rows(t) == [[(3, 0.5), (0, 0.5)], [(3, 0.5), (0, 0.5)], [(0, 1.0)], [(0, 1.0 - 5.0 / 90.0), (1, 5.0 / 90.0)]]
    t = axis_table(lon, [314.0, 315.0, 316.0], 'nearest', periodic=True)
    assert rows(t) == [[(3, 1.0)], [(0, 1.0)], [(0, 1.0)]]


@pytest.mark.parametrize('name', CASES)
def test_sparse_tables_equal_the_dense_matrix(name):
    from dl4ds_amd.regrid import Regridder
    case, _ = reference(name)
    r = Regridder(case['src_lat'], case['src_lon'], case['dst_lat'], case['dst_lon'], **case['kw'])
    ty, tx, ay, ax = case['tables']
    for got, want in ((r.lat_table_, ty), (r.lon_table_, tx)):
        assert got.ptr.tolist() == want[0].tolist()
        assert regrid_ref.triples(got.ptr, got.idx, got.w) == regrid_ref.triples(*want)
        assert got.idx.tolist() == want[1].tolist()                      # and in the same order
    regrid_ref.same_bits(r.lat_table_.dst_measure, ay)
    regrid_ref.same_bits(r.lon_table_.dst_measure, ax)
    regrid_ref.same_bits(r.dst_area_, np.outer(ay, ax))
    assert r.coverage_.shape == r.shape_out == (len(ay), len(ax))
    if case['kw']['method'] == 'conservative':
        np.testing.assert_allclose(r.coverage_, 1.0, rtol=0, atol=1e-12)   # the grids of the cases cover one domain


@pytest.mark.parametrize('name', [n for n in CASES if 'skipna' not in n and n != 'nan_propagates'])
def test_restatement_against_dense_einsum(name):
    case, res = reference(name)
    ty, tx, ay, ax = case['tables']
    want, mag, taps = regrid_ref.dense_apply(case['x'], ty, tx, case['x'].shape[1:3])
    got = res['out'].astype(np.float64)
    some = np.broadcast_to(taps > 0, got.shape)
    assert np.isnan(got[~some]).all() and np.isfinite(got[some]).all()
    if case['kw']['extrapolate'] == 'nan':
        assert (~some).any()
    bound = U24 * np.abs(want) + taps * U53 * mag                        # one fp32 rounding + the fp64 sum's bound
    assert (np.abs(got - want)[some] <= bound[some]).all()


@pytest.mark.parametrize('name', ['cons_7x9_3x4', 'cons_8x8_2x2_planar', 'cons_64x96_17x23_c3', 'cons_96x64_23x17_c4',
                                  'cons_descending_lat', 'periodic_seam_6_4', 'long_taps_2400_4'])
def test_conservation_of_the_area_integral(name):
    from dl4ds_amd.regrid import Regridder
    case, res = reference(name)
    r = Regridder(case['src_lat'], case['src_lon'], case['dst_lat'], case['dst_lon'], **case['kw'])
    a_src = np.outer(r.lat_table_.src_measure, r.lon_table_.src_measure)
    x, out = case['x'].astype(np.float64), res['out'].astype(np.float64)
    taps = np.outer(np.diff(r.lat_table_.ptr), np.diff(r.lon_table_.ptr)).max()
    for n in range(x.shape[0]):
        for c in range(x.shape[3]):
            src = math.fsum((a_src * x[n, :, :, c]).ravel())
            dst = math.fsum((r.dst_area_ * out[n, :, :, c]).ravel())
            mag = math.fsum((r.dst_area_ * np.abs(out[n, :, :, c])).ravel())
            assert abs(dst - src) <= U24 * mag + (taps + 4) * U53 * math.fsum((a_src * np.abs(x[n, :, :, c])).ravel())


def test_consistency_from_sums_against_numpy():
    from dl4ds_amd.regrid import consistency_from_sums
    rng = np.random.default_rng(5)
    N, C, P = 3, 2, 40
    A = rng.random((N, C, P)) + 0.5
    y, d = rng.standard_normal((N, C, P)) + 5, rng.standard_normal((N, C, P)) * 0.1
    r = y + d
    sums = np.stack([A.sum(-1), (A * d).sum(-1), (A * d * d).sum(-1), (A * y).sum(-1), (A * r).sum(-1), np.abs(d).max(-1)], -1)
    counts = np.stack([np.full((N, C), P), np.arange(N * C).reshape(N, C)], -1).astype(np.int64)
    sums[2, 1], counts[2, 1] = 0.0, (0, 7)                               # a field without a valid cell
    res = consistency_from_sums(sums, counts)
    ok = counts[..., 0] > 0
    np.testing.assert_array_equal(res['bias'][ok], sums[..., 1][ok] / sums[..., 0][ok])
    np.testing.assert_array_equal(res['rmse'][ok], np.sqrt(sums[..., 2][ok] / sums[..., 0][ok]))
    np.testing.assert_array_equal(res['max_abs'][ok], sums[..., 5][ok])
    np.testing.assert_array_equal(res['relative_mass_error'][ok], (sums[..., 4][ok] - sums[..., 3][ok]) / sums[..., 3][ok])
    assert all(np.isnan(res[k][2, 1]) for k in ('bias', 'rmse', 'max_abs', 'relative_mass_error'))
    np.testing.assert_allclose(res['bias'][ok], ((A * d).sum(-1) / A.sum(-1))[ok], rtol=1e-13)
    assert res['n_valid'].tolist() == counts[..., 0].tolist() and res['n_mismatch'].tolist() == counts[..., 1].tolist()
    for c in range(C):
        s = [math.fsum(sums[:, c, k]) for k in range(5)]
        assert res['bias_pooled'][c] == s[1] / s[0] and res['rmse_pooled'][c] == math.sqrt(s[2] / s[0])
        assert res['relative_mass_error_pooled'][c] == (s[4] - s[3]) / s[3] and res['max_abs_pooled'][c] == sums[:, c, 5].max()
    assert res['n_valid_pooled'].tolist() == counts[..., 0].sum(0).tolist()
    with pytest.raises(ValueError):
        consistency_from_sums(sums[..., :5], counts)


def test_exact_refinement_scores_zero_in_the_restatement():
    """a prediction that repeats every coarse value over its 4 x 4 fine cells: conservative means over unit cells give it back"""
    from dl4ds_amd.regrid import Regridder, consistency_from_sums
    lr = (np.random.default_rng(6).standard_normal((2, 3, 5, 2)) * 10 + 280).astype(np.float32)
    hr = lr.repeat(4, axis=1).repeat(4, axis=2)
    r = Regridder.from_scale((12, 20), 4)
    assert r.shape_in == (12, 20) and r.shape_out == (3, 5) and (r.coverage_ == 1).all() and (r.dst_area_ == 16).all()
    assert set(r.lat_table_.w.tolist()) == {1.0} and np.diff(r.lon_table_.ptr).tolist() == [4] * 5
    t = lambda a: (a.ptr, a.idx, a.w)                                   # noqa: E731
    res = regrid_ref.consistency(hr, lr, t(r.lat_table_), t(r.lon_table_), r.lat_table_.dst_measure, r.lon_table_.dst_measure)
    regrid_ref.same_bits(res['out'], lr)
    s = consistency_from_sums(res['sums'], res['counts'])
    assert (s['max_abs'] == 0).all() and (s['bias'] == 0).all() and (s['rmse'] == 0).all() and (s['n_valid'] == 15).all()
    assert (s['relative_mass_error'] == 0).all() and (s['max_abs_pooled'] == 0).all()
    r = Regridder.from_scale((10, 9), 2.5)                               # a non-integer ratio: 4 x 3 coarse cells over the same domain
    assert r.shape_out == (4, 3) and np.allclose(r.coverage_, 1) and np.allclose(r.dst_area_, 2.5 * 3.0)
    r = Regridder.from_scale((12, 20), 4, method='bilinear', refine=True)
    assert r.shape_in == (3, 5) and r.shape_out == (12, 20)


LAT, LON = [-10.0, 0.0, 10.0], [0.0, 120.0, 240.0]


@pytest.mark.parametrize('args,kw', [
    ((LAT, LON, [0.0, 5.0, 2.0], LON), {}),                                        # non-monotone
    ((LAT, LON, LAT, [0.0, 0.0, 1.0]), {}),
    (([0.0, np.nan, 2.0], LON, LAT, LON), {}),                                     # non-finite
    ((LAT, [0.0, np.inf], LAT, LON), {}),
    (([], LON, LAT, LON), {}),                                                     # fewer than 1 cell
    ((LAT, LON, LAT, np.zeros((2, 2))), {}),
    ((LAT, LON, LAT, LON), dict(src_lat_bounds=[-15.0, -5.0, 5.0])),               # bounds of the wrong length
    ((LAT, LON, LAT, LON), dict(dst_lon_bounds=[0.0, 1.0, 2.0, 3.0, 4.0])),
    (([-95.0, 0.0, 10.0], LON, LAT, LON), {}),                                     # beyond the poles
    ((LAT, LON, LAT, LON), dict(dst_lat_bounds=[-100.0, -5.0, 5.0, 15.0])),
    ((LAT, LON, LAT, LON), dict(periodic=True, src_lon_bounds=[0.0, 100.0, 200.0, 300.0])),      # not one period
    ((LAT, [0.0, 100.0, 200.0], LAT, LON), dict(periodic=True)),
    ((LAT, LON, LAT, LON), dict(periodic=True, src_lon_bounds=[-60.0, 60.0, 180.0, 300.0 + 1e-6])),
    ((LAT, LON, LAT, LON), dict(method='bicubic')),
    ((LAT, LON, LAT, LON), dict(geometry='flat')),
    ((LAT, LON, LAT, LON), dict(extrapolate='linear')),
    ((LAT, LON, LAT, LON), dict(min_valid=1.5)),
    ((LAT, LON, LAT, LON), dict(min_valid=np.nan)),
    ((LAT, LON, LAT, LON), dict(min_valid=-0.1)),
    ((LAT, LON, LAT, LON), dict(batch_size=0)),
    (([5.0], LON, LAT, LON), {}),                                                  # one conservative cell without bounds
])
def test_refusals(monkeypatch, args, kw):
    import dl4ds_amd._lib as L
    from dl4ds_amd.regrid import Regridder, check_regrid_args

    def boom(*a, **k):
        raise AssertionError('the library was touched')
    monkeypatch.setattr(L, 'lib', boom)
    monkeypatch.setattr(L, 'load', boom)
    with pytest.raises(ValueError):
        check_regrid_args(*args, **kw)
    with pytest.raises(ValueError):
        Regridder(*args, **kw)


def test_accepted_edge_arguments():
    from dl4ds_amd.regrid import Regridder, check_regrid_args
    ty, tx = check_regrid_args(LAT, LON, LAT, LON, periodic=True, src_lon_bounds=[-60.0, 60.0, 180.0, 300.0 + 5e-10])
    assert tx.ptr[-1] >= 3 and np.diff(ty.ptr).tolist() == [1, 1, 1]
    r = Regridder([5.0], [7.0], LAT, LON, method='nearest', geometry='planar')     # one cell is a grid
    assert r.shape_in == (1, 1) and r.lat_table_.idx.tolist() == [0, 0, 0]
    r = Regridder([5.0], [7.0], [5.0], [7.0], src_lat_bounds=[0, 10], src_lon_bounds=[0, 14], dst_lat_bounds=[10, 0],
                  dst_lon_bounds=[0, 14])
    assert r.coverage_.tolist() == [[1.0]]
    for bad in ((12, 20, 3), 'ab', (0, 4)):
        with pytest.raises(ValueError):
            Regridder.from_scale(bad, 2)
    for bad in (0.5, np.nan, 'x', True, 40):
        with pytest.raises(ValueError):
            Regridder.from_scale((12, 20), bad)


def test_shape_refusals_without_a_library_call(monkeypatch):
    import dl4ds_amd._lib as L
    from dl4ds_amd.regrid import Regridder, consistency_scores

    def boom(*a, **k):
        raise AssertionError('the library was touched')
    monkeypatch.setattr(L, 'lib', boom)
    monkeypatch.setattr(L, 'load', boom)
    r = Regridder.from_scale((8, 8), 2)
    with pytest.raises(ValueError):
        r.transform(np.zeros((1, 8, 7, 1), np.float32))
    with pytest.raises(ValueError):
        r.transform(np.zeros((0, 8, 8, 1), np.float32))
    with pytest.raises(ValueError):
        r.transform(np.zeros((1, 8, 8, 1), np.float32), batch_size=0)
    with pytest.raises(ValueError):
        consistency_scores(np.zeros((1, 4, 4, 1)), np.zeros((1, 8, 8, 1)))                      # neither a regridder nor a scale
    with pytest.raises(ValueError):
        consistency_scores(np.zeros((1, 4, 4, 1)), np.zeros((1, 8, 8, 1)), regridder=r, scale=2)
    with pytest.raises(ValueError):
        consistency_scores(np.zeros((1, 4, 3, 1)), np.zeros((1, 8, 8, 1)), scale=2)
    with pytest.raises(ValueError):
        consistency_scores(np.zeros((2, 4, 4, 1)), np.zeros((1, 8, 8, 1)), scale=2)
    with pytest.raises(ValueError):
        consistency_scores(np.zeros((1, 4, 4, 1)), np.zeros((1, 8, 8, 1)), scale=2, mask=np.ones((3, 3)))


def test_exports_and_header(monkeypatch):
    import dl4ds_amd as dds
    import dl4ds_amd._lib as L
    from dl4ds_amd import regrid
    for name in ('Regridder', 'axis_table', 'check_regrid_args', 'consistency_scores', 'consistency_from_sums'):
        assert getattr(dds, name) is getattr(regrid, name)
    seen = []
    monkeypatch.setattr(regrid, 'regrid', lambda *a, **k: seen.append((a, k)))
    dds.regrid(1, 2, method='nearest')                                   # the one-call form: the module of that name forwards the call
    assert seen == [((1, 2), dict(method='nearest'))]
    sig = inspect.signature(regrid.Regridder.__init__)
    assert list(sig.parameters)[1:8] == ['src_lat', 'src_lon', 'dst_lat', 'dst_lon', 'method', 'geometry', 'periodic']
    assert sig.parameters['method'].default == 'conservative' and sig.parameters['geometry'].default == 'spherical'
    assert sig.parameters['extrapolate'].default == 'nearest' and sig.parameters['min_valid'].default == 0.5
    assert sig.parameters['skipna'].default is False and sig.parameters['batch_size'].default is None
    assert list(inspect.signature(regrid.consistency_scores).parameters) == ['lr', 'hr_pred', 'regridder', 'scale', 'mask', 'batch_size',
                                                                             'return_residual']
    protos = L.parse_header()
    assert [len(protos[n][1]) for n in ('dl4ds_regrid_plan_create', 'dl4ds_regrid_plan_destroy', 'dl4ds_regrid_apply',
                                        'dl4ds_regrid_consistency')] == [13, 1, 7, 10]
    core = open(os.path.join(ROOT, 'dl4ds_amd', 'csrc', 'regrid_core.h')).read()
    assert f'RG_THREADS = {regrid_ref.THREADS};' in core and 'RG_CELL_BOUND = 2147483648ll' in core and regrid.CELL_BOUND == 1 << 31
