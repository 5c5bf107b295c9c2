"""Checks of the object-based verification's host side (dl4ds_amd.objects): the sequential restatement tests/objects_ref.py
against scipy.ndimage on every case of tests/objects_cases.py at both connectivities, SAL answers worked by hand, the attribute
summary, the argument rules with the library made unreachable, and the exports."""
import inspect

import numpy as np
import pytest
from scipy import ndimage

from tests import objects_ref
from tests.objects_cases import CASES, field_thresholds


@pytest.mark.parametrize('connectivity', [1, 2])
@pytest.mark.parametrize('name', sorted(CASES))
def test_restatement_against_scipy(name, connectivity):
    """labels equal scipy.ndimage.label's (the same raster-order numbering); area, mass, vmax, centroid and bbox agree with
    ndimage.sum / maximum / center_of_mass / find_objects"""
    c = CASES[name]()
    x, thr = c['x'], field_thresholds(c)
    got = objects_ref.objects(x, thr, connectivity)
    N, H, W, C = x.shape
    structure = ndimage.generate_binary_structure(2, connectivity)
    for f in range(N * C):
        v = x[f // C, :, :, f % C]
        with np.errstate(invalid='ignore'):
            event = np.isfinite(v) & (v >= thr[f])
        lab, n = ndimage.label(event, structure)
        assert n == got['count'][f]
        np.testing.assert_array_equal(lab, got['labels'][f])
        assert got['nvalid'][f] == np.isfinite(v).sum()
        assert (got['sums'][f, n:] == 0).all() and (got['mass'][f, n:] == 0).all()
        if n == 0:
            continue
        idx = np.arange(1, n + 1)
        clean = np.where(event, v, 0).astype(np.float64)
        np.testing.assert_array_equal(got['sums'][f, :n, 0], ndimage.sum(event, lab, idx).astype(np.int64))
        np.testing.assert_allclose(got['mass'][f, :n, 0], ndimage.sum(clean, lab, idx), rtol=1e-12, atol=0)
        np.testing.assert_array_equal(got['vmax'][f, :n], ndimage.maximum(np.where(event, v, -np.inf), lab, idx).astype(np.float32))
        com = np.array(ndimage.center_of_mass(event, lab, idx))
        np.testing.assert_allclose(got['sums'][f, :n, 1] / got['sums'][f, :n, 0], com[:, 0], rtol=1e-12, atol=1e-12)
        np.testing.assert_allclose(got['sums'][f, :n, 2] / got['sums'][f, :n, 0], com[:, 1], rtol=1e-12, atol=1e-12)
        for k, sl in enumerate(ndimage.find_objects(lab)):
            assert got['bbox'][f, k].tolist() == [sl[0].start, sl[0].stop - 1, sl[1].start, sl[1].stop - 1]
            assert got['first'][f, k] == np.flatnonzero(lab.ravel() == k + 1)[0]
        # second moments by definition
        ii, jj = np.nonzero(lab == 1)
        assert got['sums'][f, 0].tolist() == [len(ii), ii.sum(), jj.sum(), (ii * ii).sum(), (jj * jj).sum(), (ii * jj).sum()]
        assert (got['mass_bound'][f, :n] >= 0).all() and (got['mass_bound'][f, :n][got['sums'][f, :n, 0] == 1] == 0).all()


def test_gamma_bound():
    assert objects_ref.gamma(0) == 0.0 and objects_ref.gamma(1) == 2.0 ** -53 / (1 - 2.0 ** -53)
    assert objects_ref.ordered_key(0.0) > objects_ref.ordered_key(-0.0) > objects_ref.ordered_key(-1e-30)
    assert objects_ref.ordered_key(2.0) > objects_ref.ordered_key(1.0) > objects_ref.ordered_key(0.0)


def _objs(x, threshold=None, factor=None, connectivity=1):
    """object_attributes of the restatement's sums"""
    from dl4ds_amd.objects import object_attributes
    x = np.asarray(x, np.float32)
    thr = objects_ref.factor_thresholds(x, factor) if factor is not None else \
        np.broadcast_to(np.float32(threshold), (x.shape[0] * x.shape[3],))
    raw = objects_ref.objects(x, thr, connectivity)
    return object_attributes({k: raw[k] for k in ('labels', 'count', 'nvalid', 'field_sums', 'sums', 'bbox', 'first', 'vmax', 'mass')},
                       x.shape, thr, connectivity)


def _field(h, w, blocks):
    a = np.zeros((1, h, w, 1), np.float32)
    for i0, j0, hh, ww, v in blocks:
        a[0, i0:i0 + hh, j0:j0 + ww, 0] = v
    return a


def test_sal_identical_fields():
    """The same two objects on both sides: D, V, the centre of mass and r are the same numbers, so S = A = L1 = L2 = 0 exactly."""
    from dl4ds_amd.objects import sal_from_objects
    x = _field(30, 40, [(2, 3, 4, 5, 2.0), (20, 25, 3, 3, 5.0)])
    o = _objs(x, factor=1 / 15)
    assert o['count'].tolist() == [[2]] and o['area'].tolist() == [[[20, 9]]]
    r = sal_from_objects(o, _objs(x.copy(), factor=1 / 15), (30, 40))
    for k in ('S', 'A', 'L', 'L1', 'L2'):
        assert r[k].tolist() == [[0.0]], k


def test_sal_displaced_object():
    """One 4 x 5 object of value 2 at columns 3..7, displaced by k = 6 columns on a 30 x 40 field.  Mass 40, vmax 2 on both
    sides: V = R * (R / vmax) / R = 20 on both, S = 0; D = 40 / 1200 on both, A = 0.  The field has nothing but the object, so
    its centre of mass is the object's: r = 0 on both sides, L2 = 0.  Centres of mass (3.5, 5) and (3.5, 11):
    L1 = 6 / d with d = sqrt(29^2 + 39^2)."""
    from dl4ds_amd.objects import sal_from_objects
    o = _objs(_field(30, 40, [(2, 3, 4, 5, 2.0)]), factor=1 / 15)
    p = _objs(_field(30, 40, [(2, 9, 4, 5, 2.0)]), factor=1 / 15)
    assert o['mass'].tolist() == [[[40.0]]] and o['mass_centroid'].tolist() == [[[[3.5, 5.0]]]] and p['mass_centroid'].tolist() == [[[[3.5, 11.0]]]]
    r = sal_from_objects(o, p, (30, 40))
    assert r['S'].tolist() == [[0.0]] and r['A'].tolist() == [[0.0]] and r['L2'].tolist() == [[0.0]]
    assert r['L1'][0, 0] == 6.0 / np.hypot(29, 39) and r['L'][0, 0] == r['L1'][0, 0]


def test_sal_doubled_prediction():
    """prediction = 2 x observation with factor thresholds: the thresholds double too, so the objects are the same cells.
    D_p = 2 D_o: A = (2 - 1) / (0.5 * 3) = 2/3.  R and vmax both double, and SAL scales each mass by its maximum:
    V_p = sum 2R (2R / 2 vmax) / sum 2R = V_o, so S = 0.  Centres of mass and r do not depend on a common factor: L = 0."""
    from dl4ds_amd.objects import sal_from_objects
    x = _field(30, 40, [(2, 3, 4, 5, 2.0), (20, 25, 3, 3, 5.0), (10, 10, 2, 2, 0.25)])     # 0.25 < 5/15: below the threshold
    o, p = _objs(x, factor=1 / 15), _objs(2 * x, factor=1 / 15)
    assert o['count'].tolist() == [[2]] and p['count'].tolist() == [[2]]
    assert p['thresholds'][0, 0] == 2 * o['thresholds'][0, 0]
    r = sal_from_objects(o, p, (30, 40))
    assert abs(r['A'][0, 0] - 2.0 / 3.0) <= 2.0 ** -52
    assert r['S'].tolist() == [[0.0]] and r['L'].tolist() == [[0.0]]


def test_sal_structure_sign_and_empty_side():
    """One broad flat object (10 x 10 cells of 1: mass 100, vmax 1, V = 100) against one peaked object of equal mass (a 3 x 3
    block of 5 around a centre of 60: 8 * 5 + 60 = 100, vmax 60, V = 100 / 60).  Predicting the peaked one for the flat one:
    S = (100/60 - 100) / (0.5 (100/60 + 100)) < 0, too small / too peaked; the other way round S > 0.  A = 0: equal mass.
    A side without objects (threshold above everything): S and L are NaN, and so is A by this module's convention."""
    from dl4ds_amd.objects import sal_from_objects
    flat = _field(40, 40, [(10, 10, 10, 10, 1.0)])
    peak = _field(40, 40, [(14, 14, 3, 3, 5.0), (15, 15, 1, 1, 60.0)])
    of, op = _objs(flat, threshold=0.5), _objs(peak, threshold=0.5)
    assert of['mass'].tolist() == [[[100.0]]] and op['mass'].tolist() == [[[100.0]]] and op['vmax'].tolist() == [[[60.0]]]
    r = sal_from_objects(of, op, (40, 40))
    want = (100 / 60 - 100) / (0.5 * (100 / 60 + 100))
    assert abs(r['S'][0, 0] - want) <= 4 * 2.0 ** -53 * abs(want) and r['S'][0, 0] < 0 and r['A'].tolist() == [[0.0]]
    assert sal_from_objects(op, of, (40, 40))['S'][0, 0] == -r['S'][0, 0]
    none = _objs(flat, threshold=2.0)
    assert none['count'].tolist() == [[0]] and none['area'].shape == (1, 1, 0)
    for a, b in ((of, none), (none, of), (none, none)):
        r = sal_from_objects(a, b, (40, 40))
        for k in ('S', 'A', 'L', 'L1', 'L2'):
            assert np.isnan(r[k]).all(), k


def test_sal_zero_denominators_are_nan_and_leave_the_means():
    """Three field pairs of 6 x 6 cells, threshold 0.5 on both sides, the prediction always one cell of 1 at (0, 0).
    Pair 0: the observation is one cell of 2 at (0, 0): an ordinary pair, D_o = 2/36, D_p = 1/36, A = -1/36 / (1.5/36) = -2/3;
      V = R (R / vmax) / R = R / vmax = 1 on both sides (one cell: R = vmax), S = 0; both centres of mass at (0, 0), r = 0: L = 0.
    Pair 1: the observation is -1 everywhere but for cells of 16 and 18: its field sum is 34 * (-1) + 34 = 0, so its centre of
      mass has a zero denominator: L1, L2 (r is measured from that centre) and L are NaN.  Its two objects have masses 16 and
      18 and V = (16 + 18) / 34 = 1, so S = 0 stays defined, and D_o = 0, D_p = 1/36: A = 2.
    Pair 2: a zero mass total, set in the attributes directly: the observed side's one object gets mass 0 (as cells of +1 and
      -1 under a negative threshold would give).  It has no weight: the mass total is 0, V and r are NaN: S, L2 and L are NaN.
    The means run over the fields that are not NaN: S over pairs 0 and 1, L over pair 0 alone."""
    from dl4ds_amd.objects import sal_from_objects
    one = _field(6, 6, [(0, 0, 1, 1, 1.0)])
    zero_sum = np.full((1, 6, 6, 1), -1, np.float32)
    zero_sum[0, 1, 1, 0], zero_sum[0, 4, 4, 0] = 16, 18
    obs = np.concatenate([_field(6, 6, [(0, 0, 1, 1, 2.0)]), zero_sum, _field(6, 6, [(2, 2, 1, 2, 1.0)])])
    o, p = _objs(obs, threshold=0.5), _objs(np.concatenate([one] * 3), threshold=0.5)
    assert o['count'].tolist() == [[1], [2], [1]] and o['field_sums'][1, 0, 0] == 0.0 and o['mass'][1, 0].tolist() == [16.0, 18.0]
    o['mass'][2, 0, 0], o['raw']['mass'][2, 0, 0] = 0.0, 0.0                      # pair 2: an object of +1 and -1
    o['mass_centroid'][2, 0, 0] = np.nan
    r = sal_from_objects(o, p, (6, 6))
    assert r['S'][:2, 0].tolist() == [0.0, 0.0] and np.isnan(r['S'][2, 0])
    assert abs(r['A'][0, 0] + 2.0 / 3.0) <= 2.0 ** -52 and r['A'][1, 0] == 2.0
    assert r['L'][0, 0] == 0.0 and r['L1'][0, 0] == 0.0 and r['L2'][0, 0] == 0.0
    for k in ('L', 'L1', 'L2'):
        assert np.isnan(r[k][1, 0]), k
    assert np.isnan(r['L2'][2, 0]) and np.isnan(r['L'][2, 0])
    assert r['S_mean'] == 0.0 and r['L_mean'] == 0.0 and r['L1_mean'] == r['L1'][[0, 2], 0].mean() and r['L2_mean'] == 0.0
    for k in ('S', 'A', 'L', 'L1', 'L2'):
        assert not np.isinf(r[k]).any() and np.isfinite(r[k + '_mean']), k


def test_threshold_wrappings():
    """a threshold of one element is a scalar in any wrapping, whatever N*C is"""
    from dl4ds_amd.objects import check_object_args
    for shape in ((1, 4, 4, 1), (2, 4, 4, 3)):
        for t in (0.5, [0.5], np.full((1, 1, 1), 0.5), np.float32(0.5)):
            thr, _ = check_object_args(shape, t, 1, None, None)
            assert thr.tolist() == [0.5] * (shape[0] * shape[3])


def test_orientation_and_aspect():
    """a 3 x 12 bar along j: covariances (3^2 - 1)/12 and (12^2 - 1)/12 -> angle 0, aspect sqrt(8 / 143); along i: angle pi/2;
    along the diagonal: angle pi/4; a square: aspect 1; a single cell: NaN"""
    o = _objs(_field(40, 40, [(2, 3, 3, 12, 1.0), (10, 30, 12, 3, 1.0), (30, 2, 4, 4, 1.0), (39, 39, 1, 1, 1.0)]), threshold=0.5)
    assert o['count'].tolist() == [[4]]
    assert o['orientation'][0, 0, 0] == 0.0 and abs(o['aspect'][0, 0, 0] - np.sqrt(8 / 143)) <= 1e-15
    assert o['orientation'][0, 0, 1] == np.pi / 2 and abs(o['aspect'][0, 0, 1] - np.sqrt(8 / 143)) <= 1e-15
    assert o['aspect'][0, 0, 2] == 1.0 and np.isnan(o['aspect'][0, 0, 3])
    d = np.zeros((1, 20, 20, 1), np.float32)
    d[0, np.arange(12) + 2, np.arange(12) + 3, 0] = 1.0
    o = _objs(d, threshold=0.5, connectivity=2)
    assert o['count'].tolist() == [[1]] and abs(o['orientation'][0, 0, 0] - np.pi / 4) <= 1e-15 and o['aspect'][0, 0, 0] == 0.0


def _no_library(monkeypatch):
    import dl4ds_amd._lib as L

    def boom(*a, **k):
        raise AssertionError('the library was touched')
    monkeypatch.setattr(L, 'lib', boom)
    monkeypatch.setattr(L, 'load', boom)


@pytest.mark.parametrize('kw', [dict(threshold=np.nan), dict(threshold=np.inf), dict(threshold=1e39),
                                dict(threshold=(0.1, 0.2, 0.3)), dict(threshold='a'), dict(threshold=True),
                                dict(threshold=np.zeros((1, 2))), dict(connectivity=0), dict(connectivity=3),
                                dict(connectivity=1.0), dict(connectivity=True), dict(cap=-1), dict(cap=1.5), dict(cap=2 ** 31),
                                dict(batch_size=0), dict(batch_size=1.5), dict(shape=(2, 6, 5)), dict(shape=(0, 6, 5, 1))])
def test_argument_rules_without_a_library_call(monkeypatch, kw):
    from dl4ds_amd.objects import check_object_args
    _no_library(monkeypatch)
    args = dict(shape=(2, 6, 5, 1), threshold=0.5, connectivity=1, cap=None, batch_size=None)
    check_object_args(**args)
    args.update(kw)
    with pytest.raises(ValueError):
        check_object_args(**args)


def test_size_refusals_without_a_library_call(monkeypatch):
    from dl4ds_amd.objects import check_object_args
    _no_library(monkeypatch)
    with pytest.raises(ValueError, match=r'2\^31'):
        check_object_args((1, 2 ** 16, 2 ** 15, 1), 0.0, 1, None, None)
    with pytest.raises(ValueError, match=r'2\^31'):
        check_object_args((1, 1, 2 ** 31 - 1, 1), 0.0, 1, None, None)
    with pytest.raises(ValueError, match=r'2\^29'):
        check_object_args((1, 1, 2 ** 29, 1), 0.0, 1, None, None)
    with pytest.raises(ValueError, match=r'2\^62'):
        check_object_args((1, 4, 2 ** 28, 1), 0.0, 1, None, None)
    # the largest square below 2^31 - 1 cells: 46340^4 = 4.6112e18 < 2^62 = 4.6117e18 passes
    thr, cap = check_object_args((1, 46340, 46340, 1), 0.25, 2, None, None)
    assert cap == 4096 and thr.dtype == np.float32 and thr.tolist() == [0.25]
    edge = next(w for w in range(1, 2 ** 21) if 8 * w * w * w >= 2 ** 62)                 # H = 8 rows: exactly at the bound
    check_object_args((1, 8, edge - 1, 1), 0.0, 1, 0, 3)
    with pytest.raises(ValueError, match=r'2\^62'):
        check_object_args((1, 8, edge, 1), 0.0, 1, 0, 3)
    thr, cap = check_object_args((2, 4, 4, 3), np.arange(6).reshape(2, 3), 1, np.int64(7), None)
    assert thr.tolist() == [0, 1, 2, 3, 4, 5] and cap == 7
    assert check_object_args((2, 4, 4, 3), None, 1, None, None) == (None, 4096)


def test_factor_thresholds():
    from dl4ds_amd.objects import factor_thresholds
    x = np.random.default_rng(0).random((2, 5, 6, 3)) * 30
    x[0, 0, 0, 0], x[0, 1, 1, 1], x[1, :, :, 2] = np.nan, np.inf, np.nan
    got = factor_thresholds(x, 1 / 15)
    np.testing.assert_array_equal(got, objects_ref.factor_thresholds(x, 1 / 15))
    assert got.dtype == np.float32 and got[5] == 0 and (got[:5] > 0).all()
    for bad in (0.0, -1.0, np.nan, 'x', True):
        with pytest.raises(ValueError):
            factor_thresholds(x, bad)


def test_attribute_summary_by_hand():
    """Three objects of areas 20, 4, 9 (values 2, 3, 5) against the same field doubled: counts, areas and histograms agree (bins
    [4, 8), [8, 16), [16, 32) hold one object each), the maxima double."""
    from dl4ds_amd.objects import object_scores_from_objects, sal_from_objects
    x = _field(30, 40, [(2, 3, 4, 5, 2.0), (20, 25, 3, 3, 5.0), (10, 10, 2, 2, 3.0)])
    o, p = _objs(x, threshold=0.5), _objs(2 * x, threshold=0.5)
    assert o['count'].tolist() == [[3]] and o['area'].tolist() == [[[20, 4, 9]]] and o['bbox'][0, 0, 1].tolist() == [10, 11, 10, 11]
    assert o['centroid'][0, 0, 0].tolist() == [3.5, 5.0] and o['vmax'].tolist() == [[[2.0, 3.0, 5.0]]] and o['first'].tolist() == [[[83, 410, 825]]]
    q = object_scores_from_objects(o, p, (30, 40))
    assert q['count_ratio'].tolist() == [[1.0]] and q['largest_area_ratio'].tolist() == [[1.0]] and q['mean_vmax_ratio'].tolist() == [[2.0]]
    assert q['area_bins'][:4].tolist() == [1, 2, 4, 8] and q['area_hist_obs'][:6].tolist() == [0, 0, 1, 1, 1, 0]
    np.testing.assert_array_equal(q['area_hist_obs'], q['area_hist_pred'])
    assert q['n_objects_pred'].tolist() == [[3]] and q['event_area_obs'].tolist() == [[33]]
    assert q['mean_area_obs'].tolist() == [[11.0]] and q['max_area_pred'].tolist() == [[20]]
    s = sal_from_objects(o, o, (30, 40))
    assert s['S'].tolist() == [[0.0]] and s['S_mean'] == 0.0 and s['L_mean'] == 0.0


def test_exports_and_signatures():
    import dl4ds_amd as dds
    from dl4ds_amd import objects
    for name in ('sal_from_objects', 'check_object_args'):
        assert getattr(dds, name) is getattr(objects, name)
    assert list(inspect.signature(objects.check_object_args).parameters) == ['shape', 'threshold', 'connectivity', 'cap', 'batch_size']
    assert list(inspect.signature(objects.sal_from_objects).parameters) == ['obs_objs', 'pred_objs', 'hw']
    assert list(inspect.signature(objects.object_scores_from_objects).parameters) == ['obs_objs', 'pred_objs', 'hw']
    assert list(inspect.signature(objects.object_attributes).parameters) == ['raw', 'shape', 'thr', 'connectivity']
