"""GPU checks of the device object labelling (dl4ds_label_objects, dl4ds_object_thresholds, label_objects, sal_scores,
object_scores) against the sequential restatement tests/objects_ref.py on the cases of
tests/objects_cases.py: integers, labels and vmax bit-equal, the fp64 sums within the bound any summation order keeps."""
import ctypes

import numpy as np
import pytest

from tests import objects_ref
from tests.objects_cases import CASES
from tests.objects_shared import capped, reference, same_objects

pytestmark = pytest.mark.gpu

NAMES = ('labels', 'count', 'nvalid', 'field_sums', 'sums', 'bbox', 'first', 'vmax', 'mass')


def flat(res, shape):
    """a `label_objects` result in the restatement's layout: fields on the leading axis"""
    N, H, W, C = shape
    F, K = N * C, res['area'].shape[-1]
    out = dict(count=res['count'].reshape(F), nvalid=res['nvalid'].reshape(F), field_sums=res['field_sums'].reshape(F, 3),
               sums=res['raw']['sums'].reshape(F, K, 6), bbox=res['bbox'].reshape(F, K, 4), first=res['first'].reshape(F, K),
               vmax=res['raw']['vmax'].reshape(F, K), mass=res['raw']['mass'].reshape(F, K, 3))
    if 'labels' in res:
        out['labels'] = res['labels'].reshape(F, H, W)
    return out


def raw_call(x, thr, connectivity, cap, labels=True, null=()):
    """dl4ds_label_objects itself -> (status, outputs in the restatement's layout); `null`: outputs passed as null pointers"""
    import dl4ds_amd._lib as L
    from dl4ds_amd.device import Buffers, sync
    N, H, W, C = x.shape
    F, K = N * C, max(cap, 0)
    host = dict(labels=np.zeros((F, H, W), np.int32), count=np.zeros(F, np.int32), nvalid=np.zeros(F, np.int64),
                field_sums=np.zeros((F, 3)), sums=np.zeros((F, K, 6), np.int64), bbox=np.zeros((F, K, 4), np.int32),
                first=np.zeros((F, K), np.int32), vmax=np.zeros((F, K), np.float32), mass=np.zeros((F, K, 3)))
    with Buffers() as buf:
        dx, dthr = buf.alloc(x.shape), buf.alloc((F,))
        dx.upload(np.ascontiguousarray(x, np.float32))
        dthr.upload(np.ascontiguousarray(thr, np.float32))
        devs = {k: buf.alloc(v.shape, v.dtype) for k, v in host.items() if k not in null and (labels or k != 'labels')}
        ptr = lambda k: devs[k].ptr if k in devs else None
        st = L.lib().dl4ds_label_objects(None if 'x' in null else dx.ptr, N, H, W, C, None if 'thr' in null else dthr.ptr,
                                         connectivity, cap, *(ptr(k) for k in NAMES))
        if st == 0:
            sync()
            for k, d in devs.items():
                if host[k].nbytes:
                    d.download(host[k])
    return st, {k: v for k, v in host.items() if k in devs}


@pytest.mark.parametrize('connectivity', [1, 2])
@pytest.mark.parametrize('name', sorted(CASES))
def test_label_objects_against_restatement(name, connectivity):
    from dl4ds_amd import label_objects
    x, thr, ref = reference(name, connectivity)
    N, H, W, C = x.shape
    res = label_objects(x, threshold=thr, connectivity=connectivity)
    same_objects(flat(res, x.shape), capped(ref, res['area'].shape[-1]))
    count = ref['count'].reshape(N, C)
    K = int(count.max())
    assert res['area'].shape == (N, C, K) and res['truncated'] is False and res['labels'].shape == (N, C, H, W)
    np.testing.assert_array_equal(res['thresholds'].reshape(-1), thr)
    beyond = np.arange(K)[None, None, :] >= count[..., None]                           # padding as object_attributes defines it
    for k in ('mass', 'vmax', 'orientation', 'aspect'):
        assert np.isnan(res[k][beyond]).all() and (k == 'aspect' or not np.isnan(res[k][~beyond]).any()), k
    assert np.isnan(res['centroid'][beyond]).all() and not res['area'][beyond].any() and not res['bbox'][beyond].any()


@pytest.mark.parametrize('name', ['random_04', 'u_and_comb'])
def test_cap_cuts_rows_and_keeps_count_and_labels(name):
    from dl4ds_amd import label_objects
    x, thr, ref = reference(name, 1)
    biggest = int(ref['count'].max())
    for cap in (0, 1, biggest - 1, biggest, biggest + 3):
        res = label_objects(x, threshold=thr, cap=cap)
        got = flat(res, x.shape)
        K = min(cap, biggest)
        assert got['sums'].shape[1] == K and res['truncated'] is (cap < biggest)
        same_objects(got, capped(ref, K))
        st, raw = raw_call(x, thr, 1, cap)                                            # the raw tables: cap rows, zero from count on
        assert st == 0
        same_objects(raw, capped(ref, cap))


def test_raw_entry_without_labels_gives_the_same_tables():
    x, thr, ref = reference('nested_rings', 2)
    cap = int(ref['count'].max()) + 2
    st, got = raw_call(x, thr, 2, cap, labels=False)
    assert st == 0 and 'labels' not in got
    same_objects(got, capped(ref, cap))
    st, only = raw_call(x, thr, 2, 0, null=('nvalid', 'field_sums', 'sums', 'bbox', 'first', 'vmax', 'mass'))
    assert st == 0
    np.testing.assert_array_equal(only['labels'], ref['labels'])
    np.testing.assert_array_equal(only['count'], ref['count'])


def test_two_calls_give_the_same_bits():
    from dl4ds_amd import label_objects
    x, thr, _ = reference('random_06', 1)
    a, b = (flat(label_objects(x, threshold=thr), x.shape) for _ in range(2))
    for k in ('labels', 'count', 'nvalid', 'sums', 'bbox', 'first', 'vmax', 'field_sums'):
        assert a[k].tobytes() == b[k].tobytes(), k


def test_device_array_and_chunks():
    from dl4ds_amd import label_objects
    from dl4ds_amd.device import DeviceArray
    x, thr, ref = reference('three_channels', 1)
    one = flat(label_objects(x, threshold=thr), x.shape)
    per_sample = flat(label_objects(x, threshold=thr, batch_size=1), x.shape)
    d = DeviceArray.from_numpy(x)
    try:
        dev = flat(label_objects(d, threshold=thr), x.shape)
        fac = label_objects(d, factor=0.5, return_labels=False)
    finally:
        d.free()
    for got in (per_sample, dev):
        same_objects(got, capped(ref, got['sums'].shape[1]))
        for k in ('labels', 'count', 'sums', 'bbox', 'first', 'vmax', 'field_sums'):
            assert got[k].tobytes() == one[k].tobytes(), k
    host_fac = label_objects(x, factor=0.5, return_labels=False, batch_size=1)
    np.testing.assert_array_equal(fac['thresholds'].reshape(-1), objects_ref.factor_thresholds(x, 0.5))
    np.testing.assert_array_equal(host_fac['thresholds'], fac['thresholds'])
    np.testing.assert_array_equal(host_fac['count'], fac['count'])
    assert 'labels' not in fac


def test_mask_sets_cells_to_nan():
    from dl4ds_amd import label_objects
    x, thr, _ = reference('random_06', 2)
    mask = np.ones(x.shape[1:3], np.int8)
    mask[10:30, 40:90] = 0
    xm = np.array(x)
    xm[:, 10:30, 40:90] = np.nan
    want = objects_ref.objects(xm, thr, 2)
    got = label_objects(x, threshold=thr, connectivity=2, mask=mask)
    same_objects(flat(got, x.shape), want)


def test_object_thresholds_bit_equal():
    import dl4ds_amd._lib as L
    from dl4ds_amd.device import Buffers
    from dl4ds_amd.objects import factor_thresholds
    empty = np.full((1, 40, 70, 1), np.nan, np.float32)
    empty[0, 3, 3, 0], empty[0, 5, 5, 0] = np.inf, -np.inf
    negative = -1 - np.random.default_rng(5).random((1, 40, 70, 1)).astype(np.float32)
    for x in (CASES['nonfinite']()['x'], CASES['threshold_edges']()['x'], empty, negative, CASES['three_channels']()['x']):
        N, H, W, C = x.shape
        for factor in (1 / 15, 0.5, 1e39):
            got = np.zeros(N * C, np.float32)
            with Buffers() as buf:
                dx, dt = buf.alloc(x.shape), buf.alloc((N * C,))
                dx.upload(x)
                L.check(L.lib().dl4ds_object_thresholds(dx.ptr, N, H, W, C, factor, dt.ptr))
                dt.download(got)
            with np.errstate(over='ignore'):
                want = objects_ref.factor_thresholds(x, factor)
            np.testing.assert_array_equal(got, want)
            np.testing.assert_array_equal(got, factor_thresholds(x, factor))
            assert np.isfinite(got).all()


def _field(h, w, blocks, n=1):
    a = np.zeros((n, h, w, 1), np.float32)
    for i0, j0, hh, ww, v in blocks:
        a[:, i0:i0 + hh, j0:j0 + ww, 0] = v
    return a


def _pairs():
    """the hand-worked pairs of tests/test_objects_api.py and one seeded pair of positive random fields: (obs, pred, kwargs)"""
    two = _field(30, 40, [(2, 3, 4, 5, 2.0), (20, 25, 3, 3, 5.0)])
    three = _field(30, 40, [(2, 3, 4, 5, 2.0), (20, 25, 3, 3, 5.0), (10, 10, 2, 2, 0.25)])
    flat_, peak = _field(40, 40, [(10, 10, 10, 10, 1.0)]), _field(40, 40, [(14, 14, 3, 3, 5.0), (15, 15, 1, 1, 60.0)])
    zero_sum = np.full((1, 6, 6, 1), -1, np.float32)
    zero_sum[0, 1, 1, 0], zero_sum[0, 4, 4, 0] = 16, 18
    one = _field(6, 6, [(0, 0, 1, 1, 1.0)])
    rng = np.random.default_rng(77)
    ro, rp = (rng.gamma(0.6, 2.0, (3, 50, 90, 2)).astype(np.float32) for _ in range(2))
    return dict(identical=(two, two.copy(), dict(factor=1 / 15)),
                displaced=(_field(30, 40, [(2, 3, 4, 5, 2.0)]), _field(30, 40, [(2, 9, 4, 5, 2.0)]), dict(factor=1 / 15)),
                doubled=(three, 2 * three, dict(factor=1 / 15)),
                flat_peaked=(flat_, peak, dict(threshold=0.5)), peaked_flat=(peak, flat_, dict(threshold=0.5)),
                empty_side=(flat_, peak, dict(threshold=30.0)), both_empty=(flat_, peak, dict(threshold=90.0)),
                zero_field_sum=(np.concatenate([_field(6, 6, [(0, 0, 1, 1, 2.0)]), zero_sum]), np.concatenate([one, one]), dict(threshold=0.5)),
                random_factor=(ro, rp, dict(factor=1 / 15)), random_threshold=(ro, rp, dict(threshold=1.5, connectivity=2)))


def _restated(x, threshold=None, factor=None, connectivity=1):
    from dl4ds_amd.objects import object_attributes
    thr = objects_ref.factor_thresholds(x, factor) if factor is not None else \
        np.broadcast_to(np.float32(threshold), (x.shape[0] * x.shape[3],))
    raw = objects_ref.objects(x, thr, connectivity)
    return object_attributes({k: raw[k] for k in NAMES[1:]}, x.shape, thr, connectivity)


def _close(got, want, keys, exact):
    for k in keys:
        g, w = np.asarray(got[k]), np.asarray(want[k])
        assert g.shape == w.shape, k
        np.testing.assert_array_equal(np.isnan(g), np.isnan(w), err_msg=k)
        ok = ~np.isnan(w)
        if k in exact:
            np.testing.assert_array_equal(g[ok], w[ok], err_msg=k)
        else:
            assert (np.abs(g[ok] - w[ok]) <= 1e-9).all(), (k, g, w)


@pytest.mark.parametrize('pair', sorted(_pairs()))
def test_sal_and_object_scores_against_restatement(pair):
    from dl4ds_amd import object_scores, sal_scores
    from dl4ds_amd.objects import object_scores_from_objects, sal_from_objects
    obs, pred, kw = _pairs()[pair]
    o, p = _restated(obs, **kw), _restated(pred, **kw)
    hw = obs.shape[1:3]
    got, want = sal_scores(obs, pred, **kw), sal_from_objects(o, p, hw)
    sal = ('S', 'A', 'L', 'L1', 'L2')
    _close(got, want, sal + tuple(k + '_mean' for k in sal), ())
    np.testing.assert_array_equal(got['n_objects_obs'], o['count'])
    np.testing.assert_array_equal(got['n_objects_pred'], p['count'])
    np.testing.assert_array_equal(got['thresholds_obs'], o['thresholds'])
    np.testing.assert_array_equal(got['thresholds_pred'], p['thresholds'])
    assert got['truncated'] is False
    if 'threshold' in kw:
        got, want = object_scores(obs, pred, **kw), object_scores_from_objects(o, p, hw)
        ratios = ('count_ratio', 'largest_area_ratio', 'mean_vmax_ratio', 'mean_area_obs', 'mean_area_pred')
        _close(got, want, [k for k in want], set(want) - set(ratios))


def test_raw_entry_refusals():
    """non-zero with a message, before any launch: nothing is written (the outputs keep the zeros they were uploaded with)"""
    import dl4ds_amd._lib as L
    x, thr = np.ones((1, 4, 5, 1), np.float32), np.full(1, 0.5, np.float32)
    for kw in (dict(connectivity=3), dict(connectivity=0), dict(cap=-1), dict(null=('x',)), dict(null=('thr',)), dict(null=('count',)),
               dict(cap=2, null=('sums',)), dict(cap=2, null=('bbox',)), dict(cap=2, null=('first',)), dict(cap=2, null=('vmax',)),
               dict(cap=2, null=('mass',))):
        st, out = raw_call(x, thr, kw.get('connectivity', 1), kw.get('cap', 2), null=kw.get('null', ()))
        assert st != 0 and L.load().dl4ds_last_error(), kw
    lib = L.lib()
    one = ctypes.c_void_p(8)                                              # (never dereferenced: the sizes are refused first)
    for N, H, W, C in ((1, 2 ** 16, 2 ** 15, 1), (1, 1, 2 ** 29, 1), (1, 4, 2 ** 28, 1), (0, 4, 4, 1), (1, 0, 4, 1), (1, 4, 4, 0)):
        assert lib.dl4ds_label_objects(one, N, H, W, C, one, 1, 0, None, one, None, None, None, None, None, None, None) != 0
        assert b'label_objects' in lib.dl4ds_last_error()
        assert lib.dl4ds_object_thresholds(one, N, H, W, C, 0.5, one) != 0
    assert lib.dl4ds_object_thresholds(one, 1, 4, 4, 1, 0.0, one) != 0
    st, out = raw_call(x, thr, 1, 2)                                      # and the entry still works afterwards
    assert st == 0 and out['count'].tolist() == [1] and out['sums'][0, 0].tolist() == [20, 30, 40, 70, 120, 60]
