"""GPU checks of the distance-map verification (dl4ds_distance_scores, distance_scores, distance_transform)
against the restatement tests/distance_ref.py on the cases of tests/distance_cases.py: the squared maps and the eight integers
bit-equal, the fp64 sums within gamma_(n-1) * sum |term| of math.fsum, bit-equal where a sum has at most one term."""
import ctypes
import math

import numpy as np
import pytest

from tests import distance_ref
from tests.distance_cases import CASES, reference

pytestmark = pytest.mark.gpu


def flat(res):
    """a `distance_scores` result in the restatement's layout: fields on the leading axis"""
    N, C, T = res['counts'].shape[:3]
    out = dict(counts=res['counts'].reshape(N * C, T, 8), sums=res['sums'].reshape(N * C, T, 7))
    for k in ('d2_obs', 'd2_pred'):
        if k in res:
            out[k] = res[k].reshape((N * C, T) + res[k].shape[3:])
    return out


def scores(case, **kw):
    from dl4ds_amd import distance_scores
    return distance_scores(case['y'], case['p'], case['thresholds'], cutoff=case['cutoff'], alpha=case['alpha'], **kw)


def check_case(name):
    from dl4ds_amd import distance_transform
    from dl4ds_amd.distance import distance_from_sums
    case, ref = reference(name)
    res = scores(case, return_maps=True)
    distance_ref.same(flat(res), ref)
    want = distance_from_sums(ref['counts'], ref['sums'], case['y'].shape, case['thresholds'])
    np.testing.assert_array_equal(res['n_obs'], want['n_obs'])
    np.testing.assert_array_equal(res['hausdorff'], want['hausdorff'])               # (from integers alone: equal)
    y, t = case['y'], case['thresholds'][0]                                           # the transform of y alone: p plays no part
    with np.errstate(invalid='ignore'):
        ev = (np.isfinite(y) & (y >= t)).transpose(0, 3, 1, 2)
    d2 = distance_transform(y, float(t))
    assert d2.dtype == np.int32 and d2.shape == ev.shape
    for n in range(ev.shape[0]):
        for c in range(ev.shape[1]):
            np.testing.assert_array_equal(d2[n, c], distance_ref.edt_separable(ev[n, c]))
    return case, d2


@pytest.mark.parametrize('name', sorted(CASES))
def test_scores_and_transform_against_restatement(name):
    from dl4ds_amd import distance_transform
    case, d2 = check_case(name)
    if name in ('one_cell', 'w129'):
        d = distance_transform(case['y'], float(case['thresholds'][0]), squared=False)
        with np.errstate(invalid='ignore'):
            np.testing.assert_array_equal(d, np.where(d2 == distance_ref.DIST_EMPTY, np.inf, np.sqrt(d2.astype(np.float64))))


SEGMENTED = [(name, '64') for name in sorted(CASES)] + \
    [(name, '1') for name in ('w65', 'w129', 'gap_columns', 'nonfinite', 'empty_pred', 'three_channels', 'single_row')]


@pytest.mark.parametrize('name,seg', SEGMENTED)
def test_rows_walked_segment_by_segment(monkeypatch, name, seg):
    """DL4DS_EDT_SEG lowers the columns of a row segment: at 64 every case goes through it again and the 65- to 193-wide ones cross
    segments, at 1 every column is a segment of its own"""
    monkeypatch.setenv('DL4DS_EDT_SEG', seg)
    check_case(name)


def test_two_calls_give_the_same_bits():
    case, _ = reference('random_005')
    a, b = (flat(scores(case, return_maps=True)) for _ in range(2))
    for k in a:
        assert a[k].tobytes() == b[k].tobytes(), k


def test_device_array_and_chunks():
    from dl4ds_amd import distance_scores, distance_transform
    from dl4ds_amd.device import DeviceArray
    for name in ('three_channels', 'w129', 'nonfinite'):
        case, ref = reference(name)
        one = flat(scores(case, return_maps=True))
        per_sample = flat(scores(case, return_maps=True, batch_size=1))
        dy, dp = DeviceArray.from_numpy(case['y']), DeviceArray.from_numpy(case['p'])
        try:
            dev = flat(distance_scores(dy, dp, case['thresholds'], cutoff=case['cutoff'], alpha=case['alpha'], return_maps=True))
            t0 = float(case['thresholds'][0])
            np.testing.assert_array_equal(distance_transform(dy, t0), distance_transform(case['y'], t0, batch_size=1))
        finally:
            dy.free()
            dp.free()
        for got in (per_sample, dev):
            distance_ref.same(got, ref)
            for k in one:
                assert got[k].tobytes() == one[k].tobytes(), (name, k)


def test_mask_sets_cells_to_nan():
    from dl4ds_amd import distance_scores, distance_transform
    case, _ = reference('random_005')
    y, p = case['y'], case['p']
    mask = np.ones(y.shape[1:3], np.int8)
    mask[10:30, 40:90] = 0
    ym = np.array(y)
    ym[:, 10:30, 40:90] = np.nan
    cutoff = math.hypot(y.shape[1] - 1, y.shape[2] - 1)
    want = distance_ref.distance(ym, p, case['thresholds'], cutoff, case['alpha'])
    got = distance_scores(y, p, case['thresholds'], mask=mask, return_maps=True)
    distance_ref.same(flat(got), want)
    assert got['cutoff'] == cutoff and (got['n_valid'] == y.shape[1] * y.shape[2] - 20 * 50).all()
    d2 = distance_transform(y, float(case['thresholds'][0]), mask=mask)
    with np.errstate(invalid='ignore'):
        np.testing.assert_array_equal(d2[0, 0], distance_ref.edt_separable(ym[0, :, :, 0] >= case['thresholds'][0]))


def test_prediction_is_the_observation():
    """p is y, host arrays and one DeviceArray given twice: both maps are the one transform, every distance is 0"""
    from dl4ds_amd import distance_scores
    from dl4ds_amd.device import DeviceArray
    case, _ = reference('nonfinite')
    y = case['y']
    want = distance_ref.distance(y, y, case['thresholds'], 7.5, case['alpha'])
    distance_ref.same(flat(distance_scores(y, y, case['thresholds'], cutoff=7.5, return_maps=True)), want)
    d = DeviceArray.from_numpy(y)
    try:
        got = distance_scores(d, d, case['thresholds'], cutoff=7.5, return_maps=True)
    finally:
        d.free()
    distance_ref.same(flat(got), want)
    np.testing.assert_array_equal(got['d2_obs'], got['d2_pred'])
    assert (got['hausdorff'] == 0).all() and (got['pratt'] == 1).all() and (got['baddeley_max'] == 0).all()


def raw_call(y, p, thr, cutoff, alpha, null=(), shape=None):
    """dl4ds_distance_scores itself -> (status, outputs in the restatement's layout); `null`: arguments passed as null pointers"""
    import dl4ds_amd._lib as L
    from dl4ds_amd.device import Buffers, sync
    N, H, W, C = shape or y.shape
    F, T = y.shape[0] * y.shape[3], len(thr)
    thr = np.ascontiguousarray(thr, np.float32)
    host = dict(counts=np.full((F, T, 8), -3, np.int64), sums=np.full((F, T, 7), -3.0), d2_obs=np.full((F, T) + y.shape[1:3], -3, np.int32),
                d2_pred=np.full((F, T) + y.shape[1:3], -3, np.int32))
    with Buffers() as buf:
        dy, dp = buf.alloc(y.shape), buf.alloc(y.shape)
        dy.upload(np.ascontiguousarray(y, np.float32))
        dp.upload(np.ascontiguousarray(p, np.float32))
        devs = {k: buf.alloc(v.shape, v.dtype) for k, v in host.items()}
        for k, d in devs.items():
            d.upload(host[k])
        ptr = lambda k: None if k in null else devs[k].ptr                            # noqa: E731
        st = L.lib().dl4ds_distance_scores(None if 'y' in null else dy.ptr, None if 'p' in null else dp.ptr, N, H, W, C,
                                           None if 'thr' in null else thr.ctypes.data, T, cutoff, alpha, ptr('counts'), ptr('sums'),
                                           ptr('d2_obs'), ptr('d2_pred'))
        if st == 0:
            sync()
        for k, d in devs.items():
            d.download(host[k])
    return st, host


def test_raw_entry_with_null_map_pointers():
    case, ref = reference('three_channels')
    cutoff = math.hypot(19, 29)
    for null in (('d2_obs', 'd2_pred'), ('d2_pred',), ('d2_obs',)):
        st, got = raw_call(case['y'], case['p'], case['thresholds'], cutoff, case['alpha'], null=null)
        assert st == 0
        distance_ref.same(got, ref, maps=False)
        for k in ('d2_obs', 'd2_pred'):
            if k in null:
                assert (got[k] == -3).all()                                           # (its buffer was not handed over: untouched)
            else:
                np.testing.assert_array_equal(got[k], ref[k])


def test_raw_entry_refusals():
    """non-zero with a message, before any launch: nothing is written (the outputs keep what they were uploaded with)"""
    import dl4ds_amd._lib as L
    y = np.ones((1, 4, 5, 1), np.float32)
    ok = dict(thr=[0.5], cutoff=2.0, alpha=1 / 9)
    for kw in (dict(null=('y',)), dict(null=('p',)), dict(null=('thr',)), dict(null=('counts',)), dict(null=('sums',)),
               dict(thr=[np.nan]), dict(thr=[0.5, np.inf]), dict(thr=[-np.inf]), dict(cutoff=0.0), dict(cutoff=-1.0), dict(cutoff=np.nan),
               dict(alpha=0.0), dict(alpha=-1.0), dict(alpha=np.inf), dict(alpha=np.nan), dict(shape=(0, 4, 5, 1)),
               dict(shape=(1, 0, 5, 1)), dict(shape=(1, 4, 0, 1)), dict(shape=(1, 4, 5, 0)), dict(shape=(1, 46342, 1, 1)),
               dict(shape=(1, 1, 46342, 1)), dict(shape=(1, 32769, 32769, 1))):
        a = dict(ok, **kw)
        st, out = raw_call(y, y, a['thr'], a['cutoff'], a['alpha'], null=a.get('null', ()), shape=a.get('shape'))
        assert st != 0 and b'distance_scores' in L.load().dl4ds_last_error(), kw
        assert all((v == -3).all() for v in out.values()), kw
    lib = L.lib()
    one = ctypes.c_void_p(8)                                              # (never dereferenced: T is refused first)
    assert lib.dl4ds_distance_scores(one, one, 1, 4, 5, 1, one, 0, 2.0, 0.5, one, one, None, None) != 0
    st, out = raw_call(y, y, [0.5], math.inf, 1 / 9)                      # and the entry still works afterwards; cutoff may be +inf
    assert st == 0 and out['counts'][0, 0].tolist() == [20, 20, 20, 20, 0, 0, 0, 0] and out['sums'][0, 0].tolist() == [0, 0, 20, 20, 0, 0, 0]
    assert not out['d2_obs'].any() and not out['d2_pred'].any()
