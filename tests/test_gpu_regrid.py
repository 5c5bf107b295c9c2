"""GPU checks of the regridding (dl4ds_regrid_plan_create / _apply / _consistency, Regridder, regrid, consistency_scores; DESIGN.md
section 30) against the restatement tests/regrid_ref.py on the cases of tests/regrid_cases.py, bit for bit: outputs and residuals on
their uint32 views (NaN included), the sums on their uint64 views, the counts as integers."""
import ctypes

import numpy as np
import pytest

from tests import regrid_ref
from tests.regrid_cases import CASES, reference

pytestmark = pytest.mark.gpu


def regridder(case, **kw):
    from dl4ds_amd import Regridder
    return Regridder(case['src_lat'], case['src_lon'], case['dst_lat'], case['dst_lon'], **dict(case['kw'], **kw))


@pytest.mark.parametrize('name', CASES)
def test_apply_and_consistency_against_restatement(name):
    case, ref = reference(name)
    r = regridder(case)
    try:
        out = r.transform(case['x'])
        assert out.dtype == np.float32
        regrid_ref.same_bits(out, ref['out'], 'out')
        sums, counts, resid = r.consistency_sums(case['x'], case['ref'], return_residual=True)
        regrid_ref.same_bits(sums, ref['sums'], 'sums')
        np.testing.assert_array_equal(counts, ref['counts'])
        regrid_ref.same_bits(resid, ref['resid'], 'resid')
        sums2, counts2, none = r.consistency_sums(case['x'], case['ref'])             # without the residual; a repeated call
        assert none is None
        regrid_ref.same_bits(sums2, ref['sums'], 'sums again')
        np.testing.assert_array_equal(counts2, ref['counts'])
    finally:
        r.close()


@pytest.mark.parametrize('name', ['cons_64x96_17x23_c3', 'cons_descending_lat', 'bilinear_3x4_7x9_nan_outside', 'wide_bilinear_520'])
def test_calling_paths_give_the_same_bits(name):
    """a host array in two chunks and in one, a DeviceArray, and N = 3 against three calls of N = 1"""
    from dl4ds_amd.device import DeviceArray
    case, ref = reference(name)
    x, y = case['x'], case['ref']
    assert x.shape[0] == 3
    r = regridder(case)
    try:
        for bs in (2, 3, None):
            regrid_ref.same_bits(r.transform(x, batch_size=bs), ref['out'], f'batch_size {bs}')
            sums, counts, resid = r.consistency_sums(x, y, return_residual=True, batch_size=bs)
            regrid_ref.same_bits(sums, ref['sums'])
            regrid_ref.same_bits(resid, ref['resid'])
            np.testing.assert_array_equal(counts, ref['counts'])
        dx, dy = DeviceArray.from_numpy(x), DeviceArray.from_numpy(y)
        dout = r.transform(dx)
        assert isinstance(dout, DeviceArray) and dout.shape == ref['out'].shape
        regrid_ref.same_bits(dout.numpy(), ref['out'], 'device array')
        sums, counts, resid = r.consistency_sums(dx, dy, return_residual=True)
        regrid_ref.same_bits(sums, ref['sums'])
        regrid_ref.same_bits(resid, ref['resid'])
        for n in range(3):
            regrid_ref.same_bits(r.transform(x[n:n + 1]), ref['out'][n:n + 1], f'sample {n} alone')
            s1, c1, _ = r.consistency_sums(x[n:n + 1], y[n:n + 1])
            regrid_ref.same_bits(s1, ref['sums'][n:n + 1])
            np.testing.assert_array_equal(c1, ref['counts'][n:n + 1])
        for d in (dx, dy, dout):
            d.free()
    finally:
        r.close()


@pytest.mark.parametrize('name', ['cons_96x64_23x17_c4', 'nearest_3x4_7x9', 'cons_descending_lat'])
def test_four_byte_form_on_unaligned_pointers(name):
    """C = 4 takes the 16-byte form on aligned buffers (every other test); pointers that are only 4-byte aligned take the 4-byte
    form and give the same bits"""
    import dl4ds_amd._lib as L
    from dl4ds_amd.device import Buffers, sync
    case, ref = reference(name)
    x = case['x']
    N, H, W, C = x.shape
    assert C % 4 == 0
    r = regridder(case)
    try:
        with Buffers() as buf:
            flat = np.ascontiguousarray(x).reshape(-1)
            aligned, shifted, dout = buf.alloc((x.size,)), buf.alloc((x.size + 1,)), buf.zeros((ref['out'].size + 1,))
            aligned.upload(flat)
            shifted.upload(flat, 1)
            for xp, oo in ((shifted.ptr + 4, 1), (aligned.ptr, 1), (shifted.ptr + 4, 0)):
                L.check(L.lib().dl4ds_regrid_apply(r._handle(), xp, N, C, int(r.skipna), r.min_valid, dout.ptr + 4 * oo))
                sync()
                got = np.empty(ref['out'].shape, np.float32)
                dout.download(got, oo)
                regrid_ref.same_bits(got, ref['out'], (xp % 16, oo))
    finally:
        r.close()


def test_one_call_form_and_exact_refinement():
    import dl4ds_amd as dds
    case, ref = reference('periodic_seam_6_4')
    regrid_ref.same_bits(dds.regrid(case['x'], case['src_lat'], case['src_lon'], case['dst_lat'], case['dst_lon'], **case['kw']), ref['out'])
    lr = (np.random.default_rng(6).standard_normal((2, 3, 5, 2)) * 10 + 280).astype(np.float32)
    hr = lr.repeat(4, axis=1).repeat(4, axis=2)
    res = dds.consistency_scores(lr, hr, scale=4, return_residual=True)
    assert (res['max_abs'] == 0).all() and (res['bias'] == 0).all() and (res['n_valid'] == 15).all() and (res['residual'] == 0).all()
    mask = np.ones((3, 5))
    mask[1, 2] = 0
    res = dds.consistency_scores(lr, hr + np.float32(0.5), scale=4, mask=mask, batch_size=1)
    assert (res['n_valid'] == 14).all() and (res['n_mismatch'] == 1).all() and (res['max_abs'] == 0.5).all()
    assert (res['bias'] == 0.5).all() and (res['bias_pooled'] == 0.5).all()


def _tables():
    return dict(yptr=np.array([0, 2, 4], np.int32), yidx=np.array([0, 1, 2, 3], np.int32), yw=np.ones(4),
                xptr=np.array([0, 1, 2], np.int32), xidx=np.array([0, 1], np.int32), xw=np.ones(2), ay=np.ones(2), ax=np.ones(2))


def _create(H=4, W=2, Ho=2, Wo=2, **change):
    import dl4ds_amd._lib as L
    t = dict(_tables(), **change)
    keep = [None if t[k] is None else np.ascontiguousarray(t[k]) for k in ('yptr', 'yidx', 'yw', 'xptr', 'xidx', 'xw', 'ay', 'ax')]
    h = ctypes.c_void_p()
    st = L.lib().dl4ds_regrid_plan_create(H, W, Ho, Wo, *(None if a is None else a.ctypes.data for a in keep), ctypes.byref(h))
    return st, h.value


@pytest.mark.parametrize('change', [dict(yptr=np.array([1, 2, 4], np.int32)), dict(xptr=np.array([0, 2, 1], np.int32)),
                                    dict(yidx=np.array([0, 1, 2, 4], np.int32)), dict(xidx=np.array([-1, 1], np.int32)),
                                    dict(yw=np.array([1.0, -1.0, 1.0, 1.0])), dict(xw=np.array([np.nan, 1.0])),
                                    dict(xw=np.array([np.inf, 1.0])), dict(ay=np.array([1.0, np.nan])), dict(ax=None), dict(yptr=None),
                                    dict(H=0), dict(Wo=0), dict(H=1 << 16, W=1 << 15)])
def test_plan_create_refusals(change):
    import dl4ds_amd._lib as L
    sizes = {k: change.pop(k) for k in list(change) if k in ('H', 'W', 'Ho', 'Wo')}
    st, h = _create(**sizes, **change)
    assert st != 0 and not h and b'regrid_plan_create' in L.lib().dl4ds_last_error()


def test_call_refusals():
    import dl4ds_amd._lib as L
    from dl4ds_amd.device import Buffers, sync
    lib = L.lib()
    st, plan = _create()
    assert st == 0 and plan
    with Buffers() as buf:
        x, out, ref = buf.zeros((1, 4, 2, 1)), buf.zeros((1, 2, 2, 1)), buf.zeros((1, 2, 2, 1))
        sums, counts = buf.zeros((1, 1, 6), np.float64), buf.zeros((1, 1, 2), np.int64)
        good = (plan, x.ptr, 1, 1, 0, 0.5, out.ptr)
        assert lib.dl4ds_regrid_apply(*good) == 0
        cgood = (plan, x.ptr, ref.ptr, 1, 1, 0, 0.5, sums.ptr, counts.ptr, None)
        assert lib.dl4ds_regrid_consistency(*cgood) == 0
        sync()
        for k, v in ((0, None), (1, None), (6, None), (6, x.ptr), (2, 0), (3, 0), (2, -1), (5, -0.01), (5, 1.01), (5, float('nan'))):
            bad = list(good)
            bad[k] = v
            assert lib.dl4ds_regrid_apply(*bad) != 0 and b'regrid_apply' in lib.dl4ds_last_error(), (k, v)
        for k, v in ((0, None), (1, None), (2, None), (7, None), (8, None), (3, 0), (4, 0), (6, 2.0), (6, float('nan'))):
            bad = list(cgood)
            bad[k] = v
            assert lib.dl4ds_regrid_consistency(*bad) != 0 and b'regrid_consistency' in lib.dl4ds_last_error(), (k, v)
        assert lib.dl4ds_regrid_plan_destroy(plan) == 0
        assert lib.dl4ds_regrid_apply(*good) != 0 and b'destroyed' in lib.dl4ds_last_error()
        assert lib.dl4ds_regrid_consistency(*cgood) != 0 and lib.dl4ds_regrid_plan_destroy(plan) != 0
        assert lib.dl4ds_regrid_plan_destroy(None) != 0
        sync()                                                           # nothing was launched by a refused call: the stream is clean
