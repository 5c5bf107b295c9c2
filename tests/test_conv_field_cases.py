"""CPU tests of tests/conv_field_cases.py: the references, the emulations and the four conditions under which the GPU tests of
tests/test_gpu_conv_fields.py mean what they say -- exactness of the integer fields, the range of the power-of-two scalings, a
narrower type being visible at the bar, another summation order staying inside it."""
import numpy as np
import pytest

from oracle import np_ops as N
from tests import conv_field_cases as CF
from tests import conv_view_cases as CV

FWD_NAMES = [f.name for f in CF.FWD]
WG_NAMES = [f.name for f in CF.WG]
NARROW_SHAPES = ('split', 'stream', 'wino_24_32', 'gemm')


def test_every_family_of_the_view_table_is_covered():
    assert set(FWD_NAMES + WG_NAMES) == {f.name for f in CV.FAMILIES} and CF.F44.name not in FWD_NAMES
    assert CF.F44.shape[:5] in __import__('tests.test_gpu_ops', fromlist=['F44_CASES']).F44_CASES
    assert not CF.NOT_EXACT


# ---- references ---------------------------------------------------------------------------------------------------------------------
def test_references_agree_with_the_oracle():
    for name in ('pair_5_8', 'igemm5', 'point'):
        d = CV.fwd_case(name)
        np.testing.assert_allclose(CF.conv_any(d['x'].astype(np.float64), d['w'].astype(np.float64)) + d['b'], d['conv64'], rtol=0, atol=1e-12)
        for epi in range(16):
            np.testing.assert_array_equal(CF.epilogue(d['conv64'] - d['b'].astype(np.float64), d, epi), CV.fwd_reference(d, epi))
        g = CV.dgrad_case(name)
        ref = np.where(g['mask'] > 0, CF.conv_any(g['dz'].astype(np.float64), CF.dgrad_filter(g['w']).astype(np.float64)), 0.0) + g['old']
        np.testing.assert_allclose(ref, g['ref'], rtol=0, atol=1e-12)
    for name in ('wg_general_5', 'wg_rows'):
        d = CV.wgrad_case(name)
        dw, db = CF.wgrad_any(d['x'].astype(np.float64), d['dz'].astype(np.float64), CV.family(name).shape[5])
        np.testing.assert_allclose(dw, d['dw64'], rtol=0, atol=1e-10)
        np.testing.assert_allclose(db, d['db64'], rtol=0, atol=1e-10)


def test_emulations_compute_the_convolution():
    g = np.random.default_rng(5)
    x, w, dz = g.standard_normal((2, 7, 9, 5)), 0.2 * g.standard_normal((3, 3, 5, 6)), g.standard_normal((2, 7, 9, 6))
    ref = N.conv2d(x, w)
    for got in (CF.emul_sum_conv(x, w), CF.emul_sum_conv(x, w, 'blocked'), CF.emul_wino_conv(x, w)):
        assert got.dtype == np.float32 and np.abs(got - ref).max() < 2e-6
    dw, db = CF.wgrad_any(x, dz, 3)
    for gw, gb in (CF.emul_sum_wgrad(x, dz, 3), CF.emul_sum_wgrad(x, dz, 3, 'blocked'), CF.emul_wino_wgrad(x, dz)):
        assert gw.dtype == np.float32 and np.abs(gw - dw).max() < 2e-5 and np.abs(gb - db).max() < 2e-5
    assert np.array_equal(CF.truncate16(np.float32([1 + 2.0 ** -15, 1 + 2.0 ** -16, -3.0])), np.float32([1 + 2.0 ** -15, 1, -3.0]))


# ---- part 1: the exactness condition ----------------------------------------------------------------------------------------------------
def _is_int_field(a, amp):
    return np.array_equal(a, np.round(a)) and np.abs(a).max() <= amp


@pytest.mark.parametrize('name', FWD_NAMES)
def test_exact_fields_forward_and_dgrad(name):
    """4 max(|x| (*) |w| + |b| + |add| + |old|) < 2^24, the fields are what part 1 asks for, and float32 arithmetic in two other
    orders (blocked sums, F(2x2,3x3)) reproduces the int64 reference bit for bit"""
    d, g = CF.exact_fwd(name), CF.exact_dgrad(name)
    assert 4 * d['bound'] < 2 ** 24 and 4 * g['bound'] < 2 ** 24
    assert _is_int_field(d['x'], 3) and _is_int_field(d['w'], 2) and _is_int_field(g['dz'], 3)
    assert all(_is_int_field(d[k], 4) for k in ('b', 'add', 'old')) and set(np.unique(d['mask'])) == {-1.0, 1.0}
    for f in (d['x'], g['dz']):
        assert 0.35 < (f[..., -1] == 0).mean() < 0.75
        if f.shape[-1] > 1:
            coast = f[0, :, :, 0]
            assert set(np.unique(coast)) == {0.0, 1.0} and (np.diff(coast, axis=1) >= 0).all() and (np.diff(coast, axis=0) >= 0).all()
    np.testing.assert_array_equal(CF.emul_sum_conv(d['x'], d['w'], 'blocked'), d['conv'])
    if d['w'].shape[0] == 3:
        np.testing.assert_array_equal(CF.emul_wino_conv(d['x'], d['w']), d['conv'])
        np.testing.assert_array_equal(CF.emul_wino_conv(g['dz'], CF.dgrad_filter(g['w'])), g['conv'])


@pytest.mark.parametrize('name', WG_NAMES)
def test_exact_fields_wgrad(name):
    """4 max(sum_pixels |x||dz| + |dw0|) < 2^24 (and the same for db); float32 sums in another order give the int64 reference"""
    d = CF.exact_wgrad(name)
    assert 4 * d['bound'] < 2 ** 24
    assert _is_int_field(d['x'], 3) and _is_int_field(d['dz'], 3) and _is_int_field(d['dw0'], 4) and _is_int_field(d['db0'], 4)
    ks = CF.family(name).shape[5]
    dw, db = CF.emul_sum_wgrad(d['x'], d['dz'], ks, 'blocked')
    np.testing.assert_array_equal(dw, d['dw'])
    np.testing.assert_array_equal(db, d['db'])
    if ks == 3:
        dw, db = CF.emul_wino_wgrad(d['x'], d['dz'])
        np.testing.assert_array_equal(dw, d['dw'])
        np.testing.assert_array_equal(db, d['db'])


# ---- part 2: the range condition ------------------------------------------------------------------------------------------------------
LO, HI = 2.0 ** -100, 2.0 ** 100


@pytest.mark.parametrize('name', FWD_NAMES + [CF.F44.name])
def test_scaling_stays_in_range_forward_and_dgrad(name):
    d, g = CF.scale_fwd(name), CF.scale_dgrad(name)
    conv = d['conv64'] - d['b'].astype(np.float64)
    outs = [CV.fwd_reference(d, 0), CV.fwd_reference(d, 15), conv]
    for a, b in CF.SCALES:
        lo, hi = CF.scaling_range((d['x'], d['w']), (d['b'], d['add'], d['old']), outs, a, b)
        assert LO < lo and hi < HI, (name, a, b, lo, hi)
        lo, hi = CF.scaling_range((g['dz'], g['w']), (g['old'],), (g['ref'], g['ref'] - g['old']), a, b)
        assert LO < lo and hi < HI, (name, 'dgrad', a, b, lo, hi)


@pytest.mark.parametrize('name', WG_NAMES)
def test_scaling_stays_in_range_wgrad(name):
    d = CV.wgrad_case(name)
    for a, b in CF.SCALES:
        lo, hi = CF.scaling_range((d['x'], d['dz']), (d['dw0'],), (d['dw64'], d['dw64'] + d['dw0']), a, b)
        assert LO < lo and hi < HI, (name, a, b, lo, hi)
        # db = sum dz carries 2^b alone
        lo, hi = CF.scaling_range((np.float32([1.0]), d['dz']), (d['db0'],), (d['db64'], d['db64'] + d['db0']), 0, b)
        assert LO < lo and hi < HI, (name, 'db', b, lo, hi)


def test_the_emulations_scale_exactly():
    """the identity of part 2 holds for float32 arithmetic in any order: shown on the emulations themselves"""
    d = CF.scale_fwd('pair16')
    base_s, base_w = CF.emul_sum_conv(d['x'], d['w']), CF.emul_wino_conv(d['x'], d['w'])
    for a, b in CF.SCALES:
        xs, ws = CF.scaled(d['x'], a), CF.scaled(d['w'], b)
        np.testing.assert_array_equal(CF.emul_sum_conv(xs, ws).view(np.uint32), CF.scaled(base_s, a + b).view(np.uint32))
        np.testing.assert_array_equal(CF.emul_wino_conv(xs, ws).view(np.uint32), CF.scaled(base_w, a + b).view(np.uint32))


# ---- part 3: the classes, and the two conditions on the bar -----------------------------------------------------------------------------
def test_field_classes_are_what_they_claim():
    g = np.random.default_rng(3)
    shape = (2, 40, 33, 8)
    off = CF.field('offset', shape, g)
    assert abs(off.mean() - 281) < 1 and 11 < off.std() < 13
    sm = CF.field('smooth', shape, g).astype(np.float64)
    assert 1.0 <= sm.min() and sm.max() <= 2.0                     # range 1 over the periodic grid, offset 1
    step = np.concatenate([np.abs(np.diff(sm, axis=1)).ravel(), np.abs(np.diff(sm, axis=2)).ravel()])
    assert 0.005 < step.mean() < 0.02, step.mean()                 # neighbours differ by about 1 % of the range
    sp = CF.field('sparse', shape, g)
    assert 0.88 < (sp == 0).mean() < 0.92 and (sp >= 0).all()
    cs = CF.field('channel_scales', (4, 40, 33, 8), g).astype(np.float64)
    np.testing.assert_allclose(np.log10(cs.std(axis=(0, 1, 2))), -3 + 6 * np.arange(8) / 7, atol=0.05)
    assert abs(CF.field('channel_scales', (2, 40, 33, 1), g).std() - 1) < 0.1
    w = CF.fields_fwd('pair_8_8', 'channel_scales')['w'].astype(np.float64)
    np.testing.assert_allclose(np.log10(w.std(axis=(0, 1, 2)) / 0.2), -2 + 4 * np.arange(8) / 7, atol=0.15)
    assert (CF.fwd_judge('direct_1_3', 'sparse')[0]['S'] == 0).any()          # the S == 0 branch of the statistic is exercised


@pytest.mark.parametrize('cls', CF.CLASSES)
@pytest.mark.parametrize('name', NARROW_SHAPES)
def test_a_narrower_type_is_visible(name, cls):
    """condition 1: x truncated to 16 significant bits in the `sum` emulation exceeds the bar of the untruncated one"""
    d = CF.fields_fwd(name, cls)
    ref, S = CF.conv_any(d['x'].astype(np.float64), d['w'].astype(np.float64)), CF.conv_any(CF._abs64(d['x']), CF._abs64(d['w']))
    e_emul = CF.stat(CF.emul_sum_conv(d['x'], d['w']), ref, S)[0]
    e_trunc = CF.stat(CF.emul_sum_conv(CF.truncate16(d['x']), d['w']), ref, S)[0]
    print(f'NARROW {name:12s} {cls:15s} E_emul {e_emul:.2e} bar {CF.bar(e_emul):.2e} E_trunc {e_trunc:.2e}')
    assert e_trunc > CF.bar(e_emul), (e_trunc, e_emul)


@pytest.mark.parametrize('cls', CF.CLASSES)
@pytest.mark.parametrize('name', FWD_NAMES)
def test_another_order_stays_inside_forward(name, cls):
    """condition 2: 16 partial sums, then added, against the sequential order"""
    d = CF.fields_fwd(name, cls)
    ref, S = CF.conv_any(d['x'].astype(np.float64), d['w'].astype(np.float64)), CF.conv_any(CF._abs64(d['x']), CF._abs64(d['w']))
    e_seq, z0 = CF.stat(CF.emul_sum_conv(d['x'], d['w']), ref, S)
    e_blk, z1 = CF.stat(CF.emul_sum_conv(d['x'], d['w'], 'blocked'), ref, S)
    assert z0 == z1 == 0 and e_blk <= CF.bar(e_seq), (e_blk, e_seq)


@pytest.mark.parametrize('cls', CF.CLASSES)
@pytest.mark.parametrize('name', WG_NAMES)
def test_another_order_stays_inside_wgrad(name, cls):
    d = CF.fields_wgrad(name, cls)
    ks = CF.family(name).shape[5]
    j = CF.wgrad_judge(name, cls)
    seq = CF.emul_sum_wgrad(d['x'], d['dz'], ks)
    blk = CF.emul_sum_wgrad(d['x'], d['dz'], ks, 'blocked')
    for key, s, b in zip(('dw', 'db'), seq, blk):
        e_seq, z0 = CF.stat(s, j[key]['ref'], j[key]['S'])
        e_blk, z1 = CF.stat(b, j[key]['ref'], j[key]['S'])
        assert z0 == z1 == 0 and e_blk <= CF.bar(e_seq), (key, e_blk, e_seq)


def test_wino_wgrad_does_not_return_exact_zeros():
    """where x and dz never meet under a tap (S == 0) every `sum` order is exactly zero, F(2x2,3x3) is not: those elements are
    judged on the algorithm's own magnitude sum, which bounds S from above and is positive there"""
    j = CF.wgrad_judge('wg_wino', 'sparse')['dw']
    zero = j['S'] == 0
    assert zero.any() and (j['ref'][zero] == 0).all() and (j['emul'][zero] != 0).any()
    assert (j['S0'] >= j['S'] * (1 - 1e-12)).all() and (j['S0'][zero][j['emul'][zero] != 0] > 0).all()
    assert CF.stat(j['emul'], j['ref'], j['S'])[1] > 0 and CF.stat(j['emul'], j['ref'], j['S'], j['S0'])[1] == 0
