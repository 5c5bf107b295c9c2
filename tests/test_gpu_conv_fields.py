"""The convolution kernels below the 2e-4 bar of the op tests: exact fields, power-of-two scaling and field classes, per kernel
family of tests/conv_view_cases.py plus F(4x4) Winograd (tests/conv_field_cases.py holds the fields, references and emulations;
tests/test_conv_field_cases.py the conditions under which these tests mean what they say).

1. Integer fields (half zeros, a 0/1 coast mask, integer filters / bias / residual / accumulation target, +-1 mask): forward forms
   0, 3, 12, 15, the dgrad in forms 12 (through conv2d_epilogue on the flipped filter -- ops.conv2d_dgrad takes no mask) and 8
   (ops.conv2d_dgrad), dw and db plain and accumulated: np.array_equal with the int64 reference, and the family's kernel tag.
2. x * 2^a, w * 2^b, b / add / old * 2^(a+b): the same bits as ldexp(unscaled result, a + b) and the same kernel tags.
3. white / offset / smooth / sparse / channel_scales fields: E = max |got - ref64| / S per element against the float32 emulation's,
   E_kernel <= 4 E_emul + 2^-24; exact equality where S == 0.

Measured on an MI355X: E_kernel / E_emul per (family, class), each the largest over the forms run (forward 0 and 3 and the dgrad;
dw and db); every figure in units of 1e-7; in brackets the largest E_kernel / (4 E_emul + 2^-24) of the row (the bar is 1):
  family       white          offset         smooth         sparse         channel_scales 
  direct_3_1   1.28 / 1.4     2.12 / 2.1     1.06 / 1.0     1.03 / 1.2     2.69 / 2.3     [0.28]
  direct_1_3   1.67 / 1.7     1.48 / 1.5     1.01 / 1.0     1.12 / 1.1     1.92 / 1.8     [0.25]
  direct_8_1   1.71 / 2.0     1.94 / 1.9     1.33 / 1.7     1.29 / 1.8     2.63 / 2.6     [0.24]
  pair_8_8     2.72 / 2.5     1.84 / 2.4     1.95 / 1.8     2.27 / 2.3     4.06 / 4.2     [0.35]
  pair_5_8     2.03 / 2.4     1.39 / 1.4     2.05 / 2.3     1.93 / 2.3     3.65 / 4.4     [0.32]
  narrow16     2.29 / 2.6     1.72 / 1.7     1.80 / 1.9     2.62 / 2.1     4.04 / 4.2     [0.29]
  pair16       2.38 / 2.4     2.04 / 2.5     1.53 / 1.5     1.77 / 2.1     5.17 / 4.5     [0.36]
  stream       3.81 / 2.9     2.02 / 2.1     1.59 / 1.8     2.56 / 3.1     5.84 / 5.8     [0.32]
  stream_ws    2.64 / 2.8     2.55 / 2.1     1.77 / 1.6     3.29 / 2.8     4.26 / 6.3     [0.29]
  wino_24_32   1.14 / 1.1     1.13 / 1.0     1.03 / 1.0     6.75 / 10.7    3.88 / 2.3     [0.40]
  wino_28_36   1.41 / 1.3     1.13 / 1.3     1.42 / 1.0     29.90 / 23.1   2.33 / 2.3     [0.35]
  split        0.74 / 3.1     0.54 / 2.4     0.68 / 2.1     3.20 / 3.7     2.57 / 6.8     [0.21]
  gemm         1.07 / 2.7     0.83 / 2.2     0.74 / 1.9     1.76 / 2.7     3.16 / 6.3     [0.16]
  point        2.12 / 2.1     1.95 / 2.0     2.04 / 1.9     1.41 / 1.5     1.79 / 1.7     [0.25]
  igemm3       1.78 / 2.5     1.49 / 2.0     1.04 / 1.9     3.20 / 3.5     3.92 / 6.0     [0.27]
  igemm5       1.54 / 1.8     0.98 / 1.2     0.93 / 1.5     1.48 / 2.5     2.74 / 3.9     [0.28]
  igemm7       1.29 / 1.9     1.50 / 1.6     0.92 / 1.7     1.29 / 1.9     1.76 / 4.3     [0.22]
  stream_d2s   3.25 / 2.6     1.92 / 2.0     2.96 / 2.1     2.97 / 4.6     6.91 / 6.5     [0.35]
  wg_general_1 0.11 / 1.5     3.70 / 60.0    4.14 / 60.5    4.18 / 13.1    0.12 / 1.6     [0.17]
  wg_general_3 0.36 / 2.7     2.43 / 20.8    2.31 / 19.7    2.08 / 3.9     0.31 / 2.5     [0.18]
  wg_general_5 0.31 / 1.6     1.50 / 12.3    1.45 / 10.5    1.41 / 1.9     0.33 / 1.7     [0.23]
  wg_direct    0.12 / 0.6     1.19 / 7.3     0.95 / 7.4     0.85 / 1.2     0.16 / 0.5     [0.16]
  wg_direct2   0.09 / 1.0     1.58 / 15.0    1.67 / 14.7    1.63 / 2.0     0.12 / 0.7     [0.19]
  wg_narrow8   0.19 / 2.2     2.04 / 26.7    2.22 / 30.1    1.92 / 4.9     0.27 / 1.3     [0.16]
  wg_two_slice 0.31 / 1.1     2.35 / 19.4    2.28 / 15.7    1.62 / 2.0     0.41 / 1.6     [0.19]
  wg_rows      0.51 / 1.9     2.62 / 13.6    2.13 / 12.8    1.74 / 2.2     0.59 / 1.8     [0.21]
  wg_wino      0.61 / 1.4     2.29 / 9.3     2.35 / 10.4    379.00 / 685.0 0.50 / 1.6     [0.17]
  wg_d2s       0.58 / 3.1     3.49 / 22.8    3.54 / 26.0    2.91 / 5.5     0.55 / 2.7     [0.22]
No family was inexact under part 1, none changed a bit under part 2, none exceeded the bar under part 3, and every element with S == 0
(direct_1_3 / direct_3_1 / direct_8_1 sparse forward and dgrad, wg_rows sparse) equalled the reference; no defect was found in the
kernels.  wino_* / wg_wino on sparse fields: where S is small but the tile's other taps are not, F(2x2,3x3) cancels to rounding of the
larger sums -- the emulation shows the same figures (conv_field_cases: the correction for the `wino` weight gradient).
Wall time of the module: 12.7 s (85 tests; the slowest, wg_d2s field classes, 6.1 s of float32 emulation on the CPU, every other below 0.8 s).
"""
import numpy as np
import pytest

from oracle import np_ops as N
from tests import conv_field_cases as CF
from tests import conv_view_cases as CV

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def ops():
    import dl4ds_amd.ops as o
    return o


def set_env(monkeypatch, fam):
    for k in CF.ENV_KEYS:
        monkeypatch.delenv(k, raising=False)
    for k, v in fam.env.items():
        monkeypatch.setenv(k, v)


def conv_tags(tags):
    return sorted(t for t in tags if t.startswith('conv_'))


def ran(tags, want):
    return any(t.startswith(want) for t in tags)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _s2d(y, r):
    n, hh, ww, cp = y.shape
    return y.reshape(n, hh // r, r, ww // r, r, cp).transpose(0, 1, 3, 2, 4, 5).reshape(n, hh // r, ww // r, r * r * cp)


def _d2s(a, r):
    return np.ascontiguousarray(N.depth_to_space(a, r))


# ---- the calls: dense operands, (result, conv tags) -------------------------------------------------------------------------------
def call_fwd(ops, fam, d, epi, bias=True):
    """forward form `epi` (bit 0 residual, 1 ReLU, 2 mask, 3 accumulate) through ops.conv2d_epilogue; the family that stores through
    depth_to_space has no such entry and goes through conv2d_views with dense depth_to_space views"""
    from tests.parity import kernel_tags
    b = d['b'] if bias else None
    add, mask, old = (d['add'] if epi & 1 else None), (d['mask'] if epi & 4 else None), (d['old'] if epi & 8 else None)
    if not fam.d2s:
        got, tags = kernel_tags(lambda: ops.conv2d_epilogue(d['x'], d['w'], b, add=add, mask=mask, relu=bool(epi & 2), accumulate_into=old))
        return got, conv_tags(tags)
    r, co = fam.d2s[1], fam.shape[4]
    n, h, w = d['x'].shape[:3]
    view = lambda a: None if a is None else ops.View(_d2s(a, r), C=co, d2s=r)
    y = view(old if old is not None else np.zeros((n, h, w, co), np.float32))
    bufs, tags = kernel_tags(lambda: ops.conv2d_views(ops.View(d['x']), d['w'], y, b=b, add=view(add), mask=view(mask), relu=bool(epi & 2),
                                                      accumulate=bool(epi & 8)))
    return np.ascontiguousarray(_s2d(bufs['y'][0], r)), conv_tags(tags)


def call_dgrad(ops, fam, dz, w, mask=None, old=None):
    """dx = [old +] [where(mask > 0,] dgrad(dz, w) [, 0)]: ops.conv2d_dgrad; with a mask, the same convolution through
    ops.conv2d_epilogue on the flipped filter (conv2d_views(dgrad=True) for the depth_to_space family)"""
    from tests.parity import kernel_tags
    r = fam.d2s[1] if fam.d2s else 0
    if mask is None:
        got, tags = kernel_tags(lambda: ops.conv2d_dgrad(_d2s(dz, r) if r else dz, w, d2s=r, accumulate_into=old))
    elif not r:
        got, tags = kernel_tags(lambda: ops.conv2d_epilogue(dz, CF.dgrad_filter(w), mask=mask, accumulate_into=old))
    else:
        y = ops.View(old if old is not None else np.zeros(mask.shape, np.float32))
        bufs, tags = kernel_tags(lambda: ops.conv2d_views(ops.View(_d2s(dz, r), C=dz.shape[-1], d2s=r), w, y, mask=ops.View(mask),
                                                          accumulate=old is not None, dgrad=True))
        got = bufs['y'][0]
    return got, conv_tags(tags)


def call_wgrad(ops, fam, x, dz, dw0=None, db0=None):
    """dz in logical layout -> (dw, db, conv tags) of conv2d_wgrad_views on dense views (the entry point that returns db)"""
    from tests.parity import kernel_tags
    r = fam.d2s[1] if fam.d2s else 0
    dzv = ops.View(_d2s(dz, r) if r else dz, C=dz.shape[-1], d2s=r)
    (dw, db, _), tags = kernel_tags(lambda: ops.conv2d_wgrad_views(ops.View(x), dzv, fam.shape[5], dw0=dw0, db0=db0))
    return dw, db, conv_tags(tags)


# ---- 1. exact fields ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('fam', CF.FWD, ids=lambda f: f.name)
def test_exact_fields_forward_and_dgrad(ops, monkeypatch, fam):
    set_env(monkeypatch, fam)
    d = CF.exact_fwd(fam.name)
    for epi in CF.EXACT_FORMS:
        got, tags = call_fwd(ops, fam, d, epi)
        want = fam.epi_tags.get(epi, fam.tag)
        assert ran(tags, want), (fam.name, epi, want, tags)
        ref = CF.epilogue(d['conv'], d, epi)
        assert np.array_equal(got, ref), f'{fam.name} form {epi} ({tags}): {int((got != ref).sum())} of {ref.size} elements differ, max {np.abs(got - ref).max()}'
    g = CF.exact_dgrad(fam.name)
    for form, mask in ((12, g['mask']), (8, None)):
        got, tags = call_dgrad(ops, fam, g['dz'], g['w'], mask=mask, old=g['old'])
        assert ran(tags, CF.dgrad_tag(fam)), (fam.name, 'dgrad', form, tags)
        ref = (np.where(mask > 0, g['conv'], 0) if mask is not None else g['conv']) + g['old'].astype(np.int64)
        assert np.array_equal(got, ref), f'{fam.name} dgrad form {form} ({tags}): {int((got != ref).sum())} of {ref.size} elements differ'


@pytest.mark.parametrize('fam', CF.WG, ids=lambda f: f.name)
def test_exact_fields_wgrad(ops, monkeypatch, fam):
    set_env(monkeypatch, fam)
    d = CF.exact_wgrad(fam.name)
    r = fam.d2s[1] if fam.d2s else 0
    for dw0, db0 in ((None, None), (d['dw0'], d['db0'])):
        dw, db, tags = call_wgrad(ops, fam, d['x'], d['dz'], dw0, db0)
        assert ran(tags, fam.tag), (fam.name, tags)
        rw = d['dw'] + (0 if dw0 is None else dw0.astype(np.int64))
        rb = d['db'] + (0 if db0 is None else db0.astype(np.int64))
        assert np.array_equal(dw, rw), f'{fam.name} dw ({tags}): {int((dw != rw).sum())} of {rw.size} elements differ, max {np.abs(dw - rw).max()}'
        assert np.array_equal(db, rb), f'{fam.name} db ({tags}): {db - rb}'
        one = ops.conv2d_wgrad(d['x'], _d2s(d['dz'], r) if r else d['dz'], fam.shape[5], d2s=r, accumulate_into=dw0)
        assert np.array_equal(one, rw), f'{fam.name} conv2d_wgrad'


# ---- 2. power-of-two scaling --------------------------------------------------------------------------------------------------------
def _scaled(d, a, b, data, filt, both):
    out = dict(d)
    for keys, k in ((data, a), (filt, b), (both, a + b)):
        for key in keys:
            out[key] = CF.scaled(d[key], k)
    return out


@pytest.mark.parametrize('fam', CF.FWD + [CF.F44], ids=lambda f: f.name)
def test_scaling_forward_and_dgrad(ops, monkeypatch, fam):
    set_env(monkeypatch, fam)
    d, g = CF.scale_fwd(fam.name), CF.scale_dgrad(fam.name)
    base = {epi: call_fwd(ops, fam, d, epi) for epi in (0, 15)}
    assert ran(base[0][1], fam.tag) and ran(base[15][1], fam.epi_tags.get(15, 'conv_' if fam is CF.F44 else fam.tag)), (fam.name, base[0][1], base[15][1])
    gbase = call_dgrad(ops, fam, g['dz'], g['w'], old=g['old'])
    assert ran(gbase[1], CF.dgrad_tag(fam)), (fam.name, gbase[1])
    for a, b in CF.SCALES:
        ds = _scaled(d, a, b, ('x',), ('w',), ('b', 'add', 'old'))
        for epi in (0, 15):
            got, tags = call_fwd(ops, fam, ds, epi)
            assert tags == base[epi][1], (fam.name, epi, a, b, tags, base[epi][1])
            diff = bits(got) != bits(CF.scaled(base[epi][0], a + b))
            assert not diff.any(), f'{fam.name} form {epi} x 2^{a} w 2^{b} ({tags}): {int(diff.sum())} of {diff.size} elements are not the scaled bits'
        gs = _scaled(g, a, b, ('dz',), ('w',), ('old',))
        got, tags = call_dgrad(ops, fam, gs['dz'], gs['w'], old=gs['old'])
        assert tags == gbase[1], (fam.name, 'dgrad', a, b, tags, gbase[1])
        diff = bits(got) != bits(CF.scaled(gbase[0], a + b))
        assert not diff.any(), f'{fam.name} dgrad dz 2^{a} w 2^{b} ({tags}): {int(diff.sum())} of {diff.size} elements are not the scaled bits'


@pytest.mark.parametrize('fam', CF.WG, ids=lambda f: f.name)
def test_scaling_wgrad(ops, monkeypatch, fam):
    """dw scales by 2^(a+b), db = sum dz by 2^b; plain and accumulated into dw0 * 2^(a+b), db0 * 2^b"""
    set_env(monkeypatch, fam)
    d = dict(CV.wgrad_case(fam.name))
    if fam.d2s:
        d['dz'] = _s2d(d['dz'], fam.d2s[1])                       # (the case holds dz in memory layout; call_wgrad takes the logical one)
    for acc in (False, True):
        pick = lambda dd: (dd['dw0'], dd['db0']) if acc else (None, None)
        dw, db, tags = call_wgrad(ops, fam, d['x'], d['dz'], *pick(d))
        assert ran(tags, fam.tag), (fam.name, tags)
        for a, b in CF.SCALES:
            ds = _scaled(_scaled(d, a, b, ('x',), ('dz',), ('dw0',)), 0, b, (), ('db0',), ())
            sw, sb, stags = call_wgrad(ops, fam, ds['x'], ds['dz'], *pick(ds))
            assert stags == tags, (fam.name, a, b, stags, tags)
            dif_w, dif_b = bits(sw) != bits(CF.scaled(dw, a + b)), bits(sb) != bits(CF.scaled(db, b))
            assert not dif_w.any() and not dif_b.any(), \
                f'{fam.name} acc {acc} x 2^{a} dz 2^{b} ({tags}): {int(dif_w.sum())} of {dif_w.size} dw, {int(dif_b.sum())} of {dif_b.size} db elements are not the scaled bits'


# ---- 3. field classes ------------------------------------------------------------------------------------------------------------------
def judge(rows, what, got, j):
    e, zeros = CF.stat(got, j['ref'], j['S'], j.get('S0'))
    print(f'FIELDS {what:44s} E_kernel {e:.2e}  E_emul {j["e_emul"]:.2e}  bar {CF.bar(j["e_emul"]):.2e}  S==0 {int((j["S"] == 0).sum())}')
    if zeros:
        rows.append(f'{what}: {zeros} elements with S == 0 differ from the reference')
    if not e <= CF.bar(j['e_emul']):
        rows.append(f'{what}: E_kernel {e:.3e} > 4 * {j["e_emul"]:.3e} + 2^-24')


@pytest.mark.parametrize('fam', CF.FWD, ids=lambda f: f.name)
def test_field_classes_forward_and_dgrad(ops, monkeypatch, fam):
    set_env(monkeypatch, fam)
    bad = []
    for cls in CF.CLASSES:
        d, j = CF.fields_fwd(fam.name, cls), CF.fwd_judge(fam.name, cls)
        for epi in (0, 3):
            got, tags = call_fwd(ops, fam, d, epi, bias=bool(epi))
            assert ran(tags, fam.epi_tags.get(epi, fam.tag)), (fam.name, cls, epi, tags)
            judge(bad, f'{fam.name} {cls} form {epi}', got, j[epi])
        g = CF.fields_dgrad(fam.name, cls)
        got, tags = call_dgrad(ops, fam, g['dz'], g['w'])
        assert ran(tags, CF.dgrad_tag(fam)), (fam.name, cls, 'dgrad', tags)
        judge(bad, f'{fam.name} {cls} dgrad', got, CF.dgrad_judge(fam.name, cls))
    assert not bad, '\n'.join(bad)


@pytest.mark.parametrize('fam', CF.WG, ids=lambda f: f.name)
def test_field_classes_wgrad(ops, monkeypatch, fam):
    set_env(monkeypatch, fam)
    bad = []
    for cls in CF.CLASSES:
        d, j = CF.fields_wgrad(fam.name, cls), CF.wgrad_judge(fam.name, cls)
        dw, db, tags = call_wgrad(ops, fam, d['x'], d['dz'])
        assert ran(tags, fam.tag), (fam.name, cls, tags)
        judge(bad, f'{fam.name} {cls} dw', dw, j['dw'])
        judge(bad, f'{fam.name} {cls} db', db, j['db'])
    assert not bad, '\n'.join(bad)
