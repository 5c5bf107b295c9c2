"""The case table of tests/conv_view_cases.py is complete and its inputs are well posed (no GPU)."""
import numpy as np
import pytest

from oracle import np_ops as N
from tests import conv_view_cases as CV

GRID = [f for f in CV.FAMILIES if f.grid]


def test_every_cell_is_tabulated():
    """every (family, role, form) cell has an outcome; none is reasoned out (0 <= 10 % per family); refusals carry a message and
    every deviation from the family's own kernel carries a code-level reason"""
    assert {f.kind for f in GRID} == {'fwd', 'wgrad'}
    for fam in GRID:
        cells = fam.cells()
        for role in fam.roles:
            for form in CV.FORMS:
                assert (role, form) in cells
                kind, what = fam.outcome(role, form)
                assert kind in ('run', 'refused') and isinstance(what, str) and what
        assert ('all', 'dense') in cells and ('all', 'frame+slice4') in cells
        assert fam.outcomes == {} or fam.why, fam.name
        for form in ('slice1', 'frame'):
            assert sum(1 for r, f in cells if f == form) >= len(fam.roles), (fam.name, form)
        for cell in fam.bits_differ:
            assert 'bits' in fam.why and fam.outcome(*cell)[0] == 'run', (fam.name, cell)
        assert fam.shape[0] >= 2                                  # frame and affine forms need two images


def test_affine_is_run_or_refused_never_dropped():
    for fam in GRID:
        for role in fam.roles:
            for form in ('affine_s', 'affine_sh'):
                kind, what = fam.outcome(role, form)
                if kind == 'run':
                    assert role in ('x', 'dz')
                else:
                    assert what in (CV.R_ENTRY, CV.R_DIRECT, CV.R_CONV, CV.R_WGRAD, CV.R_DIRECT_WG, CV.R_NARROW)
    sc0, sh0 = CV.affine_of('affine_sh', 3, 8, 5)
    assert (np.abs(sc0[0] - sc0[1]) > 0.01).any() and (np.abs(sh0[1] - sh0[2]) > 0.01).any() and (sc0 >= 0.5).all()
    assert CV.affine_of('affine_s', 2, 4, 5)[1] is None and CV.affine_of('frame', 2, 4, 5) == (None, None)


@pytest.mark.parametrize('form', ('dense',) + CV.PLACEMENTS)
@pytest.mark.parametrize('c', [1, 8, 13])
def test_embed_extract_round_trip(form, c):
    mem = np.random.default_rng(c).standard_normal((2, 5, 7, c)).astype(np.float32)
    buf, kw = CV.embed(mem, form, 11)
    got, inside = CV.extract(buf, form, c)
    np.testing.assert_array_equal(got, mem)
    assert inside.sum() == mem.size and np.isfinite(buf).all()
    ld, coff, framed = CV.placement(form, c)
    assert buf.shape[-1] == ld and kw['coff'] == coff and (kw['t'] is not None) == framed == (buf.ndim == 5)
    if form != 'dense':
        assert (buf[~inside] != 0).all()                         # the neighbours are random, not zeros
    if form == 'tail':
        assert coff + c == ld                                    # nothing above the slice


@pytest.mark.parametrize('fam', [f for f in CV.FAMILIES if f.kind == 'fwd'], ids=lambda f: f.name)
def test_forward_references(fam):
    """dense reference == N.conv2d on the same arrays; no ReLU argument within KINK of zero in any case; nothing excluded"""
    kinds = [''] + [f for f in ('affine_s', 'affine_sh') if fam.grid and fam.outcome('x', f)[0] == 'run']
    for affine in kinds:
        d = CV.fwd_case(fam.name, affine)
        x64 = CV.logical(d['x'], d['sc'], d['sh'])
        ref = N.conv2d(x64, d['w'].astype(np.float64), d['b'].astype(np.float64))
        np.testing.assert_array_equal(d['conv64'], ref)
        assert not CV.kink_offenders(d['conv64'], d['add']).any()
        if not affine:
            np.testing.assert_array_equal(x64, d['x'].astype(np.float64))
            np.testing.assert_array_equal(CV.fwd_reference(d, 0), ref)
        full = CV.fwd_reference(d, 15)
        want = np.where(d['mask'] > 0, np.maximum(ref + d['add'], 0.0), 0.0) + d['old']
        np.testing.assert_array_equal(full, want)
        assert full.shape == d['old'].shape and np.isfinite(full).all()


@pytest.mark.parametrize('fam', [f for f in CV.FAMILIES if f.kind == 'wgrad'], ids=lambda f: f.name)
def test_wgrad_references(fam):
    """db = sum dz carries a per-channel offset of order one, so one slab of the sum is far above the comparison's bar"""
    d = CV.wgrad_case(fam.name)
    n, h, w, ci, co, ks = fam.shape
    assert d['dw64'].shape == (ks, ks, ci, co) and d['db64'].shape == (co,)
    assert (np.abs(d['db64']) > 0.3 * n * h * w).all()
    # the centre tap of dw is the plain pixel sum of x (x) dz
    dz = d['dz'] if not fam.d2s else None
    if dz is not None:
        centre = np.tensordot(d['x'].astype(np.float64), dz.astype(np.float64), axes=([0, 1, 2], [0, 1, 2]))
        np.testing.assert_allclose(d['dw64'][ks // 2, ks // 2], centre, rtol=1e-10, atol=1e-9)
