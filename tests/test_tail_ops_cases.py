"""The cases of tests/test_gpu_tail_ops.py, checked on the CPU: the committed seeds keep every ReLU pre-activation of the float64
reference outside the margin with nothing excluded, every ReLU has both branches populated, every reference gradient is non-zero,
and the rec_tail cases select the loops they are named for."""
import numpy as np
import pytest

from tests import tail_ops_cases as K
from tests import tail_ops_ref as R


def test_case_ids_are_unique_and_every_required_geometry_is_there():
    ids = [c.id for c in K.ALL_CASES]
    assert len(ids) == len(set(ids))
    geo = {c.id: K.rec_tail_geometry(c) for c in K.REC_TAIL_CASES}
    staged = [g for g in geo.values() if g['staged']]
    assert {g['nblk'] for g in staged} >= {1, 2, 9, 72}
    assert any(g['nblk'] > K.WSUM_GROUPS and g['G'] == K.WSUM_GROUPS for g in staged)            # the group stride loop
    assert any(g['G'] >= 8 and g['G'] % 8 for g in staged)                                       # unrolled loop plus its tail
    assert any(g['staged'] and g['T'] == 1 for g in geo.values()) and any(not g['staged'] and g['T'] == 1 for g in geo.values())
    plain = [g for g in geo.values() if not g['staged']]
    assert {g['HW'] for g in plain} >= {30, 255, 256, 257, 289, 120}
    assert max(g['samples_per_block'] for g in plain) >= 9
    for chans in K.REC_TAIL_SHAPES:                                                              # every combination in both forms
        tag = 'rt_%d_%d_%d_' % chans
        assert {geo[i]['staged'] for i in geo if i.startswith(tag)} == {True, False}
    assert min(k * k * ci * max(d, 1) ** 2 for k, d, ci, _, _ in K.FOLD_GEOMS) < 64                 # idle lanes in unfold_w2_kernel
    assert len(K.FOLDED_REFUSED) == 8 and all(c.raises for c in K.FOLDED_REFUSED)


@pytest.mark.parametrize('case', K.ALL_CASES, ids=lambda c: c.id)
def test_reference_is_clear_of_the_relu_kinks(case):
    d = K.make(case)
    ref = d['ref']
    for name, inside, pos in R.margin_report(ref['relus']):
        assert inside == 0, f'{name}: {inside} pre-activations within {R.DELTA} of zero'
        assert R.MIN_SIDE <= pos <= 1.0 - R.MIN_SIDE, f'{name}: {pos:.3f} of the elements are positive'
    assert np.abs(ref['y']).max() > 0
    for k, g in ref['grads'].items():
        assert np.abs(g).max() > 0, f'gradient of {k} is zero'
    for (spec, grad, _), g in zip(case.inputs, ref['dx']):
        assert g is not None and np.abs(g).max() > 0, f'gradient of input {spec} is zero'
    for k, g in ref['grads'].items():                      # non-zero biases
        if k.endswith('bias'):
            assert np.all(d['w'](k, g.shape) != 0)


@pytest.mark.parametrize('family', list(K.TABLES) + ['stale'])
def test_committed_seeds_are_what_the_search_finds(family):
    for case in (K.RT_STALE if family == 'stale' else K.TABLES[family]):
        assert K.find_seed(case) == K.seed_of(case), case.id


def test_stale_buffer_subsets_keep_the_margin():
    for case in K.RT_STALE:
        _, _, ref = K.first_samples(case, K.make(case), 1)
        assert all(inside == 0 for _, inside, _ in R.margin_report(ref['relus']))
