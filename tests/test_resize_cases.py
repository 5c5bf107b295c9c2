"""CPU-only checks behind tests/test_gpu_resize.py: the cases select the kernels they are there for, every kernel and every loop of
the resize family is reached, the matrix references agree with oracle.torch_ops' own resizes, and the float32 evaluation of the
transpose that fixes the dX tolerance stays where the GPU tests' docstring says it does."""
import os
import re

import numpy as np
import pytest

from tests import resize_cases as K
from tests import graph_ops_cases as G

ALL = K.TABLE + K.NEAREST + K.NEAREST_LARGE + [c for _, c, _ in K.ACCUMULATE]


def _ids(cases):
    return [c.id for c in cases]


def test_case_names_are_unique_and_every_method_is_there():
    ids = _ids(ALL)
    assert len(set(ids)) == len(ids)
    assert {c.method for c in K.TABLE} == set(K.TABLE_METHODS)
    assert set(K.EXPECT) <= set(ids) and set(K.EXPECT_LOOPS) <= set(ids)
    for c in ALL:
        assert all(v >= 1 for v in c[2:]), c


def test_named_cases_select_their_kernels():
    by_id = {c.id: c for c in ALL}
    for cid, want in K.EXPECT.items():
        s = K.select(by_id[cid])
        assert (s['fwd'], s['bwd']) == want, (cid, s)
    for cid, loops in K.EXPECT_LOOPS.items():
        assert K.select(by_id[cid])['loops'] == loops, cid
    for c in K.SCALAR + [c for c in K.DEGENERATE if c.c == 3]:
        s = K.select(c)
        assert (s['fwd'], s['bwd']) == ('fwd', 'bwd'), c
    for c in K.NEAREST + K.NEAREST_LARGE:
        s = K.select(c)
        assert (s['fwd'], s['bwd']) == ('nearest_fwd', 'nearest_bwd'), c
    for kind, c, second in K.ACCUMULATE:
        assert K.select(c)['bwd'] == kind and second != c.method, c
    assert {kind for kind, _, _ in K.ACCUMULATE} == {'nearest_bwd', 'bwd', 'bwd4', 'bwd4u<4>', 'bwd4u<8>'}


def test_every_kernel_is_selected_twice_and_every_loop_once():
    hits = {k: 0 for k in K.ALL_KERNELS}
    loops = set()
    for c in K.TABLE + K.NEAREST + K.NEAREST_LARGE:
        s = K.select(c)
        hits[s['fwd']] += 1
        hits[s['bwd']] += 1
        loops |= s['loops']
    assert all(n >= 2 for n in hits.values()), hits
    assert loops == {'rows', 'per_row', 'grid_fwd', 'grid_bwd'}
    # the grid-stride loop: a float4 launch over dX, one over Y and a scalar one over both
    sel = {c.id: K.select(c) for c in K.LARGE}
    assert sel['bl_half_c64_large_dx']['bwd'] == 'bwd4u<4>' and 'grid_bwd' in sel['bl_half_c64_large_dx']['loops']
    assert sel['ga_x2_c64_large_y']['fwd'] == 'fwd4' and 'grid_fwd' in sel['ga_x2_c64_large_y']['loops']
    assert sel['bl_half_x2_c3_large']['loops'] == {'grid_fwd', 'grid_bwd'}


def test_row_width_cases():
    """C = 4 with 4 <= Wo <= 64: at most one float4 per thread of the 64-thread launch; 256 float4 exactly: the 256-thread launch, one
    trip; C = 16 with Wo >= 70: 256 threads, a second ragged trip.  80 float4 on 64 threads: a second ragged trip there too."""
    by_id = {c.id: c for c in K.BILINEAR_VEC}
    assert [K.per_row4(by_id[i]) for i in ('bl_wo4_c4', 'bl_wo64_c4', 'bl_x4_c8', 'bl_wo64_c16', 'bl_wo70_c16', 'bl_wo72_c16_x4')] \
        == [4, 64, 80, 256, 280, 288]
    rows = by_id['bl_rows']
    assert rows.n * rows.t * rows.ho > K.FWDK_MAX_BLOCKS and (rows.w, rows.wo) == (1, 2)


def test_launcher_conditions_match_the_source():
    """The conjuncts ``select`` restates, as written in csrc/elementwise.hip and csrc/graph.hip."""
    root = os.path.join(G.ROOT, 'dl4ds_amd', 'csrc')
    ew = re.sub(r'\s+', '', open(os.path.join(root, 'elementwise.hip')).read())
    gr = re.sub(r'\s+', '', open(os.path.join(root, 'graph.hip')).read())
    for piece in ('ky==kx&&(ky==2||ky==4)&&rows<(1ull<<31)&&per_row4<(1u<<20)&&(y.C>>2)<=4096',
                  'constintthreads=per_row4>=256?256:64;',
                  'dim3((unsigned)std::min<size_t>(rows,65536))',
                  'if(max_taps_x>0&&max_taps_x<=8&&!no_u)',
                  'max_taps_x<=4?resize_table_bwd4u_kernel<4>:resize_table_bwd4u_kernel<8>',
                  'DL4DS_LAUNCH(resize_table_fwd4_kernel,dim3(ew_blocks(total/4))',
                  'DL4DS_LAUNCH(resize_table_bwd4_kernel,dim3(ew_blocks(total/4))',
                  'DL4DS_LAUNCH(resize_table_fwd_kernel,dim3(ew_blocks(total))',
                  'DL4DS_LAUNCH(resize_table_bwd_kernel,dim3(ew_blocks(total))'):
        assert piece in ew, piece
    for piece in ('if(w[(size_t)o*K+k]!=0.f)cols[idx[(size_t)o*K+k]].push_back',
                  'max_back=std::max(max_back,(int)cols[i].size());',
                  'op->bicubic=nearest>=2||(nearest==0&&!exp_env("DL4DS_RESIZE_BILINEAR_DIRECT"));'):
        assert piece in gr, piece
    # a resize input counts as "other" use: it is never aliased into a Concatenate, so no strided view reaches these kernels
    assert 'g.tensors[in].n_other++;' in re.search(r'intg_resize\(.*?returnout;}', gr).group(0)
    assert K.EW_GRID_THREADS == G.EW_GRID_THREADS == G.ew_grid_threads_in_source()


@pytest.mark.parametrize('case', K.TABLE, ids=_ids(K.TABLE))
def test_float32_tables_have_the_oracles_pattern(case):
    """The launcher sees tables built in float32; the references are built in float64.  On every case the two agree on what
    decides the kernel: the bilinear taps and which of them are non-zero, and the span of the ScaleAndTranslate methods covers every
    non-zero entry of the oracle's matrix."""
    for inn, out in ((case.h, case.ho), (case.w, case.wo)):
        if case.method == 'bilinear':
            lo64, hi64, f64 = K.bilinear_taps(inn, out)
            lo32, hi32, f32 = K.bilinear_taps(inn, out, np.float32)
            assert f32.dtype == np.float32
            np.testing.assert_array_equal(lo32, lo64)
            np.testing.assert_array_equal(hi32, hi64)
            np.testing.assert_array_equal(K.back_counts('bilinear', inn, out, np.float32), K.back_counts('bilinear', inn, out))
            assert np.abs(f32 - f64).max() <= 2e-6          # a fifth of the forward tolerance at |x| <= max |x|
        else:
            M = K.axis_matrix(case.method, inn, out)
            assert K.taps(case.method, inn, out) >= (M != 0).sum(axis=1).max()
            if case.method != 'bicubic':                     # a span is contiguous
                nz = M != 0
                first, last = nz.argmax(axis=1), inn - 1 - nz[:, ::-1].argmax(axis=1)
                assert K.taps(case.method, inn, out) >= (last - first + 1).max()


@pytest.mark.parametrize('case', K.SMALL_TABLE + K.NEAREST, ids=_ids(K.SMALL_TABLE + K.NEAREST))
def test_matrix_reference_equals_the_oracle(case):
    """Y = My X Mx^T and dX = My^T dY Mx against oracle.torch_ops' resize and autograd through it, to 1e-12."""
    x, dy = K.case_input(case), K.case_target(case)
    y, dx = K.torch_refs(case, x, dy)
    np.testing.assert_allclose(K.forward_ref(case, x), y, rtol=0, atol=1e-12)
    np.testing.assert_allclose(K.backward_ref(case, dy), dx, rtol=0, atol=1e-12)
    My, Mx = K.matrices(case)
    np.testing.assert_allclose(My.sum(axis=1), 1.0, rtol=0, atol=1e-6)
    np.testing.assert_allclose(Mx.sum(axis=1), 1.0, rtol=0, atol=1e-6)


def test_matrix_reference_of_a_two_resize_sum():
    for _, case, second in K.ACCUMULATE:
        x, dy = K.case_input(case), K.case_target(case)
        y, dx = K.torch_refs(case, x, dy, (case.method, second))
        np.testing.assert_allclose(K.forward_ref(case, x) + K.forward_ref(case, x, second), y, rtol=0, atol=1e-12)
        np.testing.assert_allclose(K.backward_ref(case, dy) + K.backward_ref(case, dy, second), dx, rtol=0, atol=1e-12)


def test_float32_evaluation_of_the_transpose_supports_the_dx_tolerance():
    """My^T dY Mx in numpy float32 with float32 weights against float64, on every table-driven case and both members of every
    accumulation pair: under a quarter of 1e-5 everywhere (measured maximum 1.5e-7), so the dX tolerance stays at 1e-5."""
    worst = max([K.dx_emulation_error(c) for c in K.TABLE]
                + [K.dx_emulation_error(c, m) for _, c, second in K.ACCUMULATE for m in (c.method, second)])
    print(f'largest float32-emulation error of dX: {worst:.3e}')
    assert 0 < worst < K.DX_EMULATION_CAP
    assert K.DX_TOL == K.FWD_TOL == 1e-5 and K.DX_EMULATION_CAP == K.DX_TOL / 4


@pytest.mark.parametrize('case', K.NEAREST + K.NEAREST_LARGE, ids=_ids(K.NEAREST + K.NEAREST_LARGE))
def test_nearest_cases(case):
    """No case sits on a rounding boundary of the source index (float32 as in the kernel, float64 as in the oracle), and no input
    element is copied more than k = ceil(Ho / H) * ceil(Wo / W) times."""
    for inn, out in ((case.h, case.ho), (case.w, case.wo)):
        np.testing.assert_array_equal(K.nearest_src(inn, out, np.float32), K.nearest_src(inn, out))
        np.testing.assert_array_equal(K.axis_matrix('nearest', inn, out).argmax(axis=1), K.nearest_src(inn, out))
    My, Mx = K.matrices(case)
    assert My.sum(axis=0).max() * Mx.sum(axis=0).max() <= K.nearest_terms(case)


def test_nearest_reference_on_a_hand_made_row():
    """3 -> 7: sources floor((o + 0.5) * 3 / 7) = 0 0 1 1 1 2 2."""
    c = K.Case('hand', 'nearest', 1, 1, 1, 3, 1, 1, 7)
    dy = np.array([1, -2, 4, 8, -16, 32, 64], np.float32).reshape(1, 1, 7, 1)
    s, a = K.nearest_backward_ref(c, dy)
    np.testing.assert_array_equal(s.ravel(), [-1, -4, 96])
    np.testing.assert_array_equal(a.ravel(), [3, 28, 96])
    assert K.nearest_terms(c) == 3
