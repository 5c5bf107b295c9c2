"""CPU-only checks behind tests/test_gpu_norm.py: the constants and launch expressions restated in tests/norm_cases.py stand in
csrc/norm.hip and csrc/dwconv.hip; the cases select the forms they are named for, every listed form at least twice; the references
written out there agree with oracle.torch_ops; and the float64 reference alone shows that the cases are sensitive:

  - a reference that loses the partial slabs of index >= 64, the last chunk, or the pixels of the second grid-stride trip differs
    from the full one, per affected output, by at least 10 x that output's tolerance in the tolerance's own measure.  Smallest
    factor found over all cases and outputs: 15.5 x (BatchNorm 'nb66_s', dgamma without the two slabs beyond 64; without the last
    chunk the smallest is 58.9 x, BatchNorm 'cap_s_short' dx: its 8 pixels of 9215 carry offsets of +-8 in x and dy, on plain noise
    they would not show).  Outputs an omission cannot reach are not
    asserted: LayerNorm's y and dx without slabs (they are written per pixel), the depthwise y and dx (no partial sums);
  - on an accumulate case neither the gradients without the preload nor the preload alone pass for the expected result: both are
    off by at least 10 x the tolerance (gradients that are identically zero excepted, where the preload IS the result:
    LayerNorm's dx and dgamma at C = 1, BatchNorm's at one pixel);
  - with the ReLU fused, every float64 pre-activation lies at least 2e-4 from zero: a condition on the inputs, no element is
    excluded from any comparison.
"""
import os
import re

import numpy as np
import pytest

from tests import graph_ops_cases as G
from tests import norm_cases as K

OPS = ('ln', 'bn', 'dw')
ALL = [(op, c) for op in OPS for c in K.TABLES[op]]
SMALLEST = {}


def _ids(pairs):
    return [f'{op}-{c.id}' for op, c in pairs]


def _src(name):
    return re.sub(r'\s+', '', open(os.path.join(G.ROOT, 'dl4ds_amd', 'csrc', name)).read())


def test_constants_and_launch_expressions_match_the_source():
    norm = _src('norm.hip')
    for piece in (f'constexprintNORM_THREADS={K.NORM_THREADS};',
                  f'constexprintNORM_KMAX={K.NORM_KMAX};',
                  f'constexprintNORM_MAX_BLOCKS={K.NORM_MAX_BLOCKS};',
                  'for(intb=threadIdx.x&63;b<nb;b+=64)t+=(double)partial[(size_t)b*stride+col];',
                  'inlineboolvec_ok(intC,std::initializer_list<constvoid*>ptrs){if(C&3)returnfalse;',
                  'inlineintln_lanes(intCP){intL=1;while(L<CP&&L<64)L<<=1;returnL;}',
                  'inlineintln_blocks(size_tnpix,intL){constsize_tgpb=NORM_THREADS/L;'
                  'return(int)std::max<size_t>(1,std::min<size_t>(NORM_MAX_BLOCKS,(npix+gpb-1)/gpb));}',
                  'constintL=ln_lanes(v4?C/4:C);constintnb=ln_blocks(npix,L);',
                  'for(size_tp=(size_t)blockIdx.x*gpb+threadIdx.x/L;p<npix;p+=(size_t)gridDim.x*gpb){',
                  'constintj=threadIdx.x&(L-1);constsize_tgpb=NORM_THREADS/L;',
                  'for(intsl=0;sl<NORM_KMAX;++sl){constintk=j+sl*L;if(k<CP){',
                  'DL4DS_REQUIRE(C>=1&&C/V<=64*NORM_KMAX&&C/V<=NORM_THREADS,',
                  'g.CP=C/V;g.R=NORM_THREADS/g.CP;g.T=g.R*g.CP;'
                  'constsize_twant=std::max<size_t>(1,std::min<size_t>(NORM_MAX_BLOCKS,npix/(size_t)(g.R*8)+1));'
                  'g.chunk=(npix+want-1)/want;g.nb=(int)((npix+g.chunk-1)/g.chunk);',
                  'constsize_tp0=(size_t)blockIdx.x*g.chunk,p1=min(p0+g.chunk,npix);for(size_tp=p0+row;p<p1;p+=g.R){',
                  'if(d0==nullptr)return;',
                  '*d=acc?*d+(float)t:(float)t;',
                  'w.v[i]=acc_dx?w.v[i]+t:t;',
                  'w.v[i]=acc_dx?w.v[i]+u:u;',
                  'if(dgamma){dgamma[c]=acc?dgamma[c]+(float)s1:(float)s1;dbeta[c]=acc?dbeta[c]+(float)s2:(float)s2;}',
                  'sums[c]=(float)(s1/(double)npix);sums[C+c]=(float)(s2/(double)npix);if(dgamma){',
                  'constdoubleunbiased=npix>1?var*n/(n-1.0):var;',
                  'DL4DS_LAUNCH(partial_reduce_kernel,dim3((2*C+3)/4),dim3(256),0,s,ws,nb,2*C,dgamma,dbeta,C,acc_dw);',
                  'if(dx){if(v4)DL4DS_LAUNCH(bn_bwd_apply_kernel<4>,dim3(g.nb),',
                  'constBnGeomg=bn_geom(npix,C,V);'):
        assert piece in norm, piece
    assert norm.count('p1=min(p0+g.chunk,npix);') == 4 and norm.count('dim3(g.nb),dim3(NORM_THREADS)') == 8
    dw = _src('dwconv.hip')
    for piece in (f'constexprintDW_PW={K.DW_PW};',
                  f'constexprintDW_MAX_CHUNKS={K.DW_MAX_CHUNKS};',
                  'DL4DS_REQUIRE(KS==7,',
                  'g.CPB=std::min(CP,256/K);',
                  'g.LANES=std::max(1,256/(g.CPB*K));g.groups=(CP+g.CPB-1)/g.CPB;'
                  'constsize_twant=std::max<size_t>(1,std::min<size_t>(DW_MAX_CHUNKS,npix/(size_t)(g.LANES*4)+1));'
                  'g.chunk=(npix+want-1)/want;g.nchunks=(int)((npix+g.chunk-1)/g.chunk);',
                  'constWgradGeomg=wgrad_geom((size_t)N*H*((W+DW_PW-1)/DW_PW),C,v4?4:1,KS);',
                  'dim3(g.nchunks,g.groups),dim3(256)',
                  'constsize_tp0=(size_t)blockIdx.x*chunk,p1=min(p0+chunk,nitems);',
                  'for(size_tit=p0+lane;it<p1;it+=LANES){constintwg=(int)(it%WG);constsize_tq=it/WG;',
                  'for(intb=threadIdx.x&63;b<nchunks;b+=64)s+=(double)partial[(size_t)b*n+e];',
                  'float*d=e<KK*C?dk+e:(db?db+(e-KK*C):nullptr);if(d)*d=accumulate?*d+(float)s:(float)s;',
                  'inlineboolvec_ok(intC,std::initializer_list<constvoid*>ptrs){if(C&3)returnfalse;'):
        assert piece in dw, piece
    capi = _src('capi.cpp')
    for piece in ('if(dx)dwconv_forward(S(),dy,k,nullptr,dx,N,H,W,C,KS,1,accumulate);if(dk){',
                  'dwconv_wgrad(S(),x,dy,dk,db,accumulate,N,H,W,C,KS,scratch(ws),ws);',
                  'layernorm_backward(S(),x,y,dy,gamma,dx,accumulate,dgamma,dbeta,accumulate,npix,C,eps,relu,scratch(ws),ws);',
                  'batchnorm_backward(S(),x,y,dy,gamma,saved,dx,accumulate,dgamma,dbeta,accumulate,npix,C,relu,scratch(ws),ws);'):
        assert piece in capi, piece
    ops3 = _src('graph_ops3.hip')
    for piece in ('constbooldx=wants_grad(g,in,c);',
                  'float*dg=c.param_grads?g.gp(gamma):nullptr;',
                  'constintaccw=g.params[gamma].grad_written;',
                  'dxp,t.grad_written,dg,db,accw,n,t.C,eps,relu,',
                  'dx?t.grad+k*gs:nullptr,t.grad_written,dg,db,first?accw:1,',
                  'dwconv_wgrad(g.stream,t.data+off,dy,g.gp(w),b>=0?g.gp(b):nullptr,g.params[w].grad_written,cnt,',
                  'dwconv_forward(g.stream,dy,g.wp(w),nullptr,t.grad+off,cnt,t.H,t.W,t.C,KS,1,t.grad_written);'):
        assert piece in ops3, piece


def test_case_names_are_unique_and_shapes_are_supported():
    for op in OPS:
        ids = [c.id for c in K.TABLES[op]]
        assert len(set(ids)) == len(ids)
        for c in K.TABLES[op]:
            C = c.shape[-1]
            assert len(c.shape) == 4 and all(v >= 1 for v in c.shape)
            assert C // K.vec(C) <= 64 * K.NORM_KMAX and C // K.vec(C) <= K.NORM_THREADS
            assert 12 * int(np.prod(c.shape[:-1])) < 2 ** 24          # integer sums stay exact in float32
            assert c.dx or c.dw or op == 'dw', 'a case that requests nothing'
    assert {k[0] for k in K.EXPECT} == set(OPS)
    for c in K.G_RESIDUAL + K.G_SHARED + K.G_FIRST + K.G_INFER + K.G_DW:
        assert len(c.shape) in (4, 5)
    assert {(c.kind, len(c.shape), K.vec(c.shape[-1]), c.relu) for c in K.G_RESIDUAL} \
        == {(k, n, v, r) for k in ('ln', 'bn') for n, v in ((4, 4), (4, 1), (5, 4)) for r in (False, True)}


def test_named_cases_select_what_they_are_named_for():
    sel = {'ln': K.ln_select, 'bn': K.bn_select, 'dw': K.dw_select}
    for (op, cid), want in K.EXPECT.items():
        case = {c.id: c for c in K.TABLES[op]}[cid]
        s = sel[op](case.shape)
        for k, v in want.items():
            assert s[k] == v, (op, cid, k, s[k], v)
    # the figures quoted by the issue, from the restated geometry
    assert K.bn_select((1, 48, 48, 256))['nb'] == 72 and K.bn_select((1, 96, 96, 130))['chunk'] == 9
    assert K.dw_select((2, 40, 40, 48))['nchunks'] == 67 and K.dw_select((2, 40, 35, 48))['nchunks'] <= 61
    assert K.dw_select((1, 64, 128, 80))['nchunks'] == 512 and K.dw_select((1, 64, 128, 80))['LANES'] == 1
    assert K.ln_select((1, 33, 17, 256))['nb'] == 141
    assert max(K.bn_select(s)['nb'] for s in K.NORM_SHAPES) <= 18


def test_every_listed_form_is_selected_twice():
    for op in OPS:
        hits = {}
        for c in K.TABLES[op]:
            for f in K.FEATURES_OF[op](c):
                hits.setdefault(f, []).append(c.id)
        for f in K.REQUIRED[op]:
            assert len(hits.get(f, [])) >= 2, (op, f, hits.get(f))
        for f in K.ONCE.get(op, []):
            assert len(hits.get(f, [])) >= 1, (op, f)
    # every (V, L, slots) form of tests/test_gpu_ops.py::NORM_SHAPES, and with them L in {1, 4, 8, 16, 64} and slots 1, 3, 4
    forms = [K.ln_select(s) for s in K.NORM_SHAPES]
    assert {f['L'] for f in forms} == {1, 4, 8, 16, 64} and {f['slots'] for f in forms} == {1, 3, 4}
    from tests import test_gpu_ops
    assert test_gpu_ops.NORM_SHAPES == K.NORM_SHAPES


@pytest.mark.parametrize('op,case', ALL, ids=_ids(ALL))
def test_inputs(op, case):
    """Integer operands are integers in range; with the ReLU fused no float64 pre-activation lies within 2e-4 of zero; the preloads
    have the magnitude of the gradients; the written-out BatchNorm equals the oracle."""
    d = K.inputs(op, case)
    for k, lo, hi in (('dyi', -4, 4), ('xi', -4, 12), ('prei', -4, 4)):
        a = d[k]
        assert a.dtype == np.float32 and a.min() >= lo and a.max() <= hi and (a == np.round(a)).all()
    ref = K.reference(op, case, d, preload=False)
    if op != 'dw' and case.relu:
        pre = K.preact(op, d['x'], d['gamma'], d['beta'], 1e-3)
        assert np.abs(pre).min() >= K.RELU_MARGIN, (op, case.id, np.abs(pre).min())
        assert (pre > 0).any() and ((pre < 0).any() or pre.size < 16)
    if op == 'bn':
        w = K.bn_written_out(case, d)
        for k in ('y', 'dx', 'dgamma', 'dbeta', 'mean', 'var'):
            np.testing.assert_allclose(w[k], ref[k], rtol=0, atol=1e-9 * max(1.0, np.abs(ref[k]).max()), err_msg=k)
    if case.acc:
        names = ('dx',) + (('dk', 'db') if op == 'dw' else ('dgamma', 'dbeta'))
        full = K.reference(op, case, d)
        for n, p in zip(names, d['pre']):
            if n not in K.outputs(op, case) or (op == 'ln' and n != 'dbeta' and case.shape[-1] == 1):
                continue                                   # one channel: xhat = 0, dx and dgamma are identically zero
            if op == 'bn' and n != 'dbeta' and int(np.prod(case.shape[:-1])) == 1:
                continue                                   # one pixel: dx and dgamma are identically zero
            tol = K.TOL[op][n]
            a, b = K.rel_err(ref[n], full[n]), K.rel_err(p.reshape(full[n].shape), full[n])
            assert a >= 10 * tol and b >= 10 * tol, (op, case.id, n, a, b)


SENSITIVE = [(op, c) for op, c in ALL if K.keep_masks(op, c)]


@pytest.mark.parametrize('op,case', SENSITIVE, ids=_ids(SENSITIVE))
def test_reference_is_sensitive_to_lost_work(op, case):
    d = K.inputs(op, case)
    masks = K.keep_masks(op, case)
    full = K.reference(op, case, d)
    sums = ('dk', 'db') if op == 'dw' else ('dgamma', 'dbeta')
    checked = 0
    for kind, keep in masks.items():
        if kind == 'last_chunk' and not case.hot:
            continue
        assert 0 < keep.sum() < keep.size
        if op == 'bn':
            moved = dict(K.bn_written_out(case, d, keep_bwd=keep), y=K.bn_written_out(case, d, keep_stats=keep)['y'])
            if case.acc:
                for n, p in zip(('dx', 'dgamma', 'dbeta'), d['pre']):
                    moved[n] = moved[n] + p.astype(np.float64).reshape(moved[n].shape)
            names = ['y'] + K.outputs(op, case)
        else:
            moved = K.reference(op, case, d, keep=keep)
            names = [n for n in K.outputs(op, case) if n in sums or (op == 'ln' and kind == 'trip')]
        for n in names:
            factor = K.rel_err(moved[n], full[n]) / K.TOL[op][n]
            key = (op, kind, n)
            SMALLEST[key] = min(SMALLEST.get(key, np.inf), factor)
            print(f'{op} {case.id}: without {kind}, {n} moves by {factor:.1f} x its tolerance')
            assert factor >= 10, (op, case.id, kind, n, factor)
            checked += 1
    if op == 'ln' or case.hot or 'slabs' in masks:
        assert checked, (op, case.id)


def test_omissions_cover_what_the_issue_names():
    kinds = {op: set() for op in OPS}
    for op, c in SENSITIVE:
        for kind in K.keep_masks(op, c):
            if kind != 'last_chunk' or c.hot:
                kinds[op].add(kind)
    assert kinds == {'ln': {'slabs', 'trip'}, 'bn': {'slabs', 'last_chunk'}, 'dw': {'slabs', 'last_chunk'}}


GRAPH = ([(c, 'residual') for c in K.G_RESIDUAL] + [(c, 'shared') for c in K.G_SHARED] + [(c, 'first') for c in K.G_FIRST])


@pytest.mark.parametrize('case,mode', GRAPH, ids=[f'{m}-{c.id}' for c, m in GRAPH])
def test_graph_inputs(case, mode):
    """ReLU margins of the in-graph cases; the residual path and the second norm carry weight: the norm's share alone, or one
    norm's parameter gradients alone, miss the expected result by 10 x the tolerance or more."""
    inp = K.graph_inputs(case, mode)
    if case.relu:
        for p in K.graph_norm_preact(case, inp['xs'], inp['w'], mode):
            assert np.abs(p).min() >= K.RELU_MARGIN
    dy = inp['target'].astype(np.float64)
    out, dxs, grads = K.graph_norm_ref(case, inp['xs'], inp['w'], dy, mode)
    assert out.shape == case.shape
    if mode == 'residual':
        _, dxs1, grads1 = K.graph_norm_ref(case, inp['xs'], inp['w'], dy, 'plain')
        assert K.rel_err(dxs1[0], dxs[0]) >= 10e-3 and K.rel_err(grads1['p/kernel'], grads['p/kernel']) >= 10e-3
    if mode == 'shared':
        for k in (0, 1):
            one = K.graph_norm_ref(case, [inp['xs'][k]], inp['w'], dy, 'first')[2]
            assert all(K.rel_err(one[n], grads[n]) >= 10e-3 for n in ('n/gamma', 'n/beta')), case.id


@pytest.mark.parametrize('case', K.G_DW, ids=[c.id for c in K.G_DW])
def test_graph_depthwise_inputs(case):
    from oracle import torch_ops as T
    inp = K.graph_inputs(case, 'dw')
    assert ('d/bias' in inp['w']) == case.relu
    dy = inp['target'].astype(np.float64)
    _, _, both = K.graph_dw_ref(case, inp['xs'], inp['w'], dy)
    for x in inp['xs']:
        _, _, one = K.graph_dw_ref(case, [x], inp['w'], dy)
        assert K.rel_err(one['d/depthwise_kernel'], both['d/depthwise_kernel']) >= 10e-3
