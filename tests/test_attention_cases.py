"""CPU-only checks behind tests/test_gpu_attention.py: the cases select the kernels, template instantiations and loops they are there
for; every one of them is reached at least twice; the restated launcher conditions stand in the source; the inputs keep the hidden
ReLU off its kink, keep the integer column sums exact, and make the hand-over references sensitive to one missing pooling tile; and
the references written out here agree with oracle.models."""
import os
import re

import numpy as np
import pytest

from tests import attention_cases as K
from tests import graph_ops_cases as G

GRAPH_CASES = K.ACC_DX + K.ACC_DW


def _ids(cases):
    return [c.id for c in cases]


def _src(name):
    return re.sub(r'\s+', '', open(os.path.join(G.ROOT, 'dl4ds_amd', 'csrc', name)).read())


def test_case_names_are_unique_and_shapes_are_sane():
    ids = _ids(K.EAGER + GRAPH_CASES + K.HANDOVER)
    assert len(set(ids)) == len(ids)
    assert set(K.EXPECT) == set(_ids(K.EAGER))
    for c in K.EAGER + GRAPH_CASES:
        assert len(c.shape) in (4, 5) and all(v >= 1 for v in c.shape) and c.shape[-1] >= 4, c
        d = K.dims(c)
        assert d['Cr'] >= 1 and d['G'] * d['R'] * d['Q'] == int(np.prod(c.shape))


def test_named_cases_select_what_they_are_named_for():
    for c in K.EAGER:
        s = K.select(c)
        want = dict(K.EXPECT[c.id])
        has, lacks = want.pop('has', set()), want.pop('lacks', set())
        for k, v in want.items():
            assert s[k] == v, (c.id, k, s[k], v)
        assert has <= s['features'] and not (lacks & s['features']), (c.id, s['features'])


def test_every_kernel_template_and_loop_is_selected_twice():
    hits = {f: [] for f in K.FEATURES}
    for c in K.EAGER:
        for f in K.select(c)['features']:
            hits[f].append(c.id)              # (KeyError: a feature select() names and FEATURES does not)
    for f, ids in hits.items():
        assert len(ids) >= (1 if f in K.ONCE else 2), (f, ids)
    assert sum(len(hits[f]) for f in K.ONCE) >= 2
    # the accumulating backward: the float4 form, the float4 form straddling rows, the scalar form, a 5-D input
    sel = {c.id: K.select(c) for c in K.ACC_DX}
    assert [sel[i]['V'] for i in ('accdx_v4', 'accdx_v4_straddle', 'accdx_v1')] == [4, 4, 1]
    assert sel['accdx_v4_straddle']['straddle'] and not sel['accdx_v4']['straddle']
    assert [len(c.shape) for c in K.ACC_DX].count(5) >= 1 and [len(c.shape) for c in K.ACC_DW].count(5) >= 1
    assert K.select(K.ACC_DW[-1])['lane_trips'] == 2


def test_launcher_conditions_match_the_source():
    """The conjuncts ``select``, ``pool_tiles`` and ``expected_flags`` restate, as written in the sources."""
    att = _src('attention.hip')
    for piece in ('intpick_tx(intQ){returnQ<=8?8:(Q<=16?16:(Q<=32?32:64));}',
                  'intcolsum_blocks(intR,intTY){returnstd::max(1,std::min(cdiv(R,TY*8),256));}',
                  'constintTX=pick_tx(Q),TY=256/TX;',
                  'if(Q>=256&&(Q&3)==0&&((uintptr_t)a&15)==0&&',
                  'constintnb4=std::max(1,std::min(cdiv(R,4*8),256));',
                  'constexprintTX=64,TY=4;',
                  'constintstep=gridDim.x*TY;intr=blockIdx.x*TY+tyi;for(;r+7*step<R;r+=8*step){',
                  'for(;r<R;r+=step){',
                  'for(intr=blockIdx.x*TY+tyi;r<R;r+=gridDim.x*TY){',
                  'for(;k+8<=nb;k+=8){',
                  'for(;k<nb;++k)s[0]+=',
                  'constboolv4=(RQ&3)==0&&',
                  'constsize_tn=v4?RQ/4:RQ;',
                  'constunsignedbx=(unsigned)std::max<size_t>(1,std::min<size_t>((n+255)/256,std::max<size_t>(1,8192/(size_t)G)));',
                  'constintdq=(int)(((unsignedlonglong)stride*V)%(unsigned)Q);',
                  'q+=dq;if(q>=Q)q-=Q;',
                  'qq=(qq+1==Q)?0:qq+1;',
                  'for(intinst=lane;inst<ninst;inst+=64)',
                  'DL4DS_LAUNCH(chatt_mlp_bwd_inst_kernel,dim3(cdiv(ninst,256)),dim3(256)',
                  'constintg=blockIdx.x*4+(threadIdx.x>>6);',
                  'constintfull=tiles&~7;',
                  'if(u==0&&c<C)out[(size_t)g*C+c]=s*scale;'):
        assert piece in att, piece
    narrow = _src('conv_narrow.hip')
    assert f'#defineNARROW_PAIR_ROWS{K.NARROW_PAIR_ROWS}#endif' in narrow
    assert f'returncdiv(W,{K.POOL_TILE_W})*cdiv(H,4*NARROW_PAIR_ROWS);' in narrow
    # which family takes a layer is stated once, in conv_route.h: the families' conditions ...
    route = _src('conv_route.h')
    assert 'returnin.C<=8&&out.C<=8&&(out.C&3)==0&&out.vec&&' in route
    assert 'returnpad_pow2(in.C)*pad_pow2(out.C)<=8;' in route
    assert 'inlineboolaffine_ok(constTView&v){return!v.sc||(v.vec&&(v.C&3)==0&&v.C>=4);}' in route
    # ... the order in which the routes ask them (the stencil kernels first, the pair kernel before the other narrow ones) ...
    for piece in ('if(eligible(in,out,KS)){if(!affine_ok(in)||ep.pool)return{ConvFwdFamily::Direct,"conv_direct:',
                  'if(pair)return{ConvFwdFamily::NarrowPair,nullptr};',
                  'if(eligible(x,dz,KS))return{WgradFamily::Direct,slabs(DTX,DTY),(affine_ok(x)&&!dz.sc)?nullptr:"conv_directwgrad:',
                  'if(narrow_wgrad_eligible(x,dz,KS))return{WgradFamily::Narrow,slabs(NTW,NTH),nullptr};'):
        assert piece in route, piece
    # ... and the planner's three decisions as questions put to the routes
    gr = _src('graph.hip')
    for piece in ('if(producer&&producer->d2s<=1&&ti.C<=8){',
                  'fz.fuse_pool=conv2d_forward_route(pin,pout,producer->KS,ep).family==ConvFwdFamily::NarrowPair;',
                  'constConvFwdRouter=conv2d_forward_route(x,y,3,ConvEpilogue());fz.fuse_scale=r.family==ConvFwdFamily::Direct&&!r.refusal;',
                  'constboolok=conv2d_wgrad_route(px,dz,3).family==WgradFamily::Narrow;',
                  'constConvFwdRouterd=conv2d_forward_route(dz,dx,3,ep);'
                  'fz.fuse_dx=ok&&!rd.refusal&&(rd.family==ConvFwdFamily::Direct||rd.family==ConvFwdFamily::NarrowPair);',
                  'if(T5>0||test_env("DL4DS_NO_TAIL_FUSION"))return;',
                  'g.tensors[in].grad_written,shape(g,c.B)',                    # accumulate_dx
                  'constintaccw=g.params[w1].grad_written;'):                    # accumulate_dw
        assert piece in gr, piece
    # the layout of ``saved`` the eager tests read: [mean: inst * C][scale: inst * C][hidden: inst * Cr]
    assert 'float*mean=saved;float*scale=mean+inst*C;float*hidden=scale+inst*C;' in _src('capi.cpp')


@pytest.mark.parametrize('case', K.EAGER, ids=_ids(K.EAGER))
def test_eager_inputs(case):
    """Conditions on the inputs: x is not zero-mean, no hidden pre-activation within 1e-3 of the ReLU's kink, both signs present when
    Cr >= 2, and integer column sums that float32 holds exactly."""
    d = K.dims(case)
    assert 12 * d['R'] < 2 ** 24
    xi = K.integer_x(case)
    assert xi.dtype == np.float32 and xi.min() >= -4 and xi.max() <= 12 and (xi == np.round(xi)).all()
    inp = K.eager_inputs(case)
    mean = K.mean_ref(inp['x'])
    assert mean.shape == (d['ninst'], d['C'])
    assert np.median(np.abs(mean)) > 0.5                # offsets of magnitude 0.5 .. 1.5 under noise of 1 / sqrt(R)
    h = K.preact_ref(mean, inp['w'])
    assert h.shape == (d['ninst'], d['Cr'])
    assert np.abs(h).min() >= K.RELU_MARGIN
    if d['Cr'] >= 2:
        assert (h > 0).any() and (h < 0).any()
    assert K.relu_is_clear(h, d['Cr'])
    # the float32 rounding of the MLP cannot flip a ReLU either
    assert K.mlp_bounds(mean, inp['w'])[4] > 0.5 * K.RELU_MARGIN


SMALL = [c for c in K.EAGER if int(np.prod(c.shape)) < 200000]


@pytest.mark.parametrize('case', SMALL, ids=_ids(SMALL))
def test_written_out_reference_equals_the_oracle(case):
    """mean_ref and mlp_ref against oracle.models.channel_attention (numpy and torch backends), 4-D and 5-D."""
    from oracle import models as M
    from oracle import np_ops as N
    inp = K.eager_inputs(case)
    x = inp['x'].astype(np.float64)
    _, scale = K.mlp_ref(K.mean_ref(x), inp['w'])
    lead = (x.shape[0],) + (1,) * (x.ndim - 3)
    y = x * scale.reshape(lead + x.shape[-2:] if x.ndim == 5 else lead + (1, x.shape[-1]))
    ref = K.oracle_refs(x, inp['w'])
    np.testing.assert_allclose(y, ref, rtol=0, atol=1e-12)
    pn = K.Params({f'a/{k}': v.astype(np.float64) for k, v in inp['w'].items()})
    np.testing.assert_allclose(M.channel_attention(N, pn, 'a', x, x.shape[-1]), ref, rtol=0, atol=1e-12)
    y2, dx, grads = K.oracle_refs(x, inp['w'], inp['dy'])
    np.testing.assert_array_equal(y2, ref)
    assert dx.shape == x.shape and set(grads) == set(K.W_KEYS) and all(np.abs(g).max() > 0 for g in grads.values())


def test_mlp_bounds_hold_for_a_float32_evaluation():
    """The element-wise bounds of step 2 admit a plain numpy float32 evaluation of the MLP and are far below the tolerance of step 3."""
    for case in SMALL:
        inp = K.eager_inputs(case)
        w = inp['w']
        C = K.dims(case)['C']
        m = K.mean_ref(inp['x']).astype(np.float32)
        h = np.maximum(m @ w['conv1/kernel'].reshape(C, -1) + w['conv1/bias'], 0)
        s = 1 / (1 + np.exp(-(h @ w['conv2/kernel'].reshape(-1, C) + w['conv2/bias'])))
        assert h.dtype == s.dtype == np.float32
        h64, bh, s64, bs, clear = K.mlp_bounds(m, w)
        assert clear > 0 and (np.abs(h - h64) <= bh).all() and (np.abs(s - s64) <= bs).all(), case.id
        assert bh.max() < 1e-4 and bs.max() < 1e-4, (case.id, bh.max(), bs.max())


@pytest.mark.parametrize('case', GRAPH_CASES, ids=_ids(GRAPH_CASES))
def test_accumulation_inputs(case):
    n = 2 if case in K.ACC_DW else 1
    inp = K.graph_inputs(case, n)
    d = K.dims(case)
    for x in inp['xs']:
        assert K.relu_is_clear(K.preact_ref(K.mean_ref(x), inp['w']), d['Cr'])
    if n == 2:
        # neither attention alone gives the summed parameter gradients: the test can tell a store from an accumulation
        x1, x2 = inp['xs']
        dy = inp['target']
        both = K.shared_refs(x1, x2, inp['w'], dy)[3]
        for x in (x1, x2):
            one = K.oracle_refs(x, inp['w'], dy)[2]
            assert all(K.rel_err(one[k], both[k]) > 100 * K.TOL for k in K.W_KEYS), case.id
        np.testing.assert_allclose(both['conv2/bias'], K.oracle_refs(x1, inp['w'], dy)[2]['conv2/bias']
                                   + K.oracle_refs(x2, inp['w'], dy)[2]['conv2/bias'], rtol=0, atol=1e-12)
    else:
        x, dy = inp['xs'][0], inp['target']
        _, dx_att, _ = K.oracle_refs(x, inp['w'], dy)
        y, dx, _ = K.oracle_refs(x, inp['w'], dy, residual=True)
        np.testing.assert_allclose(dx, dx_att + dy, rtol=0, atol=1e-12)
        assert K.rel_err(dx_att, dx) > 100 * K.TOL and K.rel_err(dy.astype(np.float64), dx) > 100 * K.TOL


def test_handover_table():
    """ci in {2, 5, 8}; c in {4, 8}; B in {1, 3, 5}; tile counts 1, one of 2..7, one above 8 that is no multiple of 8, 8 and 16; grids
    ragged in both axes; the recorded flags are what the restated eligibility rules give; the baseline shows all four."""
    assert {c.ci for c in K.HANDOVER} == {2, 5, 8} and {c.c for c in K.HANDOVER} == {4, 8}
    assert {b for c in K.HANDOVER for b in c.batches} >= {1, 2, 3, 5}
    tiles = {c.id: K.pool_tiles(c.h, c.w) for c in K.HANDOVER}
    assert tiles['c4_one_tile'] == 1 and tiles['base'] == 4 and tiles['ci2_nine_tiles'] == 9 and tiles['ci5_eight_tiles'] == 8
    assert tiles['sixteen_tiles'] == 16 and tiles['twelve_tiles'] == 12 and tiles['ci5_c4_co2'] == 3 and tiles['b5_then_b2'] == 6
    for c in K.HANDOVER:
        assert c.w % K.POOL_TILE_W and c.h % K.POOL_TILE_H, c.id
        want = (False, False, False) if c.no_fusion else K.expected_flags(c.ci, c.c, c.co)
        assert (c.pool, c.scale, c.dx) == want and c.dscale == c.scale, c.id
    by_id = {c.id: c for c in K.HANDOVER}
    base = by_id['base']
    assert (base.ci, base.c, base.co) == (8, 8, 1) and base.pool and base.scale and base.dx and base.dscale
    assert by_id['b5_then_b2'].batches == (5, 2)
    for i in ('co_eq_c', 'co_eq_c4'):
        assert by_id[i].co == by_id[i].c and by_id[i].pool and not by_id[i].scale
    assert [c.id for c in K.HANDOVER if c.no_fusion] == ['no_fusion']


@pytest.mark.parametrize('case', K.HANDOVER, ids=_ids(K.HANDOVER))
def test_handover_inputs_and_sensitivity(case):
    """The hidden ReLU is clear of its kink on the producer's float64 output; biases are non-zero; the written-out form of the
    reference equals the composition through oracle.models; and a mean that misses any one pooling tile moves the reference output
    by at least 10 x the tolerance, in the tolerance's own measure."""
    inp = K.handover_inputs(case)
    w = inp['w']
    assert set(w) == set(K.H_KEYS) and all(np.abs(w[k]).min() > 0 for k in K.H_KEYS if k.endswith('bias'))
    p = K.handover_ref(case, inp['x'], w, upto='p')
    assert np.median(np.abs(K.mean_ref(p))) > 0.3
    assert K.relu_is_clear(K.preact_ref(K.mean_ref(p), {k[4:]: v for k, v in w.items() if k.startswith('att/')}), case.c // 4, every_instance=True)
    full = K.handover_ref(case, inp['x'], w)
    np.testing.assert_allclose(K.handover_ref(case, inp['x'], w, drop_tile=()), full, rtol=0, atol=1e-12)
    worst = K.handover_sensitivity(case)
    print(f'{case.id}: a missing pooling tile moves the output by at least {worst:.3e}')
    assert worst >= 10 * K.TOL
    # a smaller batch is the leading samples of the larger
    for b in case.batches:
        np.testing.assert_array_equal(K.handover_ref(case, inp['x'][:b], w), full[:b])
