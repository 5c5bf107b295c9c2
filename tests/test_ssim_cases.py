"""CPU-only checks behind tests/test_gpu_ssim.py: the constants and launch expressions restated in tests/ssim_cases.py stand in
csrc/dssim.hip; every long loop of that file takes a second trip in at least one case and every tile-edge class is met by at least
two; the float64 restatements written out in the case module agree with the oracle; and the reference alone shows that the cases
are sensitive -- a result that loses what only a second trip reads differs from the full one by at least 10 x the bound of the
output it reaches:

  - the prediction's late maximum or minimum (min/max grid stride; min/max finish), the second-trip tiles of the compaction,
    the planes >= 256 of ms_combine, the tiles >= 64 of a plane (multi-scale loss and the metrics' SSIM), the pairs >= 64, the
    elements beyond 256 of a pair chunk, the grid points of met_grid's second trip, the pooled elements beyond 8192 x 256.

No case has an unintended tie in a prediction extreme, and no minimum is zero or equal to the other array's minimum (nor a maximum to the other's
maximum) unless the case is about exactly that: the extremes are selected, not computed, so nothing short of equality can flip a branch.  The per-pair Pearson arithmetic of image_metrics is
restated with and without the pivot: float partials of the raw moments miss the 2e-5 bound on the offset cases at (280, 1),
(1000, 1) and (101325, 300) (2.3e-4 .. 1.3e-3; at (280, 5) these draws give 1.3e-5 and 7.5e-6), with the pivot the worst is 2.3e-8.
The field classes (FIELD_CASES): the float32 arithmetic of the loss kernels is restated twice in numpy (K.loss32), with the window
moments of the values themselves and of pivoted values.  The pivoted form holds a quarter of the loss and gradient bounds on every
case (worst: loss 3.8e-2 of its bound on scale1e-3 / msdssim, gradient 0.15 of its bound on mixed-sign / msdssim, at the entry the
min-shift term goes to), so the GPU test's bounds are attainable; the raw form misses both bounds on the SSIM terms of kelvin, pascal
and offset1000 (loss 8 .. 1e5 x its bound) and a bound on near-constant's multi-scale loss, so the cases discriminate.
Largest float64 references: ms-pool 8.7 s, ms-long 4.2 s, grid-trip 3.5 s (test_reference_times prints them).
"""
import os
import re

import numpy as np
import pytest
import torch

from oracle import torch_ops as T
from tests import ssim_cases as K

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FACTOR = 10.0


def _src(*parts):
    return re.sub(r'\s+', '', open(os.path.join(ROOT, *parts)).read())


def _loss_tol(ref):
    return max(K.TOL_LOSS['rel'] * abs(ref), K.TOL_LOSS['abs'])


def test_constants_and_launch_expressions_match_the_source():
    d = _src('dl4ds_amd', 'csrc', 'dssim.hip')
    for piece, count in (
            (f'constexprintKF={K.KF},KH=5,TS={K.TS},TL=TS+KF-1;', 1),
            (f'constexprintCOMPACT_G={K.COMPACT_G};', 1),
            (f'constexprintMS_SCALES={K.MS_SCALES};', 1),
            (f'constexprintMET_CHUNKS={K.MET_CHUNKS},MET_K=7;', 1),
            (f'h.nb_mm={K.MM_CAP};', 1),                                                   # carve_stats
            ('constintnb=(int)std::min<size_t>(h.nb_mm,cdivz(n,256));', 1),               # run_minmax, the one min/max launch pair
            ('DL4DS_LAUNCH(minmax_kernel,dim3(nb),dim3(256)', 1),
            ('run_minmax(s,y_true,y_pred,', 3),
            ('for(size_te=(size_t)blockIdx.x*256+threadIdx.x;e<n;e+=(size_t)gridDim.x*256){constfloata=t[e],b=p[e];', 1),
            ('for(intk=i;k<nb;k+=256){mnT=fminf(mnT,pf[4*k]);', 1),
            ('constintchunk=(nb+(int)gridDim.x-1)/(int)gridDim.x;constintr0=blockIdx.x*chunk,r1=min(r0+chunk,nb);', 1),
            ('for(intr=r0+threadIdx.x;r<r1;r+=256)', 1),
            ('dim3(COMPACT_G),dim3(256)', 3),
            ('returnMapGeom{Ho,Wo,cdiv(Wo,TS),cdiv(Ho,TS)};', 1),                          # map_geom: txo, tyo of every launch
            ('constinttxi=cdiv(W,TS),tyi=cdiv(H,TS);', 1),
            ('constinttxi=cdiv(Wk,TS),tyi=cdiv(Hk,TS);', 1),
            ('constintHo=H-KF+1,Wo=W-KF+1;', 1),
            ('l.g[k]=map_geom(l.d.H[k],l.d.W[k]);', 1),
            ('for(intk=1;k<MS_SCALES;++k){l.d.H[k]=(l.d.H[k-1]+1)/2;l.d.W[k]=(l.d.W[k-1]+1)/2;}', 1),
            ('DL4DS_REQUIRE(((H+7)/8)>=KF&&((W+7)/8)>=KF,', 1),
            ('__launch_bounds__(64)ms_means_kernel(', 1),
            ('for(intk=threadIdx.x;k<tiles;k+=64){', 1),
            ('for(intnc=threadIdx.x;nc<NC;nc+=256){', 1),
            ('constfloatpw[MS_SCALES]={' + ','.join(f'{v}f' for v in K.MS_POWERS) + '};', 1),
            (f'constintnba=(int)std::min<size_t>(cdivz(n0,256),{K.MS_APPLY_CAP});', 1),
            (f'autoew=[](size_tn){{return(int)std::max<size_t>(1,std::min<size_t>(cdivz(n,256),{K.MS_EW_CAP}));}};', 1),
            ('DL4DS_LAUNCH(ms_pool_kernel,dim3(ew(n)),dim3(256)', 2),
            ('DL4DS_LAUNCH(ms_unpool_add_kernel,dim3(ew(n)),dim3(256)', 1),
            ('DL4DS_LAUNCH(compact_partials_kernel<2>,dim3(COMPACT_G),dim3(256),0,s,gcp,(int)gcp_total,part2);', 1),
            ('constsize_tchunk=(per+gridDim.x-1)/gridDim.x;', 1),
            ('for(size_te=e0+threadIdx.x;e<e1;e+=256){', 1),
            ('constdoublex0=a[0],y0=b[0];', 1),
            ('DL4DS_LAUNCH(met_pair_partial_kernel,dim3(MET_CHUNKS,N),dim3(256)', 1),
            ('DL4DS_LAUNCH(met_pair_finish_kernel,dim3(cdiv(N,64)),dim3(64)', 1),
            ('DL4DS_LAUNCH(met_assemble_kernel,dim3(cdiv(N,64)),dim3(64)', 1),
            (f'dim3((unsigned)std::min<size_t>(cdivz(per,256),{K.MET_GRID_CAP})),dim3(256)', 1),
            ('if(st->maxP>st->maxT)dpred[st->argmaxP]+=ddr;', 1),                          # route_range_and_shift
            ('if(st->minP<st->minT)dpred[st->argminP]-=ddr;', 1),
            ('if(st->minP<0.f)dpred[st->argminP]-=sumdy;', 1),
            ('route_range_and_shift(st,', 2),
            ('constfloatshT=(shift&&st->minT<0.f)?st->minT:0.f,shP=(shift&&st->minP<0.f)?st->minP:0.f;', 1),
            ('returnPivot{st->pivT,st->pivP,st->pivT-shT,st->pivP-shP};', 1),
            ('constPivotpv=pivot_of(st,true);', 1),
            ('constfloatpT=raw?st->pivT:0.f,pP=raw?st->pivP:0.f;', 1),                    # the one backward tile kernel
            ('constPivotpv=pivot_of(st,shift!=0);', 1),
            ('st->pivT=(float)(r.sd[0][0]*inv_n);st->pivP=(float)(r.sd[1][0]*inv_n);', 1)):
        assert d.count(piece) == count, (piece, d.count(piece))
    tree = 'for(into=128;o>0;o>>=1)'                 # the block reduction tree has one home: block_tree of common.h
    assert d.count(tree) == 0 and _src('dl4ds_amd', 'csrc', 'common.h').count(tree) == 1
    capi = _src('dl4ds_amd', 'csrc', 'capi.cpp')
    assert 'loss_forward_backward(S(),kind,yt,yp,dpred,N,H,W,C,scale,loss_dev,accumulate,scratch(ws),ws);' in capi
    losses = _src('dl4ds_amd', 'csrc', 'losses.hip')
    for piece in ('dssim_forward_backward(s,y_true,y_pred,dpred,N,H,W,C,scale*wd,loss_out,1,',
                  'msdssim_forward_backward(s,y_true,y_pred,dpred,N,H,W,C,scale*wm,loss_out,1,',
                  'scale*wa*inv_n,scale*ws*inv_n,accumulate,workspace);'):
        assert piece in losses, piece


# ------------------------------------------------------------------------------------------------------------ second trips
def test_every_long_loop_takes_a_second_trip_in_some_case():
    g = {c.id: K.dssim_geom(c.shape) for c in K.LONG_CASES}
    assert g['long-minmax']['mm'] == dict(nb=512, trips=2, finish_trips=2)
    assert g['long-compact']['nbf'] == 20000 and g['long-compact']['compact_fwd'] == dict(chunk=313, trips=2)
    assert len(K.compact_second_trip_rows(20000)) == 63 * 57 + (20000 - 63 * 313 - 256)
    assert g['long-compact']['mm']['trips'] == 19
    for cid, (imax, imin) in K.LATE.items():
        n = g[cid]['n']
        assert imin == n - 1 and imax < n
        assert K.mm_block(imax, n) >= 256                                  # the finish loop's second trip holds the maximum
    n = g['long-minmax']['n']
    assert K.mm_trip(K.LATE['long-minmax'][1], n) == 1 and K.mm_block(K.LATE['long-minmax'][1], n) < 256
    n = g['long-compact']['n']
    assert K.mm_trip(K.LATE['long-compact'][0], n) == 10 and K.mm_trip(K.LATE['long-compact'][1], n) == 18
    ms = {c.id: K.ms_geom(c.shape) for c in K.MS_CASES}
    assert ms['ms-tiles81']['tiles'][0] == 81 and ms['ms-tiles81']['means_trips'][0] == 2
    lg = ms['ms-long']
    assert lg['gcp_total'] == 530 * 31 > 16384 and lg['compact']['trips'] == 2
    assert lg['combine_trips'] == 3 and lg['apply_trips'] >= 2 and lg['nba'] == 2048
    assert lg['unpool_trips'][0] == 2 and max(lg['pool_trips']) == 1       # 530 samples do not reach the pooling loop's second trip
    assert ms['ms-pool']['pool_trips'][0] == 2 and K.ms_geom((1247, 81, 81, 1))['pool_trips'][0] == 1
    met = {c.id: K.met_geom(c.shape) for c in K.MET_CASES}
    assert met['pairs65']['pair_blocks'] == 2 and met['pairs130-c2']['pair_blocks'] == 3
    assert met['chunk258']['chunk'] == 258 and met['chunk258']['partial_trips'] == 2
    assert met['tiles81']['tiles'] == 81 and met['tiles81']['means_trips'] == 2
    assert met['grid-trip']['grid_blocks'] == 4096 and met['grid-trip']['grid_trips'] == 2
    assert met['grid-trip']['mm']['trips'] > 2 and met['grid-trip']['partial_trips'] > 2
    assert met['empty-chunks']['chunk'] == 1 and met['empty-chunks']['empty_chunks'] == 34
    assert not met['no-window']['has_ssim'] and not met['empty-chunks']['has_ssim']


def test_every_tile_edge_class_is_met_twice():
    cases = K.TILE_CASES + K.LONG_CASES + [K.LossCase('route', 'dssim', K.ROUTE_SHAPE, '')]
    shapes = sorted({c.shape for c in cases if c.kind == 'dssim'})
    assert set(K.TILE_SHAPES) <= set(shapes)

    def count(pred):
        return sum(bool(pred(*s)) for s in shapes)
    classes = {
        'map of one pixel': lambda N, H, W, C: K.map_size(H, W) == (1, 1),
        'map narrower than a tile': lambda N, H, W, C: 1 < min(K.map_size(H, W)) < K.TS,
        'map of exactly one tile': lambda N, H, W, C: K.TS in K.map_size(H, W),
        'map one over a tile': lambda N, H, W, C: K.TS + 1 in K.map_size(H, W),
        'input of exactly one tile': lambda N, H, W, C: K.TS in (H, W),
        'input one over a tile': lambda N, H, W, C: K.TS + 1 in (H, W),
        'several tiles each way, backward': lambda N, H, W, C: min(K.tiles_bwd(H, W)) >= 2,
        'N = 1': lambda N, H, W, C: N == 1,
        'C = 3': lambda N, H, W, C: C == 3,
    }
    for name, pred in classes.items():
        assert count(pred) >= 2, name
    ms_shapes = sorted({c.shape for c in K.LOSS_CASES if c.kind.startswith('msdssim')})
    assert sum(81 in s[1:3] for s in ms_shapes) >= 2 and sum(88 in s[1:3] for s in ms_shapes) >= 2
    assert [h for h, _ in K.pyramid(81, 81)] == [81, 41, 21, 11] and [h for h, _ in K.pyramid(88, 88)] == [88, 44, 22, 11]
    assert K.map_size(*K.pyramid(81, 81)[-1]) == (1, 1)
    assert all(h % 2 for h, _ in K.pyramid(81, 81)) and not any(h % 2 for h, _ in K.pyramid(88, 88)[:-1])
    mixes = {k: sum(c.kind == k for c in K.TILE_CASES) for k in ('dssim_mae', 'dssim_mse', 'dssim_mae_mse')}
    assert min(mixes.values()) >= 2


# ---------------------------------------------------------------------------------------- restatements against the oracle
@pytest.mark.parametrize('case', [c for c in K.TILE_CASES if c.kind == 'dssim'][:4], ids=lambda c: c.id)
def test_dssim_restatement_is_the_oracle(case):
    yt, yp = K.loss_inputs(case)
    assert K.dssim_value(yt, yp) == pytest.approx(K.loss_ref(case)[0], rel=1e-12)


@pytest.mark.parametrize('case', [c for c in K.MS_CASES if c.kind == 'msdssim'][:3], ids=lambda c: c.id)
def test_msdssim_restatement_is_the_oracle(case):
    yt, yp = K.loss_inputs(case)
    assert K.msdssim_value(K.ms_means(yt, yp)) == pytest.approx(K.loss_ref(case)[0], rel=1e-12)


# ------------------------------------------------------------------------------------------------------------- sensitivity
def test_losing_the_late_extremes_moves_the_loss():
    for case in K.LONG_CASES:
        yt, yp = K.loss_inputs(case)
        n = yt.size
        e = np.arange(n)
        ref = K.loss_ref(case)[0]
        assert K.dssim_value(yt, yp) == pytest.approx(ref, rel=1e-12)
        first_grid_trip = e < K.mm_geom(n)['nb'] * K.THREADS
        first_finish_trip = (e // K.THREADS) % K.mm_geom(n)['nb'] < K.THREADS
        for keep in (first_grid_trip, first_finish_trip):
            assert not keep.all()
            lost = K.dssim_value(yt, yp, stats=K.stats_of(yt, yp, keep))
            assert abs(lost - ref) >= FACTOR * _loss_tol(ref), (case.id, lost, ref)


def test_losing_the_compaction_second_trip_moves_the_loss():
    case = K.LONG_CASES[1]
    yt, yp = K.loss_inputs(case)
    keep = np.ones(K.dssim_geom(case.shape)['nbf'], bool)
    keep[K.compact_second_trip_rows(keep.size)] = False
    ref = K.loss_ref(case)[0]
    assert abs(K.dssim_value(yt, yp, keep_tiles=keep) - ref) >= FACTOR * _loss_tol(ref)


def test_losing_planes_or_tiles_moves_the_multiscale_loss():
    by_id = {c.id: c for c in K.MS_CASES}
    case = by_id['ms-long']
    ref = K.loss_ref(case)[0]
    means = K.ms_means(*K.loss_inputs(case))
    assert K.msdssim_value(means) == pytest.approx(ref, rel=1e-12)
    lost = K.msdssim_value(means, keep_planes=np.arange(K.ms_geom(case.shape)['NC']) < K.THREADS)
    assert abs(lost - ref) >= FACTOR * _loss_tol(ref)
    case = by_id['ms-tiles81']
    ref = K.loss_ref(case)[0]
    lost = K.msdssim_value(K.ms_means(*K.loss_inputs(case), keep_tiles0=np.arange(81) < 64))
    assert abs(lost - ref) >= FACTOR * _loss_tol(ref)


def test_losing_the_pooling_second_trip_moves_the_multiscale_loss():
    """ms-pool, on its last 13 samples (the only ones the second trip writes): with their first pooled level left at zero beyond
    element 8192 x 256 the loss of the whole batch moves by more than 10 x its bound."""
    case = next(c for c in K.MS_CASES if c.id == 'ms-pool')
    yt, yp = K.loss_inputs(case)
    g = K.ms_geom(case.shape)
    first = K.MS_EW_CAP * K.THREADS
    h1, w1 = g['dims'][1]
    n_first = first // (h1 * w1)                                   # samples wholly written by the first trip
    assert case.shape[0] - n_first == 13 and g['n'][1] - first == 20908
    x, q, drange = K.shifted(yt, yp, K.stats_of(yt, yp))
    x, q = x[n_first:], q[n_first:]

    def value(lose):
        ms, mc = [], []
        a, b = x, q
        for k in range(K.MS_SCALES):
            if k:
                a, b = K._pool(a), K._pool(b)
                if k == 1 and lose:
                    a, b = a.copy(), b.copy()
                    a.reshape(-1)[first - n_first * h1 * w1:] = 0.0
                    b.reshape(-1)[first - n_first * h1 * w1:] = 0.0
            s, cs = K.ssim_maps(a, b, drange)
            ms.append(s.mean(axis=(1, 2)))
            mc.append(cs.mean(axis=(1, 2)))
        v = [np.maximum(mc[k], 0.0) ** K.MS_POWERS[k] for k in range(3)] + [np.maximum(ms[3], 0.0) ** K.MS_POWERS[3]]
        return np.prod(v, axis=0).sum()
    ref = K.loss_ref(case)[0]
    moved = 0.5 * abs(value(True) - value(False)) / g['NC']
    assert moved >= FACTOR * _loss_tol(ref), (moved, ref)


def test_losing_pairs_elements_tiles_or_grid_points_moves_the_metrics():
    by_id = {c.id: c for c in K.MET_CASES}
    for cid in ('pairs65', 'pairs130-c2'):                          # an unwritten pair reads 0: the whole value is the error
        ref = K.met_ref(by_id[cid])[0]
        for k in ('mae', 'mse', 'pearson', 'ssim'):
            assert np.all(np.abs(ref[k][64:]) > 0.05), (cid, k)
    case = by_id['chunk258']
    y, p = (np.asarray(a, np.float64).reshape(case.shape[0], -1) for a in K.met_inputs(case))
    ref = K.met_ref(case)[0]
    g = K.met_geom(case.shape)
    keep = (np.arange(g['per']) % g['chunk']) < K.THREADS
    assert (~keep).sum() == 2 * 64
    d = (p - y) * keep
    x, z = y * keep, p * keep
    per = g['per']
    mx, my = x.sum(1) / per, z.sum(1) / per
    cov, vx, vy = (x * z).sum(1) / per - mx * my, (x * x).sum(1) / per - mx * mx, (z * z).sum(1) / per - my * my
    for k, lost in (('mae', np.abs(d).sum(1) / per), ('mse', (d * d).sum(1) / per), ('pearson', cov / np.sqrt(vx * vy))):
        assert np.all(np.abs(lost - ref[k]) >= FACTOR * K.TOL_PAIR * np.abs(ref[k])), k
    case = by_id['tiles81']
    y, p = K.met_inputs(case)
    ref = K.met_ref(case)[0]
    s, _ = K.ssim_maps(y, p, ref['drange'])
    assert s.mean(axis=(1, 2, 3)) == pytest.approx(ref['ssim'], rel=1e-12)
    lost = (s * K.tile_mask(s.shape, np.arange(81) < 64)).sum(axis=(1, 2, 3)) / s[0].size
    assert np.all(np.abs(lost - ref['ssim']) >= FACTOR * K.TOL_SSIM * np.abs(ref['ssim']))
    case = by_id['grid-trip']
    ref = K.met_ref(case)[0]
    tail = slice(K.MET_GRID_CAP * K.THREADS, None)
    assert ref['rmse_map'].reshape(-1)[tail].size == 1024
    for k in ('rmse_map', 'bias_map', 'pearson_map'):               # unwritten grid points read 0
        v = np.abs(ref[k].reshape(-1)[tail])
        assert np.median(v) >= FACTOR * (K.TOL_MAP['atol'] + K.TOL_MAP['rtol'] * np.median(v)), k


def test_scale_and_accumulate_cases_are_sensitive():
    """a result without the scale, without the preload or without the gradient is off by more than 10 x the bound"""
    for case in K.SCALE_CASES:
        ref, g, _ = K.loss_ref(case)
        for s in K.SCALES:
            assert abs(s * ref - ref) >= FACTOR * _loss_tol(s * ref)
    for case in K.ACCUMULATE_CASES:
        g = K.loss_ref(case)[1]
        pre = K.preload(case)
        assert np.abs(pre).max() >= FACTOR * K.TOL_GRAD * np.abs(g).max()
        assert 4 * np.finfo(np.float32).eps * np.abs(pre).max() <= 0.1 * K.TOL_GRAD * np.abs(g).max()       # the preload's rounding


# ------------------------------------------------------------------------------------------------------ ties and branches
def _extremes(a):
    flat = np.asarray(a).reshape(-1)
    return flat.min(), int((flat == flat.min()).sum()), flat.max(), int((flat == flat.max()).sum())


def _check_margins(yt, yp, exact=()):
    """no branch of the kernels sits on an equality: sign of either minimum, order of the minima, of the maxima"""
    minT, _, maxT, _ = _extremes(yt)
    minP, _, maxP, _ = _extremes(yp)
    for name, v in (('minT', minT), ('minP', minP), ('min', minP - minT), ('max', maxP - maxT)):
        v = float(v)
        if name in exact:
            assert v == 0.0, (name, v)
        else:
            assert abs(v) > K.BRANCH_MARGIN, (name, v)


@pytest.mark.parametrize('case', K.LOSS_CASES, ids=lambda c: c.id)
def test_loss_cases_have_no_tie_and_no_close_branch(case):
    yt, yp = K.loss_inputs(case)
    assert yt.dtype == np.float32 and yp.dtype == np.float32
    _, nmin, _, nmax = _extremes(yp)
    assert nmin == 1 and nmax == 1
    _check_margins(yt, yp)
    if case.variant == 'late_extremes':
        flat = yp.reshape(-1)
        assert (int(flat.argmax()), int(flat.argmin())) == K.LATE[case.id]
    minT, minP = float(yt.min()), float(yp.min())
    want = dict(positive=(False, False), negative_min=(True, True), pred_sets_range=(False, True),
                late_extremes=(False, True))[case.variant]
    assert (minT < 0, minP < 0) == want
    if case.variant != 'positive':
        assert minP < minT                                            # the lower end of the range reaches the prediction
    if case.variant in ('pred_sets_range', 'late_extremes'):
        assert yp.max() > yt.max()                                    # ... and the upper end


@pytest.mark.parametrize('route', K.ROUTE_CASES, ids=lambda r: r.id)
def test_routing_cases_are_what_they_are_named_for(route):
    yt, yp = K.route_inputs(route.id)
    minT, _, maxT, _ = _extremes(yt)
    minP, nmin, maxP, nmax = _extremes(yp)
    flat = yp.reshape(-1)
    exact = {'max-equal': ('max',), 'min-equal': ('min',), 'pred-min-zero': ('minP',)}.get(route.id, ())
    _check_margins(yt, yp, exact)
    assert (nmin, nmax) == {'tied-max': (1, 2), 'tied-min': (2, 1)}.get(route.id, (1, 1))
    if route.id == 'true-neg-pred-pos':
        assert minT < 0 <= minP
    if route.id == 'pred-neg-true-pos':
        assert minP < 0 <= minT
    if route.id == 'last-max':
        assert flat.argmax() == flat.size - 1
    if route.id == 'last-min':
        assert flat.argmin() == flat.size - 1
    if route.id.startswith('tied'):
        assert K.R_PRED < K.R_PRED2 and flat[K.R_PRED] == flat[K.R_PRED2] and K.R_PRED2 // (27 * 17) == 1
    plain, nudged = K.route_ref(route.id, False), K.route_ref(route.id, True)
    assert nudged[0] == pytest.approx(plain[0], rel=1e-7)                    # the nudge moves nothing but the tie
    tol = K.TOL_GRAD * np.abs(nudged[1]).max()
    diff = np.abs(nudged[1] - plain[1]).reshape(-1)
    if route.tie is None:
        assert diff.max() == 0.0
    elif route.tie[0] == 'true':
        # torch.maximum / minimum halve a tie: the even split differs from the product's convention at the prediction's extreme,
        # by half the range term -- 5 x the gradient bound here, enough to tell the two conventions apart
        i = int(flat.argmax() if route.tie[1] == 'max' else flat.argmin())
        assert diff[i] >= 3.0 * tol and np.delete(diff, i).max() <= 1e-4 * tol
    else:
        assert diff[K.R_PRED] >= FACTOR * tol and diff[K.R_PRED2] >= FACTOR * tol
        assert np.delete(diff, [K.R_PRED, K.R_PRED2]).max() <= 1e-4 * tol
        assert nudged[1].reshape(-1)[[K.R_PRED, K.R_PRED2]].sum() == pytest.approx(plain[1].reshape(-1)[[K.R_PRED, K.R_PRED2]].sum(),
                                                                                    rel=1e-6)


# ------------------------------------------------------------------------------------------------------------ field classes
_SMOOTH01 = ('smooth01', 'smooth-err', 'scale1e4', 'scale1e-3')          # the rescaled target's minimum is exactly 0: no shift either side


@pytest.mark.parametrize('case', K.FIELD_CASES, ids=lambda c: c.id)
def test_field_cases_are_what_they_are_named_for(case):
    """finite float64 reference in well under a second; unique selections; the class's own property"""
    cls = K.field_class(case)
    yt, yp = K.loss_inputs(case)
    assert yt.dtype == np.float32 and yp.dtype == np.float32 and not yt.flags.writeable and not yp.flags.writeable
    ref, gref, seconds = K.loss_ref(case)
    assert np.isfinite(ref) and np.isfinite(gref).all() and seconds < 0.5
    minT, _, maxT, _ = _extremes(yt)
    minP, nmin, maxP, nmax = _extremes(yp)
    drange = float(max(maxT, maxP)) - float(min(minT, minP))
    if cls == 'constant-both':
        assert np.ptp(yt) == 0 and np.ptp(yp) == 0 and minP > maxT > 0          # the tie of the maxima: K._loss_ref
        return
    assert (nmin, nmax) == (1, 1)
    if cls == 'identical':
        assert yt.tobytes() == yp.tobytes() and ref == 0.0
        _check_margins(yt, yp, ('minT', 'minP', 'min', 'max'))
        return
    _check_margins(yt, yp, ('minT',) if cls in _SMOOTH01 else ())
    if cls in ('kelvin', 'pascal', 'offset1000'):
        assert min(minT, minP) > 0 and float(yt.mean()) / drange >= 4.0
    elif cls == 'celsius':
        assert minP < minT < 0 and maxT > 0
    elif cls == 'mixed-sign':
        assert minT > 0 and (yp < 0).sum() == 1 and float(yt.mean()) / drange > 0.75
    elif cls == 'near-constant':
        assert np.ptp(yt) == 0 and minP < minT < maxP
    elif cls.startswith('scale'):
        base = next(c for c in K.FIELD_CASES if c.kind == case.kind and K.field_class(c) == 'smooth01')
        s = {'scale1e4': 1e4, 'scale1e-3': 1e-3}[cls]
        np.testing.assert_array_equal(yt, K.loss_inputs(base)[0] * np.float32(s))
        if case.kind in ('dssim', 'msdssim'):          # SSIM does not see the scale; the gradient goes with 1 / scale
            assert ref == pytest.approx(K.loss_ref(base)[0], rel=1e-5)
            assert np.abs(gref).max() * s == pytest.approx(np.abs(K.loss_ref(base)[1]).max(), rel=1e-3)


@pytest.mark.parametrize('case', K.FIELD_CASES, ids=lambda c: c.id)
def test_pivoted_float32_moments_hold_a_quarter_of_the_bounds(case):
    """the bounds of the GPU test are attainable by straightforward float32 code on every field case"""
    loss_err, grad_err = K.field_errors(case, True)
    print(f'{case.id}: pivoted float32, loss {loss_err:.2e} of its bound, gradient {grad_err:.2e} of max |ref|')
    assert loss_err <= 0.25
    if K.field_class(case) in K.ZERO_GRAD_CLASSES:
        # nothing to be relative to: the restatement's own largest entry is the GPU test's yardstick, and it is small
        # against a typical gradient of the smooth01 case of the same kind
        base = next(c for c in K.FIELD_CASES if c.kind == case.kind and K.field_class(c) == 'smooth01')
        typical = np.median(np.abs(K.loss_ref(base)[1]))
        print(f'{case.id}: largest float32 entry {K.identical_grad32(case):.2e}, typical smooth01 entry {typical:.2e}')
        assert 0.0 < 10.0 * K.identical_grad32(case) <= 1e-3 * typical
    else:
        assert grad_err <= 0.25 * K.TOL_GRAD


_PURE_OFFSET = [c for c in K.FIELD_CASES if K.field_class(c) in K.OFFSET_CLASSES and c.kind in ('dssim', 'msdssim')]


@pytest.mark.parametrize('case', _PURE_OFFSET, ids=lambda c: c.id)
def test_raw_float32_moments_miss_the_bounds_on_the_offset_classes(case):
    """The cases discriminate: moments of the values themselves (what the kernels formed before the pivot) miss both bounds on the
    SSIM terms of kelvin, pascal and offset1000, and a bound on near-constant's multi-scale loss.  (The mixes carry the same SSIM
    term beside pixel terms that raw float32 gets right, so their totals may pass.  near-constant at one scale passes too in the
    kernels' filter order: the target 0.5 is a power of two, every product with a tap is exact and the target's side leaves no
    residue -- 1.9e-2 of the loss bound, 7.6e-5 of the gradient's; the pooled scales do not have that luck.)"""
    loss_err, grad_err = K.field_errors(case, False)
    print(f'{case.id}: raw float32, loss {loss_err:.2e} of its bound, gradient {grad_err:.2e} of max |ref|')
    if K.field_class(case) != 'near-constant':
        assert loss_err > 1.0 and grad_err > K.TOL_GRAD
    elif case.kind == 'msdssim':
        assert loss_err > 1.0 or grad_err > K.TOL_GRAD


def test_field_classes_each_have_both_loss_families():
    for cls in K.FIELD_CLASSES:
        kinds = {c.kind for c in K.FIELD_CASES if K.field_class(c) == cls}
        assert any(k.startswith('dssim') for k in kinds) and any(k.startswith('msdssim') for k in kinds), cls
    assert {c.shape for c in K.FIELD_CASES} == set(K.FIELD_SHAPES.values())
    assert K.pyramid(81, 88)[-1] == (11, 11) and K.pyramid(80, 88)[-1][0] < K.KF          # 81: the least height with four scales
    assert K.tiles_fwd(27, 43) == (3, 2) and (43 - K.KF + 1) % K.TS != 0                    # two and more tile columns, ragged
    om = np.ones(K.FIELD_SHAPES['dssim'][1:3])
    om[K.FIELD_MASK_BLOCK] = 0.0
    full = [(y, x) for y in range(17) for x in range(33) if not om[y:y + 11, x:x + 11].any()]
    assert len(full) == 7 * 10                                                               # windows the weighted case excludes


def test_field_accumulate_case_is_sensitive():
    case = K.FIELD_ACCUMULATE_CASE
    g = K.loss_ref(case)[1]
    pre = K.field_preload(case)
    assert np.abs(pre).max() >= FACTOR * K.TOL_GRAD * np.abs(g).max()
    assert 4 * np.finfo(np.float32).eps * np.abs(pre).max() <= 0.1 * K.TOL_GRAD * np.abs(g).max()       # the preload's rounding
    assert np.isfinite(K.loss_ref(K.FIELD_NULL_GRAD_CASE)[0]) and K.loss_ref(K.FIELD_NULL_GRAD_CASE)[1] is None


def test_metric_offset_cases_assert_ssim():
    assert all(c.ssim for c in K.MET_OFFSET_CASES) and len(K.MET_OFFSET_CASES) == 8
    for c in K.MET_CASES:
        if c.id in ('const-point', 'const-pair'):
            assert c.ssim == bool(np.isfinite(K.met_ref(c)[0]['ssim']).all())


# --------------------------------------------------------------------------------------------- the pair sums of the metrics
def test_float_partials_of_raw_moments_miss_the_bound_and_the_pivot_keeps_it():
    worst_raw, worst_pivot = 0.0, 0.0
    for case in K.MET_OFFSET_CASES:
        y, p = K.met_inputs(case)
        ref = K.met_ref(case)[0]['pearson']
        raw = np.abs(K.pair_pearson_sim(y, p, False) / ref - 1).max()
        piv = np.abs(K.pair_pearson_sim(y, p, True) / ref - 1).max()
        print(f'{case.id}: raw moments {raw:.1e}, with the pivot {piv:.1e}')
        if case.mean / case.sd >= 280:                              # at (280, 5) a draw may stay below the bound (1.3e-5 and 2.6e-5 here)
            assert raw > K.TOL_PAIR, (case.id, raw)                  # what the kernel did before the pivot
        assert piv < K.TOL_PAIR / FACTOR, (case.id, piv)
        worst_raw, worst_pivot = max(worst_raw, raw), max(worst_pivot, piv)
    print(f'per-pair Pearson, float partials: raw moments {worst_raw:.1e}, with the pivot {worst_pivot:.1e}')
    for case in K.MET_SHAPE_CASES[:3]:                               # data of mean 1 and sd 2 passed before and passes now
        y, p = K.met_inputs(case)
        ref = K.met_ref(case)[0]['pearson']
        assert np.abs(K.pair_pearson_sim(y, p, True) / ref - 1).max() < K.TOL_PAIR / FACTOR


def test_degenerate_metric_cases():
    by_id = {c.id: c for c in K.MET_CASES}
    y, p = K.met_inputs(by_id['const-pair'])
    assert np.ptp(y[1]) == 0 and np.ptp(p[2]) == 0 and np.ptp(y[0]) > 0 and np.ptp(p[1]) > 0
    sim = K.pair_pearson_sim(y, p, True)
    assert sim[1] == 0.0 and sim[2] == 0.0                           # exact zero moments of the constant side
    ref = K.met_ref(by_id['const-pair'])[0]['pearson']
    assert np.isnan(ref[1]) and np.isnan(ref[2]) and np.isfinite(ref[[0, 3]]).all()
    ref = K.met_ref(by_id['const-point'])[0]['pearson_map']
    assert np.isnan(ref[K.MET_CONST_POINT]) and np.isnan(ref).sum() == 1
    assert np.isnan(K.met_ref(by_id['one-pair'])[0]['pearson_map']).all()


# -------------------------------------------------------------------------------------------------------------------- time
def test_reference_times():
    """every float64 reference the GPU tests call, timed on the CPU (the caches make the GPU tests pay each once)"""
    rows = [(c.id, K.loss_ref(c)[2]) for c in K.LOSS_CASES] + [(c.id, K.met_ref(c)[1]) for c in K.MET_CASES]
    rows += [(r.id, K.route_ref(r.id)[2]) for r in K.ROUTE_CASES]
    rows.sort(key=lambda r: -r[1])
    print('float64 references, seconds: ' + ', '.join(f'{i} {s:.2f}' for i, s in rows[:8]) + f'; all {sum(s for _, s in rows):.1f}')
    assert rows[0][1] < 30.0
