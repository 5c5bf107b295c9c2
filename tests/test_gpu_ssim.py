"""Op-level tests of csrc/dssim.hip against float64 references -- runs on MI355X only.  Cases, launch restatements and references:
tests/ssim_cases.py; what the cases reach and why a wrong result could not pass: tests/test_ssim_cases.py.

  - DSSIM and its mixes at the tile edges (maps of one pixel, narrower than a tile, of one tile, one over; N = 1, C = 3) and at the
    long loops (second trips of the min/max grid stride, of its finish, of the compaction), the extremes where only a late trip reads
    them; multi-scale DSSIM at 81 x 81 (odd at every level, one-pixel coarsest map), on an even pyramid, with 81 tiles per plane,
    and at 530 and 1260 samples (compaction, ms_combine, ms_apply, unpool and pool second trips);
  - the trainers' form: scale != 1, a null gradient, accumulation onto a preloaded gradient (dl4ds_op_loss_scaled);
  - routing of the range and min-shift terms: equal extremes (tf.maximum / tf.minimum hand a tie to y_true: the prediction gets
    nothing), sign cases, extremes at the last element, tied prediction extremes (the whole term on the smallest flat index);
  - the field classes (FIELD_CASES): smooth fields, smooth errors, Kelvin-, Pascal- and 1000-offset data, Celsius (both arrays shifted),
    a shifted prediction beside an unshifted target, a constant target, two constants, identical arrays, and the smooth pair scaled by
    1e4 and 1e-3 -- at the smallest shapes, since what the values do to the 11 x 11 window moments does not depend on the grid; with
    an accumulate, a null-gradient and (tests/test_gpu_weighted_loss.py) a weighted case on the Kelvin class;
  - image_metrics on Kelvin- and Pascal-like data, across the 64-pair blocks, the 256-element chunk trips, 81 SSIM tiles, the second
    trip of the grid kernel, empty chunks, no SSIM window, and degenerate inputs.

Bounds: loss rel 2e-4 / abs 1e-6; gradients 1e-3 of max |reference|; per-pair metrics rtol 2e-5, SSIM 2e-4, maps rtol 2e-4 / atol 2e-6.
Largest errors observed on the MI355X (in units of the bound where it is not a plain relative error):
  loss (rel)              tile edges 2.7e-6, long loops 4.9e-7, multi-scale 2.9e-5, scale 7.5e-6, null gradient 4.7e-5,
                          accumulate 2.6e-5, routing 3.5e-5
  gradient (max |ref|)    tile edges 1.2e-6, long loops 8.5e-7, multi-scale 4.6e-5, scale 7.2e-5, accumulate 2.2e-5, routing 7.5e-6
  metrics, per pair (rel) mae 5.4e-8, pearson 4.4e-8 on the offset data and 8.6e-8 elsewhere, ssim 2.6e-7 (mean 1, sd 2)
  metrics, maps           rmse 2.9e-4, bias 3.0e-4, pearson 5.8e-3 of the bound
  metrics, ssim (rel)     offset data 5.7e-8, degenerate 1.1e-6
  field classes           loss, of its bound: smooth01 3.8e-2, smooth-err 3.6e-2, kelvin 3.2e-2, pascal 1.1e-2, offset1000 3.0e-3,
                          celsius 3.0e-2, mixed-sign 1.3e-2, near-constant 3.6e-4, constant-both 8.6e-4, scale 3.8e-2; gradient, of
                          max |ref|: smooth01 4.0e-5, smooth-err 3.1e-5, kelvin 3.8e-5, pascal 4.5e-6, offset1000 1.4e-6, celsius
                          2.2e-6, mixed-sign 1.2e-4, near-constant 1.6e-7, constant-both 2.1e-7, scale 3.0e-5; identical: |loss|
                          6.0e-8, largest gradient entry 2.6 x the float32 restatement's (bound: 10 x)
  the same field classes with window moments of the unpivoted values (the kernels before the pivot of csrc/dssim.hip), loss of its
  bound / gradient of max |ref|: kelvin 27 / 9.3e-3, pascal 2.9e5 / 5.5e3, offset1000 2.6e4 / 1.4e3, mixed-sign 4.5 / 2.1e-3,
  constant-both 49 / 17, identical 12 x the restatement's gradient; metrics ssim 4.1e-3 on the offset data, 0.25 on a constant pair
References on the CPU: ms-pool 8.7 s (loss only: 1260 is the smallest round batch at which the pooling loop's second trip moves the
loss by 10 x its bound; 1248 is where the trip begins), ms-long 4.2 s (530 samples as stated), grid-trip 3.5 s, all others < 0.2 s.
The per-pair Pearson of the offset cases misses its bound without the pivot of met_pair_partial_kernel (float partials of raw
moments; measured on the parent commit's arithmetic restated on the CPU: up to 1.3e-3 at (280, 1), (1000, 1) and (101325, 300),
1.3e-5 at (280, 5)).  SSIM is asserted on the offset and the constant cases like everywhere else: the window moments are taken of
pivoted values (csrc/dssim.hip), so sigma = E[x^2] - mu^2 no longer cancels at the size of the mean.
"""
import numpy as np
import pytest

from tests import ssim_cases as K

pytestmark = pytest.mark.gpu

OBSERVED = {}


@pytest.fixture(scope='module')
def ops():
    import dl4ds_amd.ops as o
    return o


def _note(group, err):
    OBSERVED[group] = max(OBSERVED.get(group, 0.0), float(err))
    print(f'[ssim] {group}: {err:.3e}')


def check_loss(group, a, ref):
    _note(group + ' loss (rel)', abs(a - ref) / abs(ref))
    assert a == pytest.approx(ref, **K.TOL_LOSS)


def check_grad(group, g, ref):
    ref = np.asarray(ref, np.float64)
    g = np.asarray(g, np.float64)
    assert g.shape == ref.shape
    err = np.abs(g - ref).max() / max(np.abs(ref).max(), 1e-6)
    _note(group + ' grad (of max |ref|)', err)
    assert err < K.TOL_GRAD, f'max rel err {err:.3e}'


def run_case(ops, group, case, scale=1.0):
    yt, yp = K.loss_inputs(case)
    ref, gref, _ = K.loss_ref(case)
    a, g = ops.loss(case.kind, yt, yp, want_grad=case.grad, scale=scale)
    check_loss(group, a, scale * ref)
    if case.grad:
        check_grad(group, g, scale * gref)
    return a, g


@pytest.mark.parametrize('case', K.TILE_CASES, ids=lambda c: c.id)
def test_dssim_tile_edges(ops, case):
    run_case(ops, 'tile edges', case)


@pytest.mark.parametrize('case', K.LONG_CASES, ids=lambda c: c.id)
def test_dssim_long_loops(ops, case):
    _, g = run_case(ops, 'long loops', case)
    gref = K.loss_ref(case)[1].reshape(-1)
    for i in K.LATE[case.id]:          # the routed terms land on the late extremes
        assert abs(g.reshape(-1)[i] - gref[i]) < K.TOL_GRAD * np.abs(gref).max()


@pytest.mark.parametrize('case', K.MS_CASES, ids=lambda c: c.id)
def test_msdssim(ops, case):
    a, g = run_case(ops, 'multi-scale', case)
    yt, yp = K.loss_inputs(case)
    a2, g2 = ops.loss(case.kind, yt, yp, want_grad=case.grad)
    assert a2 == a
    if case.grad:
        np.testing.assert_array_equal(g, g2)                    # deterministic reductions


@pytest.mark.parametrize('scale', K.SCALES)
@pytest.mark.parametrize('case', K.SCALE_CASES, ids=lambda c: c.id)
def test_scale(ops, case, scale):
    run_case(ops, 'scale', case, scale)


@pytest.mark.parametrize('case', K.NULL_GRAD_CASES, ids=lambda c: c.id)
def test_null_gradient_returns_the_same_loss(ops, case):
    yt, yp = K.loss_inputs(case)
    a, g = ops.loss(case.kind, yt, yp)
    b, none = ops.loss(case.kind, yt, yp, want_grad=False)
    assert none is None and np.float32(a).tobytes() == np.float32(b).tobytes()
    check_loss('null gradient', b, K.loss_ref(case)[0])
    for scale in K.SCALES:                                      # ... and through the scaled entry
        a, _ = ops.loss(case.kind, yt, yp, scale=scale)
        b, _ = ops.loss(case.kind, yt, yp, want_grad=False, scale=scale)
        assert np.float32(a).tobytes() == np.float32(b).tobytes()


@pytest.mark.parametrize('case', K.ACCUMULATE_CASES, ids=lambda c: c.id)
def test_accumulate_into_a_preloaded_gradient(ops, case):
    yt, yp = K.loss_inputs(case)
    ref, gref, _ = K.loss_ref(case)
    pre = K.preload(case)
    a, g = ops.loss(case.kind, yt, yp, accumulate_into=pre)
    check_loss('accumulate', a, ref)
    check_grad('accumulate', g.astype(np.float64) - pre, gref)          # at the gradient's own size, the preload taken off exactly
    flat = yp.reshape(-1)
    for i in (int(flat.argmax()), int(flat.argmin())):          # the entries the scalar fix-ups go to keep their preload too
        assert abs(g.reshape(-1)[i] - float(pre.reshape(-1)[i]) - gref.reshape(-1)[i]) < K.TOL_GRAD * np.abs(gref).max()
    a1, g1 = ops.loss(case.kind, yt, yp, scale=1.0, accumulate_into=np.zeros_like(pre))
    a0, g0 = ops.loss(case.kind, yt, yp)
    assert a1 == a0
    np.testing.assert_array_equal(g1, g0)                       # scale 1 onto zeros is the plain entry, bit for bit


@pytest.mark.parametrize('route', K.ROUTE_CASES, ids=lambda r: r.id)
def test_routing_edges(ops, route):
    yt, yp = K.route_inputs(route.id)
    ref, gref, _ = K.route_ref(route.id)                         # exact ties decided the product's way (tests/ssim_cases.py)
    a, g = ops.loss('dssim', yt, yp)
    check_loss('routing', a, ref)
    check_grad('routing', g, gref)
    if route.id.startswith('tied'):
        # the convention: the whole routed term goes to the smallest flat index (TensorFlow splits it evenly).  The sum over the
        # tied entries is the reference's whatever the split; the entry at the larger index holds no routed term
        even = K.route_ref(route.id, False)[1].reshape(-1)
        tied = [K.R_PRED, K.R_PRED2]
        tol = K.TOL_GRAD * np.abs(even).max()
        assert abs(g.reshape(-1)[tied].sum() - even[tied].sum()) < tol
        routed = 2.0 * (even[K.R_PRED2] - gref.reshape(-1)[K.R_PRED2])          # the even split gave half of it to either entry
        assert abs(routed) > 20 * tol
        assert abs(g.reshape(-1)[K.R_PRED2] - (even[K.R_PRED2] - routed / 2)) < tol
        assert abs(g.reshape(-1)[K.R_PRED] - (even[K.R_PRED] + routed / 2)) < tol


# ------------------------------------------------------------------------------------------------------------ field classes
@pytest.mark.parametrize('case', K.FIELD_CASES, ids=lambda c: c.id)
def test_losses_on_field_classes(ops, case):
    """smooth, offset, shifted and degenerate fields (tests/ssim_cases.py: FIELD_CASES) at the bounds of the white-noise cases"""
    cls = K.field_class(case)
    yt, yp = K.loss_inputs(case)
    ref, gref, _ = K.loss_ref(case)
    a, g = ops.loss(case.kind, yt, yp)
    assert np.isfinite(a) and np.isfinite(g).all()
    if cls in K.ZERO_GRAD_CLASSES:
        yardstick = K.identical_grad32(case)
        _note(f'field {cls} |loss|', abs(a))
        _note(f'field {cls} max |grad| (of the float32 restatement)', np.abs(g).max() / yardstick)
        assert abs(a) <= K.TOL_LOSS['abs']
        assert np.abs(g).max() <= 10.0 * yardstick
        return
    _note(f'field {cls} loss (of the bound)', abs(a - ref) / max(K.TOL_LOSS['rel'] * abs(ref), K.TOL_LOSS['abs']))
    _note(f'field {cls} grad (of max |ref|)', np.abs(g - gref).max() / max(np.abs(gref).max(), 1e-6))
    check_loss(f'field {cls}', a, ref)
    check_grad(f'field {cls}', g, gref)


def test_field_accumulate_onto_a_preload(ops):
    case = K.FIELD_ACCUMULATE_CASE
    yt, yp = K.loss_inputs(case)
    ref, gref, _ = K.loss_ref(case)
    pre = K.field_preload(case)
    a, g = ops.loss(case.kind, yt, yp, accumulate_into=pre)
    check_loss('field accumulate', a, ref)
    check_grad('field accumulate', g.astype(np.float64) - pre, gref)          # the preload taken off exactly


def test_field_null_gradient(ops):
    case = K.FIELD_NULL_GRAD_CASE
    yt, yp = K.loss_inputs(case)
    b, none = ops.loss(case.kind, yt, yp, want_grad=False)
    a, _ = ops.loss(case.kind, yt, yp)
    assert none is None and np.float32(a).tobytes() == np.float32(b).tobytes()
    check_loss('field null gradient', b, K.loss_ref(case)[0])


# ------------------------------------------------------------------------------------------------------------ image_metrics
def check_metrics(group, case, m, ref, pairs=None):
    """every key of image_metrics at the existing bounds; ``pairs``: the pairs whose Pearson is compared (default: all)"""
    assert m['drange'] == pytest.approx(ref['drange'], rel=1e-6)
    for k in ('mae', 'mse', 'rmse', 'psnr', 'pearson'):
        a, r = (m[k], ref[k]) if pairs is None or k != 'pearson' else (m[k][pairs], ref[k][pairs])
        _note(f'{group} {k} (rel)', np.abs(a / r - 1).max())
        np.testing.assert_allclose(a, r, rtol=K.TOL_PAIR, err_msg=k)
    for k in ('rmse_map', 'bias_map', 'pearson_map'):
        ok = np.isfinite(ref[k])
        np.testing.assert_array_equal(np.isnan(m[k]), ~ok, err_msg=k)
        err = np.abs(m[k][ok] - ref[k][ok]) / (K.TOL_MAP['atol'] + K.TOL_MAP['rtol'] * np.abs(ref[k][ok]))
        if err.size:
            _note(f'{group} {k} (of the bound)', err.max())
        np.testing.assert_allclose(m[k][ok], ref[k][ok], **K.TOL_MAP, err_msg=k)
    if not K.met_geom(case.shape)['has_ssim']:
        assert np.isnan(m['ssim']).all() and np.isnan(ref['ssim']).all()
    else:
        assert case.ssim
        _note(f'{group} ssim (rel)', np.abs(m['ssim'] / ref['ssim'] - 1).max())
        np.testing.assert_allclose(m['ssim'], ref['ssim'], rtol=K.TOL_SSIM, err_msg='ssim')


@pytest.mark.parametrize('case', K.MET_OFFSET_CASES, ids=lambda c: c.id)
def test_image_metrics_offset_data(case):
    from dl4ds_amd.metrics import image_metrics
    y, p = K.met_inputs(case)
    check_metrics('offset data', case, image_metrics(y, p), K.met_ref(case)[0])


@pytest.mark.parametrize('case', K.MET_SHAPE_CASES, ids=lambda c: c.id)
def test_image_metrics_trips_and_edges(case):
    from dl4ds_amd.metrics import image_metrics
    y, p = K.met_inputs(case)
    m = image_metrics(y, p)
    check_metrics('metric shapes', case, m, K.met_ref(case)[0])
    m2 = image_metrics(y, p)
    for k in ('mae', 'mse', 'pearson'):
        np.testing.assert_array_equal(m[k], m2[k])              # bitwise reproducible


def test_image_metrics_one_pair():
    from dl4ds_amd.metrics import image_metrics
    case = next(c for c in K.MET_CASES if c.id == 'one-pair')
    m = image_metrics(*K.met_inputs(case))
    assert np.isnan(m['pearson_map']).all()
    check_metrics('degenerate', case, m, K.met_ref(case)[0])


def test_image_metrics_constant_grid_point():
    from dl4ds_amd.metrics import image_metrics
    case = next(c for c in K.MET_CASES if c.id == 'const-point')
    m = image_metrics(*K.met_inputs(case))
    assert np.isnan(m['pearson_map'][K.MET_CONST_POINT]) and np.isnan(m['pearson_map']).sum() == 1
    check_metrics('degenerate', case, m, K.met_ref(case)[0])


def test_image_metrics_constant_pair():
    """A pair with a constant side has no correlation; dl4ds_amd.metrics documents 0.0 for it (the float64 restatement: NaN)."""
    from dl4ds_amd.metrics import image_metrics
    case = next(c for c in K.MET_CASES if c.id == 'const-pair')
    m = image_metrics(*K.met_inputs(case))
    assert m['pearson'][1] == 0.0 and m['pearson'][2] == 0.0
    check_metrics('degenerate', case, m, K.met_ref(case)[0], pairs=[0, 3])


def test_zz_report():
    print('[ssim] largest errors: ' + '; '.join(f'{k} {v:.1e}' for k, v in sorted(OBSERVED.items())))
