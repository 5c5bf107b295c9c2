"""Op-level tests of every kernel of csrc/head.hip against the numpy references of tests/head_ref.py: the counter-based dropout noise
(dropout_mask_kernel and the seeds it is given), the two dropout apply kernels, Dense forward / backward, and the three forward and
three backward kernels of GlobalAveragePooling -- each through a graph of one to three ops, driven through GraphBuilder / Model /
SupervisedEngine.  Gradients are read where the kernel under test (or, for the pooling, the 1x1 convolution in front of it) wrote
them: parameter gradients, and the gradient buffer of a graph input created with requires_grad.

Dense and GAP are compared per element with head_ref.sum_bound -- (K + 2) * 2^-24 * sum|terms| + 4 ulp(|ref|), K the length of that
element's sum -- so that a wrong small entry cannot hide behind a large neighbour.  The backward references are the fp64 value of the
kernel's own operands: the float32 forward output the device produced (dense_bwd_kernel reads it for the activation derivative, the
loss kernel for dL/dy) and dL/dy = 2 * (y - t) / size with the float32 difference y - t (head_ref.mse_targets).  No element is ever
left out of a comparison; the inputs keep every ReLU pre-activation 1e-4 away from 0 (tests/test_head_oracle.py asserts it).

Left to the CGAN step tests (tests/test_gpu_models.py), which are the only way to reach them: dense_bwd_kernel with b0 > 0 and with
acc_dw, and the batch halves (b_off > 0) of gap_backward and of the dropout backward."""
import ctypes

import numpy as np
import pytest

from tests import head_cases as K
from tests import head_ref as R

pytestmark = pytest.mark.gpu

F32, F64 = np.float32, np.float64


# ------------------------------------------------------------------------------------------------------------------- plumbing
def _builder():
    from dl4ds_amd.graph import GraphBuilder
    return GraphBuilder()


def _keras(t):
    return (t.H, t.W, t.C) if t.nmul == 1 else (t.nmul, t.H, t.W, t.C)


def _model(g, out, xs, weights=None):
    from dl4ds_amd.graph import Model
    g.finalize(out, seed=0)
    m = Model(g, 'head', [_keras(x) for x in xs])
    if weights:
        m.set_weights(weights)
    return m


def _read(g, t, batch, grad=1):
    from dl4ds_amd import _lib
    p = ctypes.c_void_p()
    _lib.check(_lib.lib().dl4ds_graph_tensor_ptr(g.h, t.id, int(grad), ctypes.byref(p)))
    assert p.value, 'tensor has no such buffer'
    a = np.empty((batch * t.nmul, t.H, t.W, t.C), F32)
    _lib.check(_lib.lib().dl4ds_memcpy_d2h(a.ctypes.data, p, a.nbytes))
    return a


def _engine(m):
    from dl4ds_amd.training import SupervisedEngine
    return SupervisedEngine(m, loss='mse', learning_rate=1e-3)


def _within(got, ref, bound, what):
    got = np.asarray(got, F64).reshape(np.shape(ref))
    ratio, i, gv, rv = R.worst(got, ref, bound)
    print(f'{what}: worst error / bound {ratio:.3f} at flat element {i} (got {gv!r}, reference {rv!r})')
    assert np.isfinite(got).all() and ratio <= 1.0, (what, ratio, i, gv, rv)


# ------------------------------------------------------------------------------------------------------------------- noise
def _noise_graph(shape, rates, variant):
    b, h, w, c = shape
    g = _builder()
    x = g.input(h, w, c)
    t = x
    for k, rate in enumerate(rates):
        t = g.dropout(t, rate, f'drop{k}', variant=variant)
    assert g.dropout_count() == len(rates)
    return g, _model(g, t, [x]), np.ones(shape, F32)


def _draw(g, m, x, draws):
    """Training-mode forward passes 1 .. max(draws) -> {(op, draw): noise}."""
    out = {}
    for k in range(1, max(draws) + 1):
        m([x], training=True)
        if k in draws:
            for i in range(g.dropout_count()):
                out[i, k] = g.dropout_mask(i, x.shape[0])
    return out


@pytest.mark.parametrize('seed', K.RESEEDS)
@pytest.mark.parametrize('shape', [K.LARGE_MASK, K.SMALL_MASK])
def test_keep_masks_are_the_documented_function_of_the_seed(shape, seed):
    """After reseed_dropout(s) the keep masks of ops 0 .. 2 at draws 1 .. 3 equal the numpy replica of the documented scheme bit for
    bit; the large mask has more elements than one grid of dropout_mask_kernel (second trip of its grid-stride loop)."""
    n = K.mask_size(shape)
    assert (n > K.NOISE_GRID_THREADS) == (shape == K.LARGE_MASK)
    rate = 0.4
    g, m, x = _noise_graph(shape, [rate] * K.N_OPS, None)
    m.reseed_dropout(seed)
    got = _draw(g, m, x, K.DRAWS)
    for (i, k), mask in got.items():
        assert mask.size == n
        np.testing.assert_array_equal(mask, R.keep_mask(R.op_seed(seed, i), k, n, rate), err_msg=f'op {i} draw {k}')


@pytest.mark.parametrize('seed', K.RESEEDS)
@pytest.mark.parametrize('shape', [K.LARGE_MASK, K.SMALL_MASK])
def test_gaussian_noise_against_fp64(shape, seed):
    """GaussianDropout noise after reseed_dropout(s) against the fp64 replica: absolute error at most 1e-5 * sigma (1 - u and 2 * u2
    are exact in fp32, logf / sqrtf / cospif within 2 ulp each and r <= sqrt(48 ln 2) = 5.77 give about 3e-6 * sigma)."""
    n, rate = K.mask_size(shape), 0.4
    sigma = R.gaussian_sigma(rate)
    g, m, x = _noise_graph(shape, [rate] * K.N_OPS, 'gaussian')
    m.reseed_dropout(seed)
    got = _draw(g, m, x, K.DRAWS)
    worst = (0.0, None)
    for (i, k), mask in got.items():
        err = np.abs(mask.astype(F64) - R.gaussian_mask(R.op_seed(seed, i), k, n, rate))
        e = int(np.argmax(err))
        worst = max(worst, (float(err[e]), (i, k, e)))
    print(f'gaussian noise: largest error {worst[0] / sigma:.3e} * sigma at (op, draw, element) {worst[1]}')
    assert worst[0] <= 1e-5 * sigma, worst


@pytest.mark.parametrize('variant', [None, 'gaussian'])
def test_noise_frequencies(variant):
    """One op per rate on the large mask, built-in seeds: keep fraction within 6 binomial standard deviations of
    1 - ceil(rate * 2^24) / 2^24; Gaussian mean within 6 sigma / sqrt(n) of 1 and variance within 6 sigma^2 sqrt(2 / n) of sigma^2."""
    n = K.mask_size(K.LARGE_MASK)
    g, m, x = _noise_graph(K.LARGE_MASK, K.RATES, variant)
    got = _draw(g, m, x, (1,))
    for i, rate in enumerate(K.RATES):
        a = got[i, 1].astype(F64)
        if variant is None:
            p = R.keep_probability(rate)
            assert set(np.unique(a)) <= {0.0, 1.0}
            print(f'rate {rate}: keep fraction {a.mean():.6f}, expected {p:.6f}')
            assert abs(a.mean() - p) <= 6.0 * np.sqrt(p * (1.0 - p) / n), (rate, a.mean(), p)
        else:
            sigma = R.gaussian_sigma(rate)
            print(f'rate {rate}: mean {a.mean():.6f}, variance {a.var():.6f}, sigma^2 {sigma ** 2:.6f}')
            assert abs(a.mean() - 1.0) <= 6.0 * sigma / np.sqrt(n), (rate, a.mean())
            assert abs(a.var() - sigma ** 2) <= 6.0 * sigma ** 2 * np.sqrt(2.0 / n), (rate, a.var(), sigma ** 2)


@pytest.mark.parametrize('reseed', [False, True], ids=['builtin', 'reseeded'])
@pytest.mark.parametrize('variant', [None, 'gaussian'])
def test_noise_streams_are_independent(variant, reseed):
    """Three dropout ops with masks of 65 536 elements at rate 0.5, draws 1 .. 3: nine streams.  For every pair of distinct streams
    and every lag in -8 .. 8 (612 comparisons) the agreement fraction of the keep masks is within 6 binomial standard deviations of
    0.5 (+-0.0117), the correlation of the Gaussian noise below 6 / sqrt(n).  A stream that is a shifted copy of another scores 1.0:
    with the un-hashed built-in seeds op i + 1 drew op i's mask shifted by one element.  Then the streams against the replica: a graph
    that was never reseeded draws as if reseeded with the built-in seed."""
    g, m, x = _noise_graph(K.INDEP_MASK, [K.INDEP_RATE] * K.N_OPS, variant)
    if reseed:
        m.reseed_dropout(K.INDEP_RESEED)
    got = _draw(g, m, x, K.DRAWS)
    streams = [got[i, k] for i in range(K.N_OPS) for k in K.DRAWS]
    assert all(s.size == K.mask_size(K.INDEP_MASK) for s in streams)
    bad, count = (R.agreement_violations if variant is None else R.correlation_violations)(streams)
    assert count == 612
    assert not bad, f'{len(bad)} of {count} (stream, stream, lag, score, bound): {bad[:6]}'
    seed_of_op = (lambda i: R.op_seed(K.INDEP_RESEED, i)) if reseed else R.builtin_seed
    for got_s, want in zip(streams, K.replica_streams(seed_of_op, streams[0].size, K.INDEP_RATE, variant == 'gaussian')):
        if variant is None:
            np.testing.assert_array_equal(got_s, want)
        else:
            assert np.abs(got_s.astype(F64) - want).max() <= 1e-5 * R.gaussian_sigma(K.INDEP_RATE)


# ------------------------------------------------------------------------------------------------------------------- dropout apply
def _ulp_close(got, ref, ulps, what):
    got = np.asarray(got, F64).reshape(ref.shape)
    _within(got, ref, ulps * R.ulp(ref), what)


def _apply_case(variant, shape, rate, dim=None, skip=False, seed=3):
    """input -> dropout [-> add(dropout, input)] on a (B, T, H, W, C) tensor with an injected mask: inference pass, training forward
    (bitwise), backward (dX at the graph input)."""
    b, t, h, w, c = shape
    gaussian = variant in ('gaussian', 'mcgaussiandrop')
    spatial = variant in ('spatial', 'mcspatialdrop')
    mc = variant is not None and variant.startswith('mc')
    g = _builder()
    xin = g.input(h, w, c, nmul=t, requires_grad=True)
    d = g.dropout(xin, rate, 'drop', variant=variant, dim=dim or 2)
    out = g.add(d, xin) if skip else d
    m = _model(g, out, [xin])
    x = np.random.default_rng(seed).standard_normal(shape).astype(F32)
    xs = x.reshape((b,) + _keras(xin))
    mshape = {None: shape, 2: (b * t, c), 3: (b, c)}[dim if spatial else None]
    mask = (K.gaussian_noise if gaussian else K.irregular_keep)(mshape, seed + 1, rate)
    if skip:
        assert (mask >= 0).all()            # (both terms of dX keep dY's sign: no cancellation under the 2 ulp bound)
    else:
        assert gaussian or 0 < mask.mean() < 1
    full = R.broadcast_mask(mask, shape, dim if spatial else None)
    scale = R.dropout_scale(rate, gaussian)
    want = R.dropout_forward(x, full, scale)
    assert want.dtype == F32
    if skip:
        want = want + x

    # inference: identity for the plain variants; the MC* variants stay active (and take the injected noise)
    y0 = m([xs])
    assert g.dropout_mask(0, b).size == mask.size == (t * h * w * c * b if not spatial else (b * t * c if dim == 2 else b * c))
    if mc:
        g.set_dropout_mask(0, b, mask)
        y0 = m([xs])
    np.testing.assert_array_equal(y0.reshape(shape), want if mc else (x + x if skip else x), err_msg='inference')

    g.set_dropout_mask(0, b, mask)
    y = m([xs], training=True)
    np.testing.assert_array_equal(g.dropout_mask(0, b), mask.ravel())
    np.testing.assert_array_equal(y.reshape(shape), want, err_msg='training forward')

    tgt, _ = R.mse_targets(y, seed + 2)
    g.set_dropout_mask(0, b, mask)
    _engine(m).loss_and_grads([xs], tgt)
    dy = _read(g, out, b).reshape(shape)
    assert np.abs(dy).min() > 0
    dx = _read(g, xin, b).reshape(shape)
    ref = R.dropout_backward(dy, full, scale)
    _ulp_close(dx, ref + dy.astype(F64) if skip else ref, 2 if skip else 1, f'dX {variant} skip={skip}')


@pytest.mark.parametrize('variant', [None, 'gaussian', 'mcdrop', 'mcgaussiandrop'])
def test_dropout_apply(variant):
    """dropout_apply_kernel (six blocks): training forward float32(float32(x * mask) * scale) bitwise with an irregular keep mask /
    Gaussian noise, dX = dY * mask * scale within 1 ulp, inference a bitwise copy (plain) or the training formula (MC*)."""
    _apply_case(variant, (3, 1, 9, 11, 5), 0.4)


@pytest.mark.parametrize('variant,rate', [(None, 0.4), ('gaussian', 0.05), ('spatial', 0.4)])
def test_dropout_backward_accumulates(variant, rate):
    """The input also feeds a skip Add, whose backward writes the input's gradient first: the dropout backward accumulates, within
    2 ulp of the fp64 sum dY + dY * mask * scale (Gaussian noise at a rate whose noise stays positive)."""
    _apply_case(variant, (2, 3, 7, 9, 5) if variant == 'spatial' else (3, 1, 9, 11, 5), rate, dim=2, skip=True)


@pytest.mark.parametrize('dim', [2, 3])
@pytest.mark.parametrize('variant', ['spatial', 'mcspatialdrop'])
def test_spatial_dropout_apply(variant, dim):
    """dropout_apply_bcast_kernel on a (B=2, T=3, 7x9, C=5) tensor: SpatialDropout2D draws one mask entry per (frame, channel)
    (mask (B * T, C)), SpatialDropout3D one per (sample, channel) shared over the frames (mask (B, C)); the size dropout_mask reports,
    forward and backward against the numpy broadcast."""
    _apply_case(variant, (2, 3, 7, 9, 5), 0.4, dim=dim)


def test_dropout_rate_zero_is_the_input_tensor():
    g = _builder()
    x = g.input(4, 4, 3)
    assert g.dropout(x, 0.0) is x and g.dropout(x, 0, variant='mcdrop') is x and g.dropout(x, None) is x
    assert g.dropout_count() == 0


# ------------------------------------------------------------------------------------------------------------------- Dense
def _dense_check(grads, dx, x, heads, dy, names):
    """heads: [(w, b, act, y_dev slice)]; the shared input's dX is the sum over the heads (K and the terms add up)."""
    dx_ref, dx_terms, k = 0.0, 0.0, 0
    for (w, b, act, y), dyh, name in zip(heads, dy, names):
        ref = R.dense_backward(x, w, y, dyh, act)
        _within(grads[name + '/kernel'], *ref['dW'], f'{name} dW')
        _within(grads[name + '/bias'], *ref['db'], f'{name} db')
        dx_ref = dx_ref + ref['dX'][0]
        dx_terms = dx_terms + np.abs(ref['dz'][0]) @ np.abs(w.astype(F64)).T
        k += w.shape[1]
    _within(dx, dx_ref, R.sum_bound(k, dx_terms, dx_ref), 'dX')


@pytest.mark.parametrize('act', R.ACTS)
@pytest.mark.parametrize('case', K.DENSE_CASES)
def test_dense(case, act):
    """input(1, 1, Cin[, nmul]) -> Dense(F, act), MSE: y, dW, db and dX per element against fp64."""
    b, cin, f, nmul = case
    x, w, bias, _ = K.dense_case_inputs(case)
    g = _builder()
    xin = g.input(1, 1, cin, nmul=nmul, requires_grad=True)
    out = g.dense(xin, 'd', f, activation=act)
    m = _model(g, out, [xin], {'d/kernel': w, 'd/bias': bias})
    xs = x.reshape((b,) + _keras(xin))
    y = m([xs])
    z, y_ref, bound = R.dense_forward(x, w, bias, act)
    _within(y, y_ref, bound, 'y')
    y2 = y.reshape(y_ref.shape)
    if act == 'relu':
        np.testing.assert_array_equal(y2 > 0, z > 0)
    tgt, dy = R.mse_targets(y, 5)
    _, grads = _engine(m).loss_and_grads([xs], tgt)
    _dense_check(grads, _read(g, xin, b), x, [(w, bias, act, y2)], [dy.reshape(y2.shape)], ['d'])


@pytest.mark.parametrize('case', K.DENSE_SHARED_CASES)
def test_dense_shared_input_accumulates_dx(case):
    """One tensor feeds two Dense heads whose outputs are concatenated: the head created first runs its backward last, finds the
    input's gradient written and takes the acc_dx branch; dX is the sum of both heads'."""
    b, cin, (f1, a1), (f2, a2) = case
    x, heads, _ = K.dense_shared_inputs(case)
    g = _builder()
    xin = g.input(1, 1, cin, requires_grad=True)
    out = g.concat([g.dense(xin, 'h1', f1, activation=a1), g.dense(xin, 'h2', f2, activation=a2)])
    m = _model(g, out, [xin], {'h1/kernel': heads[0][0], 'h1/bias': heads[0][1], 'h2/kernel': heads[1][0], 'h2/bias': heads[1][1]})
    xs = x.reshape(b, 1, 1, cin)
    y = m([xs])
    y2 = y.reshape(b, f1 + f2)
    parts = [y2[:, :f1], y2[:, f1:]]
    for (w, bias), act, yp in zip(heads, (a1, a2), parts):
        z, y_ref, bound = R.dense_forward(x, w, bias, act)
        _within(yp, y_ref, bound, 'y')
        if act == 'relu':
            np.testing.assert_array_equal(yp > 0, z > 0)
    tgt, dy = R.mse_targets(y, 6)
    dy = dy.reshape(b, f1 + f2)
    _, grads = _engine(m).loss_and_grads([xs], tgt)
    _dense_check(grads, _read(g, xin, b), x, [(heads[0][0], heads[0][1], a1, parts[0]), (heads[1][0], heads[1][1], a2, parts[1])],
                 [dy[:, :f1], dy[:, f1:]], ['h1', 'h2'])


# ------------------------------------------------------------------------------------------------------------------- GAP
@pytest.mark.parametrize('case', K.GAP_FWD_CASES)
def test_gap_forward(case):
    """gap_fwd_kernel / gap_partial_kernel<4 | 1> + gap_finish_kernel on means of O(10 .. 100): relative error below 1e-5 per element
    (a pixel dropped or counted twice moves a mean by 1 / HW >= 1.2e-4; the fp32 chains give about 3e-6)."""
    n, t, h, w, c, over_time = case
    x = K.gap_fwd_input(case)
    g = _builder()
    xin = g.input(h, w, c, nmul=t)
    out = g.gap(xin, over_time=over_time)
    m = _model(g, out, [xin])
    y = m([x.reshape((n,) + _keras(xin))])
    ref = R.gap_forward(x, over_time)
    rel = np.abs(y.reshape(ref.shape).astype(F64) - ref) / np.abs(ref)
    i = int(np.argmax(rel))
    print(f'gap forward {case}: largest relative error {rel.flat[i]:.3e} at flat element {i}')
    assert y.size == ref.size and np.isfinite(y).all() and rel.max() < 1e-5, (rel.flat[i], i)


@pytest.mark.parametrize('case', K.GAP_BWD_CASES)
def test_gap_backward(case):
    """input -> Conv2D(1x1, bias[, ReLU]) = feat -> pooling [twice, concatenated], MSE.  The pooling's backward writes
    dfeat = dy / HW where feat > 0 (gap_bwd4_kernel / gap_bwd_masked_kernel with the ReLU mask), or everywhere (gap_bwd4_kernel without a
    mask / gap_bwd_kernel), accumulating when feat's gradient is already written; db, dW and dX of the convolution per element
    against fp64."""
    n, t, h, w, cin, c, relu, over_time, twice = case
    x, wk, bias, _ = K.gap_bwd_inputs(case)
    g = _builder()
    xin = g.input(h, w, cin, nmul=t, requires_grad=True)
    feat = g.conv2d(xin, 'pre', c, 1, use_bias=True, activation='relu' if relu else None)
    out = g.gap(feat, 'gap', over_time=over_time)
    if twice:
        out = g.concat([out, g.gap(feat, 'gap2', over_time=over_time)])
    m = _model(g, out, [xin], {'pre/kernel': wk.reshape(1, 1, cin, c), 'pre/bias': bias})
    xs = x.reshape((n,) + _keras(xin))
    y = m([xs])
    z, feat_ref = R.gap_feat(x, wk, bias, relu)
    y_ref = R.gap_forward(feat_ref, over_time)
    y2 = y.reshape(y_ref.shape[:-1] + (-1,))
    hw = h * w * (t if over_time else 1)
    terms = R.gap_forward(np.abs(x.astype(F64)) @ np.abs(wk.astype(F64)) + np.abs(bias.astype(F64)), over_time)
    for part in ([y2[..., :c], y2[..., c:]] if twice else [y2]):
        _within(part, y_ref, R.sum_bound(hw + cin, terms, y_ref), 'pooled')
    tgt, dy = R.mse_targets(y, 7)
    dy = dy.reshape(y2.shape)
    _, grads = _engine(m).loss_and_grads([xs], tgt)
    ref = R.gap_backward(x, wk, z, [dy[..., :c], dy[..., c:]] if twice else [dy], over_time, relu)
    _within(grads['pre/bias'], *ref['db'], 'db')
    _within(grads['pre/kernel'], *ref['dW'], 'dW')
    _within(_read(g, xin, n), *ref['dX'], 'dX')
