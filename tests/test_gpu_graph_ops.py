"""Op-level, bit-exact tests of the kernels that move activations and gradients between the convolutions: Concatenate (concat_join /
concat_split and the per-slice view_axpy / view_axpy_masked fallback), Add (add_act, view_axpy, masked_axpy, masked_axpy_pair),
Activation (act_forward / act_backward), slice / crop / zero padding, repeat_time and MaxPooling2D (maxpool2_forward /
maxpool2_backward) -- each through a one- or two-op graph.

How the gradient is made exact (tests/graph_ops_cases.py): the MAE loss writes dY = g * sign(pred - target) with g = 1 / size; the
targets are ``forward - s`` for a +-1 pattern s, so dY = g * s and the expected gradient of a copy op is a selection of g * s.  g is
taken from the result (one non-zero magnitude, within 1 ulp of 1 / size); sums of two such terms are exact for any g, longer sums
use a power-of-two size or the kernel's documented summation order.  Gradients are read from the buffer the kernel under test
wrote (dl4ds_graph_tensor_ptr(grad=1)), never through a convolution.  ReLU masks come from a bias-free 1x1 identity-kernel
Conv2D(activation='relu') in front of an input: its output relu(x) is exact for the integer inputs and takes grad_masked.
"""
import ctypes

import numpy as np
import pytest

from tests import graph_ops_cases as K
from tests.parity import kernel_tags

pytestmark = pytest.mark.gpu

F32 = np.float32


# ------------------------------------------------------------------------------------------------------------------- plumbing
def _builder():
    from dl4ds_amd.graph import GraphBuilder
    return GraphBuilder()


def _relu_id(g, x, name):
    return g.conv2d(x, name, x.C, 1, use_bias=False, activation='relu')


def _model(g, out, xs):
    from dl4ds_amd.graph import Model
    g.finalize(out, seed=0)
    m = Model(g, 'graph_ops', [tuple(x.shape[1:]) for x in xs])
    for k, p in g.params.items():
        c = p['shape'][-1]
        m.set_weights({k: np.eye(c, dtype=F32).reshape(1, 1, c, c)})
    return m


def _read(g, t, batch, grad):
    from dl4ds_amd import _lib
    p = ctypes.c_void_p()
    _lib.check(_lib.lib().dl4ds_graph_tensor_ptr(g.h, t.id, int(grad), ctypes.byref(p)))
    assert p.value, 'tensor has no such buffer'
    a = np.empty((batch * t.nmul, t.H, t.W, t.C), F32)
    _lib.check(_lib.lib().dl4ds_memcpy_d2h(a.ctypes.data, p, a.nbytes))
    return a


def _run(g, out, xs, grads_of, seed=11, dense_dy=True):
    """forward through Model, backward through SupervisedEngine.loss_and_grads('mae') with targets forward - s
    -> (forward, s, gradients of ``grads_of``, forward tags, forward + backward tags, g).  g is taken from the output's gradient
    buffer as the loss kernel left it: one non-zero magnitude, within 1 ulp of 1 / size, and dY = g * s (``dense_dy=False``: or 0,
    for an output whose own ReLU backward has masked dY in place)."""
    from dl4ds_amd.training import SupervisedEngine
    m = _model(g, out, xs)
    y, tf = kernel_tags(lambda: m(xs))
    s = K.signs(y.shape, seed)
    eng = SupervisedEngine(m, loss='mae', learning_rate=1e-3)
    _, tb = kernel_tags(lambda: eng.loss_and_grads(xs, y - s))
    batch = xs[0].shape[0]
    dy = _read(g, out, batch, 1).reshape(y.shape)
    nz = np.abs(dy[dy != 0])
    assert nz.size, 'dY is all zero'
    gu, ideal = F32(nz.min()), F32(1) / F32(y.size)
    assert nz.max() == gu, 'dY has more than one non-zero magnitude'
    assert abs(np.float64(gu) - np.float64(ideal)) <= np.spacing(ideal), (gu, ideal)
    ok = dy == gu * s
    assert ok.all() if dense_dy else (ok | (dy == 0)).all()
    return y, s, [_read(g, t, batch, 1) for t in grads_of], tf, tb, gu


def _eq(got, want, what=''):
    np.testing.assert_array_equal(got, np.asarray(want, F32), err_msg=what)


# ------------------------------------------------------------------------------------------------------------------- Concatenate
def _concat_case(monkeypatch, chans, grid, relu=(), dup=False, again=False, seed=1):
    """concat of one input per entry of ``chans`` (``relu``: indices with the ReLU identity convolution in front; ``dup``: the last
    entry is the first tensor once more; ``again``: the result is concatenated with the first tensor once more, so that tensor's
    gradient is already written when the inner Concatenate's backward runs).  Checks forward and every gradient bitwise."""
    monkeypatch.setenv('DL4DS_NO_CONCAT_ALIAS', '1')
    n, h, w = grid
    g = _builder()
    parts, vals, xs = [], [], []
    for k, c in enumerate(chans):
        if dup and k == len(chans) - 1:
            assert c == chans[0]
            parts.append(parts[0]); vals.append(vals[0])
            continue
        t = g.input(h, w, c, requires_grad=True)
        x = K.hashed_ints((n, h, w, c), seed * 100 + k, zeros=k in relu)
        xs.append(x)
        parts.append(_relu_id(g, t, f'id{k}') if k in relu else t)
        vals.append(np.maximum(x, 0) if k in relu else x)
    out = g.concat(parts)
    order = list(range(len(parts)))
    if again:
        out = g.concat([out, parts[0]])
        order.append(0)
    uniq = parts[:-1] if dup else parts
    y, s, grads, tf, tb, gu = _run(g, out, xs, uniq)
    _eq(y, np.concatenate([vals[k] for k in order], axis=-1), 'forward')
    off, want = 0, [np.zeros_like(v) for v in vals[:len(uniq)]]
    for k in order:
        c = vals[k].shape[-1]
        tgt = 0 if (dup and k == len(chans) - 1) else k
        want[tgt] = want[tgt] + gu * s[..., off:off + c]
        off += c
    for k, (got, wk) in enumerate(zip(grads, want)):
        _eq(got, np.where(vals[k] > 0, wk, 0) if k in relu else wk, f'gradient of input {k}')
    return tf, tb


ONEPASS_CHANS = [(16, 8, 2), (5, 3, 1, 4), (4, 4), (1, 1)]
ONEPASS_VEC = {(16, 8, 2): (2, 13), (5, 3, 1, 4): (1, 13), (4, 4): (2, 4), (1, 1): (1, 2)}


@pytest.mark.parametrize('grid', [(2, 9, 7), (1, 3, 2)])
@pytest.mark.parametrize('chans', ONEPASS_CHANS)
def test_concat_one_pass(monkeypatch, chans, grid):
    """Two to four dense graph inputs: forward is ONE concat_join launch, backward ONE concat_split launch (ConcatOp: wide tensor and
    every input dense, 2 <= copies <= 4).  V = 2 iff the pitch and every slice offset and width are even: (16, 8, 2) -> V 2, cvn 13;
    (5, 3, 1, 4) -> V 1, four slices at odd offsets, cvn 13; (4, 4) -> V 2, cvn 4; (1, 1) -> V 1, cvn 2."""
    assert K.concat_onepass_vec(chans) == ONEPASS_VEC[chans]
    tf, tb = _concat_case(monkeypatch, chans, grid)
    assert tf.get('concat_join') == 1 and 'view_axpy' not in tf
    assert tb.get('concat_split') == 1 and 'view_axpy' not in tb and 'view_axpy_masked' not in tb


@pytest.mark.parametrize('chans', ONEPASS_CHANS)
def test_concat_one_pass_second_iteration(monkeypatch, chans):
    """The same launches with 1.25 .. 1.5 x (8192 * 256) vector elements, so a quarter of the threads take the (pix, cv) step of
    concat_join_kernel<V> / concat_split_kernel<V>: cvn 13 (step_cv != 0, wraps) for V = 2 and V = 1, cvn 4 and 2 (powers of two:
    step_cv == 0) for V = 2 and V = 1.  (5, 3, 1, 4) runs with a ReLU mask on two slices and the first tensor concatenated once
    more behind the result, i.e. four slices with mask and accumulation past the first iteration."""
    v, cvn = K.concat_onepass_vec(chans)
    grid = K.large_grid(cvn)
    assert K.is_large(grid[0] * grid[1] * grid[2] * cvn)
    four = chans == (5, 3, 1, 4)
    tf, tb = _concat_case(monkeypatch, chans, grid, relu=(0, 2) if four else (), again=four)
    assert tf.get('concat_join') == (2 if four else 1)
    assert tb.get('concat_split') == (2 if four else 1) and 'view_axpy_masked' not in tb


@pytest.mark.parametrize('chans,relu', [((16, 8, 2), (0, 2)), ((5, 3, 1, 4), (1, 3)), ((4, 4), (0, 1)), ((5, 3, 1, 4), (0, 1, 2, 3))])
def test_concat_one_pass_relu_mask(monkeypatch, chans, relu):
    """Inputs behind a ReLU identity convolution are grad_masked (one consumer, a Concatenate): concat_split applies the mask,
    expected where(x > 0, slice, 0) with exact zeros in x; V = 2 and V = 1."""
    tf, tb = _concat_case(monkeypatch, chans, (2, 9, 7), relu=relu)
    assert tf.get('concat_join') == 1 and tb.get('concat_split') == 1 and 'view_axpy_masked' not in tb


@pytest.mark.parametrize('chans,relu', [((4, 8, 4), ()), ((3, 2, 3), ()), ((4, 8, 4), (0,)), ((3, 2, 3), (0, 1))])
def test_concat_same_tensor_twice(monkeypatch, chans, relu):
    """concat([a, b, a]): the gradient of a is the sum of its two slices, {-2g, 0, 2g}.  One concat_split launch cannot form it (two
    slices of one launch would store into the same buffer), so ConcatOp's backward takes the per-slice copies, the second one
    accumulating: view_axpy / view_axpy_masked."""
    tf, tb = _concat_case(monkeypatch, chans, (2, 9, 7), relu=relu, dup=True)
    assert tf.get('concat_join') == 1
    assert 'concat_split' not in tb and tb.get('view_axpy', 0) + tb.get('view_axpy_masked', 0) >= 3


@pytest.mark.parametrize('chans,relu', [((16, 8, 2), ()), ((5, 3, 1, 4), (0, 3)), ((4, 4), (0,))])
def test_concat_one_pass_accumulate(monkeypatch, chans, relu):
    """concat([concat([a, ...]), a]): the outer split writes a's gradient first, the inner split's slice of a accumulates
    (ConcatSlice::accumulate = grad_written), with and without a's ReLU mask: {-2g, 0, 2g}."""
    tf, tb = _concat_case(monkeypatch, chans, (2, 9, 7), relu=relu, again=True)
    assert tf.get('concat_join') == 2 and tb.get('concat_split') == 2


def _slice_variants(chans, npix):
    ld, off, out = sum(chans), 0, []
    for c in chans:
        out.append((K.view_axpy_variant(c, c, 0, ld, off, npix)[0], K.view_axpy_masked_variant(c, ld, off)))
        off += c
    return out


FALLBACK = [
    # chans, relu, variant of every unmasked copy, variant of the masked copies
    ((16, 4, 4, 4, 4), (), 'strided4', None),
    ((2, 6, 2, 4, 2), (), 'small2', None),
    ((3, 4, 2, 8, 1), (), 'small1', None),
    ((16, 4, 4, 4, 4), (0, 2), 'strided4', 'masked4'),
    ((3, 4, 2, 8, 1), (0, 3), 'small1', 'generic'),       # masked operands of 3 channels, and of 8 at offset 9
    ((2, 6, 2, 4, 2), (1,), 'small2', 'generic'),         # masked operand with C % 4 != 0
]


def _check_fallback(monkeypatch, chans, relu, plain, masked, grid, **kw):
    npix = grid[0] * grid[1] * grid[2]
    for k, (pv, mv) in enumerate(_slice_variants(chans, npix)):
        assert pv == plain
        if k in relu:
            assert mv == masked
    tf, tb = _concat_case(monkeypatch, chans, grid, relu=relu, **kw)
    assert 'concat_join' not in tf and tf.get('view_axpy') == 5
    assert 'concat_split' not in tb
    assert tb.get('view_axpy') == 5 + (5 - len(relu)) and tb.get('view_axpy_masked', 0) == len(relu)


@pytest.mark.parametrize('grid', [(2, 9, 7), (1, 3, 2)])
@pytest.mark.parametrize('chans,relu,plain,masked', FALLBACK)
def test_concat_per_slice(monkeypatch, chans, relu, plain, masked, grid):
    """Five inputs exceed the four-slice limit of the one-pass kernels: forward is one view_axpy per input into its slice view,
    backward one view_axpy (unmasked) or view_axpy_masked (ReLU input) out of it.  view_axpy on a slice: strided float4 iff C, both
    pitches and the slice offset are multiples of 4 ((16, 4, 4, 4, 4): ld 32); else float2 iff all of them are even ((2, 6, 2, 4, 2):
    ld 16, the 4-wide slice sits at offset 10); else one float ((3, 4, 2, 8, 1): ld 18).  view_axpy_masked: the strided float4
    kernel under the same rule, else the generic view_masked_axpy_kernel (C % 4 != 0, or an unaligned slice)."""
    _check_fallback(monkeypatch, chans, relu, plain, masked, grid)


@pytest.mark.parametrize('chans,relu,plain,masked,widest', [
    ((16, 4, 4, 4, 4), (0,), 'strided4', 'masked4', (16, 4)),     # c4n 4: step_c4 == 0
    ((12, 4, 4, 4, 8), (0,), 'strided4', 'masked4', (12, 4)),     # c4n 3: wraps
    ((2, 6, 2, 4, 2), (), 'small2', None, (6, 2)),                # cvn 3
    ((2, 8, 2, 2, 2), (), 'small2', None, (8, 2)),                # cvn 4 (8 channels at offset 2: no float4)
    ((3, 4, 2, 8, 1), (), 'small1', None, (8, 1)),                # cvn 8
    ((3, 4, 2, 5, 1), (), 'small1', None, (5, 1)),                # cvn 5
])
def test_concat_per_slice_second_iteration(monkeypatch, chans, relu, plain, masked, widest):
    """The per-slice kernels past their first grid-stride iteration, the size rule counted on the widest slice: strided_axpy4_kernel
    (forward) and strided_masked_axpy4_kernel (backward of the ReLU input) with c4n 4 and 3, strided_axpy_small_kernel<2> with cvn 4
    and 3, strided_axpy_small_kernel<1> with cvn 8 and 5 (forward and backward)."""
    c, v = widest
    assert c == max(chans)
    grid = K.large_grid(c // v)
    assert K.is_large(grid[0] * grid[1] * grid[2] * (c // v))
    _check_fallback(monkeypatch, chans, relu, plain, masked, grid)


# ------------------------------------------------------------------------------------------------------------------- Add (+ ReLU)
def _add_case(shape, relu_out, mask_a, mask_b, mode='ab', seed=3):
    """mode 'ab': a + b; 'aa': a + a; 'again': (a + b) + a, so a's gradient is written before the first Add's backward."""
    n, h, w, c = shape
    g = _builder()
    ta, tb_ = g.input(h, w, c, requires_grad=True), g.input(h, w, c, requires_grad=True)
    a, b = K.hashed_ints(shape, seed * 100, zeros=True), K.hashed_ints(shape, seed * 100 + 1, zeros=True)
    hit = K.hashed_ints(shape, seed * 100 + 2) > 40
    b[hit] = -a[hit]                                   # sums of exactly 0 (under the ReLU: on the kink)
    pa = _relu_id(g, ta, 'ida') if mask_a else ta
    pb = _relu_id(g, tb_, 'idb') if mask_b else tb_
    va, vb = (np.maximum(a, 0) if mask_a else a), (np.maximum(b, 0) if mask_b else b)
    if mode == 'aa':
        out, ysum, ca, cb = g.add(pa, pa, relu=relu_out), va + va, 2, 0
    elif mode == 'again':
        out, ysum, ca, cb = g.add(g.add(pa, pb), pa, relu=relu_out), (va + vb) + va, 2, 1
    else:
        out, ysum, ca, cb = g.add(pa, pb, relu=relu_out), va + vb, 1, 1
    assert (ysum == 0).any() and (va == 0).any()
    want_y = np.maximum(ysum, 0) if relu_out else ysum
    y, s, (ga, gb), tf, tb, gu = _run(g, out, [a, b], [pa, pb], dense_dy=not relu_out)
    _eq(y, want_y, 'forward')
    dy = gu * s * (want_y > 0) if relu_out else gu * s
    _eq(ga, F32(ca) * dy * (va > 0) if mask_a else F32(ca) * dy, 'gradient of a')
    if cb:
        _eq(gb, dy * (vb > 0) if mask_b else dy, 'gradient of b')
    return tf, tb


@pytest.mark.parametrize('relu_out', [False, True])
@pytest.mark.parametrize('shape,variant', [((2, 9, 7, 4), 'flat4'), ((1, 3, 5, 3), 'small1'), ((1, 3, 5, 2), 'small2')])
def test_add_plain_operands(shape, variant, relu_out):
    """add_act forward = fl(a + b) [max(., 0)], operand values and sums of exactly 0 included; backward into plain operands is one
    view_axpy each: flat float4 when n % 4 == 0, else the strided small kernels (n = 45: one float; n = 30: float2)."""
    assert K.view_axpy_variant(shape[3], shape[3], 0, shape[3], 0, shape[0] * shape[1] * shape[2])[0] == variant
    tf, tb = _add_case(shape, relu_out, False, False)
    assert tf.get('add_act') == 1 and tb.get('view_axpy') == 2 and 'masked_axpy' not in tb


@pytest.mark.parametrize('relu_out', [False, True])
@pytest.mark.parametrize('shape,mask_a,mask_b,launches', [
    ((2, 9, 7, 4), True, True, 1),        # both masked, distinct, n % 4 == 0: masked_axpy_pair (one launch)
    ((1, 3, 5, 3), True, True, 2),        # n % 4 != 0: the pair kernel declines, masked_axpy's scalar branch twice
    ((2, 9, 7, 4), True, False, 1),       # one masked operand: masked_axpy's float4 branch (+ view_axpy for the plain one)
    ((1, 3, 5, 3), False, True, 1),       # ... its scalar branch
])
def test_add_relu_conv_operands(shape, mask_a, mask_b, launches, relu_out):
    """Operands that are ReLU outputs whose only consumer is the Add take grad_masked: AddOp's backward folds where(x > 0, ., 0)
    into the copy -- masked_axpy4_pair_kernel, masked_axpy4_kernel or masked_axpy1_kernel as listed."""
    tf, tb = _add_case(shape, relu_out, mask_a, mask_b)
    assert tf.get('add_act') == 1 and tb.get('masked_axpy') == launches
    assert tb.get('view_axpy', 0) == (0 if mask_a and mask_b else 1)


@pytest.mark.parametrize('shape', [(2, 9, 7, 4), (1, 3, 5, 3)])
@pytest.mark.parametrize('masked', [False, True])
@pytest.mark.parametrize('mode', ['aa', 'again'])
def test_add_accumulates(shape, masked, mode):
    """a + a (the same tensor twice: two copies, the second accumulating, never the pair kernel) and (a + b) + a (a's gradient is
    written by the later Add before the first Add's backward accumulates: grad_written set; with masks that one is the pair
    kernel with acc_a = 1 when n % 4 == 0): gradient of a = 2 dY [* mask]."""
    tf, tb = _add_case(shape, False, masked, masked, mode=mode)
    n_axpy = 2 if mode == 'aa' else 4
    if not masked:
        assert tb.get('view_axpy') == n_axpy and 'masked_axpy' not in tb
    elif mode == 'aa':
        assert tb.get('masked_axpy') == 2
    else:       # later Add: a masked + (a + b) plain; first Add: pair (n % 4 == 0) or two scalar launches
        assert tb.get('masked_axpy') == (2 if shape[3] == 4 else 3) and tb.get('view_axpy') == 1


def test_add_masked_pair_second_iteration():
    """masked_axpy4_pair_kernel with n / 4 between 1.25 and 1.5 x the grid cap (plain grid-stride loop, second iteration)."""
    grid = K.large_grid(1)
    assert K.is_large(grid[0] * grid[1] * grid[2] * 4 // 4)
    tf, tb = _add_case(grid + (4,), True, True, True)
    assert tb.get('masked_axpy') == 1 and 'view_axpy' not in tb


# ------------------------------------------------------------------------------------------------------------------- Activation
def _act_run(kind, shape, residual, seed=5):
    x = K.act_inputs(shape, seed)
    g = _builder()
    t = g.input(shape[1], shape[2], shape[3], requires_grad=True)
    a = g.act(t, kind)
    out = g.add(a, t) if residual else a
    y, s, (dx,), tf, tb, gu = _run(g, out, [x], [t])
    assert tf.get('act_fwd') == 1 and tb.get('act_bwd') == 1
    assert np.isfinite(y).all() and np.isfinite(dx).all()
    return x, y, s, dx, gu


@pytest.mark.parametrize('kind', ['relu', 'leaky_relu'])
def test_act_piecewise_linear_bit_exact(kind):
    """relu = fmaxf(x, 0), leaky_relu = x > 0 ? x : 0.2f * x; backward dy * (x > 0 ? 1 : 0 | 0.2f): forward and gradient bitwise
    against numpy float32 on n = 9657 (n % 4 != 0) with the special values; at x == 0 the gradient is 0 (relu) / 0.2 (leaky), which
    is what oracle.torch_ops gives.  With prior accumulation (the input also feeds an Add: dx = dy + dy * f') on a power-of-two
    size, where dy * 0.2f is exact, so a fused multiply-add cannot change the bits."""
    slope = F32(0.2)
    df = lambda x: np.where(x > 0, F32(1), F32(0) if kind == 'relu' else slope).astype(F32)
    x, y, s, dx, gu = _act_run(kind, (3, 37, 29, 3), False)
    _eq(y, np.maximum(x, 0) if kind == 'relu' else np.where(x > 0, x, slope * x), 'forward')
    dy = gu * s
    _eq(dx, dy * df(x), 'gradient')
    _, odf = K.act_oracle(kind, x, np.ones_like(x), __import__('torch').float64)
    np.testing.assert_allclose(odf, df(x).astype(np.float64), rtol=0, atol=1e-8)
    assert (x == 0).any()
    x, y, s, dx, gu = _act_run(kind, (2, 16, 16, 16), True)
    assert y.size & (y.size - 1) == 0
    dy = gu * s
    _eq(dx, dy + dy * df(x), 'gradient with accumulation')


def _act_errors(kind, shape, residual):
    import torch
    x, y, s, dx, gu = _act_run(kind, shape, residual)
    dy = (gu * s).astype(np.float64)
    y64, dx64 = K.act_oracle(kind, x, dy, torch.float64, residual)
    y32, dx32 = K.act_oracle(kind, x, dy, torch.float32, residual)
    e = dict(fwd=K.act_error(y, y64, x), fwd_cpu=K.act_error(y32, y64, x),
             bwd=K.act_error(dx, dx64, x, float(gu)), bwd_cpu=K.act_error(dx32, dx64, x, float(gu)))
    print(f'activation {kind} n={x.size} residual={residual}: E_fwd {e["fwd"]:.3e} (cpu {e["fwd_cpu"]:.3e})  '
          f'E_bwd {e["bwd"]:.3e} (cpu {e["bwd_cpu"]:.3e})')
    return e


@pytest.mark.parametrize('residual', [False, True])
@pytest.mark.parametrize('kind', K.ACT_SMOOTH)
def test_act_smooth_kinds(kind, residual):
    """sigmoid / tanh / elu / selu / gelu through act_forward and act_backward against oracle.torch_ops at float64 (autograd for the
    gradient), n = 9657 (n % 4 != 0): a dense sample of [-20, 20] plus {0, +-1e-30, +-1e-6, +-0.5, +-3, +-30, +-88, +-104}; everything
    finite.  ``residual``: the input also feeds an Add behind the activation, so act_backward accumulates onto the Add's copy (the
    forward is then compared through the Add as well).  Metric E = max |got - ref| / max(1, |x|) (gradients in units of the
    upstream magnitude g); bound E <= max(4 E_cpu, 2^-22) with E_cpu the same oracle at float32 on the CPU, same inputs.
    Measured on an MI355X: ACT_MEASURED below; every kind sits within 1.4 x its E_cpu or under the floor."""
    e = _act_errors(kind, (3, 37, 29, 3), residual)
    assert e['fwd'] <= K.act_bound(e['fwd_cpu']), e
    assert e['bwd'] <= K.act_bound(e['bwd_cpu']), e


def test_act_gelu_second_iteration():
    """gelu on n = 2 112 519 > 8192 * 256 elements: act_fwd_kernel / act_bwd_kernel past the first grid-stride iteration."""
    shape = (1, 1031, 683, 3)
    assert int(np.prod(shape)) > K.EW_GRID_THREADS and int(np.prod(shape)) % 4 != 0
    e = _act_errors('gelu', shape, False)
    assert e['fwd'] <= K.act_bound(e['fwd_cpu']), e
    assert e['bwd'] <= K.act_bound(e['bwd_cpu']), e


# Measured on an MI355X with the cases above: kind -> (E forward, E_cpu forward, E backward, E_cpu backward), n = 9657, without / with
# the residual Add; the bound in force is max(4 E_cpu, 2^-22 = 2.38e-07).  A record, not a tolerance: nothing reads it.
ACT_MEASURED = {
    ('sigmoid', False): (6.136e-08, 6.827e-08, 3.393e-08, 3.813e-08), ('sigmoid', True): (1.301e-07, 1.301e-07, 9.600e-08, 9.641e-08),
    ('tanh', False): (6.363e-08, 2.974e-08, 1.048e-07, 8.558e-08), ('tanh', True): (1.260e-07, 1.219e-07, 1.387e-07, 1.486e-07),
    ('elu', False): (3.454e-08, 2.889e-08, 6.173e-08, 6.906e-08), ('elu', True): (1.046e-07, 1.046e-07, 1.223e-07, 1.212e-07),
    ('selu', False): (1.416e-07, 1.046e-07, 1.835e-07, 1.551e-07), ('selu', True): (2.556e-07, 2.120e-07, 2.538e-07, 2.254e-07),
    ('gelu', False): (9.317e-08, 2.643e-07, 1.153e-07, 2.106e-07), ('gelu', True): (1.983e-07, 2.856e-07, 1.744e-07, 2.416e-07),
    ('gelu', 'n=2112519'): (1.218e-07, 3.477e-07, 1.883e-07, 2.820e-07),
}


# ------------------------------------------------------------------------------------------------------------------- slice / pad
def _np_slice(x, oy, ox, step, ho, wo):
    return x[:, oy:oy + (ho - 1) * step + 1:step, ox:ox + (wo - 1) * step + 1:step, :]


@pytest.mark.parametrize('twice', [False, True])
@pytest.mark.parametrize('oy,ox,step', [(0, 0, 1), (1, 1, 2), (0, 1, 2), (2, 3, 1), (1, 0, 3)])
@pytest.mark.parametrize('shape,nmul', [((2, 9, 7, 3), 1), ((1, 12, 10, 8), 1), ((2, 6, 5, 2), 3)])
def test_slice2d(shape, nmul, oy, ox, step, twice):
    """slice_fwd_kernel / slice_bwd_kernel: y[n, i, j] = x[n, oy + i step, ox + j step] for crops (step 1) and strided
    sub-sampling, the largest valid window and a smaller one, one nmul = 3 input; the gradient is the scatter of dY with zeros
    elsewhere.  ``twice``: x + the same slice again through an Add, so the second SliceOp's backward accumulates (2 dY)."""
    n, h, w, c = shape
    ho, wo = (h - 1 - oy) // step + 1, (w - 1 - ox) // step + 1
    if oy == 0:
        ho, wo = ho - 1, max(wo - 2, 1)
    g = _builder()
    t = g.input(h, w, c, nmul=nmul, requires_grad=True)
    x = K.hashed_ints((n, nmul, h, w, c) if nmul > 1 else shape, 17 + oy)
    out = g.slice2d(t, oy, ox, step, ho, wo)
    if twice:
        out = g.add(out, g.slice2d(t, oy, ox, step, ho, wo))
    y, s, (dx,), _, _, gu = _run(g, out, [x], [t])
    xf = x.reshape(n * nmul, h, w, c)
    ref = _np_slice(xf, oy, ox, step, ho, wo)
    k = F32(2 if twice else 1)
    _eq(y.reshape(ref.shape), k * ref, 'forward')
    want = np.zeros_like(xf)
    _np_slice(want, oy, ox, step, ho, wo)[...] = k * gu * s.reshape(ref.shape)
    _eq(dx, want, 'gradient')


@pytest.mark.parametrize('twice', [False, True])
@pytest.mark.parametrize('to', [(8, 8), (5, 7)])
def test_pad_bottom_right(to, twice):
    """ZeroPadding2D at the bottom / right (slice_bwd_kernel as the forward scatter, slice_acc_kernel as the backward crop) from
    (5, 7) to (8, 8) and to (5, 7) (nothing to pad); ``twice``: two pads of the same input summed, the second crop accumulates."""
    n, h, w, c = 2, 5, 7, 3
    g = _builder()
    t = g.input(h, w, c, requires_grad=True)
    x = K.hashed_ints((n, h, w, c), 23)
    out = g.pad_bottom_right(t, *to)
    if twice:
        out = g.add(out, g.pad_bottom_right(t, *to))
    y, s, (dx,), _, _, gu = _run(g, out, [x], [t])
    k = F32(2 if twice else 1)
    ref = np.zeros((n,) + to + (c,), F32)
    ref[:, :h, :w] = k * x
    _eq(y, ref, 'forward')
    _eq(dx, k * gu * s[:, :h, :w], 'gradient')


def test_pad_concat(monkeypatch):
    """PadConcat of the U-Net decoder: pad_bottom_right of the smaller tensor, then concat with the larger one."""
    monkeypatch.setenv('DL4DS_NO_CONCAT_ALIAS', '1')
    g = _builder()
    ta, tb_ = g.input(5, 7, 3, requires_grad=True), g.input(6, 8, 5, requires_grad=True)
    a, b = K.hashed_ints((2, 5, 7, 3), 31), K.hashed_ints((2, 6, 8, 5), 32)
    out = g.concat([g.pad_bottom_right(ta, 6, 8), tb_])
    y, s, (da, db), tf, tb, gu = _run(g, out, [a, b], [ta, tb_])
    ref = np.zeros((2, 6, 8, 8), F32)
    ref[:, :5, :7, :3] = a
    ref[..., 3:] = b
    _eq(y, ref, 'forward')
    _eq(da, gu * s[:, :5, :7, :3], 'gradient of the padded input')
    _eq(db, gu * s[..., 3:], 'gradient of the full-size input')
    assert tf.get('concat_join') == 1 and tb.get('concat_split') == 1


# ------------------------------------------------------------------------------------------------------------------- repeat_time
def _seq_sum(d):
    """sum over axis 1 in the kernels' order: 0 + d[:, 0] + d[:, 1] + ... in float32."""
    acc = np.zeros_like(d[:, 0])
    for t in range(d.shape[1]):
        acc = acc + d[:, t]
    return acc


@pytest.mark.parametrize('hwc', [(3, 5, 3), (4, 4, 4), (1, 1, 2)])
@pytest.mark.parametrize('T', [1, 2, 8])
@pytest.mark.parametrize('B', [1, 3])
def test_repeat_time_plain(B, T, hwc):
    """repeat_time_fwd_kernel / repeat_time_bwd_kernel (the repeated tensor is the graph's output, nothing to alias): forward is T
    bit-exact copies, backward the sum over T in the kernel's stated order t = 0 .. T-1 starting from 0 (IEEE adds; with a
    power-of-two element count -- B = 1 and ps = 64 or 2 -- every partial sum is exact, so the order does not matter there);
    ps % 4 != 0 (45, 2) and ps % 4 == 0 (64)."""
    h, w, c = hwc
    g = _builder()
    t = g.input(h, w, c, requires_grad=True)
    x = K.hashed_ints((B, h, w, c), 41)
    out = g.repeat_time(t, T)
    y, s, (dx,), tf, tb, gu = _run(g, out, [x], [t])
    assert tf.get('repeat_time_fwd') == 1 and tb.get('repeat_time_bwd') == 1
    _eq(y.reshape((B, T, h, w, c)), np.repeat(x[:, None], T, axis=1), 'forward')
    _eq(dx, _seq_sum(gu * s.reshape((B, T, h, w, c))), 'gradient')


@pytest.mark.parametrize('chans', [(4, 4), (2, 6), (3, 5)])
@pytest.mark.parametrize('T', [1, 2, 8])
@pytest.mark.parametrize('B', [1, 3])
def test_repeat_time_into_concat(monkeypatch, B, T, chans):
    """concat([repeat_time(a), repeat_time(b)]) read by a convolution.  With concatenation aliasing (8 channels: whole 32-byte
    pixels) both repeats are written straight into the concatenation by repeat_time_fwd_view_kernel<V> (V = 4 / 2 / 1 for slices
    (4, 4) / (2, 6) / (3, 5)): no concat_join, no view_axpy.  For (4, 4) the gradients alias too, so repeat_time_bwd_view_kernel sums
    out of the concatenation's gradient (no concat_split); the other lists keep dense gradients and go through concat_split and
    the plain kernel.  With DL4DS_NO_CONCAT_ALIAS=1 the same graph takes the plain kernels and concat_join / concat_split.  The
    expected sums are formed, in the kernel's order, from the concatenation's gradient as the convolution wrote it."""
    h, w = 5, 3
    a, b = K.hashed_ints((B, h, w, chans[0]), 51), K.hashed_ints((B, h, w, chans[1]), 52)
    want_y = np.repeat(np.concatenate([a, b], axis=-1)[:, None], T, axis=1).reshape(B * T, h, w, 8)
    for alias in (True, False):
        if not alias:
            monkeypatch.setenv('DL4DS_NO_CONCAT_ALIAS', '1')
        g = _builder()
        ta, tb_ = g.input(h, w, chans[0], requires_grad=True), g.input(h, w, chans[1], requires_grad=True)
        cat = g.concat([g.repeat_time(ta, T), g.repeat_time(tb_, T)])
        out = g.conv2d(cat, 'id', 8, 1, use_bias=False)
        y, s, (da, db, dcat), tf, tb, gu = _run(g, out, [a, b], [ta, tb_, cat])
        _eq(_read(g, cat, B, 0), want_y, 'concatenation')
        _eq(y.reshape(want_y.shape), want_y, 'forward')
        assert tf.get('repeat_time_fwd') == 2 and tb.get('repeat_time_bwd') == 2
        if alias:
            assert 'concat_join' not in tf and 'view_axpy' not in tf
            assert ('concat_split' in tb) == (chans != (4, 4)) and 'view_axpy_masked' not in tb
        else:
            assert tf.get('concat_join') == 1 and tb.get('concat_split') == 1
        d = dcat.reshape(B, T, h, w, 8)
        assert np.abs(d).max() > 0
        _eq(da, _seq_sum(d[..., :chans[0]]), 'gradient of a')
        _eq(db, _seq_sum(d[..., chans[0]:]), 'gradient of b')


# ------------------------------------------------------------------------------------------------------------------- MaxPooling2D
def _pool_case(monkeypatch, c, grid, relu=False, twice=False, x=None):
    """maxpool2 of one input (``relu``: behind the ReLU identity convolution, so the pooled tensor is grad_masked; ``twice``: pooled
    by two ops whose results are concatenated, so the second backward to run accumulates onto the first's).  Forward and the
    gradient of the pooled tensor bitwise against tests/graph_ops_cases.maxpool2_ref / maxpool2_bwd_ref."""
    monkeypatch.setenv('DL4DS_NO_CONCAT_ALIAS', '1')
    n, h, w = grid
    if x is None:
        x = K.pool_input((n, h, w, c), relu)
    g = _builder()
    t = g.input(h, w, c, requires_grad=True)
    src = _relu_id(g, t, 'id') if relu else t
    xv = np.maximum(x, 0) if relu else x
    out = g.concat([g.maxpool2(src, 'p0'), g.maxpool2(src, 'p1')]) if twice else g.maxpool2(src)
    y, s, (dx,), tf, tb, gu = _run(g, out, [x], [src])
    ref = K.maxpool2_ref(xv)
    _eq(y, np.concatenate([ref, ref], axis=-1) if twice else ref, 'forward')
    dy = gu * s
    want = K.maxpool2_bwd_ref(xv, dy[..., :c])
    if twice:
        want = want + K.maxpool2_bwd_ref(xv, dy[..., c:])
    if relu:
        want = np.where(xv > 0, want, 0)
    _eq(dx, want, 'gradient of the pooled tensor')
    dropped = np.ones((h, w), bool)
    dropped[:h // 2 * 2, :w // 2 * 2] = False
    assert (dx[:, dropped] == 0).all()
    k = 2 if twice else 1
    assert tf.get('maxpool2_fwd') == k and tb.get('maxpool2_bwd') == k
    return tf, tb


@pytest.mark.parametrize('relu', [False, True])
@pytest.mark.parametrize('grid', K.POOL_GRIDS)
@pytest.mark.parametrize('c', K.POOL_QUAD_CHANS + K.POOL_SCALAR_CHANS)
def test_maxpool(monkeypatch, c, grid, relu):
    """maxpool2_fwd4_kernel / maxpool2_bwd4_kernel (C = 4, 8: pool_quad_ok) and maxpool2_fwd_kernel / maxpool2_bwd_kernel (C = 3, 6)
    on inputs from {-2 .. 2} where at least a quarter of the windows hold their maximum more than once: y is the window maximum,
    dx gets dY at the first maximum in the order (0,0), (0,1), (1,0), (1,1) and exact zeros elsewhere, the row / column dropped by
    VALID pooling on (7, 9) and (3, 2) included (MaxPoolOp::backward fills, then accumulates).  ``relu``: the pooled tensor is a
    ReLU output whose only consumer is the pooling (grad_masked): relu_mask = 1, expected where(x > 0, routed, 0); at least one
    window is all zero there, so its first entry is selected and then masked."""
    assert K.pool_quad(c) == (c in K.POOL_QUAD_CHANS)
    _pool_case(monkeypatch, c, grid, relu=relu)


@pytest.mark.parametrize('relu', [False, True])
@pytest.mark.parametrize('grid', K.POOL_GRIDS)
@pytest.mark.parametrize('c', K.POOL_QUAD_CHANS + K.POOL_SCALAR_CHANS)
def test_maxpool_same_tensor_twice(monkeypatch, c, grid, relu):
    """concat([maxpool2(x), maxpool2(x)]): the pooling whose backward runs second finds grad_written set and accumulates
    (accumulate = 1 in both kernels, with and without relu_mask); the sum of two g * s terms is exact: {-2g, 0, 2g}.  On the odd
    grids the first backward fills and accumulates, the second accumulates again: the dropped row and column stay 0."""
    tf, tb = _pool_case(monkeypatch, c, grid, relu=relu, twice=True)
    assert tf.get('concat_join') == 1 and tb.get('concat_split') == 1


def test_maxpool_quad_second_iteration(monkeypatch):
    """C = 4 with total / 4 output quads between 1.25 and 1.5 x the grid cap: maxpool2_fwd4_kernel / maxpool2_bwd4_kernel past the
    first grid-stride iteration, forward and backward bitwise."""
    n, ho, wo = K.large_grid(1)
    assert K.is_large(n * ho * wo * 4 // 4)
    grid = (n, 2 * ho, 2 * wo)
    _pool_case(monkeypatch, 4, grid, x=K.hashed_small_ints(grid + (4,), 7))
