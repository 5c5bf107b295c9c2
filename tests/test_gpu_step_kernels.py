"""Op-level tests of the small kernels every train step runs, through the C ABI (dl4ds_amd.ops), at the sizes where their loops,
tails and launch caps change behaviour: pixel loss (mae / mse), binary cross-entropy, Adam and the ReLU-mask + bias-gradient
reduction.  Inputs, float64 references, the restated launch figures and the derivation of every bound are in
tests/step_kernels_cases.py; tests/test_step_kernels_oracle.py checks them without a GPU.  Selections (masks, signs, exact zeros)
are compared bitwise, sums against a count of float32 roundings, and every reduction is run twice and must repeat its bits.
Each test prints its largest error over its bound.

Measured on an MI355X (largest error / bound over the cases; a record, nothing reads it): pixel-loss value 0.023, MSE gradient
0.54; BCE loss 0.54, gradient 0.25; Adam m' 0.48, v' 0.70, w' 0.54; db 0.12 (small shapes), 0.0016 (129 and 1024 slabs)."""
import numpy as np
import pytest

from tests import graph_ops_cases as K
from tests import step_kernels_cases as S
from tests.parity import kernel_tags

pytestmark = pytest.mark.gpu

F32, F64 = np.float32, np.float64


@pytest.fixture(scope='module')
def ops():
    import dl4ds_amd.ops as o
    return o


# ------------------------------------------------------------------------------------------------------------------- pixel loss
@pytest.mark.parametrize('kind', ['mae', 'mse'])
@pytest.mark.parametrize('shape', S.LOSS_SHAPES)
def test_pixel_loss(ops, shape, kind):
    """pixel_loss_kernel + pixel_loss_finish_kernel at n = 1, 2047, 2049 (one block, two blocks), 64 * 2048 + 1 (65 partials: the
    finish kernel's lane-strided loop runs twice), 1024 * 2048 + 3 * 2048 + 5 (the block cap: a second grid-stride pass) and one
    multi-channel shape, with p == t on a fifth of the entries.
    Value: |got - ref| <= 2^-18 sum|terms| / n against the float64 sum of the float32 terms -- the longest chain is 45 roundings
    (step_kernels_cases.loss_chain: 9 thread-loop additions, 6 wave, 4 block, 16 + 6 finish, 4 for a contracted d * d, inv_n and the
    two closing multiplications), 64 is the next power of two.  MAE gradient: bitwise g * sign(p - t) with one magnitude g within
    1 ulp of 1 / n, 0 exactly where p == t.  MSE gradient: within 2^-22 of 2 (p - t) / n (three roundings).  The same loss bits
    without a gradient buffer (dp == nullptr) and on a second call."""
    t, p = S.loss_inputs(shape, 7)
    n = t.size
    lv, g = ops.loss(kind, t, p)
    ref, mag = S.loss_ref(kind, t, p)
    err = abs(lv - ref) / (S.LOSS_VALUE_BOUND * mag)
    d = p.astype(F64) - t.astype(F64)
    if kind == 'mae':
        nz = np.abs(g[g != 0])
        gu, ideal = F32(nz.min()), F32(1) / F32(n)
        assert nz.max() == gu, 'more than one non-zero magnitude'
        assert abs(F64(gu) - F64(ideal)) <= np.spacing(ideal), (gu, ideal)
        np.testing.assert_array_equal(g, (gu * np.sign(d)).astype(F32))
        gerr = 0.0
    else:
        gref = S.mse_grad_ref(t, p)
        assert (g[p == t] == 0).all()
        with np.errstate(divide='ignore', invalid='ignore'):
            gerr = float(np.where(gref != 0, np.abs(g.astype(F64) - gref) / np.abs(gref), 0.0).max() / S.LOSS_MSE_GRAD_BOUND)
    print(f'pixel loss {kind} n={n}: value error / bound {err:.3e} (chain {S.loss_chain(n)}), gradient error / bound {gerr:.3e}')
    assert (p == t).any() or n == 1
    assert err <= 1.0, (lv, ref)
    assert gerr <= 1.0
    lv2, none = ops.loss(kind, t, p, want_grad=False)
    assert none is None and F32(lv2).tobytes() == F32(lv).tobytes()
    lv3, g3 = ops.loss(kind, t, p)
    assert F32(lv3).tobytes() == F32(lv).tobytes() and np.array_equal(g3, g)


# ------------------------------------------------------------------------------------------------------------------- BCE
@pytest.mark.parametrize('label', S.BCE_LABELS)
@pytest.mark.parametrize('n', S.BCE_SIZES)
def test_bce_clip_and_stride_loop(ops, n, label):
    """bce_kernel (one block of 256) for n = 1 .. 1000 (n > 256: its stride loop) and labels 0, 1, 0.9 on probabilities that include
    0, 1, 1e-9 (clipped: gradient exactly 0), eps = float32(1e-7) and float32(1) - eps (inclusive: gradient not 0) and 0.5.
    Reference in float64 with the float32 eps and 1 - eps.  Bound: the activations' rule, max(4 E_cpu, 2^-22), E_cpu being the same
    expression in float32 on the CPU, errors relative to the mean term magnitude (loss) and to l / pc + (1 - l) / (1 - pc) over n
    (each gradient entry)."""
    p = S.bce_inputs(n)
    lv, g = ops.bce(p, label)
    assert np.isfinite(lv) and np.isfinite(g).all()
    zero = S.bce_zero_gradient(p)
    assert (g[zero] == 0).all() and (g[~zero] != 0).all()
    e_loss, e_grad = S.bce_errors(lv, g, p, label)
    c_loss, c_grad = S.bce_errors(*S.bce32(p, label), p, label)
    b_loss, b_grad = K.act_bound(c_loss), K.act_bound(c_grad)
    print(f'bce n={n} label={label}: loss error / bound {e_loss / b_loss:.3e} (E {e_loss:.3e}, cpu {c_loss:.3e}), '
          f'gradient error / bound {e_grad / b_grad:.3e} (E {e_grad:.3e}, cpu {c_grad:.3e})')
    assert e_loss <= b_loss and e_grad <= b_grad
    lv2, g2 = ops.bce(p, label)
    assert F32(lv2).tobytes() == F32(lv).tobytes() and np.array_equal(g2, g)


# ------------------------------------------------------------------------------------------------------------------- Adam
@pytest.mark.parametrize('n', S.ADAM_SIZES)
def test_adam_tails_and_block_cap(ops, n):
    """adam_kernel for n = 1, 2, 3 (scalar tail only), 4, 5, 1023, 1025 and 2051 (a tail behind one to three blocks of float4 work)
    and 4 * 256 * 2048 + 4 * 256 * 600 + 3 (the 2048-block cap: 600 blocks take a second grid-stride pass, then a tail of 3), for
    t = 1, 7, 10000 and grad_scale = 1, 0.5, 1 / 3 (all nine pairs; three at the largest size), with g = 1e-30, g = 1e15 and idle
    entries (g = m = v = 0: m', v' stay 0 and w' == w bitwise, sqrt(0) + eps in the denominator).
    m' within 2^-22 (|b1 m| + |(1 - b1) g|) and v' within 2^-22 (|b2 v| + |(1 - b2) g^2|) of float64 (g scaled; wide enough that a
    fused multiply-add does not matter); w' within 2^-22 (|w| + |step|) of w - lr_t m' / (sqrt(v') + eps) evaluated in float64 from
    the returned m', v'."""
    w, g, m, v, idle = S.adam_inputs(n)
    pairs = [(t, gs) for t in S.ADAM_STEPS for gs in S.ADAM_SCALES]
    if n == S.ADAM_LARGEST:
        pairs = list(zip(S.ADAM_STEPS, S.ADAM_SCALES))
    worst = (0.0, 0.0, 0.0)
    for t, gs in pairs:
        w1, m1, v1 = ops.adam(w, g, m, v, t, S.ADAM_LR, S.ADAM_B1, S.ADAM_B2, S.ADAM_EPS, gs)
        assert np.isfinite(w1).all() and np.isfinite(m1).all() and np.isfinite(v1).all()
        assert np.array_equal(w1[idle], w[idle]) and (m1[idle] == 0).all() and (v1[idle] == 0).all()
        e = S.adam_errors(w1, m1, v1, w, g, m, v, t, gs)
        worst = tuple(max(a, b) for a, b in zip(worst, e))
        assert max(e) <= 1.0, (t, gs, e)
    print(f'adam n={n}: error / bound m {worst[0]:.3e}, v {worst[1]:.3e}, w {worst[2]:.3e}')


# ------------------------------------------------------------------------------------------------------------------- bias_act_bwd
def _bias_case(ops, c, npix):
    dy, y = S.bias_inputs((1, 1, npix, c), 5)
    want_dz, ref_db, mag = S.bias_ref(dy, y)
    (dz, db), tags = kernel_tags(lambda: ops.bias_act_bwd(dy, y))
    assert tags.get('bias_act_bwd') == 1 and 'relu_mask_flat' not in tags
    np.testing.assert_array_equal(dz, want_dz)
    bound = S.bias_db_bound(c, npix, mag)
    err = np.abs(db.astype(F64) - ref_db)
    assert (err[bound == 0] == 0).all()
    ratio = float((err[bound > 0] / bound[bound > 0]).max()) if (bound > 0).any() else 0.0
    dz2, db2 = ops.bias_act_bwd(dy, y)
    assert np.array_equal(dz2, dz) and db2.tobytes() == db.tobytes()
    assert ratio <= 1.0, (c, npix, ratio)
    return ratio


@pytest.mark.parametrize('c', S.BIAS_CHANS)
def test_bias_act_bwd_small(ops, c):
    """bias_act_bwd_kernel<TX> + reduce_slabs_kernel2 for C = 1 .. 130 (TX = 8, 16, 32, 64; one to three channel blocks, the last
    one ragged) at 1, TY - 1 and TY + 1 pixels (TY + 1: row 0 runs its pixel loop twice), y holding +0.0, -0.0 and negatives:
    dz bitwise where(y > 0, dy, 0); db within next_pow2(iters + TY + blocks) roundings of the float64 sum, relative to the
    channel's sum |dz| (step_kernels_cases.bias_geometry)."""
    worst = max(_bias_case(ops, c, npix) for npix in S.bias_pixel_counts(c))
    print(f'bias_act_bwd C={c} pixels={S.bias_pixel_counts(c)}: db error / bound {worst:.3e}')


@pytest.mark.parametrize('c,npix', S.BIAS_LARGE)
def test_bias_act_bwd_many_slabs(ops, c, npix):
    """1024 x TY + 1 pixels per TX (129 slabs, eight to nine pixels per thread) and, for TX = 8 and 64, 1024 x TY x 8 + 1 pixels: the
    block cap holds, the pixel loop strides by the capped grid into a ninth pass, and reduce_slabs_kernel2 adds 1024 slabs."""
    geo = S.bias_geometry(c, npix)
    ratio = _bias_case(ops, c, npix)
    print(f'bias_act_bwd C={c} pixels={npix}: slabs {geo["nb"]}, chain {geo["chain"]}, db error / bound {ratio:.3e}')


@pytest.mark.parametrize('shape', [(2, 9, 7, 4), (1, 3, 5, 8), (1, 1, 1, 4), (1, 3, 5, 3), (1, 1, 1, 1), (2, 9, 7, 13), (1, 1, 33, 130)])
def test_bias_act_bwd_mask_only(ops, shape):
    """want_db = False: relu_mask_flat4_kernel when the element count is a multiple of 4 (tag relu_mask_flat), else
    bias_act_bwd_kernel without a partial buffer; dz bitwise either way."""
    dy, y = S.bias_inputs(shape, 9)
    (dz, db), tags = kernel_tags(lambda: ops.bias_act_bwd(dy, y, want_db=False))
    assert db is None
    if dy.size % 4 == 0:
        assert tags.get('relu_mask_flat') == 1 and 'bias_act_bwd' not in tags
    else:
        assert tags.get('bias_act_bwd') == 1 and 'relu_mask_flat' not in tags
    np.testing.assert_array_equal(dz, S.bias_ref(dy, y)[0])


def test_relu_mask_flat_second_iteration(ops):
    """relu_mask_flat4_kernel with total / 4 between 1.25 and 1.5 x the element-wise grid cap: a second grid-stride iteration."""
    shape = S.flat4_large_shape()
    assert K.is_large(int(np.prod(shape)) // 4)
    dy, y = S.bias_inputs(shape, 13)
    (dz, _), tags = kernel_tags(lambda: ops.bias_act_bwd(dy, y, want_db=False))
    assert tags.get('relu_mask_flat') == 1 and 'bias_act_bwd' not in tags
    np.testing.assert_array_equal(dz, S.bias_ref(dy, y)[0])
