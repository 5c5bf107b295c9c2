"""CPU-only checks behind tests/test_gpu_step_kernels.py: the restated launch figures are the ones in the source, the chain counts
follow from them, the inputs hold the edge values the GPU tests are there for, and each kernel's expression evaluated in float32 on
the CPU stays inside the bound its GPU test uses."""
import numpy as np
import pytest

from tests import graph_ops_cases as K
from tests import step_kernels_cases as S

F32, F64 = np.float32, np.float64


# ------------------------------------------------------------------------------------------------------------------- figures
def test_launch_figures_match_the_source():
    assert S.loss_figures_in_source() == (S.LOSS_BLOCK_ELEMS, S.LOSS_BLOCK_CAP, S.LOSS_FINISH_LANES, S.WAVE) == (2048, 1024, 64, 64)
    assert S.bce_launch_in_source() == (1, S.THREADS)
    assert S.adam_figures_in_source() == (S.THREADS, S.ADAM_BLOCK_CAP) == (256, 2048)
    assert S.pick_tx_in_source() == (8, 8, 16, 16, 32, 32, 64)
    assert [S.pick_tx(c) for c in (1, 8, 9, 16, 17, 32, 33, 130)] == [8, 8, 16, 16, 32, 32, 64, 64]
    assert S.bias_blocks_in_source() == (S.BIAS_ROWS_PER_BLOCK, S.BIAS_BLOCK_CAP) == (8, 1024)
    assert K.ew_grid_threads_in_source() == K.EW_GRID_THREADS


def test_helpers():
    assert [S.next_pow2(k) for k in (1, 2, 3, 45, 64, 65, 1065)] == [1, 2, 4, 64, 64, 128, 2048]
    v = np.arange(128, dtype=F32).reshape(2, 64)
    np.testing.assert_array_equal(S._wave_sum(v), v.sum(axis=1))
    np.testing.assert_array_equal(S._serial_sum(v, 1), v.sum(axis=1))
    np.testing.assert_array_equal(S._block_sums(np.ones(1000, F32), 2), [512, 488])


# ------------------------------------------------------------------------------------------------------------------- pixel loss
def test_loss_sizes_reach_the_loops():
    n = [int(np.prod(s)) for s in S.LOSS_SHAPES]
    assert n == [1, 2047, 2049, 131073, 2103301, 378] and max(n) == S.LOSS_LARGEST
    assert [S.loss_blocks(k) for k in n] == [1, 1, 2, 65, 1024, 1]
    assert S.loss_blocks(131073) > S.LOSS_FINISH_LANES                               # the finish kernel's lane loop runs twice
    assert S.LOSS_LARGEST > S.LOSS_BLOCK_CAP * S.LOSS_BLOCK_ELEMS                   # pixel_loss_kernel's loop past one block's 2048
    assert S.cdiv(S.LOSS_LARGEST, 1024 * 256) == 9
    assert max(S.loss_chain(k) for k in n) == S.loss_chain(S.LOSS_LARGEST) == S.LOSS_CHAIN_LARGEST == 45
    assert S.LOSS_VALUE_BOUND == 2.0 ** -18


@pytest.mark.parametrize('shape', S.LOSS_SHAPES)
def test_loss_inputs_and_float32_evaluation(shape):
    t, p = S.loss_inputs(shape, 7)
    n = t.size
    eq = (p == t).mean()
    assert (n < 4 and eq == 0) or 0.15 < eq < 0.25
    for kind in ('mae', 'mse'):
        ref, mag = S.loss_ref(kind, t, p)
        assert ref > 0 and abs(S.loss_value32(kind, t, p) - ref) <= S.LOSS_VALUE_BOUND * mag
    d = (p - t).astype(F32)
    g32 = (F32(1) / F32(n)) * F32(2) * d
    ref = S.mse_grad_ref(t, p)
    assert (np.abs(g32.astype(F64) - ref) <= S.LOSS_MSE_GRAD_BOUND * np.abs(ref)).all() and (ref[p == t] == 0).all()


# ------------------------------------------------------------------------------------------------------------------- BCE
def test_bce_constants_and_inputs():
    assert S.BCE_ONE_M == F32(1) - F32(1e-7) and S.BCE_ONE_M < 1 and S.BCE_EPS > 0
    p = S.bce_inputs(1000)
    assert p.dtype == F32 and np.array_equal(p[:6], S.BCE_SPECIALS) and (p[6:] > 0).all() and (p[6:] < 1).all()
    z = S.bce_zero_gradient(p)
    assert list(z[:6]) == [True, True, True, False, False, False]                   # 0, 1, 1e-9 clipped; eps and 1 - eps inclusive
    assert np.array_equal(S.bce_inputs(16), p[:16]) and S.bce_inputs(1).tolist() == [0.0]
    assert max(S.BCE_SIZES) > S.THREADS                                              # bce_kernel's stride loop runs


def test_bce_reference():
    """Against oracle.torch_ops.bce at float64 away from the clip, and the clip's zero gradient by hand."""
    import torch
    from oracle import torch_ops as T
    p = S.bce_inputs(300)[6:]
    for label in S.BCE_LABELS:
        t = torch.tensor(p.astype(F64).reshape(-1, 1), requires_grad=True)
        lv = T.bce(torch.full_like(t, float(F32(label))), t)
        lv.backward()
        ref, mag, g, gmag = S.bce_ref(p, label)
        assert ref == pytest.approx(float(lv.detach()), rel=1e-6) and mag == pytest.approx(ref, rel=1e-12)
        np.testing.assert_allclose(g, t.grad.numpy().ravel(), rtol=1e-6, atol=0)
        assert (gmag >= np.abs(g)).all()
    _, _, g, _ = S.bce_ref(S.BCE_SPECIALS, 1.0)
    assert list(g[:3]) == [0, 0, 0] and g[3] == pytest.approx(-1e7 / 6, rel=1e-6) and (g[3:] != 0).all()


@pytest.mark.parametrize('label', S.BCE_LABELS)
@pytest.mark.parametrize('n', S.BCE_SIZES)
def test_bce_float32_evaluation(n, label):
    """The float32 evaluation is finite, has exact zeros where the reference has, and its error -- which sets the GPU bound
    max(4 E_cpu, 2^-22) -- is what the expression allows: below 2^-20 except where 1 - pc is formed for pc = eps, whose float32
    rounding (1 - 1.19e-7) is a quarter of the term log(1 - pc) itself."""
    p = S.bce_inputs(n)
    lv, g = S.bce32(p, label)
    assert np.isfinite(lv) and np.isfinite(g).all() and (g[S.bce_zero_gradient(p)] == 0).all()
    e_loss, e_grad = S.bce_errors(lv, g, p, label)
    assert e_grad <= 2.0 ** -20
    assert e_loss <= (0.25 if n == 1 and label != 1.0 else 2.0 ** -20)


# ------------------------------------------------------------------------------------------------------------------- Adam
def test_adam_sizes_reach_the_paths():
    assert S.ADAM_LARGEST == 2711555 and S.ADAM_LARGEST % 4 == 3
    assert [S.adam_blocks(n) for n in S.ADAM_SIZES] == [1, 1, 1, 1, 1, 1, 2, 3, 2048]
    n4 = S.ADAM_LARGEST // 4
    assert S.ADAM_BLOCK_CAP * S.THREADS < n4 < 2 * S.ADAM_BLOCK_CAP * S.THREADS      # a second pass on 600 of the 2048 blocks
    assert n4 - S.ADAM_BLOCK_CAP * S.THREADS == 600 * S.THREADS
    assert [n % 4 for n in S.ADAM_SIZES[:8]] == [1, 2, 3, 0, 1, 3, 1, 3]              # n < 4: tail only; 1025, 2051: tail on a 2- / 3-block grid


@pytest.mark.parametrize('n', S.ADAM_SIZES)
def test_adam_inputs_and_float32_evaluation(n):
    w, g, m, v, idle = S.adam_inputs(n)
    if n >= 1023:
        assert idle.any() and (g == F32(1e-30)).any() and (g == F32(1e15)).any() and idle[-1]
    assert (v[~idle] > 0).all() and (g[idle] == 0).all() and (m[idle] == 0).all() and (v[idle] == 0).all()
    for t in S.ADAM_STEPS:
        for gs in S.ADAM_SCALES:
            w1, m1, v1 = S.adam32(w, g, m, v, t, gs)
            assert np.isfinite(w1).all() and np.isfinite(m1).all() and np.isfinite(v1).all()
            assert np.array_equal(w1[idle], w[idle]) and (m1[idle] == 0).all() and (v1[idle] == 0).all()
            assert max(S.adam_errors(w1, m1, v1, w, g, m, v, t, gs)) <= 1.0


def test_adam_reference_matches_the_oracle():
    """oracle.np_ops.adam_step has the constants in double (0.999 against float32(0.999): 1.3e-5 of 1 - b2), so: within 2e-5 of the
    magnitudes that each bound is made of."""
    from oracle import np_ops as N
    w, g, m, v, _ = S.adam_inputs(1023)
    keep = np.abs(g) < 10
    for t in (1, 7):
        rw, rm, rv = N.adam_step(w.astype(F64), 0.5 * g.astype(F64), m.astype(F64), v.astype(F64), t, 1e-3)
        am, bm, av, bv = S.adam_moments_ref(g, m, v, 0.5)
        aw, bw = S.adam_w_ref(w, am, av, t)
        for got, ref, bound in ((am, rm, bm), (av, rv, bv), (aw, rw, bw)):
            assert (np.abs(got - ref)[keep] <= 2e-5 * bound[keep] / S.ADAM_BOUND).all()


# ------------------------------------------------------------------------------------------------------------------- bias_act_bwd
def test_bias_geometry():
    assert sorted({S.pick_tx(c) for c in S.BIAS_CHANS}) == [8, 16, 32, 64]
    assert sorted({S.bias_geometry(c, 1)['cblocks'] for c in S.BIAS_CHANS}) == [1, 2, 3]
    for c in S.BIAS_CHANS:
        ty = S.THREADS // S.pick_tx(c)
        assert S.bias_pixel_counts(c) == (1, ty - 1, ty + 1)
        assert [S.bias_geometry(c, n)['iters'] for n in S.bias_pixel_counts(c)] == [1, 1, 2]       # TY + 1: row 0 takes two pixels
    for c, npix in S.BIAS_LARGE:
        geo = S.bias_geometry(c, npix)
        if npix == S.BIAS_BLOCK_CAP * geo['ty'] + 1:
            assert geo['nb'] == 129 and geo['iters'] == 8
        else:                                              # the cap holds: more pixels than 1024 blocks x TY rows x 8
            assert npix == S.BIAS_BLOCK_CAP * geo['ty'] * S.BIAS_ROWS_PER_BLOCK + 1
            assert geo['nb'] == S.BIAS_BLOCK_CAP and geo['iters'] == 9 and geo['chain'] == 9 + geo['ty'] + 1024
    assert {S.pick_tx(c) for c, _ in S.BIAS_LARGE} == {8, 16, 32, 64}
    shape = S.flat4_large_shape()
    assert shape[3] == 4 and K.is_large(int(np.prod(shape)) // 4)


@pytest.mark.parametrize('c,npix', [(c, n) for c in S.BIAS_CHANS for n in S.bias_pixel_counts(c)] + S.BIAS_LARGE)
def test_bias_inputs_and_float32_evaluation(c, npix):
    dy, y = S.bias_inputs((1, 1, npix, c), 5)
    if npix * c >= 100:
        assert (y < 0).any() and (y > 0).any()
        zero = y == 0
        assert np.signbit(y[zero]).any() and not np.signbit(y[zero]).all()
    dz, db, mag = S.bias_ref(dy, y)
    assert (dz[y <= 0] == 0).all() and np.array_equal(dz[y > 0], dy[y > 0]) and not (dz[np.signbit(y)] != 0).any()
    assert (np.abs(S.bias_db32(dz).astype(F64) - db) <= S.bias_db_bound(c, npix, mag)).all()
