"""CPU-only checks behind tests/test_gpu_graph_ops.py: the float32 oracle that sets the activation bound is itself close to the
float64 one, the grid cap the size rule is built on is the one in the source, and the input generators do what the GPU tests
rely on."""
import numpy as np
import pytest

from tests import graph_ops_cases as K


@pytest.mark.parametrize('residual', [False, True])
@pytest.mark.parametrize('kind', K.ACT_SMOOTH)
def test_float32_oracle_is_close_to_float64(kind, residual):
    """E_cpu <= 2^-20 per kind and direction, on the inputs of the GPU test: a broken oracle cannot loosen max(4 E_cpu, 2^-22)
    unnoticed."""
    import torch
    x = K.act_inputs((3, 37, 29, 3), 5)
    gu = np.float32(1) / np.float32(x.size)
    dy = (gu * K.signs(x.shape, 11)).astype(np.float64)
    y64, dx64 = K.act_oracle(kind, x, dy, torch.float64, residual)
    y32, dx32 = K.act_oracle(kind, x, dy, torch.float32, residual)
    assert np.isfinite(y64).all() and np.isfinite(dx64).all()
    assert K.act_error(y32, y64, x) <= K.ACT_CPU_CAP
    assert K.act_error(dx32, dx64, x, float(gu)) <= K.ACT_CPU_CAP


def test_oracle_kink_conventions():
    """At x == 0 the oracle's gradient is 0 for relu and 0.2 for leaky_relu (what act_df computes with its x > 0 branch)."""
    import torch
    x = np.array([0.0, -1.0, 1.0], np.float32)
    for kind, at0 in (('relu', 0.0), ('leaky_relu', 0.2)):
        _, df = K.act_oracle(kind, x, np.ones(3), torch.float64)
        np.testing.assert_allclose(df, [at0, at0, 1.0], rtol=0, atol=1e-12)


def test_grid_cap_matches_the_source():
    assert K.ew_grid_threads_in_source() == K.EW_GRID_THREADS == 2097152


@pytest.mark.parametrize('cvn', [1, 2, 3, 4, 5, 8, 13])
def test_large_grid_satisfies_the_rule(cvn):
    n, h, w = K.large_grid(cvn)
    assert n == 1 and K.is_large(n * h * w * cvn)


def test_input_generators():
    x = K.hashed_ints((2, 9, 7, 13), 3)
    assert x.dtype == np.float32 and (x == np.round(x)).all() and (x != 0).all() and np.abs(x).max() <= 64
    flat = x.ravel()
    assert (flat[1:] != flat[:-1]).mean() > 0.98 and (x[..., 1:, :] != x[..., :-1, :]).mean() > 0.98
    z = K.hashed_ints((2, 9, 7, 13), 3, zeros=True)
    assert 0.1 < (z == 0).mean() < 0.3 and (z[z != 0] == x[z != 0]).all()
    s = K.signs((4, 5, 6), 11)
    assert set(np.unique(s)) == {-1.0, 1.0} and abs(s.mean()) < 0.3
    assert not np.array_equal(K.hashed_ints((64,), 1), K.hashed_ints((64,), 2))
    a = K.act_inputs((3, 37, 29, 3), 5)
    assert a.size % 4 != 0 and np.array_equal(a.ravel()[:K.ACT_SPECIALS.size], K.ACT_SPECIALS) and np.abs(a).max() == 104


def test_dispatch_restatements():
    assert K.concat_onepass_vec((16, 8, 2)) == (2, 13) and K.concat_onepass_vec((5, 3, 1, 4)) == (1, 13)
    assert K.concat_onepass_vec((4, 4)) == (2, 4) and K.concat_onepass_vec((1, 1)) == (1, 2)
    assert K.view_axpy_variant(4, 4, 0, 4, 0, 126) == ('flat4', 4) and K.view_axpy_variant(3, 3, 0, 3, 0, 15) == ('small1', 1)
    assert K.view_axpy_variant(16, 16, 0, 32, 0, 6) == ('strided4', 4) and K.view_axpy_variant(4, 4, 0, 16, 10, 6) == ('small2', 2)
    assert K.view_axpy_variant(8, 8, 0, 18, 9, 6) == ('small1', 1)
    assert K.view_axpy_masked_variant(16, 32, 0) == 'masked4' and K.view_axpy_masked_variant(6, 16, 2) == 'generic'


# ------------------------------------------------------------------------------------------------------------------- max-pool
def test_small_int_generator():
    x = K.hashed_small_ints((2, 9, 7, 13), 3)
    assert x.dtype == np.float32 and set(np.unique(x)) == {-2.0, -1.0, 1.0, 2.0}
    z = K.hashed_small_ints((2, 9, 7, 13), 3, zeros=True)
    assert 0.1 < (z == 0).mean() < 0.3 and (z[z != 0] == x[z != 0]).all()
    assert not np.array_equal(K.hashed_small_ints((64,), 1), K.hashed_small_ints((64,), 2))


def test_maxpool_reference_on_hand_made_windows():
    """One channel, 5 x 4 (the last row is dropped): windows with the maximum at each position alone, twice, and four times."""
    x = np.array([[1, 2, 2, 2],
                  [2, 0, 2, 2],
                  [-1, -1, 0, -2],
                  [-1, -2, -1, 0],
                  [9, 9, 9, 9]], np.float32).reshape(1, 5, 4, 1)
    dy = np.array([[10, 20], [30, 40]], np.float32).reshape(1, 2, 2, 1)
    np.testing.assert_array_equal(K.maxpool2_ref(x)[0, :, :, 0], [[2, 2], [-1, 0]])
    np.testing.assert_array_equal(K.maxpool2_bwd_ref(x, dy)[0, :, :, 0], [[0, 10, 20, 0],     # (0,1) before (1,0); (0,0) of four
                                                                          [0, 0, 0, 0],
                                                                          [30, 0, 40, 0],      # (0,0) of three; (0,0) before (1,1)
                                                                          [0, 0, 0, 0],
                                                                          [0, 0, 0, 0]])
    assert K.pool_tie_share(x) == 1.0 and K.pool_has_dead_window(x) and not K.pool_has_dead_window(np.abs(x) + 1)
    lone = np.array([[1, 2], [4, 3]], np.float32).reshape(1, 2, 2, 1)
    np.testing.assert_array_equal(K.maxpool2_bwd_ref(lone, np.full((1, 1, 1, 1), 5, np.float32))[0, :, :, 0], [[0, 0], [5, 0]])
    assert K.pool_tie_share(lone) == 0.0


def test_maxpool_reference_against_autograd_without_ties():
    """Where no window has a tie the routing is unambiguous: the same as oracle.torch_ops.max_pool2 under autograd, odd sizes too."""
    import torch
    from oracle import torch_ops as T
    x = np.random.default_rng(3).permutation(2 * 7 * 9 * 3).astype(np.float32).reshape(2, 7, 9, 3)
    dy = K.hashed_ints((2, 3, 4, 3), 5)
    xt = torch.tensor(x, dtype=torch.float64, requires_grad=True)
    yt = T.max_pool2(xt)
    (yt * torch.tensor(dy, dtype=torch.float64)).sum().backward()
    np.testing.assert_array_equal(K.maxpool2_ref(x), yt.detach().numpy())
    np.testing.assert_array_equal(K.maxpool2_bwd_ref(x, dy), xt.grad.numpy())


@pytest.mark.parametrize('relu', [False, True])
@pytest.mark.parametrize('grid', K.POOL_GRIDS)
@pytest.mark.parametrize('c', K.POOL_QUAD_CHANS + K.POOL_SCALAR_CHANS)
def test_maxpool_inputs_have_ties_and_dead_windows(c, grid, relu):
    x = K.pool_input(grid + (c,), relu)
    assert set(np.unique(x)) <= {-2.0, -1.0, 0.0, 1.0, 2.0}
    assert K.pool_tie_share(np.maximum(x, 0) if relu else x) >= 0.25
    if relu:
        assert (x == 0).any() and K.pool_has_dead_window(x)
        dead = K.pool_windows(x).max(axis=0) <= 0                  # such a window is all zero behind the ReLU: routed to (0,0), masked
        routed = K.maxpool2_bwd_ref(np.maximum(x, 0), np.ones_like(K.maxpool2_ref(x)))
        assert (K.pool_windows(routed)[0][dead] == 1).all() and (K.pool_windows(np.where(x > 0, routed, 0))[:, dead] == 0).all()


def test_maxpool_large_input_has_ties():
    n, ho, wo = K.large_grid(1)
    assert K.pool_tie_share(K.hashed_small_ints((n, 2 * ho, 2 * wo, 4), 7)) >= 0.25


def test_pool_quad_rule_matches_the_source():
    """pool_quad_ok is vec && d2s <= 1 && C % 4 == 0 && no channel affine, and make_view sets vec = (C % 4 == 0 and 16-byte aligned)
    with d2s = 0 and sc = nullptr: for dense aligned tensors the rule is C % 4 == 0, which is what pool_quad restates."""
    terms, vec = K.pool_quad_ok_in_source()
    assert terms == sorted(['v.vec', 'v.d2s <= 1', '(v.C & 3) == 0', '!v.sc'])
    assert vec == '((C&3)==0)&&((((uintptr_t)p)&15)==0)'
    assert [K.pool_quad(c) for c in (3, 4, 6, 8)] == [False, True, False, True]
    assert all(K.pool_quad(c) for c in K.POOL_QUAD_CHANS) and not any(K.pool_quad(c) for c in K.POOL_SCALAR_CHANS)
    assert K.POOL_ODD_GRIDS == ((1, 7, 9), (1, 3, 2))
