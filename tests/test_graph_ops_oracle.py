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
