"""Seeded cases of the multivariate ensemble verification, shared by tests/test_multivariate_api.py (CPU) and
tests/test_gpu_multivariate.py: the synthetic member stacks of the kernel tests and the two ensembles with identical per-cell
marginals (one smooth, one shuffled per cell) that show what the variogram score is for."""
import numpy as np

KS = (2, 3, 8, 33, 128)
SHAPES = ((5, 7, 1),                   # smaller than one tile, and than the largest lags
          (16, 16, 1),
          (9, 130, 1),                 # crosses tile edges on both axes (tiles are 32 x 8), ragged tail
          (2, 6, 5, 3))                # time and channels: pairs must not cross planes or channels
MAX_LAGS = (1, 3, 8)
ORDERS = (0.5, 1, 2)
LAG_WEIGHTS = ('inverse', 'uniform')
N_SAMPLES = 3                          # batch_size 2 leaves a ragged last batch


def smooth_fields(rng, count, shape, waves=6):
    """``count`` smooth random fields of ``shape`` = (..., H, W, C): a few low-frequency cosines per field -> float64"""
    H, W = shape[-3], shape[-2]
    yy, xx = np.meshgrid(np.arange(H) / max(H, 1), np.arange(W) / max(W, 1), indexing='ij')
    lead = int(np.prod(shape[:-3], dtype=np.int64)) * shape[-1]
    out = np.zeros((count, lead, H, W))
    for i in range(count):
        for j in range(lead):
            for _ in range(waves):
                u, v = rng.integers(0, 3, 2)
                out[i, j] += rng.standard_normal() * np.cos(2 * np.pi * (u * yy + v * xx) + rng.uniform(0, 2 * np.pi))
    out = out.reshape((count,) + tuple(shape[:-3]) + (shape[-1], H, W))
    return np.moveaxis(out, -3, -1)                                         # channel innermost


def data(seed, K, shape, n=N_SAMPLES):
    """-> members (K, n) + shape, observation (n,) + shape, float32: a smooth truth, members = truth + smooth error + noise"""
    rng = np.random.default_rng(seed)
    truth = smooth_fields(rng, n, shape)
    y = truth + 0.2 * rng.standard_normal(truth.shape)
    members = truth[None] + 0.5 * smooth_fields(rng, K * n, shape, waves=2).reshape((K, n) + tuple(shape)) \
        + 0.1 * rng.standard_normal((K, n) + tuple(shape))
    return members.astype(np.float32), y.astype(np.float32)


def kernel_cases(K, shape):
    """The (max_lag, order, fair, lag_weights) of one (K, shape): all three lags; orders, fair and the lag weighting rotate so that
    every value of each appears with every K and every shape"""
    ki, si = KS.index(K), SHAPES.index(tuple(shape))
    return [dict(max_lag=lag, order=ORDERS[(ki + si + li) % 3], fair=bool((ki + li) % 2), lag_weights=LAG_WEIGHTS[(si + li) % 2])
            for li, lag in enumerate(MAX_LAGS)]


def structure_case():
    """Two ensembles on (4, 32, 32, 1) with K = 8 and identical per-cell marginals against a smooth observation -> (y, smooth,
    shuffled): in ``shuffled`` each cell's 8 member values are permuted across the members, independently per cell."""
    rng = np.random.default_rng(2015)
    shape, K, n = (32, 32, 1), 8, 4
    truth = smooth_fields(rng, n, shape)
    y = (truth + 0.3 * smooth_fields(rng, n, shape, waves=3)).astype(np.float32)
    smooth = (truth[None] + 0.6 * smooth_fields(rng, K * n, shape, waves=3).reshape((K, n) + shape)).astype(np.float32)
    order = rng.random(smooth.shape).argsort(axis=0)
    shuffled = np.take_along_axis(smooth, order, axis=0)
    return y, smooth, shuffled
