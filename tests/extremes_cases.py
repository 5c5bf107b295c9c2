"""Seeded cases of the extreme-value tests, shared by tests/test_extremes_api.py (CPU) and tests/test_gpu_extremes.py."""
import numpy as np

LDS_MAX = 512                  # longest segment the sorter sorts in LDS (csrc/sort_keys.h: SORT_STRIDED_MAX)
LM_LENGTHS = (1, 2, 3, 4, 5, 37, LDS_MAX, LDS_MAX + 1, 700)
LM_CELLS = (1, 63, 65, 300)
POT_LENGTHS = (1, 2, 7, 64, 365)
POT_CELLS = (1, 65, 300)
POT_RUNS = (1, 2, 32)
SENTINEL = np.float32(-7.0e37)  # fills the rows a strided read must skip: finite, so a read of it changes every moment


def sample(n, cells, pattern, seed=0):
    """(n, cells) float32.  'spoiled': a skewed sample with NaN / +-inf sprinkled, cell 0 all NaN, cell 1 constant, cell 2 with one
    valid value (where there are that many cells); 'ties': a handful of distinct values and both zeros; 'wide': magnitudes from
    1e-30 to 1e30 of both signs"""
    rng = np.random.default_rng(7000 + 131 * seed + n + 17 * cells)
    if pattern == 'spoiled':
        x = rng.gumbel(20.0, 6.0, (n, cells)).astype(np.float32)
        u = rng.random((n, cells))
        x[u < 0.08] = np.nan
        x[(u >= 0.08) & (u < 0.10)] = np.inf
        x[(u >= 0.10) & (u < 0.12)] = -np.inf
        x[:, 0] = np.nan
        if cells > 1:
            x[:, 1] = 3.25
        if cells > 2:
            x[:, 2] = np.nan
            x[n // 2, 2] = -1.5
    elif pattern == 'ties':
        x = rng.choice(np.array([0.0, -0.0, 1.0, 1.0, 2.5, -3.0, 10.0], np.float32), (n, cells))
        x[rng.random((n, cells)) < 0.05] = np.nan
    elif pattern == 'wide':
        x = (10.0 ** rng.uniform(-30, 30, (n, cells)) * rng.choice([-1.0, 1.0], (n, cells))).astype(np.float32)
    else:
        raise ValueError(pattern)
    return x


def interleave(x):
    """(n, cells) -> (n, 2, cells) with row 1 of every sample the sentinel: row 0 read at stride 2*cells is x"""
    out = np.full((x.shape[0], 2, x.shape[1]), SENTINEL, np.float32)
    out[:, 0] = x
    return out


def series(n, cells, seed=0):
    """daily precipitation, more or less, for the peaks: dry days, ties with the threshold 10 and with the peak of a cluster, NaN,
    +-inf and -0.0; cell 0 exceeds 10 from the first sample to the last, cell 3 is all NaN (where there are that many cells)"""
    rng = np.random.default_rng(8000 + 131 * seed + n + 17 * cells)
    x = np.round(rng.gamma(0.7, 9.0, (n, cells)), 0).astype(np.float32)          # whole numbers: ties inside clusters
    u = rng.random((n, cells))
    x[u < 0.25] = 0.0
    x[(u >= 0.25) & (u < 0.30)] = -0.0
    x[(u >= 0.30) & (u < 0.35)] = 10.0
    x[(u >= 0.35) & (u < 0.39)] = np.nan
    x[(u >= 0.39) & (u < 0.40)] = np.inf
    x[(u >= 0.40) & (u < 0.41)] = -np.inf
    x[:, 0] = 11.0 + (np.arange(n) % 5 == 2)
    if cells > 3:
        x[:, 3] = np.nan
    return x


def starts(n, P):
    """P = 1: one period; P = 3: three uneven ones, the middle one a single sample (fewer where n does not hold three)"""
    if P == 1 or n == 1:
        return np.array([0, n], np.int64)
    if n == 2:
        return np.array([0, 1, 2], np.int64)
    a = max(1, (2 * n) // 5)
    return np.array([0, a, a + 1, n], np.int64)


def cell_threshold(cells, seed=0):
    """(cells,) thresholds per cell around 10: 10 in cell 0, NaN in cell 1 (where there is more than one cell)"""
    rng = np.random.default_rng(9000 + seed)
    thr = (10.0 + rng.choice([0.0, -6.0, 5.0], cells)).astype(np.float32)
    thr[0] = 10.0
    if cells > 1:
        thr[1] = np.nan
    return thr


def gev_lmoments(loc, scale, shape):
    """analytic (l1, l2, t3) of a GEV with `shape` in the sign of scipy's -c (positive: heavy tail), shape != 0 (Hosking 1990)"""
    from math import gamma
    k = -shape
    g = gamma(1.0 + k)
    l1 = loc + scale * (1.0 - g) / k
    l2 = scale * (1.0 - 2.0 ** -k) * g / k
    t3 = 2.0 * (1.0 - 3.0 ** -k) / (1.0 - 2.0 ** -k) - 3.0
    return l1, l2, t3
