"""Seeded cases of the climate-index tests, shared by tests/test_indices_api.py (CPU) and tests/test_gpu_indices.py."""
import numpy as np

GROUP = 256                    # cells per workgroup of climate_indices_kernel (csrc/indices.hip: IDX_CELLS)
DEPTH = 8                      # samples a lane loads at once (IDX_DEPTH)
WINDOW = 5
CELLS = (1, 63, 64, 65, GROUP + 1)
LENGTHS = (1, 2, WINDOW - 1, WINDOW, WINDOW + 1, DEPTH - 1, DEPTH + 1, 97)
PERIOD_KINDS = ('one', 'uneven', 'each')
SCALARS = (1.0, 10.0, 20.0, 0.0)


def field(n, cells, seed=0):
    """daily precipitation, more or less: dry days, ties with the thresholds 1 and 10, a long tail"""
    rng = np.random.default_rng(1000 + seed)
    x = rng.gamma(0.6, 6.0, (n, cells)).astype(np.float32)
    x[rng.random((n, cells)) < 0.35] = 0.0
    x[rng.random((n, cells)) < 0.05] = 1.0
    x[rng.random((n, cells)) < 0.03] = 10.0
    return x


def spoiled(n, cells, seed=0):
    """`field` with NaN, +-inf and -0.0 strewn in; cell 0 is one event run from the first sample to the last, cell 3 is all NaN,
    cell 5 has one valid sample, cell 7 is an event run up to the last sample after an invalid first one"""
    rng = np.random.default_rng(2000 + seed)
    x = field(n, cells, seed)
    u = rng.random((n, cells))
    x[u < 0.06] = np.nan
    x[(u >= 0.06) & (u < 0.07)] = np.inf
    x[(u >= 0.07) & (u < 0.08)] = -np.inf
    x[(u >= 0.08) & (u < 0.12)] = -0.0
    x[:, 0] = 50.0 + np.arange(n, dtype=np.float32) / 8
    if cells > 3:
        x[:, 3] = np.nan
    if cells > 5:
        x[:, 5] = np.nan
        x[n // 2, 5] = 1.25
    if cells > 7:
        x[:, 7] = 30.0
        x[0, 7] = np.inf
    return x


def temperatures(n, cells, seed=0):
    """daily temperatures around the two thresholds 0 and 25, with signed zeros"""
    rng = np.random.default_rng(3000 + seed)
    x = (12.0 + 14.0 * np.sin(np.arange(n)[:, None] * (2 * np.pi / 30.0)) + rng.normal(0, 4, (n, cells))).astype(np.float32)
    u = rng.random((n, cells))
    x[u < 0.05] = 0.0
    x[(u >= 0.05) & (u < 0.10)] = -0.0
    x[(u >= 0.10) & (u < 0.13)] = 25.0
    x[(u >= 0.13) & (u < 0.16)] = np.nan
    return x


def starts(n, kind):
    """period starts over n samples: 'one' period; 'uneven': three of unequal length, the middle one a single sample (fewer where n
    does not hold three); 'each': every sample its own period"""
    if kind == 'one' or n == 1:
        return np.array([0, n], np.int64)
    if kind == 'each':
        return np.arange(n + 1, dtype=np.int64)
    if n == 2:
        return np.array([0, 1, 2], np.int64)
    a = max(1, (2 * n) // 5)
    return np.array([0, a, a + 1, n], np.int64)


def cell_thresholds(T, cells, seed=0):
    """(T, cells) thresholds per cell, NaN in one cell of one t only (cell 1 of the last t)"""
    rng = np.random.default_rng(4000 + seed)
    thr = (np.asarray(SCALARS[:T], np.float32)[:, None] + rng.choice([0.0, 0.5, 2.0], (T, cells))).astype(np.float32)
    thr[T - 1, min(1, cells - 1)] = np.nan
    return thr


def reaches(x, st, window):
    """what a case must contain to test the kernel's walk: (the longest stretch of valid samples inside a period, whether a
    window of all-valid samples spans two load blocks of a period, whether NaN occurs, whether +-inf occurs)"""
    ok = np.isfinite(x)
    longest, spans = 0, False
    for p in range(len(st) - 1):
        run = np.zeros(x.shape[1], np.int64)
        for i in range(st[p + 1] - st[p]):
            run = np.where(ok[st[p] + i], run + 1, 0)
            longest = max(longest, int(run.max()))
            if i % DEPTH < window - 1 and i >= DEPTH and (run >= window).any():      # the window ending at i began in the block before
                spans = True
    return longest, spans, bool(np.isnan(x).any()), bool(np.isinf(x).any())
