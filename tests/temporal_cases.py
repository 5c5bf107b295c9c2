"""Seeded cases of the temporal-verification tests, shared by tests/test_temporal_api.py (CPU) and tests/test_gpu_temporal.py.
The data are small integers and halves in float32, so every product and most sums are exact, with NaN, +-inf and -0.0 strewn in;
a spike of 1e30 in one cell, taken away again later, makes a sum that was added in another order show."""
import numpy as np

GROUP = 256                    # cells per workgroup of temporal_kernel (csrc/temporal.hip: TMP_CELLS)
DEPTH = 8                      # samples a lane loads at once (TMP_DEPTH)
RING = 32                      # the LDS ring and the largest lag (TMP_RING)
CELLS = (1, 63, 64, 65, GROUP + 1)
LENGTHS = (1, 2, 4, 5, 9, 33, 34, 97)
PERIOD_KINDS = ('one', 'uneven', 'each')
LAG_SETS = ((), (1,), (1, 2, 5, 32), (32,), (2, 3), (1, 4, 31))
SCALARS = (1.0, 3.0, 0.0, 5.5)
BINS = (1, 2, 16, 32)
TREND_PERIODS = (1, 2, 3, 4, 5, 32, 33, 64, 65, 127, 128)


def series(n, cells, seed=0):
    """(n, cells) float32: halves between 0 and 8 with many zeros (dry days), persistent in time so that long runs occur.
    Cell 0 is one event run from the first sample to the last, cell 2 carries the spike of 1e30 and later -1e30, cell 3 is all NaN, cell 5 has one
    valid sample, cell 7 is an event run up to the last sample after an invalid first one"""
    rng = np.random.default_rng(5000 + seed)
    x = (rng.integers(0, 17, (n, cells)) / 2).astype(np.float32)
    keep = rng.random((n, cells)) < 0.6                                  # persistence: a sample repeats the one before
    for i in range(1, n):
        x[i] = np.where(keep[i], x[i - 1], x[i])
    x[rng.random((n, cells)) < 0.2] = 0.0
    u = rng.random((n, cells))
    x[u < 0.05] = np.nan
    x[(u >= 0.05) & (u < 0.06)] = np.inf
    x[(u >= 0.06) & (u < 0.07)] = -np.inf
    x[(u >= 0.07) & (u < 0.11)] = -0.0
    x[:, 0] = 6.0 + (np.arange(n) % 5).astype(np.float32) / 2
    if cells > 2:
        x[n // 3, 2] = 1e30                                             # swallows what is added to it ...
        x[(2 * n) // 3, 2] = -1e30                                      # ... until it is taken away again
    if cells > 3:
        x[:, 3] = np.nan
    if cells > 5:
        x[:, 5] = np.nan
        x[n // 2, 5] = 1.5
    if cells > 7:
        x[:, 7] = 7.0
        x[0, 7] = np.inf
    return x


def second(n, cells, seed=0):
    """a second series on the same grid whose NaN lie elsewhere, so that common validity matters"""
    x = series(n, cells, seed + 77)
    x[:, :1] = series(n, cells, seed)[:, :1] + np.float32(0.5)
    if cells > 2:
        x[:, 2] = np.where(np.abs(x[:, 2]) < 100, x[:, 2], np.float32(2.0))
    if cells > 3:
        x[:, 3] = 1.0                                                   # valid here, all NaN in the first series
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
    rng = np.random.default_rng(6000 + seed)
    thr = (np.asarray(SCALARS[:T], np.float32)[:, None] + rng.choice([0.0, 0.5, 2.0], (T, cells))).astype(np.float32)
    thr[T - 1, min(1, cells - 1)] = np.nan
    return thr


def trend_values(P, cells, seed=0):
    """(P, cells) float64 annual values: a trend plus noise in most cells, heavy ties (five integers) in every fourth cell, signed
    zeros in every seventh, NaN gaps; cell 1 has no valid value, cell 2 one, cell 3 two (where P allows), cell 4 is all tied,
    cell 6 is strictly increasing"""
    rng = np.random.default_rng(7000 + seed)
    t = np.arange(P, dtype=np.float64)[:, None]
    v = np.round(rng.normal(0, 4, (P, cells)) + 0.25 * t * rng.choice([-1.0, 0.0, 1.0], (1, cells)), 2)
    tied = np.arange(cells) % 4 == 0
    v[:, tied] = rng.integers(0, 5, (P, int(tied.sum()))).astype(np.float64)
    zeros = np.arange(cells) % 7 == 0
    v[:, zeros] = rng.choice([-0.0, 0.0, 1.0], (P, int(zeros.sum())))
    v[rng.random((P, cells)) < 0.08] = np.nan
    if cells > 1:
        v[:, 1] = np.nan
    if cells > 2:
        v[:, 2] = np.nan
        v[P // 2, 2] = 3.0
    if cells > 3:
        v[:, 3] = np.nan
        v[0, 3], v[P - 1, 3] = 1.0, -2.0
    if cells > 4:
        v[:, 4] = 2.5
    if cells > 6:
        v[:, 6] = t[:, 0] * 0.5 - 3.0
    return v


def reaches(x, st, lags, thr, bins):
    """what a case must contain to test the kernel's walk: (the longest event run of threshold `thr` inside a period, whether a
    valid lag pair spans two load blocks of a period, whether a run is longer than `bins`, whether a cell is all NaN)"""
    ok = np.isfinite(x)
    ev = ok & (np.where(x == 0, np.float32(0), x) >= np.float32(thr))
    longest, spans = 0, False
    for p in range(len(st) - 1):
        run = np.zeros(x.shape[1], np.int64)
        for i in range(st[p + 1] - st[p]):
            run = np.where(ev[st[p] + i], run + 1, 0)
            longest = max(longest, int(run.max()))
            for k in lags:
                if i - k >= 0 and i // DEPTH != (i - k) // DEPTH and (ok[st[p] + i] & ok[st[p] + i - k]).any():
                    spans = True
    return longest, spans, longest > bins, bool(np.isnan(x).all(axis=0).any())
