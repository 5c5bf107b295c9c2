"""Seeded inputs of the tests of the neighbourhood verification of an ensemble, shared by tests/test_gpu_ensemble_fss.py (device
against tests/ensemble_fss_ref.py) and tests/test_ensemble_fss_api.py (which pins down where the restatement may yield NaN).  Built
from the generators of tests/fss_cases.py; imports nothing from the product.

Every case is ``dict(y, members, thresholds, windows, mask, nan_thresholds)``: ``members`` is (K,) + y.shape, the displaced forecast
of fss_cases plus per-member noise, rounded to 0.1 so that ties with the thresholds are common; ``nan_thresholds`` lists the
threshold indices whose pFSS is NaN by construction (no event on either side: F + K^2 O = 0)."""
import numpy as np

# the constants of csrc/neighbourhood.h the shapes below are built around: one set for both entries.  Here NARROW_MAX is the
# largest K * W with 16-bit prefixes and the largest K * m squared in 32 bits, THRESHOLD_GROUP the thresholds per pass over the stack
from tests.fss_cases import (COLUMNS, NARROW_MAX, NEAR, PREFIX_ROWS, SEGMENT, THRESHOLD_GROUP, WS_BUDGET,  # noqa: F401
                             normal_pair, precip_pair)


def ensemble(rng, p, K, noise=0.4):
    """K members around the forecast ``p``: per-member noise, rounded to 0.1"""
    return np.round(p[None] + noise * rng.standard_normal((K,) + p.shape), 1).astype(np.float32)


def _case(y, members, thresholds, windows, mask=None, nan_thresholds=()):
    return dict(y=y, members=members, thresholds=tuple(thresholds), windows=tuple(windows), mask=mask,
                nan_thresholds=tuple(nan_thresholds))


def _normal(seed, shape, K):
    r = np.random.default_rng(seed)
    y, p = normal_pair(r, shape)
    return np.round(y, 1), ensemble(r, p, K)


def _precip(seed, shape, K):
    r = np.random.default_rng(seed)
    y, p = precip_pair(r, shape)
    return y, ensemble(r, p, K, 0.3)


def tiny():
    y, x = _normal(9, (5, 9, 8, 1), 7)
    return _case(y, x, (-1.0, 0.0, 1.0), (1, 2, 3, 7, 8, 9, 10, 64, 100000))


def width(w, K):
    """40 rows (more than PREFIX_ROWS) of a width at a SEGMENT or COLUMNS edge"""
    y, x = _precip(w, (2, 40, w, 1), K)
    return _case(y, x, (0.1, 1.0), (1, 4, 33, w - 1, w, w + 1))


def height(h):
    y, x = _precip(1000 + h, (2, h, 70, 1), 7)
    return _case(y, x, (0.1,), (1, 2, h - 1, h, h + 1))


def single_row():
    y, x = _normal(200, (2, 1, 200, 1), 16)
    return _case(y, x, (0.0,), (1, 2, 3, 199, 200, 201))


def single_column():
    y, x = _normal(201, (2, 200, 1, 1), 16)
    return _case(y, x, (0.0,), (1, 2, 3, 199, 200, 201))


def two_channels():
    y, x = _normal(96, (2, 33, 35, 2), 64)
    return _case(y, x, (-0.5, 0.0, 0.5, 1.5), (1, 2, 4, 9, 32, 33, 34, 35, 36))


def three_channels():
    y, x = _precip(65, (2, 65, 63, 3), 7)
    return _case(y, x, (0.1, 2.0), (1, 5, 62, 63, 64, 65, 66, 129))


def most_members():
    y, x = _normal(256, (1, 20, 70, 1), 256)
    return _case(y, x, (-0.5, 0.5), (1, 3, 20, 70))


def prefix_edge(K, w):
    """K * W on either side of NARROW_MAX: 16-bit and 32-bit row prefixes"""
    y, x = _normal(K + w, (1, 6, w, 1), K)
    return _case(y, x, (0.0,), (1, 5, w))


def square_edge():
    """K = 16 on 80 x 80: K * m = 16 * 63^2 = 63504 <= NARROW_MAX < 16 * 64^2 = 65536: the 32-bit and the 64-bit squares"""
    y, x = _precip(80, (1, 80, 80, 1), 16)
    return _case(y, x, (0.1, 1.0), (62, 63, 64, 65))


def saturated():
    """the threshold lies between the observation's values and the members': in sample 0 every member forecasts the event and it
    is never observed (cf - K co = K m in the interior), in sample 1 the reverse (-K m); at the edge of the 32-bit squares"""
    y = np.zeros((2, 80, 80, 1), np.float32)
    x = np.ones((16,) + y.shape, np.float32)
    y[1], x[:, 1] = 1.0, 0.0
    return _case(y, x, (0.5,), (1, 63, 64, 200))


def threshold_groups(T):
    """THRESHOLD_GROUP + 1 thresholds: two passes over the stack; 16: the most the entry takes"""
    y, x = _normal(8 + T, (2, 50, 70, 1), 7)
    return _case(y, x, np.linspace(-1.5, 1.5, T), (1, 6))


def extremes():
    """thresholds below the minimum (every valid cell an event on both sides), 0.0 with -0.0 in the data (an event), one that
    exceeds a data value only beyond float32 precision (an event after the cast), and above the maximum (no event: NaN)"""
    r = np.random.default_rng(33)
    y, p = normal_pair(r, (2, 33, 70, 2))
    x = np.clip(ensemble(r, p, 5), -50, 50)
    y = np.clip(y, -50, 50)
    y[:, ::3, ::2], x[1:3, :, 1::3, ::2] = -0.0, -0.0
    y[:, ::5, 1::4], x[0, :, ::4, 1::6] = 0.0, 0.0
    y[:, 2::7, 3::5], x[3:, :, 3::7, 3::5] = np.float32(0.3), np.float32(0.3)
    assert np.signbit(y[y == 0]).any() and not np.signbit(y[y == 0]).all() and np.signbit(x[x == 0]).any()
    assert np.float32(NEAR) == np.float32(0.3) and NEAR > float(np.float32(0.3))
    return _case(y, x, (-100.0, 0.0, NEAR, 100.0), (1, 2, 5, 33, 70, 71), nan_thresholds=(3,))


def _spoil(r, y, x):
    """NaN and both infinities in the observation and in single members"""
    for v in (np.nan, np.inf, -np.inf):
        y[r.random(y.shape) < 0.02] = v
        x[r.integers(0, x.shape[0])][r.random(y.shape) < 0.02] = v
    x[r.random(x.shape) < 0.002] = np.nan
    y[0, 0, 0, 0], x[-1, -1, -1, -1, -1] = np.nan, np.inf


def nonfinite_mask2d():
    r = np.random.default_rng(40)
    y, p = precip_pair(r, (3, 40, 70, 2))
    x = ensemble(r, p, 7, 0.3)
    _spoil(r, y, x)
    mask = (r.random((40, 70)) > 0.25).astype(np.float32)
    mask[5:12, 60:] = 0
    return _case(y, x, (0.0, 0.1, 1.0), (1, 2, 7, 40, 200), mask=mask)


def nonfinite_mask_channels():
    r = np.random.default_rng(41)
    y, p = precip_pair(r, (3, 40, 70, 2))
    x = ensemble(r, p, 2, 0.3)
    _spoil(r, y, x)
    mask = (r.random((40, 70, 2)) > 0.25).astype(np.int64)
    mask[:, :9, 1] = 0
    return _case(y, x, (0.1, 1.0), (1, 3, 8, 69), mask=mask)


def bands():
    """one 300 x 300 field, one threshold: a small grid, so the window kernel cuts the field into bands of rows (at least
    max(n, 32) rows each: ten bands at n = 1, two at n = 150, one from n = 300 on)"""
    y, x = _precip(300, (1, 300, 300, 1), 2)
    return _case(y, x, (0.5,), (1, 2, 31, 33, 150, 299, 300, 301))


CASES = {'tiny': tiny, 'single_row': single_row, 'single_column': single_column, 'two_channels': two_channels,
         'three_channels': three_channels, 'most_members': most_members, 'square_edge': square_edge, 'saturated': saturated,
         'extremes': extremes, 'nonfinite_mask2d': nonfinite_mask2d, 'nonfinite_mask_channels': nonfinite_mask_channels,
         'bands': bands, 'prefix16': lambda: prefix_edge(255, 257), 'prefix32': lambda: prefix_edge(256, 256),
         'thresholds9': lambda: threshold_groups(THRESHOLD_GROUP + 1), 'thresholds16': lambda: threshold_groups(16)}
for _w, _k in zip((SEGMENT - 1, SEGMENT, SEGMENT + 1, COLUMNS - 1, COLUMNS, COLUMNS + 1), (1, 2, 7, 16, 2, 7)):
    CASES[f'width{_w}'] = (lambda w=_w, k=_k: width(w, k))
for _h in (PREFIX_ROWS - 1, PREFIX_ROWS, PREFIX_ROWS + 1):
    CASES[f'height{_h}'] = (lambda h=_h: height(h))
