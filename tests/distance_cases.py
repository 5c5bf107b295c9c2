"""Seeded cases of the distance-map verification, each at most 97 x 193 cells: name -> a function that
returns dict(y, p (N, H, W, C) float32, thresholds, cutoff (None: the field diagonal), alpha).  `reference(name)` is the
restatement's answer, computed once per process and shared by every test that needs it; it must not be written to.

The hand-worked case `shifted`: on a 30 x 40 field the observed events are the block rows 10..14 x columns 20..27 and the predicted
ones the same block moved by (3, -5), rows 13..17 x columns 15..22.  n_A = n_B = 40, the blocks share rows 13..14 x columns 20..22:
n_AB = 6, n_valid = 1200.  For a in A, d2(a, B) = max(0, 13 - i)^2 + max(0, j - 22)^2: the rows give 9 + 4 + 1 + 0 + 0 = 14 for each of
the 8 columns, the columns 1 + 4 + 9 + 16 + 25 = 55 for each of the 5 rows: sum_d2_AB = 112 + 275 = 387, max_d2_AB = 9 + 25 = 34 at
the corner (10, 27).  The move is a point reflection of the pair, so B to A gives the same: Hausdorff = sqrt(34), the RMS distance
sqrt(387 / 40) both ways."""
import functools
import math

import numpy as np

from tests import distance_ref

ALPHA = 1.0 / 9.0


def _case(y, p, thresholds, cutoff=None, alpha=ALPHA):
    y, p = (np.ascontiguousarray(a, np.float32) for a in (y, p))
    assert y.shape == p.shape and y.ndim == 4 and y.shape[1] <= 97 and y.shape[2] <= 193
    return dict(y=y, p=p, thresholds=np.asarray(thresholds, np.float32).reshape(-1), cutoff=cutoff, alpha=alpha)


def _random(seed, shape, density, thresholds=None):
    rng = np.random.default_rng(seed)
    y, p = rng.random(shape, np.float32), rng.random(shape, np.float32)
    return _case(y, p, [1.0 - density] if thresholds is None else thresholds)


def _zeros(h, w, n=1, c=1):
    return np.zeros((n, h, w, c), np.float32)


def one_cell():
    y, p = _zeros(1, 1, 3), _zeros(1, 1, 3)
    y[0], p[0], y[1] = 1, 1, 1                                           # both events; only the observation; neither
    return _case(y, p, [0.5])


def corners():
    """one event in each corner against one in the opposite corner: the Hausdorff distance is the diagonal, every sum has one term"""
    h, w = 17, 23
    y, p = _zeros(h, w, 4), _zeros(h, w, 4)
    for n, (i, j) in enumerate(((0, 0), (0, w - 1), (h - 1, 0), (h - 1, w - 1))):
        y[n, i, j, 0], p[n, h - 1 - i, w - 1 - j, 0] = 1, 1
    return _case(y, p, [0.5])


def column_and_row():
    y, p = _zeros(33, 65), _zeros(33, 65)
    y[0, :, 5, 0], p[0, 7, :, 0] = 1, 1
    return _case(y, p, [0.5])


def gap_columns():
    """columns without any event between full ones"""
    y = _zeros(20, 129)
    y[0, :, :10, 0], y[0, :, 70:72, 0], y[0, :, 120:, 0] = 1, 1, 1
    p = np.random.default_rng(11).random(y.shape, np.float32)
    p[0, :, 30:60, 0] = 0
    return _case(y, p, [0.9])


def checkerboard():
    i, j = np.indices((32, 64))
    y = ((i + j) % 2).astype(np.float32)[None, :, :, None]
    return _case(y, 1 - y, [0.5])


def identical():
    c = _random(12, (2, 40, 70, 1), 0.05)
    return _case(c['y'], c['y'].copy(), c['thresholds'])


def shifted():
    y, p = _zeros(30, 40), _zeros(30, 40)
    y[0, 10:15, 20:28, 0], p[0, 13:18, 15:23, 0] = 1, 1
    return _case(y, p, [0.5])


def empty_pred():
    c = _random(13, (1, 31, 64, 1), 0.05)
    return _case(c['y'], np.zeros_like(c['p']), c['thresholds'])


def empty_obs_infinite_cutoff():
    c = _random(14, (1, 20, 30, 1), 0.05)
    return _case(np.zeros_like(c['y']), c['p'], c['thresholds'], cutoff=math.inf)


def empty_both():
    return _case(_zeros(12, 65), _zeros(12, 65), [0.5])


def empty_both_infinite_cutoff():
    return _case(_zeros(12, 65), _zeros(12, 65), [0.5], cutoff=math.inf)


def all_event():
    return _case(_zeros(33, 65) + 1, _zeros(33, 65) + 1, [0.5], cutoff=2.5)


def nonfinite():
    """NaN and +-inf cells inside and beside events, in both arrays"""
    rng = np.random.default_rng(15)
    y, p = rng.random((2, 33, 70, 1), np.float32), rng.random((2, 33, 70, 1), np.float32)
    y[0, 5:9, 10:20], p[0, 20:25, 30:50] = 0.95, 0.95                   # event blocks ...
    y[0, 6, 12:15], y[0, 7, 19], y[0, 4, 10] = np.nan, np.inf, -np.inf    # ... with holes inside and non-finite neighbours
    p[0, 22, 35:40], p[0, 19, 30], p[0, 25, 49] = np.inf, np.nan, -np.inf
    for a in (y, p):
        a[1][rng.random(a[1].shape) < 0.1] = np.nan
        a[1][rng.random(a[1].shape) < 0.02] = np.inf
    y[1, 0, 0], p[1, 32, 69] = np.nan, np.nan
    return _case(y, p, [0.9, 0.95])


def threshold_equals_data():
    rng = np.random.default_rng(16)
    levels = np.array([0, 0.25, 0.5, 0.75, 1], np.float32)
    return _case(levels[rng.integers(0, 5, (1, 31, 63, 1))], levels[rng.integers(0, 5, (1, 31, 63, 1))], [0.5, 0.75, 1.0])


def signed_zero():
    rng = np.random.default_rng(17)
    levels = np.array([0.0, -0.0, -1.0, -1.0, -1.0, -1.0], np.float32)
    return _case(levels[rng.integers(0, 6, (1, 32, 65, 1))], levels[rng.integers(0, 6, (1, 32, 65, 1))], [0.0, -0.0])


CASES = dict(
    one_cell=one_cell, single_row=lambda: _random(1, (2, 1, 70, 1), 0.1), single_column=lambda: _random(2, (2, 70, 1, 1), 0.1),
    w63=lambda: _random(3, (1, 9, 63, 1), 0.05), w64=lambda: _random(4, (1, 9, 64, 1), 0.05), w65=lambda: _random(5, (1, 9, 65, 1), 0.05),
    w127=lambda: _random(6, (1, 9, 127, 1), 0.03), w128=lambda: _random(7, (1, 9, 128, 1), 0.03),
    w129=lambda: _random(8, (2, 9, 129, 1), 0.03), h31=lambda: _random(9, (1, 31, 20, 1), 0.05), h32=lambda: _random(10, (1, 32, 20, 1), 0.05),
    h33=lambda: _random(18, (1, 33, 20, 1), 0.05), h65=lambda: _random(19, (1, 65, 20, 1), 0.05),
    three_channels=lambda: _random(20, (2, 20, 30, 3), None, [0.3, 0.6, 0.9]),
    nine_thresholds=lambda: _random(21, (1, 24, 40, 2), None, np.linspace(0.1, 0.99, 9)),
    random_0001=lambda: _random(22, (1, 97, 193, 1), 0.001), random_005=lambda: _random(23, (1, 97, 193, 1), 0.05),
    random_05=lambda: _random(24, (1, 48, 129, 1), 0.5), random_095=lambda: _random(25, (1, 33, 65, 1), 0.95),
    corners=corners, column_and_row=column_and_row, gap_columns=gap_columns, checkerboard=checkerboard, identical=identical,
    shifted=shifted, empty_pred=empty_pred, empty_obs_infinite_cutoff=empty_obs_infinite_cutoff, empty_both=empty_both,
    empty_both_infinite_cutoff=empty_both_infinite_cutoff, all_event=all_event, nonfinite=nonfinite,
    threshold_equals_data=threshold_equals_data, signed_zero=signed_zero)


def cutoff_of(case):
    """the cutoff as `check_distance_args` fills it in"""
    _, H, W, _ = case['y'].shape
    return case['cutoff'] if case['cutoff'] is not None else (math.sqrt((H - 1) ** 2 + (W - 1) ** 2) or 1.0)


@functools.lru_cache(maxsize=None)
def reference(name):
    """-> (the case, distance_ref.distance of it); shared: read only"""
    case = CASES[name]()
    ref = distance_ref.distance(case['y'], case['p'], case['thresholds'], cutoff_of(case), case['alpha'])
    for a in list(case.values()) + list(ref.values()):
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return case, ref
