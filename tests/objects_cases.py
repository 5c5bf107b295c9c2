"""The seeded cases of tests/test_objects_api.py (restatement against scipy), kept apart so that a test of a device labelling
can share them.  CASES[name]() -> dict(x=(N, H, W, C) float32, thr=a scalar or one threshold per field).  The shapes sit on, one
below and one above the edges of tiles of 32 rows x 64 columns (the shape a wave-per-row-segment kernel would take, as the FSS
prefix kernel does) and span up to 3 x 3 of them, and are otherwise as small as the restatement's Python loops like them."""
import numpy as np

TILE_ROWS, TILE_COLS = 32, 64


def _values(event, seed):
    """event cells in [0.5, 1.5), the others in [0, 0.4): float32 (1, H, W, 1) and the threshold 0.5"""
    rng = np.random.default_rng(seed)
    v = np.where(event, 0.5 + rng.random(event.shape), 0.4 * rng.random(event.shape)).astype(np.float32)
    return dict(x=v[None, :, :, None], thr=0.5)


def _stack(cases):
    return dict(x=np.concatenate([c['x'] for c in cases]), thr=np.array([c['thr'] for c in cases], np.float32))


def _random(shape, density, seed):
    rng = np.random.default_rng(seed)
    return dict(x=rng.random(shape).astype(np.float32), thr=float(np.float32(1.0 - density)))


def spiral(H, W):
    """a one-cell-wide arm that winds inwards with one background cell between its turns"""
    a = np.zeros((H, W), bool)
    t, l, b, r, start = 0, 0, H - 1, W - 1, 0
    while b - t >= 0 and r - l >= 0:
        a[t, start:r + 1] = True
        a[t:b + 1, r] = True
        if b - t < 2 or r - l < 2:
            break
        a[b, l:r + 1] = True
        a[t + 2:b + 1, l] = True
        start, t, b, l, r = l, t + 2, b - 2, l + 2, r - 2
    return a


def serpentine(H, W):
    a = np.zeros((H, W), bool)
    a[0::2] = True
    a[1::4, W - 1] = True
    a[3::4, 0] = True
    return a


def comb(H, W):
    """teeth in every other column that join only in the last row"""
    a = np.zeros((H, W), bool)
    a[:, 0::2] = True
    a[H - 1] = True
    return a


def u_shape(H, W):
    a = np.zeros((H, W), bool)
    a[:, 1] = a[:, W - 2] = True
    a[H - 2, 1:W - 1] = True
    a[:H - 4, W // 2] = True                       # a separate bar between the arms
    return a


def rings(H, W):
    i, j = np.mgrid[:H, :W]
    return np.minimum(np.minimum(i, j), np.minimum(H - 1 - i, W - 1 - j)) % 2 == 0


def checkerboard(H, W):
    i, j = np.mgrid[:H, :W]
    return (i + j) % 2 == 0


def _corner(cells):
    a = np.zeros((2 * TILE_ROWS, 2 * TILE_COLS), bool)
    for c in cells:
        a[c] = True
    return a


def diagonal_corners():
    """cells that touch only diagonally across the corner where four tiles meet, in the four orientations: the two diagonals, each
    alone and each with a tail that puts the object's first cell into another tile"""
    r, c = TILE_ROWS, TILE_COLS
    tl, tr, bl, br = (r - 1, c - 1), (r - 1, c), (r, c - 1), (r, c)
    shapes = [[tl, br], [tr, bl], [tl, br, (r + 1, c), (r + 2, c)], [tr, bl, (r, c - 2), (r - 1, c - 2)]]
    return _stack([_values(_corner(s), 40 + k) for k, s in enumerate(shapes)])


def three_channels():
    x = np.random.default_rng(7).random((2, 40, 70, 3)).astype(np.float32)
    return dict(x=x, thr=np.array([0.3, 0.5, 0.7, 0.6, 0.45, 0.8], np.float32))


def nonfinite():
    rng = np.random.default_rng(11)
    x = rng.random((2, 40, 70, 1)).astype(np.float32)
    bad = rng.random(x.shape)
    x[bad < 0.05] = np.nan
    x[(bad >= 0.05) & (bad < 0.08)] = np.inf
    x[(bad >= 0.08) & (bad < 0.11)] = -np.inf
    x[0, 0, :5, 0] = np.nan                        # on the edge of the field
    x[1, 10:20, 10:20, 0] = 0.9                    # a solid object with holes that are not numbers
    x[1, 12, 12, 0], x[1, 15, 10, 0], x[1, 19, 19, 0] = np.nan, np.inf, -np.inf
    return dict(x=x, thr=0.5)


def threshold_edges():
    """field 0: the threshold IS a data value (those cells are events); field 1: the threshold 0.3 + 1e-12 differs from the data
    value float32(0.3) only beyond float32 (events again); field 2: threshold 0.0 with -0.0 in the data (-0.0 >= 0.0 holds) and
    negative values next to it; field 3: a negative threshold, objects of negative values"""
    rng = np.random.default_rng(13)
    x = rng.random((4, 20, 70, 1)).astype(np.float32)
    x[0, 5:9, 5:30, 0] = x[0, 0, 0, 0] = np.float32(0.625)
    x[1, 5:9, 5:30, 0] = np.float32(0.3)
    x[1][x[1] > 0.3] *= np.float32(0.25)
    x[2] -= np.float32(0.5)
    x[2, 3:6, 60:68, 0] = np.float32(-0.0)
    x[2, 10, :, 0] = np.float32(-0.0)
    x[2, 11, :, 0] = np.float32(-1e-30)
    x[3] = -x[3] - np.float32(0.25)
    return dict(x=x, thr=np.array([0.625, 0.3 + 1e-12, 0.0, -0.6], np.float64))


CASES = {
    'one_cell': lambda: dict(x=np.ones((1, 1, 1, 1), np.float32), thr=0.5),
    'single_row': lambda: _random((2, 1, 130, 1), 0.6, 1),
    'single_column': lambda: _random((2, 130, 1, 1), 0.6, 2),
    'h31_w63': lambda: _random((1, 31, 63, 1), 0.5, 3),
    'h32_w64': lambda: _random((1, 32, 64, 1), 0.5, 4),
    'h33_w65': lambda: _random((1, 33, 65, 1), 0.5, 5),
    'h65_w127': lambda: _random((1, 65, 127, 1), 0.5, 6),
    'h33_w128': lambda: _random((1, 33, 128, 1), 0.5, 8),
    'h65_w129': lambda: _random((1, 65, 129, 1), 0.5, 9),
    'three_channels': three_channels,
    'all_event': lambda: _values(np.ones((33, 65), bool), 20),
    'no_event': lambda: _values(np.zeros((33, 65), bool), 21),
    'checkerboard': lambda: _values(checkerboard(34, 66), 22),
    'diagonal_corners': diagonal_corners,
    'spiral': lambda: _values(spiral(3 * TILE_ROWS + 1, 3 * TILE_COLS + 1), 23),
    'serpentine': lambda: _values(serpentine(3 * TILE_ROWS + 1, 3 * TILE_COLS + 1), 24),
    'u_and_comb': lambda: _stack([_values(u_shape(70, 130), 25), _values(comb(70, 130), 26)]),
    'nested_rings': lambda: _values(rings(70, 130), 27),
    'random_005': lambda: _random((1, 70, 130, 1), 0.05, 30),
    'random_04': lambda: _random((1, 70, 130, 1), 0.4, 31),
    'random_06': lambda: _random((1, 70, 130, 1), 0.6, 32),
    'random_095': lambda: _random((1, 70, 130, 1), 0.95, 33),
    'nonfinite': nonfinite,
    'threshold_edges': threshold_edges,
}


def field_thresholds(case):
    """the thresholds of a case as float32, one per field"""
    n, _, _, c = case['x'].shape
    return np.broadcast_to(np.asarray(case['thr'], np.float64).astype(np.float32).reshape(-1), (n * c,)).copy()
