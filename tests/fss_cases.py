"""Seeded inputs of the neighbourhood-verification tests, shared by tests/test_gpu_fss.py (device against tests/fss_ref.py) and
tests/test_fss_api.py (which pins down where the reference may yield NaN).  Imports nothing from the product.

Every case is ``dict(y, p, thresholds, windows, mask, nan_thresholds)``: ``nan_thresholds`` lists the threshold indices whose FSS
is NaN by construction (no event on either side: F + O = 0); everywhere else the FSS is finite."""
import numpy as np

# constants of csrc/neighbourhood.h (shared by fss.hip and ensemble_fss.hip) the shapes below are built around
SEGMENT = 64                  # cells a wave scans at a time (one __ballot)
COLUMNS = 256                 # NB_THREADS: columns per workgroup of the window kernel
PREFIX_ROWS = 32              # NB_PREFIX_ROWS: rows per workgroup of the prefix kernel
THRESHOLD_GROUP = 8           # NB_TG: thresholds handled per pass over the data
WS_BUDGET = 128 << 20         # NB_WS_BUDGET: workspace of one chunk of fields
NARROW_MAX = 65535            # largest window count squared in 32 bits; also the widest row with 16-bit prefixes


def precip(rng, shape):
    """precipitation-like fields: about 60 % exact zeros, values rounded to 0.1 (heavy ties)"""
    v = np.round(rng.gamma(0.6, 3.0, shape), 1) * (rng.random(shape) > 0.6)
    return v.astype(np.float32)


def precip_pair(rng, shape):
    """an observation and a forecast of it that is displaced by (2, -3) cells, rescaled and has spurious showers"""
    y = precip(rng, shape)
    p = np.roll(y, (2, -3), axis=(1, 2)) * rng.uniform(0.5, 1.5, shape) + 0.3 * precip(rng, shape)
    return y, np.round(p, 1).astype(np.float32)


def normal_pair(rng, shape):
    y = rng.standard_normal(shape).astype(np.float32)
    return y, (0.7 * np.roll(y, 1, axis=2) + 0.7 * rng.standard_normal(shape)).astype(np.float32)


def _case(y, p, thresholds, windows, mask=None, nan_thresholds=()):
    return dict(y=y, p=p, thresholds=tuple(thresholds), windows=tuple(windows), mask=mask, nan_thresholds=tuple(nan_thresholds))


def precip512():
    """three 512 x 512 fields; windows at the 32-bit / 64-bit squares' edge (255^2 <= NARROW_MAX < 256^2), around H = W and far
    beyond; few fields, so the window kernel cuts them into bands of rows"""
    y, p = precip_pair(np.random.default_rng(512), (3, 512, 512, 1))
    return _case(y, p, (0.1, 1.0, 5.0), (1, 3, 8, 65, 255, 256, 257, 511, 512, 513, 5000))


def two_channels():
    y, p = normal_pair(np.random.default_rng(96), (4, 96, 104, 2))
    return _case(y, p, (-0.5, 0.0, 0.5, 1.5), (1, 2, 4, 9, 17, 95, 96, 97, 103, 104, 105))


def tiny():
    y, p = normal_pair(np.random.default_rng(9), (5, 9, 8, 1))
    return _case(y, p, (-1.0, 0.0, 1.0), (1, 2, 3, 7, 8, 9, 10, 64, 100000))


def odd_three_channels():
    y, p = precip_pair(np.random.default_rng(65), (2, 65, 63, 3))
    return _case(y, p, (0.1, 2.0), (1, 5, 62, 63, 64, 65, 66, 129))


def single_row():
    y, p = normal_pair(np.random.default_rng(200), (2, 1, 200, 1))
    return _case(y, p, (0.0,), (1, 2, 3, 199, 200, 201))


def single_column():
    y, p = normal_pair(np.random.default_rng(201), (2, 200, 1, 1))
    return _case(y, p, (0.0,), (1, 2, 3, 199, 200, 201))


def width(w):
    """40 rows (more than PREFIX_ROWS) of a width at a SEGMENT or COLUMNS edge"""
    y, p = precip_pair(np.random.default_rng(w), (2, 40, w, 1))
    return _case(y, p, (0.1, 1.0), (1, 4, 33, w - 1, w, w + 1))


def height(h):
    y, p = precip_pair(np.random.default_rng(1000 + h), (2, h, 70, 1))
    return _case(y, p, (0.1,), (1, 2, h - 1, h, h + 1))


NEAR = float(np.float32(0.3)) + 1e-10        # above float32(0.3) as a double, equal to it once cast to float32


def extremes():
    """thresholds below the minimum (every valid cell an event), 0.0 with -0.0 in the data (an event), one that exceeds a data
    value only beyond float32 precision (an event after the cast), and above the maximum (no event: NaN)"""
    r = np.random.default_rng(33)
    y, p = normal_pair(r, (2, 33, 70, 2))
    y, p = np.clip(y, -50, 50), np.clip(p, -50, 50)
    y[:, ::3, ::2], p[:, 1::3, ::2] = -0.0, -0.0
    y[:, ::5, 1::4], p[:, ::4, 1::6] = 0.0, 0.0
    y[:, 2::7, 3::5], p[:, 3::7, 3::5] = np.float32(0.3), np.float32(0.3)
    assert np.signbit(y[y == 0]).any() and not np.signbit(y[y == 0]).all()
    assert np.float32(NEAR) == np.float32(0.3) and NEAR > float(np.float32(0.3))
    return _case(y, p, (-100.0, 0.0, NEAR, 100.0), (1, 2, 5, 33, 70, 71), nan_thresholds=(3,))


def _spoil(r, y, p):
    for a, v in ((y, np.nan), (p, np.nan), (y, np.inf), (p, -np.inf), (y, -np.inf), (p, np.inf)):
        a[r.random(a.shape) < 0.02] = v
    y[0, 0, 0, 0], p[-1, -1, -1, -1] = np.nan, np.inf


def nonfinite_mask2d():
    r = np.random.default_rng(40)
    y, p = precip_pair(r, (3, 40, 70, 2))
    _spoil(r, y, p)
    mask = (r.random((40, 70)) > 0.25).astype(np.float32)
    mask[5:12, 60:] = 0
    return _case(y, p, (0.0, 0.1, 1.0), (1, 2, 7, 40, 200), mask=mask)


def nonfinite_mask_channels():
    r = np.random.default_rng(41)
    y, p = precip_pair(r, (3, 40, 70, 2))
    _spoil(r, y, p)
    mask = (r.random((40, 70, 2)) > 0.25).astype(np.int64)
    mask[:, :9, 1] = 0
    return _case(y, p, (0.1, 1.0), (1, 3, 8, 69), mask=mask)


def threshold_groups():
    """THRESHOLD_GROUP + 1 thresholds: two passes over the data"""
    y, p = normal_pair(np.random.default_rng(8), (2, 50, 70, 1))
    return _case(y, p, np.linspace(-1.5, 1.5, THRESHOLD_GROUP + 1), (1, 6))


def wide_rows():
    """rows longer than NARROW_MAX: 32-bit prefixes; the last window holds 2 * 65541 > NARROW_MAX cells"""
    y, p = normal_pair(np.random.default_rng(7), (1, 2, NARROW_MAX + 6, 1))
    return _case(y, p, (0.0,), (1, 1000, 70000))


def workspace_chunks():
    """four 1024 x 1024 fields at THRESHOLD_GROUP thresholds: 8 * 2 * 1024 * 1025 * 2 B = 32.03 MiB of 16-bit row prefixes per
    field, three fields per WS_BUDGET: two chunks"""
    y, p = precip_pair(np.random.default_rng(1024), (4, 1024, 1024, 1))
    per_field = THRESHOLD_GROUP * 2 * 1024 * 1025 * 2
    assert 1 <= WS_BUDGET // per_field < 4
    return _case(y, p, (0.1, 0.5, 1.0, 2.0, 3.0, 5.0, 8.0, 12.0), (3, 64))


CASES = {'precip512': precip512, 'two_channels': two_channels, 'tiny': tiny, 'odd_three_channels': odd_three_channels,
         'single_row': single_row, 'single_column': single_column, 'extremes': extremes, 'nonfinite_mask2d': nonfinite_mask2d,
         'nonfinite_mask_channels': nonfinite_mask_channels, 'threshold_groups': threshold_groups, 'wide_rows': wide_rows,
         'workspace_chunks': workspace_chunks}
for _w in (SEGMENT - 1, SEGMENT, SEGMENT + 1, COLUMNS - 1, COLUMNS, COLUMNS + 1):
    CASES[f'width{_w}'] = (lambda w=_w: width(w))
for _h in (PREFIX_ROWS - 1, PREFIX_ROWS, PREFIX_ROWS + 1):
    CASES[f'height{_h}'] = (lambda h=_h: height(h))
