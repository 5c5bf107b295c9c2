"""Seeded inputs of the distribution-verification tests, shared by tests/test_gpu_distribution.py (device against
tests/distribution_ref.py) and tests/test_distribution_api.py (which pins down where the reference may yield NaN).  Imports nothing
from the product.

Every case is ``dict(y, p, quantiles, bins, over, mask, empty)``: ``empty`` is the number of segments without a valid element by
construction (their quantiles, W1, KS and Perkins score are NaN); everywhere else the expected arrays are finite."""
import numpy as np

# constants of csrc/distribution.hip and csrc/sort_keys.h the shapes below are built around
LDS_MAX = 8192                # DS_LDS_MAX: longest contiguous segment sorted in LDS
STRIDED_MAX = 512             # DS_STRIDED_MAX: longest segment of the strided LDS engine
TILE = 4096                   # SORT_TILE: elements per tile of the global engine
WS_BUDGET = 128 << 20         # SORT_WS_BUDGET: workspace of one chunk of segments of the global engine
MAX_Q, MAX_E = 64, 257        # caps of the C entry


def strided_group(n):
    """G of the strided engine at segment length n: the segments a workgroup takes (launch_strided)"""
    assert 1 <= n <= STRIDED_MAX
    return 64 if n <= 64 else 32 if n <= 128 else 16


def global_bytes_per_segment(n):
    """workspace of one segment of the global engine (Workspace, for one segment): three key buffers, digit counts, two partials per tile"""
    al = lambda b: (b + 255) & ~255
    tiles = max(1, -(-n // TILE))
    return 3 * al(n * 4) + al(tiles * 1024) + al(tiles * 8) + al(tiles * 4)


QUANTILES = (0.01, 0.05, 0.25, 0.5, 0.75, 0.95, 0.99)
PRECIP_BINS = (0.0, 0.1, 1.0, 2.0, 5.0, 10.0, 20.0, 50.0)
NORMAL_BINS = tuple(np.linspace(-3.0, 3.0, 13))


def precip(rng, shape, zeros=0.6):
    """precipitation-like: about 60 % exact zeros, values rounded to 0.1 (heavy ties)"""
    v = np.round(rng.gamma(0.6, 3.0, shape), 1) * (rng.random(shape) > zeros)
    return v.astype(np.float32)


def precip_pair(rng, shape, zeros=0.6):
    y = precip(rng, shape, zeros)
    p = np.round(0.8 * precip(rng, shape, zeros) + 0.3 * precip(rng, shape, zeros), 1).astype(np.float32)
    return y, p


def normal_pair(rng, shape):
    y = rng.standard_normal(shape).astype(np.float32)
    return y, (0.9 * rng.standard_normal(shape) + 0.2).astype(np.float32)


def _case(y, p, over, quantiles=QUANTILES, bins=None, mask=None, empty=0):
    return dict(y=y, p=p, quantiles=tuple(quantiles), bins=None if bins is None else tuple(bins), over=over, mask=mask, empty=empty)


def space(length, seed, n=3):
    """n samples of `length` values each: the one-segment LDS engine up to LDS_MAX, the global engine beyond"""
    r = np.random.default_rng(seed)
    y, p = precip_pair(r, (n, 1, length, 1)) if seed % 2 else normal_pair(r, (n, 1, length, 1))
    return _case(y, p, 'space', bins=PRECIP_BINS if seed % 2 else NORMAL_BINS)


def space_3d():
    y, p = precip_pair(np.random.default_rng(575), (5, 7, 5, 3))
    return _case(y, p, 'space', bins=PRECIP_BINS)


def time(n, cells, seed):
    """n samples of a (1, cells, 1) or (7, 5, 3) grid: the strided LDS engine up to STRIDED_MAX, the global engine beyond"""
    r = np.random.default_rng(seed)
    shape = (n, 7, 5, 3) if cells == 105 else (n, 2, 3, 1) if cells == 6 else (n, 1, cells, 1)
    y, p = precip_pair(r, shape) if seed % 2 else normal_pair(r, shape)
    return _case(y, p, 'time', bins=PRECIP_BINS if seed % 2 else NORMAL_BINS)


def single_column_grid():
    """a grid of 3 x 1 cells: a band of one row is one segment with both strides 1; longer than STRIDED_MAX: the global engine"""
    y, p = normal_pair(np.random.default_rng(600), (STRIDED_MAX + 88, 3, 1, 1))
    return _case(y, p, 'time', bins=NORMAL_BINS)


def workspace_chunks():
    """STRIDED_MAX + 1 samples of 128 x 130 cells through the global engine: more segments than one workspace chunk holds"""
    n, h, w = STRIDED_MAX + 1, 128, 130
    assert h * w * global_bytes_per_segment(n) > WS_BUDGET
    y, p = normal_pair(np.random.default_rng(130), (n, h, w, 1))
    return _case(y, p, 'time', quantiles=(0.05, 0.5, 0.95), bins=(-1.0, 0.0, 1.0))


def zeros70():
    y, p = precip_pair(np.random.default_rng(70), (40, 7, 5, 1), zeros=0.7)
    assert 0.6 < (y == 0).mean() < 0.8
    return _case(y, p, 'time', bins=PRECIP_BINS)


def signed_zeros():
    """+0.0 and -0.0 mixed on both sides: one tie group, counted in the bin that starts at 0"""
    r = np.random.default_rng(5)
    y, p = normal_pair(r, (50, 4, 5, 1))
    for a in (y, p):
        a[r.random(a.shape) < 0.3] = 0.0
        a[r.random(a.shape) < 0.3] = -0.0
    assert np.signbit(y[y == 0]).any() and not np.signbit(y[y == 0]).all()
    return _case(y, p, 'time', bins=(-2.0, 0.0, 2.0))


def all_equal():
    y = np.full((30, 3, 4, 1), 2.5, np.float32)
    return _case(y, y.copy() + np.float32(0.5), 'time', bins=(0.0, 2.5, 3.0))


def _spoil(r, y, p):
    for a, v in ((y, np.nan), (p, np.nan), (y, np.inf), (p, -np.inf), (y, -np.inf), (p, np.inf)):
        a[r.random(a.shape) < 0.03] = v
    y[0, 0, 0, 0], p[-1, -1, -1, -1] = np.nan, np.inf


def nonfinite_time():
    r = np.random.default_rng(44)
    y, p = precip_pair(r, (60, 6, 7, 2))
    _spoil(r, y, p)
    return _case(y, p, 'time', bins=PRECIP_BINS)


def nonfinite_space():
    r = np.random.default_rng(45)
    y, p = normal_pair(r, (4, 30, 31, 1))
    _spoil(r, y, p)
    return _case(y, p, 'space', bins=NORMAL_BINS)


def masked_cells():
    """a 2-D mask removes 11 cells at every time, in both channels: 22 segments without a valid element"""
    r = np.random.default_rng(46)
    y, p = precip_pair(r, (37, 6, 7, 2))
    mask = np.ones((6, 7), np.float32)
    mask[1, 2:6], mask[4:, 0], mask[3, 1:6] = 0, 0, 0
    assert int((mask == 0).sum()) == 11
    return _case(y, p, 'time', bins=PRECIP_BINS, mask=mask, empty=22)


def single_valid_element():
    """the segment of cell (0, 0, 0) is valid at one time only; its neighbour has none"""
    r = np.random.default_rng(47)
    y, p = normal_pair(r, (20, 2, 3, 1))
    y[:, 0, 0, 0] = np.nan
    y[7, 0, 0, 0] = 1.25
    p[:, 0, 1, 0] = np.inf
    return _case(y, p, 'time', bins=NORMAL_BINS, empty=1)


def quantiles_0_and_1():
    y, p = normal_pair(np.random.default_rng(48), (37, 3, 4, 1))
    return _case(y, p, 'time', quantiles=(0.0, 1.0, 0.5, 1.0 - 2.0 ** -53, 2.0 ** -60))


def caps():
    """MAX_Q quantiles and MAX_E bin edges"""
    y, p = normal_pair(np.random.default_rng(49), (100, 3, 4, 1))
    return _case(y, p, 'time', quantiles=np.linspace(0.0, 1.0, MAX_Q), bins=np.linspace(-4.0, 4.0, MAX_E))


def no_bins():
    y, p = precip_pair(np.random.default_rng(50), (37, 3, 4, 2))
    return _case(y, p, 'time')


CASES = {'space_3d': space_3d, 'single_column_grid': single_column_grid, 'workspace_chunks': workspace_chunks, 'zeros70': zeros70, 'signed_zeros': signed_zeros,
         'all_equal': all_equal, 'nonfinite_time': nonfinite_time, 'nonfinite_space': nonfinite_space, 'masked_cells': masked_cells,
         'single_valid_element': single_valid_element, 'quantiles_0_and_1': quantiles_0_and_1, 'caps': caps, 'no_bins': no_bins}
# the one-segment LDS engine: lengths 1, 2, 3, 37, a power of two, the limit; the global engine: the limit + 1, three tiles + 5
for _l in (1, 2, 3, 37, 1024, LDS_MAX):
    CASES[f'space{_l}'] = (lambda l=_l: space(l, l, n=1 if l == LDS_MAX else 3))
CASES[f'space{LDS_MAX + 1}'] = lambda: space(LDS_MAX + 1, LDS_MAX + 1, n=2)
CASES[f'space{3 * TILE + 5}'] = lambda: space(3 * TILE + 5, 3 * TILE + 5, n=1)
# the strided LDS engine on 105 cells, on G + 1 cells, at its longest segment; the global engine just beyond
for _n in (1, 2, 37, 365):
    CASES[f'time{_n}x105'] = (lambda n=_n: time(n, 105, n))
for _n in (37, 100, 365):
    CASES[f'time{_n}x{strided_group(_n) + 1}'] = (lambda n=_n: time(n, strided_group(n) + 1, n + 1000))
CASES[f'time{STRIDED_MAX}x6'] = lambda: time(STRIDED_MAX, 6, STRIDED_MAX)
CASES[f'time{STRIDED_MAX + 1}x6'] = lambda: time(STRIDED_MAX + 1, 6, STRIDED_MAX + 1)
