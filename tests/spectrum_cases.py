"""Seeded inputs of the spectral-verification tests, shared by tests/test_gpu_spectral.py (device against tests/spectrum_ref.py) and
tests/test_spectral_api.py (which measures C_REF on them and pins down where the reference may yield NaN).  Imports nothing from
the product.  Every case is a dict: y, p (N, H, W, C) float32, bins ('radial' or an int32 (H, W) map), detrend, window, mask,
empty (the number of fields built to have no kept cell)."""
import numpy as np

# constants of csrc/spectrum.hip and csrc/sort_keys.h the shapes below are built around
WS_BUDGET = 128 << 20                              # workspace of one chunk of fields
ROW_TILE, COL_TILE, K_STEP = 128, 64, 16           # rows x kx of the row transform's tile, ky = kx of the column transform's, K step
MAX_DIM, MAX_BINS = 16384, 16384

# Error model of the comparison.  C_REF: the largest coefficient-wise |np.fft.fft2 - matrix-product DFT| /
# (2^-52 sqrt(T)) between the two CPU references over the cases below (tests/test_spectral_api.py asserts that it is not exceeded;
# `workspace_chunks` enters with its first four fields).  The device sums rows of up to 256 terms sequentially or in tiles, which
# may exceed pocketfft's log-depth sums by sqrt(256): C = 16 C_REF.
C_REF = 0.45
C = 16 * C_REF


def bytes_per_field(H, W):
    """workspace of one field with two sides: two complex fp64 row transforms and four fp64 products per half-plane coefficient"""
    return 64 * H * (W // 2 + 1)


def precip(rng, shape):
    """precipitation-like: 60 % exact zeros, the rest gamma-distributed"""
    v = rng.gamma(0.6, 4.0, shape)
    v[rng.random(shape) < 0.6] = 0.0
    return v.astype(np.float32)


def _pair(seed, shape, kind='normal'):
    rng = np.random.default_rng(seed)
    if kind == 'precip':
        y = precip(rng, shape)
        p = (0.8 * y + 0.3 * precip(rng, shape)).astype(np.float32)
    elif kind == 'offset':
        y = (280.0 + rng.standard_normal(shape)).astype(np.float32)
        p = (280.5 + 0.7 * rng.standard_normal(shape)).astype(np.float32)
    else:
        y = rng.standard_normal(shape).astype(np.float32)
        p = (0.6 * y + 0.5 * rng.standard_normal(shape)).astype(np.float32)
    return y, p


def _case(seed, shape, kind='normal', bins='radial', detrend='mean', window=None, mask=None, empty=0, edit=None):
    def make():
        y, p = _pair(seed, shape, kind)
        if edit is not None:
            edit(y, p)
        b = bins(shape[1], shape[2]) if callable(bins) else bins
        m = mask(shape[1], shape[2]) if callable(mask) else mask
        return dict(y=y, p=p, bins=b, detrend=detrend, window=window, mask=m, empty=empty)
    return make


def _nonfinite(y, p):
    y[0, 1, 2, 0] = np.nan
    y[0, 3, 0, 0] = np.inf
    p[0, 0, 4, 0] = -np.inf
    p[0, 4, 1, 0] = np.nan
    p[0, 1, 2, 0] = np.inf                          # (where y is NaN already)
    y[-1, 2, 2, -1] = -np.inf


def _one_field_masked(y, p):
    y[1] = np.nan


def _mask2d(H, W):
    m = np.ones((H, W), np.int32)
    m[:, :3] = 0
    m[H // 2, W // 2] = 0
    return m


def _one_bin(H, W):
    return np.zeros((H, W), np.int32)


def _one_coefficient(H, W):
    m = np.full((H, W), -1, np.int32)
    m[2, 3] = m[-2, -3] = 0                         # one half-plane coefficient and its mirror image
    return m


def _directional(H, W):
    """bin 0: kx = 0 column, bin 1: ky = 0 row without the origin, bin 2: the rest of |kx| <= 2, everything else dropped"""
    kx = np.minimum(np.arange(W), W - np.arange(W))[None, :] + np.zeros((H, 1), np.int64)
    ky = np.minimum(np.arange(H), H - np.arange(H))[:, None] + np.zeros((1, W), np.int64)
    m = np.full((H, W), -1, np.int32)
    m[kx <= 2] = 2
    m[ky == 0] = 1
    m[kx == 0] = 0
    return m


CHUNK_FIELDS = WS_BUDGET // bytes_per_field(64, 64) + 7   # more 64 x 64 fields than one workspace chunk holds

CASES = {
    'shape1x1': _case(1, (2, 1, 1, 1), detrend=None),
    'shape1x8': _case(2, (2, 1, 8, 1)),
    'shape8x1': _case(3, (2, 8, 1, 1)),
    'shape5x8': _case(4, (2, 5, 8, 1)),
    'shape8x5': _case(5, (2, 8, 5, 1)),
    'shape17x33': _case(6, (2, 17, 33, 1)),
    'shape64x64': _case(7, (2, 64, 64, 1)),
    'shape96x130': _case(8, (1, 96, 130, 1)),
    'shape255x256': _case(9, (1, 255, 256, 1)),
    'channels17x33': _case(10, (3, 17, 33, 2)),
    'precip17x33': _case(11, (2, 17, 33, 1), 'precip'),
    'offset280': _case(12, (2, 17, 33, 1), 'offset'),
    'offset280_hann': _case(13, (1, 64, 64, 1), 'offset', window='hann'),
    'nonfinite': _case(14, (3, 17, 33, 2), edit=_nonfinite),
    'nonfinite_hann': _case(15, (2, 8, 5, 1), 'precip', window='hann', edit=_nonfinite),
    'mask2d': _case(16, (2, 17, 33, 2), mask=_mask2d),
    'one_field_masked': _case(17, (3, 8, 5, 1), edit=_one_field_masked, empty=1),
    'hann17x33': _case(18, (2, 17, 33, 1), window='hann'),
    'no_detrend': _case(19, (2, 17, 33, 1), 'precip', detrend=None),
    'no_detrend_offset_hann': _case(20, (1, 5, 8, 1), 'offset', detrend=None, window='hann'),
    'map_one_bin': _case(21, (2, 17, 33, 1), bins=_one_bin),
    'map_one_coefficient': _case(22, (2, 17, 33, 1), bins=_one_coefficient),
    'map_directional': _case(23, (1, 96, 130, 1), 'precip', bins=_directional),
    'workspace_chunks': _case(24, (CHUNK_FIELDS, 64, 64, 1)),
}
