"""Seeded cases shared by tests/test_weighted_loss_api.py (CPU) and tests/test_gpu_weighted_loss.py.  Not a test module."""
import zlib

import numpy as np

# (B, H, W, C); (2,40,40,1): more than one block of the grid-stride loop and n not a multiple of 256 * 8
PIXEL_SHAPES = [(2, 5, 7, 1), (3, 16, 16, 2), (2, 40, 40, 1), (4, 9, 11, 3)]
# 'nmul2': a spatio-temporal output of two frames per sample -- the batch is (2 B, H, W, C) and sample row r uses map r // 2
PIXEL_FORMS = ['hw', 'hwc', 'per_sample', 'nmul2']
# (2,11,11,1): one window; (1,27,30,2): Ho x Wo = 17 x 20 crosses the 16-pixel tile in both axes
DSSIM_SHAPES = [(2, 11, 11, 1), (1, 27, 30, 2), (2, 33, 20, 1)]
# 'left_zero': columns 0..14 are zero, so windows with ox <= 4 have omega == 0 and are excluded
DSSIM_FORMS = ['random', 'left_zero', 'per_sample']
# 'fixups': min(p) < 0 (min-shift route), max(p) > max(t) and min(p) < min(t) (both drange routes of the finishing kernel)
DSSIM_DATA = ['positive', 'fixups']
MIN_RESIDUAL = 1e-3


def _rng(*key):
    return np.random.default_rng(zlib.crc32(repr(key).encode()))


def random_weights(rng, shape):
    """Uniform in [0, 2) with about 30 % exact zeros."""
    w = rng.uniform(0.0, 2.0, shape)
    w[rng.random(shape) < 0.3] = 0.0
    return w.astype(np.float32)


def pixel_case(shape, form):
    """-> (y_true, y_pred, weights): normal inputs with no |p - t| below MIN_RESIDUAL (the MAE sign is never in question)."""
    rng = _rng('pixel', shape, form)
    b, h, w, c = shape
    n = 2 * b if form == 'nmul2' else b
    t = rng.standard_normal((n, h, w, c)).astype(np.float32)
    d = rng.standard_normal((n, h, w, c))
    d[np.abs(d) < 0.01] = 0.5
    p = (t + d).astype(np.float32)
    assert (np.abs(p - t) >= MIN_RESIDUAL).all()
    wshape = {'hw': (h, w), 'hwc': (h, w, c), 'per_sample': (n, h, w, 1), 'nmul2': (b, h, w, c)}[form]
    wt = random_weights(rng, wshape)
    assert (wt == 0).any() and (wt > 0).any()
    return t, p, wt


def with_masked_truth(y_true, weights, fill):
    """y_true with `fill` (NaN, +Inf) wherever the broadcast weight is zero."""
    n, h, w, c = y_true.shape
    wt = np.asarray(weights)
    if wt.ndim == 2:
        wt = wt[None, :, :, None]
    elif wt.ndim == 3:
        wt = wt[None]
    full = np.broadcast_to(np.repeat(wt, n // wt.shape[0], axis=0), y_true.shape)
    out = y_true.copy()
    out[full == 0] = fill
    return out, full == 0


def dssim_case(shape, form, data):
    rng = _rng('dssim', shape, form, data)
    n, h, w, c = shape
    t = rng.random(shape).astype(np.float32)
    p = (t + 0.1 * rng.standard_normal(shape)).astype(np.float32)
    if data == 'positive':
        p = np.abs(p) + 0.01
    else:
        p[n - 1, h // 2, w // 3, 0] = 3.0
        p[0, h // 3, w // 2, c - 1] = -1.0
        assert p.min() < 0 and p.max() > t.max() and p.min() < t.min()
    d = p - t
    p = np.where(np.abs(d) < MIN_RESIDUAL, t + 0.05, p).astype(np.float32)      # the mixes hold an MAE term
    if form == 'per_sample':
        wt = random_weights(rng, (n, h, w, 1))
    else:
        wt = random_weights(rng, (h, w))
        if form == 'left_zero':
            wt = rng.uniform(0.5, 2.0, (h, w)).astype(np.float32)
            wt[:, :15] = 0.0
    return t, p, wt
