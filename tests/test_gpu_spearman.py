"""Spearman rank correlation on the device (dl4ds_spearman, csrc/rank.hip) and the metrics built on it -- compute_correlation,
compute_rmse, compute_metrics' Spearman entries -- against the fp64 restatement tests/spearman_ref.py (itself checked against
scipy.stats.spearmanr in tests/test_metrics_api.py).  Ranks are exact and the sums fp64, so rho is compared at 1e-9 absolute."""
import os

import numpy as np
import pytest

from tests.spearman_ref import spearman_space, spearman_time

pytestmark = pytest.mark.gpu

ATOL = 1e-9
LDS_MAX = 4096            # rank.hip RK_LDS_MAX: longest sequence the one-workgroup LDS engine sorts
TILE = 4096               # sort_keys.h SORT_TILE: elements per tile of the global radix engine


def precip(rng, shape):
    """precipitation-like fields: about 60 % exact zeros, values rounded to 0.1 (heavy ties)"""
    v = np.round(rng.gamma(0.6, 3.0, shape), 1) * (rng.random(shape) > 0.6)
    return v.astype(np.float32)


def pair(rng, shape, kind):
    if kind == 'normal':
        y = rng.standard_normal(shape).astype(np.float32)
        return y, (y + 0.7 * rng.standard_normal(shape)).astype(np.float32)
    if kind == 'ties':
        y = precip(rng, shape)
        return y, np.round(y * rng.uniform(0.5, 1.5, shape) + precip(rng, shape) * 0.3, 1).astype(np.float32)
    if kind == 'signed_zero':         # the reference's mask multiplies negative fields by 0 (metrics.py:156-162): -0.0
        f = rng.standard_normal(shape).astype(np.float32)
        g = (f + 0.5 * rng.standard_normal(shape)).astype(np.float32)
        y = f * (f > 0).astype(np.float32)                  # -0.0 where f < 0
        p = np.round(g, 1) * (g > 0).astype(np.float32)
        y[:, :, ::2] = np.abs(y[:, :, ::2])                 # and +0.0 on every other column
        assert np.signbit(y[y == 0]).any() and not np.signbit(y[y == 0]).all()
        return y.astype(np.float32), p.astype(np.float32)
    raise ValueError(kind)


def check(got, want):
    got = np.asarray(got, np.float64)
    assert got.shape == want.shape
    np.testing.assert_array_equal(np.isnan(got), np.isnan(want))
    np.testing.assert_allclose(got, want, rtol=0, atol=ATOL, equal_nan=True)


@pytest.mark.parametrize('shape,kind', [((3, 512, 512, 1), 'ties'), ((3, 512, 512, 1), 'signed_zero'), ((4, 96, 104, 2), 'normal'),
                                        ((4, 96, 104, 2), 'ties'), ((5, 9, 8, 1), 'normal'), ((5, 9, 8, 1), 'signed_zero'),
                                        ((2, 1, 2 * TILE + 64, 1), 'ties')])
def test_per_pair(shape, kind):
    """the last shape: two full tiles of the radix sort with the index payload and a third of 64 elements, one chunk of one wave
    (the tile's three other waves hold no valid lane)"""
    from dl4ds_amd.metrics import spearman
    y, p = pair(np.random.default_rng(sum(shape)), shape, kind)
    got = spearman(y, p, over='space')
    assert got.dtype == np.float64
    check(got, spearman_space(y, p))
    assert not np.isnan(got).any()


@pytest.mark.parametrize('hwc', [(64, 64, 1), (65, 63, 1), (17, 241, 1), (2, 32, 64)], ids=['L4096', 'L4095', 'L4097', 'L4096c2'])
def test_per_pair_around_the_lds_threshold(hwc):
    """sequence lengths at, one below and one above the longest the LDS engine takes (one above: the global radix engine, a
    second tile holding one element)"""
    from dl4ds_amd.metrics import spearman
    L = int(np.prod(hwc))
    assert abs(L - LDS_MAX) <= 1
    r = np.random.default_rng(L)
    y, p = pair(r, (3,) + hwc, 'ties')
    y2, p2 = pair(r, (3,) + hwc, 'normal')
    y, p = np.concatenate([y, y2]), np.concatenate([p, p2])
    check(spearman(y, p, over='space'), spearman_space(y, p))


def test_constant_and_nan_pairs_only_spoil_themselves():
    from dl4ds_amd.metrics import spearman
    for shape in [(6, 9, 8, 1), (6, 96, 104, 2)]:            # the LDS engine and the global engine
        y, p = pair(np.random.default_rng(11), shape, 'ties')
        y[1] = 0.5                                          # constant ground truth
        p[3] = -0.0                                         # constant prediction (all zeros of both signs)
        p[3, 0, 0, 0] = 0.0
        p[4, 3, 2, 0] = np.nan
        y[5, -1, -1, -1] = np.nan
        want = spearman_space(y, p)
        got = spearman(y, p, over='space')
        assert np.isnan(got[[1, 3, 4, 5]]).all() and not np.isnan(got[[0, 2]]).any()
        check(got, want)


def test_several_workspace_chunks():
    """1600 pairs of 4097 values: the global engine's 128 MiB workspace budget holds 1565 such pairs (5 x 16 640 B of per-element
    buffers + 2 KiB of histograms + the per-tile NaN flags and partial sums, 256-B aligned), so this call takes two chunks"""
    from dl4ds_amd.metrics import spearman
    y, p = pair(np.random.default_rng(5), (1600, 17, 241, 1), 'ties')
    y[1599] = 3.0
    p[1570, 0, 5, 0] = np.nan
    check(spearman(y, p, over='space'), spearman_space(y, p))


@pytest.mark.parametrize('n', [2, 37, 365, LDS_MAX + 904])
def test_per_grid_point(n):
    """over the N pairs per grid point of channel 0 (elements strided by H*W*C): the LDS engine for N = 2 ... 365, the global
    engine above its threshold on a small grid"""
    from dl4ds_amd.metrics import spearman
    h, w = (24, 20) if n <= 365 else (3, 5)
    r = np.random.default_rng(n)
    y, p = pair(r, (n, h, w, 2), 'ties')
    ys, ps = pair(r, (n, h, w, 2), 'signed_zero')
    y[:, :, : w // 2], p[:, :, : w // 2] = ys[:, :, : w // 2], ps[:, :, : w // 2]
    y[:, 0, 0, 0] = 1.5                                     # a constant grid point
    p[n // 2, 1, 1, 0] = np.nan
    p[:, 2, 2, 1] = np.nan                                  # channel 1 is not read
    got = spearman(y, p, over='time')
    assert got.shape == (h, w) and got.dtype == np.float64
    check(got, spearman_time(y, p))
    assert np.isnan(got[0, 0]) and np.isnan(got[1, 1]) and not np.isnan(got[2, 2])


def test_bitwise_reproducible():
    from dl4ds_amd.metrics import spearman
    for shape, over in [((4, 96, 104, 2), 'space'), ((5, 9, 8, 1), 'space'), ((365, 24, 20, 1), 'time'), ((5000, 3, 5, 1), 'time')]:
        y, p = pair(np.random.default_rng(1), shape, 'ties')
        a, b = spearman(y, p, over=over), spearman(y, p, over=over)
        assert a.tobytes() == b.tobytes(), (shape, over)


def _masked_pair(dtype=np.float32):
    r = np.random.default_rng(21)
    y, p = pair(r, (40, 12, 10, 2), 'normal')
    y[0, 3, 4, 0] = 0.0                                     # the reference only visits np.where(y[0, :, :, 0])
    y[0, 7, 1, 0] = -0.0
    y[0, 5, 5, 1] = 0.0                                     # channel 1: no effect
    return y.astype(dtype), p.astype(dtype)


def _nan_where_y0_zero(y, m):
    m = m.copy()
    m[y[0, :, :, 0] == 0] = np.nan
    return m


def test_compute_correlation():
    import dl4ds_amd as dds
    y, p = _masked_pair(np.float64)                          # float64 holding float32 values: the maps come back as float64
    got = dds.compute_correlation(y, p)                      # defaults: over='time', mode='spearman'
    assert isinstance(got, np.ndarray) and got.dtype == np.float64 and got.shape == (12, 10)
    want = _nan_where_y0_zero(y, spearman_time(y, p))
    assert np.isnan(want[3, 4]) and np.isnan(want[7, 1]) and not np.isnan(want[5, 5])
    check(got, want)
    sp = dds.compute_correlation(y, p, over='space', n_jobs=3)
    assert isinstance(sp, list) and len(sp) == 40
    check(np.array(sp), spearman_space(y, p))
    f32 = dds.compute_correlation(y.astype(np.float32), p.astype(np.float32))
    assert f32.dtype == np.float32
    np.testing.assert_allclose(f32, want.astype(np.float32), rtol=0, atol=1e-7)

    from dl4ds_amd.metrics import image_metrics
    m = image_metrics(y, p)
    pe = dds.compute_correlation(y, p, mode='pearson')
    np.testing.assert_array_equal(pe, _nan_where_y0_zero(y, m['pearson_map'][..., 0].astype(np.float64)))
    ps = dds.compute_correlation(y, p, over='space', mode='pearson')
    assert isinstance(ps, list) and np.array_equal(np.array(ps), m['pearson'])
    d = lambda a: a - a.mean(0)
    num = (d(y) * d(p)).sum(0)[..., 0] / np.sqrt((d(y) ** 2).sum(0) * (d(p) ** 2).sum(0))[..., 0]
    np.testing.assert_allclose(pe, _nan_where_y0_zero(y, num), rtol=0, atol=2e-5)
    with pytest.raises(ValueError):
        dds.compute_correlation(y, p, mode='kendall')


def test_compute_rmse():
    import dl4ds_amd as dds
    y, p = _masked_pair(np.float64)
    mse = ((p - y) ** 2).mean(0)[..., 0]
    got = dds.compute_rmse(y, p)                             # over='time': the MSE map (the reference ignores squared there)
    assert got.dtype == np.float64 and got.shape == (12, 10)
    np.testing.assert_allclose(got, _nan_where_y0_zero(y, mse), rtol=1e-5, atol=0)
    np.testing.assert_array_equal(dds.compute_rmse(y, p, squared=True), got)
    per = ((p - y) ** 2).reshape(40, -1).mean(1)
    r = dds.compute_rmse(y, p, over='space')
    assert isinstance(r, list) and len(r) == 40
    np.testing.assert_allclose(r, np.sqrt(per), rtol=1e-5)
    np.testing.assert_allclose(dds.compute_rmse(y, p, over='space', squared=True), per, rtol=1e-5)


def test_compute_metrics_spearman_entries(tmp_path):
    from dl4ds_amd.metrics import compute_metrics, image_metrics
    y, p = pair(np.random.default_rng(8), (6, 40, 36, 1), 'ties')
    rmse_map, corr_map, nmb, m = compute_metrics(y, p, save_path=str(tmp_path), verbose=False)
    keys = list(m['summary'])
    assert keys == ['PSNR', 'SSIM', 'MAE', 'Per-grid-point RMSE', 'Per-grid-point nRMSE', 'Per-grid-point Spearman correlation',
                    'Per-grid-point Pearson correlation', 'Spatial MSE', 'Spatial Spearman correlation',
                    'Spatial Pearson correlation']
    want = spearman_space(y, p)
    check(m['spearman'], want)
    for k in ('Per-grid-point Spearman correlation', 'Spatial Spearman correlation'):      # both the spatial values (metrics.py:316)
        assert abs(m['summary'][k][0] - want.mean()) <= ATOL and abs(m['summary'][k][1] - want.std()) <= ATOL
    np.testing.assert_array_equal(np.load(tmp_path / 'metrics_spearcorr_pergridpair.npy'), m['spearman'])
    np.testing.assert_array_equal(np.load(tmp_path / 'metrics_mse_pergridpair.npy'), m['rmse'])
    np.testing.assert_array_equal(np.load(tmp_path / 'metrics_pearcorr_pergridpair.npy'), m['pearson'])
    text = open(tmp_path / 'metrics_summary.txt').read()
    assert 'Per-grid-point Spearman correlation \tmu = ' in text and 'Spatial Spearman correlation \tmu = ' in text

    ref = image_metrics(y, p)                                # what existed before is unchanged
    for k, v in ref.items():
        np.testing.assert_array_equal(m[k], v, err_msg=k)
    np.testing.assert_array_equal(rmse_map, ref['rmse_map'].astype(np.float64))
    np.testing.assert_array_equal(corr_map, ref['pearson_map'].astype(np.float64))
    np.testing.assert_array_equal(nmb, ref['bias_map'].astype(np.float64) / (np.mean(y) * 100))
    s = m['summary']
    assert s['PSNR'] == (np.mean(ref['psnr']), np.std(ref['psnr'])) and s['Spatial MSE'] == (np.mean(ref['rmse']), np.std(ref['rmse']))
    g = ref['rmse_map'].astype(np.float64)
    assert s['Per-grid-point RMSE'] == (np.nanmean(g), np.nanstd(g))
