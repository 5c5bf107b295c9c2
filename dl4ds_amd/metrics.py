"""compute_metrics, compute_rmse and compute_correlation of dl4ds/metrics.py:15-330 without the plotting: the per-pair and
per-grid-point test metrics are reduced on the device (`dl4ds_metrics`), Spearman rank correlations are computed by the
segmented rank engine (`dl4ds_spearman`, csrc/rank.hip), the summary statistics the reference prints are assembled here.
`neighbourhood_scores` / `fss` (no counterpart in the reference): Fractions Skill Score and contingency scores per threshold and
neighbourhood size from the exact integer sums of `dl4ds_fss` (csrc/fss.hip).
`distribution_scores` / `quantile_maps` (no counterpart either): sample quantiles, 1-Wasserstein distance, Kolmogorov-Smirnov
statistic, histograms and Perkins skill score per grid cell or per sample from `dl4ds_distribution` (csrc/distribution.hip).
`spectral_scores` / `power_spectrum` (no counterpart either): radially averaged power spectral density, spectral ratio, coherence,
log-spectral distance and effective resolution per field from the binned power and cross spectra of `dl4ds_spectrum`
(csrc/spectrum.hip)."""
import math

import numpy as np

from . import _exact, _lib
from ._chunks import check_batch_size, host_ensemble, paired_chunks
from .device import DeviceArray
from .dataloader import checkarray_ndim
from .ensemble_score import (ExceedanceScorer, MultivariateScorer, NeighbourhoodScorer, Scorer, check_exceedance_args,
                             check_multivariate_args, check_neighbourhood_ensemble_args, check_score_args)
from .graph import check_ensemble_args


def _upload(y_test, y_test_hat):
    """-> (y, p, dy, dp): both arrays as contiguous float32 (N, H, W, C) on the host and on the device."""
    y = np.ascontiguousarray(y_test, np.float32)
    p = np.ascontiguousarray(y_test_hat, np.float32)
    if y.shape != p.shape or y.ndim != 4:
        raise ValueError(f'expected two (N, H, W, C) arrays of one shape, got {y.shape} and {p.shape}')
    return y, p, DeviceArray.from_numpy(y), DeviceArray.from_numpy(p)


def _device_metrics(dy, dp, shape):
    n, h, w, c = shape
    pair, grid, rng = DeviceArray.zeros((n, 4)), DeviceArray.zeros((3, h, w, c)), DeviceArray.zeros((2,))
    _lib.check(_lib.lib().dl4ds_metrics(dy.ptr, dp.ptr, n, h, w, c, pair.ptr, grid.ptr, rng.ptr))
    pair, grid, rng = pair.numpy().astype(np.float64), grid.numpy(), rng.numpy().astype(np.float64)
    drange = float(rng[1] - rng[0])
    mse = pair[:, 1]
    with np.errstate(divide='ignore'):
        psnr = 20.0 * np.log10(drange) - 10.0 * np.log10(mse)          # tf.image.psnr(y, y_hat, max_val=drange)
    return dict(mae=pair[:, 0], mse=mse, rmse=np.sqrt(mse), psnr=psnr, ssim=pair[:, 3], pearson=pair[:, 2],
                rmse_map=grid[0], bias_map=grid[1], pearson_map=grid[2], drange=drange)


def _device_spearman(dy, dp, shape, over):
    """Spearman rho in fp64 per test pair over all H*W*C values (``over='space'``, shape (N,)) or per grid point of channel 0
    over the N pairs (``over='time'``, shape (H, W))."""
    n, h, w, c = shape
    _check_over(over)
    if over == 'space':
        segs, length, seg_stride, elem_stride, out_shape = n, h * w * c, h * w * c, 1, (n,)
    else:
        segs, length, seg_stride, elem_stride, out_shape = h * w, n, c, h * w * c, (h, w)
    out = DeviceArray(out_shape, np.float64)
    _lib.check(_lib.lib().dl4ds_spearman(dy.ptr, dp.ptr, segs, length, seg_stride, elem_stride, out.ptr))
    return out.numpy()


def image_metrics(y_test, y_test_hat):
    """Raw device reductions -> dict of arrays: per pair ``mae``, ``mse``, ``rmse``, ``psnr``, ``ssim``, ``pearson``; per grid
    point ``rmse_map``, ``bias_map``, ``pearson_map``; ``drange``.  ``pearson`` of a pair one side of which is constant is 0.0
    (scipy.stats.pearsonr: NaN); ``pearson_map`` is NaN where either side of a grid point is constant over the pairs, hence
    everywhere for a single pair; ``ssim`` is NaN on grids below the 11x11 window.  The per-pair moments are taken about the pair's
    first elements, so data with a large mean (Kelvin, Pascal) keeps its correlation."""
    y, _, dy, dp = _upload(y_test, y_test_hat)
    return _device_metrics(dy, dp, y.shape)


def spearman(y, p, over='space'):
    """scipy.stats.spearmanr(...)[0] of every test pair over all its H*W*C values (``over='space'``: float64 (N,)) or of every
    grid point of channel 0 over the N pairs (``over='time'``: float64 (H, W)), on the device.  Ties get average ranks, -0.0
    ties with +0.0; a NaN, a constant side or fewer than two values give NaN.  Inputs are (N, H, W, C), read as float32."""
    y, _, dy, dp = _upload(y, p)
    return _device_spearman(dy, dp, y.shape, over)


def _map_dtype(y):
    return y.dtype if np.issubdtype(y.dtype, np.floating) else np.dtype(np.float64)


def _channel0_map(y, values):
    """The reference's per-grid-point maps (metrics.py:35-45, 75-85): start from NaN and fill only the grid points where
    ``y[0, :, :, 0]`` is non-zero, in the dtype of ``y``."""
    out = np.full(y.shape[1:3], np.nan, dtype=_map_dtype(y))
    sel = y[0, :, :, 0] != 0
    out[sel] = values[sel]
    return out


def _check_over(over):
    if over not in ('time', 'space'):
        raise ValueError(f"over must be 'time' or 'space', got {over!r}")


def compute_rmse(y, y_hat, over='time', squared=False, n_jobs=40):
    """metrics.py:15-48 on the device (``n_jobs`` is accepted and ignored).  ``over='time'``: the per-grid-point MSE map of
    channel 0, NaN where ``y[0, :, :, 0] == 0`` -- the reference's per-pixel helper calls mean_squared_error without
    ``squared``, so this map is always the MSE.  ``over='space'``: a list of per-pair RMSE values (MSE if ``squared``)."""
    _check_over(over)
    y, y_hat = np.asarray(y), np.asarray(y_hat)
    _, _, dy, dp = _upload(y, y_hat)
    m = _device_metrics(dy, dp, y.shape)
    if over == 'time':
        return _channel0_map(y, m['rmse_map'][..., 0].astype(np.float64) ** 2)
    return list(m['mse'] if squared else m['rmse'])


def compute_correlation(y, y_hat, over='time', mode='spearman', n_jobs=40):
    """metrics.py:51-97 on the device (``n_jobs`` is accepted and ignored).  ``over='time'``: the (H, W) map of channel 0 of
    per-grid-point correlations over the pairs, NaN where ``y[0, :, :, 0] == 0``; ``over='space'``: a list with one
    correlation per test pair over all its H*W*C values.  ``mode``: 'spearman' (scipy.stats.spearmanr) or 'pearson'
    (scipy.stats.pearsonr)."""
    if mode not in ('spearman', 'pearson'):
        raise ValueError(f"mode must be 'spearman' or 'pearson', got {mode!r}")
    _check_over(over)
    y, y_hat = np.asarray(y), np.asarray(y_hat)
    _, _, dy, dp = _upload(y, y_hat)
    if mode == 'spearman':
        vals = _device_spearman(dy, dp, y.shape, over)
    else:
        m = _device_metrics(dy, dp, y.shape)
        vals = m['pearson'] if over == 'space' else m['pearson_map'][..., 0].astype(np.float64)
    return list(vals) if over == 'space' else _channel0_map(y, vals)


def compute_metrics(y_test, y_test_hat, dpi=150, plot_size_px=1000, n_jobs=-1, scaler=None, mask=None, save_path=None,
                    verbose=True):
    """Same preparation as the reference (squeeze 5-D, optional ``scaler.inverse_transform``, optional validity mask) and the
    same printed summary; returns ``(temp_rmse_map, temp_pearson_corrmap, nmeanbias)`` like metrics.py:326, plus the full
    dictionary of per-pair / per-grid-point arrays as a fourth element (``spearman``: the per-pair Spearman correlations).
    The arrays go to the device once; the reductions and the Spearman ranks share them.  With ``save_path`` the per-pair
    RMSE, Spearman and Pearson values are also saved as metrics_{mse,spearcorr,pearcorr}_pergridpair.npy (metrics.py:188-250).
    As in the reference (metrics.py:316), the 'Per-grid-point Spearman correlation' line reports the SPATIAL (per-pair)
    Spearman values, the same numbers as 'Spatial Spearman correlation'."""
    y_test, y_test_hat = np.asarray(y_test), np.asarray(y_test_hat)
    if y_test.ndim == 5:
        y_test, y_test_hat = np.squeeze(y_test, -1), np.squeeze(y_test_hat, -1)
    y_test, y_test_hat = checkarray_ndim(y_test, 4, -1), checkarray_ndim(y_test_hat, 4, -1)
    if scaler is not None and hasattr(scaler, 'inverse_transform'):
        y_test, y_test_hat = scaler.inverse_transform(y_test), scaler.inverse_transform(y_test_hat)
    mask_nan = None
    if mask is not None:
        mask = np.asarray(getattr(mask, 'values', mask)).copy()
        if mask.ndim == 2:
            mask = mask[..., None]
        y_test, y_test_hat = y_test * mask, y_test_hat * mask
        mask_nan = np.where(mask == 0, np.nan, 1.0)
    y32, _, dy, dp = _upload(y_test, y_test_hat)
    m = _device_metrics(dy, dp, y32.shape)
    m['spearman'] = _device_spearman(dy, dp, y32.shape, 'space')
    del dy, dp
    rmse_map, corr_map = m['rmse_map'].astype(np.float64), m['pearson_map'].astype(np.float64)
    nmeanbias = m['bias_map'].astype(np.float64) / (np.mean(y_test) * 100)            # metrics.py:219-220
    norm_rmse_map = rmse_map / (np.mean(y_test) * 100)
    if mask_nan is not None:
        rmse_map, corr_map, nmeanbias, norm_rmse_map = (a * mask_nan for a in (rmse_map, corr_map, nmeanbias, norm_rmse_map))
    spear = (np.mean(m['spearman']), np.std(m['spearman']))
    summary = {
        'PSNR': (np.mean(m['psnr']), np.std(m['psnr'])), 'SSIM': (np.mean(m['ssim']), np.std(m['ssim'])),
        'MAE': (np.mean(m['mae']), np.std(m['mae'])),
        'Per-grid-point RMSE': (np.nanmean(rmse_map), np.nanstd(rmse_map)),
        'Per-grid-point nRMSE': (np.nanmean(norm_rmse_map), np.nanstd(norm_rmse_map)),
        'Per-grid-point Spearman correlation': spear,                                      # metrics.py:316: the spatial values
        'Per-grid-point Pearson correlation': (np.nanmean(corr_map), np.nanstd(corr_map)),
        'Spatial MSE': (np.mean(m['rmse']), np.std(m['rmse'])),
        'Spatial Spearman correlation': spear,
        'Spatial Pearson correlation': (np.mean(m['pearson']), np.std(m['pearson'])),
    }
    m['summary'] = summary
    if verbose or save_path is not None:
        lines = ['Metrics on y_test and y_test_hat:\n'] + [f'{k} \tmu = {a} \tsigma = {b}' for k, (a, b) in summary.items()]
        if save_path is not None:
            import os
            for name, key in (('mse', 'rmse'), ('spearcorr', 'spearman'), ('pearcorr', 'pearson')):
                np.save(os.path.join(save_path, f'metrics_{name}_pergridpair.npy'), m[key])
            with open(os.path.join(save_path, 'metrics_summary.txt'), 'a') as f:
                f.write('\n'.join(lines) + '\n')
        elif verbose:
            print('\n'.join(lines))
    if mask is not None:
        for a in (rmse_map, corr_map, nmeanbias):
            a[np.where(np.broadcast_to(mask, a.shape) == 0)] = 0
    return rmse_map, corr_map, nmeanbias, m


def _masked_observation(y, mask):
    """``y`` as float32 with NaN where ``mask`` (2-D, or with a channel axis; 0 = excluded) is 0, as ``compute_metrics`` reads it."""
    y = np.array(y, np.float32)                    # (a copy: the caller's array is not written)
    if mask is not None:
        mask = np.asarray(getattr(mask, 'values', mask))
        if mask.ndim == 2 and y.ndim >= 4:
            mask = mask[..., None]
        try:
            excluded = np.broadcast_to(mask == 0, y.shape)
        except ValueError:
            raise ValueError(f'`mask` of shape {mask.shape} does not broadcast to the observation {y.shape}') from None
        y[excluded] = np.nan
    return y


def _prepared(y_test, y_test_hat, scaler, mask, check):
    """Both arrays as `compute_metrics` prepares them -> (masked float32 observation, prediction, ``check(shape)``'s result)."""
    y_test, y_test_hat = np.asarray(getattr(y_test, 'values', y_test)), np.asarray(getattr(y_test_hat, 'values', y_test_hat))
    if y_test.ndim == 5:
        y_test, y_test_hat = np.squeeze(y_test, -1), np.squeeze(y_test_hat, -1)
    y_test, y_test_hat = checkarray_ndim(y_test, 4, -1), checkarray_ndim(y_test_hat, 4, -1)
    if y_test.shape != y_test_hat.shape or y_test.ndim != 4:
        raise ValueError(f'expected two (N, H, W, C) arrays of one shape, got {y_test.shape} and {y_test_hat.shape}')
    checked = check(y_test.shape)                  # every ValueError comes before inverse_transform and before any library call
    if scaler is not None and hasattr(scaler, 'inverse_transform'):
        y_test, y_test_hat = scaler.inverse_transform(y_test), scaler.inverse_transform(y_test_hat)
    return _masked_observation(y_test, mask), y_test_hat, checked


def _host_ensemble_args(y_true, members, quantiles, seed, batch_size):
    """What `ensemble_scores` and `exceedance_scores` check alike -> (members, K, quantiles as float32, y_true), all arrays."""
    members = np.asarray(members)
    if members.ndim < 2:
        raise ValueError(f'`members` must be shaped (K,) + y_true.shape, got {members.shape}')
    K, q = check_ensemble_args(int(members.shape[0]), quantiles, seed, batch_size)
    y_true = np.asarray(getattr(y_true, 'values', y_true))
    if y_true.ndim < 1 or members.shape[1:] != y_true.shape:
        raise ValueError(f'`members` must be shaped (K,) + y_true.shape = (K,) + {y_true.shape}, got {members.shape}')
    return members, K, q, y_true


def ensemble_scores(y_true, members, quantiles=(), fair=False, seed=0, mask=None, batch_size=None, scale=None,
                    return_fields=False):
    """Verification scores of an ensemble the caller already has on the host: ``members`` shaped (K,) + y_true.shape against the
    observation ``y_true`` (samples on the leading axis), uploaded in chunks of ``batch_size`` samples (default: chunks of at most
    256 MiB of members) and scored on the device by the entry ``Model.score_ensemble`` uses (csrc/ensemble_score.hip).  Returns the
    'scores' dict described there: CRPS (``fair``: the fair form), spread, RMSE of the ensemble mean and their ratio, per sample and
    per cell, the rank histogram with ties broken by a hash of (``seed``, element index), the coverage of ``quantiles``.  The result
    does not depend on ``batch_size``.  ``mask``: 2-D or with a channel axis, 0 = excluded (NaN is written into the observation;
    elements next to a non-finite value are excluded anyway).  The folds run one lane per cell and walk a chunk's samples in
    turn: made for fields; samples of very few cells (a 1-D ``y_true`` has one) are slow.  ``scale``: a positive factor per cell, see ``Model.score_ensemble``."""
    members, K, q, y_true = _host_ensemble_args(y_true, members, quantiles, seed, batch_size)
    N, sample_shape = y_true.shape[0], tuple(y_true.shape[1:])
    scale = check_score_args(fair, scale, sample_shape)
    return host_ensemble(_masked_observation(y_true, mask), members, batch_size=batch_size,
                         make_scorer=lambda bmax: Scorer(K, N, sample_shape, q, fair, seed, scale, return_fields, bmax))


def exceedance_scores(y_true, members, thresholds, mask=None, batch_size=None, return_fields=False):
    """Verification of an ensemble the caller already has on the host as a PROBABILITY forecast of the events ``value >=
    threshold``: ``members`` shaped (K,) + y_true.shape against the observation ``y_true`` (samples on the leading axis), uploaded
    in chunks of ``batch_size`` samples (default: chunks of at most 256 MiB of members) and counted on the device by the entry
    ``Model.score_exceedance`` uses (csrc/exceedance.hip).  ``thresholds``: up to 16 finite numbers, or one
    field per threshold shaped (T,) + y_true.shape[1:] (a local percentile; NaN excludes the cell for that threshold).  An element
    is valid iff its observation and all its members are finite and ``mask`` (2-D or with a channel axis, 0 = excluded) keeps it.
    With c of the K members at or above the threshold the forecast probability is c / K: the device returns exact int64 sums, so
    the result equals an integer reference and does not depend on ``batch_size``.  Returns a dict (T thresholds, N samples):

    * ``thresholds`` (float32, as used), ``n_members``, ``table`` (T, K + 1, 2) int64: valid elements with c = i and the event
      not observed / observed; ``n_valid``, ``n_events``, ``base_rate`` (T,);
    * ``brier`` (T,), ``brier_fair`` (Ferro's fair Brier score, NaN for K = 1), ``reliability``, ``resolution``, ``uncertainty``
      (brier = reliability - resolution + uncertainty holds exactly: the forecast takes only the K + 1 values i / K), ``bss`` =
      1 - brier / uncertainty;
    * ``forecast_probability`` (K + 1,), ``observed_frequency`` and ``forecast_count`` (T, K + 1): the reliability diagram and
      the sharpness histogram;
    * ``roc_pod``, ``roc_pofd`` (T, K + 2): point j warns iff c >= K + 1 - j, from (0, 0) to (1, 1); ``roc_auc`` (T,): the
      trapezoid area (Mann-Whitney with ties);
    * ``sample_sums`` (N, T, 4) and ``cell_sums`` (T, 4) + sample shape, int64: n_valid, sum o, sum c, sum (c - K o)^2;
      ``brier_per_sample``, ``n_valid_per_sample`` (N, T); ``brier_map``, ``base_rate_map``, ``forecast_rate_map``, ``bss_map``,
      ``n_valid_map`` (T,) + sample shape;
    * with ``return_fields``: ``count_field`` int16 (N, T) + sample shape (c, -1 where invalid) and ``probability_field``
      float32 (c / K, NaN where invalid).

    Every ratio is a quotient of integers rounded to float64 once (Python integers, or one IEEE division where both operands are
    below 2^53), NaN on a zero denominator."""
    members, K, _, y_true = _host_ensemble_args(y_true, members, (), None, batch_size)
    N, sample_shape = y_true.shape[0], tuple(y_true.shape[1:])
    thr = check_exceedance_args(thresholds, sample_shape)
    return host_ensemble(_masked_observation(y_true, mask), members, batch_size=batch_size,
                         make_scorer=lambda bmax: ExceedanceScorer(K, N, sample_shape, thr, return_fields, bmax))


def multivariate_scores(y_true, members, max_lag=4, order=0.5, lag_weights='inverse', fair=False, weights=None, mask=None,
                        batch_size=None):
    """Verification of an ensemble the caller already has on the host as a forecast of a FIELD: the energy score (Gneiting et al.
    2008, the multivariate CRPS) and the variogram score (Scheuerer & Hamill 2015, which sees the dependence between cells that
    the per-cell scores of ``ensemble_scores`` cannot).  ``members`` shaped (K,) + y_true.shape, 2 <= K <= 128, against the
    observation ``y_true`` shaped (N, H, W, C) or (N, T, H, W, C); uploaded in chunks of ``batch_size`` samples and reduced on the
    device by the entries ``Model.score_multivariate`` uses (csrc/ensemble_multi.hip).  An element is valid
    iff its observation and all its members are finite, ``mask`` (2-D or with a channel axis, 0 = excluded) keeps it and its
    weight is > 0.  ``weights``: finite numbers >= 0 that broadcast to one sample (``losses.latitude_weights``); they weight the
    squared differences of the energy score and only decide validity for the variogram score.  ``fair``: the pair term of the
    energy score over K (K - 1) instead of K^2.  ``max_lag`` (1 ... 8): pairs of cells of one H x W plane up to that distance;
    ``order``: 0.5, 1 or 2; ``lag_weights``: 'inverse' (1 / distance) or 'uniform'.  Returns a dict (N samples, L lags):

    * ``energy_score`` (mean over the samples with a valid element), ``energy_score_per_sample`` (N,), ``member_distance`` (N, K)
      = sqrt(D_k), ``pair_distance`` (N, K (K - 1) / 2) = sqrt(G_kj) over k < j;
    * ``variogram_score``, ``variogram_score_per_sample`` (N,): sum_l w_l sum (o - e)^2 / sum_l w_l n_pairs; ``lags`` (L, 2) as
      (dy, dx), ``lag_distance``, ``lag_weight`` (L,); ``variogram_obs``, ``variogram_ens``, ``variogram_error`` (L,): the mean
      of o, e and (o - e)^2 over all valid pairs of the lag; ``n_pairs`` (N, L);
    * ``n_valid_per_sample`` (N,), ``n_members``, ``order``, ``fair``, and the raw float64 sums ``dist_sums`` (N, K (K + 1) / 2)
      and ``variogram_sums`` (N, L, 3).

    The per-sample sums have the same bits for every ``batch_size``."""
    members, K, _, y_true = _host_ensemble_args(y_true, members, (), None, batch_size)
    N, sample_shape = y_true.shape[0], tuple(y_true.shape[1:])
    lag, code, w32 = check_multivariate_args(max_lag, order, lag_weights, fair, weights, sample_shape, K)
    return host_ensemble(_masked_observation(y_true, mask), members, batch_size=batch_size,
                         make_scorer=lambda bmax: MultivariateScorer(K, N, sample_shape, lag, order, code, lag_weights, fair, w32,
                                                                     bmax))


FSS_DEFAULT_WINDOWS = (1, 3, 5, 9, 17, 33, 65)
FSS_SUM_BOUND = 1 << 62                            # H*W*m^2 must stay below it: the 64-bit sums of dl4ds_fss are exact
FSS_CELL_BOUND = 1 << 31


def check_neighbourhood_args(shape, thresholds, windows, batch_size=None):
    """Validation of `neighbourhood_scores` (no library call) -> (thresholds as float32 (T,), windows as int32 (S,))."""
    if len(shape) != 4 or min(shape) < 1:
        raise ValueError(f'expected non-empty (N, H, W, C) arrays, got shape {tuple(shape)}')
    _, h, w, _ = (int(v) for v in shape)
    thr = _exact.finite_float32(np.atleast_1d(np.asarray(thresholds, np.float64)), '`thresholds`', increasing=True)
    win = np.atleast_1d(np.asarray(windows))
    if win.ndim != 1 or win.size == 0:
        raise ValueError('`windows` must be a non-empty 1-D sequence')
    if win.dtype == bool or not np.issubdtype(win.dtype, np.integer):
        raise ValueError('`windows` must be integers')
    wl = [int(v) for v in win]
    if min(wl) < 1 or max(wl) >= 1 << 31:
        raise ValueError('`windows` must be positive (and below 2^31)')
    if any(b <= a for a, b in zip(wl, wl[1:])):
        raise ValueError('`windows` must be strictly increasing')
    if h * w >= FSS_CELL_BOUND:
        raise ValueError(f'fields of H*W = {h * w} cells are not supported: H*W must stay below 2^31')
    for n in wl:
        m = min(n, h) * min(n, w)
        if h * w * m * m >= FSS_SUM_BOUND:
            raise ValueError(f'window {n} on a {h} x {w} field: H*W*m^2 = {h * w * m * m} with m = min(n, H)*min(n, W) = {m} '
                             'must stay below 2^62 for the exact 64-bit sums')
    check_batch_size(batch_size)
    return thr, np.asarray(wl, np.int32)


def _contingency_scores(hits, misses, fa, nvalid):
    """POD, FAR, CSI, ETS, frequency bias from integer counts (int64 arrays, or object arrays of Python integers)."""
    to = lambda a: np.asarray(a, np.float64)
    obs, fc = hits + misses, hits + fa
    hr = _exact.ratio(to(obs) * to(fc), nvalid)                              # hits expected by chance
    ets_den = to(hits + misses + fa) - hr
    with np.errstate(invalid='ignore'):
        ets = np.where(np.isnan(hr) | (ets_den == 0), np.nan, (to(hits) - hr) / np.where(ets_den == 0, 1.0, ets_den))
    ratio = _exact.ratio
    return dict(pod=ratio(hits, obs), far=ratio(fa, fc), csi=ratio(hits, hits + misses + fa), ets=ets, bias=ratio(fc, obs))


def neighbourhood_scores(y_test, y_test_hat, thresholds, windows=FSS_DEFAULT_WINDOWS, scaler=None, mask=None, batch_size=None):
    """Scale- and threshold-dependent verification of (N, H, W, C) predictions on the device (csrc/fss.hip): the Fractions Skill
    Score (Roberts & Lean 2008) per field, exceedance threshold and neighbourhood size, and the categorical contingency scores at
    the same thresholds.  Every one of the N*C planes is one field.  Inputs are prepared as in `compute_metrics` (5-D squeezed,
    optional ``scaler.inverse_transform``) and read as float32; ``thresholds`` are cast to float32.  A cell is valid when both
    arrays are finite there and ``mask`` (2-D or with a channel axis, 0 = excluded) keeps it; an event is ``value >= threshold``
    on a valid cell.  The window of size n at (i, j) is rows [i - n//2, i - n//2 + n), columns likewise, clipped to the field
    (``scipy.ndimage.uniform_filter(mode='constant')`` times n^2, even n included).  The device returns exact int64 sums, so the
    result equals an integer reference and does not depend on ``batch_size`` (samples per upload; default: chunks of at most 256 MiB
    per array).  Returns a dict:

    * ``sums`` (N, C, T, S, 3) int64: D = sum (cf - co)^2, F = sum cf^2, O = sum co^2 of the window counts over all cells;
      ``fss`` (N, C, T, S) = 1 - D / (F + O) (NaN when F + O = 0), ``fss_pooled`` (T, S) and ``fss_pooled_per_channel``
      (C, T, S) = 1 - sum D / sum (F + O) over the fields;
    * ``hits``, ``misses``, ``false_alarms``, ``correct_negatives`` (N, C, T) int64 and ``n_valid`` (N, C);
    * ``pod``, ``far``, ``csi``, ``ets``, ``bias`` (N, C, T) and pooled over all fields as ``pod_pooled`` ... (T,), NaN on a zero
      denominator;
    * ``base_rate`` = ``fss_random`` (T,): the pooled observed event frequency, ``fss_useful`` = 0.5 + base_rate / 2 and
      ``useful_window`` (T,): the smallest requested window whose pooled FSS reaches it, or -1;
    * ``thresholds`` (float32) and ``windows`` as used."""
    obs, y_test_hat, (thr, win) = _prepared(y_test, y_test_hat, scaler, mask,
                                            lambda shape: check_neighbourhood_args(shape, thresholds, windows, batch_size))
    N, H, W, C = obs.shape
    T, S = len(thr), len(win)
    sums = np.empty((N, C, T, S, 3), np.int64)
    cont = np.empty((N, C, T, 4), np.int64)
    nvalid = np.empty((N, C), np.int64)
    lib = _lib.lib()

    def call(b, dy, dp, dsums, dcont, dvalid):
        _lib.check(lib.dl4ds_fss(dy, dp, b, H, W, C, thr.ctypes.data, T, win.ctypes.data, S, dsums, dcont, dvalid))
    paired_chunks(obs, y_test_hat, (sums, cont, nvalid), call, batch_size)
    return scores_from_counts(sums, cont, nvalid, thr, win)


def scores_from_counts(sums, cont, nvalid, thresholds, windows):
    """The result dict of `neighbourhood_scores` from the integer outputs of `dl4ds_fss` (host arithmetic only)."""
    sums, cont, nvalid = np.asarray(sums, np.int64), np.asarray(cont, np.int64), np.asarray(nvalid, np.int64)
    D, FO = sums[..., 0], sums[..., 1] + sums[..., 2]                  # F + O < 2^63 by the overflow rule
    res = dict(sums=sums, fss=1.0 - _exact.ratio(D, FO), n_valid=nvalid, thresholds=np.asarray(thresholds, np.float32),
               windows=np.asarray(windows, np.int64))
    so = sums.astype(object)
    res['fss_pooled'] = 1.0 - _exact.ratio_exact(np.sum(so[..., 0], axis=(0, 1)), np.sum(so[..., 1] + so[..., 2], axis=(0, 1)))
    res['fss_pooled_per_channel'] = 1.0 - _exact.ratio_exact(np.sum(so[..., 0], axis=0), np.sum(so[..., 1] + so[..., 2], axis=0))
    hits, misses, fa, cn = (cont[..., k] for k in range(4))
    res.update(hits=hits, misses=misses, false_alarms=fa, correct_negatives=cn)
    res.update(_contingency_scores(hits, misses, fa, nvalid[..., None]))
    ph, pm, pf = (_exact.pysum(a, (0, 1)) for a in (hits, misses, fa))
    pn = int(_exact.pysum(nvalid, (0, 1)))
    for k, v in _contingency_scores(ph, pm, pf, np.full(ph.shape, pn, object)).items():
        res[k + '_pooled'] = v
    base = _exact.ratio_exact(ph + pm, np.full(ph.shape, pn, object))
    res.update(base_rate=base, fss_random=base.copy(), fss_useful=0.5 + base / 2.0)
    with np.errstate(invalid='ignore'):
        reach = res['fss_pooled'] >= res['fss_useful'][:, None]       # NaN compares false
    res['useful_window'] = np.where(reach.any(1), res['windows'][np.argmax(reach, 1)], -1).astype(np.int64)
    return res


def neighbourhood_ensemble_scores(y_true, members, thresholds, windows=FSS_DEFAULT_WINDOWS, mask=None, batch_size=None):
    """Scale- and threshold-dependent verification of an ensemble the caller already has on the host as a PROBABILITY forecast:
    ``members`` shaped (K,) + y_true.shape against the observation ``y_true`` (N, H, W, C), uploaded in chunks of ``batch_size``
    samples (default: chunks of at most 256 MiB of members) and reduced on the device by the entry ``Model.score_neighbourhood``
    uses (csrc/ensemble_fss.hip).  Every one of the N*C planes is one field.  ``thresholds``: up to 16
    finite, strictly increasing numbers (cast to float32); ``windows``: strictly increasing sizes >= 1.  A cell is valid iff its
    observation and all K members are finite and ``mask`` (2-D or with a channel axis, 0 = excluded) keeps it.  On a valid cell
    o = [y >= t] and c = #{k : x_k >= t}; co, cf are their sums over the window of `neighbourhood_scores`.  The neighbourhood
    ensemble probability (Schwartz et al. 2010) is cf / (K n^2): a sharp member that is displaced by less than the window still
    counts, which the per-cell scores of `exceedance_scores` punish twice.  The device returns exact int64 sums, so the result
    equals an integer reference and does not depend on ``batch_size``.  Returns a dict:

    * ``sums`` (N, C, T, S, 5) int64: D = sum (cf - K co)^2, F = sum cf^2, O = sum co^2 over all cells, Fv = sum cf^2 over the
      valid cells, X = sum cf over the cells with o = 1; ``events`` = sum o and ``member_events`` = sum c (N, C, T), ``n_valid``
      (N, C), all int64;
    * ``pfss`` (N, C, T, S) = 1 - D / (F + K^2 O): the FSS of the neighbourhood ensemble probability against the observed
      fraction co / n^2; ``pfss_pooled`` (T, S) = 1 - sum D / sum (F + K^2 O) over the fields;
    * ``nbs`` (N, C, T, S) and ``nbs_pooled`` (T, S): the neighbourhood Brier score, the mean over the valid cells of
      (cf / (K n^2) - o)^2 with the requested n (at n = 1 the Brier score of `exceedance_scores`); ``nbss_pooled`` (T, S) =
      1 - nbs / (f_o (1 - f_o));
    * ``base_rate`` = ``fss_random`` (T,): the pooled observed frequency f_o, ``forecast_rate`` (T,) = sum c / (K n_valid),
      ``fss_useful`` = 0.5 + base_rate / 2 and ``useful_window`` (T,): the smallest requested window whose pooled pFSS reaches
      it, or -1;
    * ``thresholds`` (float32), ``windows`` and ``n_members`` as used.  Every ratio is NaN on a zero denominator."""
    members, K, _, y_true = _host_ensemble_args(y_true, members, (), None, batch_size)
    if y_true.ndim != 4 or min(y_true.shape) < 1:
        raise ValueError(f'expected a non-empty (N, H, W, C) observation, got shape {y_true.shape}')
    N, sample_shape = y_true.shape[0], tuple(y_true.shape[1:])
    thr, win = check_neighbourhood_ensemble_args(sample_shape, K, thresholds, windows)
    return host_ensemble(_masked_observation(y_true, mask), members, batch_size=batch_size,
                         make_scorer=lambda bmax: NeighbourhoodScorer(K, N, sample_shape, thr, win, bmax))


def fss(y, y_hat, thresholds, windows=FSS_DEFAULT_WINDOWS, scaler=None, mask=None, batch_size=None):
    """``(fss, fss_pooled)`` of `neighbourhood_scores`: the Fractions Skill Score per field (N, C, T, S) and pooled (T, S)."""
    r = neighbourhood_scores(y, y_hat, thresholds, windows, scaler=scaler, mask=mask, batch_size=batch_size)
    return r['fss'], r['fss_pooled']


DIST_DEFAULT_QUANTILES = (0.01, 0.05, 0.25, 0.5, 0.75, 0.95, 0.99)
DIST_MAX_QUANTILES = 64                            # caps of dl4ds_distribution: q and the edges travel as kernel arguments
DIST_MAX_EDGES = 257
DIST_LENGTH_BOUND = 1 << 31


def check_distribution_args(shape, quantiles, bins=None, over='time', batch_size=None):
    """Validation of `distribution_scores` (no library call) -> (quantiles as float64 (Q,), bin edges as float32 (E,) or None)."""
    if len(shape) != 4 or min(shape) < 1:
        raise ValueError(f'expected non-empty (N, H, W, C) arrays, got shape {tuple(shape)}')
    _check_over(over)
    n, h, w, c = (int(v) for v in shape)
    length = n if over == 'time' else h * w * c
    if length >= DIST_LENGTH_BOUND:
        raise ValueError(f'segments of {length} elements are not supported: the length must stay below 2^31')
    q = np.asarray(quantiles, np.float64)
    if q.ndim == 0:
        q = q.reshape(1)
    if q.ndim != 1:
        raise ValueError('`quantiles` must be a 1-D sequence')
    if q.size > DIST_MAX_QUANTILES:
        raise ValueError(f'at most {DIST_MAX_QUANTILES} quantiles are supported, got {q.size}')
    if not ((q >= 0.0) & (q <= 1.0)).all():                            # NaN compares false
        raise ValueError('`quantiles` must lie in [0, 1]')
    edges = None
    if bins is not None:
        edges = _exact.finite_float32(bins, '`bins` (the bin edges)', least=2, increasing=True)
        if edges.size > DIST_MAX_EDGES:
            raise ValueError(f'at most {DIST_MAX_EDGES} bin edges are supported, got {edges.size}')
    check_batch_size(batch_size)
    return np.ascontiguousarray(q), edges


def distribution_from_counts(quant, w1, ks_count, hist, nvalid, quantiles, bins):
    """The result dict of `distribution_scores` from the outputs of `dl4ds_distribution` (host arithmetic only): ``quant``
    (..., 2, Q), ``w1``, ``ks_count``, ``nvalid`` (...), ``hist`` (..., 2, B) or None."""
    quant, nvalid = np.asarray(quant, np.float64), np.asarray(nvalid, np.int64)
    ks_count = np.asarray(ks_count, np.int64)
    res = dict(n_valid=nvalid, q_obs=quant[..., 0, :], q_pred=quant[..., 1, :], q_bias=quant[..., 1, :] - quant[..., 0, :],
               wasserstein=np.asarray(w1, np.float64), ks_count=ks_count, ks=_exact.ratio(ks_count, nvalid),
               quantiles=np.asarray(quantiles, np.float64), bins=None)
    if hist is not None:
        hist = np.asarray(hist, np.int64)
        ho, hp = hist[..., 0, :], hist[..., 1, :]
        lead = tuple(range(nvalid.ndim))
        po, pp = np.atleast_1d(_exact.pysum(ho, lead)), np.atleast_1d(_exact.pysum(hp, lead))
        common = sum(min(int(a), int(b)) for a, b in zip(po, pp))
        total = sum(int(v) for v in nvalid.ravel())
        res.update(hist_obs=ho, hist_pred=hp, perkins=_exact.ratio(np.minimum(ho, hp).sum(-1), nvalid),
                   hist_obs_pooled=po.astype(np.int64), hist_pred_pooled=pp.astype(np.int64),
                   perkins_pooled=_exact.ratio_exact(common, total)[()], bins=np.asarray(bins, np.float32))
    return res


def distribution_scores(y_test, y_test_hat, quantiles=DIST_DEFAULT_QUANTILES, bins=None, over='time', scaler=None, mask=None,
                        batch_size=None):
    """Does the prediction have the observation's distribution?  Per segment, on the device (csrc/distribution.hip): the sample
    quantiles of both (N, H, W, C) arrays, their 1-Wasserstein distance, the two-sample Kolmogorov-Smirnov statistic and, with
    ``bins`` (bin edges, cast to float32), both histograms and the Perkins skill score.  ``over='time'``: one segment per grid cell
    and channel over the N samples, results shaped (H, W, C) + ...; ``over='space'``: one segment per sample over its H*W*C values,
    results shaped (N,) + ... (the convention of `spearman`).  Inputs are prepared as in `neighbourhood_scores` (5-D squeezed,
    optional ``scaler.inverse_transform``) and read as float32.  An element is valid when both arrays are finite there and
    ``mask`` (2-D or with a channel axis, 0 = excluded) keeps it; invalid elements leave both samples, so both have ``n_valid``
    values.  Quantiles are numpy's ``method='linear'`` in fp64; histogram bins are [e_b, e_b+1), the last one closed on the right
    (``np.histogram``), values outside the edges are counted nowhere.  The arrays are uploaded in chunks of at most 256 MiB each
    (``batch_size``: grid rows per upload for 'time', samples for 'space'); the result does not depend on it.  Returns a dict:

    * ``n_valid`` int64; ``q_obs``, ``q_pred``, ``q_bias`` = q_pred - q_obs (..., Q); ``wasserstein``;
    * ``ks_count`` int64 = n_valid times the KS statistic, ``ks`` = ks_count / n_valid;
    * with ``bins``: ``hist_obs``, ``hist_pred`` (..., B) int64, ``perkins`` = sum_b min(hist_obs, hist_pred) / n_valid, and
      pooled over all segments ``hist_obs_pooled``, ``hist_pred_pooled`` (B,), ``perkins_pooled``;
    * ``quantiles`` (float64) and ``bins`` (float32, or None) as used.  Every ratio is NaN where ``n_valid == 0``."""
    obs, y_test_hat, (q, edges) = _prepared(y_test, y_test_hat, scaler, mask,
                                            lambda shape: check_distribution_args(shape, quantiles, bins, over, batch_size))
    N, H, W, C = obs.shape
    Q, E = len(q), 0 if edges is None else len(edges)
    if over == 'time':
        lead, axis, segs = (H, W, C), 1, H * W * C                         # uploaded in bands of rows: W * C segments per row
    else:
        lead, axis, segs = (N,), 0, N                                      # uploaded in blocks of samples: one segment each
    quant = np.empty((segs, 2, Q), np.float64)
    w1 = np.empty((segs,), np.float64)
    ks, nvalid = np.empty((segs,), np.int64), np.empty((segs,), np.int64)
    hist = np.empty((segs, 2, E - 1), np.int64) if E else None
    lib = _lib.lib()

    def call(b, dy, dp, dquant, dw1, dks, dvalid, dhist=None):
        s = b * W * C if over == 'time' else b                             # segments of the chunk
        length, seg_stride, elem_stride = (N, 1, s) if over == 'time' else (H * W * C, H * W * C, 1)
        _lib.check(lib.dl4ds_distribution(dy, dp, s, length, seg_stride, elem_stride, q.ctypes.data, Q,
                                          edges.ctypes.data if E else None, E, dquant, dw1, dks, dhist, dvalid))
    paired_chunks(obs, y_test_hat, (quant, w1, ks, nvalid) + ((hist,) if E else ()), call, batch_size, axis)
    return distribution_from_counts(quant.reshape(lead + (2, Q)), w1.reshape(lead), ks.reshape(lead),
                                    None if hist is None else hist.reshape(lead + (2, E - 1)), nvalid.reshape(lead), q, edges)


def quantile_maps(y, y_hat, quantiles, over='time', scaler=None, mask=None):
    """``(q_obs, q_pred)`` of `distribution_scores`: the sample quantiles of observation and prediction per segment, (..., Q)."""
    r = distribution_scores(y, y_hat, quantiles, over=over, scaler=scaler, mask=mask)
    return r['q_obs'], r['q_pred']


SPECTRUM_MAX_DIM = 16384                           # caps of dl4ds_spectrum
SPECTRUM_MAX_BINS = 16384
SPECTRUM_FIELD_BOUND = 1 << 31


def _folded(n):
    """|signed wavenumber| of every DFT index of an axis of n points, as Python integers."""
    return [min(k, n - k) for k in range(n)]


def radial_bin_map(H, W):
    """-> (int32 (H, W) full-plane bin map, B): bin b = round(L * sqrt((ky/H)^2 + (kx/W)^2)) with L = max(H, W), halves rounded up,
    evaluated in Python integers as (isqrt(4 L^2 (ky^2 W^2 + kx^2 H^2) // (H W)^2) + 1) // 2; -1 where b >= B = L // 2 + 1."""
    L = max(H, W)
    B = L // 2 + 1
    hw2 = (H * W) ** 2
    quad = np.empty((H // 2 + 1, W // 2 + 1), np.int32)           # the map depends on (|ky|, |kx|) alone
    for ky in range(H // 2 + 1):
        for kx in range(W // 2 + 1):
            b = (math.isqrt(4 * L * L * (ky * ky * W * W + kx * kx * H * H) // hw2) + 1) // 2
            quad[ky, kx] = b if b < B else -1
    return np.ascontiguousarray(quad[np.ix_(_folded(H), _folded(W))]), B


def check_spectral_args(shape, bins='radial', detrend='mean', window=None, spacing=1.0, ratio_floor=0.5, batch_size=None):
    """Validation of `spectral_scores` (no library call) -> (int32 (H, W) full-plane bin map, B, detrend flag, window flag)."""
    if len(shape) != 4 or min(shape) < 1:
        raise ValueError(f'expected non-empty (N, H, W, C) arrays, got shape {tuple(shape)}')
    n, h, w, c = (int(v) for v in shape)
    if max(h, w) > SPECTRUM_MAX_DIM:
        raise ValueError(f'fields of {h} x {w} cells are not supported: H and W must not exceed {SPECTRUM_MAX_DIM}')
    if n * c >= SPECTRUM_FIELD_BOUND:
        raise ValueError(f'{n * c} fields are not supported: N*C must stay below 2^31')
    if detrend not in ('mean', None):
        raise ValueError(f"`detrend` must be 'mean' or None, got {detrend!r}")
    if window not in ('hann', None):
        raise ValueError(f"`window` must be 'hann' or None, got {window!r}")
    for name, v in (('spacing', spacing), ('ratio_floor', ratio_floor)):
        if isinstance(v, (bool, str)) or not np.isscalar(v) or not np.isfinite(v) or not v > 0:
            raise ValueError(f'`{name}` must be a positive finite number, got {v!r}')
    check_batch_size(batch_size)
    if isinstance(bins, str):
        if bins != 'radial':
            raise ValueError(f"`bins` must be 'radial' or an integer (H, W) map, got {bins!r}")
        full, B = radial_bin_map(h, w)
        return full, B, int(detrend == 'mean'), int(window == 'hann')
    m = np.asarray(bins)
    if m.dtype == bool or not np.issubdtype(m.dtype, np.integer) or m.shape != (h, w):
        raise ValueError(f"`bins` must be 'radial' or an integer map shaped (H, W) = ({h}, {w})")
    lo, hi = int(m.min()), int(m.max())
    if lo < -1 or hi < 0 or hi >= SPECTRUM_MAX_BINS:
        raise ValueError(f'the entries of `bins` must lie in [-1, {SPECTRUM_MAX_BINS}) and name at least one bin')
    mirror = m[np.ix_([(-k) % h for k in range(h)], [(-k) % w for k in range(w)])]
    if not np.array_equal(m, mirror):
        raise ValueError('`bins` must be symmetric under (ky, kx) -> (-ky, -kx): a real field has a Hermitian transform')
    return np.ascontiguousarray(m, np.int32), hi + 1, int(detrend == 'mean'), int(window == 'hann')


def _fsum_axis0(a, keep):
    """math.fsum over the kept entries of axis 0 of a float64 array: the correctly rounded sum, whatever the order."""
    a = np.asarray(a, np.float64)
    out = np.zeros(a.shape[1:])
    for idx in np.ndindex(out.shape):
        out[idx] = math.fsum(float(a[(n,) + idx]) for n in range(a.shape[0]) if keep[(n,) + idx[:keep.ndim - 1]])
    return out


def _lsd(ratio, usable):
    """sqrt(mean((10 log10 ratio)^2)) over the usable bins of the last axis (math.fsum of the squares); NaN without one."""
    ratio, usable = np.asarray(ratio, np.float64), np.asarray(usable, bool)
    out = np.full(ratio.shape[:-1], np.nan)
    for idx in np.ndindex(out.shape):
        sel = usable[idx]
        if sel.any():
            d = 10.0 * np.log10(np.ascontiguousarray(ratio[idx][sel]))
            out[idx] = math.sqrt(math.fsum(float(v) * float(v) for v in d) / int(sel.sum()))
    return out


def _spectral_ratios(po, pp, cr, ci, count):
    """(psd_ratio, coherence, bins usable for the log-spectral distance) of power and cross spectra over the last axis."""
    ratio, coh = _exact.ratio(pp, po), _exact.ratio(cr * cr + ci * ci, po * pp)
    usable = (np.arange(po.shape[-1]) >= 1) & (count > 0) & (po > 0) & (pp > 0)
    return ratio, coh, usable


def spectra_from_sums(power, nvalid, mean, count, hw, spacing=1.0, ratio_floor=0.5):
    """The result dict of `spectral_scores` from the outputs of `dl4ds_spectrum` (host arithmetic only): ``power`` (N, C, 4, B),
    ``nvalid`` (N, C), ``mean`` (N, C, 2), ``count`` (B,) full-plane coefficients per bin, ``hw`` = (H, W)."""
    power, nvalid = np.asarray(power, np.float64), np.asarray(nvalid, np.int64)
    mean, count = np.asarray(mean, np.float64), np.asarray(count, np.int64)
    H, W = (int(v) for v in hw)
    B = power.shape[-1]
    norm = float((H * W) ** 2)
    empty = nvalid == 0
    with np.errstate(divide='ignore'):
        wavenumber = np.arange(B, dtype=np.float64) / (float(max(H, W)) * float(spacing))
        wavelength = 1.0 / wavenumber
    po, pp, cr, ci = (np.ascontiguousarray(power[:, :, k]) / norm for k in range(4))
    cross = np.empty(po.shape, np.complex128)
    cross.real, cross.imag = cr, ci
    ratio, coh, usable = _spectral_ratios(po, pp, cr, ci, count)
    blank = lambda a: np.where(empty[(...,) + (None,) * (a.ndim - 2)], np.nan, a)     # every score of an empty field is NaN
    res = dict(wavenumber=wavenumber, wavelength=wavelength, count=count, n_valid=nvalid, mean_obs=mean[..., 0],
               mean_pred=mean[..., 1], power_obs=po, power_pred=pp, psd_obs=blank(_exact.ratio(po, count)),
               psd_pred=blank(_exact.ratio(pp, count)), cross=cross, coherence=blank(coh), psd_ratio=blank(ratio),
               lsd=blank(_lsd(ratio, usable)))
    keep = ~empty
    pool = [_fsum_axis0(a, keep) for a in (po, pp, cr, ci)]
    cpool = np.empty(pool[0].shape, np.complex128)
    cpool.real, cpool.imag = pool[2], pool[3]
    pratio, pcoh, pusable = _spectral_ratios(*pool, count)
    eff = np.full(pratio.shape[0], np.nan)
    for c in range(pratio.shape[0]):
        best = 0
        for b in range(1, B):
            if count[b] > 0 and not pratio[c, b] >= ratio_floor:          # (NaN fails)
                break
            best = b
        if best:
            eff[c] = wavelength[best]
    res.update(power_obs_pooled=pool[0], power_pred_pooled=pool[1], cross_pooled=cpool, psd_ratio_pooled=pratio,
               coherence_pooled=pcoh, lsd_pooled=_lsd(pratio, pusable), effective_wavelength=eff)
    return res


def _device_spectra(obs, pred, full, B, detrend, window, batch_size):
    """`dl4ds_spectrum` over sample blocks of the float32 observation (and prediction, or None) -> (power (N, C, 4, B), n_valid
    (N, C), mean (N, C, 2))."""
    N, H, W, C = obs.shape
    half = np.ascontiguousarray(full[:, :W // 2 + 1], np.int32)
    power, nvalid, mean = np.empty((N, C, 4, B), np.float64), np.empty((N, C), np.int64), np.empty((N, C, 2), np.float64)
    lib = _lib.lib()

    def call(b, dy, dp, dpower, dvalid, dmean):
        _lib.check(lib.dl4ds_spectrum(dy, dp, b, H, W, C, detrend, window, half.ctypes.data, B, dpower, dvalid, dmean))
    paired_chunks(obs, pred, (power, nvalid, mean), call, batch_size)
    return power, nvalid, mean


def _bin_counts(full, B):
    return np.bincount(full[full >= 0].ravel(), minlength=B).astype(np.int64)


def spectral_scores(y_test, y_test_hat, bins='radial', detrend='mean', window=None, spacing=1.0, ratio_floor=0.5, scaler=None,
                    mask=None, batch_size=None):
    """Does the prediction have the observation's variance at every spatial scale, and below which wavelength is it merely smooth?
    Per field (each of the N*C planes of the (N, H, W, C) arrays), on the device (csrc/spectrum.hip): the two-dimensional DFT of
    both sides in fp64, folded over wavenumber bins into power and cross spectra.  Inputs are prepared as in `neighbourhood_scores`
    (5-D squeezed, optional ``scaler.inverse_transform``) and read as float32.  A cell is kept when both arrays are finite there
    and ``mask`` (2-D or with a channel axis, 0 = excluded) keeps it; ``detrend='mean'`` subtracts each side's own mean over the
    kept cells (``None``: nothing); excluded cells are then 0; ``window='hann'`` multiplies by the periodic Hann window of either
    axis.  ``bins='radial'``: bin b = round(L sqrt((ky/H)^2 + (kx/W)^2)) with L = max(H, W), halves up, in exact integers,
    B = L // 2 + 1 bins, coefficients beyond dropped; or an integer (H, W) map of the full plane with values in [0, B) or -1
    (dropped), symmetric under (ky, kx) -> (-ky, -kx) (directional spectra).  ``spacing``: the grid spacing, the unit of the
    wavelengths.  The arrays are uploaded in chunks of ``batch_size`` samples (default: at most 256 MiB per array); the result is
    bitwise independent of it.  Returns a dict (float64 unless said otherwise):

    * ``wavenumber`` (B,) = b / (L spacing), ``wavelength`` its inverse (inf at b = 0), ``count`` (B,) int64 coefficients per bin;
    * ``n_valid`` (N, C) int64, ``mean_obs``, ``mean_pred`` (N, C): the subtracted means (0 without detrending);
    * ``power_obs``, ``power_pred`` (N, C, B): sum of |X|^2 over the bin / (H W)^2 -- with detrending and no window they add up to
      the variance over the kept cells times n_valid / (H W), less the dropped coefficients; ``psd_obs``, ``psd_pred`` = power /
      count; ``cross`` (N, C, B) complex128 = sum of Y conj(P) / (H W)^2;
    * ``coherence`` = |cross|^2 / (power_obs power_pred), ``psd_ratio`` = power_pred / power_obs (N, C, B);
    * ``lsd`` (N, C) = sqrt(mean((10 log10 psd_ratio)^2)) over the bins b >= 1 with count > 0 and both powers > 0;
    * pooled over the samples with n_valid > 0, per channel: ``power_obs_pooled``, ``power_pred_pooled``, ``cross_pooled`` (C, B)
      (math.fsum), ``psd_ratio_pooled``, ``coherence_pooled`` (C, B), ``lsd_pooled`` (C,) and ``effective_wavelength`` (C,): the
      wavelength of the largest b* with psd_ratio_pooled >= ``ratio_floor`` on every bin 1 .. b* with count > 0, NaN when bin 1 fails.

    Every ratio is NaN on a zero denominator; psd, coherence, psd_ratio and lsd of a field with n_valid = 0 are NaN (its power is 0)."""
    obs, y_test_hat, (full, B, dt, win) = _prepared(
        y_test, y_test_hat, scaler, mask, lambda shape: check_spectral_args(shape, bins, detrend, window, spacing, ratio_floor, batch_size))
    power, nvalid, mean = _device_spectra(obs, y_test_hat, full, B, dt, win, batch_size)
    return spectra_from_sums(power, nvalid, mean, _bin_counts(full, B), obs.shape[1:3], spacing, ratio_floor)


def power_spectrum(y, bins='radial', detrend='mean', window=None, spacing=1.0, scaler=None, mask=None):
    """``(wavenumber, psd)`` of one (N, H, W, C) array: (B,) and (N, C, B) as ``psd_obs`` of `spectral_scores`, without a prediction."""
    y = np.asarray(getattr(y, 'values', y))
    if y.ndim == 5:
        y = np.squeeze(y, -1)
    y = checkarray_ndim(y, 4, -1)
    if y.ndim != 4:
        raise ValueError(f'expected an (N, H, W, C) array, got {y.shape}')
    full, B, dt, win = check_spectral_args(y.shape, bins, detrend, window, spacing)
    if scaler is not None and hasattr(scaler, 'inverse_transform'):
        y = scaler.inverse_transform(y)
    obs = _masked_observation(y, mask)
    power, nvalid, mean = _device_spectra(obs, None, full, B, dt, win, None)
    r = spectra_from_sums(power, nvalid, mean, _bin_counts(full, B), obs.shape[1:3], spacing)
    return r['wavenumber'], r['psd_obs']
