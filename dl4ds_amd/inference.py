"""Predictor / predict -- dl4ds/inference.py:12-255: forward-only entry on the same graph runtime."""
import numpy as np

from . import POSTUPSAMPLING_METHODS
from .dataloader import create_batch_hr_lr
from .ensemble_score import (NEIGHBOURHOOD_DEFAULT_WINDOWS, check_exceedance_args, check_multivariate_args,
                             check_neighbourhood_ensemble_args, check_score_args)
from .graph import check_ensemble_args
from .metrics import _masked_observation


def _prepare_inputs(trainer, array, scale, array_in_hr, static_vars, predictors, time_window, interpolation):
    """The part of ``predict`` in front of the network (inference.py:172-236) -> (model, list of input arrays): HR arrays are
    coarsened by the batch builder, LR arrays are first re-expanded to the HR grid (``resize_array``, :196-199) and handed over as
    ``array_lr``; one batch of all ``n - (time_window - 1)`` samples (:186-189)."""
    from .dataloader import resize_array, checkarray_ndim
    if hasattr(trainer, 'model'):
        model = trainer.model
    elif hasattr(trainer, 'generator'):
        model = trainer.generator
    else:
        model = trainer
    upsampling = model.name.split('_')[-1]                       # inference.py:172
    if len(model.input_shapes[0]) == 4 and time_window is None:  # (T,H,W,C) per sample == a 5-D Keras input, :173-175
        raise ValueError('`time_window` must be provided for spatiotemporal model')
    array = np.asarray(getattr(array, 'values', array))
    if static_vars is not None:
        static_vars = [np.asarray(getattr(v, 'values', v)) for v in static_vars]
    n_samples = array.shape[0]
    if time_window is not None:
        n_samples -= time_window - 1                             # inference.py:187-189
    preds = None if predictors is None else np.concatenate([np.asarray(p) for p in predictors], axis=-1)
    if array_in_hr:
        array_hr, array_lr = array, None
    else:
        array = checkarray_ndim(array, 4, -1)
        hr_xy = (array.shape[2] * scale, array.shape[1] * scale)
        array_hr = resize_array(array, hr_xy, interpolation, squeezed=False)
        array_lr = array
    x, _ = create_batch_hr_lr(np.arange(n_samples), 0, array_hr, array_lr, upsampling=upsampling, scale=scale,
                              batch_size=n_samples, patch_size=None, time_window=time_window, static_vars=static_vars,
                              predictors=preds, interpolation=interpolation)
    return model, x


def predict(trainer, array, scale, array_in_hr=True, static_vars=None, predictors=None, time_window=None,
            time_metadata=None, interpolation='inter_area', batch_size=64, scaler=None, save_path=None,
            save_fname='y_hat.npy', return_lr=False, device='GPU'):
    """inference.py:109-255, step for step: the inputs are prepared as the reference does (``_prepare_inputs``) and go through
    ``model.predict``."""
    model, inputs = _prepare_inputs(trainer, array, scale, array_in_hr, static_vars, predictors, time_window, interpolation)
    y = model.predict(inputs, batch_size=batch_size, verbose=0)
    if y.ndim == 5 and time_window is not None:                  # inference.py:241-242
        from .utils import spatiotemporal_to_spatial_samples
        y = spatiotemporal_to_spatial_samples(y, time_window)
    if scaler is not None:
        y = scaler.inverse_transform(y)
    y = np.asarray(y, np.float32)
    if save_path is not None and save_fname is not None:
        np.save(save_path + ('' if save_path.endswith('/') else '/') + save_fname, y)
    return (y, np.asarray(inputs[0])) if return_lr else y


def predict_tiled(trainer, array, scale, tile, halo=None, blend='crop', array_in_hr=True, static_vars=None, predictors=None,
                  time_window=None, time_metadata=None, interpolation='inter_area', batch_size=32, scaler=None, save_path=None,
                  save_fname='y_hat.npy', return_lr=False, device='GPU'):
    """``predict`` on a grid that is run tile by tile (``Model.predict_tiled``): the inputs are prepared as
    ``predict`` prepares them, the network runs on overlapping tiles of ``tile`` pixels of its first input (the LR grid of a
    post-upsampling model, the HR grid of a 'pin' model) and the tile outputs are merged on the device.  ``halo``, ``blend``: see
    ``Model.predict_tiled`` (None: the model's ``receptive_halo``; a model whose reach is unbounded needs an explicit halo and
    gives an approximation).  ``batch_size``: tiles per forward pass.  Scaler, saving and ``return_lr`` as in ``predict``.
    Spatio-temporal models are out of scope (ValueError)."""
    if time_window is not None:
        raise ValueError('predict_tiled: spatio-temporal models (`time_window`) are out of scope of tiled prediction; use predict')
    model, inputs = _prepare_inputs(trainer, array, scale, array_in_hr, static_vars, predictors, time_window, interpolation)
    y = model.predict_tiled(inputs, tile, halo=halo, blend=blend, batch_size=batch_size)
    if scaler is not None:
        y = scaler.inverse_transform(y)
    y = np.asarray(y, np.float32)
    if save_path is not None and save_fname is not None:
        np.save(save_path + ('' if save_path.endswith('/') else '/') + save_fname, y)
    return (y, np.asarray(inputs[0])) if return_lr else y


def _slope(scaler, shape):
    one = np.asarray(scaler.inverse_transform(np.ones(tuple(shape), np.float64)), np.float64)
    zero = np.asarray(scaler.inverse_transform(np.zeros(tuple(shape), np.float64)), np.float64)
    return one - zero


def scaler_slope(scaler, sample_shape):
    """Slope of ``scaler.inverse_transform`` per cell of one sample: inverse_transform(ones) - inverse_transform(zeros) in float64.
    Exact for MinMaxScaler and StandardScaler of dl4ds_amd.preprocessing, whose inverse transforms are affine per cell.  Evaluated on
    two samples, of which the first is returned: the scalers drop size-1 axes, a lone sample would lose its sample axis."""
    return _slope(scaler, (2,) + tuple(sample_shape))[0]


def _finish_ensemble(res, scaler, time_window):
    """What ``predict_ensemble`` does to the raw statistics of ``Model.predict_ensemble``: spatio-temporal flattening, the scaler's
    inverse transform of the values and its slope on the spread; in place."""
    stacked = ('quantiles', 'members')                 # leading axis in front of the sample axis

    def each(key, fn):
        a = res[key]
        if key in stacked:
            if a.shape[0]:
                res[key] = np.stack([np.asarray(fn(a[j]), np.float32) for j in range(a.shape[0])])
        else:
            res[key] = np.asarray(fn(a), np.float32)

    if res['mean'].ndim == 5 and time_window is not None:        # inference.py:241-242
        from .utils import spatiotemporal_to_spatial_samples
        for key in list(res):
            each(key, lambda a: spatiotemporal_to_spatial_samples(a, time_window))
    if scaler is not None:
        try:
            slope = scaler_slope(scaler, res['mean'].shape[1:])
        except IndexError:                 # a scaler fitted on data with NaNs carries a mask of the full array's shape
            slope = _slope(scaler, res['mean'].shape)
        std64 = res['std'].astype(np.float64)
        for key in list(res):
            if key != 'std':
                each(key, scaler.inverse_transform)
        # (the scalers drop size-1 axes: the slope then has the trailing axes of the transformed mean and broadcasts over the samples)
        res['std'] = (np.abs(slope) * std64.reshape(res['mean'].shape)).astype(np.float32)
    if not len(res['quantiles']):
        res['quantiles'] = np.empty((0,) + res['mean'].shape, np.float32)


def predict_ensemble(trainer, array, scale, n_members, quantiles=(), seed=None, array_in_hr=True, static_vars=None,
                     predictors=None, time_window=None, time_metadata=None, interpolation='inter_area', batch_size=64,
                     scaler=None, save_path=None, save_fname='y_hat_ensemble.npz', return_lr=False, return_members=False,
                     device='GPU'):
    """``predict`` for a model built with one of the MC dropout variants ('mcdrop', 'mcgaussiandrop', 'mcspatialdrop' --
    blocks.py:658-676, active at inference): ``n_members`` stochastic forward passes per sample, reduced on the device
    (``Model.predict_ensemble``).  Returns a dict of float32 arrays: 'mean', 'std' (population), 'min', 'max' shaped like the
    result of ``predict``, 'quantiles' with a leading axis of len(quantiles) (np.quantile's 'linear' method), and 'members' with a
    leading axis of n_members when ``return_members``; ``(dict, lr)`` with ``return_lr``.  ``seed``: an integer makes the result
    reproducible -- it is a function of (weights, inputs, n_members, batch_size, seed); None lets the model's noise continue.

    Spatio-temporal outputs: every statistic goes through ``spatiotemporal_to_spatial_samples`` like ``predict``'s result.
    ``scaler``: 'mean', 'min', 'max', 'quantiles' and 'members' go through ``scaler.inverse_transform``; 'std' is a spread, not a
    value, and is multiplied by the transform's slope ``inverse_transform(ones) - inverse_transform(zeros)``, evaluated once in
    float64 on one sample's shape (``scaler_slope``).  That is exact for both scalers of ``dl4ds_amd.preprocessing``, which are
    affine per cell (for an inverse transform that is not affine it would be meaningless).  ``save_path``: one ``np.savez`` of
    the dict."""
    check_ensemble_args(n_members, quantiles, seed, batch_size)         # before anything touches the device
    model, inputs = _prepare_inputs(trainer, array, scale, array_in_hr, static_vars, predictors, time_window, interpolation)
    res = model.predict_ensemble(inputs, n_members, batch_size=batch_size, quantiles=quantiles, seed=seed,
                                 return_members=return_members)
    _finish_ensemble(res, scaler, time_window)
    if save_path is not None and save_fname is not None:
        np.savez(save_path + ('' if save_path.endswith('/') else '/') + save_fname, **res)
    return (res, np.asarray(inputs[0])) if return_lr else res


def _check_verify_args(array, scale, n_members, y_true, quantiles, seed, fair, array_in_hr, time_window, batch_size, scaler=None,
                       who='verify_ensemble', model_method='Model.score_ensemble'):
    """Everything ``verify_ensemble`` / ``verify_exceedance`` can refuse from the arguments they share (no library, no device) ->
    the observation as an array with a channel axis."""
    check_ensemble_args(n_members, quantiles, seed, batch_size)
    check_score_args(fair)
    if time_window is not None:
        raise ValueError(f'{who}: `time_window` is not supported: how scores of overlapping windows flatten to spatial '
                         f'samples is not defined yet (score the 5-D output with {model_method})')
    array = np.asarray(getattr(array, 'values', array))
    if y_true is None:
        if not array_in_hr:
            raise ValueError('`y_true` is required when `array_in_hr` is False (there is no HR field to verify against)')
        if scaler is not None:
            raise ValueError('`y_true` is required with a `scaler`: the observation is taken in physical units, while the HR '
                             '`array` that feeds the model is in the model\'s units then')
        y_true = array
    y_true = np.asarray(getattr(y_true, 'values', y_true))
    if y_true.ndim == 3:
        y_true = y_true[..., None]
    grid = tuple(array.shape[1:3]) if array_in_hr else (array.shape[1] * scale, array.shape[2] * scale)
    if y_true.ndim != 4 or tuple(y_true.shape[:3]) != (array.shape[0],) + grid:
        raise ValueError(f"`y_true` must have the shape of predict's result {(array.shape[0],) + grid + ('C',)}, got {y_true.shape}")
    return y_true


def _model_unit_observation(y_true, scaler, mask):
    """The physical observation as the model sees it: through ``scaler.transform`` (if any), NaN kept as NaN, NaN where ``mask``
    excludes.  The scalers' transform replaces NaN by a fill value and, built with copy=False, writes into its argument: the
    positions that are not finite are recorded first and the transform gets a copy."""
    obs = y_true
    if scaler is not None:
        bad = ~np.isfinite(np.asarray(y_true, np.float64))
        obs = np.array(scaler.transform(np.array(y_true, copy=True)), np.float32).reshape(y_true.shape)
        obs[bad] = np.nan
    return _masked_observation(obs, mask)


def _saved_and_returned(res, key, inputs, save_path, save_fname, return_lr):
    """The end of ``verify_ensemble`` / ``verify_exceedance``: one ``np.savez`` of the statistics and of the scores ``res[key]``
    (flattened with a ``key_`` prefix) -> ``res``, or ``(res, lr)`` with ``return_lr``."""
    if save_path is not None and save_fname is not None:
        flat = {k: v for k, v in res.items() if k != key}
        flat.update({f'{key}_{k}': np.asarray(v) for k, v in res[key].items()})
        np.savez(save_path + ('' if save_path.endswith('/') else '/') + save_fname, **flat)
    return (res, np.asarray(inputs[0])) if return_lr else res


def verify_ensemble(trainer, array, scale, n_members, y_true=None, quantiles=(), seed=None, fair=False, mask=None,
                    array_in_hr=True, static_vars=None, predictors=None, time_window=None, time_metadata=None,
                    interpolation='inter_area', batch_size=64, scaler=None, save_path=None,
                    save_fname='y_hat_ensemble_scores.npz', return_lr=False, device='GPU'):
    """``predict_ensemble`` plus the verification of the ensemble against the observation, scored on the device while the member
    stack is resident (``Model.score_ensemble``, csrc/ensemble_score.hip): returns ``predict_ensemble``'s dict of statistics with
    one more key, 'scores' -- CRPS (``fair``: the fair form), spread, RMSE of the ensemble mean, spread / RMSE, each over all valid
    elements, per sample and as a map; the rank histogram; the coverage of ``quantiles``; see ``Model.score_ensemble`` for every key.

    ``y_true``: the observation in physical units, shaped like ``predict``'s result; None means the HR ``array`` itself and is
    allowed only with ``array_in_hr=True`` and without a ``scaler`` (with one, ``array`` is in the model's units).  ``mask``: as in ``compute_metrics`` (2-D or with a channel axis, 0 = excluded); NaN
    and infinite observations or members exclude their element too.  ``scaler``: the observation goes through
    ``scaler.transform`` (the members live in the model's units, scoring happens there) and the slope of
    ``scaler.inverse_transform`` per cell (``scaler_slope``) carries CRPS, spread and RMSE back into physical units; the ranks do
    not change.  Cells whose slope is not finite and positive are excluded and counted in ``scores['n_cells_excluded']``.  NaN in ``y_true``
    stays NaN through the transform (which would otherwise fill it); a scaler fitted on data with NaNs, whose inverse transform has
    no per-cell slope for one sample, raises ValueError.
    ``save_path``: one ``np.savez`` of the statistics and the scores (flattened with a ``scores_`` prefix).

    Out of scope: recurrent models.  ``time_window is not None`` raises ValueError, because how the scores of overlapping windows
    flatten to spatial samples is not defined yet."""
    y_true = _check_verify_args(array, scale, n_members, y_true, quantiles, seed, fair, array_in_hr, time_window, batch_size,
                                scaler)
    model, inputs = _prepare_inputs(trainer, array, scale, array_in_hr, static_vars, predictors, time_window, interpolation)
    obs, slope = _model_unit_observation(y_true, scaler, mask), None
    if scaler is not None:
        try:
            slope = np.asarray(scaler_slope(scaler, y_true.shape[1:]), np.float64)
        except IndexError:
            raise ValueError('verify_ensemble: `scaler` has no per-cell slope for one sample (a scaler fitted on data with NaNs '
                             'carries a mask of the full array\'s shape); that is not supported') from None
        if slope.size == int(np.prod(y_true.shape[1:])):       # (the scalers drop size-1 axes)
            slope = slope.reshape(y_true.shape[1:])
    res = model.score_ensemble(inputs, obs, n_members, batch_size=batch_size, quantiles=quantiles, seed=seed, fair=fair,
                               scale=slope)
    scores = res.pop('scores')
    _finish_ensemble(res, scaler, time_window)
    res['scores'] = scores
    return _saved_and_returned(res, 'scores', inputs, save_path, save_fname, return_lr)


def _model_unit_thresholds(thresholds, scaler, sample_shape, who='verify_exceedance'):
    """Physical ``thresholds`` (checked by ``check_exceedance_args``; (T,) values or (T,) + sample_shape fields) -> (float32 threshold fields (T,) + sample_shape in the
    model's units, number of cells excluded): every threshold goes through ``scaler.transform`` as a field, evaluated on two
    samples of which the first is kept (the scalers drop size-1 axes); cells whose ``scaler_slope`` is not finite and positive
    get NaN."""
    sample_shape = tuple(sample_shape)
    try:
        slope = np.asarray(scaler_slope(scaler, sample_shape), np.float64)
        fields = []
        for t in thresholds:
            both = np.broadcast_to(np.asarray(t, np.float64), (2,) + sample_shape).copy()
            fields.append(np.asarray(scaler.transform(both), np.float32)[0].reshape(sample_shape))
    except IndexError:
        raise ValueError(f'{who}: `scaler` has no per-cell transform for one sample (a scaler fitted on data with NaNs '
                         'carries a mask of the full array\'s shape); that is not supported') from None
    thr = np.stack(fields)
    with np.errstate(invalid='ignore'):
        bad = ~(np.isfinite(slope) & (slope > 0))
    bad = np.broadcast_to(bad.reshape(sample_shape) if bad.size == int(np.prod(sample_shape)) else bad, sample_shape)
    thr[:, bad] = np.nan
    return thr, int(np.count_nonzero(bad))


def verify_exceedance(trainer, array, scale, n_members, thresholds, y_true=None, seed=None, mask=None, array_in_hr=True,
                      static_vars=None, predictors=None, time_window=None, time_metadata=None, interpolation='inter_area',
                      batch_size=64, scaler=None, save_path=None, save_fname='y_hat_exceedance.npz', return_lr=False, device='GPU'):
    """``predict_ensemble`` plus the verification of the ensemble as a PROBABILITY forecast of the events ``value >= threshold``,
    counted on the device while the member stack is resident (``Model.score_exceedance``, csrc/exceedance.hip): returns
    ``predict_ensemble``'s dict of statistics with one more key, 'exceedance' -- the contingency table of the forecast count
    against the observed event, the Brier score with its reliability / resolution / uncertainty decomposition and the skill
    score, the reliability diagram, the ROC curve and its area, Brier maps and per-sample scores; see
    ``metrics.exceedance_scores`` for every key.  All of them come from exact integer sums.

    ``thresholds``: up to 16 numbers in PHYSICAL units (or one field per threshold shaped like one sample of the result).
    ``y_true``, ``mask``: as in ``verify_ensemble`` (the observation in physical units; None means the HR ``array`` itself, allowed
    only with ``array_in_hr=True`` and without a ``scaler``).  ``scaler``: the observation goes through ``scaler.transform`` and
    each threshold becomes a per-cell field in the model's units (``scaler.transform`` of a constant field): EVENTS ARE DECIDED IN
    THE MODEL'S UNITS, where the members live; for the increasing affine scalers of ``dl4ds_amd.preprocessing`` that is the event
    in physical units up to the float32 rounding of the transform.  Cells whose ``scaler_slope`` is not finite and positive get a
    NaN threshold, take no part, and are counted in ``exceedance['n_cells_excluded']``.  NaN in ``y_true`` stays NaN through the
    transform.  ``save_path``: one ``np.savez`` of the statistics and the scores (flattened with an ``exceedance_`` prefix).

    Out of scope: recurrent models.  ``time_window is not None`` raises ValueError, because how the scores of overlapping windows
    flatten to spatial samples is not defined yet."""
    y_true = _check_verify_args(array, scale, n_members, y_true, (), seed, False, array_in_hr, time_window, batch_size, scaler,
                                who='verify_exceedance', model_method='Model.score_exceedance')
    thr = check_exceedance_args(thresholds, y_true.shape[1:])
    model, inputs = _prepare_inputs(trainer, array, scale, array_in_hr, static_vars, predictors, time_window, interpolation)
    obs, excluded = _model_unit_observation(y_true, scaler, mask), 0
    if scaler is not None:
        # (the caller's float64 values are transformed, not their float32 roundings)
        physical = np.asarray(getattr(thresholds, 'values', thresholds), np.float64).reshape(thr.shape)
        thr, excluded = _model_unit_thresholds(physical, scaler, y_true.shape[1:])
    res = model.score_exceedance(inputs, obs, n_members, thr, batch_size=batch_size, seed=seed)
    scores = res.pop('exceedance')
    scores['n_cells_excluded'] = excluded
    _finish_ensemble(res, scaler, time_window)
    res['exceedance'] = scores
    return _saved_and_returned(res, 'exceedance', inputs, save_path, save_fname, return_lr)


def verify_multivariate(trainer, array, scale, n_members, y_true=None, seed=None, max_lag=4, order=0.5, lag_weights='inverse',
                        fair=False, weights=None, mask=None, array_in_hr=True, static_vars=None, predictors=None, time_window=None,
                        time_metadata=None, interpolation='inter_area', batch_size=64, scaler=None, save_path=None,
                        save_fname='y_hat_multivariate.npz', return_lr=False, device='GPU'):
    """``predict_ensemble`` plus the verification of the ensemble as a forecast of a FIELD: the energy score and the variogram
    score, reduced on the device while the member stack is resident (``Model.score_multivariate``, csrc/ensemble_multi.hip):
    returns ``predict_ensemble``'s dict of statistics with one more key, 'multivariate'; see ``metrics.multivariate_scores`` for
    every key and for ``max_lag``, ``order``, ``lag_weights``, ``fair`` and ``weights`` (``losses.latitude_weights`` fits).

    ``y_true``, ``mask``: as in ``verify_ensemble`` (the observation in physical units; None means the HR ``array`` itself, allowed
    only with ``array_in_hr=True`` and without a ``scaler``).  ``scaler``: the observation goes through ``scaler.transform`` and
    THE SCORES ARE TAKEN IN THE MODEL'S UNITS, where the members live: a distance between fields has no per-cell slope that would
    carry it back.  NaN in ``y_true`` stays NaN through the transform.  ``save_path``: one ``np.savez`` of the statistics and the
    scores (flattened with a ``multivariate_`` prefix).

    Out of scope: recurrent models.  ``time_window is not None`` raises ValueError, because how the scores of overlapping windows
    flatten to spatial samples is not defined yet."""
    y_true = _check_verify_args(array, scale, n_members, y_true, (), seed, False, array_in_hr, time_window, batch_size, scaler,
                                who='verify_multivariate', model_method='Model.score_multivariate')
    check_multivariate_args(max_lag, order, lag_weights, fair, weights, None, n_members)
    model, inputs = _prepare_inputs(trainer, array, scale, array_in_hr, static_vars, predictors, time_window, interpolation)
    obs = _model_unit_observation(y_true, scaler, mask)
    res = model.score_multivariate(inputs, obs, n_members, batch_size=batch_size, seed=seed, max_lag=max_lag, order=order,
                                   lag_weights=lag_weights, fair=fair, weights=weights)
    scores = res.pop('multivariate')
    _finish_ensemble(res, scaler, time_window)
    res['multivariate'] = scores
    return _saved_and_returned(res, 'multivariate', inputs, save_path, save_fname, return_lr)


def verify_neighbourhood(trainer, array, scale, n_members, thresholds, windows=NEIGHBOURHOOD_DEFAULT_WINDOWS, y_true=None, seed=None,
                         mask=None, array_in_hr=True, static_vars=None, predictors=None, time_window=None, time_metadata=None,
                         interpolation='inter_area', batch_size=64, scaler=None, save_path=None,
                         save_fname='y_hat_neighbourhood.npz', return_lr=False, device='GPU'):
    """``predict_ensemble`` plus the NEIGHBOURHOOD verification of the ensemble as a probability forecast of the events ``value >=
    threshold``, reduced on the device while the member stack is resident (``Model.score_neighbourhood``, csrc/ensemble_fss.hip):
    returns ``predict_ensemble``'s dict of statistics with one more key, 'neighbourhood' -- the Fractions Skill Score of the
    neighbourhood ensemble probability and the neighbourhood Brier score per threshold and window size; see
    ``metrics.neighbourhood_ensemble_scores`` for every key.  All of them come from exact integer sums.

    ``thresholds``: up to 16 strictly increasing numbers in PHYSICAL units; ``windows``: strictly increasing sizes >= 1.
    ``y_true``, ``mask``: as in ``verify_ensemble`` (the observation in physical units; None means the HR ``array`` itself, allowed
    only with ``array_in_hr=True`` and without a ``scaler``).  ``scaler``: the observation and the thresholds go through
    ``scaler.transform``: EVENTS ARE DECIDED IN THE MODEL'S UNITS, where the members live.  The entry takes one value per threshold,
    so the transform must map a threshold to the same value in every cell (a scaler fitted over all axes does) and keep the
    thresholds increasing; anything else raises ValueError.  NaN in ``y_true`` stays NaN through the transform.  ``save_path``: one
    ``np.savez`` of the statistics and the scores (flattened with a ``neighbourhood_`` prefix).

    Out of scope: recurrent models.  ``time_window is not None`` raises ValueError, because how the scores of overlapping windows
    flatten to spatial samples is not defined yet."""
    y_true = _check_verify_args(array, scale, n_members, y_true, (), seed, False, array_in_hr, time_window, batch_size, scaler,
                                who='verify_neighbourhood', model_method='Model.score_neighbourhood')
    thr, win = check_neighbourhood_ensemble_args(y_true.shape[1:], n_members, thresholds, windows)
    model, inputs = _prepare_inputs(trainer, array, scale, array_in_hr, static_vars, predictors, time_window, interpolation)
    obs = _model_unit_observation(y_true, scaler, mask)
    if scaler is not None:
        physical = np.atleast_1d(np.asarray(getattr(thresholds, 'values', thresholds), np.float64))
        fields, _ = _model_unit_thresholds(physical, scaler, y_true.shape[1:], who='verify_neighbourhood')
        flat = fields.reshape(len(physical), -1)
        if not (flat == flat[:, :1]).all():                    # (a NaN, the mark of an unusable cell, fails it too)
            raise ValueError('verify_neighbourhood: `scaler` maps a threshold to different values in different cells; the '
                             'neighbourhood verification takes one value per threshold (score in the model\'s units instead)')
        thr = flat[:, 0]
    res = model.score_neighbourhood(inputs, obs, n_members, thr, win.tolist(), batch_size=batch_size, seed=seed)
    scores = res.pop('neighbourhood')
    _finish_ensemble(res, scaler, time_window)
    res['neighbourhood'] = scores
    return _saved_and_returned(res, 'neighbourhood', inputs, save_path, save_fname, return_lr)


class Predictor:
    """inference.py:12-106."""

    def __init__(self, trainer, array, scale, array_in_hr=False, static_vars=None, predictors=None, time_window=None,
                 time_metadata=None, interpolation='inter_area', batch_size=64, scaler=None, save_path=None, save_fname='y_hat.npy',
                 return_lr=False, device='GPU'):
        self.kw = dict(trainer=trainer, array=array, scale=scale, array_in_hr=array_in_hr, static_vars=static_vars,
                       predictors=predictors, time_window=time_window, time_metadata=time_metadata,
                       interpolation=interpolation,
                       batch_size=batch_size, scaler=scaler, save_path=save_path, save_fname=save_fname,
                       return_lr=return_lr, device=device)

    def run(self):
        return predict(**self.kw)


class TiledPredictor:
    """``Predictor`` for tiled prediction: same constructor-then-``.run()`` shape, runs ``predict_tiled``."""

    def __init__(self, trainer, array, scale, tile, halo=None, blend='crop', array_in_hr=False, static_vars=None, predictors=None,
                 time_window=None, time_metadata=None, interpolation='inter_area', batch_size=32, scaler=None, save_path=None,
                 save_fname='y_hat.npy', return_lr=False, device='GPU'):
        self.kw = dict(trainer=trainer, array=array, scale=scale, tile=tile, halo=halo, blend=blend, array_in_hr=array_in_hr,
                       static_vars=static_vars, predictors=predictors, time_window=time_window, time_metadata=time_metadata,
                       interpolation=interpolation, batch_size=batch_size, scaler=scaler, save_path=save_path,
                       save_fname=save_fname, return_lr=return_lr, device=device)

    def run(self):
        return predict_tiled(**self.kw)


class EnsemblePredictor:
    """``Predictor`` for MC-dropout ensembles: same constructor-then-``.run()`` shape, runs ``predict_ensemble``."""

    def __init__(self, trainer, array, scale, n_members, quantiles=(), seed=None, array_in_hr=False, static_vars=None,
                 predictors=None, time_window=None, time_metadata=None, interpolation='inter_area', batch_size=64, scaler=None,
                 save_path=None, save_fname='y_hat_ensemble.npz', return_lr=False, return_members=False, device='GPU'):
        self.kw = dict(trainer=trainer, array=array, scale=scale, n_members=n_members, quantiles=quantiles, seed=seed,
                       array_in_hr=array_in_hr, static_vars=static_vars, predictors=predictors, time_window=time_window,
                       time_metadata=time_metadata, interpolation=interpolation, batch_size=batch_size, scaler=scaler,
                       save_path=save_path, save_fname=save_fname, return_lr=return_lr, return_members=return_members,
                       device=device)

    def run(self):
        return predict_ensemble(**self.kw)


class EnsembleVerifier:
    """``EnsemblePredictor`` for the verification: same constructor-then-``.run()`` shape, runs ``verify_ensemble``."""

    def __init__(self, trainer, array, scale, n_members, y_true=None, quantiles=(), seed=None, fair=False, mask=None,
                 array_in_hr=False, static_vars=None, predictors=None, time_window=None, time_metadata=None,
                 interpolation='inter_area', batch_size=64, scaler=None, save_path=None, save_fname='y_hat_ensemble_scores.npz',
                 return_lr=False, device='GPU'):
        self.kw = dict(trainer=trainer, array=array, scale=scale, n_members=n_members, y_true=y_true, quantiles=quantiles,
                       seed=seed, fair=fair, mask=mask, array_in_hr=array_in_hr, static_vars=static_vars, predictors=predictors,
                       time_window=time_window, time_metadata=time_metadata, interpolation=interpolation, batch_size=batch_size,
                       scaler=scaler, save_path=save_path, save_fname=save_fname, return_lr=return_lr, device=device)

    def run(self):
        return verify_ensemble(**self.kw)


class ExceedanceVerifier:
    """``EnsembleVerifier`` for exceedance probabilities: same constructor-then-``.run()`` shape, runs ``verify_exceedance``."""

    def __init__(self, trainer, array, scale, n_members, thresholds, y_true=None, seed=None, mask=None, array_in_hr=False,
                 static_vars=None, predictors=None, time_window=None, time_metadata=None, interpolation='inter_area', batch_size=64,
                 scaler=None, save_path=None, save_fname='y_hat_exceedance.npz', return_lr=False, device='GPU'):
        self.kw = dict(trainer=trainer, array=array, scale=scale, n_members=n_members, thresholds=thresholds, y_true=y_true,
                       seed=seed, mask=mask, array_in_hr=array_in_hr, static_vars=static_vars, predictors=predictors,
                       time_window=time_window, time_metadata=time_metadata, interpolation=interpolation, batch_size=batch_size,
                       scaler=scaler, save_path=save_path, save_fname=save_fname, return_lr=return_lr, device=device)

    def run(self):
        return verify_exceedance(**self.kw)


class NeighbourhoodVerifier:
    """``EnsembleVerifier`` for neighbourhood probabilities: same constructor-then-``.run()`` shape, runs ``verify_neighbourhood``."""

    def __init__(self, trainer, array, scale, n_members, thresholds, windows=NEIGHBOURHOOD_DEFAULT_WINDOWS, y_true=None, seed=None,
                 mask=None, array_in_hr=False, static_vars=None, predictors=None, time_window=None, time_metadata=None,
                 interpolation='inter_area', batch_size=64, scaler=None, save_path=None, save_fname='y_hat_neighbourhood.npz',
                 return_lr=False, device='GPU'):
        self.kw = dict(trainer=trainer, array=array, scale=scale, n_members=n_members, thresholds=thresholds, windows=windows,
                       y_true=y_true, seed=seed, mask=mask, array_in_hr=array_in_hr, static_vars=static_vars, predictors=predictors,
                       time_window=time_window, time_metadata=time_metadata, interpolation=interpolation, batch_size=batch_size,
                       scaler=scaler, save_path=save_path, save_fname=save_fname, return_lr=return_lr, device=device)

    def run(self):
        return verify_neighbourhood(**self.kw)


class MultivariateVerifier:
    """``EnsembleVerifier`` for the energy and variogram scores: same constructor-then-``.run()`` shape, runs
    ``verify_multivariate``."""

    def __init__(self, trainer, array, scale, n_members, y_true=None, seed=None, max_lag=4, order=0.5, lag_weights='inverse',
                 fair=False, weights=None, mask=None, array_in_hr=False, static_vars=None, predictors=None, time_window=None,
                 time_metadata=None, interpolation='inter_area', batch_size=64, scaler=None, save_path=None,
                 save_fname='y_hat_multivariate.npz', return_lr=False, device='GPU'):
        self.kw = dict(trainer=trainer, array=array, scale=scale, n_members=n_members, y_true=y_true, seed=seed, max_lag=max_lag,
                       order=order, lag_weights=lag_weights, fair=fair, weights=weights, mask=mask, array_in_hr=array_in_hr,
                       static_vars=static_vars, predictors=predictors, time_window=time_window, time_metadata=time_metadata,
                       interpolation=interpolation, batch_size=batch_size, scaler=scaler, save_path=save_path,
                       save_fname=save_fname, return_lr=return_lr, device=device)

    def run(self):
        return verify_multivariate(**self.kw)
