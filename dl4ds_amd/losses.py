"""dl4ds/losses.py:5-149 on MI355X: callables with the reference signature ``loss(y_true, y_pred) -> float``.
Inside the trainers the fused loss+gradient kernels are selected by NAME; these wrappers exist for
stand-alone evaluation."""
import numpy as _np

from . import ops as _ops


def _make(kind):
    def f(y_true, y_pred):
        return _ops.loss(kind, y_true, y_pred, want_grad=False)[0]
    f.__name__ = kind
    f.__doc__ = f'{kind} (dl4ds/losses.py) evaluated by the gfx950 loss kernels'
    return f


mae = _make('mae')
mse = _make('mse')
dssim = _make('dssim')
dssim_mae = _make('dssim_mae')
dssim_mse = _make('dssim_mse')
dssim_mae_mse = _make('dssim_mae_mse')
msdssim = _make('msdssim')                       # losses.py:92-130 (tf.image.ssim_multiscale, four scales)
msdssim_mae = _make('msdssim_mae')               # losses.py:133-139
msdssim_mae_mse = _make('msdssim_mae_mse')       # losses.py:142-149

def check_loss_weights(weights, hr_shape, loss):
    """Validate a full-field loss-weight map for training on an HR grid and return it as a contiguous float32 array.

    weights: (H, W), (H, W, 1) or (H, W, C); hr_shape: (H, W) or (H, W, C) of the HR fields (longer shapes: their last three
    entries); loss: the loss name.  ValueError for a shape that does not fit, a NaN / Inf, a negative value, a map that is zero
    everywhere (no cell would be trained on) and for the multi-scale kinds, which have no weighted form.  Runs on the CPU."""
    name = loss if isinstance(loss, str) else getattr(loss, '__name__', str(loss))
    if name.startswith('msdssim'):
        raise ValueError(f'loss weights are not available for the multi-scale kind {name!r}')
    hr_shape = tuple(int(v) for v in hr_shape)
    if len(hr_shape) == 2:
        hr_shape = hr_shape + (1,)
    if len(hr_shape) < 3:
        raise ValueError(f'`hr_shape` must be (H, W) or (H, W, C), got {hr_shape}')
    h, w, c = hr_shape[-3:]
    a = _np.asarray(getattr(weights, 'values', weights))
    if a.dtype.kind not in 'fiub':
        raise ValueError(f'loss weights must be numeric, got dtype {a.dtype}')
    if not (a.shape == (h, w) or (a.ndim == 3 and a.shape[:2] == (h, w) and a.shape[2] in (1, c))):
        raise ValueError(f'loss weights of shape {a.shape} do not fit the HR grid: expected {(h, w)}, {(h, w, 1)} or {(h, w, c)}')
    a = _np.ascontiguousarray(a, _np.float32)
    if not _np.isfinite(a).all():
        raise ValueError('loss weights must be finite (mask a cell with weight 0, not NaN)')
    if (a < 0).any():
        raise ValueError('loss weights must be >= 0')
    if not (a > 0).any():
        raise ValueError('loss weights are zero everywhere: no grid cell would enter the loss')
    return a


def latitude_weights(lat_degrees, n_lon):
    """cos(latitude) area weights of a regular lat-lon grid: an (H, W) float32 map whose row y is cos(lat_degrees[y]), clipped at 0
    (|lat| >= 90 gets no weight)."""
    lat = _np.asarray(getattr(lat_degrees, 'values', lat_degrees), _np.float64).reshape(-1)
    if not _np.isfinite(lat).all():
        raise ValueError('`lat_degrees` must be finite')
    row = _np.clip(_np.cos(_np.deg2rad(lat)), 0.0, None)
    return _np.ascontiguousarray(_np.repeat(row[:, None], int(n_lon), axis=1), _np.float32)


__all__ = ['check_loss_weights', 'latitude_weights', 'mae', 'mse', 'dssim', 'dssim_mae', 'dssim_mse', 'dssim_mae_mse', 'msdssim', 'msdssim_mae', 'msdssim_mae_mse']
