"""MinMaxScaler and StandardScaler of the reference's preprocessing.py on the MI355X (csrc/scaler.hip).

Same names, parameter order and defaults as the reference.  ``fit`` is one NaN-skipping pass over the array on the device (min, max,
mean, population std per kept cell, the NaN mask as one bit per element); ``transform`` / ``inverse_transform`` are one streaming
pass whose arithmetic is rounded operation by operation like numpy's in-place ``*=``, ``+=``, ``-=``, ``/=``.  numpy in / numpy
out; a ``dl4ds_amd.device.DeviceArray`` is used where it lies and the two transforms then return a DeviceArray.  An object with a
``.values`` ndarray (xarray's DataArray) is read through it; xarray out and dimension names as ``axis`` are not supported.
"""
import ctypes
import inspect

import numpy as np

__all__ = ['MinMaxScaler', 'StandardScaler', 'NotFittedError']

_OP_NONE, _OP_MUL, _OP_ADD, _OP_SUB, _OP_DIV = range(5)
_NAN_FILL, _NAN_MASK = 0, 1


class NotFittedError(ValueError, AttributeError):
    """transform / inverse_transform before fit (what scikit-learn's NotFittedError is)."""


def _is_device(X):
    from .device import DeviceArray
    return isinstance(X, DeviceArray)


def _squeezed(shape):
    return tuple(int(s) for s in shape if s != 1)


def _as_input(X):
    """-> (ndarray or DeviceArray).  TypeError for anything that is not float32 / float64 array data."""
    if not isinstance(X, np.ndarray):
        if type(X).__module__.startswith('dl4ds_amd.') and _is_device(X):
            if X.dtype not in (np.float32, np.float64):
                raise TypeError(f'scalers work on float32 or float64 data, got {X.dtype}')
            return X
        v = getattr(X, 'values', None)
        if not isinstance(v, np.ndarray):
            raise TypeError('`X` is neither a np.ndarray or xr.DataArray')
        X = v
    if X.dtype not in (np.float32, np.float64):
        raise TypeError(f'scalers work on float32 or float64 data, got {X.dtype}')
    return X


def _reduce_flags(ndim, axis):
    if axis is None:
        return [1] * ndim
    axes = axis if isinstance(axis, (tuple, list)) else (axis,)
    flags = [0] * ndim
    for a in axes:
        if not isinstance(a, (int, np.integer)):
            raise TypeError('`axis` must be None, an int or a tuple of ints (dimension names are not supported)')
        if not -ndim <= a < ndim:
            raise np.exceptions.AxisError(int(a), ndim) if hasattr(np, 'exceptions') else ValueError(f'axis {a} out of bounds')
        if flags[a % ndim]:
            raise ValueError('duplicate value in `axis`')
        flags[a % ndim] = 1
    return flags


def _c_shape(shape, flags):
    n = len(shape)
    return (ctypes.c_size_t * max(n, 1))(*shape), (ctypes.c_int * max(n, 1))(*flags), n


class _DeviceScaler:
    """The parts both scalers share: parameters, upload, the two device calls, the bit mask."""

    # ---- scikit-learn's BaseEstimator surface, restated
    def get_params(self, deep=True):
        names = [p for p in inspect.signature(type(self).__init__).parameters if p != 'self']
        return {k: getattr(self, k) for k in names}

    def set_params(self, **params):
        valid = self.get_params()
        for k, v in params.items():
            if k not in valid:
                raise ValueError(f'Invalid parameter {k!r} for estimator {type(self).__name__}. Valid parameters are: {sorted(valid)}.')
            setattr(self, k, v)
        return self

    def fit_transform(self, X, y=None, **fit_params):
        return self.fit(X, **fit_params).transform(X)

    def fit(self, X, y=None):
        self._reset()
        return self.partial_fit(X, y)

    # ---- NaN mask: kept on the device as one bit per element
    @property
    def nan_mask(self):
        m = self.__dict__.get('_mask_bits')
        if m is None:
            raise AttributeError(f'{type(self).__name__!r} object has no attribute \'nan_mask\'')
        shape = self._mask_shape
        n = int(np.prod(shape, dtype=np.int64))
        bits = np.unpackbits(m.numpy().view(np.uint8), bitorder='little')[:n]
        return bits.astype(bool).reshape(shape)

    # ---- device plumbing
    def _stats(self, X):
        """One pass over X (ndarray or DeviceArray): -> dict of keepdims statistics in X's dtype; sets the mask if X holds a NaN."""
        from . import _lib
        from .device import DeviceArray
        X = _as_input(X)
        shape = _squeezed(X.shape)
        flags = _reduce_flags(len(shape), self.axis)
        if int(np.prod(shape, dtype=np.int64)) == 0:
            raise ValueError('zero-size array to reduction operation fmin which has no identity')
        dX = X if _is_device(X) else DeviceArray.from_numpy(X)
        cshape, cflags, nd = _c_shape(shape, flags)
        lib = _lib.lib()
        cells = ctypes.c_size_t(0)
        _lib.check(lib.dl4ds_scaler_cells(cshape, nd, cflags, ctypes.byref(cells)))
        n = int(np.prod(shape, dtype=np.int64))
        out = DeviceArray((5, cells.value), np.float64)
        flag = DeviceArray((1,), np.uint32)
        bits = DeviceArray(((n + 31) // 32,), np.uint32)
        _lib.check(lib.dl4ds_scaler_stats(dX.ptr, int(X.dtype == np.float64), cshape, nd, cflags, out.ptr, flag.ptr, bits.ptr))
        st = out.numpy()
        if int(flag.numpy()[0]):
            self._mask_bits, self._mask_shape = bits, shape
        keep = tuple(1 if f else s for s, f in zip(shape, flags))
        names = ('count', 'min', 'max', 'mean', 'std')
        return {k: (st[i].reshape(keep) if k == 'count' else st[i].astype(X.dtype).reshape(keep)) for i, k in enumerate(names)}

    def _apply(self, X, op1, a, op2, b, nan_mode):
        from . import _lib
        from .device import DeviceArray
        X = _as_input(X)
        shape = _squeezed(X.shape)
        dt = X.dtype
        mask = self.__dict__.get('_mask_bits') if nan_mode == _NAN_MASK else None
        if mask is not None and shape != self._mask_shape:
            raise IndexError(f'boolean index did not match indexed array: the array has shape {shape} but the fitted nan_mask '
                             f'has shape {self._mask_shape}')
        cell_shape = None
        for st in (a, b):
            if st is not None:
                st_shape = np.shape(st)
                if len(st_shape) > len(shape):
                    raise ValueError(f'operands could not be broadcast together with shapes {shape} {st_shape}')
                st_shape = (1,) * (len(shape) - len(st_shape)) + tuple(st_shape)
                if any(k != 1 and k != s for k, s in zip(st_shape, shape)):
                    raise ValueError(f'operands could not be broadcast together with shapes {shape} {st_shape}')
                cell_shape = st_shape if cell_shape is None else tuple(max(p, q) for p, q in zip(cell_shape, st_shape))
        flags = [1] * len(shape) if cell_shape is None else [int(k == 1) for k in cell_shape]
        cshape, cflags, nd = _c_shape(shape, flags)
        keep = tuple(1 if f else s for s, f in zip(shape, flags))

        def operand(st):
            if st is None:
                return None
            return DeviceArray.from_numpy(np.ascontiguousarray(np.broadcast_to(np.asarray(st, dt).reshape(
                (1,) * (len(shape) - np.ndim(st)) + np.shape(st)), keep)))
        da, db = operand(a), operand(b)
        on_device = _is_device(X)
        if on_device:
            dX = X
            dOut = DeviceArray(shape, dt) if self.copy else X
        else:
            dX = dOut = DeviceArray.from_numpy(X)
        _lib.check(_lib.lib().dl4ds_scaler_apply(dX.ptr, dOut.ptr, int(dt == np.float64), cshape, nd, cflags,
                                                 op1 if da is not None else _OP_NONE, da.ptr if da is not None else None,
                                                 op2 if db is not None else _OP_NONE, db.ptr if db is not None else None,
                                                 nan_mode, float(self.fillnanto), mask.ptr if mask is not None else None))
        if on_device:
            if dOut is X:
                X.shape = shape
            return dOut
        if not self.copy and X.flags.c_contiguous and X.flags.writeable:
            res = X.reshape(shape)                      # a view of the caller's buffer
            _lib.check(_lib.lib().dl4ds_memcpy_d2h(res.ctypes.data, dOut.ptr, dOut.nbytes))
            return res
        return dOut.numpy().reshape(shape)


class MinMaxScaler(_DeviceScaler):
    """Transform data to ``value_range`` (preprocessing.py:9-167): ``X * scale_ + min_`` with the minimum and maximum taken over
    ``axis`` (NaNs disregarded), NaNs then replaced by ``fillnanto``."""

    def __init__(self, value_range=(0, 1), copy=True, axis=None, fillnanto=-1):
        self.value_range = value_range
        self.copy = copy
        self.fillnanto = fillnanto
        self.axis = axis

    def _reset(self):
        if hasattr(self, 'scale_'):
            del self.scale_
            del self.min_
            del self.data_min_
            del self.data_max_
            del self.data_range_

    def partial_fit(self, X, y=None):
        value_range = self.value_range
        if value_range[0] >= value_range[1]:
            raise ValueError('Minimum of desired value_range must be smaller than maximum. Got %s.' % str(value_range))
        st = self._stats(X)
        data_min, data_max = st['min'], st['max']
        data_range = data_max - data_min
        scale = data_range.copy()                                   # scikit-learn's _handle_zeros_in_scale
        scale[scale < 10 * np.finfo(scale.dtype).eps] = 1.0
        self.scale_ = (value_range[1] - value_range[0]) / scale
        self.min_ = value_range[0] - data_min * self.scale_
        self.data_min_ = data_min
        self.data_max_ = data_max
        self.data_range_ = data_range
        return self

    def _check_fitted(self):
        if not hasattr(self, 'scale_'):
            raise NotFittedError("This MinMaxScaler instance is not fitted yet. Call 'fit' with appropriate arguments before "
                                 'using this estimator.')

    def transform(self, X):
        self._check_fitted()
        return self._apply(X, _OP_MUL, self.scale_, _OP_ADD, self.min_, _NAN_FILL)

    def inverse_transform(self, X):
        self._check_fitted()
        return self._apply(X, _OP_SUB, self.min_, _OP_DIV, self.scale_, _NAN_MASK)


class StandardScaler(_DeviceScaler):
    """Remove the mean and scale to unit variance over ``axis`` (preprocessing.py:170-334), NaNs disregarded in ``fit`` and
    replaced by ``fillnanto`` in ``transform``.  The reference's behaviour is kept as it is: ``transform`` subtracts the mean if
    and only if ``with_std`` (preprocessing.py:300)."""

    def __init__(self, copy=True, with_mean=True, with_std=True, axis=None, fillnanto=0):
        self.with_mean = with_mean
        self.with_std = with_std
        self.copy = copy
        self.axis = axis
        self.fillnanto = fillnanto

    def _reset(self):
        if hasattr(self, 'mean_'):
            del self.mean_
            del self.std_

    def partial_fit(self, X, y=None):
        st = self._stats(X)
        if self.with_mean:
            self.mean_ = st['mean']
        if self.with_std:
            self.std_ = st['std']
        return self

    def _check_fitted(self):
        if not any(k.endswith('_') and not k.startswith('_') for k in vars(self)):
            raise NotFittedError("This StandardScaler instance is not fitted yet. Call 'fit' with appropriate arguments before "
                                 'using this estimator.')

    def transform(self, X):
        self._check_fitted()
        if self.with_std:
            return self._apply(X, _OP_SUB, self.mean_, _OP_DIV, self.std_, _NAN_FILL)
        return self._apply(X, _OP_NONE, None, _OP_NONE, None, _NAN_FILL)

    def inverse_transform(self, X):
        self._check_fitted()
        return self._apply(X, _OP_MUL, self.std_ if self.with_std else None, _OP_ADD, self.mean_ if self.with_mean else None,
                           _NAN_MASK)
