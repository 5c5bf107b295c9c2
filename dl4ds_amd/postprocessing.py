"""Quantile-mapping bias correction of predictions on the MI355X (csrc/qmap.hip).

The reference has no counterpart: where its users find a per-cell distribution bias (`metrics.quantile_maps`) they leave for numpy
or xarray.  ``QuantileMapper`` is the fit / transform object for it, in the shape of the scalers of `preprocessing`: ``fit``
builds, per grid cell and channel, the sample quantiles of the observation and of the model's historical run on the device (one
segmented sort per array), ``transform`` maps every value of a prediction from the model's distribution onto the observed one in
one streaming pass.  Empirical quantile mapping (``method='eqm'``) and its trend-preserving form, quantile delta mapping
(``'qdm'``, Cannon et al. 2015), additive (``kind='+'``) or multiplicative (``'*'``).  numpy in / numpy out; a
``dl4ds_amd.device.DeviceArray`` is used where it lies and ``transform`` then returns a DeviceArray.
"""
import numpy as np

from ._chunks import as_4d as _as_4d, cell_bands, check_4d_shape, check_batch_size, is_device as _is_device, masked, paired_chunks
from .preprocessing import NotFittedError

__all__ = ['QuantileMapper', 'quantile_map', 'check_qmap_args', 'QMAP_MIN_QUANTILES', 'QMAP_MAX_QUANTILES']

QMAP_MIN_QUANTILES, QMAP_MAX_QUANTILES = 2, 256        # caps of dl4ds_quantile_table / dl4ds_qmap_apply
QMAP_LENGTH_BOUND = 1 << 31
_METHODS, _KINDS = ('eqm', 'qdm'), ('+', '*')
COUNT_NAMES = ('n_nonfinite', 'n_unfitted', 'n_below', 'n_above')


def _check_shape(name, shape):
    if shape is None:
        return None
    shape = check_4d_shape(shape, name)
    if shape[0] >= QMAP_LENGTH_BOUND:
        raise ValueError(f'`{name}` has {shape[0]} samples: the number must stay below 2^31')
    return shape


def check_qmap_args(n_quantiles=101, quantiles=None, method='eqm', kind='+', batch_size=None, obs_shape=None, model_shape=None,
                    x_shape=None, grid=None, fitted=True):
    """Validation of `QuantileMapper` (no library call) -> the probabilities as float64 (Q,).  ``obs_shape`` / ``model_shape``:
    the two arrays of ``fit``, (N, H, W, C) with one grid; ``x_shape``: the array of ``transform``, whose grid must be ``grid``,
    the fitted (H, W, C); ``fitted=False`` stands for ``transform`` before ``fit`` (NotFittedError)."""
    if method not in _METHODS:
        raise ValueError(f"`method` must be 'eqm' or 'qdm', got {method!r}")
    if kind not in _KINDS:
        raise ValueError(f"`kind` must be '+' (additive) or '*' (multiplicative), got {kind!r}")
    check_batch_size(batch_size)
    if quantiles is None:
        if isinstance(n_quantiles, (bool, np.bool_)) or not isinstance(n_quantiles, (int, np.integer)):
            raise ValueError(f'`n_quantiles` must be an integer, got {n_quantiles!r}')
        if not QMAP_MIN_QUANTILES <= n_quantiles <= QMAP_MAX_QUANTILES:
            raise ValueError(f'between {QMAP_MIN_QUANTILES} and {QMAP_MAX_QUANTILES} quantiles are supported, got {n_quantiles}')
        q = np.linspace(0.0, 1.0, int(n_quantiles))
    else:
        q = np.asarray(quantiles, np.float64)
        if q.ndim != 1:
            raise ValueError('`quantiles` must be a 1-D sequence')
        if not QMAP_MIN_QUANTILES <= q.size <= QMAP_MAX_QUANTILES:
            raise ValueError(f'between {QMAP_MIN_QUANTILES} and {QMAP_MAX_QUANTILES} quantiles are supported, got {q.size}')
        if not ((q >= 0.0) & (q <= 1.0)).all():                        # NaN compares false
            raise ValueError('`quantiles` must lie in [0, 1]')
        if not (np.diff(q) > 0.0).all():
            raise ValueError('`quantiles` must be strictly increasing')
    obs_shape, model_shape, x_shape = (_check_shape(n, s) for n, s in (('obs', obs_shape), ('model', model_shape), ('x', x_shape)))
    if obs_shape is not None and model_shape is not None and obs_shape[1:] != model_shape[1:]:
        raise ValueError(f'`obs` and `model` must share their grid (H, W, C), got {obs_shape[1:]} and {model_shape[1:]}')
    if x_shape is not None:
        if not fitted:
            raise NotFittedError("This QuantileMapper instance is not fitted yet. Call 'fit' with appropriate arguments before "
                                 'using this estimator.')
        if grid is not None and x_shape[1:] != tuple(grid):
            raise ValueError(f'`x` has the grid {x_shape[1:]}, the mapper was fitted on {tuple(grid)}')
    return np.ascontiguousarray(q)


def _device_table(x, shape, q, batch_size=None):
    """(table float32 (Q, H, W, C), valid int64 (H, W, C)) of the array ``x`` of ``shape`` (N, H, W, C): a DeviceArray in one call,
    a host array in bands of grid rows."""
    from . import _lib
    lib = _lib.lib()
    N, H, W, C = shape
    Q = len(q)
    table, valid = np.empty((Q, H * W * C), np.float32), np.empty((H * W * C,), np.int64)
    cell_bands(x, None, shape, (table, valid),
               lambda band: _lib.check(lib.dl4ds_quantile_table(band.x, N, band.cells, q.ctypes.data, Q, *band.outs)), batch_size)
    return table.reshape(Q, H, W, C), valid.reshape(H, W, C)


class QuantileMapper:
    """Quantile mapping per grid cell and channel.  ``fit(obs, model)`` takes the observation (N_o, H, W, C) and the model's
    historical run (N_m, H, W, C) over the same period and grid; ``transform(x)`` corrects a prediction (N, H, W, C).

    * ``n_quantiles`` / ``quantiles``: the probabilities of the tables, by default ``np.linspace(0, 1, n_quantiles)``; between 2
      and 256, strictly increasing, in [0, 1].
    * ``method='eqm'``: a value is located in the model's table and read off the observed one, linearly between knots; beyond the
      two ends the correction of the end knot is kept.  ``'qdm'``: the value is located in the table of ``x`` itself (fitted by
      ``transform``), and the change between the model's historical quantile and the value is carried onto the observed quantile.
    * ``kind='+'``: corrections are differences (temperature); ``'*'``: ratios (precipitation), with the observed quantile taken
      where the model's is 0.
    * A cell without a finite value in a table is unfitted: its output is NaN, or the input with ``keep_unfitted``.  Non-finite
      inputs pass through.  ``diagnostics_`` counts both, and the values below / at or above the search table's ends.
    * Host arrays are uploaded in chunks of at most 256 MiB (``batch_size``: grid rows per upload in ``fit``, samples in
      ``transform``); the result does not depend on it.

    Fitted attributes: ``quantiles_`` float64 (Q,), ``obs_quantiles_`` / ``model_quantiles_`` float32 (Q, H, W, C), ``n_obs_`` /
    ``n_model_`` int64 (H, W, C), the numbers of finite values per cell."""

    def __init__(self, n_quantiles=101, quantiles=None, method='eqm', kind='+', keep_unfitted=False, batch_size=None):
        self.n_quantiles = n_quantiles
        self.quantiles = quantiles
        self.method = method
        self.kind = kind
        self.keep_unfitted = keep_unfitted
        self.batch_size = batch_size

    def _check(self, **shapes):
        return check_qmap_args(self.n_quantiles, self.quantiles, self.method, self.kind, self.batch_size, **shapes)

    @classmethod
    def from_tables(cls, quantiles, obs_quantiles, model_quantiles, n_obs, n_model, **params):
        """A fitted mapper from tables made elsewhere (no library call)."""
        self = cls(quantiles=np.asarray(quantiles, np.float64), **params)
        self.quantiles_ = self._check()
        self.obs_quantiles_, self.model_quantiles_ = np.asarray(obs_quantiles, np.float32), np.asarray(model_quantiles, np.float32)
        self.n_obs_, self.n_model_ = np.asarray(n_obs, np.int64), np.asarray(n_model, np.int64)
        want = (len(self.quantiles_),) + self.n_obs_.shape
        if self.n_obs_.ndim != 3 or self.n_model_.shape != self.n_obs_.shape or self.obs_quantiles_.shape != want \
                or self.model_quantiles_.shape != want:
            raise ValueError(f'expected tables of shape (Q, H, W, C) = {want} and counts of shape (H, W, C)')
        return self

    def fit(self, obs, model, mask=None):
        (obs, obs_shape), (model, model_shape) = _as_4d(obs, 'obs'), _as_4d(model, 'model')
        q = self._check(obs_shape=obs_shape, model_shape=model_shape)
        obs = masked(obs, mask, 'observation')                          # (a copy; without a mask the bands are cut from the caller's array)
        self.obs_quantiles_, self.n_obs_ = _device_table(obs, obs_shape, q, self.batch_size)
        self.model_quantiles_, self.n_model_ = _device_table(model, model_shape, q, self.batch_size)
        self.quantiles_ = q
        return self

    def transform(self, x):
        from . import _lib
        from .device import Buffers, DeviceArray
        x, shape = _as_4d(x, 'x')
        fitted = hasattr(self, 'quantiles_')
        self._check(x_shape=shape, grid=self.n_obs_.shape if fitted else None, fitted=fitted)
        q = self.quantiles_
        lib = _lib.lib()
        N, per, Q = shape[0], int(np.prod(shape[1:], dtype=np.int64)), len(q)
        kind, keep = _KINDS.index(self.kind), int(bool(self.keep_unfitted))
        target = _device_table(x, shape, q, self.batch_size)[0] if self.method == 'qdm' else None
        with Buffers() as buf:
            dm, do = buf.own(DeviceArray.from_numpy(self.model_quantiles_)), buf.own(DeviceArray.from_numpy(self.obs_quantiles_))
            df = buf.own(DeviceArray.from_numpy(target)) if target is not None else None
            counts = buf.zeros((4,), np.uint64)

            def call(b, dx, _, dout):
                _lib.check(lib.dl4ds_qmap_apply(dx, dout, b, per, dm.ptr, do.ptr, df.ptr if df is not None else None, Q, kind, keep,
                                                counts.ptr))
            if _is_device(x):
                out = DeviceArray(shape)
                try:
                    call(N, x.ptr, None, out.ptr)
                except Exception:
                    out.free()
                    raise
            else:
                out = np.empty(shape, np.float32)
                paired_chunks(x, None, (out,), call, self.batch_size, axis=0)
            self.diagnostics_ = {k: int(v) for k, v in zip(COUNT_NAMES, counts.numpy())}
        return out

    def fit_transform(self, obs, model, mask=None):
        """Fits on (obs, model) and corrects the historical model run."""
        return self.fit(obs, model, mask=mask).transform(model)

    def save(self, path):
        """The fitted tables and the parameters into one ``.npz``."""
        if not hasattr(self, 'quantiles_'):
            self._check(x_shape=(1, 1, 1, 1), fitted=False)
        np.savez(path, quantiles=self.quantiles_, obs_quantiles=self.obs_quantiles_, model_quantiles=self.model_quantiles_,
                 n_obs=self.n_obs_, n_model=self.n_model_, method=np.array(self.method), kind=np.array(self.kind),
                 keep_unfitted=np.array(bool(self.keep_unfitted)))

    @classmethod
    def load(cls, path):
        with np.load(path, allow_pickle=False) as z:
            return cls.from_tables(z['quantiles'], z['obs_quantiles'], z['model_quantiles'], z['n_obs'], z['n_model'],
                                   method=str(z['method']), kind=str(z['kind']), keep_unfitted=bool(z['keep_unfitted']))


def quantile_map(obs, model, x, mask=None, **kw):
    """``QuantileMapper(**kw).fit(obs, model, mask).transform(x)`` in one call."""
    return QuantileMapper(**kw).fit(obs, model, mask=mask).transform(x)
