"""The chunked upload loops of the verification scores (metrics.py) and of the time-axis scores (indices.py, postprocessing.py,
temporal.py, extremes.py): host arrays go to the device in chunks of whole units, one library call per chunk, the chunk's outputs
come back into their slice of the host result; the rule for ``batch_size``; and the argument checks the time-axis scores share."""
from types import SimpleNamespace

import numpy as np

from .device import Buffers


def is_int(v):
    return isinstance(v, (int, np.integer)) and not isinstance(v, (bool, np.bool_))


def check_batch_size(batch_size, integers_only=False):
    """``batch_size`` must be None or a positive integer.  An integral float such as 4.0 passes too, unless ``integers_only``: the
    ensemble entries have always refused it, the paired-field scores have always taken it."""
    if batch_size is None:
        return
    whole = is_int(batch_size) if integers_only else int(batch_size) == batch_size
    if not whole or batch_size < 1:
        raise ValueError(f'`batch_size` must be a positive integer, got {batch_size!r}')


def upload_batch(batch_size, per, count):
    """Units per upload out of `count`, `per` floats each: ``batch_size``, by default chunks of at most 256 MiB per array."""
    return max(min(int(max(1, (1 << 26) // per) if batch_size is None else batch_size), count), 1)


def is_device(a):
    from .device import DeviceArray
    return isinstance(a, DeviceArray)


def as_4d(a, name='x'):
    """-> (the array, its shape as (N, H, W, C)): an ndarray of any dtype (3-D input gets a channel axis) or a float32 DeviceArray,
    which is left as it is (a 3-D one is read as (N, H, W, 1))."""
    if is_device(a):
        if a.dtype != np.float32:
            raise TypeError(f'`{name}`: a DeviceArray must hold float32, got {a.dtype}')
        return a, tuple(a.shape) + ((1,) if len(a.shape) == 3 else ())
    from .dataloader import checkarray_ndim
    a = checkarray_ndim(np.asarray(getattr(a, 'values', a)), 4, -1)
    return a, a.shape


def check_4d_shape(shape, name=None):
    """-> ``shape`` as a tuple of ints; refuses what is not a non-empty (N, H, W, C)"""
    shape = tuple(int(v) for v in shape)
    if len(shape) != 4 or min(shape) < 1:
        raise ValueError(f'expected a non-empty (N, H, W, C) array{f" for `{name}`" if name else ""}, got shape {shape}')
    return shape


def numeric_array(v, message):
    """``v`` (or its ``.values``) as an array of floats or integers; anything else is refused with ``message``"""
    a = np.asarray(getattr(v, 'values', v))
    if a.dtype == object or not (np.issubdtype(a.dtype, np.floating) or np.issubdtype(a.dtype, np.integer)):
        raise ValueError(message)
    return a


def masked(x, mask, what='array'):
    """``x`` with the cells that ``mask`` excludes set to NaN (a float32 copy); ``x`` itself without a mask.  A DeviceArray cannot
    take one."""
    if mask is None:
        return x
    if is_device(x):
        raise ValueError(f'`mask` needs a host {what}: mark the excluded cells of a DeviceArray with NaN')
    from .metrics import _masked_observation
    return _masked_observation(x, mask)


def cell_bands(x, pred, shape, outputs, call, batch_size=None, fields=(), dtype=np.float32):
    """Runs ``call`` over the grid cells of ``x`` of ``shape`` (N, H, W, C), a score along the time axis: one library call over
    all per = H*W*C cells of a DeviceArray, which is used where it lies; a host array (any dtype) goes up in bands of
    ``upload_batch`` grid rows with the whole time axis, as contiguous ``dtype`` (float32 or float64), cell c of sample n of the
    band at [n*cells + c].  ``pred`` is a second input of the same kind, or None.

    * ``outputs``: host arrays [...][per], or None for an output that is not wanted (nothing is allocated for it).  Their device
      buffers are allocated once, at the widest band; after each call the band's [...][cells] is downloaded from the front of the
      buffer into the columns [..., c0:c0 + cells] of the host array.
    * ``fields``: side inputs.  A per-cell one, (..., H, W, C), is cut and uploaded per band as [...][cells]; any other is uploaded
      once; an empty one is not uploaded at all (its pointer is None).
    * ``call(band)`` makes the library call for ``band.cells`` cells from cell ``band.c0`` on: ``band.x``, ``band.pred``,
      ``band.fields`` and ``band.outs`` are the device pointers (None where there is nothing), ``band.buf`` is a buffer scope that
      lives as long as the band, for what a second call needs.

    Bands run in ascending order; every device buffer is freed on the way out."""
    N, H, W, C = shape
    row, dtype, device = W * C, np.dtype(dtype), is_device(x)
    bmax = H if device else upload_batch(batch_size, N * row * (dtype.itemsize // 4), H)
    wide = bmax * row

    def ptr(d):
        return d.ptr if d is not None else None
    with Buffers() as buf:
        dx = buf.alloc((N * wide,), dtype) if not device else x
        dp = (buf.alloc((N * wide,), dtype) if not device else pred) if pred is not None else None
        devs = [buf.alloc(h.shape[:-1] + (wide,), h.dtype) if h is not None else None for h in outputs]
        dfs = []
        for f in fields:
            assert f.ndim < 3 or f.shape[-3:] == (H, W, C), (f.shape, shape)           # a per-cell field lies on the grid
            d = buf.alloc(f.shape[:-3] + (wide,) if f.ndim >= 3 else f.shape, f.dtype) if f.size else None
            if d is not None and f.ndim < 3:
                d.upload(np.ascontiguousarray(f))
            dfs.append(d)
        for i in range(0, H, bmax):
            b = min(bmax, H - i)
            cells, c0 = b * row, i * row
            if not device:
                dx.upload(np.ascontiguousarray(x[:, i:i + b], dtype))
                if dp is not None:
                    dp.upload(np.ascontiguousarray(pred[:, i:i + b], dtype))
            for f, d in zip(fields, dfs):
                if d is not None and f.ndim >= 3:
                    d.upload(np.ascontiguousarray(f[..., i:i + b, :, :]))
            with Buffers() as scope:
                call(SimpleNamespace(x=dx.ptr, pred=ptr(dp), cells=cells, c0=c0, fields=[ptr(d) for d in dfs],
                                     outs=[ptr(d) for d in devs], buf=scope))
            for h, d in zip(outputs, devs):
                if d is None:
                    continue
                part = h[..., c0:c0 + cells]                            # contiguous for a 1-D output and for a single band
                if part.flags.c_contiguous:
                    d.download(part)
                else:
                    part = np.empty(part.shape, h.dtype)
                    d.download(part)
                    h[..., c0:c0 + cells] = part


def paired_chunks(obs, pred, outputs, call, batch_size=None, axis=0):
    """Runs ``call`` over the chunks of a float32 observation and its prediction (any dtype, or None: nothing is uploaded for it).
    A unit is one index of ``axis``: a sample (axis 0) or, for segments that run over the samples, a row of the grid (axis 1); a
    chunk is ``upload_batch`` consecutive units, copied into contiguous float32 and uploaded.  ``call(b, obs_ptr, pred_ptr,
    *output_ptrs)`` makes the library call for a chunk of ``b`` units (``pred_ptr`` is None without a prediction).  Every host
    array of ``outputs`` has the same number of rows per unit on its leading axis; the rows of a chunk are downloaded from the
    front of that output's device buffer.  Chunks run in ascending order; all device buffers are freed on the way out."""
    units = obs.shape[axis]
    per = obs.size // units
    bmax = upload_batch(batch_size, per, units)
    index = (slice(None),) * axis
    with Buffers() as buf:
        dy = buf.alloc((bmax * per,))
        dp = buf.alloc((bmax * per,)) if pred is not None else None
        devs = [buf.alloc((bmax * (host.shape[0] // units),) + host.shape[1:], host.dtype) for host in outputs]
        for i in range(0, units, bmax):
            b = min(bmax, units - i)
            chunk = index + (slice(i, i + b),)
            dy.upload(np.ascontiguousarray(obs[chunk], np.float32))
            if dp is not None:
                dp.upload(np.ascontiguousarray(pred[chunk], np.float32))
            call(b, dy.ptr, dp.ptr if dp is not None else None, *(d.ptr for d in devs))
            for host, dev in zip(outputs, devs):
                rows = host.shape[0] // units
                part = host[i * rows:(i + b) * rows]
                if part.nbytes:
                    dev.download(part)


def host_ensemble(obs, members, make_scorer, batch_size=None):
    """Scores ``members`` (K,) + obs.shape, of any dtype, against the float32 observation ``obs`` in chunks of whole samples: each
    chunk's members go into one device stack, its observation next to it, and ``scorer.score`` runs while both are resident.
    ``make_scorer(bmax)`` builds the scorer (ensemble_score.py) for chunks of at most ``bmax`` samples.  -> ``scorer.result()``."""
    K, N = members.shape[0], obs.shape[0]
    per = int(np.prod(obs.shape[1:], dtype=np.int64))
    bmax = upload_batch(batch_size, max(K * per, 1), N)
    stride = bmax * per
    with Buffers() as buf:
        scorer, stack, dev_obs = buf.own(make_scorer(bmax)), buf.alloc((K, stride)), buf.alloc((stride,))
        for i in range(0, N, bmax):
            b = min(bmax, N - i)
            for k in range(K):
                stack.upload(np.ascontiguousarray(members[k, i:i + b], np.float32), k * stride)
            dev_obs.upload(obs[i:i + b])
            scorer.score(stack.ptr, stride, dev_obs.ptr, i, b)
        return scorer.result()
