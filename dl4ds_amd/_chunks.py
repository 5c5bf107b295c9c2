"""The chunked upload loops of the verification scores (metrics.py): host arrays go to the device in chunks of whole units, one
library call per chunk, the chunk's outputs come back into their slice of the host result; and the rule for ``batch_size``."""
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
