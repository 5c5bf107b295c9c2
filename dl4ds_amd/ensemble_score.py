"""Device-side verification of an ensemble against an observation (csrc/ensemble_score.hip): the accumulators
and the per-batch call shared by ``Model.score_ensemble`` (members produced on the device) and ``metrics.ensemble_scores`` (members
the caller already has on the host)."""
import ctypes

import numpy as np

from . import _lib

U64 = 0xFFFFFFFFFFFFFFFF


def check_score_args(fair, scale=None, sample_shape=None):
    """``fair`` must be a bool; ``scale`` None or something that broadcasts to one sample -> float32 array of ``sample_shape`` (or
    None).  Looks at its arguments only (no library, no device)."""
    if not isinstance(fair, (bool, np.bool_)):
        raise ValueError(f'`fair` must be True or False, got {fair!r}')
    if scale is None or sample_shape is None:
        return None
    try:
        s = np.broadcast_to(np.asarray(scale, np.float64), tuple(sample_shape))
    except ValueError:
        raise ValueError(f'`scale` of shape {np.shape(scale)} does not broadcast to one sample {tuple(sample_shape)}') from None
    return np.ascontiguousarray(s, np.float32)


def as_signed64(v):
    v = int(v) & U64
    return v - (1 << 64) if v >> 63 else v


class Scorer:
    """Accumulators of one verification run on the device.  ``score`` is called once per batch of whole samples while the batch's
    member stack is resident; ``result`` downloads the sums and takes the means in float64."""

    def __init__(self, n_members, n_samples, sample_shape, q32, fair, seed, scale, return_fields, bmax):
        from .device import DeviceArray
        self.lib = _lib.lib()
        self.K, self.N, self.sample_shape = int(n_members), int(n_samples), tuple(sample_shape)
        self.per = int(np.prod(self.sample_shape, dtype=np.int64))
        self.q = np.asarray(q32, np.float32)
        self.nq = len(self.q)
        self.qc = (ctypes.c_float * max(self.nq, 1))(*self.q.tolist())
        self.fair, self.seed = int(bool(fair)), as_signed64(0 if seed is None else seed)
        self.return_fields = bool(return_fields)
        self.bmax = int(bmax)
        self.n_cells_excluded = 0
        self.dev = dict(cell=DeviceArray.zeros((4, self.per), np.float64), hist=DeviceArray.zeros((self.K + 1,), np.uint64),
                        cov=DeviceArray.zeros((max(self.nq, 1),), np.uint64), sample=DeviceArray((self.bmax, 4), np.float64))
        if scale is not None:
            scale = np.ascontiguousarray(scale, np.float32).reshape(self.per)
            with np.errstate(invalid='ignore'):
                self.n_cells_excluded = int(np.count_nonzero(~(np.isfinite(scale) & (scale > 0))))
            self.dev['scale'] = DeviceArray.from_numpy(scale)
        self.sample_sums = np.zeros((self.N, 4), np.float64)
        self.fields = {}
        if self.return_fields:
            for k in ('crps', 'sqerr', 'var', 'rank'):
                self.dev[k] = DeviceArray((self.bmax * self.per,), np.int32 if k == 'rank' else np.float32)
                self.fields[k + '_field'] = np.empty((self.N,) + self.sample_shape, self.dev[k].dtype)

    def score(self, stack_ptr, stride, obs_ptr, first, b):
        """samples [first, first + b) of the run: their members at stack_ptr (member stride ``stride`` elements), their observation at
        obs_ptr"""
        lib, d = self.lib, self.dev
        m = b * self.per
        ptr = lambda k: d[k].ptr if k in d else None                                       # noqa: E731
        _lib.check(lib.dl4ds_ensemble_score(stack_ptr, self.K, m, stride, obs_ptr, b, first * self.per, ptr('scale'), self.fair,
                                            self.seed, self.qc, self.nq, ptr('crps'), ptr('sqerr'), ptr('var'), ptr('rank'), d['sample'].ptr,
                                            d['cell'].ptr, d['hist'].ptr, d['cov'].ptr))
        _lib.check(lib.dl4ds_memcpy_d2h(self.sample_sums[first:first + b].ctypes.data, d['sample'].ptr, b * 4 * 8))
        if self.return_fields:
            for k in ('crps', 'sqerr', 'var', 'rank'):
                _lib.check(lib.dl4ds_memcpy_d2h(self.fields[k + '_field'][first:first + b].ctypes.data, d[k].ptr, m * 4))

    def free(self):
        for a in self.dev.values():
            a.free()
        self.dev = {}

    def result(self):
        cell = self.dev['cell'].numpy()
        hist = self.dev['hist'].numpy().astype(np.int64)
        covered = self.dev['cov'].numpy()[:self.nq].astype(np.int64)
        s = self.sample_sums
        n_valid = int(round(s[:, 3].sum()))
        tot = s[:, :3].sum(axis=0)
        with np.errstate(invalid='ignore', divide='ignore'):
            mean = tot / n_valid if n_valid else np.full(3, np.nan)
            res = dict(crps=float(mean[0]), spread=float(np.sqrt(mean[2])), rmse=float(np.sqrt(mean[1])))
            res['spread_skill'] = float(np.float64(res['spread']) / np.float64(res['rmse']))
            per_sample = np.where(s[:, 3:4] > 0, s[:, :3] / s[:, 3:4], np.nan)
            res.update(crps_per_sample=per_sample[:, 0], spread_per_sample=np.sqrt(per_sample[:, 2]),
                       rmse_per_sample=np.sqrt(per_sample[:, 1]))
            maps = np.where(cell[3] > 0, cell[:3] / cell[3], np.nan).reshape((3,) + self.sample_shape)
            res.update(crps_map=maps[0], spread_map=np.sqrt(maps[2]), rmse_map=np.sqrt(maps[1]))
            res.update(rank_histogram=hist, covered=covered,
                       coverage=covered / np.float64(n_valid) if n_valid else np.full(self.nq, np.nan),
                       n_valid=n_valid, n_valid_per_sample=np.rint(s[:, 3]).astype(np.int64),
                       n_valid_map=np.rint(cell[3]).astype(np.int64).reshape(self.sample_shape),
                       sample_sums=s.copy(), cell_sums=cell.reshape((4,) + self.sample_shape),
                       n_cells_excluded=self.n_cells_excluded)
        res.update(self.fields)
        return res
