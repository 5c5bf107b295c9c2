"""Spearman rank correlation of compute_metrics on one GPU, one JSON line: N = 365 synthetic 512 x 512 x 1 precipitation-like
fields (about 60 % exact zeros, values rounded to 0.1: heavy ties).

* ``per_pair`` / ``per_grid_point``: dl4ds_spearman on device-resident arrays after warm-up.  ``device_ms``: the summed kernel
  time of the 'spearman' profiler scope (per-launch timestamps); ``wall_ms``: host time of the call bracketed by device syncs.
  ``bytes_min``: both inputs read once; ``bytes_engine``: what the engine's passes read and write (rank.hip / DESIGN.md
  section 10: the global radix engine moves 176 B per element of a pair, the LDS engine 8); ``hbm_share``: bytes_engine over
  device time against the 8 TB/s HBM peak.
* ``compute_metrics_wall_s``: the whole compute_metrics call from host arrays (uploads included).
* ``scipy``: scipy.stats.spearmanr on the same data, 16 CPU threads, timed on a stated subset of pairs / grid points and
  scaled to the full set (``extrapolated``), with the largest difference from the device values on that subset.

    python tools/bench_metrics.py [reps]
"""
import ctypes
import json
import os
import sys
import time
import warnings
from concurrent.futures import ThreadPoolExecutor

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

import dl4ds_amd._lib as L
from dl4ds_amd.device import DeviceArray
from dl4ds_amd.metrics import compute_metrics

N, H, W, C = 365, 512, 512, 1
HBM_PEAK = 8.0e12
THREADS = 16
reps = int(sys.argv[1]) if len(sys.argv) > 1 else 5


def precip(rng, shape):
    return (np.round(rng.gamma(0.6, 3.0, shape), 1) * (rng.random(shape) > 0.6)).astype(np.float32)


rng = np.random.default_rng(0)
y = precip(rng, (N, H, W, C))
p = np.round(y * rng.uniform(0.6, 1.4, y.shape) + 0.3 * precip(rng, y.shape), 1).astype(np.float32)
lib = L.lib()
dy, dp = DeviceArray.from_numpy(y), DeviceArray.from_numpy(p)
HWC = H * W * C
cases = {'per_pair': (N, HWC, HWC, 1, (N,)), 'per_grid_point': (H * W, N, C, HWC, (H, W))}
outs, res = {}, {}
for name, (segs, length, ss, es, shape) in cases.items():
    out = DeviceArray(shape, np.float64)
    call = lambda: L.check(lib.dl4ds_spearman(dy.ptr, dp.ptr, segs, length, ss, es, out.ptr))
    for _ in range(2):
        call()
    L.check(lib.dl4ds_sync())
    t0 = time.perf_counter()
    for _ in range(reps):
        call()
    L.check(lib.dl4ds_sync())
    wall = (time.perf_counter() - t0) / reps
    L.check(lib.dl4ds_profile_enable(1))
    for _ in range(reps):
        call()
    buf = ctypes.create_string_buffer(1 << 16)
    L.check(lib.dl4ds_profile_report(buf, len(buf)))
    L.check(lib.dl4ds_profile_enable(0))
    rep = json.loads(buf.value.decode())['spearman']
    dev = rep['ms'] / reps
    elems = segs * length
    b_eng = elems * (176 if length > 4096 else 8)
    res[name] = dict(segments=segs, length=length, engine='global radix' if length > 4096 else 'LDS',
                     device_ms=round(dev, 3), wall_ms=round(1e3 * wall, 3), bytes_min=elems * 8, bytes_engine=b_eng,
                     hbm_share=round(b_eng / (dev * 1e-3) / HBM_PEAK, 3))
    outs[name] = out.numpy()
del dy, dp

compute_metrics(y[:8], p[:8], verbose=False)        # warm-up (library load, scratch)
t0 = time.perf_counter()
compute_metrics(y, p, verbose=False)
cm_wall = time.perf_counter() - t0

from scipy.stats import spearmanr   # noqa: E402


def scipy_time(fn, items):
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        t0 = time.perf_counter()
        with ThreadPoolExecutor(THREADS) as ex:
            vals = list(ex.map(fn, items))
        return time.perf_counter() - t0, np.array(vals)


pair_sub = list(range(0, N, N // 32))[:32]
t_pair, v_pair = scipy_time(lambda i: spearmanr(y[i].ravel(), p[i].ravel())[0], pair_sub)
yt, pt = y[..., 0].reshape(N, H * W), p[..., 0].reshape(N, H * W)
pts = list(range(0, H * W, 64))
t_pt, v_pt = scipy_time(lambda j: spearmanr(yt[:, j], pt[:, j])[0], pts)
diff = lambda a, b: float(np.nanmax(np.abs(a - b))) if np.isnan(a).tolist() == np.isnan(b).tolist() else float('inf')
scipy = {'threads': THREADS,
         'per_pair': dict(subset=len(pair_sub), subset_s=round(t_pair, 3), extrapolated_s=round(t_pair * N / len(pair_sub), 2),
                          max_abs_diff=diff(outs['per_pair'][pair_sub], v_pair)),
         'per_grid_point': dict(subset=len(pts), subset_s=round(t_pt, 3), extrapolated_s=round(t_pt * H * W / len(pts), 2),
                                max_abs_diff=diff(outs['per_grid_point'].ravel()[pts], v_pt))}
print(json.dumps(dict(bench='spearman', device=L.device_name(), shape=[N, H, W, C], zero_fraction=round(float((y == 0).mean()), 3),
                      reps=reps, **res, compute_metrics_wall_s=round(cm_wall, 3), scipy=scipy)))
