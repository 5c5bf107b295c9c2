"""Neighbourhood verification (FSS + contingency scores) on one GPU, one JSON line, also written to profiles/fss.json: N = 365
synthetic 512 x 512 x 1 precipitation-like fields (about 60 % exact zeros, values rounded to 0.1), 5 thresholds, the default
7 windows.

* ``device``: dl4ds_fss on device-resident arrays after warm-up.  ``kernel_ms``: kernel time per launch kind from the library
  profiler (per-launch timestamps, summed over the launches of one call); ``wall_ms``: host time of the call bracketed by device
  syncs.  ``bytes``: what the design moves by its own count (csrc/fss.hip) -- the prefix kernel reads
  8 B per cell and writes 2 sides x T two-byte prefixes, the window kernel reads 8 two-byte prefixes per cell, threshold and
  window -- and ``hbm_share``: those bytes over the kernel time against the 8 TB/s HBM peak (most window reads are served by
  the caches: a share of the peak, not a measured HBM rate).
* ``neighbourhood_scores_wall_s``: the whole call from host arrays (uploads in chunks, host arithmetic included).
* ``cpu``: tests/fss_ref.py (int64 integral images) and the scipy.ndimage.uniform_filter formulation on the same data in the
  same run, OMP_NUM_THREADS as the machine sets it (numpy and scipy run these single-threaded), timed on a stated subset of
  fields and scaled to the full set (``extrapolated_s``), with the largest difference of FSS from the device on that subset.

    python tools/bench_fss.py [reps] [output.json]
"""
import ctypes
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np

import dl4ds_amd._lib as L
from dl4ds_amd.device import DeviceArray
from dl4ds_amd.metrics import FSS_DEFAULT_WINDOWS, neighbourhood_scores, scores_from_counts
from tests import fss_ref

N, H, W, C = 365, 512, 512, 1
THRESHOLDS = np.array([0.1, 1.0, 2.0, 5.0, 10.0], np.float32)
WINDOWS = np.array(FSS_DEFAULT_WINDOWS, np.int32)
T, S = len(THRESHOLDS), len(WINDOWS)
HBM_PEAK = 8.0e12
CPU_FIELDS = 4
reps = int(sys.argv[1]) if len(sys.argv) > 1 else 5
out_path = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, 'profiles', 'fss.json')


def precip(rng, shape):
    return (np.round(rng.gamma(0.6, 3.0, shape), 1) * (rng.random(shape) > 0.6)).astype(np.float32)


rng = np.random.default_rng(0)
y = precip(rng, (N, H, W, C))
p = np.round(np.roll(y, (2, -3), axis=(1, 2)) * rng.uniform(0.6, 1.4, y.shape) + 0.3 * precip(rng, y.shape), 1).astype(np.float32)
lib = L.lib()
dy, dp = DeviceArray.from_numpy(y), DeviceArray.from_numpy(p)
outs = [DeviceArray(s, np.int64) for s in ((N, C, T, S, 3), (N, C, T, 4), (N, C))]
call = lambda: L.check(lib.dl4ds_fss(dy.ptr, dp.ptr, N, H, W, C, THRESHOLDS.ctypes.data, T, WINDOWS.ctypes.data, S,
                                     *(o.ptr for o in outs)))
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
rep = json.loads(buf.value.decode())
cells = N * H * W * C
nbytes = {'fss_prefix': cells * (8 + 2 * T * 2), 'fss_window': cells * T * S * 8 * 2}
kernel_ms = {k: rep[k]['ms'] / reps for k in nbytes}
total_ms = sum(kernel_ms.values())
device = dict(kernel_ms={k: round(v, 3) for k, v in kernel_ms.items()}, kernel_ms_total=round(total_ms, 3),
              launches_per_call={k: rep[k]['n'] // reps for k in nbytes}, wall_ms=round(1e3 * wall, 3),
              bytes=nbytes, bytes_min=cells * 8,
              hbm_share={k: round(nbytes[k] / (kernel_ms[k] * 1e-3) / HBM_PEAK, 3) for k in nbytes},
              hbm_share_total=round(sum(nbytes.values()) / (total_ms * 1e-3) / HBM_PEAK, 3),
              us_per_field_threshold_window=round(1e3 * total_ms / (N * C * T * S), 3))
dev = scores_from_counts(*(o.numpy() for o in outs), THRESHOLDS, WINDOWS)
del dy, dp, outs

neighbourhood_scores(y[:8], p[:8], THRESHOLDS, WINDOWS)        # warm-up
t0 = time.perf_counter()
full = neighbourhood_scores(y, p, THRESHOLDS, WINDOWS)
ns_wall = time.perf_counter() - t0
assert np.array_equal(full['sums'], dev['sums'])

sub = list(range(0, N, N // CPU_FIELDS))[:CPU_FIELDS]
t0 = time.perf_counter()
ref = fss_ref.neighbourhood_scores(y[sub], p[sub], THRESHOLDS, WINDOWS)
t_ref = time.perf_counter() - t0
assert np.array_equal(ref['sums'], dev['sums'][sub])

from scipy.ndimage import uniform_filter   # noqa: E402

t0 = time.perf_counter()
sc = np.empty((len(sub), T, S))
for a, i in enumerate(sub):
    ok = np.isfinite(y[i, :, :, 0]) & np.isfinite(p[i, :, :, 0])
    for k, t in enumerate(THRESHOLDS):
        bo, bf = (ok & (y[i, :, :, 0] >= t)).astype(np.float64), (ok & (p[i, :, :, 0] >= t)).astype(np.float64)
        for s, n in enumerate(WINDOWS):
            fo, ff = (uniform_filter(b, size=int(n), mode='constant', cval=0.0) for b in (bo, bf))
            sc[a, k, s] = 1.0 - ((ff - fo) ** 2).sum() / ((ff ** 2).sum() + (fo ** 2).sum())
t_sc = time.perf_counter() - t0
scale = N / len(sub)
cpu = dict(omp_num_threads=os.environ.get('OMP_NUM_THREADS'), subset_fields=len(sub),
           fss_ref=dict(subset_s=round(t_ref, 3), extrapolated_s=round(t_ref * scale, 1),
                        ms_per_field_threshold_window=round(1e3 * t_ref / (len(sub) * T * S), 2), sums_equal=True),
           scipy_uniform_filter=dict(subset_s=round(t_sc, 3), extrapolated_s=round(t_sc * scale, 1),
                                     ms_per_field_threshold_window=round(1e3 * t_sc / (len(sub) * T * S), 2),
                                     max_abs_diff_fss=float(np.abs(sc - dev['fss'][sub, 0]).max())))
line = json.dumps(dict(bench='fss', device_name=L.device_name(), shape=[N, H, W, C], thresholds=THRESHOLDS.tolist(),
                       windows=WINDOWS.tolist(), zero_fraction=round(float((y == 0).mean()), 3), reps=reps, device=device,
                       neighbourhood_scores_wall_s=round(ns_wall, 3), fss_pooled_first_threshold=np.round(dev['fss_pooled'][0], 4).tolist(),
                       cpu=cpu))
print(line)
with open(out_path, 'w') as f:
    f.write(line + '\n')
