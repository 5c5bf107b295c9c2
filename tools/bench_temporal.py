"""Temporal verification on one GPU, one JSON line, also written to profiles/temporal.json.  Data: ten years of daily 512 x 512 x 1
precipitation-like fields (3650, 512, 512, 1), P = 10 periods of 365 days, lags (1, 2, 5), B = 16 spell bins; the second series is
the first shifted by one grid row.  Everything is measured in one run:

* ``temporal``: dl4ds_temporal on the device-resident arrays after warm-up, all six outputs, at S = 1 and 2 and T = 1 and 3
  (thresholds 1, 10, 20, '>=').  ``kernel_ms``: kernel time of one call from the library profiler (per-launch timestamps);
  ``wall_ms``: host time of the call bracketed by device syncs; ``read_tb_s`` = the 4*S B per element read once over the kernel
  time, next to ``hbm_peak_tb_s``, the project's 6.3 TB/s figure.
* ``climate_indices`` (T = 1 and 3, window 5) and ``scaler_stats`` (axis 0) on the same array: the two yardsticks, each also one
  ordered read of x; ``over_climate_indices`` / ``over_scaler_stats`` = kernel time / their kernel time (same T).
* ``trend``: dl4ds_trend at P = 30, 64 and 128 on 512 x 512 cells, all three outputs: kernel ms and slopes sorted per second.
* ``host``: `temporal_scores` and `mann_kendall` from host arrays (uploads in bands, downloads and host copies included).
* ``numpy``: tests/temporal_ref.py, the restatement, on ``numpy.cells`` whole grid rows, extrapolated to the grid; it agrees bit
  for bit with the device on that subset (asserted).

    python tools/bench_temporal.py [reps] [output.json] [--kernel-only]
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
from dl4ds_amd.temporal import mann_kendall, temporal_scores
from tests import temporal_ref

HBM_PEAK = 6.3e12
YEARS, H, W, C = 10, 512, 512, 1
N, WINDOW, BINS = 365 * YEARS, 5, 16
LAGS = np.array([1, 2, 5], np.int32)
THRESHOLDS = np.array([1.0, 10.0, 20.0], np.float32)
CPU_ROWS = 1
args = [a for a in sys.argv[1:] if not a.startswith('--')]
kernel_only = '--kernel-only' in sys.argv
reps = int(args[0]) if args else 5
out_path = args[1] if len(args) > 1 else os.path.join(ROOT, 'profiles', 'temporal.json')
per = H * W * C
starts = np.arange(0, N + 1, 365, dtype=np.int64)
P, NL = len(starts) - 1, len(LAGS)
lib = L.lib()


def fields(seed):
    """about 40 % dry days, an exponential tail, a few missing values"""
    r = np.random.default_rng(seed)
    out = np.empty((N, H, W, C), np.float32)
    for n in range(N):
        v = 8.0 * r.standard_exponential((H, W, C), np.float32) - 3.0
        out[n] = np.maximum(v, 0.0)
    out[::97, ::5, ::7] = np.nan
    return out


def timed(call, tag):
    """-> (kernel ms, wall ms) of one call"""
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
    return json.loads(buf.value.decode())[tag]['ms'] / reps, 1e3 * wall


x = fields(0)
p = np.roll(x, 1, axis=1)
d_x, d_p = DeviceArray.from_numpy(x), DeviceArray.from_numpy(p)
thr = DeviceArray.from_numpy(THRESHOLDS)

# ---- the yardsticks: dl4ds_climate_indices and dl4ds_scaler_stats, each one ordered read of x
indices = {}
for T in (3, 1):
    devs = [DeviceArray((P, per), np.int32), DeviceArray((P, T, 6, per), np.int32), DeviceArray((P, 2, per)),
            DeviceArray((P, 2 + T, per), np.float64)]
    ms, wall = timed(lambda: L.check(lib.dl4ds_climate_indices(d_x.ptr, N, per, starts.ctypes.data, P, thr.ptr, T, 0, 0, WINDOW,
                                                               *(d.ptr for d in devs))), 'climate_indices')
    indices[f'T{T}'] = dict(kernel_ms=round(ms, 3), wall_ms=round(wall, 3), read_tb_s=round(4 * N * per / (ms * 1e-3) / 1e12, 3))
    for d in devs:
        d.free()
shape, reduce_ = (ctypes.c_size_t * 2)(N, per), (ctypes.c_int * 2)(1, 0)
stats, flag = DeviceArray((5, per), np.float64), DeviceArray.zeros((1,), np.uint32)
ms_sc, wall_sc = timed(lambda: L.check(lib.dl4ds_scaler_stats(d_x.ptr, 0, shape, 2, reduce_, stats.ptr, flag.ptr, None)), 'scaler_stats')
scaler = dict(kernel_ms=round(ms_sc, 3), wall_ms=round(wall_sc, 3), read_tb_s=round(4 * N * per / (ms_sc * 1e-3) / 1e12, 3))
for d in (stats, flag):
    d.free()

# ---- dl4ds_temporal
temporal, outs = {}, None
for S in (1, 2):
    for T in (3, 1):
        devs = [DeviceArray((P, per), np.int32), DeviceArray((P, S, 2, per), np.float64), DeviceArray((P, NL, per), np.int32),
                DeviceArray((P, S, NL, 3, per), np.float64), DeviceArray((P, S, T, 4, per), np.int32),
                DeviceArray((P, S, T, 2, BINS, per), np.int32)]
        ms, wall = timed(lambda: L.check(lib.dl4ds_temporal(d_x.ptr, d_p.ptr if S == 2 else None, N, per, starts.ctypes.data, P,
                                                            LAGS.ctypes.data, NL, thr.ptr, T, 0, 0, BINS, *(d.ptr for d in devs))),
                         'temporal')
        read = 4 * S * N * per
        temporal[f'S{S}T{T}'] = dict(series=S, thresholds=T, kernel_ms=round(ms, 3), wall_ms=round(wall, 3), read_bytes=read,
                                     read_tb_s=round(read / (ms * 1e-3) / 1e12, 3),
                                     ns_per_element=round(1e6 * ms / (S * N * per), 5), output_bytes=sum(d.nbytes for d in devs),
                                     over_climate_indices=round(ms / indices[f'T{T}']['kernel_ms'], 2),
                                     over_scaler_stats=round(ms / ms_sc, 2))
        if S == 2 and T == 3 and not kernel_only:
            cells = CPU_ROWS * W * C
            outs = [np.ascontiguousarray(d.numpy()[..., :cells]) for d in devs]
        for d in devs:
            d.free()
for d in (d_x, d_p, thr):
    d.free()

# ---- dl4ds_trend
trend = {}
rng = np.random.default_rng(1)
for periods in (30, 64, 128):
    v = rng.normal(0, 4, (periods, per)) + 0.05 * np.arange(periods)[:, None]
    v[rng.random((periods, per)) < 0.02] = np.nan
    d_v = DeviceArray.from_numpy(v)
    devs = [DeviceArray((per,), np.int32), DeviceArray((2, per), np.int64), DeviceArray((per,), np.float64)]
    ms, wall = timed(lambda: L.check(lib.dl4ds_trend(d_v.ptr, periods, per, *(d.ptr for d in devs))), 'trend')
    slopes = int((np.isfinite(v).sum(axis=0).astype(np.int64) * (np.isfinite(v).sum(axis=0) - 1) // 2).sum())
    trend[f'P{periods}'] = dict(periods=periods, kernel_ms=round(ms, 3), wall_ms=round(wall, 3), slopes=slopes,
                                gslopes_per_s=round(slopes / (ms * 1e-3) / 1e9, 3))
    if periods == 30 and not kernel_only:
        cells = CPU_ROWS * W * C
        got = [d.numpy() for d in devs]
        t0 = time.perf_counter()
        want = temporal_ref.trend(v[:, :cells])
        t_trend_ref = time.perf_counter() - t0
        assert np.array_equal(got[0][:cells], want[0]) and np.array_equal(got[1][:, :cells], want[1])
        assert np.array_equal(got[2][:cells].view(np.uint64), want[2].view(np.uint64))
        v30 = v
    for d in devs + [d_v]:
        d.free()

result = dict(bench='temporal', device_name=L.device_name(), shape=[N, H, W, C], periods=P, lags=LAGS.tolist(), spell_bins=BINS,
              reps=reps, hbm_peak_tb_s=HBM_PEAK / 1e12, temporal=temporal, climate_indices=indices, scaler_stats=scaler, trend=trend)
if not kernel_only:
    # ---- the restatement on a few grid rows, bit for bit
    cells = CPU_ROWS * W * C
    t0 = time.perf_counter()
    want = temporal_ref.temporal(x[:, :CPU_ROWS].reshape(N, cells), p[:, :CPU_ROWS].reshape(N, cells), starts, LAGS, THRESHOLDS, 0, BINS)
    t_ref = time.perf_counter() - t0
    for got, exp in zip(outs, want):
        assert got.dtype == exp.dtype and got.shape == exp.shape
        assert np.array_equal(got.view(np.uint64) if exp.dtype.kind == 'f' else got, exp.view(np.uint64) if exp.dtype.kind == 'f' else exp)

    # ---- the public functions from host arrays
    temporal_scores(x[:, :8], p[:, :8], period_starts=starts)              # warm-up
    t0 = time.perf_counter()
    r = temporal_scores(x, p, period_starts=starts, lags=LAGS.tolist(), thresholds=THRESHOLDS, spell_bins=BINS)
    t_host = time.perf_counter() - t0
    assert np.array_equal(r['pred']['sum_sq'].reshape(P, per)[:, :cells].view(np.uint64), want[1][:, 1, 1].view(np.uint64))
    t0 = time.perf_counter()
    mk = mann_kendall(v30.reshape(30, H, W, C))
    t_mk = time.perf_counter() - t0
    assert np.array_equal(mk['s'].reshape(per)[:cells], temporal_ref.trend(v30[:, :cells])[1][0])
    result['host'] = dict(temporal_scores_wall_s=round(t_host, 3), mann_kendall_wall_s=round(t_mk, 3),
                          input_gb=round((x.nbytes + p.nbytes) / 1e9, 2))
    result['numpy'] = dict(omp_num_threads=os.environ.get('OMP_NUM_THREADS'), cells=cells, temporal_subset_s=round(t_ref, 3),
                           temporal_extrapolated_s=round(t_ref * per / cells, 1), trend_p30_subset_s=round(t_trend_ref, 3),
                           trend_p30_extrapolated_s=round(t_trend_ref * per / cells, 1), bits_equal=True)

line = json.dumps(result)
print(line)
os.makedirs(os.path.dirname(out_path), exist_ok=True)
with open(out_path, 'w') as f:
    f.write(line + '\n')
