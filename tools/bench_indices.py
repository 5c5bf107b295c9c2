"""Climate indices on one GPU, one JSON line, also written to profiles/indices.json.  Data: ten years of daily 512 x 512 x 1
precipitation-like fields (3650, 512, 512, 1), P = 10 periods of 365 days, window 5.  Everything is measured in one run:

* ``kernel``: dl4ds_climate_indices on the device-resident array after warm-up, all four outputs, at T = 3 (thresholds 1, 10, 20,
  '>=': one call gives every precipitation index) and at T = 1.  ``kernel_ms``: kernel time of one call from the library profiler
  (per-launch timestamps); ``wall_ms``: host time of the call bracketed by device syncs; ``read_tb_s`` = the 4 B per element read
  once over the kernel time, next to ``hbm_peak_tb_s``, the project's 6.3 TB/s figure.
* ``scaler_stats``: dl4ds_scaler_stats reducing axis 0 of the same array: also one read of x with fp64 accumulation per cell, the
  yardstick; ``over_scaler_stats`` = kernel time / its kernel time.
* ``host``: `climate_indices` and `precipitation_indices` from host arrays (uploads in bands, downloads and host copies included).
* ``numpy``: tests/indices_ref.py, the restatement, on ``numpy.cells`` whole grid rows, extrapolated to the grid; it agrees bit
  for bit with the device on that subset (asserted).
``window_values`` says where the kernel takes a window's values from: 'lds_ring' in the product library; 'global' in an
experiments build (DL4DS_BUILD_EXPERIMENTS=1, loaded through DL4DS_HIP_LIB) run with DL4DS_INDICES_WINDOW_GLOBAL=1.

    python tools/bench_indices.py [reps] [output.json] [--kernel-only]
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
from dl4ds_amd.indices import climate_indices, precipitation_indices
from tests import indices_ref

HBM_PEAK = 6.3e12
YEARS, H, W, C = 10, 512, 512, 1
N, WINDOW = 365 * YEARS, 5
CPU_ROWS = 2
args = [a for a in sys.argv[1:] if not a.startswith('--')]
kernel_only = '--kernel-only' in sys.argv
reps = int(args[0]) if args else 5
out_path = args[1] if len(args) > 1 else os.path.join(ROOT, 'profiles', 'indices.json')
per = H * W * C
starts = np.arange(0, N + 1, 365, dtype=np.int64)
P = len(starts) - 1
lib = L.lib()
window_values = 'global' if os.environ.get('DL4DS_INDICES_WINDOW_GLOBAL') and os.environ.get('DL4DS_HIP_LIB') else 'lds_ring'


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
d_x = DeviceArray.from_numpy(x)
read = 4 * N * per
kernel, outs = {}, {}
for T in (3, 1):
    thr = DeviceArray.from_numpy(np.array([1.0, 10.0, 20.0][:T], np.float32))
    devs = [DeviceArray((P, per), np.int32), DeviceArray((P, T, 6, per), np.int32), DeviceArray((P, 2, per)),
            DeviceArray((P, 2 + T, per), np.float64)]
    ms, wall = timed(lambda: L.check(lib.dl4ds_climate_indices(d_x.ptr, N, per, starts.ctypes.data, P, thr.ptr, T, 0, 0, WINDOW,
                                                               *(d.ptr for d in devs))), 'climate_indices')
    kernel[f'T{T}'] = dict(thresholds=T, kernel_ms=round(ms, 3), wall_ms=round(wall, 3), read_bytes=read,
                           read_tb_s=round(read / (ms * 1e-3) / 1e12, 3), ns_per_element=round(1e6 * ms / (N * per), 5),
                           output_bytes=sum(d.nbytes for d in devs))
    if T == 3:
        outs = [d.numpy() for d in devs]
    for d in devs + [thr]:
        d.free()

# ---- the yardstick: one read of x, fp64 accumulation per cell
shape, reduce_ = (ctypes.c_size_t * 2)(N, per), (ctypes.c_int * 2)(1, 0)
stats, flag = DeviceArray((5, per), np.float64), DeviceArray.zeros((1,), np.uint32)
ms_sc, wall_sc = timed(lambda: L.check(lib.dl4ds_scaler_stats(d_x.ptr, 0, shape, 2, reduce_, stats.ptr, flag.ptr, None)), 'scaler_stats')
scaler = dict(kernel_ms=round(ms_sc, 3), wall_ms=round(wall_sc, 3), read_tb_s=round(read / (ms_sc * 1e-3) / 1e12, 3))
for k in kernel.values():
    k['over_scaler_stats'] = round(k['kernel_ms'] / ms_sc, 2)
for d in (d_x, stats, flag):
    d.free()

result = dict(bench='indices', device_name=L.device_name(), shape=[N, H, W, C], periods=P, window=WINDOW, reps=reps,
              window_values=window_values, hbm_peak_tb_s=HBM_PEAK / 1e12, kernel=kernel, scaler_stats=scaler)
if not kernel_only:
    # ---- the restatement on a few grid rows, bit for bit
    cells = CPU_ROWS * W * C
    t0 = time.perf_counter()
    want = indices_ref.climate_indices(x[:, :CPU_ROWS].reshape(N, cells), starts, np.array([1.0, 10.0, 20.0], np.float32), 0, WINDOW)
    t_ref = time.perf_counter() - t0
    for got, exp in zip(outs, want):
        bits = {4: np.uint32, 8: np.uint64}[exp.dtype.itemsize]
        assert got.dtype == exp.dtype and np.array_equal(got[..., :cells].view(bits), exp.view(bits))

    # ---- the public functions from host arrays
    climate_indices(x[:, :8], period_starts=starts)                         # warm-up
    t0 = time.perf_counter()
    r = climate_indices(x, period_starts=starts, thresholds=(1.0, 10.0, 20.0), window=WINDOW)
    t_host = time.perf_counter() - t0
    assert np.array_equal(r['sum'].reshape(P, per)[:, :cells].view(np.uint64), want[3][:, 0].view(np.uint64))
    t0 = time.perf_counter()
    pr = precipitation_indices(x, np.repeat(np.arange(1991, 1991 + YEARS), 365))
    t_pr = time.perf_counter() - t0
    assert np.array_equal(pr['cdd'].reshape(P, per), outs[1][:, 0, 2])
    result['host'] = dict(climate_indices_wall_s=round(t_host, 3), precipitation_indices_wall_s=round(t_pr, 3),
                          input_gb=round(x.nbytes / 1e9, 2))
    result['numpy'] = dict(omp_num_threads=os.environ.get('OMP_NUM_THREADS'), cells=cells, subset_s=round(t_ref, 3),
                           extrapolated_s=round(t_ref * per / cells, 1), bits_equal=True)

line = json.dumps(result)
print(line)
os.makedirs(os.path.dirname(out_path), exist_ok=True)
with open(out_path, 'w') as f:
    f.write(line + '\n')
