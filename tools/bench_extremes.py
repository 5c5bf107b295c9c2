"""Extreme-value verification on one GPU, one JSON line, also written to profiles/extremes.json.  Data: ten years of daily
512 x 512 x 1 precipitation-like fields (3650, 512, 512, 1) and a hundred annual maxima (100, 512, 512, 1).  Everything is measured
in one run:

* ``lmoments``: dl4ds_lmoments at (100, 512, 512, 1) (block maxima; the bitonic rows in LDS) and at (3650, 512, 512, 1) (the radix
  sort), next to dl4ds_quantile_table (two probabilities) on the same arrays.  Both sort the same keys with the same engine;
  ``minus_quantile_table_ms`` is what the rank-order walk costs over reading two quantiles.  ``kernel_ms``: kernel time of one call
  from the library profiler; ``wall_ms``: host time of the call bracketed by device syncs.
* ``pot_peaks``: dl4ds_pot_peaks at (3650, 512, 512, 1) over the per-cell 95th percentile (from dl4ds_quantile_table), ten periods,
  run 1: the counting call (K = 0) and the call that stores every peak, next to dl4ds_climate_indices (T = 1, all outputs) on the
  same array.  ``read_tb_s`` = the 4 B per element read once over the kernel time, next to ``hbm_peak_tb_s``, the project's
  6.3 TB/s figure.
* ``host``: `extreme_scores` from host arrays (method 'gev' on the ten annual maxima and 'pot' over the threshold field; uploads in
  bands, downloads and the host fits included).
* ``numpy``: tests/extremes_ref.py, the restatement, on ``numpy.cells`` whole grid rows, extrapolated to the grid; it agrees bit
  for bit with the device on that subset (asserted).

    python tools/bench_extremes.py [reps] [output.json] [--kernel-only]
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
from dl4ds_amd.extremes import extreme_scores
from tests import extremes_ref

HBM_PEAK = 6.3e12
YEARS, H, W, C = 10, 512, 512, 1
N, BLOCKS, RUN = 365 * YEARS, 100, 1
CPU_ROWS = 2
args = [a for a in sys.argv[1:] if not a.startswith('--')]
kernel_only = '--kernel-only' in sys.argv
reps = int(args[0]) if args else 5
out_path = args[1] if len(args) > 1 else os.path.join(ROOT, 'profiles', 'extremes.json')
per = H * W * C
starts = np.arange(0, N + 1, 365, dtype=np.int64)
P = len(starts) - 1
lib = L.lib()


def fields(seed, n=N):
    """about 40 % dry days, an exponential tail, a few missing values"""
    r = np.random.default_rng(seed)
    out = np.empty((n, H, W, C), np.float32)
    for i in range(n):
        v = 8.0 * r.standard_exponential((H, W, C), np.float32) - 3.0
        out[i] = np.maximum(v, 0.0)
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


def same_bits(got, want):
    bits = {4: np.uint32, 8: np.uint64}[want.dtype.itemsize] if want.dtype.kind == 'f' else want.dtype
    return got.dtype == want.dtype and np.array_equal(got.view(bits), want.view(bits))


# ---- dl4ds_lmoments next to dl4ds_quantile_table: the same sort
q2 = np.array([0.95, 1.0], np.float64)
x = fields(0)
maxima = (30.0 + 8.0 * np.random.default_rng(1).gumbel(size=(BLOCKS, H, W, C))).astype(np.float32)
lmoments, pwm_long = {}, None
valid, pwm = DeviceArray((per,), np.int32), DeviceArray((4, per), np.float64)
table, valid64 = DeviceArray((2, per)), DeviceArray((per,), np.int64)
d_x = None
for name, host, engine in (('block_maxima', maxima, 'strided'), ('daily', x, 'global')):
    d = DeviceArray.from_numpy(host)
    n = host.shape[0]
    ms, wall = timed(lambda: L.check(lib.dl4ds_lmoments(d.ptr, n, per, per, 1, valid.ptr, pwm.ptr)), 'lmoments_' + engine)
    ms_q, wall_q = timed(lambda: L.check(lib.dl4ds_quantile_table(d.ptr, n, per, q2.ctypes.data, 2, table.ptr, valid64.ptr)),
                         'quantile_table_' + engine)
    lmoments[name] = dict(shape=[n, H, W, C], engine=engine, kernel_ms=round(ms, 3), wall_ms=round(wall, 3),
                          quantile_table_kernel_ms=round(ms_q, 3), quantile_table_wall_ms=round(wall_q, 3),
                          minus_quantile_table_ms=round(ms - ms_q, 3), over_quantile_table=round(ms / ms_q, 2),
                          input_tb_s=round(4 * n * per / (ms * 1e-3) / 1e12, 3))
    if name == 'daily':
        d_x, pwm_long = d, pwm.numpy()
    else:
        d.free()

# ---- dl4ds_pot_peaks next to dl4ds_climate_indices: the same 4 B / element read (the threshold: row 0 of the table, in place)
read = 4 * N * per
count = DeviceArray((per,), np.int32)
ms_c, wall_c = timed(lambda: L.check(lib.dl4ds_pot_peaks(d_x.ptr, N, per, starts.ctypes.data, P, table.ptr, 1, 1, RUN, 0, count.ptr,
                                                          None, None)), 'pot_peaks')
counts = count.numpy()
K = int(counts.max())
peak, pos = DeviceArray((K, per)), DeviceArray((K, per), np.int32)
ms_p, wall_p = timed(lambda: L.check(lib.dl4ds_pot_peaks(d_x.ptr, N, per, starts.ctypes.data, P, table.ptr, 1, 1, RUN, K, count.ptr,
                                                          peak.ptr, pos.ptr)), 'pot_peaks')
thr1 = DeviceArray.from_numpy(np.array([1.0], np.float32))
devs = [DeviceArray((P, per), np.int32), DeviceArray((P, 1, 6, per), np.int32), DeviceArray((P, 2, per)),
        DeviceArray((P, 3, per), np.float64)]
ms_i, wall_i = timed(lambda: L.check(lib.dl4ds_climate_indices(d_x.ptr, N, per, starts.ctypes.data, P, thr1.ptr, 1, 0, 0, 5,
                                                                *(v.ptr for v in devs))), 'climate_indices')
rate = lambda ms: round(read / (ms * 1e-3) / 1e12, 3)
pot = dict(shape=[N, H, W, C], periods=P, run=RUN, threshold='per-cell 95th percentile', read_bytes=read,
           count_only=dict(kernel_ms=round(ms_c, 3), wall_ms=round(wall_c, 3), read_tb_s=rate(ms_c),
                           over_climate_indices=round(ms_c / ms_i, 2)),
           all_peaks=dict(K=K, mean_peaks_per_cell=round(float(counts[counts >= 0].mean()), 1), kernel_ms=round(ms_p, 3),
                          wall_ms=round(wall_p, 3), read_tb_s=rate(ms_p), output_bytes=peak.nbytes + pos.nbytes + count.nbytes,
                          over_climate_indices=round(ms_p / ms_i, 2)),
           climate_indices_T1=dict(kernel_ms=round(ms_i, 3), wall_ms=round(wall_i, 3), read_tb_s=rate(ms_i),
                                   output_bytes=sum(v.nbytes for v in devs)))
thr_host, peaks_host, pos_host = table.numpy()[0], peak.numpy(), pos.numpy()
for v in devs + [thr1, peak, pos, count, d_x, valid, pwm, table, valid64]:
    v.free()

result = dict(bench='extremes', device_name=L.device_name(), reps=reps, hbm_peak_tb_s=HBM_PEAK / 1e12, lmoments=lmoments,
              pot_peaks=pot)
if not kernel_only:
    # ---- the restatement on a few grid rows, bit for bit
    cells = CPU_ROWS * W * C
    sub = x[:, :CPU_ROWS].reshape(N, cells)
    t0 = time.perf_counter()
    want_pwm = extremes_ref.pwm(sub)[1]
    t_pwm = time.perf_counter() - t0
    t0 = time.perf_counter()
    want_pot = extremes_ref.pot_peaks(sub, starts, thr_host[:cells], 1, RUN, K)
    t_pot = time.perf_counter() - t0
    assert same_bits(pwm_long[:, :cells], want_pwm)
    assert same_bits(counts[:cells], want_pot[0]) and same_bits(pos_host[:, :cells], want_pot[2])
    assert np.array_equal(np.isnan(peaks_host[:, :cells]), np.isnan(want_pot[1]))
    assert np.array_equal(np.nan_to_num(peaks_host[:, :cells]).view(np.uint32), np.nan_to_num(want_pot[1]).view(np.uint32))

    # ---- the public function from host arrays
    pred = fields(2)
    field = thr_host.reshape(H, W, C)
    extreme_scores(x[:, :8], pred[:, :8], period_starts=starts)                        # warm-up
    t0 = time.perf_counter()
    gev = extreme_scores(x, pred, period_starts=starts, method='gev')
    t_gev = time.perf_counter() - t0
    t0 = time.perf_counter()
    gpd = extreme_scores(x, pred, period_starts=starts, method='pot', threshold=field, run=RUN)
    t_gpd = time.perf_counter() - t0
    assert same_bits(gpd['obs']['n_valid'].reshape(per), counts)
    result['host'] = dict(extreme_scores_gev_wall_s=round(t_gev, 3), extreme_scores_pot_wall_s=round(t_gpd, 3),
                          input_gb=round((x.nbytes + pred.nbytes) / 1e9, 2), gev_not_converged=gev['obs']['fit']['n_not_converged'],
                          median_abs_bias_20=round(float(np.nanmedian(np.abs(gev['bias'][2]))), 3))
    result['numpy'] = dict(cells=cells, pwm_subset_s=round(t_pwm, 3), pwm_extrapolated_s=round(t_pwm * per / cells, 1),
                           pot_subset_s=round(t_pot, 3), pot_extrapolated_s=round(t_pot * per / cells, 1), bits_equal=True)

line = json.dumps(result)
print(line)
os.makedirs(os.path.dirname(out_path), exist_ok=True)
with open(out_path, 'w') as f:
    f.write(line + '\n')
