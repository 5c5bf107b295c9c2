"""Distribution verification (quantiles, W1, KS, histograms) on one GPU, one JSON line, also written to profiles/distribution.json.
Data: N = 365 synthetic 128 x 128 x 1 precipitation-like fields (about 60 % exact zeros, values rounded to 0.1) and one larger set
of 730 fields of 256 x 256; 7 quantiles, 7 bins.

* ``engines``: dl4ds_distribution on device-resident arrays after warm-up, one entry per engine of csrc/distribution.hip:
  ``strided`` (per grid cell over 365 samples), ``lds`` (contiguous segments of 8192 values: the same data cut in rows),
  ``global_contiguous`` (per sample over its 16384 values) and ``global_strided`` (per grid cell over 730 samples).
  ``kernel_ms``: kernel time of one call from the library profiler (per-launch timestamps, summed); ``wall_ms``: host time of the
  call bracketed by device syncs; ``input_bytes`` = 8 B per element, read once; ``input_read_tb_s`` = those bytes over the
  kernel time -- for the LDS engines the input read is all the HBM traffic there is apart from the small outputs, for the global
  engine the radix passes move several times more -- next to ``hbm_peak_tb_s``, the project's 6.3 TB/s figure.
* ``distribution_scores_wall_s``: the whole call from host arrays (row bands copied contiguous, uploads, host arithmetic).
* ``cpu``: tests/distribution_ref.py on a stated subset of cells, scaled to all of them (``extrapolated_s``), and a plain
  ``np.quantile(..., axis=0)`` of both arrays over the time axis (quantiles only: no W1, KS or histogram) on the same data in the
  same run, OMP_NUM_THREADS as the machine sets it (numpy runs these single-threaded).

    python tools/bench_distribution.py [reps] [output.json]
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
from dl4ds_amd.metrics import DIST_DEFAULT_QUANTILES, distribution_scores
from tests import distribution_ref

QUANT = np.array(DIST_DEFAULT_QUANTILES, np.float64)
EDGES = np.array([0.0, 0.1, 1.0, 2.0, 5.0, 10.0, 20.0, 50.0], np.float32)
Q, E = len(QUANT), len(EDGES)
HBM_PEAK = 6.3e12
CPU_CELLS = 512
reps = int(sys.argv[1]) if len(sys.argv) > 1 else 5
out_path = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, 'profiles', 'distribution.json')


def precip(rng, shape):
    return (np.round(rng.gamma(0.6, 3.0, shape), 1) * (rng.random(shape) > 0.6)).astype(np.float32)


def pair(seed, shape):
    rng = np.random.default_rng(seed)
    y = precip(rng, shape)
    return y, np.round(0.8 * precip(rng, shape) + 0.3 * precip(rng, shape), 1).astype(np.float32)


lib = L.lib()


def device_call(dy, dp, S, length, ss, es, tag):
    """one engine on device-resident arrays -> dict of timings"""
    outs = [DeviceArray((S, 2, Q), np.float64), DeviceArray((S,), np.float64), DeviceArray((S,), np.int64),
            DeviceArray((S, 2, E - 1), np.int64), DeviceArray((S,), np.int64)]
    call = lambda: L.check(lib.dl4ds_distribution(dy.ptr, dp.ptr, S, length, ss, es, QUANT.ctypes.data, Q, EDGES.ctypes.data, E,
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
    ms = json.loads(buf.value.decode())[tag]['ms'] / reps
    w1 = outs[1].numpy()
    for o in outs:
        o.free()
    nbytes = 8 * S * length
    return dict(segments=S, length=length, seg_stride=ss, elem_stride=es, kernel_ms=round(ms, 3), wall_ms=round(1e3 * wall, 3),
                input_bytes=nbytes, input_read_tb_s=round(nbytes / (ms * 1e-3) / 1e12, 3),
                ns_per_element=round(1e6 * ms / (S * length), 4), mean_w1=float(np.nanmean(w1)))


N, H, W, C = 365, 128, 128, 1
y, p = pair(0, (N, H, W, C))
cells = H * W * C
dy, dp = DeviceArray.from_numpy(y), DeviceArray.from_numpy(p)
engines = dict(strided=device_call(dy, dp, cells, N, 1, cells, 'distribution_strided'),
               lds=device_call(dy, dp, N * cells // 8192, 8192, 8192, 1, 'distribution_lds'),
               global_contiguous=device_call(dy, dp, N, cells, cells, 1, 'distribution_global'))
dy.free()
dp.free()

distribution_scores(y[:, :8], p[:, :8], QUANT, EDGES)          # warm-up
t0 = time.perf_counter()
full = distribution_scores(y, p, QUANT, EDGES)
ds_wall = time.perf_counter() - t0

sub = np.linspace(0, W - 1, CPU_CELLS // H).astype(int)          # CPU_CELLS cells: a few whole columns of the grid
t0 = time.perf_counter()
ref = distribution_ref.distribution_scores(y[:, :, sub], p[:, :, sub], QUANT, EDGES)
t_ref = time.perf_counter() - t0
assert np.array_equal(ref['ks_count'], full['ks_count'][:, sub]) and np.array_equal(ref['hist_obs'], full['hist_obs'][:, sub])
q_diff = float(np.abs(ref['q_obs'] - full['q_obs'][:, sub]).max())
t0 = time.perf_counter()
nq = [np.quantile(a, QUANT, axis=0) for a in (y, p)]
t_np = time.perf_counter() - t0
np_diff = float(np.abs(np.moveaxis(nq[0], 0, -1) - full['q_obs']).max())
small = dict(shape=[N, H, W, C], distribution_scores_wall_s=round(ds_wall, 3),
             cpu=dict(omp_num_threads=os.environ.get('OMP_NUM_THREADS'),
                      distribution_ref=dict(subset_cells=len(sub) * H, subset_s=round(t_ref, 3),
                                            extrapolated_s=round(t_ref * cells / (len(sub) * H), 1), counts_equal=True,
                                            max_abs_diff_q_obs=q_diff),
                      np_quantile_axis0=dict(both_arrays_s=round(t_np, 3), max_abs_diff_q_obs=np_diff)))
del full, ref, nq

N2, H2, W2 = 730, 256, 256
y, p = pair(1, (N2, H2, W2, 1))
cells2 = H2 * W2
dy, dp = DeviceArray.from_numpy(y), DeviceArray.from_numpy(p)
engines['global_strided'] = device_call(dy, dp, cells2, N2, 1, cells2, 'distribution_global')
dy.free()
dp.free()
t0 = time.perf_counter()
full = distribution_scores(y, p, QUANT, EDGES)
ds_wall2 = time.perf_counter() - t0
t0 = time.perf_counter()
nq = [np.quantile(a, QUANT, axis=0) for a in (y, p)]
t_np2 = time.perf_counter() - t0
large = dict(shape=[N2, H2, W2, 1], distribution_scores_wall_s=round(ds_wall2, 3),
             cpu=dict(np_quantile_axis0=dict(both_arrays_s=round(t_np2, 3),
                                             max_abs_diff_q_obs=float(np.abs(np.moveaxis(nq[0], 0, -1) - full['q_obs']).max()))))
line = json.dumps(dict(bench='distribution', device_name=L.device_name(), quantiles=QUANT.tolist(), bins=EDGES.tolist(), reps=reps,
                       hbm_peak_tb_s=HBM_PEAK / 1e12, engines=engines, small=small, large=large,
                       naive_one_lane_per_column='not measured'))
print(line)
os.makedirs(os.path.dirname(out_path), exist_ok=True)
with open(out_path, 'w') as f:
    f.write(line + '\n')
