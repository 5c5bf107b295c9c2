"""Multivariate ensemble verification on one GPU: the two entries of csrc/ensemble_multi.hip next to the score kernels
(csrc/ensemble_score.hip) on the same device-resident stack in the same run, and ``metrics.multivariate_scores`` from host arrays
against the numpy restatement.

Kernel: stacks of n = 16 x 512^2 elements (16 samples of (512, 512, 1)), K = 8, 16, 32 members.  After warming all of them,
alternating repetitions of dl4ds_ensemble_energy, dl4ds_ensemble_variogram (order 0.5; max_lag 2, 4, 8) and dl4ds_ensemble_score;
kernel time from the profiler's per-launch timestamps (tags ``ensemble_energy``, ``ensemble_variogram``, ``ensemble_score``).
Energy: ``fp64_tflops`` counts the 3 K (K + 1) / 2 fp64 operations per element of the definition (difference, square, weighted
add) over the kernel time, ``of_fp64_peak`` its share of the chip's 78.6 TFLOP/s vector-fp64 figure; ``read_tbs`` is the
(K + 1) * 4 * n bytes of the stack and the observation over the kernel time, ``of_6p3`` its share of the 6.3 TB/s the project
measured for streaming reads.  Variogram: ``gpairs_per_s`` counts (lags x elements x members) pair terms over the kernel time.

Host: N = 4 samples of (64, 64, 1), K = 8, max_lag 4: ``multivariate_scores`` (upload included) against
tests/multivariate_ref.scores_ref (the stated subset: the restatement sums in Python).

    timeout -k 10 500 python tools/bench_multivariate.py [out.json]
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
from dl4ds_amd.ensemble_score import variogram_lags
from dl4ds_amd.metrics import multivariate_scores
from tests import multivariate_ref as R

STREAM_TBS, FP64_TFLOPS = 6.3, 78.6
out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, 'profiles', 'multivariate.json')
lib = L.lib()
result = dict(bench='multivariate', device=L.device_name(), kernel=[])

B, H, W, nq = 16, 512, 512, 3
n = B * H * W
per = n // B
qc = (ctypes.c_float * nq)(0.05, 0.5, 0.95)
rng = np.random.default_rng(1)
slab = (281.0 + 12.0 * rng.standard_normal((8, n))).astype(np.float32)
obs = DeviceArray.from_numpy((281.0 + 12.0 * rng.standard_normal(n)).astype(np.float32))
s_sample, s_cell, s_cov = DeviceArray((B, 4), np.float64), DeviceArray.zeros((4, per), np.float64), DeviceArray.zeros((nq,), np.uint64)


def report():
    """{tag: {'ms': ...}} of the launches since the profiler was enabled (the report empties the profiler: read once)"""
    buf = ctypes.create_string_buffer(1 << 16)
    L.check(lib.dl4ds_profile_report(buf, len(buf)))
    return json.loads(buf.value.decode())


def timed(calls, runs=5):
    """{tag: ms per call} of the alternating calls, after three warm rounds"""
    for _ in range(3):
        for c in calls.values():
            c()
    L.check(lib.dl4ds_sync())
    L.check(lib.dl4ds_profile_enable(1))
    for _ in range(runs):
        for c in calls.values():
            c()
    rep = report()
    ms = {tag: rep[tag]['ms'] / runs for tag in calls}
    L.check(lib.dl4ds_profile_enable(0))
    return ms


for K in (8, 16, 32):
    stack = DeviceArray((K, n))
    for i in range(0, K, 8):
        L.check(lib.dl4ds_memcpy_h2d(stack.ptr + i * n * 4, slab.ctypes.data, slab.nbytes))
    hist = DeviceArray.zeros((K + 1,), np.uint64)
    dist, nvalid = DeviceArray((B, K * (K + 1) // 2), np.float64), DeviceArray((B,), np.int64)
    calls = dict(
        ensemble_energy=lambda: L.check(lib.dl4ds_ensemble_energy(stack.ptr, K, n, n, obs.ptr, B, None, dist.ptr, nvalid.ptr)),
        ensemble_score=lambda: L.check(lib.dl4ds_ensemble_score(stack.ptr, K, n, n, obs.ptr, B, 0, None, 0, 0, qc, nq, None, None, None,
                                                                None, s_sample.ptr, s_cell.ptr, hist.ptr, s_cov.ptr)))
    row = dict(K=K, n=n)
    for lag in (2, 4, 8):
        nl = len(variogram_lags(lag))
        npairs, vsums = DeviceArray((B, nl), np.int64), DeviceArray((B, nl, 3), np.float64)
        calls['ensemble_variogram'] = lambda: L.check(lib.dl4ds_ensemble_variogram(stack.ptr, K, n, n, obs.ptr, B, None, 1, H, W, 1, lag,  # noqa: E731
                                                                                   0, npairs.ptr, vsums.ptr))
        ms = timed(calls)
        row[f'variogram_lag{lag}_ms'] = round(ms['ensemble_variogram'], 4)
        row[f'variogram_lag{lag}_gpairs_per_s'] = round(nl * n * K / ms['ensemble_variogram'] / 1e6, 2)
        for d in (npairs, vsums):
            d.free()
    read, flops = (K + 1) * 4 * n, 3.0 * (K * (K + 1) // 2) * n
    row.update(energy_ms=round(ms['ensemble_energy'], 4), fp64_tflops=round(flops / ms['ensemble_energy'] / 1e9, 3),
               of_fp64_peak=round(flops / ms['ensemble_energy'] / 1e9 / FP64_TFLOPS, 4),
               read_tbs=round(read / ms['ensemble_energy'] / 1e9, 3), of_6p3=round(read / ms['ensemble_energy'] / 1e9 / STREAM_TBS, 3),
               ensemble_score_ms=round(ms['ensemble_score'], 4), ratio_energy_over_score=round(ms['ensemble_energy'] / ms['ensemble_score'], 3))
    result['kernel'].append(row)
    for d in (stack, hist, dist, nvalid):
        d.free()

# ---------------------------------------------------------------------------------------------- from host arrays
N, K, shape = 4, 8, (64, 64, 1)
members = (281.0 + 12.0 * rng.standard_normal((K, N) + shape)).astype(np.float32)
y = (281.0 + 12.0 * rng.standard_normal((N,) + shape)).astype(np.float32)
multivariate_scores(y, members)
t_dev, t_ref = [], []
for _ in range(3):
    t0 = time.perf_counter()
    got = multivariate_scores(y, members)
    t_dev.append(time.perf_counter() - t0)
t0 = time.perf_counter()
ref = R.scores_ref(members, y)
t_ref.append(time.perf_counter() - t0)
R.assert_same(got, ref, 'bench')
result.update(host=dict(n_samples=N, n_members=K, sample_shape=list(shape), max_lag=4, order=0.5,
                        multivariate_scores_s=round(float(np.median(t_dev)), 4), numpy_restatement_s=round(float(np.median(t_ref)), 4),
                        ratio=round(float(np.median(t_dev) / np.median(t_ref)), 4)))

os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
with open(out_path, 'w') as f:
    json.dump(result, f, indent=1)
print(json.dumps(result))
