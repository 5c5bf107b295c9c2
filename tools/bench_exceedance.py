"""Exceedance verification on one GPU: the kernel (csrc/exceedance.hip) next to the score kernels (csrc/ensemble_score.hip) on the
same device-resident stack in the same run, and ``metrics.exceedance_scores`` from host arrays against the numpy restatement.

Kernel: stacks of n = 16 x 512^2 elements (16 samples), K = 8, 32, 128 members, T = 1, 4, 16 thresholds spread over the data's
distribution (so the (c, o) table is populated, the case that costs LDS atomics), plus one 'sharp' row per K where every
threshold lies above the data (nearly every element in one corner bin).  After warming both, alternating repetitions of
dl4ds_ensemble_exceedance (all four outputs but count_dev) and dl4ds_ensemble_score; kernel time from the profiler's per-launch
timestamps (tags ``ensemble_exceedance``, ``ensemble_score``).  The yardstick reads the same (K + 1) * 4 * n bytes and sorts on
top.  ``read_tbs`` is that traffic over the kernel time, ``of_6p3`` its share of the 6.3 TB/s the project measured for streaming
reads.

Host: N = 16 samples of 256 x 256, K = 16, T = 4: ``exceedance_scores`` (upload included) against tests/exceedance_ref.scores_ref.

    timeout -k 10 500 python tools/bench_exceedance.py [out.json]
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
from dl4ds_amd.metrics import exceedance_scores
from tests import exceedance_ref as R

STREAM_TBS = 6.3
out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, 'profiles', 'exceedance.json')
lib = L.lib()
result = dict(bench='exceedance', device=L.device_name(), kernel=[])

B, n, nq = 16, 16 * 512 * 512, 3
per = n // B
qc = (ctypes.c_float * nq)(0.05, 0.5, 0.95)
rng = np.random.default_rng(1)
slab = (281.0 + 12.0 * rng.standard_normal((8, n))).astype(np.float32)
obs = DeviceArray.from_numpy((281.0 + 12.0 * rng.standard_normal(n)).astype(np.float32))
s_sample, s_cell, s_cov = DeviceArray((B, 4), np.float64), DeviceArray.zeros((4, per), np.float64), DeviceArray.zeros((nq,), np.uint64)


def kernel_ms(runs, *tags):
    """ms per call of each tag (the report empties the profiler: read once)"""
    buf = ctypes.create_string_buffer(1 << 16)
    L.check(lib.dl4ds_profile_report(buf, len(buf)))
    rep = json.loads(buf.value.decode())
    return [rep[tag]['ms'] / runs for tag in tags]


for K in (8, 32, 128):
    stack = DeviceArray((K, n))
    for i in range(0, K, 8):
        L.check(lib.dl4ds_memcpy_h2d(stack.ptr + i * n * 4, slab.ctypes.data, slab.nbytes))
    hist = DeviceArray.zeros((K + 1,), np.uint64)
    score = lambda: L.check(lib.dl4ds_ensemble_score(stack.ptr, K, n, n, obs.ptr, B, 0, None, 0, 0, qc, nq, None, None, None, None,  # noqa: E731
                                                     s_sample.ptr, s_cell.ptr, hist.ptr, s_cov.ptr))
    for T, sharp in ((1, False), (4, False), (16, False), (4, True)):
        q = np.linspace(0.0, 1.0, T + 2)[1:-1]
        thr = np.asarray(400.0 + np.arange(T) if sharp else np.quantile(slab[0, :100000], q), np.float32)
        dthr = DeviceArray.from_numpy(thr)
        sample, cell = DeviceArray((B, T, 4), np.int64), DeviceArray.zeros((T, 4, per), np.int64)
        table = DeviceArray.zeros((T, K + 1, 2), np.uint64)
        exc = lambda: L.check(lib.dl4ds_ensemble_exceedance(stack.ptr, K, n, n, obs.ptr, B, dthr.ptr, T, 0, None, sample.ptr,  # noqa: E731
                                                            cell.ptr, table.ptr))
        for _ in range(3):
            exc()
            score()
        L.check(lib.dl4ds_sync())
        L.check(lib.dl4ds_profile_enable(1))
        runs = 10
        for _ in range(runs):
            exc()
            score()
        ms_e, ms_s = kernel_ms(runs, 'ensemble_exceedance', 'ensemble_score')
        L.check(lib.dl4ds_profile_enable(0))
        read = (K + 1) * 4 * n
        result['kernel'].append(dict(K=K, T=T, sharp=sharp, n=n, exceedance_ms=round(ms_e, 4), read_tbs=round(read / ms_e / 1e9, 3),
                                     of_6p3=round(read / ms_e / 1e9 / STREAM_TBS, 3), ensemble_score_ms=round(ms_s, 4),
                                     ratio_exceedance_over_score=round(ms_e / ms_s, 3)))
        for d in (dthr, sample, cell, table):
            d.free()
    stack.free()
    hist.free()

# ---------------------------------------------------------------------------------------------- from host arrays
N, K, shape = 16, 16, (256, 256, 1)
members = (281.0 + 12.0 * rng.standard_normal((K, N) + shape)).astype(np.float32)
y = (281.0 + 12.0 * rng.standard_normal((N,) + shape)).astype(np.float32)
thr = [270.0, 281.0, 290.0, 300.0]
exceedance_scores(y, members, thr)
t_dev, t_ref = [], []
for _ in range(3):
    t0 = time.perf_counter()
    got = exceedance_scores(y, members, thr)
    t_dev.append(time.perf_counter() - t0)
    t0 = time.perf_counter()
    ref = R.scores_ref(members, y, thr, fields=False)
    t_ref.append(time.perf_counter() - t0)
R.assert_same(got, ref, 'bench', fields=False)
result.update(host=dict(n_samples=N, n_members=K, sample_shape=list(shape), thresholds=thr,
                        exceedance_scores_s=round(float(np.median(t_dev)), 4), numpy_restatement_s=round(float(np.median(t_ref)), 4),
                        ratio=round(float(np.median(t_dev) / np.median(t_ref)), 4)))

os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
with open(out_path, 'w') as f:
    json.dump(result, f, indent=1)
print(json.dumps(result))
