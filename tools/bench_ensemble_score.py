"""Ensemble verification on one GPU: the score kernels (csrc/ensemble_score.hip) next to the member-statistics kernel
(csrc/ensemble.hip) measured in the same run, and ``verify_ensemble`` against what a user had to write before it existed.

Kernel: device-resident stacks of n = 16 x 512^2 elements (16 samples), nq = 3, K = 8, 16, 32, 64; after warming both, alternating
repetitions of dl4ds_ensemble_score and dl4ds_ensemble_reduce, kernel time from the profiler's per-launch timestamps (tags
``ensemble_score``: stage 1 plus the two fold launches; ``ensemble_reduce``).  Traffic model of the score: (K + 1) * 4 * n read plus
the hand-over of five 4-byte words per element written and read once.  Expectation stated before the first run: the same band as the
reduce kernel for K <= 32 (same sort, O(K) more fp64 arithmetic); a ratio above about 1.5 there is to be explained (DESIGN.md
section 13), not tuned away by loosening semantics.

End to end: BASELINE configs[1] with mcdrop 0.2, N = 64, K = 16, batch 32; in ONE process, after a warm-up of both, ``reps``
alternating repetitions of (a) ``predict_ensemble(return_members=True)`` plus the O(K log K) numpy scores on the host and (b)
``verify_ensemble``; medians and their ratio.  Expectation: (b) clearly faster, the K-fold download and the host reduction go away.
Writes profiles/ensemble_score.json (or the path given) and prints it.

    timeout -k 10 400 python tools/bench_ensemble_score.py [out.json] [reps]
"""
import ctypes
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np

import dl4ds_amd
import dl4ds_amd._lib as L
import dl4ds_amd.models as PM
from dl4ds_amd.device import DeviceArray

HBM_PEAK = 8e12
out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, 'profiles', 'ensemble_score.json')
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 5
N, K, Q, BATCH = 64, 16, (0.05, 0.5, 0.95), 32
lib = L.lib()
result = dict(bench='ensemble_score', device=L.device_name(), kernel=[])

# ---------------------------------------------------------------------------------------------- kernels
B, n, nq = 16, 16 * 512 * 512, len(Q)
qc = (ctypes.c_float * nq)(*Q)
stats = DeviceArray((4 + nq, n))
sp = [stats.ptr + r * n * 4 for r in range(5)]
rng = np.random.default_rng(1)
slab = (281.0 + 12.0 * rng.standard_normal((8, n))).astype(np.float32)
obs_host = (281.0 + 12.0 * rng.standard_normal(n)).astype(np.float32)
obs = DeviceArray.from_numpy(obs_host)
# the same observation 4 bytes off a 16-byte boundary: the library then takes its one-element-per-lane instances (fewer registers,
# more waves per SIMD, 4-byte loads), which measures the narrower width without another build
obs_odd = DeviceArray((n + 4,))
L.check(lib.dl4ds_memcpy_h2d(obs_odd.ptr + 4, obs_host.ctypes.data, obs_host.nbytes))
sample, cell, cov = DeviceArray((B, 4), np.float64), DeviceArray.zeros((4, n // B), np.float64), DeviceArray.zeros((nq,), np.uint64)


def kernel_ms(runs, *tags):
    """ms per call of each tag (the report empties the profiler: read once)"""
    buf = ctypes.create_string_buffer(1 << 16)
    L.check(lib.dl4ds_profile_report(buf, len(buf)))
    rep = json.loads(buf.value.decode())
    return [rep[tag]['ms'] / runs for tag in tags]


for Kk in (8, 16, 32, 64):
    stack = DeviceArray((Kk, n))
    hist = DeviceArray.zeros((Kk + 1,), np.uint64)
    for i in range(0, Kk, 8):
        L.check(lib.dl4ds_memcpy_h2d(stack.ptr + i * n * 4, slab.ctypes.data, slab.nbytes))
    score = lambda: L.check(lib.dl4ds_ensemble_score(stack.ptr, Kk, n, n, obs.ptr, B, 0, None, 0, 0, qc, nq, None, None, None, None,  # noqa: E731
                                                     sample.ptr, cell.ptr, hist.ptr, cov.ptr))
    narrow = lambda: L.check(lib.dl4ds_ensemble_score(stack.ptr, Kk, n, n, obs_odd.ptr + 4, B, 0, None, 0, 0, qc, nq, None, None, None,  # noqa: E731
                                                      None, sample.ptr, cell.ptr, hist.ptr, cov.ptr))
    reduce_ = lambda: L.check(lib.dl4ds_ensemble_reduce(stack.ptr, Kk, n, n, qc, nq, sp[0], sp[1], sp[2], sp[3], sp[4]))  # noqa: E731
    for _ in range(3):
        score()
        reduce_()
    L.check(lib.dl4ds_sync())
    L.check(lib.dl4ds_profile_enable(1))
    runs = 10
    for _ in range(runs):
        score()
        reduce_()
    ms_s, ms_r = kernel_ms(runs, 'ensemble_score', 'ensemble_reduce')
    L.check(lib.dl4ds_profile_enable(0))
    for _ in range(3):
        narrow()
    L.check(lib.dl4ds_sync())
    L.check(lib.dl4ds_profile_enable(1))
    for _ in range(runs):
        narrow()
    ms_n, = kernel_ms(runs, 'ensemble_score')
    L.check(lib.dl4ds_profile_enable(0))
    by_s, by_r = (Kk + 1 + 10) * 4 * n, (Kk + 4 + nq) * 4 * n
    result['kernel'].append(dict(K=Kk, n=n, nq=nq, score_ms=round(ms_s, 4), score_gbs=round(by_s / ms_s / 1e6, 1),
                                 score_of_8tbs=round(by_s / (ms_s * 1e-3) / HBM_PEAK, 3), reduce_ms=round(ms_r, 4),
                                 reduce_gbs=round(by_r / ms_r / 1e6, 1), ratio_score_over_reduce=round(ms_s / ms_r, 3),
                                 score_one_per_lane_ms=round(ms_n, 4), ratio_one_per_lane_over_reduce=round(ms_n / ms_r, 3)))
    stack.free()
    hist.free()

# ---------------------------------------------------------------------------------------------- end to end
model = PM.net_postupsampling('resnet', 'spc', 4, 1, 0, (128, 128), dropout_rate=0.2, dropout_variant='mcdrop', seed=7)
hr = np.random.default_rng(0).random((N, 512, 512, 1)).astype(np.float32)


def host_scores(members, y):
    """what a user writes today: the sorted form on the host (O(K log K) per element), float64"""
    x = np.sort(members.astype(np.float64), axis=0)
    Kh = x.shape[0]
    y = y.astype(np.float64)
    coef = (2 * np.arange(Kh) - Kh + 1).reshape((Kh,) + (1,) * y.ndim)
    crps = np.abs(x - y).mean(axis=0) - (coef * x).sum(axis=0) / Kh**2
    below = (x < y).sum(axis=0)
    return dict(crps=crps.mean(), spread=np.sqrt(x.var(axis=0, ddof=1).mean()), rmse=np.sqrt(((x.mean(axis=0) - y) ** 2).mean()),
                rank_histogram=np.bincount(below.reshape(-1), minlength=Kh + 1),
                coverage=[(y <= np.quantile(x, p, axis=0)).mean() for p in Q])


def user_loop():
    res = dl4ds_amd.predict_ensemble(model, hr, 4, K, quantiles=Q, batch_size=BATCH, return_members=True)
    return host_scores(res['members'], hr)


def verify():
    return dl4ds_amd.verify_ensemble(model, hr, 4, K, quantiles=Q, batch_size=BATCH)['scores']


def wall(fn):
    L.check(lib.dl4ds_sync())
    t0 = time.perf_counter()
    fn()
    L.check(lib.dl4ds_sync())
    return time.perf_counter() - t0


for fn in (user_loop, verify):
    fn()
ta, tb = [], []
for _ in range(reps):
    ta.append(wall(user_loop))
    tb.append(wall(verify))
a, b = float(np.median(ta)), float(np.median(tb))
result.update(model='net_postupsampling resnet spc x4 128->512, mcdrop 0.2', n_samples=N, n_members=K, quantiles=list(Q),
              batch_size=BATCH, reps=reps, user_loop_s=round(a, 4), user_loop_all_s=[round(t, 4) for t in ta],
              verify_ensemble_s=round(b, 4), verify_ensemble_all_s=[round(t, 4) for t in tb],
              ratio_verify_over_loop=round(b / a, 4))

os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
with open(out_path, 'w') as f:
    json.dump(result, f, indent=1)
print(json.dumps(result))
