"""MC-dropout ensemble prediction on one GPU: Model.predict_ensemble against the loop a user had to write before it existed, and
the member-statistics kernel (csrc/ensemble.hip) alone.

Model: BASELINE configs[1] (residual backbone, sub-pixel post-upsampling 4x, 128^2 -> 512^2) with dropout_rate=0.2,
dropout_variant='mcdrop'; N = 64 host fields, K = 16 members, quantiles (0.05, 0.5, 0.95), batch 32.  In ONE process, after a warm-up
of both paths, ``reps`` alternating repetitions of
  (a) K x model.predict, np.stack, np.mean / np.std / np.min / np.max / np.quantile along the member axis, and
  (b) model.predict_ensemble;
the median wall time of each and their ratio are reported.  Then the reduce kernel on device-resident stacks of n = 16 x 512^2
elements at K = 8, 16, 32, 64, 128 (nq = 3): kernel time from the profiler's per-launch timestamps (tag ``ensemble_reduce``), the
algorithmic traffic (K + 4 + nq) * 4 * n over that time, and its fraction of the 8 TB/s HBM kernels are quoted against here.
Writes profiles/ensemble_predict.json (or the path given) and prints it.

    timeout -k 10 300 python tools/bench_ensemble.py [out.json] [reps]
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
import dl4ds_amd.models as PM
from dl4ds_amd.device import DeviceArray

HBM_PEAK = 8e12
out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, 'profiles', 'ensemble_predict.json')
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 5
N, K, Q, BATCH = 64, 16, (0.05, 0.5, 0.95), 32
lib = L.lib()

model = PM.net_postupsampling('resnet', 'spc', 4, 1, 0, (128, 128), dropout_rate=0.2, dropout_variant='mcdrop', seed=7)
x = np.random.default_rng(0).random((N, 128, 128, 1)).astype(np.float32)


def user_loop():
    members = np.stack([model.predict(x, batch_size=BATCH) for _ in range(K)])
    return dict(mean=np.mean(members, axis=0), std=np.std(members, axis=0), min=np.min(members, axis=0), max=np.max(members, axis=0),
                quantiles=np.quantile(members, Q, axis=0))


def ensemble():
    return model.predict_ensemble(x, K, batch_size=BATCH, quantiles=Q)


def wall(fn):
    L.check(lib.dl4ds_sync())
    t0 = time.perf_counter()
    fn()
    L.check(lib.dl4ds_sync())
    return time.perf_counter() - t0


for fn in (user_loop, ensemble):                 # warm-up: graph planning, allocations, first-touch of the result pages
    fn()
ta, tb = [], []
for _ in range(reps):
    ta.append(wall(user_loop))
    tb.append(wall(ensemble))
a, b = float(np.median(ta)), float(np.median(tb))
result = dict(bench='ensemble_predict', device=L.device_name(), model='net_postupsampling resnet spc x4 128->512, mcdrop 0.2',
              n_samples=N, n_members=K, quantiles=list(Q), batch_size=BATCH, reps=reps,
              user_loop_s=round(a, 4), user_loop_all_s=[round(t, 4) for t in ta],
              predict_ensemble_s=round(b, 4), predict_ensemble_all_s=[round(t, 4) for t in tb],
              ratio_ensemble_over_loop=round(b / a, 4), kernel=[])

n = 16 * 512 * 512
nq = len(Q)
qc = (ctypes.c_float * nq)(*Q)
stats = DeviceArray((4 + nq, n))
sp = [stats.ptr + r * n * 4 for r in range(5)]
slab = (281.0 + 12.0 * np.random.default_rng(1).standard_normal((8, n))).astype(np.float32)
for Kk in (8, 16, 32, 64, 128):
    stack = DeviceArray((Kk, n))
    for i in range(0, Kk, 8):
        L.check(lib.dl4ds_memcpy_h2d(stack.ptr + i * n * 4, slab.ctypes.data, slab.nbytes))
    call = lambda: L.check(lib.dl4ds_ensemble_reduce(stack.ptr, Kk, n, n, qc, nq, sp[0], sp[1], sp[2], sp[3], sp[4]))  # noqa: E731
    for _ in range(3):
        call()
    L.check(lib.dl4ds_sync())
    L.check(lib.dl4ds_profile_enable(1))
    runs = 10
    for _ in range(runs):
        call()
    buf = ctypes.create_string_buffer(1 << 16)
    L.check(lib.dl4ds_profile_report(buf, len(buf)))
    L.check(lib.dl4ds_profile_enable(0))
    ms = json.loads(buf.value.decode())['ensemble_reduce']['ms'] / runs
    nbytes = (Kk + 4 + nq) * 4 * n
    result['kernel'].append(dict(K=Kk, n=n, nq=nq, ms=round(ms, 4), gbs=round(nbytes / ms / 1e6, 1),
                                 of_8tbs=round(nbytes / (ms * 1e-3) / HBM_PEAK, 3)))
    stack.free()

os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
with open(out_path, 'w') as f:
    json.dump(result, f, indent=1)
print(json.dumps(result))
