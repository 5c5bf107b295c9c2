"""Neighbourhood verification of an ensemble on one GPU: the entry (csrc/ensemble_fss.hip) next to the exceedance kernel
(csrc/exceedance.hip) on the same device-resident stack and next to ``dl4ds_fss`` (csrc/fss.hip) on member 0, in the same run, and
``metrics.neighbourhood_ensemble_scores`` from host arrays next to the numpy restatement.

Kernel: stacks of (64, 512, 512, 1) samples, K = 8 and 32 members (eight distinct precipitation-like rows, repeated), T = 5
thresholds, the seven default windows.  After warming all three, alternating repetitions of dl4ds_ensemble_fss,
dl4ds_ensemble_exceedance (sample, cell and table outputs) and dl4ds_fss; kernel times from the profiler's per-launch timestamps
(tags ``ensemble_fss_prefix``, ``ensemble_fss_window``, ``ensemble_exceedance``, ``fss_prefix``, ``fss_window``).  ``read_tbs`` is
the stack read (K + 1) * 4 * n bytes over the kernel time, ``of_6p3`` its share of the 6.3 TB/s the project measured for streaming
reads; the window kernels are compared per window launch.

Host: N = 8 samples of 256 x 256, K = 8, T = 3, the default windows: ``neighbourhood_ensemble_scores`` (upload included); the
restatement tests/ensemble_fss_ref.py is timed on the first two samples only (it is slow) and its integers are compared.

    timeout -k 10 500 python tools/bench_ensemble_fss.py [out.json]
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
from dl4ds_amd.metrics import FSS_DEFAULT_WINDOWS, neighbourhood_ensemble_scores
from tests import ensemble_fss_ref as R
from tests.fss_cases import precip

STREAM_TBS = 6.3
out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, 'profiles', 'ensemble_fss.json')
lib = L.lib()
result = dict(bench='ensemble_fss', device=L.device_name(), kernel=[])

B, H, W, C, T = 64, 512, 512, 1, 5
n = B * H * W * C
per = n // B
rng = np.random.default_rng(1)
truth = precip(rng, (B, H, W, C))
slab = np.stack([np.round(np.roll(truth, (k % 3, -(k % 4)), axis=(1, 2)) + 0.3 * precip(rng, (B, H, W, C)), 1).reshape(n)
                 for k in range(8)]).astype(np.float32)
obs = DeviceArray.from_numpy(truth.reshape(n))
thr = np.asarray([0.1, 0.5, 1.0, 2.0, 5.0], np.float32)
win = np.asarray(FSS_DEFAULT_WINDOWS, np.int32)
S = len(win)
dthr = DeviceArray.from_numpy(thr)


def kernel_ms(tags, runs):
    buf = ctypes.create_string_buffer(1 << 16)
    L.check(lib.dl4ds_profile_report(buf, len(buf)))
    rep = json.loads(buf.value.decode())
    return [rep[t]['ms'] / runs for t in tags]


e_sums, e_cont, e_valid = DeviceArray((B, C, T, S, 5), np.int64), DeviceArray((B, C, T, 2), np.int64), DeviceArray((B, C), np.int64)
f_sums, f_cont, f_valid = DeviceArray((B, C, T, S, 3), np.int64), DeviceArray((B, C, T, 4), np.int64), DeviceArray((B, C), np.int64)
x_sample, x_cell = DeviceArray((B, T, 4), np.int64), DeviceArray.zeros((T, 4, per), np.int64)
for K in (8, 32):
    stack = DeviceArray((K, n))
    for i in range(0, K, 8):
        L.check(lib.dl4ds_memcpy_h2d(stack.ptr + i * n * 4, slab.ctypes.data, slab.nbytes))
    table = DeviceArray.zeros((T, K + 1, 2), np.uint64)
    efss = lambda: L.check(lib.dl4ds_ensemble_fss(stack.ptr, K, n, n, obs.ptr, B, H, W, C, thr.ctypes.data, T, win.ctypes.data, S,  # noqa: E731
                                                  e_sums.ptr, e_cont.ptr, e_valid.ptr))
    exc = lambda: L.check(lib.dl4ds_ensemble_exceedance(stack.ptr, K, n, n, obs.ptr, B, dthr.ptr, T, 0, None, x_sample.ptr,  # noqa: E731
                                                        x_cell.ptr, table.ptr))
    fss = lambda: L.check(lib.dl4ds_fss(obs.ptr, stack.ptr, B, H, W, C, thr.ctypes.data, T, win.ctypes.data, S, f_sums.ptr,  # noqa: E731
                                        f_cont.ptr, f_valid.ptr))
    for _ in range(2):
        efss()
        exc()
        fss()
    L.check(lib.dl4ds_sync())
    L.check(lib.dl4ds_profile_enable(1))
    runs = 5
    for _ in range(runs):
        efss()
        exc()
        fss()
    ep, ew, ex, fp, fw = kernel_ms(('ensemble_fss_prefix', 'ensemble_fss_window', 'ensemble_exceedance', 'fss_prefix', 'fss_window'),
                                   runs)
    L.check(lib.dl4ds_profile_enable(0))
    read = (K + 1) * 4 * n
    result['kernel'].append(dict(
        K=K, T=T, windows=win.tolist(), shape=[B, H, W, C],
        prefix_ms=round(ep, 4), prefix_read_tbs=round(read / ep / 1e9, 3), prefix_of_6p3=round(read / ep / 1e9 / STREAM_TBS, 3),
        exceedance_ms=round(ex, 4), exceedance_read_tbs=round(read / ex / 1e9, 3), ratio_prefix_over_exceedance=round(ep / ex, 3),
        window_ms_per_window=round(ew / S, 4), fss_window_ms_per_window=round(fw / S, 4), ratio_window_over_fss_window=round(ew / fw, 3),
        fss_prefix_ms=round(fp, 4), entry_ms=round(ep + ew, 4), fss_entry_ms=round(fp + fw, 4)))
    stack.free()
    table.free()

# ---------------------------------------------------------------------------------------------- from host arrays
N, K, shape, subset = 8, 8, (256, 256, 1), 2
y = precip(rng, (N,) + shape)
members = np.stack([np.round(np.roll(y, (1, -2), axis=(1, 2)) + 0.3 * precip(rng, (N,) + shape), 1) for _ in range(K)]).astype(np.float32)
thr_h = [0.1, 1.0, 5.0]
neighbourhood_ensemble_scores(y, members, thr_h)
t_dev = []
for _ in range(3):
    t0 = time.perf_counter()
    got = neighbourhood_ensemble_scores(y, members, thr_h)
    t_dev.append(time.perf_counter() - t0)
t0 = time.perf_counter()
sums, cont, nvalid = R.integer_sums(members[:, :subset], y[:subset], thr_h, FSS_DEFAULT_WINDOWS)
t_ref = time.perf_counter() - t0
np.testing.assert_array_equal(got['sums'][:subset], sums)
np.testing.assert_array_equal(got['events'][:subset], cont[..., 0])
np.testing.assert_array_equal(got['n_valid'][:subset], nvalid)
result.update(host=dict(n_samples=N, n_members=K, sample_shape=list(shape), thresholds=thr_h, windows=list(FSS_DEFAULT_WINDOWS),
                        neighbourhood_ensemble_scores_s=round(float(np.median(t_dev)), 4), restatement_samples=subset,
                        numpy_restatement_s=round(t_ref, 4)))

os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
with open(out_path, 'w') as f:
    json.dump(result, f, indent=1)
print(json.dumps(result))
