"""The weighted loss op next to the unweighted one on one GPU, one JSON line, also written to profiles/weighted_loss.json.
Batch (64, 512, 512, 1), device-resident; in ONE run, for `mae` and for `dssim_mae`:

* ``unweighted``: dl4ds_op_loss;
* ``shared``: dl4ds_op_loss_weighted with one (512, 512) map for all samples (1 MB: it should come from cache);
* ``per_sample``: dl4ds_op_loss_weighted with one map per sample (64, 512, 512, 1).

``ms`` is the host time of one call, averaged over `reps` back-to-back calls bracketed by device synchronisations after warm-up
(the calls are asynchronous, so this is the device time of the op's kernels plus whatever launch gaps the queue cannot hide).
``bytes`` is what the algorithm has to move, from the shapes: the pixel pass reads y_true and y_pred and writes dpred (12 B per
element) plus 4 B per weight it reads (the map once for ``shared``, one per element for ``per_sample``) plus the weight-sum pass
(4 B per weight); the DSSIM passes are counted as the library's own profile scope counts them (32 B per element) plus, weighted,
the map read of the omega pass and the write and read of the omega map.  ``tb_s`` = bytes / ms next to ``hbm_peak_tb_s``, the
project's 6.3 TB/s figure; ``over_unweighted`` = ms over the unweighted op's ms of the same kind in the same run (the traffic bound
for the weighted mae is 16/12 with per-sample maps).

    python tools/bench_weighted_loss.py [reps] [output.json]
"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np

import dl4ds_amd._lib as L
from dl4ds_amd.device import DeviceArray
from dl4ds_amd.ops import LOSS_KINDS

HBM_PEAK = 6.3e12
N, H, W, C = 64, 512, 512, 1
reps = int(sys.argv[1]) if len(sys.argv) > 1 else 50
out_path = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, 'profiles', 'weighted_loss.json')
lib = L.lib()
n = N * H * W * C
n_windows = N * C * (H - 10) * (W - 10)


def timed(call):
    for _ in range(3):
        call()
    L.check(lib.dl4ds_sync())
    t0 = time.perf_counter()
    for _ in range(reps):
        call()
    L.check(lib.dl4ds_sync())
    return 1e3 * (time.perf_counter() - t0) / reps


def main():
    rng = np.random.default_rng(0)
    yt = np.empty((N, H, W, C), np.float32)
    yp = np.empty((N, H, W, C), np.float32)
    ws = np.empty((N, H, W, 1), np.float32)
    for k in range(N):
        yt[k] = rng.random((H, W, C), np.float32)
        yp[k] = yt[k] + 0.1 * rng.standard_normal((H, W, C), np.float32)
        ws[k] = rng.random((H, W, 1), np.float32) * (rng.random((H, W, 1), np.float32) > 0.3)
    dt, dp, dg, lv = DeviceArray.from_numpy(yt), DeviceArray.from_numpy(yp), DeviceArray.zeros(yp.shape), DeviceArray.zeros((8,))
    forms = {'shared': (DeviceArray.from_numpy(ws[0]), 1), 'per_sample': (DeviceArray.from_numpy(ws), N)}
    res = {'shape': [N, H, W, C], 'reps': reps, 'hbm_peak_tb_s': HBM_PEAK / 1e12, 'device': L.device_name(), 'kinds': {}}
    for kind in ('mae', 'dssim_mae'):
        k = LOSS_KINDS[kind]
        dssim_bytes = 32 * n if kind != 'mae' else 0
        rows = {}
        ms = timed(lambda: L.check(lib.dl4ds_op_loss(k, dt.ptr, dp.ptr, dg.ptr, N, H, W, C, lv.ptr)))
        rows['unweighted'] = dict(ms=ms, bytes=12 * n + dssim_bytes)
        rows['unweighted']['loss'] = float(lv.numpy()[0])
        for form, (dw, wb) in forms.items():
            nw = wb * H * W
            ms = timed(lambda: L.check(lib.dl4ds_op_loss_weighted(k, dt.ptr, dp.ptr, dg.ptr, N, H, W, C, dw.ptr, wb, 1, lv.ptr)))
            b = 12 * n + 4 * nw * 2
            if dssim_bytes:
                b += dssim_bytes + 4 * nw + 8 * (n_windows * wb // N)
            rows[form] = dict(ms=ms, bytes=b, loss=float(lv.numpy()[0]))
        for r in rows.values():
            r['tb_s'] = r['bytes'] / (r['ms'] * 1e-3) / 1e12
            r['over_unweighted'] = r['ms'] / rows['unweighted']['ms']
        res['kinds'][kind] = rows
    line = json.dumps(res)
    print(line)
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    with open(out_path, 'w') as f:
        f.write(line + '\n')


if __name__ == '__main__':
    main()
