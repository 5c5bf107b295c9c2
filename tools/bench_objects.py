"""Object labelling on one GPU: ``dl4ds_label_objects`` (csrc/objects.hip) kernel by kernel next to ``dl4ds_scaler_stats``, the
one-read floor, over the same device array in the same run, and ``sal_scores`` from host arrays next to scipy.ndimage on the host.

Kernel: (64, 512, 512, 1) uniform random fields, thresholds 1 - density for event densities 0.05, 0.4, 0.6 (near the 4-neighbour
percolation point 0.593: the longest union chains) and 0.95, connectivity 1 and 2, cap 4096, with and without ``labels``.  After a
warm-up, alternating repetitions of the entry and of dl4ds_scaler_stats; kernel times from the profiler's per-launch timestamps
(tags ``objects_init`` ... ``objects_finish``, ``scaler_stats``).  ``cell_bytes`` is the entry's algorithmic traffic per cell (4 B
read, twice with tables; the 8 B workspace written once and read by flatten, number and gather; 4 B of labels), ``tbs`` that
traffic over the entry's kernel time and ``of_6p3`` its share of the 6.3 TB/s the project measured for streaming reads.

Host: ``sal_scores`` of (16, 512, 512, 1) gamma fields (upload included) at the default factor; scipy.ndimage.label +
ndimage.sum + ndimage.maximum on the first two samples of both sides, and their counts compared.

Every GPU step is a child process under a time limit of its own; the first one that fails ends the run.

    python tools/bench_objects.py [out.json]
"""
import ctypes
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np

STREAM_TBS = 6.3
STEPS = (('kernel', 300), ('host', 300))


def kernel_step():
    import dl4ds_amd._lib as L
    from dl4ds_amd.device import DeviceArray
    lib = L.lib()
    N, H, W, C, cap, runs = 64, 512, 512, 1, 4096, 3
    F, n = N * C, N * H * W * C
    x = DeviceArray.from_numpy(np.random.default_rng(1).random((N, H, W, C), np.float32))
    labels, count, nvalid, fsum = DeviceArray((F, H, W), np.int32), DeviceArray((F,), np.int32), DeviceArray((F,), np.int64), DeviceArray((F, 3), np.float64)
    sums, bbox, first = DeviceArray((F, cap, 6), np.int64), DeviceArray((F, cap, 4), np.int32), DeviceArray((F, cap), np.int32)
    vmax, mass, thr = DeviceArray((F, cap)), DeviceArray((F, cap, 3), np.float64), DeviceArray((F,))
    st_out, st_flag = DeviceArray((5, 1), np.float64), DeviceArray((1,), np.uint32)
    cshape, cflags = (ctypes.c_size_t * 1)(n), (ctypes.c_int * 1)(1)
    floor = lambda: L.check(lib.dl4ds_scaler_stats(x.ptr, 0, cshape, 1, cflags, st_out.ptr, st_flag.ptr, None))  # noqa: E731
    tags = ('init', 'merge', 'flatten', 'field', 'number', 'gather', 'finish')
    rows = []
    for density in (0.05, 0.4, 0.6, 0.95):
        thr.upload(np.full(F, 1.0 - density, np.float32))
        for connectivity in (1, 2):
            for with_labels in (True, False):
                entry = lambda: L.check(lib.dl4ds_label_objects(x.ptr, N, H, W, C, thr.ptr, connectivity, cap,  # noqa: E731
                                                                labels.ptr if with_labels else None, count.ptr, nvalid.ptr, fsum.ptr,
                                                                sums.ptr, bbox.ptr, first.ptr, vmax.ptr, mass.ptr))
                entry()
                floor()
                L.check(lib.dl4ds_sync())
                L.check(lib.dl4ds_profile_enable(1))
                for _ in range(runs):
                    entry()
                    floor()
                buf = ctypes.create_string_buffer(1 << 16)
                L.check(lib.dl4ds_profile_report(buf, len(buf)))
                rep = json.loads(buf.value.decode())
                L.check(lib.dl4ds_profile_enable(0))
                L.check(lib.dl4ds_sync())
                ms = {t: rep['objects_' + t]['ms'] / runs for t in tags}
                total, stats = sum(ms.values()), rep['scaler_stats']['ms'] / runs
                cell_bytes = 4 + 4 + 8 + 3 * 4 + 2 * 4 + (4 if with_labels else 0)      # x twice, workspace written, parent x 3, rootlabel x 2
                c = count.numpy()
                rows.append(dict(density=density, connectivity=connectivity, labels=with_labels, shape=[N, H, W, C], cap=cap,
                                 kernel_ms={t: round(v, 4) for t, v in ms.items()}, entry_ms=round(total, 4),
                                 scaler_stats_ms=round(stats, 4), ratio_entry_over_one_read=round(total / stats, 2),
                                 cell_bytes=cell_bytes, tbs=round(cell_bytes * n / total / 1e9, 3),
                                 of_6p3=round(cell_bytes * n / total / 1e9 / STREAM_TBS, 3),
                                 gather_tbs=round((12 if with_labels else 8) * n / ms['gather'] / 1e9, 3),
                                 objects_per_field=round(float(c.mean()), 1), fields_beyond_cap=int((c > cap).sum())))
    return dict(device=L.device_name(), kernel=rows)


def host_step():
    from scipy import ndimage
    from dl4ds_amd.objects import SAL_DEFAULT_FACTOR, factor_thresholds, sal_scores
    N, H, W, subset = 16, 512, 512, 2
    rng = np.random.default_rng(2)
    obs, pred = (rng.gamma(0.5, 2.0, (N, H, W, 1)).astype(np.float32) for _ in range(2))
    sal_scores(obs, pred)
    t_dev = []
    for _ in range(3):
        t0 = time.perf_counter()
        got = sal_scores(obs, pred)
        t_dev.append(time.perf_counter() - t0)
    t0 = time.perf_counter()
    counts = []
    for side in (obs, pred):
        thr = factor_thresholds(side[:subset], SAL_DEFAULT_FACTOR)
        for k in range(subset):
            v = side[k, :, :, 0]
            lab, n = ndimage.label(v >= thr[k])
            idx = np.arange(1, n + 1)
            ndimage.sum(v, lab, idx), ndimage.maximum(v, lab, idx), ndimage.center_of_mass(v, lab, idx)
            counts.append(n)
    t_ref = time.perf_counter() - t0
    assert counts == got['n_objects_obs'][:subset, 0].tolist() + got['n_objects_pred'][:subset, 0].tolist()
    return dict(host=dict(n_samples=N, sample_shape=[H, W, 1], factor=SAL_DEFAULT_FACTOR, sal_scores_s=round(float(np.median(t_dev)), 4),
                          scipy_samples=subset, scipy_label_sum_max_com_s=round(t_ref, 4),
                          scipy_s_scaled_to_all_samples=round(t_ref * N / subset, 4), truncated=bool(got['truncated']),
                          objects_per_field=round(float(got['n_objects_obs'].mean()), 1)))


if __name__ == '__main__':
    if len(sys.argv) > 2 and sys.argv[1] == '--step':
        print(json.dumps(dict(kernel=kernel_step, host=host_step)[sys.argv[2]]()))
        sys.exit(0)
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, 'profiles', 'objects.json')
    result = dict(bench='objects')
    for step, limit in STEPS:                                               # a failure or a time limit ends the run: nothing more starts
        r = subprocess.run([sys.executable, os.path.abspath(__file__), '--step', step], capture_output=True, text=True, timeout=limit)
        if r.returncode != 0:
            sys.stderr.write(r.stdout + r.stderr)
            sys.exit(f'bench_objects: step {step} ended with status {r.returncode}')
        result.update(json.loads(r.stdout.strip().splitlines()[-1]))
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, 'w') as f:
        json.dump(result, f, indent=1)
    print(json.dumps(result))
