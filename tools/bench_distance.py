"""Distance-map verification on one GPU: ``dl4ds_distance_scores`` (csrc/distance.hip) kernel by kernel next to
``dl4ds_scaler_stats``, the one-read floor, and ``dl4ds_fss`` at one window over the same device arrays in the same run, and
``distance_scores`` from host arrays next to scipy.ndimage.distance_transform_edt on the host.

Kernel: (64, 512, 512, 1) uniform random fields, event densities 0.001, 0.05 and 0.5 and a field without any event (the early exit
of the row scan makes the time depend on the density), T = 1 and T = 8 thresholds (at T = 8 the densities run from the stated one
down to 0.56 of it), with and without the two squared maps.  After a warm-up, alternating repetitions of the entry, of
dl4ds_scaler_stats and of dl4ds_fss (window 9, the first threshold); kernel times from the profiler's per-launch timestamps (tags
``distance_col``, ``distance_row``, ``distance_final``, ``scaler_stats``, ``fss_prefix``, ``fss_window``).  ``cell_bytes`` is the
entry's algorithmic traffic per cell: 8 B of y and p per group of 8 thresholds, per threshold the two 2-byte vertical distances
written once and read twice (the upward walk, the row pass; rewrites are not counted) and 4 B per map wanted; ``tbs`` is that
traffic over the entry's kernel time and ``of_6p3`` its share of the 6.3 TB/s the project measured for streaming reads.

Host: ``distance_scores`` of (16, 512, 512, 1) uniform fields at density 0.05 (upload included); scipy's transform of both sides
of the first two samples, and the squared maps compared.

Every GPU step is a child process under a time limit of its own; the first one that fails ends the run.

    python tools/bench_distance.py [out.json]
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
STEPS = (('kernel', 600), ('host', 300))


def kernel_step():
    import dl4ds_amd._lib as L
    from dl4ds_amd.device import DeviceArray
    lib = L.lib()
    N, H, W, C, runs, TMAX = 64, 512, 512, 1, 3, 8
    F, n = N * C, N * H * W * C
    rng = np.random.default_rng(1)
    y, p = (DeviceArray.from_numpy(rng.random((N, H, W, C), np.float32)) for _ in range(2))
    counts, sums = DeviceArray((F, TMAX, 8), np.int64), DeviceArray((F, TMAX, 7), np.float64)
    maps = [DeviceArray((F, TMAX, H, W), np.int32) for _ in range(2)]
    st_out, st_flag = DeviceArray((5, 1), np.float64), DeviceArray((1,), np.uint32)
    cshape, cflags = (ctypes.c_size_t * 1)(n), (ctypes.c_int * 1)(1)
    fsums, fcont, fvalid = DeviceArray((F, 1, 1, 3), np.int64), DeviceArray((F, 1, 4), np.int64), DeviceArray((F,), np.int64)
    window = np.array([9], np.int32)
    cutoff, alpha = float(np.hypot(H - 1, W - 1)), 1.0 / 9.0
    floor = lambda: L.check(lib.dl4ds_scaler_stats(y.ptr, 0, cshape, 1, cflags, st_out.ptr, st_flag.ptr, None))  # noqa: E731
    tags = ('col', 'row', 'final')
    rows = []
    for density in (0.001, 0.05, 0.5, 0.0):
        for T in (1, TMAX):
            thr = np.array([1.0 - density * (1.0 - k / 16.0) if density else 2.0 + k for k in range(T)], np.float32)
            fss = lambda: L.check(lib.dl4ds_fss(y.ptr, p.ptr, N, H, W, C, thr.ctypes.data, 1, window.ctypes.data, 1,  # noqa: E731
                                                fsums.ptr, fcont.ptr, fvalid.ptr))
            for with_maps in (True, False):
                m = [d.ptr if with_maps else None for d in maps]
                entry = lambda: L.check(lib.dl4ds_distance_scores(y.ptr, p.ptr, N, H, W, C, thr.ctypes.data, T, cutoff, alpha,  # noqa: E731
                                                                  counts.ptr, sums.ptr, m[0], m[1]))
                entry()
                floor()
                fss()
                L.check(lib.dl4ds_sync())
                L.check(lib.dl4ds_profile_enable(1))
                for _ in range(runs):
                    entry()
                    floor()
                    fss()
                buf = ctypes.create_string_buffer(1 << 16)
                L.check(lib.dl4ds_profile_report(buf, len(buf)))
                rep = json.loads(buf.value.decode())
                L.check(lib.dl4ds_profile_enable(0))
                L.check(lib.dl4ds_sync())
                ms = {t: rep['distance_' + t]['ms'] / runs for t in tags}
                total, stats = sum(ms.values()), rep['scaler_stats']['ms'] / runs
                fss_ms = (rep['fss_prefix']['ms'] + rep['fss_window']['ms']) / runs
                cell_bytes = 8 + T * (2 * 2 * 3 + (8 if with_maps else 0))
                c = counts.numpy().reshape(-1)[:F * T * 8].reshape(F, T, 8)          # (the entry's layout is [F][T][8] for the T of the call)
                rows.append(dict(density=density, T=T, maps=with_maps, shape=[N, H, W, C],
                                 kernel_ms={t: round(v, 4) for t, v in ms.items()}, entry_ms=round(total, 4),
                                 scaler_stats_ms=round(stats, 4), fss_one_window_ms=round(fss_ms, 4),
                                 ratio_entry_over_one_read=round(total / stats, 2), cell_bytes=cell_bytes,
                                 tbs=round(cell_bytes * n / total / 1e9, 3), of_6p3=round(cell_bytes * n / total / 1e9 / STREAM_TBS, 3),
                                 ns_per_cell_and_threshold=round(total * 1e6 / (n * T), 5),
                                 events_per_field=round(float(c[..., 1].mean()), 1)))
    return dict(device=L.device_name(), kernel=rows)


def host_step():
    from scipy import ndimage
    from dl4ds_amd.distance import distance_scores
    N, H, W, subset, thr = 16, 512, 512, 2, 0.95
    rng = np.random.default_rng(2)
    obs, pred = (rng.random((N, H, W, 1), np.float32) for _ in range(2))
    distance_scores(obs, pred, thr)
    t_dev = []
    for _ in range(3):
        t0 = time.perf_counter()
        got = distance_scores(obs, pred, thr, return_maps=True)
        t_dev.append(time.perf_counter() - t0)
    t0 = time.perf_counter()
    ref = [[ndimage.distance_transform_edt(~(side[k, :, :, 0] >= np.float32(thr))) for k in range(subset)] for side in (obs, pred)]
    t_ref = time.perf_counter() - t0
    for side, key in enumerate(('d2_obs', 'd2_pred')):
        for k in range(subset):
            assert (np.rint(ref[side][k] ** 2) == got[key][k, 0, 0]).all()
    return dict(host=dict(n_samples=N, sample_shape=[H, W, 1], threshold=thr, maps=True,
                          distance_scores_s=round(float(np.median(t_dev)), 4), scipy_samples=subset,
                          scipy_edt_both_sides_s=round(t_ref, 4), scipy_s_scaled_to_all_samples=round(t_ref * N / subset, 4),
                          hausdorff_mean=float(got['hausdorff_mean'][0])))


if __name__ == '__main__':
    if len(sys.argv) > 2 and sys.argv[1] == '--step':
        print(json.dumps(dict(kernel=kernel_step, host=host_step)[sys.argv[2]]()))
        sys.exit(0)
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, 'profiles', 'distance.json')
    result = dict(bench='distance')
    for step, limit in STEPS:                                               # a failure or a time limit ends the run: nothing more starts
        r = subprocess.run([sys.executable, os.path.abspath(__file__), '--step', step], capture_output=True, text=True, timeout=limit)
        if r.returncode != 0:
            sys.stderr.write(r.stdout + r.stderr)
            sys.exit(f'bench_distance: step {step} ended with status {r.returncode}')
        result.update(json.loads(r.stdout.strip().splitlines()[-1]))
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, 'w') as f:
        json.dump(result, f, indent=1)
    print(json.dumps(result))
