"""`Model.predict` next to `Model.predict_tiled` on BASELINE configs[1] (residual backbone, sub-pixel post-upsampling
4x, 204405 parameters) -> profiles/tiled_predict.json.       python tools/bench_tiled.py [out.json]

In ONE process, after a warm-up of each path:
  * own grid: 8 LR fields of 128 x 128 -> 512 x 512, `predict` (the graph the model was built with) and `predict_tiled` with 64-pixel
    tiles, crop, halo = receptive_halo (two passes over the tiles: the tail's channel attention needs the field's means);
  * a domain four times larger per axis: 8 LR fields of 512 x 512 -> 2048 x 2048, `predict` (a sibling graph for the full grid, batch
    8; MemoryError / a refused allocation is recorded if it does not fit) and `predict_tiled` with 128-pixel tiles (the model's own graph);
  * both with numpy arrays in and out, wall clock around the call, the best of `REPS` repetitions; the largest relative difference of
    the two results;
  * peak device memory of either path: hipMemGetInfo after every dl4ds_graph_forward of the run (all buffers of a run are allocated
    before its first forward pass), less what was in use before the run's own model was built;
  * the merge kernel alone: 32 HR tiles of 512 x 512 x 1 of the large plan into the 2048 x 2048 field (HIP events on the library stream),
    its rate on the bytes it touches (12 per element with a non-zero weight: tile read, output read and write) next to the 6.3 TB/s
    HBM figure and next to dl4ds_memcpy_d2d moving the same number of bytes (half of them read, half written)."""
import ctypes
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_TBPS = 6.3
REPS = 3


def main(out_path):
    import dl4ds_amd._lib as L
    import dl4ds_amd.models as PM
    from dl4ds_amd.device import DeviceArray
    from dl4ds_amd.tiling import plan_tiles, tile_list
    lib = L.lib()
    hip = ctypes.CDLL('libamdhip64.so')

    def used():
        free, total = ctypes.c_size_t(), ctypes.c_size_t()
        assert hip.hipMemGetInfo(ctypes.byref(free), ctypes.byref(total)) == 0
        return total.value - free.value

    import gc
    build = lambda: PM.net_postupsampling('resnet', 'spc', 4, 1, 0, (128, 128), seed=7)
    model = build()
    halo = model.receptive_halo
    peak, base = [0], [0]
    forward = lib.dl4ds_graph_forward

    def watched(*a):
        st = forward(*a)
        peak[0] = max(peak[0], used() - base[0])
        return st
    lib.dl4ds_graph_forward = watched

    def timed(call):
        # a model of its own per measurement (same seed, same weights), so that no graph of the other path is alive while the peak is read
        gc.collect()
        L.check(lib.dl4ds_sync())
        base[0], peak[0] = used(), 0
        m = build()
        call(m)                                                # warm-up: sibling graph, filter cache, page faults of the result
        best, res = None, None
        for _ in range(REPS):
            t0 = time.perf_counter()
            res = call(m)
            dt = time.perf_counter() - t0
            best = dt if best is None else min(best, dt)
        top = peak[0]
        del m
        return res, best, top

    rng = np.random.default_rng(1)
    rec = {'model': 'BASELINE configs[1]: net_postupsampling(resnet, spc, scale=4), built for lr 128 x 128', 'device': L.device_name(),
           'receptive_halo': halo, 'tile_align': model.tile_align, 'reps': REPS, 'timing': 'wall clock around the call, numpy in and out, best of reps'}
    for key, grid, tile in (('own_grid', 128, 64), ('four_times_per_axis', 512, 128)):
        x = rng.standard_normal((8, grid, grid, 1)).astype(np.float32)
        plan = plan_tiles(grid, tile, halo, model.tile_align, 'crop', 4)
        r = {'lr_grid': [grid, grid], 'hr_grid': [4 * grid, 4 * grid], 'samples': 8, 'tile': tile, 'blend': 'crop', 'halo': halo,
             'tiles_per_sample': len(plan[0].origins) * len(plan[1].origins), 'origins': [int(o) for o in plan[0].origins]}
        full = None
        try:
            full, dt, mem = timed(lambda m: m.predict(x, batch_size=8))
            r['predict'] = {'s': dt, 'hr_samples_per_s': 8 / dt, 'peak_device_bytes': mem, 'batch_size': 8}
        except (MemoryError, L.Dl4dsHipError) as e:
            r['predict'] = {'does_not_fit': str(e)}
        out, dt, mem = timed(lambda m: m.predict_tiled(x, tile, blend='crop', batch_size=32))
        r['predict_tiled'] = {'s': dt, 'hr_samples_per_s': 8 / dt, 'peak_device_bytes': mem, 'batch_size': 32, 'passes': 2}
        if full is not None:
            r['max_abs_diff_over_max_abs'] = float(np.abs(out - full).max() / np.abs(full).max())
            r['tiled_over_full_time'] = r['predict_tiled']['s'] / r['predict']['s']
            r['tiled_over_full_peak_bytes'] = r['predict_tiled']['peak_device_bytes'] / max(r['predict']['peak_device_bytes'], 1)
        rec[key] = r
    lib.dl4ds_graph_forward = forward

    # ---- the merge kernel alone
    plan = plan_tiles(512, 128, halo, model.tile_align, 'crop', 4)
    iy, ix = tile_list(plan)
    n, th = 32, 512
    iy, ix = iy[:n], ix[:n]
    i32 = lambda a: np.ascontiguousarray(a, np.int32)
    oy, ox, smp = i32(plan[0].origins[iy] * 4), i32(plan[1].origins[ix] * 4), i32(np.zeros(n))
    ry, rx = i32(iy), i32(ix)
    tiles = DeviceArray.from_numpy(rng.standard_normal((n, th, th, 1)).astype(np.float32))
    field = DeviceArray.zeros((1, 2048, 2048, 1))
    wy, wx = DeviceArray.from_numpy(plan[0].weights), DeviceArray.from_numpy(plan[1].weights)
    touched = sum(int(np.count_nonzero(plan[0].weights[a])) * int(np.count_nonzero(plan[1].weights[b])) for a, b in zip(iy, ix))
    nbytes = 12 * touched

    def event_ms(fn, reps=20):
        fn()
        ms = ctypes.c_float()
        L.check(lib.dl4ds_event_timer_start())
        for _ in range(reps):
            fn()
        L.check(lib.dl4ds_event_timer_stop(ctypes.byref(ms)))
        return ms.value / reps
    merge = lambda: L.check(lib.dl4ds_tile_merge(tiles.ptr, n, th, th, 1, oy.ctypes.data, ox.ctypes.data, smp.ctypes.data, ry.ctypes.data,
                                                 rx.ctypes.data, wy.ptr, plan[0].weights.shape[0], wx.ptr, plan[1].weights.shape[0],
                                                 field.ptr, 1, 2048, 2048))
    ms_merge = event_ms(merge)
    half = nbytes // 2 // 4 * 4
    src, dst = DeviceArray((half // 4,)), DeviceArray((half // 4,))
    ms_copy = event_ms(lambda: L.check(lib.dl4ds_memcpy_d2d(dst.ptr, src.ptr, half)))
    rec['merge_kernel'] = {'tiles': n, 'tile': [th, th, 1], 'field': [2048, 2048, 1], 'blend': 'crop', 'elements_with_weight': touched,
                           'bytes': nbytes, 'ms': ms_merge, 'tbps': nbytes / (ms_merge * 1e-3) / 1e12,
                           'frac_of_hbm_6p3': nbytes / (ms_merge * 1e-3) / 1e12 / HBM_TBPS,
                           'memcpy_d2d': {'bytes_moved': 2 * half, 'ms': ms_copy, 'tbps': 2 * half / (ms_copy * 1e-3) / 1e12},
                           'merge_over_memcpy_time': ms_merge / ms_copy}
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    json.dump(rec, open(out_path, 'w'), indent=1)
    print(json.dumps(rec))


if __name__ == '__main__':
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, 'profiles', 'tiled_predict.json'))
