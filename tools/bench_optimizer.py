"""Times the optimiser kernels and the optimiser's share of a step, all in ONE run, and writes profiles/optimizer.json.

    python tools/bench_optimizer.py [--reps 200] [--steps 20] [--warmup 5] [--batch 64] [--out profiles/optimizer.json]

Op level, on an arena of cfg2's parameter count (the library profiler's HIP events around every launch): dl4ds_op_adam -- the
yardstick: the same kernel as the parent commit's `adam` tag, measured in the same run -- and dl4ds_op_adam_ext with clipping only,
clipping + decay, and clipping + decay + average.  Each mode reports its bytes per parameter, its time per step and the rate of
those bytes next to the 6.3 TB/s the card reaches on long streams; cfg2's arena is under 1 MB, so every mode is a launch-latency
figure, and a second, 64 Mi-element arena shows the streaming rate of the same kernels.
Step level: a bench.py-shaped cfg2 step with the features off (the plain `adam` launch: the same code path as before the extensions
existed) and with all three on, wall clock over --steps steps after --warmup."""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
HBM_TBPS = 6.3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=200)
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--batch', type=int, default=64)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'optimizer.json'))
    args = ap.parse_args()
    import bench
    import dl4ds_amd._lib as L
    import dl4ds_amd.models as PM
    from dl4ds_amd.device import DeviceArray, sync
    from dl4ds_amd.training import SupervisedEngine
    lib = L.lib()

    def report():
        buf = ctypes.create_string_buffer(1 << 17)
        L.check(lib.dl4ds_profile_report(buf, len(buf)))
        return json.loads(buf.value.decode())

    model = PM.net_postupsampling('resnet', 'spc', 4, 1, 0, (128, 128), seed=7)
    n_arena = ctypes.c_size_t()
    n_par = ctypes.c_int()
    L.check(lib.dl4ds_graph_param_count(model.graph.h, ctypes.byref(n_arena), ctypes.byref(n_par)))
    kernels = model.graph.params
    from dl4ds_amd.training.engine import decayed_parameters
    dec = decayed_parameters(kernels)

    def op_level(n, ranges):
        rng = np.random.default_rng(0)
        w, g, m, e = (DeviceArray.from_numpy(rng.standard_normal(n).astype(np.float32)) for _ in range(4))
        v = DeviceArray.from_numpy(np.abs(rng.standard_normal(n)).astype(np.float32))
        st = DeviceArray.zeros((4,))
        r = np.ascontiguousarray(np.asarray(ranges, np.uint64).reshape(-1, 2))
        adam = (1, 1e-3, 0.9, 0.999, 1e-7, 1.0)
        modes = {
            'adam': (28, lambda: lib.dl4ds_op_adam(w.ptr, g.ptr, m.ptr, v.ptr, n, *adam)),
            'ext_clip': (32, lambda: lib.dl4ds_op_adam_ext(w.ptr, g.ptr, m.ptr, v.ptr, None, n, *adam, 1.0, 0.0, None, 0, 0.0, st.ptr)),
            'ext_clip_decay': (32, lambda: lib.dl4ds_op_adam_ext(w.ptr, g.ptr, m.ptr, v.ptr, None, n, *adam, 1.0, 1e-4, r.ctypes.data,
                                                                 len(r), 0.0, st.ptr)),
            'ext_clip_decay_ema': (40, lambda: lib.dl4ds_op_adam_ext(w.ptr, g.ptr, m.ptr, v.ptr, e.ptr, n, *adam, 1.0, 1e-4,
                                                                     r.ctypes.data, len(r), 0.99, st.ptr)),
        }
        out = {}
        for name, (bpp, call) in modes.items():
            for _ in range(10):
                L.check(call())
            L.check(lib.dl4ds_profile_filter(b'adam'))
            L.check(lib.dl4ds_profile_enable(1))
            for _ in range(args.reps):
                L.check(call())
            rep = report()
            L.check(lib.dl4ds_profile_enable(0))
            L.check(lib.dl4ds_profile_filter(b''))
            us = {k: 1e3 * x['ms'] / args.reps for k, x in rep.items()}
            tot = sum(us.values())
            out[name] = {'bytes_per_parameter': bpp, 'launches': len(us), 'us_per_step': round(tot, 3),
                         'us_by_tag': {k: round(x, 3) for k, x in us.items()},
                         'tb_per_s': round(bpp * n / (tot * 1e-6) / 1e12, 4), 'share_of_6.3_tb_per_s': round(bpp * n / (tot * 1e-6) / 1e12 / HBM_TBPS, 4)}
        for name in out:
            out[name]['vs_adam'] = round(out[name]['us_per_step'] / out['adam']['us_per_step'], 3)
        for d in (w, g, m, v, e, st):
            d.free()
        return out

    spans = []
    for k in dec:
        off, cnt = ctypes.c_size_t(), ctypes.c_size_t()
        L.check(lib.dl4ds_graph_param_info(model.graph.h, kernels[k]['pid'], ctypes.byref(off), ctypes.byref(cnt)))
        spans.append((off.value, off.value + cnt.value))
    from dl4ds_amd.ops import merge_ranges
    spans = merge_ranges(spans)
    res = {'device': L.device_name(), 'reps': args.reps, 'yardstick': "the `adam` row: dl4ds_op_adam, unchanged from the parent commit, same run",
           'cfg2_arena': {'elements': n_arena.value, 'decay_ranges': len(spans), 'modes': op_level(n_arena.value, spans)}}
    big = 64 << 20
    res['streaming_arena'] = {'elements': big, 'decay_ranges': 64,
                              'modes': op_level(big, [(k * (big // 64) + 1, (k + 1) * (big // 64) - 2) for k in range(64)])}
    del model

    def step_ms(**ext):
        mdl = PM.net_postupsampling('resnet', 'spc', 4, 1, 0, (128, 128), seed=7)
        eng = SupervisedEngine(mdl, loss='mae', learning_rate=(1e-3, 1e-4), lr_decay_after=1e5, **ext)
        x, y = bench.synthetic_batch(1002, args.batch)
        dx, dy = DeviceArray.from_numpy(x), DeviceArray.from_numpy(y)
        for _ in range(args.warmup):
            eng.step_device([dx.ptr], dy.ptr, args.batch)
        sync()
        t0 = time.perf_counter()
        for _ in range(args.steps):
            eng.step_device([dx.ptr], dy.ptr, args.batch)
        sync()
        ms = 1e3 * (time.perf_counter() - t0) / args.steps
        L.check(lib.dl4ds_profile_filter(b''))
        L.check(lib.dl4ds_profile_enable(1))
        for _ in range(3):
            eng.step_device([dx.ptr], dy.ptr, args.batch)
        rep = report()
        L.check(lib.dl4ds_profile_enable(0))
        tags = {k: round(1e3 * v['ms'] / 3, 3) for k, v in rep.items() if k.startswith(('adam', 'ema'))}
        return {'ms_per_step': round(ms, 4), 'optimiser_tags_us_per_step': tags, 'stats': eng.optimizer_stats()}

    off_a = step_ms()
    on = step_ms(global_clipnorm=1.0, weight_decay=1e-4, ema_momentum=0.99)
    off_b = step_ms()
    res['cfg2_step'] = {'batch': args.batch, 'steps': args.steps, 'features_off': off_a, 'features_on': on, 'features_off_again': off_b,
                        'note': 'features off runs the plain adam launch; the two off figures bracket the run-to-run noise'}
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, 'w') as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == '__main__':
    main()
