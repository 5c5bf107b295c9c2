"""Quantile-mapping bias correction on one GPU, one JSON line, also written to profiles/qmap.json.  Data: a year of daily
512 x 512 x 1 temperature-like fields (365, 512, 512, 1), Q = 101 probabilities; the observation and the model's history have the
same shape.  Everything is measured in one run:

* ``map``: dl4ds_qmap_apply on the device-resident array after warm-up, EQM and QDM, additive.  ``kernel_ms``: kernel time of one
  call from the library profiler (per-launch timestamps); ``wall_ms``: host time of the call bracketed by device syncs;
  ``stream_bytes`` = 8 B per element (one read, one write), ``stream_tb_s`` = those bytes over the kernel time, next to
  ``hbm_peak_tb_s``, the project's 6.3 TB/s figure; ``table_bytes`` = 4 * Q B per cell and table in use, read once per workgroup.
* ``scaler_apply``: dl4ds_scaler_apply (x - mean) / std per cell on the same array: a streaming kernel with the same 8 B per
  element, the yardstick; ``map_over_scaler`` = map kernel time / scaler kernel time.
* ``fit``: dl4ds_quantile_table of one array next to dl4ds_distribution over time of the pair (observation, model) with the same
  probabilities (its cap is 64, so it gets every other one of the 101: 51) on the same data; both sort 365 samples per cell in LDS.
* ``mapper``: QuantileMapper.fit and .transform from host arrays (uploads, downloads and host copies included).
* ``numpy``: tests/qmap_ref.py, the restatement (np.sort along time, vectorised gathers), on ``numpy.cells`` whole grid rows,
  extrapolated to the grid; it agrees bit for bit with the device on that subset (asserted).

    python tools/bench_qmap.py [reps] [output.json]
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
from dl4ds_amd.postprocessing import QuantileMapper
from tests import qmap_ref

HBM_PEAK = 6.3e12
N, H, W, C = 365, 512, 512, 1
Q = 101
CPU_ROWS = 4
reps = int(sys.argv[1]) if len(sys.argv) > 1 else 5
out_path = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, 'profiles', 'qmap.json')
q = np.linspace(0.0, 1.0, Q)
per = H * W * C
lib = L.lib()


def fields(seed, shift, scale):
    r = np.random.default_rng(seed)
    out = np.empty((N, H, W, C), np.float32)
    for n in range(N):
        out[n] = 280.0 + shift + scale * r.standard_normal((H, W, C), np.float32)
    return out


def timed(call, tag):
    """-> (kernel ms, wall ms) of one call"""
    for _ in range(2):
        call()
    L.check(lib.dl4ds_sync())
    t0 = time.perf_counter()
    for _ in range(reps):
        call()
    L.check(lib.dl4ds_sync())
    wall = (time.perf_counter() - t0) / reps
    L.check(lib.dl4ds_profile_enable(1))
    for _ in range(reps):
        call()
    buf = ctypes.create_string_buffer(1 << 16)
    L.check(lib.dl4ds_profile_report(buf, len(buf)))
    L.check(lib.dl4ds_profile_enable(0))
    return json.loads(buf.value.decode())[tag]['ms'] / reps, 1e3 * wall


obs, model, future = fields(0, 0.0, 8.0), fields(1, 3.0, 10.0), fields(2, 5.0, 10.0)
d_obs, d_model, d_x = (DeviceArray.from_numpy(a) for a in (obs, model, future))
d_out = DeviceArray((N, per))
tabs = {k: DeviceArray((Q, per)) for k in 'omf'}
valid = DeviceArray((per,), np.int64)

# ---- fit
fit = {}
for name, src in (('o', d_obs), ('m', d_model), ('f', d_x)):
    call = lambda: L.check(lib.dl4ds_quantile_table(src.ptr, N, per, q.ctypes.data, Q, tabs[name].ptr, valid.ptr))
    if name == 'o':
        ms, wall = timed(call, 'quantile_table_strided')
        fit['quantile_table'] = dict(arrays=1, probabilities=Q, kernel_ms=round(ms, 3), wall_ms=round(wall, 3),
                                     input_read_tb_s=round(4 * N * per / (ms * 1e-3) / 1e12, 3))
    else:
        call()
q2 = np.ascontiguousarray(q[::2])
outs = [DeviceArray((per, 2, len(q2)), np.float64), DeviceArray((per,), np.float64), DeviceArray((per,), np.int64),
        DeviceArray((per,), np.int64)]
ms, wall = timed(lambda: L.check(lib.dl4ds_distribution(d_obs.ptr, d_model.ptr, per, N, 1, per, q2.ctypes.data, len(q2), None, 0,
                                                        outs[0].ptr, outs[1].ptr, outs[2].ptr, None, outs[3].ptr)),
                 'distribution_strided')
fit['distribution_over_time'] = dict(arrays=2, probabilities=len(q2), kernel_ms=round(ms, 3), wall_ms=round(wall, 3),
                                     input_read_tb_s=round(8 * N * per / (ms * 1e-3) / 1e12, 3))
for o in outs:
    o.free()

# ---- the map and its yardstick
counts = DeviceArray.zeros((4,), np.uint64)
stream = 8 * N * per
maps = {}
for method, target in (('eqm', None), ('qdm', tabs['f'].ptr)):
    ms, wall = timed(lambda: L.check(lib.dl4ds_qmap_apply(d_x.ptr, d_out.ptr, N, per, tabs['m'].ptr, tabs['o'].ptr, target, Q, 0, 0,
                                                          counts.ptr)), 'qmap_apply_' + method)
    maps[method] = dict(kernel_ms=round(ms, 3), wall_ms=round(wall, 3), stream_bytes=stream,
                        stream_tb_s=round(stream / (ms * 1e-3) / 1e12, 3), table_bytes=4 * Q * per * (2 if target is None else 3),
                        ns_per_element=round(1e6 * ms / (N * per), 5))
mean, std = DeviceArray.from_numpy(model.mean(0).ravel()), DeviceArray.from_numpy(model.std(0).ravel())
shape, reduce_ = (ctypes.c_size_t * 2)(N, per), (ctypes.c_int * 2)(1, 0)
ms_sc, wall_sc = timed(lambda: L.check(lib.dl4ds_scaler_apply(d_x.ptr, d_out.ptr, 0, shape, 2, reduce_, 3, mean.ptr, 4, std.ptr, 0, 0.0,
                                                              None)), 'scaler_apply')
scaler = dict(kernel_ms=round(ms_sc, 3), wall_ms=round(wall_sc, 3), stream_tb_s=round(stream / (ms_sc * 1e-3) / 1e12, 3))
for m in maps.values():
    m['map_over_scaler'] = round(m['kernel_ms'] / ms_sc, 2)

# ---- the restatement on a few grid rows, bit for bit
cells = CPU_ROWS * W * C
t0 = time.perf_counter()
want, want_counts, _ = qmap_ref.quantile_mapper(obs[:, :CPU_ROWS], model[:, :CPU_ROWS], future[:, :CPU_ROWS], q, 'qdm', '+')[:3]
t_ref = time.perf_counter() - t0
L.check(lib.dl4ds_qmap_apply(d_x.ptr, d_out.ptr, N, per, tabs['m'].ptr, tabs['o'].ptr, tabs['f'].ptr, Q, 0, 0, None))
got = d_out.numpy().reshape(N, H, W, C)[:, :CPU_ROWS]
assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
for d in (d_obs, d_model, d_x, d_out, valid, counts, mean, std) + tuple(tabs.values()):
    d.free()

# ---- the public object from host arrays
mapper = QuantileMapper(n_quantiles=Q, method='qdm')
mapper.fit(obs[:, :8], model[:, :8]).transform(future[:, :8])          # warm-up
t0 = time.perf_counter()
mapper.fit(obs, model)
t_fit = time.perf_counter() - t0
t0 = time.perf_counter()
out = mapper.transform(future)
t_tr = time.perf_counter() - t0
assert np.array_equal(out[:, :CPU_ROWS].view(np.uint32), want.view(np.uint32))

line = json.dumps(dict(bench='qmap', device_name=L.device_name(), shape=[N, H, W, C], probabilities=Q, reps=reps,
                       hbm_peak_tb_s=HBM_PEAK / 1e12, map=maps, scaler_apply=scaler, fit=fit,
                       mapper=dict(method='qdm', fit_wall_s=round(t_fit, 3), transform_wall_s=round(t_tr, 3),
                                   diagnostics=mapper.diagnostics_),
                       numpy=dict(omp_num_threads=os.environ.get('OMP_NUM_THREADS'), method='qdm', cells=cells,
                                  subset_s=round(t_ref, 3), extrapolated_s=round(t_ref * per / cells, 1), bits_equal=True)))
print(line)
os.makedirs(os.path.dirname(out_path), exist_ok=True)
with open(out_path, 'w') as f:
    f.write(line + '\n')
