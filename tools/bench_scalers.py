"""MinMaxScaler / StandardScaler on one GPU: device time per fit and per transform on arrays resident in HBM.

For (365,512,512) [``small``] and (3650,512,512) [``large``] float32 with axis None / 0 / (1,2), plus (365,512,512,3) with
axis=(0,1,2): per-call device time from the profiler's per-launch timestamps after warm-up, as GB/s of algorithmic bytes (fit: one
read; transform: one read + one write) and as a fraction of the 6.3 TB/s a float4 copy sustains on this chip.  ``small`` also times
numpy's statement of the reference (np.nanmin + np.nanmax / np.nanmean + np.nanstd, and the two in-place passes) on the host.
One JSON line per row.  Each size is its own process: run them under their own `timeout`, chained with `&&`.

    python tools/bench_scalers.py small|large [reps]
"""
import ctypes
import json
import os
import sys
import time
import warnings

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

import dl4ds_amd._lib as L
from dl4ds_amd.device import DeviceArray
from dl4ds_amd.preprocessing import MinMaxScaler, StandardScaler

COPY_RATE = 6.3e12
which = sys.argv[1] if len(sys.argv) > 1 else 'small'
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 5
N = 365 if which == 'small' else 3650
lib = L.lib()


def device_ms(fn, scope):
    for _ in range(2):
        fn()
    L.check(lib.dl4ds_sync())
    L.check(lib.dl4ds_profile_enable(1))
    for _ in range(reps):
        fn()
    buf = ctypes.create_string_buffer(1 << 16)
    L.check(lib.dl4ds_profile_report(buf, len(buf)))
    L.check(lib.dl4ds_profile_enable(0))
    return json.loads(buf.value.decode())[scope]['ms'] / reps


def fill(shape):
    """kelvin-like field with 1 % NaNs, uploaded in slabs of five samples (the host never holds the large array)"""
    rng = np.random.default_rng(0)
    slab = (281.0 + 12.0 * rng.standard_normal((5,) + shape[1:])).astype(np.float32)
    slab[rng.random(slab.shape) < 0.01] = np.nan
    d = DeviceArray(shape, np.float32)
    per = slab.nbytes // 5
    for i in range(0, shape[0], 5):
        k = min(5, shape[0] - i)
        L.check(lib.dl4ds_memcpy_h2d(d.ptr + i * per, slab.ctypes.data, k * per))
    return d, slab


rows = [((N, 512, 512), None), ((N, 512, 512), 0), ((N, 512, 512), (1, 2))]
if which == 'small':
    rows.append(((N, 512, 512, 3), (0, 1, 2)))
for shape, axis in rows:
    dx, slab = fill(shape)
    nbytes = dx.nbytes
    for cls in (MinMaxScaler, StandardScaler):
        sc = cls(axis=axis)
        t_fit = device_ms(lambda: sc.partial_fit(dx), 'scaler_stats')
        out = {}
        t_tr = device_ms(lambda: out.__setitem__('y', sc.transform(dx)), 'scaler_apply')
        row = dict(bench='scalers', cls=cls.__name__, shape=list(shape), axis=axis, gb=round(nbytes / 1e9, 3),
                   fit_ms=round(t_fit, 3), fit_gbs=round(nbytes / t_fit / 1e6, 1),
                   fit_of_copy=round(nbytes / (t_fit * 1e-3) / COPY_RATE, 3),
                   transform_ms=round(t_tr, 3), transform_gbs=round(2 * nbytes / t_tr / 1e6, 1),
                   transform_of_copy=round(2 * nbytes / (t_tr * 1e-3) / COPY_RATE, 3))
        if which == 'small' and len(shape) == 3:
            x = np.tile(slab, (shape[0] // 5, 1, 1))
            with warnings.catch_warnings():
                warnings.simplefilter('ignore')
                t0 = time.perf_counter()
                if cls is MinMaxScaler:
                    np.nanmin(x, axis=axis, keepdims=True), np.nanmax(x, axis=axis, keepdims=True)
                else:
                    np.nanmean(x, axis=axis, keepdims=True), np.nanstd(x, axis=axis, keepdims=True)
                t1 = time.perf_counter()
                y = x.copy()
                y *= np.float32(0.5)
                y += np.float32(1.0)
                np.nan_to_num(y, nan=-1)
                t2 = time.perf_counter()
            row.update(numpy_fit_ms=round(1e3 * (t1 - t0), 1), numpy_transform_ms=round(1e3 * (t2 - t1), 1),
                       numpy_elements=int(x.size))
            del x, y
        print(json.dumps(row), flush=True)
        del out
    del dx
