"""Regridding on one GPU (csrc/regrid.hip): ``dl4ds_regrid_apply`` for a conservative 512^2 -> 128^2 coarsening
and a bilinear 128^2 -> 512^2 refinement of (64, ., ., 1) fields, and ``dl4ds_regrid_consistency`` on the first of the two, each
next to ``dl4ds_memcpy_d2d`` and ``dl4ds_scaler_apply`` (one multiply) moving the same number of bytes, in the same run.

``bytes`` is the algorithmic traffic: one read of the input and one write of the output for apply, one read of the fine field and
of the coarse reference for consistency (its sums are a few KiB).  The copy and the scaler move bytes / 2 in and bytes / 2 out.
After a warm-up the three run in alternating rounds of ``INNER`` launches between two device events; ``ms`` is the median round
over its launches, ``tbs`` = bytes / ms and ``of_6p3`` its share of the 6.3 TB/s the project measured for streaming copies.  The
arrays (64 MiB + 4 MiB) fit the 256 MiB Infinity Cache, for the copy and the scaler as for the regridding: the figures compare the
three at that size and are no HBM rates.

The GPU work runs in one child process under a time limit; a failure ends the run.

    python tools/bench_regrid.py [out.json]
"""
import ctypes
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np

STREAM_TBS = 6.3
ROUNDS, INNER = 7, 20


def kernel_step():
    import dl4ds_amd._lib as L
    from dl4ds_amd.device import DeviceArray
    from dl4ds_amd.regrid import Regridder
    lib = L.lib()
    N, C, HR, LR = 64, 1, 512, 128
    rng = np.random.default_rng(1)
    fine = DeviceArray.from_numpy(rng.standard_normal((N, HR, HR, C)).astype(np.float32))
    coarse = DeviceArray.from_numpy(rng.standard_normal((N, LR, LR, C)).astype(np.float32))
    fine_out, coarse_out = DeviceArray((N, HR, HR, C)), DeviceArray((N, LR, LR, C))
    sums, counts = DeviceArray((N, C, 6), np.float64), DeviceArray((N, C, 2), np.int64)
    factor = DeviceArray.from_numpy(np.array([1.5], np.float32))
    down = Regridder.from_scale((HR, HR), 4, method='conservative')
    up = Regridder.from_scale((HR, HR), 4, method='bilinear', refine=True)

    def timed(fn):
        ms = ctypes.c_float()
        L.check(lib.dl4ds_event_timer_start())
        for _ in range(INNER):
            fn()
        L.check(lib.dl4ds_event_timer_stop(ctypes.byref(ms)))
        return ms.value / INNER

    def same_bytes(nbytes):
        n = nbytes // 8                                                  # floats read = floats written
        shape, reduce = (ctypes.c_size_t * 1)(n), (ctypes.c_int * 1)(1)
        copy = lambda: L.check(lib.dl4ds_memcpy_d2d(fine_out.ptr, fine.ptr, n * 4))                          # noqa: E731
        scale = lambda: L.check(lib.dl4ds_scaler_apply(fine.ptr, fine_out.ptr, 0, shape, 1, reduce, 1, factor.ptr, 0, None, 0, 0.0,   # noqa: E731
                                                       None))
        return copy, scale

    n_f, n_c = N * HR * HR * C * 4, N * LR * LR * C * 4
    ops = (('conservative_512_to_128', n_f + n_c,
            lambda: L.check(lib.dl4ds_regrid_apply(down._handle(), fine.ptr, N, C, 0, 0.5, coarse_out.ptr))),
           ('bilinear_128_to_512', n_f + n_c,
            lambda: L.check(lib.dl4ds_regrid_apply(up._handle(), coarse.ptr, N, C, 0, 0.5, fine_out.ptr))),
           ('consistency_512_to_128', n_f + n_c,
            lambda: L.check(lib.dl4ds_regrid_consistency(down._handle(), fine.ptr, coarse.ptr, N, C, 0, 0.5, sums.ptr, counts.ptr, None))))
    rows = []
    for name, nbytes, entry in ops:
        copy, scale = same_bytes(nbytes)
        fns = dict(entry=entry, memcpy_d2d=copy, scaler_apply=scale)
        for fn in fns.values():
            for _ in range(3):
                fn()
        L.check(lib.dl4ds_sync())
        ms = {k: [] for k in fns}
        for _ in range(ROUNDS):
            for k, fn in fns.items():
                ms[k].append(timed(fn))
        med = {k: float(np.median(v)) for k, v in ms.items()}
        rate = lambda t: round(nbytes / t / 1e9, 3)                       # noqa: E731
        rows.append(dict(op=name, shape=[N, HR if 'to_128' in name else LR, HR if 'to_128' in name else LR, C], bytes=nbytes,
                         ms={k: round(v, 4) for k, v in med.items()}, spread_ms={k: [round(min(v), 4), round(max(v), 4)] for k, v in ms.items()},
                         tbs={k: rate(v) for k, v in med.items()}, of_6p3=round(nbytes / med['entry'] / 1e9 / STREAM_TBS, 3),
                         entry_over_copy=round(med['entry'] / med['memcpy_d2d'], 2)))
    down.close()
    up.close()
    return dict(device=L.device_name(), rounds=ROUNDS, launches_per_round=INNER, kernel=rows)


if __name__ == '__main__':
    if len(sys.argv) > 2 and sys.argv[1] == '--step':
        print(json.dumps(kernel_step()))
        sys.exit(0)
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, 'profiles', 'regrid.json')
    r = subprocess.run([sys.executable, os.path.abspath(__file__), '--step', 'kernel'], capture_output=True, text=True, timeout=300)
    if r.returncode != 0:
        sys.stderr.write(r.stdout + r.stderr)
        sys.exit(f'bench_regrid: the kernel step ended with status {r.returncode}')
    result = dict(bench='regrid', **json.loads(r.stdout.strip().splitlines()[-1]))
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, 'w') as f:
        json.dump(result, f, indent=1)
    print(json.dumps(result))
