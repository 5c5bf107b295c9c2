"""Spectral verification (binned power and cross spectra) on one GPU, one JSON line, also written to profiles/spectrum.json.
Data: N = 365 synthetic 512 x 512 x 1 fields (a smooth random field plus noise, the prediction a blurred copy) and 64 fields of
365 x 400, a grid that is no power of two; radial bins, detrended, no window.

* ``grids``: dl4ds_spectrum on device-resident arrays after warm-up, per grid: ``kernel_ms`` per stage of csrc/spectrum.hip from
  the library profiler (per-launch timestamps, summed over the chunks of one call), ``flops`` = the algorithmic fp64 count of the two
  matrix products (4 H W (W/2+1) + 8 H^2 (W/2+1) per field and side), ``tflops`` over the kernel time of those two stages and over
  all four, next to ``fp64_peak_tflops``, the public 78.6 TFLOP/s vector fp64 figure of the MI355X; ``wall_ms``: host time of the
  call bracketed by device syncs.
* ``spectral_scores_wall_s``: the whole call from host arrays (bin map, uploads, host arithmetic).
* ``cpu``: tests/spectrum_ref.py (np.fft.fft2 per field) on a stated subset of fields in the same run, scaled to all of them.

    python tools/bench_spectrum.py [reps] [output.json]
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
from dl4ds_amd.metrics import radial_bin_map, spectral_scores
from tests import spectrum_ref

FP64_PEAK = 78.6e12
STAGES = ('spectrum_prepare', 'spectrum_rows', 'spectrum_cols', 'spectrum_bins')
CPU_FIELDS = 4
reps = int(sys.argv[1]) if len(sys.argv) > 1 else 5
out_path = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, 'profiles', 'spectrum.json')
lib = L.lib()


def pair(seed, shape):
    """a red-noise field (white noise smoothed along both axes by a running mean) plus white noise; the prediction keeps the
    smooth part and loses most of the noise, as a network trained on MAE does"""
    rng = np.random.default_rng(seed)
    white = rng.standard_normal(shape).astype(np.float32)
    smooth = white.copy()
    for axis in (1, 2):
        smooth = sum(np.roll(smooth, s, axis) for s in range(-4, 5)) / np.float32(9)
    y = (3.0 * smooth + 0.3 * white).astype(np.float32)
    p = (3.0 * smooth + 0.05 * rng.standard_normal(shape)).astype(np.float32)
    return y, p


def device_call(y, p):
    N, H, W, C = y.shape
    full, B = radial_bin_map(H, W)
    half = np.ascontiguousarray(full[:, :W // 2 + 1])
    dy, dp = DeviceArray.from_numpy(y), DeviceArray.from_numpy(p)
    outs = [DeviceArray((N * C, 4, B), np.float64), DeviceArray((N * C,), np.int64), DeviceArray((N * C, 2), np.float64)]
    call = lambda: L.check(lib.dl4ds_spectrum(dy.ptr, dp.ptr, N, H, W, C, 1, 0, half.ctypes.data, B, *(o.ptr for o in outs)))
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
    rep = json.loads(buf.value.decode())
    ms = {k: rep[k]['ms'] / reps for k in STAGES}
    for d in [dy, dp] + outs:
        d.free()
    wh = W // 2 + 1
    flops = 2.0 * N * C * (4.0 * H * W * wh + 8.0 * H * H * wh)
    gemm_ms, all_ms = ms['spectrum_rows'] + ms['spectrum_cols'], sum(ms.values())
    return dict(shape=[N, H, W, C], bins=B, kernel_ms={k: round(v, 3) for k, v in ms.items()}, kernel_ms_total=round(all_ms, 3),
                wall_ms=round(1e3 * wall, 3), flops=flops, tflops_matrix_stages=round(flops / (gemm_ms * 1e-3) / 1e12, 2),
                tflops_all_stages=round(flops / (all_ms * 1e-3) / 1e12, 2),
                fraction_of_fp64_peak=round(flops / (all_ms * 1e-3) / FP64_PEAK, 3))


def whole_call(y, p):
    spectral_scores(y[:2], p[:2])                                  # warm-up
    t0 = time.perf_counter()
    r = spectral_scores(y, p)
    wall = time.perf_counter() - t0
    t0 = time.perf_counter()
    ref, power, T = spectrum_ref.spectral_scores(y[:CPU_FIELDS], p[:CPU_FIELDS])
    t_ref = time.perf_counter() - t0
    rel = float(np.max(np.abs(r['power_obs'][:CPU_FIELDS] - ref['power_obs']) / ref['power_obs'].max()))
    return r, dict(spectral_scores_wall_s=round(wall, 3),
                   cpu=dict(omp_num_threads=os.environ.get('OMP_NUM_THREADS'), subset_fields=CPU_FIELDS, subset_s=round(t_ref, 3),
                            extrapolated_s=round(t_ref * y.shape[0] * y.shape[3] / CPU_FIELDS, 1),
                            max_diff_power_obs_over_largest_power=rel),
                   effective_wavelength=r['effective_wavelength'].tolist(), lsd_pooled=r['lsd_pooled'].tolist())


grids = []
for seed, shape in ((0, (365, 512, 512, 1)), (1, (64, 365, 400, 1))):
    y, p = pair(seed, shape)
    g = device_call(y, p)
    g.update(whole_call(y, p)[1])
    grids.append(g)
    del y, p
line = json.dumps(dict(bench='spectrum', device_name=L.device_name(), reps=reps, fp64_peak_tflops=FP64_PEAK / 1e12,
                       kernel_form='LDS-tiled fp64 FMA (no MFMA)', grids=grids))
print(line)
os.makedirs(os.path.dirname(out_path), exist_ok=True)
with open(out_path, 'w') as f:
    f.write(line + '\n')
