"""Case tables and input builders of tests/test_gpu_head.py (not a test module; needs no GPU).  tests/test_head_oracle.py checks, on
the CPU, every condition the GPU tests rely on: the dispatch restated here against the source, no ReLU pre-activation within 1e-4
of 0, the independence bounds for exactly the seeds used."""
import os
import re

import numpy as np

from tests import head_ref as R

F32, F64 = np.float32, np.float64
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KINK_MARGIN = 1e-4


def source(name):
    return open(os.path.join(ROOT, 'dl4ds_amd', 'csrc', name)).read()


# ---------------------------------------------------------------------------------------------------------------- noise
# ew_blocks of csrc/head.hip: at most 4096 blocks of 256 threads; a mask with more elements runs the grid-stride loop a second time
NOISE_GRID_THREADS = 4096 * 256
LARGE_MASK = (2, 96, 96, 64)          # B, H, W, C: 1 179 648 elements
SMALL_MASK = (1, 1, 1, 5)
RESEEDS = (20240229, 0xD1B54A32D192ED03)          # the second one has bit 63 set
DRAWS = (1, 2, 3)
N_OPS = 3
RATES = (0.1, 0.4, 0.5, 0.9)
INDEP_MASK = (1, 32, 32, 64)          # 65 536 elements
INDEP_RATE = 0.5                      # keep probability exactly 1/2, sigma exactly 1
INDEP_RESEED = 777


def noise_grid_threads_in_source():
    m = re.search(r'inline int ew_blocks\(size_t n\) \{[^}]*cdivz\(n, (\d+)\), (\d+)\)', source('head.hip'))
    return int(m.group(1)) * int(m.group(2))


def mask_size(shape):
    return int(np.prod(shape))


def replica_streams(seed_of_op, n, rate, gaussian, ops=N_OPS, draws=DRAWS):
    """Streams of ops 0 .. ops-1 at the given draws, op-major -- the order the GPU test collects them in."""
    make = R.gaussian_mask if gaussian else R.keep_mask
    return [make(seed_of_op(i), k, n, rate) for i in range(ops) for k in draws]


def irregular_keep(shape, seed, rate):
    return (np.random.default_rng(seed).random(shape) >= rate).astype(F32)


def gaussian_noise(shape, seed, rate):
    return (1.0 + R.gaussian_sigma(rate) * np.random.default_rng(seed).standard_normal(shape)).astype(F32)


# ---------------------------------------------------------------------------------------------------------------- Dense
# B, Cin, F, nmul.  One block of 256 threads runs every loop of the backward kernel, forward has one thread per output:
#   (9, 40, 32): B*F = 288 > 256 -> second forward block, strided dz loop;   (3, 300, 1): B*Cin = 900 > 256 (strided dX loop), F = 1;
#   (2, 17, 20): Cin*F = 340 > 256 (strided dW loop);   (5, 1, 3) and (1, 7, 2): one-term sums;   (2, 6, 4, nmul 3): rows = B * nmul.
# Not reached from a SupervisedEngine graph and left to the CGAN step tests (tests/test_gpu_models.py): b0 > 0 (the fake half of the
# discriminator batch) and acc_dw (the second discriminator pass accumulating its parameter gradients).
DENSE_CASES = [(9, 40, 32, 1), (3, 300, 1, 1), (2, 17, 20, 1), (5, 1, 3, 1), (1, 7, 2, 1), (2, 6, 4, 3)]
# acc_dx: one tensor feeds two Dense heads whose outputs are concatenated.  B, Cin, (F, act) of the two heads
DENSE_SHARED_CASES = [(4, 10, (6, 'relu'), (3, None)), (3, 7, (5, 'sigmoid'), (8, 'tanh'))]


def _clear_of_kink(z):
    return bool(np.abs(z).min() >= KINK_MARGIN)


def dense_inputs(rows, cin, f, tag=0):
    """x (rows, Cin), w (Cin, F), b (F,) float32 from the first seed >= 1 at which no fp64 pre-activation lies within 1e-4 of 0
    (so the ReLU mask of the device is the reference's; the same inputs serve every activation) -> (x, w, b, seed)."""
    for seed in range(1, 1000):
        r = np.random.default_rng(1000 * (tag + 1) + seed)
        x = r.standard_normal((rows, cin)).astype(F32)
        w = (1.5 * r.standard_normal((cin, f)) / np.sqrt(cin)).astype(F32)
        b = (0.5 * r.standard_normal(f)).astype(F32)
        if _clear_of_kink(x.astype(F64) @ w.astype(F64) + b.astype(F64)):
            return x, w, b, seed
    raise AssertionError((rows, cin, f))


def dense_case_inputs(case):
    b, cin, f, nmul = case
    return dense_inputs(b * nmul, cin, f, tag=DENSE_CASES.index(case))


def dense_shared_inputs(case):
    """x and the two heads' (w, b): no pre-activation of either head within 1e-4 of 0."""
    b, cin, (f1, _), (f2, _) = case
    tag = 100 + DENSE_SHARED_CASES.index(case)
    for seed in range(1, 1000):
        r = np.random.default_rng(1000 * tag + seed)
        x = r.standard_normal((b, cin)).astype(F32)
        heads = [((1.5 * r.standard_normal((cin, f)) / np.sqrt(cin)).astype(F32), (0.5 * r.standard_normal(f)).astype(F32))
                 for f in (f1, f2)]
        if all(_clear_of_kink(x.astype(F64) @ w.astype(F64) + bb.astype(F64)) for w, bb in heads):
            return x, heads, seed
    raise AssertionError(case)


# ---------------------------------------------------------------------------------------------------------------- GAP
GAP_CHUNKS = 128
GAP_CHUNKED_MIN_HW = 4096
# N, T, H, W, C, over_time
GAP_FWD_CASES = [
    (2, 1, 64, 64, 20, False), (2, 1, 64, 64, 7, False), (2, 1, 64, 64, 260, False),       # HW = 4096: first size on the chunked path
    (2, 1, 63, 65, 20, False), (2, 1, 63, 65, 7, False), (2, 1, 63, 65, 260, False),       # HW = 4095: last on the per-(n, c) path
    (2, 1, 64, 64, 1028, False),                                                           # CP = 257 > 256: falls back
    (2, 3, 48, 40, 8, True), (2, 1, 3, 2, 5, False), (2, 3, 3, 2, 5, False),
]


def gap_path(hw, c):
    """gap_forward's dispatch for a 16-byte-aligned tensor with a workspace -> ('per_nc', None) or ('partial4' | 'partial1', (CP, rows per
    pass R, idle threads 256 - R * CP))."""
    v4 = c % 4 == 0
    cp = c // 4 if v4 else c
    if cp > 256 or hw < GAP_CHUNKED_MIN_HW:
        return 'per_nc', None
    r = 256 // cp
    return ('partial4' if v4 else 'partial1'), (cp, r, 256 - r * cp)


def gap_dispatch_in_source():
    src = source('head.hip')
    chunks = int(re.search(r'constexpr int GAP_CHUNKS = (\d+);', src).group(1))
    m = re.search(r'ws_bytes < gap_workspace_bytes\(N, C\) \|\| CP > (\d+) \|\| HW < (\d+)\)', src)
    return chunks, int(m.group(1)), int(m.group(2))


def gap_fwd_input(case):
    """N(0, 1) plus a per-channel offset in 10 .. 100: every mean is O(offset), a pixel dropped or counted twice moves it by
    offset / HW >= 1.2e-4 relative for HW <= 8192."""
    n, t, h, w, c, _ = case
    r = np.random.default_rng(GAP_FWD_CASES.index(case) + 1)
    return (r.standard_normal((n, t, h, w, c)) + r.uniform(10.0, 100.0, c)).astype(F32)


# N, T, H, W, Cin, C, relu, over_time, twice (feat is pooled by two ops whose outputs are concatenated: the first pooling's backward
# finds feat's gradient written and accumulates)
GAP_BWD_CASES = [
    (2, 1, 9, 7, 3, 8, True, False, False), (2, 1, 33, 31, 3, 20, True, False, False),     # gap_bwd4_kernel with a mask
    (2, 1, 9, 7, 3, 5, True, False, False), (2, 1, 9, 7, 3, 6, True, False, False),        # gap_bwd_masked_kernel
    (2, 1, 9, 7, 3, 8, False, False, False), (2, 1, 9, 7, 3, 5, False, False, False),      # gap_bwd4_kernel without, gap_bwd_kernel
    (2, 3, 5, 4, 3, 8, True, True, False), (2, 3, 5, 4, 3, 6, True, True, False),          # over_time, masked, float4 and scalar
    (2, 1, 9, 7, 3, 8, True, False, True), (2, 1, 9, 7, 3, 5, True, False, True),          # accumulate, masked
    (2, 1, 9, 7, 3, 8, False, False, True), (2, 1, 9, 7, 3, 5, False, False, True),        # accumulate, unmasked
]


def gap_bwd_kernel_of(c, relu):
    """gap_backward's dispatch for 16-byte-aligned buffers."""
    if c % 4 == 0:
        return 'gap_bwd4_kernel'
    return 'gap_bwd_masked_kernel' if relu else 'gap_bwd_kernel'


def gap_bwd_inputs(case):
    """x (N, T, H, W, Cin), w (Cin, C), b (C,) float32 from the first seed >= 1 at which no fp64 value of xW + b lies within 1e-4 of
    0 -> (x, w, b, seed)."""
    n, t, h, wd, cin, c = case[:6]
    tag = 200 + GAP_BWD_CASES.index(case)
    for seed in range(1, 1000):
        r = np.random.default_rng(1000 * tag + seed)
        x = r.standard_normal((n, t, h, wd, cin)).astype(F32)
        w = (0.7 * r.standard_normal((cin, c))).astype(F32)
        b = (0.5 * r.standard_normal(c)).astype(F32)
        if _clear_of_kink(R.gap_feat(x, w, b, False)[0]):
            return x, w, b, seed
    raise AssertionError(case)
