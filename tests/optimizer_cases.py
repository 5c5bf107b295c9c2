"""Seeded cases shared by tests/test_optimizer_api.py (no GPU) and tests/test_gpu_optimizer.py: sizes, decayed ranges, inputs and
the feature combinations of the extended optimiser step (csrc/adam_ext.hip).  Not a test module; needs no GPU."""
import itertools
import re

import numpy as np

from tests import step_kernels_cases as S

F32, F64 = np.float32, np.float64

# the norm launch: blocks = min(cdiv(n / 4 + 1, NORM_THREADS), NORM_BLOCK_CAP), 4 elements per thread and pass
NORM_THREADS, NORM_BLOCK_CAP = 256, 1024
# just above cap x per-block work: every one of the 1024 partials is written, 3 blocks take a second grid-stride pass, tail of 3
NORM_LARGEST = 4 * NORM_THREADS * NORM_BLOCK_CAP + 4 * NORM_THREADS * 3 + 3
SIZES = (1, 2, 3, 4, 5, 1023, 1025, 2051, NORM_LARGEST)
SCALES = (1.0, 1.0 / 3.0)
STEPS = (1, 7)
WEIGHT_DECAY, EMA_MOMENTUM = 0.004, 0.99


def norm_figures_in_source():
    """-> (threads, block cap) of sqnorm_blocks in csrc/adam_ext.hip, and the threads of the norm kernel's launch bound."""
    src = S._src('adam_ext.hip')
    m = re.search(r'int sqnorm_blocks\(size_t n\) \{ return \(int\)std::max<size_t>\(1, std::min<size_t>\(cdivz\(n / 4 \+ 1, (\d+)\), (\d+)\)\); \}', src)
    t = re.search(r'constexpr int SQNORM_THREADS = (\d+);', src)
    c = re.search(r'constexpr int SQNORM_BLOCK_CAP = (\d+);', src)
    assert int(t.group(1)) == int(m.group(1)) and int(c.group(1)) == int(m.group(2))
    return int(m.group(1)), int(m.group(2))


def norm_blocks(n):
    return max(1, min(S.cdiv(n // 4 + 1, NORM_THREADS), NORM_BLOCK_CAP))


def decay_range_sets(n):
    """None, the whole arena, [(1, 2)] and, from n = 1023 on, [(0, 5), (7, 1022)] and a range that ends at n: starts and ends off
    the multiples of four, inside one float4 and in the scalar tail."""
    sets = [[], [(0, n)]]
    if n >= 2:
        sets.append([(1, 2)])
    if n >= 1023:
        sets.append([(0, 5), (7, 1022)])
        sets.append([(n - 6, n)])
    return sets


def inputs(n, seed=0):
    """(w, g, m, v, ema): unit-scale weights and gradients, moments as a few steps in, v > 0; every 7th entry from 3 idle
    (g = m = v = 0: the moments stay 0 and only decay and the average move it)."""
    rng = np.random.default_rng(1000 + seed)
    w, g = rng.standard_normal(n).astype(F32), rng.standard_normal(n).astype(F32)
    m = (F32(0.1) * rng.standard_normal(n)).astype(F32)
    v = (F32(0.1) * np.abs(rng.standard_normal(n)) + F32(1e-6)).astype(F32)
    ema = (w + F32(0.05) * rng.standard_normal(n)).astype(F32)
    idle = np.arange(n) % 7 == 3
    g[idle] = m[idle] = v[idle] = 0
    if not g.any():
        g[0] = F32(0.75)                       # n = 1 .. 3 never reach entry 3; keep a gradient for the norm
    return w, g, m, v, ema


# (clip, decay, ema) on / off: all eight
FEATURES = tuple(itertools.product((False, True), repeat=3))
