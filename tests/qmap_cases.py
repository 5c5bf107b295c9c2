"""Seeded inputs of the quantile-mapping tests, shared by tests/test_gpu_qmap.py (device against tests/qmap_ref.py) and
tests/test_qmap_api.py (the restatement against independent answers).  Imports nothing from the product.  Magnitudes stay in the
normal float32 range, about 1e-3 ... 1e4 (and exact zeros), so that denormal handling is not what is being compared."""
import numpy as np

from tests.distribution_cases import STRIDED_MAX, TILE, WS_BUDGET, precip, strided_group

# constants of csrc/qmap.hip the shapes below are built around
MAX_Q = 256                   # QM_MAX_Q
GATHER_TILE = 64              # QM_TR: cells per workgroup of the global engine's gather and finish kernels
MAP_CELLS = 64                # QM_CELLS: cells per workgroup of the map
LDS_BUDGET = 80 << 10         # QM_LDS_BUDGET: all tables of a workgroup are staged while Q * MAP_CELLS * 4 * tables fits

TABLE_LENGTHS = (1, 2, 3, 64, 511, 512, 513, TILE + 5)


def table_group(n):
    """cells a workgroup of the one-sided strided engine takes at n samples (tab_group): twice distribution.hip's"""
    return 2 * strided_group(n)


def table_cells(n):
    """the numbers of cells a table case of n samples runs at: one, a partial wave, 105, and one cell more than a workgroup's
    group (distribution.hip's and this engine's own; beyond STRIDED_MAX the gather tile)"""
    if n <= STRIDED_MAX:
        return (1, 6, 105, strided_group(n) + 1, table_group(n) + 1)
    return (1, 6, 105, GATHER_TILE + 1)


def global_bytes_per_cell(n):
    """workspace of one cell of the global engine (qmap.hip's Workspace): two key buffers and the digit counts per tile"""
    al = lambda b: (b + 255) & ~255
    return 2 * al(n * 4) + al(max(1, -(-n // TILE)) * 1024)


def max_staged_q(tables):
    """the largest Q at which the map stages `tables` tables in LDS"""
    return LDS_BUDGET // (MAP_CELLS * 4 * tables)


def temperature(rng, shape, shift=0.0, scale=8.0):
    return (280.0 + shift + scale * rng.standard_normal(shape)).astype(np.float32)


def field(n, cells, seed):
    """(n, cells) temperatures (even seed) or precipitation with about 60 % zeros (odd seed)"""
    r = np.random.default_rng(seed)
    return precip(r, (n, cells)) + np.float32(0.0) if seed % 2 else temperature(r, (n, cells))


def zeros70(n=40, cells=35):
    x = precip(np.random.default_rng(70), (n, cells), zeros=0.7)
    assert 0.6 < (x == 0).mean() < 0.8
    return x


def signed_zeros(n=50, cells=20):
    r = np.random.default_rng(5)
    x = r.standard_normal((n, cells)).astype(np.float32)
    x[r.random(x.shape) < 0.3] = 0.0
    x[r.random(x.shape) < 0.3] = -0.0
    assert np.signbit(x[x == 0]).any() and not np.signbit(x[x == 0]).all()
    return x


def spoiled(n=60, cells=84, seed=44):
    """NaN and both infinities sprinkled in, one cell all NaN (cell 3), one with a single valid value (cell 5)"""
    r = np.random.default_rng(seed)
    x = temperature(r, (n, cells))
    for v in (np.nan, np.inf, -np.inf, -np.nan):
        x[r.random(x.shape) < 0.03] = v
    x[:, 3] = np.nan
    x[:, 5] = np.inf
    x[n // 3, 5] = 1.25
    return x


def workspace_chunks():
    """STRIDED_MAX + 1 samples of 128 x 190 cells through the global engine: more cells than one workspace chunk holds"""
    n, cells = STRIDED_MAX + 1, 128 * 190
    assert cells * global_bytes_per_cell(n) > WS_BUDGET
    return temperature(np.random.default_rng(130), (n, cells))


def probabilities(Q):
    """Q probabilities from 0.01 to 0.99: values below the first and above the last knot exist in every sample"""
    return np.linspace(0.01, 0.99, Q)


def history(kind, cells, seed, n_obs=61, n_model=47):
    """(obs, model, future) of `cells` cells for a map case.  Additive: temperatures, the model 3 K warm and too variable, the
    future 2 K warmer still.  Multiplicative: precipitation with about 70 % zeros, rounded to 0.1 (tied knots, knots equal to 0)."""
    r = np.random.default_rng(seed)
    if kind == 0:
        return (temperature(r, (n_obs, cells)), temperature(r, (n_model, cells), 3.0, 10.0), temperature(r, (n_model + 5, cells), 5.0, 10.0))
    out = tuple(np.round(f * precip(r, (n, cells), zeros=0.7), 1).astype(np.float32) + np.float32(0.0)
                for f, n in ((1.0, n_obs), (1.4, n_model), (1.6, n_model + 5)))
    for a in out:
        a[:, 3::4] += np.float32(0.5)                                   # every fourth cell is never dry: values below its first knot exist
    if cells > 8:
        out[1][:, 4] = 0                                                # the model never rains in cell 4: m_t == 0 at the ends too
    return out


def spoil_cells(obs, model):
    """an all-NaN cell on either side (when there are cells to spare): unfitted cells 1 (observation) and 2 (model)"""
    if obs.shape[1] > 4:
        obs[:, 1] = np.nan
        model[:, 2] = np.nan


def map_input(kind, B, search, seed):
    """(B, cells) values to map through the search table `search` (Q, cells): drawn wider than the table (both ends are left),
    then, as far as B allows, rows that sit exactly on the first knot, on the last knot and on an inner knot, and a sprinkling of
    non-finite values and (multiplicative) zeros"""
    r = np.random.default_rng(seed)
    Q, cells = search.shape
    x = temperature(r, (B, cells), 3.0, 14.0) if kind == 0 else np.round(2.0 * precip(r, (B, cells), zeros=0.5), 1).astype(np.float32)
    x = x + np.float32(0.0)
    fitted = np.where(np.isnan(search), np.float32(1.0), search)
    for row, knot in zip(range(1, B), (0, Q - 1, Q // 2, Q // 3)):
        x[row] = fitted[knot]
    if B * cells > 8:
        for v in (np.nan, np.inf, -np.inf):
            x[r.random(x.shape) < 0.02] = v
    return x
