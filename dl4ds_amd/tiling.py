"""Tile plans for ``Model.predict_tiled``: where the tiles of a large grid lie and with which weights their
outputs are merged.  Pure numpy; importable without the HIP library.

A plan is made per axis.  ``grid``, ``tile``, ``halo`` and ``align`` are in pixels of the model's first input; the weights are per
OUTPUT pixel (``out_scale`` output pixels per input pixel: ``scale`` for a post-upsampling model, 1 for a 'pin' model).

* Origins: 0, s, 2 s, ... with s = ``tile - 2 halo`` rounded down to a multiple of ``align``, the last one clamped to ``grid - tile``
  (flush with the end of the domain).  A grid that is not larger than the tile gets one tile of the grid's own size.
* The CORE of a tile is what is left of it ``halo`` pixels inside every edge that is not flush with the domain: there the tile's output
  equals the full grid's when ``halo`` is at least the model's reach.  Consecutive cores overlap or abut, because s <= tile - 2 halo.
* Weights are zero outside the core, so nothing from a halo is ever merged.  'crop': 1 up to the seam in the middle of the overlap with
  either neighbour, 0 beyond it; exactly one tile owns each pixel.  'linear' / 'hann': a ramp a (resp. sin^2(pi a / 2)) across the
  overlap of the two CORES, 1 where a single core covers the pixel.  All of them are built in float64, divided by their sum over the
  tiles at each pixel, and rounded once to float32.
"""
from collections import namedtuple

import numpy as np

BLENDS = ('crop', 'linear', 'hann')

AxisPlan = namedtuple('AxisPlan', 'origins weights tile')
AxisPlan.__doc__ = """origins: int64 [n_tiles], input pixels; weights: float32 [n_tiles][tile * out_scale]; tile: the tile's size on this
axis in input pixels (the grid's size where the grid is not larger than the requested tile)."""


def _pair(v, name):
    if np.ndim(v) == 0:
        v = (v, v)
    v = tuple(v)
    if len(v) != 2 or any(int(a) != a for a in v):
        raise ValueError(f'`{name}` must be an integer or a pair of integers, got {v!r}')
    return int(v[0]), int(v[1])


def plan_axis(grid, tile, halo, align=1, blend='crop', out_scale=1):
    """One axis of ``plan_tiles`` -> AxisPlan."""
    grid, tile, halo, align, out_scale = int(grid), int(tile), int(halo), int(align), int(out_scale)
    if blend not in BLENDS:
        raise ValueError(f'unknown blend {blend!r}: use one of {BLENDS}')
    if grid < 1 or tile < 1 or halo < 0 or align < 1 or out_scale < 1:
        raise ValueError(f'plan_tiles: grid {grid}, tile {tile}, align {align} and out_scale {out_scale} must be >= 1 and halo {halo} >= 0')
    if grid <= tile:
        return AxisPlan(np.zeros(1, np.int64), np.ones((1, grid * out_scale), np.float32), grid)
    if tile % align:
        lo = tile // align * align
        raise ValueError(f'tile size {tile} is not a multiple of the model\'s tile_align {align} (tiles must pool the same pixels as '
                         f'the full grid): use {lo if lo > 2 * halo else lo + align} or {lo + align}')
    if tile <= 2 * halo:
        need = (2 * halo // align + 1) * align
        raise ValueError(f'tile size {tile} leaves no core inside a halo of {halo} on either side: use a tile of at least {need} '
                         f'(or a smaller halo)')
    if (grid - tile) % align:
        # tile is a multiple of align, so this is the grid's own remainder: no tile size moves the last origin onto the lattice
        lo = grid // align * align
        raise ValueError(f'the last tile starts at grid - tile = {grid - tile}, which is not a multiple of tile_align {align}, and no '
                         f'tile size that is a multiple of {align} changes that on a grid of {grid}: crop the domain to {lo} or pad it '
                         f'to {lo + align} pixels (nearest tile sizes that then fit: {tile}, {tile + align})')
    stride = (tile - 2 * halo) // align * align
    if stride < 1:
        need = (2 * halo // align + 1) * align
        raise ValueError(f'tile size {tile} minus two halos of {halo} is less than tile_align {align}: use a tile of at least {need}')
    origins = np.array(list(range(0, grid - tile, stride)) + [grid - tile], np.int64)
    n, s = len(origins), out_scale
    # cores in output pixels
    lo = origins * s + np.where(origins > 0, halo * s, 0)
    hi = (origins + tile) * s - np.where(origins + tile < grid, halo * s, 0)
    c = np.arange(grid * s, dtype=np.float64) + 0.5                     # pixel centres
    win = np.zeros((n, grid * s), np.float64)
    for i in range(n):
        w = ((c > lo[i]) & (c < hi[i])).astype(np.float64)
        if i > 0:
            w *= _ramp(c, lo[i], hi[i - 1], blend)                      # rises across the overlap with the previous core
        if i + 1 < n:
            w *= 1.0 - _ramp(c, lo[i + 1], hi[i], blend)                # falls across the overlap with the next one
        win[i] = w
    total = win.sum(axis=0)
    if not np.all(total > 0):                                           # (cannot happen: consecutive cores overlap or abut)
        raise AssertionError('plan_tiles: a pixel without a covering core')
    win /= total
    weights = np.zeros((n, tile * s), np.float32)
    for i in range(n):
        weights[i] = win[i, origins[i] * s:(origins[i] + tile) * s]
    return AxisPlan(origins, weights, tile)


def _ramp(c, a, b, blend):
    """0 -> 1 across [a, b) at the pixel centres ``c``; 'crop': the step at the middle pixel boundary."""
    if blend == 'crop' or b <= a:
        return (c > (a + b) // 2).astype(np.float64)
    t = np.clip((c - a) / float(b - a), 0.0, 1.0)
    return t if blend == 'linear' else np.sin(0.5 * np.pi * t) ** 2


def plan_tiles(grid, tile, halo, align=1, blend='crop', out_scale=1):
    """-> (AxisPlan of the rows, AxisPlan of the columns).  ``grid`` and ``tile``: an int or a (rows, columns) pair.  Raises ValueError
    (with the remedy in the message) for a tile that is not a multiple of ``align``, a tile of at most ``2 halo``, a clamped last origin
    off the ``align`` lattice, and an unknown ``blend``."""
    grid, tile = _pair(grid, 'grid'), _pair(tile, 'tile')
    return tuple(plan_axis(g, t, halo, align, blend, out_scale) for g, t in zip(grid, tile))


def tile_list(plan):
    """The tiles of a two-axis plan in merge order (row-major): int arrays (iy, ix) of each tile's index on either axis."""
    ny, nx = len(plan[0].origins), len(plan[1].origins)
    iy, ix = np.divmod(np.arange(ny * nx), nx)
    return iy.astype(np.int64), ix.astype(np.int64)
