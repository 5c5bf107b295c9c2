"""Numpy restatement of tiled prediction, written independently of dl4ds_amd/tiling.py and csrc/tiles.hip:
the tile plan of one axis pixel by pixel, the merge tap by tap, and a tile-by-tile driver for any forward function (the fp64 oracle)."""
import math

import numpy as np


def plan_axis_ref(grid, tile, halo, align=1, blend='crop', out_scale=1):
    """-> (origins, weights float64 [n][tile * out_scale], tile).  Pixel by pixel: every tile's core is the tile minus ``halo`` at
    each edge that is not the domain's; a pixel's raw weight in tile i is 0 outside the core, and inside it the product of a ramp
    rising over the overlap of core i with core i - 1 and one falling over the overlap with core i + 1 (crop: a step at the middle
    pixel boundary of that overlap); the raw weights are divided by their sum over the tiles."""
    if grid <= tile:
        return [0], np.ones((1, grid * out_scale)), grid
    stride = (tile - 2 * halo) // align * align
    origins = []
    o = 0
    while o < grid - tile:
        origins.append(o)
        o += stride
    origins.append(grid - tile)
    s, n = out_scale, len(origins)
    lo = [o * s + (halo * s if o > 0 else 0) for o in origins]
    hi = [(o + tile) * s - (halo * s if o + tile < grid else 0) for o in origins]

    def ramp(c, a, b):
        if blend == 'crop' or b <= a:
            return 1.0 if c > (a + b) // 2 else 0.0
        t = min(max((c - a) / (b - a), 0.0), 1.0)
        return t if blend == 'linear' else math.sin(0.5 * math.pi * t) ** 2
    raw = np.zeros((n, grid * s))
    for p in range(grid * s):
        c = p + 0.5
        for i in range(n):
            if not lo[i] < c < hi[i]:
                continue
            w = 1.0
            if i > 0:
                w *= ramp(c, lo[i], hi[i - 1])
            if i + 1 < n:
                w *= 1.0 - ramp(c, lo[i + 1], hi[i])
            raw[i, p] = w
    raw /= raw.sum(axis=0)
    return origins, np.stack([raw[i, origins[i] * s:(origins[i] + tile) * s] for i in range(n)]), tile


def merge_ref(out, tiles, oy, ox, smp, ry, rx, wy, wx, exact=False):
    """out[smp[t], oy[t] + y, ox[t] + x, :] += wy[ry[t], y] * wx[rx[t], x] * tiles[t, y, x, :] for t ascending, zero weights skipped.
    ``exact=False``: the kernel's float32 arithmetic -- w = fl32(wy * wx), acc = fl32(w * v + acc) with the product exact (a float64
    holds the 48-bit product of two float32; the sum is then rounded twice, which differs from a fused multiply-add only in rare
    ties: bit-exact for 0/1 weights, where it is the only use that is asserted bit for bit).  ``exact=True``: everything in float64."""
    tiles = np.asarray(tiles)
    th, tw = tiles.shape[1:3]
    for t in range(tiles.shape[0]):
        for y in range(th):
            a = wy[ry[t], y]
            if a == 0:
                continue
            for x in range(tw):
                b = wx[rx[t], x]
                if b == 0:
                    continue
                v = tiles[t, y, x].astype(np.float64)
                acc = out[smp[t], oy[t] + y, ox[t] + x]
                if exact:
                    out[smp[t], oy[t] + y, ox[t] + x] = acc + float(a) * float(b) * v
                else:
                    w = np.float32(np.float32(a) * np.float32(b))
                    out[smp[t], oy[t] + y, ox[t] + x] = (np.float64(w) * v + acc.astype(np.float64)).astype(np.float32)
    return out


def stitch(forward, inputs, ratios, plan_y, plan_x, out_scale):
    """Tile-by-tile evaluation of ``forward(list of input tiles) -> output tile`` merged in float64.  ``inputs``: (N, H, W, C) arrays,
    input k on a grid ``ratios[k]`` times the first one's; plan_*: (origins, weights, tile) of either axis."""
    (oys, wys, th), (oxs, wxs, tw) = plan_y, plan_x
    n = inputs[0].shape[0]
    out = None
    for iy, oy in enumerate(oys):
        for ix, ox in enumerate(oxs):
            parts = [a[:, oy * r:(oy + th) * r, ox * r:(ox + tw) * r] for a, r in zip(inputs, ratios)]
            t = np.asarray(forward(parts), np.float64)
            if out is None:
                out = np.zeros((n, inputs[0].shape[1] * out_scale, inputs[0].shape[2] * out_scale, t.shape[-1]))
            w = np.asarray(wys[iy], np.float64)[:, None] * np.asarray(wxs[ix], np.float64)[None, :]
            keep = w != 0                                         # a zero weight drops the tap, whatever the value
            region = out[:, oy * out_scale:(oy + th) * out_scale, ox * out_scale:(ox + tw) * out_scale]
            region[:, keep] += w[keep][None, :, None] * t[:, keep]
    return out
