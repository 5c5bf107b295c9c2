"""Tiled prediction without a GPU: the tile plan of dl4ds_amd/tiling.py against its properties and against the
pixel-by-pixel restatement in tests/tiles_ref.py, every ValueError of the plan, the lazy public names and the C header entry.

Reach and alignment of built models are checked in tests/test_gpu_tiles.py: building a ``Model`` goes through GraphBuilder, which
creates the graph in the HIP library and so needs the device."""
import inspect

import numpy as np
import pytest

from dl4ds_amd.tiling import BLENDS, plan_axis, plan_tiles, tile_list
from tests.tiles_ref import merge_ref, plan_axis_ref

# (grid, tile, halo, align, out_scale): grid 40 / tile 16 / halo 3, grid 64 / tile 32 / halo 8 on a lattice of 4, a grid smaller than the tile; the second also with two output pixels per input pixel, and
# one whose clamped last tile overlaps TWO earlier tiles (three cores over some pixels)
CASES = [(40, 16, 3, 1, 1), (64, 32, 8, 4, 1), (64, 32, 8, 4, 2), (10, 16, 3, 1, 2), (50, 24, 4, 2, 1), (36, 16, 2, 4, 1)]


@pytest.mark.parametrize('blend', BLENDS)
@pytest.mark.parametrize('grid,tile,halo,align,s', CASES)
def test_plan_axis_properties(grid, tile, halo, align, s, blend):
    p = plan_axis(grid, tile, halo, align, blend, s)
    o, w = p.origins, p.weights
    assert w.dtype == np.float32 and w.shape == (len(o), p.tile * s)
    if grid <= tile:
        assert p.tile == grid and list(o) == [0] and np.all(w == 1)
        return
    assert p.tile == tile
    assert np.all(np.diff(o) > 0) and np.all(o % align == 0) and o[0] == 0 and o[-1] == grid - tile        # ascending, aligned, flush
    stride = (tile - 2 * halo) // align * align
    assert np.all(np.diff(o)[:-1] == stride) and 0 < o[-1] - o[-2] <= stride
    total = np.zeros(grid * s, np.float64)
    cover = np.zeros(grid * s, int)
    owners = np.zeros(grid * s, int)
    for i, oi in enumerate(o):
        sl = slice(oi * s, (oi + tile) * s)
        total[sl] += w[i].astype(np.float64)
        cover[sl] += 1
        owners[sl] += w[i] != 0
        # nothing is taken from a halo: zero weight within `halo` of every edge that is not the domain's
        if oi > 0:
            assert np.all(w[i, :halo * s] == 0)
        if oi + tile < grid:
            assert np.all(w[i, (tile - halo) * s:] == 0)
    assert np.all(cover >= 1) and np.all(owners >= 1)
    # each weight is one float32 rounding (half an ulp of a number <= 1) of a float64 partition of 1: 2 ulp per covering tile is ample
    assert np.all(np.abs(total - 1.0) <= 2 * np.finfo(np.float32).eps * cover), np.abs(total - 1).max()
    if blend == 'crop':
        assert np.all((w == 0) | (w == 1)) and np.all(owners == 1)
    else:
        assert np.all(w[:, :] >= 0) and np.all(total[cover == 1] == 1.0)       # flat 1 where a single tile covers the pixel
    ro, rw, rt = plan_axis_ref(grid, tile, halo, align, blend, s)
    assert list(ro) == list(o) and rt == p.tile
    assert np.array_equal(w, rw.astype(np.float32)) or np.abs(w - rw).max() <= np.finfo(np.float32).eps


def test_plan_tiles_two_axes_and_tile_order():
    py, px = plan_tiles((40, 64), (16, 32), 3, 1, 'linear', 2)
    assert list(py.origins) == list(plan_axis(40, 16, 3, 1, 'linear', 2).origins)
    assert np.array_equal(px.weights, plan_axis(64, 32, 3, 1, 'linear', 2).weights)
    iy, ix = tile_list((py, px))
    ny, nx = len(py.origins), len(px.origins)
    assert list(zip(iy, ix)) == [(a, b) for a in range(ny) for b in range(nx)]           # row-major: the merge order
    one = plan_tiles(20, 32, 3)                                                           # an int serves both axes
    assert one[0].tile == one[1].tile == 20


def test_plan_value_errors_name_the_remedy():
    with pytest.raises(ValueError, match=r'not a multiple of .*tile_align 4.*use 16 or 20'):
        plan_axis(64, 18, 2, 4)
    with pytest.raises(ValueError, match=r'no core.*at least 20'):
        plan_axis(64, 16, 8, 4)
    with pytest.raises(ValueError, match=r'at least 17'):
        plan_axis(64, 16, 8, 1)
    with pytest.raises(ValueError, match=r'last tile starts at .*46.*crop the domain to 60 or pad it to 64.*16, 20'):
        plan_axis(62, 16, 2, 4)
    with pytest.raises(ValueError, match=r"unknown blend 'cosine'.*crop"):
        plan_axis(64, 16, 2, 1, 'cosine')
    with pytest.raises(ValueError, match='unknown blend'):
        plan_tiles((8, 8), 16, 2, 1, 'cosine')                      # (also when no axis is tiled)
    with pytest.raises(ValueError, match='integer or a pair'):
        plan_tiles((64, 64, 64), 16, 2)


def test_merge_restatement_is_a_weighted_sum():
    """tests/tiles_ref.py against itself: the float32 form of the merge stays within one rounding per tap of the float64 form, zero
    weights drop non-finite values, and 0/1 weights copy the tile."""
    rng = np.random.default_rng(0)
    py = plan_axis(20, 12, 2, 1, 'hann')
    iy, ix = tile_list((py, py))
    oy, ox = py.origins[iy], py.origins[ix]
    tiles = rng.standard_normal((len(iy), 12, 12, 2)).astype(np.float32)
    smp = np.zeros(len(iy), int)
    a = merge_ref(np.zeros((1, 20, 20, 2), np.float32), tiles, oy, ox, smp, iy, ix, py.weights, py.weights)
    b = merge_ref(np.zeros((1, 20, 20, 2), np.float64), tiles, oy, ox, smp, iy, ix, py.weights, py.weights, exact=True)
    assert np.abs(a - b).max() <= 8 * 2.0 ** -24 * np.abs(tiles).max()
    pc = plan_axis(20, 12, 2, 1, 'crop')
    bad = tiles.copy()
    for t in range(len(iy)):                                        # poison what 'crop' discards
        wyx = pc.weights[iy[t]][:, None] * pc.weights[ix[t]][None, :]
        bad[t][wyx == 0] = [np.nan, np.inf]
    c = merge_ref(np.zeros((1, 20, 20, 2), np.float32), bad, oy, ox, smp, iy, ix, pc.weights, pc.weights)
    assert np.all(np.isfinite(c))
    for t in range(len(iy)):
        wyx = pc.weights[iy[t]][:, None] * pc.weights[ix[t]][None, :]
        assert np.array_equal(c[0, oy[t]:oy[t] + 12, ox[t]:ox[t] + 12][wyx == 1], tiles[t][wyx == 1])


def test_lazy_names_and_signatures():
    import dl4ds_amd
    from dl4ds_amd import inference
    assert dl4ds_amd.predict_tiled is inference.predict_tiled
    assert dl4ds_amd.TiledPredictor is inference.TiledPredictor
    assert dl4ds_amd.plan_tiles is plan_tiles
    ref = list(inspect.signature(inference.predict).parameters.items())
    got = list(inspect.signature(inference.predict_tiled).parameters.items())
    assert [k for k, _ in got[:6]] == ['trainer', 'array', 'scale', 'tile', 'halo', 'blend']
    assert got[4][1].default is None and got[5][1].default == 'crop'
    # the remaining arguments are predict's, in its order (batch_size counts tiles and defaults to Model.predict_tiled's 32)
    assert [k for k, _ in got[6:]] == [k for k, _ in ref[3:]]
    for (k, a), (_, b) in zip(got[6:], ref[3:]):
        assert a.default == b.default or k == 'batch_size', k
    ctor = list(inspect.signature(inference.TiledPredictor.__init__).parameters)
    assert ctor[1:7] == ['trainer', 'array', 'scale', 'tile', 'halo', 'blend']
    assert ctor[7:] == list(inspect.signature(inference.Predictor.__init__).parameters)[4:]
    m = inspect.signature(dl4ds_amd.graph.Model.predict_tiled)
    assert list(m.parameters) == ['self', 'inputs', 'tile', 'halo', 'blend', 'batch_size']
    assert m.parameters['batch_size'].default == 32


def test_header_declares_the_merge_entry():
    from dl4ds_amd import _lib
    protos = _lib.parse_header()
    assert 'dl4ds_tile_merge' in protos
    assert len(protos['dl4ds_tile_merge'][1]) == 18
    text = open(_lib.HEADER_PATH).read()
    assert 'inference.py:238' in text[text.index('tiled prediction'):text.index('int dl4ds_tile_merge')]
