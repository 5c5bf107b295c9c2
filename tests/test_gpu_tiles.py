"""Tiled prediction on the MI355X: the merge kernel op by op against tests/tiles_ref.py, reach and alignment of
built models (here because building a ``Model`` creates its graph in the HIP library), and ``predict_tiled`` end to end.

CHANNEL ATTENTION.  Every builder of ``dl4ds_amd.models`` ends in ``ConvBlock_att``, a ConvBlock with ChannelAttention2D
(sp_postups.py:204, sp_preups.py:175,301), whose scale is a function of the mean over the whole field, also with ``attention=False``.
``predict_tiled`` computes that mean in a first pass over the tiles, so the end-to-end cases run with ``halo=None`` against the fp64
oracle on the full grid.  (With per-tile means instead, the oracle run tile by tile on the CPU is 1.48e-3 away for resnet/spc scale 2
and 6.0e-3 for net_pin at halo 7 resp. 8, tile 24 on a 40 x 40 domain: above the 1e-3 criterion.)

THE IMPULSE TESTS.  Through the tail attention a changed input pixel moves the field's channel means and with them every output
pixel; ``receptive_halo`` counts the dependence other than through those means.  ``test_reach_with_the_attention_means_pinned`` tests
exactly that, with the means held fixed.  The unpinned test on the resnet/spc model holds because, for the weights ``build_pair``
seeds, the one ReLU unit of the attention's bottleneck (int(4 / 4) = 1) is inactive with and without the impulse; the test asserts
that too, so a change of the seeding shows up as that assertion and not as a wrong reach."""
import ctypes

import numpy as np
import pytest

from oracle import models as M
from oracle import np_ops as N
from tests.tiles_ref import merge_ref, plan_axis_ref, stitch

pytestmark = pytest.mark.gpu


def rel(a, ref):
    ref = np.asarray(ref, np.float64)
    return np.abs(np.asarray(a, np.float64) - ref).max() / max(np.abs(ref).max(), 1e-12)


# ------------------------------------------------------------------------------------------------------------ merge kernel, op level
def _merge_case(C, blend, seed=0):
    """Output 2 x 20 x 28 x C; 12 x 12 tiles on a 3 x 3 origin grid (rows 0, 4, 8: halo 4; columns 0, 8, 16: halo 2) per sample, plus one
    tile at the odd origin (3, 5) of sample 1 with a table row of its own (for C = 1 and 3 its batch takes the 4-byte path)."""
    from dl4ds_amd.tiling import plan_axis, tile_list
    py, px = plan_axis(20, 12, 4, 1, blend), plan_axis(28, 12, 2, 1, blend)
    assert list(py.origins) == [0, 4, 8] and list(px.origins) == [0, 8, 16]
    iy, ix = tile_list((py, px))
    extra = np.zeros(12, np.float32)
    extra[3:9] = 1.0 if blend == 'crop' else 0.375
    wy, wx = np.vstack([py.weights, extra]), np.vstack([px.weights, extra])
    oy = np.concatenate([py.origins[iy], py.origins[iy], [3]])
    ox = np.concatenate([px.origins[ix], px.origins[ix], [5]])
    smp = np.concatenate([np.zeros(9, int), np.ones(9, int), [1]])
    ry, rx = np.concatenate([iy, iy, [3]]), np.concatenate([ix, ix, [3]])
    rng = np.random.default_rng(seed + C)
    tiles = rng.standard_normal((19, 12, 12, C)).astype(np.float32)
    return tiles, oy, ox, smp, ry, rx, wy, wx


def _gpu_merge(tiles, oy, ox, smp, ry, rx, wy, wx, splits, shape=(2, 20, 28)):
    from dl4ds_amd import _lib
    from dl4ds_amd.device import DeviceArray
    lib = _lib.lib()
    C = tiles.shape[-1]
    d_out = DeviceArray.zeros(shape + (C,))
    d_wy, d_wx = DeviceArray.from_numpy(wy), DeviceArray.from_numpy(wx)
    i32 = lambda a: np.ascontiguousarray(a, np.int32)
    start = 0
    for n in splits:
        d_t = DeviceArray.from_numpy(tiles[start:start + n])
        lists = [i32(v[start:start + n]) for v in (oy, ox, smp, ry, rx)]
        _lib.check(lib.dl4ds_tile_merge(d_t.ptr, n, tiles.shape[1], tiles.shape[2], C, *[v.ctypes.data for v in lists], d_wy.ptr,
                                        wy.shape[0], d_wx.ptr, wx.shape[0], d_out.ptr, *shape))
        _lib.check(lib.dl4ds_sync())
        start += n
    assert start == len(tiles)
    return d_out.numpy()


@pytest.mark.parametrize('C', [1, 3, 4])
def test_merge_crop_is_bit_equal_and_drops_poisoned_halos(C):
    for n in (19, 18):            # all tiles: the odd origin puts C = 1 and 3 on the 4-byte path; without it every C takes 16 bytes
        tiles, oy, ox, smp, ry, rx, wy, wx = [v[:n] if i < 6 else v for i, v in enumerate(_merge_case(C, 'crop'))]
        want = merge_ref(np.zeros((2, 20, 28, C), np.float32), tiles, oy, ox, smp, ry, rx, wy, wx)
        got = _gpu_merge(tiles, oy, ox, smp, ry, rx, wy, wx, [n])
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), n
        bad = tiles.copy()
        for t in range(len(bad)):                                  # NaN and inf wherever the weight is exactly 0
            w = wy[ry[t]][:, None] * wx[rx[t]][None, :]
            bad[t][w == 0] = np.resize([np.nan, np.inf, -np.inf], C)
        assert not np.all(np.isfinite(bad))
        got = _gpu_merge(bad, oy, ox, smp, ry, rx, wy, wx, [n])
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), n


@pytest.mark.parametrize('blend', ['linear', 'hann'])
@pytest.mark.parametrize('C', [1, 3, 4])
def test_merge_blends_within_the_rounding_bound(C, blend):
    """Against the float64 restatement on the same float32 tables.  For a pixel with K taps of non-zero weight the kernel rounds, per
    tap, the product w = wy * wx (relative 2^-24, so at most 2^-24 |w v| in the sum) and the fmaf (2^-24 of the partial sum, which is
    at most S = sum |w v|): |error| <= K 2^-24 S + 2^-24 S <= (K + 1) 2^-24 S up to second order, for which one more unit is
    granted: (K + 2) 2^-24 S.  Here K <= 3 * 3 + 1."""
    for n in (19, 18):            # (18: without the odd-origin tile, so that C = 1 and 3 take the 16-byte path too)
        tiles, oy, ox, smp, ry, rx, wy, wx = [v[:n] if i < 6 else v for i, v in enumerate(_merge_case(C, blend))]
        want = merge_ref(np.zeros((2, 20, 28, C), np.float64), tiles, oy, ox, smp, ry, rx, wy, wx, exact=True)
        ones = np.ones_like(tiles)
        S = merge_ref(np.zeros((2, 20, 28, C), np.float64), np.abs(tiles), oy, ox, smp, ry, rx, wy, wx, exact=True)
        K = merge_ref(np.zeros((2, 20, 28, C), np.float64), ones, oy, ox, smp, ry, rx, (wy != 0).astype(np.float32),
                      (wx != 0).astype(np.float32), exact=True)
        assert 1 <= K.min() and K.max() <= 10
        got = _gpu_merge(tiles, oy, ox, smp, ry, rx, wy, wx, [n])
        err = np.abs(got.astype(np.float64) - want)
        print('merge', blend, C, n, 'max err / bound', (err / ((K + 2) * 2.0 ** -24 * S)).max())
        assert np.all(err <= (K + 2) * 2.0 ** -24 * S)


@pytest.mark.parametrize('blend', ['crop', 'hann'])
@pytest.mark.parametrize('C', [1, 3, 4])
def test_merge_is_bitwise_independent_of_the_batch_split(C, blend):
    case = _merge_case(C, blend)
    whole = _gpu_merge(*case, [19])
    for splits in ([1] * 19, [2] * 9 + [1], [7, 12]):
        assert np.array_equal(_gpu_merge(*case, splits).view(np.uint32), whole.view(np.uint32)), splits


@pytest.mark.parametrize('C', [1, 3, 8])
def test_pool_sums_every_pixel_once_in_a_fixed_order(C):
    """dl4ds_tile_pool with the 0/1 weights of a crop plan against numpy in float64: products by 1 are exact, the fp64 sums of up to
    560 float32 values per sample differ by rounding only (2^-52 per addition of at most S = sum |v|: 560 * 2^-52 * S is granted); the
    same bits for every split into calls; refusals."""
    from dl4ds_amd import _lib
    from dl4ds_amd.device import DeviceArray
    lib = _lib.lib()
    tiles, oy, ox, smp, ry, rx, wy, wx = _merge_case(C, 'crop')
    tiles, oy, ox, smp, ry, rx, wy, wx = tiles[:18], oy[:18], ox[:18], smp[:18], ry[:18], rx[:18], wy[:3], wx[:3]
    field = merge_ref(np.zeros((2, 20, 28, C), np.float64), tiles, oy, ox, smp, ry, rx, wy, wx, exact=True)
    want, S = field.sum(axis=(1, 2)), np.abs(field).sum(axis=(1, 2))
    d_wy, d_wx = DeviceArray.from_numpy(wy), DeviceArray.from_numpy(wx)
    i32 = lambda a: np.ascontiguousarray(a, np.int32)

    def run(splits, **kw):
        d_s = DeviceArray.zeros((2, C), np.float64)
        start = 0
        for n in splits:
            d_t = DeviceArray.from_numpy(tiles[start:start + n])
            lists = [i32(v[start:start + n]) for v in (smp, ry, rx)]
            a = dict(tiles=d_t.ptr, n=n, th=12, tw=12, C=C, wy=d_wy.ptr, wy_rows=3, wx=d_wx.ptr, wx_rows=3, sums=d_s.ptr, N=2)
            a.update(kw)
            st = lib.dl4ds_tile_pool(a['tiles'], a['n'], a['th'], a['tw'], a['C'], *[v.ctypes.data for v in lists], a['wy'],
                                     a['wy_rows'], a['wx'], a['wx_rows'], a['sums'], a['N'])
            if st != 0:
                return None
            start += n
        return d_s.numpy()
    got = run([18])
    assert np.all(np.abs(got - want) <= 560 * 2.0 ** -52 * S)
    for splits in ([1] * 18, [5, 13]):
        assert np.array_equal(run(splits).view(np.uint64), got.view(np.uint64)), splits
    for kw in (dict(tiles=None), dict(sums=None), dict(wy=None), dict(n=0), dict(C=0), dict(N=1), dict(wy_rows=2), dict(wx_rows=2)):
        assert run([18], **kw) is None and b'tile_pool' in lib.dl4ds_last_error(), kw


def test_merge_refusals():
    from dl4ds_amd import _lib
    from dl4ds_amd.device import DeviceArray
    lib = _lib.lib()
    tiles, oy, ox, smp, ry, rx, wy, wx = _merge_case(1, 'crop')
    d_t, d_wy, d_wx, d_out = (DeviceArray.from_numpy(a) for a in (tiles, wy, wx, np.zeros((2, 20, 28, 1), np.float32)))
    i32 = lambda a: np.ascontiguousarray(a, np.int32)
    good = dict(tiles=d_t.ptr, n=19, th=12, tw=12, C=1, oy=i32(oy), ox=i32(ox), smp=i32(smp), ry=i32(ry), rx=i32(rx), wy=d_wy.ptr,
                wy_rows=4, wx=d_wx.ptr, wx_rows=4, out=d_out.ptr, N=2, H=20, W=28)

    def call(**kw):
        a = dict(good, **kw)
        p = lambda v: v.ctypes.data if isinstance(v, np.ndarray) else v
        return lib.dl4ds_tile_merge(a['tiles'], a['n'], a['th'], a['tw'], a['C'], p(a['oy']), p(a['ox']), p(a['smp']), p(a['ry']),
                                    p(a['rx']), a['wy'], a['wy_rows'], a['wx'], a['wx_rows'], a['out'], a['N'], a['H'], a['W'])

    def moved(v, i, x):
        v = v.copy()
        v[i] = x
        return v
    refused = [dict(n=257), dict(tiles=None), dict(wy=None), dict(wx=None), dict(out=None), dict(oy=None), dict(ox=None), dict(smp=None),
               dict(ry=None), dict(rx=None), dict(n=0), dict(th=0), dict(tw=0), dict(C=0), dict(N=0), dict(wy_rows=0),
               dict(H=11), dict(W=11),                                                  # tile larger than the output
               dict(oy=moved(good['oy'], 5, 9)), dict(ox=moved(good['ox'], 5, 17)),     # one pixel past the edge
               dict(oy=moved(good['oy'], 0, -1)), dict(ox=moved(good['ox'], 0, -1)),
               dict(smp=moved(good['smp'], 3, 2)), dict(smp=moved(good['smp'], 3, -1)),
               dict(ry=moved(good['ry'], 18, 4)), dict(rx=moved(good['rx'], 18, 4)), dict(ry=moved(good['ry'], 0, -1)),
               dict(wy_rows=3), dict(wx_rows=3)]                                        # table shorter than a row index
    for kw in refused:
        assert call(**kw) != 0, kw
        assert b'tile_merge' in lib.dl4ds_last_error(), kw
    _lib.check(lib.dl4ds_sync())
    assert not d_out.numpy().any()                              # nothing was launched
    # the sticky device error word: raised by the library's diagnostic kernel, seen once the stream has drained
    ms = ctypes.c_float()
    _lib.check(lib.dl4ds_event_timer_start())
    _lib.check(lib.dl4ds_debug_raise_device_error(4))
    _lib.check(lib.dl4ds_event_timer_stop(ctypes.byref(ms)))    # (waits for the kernel without looking at the word)
    assert call() != 0 and b'device error word' in lib.dl4ds_last_error()
    assert lib.dl4ds_sync() != 0                                # reported and cleared by the next wait, as for every entry
    _lib.check(lib.dl4ds_sync())
    assert not d_out.numpy().any()
    assert call() == 0
    _lib.check(lib.dl4ds_sync())
    assert d_out.numpy().any()


# ------------------------------------------------------------------------------------------------ graphs without a global op
def _bias(model, seed=12):
    rng = np.random.default_rng(seed)
    w = model.get_weights()
    for k in w:
        if k.endswith('bias'):
            w[k] = (rng.standard_normal(w[k].shape) * 0.05).astype(np.float32)
    model.set_weights(w)
    return {k: v.astype(np.float64) for k, v in w.items()}


def plain_spc(lr_size, seed=3):
    """conv3 - conv3 - conv3 + depth_to_space(2) - concat(conv3 of an HR input) - conv3 - conv3: reach 1 + 1 + 1 + (1 + 1) / 2 = 4 LR
    pixels (the HR branch reaches 1/2 + 1 = 3/2)."""
    from dl4ds_amd.graph import GraphBuilder, Model, resizable

    @resizable('lr_size')
    def build(lr_size, seed=None):
        h, w = lr_size
        g = GraphBuilder()
        x, s = g.input(h, w, 2), g.input(2 * h, 2 * w, 1)
        y = g.conv2d(x, 'c1', 4, 3, activation='relu')
        y = g.conv2d(y, 'c2', 4, 3, activation='relu')
        y = g.conv2d(y, 'up', 16, 3, d2s=2)
        a = g.conv2d(s, 'aux', 4, 3, activation='relu')
        y = g.conv2d(g.concat([y, a]), 'c3', 4, 3, activation='relu')
        g.finalize(g.conv2d(y, 'out', 1, 3), seed)
        return Model(g, 'plain_spc', [(h, w, 2), (2 * h, 2 * w, 1)])
    return build(lr_size=tuple(lr_size), seed=seed)


def plain_spc_ref(P, x, s):
    c = lambda t, k, act=True: (N.relu if act else (lambda v: v))(N.conv2d(t, P[k + '/kernel'], P[k + '/bias']))
    y = N.depth_to_space(c(c(c(x, 'c1'), 'c2'), 'up', False), 2)
    y = np.concatenate([y, c(s, 'aux')], axis=-1)
    return c(c(y, 'c3'), 'out', False)


def mini_unet(hr_size, seed=4):
    """conv3 - maxpool - conv3 - bilinear x2 - conv3 - concat(skip) - conv3 - conv3.  Reach: 1; pool: pixels 2 wide, + 1 for the
    footprint -> 2; conv at width 2: + 2 -> 4; bilinear: + 1 * 2 -> 6; three convs at width 1 -> 9.  tile_align 2."""
    from dl4ds_amd.graph import GraphBuilder, Model, resizable

    @resizable('hr_size')
    def build(hr_size, seed=None):
        h, w = hr_size
        g = GraphBuilder()
        x = g.input(h, w, 2)
        e = g.conv2d(x, 'e1', 4, 3, activation='relu')
        b = g.conv2d(g.maxpool2(e), 'b', 8, 3, activation='relu')
        u = g.conv2d(g.resize(b, h, w, 'u', 'bilinear'), 'uc', 4, 3)
        y = g.conv2d(g.concat([u, e]), 'd', 4, 3, activation='relu')
        g.finalize(g.conv2d(y, 'out', 1, 3), seed)
        return Model(g, 'mini_unet', [(h, w, 2)])
    return build(hr_size=tuple(hr_size), seed=seed)


def mini_unet_ref(P, x, s=None):
    c = lambda t, k, act=True: (N.relu if act else (lambda v: v))(N.conv2d(t, P[k + '/kernel'], P[k + '/bias']))
    e = c(x, 'e1')
    b = c(N.max_pool2(e), 'b')
    u = c(N.resize_bilinear(b, x.shape[1], x.shape[2]), 'uc', False)
    return c(c(np.concatenate([u, e], axis=-1), 'd'), 'out', False)


# ------------------------------------------------------------------------------------------------------------ reach and alignment
def _built(kind, **cfg):
    import dl4ds_amd.models as PM
    if kind == 'post':
        return PM.net_postupsampling(n_channels=1, n_aux_channels=cfg.pop('aux', 0), lr_size=cfg.pop('size', (16, 16)), scale=2,
                                     n_filters=4, n_blocks=1, seed=1, **cfg)
    if kind == 'pin':
        return PM.net_pin(n_channels=1, n_aux_channels=0, hr_size=(16, 16), n_filters=4, n_blocks=1, seed=1, **cfg)
    return PM.unet_pin('unet', n_channels=1, n_aux_channels=0, n_filters=4, hr_size=(32, 32), seed=1, **cfg)


def test_reach_and_alignment_of_built_models():
    """Hand-derived, in pixels of the first input.  B = stem + ResidualBlock (2 convs) + backbone_last = 4 for n_blocks = 1 (3 x 3
    convolutions add 1, 1 x 1 add 0); T = ConvBlock_att + ConvBlock_out = 4 convolutions 3 x 3 on the output grid.
      resnet/spc x2     B + conv2x (1) + T / 2                                   = 4 + 1 + 2          = 7
      resnet/rc bilinear  B + 1 (two taps) + (conv + T) / 2                      = 4 + 1 + 0.5 + 2    = 7.5 -> 8
      resnet/rc bicubic   B + 2 (tap radius) + 0.5 + 2                                                = 8.5 -> 9
      resnet/dc x2      B + 2 (9 x 9, stride 2: inputs m - 2 .. m + 2 feed output 2 m + 1) + T / 2   = 8
      net_pin           B + T                                                                         = 8
      unet_pin, L levels of conv-conv-pool, bottleneck, L x (bilinear x2, conv, conv-conv), T, at pixel widths 1, 2, .., 2^L; a pool
      to width 2 p adds the footprint p:
        L = 2: 2, +1, +4, +2 (width 4), bottleneck +8 = 17; up: +4, +2, +4 = 27; +2, +1, +2 = 32; T: +4                     = 36
        L = 3: 2, +1, +4, +2, +8, +4 (width 8), +16 = 37; up: +8, +4, +8 = 57; +4, +2, +4 = 67; +2, +1, +2 = 72; T: +4      = 76
      tile_align = 2^L (the builder pools once per level: models/sp_preups.py unet_pin, `for i in range(n_blocks)`), 1 without pooling.
    The one ChannelAttention2D of every builder's tail costs no halo (module docstring): ``receptive_halo`` equals ``local_halo``.  With
    ``attention=True`` the backbone holds more of them and ``receptive_halo`` is None."""
    want = [(_built('post', upsampling='spc', backbone_block='resnet'), 7, 1),
            (_built('post', upsampling='spc', backbone_block='resnet', aux=1), 7, 1),
            (_built('post', upsampling='rc', backbone_block='resnet'), 8, 1),
            (_built('post', upsampling='rc', backbone_block='resnet', rc_interpolation='bicubic'), 9, 1),
            (_built('post', upsampling='dc', backbone_block='resnet'), 8, 1),
            (_built('pin', backbone_block='resnet'), 8, 1),
            (_built('unet', n_blocks=2), 36, 4),
            (_built('unet', n_blocks=3), 76, 8),
            (_built('post', upsampling='spc', backbone_block='resnet', attention=True), 7, 1),
            (_built('post', upsampling='spc', backbone_block='resnet', attention=True, aux=1), 7, 1)]
    for model, halo, align in want:
        assert (model.local_halo, model.tile_align) == (halo, align), (model.name, model.local_halo, model.tile_align)
        many = len(model.graph.outputs[0].stats) > 1
        assert model.receptive_halo == (None if many else halo) and many == bool(model._rebuild[1]['attention'])
        assert isinstance(model.local_halo, int) and isinstance(model.tile_align, int)
    m = plain_spc((12, 12))
    assert (m.receptive_halo, m.local_halo, m.tile_align) == (4, 4, 1)
    m = mini_unet((16, 16))
    assert (m.receptive_halo, m.local_halo, m.tile_align) == (9, 9, 2)
    # the reach does not depend on the grid the graph is planned for
    assert _built('post', upsampling='spc', backbone_block='resnet', size=(24, 40)).local_halo == 7


def _attention_hidden(model):
    """The bottleneck activations relu(mean W1 + b1) of the model's (one) ChannelAttention2D in its last forward pass, from the tensor
    the op pooled (read back from the graph) and the model's weights."""
    from dl4ds_amd import _lib
    from dl4ds_amd.device import DeviceArray
    lib = _lib.lib()
    tid, c, plain = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
    _lib.check(lib.dl4ds_graph_chatt_info(model.graph.h, 0, ctypes.byref(tid), ctypes.byref(c), ctypes.byref(plain)))
    assert plain.value and lib.dl4ds_graph_chatt_info(model.graph.h, 1, ctypes.byref(tid), ctypes.byref(c), ctypes.byref(plain)) != 0
    p = ctypes.c_void_p()
    _lib.check(lib.dl4ds_graph_tensor_ptr(model.graph.h, tid.value, 0, ctypes.byref(p)))
    ho, wo = model.output_shape[:2]
    y = np.empty((ho, wo, c.value), np.float32)
    _lib.check(lib.dl4ds_memcpy_d2h(y.ctypes.data, p, y.nbytes))
    w = model.get_weights()
    k = [n for n in w if n.endswith('/att/conv1/kernel')]
    assert len(k) == 1
    pre = y.astype(np.float64).mean(axis=(0, 1)) @ w[k[0]][0, 0].astype(np.float64) + w[k[0].replace('kernel', 'bias')]
    return np.maximum(pre, 0.0), pre


def _impulse_extent(model, shapes, scale, after=None):
    rng = np.random.default_rng(3)
    ins = [rng.standard_normal(s).astype(np.float32) for s in shapes]
    base = model(ins)
    if after:
        after()
    cy, cx = shapes[0][1] // 2, shapes[0][2] // 2
    ins[0] = ins[0].copy()
    ins[0][0, cy, cx, :] += 4.0
    moved = np.argwhere(np.any(model(ins) != base, axis=-1)[0])
    if after:
        after()
    # distance, in output pixels, to the block of scale x scale output pixels of the input pixel that was changed
    dy = np.maximum(np.maximum(cy * scale - moved[:, 0], moved[:, 0] - (cy * scale + scale - 1)), 0)
    dx = np.maximum(np.maximum(cx * scale - moved[:, 1], moved[:, 1] - (cx * scale + scale - 1)), 0)
    return int(np.maximum(dy, dx).max())


def test_reach_is_an_upper_bound_and_tight_resnet_spc():
    """resnet/spc, scale 2, n_filters 4, one block, weights randomised as ``build_pair`` does, LR 32 x 32, impulse at the centre: no
    output pixel farther than receptive_halo * scale from the changed pixel's block moves, one at that distance does.  The full model
    has this property only while the tail attention does not respond to the impulse (module docstring); that it does not, for these
    weights, is asserted: the one unit of its bottleneck is inactive before and after the impulse.  The next test pins the means."""
    from tests.test_gpu_models import build_pair
    model, _, _ = build_pair('net_postupsampling', dict(backbone_block='resnet', upsampling='spc', scale=2, n_filters=4, n_blocks=1),
                             (1, 32, 32, 1), None)
    halo = model.receptive_halo
    assert halo == 7
    seen = []
    assert _impulse_extent(model, [(1, 32, 32, 1)], 2, after=lambda: seen.append(_attention_hidden(model))) == halo * 2
    print('attention bottleneck pre-activations', [pre for _, pre in seen])
    assert len(seen) == 2 and all(h.shape == (1,) and h[0] == 0.0 for h, _ in seen)


@pytest.mark.parametrize('seed', [11, 12, 13])
def test_reach_with_the_attention_means_pinned(seed):
    """What ``receptive_halo`` claims for a model with one channel attention: with the attention's channel means held fixed
    (dl4ds_graph_chatt_set_mean, as predict_tiled's second pass runs), an impulse moves output pixels up to exactly receptive_halo *
    scale away and none beyond, whatever the weights (three seeds)."""
    from dl4ds_amd import _lib
    from dl4ds_amd.device import DeviceArray
    from tests.test_gpu_models import build_pair
    model, _, _ = build_pair('net_postupsampling', dict(backbone_block='resnet', upsampling='spc', scale=2, n_filters=4, n_blocks=1),
                             (1, 32, 32, 1), None, seed=seed)
    mean = DeviceArray.from_numpy(np.array([[0.3, -0.2, 0.9, 0.1]], np.float32))
    lib = _lib.lib()
    _lib.check(lib.dl4ds_graph_chatt_set_mean(model.graph.h, 0, mean.ptr))
    try:
        assert _impulse_extent(model, [(1, 32, 32, 1)], 2) == model.receptive_halo * 2
    finally:
        lib.dl4ds_graph_chatt_set_mean(model.graph.h, 0, None)
    assert lib.dl4ds_graph_chatt_set_mean(model.graph.h, 1, None) != 0 and lib.dl4ds_graph_chatt_set_mean(None, 0, None) != 0


@pytest.mark.parametrize('make,shapes,scale', [(plain_spc, [(1, 32, 32, 2), (1, 64, 64, 1)], 2), (mini_unet, [(1, 32, 32, 2)], 1)])
def test_reach_is_an_upper_bound_and_tight_without_global_ops(make, shapes, scale):
    """An impulse at the centre moves no output pixel farther than receptive_halo * scale from the changed pixel's own block of output
    pixels, and moves one at exactly that distance (plain_spc).  For mini_unet the bound 9 is one more than what any single pixel
    shows (8, worked out by hand: e1 15..17 -> cells 7, 8 -> b 6..9 -> bilinear 11..20 -> three convolutions 8..23 around pixel 16): the
    footprint of the pooled pixel and the far tap of the bilinear resize are counted separately although they overlap by one pixel."""
    model = make(shapes[0][1:3])
    _bias(model)
    extent, bound = _impulse_extent(model, shapes, scale), model.receptive_halo * scale
    assert extent == (bound if make is plain_spc else bound - 1)


# ------------------------------------------------------------------------------------------------------------ end to end
E2E = [('net_postupsampling', dict(backbone_block='resnet', upsampling='spc', scale=2, n_filters=4, n_blocks=1), (1, 40, 40, 1),
        (1, 80, 80, 1), 24, True),
       ('net_postupsampling', dict(backbone_block='resnet', upsampling='rc', scale=2, n_filters=4, n_blocks=1,
                                   rc_interpolation='bicubic'), (1, 36, 36, 1), None, 26, False),
       ('net_postupsampling', dict(backbone_block='resnet', upsampling='dc', scale=2, n_filters=4, n_blocks=1), (1, 40, 40, 1), None,
        26, False),
       ('net_pin', dict(backbone_block='resnet', n_filters=4, n_blocks=1), (1, 40, 40, 2), None, 26, True),
       ('unet_pin', dict(n_filters=4, n_blocks=2, decoder_upsampling='rc'), (1, 92, 92, 1), None, 80, False)]
E2E_RUNS = [(c, 'crop') for c in range(5)] + [(c, 'hann') for c in range(5) if E2E[c][5]]


@pytest.mark.parametrize('case,blend', E2E_RUNS)
def test_end_to_end_against_the_full_grid_oracle(case, blend):
    """``halo=None`` (= receptive_halo), fp64 oracle on the FULL grid, inputs from ``tie_free_inputs``, the project's forward criterion
    max |out - ref| / max |ref| < 1e-3; domains with a first, an interior and a clamped last tile on each axis."""
    from tests.test_gpu_models import build_pair, tie_free_inputs
    kind, cfg, xs, ss, tile, _ = E2E[case]
    model, P, ocfg = build_pair(kind, cfg, xs, ss)
    o = plan_axis_ref(xs[1], tile, model.receptive_halo, model.tile_align, blend, cfg.get('scale', 1))[0]
    assert len(o) == 3 and o[2] - o[1] < o[1]                                     # first, interior, clamped
    _, x, s, ref = tie_free_inputs(kind, P, ocfg, xs, ss)
    out = model.predict_tiled([x] if s is None else [x, s], tile, halo=None, blend=blend)
    print(kind, cfg.get('upsampling'), blend, 'rel', rel(out, ref))
    assert out.shape == ref.shape and rel(out, ref) < 1e-3


@pytest.mark.parametrize('case,blend', [(0, 'crop'), (0, 'hann')])
def test_builder_models_against_the_oracle_run_tile_by_tile(case, blend):
    """The approximate path: with ``attention=True`` the backbone holds channel attentions too, ``receptive_halo`` is None and an explicit
    halo gives per-tile statistics.  That is what the fp64 oracle evaluated tile by tile and merged by tests/tiles_ref.py with the same
    plan computes: same crops at every input's grid ratio, same merge, the project's forward criterion."""
    from tests.test_gpu_models import build_pair
    kind, cfg, xs, ss, tile, _ = E2E[case]
    model, P, ocfg = build_pair(kind, dict(cfg, attention=True), xs, ss)
    assert model.receptive_halo is None
    rng = np.random.default_rng(7)
    ins = [rng.standard_normal(s).astype(np.float32) for s in (xs, ss) if s is not None]
    halo, scale = model.local_halo, cfg.get('scale', 1)
    plan = plan_axis_ref(xs[1], tile, halo, model.tile_align, blend, scale)
    assert len(plan[0]) == 3 and plan[0][-1] - plan[0][-2] < plan[0][1]           # first, interior, clamped
    fwd = lambda parts: M.MODELS[kind](N, P, parts[0].astype(np.float64), parts[1].astype(np.float64) if len(parts) > 1 else None,
                                       **ocfg)
    ref = stitch(fwd, ins, [1, scale][:len(ins)], plan, plan, scale)
    out = model.predict_tiled(ins, tile, halo=halo, blend=blend, batch_size=4)
    print(kind, cfg.get('upsampling'), blend, 'rel', rel(out, ref))
    assert out.shape == ref.shape and rel(out, ref) < 1e-3


@pytest.mark.parametrize('make,ref_fn,shapes,tile,scale', [(plain_spc, plain_spc_ref, [(2, 28, 36, 2), (2, 56, 72, 1)], (16, 20), 2),
                                                           (mini_unet, mini_unet_ref, [(2, 36, 48, 2)], (24, 32), 1)])
def test_tiled_equals_full_grid_without_global_ops(make, ref_fn, shapes, tile, scale):
    """Graphs with a bounded reach: ``halo=None`` (= receptive_halo), fp64 numpy reference on the FULL grid, max |out - ref| / max |ref| <
    1e-3, for crop and hann; and the test has power: stitched with halo=0 the same comparison misses the criterion."""
    model = make(tile)
    P = _bias(model)
    rng = np.random.default_rng(9)
    ins = [rng.standard_normal(s).astype(np.float32) for s in shapes]
    ref = ref_fn(P, *[a.astype(np.float64) for a in ins])
    for blend in ('crop', 'hann'):
        out = model.predict_tiled(ins, tile, blend=blend, batch_size=5)
        print(model.name, blend, 'rel', rel(out, ref))
        assert out.shape == ref.shape and rel(out, ref) < 1e-3
    full = model.predict(ins)
    assert rel(full, ref) < 1e-3
    assert rel(model.predict_tiled(ins, tile, halo=0), ref) > 1e-3


def test_halo_zero_misses_the_criterion_on_a_builder_model():
    """Power of the 1e-3 criterion on the first end-to-end case (resnet/spc scale 2 with an HR static input): stitched with ``halo=0`` the prediction is 6.3e-2 away from the full-grid
    oracle (seed and sizes checked with the oracle run tile by tile on the CPU: 6.25e-2 there, against 1.48e-3 with halo 7)."""
    from tests.test_gpu_models import build_pair, tie_free_inputs
    kind, cfg, xs, ss, tile, _ = E2E[0]
    model, P, ocfg = build_pair(kind, cfg, xs, ss)
    _, x, s, ref = tie_free_inputs(kind, P, ocfg, xs, ss)
    assert rel(model.predict_tiled([x, s], tile, halo=0), ref) > 1e-3


def test_batch_size_does_not_change_a_bit_and_one_tile_is_predict():
    from tests.test_gpu_models import build_pair
    kind, cfg, xs, ss, tile, _ = E2E[0]
    xs, ss = (3,) + xs[1:], (3,) + ss[1:]
    model, _, _ = build_pair(kind, cfg, xs, ss)
    rng = np.random.default_rng(2)
    ins = [rng.standard_normal(s).astype(np.float32) for s in (xs, ss)]
    for blend in ('crop', 'linear'):
        outs = [model.predict_tiled(ins, tile, halo=model.local_halo, blend=blend, batch_size=b) for b in (1, 3, 32)]
        assert np.array_equal(outs[0].view(np.uint32), outs[1].view(np.uint32))
        assert np.array_equal(outs[0].view(np.uint32), outs[2].view(np.uint32))
    # 3 x 13 x 13 = 507 tiles of 16 pixels in one batch: the merge entry takes 256 per call and the batch is split, to the same bits
    many = [model.predict_tiled(ins, 16, halo=model.local_halo, blend='linear', batch_size=b) for b in (32, 1000)]
    assert np.array_equal(many[0].view(np.uint32), many[1].view(np.uint32))
    # a tile at least as large as the domain: one tile per sample, the model's own graph, predict's bits
    full = model.predict(ins, batch_size=3)
    for t in (40, 64, (40, 100)):
        assert np.array_equal(model.predict_tiled(ins, t, halo=5, batch_size=3).view(np.uint32), full.view(np.uint32)), t
    other = model.predict([a[:, :30 * r, :34 * r] for a, r in zip(ins, (1, 2))], batch_size=3)        # on a re-planned sibling too
    got = model.predict_tiled([a[:, :30 * r, :34 * r] for a, r in zip(ins, (1, 2))], 48, halo=5, batch_size=3)
    assert np.array_equal(got.view(np.uint32), other.view(np.uint32))


@pytest.mark.parametrize('array_in_hr', [True, False])
def test_public_entries_from_host_arrays(array_in_hr, tmp_path):
    import dl4ds_amd
    from dl4ds_amd.inference import _prepare_inputs
    from tests.test_gpu_models import build_pair
    kind, cfg, xs, ss, tile, _ = E2E[0]
    # (for a spatial model the batch builder appends the coarsened static variable to the LR input: two LR channels)
    model, _, _ = build_pair(kind, cfg, (2, 40, 40, 2), (2, 80, 80, 1))
    rng = np.random.default_rng(4)
    hr = (rng.standard_normal((2, 80, 80, 1)) * 3 + 280).astype(np.float32)
    static = rng.standard_normal((80, 80, 1)).astype(np.float32)
    scaler = dl4ds_amd.StandardScaler(axis=None)
    scaler.fit(hr)
    array = np.asarray(scaler.transform(hr.copy()), np.float32).reshape(hr.shape)
    if not array_in_hr:
        array = array[:, ::2, ::2]
    kw = dict(array_in_hr=array_in_hr, static_vars=[static])
    _, inputs = _prepare_inputs(model, array, 2, array_in_hr, [static], None, None, 'inter_area')
    want = np.asarray(scaler.inverse_transform(model.predict_tiled(inputs, tile, halo=model.local_halo, blend='hann')), np.float32)
    got, lr = dl4ds_amd.predict_tiled(model, array, 2, tile, halo=model.local_halo, blend='hann', scaler=scaler, return_lr=True,
                                      save_path=str(tmp_path), **kw)
    assert np.array_equal(got, want) and np.array_equal(lr, inputs[0]) and got.size == 2 * 80 * 80
    assert np.array_equal(np.load(tmp_path / 'y_hat.npy'), want)
    run = dl4ds_amd.TiledPredictor(model, array, 2, tile, halo=model.local_halo, blend='hann', scaler=scaler, **kw).run()
    assert np.array_equal(run, want)


def test_predict_tiled_value_errors():
    import dl4ds_amd.models as PM
    import dl4ds_amd
    rng = np.random.default_rng(0)
    x = rng.standard_normal((1, 40, 40, 1)).astype(np.float32)
    model = _built('post', upsampling='spc', backbone_block='resnet')
    with pytest.raises(ValueError, match='depends on the whole field.*`halo` must be given.*local_halo = 7'):
        _built('post', upsampling='spc', backbone_block='resnet', attention=True).predict_tiled(x, 24)
    with pytest.raises(ValueError, match='unknown blend'):
        model.predict_tiled(x, 24, halo=7, blend='cosine')
    with pytest.raises(ValueError, match='no core'):
        model.predict_tiled(x, 14, halo=7)
    lc = _built('post', upsampling='spc', backbone_block='resnet', localcon_layer=True)
    with pytest.raises(ValueError, match='localcon_layer=True.*out of scope'):
        lc.predict_tiled(x, 24, halo=7)
    rec = PM.recnet_postupsampling('resnet', 'spc', 2, 1, 0, (8, 8), time_window=2, n_filters=4, n_blocks=1)
    with pytest.raises(ValueError, match='spatio-temporal.*out of scope'):
        rec.predict_tiled(rng.standard_normal((1, 2, 8, 8, 1)).astype(np.float32), 4, halo=1)
    with pytest.raises(ValueError, match='out of scope'):
        dl4ds_amd.predict_tiled(rec, np.zeros((3, 16, 16, 1), np.float32), 2, 4, halo=1, time_window=2)
    unet = _built('unet', n_blocks=2)
    u = rng.standard_normal((1, 96, 96, 1)).astype(np.float32)
    with pytest.raises(ValueError, match='not a multiple of .*tile_align 4'):
        unet.predict_tiled(u, 82, halo=36)
    with pytest.raises(ValueError, match='not a multiple of tile_align 4'):
        unet.predict_tiled(u[:, :94, :94], 80, halo=36)           # the clamped last origin 14 is off the lattice
    with pytest.raises(ValueError, match='integer multiple'):
        _built('post', upsampling='spc', backbone_block='resnet', aux=1).predict_tiled([x, np.zeros((1, 60, 60, 1), np.float32)], 24, halo=7)
