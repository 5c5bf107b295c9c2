"""conv_pointwise_kernel (csrc/conv_pointwise.hip): the 1x1 layers with float4-able channel counts up to 48, forward and dgrad calls
alike (a dgrad is the same call with the transposed filter), through dl4ds_amd.ops.conv2d_views.

Every case is compared

* with an fp64 numpy restatement at the bar of the conv family tests (tests/test_gpu_ops.py ``close``, tests/test_gpu_conv_views.py
  ``TOL``: 2e-4 of the largest reference magnitude);
* with the same call under DL4DS_NO_POINTWISE=1, i.e. on the kernel that took the layer before.  Where that kernel sums in the same
  order the bits must be equal: conv_stream<1,..> and conv_stream_ws<1,..> always (k-slot q of step e carries channel (Cin / 4) q + e
  as here; the first adds the bias to the finished sum, the second starts its accumulators at it, and the new kernel does what the
  one that would have run does), conv_igemm with fewer than 16 input channels (k-slot q carries channel 4 e + q, which the new kernel
  keeps for those layers).  conv_igemm on 16 and more input channels (grids under 256 pixels per image) orders its sums differently:
  there the two results may differ by at most twice the old kernel's own distance from fp64 on the same inputs, measured here
  (both are roundings of the same exact value, so their distance is bounded by the sum of their errors);
* outside the output view (the other channels of a wider buffer, the slack behind every buffer) nothing may change.

Routing is asserted by launch tag; the pooling epilogue, which no entry point can hand to a 1x1 layer, is covered on the host side by
tests/test_conv_route_pointwise.py.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
TOL = 2e-4      # tests/test_gpu_ops.py close(), tests/test_gpu_conv_views.py TOL

PAIRS = [(8, 16), (16, 24), (24, 32), (40, 48), (48, 8), (48, 40), (24, 16)]
GRIDS = [(2, 5, 7), (2, 33, 19), (3, 16, 16)]       # 70, 1254 and 768 pixels: no multiple of the 32- / 64-pixel block but the last
EPILOGUES = {                                        # name: (bias, add, mask, relu, accumulate)
    'bias': (1, 0, 0, 0, 0), 'bias_relu': (1, 0, 0, 1, 0), 'add': (0, 1, 0, 0, 0), 'mask': (0, 0, 1, 0, 0),
    'accumulate': (0, 0, 0, 0, 1), 'add_relu': (1, 1, 0, 1, 0), 'mask_accumulate': (0, 0, 1, 0, 1),
}
VIEWS = ('plain', 'sliced')


@pytest.fixture(scope='module')
def ops():
    import dl4ds_amd.ops as o
    return o


def _data(n, h, w, ci, co):
    rng = np.random.default_rng(1000 * ci + 10 * co + h)
    f = lambda *s: rng.standard_normal(s).astype(np.float32)
    return dict(x=f(n, h, w, ci), w=f(1, 1, ci, co) * 0.2, b=f(co), add=f(n, h, w, co), mask=f(n, h, w, co), old=f(n, h, w, co))


def _reference(d, epi):
    bias, add, mask, relu, acc = EPILOGUES[epi]
    y = np.einsum('nhwc,cd->nhwd', d['x'].astype(np.float64), d['w'][0, 0].astype(np.float64))
    if bias:
        y = y + d['b'].astype(np.float64)
    if add:
        y = y + d['add'].astype(np.float64)
    if relu:
        y = np.maximum(y, 0)
    if mask:
        y = np.where(d['mask'] > 0, y, 0)
    if acc:
        y = y + d['old'].astype(np.float64)
    return y


def _embed(a, view, seed, pad, off):
    """-> (buffer, kwargs of ops.View): ``a`` itself, or channels [off, off + C) of a buffer with ``pad`` more channels"""
    if view == 'plain':
        return a.copy(), {}
    rng = np.random.default_rng(seed)
    buf = rng.standard_normal(a.shape[:-1] + (a.shape[-1] + pad,)).astype(np.float32)
    buf[..., off:off + a.shape[-1]] = a
    return buf, dict(C=a.shape[-1], coff=off)


def _run(ops, d, epi, view):
    """-> (the output view's contents, launch tags, names of buffers changed outside the output view)"""
    from tests.parity import kernel_tags
    from dl4ds_amd.ops import slack_values
    bias, add, mask, relu, acc = EPILOGUES[epi]
    xb, xk = _embed(d['x'], view, 1, 8, 4)           # input: a slice of a wider buffer
    yb, yk = _embed(d['old'], view, 2, 12, 8)         # output: another one
    sent = dict(x=xb, y=yb)
    views = dict(x=ops.View(xb, **xk), y=ops.View(yb, **yk))
    kw = {}
    for name, on in (('add', add), ('mask', mask)):
        if on:
            sent[name] = d[name].copy()
            kw[name] = ops.View(sent[name])
    bufs, tags = kernel_tags(lambda: ops.conv2d_views(views['x'], d['w'], views['y'], b=d['b'] if bias else None, relu=bool(relu),
                                                       accumulate=bool(acc), **kw))
    co, off = d['old'].shape[-1], yk.get('coff', 0)
    bad = []
    for name, (after, slack) in bufs.items():
        same = after.view(np.uint32) == sent[name].view(np.uint32)
        if name == 'y':
            same[..., off:off + co] = True
        if not same.all():
            bad.append(name)
        if not np.array_equal(slack.view(np.uint32), slack_values().view(np.uint32)):
            bad.append(name + '.slack')
    return np.array(bufs['y'][0][..., off:off + co]), tags, bad


def _tag(ci, co):
    return f'conv_pointwise<{ci // 4},{(co + 15) // 16}>'


def _rel(a, ref, scale):
    return float(np.abs(np.asarray(a, np.float64) - ref).max() / scale)


@pytest.mark.parametrize('n,h,w', GRIDS)
@pytest.mark.parametrize('ci,co', PAIRS)
def test_pointwise_against_fp64_and_the_kernel_it_replaces(ops, monkeypatch, ci, co, n, h, w):
    d = _data(n, h, w, ci, co)
    for view in VIEWS:
        for epi, (bias, *_rest) in EPILOGUES.items():
            what = (ci, co, (n, h, w), view, epi)
            ref = _reference(d, epi)
            scale = max(np.abs(ref).max(), 1e-6)
            monkeypatch.delenv('DL4DS_NO_POINTWISE', raising=False)
            new, tags, bad = _run(ops, d, epi, view)
            assert _tag(ci, co) in tags, (what, sorted(tags))
            assert not bad, (what, bad)
            monkeypatch.setenv('DL4DS_NO_POINTWISE', '1')
            old, old_tags, bad = _run(ops, d, epi, view)
            assert not any(t.startswith('conv_pointwise') for t in old_tags), (what, sorted(old_tags))
            assert not bad, (what, bad)
            e_new, e_old, diff = _rel(new, ref, scale), _rel(old, ref, scale), _rel(new, old.astype(np.float64), scale)
            print(f'{what}: new {e_new:.2e} old {e_old:.2e} new-old {diff:.2e} {sorted(t for t in old_tags if t.startswith("conv_"))}')
            assert e_new < TOL, (what, e_new)
            same_order = any(t.startswith(('conv_stream<1,', 'conv_stream_ws<1,')) for t in old_tags) or \
                (ci < 16 and any(t.startswith('conv_igemm<1,') for t in old_tags))
            if same_order:
                assert np.array_equal(new.view(np.uint32), old.view(np.uint32)), (what, diff, sorted(old_tags))
            else:
                assert diff <= 2 * e_old, (what, diff, e_old, sorted(old_tags))


@pytest.mark.parametrize('ci,co,epi', [(40, 48, 'bias'), (48, 40, 'mask_accumulate'), (8, 48, 'bias_relu'), (16, 24, 'add_relu')])
def test_pointwise_on_a_grid_the_producer_consumer_kernel_took(ops, monkeypatch, ci, co, epi):
    """4 x 64 x 128 pixels: enough 16 x 16 tiles for conv_stream_ws<1,..> to be the kernel that ran the 24- to 48-channel layers, as at
    the headline shape -- the bits must be the old kernel's, with a bias too; with DL4DS_POINTWISE_GRID=8 (32 waves) every wave
    walks 16 or 32 blocks, prefetching the next one, and the bits must still be the same"""
    n, h, w = 4, 64, 128
    d = _data(n, h, w, ci, co)
    ref = _reference(d, epi)
    monkeypatch.setenv('DL4DS_NO_POINTWISE', '1')
    old, old_tags, bad = _run(ops, d, epi, 'plain')
    assert not bad and not any(t.startswith('conv_pointwise') for t in old_tags), (bad, sorted(old_tags))
    assert ci < 24 or any(t.startswith('conv_stream_ws<1,') for t in old_tags), sorted(old_tags)
    monkeypatch.delenv('DL4DS_NO_POINTWISE')
    for grid in (None, '8'):
        if grid:
            monkeypatch.setenv('DL4DS_POINTWISE_GRID', grid)
        new, tags, bad = _run(ops, d, epi, 'plain')
        assert _tag(ci, co) in tags and not bad, (grid, sorted(tags), bad)
        assert _rel(new, ref, np.abs(ref).max()) < TOL
        assert np.array_equal(new.view(np.uint32), old.view(np.uint32)), (grid, _rel(new, old.astype(np.float64), np.abs(ref).max()))


def test_pointwise_dgrad_call(ops, monkeypatch):
    """the dgrad entry (transposed filter, ReLU mask of the layer's input, accumulation into the gradient) takes the kernel too"""
    from tests.parity import kernel_tags
    monkeypatch.delenv('DL4DS_NO_POINTWISE', raising=False)
    n, h, w, ci, co = 2, 33, 19, 24, 40
    rng = np.random.default_rng(5)
    dz = rng.standard_normal((n, h, w, co)).astype(np.float32)
    wt = (rng.standard_normal((1, 1, ci, co)) * 0.2).astype(np.float32)
    mask = rng.standard_normal((n, h, w, ci)).astype(np.float32)
    old = rng.standard_normal((n, h, w, ci)).astype(np.float32)
    ref = np.where(mask > 0, np.einsum('nhwd,cd->nhwc', dz.astype(np.float64), wt[0, 0].astype(np.float64)), 0) + old
    bufs, tags = kernel_tags(lambda: ops.conv2d_views(ops.View(dz), wt, ops.View(old.copy()), mask=ops.View(mask), accumulate=True,
                                                       dgrad=True))
    assert _tag(co, ci) in tags, sorted(tags)
    assert _rel(bufs['y'][0], ref, np.abs(ref).max()) < TOL


def test_what_the_pointwise_kernel_leaves_to_the_others(ops, monkeypatch):
    """a depth_to_space output, a channel count that is no multiple of four and an epilogue form that is not built keep their kernels"""
    from tests.parity import kernel_tags
    monkeypatch.delenv('DL4DS_NO_POINTWISE', raising=False)
    rng = np.random.default_rng(6)
    f = lambda *s: rng.standard_normal(s).astype(np.float32)
    n, h, w = 2, 16, 18

    def tags_of(x, wt, y, **kw):
        return sorted(kernel_tags(lambda: ops.conv2d_views(x, wt, y, **kw))[1])

    t = tags_of(ops.View(f(n, h, w, 16)), f(1, 1, 16, 32), ops.View(f(n, 2 * h, 2 * w, 8), C=32, d2s=2))
    assert t and not any(k.startswith('conv_pointwise') for k in t), t
    t = tags_of(ops.View(f(n, h, w, 26)), f(1, 1, 26, 16), ops.View(f(n, h, w, 16)))
    assert t and not any(k.startswith('conv_pointwise') for k in t), t
    t = tags_of(ops.View(f(n, h, w, 16)), f(1, 1, 16, 16), ops.View(f(n, h, w, 16)), add=ops.View(f(n, h, w, 16)),
                mask=ops.View(f(n, h, w, 16)))
    assert t and not any(k.startswith('conv_pointwise') for k in t), t
    # ... and the same layer in a built form does come here
    t = tags_of(ops.View(f(n, h, w, 16)), f(1, 1, 16, 16), ops.View(f(n, h, w, 16)), add=ops.View(f(n, h, w, 16)))
    assert _tag(16, 16) in t, t
