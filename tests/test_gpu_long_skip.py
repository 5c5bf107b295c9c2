"""The long skip of the residual backbone, out = relu(1x1(stem)) + relu(3x3(b)) (sp_postups.py:154-158), without its two element-wise
passes: the 3x3 convolution writes the sum as a second output (ConvEpilogue::sum_out: conv_split, conv_wino<3,3>), the dgrad that makes
the Add's output gradient stores both operands' masked gradients (ConvEpilogue::out2: conv_wino<3,3>).  Everything is compared bit for
bit with the stand-alone passes (add_act, masked_axpy_pair), op by op and through the graph (DL4DS_NO_LONG_SKIP_FUSION keeps them)."""
import numpy as np
import pytest

from tests.parity import kernel_tags

pytestmark = pytest.mark.gpu

GRIDS = [(2, 10, 14), (2, 7, 9)]        # ragged 2 x 2 tiles at both edges; odd extents


@pytest.fixture
def ops():
    import dl4ds_amd.ops as O
    return O


def _normal(shape, seed, zeros=0.0):
    rng = np.random.default_rng(seed)
    a = rng.standard_normal(shape).astype(np.float32)
    if zeros:
        a[rng.random(shape) < zeros] = 0.0
    return a


@pytest.fixture(scope='module')
def operands():
    """One set of arrays per (grid, channels), shared by the tests (never written)."""
    cache = {}

    def get(grid, ci, co):
        key = (grid, ci, co)
        if key not in cache:
            n, h, w = grid
            seed = 1000 * ci + 10 * co + h
            cache[key] = dict(x=_normal((n, h, w, ci), seed), wt=_normal((3, 3, ci, co), seed + 1) * np.float32(0.1),
                              b=_normal((co,), seed + 2), ma=_normal((n, h, w, co), seed + 3, 0.05),
                              mb=_normal((n, h, w, co), seed + 4, 0.05), s=_normal((n, h, w, co), seed + 5, 0.05))
        return cache[key]
    return get


@pytest.mark.parametrize('grid', GRIDS)
@pytest.mark.parametrize('ci,co', [(192, 48), (96, 48), (48, 48), (48, 40)])
def test_dual_mask_dgrad_epilogue_bit_for_bit(ops, operands, monkeypatch, grid, ci, co):
    """conv_wino<3,3> with four, two and one pass over the input channels (the masks ride on the last one; one pass: no partial sums)
    and with 40 output channels of the 48 tile: both masked outputs equal masked_axpy_pair on the unmasked convolution."""
    monkeypatch.setenv('DL4DS_WINO_FORCE', '2')          # (the product dispatch leaves grids this small to the streaming kernels)
    o = operands(grid, ci, co)
    (ya, yb, launched), tags = kernel_tags(lambda: ops.conv2d_dual_mask(o['x'], o['wt'], o['ma'], o['mb']))
    assert launched and tags.get('conv_wino<3,3>') == 1 and 'masked_axpy' not in tags, tags
    plain, tags = kernel_tags(lambda: ops.conv2d_epilogue(o['x'], o['wt']))
    assert tags.get('conv_wino<3,3>') == 1, tags
    ra, rb = ops.masked_axpy_pair(plain, o['ma'], o['mb'])
    assert (o['ma'] == 0).any() and (o['ma'] < 0).any() and (ra != 0).any() and (rb != 0).any()
    assert np.array_equal(ya, ra) and np.array_equal(yb, rb)


@pytest.mark.parametrize('grid', GRIDS)
@pytest.mark.parametrize('ci,co', [(48, 48), (40, 48)])
@pytest.mark.parametrize('path', ['conv_split<3,3>', 'conv_wino<3,3>'])
def test_sum_output_forward_epilogue_bit_for_bit(ops, operands, monkeypatch, grid, ci, co, path):
    """out = relu(conv + b) as the plain call stores it, sum_out = add_act(out, s) for an s with negative values and exact zeros."""
    if path.startswith('conv_split'):
        monkeypatch.setenv('DL4DS_SPLIT_FORCE', '2')
    else:
        monkeypatch.setenv('DL4DS_NO_SPLIT', '1')
        monkeypatch.setenv('DL4DS_WINO_FORCE', '2')
    o = operands(grid, ci, co)
    assert (o['s'] == 0).any() and (o['s'] < 0).any()
    (y, ys, launched), tags = kernel_tags(lambda: ops.conv2d_sum_output(o['x'], o['wt'], o['b'], o['s'], relu=True))
    assert launched and tags.get(path) == 1 and 'add_act' not in tags, tags
    plain, tags = kernel_tags(lambda: ops.conv2d_epilogue(o['x'], o['wt'], o['b'], relu=True))
    assert tags.get(path) == 1, tags
    assert (plain == 0).any() and (plain > 0).any()
    assert np.array_equal(y, plain)
    assert np.array_equal(ys, ops.add_act(plain, o['s'])) and np.array_equal(ys, ops.add_act(o['s'], plain))


def test_second_output_is_refused_where_no_kernel_has_the_form(ops, operands, monkeypatch):
    """A layer whose kernel has no second-output form launches nothing: the 48 -> 48 layer on the streaming kernels (no hook forces
    the Winograd / six-term kernels onto this grid), and the dual mask on the six-term kernel."""
    o = operands(GRIDS[0], 48, 48)
    (_, _, launched), tags = kernel_tags(lambda: ops.conv2d_sum_output(o['x'], o['wt'], o['b'], o['s'], relu=True))
    assert not launched and not tags, tags
    monkeypatch.setenv('DL4DS_SPLIT_FORCE', '2')
    monkeypatch.setenv('DL4DS_WINO_FORCE', '2')
    (_, _, launched), tags = kernel_tags(lambda: ops.conv2d_dual_mask(o['x'], o['wt'], o['ma'], o['mb']))
    assert not launched and not tags, tags


def _train_step(kind, scale, lr_size, batch, seed=5, **cfg):
    """One seeded MAE train step -> (loss, gradients, updated weights, kernel tags of the step)."""
    import dl4ds_amd.models as PM
    from dl4ds_amd.training import SupervisedEngine
    model = PM.net_postupsampling(kind, 'spc', scale, 1, 0, lr_size, seed=seed, **cfg)
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((batch,) + tuple(lr_size) + (1,)).astype(np.float32)
    y = rng.standard_normal((batch, lr_size[0] * scale, lr_size[1] * scale, 1)).astype(np.float32)
    eng = SupervisedEngine(model, loss='mae', learning_rate=1e-3)
    (loss, grads), tags = kernel_tags(lambda: eng.loss_and_grads([x], y))
    eng.step([x], y)
    return loss, grads, model.get_weights(), tags


def _ab(monkeypatch, kind, scale, lr_size=(12, 20), batch=3, **cfg):
    res = []
    for off in (False, True):
        if off:
            monkeypatch.setenv('DL4DS_NO_LONG_SKIP_FUSION', '1')
        else:
            monkeypatch.delenv('DL4DS_NO_LONG_SKIP_FUSION', raising=False)
        res.append(_train_step(kind, scale, lr_size, batch, **cfg))
    (l0, g0, w0, t0), (l1, g1, w1, t1) = res
    assert l0 == l1
    assert set(g0) == set(g1) and all(np.array_equal(g0[k], g1[k]) for k in g0), [k for k in g0 if not np.array_equal(g0[k], g1[k])]
    w0, w1 = (w if isinstance(w, dict) else dict(enumerate(w)) for w in (w0, w1))
    assert set(w0) == set(w1) and all(np.array_equal(w0[k], w1[k]) for k in w0)
    assert any(np.abs(g0[k]).max() > 0 for k in g0)
    return t0, t1


@pytest.mark.parametrize('no_split', [False, True])
def test_graph_long_skip_fused_equals_the_two_passes(monkeypatch, no_split):
    """Six residual blocks (48 channels, the 192 -> 48 dgrad of conv2x): loss, every gradient and every updated weight of a train step
    are those of the step with the stand-alone passes, and neither pass is launched."""
    monkeypatch.setenv('DL4DS_WINO_FORCE', '2')
    if no_split:
        monkeypatch.setenv('DL4DS_NO_SPLIT', '1')
    fused, plain = _ab(monkeypatch, 'resnet', 4)
    assert 'add_act' not in fused and 'masked_axpy' not in fused, fused
    assert plain.get('add_act') == 1 and plain.get('masked_axpy') == 1, plain
    assert 'conv_wino<3,3>' in fused


def test_graph_long_skip_on_the_six_term_kernel_keeps_the_backward_pass(monkeypatch):
    """With every eligible layer on conv_split (multi-pass dgrad included) the sum rides on backbone_last's conv_split launch and the
    backward keeps masked_axpy_pair: that kernel has no dual-mask form."""
    monkeypatch.setenv('DL4DS_SPLIT_FORCE', '2')
    monkeypatch.setenv('DL4DS_WINO_FORCE', '2')
    fused, plain = _ab(monkeypatch, 'resnet', 4)
    assert 'add_act' not in fused and fused.get('masked_axpy') == 1, fused
    assert plain.get('add_act') == 1 and plain.get('masked_axpy') == 1, plain
    assert 'conv_split<3,3>' in fused


def test_graph_long_skip_scale_2_folded_consumer(monkeypatch):
    """scale = 2: the Add's consumer is the folded convolution (d2s view), not a plain Conv2D.  Observed: the forward sum is fused, the
    backward keeps masked_axpy_pair (the planner only takes a plain Conv2D's dgrad); results are equal either way."""
    monkeypatch.setenv('DL4DS_WINO_FORCE', '2')
    fused, plain = _ab(monkeypatch, 'resnet', 2)
    assert plain.get('add_act') == 1 and plain.get('masked_axpy') == 1, plain
    assert 'add_act' not in fused and fused.get('masked_axpy') == 1, fused


def test_graph_convnext_long_skip_falls_back(monkeypatch):
    """ConvNext backbone: backbone_add has no ReLU operands and no 3x3 producer -- both passes stay, fused or not."""
    monkeypatch.setenv('DL4DS_WINO_FORCE', '2')
    fused, plain = _ab(monkeypatch, 'convnext', 2, lr_size=(8, 10), batch=2, normalization='ln', n_blocks=2)
    assert fused.get('add_act') == plain.get('add_act') and fused.get('add_act', 0) >= 1, (fused, plain)
