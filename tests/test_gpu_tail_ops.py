"""Op-level tests of the fused ops that close the spatio-temporal and post-upsampling models -- RecTailOp (csrc/graph_ops4.hip),
FoldedConvOp (csrc/graph_ops3.hip), ConvTOp / csrc/deconv.hip, LocalConvOp -- each against a float64 reference evaluated layer by
layer with oracle.torch_ops and differentiated by torch autograd (tests/tail_ops_ref.py), at the grids, channel counts and flag
combinations listed in tests/tail_ops_cases.py (the model-level tests compare one GPU path with another at B = 2 and reach none of
them).

Each case builds a one- to three-op graph with GraphBuilder, sets the case's weights (non-zero biases) with Model.set_weights, runs
forward through Model and backward through SupervisedEngine.loss_and_grads(loss='mse') against a random target, reads parameter
gradients from the returned dict and input gradients from dl4ds_graph_tensor_ptr(grad=1), and compares the forward output, every
input gradient and every parameter gradient with tests/test_gpu_ops.py's close(): max error below 2e-4 of the reference's max
magnitude.  Which kernel form ran is asserted through tests.parity.kernel_tags.  No float64 ReLU pre-activation of a reference lies
within 1e-4 of its tensor's max magnitude of zero (tests/test_tail_ops_cases.py), so a kernel within tolerance takes the branches of
the reference.

Worst observed max error / max |reference| per family over all cases (MI355X), next to the 2e-4 criterion it is held to:
                 forward    input gradients   parameter gradients   criterion
    rec_tail     2.7e-7     4.2e-7            3.4e-7                2e-4
    folded       1.2e-6     7.1e-7            4.5e-7                2e-4
    deconv       3.0e-7     4.7e-7            2.3e-7                2e-4
    localconv    1.6e-7     1.8e-7            3.6e-7                2e-4
Every comparison prints its figure before it asserts (pytest -s).

Partial-batch backward (BwdCtx b_off / b_cnt) is reachable only through the shared-group plan of the cGAN graphs, not from a two-op
graph built here: it stays covered by tests/test_gpu_trainers.py only."""
import ctypes

import numpy as np
import pytest

from tests import tail_ops_cases as K
from tests.parity import kernel_tags
from tests.tail_ops_ref import rel_err
from tests.test_gpu_ops import close

pytestmark = pytest.mark.gpu

F32 = np.float32
TOL = 2e-4                      # close()'s default, the criterion of every comparison here


# ------------------------------------------------------------------------------------------------------------------- plumbing
def _builder():
    from dl4ds_amd.graph import GraphBuilder
    return GraphBuilder()


def _model(g, out, case, w):
    from dl4ds_amd.graph import Model
    g.finalize(out, seed=0)
    m = Model(g, 'tail_ops', [s[1:] if s[0] == 1 else s for s, _, _ in case.inputs])
    m.set_weights({k: w(k, p['shape']) for k, p in g.params.items()})
    return m


def _read(g, t, batch, grad):
    from dl4ds_amd import _lib
    p = ctypes.c_void_p()
    _lib.check(_lib.lib().dl4ds_graph_tensor_ptr(g.h, t.id, int(grad), ctypes.byref(p)))
    assert p.value, 'tensor has no such buffer'
    a = np.empty((batch * t.nmul, t.H, t.W, t.C), F32)
    _lib.check(_lib.lib().dl4ds_memcpy_d2h(a.ctypes.data, p, a.nbytes))
    return a


def _graph(case, w, monkeypatch):
    for k, v in case.env:                    # test hooks the library reads while the op is created
        monkeypatch.setenv(k, v)
    g = _builder()
    xs = [g.input(H, W, C, nmul, requires_grad=grad) for (nmul, H, W, C), grad, _ in case.inputs]
    out = case.build(g, xs)
    return g, xs, out, _model(g, out, case, w)


def _check(case, what, got, ref):
    err = rel_err(got, ref)
    print(f'tail_ops {case.family} {case.id} {what} {err:.3e}')
    close(got, ref, TOL)


def _step(case, g, xs, out, m, eng, arrays, target, ref):
    """One forward and one loss_and_grads on ``arrays`` compared with ``ref`` -> the forward + backward tags."""
    B = arrays[0].shape[0]
    y = m(arrays)
    _check(case, 'y', y.reshape(ref['y'].shape), ref['y'])
    (_, grads), tags = kernel_tags(lambda: eng.loss_and_grads(arrays, target.reshape(y.shape)))
    for t, (_, grad, _), dx in zip(xs, case.inputs, ref['dx']):
        if grad:
            _check(case, f'd_input{t.id}', _read(g, t, B, 1), dx)
    assert set(grads) == set(ref['grads'])
    for k, v in ref['grads'].items():
        _check(case, f'd_{k}', grads[k], v)
    return tags


def _run(case, monkeypatch):
    from dl4ds_amd.training import SupervisedEngine
    d = K.make(case)
    g, xs, out, m = _graph(case, d['w'], monkeypatch)
    eng = SupervisedEngine(m, loss='mse', learning_rate=1e-3)
    tags = _step(case, g, xs, out, m, eng, d['arrays'], d['target'], d['ref'])
    print(f'tail_ops tags {case.id} {sorted(tags.items())}')
    for tag, n in case.tags:                 # a case that silently takes another kernel fails here
        assert tags.get(tag, 0) == n, (tag, n, tags)
    for tag in case.absent:
        assert tag not in tags, (tag, tags)
    if case.wgrad1x1:                        # plain rec_tail: three ordinary 1x1 weight-gradient launches per application, one per other convolution
        n = sum(v for k, v in tags.items() if k.startswith(('conv_wgrad', 'conv_narrow_wgrad')))
        assert n == case.wgrad1x1, tags
    return tags


# ------------------------------------------------------------------------------------------------------------------- the families
@pytest.mark.parametrize('case', K.REC_TAIL_CASES, ids=lambda c: c.id)
def test_rec_tail(monkeypatch, case):
    """Both kernel forms at every channel combination; staged: nblk = 1, 2, 9 (G = 9: the unrolled loop of tile() plus its scalar
    tail), 72 (G = 64: the group stride loop of rec_tail_wsum_kernel), T = 1; plain: a block over nine samples, HW = 255, 257, 289,
    120, T = 1, a 256-point grid under DL4DS_REC_TAIL_NO_STAGED; want_dx = 0, mask_x / mask_s, acc_dx / acc_ds, f.acc."""
    _run(case, monkeypatch)


@pytest.mark.parametrize('case', K.RT_STALE, ids=lambda c: c.id)
def test_rec_tail_batch_sizes_on_one_graph(monkeypatch, case):
    """B = 3, B = 1, B = 3 on one graph: the partial tiles, per-sample partials and saved activations of the larger batch are stale
    during the smaller one; every pass matches its own reference."""
    from dl4ds_amd.training import SupervisedEngine
    d = K.make(case)
    g, xs, out, m = _graph(case, d['w'], monkeypatch)
    eng = SupervisedEngine(m, loss='mse', learning_rate=1e-3)
    small = K.first_samples(case, d, 1)
    _step(case, g, xs, out, m, eng, d['arrays'], d['target'], d['ref'])
    _step(case, g, xs, out, m, eng, *small)
    _step(case, g, xs, out, m, eng, d['arrays'], d['target'], d['ref'])


@pytest.mark.parametrize('case', K.FOLDED_CASES, ids=lambda c: c.id)
def test_folded_conv(monkeypatch, case):
    """(ks, d2s, Cin, Cm, Co) with and without the auxiliary input, ReLU and tanh; K R2 = 2 (62 idle lanes in unfold_w2_kernel), Cm /
    Co not multiples of 4, d2s = 0 with ks = 1, masked and accumulated input gradients of the auxiliary form, w1 shared with a plain
    convolution in both creation orders (acc_w = 1 in the unfold kernels when the plain convolution comes later)."""
    _run(case, monkeypatch)


@pytest.mark.parametrize('case', K.FOLDED_REFUSED, ids=lambda c: c.id)
def test_folded_conv_aux_needs_four_output_channels(case):
    """The auxiliary form with Co % 4 != 0 is refused when the graph is built, not run on a path that cannot store it."""
    g = _builder()
    xs = [g.input(H, W, C, nmul, requires_grad=grad) for (nmul, H, W, C), grad, _ in case.inputs]
    with pytest.raises(Exception, match=case.raises):
        case.build(g, xs)


@pytest.mark.parametrize('case', K.DECONV_CASES, ids=lambda c: c.id)
def test_conv2d_transpose(monkeypatch, case):
    """Virtual kernels 5x5, 3x3 and 1x1 (KS = s); ReLU as graph output and in front of a convolution, dgrad with relu_mask and with
    accumulate, wgrad accumulate (one variable applied twice), output and gradient as channel slices of a Concatenate's buffers
    (both aliases asserted taken: no concat_join / concat_split / view_axpy launch)."""
    _run(case, monkeypatch)


@pytest.mark.parametrize('geom,chans,grid', K.DC_DIRECT)
def test_conv2d_transpose_accumulate_through_the_c_api(geom, chans, grid):
    """dl4ds_op_conv2d_transpose_dgrad / _wgrad with accumulate = 1 onto a non-zero destination."""
    import torch
    from dl4ds_amd import ops
    from oracle import torch_ops as T
    (ks, s), (ci, co), (h, w) = geom, chans, grid
    r = np.random.default_rng([ks, s, ci, co])
    x, wt = r.standard_normal((2, h, w, ci)).astype(F32), (r.standard_normal((ks, ks, co, ci)) * 0.2).astype(F32)
    dz = r.standard_normal((2, h * s, w * s, co)).astype(F32)
    xt, wtt = (torch.tensor(a, dtype=torch.float64, requires_grad=True) for a in (x, wt))
    (T.conv2d_transpose(xt, wtt, s) * torch.tensor(dz, dtype=torch.float64)).sum().backward()
    dx0 = (r.standard_normal(x.shape) * np.abs(xt.grad.numpy()).max()).astype(F32)
    dw0 = (r.standard_normal(wt.shape) * np.abs(wtt.grad.numpy()).max()).astype(F32)
    close(ops.conv2d_transpose_dgrad(dz, wt, s, accumulate=dx0), xt.grad.numpy() + dx0, TOL)
    close(ops.conv2d_transpose_wgrad(x, dz, ks, s, accumulate=dw0), wtt.grad.numpy() + dw0, TOL)
    close(ops.conv2d_transpose_dgrad(dz, wt, s), xt.grad.numpy(), TOL)
    close(ops.conv2d_transpose_wgrad(x, dz, ks, s), wtt.grad.numpy(), TOL)


@pytest.mark.parametrize('case', K.LOCALCONV_CASES, ids=lambda c: c.id)
def test_localconv(monkeypatch, case):
    """The compiled-in 2 -> 2 kernel and the run-time channel counts at N = 1, 5, 13 on 1x1, 3x2 and 9x11 grids, without bias, with
    accumulate_dx (a later-created consumer of the input) and accumulate_dw (one pair of variables on two inputs)."""
    _run(case, monkeypatch)
