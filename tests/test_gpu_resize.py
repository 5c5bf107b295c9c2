"""Op-level tests of the Resizing kernels of csrc/elementwise.hip: the table-driven family (resize_table_fwd / fwd4 / fwdk<2> / fwdk<4>,
resize_table_bwd / bwd4 / bwd4u<4> / bwd4u<8>), which every interpolation but 'nearest' runs in a graph -- bilinear included: the
direct bilinear kernels of test_gpu_ops.py::test_resize_bilinear are reached only under the experiments switch -- and
resize_nearest_fwd / resize_nearest_bwd.

Every graph's only compute op is the resize (two of them and an Add in the accumulation tests): the input is a graph input with
requires_grad, the resize is the output.  Forward runs through Model, backward through SupervisedEngine.loss_and_grads('mse') with
random targets, so dY is dense and varied.  dY and dX are read from the buffers the kernels wrote (dl4ds_graph_tensor_ptr(grad=1)),
and the expected dX is computed in float64 FROM THE dY READ BACK, by autograd through oracle.torch_ops' resize (the large cases: by
the axis matrices of tests/resize_cases.py, which tests/test_resize_cases.py holds to the same oracle): the comparison isolates the
resize kernel from the loss kernel.

Which kernel a case selects is a matter of shape alone (tests/resize_cases.py::select restates the launchers; the CPU test module
checks the restatement against the source and that every kernel is selected at least twice):

  bilinear C in {4, 8}, x2, x1/2, fractional, same size   fwdk<2> (C % 4 == 0, 2 x 2 taps)    bwd4u<4> (an input column feeds <= 4
                                                                                               taps: 4 at x2, 1 when shrinking)
  bilinear C in {4, 8}, x3, x4 (also T = 3, cfg4's form)   fwdk<2>                             bwd4u<8> (5 and 8 taps)
  bilinear C in {4, 8}, x5, x8                             fwdk<2>                             bwd4     (9 and 16 taps)
  bilinear C = 4, Wo 4 / 64; C = 8, Wo 40                  fwdk<2> on 64 threads: 4, 64 and 80 float4 per row (fast_div by 1; a
                                                           ragged second trip at 80)
  bilinear C = 16, Wo 64 / 70 / 72                         fwdk<2> on 256 threads: 256 (one trip), 280 and 288 float4 per row
  bilinear C = 4, 33 x 1024 x 1 -> 2048 x 2                fwdk<2> looping over 67584 rows with 65536 blocks
  bicubic C in {4, 8}, x2 / x3                             fwdk<4> (4 x 4 taps)                bwd4u<8> (8 taps) / bwd4 (9)
  mitchellcubic x2 on both axes                            fwdk<4> (widest span 4 on both)     bwd4u<8>
  lanczos3, lanczos5, gaussian; mitchellcubic x2 by x3     fwd4 (spans 6, 10, 3; 4 and 5)      bwd4 / bwd4u<8> / bwd4u<4>
  any method, C in {1, 2, 3, 6}                            fwd                                 bwd
  H or W of 1 on either side, 2 -> 3; C = 3 and C = 4      the scalar and the float4 kernels at their border arithmetic
  (3, 192, 256, 64) bilinear x1/2                          bwd4u<4> with 1.125 x (8192 * 256) float4 of dX: the grid-stride loop
  (3, 96, 128, 64) gaussian x2                             fwd4 with as many float4 of Y
  (1, 1024, 768, 3) bilinear x1/2 by x2                    fwd and bwd with 1.125 x (8192 * 256) elements each
  nearest                                                  resize_nearest_fwd                  resize_nearest_bwd

Strided views do not reach these kernels: g_resize counts its input as an "other" use, so it is never aliased into a Concatenate.

Tolerances.  Forward: max error over the tensor's maximum < 1e-5, the project's figure for these kernels.  dX of the table-driven
kernels: the transpose applies the same float32 weights in sums of the same length, and its evaluation in numpy float32 (weights
rounded to float32) differs from float64 by at most 1.5e-7 over all cases (tests/test_resize_cases.py asserts < 2.5e-6, a quarter
of the bound), so the same 1e-5.  Nearest: the forward is a copy, compared bitwise; dX is a float32 sum of k <= ceil(Ho / H) *
ceil(Wo / W) terms, off by at most (k - 1) * 2^-24 * sum |terms| per element -- asserted element-wise, and bitwise where k = 1.  A
second loss_and_grads on the same engine must reproduce the first dX bitwise.
"""
import ctypes

import numpy as np
import pytest

from oracle import np_ops as N
from tests import resize_cases as K
from tests.parity import kernel_tags

pytestmark = pytest.mark.gpu

F32 = np.float32


# ------------------------------------------------------------------------------------------------------------------- plumbing
def _read(g, t, batch, grad):
    from dl4ds_amd import _lib
    p = ctypes.c_void_p()
    _lib.check(_lib.lib().dl4ds_graph_tensor_ptr(g.h, t.id, int(grad), ctypes.byref(p)))
    assert p.value, 'tensor has no such buffer'
    a = np.empty((batch * t.nmul, t.H, t.W, t.C), F32)
    _lib.check(_lib.lib().dl4ds_memcpy_d2h(a.ctypes.data, p, a.nbytes))
    return a


class _Run:
    """One graph: x -> resize (``methods``: one per resize; two are summed by an Add) -> output."""

    def __init__(self, case, methods=None):
        from dl4ds_amd.graph import GraphBuilder, Model
        from dl4ds_amd.training import SupervisedEngine
        self.case, self.methods = case, tuple(methods or (case.method,))
        g = self.g = GraphBuilder()
        self.x_in = g.input(case.h, case.w, case.c, nmul=case.t, requires_grad=True)
        outs = [g.resize(self.x_in, case.ho, case.wo, name=f'resize{k}', interpolation=m) for k, m in enumerate(self.methods)]
        self.out = outs[0] if len(outs) == 1 else g.add(outs[0], outs[1])
        g.finalize(self.out, seed=0)
        assert not g.params
        self.x, self.target = K.case_input(case), K.case_target(case)
        self.model = Model(g, 'resize', [tuple(self.x.shape[1:])])
        self.engine = SupervisedEngine(self.model, loss='mse', learning_rate=1e-3)

    def forward(self):
        return K.flat(self.case, self.model([self.x]))

    def backward(self):
        """-> (dY, dX) as the loss kernel and the resize kernel left them."""
        self.engine.loss_and_grads([self.x], self.target)
        dy, dx = _read(self.g, self.out, self.case.n, 1), _read(self.g, self.x_in, self.case.n, 1)
        assert np.isfinite(dy).all() and np.count_nonzero(dy) >= 0.99 * dy.size, 'dY is not dense'
        return dy, dx


def _close(got, ref, tol, what):
    err = K.rel_err(got, ref)
    print(f'{what}: max error over the maximum {err:.3e} (bound {tol:.0e})')
    assert err < tol, f'{what}: {err:.3e}'


def _ids(cases):
    return [c.id for c in cases]


# ------------------------------------------------------------------------------------------------------------------- table-driven
@pytest.mark.parametrize('case', K.SMALL_TABLE, ids=_ids(K.SMALL_TABLE))
def test_table_resize(case):
    """Forward and dX per element against oracle.torch_ops (float64, autograd for the dY read back)."""
    r = _Run(case)
    y = r.forward()
    dy, dx = r.backward()
    y_ref, dx_ref = K.torch_refs(case, r.x, dy)
    _close(y, y_ref, K.FWD_TOL, f'{case.id} forward')
    _close(dx, dx_ref, K.DX_TOL, f'{case.id} dX')
    dy2, dx2 = r.backward()
    np.testing.assert_array_equal(dy2, dy)
    np.testing.assert_array_equal(dx2, dx, err_msg='the second iteration differs from the first')


LARGE_TABLE = [c for c in K.TABLE if c not in K.SMALL_TABLE]


@pytest.mark.parametrize('case', LARGE_TABLE, ids=_ids(LARGE_TABLE))
def test_table_resize_loops(case):
    """The loops that the small cases run once: fwdk over more rows than blocks, and the grid-stride loop of the float4 and scalar
    kernels over more than 8192 * 256 work items, forward and backward.  Reference: the axis matrices (BLAS)."""
    assert K.select(case)['loops'] & {'rows', 'grid_fwd', 'grid_bwd'}
    r = _Run(case)
    y = r.forward()
    dy, dx = r.backward()
    _close(y, K.forward_ref(case, r.x), K.FWD_TOL, f'{case.id} forward')
    _close(dx, K.backward_ref(case, dy), K.DX_TOL, f'{case.id} dX')


def test_graph_runs_the_table_kernels_for_bilinear():
    """A bilinear Resizing in a graph launches resize_table_fwd / resize_table_bwd, not the direct bilinear kernels; nearest has its
    own pair."""
    for case, fwd, bwd in ((K.BILINEAR_VEC[0], 'resize_table_fwd', 'resize_table_bwd'), (K.SCALAR[0], 'resize_table_fwd', 'resize_table_bwd'),
                           (K.NEAREST[0], 'resize_nearest_fwd', 'resize_nearest_bwd')):
        r = _Run(case)
        _, tf = kernel_tags(r.forward)
        _, tb = kernel_tags(r.backward)
        assert tf.get(fwd) == 1 and tb.get(fwd, 0) >= 1 and tb.get(bwd) == 1, (case.id, tf, tb)
        assert not any('resize_bilinear' in t for t in list(tf) + list(tb)), (case.id, tf, tb)


# ------------------------------------------------------------------------------------------------------------------- nearest
@pytest.mark.parametrize('case', K.NEAREST + K.NEAREST_LARGE, ids=_ids(K.NEAREST + K.NEAREST_LARGE))
def test_nearest_resize(case):
    """The forward is a copy: bitwise equal to oracle.np_ops.resize_nearest.  dX against the float64 sum of the dY read back, within
    (k - 1) * 2^-24 * sum |terms| per element."""
    r = _Run(case)
    np.testing.assert_array_equal(r.forward(), N.resize_nearest(K.flat(case, r.x), case.ho, case.wo))
    dy, dx = r.backward()
    ref, ref_abs = K.nearest_backward_ref(case, dy)
    bound = (K.nearest_terms(case) - 1) * 2.0 ** -24 * ref_abs
    excess = np.abs(dx.astype(np.float64) - ref) - bound
    print(f'{case.id} dX: k = {K.nearest_terms(case)}, largest error {np.abs(dx - ref).max():.3e}, largest bound {bound.max():.3e}')
    assert (excess <= 0).all(), f'{case.id}: {int((excess > 0).sum())} elements beyond their bound, worst by {excess.max():.3e}'
    _, dx2 = r.backward()
    np.testing.assert_array_equal(dx2, dx, err_msg='the second iteration differs from the first')


# ------------------------------------------------------------------------------------------------------------------- accumulation
@pytest.mark.parametrize('kind,case,second', K.ACCUMULATE, ids=[c.id for _, c, _ in K.ACCUMULATE])
def test_resize_backward_accumulates(kind, case, second):
    """add(resize(x, first method), resize(x, second method)): the resize created second runs its backward first and stores, the one
    created first -- the kernel named by ``kind`` -- runs second with accumulate = 1 (g.tensors[in].grad_written).  Expected
    dX = (M1^T + M2^T) dY; two different methods, so swapped operands or a dropped term cannot cancel.  A second loss_and_grads on the
    same engine reproduces the first bitwise: no stale grad_written, no accumulation across iterations."""
    assert K.select(case)['bwd'] == kind
    r = _Run(case, (case.method, second))
    y = r.forward()
    dy, dx = r.backward()
    y_ref, dx_ref = K.torch_refs(case, r.x, dy, r.methods)
    _close(y, y_ref, K.FWD_TOL, f'{case.id} forward')
    _close(dx, dx_ref, K.DX_TOL, f'{case.id} dX')
    # neither term alone passes: the test can tell a store from an accumulation
    for m in r.methods:
        assert K.rel_err(K.torch_refs(case, r.x, dy, (m,))[1], dx_ref) > 100 * K.DX_TOL
    dy2, dx2 = r.backward()
    np.testing.assert_array_equal(dy2, dy)
    np.testing.assert_array_equal(dx2, dx, err_msg='the second iteration differs from the first')
