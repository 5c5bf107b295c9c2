"""Op-level tests of csrc/norm.hip (ln_fwd_kernel / ln_bwd_kernel<1 / 4>, partial_reduce_kernel, bn_stats / bn_finalize / bn_apply /
bn_bwd_reduce / bn_bwd_finalize / bn_bwd_apply) and csrc/dwconv.hip (dwconv_kernel, dwconv_wgrad_kernel<7, 1 / 4>,
dwconv_reduce_kernel) in the forms tests/test_gpu_ops.py does not reach: accumulate = 1 onto preloaded gradients, null dx / dgamma /
dbeta / db, more than 64 partial slabs, the block caps (1024 blocks with a growing chunk or a second grid-stride trip, 512 chunks),
a last chunk shorter than the others, one pixel per channel.  tests/norm_cases.py restates the launch geometry and holds the cases;
the CPU module tests/test_norm_cases.py ties the restatement to the source and shows each form selected twice and each case
sensitive to the loss of the work it is there for.

1. Eager (ops.layernorm / ops.batchnorm / ops.dwconv), one test per case:
   - y, dx, dgamma / dk, dbeta / db against oracle.torch_ops in float64 with autograd, max error over max |reference|, bounds as in
     tests/test_gpu_ops.py (y 1e-4 LayerNorm, 2e-4 BatchNorm and depthwise; depthwise dx 2e-4; every other gradient 1e-3); on
     accumulate cases the preload (of the gradient's own magnitude) is part of the expected result;
   - a second call with integer dy in [-4, 4] and no ReLU: dbeta / db equals the integer sum (plus an integer preload) exactly;
   - BatchNorm: on integer x the saved batch mean lies within 2 ulp; moving averages by the formula of test_batchnorm; one pixel
     per channel gives y = [relu](beta) to the rounding of x * gamma / sqrt(eps) (the kernel evaluates x a + (beta - mean a)),
     moving_variance updated with variance 0, dx = dgamma = 0, no NaN;
   - null outputs: what is requested equals, bitwise, the same call with everything requested; a dbeta / db buffer passed next to a
     null dgamma / dk comes back untouched (partial_reduce_kernel returns, bn_bwd_finalize_kernel and dl4ds_op_dwconv_bwd skip);
   - a second backward call reproduces the first bitwise.
2. In a graph (GraphBuilder -> Model, SupervisedEngine.loss_and_grads('mse'), tensors through dl4ds_graph_tensor_ptr, expected
   gradients by float64 autograd FROM THE dY READ BACK):
   (a) x = conv1x1(input); out = add(norm(x), x): the norm's backward runs acc_dx = 1 (checked through dInput and the convolution's
       gradients, which see x.grad); float4, scalar, 5-D; 'ln' and 'bn'; ReLU fused and not;
   (b) two norms under one name: the second backward runs acc_dw = 1; 'bn': the moving averages equal two updates in call order;
   (c) a norm on the graph's input: dx == nullptr;
   (d) 'bn' forward in inference mode: output from the moving statistics, which stay bitwise unchanged;
   (e) two depthwise layers under one name, with and without bias: dk (and db) accumulate;
   a second iteration reproduces the first bitwise.

Observed on the MI355X, largest over the cases (every test prints its own figures), next to the bound:
  LayerNorm   eager: y 5.9e-07 (1e-4), dx 7.9e-07 (1e-3), dgamma 1.9e-07 (1e-3), dbeta 3.1e-07 (1e-3)
  BatchNorm   eager: y 3.0e-05 (2e-4; one pixel per channel, where y = beta is what is left of x a - mean a: 3.3e-06 absolute against
              an element-wise bound of 3.8e-05; 2.1e-06 on every other case), dx 2.0e-06 (1e-3), dgamma 1.4e-05 (1e-3; at C = 1, the
              sum over 30 pixels cancels to a tenth of its terms; 4.9e-06 otherwise), dbeta 1.7e-07 (1e-3); saved mean 5.8e-07,
              saved 1 / std 1.8e-06; batch mean of integers within 0.50 ulp (bound 2)
  depthwise   eager: y 3.2e-07 (2e-4), dx 2.3e-07 (2e-4), dk 1.6e-07 (1e-3), db 1.3e-07 (1e-3)
  in a graph  y 6.6e-07, dX 9.5e-07 (1e-3; 2e-4 depthwise), parameter gradients 7.5e-07 (1e-3)
  dbeta / db of integer dy equalled the integer sum in every case; every null-output, canary and second-call comparison was bitwise.
No case found a defect in norm.hip, dwconv.hip or the graph operators.
"""
import ctypes

import numpy as np
import pytest

from tests import norm_cases as K

pytestmark = pytest.mark.gpu

F32 = np.float32
OBSERVED = {}


@pytest.fixture(scope='module')
def ops():
    import dl4ds_amd.ops as o
    return o


def _ids(cases):
    return [c.id for c in cases]


def _close(got, ref, what, tol):
    err = K.rel_err(got, ref)
    kind = what.split(' ', 1)[0] + ' ' + what.rsplit(' ', 1)[1]
    OBSERVED[kind] = max(OBSERVED.get(kind, 0.0), err)
    print(f'{what}: max error over the maximum {err:.3e} (bound {tol:.0e}; largest so far for {kind}: {OBSERVED[kind]:.3e})')
    assert err < tol, f'{what}: {err:.3e} (bound {tol:.0e})'


def _same(a, b, what):
    assert (a is None) == (b is None), what
    if a is not None:
        np.testing.assert_array_equal(a, b, err_msg=what)


# ------------------------------------------------------------------------------------------------------------------- 1. eager norms
def _norm_call(ops, op, d, case, **kw):
    """-> dict(y, dx, dgamma, dbeta[, mm, mv, saved]) of one forward + backward call."""
    args = dict(x=d['x'], dy=d['dy'], relu=case.relu, want_dx=case.dx, want_dw=case.dw,
                accumulate_into=d['pre'] if case.acc else None)
    args.update(kw)
    x = args.pop('x')
    if op == 'ln':
        r = ops.layernorm(x, d['gamma'], d['beta'], **args)
        return dict(zip(('y', 'dx', 'dgamma', 'dbeta'), r))
    r = ops.batchnorm(x, d['gamma'], d['beta'], d['mm'], d['mv'], return_saved=True, **args)
    return dict(zip(('y', 'mm', 'mv', 'dx', 'dgamma', 'dbeta', 'saved'), r))


def _check_norm(ops, op, case):
    d = K.inputs(op, case)
    tol = K.TOL[op]
    C = case.shape[-1]
    npix = int(np.prod(case.shape[:-1]))
    tag = f'{op} {case.id}'
    ref = K.reference(op, case, d)
    got = _norm_call(ops, op, d, case)
    assert all(np.isfinite(v).all() for v in got.values() if v is not None), f'{tag}: NaN or Inf'
    _close(got['y'], ref['y'], f'{tag} y', tol['y'])
    wanted = K.outputs(op, case)
    for n in ('dx', 'dgamma', 'dbeta'):
        if n not in wanted:
            assert got[n] is None
        elif n == 'dx' and op == 'ln' and C == 1:
            # a single channel normalises to exactly beta: dx is identically 0, up to rounding / sqrt(eps) (test_layernorm)
            assert np.abs(got['dx'] - (d['pre'][0] if case.acc else 0)).max() < 1e-6 / np.sqrt(1e-3)
        else:
            _close(got[n], ref[n], f'{tag} {n}', tol[n])
    if op == 'bn':
        n = float(npix)
        unbiased = ref['var'] * n / (n - 1) if npix > 1 else ref['var']
        np.testing.assert_allclose(got['mm'], 0.99 * d['mm'] + 0.01 * ref['mean'], rtol=1e-5, atol=1e-6)
        np.testing.assert_allclose(got['mv'], 0.99 * d['mv'] + 0.01 * unbiased, rtol=1e-4, atol=1e-6)
        _close(got['saved'][0], ref['mean'], f'{tag} saved_mean', 2e-4)
        _close(got['saved'][1], 1 / np.sqrt(ref['var'] + K.BN_EPS), f'{tag} saved_invstd', 2e-4)
        if npix == 1:
            beta = d['beta'].astype(np.float64)
            want = np.maximum(beta, 0) if case.relu else beta
            bound = 4 * 2.0 ** -24 * np.abs(d['x'].reshape(-1).astype(np.float64) * d['gamma']) / np.sqrt(K.BN_EPS) + 2.0 ** -24
            err = np.abs(got['y'].reshape(-1) - want)
            print(f'{tag}: |y - beta| at most {err.max():.3e} (element-wise bound at most {bound.max():.3e})')
            assert (err <= bound).all()
            np.testing.assert_allclose(got['mv'], 0.99 * d['mv'], rtol=1e-6, atol=0)
            if case.dx:
                baseline = d['pre'][0].reshape(-1) if case.acc else 0
                np.testing.assert_array_equal(got['dx'].reshape(-1), np.zeros(C, F32) + baseline)
    # null outputs: bitwise the same as with everything requested; a buffer next to a null dgamma stays as it was
    if not (case.dx and case.dw):
        full = _norm_call(ops, op, d, case, want_dx=True, want_dw=True)
        for n in ['y'] + wanted:
            _same(got[n], full[n], f'{tag}: {n} with a null output differs from {n} with every output requested')
    if not case.dw:
        can = _norm_call(ops, op, d, case, want_dw='canary')
        assert can['dgamma'] is None
        np.testing.assert_array_equal(can['dbeta'], np.full(C, ops.CANARY, F32), err_msg=f'{tag}: dbeta written next to a null dgamma')
        _same(can['dx'], got['dx'], f'{tag}: dx')
    # fixed-order reductions
    again = _norm_call(ops, op, d, case)
    for n in ('y', 'dx', 'dgamma', 'dbeta'):
        _same(again[n], got[n], f'{tag}: {n} of a second call differs from the first')
    # exact bias sums (and, for BatchNorm, the batch mean of integers)
    pre = (None, None, d['prei']) if case.acc else None
    it = _norm_call(ops, op, d, case, x=d['xi'] if op == 'bn' else d['x'], dy=d['dyi'], relu=False, want_dw=True, accumulate_into=pre)
    exact = d['dyi'].reshape(-1, C).astype(np.float64).sum(0) + (d['prei'] if case.acc else 0)
    np.testing.assert_array_equal(it['dbeta'].astype(np.float64), exact, err_msg=f'{tag}: dbeta of integer dy is not the integer sum')
    if op == 'bn':
        mean = d['xi'].reshape(-1, C).astype(np.float64).mean(0)
        ulp = np.spacing(np.abs(mean).astype(F32)).astype(np.float64)
        off = np.abs(it['saved'][0] - mean) / ulp
        print(f'{tag}: batch mean of integers off by at most {off.max():.2f} ulp')
        assert (off <= 2).all()


@pytest.mark.parametrize('case', K.LN_CASES, ids=_ids(K.LN_CASES))
def test_eager_layernorm(ops, case):
    _check_norm(ops, 'ln', case)


@pytest.mark.parametrize('case', K.BN_CASES, ids=_ids(K.BN_CASES))
def test_eager_batchnorm(ops, case):
    _check_norm(ops, 'bn', case)


# ------------------------------------------------------------------------------------------------------------------- 1. eager depthwise
def _dw_call(ops, d, case, **kw):
    args = dict(dy=d['dy'], accumulate_into=d['pre'] if case.acc else None, want_dx=case.dx, want_db=case.dw)
    args.update(kw)
    return dict(zip(('y', 'dx', 'dk', 'db'), ops.dwconv(d['x'], d['k'], d['b'] if case.dw else None, **args)))


@pytest.mark.parametrize('case', K.DW_CASES, ids=_ids(K.DW_CASES))
def test_eager_depthwise(ops, case):
    d = K.inputs('dw', case)
    tol = K.TOL['dw']
    C = case.shape[-1]
    tag = f'dw {case.id}'
    ref = K.reference('dw', case, d)
    got = _dw_call(ops, d, case)
    _close(got['y'], ref['y'], f'{tag} y', tol['y'])
    wanted = K.outputs('dw', case)
    for n in ('dx', 'dk', 'db'):
        if n in wanted:
            _close(got[n], ref[n].reshape(got[n].shape), f'{tag} {n}', tol[n])
        else:
            assert got[n] is None
    if not (case.dx and case.dw):
        full = _dw_call(ops, d, case, want_dx=True, want_db=True)
        for n in ['y'] + wanted:
            _same(got[n], full[n], f'{tag}: {n} with a null output differs from {n} with every output requested')
        can = _dw_call(ops, d, case, want_dk='canary', want_db=True)
        assert can['dk'] is None
        np.testing.assert_array_equal(can['db'], np.full(C, ops.CANARY, F32), err_msg=f'{tag}: db written without a weight-gradient pass')
        _same(can['dx'], got['dx'], f'{tag}: dx')
    again = _dw_call(ops, d, case)
    for n in ('y', 'dx', 'dk', 'db'):
        _same(again[n], got[n], f'{tag}: {n} of a second call differs from the first')
    pre = (None, None, d['prei']) if case.acc else None
    it = _dw_call(ops, d, case, dy=d['dyi'], want_db=True, accumulate_into=pre)
    exact = d['dyi'].reshape(-1, C).astype(np.float64).sum(0) + (d['prei'] if case.acc else 0)
    np.testing.assert_array_equal(it['db'].astype(np.float64), exact, err_msg=f'{tag}: db of integer dy is not the integer sum')


# ------------------------------------------------------------------------------------------------------------------- graph plumbing
def _read(g, t, batch, grad):
    from dl4ds_amd import _lib
    p = ctypes.c_void_p()
    _lib.check(_lib.lib().dl4ds_graph_tensor_ptr(g.h, t.id, int(grad), ctypes.byref(p)))
    assert p.value, 'tensor has no such buffer'
    a = np.empty((batch * t.nmul, t.H, t.W, t.C), F32)
    _lib.check(_lib.lib().dl4ds_memcpy_d2h(a.ctypes.data, p, a.nbytes))
    return a


def _dense(dy):
    assert np.isfinite(dy).all() and np.count_nonzero(dy) >= 0.99 * dy.size, 'dY is not dense'
    return dy


MOVING = ('n/moving_mean', 'n/moving_variance')


class _Graph:
    """The graphs of section 2 (modes 'residual', 'shared', 'first', 'infer', 'dw'; tests/norm_cases.py::graph_norm_ref)."""

    def __init__(self, case, mode):
        from dl4ds_amd.graph import GraphBuilder, Model
        from dl4ds_amd.training import SupervisedEngine
        self.case, self.mode, self.inp = case, mode, K.graph_inputs(case, mode)
        s = case.shape
        C = s[-1]
        t5 = s[1] if len(s) == 5 else 0
        n_in = len(self.inp['xs'])
        g = self.g = GraphBuilder()
        self.x_in = [g.input(s[-3], s[-2], C, nmul=t5 or 1, requires_grad=mode not in ('first', 'infer')) for _ in range(n_in)]
        act = 'relu' if case.relu else None
        if mode == 'residual':
            p = g.conv2d(self.x_in[0], 'p', C, 1)
            self.out = g.add(g.norm(p, 'n', case.kind, activation=act), p)
        elif mode == 'shared':
            a, b = [g.norm(x, 'n', case.kind, activation=act) for x in self.x_in]
            self.out = g.add(a, b)
        elif mode == 'dw':
            a, b = [g.dwconv(x, 'd', use_bias=case.relu) for x in self.x_in]
            self.out = g.add(a, b)
        else:
            self.out = g.norm(self.x_in[0], 'n', case.kind, activation=act)
        g.finalize(self.out, seed=0)
        extra = set(MOVING) if case.kind == 'bn' else set()
        assert set(g.params) == set(self.inp['w']) | extra, 'the layers do not share their parameters'
        for k, v in self.inp['w'].items():
            g.set_param(k, v)
        self.reset_moving()
        self.model = Model(g, 'norm', [tuple(s[1:])] * n_in)
        self.engine = SupervisedEngine(self.model, loss='mse', learning_rate=1e-3)

    def reset_moving(self):
        if self.case.kind == 'bn':
            self.g.set_param(MOVING[0], self.inp['mm'])
            self.g.set_param(MOVING[1], self.inp['mv'])

    def moving(self):
        return [self.g.get_param(k) for k in MOVING]

    def backward(self):
        """-> (y of the training-mode forward, dY, [dX per input that has one], {name: parameter gradient})."""
        _, grads = self.engine.loss_and_grads(self.inp['xs'], self.inp['target'])
        B, s = self.case.shape[0], self.case.shape
        y = _read(self.g, self.out, B, 0).reshape(s)
        dy = _dense(_read(self.g, self.out, B, 1)).reshape(s)
        dxs = [_read(self.g, x, B, 1).reshape(s) for x in self.x_in] if self.mode not in ('first', 'infer') else []
        return y, dy, dxs, {k: grads[k] for k in self.inp['w']}


def _same_again(first, second, what):
    np.testing.assert_array_equal(second[0], first[0], err_msg=f'{what}: y')
    np.testing.assert_array_equal(second[1], first[1], err_msg=f'{what}: dY')
    for a, b in zip(first[2], second[2]):
        np.testing.assert_array_equal(b, a, err_msg=f'{what}: dX of the second iteration differs from the first')
    for k in first[3]:
        np.testing.assert_array_equal(second[3][k], first[3][k], err_msg=f'{what}: d({k}) of the second iteration differs from the first')


def _check_graph(case, mode):
    r = _Graph(case, mode)
    inp = r.inp
    first = r.backward()
    y, dy, dxs, grads = first
    after_one = r.moving() if case.kind == 'bn' else None
    tol = K.TOL[case.kind]
    tag = f'graph {mode}/{case.id}'
    y_ref, dx_ref, g_ref = K.graph_norm_ref(case, inp['xs'], inp['w'], dy, mode)
    _close(y, y_ref, f'{tag} y', tol['y'])
    for a, b in zip(dxs, dx_ref):
        _close(a, b, f'{tag} dX', tol['dx'])
    for k in inp['w']:
        _close(grads[k], g_ref[k], f'{tag} dW', 1e-3)
    if case.kind == 'bn':
        from oracle import np_ops as N
        mm, mv = inp['mm'].astype(np.float64), inp['mv'].astype(np.float64)
        if mode == 'residual':
            calls = [N.conv2d(inp['xs'][0].astype(np.float64), inp['w']['p/kernel'].astype(np.float64), inp['w']['p/bias'].astype(np.float64))]
        else:
            calls = [x.astype(np.float64) for x in inp['xs']]
        for v in calls:                                    # one update per norm, in call order
            mu, var = N.channel_moments(v)
            n = v.size // v.shape[-1]
            mm, mv = 0.99 * mm + 0.01 * mu, 0.99 * mv + 0.01 * var * n / (n - 1)
        np.testing.assert_allclose(after_one[0], mm, rtol=1e-5, atol=1e-6)
        np.testing.assert_allclose(after_one[1], mv, rtol=1e-4, atol=1e-6)
    _same_again(first, r.backward(), tag)


@pytest.mark.parametrize('case', K.G_RESIDUAL, ids=_ids(K.G_RESIDUAL))
def test_graph_norm_accumulates_into_dx(case):
    """x = conv1x1(input); out = add(norm(x), x): the Add's backward writes x.grad, the norm's adds to it (acc_dx = 1).  The norm's
    share alone misses dInput and the convolution's kernel gradient by 10 x the tolerance or more (tests/test_norm_cases.py)."""
    _check_graph(case, 'residual')


@pytest.mark.parametrize('case', K.G_SHARED, ids=_ids(K.G_SHARED))
def test_graph_norms_share_parameters(case):
    """out = add(norm(x1), norm(x2)) under one name: the norm created second runs its backward first and stores dgamma / dbeta, the
    first adds to them (acc_dw = 1)."""
    _check_graph(case, 'shared')


@pytest.mark.parametrize('case', K.G_FIRST, ids=_ids(K.G_FIRST))
def test_graph_norm_on_the_input_has_no_dx(case):
    _check_graph(case, 'first')


@pytest.mark.parametrize('case', K.G_INFER, ids=_ids(K.G_INFER))
def test_graph_batchnorm_inference(case):
    """The inference-mode forward inside a graph normalises with the moving statistics and leaves them bitwise unchanged."""
    r = _Graph(case, 'infer')
    x = r.inp['xs'][0]
    before = r.moving()
    y = r.model([x])
    mm, mv = r.inp['mm'].astype(np.float64), r.inp['mv'].astype(np.float64)
    ref = (x.astype(np.float64) - mm) / np.sqrt(mv + 1e-3) * r.inp['w']['n/gamma'] + r.inp['w']['n/beta']
    _close(y, np.maximum(ref, 0) if case.relu else ref, f'graph infer/{case.id} y', K.TOL['bn']['y'])
    for a, b, k in zip(before, r.moving(), MOVING):
        np.testing.assert_array_equal(b, a, err_msg=k)
    np.testing.assert_array_equal(before[0], r.inp['mm'])
    np.testing.assert_array_equal(r.model([x]), y)


@pytest.mark.parametrize('case', K.G_DW, ids=_ids(K.G_DW))
def test_graph_depthwise_layers_share_parameters(case):
    """out = add(dw(x1), dw(x2)) under one name, with and without bias: the second backward accumulates dk (and db)."""
    r = _Graph(case, 'dw')
    first = r.backward()
    y, dy, dxs, grads = first
    tag = f'graph dw/{case.id}'
    y_ref, dx_ref, g_ref = K.graph_dw_ref(case, r.inp['xs'], r.inp['w'], dy)
    _close(y, y_ref, f'{tag} y', K.TOL['dw']['y'])
    for a, b in zip(dxs, dx_ref):
        _close(a, b, f'{tag} dX', K.TOL['dw']['dx'])
    for k in r.inp['w']:
        _close(grads[k], g_ref[k], f'{tag} dW', 1e-3)
    _same_again(first, r.backward(), tag)
