"""Float64 references of tests/test_gpu_tail_ops.py (not a test module; needs no GPU).

``RefBuilder`` has the op methods of ``dl4ds_amd.graph.GraphBuilder`` that the cases of tests/tail_ops_cases.py call, so ONE function
per case builds the graph under test and its reference.  Every op is evaluated layer by layer with ``oracle.torch_ops`` on float64
tensors -- rec_tail as expand_repeat_time, concat, conv2d 1x1, relu, locally_connected_1x1, concat, conv2d 1x1, relu; the folded
convolution as its two convolutions with depth_to_space (and concat for the auxiliary form) in between -- and the gradients are
torch autograd's.  Nothing of the kernels' fused algebra (composed filters, split 1x1 kernels, time-summed gradients) is restated.
Every ReLU's float64 pre-activation is recorded (``relus``) for the margin checks of tests/test_tail_ops_cases.py."""
import numpy as np

DELTA = 1e-4            # every ReLU pre-activation keeps |v| >= DELTA * max|v|: half of close()'s 2e-4, so a kernel within tolerance keeps its branch
MIN_SIDE = 0.2          # share of a ReLU's elements on either side


class RefTensor:
    def __init__(self, t, nmul=1):
        self.t, self.nmul = t, nmul
        _, self.H, self.W, self.C = t.shape

    @property
    def shape(self):
        return (self.nmul, self.H, self.W, self.C)


class RefBuilder:
    def __init__(self, weight_of, arrays):
        """``weight_of(name, shape)`` -> float32 array; ``arrays``: the input arrays in creation order, (B, [T,] H, W, C)."""
        self.weight_of, self.arrays = weight_of, arrays
        self.params, self.inputs, self.relus = {}, [], []

    # ---------------------------------------------------------------- tensors / params
    def input(self, H, W, C, nmul=1, requires_grad=False):
        import torch
        a = np.asarray(self.arrays[len(self.inputs)], np.float64).reshape(-1, H, W, C)
        t = RefTensor(torch.tensor(a, requires_grad=True), nmul)
        self.inputs.append(t)
        return t

    def param(self, name, shape):
        import torch
        if name not in self.params:
            w = np.asarray(self.weight_of(name, tuple(shape)), np.float64)
            assert w.shape == tuple(shape), (name, w.shape, shape)
            self.params[name] = torch.tensor(w, requires_grad=True)
        assert tuple(self.params[name].shape) == tuple(shape), name
        return self.params[name]

    def _relu(self, name, v):
        from oracle import torch_ops as T
        self.relus.append((name, v.detach().numpy().reshape((-1,) + tuple(v.shape[-3:]))))
        return T.relu(v)

    def _act(self, name, v, activation):
        from oracle import torch_ops as T
        if activation in (None, 'linear'):
            return v
        return self._relu(name, v) if activation == 'relu' else T.activation(v, activation)

    # ---------------------------------------------------------------- ops
    def conv2d(self, x, name, filters, ks, use_bias=True, activation=None, add=None, d2s=0):
        from oracle import torch_ops as T
        r2 = d2s * d2s if d2s and d2s > 1 else 1
        w = self.param(name + '/kernel', (ks, ks, x.C, filters))
        b = self.param(name + '/bias', (filters,)) if use_bias else None
        v = T.conv2d(x.t, w, b)
        if add is not None:
            v = T.add(v, add.t)
        v = self._act(name, v, activation)
        if r2 > 1:
            v = T.depth_to_space(v, d2s)
        return RefTensor(v, x.nmul)

    def conv2d_folded(self, x, name, filters, ks, d2s, name2, filters2, activation=None, aux=None):
        from oracle import torch_ops as T
        r2 = d2s * d2s if d2s and d2s > 1 else 1
        w1 = self.param(name + '/kernel', (ks, ks, x.C, r2 * filters))
        b1 = self.param(name + '/bias', (r2 * filters,))
        w2 = self.param(name2 + '/kernel', (1, 1, filters + (aux.C if aux is not None else 0), filters2))
        b2 = self.param(name2 + '/bias', (filters2,))
        v = T.conv2d(x.t, w1, b1)
        if r2 > 1:
            v = T.depth_to_space(v, d2s)
        if aux is not None:
            v = T.concat([v, aux.t])
        return RefTensor(self._act(name2, T.conv2d(v, w2, b2), activation), x.nmul)

    def conv2d_transpose(self, x, name, filters, ks, stride, activation=None):
        from oracle import torch_ops as T
        w = self.param(name + '/kernel', (ks, ks, filters, x.C))
        return RefTensor(self._act(name, T.conv2d_transpose(x.t, w, stride), activation), x.nmul)

    def localconv(self, x, name, filters=2, use_bias=True):
        import torch
        from oracle import torch_ops as T
        w = self.param(name + '/kernel', (x.H, x.W, x.C, filters))
        b = self.param(name + '/bias', (x.H, x.W, filters)) if use_bias else torch.zeros((x.H, x.W, filters), dtype=torch.float64)
        return RefTensor(T.locally_connected_1x1(x.t, w, b), x.nmul)

    def rec_tail(self, x, s, T_, co, lcb_name='LocalizedConvBlock', tl_name='TransitionLast'):
        from oracle import torch_ops as T
        c24 = x.C + s.C
        wt = self.param(lcb_name + '/transition/conv/kernel', (1, 1, c24, 2))
        bt = self.param(lcb_name + '/transition/conv/bias', (2,))
        wl = self.param(lcb_name + '/localconv/kernel', (x.H, x.W, 2, 2))
        bl = self.param(lcb_name + '/localconv/bias', (x.H, x.W, 2))
        w = self.param(tl_name + '/conv/kernel', (1, 1, c24 + 2, co))
        b = self.param(tl_name + '/conv/bias', (co,))
        assert x.nmul == T_ and s.nmul == 1
        B = s.t.shape[0]
        x5 = x.t.reshape(B, T_, x.H, x.W, x.C)
        x24 = T.concat([x5, T.expand_repeat_time(s.t, T_)])
        u = self._relu(lcb_name + '/transition', T.conv2d(x24, wt, bt))
        lws = T.locally_connected_1x1(u.reshape(B * T_, x.H, x.W, 2), wl, bl).reshape(B, T_, x.H, x.W, 2)
        y = self._relu(tl_name, T.conv2d(T.concat([x24, lws]), w, b))
        return RefTensor(y.reshape(B * T_, x.H, x.W, co), T_)

    def concat(self, xs, name='concat'):
        from oracle import torch_ops as T
        return RefTensor(T.concat([t.t for t in xs]), xs[0].nmul)

    def add(self, a, b, relu=False, name='add'):
        from oracle import torch_ops as T
        v = T.add(a.t, b.t)
        return RefTensor(self._relu(name, v) if relu else v, a.nmul)

    def repeat_time(self, x, T_, name='repeat_time'):
        from oracle import torch_ops as T
        v = T.expand_repeat_time(x.t, T_)
        return RefTensor(v.reshape((-1,) + tuple(v.shape[2:])), T_)


def run(build, specs, arrays, weight_of, target=None):
    """``build(g, inputs) -> out`` on a RefBuilder.  -> dict(y (N, H, W, C), relus [(name, pre-activation)]) and, with ``target``
    (the MSE target, any shape of y's size), dx [one (N, H, W, C) gradient per input] and grads {name: gradient} of
    mean((y - target)^2)."""
    import torch
    g = RefBuilder(weight_of, arrays)
    xs = [g.input(H, W, C, nmul, grad) for (nmul, H, W, C), grad, _ in specs]
    out = build(g, xs)
    res = dict(y=out.t.detach().numpy(), relus=g.relus)
    if target is not None:
        t = torch.tensor(np.asarray(target, np.float64).reshape(res['y'].shape))
        ((out.t - t) ** 2).mean().backward()
        res['dx'] = [x.t.grad.numpy() if x.t.grad is not None else None for x in xs]
        res['grads'] = {k: (p.grad.numpy() if p.grad is not None else np.zeros(tuple(p.shape))) for k, p in g.params.items()}
    return res


def margin_report(relus, delta=DELTA):
    """-> [(name, elements within delta * max|v| of zero, share of positive elements)] per recorded ReLU."""
    rows = []
    for name, v in relus:
        m = np.abs(v).max()
        rows.append((name, int((np.abs(v) < delta * m).sum()), float((v > 0).mean())))
    return rows


def rel_err(got, ref):
    """max |got - ref| over max |ref|: the figure of tests/test_gpu_ops.py's close()."""
    ref, got = np.asarray(ref, np.float64), np.asarray(got, np.float64)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    return float(np.abs(got - ref).max() / max(np.abs(ref).max(), 1e-6))
