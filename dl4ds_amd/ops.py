"""numpy-in / numpy-out wrappers over the single-op C-ABI entry points (dl4ds_op_*).

Each call uploads its operands to HBM, runs the gfx950 kernel and downloads the result -- meant for
unit tests and experiments, not for speed (the train step runs through the graph runtime instead).
Layouts follow Keras: activations NHWC, conv kernels HWIO, transposed-conv kernels HWOI.
"""
import ctypes
import numpy as np
from . import _lib
from .device import DeviceArray

LOSS_KINDS = {'mae': 0, 'mse': 1, 'dssim': 2, 'dssim_mae': 3, 'dssim_mse': 4, 'dssim_mae_mse': 5,
              'msdssim': 6, 'msdssim_mae': 7, 'msdssim_mae_mse': 8}


def _d(a):
    return None if a is None else DeviceArray.from_numpy(np.asarray(a, np.float32))


def _p(d):
    return None if d is None else d.ptr


def conv2d(x, w, b=None, add=None, relu=False, d2s=0):
    """y = [relu](conv_same(x,w)+b+add) [-> depth_to_space(d2s)]"""
    n, h, wd, cin = x.shape
    ks, _, ci, cout = w.shape
    assert ci == cin
    dx, dw, db, da = _d(x), _d(w), _d(b), _d(add)
    if d2s > 1:
        y = DeviceArray.zeros((n, h * d2s, wd * d2s, cout // (d2s * d2s)))
    else:
        y = DeviceArray.zeros((n, h, wd, cout))
    _lib.check(_lib.lib().dl4ds_op_conv2d_fwd(dx.ptr, dw.ptr, _p(db), _p(da), y.ptr, n, h, wd, cin, cout, ks,
                                              int(relu), int(d2s)))
    return y.numpy()


def conv2d_epilogue(x, w, b=None, add=None, mask=None, relu=False, accumulate_into=None):
    """y = [y_old +] where(mask > 0, [relu](conv_same(x,w) + b + add), 0): every operand of the fused epilogue."""
    n, h, wd, cin = x.shape
    ks, _, ci, cout = w.shape
    assert ci == cin
    dx, dw, db, da, dm = _d(x), _d(w), _d(b), _d(add), _d(mask)
    y = DeviceArray.zeros((n, h, wd, cout)) if accumulate_into is None else _d(accumulate_into)
    _lib.check(_lib.lib().dl4ds_op_conv2d_epilogue(dx.ptr, dw.ptr, _p(db), _p(da), _p(dm), y.ptr, n, h, wd, cin, cout, ks,
                                                   int(relu), int(accumulate_into is not None)))
    return y.numpy()


def conv2d_sum_output(x, w, b, s, relu=False):
    """-> (y, s + y, launched) with y = [relu](conv_same(x,w)+b): the Add behind a layer written by the layer's own kernel.
    launched False: the kernel that takes this layer has no such form (nothing was written)."""
    n, h, wd, cin = x.shape
    ks, _, ci, cout = w.shape
    assert ci == cin and s.shape == (n, h, wd, cout)
    dx, dw, db, ds = _d(x), _d(w), _d(b), _d(s)
    y, y2 = DeviceArray.zeros((n, h, wd, cout)), DeviceArray.zeros((n, h, wd, cout))
    ok = ctypes.c_int(0)
    _lib.check(_lib.lib().dl4ds_op_conv2d_second_output(dx.ptr, dw.ptr, _p(db), ds.ptr, y2.ptr, None, None, None, None, y.ptr, n, h, wd,
                                                        cin, cout, ks, int(relu), ctypes.byref(ok)))
    return y.numpy(), y2.numpy(), bool(ok.value)


def conv2d_dual_mask(x, w, mask, mask2):
    """-> (conv * [mask > 0], conv * [mask2 > 0], launched) with conv = conv_same(x,w): the backward of an Add of two ReLU outputs
    written by the dgrad that produces the Add's output gradient."""
    n, h, wd, cin = x.shape
    ks, _, ci, cout = w.shape
    assert ci == cin and mask.shape == mask2.shape == (n, h, wd, cout)
    dx, dw, dm, dm2 = _d(x), _d(w), _d(mask), _d(mask2)
    y, y2, part = (DeviceArray.zeros((n, h, wd, cout)) for _ in range(3))
    ok = ctypes.c_int(0)
    _lib.check(_lib.lib().dl4ds_op_conv2d_second_output(dx.ptr, dw.ptr, None, None, None, dm.ptr, dm2.ptr, y2.ptr, part.ptr, y.ptr, n, h,
                                                        wd, cin, cout, ks, 0, ctypes.byref(ok)))
    return y.numpy(), y2.numpy(), bool(ok.value)


def add_act(a, b, relu=False):
    """[relu](a + b), the stand-alone Add pass."""
    da, db = _d(a), _d(b)
    out = DeviceArray.zeros(a.shape)
    _lib.check(_lib.lib().dl4ds_op_add_act(da.ptr, db.ptr, out.ptr, a.size, int(relu)))
    return out.numpy()


def masked_axpy_pair(dy, ya, yb):
    """-> (dy * [ya > 0], dy * [yb > 0]), the stand-alone backward pass of an Add of two ReLU outputs."""
    ddy, dya, dyb = _d(dy), _d(ya), _d(yb)
    da, db = DeviceArray.zeros(dy.shape), DeviceArray.zeros(dy.shape)
    ok = ctypes.c_int(0)
    _lib.check(_lib.lib().dl4ds_op_masked_axpy_pair(ddy.ptr, dya.ptr, da.ptr, dyb.ptr, db.ptr, dy.size, ctypes.byref(ok)))
    if not ok.value:
        raise ValueError('masked_axpy_pair: size not a multiple of four')
    return da.numpy(), db.numpy()


def conv2d_dgrad(dz, w, d2s=0, accumulate_into=None):
    """dx = dgrad(dz, w).  dz: gradient of the conv output (in d2s layout if d2s>1)."""
    ks, _, cin, cout = w.shape
    if d2s > 1:
        n, h, wd = dz.shape[0], dz.shape[1] // d2s, dz.shape[2] // d2s
    else:
        n, h, wd = dz.shape[:3]
    ddz, dw = _d(dz), _d(w)
    dx = DeviceArray.zeros((n, h, wd, cin)) if accumulate_into is None else _d(accumulate_into)
    _lib.check(_lib.lib().dl4ds_op_conv2d_dgrad(ddz.ptr, dw.ptr, dx.ptr, n, h, wd, cin, cout, ks, int(d2s),
                                                int(accumulate_into is not None)))
    return dx.numpy()


def conv2d_wgrad(x, dz, ks, d2s=0, accumulate_into=None):
    n, h, wd, cin = x.shape
    cout = dz.shape[-1] * (d2s * d2s if d2s > 1 else 1)
    dx, ddz = _d(x), _d(dz)
    dw = DeviceArray.zeros((ks, ks, cin, cout)) if accumulate_into is None else _d(accumulate_into)
    _lib.check(_lib.lib().dl4ds_op_conv2d_wgrad(dx.ptr, ddz.ptr, dw.ptr, n, h, wd, cin, cout, ks, int(d2s),
                                                int(accumulate_into is not None)))
    return dw.numpy()


def bias_act_bwd(dy, y=None, want_db=True):
    n, h, w, c = dy.shape
    ddy, dyy = _d(dy), _d(y)
    db = DeviceArray.zeros((c,)) if want_db else None
    _lib.check(_lib.lib().dl4ds_op_bias_act_bwd(ddy.ptr, _p(dyy), _p(db), n, h, w, c))
    return ddy.numpy(), (db.numpy() if want_db else None)


def conv2d_transpose(x, w, stride, relu=False):
    n, h, wd, cin = x.shape
    ks, _, cout, ci = w.shape
    assert ci == cin
    dx, dw = _d(x), _d(w)
    y = DeviceArray.zeros((n, h * stride, wd * stride, cout))
    _lib.check(_lib.lib().dl4ds_op_conv2d_transpose_fwd(dx.ptr, dw.ptr, y.ptr, n, h, wd, cin, cout, ks, stride, int(relu)))
    return y.numpy()


def conv2d_transpose_dgrad(dz, w, stride, accumulate=None):
    """``accumulate``: an (N, H, W, Cin) array the gradient is added to (accumulate = 1 of the entry point)."""
    ks, _, cout, cin = w.shape
    n, h, wd = dz.shape[0], dz.shape[1] // stride, dz.shape[2] // stride
    ddz, dw = _d(dz), _d(w)
    if accumulate is not None:
        assert accumulate.shape == (n, h, wd, cin)
    dx = DeviceArray.zeros((n, h, wd, cin)) if accumulate is None else _d(accumulate)
    _lib.check(_lib.lib().dl4ds_op_conv2d_transpose_dgrad(ddz.ptr, dw.ptr, dx.ptr, n, h, wd, cin, cout, ks, stride,
                                                          int(accumulate is not None)))
    return dx.numpy()


def conv2d_transpose_wgrad(x, dz, ks, stride, accumulate=None):
    """``accumulate``: a (KS, KS, Cout, Cin) array the gradient is added to (accumulate = 1 of the entry point)."""
    n, h, wd, cin = x.shape
    cout = dz.shape[-1]
    dx, ddz = _d(x), _d(dz)
    if accumulate is not None:
        assert accumulate.shape == (ks, ks, cout, cin)
    dw = DeviceArray.zeros((ks, ks, cout, cin)) if accumulate is None else _d(accumulate)
    _lib.check(_lib.lib().dl4ds_op_conv2d_transpose_wgrad(dx.ptr, ddz.ptr, dw.ptr, n, h, wd, cin, cout, ks, stride,
                                                          int(accumulate is not None)))
    return dw.numpy()


def depth_to_space(x, r):
    n, h, w, c = x.shape
    dx = _d(x)
    y = DeviceArray.zeros((n, h * r, w * r, c // (r * r)))
    _lib.check(_lib.lib().dl4ds_op_depth_to_space(dx.ptr, y.ptr, n, h, w, c, r))
    return y.numpy()


def space_to_depth(y, r):
    n, hh, ww, cp = y.shape
    h, w, c = hh // r, ww // r, cp * r * r
    dy = _d(y)
    x = DeviceArray.zeros((n, h, w, c))
    _lib.check(_lib.lib().dl4ds_op_space_to_depth(dy.ptr, x.ptr, n, h, w, c, r))
    return x.numpy()


def maxpool2(x):
    n, h, w, c = x.shape
    dx = _d(x)
    y = DeviceArray.zeros((n, h // 2, w // 2, c))
    _lib.check(_lib.lib().dl4ds_op_maxpool2_fwd(dx.ptr, y.ptr, n, h, w, c))
    return y.numpy()


def maxpool2_bwd(x, y, dy):
    n, h, w, c = x.shape
    dx_, dy_, ddy = _d(x), _d(y), _d(dy)
    dx = DeviceArray.zeros(x.shape)
    _lib.check(_lib.lib().dl4ds_op_maxpool2_bwd(dx_.ptr, dy_.ptr, ddy.ptr, dx.ptr, n, h, w, c))
    return dx.numpy()


CANARY = -777.25          # fills a gradient buffer that the kernels must leave alone (``want_dw='canary'``)


def _grad_buffers(accumulate_into, shapes):
    """-> (DeviceArrays, accumulate): zeros, or the preloads of ``accumulate_into`` (None entries stay zero)."""
    if accumulate_into is None:
        return [DeviceArray.zeros(s) for s in shapes], 0
    assert len(accumulate_into) == len(shapes)
    return [DeviceArray.zeros(s) if a is None else _d(np.asarray(a, np.float32).reshape(s))
            for a, s in zip(accumulate_into, shapes)], 1


def _np(d):
    return None if d is None else d.numpy()


def dwconv(x, k, bias=None, dy=None, accumulate_into=None, want_dx=True, want_dk=True, want_db=True):
    """DepthwiseConv2D(7, 'same')(x); with ``dy`` also (dx, dk, db).  k: (7,7,C,1) or (7,7,C).
    ``accumulate_into``: an array preloads dx alone (dk, db add to zeros); a tuple (dx0, dk0, db0) preloads all three.
    ``want_dx`` / ``want_db`` False pass a null pointer and return None in that place; ``want_dk`` False passes a null dk (no
    weight-gradient pass at all), ``want_dk='canary'`` a null dk with a db filled with CANARY, which must come back as it went."""
    n, h, w, c = x.shape
    ks = k.shape[0]
    dx_, dk_ = _d(x), _d(np.ascontiguousarray(k, np.float32).reshape(ks, ks, c))
    db_ = None if bias is None else _d(bias)
    y = DeviceArray.zeros(x.shape)
    _lib.check(_lib.lib().dl4ds_op_dwconv_fwd(dx_.ptr, dk_.ptr, None if db_ is None else db_.ptr, y.ptr, n, h, w, c, ks))
    if dy is None:
        return y.numpy()
    ddy = _d(dy)
    if accumulate_into is not None and not isinstance(accumulate_into, (tuple, list)):
        accumulate_into = (accumulate_into, None, None)
    (gx, gk, gb), acc = _grad_buffers(accumulate_into, [x.shape, (ks, ks, c), (c,)])
    if want_dk == 'canary':
        gb = _d(np.full((c,), CANARY, np.float32))
    gx = gx if want_dx else None
    gk = gk if want_dk is True else None
    gb = gb if want_db else None
    _lib.check(_lib.lib().dl4ds_op_dwconv_bwd(dx_.ptr, dk_.ptr, ddy.ptr, _p(gx), _p(gk), _p(gb), n, h, w, c, ks, acc))
    gk_host = None if gk is None else gk.numpy().reshape(k.shape)
    return y.numpy(), _np(gx), gk_host, _np(gb)


def _norm_grads(x, c, accumulate_into, want_dx, want_dw):
    (dx, dgam, dbet), acc = _grad_buffers(accumulate_into, [x.shape, (c,), (c,)])
    if want_dw == 'canary':
        dbet = _d(np.full((c,), CANARY, np.float32))
    return (dx if want_dx else None), (dgam if want_dw is True else None), (dbet if want_dw else None), acc


def layernorm(x, gamma, beta, eps=1e-3, relu=False, dy=None, accumulate_into=None, want_dx=True, want_dw=True):
    """LayerNormalization(axis=-1)(x) [+ ReLU]; with ``dy`` also (dx, dgamma, dbeta).
    ``accumulate_into=(dx0, dgamma0, dbeta0)``: the gradients are added to these (accumulate = 1).  ``want_dx=False`` passes a null
    dx, ``want_dw=False`` null dgamma and dbeta (None is returned in their places); ``want_dw='canary'`` a null dgamma with a dbeta
    filled with CANARY, which must come back as it went."""
    c = x.shape[-1]
    npix = x.size // c
    dx_, dg_, db_ = _d(x), _d(gamma), _d(beta)
    y = DeviceArray.zeros(x.shape)
    _lib.check(_lib.lib().dl4ds_op_layernorm_fwd(dx_.ptr, dg_.ptr, db_.ptr, y.ptr, npix, c, float(eps), int(relu)))
    if dy is None:
        return y.numpy()
    ddy = _d(dy)
    dx, dgam, dbet, acc = _norm_grads(x, c, accumulate_into, want_dx, want_dw)
    _lib.check(_lib.lib().dl4ds_op_layernorm_bwd(dx_.ptr, y.ptr, ddy.ptr, dg_.ptr, _p(dx), _p(dgam), _p(dbet), npix, c,
                                                 float(eps), int(relu), acc))
    return y.numpy(), _np(dx), _np(dgam), _np(dbet)


def batchnorm(x, gamma, beta, moving_mean, moving_var, eps=1e-3, momentum=0.99, training=True, relu=False, dy=None,
              accumulate_into=None, want_dx=True, want_dw=True, return_saved=False):
    """BatchNormalization(axis=-1)(x, training) [+ ReLU] -> (y, new moving_mean, new moving_var[, dx, dgamma, dbeta][, saved]).
    ``accumulate_into``, ``want_dx``, ``want_dw``: as for ``layernorm``.  ``return_saved``: append the (2, C) array of the batch
    mean and 1 / sqrt(var + eps) that the training-mode forward hands to the backward."""
    c = x.shape[-1]
    npix = x.size // c
    dx_, dg_, db_, dmm, dmv = _d(x), _d(gamma), _d(beta), _d(moving_mean), _d(moving_var)
    y, saved = DeviceArray.zeros(x.shape), DeviceArray.zeros((2 * c,))
    _lib.check(_lib.lib().dl4ds_op_batchnorm_fwd(dx_.ptr, dg_.ptr, db_.ptr, dmm.ptr, dmv.ptr, y.ptr, saved.ptr, npix, c,
                                                 float(eps), float(momentum), int(training), int(relu)))
    tail = (saved.numpy().reshape(2, c),) if return_saved else ()
    if dy is None:
        return (y.numpy(), dmm.numpy(), dmv.numpy()) + tail
    ddy = _d(dy)
    dx, dgam, dbet, acc = _norm_grads(x, c, accumulate_into, want_dx, want_dw)
    _lib.check(_lib.lib().dl4ds_op_batchnorm_bwd(dx_.ptr, y.ptr, ddy.ptr, dg_.ptr, saved.ptr, _p(dx), _p(dgam), _p(dbet),
                                                 npix, c, int(relu), acc))
    return (y.numpy(), dmm.numpy(), dmv.numpy(), _np(dx), _np(dgam), _np(dbet)) + tail


def resize_bilinear(x, ho, wo):
    n, h, w, c = x.shape
    dx = _d(x)
    y = DeviceArray.zeros((n, ho, wo, c))
    _lib.check(_lib.lib().dl4ds_op_resize_bilinear_fwd(dx.ptr, y.ptr, n, h, w, c, ho, wo))
    return y.numpy()


def resize_bilinear_bwd(dy, h, w):
    n, ho, wo, c = dy.shape
    ddy = _d(dy)
    dx = DeviceArray.zeros((n, h, w, c))
    _lib.check(_lib.lib().dl4ds_op_resize_bilinear_bwd(ddy.ptr, dx.ptr, n, h, w, c, ho, wo))
    return dx.numpy()


def localconv(x, w, b):
    n, h, wd, c = x.shape
    f = w.shape[-1]
    dx, dw, db = _d(x), _d(w), _d(b)
    y = DeviceArray.zeros((n, h, wd, f))
    _lib.check(_lib.lib().dl4ds_op_localconv_fwd(dx.ptr, dw.ptr, _p(db), y.ptr, n, h, wd, c, f))
    return y.numpy()


def localconv_bwd(x, w, dy):
    n, h, wd, c = x.shape
    f = w.shape[-1]
    dx_, dw_, ddy = _d(x), _d(w), _d(dy)
    dx = DeviceArray.zeros(x.shape)
    dw = DeviceArray.zeros(w.shape)
    db = DeviceArray.zeros((h, wd, f))
    _lib.check(_lib.lib().dl4ds_op_localconv_bwd(dx_.ptr, dw_.ptr, ddy.ptr, dx.ptr, dw.ptr, db.ptr, n, h, wd, c, f))
    return dx.numpy(), dw.numpy(), db.numpy()


def _att_shape(x):
    if x.ndim == 4:
        b, h, w, c = x.shape
        return b, h * w, 1, c
    b, t, h, w, c = x.shape
    return b, t * h, w, c


def channel_attention(x, w1, b1, w2, b2, return_saved=False):
    g, r, p, c = _att_shape(x)
    cr = w1.shape[-1]
    dx = _d(x)
    ws = [_d(np.asarray(v).reshape(-1)) for v in (w1, b1, w2, b2)]
    y = DeviceArray.zeros(x.shape)
    saved = DeviceArray.zeros((g * p * (2 * c + cr),))
    _lib.check(_lib.lib().dl4ds_op_chatt_fwd(dx.ptr, y.ptr, g, r, p, c, cr, ws[0].ptr, ws[1].ptr, ws[2].ptr,
                                             ws[3].ptr, saved.ptr))
    if return_saved:
        return y.numpy(), saved
    return y.numpy()


def channel_attention_bwd(x, dy, w1, b1, w2, b2):
    g, r, p, c = _att_shape(x)
    cr = w1.shape[-1]
    _, saved = channel_attention(x, w1, b1, w2, b2, return_saved=True)
    dx_, ddy = _d(x), _d(dy)
    dw1_, dw2_ = _d(np.asarray(w1).reshape(-1)), _d(np.asarray(w2).reshape(-1))
    dx = DeviceArray.zeros(x.shape)
    g1, gb1, g2, gb2 = (DeviceArray.zeros((c * cr,)), DeviceArray.zeros((cr,)), DeviceArray.zeros((cr * c,)),
                        DeviceArray.zeros((c,)))
    _lib.check(_lib.lib().dl4ds_op_chatt_bwd(dx_.ptr, ddy.ptr, dx.ptr, g, r, p, c, cr, dw1_.ptr, dw2_.ptr, saved.ptr,
                                             g1.ptr, gb1.ptr, g2.ptr, gb2.ptr))
    return dx.numpy(), g1.numpy().reshape(np.shape(w1)), gb1.numpy(), g2.numpy().reshape(np.shape(w2)), gb2.numpy()


def weight_form(shape, batch_shape):
    """(w_batch, w_channels) of a loss-weight array of `shape` for a (N, H, W, C) batch: (H, W), (H, W, 1) and (H, W, C) are one map
    shared by all samples; (M, H, W, 1) and (M, H, W, C) are M maps, M a divisor of N, sample row r using map r // (N // M) -- M = N:
    one map per sample; M = N / nmul: one per sample of a spatio-temporal output of nmul frames.  ValueError for anything else."""
    n, h, w, c = (int(v) for v in batch_shape)
    shape = tuple(int(v) for v in shape)
    if shape == (h, w):
        return 1, 1
    if len(shape) == 3 and shape[:2] == (h, w) and shape[2] in (1, c):
        return 1, shape[2]
    if len(shape) == 4 and shape[1:3] == (h, w) and shape[3] in (1, c) and shape[0] >= 1 and n % shape[0] == 0:
        return shape[0], shape[3]
    raise ValueError(f'loss weights of shape {shape} do not fit a batch of shape {(n, h, w, c)}: expected (H, W), (H, W, 1), '
                     f'(H, W, C) or (M, H, W, 1 | C) with M a divisor of the batch size')


def loss(kind, y_true, y_pred, want_grad=True, weights=None, scale=1.0, accumulate_into=None):
    """Loss value and dloss/dpred.  weights: per-grid-cell weights, float32, finite, >= 0, in one of the forms of `weight_form`
    (semantics: dl4ds_op_loss_weighted in include/dl4ds_hip.h -- entries with weight 0 are excluded by selection, the multi-scale
    kinds are refused).  scale multiplies the loss and its gradient (the trainers' lambda); accumulate_into: an array of y_pred's
    shape that the gradient is ADDED to (dl4ds_op_loss_scaled; unweighted kinds only)."""
    n, h, w, c = y_true.shape
    if weights is not None and kind.startswith('msdssim'):
        raise ValueError(f'loss weights are not available for the multi-scale kind {kind!r}')
    scaled = scale != 1.0 or accumulate_into is not None
    if scaled and (weights is not None or (accumulate_into is not None and not want_grad)):
        raise ValueError('scale / accumulate_into go with the unweighted loss, accumulate_into with want_grad')
    dt, dp = _d(y_true), _d(y_pred)
    g = DeviceArray.zeros(y_pred.shape) if want_grad else None
    lv = DeviceArray.zeros((8,))
    if scaled:
        if accumulate_into is not None:
            if np.shape(accumulate_into) != tuple(y_pred.shape):
                raise ValueError(f'accumulate_into of shape {np.shape(accumulate_into)} for a prediction of shape {tuple(y_pred.shape)}')
            g = _d(np.ascontiguousarray(accumulate_into, np.float32))
        _lib.check(_lib.lib().dl4ds_op_loss_scaled(LOSS_KINDS[kind], dt.ptr, dp.ptr, _p(g), n, h, w, c, float(scale),
                                                   int(accumulate_into is not None), lv.ptr))
    elif weights is None:
        _lib.check(_lib.lib().dl4ds_op_loss(LOSS_KINDS[kind], dt.ptr, dp.ptr, _p(g), n, h, w, c, lv.ptr))
    else:
        wb, wc = weight_form(np.shape(weights), y_true.shape)
        dw = _d(weights)
        _lib.check(_lib.lib().dl4ds_op_loss_weighted(LOSS_KINDS[kind], dt.ptr, dp.ptr, _p(g), n, h, w, c, dw.ptr, wb, wc, lv.ptr))
    return float(lv.numpy()[0]), (g.numpy() if want_grad else None)


def bce(p, label):
    dp = _d(np.asarray(p, np.float32).reshape(-1))
    g = DeviceArray.zeros((dp.shape[0],))
    lv = DeviceArray.zeros((8,))
    _lib.check(_lib.lib().dl4ds_op_bce(dp.ptr, float(label), dp.shape[0], lv.ptr, g.ptr))
    return float(lv.numpy()[0]), g.numpy().reshape(np.shape(p))


def adam(w, g, m, v, t, lr, beta1=0.9, beta2=0.999, eps=1e-7, grad_scale=1.0):
    dw, dg, dm, dv = (_d(np.asarray(a).reshape(-1)) for a in (w, g, m, v))
    _lib.check(_lib.lib().dl4ds_op_adam(dw.ptr, dg.ptr, dm.ptr, dv.ptr, dw.shape[0], int(t), float(lr), float(beta1),
                                        float(beta2), float(eps), float(grad_scale)))
    sh = np.shape(w)
    return dw.numpy().reshape(sh), dm.numpy().reshape(sh), dv.numpy().reshape(sh)


def merge_ranges(ranges):
    """[begin, end) element ranges in any order -> the sorted list with touching and overlapping ranges merged and empty ones
    dropped (what the library makes of a decayed set; csrc/adam_ext.hip: decay_bounds)."""
    out = []
    for b, e in sorted((int(b), int(e)) for b, e in ranges):
        if b < 0 or e < b:
            raise ValueError(f'not a range: [{b}, {e})')
        if b == e:
            continue
        if out and b <= out[-1][1]:
            out[-1][1] = max(out[-1][1], e)
        else:
            out.append([b, e])
    return [(b, e) for b, e in out]


def adam_ext(w, g, m, v, t, lr, beta1=0.9, beta2=0.999, eps=1e-7, grad_scale=1.0, global_clipnorm=None, weight_decay=0.0,
             decay_ranges=(), ema=None, ema_momentum=0.0, skipped=0):
    """dl4ds_op_adam_ext -> (w', m', v', ema' or None, {'grad_norm', 'clip_factor', 'skipped_steps'}); `skipped`: the count the
    statistics words start with."""
    dw, dg, dm, dv = (_d(np.asarray(a).reshape(-1)) for a in (w, g, m, v))
    de = None if ema is None else _d(np.asarray(ema).reshape(-1))
    n = dw.shape[0]
    r = np.asarray(merge_ranges(decay_ranges), np.uint64).reshape(-1, 2)
    if r.size and int(r.max()) > n:
        raise ValueError(f'decay range beyond the {n} elements')
    r = np.ascontiguousarray(r)
    words = np.zeros(3, np.float32)
    words.view(np.uint32)[2] = int(skipped)
    st = DeviceArray.from_numpy(words)
    _lib.check(_lib.lib().dl4ds_op_adam_ext(dw.ptr, dg.ptr, dm.ptr, dv.ptr, _p(de), n, int(t), float(lr), float(beta1), float(beta2),
                                            float(eps), float(grad_scale), float(global_clipnorm or 0.0), float(weight_decay),
                                            r.ctypes.data if len(r) else None, len(r), float(ema_momentum), st.ptr))
    sh = np.shape(w)
    words = st.numpy()
    stats = dict(grad_norm=np.float32(words[0]), clip_factor=np.float32(words[1]), skipped_steps=int(words.view(np.uint32)[2]))
    return (dw.numpy().reshape(sh), dm.numpy().reshape(sh), dv.numpy().reshape(sh), None if de is None else de.numpy().reshape(sh),
            stats)


def arena_swap(a, b):
    """dl4ds_op_arena_swap (the kernel of the engines' swap_ema) -> (a', b') = (b, a)."""
    da, db = _d(np.asarray(a).reshape(-1)), _d(np.asarray(b).reshape(-1))
    assert da.shape == db.shape
    _lib.check(_lib.lib().dl4ds_op_arena_swap(da.ptr, db.ptr, da.shape[0]))
    return da.numpy().reshape(np.shape(a)), db.numpy().reshape(np.shape(b))


# ---- convolutions on the operand forms the graph passes (dl4ds_op_conv2d_views, dl4ds_op_conv2d_wgrad_views) ---------------------
class _ViewDesc(ctypes.Structure):
    _fields_ = [('p', ctypes.c_void_p), ('C', ctypes.c_int), ('ld', ctypes.c_int), ('d2s', ctypes.c_int), ('nstride', ctypes.c_size_t),
                ('sc', ctypes.c_void_p), ('sh', ctypes.c_void_p)]


SLACK = 256          # floats allocated (and uploaded) behind every view buffer, as the graph's slabs leave room behind a tensor


def slack_values(n=SLACK):
    return (np.arange(n, dtype=np.float32) * 0.37 - 41.0).astype(np.float32)


class View:
    """One operand of conv2d_views / conv2d_wgrad_views: ``C`` channels from channel ``coff`` on of the float32 buffer ``buf`` --
    (N, H, W, ld), or (B, T, H, W, ld) with frame ``t`` of every sample; with ``d2s`` = r the buffer holds depth_to_space(r) of the
    logical tensor, (N, H*r, W*r, ld) with C / r^2 of the ld channels.  ``sc`` / ``sh``: (N, C) per-image channel affine."""

    def __init__(self, buf, C=None, coff=0, t=None, d2s=0, sc=None, sh=None):
        self.buf = np.ascontiguousarray(buf, np.float32)
        assert self.buf.ndim == (5 if t is not None else 4)
        r2 = d2s * d2s if d2s > 1 else 1
        self.ld = self.buf.shape[-1]
        self.C = int(C) if C is not None else self.ld * r2
        self.coff, self.t, self.d2s, self.sc, self.sh = int(coff), t, int(d2s), sc, sh
        assert self.coff + self.C // r2 <= self.ld

    def upload(self, keep):
        img = int(np.prod(self.buf.shape[-3:]))
        dev = DeviceArray((self.buf.size + SLACK,))
        dev.upload(self.buf.reshape(-1))
        dev.upload(slack_values(), self.buf.size)
        keep.append(dev)
        d = _ViewDesc()
        d.p = dev.ptr + 4 * ((0 if self.t is None else self.t * img) + self.coff)
        d.C, d.ld, d.d2s = self.C, self.ld, self.d2s
        d.nstride = 0 if self.t is None else self.buf.shape[1] * img
        for name in ('sc', 'sh'):
            a = getattr(self, name)
            if a is not None:
                keep.append(_d(np.asarray(a, np.float32).reshape(-1)))
            setattr(d, name, None if a is None else keep[-1].ptr)
        self._dev = dev
        return d

    def download(self):
        """-> (the whole buffer as the device holds it now, the slack behind it)"""
        flat = self._dev.numpy()
        return flat[:self.buf.size].reshape(self.buf.shape), flat[self.buf.size:]


def _run_views(call, views):
    """Uploads every view's WHOLE buffer, runs ``call(descriptors)``, downloads every buffer again -> {name: (buffer, slack)}; a
    refused call raises Dl4dsHipError carrying the same dict as ``.buffers``."""
    keep = []
    descs = {k: (None if v is None else v.upload(keep)) for k, v in views.items()}
    try:
        _lib.check(call({k: (None if d is None else ctypes.byref(d)) for k, d in descs.items()}))
    except _lib.Dl4dsHipError as e:
        e.buffers = {k: v.download() for k, v in views.items() if v is not None}
        raise
    return {k: v.download() for k, v in views.items() if v is not None}


def conv2d_views(x, w, y, b=None, add=None, mask=None, relu=False, accumulate=False, dgrad=False):
    """y = [y +] where(mask > 0, [relu](conv_same(x, w) + b + add), 0) with every activation operand a ``View``; ``dgrad``: w is the
    forward layer's (KS, KS, y.C, x.C) filter.  -> {'x' | 'y' | 'add' | 'mask': (whole buffer after the call, slack)}."""
    n, h, wd = (y.buf.shape[0],) + tuple(s // max(y.d2s, 1) for s in y.buf.shape[-3:-1])
    ks = w.shape[0]
    assert w.shape[2:] == ((y.C, x.C) if dgrad else (x.C, y.C)), (w.shape, x.C, y.C)
    dw, db = _d(w), _d(b)
    return _run_views(lambda d: _lib.lib().dl4ds_op_conv2d_views(d['x'], dw.ptr, _p(db), d['add'], d['mask'], d['y'], n, h, wd, ks,
                                                                 int(relu), int(accumulate), int(dgrad)),
                      dict(x=x, y=y, add=add, mask=mask))


def conv2d_wgrad_views(x, dz, ks, dw0=None, db0=None, want_db=True):
    """-> (dw, db or None, {'x' | 'dz': (buffer, slack)}).  dw0 / db0: arrays the gradients are ADDED to (accumulate /
    accumulate_db = 1, independently); otherwise the outputs start from CANARY and must be overwritten."""
    n, h, wd = (x.buf.shape[0],) + x.buf.shape[-3:-1]
    cin, cout = x.C, dz.C
    dw = _d(np.full((ks, ks, cin, cout), CANARY, np.float32) if dw0 is None else dw0)
    db = None if not want_db else _d(np.full((cout,), CANARY, np.float32) if db0 is None else db0)
    bufs = _run_views(lambda d: _lib.lib().dl4ds_op_conv2d_wgrad_views(d['x'], d['dz'], dw.ptr, n, h, wd, ks, int(dw0 is not None),
                                                                       _p(db), int(db0 is not None)), dict(x=x, dz=dz))
    return dw.numpy(), _np(db), bufs


def conv2d_wgrad_attention(x, dz, scale, w, dw0=None, db0=None):
    """-> (dw, db, ds, launched) of dl4ds_op_conv2d_wgrad_attention: x the RAW input view, scale (N, Cin), w (KS, KS, Cin, Cout)."""
    n, h, wd = (x.buf.shape[0],) + x.buf.shape[-3:-1]
    ks, _, cin, cout = w.shape
    dw = _d(np.full(w.shape, CANARY, np.float32) if dw0 is None else dw0)
    db = _d(np.full((cout,), CANARY, np.float32) if db0 is None else db0)
    ds = _d(np.full((n, cin), CANARY, np.float32))
    dsc, dwt = _d(np.asarray(scale, np.float32).reshape(-1)), _d(w)
    ok = ctypes.c_int(0)
    _run_views(lambda d: _lib.lib().dl4ds_op_conv2d_wgrad_attention(d['x'], d['dz'], dsc.ptr, dwt.ptr, dw.ptr, n, h, wd, ks,
                                                                    int(dw0 is not None), db.ptr, int(db0 is not None), ds.ptr,
                                                                    ctypes.byref(ok)), dict(x=x, dz=dz))
    return dw.numpy(), db.numpy(), ds.numpy(), bool(ok.value)
