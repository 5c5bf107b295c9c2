"""Python side of the graph runtime: lowers layer calls to the C-ABI graph (dl4ds_graph_*) and wraps
the result in a Keras-like ``Model`` (the surface the reference uses: ``model(inputs, training=)``,
``.predict``, ``.name``, ``.count_params``, ``.get_weights/.set_weights``, ``.summary`` --
dl4ds/training/supervised.py:320,396-409; cgan.py:597-600; inference.py:172-173,238)."""
import ctypes
import math
from collections import OrderedDict
from fractions import Fraction

import numpy as np

from . import _lib
from ._chunks import check_batch_size, is_int
from .device import Buffers, DeviceArray
from .ensemble_score import (NEIGHBOURHOOD_DEFAULT_WINDOWS, ExceedanceScorer, MultivariateScorer, NeighbourhoodScorer, Scorer,
                             check_exceedance_args, check_multivariate_args, check_neighbourhood_ensemble_args, check_score_args)

ACT_KINDS = {'relu': 1, 'sigmoid': 2, 'tanh': 3, 'elu': 4, 'leaky_relu': 5, 'selu': 6, 'gelu': 7}


class Tensor:
    """``px``, ``reach``, ``local_reach`` and ``align`` are the tile-planning quantities GraphBuilder tracks (``_track``), all in pixels of
    the first graph input: the width of one pixel of this tensor, how far one of its values can depend on the inputs (None: on the
    whole field), the same without the ops that look at the whole field, and the lattice tile origins have to lie on."""
    __slots__ = ('id', 'H', 'W', 'C', 'nmul', 'px', 'reach', 'local_reach', 'align', 'stats')

    def __init__(self, id, H, W, C, nmul=1):
        self.id, self.H, self.W, self.C, self.nmul = id, H, W, C, nmul
        self.px, self.reach, self.local_reach, self.align = Fraction(1), Fraction(0), Fraction(0), 1
        self.stats = frozenset()             # the channel-attention ops upstream: (op index, pixel width of its input, 5-D form)

    @property
    def shape(self):
        return (self.nmul, self.H, self.W, self.C)


def _check_activation(act):
    if act is None or act == 'linear':
        return None
    if act not in ACT_KINDS:
        raise ValueError(f'activation {act!r} not supported; one of {sorted(ACT_KINDS)} or None')
    return act


class GraphBuilder:
    """Thin object API over dl4ds_graph_*; owns parameter names, shapes and initialisers."""

    def __init__(self):
        self._l = _lib.lib()
        h = ctypes.c_void_p()
        _lib.check(self._l.dl4ds_graph_create(ctypes.byref(h)))
        self.h = h
        self.params = OrderedDict()          # name -> dict(pid, shape, init)
        self.inputs = []
        self.outputs = []
        self.layers = []                     # (kind, name, out_shape) for summary()
        self.finalized = False
        self._n_chatt = 0                    # channel-attention ops so far (their order in the graph)

    def __del__(self):
        try:
            if getattr(self, 'h', None):
                self._l.dl4ds_graph_destroy(self.h)
                self.h = None
        except Exception:
            pass

    # ---------------------------------------------------------------- tensors / params
    def input(self, H, W, C, nmul=1, requires_grad=False):
        tid = ctypes.c_int()
        _lib.check(self._l.dl4ds_graph_input(self.h, int(H), int(W), int(C), int(nmul), ctypes.byref(tid)))
        if requires_grad:
            _lib.check(self._l.dl4ds_graph_input_requires_grad(self.h, tid.value))
        t = Tensor(tid.value, int(H), int(W), int(C), int(nmul))
        if self.inputs:                      # a later input on a finer (or coarser) grid, e.g. the HR static variables
            t.px = Fraction(self.inputs[0].H, t.H)
        self.inputs.append(t)
        return t

    # ---------------------------------------------------------------- reach and alignment
    RESIZE_SUPPORT = {'nearest': 0, 'bilinear': 1, 'bicubic': 2, 'lanczos3': 3, 'lanczos5': 5, 'gaussian': 2, 'mitchellcubic': 2}

    @staticmethod
    def _track(y, srcs, add=0, px=None, unbounded=False, phase=False):
        """Reach and alignment of the op output ``y`` from those of its operands ``srcs``.  ``add``: what the op adds to the reach, in
        pixels of the first input (the caller scales by the operand's pixel width); ``px``: the output's pixel width where the op
        changes it; ``unbounded``: the output depends on the whole field; ``phase``: the op shrinks the grid by a factor whose
        groups start at pixel 0 (max-pool, a stride, a stepped slice), so tile origins must be multiples of the output's pixel width.
        An op that makes pixels wider also reads the whole footprint of the wider pixel: px_out - px_in is added."""
        y.px = Fraction(srcs[0].px if px is None else px)
        grow = max(y.px - srcs[0].px, 0)
        y.local_reach = max(s.local_reach for s in srcs) + Fraction(add) + grow
        y.reach = None if unbounded or any(s.reach is None for s in srcs) else max(s.reach for s in srcs) + Fraction(add) + grow
        align, stats = 1, frozenset()                          # (y may be one of its own operands: conv2d_folded's second call)
        for s in srcs:
            align, stats = math.lcm(align, s.align), stats | s.stats
        y.align, y.stats = align, stats
        if phase and y.px.denominator == 1:                    # (a group inside one input pixel never straddles a tile origin)
            y.align = math.lcm(y.align, y.px.numerator)
        return y

    def param(self, name, shape, init='glorot', trainable=True):
        shape = tuple(int(s) for s in shape)
        if name in self.params:                 # shared weights (e.g. spc conv2x applied twice)
            p = self.params[name]
            if p['shape'] != shape:
                raise ValueError(f'parameter {name} re-used with shape {shape} != {p["shape"]}')
            return p['pid']
        pid = ctypes.c_int()
        _lib.check(self._l.dl4ds_graph_param(self.h, int(np.prod(shape)), ctypes.byref(pid)))
        self.params[name] = dict(pid=pid.value, shape=shape, init=init, trainable=trainable)
        return pid.value

    def _out(self, tid, kind, name):
        s = (ctypes.c_int * 4)()
        _lib.check(self._l.dl4ds_graph_tensor_shape(self.h, tid, s))
        t = Tensor(tid, s[1], s[2], s[3], s[0])
        self.layers.append((kind, name, t.shape))
        return t

    # ---------------------------------------------------------------- ops
    def conv2d(self, x, name, filters, ks, use_bias=True, activation=None, add=None, d2s=0, dense=False):
        """``dense=True``: a Keras Dense layer applied to the channel axis (ConvNextBlock.pwconv1/2, blocks.py:146,149)
        -- a 1x1 convolution whose kernel variable keeps the Dense shape (Cin, units)."""
        activation = _check_activation(activation)
        w = self.param(name + '/kernel', (x.C, filters) if dense else (ks, ks, x.C, filters))
        b = self.param(name + '/bias', (filters,), 'zeros') if use_bias else -1
        out = ctypes.c_int()
        _lib.check(self._l.dl4ds_graph_conv2d(self.h, x.id, w, b, -1 if add is None else add.id, int(ks),
                                              int(filters), int(activation == 'relu'), int(d2s), ctypes.byref(out)))
        y = self._out(out.value, 'conv2d', name)
        self._track(y, [x] + ([add] if add is not None else []), Fraction(int(ks) - 1, 2) * x.px,
                    x.px / int(d2s) if d2s and d2s > 1 else None)
        if activation not in (None, 'relu'):
            y = self.act(y, activation, name + '/act')
        return y

    def conv2d_folded(self, x, name, filters, ks, d2s, name2, filters2, activation=None, aux=None):
        """Conv2D(ks, d2s^2 * filters) [+ depth_to_space(d2s)] directly followed by Conv2D(1x1, filters2) + activation,
        evaluated with the composed filter (csrc/graph_ops3.hip).  Variables are those of the two Keras layers.
        ``aux``: an HR tensor that the reference concatenates to the first convolution's output before the 1x1 layer
        (Concatenate([x, s]) -> TransitionLast, sp_postups.py:184-203): the 1x1 kernel then has filters + aux.C input
        channels and the auxiliary part is added as a separate 1x1 convolution."""
        activation = _check_activation(activation)
        r2 = d2s * d2s if d2s and d2s > 1 else 1
        w1 = self.param(name + '/kernel', (ks, ks, x.C, r2 * filters))
        b1 = self.param(name + '/bias', (r2 * filters,), 'zeros')
        w2 = self.param(name2 + '/kernel', (1, 1, filters + (aux.C if aux is not None else 0), filters2))
        b2 = self.param(name2 + '/bias', (filters2,), 'zeros')
        out = ctypes.c_int()
        if aux is not None:
            _lib.check(self._l.dl4ds_graph_conv2d_folded_aux(self.h, x.id, aux.id, w1, b1, w2, b2, int(ks), int(filters),
                                                             int(filters2), int(activation == 'relu'), int(d2s or 0),
                                                             ctypes.byref(out)))
        else:
            _lib.check(self._l.dl4ds_graph_conv2d_folded(self.h, x.id, w1, b1, w2, b2, int(ks), int(filters), int(filters2),
                                                         int(activation == 'relu'), int(d2s or 0), ctypes.byref(out)))
        y = self._out(out.value, 'conv2d+conv1x1 (folded)', name + ' -> ' + name2)
        self._track(y, [x], Fraction(int(ks) - 1, 2) * x.px, x.px / int(d2s) if r2 > 1 else None)
        if aux is not None:
            self._track(y, [y, aux])
        if activation not in (None, 'relu'):
            y = self.act(y, activation, name2 + '/act')
        return y

    def dwconv(self, x, name, ks=7, use_bias=True):
        """DepthwiseConv2D(kernel_size=ks, padding='same', depth_multiplier=1) -- blocks.py:143-144."""
        w = self.param(name + '/depthwise_kernel', (ks, ks, x.C, 1))
        b = self.param(name + '/bias', (x.C,), 'zeros') if use_bias else -1
        out = ctypes.c_int()
        _lib.check(self._l.dl4ds_graph_dwconv(self.h, x.id, w, b, int(ks), ctypes.byref(out)))
        return self._track(self._out(out.value, 'depthwise_conv2d', name), [x], Fraction(int(ks) - 1, 2) * x.px)

    def conv2d_transpose(self, x, name, filters, ks, stride, activation=None):
        activation = _check_activation(activation)
        w = self.param(name + '/kernel', (ks, ks, filters, x.C))
        out = ctypes.c_int()
        _lib.check(self._l.dl4ds_graph_conv2d_transpose(self.h, x.id, w, int(ks), int(stride), int(filters),
                                                        int(activation == 'relu'), ctypes.byref(out)))
        y = self._out(out.value, 'conv2d_transpose', name)
        # y[i s + k - pb] += x[i] w[k], pb = (ks - s) // 2: output pixel Y = m s + f reads inputs ceil((f + pb - ks + 1) / s) ..
        # floor((f + pb) / s) around m
        ks_, s_ = int(ks), int(stride)
        pb = max(ks_ - s_, 0) // 2
        taps = max(max((ks_ - 1 - f - pb) // s_ if f + pb - ks_ + 1 < 0 else 0, (f + pb) // s_) for f in range(s_))
        self._track(y, [x], taps * x.px, x.px / s_)
        if activation not in (None, 'relu'):
            y = self.act(y, activation, name + '/act')
        return y

    def channel_attention(self, x, name, nf, r=4, time_window_5d=0):
        cr = int(nf / r)
        if cr < 1:
            raise ValueError(f'ChannelAttention2D needs nf >= r (got nf={nf}, r={r})')
        w1 = self.param(name + '/conv1/kernel', (1, 1, x.C, cr))
        b1 = self.param(name + '/conv1/bias', (cr,), 'zeros')
        w2 = self.param(name + '/conv2/kernel', (1, 1, cr, nf))
        b2 = self.param(name + '/conv2/bias', (nf,), 'zeros')
        out = ctypes.c_int()
        _lib.check(self._l.dl4ds_graph_chatt(self.h, x.id, w1, b1, w2, b2, cr, int(time_window_5d), ctypes.byref(out)))
        # the output depends on the rest of the field through the C channel means only: the reach stays that of the local ops and the op
        # is recorded, so that Model.receptive_halo / predict_tiled can decide whether those means can be supplied
        y = self._track(self._out(out.value, 'channel_attention', name), [x])
        y.stats = y.stats | {(self._n_chatt, x.px, bool(time_window_5d))}
        self._n_chatt += 1
        return y

    def concat(self, xs, name='concat'):
        ids = (ctypes.c_int * len(xs))(*[t.id for t in xs])
        out = ctypes.c_int()
        _lib.check(self._l.dl4ds_graph_concat(self.h, ids, len(xs), ctypes.byref(out)))
        return self._track(self._out(out.value, 'concat', name), list(xs))

    def add(self, a, b, relu=False, name='add'):
        out = ctypes.c_int()
        _lib.check(self._l.dl4ds_graph_add(self.h, a.id, b.id, int(relu), ctypes.byref(out)))
        return self._track(self._out(out.value, 'add', name), [a, b])

    def act(self, x, kind, name='act'):
        kind = _check_activation(kind)
        if kind is None:
            return x
        out = ctypes.c_int()
        _lib.check(self._l.dl4ds_graph_act(self.h, x.id, ACT_KINDS[kind], ctypes.byref(out)))
        return self._track(self._out(out.value, 'activation:' + kind, name), [x])

    def maxpool2(self, x, name='maxpool'):
        out = ctypes.c_int()
        _lib.check(self._l.dl4ds_graph_maxpool2(self.h, x.id, ctypes.byref(out)))
        return self._track(self._out(out.value, 'maxpool2', name), [x], px=2 * x.px, phase=True)

    def resize(self, x, ho, wo, name='resize', interpolation='bilinear'):
        methods = {'bilinear': 0, 'nearest': 1, 'bicubic': 2, 'lanczos3': 3, 'lanczos5': 4, 'gaussian': 5, 'mitchellcubic': 6}
        if interpolation == 'area':
            raise NotImplementedError("Resizing(interpolation='area'): TensorFlow's ResizeArea op has no gradient, the reference "
                                      "cannot train a model built with it either")
        if interpolation not in methods:
            raise ValueError(f'unknown Resizing interpolation {interpolation!r}; one of {sorted(methods)}')
        out = ctypes.c_int()
        _lib.check(self._l.dl4ds_graph_resize_method(self.h, x.id, int(ho), int(wo), methods[interpolation], ctypes.byref(out)))
        y = self._out(out.value, 'resize_' + interpolation, name)
        fy, fx = Fraction(int(ho), x.H), Fraction(int(wo), x.W)
        # an integer enlargement samples every source pixel at the same sub-pixel offsets wherever a tile starts; any other ratio ties
        # the sampling positions to the size of the grid
        whole = fy == fx and fy.denominator == 1
        return self._track(y, [x], self.RESIZE_SUPPORT[interpolation] * x.px, x.px / fy if whole else None, unbounded=not whole)

    def localconv(self, x, name, filters=2, use_bias=True):
        w = self.param(name + '/kernel', (x.H, x.W, x.C, filters))
        b = self.param(name + '/bias', (x.H, x.W, filters), 'zeros') if use_bias else -1
        out = ctypes.c_int()
        _lib.check(self._l.dl4ds_graph_localconv(self.h, x.id, w, b, int(filters), ctypes.byref(out)))
        return self._track(self._out(out.value, 'locally_connected', name), [x], unbounded=True)      # (weights per grid point)

    def rec_tail_supported(self, cx, cs, co):
        yes = ctypes.c_int(0)
        _lib.check(self._l.dl4ds_rec_tail_supported(int(cx), int(cs), int(co), ctypes.byref(yes)))
        return bool(yes.value)

    def rec_tail(self, x, s, T, co, lcb_name='LocalizedConvBlock', tl_name='TransitionLast'):
        """[x, repeat(s, T)] -> LocalizedConvBlock -> Concatenate -> TransitionLast as one op (csrc/graph_ops4.hip); the
        variables carry the names and shapes of the separate layers (creation order as in models/spt_postups.py: rec_tail)."""
        c24 = x.C + s.C
        wt = self.param(lcb_name + '/transition/conv/kernel', (1, 1, c24, 2))
        bt = self.param(lcb_name + '/transition/conv/bias', (2,), 'zeros')
        wl = self.param(lcb_name + '/localconv/kernel', (x.H, x.W, 2, 2))
        bl = self.param(lcb_name + '/localconv/bias', (x.H, x.W, 2), 'zeros')
        w = self.param(tl_name + '/conv/kernel', (1, 1, c24 + 2, co))
        b = self.param(tl_name + '/conv/bias', (co,), 'zeros')
        out = ctypes.c_int()
        _lib.check(self._l.dl4ds_graph_rec_tail(self.h, x.id, s.id, wt, bt, wl, bl, w, b, int(T), int(co), ctypes.byref(out)))
        return self._track(self._out(out.value, 'rec_tail', tl_name), [x, s], unbounded=True)           # (holds a localconv)

    def repeat_time(self, x, T, name='repeat_time'):
        out = ctypes.c_int()
        _lib.check(self._l.dl4ds_graph_repeat_time(self.h, x.id, int(T), ctypes.byref(out)))
        return self._track(self._out(out.value, 'repeat_time', name), [x])

    def convlstm(self, x, name, filters, ks, T, activation=None):
        activation = _check_activation(activation)
        wk = self.param(name + '/kernel', (ks, ks, x.C, 4 * filters))
        wr = self.param(name + '/recurrent_kernel', (ks, ks, filters, 4 * filters), 'orthogonal')
        b = self.param(name + '/bias', (4 * filters,), 'lstm_bias')
        out = ctypes.c_int()
        _lib.check(self._l.dl4ds_graph_convlstm(self.h, x.id, wk, wr, b, int(ks), int(filters), int(T),
                                                int(activation == 'relu'), ctypes.byref(out)))
        y = self._out(out.value, 'convlstm2d', name)
        self._track(y, [x], Fraction(int(ks) - 1, 2) * int(T) * x.px)       # (the recurrent kernel is applied once per time step)
        if activation not in (None, 'relu'):
            y = self.act(y, activation, name + '/act')
        return y

    def gap(self, x, name='gap', over_time=False):
        out = ctypes.c_int()
        fn = self._l.dl4ds_graph_gap3d if over_time else self._l.dl4ds_graph_gap
        _lib.check(fn(self.h, x.id, ctypes.byref(out)))
        return self._track(self._out(out.value, 'global_avg_pool', name), [x], unbounded=True)

    def slice2d(self, x, oy, ox, step, ho, wo, name='slice'):
        out = ctypes.c_int()
        _lib.check(self._l.dl4ds_graph_slice(self.h, x.id, int(oy), int(ox), int(step), int(ho), int(wo), ctypes.byref(out)))
        return self._track(self._out(out.value, 'slice', name), [x], max(abs(int(oy)), abs(int(ox))) * x.px, x.px * int(step),
                           phase=int(step) > 1)

    def pad_bottom_right(self, x, ho, wo, name='zero_padding'):
        out = ctypes.c_int()
        _lib.check(self._l.dl4ds_graph_pad(self.h, x.id, int(ho), int(wo), ctypes.byref(out)))
        return self._track(self._out(out.value, 'zero_padding', name), [x])

    def conv2d_strided(self, x, name, filters, ks, stride, padding='same'):
        """Conv2D(filters, ks, strides=stride, padding=...) as the stride-1 'same' convolution (MFMA path) followed by
        the sub-sampling slice; see csrc/graph_ops3.hip for the index algebra."""
        if padding not in ('same', 'valid'):
            raise ValueError(padding)
        half = ks // 2

        def geom(n):
            if padding == 'same':
                out = -(-n // stride)
                pad = max((out - 1) * stride + ks - n, 0)
                return out, half - pad // 2
            return (n - ks) // stride + 1, half
        (ho, oy), (wo, ox) = geom(x.H), geom(x.W)
        y = self.conv2d(x, name, filters, ks)
        return self.slice2d(y, oy, ox, stride, ho, wo, name + '/stride')

    def dense(self, x, name, units, activation=None):
        activation = _check_activation(activation)
        w = self.param(name + '/kernel', (x.C, units))
        b = self.param(name + '/bias', (units,), 'zeros')
        out = ctypes.c_int()
        _lib.check(self._l.dl4ds_graph_dense(self.h, x.id, w, b, int(units), ACT_KINDS.get(activation, 0),
                                             ctypes.byref(out)))
        return self._track(self._out(out.value, 'dense', name), [x], unbounded=True)

    def dropout(self, x, rate, name='dropout', variant=None, dim=2):
        """get_dropout_layer -- blocks.py:679-706: identity for rate 0; 'vanilla' / 'gaussian' / 'spatial' and their
        'mc*' forms that stay active at inference.  ``dim=3``: SpatialDropout3D (mask shared over the time axis)."""
        if not rate or rate <= 0:
            return x
        kinds = {None: (0, 0), 'vanilla': (0, 0), 'gaussian': (1, 0), 'spatial': (2, 0), 'mcdrop': (0, 1),
                 'mcgaussiandrop': (1, 1), 'mcspatialdrop': (2, 1)}
        if variant not in kinds:
            raise ValueError(f'dropout variant {variant!r} not supported')
        kind, mc = kinds[variant]
        out = ctypes.c_int()
        _lib.check(self._l.dl4ds_graph_dropout_variant(self.h, x.id, float(rate), kind, mc, int(dim), ctypes.byref(out)))
        return self._track(self._out(out.value, 'dropout' if variant is None else variant, name), [x])

    def norm(self, x, name, kind, activation=None, epsilon=1e-3):
        """LayerNormalization() ('ln') / BatchNormalization() ('bn') with Keras variable names; a ReLU that follows is
        fused, any other activation is appended."""
        activation = _check_activation(activation)
        if kind not in ('bn', 'ln'):
            raise ValueError(f'Normalization not supported, got {kind}')
        gamma = self.param(name + '/gamma', (x.C,), 'ones')
        beta = self.param(name + '/beta', (x.C,), 'zeros')
        mm = mv = -1
        if kind == 'bn':
            mm = self.param(name + '/moving_mean', (x.C,), 'zeros', trainable=False)
            mv = self.param(name + '/moving_variance', (x.C,), 'ones', trainable=False)
        out = ctypes.c_int()
        _lib.check(self._l.dl4ds_graph_norm(self.h, x.id, gamma, beta, mm, mv, int(kind == 'bn'), float(epsilon),
                                            int(activation == 'relu'), ctypes.byref(out)))
        y = self._out(out.value, 'batch_norm' if kind == 'bn' else 'layer_norm', name)
        self._track(y, [x])               # (both normalise over the channel axis of one pixel; BatchNormalization predicts with moving statistics)
        if activation not in (None, 'relu'):
            y = self.act(y, activation, name + '/act')
        return y

    def norm_variables(self, name, channels, kind):
        """Variables of a normalisation layer the reference builds and calls but whose output it discards
        (DenseBlock.norm1, blocks.py:263-267): present in the weight list, absent from the graph."""
        self.param(name + '/gamma', (channels,), 'ones')
        self.param(name + '/beta', (channels,), 'zeros')
        if kind == 'bn':
            self.param(name + '/moving_mean', (channels,), 'zeros', trainable=False)
            self.param(name + '/moving_variance', (channels,), 'ones', trainable=False)

    def aux_launches(self):
        """Weight-gradient calls issued on the second stream since the graph was created (0 without DL4DS_AUX_STREAM)."""
        n = ctypes.c_long()
        _lib.check(self._l.dl4ds_graph_aux_launches(self.h, ctypes.byref(n)))
        return n.value

    # ---------------------------------------------------------------- dropout noise (tests / reproducibility)
    def dropout_count(self):
        n = ctypes.c_int()
        _lib.check(self._l.dl4ds_graph_dropout_count(self.h, ctypes.byref(n)))
        return n.value

    def dropout_mask(self, index, batch):
        """Noise the last forward pass of dropout op ``index`` used (flat array, see include/dl4ds_hip.h)."""
        n = ctypes.c_size_t()
        _lib.check(self._l.dl4ds_graph_dropout_mask_size(self.h, int(index), int(batch), ctypes.byref(n)))
        out = np.empty(n.value, np.float32)
        _lib.check(self._l.dl4ds_graph_dropout_get_mask(self.h, int(index), int(batch), out.ctypes.data))
        return out

    def dropout_mc_count(self):
        """Dropout ops that stay active at inference (the MC* variants with rate > 0)."""
        n = ctypes.c_int()
        _lib.check(self._l.dl4ds_graph_dropout_mc_count(self.h, ctypes.byref(n)))
        return n.value

    def reseed_dropout(self, seed):
        """Every dropout op: seed = mix(seed, op index), draw counter = 0 (include/dl4ds_hip.h)."""
        seed = int(seed) & 0xFFFFFFFFFFFFFFFF
        _lib.check(self._l.dl4ds_graph_dropout_reseed(self.h, seed - (1 << 64) if seed >> 63 else seed))

    def set_dropout_mask(self, index, batch, mask):
        n = ctypes.c_size_t()
        _lib.check(self._l.dl4ds_graph_dropout_mask_size(self.h, int(index), int(batch), ctypes.byref(n)))
        mask = np.ascontiguousarray(mask, np.float32).ravel()
        if mask.size != n.value:
            raise ValueError(f'dropout op {index}: mask of {n.value} entries expected, got {mask.size}')
        _lib.check(self._l.dl4ds_graph_dropout_set_mask(self.h, int(index), int(batch), mask.ctypes.data))

    # ---------------------------------------------------------------- finish
    def finalize(self, output, seed=None):
        _lib.check(self._l.dl4ds_graph_output(self.h, output.id))
        self.outputs.append(output)
        _lib.check(self._l.dl4ds_graph_finalize(self.h))
        self.finalized = True
        self.initialize(seed)

    def initialize(self, seed=None):
        """Keras default initialisers: glorot_uniform kernels, zero biases, ConvLSTM2D orthogonal
        recurrent kernel and unit forget bias."""
        rng = np.random.default_rng(seed)
        for name, p in self.params.items():
            shape, init = p['shape'], p['init']
            if init == 'zeros':
                val = np.zeros(shape, np.float32)
            elif init == 'ones':
                val = np.ones(shape, np.float32)
            elif init == 'lstm_bias':
                f = shape[0] // 4
                val = np.zeros(shape, np.float32)
                val[f:2 * f] = 1.0
            elif init == 'orthogonal':
                rows = int(np.prod(shape[:-1]))
                a = rng.standard_normal((max(rows, shape[-1]), min(rows, shape[-1])))
                q, r = np.linalg.qr(a)
                q *= np.sign(np.diag(r))
                if rows < shape[-1]:
                    q = q.T
                val = q[:rows, :shape[-1]].reshape(shape).astype(np.float32)
            else:
                if len(shape) == 4:
                    rf = shape[0] * shape[1]
                    fan_in, fan_out = rf * shape[2], rf * shape[3]
                else:
                    fan_in, fan_out = shape[0], shape[-1]
                lim = np.sqrt(6.0 / (fan_in + fan_out))
                val = rng.uniform(-lim, lim, size=shape).astype(np.float32)
            self.set_param(name, val)

    def set_param(self, name, value):
        p = self.params[name]
        value = np.ascontiguousarray(value, np.float32)
        if value.shape != p['shape']:
            raise ValueError(f'{name}: expected shape {p["shape"]}, got {value.shape}')
        _lib.check(self._l.dl4ds_graph_set_param(self.h, p['pid'], value.ctypes.data))

    def get_param(self, name, grad=False):
        p = self.params[name]
        out = np.empty(p['shape'], np.float32)
        fn = self._l.dl4ds_graph_get_grad if grad else self._l.dl4ds_graph_get_param
        _lib.check(fn(self.h, p['pid'], out.ctypes.data))
        return out


ENSEMBLE_MAX_MEMBERS = 256        # ENS_MAX_MEMBERS / ENS_MAX_QUANTILES of csrc/ops.h
ENSEMBLE_MAX_QUANTILES = 32


def check_ensemble_args(n_members, quantiles, seed=None, batch_size=None):
    """Arguments of ``predict_ensemble`` -> (n_members as int, probabilities as a float32 array).  Raises ValueError for anything
    else; looks at its arguments only (no library, no device)."""
    if not is_int(n_members):
        raise ValueError(f'`n_members` must be an integer, got {n_members!r}')
    if not 1 <= n_members <= ENSEMBLE_MAX_MEMBERS:
        raise ValueError(f'`n_members` must be in [1, {ENSEMBLE_MAX_MEMBERS}], got {n_members}')
    try:
        q = np.asarray(quantiles, np.float64)
    except (TypeError, ValueError):
        raise ValueError(f'`quantiles` must be a sequence of probabilities, got {quantiles!r}') from None
    if q.ndim == 0:
        q = q.reshape(1)
    if q.ndim != 1 or not np.all((q >= 0.0) & (q <= 1.0)):          # (a NaN fails both comparisons)
        raise ValueError(f'`quantiles` must be a flat sequence of probabilities in [0, 1], got {quantiles!r}')
    if q.size > ENSEMBLE_MAX_QUANTILES:
        raise ValueError(f'at most {ENSEMBLE_MAX_QUANTILES} quantiles per call, got {q.size}')
    if seed is not None and not is_int(seed):
        raise ValueError(f'`seed` must be None or an integer, got {seed!r}')
    check_batch_size(batch_size, integers_only=True)
    return int(n_members), q.astype(np.float32)


def _gather_group_type():
    """ctypes mirror of dl4ds_gather_group (include/dl4ds_hip.h)."""
    class TapAxis(ctypes.Structure):
        _fields_ = [('idx', ctypes.c_void_p), ('wt', ctypes.c_void_p), ('k', ctypes.c_int)]

    class Group(ctypes.Structure):
        _fields_ = [('src', ctypes.c_void_p), ('channels', ctypes.c_int), ('frames', ctypes.c_int), ('src_h', ctypes.c_int),
                    ('src_w', ctypes.c_int), ('raw', ctypes.c_int), ('origin_from_crop', ctypes.c_int), ('row_div', ctypes.c_int),
                    ('taps', TapAxis * 2)]
    return Group


class Model:
    """What a dl4ds builder returns (stands in for tf.keras.Model on the hot path)."""

    def __init__(self, gb, name, input_shapes):
        self.graph = gb
        self.name = name
        self.input_shapes = input_shapes      # list of per-sample shapes, Keras style (H,W,C) / (T,H,W,C)
        self.output_shape = self._keras_shape(gb.outputs[0])

    @staticmethod
    def _keras_shape(t):
        return (t.H, t.W, t.C) if t.nmul == 1 else (t.nmul, t.H, t.W, t.C)

    # --- weights
    def count_params(self):
        return int(sum(np.prod(p['shape']) for p in self.graph.params.values()))

    @property
    def weight_names(self):
        return list(self.graph.params.keys())

    def get_weights(self):
        return OrderedDict((k, self.graph.get_param(k)) for k in self.graph.params)

    def set_weights(self, weights):
        if isinstance(weights, dict):
            for k, v in weights.items():
                self.graph.set_param(k, np.asarray(v))
        else:
            for k, v in zip(self.graph.params, weights):
                self.graph.set_param(k, np.asarray(v))

    def get_gradients(self):
        return OrderedDict((k, self.graph.get_param(k, grad=True)) for k in self.graph.params)

    @property
    def variables(self):
        return list(self.get_weights().items())

    @property
    def trainable_variables(self):
        """Everything but the BatchNormalization moving statistics (they live in the same arena; their gradient is
        identically zero, so Adam leaves them to the forward pass that maintains them)."""
        return [(k, v) for k, v in self.get_weights().items() if self.graph.params[k].get('trainable', True)]

    # --- forward
    def _prep_inputs(self, inputs):
        if isinstance(inputs, np.ndarray):
            inputs = [inputs]
        inputs = [np.ascontiguousarray(a, np.float32) for a in inputs]
        if len(inputs) != len(self.graph.inputs):
            raise ValueError(f'model {self.name} expects {len(self.graph.inputs)} inputs, got {len(inputs)}')
        b = inputs[0].shape[0]
        for a, t, ks in zip(inputs, self.graph.inputs, self.input_shapes):
            if tuple(a.shape[1:]) != tuple(ks) or a.shape[0] != b:
                raise ValueError(f'input shape {a.shape} does not match (batch,)+{tuple(ks)}')
        return inputs, b

    def __call__(self, inputs, training=False):
        inputs, b = self._prep_inputs(inputs)
        out = np.empty((b,) + self.output_shape, np.float32)
        ptrs = (ctypes.c_void_p * len(inputs))(*[a.ctypes.data for a in inputs])
        _lib.check(self.graph._l.dl4ds_graph_forward(self.graph.h, ptrs, len(inputs), b, int(training), 1,
                                                     out.ctypes.data))
        return out

    def predict(self, inputs, batch_size=32, verbose=0):
        """model.predict.  The reference builds its generators on ``Input(shape=(None, None, C))`` (sp_postups.py:112-115),
        so a trained model predicts on ANY grid; the graph here is planned for the grid it was built with, so an input of
        another size runs on a sibling graph planned for that size (cached per grid) that receives the current weights."""
        if isinstance(inputs, np.ndarray):
            inputs = [inputs]
        first = np.asarray(inputs[0])
        grid = tuple(first.shape[-3:-1])
        if grid != tuple(self.input_shapes[0][-3:-1]):
            return self.resized(grid).predict(inputs, batch_size=batch_size, verbose=verbose)
        n = first.shape[0]
        inputs = [np.ascontiguousarray(a, np.float32) for a in inputs]
        # one result array, page-locked while the batches land in it: no per-batch allocation, no concatenation, device-to-host copies
        # at the link's rate (a pageable 67 MB batch of 512^2 fields took 18 ms of the 22 ms per batch)
        out = np.empty((n,) + self.output_shape, np.float32)
        lib = self.graph._l
        pinned = n > 0 and out.nbytes >= (1 << 22) and lib.dl4ds_host_register(out.ctypes.data, out.nbytes) == 0
        try:
            for i in range(0, n, batch_size):
                part, b = self._prep_inputs([a[i:i + batch_size] for a in inputs])
                ptrs = (ctypes.c_void_p * len(part))(*[a.ctypes.data for a in part])
                _lib.check(lib.dl4ds_graph_forward(self.graph.h, ptrs, len(part), b, 0, 1, out[i:i + b].ctypes.data))
        finally:
            if pinned:
                lib.dl4ds_host_unregister(out.ctypes.data)
        return out

    # --- tiled prediction
    def _field_mean_op(self):
        """The index of the model's ChannelAttention2D op whose channel means ``predict_tiled`` supplies from a first pass over the
        tiles; None without one; False when the attention ops cannot be served: more than one (each would need a pass of its own
        behind the previous one's), the 5-D form, or one that pools a tensor on another grid than the output's."""
        t = self.graph.outputs[0]
        if not t.stats:
            return None
        if len(t.stats) > 1:
            return False
        (index, px, five_d), = t.stats
        return False if five_d or px != t.px else index

    @property
    def receptive_halo(self):
        """How far, in pixels of the first input (rounded up), an output value can depend on the inputs other than through the
        channel means of ONE ChannelAttention2D layer on the output grid: that is what every builder of ``dl4ds_amd.models`` ends in
        (ConvBlock_att, sp_postups.py:204), and ``predict_tiled`` computes those means over the whole field in a first pass, so they
        cost no halo.  None when the output depends on the whole field in any other way: global pooling, dense and locally connected
        layers, or more than one channel attention (``attention=True``).  Farther than this from every tile edge that is not an edge
        of the domain, a tile's output (given the field's channel means) equals the full grid's."""
        t = self.graph.outputs[0]
        return None if t.reach is None or self._field_mean_op() is False else int(math.ceil(t.reach))

    @property
    def local_halo(self):
        """The same count with every op that looks at the whole field left out: the halo to hand to ``predict_tiled`` when
        ``receptive_halo`` is None and per-tile statistics in those ops are acceptable."""
        return int(math.ceil(self.graph.outputs[0].local_reach))

    @property
    def tile_align(self):
        """Tile origins (and sizes) must be multiples of this many first-input pixels, so that max-pooling and strides group the same
        pixels in a tile as on the full grid."""
        return int(self.graph.outputs[0].align)

    def predict_tiled(self, inputs, tile, halo=None, blend='crop', batch_size=32):
        """``predict`` for grids whose full-grid graph does not fit (or is not wanted) in device memory: the network runs on
        overlapping tiles of ``tile`` pixels (an int or a (rows, columns) pair, in pixels of the first input) and the tile outputs are
        merged on the device (csrc/tiles.hip).  One sibling graph, planned for the tile, is all that is allocated (``resized``).

        ``halo``: how many pixels inside each tile edge are discarded; None takes ``receptive_halo``.  With ``halo >=
        receptive_halo`` every merged value comes from a position where the tile sees all the input it depends on, and the result
        is the full-grid prediction up to the rounding of a different kernel schedule and of the channel means.  A model with one
        ChannelAttention2D on the output grid (every builder's tail) takes TWO passes over the tiles: the first sums the attention's
        input over the cores of the tiles (dl4ds_tile_pool, fp64, fixed order), the second runs with the field's means in place of
        the tile's (dl4ds_graph_chatt_set_mean); that doubles the forward work and is skipped when one tile covers the domain.
        When ``receptive_halo`` is None, ``halo`` MUST be given and the result is an APPROXIMATION: the ops that look at the whole
        field then see one tile.  ``local_halo`` is the natural choice there.  ``blend``: 'crop' (each pixel from one tile), 'linear'
        or 'hann' (a ramp across the overlap of the tiles' cores), see ``dl4ds_amd.tiling``.  ``tile`` must be a multiple of
        ``tile_align``.

        Per chunk of samples the inputs are uploaded once, tile batches of ``batch_size`` are cropped on the device
        (dl4ds_batch_gather), run (dl4ds_graph_forward on device pointers) and merged (dl4ds_tile_merge), and the finished samples
        come back into a page-locked result.  Sums and merge take the tiles in plan order whatever the batch size.  Every input's
        grid must be an integer multiple of the first input's (the HR static variables of a post-upsampling model).

        Out of scope (ValueError): models with ``localcon_layer=True`` (tied to their grid, as in ``resized``) and spatio-temporal
        models (5-D inputs)."""
        from .tiling import BLENDS, plan_tiles, tile_list, _pair
        if isinstance(inputs, np.ndarray):
            inputs = [inputs]
        if len(self.input_shapes[0]) == 4 or np.ndim(inputs[0]) == 5:
            raise ValueError('predict_tiled: spatio-temporal (5-D input) models are out of scope of tiled prediction; use predict')
        rb = getattr(self, '_rebuild', None)
        if rb is not None and rb[1].get('localcon_layer'):
            raise ValueError('predict_tiled: a model with localcon_layer=True is tied to the grid it was built for and is out of '
                             'scope of tiled prediction')
        if blend not in BLENDS:
            raise ValueError(f'unknown blend {blend!r}: use one of {BLENDS}')
        check_batch_size(batch_size, integers_only=True)
        if len(inputs) != len(self.graph.inputs):
            raise ValueError(f'model {self.name} expects {len(self.graph.inputs)} inputs, got {len(inputs)}')
        inputs = [np.ascontiguousarray(a, np.float32) for a in inputs]
        first = inputs[0]
        if first.ndim != 4:
            raise ValueError(f'predict_tiled: inputs must be (N, H, W, C) arrays, got shape {first.shape}')
        n, grid = first.shape[0], (first.shape[1], first.shape[2])
        ratios = []
        for a, ks in zip(inputs, self.input_shapes):
            ry, rx = Fraction(a.shape[1], grid[0]), Fraction(a.shape[2], grid[1])
            if a.ndim != 4 or a.shape[0] != n or a.shape[3] != ks[-1] or ry != rx or ry.denominator != 1 or \
                    ry != Fraction(ks[0], self.input_shapes[0][0]):
                raise ValueError(f'predict_tiled: input of shape {a.shape} does not go with a first input of shape {first.shape} (model '
                                 f'inputs {self.input_shapes}): grids must be the integer multiple of the first input\'s that the '
                                 'model was built with')
            ratios.append(int(ry))
        out_scale = Fraction(self.output_shape[0], self.input_shapes[0][0])
        if out_scale.denominator != 1:
            raise ValueError(f'predict_tiled: the output grid is {out_scale} times the first input\'s; only integer ratios can be tiled')
        out_scale, c_out = int(out_scale), self.output_shape[-1]
        if halo is None:
            halo = self.receptive_halo
            if halo is None:
                raise ValueError(f'predict_tiled: the output of model {self.name} depends on the whole field (receptive_halo is None: '
                                 'global pooling / channel attention / dense layers), so `halo` must be given and the result is an '
                                 f'approximation; the reach of the convolutional part is local_halo = {self.local_halo}')
        if int(halo) != halo or halo < 0:
            raise ValueError(f'`halo` must be a non-negative integer, got {halo!r}')
        plan = plan_tiles(grid, _pair(tile, 'tile'), int(halo), self.tile_align, blend, out_scale)
        th, tw = plan[0].tile, plan[1].tile
        sib = self if (th, tw) == tuple(self.input_shapes[0][:2]) else self.resized((th, tw))
        iy, ix = tile_list(plan)
        nt = len(iy)
        oy, ox = plan[0].origins[iy], plan[1].origins[ix]
        ho, wo = grid[0] * out_scale, grid[1] * out_scale
        out = np.empty((n, ho, wo, c_out), np.float32)
        if n == 0:
            return out
        lib = self.graph._l
        per_sample = 4 * (sum(int(np.prod(a.shape[1:])) for a in inputs) + ho * wo * c_out)
        chunk = int(max(1, min(n, self.TILED_CHUNK_BYTES // per_sample)))
        bmax = int(max(1, min(int(batch_size), chunk * nt)))
        i32 = lambda a: np.ascontiguousarray(a, np.int32)
        Group = _gather_group_type()
        # one channel attention on the output grid: its means over the FIELD come from a first pass (not needed when a tile is the field)
        att = self._field_mean_op()
        att = None if att is False or nt == 1 else att
        if att is not None:
            tid, c_att, plain = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
            _lib.check(lib.dl4ds_graph_chatt_info(sib.graph.h, att, ctypes.byref(tid), ctypes.byref(c_att), ctypes.byref(plain)))
            if not plain.value:
                raise ValueError('predict_tiled: the input of the channel attention is not a plain array in this graph')
            c_att = c_att.value
            crop = plan if blend == 'crop' else plan_tiles(grid, _pair(tile, 'tile'), int(halo), self.tile_align, 'crop', out_scale)
        pinned = out.nbytes >= (1 << 22) and lib.dl4ds_host_register(out.ctypes.data, out.nbytes) == 0
        try:
            with Buffers() as buf:
                dev_in = [buf.alloc((chunk,) + tuple(a.shape[1:])) for a in inputs]
                dev_out = buf.alloc((chunk, ho, wo, c_out))
                tiles_in = [buf.alloc((bmax, th * r, tw * r, a.shape[3])) for a, r in zip(inputs, ratios)]
                tiles_out = buf.alloc((bmax, th * out_scale, tw * out_scale, c_out))
                wy, wx = buf.own(DeviceArray.from_numpy(plan[0].weights)), buf.own(DeviceArray.from_numpy(plan[1].weights))
                if att is not None:
                    cwy, cwx = (buf.own(DeviceArray.from_numpy(p.weights)) for p in crop)
                    sums, dev_mean = buf.alloc((chunk, c_att), np.float64), buf.alloc((chunk, 1, 1, c_att))
                    tile_mean = buf.alloc((bmax, c_att))
                in_ptrs = (ctypes.c_void_p * len(inputs))(*[d.ptr for d in tiles_in])
                groups = (Group * 1)()

                def gather(src_ptr, shape, s_, cy, cx, dst, h, w, b):
                    g = groups[0]
                    g.src, g.channels, g.frames, g.src_h, g.src_w = src_ptr, shape[3], 0, shape[1], shape[2]
                    g.raw, g.origin_from_crop, g.row_div = 1, 0, 0
                    _lib.check(lib.dl4ds_batch_gather(ctypes.addressof(groups), 1, s_.ctypes.data, None if cy is None else cy.ctypes.data,
                                                      None if cx is None else cx.ctypes.data, dst.ptr, h, w, 1, b))

                for i in range(0, n, chunk):
                    m = min(chunk, n - i)
                    for d, a in zip(dev_in, inputs):                               # the only upload of this chunk
                        d.upload(a[i:i + m])
                    _lib.check(lib.dl4ds_memset(dev_out.ptr, 0, m * ho * wo * c_out * 4))
                    # the chunk's tiles, sample by sample in plan order, in batches of bmax
                    smp = np.repeat(np.arange(m), nt)
                    t_iy, t_ix, t_oy, t_ox = (np.tile(v, m) for v in (iy, ix, oy, ox))

                    def run(each):
                        for j in range(0, m * nt, bmax):
                            b = min(bmax, m * nt - j)
                            s_ = i32(smp[j:j + b])
                            for d, a, r, dst in zip(dev_in, inputs, ratios, tiles_in):
                                gather(d.ptr, a.shape, s_, i32(t_oy[j:j + b] * r), i32(t_ox[j:j + b] * r), dst, th * r, tw * r, b)
                            each(j, b, s_)

                    def pool(j, b, s_):
                        _lib.check(lib.dl4ds_graph_forward(sib.graph.h, in_ptrs, len(inputs), b, 0, 0, tiles_out.ptr))
                        p = ctypes.c_void_p()
                        _lib.check(lib.dl4ds_graph_tensor_ptr(sib.graph.h, tid.value, 0, ctypes.byref(p)))
                        ry, rx = i32(t_iy[j:j + b]), i32(t_ix[j:j + b])
                        _lib.check(lib.dl4ds_tile_pool(p, b, th * out_scale, tw * out_scale, c_att, s_.ctypes.data, ry.ctypes.data,
                                                       rx.ctypes.data, cwy.ptr, crop[0].weights.shape[0], cwx.ptr,
                                                       crop[1].weights.shape[0], sums.ptr, m))

                    def merge(j, b, s_):
                        if att is not None:                                        # each tile gets the means of its sample's field
                            gather(dev_mean.ptr, (m, 1, 1, c_att), s_, None, None, tile_mean, 1, 1, b)
                        _lib.check(lib.dl4ds_graph_forward(sib.graph.h, in_ptrs, len(inputs), b, 0, 0, tiles_out.ptr))
                        my, mx = i32(t_oy[j:j + b] * out_scale), i32(t_ox[j:j + b] * out_scale)
                        ry, rx = i32(t_iy[j:j + b]), i32(t_ix[j:j + b])
                        per_tile = th * out_scale * tw * out_scale * c_out
                        for k in range(0, b, self.MERGE_MAX_TILES):                # (the entry takes 256 tiles; the split changes no bit)
                            e = min(b, k + self.MERGE_MAX_TILES)
                            parts = [v[k:e] for v in (my, mx, s_, ry, rx)]         # (contiguous int32 views, alive during the call)
                            _lib.check(lib.dl4ds_tile_merge(tiles_out.ptr + 4 * k * per_tile, e - k, th * out_scale, tw * out_scale,
                                                            c_out, *[v.ctypes.data for v in parts], wy.ptr, plan[0].weights.shape[0],
                                                            wx.ptr, plan[1].weights.shape[0], dev_out.ptr, m, ho, wo))

                    if att is not None:
                        _lib.check(lib.dl4ds_memset(sums.ptr, 0, sums.nbytes))
                        run(pool)
                        total = sums.numpy()[:m]                                   # (m x C doubles: the only thing that comes back early)
                        dev_mean.upload(np.ascontiguousarray((total / float(ho * wo)).astype(np.float32)))
                        _lib.check(lib.dl4ds_graph_chatt_set_mean(sib.graph.h, att, tile_mean.ptr))
                    try:
                        run(merge)
                    finally:
                        if att is not None:                # (the sibling graph is cached: it must pool again; an error here must not
                            lib.dl4ds_graph_chatt_set_mean(sib.graph.h, att, None)   # hide the one that is already on its way)
                    dev_out.download(out[i:i + m])
        finally:
            if pinned:
                lib.dl4ds_host_unregister(out.ctypes.data)
        return out

    MERGE_MAX_TILES = 256                  # tiles per dl4ds_tile_merge call (include/dl4ds_hip.h)
    TILED_CHUNK_BYTES = 1 << 30            # device-resident inputs + output of one chunk of samples (predict_tiled)

    # --- MC-dropout ensembles (the MC* dropout variants of blocks.py:658-676 stay active at inference)
    def reseed_dropout(self, seed):
        """Seed the dropout noise of this model's graph: the masks of the forward passes that follow (at a fixed batch size)
        are a function of ``seed`` alone.  Dropout op i draws from splitmix64(seed + golden * (i + 1)), so the ops' streams (and those
        of neighbouring seeds) are unrelated; the scheme is spelled out in include/dl4ds_hip.h.  A model that is never reseeded
        draws as if it had been reseeded with the library's built-in seed: its ops get hashed seeds in the same way."""
        self.graph.reseed_dropout(seed)

    def predict_ensemble(self, inputs, n_members, batch_size=32, quantiles=(), seed=None, return_members=False):
        """``n_members`` stochastic forward passes per sample, reduced on the device (csrc/ensemble.hip): a dict with 'mean',
        'std' (population), 'min', 'max' of shape (N,) + output_shape, 'quantiles' of shape (len(quantiles), N) + output_shape
        (np.quantile's default 'linear' method; at most 32 probabilities, taken in float32) and, with ``return_members``,
        'members' (n_members, N) + output_shape.  All float32.

        Per batch the inputs are uploaded once, the members are written into one device stack and only the statistics come
        back.  The result is a function of (weights, inputs, n_members, batch_size, seed): the masks depend on how the samples
        are split into batches, so a stack that does not fit raises MemoryError instead of being re-chunked.  ``seed=None``:
        the graph's noise counters simply continue."""
        n_members, q = check_ensemble_args(n_members, quantiles, seed, batch_size)
        return self._run_ensemble(inputs, n_members, q, batch_size, seed, return_members)

    def score_ensemble(self, inputs, y_true, n_members, batch_size=32, quantiles=(), seed=None, fair=False, scale=None,
                       return_fields=False):
        """``predict_ensemble`` plus the verification of the ensemble against the observation ``y_true`` of shape
        (N,) + output_shape, scored on the device while each batch's member stack is resident (csrc/ensemble_score.hip, DESIGN.md
        section 13).  Returns ``predict_ensemble``'s dict with one more key, 'scores': a dict with the scalars 'crps', 'spread'
        (sqrt of the mean ensemble variance, ddof 1), 'rmse' (of the ensemble mean), 'spread_skill' (spread / rmse) over all valid
        elements; 'crps_per_sample', 'spread_per_sample', 'rmse_per_sample' (N,); 'crps_map', 'spread_map', 'rmse_map' shaped like
        one sample (NaN where no sample was valid); 'rank_histogram' int64 (n_members + 1,); 'covered' int64 and 'coverage'
        (= covered / n_valid) per quantile: how often the observation is <= that quantile; 'n_valid' (with '_per_sample' and
        '_map'), the raw float64 sums 'sample_sums' (N, 4) and 'cell_sums' (4,) + output_shape (crps, squared error, variance,
        count), 'n_cells_excluded'; and with ``return_fields`` the per-element 'crps_field', 'sqerr_field', 'var_field'
        (float32, NaN where invalid) and 'rank_field' (int32, -1 where invalid).

        An element is valid iff its observation and all its members are finite: write NaN into ``y_true`` to mask.  ``fair``: the
        fair CRPS (pair term over K (K - 1) instead of K^2).  ``scale``: a positive factor per cell (broadcast to one sample)
        that carries CRPS, spread and RMSE into physical units; cells where it is not finite and > 0 are excluded and counted in
        'n_cells_excluded'.  Ties between the observation and members are broken by a hash of (seed, element index), 0 for
        ``seed=None``: the ranks do not depend on ``batch_size`` (the members do, as in ``predict_ensemble``).  Scores are per
        element and "sample" is the leading axis, whatever the output's rank; the stack is read twice (statistics, then scores)."""
        n_members, q = check_ensemble_args(n_members, quantiles, seed, batch_size)
        check_score_args(fair)

        def prepare(shape):
            scale32 = check_score_args(fair, scale, shape)
            return lambda n, bmax: Scorer(n_members, n, shape, q, fair, seed, scale32, return_fields, bmax)
        return self._run_ensemble(inputs, n_members, q, batch_size, seed, False, ('scores', y_true, prepare), 'score_ensemble')

    def score_exceedance(self, inputs, y_true, n_members, thresholds, batch_size=32, seed=None, return_fields=False):
        """``predict_ensemble`` plus the verification of the ensemble as a probability forecast of the events ``value >=
        threshold`` against the observation ``y_true`` of shape (N,) + output_shape, counted on the device while each batch's
        member stack is resident (csrc/exceedance.hip).  Returns ``predict_ensemble``'s dict with one more
        key, 'exceedance': the dict ``metrics.exceedance_scores`` describes (contingency table of the forecast count c against the
        observed event, Brier score and its decomposition, reliability diagram, ROC curve and area, Brier maps and per-sample
        scores, all from exact integer sums).  ``thresholds``: up to 16 finite numbers, or one field per threshold shaped
        (T,) + output_shape (NaN excludes the cell for that threshold), in the units of the model's output.  An element is valid
        iff its observation and all its members are finite: write NaN into ``y_true`` to mask.  The counts do not depend on how
        the scored samples are grouped (the members do depend on ``batch_size``, as in ``predict_ensemble``).  Inputs on another
        grid than the model was built for run on the re-planned sibling (``resized``); threshold fields then have ITS output's
        shape."""
        n_members, q = check_ensemble_args(n_members, (), seed, batch_size)
        # (fields are checked against the output's shape in _run_ensemble, once the model is the one planned for the inputs' grid)
        check_exceedance_args(thresholds, None)

        def prepare(shape):
            thr = check_exceedance_args(thresholds, shape)
            return lambda n, bmax: ExceedanceScorer(n_members, n, shape, thr, return_fields, bmax)
        return self._run_ensemble(inputs, n_members, q, batch_size, seed, False, ('exceedance', y_true, prepare), 'score_exceedance')

    def score_multivariate(self, inputs, y_true, n_members, batch_size=32, seed=None, max_lag=4, order=0.5, lag_weights='inverse',
                           fair=False, weights=None):
        """``predict_ensemble`` plus the verification of the ensemble as a forecast of a FIELD against the observation ``y_true``
        of shape (N,) + output_shape: the energy score and the variogram score, reduced on the device while each batch's member
        stack is resident (csrc/ensemble_multi.hip).  Returns ``predict_ensemble``'s dict with one more key,
        'multivariate': the dict ``metrics.multivariate_scores`` describes.  2 <= ``n_members`` <= 128.  An element is valid iff
        its observation and all its members are finite (write NaN into ``y_true`` to mask) and its weight is > 0.  ``weights``:
        finite numbers >= 0 that broadcast to one sample of the output (``losses.latitude_weights``); on another grid than the
        model was built for that is the output of the re-planned sibling (``resized``).  The sums of a sample do not depend on
        how the scored samples are grouped (the members do depend on ``batch_size``, as in ``predict_ensemble``)."""
        n_members, q = check_ensemble_args(n_members, (), seed, batch_size)
        # (weights are checked against the output's shape in _run_ensemble, once the model is the one planned for the inputs' grid)
        check_multivariate_args(max_lag, order, lag_weights, fair, weights, None, n_members)

        def prepare(shape):
            lag, code, w32 = check_multivariate_args(max_lag, order, lag_weights, fair, weights, shape, n_members)
            return lambda n, bmax: MultivariateScorer(n_members, n, shape, lag, order, code, lag_weights, fair, w32, bmax)
        return self._run_ensemble(inputs, n_members, q, batch_size, seed, False, ('multivariate', y_true, prepare),
                                  'score_multivariate')

    def score_neighbourhood(self, inputs, y_true, n_members, thresholds, windows=NEIGHBOURHOOD_DEFAULT_WINDOWS, batch_size=32,
                            seed=None):
        """``predict_ensemble`` plus the neighbourhood verification of the ensemble as a probability forecast of the events
        ``value >= threshold`` against the observation ``y_true`` of shape (N,) + output_shape, reduced on the device while each
        batch's member stack is resident (csrc/ensemble_fss.hip).  Returns ``predict_ensemble``'s dict with
        one more key, 'neighbourhood': the dict ``metrics.neighbourhood_ensemble_scores`` describes (the Fractions Skill Score of
        the neighbourhood ensemble probability and the neighbourhood Brier score per threshold and window size, all from exact
        integer sums).  ``thresholds``: up to 16 finite, strictly increasing numbers in the units of the model's output;
        ``windows``: strictly increasing sizes >= 1.  A cell is valid iff its observation and all its members are finite: write
        NaN into ``y_true`` to mask.  The output must be shaped (H, W, C): a recurrent model's is refused.  The sums do not depend
        on how the scored samples are grouped (the members do depend on ``batch_size``, as in ``predict_ensemble``)."""
        n_members, q = check_ensemble_args(n_members, (), seed, batch_size)
        # (the sample's shape and the overflow rule are checked in _run_ensemble, once the model is the one planned for the grid)
        check_neighbourhood_ensemble_args(None, n_members, thresholds, windows)

        def prepare(shape):
            thr, win = check_neighbourhood_ensemble_args(shape, n_members, thresholds, windows)
            return lambda n, bmax: NeighbourhoodScorer(n_members, n, shape, thr, win, bmax)
        return self._run_ensemble(inputs, n_members, q, batch_size, seed, False, ('neighbourhood', y_true, prepare),
                                  'score_neighbourhood')

    def _run_ensemble(self, inputs, n_members, q, batch_size, seed, return_members, verify=None, who='predict_ensemble'):
        """The per-batch loop of ``predict_ensemble`` / ``score_ensemble`` / ``score_exceedance``: inputs (and the observation)
        uploaded once per batch, the members written into one device stack, reduced (and scored) there.  ``verify``: (the result's
        key, the observation, prepare), where prepare(output_shape) checks the arguments that need the output's shape and returns
        what builds the scorer (ensemble_score.py) for n samples in batches of bmax: prepare(output_shape)(n, bmax)."""
        if isinstance(inputs, np.ndarray):
            inputs = [inputs]
        first = np.asarray(inputs[0])
        grid = tuple(first.shape[-3:-1])
        if grid != tuple(self.input_shapes[0][-3:-1]):
            return self.resized(grid)._run_ensemble(inputs, n_members, q, batch_size, seed, return_members, verify, who)
        inputs = [np.ascontiguousarray(a, np.float32) for a in inputs]
        n, K, nq = first.shape[0], n_members, len(q)
        if verify is not None:
            result_key, y_true, prepare = verify
            y_true = np.ascontiguousarray(y_true, np.float32)
            if y_true.shape != (n,) + self.output_shape:
                raise ValueError(f'`y_true` must have the shape of the prediction {(n,) + self.output_shape}, got {y_true.shape}')
            make_scorer = prepare(self.output_shape)
        if self.graph.dropout_mc_count() == 0:
            import warnings
            warnings.warn(f'model {self.name} has no MC dropout layer: the {K} ensemble members are identical (build it with '
                          "dropout_variant 'mcdrop', 'mcgaussiandrop' or 'mcspatialdrop' and a dropout_rate > 0)", UserWarning,
                          stacklevel=2)
        if seed is not None:
            self.reseed_dropout(seed)
        lib = self.graph._l
        per = int(np.prod(self.output_shape))
        bmax = max(min(int(batch_size), n), 1)
        stride = bmax * per                                    # member stride of the stack, in elements
        with Buffers() as buf:
            try:
                stack = buf.alloc((K, stride))
            except _lib.Dl4dsHipError as e:
                raise MemoryError(f'{who}: the member stack of {K} x {bmax} outputs ({K * stride * 4 / 2**30:.2f} GiB) does '
                                  f'not fit on the device; lower batch_size ({e})') from None
            stats = buf.alloc((4 + nq, stride))
            dev_in = [buf.alloc((bmax,) + tuple(a.shape[1:])) for a in inputs]
            in_ptrs = (ctypes.c_void_p * len(dev_in))(*[d.ptr for d in dev_in])
            qc = (ctypes.c_float * max(nq, 1))(*q.tolist())
            res = {k: np.empty((n,) + self.output_shape, np.float32) for k in ('mean', 'std', 'min', 'max')}
            res['quantiles'] = np.empty((nq, n) + self.output_shape, np.float32)
            if return_members:
                res['members'] = np.empty((K, n) + self.output_shape, np.float32)
            pinned = [a for a in res.values() if a.nbytes >= (1 << 22) and lib.dl4ds_host_register(a.ctypes.data, a.nbytes) == 0]
            scorer = None
            try:
                if verify is not None:                 # (inside the try: a refusal here still unpins the result arrays)
                    dev_obs, scorer = buf.alloc((stride,)), buf.own(make_scorer(n, bmax))
                for i in range(0, n, bmax):
                    part, b = self._prep_inputs([a[i:i + bmax] for a in inputs])
                    m = b * per
                    for d, a in zip(dev_in, part):                             # the only upload of this batch
                        d.upload(a)
                    for k in range(K):
                        _lib.check(lib.dl4ds_graph_forward(self.graph.h, in_ptrs, len(part), b, 0, 0, stack.ptr + k * stride * 4))
                    sp = [stats.ptr + r * stride * 4 for r in range(5)]
                    _lib.check(lib.dl4ds_ensemble_reduce(stack.ptr, K, m, stride, qc, nq, sp[0], sp[1], sp[2], sp[3],
                                                         sp[4] if nq else None))
                    for r, key in enumerate(('mean', 'std', 'min', 'max')):
                        stats.download(res[key][i:i + b], r * stride)
                    for j in range(nq):                                        # quant[j] lies at j * m for this batch's m
                        stats.download(res['quantiles'][j, i:i + b], 4 * stride + j * m)
                    if scorer is not None:                                     # the stack is still resident: second read
                        dev_obs.upload(y_true[i:i + b])
                        scorer.score(stack.ptr, stride, dev_obs.ptr, i, b)
                    if return_members:
                        for k in range(K):
                            stack.download(res['members'][k, i:i + b], k * stride)
                if scorer is not None:
                    res[result_key] = scorer.result()
            finally:
                for a in pinned:
                    lib.dl4ds_host_unregister(a.ctypes.data)
        return res

    def resized(self, grid):
        """The same architecture planned for inputs of spatial size ``grid`` (size of the FIRST input: the LR grid of a
        post-upsampling model, the HR grid of a 'pin' model), carrying this model's current weights."""
        rb = getattr(self, '_rebuild', None)
        if rb is None:
            raise ValueError(f'model {self.name} was not built by a dl4ds_amd.models builder: cannot re-plan it for grid {grid}')
        fn, kwargs, size_key = rb
        if kwargs.get('localcon_layer'):
            # LocallyConnected2D weights are per grid point: the reference fixes the Input shape too (sp_postups.py:106-115)
            raise ValueError('a model with localcon_layer=True is tied to the grid it was built for')
        cache = self.__dict__.setdefault('_resized_cache', OrderedDict())
        grid = (int(grid[0]), int(grid[1]))
        m = cache.get(grid)
        if m is None:
            m = fn(**dict(kwargs, **{size_key: grid}))
            cache[grid] = m
            while len(cache) > self.RESIZED_CACHE_GRIDS:       # least recently used grid goes (its graph frees its HBM)
                cache.popitem(last=False)
        else:
            cache.move_to_end(grid)
        self._copy_weights_to(m)
        return m

    RESIZED_CACHE_GRIDS = 4

    def _arena(self):
        w, g = ctypes.c_void_p(), ctypes.c_void_p()
        _lib.check(self.graph._l.dl4ds_graph_arena_ptrs(self.graph.h, ctypes.byref(w), ctypes.byref(g)))
        n, k = ctypes.c_size_t(), ctypes.c_int()
        _lib.check(self.graph._l.dl4ds_graph_param_count(self.graph.h, ctypes.byref(n), ctypes.byref(k)))
        return w, n.value

    def _copy_weights_to(self, other):
        """Current weights -> a sibling graph of the same architecture: the parameter arenas have the same layout (no
        parameter of a resizable model depends on the grid), so ONE device-to-device copy replaces the per-variable
        download + upload (13.6 M parameters for the U-Net)."""
        (src, n), (dst, m) = self._arena(), other._arena()
        same = n == m and [(k, p['shape']) for k, p in self.graph.params.items()] == \
            [(k, p['shape']) for k, p in other.graph.params.items()]
        if same and n:
            _lib.check(self.graph._l.dl4ds_memcpy_d2d(dst, src, n * 4))
            _lib.check(self.graph._l.dl4ds_sync())
        else:
            other.set_weights(self.get_weights())

    def summary(self, line_length=100, print_fn=print):
        print_fn(f'Model: "{self.name}"')
        print_fn('_' * line_length)
        for kind, name, shape in self.graph.layers:
            print_fn(f'{name[:50]:52s}{kind:24s}{str(shape)}')
        print_fn('=' * line_length)
        print_fn(f'Total params: {self.count_params():,}')


def resizable(size_key):
    """Decorator of the model builders: remembers the call so that ``Model.predict`` can re-plan the graph for another
    grid (``size_key``: the builder argument that holds the grid of the first input, 'lr_size' or 'hr_size')."""
    import functools
    import inspect

    def deco(fn):
        sig = inspect.signature(fn)

        @functools.wraps(fn)
        def wrapper(*args, **kw):
            model = fn(*args, **kw)
            bound = sig.bind(*args, **kw)
            bound.apply_defaults()
            model._rebuild = (wrapper, dict(bound.arguments), size_key)
            return model
        return wrapper
    return deco
