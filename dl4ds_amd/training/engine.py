"""Thin Python handles over the C-ABI trainers (dl4ds_trainer_* / dl4ds_cgan_*): one call = one
optimisation step executed entirely by libdl4ds_hip.so (forward, loss, backward, RCCL gradient
all-reduce, Keras-form Adam)."""
import ctypes
from collections import OrderedDict

import numpy as np

from .. import _lib
from ..ops import LOSS_KINDS, weight_form


def _lr_schedule(learning_rate, lr_decay_after):
    """supervised.py:336-352: a (lr0, lr1) pair becomes PiecewiseConstantDecay([lr_decay_after], [lr0, lr1])."""
    if isinstance(learning_rate, (tuple, list)) and len(learning_rate) > 1:
        return float(learning_rate[0]), float(learning_rate[1]), float(lr_decay_after)
    if isinstance(learning_rate, (tuple, list)):
        learning_rate = learning_rate[0]
    return float(learning_rate), float(learning_rate), 1e30


def _set_loss_weights(engine, setter, model, loss, w):
    """Shared by both engines: hand a weight array (numpy or DeviceArray; None clears) to the library.  (H, W), (H, W, 1) and
    (H, W, C) are one map for every sample; (B, H, W, 1 | C) is one map per sample of the following steps (all frames of a
    spatio-temporal sample use their sample's map)."""
    if w is None:
        _lib.check(setter(engine.h, None, 0, 0, 0, 0, 0))
        engine._loss_weights = None
        return
    if loss.startswith('msdssim'):
        raise ValueError(f'loss weights are not available for the multi-scale kind {loss!r}')
    out = tuple(model.output_shape)
    h, wd, c = out[-3:]
    is_dev = hasattr(w, 'ptr')
    if not is_dev:
        w = np.ascontiguousarray(getattr(w, 'values', w), np.float32)
    shape = tuple(w.shape)
    per_sample = len(shape) == 4
    wb, wc = weight_form(shape, ((shape[0] if per_sample else 1), h, wd, c))
    _lib.check(setter(engine.h, w.ptr if is_dev else w.ctypes.data, wb, h, wd, wc, 0 if is_dev else 1))
    engine._loss_weights = w            # the copy is asynchronous: the source stays alive until it is replaced


def _check_scalar(name, v):
    if isinstance(v, (bool, np.bool_)) or not isinstance(v, (int, float, np.integer, np.floating)):
        raise TypeError(f'`{name}` must be None or a number, got {v!r}')
    return float(v)


def check_optimizer_args(global_clipnorm=None, weight_decay=None, ema_momentum=None):
    """The optimiser extensions of the engines and trainers -> (global_clipnorm, weight_decay, ema_momentum) as floats or None.

    global_clipnorm (Keras ``global_clipnorm``): finite and > 0; weight_decay (Keras ``weight_decay``, decoupled): finite and >= 0;
    ema_momentum (Keras ``use_ema`` + ``ema_momentum``): 0 <= momentum < 1.  None leaves a feature off.  TypeError for anything
    that is not None or a number (a bool is not a number here), ValueError for a number outside its range.  Looks at its arguments
    only (no library, no device)."""
    if global_clipnorm is not None:
        global_clipnorm = _check_scalar('global_clipnorm', global_clipnorm)
        if not (np.isfinite(global_clipnorm) and global_clipnorm > 0):
            raise ValueError(f'`global_clipnorm` must be finite and > 0, got {global_clipnorm}')
    if weight_decay is not None:
        weight_decay = _check_scalar('weight_decay', weight_decay)
        if not (np.isfinite(weight_decay) and weight_decay >= 0):
            raise ValueError(f'`weight_decay` must be finite and >= 0, got {weight_decay}')
    if ema_momentum is not None:
        ema_momentum = _check_scalar('ema_momentum', ema_momentum)
        if not 0.0 <= ema_momentum < 1.0:                     # (a NaN fails both comparisons)
            raise ValueError(f'`ema_momentum` must be in [0, 1), got {ema_momentum}')
    return global_clipnorm, weight_decay, ema_momentum


def cgan_optimizer_pair(name, value):
    """``global_clipnorm`` / ``weight_decay`` of the CGAN engine: None, a number for both optimisers or a (generator,
    discriminator) pair whose entries may be None -- the forms of `cgan_learning_rates`.  -> (generator, discriminator)."""
    if value is None:
        return None, None
    if isinstance(value, (tuple, list)):
        if len(value) == 1:
            return value[0], value[0]
        if len(value) != 2:
            raise ValueError(f'`{name}` must be a number or a (generator, discriminator) pair')
        return value[0], value[1]
    return value, value


def default_decay_filter(name, shape):
    """The decayed set: every parameter with two or more dimensions -- convolution, transposed-convolution, localized-convolution,
    ConvLSTM and dense kernels -- and so no bias, no normalisation gamma / beta and no BatchNormalization moving statistic.  The one
    bias with more than one dimension, the (H, W, F) field of a localized convolution, is left out by its name."""
    return len(tuple(shape)) >= 2 and name.rsplit('/', 1)[-1] != 'bias'


def decayed_parameters(params, decay_filter=None):
    """Names of the parameters weight decay applies to, in parameter order.  params: name -> dict(shape=..., trainable=...) (a
    GraphBuilder's ``params``) or name -> array / shape.  Non-trainable variables are never decayed, whatever the filter says."""
    f = default_decay_filter if decay_filter is None else decay_filter
    out = []
    for name, p in params.items():
        if isinstance(p, dict):
            shape, trainable = p['shape'], p.get('trainable', True)
        else:
            shape, trainable = (tuple(p) if isinstance(p, (tuple, list)) else tuple(np.shape(p))), True
        if trainable and f(name, tuple(shape)):
            out.append(name)
    return out


def _apply_optimizer_ext(setter, model, clip, wd, mu, decay_filter):
    """Hand one optimiser's extensions to the library (setter: the C entry point with the trainer and `which` bound)."""
    names = decayed_parameters(model.graph.params, decay_filter) if wd else []
    ids = (ctypes.c_int * max(len(names), 1))(*[model.graph.params[k]['pid'] for k in names])
    _lib.check(setter(float(clip or 0.0), float(wd or 0.0), ids, len(names), -1.0 if mu is None else float(mu)))
    return names


class _EmaWeights:
    """`with engine.ema_weights():` -- the averages are the model's weights inside the block; the training weights are back after it,
    also when the body raises."""

    def __init__(self, engine):
        self.engine = engine

    def __enter__(self):
        self.engine.swap_ema()
        return self.engine

    def __exit__(self, *exc):
        self.engine.swap_ema()
        return False


class SupervisedEngine:
    """fit() inner step of SupervisedTrainer.run (supervised.py:353,396-406)."""

    def __init__(self, model, loss='mae', learning_rate=1e-3, lr_decay_after=1e5, beta_1=0.9, beta_2=0.999,
                 epsilon=1e-7, global_clipnorm=None, weight_decay=None, ema_momentum=None, decay_filter=None):
        if loss not in LOSS_KINDS:
            raise ValueError(f'loss {loss!r} not available on the MI355X path; one of {sorted(LOSS_KINDS)}')
        ext = check_optimizer_args(global_clipnorm, weight_decay, ema_momentum)
        self.model = model
        self.loss = loss
        self._l = _lib.lib()
        lr0, lr1, boundary = _lr_schedule(learning_rate, lr_decay_after)
        h = ctypes.c_void_p()
        _lib.check(self._l.dl4ds_trainer_create(model.graph.h, LOSS_KINDS[loss], lr0, lr1, boundary, beta_1, beta_2,
                                                epsilon, ctypes.byref(h)))
        self.h = h
        self.global_clipnorm = self.weight_decay = self.ema_momentum = None
        self.decayed = []
        if any(v is not None for v in ext):
            self.set_optimizer_ext(*ext, decay_filter=decay_filter)

    def __del__(self):
        try:
            if getattr(self, 'h', None):
                self._l.dl4ds_trainer_destroy(self.h)
                self.h = None
        except Exception:
            pass

    # --- clipping by the global gradient norm, decoupled weight decay, weight average (csrc/adam_ext.hip)
    def set_optimizer_ext(self, global_clipnorm=None, weight_decay=None, ema_momentum=None, decay_filter=None):
        """Switch the optimiser's extensions (check_optimizer_args; None: off), between steps.  decay_filter: a callable
        (name, shape) -> bool choosing the decayed parameters instead of `default_decay_filter`.  Turning the average on starts it
        as a copy of the current weights; while it stays on, further calls keep it."""
        clip, wd, mu = check_optimizer_args(global_clipnorm, weight_decay, ema_momentum)
        self.decayed = _apply_optimizer_ext(lambda *a: self._l.dl4ds_trainer_set_optimizer_ext(self.h, *a), self.model, clip, wd, mu,
                                            decay_filter)
        self.global_clipnorm, self.weight_decay, self.ema_momentum = clip, wd, mu

    def optimizer_stats(self):
        """{'grad_norm', 'clip_factor', 'skipped_steps'} of the last step (synchronises).  grad_norm is 0 and clip_factor 1 while
        clipping is off; skipped_steps counts the steps left out because the gradient norm was not finite."""
        norm, fac, sk = ctypes.c_float(), ctypes.c_float(), ctypes.c_long()
        _lib.check(self._l.dl4ds_trainer_optimizer_stats(self.h, ctypes.byref(norm), ctypes.byref(fac), ctypes.byref(sk)))
        return {'grad_norm': float(norm.value), 'clip_factor': float(fac.value), 'skipped_steps': int(sk.value)}

    def swap_ema(self):
        """Exchange the model's weights and their averages (one kernel, exact; twice is the identity)."""
        _lib.check(self._l.dl4ds_trainer_ema_swap(self.h))

    def ema_weights(self):
        """Context manager: the averages are the model's weights inside the block."""
        return _EmaWeights(self)

    def _arena_spans(self):
        n_arena, n_params = ctypes.c_size_t(), ctypes.c_int()
        _lib.check(self._l.dl4ds_graph_param_count(self.model.graph.h, ctypes.byref(n_arena), ctypes.byref(n_params)))
        spans = OrderedDict()
        for name, p in self.model.graph.params.items():
            off, n = ctypes.c_size_t(), ctypes.c_size_t()
            _lib.check(self._l.dl4ds_graph_param_info(self.model.graph.h, p['pid'], ctypes.byref(off), ctypes.byref(n)))
            spans[name] = (off.value, n.value, p['shape'])
        return n_arena.value, spans

    def ema_state(self):
        """The averages by variable name (the average must be on)."""
        n, spans = self._arena_spans()
        a = np.empty(n, np.float32)
        _lib.check(self._l.dl4ds_trainer_ema_get(self.h, a.ctypes.data))
        return OrderedDict((k, a[o:o + c].reshape(sh)) for k, (o, c, sh) in spans.items())

    def set_ema_state(self, averages):
        n, spans = self._arena_spans()
        a = np.zeros(n, np.float32)
        for k, (o, c, sh) in spans.items():
            a[o:o + c] = np.asarray(averages[k], np.float32).ravel()
        _lib.check(self._l.dl4ds_trainer_ema_set(self.h, a.ctypes.data))

    def set_loss_weights(self, w):
        """Per-grid-cell weights of the loss (masks, area weights; semantics: dl4ds_op_loss_weighted in include/dl4ds_hip.h), numpy
        or DeviceArray: (H, W), (H, W, 1) or (H, W, C) for one map shared by all samples, (B, H, W, 1 | C) for one map per sample of
        the following steps.  In force for step, loss_and_grads and evaluate (and their _device forms) until replaced; None clears.

        Data parallel: each rank normalises by its own sum of weights, so the average over ranks is the exact global weighted mean
        for a shared map (equal batch sizes) and an approximation for per-sample crops, whose weight sums differ between ranks."""
        _set_loss_weights(self, self._l.dl4ds_trainer_set_loss_weights, self.model, self.loss, w)

    def _host_args(self, inputs, y_true):
        inputs, b = self.model._prep_inputs(inputs)
        y = np.ascontiguousarray(y_true, np.float32)
        if y.shape != (b,) + self.model.output_shape:
            raise ValueError(f'y_true shape {y.shape} != {(b,) + self.model.output_shape}')
        ptrs = (ctypes.c_void_p * len(inputs))(*[a.ctypes.data for a in inputs])
        return inputs, y, ptrs, b

    def step(self, inputs, y_true):
        """One optimisation step on host arrays; returns the batch loss (synchronises)."""
        inputs, y, ptrs, b = self._host_args(inputs, y_true)
        loss = ctypes.c_float()
        _lib.check(self._l.dl4ds_trainer_step(self.h, ptrs, len(inputs), y.ctypes.data, b, 1, ctypes.byref(loss)))
        return float(loss.value)

    def step_device(self, input_ptrs, y_ptr, batch, want_loss=False):
        """One step on HBM-resident buffers (raw device pointers); asynchronous unless want_loss."""
        ptrs = (ctypes.c_void_p * len(input_ptrs))(*input_ptrs)
        loss = ctypes.c_float()
        _lib.check(self._l.dl4ds_trainer_step(self.h, ptrs, len(input_ptrs), y_ptr, int(batch), 0,
                                              ctypes.byref(loss) if want_loss else None))
        return float(loss.value) if want_loss else None

    def loss_and_grads(self, inputs, y_true):
        """Loss and parameter gradients without the Adam update (model.evaluate / test hook)."""
        inputs, y, ptrs, b = self._host_args(inputs, y_true)
        loss = ctypes.c_float()
        _lib.check(self._l.dl4ds_trainer_loss_and_grads(self.h, ptrs, len(inputs), y.ctypes.data, b, 1,
                                                        ctypes.byref(loss)))
        return float(loss.value), self.model.get_gradients()

    def evaluate(self, inputs, y_true):
        """model.evaluate: inference-mode forward + loss (no dropout, BatchNormalization on its moving statistics)."""
        inputs, y, ptrs, b = self._host_args(inputs, y_true)
        loss = ctypes.c_float()
        _lib.check(self._l.dl4ds_trainer_evaluate(self.h, ptrs, len(inputs), y.ctypes.data, b, 1, ctypes.byref(loss)))
        return float(loss.value)

    def evaluate_device(self, input_ptrs, y_ptr, batch):
        """Loss on HBM-resident buffers (no update)."""
        ptrs = (ctypes.c_void_p * len(input_ptrs))(*input_ptrs)
        loss = ctypes.c_float()
        _lib.check(self._l.dl4ds_trainer_evaluate(self.h, ptrs, len(input_ptrs), y_ptr, int(batch), 0,
                                                  ctypes.byref(loss)))
        return float(loss.value)

    def save_checkpoint(self, path):
        """Weights (by variable name) + Adam slots + optimizer.iterations in one .npz -- the native counterpart of the
        reference's tf.train.Checkpoint (cgan.py:288-292) / saved model + trained_epochs (supervised.py:322-325)."""
        m, v, step = self.optimizer_state()
        blob = {'w/' + k: a for k, a in self.model.get_weights().items()}
        blob.update({'m/' + k: a for k, a in m.items()})
        blob.update({'v/' + k: a for k, a in v.items()})
        blob['step'] = np.int64(step)
        if self.ema_momentum is not None:
            blob.update({'ema/' + k: a for k, a in self.ema_state().items()})
        np.savez(path, **blob)

    def load_checkpoint(self, path):
        """Restore a `save_checkpoint` file into this engine (same architecture); returns optimizer.iterations.  With the weight
        average on, the file's ``ema/<name>`` entries are restored; a file without them re-initialises the averages from the
        restored weights."""
        z = np.load(path if str(path).endswith('.npz') else str(path) + '.npz')
        names = list(self.model.get_weights().keys())
        missing = [k for k in names if 'w/' + k not in z]
        if missing:
            raise ValueError(f'checkpoint lacks variables {missing[:3]}...')
        self.model.set_weights({k: z['w/' + k] for k in names})
        n_arena = ctypes.c_size_t()
        n_params = ctypes.c_int()
        _lib.check(self._l.dl4ds_graph_param_count(self.model.graph.h, ctypes.byref(n_arena), ctypes.byref(n_params)))
        m = np.zeros(n_arena.value, np.float32)
        v = np.zeros(n_arena.value, np.float32)
        for name, p in self.model.graph.params.items():
            off, n = ctypes.c_size_t(), ctypes.c_size_t()
            _lib.check(self._l.dl4ds_graph_param_info(self.model.graph.h, p['pid'], ctypes.byref(off), ctypes.byref(n)))
            m[off.value:off.value + n.value] = np.asarray(z['m/' + name], np.float32).ravel()
            v[off.value:off.value + n.value] = np.asarray(z['v/' + name], np.float32).ravel()
        step = int(z['step'])
        _lib.check(self._l.dl4ds_trainer_set_state(self.h, m.ctypes.data, v.ctypes.data, step))
        if self.ema_momentum is not None:
            w = self.model.get_weights()
            self.set_ema_state({k: (z['ema/' + k] if 'ema/' + k in z else w[k]) for k in names})
        return step

    def last_loss(self):
        loss = ctypes.c_float()
        _lib.check(self._l.dl4ds_trainer_last_loss(self.h, ctypes.byref(loss)))
        return float(loss.value)

    def optimizer_state(self):
        n_arena = ctypes.c_size_t()
        n_params = ctypes.c_int()
        _lib.check(self._l.dl4ds_graph_param_count(self.model.graph.h, ctypes.byref(n_arena), ctypes.byref(n_params)))
        m = np.empty(n_arena.value, np.float32)
        v = np.empty(n_arena.value, np.float32)
        step = ctypes.c_long()
        _lib.check(self._l.dl4ds_trainer_get_state(self.h, m.ctypes.data, v.ctypes.data, ctypes.byref(step)))
        out_m, out_v = OrderedDict(), OrderedDict()
        for name, p in self.model.graph.params.items():
            off, n = ctypes.c_size_t(), ctypes.c_size_t()
            _lib.check(self._l.dl4ds_graph_param_info(self.model.graph.h, p['pid'], ctypes.byref(off), ctypes.byref(n)))
            out_m[name] = m[off.value:off.value + n.value].reshape(p['shape'])
            out_v[name] = v[off.value:off.value + n.value].reshape(p['shape'])
        return out_m, out_v, int(step.value)


def cgan_learning_rates(learning_rates):
    """cgan.py:271-278: ``genlr, dislr = learning_rates`` for a pair; a float or a 1-tuple sets both."""
    if isinstance(learning_rates, (tuple, list)) and len(learning_rates) > 1:
        if len(learning_rates) != 2:
            raise ValueError('`learning_rates` must be a float or a (generator, discriminator) pair')
        genlr, dislr = learning_rates
    elif isinstance(learning_rates, (tuple, list)) and len(learning_rates) == 1:
        genlr = dislr = learning_rates[0]
    elif isinstance(learning_rates, (int, float, np.floating)):
        genlr = dislr = learning_rates
    else:
        raise TypeError('`learning_rates` must be a float or a tuple/list of one or two floats')
    return float(genlr), float(dislr)


class CGANEngine:
    """train_step of the CGAN trainer (cgan.py:575-639): one simultaneous generator + discriminator update."""

    def __init__(self, generator, discriminator, loss='mae', learning_rate=2e-4, beta_1=0.5, lambda_scaling_factor=100.0,
                 global_clipnorm=None, weight_decay=None, ema_momentum=None, decay_filter=None):
        if loss not in LOSS_KINDS:
            raise ValueError(f'loss {loss!r} not available on the MI355X path; one of {sorted(LOSS_KINDS)}')
        genlr, dislr = cgan_learning_rates(learning_rate)
        clips, wds = cgan_optimizer_pair('global_clipnorm', global_clipnorm), cgan_optimizer_pair('weight_decay', weight_decay)
        ext = [check_optimizer_args(clips[i], wds[i], ema_momentum if i == 0 else None) for i in (0, 1)]
        self.generator, self.discriminator = generator, discriminator
        self.loss = loss
        self.learning_rates = (genlr, dislr)
        self._l = _lib.lib()
        h = ctypes.c_void_p()
        _lib.check(self._l.dl4ds_cgan_create(generator.graph.h, discriminator.graph.h, LOSS_KINDS[loss],
                                             genlr, float(beta_1), float(lambda_scaling_factor), ctypes.byref(h)))
        self.h = h
        _lib.check(self._l.dl4ds_cgan_set_learning_rates(self.h, genlr, dislr))
        self.global_clipnorm, self.weight_decay, self.ema_momentum = (None, None), (None, None), None
        self.decayed = ([], [])
        if any(v is not None for e in ext for v in e):
            self.set_optimizer_ext((ext[0][0], ext[1][0]), (ext[0][1], ext[1][1]), ext[0][2], decay_filter=decay_filter)

    # --- clipping, decoupled weight decay (a number or a (generator, discriminator) pair each) and the GENERATOR's weight average
    def set_optimizer_ext(self, global_clipnorm=None, weight_decay=None, ema_momentum=None, decay_filter=None):
        clips, wds = cgan_optimizer_pair('global_clipnorm', global_clipnorm), cgan_optimizer_pair('weight_decay', weight_decay)
        ext = [check_optimizer_args(clips[i], wds[i], ema_momentum if i == 0 else None) for i in (0, 1)]
        dec = []
        for i, model in enumerate((self.generator, self.discriminator)):
            dec.append(_apply_optimizer_ext(lambda *a, i=i: self._l.dl4ds_cgan_set_optimizer_ext(self.h, i, *a), model, *ext[i],
                                            decay_filter))
        self.global_clipnorm, self.weight_decay = (ext[0][0], ext[1][0]), (ext[0][1], ext[1][1])
        self.ema_momentum, self.decayed = ext[0][2], tuple(dec)

    def optimizer_stats(self, which='generator'):
        """{'grad_norm', 'clip_factor', 'skipped_steps'} of the generator's or the discriminator's optimiser (synchronises)."""
        if which not in ('generator', 'discriminator'):
            raise ValueError("`which` must be 'generator' or 'discriminator'")
        norm, fac, sk = ctypes.c_float(), ctypes.c_float(), ctypes.c_long()
        _lib.check(self._l.dl4ds_cgan_optimizer_stats(self.h, 0 if which == 'generator' else 1, ctypes.byref(norm), ctypes.byref(fac),
                                                      ctypes.byref(sk)))
        return {'grad_norm': float(norm.value), 'clip_factor': float(fac.value), 'skipped_steps': int(sk.value)}

    def swap_ema(self):
        """Exchange the generator's weights and their averages (one kernel, exact; twice is the identity)."""
        _lib.check(self._l.dl4ds_cgan_ema_swap(self.h))

    def ema_weights(self):
        """Context manager: the averages are the generator's weights inside the block."""
        return _EmaWeights(self)

    def ema_state(self):
        """The generator's averages by variable name (the average must be on)."""
        n, spans = self._arena(self.generator)
        a = np.empty(n, np.float32)
        _lib.check(self._l.dl4ds_cgan_ema_get(self.h, a.ctypes.data))
        return OrderedDict((k, a[o:o + c].reshape(sh)) for k, (o, c, sh) in spans.items())

    def set_ema_state(self, averages):
        n, spans = self._arena(self.generator)
        a = np.zeros(n, np.float32)
        for k, (o, c, sh) in spans.items():
            a[o:o + c] = np.asarray(averages[k], np.float32).ravel()
        _lib.check(self._l.dl4ds_cgan_ema_set(self.h, a.ctypes.data))

    def __del__(self):
        try:
            if getattr(self, 'h', None):
                self._l.dl4ds_trainer_destroy(self.h)
                self.h = None
        except Exception:
            pass

    def set_loss_weights(self, w):
        """Per-grid-cell weights of the generator's PIXEL loss (same forms and semantics as SupervisedEngine.set_loss_weights,
        including the data-parallel note); the adversarial terms are untouched.  None clears."""
        _set_loss_weights(self, self._l.dl4ds_cgan_set_loss_weights, self.generator, self.loss, w)

    def step(self, gen_inputs, hr_array, dropout_keep=None, apply_update=True):
        """Returns (gen_total_loss, gen_gan_loss, gen_px_loss, disc_loss).  dropout_keep: optional (2B, C) keep-mask
        (real rows first) for the discriminator's Dropout(0.4); None -> generated on the device."""
        inputs, b = self.generator._prep_inputs(gen_inputs)
        hr = np.ascontiguousarray(hr_array, np.float32)
        if hr.shape != (b,) + self.generator.output_shape:
            raise ValueError(f'hr_array shape {hr.shape} != {(b,) + self.generator.output_shape}')
        ptrs = (ctypes.c_void_p * len(inputs))(*[a.ctypes.data for a in inputs])
        mask = None
        if dropout_keep is not None:
            mask = np.ascontiguousarray(dropout_keep, np.float32)
        out = (ctypes.c_float * 4)()
        _lib.check(self._l.dl4ds_cgan_step(self.h, ptrs, len(inputs), hr.ctypes.data, b, 1,
                                           None if mask is None else mask.ctypes.data, int(apply_update), out))
        return tuple(float(v) for v in out)

    # --- optimiser state / checkpoints (tf.train.Checkpoint of both optimisers and both models, cgan.py:288-292,370-382)
    def _arena(self, model):
        n_arena, n_params = ctypes.c_size_t(), ctypes.c_int()
        _lib.check(self._l.dl4ds_graph_param_count(model.graph.h, ctypes.byref(n_arena), ctypes.byref(n_params)))
        spans = {}
        for name, p in model.graph.params.items():
            off, n = ctypes.c_size_t(), ctypes.c_size_t()
            _lib.check(self._l.dl4ds_graph_param_info(model.graph.h, p['pid'], ctypes.byref(off), ctypes.byref(n)))
            spans[name] = (off.value, n.value, p['shape'])
        return n_arena.value, spans

    def optimizer_state(self, which):
        """(m, v, iterations) of the generator (``which='generator'``) or discriminator optimiser, by variable name."""
        model = self.generator if which == 'generator' else self.discriminator
        n, spans = self._arena(model)
        m, v, step = np.empty(n, np.float32), np.empty(n, np.float32), ctypes.c_long()
        _lib.check(self._l.dl4ds_cgan_get_state(self.h, 0 if which == 'generator' else 1, m.ctypes.data, v.ctypes.data,
                                                ctypes.byref(step)))
        return (OrderedDict((k, m[o:o + c].reshape(s)) for k, (o, c, s) in spans.items()),
                OrderedDict((k, v[o:o + c].reshape(s)) for k, (o, c, s) in spans.items()), int(step.value))

    def save_checkpoint(self, path):
        blob = {}
        for which, model in (('generator', self.generator), ('discriminator', self.discriminator)):
            m, v, step = self.optimizer_state(which)
            blob.update({f'{which}/w/{k}': a for k, a in model.get_weights().items()})
            blob.update({f'{which}/m/{k}': a for k, a in m.items()})
            blob.update({f'{which}/v/{k}': a for k, a in v.items()})
            blob[f'{which}/step'] = np.int64(step)
        if self.ema_momentum is not None:
            blob.update({'generator/ema/' + k: a for k, a in self.ema_state().items()})
        np.savez(path, **blob)

    def load_checkpoint(self, path):
        """Restore a `save_checkpoint` file (same architectures) -- cgan.py:447-522 `load_checkpoint`."""
        z = np.load(path if str(path).endswith('.npz') else str(path) + '.npz')
        for idx, (which, model) in enumerate((('generator', self.generator), ('discriminator', self.discriminator))):
            names = list(model.get_weights().keys())
            missing = [k for k in names if f'{which}/w/{k}' not in z]
            if missing:
                raise ValueError(f'checkpoint lacks {which} variables {missing[:3]}...')
            model.set_weights({k: z[f'{which}/w/{k}'] for k in names})
            n, spans = self._arena(model)
            m, v = np.zeros(n, np.float32), np.zeros(n, np.float32)
            for k, (o, c, s) in spans.items():
                m[o:o + c] = np.asarray(z[f'{which}/m/{k}'], np.float32).ravel()
                v[o:o + c] = np.asarray(z[f'{which}/v/{k}'], np.float32).ravel()
            _lib.check(self._l.dl4ds_cgan_set_state(self.h, idx, m.ctypes.data, v.ctypes.data, int(z[f'{which}/step'])))
        if self.ema_momentum is not None:
            w = self.generator.get_weights()
            self.set_ema_state({k: (z['generator/ema/' + k] if 'generator/ema/' + k in z else w[k]) for k in w})

    def step_device(self, input_ptrs, hr_ptr, batch, want_losses=False):
        ptrs = (ctypes.c_void_p * len(input_ptrs))(*input_ptrs)
        out = (ctypes.c_float * 4)()
        _lib.check(self._l.dl4ds_cgan_step(self.h, ptrs, len(input_ptrs), hr_ptr, int(batch), 0, None, 1,
                                           out if want_losses else None))
        return tuple(float(v) for v in out) if want_losses else None
