"""float64 numpy restatement of the extended optimiser step (csrc/adam_ext.hip): clipping by the global
gradient norm, decoupled weight decay and the weight average around Keras Adam.  Not a test module; needs no GPU.

The constants are the float32 values the kernel receives (tests/step_kernels_cases.py: adam_consts) and every output comes with an
error bound built like adam_moments_ref / adam_w_ref there, which this module calls:

  scale   the kernel multiplies the gradient by ONE float32 factor fl32(grad_scale * c), so the moments are adam_moments_ref with that
          factor in the place of grad_scale -- same bound, 2^-22 (|b1 m| + |(1 - b1) gr|) and 2^-22 (|b2 v| + |(1 - b2) gr^2|);
  decay   w_d = w - lw w with lw = fl32(lr * weight_decay) where the element is decayed: its own 2^-22 (|w| + |lw w|);
  w       adam_w_ref from w_d and the moments the device returned: 2^-22 (|w_d| + |step|), plus the decay term's bound, which
          passes into w' one to one;
  ema     mu ema + (1 - mu) w' from the w' the device returned: its own 2^-22 (|mu ema| + |(1 - mu) w'|)."""
import numpy as np

from tests.step_kernels_cases import ADAM_BOUND, ADAM_LR, F32, F64, adam_consts, adam_moments_ref, adam_w_ref


def global_norm64(g, gs):
    """grad_scale * ||g||_2 in float64 (grad_scale as the float32 the kernel receives)."""
    g = np.asarray(g, F64).reshape(-1)
    return F64(F32(gs)) * np.sqrt(np.sum(g * g))


def clip_factor32(norm, clip):
    """fl32(clip / max(norm, clip)) of a float32 norm: tf.clip_by_global_norm's factor, 1 exactly when norm <= clip."""
    norm, clip = F32(norm), F32(clip)
    return F32(clip / max(norm, clip))


def grad_factor32(gs, c):
    """The one float32 factor the gradient is multiplied by."""
    return F32(F32(gs) * F32(c))


def decay_mask(n, ranges):
    mask = np.zeros(n, bool)
    for b, e in ranges:
        mask[b:e] = True
    return mask


def decay_ref(w, weight_decay, mask, lr=ADAM_LR):
    """-> (w_d, bound): w - fl32(lr * weight_decay) w inside the mask, w (bound 0) outside."""
    w = np.asarray(w, F64)
    lw = F64(F32(F32(lr) * F32(weight_decay)))
    term = np.where(mask, lw * w, 0.0)
    return w - term, np.where(mask, ADAM_BOUND * (np.abs(w) + np.abs(term)), 0.0)


def ema_ref(ema, w1, mu):
    """-> (ema', bound) from the new weights: mu ema + (1 - mu) w' with 1 - mu formed in float32."""
    a = F64(F32(mu)) * np.asarray(ema, F64)
    b = F64(F32(1) - F32(mu)) * np.asarray(w1, F64)
    return a + b, ADAM_BOUND * (np.abs(a) + np.abs(b))


def step_ref(w, g, m, v, ema, t, gs, c, weight_decay, mask, mu, m1=None, v1=None, w1=None, lr=ADAM_LR):
    """One extended step in float64 -> {'m': (value, bound), 'v': ..., 'w': ..., 'ema': ... (if ema is not None)}.

    c: the clip factor (1 without clipping), float32 as the device reported it.  mask: the decayed elements (None: none).
    m1, v1, w1: what the device returned; where given, w' is evaluated from the returned moments and ema' from the returned w', as
    adam_w_ref does -- otherwise the float64 values take their place (a pure float64 step, for the hand-worked cases)."""
    n = np.size(w)
    mask = np.zeros(n, bool).reshape(np.shape(w)) if mask is None else np.asarray(mask, bool).reshape(np.shape(w))
    rm, bm, rv, bv = adam_moments_ref(np.asarray(g, F32), np.asarray(m, F32), np.asarray(v, F32), grad_factor32(gs, c))
    wd, bd = decay_ref(w, weight_decay, mask, lr) if weight_decay else (np.asarray(w, F64), np.zeros(np.shape(w)))
    rw, bw = adam_w_ref(wd, rm if m1 is None else np.asarray(m1), rv if v1 is None else np.asarray(v1), t)
    out = {'m': (rm, bm), 'v': (rv, bv), 'w': (rw, bw + bd)}
    if ema is not None:
        out['ema'] = ema_ref(ema, rw if w1 is None else w1, mu)
    return out


def ratios(got, ref):
    """Largest error over its bound per output; an entry with a zero bound must be exact (ratio 0, else inf)."""
    out = {}
    for k, (val, bound) in ref.items():
        err = np.abs(np.asarray(got[k], F64) - val)
        with np.errstate(divide='ignore', invalid='ignore'):
            r = np.where(bound > 0, err / bound, np.where(err == 0, 0.0, np.inf))
        out[k] = float(np.max(r)) if r.size else 0.0
    return out


__all__ = ['global_norm64', 'clip_factor32', 'grad_factor32', 'decay_mask', 'decay_ref', 'ema_ref', 'step_ref', 'ratios',
           'adam_consts']
