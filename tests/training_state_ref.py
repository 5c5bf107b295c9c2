"""float64 numpy restatement of what the reference's optimiser does between steps (not a test module; needs no GPU and imports
nothing from the product): Keras Adam driven by PiecewiseConstantDecay, with the optional clipping by the global norm, decoupled
weight decay and weight average of the Keras optimiser base class, and the bounds tests/test_gpu_training_state.py holds a device
step to.

The schedule (reference supervised.py:340-346): a (lr0, lr1) pair becomes PiecewiseConstantDecay([lr_decay_after], [lr0, lr1]),
and Keras evaluates it on ``optimizer.iterations`` BEFORE the update increments it: lr = lr0 while iterations <= boundary, lr1
after, where iterations = the number of updates already applied.  With boundary 2 the updates number 0, 1, 2 take lr0.

Keras Adam (keras/optimizers/adam.py, update_step), for the update that takes iterations from t - 1 to t:
    lr_t = lr * sqrt(1 - beta_2^t) / (1 - beta_1^t)
    m_t  = m + (1 - beta_1) (g - m)             = beta_1 m + (1 - beta_1) g
    v_t  = v + (1 - beta_2) (g^2 - v)           = beta_2 v + (1 - beta_2) g^2
    w_t  = w - lr_t m_t / (sqrt(v_t) + epsilon)
beta_1, beta_2 and epsilon are float32 variables' dtype casts there, so the float64 restatement uses the float32 values of the
constants (1 - beta in float32 is exact, Sterbenz), never the decimal ones.

Around it (keras/optimizers/optimizer.py): tf.clip_by_global_norm scales every gradient by clip / max(||g||, clip) first;
decoupled weight decay subtracts lr * weight_decay * w from the decayed variables with the PLAIN scheduled lr (not lr_t) before
the Adam update; the average follows average = momentum * average + (1 - momentum) * w_t after it.

Bounds, per entry.  u = 2^-24 is one rounding to nearest:
  m, v   4 ulp of float32 at the size of the larger of the two terms of the update.  Each is two products and a sum: half an ulp
         per product at its own size, half an ulp of the sum, which is at most twice the larger term (one ulp of the larger term),
         the squaring and the scale factor of g at most 1.5 more: below 4.  Terms under the smallest normal float32 have no
         relative precision and may be flushed to zero: 2 * 2^-126 is added for the two of them.
  w      |dw - dw_ref| <= 2e-3 * lr + 2^-23 |w|: the project's first-step figure (2e-6 at lr = 1e-3, 0.2 % of one step, which is
         what lr_t * m / (sqrt(v) + eps) moves an entry by when |m| / sqrt(v) is of order one) scaled with lr, plus the rounding of
         the subtraction at the size of w."""
import numpy as np

F32, F64 = np.float32, np.float64
TINY = 2.0 ** -126
W_REL, W_ULP = 2e-3, 2.0 ** -23


def scheduled_lr(iterations, lr0, lr1, boundary):
    """PiecewiseConstantDecay([boundary], [lr0, lr1]) at optimizer.iterations = updates already applied."""
    return lr0 if iterations <= boundary else lr1


def consts32(beta_1, beta_2, epsilon):
    return F64(F32(beta_1)), F64(F32(beta_2)), F64(F32(epsilon))


def ulp32(x):
    """Spacing of float32 at |x| (float64 in, float64 out)."""
    return np.spacing(np.abs(np.asarray(x, F64)).astype(F32)).astype(F64)


def clip_factor(grads, clipnorm):
    """tf.clip_by_global_norm's factor over a list / dict of gradient arrays, float64."""
    gs = grads.values() if isinstance(grads, dict) else grads
    norm = np.sqrt(sum(float(np.sum(np.asarray(g, F64) ** 2)) for g in gs))
    return clipnorm / max(norm, clipnorm), norm


def adam_step(w, g, m, v, iterations, lr, beta_1=0.9, beta_2=0.999, epsilon=1e-7, t_shift=0, grad_factor=1.0, decay=0.0):
    """One Keras-Adam update in float64 from the state before it -> dict(w, m, v, dw, m_bound, v_bound, w_bound).

    iterations: updates already applied; the update uses t = iterations + 1 (+ t_shift: a deliberately wrong restatement, for the
    proof that the bounds discriminate).  lr: the scheduled rate of this update.  grad_factor: the clipping factor (a float32 as the
    optimiser holds it).  decay: weight_decay for this tensor (0: not decayed); applied with the plain lr before the update."""
    b1, b2, eps = consts32(beta_1, beta_2, epsilon)
    w, g, m, v = (np.asarray(a, F64) for a in (w, g, m, v))
    gr = g * F64(F32(grad_factor))
    t = iterations + 1 + t_shift
    lr_t = lr * np.sqrt(1.0 - b2 ** t) / (1.0 - b1 ** t)
    am, bm = b1 * m, (1.0 - b1) * gr
    av, bv = b2 * v, (1.0 - b2) * gr * gr
    m1, v1 = am + bm, av + bv
    wd = w - F64(lr) * F64(decay) * w if decay else w
    w1 = wd - lr_t * m1 / (np.sqrt(v1) + eps)
    return dict(w=w1, m=m1, v=v1, dw=w1 - w,
                m_bound=4.0 * ulp32(np.maximum(np.abs(am), np.abs(bm))) + 2 * TINY,
                v_bound=4.0 * ulp32(np.maximum(av, bv)) + 2 * TINY,
                w_bound=W_REL * lr + W_ULP * np.abs(w))


def ema_step(average, w_new, momentum):
    """average' = momentum * average + (1 - momentum) * w' (float32 momentum) -> (value, bound: 4 ulp at the larger term)."""
    mu = F64(F32(momentum))
    a, b = mu * np.asarray(average, F64), (1.0 - mu) * np.asarray(w_new, F64)
    return a + b, 4.0 * ulp32(np.maximum(np.abs(a), np.abs(b))) + 2 * TINY


def check_step(before, g, after, iterations, lr, **kw):
    """Device state (w, m, v) before and after one update against adam_step -> dict of worst figures and failure masks:
    m_ulps / v_ulps (largest error in units of the bound's ulp, i.e. 4 = the bound), w_over_lr (largest |dw - dw_ref| / lr),
    m_bad, v_bad, w_bad (boolean arrays of the entries over their bound)."""
    w0, m0, v0 = before
    w1, m1, v1 = after
    r = adam_step(w0, g, m0, v0, iterations, lr, **kw)
    em = np.abs(np.asarray(m1, F64) - r['m'])
    ev = np.abs(np.asarray(v1, F64) - r['v'])
    ew = np.abs((np.asarray(w1, F64) - np.asarray(w0, F64)) - r['dw'])
    return dict(m_ulps=float((4.0 * em / r['m_bound']).max(initial=0.0)), v_ulps=float((4.0 * ev / r['v_bound']).max(initial=0.0)),
                w_over_lr=float(ew.max(initial=0.0) / lr), m_bad=em > r['m_bound'], v_bad=ev > r['v_bound'], w_bad=ew > r['w_bound'],
                ref=r)


def implied_lr(before, after, iterations, beta_1=0.9, beta_2=0.999, epsilon=1e-7):
    """The rate a device update used, read off its own result: the median over the entries that moved of dw / (dw at lr = 1 from the
    moments the device returned)."""
    w0, w1, m1, v1 = (np.asarray(a, F64).ravel() for a in (before, after[0], after[1], after[2]))
    b1, b2, eps = consts32(beta_1, beta_2, epsilon)
    t = iterations + 1
    unit = np.sqrt(1.0 - b2 ** t) / (1.0 - b1 ** t) * m1 / (np.sqrt(v1) + eps)
    ok = np.abs(unit) > 0.1                       # entries that move by a good part of a step: w1 - w0 carries 3+ digits of it
    return float(np.median((w0[ok] - w1[ok]) / unit[ok]))


def adam32(w, g, m, v, iterations, lr, beta_1=0.9, beta_2=0.999, epsilon=1e-7):
    """The same update evaluated in float32 (what a correct device does, up to the order of roundings) -> (w', m', v')."""
    b1, b2, eps = F32(beta_1), F32(beta_2), F32(epsilon)
    t = iterations + 1
    lr_t = F32(lr * np.sqrt(1.0 - F64(b2) ** t) / (1.0 - F64(b1) ** t))
    one = F32(1)
    with np.errstate(under='ignore'):
        m1 = b1 * m + (one - b1) * g
        v1 = b2 * v + (one - b2) * g * g
        w1 = w - lr_t * m1 / (np.sqrt(v1) + eps)
    assert w1.dtype == m1.dtype == v1.dtype == F32
    return w1, m1, v1
