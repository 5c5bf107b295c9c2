"""fp64 restatement of the weighted losses (torch autograd on the CPU) -- the reference of tests/test_weighted_loss_api.py and
tests/test_gpu_weighted_loss.py.  Not a test module.

With d = p - t, w broadcast to the (N, H, W, C) batch and sums over all its entries:
    mae_w = sum w|d| / sum w          mse_w = sum w d^2 / sum w
    dssim_w = sum omega (1 - s)/2 / sum omega,  omega = G * w over the VALID 11x11 windows (G: the Gaussian of the SSIM moments),
              s the per-window, per-channel SSIM of the shifted arrays with the whole arrays' dynamic range (oracle.torch_ops.dssim)
and the mixes 0.8/0.2 and 0.6/0.2/0.2 over those terms.  Entries (windows) of weight 0 are excluded with torch.where on the INPUTS,
so that a NaN / Inf there reaches neither the value nor the gradient; a zero weight sum gives 0.
The Gaussian window and the depthwise VALID filter are oracle.torch_ops' own."""
import numpy as np
import torch

from oracle import torch_ops as T

KINDS = ('mae', 'mse', 'dssim', 'dssim_mae', 'dssim_mse', 'dssim_mae_mse')
MIX = {'mae': (0.0, 1.0, 0.0), 'mse': (0.0, 0.0, 1.0), 'dssim': (1.0, 0.0, 0.0), 'dssim_mae': (0.8, 0.2, 0.0),
       'dssim_mse': (0.8, 0.0, 0.2), 'dssim_mae_mse': (0.6, 0.2, 0.2)}          # (dssim, mae, mse)


def broadcast_weights(w, shape):
    """Weights in any accepted form -> float64 tensor of the batch's shape (N, H, W, C); M maps: sample row r uses map r // (N // M)."""
    n, h, wd, c = shape
    w = torch.as_tensor(np.asarray(w, np.float64))
    if w.ndim == 2:
        w = w[None, :, :, None]
    elif w.ndim == 3:
        w = w[None]
    assert w.ndim == 4 and n % w.shape[0] == 0 and tuple(w.shape[1:3]) == (h, wd) and w.shape[3] in (1, c), (tuple(w.shape), shape)
    return w.repeat_interleave(n // w.shape[0], dim=0).expand(n, h, wd, c)


def _residual(y_true, y_pred, w):
    keep = w > 0
    zero = torch.zeros_like(y_pred)
    return torch.where(keep, y_pred - torch.where(keep, y_true, zero), zero), keep


def mae_w(y_true, y_pred, w):
    d, keep = _residual(y_true, y_pred, w)
    sw = w.sum()
    if float(sw) == 0.0:
        return (y_pred * 0.0).sum()
    return torch.where(keep, w * d.abs(), torch.zeros_like(d)).sum() / sw


def mse_w(y_true, y_pred, w):
    d, keep = _residual(y_true, y_pred, w)
    sw = w.sum()
    if float(sw) == 0.0:
        return (y_pred * 0.0).sum()
    return torch.where(keep, w * d ** 2, torch.zeros_like(d)).sum() / sw


def ssim_map(img1, img2, max_val, k1=0.01, k2=0.03):
    """Per-window, per-channel SSIM (N, Ho, Wo, C): the body of oracle.torch_ops.ssim before its mean."""
    g = T._gauss_kernel(11, 1.5, img1.dtype)
    c1, c2 = (k1 * max_val) ** 2, (k2 * max_val) ** 2
    m0, m1 = T._valid_depthwise(img1, g), T._valid_depthwise(img2, g)
    num0, den0 = m0 * m1 * 2.0, m0 ** 2 + m1 ** 2
    lum = (num0 + c1) / (den0 + c1)
    num1 = T._valid_depthwise(img1 * img2, g) * 2.0
    den1 = T._valid_depthwise(img1 ** 2 + img2 ** 2, g)
    return lum * (num1 - num0 + c2) / (den1 - den0 + c2)


def window_weights(w):
    return T._valid_depthwise(w.contiguous(), T._gauss_kernel(11, 1.5, w.dtype))


def dssim_w(y_true, y_pred, w):
    drange = torch.maximum(y_true.max(), y_pred.max()) - torch.minimum(y_true.min(), y_pred.min())
    yt = y_true - y_true.min() if y_true.min() < 0 else y_true
    yp = y_pred - y_pred.min() if y_pred.min() < 0 else y_pred
    s = ssim_map(yt, yp, drange)
    om = window_weights(w)
    so = om.sum()
    if float(so) == 0.0:
        return (y_pred * 0.0).sum()
    return torch.where(om > 0, om * (1.0 - s) / 2.0, torch.zeros_like(s)).sum() / so


def loss_w(kind, y_true, y_pred, w):
    """The weighted loss `kind` of fp64 tensors, w already broadcast (broadcast_weights)."""
    a, b, c = MIX[kind]
    v = 0.0
    if a:
        v = v + a * dssim_w(y_true, y_pred, w)
    if b:
        v = v + b * mae_w(y_true, y_pred, w)
    if c:
        v = v + c * mse_w(y_true, y_pred, w)
    return v


def value_and_grad(kind, y_true, y_pred, weights):
    """numpy in -> (loss, dloss/dpred as float64 numpy)."""
    t = torch.tensor(np.asarray(y_true, np.float64))
    p = torch.tensor(np.asarray(y_pred, np.float64), requires_grad=True)
    v = loss_w(kind, t, p, broadcast_weights(weights, tuple(t.shape)))
    v.backward()
    return float(v.detach()), p.grad.numpy()
