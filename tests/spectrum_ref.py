"""numpy restatement of the spectral verification of dl4ds_amd.metrics.spectral_scores: per field
np.fft.fft2 in fp64 on the float32 values, binned over the half plane through the same integer map with the same multiplicities
(tests/test_spectral_api.py checks the power against the full-plane sum through Parseval), and the host arithmetic of the result
dict written out again.  `dft2_matrix` is a second, independent fp64 evaluation of the transform (the DFT matrices applied by
``@``); tests/test_spectral_api.py checks one against the other and both against answers worked by hand.  Imports nothing from the product."""
import math

import numpy as np


def radial_map(H, W):
    """-> (int32 (H, W) full-plane map, B) with signed wavenumbers, coefficient by coefficient in Python integers."""
    L = max(H, W)
    B = L // 2 + 1
    m = np.empty((H, W), np.int32)
    for i in range(H):
        ky = i if i <= H // 2 else i - H
        for j in range(W):
            kx = j if j <= W // 2 else j - W
            b = (math.isqrt((4 * L ** 2 * (ky ** 2 * W ** 2 + kx ** 2 * H ** 2)) // (H * W) ** 2) + 1) // 2
            m[i, j] = b if b < B else -1
    return m, B


def hann(n):
    return 0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(n) / n)


def prepared_field(y, p, detrend, window):
    """One (H, W) field of either side as the transform sees it -> (vy, vp or None, n_valid, (mean_y, mean_p), T) with
    T = H W sum over the kept cells of the raw y^2 + p^2 (the scale of the error bound)."""
    y64 = np.asarray(y, np.float32).astype(np.float64)
    p64 = None if p is None else np.asarray(p, np.float32).astype(np.float64)
    keep = np.isfinite(y64) if p64 is None else np.isfinite(y64) & np.isfinite(p64)
    n = int(keep.sum())
    H, W = y64.shape
    w2 = np.outer(hann(H), hann(W)) if window else None
    out, means, T = [], [], 0.0
    for a in (y64, p64):
        if a is None:
            out.append(None)
            means.append(0.0)
            continue
        m = float(np.mean(a[keep])) if detrend and n else 0.0
        v = np.where(keep, np.where(keep, a, 0.0) - m, 0.0)
        out.append(v * w2 if window else v)
        means.append(m)
        T += float(np.sum(np.where(keep, a, 0.0) ** 2))
    return out[0], out[1], n, tuple(means), H * W * T


def dft2_matrix(v):
    """The unnormalised 2-D DFT by two matrix products; the angles are reduced as integers (k i mod n) first."""
    H, W = v.shape
    fy = np.exp(-2j * np.pi * ((np.arange(H)[:, None] * np.arange(H)[None, :]) % H) / H)
    fx = np.exp(-2j * np.pi * ((np.arange(W)[:, None] * np.arange(W)[None, :]) % W) / W)
    return fy @ v.astype(np.complex128) @ fx


def binned(X, Y, full, B):
    """sum over the half-plane coefficients kx = 0 .. W/2 of every bin of mult X conj(Y) -> complex (B,); mult = 1 for kx = 0 and for
    kx = W/2 when W is even, else 2.  For a symmetric map the real part is the full-plane sum; the imaginary part of the full-plane
    sum would vanish (the mirror coefficient is the conjugate), the half plane keeps the phase."""
    W = full.shape[1]
    wh = W // 2 + 1
    mult = np.full(wh, 2.0)
    mult[0] = 1.0
    if W % 2 == 0:
        mult[-1] = 1.0
    half = full[:, :wh]
    sel = half >= 0
    idx = half[sel]
    prod = ((X * np.conj(Y))[:, :wh] * mult)[sel]
    return np.bincount(idx, weights=prod.real, minlength=B) + 1j * np.bincount(idx, weights=prod.imag, minlength=B)


def field_sums(y, p, full, B, detrend=True, window=False, transform=np.fft.fft2):
    """What dl4ds_spectrum returns for one field -> (sums (4, B), n_valid, (mean_y, mean_p), T)."""
    vy, vp, n, means, T = prepared_field(y, p, detrend, window)
    sums = np.zeros((4, B))
    Y = transform(vy)
    sums[0] = binned(Y, Y, full, B).real
    if vp is not None:
        P = transform(vp)
        sums[1] = binned(P, P, full, B).real
        c = binned(Y, P, full, B)
        sums[2], sums[3] = c.real, c.imag
    return sums, n, means, T


def device_outputs(y, p, full, B, detrend=True, window=False, mask=None):
    """The three arrays of the C entry for (N, H, W, C) inputs -> (power (N, C, 4, B), n_valid (N, C), mean (N, C, 2), T (N, C))."""
    y = np.array(y, np.float32)
    if mask is not None:
        mask = np.asarray(mask)
        y[np.broadcast_to((mask[..., None] if mask.ndim == 2 else mask) == 0, y.shape)] = np.nan
    N, H, W, C = y.shape
    power, nvalid, mean, T = np.zeros((N, C, 4, B)), np.zeros((N, C), np.int64), np.zeros((N, C, 2)), np.zeros((N, C))
    for n in range(N):
        for c in range(C):
            power[n, c], nvalid[n, c], mean[n, c], T[n, c] = field_sums(y[n, :, :, c], None if p is None else p[n, :, :, c], full, B,
                                                                        detrend, window)
    return power, nvalid, mean, T


def bound(want_power, T, count, c):
    """|got - want| <= 2 d sqrt(M S) + M d^2 per field and bin, d = c 2^-52 sqrt(T), S the larger reference power of the bin"""
    d = c * 2.0 ** -52 * np.sqrt(T)[..., None, None]
    S = np.maximum(want_power[:, :, 0], want_power[:, :, 1])[:, :, None, :]
    M = np.asarray(count, np.float64)[None, None, None, :]
    return 2.0 * d * np.sqrt(M * S) + M * d * d


def _div(num, den):
    num, den = np.asarray(num, np.float64), np.asarray(den, np.float64)
    out = np.full(np.broadcast(num, den).shape, np.nan)
    np.divide(num, den, out=out, where=den != 0)
    return out


def _lsd(ratio, usable):
    out = np.full(ratio.shape[:-1], np.nan)
    for idx in np.ndindex(out.shape):
        d = [10.0 * float(np.log10(r)) for r, u in zip(ratio[idx], usable[idx]) if u]
        if d:
            out[idx] = math.sqrt(math.fsum(v * v for v in d) / len(d))
    return out


def scores_from_sums(power, nvalid, mean, count, hw, spacing=1.0, ratio_floor=0.5):
    """The dict of spectral_scores from the device's three arrays, restated."""
    H, W = hw
    N, C, _, B = power.shape
    L = max(H, W)
    norm = float((H * W) ** 2)
    wavenumber = np.array([b / (float(L) * float(spacing)) for b in range(B)])
    wavelength = np.array([math.inf if b == 0 else 1.0 / wavenumber[b] for b in range(B)])
    po, pp, cr, ci = (power[:, :, k] / norm for k in range(4))
    empty = (nvalid == 0)
    e3 = np.broadcast_to(empty[..., None], po.shape)
    nan_if = lambda a, e: np.where(e, np.nan, a)
    late = np.arange(B) >= 1

    def derived(po, pp, cr, ci):
        usable = late & (count > 0) & (po > 0) & (pp > 0)
        ratio = _div(pp, po)
        return ratio, _div(cr * cr + ci * ci, po * pp), _lsd(ratio, usable)

    ratio, coh, lsd = derived(po, pp, cr, ci)
    res = dict(wavenumber=wavenumber, wavelength=wavelength, count=np.asarray(count, np.int64), n_valid=nvalid,
               mean_obs=mean[..., 0], mean_pred=mean[..., 1], power_obs=po, power_pred=pp,
               psd_obs=nan_if(_div(po, np.broadcast_to(count, po.shape)), e3),
               psd_pred=nan_if(_div(pp, np.broadcast_to(count, pp.shape)), e3), cross=cr + 1j * ci, coherence=nan_if(coh, e3),
               psd_ratio=nan_if(ratio, e3), lsd=nan_if(lsd, empty))
    pooled = []
    for a in (po, pp, cr, ci):
        out = np.zeros((C, B))
        for c in range(C):
            for b in range(B):
                out[c, b] = math.fsum(float(a[n, c, b]) for n in range(N) if not empty[n, c])
        pooled.append(out)
    pratio, pcoh, plsd = derived(*pooled)
    eff = np.full(C, np.nan)
    for c in range(C):
        best = 0
        for b in range(1, B):
            if count[b] > 0 and not (pratio[c, b] >= ratio_floor):
                break
            best = b
        if best > 0:
            eff[c] = wavelength[best]
    res.update(power_obs_pooled=pooled[0], power_pred_pooled=pooled[1], cross_pooled=pooled[2] + 1j * pooled[3],
               psd_ratio_pooled=pratio, coherence_pooled=pcoh, lsd_pooled=plsd, effective_wavelength=eff)
    return res


def spectral_scores(y, p, bins='radial', detrend='mean', window=None, spacing=1.0, ratio_floor=0.5, mask=None):
    """-> (the dict dl4ds_amd.metrics.spectral_scores returns, the raw sums (N, C, 4, B), T (N, C))"""
    H, W = y.shape[1:3]
    if isinstance(bins, str):
        full, B = radial_map(H, W)
    else:
        full = np.asarray(bins, np.int32)
        B = int(full.max()) + 1
    count = np.bincount(full[full >= 0].ravel(), minlength=B).astype(np.int64)
    power, nvalid, mean, T = device_outputs(y, p, full, B, detrend == 'mean', window == 'hann', mask)
    return scores_from_sums(power, nvalid, mean, count, (H, W), spacing, ratio_floor), power, T
