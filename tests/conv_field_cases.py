"""Fields, references, float32 emulations and conditions of the convolution field tests (not a test module; needs no GPU).

tests/test_gpu_ops.py and tests/test_gpu_conv_views.py judge every convolution on N(0,1) data at max|err| < 2e-4 max|ref|, 200 to 2000
times above what the kernels achieve.  This module serves three kinds of test that need little or no tolerance, on the family table of
tests/conv_view_cases.py (shapes, test hooks and kernel tags unchanged, dense operands only) plus one F(4x4) Winograd family (F44):

1. EXACT fields (exact_fwd / exact_dgrad / exact_wgrad): small integers, half of the pixels zero, one channel a 0/1 land-sea mask with a
   straight coast; references in int64 by the formulas of conv_view_cases.fwd_reference (`epilogue`).  Every product and every partial
   sum in any order is an integer (a multiple of 1/4 inside F(2x2,3x3), whose matrices hold 0, +-1, +-1/2) below 2^24, hence exact in
   float32, and such integers sit wholly in the high bf16 part of the three-way split.  The cases carry `bound`, the quantity the condition
   4 * bound < 2^24 is asserted on.
2. POWER-OF-TWO SCALING (SCALES, scaled, scaling_range): x * 2^a, w * 2^b and b / add / old * 2^(a+b) must scale the output by exactly
   2^(a+b) as long as nothing leaves [2^-100, 2^100]; scaling_range() returns the extreme magnitudes of every operand, its low split part,
   every product and every output.
3. FIELD CLASSES (CLASSES, fields_fwd / fields_dgrad / fields_wgrad) judged per element: e = |got - ref64| / S with S the float64 sum of
   the magnitudes of everything that enters the element (`stat`), against the same statistic of a float32 emulation of the family's
   algorithm class, bar E_kernel <= 4 * E_emul + 2^-24 (`bar`; factor and rounding unit are those of test_conv2d_split_bf16).

The emulations (plain numpy float32: every product is rounded, then every addition; no fused multiply-add):
* `sum` (emul_sum_conv, emul_sum_wgrad): ONE sequential accumulation.  Forward / dgrad: acc = 0, then for ky, for kx, for c (in this
  nesting, c fastest): acc = fl(acc + fl(x[y+ky-p, x+kx-p, c] * w[ky, kx, c, k])), zero padding taking part as products with 0.  Weight
  gradient: per tap and (c, k) the products of the pixels in memory order (image, row, column), accumulated one after the other
  (numpy.cumsum, which adds sequentially in the array's type).  The 'blocked' order is the second order of condition 2: term t goes to
  partial sum t mod 16 (weight gradient: pixels cut into 16 contiguous runs), the 16 partial sums are then added in sequence.
* `wino` (emul_wino_conv, emul_wino_wgrad): F(2x2,3x3) with BT, G, AT of tests/test_winograd_algebra.py, every transform a sequential
  float32 sum of its non-zero terms, the channel (weight gradient: tile) sum sequential.
ReLU: the forward forms with a ReLU need no redraw here and exclude nothing -- ReLU is 1-Lipschitz, so |relu(a) - relu(b)| <= |a - b| and
an element on its kink has a SMALLER per-element error than its pre-activation; the statistic is an absolute error over S, never a
derivative.  Form 0 of part 3 runs without a bias so that S == 0 (a neighbourhood of zeros in a sparse field) is reachable: there the
kernel must return exactly the reference.

Correction of the statistic for the `wino` weight gradient (found on the CPU, by the emulation alone): where x and dz never meet under
tap (a, b), S[a, b, c, k] == 0 and every `sum` order returns an exact zero, but F(2x2,3x3) forms dW = G^T dU G from Winograd-domain
sums that are non-zero whenever x and dz meet under ANOTHER tap of the tile, and these cancel to rounding only: "exactly the
reference" is not a property of the algorithm (test_conv_field_cases.test_wino_wgrad_does_not_return_exact_zeros shows it on
wg_wino / sparse).  Those elements -- and only those -- are scaled by wino_wgrad_scale, the magnitude sum of what the algorithm
adds up, and take part in E under the same bar.  The forward `wino` families never reach S == 0 (24 and more input channels).
"""
import functools

import numpy as np

from oracle import np_ops as N
from tests import conv_view_cases as CV
from tests.test_winograd_algebra import AT, BT, G

F32 = np.float32
UNIT = 2.0 ** -24
SCALES = ((40, 0), (-40, 0), (0, -30), (20, -50), (-33, 17))
CLASSES = ('white', 'offset', 'smooth', 'sparse', 'channel_scales')
EXACT_FORMS = (0, 3, 12, 15)
ENV_KEYS = ('DL4DS_STREAM_FORCE_WS', 'DL4DS_WINO_FORCE', 'DL4DS_SPLIT_FORCE', 'DL4DS_WINO_F44')

# F(4x4,3x3): the ragged one-chunk shape of test_gpu_ops.F44_CASES; part 2 only (its transforms hold 1/6, 1/12, 1/24: not exact on integers)
F44 = CV.Family('wino4_24_32', 'fwd', (1, 17, 19, 24, 32, 3), 'conv_wino4<', env={'DL4DS_WINO_FORCE': 'all', 'DL4DS_WINO_F44': 'force'},
                dgrad_tag='conv_wino')
FWD = [f for f in CV.FAMILIES if f.kind == 'fwd']
WG = [f for f in CV.FAMILIES if f.kind == 'wgrad']
# dgrad of the depth_to_space layer (192 gradient channels read through the view, 48 out, 16 x 18): the streamed-filter kernel
DGRAD_TAG = {'stream_d2s': 'conv_stream<'}
# Families that are not exact under part 1, with the file:line of the cause (none: every family is exact on such data).
NOT_EXACT = {}


def family(name):
    return F44 if name == F44.name else CV.family(name)


def dgrad_tag(fam):
    return DGRAD_TAG.get(fam.name, fam.dgrad_tag)


def algo(tag):
    """the algorithm class of a kernel tag"""
    return 'wino' if tag.startswith('conv_wino') else 'sum'


def rng_of(*what):
    return np.random.default_rng(CV.seed_of('fields', *what))


def frozen(d):
    for v in d.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return d


# ---- references (any dtype: int64 for part 1, float64 for parts 2 and 3) ------------------------------------------------------------
def conv_any(x, w):
    """same-padded cross-correlation of x (N, H, W, Cin) with w (KS, KS, Cin, Cout) in the operands' own type"""
    n, h, wd, ci = x.shape
    ks, _, _, co = w.shape
    p = ks // 2
    xp = np.pad(x, ((0, 0), (p, p), (p, p), (0, 0)))
    y = np.zeros((n, h, wd, co), np.result_type(x.dtype, w.dtype))
    for ky in range(ks):
        for kx in range(ks):
            y += xp[:, ky:ky + h, kx:kx + wd, :] @ w[ky, kx]
    return y


def dgrad_filter(w):
    """(KS, KS, Cin, Cout) -> the (KS, KS, Cout, Cin) filter whose forward convolution of dz is the input gradient"""
    return np.ascontiguousarray(w[::-1, ::-1].transpose(0, 1, 3, 2))


def wgrad_any(x, dz, ks):
    """dw[a, b, c, k] = sum over pixels of xpad[y + a, x + b, c] dz[y, x, k]; db[k] = sum dz"""
    n, h, wd, ci = x.shape
    co = dz.shape[-1]
    p = ks // 2
    xp = np.pad(x, ((0, 0), (p, p), (p, p), (0, 0)))
    dw = np.zeros((ks, ks, ci, co), np.result_type(x.dtype, dz.dtype))
    flat = dz.reshape(-1, co)
    for a in range(ks):
        for b in range(ks):
            dw[a, b] = xp[:, a:a + h, b:b + wd, :].reshape(-1, ci).T @ flat
    return dw, flat.sum(axis=0)


def epilogue(conv, d, epi, bias=True):
    """conv_view_cases.fwd_reference in the type of `conv`: [old +] where(mask > 0, [relu](conv + b + add), 0)"""
    t = conv.dtype
    v = conv + d['b'].astype(t) if bias and d.get('b') is not None else conv
    if epi & 1:
        v = v + d['add'].astype(t)
    if epi & 2:
        v = np.maximum(v, 0)
    if epi & 4:
        v = np.where(d['mask'] > 0, v, 0)
    if epi & 8:
        v = v + d['old'].astype(t)
    return v


# ---- part 1: exact fields ------------------------------------------------------------------------------------------------------------
def _int_field(g, shape, amp):
    """integers in [-amp, amp], about half of the pixels exactly zero; channel 0 a 0/1 mask with a straight coast line (a
    single-channel field keeps its integers)"""
    n, h, w, c = shape
    v = g.integers(-amp, amp + 1, shape) * (g.random((n, h, w, 1)) < 0.5)
    yy, xx = np.mgrid[0:h, 0:w]
    if c > 1:
        v[..., 0] = (2 * xx + 3 * yy > (2 * w + 3 * h) // 2)[None]
    return v.astype(F32)


def _ints(g, shape, amp):
    return g.integers(-amp, amp + 1, shape).astype(F32)


def _signs(g, shape):
    return np.where(g.random(shape) < 0.5, -1.0, 1.0).astype(F32)


@functools.lru_cache(maxsize=None)
def exact_fwd(name):
    fam = family(name)
    n, h, w, ci, co, ks = fam.shape
    g = rng_of(name, 'exact')
    d = dict(x=_int_field(g, (n, h, w, ci), 3), w=_ints(g, (ks, ks, ci, co), 2), b=_ints(g, (co,), 3), add=_ints(g, (n, h, w, co), 4),
             old=_ints(g, (n, h, w, co), 4), mask=_signs(g, (n, h, w, co)))
    d['conv'] = conv_any(d['x'].astype(np.int64), d['w'].astype(np.int64))
    a = lambda k: np.abs(d[k]).astype(np.int64)
    d['bound'] = int((conv_any(a('x'), a('w')) + a('b') + a('add') + a('old')).max())
    return frozen(d)


@functools.lru_cache(maxsize=None)
def exact_dgrad(name):
    """dx = old + where(mask > 0, dgrad(dz, w), 0) (form 12) and old + dgrad(dz, w) (form 8) on integers"""
    fam = family(name)
    n, h, w, ci, co, ks = fam.shape
    g = rng_of(name, 'exact', 'dgrad')
    d = dict(dz=_int_field(g, (n, h, w, co), 3), w=_ints(g, (ks, ks, ci, co), 2), old=_ints(g, (n, h, w, ci), 4), mask=_signs(g, (n, h, w, ci)))
    d['conv'] = conv_any(d['dz'].astype(np.int64), dgrad_filter(d['w']).astype(np.int64))
    d['bound'] = int((conv_any(np.abs(d['dz']).astype(np.int64), np.abs(dgrad_filter(d['w'])).astype(np.int64)) + np.abs(d['old']).astype(np.int64)).max())
    return frozen(d)


@functools.lru_cache(maxsize=None)
def exact_wgrad(name):
    fam = family(name)
    n, h, w, ci, co, ks = fam.shape
    g = rng_of(name, 'exact', 'wgrad')
    d = dict(x=_int_field(g, (n, h, w, ci), 3), dz=_int_field(g, (n, h, w, co), 3), dw0=_ints(g, (ks, ks, ci, co), 4), db0=_ints(g, (co,), 4))
    d['dw'], d['db'] = wgrad_any(d['x'].astype(np.int64), d['dz'].astype(np.int64), ks)
    sw, sb = wgrad_any(np.abs(d['x']).astype(np.int64), np.abs(d['dz']).astype(np.int64), ks)
    d['bound'] = int(max((sw + np.abs(d['dw0']).astype(np.int64)).max(), (sb + np.abs(d['db0']).astype(np.int64)).max()))
    return frozen(d)


# ---- part 2: power-of-two scaling ----------------------------------------------------------------------------------------------------
def scaled(a, k):
    return None if a is None else np.ldexp(a, k).astype(F32)


@functools.lru_cache(maxsize=None)
def scale_fwd(name):
    """N(0,1) operands of conv_view_cases.fwd_case (F44: the same draw at its own shape)"""
    if name != F44.name:
        return CV.fwd_case(name)
    n, h, w, ci, co, ks = F44.shape
    g = rng_of(name, 'scale')
    r = lambda *s: g.standard_normal(s).astype(F32)
    d = dict(x=r(n, h, w, ci), w=r(ks, ks, ci, co) * F32(0.2), b=r(co), add=r(n, h, w, co), mask=r(n, h, w, co), old=r(n, h, w, co))
    d['conv64'] = conv_any(d['x'].astype(np.float64), d['w'].astype(np.float64)) + d['b']
    return frozen(d)


@functools.lru_cache(maxsize=None)
def scale_dgrad(name):
    if name != F44.name:
        return CV.dgrad_case(name)
    n, h, w, ci, co, ks = F44.shape
    g = rng_of(name, 'scale', 'dgrad')
    r = lambda *s: g.standard_normal(s).astype(F32)
    d = dict(dz=r(n, h, w, co), w=r(ks, ks, ci, co) * F32(0.2), mask=r(n, h, w, ci), old=r(n, h, w, ci))
    d['ref'] = np.where(d['mask'] > 0, conv_any(d['dz'].astype(np.float64), dgrad_filter(d['w']).astype(np.float64)), 0.0) + d['old']
    return frozen(d)


def _extremes(*arrays):
    mags = [np.abs(np.asarray(a, np.float64)).ravel() for a in arrays]
    mags = np.concatenate([m[m > 0] for m in mags])
    return float(mags.min()), float(mags.max())


def scaling_range(inputs, others, outputs, a, b):
    """inputs: (data, filter-side) operand pair scaled by 2^a / 2^b; others: operands scaled by 2^(a+b); outputs: unscaled float64
    references.  -> (smallest, largest) magnitude among every non-zero operand, its low split part 2^-16 below it, every product of
    a data and a filter-side value (the smallest: a high part times a low part) and every non-zero output, after scaling."""
    (x0, x1), (w0, w1) = _extremes(inputs[0]), _extremes(inputs[1])
    lo = [x0 * 2.0 ** (a - 16), w0 * 2.0 ** (b - 16), x0 * w0 * 2.0 ** (a + b - 16)]
    hi = [x1 * 2.0 ** a, w1 * 2.0 ** b, x1 * w1 * 2.0 ** (a + b)]
    for group, low in ((others, 16), (outputs, 0)):
        for o in group:
            o0, o1 = _extremes(o)
            lo.append(o0 * 2.0 ** (a + b - low))
            hi.append(o1 * 2.0 ** (a + b))
    return min(lo), max(hi)


# ---- part 3: field classes -------------------------------------------------------------------------------------------------------------
SMOOTH_GRID, SMOOTH_L = 128, 12.0


def field(cls, shape, g):
    """one field class on (N, H, W, C), float32"""
    n, h, w, c = shape
    if cls in ('white', 'channel_scales'):
        v = g.standard_normal(shape)
        if cls == 'channel_scales' and c > 1:
            v = v * 10.0 ** (-3 + 6 * np.arange(c) / (c - 1))
    elif cls == 'offset':
        v = 281 + 12 * g.standard_normal(shape)
    elif cls == 'smooth':
        # white noise on a periodic 128 x 128 grid, Gaussian low-pass of 12 pixels, scaled to a range of 1 over that grid, offset by
        # the range's size; the field is a window of it (neighbouring pixels then differ by about 1 % of the range)
        assert h <= SMOOTH_GRID and w <= SMOOTH_GRID
        k = np.fft.fftfreq(SMOOTH_GRID)[:, None] ** 2 + np.fft.rfftfreq(SMOOTH_GRID)[None, :] ** 2
        f = np.fft.irfft2(np.fft.rfft2(g.standard_normal((n, c, SMOOTH_GRID, SMOOTH_GRID))) * np.exp(-0.5 * (2 * np.pi * SMOOTH_L) ** 2 * k),
                          s=(SMOOTH_GRID, SMOOTH_GRID))
        lo, hi = f.min(axis=(2, 3), keepdims=True), f.max(axis=(2, 3), keepdims=True)
        v = ((f - lo) / (hi - lo) + 1.0)[:, :, :h, :w].transpose(0, 2, 3, 1)
    elif cls == 'sparse':
        v = np.exp(g.standard_normal(shape)) * (g.random(shape) < 0.1)
    else:
        raise KeyError(cls)
    return np.ascontiguousarray(v, F32)


def _out_scale(cls, k):
    return 10.0 ** (-2 + 4 * np.arange(k) / (k - 1)) if cls == 'channel_scales' and k > 1 else np.ones(k)


@functools.lru_cache(maxsize=None)
def fields_fwd(name, cls):
    """x of the class; w = 0.2 N(0,1), b and add N(0,1), all three times the output channel's scale (channel_scales; 1 otherwise)"""
    n, h, w, ci, co, ks = family(name).shape
    g = rng_of(name, cls, 'fwd')
    so = _out_scale(cls, co)
    return frozen(dict(x=field(cls, (n, h, w, ci), g), w=(0.2 * g.standard_normal((ks, ks, ci, co)) * so).astype(F32),
                       b=(g.standard_normal(co) * so).astype(F32), add=(g.standard_normal((n, h, w, co)) * so).astype(F32)))


@functools.lru_cache(maxsize=None)
def fields_dgrad(name, cls):
    """dz of the class (its Cout channels are the input channels of the dgrad); the filters of the dgrad's output channel c scaled"""
    n, h, w, ci, co, ks = family(name).shape
    g = rng_of(name, cls, 'dgrad')
    return frozen(dict(dz=field(cls, (n, h, w, co), g), w=(0.2 * g.standard_normal((ks, ks, ci, co)) * _out_scale(cls, ci)[:, None]).astype(F32)))


@functools.lru_cache(maxsize=None)
def fields_wgrad(name, cls):
    """x and dz of the class (logical layout); channel_scales: dz channel k carries the scale of output channel k's filters"""
    n, h, w, ci, co, ks = family(name).shape
    g = rng_of(name, cls, 'wgrad')
    x = field(cls, (n, h, w, ci), g)
    dz = field('white' if cls == 'channel_scales' else cls, (n, h, w, co), g)
    return frozen(dict(x=x, dz=(dz * _out_scale(cls, co)).astype(F32)))


def stat(got, ref, S, S0=None):
    """-> (E = max over S > 0 of |got - ref| / S, the number of elements with S == 0 that differ from the reference).  S0: the
    `wino` weight gradient's own magnitude sum (wino_wgrad_scale), which takes the place of S where S == 0."""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    assert got.shape == ref.shape == S.shape, (got.shape, ref.shape, S.shape)
    if S0 is not None:
        S = np.where(S > 0, S, S0)
    pos = S > 0
    e = float((np.abs(got - ref)[pos] / S[pos]).max()) if pos.any() else 0.0
    return e, int((got[~pos] != ref[~pos]).sum())


def bar(e_emul):
    return 4.0 * e_emul + UNIT


def truncate16(x):
    """x with 16 significant bits: its two upper bf16 parts (chopped)"""
    return (np.ascontiguousarray(x, F32).view(np.uint32) & np.uint32(0xFFFFFF00)).view(F32)


# ---- float32 emulations ----------------------------------------------------------------------------------------------------------------
def emul_sum_conv(x, w, order='seq'):
    """the `sum` class, forward / dgrad (module docstring); order 'seq' | 'blocked'"""
    x, w = np.asarray(x, F32), np.asarray(w, F32)
    n, h, wd, ci = x.shape
    ks, _, _, co = w.shape
    p = ks // 2
    xp = np.pad(x, ((0, 0), (p, p), (p, p), (0, 0)))
    parts = np.zeros((16 if order == 'blocked' else 1, n, h, wd, co), F32)
    t = 0
    for ky in range(ks):
        for kx in range(ks):
            for c in range(ci):
                parts[t % len(parts)] += xp[:, ky:ky + h, kx:kx + wd, c, None] * w[ky, kx, c]
                t += 1
    acc = parts[0]
    for part in parts[1:]:
        acc = acc + part
    return acc


def _seq_sum(prod, order):
    """sequential float32 sum over axis 0 ('blocked': 16 contiguous runs, each sequential, then added in sequence)"""
    if order == 'seq':
        return np.cumsum(prod, axis=0, dtype=F32)[-1]
    acc = None
    for run in np.array_split(prod, 16, axis=0):
        if len(run):
            s = np.cumsum(run, axis=0, dtype=F32)[-1]
            acc = s if acc is None else acc + s
    return acc


def emul_sum_wgrad(x, dz, ks, order='seq'):
    """the `sum` class, weight gradient -> (dw, db)"""
    x, dz = np.asarray(x, F32), np.asarray(dz, F32)
    n, h, wd, ci = x.shape
    co = dz.shape[-1]
    p = ks // 2
    xp = np.pad(x, ((0, 0), (p, p), (p, p), (0, 0)))
    flat = dz.reshape(-1, co)
    dw = np.zeros((ks, ks, ci, co), F32)
    for a in range(ks):
        for b in range(ks):
            xs = xp[:, a:a + h, b:b + wd, :].reshape(-1, ci)
            for c0 in range(0, ci, 16):                                   # (bounds the size of the product array; no effect on the order)
                dw[a, b, c0:c0 + 16] = _seq_sum(xs[:, c0:c0 + 16, None] * flat[:, None, :], order)
    return dw, _seq_sum(flat, order)


def _mat(m, t, axis):
    """m applied along `axis` of t: every output row a sequential float32 sum of its non-zero terms"""
    rows = []
    for row in np.asarray(m, F32):
        acc = None
        for j, v in enumerate(row):
            if v != 0:
                term = np.take(t, j, axis=axis) * v
                acc = term if acc is None else acc + term
        rows.append(acc)
    return np.stack(rows, axis=axis)


def _tiles(x, size, halo):
    """(N, H, W, C) -> (size, size, N, Ty, Tx, C): the 2-strided tiles of the zero-padded field (H, W padded to even)"""
    n, h, w, c = x.shape
    he, we = h + (h & 1), w + (w & 1)
    xp = np.pad(x, ((0, 0), (halo, he - h + halo), (halo, we - w + halo), (0, 0)))
    return np.stack([np.stack([xp[:, r:r + he:2, s:s + we:2, :] for s in range(size)]) for r in range(size)])


def emul_wino_conv(x, w):
    """the `wino` class, forward / dgrad: Y = A^T [sum_c (G g G^T) . (B^T d B)] A per 2 x 2 output tile"""
    x, w = np.asarray(x, F32), np.asarray(w, F32)
    n, h, wd, ci = x.shape
    co = w.shape[-1]
    U = _mat(G, _mat(G, w, 0), 1)                                       # (4, 4, ci, co)
    V = _mat(BT, _mat(BT, _tiles(x, 4, 1), 0), 1)                      # (4, 4, n, Ty, Tx, ci)
    M = np.zeros(V.shape[:-1] + (co,), F32)
    for c in range(ci):
        M += V[..., c, None] * U[:, :, None, None, None, c, :]
    Y = _mat(AT, _mat(AT, M, 0), 1)                                     # (2, 2, n, Ty, Tx, co)
    ty, tx = Y.shape[3:5]
    return np.ascontiguousarray(Y.transpose(2, 3, 0, 4, 1, 5).reshape(n, 2 * ty, 2 * tx, co)[:, :h, :wd])


def emul_wino_wgrad(x, dz, order='seq'):
    """the `wino` class, weight gradient: dW = G^T [sum over tiles (B^T d B) . (A dY A^T)] G; db: the tiles' pixel sums in sequence"""
    x, dz = np.asarray(x, F32), np.asarray(dz, F32)
    ci, co = x.shape[-1], dz.shape[-1]
    V = _mat(BT, _mat(BT, _tiles(x, 4, 1), 0), 1).reshape(16, -1, ci)
    t = _tiles(dz, 2, 0)
    dM = _mat(AT.T, _mat(AT.T, t, 0), 1).reshape(16, -1, co)
    dU = np.stack([_seq_sum(V[i][:, :, None] * dM[i][:, None, :], order) for i in range(16)]).reshape(4, 4, ci, co)
    db = _seq_sum(((t[0, 0] + t[0, 1]) + t[1, 0] + t[1, 1]).reshape(-1, co), order)
    return _mat(G.T, _mat(G.T, dU, 0), 1), db


def wino_wgrad_scale(x, dz):
    """float64 sum of the magnitudes of everything the F(2x2,3x3) weight gradient adds up: |G^T| [sum over tiles (|B^T| |d| |B|) .
    (|A| |dY| |A^T|)] |G|.  It bounds S = sum |x||dz| from above and is positive wherever x and dz meet under ANY tap of the tile."""
    ci, co = x.shape[-1], dz.shape[-1]
    V = _mat(np.abs(BT), _mat(np.abs(BT), _tiles(_abs64(x), 4, 1), 0), 1).reshape(16, -1, ci)
    dM = _mat(np.abs(AT.T), _mat(np.abs(AT.T), _tiles(_abs64(dz), 2, 0), 0), 1).reshape(16, -1, co)
    dU = np.einsum('itc,itk->ick', V, dM).reshape(4, 4, ci, co)
    return _mat(np.abs(G.T), _mat(np.abs(G.T), dU, 0), 1)


# ---- part 3: cached references, S and emulations per (family, class) ------------------------------------------------------------------
def _abs64(a):
    return np.abs(a.astype(np.float64))


def _emul_conv(kind, x, w):
    return emul_wino_conv(x, w) if kind == 'wino' else emul_sum_conv(x, w)


@functools.lru_cache(maxsize=None)
def fwd_judge(name, cls):
    """-> {form: dict(ref, S, emul, e_emul)} for forms 0 (no bias) and 3 (bias, residual, ReLU) of the family's forward"""
    fam = family(name)
    d = fields_fwd(name, cls)
    conv = conv_any(d['x'].astype(np.float64), d['w'].astype(np.float64))
    s0 = conv_any(_abs64(d['x']), _abs64(d['w']))
    c32 = _emul_conv(algo(fam.tag), d['x'], d['w'])
    out = {0: dict(ref=conv, S=s0, emul=c32),
           3: dict(ref=epilogue(conv, d, 3), S=s0 + _abs64(d['b']) + _abs64(d['add']), emul=np.maximum((c32 + d['b']) + d['add'], F32(0)))}
    for v in out.values():
        v['e_emul'], zeros = stat(v['emul'], v['ref'], v['S'])
        assert zeros == 0
    return out


@functools.lru_cache(maxsize=None)
def dgrad_judge(name, cls):
    fam = family(name)
    d = fields_dgrad(name, cls)
    wt = dgrad_filter(d['w'])
    out = dict(ref=conv_any(d['dz'].astype(np.float64), wt.astype(np.float64)), S=conv_any(_abs64(d['dz']), _abs64(wt)),
               emul=_emul_conv(algo(dgrad_tag(fam)), d['dz'], wt))
    out['e_emul'], zeros = stat(out['emul'], out['ref'], out['S'])
    assert zeros == 0
    return out


@functools.lru_cache(maxsize=None)
def wgrad_judge(name, cls):
    """-> dict(dw=dict(ref, S, emul, e_emul), db=...)"""
    fam = family(name)
    ks = fam.shape[5]
    d = fields_wgrad(name, cls)
    dw, db = wgrad_any(d['x'].astype(np.float64), d['dz'].astype(np.float64), ks)
    sw, sb = wgrad_any(_abs64(d['x']), _abs64(d['dz']), ks)
    wino = algo(fam.tag) == 'wino'
    ew, eb = emul_wino_wgrad(d['x'], d['dz']) if wino else emul_sum_wgrad(d['x'], d['dz'], ks)
    out = dict(dw=dict(ref=dw, S=sw, emul=ew, S0=wino_wgrad_scale(d['x'], d['dz']) if wino else None), db=dict(ref=db, S=sb, emul=eb, S0=None))
    for v in out.values():
        v['e_emul'], zeros = stat(v['emul'], v['ref'], v['S'], v['S0'])
        assert zeros == 0
    return out
