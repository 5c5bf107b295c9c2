"""Inputs, float64 references, launch-geometry restatements and float32 CPU evaluations of tests/test_gpu_step_kernels.py (not a
test module; needs no GPU): the pixel loss (csrc/losses.hip: pixel_loss_kernel / pixel_loss_finish_kernel), binary cross-entropy
(bce_kernel), Adam (csrc/adam.hip) and the ReLU-mask + bias-gradient reduction (csrc/elementwise.hip: bias_act_bwd_kernel,
reduce_slabs_kernel2, relu_mask_flat4_kernel).

Every bound is a count of float32 roundings times u = 2^-24 (the relative error of one rounding to nearest), applied to the sum of
the magnitudes that were added: a chain of k additions of terms x_i is within k u sum|x_i| of the exact sum (first order).  The
launch figures the counts depend on are restated here and tests/test_step_kernels_oracle.py checks each against the source text."""
import os
import re

import numpy as np

from tests import graph_ops_cases as K

F32, F64 = np.float32, np.float64
U = 2.0 ** -24
THREADS = 256           # every kernel here runs blocks of 256 threads = 4 waves of 64
WAVE = 64


def _src(name):
    return open(os.path.join(K.ROOT, 'dl4ds_amd', 'csrc', name)).read()


def cdiv(a, b):
    return -(-a // b)


def next_pow2(k):
    return 1 << (int(k) - 1).bit_length()


# ---------------------------------------------------------------------------------------------------------------- launch figures
LOSS_BLOCK_ELEMS, LOSS_BLOCK_CAP, LOSS_FINISH_LANES = 2048, 1024, 64
ADAM_BLOCK_CAP = 2048
BIAS_ROWS_PER_BLOCK, BIAS_BLOCK_CAP = 8, 1024


def loss_blocks(n):
    return max(1, min(cdiv(n, LOSS_BLOCK_ELEMS), LOSS_BLOCK_CAP))


def loss_figures_in_source():
    """-> (elements per block, block cap, lanes of the finish kernel's strided loop, threads of its launch)."""
    src = _src('losses.hip')
    m = re.search(r'int loss_blocks\(size_t n\) \{ return \(int\)std::max<size_t>\(1, std::min<size_t>\(cdivz\(n, (\d+) \* (\d+)\), (\d+)\)\); \}', src)
    lanes = re.search(r'for \(int k = threadIdx\.x; k < nb; k \+= (\d+)\)', src)
    launch = re.search(r'DL4DS_LAUNCH\(pixel_loss_finish_kernel, dim3\(1\), dim3\((\d+)\)', src)
    block = re.search(r'DL4DS_LAUNCH\(pixel_loss_kernel, dim3\(nb\), dim3\((\d+)\)', src)
    assert int(block.group(1)) == int(m.group(1)) == THREADS
    return int(m.group(1)) * int(m.group(2)), int(m.group(3)), int(lanes.group(1)), int(launch.group(1))


def bce_launch_in_source():
    m = re.search(r'DL4DS_LAUNCH\(bce_kernel, dim3\((\d+)\), dim3\((\d+)\)', _src('losses.hip'))
    return int(m.group(1)), int(m.group(2))


def adam_blocks(n):
    return max(1, min(cdiv(n // 4 + 1, THREADS), ADAM_BLOCK_CAP))


def adam_figures_in_source():
    m = re.search(r'std::min<size_t>\(cdivz\(n / 4 \+ 1, (\d+)\), (\d+)\)', _src('adam.hip'))
    return int(m.group(1)), int(m.group(2))


def pick_tx(c):
    return 8 if c <= 8 else (16 if c <= 16 else (32 if c <= 32 else 64))


def pick_tx_in_source():
    m = re.search(r'int pick_tx\(int C\) \{ return C <= (\d+) \? (\d+) : \(C <= (\d+) \? (\d+) : \(C <= (\d+) \? (\d+) : (\d+)\)\); \}',
                  _src('elementwise.hip'))
    return tuple(int(v) for v in m.groups())


def bias_blocks(npix, ty):
    return min(cdiv(npix, ty * BIAS_ROWS_PER_BLOCK), BIAS_BLOCK_CAP)


def bias_blocks_in_source():
    m = re.search(r'int bias_blocks\(size_t npix, int TY\) \{ return \(int\)std::min<size_t>\(cdivz\(npix, \(size_t\)TY \* (\d+)\), (\d+)\); \}',
                  _src('elementwise.hip'))
    return int(m.group(1)), int(m.group(2))


def _wave_sum(v):
    """wave_sum (csrc/common.h) as lane 0 sees it: v[i] += v[i + o] for o = 32 .. 1 over the last axis of 64 lanes -> (...,)."""
    v = v.astype(F32).copy()
    for o in (32, 16, 8, 4, 2, 1):
        v[..., :o] = v[..., :o] + v[..., o:2 * o]
    return v[..., 0]


def _serial_sum(v, axis):
    """0 + v[0] + v[1] + ... in float32 along ``axis``."""
    v = np.moveaxis(v.astype(F32), axis, 0)
    s = np.zeros(v.shape[1:], F32)
    for k in range(v.shape[0]):
        s = s + v[k]
    return s


def _block_sums(terms, nblocks):
    """A grid-stride thread loop over ``terms`` (float32, flat) with ``nblocks`` blocks of 256 threads followed by block_sum
    (csrc/losses.hip): per-thread serial sum, wave_sum, then thread 0 adds the four waves in order -> (nblocks,) float32."""
    nthr = nblocks * THREADS
    iters = cdiv(terms.size, nthr)
    pad = np.zeros(iters * nthr, F32)
    pad[:terms.size] = terms
    per_thread = _serial_sum(pad.reshape(iters, nthr), 0)
    return _serial_sum(_wave_sum(per_thread.reshape(nblocks, THREADS // WAVE, WAVE)), 1)


# ---------------------------------------------------------------------------------------------------------------- pixel loss
LOSS_SHAPES = [(1, 1, 1, 1), (1, 1, 2047, 1), (1, 1, 2049, 1), (1, 1, 64 * 2048 + 1, 1), (1, 1, 1024 * 2048 + 3 * 2048 + 5, 1),
               (2, 9, 7, 3)]
LOSS_LARGEST = 1024 * 2048 + 3 * 2048 + 5


def loss_chain(n):
    """The longest chain of float32 roundings between the float32 terms |d| / d^2 and the loss value, counted from losses.hip:
    thread loop (one addition per grid-stride iteration) + wave_sum (6) + block_sum's thread 0 over the four waves (4) + the finish
    kernel's lane-strided loop (ceil(blocks / 64)) + its wave_sum (6) + 4: the term itself when ``ss += d * d`` is contracted into a
    fused multiply-add (the product is then not rounded to the float32 term), inv_n = fl(1 / n), and the two multiplications of
    wa * a * inv_n.  45 at the largest size."""
    nb = loss_blocks(n)
    return cdiv(n, nb * THREADS) + 6 + THREADS // WAVE + cdiv(nb, LOSS_FINISH_LANES) + 6 + 4


LOSS_CHAIN_LARGEST = 45
LOSS_VALUE_BOUND = next_pow2(LOSS_CHAIN_LARGEST) * U          # 64 roundings = 2^-18, relative to sum |terms| (/ n)
LOSS_MSE_GRAD_BOUND = 2.0 ** -22                              # three roundings (d, inv_n, gs * 2 * d) < 4 u, relative to |2 (p - t) / n|


def loss_inputs(shape, seed):
    """(t, p): seeded normals with p == t exactly on a fifth of the entries (flat index = 3 mod 5)."""
    rng = np.random.default_rng(seed)
    t = rng.standard_normal(shape).astype(F32)
    p = (t + F32(0.5) * rng.standard_normal(shape).astype(F32)).astype(F32)
    hit = (np.arange(t.size) % 5 == 3).reshape(shape)
    p[hit] = t[hit]
    return t, p


def loss_terms32(kind, t, p):
    d = (p - t).astype(F32)
    return (np.abs(d) if kind == 'mae' else d * d).astype(F32).ravel()


def loss_ref(kind, t, p):
    """-> (float64 mean of the float32-evaluated terms, mean of their magnitudes: the same number, the terms are >= 0)."""
    v = float(loss_terms32(kind, t, p).astype(F64).sum() / t.size)
    return v, v


def loss_value32(kind, t, p):
    """The loss in float32 on the CPU in the kernels' order of additions (no fused multiply-add)."""
    n = t.size
    partial = _block_sums(loss_terms32(kind, t, p), loss_blocks(n))
    lanes = np.zeros(cdiv(partial.size, LOSS_FINISH_LANES) * LOSS_FINISH_LANES, F32)
    lanes[:partial.size] = partial
    a = _wave_sum(_serial_sum(lanes.reshape(-1, LOSS_FINISH_LANES), 0))
    return float(F32(a) * (F32(1) / F32(n)))


def mse_grad_ref(t, p):
    return 2.0 * (p.astype(F64) - t.astype(F64)) / t.size


# ---------------------------------------------------------------------------------------------------------------- BCE
BCE_EPS = F32(1e-7)
BCE_ONE_M = F32(1) - BCE_EPS
BCE_SIZES = (1, 16, 255, 256, 257, 1000)
BCE_LABELS = (0.0, 1.0, 0.9)
BCE_SPECIALS = np.array([0.0, 1.0, 1e-9, BCE_EPS, BCE_ONE_M, 0.5], F32)


def bce_inputs(n, seed=0):
    p = np.concatenate([BCE_SPECIALS, np.random.default_rng(seed).random(max(n, 8)).astype(F32)])
    return p[:n].copy()


def bce_ref(p, label):
    """float64 with the float32 values of label, eps and 1 - eps -> (loss, mean magnitude of the terms, gradient, its magnitude).
    Both halves of a term, -l log(pc) and -(1 - l) log(1 - pc), are >= 0, so the magnitude of a term is the term; the magnitude of a
    gradient entry is l / pc + (1 - l) / (1 - pc) (over n), the sum of the two parts whose difference it is: rounding errors of a
    difference are relative to that, not to what is left after cancellation (label 0.9 near p = 0.9).  For labels 0 and 1 it is
    |gradient|.  The gradient is exactly 0 where p < eps or p > 1 - eps."""
    n = p.size
    l, p64 = F64(F32(label)), p.astype(F64)
    pc = np.clip(p64, F64(BCE_EPS), F64(BCE_ONE_M))
    terms = -(l * np.log(pc) + (1.0 - l) * np.log1p(-pc))
    inside = (p64 >= F64(BCE_EPS)) & (p64 <= F64(BCE_ONE_M))
    g = np.where(inside, -(l / pc - (1.0 - l) / (1.0 - pc)), 0.0) / n
    gmag = (l / pc + (1.0 - l) / (1.0 - pc)) / n
    return float(terms.sum() / n), float(np.abs(terms).sum() / n), g, gmag


def bce32(p, label):
    """bce_kernel's expressions in float32 on the CPU, summed in its order (one block) -> (loss, gradient)."""
    n = p.size
    l, one = F32(label), F32(1)
    pc = np.minimum(np.maximum(p, BCE_EPS), BCE_ONE_M).astype(F32)
    terms = (-(l * np.log(pc) + (one - l) * np.log(one - pc))).astype(F32)
    assert terms.dtype == F32
    tot = _block_sums(terms, 1)[0]
    inside = (p >= BCE_EPS) & (p <= BCE_ONE_M)
    g = np.where(inside, -(l / pc - (one - l) / (one - pc)), F32(0)).astype(F32)
    return float(F32(tot) / F32(n)), (g / F32(n)).astype(F32)


def bce_errors(loss, grad, p, label):
    """-> (loss error relative to the mean term magnitude, largest gradient error relative to the entry's magnitude)."""
    ref, mag, g, gmag = bce_ref(p, label)
    return abs(loss - ref) / mag, float((np.abs(grad.astype(F64).ravel() - g) / gmag).max())


def bce_zero_gradient(p):
    return (p < BCE_EPS) | (p > BCE_ONE_M)


# ---------------------------------------------------------------------------------------------------------------- Adam
ADAM_SIZES = (1, 2, 3, 4, 5, 1023, 1025, 2051, 4 * 256 * 2048 + 4 * 256 * 600 + 3)
ADAM_LARGEST = ADAM_SIZES[-1]
ADAM_STEPS = (1, 7, 10000)
ADAM_SCALES = (1.0, 0.5, 1.0 / 3.0)
ADAM_LR, ADAM_B1, ADAM_B2, ADAM_EPS = 1e-3, 0.9, 0.999, 1e-7
ADAM_BOUND = 2.0 ** -22


def adam_inputs(n, seed=0):
    """(w, g, m, v) and the mask of idle entries (g = m = v = 0: nothing may move, w' == w bitwise).  g = 1e-30 at i = 1 mod 11,
    g = 1e15 at i = 2 mod 13, idle entries at i = 3 mod 7 and, from n = 5 on, the last entry (in the scalar tail when n % 4 != 0).
    v > 0 outside the idle entries: where g^2 underflows in float32 (1e-60), b2 v carries the bound."""
    rng = np.random.default_rng(seed)
    w, g = rng.standard_normal(n).astype(F32), rng.standard_normal(n).astype(F32)
    m = (F32(0.1) * rng.standard_normal(n)).astype(F32)
    v = (F32(0.1) * np.abs(rng.standard_normal(n)) + F32(1e-6)).astype(F32)
    i = np.arange(n)
    g[i % 11 == 1] = F32(1e-30)
    g[i % 13 == 2] = F32(1e15)
    idle = i % 7 == 3
    if n >= 5:
        idle[-1] = True
    g[idle] = m[idle] = v[idle] = 0
    return w, g, m, v, idle


def adam_consts(t):
    """float64 values of the float32 constants the kernel receives (dl4ds_op_adam folds lr_t in double and passes it as float)."""
    b1, b2, eps, lr = F64(F32(ADAM_B1)), F64(F32(ADAM_B2)), F64(F32(ADAM_EPS)), F64(F32(ADAM_LR))
    lr_t = F64(F32(lr * np.sqrt(1.0 - b2 ** t) / (1.0 - b1 ** t)))
    return b1, b2, eps, lr_t


def adam_moments_ref(g, m, v, gs):
    """-> (m', bound on m', v', bound on v') in float64: 2^-22 (|b1 m| + |(1 - b1) g|) and 2^-22 (|b2 v| + |(1 - b2) g^2|), g scaled."""
    b1, b2, _, _ = adam_consts(1)
    gr = g.astype(F64) * F64(F32(gs))
    am, bm = b1 * m.astype(F64), (1.0 - b1) * gr
    av, bv = b2 * v.astype(F64), (1.0 - b2) * gr * gr
    return am + bm, ADAM_BOUND * (np.abs(am) + np.abs(bm)), av + bv, ADAM_BOUND * (av + bv)


def adam_w_ref(w, m1, v1, t):
    """w - lr_t m' / (sqrt(v') + eps) in float64 from the moments the kernel returned -> (w', bound 2^-22 (|w| + |step|))."""
    _, _, eps, lr_t = adam_consts(t)
    step = lr_t * m1.astype(F64) / (np.sqrt(v1.astype(F64)) + eps)
    return w.astype(F64) - step, ADAM_BOUND * (np.abs(w.astype(F64)) + np.abs(step))


def adam32(w, g, m, v, t, gs):
    """adam_kernel's expressions in float32 on the CPU (no fused multiply-add) -> (w', m', v')."""
    b1, b2, eps, lr_t = (F32(c) for c in adam_consts(t))
    one = F32(1)
    with np.errstate(under='ignore'):
        gr = g * F32(gs)
        m1 = b1 * m + (one - b1) * gr
        v1 = b2 * v + (one - b2) * gr * gr
        w1 = w - lr_t * m1 / (np.sqrt(v1) + eps)
    assert w1.dtype == m1.dtype == v1.dtype == F32
    return w1, m1, v1


def adam_errors(w1, m1, v1, w, g, m, v, t, gs):
    """Largest error over its bound for (m', v', w'); an entry with a zero bound must be exact (ratio 0, else inf)."""
    def ratio(got, ref, bound):
        err = np.abs(got.astype(F64) - ref)
        with np.errstate(divide='ignore', invalid='ignore'):
            r = np.where(bound > 0, err / bound, np.where(err == 0, 0.0, np.inf))
        return float(r.max())
    rm, bm, rv, bv = adam_moments_ref(g, m, v, gs)
    rw, bw = adam_w_ref(w, m1, v1, t)
    return ratio(m1, rm, bm), ratio(v1, rv, bv), ratio(w1, rw, bw)


# ---------------------------------------------------------------------------------------------------------------- bias_act_bwd
BIAS_CHANS = (1, 3, 8, 13, 32, 48, 100, 130)


def bias_geometry(c, npix):
    """-> dict(tx, ty, cblocks, nb, iters, chain): bias_act_backward's launch for C channels and npix pixels.  chain: the roundings
    between the dz entries and db[c] -- the thread's pixel loop (iters additions), the block's sum over its TY rows (TY) and
    reduce_slabs_kernel2's serial sum over the nb slabs (nb)."""
    tx = pick_tx(c)
    ty = THREADS // tx
    nb = bias_blocks(npix, ty)
    iters = cdiv(npix, nb * ty)
    return dict(tx=tx, ty=ty, cblocks=cdiv(c, tx), nb=nb, iters=iters, chain=iters + ty + nb)


def bias_pixel_counts(c):
    ty = THREADS // pick_tx(c)
    return (1, ty - 1, ty + 1)


# one pixel count just above cap x TY per TX (129 blocks: every thread's pixel loop runs eight times, the ninth for one row) and, for
# TX = 8 and 64, just above cap x TY x 8, where the cap holds the grid at 1024 blocks and the loop stride is the capped grid's
BIAS_LARGE = [(8, BIAS_BLOCK_CAP * 32 + 1), (13, BIAS_BLOCK_CAP * 16 + 1), (32, BIAS_BLOCK_CAP * 8 + 1), (130, BIAS_BLOCK_CAP * 4 + 1),
              (3, BIAS_BLOCK_CAP * 32 * BIAS_ROWS_PER_BLOCK + 1), (100, BIAS_BLOCK_CAP * 4 * BIAS_ROWS_PER_BLOCK + 1)]


def bias_inputs(shape, seed):
    """(dy, y): seeded normals; a fifth of y is +0.0, a fifth -0.0 (by hash of the flat index, so every channel gets each)."""
    rng = np.random.default_rng(seed)
    dy, y = rng.standard_normal(shape).astype(F32), rng.standard_normal(shape).astype(F32)
    cls = (K._mix(dy.size, seed) >> np.uint32(8)) % np.uint32(5)
    y.ravel()[cls == 0] = F32(0.0)
    y.ravel()[cls == 1] = F32(-0.0)
    return dy, y


def bias_ref(dy, y):
    """-> (dz = where(y > 0, dy, 0) in float32, float64 channel sums of dz, channel sums of |dz|)."""
    dz = np.where(y > 0, dy, F32(0)).astype(F32)
    flat = dz.reshape(-1, dz.shape[-1]).astype(F64)
    return dz, flat.sum(axis=0), np.abs(flat).sum(axis=0)


def bias_db_bound(c, npix, abs_sum):
    return next_pow2(bias_geometry(c, npix)['chain']) * U * abs_sum


def bias_db32(dz):
    """db in float32 on the CPU in the kernels' order of additions."""
    c = dz.shape[-1]
    flat = dz.reshape(-1, c)
    geo = bias_geometry(c, flat.shape[0])
    pad = np.zeros((geo['iters'] * geo['nb'] * geo['ty'], c), F32)
    pad[:flat.shape[0]] = flat
    rows = _serial_sum(pad.reshape(geo['iters'], geo['nb'], geo['ty'], c), 0)
    return _serial_sum(_serial_sum(rows, 1), 0)


def flat4_large_shape():
    """(1, H, W, 4) with total / 4 inside the second-iteration rule of relu_mask_flat4_kernel's ew_blocks launch."""
    return K.large_grid(1) + (4,)
