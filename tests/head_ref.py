"""Pure numpy references of the kernels of csrc/head.hip (not a test module; needs no GPU): the counter-based dropout noise, the two
dropout apply kernels, Dense and GlobalAveragePooling -- plus the per-element error bound the Dense / GAP tests use.

Noise scheme (include/dl4ds_hip.h, csrc/graph.h dropout_op_seed, csrc/graph_ops2.hip DropoutOp::forward, csrc/head.hip
dropout_mask_kernel), all arithmetic mod 2^64:

    op seed    s_i = splitmix64(S + GOLDEN * (i + 1))          S: the built-in seed or the one given to reseed_dropout; i: op index
    draw k     d   = s_i + k * 0x1000003                       k = 1, 2, ...: the op's k-th drawing forward pass since the (re)seed
    element e  z   = splitmix64(d + GOLDEN * (e + 1))
               u   = (z >> 40) / 2^24,  u2 = ((z >> 16) & 0xFFFFFF) / 2^24
    keep mask  1 iff u >= float32(rate)
    Gaussian   1 + sigma * sqrt(-2 ln(1 - u)) * cos(2 pi u2),  sigma = sqrt(rate / (1 - rate))

``old_builtin_seed`` is the scheme un-reseeded graphs had before: s_i = BUILTIN + GOLDEN * (i + 1) without the hash, so that
d + GOLDEN * (e + 1) of op i + 1 at element e and of op i at element e + 1 were the same number."""
import numpy as np

F32, F64, U64 = np.float32, np.float64, np.uint64
GOLDEN = 0x9E3779B97F4A7C15
DRAW_STEP = 0x1000003
BUILTIN_SEED = 0x5DEECE66D
_M64 = (1 << 64) - 1
U = 2.0 ** -24                    # unit round-off of float32


# ---------------------------------------------------------------------------------------------------------------- noise
def splitmix64(z):
    """The splitmix64 finaliser on a uint64 array (or a Python int -> Python int)."""
    if isinstance(z, int):
        z &= _M64
        z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & _M64
        z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & _M64
        return z ^ (z >> 31)
    z = np.asarray(z, U64)
    with np.errstate(over='ignore'):
        z = (z ^ (z >> U64(30))) * U64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> U64(27))) * U64(0x94D049BB133111EB)
    return z ^ (z >> U64(31))


def op_seed(seed, index):
    """Seed of dropout op ``index`` of a graph (re)seeded with ``seed``."""
    return splitmix64((int(seed) + GOLDEN * (index + 1)) & _M64)


def builtin_seed(index):
    return op_seed(BUILTIN_SEED, index)


def old_builtin_seed(index):
    return (BUILTIN_SEED + GOLDEN * (index + 1)) & _M64


def hash_bits(seed, draw, n):
    """z of elements 0 .. n-1 of draw ``draw`` (1-based) of the op whose seed is ``seed``."""
    d = (int(seed) + draw * DRAW_STEP) & _M64
    with np.errstate(over='ignore'):
        z = U64(d) + U64(GOLDEN) * (np.arange(n, dtype=U64) + U64(1))
    return splitmix64(z)


def keep_threshold(rate):
    """u >= float32(rate) with u = m / 2^24 <=> m >= ceil(float32(rate) * 2^24): the smallest kept 24-bit value."""
    return int(np.ceil(F64(F32(rate)) * 2.0 ** 24))


def keep_probability(rate):
    return 1.0 - keep_threshold(rate) / 2.0 ** 24


def keep_mask(seed, draw, n, rate):
    m = (hash_bits(seed, draw, n) >> U64(40)).astype(np.int64)
    return (m >= keep_threshold(rate)).astype(F32)


def gaussian_sigma(rate):
    r = F64(F32(rate))
    return float(np.sqrt(r / (1.0 - r)))


def gaussian_mask(seed, draw, n, rate):
    """fp64 values of the multiplicative N(1, sigma^2) noise."""
    z = hash_bits(seed, draw, n)
    u = (z >> U64(40)).astype(F64) * U
    u2 = ((z >> U64(16)) & U64(0xFFFFFF)).astype(F64) * U
    return 1.0 + gaussian_sigma(rate) * np.sqrt(-2.0 * np.log(1.0 - u)) * np.cos(2.0 * np.pi * u2)


def draw_alignment_shifts(max_distance):
    """|s| for every draw distance 1 .. max_distance, where s is the one element shift (mod 2^64, taken as a signed number) at which
    two draws of one op that far apart would read the same hash inputs: dk * DRAW_STEP == GOLDEN * s."""
    q = (DRAW_STEP * pow(GOLDEN, -1, 1 << 64)) & _M64
    with np.errstate(over='ignore'):
        s = U64(q) * np.arange(1, max_distance + 1, dtype=U64)
    return np.abs(s.view(np.int64).astype(F64))


# ---------------------------------------------------------------------------------------------------------------- independence
LAGS = range(-8, 9)


def _overlap(a, b, lag):
    """a[e] against b[e + lag] over the elements both have."""
    n = a.size
    return (a[:n - lag], b[lag:]) if lag >= 0 else (a[-lag:], b[:n + lag])


def agreement_violations(streams, p=0.5):
    """Keep masks (rate such that keep probability is ``p`` = 0.5): every pair of distinct streams at every lag in -8 .. 8 -> list of
    (i, j, lag, agreement fraction, bound) whose agreement fraction over the overlap is further than 6 binomial standard deviations
    from 0.5, and the number of comparisons made."""
    bad, count = [], 0
    for i in range(len(streams)):
        for j in range(i + 1, len(streams)):
            for lag in LAGS:
                a, b = _overlap(streams[i], streams[j], lag)
                frac, bound = float((a == b).mean()), 6.0 * 0.5 / np.sqrt(a.size)
                count += 1
                if abs(frac - 0.5) > bound:
                    bad.append((i, j, lag, frac, bound))
    return bad, count


def correlation_violations(streams):
    """Gaussian noise: the same pairing with |Pearson correlation| < 6 / sqrt(overlap)."""
    bad, count = [], 0
    z = [np.asarray(s, F64) for s in streams]
    for i in range(len(z)):
        for j in range(i + 1, len(z)):
            for lag in LAGS:
                a, b = _overlap(z[i], z[j], lag)
                r, bound = float(np.corrcoef(a, b)[0, 1]), 6.0 / np.sqrt(a.size)
                count += 1
                if not abs(r) < bound:
                    bad.append((i, j, lag, r, bound))
    return bad, count


# ---------------------------------------------------------------------------------------------------------------- dropout apply
def dropout_scale(rate, gaussian):
    """DropoutOp::scale(): 1 / (1 - rate) in float32 (inverted dropout), 1 for the Gaussian variant."""
    return F32(1.0) if gaussian else F32(1.0) / (F32(1.0) - F32(rate))


def broadcast_mask(mask, shape, dim):
    """The spatial variants' mask over a (B, T, H, W, C) tensor: dim 2 -> mask (B * T, C) per frame, dim 3 -> (B, C) per sample;
    None: one entry per element."""
    b, t, h, w, c = shape
    if dim is None:
        return np.asarray(mask).reshape(shape)
    if dim == 2:
        return np.broadcast_to(np.asarray(mask).reshape(b, t, 1, 1, c), shape)
    return np.broadcast_to(np.asarray(mask).reshape(b, 1, 1, 1, c), shape)


def dropout_forward(x, mask, scale):
    """float32(float32(x * mask) * scale): the kernel's two roundings."""
    return (x.astype(F32) * mask.astype(F32)).astype(F32) * F32(scale)


def dropout_backward(dy, mask, scale):
    """fp64 dY * mask * scale."""
    return dy.astype(F64) * mask.astype(F64) * F64(scale)


# ---------------------------------------------------------------------------------------------------------------- error bound
def ulp(ref):
    """Spacing of float32 at |ref|."""
    return np.spacing(np.abs(np.asarray(ref, F64)).astype(F32)).astype(F64)


def sum_bound(k, abs_terms, ref):
    """|err| <= (K + 2) * 2^-24 * sum|terms| + 4 ulp(|ref|): the recursive-summation bound of a K-term fp32 sum (any order) with two
    more roundings for what feeds it, and 4 ulp for expf / tanhf and the activation derivative."""
    return (k + 2) * U * np.asarray(abs_terms, F64) + 4.0 * ulp(ref)


def worst(got, ref, bound):
    """-> (largest err / bound, flat index of it, got, ref there) for the assertion message."""
    err = np.abs(np.asarray(got, F64) - ref) / np.maximum(bound, np.finfo(F64).tiny)
    err = np.where((np.asarray(got, F64) == ref), 0.0, err)
    i = int(np.argmax(err))
    return float(err.flat[i]), i, float(np.asarray(got).flat[i]), float(np.asarray(ref).flat[i])


# ---------------------------------------------------------------------------------------------------------------- loss gradient
def mse_targets(y_dev, seed):
    """Targets y - d with |d| in 0.5 .. 1.5 of either sign, and the float32 difference the loss kernel forms from them: d32 = y - t in
    float32 (one correctly rounded subtraction, the same on the device).  dL/dy = 2 * d32 / size then holds up to the loss kernel's
    two roundings (the factor 2 / size, the product)."""
    r = np.random.default_rng(seed)
    d = r.uniform(0.5, 1.5, y_dev.shape) * r.choice([-1.0, 1.0], y_dev.shape)
    t = (y_dev.astype(F64) - d).astype(F32)
    d32 = y_dev.astype(F32) - t
    return t, 2.0 * d32.astype(F64) / y_dev.size


# ---------------------------------------------------------------------------------------------------------------- Dense
ACTS = (None, 'sigmoid', 'relu', 'tanh')


def act_fwd(z, act):
    if act == 'sigmoid':
        return 1.0 / (1.0 + np.exp(-z))
    if act == 'relu':
        return np.maximum(z, 0.0)
    if act == 'tanh':
        return np.tanh(z)
    return z


def act_grad_from_output(y, act):
    """act'(z) written in terms of the output y, as the backward kernel evaluates it."""
    if act == 'sigmoid':
        return y * (1.0 - y)
    if act == 'relu':
        return (y > 0).astype(F64)
    if act == 'tanh':
        return 1.0 - y * y
    return np.ones_like(y)


def dense_forward(x, w, b, act):
    """x (R, Cin), w (Cin, F), b (F,) -> (pre-activation, y, bound on |y_dev - y|) in fp64; K = Cin (the bias starts the chain)."""
    x, w, b = (np.asarray(a, F64) for a in (x, w, b))
    z = x @ w + b
    y = act_fwd(z, act)
    return z, y, sum_bound(x.shape[1], np.abs(x) @ np.abs(w) + np.abs(b), y)


def dense_backward(x, w, y_dev, dy, act):
    """fp64 backward of the kernel's own operands: x, w, the float32 forward output y_dev (what dense_bwd_kernel reads for the
    activation derivative) and dy -> {name: (value, bound)} for dW (K = rows), db (K = rows), dX (K = F)."""
    x, w, y, dy = (np.asarray(a, F64) for a in (x, w, y_dev, dy))
    dz = dy * act_grad_from_output(y, act)
    rows, f = dz.shape
    dw, db, dx = x.T @ dz, dz.sum(axis=0), dz @ w.T
    return {'dW': (dw, sum_bound(rows, np.abs(x).T @ np.abs(dz), dw)),
            'db': (db, sum_bound(rows, np.abs(dz).sum(axis=0), db)),
            'dX': (dx, sum_bound(f, np.abs(dz) @ np.abs(w).T, dx)),
            'dz': (dz, None)}


# ---------------------------------------------------------------------------------------------------------------- GAP
def gap_forward(x, over_time):
    """x (N, T, H, W, C) fp64 -> mean over the pixels of a frame (N, T, C), or of a sample's frames too (N, C)."""
    return np.asarray(x, F64).mean(axis=(1, 2, 3) if over_time else (2, 3))


def gap_feat(x, w, b, relu):
    """The 1x1 Conv2D with bias in front of the pooling, fp64: (pre-activation, feat)."""
    z = np.asarray(x, F64) @ np.asarray(w, F64) + np.asarray(b, F64)
    return z, (np.maximum(z, 0.0) if relu else z)


def gap_backward(x, w, z, dys, over_time, relu):
    """dys: dL/d(pooled) of every pooling op that reads feat, each shaped (N, T, C) or (N, C).  dfeat = sum(dys) / HW where feat > 0
    (everywhere without the ReLU), else exactly 0; then db, dW, dX of the 1x1 convolution -> {name: (value, bound)}.  Each pooling's
    contribution is a term of its own in the bound (the second one is accumulated in fp32): K and sum|terms| count len(dys) per
    element of dfeat."""
    x, w = np.asarray(x, F64), np.asarray(w, F64)
    n, t, h, wd, cin = x.shape
    c = w.shape[1]
    hw = h * wd * (t if over_time else 1)
    parts = [np.broadcast_to(np.asarray(dy, F64).reshape((n, 1, 1, 1, c) if over_time else (n, t, 1, 1, c)) / hw, z.shape) for dy in dys]
    dfeat, dabs = sum(parts), sum(np.abs(p) for p in parts)
    if relu:
        dfeat, dabs = np.where(z > 0, dfeat, 0.0), np.where(z > 0, dabs, 0.0)
    xf, df, da = x.reshape(-1, cin), dfeat.reshape(-1, c), dabs.reshape(-1, c)
    rows = xf.shape[0] * len(dys)
    dw, db, dx = xf.T @ df, df.sum(axis=0), (df @ w.T).reshape(x.shape)
    return {'dW': (dw, sum_bound(rows, np.abs(xf).T @ da, dw)),
            'db': (db, sum_bound(rows, da.sum(axis=0), db)),
            'dX': (dx, sum_bound(c * len(dys), (da @ np.abs(w).T).reshape(x.shape), dx))}
