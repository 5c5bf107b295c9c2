"""Seeded cases of the exceedance verification, shared by tests/test_exceedance_api.py (which checks that the restatement is NaN
exactly where a case is built to be) and tests/test_gpu_exceedance.py (which runs them on the device).

Data kinds:
* 'relu'     max(z, 0) of standard normals, the kind of the existing ensemble tests: about half of all values are exactly 0, and
             every third of those zeros is written as -0.0.  Nothing is negative: at the thresholds 0.0 and -0.0 every member and
             every observation is an event (only a comparison that takes -0.0 for smaller than 0.0 would see anything else).
* 'deadzone' z where |z| > 0.5, else a zero with the sign of z: negatives, both zeros and positives; 0.0 is a threshold with events
             and non-events, and ties on both sides of it.
A case says per threshold what it is built to be: 'mixed' (events and non-events: every score is a number), 'all' (only events) /
'none' (no event): no uncertainty, so bss, roc_auc and one ROC coordinate are NaN; 'empty' (no valid element): everything is NaN.
A single element is never 'mixed'."""
import numpy as np

KS = (1, 2, 3, 17, 64, 65, 256)
# (shape, batch): one element; 5 samples of 207 cells in chunks of 2 (unaligned tails, several calls); whole 16-byte groups
SHAPES = (((1, 1), None), ((5, 207), 2), ((4, 1024), None))


def data(rng, kind, K, shape):
    """-> (members (K,) + shape, obs shape) float32"""
    z = rng.standard_normal((K + 1,) + tuple(shape))
    if kind == 'relu':
        z = np.maximum(z, 0.0)
        zero = np.flatnonzero(z.reshape(-1) == 0)
        z.reshape(-1)[zero[::3]] = -0.0
    elif kind == 'deadzone':
        z = np.where(np.abs(z) > 0.5, z, np.copysign(0.0, z))
    else:
        raise ValueError(kind)
    z = z.astype(np.float32)
    return z[:K], z[K]


def thresholds(T, kind, members):
    """-> (float32 thresholds (T,), what each is built to be on a field of many elements)"""
    pos = np.sort(members[members > 0.25].reshape(-1))
    dv = float(pos[len(pos) // 2]) if len(pos) else 0.5          # a value the data really takes: ties at the threshold
    zero = 'all' if kind == 'relu' else 'mixed'
    if T == 1:
        thr, what = [0.0], [zero]
    elif T == 3:
        thr, what = [dv, 0.0, 0.5], ['mixed', zero, 'mixed']
    elif T == 16:                                                  # any order, repeats, below the minimum, above the maximum
        thr = [0.5, -7.0, 0.0, 1e6, dv, 0.5, 0.25, 1.5, 0.75, -0.0, 2.0, 1.0, 0.125, dv, 1.25, 0.3]
        what = ['mixed', 'all', zero, 'none', 'mixed', 'mixed', 'mixed', 'mixed', 'mixed', zero, 'mixed', 'mixed', 'mixed', 'mixed',
                'mixed', 'mixed']
    else:
        raise ValueError(T)
    return np.asarray(thr, np.float32), what


def synthetic_cases():
    """-> list of dicts(name, K, shape, batch, kind, T, seed): every K at every shape, T cycling so that every shape sees 1, 3, 16"""
    out = []
    for i, K in enumerate(KS):
        for j, (shape, batch) in enumerate(SHAPES):
            T = (1, 3, 16)[(i + j) % 3]
            kind = 'deadzone' if (i + j) % 2 else 'relu'
            out.append(dict(name=f'K={K} {shape} T={T} {kind}', K=K, shape=shape, batch=batch, kind=kind, T=T, seed=3000 + 10 * K + j))
    return out


def build(case):
    """-> (members, obs, thr, what)"""
    rng = np.random.default_rng(case['seed'])
    m, y = data(rng, case['kind'], case['K'], case['shape'])
    thr, what = thresholds(case['T'], case['kind'], m)
    if int(np.prod(case['shape'])) == 1:
        what = ['single'] * len(what)
    return m, y, thr, what


def per_cell_case(K=17, shape=(5, 207), seed=41):
    """Threshold fields per cell: [0] a smooth positive field, [1] its first ten cells NaN, [2] NaN everywhere ('empty'), [3] 0.0
    with NaN in every seventh cell -> (members, obs, thr (4,) + shape[1:], what)"""
    rng = np.random.default_rng(seed)
    m, y = data(rng, 'deadzone', K, shape)
    s = shape[1:]
    f = (0.6 + 0.2 * rng.standard_normal(s)).astype(np.float32)
    thr = np.stack([f, f.copy(), np.full(s, np.nan, np.float32), np.zeros(s, np.float32)])
    thr[1].reshape(-1)[:10] = np.nan
    thr[3].reshape(-1)[::7] = np.nan
    return m, y, thr, ['mixed', 'mixed', 'empty', 'mixed']


def invalid_case(K=20, seed=5):
    """NaN / +-inf in the observation and in single members of (6, 8, 9, 1) fields, and a 2-D mask that drops row 5 ->
    (members, obs, mask2d, number of invalid elements before the mask)"""
    rng = np.random.default_rng(seed)
    m, y = data(rng, 'deadzone', K, (6, 8, 9, 1))
    y[0, 0, 0, 0] = np.nan
    y[1, 1, 1, 0] = -np.inf
    y[1, 1, 2, 0] = np.inf
    m[K - 1, 2, 2, 2, 0] = np.nan
    m[0, 3, 3, 3, 0] = np.inf
    m[K // 2, 3, 3, 4, 0] = -np.inf
    m[:, 4, 7, 8, 0] = np.nan
    mask = np.ones((8, 9))
    mask[5] = 0
    return m, y, mask, 7


def expected_nan(what, K):
    """Which scalar scores are NaN for a threshold built to be ``what``"""
    some = what != 'empty'
    mixed = what == 'mixed'
    return dict(base_rate=not some, brier=not some, reliability=not some, resolution=not some, uncertainty=not some,
                brier_fair=(not some) or K == 1, bss=not mixed, roc_auc=not mixed)
