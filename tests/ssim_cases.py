"""Cases, launcher restatements and float64 references of tests/test_gpu_ssim.py (not a test module; needs no GPU).

csrc/dssim.hip picks its launch geometry from the array shape (N, H, W, C) alone:

  min/max      run_minmax: n = N H W C elements; nb = min(512, cdiv(n, 256)) blocks of minmax_kernel walk them with a grid stride (a
               second trip when n > 131072); minmax_finish_kernel reads the nb block results, thread k, k + 256, ... (a second trip
               when nb > 256)
  SSIM tiles   16 x 16 tiles over the (H - 10, W - 10) map (map_geom), forward: ssim_fwd_kernel, ms_ssim_kernel; 16 x 16 tiles over
               (H, W), backward: ssim_bwd_kernel, for the loss and for every pyramid level; one block per tile and plane
  compaction   compact_partials_kernel: 64 blocks, block g sums rows [g chunk, (g + 1) chunk) of the per-tile partials,
               chunk = cdiv(rows, 64), thread r, r + 256, ... (a second trip when rows > 16384)
  multi-scale  four scales, sizes halved upwards; ms_means_kernel: one wavefront per plane, lane k, k + 64, ... over the plane's tiles;
               ms_combine_kernel: one block, thread nc, nc + 256, ... over the N C planes; ms_apply_kernel: min(cdiv(n, 256), 2048)
               blocks; ms_pool_kernel / ms_unpool_add_kernel: min(cdiv(n, 256), 8192) blocks over the elements of the coarser / finer
               image; the compaction runs over the tiles of all four scales
  metrics      met_pair_partial_kernel: 64 chunks per pair of cdiv(H W C, 64) elements, thread e, e + 256, ...;
               met_pair_finish_kernel and met_assemble_kernel: blocks of 64 pairs; met_grid_kernel: min(cdiv(H W C, 256), 4096) blocks

tests/test_ssim_cases.py holds these restatements to the source text and the float64 restatements below to the oracle.
"""
import functools
import time
import zlib
from collections import namedtuple

import numpy as np

F32 = np.float32
KF, TS, COMPACT_G, MS_SCALES, MET_CHUNKS = 11, 16, 64, 4, 64
THREADS = 256
MM_CAP, MS_APPLY_CAP, MET_GRID_CAP, MS_EW_CAP = 512, 2048, 4096, 8192
MS_POWERS = (0.0448, 0.2856, 0.3001, 0.2363)

# the project's bounds (tests/test_gpu_ops.py: test_dssim_losses, test_msdssim_losses, test_image_metrics)
TOL_LOSS = dict(rel=2e-4, abs=1e-6)
TOL_GRAD = 1e-3                     # max error over max |reference|
TOL_PAIR = 2e-5                     # mae, mse, rmse, psnr, pearson
TOL_SSIM = 2e-4
TOL_MAP = dict(rtol=2e-4, atol=2e-6)
# The extremes are selected, not computed: the kernels and the float64 reference branch on the same float32 numbers, so only an exact
# zero or an exact tie could be read differently, and no case may hold one unless it is named for it
BRANCH_MARGIN = 0.0
TIE_NUDGE = 1e-9                    # float64 displacement that decides an exact tie the way the product (and TensorFlow) does


def cdiv(a, b):
    return -(-a // b)


def seed_of(name):
    return zlib.crc32(name.encode())


# ----------------------------------------------------------------------------------------------------------------- geometry
def mm_geom(n):
    nb = min(MM_CAP, cdiv(n, THREADS))
    return dict(nb=nb, trips=cdiv(n, nb * THREADS), finish_trips=cdiv(nb, THREADS))


def mm_trip(e, n):
    """which grid-stride trip of minmax_kernel reads element e"""
    return e // (mm_geom(n)['nb'] * THREADS)


def mm_block(e, n):
    """which block reads element e (minmax_finish_kernel reads block b on trip b // 256)"""
    return (e // THREADS) % mm_geom(n)['nb']


def map_size(H, W):
    return H - KF + 1, W - KF + 1


def tiles_fwd(H, W):
    return cdiv(W - KF + 1, TS), cdiv(H - KF + 1, TS)          # tiles_x, tiles_y


def tiles_bwd(H, W):
    return cdiv(W, TS), cdiv(H, TS)


def compact_geom(rows):
    chunk = cdiv(rows, COMPACT_G)
    return dict(chunk=chunk, trips=cdiv(chunk, THREADS))


def compact_second_trip_rows(rows):
    """row indices that compact_partials_kernel reads on its second and later trips"""
    chunk = compact_geom(rows)['chunk']
    r = np.arange(rows)
    return r[(r % chunk) >= THREADS]


def dssim_geom(shape):
    N, H, W, C = shape
    n = N * H * W * C
    nbf = N * C * int(np.prod(tiles_fwd(H, W)))
    nbb = N * C * int(np.prod(tiles_bwd(H, W)))
    return dict(n=n, mm=mm_geom(n), nbf=nbf, nbb=nbb, compact_fwd=compact_geom(nbf), compact_bwd=compact_geom(nbb))


def pyramid(H, W):
    dims = [(H, W)]
    for _ in range(1, MS_SCALES):
        dims.append(((dims[-1][0] + 1) // 2, (dims[-1][1] + 1) // 2))
    return dims


def ew_blocks(n):
    return max(1, min(cdiv(n, THREADS), MS_EW_CAP))


def ms_geom(shape):
    N, H, W, C = shape
    dims = pyramid(H, W)
    NC = N * C
    n = [N * h * w * C for h, w in dims]
    tiles = [int(np.prod(tiles_fwd(h, w))) for h, w in dims]
    gcp_total = NC * sum(tiles)
    nba = min(cdiv(n[0], THREADS), MS_APPLY_CAP)
    return dict(dims=dims, NC=NC, n=n, tiles=tiles, gcp_total=gcp_total, compact=compact_geom(gcp_total), mm=mm_geom(n[0]),
                combine_trips=cdiv(NC, THREADS), means_trips=[cdiv(t, 64) for t in tiles], nba=nba,
                apply_trips=cdiv(n[0], nba * THREADS),
                pool_trips=[cdiv(n[k], ew_blocks(n[k]) * THREADS) for k in range(1, MS_SCALES)],          # over the coarser image
                unpool_trips=[cdiv(n[k], ew_blocks(n[k]) * THREADS) for k in range(MS_SCALES - 1)])       # over the finer image


def met_geom(shape):
    N, H, W, C = shape
    per = H * W * C
    chunk = cdiv(per, MET_CHUNKS)
    blocks = min(cdiv(per, THREADS), MET_GRID_CAP)
    has_ssim = H >= KF and W >= KF
    tiles = int(np.prod(tiles_fwd(H, W))) if has_ssim else 0
    return dict(per=per, chunk=chunk, partial_trips=cdiv(chunk, THREADS), empty_chunks=MET_CHUNKS - cdiv(per, chunk),
                pair_blocks=cdiv(N, 64), grid_blocks=blocks, grid_trips=cdiv(per, blocks * THREADS), has_ssim=has_ssim, tiles=tiles,
                means_trips=cdiv(tiles, 64), mm=mm_geom(N * per))


# -------------------------------------------------------------------------------------------------------------- loss cases
# variant: how the extremes are set.  'positive': no shift, the targets set the range; 'negative_min': both minima negative, the
# prediction's the lower (shift and the lower end of the range reach the prediction); 'pred_sets_range': the prediction holds a
# 3.0 and a -1.0 (both ends of the range and the shift); 'late_extremes': the same two values at the flat indices LATE[id]
# grad: False asks for the loss alone (a null gradient pointer) and compares the loss alone
LossCase = namedtuple('LossCase', 'id kind shape variant grad', defaults=(True,))

TILE_SHAPES = [(1, 11, 11, 1), (2, 11, 27, 3), (1, 26, 16, 1), (1, 27, 17, 2), (3, 12, 43, 1), (1, 16, 33, 1), (1, 26, 13, 3)]
_VARIANTS = ('pred_sets_range', 'negative_min', 'positive')


def _sid(shape):
    return 'x'.join(str(v) for v in shape)


TILE_CASES = [LossCase(f'tile-dssim-{_sid(s)}', 'dssim', s, _VARIANTS[i % 3]) for i, s in enumerate(TILE_SHAPES)]
TILE_CASES += [LossCase(f'tile-{k}-{_sid(s)}', k, s, v) for k in ('dssim_mae', 'dssim_mse', 'dssim_mae_mse')
               for s, v in (((2, 11, 27, 3), 'pred_sets_range'), ((1, 27, 17, 2), 'negative_min'))]

LONG_CASES = [LossCase('long-minmax', 'dssim', (1200, 11, 11, 1), 'late_extremes'),
              LossCase('long-compact', 'dssim', (20000, 11, 11, 1), 'late_extremes')]
# (flat index of the prediction's maximum, of its minimum): the minimum is the last element; the maximum lies in a block that
# minmax_finish_kernel reads on its second trip -- and, where the array is long enough, that minmax_kernel reads on a late trip
LATE = {'long-minmax': (100000, 1200 * 121 - 1), 'long-compact': (10 * 131072 + 100000, 20000 * 121 - 1)}

# ms-pool: the coarser image of the first pooling step must exceed 8192 x 256 elements, N ceil(81 / 2)^2 > 2097152: N >= 1248; at
# 1260 the second trip writes 13 samples, enough to move the loss of the batch by 10 x its bound (tests/test_ssim_cases.py)
MS_CASES = [LossCase('ms-min', 'msdssim', (1, 81, 81, 1), 'pred_sets_range'),
            LossCase('ms-even-c2', 'msdssim', (2, 81, 88, 2), 'negative_min'),
            LossCase('ms-tiles81', 'msdssim', (1, 150, 139, 1), 'pred_sets_range'),
            LossCase('ms-long', 'msdssim', (530, 81, 81, 1), 'pred_sets_range'),
            LossCase('ms-pool', 'msdssim', (1260, 81, 81, 1), 'negative_min', False),
            LossCase('ms-mix-even', 'msdssim_mae_mse', (1, 88, 88, 1), 'negative_min')]

SCALES = (0.25, 100.0)
SCALE_CASES = [LossCase(f'scale-{k}-{v}', k, s, v) for k, s in (('dssim_mae_mse', (2, 27, 17, 1)), ('msdssim_mae', (1, 81, 88, 1)))
               for v in ('negative_min', 'pred_sets_range')]
NULL_GRAD_CASES = [LossCase('null-dssim_mae', 'dssim_mae', (2, 11, 27, 3), 'pred_sets_range'),
                   LossCase('null-msdssim', 'msdssim', (1, 81, 81, 1), 'negative_min')]
ACCUMULATE_CASES = [LossCase('acc-dssim_mae_mse', 'dssim_mae_mse', (2, 27, 17, 1), 'pred_sets_range'),
                    LossCase('acc-dssim', 'dssim', (1, 11, 11, 1), 'negative_min'),
                    LossCase('acc-msdssim_mae', 'msdssim_mae', (1, 81, 88, 1), 'pred_sets_range')]

# routing edges of the scalar fix-ups on one shape; the entries: what is written into y_true / y_pred at the flat indices
# (R_TRUE, R_PRED, R_PRED2) of otherwise tame arrays (targets in [0.1, 0.9), predictions within 0.04 of them), and which exact tie
# the reference decides with TIE_NUDGE: ('true', 'max' | 'min') moves the target's extreme outwards (tf.maximum / tf.minimum hand a
# tie to their first argument, y_true: the prediction gets nothing), ('pred', ...) moves the prediction's first tied extreme outwards
ROUTE_SHAPE = (2, 27, 17, 1)
R_TRUE, R_PRED, R_PRED2, R_LAST = 333, 150, 700, 2 * 27 * 17 - 1
Route = namedtuple('Route', 'id true pred tie', defaults=({}, {}, None))
ROUTE_CASES = [Route('max-equal', {R_TRUE: 1.5}, {R_PRED: 1.5}, ('true', 'max')),
               Route('min-equal', {R_TRUE: -0.25}, {R_PRED: -0.25}, ('true', 'min')),
               Route('true-neg-pred-pos', {R_TRUE: -0.5}, {}),
               Route('pred-neg-true-pos', {}, {R_PRED: -0.5}),
               Route('pred-min-zero', {}, {R_PRED: 0.0}),
               Route('last-max', {}, {R_LAST: 2.0}),
               Route('last-min', {}, {R_LAST: -0.5}),
               Route('tied-max', {}, {R_PRED: 2.0, R_PRED2: 2.0}, ('pred', 'max')),
               Route('tied-min', {}, {R_PRED: -0.5, R_PRED2: -0.5}, ('pred', 'min'))]

LOSS_CASES = TILE_CASES + LONG_CASES + MS_CASES + SCALE_CASES + NULL_GRAD_CASES + ACCUMULATE_CASES

# Field classes: what the values do to the float32 moments, at the smallest shapes (the window is 11 x 11 whatever the grid).  A
# 'smooth' field is a sum of low-wavenumber cosines with 1 / (k^2 + l^2) amplitudes, rescaled over the whole array to [0, 1].
#   class          target                          prediction                                mean / drange
#   smooth01       smooth                          target + 0.02 N(0,1)                      0.5
#   smooth-err     smooth                          target + 0.05 x another smooth field      0.5
#   kelvin         280 + 40 (smooth - 0.5)         target + 0.5 N(0,1)                       6.6     no shift is taken
#   pascal         101325 + 600 (smooth - 0.5)     target + 15 N(0,1)                        150
#   offset1000     1000 + U[0,1)                   target + 0.1 N(0,1)                       600
#   celsius        -30 + 40 smooth                 target + 0.5 N(0,1), one element -32      both arrays shifted, the prediction lower
#   mixed-sign     30 + 10 smooth                  target + 0.2 N(0,1), one element -2       0.8     only the prediction is shifted
#   near-constant  0.5 everywhere                  0.5 + 0.01 N(0,1)
#   constant-both  0.25 everywhere                 0.75 everywhere                           every window variance is 0: cs = 1 exactly
#   identical      smooth                          the target, bit for bit                   loss 0, gradient 0
#   scale1e4, scale1e-3   the smooth01 pair times 1e4, 1e-3 (c1, c2 scale with drange^2; the gradient with 1 / scale)
# kelvin, pascal and offset1000 stand at the offsets they are named for: the pivoted float32 restatement (loss32 with pivot=True)
# holds a quarter of TOL_LOSS / TOL_GRAD there -- loss 3.3e-2, 7.8e-3, 7.3e-3 of its bound, gradient 3.3e-2, 3.5e-3, 7.7e-4 of its
# bound (tests/test_ssim_cases.py prints every figure).  mixed-sign: at an offset of 50 the restatement's gradient stood at 0.27 of
# its bound in one entry of the multi-scale case, the one that takes the min-shift term (a sum over all entries that cancels to the
# size of one of them); at 30 it is 0.15, and the mean is still 0.8 of a dynamic range that the one negative element sets.
# constant-both: the two constants differ, so the luminance term is 0.6, the loss 0.2 and the gradient that of the luminance -- it
# is compared like any other case.  Every element of its prediction is the maximum: the reference decides the tie the product's way
# (TIE_NUDGE on the first element), as the routing cases do.
# identical: the float64 gradient is rounding-small (below 1e-16 here); the bound of the GPU test is 10 x the largest gradient entry
# of the pivoted float32 restatement on the same input, IDENTICAL_GRAD32 (test_ssim_cases.py holds it below 1e-3 of smooth01's).
FIELD_SHAPES = {'dssim': (2, 27, 43, 1), 'dssim_mae_mse': (1, 27, 17, 2), 'msdssim': (1, 81, 88, 1), 'msdssim_mae': (2, 81, 81, 1)}
FIELD_CLASSES = ('smooth01', 'smooth-err', 'kelvin', 'pascal', 'offset1000', 'celsius', 'mixed-sign', 'near-constant',
                 'constant-both', 'identical', 'scale1e4', 'scale1e-3')
OFFSET_CLASSES = ('kelvin', 'pascal', 'offset1000', 'near-constant')          # raw float32 moments miss the bounds here
ZERO_GRAD_CLASSES = ('identical',)
_MIX_CLASSES = {'dssim_mae_mse': ('smooth01', 'kelvin', 'celsius', 'scale1e4'),
                'msdssim_mae': ('smooth01', 'pascal', 'mixed-sign', 'scale1e-3')}


def field_class(case):
    return case.variant[len('field:'):]


FIELD_CASES = [LossCase(f'field-{c}-{k}', k, FIELD_SHAPES[k], 'field:' + c) for c in FIELD_CLASSES for k in ('dssim', 'msdssim')]
FIELD_CASES += [LossCase(f'field-{c}-{k}', k, FIELD_SHAPES[k], 'field:' + c) for k, cs in _MIX_CLASSES.items() for c in cs]
FIELD_NULL_GRAD_CASE = LossCase('field-null-kelvin', 'dssim', FIELD_SHAPES['dssim'], 'field:kelvin', False)
FIELD_ACCUMULATE_CASE = LossCase('field-acc-kelvin', 'dssim_mae_mse', FIELD_SHAPES['dssim_mae_mse'], 'field:kelvin')
FIELD_WEIGHTED_CASE = LossCase('field-weighted-kelvin', 'dssim_mae', FIELD_SHAPES['dssim'], 'field:kelvin')
# the weighted case's mask: a block of zeros wide enough to hold whole windows (omega == 0 for 7 x 10 of them per sample)
FIELD_MASK_BLOCK = (slice(5, 22), slice(10, 30))


def smooth_field(r, shape, kmax=3):
    """float64 (N, H, W, C) in [0, 1] (both ends reached, over the whole array): per plane sum_{k,l <= kmax, (k,l) != (0,0)}
    a_kl cos(2 pi k y / H + phi) cos(2 pi l x / W + psi) / (k^2 + l^2), a_kl ~ N(0,1), phases uniform"""
    N, H, W, C = shape
    y, x = np.arange(H)[:, None] / H, np.arange(W)[None, :] / W
    f = np.zeros(shape)
    for n in range(N):
        for c in range(C):
            for k in range(kmax + 1):
                for l in range(kmax + 1):
                    if k or l:
                        a, phi, psi = r.standard_normal(), *(2 * np.pi * r.random(2))
                        f[n, :, :, c] += a / (k * k + l * l) * np.cos(2 * np.pi * k * y + phi) * np.cos(2 * np.pi * l * x + psi)
    return (f - f.min()) / (f.max() - f.min())


def _field_inputs(cid, shape, cls):
    # the scale classes hold the smooth01 pair of the same kind
    r = np.random.default_rng(seed_of(cid.replace(cls, 'smooth01') if cls.startswith('scale') else cid))
    noise = lambda sd: sd * r.standard_normal(shape)
    if cls in ('smooth01', 'scale1e4', 'scale1e-3'):
        yt = smooth_field(r, shape)
        yp = yt + noise(0.02)
        if cls != 'smooth01':
            s = F32({'scale1e4': 1e4, 'scale1e-3': 1e-3}[cls])
            yt, yp = yt.astype(F32) * s, yp.astype(F32) * s
    elif cls == 'smooth-err':
        yt = smooth_field(r, shape)
        yp = yt + 0.05 * smooth_field(r, shape)
    elif cls == 'kelvin':
        yt = 280.0 + 40.0 * (smooth_field(r, shape) - 0.5)
        yp = yt + noise(0.5)
    elif cls == 'pascal':
        yt = 101325.0 + 600.0 * (smooth_field(r, shape) - 0.5)
        yp = yt + noise(15.0)
    elif cls == 'offset1000':
        yt = 1000.0 + r.random(shape)
        yp = yt + noise(0.1)
    elif cls == 'celsius':
        yt = -30.0 + 40.0 * smooth_field(r, shape)
        yp = yt + noise(0.5)
        yp.reshape(-1)[int(r.integers(0, yt.size))] = -32.0
    elif cls == 'mixed-sign':
        yt = 30.0 + 10.0 * smooth_field(r, shape)
        yp = yt + noise(0.2)
        yp.reshape(-1)[int(r.integers(0, yt.size))] = -2.0
    elif cls == 'near-constant':
        yt = np.full(shape, 0.5)
        yp = yt + noise(0.01)
    elif cls == 'constant-both':
        yt, yp = np.full(shape, 0.25), np.full(shape, 0.75)
    elif cls == 'identical':
        yt = smooth_field(r, shape)
        yp = yt
    else:
        raise ValueError(cls)
    return yt.astype(F32), yp.astype(F32).copy()


@functools.lru_cache(maxsize=None)
def _loss_inputs(cid, shape, variant):
    if variant.startswith('field:'):
        yt, yp = _field_inputs(cid, shape, variant[len('field:'):])
        yt.setflags(write=False)
        yp.setflags(write=False)
        return yt, yp
    r = np.random.default_rng(seed_of(cid))
    yt = r.random(shape).astype(F32)
    yp = (yt + 0.1 * r.standard_normal(shape)).astype(F32)
    n = yt.size
    if variant == 'positive':
        yp = np.abs(yp) + F32(0.01)
    elif variant == 'negative_min':
        yp = yp - F32(0.3)
        yt = yt - F32(0.1)
    elif variant in ('pred_sets_range', 'late_extremes'):
        imax, imin = LATE[cid] if variant == 'late_extremes' else (int(r.integers(0, n // 2)), int(r.integers(n // 2, n)))
        yp.reshape(-1)[imax] = 3.0
        yp.reshape(-1)[imin] = -1.0
    else:
        raise ValueError(variant)
    yt.setflags(write=False)
    yp.setflags(write=False)
    return yt, yp


def loss_inputs(case):
    """-> (y_true, y_pred) float32, read-only, the same arrays on every call"""
    return _loss_inputs(case.id, case.shape, case.variant)


def preload(case):
    """small integers that an accumulate case finds in dpred"""
    return np.random.default_rng(seed_of(case.id + '/preload')).integers(-3, 4, case.shape).astype(F32)


def field_preload(case):
    """The preload of the field accumulate case: multiples of 1/64 up to 3/64.  A Kelvin gradient is about 1e-3, so integers would
    round the sum at 2e-7, the size of the gradient's bound; these round it below a tenth of the bound and still exceed it 10 x
    (tests/test_ssim_cases.py)"""
    return preload(case) / F32(64)


@functools.lru_cache(maxsize=None)
def route_inputs(rid):
    route = next(c for c in ROUTE_CASES if c.id == rid)
    r = np.random.default_rng(seed_of(rid))
    yt = (0.1 + 0.8 * r.random(ROUTE_SHAPE)).astype(F32)
    yp = (yt + 0.04 * (2.0 * r.random(ROUTE_SHAPE) - 1.0)).astype(F32)
    for arr, entries in ((yt, route.true), (yp, route.pred)):
        for i, v in entries.items():
            arr.reshape(-1)[i] = v
    yt.setflags(write=False)
    yp.setflags(write=False)
    return yt, yp


# --------------------------------------------------------------------------------------------------------- loss references
def torch_loss(kind, yt, yp, grad=True):
    """oracle.torch_ops in float64 -> (loss, dloss/dpred or None, seconds)"""
    import torch
    from oracle import torch_ops as T
    t0 = time.perf_counter()
    t = torch.tensor(np.asarray(yp, np.float64), requires_grad=grad)
    with torch.set_grad_enabled(grad):
        lv = getattr(T, kind)(torch.tensor(np.asarray(yt, np.float64)), t)
    if grad:
        lv.backward()
    return float(lv.detach()), (t.grad.numpy() if grad else None), time.perf_counter() - t0


@functools.lru_cache(maxsize=None)
def _loss_ref(cid, kind, shape, variant, grad):
    yt, yp = _loss_inputs(cid, shape, variant)
    if variant == 'field:constant-both':          # every element is the maximum: the first one takes the range term, as in the product
        yp = np.asarray(yp, np.float64).copy()
        yp.reshape(-1)[0] += TIE_NUDGE
    return torch_loss(kind, yt, yp, grad=grad)


def loss_ref(case):
    return _loss_ref(case.id, case.kind, case.shape, case.variant, case.grad)


def _extreme_index(a, which):
    flat = np.asarray(a).reshape(-1)
    return int(np.argmax(flat) if which == 'max' else np.argmin(flat))          # the first one of a tie


@functools.lru_cache(maxsize=None)
def route_ref(rid, nudge=True):
    """Float64 reference of a routing case.  With ``nudge`` an exact tie is decided as the product decides it: torch.maximum
    halves the gradient of a tie where tf.maximum gives it to y_true, and torch's max() shares it among tied elements where
    the product gives it to the first."""
    route = next(c for c in ROUTE_CASES if c.id == rid)
    yt, yp = (np.asarray(a, np.float64).copy() for a in route_inputs(rid))
    if nudge and route.tie:
        side, which = route.tie
        arr = yp if side == 'pred' else yt
        arr.reshape(-1)[_extreme_index(arr, which)] += TIE_NUDGE if which == 'max' else -TIE_NUDGE
    return torch_loss('dssim', yt, yp)


# ----------------------------------------------------------------------- float64 restatements with their parts exposed
def ssim_maps(x, q, drange):
    """(luminance * contrast-structure, contrast-structure) maps (N, H - 10, W - 10, C) of tf.image.ssim, float64"""
    import torch
    from oracle import torch_ops as T
    x, q = torch.tensor(np.asarray(x, np.float64)), torch.tensor(np.asarray(q, np.float64))
    g = T._gauss_kernel(KF, 1.5, torch.float64)
    c1, c2 = (0.01 * drange) ** 2, (0.03 * drange) ** 2
    m0, m1 = T._valid_depthwise(x, g), T._valid_depthwise(q, g)
    num0, den0 = 2.0 * m0 * m1, m0 ** 2 + m1 ** 2
    lum = (num0 + c1) / (den0 + c1)
    cs = (2.0 * T._valid_depthwise(x * q, g) - num0 + c2) / (T._valid_depthwise(x * x + q * q, g) - den0 + c2)
    return (lum * cs).numpy(), cs.numpy()


def stats_of(yt, yp, keep=None):
    """(minT, maxT, minP, maxP) over the flat elements selected by ``keep`` (all of them by default)"""
    a, b = np.asarray(yt, np.float64).reshape(-1), np.asarray(yp, np.float64).reshape(-1)
    if keep is not None:
        a, b = a[keep], b[keep]
    return a.min(), a.max(), b.min(), b.max()


def shifted(yt, yp, stats):
    minT, maxT, minP, maxP = stats
    drange = max(maxT, maxP) - min(minT, minP)
    x = np.asarray(yt, np.float64) - (minT if minT < 0 else 0.0)
    q = np.asarray(yp, np.float64) - (minP if minP < 0 else 0.0)
    return x, q, drange


def dssim_value(yt, yp, stats=None, keep_tiles=None):
    """dssim restated: 1/2 - 1/2 sum S / count.  ``stats``: the extremes the kernel would hold (default: the true ones);
    ``keep_tiles``: boolean per (n, c, tile_y, tile_x) in the order of the forward launch -- tiles left out of sum S."""
    x, q, drange = shifted(yt, yp, stats or stats_of(yt, yp))
    s, _ = ssim_maps(x, q, drange)
    if keep_tiles is None:
        return 0.5 - 0.5 * s.mean()
    return 0.5 - 0.5 * (s * tile_mask(s.shape, keep_tiles)).sum() / s.size


def tile_mask(map_shape, keep_tiles):
    """map (N, Ho, Wo, C) mask from a flat boolean over blocks b = ((n C + c) tiles_y + ty) tiles_x + tx"""
    N, Ho, Wo, C = map_shape
    tx, ty = cdiv(Wo, TS), cdiv(Ho, TS)
    k = np.asarray(keep_tiles, bool).reshape(N, C, ty, tx)
    m = np.repeat(np.repeat(k, TS, axis=2), TS, axis=3)[:, :, :Ho, :Wo]
    return m.transpose(0, 2, 3, 1)


def _pool(x):
    from oracle import np_ops as N
    return N._downsample2_symmetric(x)


def ms_means(yt, yp, keep_tiles0=None):
    """per scale the (N, C) means of ssim and cs of the multi-scale loss, float64; ``keep_tiles0``: tiles of scale 0 that
    ms_means_kernel sums (boolean per block of the scale-0 launch)"""
    x, q, drange = shifted(yt, yp, stats_of(yt, yp))
    ms, mc = [], []
    for k in range(MS_SCALES):
        if k:
            x, q = _pool(x), _pool(q)
        s, cs = ssim_maps(x, q, drange)
        if k == 0 and keep_tiles0 is not None:
            m = tile_mask(s.shape, keep_tiles0)
            ms.append((s * m).sum(axis=(1, 2)) / (s.shape[1] * s.shape[2]))
            mc.append((cs * m).sum(axis=(1, 2)) / (s.shape[1] * s.shape[2]))
        else:
            ms.append(s.mean(axis=(1, 2)))
            mc.append(cs.mean(axis=(1, 2)))
    return ms, mc


def msdssim_value(means, keep_planes=None):
    """ms_combine_kernel restated: 1/2 - 1/2 sum_nc ms[n, c] / (N C); ``keep_planes``: boolean per plane n C + c"""
    ms, mc = means
    v = [np.maximum(mc[k], 0.0) for k in range(MS_SCALES - 1)] + [np.maximum(ms[MS_SCALES - 1], 0.0)]
    prod = np.prod([v[k] ** MS_POWERS[k] for k in range(MS_SCALES)], axis=0)          # (N, C)
    if keep_planes is not None:
        prod = prod * np.asarray(keep_planes, bool).reshape(prod.shape)
    return 0.5 - 0.5 * prod.sum() / prod.size


# ------------------------------------------------------------------------------------------------------------ metric cases
# const: None | 'n1' (one pair) | 'point' (grid point MET_CONST_POINT holds one value in every pair, both arrays) |
#        'pair' (pair 1: constant target; pair 2: constant prediction) | 'tail' (the elements beyond 256 of every pair chunk hold
#        the target mirrored at the mean: without them the per-pair Pearson moves, not only MAE and MSE)
# ssim: the per-pair SSIM is compared at TOL_SSIM -- every case with an 11 x 11 window, the offset data included (the window moments
#        are pivoted like the losses'); the float64 SSIM of the constant pairs is finite (c2 keeps the structure term defined)
MetCase = namedtuple('MetCase', 'id shape mean sd ssim const', defaults=(True, None))
MET_OFFSETS = ((280.0, 5.0), (280.0, 1.0), (1000.0, 1.0), (101325.0, 300.0))
MET_OFFSET_CASES = [MetCase(f'offset-{m:g}-{s:g}-{_sid(shape)}', shape, m, s, True)
                    for m, s in MET_OFFSETS for shape in ((3, 32, 32, 1), (2, 64, 64, 1))]
MET_SHAPE_CASES = [MetCase('pairs65', (65, 12, 11, 1), 1.0, 2.0), MetCase('pairs130-c2', (130, 11, 13, 2), 1.0, 2.0),
                   MetCase('chunk258', (2, 129, 128, 1), 1.0, 2.0, True, 'tail'), MetCase('tiles81', (1, 150, 139, 1), 1.0, 2.0),
                   MetCase('grid-trip', (2, 1024, 1025, 1), 1.0, 2.0), MetCase('empty-chunks', (3, 5, 6, 1), 1.0, 2.0),
                   MetCase('no-window', (2, 20, 9, 1), 1.0, 2.0)]
MET_DEGENERATE_CASES = [MetCase('one-pair', (1, 14, 12, 1), 1.0, 2.0, True, 'n1'),
                        MetCase('const-point', (5, 12, 13, 1), 280.37, 2.0, True, 'point'),
                        MetCase('const-pair', (4, 13, 12, 1), 280.37, 2.0, True, 'pair')]
MET_CASES = MET_OFFSET_CASES + MET_SHAPE_CASES + MET_DEGENERATE_CASES
MET_CONST_POINT = (3, 7, 0)


@functools.lru_cache(maxsize=None)
def _met_inputs(cid, shape, mean, sd, const):
    r = np.random.default_rng(seed_of(cid))
    y = (r.standard_normal(shape) * sd + mean).astype(F32)
    p = (y + 0.3 * sd * r.standard_normal(shape)).astype(F32)
    if const == 'point':
        y[(slice(None),) + MET_CONST_POINT] = y[(0,) + MET_CONST_POINT]
        p[(slice(None),) + MET_CONST_POINT] = p[(0,) + MET_CONST_POINT]
    elif const == 'tail':
        tail = (np.arange(y[0].size) % met_geom(shape)['chunk']) >= THREADS
        p.reshape(shape[0], -1)[:, tail] = F32(2.0 * mean) - y.reshape(shape[0], -1)[:, tail]
    elif const == 'pair':
        y[1] = y[1, 0, 0, 0]
        p[2] = p[2, 0, 0, 0]
    y.setflags(write=False)
    p.setflags(write=False)
    return y, p


def met_inputs(case):
    return _met_inputs(case.id, case.shape, case.mean, case.sd, case.const)


@functools.lru_cache(maxsize=None)
def _met_ref(cid, shape, mean, sd, const):
    from oracle import np_ops as N
    t0 = time.perf_counter()
    with np.errstate(invalid='ignore', divide='ignore'):
        ref = N.image_metrics(*_met_inputs(cid, shape, mean, sd, const))
    return ref, time.perf_counter() - t0


def met_ref(case):
    """oracle.np_ops.image_metrics in float64 -> (dict, seconds)"""
    return _met_ref(case.id, case.shape, case.mean, case.sd, case.const)


# the arithmetic of the pair sums, restated to show what the float partials do (tests/test_ssim_cases.py)
def pair_pearson_sim(y, p, pivot):
    """Per-pair Pearson as met_pair_partial_kernel + met_pair_finish_kernel compute it: 64 chunks, double sums, each chunk's
    sums stored as float32, double finish.  ``pivot``: subtract the pair's first elements before the products."""
    n = y.shape[0]
    a, b = np.asarray(y, np.float64).reshape(n, -1), np.asarray(p, np.float64).reshape(n, -1)
    if pivot:
        a, b = a - a[:, :1], b - b[:, :1]
    per = a.shape[1]
    chunk = cdiv(per, MET_CHUNKS)
    s = np.zeros((5, n))
    for c in range(cdiv(per, chunk)):
        x, z = a[:, c * chunk:(c + 1) * chunk], b[:, c * chunk:(c + 1) * chunk]
        for k, v in enumerate((x, z, x * z, x * x, z * z)):
            s[k] += v.sum(1).astype(F32).astype(np.float64)
    mx, my = s[0] / per, s[1] / per
    cov, vx, vy = s[2] / per - mx * my, s[3] / per - mx * mx, s[4] / per - my * my
    return cov / np.sqrt(np.maximum(vx * vy, 1e-300))


# --------------------------------------------------------------- float32 restatements of the loss kernels' arithmetic
# What float32 does to the window moments, in numpy float32 with the separable 11-tap filter in the kernels' order (row pass over
# W, taps ascending, then the column pass over H; reductions over windows in float64, as the kernels' compaction has them).
#   pivot=False  the moments of the shifted values themselves: sigma = E[x^2] - mu^2 cancels at the size of the mean
#   pivot=True   the moments of t - pT, p - pP (the means of the two arrays, rounded to float32); the pivots come back only in the
#                luminance term, mu = (pT - shift) + mu'; the backward combines the same pivoted pixels with the transposed maps
def gauss32():
    c = np.arange(KF) - (KF - 1) / 2.0
    g = np.exp(-c * c / (2.0 * 1.5 * 1.5)).astype(F32)
    return (g / g.astype(np.float64).sum()).astype(F32)


def _sep32(a, g):
    """VALID separable filter of a float32 (N, H, W, C) array"""
    Ho, Wo = a.shape[1] - KF + 1, a.shape[2] - KF + 1
    r = np.zeros(a[:, :, :Wo].shape, F32)
    for j in range(KF):
        r += g[j] * a[:, :, j:j + Wo]
    o = np.zeros(r[:, :Ho].shape, F32)
    for i in range(KF):
        o += g[i] * r[:, i:i + Ho]
    return o


def _sep32_t(s, g):
    """transposed filter of a float32 map (N, Ho, Wo, C) -> (N, Ho + 10, Wo + 10, C): T[y, x] = sum g[i] g[j] s[y - i, x - j]"""
    k = KF - 1
    pad = np.pad(s, ((0, 0), (k, k), (k, k), (0, 0)))
    H, W = s.shape[1] + k, s.shape[2] + k
    r = np.zeros(pad[:, :, :W].shape, F32)
    for j in range(KF):
        r += g[j] * pad[:, :, k - j:k - j + W]
    o = np.zeros(r[:, :H].shape, F32)
    for i in range(KF):
        o += g[i] * r[:, k - i:k - i + H]
    return o


def _pool32(a):
    """2 x 2 average, an odd edge row / column repeated; the sum in the kernel's order"""
    if a.shape[1] % 2:
        a = np.concatenate([a, a[:, -1:]], axis=1)
    if a.shape[2] % 2:
        a = np.concatenate([a, a[:, :, -1:]], axis=2)
    return F32(0.25) * (((a[:, 0::2, 0::2] + a[:, 0::2, 1::2]) + a[:, 1::2, 0::2]) + a[:, 1::2, 1::2])


def _unpool32(fine_shape, coarse):
    """adjoint of _pool32: every source gets a quarter, the repeated edge counts twice"""
    _, Hs, Ws, _ = fine_shape
    up = np.repeat(np.repeat(coarse, 2, axis=1), 2, axis=2)[:, :Hs, :Ws]
    wy, wx = np.ones(Hs, F32), np.ones(Ws, F32)
    if Hs % 2:
        wy[-1] = 2.0
    if Ws % 2:
        wx[-1] = 2.0
    return F32(0.25) * wy[None, :, None, None] * wx[None, None, :, None] * up


def _maps32(xs, qs, oT, oP, c1, c2, g):
    """per-window terms of one scale from the staged (pivoted or shifted) images; oT, oP: what the luminance adds to their means"""
    mxs, mys = _sep32(xs, g), _sep32(qs, g)
    A, Bq = _sep32(xs * qs, g), _sep32(xs * xs + qs * qs, g)
    mx, my = oT + mxs, oP + mys
    N1, D1 = F32(2) * mx * my + c1, mx * mx + my * my + c1
    N2, D2 = F32(2) * A - F32(2) * mxs * mys + c2, Bq - mxs * mxs - mys * mys + c2
    lum, cs = N1 / D1, N2 / D2
    dlum = F32(2) * mx / D1 - N1 * F32(2) * my / (D1 * D1)
    dcs = -F32(2) * mxs / D2 + N2 * F32(2) * mys / (D2 * D2)
    return dict(lum=lum, cs=cs, dlum=dlum, dcs=dcs, D1=D1, N1=N1, D2=D2, N2=N2)


def _stage32(yt, yp, pivot):
    """-> staged images, luminance offsets, drange, and the float32 extremes"""
    yt, yp = np.asarray(yt, F32), np.asarray(yp, F32)
    minT, maxT, minP, maxP = yt.min(), yt.max(), yp.min(), yp.max()
    shT, shP = (minT if minT < 0 else F32(0)), (minP if minP < 0 else F32(0))
    drange = F32(max(maxT, maxP)) - F32(min(minT, minP))
    if pivot:
        pT, pP = F32(yt.astype(np.float64).mean()), F32(yp.astype(np.float64).mean())
    else:
        pT, pP = shT, shP
    return (pT, pP), (F32(pT - shT), F32(pP - shP)), drange, (minT, maxT, minP, maxP)


def _fixups32(grad, yp, ext, drange, gc1, gc2):
    minT, maxT, minP, maxP = ext
    ddr = F32(gc1 * 2.0 * 0.01 * 0.01) * drange + F32(gc2 * 2.0 * 0.03 * 0.03) * drange
    sumdy = F32(grad.astype(np.float64).sum())
    flat, p = grad.reshape(-1), np.asarray(yp).reshape(-1)
    if maxP > maxT:
        flat[int(p.argmax())] += ddr
    if minP < minT:
        flat[int(p.argmin())] -= ddr
    if minP < 0:
        flat[int(p.argmin())] -= sumdy
    return grad


def dssim32(yt, yp, pivot):
    """(loss, dloss/dpred) of the single-scale kernels' arithmetic"""
    g = gauss32()
    (pT, pP), (oT, oP), drange, ext = _stage32(yt, yp, pivot)
    c1, c2 = (F32(0.01) * drange) ** 2, (F32(0.03) * drange) ** 2
    xs, qs = np.asarray(yt, F32) - pT, np.asarray(yp, F32) - pP
    m = _maps32(xs, qs, oT, oP, c1, c2, g)
    S = m['lum'] * m['cs']
    inv_m = F32(1.0 / S.size)
    loss = F32(0.5) - F32(0.5) * F32(S.astype(np.float64).sum()) * inv_m
    vmu = m['cs'] * m['dlum'] + m['lum'] * m['dcs']
    va, vb = m['lum'] * F32(2) / m['D2'], -m['lum'] * m['N2'] / (m['D2'] * m['D2'])
    gc1 = (m['cs'] * (m['D1'] - m['N1']) / (m['D1'] * m['D1'])).astype(np.float64).sum()
    gc2 = (m['lum'] * (m['D2'] - m['N2']) / (m['D2'] * m['D2'])).astype(np.float64).sum()
    coef = F32(-0.5) * inv_m
    grad = coef * (_sep32_t(vmu, g) + xs * _sep32_t(va, g) + F32(2) * qs * _sep32_t(vb, g))
    return float(loss), _fixups32(grad, yp, ext, drange, float(coef) * gc1, float(coef) * gc2)


def msdssim32(yt, yp, pivot):
    """(loss, dloss/dpred) of the multi-scale kernels' arithmetic; the pyramid holds the staged (pivoted) images"""
    g = gauss32()
    (pT, pP), (oT, oP), drange, ext = _stage32(yt, yp, pivot)
    c1, c2 = (F32(0.01) * drange) ** 2, (F32(0.03) * drange) ** 2
    yt, yp = np.asarray(yt, F32), np.asarray(yp, F32)
    xs, qs = [yt - pT], [yp - pP]
    for k in range(1, MS_SCALES):
        if k == 1 and not pivot:          # the unpivoted kernels pool the raw values and take the shift off the average
            xs.append(_pool32(yt) - pT)
            qs.append(_pool32(yp) - pP)
        else:
            xs.append(_pool32(xs[-1]))
            qs.append(_pool32(qs[-1]))
    maps = [_maps32(xs[k], qs[k], oT, oP, c1, c2, g) for k in range(MS_SCALES)]
    mean = lambda a: (a.astype(np.float64).sum(axis=(1, 2), keepdims=True) * F32(1.0 / (a.shape[1] * a.shape[2]))).astype(F32)
    v = [np.maximum(mean(maps[k]['cs']), F32(0)) for k in range(MS_SCALES - 1)]
    v.append(np.maximum(mean(maps[-1]['lum'] * maps[-1]['cs']), F32(0)))
    pw = [F32(p) for p in MS_POWERS]
    ms = np.ones_like(v[0])
    for k in range(MS_SCALES):
        ms = ms * np.power(v[k], pw[k])
    NC = ms.size
    loss = F32(0.5) - F32(0.5) * F32(ms.astype(np.float64).sum() / NC)
    up = F32(-0.5) / F32(NC)
    grads, gc1, gc2 = [None] * MS_SCALES, 0.0, 0.0
    for k in range(MS_SCALES - 1, -1, -1):
        m = maps[k]
        with np.errstate(divide='ignore', invalid='ignore'):
            gk = np.where(v[k] > 0, up * pw[k] * ms / v[k], F32(0)).astype(F32)
        inv_m = F32(1.0) / (F32(m['cs'].shape[1]) * F32(m['cs'].shape[2]))
        ws, wc = (gk * inv_m, F32(0) * gk) if k == MS_SCALES - 1 else (F32(0) * gk, gk * inv_m)
        wl = ws * m['lum'] + wc
        dmu = ws * (m['cs'] * m['dlum'] + m['lum'] * m['dcs']) + wc * m['dcs']
        da, db = wl * F32(2) / m['D2'], -wl * m['N2'] / (m['D2'] * m['D2'])
        gc1 += (ws * m['cs'] * (m['D1'] - m['N1']) / (m['D1'] * m['D1'])).astype(np.float64).sum()
        gc2 += (wl * (m['D2'] - m['N2']) / (m['D2'] * m['D2'])).astype(np.float64).sum()
        grads[k] = _sep32_t(dmu, g) + xs[k] * _sep32_t(da, g) + F32(2) * qs[k] * _sep32_t(db, g)
        if k < MS_SCALES - 1:
            grads[k] = grads[k] + _unpool32(grads[k].shape, grads[k + 1])
    return float(loss), _fixups32(grads[0].astype(F32), yp, ext, drange, gc1, gc2)


def loss32(kind, yt, yp, pivot):
    """(loss, gradient) of any loss kind: the SSIM term in float32 as above, the pixel terms of the mixes in float64"""
    base = 'msdssim' if kind.startswith('msdssim') else 'dssim'
    lv, grad = (msdssim32 if base == 'msdssim' else dssim32)(yt, yp, pivot)
    mix = kind[len(base):]
    wd, wa, ws = {'': (1.0, 0.0, 0.0), '_mae': (0.8, 0.2, 0.0), '_mse': (0.8, 0.0, 0.2), '_mae_mse': (0.6, 0.2, 0.2)}[mix]
    d = np.asarray(yp, np.float64) - np.asarray(yt, np.float64)
    lv = wd * lv + wa * np.abs(d).mean() + ws * (d * d).mean()
    grad = wd * grad.astype(np.float64) + wa * np.sign(d) / d.size + ws * 2.0 * d / d.size
    return float(lv), grad


@functools.lru_cache(maxsize=None)
def field_sim(cid, pivot):
    """loss32 of a field case -> (loss, gradient)"""
    case = next(c for c in FIELD_CASES if c.id == cid)
    return loss32(case.kind, *loss_inputs(case), pivot)


def field_errors(case, pivot):
    """(loss error in units of its bound, gradient error over max |reference|) of the float32 restatement against float64"""
    ref, gref, _ = loss_ref(case)
    lv, grad = field_sim(case.id, pivot)
    tol = max(TOL_LOSS['rel'] * abs(ref), TOL_LOSS['abs'])
    return abs(lv - ref) / tol, np.abs(grad - gref).max() / max(np.abs(gref).max(), 1e-6)


def identical_grad32(case):
    """largest gradient entry of the pivoted restatement on a zero-gradient case: the yardstick of the GPU test"""
    return float(np.abs(field_sim(case.id, True)[1]).max())
