"""Cases, launcher restatements and float64 references of tests/test_gpu_norm.py (not a test module; needs no GPU).

csrc/norm.hip and csrc/dwconv.hip pick their launch geometry from the pixel count and the channel count alone (for dense,
16-byte-aligned operands, which every DeviceArray and every graph buffer is):

  V            4 when C % 4 == 0, else 1 (vec_ok); CP = C / V channel packs
  LayerNorm    L = ln_lanes(CP) lanes share a pixel (power of two <= 64), lane j owns packs j, j + L, ...: slots = cdiv(CP, L) <= 4;
               a block holds gpb = 256 / L pixels, nb = ln_blocks = min(cdiv(npix, gpb), 1024) blocks walk the pixels with a
               grid stride (a second trip when npix > 1024 gpb); partial_reduce_kernel sums the nb slabs, lane b, b + 64, ...
  BatchNorm    bn_geom: R = 256 / CP pixel rows per block, want = min(1024, npix / (8 R) + 1), chunk = cdiv(npix, want),
               nb = cdiv(npix, chunk) blocks of ``chunk`` consecutive pixels (the last one short); wave_col_sum over the nb slabs
  depthwise    wgrad_geom on items = N H cdiv(W, 4) row segments of 4 pixels: CPB = min(CP, 36) packs per block,
               LANES = max(1, 256 / (7 CPB)), groups = cdiv(CP, CPB), want = min(512, items / (4 LANES) + 1),
               chunk = cdiv(items, want), nchunks = cdiv(items, chunk); dwconv_reduce_kernel sums the slabs, lane b, b + 64, ...

tests/test_norm_cases.py holds these restatements to the source text and the references written out here to oracle.torch_ops.
"""
import functools
import zlib
from collections import namedtuple

import numpy as np

F32 = np.float32
NORM_THREADS, NORM_KMAX, NORM_MAX_BLOCKS = 256, 4, 1024
DW_PW, DW_MAX_CHUNKS, DW_K = 4, 512, 7
RELU_MARGIN = 2e-4                 # tests/test_gpu_ops.py::untie: every float64 pre-activation keeps this distance from zero
BN_EPS, BN_MOMENTUM = 1e-3, 0.99
# max error over max |reference| (tests/test_gpu_ops.py: test_layernorm, test_batchnorm, test_depthwise_conv7)
TOL = {'ln': dict(y=1e-4, dx=1e-3, dgamma=1e-3, dbeta=1e-3),
       'bn': dict(y=2e-4, dx=1e-3, dgamma=1e-3, dbeta=1e-3),
       'dw': dict(y=2e-4, dx=2e-4, dk=1e-3, db=1e-3)}

# relu: the fused ReLU; acc: accumulate = 1 onto preloaded gradients; dx / dw: False passes null pointers (for the depthwise
# convolution ``dw`` False is a layer without bias, db == nullptr); hot: the pixels of the last chunk carry offsets of +-HOT
Case = namedtuple('Case', 'id shape relu acc dx dw hot', defaults=(False, False, True, True, False))
HOT = 8.0


def cdiv(a, b):
    return -(-a // b)


# ---------------------------------------------------------------------------------------------------------------- selection
def vec(C):
    return 4 if C % 4 == 0 else 1


def ln_lanes(CP):
    L = 1
    while L < CP and L < 64:
        L <<= 1
    return L


def ln_blocks(npix, L, max_blocks=NORM_MAX_BLOCKS):
    gpb = NORM_THREADS // L
    return max(1, min(max_blocks, cdiv(npix, gpb)))


def ln_select(shape):
    C = shape[-1]
    npix = int(np.prod(shape[:-1]))
    V = vec(C)
    CP = C // V
    L = ln_lanes(CP)
    gpb = NORM_THREADS // L
    nb = ln_blocks(npix, L)
    return dict(V=V, CP=CP, L=L, slots=cdiv(CP, L), gpb=gpb, nb=nb, npix=npix, trips=cdiv(npix, nb * gpb), first_trip=nb * gpb)


def bn_geom(npix, C):
    V = vec(C)
    CP = C // V
    R = NORM_THREADS // CP
    want = max(1, min(NORM_MAX_BLOCKS, npix // (R * 8) + 1))
    chunk = cdiv(npix, want)
    return dict(V=V, CP=CP, R=R, T=R * CP, chunk=chunk, nb=cdiv(npix, chunk), npix=npix)


def bn_select(shape):
    return bn_geom(int(np.prod(shape[:-1])), shape[-1])


def wgrad_geom(N, H, W, C):
    V = vec(C)
    CP = C // V
    items = N * H * cdiv(W, DW_PW)
    CPB = min(CP, 256 // DW_K)
    LANES = max(1, 256 // (CPB * DW_K))
    want = max(1, min(DW_MAX_CHUNKS, items // (LANES * 4) + 1))
    chunk = cdiv(items, want)
    return dict(V=V, CP=CP, CPB=CPB, LANES=LANES, groups=cdiv(CP, CPB), chunk=chunk, nchunks=cdiv(items, chunk), items=items,
                last_group=CP - (cdiv(CP, CPB) - 1) * CPB)


def dw_select(shape):
    return wgrad_geom(*shape)


def ln_features(case):
    s = ln_select(case.shape)
    f = {f'V{s["V"]}', f'L{s["L"]}', f'slots{s["slots"]}', f'form:V{s["V"]}/L{s["L"]}/slots{s["slots"]}'}
    if s['nb'] > 64:
        f.add('slabs>64')
    if s['trips'] > 1:
        f.add('second_trip')
        if s['L'] == 64 and s['V'] == 4:
            f.add('second_trip:L64/float4')
        if s['L'] == 64 and s['V'] == 1 and s['slots'] == 3:
            f.add('second_trip:L64/scalar/slots3')
        if s['L'] == 16:
            f.add('second_trip:L16')
    return f | _flag_features(case, s['V'])


def bn_features(case):
    g = bn_select(case.shape)
    f = {f'V{g["V"]}'}
    if g['nb'] > 64:
        f.add('slabs>64')
    if g['nb'] == NORM_MAX_BLOCKS and g['chunk'] > 8 * g['R']:
        f.add('capped')
        f.add(f'capped:V{g["V"]}')
        if g['V'] == 4 and g['CP'] > 128:
            f.add('capped:CP>128')
    if g['npix'] % g['chunk']:
        f.add('short_last_chunk')
    if g['npix'] == 1:
        f.add('npix1')
    if g['T'] < NORM_THREADS:
        f.add('idle_threads')
    return f | _flag_features(case, g['V'])


def dw_features(case):
    g = dw_select(case.shape)
    f = {f'V{g["V"]}'}
    if g['nchunks'] > 64:
        f.add('slabs>64')
    if g['nchunks'] == DW_MAX_CHUNKS:
        f.add('capped')
    if g['items'] % g['chunk']:
        f.add('short_last_chunk')
    if g['V'] == 1 and g['groups'] == 2 and g['last_group'] == 1:
        f.add('scalar:groups2:last_one_pack')
    if g['groups'] > 1:
        f.add('groups>1')
    if g['LANES'] > 1:
        f.add('lanes>1')
    if case.shape[2] % DW_PW:
        f.add('ragged_w')
    return f | _flag_features(case, g['V'], dw='null_db')


def _flag_features(case, V, dw='null_dw'):
    f = set()
    lay = 'float4' if V == 4 else 'scalar'
    relu = 'relu' if case.relu else 'linear'
    if case.acc:
        f |= {'acc', f'acc:{lay}', f'acc:{relu}'}
    if not case.dx:
        f |= {'null_dx', f'null_dx:{lay}', f'null_dx:{relu}'}
    if not case.dw:
        f |= {dw, f'{dw}:{lay}', f'{dw}:{relu}'}
    return f


# the forms tests/test_gpu_ops.py::NORM_SHAPES selects in ln_fwd / ln_bwd: (V, L, slots)
NORM_SHAPES = [(2, 9, 7, 3), (1, 16, 16, 64), (3, 5, 11, 20), (2, 4, 6, 130), (1, 33, 17, 256), (2, 3, 5, 1), (1, 8, 8, 1000)]

# ---------------------------------------------------------------------------------------------------------------- cases
# the accumulate and null-output forms, both lane layouts, with and without the fused ReLU (LayerNorm and BatchNorm alike)
FLAG_CASES = [
    Case('acc_v4', (2, 5, 7, 20), acc=True),                       # L = 8
    Case('acc_v4_relu', (1, 16, 16, 64), relu=True, acc=True),     # L = 16
    Case('acc_s', (2, 9, 7, 3), acc=True),                         # L = 4
    Case('acc_s_relu', (2, 4, 6, 130), relu=True, acc=True),       # L = 64, three slots
    Case('nodx_v4_relu', (1, 8, 8, 1000), relu=True, dx=False),    # L = 64, four slots
    Case('nodx_v4', (2, 5, 6, 24), dx=False),
    Case('nodx_s', (3, 5, 11, 5), dx=False),
    Case('nodx_s_relu', (2, 3, 7, 7), relu=True, dx=False),
    Case('nodw_v4', (2, 5, 7, 20), dw=False),
    Case('nodw_v4_relu', (1, 6, 5, 64), relu=True, dw=False),
    Case('nodw_s', (2, 4, 6, 130), dw=False),
    Case('nodw_s_relu', (2, 9, 7, 3), relu=True, dw=False),
    Case('acc_nodx_v4', (2, 5, 6, 24), acc=True, dx=False),        # acc_dw = 1 with a null dx
    Case('acc_nodw_s', (3, 5, 11, 5), acc=True, dw=False),         # acc_dx = 1 with null dgamma / dbeta
    Case('c1', (2, 3, 5, 1)),                                      # L = 1
    Case('c1_acc', (3, 4, 4, 1), acc=True),
    Case('c1000_acc', (1, 4, 5, 1000), acc=True),                  # L = 64, four slots
]
LN_CASES = FLAG_CASES + [
    Case('slabs141', (1, 33, 17, 256), relu=True),                 # nb = 141: three lane-strided trips over the slabs
    Case('trip2_v4', (1, 65, 64, 256)),                            # npix = 4160 > 1024 * 4: 64 pixels in a second trip
    Case('trip2_v4_slots2', (2, 33, 63, 512), relu=True, acc=True),    # npix = 4158, two slots
    Case('trip2_s3', (1, 65, 64, 130), relu=True),                 # scalar, three slots
    Case('trip2_s3_c131', (1, 64, 65, 131), acc=True),
    Case('trip2_l16', (1, 129, 128, 64)),                          # npix = 16512 > 1024 * 16: 128 pixels in a second trip
    Case('trip2_l16_c60', (3, 43, 128, 60), relu=True, dx=False),  # CP = 15
]
BN_CASES = FLAG_CASES + [
    Case('nb72', (1, 48, 48, 256)),                                # R = 4: nb = 72, chunk = 32
    Case('nb66_s', (1, 32, 33, 101), relu=True, acc=True),         # scalar, R = 2: nb = 66, chunk = 16
    Case('cap_s', (1, 96, 96, 130), hot=True),                     # R = 1: nb = 1024, chunk = 9
    Case('cap_s_short', (1, 95, 97, 130), relu=True, acc=True, hot=True),   # npix = 9215: the last chunk holds 8 pixels
    Case('cap_v4', (1, 95, 97, 516), hot=True),                    # float4, CP = 129: nb = 1024, chunk = 9, the last chunk 8 pixels
    Case('npix1_v4', (1, 1, 1, 8), relu=True),
    Case('npix1_s', (1, 1, 1, 5), acc=True),
]
DW_CASES = [
    Case('acc_v4', (2, 5, 7, 20), acc=True),
    Case('acc_s', (2, 9, 7, 3), acc=True),
    Case('nodx_v4', (1, 6, 6, 24), dx=False),
    Case('nodx_s', (1, 3, 2, 5), dx=False),
    Case('nodb_v4', (2, 5, 20, 20), dw=False),
    Case('nodb_s', (1, 6, 6, 130), dw=False),                      # scalar, four channel groups
    Case('acc_nodb_v4', (1, 7, 9, 8), acc=True, dw=False),
    Case('acc_nodx_s', (2, 4, 5, 6), acc=True, dx=False),
    Case('c37_small', (1, 5, 6, 37), acc=True),                    # scalar, CPB = 36: the second group is one pack wide
    Case('c37_nchunks65', (1, 20, 52, 37), hot=True),              # items = 260, LANES = 1: nchunks = 65
    Case('nchunks67', (2, 40, 40, 48), acc=True, hot=True),        # items = 800, LANES = 3: nchunks = 67, chunk = 12, the last 8
    Case('cap_v4', (1, 64, 128, 80), dx=False, hot=True),          # items = 2048, LANES = 1: nchunks = 512, chunk = 4
    Case('cap_s_short', (1, 36, 283, 21), dw=False, hot=True),     # items = 2556: nchunks = 512, chunk = 5, the last chunk 1 item
]
TABLES = {'ln': LN_CASES, 'bn': BN_CASES, 'dw': DW_CASES}
FEATURES_OF = {'ln': ln_features, 'bn': bn_features, 'dw': dw_features}
_FLAGS = ['acc', 'acc:float4', 'acc:scalar', 'acc:relu', 'acc:linear', 'null_dx', 'null_dx:float4', 'null_dx:scalar', 'null_dx:relu',
          'null_dx:linear']
_DW = ['null_dw', 'null_dw:float4', 'null_dw:scalar', 'null_dw:relu', 'null_dw:linear']
# every one of these is selected by at least two cases of its table
REQUIRED = {
    'ln': _FLAGS + _DW + ['slabs>64', 'second_trip:L64/float4', 'second_trip:L64/scalar/slots3', 'second_trip:L16']
          + sorted({'form:V{V}/L{L}/slots{slots}'.format(**ln_select(s)) for s in NORM_SHAPES}),
    'bn': _FLAGS + _DW + ['slabs>64', 'capped', 'capped:V1', 'short_last_chunk', 'npix1', 'V1', 'V4', 'idle_threads'],
    'dw': [f for f in _FLAGS if 'relu' not in f and 'linear' not in f] + ['null_db', 'null_db:float4', 'null_db:scalar', 'slabs>64',
                                                                        'capped', 'short_last_chunk',
                                                                        'scalar:groups2:last_one_pack', 'groups>1', 'lanes>1',
                                                                        'ragged_w'],
}
ONCE = {'bn': ['capped:V4', 'capped:CP>128']}          # "one float4 case with C / 4 > 128"

# what the named cases are there for: a subset of the restated geometry
EXPECT = {
    ('ln', 'slabs141'): dict(V=4, L=64, nb=141, trips=1),
    ('ln', 'trip2_v4'): dict(V=4, L=64, slots=1, nb=1024, trips=2, npix=4160, first_trip=4096),
    ('ln', 'trip2_v4_slots2'): dict(V=4, L=64, slots=2, nb=1024, trips=2),
    ('ln', 'trip2_s3'): dict(V=1, L=64, slots=3, nb=1024, trips=2),
    ('ln', 'trip2_s3_c131'): dict(V=1, L=64, slots=3, nb=1024, trips=2),
    ('ln', 'trip2_l16'): dict(V=4, L=16, slots=1, nb=1024, trips=2, npix=16512, first_trip=16384),
    ('ln', 'trip2_l16_c60'): dict(V=4, L=16, CP=15, nb=1024, trips=2),
    ('ln', 'c1'): dict(V=1, L=1, slots=1),
    ('ln', 'nodx_v4_relu'): dict(V=4, L=64, slots=4),
    ('bn', 'nb72'): dict(V=4, R=4, nb=72, chunk=32),
    ('bn', 'nb66_s'): dict(V=1, R=2, nb=66, chunk=16),
    ('bn', 'cap_s'): dict(V=1, R=1, nb=1024, chunk=9),
    ('bn', 'cap_s_short'): dict(V=1, R=1, nb=1024, chunk=9, npix=9215),
    ('bn', 'cap_v4'): dict(V=4, CP=129, R=1, nb=1024, chunk=9, npix=9215),
    ('bn', 'npix1_v4'): dict(npix=1, nb=1, chunk=1),
    ('bn', 'npix1_s'): dict(npix=1, nb=1, chunk=1),
    ('dw', 'c37_small'): dict(V=1, CPB=36, LANES=1, groups=2, last_group=1),
    ('dw', 'c37_nchunks65'): dict(V=1, CPB=36, LANES=1, groups=2, last_group=1, nchunks=65, chunk=4),
    ('dw', 'nchunks67'): dict(V=4, CPB=12, LANES=3, nchunks=67, chunk=12, items=800),
    ('dw', 'cap_v4'): dict(V=4, LANES=1, nchunks=512, chunk=4),
    ('dw', 'cap_s_short'): dict(V=1, LANES=1, nchunks=512, chunk=5, items=2556),
    ('dw', 'nodb_s'): dict(V=1, groups=4),
}


# ---------------------------------------------------------------------------------------------------------------- omissions
def _chunk_of_pixel(npix, chunk):
    return np.arange(npix) // chunk


def keep_masks(op, case):
    """-> {name: boolean mask over the pixels (row-major over all but the channel axis)} of what a kernel that loses part of its
    work would still add up: 'slabs' without the partial slabs of index >= 64, 'last_chunk' without the last chunk, 'trip'
    (LayerNorm) without the pixels of the second grid-stride trip.  Only the omissions the case's geometry has."""
    shape = case.shape
    npix = int(np.prod(shape[:-1]))
    out = {}
    if op == 'ln':
        s = ln_select(shape)
        p = np.arange(npix)
        block = (p // s['gpb']) % s['nb']
        if s['nb'] > 64:
            out['slabs'] = block < 64
        if s['trips'] > 1:
            out['trip'] = p < s['first_trip']
    elif op == 'bn':
        g = bn_select(shape)
        b = _chunk_of_pixel(npix, g['chunk'])
        if g['nb'] > 64:
            out['slabs'] = b < 64
        if g['nb'] > 1:
            out['last_chunk'] = b < g['nb'] - 1
    else:
        g = dw_select(shape)
        N, H, W, _ = shape
        WG = cdiv(W, DW_PW)
        item = (np.arange(N * H)[:, None] * WG + np.arange(W)[None, :] // DW_PW).reshape(-1)        # pixel -> work item
        b = item // g['chunk']
        if g['nchunks'] > 64:
            out['slabs'] = b < 64
        if g['nchunks'] > 1:
            out['last_chunk'] = b < g['nchunks'] - 1
    return out


# ---------------------------------------------------------------------------------------------------------------- inputs
def case_rng(name, salt=0):
    return np.random.default_rng(zlib.crc32(name.encode()) + salt)


def _offsets(rng, shape):
    """Order-one offsets with either sign: magnitude in [0.5, 1.5)."""
    return rng.choice([-1.0, 1.0], shape) * rng.uniform(0.5, 1.5, shape)


def untie(x, pre_fn, thr=RELU_MARGIN):
    """tests/test_gpu_ops.py::untie: move the inputs whose float64 pre-activation lies within ``thr`` of zero."""
    for _ in range(12):
        bad = np.abs(pre_fn(x.astype(np.float64))) < thr
        if not bad.any():
            return x
        x = x.copy()
        x[bad] += F32(0.03)
    raise AssertionError('could not remove the ReLU ties')


def preact(op, x, gamma, beta, eps):
    from oracle import np_ops as N
    x = np.asarray(x, np.float64)
    g, b = gamma.astype(np.float64), beta.astype(np.float64)
    if op == 'ln':
        return N.layer_norm(x, g, b, eps)
    mu, var = N.channel_moments(x)
    return N.batch_norm(x, g, b, mu, var, eps)


def _tail_pixels(op, case):
    """The pixels of the last chunk (what 'last_chunk' omits)."""
    keep = keep_masks(op, case).get('last_chunk')
    return None if keep is None else ~keep


@functools.lru_cache(maxsize=None)
def inputs(op, case, eps=1e-3):
    """-> dict of read-only float32 operands.  Norms: x, gamma, beta, dy, dyi (integers in [-4, 4]), xi (integers in [-4, 12]), mm,
    mv (moving statistics), pre = (dx0, dgamma0, dbeta0), prei (integer dbeta0).  Depthwise: x, k, b, dy, dyi, pre = (dx0, dk0, db0),
    prei.  x is unit noise on an offset per channel, its first pixel (BatchNorm's pilot) two units off.  dy is unit noise, for
    BatchNorm and the depthwise convolution on an offset per channel (a lost slab then moves mean(dy) and with it BatchNorm's dx);
    with ``case.hot`` it is the pixels of the last chunk that carry offsets instead, of +-HOT per channel in x and dy (a channel
    offset would bury them: the last chunk is 8 pixels of 9215).  The preloads have the root mean square of the float64
    gradients they are added to."""
    shape = case.shape
    C = shape[-1]
    rng = case_rng(f'{op}/{case.id}')
    x = rng.standard_normal(shape) + _offsets(rng, (C,))
    dy = rng.standard_normal(shape) + (0.0 if op == 'ln' or case.hot else _offsets(rng, (C,)))
    x.reshape(-1, C)[0] += 2.0 * rng.choice([-1.0, 1.0], C)
    if case.hot:
        tail = _tail_pixels(op, case)
        x.reshape(-1, C)[tail] += HOT * rng.choice([-1.0, 1.0], C)
        dy.reshape(-1, C)[tail] += HOT * rng.choice([-1.0, 1.0], C)
    x, dy = x.astype(F32), dy.astype(F32)
    d = dict(dy=dy, dyi=rng.integers(-4, 5, shape).astype(F32), xi=rng.integers(-4, 13, shape).astype(F32),
             prei=rng.integers(-4, 5, C).astype(F32))
    if op == 'dw':
        d['k'] = (rng.standard_normal((DW_K, DW_K, C, 1)) * 0.2).astype(F32)
        d['b'] = _offsets(rng, (C,)).astype(F32)
        d['x'] = x
        names = ('dx', 'dk', 'db')
    else:
        d['gamma'] = (1 + 0.2 * rng.standard_normal(C)).astype(F32)
        d['beta'] = (0.1 * rng.standard_normal(C)).astype(F32)
        d['mm'] = rng.standard_normal(C).astype(F32)
        d['mv'] = (0.5 + rng.random(C)).astype(F32)
        if case.relu and int(np.prod(shape[:-1])) > 1 and C > 1:
            x = untie(x, lambda v: preact(op, v, d['gamma'], d['beta'], eps))
        d['x'] = x
        names = ('dx', 'dgamma', 'dbeta')
    ref = reference(op, case, d, eps=eps, preload=False)
    d['pre'] = tuple((rng.standard_normal(ref[n].shape) * max(np.sqrt((ref[n] ** 2).mean()), 1e-3)).astype(F32) for n in names)
    for v in d.values():
        for a in (v if isinstance(v, tuple) else (v,)):
            a.setflags(write=False)
    return d


# ---------------------------------------------------------------------------------------------------------------- references
def _t64(a, grad=False):
    import torch
    return torch.tensor(np.asarray(a, np.float64), requires_grad=grad)


def reference(op, case, d, eps=1e-3, preload=True, dy=None, relu=None, keep=None, pre=None):
    """oracle.torch_ops in float64 with autograd -> dict(y, dx, dgamma | dk, dbeta | db [, mean, var]); the case's preloads added
    when it accumulates (``preload``; ``pre`` overrides the arrays).  ``keep``: a pixel mask; the sums over pixels (dgamma / dk,
    dbeta / db) then run over the kept pixels alone and LayerNorm's dx is left unwritten elsewhere -- exact for these ops, whose
    parameter gradients are linear in dy (for BatchNorm see ``bn_written_out``)."""
    import torch
    from oracle import torch_ops as T
    relu = case.relu if relu is None else relu
    dy = np.asarray(d['dy'] if dy is None else dy, np.float64)
    if keep is not None:
        assert op != 'bn'
        dy = dy * keep.reshape(case.shape[:-1] + (1,))
    xt = _t64(d['x'], True)
    if op == 'dw':
        kt, bt = _t64(d['k'], True), _t64(d['b'], True)
        y = T.depthwise_conv2d(xt, kt, bt if case.dw else None)
        names, params = ('dk', 'db'), (kt, bt)
    else:
        gt, bt = _t64(d['gamma'], True), _t64(d['beta'], True)
        if op == 'ln':
            y = T.layer_norm(xt, gt, bt, eps)
        else:
            mu, var = T.channel_moments(xt)
            y = T.batch_norm(xt, gt, bt, mu, var, eps)
        if relu:
            y = torch.relu(y)
        names, params = ('dgamma', 'dbeta'), (gt, bt)
    (y * _t64(dy)).sum().backward()
    out = dict(y=y.detach().numpy(), dx=xt.grad.numpy())
    for n, p in zip(names, params):
        out[n] = p.grad.numpy() if p.grad is not None else np.zeros(p.shape)
    if op == 'bn':
        out['mean'], out['var'] = mu.detach().numpy(), var.detach().numpy()
    if preload and case.acc:
        pre = d['pre'] if pre is None else pre
        for n, p in zip(('dx',) + names, pre):
            out[n] = out[n] + p.astype(np.float64).reshape(out[n].shape)
    return out


def bn_written_out(case, d, keep_stats=None, keep_bwd=None, eps=BN_EPS):
    """BatchNorm as csrc/norm.hip computes it, in float64: shifted sums about the pilot x[0][c] divided by the FULL pixel count,
    y = a x + b, dx = gamma invstd (de - mean(de) - xhat mean(de xhat)).  ``keep_stats`` / ``keep_bwd``: pixel masks of what the
    forward / backward sums still see (a kernel that loses slabs or a chunk divides by npix all the same).  No preload."""
    C = case.shape[-1]
    x = np.asarray(d['x'], np.float64).reshape(-1, C)
    dy = np.asarray(d['dy'], np.float64).reshape(-1, C)
    g, b = d['gamma'].astype(np.float64), d['beta'].astype(np.float64)
    n = x.shape[0]
    ks = np.ones(n, bool) if keep_stats is None else keep_stats
    kb = np.ones(n, bool) if keep_bwd is None else keep_bwd
    dev = x - x[0]
    m = dev[ks].sum(0) / n
    var = np.maximum((dev[ks] ** 2).sum(0) / n - m * m, 0.0)
    mean, inv = x[0] + m, 1.0 / np.sqrt(var + eps)
    y = (x - mean) * inv * g + b
    de = dy * (y > 0) if case.relu else dy
    if case.relu:
        y = np.maximum(y, 0.0)
    xh = (x - mean) * inv
    s1, s2 = (de * xh)[kb].sum(0), de[kb].sum(0)
    dx = g * inv * (de - s2 / n - xh * s1 / n)
    return dict(y=y.reshape(case.shape), dx=dx.reshape(case.shape), dgamma=s1, dbeta=s2, mean=mean, var=var)


def rel_err(got, ref):
    """max |got - ref| over max |ref|: the figure of tests/test_gpu_ops.py's close()."""
    ref = np.asarray(ref, np.float64)
    got = np.asarray(got, np.float64)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    return float(np.abs(got - ref).max() / max(np.abs(ref).max(), 1e-6))


def outputs(op, case):
    """The gradient outputs a case requests, by name."""
    names = ['dx'] if case.dx else []
    if op == 'dw':
        return names + ['dk'] + (['db'] if case.dw else [])
    return names + (['dgamma', 'dbeta'] if case.dw else [])


# ---------------------------------------------------------------------------------------------------------------- in-graph cases
# shape (B, H, W, C) or (B, T, H, W, C); kind 'ln' / 'bn'
GCase = namedtuple('GCase', 'id kind shape relu')
_G_SHAPES = [('v4', (2, 6, 10, 8)), ('s', (2, 7, 9, 5)), ('5d', (2, 3, 5, 6, 8))]
G_RESIDUAL = [GCase(f'{k}_{n}{"_relu" if r else ""}', k, s, r) for k in ('ln', 'bn') for n, s in _G_SHAPES for r in (False, True)]
G_SHARED = [GCase(f'{k}_{n}', k, s, r) for k in ('ln', 'bn') for (n, s), r in zip(_G_SHAPES, (True, False, True))]
G_FIRST = [GCase(f'{k}_{n}', k, s, r) for k in ('ln', 'bn') for (n, s), r in zip(_G_SHAPES[:2], (False, True))]
G_INFER = [GCase(f'bn_{n}', 'bn', s, r) for (n, s), r in zip(_G_SHAPES, (True, False, False))]
G_DW = [GCase(f'dw_{n}{"_bias" if bias else ""}', 'dw', s, bias) for n, s in _G_SHAPES[:2] for bias in (False, True)]   # relu: use_bias


def graph_norm_ref(case, xs, w, dy=None, mode='residual', eps=1e-3):
    """The float64 compositions of section 2 of tests/test_gpu_norm.py -> out, or with ``dy`` (out, [dX per input], {name: gradient}).
    mode 'residual': x = conv1x1(input); out = norm(x) + x ('plain': out = norm(x), the norm's share alone).
    mode 'shared': out = norm(x1) + norm(x2) with one gamma / beta.   mode 'first': out = norm(input).
    For 'bn' the statistics are those of each call's own batch (training mode)."""
    import torch
    from oracle import torch_ops as T
    pt = {k: _t64(v, True) for k, v in w.items() if 'moving' not in k}
    xt = [_t64(x, True) for x in xs]

    def norm(v):
        if case.kind == 'ln':
            y = T.layer_norm(v, pt['n/gamma'], pt['n/beta'], eps)
        else:
            mu, var = T.channel_moments(v)
            y = T.batch_norm(v, pt['n/gamma'], pt['n/beta'], mu, var, eps)
        return torch.relu(y) if case.relu else y
    if mode in ('residual', 'plain'):
        p = T.conv2d(xt[0], pt['p/kernel'], pt['p/bias'])
        out = norm(p) + p if mode == 'residual' else norm(p)
    elif mode == 'shared':
        out = norm(xt[0]) + norm(xt[1])
    else:
        out = norm(xt[0])
    if dy is None:
        return out.detach().numpy()
    (out * _t64(dy)).sum().backward()
    return out.detach().numpy(), [None if t.grad is None else t.grad.numpy() for t in xt], {k: v.grad.numpy() for k, v in pt.items()}


def graph_norm_preact(case, xs, w, mode, eps=1e-3):
    """Every float64 pre-activation of the norms of ``graph_norm_ref`` -> list of arrays."""
    from oracle import np_ops as N
    g, b = w['n/gamma'], w['n/beta']
    vs = [N.conv2d(np.asarray(xs[0], np.float64), w['p/kernel'].astype(np.float64), w['p/bias'].astype(np.float64))] \
        if mode == 'residual' else [np.asarray(x, np.float64) for x in xs]
    return [preact(case.kind, v, g, b, eps) for v in vs]


@functools.lru_cache(maxsize=None)
def graph_inputs(case, mode):
    """-> dict(xs, target, w, mm, mv) of an in-graph case.  With the ReLU fused, whole input pixels are redrawn until no float64
    pre-activation lies within RELU_MARGIN of zero."""
    s = case.shape
    C = s[-1]
    rng = case_rng(f'graph/{mode}/{case.id}')
    n_in = 2 if mode in ('shared', 'dw') else 1
    xs = [(rng.standard_normal(s) + _offsets(rng, (C,))).astype(F32) for _ in range(n_in)]
    target = rng.standard_normal(s).astype(F32)
    if case.kind == 'dw':
        w = {'d/depthwise_kernel': (rng.standard_normal((DW_K, DW_K, C, 1)) * 0.2).astype(F32)}
        if case.relu:
            w['d/bias'] = _offsets(rng, (C,)).astype(F32)
        return dict(xs=xs, target=target, w=w)
    w = {}
    if mode == 'residual':
        w['p/kernel'] = (rng.standard_normal((1, 1, C, C)) / np.sqrt(C)).astype(F32)
        w['p/bias'] = _offsets(rng, (C,)).astype(F32)
    w['n/gamma'] = (1 + 0.2 * rng.standard_normal(C)).astype(F32)
    w['n/beta'] = (0.1 * rng.standard_normal(C)).astype(F32)
    mm, mv = rng.standard_normal(C).astype(F32), (0.5 + rng.random(C)).astype(F32)
    if case.relu and mode != 'infer':
        for _ in range(20):
            bad = [(np.abs(p) < RELU_MARGIN).any(axis=-1) for p in graph_norm_preact(case, xs, w, mode)]
            if not any(b.any() for b in bad):
                break
            for x, b in zip(xs, bad):
                x[b] += (0.05 * rng.standard_normal((int(b.sum()), C))).astype(F32)
        else:
            raise AssertionError('could not remove the ReLU ties')
    return dict(xs=xs, target=target, w=w, mm=mm, mv=mv)


def graph_dw_ref(case, xs, w, dy):
    """out = dw(x1) + dw(x2) with one kernel (and bias) -> (out, [dX1, dX2], {name: gradient summed over both})."""
    from oracle import torch_ops as T
    pt = {k: _t64(v, True) for k, v in w.items()}
    xt = [_t64(x, True) for x in xs]
    out = sum(T.depthwise_conv2d(t, pt['d/depthwise_kernel'], pt.get('d/bias')) for t in xt)
    (out * _t64(dy)).sum().backward()
    return out.detach().numpy(), [t.grad.numpy() for t in xt], {k: v.grad.numpy() for k, v in pt.items()}
