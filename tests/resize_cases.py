"""Cases, launcher restatements and CPU references of tests/test_gpu_resize.py (not a test module; needs no GPU).

A case is one Resizing op on a dense graph input of shape (n * t, h, w, c) -> (n * t, ho, wo, c).  For every case ``select`` names
the kernels that csrc/elementwise.hip's resize_table_forward / resize_table_backward (and the nearest launchers) pick for it, from a
restatement of their conditions for dense, 16-byte-aligned tensors (Graph::prepare aligns every buffer to 256 bytes; a resize input
is never aliased into a Concatenate):

  forward   C % 4 == 0 and ky == kx in {2, 4}                -> fwdk<2> / fwdk<4>   (one block per output row; 256 threads when
                                                                 Wo * C / 4 >= 256, else 64; at most 65536 blocks)
            C % 4 == 0 otherwise                              -> fwd4                (grid-stride over Y / 4)
            C % 4 != 0                                        -> fwd                 (grid-stride over Y)
  backward  C % 4 == 0 and max_back_x <= 4 / <= 8             -> bwd4u<4> / bwd4u<8> (grid-stride over dX / 4)
            C % 4 == 0 otherwise                              -> bwd4
            C % 4 != 0                                        -> bwd                 (grid-stride over dX)

ky / kx are the taps per output the table builders of csrc/graph.hip emit (bilinear 2, bicubic 4, the ScaleAndTranslate family its
widest clamped span); max_back_x is the largest number of non-zero (output, tap) entries one input column receives.  Both are taken
from the oracle's axis matrices (oracle/np_ops.py) and the bilinear matrix built here in the oracle's arithmetic; a bilinear border
output clamps both taps onto one column and they count separately, as in ResizeOp::axis.

References are dense axis matrices applied with BLAS-backed einsum in float64: Y = My X Mx^T, dX = My^T dY Mx.
tests/test_resize_cases.py holds them to oracle.torch_ops' own resizes.
"""
import functools
import zlib
from collections import namedtuple

import numpy as np

from oracle import np_ops as N

F32 = np.float32
TABLE_METHODS = ('bilinear', 'bicubic', 'lanczos3', 'lanczos5', 'gaussian', 'mitchellcubic')
EW_GRID_THREADS = 8192 * 256       # ew_blocks: tests/test_graph_ops_oracle.py checks the figure against the source
FWDK_MAX_BLOCKS = 65536            # resize_table_forward: dim3(min(rows, 65536))
FWDK_WIDE_ROW = 256                # ... and 256 threads per block once a row has this many float4, else 64

Case = namedtuple('Case', 'id method n t h w c ho wo')


def _case(id, method, n, t, h, w, c, ho, wo):
    return Case(id, method, n, t, h, w, c, ho, wo)


# ---------------------------------------------------------------------------------------------------------------- axis matrices
def bilinear_taps(inn, out, dtype=np.float64):
    """(lo, hi, f) of tf.image.resize(method='bilinear') along one axis, half-pixel centres: float64 is the arithmetic of
    oracle.np_ops.resize_bilinear, float32 that of bilinear_axis_tables in csrc/graph.hip."""
    t = np.dtype(dtype).type
    scale = t(inn) / t(out)
    src = (np.arange(out).astype(dtype) + t(0.5)) * scale - t(0.5)
    fl = np.floor(src)
    lo = np.maximum(fl, 0).astype(np.int64)
    hi = np.minimum(np.ceil(src), inn - 1).astype(np.int64)
    return lo, hi, src - fl


def bilinear_axis_matrix(inn, out):
    """Dense (out, inn) matrix of the oracle's bilinear resize along one axis."""
    lo, hi, f = bilinear_taps(inn, out)
    M = np.zeros((out, inn), np.float64)
    o = np.arange(out)
    M[o, lo] += 1.0 - f
    M[o, hi] += f
    return M


@functools.lru_cache(maxsize=None)
def axis_matrix(method, inn, out):
    if method == 'bilinear':
        M = bilinear_axis_matrix(inn, out)
    elif method == 'bicubic':
        M = N.bicubic_axis_matrix(inn, out)
    elif method == 'nearest':
        src = N.resize_nearest(np.arange(inn).reshape(1, inn, 1, 1), out, 1).reshape(out)
        M = np.zeros((out, inn), np.float64)
        M[np.arange(out), src] = 1.0
    else:
        M = N.scale_translate_axis_matrix(inn, out, method)
    M.setflags(write=False)
    return M


def back_counts(method, inn, out, dtype=np.float64):
    """Per input index: how many non-zero (output, tap) entries it receives."""
    if method == 'bilinear':
        lo, hi, f = bilinear_taps(inn, out, dtype)
        one = np.dtype(dtype).type(1)
        return np.bincount(lo[(one - f) != 0], minlength=inn) + np.bincount(hi[f != 0], minlength=inn)
    return (axis_matrix(method, inn, out) != 0).sum(axis=0)


def scale_translate_span(inn, out, method):
    """Widest clamped span of ScaleAndTranslate along one axis, float32 like scale_translate_axis_tables: the K it returns."""
    R = F32({'lanczos3': 3.0, 'lanczos5': 5.0, 'gaussian': 1.5, 'mitchellcubic': 2.0}[method])
    sample = (np.arange(out, dtype=F32) + F32(0.5)) * (F32(1) / (F32(out) / F32(inn)))
    s0 = np.clip(np.ceil(sample - R - F32(0.5)), 0, inn - 1)
    s1 = np.clip(np.floor(sample + R - F32(0.5)), 0, inn - 1) + 1
    return int(max(1, (s1 - s0).max()))


def taps(method, inn, out):
    return 2 if method == 'bilinear' else 4 if method == 'bicubic' else scale_translate_span(inn, out, method)


# ---------------------------------------------------------------------------------------------------------------- selection
def select(case):
    """-> dict(fwd, bwd, loops): the forward and backward kernel of the case and which of their loops run more than once
    ('rows': fwdk over rows, 'per_row': fwdk over a row of more than 256 float4, 'grid_fwd' / 'grid_bwd': the grid-stride loop)."""
    rows, vec = case.n * case.t * case.ho, case.c % 4 == 0
    y_items = rows * case.wo * case.c
    x_items = case.n * case.t * case.h * case.w * case.c
    loops = set()
    if case.method == 'nearest':
        fwd, bwd, fwd_items, bwd_items = 'nearest_fwd', 'nearest_bwd', y_items, x_items
    else:
        ky, kx = taps(case.method, case.h, case.ho), taps(case.method, case.w, case.wo)
        max_back_x = int(back_counts(case.method, case.w, case.wo).max())
        per_row4 = case.wo * (case.c // 4)
        if vec and ky == kx and ky in (2, 4) and rows < 2 ** 31 and per_row4 < 2 ** 20 and case.c // 4 <= 4096:
            fwd, fwd_items = f'fwdk<{ky}>', 0
            if rows > FWDK_MAX_BLOCKS:
                loops.add('rows')
            if per_row4 > FWDK_WIDE_ROW:
                loops.add('per_row')
        elif vec:
            fwd, fwd_items = 'fwd4', y_items // 4
        else:
            fwd, fwd_items = 'fwd', y_items
        if vec:
            bwd = 'bwd4u<4>' if 0 < max_back_x <= 4 else 'bwd4u<8>' if 0 < max_back_x <= 8 else 'bwd4'
            bwd_items = x_items // 4
        else:
            bwd, bwd_items = 'bwd', x_items
    if fwd_items > EW_GRID_THREADS:
        loops.add('grid_fwd')
    if bwd_items > EW_GRID_THREADS:
        loops.add('grid_bwd')
    return dict(fwd=fwd, bwd=bwd, loops=loops)


def per_row4(case):
    return case.wo * (case.c // 4)


# ---------------------------------------------------------------------------------------------------------------- cases
# id, method, n, t, h, w, c, ho, wo -- the smallest shapes that still select each kernel; EXPECT below names it per case
BILINEAR_VEC = [
    _case('bl_x2_c4', 'bilinear', 2, 1, 5, 7, 4, 10, 14),
    _case('bl_x2_c8', 'bilinear', 1, 1, 6, 5, 8, 12, 10),
    _case('bl_x3_c4', 'bilinear', 1, 1, 5, 6, 4, 15, 18),
    _case('bl_x3_c8_t3', 'bilinear', 1, 3, 4, 5, 8, 12, 15),
    _case('bl_x4_c4_t3', 'bilinear', 2, 3, 4, 6, 4, 16, 24),          # the cfg4 form: x4, T > 1
    _case('bl_x4_c8', 'bilinear', 1, 1, 5, 10, 8, 20, 40),            # 80 float4 per row on 64 threads: ragged second trip
    _case('bl_x5_c4', 'bilinear', 1, 1, 4, 5, 4, 20, 25),
    _case('bl_x5_c8', 'bilinear', 1, 1, 3, 4, 8, 15, 20),
    _case('bl_x8_c4', 'bilinear', 1, 1, 3, 4, 4, 24, 32),
    _case('bl_x8_c8', 'bilinear', 1, 1, 4, 3, 8, 32, 24),
    _case('bl_half_c4', 'bilinear', 2, 1, 12, 10, 4, 6, 5),
    _case('bl_half_c8', 'bilinear', 1, 1, 8, 14, 8, 4, 7),
    _case('bl_fracdown_c4', 'bilinear', 1, 1, 12, 10, 4, 5, 4),
    _case('bl_fracdown_c8', 'bilinear', 1, 1, 12, 10, 8, 5, 4),
    _case('bl_fracup_c4', 'bilinear', 1, 1, 6, 5, 4, 15, 8),
    _case('bl_fracup_c8', 'bilinear', 1, 1, 6, 5, 8, 15, 8),
    _case('bl_same_c4', 'bilinear', 2, 1, 7, 9, 4, 7, 9),
    _case('bl_same_c8', 'bilinear', 1, 1, 7, 9, 8, 7, 9),
    _case('bl_wo4_c4', 'bilinear', 1, 1, 3, 2, 4, 6, 4),              # 4 float4 per row: 64 threads, fast_div by 1
    _case('bl_wo64_c4', 'bilinear', 1, 1, 2, 32, 4, 4, 64),           # 64 float4 per row: every thread of the 64 once
    _case('bl_wo64_c16', 'bilinear', 1, 1, 2, 32, 16, 4, 64),         # exactly 256: the 256-thread launch, one trip
    _case('bl_wo70_c16', 'bilinear', 1, 1, 3, 35, 16, 6, 70),         # 280: 256 threads, second trip of 24
    _case('bl_wo72_c16_x4', 'bilinear', 1, 2, 2, 18, 16, 8, 72),      # 288
    _case('bl_rows', 'bilinear', 33, 1, 1024, 1, 4, 2048, 2),         # 67584 rows on 65536 blocks
]
BICUBIC_VEC = [
    _case('bc_x2_c4', 'bicubic', 2, 1, 5, 7, 4, 10, 14),
    _case('bc_x2_c8_t3', 'bicubic', 1, 3, 4, 6, 8, 8, 12),
    _case('bc_x3_c4', 'bicubic', 1, 1, 5, 6, 4, 15, 18),
    _case('bc_fracup_c4', 'bicubic', 1, 1, 6, 5, 4, 15, 8),
]
OTHER_VEC = [
    _case('l3_x2_c4', 'lanczos3', 1, 1, 8, 7, 4, 16, 14),
    _case('l3_fracdown_c4', 'lanczos3', 1, 1, 12, 10, 4, 5, 4),
    _case('l5_x2_c4', 'lanczos5', 1, 1, 6, 11, 4, 12, 22),
    _case('ga_x2_c4', 'gaussian', 2, 1, 5, 7, 4, 10, 14),
    _case('ga_x4_c8', 'gaussian', 1, 1, 4, 6, 8, 16, 24),
    _case('mi_x2_c4', 'mitchellcubic', 2, 1, 5, 6, 4, 10, 12),        # widest span 4 on both axes: the second way into fwdk<4>
    _case('mi_x2_c8_t3', 'mitchellcubic', 1, 3, 4, 7, 8, 8, 14),
    _case('mi_x2x3_c4', 'mitchellcubic', 1, 1, 6, 5, 4, 12, 15),      # spans 4 and 5: ky != kx
    _case('l3_same_c4', 'lanczos3', 1, 1, 7, 9, 4, 7, 9),
]
SCALAR = [
    _case('bl_x2_c3', 'bilinear', 2, 1, 5, 7, 3, 10, 14),
    _case('bl_x3_c1', 'bilinear', 2, 1, 9, 9, 1, 27, 27),
    _case('bl_fracup_c6', 'bilinear', 1, 1, 6, 5, 6, 15, 8),
    _case('bl_fracdown_c3', 'bilinear', 1, 1, 12, 10, 3, 5, 4),
    _case('bl_x4_c6_t3', 'bilinear', 1, 3, 4, 6, 6, 16, 24),
    _case('bc_x2_c3', 'bicubic', 2, 1, 5, 7, 3, 10, 14),
    _case('l3_x3_c1', 'lanczos3', 1, 1, 9, 9, 1, 27, 27),
    _case('l5_fracdown_c2', 'lanczos5', 1, 1, 12, 10, 2, 5, 4),
    _case('ga_fracup_c6', 'gaussian', 1, 1, 6, 5, 6, 15, 8),
    _case('mi_x2_c3', 'mitchellcubic', 1, 1, 5, 6, 3, 10, 12),
]
_DEGENERATE_GRIDS = [('hi1', 1, 5, 3, 10), ('wi1', 5, 1, 10, 3), ('ho1', 6, 5, 1, 10), ('wo1', 6, 5, 12, 1), ('2to3', 2, 2, 3, 3)]
DEGENERATE = [_case(f'{p}_{tag}_c{c}', m, 2, 1, h, w, c, ho, wo)
              for p, m in (('bl', 'bilinear'), ('bc', 'bicubic'), ('l3', 'lanczos3')) for c in (3, 4)
              for tag, h, w, ho, wo in _DEGENERATE_GRIDS]
# more than 8192 * 256 work items; power-of-two ratios, so that the float32 source coordinates of the tables are exact at these sizes
LARGE = [
    _case('bl_half_c64_large_dx', 'bilinear', 3, 1, 192, 256, 64, 96, 128),          # 1.125 x the cap in float4 of dX (bwd4u<4>)
    _case('ga_x2_c64_large_y', 'gaussian', 3, 1, 96, 128, 64, 192, 256),             # ... in float4 of Y (fwd4)
    _case('bl_half_x2_c3_large', 'bilinear', 1, 1, 1024, 768, 3, 512, 1536),         # ... in elements of Y and of dX (fwd, bwd)
]
SMALL_TABLE = BILINEAR_VEC[:-1] + BICUBIC_VEC + OTHER_VEC + SCALAR + DEGENERATE
TABLE = SMALL_TABLE + [BILINEAR_VEC[-1]] + LARGE

NEAREST = [_case(f'nn_{tag}_c{c}', 'nearest', n, 1, h, w, c, ho, wo)
           for c in (1, 3, 4)
           for tag, n, h, w, ho, wo in [('x2', 2, 5, 7, 10, 14), ('x3', 1, 9, 9, 27, 27), ('fracup', 1, 5, 7, 12, 15),
                                        ('fracdown', 1, 12, 10, 5, 4), ('same', 2, 7, 9, 7, 9)]
           + [(tag, 2, h, w, ho, wo) for tag, h, w, ho, wo in _DEGENERATE_GRIDS]]
NEAREST.append(_case('nn_x4_c4_t3', 'nearest', 2, 3, 4, 6, 4, 16, 24))
NEAREST_LARGE = [_case('nn_half_x2_c3_large', 'nearest', 1, 1, 1024, 768, 3, 512, 1536)]

# resize created first (its backward runs second, accumulating), resize created second, shape
ACCUMULATE = [
    ('nearest_bwd', _case('acc_nn_c3', 'nearest', 2, 1, 5, 7, 3, 10, 14), 'bilinear'),
    ('nearest_bwd', _case('acc_nn_c4', 'nearest', 1, 1, 5, 7, 4, 12, 15), 'bicubic'),
    ('bwd', _case('acc_bl_c3', 'bilinear', 2, 1, 5, 7, 3, 10, 14), 'bicubic'),
    ('bwd', _case('acc_l3_c6', 'lanczos3', 1, 1, 6, 5, 6, 15, 8), 'bilinear'),
    ('bwd4', _case('acc_bl_x5_c4', 'bilinear', 1, 1, 4, 5, 4, 20, 25), 'bicubic'),
    ('bwd4', _case('acc_bc_x3_c8', 'bicubic', 1, 1, 5, 6, 8, 15, 18), 'bilinear'),
    ('bwd4u<4>', _case('acc_bl_x2_c4', 'bilinear', 2, 1, 5, 7, 4, 10, 14), 'bicubic'),
    ('bwd4u<4>', _case('acc_bl_half_c8', 'bilinear', 1, 1, 8, 14, 8, 4, 7), 'gaussian'),
    ('bwd4u<8>', _case('acc_bl_x4_c8_t3', 'bilinear', 1, 3, 4, 6, 8, 16, 24), 'gaussian'),
    ('bwd4u<8>', _case('acc_bc_x2_c4', 'bicubic', 2, 1, 5, 7, 4, 10, 14), 'nearest'),
]

# what each named group is there for: (forward kernel, backward kernel) that ``select`` must return
EXPECT = {
    'bl_x2_c4': ('fwdk<2>', 'bwd4u<4>'), 'bl_x2_c8': ('fwdk<2>', 'bwd4u<4>'),
    'bl_x3_c4': ('fwdk<2>', 'bwd4u<8>'), 'bl_x3_c8_t3': ('fwdk<2>', 'bwd4u<8>'),
    'bl_x4_c4_t3': ('fwdk<2>', 'bwd4u<8>'), 'bl_x4_c8': ('fwdk<2>', 'bwd4u<8>'),
    'bl_x5_c4': ('fwdk<2>', 'bwd4'), 'bl_x5_c8': ('fwdk<2>', 'bwd4'), 'bl_x8_c4': ('fwdk<2>', 'bwd4'), 'bl_x8_c8': ('fwdk<2>', 'bwd4'),
    'bl_half_c4': ('fwdk<2>', 'bwd4u<4>'), 'bl_same_c4': ('fwdk<2>', 'bwd4u<4>'),
    'bl_wo4_c4': ('fwdk<2>', 'bwd4u<4>'), 'bl_wo64_c4': ('fwdk<2>', 'bwd4u<4>'), 'bl_wo64_c16': ('fwdk<2>', 'bwd4u<4>'),
    'bl_wo70_c16': ('fwdk<2>', 'bwd4u<4>'), 'bl_wo72_c16_x4': ('fwdk<2>', 'bwd4u<8>'), 'bl_rows': ('fwdk<2>', 'bwd4u<4>'),
    'bc_x2_c4': ('fwdk<4>', 'bwd4u<8>'), 'bc_x2_c8_t3': ('fwdk<4>', 'bwd4u<8>'), 'bc_x3_c4': ('fwdk<4>', 'bwd4'),
    'l3_x2_c4': ('fwd4', 'bwd4'), 'l5_x2_c4': ('fwd4', 'bwd4'), 'ga_x2_c4': ('fwd4', 'bwd4u<8>'),
    'mi_x2_c4': ('fwdk<4>', 'bwd4u<8>'), 'mi_x2_c8_t3': ('fwdk<4>', 'bwd4u<8>'), 'mi_x2x3_c4': ('fwd4', 'bwd4'),
    'bl_x2_c3': ('fwd', 'bwd'), 'bl_x3_c1': ('fwd', 'bwd'), 'bl_fracup_c6': ('fwd', 'bwd'), 'bc_x2_c3': ('fwd', 'bwd'),
    'bl_half_c64_large_dx': ('fwdk<2>', 'bwd4u<4>'), 'ga_x2_c64_large_y': ('fwd4', 'bwd4u<8>'), 'bl_half_x2_c3_large': ('fwd', 'bwd'),
}
EXPECT_LOOPS = {
    'bl_rows': {'rows'}, 'bl_wo70_c16': {'per_row'}, 'bl_wo72_c16_x4': {'per_row'}, 'bl_wo64_c16': set(), 'bl_wo64_c4': set(),
    'bl_half_c64_large_dx': {'grid_bwd', 'per_row'}, 'ga_x2_c64_large_y': {'grid_fwd'}, 'bl_half_x2_c3_large': {'grid_fwd', 'grid_bwd'},
    'nn_half_x2_c3_large': {'grid_fwd', 'grid_bwd'},
}
ALL_KERNELS = ('fwd', 'fwd4', 'fwdk<2>', 'fwdk<4>', 'bwd', 'bwd4', 'bwd4u<4>', 'bwd4u<8>', 'nearest_fwd', 'nearest_bwd')


# ---------------------------------------------------------------------------------------------------------------- data and references
def case_rng(case, salt=0):
    return np.random.default_rng(zlib.crc32(case.id.encode()) + salt)


def case_input(case):
    """(n, [t,] h, w, c) float32 standard normal, seeded by the case's name."""
    lead = (case.n,) if case.t == 1 else (case.n, case.t)
    return case_rng(case).standard_normal(lead + (case.h, case.w, case.c)).astype(F32)


def case_target(case):
    lead = (case.n,) if case.t == 1 else (case.n, case.t)
    return case_rng(case, 1).standard_normal(lead + (case.ho, case.wo, case.c)).astype(F32)


def matrices(case, method=None):
    m = method or case.method
    return axis_matrix(m, case.h, case.ho), axis_matrix(m, case.w, case.wo)


def apply_forward(x, My, Mx):
    """Y = My X Mx^T per image and channel, in the dtype of the operands; x: (N, h, w, c)."""
    rows = np.einsum('oh,nhwc->nowc', My, x, optimize=True)
    return np.einsum('pw,nowc->nopc', Mx, rows, optimize=True)


def apply_backward(dy, My, Mx):
    """dX = My^T dY Mx; dy: (N, ho, wo, c)."""
    cols = np.einsum('pw,nopc->nowc', Mx, dy, optimize=True)
    return np.einsum('oh,nowc->nhwc', My, cols, optimize=True)


def flat(case, a):
    """(n, [t,] H, W, c) -> (n * t, H, W, c)."""
    return np.asarray(a).reshape((case.n * case.t,) + a.shape[-3:])


def forward_ref(case, x, method=None):
    My, Mx = matrices(case, method)
    return apply_forward(flat(case, x).astype(np.float64), My, Mx)


def backward_ref(case, dy, method=None):
    My, Mx = matrices(case, method)
    return apply_backward(flat(case, dy).astype(np.float64), My, Mx)


def torch_resize(method):
    """oracle.torch_ops' resize of ``method`` as f(x, ho, wo)."""
    from oracle import torch_ops as T
    if method in ('bilinear', 'bicubic', 'nearest'):
        return getattr(T, 'resize_' + method)
    return lambda x, ho, wo: T.resize_scale_translate(x, ho, wo, method)


def torch_refs(case, x, dy, methods=None):
    """float64 forward and dX of the sum of the resizes ``methods`` (default: the case's own) by autograd through oracle.torch_ops,
    for the upstream gradient ``dy``; all arrays (n * t, H, W, c)."""
    import torch
    xt = torch.tensor(flat(case, x).astype(np.float64), requires_grad=True)
    y = sum(torch_resize(m)(xt, case.ho, case.wo) for m in (methods or (case.method,)))
    (y * torch.tensor(flat(case, dy).astype(np.float64))).sum().backward()
    return y.detach().numpy(), xt.grad.numpy()


def rel_err(got, ref):
    """max |got - ref| over max |ref|: the figure of tests/test_gpu_ops.py's close()."""
    ref = np.asarray(ref, np.float64)
    got = np.asarray(got, np.float64)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    return float(np.abs(got - ref).max() / max(np.abs(ref).max(), 1e-6))


# ---------------------------------------------------------------------------------------------------------------- tolerances
FWD_TOL = 1e-5            # the project's figure for these kernels (test_resize_bicubic_in_graph)
DX_TOL = 1e-5             # the same, kept because the float32 evaluation below stays under a quarter of it on every case
DX_EMULATION_CAP = 2.5e-6


def dx_emulation_error(case, method=None):
    """rel_err of My^T dY Mx evaluated in numpy float32 (weights rounded to float32, dY a float32 standard normal) against the float64
    evaluation with the unrounded weights."""
    My, Mx = matrices(case, method)
    dy = flat(case, case_target(case))
    got = apply_backward(dy, My.astype(F32), Mx.astype(F32))
    assert got.dtype == F32
    return rel_err(got, apply_backward(dy.astype(np.float64), My, Mx))


# ---------------------------------------------------------------------------------------------------------------- nearest
def nearest_src(inn, out, dtype=np.float64):
    """Source index per output of the half-pixel nearest resize: float64 as the oracle evaluates it, float32 as nearest_src of
    csrc/elementwise.hip does."""
    t = np.dtype(dtype).type
    return np.minimum(np.floor((np.arange(out).astype(dtype) + t(0.5)) * (t(inn) / t(out))).astype(np.int64), inn - 1)


def nearest_backward_ref(case, dy):
    """(float64 sum of the dY entries every input element was copied to, the sum of their absolute values)."""
    My, Mx = matrices(case, 'nearest')
    d = flat(case, dy).astype(np.float64)
    return apply_backward(d, My, Mx), apply_backward(np.abs(d), My, Mx)


def nearest_terms(case):
    """k: no input element is copied to more than ceil(Ho / H) * ceil(Wo / W) outputs."""
    return -(-case.ho // case.h) * -(-case.wo // case.w)
