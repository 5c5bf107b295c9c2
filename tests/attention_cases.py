"""Cases, launcher restatements and float64 references of tests/test_gpu_attention.py (not a test module; needs no GPU).

ChannelAttention2D (csrc/attention.hip) views its input as [G][R][Q = P * C]: the mean runs over R, the two-layer MLP over the C
channels of each of the ninst = G * P instances.  (B, H, W, C): G = B, R = H W, P = 1.  (B, T, H, W, C): G = B, R = T H, P = W.

``select`` restates what the launchers of csrc/attention.hip pick for dense, 16-byte-aligned operands (every DeviceArray and every
graph buffer is):

  column sum   Q >= 256 and Q % 4 == 0             -> colsum4   (64 column quads x 4 row phases per block, nb4 = min(cdiv(R, 32), 256)
                                                                  row blocks; per thread an 8-row unrolled loop, then a tail loop)
               otherwise                           -> colsum<TX> (TX = pick_tx(Q), TY = 256 / TX, nb = min(cdiv(R, 8 TY), 256))
  finish       colsum_finish_kernel                   an 8-way loop over nb & ~7 partial rows, then the remainder
  apply        R Q % 4 == 0                        -> chatt_apply<4> (a float4 straddles two rows when Q % 4 != 0), else chatt_apply<1>;
                                                      bx = min(cdiv(n, 256), max(1, 8192 / G)) blocks per sample, grid-stride beyond
  MLP backward chatt_mlp_bwd_inst_kernel              one thread per instance, 256 per block
               chatt_mlp_bwd_param_kernel             one wave per output, lanes stride the instances by 64

tests/test_attention_cases.py holds the restated conjuncts to the source text, and the references here to oracle.models.
"""
import functools
import zlib
from collections import namedtuple

import numpy as np

F32 = np.float32
U = 2.0 ** -24                     # unit roundoff of float32
TOL = 2e-4                         # tests/test_gpu_ops.py::close: max error over max |reference|
RELU_MARGIN = 1e-3                 # every float64 hidden pre-activation keeps this distance from the ReLU's kink
MEAN_BOUND = 4 * U                 # |mean - exact| <= 4 * 2^-24 |exact| on integer data: the rounding of 1.f / R, the product, x 2
NARROW_PAIR_ROWS = 4               # csrc/conv_narrow.hip; a pooling tile of the pair convolution is 32 x (4 * NARROW_PAIR_ROWS) pixels
POOL_TILE_W, POOL_TILE_H = 32, 4 * NARROW_PAIR_ROWS

Case = namedtuple('Case', 'id shape')


def cdiv(a, b):
    return -(-a // b)


def dims(case):
    """-> dict(G, R, P, C, Cr, Q, ninst): ops._att_shape."""
    s = case.shape
    if len(s) == 4:
        G, R, P, C = s[0], s[1] * s[2], 1, s[3]
    else:
        G, R, P, C = s[0], s[1] * s[2], s[3], s[4]
    return dict(G=G, R=R, P=P, C=C, Cr=C // 4, Q=P * C, ninst=G * P)


# ---------------------------------------------------------------------------------------------------------------- selection
def pick_tx(Q):
    return 8 if Q <= 8 else 16 if Q <= 16 else 32 if Q <= 32 else 64


def colsum_blocks(R, TY):
    return max(1, min(cdiv(R, TY * 8), 256))


def _colsum4_loops(R, nb4):
    """Per row phase r0 = blockIdx.x * 4 + tyi of colsum4_kernel: (trips of the 8-row unrolled loop, trips of the tail loop)."""
    step = nb4 * 4
    out = []
    for r0 in range(step):
        r, unrolled, tail = r0, 0, 0
        while r + 7 * step < R:
            r += 8 * step
            unrolled += 1
        while r < R:
            r += step
            tail += 1
        out.append((unrolled, tail))
    return out


def _some(n, of):
    return 'none' if n == 0 else 'all' if n == of else 'some'


def select(case):
    """-> dict: the column-sum kernel (``colsum``) with TX, nb and the largest number of rows one thread adds (``row_trips``); for
    colsum4 which of its row phases enter the unrolled loop, the tail loop, and both in turn ('none' / 'some' / 'all' of the
    4 * nb4 phases); which loops of colsum_finish_kernel run; the apply kernel's V, bx, grid-stride trips and dq; ninst with the
    trips of the parameter kernel's lane-stride loop and the blocks of the instance kernel; and ``features``, the names
    tests/test_attention_cases.py counts."""
    d = dims(case)
    G, R, Q, ninst = d['G'], d['R'], d['Q'], d['ninst']
    f = set()
    TX = pick_tx(Q)
    sel = dict(TX=TX, ninst=ninst)
    if Q >= 256 and (Q & 3) == 0:
        nb = max(1, min(cdiv(R, 4 * 8), 256))
        loops = _colsum4_loops(R, nb)
        n = len(loops)
        sel.update(colsum='colsum4', nb=nb, row_trips=max(8 * u + t for u, t in loops),
                   unrolled=_some(sum(u > 0 for u, _ in loops), n), tail=_some(sum(t > 0 for _, t in loops), n),
                   unrolled_then_tail=_some(sum(u > 0 and t > 0 for u, t in loops), n))
        f.add('colsum4')
        if sel['unrolled'] != 'none':
            f.add('colsum4:unrolled')
        if sel['tail'] != 'none':
            f.add('colsum4:tail')
        if sel['unrolled_then_tail'] != 'none':
            f.add('colsum4:unrolled_then_tail')
        if sel['unrolled'] == 'some' and sel['tail'] == 'some' and sel['unrolled_then_tail'] == 'none':
            f.add('colsum4:split')                      # some phases take the unrolled loop alone, the others the tail alone
        if Q % 256:
            f.add('colsum4:dead_quads')                 # the last column block has quads behind q < Q
        if cdiv(R, 32) > 256:
            f.add('colsum4:capped')
    else:
        TY = 256 // TX
        nb = colsum_blocks(R, TY)
        trips = [cdiv(R - r0, nb * TY) if r0 < R else 0 for r0 in range(nb * TY)]
        sel.update(colsum=f'colsum<{TX}>', nb=nb, row_trips=max(trips), unrolled='none', tail='none', unrolled_then_tail='none')
        f.add(sel['colsum'])
        if max(trips) > 1:
            f.add('colsum:rows>1')
        if min(trips) == 0:
            f.add('colsum:idle_phase')                  # a row phase with no row (R < nb * TY)
        if Q % TX:
            f.add('colsum:ragged_q')
        if cdiv(R, TY * 8) > 256:
            f.add('colsum:capped')
        if Q >= 256:
            f.add('colsum:wide_scalar')                 # wide enough for colsum4, refused for Q % 4 != 0
    sel['finish'] = {'eight'} if nb >= 8 else set()
    if nb % 8:
        sel['finish'].add('rest')
    f.add('finish:' + '+'.join(sorted(sel['finish'])))
    RQ = R * Q
    V = 4 if (RQ & 3) == 0 else 1
    n = RQ // V
    bx = max(1, min((n + 255) // 256, max(1, 8192 // G)))
    sel.update(V=V, bx=bx, trips=cdiv(n, bx * 256), dq=(bx * 256 * V) % Q, straddle=V == 4 and Q % 4 != 0)
    f.add(f'apply<{V}>')
    if sel['straddle']:
        f.add('apply<4>:straddle')
    if sel['trips'] > 1:
        f.add(f'apply<{V}>:grid_stride')
    sel.update(lane_trips=cdiv(ninst, 64), inst_blocks=cdiv(ninst, 256))
    if sel['lane_trips'] > 1:
        f.add('mlp:lane_trips>1')
    if sel['inst_blocks'] > 1:
        f.add('mlp:inst_blocks>1')
    sel['features'] = f
    return sel


# every kernel, template instantiation and loop of the eager path: each must be selected by at least two cases
FEATURES = ('colsum<8>', 'colsum<16>', 'colsum<32>', 'colsum<64>', 'colsum4', 'colsum:rows>1', 'colsum:idle_phase', 'colsum:ragged_q',
            'colsum:capped', 'colsum:wide_scalar', 'colsum4:unrolled', 'colsum4:tail', 'colsum4:unrolled_then_tail', 'colsum4:split',
            'colsum4:dead_quads', 'colsum4:capped', 'finish:eight', 'finish:rest', 'finish:eight+rest', 'apply<1>', 'apply<4>',
            'apply<4>:straddle', 'apply<4>:grid_stride', 'apply<1>:grid_stride', 'mlp:lane_trips>1', 'mlp:inst_blocks>1')
# the two grid-stride launches are one loop of one kernel template each: together they make the loop's two cases
ONCE = ('apply<4>:grid_stride', 'apply<1>:grid_stride')

# ---------------------------------------------------------------------------------------------------------------- eager cases
EAGER = [
    Case('tx32_ragged', (2, 9, 11, 20)),            # colsum<32>, 20 of 32 columns live
    Case('tx32_full', (1, 5, 7, 32)),               # colsum<32>, every column live
    Case('r1', (3, 1, 1, 8)),                       # R = 1: 31 of 32 row phases idle, mean == x
    Case('r3_tx16', (2, 1, 3, 12)),                 # R = 3 < TY = 16
    Case('tx16', (2, 5, 6, 12)),                    # colsum<16> with every row phase busy
    Case('nb11', (2, 16, 22, 64)),                  # R = 352, TX = 64: nb = 11 -> the 8-way loop, then three more
    Case('nb_cap_tx64', (1, 96, 96, 64)),           # R = 9216: cdiv(R, 32) = 288 > 256 blocks, nine rows per thread
    Case('nb_cap_tx8', (1, 260, 260, 8)),           # R = 67600: cdiv(R, 256) = 265 > 256 blocks, eight or nine rows per thread
    Case('c4_split', (2, 3, 100, 13, 20)),          # R = 300, Q = 260: nb4 = 10; phases 0..19 unrolled, 20..39 tail; one live quad behind 256
    Case('c4_split_r60', (1, 6, 10, 32, 8)),        # R = 60, Q = 256: nb4 = 2; phases 0..3 unrolled, 4..7 tail
    Case('c4_tail', (2, 5, 8, 33, 8)),             # R = 40, Q = 264: the tail loop alone
    Case('c4_unrolled', (2, 4, 8, 16, 16)),         # R = 32, Q = 256: the unrolled loop alone
    Case('c4_cap', (1, 130, 64, 32, 8)),            # R = 8320: nb4 capped at 256; every phase unrolled once, phases 0..127 one tail row
    Case('c4_cap_c4', (1, 2, 4100, 64, 4)),         # R = 8200: the same with C = 4, Cr = 1; phases 0..7 take the tail row
    Case('wide_scalar', (1, 2, 9, 43, 6)),          # Q = 258: refused by colsum4, five column blocks of colsum<64>
    Case('wide_scalar_c5', (1, 3, 5, 65, 5)),       # Q = 325, Cr = 1
    Case('v1', (2, 7, 9, 5)),                       # R Q = 315: scalar apply, forward and backward
    Case('v4_straddle', (1, 6, 10, 6)),             # R Q = 360, Q = 6: qq wraps inside a float4
    Case('v4_straddle_q10', (3, 4, 5, 10)),         # R Q = 200, Q = 10
    Case('stride_v4', (64, 48, 48, 60)),            # 34560 float4 per sample on 128 * 256 threads: a second ragged trip, dq = 32
    Case('stride_v1', (64, 23, 29, 50)),            # 33350 elements per sample on 128 * 256 threads, dq = 18
    Case('inst70', (70, 4, 5, 8)),                  # 70 instances: lanes 0..5 of the parameter kernel take a second one
    Case('inst300', (3, 2, 4, 100, 8)),             # 300 instances: five lane trips, a second block of the instance kernel
    Case('inst260_c4', (2, 2, 3, 130, 4)),          # 260 instances with Cr = 1
]

# what each named case is there for: a subset of select()'s result
EXPECT = {
    'tx32_ragged': dict(colsum='colsum<32>', has={'colsum:ragged_q'}),
    'tx32_full': dict(colsum='colsum<32>', lacks={'colsum:ragged_q'}),
    'r1': dict(colsum='colsum<8>', nb=1, row_trips=1, has={'colsum:idle_phase'}),
    'r3_tx16': dict(colsum='colsum<16>', nb=1, has={'colsum:idle_phase', 'colsum:ragged_q'}),
    'tx16': dict(colsum='colsum<16>', lacks={'colsum:idle_phase'}),
    'nb11': dict(colsum='colsum<64>', nb=11, finish={'eight', 'rest'}),
    'nb_cap_tx64': dict(colsum='colsum<64>', nb=256, row_trips=9, has={'colsum:capped'}),
    'nb_cap_tx8': dict(colsum='colsum<8>', nb=256, row_trips=9, has={'colsum:capped'}),
    'c4_split': dict(colsum='colsum4', nb=10, unrolled='some', tail='some', unrolled_then_tail='none', finish={'eight', 'rest'},
                     has={'colsum4:split', 'colsum4:dead_quads'}),
    'c4_split_r60': dict(colsum='colsum4', nb=2, unrolled='some', tail='some', unrolled_then_tail='none', has={'colsum4:split'},
                         lacks={'colsum4:dead_quads'}),
    'c4_tail': dict(colsum='colsum4', nb=2, unrolled='none', tail='all', has={'colsum4:dead_quads'}),
    'c4_unrolled': dict(colsum='colsum4', nb=1, unrolled='all', tail='none', lacks={'colsum4:dead_quads'}),
    'c4_cap': dict(colsum='colsum4', nb=256, unrolled='all', tail='some', unrolled_then_tail='some', has={'colsum4:capped'}),
    'c4_cap_c4': dict(colsum='colsum4', nb=256, unrolled='all', tail='some', unrolled_then_tail='some', has={'colsum4:capped'}),
    'wide_scalar': dict(colsum='colsum<64>', has={'colsum:wide_scalar', 'colsum:ragged_q'}),
    'wide_scalar_c5': dict(colsum='colsum<64>', V=1, has={'colsum:wide_scalar'}),
    'v1': dict(V=1, trips=1),
    'v4_straddle': dict(V=4, straddle=True),
    'v4_straddle_q10': dict(V=4, straddle=True),
    'stride_v4': dict(V=4, bx=128, trips=2, dq=32, straddle=False),
    'stride_v1': dict(V=1, bx=128, trips=2, dq=18),
    'inst70': dict(ninst=70, lane_trips=2, inst_blocks=1),
    'inst300': dict(ninst=300, lane_trips=5, inst_blocks=2, colsum='colsum4'),
    'inst260_c4': dict(ninst=260, lane_trips=5, inst_blocks=2),
}


# ---------------------------------------------------------------------------------------------------------------- inputs
def case_rng(name, salt=0):
    return np.random.default_rng(zlib.crc32(name.encode()) + salt)


def _offsets(rng, shape):
    """Order-one offsets with either sign: magnitude in [0.5, 1.5)."""
    return rng.choice([-1.0, 1.0], shape) * rng.uniform(0.5, 1.5, shape)


def real_x(name, shape, P):
    """Unit noise on an offset per sample and column of [G][R][Q] (per sample and channel for a 4-D input): not zero-mean."""
    rng = case_rng(name)
    lead, C = shape[:-1], shape[-1]
    off_shape = (shape[0],) + (1,) * (len(shape) - 3) + ((P, C) if P > 1 else (1, C))
    return (rng.standard_normal(lead + (C,)) + _offsets(rng, off_shape)).astype(F32)


def integer_x(case):
    """Integers in [-4, 12] as float32: every column sum is exact in float32 in any order while 12 R < 2^24."""
    return case_rng(case.id, 1).integers(-4, 13, case.shape).astype(F32)


def att_weights(rng, C, Cr, gain=1.0):
    """float32 kernels with fan-in scaling (pre-activations of order ``gain``) and order-one biases."""
    return {'conv1/kernel': (rng.standard_normal((1, 1, C, Cr)) * gain / np.sqrt(C)).astype(F32),
            'conv1/bias': (rng.standard_normal(Cr) * 0.5).astype(F32),
            'conv2/kernel': (rng.standard_normal((1, 1, Cr, C)) * gain / np.sqrt(Cr)).astype(F32),
            'conv2/bias': (rng.standard_normal(C) * 0.5).astype(F32)}


def mean_ref(x):
    """float64 mean over axes (1, 2) -> (ninst, C), instance = g * P + p."""
    x = np.asarray(x, np.float64)
    return x.mean(axis=(1, 2)).reshape(-1, x.shape[-1])


def preact_ref(mean, w):
    C = mean.shape[-1]
    return mean @ w['conv1/kernel'].astype(np.float64).reshape(C, -1) + w['conv1/bias'].astype(np.float64)


def mlp_ref(mean, w):
    """-> (hidden, scale) of the two-layer MLP in float64; mean (ninst, C)."""
    C = mean.shape[-1]
    hidden = np.maximum(preact_ref(mean, w), 0.0)
    z = hidden @ w['conv2/kernel'].astype(np.float64).reshape(-1, C) + w['conv2/bias'].astype(np.float64)
    return hidden, 1.0 / (1.0 + np.exp(-z))


def relu_is_clear(h, Cr, every_instance=False):
    """The condition on the inputs: no hidden pre-activation within RELU_MARGIN of zero; a unit that is active (a case whose hidden
    units are all off has a scale that ignores the mean and zero gradients for the first layer) -- with ``every_instance`` one per
    instance; and both signs present when Cr >= 2."""
    active = (h > 0).any(axis=1).all() if every_instance else (h > 0).any()
    return bool(np.abs(h).min() >= RELU_MARGIN and active and (Cr < 2 or (h < 0).any()))


def draw_weights(name, means, C, Cr, gain=1.0, every_instance=False, accept=None):
    """The first draw (seeds salt = 10, 11, ...) whose pre-activations on every mean of ``means`` are clear of the ReLU (and that
    ``accept`` takes: a further condition on the reference alone)."""
    for salt in range(10, 60):
        w = att_weights(case_rng(name, salt), C, Cr, gain)
        if all(relu_is_clear(preact_ref(m, w), Cr, every_instance) for m in means) and (accept is None or accept(w)):
            return w
    raise AssertionError(f'{name}: no draw clear of the ReLU')


@functools.lru_cache(maxsize=None)
def eager_inputs(case):
    """-> dict(x, dy, w): float32 operands of one eager case (read-only)."""
    d = dims(case)
    x = real_x(case.id, case.shape, d['P'])
    dy = case_rng(case.id, 2).standard_normal(case.shape).astype(F32)
    w = draw_weights(case.id, [mean_ref(x)], d['C'], d['Cr'])
    for a in (x, dy) + tuple(w.values()):
        a.setflags(write=False)
    return dict(x=x, dy=dy, w=w)


# ---------------------------------------------------------------------------------------------------------------- references
class Params(dict):
    """The parameter store oracle.models expects, filled in advance."""

    def get(self, ops_, name, shape, init='glorot'):
        assert tuple(self[name].shape) == tuple(shape), (name, shape)
        return self[name]


W_KEYS = ('conv1/kernel', 'conv1/bias', 'conv2/kernel', 'conv2/bias')


def _t64(a, grad=False):
    import torch
    return torch.tensor(np.asarray(a, np.float64), requires_grad=grad)


def _att(xt, pt, name='a'):
    from oracle import models as M
    from oracle import torch_ops as T
    return M.channel_attention(T, pt, name, xt, xt.shape[-1])


def _torch_params(w, name='a'):
    return Params({f'{name}/{k}': _t64(v, True) for k, v in w.items()})


def oracle_refs(x, w, dy=None, residual=False):
    """oracle.models.channel_attention in float64 (plus x itself with ``residual``) -> y, or with ``dy`` (y, dx, {key: gradient}) by
    autograd.  x (B, H, W, C) or (B, T, H, W, C)."""
    pt = _torch_params(w)
    xt = _t64(x, True)
    y = _att(xt, pt) + xt if residual else _att(xt, pt)
    if dy is None:
        return y.detach().numpy()
    (y * _t64(dy)).sum().backward()
    return y.detach().numpy(), xt.grad.numpy(), {k: pt[f'a/{k}'].grad.numpy() for k in W_KEYS}


def shared_refs(x1, x2, w, dy):
    """att(x1) + att(x2) with ONE set of parameters -> (y, dx1, dx2, {key: gradient summed over both})."""
    pt = _torch_params(w)
    a, b = _t64(x1, True), _t64(x2, True)
    y = _att(a, pt) + _att(b, pt)
    (y * _t64(dy)).sum().backward()
    return y.detach().numpy(), a.grad.numpy(), b.grad.numpy(), {k: pt[f'a/{k}'].grad.numpy() for k in W_KEYS}


def rel_err(got, ref):
    """max |got - ref| over max |ref|: the figure of tests/test_gpu_ops.py's close()."""
    ref = np.asarray(ref, np.float64)
    got = np.asarray(got, np.float64)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    return float(np.abs(got - ref).max() / max(np.abs(ref).max(), 1e-6))


def mlp_bounds(mean, w):
    """Element-wise bounds on what chatt_mlp_fwd_kernel may differ by from ``mlp_ref`` of the SAME float32 mean -> (hidden64,
    bound_h, scale64, bound_s, clearance).

    hidden: a float32 sum of C products on a bias, C + 1 roundings in any order (an FMA saves some): at most (C + 2) u S_h with
    S_h = |b1| + sum |m_k| |w1_kj| (Higham, gamma_n <= (n + 1) u here).  The ReLU passes the error on or removes it.
    z: the kernel sums its own hidden values, so bound_h enters through |w2|, plus (Cr + 2) u S_z for its own Cr + 1 roundings.
    scale = 1 / (1 + exp(-z)): d scale / dz <= 1/4.  expf to 4 ulp (8 u relative) moves scale by s (1 - s) 8 u <= 2 u; a fast
    exp2-based form adds |z| 1.5 u relative, times s (1 - s) <= 0.23 / |z|: under u; the sum and the division add u each.  8 u covers
    them.  ``clearance``: min |pre-activation| - bound_h, positive when the rounding cannot flip a ReLU."""
    C = mean.shape[-1]
    m = np.asarray(mean, np.float64)
    w1 = w['conv1/kernel'].astype(np.float64).reshape(C, -1)
    w2 = w['conv2/kernel'].astype(np.float64).reshape(-1, C)
    b1, b2 = w['conv1/bias'].astype(np.float64), w['conv2/bias'].astype(np.float64)
    Cr = w1.shape[1]
    pre = m @ w1 + b1
    bound_h = (C + 2) * U * (np.abs(m) @ np.abs(w1) + np.abs(b1))
    hidden = np.maximum(pre, 0.0)
    z = hidden @ w2 + b2
    bound_z = bound_h @ np.abs(w2) + (Cr + 2) * U * (hidden @ np.abs(w2) + np.abs(b2))
    scale = 1.0 / (1.0 + np.exp(-z))
    return hidden, bound_h, scale, 0.25 * bound_z + 8 * U, float((np.abs(pre) - bound_h).min())


# ---------------------------------------------------------------------------------------------------------------- in-graph: accumulation
# out = add(channel_attention(x), x): the Add's backward writes x.grad first, the attention's accumulates (accumulate_dx = 1)
ACC_DX = [
    Case('accdx_v4', (2, 6, 10, 8)),                # R Q = 480: chatt_apply<4, true>
    Case('accdx_v4_straddle', (2, 6, 10, 6)),       # R Q = 360, Q = 6: the accumulating float4 straddles rows
    Case('accdx_v1', (2, 7, 9, 5)),                 # R Q = 315: chatt_apply<1, true>
    Case('accdx_5d', (2, 3, 5, 6, 8)),              # (B, T, H, W, C): R = 15, P = 6
]
# two attentions of one name share their four parameters; out = add(att(x1), att(x2)): the second backward runs accumulate_dw = 1
ACC_DW = [
    Case('accdw_4d', (3, 5, 7, 8)),
    Case('accdw_5d', (2, 2, 3, 5, 12)),
    Case('accdw_inst70', (70, 3, 3, 8)),            # the accumulating store behind a two-trip lane loop
]


@functools.lru_cache(maxsize=None)
def graph_inputs(case, n_inputs=1):
    """-> dict(xs, target, w) of an accumulation case."""
    d = dims(case)
    xs = [real_x(f'{case.id}/x{k}', case.shape, d['P']) for k in range(n_inputs)]
    w = draw_weights(case.id, [mean_ref(x) for x in xs], d['C'], d['Cr'])
    target = case_rng(case.id, 3).standard_normal(case.shape).astype(F32)
    return dict(xs=xs, target=target, w=w)


# ---------------------------------------------------------------------------------------------------------------- in-graph: hand-over
# p = conv2d(x, ci -> c, 3x3, linear, bias); a = channel_attention(p); out = conv2d(a, c -> co, 3x3, linear, bias)
Handover = namedtuple('Handover', 'id ci c co h w batches pool scale dx dscale no_fusion')


def _h(id, ci, c, co, h, w, batches, pool, scale, dx, no_fusion=False):
    return Handover(id, ci, c, co, h, w, tuple(batches), pool, scale, dx, scale, no_fusion)


# flags: pool_from_producer, scale_in_consumer_load, dx_in_producer_backward (dscale_from_consumer_wgrad follows the second)
HANDOVER = [
    _h('base', 8, 8, 1, 21, 37, (3,), True, True, True),                  # 2 x 2 = 4 tiles: the remainder loop of pool_finish alone
    _h('c4_one_tile', 8, 4, 1, 9, 13, (1,), True, True, True),            # C = 4: 4 of 8 lanes stored; one tile; one instance
    _h('ci2_nine_tiles', 2, 8, 1, 42, 84, (5,), True, True, False),       # 3 x 3 = 9 tiles: one full round of eight, then one; B = 5
    _h('ci5_eight_tiles', 5, 8, 1, 58, 52, (3,), True, True, False),      # 4 x 2 = 8 tiles: the eight-way loop alone
    _h('ci5_c4_co2', 5, 4, 2, 40, 20, (5,), True, True, False),           # 3 x 1 = 3 tiles, C = 4, a two-channel consumer
    _h('sixteen_tiles', 8, 8, 1, 60, 120, (1,), True, True, True),        # 4 x 4 = 16 tiles: two rounds, no remainder
    _h('twelve_tiles', 8, 8, 1, 44, 120, (3,), True, True, True),         # 3 x 4 = 12 tiles: one round, then four
    _h('co_eq_c', 8, 8, 8, 21, 37, (3,), True, False, True),              # the consumer is no stencil: y is stored, from pooled partials
    _h('co_eq_c4', 8, 4, 4, 42, 84, (1,), True, False, True),
    _h('b5_then_b2', 8, 8, 1, 42, 45, (5, 2), True, True, True),          # 3 x 2 = 6 tiles; buffers laid out for 5 samples, then 2 run
    _h('no_fusion', 8, 8, 1, 21, 37, (3,), False, False, False, no_fusion=True),        # DL4DS_NO_TAIL_FUSION=1: three plain passes
]
H_KEYS = ('p/kernel', 'p/bias') + tuple('att/' + k for k in W_KEYS) + ('out/kernel', 'out/bias')


def pool_tiles(h, w):
    """conv2d_narrow_pair_tiles_per_image."""
    return cdiv(w, POOL_TILE_W) * cdiv(h, POOL_TILE_H)


def _pad_pow2(c):
    p = 1
    while p < c:
        p <<= 1
    return p


def expected_flags(ci, c, co):
    """(pool, scale, dx) as ChAttOp::on_prepare decides them for dense, aligned 3x3 linear neighbours: the stencil kernels take a
    layer with pad_pow2(Cin) * pad_pow2(Cout) <= 8 (and a channel affine on float4-loadable channels), the pair kernel Cin <= 8 and
    Cout in {4, 8}."""
    def direct(a, b):
        return _pad_pow2(a) * _pad_pow2(b) <= 8

    def pair(a, b):
        return a <= 8 and b <= 8 and b % 4 == 0
    affine = c % 4 == 0 and c >= 4
    pool = c <= 8 and not direct(ci, c) and pair(ci, c)
    scale = direct(c, co) and affine
    dx = (not direct(ci, c)) and ci <= 8 and c <= 16 and ((direct(c, ci) and affine) or (not direct(c, ci) and pair(c, ci) and affine))
    return pool, scale, dx


@functools.lru_cache(maxsize=None)
def handover_inputs(case):
    """-> dict(x, target, w): x and the targets for the largest batch (smaller batches take the leading samples); w by H_KEYS.
    Order-one biases on the producer give the pooled channels their offsets."""
    B = max(case.batches)
    rng = case_rng(case.id)
    x = (rng.standard_normal((B, case.h, case.w, case.ci)) + _offsets(rng, (B, 1, 1, case.ci))).astype(F32)
    w = {'p/kernel': (rng.standard_normal((3, 3, case.ci, case.c)) * 0.3 / np.sqrt(case.ci)).astype(F32),
         'p/bias': _offsets(rng, (case.c,)).astype(F32),
         'out/kernel': (rng.standard_normal((3, 3, case.c, case.co)) * 0.3).astype(F32),
         'out/bias': _offsets(rng, (case.co,)).astype(F32)}
    p = handover_ref(case, x, w, upto='p')

    def sensitive(att):            # (twice what tests/test_attention_cases.py asserts of the draw that is kept)
        return handover_sensitivity(case, x, dict(w, **{'att/' + k: v for k, v in att.items()})) >= 20 * TOL
    att = draw_weights(case.id, [mean_ref(p)], case.c, case.c // 4, gain=1.5, every_instance=True, accept=sensitive)
    w.update({'att/' + k: v for k, v in att.items()})
    target = rng.standard_normal((B, case.h, case.w, case.co)).astype(F32)
    return dict(x=x, target=target, w=w)


def handover_ref(case, x, w, dy=None, upto=None, drop_tile=None):
    """The float64 composition oracle conv2d -> oracle.models.channel_attention -> oracle conv2d.  -> out; with ``dy`` (out, dX,
    {key: gradient}); ``upto='p'``: the producer's output alone.  ``drop_tile=(ty, tx)``: the forward with that pooling tile's
    contribution missing from every sample's mean (the MLP and the product written out; drop_tile=() is that form unchanged)."""
    import torch
    from oracle import torch_ops as T
    pt = Params({k: _t64(v, True) for k, v in w.items()})
    xt = _t64(x, True)
    p = T.conv2d(xt, pt['p/kernel'], pt['p/bias'])
    if upto == 'p':
        return p.detach().numpy()
    if drop_tile is None:
        a = _att(p, pt, 'att')
    else:
        total = p.sum(dim=(1, 2))
        if drop_tile:
            ty, tx = drop_tile
            total = total - p[:, ty * POOL_TILE_H:(ty + 1) * POOL_TILE_H, tx * POOL_TILE_W:(tx + 1) * POOL_TILE_W].sum(dim=(1, 2))
        mean = total / (case.h * case.w)
        hid = torch.relu(mean @ pt['att/conv1/kernel'].reshape(case.c, -1) + pt['att/conv1/bias'])
        s = torch.sigmoid(hid @ pt['att/conv2/kernel'].reshape(-1, case.c) + pt['att/conv2/bias'])
        a = p * s[:, None, None, :]
    out = T.conv2d(a, pt['out/kernel'], pt['out/bias'])
    if dy is None:
        return out.detach().numpy()
    (out * _t64(dy)).sum().backward()
    return out.detach().numpy(), xt.grad.numpy(), {k: pt[k].grad.numpy() for k in H_KEYS}


def handover_sensitivity(case, x=None, w=None):
    """The smallest rel_err, over the pooling tiles of the image, between the reference output and the reference output with that
    tile missing from the mean (of the case's own inputs unless given)."""
    if x is None:
        inp = handover_inputs(case)
        x, w = inp['x'], inp['w']
    full = handover_ref(case, x, w)
    worst = np.inf
    for ty in range(cdiv(case.h, POOL_TILE_H)):
        for tx in range(cdiv(case.w, POOL_TILE_W)):
            worst = min(worst, rel_err(handover_ref(case, x, w, drop_tile=(ty, tx)), full))
    return worst
