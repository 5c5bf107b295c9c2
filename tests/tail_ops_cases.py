"""Case tables and input generators of tests/test_gpu_tail_ops.py (not a test module; needs no GPU).

A case is a function ``build(g, inputs) -> out`` that runs unchanged on ``dl4ds_amd.graph.GraphBuilder`` and on
``tests.tail_ops_ref.RefBuilder``, the specification of its graph inputs, a batch size and a seed.  Families:

  rec_tail   RecTailOp (csrc/graph_ops4.hip).  Staged form (HW % 256 == 0): nblk = B HW / 256 partial tiles, G = min(nblk, 64) groups in
             rec_tail_wsum_kernel, the 8-wide loop plus scalar tail of rec_tail_finish_kernel's tile().  Plain form: every other grid
             (and DL4DS_REC_TAIL_NO_STAGED=1, a test hook read when the op is created).
  folded     FoldedConvOp (csrc/graph_ops3.hip), (ks, d2s, Cin, Cm, Co); K R2 = ks^2 Cin d2s^2 terms per lane loop of unfold_w2_kernel.
  deconv     ConvTOp / csrc/deconv.hip, (KS, s): virtual kernel KV = 5 for (9, 2), 3 for (9, 4), (4, 2), (6, 3), 1 for (2, 2), (3, 3).
  localconv  LocalConvOp: the compiled-in 2 -> 2 kernel and the run-time channel counts.

Inputs and ReLU kinks.  ``make(case)`` draws inputs, weights (non-zero biases) and the MSE target from the case's seed.  A float64
pre-activation that is ~0 may take the other ReLU branch in fp32, which changes gradients legitimately, so every ReLU of the
reference must keep |v| >= DELTA max|v| with NO element excluded.  A search over seeds alone cannot deliver that for the grids the
kernels need (the nblk = 72 case has 5e5 pre-activations, ~150 of them inside the margin for any seed), so the generator redraws the
input pixels under an offending pre-activation -- from the seed's own stream, looking at the reference alone -- until none is left;
inputs that feed a ReLU directly (the identity convolution of ``relu_id``) are drawn with 0.3 <= |x| < 1.5.  On top of that
``find_seed`` takes the first of 32 seeds for which every ReLU has MIN_SIDE of its elements on either side; the chosen seeds are the
literals of SEEDS (every case not listed there: seed 0).  tests/test_tail_ops_cases.py holds all of this for every case."""
import functools
import zlib
from collections import namedtuple

import numpy as np

from tests import tail_ops_ref as R

F32 = np.float32
REC_TAIL_SHAPES = [(16, 8, 13), (8, 8, 9), (16, 8, 8), (8, 8, 8)]
WSUM_GROUPS = 64

# inputs: ((nmul, H, W, C), requires_grad, away) per graph input; env: test hooks set while the graph is built;
# tags: {tag: launches} the forward + backward pass must show; absent: tags it must not show; wgrad1x1: the launches of the ordinary
# weight-gradient kernels (plain rec_tail: three per application, plus one per convolution of the variant); raises: the builder must refuse the graph with this message
Case = namedtuple('Case', 'id family build inputs batch tags absent wgrad1x1 env raises', defaults=((), 0, (), None))


def relu_id(g, x, name):
    """tests/test_gpu_graph_ops.py::_relu_id: the bias-free identity ReLU convolution ('id*' kernels are identities)."""
    return g.conv2d(x, name, x.C, 1, use_bias=False, activation='relu')


# ---------------------------------------------------------------------------------------------------------------- rec_tail
def _rt_build(variant, T, co, g, xs):
    if variant == 'twice':
        x1, x2, s = xs
        return g.add(g.rec_tail(x1, s, T, co), g.rec_tail(x2, s, T, co))
    x, s = xs
    if variant == 'mask':
        return g.rec_tail(relu_id(g, x, 'idx'), relu_id(g, s, 'ids'), T, co)
    r = g.rec_tail(x, s, T, co)
    if variant == 'second':           # both consumers are created after the rec_tail: their backward runs first, rec_tail accumulates
        a = g.add(r, g.conv2d(x, 'cx', co, 1))
        return g.concat([a, g.repeat_time(g.conv2d(s, 'cs', 3, 1), T)])
    return r


def rec_tail_case(B, T, H, W, chans=(16, 8, 13), variant='base', no_staged=False):
    cx, cs, co = chans
    staged = (H * W) % 256 == 0 and not no_staged
    n = 2 if variant == 'twice' else 1
    away = variant == 'mask'
    inputs = tuple(((T, H, W, cx), variant != 'nodx', away) for _ in range(n)) + (((1, H, W, cs), True, away),)
    tags = {'rec_tail_fwd': n, 'rec_tail_bwd': n, 'rec_tail_finish': n}
    if staged:
        tags['rec_tail_wsum'] = n
    cid = f'rt_{cx}_{cs}_{co}_b{B}t{T}_{H}x{W}_{variant}' + ('_nostaged' if no_staged else '')
    return Case(cid, 'rec_tail', functools.partial(_rt_build, variant, T, co), inputs, B, tuple(sorted(tags.items())),
                () if staged else ('rec_tail_wsum',), 0 if staged else 3 * n + (2 if variant in ('mask', 'second') else 0),
                (('DL4DS_REC_TAIL_NO_STAGED', '1'),) if no_staged else ())


def rec_tail_geometry(case):
    (T, H, W, _), _, _ = case.inputs[0]
    HW = H * W
    staged = HW % 256 == 0 and not case.env
    nblk = case.batch * HW // 256 if staged else 0
    first = np.arange(0, case.batch * HW, 256)                                   # a plain block's first and last grid point
    last = np.minimum(first + 255, case.batch * HW - 1)
    return dict(staged=staged, HW=HW, T=T, nblk=nblk, G=min(nblk, WSUM_GROUPS), samples_per_block=int((last // HW - first // HW).max()) + 1)


RT_STAGED = [(2, 3, 16, 16), (1, 2, 16, 32), (3, 2, 24, 32), (3, 2, 32, 192), (1, 1, 16, 16)]
RT_PLAIN = [(20, 2, 5, 6), (2, 3, 17, 17), (2, 2, 3, 85), (1, 2, 1, 257), (3, 1, 12, 10)]
RT_FLAG_GRIDS = [(2, 3, 16, 16), (3, 2, 12, 10)]
RT_VARIANTS = ['nodx', 'mask', 'second', 'twice']
RT_STALE = rec_tail_case(3, 2, 16, 16), rec_tail_case(3, 2, 9, 7)
REC_TAIL_CASES = (
    [rec_tail_case(*grid, chans=c) for grid in (RT_STAGED[0], RT_PLAIN[1]) for c in REC_TAIL_SHAPES]
    + [rec_tail_case(*grid, chans=c) for grid in RT_STAGED[1:] + RT_PLAIN[:1] + RT_PLAIN[2:] for c in (REC_TAIL_SHAPES[0], REC_TAIL_SHAPES[3])]
    + [rec_tail_case(*RT_STAGED[0], chans=c, no_staged=True) for c in (REC_TAIL_SHAPES[0], REC_TAIL_SHAPES[3])]
    + [rec_tail_case(*grid, variant=v) for grid in RT_FLAG_GRIDS for v in RT_VARIANTS])


# ---------------------------------------------------------------------------------------------------------------- folded conv
def _fold_build(ks, d2s, cm, co, act, variant, g, xs):
    x, aux = xs[0], (xs[1] if len(xs) > 1 and variant not in ('shared_before', 'shared_after') else None)
    r = d2s if d2s > 1 else 1
    if variant == 'mask':
        return g.conv2d_folded(relu_id(g, x, 'idx'), 'c1', cm, ks, d2s, 'c2', co, act, aux=relu_id(g, aux, 'ida'))
    if variant == 'shared_before':            # the spc block's order: the plain convolution first (its backward accumulates)
        p = g.conv2d(xs[1], 'c1', r * r * cm, ks, d2s=d2s)
        f = g.conv2d_folded(x, 'c1', cm, ks, d2s, 'c2', co, act)
        return g.add(f, g.conv2d(p, 'cq', co, 1))
    f = g.conv2d_folded(x, 'c1', cm, ks, d2s, 'c2', co, act, aux=aux)
    if variant == 'shared_after':             # the plain convolution's backward runs first: unfold_w1_kernel takes acc_w = 1
        p = g.conv2d(xs[1], 'c1', r * r * cm, ks, d2s=d2s)
        return g.add(f, g.conv2d(p, 'cq', co, 1))
    if variant == 'second':                   # later-created consumers of x and aux: the folded op accumulates both input gradients
        f = g.add(f, g.conv2d(x, 'cx', r * r * co, 1, d2s=d2s))
        return g.add(f, g.conv2d(aux, 'ca', co, 1))
    return f


def folded_case(geom, grid, cs=0, act='relu', variant='base', N=2):
    ks, d2s, cin, cm, co = geom
    h, w = grid
    r = d2s if d2s > 1 else 1
    inputs = (((1, h, w, cin), True, variant == 'mask'),)
    if cs:
        inputs += (((1, h * r, w * r, cs), True, variant == 'mask'),)
    if variant.startswith('shared'):
        inputs += (((1, h, w, cin), True, False),)
    cid = f'fold_k{ks}d{d2s}_{cin}_{cm}_{co}_{h}x{w}_aux{cs}_{act}_{variant}'
    raises = 'Cout % 4 == 0' if cs and co % 4 else None
    return Case(cid, 'folded', functools.partial(_fold_build, ks, d2s, cm, co, act, variant), inputs, N,
                (('fold_weights', 1), ('unfold_weight_grads', 1)), raises=raises)


FOLD_GEOMS = [(3, 2, 8, 8, 8), (3, 0, 8, 6, 3), (1, 0, 2, 5, 1), (3, 2, 4, 3, 1), (3, 5, 2, 2, 1), (5, 2, 6, 8, 8)]
FOLD_GRIDS = [((9, 7), 2), ((16, 16), 3)]            # (LR grid, channels of the auxiliary tensor on it)
FOLD_ACT = 'tanh'                                   # the non-ReLU activation: an Activation op behind the folded convolution
_FOLD_ALL = [folded_case(gm, grid, cs, act) for gm in FOLD_GEOMS for grid, c in FOLD_GRIDS for cs in (0, c) for act in ('relu', FOLD_ACT)]
FOLDED_CASES = [c for c in _FOLD_ALL if not c.raises] + [
    folded_case(FOLD_GEOMS[0], (9, 7), 2, 'relu', 'mask'), folded_case(FOLD_GEOMS[5], (16, 16), 3, FOLD_ACT, 'mask'),
    folded_case(FOLD_GEOMS[0], (9, 7), 2, 'relu', 'second'), folded_case(FOLD_GEOMS[5], (16, 16), 3, FOLD_ACT, 'second'),
    folded_case(FOLD_GEOMS[0], (9, 7), 0, 'relu', 'shared_before'), folded_case(FOLD_GEOMS[3], (9, 7), 0, 'relu', 'shared_before'),
    folded_case(FOLD_GEOMS[0], (9, 7), 0, 'relu', 'shared_after'), folded_case(FOLD_GEOMS[1], (16, 16), 0, FOLD_ACT, 'shared_after')]
# the auxiliary form stores through float4 rows: the builder refuses it for Co % 4 != 0 (csrc/graph_ops3.hip: g_conv2d_folded)
FOLDED_REFUSED = [c for c in _FOLD_ALL if c.raises and c.id.endswith('relu_base')]


# ---------------------------------------------------------------------------------------------------------------- conv2d_transpose
def _dc_build(ks, s, co, variant, g, xs):
    x = xs[0]
    if variant == 'relu_out':                 # ReLU on the graph output: the explicit bias_act_backward
        return g.conv2d_transpose(x, 'dc', co, ks, s, activation='relu')
    if variant == 'relu_conv':                # ReLU in front of a convolution: grad_masked
        return g.conv2d(g.conv2d_transpose(x, 'dc', co, ks, s, activation='relu'), 'c', 3, 3)
    if variant == 'mask':                     # dgrad with relu_mask
        return g.conv2d_transpose(relu_id(g, x, 'idx'), 'dc', co, ks, s)
    if variant == 'second':                   # a later-created consumer of x: dgrad accumulates
        return g.add(g.conv2d_transpose(x, 'dc', co, ks, s), g.conv2d_transpose(x, 'dc2', co, s, s))
    if variant == 'twice':                    # deconv_block(scale=8): one variable applied twice in a row, wgrad accumulates
        return g.conv2d_transpose(g.conv2d_transpose(x, 'dc', co, ks, s), 'dc', co, ks, s)
    if variant == 'concat':
        # the output is a channel slice of the Concatenate's buffer (out.ld > C), its gradient a slice of the Concatenate's (dz.ld > C).
        # Graph::plan_concat_aliases / plan_grad_aliases take both only for a 16-channel concatenation of quad-aligned slices that are
        # no graph inputs, whose result is no graph output: 8 + 8 channels, the partner behind a convolution, a convolution behind.
        k = g.concat([g.conv2d_transpose(x, 'dc', co, ks, s), g.conv2d(xs[1], 'cz', 8, 3)])
        return g.conv2d(k, 'c', 3, 3)
    return g.conv2d_transpose(x, 'dc', co, ks, s)


def deconv_case(geom, chans, grid, variant='base', N=2):
    ks, s = geom
    ci, co = chans
    h, w = grid
    inputs = (((1, h, w, ci), True, variant == 'mask'),)
    if variant == 'concat':
        assert co == 8
        inputs += (((1, h * s, w * s, 8), True, False),)
    # with both aliases taken no copy kernel runs in either direction
    absent = ('concat_join', 'concat_split', 'view_axpy', 'view_axpy_masked') if variant == 'concat' else ()
    return Case(f'dc_k{ks}s{s}_{ci}_{co}_{h}x{w}_{variant}', 'deconv', functools.partial(_dc_build, ks, s, co, variant), inputs, N,
                (('dgrad_weights', 2 if variant in ('second', 'twice') else 1),), absent)


DC_GEOMS = [(9, 2), (9, 4), (4, 2), (2, 2), (3, 3), (6, 3)]
DC_CHANS = [(4, 3), (16, 8), (5, 2)]
DC_GRIDS = [(6, 7), (4, 5)]
DC_VARIANTS = ['relu_out', 'relu_conv', 'mask', 'second']
DECONV_CASES = (
    [deconv_case(gm, ch, grid) for gm in DC_GEOMS for ch in DC_CHANS for grid in DC_GRIDS]
    + [deconv_case(gm, DC_CHANS[(i + j) % 3], DC_GRIDS[(i + j) % 2], v) for i, gm in enumerate(DC_GEOMS) for j, v in enumerate(DC_VARIANTS)]
    + [deconv_case(gm, (DC_CHANS[i % 3][0], 8), DC_GRIDS[i % 2], 'concat') for i, gm in enumerate(DC_GEOMS)]
    + [deconv_case(gm, (c, c), DC_GRIDS[i % 2], 'twice') for i, (gm, c) in enumerate(zip(DC_GEOMS, (4, 5, 8, 5, 4, 3)))])
# dl4ds_op_conv2d_transpose_dgrad / _wgrad with accumulate = 1: (KS, s), (Cin, Cout), grid
DC_DIRECT = [((9, 2), (4, 3), (6, 7)), ((4, 2), (16, 8), (4, 5)), ((2, 2), (5, 2), (6, 7)), ((6, 3), (4, 3), (4, 5)), ((9, 4), (5, 2), (4, 5))]


# ---------------------------------------------------------------------------------------------------------------- localconv
def _lc_build(f, variant, g, xs):
    if variant == 'twice':                    # one pair of variables on two inputs: accumulate_dw
        return g.add(g.localconv(xs[0], 'lc', f), g.localconv(xs[1], 'lc', f))
    y = g.localconv(xs[0], 'lc', f, use_bias=variant != 'nobias')
    if variant == 'second':                   # a later-created consumer of x: accumulate_dx
        return g.add(y, g.conv2d(xs[0], 'cx', f, 1))
    return y


def localconv_case(cf, N, grid, variant='base'):
    c, f = cf
    h, w = grid
    inputs = (((1, h, w, c), True, False),) * (2 if variant == 'twice' else 1)
    n = 2 if variant == 'twice' else 1
    return Case(f'lc_{c}_{f}_n{N}_{h}x{w}_{variant}', 'localconv', functools.partial(_lc_build, f, variant), inputs, N,
                (('localconv_fwd', n), ('localconv_bwd', n)))


LC_CHANS = [(2, 2), (3, 2), (8, 8), (1, 5)]
LC_BATCH = [1, 5, 13]
LC_GRIDS = [(1, 1), (3, 2), (9, 11)]
LOCALCONV_CASES = (
    [localconv_case(cf, n, grid, v) for cf in LC_CHANS for n in LC_BATCH for grid in LC_GRIDS for v in ('base', 'nobias')]
    + [localconv_case(cf, n, grid, v) for cf in LC_CHANS for n, grid in ((5, (3, 2)), (13, (9, 11))) for v in ('second', 'twice')])

TABLES = {'rec_tail': REC_TAIL_CASES, 'folded': FOLDED_CASES, 'deconv': DECONV_CASES, 'localconv': LOCALCONV_CASES}
ALL_CASES = [c for t in TABLES.values() for c in t] + list(RT_STALE)

# ---------------------------------------------------------------------------------------------------------------- inputs
SEED_TRIES = 32
# the seed find_seed chooses: 0 for every case but the ones listed here (tests/test_tail_ops_cases.py repeats the search for every case
# and holds it to this table)
SEEDS = {
}


def seed_of(case):
    return SEEDS.get(case.id, 0)


def _rng(name, seed):
    return np.random.default_rng([zlib.crc32(name.encode()), seed])


def weight_of(seed):
    def get(name, shape):
        r = _rng(name, seed)
        if name.startswith('id'):                                   # relu_id
            return np.eye(shape[-1], dtype=F32).reshape(shape)
        if name.endswith('bias'):
            return (r.choice([-1.0, 1.0], shape) * r.uniform(0.1, 0.5, shape)).astype(F32)
        if name.startswith('dc'):                                   # (KS, KS, Cout, Cin): about (KS / s)^2 Cin terms per output
            fan = shape[0] * shape[1] * shape[3] / 4.0
        elif 'localconv' in name or name.startswith('lc'):          # (H, W, C, F)
            fan = shape[2]
        else:
            fan = int(np.prod(shape[:-1]))
        return (r.standard_normal(shape) / np.sqrt(fan)).astype(F32)
    return get


def _draw(r, shape, away):
    if away:
        return (r.choice([-1.0, 1.0], shape) * r.uniform(0.3, 1.5, shape)).astype(F32)
    return r.standard_normal(shape).astype(F32)


def _offenders(relus, arrays, specs):
    """The pixels of every input under a pre-activation inside the margin -> [boolean (N, H, W) mask or None per input]."""
    masks = [None] * len(arrays)
    for name, v in relus:
        bad = (np.abs(v) < R.DELTA * np.abs(v).max()).any(axis=-1)
        if not bad.any():
            continue
        n, i, j = np.nonzero(bad)
        hit = False
        for k, ((nmul, H, W, C), _, _) in enumerate(specs):
            a = arrays[k].reshape(-1, H, W, C)
            if a.shape[0] != v.shape[0]:
                continue
            hit = True
            if masks[k] is None:
                masks[k] = np.zeros(a.shape[:3], bool)
            masks[k][n, i * H // v.shape[1], j * W // v.shape[2]] = True
        assert hit, f'{name}: no input on this pre-activation\'s batch axis to redraw'
    return masks


def generate(case, seed, rounds=60):
    """-> dict(arrays [float32 (B, [T,] H, W, C) per input], target, seed, rounds); see the module docstring."""
    r = _rng('inputs/' + case.id, seed)
    B = case.batch
    arrays = [_draw(r, (B,) + (s[1:] if s[0] == 1 else s), away) for s, _, away in case.inputs]
    w = weight_of(seed)
    for it in range(rounds):
        res = R.run(case.build, case.inputs, arrays, w)
        masks = _offenders(res['relus'], arrays, case.inputs)
        if all(m is None for m in masks):
            break
        for a, m, (s, _, away) in zip(arrays, masks, case.inputs):
            if m is not None:
                a.reshape((-1,) + s[1:])[m] = _draw(r, (int(m.sum()), s[3]), away)
    else:
        raise AssertionError(f'{case.id}: pre-activations inside the margin after {rounds} rounds')
    target = r.standard_normal(res['y'].shape).astype(F32)
    return dict(arrays=arrays, target=target, seed=seed, rounds=it)


def sides_ok(relus):
    return all(R.MIN_SIDE <= pos <= 1.0 - R.MIN_SIDE for _, _, pos in R.margin_report(relus))


def find_seed(case):
    """The first of SEED_TRIES seeds whose inputs give every ReLU of the reference MIN_SIDE of its elements on either side."""
    for seed in range(SEED_TRIES):
        d = generate(case, seed)
        if sides_ok(R.run(case.build, case.inputs, d['arrays'], weight_of(seed))['relus']):
            return seed
    raise AssertionError(f'{case.id}: no seed in {SEED_TRIES} tries; shrink the case')


@functools.lru_cache(maxsize=None)
def make(case):
    """-> dict(arrays, target, w (the weight generator), ref (tests.tail_ops_ref.run with gradients)); read-only."""
    seed = seed_of(case)
    d = generate(case, seed)
    d['w'] = weight_of(seed)
    d['ref'] = R.run(case.build, case.inputs, d['arrays'], d['w'], d['target'])
    for a in d['arrays'] + [d['target']]:
        a.setflags(write=False)
    return d


def first_samples(case, d, n):
    """The case on its first ``n`` samples -> (arrays, target, reference)."""
    arrays = [a[:n] for a in d['arrays']]
    target = d['target'].reshape((case.batch, -1) + d['target'].shape[1:])[:n].reshape((-1,) + d['target'].shape[1:])
    return arrays, target, R.run(case.build, case.inputs, arrays, d['w'], target)
