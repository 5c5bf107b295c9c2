"""Cases and a restatement of the host-side tiling arithmetic of tests/test_gpu_convlstm.py (not a test module; needs no GPU).

A case is one ConvLSTM2D(F, KS, 'same', return_sequences=True) [+ ReLU] op on a graph input of shape (B, T, H, W, C), run forward
and backward once per ``Run`` = the test hooks in force (csrc/convlstm_seq.hip):

  tr   DL4DS_CONVLSTM_SEQ_TR   None: the library's own choice; 2 / 4: that many pixel rows per wave in BOTH directions
  cap  DL4DS_SEQ_GRID          None: min(tiles, CUs) workgroups; n: at most n

``form`` restates, for a given number of CUs, what the launch wrappers of csrc/convlstm_seq.hip derive from a shape and the hooks:

  convlstm_seq_supported   KS in {3, 5}, F in {4, 8, 16}, not (5, 16); not under DL4DS_NO_CONVLSTM_SEQ / DL4DS_AUX_STREAM
  seq_tr                   backward: 2 while there are fewer than 2 * CUs 16 x 16 tiles and H > 8, else 4; forward: 4
  tiles                    tiles_x = ceil(W / 16), tiles_y = ceil(H / (4 tr)), ntiles = tiles_x * tiles_y * B
  seq_grid                 min(ntiles, max(CUs - reserve, 8), cap)
  my_tile(i, grid)         i * grid + lin, lin = blockIdx for grid & 7 != 0 ('linear'), else the XCD permutation
                           (blockIdx & 7) * (grid >> 3) + (blockIdx >> 3) ('permuted')
  rounds                   ceil(ntiles / grid): the trips of the tile loop that reach a tile; in a ragged last round the blocks whose
                           tile index is past the end skip it, and under the permutation those are not the last blocks of the grid
  single                   forward only: ntiles <= grid, the cell state stays in registers; otherwise it is reloaded from C
  pair                     backward, F = 8, tr = 2: two pixel rows share one accumulator (the PAIR filter layout)

tests/test_convlstm_cases.py holds the restatement to the source text and proves that the tables below reach every form they are
listed for at 256 CUs; the GPU tests evaluate it for the CU count of the device they run on and compare with the profiler tags.
"""
import os
import re
from collections import namedtuple

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SOURCE = os.path.join(ROOT, 'dl4ds_amd', 'csrc', 'convlstm_seq.hip')

PAIRS = [(3, 4), (3, 8), (3, 16), (5, 4), (5, 8)]          # every (KS, F) the persistent kernel is instantiated for
CINS = (1, 2, 5, 8)
REFERENCE_CUS = 256                                        # MI355X; the CPU test proves the conditions for this count

Case = namedtuple('Case', 'id B T H W C F KS relu')
Run = namedtuple('Run', 'tr cap')
Item = namedtuple('Item', 'case runs')
Form = namedtuple('Form', 'tr tiles_x tiles_y ntiles grid rounds mapping single pair')

NO_HOOK = Run(None, None)


def cdiv(a, b):
    return -(-a // b)


# ---------------------------------------------------------------------------------------------------- the launch wrappers, restated
def supported(KS, F, H, W, B, env=()):
    if 'DL4DS_NO_CONVLSTM_SEQ' in env or 'DL4DS_AUX_STREAM' in env:
        return False
    if KS not in (3, 5) or F not in (4, 8, 16):
        return False
    if F == 16 and KS == 5:
        return False
    tiles = cdiv(H, 16) * cdiv(W, 16) * B
    return 1 <= tiles < (1 << 24)


def seq_tr(H, W, B, backward, cus, hook=None):
    if hook is not None:
        return 2 if int(hook) == 2 else 4
    t16 = cdiv(H, 16) * cdiv(W, 16) * B
    return 2 if (backward and t16 < 2 * max(cus, 8) and H > 8) else 4


def my_tile(i, grid, block):
    per = grid >> 3
    lin = block if (grid & 7) else (block & 7) * per + (block >> 3)
    return i * grid + lin


def form(case, backward, cus=REFERENCE_CUS, run=NO_HOOK, reserve=0):
    tr = seq_tr(case.H, case.W, case.B, backward, cus, run.tr)
    tiles_x, tiles_y = cdiv(case.W, 16), cdiv(case.H, 4 * tr)
    ntiles = tiles_x * tiles_y * case.B
    grid = min(ntiles, max(cus - reserve, 8))
    if run.cap is not None and run.cap >= 1:
        grid = min(grid, run.cap)
    return Form(tr, tiles_x, tiles_y, ntiles, grid, cdiv(ntiles, grid), 'linear' if grid & 7 else 'permuted',
                (not backward) and ntiles <= grid, backward and case.F == 8 and tr == 2)


def schedule(ntiles, grid):
    """The tile loop of both kernels for every block: -> (tiles[block] in the order the block takes them, skipped[block] = the
    trips it passes over because its tile index is past the end while the round still holds tiles)."""
    tiles, skipped = [[] for _ in range(grid)], [0] * grid
    for b in range(grid):
        it = 0
        while True:
            tl = my_tile(it, grid, b)
            if tl >= ntiles:
                if it * grid >= ntiles:
                    break
                skipped[b] += 1
            else:
                tiles[b].append(tl)
            it += 1
    return tiles, skipped


def flag_words(H, W, B):                # convlstm_seq_flag_bytes / 8: one 64-bit word per tile of the finest tiling
    return cdiv(H, 8) * cdiv(W, 16) * B


def flag_quota_words(H, W):             # ConvLSTMOp::flag_quota (floats per sample) as 64-bit words
    return (2 * cdiv(H, 8) * cdiv(W, 16) + 64) // 2


def tag(case, backward, f, forms=True):
    """The profiler tag of a launch; ``forms``: with the suffix DL4DS_SEQ_TAG_FORMS=1 adds."""
    base = f'convlstm_seq_{"bwd" if backward else "fwd"}<{case.KS},{case.F}>'
    return base + (f'tr{f.tr}g{f.grid}n{f.ntiles}' if forms else '')


def expected_tags(case, cus, run=NO_HOOK):
    return {tag(case, False, form(case, False, cus, run)), tag(case, True, form(case, True, cus, run))}


def source_text():
    return re.sub(r'\s+', '', open(SOURCE).read())


# ------------------------------------------------------------------------------------------------------------------------- cases
def _case(shape, C, F, KS, relu, name=None):
    B, T, H, W = shape
    return Case(name or f'b{B}t{T}_{H}x{W}_c{C}_k{KS}f{F}{"_relu" if relu else ""}', B, T, H, W, C, F, KS, bool(relu))


SHAPE_A = (2, 3, 37, 23)        # 3 x 2 x 2 = 12 tiles of 16 x 16, 5 x 2 x 2 = 20 of 8 x 16; ragged right and bottom edges
SHAPE_B = (3, 3, 33, 40)        # 3 x 3 x 3 = 27 tiles of 16 x 16, 5 x 3 x 3 = 45 of 8 x 16
CAPS = (1, 5, 16)

# every pair on shape A: the library's own tilings (forward 16 x 16, backward 8 x 16) and 16 x 16 in both directions, each without
# a cap and under the three caps
A_CASES = [_case(SHAPE_A, 1, 4, 3, False), _case(SHAPE_A, 8, 8, 3, True), _case(SHAPE_A, 2, 16, 3, True),
           _case(SHAPE_A, 5, 4, 5, False), _case(SHAPE_A, 1, 8, 5, True)]
A_RUNS = [NO_HOOK] + [Run(None, c) for c in CAPS] + [Run(4, None)] + [Run(4, c) for c in CAPS]
B_CASES = [_case(SHAPE_B, 2, 8, 5, True), _case(SHAPE_B, 5, 16, 3, False)]
B_RUNS = [NO_HOOK, Run(None, 5), Run(None, 16), Run(4, None), Run(4, 16), Run(2, None), Run(2, 16)]

# H <= 8: 16 x 16 tiles backward without a hook; H below the kernel size, W below and above one tile
LOW_CASES = [_case((2, 3, 8, 20), 2, 16, 3, True), _case((2, 3, 8, 20), 8, 8, 3, False), _case((1, 2, 5, 7), 1, 8, 5, False),
             _case((2, 3, 3, 40), 5, 4, 5, True), _case((2, 3, 3, 40), 2, 4, 3, False)]
LOW_RUNS = [NO_HOOK, Run(None, 1)]

# at least 2 * 256 tiles of 16 x 16 with no hook at all: several rounds forward, 16 x 16 tiles backward, a ragged last round
LARGE = _case((57, 2, 33, 33), 1, 4, 3, True)
LARGE_RUNS = [NO_HOOK]

SHORT_CASES = [_case((2, t, 19, 23), c, f, ks, relu) for t in (1, 2) for c, f, ks, relu in ((2, 8, 3, True), (5, 4, 5, False))]
SHORT_RUNS = [NO_HOOK, Run(None, 5), Run(4, None), Run(4, 5)]

SEQ_ITEMS = ([Item(c, A_RUNS) for c in A_CASES] + [Item(c, B_RUNS) for c in B_CASES] + [Item(c, LOW_RUNS) for c in LOW_CASES]
             + [Item(LARGE, LARGE_RUNS)] + [Item(c, SHORT_RUNS) for c in SHORT_CASES])

# the step-by-step path: switched on for three supported pairs on shape A (the cases above, so the references are shared), and
# taken by itself for a filter count the persistent kernel is not built for
FALLBACK_SWITCHED = [c for c in A_CASES if (c.KS, c.F) in ((3, 8), (5, 4), (3, 16))]
FALLBACK_UNSUPPORTED = _case(SHAPE_A, 2, 12, 3, True)

# flags across launches: one model planned for batch 3, (batch, run) after (batch, run) on the same slab
FLAGS_CASE = B_CASES[0]
FLAGS_STEPS = [(3, NO_HOOK), (3, Run(4, 1)), (3, Run(2, 5)), (1, NO_HOOK), (3, NO_HOOK)]


def with_batch(case, B):
    return case._replace(B=B)


# what the issue lists for 256 CUs, by hand: (case index, run) -> ((tr, ntiles, grid, rounds, mapping) forward, ... backward)
HAND_CHECKED = {
    ('A', NO_HOOK): ((4, 12, 12, 1, 'linear'), (2, 20, 20, 1, 'linear')),
    ('A', Run(None, 1)): ((4, 12, 1, 12, 'linear'), (2, 20, 1, 20, 'linear')),
    ('A', Run(None, 5)): ((4, 12, 5, 3, 'linear'), (2, 20, 5, 4, 'linear')),
    ('A', Run(None, 16)): ((4, 12, 12, 1, 'linear'), (2, 20, 16, 2, 'permuted')),
    ('A', Run(4, None)): ((4, 12, 12, 1, 'linear'), (4, 12, 12, 1, 'linear')),
    ('A', Run(4, 5)): ((4, 12, 5, 3, 'linear'), (4, 12, 5, 3, 'linear')),
    ('B', NO_HOOK): ((4, 27, 27, 1, 'linear'), (2, 45, 45, 1, 'linear')),
    ('B', Run(None, 16)): ((4, 27, 16, 2, 'permuted'), (2, 45, 16, 3, 'permuted')),
    ('B', Run(4, 16)): ((4, 27, 16, 2, 'permuted'), (4, 27, 16, 2, 'permuted')),
    ('LARGE', NO_HOOK): ((4, 513, 256, 3, 'permuted'), (4, 513, 256, 3, 'permuted')),
}


# ------------------------------------------------------------------------------------------------------- inputs and fp64 reference
def oracle_call(x, w, y, relu):
    """-> call(dtype) for tests.parity.banded_reference: MSE loss of the oracle's ConvLSTM2D [+ ReLU] against ``y`` with the gradients
    of the input, both kernels and the bias."""
    import numpy as np
    import torch
    from oracle import torch_ops as T

    def call(dt):
        t = lambda a: torch.tensor(np.asarray(a, dt), requires_grad=True)
        xt, kt, ut, bt = t(x), t(w['lstm/kernel']), t(w['lstm/recurrent_kernel']), t(w['lstm/bias'])
        out = T.conv_lstm2d(xt, kt, ut, bt)
        if relu:
            out = T.relu(out)
        loss = ((out - torch.tensor(y.astype(dt))) ** 2).mean()
        gx, gk, gu, gb_ = torch.autograd.grad(loss, [xt, kt, ut, bt])
        return float(loss), {'x': gx, 'lstm/kernel': gk, 'lstm/recurrent_kernel': gu, 'lstm/bias': gb_}, out.detach()
    return call


def oracle_output(x, w, relu):
    import numpy as np
    import torch
    from oracle import torch_ops as T
    with torch.no_grad():
        t64 = lambda a: torch.tensor(np.asarray(a, np.float64))
        o64 = T.conv_lstm2d(t64(x), t64(w['lstm/kernel']), t64(w['lstm/recurrent_kernel']), t64(w['lstm/bias']))
        return (T.relu(o64) if relu else o64).numpy()


def weights(case):
    """Weights of a case as a function of (C, F, KS) alone, so that cases which differ only in their batch or grid share them: the
    input kernel at twice Glorot's scale and inputs of 1.5 sigma (the hard sigmoids saturate in places: both clip branches of the
    backward pass run), a recurrent kernel of orthogonal-initialiser size, unit forget bias, 0.1 sigma on every bias."""
    import numpy as np
    import zlib
    r = np.random.default_rng(zlib.crc32(f'w{case.C}_{case.F}_{case.KS}'.encode()))
    ks, c, f = case.KS, case.C, case.F
    lim = np.sqrt(6.0 / (ks * ks * (c + 4 * f)))
    bias = 0.1 * r.standard_normal(4 * f)
    bias[f:2 * f] += 1.0
    return {'lstm/kernel': (2.0 * r.uniform(-lim, lim, (ks, ks, c, 4 * f))).astype(np.float32),
            'lstm/recurrent_kernel': (r.standard_normal((ks, ks, f, 4 * f)) / np.sqrt(ks * ks * f)).astype(np.float32),
            'lstm/bias': bias.astype(np.float32)}


_PROBLEMS = {}


def problem(case):
    """-> dict(w, x, y, ref) of a case, computed once per session and shared by every test that runs the case (read-only)."""
    import numpy as np
    import zlib
    from tests.parity import banded_reference, targets_clear_of_the_kink
    key = case._replace(id='')
    if key not in _PROBLEMS:
        r = np.random.default_rng(zlib.crc32(repr(tuple(key)).encode()))
        w = weights(case)
        x = (1.5 * r.standard_normal((case.B, case.T, case.H, case.W, case.C))).astype(np.float32)
        y = targets_clear_of_the_kink(oracle_output(x, w, case.relu), r)
        ref = banded_reference(oracle_call(x, w, y, case.relu))
        for a in [x, y, *w.values(), ref['pred'], *ref['grads'].values(), *ref['band'].values(), *ref['noise'].values()]:
            a.setflags(write=False)
        _PROBLEMS[key] = dict(w=w, x=x, y=y, ref=ref)
    return _PROBLEMS[key]
