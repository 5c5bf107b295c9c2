"""The persistent ConvLSTM kernel (csrc/convlstm_seq.hip) form by form -- runs on MI355X only.

tests/test_gpu_ops.py::test_conv_lstm2d reaches one tile per workgroup, 8 x 16 tiles backward and sequences of three steps and more.
Here every (kernel size, filters) pair also runs with several tiles per workgroup under both tile-to-workgroup mappings, with
16 x 16 tiles backward, on sequences of one and two steps, and one graph runs tilings, grids and batch sizes one after another on
the same never-reset tile flags.  tests/convlstm_cases.py holds the cases and predicts the form of every launch for the device's CU
count; tests/test_convlstm_cases.py proves that the cases reach the forms they are listed for.

Per run of a case (= one setting of the test hooks DL4DS_CONVLSTM_SEQ_TR / DL4DS_SEQ_GRID):
  * output, loss, dX, dK, dU, db against the fp64 oracle, with the graph, criterion and tolerances of test_conv_lstm2d;
  * the profiler tags (DL4DS_SEQ_TAG_FORMS=1: rows per wave, grid, tiles) are exactly the predicted ones;
  * under a grid cap everything equals the uncapped run of the same tiling BIT FOR BIT.  The cap changes which workgroup computes a
    tile and whether the cell state comes from a register or from the float it was stored as; no sum changes its order.  A halo one
    step old often stays inside an fp64 tolerance on smooth data: this is the assertion that sees it.
"""
import numpy as np
import pytest

from tests import convlstm_cases as K

pytestmark = pytest.mark.gpu

HOOKS = ('DL4DS_CONVLSTM_SEQ_TR', 'DL4DS_SEQ_GRID')
GRADS = ('x', 'lstm/kernel', 'lstm/recurrent_kernel', 'lstm/bias')


@pytest.fixture(scope='module')
def cus():
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count


@pytest.fixture(autouse=True)
def tagged_and_drained(monkeypatch):
    """Form tags on, no hook left over from the environment; afterwards the device-side error word must be clear: a spin of the
    persistent kernel that gave up fails the test through dl4ds_sync."""
    import dl4ds_amd._lib as L
    monkeypatch.setenv('DL4DS_SEQ_TAG_FORMS', '1')
    for name in HOOKS + ('DL4DS_NO_CONVLSTM_SEQ', 'DL4DS_AUX_STREAM'):
        monkeypatch.delenv(name, raising=False)
    yield
    L.check(L.lib().dl4ds_sync())


def set_hooks(monkeypatch, run):
    for name, v in zip(HOOKS, run):
        if v is None:
            monkeypatch.delenv(name, raising=False)
        else:
            monkeypatch.setenv(name, str(v))


def one_op(case, w):
    from tests.convlstm_op import OneOp
    op = OneOp(case.T, case.H, case.W, case.C, case.F, case.KS, case.relu)
    op.model.set_weights(w)
    return op


def run_tagged(op, P):
    from tests.parity import kernel_tags
    (got, loss, grads), tags = kernel_tags(lambda: op.run(P['x'], P['y']))
    return (got, loss, grads), tags


def seq_tags(tags):
    return {t for t in tags if t.startswith('convlstm_seq_')}


def assert_bit_equal(res, base, what):
    np.testing.assert_array_equal(res[0], base[0], err_msg=f'{what}: output')
    assert res[1] == base[1], (what, 'loss', res[1], base[1])
    for k in GRADS:
        np.testing.assert_array_equal(res[2][k], base[2][k], err_msg=f'{what}: gradient {k}')


@pytest.mark.parametrize('item', K.SEQ_ITEMS, ids=[i.case.id for i in K.SEQ_ITEMS])
def test_persistent_kernel_forms(item, cus, monkeypatch):
    from tests.convlstm_op import assert_against_fp64
    case = item.case
    P = K.problem(case)
    op = one_op(case, P['w'])
    base = {}
    for run in item.runs:
        set_hooks(monkeypatch, run)
        what = (case.id,) + tuple(run)
        res, tags = run_tagged(op, P)
        print(what, sorted(seq_tags(tags)))
        assert seq_tags(tags) == K.expected_tags(case, cus, run), what
        assert not any(t.startswith('convlstm_gates') for t in tags), what
        assert_against_fp64(*res, P['ref'], what=what)
        if case.T == 1:          # no step has a recurrent input: dU is the graph's zero fill, never written
            assert not np.any(res[2]['lstm/recurrent_kernel']), what
        if run.cap is None:
            base[run.tr] = res
        else:
            assert_bit_equal(res, base[run.tr], what)


def test_cases_reach_every_form_on_this_device(cus):
    """Every run above asserts that its tags are the predicted ones, so what the suite has launched on THIS device follows from
    the prediction: the forward kernel over several rounds and the backward kernel on 16 x 16 tiles for all five pairs, 8 x 16 tiles
    over several rounds, and -- without any hook -- the large batch over several rounds in both directions."""
    fwd_rounds, bwd_tr4, bwd_tr2_rounds = set(), set(), set()
    for item in K.SEQ_ITEMS:
        for run in item.runs:
            f, b = K.form(item.case, False, cus, run), K.form(item.case, True, cus, run)
            pair = (item.case.KS, item.case.F)
            if f.rounds >= 2 and not f.single:
                fwd_rounds.add(pair)
            if b.tr == 4:
                bwd_tr4.add(pair)
            if b.tr == 2 and b.rounds >= 2:
                bwd_tr2_rounds.add(pair)
    assert sorted(fwd_rounds) == sorted(bwd_tr4) == sorted(bwd_tr2_rounds) == K.PAIRS
    f, b = K.form(K.LARGE, False, cus), K.form(K.LARGE, True, cus)
    if f.ntiles >= 2 * max(cus, 8):                # (true on MI355X: 513 tiles of 16 x 16, 256 CUs)
        assert not f.single and f.rounds >= 2 and b.tr == 4 and b.rounds >= 2


@pytest.mark.parametrize('case', K.FALLBACK_SWITCHED + [K.FALLBACK_UNSUPPORTED], ids=lambda c: c.id)
def test_step_by_step_path(case, monkeypatch):
    """The documented fall-back (one convolution and one gate kernel per step): under DL4DS_NO_CONVLSTM_SEQ=1 for pairs the persistent
    kernel supports -- read when the graph is finalized -- and by itself for a filter count it is not built for."""
    from tests.convlstm_op import assert_against_fp64
    if K.supported(case.KS, case.F, case.H, case.W, 1):
        monkeypatch.setenv('DL4DS_NO_CONVLSTM_SEQ', '1')
    P = K.problem(case)
    op = one_op(case, P['w'])
    res, tags = run_tagged(op, P)
    assert not seq_tags(tags), tags
    assert tags.get('convlstm_gates_fwd') == 2 * case.T and tags.get('convlstm_gates_bwd') == case.T, tags      # (two forward passes)
    assert_against_fp64(*res, P['ref'], what=(case.id, 'step by step'))


def test_tile_flags_across_tilings_grids_and_batch_sizes(cus, monkeypatch):
    """The flags are never reset: whatever an earlier launch of any tiling, grid or batch size left in a flag word must read as
    'nothing done'.  One graph planned for batch 3 runs the library's own forms, one workgroup on 16 x 16 tiles, five on 8 x 16 tiles
    (other tile indices on the same words), batch 1, and the first step again: every step against fp64, the last equal to the first
    bit for bit."""
    from tests.convlstm_op import assert_against_fp64
    case = K.FLAGS_CASE
    w = K.problem(case)['w']
    op = one_op(case, w)
    results = []
    for i, (batch, run) in enumerate(K.FLAGS_STEPS):
        c = K.with_batch(case, batch)
        P = K.problem(c)
        assert all(np.array_equal(P['w'][k], w[k]) for k in w)
        set_hooks(monkeypatch, run)
        what = (case.id, 'flags', i, batch) + tuple(run)
        res, tags = run_tagged(op, P)
        print(what, sorted(seq_tags(tags)))
        assert seq_tags(tags) == K.expected_tags(c, cus, run), what
        assert_against_fp64(*res, P['ref'], what=what)
        results.append(res)
    assert K.FLAGS_STEPS[0] == K.FLAGS_STEPS[-1]
    assert_bit_equal(results[-1], results[0], 'last step against the first')
