"""CPU-only checks behind tests/test_gpu_convlstm.py: the restatement of the persistent ConvLSTM kernel's host-side arithmetic
(tests/convlstm_cases.py) follows the source text, its tile loop visits every tile exactly once under both mappings, and the case
tables reach -- at 256 CUs -- every form they are listed for."""
import pytest

from tests import convlstm_cases as K

CUS = K.REFERENCE_CUS


def _launches(items=None):
    """-> [(case, run, backward, form)] of every launch of the persistent kernel the GPU tests make (at 256 CUs)."""
    out = []
    for item in (K.SEQ_ITEMS if items is None else items):
        for run in item.runs:
            for backward in (False, True):
                out.append((item.case, run, backward, K.form(item.case, backward, CUS, run)))
    return out


def _brief(f):
    return (f.tr, f.ntiles, f.grid, f.rounds, f.mapping)


def test_restatement_follows_the_source():
    src = K.source_text()
    for piece in ('if(getenv("DL4DS_NO_CONVLSTM_SEQ"))returnfalse;',
                  'if(getenv("DL4DS_AUX_STREAM"))returnfalse;',
                  'if(!(KS==3||KS==5)||!(F==4||F==8||F==16))returnfalse;',
                  'if(F==16&&KS==5)returnfalse;',
                  'constlongtiles=(long)cdiv(H,16)*cdiv(W,16)*B;returntiles>=1&&tiles<(1l<<24);',
                  'if(constchar*e=test_env("DL4DS_CONVLSTM_SEQ_TR"))returnatoi(e)==2?2:4;',
                  'constlongt16=(long)cdiv(H,16)*cdiv(W,16)*B;return(backward&&t16<2l*std::max(cu_count(),8)&&H>8)?2:4;',
                  'p.tiles_x=cdiv(W,16);p.tiles_y=cdiv(H,4*p.tr);p.ntiles=p.tiles_x*p.tiles_y*B;',
                  'constintcus=std::max(cu_count()-(dist_active()?reserve:0),8);intgrid=std::min(p.ntiles,cus);',
                  'if(constchar*e=test_env("DL4DS_SEQ_GRID")){constintn=atoi(e);if(n>=1)grid=std::min(grid,n);}returngrid;',
                  'constintper=grid>>3;constintlin=(grid&7)?b:(b&7)*per+(b>>3);returni*grid+lin;',
                  'constboolsingle=p.ntiles<=grid;',
                  'staticconstexprboolPAIR=BWD&&F==8&&TR==2;',
                  'return"tr"+std::to_string(p.tr)+"g"+std::to_string(grid)+"n"+std::to_string(p.ntiles);',
                  'size_tconvlstm_seq_flag_bytes(intH,intW,intB){return(size_t)cdiv(H,8)*cdiv(W,16)*B*sizeof(unsignedlonglong);}'):
        assert piece in src, piece
    # the tile loop, the same in both kernels
    assert src.count('constinttl=my_tile(it,grid);if(tl>=p.ntiles){if(it*grid>=p.ntiles)break;elsecontinue;}') == 2
    # every supported pair is instantiated in both directions, and nothing else
    cases = 'DL4DS_SEQ_CASE(3,4)DL4DS_SEQ_CASE(3,8)DL4DS_SEQ_CASE(3,16)DL4DS_SEQ_CASE(5,4)DL4DS_SEQ_CASE(5,8)#undef'
    assert src.count(cases) == 2
    for ks in (1, 3, 5, 7):
        for f in (2, 4, 8, 12, 16, 32):
            assert K.supported(ks, f, 37, 23, 2) == ((ks, f) in K.PAIRS)
    # the three hooks go through test_env, i.e. they do nothing unless the suite's switch is set
    for name in ('DL4DS_SEQ_GRID', 'DL4DS_CONVLSTM_SEQ_TR', 'DL4DS_SEQ_TAG_FORMS'):
        assert src.count(f'test_env("{name}")') == 1 and f'getenv("{name}")' not in src.replace(f'test_env("{name}")', '')


def test_tile_loop_visits_every_tile_once():
    """For every (tiles, grid) of the suite, and exhaustively for small ones: each tile belongs to exactly one block, a block takes
    its tiles in increasing order, never more than ``rounds`` of them, and only a ragged last round is skipped."""
    pairs = {(f.ntiles, f.grid) for _, _, _, f in _launches()} | {(n, g) for g in range(1, 41) for n in range(g, 4 * g + 3)}
    for ntiles, grid in sorted(pairs):
        tiles, skipped = K.schedule(ntiles, grid)
        flat = sorted(t for b in tiles for t in b)
        assert flat == list(range(ntiles)), (ntiles, grid)
        rounds = K.cdiv(ntiles, grid)
        for b in range(grid):
            assert tiles[b] == sorted(tiles[b]) and len(tiles[b]) + skipped[b] == rounds and skipped[b] <= 1
            assert tiles[b][0] < grid                                 # round 0 is never skipped: grid <= ntiles
        assert (sum(skipped) > 0) == (ntiles % grid != 0)


def test_the_permutation_leaves_holes_in_a_ragged_round():
    """20 tiles on 16 blocks (shape A, 8 x 16 tiles, cap 16): round 1 holds tiles 16 .. 19, which go to blocks 0, 8, 1, 9 -- blocks
    2 .. 7 pass over it although later blocks do not."""
    tiles, skipped = K.schedule(20, 16)
    assert [b for b in range(16) if not skipped[b]] == [0, 1, 8, 9]
    assert [tiles[b][1] for b in (0, 8, 1, 9)] == [16, 17, 18, 19]
    tiles, skipped = K.schedule(513, 256)                            # the large batch: one tile in the third round
    assert sum(len(t) == 3 for t in tiles) == 1 and len(tiles[0]) == 3 and sum(skipped) == 255


def test_hand_checked_forms():
    named = {'A': K.A_CASES, 'B': K.B_CASES, 'LARGE': [K.LARGE]}
    for (name, run), (fwd, bwd) in K.HAND_CHECKED.items():
        for case in named[name]:
            assert _brief(K.form(case, False, CUS, run)) == fwd, (case, run)
            assert _brief(K.form(case, True, CUS, run)) == bwd, (case, run)
    assert K.SHAPE_A == (2, 3, 37, 23) and K.SHAPE_B == (3, 3, 33, 40)
    for case in K.A_CASES:                                           # halos cross tile borders both ways at both tilings
        for run in (K.NO_HOOK, K.Run(4, None)):
            f = K.form(case, True, CUS, run)
            assert f.tiles_y >= 2 and f.tiles_x >= 2 and case.H % (4 * f.tr) and case.W % 16


def test_multi_round_conditions_of_the_suite():
    L = _launches()
    for backward in (False, True):
        for mapping in ('linear', 'permuted'):
            assert any(b == backward and f.mapping == mapping and f.ntiles % f.grid and f.rounds >= 2 for _, _, b, f in L), \
                (backward, mapping)
        assert any(b == backward and f.ntiles % f.grid == 0 and f.rounds >= 2 for _, _, b, f in L)
        assert any(b == backward and r.cap == 1 and f.grid == 1 and f.rounds >= 12 for _, r, b, f in L)
    assert any(f.mapping == 'permuted' and f.grid >> 3 == 2 and f.ntiles % f.grid for _, _, b, f in L if b)
    # the forward kernel both ways: cell state in registers / reloaded from C
    assert {f.single for _, _, b, f in L if not b} == {True, False}


def test_every_pair_in_four_forms_on_shape_a():
    assert sorted((c.KS, c.F) for c in K.A_CASES) == K.PAIRS
    assert {c.C for c in K.A_CASES} == set(K.CINS) and {c.relu for c in K.A_CASES} == {True, False}
    for case in K.A_CASES:
        assert (case.B, case.T, case.H, case.W) == K.SHAPE_A and K.supported(case.KS, case.F, case.H, case.W, 1)
        forms = {(b, f.tr, f.rounds >= 2) for c, _, b, f in _launches([K.Item(case, K.A_RUNS)])}
        assert {(False, 4, True), (True, 2, True), (True, 4, False), (True, 4, True)} <= forms, case
        # F = 8 backward: with the PAIR layout at 8 x 16 tiles, without it at 16 x 16
        if case.F == 8:
            assert {f.pair for _, _, b, f in _launches([K.Item(case, K.A_RUNS)]) if b} == {True, False}
    # each capped run has an uncapped one of the same tiling to be compared with bit for bit
    for item in K.SEQ_ITEMS:
        for run in item.runs:
            assert K.Run(run.tr, None) in item.runs, (item.case, run)


def test_sixteen_row_tiles_backward_without_a_hook():
    shapes = {(c.B, c.T, c.H, c.W) for c in K.LOW_CASES}
    assert shapes == {(2, 3, 8, 20), (1, 2, 5, 7), (2, 3, 3, 40)}
    for case in K.LOW_CASES:
        f = K.form(case, True, CUS)
        assert case.H <= 8 and f.tr == 4 and f.tiles_y == 1 and K.supported(case.KS, case.F, case.H, case.W, 1)
    assert any(c.H < c.KS for c in K.LOW_CASES) and {c.W < 16 for c in K.LOW_CASES} == {True, False}
    assert K.NO_HOOK in K.LOW_RUNS


def test_large_batch_without_a_hook():
    c = K.LARGE
    assert (c.B, c.T, c.H, c.W, c.C, c.F, c.KS) == (57, 2, 33, 33, 1, 4, 3) and K.LARGE_RUNS == [K.NO_HOOK]
    fwd, bwd = K.form(c, False, CUS), K.form(c, True, CUS)
    assert fwd.ntiles == 513 >= 2 * CUS and not fwd.single and fwd.mapping == 'permuted' and fwd.ntiles % fwd.grid
    assert bwd.tr == 4 and bwd.rounds == 3 and not bwd.pair
    assert c.B * c.T * c.H * c.W == 124146 and c.B * c.T * c.H * c.W * 4 * c.F * 4 < 8 << 20       # Z: under 8 MB
    # no case of the suite is larger
    assert all(i.case.B * i.case.T * i.case.H * i.case.W <= 124146 for i in K.SEQ_ITEMS)


def test_short_sequences_and_fallback_tables():
    assert sorted((c.T, c.KS, c.F) for c in K.SHORT_CASES) == [(1, 3, 8), (1, 5, 4), (2, 3, 8), (2, 5, 4)]
    assert all((c.B, c.H, c.W) == (2, 19, 23) for c in K.SHORT_CASES)
    assert sorted((c.KS, c.F) for c in K.FALLBACK_SWITCHED) == [(3, 8), (3, 16), (5, 4)]
    for c in K.FALLBACK_SWITCHED:
        assert K.supported(c.KS, c.F, c.H, c.W, 1) and not K.supported(c.KS, c.F, c.H, c.W, 1, env=('DL4DS_NO_CONVLSTM_SEQ',))
    u = K.FALLBACK_UNSUPPORTED
    assert u.F == 12 and not K.supported(u.KS, u.F, u.H, u.W, 1) and (u.B, u.T, u.H, u.W) == K.SHAPE_A


def test_flag_sequence_mixes_tilings_grids_and_batches():
    c = K.FLAGS_CASE
    assert [(b, tuple(r)) for b, r in K.FLAGS_STEPS] == [(3, (None, None)), (3, (4, 1)), (3, (2, 5)), (1, (None, None)), (3, (None, None))]
    assert c.B == 3 == max(b for b, _ in K.FLAGS_STEPS)
    seen = set()
    for b, run in K.FLAGS_STEPS:
        for backward in (False, True):
            f = K.form(K.with_batch(c, b), backward, CUS, run)
            seen.add((backward, f.tr, f.grid))
            # every tiling of every step fits the flag area of its batch (graph_ops2.hip: the DL4DS_REQUIRE of ConvLSTMOp::forward)
            assert f.ntiles <= K.flag_words(c.H, c.W, b) <= K.flag_quota_words(c.H, c.W) * b
    assert {(bw, tr) for bw, tr, _ in seen} == {(False, 4), (False, 2), (True, 4), (True, 2)}
    assert len({g for _, _, g in seen}) >= 4
    for item in K.SEQ_ITEMS:
        for run in item.runs:
            for backward in (False, True):
                f = K.form(item.case, backward, CUS, run)
                assert f.ntiles <= K.flag_words(item.case.H, item.case.W, item.case.B)


@pytest.mark.parametrize('cus', [8, 64, 104, 256, 304])
def test_tags_for_other_cu_counts(cus):
    """The GPU tests predict the tags from the device's own CU count: the prediction is well formed for any."""
    for item in K.SEQ_ITEMS:
        for run in item.runs:
            fwd, bwd = K.form(item.case, False, cus, run), K.form(item.case, True, cus, run)
            assert 1 <= fwd.grid <= min(cus, fwd.ntiles) and 1 <= bwd.grid <= min(cus, bwd.ntiles)
            if run.cap:
                assert fwd.grid <= run.cap and bwd.grid <= run.cap
            tags = K.expected_tags(item.case, cus, run)
            assert len(tags) == 2 and all(t.startswith(f'convlstm_seq_') and f'<{item.case.KS},{item.case.F}>tr' in t for t in tags)
    assert K.tag(K.A_CASES[4], True, K.form(K.A_CASES[4], True, 256, K.Run(4, 5))) == 'convlstm_seq_bwd<5,8>tr4g5n12'
    assert K.tag(K.A_CASES[4], True, None, forms=False) == 'convlstm_seq_bwd<5,8>'
