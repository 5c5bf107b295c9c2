"""CPU side of the neighbourhood verification of an ensemble: the restatement tests/ensemble_fss_ref.py
against its brute-force form, against tests/fss_ref.py at K = 1 and against tests/exceedance_ref.py at n = 1, hand-worked answers,
the host arithmetic of ``neighbourhood_from_sums``, every refusal of the Python layer with the library out of reach, the exports
and the C declaration.  Needs no GPU."""
import ctypes

import numpy as np
import pytest

from tests import ensemble_fss_ref as R
from tests import exceedance_ref, fss_ref
from tests.ensemble_fss_cases import CASES


def test_restatement_against_brute_force():
    c = CASES['tiny']()
    y, x = c['y'].copy(), c['members'].copy()
    y[1, 2, 3, 0], x[2, 3, 4, 5, 0] = np.nan, np.inf
    K = x.shape[0]
    valid, o, cc = R.cell_counts(x, y, c['thresholds'])
    assert not valid[1, 2, 3, 0] and not valid[3, 4, 5, 0] and valid.sum() == valid.size - 2
    assert (o[:, ~valid] == 0).all() and (cc[:, ~valid] == 0).all()
    sums, cont, nvalid = R.integer_sums(x, y, c['thresholds'], c['windows'])
    for i in (0, 1, 3):
        for t in range(len(c['thresholds'])):
            for s, n in enumerate(c['windows'][:8]):                      # (100000 clipped to the field is window 64)
                want = R.brute_force(o[t, i, :, :, 0], cc[t, i, :, :, 0], valid[i, :, :, 0], K, n)
                assert tuple(int(v) for v in sums[i, 0, t, s]) == want, (i, t, n)
    np.testing.assert_array_equal(sums[:, :, :, 7], sums[:, :, :, 8])     # both hold the whole field from every cell
    np.testing.assert_array_equal(cont[..., 0], o.sum(axis=(2, 3)).transpose(1, 2, 0))
    np.testing.assert_array_equal(nvalid, valid.sum(axis=(1, 2)))


def test_one_member_is_the_fractions_skill_score():
    """K = 1: D, F, O are dl4ds_fss's, E is hits + misses, Cs is hits + false alarms"""
    c = CASES['nonfinite_mask2d']()
    x = c['members'][:1]
    sums, cont, nvalid = R.integer_sums(x, c['y'], c['thresholds'], c['windows'], c['mask'])
    want = fss_ref.neighbourhood_scores(c['y'], x[0], c['thresholds'], c['windows'], mask=c['mask'])
    np.testing.assert_array_equal(sums[..., :3], want['sums'])
    np.testing.assert_array_equal(cont[..., 0], want['hits'] + want['misses'])
    np.testing.assert_array_equal(cont[..., 1], want['hits'] + want['false_alarms'])
    np.testing.assert_array_equal(nvalid, want['n_valid'])
    got = R.from_sums(sums, cont, nvalid, 1, c['thresholds'], c['windows'])
    np.testing.assert_array_equal(got['pfss'], want['fss'])
    np.testing.assert_array_equal(got['pfss_pooled'], want['fss_pooled'])
    np.testing.assert_array_equal(got['useful_window'], want['useful_window'])


def test_window_one_is_the_brier_score():
    """n = 1: D = sum (c - K o)^2 and nbs is the Brier score of tests/exceedance_ref.py"""
    c = CASES['nonfinite_mask_channels']()
    y = np.where(np.broadcast_to(c['mask'] != 0, c['y'].shape), c['y'], np.nan).astype(np.float32)
    x, K = c['members'], c['members'].shape[0]
    sums, cont, nvalid = R.integer_sums(x, y, c['thresholds'], (1,))
    er = exceedance_ref.counts_ref(x, y, np.asarray(c['thresholds'], np.float32))
    np.testing.assert_array_equal(sums[..., 0, 0].sum(axis=1), er['sample'][..., 3])
    np.testing.assert_array_equal(cont[..., 0].sum(axis=1), er['sample'][..., 1])
    np.testing.assert_array_equal(cont[..., 1].sum(axis=1), er['sample'][..., 2])
    got = R.from_sums(sums, cont, nvalid, K, c['thresholds'], (1,))
    want = exceedance_ref.from_counts_ref(er['table'], er['cell'], er['sample'], K, c['thresholds'])
    np.testing.assert_allclose(got['nbs_pooled'][:, 0], want['brier'], rtol=1e-15, atol=0)
    np.testing.assert_allclose(got['nbss_pooled'][:, 0], want['bss'], rtol=0, atol=1e-12)
    np.testing.assert_allclose(got['base_rate'], want['base_rate'], rtol=1e-15, atol=0)


def test_hand_worked_answers():
    """* a perfect ensemble (every member is the observation): cf = K co, D = 0, pfss = 1; at n = 1 c = K o and nbs = 0;
    * no event on either side: F + K^2 O = 0, pfss NaN; nbs = 0 / n_valid = 0, nbss NaN (f_o = 0);
    * every member forecasts the event everywhere, never observed: co = 0, D = F, pfss = 0;
    * 1 x 7 field, K = 2, the event observed in cell 1, forecast by both members in cell 3 (displaced by two cells):
        n = 1: cf = (0,0,0,2,0,0,0), co = (0,1,0,0,0,0,0): D = 4 + 4 = 8, F = 4, O = 1, pfss = 1 - 8 / (4 + 4) = 0;
               Fv = 4, X = 0, E = 1: nbs = (4 - 0 + 4) / (4 * 7) = 2 / 7
        n = 3: cf = (0,0,2,2,2,0,0), co = (1,1,1,0,0,0,0): cf - 2 co = (-2,-2,0,2,2,0,0): D = 16, F = 12, O = 3,
               pfss = 1 - 16 / 24 = 1 / 3; X = cf[1] = 0; nbs = (12 - 0 + 4 * 81 * 1) / (4 * 81 * 7) = 336 / 2268 = 4 / 27
        n = 5: cf = (0,2,2,2,2,2,0), co = (1,1,1,1,0,0,0): cf - 2 co = (-2,0,0,0,2,2,0): D = 12, F = 20, O = 4,
               pfss = 1 - 12 / 36 = 2 / 3; X = cf[1] = 2; nbs = (20 - 2*2*25*2 + 4*625) / (4 * 625 * 7) = 2320 / 17500 = 116 / 875"""
    y, _ = CASES['tiny']()['y'], None
    x = np.repeat(y[None], 3, axis=0)
    r = R.scores(x, y, (0.0,), (1, 3))
    assert (r['sums'][..., 0] == 0).all() and (r['pfss'] == 1.0).all() and (r['nbs'][..., 0] == 0.0).all()
    r = R.scores(x, y, (100.0,), (1, 3))
    assert np.isnan(r['pfss']).all() and np.isnan(r['pfss_pooled']).all() and (r['nbs'] == 0.0).all()
    assert np.isnan(r['nbss_pooled']).all() and (r['useful_window'] == -1).all()
    r = R.scores(np.ones_like(x), np.zeros_like(y), (0.5,), (1, 3, 64))
    np.testing.assert_array_equal(r['sums'][..., 0], r['sums'][..., 1])
    assert (r['sums'][..., 2] == 0).all() and (r['pfss'] == 0.0).all() and (r['sums'][..., 4] == 0).all()
    y = np.zeros((1, 1, 7, 1), np.float32)
    x = np.zeros((2, 1, 1, 7, 1), np.float32)
    y[0, 0, 1, 0], x[:, 0, 0, 3, 0] = 1.0, 1.0
    r = R.scores(x, y, (0.5,), (1, 3, 5))
    assert r['sums'][0, 0, 0].tolist() == [[8, 4, 1, 4, 0], [16, 12, 3, 12, 0], [12, 20, 4, 20, 2]]
    assert r['events'].tolist() == [[[1]]] and r['member_events'].tolist() == [[[2]]] and r['n_valid'].tolist() == [[7]]
    np.testing.assert_allclose(r['pfss'][0, 0, 0], [0.0, 1 / 3, 2 / 3], rtol=0, atol=1e-15)
    np.testing.assert_allclose(r['nbs'][0, 0, 0], [2 / 7, 4 / 27, 116 / 875], rtol=1e-15, atol=0)
    np.testing.assert_allclose(r['nbss_pooled'][0], [1 - (2 / 7) / (6 / 49), 1 - (4 / 27) / (6 / 49), 1 - (116 / 875) / (6 / 49)],
                               rtol=1e-14, atol=0)
    assert r['base_rate'].tolist() == [1 / 7] and r['forecast_rate'].tolist() == [2 / 14]
    assert r['useful_window'].tolist() == [5]                             # 0.5 + 1 / 14 = 0.571 is first reached at n = 5


def test_the_restatement_yields_nan_only_where_the_cases_are_built_to():
    for name in ('extremes', 'tiny', 'saturated'):
        c = CASES[name]()
        r = R.scores(c['members'], c['y'], c['thresholds'], c['windows'][:2], c['mask'])
        nan = np.zeros(r['pfss'].shape, bool)
        nan[:, :, list(c['nan_thresholds'])] = True
        np.testing.assert_array_equal(np.isnan(r['pfss']), nan, err_msg=name)
        assert not np.isnan(r['nbs']).any(), name


def test_neighbourhood_from_sums_on_hand_made_sums():
    from dl4ds_amd.ensemble_score import neighbourhood_from_sums
    c = CASES['three_channels']()
    K = c['members'].shape[0]
    sums, cont, nvalid = R.integer_sums(c['members'][:, :, :20, :21], c['y'][:, :20, :21], c['thresholds'], c['windows'])
    R.assert_same(neighbourhood_from_sums(sums, cont, nvalid, K, c['thresholds'], c['windows']),
                  R.from_sums(sums, cont, nvalid, K, c['thresholds'], c['windows']), 'small')
    # the hand-worked field of test_hand_worked_answers, by hand
    got = neighbourhood_from_sums([[[[[8, 4, 1, 4, 0], [16, 12, 3, 12, 0], [12, 20, 4, 20, 2]]]]], [[[[1, 2]]]], [[7]], 2, (0.5,),
                                  (1, 3, 5))
    np.testing.assert_allclose(got['pfss'][0, 0, 0], [0.0, 1 / 3, 2 / 3], rtol=0, atol=1e-15)
    assert got['nbs'][0, 0, 0].tolist() == [2 / 7, 4 / 27, 116 / 875] and got['useful_window'].tolist() == [5]
    # two fields whose sums are each close to 2^62: the pooled sums pass int64; a window of 10^6 has n^4 = 10^24
    big = (1 << 62) - 5
    s = np.array([[[[[big - 3, big, 0, big, 7]]]], [[[[big - 1, big - 2, 0, big - 2, 9]]]]], np.int64)
    ct, nv = np.array([[[[3, 5]]], [[[4, 6]]]], np.int64), np.array([[10], [12]], np.int64)
    got = neighbourhood_from_sums(s, ct, nv, 3, (1.0,), (1000000,))
    from fractions import Fraction
    assert got['pfss_pooled'][0, 0] == 1.0 - float(Fraction(2 * big - 4, 2 * big - 2))
    kn, n2 = 9 * 10 ** 24, 10 ** 12
    num = (2 * big - 2) - 2 * 3 * n2 * 16 + kn * 7
    assert got['nbs_pooled'][0, 0] == float(Fraction(num, kn * 22))
    assert got['nbss_pooled'][0, 0] == float(1 - Fraction(num, kn * 22) / (Fraction(7, 22) * Fraction(15, 22)))
    R.assert_same(got, R.from_sums(s, ct, nv, 3, (1.0,), (1000000,)), 'big')
    with pytest.raises(ValueError, match='expected sums'):
        neighbourhood_from_sums(s[..., :3], ct, nv, 3, (1.0,), (1000000,))


@pytest.fixture
def no_library(monkeypatch):
    """the library out of reach: every refusal below must come before it is asked for"""
    import dl4ds_amd._lib as L

    def unreachable(*a, **k):
        raise AssertionError('the library was reached')
    monkeypatch.setattr(L, 'lib', unreachable)
    monkeypatch.setattr(L, 'load', unreachable)


def test_refusals_come_before_any_library_call(no_library):
    from dl4ds_amd.ensemble_score import check_neighbourhood_ensemble_args, largest_neighbourhood_window
    from dl4ds_amd.metrics import FSS_DEFAULT_WINDOWS, neighbourhood_ensemble_scores
    from dl4ds_amd.ensemble_score import NEIGHBOURHOOD_DEFAULT_WINDOWS
    assert NEIGHBOURHOOD_DEFAULT_WINDOWS == FSS_DEFAULT_WINDOWS
    y = np.zeros((2, 6, 7, 1), np.float32)
    x = np.zeros((3,) + y.shape, np.float32)
    good = dict(thresholds=(0.5,), windows=(1, 3))
    for bad, match in ((dict(thresholds=()), 'thresholds'), (dict(thresholds=(np.nan,)), 'finite'), (dict(thresholds=(np.inf,)), 'finite'),
                       (dict(thresholds=(1e39,)), 'finite'), (dict(thresholds=(1.0, 1.0)), 'increasing'),
                       (dict(thresholds=tuple(range(17))), 'at most 16'), (dict(windows=()), 'windows'), (dict(windows=(0,)), 'positive'),
                       (dict(windows=(-3, 1)), 'positive'), (dict(windows=(1.5,)), 'integers'), (dict(windows=(3, 3)), 'increasing'),
                       (dict(batch_size=0), 'batch_size'), (dict(batch_size=2.0), 'batch_size')):
        with pytest.raises(ValueError, match=match):
            neighbourhood_ensemble_scores(y, x, **dict(good, **bad))
    for yy, xx in ((y, x[:, :1]), (y[..., 0], x[..., 0]), (y, x[0]), (y, np.zeros((257,) + y.shape, np.float32)),
                   (y[:0], x[:, :0])):
        with pytest.raises(ValueError):
            neighbourhood_ensemble_scores(yy, xx, **good)
    with pytest.raises(ValueError, match='mask'):
        neighbourhood_ensemble_scores(y, x, mask=np.ones((5, 5)), **good)
    # the overflow rule carries the members: 400 x 400 cells, K = 32: the whole field is legal, (32 * 160000)^2 * 160000 = 4.19e18
    assert largest_neighbourhood_window(32, 400, 400) is None and 160000 * (32 * 160000) ** 2 < 1 << 62
    check_neighbourhood_ensemble_args((400, 400, 1), 32, (0.5,), (1, 400, 100000))
    top = largest_neighbourhood_window(34, 400, 400)                      # K = 34: 4.73e18 >= 2^62
    assert 160000 * (34 * top * top) ** 2 < 1 << 62 <= 160000 * (34 * (top + 1) ** 2) ** 2 and top == 397
    check_neighbourhood_ensemble_args((400, 400, 1), 34, (0.5,), (1, top))
    with pytest.raises(ValueError, match=rf'2\^62.*largest legal window for K = 34, H = 400, W = 400 is {top}'):
        check_neighbourhood_ensemble_args((400, 400, 1), 34, (0.5,), (1, top + 1))
    with pytest.raises(ValueError, match=r'2\^62.*largest legal window'):
        neighbourhood_ensemble_scores(np.zeros((1, 400, 400, 1), np.float32), np.zeros((34, 1, 400, 400, 1), np.float32), (0.5,), (500,))
    with pytest.raises(ValueError, match=r'2\^31'):
        check_neighbourhood_ensemble_args((1 << 16, 1 << 15, 1), 2, (0.5,), (1,))
    for shape in ((4, 6, 7, 1), (6, 7), (6, 0, 1)):                        # a recurrent model's output among them
        with pytest.raises(ValueError, match=r'one sample must be shaped \(H, W, C\)'):
            check_neighbourhood_ensemble_args(shape, 2, (0.5,), (1,))
    for K in (0, 257):
        with pytest.raises(ValueError, match='n_members'):
            check_neighbourhood_ensemble_args((6, 7, 1), K, (0.5,), (1,))
    thr, win = check_neighbourhood_ensemble_args(None, 256, (0.1, 0.2), (1, 1 << 30))          # nothing known about the shape yet
    assert thr.dtype == np.float32 and win.dtype == np.int32 and win.tolist() == [1, 1 << 30]


def test_model_and_inference_refuse_without_the_library(no_library):
    import dl4ds_amd
    from dl4ds_amd.graph import Model
    with pytest.raises(ValueError, match='increasing'):
        Model.score_neighbourhood(None, None, None, 4, (1.0, 0.5))
    with pytest.raises(ValueError, match='n_members'):
        Model.score_neighbourhood(None, None, None, 0, (0.5,))
    with pytest.raises(ValueError, match='positive'):
        Model.score_neighbourhood(None, None, None, 4, (0.5,), windows=(0,))
    a = np.zeros((3, 8, 8, 1), np.float32)
    with pytest.raises(ValueError, match='time_window'):
        dl4ds_amd.verify_neighbourhood(None, a, 2, 4, (0.5,), time_window=3)
    with pytest.raises(ValueError, match='at most 16'):
        dl4ds_amd.verify_neighbourhood(None, a, 2, 4, tuple(range(17)))
    with pytest.raises(ValueError, match='y_true'):
        dl4ds_amd.verify_neighbourhood(None, a, 2, 4, (0.5,), y_true=a[:, :4])
    v = dl4ds_amd.NeighbourhoodVerifier(None, a, 2, 4, (0.5,), windows=(3, 1), array_in_hr=True)
    with pytest.raises(ValueError, match='increasing'):
        v.run()


def test_exports():
    import dl4ds_amd
    from dl4ds_amd import ensemble_score, inference, metrics
    assert dl4ds_amd.neighbourhood_ensemble_scores is metrics.neighbourhood_ensemble_scores
    assert dl4ds_amd.verify_neighbourhood is inference.verify_neighbourhood
    assert dl4ds_amd.NeighbourhoodVerifier is inference.NeighbourhoodVerifier
    assert issubclass(ensemble_score.NeighbourhoodScorer, ensemble_score._Accumulators)
    from dl4ds_amd.graph import Model
    import inspect
    sig = inspect.signature(Model.score_neighbourhood)
    assert list(sig.parameters) == ['self', 'inputs', 'y_true', 'n_members', 'thresholds', 'windows', 'batch_size', 'seed']
    assert sig.parameters['batch_size'].default == 32 and sig.parameters['windows'].default == metrics.FSS_DEFAULT_WINDOWS
    sig = inspect.signature(metrics.neighbourhood_ensemble_scores)
    assert list(sig.parameters) == ['y_true', 'members', 'thresholds', 'windows', 'mask', 'batch_size']


def test_c_declaration():
    from dl4ds_amd._lib import parse_header
    ret, args = parse_header()['dl4ds_ensemble_fss']
    p, z, i = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int
    assert ret is ctypes.c_int
    assert args == [p, z, z, z, p, z, i, i, i, p, i, p, i, p, p, p]
