"""Neighbourhood verification of an ensemble on the device (dl4ds_ensemble_fss, csrc/ensemble_fss.hip) through
dl4ds_amd.metrics.neighbourhood_ensemble_scores, the entry called directly and Model.score_neighbourhood, against the integer
restatement tests/ensemble_fss_ref.py (itself checked against brute force, tests/fss_ref.py, tests/exceedance_ref.py and hand-worked
answers in tests/test_ensemble_fss_api.py).  The device works in integers: every sum and count is compared with assert_array_equal;
the scores are quotients of equal integers on either side and are compared at 1e-12 absolute (the figure of tests/test_gpu_fss.py)."""
import numpy as np
import pytest

from tests import ensemble_fss_ref as R
from tests.ensemble_fss_cases import CASES, NARROW_MAX, THRESHOLD_GROUP, WS_BUDGET, ensemble
from tests.fss_cases import precip_pair

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize('name', sorted(CASES))
def test_against_the_integer_reference(name):
    from dl4ds_amd.metrics import neighbourhood_ensemble_scores
    c = CASES[name]()
    got = neighbourhood_ensemble_scores(c['y'], c['members'], c['thresholds'], c['windows'], mask=c['mask'])
    want = R.scores(c['members'], c['y'], c['thresholds'], c['windows'], c['mask'])
    N, H, W, C = c['y'].shape
    K, T, S = c['members'].shape[0], len(c['thresholds']), len(c['windows'])
    assert got['sums'].shape == (N, C, T, S, 5) and got['pfss'].shape == (N, C, T, S) and got['events'].shape == (N, C, T)
    assert got['pfss_pooled'].shape == got['nbs_pooled'].shape == got['nbss_pooled'].shape == (T, S)
    R.assert_same(got, want, name)
    nan = np.zeros((N, C, T, S), bool)
    nan[:, :, list(c['nan_thresholds'])] = True
    np.testing.assert_array_equal(np.isnan(got['pfss']), nan)             # NaN where F + K^2 O = 0 by construction, nowhere else
    m = np.minimum(np.array(c['windows']), H) * np.minimum(np.array(c['windows']), W)
    if name == 'extremes':
        assert (got['events'][:, :, 0] == got['n_valid']).all() and (got['member_events'][:, :, 0] == K * got['n_valid']).all()
        assert (got['sums'][:, :, 3] == 0).all() and (got['member_events'][:, :, 3] == 0).all()
    if name == 'square_edge':
        assert (K * m[:2] <= NARROW_MAX).all() and (K * m[2:] > NARROW_MAX).all()
    if name == 'saturated':                                               # |cf - K co| reaches K m on either side of the edge
        assert K * m[1] <= NARROW_MAX < K * m[2]
        for s in (1, 2):
            assert got['sums'][0, 0, 0, s, 0] >= (K * m[s]) ** 2 and got['sums'][1, 0, 0, s, 0] >= (K * m[s]) ** 2
    if name in ('prefix16', 'prefix32'):
        assert (K * W <= NARROW_MAX) == (name == 'prefix16') and abs(K * W - NARROW_MAX) <= 1
    if name == 'thresholds9':
        assert T == THRESHOLD_GROUP + 1


def test_one_member_equals_dl4ds_fss_on_the_device():
    from dl4ds_amd.metrics import neighbourhood_ensemble_scores, neighbourhood_scores
    c = CASES['nonfinite_mask2d']()
    p = c['members'][0]
    got = neighbourhood_ensemble_scores(c['y'], p[None], c['thresholds'], c['windows'], mask=c['mask'])
    want = neighbourhood_scores(c['y'], p, c['thresholds'], c['windows'], mask=c['mask'])
    np.testing.assert_array_equal(got['sums'][..., :3], want['sums'])
    np.testing.assert_array_equal(got['events'], want['hits'] + want['misses'])
    np.testing.assert_array_equal(got['member_events'], want['hits'] + want['false_alarms'])
    np.testing.assert_array_equal(got['n_valid'], want['n_valid'])
    assert got['pfss'].tobytes() == want['fss'].tobytes() and got['pfss_pooled'].tobytes() == want['fss_pooled'].tobytes()


def test_result_does_not_depend_on_batch_size_and_is_reproducible():
    from dl4ds_amd.metrics import neighbourhood_ensemble_scores
    c = CASES['nonfinite_mask2d']()
    y = np.concatenate([c['y'], c['y'][:2, ::-1]])                        # N = 5
    x = np.concatenate([c['members'], c['members'][:, :2, ::-1]], axis=1)
    args = (y, x, c['thresholds'], c['windows'])
    ref = neighbourhood_ensemble_scores(*args, mask=c['mask'])
    R.assert_same(ref, R.scores(x, y, c['thresholds'], c['windows'], c['mask']))
    for bs in (1, 2, 5, None, None):                                      # one, a non-divisor of N, N, the default, the same call twice
        got = neighbourhood_ensemble_scores(*args, mask=c['mask'], batch_size=bs)
        for k in ref:
            assert np.asarray(got[k]).tobytes() == np.asarray(ref[k]).tobytes(), (bs, k)


def direct(rows, obs, shape, thresholds, windows, stride=None, repeat=1, fill=0, **over):
    """dl4ds_ensemble_fss called directly on a stack whose rows are ``rows`` repeated ``repeat`` times -> (status, sums, cont,
    valid); ``over`` replaces single arguments of the call (K, T, S, n, B, H, stride_arg, or names in ``null``)"""
    import dl4ds_amd._lib as L
    from dl4ds_amd.device import DeviceArray
    B, H, W, C = shape
    n = B * H * W * C
    stride = n if stride is None else stride
    K = len(rows) * repeat
    stack = DeviceArray((K, max(stride, 1)), np.float32)
    for k in range(K):
        stack.upload(np.ascontiguousarray(rows[k % len(rows)], np.float32).reshape(-1), k * stride)
    dobs = DeviceArray.from_numpy(np.ascontiguousarray(obs, np.float32).reshape(-1))
    thr, win = np.asarray(thresholds, np.float32), np.asarray(windows, np.int32)
    T, S = len(thr), len(win)
    outs = [DeviceArray.from_numpy(np.full(s, fill, np.int64)) for s in ((B, C, T, S, 5), (B, C, T, 2), (B, C))]
    null = over.pop('null', ())
    a = dict(members=stack.ptr, K=K, n=n, stride=stride, obs=dobs.ptr, B=B, H=H, W=W, C=C, thr=thr.ctypes.data, T=T,
             win=win.ctypes.data, S=S, sums=outs[0].ptr, cont=outs[1].ptr, valid=outs[2].ptr)
    a['stride'] = over.pop('stride_arg', stride)               # (the stack itself keeps its own stride)
    a.update(over)
    a.update({k: None for k in null})
    st = L.lib().dl4ds_ensemble_fss(a['members'], a['K'], a['n'], a['stride'], a['obs'], a['B'], a['H'], a['W'], a['C'], a['thr'],
                                    a['T'], a['win'], a['S'], a['sums'], a['cont'], a['valid'])
    return (st,) + tuple(o.numpy() for o in outs)


def test_direct_call_member_stride_and_overwritten_outputs():
    c = CASES['tiny']()
    want = R.integer_sums(c['members'], c['y'], c['thresholds'], c['windows'])
    n = c['y'].size
    for stride, fill in ((n, 0), (n + 37, 7)):                            # a padded stack; garbage in the outputs
        got = direct(list(c['members']), c['y'], c['y'].shape, c['thresholds'], c['windows'], stride=stride, fill=fill)
        assert got[0] == 0
        for g, w in zip(got[1:], want):
            np.testing.assert_array_equal(g, w)


def test_bad_arguments_are_errors():
    import dl4ds_amd._lib as L
    c = CASES['tiny']()
    rows, y, shape = list(c['members'][:2]), c['y'], c['y'].shape
    for over in (dict(K=0), dict(K=257), dict(T=0), dict(T=17), dict(S=0), dict(n=y.size - 1), dict(B=4), dict(stride_arg=y.size - 1),
                 dict(H=0), dict(null=('members',)), dict(null=('obs',)), dict(null=('thr',)), dict(null=('win',)),
                 dict(null=('sums',)), dict(null=('cont',)), dict(null=('valid',))):
        st, sums, _, _ = direct(rows, y, shape, (0.5,), (1, 3), fill=5, **over)
        assert st != 0 and 'ensemble_fss' in L.load().dl4ds_last_error().decode(), over
        assert (sums == 5).all()                                          # nothing was written
    for thr, win in (((np.nan,), (1,)), ((np.inf,), (1,)), ((0.5,), (0,)), ((0.5,), (1, -2))):
        assert direct(rows, y, shape, thr, win)[0] != 0


def test_sums_close_to_the_bound_and_the_refusal_beyond_it():
    """400 x 400 cells, every member forecasts the event everywhere: with K = 32 a window that holds the whole field has F =
    H*W*(K*H*W)^2 = 4.19e18, within a factor of two of 2^62 = 4.61e18, and is legal; with K = 34 it is 4.73e18: refused by the
    Python layer and by the C entry"""
    import dl4ds_amd._lib as L
    from dl4ds_amd.metrics import neighbourhood_ensemble_scores
    y = np.ones((1, 400, 400, 1), np.float32)
    y[0, :170] = 0.0
    one = np.ones(y.shape, np.float32)
    x = np.broadcast_to(one, (32,) + y.shape)
    got = neighbourhood_ensemble_scores(y, x, (0.5,), windows=(1, 399, 1000))
    R.assert_same(got, R.scores(x, y, (0.5,), (1, 399, 1000)))
    assert 1 << 61 < got['sums'][0, 0, 0, 2, 1] == 160000 * (32 * 160000) ** 2 < 1 << 62
    with pytest.raises(ValueError, match=r'2\^62.*largest legal window for K = 34, H = 400, W = 400 is 397'):
        neighbourhood_ensemble_scores(y, np.broadcast_to(one, (34,) + y.shape), (0.5,), windows=(1, 398))
    st, sums, _, _ = direct([one], y, y.shape, (0.5,), (1, 398), repeat=34, fill=3)
    assert st != 0 and '2^62' in L.load().dl4ds_last_error().decode() and (sums == 3).all()
    st, sums, _, _ = direct([one], y, y.shape, (0.5,), (1, 397), repeat=34)
    rows = R.window_sums(np.ones((400, 1), np.int64), 397)[:, 0]          # cells of the window per row; the same per column
    assert st == 0 and sums[0, 0, 0, 1, 1] == 34 * 34 * int((rows * rows).sum()) ** 2


def test_two_workspace_chunks_with_32_bit_prefixes():
    """512 x 512 fields, THRESHOLD_GROUP thresholds, K = 128: K * W = 65536 > NARROW_MAX, so 8 * 2 * 512 * 513 * 4 B = 16.03 MiB of
    32-bit row prefixes per field (plus 32 KiB of validity bits): seven fields per WS_BUDGET.  Four such fields are one chunk, so
    the call has eight: two chunks, seven fields and one.  The stack is four distinct members, each 32 times: c, cf, Cs and X are
    32 times, D, F and Fv 32^2 times those of the four-member ensemble (K co scales like cf), O is the same."""
    shape, thr, win, rep = (8, 512, 512, 1), (0.1, 0.5, 1.0, 2.0, 3.0, 5.0, 8.0, 12.0), (3, 64), 32
    r = np.random.default_rng(512)
    y, p = precip_pair(r, shape)
    x = ensemble(r, p, 4, 0.3)
    y[1, 100:110, 7:300] = np.nan
    assert 4 * rep * shape[2] > NARROW_MAX and 1 <= WS_BUDGET // (THRESHOLD_GROUP * 2 * 512 * 513 * 4 + 512 * 8 * 8) < shape[0]
    st, sums, cont, valid = direct(list(x), y, shape, thr, win, repeat=rep)
    assert st == 0
    wsums, wcont, wvalid = R.integer_sums(x, y, thr, win)
    np.testing.assert_array_equal(sums, wsums * np.array([rep * rep, rep * rep, 1, rep * rep, rep]))
    np.testing.assert_array_equal(cont, wcont * np.array([1, rep]))
    np.testing.assert_array_equal(valid, wvalid)


# ------------------------------------------------------------------------------------------------ through the model
LR, SCALE = (16, 20), 2
HR = (LR[0] * SCALE, LR[1] * SCALE)


def mc_model():                                             # (the builder and size of tests/test_gpu_ensemble_score.py)
    import dl4ds_amd.models as PM
    return PM.net_postupsampling('resnet', 'spc', SCALE, 1, 0, LR, n_filters=8, n_blocks=2, dropout_rate=0.3, dropout_variant='mcdrop',
                                 seed=1)


def fields(n, seed=0, grid=LR, c=1):
    return np.random.default_rng(seed).standard_normal((n,) + tuple(grid) + (c,)).astype(np.float32)


def test_score_neighbourhood_is_predict_ensemble_plus_the_host_entry():
    from dl4ds_amd.metrics import neighbourhood_ensemble_scores
    m = mc_model()
    x = fields(7, 1)
    y = m.predict(x) + 0.05 * fields(7, 2, HR)
    y[2, 3, 4, 0] = np.nan
    thr = sorted(float(np.nanquantile(y, q)) for q in (0.5, 0.9, 0.1))
    res = m.score_neighbourhood(x, y, 6, thr, (1, 3, 9), seed=77, batch_size=3)
    plain = m.predict_ensemble(x, 6, seed=77, batch_size=3, return_members=True)
    for k in ('mean', 'std', 'min', 'max', 'quantiles'):
        assert res[k].tobytes() == plain[k].tobytes(), k
    assert 'members' not in res
    got = res['neighbourhood']
    want = neighbourhood_ensemble_scores(y, plain['members'], thr, (1, 3, 9))
    for k in want:
        assert np.asarray(got[k]).tobytes() == np.asarray(want[k]).tobytes(), k
    R.assert_same(got, R.scores(plain['members'], y, thr, (1, 3, 9)), 'score_neighbourhood')
    assert got['n_valid'].sum() == y.size - 1
    with pytest.raises(ValueError, match='y_true'):
        m.score_neighbourhood(x, y[:, :-1], 4, thr)


def test_verify_neighbourhood(tmp_path):
    """Events are decided in the model's units: the result equals the host entry on the raw members, the transformed observation
    and the transformed thresholds."""
    import dl4ds_amd
    from dl4ds_amd.metrics import neighbourhood_ensemble_scores
    from dl4ds_amd.preprocessing import StandardScaler
    m = mc_model()
    kelvin = (281.0 + 12.0 * np.random.default_rng(12).standard_normal((5,) + HR + (1,))).astype(np.float32)
    mask = np.ones(HR)
    mask[:3] = 0
    for sc in (None, StandardScaler(axis=None).fit(kelvin)):
        thr = [0.0, 0.8] if sc is None else [281.0, 295.5]
        arr = fields(5, 14, HR) if sc is None else np.asarray(sc.transform(kelvin), np.float32).reshape(kelvin.shape)
        y_model = arr.copy() if sc is None else np.asarray(sc.transform(kelvin.copy()), np.float32).reshape(kelvin.shape)
        thr_model = thr if sc is None else [float(np.asarray(sc.transform(np.full((2,) + HR + (1,), t)), np.float32).ravel()[0])
                                            for t in thr]
        kw = dict(seed=21, batch_size=2, scaler=sc)
        res = dl4ds_amd.verify_neighbourhood(m, arr, SCALE, 6, thr, (1, 5), y_true=None if sc is None else kelvin, mask=mask,
                                             save_path=str(tmp_path), **kw)
        ens = dl4ds_amd.predict_ensemble(m, arr, SCALE, 6, **kw)
        for k in ('mean', 'std', 'min', 'max', 'quantiles'):
            assert res[k].tobytes() == ens[k].tobytes(), k
        raw = dl4ds_amd.predict_ensemble(m, arr, SCALE, 6, return_members=True, seed=21, batch_size=2)['members']
        got = res['neighbourhood']
        want = neighbourhood_ensemble_scores(y_model, raw, thr_model, (1, 5), mask=mask)
        for k in want:
            assert np.asarray(got[k]).tobytes() == np.asarray(want[k]).tobytes(), k
        assert got['n_valid'].sum() == 5 * (HR[0] - 3) * HR[1]
        saved = np.load(tmp_path / 'y_hat_neighbourhood.npz')
        assert set(saved.files) == {k for k in res if k != 'neighbourhood'} | {'neighbourhood_' + k for k in got}
        again = dl4ds_amd.NeighbourhoodVerifier(m, arr, SCALE, 6, thr, (1, 5), y_true=None if sc is None else kelvin, mask=mask,
                                                array_in_hr=True, **kw).run()
        for k in got:
            assert np.asarray(got[k]).tobytes() == np.asarray(again['neighbourhood'][k]).tobytes(), k
