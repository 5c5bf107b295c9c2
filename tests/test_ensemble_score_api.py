"""On-device ensemble verification, the parts that need no GPU: the C ABI declares and exports the new entry, the public names
resolve and keep ``predict``'s parameters, arguments are validated before anything touches the device, and the numpy restatement
tests/ensemble_score_ref.py gives the known answers of CRPS, ranks and the tie draw."""
import inspect
import os
import subprocess
import sys

import numpy as np

from tests import ensemble_score_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ADDED = ['n_members', 'y_true', 'quantiles', 'seed', 'fair', 'mask']


def test_header_declares_and_library_exports_the_new_entry():
    import ctypes
    import dl4ds_amd._lib as L
    protos = L.parse_header()
    assert 'dl4ds_ensemble_score' in protos, 'dl4ds_ensemble_score is not declared in include/dl4ds_hip.h'
    ret, args = protos['dl4ds_ensemble_score']
    P, Z, I, U = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int, ctypes.c_long
    assert ret is ctypes.c_int
    assert args == [P, Z, Z, Z, P, Z, U, P, I, U, P, I, P, P, P, P, P, P, P, P]
    if not os.path.exists(L.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    assert hasattr(L.load(), 'dl4ds_ensemble_score'), 'declared in include/dl4ds_hip.h but not exported'
    header = open(L.HEADER_PATH).read()
    doc = header[:header.index('int dl4ds_ensemble_score(')].rsplit('/*', 1)[1]
    assert 'blocks.py:658-676' in doc, 'the header comment names the reference code the entry serves'
    for word in ('0x9E3779B97F4A7C15', '0xBF58476D1CE4E5B9', '0x94D049BB133111EB', 'tie', 'fair', 'VALID'):
        assert word in doc, f'the header comment spells out the semantics ({word})'


def test_lazy_exports_and_signatures():
    import dl4ds_amd
    import dl4ds_amd.inference as I
    import dl4ds_amd.metrics as M
    assert dl4ds_amd.verify_ensemble is I.verify_ensemble and dl4ds_amd.EnsembleVerifier is I.EnsembleVerifier
    assert dl4ds_amd.ensemble_scores is M.ensemble_scores
    base = inspect.signature(I.predict).parameters
    ver = inspect.signature(I.verify_ensemble).parameters
    assert [p for p in ver if p not in base] == ADDED
    assert [p for p in ver if p in base] == list(base), 'same names in the same relative order'
    assert list(ver)[:9] == ['trainer', 'array', 'scale', 'n_members', 'y_true', 'quantiles', 'seed', 'fair', 'mask']
    assert list(ver)[9:] == list(base)[3:], "the remaining parameters of predict follow in predict's order"
    for name, p in base.items():
        if name != 'save_fname':
            assert ver[name].default == p.default and ver[name].kind == p.kind, name
    assert ver['save_fname'].default.endswith('.npz')
    assert ver['n_members'].default is inspect.Parameter.empty and ver['y_true'].default is None
    assert ver['quantiles'].default == () and ver['seed'].default is None and ver['fair'].default is False
    assert ver['mask'].default is None
    pb = inspect.signature(I.Predictor.__init__).parameters
    pv = inspect.signature(I.EnsembleVerifier.__init__).parameters
    assert [p for p in pv if p not in pb] == ADDED and [p for p in pv if p in pb] == list(pb)
    assert all(pv[k].default == pb[k].default for k in pb if k != 'save_fname')
    assert all(pv[k].default == ver[k].default for k in ADDED[1:])
    assert list(inspect.signature(I.EnsembleVerifier.run).parameters) == ['self']
    from dl4ds_amd.graph import Model
    assert str(inspect.signature(Model.score_ensemble)) == \
        '(self, inputs, y_true, n_members, batch_size=32, quantiles=(), seed=None, fair=False, scale=None, return_fields=False)'
    assert list(inspect.signature(M.ensemble_scores).parameters)[:7] == \
        ['y_true', 'members', 'quantiles', 'fair', 'seed', 'mask', 'batch_size']
    es = inspect.signature(M.ensemble_scores).parameters
    assert es['quantiles'].default == () and es['fair'].default is False and es['seed'].default == 0
    assert es['mask'].default is None and es['batch_size'].default is None


class StubModel:
    """What verify_ensemble sees of a model before it runs: enough to fail loudly if validation came too late."""
    name = 'stub_spc'
    input_shapes = [(8, 8, 1)]
    output_shape = (16, 16, 1)

    def score_ensemble(self, *a, **k):
        raise AssertionError('the model was reached with invalid arguments')

    predict_ensemble = score_ensemble


BAD = [dict(n_members=0), dict(n_members=257), dict(n_members=4.0), dict(n_members=True), dict(n_members=None),
       dict(n_members=4, quantiles=[-0.01]), dict(n_members=4, quantiles=[float('nan')]), dict(n_members=4, quantiles=[[0.1, 0.2]]),
       dict(n_members=4, quantiles=list(np.linspace(0, 1, 33))), dict(n_members=4, seed=1.5), dict(n_members=4, seed='a'),
       dict(n_members=4, fair=1), dict(n_members=4, fair='yes'), dict(n_members=4, fair=None), dict(n_members=4, batch_size=0),
       dict(n_members=4, array_in_hr=False),                                                    # y_true missing
       dict(n_members=4, y_true=np.zeros((3, 16, 15, 1), np.float32)),                          # wrong y_true shapes
       dict(n_members=4, y_true=np.zeros((2, 16, 16, 1), np.float32)),
       dict(n_members=4, y_true=np.zeros((3, 16, 16), np.float32), array_in_hr=False),          # LR 16 x 16 -> HR 32 x 32
       dict(n_members=4, y_true=np.zeros((16, 16), np.float32)),
       dict(n_members=4, scaler=object()),                                                      # y_true missing with a scaler
       dict(n_members=4, time_window=2)]


def test_argument_validation_needs_no_device():
    """in a fresh interpreter: every bad call raises ValueError and the library has not been loaded afterwards"""
    code = f'''
import sys
sys.path.insert(0, {ROOT!r})
import numpy as np
import dl4ds_amd, dl4ds_amd._lib as L
from tests.test_ensemble_score_api import StubModel, BAD
from dl4ds_amd.graph import Model
x = np.zeros((3, 16, 16, 1), np.float32)
for kw in BAD:
    kw = dict(kw)
    K = kw.pop('n_members')
    calls = [lambda: dl4ds_amd.verify_ensemble(StubModel(), x, 2, K, **dict(dict(array_in_hr=True), **kw)),
             lambda: dl4ds_amd.EnsembleVerifier(StubModel(), x, 2, K, **dict(dict(array_in_hr=True), **kw)).run()]
    if not set(kw) - {{'quantiles', 'seed', 'fair', 'batch_size'}}:
        calls.append(lambda: Model.score_ensemble(StubModel(), [x], x, K, **kw))
        if type(K) is int and 0 < K <= 256:
            calls.append(lambda: dl4ds_amd.ensemble_scores(x, np.zeros((K,) + x.shape, np.float32), **kw))
    for call in calls:
        try:
            call()
        except ValueError as e:
            if 'time_window' in kw:
                assert 'time_window' in str(e) and 'not defined' in str(e), str(e)
            continue
        raise SystemExit(f'no ValueError for n_members={{K!r}} {{kw}}')
for bad in (np.zeros((3, 2, 16, 16, 1)), np.zeros((4,) + x.shape[:-1]), np.zeros(())):
    try:
        dl4ds_amd.ensemble_scores(x, bad)
    except ValueError:
        continue
    raise SystemExit(f'no ValueError for members of shape {{bad.shape}}')
assert L._lib is None and not L._inited, 'validation loaded the library'
print('ok')
'''
    r = subprocess.run([sys.executable, '-c', code], capture_output=True, text=True, cwd=ROOT)
    assert r.returncode == 0 and r.stdout.strip().endswith('ok'), r.stdout + r.stderr


def test_tie_hash_restatements_agree_and_stay_in_range():
    rng = np.random.default_rng(0)
    g = rng.integers(0, 2**40, 2000)
    m = rng.integers(0, 257, 2000)
    for seed in (0, 1, 12345, 2**64 - 1):
        arr = R.tie_array(seed, g, m)
        assert arr.tolist() == [R.tie(seed, int(a), int(b)) for a, b in zip(g, m)]
        assert (arr >= 0).all() and (arr <= m).all()
    assert (R.tie_array(7, g, np.zeros_like(m)) == 0).all(), 'no tie: no draw'
    # splitmix64's published first output for state 0 (the finaliser of 0x9E3779B97F4A7C15): pins the constants
    assert R.tie(0, 0, 2**32 - 1) == 0xE220A8397B1DCDAF >> 32
    draws = R.tie_array(3, np.arange(60000), np.full(60000, 2))
    share = np.bincount(draws, minlength=3) / 60000.0
    assert np.abs(share - 1 / 3).max() < 0.01, share                 # (5 sigma of a fair three-sided draw is 0.0096)


def test_restatement_known_answers():
    rng = np.random.default_rng(1)
    y = rng.standard_normal(50).astype(np.float32)
    # K = 1: |x - y| in both forms, variance 0
    x = rng.standard_normal((1, 50)).astype(np.float32)
    for fair in (False, True):
        r = R.score_ref(x, y, fair=fair)
        np.testing.assert_array_equal(r['crps'], np.abs(x[0].astype(np.float64) - y))
        assert (r['var'] == 0).all()
    # every member equal to the observation: CRPS 0, squared error 0, the rank is the tie draw alone
    r = R.score_ref(np.broadcast_to(y, (7, 50)), y, quantiles=[0.5], seed=5)
    assert (r['crps'] == 0).all() and (r['sqerr'] == 0).all() and (r['equal'] == 7).all() and (r['below'] == 0).all()
    assert r['rank'].tolist() == [R.tie(5, g, 7) for g in range(50)] and r['covered'].all()
    # two members by hand: x = (1, 4), y = 2: (1 + 2) / 2 - 3 / 4 = 0.75; fair: 1.5 - 3 / 2 = 0
    x2 = np.array([[1.0], [4.0]], np.float32)
    y2 = np.array([2.0], np.float32)
    assert R.score_ref(x2, y2)['crps'][0] == 0.75 and R.score_ref(x2, y2, fair=True)['crps'][0] == 0.0
    r = R.score_ref(x2, y2, quantiles=[0.0, 0.25, 0.5, 1.0])
    assert r['sqerr'][0] == 0.25 and r['var'][0] == 4.5 and r['rank'][0] == 1
    assert r['covered'][:, 0].tolist() == [False, False, True, True] and r['Q'][:, 0].tolist() == [1.0, 1.75, 2.5, 4.0]
    assert r['interp'][:, 0].tolist() == [False, True, True, False]
    # fair and plain differ by the factor K / (K - 1) on the pair term
    for K in (2, 3, 8, 17):
        x = rng.standard_normal((K, 50)).astype(np.float32)
        first = np.abs(x.astype(np.float64) - y).mean(axis=0)
        plain, fair = R.score_ref(x, y)['crps'], R.score_ref(x, y, fair=True)['crps']
        np.testing.assert_allclose(first - fair, (first - plain) * K / (K - 1), rtol=1e-13)
        assert (fair <= plain).all()
    # an observation below / above every member has rank 0 / K, and distinct values use no tie draw whatever the seed
    x = rng.standard_normal((9, 50)).astype(np.float32)
    assert (R.score_ref(x, x.min(axis=0) - 1)['rank'] == 0).all() and (R.score_ref(x, x.max(axis=0) + 1)['rank'] == 9).all()
    a, b = R.score_ref(x, y, seed=1), R.score_ref(x, y, seed=2)
    assert (a['equal'] == 0).all() and (a['rank'] == b['rank']).all() and (a['rank'] == a['below']).all()
    # the sorted form the kernel evaluates IS the pairwise sum
    d = np.sort(x.astype(np.float64) - y, axis=0)
    pair = ((2 * np.arange(9) - 9 + 1)[:, None] * d).sum(axis=0)
    np.testing.assert_allclose(np.abs(x.astype(np.float64) - y).mean(axis=0) - pair / 81, a['crps'], rtol=1e-12)


def test_restatement_validity_scale_and_folds():
    rng = np.random.default_rng(2)
    x = rng.standard_normal((5, 4, 6, 3)).astype(np.float32)
    y = rng.standard_normal((4, 6, 3)).astype(np.float32)
    y[0, 0, 0] = np.nan
    y[1, 1, 1] = np.inf
    x[2, 2, 2, 2] = np.nan
    x[4, 3, 3, 0] = -np.inf
    scale = np.full((6, 3), 2.0, np.float32)
    scale[5, 2] = 0.0
    scale[4, 1] = np.nan
    r = R.score_ref(x, y, quantiles=[0.5], scale=scale)
    bad = [(0, 0, 0), (1, 1, 1), (2, 2, 2), (3, 3, 0)] + [(n, 5, 2) for n in range(4)] + [(n, 4, 1) for n in range(4)]
    assert int((~r['valid']).sum()) == len(bad) and all(not r['valid'][i] for i in bad)
    for k in ('crps', 'sqerr', 'var'):
        np.testing.assert_array_equal(np.isnan(r[k]), ~r['valid'])
    assert (r['rank'][~r['valid']] == -1).all() and not r['covered'][0][~r['valid']].any()
    plain = R.score_ref(x, y, quantiles=[0.5])
    v = r['valid']
    np.testing.assert_allclose(r['crps'][v], 2 * plain['crps'][v], rtol=1e-15)
    np.testing.assert_allclose(r['var'][v], 4 * plain['var'][v], rtol=1e-15)
    np.testing.assert_array_equal(r['rank'][v], plain['rank'][v])
    ps, pc = R.folds(r)
    assert ps.shape == (4, 4) and pc.shape == (4, 6, 3) and ps[:, 3].sum() == v.sum() == pc[3].sum()
    s = R.summary(r, 5)
    assert s['rank_histogram'].sum() == s['n_valid'] == v.sum() and s['rank_histogram'].shape == (6,)
    assert abs(R.ulp32(1.0) - 2.0**-23) == 0 and R.ulp32(0.0) > 0
