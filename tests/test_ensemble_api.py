"""MC-dropout ensemble prediction, the parts that need no GPU: the C ABI declares and exports the three new entries, the public
names resolve and keep ``predict``'s parameters, arguments are validated before anything touches the device, the numpy restatement
tests/ensemble_ref.py says what np.quantile says, and the rule that carries the ensemble's std through a scaler is exact for affine
inverse transforms."""
import inspect
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from tests import ensemble_ref as R
from tests import scaler_ref as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_ENTRIES = ('dl4ds_ensemble_reduce', 'dl4ds_graph_dropout_reseed', 'dl4ds_graph_dropout_mc_count')


def test_header_declares_and_library_exports_the_new_entries():
    import ctypes
    import dl4ds_amd._lib as L
    protos = L.parse_header()
    for name in NEW_ENTRIES:
        assert name in protos, f'{name} is not declared in include/dl4ds_hip.h'
    ret, args = protos['dl4ds_ensemble_reduce']
    assert ret is ctypes.c_int and len(args) == 11
    assert args[1:4] == [ctypes.c_size_t] * 3 and args[5] is ctypes.c_int
    assert all(a is ctypes.c_void_p for a in [args[0], args[4]] + args[6:])
    assert protos['dl4ds_graph_dropout_reseed'][1] == [ctypes.c_void_p, ctypes.c_long]           # 64-bit seed
    if not os.path.exists(L.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    lib = L.load()
    for name in NEW_ENTRIES:
        assert hasattr(lib, name), f'{name} declared in include/dl4ds_hip.h but not exported'
    header = open(L.HEADER_PATH).read()
    doc = header[:header.index('int dl4ds_ensemble_reduce(')].rsplit('/*', 1)[1]
    assert 'blocks.py:658-676' in doc, 'the header comment names the reference code the entry serves'


def test_lazy_exports_and_signatures():
    import dl4ds_amd
    import dl4ds_amd.inference as I
    assert dl4ds_amd.predict_ensemble is I.predict_ensemble and dl4ds_amd.EnsemblePredictor is I.EnsemblePredictor
    base = inspect.signature(I.predict).parameters
    ens = inspect.signature(I.predict_ensemble).parameters
    added = ['n_members', 'quantiles', 'seed', 'return_members']
    assert [p for p in ens if p not in base] == added
    assert [p for p in ens if p in base] == list(base), 'same names in the same relative order'
    for name, p in base.items():
        if name == 'save_fname':
            assert ens[name].default == 'y_hat_ensemble.npz'
        else:
            assert ens[name].default == p.default and ens[name].kind == p.kind, name
    assert ens['n_members'].default is inspect.Parameter.empty
    assert ens['quantiles'].default == () and ens['seed'].default is None and ens['return_members'].default is False
    # the class mirrors Predictor: constructor-then-run, Predictor's defaults (array_in_hr=False) plus the added parameters
    pb = inspect.signature(I.Predictor.__init__).parameters
    pe = inspect.signature(I.EnsemblePredictor.__init__).parameters
    assert [p for p in pe if p not in pb] == added and [p for p in pe if p in pb] == list(pb)
    assert all(pe[k].default == pb[k].default for k in pb if k != 'save_fname')
    assert list(inspect.signature(I.EnsemblePredictor.run).parameters) == ['self']
    from dl4ds_amd.graph import Model
    assert list(inspect.signature(Model.predict_ensemble).parameters) == \
        ['self', 'inputs', 'n_members', 'batch_size', 'quantiles', 'seed', 'return_members']
    assert inspect.signature(Model.predict_ensemble).parameters['batch_size'].default == 32
    assert callable(Model.reseed_dropout)


class StubModel:
    """What predict_ensemble sees of a model before it runs: enough to fail loudly if validation came too late."""
    name = 'stub_spc'
    input_shapes = [(8, 8, 1)]

    def predict_ensemble(self, *a, **k):
        raise AssertionError('the model was reached with invalid arguments')


BAD = [dict(n_members=0), dict(n_members=257), dict(n_members=-3), dict(n_members=4.0), dict(n_members='4'), dict(n_members=True),
       dict(n_members=None), dict(n_members=4, quantiles=[-0.01]), dict(n_members=4, quantiles=[0.5, 1.0001]),
       dict(n_members=4, quantiles=[float('nan')]), dict(n_members=4, quantiles=5), dict(n_members=4, quantiles=[[0.1, 0.2]]),
       dict(n_members=4, quantiles=['a']), dict(n_members=4, quantiles=list(np.linspace(0, 1, 33))),
       dict(n_members=4, seed=1.5), dict(n_members=4, batch_size=0)]


def test_argument_validation_needs_no_device():
    """in a fresh interpreter: every bad call raises ValueError and the library has not been loaded afterwards"""
    code = f'''
import sys
sys.path.insert(0, {ROOT!r})
import numpy as np
import dl4ds_amd, dl4ds_amd._lib as L
from tests.test_ensemble_api import StubModel, BAD
from dl4ds_amd.graph import Model, check_ensemble_args
x = np.zeros((3, 16, 16, 1), np.float32)
for kw in BAD:
    kw = dict(kw)
    K = kw.pop('n_members')
    for call in (lambda: dl4ds_amd.predict_ensemble(StubModel(), x, 2, K, **kw),
                 lambda: dl4ds_amd.EnsemblePredictor(StubModel(), x, 2, K, **kw).run(),
                 lambda: Model.predict_ensemble(StubModel(), [x], K, **kw)):
        try:
            call()
        except ValueError:
            continue
        raise SystemExit(f'no ValueError for n_members={{K!r}} {{kw}}')
K, q = check_ensemble_args(np.int64(5), (0, 0.5, 1), seed=2**64 - 1, batch_size=np.int32(3))
assert K == 5 and type(K) is int and q.dtype == np.float32 and q.tolist() == [0.0, 0.5, 1.0]
assert check_ensemble_args(256, ())[1].shape == (0,) and check_ensemble_args(1, 0.5)[1].tolist() == [0.5]
assert L._lib is None and not L._inited, 'validation loaded the library'
print('ok')
'''
    r = subprocess.run([sys.executable, '-c', code], capture_output=True, text=True, cwd=ROOT)
    assert r.returncode == 0 and r.stdout.strip().endswith('ok'), r.stdout + r.stderr


def test_reference_restatement_is_numpys_linear_quantile():
    rng = np.random.default_rng(0)
    for K in (1, 2, 3, 8, 17, 64, 256):
        m = (281.0 + 12.0 * rng.standard_normal((K, 50))).astype(np.float32)
        q = np.array([0.0, 0.05, 0.25, 0.5, 0.75, 0.95, 1.0])
        ref = R.ensemble_ref(m, q)
        assert all(v.dtype == np.float32 for v in ref.values())
        assert ref['quantiles'].shape == (7, 50) and ref['mean'].shape == (50,)
        m64 = m.astype(np.float64)
        np.testing.assert_array_equal(ref['quantiles'], np.quantile(m64, q, axis=0, method='linear').astype(np.float32))
        np.testing.assert_array_equal(ref['quantiles'], np.percentile(m64, 100 * q, axis=0).astype(np.float32))      # the default
        np.testing.assert_array_equal(ref['quantiles'][0], ref['min'])
        np.testing.assert_array_equal(ref['quantiles'][-1], ref['max'])
        # the textbook form: a[lo] + (pos - lo) (a[min(lo + 1, K - 1)] - a[lo]) on the sorted values, to float32 rounding
        a = np.sort(m64, axis=0)
        for j, qq in enumerate(q):
            pos = qq * (K - 1)
            lo = int(np.floor(pos))
            hand = a[lo] + (pos - lo) * (a[min(lo + 1, K - 1)] - a[lo])
            assert R.ulp_diff(ref['quantiles'][j], hand.astype(np.float32)).max() <= 1
        np.testing.assert_array_equal(ref['std'], np.sqrt(np.mean((m64 - m64.mean(0)) ** 2, axis=0)).astype(np.float32))
        if K == 1:
            assert (ref['std'] == 0).all()
            for k in ('mean', 'min', 'max'):
                np.testing.assert_array_equal(ref[k], m[0])
            np.testing.assert_array_equal(ref['quantiles'], np.broadcast_to(m[0], (7, 50)))
    assert R.ensemble_ref(m, ())['quantiles'].shape == (0, 50)
    assert R.integer_position(5, [0.0, 0.25, 0.3, 1.0]).tolist() == [True, True, False, True]
    bad = m.copy()
    bad[3, 7] = np.nan
    assert all(np.isnan(v[..., 7]).all() and not np.isnan(np.delete(v, 7, axis=-1)).any() for v in R.ensemble_ref(bad, q).values())


def test_check_stats_enforces_its_bounds():
    rng = np.random.default_rng(1)
    m = rng.standard_normal((9, 40)).astype(np.float32)
    q = [0.0, 0.3, 0.5, 1.0]
    good = R.ensemble_ref(m, np.asarray(q, np.float32).astype(np.float64))
    R.check_stats(good, m, q)
    up = lambda a: np.nextafter(a, np.float32(np.inf))                      # noqa: E731
    ok = dict(good, mean=up(good['mean']))
    R.check_stats(ok, m, q)                                                  # 1 ulp on the mean is inside the bound
    for k in ('min', 'max'):
        with pytest.raises(AssertionError):
            R.check_stats(dict(good, **{k: up(good[k])}), m, q)
    with pytest.raises(AssertionError):
        R.check_stats(dict(good, std=up(up(good['std']))), m, q)
    moved = good['quantiles'].copy()
    moved[2] = up(moved[2])                                                  # q = 0.5 of 9 values: an order statistic
    with pytest.raises(AssertionError):
        R.check_stats(dict(good, quantiles=moved), m, q)


@pytest.mark.parametrize('kind', ['standard', 'minmax'])
def test_std_goes_through_a_scaler_by_its_slope(kind):
    """slope = inverse_transform(ones) - inverse_transform(zeros) in float64; for the affine-per-cell inverse transforms of both
    scalers slope * std(members) IS std(inverse_transform(members)), to fp64 rounding"""
    rng = np.random.default_rng(2)
    H, W, K = 12, 10, 16
    data = 281.0 + 12.0 * rng.standard_normal((30, H, W))
    members = rng.standard_normal((K, 4, H, W))
    if kind == 'standard':
        st = {k: v.reshape(H, W) for k, v in S.stats(data, 0).items()}
        inv = lambda x: S.standard_inverse(x, st['mean64'], st['std64'])                   # noqa: E731
    else:
        at = S.minmax_from(*(S.stats(data, 0)[k + '64'].reshape(H, W) for k in ('min', 'max')))
        inv = lambda x: S.minmax_inverse(x, at)                                            # noqa: E731
    slope = inv(np.ones((H, W))) - inv(np.zeros((H, W)))
    want = np.std(np.stack([inv(members[k]) for k in range(K)]), axis=0)
    got = np.abs(slope) * np.std(members, axis=0)
    # rounding of the 2 K affine evaluations at magnitude ~300 around a spread of ~10: a few hundred fp64 ulps at most
    assert np.max(np.abs(got - want) / want) < 1e-12
    assert np.max(np.abs(got - want) / want) < 4 * K * np.finfo(np.float64).eps * (np.abs(inv(members[0])).max() / want.min())


def test_scaler_slope_helper_evaluates_per_sample_in_float64():
    from dl4ds_amd.inference import scaler_slope

    class Affine:
        seen = []

        def inverse_transform(self, x):
            self.seen.append((x.shape, x.dtype))
            return np.squeeze(x) * 3.5 + 270.0

    sc = Affine()
    s = scaler_slope(sc, (6, 5, 1))
    assert s.dtype == np.float64 and s.shape == (6, 5) and np.all(s == 3.5)
    assert sc.seen == [((2, 6, 5, 1), np.dtype(np.float64))] * 2      # (two samples: a lone one would lose its axis to the squeeze)


def test_existing_entry_points_keep_their_source_signature():
    import dl4ds_amd.inference as I
    assert str(inspect.signature(I.predict)) == (
        "(trainer, array, scale, array_in_hr=True, static_vars=None, predictors=None, time_window=None, time_metadata=None, "
        "interpolation='inter_area', batch_size=64, scaler=None, save_path=None, save_fname='y_hat.npy', return_lr=False, "
        "device='GPU')")
    src = inspect.getsource(I)
    assert len(re.findall(r'create_batch_hr_lr\(', src)) == 1, 'one input preparation shared by predict and predict_ensemble'
