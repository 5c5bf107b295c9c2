"""MC-dropout ensembles on the device: csrc/ensemble.hip through the C ABI on synthetic member stacks, and
Model.predict_ensemble / dl4ds_amd.predict_ensemble through small models, against the fp64 numpy restatement tests/ensemble_ref.py.

Bounds (tests/ensemble_ref.py check_stats; derived, not tuned): min, max and quantiles whose position (K - 1) q is an integer are
EQUAL to numpy's; mean, std and interpolated quantiles are within 1 ulp of float32 (the kernel evaluates in fp64 like the
restatement, which leaves an error of order K 2^-53; what remains is the final rounding to float32 plus a possible double rounding).
The probabilities cross the C ABI as float32, so the restatement is given the float32-rounded values.
"""
import ctypes
import warnings

import numpy as np
import pytest

from tests import ensemble_ref as R

pytestmark = pytest.mark.gpu

KS = [1, 2, 3, 5, 8, 16, 17, 32, 63, 64, 65, 128, 256]
QS = {0: [], 1: [0.5], 3: [0.0, 0.25, 1.0], 7: [0.0, 0.05, 0.25, 0.5, 0.75, 0.95, 1.0]}


def stack(rng, kind, K, n):
    z = rng.standard_normal((K, n))
    if kind == 'kelvin':
        return (281.0 + 12.0 * z).astype(np.float32)
    if kind == 'zero':
        return (z * np.exp(rng.uniform(-6, 2, (1, n)))).astype(np.float32)          # mixed sign, spreads over several decades
    return (np.round(2.0 * z) / 2.0).astype(np.float32)                             # 'ties': values rounded to 0.5


def reduce_call(members, q=(), stride=None, want=('mean', 'std', 'min', 'max', 'quantiles')):
    """dl4ds_ensemble_reduce on a host stack (K, n) placed with member stride ``stride``; outputs not in ``want`` are passed as null."""
    import dl4ds_amd._lib as L
    from dl4ds_amd.device import DeviceArray
    lib = L.lib()
    K, n = members.shape
    stride = n if stride is None else stride
    host = np.full((K, max(stride, n)), np.float32(-777.0))       # (a stride below n is an error the library must report)
    host[:, :n] = members
    dev = DeviceArray.from_numpy(host)
    q32 = np.asarray(q, np.float32)
    nq = q32.size
    qc = (ctypes.c_float * max(nq, 1))(*q32.tolist())
    outs = {k: DeviceArray((n,)) for k in ('mean', 'std', 'min', 'max') if k in want}
    if 'quantiles' in want and nq:
        outs['quantiles'] = DeviceArray((nq, n))
    p = {k: (outs[k].ptr if k in outs else None) for k in ('mean', 'std', 'min', 'max', 'quantiles')}
    L.check(lib.dl4ds_ensemble_reduce(dev.ptr, K, n, stride, qc, nq, p['mean'], p['std'], p['min'], p['max'], p['quantiles']))
    res = {k: v.numpy() for k, v in outs.items()}
    if 'quantiles' in want and not nq:
        res['quantiles'] = np.empty((0, n), np.float32)
    return res


@pytest.mark.parametrize('K', KS)
def test_reduce_kernel_against_numpy(K):
    rng = np.random.default_rng(1000 + K)
    for n in (1, 5, 4099):
        for kind in ('kelvin', 'zero', 'ties'):
            m = stack(rng, kind, K, n)
            for stride in (n, n + 13, n + 4 - n % 4 + 8):               # equal, odd padding, padding that keeps rows 16-byte aligned
                for nq, q in QS.items():
                    got = reduce_call(m, q, stride)
                    R.check_stats(got, m, q, f'K={K} n={n} {kind} stride={stride} nq={nq}')


def test_reduce_kernel_aligned_rows_take_the_vector_path():
    """n a multiple of four with 16-byte aligned rows (the 4-elements-per-lane instances), every K class"""
    rng = np.random.default_rng(7)
    for K in (2, 4, 7, 8, 12, 16, 24, 32, 48, 64):
        m = stack(rng, 'kelvin', K, 8192)
        got = reduce_call(m, QS[7], 8192 + 64)
        R.check_stats(got, m, QS[7], f'K={K} n=8192 aligned')


def test_reduce_kernel_full_size():
    rng = np.random.default_rng(16)
    n = 16 * 512 * 512
    m = (281.0 + 12.0 * rng.standard_normal((16, n), dtype=np.float32)).astype(np.float32)
    q = [0.05, 0.5, 0.95]
    got = reduce_call(m, q)
    R.check_stats(got, m, q, 'K=16 n=16x512x512 kelvin')


@pytest.mark.parametrize('K', [1, 2, 5, 16, 33, 64, 100, 256])
def test_nan_and_inf_follow_numpy(K):
    rng = np.random.default_rng(K)
    n = 304
    m = stack(rng, 'kelvin', K, n)
    pick = lambda: int(rng.integers(0, K))                                       # noqa: E731
    m[pick(), 3] = np.nan
    m[pick(), 10] = np.inf
    m[pick(), 11] = -np.inf
    m[0, 12], m[K - 1, 12] = np.inf, (-np.inf if K > 1 else np.inf)              # both infinities in one element
    m[pick(), 13] = np.inf
    m[pick(), 13] = np.nan                                                        # NaN wins over inf
    m[:, 20] = np.inf
    m[:, 21] = np.nan
    m[pick(), 300:304] = np.nan                                                   # a whole 16-byte group
    q = QS[7]
    got = reduce_call(m, q)
    ref = R.ensemble_ref(m, np.asarray(q, np.float32).astype(np.float64))
    for k in ('mean', 'std', 'min', 'max', 'quantiles'):
        assert np.isnan(got[k][..., 3]).all() and np.isnan(got[k][..., 21]).all() and np.isnan(got[k][..., 300:]).all(), k
        np.testing.assert_array_equal(np.isnan(got[k]), np.isnan(ref[k]), err_msg=k)
    R.check_stats(got, m, q, f'K={K} with NaN / inf')


def test_null_outputs_are_skipped_and_calls_are_reproducible():
    rng = np.random.default_rng(3)
    for K, n in ((16, 4096), (20, 1001), (100, 257)):
        m = stack(rng, 'zero', K, n)
        q = QS[3]
        full = reduce_call(m, q)
        again = reduce_call(m, q)
        for k in full:
            assert full[k].tobytes() == again[k].tobytes(), (K, k)
        for want in (('mean',), ('std', 'max'), ('quantiles',), ('min', 'quantiles'), ()):
            part = reduce_call(m, q, want=want)
            assert set(part) == set(want)
            for k in want:
                assert part[k].tobytes() == full[k].tobytes(), (K, want, k)


def test_bad_arguments_are_errors():
    import dl4ds_amd._lib as L
    m = np.zeros((4, 8), np.float32)
    with pytest.raises(L.Dl4dsHipError):
        reduce_call(m, [1.5])
    with pytest.raises(L.Dl4dsHipError):
        reduce_call(m, [], stride=4)
    with pytest.raises(L.Dl4dsHipError):
        reduce_call(np.zeros((257, 8), np.float32))


# ------------------------------------------------------------------------------------------------ through the model
LR, SCALE = (16, 20), 2


def mc_model(variant='mcdrop', rate=0.3, seed=1, **kw):
    import dl4ds_amd.models as PM
    cfg = dict(n_filters=8, n_blocks=2, dropout_rate=rate, dropout_variant=variant, seed=seed)
    cfg.update(kw)
    return PM.net_postupsampling('resnet', 'spc', SCALE, 1, cfg.pop('n_aux', 0), LR, **cfg)


def lr_fields(n, seed=0, c=1, grid=LR):
    return np.random.default_rng(seed).standard_normal((n,) + tuple(grid) + (c,)).astype(np.float32)


def same_dict(a, b):
    assert set(a) == set(b)
    return all(a[k].tobytes() == b[k].tobytes() for k in a)


def run_to_run_difference(model, x, seed):
    """Two identically seeded single calls: 0.0 when the forward pass is bit-reproducible (expected: no floating-point atomics)."""
    model.reseed_dropout(seed)
    a = model(x)
    model.reseed_dropout(seed)
    b = model(x)
    d = float(np.max(np.abs(a.astype(np.float64) - b)))
    print(f'two identically seeded forward passes differ by at most {d:.3e}')
    return d


@pytest.mark.parametrize('variant', ['mcdrop', 'mcgaussiandrop', 'mcspatialdrop'])
def test_member_k_is_the_kth_forward_pass(variant):
    m = mc_model(variant)
    assert m.graph.dropout_mc_count() > 0
    N, K, s = 6, 5, 1234
    x = lr_fields(N)
    tol = run_to_run_difference(m, [x], s)
    m.reseed_dropout(s)
    singles = np.stack([m([x]) for _ in range(K)])
    assert np.abs(singles[0] - singles[1]).max() > 0, 'the MC layer is not active at inference'
    q = [0.1, 0.5, 1.0]
    res = m.predict_ensemble([x], K, batch_size=N, quantiles=q, seed=s, return_members=True)
    assert res['members'].shape == (K, N) + m.output_shape and res['quantiles'].shape == (3, N) + m.output_shape
    if tol == 0.0:
        np.testing.assert_array_equal(res['members'], singles)
    else:
        print(f'NOT bit-reproducible run to run ({tol:.3e}); members compared within that')
        assert np.abs(res['members'].astype(np.float64) - singles).max() <= tol
    R.check_stats({k: res[k] for k in ('mean', 'std', 'min', 'max', 'quantiles')}, res['members'], q, variant)


def test_seed_semantics():
    m = mc_model()
    x = lr_fields(5, 2)
    a = m.predict_ensemble(x, 4, batch_size=5, quantiles=[0.5], seed=7)
    b = m.predict_ensemble(x, 4, batch_size=5, quantiles=[0.5], seed=7)
    c = m.predict_ensemble(x, 4, batch_size=5, quantiles=[0.5], seed=8)
    assert 'members' not in a and same_dict(a, b)
    assert (a['mean'] != c['mean']).any() and (a['std'] > 0).any() and (c['std'] > 0).any()
    d = m.predict_ensemble(x, 4, batch_size=5, seed=None)
    e = m.predict_ensemble(x, 4, batch_size=5, seed=None)
    assert d['quantiles'].shape == (0, 5) + m.output_shape
    assert not same_dict(d, e)


@pytest.mark.parametrize('variant', ['vanilla', None])
def test_model_without_mc_dropout_warns_and_degenerates(variant):
    m = mc_model(variant, rate=0.3 if variant else 0)
    assert m.graph.dropout_mc_count() == 0
    x = lr_fields(4, 3)
    y = m.predict(x)
    assert y.tobytes() == m.predict(x).tobytes(), 'predict is not bit-reproducible run to run'
    with pytest.warns(UserWarning, match='mcdrop.*mcgaussiandrop.*mcspatialdrop'):
        res = m.predict_ensemble(x, 7, quantiles=[0.3], seed=1)
    assert (res['std'] == 0).all()
    for k in ('mean', 'min', 'max'):
        assert res[k].tobytes() == y.tobytes(), k
    assert res['quantiles'][0].tobytes() == y.tobytes()


def test_batches_that_do_not_divide_n():
    m = mc_model()
    x = lr_fields(7, 4)
    K, s = 3, 99
    res = m.predict_ensemble(x, K, batch_size=3, quantiles=[0.25, 0.5], seed=s, return_members=True)
    # the masks depend on the batch split: restate it with single calls over the same batches
    m.reseed_dropout(s)
    want = np.empty_like(res['members'])
    for i in range(0, 7, 3):
        for k in range(K):
            want[k, i:i + 3] = m([x[i:i + 3]])
    np.testing.assert_array_equal(res['members'], want)
    R.check_stats({k: res[k] for k in ('mean', 'std', 'min', 'max', 'quantiles')}, res['members'], [0.25, 0.5], 'N=7 batch=3')


def test_two_input_model():
    m = mc_model(n_aux=2)
    assert len(m.input_shapes) == 2
    N = 3
    x = lr_fields(N, 5)
    st = np.random.default_rng(6).standard_normal((N,) + tuple(m.input_shapes[1])).astype(np.float32)
    res = m.predict_ensemble([x, st], 4, batch_size=2, quantiles=[0.5], seed=5, return_members=True)
    m.reseed_dropout(5)
    want = np.empty_like(res['members'])
    for i in range(0, N, 2):
        for k in range(4):
            want[k, i:i + 2] = m([x[i:i + 2], st[i:i + 2]])
    np.testing.assert_array_equal(res['members'], want)
    R.check_stats({k: res[k] for k in ('mean', 'std', 'min', 'max', 'quantiles')}, res['members'], [0.5], 'two inputs')


def test_input_on_another_grid():
    m = mc_model()
    grid = (12, 24)
    x = lr_fields(3, 8, grid=grid)
    res = m.predict_ensemble(x, 4, quantiles=[0.5], seed=3, return_members=True)
    assert res['mean'].shape == (3, grid[0] * SCALE, grid[1] * SCALE, 1)
    sib = m.resized(grid)
    sib.reseed_dropout(3)                                          # the seed is applied to the graph that runs
    want = np.stack([sib([x]) for _ in range(4)])
    np.testing.assert_array_equal(res['members'], want)
    assert (res['std'] > 0).any()
    R.check_stats({k: res[k] for k in ('mean', 'std', 'min', 'max', 'quantiles')}, res['members'], [0.5], 'other grid')


def test_recurrent_model_through_the_public_entry():
    import dl4ds_amd
    import dl4ds_amd.models as PM
    from dl4ds_amd.utils import spatiotemporal_to_spatial_samples
    T, hr = 3, (LR[0] * SCALE, LR[1] * SCALE)
    m = PM.recnet_postupsampling('resnet', 'spc', SCALE, 1, 0, LR, T, n_filters=8, n_blocks=1, dropout_rate=0.3,
                                 dropout_variant='mcspatialdrop', seed=2)
    assert len(m.output_shape) == 4
    arr = np.random.default_rng(9).standard_normal((6,) + hr + (1,)).astype(np.float32)
    q = [0.5, 0.9]
    res, lr = dl4ds_amd.predict_ensemble(m, arr, SCALE, 4, quantiles=q, seed=11, time_window=T, batch_size=3, return_lr=True,
                                         return_members=True)
    y = dl4ds_amd.predict(m, arr, SCALE, time_window=T, batch_size=3)
    assert res['mean'].shape == y.shape and res['members'].shape == (4,) + y.shape and res['quantiles'].shape == (2,) + y.shape
    assert lr.shape[0] == 6 - (T - 1)
    raw = m.predict_ensemble([lr], 4, batch_size=3, quantiles=q, seed=11, return_members=True)
    for k in ('mean', 'std', 'min', 'max'):
        np.testing.assert_array_equal(res[k], spatiotemporal_to_spatial_samples(raw[k], T))
    for k in ('quantiles', 'members'):
        for j in range(raw[k].shape[0]):
            np.testing.assert_array_equal(res[k][j], spatiotemporal_to_spatial_samples(raw[k][j], T))
    R.check_stats({k: raw[k] for k in ('mean', 'std', 'min', 'max', 'quantiles')}, raw['members'], q, 'recnet 5-D')
    assert (res['std'] > 0).any()


def test_scaler_is_applied_to_values_and_its_slope_to_the_spread(tmp_path):
    import dl4ds_amd
    from dl4ds_amd.preprocessing import StandardScaler
    m = mc_model()
    hr = (LR[0] * SCALE, LR[1] * SCALE)
    rng = np.random.default_rng(12)
    kelvin = (281.0 + 12.0 * rng.standard_normal((5,) + hr + (1,))).astype(np.float32)
    sc = StandardScaler(axis=None).fit(kelvin)
    arr = np.asarray(sc.transform(kelvin), np.float32).reshape(kelvin.shape)
    kw = dict(quantiles=[0.5], seed=21, batch_size=5, return_members=True)
    plain = dl4ds_amd.predict_ensemble(m, arr, SCALE, 6, **kw)
    res = dl4ds_amd.EnsemblePredictor(m, arr, SCALE, 6, array_in_hr=True, scaler=sc, save_path=str(tmp_path), **kw).run()
    for k in ('mean', 'min', 'max'):
        R_ = np.asarray(sc.inverse_transform(plain[k]), np.float32)
        assert res[k].tobytes() == R_.tobytes(), k
    assert res['members'][2].tobytes() == np.asarray(sc.inverse_transform(plain['members'][2]), np.float32).tobytes()
    slope = float(sc.std_.reshape(-1)[0])
    want_std = (np.float64(slope) * plain['std'].astype(np.float64)).astype(np.float32).reshape(res['std'].shape)
    assert R.ulp_diff(res['std'], want_std).max() <= 1
    # ... and that IS the spread of the transformed members, to float32 rounding of the members themselves
    spread = np.std(res['members'].astype(np.float64), axis=0)
    assert np.abs(res['std'] - spread).max() <= 4 * np.finfo(np.float32).eps * np.abs(res['members']).max()
    saved = np.load(tmp_path / 'y_hat_ensemble.npz')
    assert set(saved.files) == set(res) and all(saved[k].tobytes() == res[k].tobytes() for k in res)


def test_no_shared_noise_state_between_models():
    a, b, c = mc_model(seed=1), mc_model(seed=1), mc_model(seed=5)
    x = lr_fields(4, 13)
    ya = a.predict(x)
    with warnings.catch_warnings():
        warnings.simplefilter('error')
        c.predict_ensemble(x, 4, seed=None)
    yb = b.predict(x)
    assert ya.tobytes() == yb.tobytes()
    assert (ya != a.predict(x)).any()                      # (the noise of ONE model does advance from call to call)


def test_stack_that_does_not_fit_is_a_memory_error():
    import dl4ds_amd.models as PM
    m = PM.net_postupsampling('resnet', 'spc', 4, 1, 0, (128, 128), n_filters=8, n_blocks=1, dropout_rate=0.2,
                              dropout_variant='mcdrop', seed=1)
    x = np.zeros((2048, 128, 128, 1), np.float32)
    with pytest.raises(MemoryError, match='batch_size'):                       # 256 x 2048 x 512^2 x 4 B = 512 GiB
        m.predict_ensemble(x, 256, batch_size=2048)
    # the refused allocation is over with the exception: the next launches must not inherit it as their own error
    res = m.predict_ensemble(x[:2], 3, seed=1)
    assert np.isfinite(res['mean']).all() and np.isfinite(m.predict(x[:2])).all()
