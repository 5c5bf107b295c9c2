"""Exceedance-probability verification of ensembles, the parts that need no GPU: the numpy restatement tests/exceedance_ref.py
against independent formulations and tables worked by hand, the host arithmetic ``exceedance_from_counts`` against it, validation
before anything touches the device, the rule that bounds the narrow partial sums, the public names and the C declaration."""
import inspect
import os
import subprocess
import sys
from fractions import Fraction

import numpy as np
import pytest

from tests import exceedance_cases as C
from tests import exceedance_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ADDED = ['n_members', 'thresholds', 'y_true', 'seed', 'mask']


def ulp(x):
    return np.spacing(np.abs(np.asarray(x, np.float64)))


# ------------------------------------------------------------------------------------------------ the restatement
@pytest.mark.parametrize('K', [1, 2, 5, 16])
def test_restatement_against_independent_formulations(K):
    """tie-heavy samples: Brier as a mean in fp64, the ROC area as Mann-Whitney with ties, the ROC end points"""
    rng = np.random.default_rng(100 + K)
    m, y = C.data(rng, 'deadzone', K, (40, 30))
    thr = np.asarray([0.0, 0.6, -0.7], np.float32)
    from dl4ds_amd.ensemble_score import exceedance_from_counts
    cr = R.counts_ref(m, y, thr)
    ref = R.scores_ref(m, y, thr)
    got = exceedance_from_counts(cr['table'], cr['cell'], cr['sample'], K, thr)          # the product's arithmetic, same answers
    R.assert_same(got, {k: v for k, v in ref.items() if not k.endswith('_field')}, f'K={K}', fields=False)
    assert (m == 0).mean() > 0.2 and cr['valid'].all(), 'many values tie with the threshold 0.0, and forecasts tie among themselves'
    for t in range(3):
        p = cr['c'][:, t].astype(np.float64) / K
        o = cr['o'][:, t].astype(np.float64)
        assert abs(ref['brier'][t] - np.mean((p - o) ** 2)) <= 1e-12 and abs(got['brier'][t] - np.mean((p - o) ** 2)) <= 1e-12
        ev, ne = p[o == 1], p[o == 0]
        try:
            from scipy.stats import mannwhitneyu
            u = mannwhitneyu(ev.reshape(-1), ne.reshape(-1), alternative='two-sided', method='asymptotic').statistic
        except ImportError:
            u = (ev.reshape(-1)[:, None] > ne.reshape(-1)[None]).sum() + 0.5 * (ev.reshape(-1)[:, None] == ne.reshape(-1)[None]).sum()
        assert abs(ref['roc_auc'][t] - u / (ev.size * ne.size)) <= 1e-12 and abs(got['roc_auc'][t] - u / (ev.size * ne.size)) <= 1e-12
        assert (ref['roc_pod'][t, 0], ref['roc_pofd'][t, 0]) == (0.0, 0.0)
        assert (ref['roc_pod'][t, -1], ref['roc_pofd'][t, -1]) == (1.0, 1.0)
        assert (np.diff(ref['roc_pod'][t]) >= 0).all() and (np.diff(ref['roc_pofd'][t]) >= 0).all()
        # the trapezoid area under the ROC points is the same number
        trap = np.sum(np.diff(ref['roc_pofd'][t]) * (ref['roc_pod'][t][1:] + ref['roc_pod'][t][:-1]) / 2)
        assert abs(trap - ref['roc_auc'][t]) <= 1e-12
        assert ref['table'][t].sum() == ref['n_valid'][t] == y.size
        assert (ref['table'][t] * np.arange(K + 1)[:, None]).sum() == cr['c'][:, t].sum()
    np.testing.assert_array_equal(ref['probability_field'], (cr['c'] / np.float32(K)).astype(np.float32))


def perfect_table(K):
    """A perfect forecast: 6 non-events all with c = 0, 4 events all with c = K.
    brier 0, reliability 0, resolution = uncertainty = 0.4 * 0.6 = 6/25, bss 1, roc_auc 1, fair Brier 0 (no member disagrees)."""
    t = np.zeros((1, K + 1, 2), np.int64)
    t[0, 0, 0], t[0, K, 1] = 6, 4
    return t


def constant_table(K):
    """A constant forecast c = K/2 (K even): 6 non-events and 2 events, all in bin K/2.
    brier = (6 * 1/4 + 2 * 1/4) / 8 = 1/4, observed frequency of the bin 1/4 = the base rate: reliability (1/2 - 1/4)^2 = 1/16,
    resolution 0, uncertainty 3/16, bss = 1 - (1/4)/(3/16) = -1/3, roc_auc 1/2 (all tied),
    fair Brier = 1/4 - 8 (K/2)^2 / (K^2 (K - 1) 8) = 1/4 - 1 / (4 (K - 1))."""
    t = np.zeros((1, K + 1, 2), np.int64)
    t[0, K // 2] = (6, 2)
    return t


def zeros_like_sums(T, N=1, s=(1,)):
    return np.zeros((T, 4) + s, np.int64), np.zeros((N, T, 4), np.int64)


def test_tables_worked_by_hand():
    from dl4ds_amd.ensemble_score import exceedance_from_counts
    for K in (2, 4, 10):
        for fn in (lambda t: R.from_counts_ref(t, *zeros_like_sums(1), K, [0.0]),
                   lambda t: exceedance_from_counts(t, *zeros_like_sums(1), K, [0.0])):
            r = fn(perfect_table(K))
            assert (r['brier'][0], r['reliability'][0], r['bss'][0], r['roc_auc'][0], r['brier_fair'][0]) == (0.0, 0.0, 1.0, 1.0, 0.0)
            assert r['resolution'][0] == r['uncertainty'][0] == 6 / 25 and r['base_rate'][0] == 0.4
            assert r['roc_pod'][0].tolist() == [0.0] + [1.0] * (K + 1) and r['roc_pofd'][0].tolist() == [0.0] * (K + 1) + [1.0]
            obs = r['observed_frequency'][0]
            assert obs[0] == 0.0 and obs[K] == 1.0 and np.isnan(obs[1:K]).all()
            r = fn(constant_table(K))
            assert (r['brier'][0], r['reliability'][0], r['resolution'][0], r['uncertainty'][0]) == (0.25, 1 / 16, 0.0, 3 / 16)
            assert r['bss'][0] == float(Fraction(-1, 3)) and r['roc_auc'][0] == 0.5
            assert r['brier_fair'][0] == float(Fraction(1, 4) - Fraction(1, 4 * (K - 1)))
            assert r['forecast_count'][0].tolist() == [0] * (K // 2) + [8] + [0] * (K // 2)
            assert r['roc_pod'][0].tolist() == [0.0] * (K // 2 + 1) + [1.0] * (K // 2 + 1)
            assert r['forecast_probability'].tolist() == [i / K for i in range(K + 1)]


# ------------------------------------------------------------------------------------------------ exceedance_from_counts
def random_counts(rng, K, T, N, s, scale=1):
    """consistent integer outputs of a made-up run: counts drawn per cell and sample"""
    m, y = C.data(rng, 'deadzone', K, (N,) + s)
    thr = np.asarray([0.0, 0.7, -0.6, 5.0][:T], np.float32)
    cr = R.counts_ref(m, y, thr)
    return cr['table'] * scale, cr['cell'] * scale, cr['sample'] * scale, thr


@pytest.mark.parametrize('K', [1, 3, 16, 256])
def test_from_counts_equals_the_fractions(K):
    from dl4ds_amd.ensemble_score import exceedance_from_counts
    rng = np.random.default_rng(200 + K)
    # the second scale: counts beyond 2^53 (K^2 n beyond 2^63 for K = 256), products beyond 2^64; every scaled sum still an int64
    for scale in (1, (1 << (48 if K <= 16 else 40)) + 12345):
        table, cell, sample, thr = random_counts(rng, K, 4, 6, (5, 7), scale)
        assert scale == 1 or (int(table[0].sum()) * K * K > 1 << 55 and int(cell.max()) < 1 << 62 and int(sample.max()) < 1 << 62)
        got = exceedance_from_counts(table, cell, sample, K, thr)
        ref = R.from_counts_ref(table, cell, sample, K, thr)
        assert set(got) == set(ref)
        for k in R.INT_KEYS:
            np.testing.assert_array_equal(got[k], ref[k], err_msg=k)
            assert np.asarray(got[k]).dtype == np.int64, k
        for k in R.FLOAT_KEYS:
            g, r = np.asarray(got[k], np.float64), np.asarray(ref[k], np.float64)
            np.testing.assert_array_equal(np.isnan(g), np.isnan(r), err_msg=k)
            ok = ~np.isnan(r)
            assert (np.abs(g - r)[ok] <= ulp(r)[ok]).all(), (k, scale)
        # Murphy's decomposition: at most 257 terms, each at most 1, in fp64
        rebuilt = got['reliability'] - got['resolution'] + got['uncertainty']
        assert (np.abs(got['brier'] - rebuilt) <= 1e-12).all()
        assert np.isnan(got['brier_fair']).all() == (K == 1)
        assert np.isnan(got['bss'][3]) and np.isnan(got['roc_auc'][3]) and got['n_events'][3] == 0      # threshold 5.0: no event
        assert np.isnan(got['roc_pod'][3]).all() and not np.isnan(got['roc_pofd'][3]).any()


def test_from_counts_nan_exactly_on_zero_denominators():
    from dl4ds_amd.ensemble_score import exceedance_from_counts
    K = 4
    table = np.zeros((4, K + 1, 2), np.int64)
    table[1, :, 0] = (5, 3, 0, 1, 0)                              # [1]: no event
    table[2, :, 1] = (0, 0, 2, 3, 4)                              # [2]: only events
    table[3] = [[4, 0], [2, 1], [1, 1], [0, 3], [0, 5]]           # [3]: both; [0]: no valid element
    cell, sample = zeros_like_sums(4, N=2, s=(3,))
    cell[3, :, 0] = (2, 1, 2, 7)
    sample[1, 3] = (3, 1, 5, 9)
    r = exceedance_from_counts(table, cell, sample, K, [0, 1, 2, 3])
    scal = {k: np.isnan(r[k]).tolist() for k in R.SCALARS}
    assert scal['base_rate'] == scal['brier'] == scal['brier_fair'] == scal['reliability'] == scal['resolution'] == \
        scal['uncertainty'] == [True, False, False, False]
    assert scal['bss'] == scal['roc_auc'] == [True, True, True, False]
    assert np.isnan(r['roc_pod'][:2]).all() and not np.isnan(r['roc_pod'][2:]).any()
    assert np.isnan(r['roc_pofd'][[0, 2]]).all() and not np.isnan(r['roc_pofd'][[1, 3]]).any()
    np.testing.assert_array_equal(np.isnan(r['observed_frequency']), r['forecast_count'] == 0)
    np.testing.assert_array_equal(np.isnan(r['brier_map']), cell[:, 0] == 0)
    np.testing.assert_array_equal(np.isnan(r['brier_per_sample']), sample[..., 0] == 0)
    assert r['brier_map'][3, 0] == 7 / (16 * 2) and r['base_rate_map'][3, 0] == 0.5 and r['forecast_rate_map'][3, 0] == 2 / 8
    assert r['bss_map'][3, 0] == 1 - (7 / 32) / 0.25 and r['brier_per_sample'][1, 3] == 9 / 48
    one = exceedance_from_counts(np.array([[[3, 0], [0, 2]]]), *zeros_like_sums(1), 1, [0.5])
    assert np.isnan(one['brier_fair'][0]) and one['brier'][0] == 0.0 and one['roc_auc'][0] == 1.0
    with pytest.raises(ValueError):
        exceedance_from_counts(table, cell, sample, K + 1, [0, 1, 2, 3])


# ------------------------------------------------------------------------------------------------ the cases of the GPU tests
def test_gpu_cases_are_nan_exactly_where_they_are_built_to_be():
    from dl4ds_amd.ensemble_score import exceedance_from_counts
    cases = [(c['name'],) + C.build(c) for c in C.synthetic_cases() if c['K'] <= 65]
    cases.append(('per cell',) + C.per_cell_case())
    for name, m, y, thr, what in cases:
        ref = R.scores_ref(m, y, thr, fields=False)
        K = m.shape[0]
        got = exceedance_from_counts(ref['table'], ref['cell_sums'], ref['sample_sums'], K, thr)
        for k in R.SCALARS:                                 # the product's host arithmetic is NaN in the same places
            np.testing.assert_array_equal(np.isnan(got[k]), np.isnan(ref[k]), err_msg=f'{name}: {k}')
        for t, w in enumerate(what):
            for k, nan in C.expected_nan(w, K).items():
                assert bool(np.isnan(ref[k][t])) == nan, (name, t, w, k, ref[k][t])
            if w == 'all':
                assert ref['n_events'][t] == ref['n_valid'][t] > 0 and ref['table'][t, :K].sum() == 0, (name, t)
            if w == 'none':
                assert ref['n_events'][t] == 0 and ref['table'][t, 1:].sum() == 0, (name, t)
            if w == 'empty':
                assert ref['n_valid'][t] == 0
    m, y, mask, bad = C.invalid_case()
    ref = R.scores_ref(m, y, [0.0])
    assert ref['n_valid'][0] == y.size - bad and (ref['count_field'] == -1).sum() == bad
    zeros = np.concatenate([m.reshape(-1), y.reshape(-1)])
    assert (np.signbit(zeros) & (zeros == 0)).sum() > 100 and ((zeros == 0) & ~np.signbit(zeros)).sum() > 100


# ------------------------------------------------------------------------------------------------ validation, rule, names
def test_threshold_validation():
    from dl4ds_amd.ensemble_score import check_exceedance_args
    t = check_exceedance_args([1, 2.5, -3], (4, 5, 1))
    assert t.dtype == np.float32 and t.shape == (3,) and t.tolist() == [1.0, 2.5, -3.0]
    assert check_exceedance_args(0.5, (4,)).shape == (1,)
    assert check_exceedance_args([2.0, 2.0, 1.0], ()).tolist() == [2.0, 2.0, 1.0]            # any order, repeats
    f = np.zeros((2, 4, 5, 1))
    f[0, 1, 1, 0] = np.nan                                                                    # NaN inside a field is legal
    t = check_exceedance_args(f, (4, 5, 1))
    assert t.shape == (2, 4, 5, 1) and np.isnan(t[0, 1, 1, 0]) and t.dtype == np.float32
    assert check_exceedance_args(list(range(16)), (3,)).shape == (16,)
    assert check_exceedance_args(f, None).shape == (2, 4, 5, 1), 'without a sample shape the shape of fields is not looked at'
    for bad in ([], [np.inf], ['a'], np.zeros((17, 2))):
        with pytest.raises(ValueError):
            check_exceedance_args(bad, None)
    for bad in ([], list(range(17)), ['a'], 'abc', [None], [True], [np.inf], [-np.inf], [np.nan], [1e39], [1 + 2j], None,
                np.zeros((2, 4, 5)), np.zeros((2, 5, 4, 1)), np.zeros((17, 4, 5, 1)), np.zeros((0, 4, 5, 1)), [[1.0, 2.0]]):
        with pytest.raises(ValueError):
            check_exceedance_args(bad, (4, 5, 1))


class StubModel:
    """What verify_exceedance sees of a model before it runs: enough to fail loudly if validation came too late."""
    name = 'stub_spc'
    input_shapes = [(8, 8, 1)]
    output_shape = (16, 16, 1)

    def score_exceedance(self, *a, **k):
        raise AssertionError('the model was reached with invalid arguments')


BAD = [dict(n_members=0), dict(n_members=257), dict(n_members=4.0), dict(n_members=True), dict(n_members=None),
       dict(n_members=4, thresholds=[]), dict(n_members=4, thresholds=list(range(17))), dict(n_members=4, thresholds=['x']),
       dict(n_members=4, thresholds=[np.inf]), dict(n_members=4, thresholds=[np.nan]), dict(n_members=4, thresholds=None),
       dict(n_members=4, thresholds=np.zeros((2, 16, 15, 1))), dict(n_members=4, seed=1.5), dict(n_members=4, seed='a'),
       dict(n_members=4, batch_size=0),
       dict(n_members=4, array_in_hr=False),                                                    # y_true missing
       dict(n_members=4, y_true=np.zeros((3, 16, 15, 1), np.float32)),
       dict(n_members=4, y_true=np.zeros((2, 16, 16, 1), np.float32)),
       dict(n_members=4, y_true=np.zeros((16, 16), np.float32)),
       dict(n_members=4, scaler=object()),                                                      # y_true missing with a scaler
       dict(n_members=4, time_window=2)]


def test_argument_validation_needs_no_device():
    """in a fresh interpreter, with the library made unreachable: every bad call raises ValueError before anything asks for it"""
    code = f'''
import os, sys
sys.path.insert(0, {ROOT!r})
os.environ['DL4DS_HIP_LIB'] = '/nonexistent/libdl4ds_hip.so'
import numpy as np
import dl4ds_amd, dl4ds_amd._lib as L
from tests.test_exceedance_api import StubModel, BAD
from dl4ds_amd.graph import Model
x = np.zeros((3, 16, 16, 1), np.float32)
for kw in BAD:
    kw = dict(kw)
    K = kw.pop('n_members')
    thr = kw.pop('thresholds', [0.5])
    calls = [lambda: dl4ds_amd.verify_exceedance(StubModel(), x, 2, K, thr, **dict(dict(array_in_hr=True), **kw)),
             lambda: dl4ds_amd.ExceedanceVerifier(StubModel(), x, 2, K, thr, **dict(dict(array_in_hr=True), **kw)).run()]
    if not set(kw) - {{'seed', 'batch_size'}}:
        if np.ndim(thr) < 2:          # (the shape of a threshold field is checked once the model for the inputs' grid is known)
            calls.append(lambda: Model.score_exceedance(StubModel(), [x], x, K, thr, **kw))
        if type(K) is int and 0 < K <= 256 and 'seed' not in kw:
            calls.append(lambda: dl4ds_amd.exceedance_scores(x, np.zeros((K,) + x.shape, np.float32), thr, **kw))
    for call in calls:
        try:
            call()
        except ValueError as e:
            if 'time_window' in kw:
                assert 'time_window' in str(e) and 'not defined' in str(e) and 'verify_exceedance' in str(e), str(e)
            continue
        raise SystemExit(f'no ValueError for n_members={{K!r}} thresholds={{thr!r}} {{kw}}')
for bad in (np.zeros((3, 2, 16, 16, 1)), np.zeros((4,) + x.shape[:-1]), np.zeros(())):
    try:
        dl4ds_amd.exceedance_scores(x, bad, [0.5])
    except ValueError:
        continue
    raise SystemExit(f'no ValueError for members of shape {{bad.shape}}')
assert L._lib is None and not L._inited, 'validation loaded the library'
print('ok')
'''
    r = subprocess.run([sys.executable, '-c', code], capture_output=True, text=True, cwd=ROOT)
    assert r.returncode == 0 and r.stdout.strip().endswith('ok'), r.stdout + r.stderr


def test_call_splitting_rule():
    """A lane keeps sum (c - K o)^2 of its cell in 32 bits and the two counts in 16 bits each: it may walk at most
    min(65535, (2^32 - 1) // K^2) samples; the launch splits a call by that bound, which the library states itself."""
    import ctypes
    import dl4ds_amd._lib as L
    lib = L.load()
    out = ctypes.c_size_t(0)
    for K in (1, 2, 16, 255, 256):
        assert lib.dl4ds_ensemble_exceedance_walk_limit(K, ctypes.byref(out)) == 0
        w = out.value
        assert w == min(65535, (2**32 - 1) // (K * K)) and w >= 1
        assert w * K * K < 2**32 and w < 2**16, 'the 32-bit sum of squares and the 16-bit counts cannot overflow'
        assert w * 256 < 2**32 and w * 1024 < 2**32, 'nor sum c of a lane, nor a histogram bin of a workgroup'
    for K in (0, 257):
        assert lib.dl4ds_ensemble_exceedance_walk_limit(K, ctypes.byref(out)) != 0
    src = open(os.path.join(ROOT, 'dl4ds_amd', 'csrc', 'exceedance.hip')).read()
    assert 'OVERFLOW RULE' in src and 'exc_walk_limit' in src, 'the source states the rule'
    device = src.split('namespace {', 1)[1].split('}  // namespace', 1)[0]
    assert 'double' not in device and 'float s' not in device, 'no floating-point accumulation: the kernels hold no double at all'


def test_lazy_exports_and_signatures():
    import dl4ds_amd
    import dl4ds_amd.inference as I
    import dl4ds_amd.metrics as M
    from dl4ds_amd.graph import Model
    assert dl4ds_amd.verify_exceedance is I.verify_exceedance and dl4ds_amd.ExceedanceVerifier is I.ExceedanceVerifier
    assert dl4ds_amd.exceedance_scores is M.exceedance_scores
    base = inspect.signature(I.predict).parameters
    ver = inspect.signature(I.verify_exceedance).parameters
    assert [p for p in ver if p not in base] == ADDED
    assert list(ver)[:8] == ['trainer', 'array', 'scale', 'n_members', 'thresholds', 'y_true', 'seed', 'mask']
    assert list(ver)[8:] == list(base)[3:], "the remaining parameters of predict follow in predict's order"
    for name, p in base.items():
        if name != 'save_fname':
            assert ver[name].default == p.default and ver[name].kind == p.kind, name
    assert ver['save_fname'].default == 'y_hat_exceedance.npz'
    assert ver['n_members'].default is inspect.Parameter.empty and ver['thresholds'].default is inspect.Parameter.empty
    assert ver['y_true'].default is None and ver['seed'].default is None and ver['mask'].default is None
    pb = inspect.signature(I.Predictor.__init__).parameters
    pv = inspect.signature(I.ExceedanceVerifier.__init__).parameters
    assert [p for p in pv if p not in pb] == ADDED and [p for p in pv if p in pb] == list(pb)
    assert all(pv[k].default == pb[k].default for k in pb if k != 'save_fname')
    assert all(pv[k].default == ver[k].default for k in ADDED[2:])
    assert list(inspect.signature(I.ExceedanceVerifier.run).parameters) == ['self']
    assert str(inspect.signature(Model.score_exceedance)) == \
        '(self, inputs, y_true, n_members, thresholds, batch_size=32, seed=None, return_fields=False)'
    assert str(inspect.signature(M.exceedance_scores)) == \
        '(y_true, members, thresholds, mask=None, batch_size=None, return_fields=False)'
    assert open(os.path.join(ROOT, 'dl4ds_amd', 'inference.py')).read().count('create_batch_hr_lr(') == 1


def test_header_declares_and_library_exports_the_new_entry():
    import ctypes
    import dl4ds_amd._lib as L
    protos = L.parse_header()
    assert 'dl4ds_ensemble_exceedance' in protos, 'dl4ds_ensemble_exceedance is not declared in include/dl4ds_hip.h'
    ret, args = protos['dl4ds_ensemble_exceedance']
    P, Z, I = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int
    assert ret is ctypes.c_int
    assert args == [P, Z, Z, Z, P, Z, P, I, I, P, P, P, P], 'short* count_dev is a pointer like the others'
    assert protos['dl4ds_ensemble_exceedance_walk_limit'] == (ctypes.c_int, [Z, P])
    if not os.path.exists(L.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    assert hasattr(L.load(), 'dl4ds_ensemble_exceedance'), 'declared in include/dl4ds_hip.h but not exported'
    header = open(L.HEADER_PATH).read()
    assert 'short* count_dev' in header
    doc = header[:header.index('int dl4ds_ensemble_exceedance(')].rsplit('/*', 1)[1]
    assert 'blocks.py:658-676' in doc, 'the header comment names the reference code the entry serves'
    for word in ('VALID', 'thr_per_cell', '-0.0', 'count_dev', 'sample_out_dev', 'cell_acc_dev', 'table_dev', 'ADDED', 'overwritten',
                 '(c - K o)^2', 'Integer arithmetic only', 'Refused'):
        assert word in doc, f'the header comment spells out the semantics ({word})'
