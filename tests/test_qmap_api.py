"""CPU-side checks of the quantile-mapping bias correction: the numpy restatement tests/qmap_ref.py (the expected side of
tests/test_gpu_qmap.py) against independent answers, and the argument validation, exports and persistence of
dl4ds_amd.postprocessing, none of which touches the device."""
import numpy as np
import pytest

from tests import qmap_cases as cases
from tests import qmap_ref as ref

ULP = np.float64(2.0) ** -24


def ulps_apart(a, b):
    """distance in float32 steps of two finite float32 arrays"""
    def ordered(v):
        i = np.asarray(v, np.float32).view(np.int32).astype(np.int64)
        return np.where(i < 0, -(i & 0x7FFFFFFF), i)
    return np.abs(ordered(a) - ordered(b))


# ------------------------------------------------------------------------------------------------ the restatement: the table
@pytest.mark.parametrize('x, q', [
    (cases.field(37, 12, 2), np.linspace(0, 1, 11)), (cases.field(64, 7, 3), cases.probabilities(101)),
    (cases.zeros70(), np.linspace(0, 1, 21)), (cases.signed_zeros(), (0.0, 0.3, 1.0)), (cases.spoiled(), cases.probabilities(7)),
    (cases.field(513, 3, 4), np.linspace(0, 1, 256))], ids=['normal', 'precip', 'zeros70', 'signed_zeros', 'spoiled', 'Q256'])
def test_table_against_np_quantile(x, q):
    """np.quantile(method='linear') evaluates its own fp64 formula on the finite values; the two formulas differ by a few 2^-53
    relative, which can move the final rounding to float32 by at most one step"""
    table, valid = ref.quantile_table(x, q)
    assert table.dtype == np.float32 and table.shape == (len(q), x.shape[1]) and valid.dtype == np.int64
    for c in range(x.shape[1]):
        good = x[np.isfinite(x[:, c]), c].astype(np.float64)
        assert valid[c] == good.size
        if good.size == 0:
            assert np.isnan(table[:, c]).all()
            continue
        want = np.quantile(good, q, method='linear').astype(np.float32)
        assert (ulps_apart(table[:, c] + np.float32(0), want + np.float32(0)) <= 1).all(), c
    assert not np.signbit(table[table == 0]).any()                     # -0.0 counts as +0.0


def test_table_hand_worked():
    x = np.array([[4.0], [np.nan], [1.0], [-np.inf], [2.0], [np.inf], [3.0]], np.float32)     # valid: 1 2 3 4
    table, valid = ref.quantile_table(x, (0.0, 0.25, 0.5, 1.0))
    np.testing.assert_array_equal(table[:, 0], np.array([1.0, 1.75, 2.5, 4.0], np.float32))
    assert valid[0] == 4
    table, valid = ref.quantile_table(np.array([[np.nan, 7.5], [np.nan, np.nan]], np.float32), (0.1, 0.9))
    assert np.isnan(table[:, 0]).all() and valid[0] == 0
    np.testing.assert_array_equal(table[:, 1], np.float32([7.5, 7.5]))
    assert valid[1] == 1


# -------------------------------------------------------------------------------------------------- the restatement: the map
def test_eqm_interior_against_np_interp():
    """np.interp(v, m, o) in fp64 on strictly increasing tables is o_j + (o_j+1 - o_j) * t with t = (v - m_j) / (m_j+1 - m_j) exact
    to fp64.  The float32 evaluation rounds v - m_j, m_j+1 - m_j, their quotient t, o_j+1 - o_j and the product (o_j+1 - o_j) * t:
    five roundings on the t and product path, each at most 2^-24 relative, which together move the product by less than
    6 * 2^-24 * |o_j+1 - o_j| (t <= 1; the sixth covers the second-order terms); the final sum is rounded once more, at most
    2^-24 * |result| <= 2^-24 * max(|o_j|, |o_j+1|), the result lying between the knots up to the error just bounded.  Hence
    |got - want| <= 8 * 2^-24 * (|o_j+1 - o_j| + max(|o_j|, |o_j+1|)) with room to spare."""
    r = np.random.default_rng(11)
    Q, cells, B = 101, 9, 200
    for scale in (1e-2, 1.0, 1e3):
        m = np.sort(r.standard_normal((Q, cells)) * scale + 5 * scale, 0).astype(np.float32)
        o = np.sort(r.standard_normal((Q, cells)) * scale - 2 * scale, 0).astype(np.float32)
        assert (np.diff(m, axis=0) > 0).all() and (np.diff(o, axis=0) > 0).all()
        lo, hi = m[0].astype(np.float64), m[-1].astype(np.float64)
        v = (lo + (hi - lo) * r.random((B, cells)) * 0.999).astype(np.float32)
        v = np.maximum(v, m[0])
        out, counts, taken = ref.qmap_apply(v, m, o)
        assert taken['interior'].all() and counts == dict(n_nonfinite=0, n_unfitted=0, n_below=0, n_above=0)
        for c in range(cells):
            want = np.interp(v[:, c].astype(np.float64), m[:, c].astype(np.float64), o[:, c].astype(np.float64))
            j = np.searchsorted(m[:, c], v[:, c], side='right') - 1
            o0, o1 = o[j, c].astype(np.float64), o[j + 1, c].astype(np.float64)
            bound = 8 * ULP * (np.abs(o1 - o0) + np.maximum(np.abs(o0), np.abs(o1)))
            assert (np.abs(out[:, c].astype(np.float64) - want) <= bound).all()


def _tables(obs, model, q):
    return ref.quantile_table(obs, q)[0], ref.quantile_table(model, q)[0]


def test_identical_history_leaves_the_knots_alone():
    obs = cases.field(50, 8, 6)
    q = np.linspace(0, 1, 21)
    o, m = _tables(obs, obs.copy(), q)
    for kind in (0, 1):
        out, _, _ = ref.qmap_apply(o, m, o, None, kind)                  # every knot as a value
        np.testing.assert_array_equal(out, o)


def test_additive_shift_beyond_the_ends():
    obs = cases.field(50, 8, 8)
    model = obs + np.float32(3.0)
    q = cases.probabilities(21)
    o, m = _tables(obs, model, q)
    np.testing.assert_array_equal(m, o + np.float32(3.0))              # (the shift is exact at these magnitudes)
    v = np.concatenate([m[:1] - np.float32([[2.0], [0.5]]), m[-1:] + np.float32([[0.0], [1.0], [64.0]])])
    out, counts, _ = ref.qmap_apply(v, m, o, None, 0)
    np.testing.assert_array_equal(out, v - np.float32(3.0))
    assert counts['n_below'] == 2 * 8 and counts['n_above'] == 3 * 8


def test_multiplicative_ratio_beyond_the_ends():
    obs = np.abs(cases.field(50, 8, 10)) + np.float32(1.0)
    model = np.float32(2.0) * obs
    q = cases.probabilities(21)
    o, m = _tables(obs, model, q)
    np.testing.assert_array_equal(m, np.float32(2.0) * o)
    v = np.concatenate([m[:1] * np.float32([[0.5], [0.75]]), m[-1:] * np.float32([[1.0], [3.0]])])
    out, counts, _ = ref.qmap_apply(v, m, o, None, 1)
    np.testing.assert_array_equal(out, v / np.float32(2.0))             # o_t / m_t is exactly 0.5
    assert counts['n_below'] == 2 * 8 and counts['n_above'] == 2 * 8


def test_zero_maps_onto_the_highest_tied_knot():
    """a precipitation cell with 70 % zeros: knots 0 ... k of the model's table are all 0; a zero is located at k (rule 3), so it
    comes out as the observed knot k, not as the observed minimum"""
    r = np.random.default_rng(12)
    n = 200
    model = np.zeros((n, 1), np.float32)
    model[:60, 0] = np.round(r.gamma(0.6, 3.0, 60) + 0.1, 1)
    obs = np.zeros((n, 1), np.float32)
    obs[:100, 0] = np.round(r.gamma(0.6, 3.0, 100) + 0.1, 1)           # the observation is wet more often
    q = np.linspace(0, 1, 101)
    o, m = _tables(obs, model, q)
    k = int((m[:, 0] == 0).sum()) - 1
    assert 60 < k < 75 and m[k + 1, 0] > 0 and o[k, 0] > 0 and o[0, 0] == 0
    out, counts, taken = ref.qmap_apply(np.zeros((1, 1), np.float32), m, o, None, 1)
    assert out[0, 0] == o[k, 0] and taken['tied'].all() and counts['n_below'] == counts['n_above'] == 0


def test_qdm_with_the_model_table_as_target_agrees_with_eqm_at_the_ends():
    for kind in (0, 1):
        obs, model, _ = cases.history(kind, 30, 20 + kind)
        o, m = _tables(obs, model, cases.probabilities(31))
        v = cases.map_input(kind, 37, m, 21)
        eqm, ce, _ = ref.qmap_apply(v, m, o, None, kind)
        qdm, cq, _ = ref.qmap_apply(v, m, o, m, kind)
        assert ce == cq and ce['n_below'] > 0 and ce['n_above'] > 0
        with np.errstate(invalid='ignore'):
            end = (v < m[0]) | (v >= m[-1])
        np.testing.assert_array_equal(eqm[end].view(np.uint32), qdm[end].view(np.uint32))


def test_nonfinite_and_unfitted():
    obs, model, _ = cases.history(0, 6, 30)
    cases.spoil_cells(obs, model)
    o, m = _tables(obs, model, cases.probabilities(11))
    v = cases.temperature(np.random.default_rng(31), (5, 6))
    v[0, 0], v[1, 1], v[2, 3] = np.nan, np.inf, -np.inf
    out, counts, _ = ref.qmap_apply(v, m, o)
    assert counts['n_nonfinite'] == 3 and counts['n_unfitted'] == 2 * 5 - 1
    assert np.isnan(out[0, 0]) and out[1, 1] == np.inf and out[2, 3] == -np.inf
    assert np.isnan(out[[0, 2, 3, 4], 1]).all() and np.isnan(out[:, 2]).all() and np.isfinite(out[:, 4:]).all()
    kept, counts_kept, _ = ref.qmap_apply(v, m, o, keep_unfitted=True)
    assert counts_kept == counts
    np.testing.assert_array_equal(kept[:, 2], v[:, 2])


# ------------------------------------------------------------------------------------------------------------ the public object
def test_lazy_exports():
    import dl4ds_amd
    from dl4ds_amd import postprocessing
    for name in ('QuantileMapper', 'quantile_map', 'check_qmap_args'):
        assert getattr(dl4ds_amd, name) is getattr(postprocessing, name)
    from dl4ds_amd.preprocessing import NotFittedError
    assert issubclass(NotFittedError, ValueError)


def test_check_qmap_args_accepts():
    from dl4ds_amd.postprocessing import check_qmap_args
    np.testing.assert_array_equal(check_qmap_args(), np.linspace(0, 1, 101))
    q = check_qmap_args(quantiles=(0.1, 0.5, 0.9), method='qdm', kind='*', batch_size=3, obs_shape=(5, 2, 3, 1), model_shape=(9, 2, 3, 1))
    assert q.dtype == np.float64 and q.tolist() == [0.1, 0.5, 0.9]
    assert len(check_qmap_args(2)) == 2 and len(check_qmap_args(256)) == 256
    check_qmap_args(x_shape=(4, 2, 3, 1), grid=(2, 3, 1))


@pytest.mark.parametrize('kw, message', [
    (dict(method='cdf'), 'method'), (dict(kind='-'), 'kind'), (dict(kind=0), 'kind'),
    (dict(batch_size=0), 'batch_size'), (dict(batch_size=1.5), 'batch_size'),
    (dict(n_quantiles=1), 'between 2 and 256'), (dict(n_quantiles=257), 'between 2 and 256'), (dict(n_quantiles=10.0), 'integer'),
    (dict(n_quantiles=True), 'integer'),
    (dict(quantiles=(0.5,)), 'between 2 and 256'), (dict(quantiles=np.linspace(0, 1, 257)), 'between 2 and 256'),
    (dict(quantiles=((0.1, 0.2),)), '1-D'), (dict(quantiles=(0.1, 1.1)), r'\[0, 1\]'), (dict(quantiles=(-0.1, 0.5)), r'\[0, 1\]'),
    (dict(quantiles=(0.1, np.nan)), r'\[0, 1\]'), (dict(quantiles=(0.5, 0.5)), 'strictly increasing'),
    (dict(quantiles=(0.9, 0.1)), 'strictly increasing'),
    (dict(obs_shape=(5, 2, 3)), 'obs'), (dict(obs_shape=(0, 2, 3, 1)), 'obs'), (dict(model_shape=(5, 2, 3, 1, 1)), 'model'),
    (dict(obs_shape=(5, 2, 3, 1), model_shape=(5, 2, 4, 1)), 'share their grid'),
    (dict(obs_shape=(1 << 31, 1, 1, 1)), '2\\^31'),
    (dict(x_shape=(4, 2, 3)), '`x`'), (dict(x_shape=(4, 2, 3, 2), grid=(2, 3, 1)), 'fitted on')])
def test_check_qmap_args_refuses(kw, message):
    from dl4ds_amd.postprocessing import check_qmap_args
    with pytest.raises(ValueError, match=message):
        check_qmap_args(**kw)


def test_transform_and_save_before_fit():
    from dl4ds_amd.postprocessing import QuantileMapper, check_qmap_args
    from dl4ds_amd.preprocessing import NotFittedError
    with pytest.raises(NotFittedError):
        check_qmap_args(x_shape=(4, 2, 3, 1), fitted=False)
    with pytest.raises(NotFittedError):
        QuantileMapper().transform(np.zeros((4, 2, 3, 1), np.float32))
    with pytest.raises(NotFittedError):
        QuantileMapper().save('never_written')
    with pytest.raises(ValueError, match='method'):                     # the arguments come before the fitted state
        QuantileMapper(method='x').transform(np.zeros((4, 2, 3, 1), np.float32))
    with pytest.raises(ValueError, match='share their grid'):           # and before anything touches the device
        QuantileMapper().fit(np.zeros((4, 2, 3, 1), np.float32), np.zeros((4, 3, 3, 1), np.float32))


def test_save_load_round_trip(tmp_path):
    from dl4ds_amd.postprocessing import QuantileMapper
    obs, model = cases.spoiled(40, 24).reshape(40, 2, 4, 3), cases.field(33, 24, 9).reshape(33, 2, 4, 3)
    q = cases.probabilities(17)
    (o, n_o), (m, n_m) = ref.quantile_table(obs, q), ref.quantile_table(model, q)
    mapper = QuantileMapper.from_tables(q, o, m, n_o, n_m, method='qdm', kind='*', keep_unfitted=True)
    path = tmp_path / 'mapper.npz'
    mapper.save(path)
    back = QuantileMapper.load(path)
    assert (back.method, back.kind, back.keep_unfitted, back.batch_size) == ('qdm', '*', True, None)
    for name, dtype in (('quantiles_', np.float64), ('obs_quantiles_', np.float32), ('model_quantiles_', np.float32),
                        ('n_obs_', np.int64), ('n_model_', np.int64)):
        a, b = getattr(mapper, name), getattr(back, name)
        assert b.dtype == dtype and a.shape == b.shape
        np.testing.assert_array_equal(a.view(np.uint8), b.view(np.uint8))            # bit for bit, NaN included
    assert back.obs_quantiles_.shape == (17, 2, 4, 3) and back.n_obs_.shape == (2, 4, 3) and np.isnan(back.obs_quantiles_).any()
    with pytest.raises(ValueError, match='tables of shape'):
        QuantileMapper.from_tables(q, o[:-1], m, n_o, n_m)
