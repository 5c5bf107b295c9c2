"""Quantile-mapping bias correction on the device (dl4ds_quantile_table, dl4ds_qmap_apply, csrc/qmap.hip)
against the numpy restatement tests/qmap_ref.py (itself checked against np.quantile, np.interp and hand-worked answers in
tests/test_qmap_api.py).  Everything is compared bit for bit: tables and mapped values on their uint32 views (NaN included), the
valid counts and the four diagnostic counts as integers.  The map is checked on tables taken from the device, so a table that
passes its own test is what the map's expected values are built from."""
import functools

import numpy as np
import pytest

from tests import qmap_cases as cases
from tests import qmap_ref as ref
from tests.distribution_cases import STRIDED_MAX, TILE

pytestmark = pytest.mark.gpu


def assert_same_bits(got, want, what=''):
    assert got.dtype == want.dtype == np.float32 and got.shape == want.shape, (what, got.dtype, got.shape, want.shape)
    np.testing.assert_array_equal(got.view(np.uint32), want.view(np.uint32), err_msg=what)


def device_table(x, q, with_valid=True):
    """dl4ds_quantile_table on the (N, cells) host array -> (table (Q, cells), valid (cells,))"""
    from dl4ds_amd import _lib
    from dl4ds_amd.device import Buffers
    q = np.ascontiguousarray(q, np.float64)
    N, per = x.shape
    with Buffers() as buf:
        dx, dt, dv = buf.alloc(x.shape), buf.alloc((len(q), per)), buf.alloc((per,), np.int64)
        dx.upload(np.ascontiguousarray(x, np.float32))
        _lib.check(_lib.lib().dl4ds_quantile_table(dx.ptr, N, per, q.ctypes.data, len(q), dt.ptr, dv.ptr if with_valid else None))
        return dt.numpy(), dv.numpy() if with_valid else None


def check_table(x, q):
    table, valid = device_table(x, q)
    want, n = ref.quantile_table(x, q)
    assert valid.dtype == np.int64
    np.testing.assert_array_equal(valid, n)
    assert_same_bits(table, want)
    return table, valid


# ------------------------------------------------------------------------------------------------------------------- the table
@pytest.mark.parametrize('n, cells', [(n, c) for n in cases.TABLE_LENGTHS for c in cases.table_cells(n)])
def test_table_lengths_and_cells(n, cells):
    """both LDS paddings of every padded length, the engine switch at STRIDED_MAX, two radix tiles; one cell, a partial wave, one
    cell more than a workgroup takes"""
    assert (n <= STRIDED_MAX) == (n < 513) and (n <= TILE or n == TILE + 5)
    check_table(cases.field(n, cells, n + cells), np.linspace(0.0, 1.0, 11))


def test_table_in_chunks_of_cells():
    x = cases.workspace_chunks()
    table, _ = check_table(x, (0.05, 0.5, 0.95))
    assert np.isfinite(table).all()


@pytest.mark.parametrize('name', ['zeros70', 'signed_zeros', 'spoiled'])
def test_table_ties_zeros_and_nonfinite(name):
    x = getattr(cases, name)()
    table, valid = check_table(x, cases.probabilities(13))
    if name == 'spoiled':
        assert valid[3] == 0 and np.isnan(table[:, 3]).all() and valid[5] == 1 and (table[:, 5] == np.float32(1.25)).all()
        assert (valid < x.shape[0]).sum() > 10 and np.isfinite(np.delete(table, 3, axis=1)).all()
    if name == 'signed_zeros':
        assert (table == 0).any() and not np.signbit(table[table == 0]).any()


def test_table_spoiled_through_the_global_engine():
    x = cases.spoiled(STRIDED_MAX + 9, 70, seed=45)
    _, valid = check_table(x, cases.probabilities(5))
    assert valid[3] == 0 and valid[5] == 1


@pytest.mark.parametrize('q', [(0.0, 1.0), np.linspace(0.0, 1.0, 256), np.linspace(0.2, 0.7, 6), (0.0, 2.0 ** -60, 1.0 - 2.0 ** -53, 1.0)],
                         ids=['Q2', 'Q256', 'inside', 'next_to_the_ends'])
@pytest.mark.parametrize('n', [37, STRIDED_MAX + 30])
def test_table_probabilities(n, q):
    check_table(cases.field(n, 70, 7 * n), q)


def test_table_repeats_and_valid_may_be_null():
    x = cases.spoiled(STRIDED_MAX + 1, 66)
    q = cases.probabilities(9)
    first, _ = device_table(x, q)
    again, none = device_table(x, q, with_valid=False)
    assert none is None
    assert_same_bits(again, first)


# --------------------------------------------------------------------------------------------------------------------- the map
@functools.lru_cache(maxsize=None)
def map_case(kind, cells, Q, seed=0):
    """(x, m, o, f): tables from the device (each checked against the restatement), computed once and left unchanged"""
    obs, model, future = cases.history(kind, cells, 100 * kind + cells + Q + seed)
    cases.spoil_cells(obs, model)
    q = cases.probabilities(Q)
    o, m, f = (check_table(a, q)[0] for a in (obs, model, future))
    return o, m, f


def device_map(x, m, o, f, kind, keep_unfitted=False, in_place=False, with_counts=True):
    from dl4ds_amd import _lib
    from dl4ds_amd.device import Buffers
    B, per = x.shape
    Q = m.shape[0]
    with Buffers() as buf:
        dx, dout = buf.alloc(x.shape), buf.alloc(x.shape)
        dx.upload(x)
        dm, do, df = (buf.alloc(t.shape) if t is not None else None for t in (m, o, f))
        for d, t in ((dm, m), (do, o), (df, f)):
            if d is not None:
                d.upload(t)
        counts = buf.zeros((4,), np.uint64)
        out = dx if in_place else dout
        _lib.check(_lib.lib().dl4ds_qmap_apply(dx.ptr, out.ptr, B, per, dm.ptr, do.ptr, df.ptr if df is not None else None, Q, kind,
                                               int(keep_unfitted), counts.ptr if with_counts else None))
        return out.numpy(), dict(zip(ref.COUNT_NAMES, (int(v) for v in counts.numpy())))


def check_map(method, kind, cells, B, Q, **kw):
    o, m, f = map_case(kind, cells, Q)
    f = f if method == 'qdm' else None
    x = cases.map_input(kind, B, m if f is None else f, B + cells)
    want, counts, taken = ref.qmap_apply(x, m, o, f, kind, kw.get('keep_unfitted', False))
    got, got_counts = device_map(x, m, o, f, kind, **kw)
    assert got_counts == counts
    assert_same_bits(got, want, (method, kind, cells, B, Q))
    return counts, taken


@pytest.mark.parametrize('Q', [2, 101, 256])
@pytest.mark.parametrize('B', [1, 2, 37])
@pytest.mark.parametrize('cells', [1, 105, 64 * 3 + 1])
@pytest.mark.parametrize('kind', [0, 1], ids=['additive', 'multiplicative'])
@pytest.mark.parametrize('method', ['eqm', 'qdm'])
def test_map(method, kind, cells, B, Q):
    """one cell, partial workgroups, one cell more than three workgroups; one sample, fewer samples than a workgroup has waves,
    more than one round of its unrolled walk; Q = 256 with QDM does not fit the LDS staging of all three tables"""
    assert cases.max_staged_q(3) < 256 and cases.max_staged_q(2) >= 101
    check_map(method, kind, cells, B, Q)


@pytest.mark.parametrize('method, Q', [(m, cases.max_staged_q(t) + d) for m, t in (('eqm', 2), ('qdm', 3)) for d in (0, 1)])
def test_map_at_the_staging_threshold(method, Q):
    """the last Q whose tables are all staged in LDS and the first whose o / m rows come from global memory"""
    for kind in (0, 1):
        check_map(method, kind, 70, 9, Q)


@pytest.mark.parametrize('method', ['eqm', 'qdm'])
def test_every_branch_is_reached(method):
    """a case cannot pass by never reaching a branch: both ends, unfitted cells, non-finite values, values exactly on knots,
    tied knots and (multiplicative) a model quantile of 0 all occur, with and without keep_unfitted"""
    for kind in (0, 1):
        for keep in (False, True):
            counts, taken = check_map(method, kind, 105, 37, 101, keep_unfitted=keep)
            assert min(counts.values()) > 0, counts
            assert taken['interior'].sum() > 100 and taken['on_knot'].sum() > 50
            if kind == 1:
                assert taken['tied'].sum() > 50 and taken['model_zero'].sum() > 20


@pytest.mark.parametrize('method', ['eqm', 'qdm'])
def test_map_in_place_and_without_counts(method):
    for kind in (0, 1):
        check_map(method, kind, 105, 37, 101, in_place=True)
    o, m, f = map_case(0, 105, 101)
    x = cases.map_input(0, 37, m, 3)
    got, counts = device_map(x, m, o, f if method == 'qdm' else None, 0, with_counts=False)
    assert_same_bits(got, ref.qmap_apply(x, m, o, f if method == 'qdm' else None, 0)[0])
    assert set(counts.values()) == {0}


def test_map_splits_the_samples():
    """few cells and many samples: the samples are split over workgroups (blockIdx.y), the last share shorter than the others"""
    o, m, f = map_case(0, 70, 31)
    x = cases.map_input(0, 1001, m, 5)
    for tab in (None, f):
        want, counts, _ = ref.qmap_apply(x, m, o, tab, 0)
        got, got_counts = device_map(x, m, o, tab, 0)
        assert got_counts == counts
        assert_same_bits(got, want)


# ------------------------------------------------------------------------------------------------------------------ end to end
GRID = (6, 7, 2)


@functools.lru_cache(maxsize=None)
def end_to_end(method, kind):
    """(obs, model, x, q, expected out, expected counts, expected tables): N_o != N_m, computed once and left unchanged"""
    k = ('+', '*').index(kind)
    obs, model, x = (a.reshape((a.shape[0],) + GRID) for a in cases.history(k, 84, 7 + k, n_obs=40, n_model=53))
    obs[:, 0, 1, 0] = np.nan
    x = x[:37].copy()
    x[3, 2, 2, 1], x[5, 0, 0, 0] = np.nan, np.inf
    q = cases.probabilities(51)
    return (obs, model, x, q) + ref.quantile_mapper(obs, model, x, q, method, kind)


@pytest.mark.parametrize('kind', ['+', '*'])
@pytest.mark.parametrize('method', ['eqm', 'qdm'])
def test_mapper_from_host_arrays(method, kind):
    from dl4ds_amd.postprocessing import QuantileMapper, quantile_map
    obs, model, x, q, want, counts, (ot, mt, n_o, n_m) = end_to_end(method, kind)
    outs = []
    for batch_size in (None, 1, 3):
        mapper = QuantileMapper(quantiles=q, method=method, kind=kind, batch_size=batch_size).fit(obs, model)
        assert_same_bits(mapper.obs_quantiles_, ot)
        assert_same_bits(mapper.model_quantiles_, mt)
        for got, exp in ((mapper.n_obs_, n_o), (mapper.n_model_, n_m)):
            assert got.dtype == np.int64 and got.shape == GRID
            np.testing.assert_array_equal(got, exp)
        assert mapper.quantiles_.dtype == np.float64 and mapper.obs_quantiles_.shape == (len(q),) + GRID
        out = mapper.transform(x)
        assert mapper.diagnostics_ == counts and counts['n_unfitted'] == 37 and counts['n_nonfinite'] == 2
        assert_same_bits(out, want, batch_size)
        outs.append(out)
    for other in outs[1:]:
        assert_same_bits(other, outs[0], 'batch_size')
    assert_same_bits(quantile_map(obs, model, x.astype(np.float64), quantiles=q, method=method, kind=kind), want)


def test_mapper_on_device_arrays_and_3d_input():
    from dl4ds_amd.device import DeviceArray
    from dl4ds_amd.postprocessing import QuantileMapper
    obs, model, x, q, want, counts, _ = end_to_end('qdm', '+')
    d_obs, d_model, d_x = (DeviceArray.from_numpy(a) for a in (obs, model, x))
    mapper = QuantileMapper(quantiles=q, method='qdm').fit(d_obs, d_model)
    out = mapper.transform(d_x)
    assert isinstance(out, DeviceArray) and out.shape == x.shape
    assert_same_bits(out.numpy(), want)
    assert mapper.diagnostics_ == counts
    np.testing.assert_array_equal(d_x.numpy().view(np.uint32), x.view(np.uint32))            # the input is left as it was
    flat = QuantileMapper(quantiles=q, method='qdm').fit(obs[..., 0], model[..., 0]).transform(x[..., 0])
    assert flat.shape == x.shape[:3] + (1,)
    assert_same_bits(flat, ref.quantile_mapper(obs[..., 0], model[..., 0], x[..., 0], q, 'qdm', '+')[0])
    d3 = [DeviceArray.from_numpy(a[..., 0]) for a in (obs, model, x)]      # 3-D device arrays are read as (N, H, W, 1) and left 3-D
    out3 = QuantileMapper(quantiles=q, method='qdm').fit(d3[0], d3[1]).transform(d3[2])
    assert [d.shape for d in d3] == [a.shape[:3] for a in (obs, model, x)] and out3.shape == flat.shape
    assert_same_bits(out3.numpy(), flat)


def test_mapper_mask_and_keep_unfitted():
    from dl4ds_amd.postprocessing import QuantileMapper
    obs, model, x, q = end_to_end('eqm', '+')[:4]
    mask = np.ones(GRID[:2], np.float32)
    mask[2:4, 1:5] = 0
    want, counts, _ = ref.quantile_mapper(obs, model, x, q, 'eqm', '+', keep_unfitted=True, mask=mask)
    mapper = QuantileMapper(quantiles=q, keep_unfitted=True)
    out = mapper.fit(obs, model, mask=mask).transform(x)
    assert_same_bits(out, want)
    assert mapper.diagnostics_ == counts and counts['n_unfitted'] > 8 * 2 * 30 and (mapper.n_obs_[2:4, 1:5] == 0).all()


def test_fit_transform_twice():
    from dl4ds_amd.postprocessing import QuantileMapper
    obs, model, _, q = end_to_end('qdm', '*')[:4]
    mapper = QuantileMapper(quantiles=q, method='qdm', kind='*')
    first = mapper.fit_transform(obs, model)
    again = mapper.fit_transform(obs, model)
    assert_same_bits(again, first)
    assert_same_bits(first, ref.quantile_mapper(obs, model, model, q, 'qdm', '*')[0])


# ------------------------------------------------------------------------------------------------------------------ refusals
def test_abi_refusals():
    from dl4ds_amd import _lib
    from dl4ds_amd.device import Buffers
    lib = _lib.lib()
    good = np.linspace(0.0, 1.0, 5)

    def refused(status, word):
        assert status != 0
        message = lib.dl4ds_last_error().decode()
        assert word in message, message

    def probs(v):
        v = np.ascontiguousarray(v, np.float64)
        return v, v.ctypes.data

    with Buffers() as buf:
        x, table, out = buf.zeros((8, 6)), buf.alloc((256, 6)), buf.alloc((8, 6))

        def table_call(N=8, per=6, q=good, Q=None, xp=x.ptr, tp=table.ptr, null_q=False):
            keep, qp = probs(q)
            return lib.dl4ds_quantile_table(xp, N, per, None if null_q else qp, len(keep) if Q is None else Q, tp, None)
        assert table_call() == 0
        refused(table_call(q=(0.5,)), 'between 2 and 256')
        refused(table_call(q=np.linspace(0, 1, 257)), 'between 2 and 256')
        refused(table_call(q=(0.0, 1.5)), '[0, 1]')
        refused(table_call(q=(-0.5, 1.0)), '[0, 1]')
        refused(table_call(q=(0.0, np.nan)), '[0, 1]')
        refused(table_call(q=(0.5, 0.5)), 'strictly increasing')
        refused(table_call(q=(0.9, 0.1)), 'strictly increasing')
        refused(table_call(N=0), 'empty')
        refused(table_call(per=0), 'empty')
        refused(table_call(N=1 << 31), '2^31')
        refused(table_call(xp=None), 'null')
        refused(table_call(tp=None), 'null')
        refused(table_call(null_q=True), 'null')

        def map_call(B=8, per=6, Q=5, kind=0, xp=x.ptr, op=out.ptr, mp=table.ptr, obp=table.ptr):
            return lib.dl4ds_qmap_apply(xp, op, B, per, mp, obp, None, Q, kind, 0, None)
        _lib.check(lib.dl4ds_memset(table.ptr, 0, table.nbytes))
        assert map_call() == 0
        refused(map_call(Q=1), 'between 2 and 256')
        refused(map_call(Q=257), 'between 2 and 256')
        refused(map_call(kind=2), 'kind')
        refused(map_call(kind=-1), 'kind')
        refused(map_call(per=0), 'empty')
        for null in ('xp', 'op', 'mp', 'obp'):
            refused(map_call(**{null: None}), 'null')
