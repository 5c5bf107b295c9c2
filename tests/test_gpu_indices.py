"""Climate indices on the device (dl4ds_climate_indices, csrc/indices.hip) against the numpy restatement
tests/indices_ref.py (itself checked against itertools.groupby, a plain Python loop and hand-worked answers in
tests/test_indices_api.py).  Everything is compared bit for bit: the integers as integers, fp32 and fp64 on their unsigned views,
NaN included."""
import functools

import numpy as np
import pytest

from tests import indices_cases as cases
from tests import indices_ref as ref

pytestmark = pytest.mark.gpu

OUTPUTS = ('valid', 'event', 'ext', 'sums')


def assert_same(got, want, what=''):
    assert len(got) == len(want)
    for name, g, w in zip(OUTPUTS, got, want):
        if w is None:
            assert g is None, (what, name)
            continue
        assert g.dtype == w.dtype and g.shape == w.shape, (what, name, g.dtype, g.shape, w.shape)
        bits = {4: np.uint32, 8: np.uint64}[w.dtype.itemsize]
        np.testing.assert_array_equal(g.view(bits), w.view(bits), err_msg=f'{what} {name}')


def device_indices(x, st, thr, op=0, window=cases.WINDOW, want=(True, True, True, True)):
    """dl4ds_climate_indices on the (N, cells) host array -> (valid, event, ext, sums), None where the output pointer was null"""
    from dl4ds_amd import _lib
    from dl4ds_amd.device import Buffers
    N, per = x.shape
    st, thr = np.ascontiguousarray(st, np.int64), np.ascontiguousarray(thr, np.float32)
    P, T = len(st) - 1, thr.shape[0]
    shapes = (((P, per), np.int32), ((P, T, 6, per), np.int32), ((P, 2, per), np.float32), ((P, 2 + T, per), np.float64))
    with Buffers() as buf:
        dx, dthr = buf.alloc(x.shape), buf.alloc(thr.shape)
        dx.upload(np.ascontiguousarray(x, np.float32))
        dthr.upload(thr)
        devs = [buf.alloc(s, d) if w else None for (s, d), w in zip(shapes, want)]
        for d in devs:                                          # every output is overwritten: start from a pattern
            if d is not None:
                _lib.check(_lib.lib().dl4ds_memset(d.ptr, 0x5a, d.nbytes))
        _lib.check(_lib.lib().dl4ds_climate_indices(dx.ptr, N, per, st.ctypes.data, P, dthr.ptr, T, int(thr.ndim == 2), op, window,
                                                    *(d.ptr if d is not None else None for d in devs)))
        return tuple(d.numpy() if d is not None else None for d in devs)


@functools.lru_cache(maxsize=None)
def expected(maker, n, cells, kind, T, op, window, per_cell, seed=0):
    """(x, starts, thr, the restatement's four outputs): computed once and left unchanged"""
    x = getattr(cases, maker)(n, cells, seed)
    st = cases.starts(n, kind)
    thr = cases.cell_thresholds(T, cells, seed) if per_cell else np.asarray(cases.SCALARS[:T], np.float32)
    return x, st, thr, ref.climate_indices(x, st, thr, op, window)


def check(maker, n, cells, kind, T, op, window=cases.WINDOW, per_cell=False, seed=0):
    x, st, thr, want = expected(maker, n, cells, kind, T, op, window, per_cell, seed)
    assert_same(device_indices(x, st, thr, op, window), want, (maker, n, cells, kind, T, op, window, per_cell))
    return x, st, thr, want


@pytest.mark.parametrize('n', cases.LENGTHS)
@pytest.mark.parametrize('cells', cases.CELLS)
def test_sizes(cells, n):
    """one cell, a partial wave, a whole one, one lane more, one cell more than a workgroup takes; one and two samples, the window
    and the load block +- 1, many blocks; one period, three uneven ones with a one-sample period, every sample a period; T = 1..4,
    every op, scalar and per-cell thresholds with a NaN threshold in one cell of one t"""
    assert cells <= cases.GROUP + 1 and n in (1, 2, 4, 5, 6, 7, 9, 97) and cases.DEPTH == 8 and cases.WINDOW == 5
    for k, kind in enumerate(cases.PERIOD_KINDS):
        for T in (1, 2, 3, 4):
            check('spoiled', n, cells, kind, T, (T + k) % 4, per_cell=(T + k) % 2 == 1, seed=n + cells)


@pytest.mark.parametrize('op', [0, 1, 2, 3])
@pytest.mark.parametrize('T', [1, 2, 3, 4])
def test_every_op_and_threshold_count(T, op):
    for per_cell in (False, True):
        check('spoiled', 97, 65, 'uneven', T, op, per_cell=per_cell)
        check('temperatures', 41, 70, 'uneven', T, op, per_cell=per_cell)


def test_the_case_reaches_the_walks_branches():
    """a case cannot pass by never reaching a branch: an event run longer than one load block, a window that spans two load
    blocks, NaN and +-inf, an all-NaN cell, runs from the first sample and up to the last, a run cut by a period boundary"""
    x, st, thr, (valid, event, ext, sums) = check('spoiled', 97, 65, 'uneven', 3, 0)
    longest, spans, has_nan, has_inf = cases.reaches(x, st, cases.WINDOW)
    assert longest > cases.DEPTH and spans and has_nan and has_inf
    assert event[:, 0, 1].max() > cases.DEPTH                                   # an event run longer than a load block
    assert (valid[:, 3] == 0).all() and np.isnan(ext[:, :, 3]).all() and np.isnan(sums[:, :2, 3]).all()
    lens = np.diff(st)
    assert (event[:, 0, 1, 0] == lens).all() and (event[:, 0, 4, 0] == 0).all() and (event[:, 0, 5, 0] == lens - 1).all()
    assert event[0, 0, 4, 7] == 1 and (event[:, 0, 5, 7] == lens - 1).all()       # after an invalid first sample, up to the last
    whole = ref.climate_indices(x, cases.starts(97, 'one'), thr, 0, cases.WINDOW)[1]
    assert whole[0, 0, 1, 0] == 97 > event[:, 0, 1, 0].max()                     # the run across the boundaries is cut
    assert (valid[:, 5].sum() == 1) and np.signbit(x).any() and not np.signbit(ext[np.isfinite(ext) & (ext == 0)]).any()


@pytest.mark.parametrize('window', [1, 2, 31, 32])
def test_windows(window):
    for n in (window - 1, window, window + 1, 70):
        if n >= 1:
            _, _, _, (_, _, _, sums) = check('spoiled', n, 65, 'one', 1, 0, window=window, seed=window)
            assert np.isfinite(sums[:, 1]).any() == (n >= window)
    check('spoiled', 70, 65, 'uneven', 2, 0, window=window, seed=window)


def test_repeated_and_unordered_thresholds_and_signed_zeros():
    x = cases.spoiled(40, 70, seed=3)
    st = cases.starts(40, 'uneven')
    thr = np.array([10.0, 1.0, 10.0, 0.5], np.float32)
    got = device_indices(x, st, thr)
    assert_same(got, ref.climate_indices(x, st, thr, 0, cases.WINDOW))
    np.testing.assert_array_equal(got[1][:, 0], got[1][:, 2])
    z = np.where(np.arange(30)[:, None] % 3 == 0, np.float32(-0.0), np.float32(0.0)) * np.ones((1, 66), np.float32)
    for op in range(4):
        for t0 in (0.0, -0.0):
            got = device_indices(z, cases.starts(30, 'uneven'), np.array([t0], np.float32), op, 2)
            assert_same(got, ref.climate_indices(z, cases.starts(30, 'uneven'), np.array([t0], np.float32), op, 2))
            assert not np.signbit(got[2]).any() and not np.signbit(got[3]).any()


def test_each_output_may_be_null_and_a_repeated_call_gives_the_same_bits():
    x, st, thr, want = expected('spoiled', 97, 65, 'uneven', 3, 0, cases.WINDOW, True)
    first = device_indices(x, st, thr)
    assert_same(first, want)
    assert_same(device_indices(x, st, thr), first, 'repeat')
    for k in range(4):
        keep = tuple(j != k for j in range(4))
        assert_same(device_indices(x, st, thr, want=keep), tuple(w if j != k else None for j, w in enumerate(want)), f'null {k}')
        only = tuple(j == k for j in range(4))
        assert_same(device_indices(x, st, thr, want=only), tuple(w if j == k else None for j, w in enumerate(want)), f'only {k}')


# ---------------------------------------------------------------------------------------------------------------- the host layer
GRID = (6, 7, 2)


@functools.lru_cache(maxsize=None)
def host_case():
    x = cases.spoiled(60, 84, seed=9).reshape((60,) + GRID)
    years = np.repeat([2001, 2002, 2004], [25, 1, 34])
    thr = cases.cell_thresholds(2, 84, seed=9).reshape((2,) + GRID)
    return x, years, thr


def assert_named(got, want):
    assert set(got) == set(want)
    for name, w in want.items():
        g = got[name]
        assert g.dtype == w.dtype and g.shape == w.shape, (name, g.dtype, g.shape, w.shape)
        np.testing.assert_array_equal(g.view({4: np.uint32, 8: np.uint64}[w.dtype.itemsize]) if w.dtype.kind == 'f' else g,
                                      w.view({4: np.uint32, 8: np.uint64}[w.dtype.itemsize]) if w.dtype.kind == 'f' else w, err_msg=name)


def test_climate_indices_from_host_arrays():
    from dl4ds_amd.indices import climate_indices, period_starts_from_labels
    x, years, thr = host_case()
    st = period_starts_from_labels(years)
    for thresholds, op in (((1.0, 10.0, 20.0), '>='), (thr, '<')):
        want = ref.named(x, st, thresholds, ('>=', '>', '<', '<=').index(op), 4)
        for batch_size in (None, 1, 3):
            assert_named(climate_indices(x, years, thresholds, op, 4, batch_size=batch_size), want)
        assert_named(climate_indices(x.astype(np.float64), period_starts=list(st), thresholds=thresholds, op=op, window=4), want)
    assert want['n_event'].shape == (3, 2) + GRID and want['sum'].shape == (3,) + GRID


def test_climate_indices_on_a_device_array_3d_input_and_mask():
    from dl4ds_amd.device import DeviceArray
    from dl4ds_amd.indices import climate_indices
    x, years, thr = host_case()
    st = cases.starts(60, 'uneven')
    d_x = DeviceArray.from_numpy(x)
    assert_named(climate_indices(d_x, period_starts=st, thresholds=thr, window=3), ref.named(x, st, thr, 0, 3))
    np.testing.assert_array_equal(d_x.numpy().view(np.uint32), x.view(np.uint32))            # the input is left as it was
    flat = climate_indices(x[..., 0], years)
    assert flat['sum'].shape == (3,) + GRID[:2] + (1,)
    assert_named(flat, ref.named(x[..., :1], [0, 25, 26, 60], (1.0,), 0, 5))
    d3 = DeviceArray.from_numpy(x[..., 0])
    assert_named(climate_indices(d3, years), flat)
    mask = np.ones(GRID[:2], np.float32)
    mask[2:4, 1:5] = 0
    masked = x.copy()
    masked[:, 2:4, 1:5] = np.nan
    got = climate_indices(x, years, mask=mask, batch_size=4)
    assert_named(got, ref.named(masked, [0, 25, 26, 60], (1.0,), 0, 5))
    assert (got['n_valid'][:, 2:4, 1:5] == 0).all() and np.isfinite(x[:, 2, 2, 0]).any()
    with pytest.raises(ValueError):
        climate_indices(d_x, mask=mask)


def test_precipitation_and_temperature_indices_end_to_end():
    from dl4ds_amd.indices import climate_indices, index_scores, percentile_threshold, precipitation_indices, temperature_indices
    from tests import qmap_ref
    x, years, _ = host_case()
    r = ref.named(x, [0, 25, 26, 60], (1.0, 10.0, 20.0), 0, 5)
    got = precipitation_indices(x, years)
    assert set(got) == {'rx1day', 'rx5day', 'prcptot', 'sdii', 'r1mm', 'r10mm', 'r20mm', 'cwd', 'cdd', 'n_valid', 'period_starts'}
    for name, want in (('rx1day', r['max']), ('rx5day', r['max_window_sum']), ('prcptot', r['sum']), ('r1mm', r['n_event'][:, 0]),
                       ('r10mm', r['n_event'][:, 1]), ('r20mm', r['n_event'][:, 2]), ('cwd', r['longest_event_run'][:, 0]),
                       ('cdd', r['longest_nonevent_run'][:, 0])):
        assert_named({name: got[name]}, {name: want})
    wet = r['n_event'][:, 0]
    with np.errstate(invalid='ignore', divide='ignore'):
        sdii = np.where(wet > 0, r['event_sum'][:, 0] / wet, np.nan)
    assert_named({'sdii': got['sdii']}, {'sdii': sdii})
    assert np.isnan(sdii).any() and np.isfinite(sdii).any()
    t = cases.temperatures(60, 84, seed=2).reshape((60,) + GRID)
    lo, hi = ref.named(t, [0, 25, 26, 60], (0.0,), 2, 1), ref.named(t, [0, 25, 26, 60], (25.0,), 1, 1)
    got = temperature_indices(t, years)
    for name, want in (('txx', lo['max']), ('tnn', lo['min']), ('days_below', lo['n_event'][:, 0]), ('days_above', hi['n_event'][:, 0]),
                       ('longest_run_below', lo['longest_event_run'][:, 0]), ('longest_run_above', hi['longest_event_run'][:, 0])):
        assert_named({name: got[name]}, {name: want})
    assert got['days_below'].max() > 0 and got['days_above'].max() > 0
    # R95pTOT: the amount above the 95th wet-day percentile, per cell
    p95 = percentile_threshold(x, 95, wet=1.0)
    wet_days = np.where(np.isfinite(x) & (x >= 1.0), x, np.float32(np.nan)).reshape(60, -1)
    assert_named({'p95': p95}, {'p95': qmap_ref.quantile_table(wet_days, (0.95, 1.0))[0][:1].reshape((1,) + GRID)})
    assert np.isnan(p95[0, 0, 1, 1]) and np.isfinite(p95).sum() > 70                                # cell 3 is all NaN
    assert_named(climate_indices(x, years, p95, '>'), ref.named(x, [0, 25, 26, 60], p95, 1, 5))
    scores = index_scores(x, x + np.float32(1), 'precipitation', period_starts=[0, 25, 26, 60])
    np.testing.assert_array_equal(scores['r1mm']['bias'], scores['r1mm']['pred'] - scores['r1mm']['obs'])
    assert scores['prcptot']['mean_bias'].shape == GRID and (scores['r1mm']['bias'] >= 0).all()


# ------------------------------------------------------------------------------------------------------------------ refusals
def test_abi_refusals():
    from dl4ds_amd import _lib
    from dl4ds_amd.device import Buffers
    lib = _lib.lib()

    def refused(status, word):
        assert status != 0
        message = lib.dl4ds_last_error().decode()
        assert word in message, message

    with Buffers() as buf:
        x, thr = buf.zeros((8, 6)), buf.zeros((4,))
        valid, event, ext, sums = buf.alloc((8, 6), np.int32), buf.alloc((8, 4, 6, 6), np.int32), buf.alloc((8, 2, 6)), \
            buf.alloc((8, 6, 6), np.float64)

        def call(N=8, per=6, st=(0, 3, 8), P=None, T=2, op=0, window=5, xp=x.ptr, tp=thr.ptr, null_starts=False,
                 outs=(valid.ptr, event.ptr, ext.ptr, sums.ptr)):
            keep = np.ascontiguousarray(st, np.int64)
            return lib.dl4ds_climate_indices(xp, N, per, None if null_starts else keep.ctypes.data, len(keep) - 1 if P is None else P,
                                             tp, T, 0, op, window, *outs)
        assert call() == 0
        assert call(st=np.arange(9)) == 0
        refused(call(P=0), 'at least one period')
        refused(call(P=-1), 'at least one period')
        refused(call(st=(1, 3, 8)), 'strictly increasing')
        refused(call(st=(0, 3, 7)), 'strictly increasing')
        refused(call(st=(0, 3, 9)), 'strictly increasing')
        refused(call(st=(0, 3, 3, 8)), 'strictly increasing')
        refused(call(st=(0, 5, 3, 8)), 'strictly increasing')
        refused(call(st=np.arange(10), N=8), 'strictly increasing')
        refused(call(N=0, st=(0, 0)), 'empty')
        refused(call(per=0), 'empty')
        refused(call(N=1 << 31, st=(0, 1 << 31)), '2^31')
        refused(call(T=0), 'thresholds')
        refused(call(T=5), 'thresholds')
        refused(call(window=0), 'window')
        refused(call(window=33), 'window')
        refused(call(op=-1), 'op must be')
        refused(call(op=4), 'op must be')
        refused(call(xp=None), 'null')
        refused(call(tp=None), 'null')
        refused(call(null_starts=True), 'null')
        refused(call(outs=(None, None, None, None)), 'all four outputs')
