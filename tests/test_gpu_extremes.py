"""Extreme-value verification on the device (dl4ds_lmoments, dl4ds_pot_peaks, csrc/extremes.hip) against the
restatement tests/extremes_ref.py (itself checked against scipy, plain Python and hand-written series in
tests/test_extremes_api.py).  Everything is compared bit for bit: the integers as integers, fp32 and fp64 on their unsigned views,
NaN positions included."""
import functools

import numpy as np
import pytest

from tests import extremes_cases as cases
from tests import extremes_ref as ref

pytestmark = pytest.mark.gpu


def assert_bits(got, want, what=''):
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, want.dtype, got.shape, want.shape)
    if want.dtype.kind == 'f':
        bits = {4: np.uint32, 8: np.uint64}[want.dtype.itemsize]
        np.testing.assert_array_equal(np.isnan(got), np.isnan(want), err_msg=f'{what}: NaN positions')
        keep = ~np.isnan(want)
        np.testing.assert_array_equal(got.view(bits)[keep], want.view(bits)[keep], err_msg=str(what))
    else:
        np.testing.assert_array_equal(got, want, err_msg=str(what))


def assert_all(got, want, what=''):
    assert len(got) == len(want)
    for k, (g, w) in enumerate(zip(got, want)):
        if w is None:
            assert g is None
        else:
            assert_bits(g, w, (what, k))


# -------------------------------------------------------------------------------------------------------------- dl4ds_lmoments
def device_lmoments(buffer, N, per, stride=None, sign=1, want=(True, True)):
    """dl4ds_lmoments on the host array `buffer` (N samples at `stride` floats) -> (valid, pwm), None where the pointer was null"""
    from dl4ds_amd import _lib
    from dl4ds_amd.device import Buffers
    with Buffers() as buf:
        dx = buf.alloc(buffer.shape)
        dx.upload(np.ascontiguousarray(buffer, np.float32))
        devs = [buf.alloc((per,), np.int32) if want[0] else None, buf.alloc((4, per), np.float64) if want[1] else None]
        for d in devs:                                          # every output is overwritten: start from a pattern
            if d is not None:
                _lib.check(_lib.lib().dl4ds_memset(d.ptr, 0x5a, d.nbytes))
        _lib.check(_lib.lib().dl4ds_lmoments(dx.ptr, N, per, per if stride is None else stride, sign,
                                             *(d.ptr if d is not None else None for d in devs)))
        return tuple(d.numpy() if d is not None else None for d in devs)


@functools.lru_cache(maxsize=None)
def lm_expected(n, cells, pattern, sign):
    x = cases.sample(n, cells, pattern)
    return x, ref.pwm(x, sign)


@pytest.mark.parametrize('n', cases.LM_LENGTHS)
@pytest.mark.parametrize('cells', cases.LM_CELLS)
def test_lmoments_sizes(cells, n):
    """fewer samples than moments, the bitonic rows up to their longest segment, the radix sort from one sample more; one cell, a
    partial wave, one lane more, several workgroups; both signs, every pattern, and the same samples interleaved with a sentinel
    row that a read at stride 2 * per must skip"""
    assert cases.LDS_MAX in cases.LM_LENGTHS and cases.LDS_MAX + 1 in cases.LM_LENGTHS
    for k, pattern in enumerate(('spoiled', 'ties', 'wide')):
        for sign in (1, -1):
            x, want = lm_expected(n, cells, pattern, sign)
            if (k + (sign > 0)) % 2:
                got = device_lmoments(x, n, cells, None, sign)
            else:
                got = device_lmoments(cases.interleave(x), n, cells, 2 * cells, sign)
            assert_all(got, want, (pattern, n, cells, sign))


def test_lmoments_case_contents_and_stride_both_ways():
    x, (n, pwm) = lm_expected(37, 65, 'spoiled', 1)
    assert n[0] == 0 and n[1] == 37 and n[2] == 1 and np.isnan(x).any() and np.isinf(x).any()
    assert np.isnan(pwm[:, 0]).all() and np.isnan(pwm[1:, 2]).all() and pwm[0, 2] == -1.5
    assert pwm[0, 1] == 3.25 and abs(2.0 * pwm[1, 1] - pwm[0, 1]) < 1e-13                # the constant cell: l2 = 0 up to rounding
    t = cases.sample(37, 65, 'ties')
    assert np.signbit(t[t == 0]).any() and not np.signbit(t[t == 0]).all() and len(np.unique(t[np.isfinite(t)])) <= 6
    w = np.abs(cases.sample(37, 65, 'wide'))
    assert w.min() < 1e-25 and w.max() > 1e25
    for sign in (1, -1):
        for pattern in ('spoiled', 'ties', 'wide'):
            x, want = lm_expected(37, 65, pattern, sign)
            assert_all(device_lmoments(x, 37, 65, None, sign), want)
            assert_all(device_lmoments(cases.interleave(x), 37, 65, 130, sign), want)
    # the sentinel is a valid sample: where it is read the answer changes
    x, want = lm_expected(37, 65, 'wide', 1)
    both = cases.interleave(x).reshape(74, 65)
    assert not np.array_equal(device_lmoments(both, 74, 65)[1][0], want[1][0])


@pytest.mark.parametrize('n', [37, cases.LDS_MAX + 1])
def test_lmoments_null_outputs_and_repeat(n):
    x, want = lm_expected(n, 65, 'spoiled', 1)
    first = device_lmoments(x, n, 65)
    assert_all(first, want)
    assert_all(device_lmoments(x, n, 65), first, 'repeat')
    assert_all(device_lmoments(x, n, 65, want=(True, False)), (want[0], None))
    assert_all(device_lmoments(x, n, 65, want=(False, True)), (None, want[1]))


def test_lmoments_engines_agree_at_the_seam():
    """the same 512 values, once sorted in LDS and once, with a NaN sample appended, by the radix sort: the same bits"""
    x, want = lm_expected(cases.LDS_MAX, 65, 'wide', 1)
    longer = np.concatenate([x, np.full((1, 65), np.nan, np.float32)])
    assert_all(device_lmoments(longer, cases.LDS_MAX + 1, 65), want)
    assert_all(device_lmoments(x, cases.LDS_MAX, 65), want)


def test_lmoments_and_quantile_table_read_the_same_sorted_rows():
    """dl4ds_lmoments and dl4ds_quantile_table are the two clients of one per-cell engine (csrc/cell_sort.h): on one array with
    NaN, +-inf and +-0.0 sprinkled in, each side of every step of the row-length ladder and of the LDS / radix seam, with one cell,
    a ragged 64-cell tile and a ragged last group, every cell has the same valid count from both, the table at q = (0, 1) is its
    smallest and largest valid value (tests/qmap_ref.py) and pwm[0] is tests/extremes_ref.py's, bit for bit; sign -1 against -x"""
    from tests import qmap_ref
    from tests.test_gpu_qmap import device_table
    rng = np.random.default_rng(26)
    full = (4.0 * rng.standard_normal((513, 257))).astype(np.float32)
    for value, share in ((np.nan, 0.05), (np.inf, 0.02), (-np.inf, 0.02), (0.0, 0.03), (-0.0, 0.03)):
        full[rng.random(full.shape) < share] = value
    full[:, 0] = np.nan                                                  # a cell without a valid sample
    q = np.array([0.0, 1.0])
    for n, group in ((1, 128), (64, 128), (65, 64), (512, 32), (513, 64)):               # G of the row length; the gather's tile
        for cells in (1, 65, 2 * group + 1):
            x = np.ascontiguousarray(full[:n, :cells])
            for sign in (1, -1):
                valid, pwm = device_lmoments(x, n, cells, None, sign)
                signed = x if sign > 0 else -x
                table, valid_q = device_table(signed, q)
                np.testing.assert_array_equal(valid_q, valid.astype(np.int64), err_msg=str((n, cells, sign)))
                want_table, want_n = qmap_ref.quantile_table(signed, q)
                np.testing.assert_array_equal(valid_q, want_n)
                assert_bits(table, want_table, ('table', n, cells, sign))
                assert_bits(pwm[0], ref.pwm(x, sign)[1][0], ('pwm[0]', n, cells, sign))


# -------------------------------------------------------------------------------------------------------------- dl4ds_pot_peaks
def device_pot(x, st, thr, sign=1, run=1, K=0, want=(True, True), then_lmoments=False):
    """dl4ds_pot_peaks on the (N, cells) host array -> (count, peak, pos), None where the pointer was null; with then_lmoments the
    (valid, pwm) of dl4ds_lmoments on the device's peak buffer as well"""
    from dl4ds_amd import _lib
    from dl4ds_amd.device import Buffers
    lib = _lib.lib()
    N, per = x.shape
    st, thr = np.ascontiguousarray(st, np.int64), np.ascontiguousarray(thr, np.float32).reshape(-1)
    with Buffers() as buf:
        dx, dthr = buf.alloc(x.shape), buf.alloc(thr.shape)
        dx.upload(np.ascontiguousarray(x, np.float32))
        dthr.upload(thr)
        devs = [buf.alloc((per,), np.int32), buf.alloc((K, per)) if K and want[0] else None,
                buf.alloc((K, per), np.int32) if K and want[1] else None]
        for d in devs:
            if d is not None:
                _lib.check(lib.dl4ds_memset(d.ptr, 0x5a, d.nbytes))
        _lib.check(lib.dl4ds_pot_peaks(dx.ptr, N, per, st.ctypes.data, len(st) - 1, dthr.ptr, int(thr.size > 1),
                                       sign, run, K, *(d.ptr if d is not None else None for d in devs)))
        out = tuple(d.numpy() if d is not None else None for d in devs)
        if then_lmoments:
            dv, dp = buf.alloc((per,), np.int32), buf.alloc((4, per), np.float64)
            _lib.check(lib.dl4ds_lmoments(devs[1].ptr, K, per, per, sign, dv.ptr, dp.ptr))
            out += (dv.numpy(), dp.numpy())
        return out


@functools.lru_cache(maxsize=None)
def pot_expected(n, cells, P, per_cell, sign, run, seed=0):
    """(x, starts, thr, the restatement's full result): computed once and left unchanged"""
    x = cases.series(n, cells, seed)
    st = cases.starts(n, P)
    thr = cases.cell_threshold(cells, seed) if per_cell else np.array([10.0], np.float32)
    return x, st, thr, ref.pot_peaks(x, st, thr, sign, run)


def cut(full, K):
    """the restatement's result at K rows: the first K peaks, NaN / -1 rows beyond the largest count"""
    count, peak, pos = full
    per = count.shape[0]
    pk, ps = np.full((K, per), np.nan, np.float32), np.full((K, per), -1, np.int32)
    k = min(K, peak.shape[0])
    pk[:k], ps[:k] = peak[:k], pos[:k]
    return count, pk, ps


@pytest.mark.parametrize('n', cases.POT_LENGTHS)
@pytest.mark.parametrize('cells', cases.POT_CELLS)
def test_pot_sizes(cells, n):
    """one sample, fewer than a load block, several; one cell, one lane more than a wave, several workgroups; one period and three
    with a one-sample period; every run length; scalar and per-cell thresholds with a NaN threshold; both signs; K = 0, one row
    more than the largest count (the padding) and, where there are two peaks, one row fewer"""
    for i, run in enumerate(cases.POT_RUNS):
        for j, P in enumerate((1, 3)):
            per_cell, sign = (i + j) % 2 == 1 and cells > 1, 1 if (i + 2 * j) % 3 else -1
            x, st, thr, full = pot_expected(n, cells, P, per_cell, sign, run)
            what = (n, cells, P, per_cell, sign, run)
            kmax = full[1].shape[0]
            assert_all(device_pot(x, st, thr, sign, run, 0), (full[0], None, None), what)
            assert_all(device_pot(x, st, thr, sign, run, kmax + 1), cut(full, kmax + 1), what)
            if kmax >= 2:
                assert_all(device_pot(x, st, thr, sign, run, kmax - 1), cut(full, kmax - 1), what)


def test_pot_case_contents_truncation_and_null_outputs():
    x, st, thr, full = pot_expected(365, 65, 3, True, 1, 2)
    count, peak, pos = full
    kmax = peak.shape[0]
    assert count[1] == -1 and count[3] == 0 and count[0] == 3 and kmax > 8            # NaN threshold; all-NaN cell; cut at boundaries
    assert np.isnan(x).any() and np.isinf(x).any() and np.signbit(x[x == 0]).any()
    assert pos[0, 0] == 2 and peak[0, 0] == 12.0                                        # ties at the peak: the first position
    one = pot_expected(365, 65, 1, True, 1, 2)[3][0]
    assert one[0] == 1 and (one[count >= 0] <= count[count >= 0]).all() and (one < count).any()
    assert (pot_expected(365, 65, 3, True, 1, 32)[3][0][count >= 0] <= count[count >= 0]).all()
    got = device_pot(x, st, thr, 1, 2, kmax)
    assert_all(got, full)
    assert_all(device_pot(x, st, thr, 1, 2, kmax), got, 'repeat')
    small = device_pot(x, st, thr, 1, 2, 3)
    assert_all(small, cut(full, 3))
    assert (small[0] > 3).any()                                                        # the count stays true beyond K
    assert_all(device_pot(x, st, thr, 1, 2, kmax, want=(True, False)), (count, peak, None))
    assert_all(device_pot(x, st, thr, 1, 2, kmax, want=(False, True)), (count, None, pos))


@pytest.mark.parametrize('sign', [1, -1])
def test_peaks_feed_lmoments_in_place(sign):
    x, st, thr, full = pot_expected(365, 300, 3, True, sign, 2)
    K = full[1].shape[0]
    got = device_pot(x, st, thr, sign, 2, K, then_lmoments=True)
    assert_all(got[:3], full)
    want = ref.pwm(full[1], sign)
    assert_all(got[3:], want)
    assert (want[0] == np.maximum(full[0], 0)).all() and want[0].max() == K


# ------------------------------------------------------------------------------------------------------------------ refusals
def test_abi_refusals_leave_the_outputs_untouched():
    from dl4ds_amd import _lib
    from dl4ds_amd.device import Buffers
    lib = _lib.lib()

    with Buffers() as buf:
        x, thr = buf.zeros((8, 12)), buf.zeros((6,))
        outs = [buf.alloc((6,), np.int32), buf.alloc((4, 6), np.float64), buf.alloc((6,), np.int32), buf.alloc((3, 6)),
                buf.alloc((3, 6), np.int32)]
        valid, pwm, count, peak, pos = outs
        for d in outs:
            _lib.check(lib.dl4ds_memset(d.ptr, 0x5a, d.nbytes))
        before = [d.numpy() for d in outs]

        def refused(status, word):
            assert status != 0
            message = lib.dl4ds_last_error().decode()
            assert word in message, message
            for d, b in zip(outs, before):
                np.testing.assert_array_equal(d.numpy().view(np.uint8), b.view(np.uint8))

        def lm(N=8, per=6, stride=12, sign=1, xp=x.ptr, vp=valid.ptr, pp=pwm.ptr):
            return lib.dl4ds_lmoments(xp, N, per, stride, sign, vp, pp)
        refused(lm(N=0), 'empty')
        refused(lm(per=0), 'empty')
        refused(lm(N=1 << 31), '2^31')
        refused(lm(stride=5), 'stride')
        refused(lm(sign=0), 'sign')
        refused(lm(sign=2), 'sign')
        refused(lm(xp=None), 'null')
        refused(lm(vp=None, pp=None), 'both outputs')

        def pot(N=8, per=6, st=(0, 3, 8), P=None, per_cell=0, sign=1, run=1, K=3, xp=x.ptr, tp=thr.ptr, null_starts=False,
                o=(count.ptr, peak.ptr, pos.ptr)):
            keep = np.ascontiguousarray(st, np.int64)
            return lib.dl4ds_pot_peaks(xp, N, per, None if null_starts else keep.ctypes.data, len(keep) - 1 if P is None else P, tp,
                                       per_cell, sign, run, K, *o)
        refused(pot(P=0), 'at least one period')
        refused(pot(st=(1, 3, 8)), 'strictly increasing')
        refused(pot(st=(0, 3, 7)), 'strictly increasing')
        refused(pot(st=(0, 3, 3, 8)), 'strictly increasing')
        refused(pot(st=np.arange(10)), 'strictly increasing')
        refused(pot(N=0, st=(0, 0)), 'empty')
        refused(pot(per=0), 'empty')
        refused(pot(N=1 << 31, st=(0, 1 << 31)), '2^31')
        refused(pot(sign=0), 'sign')
        refused(pot(run=0), 'run')
        refused(pot(run=33), 'run')
        refused(pot(K=-1), 'K')
        refused(pot(o=(count.ptr, None, None)), 'both')
        refused(pot(o=(None, peak.ptr, pos.ptr)), 'null')
        refused(pot(xp=None), 'null')
        refused(pot(tp=None), 'null')
        refused(pot(null_starts=True), 'null')
        # and the same requests go through once they are right
        assert lm() == 0 and lm(vp=None) == 0 and lm(pp=None) == 0 and lm(stride=6) == 0
        assert pot() == 0 and pot(K=0, o=(count.ptr, None, None)) == 0 and pot(per_cell=1, run=32, sign=-1) == 0


# ---------------------------------------------------------------------------------------------------------------- the host layer
SHAPE = (40, 9, 11, 2)
STARTS = np.arange(0, 41, 5, dtype=np.int64)                                            # 8 periods
BATCHES = (None, 1, 4)


@functools.lru_cache(maxsize=None)
def host_case():
    per = SHAPE[1] * SHAPE[2] * SHAPE[3]
    obs = cases.series(40, per, seed=5).reshape(SHAPE)
    pred = cases.series(40, per, seed=6).reshape(SHAPE)
    thr = cases.cell_threshold(per, seed=5).reshape(SHAPE[1:])
    return obs, pred, thr


def assert_dict(got, want, what=''):
    assert set(got) == set(want), (what, set(got) ^ set(want))
    for name, w in want.items():
        if isinstance(w, dict):
            assert_dict(got[name], w, (what, name))
        elif isinstance(w, np.ndarray):
            assert_bits(np.asarray(got[name]), w, (what, name))
        else:
            assert got[name] == w, (what, name)


def test_l_moments_and_block_maxima_from_host_and_device_arrays():
    from dl4ds_amd import extremes as ex
    from dl4ds_amd.device import DeviceArray
    obs, _, _ = host_case()
    grid = SHAPE[1:]
    for tail, sign in (('upper', 1), ('lower', -1)):
        n, pwm = ref.pwm(obs.reshape(40, -1), sign)
        want = {'n_valid': n.reshape(grid), 'pwm': pwm.reshape((4,) + grid)}
        want.update(ex.lmoments_from_pwm(want['pwm']))
        for b in BATCHES:
            assert_dict(ex.l_moments(obs, tail, batch_size=b), want, (tail, b))
        d = DeviceArray.from_numpy(obs)
        assert_dict(ex.l_moments(d, tail), want, (tail, 'device'))
        bm = ref.block_maxima(obs.reshape(40, -1), STARTS, sign, 4).reshape((8,) + grid)
        for b in BATCHES:
            assert_bits(ex.block_maxima(obs, period_starts=STARTS, tail=tail, min_valid=4, batch_size=b), bm, (tail, b))
        assert_bits(ex.block_maxima(d, np.repeat(np.arange(8), 5), tail=tail, min_valid=4), bm, (tail, 'device'))
        assert np.isnan(bm).any() and np.isfinite(bm).any()
        d.free()
    mask = np.ones(grid[:2], np.float32)
    mask[2:4, 1:5] = 0
    masked = obs.copy()
    masked[:, 2:4, 1:5] = np.nan
    assert_bits(ex.l_moments(obs, mask=mask, batch_size=4)['pwm'], ref.pwm(masked.reshape(40, -1))[1].reshape((4,) + grid))
    with pytest.raises(ValueError):
        ex.l_moments(DeviceArray.from_numpy(obs), mask=mask)


def test_peaks_over_threshold_from_host_and_device_arrays():
    from dl4ds_amd import extremes as ex
    from dl4ds_amd.device import DeviceArray
    obs, _, thr = host_case()
    grid = SHAPE[1:]
    for threshold, tail, sign, run in ((thr, 'upper', 1, 2), (10.0, 'lower', -1, 1)):
        flat = np.asarray(threshold, np.float32).reshape(-1)
        count, peak, pos = ref.pot_peaks(obs.reshape(40, -1), STARTS, flat, sign, run)
        K = peak.shape[0]
        want = {'n_peaks': count.reshape(grid), 'peaks': peak.reshape((K,) + grid), 'positions': pos.reshape((K,) + grid),
                'period_starts': STARTS}
        for b in BATCHES:
            assert_dict(ex.peaks_over_threshold(obs, threshold, run, tail, period_starts=STARTS, batch_size=b), want, (tail, b))
        d = DeviceArray.from_numpy(obs)
        assert_dict(ex.peaks_over_threshold(d, threshold, run, tail, periods=np.repeat(np.arange(8), 5)), want, (tail, 'device'))
        d.free()
        assert K >= 2 and (count == K).any() and (count[count >= 0] < K).any()


@pytest.mark.parametrize('method', ['gev', 'gumbel', 'pot'])
def test_extreme_scores(method):
    from dl4ds_amd import extremes as ex
    from dl4ds_amd.device import DeviceArray
    obs, pred, thr = host_case()
    grid = SHAPE[1:]
    T = (5, 10, 20, 50)

    def side(x):
        flat = x.reshape(40, -1)
        if method == 'pot':
            count, peak, _ = ref.pot_peaks(flat, STARTS, thr.reshape(-1), 1, 2)
            n, pwm = ref.pwm(peak, 1)
            fit = ex.gpd_fit_from_pwm(pwm.reshape((4,) + grid), n.reshape(grid), thr, 8, 1)
            fit['n_valid'] = count.reshape(grid)
        else:
            n, pwm = ref.pwm(ref.block_maxima(flat, STARTS), 1)
            m = ex.lmoments_from_pwm(pwm.reshape((4,) + grid))
            fit = ex.gev_from_lmoments(m['l1'], m['l2'], m['t3']) if method == 'gev' else ex.gumbel_from_lmoments(m['l1'], m['l2'])
            fit.update(n_valid=n.reshape(grid), sign=1, **m)
        return {'fit': fit, 'return_levels': ex.return_levels(fit, T), 'n_valid': fit['n_valid']}
    o, p = side(obs), side(pred)
    bias = p['return_levels'] - o['return_levels']
    with np.errstate(invalid='ignore', divide='ignore'):
        relb = np.where(np.abs(o['return_levels']) > 0, bias / np.abs(o['return_levels']), np.nan)
    want = {'obs': o, 'pred': p, 'bias': bias, 'relative_bias': relb, 'shape_difference': p['fit']['shape'] - o['fit']['shape'],
            'return_periods': np.asarray(T, np.float64)}
    kw = dict(period_starts=STARTS, return_periods=T, method=method, threshold=thr if method == 'pot' else None, run=2)
    for b in BATCHES:
        assert_dict(ex.extreme_scores(obs, pred, batch_size=b, **kw), want, (method, b))
    do, dp = DeviceArray.from_numpy(obs), DeviceArray.from_numpy(pred)
    assert_dict(ex.extreme_scores(do, dp, **kw), want, (method, 'device'))
    do.free()
    dp.free()
    assert bias.shape == (4,) + grid and np.isfinite(bias).sum() > bias.size // 2
