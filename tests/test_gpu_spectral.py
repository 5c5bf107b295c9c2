"""Spectral verification on the device (dl4ds_spectrum, csrc/spectrum.hip) through dl4ds_amd.metrics.spectral_scores against the
numpy restatement tests/spectrum_ref.py (np.fft.fft2 in fp64, itself checked by hand and against a matrix-product DFT in
tests/test_spectral_api.py).  n_valid and count are compared for equality, the means at 2^-50 max|x|.  The power and cross sums are
compared per field f and bin b by the error model of a direct fp64 transform,
    |got - want| <= 2 d sqrt(M_b S_b) + M_b d^2,  d = C 2^-52 sqrt(T_f),  T_f = H W sum over kept cells of the raw y^2 + p^2,
S_b the larger of the two reference powers of the bin, M_b = count[b], C = 16 C_REF (tests/spectrum_cases.py: C_REF = 0.45 is the
largest coefficient-wise difference of the two CPU references in these units).  Every derived score is then compared for equality,
NaN positions included, with the restated host arithmetic applied to the device's own sums, which agree with the reference sums
within that bound.  Every case prints its largest error / bound; DESIGN.md section 16 records what was observed on an MI355X."""
import functools

import numpy as np
import pytest

from tests import spectrum_ref as ref
from tests.spectrum_cases import C, CASES, MAX_BINS, MAX_DIM, WS_BUDGET, bytes_per_field

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def case(name):
    """(case, expected dict, reference sums, T), computed once per session and left unchanged"""
    c = CASES[name]()
    want, power, T = ref.spectral_scores(c['y'], c['p'], c['bins'], c['detrend'], c['window'], mask=c['mask'])
    return c, want, power, T


def check(got, want, power, T, hw, raw, spacing=1.0, ratio_floor=0.5):
    """`raw`: the largest |x| of either input (the scale of the means)"""
    assert set(got) == set(want)
    for k in ('n_valid', 'count'):
        assert got[k].dtype == np.int64 and got[k].shape == want[k].shape, k
        np.testing.assert_array_equal(got[k], want[k], err_msg=k)
    for k in ('wavenumber', 'wavelength'):
        np.testing.assert_array_equal(got[k], want[k], err_msg=k)
    for k in ('mean_obs', 'mean_pred'):
        assert got[k].dtype == np.float64 and got[k].shape == want[k].shape, k
        assert (np.abs(got[k] - want[k]) <= 2.0 ** -50 * raw).all(), (k, float(np.abs(got[k] - want[k]).max()))
    norm = float((hw[0] * hw[1]) ** 2)
    bound = ref.bound(power, T, want['count'], C)
    gp = np.stack([got['power_obs'], got['power_pred'], got['cross'].real, got['cross'].imag], 2)
    assert gp.shape == power.shape and gp.dtype == np.float64
    err = np.abs(gp * norm - power)
    # (gp * norm undoes one division: one more rounding of at most 2^-53 of the value, far inside the bound where the bound is not 0)
    slack = 2.0 ** -52 * np.abs(power)
    ratio = float(np.max(np.where(bound > 0, err / np.where(bound > 0, bound, 1.0), 0.0), initial=0.0))
    print(f'largest error / bound: {ratio:.3e}')
    assert (err <= bound + slack).all(), (ratio, float(err.max()))
    near0 = bound[:, :, 0]                                                # (one bound for the four components of a bin)
    vague = ((np.abs(power[:, :, 0]) <= near0) | (np.abs(power[:, :, 1]) <= near0)) & (want['n_valid'] > 0)[..., None]
    mean = np.stack([got['mean_obs'], got['mean_pred']], -1)
    # the host arithmetic, restated, from the normalised sums the dict carries (norm 1: hw = (1, 1), the spacing scaled to match)
    again = ref.scores_from_sums(gp, got['n_valid'], mean, got['count'], (1, 1), spacing * max(hw), ratio_floor)
    for k in want:
        if k in ('n_valid', 'count', 'wavenumber', 'wavelength'):
            continue
        g, w = np.asarray(got[k]), np.asarray(again[k])
        assert g.dtype == w.dtype and g.shape == w.shape, k
        np.testing.assert_array_equal(g, w, err_msg=k)                    # NaN positions included
        # ... and the NaN positions against the reference's own.  A ratio is NaN iff its denominator is exactly 0; where the
        # reference's power is within its bound of 0 (bin 0 after detrending: the rounding residue of the mean) that is not decided
        # by the definitions, so those denominators are compared through the sums above only
        settled = np.ones(g.shape, bool)
        if k in ('psd_ratio', 'coherence'):
            settled = ~vague
        elif k in ('psd_ratio_pooled', 'coherence_pooled'):
            settled = ~vague.any(0)
        np.testing.assert_array_equal(np.isnan(g)[settled], np.isnan(np.asarray(want[k]))[settled], err_msg=k)
    return ratio


def _raw(c):
    return float(max(np.abs(c['y'][np.isfinite(c['y'])]).max(), np.abs(c['p'][np.isfinite(c['p'])]).max()))


@pytest.mark.parametrize('name', sorted(CASES))
def test_against_the_restatement(name):
    from dl4ds_amd.metrics import spectral_scores
    c, want, power, T = case(name)
    got = spectral_scores(c['y'], c['p'], c['bins'], c['detrend'], c['window'], mask=c['mask'])
    N, H, W, Cn = c['y'].shape
    B = len(want['count'])
    assert got['power_obs'].shape == (N, Cn, B) and got['lsd'].shape == (N, Cn) and got['lsd_pooled'].shape == (Cn,)
    check(got, want, power, T, (H, W), _raw(c))
    assert int((got['n_valid'] == 0).sum()) == c['empty']
    empty = got['n_valid'] == 0
    assert (got['power_obs'][empty] == 0).all() and (got['power_pred'][empty] == 0).all() and (got['cross'][empty] == 0).all()
    for k in ('psd_obs', 'psd_pred', 'coherence', 'psd_ratio', 'lsd'):
        assert np.isnan(got[k][empty]).all(), k
    if name == 'workspace_chunks':
        assert N * Cn * bytes_per_field(H, W) > WS_BUDGET
    if name == 'map_one_bin':
        assert B == 1 and got['count'].tolist() == [H * W]
    if name == 'map_one_coefficient':
        assert B == 1 and got['count'].tolist() == [2]
    if name == 'shape1x1':
        np.testing.assert_array_equal(got['power_obs'][:, 0, 0], c['y'][:, 0, 0, 0].astype(np.float64) ** 2)
    if name.startswith('offset280') and c['detrend'] == 'mean':
        assert (np.abs(got['mean_obs'] - 280.0) < 0.5).all()


def test_power_spectrum_uses_the_entry_without_a_prediction():
    from dl4ds_amd.metrics import power_spectrum, spectral_scores
    c, want, power, T = case('nonfinite')
    y = np.array(c['y'])
    y[~np.isfinite(c['p'])] = np.nan                                      # the cells that the pair drops, so that both keep the same
    k, psd = power_spectrum(y, window=c['window'])
    np.testing.assert_array_equal(k, want['wavenumber'])
    H, W = y.shape[1:3]
    full, B = ref.radial_map(H, W)
    wp, wn, wm, wT = ref.device_outputs(y, None, full, B, True, False)
    assert (wp[:, :, 1:] == 0).all()
    norm = float((H * W) ** 2)
    bound = ref.bound(wp, wT, want['count'], C)[:, :, 0]
    with np.errstate(invalid='ignore'):
        err = np.abs(psd * want['count'] * norm - wp[:, :, 0])
    assert (err <= bound + 2.0 ** -51 * wp[:, :, 0]).all()
    np.testing.assert_array_equal(wn, want['n_valid'])
    both = spectral_scores(y, y)                                          # the same field on both sides: its power twice
    np.testing.assert_array_equal(both['power_obs'], both['power_pred'])
    np.testing.assert_array_equal(psd, both['psd_obs'])


def test_wrapper_scaler_spacing_and_5d_input():
    from dl4ds_amd.metrics import spectral_scores

    class Scaler:
        def inverse_transform(self, a):
            return a * 2.0 + 1.0

    c = CASES['channels17x33']()
    y2, p2 = (c['y'] * 2.0 + 1.0).astype(np.float32), (c['p'] * 2.0 + 1.0).astype(np.float32)
    want, power, T = ref.spectral_scores(y2, p2, 'radial', 'mean', 'hann', spacing=12.5, ratio_floor=0.8)
    got = spectral_scores(c['y'][..., None], c['p'][..., None], window='hann', spacing=12.5, ratio_floor=0.8, scaler=Scaler())
    check(got, want, power, T, (17, 33), float(max(np.abs(y2).max(), np.abs(p2).max())), 12.5, 0.8)
    direct = spectral_scores(y2, p2, window='hann', spacing=12.5, ratio_floor=0.8)
    for k in want:
        assert np.asarray(got[k]).tobytes() == np.asarray(direct[k]).tobytes(), k
    assert got['wavelength'][1] == 33 * 12.5


@pytest.mark.parametrize('name', ['nonfinite', 'mask2d', 'shape64x64'])
def test_result_does_not_depend_on_batch_size_and_is_reproducible(name):
    """samples per upload: the default, 1, 2 (a non-divisor of 3), more than there are; and the same call twice"""
    from dl4ds_amd.metrics import spectral_scores
    c, want, power, T = case(name)
    args = (c['y'], c['p'], c['bins'], c['detrend'], c['window'])
    first = spectral_scores(*args, mask=c['mask'])
    for bs in (None, 1, 2, 1000):
        got = spectral_scores(*args, mask=c['mask'], batch_size=bs)
        for k in first:
            assert np.asarray(got[k]).tobytes() == np.asarray(first[k]).tobytes(), (bs, k)
    if name == 'nonfinite':                                               # and not on which fields share a call: sample 1 alone
        alone = spectral_scores(c['y'][1:2], c['p'][1:2], c['bins'], c['detrend'], c['window'])
        for k in ('power_obs', 'power_pred', 'cross', 'mean_obs', 'lsd'):
            assert alone[k].tobytes() == first[k][1:2].tobytes(), k


def _direct(y, p, N, H, W, Cn, bins, B, detrend=1, window=0, fill=7):
    """dl4ds_spectrum called directly -> (status, power, valid, mean)"""
    import dl4ds_amd._lib as L_
    from dl4ds_amd.device import DeviceArray
    dy = DeviceArray.from_numpy(y)
    dp = DeviceArray.from_numpy(p) if p is not None else None
    Bo = max(B, 1) if B <= MAX_BINS else 1
    shapes = (((N * Cn, 4, Bo), np.float64), ((N * Cn,), np.int64), ((N * Cn, 2), np.float64))
    outs = [DeviceArray.from_numpy(np.full(s, fill, d)) for s, d in shapes]
    bins = np.ascontiguousarray(bins, np.int32)
    st = L_.lib().dl4ds_spectrum(dy.ptr, dp.ptr if dp is not None else None, N, H, W, Cn, detrend, window, bins.ctypes.data, B,
                                 *(o.ptr for o in outs))
    res = (st,) + tuple(o.numpy() for o in outs)
    for d in [dy, dp] + outs:
        if d is not None:
            d.free()
    return res


def test_refusals_of_the_c_entry():
    import dl4ds_amd._lib as L_
    y = np.zeros((2, 4, 6, 1), np.float32)
    half = np.zeros((4, 4), np.int32)
    ok = dict(N=2, H=4, W=6, Cn=1, bins=half, B=1)
    bad_map = half.copy()
    bad_map[3, 3] = 1
    low_map = half.copy()
    low_map[0, 1] = -2
    for bad, word in [(dict(H=0), '16384'), (dict(W=0), '16384'), (dict(H=MAX_DIM + 1), '16384'), (dict(W=MAX_DIM + 1), '16384'),
                      (dict(B=0), 'bins'), (dict(B=MAX_BINS + 1), 'bins'), (dict(bins=bad_map), '[-1, B)'),
                      (dict(bins=low_map), '[-1, B)'), (dict(N=2 ** 16, Cn=2 ** 15), '2^31')]:
        args = dict(ok)
        args.update(bad)
        res = _refused_big(y, half) if 'N' in bad else _direct(y, y, fill=7, **args)
        assert res[0] != 0, bad
        assert word in L_.load().dl4ds_last_error().decode(), (bad, L_.load().dl4ds_last_error().decode())
        assert all((o == 7).all() for o in res[1:]), bad                   # nothing was written


def _refused_big(y, half):
    """N*C = 2^31 with outputs sized for the real arrays: the entry must refuse before it touches anything"""
    import dl4ds_amd._lib as L_
    from dl4ds_amd.device import DeviceArray
    dy = DeviceArray.from_numpy(y)
    outs = [DeviceArray.from_numpy(np.full(s, 7, d)) for s, d in (((2, 4, 1), np.float64), ((2,), np.int64), ((2, 2), np.float64))]
    st = L_.lib().dl4ds_spectrum(dy.ptr, dy.ptr, 2 ** 16, 4, 6, 2 ** 15, 1, 0, half.ctypes.data, 1, *(o.ptr for o in outs))
    res = (st,) + tuple(o.numpy() for o in outs)
    for d in [dy] + outs:
        d.free()
    return res


def test_direct_call_overwrites_its_outputs():
    """garbage in the outputs; two sides and one; channels; the three arrays against the restatement"""
    rng = np.random.default_rng(77)
    N, H, W, Cn = 2, 9, 12, 3
    y = rng.standard_normal((N, H, W, Cn)).astype(np.float32)
    p = rng.standard_normal((N, H, W, Cn)).astype(np.float32)
    y[0, 0, 0, 1] = np.nan
    y[1, :, :, 2] = np.nan
    full, B = ref.radial_map(H, W)
    count = np.bincount(full[full >= 0].ravel(), minlength=B)
    for pred, detrend, window in [(p, 1, 0), (p, 0, 1), (None, 1, 1)]:
        st, power, valid, mean = _direct(y, pred, N, H, W, Cn, full[:, :W // 2 + 1], B, detrend, window, fill=7)
        assert st == 0
        wp, wn, wm, wT = ref.device_outputs(y, pred, full, B, bool(detrend), bool(window))
        np.testing.assert_array_equal(valid.reshape(N, Cn), wn)
        assert (np.abs(mean.reshape(N, Cn, 2) - wm) <= 2.0 ** -50 * 6.0).all()
        assert (np.abs(power.reshape(N, Cn, 4, B) - wp) <= ref.bound(wp, wT, count, C)).all()
        assert (power.reshape(N, Cn, 4, B)[1, 2] == 0).all() and valid.reshape(N, Cn)[1, 2] == 0 and (mean.reshape(N, Cn, 2)[1, 2] == 0).all()
        if pred is None:
            assert (power.reshape(N, Cn, 4, B)[:, :, 1:] == 0).all() and (mean.reshape(N, Cn, 2)[..., 1] == 0).all()
        if not detrend:
            assert (mean == 0).all()
        again = _direct(y, pred, N, H, W, Cn, full[:, :W // 2 + 1], B, detrend, window, fill=-3)
        assert again[1].tobytes() == power.tobytes() and again[3].tobytes() == mean.tobytes()   # a repeated call: the same bits
