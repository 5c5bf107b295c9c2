"""CPU-side checks of the spectral verification (dl4ds_amd.metrics.spectral_scores / power_spectrum, csrc/spectrum.hip): the numpy
restatement tests/spectrum_ref.py against answers worked by hand and against a second fp64 evaluation of the transform (the DFT
matrices applied by ``@``), which also measures the constant C_REF of the GPU comparison; the radial bin map; the host arithmetic of
the product on hand-made device outputs; the argument validation (no library call); the exports and the C declaration."""
import inspect
import math
import os

import numpy as np
import pytest

from tests import spectrum_ref as ref
from tests.spectrum_cases import C, C_REF, CASES, CHUNK_FIELDS, MAX_BINS, MAX_DIM, WS_BUDGET, bytes_per_field

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(1, 1), (1, 8), (8, 1), (5, 8), (8, 5), (17, 33), (64, 64), (96, 130), (12, 7)]


def _scores(y, p, **kw):
    return ref.spectral_scores(np.asarray(y, np.float32)[None, :, :, None], np.asarray(p, np.float32)[None, :, :, None], **kw)[0]


def test_constant_field_by_hand():
    y = np.full((6, 9), 2.5, np.float32)
    r = _scores(y, y, detrend=None)
    want = np.zeros(r['power_obs'].shape)
    want[0, 0, 0] = 2.5 ** 2                                             # |sum v|^2 / (H W)^2
    np.testing.assert_allclose(r['power_obs'], want, rtol=0, atol=1e-14)
    r = _scores(y, y)
    assert (r['power_obs'] == 0).all() and r['mean_obs'][0, 0] == 2.5 and r['n_valid'][0, 0] == 54
    assert np.isnan(r['psd_ratio']).all() and np.isnan(r['coherence']).all() and np.isnan(r['lsd']).all()
    assert np.isnan(r['effective_wavelength']).all()


def test_single_cosine_by_hand():
    W = 16
    y = np.tile(np.cos(2 * np.pi * 3 * np.arange(W) / W), (W, 1))
    r = _scores(y, y, detrend=None)
    want = np.zeros(W // 2 + 1)
    want[3] = 0.5                                                        # two coefficients of H W / 2 each: 2 (1/2)^2
    np.testing.assert_allclose(r['power_obs'][0, 0], want, rtol=0, atol=2.0 ** -22)    # the cosine is rounded to float32
    assert r['wavenumber'][3] == 3 / 16 and r['wavelength'][3] == 16 / 3 and r['wavelength'][0] == math.inf
    assert r['count'][3] == np.sum(ref.radial_map(W, W)[0] == 3)
    np.testing.assert_allclose(r['psd_obs'][0, 0, 3], 0.5 / r['count'][3], rtol=2.0 ** -21)


@pytest.mark.parametrize('shape', SHAPES)
@pytest.mark.parametrize('window', [None, 'hann'])
def test_parseval(shape, window):
    rng = np.random.default_rng(5)
    y = rng.standard_normal(shape).astype(np.float32)
    full, B = ref.radial_map(*shape)
    vy, _, _, _, _ = ref.prepared_field(y, None, False, window == 'hann')
    sums = ref.field_sums(y, None, full, B, False, window == 'hann')[0]
    dropped = float((np.abs(np.fft.fft2(vy)) ** 2)[full < 0].sum())
    hw = shape[0] * shape[1]
    np.testing.assert_allclose((sums[0].sum() + dropped) / hw ** 2, (vy ** 2).sum() / hw, rtol=1e-12)


def test_prediction_equal_to_the_observation():
    rng = np.random.default_rng(6)
    y = rng.standard_normal((12, 7))
    r = _scores(y, y)
    some = r['count'] > 0
    assert some[1:].all()
    np.testing.assert_allclose(r['coherence'][0, 0, 1:], 1.0, rtol=1e-12)
    assert (r['psd_ratio'][0, 0, 1:] == 1.0).all() and r['lsd'][0, 0] == 0.0 and r['lsd_pooled'][0] == 0.0
    assert r['effective_wavelength'][0] == r['wavelength'][-1]


def test_shifted_prediction_has_equal_power_and_the_known_phase():
    rng = np.random.default_rng(7)
    W = 16
    y = rng.standard_normal((W, W)).astype(np.float32)
    p = np.roll(y, 1, axis=1)                                            # P = Y exp(-2 pi i kx / W): Y conj(P) = |Y|^2 exp(+2 pi i kx / W)
    kx = np.minimum(np.arange(W), W - np.arange(W))
    full = np.broadcast_to(kx[None, :], (W, W)).astype(np.int32)         # bin = |kx|: symmetric, one column of the half plane each
    r = _scores(y, p, bins=full, detrend=None)
    np.testing.assert_allclose(r['power_pred'], r['power_obs'], rtol=1e-12)
    phase = np.exp(2j * np.pi * np.arange(W // 2 + 1) / W)               # (real at kx = 0 and at the Nyquist column)
    np.testing.assert_allclose(r['cross'][0, 0], r['power_obs'][0, 0] * phase, rtol=0, atol=1e-12 * r['power_obs'].max())
    np.testing.assert_allclose(r['coherence'][0, 0], 1.0, rtol=1e-12)
    # the power of a symmetric map is the full-plane sum
    vy = ref.prepared_field(y, p, False, False)[0]
    whole = np.bincount(full.ravel(), weights=(np.abs(np.fft.fft2(vy)) ** 2).ravel()) / float(W * W) ** 2
    np.testing.assert_allclose(r['power_obs'][0, 0], whole, rtol=1e-12)


@pytest.mark.parametrize('name', sorted(CASES))
def test_two_references_agree_within_c_ref(name):
    """np.fft.fft2 against the matrix-product DFT, coefficient by coefficient: |difference| <= C_REF 2^-52 sqrt(T), and the binned
    sums of the two agree within the bound the device is held to"""
    c = CASES[name]()
    y, p = c['y'][:4], c['p'][:4]
    if isinstance(c['bins'], str):
        full, B = ref.radial_map(*y.shape[1:3])
    else:
        full, B = c['bins'], int(c['bins'].max()) + 1
    count = np.bincount(full[full >= 0].ravel(), minlength=B)
    dt, win = c['detrend'] == 'mean', c['window'] == 'hann'
    a, nv, _, T = ref.device_outputs(y, p, full, B, dt, win, c['mask'])
    worst = 0.0
    ym = np.array(y)
    if c['mask'] is not None:
        ym[np.broadcast_to(c['mask'][..., None] == 0, ym.shape)] = np.nan
    b = np.zeros_like(a)
    for n in range(y.shape[0]):
        for ch in range(y.shape[3]):
            b[n, ch] = ref.field_sums(ym[n, :, :, ch], p[n, :, :, ch], full, B, dt, win, transform=ref.dft2_matrix)[0]
            vy, vp, _, _, t = ref.prepared_field(ym[n, :, :, ch], p[n, :, :, ch], dt, win)
            if t > 0:
                for v in (vy, vp):
                    worst = max(worst, float(np.abs(np.fft.fft2(v) - ref.dft2_matrix(v)).max()) / (2.0 ** -52 * math.sqrt(t)))
    assert worst <= C_REF, worst
    assert C == 16 * C_REF
    assert (np.abs(a - b) <= ref.bound(a, T, count, C)).all()
    assert np.isfinite(a).all()


@pytest.mark.parametrize('shape', SHAPES + [(255, 256)])
def test_radial_map(shape):
    from dl4ds_amd.metrics import radial_bin_map
    H, W = shape
    full, B = ref.radial_map(H, W)
    got, gb = radial_bin_map(H, W)
    assert gb == B == max(H, W) // 2 + 1 and got.dtype == np.int32
    np.testing.assert_array_equal(got, full)
    mirror = full[np.ix_([(-k) % H for k in range(H)], [(-k) % W for k in range(W)])]
    np.testing.assert_array_equal(full, mirror)
    assert full.min() >= -1 and full.max() < B and full[0, 0] == 0
    assert np.bincount(full[full >= 0].ravel(), minlength=B).sum() == H * W - int((full < 0).sum())
    if H == W:
        k = np.minimum(np.arange(H), H - np.arange(H)).astype(np.float64)
        b = np.floor(np.hypot(k[:, None], k[None, :]) + 0.5).astype(np.int64)
        np.testing.assert_array_equal(full, np.where(b < B, b, -1))
        assert (full < 0).any() == (H > 2)                                # the corners lie beyond the Nyquist circle


def _random_outputs(seed, N=4, C_=2, B=9, hw=(16, 12)):
    rng = np.random.default_rng(seed)
    power = np.zeros((N, C_, 4, B))
    power[:, :, 0] = rng.gamma(2.0, 50.0, (N, C_, B))
    power[:, :, 1] = power[:, :, 0] * rng.uniform(0.2, 1.4, (N, C_, B))
    mag = np.sqrt(power[:, :, 0] * power[:, :, 1]) * rng.uniform(0, 1, (N, C_, B))
    ang = rng.uniform(-np.pi, np.pi, (N, C_, B))
    power[:, :, 2], power[:, :, 3] = mag * np.cos(ang), mag * np.sin(ang)
    nvalid = np.full((N, C_), hw[0] * hw[1], np.int64)
    mean = rng.standard_normal((N, C_, 2))
    count = rng.integers(1, 30, B)
    return power, nvalid, mean, count


def _same(got, want):
    assert set(got) == set(want)
    for k in want:
        g, w = np.asarray(got[k]), np.asarray(want[k])
        assert g.dtype == w.dtype and g.shape == w.shape, k
        np.testing.assert_array_equal(g, w, err_msg=k)                    # NaN positions included


def test_host_arithmetic_on_hand_made_device_outputs():
    from dl4ds_amd.metrics import spectra_from_sums
    power, nvalid, mean, count = _random_outputs(11)
    power[1, 0] = 0.0
    nvalid[1, 0] = 0                                                      # an empty field: zeros from the device
    power[2, 1, 1, 3] = 0.0                                               # a zero denominator of the coherence, a zero ratio
    power[3, 0, 0, 4] = 0.0                                               # a zero denominator of the ratio
    count[5] = 0
    power[:, :, :, 5] = 0.0
    got = spectra_from_sums(power, nvalid, mean, count, (16, 12), spacing=2.5, ratio_floor=0.6)
    _same(got, ref.scores_from_sums(power, nvalid, mean, count, (16, 12), spacing=2.5, ratio_floor=0.6))
    norm = (16 * 12) ** 2
    assert got['power_obs'][0, 0, 2] == power[0, 0, 0, 2] / norm and got['psd_pred'][0, 1, 2] == power[0, 1, 1, 2] / norm / count[2]
    assert got['cross'].dtype == np.complex128 and got['cross'][0, 0, 1] == complex(power[0, 0, 2, 1], power[0, 0, 3, 1]) / norm
    assert got['wavenumber'][3] == 3 / (16 * 2.5) and got['count'].dtype == np.int64
    for k in ('psd_obs', 'psd_pred', 'coherence', 'psd_ratio'):
        assert np.isnan(got[k][1, 0]).all(), k
        assert np.isnan(got[k][:, :, 5]).all(), k
    assert np.isnan(got['lsd'][1, 0]) and np.isfinite(np.delete(got['lsd'].ravel(), 2)).all()
    assert (got['power_obs'][1, 0] == 0).all()
    assert np.isnan(got['coherence'][2, 1, 3]) and got['psd_ratio'][2, 1, 3] == 0.0 and np.isnan(got['psd_ratio'][3, 0, 4])
    np.testing.assert_allclose(got['power_obs_pooled'][0], (power[[0, 2, 3], 0, 0] / norm).sum(0), rtol=1e-14)
    np.testing.assert_allclose(got['power_obs_pooled'][1], (power[:, 1, 0] / norm).sum(0), rtol=1e-14)
    c = 1
    d = 10 * np.log10(got['psd_ratio'][0, c][[1, 2, 3, 4, 6, 7, 8]])
    np.testing.assert_allclose(got['lsd'][0, c], np.sqrt(np.mean(d ** 2)), rtol=1e-13)


def test_effective_wavelength_by_hand():
    from dl4ds_amd.metrics import spectra_from_sums
    B = 8
    power = np.zeros((1, 1, 4, B))
    power[0, 0, 0] = 1.0
    power[0, 0, 1] = [1.0, 0.9, 0.8, 0.0, 0.55, 0.45, 0.9, 0.9]
    count = np.array([1, 4, 8, 0, 12, 16, 20, 8])
    kw = dict(nvalid=np.array([[64]]), mean=np.zeros((1, 1, 2)), count=count, hw=(8, 8))
    r = spectra_from_sums(power, **kw)
    assert r['effective_wavelength'][0] == r['wavelength'][4] == 2.0       # bin 3 is empty and passes, bin 5 is the first below 0.5
    assert np.isnan(spectra_from_sums(power, ratio_floor=0.95, **kw)['effective_wavelength'][0])
    assert spectra_from_sums(power, ratio_floor=0.4, **kw)['effective_wavelength'][0] == r['wavelength'][7]
    _same(r, ref.scores_from_sums(power, kw['nvalid'], kw['mean'], count, (8, 8)))
    one = spectra_from_sums(power[..., :1], kw['nvalid'], kw['mean'], count[:1], (1, 1))
    assert np.isnan(one['effective_wavelength'][0]) and np.isnan(one['lsd'][0, 0]) and one['wavelength'][0] == math.inf


def _no_library(monkeypatch):
    import dl4ds_amd._lib as L

    def boom(*a, **k):
        raise AssertionError('the library was touched')
    monkeypatch.setattr(L, 'lib', boom)
    monkeypatch.setattr(L, 'load', boom)


def _asym():
    m = np.zeros((6, 5), np.int32)
    m[1, 2] = 1
    return m


@pytest.mark.parametrize('kw', [dict(bins='ring'), dict(bins=3), dict(bins=np.zeros((6, 4), np.int32)), dict(bins=np.zeros((6, 5))),
                                dict(bins=np.zeros((6, 5), bool)), dict(bins=np.full((6, 5), -1)), dict(bins=np.full((6, 5), -2)),
                                dict(bins=np.full((6, 5), MAX_BINS)), dict(bins=_asym()), dict(detrend='linear'), dict(detrend=1),
                                dict(window='hamming'), dict(window=True), dict(spacing=0.0), dict(spacing=-1.0),
                                dict(spacing=np.nan), dict(spacing=np.inf), dict(spacing='1'), dict(ratio_floor=0.0),
                                dict(ratio_floor=np.nan), dict(batch_size=0), dict(batch_size=1.5)])
def test_argument_validation_without_a_library_call(monkeypatch, kw):
    from dl4ds_amd.metrics import spectral_scores

    class Scaler:
        def inverse_transform(self, a):
            raise AssertionError('inverse_transform ran before the validation')

    _no_library(monkeypatch)
    y = np.zeros((2, 6, 5, 1), np.float32)
    with pytest.raises(ValueError):
        spectral_scores(y, y, scaler=Scaler(), **kw)


def test_shape_validation_and_accepted_arguments_without_a_library_call(monkeypatch):
    from dl4ds_amd.metrics import check_spectral_args, power_spectrum, spectral_scores
    _no_library(monkeypatch)
    y = np.zeros((2, 6, 5, 1), np.float32)
    for a, b in [(y, y[:1]), (y, y[:, :, :4]), (y[:0], y[:0])]:
        with pytest.raises(ValueError):
            spectral_scores(a, b)
    with pytest.raises(ValueError):
        power_spectrum(y, window='hamming')
    with pytest.raises(ValueError):
        power_spectrum(y[:0])
    with pytest.raises(ValueError, match='mask'):
        spectral_scores(y, y, mask=np.ones((3, 3)))
    with pytest.raises(ValueError, match=str(MAX_DIM)):
        check_spectral_args((1, MAX_DIM + 1, 4, 1))
    with pytest.raises(ValueError, match=str(MAX_DIM)):
        check_spectral_args((1, 4, MAX_DIM + 1, 1))
    with pytest.raises(ValueError, match=r'2\^31'):
        check_spectral_args((2 ** 16, 4, 4, 2 ** 15))
    full, B, dt, win = check_spectral_args(y.shape)
    assert full.shape == (6, 5) and full.dtype == np.int32 and B == 4 and (dt, win) == (1, 0)
    sym = np.array([[0, 1, 2, 2, 1]] * 6, np.int64)
    sym[3, 0] = -1
    full, B, dt, win = check_spectral_args(y.shape, sym, None, 'hann', 2, 0.7, 3)
    assert full.dtype == np.int32 and B == 3 and (dt, win) == (0, 1)
    np.testing.assert_array_equal(full, sym)


def test_exports_and_signatures():
    import dl4ds_amd as dds
    from dl4ds_amd import metrics
    assert dds.spectral_scores is metrics.spectral_scores and dds.power_spectrum is metrics.power_spectrum
    sig = inspect.signature(metrics.spectral_scores)
    assert list(sig.parameters) == ['y_test', 'y_test_hat', 'bins', 'detrend', 'window', 'spacing', 'ratio_floor', 'scaler', 'mask',
                                    'batch_size']
    d = {k: v.default for k, v in sig.parameters.items() if v.default is not inspect.Parameter.empty}
    assert d == dict(bins='radial', detrend='mean', window=None, spacing=1.0, ratio_floor=0.5, scaler=None, mask=None,
                     batch_size=None)
    sig = inspect.signature(metrics.power_spectrum)
    assert list(sig.parameters) == ['y', 'bins', 'detrend', 'window', 'spacing', 'scaler', 'mask']
    d = {k: v.default for k, v in sig.parameters.items() if v.default is not inspect.Parameter.empty}
    assert d == dict(bins='radial', detrend='mean', window=None, spacing=1.0, scaler=None, mask=None)


def test_c_entry_is_declared():
    import dl4ds_amd._lib as L
    protos = L.parse_header()
    assert 'dl4ds_spectrum' in protos                         # tests/test_abi.py then checks that the library exports it
    assert len(protos['dl4ds_spectrum'][1]) == 13
    assert os.path.exists(os.path.join(ROOT, 'dl4ds_amd', 'csrc', 'spectrum.hip'))
    assert CHUNK_FIELDS * bytes_per_field(64, 64) > WS_BUDGET >= (CHUNK_FIELDS - 7) * bytes_per_field(64, 64)


@pytest.mark.parametrize('name', sorted(CASES))
def test_reference_is_nan_on_the_gpu_cases_only_by_construction(name):
    """the NaNs of the expected arrays of tests/test_gpu_spectral.py: the fields built to have no kept cell, bins without a
    coefficient, and ratios whose denominator is a bin the map leaves empty -- nothing else"""
    c = CASES[name]()
    y, p = c['y'][:6], c['p'][:6]                             # (the property is per field: six fields of the long case stand for all)
    r, power, T = ref.spectral_scores(y, p, c['bins'], c['detrend'], c['window'], mask=c['mask'])
    empty = r['n_valid'] == 0
    assert int(empty.sum()) == c['empty']
    no_coeff = np.broadcast_to(r['count'] == 0, r['psd_obs'].shape)
    by_construction = no_coeff | empty[..., None]
    for k in ('psd_obs', 'psd_pred'):
        np.testing.assert_array_equal(np.isnan(r[k]), by_construction, err_msg=k)
    if name == 'shape1x1':                                    # a single cell without detrending: all power in bin 0, which is fine,
        assert (r['power_obs'] > 0).all()                     # and there is no bin b >= 1: lsd has nothing to average
        assert np.isnan(r['lsd']).all()
        return
    zero_power = power[:, :, 0] == 0                          # exact zeros: only where no coefficient lands, or the field is empty,
    if c['detrend'] == 'mean':                                # or the mean was removed from bin 0
        by_construction = by_construction | (np.arange(power.shape[-1]) == 0)
    for k in ('psd_ratio', 'coherence'):
        nan = np.isnan(r[k])
        assert (nan <= (by_construction | zero_power)).all(), k
        assert not nan[~by_construction & ~zero_power].any(), k
    assert np.isfinite(power).all() and np.isfinite(T).all()
    has_bins = (r['count'][1:] > 0).any()
    np.testing.assert_array_equal(np.isnan(r['lsd']), empty | (not has_bins))
    assert (power[empty] == 0).all()
