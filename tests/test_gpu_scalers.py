"""dl4ds_amd.preprocessing on the device (csrc/scaler.hip through the C ABI): MinMaxScaler / StandardScaler against the recorded
reference (tests/golden/reference_scalers.npz, judged by tests/scaler_ref.py check_case with the bounds stated in
tests/test_preprocessing_api.py) and, at sizes that take the multi-workgroup paths and the finishing kernel, against the fp64
restatement tests/scaler_ref.py:

* data_min_, data_max_, nan_mask: equal.  transform / inverse_transform: bit-identical to numpy's arithmetic on the scaler's own
  fitted attributes (inputs keep every result in the normal range).
* mean_ / std_, float32 data: at most 1 ulp / 2 ulp of float32 from the fp64 value (fp64 accumulation: only the final rounding, a
  double rounding and the square root remain).  Inputs have |mean| / std = 23 (kelvin-like: mean 281, std 12), within the 10^3 the
  bound assumes.
* float64 data: 2 * (ceil(log2 n) + 8) * eps64 * nanmean(|x|) absolute on the mean, the same factor relative on the std times
  (1 + |mean| / std).
"""
import math

import numpy as np
import pytest

from tests import scaler_ref as R

pytestmark = pytest.mark.gpu

META, ARRAYS = R.load_fixture()


def device_class(name):
    import dl4ds_amd.preprocessing as P
    return getattr(P, name)


def field(rng, shape, dtype, nan):
    x = (281.0 + 12.0 * rng.standard_normal(shape)).astype(dtype)
    if nan:
        x[rng.random(shape) < 0.03] = np.nan
        x[..., :2, :3] = np.nan if x.ndim == 3 else x[..., :2, :3]
        x[1] = np.nan
    return x


def check_stats(sc_attrs, x, axis, names=('min', 'max', 'mean', 'std')):
    t = R.stats(x, axis)
    n = np.squeeze(x).size
    for k in names:
        got = sc_attrs[k]
        assert got.dtype == x.dtype and got.shape == t[k].shape, (k, got.dtype, got.shape, t[k].shape)
        np.testing.assert_array_equal(np.isnan(got), np.isnan(t[k]))
        if k in ('min', 'max'):
            np.testing.assert_array_equal(got, t[k])
        elif x.dtype == np.float32:
            d = R.ulp_diff(got, t[k])
            print(f'{k}: worst {d.max():.2f} ulp of float32 over {d.size} cells')
            assert d.max() <= (1 if k == 'mean' else 2), (k, d.max())
        else:
            f = 2 * (math.ceil(math.log2(n)) + 8) * np.finfo(np.float64).eps
            with np.errstate(all='ignore'):
                bound = f * np.nanmean(np.abs(x)) if k == 'mean' else f * (np.abs(t['std64']) + np.abs(t['mean64']))
                err = np.abs(got - t[k + '64'])
            ok = ~np.isnan(t[k])
            print(f'{k}: worst |err| {np.max(err[ok], initial=0):.3e}, bound {np.min(np.broadcast_to(bound, err.shape)[ok]):.3e}')
            assert np.all(err[ok] <= np.broadcast_to(bound, err.shape)[ok]), k


@pytest.mark.parametrize('name', META['case_names'])
def test_recorded_reference_cases(name):
    cls, kw, x, xt = R.case_setup(META, ARRAYS, name)
    R.check_case(name, META, ARRAYS, R.run_case(device_class, cls, kw, x, xt))


BIG = [
    ('none', (4097, 2053), None, np.float32, True),            # one cell, 8.4 M elements (odd: the last 16-byte group is partial)
    ('none_f64', (1000, 4099), None, np.float64, True),
    ('inner_reduced', (48, 256, 512), (1, 2), np.float32, True),      # rows split over workgroups + finishing kernel
    ('inner_reduced_odd', (64, 301, 303), (1, 2), np.float32, True),  # rows not a multiple of four: the scalar-load kernel
    ('inner_kept', (400, 96, 128), 0, np.float32, True),              # lanes along the kept index, reduced range split
    ('inner_kept_odd_f64', (37, 129, 131), 0, np.float64, True),
    ('kept_3', (64, 96, 80, 3), (0, 1, 2), np.float32, True),         # kept innermost extent of 3, read flat
    ('kept_3_f64', (40, 50, 31, 3), (0, 1, 2), np.float64, False),
    ('middle', (300, 40, 257), (0, 2), np.float32, True),
    ('five_d', (6, 5, 32, 33, 4), (1, 3), np.float32, True),
    ('five_d_b', (6, 5, 32, 33, 4), (0, 2, 4), np.float32, False),
    ('last_axis', (500, 300, 24), 2, np.float32, False),
    ('empty_axis_tuple', (64, 1000), (), np.float32, True),
]


@pytest.mark.parametrize('tag,shape,axis,dtype,nan', BIG, ids=[b[0] for b in BIG])
def test_every_axis_form_against_the_restatement(tag, shape, axis, dtype, nan):
    from dl4ds_amd.preprocessing import MinMaxScaler, StandardScaler
    rng = np.random.default_rng(len(tag) + sum(shape))
    x = field(rng, shape, dtype, nan)
    if tag == 'none':
        x.ravel()[5:9] = [-0.0, 0.0, -0.0, 1e-3]
    mm, st = MinMaxScaler(axis=axis).fit(x), StandardScaler(axis=axis).fit(x)
    check_stats(dict(min=mm.data_min_, max=mm.data_max_, mean=st.mean_, std=st.std_), x, axis)
    assert hasattr(mm, 'nan_mask') == bool(np.isnan(x).any()) == hasattr(st, 'nan_mask')
    mask = None
    if nan:
        np.testing.assert_array_equal(mm.nan_mask, np.isnan(x))
        np.testing.assert_array_equal(st.nan_mask, np.isnan(x))
        mask = np.isnan(x)
    own = R.minmax_from(mm.data_min_, mm.data_max_)
    for k in ('scale_', 'min_', 'data_range_'):
        R.assert_bits_equal(getattr(mm, k), own[k])
    y = mm.transform(x)
    R.assert_bits_equal(y, R.minmax_transform(x, own))
    R.assert_bits_equal(mm.inverse_transform(y), R.minmax_inverse(y, own, mask))
    z = st.transform(x)
    R.assert_bits_equal(z, R.standard_transform(x, st.mean_, st.std_))
    back = st.inverse_transform(z)
    R.assert_bits_equal(back, R.standard_inverse(z, st.mean_, st.std_, nan_mask=mask))
    # round trip: four roundings at magnitudes up to max |x| (cells emptied by NaNs come back as NaN through the mask)
    np.testing.assert_array_equal(np.isnan(back), np.isnan(x))
    ok = ~np.isnan(x)
    assert np.max(np.abs(back[ok] - x[ok])) <= 8 * np.finfo(dtype).eps * np.nanmax(np.abs(x))


def test_fit_twice_gives_identical_bytes_and_partial_fit_overwrites():
    from dl4ds_amd.preprocessing import StandardScaler
    rng = np.random.default_rng(5)
    x = field(rng, (96, 200, 320), np.float32, True)
    for axis in (None, 0, (1, 2)):
        a, b = StandardScaler(axis=axis).fit(x), StandardScaler(axis=axis).fit(x)
        assert a.mean_.tobytes() == b.mean_.tobytes() and a.std_.tobytes() == b.std_.tobytes()
        assert a.nan_mask.tobytes() == b.nan_mask.tobytes()
    a.partial_fit(x[:10] * 2)
    R.assert_bits_equal(a.mean_, StandardScaler(axis=(1, 2)).fit(x[:10] * 2).mean_)


def test_copy_false_writes_into_the_callers_buffer():
    from dl4ds_amd.preprocessing import MinMaxScaler
    rng = np.random.default_rng(6)
    x = field(rng, (20, 64, 64), np.float32, True)
    sc = MinMaxScaler(copy=False, axis=None).fit(x)
    want = R.minmax_transform(x, vars(sc))
    keep = x.copy()
    y = sc.transform(x)
    assert np.shares_memory(y, x)
    R.assert_bits_equal(x, want)
    y2 = MinMaxScaler(axis=None).fit(keep).transform(keep)
    assert not np.shares_memory(y2, keep)
    R.assert_bits_equal(y2, want)


def test_device_array_in_and_out():
    from dl4ds_amd.device import DeviceArray
    from dl4ds_amd.preprocessing import MinMaxScaler, StandardScaler
    rng = np.random.default_rng(7)
    x = field(rng, (30, 64, 96), np.float32, True)
    dx = DeviceArray.from_numpy(x)
    for cls in (MinMaxScaler, StandardScaler):
        host = cls(axis=0).fit(x)
        dev = cls(axis=0).fit(dx)
        for k in ('scale_', 'min_', 'mean_', 'std_'):
            if hasattr(host, k):
                R.assert_bits_equal(getattr(dev, k), getattr(host, k))
        dy = dev.transform(dx)
        assert isinstance(dy, DeviceArray) and dy.ptr != dx.ptr and dy.shape == x.shape
        R.assert_bits_equal(dy.numpy(), host.transform(x))
        R.assert_bits_equal(dx.numpy(), x)                                   # copy=True left the input alone
        back = dev.inverse_transform(dy)
        assert isinstance(back, DeviceArray)
        R.assert_bits_equal(back.numpy(), host.inverse_transform(host.transform(x)))
        inplace = cls(axis=0, copy=False).fit(dx)
        d2 = DeviceArray.from_numpy(x)
        assert inplace.transform(d2) is d2
        R.assert_bits_equal(d2.numpy(), host.transform(x))


def test_scaler_quirks_of_the_reference():
    from dl4ds_amd.preprocessing import MinMaxScaler, StandardScaler
    rng = np.random.default_rng(8)
    x = field(rng, (12, 40, 50), np.float32, True)
    s = StandardScaler(with_mean=True, with_std=False).fit(x)
    R.assert_bits_equal(s.transform(x), np.nan_to_num(x, nan=0))              # identity + NaN fill
    R.assert_bits_equal(s.inverse_transform(x), R.standard_inverse(x, s.mean_, None, True, False, np.isnan(x)))
    with pytest.raises(AttributeError):
        StandardScaler(with_mean=False, with_std=True).fit(x).transform(x)
    with pytest.raises(IndexError):
        MinMaxScaler().fit(x).inverse_transform(x[:5])
    clean = field(rng, (12, 40, 50), np.float32, False)
    m = MinMaxScaler(axis=0).fit(clean)
    assert not hasattr(m, 'nan_mask')
    R.assert_bits_equal(m.inverse_transform(clean[:5]), R.minmax_inverse(clean[:5], vars(m)))
    const = np.full((6, 50, 70), 3.5, np.float32)
    R.assert_bits_equal(StandardScaler(axis=0).fit(const).transform(const), np.zeros_like(const))      # 0 / 0 -> fillnanto
    m.fit(x)                                                   # _reset leaves no stale attribute but the mask appears
    assert hasattr(m, 'nan_mask')
    m.fit(clean)
    assert hasattr(m, 'nan_mask')                              # ... and stays (stale), as in the reference


def test_predict_style_inverse_transform_of_nhw1():
    """what predict() and compute_metrics() do with their scaler= argument"""
    from dl4ds_amd.preprocessing import StandardScaler
    rng = np.random.default_rng(9)
    train = field(rng, (50, 64, 64), np.float32, False)
    sc = StandardScaler(axis=None).fit(train)
    assert sc.mean_.shape == (1, 1, 1)
    y = rng.standard_normal((8, 64, 64, 1)).astype(np.float32)
    out = sc.inverse_transform(y)
    assert out.shape == (8, 64, 64) and out.dtype == np.float32
    R.assert_bits_equal(out, R.standard_inverse(y, sc.mean_, sc.std_))
