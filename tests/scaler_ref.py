"""fp64 restatement of the reference's MinMaxScaler / StandardScaler (preprocessing.py) in this project's own words: the statistics
from ``X.astype(float64)`` with np.nanmin / nanmax / nanmean / nanstd, cast to the input dtype; the element-wise passes in the input
dtype with numpy, one separately rounded operation at a time.  The GPU tests compare against it at sizes no fixture can hold;
tests/test_preprocessing_api.py checks it against the recorded reference (tests/golden/reference_scalers.npz)."""
import warnings

import numpy as np


def stats(X, axis):
    """-> dict(min, max, mean, std) keepdims in X's dtype, plus the fp64 values under '<name>64'; X is squeezed first."""
    X = np.squeeze(X)
    X64 = X.astype(np.float64)
    out = {}
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')           # all-NaN cells: numpy warns and returns NaN
        for name, fn in (('min', np.nanmin), ('max', np.nanmax), ('mean', np.nanmean), ('std', np.nanstd)):
            v = fn(X64, axis=axis, keepdims=True)
            out[name + '64'] = v
            out[name] = v.astype(X.dtype)
    return out


def minmax_attributes(X, axis, value_range=(0, 1)):
    s = stats(X, axis)
    return minmax_from(s['min'], s['max'], value_range)


def minmax_from(data_min, data_max, value_range=(0, 1)):
    """the few host operations of MinMaxScaler.partial_fit on the statistics arrays, in their dtype"""
    with np.errstate(all='ignore'):
        data_range = data_max - data_min
        scale = data_range.copy()
        scale[scale < 10 * np.finfo(scale.dtype).eps] = 1.0
        scale_ = (value_range[1] - value_range[0]) / scale
        min_ = value_range[0] - data_min * scale_
    return dict(scale_=scale_, min_=min_, data_min_=data_min, data_max_=data_max, data_range_=data_range)


def apply(X, steps, fillnanto=None, nan_mask=None):
    """steps: sequence of (op, array) with op in '*', '+', '-', '/' applied in order, each rounded in X's dtype.  Then NaN where
    nan_mask (inverse_transform) or NaN -> fillnanto (transform)."""
    X = np.squeeze(X).copy()
    with np.errstate(all='ignore'):
        for op, a in steps:
            if a is None:
                continue
            a = np.asarray(a, X.dtype)
            if op == '*':
                X *= a
            elif op == '+':
                X += a
            elif op == '-':
                X -= a
            elif op == '/':
                X /= a
            else:
                raise ValueError(op)
    if nan_mask is not None:
        X[nan_mask] = np.nan
    if fillnanto is not None:
        X[np.isnan(X)] = fillnanto
    return X


def minmax_transform(X, attrs, fillnanto=-1):
    return apply(X, [('*', attrs['scale_']), ('+', attrs['min_'])], fillnanto=fillnanto)


def minmax_inverse(X, attrs, nan_mask=None):
    return apply(X, [('-', attrs['min_']), ('/', attrs['scale_'])], nan_mask=nan_mask)


def standard_transform(X, mean_, std_, with_std=True, fillnanto=0):
    return apply(X, [('-', mean_), ('/', std_)] if with_std else [], fillnanto=fillnanto)


def standard_inverse(X, mean_, std_, with_mean=True, with_std=True, nan_mask=None):
    return apply(X, [('*', std_ if with_std else None), ('+', mean_ if with_mean else None)], nan_mask=nan_mask)


def ulp_diff(a, b):
    """distance between equal-shaped float arrays in units in the last place of their dtype (NaN against NaN counts 0, NaN against
    a number inf)"""
    a, b = np.asarray(a), np.asarray(b)
    assert a.dtype == b.dtype and a.shape == b.shape, (a.dtype, b.dtype, a.shape, b.shape)
    with np.errstate(all='ignore'):
        ulp = np.spacing(np.maximum(np.abs(a), np.abs(b))).astype(np.float64)
        d = np.abs(a.astype(np.float64) - b.astype(np.float64)) / ulp
    d = np.where(a == b, 0.0, d)
    d = np.where(np.isnan(a) & np.isnan(b), 0.0, d)
    return np.where(np.isnan(a) != np.isnan(b), np.inf, d)


def assert_bits_equal(got, want):
    """same dtype, shape, NaN positions and bit patterns of every non-NaN value"""
    got, want = np.asarray(got), np.asarray(want)
    assert got.dtype == want.dtype and got.shape == want.shape, (got.dtype, want.dtype, got.shape, want.shape)
    np.testing.assert_array_equal(np.isnan(got), np.isnan(want))
    u = np.uint32 if got.dtype == np.float32 else np.uint64
    ok = ~np.isnan(want)
    np.testing.assert_array_equal(np.ascontiguousarray(got)[ok].view(u), np.ascontiguousarray(want)[ok].view(u))


# ------------------------------------------------------------------------------------------------ the recorded reference cases
# Shared by tests/test_preprocessing_api.py (the restatement against the record, CPU) and tests/test_gpu_scalers.py (the device
# classes against the record): one implementation of the bounds, so both are judged alike.
def load_fixture():
    import json
    import os
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'reference_scalers.npz')
    with np.load(path) as z:
        arrays = {k: z[k] for k in z.files if k != 'meta'}
        meta = json.loads(str(z['meta']))
    return meta, arrays


def case_setup(meta, arrays, name):
    kw = dict(meta[f'{name}/kwargs'])
    for k in ('axis', 'value_range'):
        if isinstance(kw.get(k), list):
            kw[k] = tuple(kw[k])
    x = arrays[meta[f'{name}/x']]
    xt = arrays[meta[f'{name}/xt']] if f'{name}/xt' in meta else x
    return meta[f'{name}/class'], kw, x, xt


def run_case(make, cls, kw, x, xt):
    """fit + transform + inverse_transform with the scaler class make(cls) -> record in the fixture's layout"""
    got = {}
    sc = make(cls)(**kw)
    sc.fit(x.copy())
    for attr in ('scale_', 'min_', 'data_min_', 'data_max_', 'data_range_', 'mean_', 'std_', 'nan_mask'):
        if hasattr(sc, attr):
            got[attr] = np.asarray(getattr(sc, attr))
    for meth in ('transform', 'inverse_transform'):
        try:
            got[meth] = np.asarray(getattr(sc, meth)(xt.copy()))
        except Exception as e:
            got[meth + '_raises'] = e
    return got


class RestatedMinMax:
    """the restatement above behind the reference's interface (what the CPU test runs through check_case)"""

    def __init__(self, value_range=(0, 1), copy=True, axis=None, fillnanto=-1):
        self.value_range, self.axis, self.fillnanto = value_range, axis, fillnanto

    def fit(self, X):
        X = np.squeeze(X)
        if np.isnan(X).any():
            self.nan_mask = np.isnan(X)
        for k, v in minmax_attributes(X, self.axis, self.value_range).items():
            setattr(self, k, v)
        return self

    def transform(self, X):
        return minmax_transform(X, vars(self), self.fillnanto)

    def inverse_transform(self, X):
        return minmax_inverse(X, vars(self), getattr(self, 'nan_mask', None))


class RestatedStandard:
    def __init__(self, copy=True, with_mean=True, with_std=True, axis=None, fillnanto=0):
        self.with_mean, self.with_std, self.axis, self.fillnanto = with_mean, with_std, axis, fillnanto

    def fit(self, X):
        X = np.squeeze(X)
        if np.isnan(X).any():
            self.nan_mask = np.isnan(X)
        s = stats(X, self.axis)
        if self.with_mean:
            self.mean_ = s['mean']
        if self.with_std:
            self.std_ = s['std']
        return self

    def _fitted(self):
        if not (hasattr(self, 'mean_') or hasattr(self, 'std_')):
            raise type('NotFittedError', (ValueError, AttributeError), {})('not fitted')

    def transform(self, X):
        self._fitted()
        if self.with_std:
            return standard_transform(X, self.mean_, self.std_, True, self.fillnanto)
        return standard_transform(X, None, None, False, self.fillnanto)

    def inverse_transform(self, X):
        self._fitted()
        return standard_inverse(X, getattr(self, 'mean_', None), getattr(self, 'std_', None), self.with_mean, self.with_std,
                                getattr(self, 'nan_mask', None))


def check_case(name, meta, arrays, got, log=print):
    """Assert a record made by run_case against the recorded reference, with the bounds of the module docstring of
    tests/test_preprocessing_api.py.  Every figure is logged before it is asserted."""
    cls, kw, x, xt = case_setup(meta, arrays, name)
    ref = {k[len(name) + 1:]: v for k, v in arrays.items() if k.startswith(name + '/')}
    exact = '_exact_' in name
    xs = np.squeeze(x)
    n = xs.size
    truth = stats(xs, kw.get('axis'))
    # the same attributes exist, with the reference's shapes and dtypes
    assert sorted(k for k in got if not k.endswith('_raises')) == sorted(ref), (sorted(got), sorted(ref))
    for k in ref:
        assert got[k].shape == ref[k].shape and got[k].dtype == ref[k].dtype, (k, got[k].shape, ref[k].shape, got[k].dtype, ref[k].dtype)
    for meth in ('transform', 'inverse_transform'):
        want = meta.get(f'{name}/{meth}_raises')
        e = got.get(meth + '_raises')
        assert (want is None) == (e is None), (meth, want, e)
        if want == 'NotFittedError':
            assert isinstance(e, ValueError) and isinstance(e, AttributeError), type(e).__mro__
        elif want is not None:
            assert type(e).__name__ == want, (meth, want, repr(e))
    if 'nan_mask' in ref:
        np.testing.assert_array_equal(got['nan_mask'], ref['nan_mask'])
    for k in ('data_min_', 'data_max_'):
        if k in ref:
            np.testing.assert_array_equal(got[k], ref[k])           # ==, NaN == NaN; -0.0 == 0.0
    with np.errstate(all='ignore'):
        for k, t in (('mean_', 'mean64'), ('std_', 'std64')):
            if k not in ref:
                continue
            g, r, t64 = got[k].astype(np.float64), ref[k].astype(np.float64), truth[t]
            np.testing.assert_array_equal(np.isnan(g), np.isnan(r))
            ok = ~np.isnan(r)
            if exact and k == 'mean_':
                log(f'{name} {k}: bit equality asked')
                assert_bits_equal(got[k], ref[k])
                continue
            if x.dtype == np.float32:
                # the reference's own float32 error (pairwise only along a contiguous axis) + 1 ulp
                bound = np.abs(r - t64) + np.spacing(np.abs(ref[k])).astype(np.float64)
            else:
                bound = n * np.finfo(np.float64).eps * np.nanmean(np.abs(xs)) * np.ones_like(r)
                if k == 'std_':
                    m = np.abs(truth['mean64'])
                    bound = n * np.finfo(np.float64).eps * (np.abs(t64) + m)       # relative on the std, times (1 + |mean| / std)
            err = np.abs(g - r)
            log(f'{name} {k}: max |got - ref| = {np.max(err[ok], initial=0.0):.3e}, smallest bound = {np.min(bound[ok], initial=np.inf):.3e}, '
                f'worst err / bound = {np.max((err / bound)[ok & (bound > 0)], initial=0.0):.3f}')
            assert np.all(err[ok] <= bound[ok]), (name, k, float(np.max((err - bound)[ok])))
    if cls == 'MinMaxScaler':
        # min and max are exact, so the host operations on them and with them every output equal the reference's bit for bit
        own = minmax_from(got['data_min_'], got['data_max_'], kw.get('value_range', (0, 1)))
        for k in ('scale_', 'min_', 'data_range_'):
            assert_bits_equal(got[k], own[k])
            assert_bits_equal(got[k], ref[k])
        for meth in ('transform', 'inverse_transform'):
            if meth in ref:
                assert_bits_equal(got[meth], ref[meth])
    else:
        # the outputs are numpy's arithmetic on the scaler's OWN fitted attributes, bit for bit
        ws, wm = kw.get('with_std', True), kw.get('with_mean', True)
        if 'transform' in ref:
            assert_bits_equal(got['transform'], standard_transform(xt, got.get('mean_'), got.get('std_'), ws, kw.get('fillnanto', 0)))
            np.testing.assert_array_equal(np.isnan(got['transform']), np.isnan(ref['transform']))
        if 'inverse_transform' in ref:
            assert_bits_equal(got['inverse_transform'],
                              standard_inverse(xt, got.get('mean_'), got.get('std_'), wm, ws, got.get('nan_mask')))
            np.testing.assert_array_equal(np.isnan(got['inverse_transform']), np.isnan(ref['inverse_transform']))
