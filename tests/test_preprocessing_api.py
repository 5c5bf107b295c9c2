"""CPU checks of dl4ds_amd.preprocessing: the signatures of MinMaxScaler / StandardScaler against the reference's
(tests/golden/reference_preprocessing_api.json), argument validation that never reaches the device, the lazy export, and the fp64
restatement the GPU tests compare with (tests/scaler_ref.py) against the recorded reference (tests/golden/reference_scalers.npz, made
by tests/golden/make_reference_scalers.py).

Bounds (tests/scaler_ref.py check_case; the same function judges the device classes in tests/test_gpu_scalers.py):
* data_min_, data_max_, nan_mask, shapes, dtypes, exception types: equal.  MinMaxScaler's scale_, min_, data_range_ and both outputs:
  bit-identical to the reference (they follow from equal min and max by numpy arithmetic in the input dtype).
* StandardScaler outputs: bit-identical to numpy's arithmetic on the scaler's own fitted attributes; NaN positions as the reference.
* mean_, std_, float32 cases: |got - ref| <= |ref - truth| + 1 ulp with truth the fp64 value -- the reference's own float32 error
  (numpy sums pairwise only along a contiguous axis), never the error of the code under test.
* float64 cases: n * eps64 * nanmean(|x|) absolute on the mean (sequential-sum bound), n * eps64 * (std + |mean|) on the std.
* the exact cases (integers 0..15): mean_ bit-identical to the reference.
"""
import inspect
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import scaler_ref as R

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
META, ARRAYS = R.load_fixture()


def test_signatures_match_the_reference():
    import dl4ds_amd.preprocessing as P
    with open(os.path.join(HERE, 'golden', 'reference_preprocessing_api.json')) as f:
        api = json.load(f)['preprocessing.py']
    assert sorted(api) == ['MinMaxScaler', 'StandardScaler']
    for cls, methods in api.items():
        for meth, spec in methods.items():
            sig = inspect.signature(getattr(getattr(P, cls), meth))
            assert list(sig.parameters) == spec['positional'], (cls, meth)
            defaults = {k: v.default for k, v in sig.parameters.items() if v.default is not inspect.Parameter.empty}
            want = {k: (tuple(v) if isinstance(v, list) else v) for k, v in spec['defaults'].items()}
            assert defaults == want, (cls, meth, defaults, want)
        for meth in ('fit_transform', 'get_params', 'set_params'):
            assert callable(getattr(getattr(P, cls), meth))


def test_get_and_set_params():
    from dl4ds_amd.preprocessing import MinMaxScaler, StandardScaler
    assert MinMaxScaler().get_params() == dict(value_range=(0, 1), copy=True, axis=None, fillnanto=-1)
    assert StandardScaler().get_params() == dict(copy=True, with_mean=True, with_std=True, axis=None, fillnanto=0)
    s = StandardScaler().set_params(axis=(1, 2), fillnanto=5)
    assert s.axis == (1, 2) and s.fillnanto == 5
    with pytest.raises(ValueError):
        s.set_params(nonsense=1)


def test_validation_never_reaches_the_device():
    from dl4ds_amd.preprocessing import MinMaxScaler, NotFittedError, StandardScaler
    assert META['bad_range/raises'] == 'ValueError'
    for bad in ((1, 1), (2, 0)):
        with pytest.raises(ValueError):
            MinMaxScaler(value_range=bad).fit(np.zeros((2, 3), np.float32))
    for cls in (MinMaxScaler, StandardScaler):
        for meth in ('transform', 'inverse_transform'):
            assert META[f'not_fitted/{cls.__name__}/{meth}_raises'] == 'NotFittedError'
            assert {'ValueError', 'AttributeError'} <= set(META[f'not_fitted/{cls.__name__}/{meth}_bases'])
            with pytest.raises(NotFittedError) as ei:
                getattr(cls(), meth)(np.zeros((2, 3), np.float32))
            assert isinstance(ei.value, ValueError) and isinstance(ei.value, AttributeError)
        for bad in ([[1.0, 2.0]], 'text', None, np.zeros((2, 3), np.int32), np.zeros((2, 3), np.float16)):
            with pytest.raises(TypeError):
                cls().fit(bad)
        assert not hasattr(cls(), 'nan_mask')
    with pytest.raises(NotFittedError):
        StandardScaler(with_mean=False, with_std=False).transform(np.zeros((2, 3), np.float32))


def test_lazy_export_does_not_load_the_library():
    code = ('import sys, dl4ds_amd\n'
            'from dl4ds_amd import StandardScaler, MinMaxScaler\n'
            'import dl4ds_amd.preprocessing as P\n'
            'assert StandardScaler is P.StandardScaler and MinMaxScaler is P.MinMaxScaler\n'
            'L = sys.modules.get("dl4ds_amd._lib")\n'
            'assert L is None or L._lib is None\n'
            'assert not any(m in sys.modules for m in ("sklearn", "scipy", "xarray"))\n')
    r = subprocess.run([sys.executable, '-c', code], cwd=ROOT, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_fixture_is_complete():
    names = META['case_names']
    assert len(names) == len(set(names)) == 59
    for cls in ('MinMaxScaler', 'StandardScaler'):
        for dt in ('float32', 'float64'):
            for nan in ('clean', 'nan'):
                for ax in ('None', '0', '12', '02', '012'):
                    assert f'{cls}_{dt}_{nan}_axis{ax}' in names
        for ax in ('None', '0', '12', '012'):
            assert f'{cls}_exact_axis{ax}' in names
    assert os.path.getsize(os.path.join(HERE, 'golden', 'reference_scalers.npz')) < 256 * 1024


@pytest.mark.parametrize('name', META['case_names'])
def test_restatement_meets_every_bound_on_the_recorded_reference(name):
    cls, kw, x, xt = R.case_setup(META, ARRAYS, name)
    make = lambda c: {'MinMaxScaler': R.RestatedMinMax, 'StandardScaler': R.RestatedStandard}[c]
    got = R.run_case(make, cls, kw, x, xt)
    if META.get(f'{name}/inverse_transform_raises') == 'IndexError':
        assert isinstance(got.get('inverse_transform_raises'), IndexError)
    R.check_case(name, META, ARRAYS, got)


def test_exact_case_is_exact():
    """the premise of the exact cases: the recorded float32 mean / min / max are the correctly rounded true values"""
    for name in META['case_names']:
        if '_exact_' not in name:
            continue
        cls, kw, x, _ = R.case_setup(META, ARRAYS, name)
        t = R.stats(x, kw['axis'])
        for attr, key in (('mean_', 'mean'), ('data_min_', 'min'), ('data_max_', 'max')):
            if f'{name}/{attr}' in ARRAYS:
                R.assert_bits_equal(ARRAYS[f'{name}/{attr}'], t[key])
