"""CPU checks of the metrics surface: the fp64 average-rank Spearman restatement the GPU tests compare with
(tests/spearman_ref.py) against scipy.stats.spearmanr, and the signatures of compute_rmse / compute_correlation /
compute_metrics against the reference's (tests/golden/reference_metrics_api.json, made by make_reference_metrics_api.py)."""
import inspect
import json
import os
import warnings

import numpy as np
import pytest

from tests.spearman_ref import spearman_rows

HERE = os.path.dirname(os.path.abspath(__file__))


def _cases():
    r = np.random.default_rng(7)
    yield 'ties', np.round(r.gamma(0.5, 2.0, 400), 1) * (r.random(400) > 0.6), np.round(r.gamma(0.5, 2.0, 400), 1)
    f = r.standard_normal(300)
    yield 'signed_zeros', f * (f > 0), np.round(f + 0.3 * r.standard_normal(300), 1) * (f > 0)     # -0.0 where f < 0
    yield 'zero_order', np.array([0.0, -0.0, 1.0, -0.0, 2.0]), np.array([3.0, 1.0, 2.0, 5.0, 4.0])
    yield 'constant', np.full(50, 2.5), r.standard_normal(50)
    yield 'constant_b', r.standard_normal(50), np.zeros(50)
    nan = r.standard_normal(60)
    nan[17] = np.nan
    yield 'nan', nan, r.standard_normal(60)
    yield 'L2_up', np.array([1.0, 2.0]), np.array([3.0, 5.0])
    yield 'L2_down', np.array([1.0, 2.0]), np.array([5.0, 3.0])
    yield 'L2_tied', np.array([1.0, 1.0]), np.array([5.0, 3.0])
    yield 'plain', r.standard_normal(1000), r.standard_normal(1000)


@pytest.mark.parametrize('name,a,b', list(_cases()), ids=[c[0] for c in _cases()])
def test_restatement_matches_scipy(name, a, b):
    stats = pytest.importorskip('scipy.stats')
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        want = stats.spearmanr(a, b)[0]
    got = spearman_rows(a[None], b[None])[0]
    if np.isnan(want):
        assert np.isnan(got), (name, got)
    else:
        assert abs(got - want) <= 1e-12, (name, got, want)


def test_restatement_rows_are_independent():
    stats = pytest.importorskip('scipy.stats')
    r = np.random.default_rng(3)
    a = np.round(r.standard_normal((6, 80)), 1)
    b = np.round(a + r.standard_normal((6, 80)), 1)
    a[2] = 1.0
    b[4, 5] = np.nan
    got = spearman_rows(a, b)
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        want = np.array([stats.spearmanr(a[i], b[i])[0] for i in range(6)])
    np.testing.assert_allclose(got, want, rtol=0, atol=1e-12, equal_nan=True)
    assert np.isnan(got[[2, 4]]).all() and not np.isnan(got[[0, 1, 3, 5]]).any()


def _signature(fn):
    ps = [p for p in inspect.signature(fn).parameters.values() if p.kind in (p.POSITIONAL_ONLY, p.POSITIONAL_OR_KEYWORD)]
    return [p.name for p in ps], {p.name: p.default for p in ps if p.default is not p.empty}


def test_metrics_signatures_match_the_reference():
    """compute_rmse / compute_correlation: the reference's parameters exactly; compute_metrics: the reference's parameters
    first, in order, with its defaults (this package adds ``verbose`` after them)."""
    import dl4ds_amd
    import dl4ds_amd.metrics as M
    ref = json.load(open(os.path.join(HERE, 'golden', 'reference_metrics_api.json')))['metrics.py']
    for name in ('compute_rmse', 'compute_correlation', 'compute_metrics'):
        fn = getattr(M, name)
        assert getattr(dl4ds_amd, name) is fn
        names, defaults = _signature(fn)
        want = ref[name]
        if name == 'compute_metrics':
            names = names[:len(want['positional'])]
            defaults = {k: v for k, v in defaults.items() if k in want['positional']}
        assert names == want['positional'], (name, names)
        assert defaults == want['defaults'], (name, defaults)
