"""CPU checks of the distance-map verification: the restatement tests/distance_ref.py against the definition
and against scipy on every case of tests/distance_cases.py; hand-worked scores; tools/distance_host_check.cpp, which runs the
kernels' steps cell by cell through dl4ds_amd/csrc/distance_core.h, against the restatement at three segment lengths; the exports,
the header's declaration and every refusal of distance_transform / distance_scores with the library made unreachable."""
import inspect
import math
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests import distance_ref
from tests.distance_cases import ALPHA, CASES, cutoff_of, reference

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMPTY = distance_ref.DIST_EMPTY


@pytest.mark.parametrize('name', sorted(CASES))
def test_separable_edt_is_the_brute_force_minimum_and_scipy(name):
    from scipy import ndimage
    case, ref = reference(name)
    _, A, B = distance_ref.event_sets(case['y'], case['p'], case['thresholds'])
    for ev, maps in ((A, ref['d2_obs']), (B, ref['d2_pred'])):
        for f in range(ev.shape[0]):
            for t in range(ev.shape[1]):
                np.testing.assert_array_equal(maps[f, t], distance_ref.edt_brute(ev[f, t]))
                if ev[f, t].any():
                    np.testing.assert_array_equal(maps[f, t], np.rint(ndimage.distance_transform_edt(~ev[f, t]) ** 2))
                else:
                    assert (maps[f, t] == EMPTY).all()


def test_hand_worked_scores():
    from dl4ds_amd.distance import distance_from_sums
    case, ref = reference('shifted')                                     # (the numbers: tests/distance_cases.py's docstring)
    assert ref['counts'][0, 0].tolist() == [1200, 40, 40, 6, 34, 34, 387, 387]
    res = distance_from_sums(ref['counts'], ref['sums'], case['y'].shape, case['thresholds'])
    assert res['hausdorff'][0, 0, 0] == math.sqrt(34) and res['rms_obs_to_pred'][0, 0, 0] == math.sqrt(387 / 40)
    assert res['rms_pred_to_obs'][0, 0, 0] == math.sqrt(387 / 40) and res['n_both'][0, 0, 0] == 6
    assert res['med_obs_to_pred'][0, 0, 0] == pytest.approx(res['med_pred_to_obs'][0, 0, 0], rel=1e-14)
    assert res['hausdorff_mean'].tolist() == [math.sqrt(34)]

    case, ref = reference('corners')                                     # one event against one in the opposite corner
    res = distance_from_sums(ref['counts'], ref['sums'], case['y'].shape, case['thresholds'])
    diag = math.sqrt(16 ** 2 + 22 ** 2)
    assert (res['hausdorff'] == diag).all() and (res['med_obs_to_pred'] == diag).all() and (res['rms_pred_to_obs'] == diag).all()
    assert (res['pratt'] == 1.0 / (1.0 + ALPHA * (16 ** 2 + 22 ** 2))).all() and (res['baddeley_max'] == diag).all()

    case, ref = reference('identical')                                   # identical non-empty sets: 0, 0, 0 and Pratt 1
    res = distance_from_sums(ref['counts'], ref['sums'], case['y'].shape, case['thresholds'])
    for k in ('hausdorff', 'med_obs_to_pred', 'med_pred_to_obs', 'rms_obs_to_pred', 'baddeley1', 'baddeley2', 'baddeley_max'):
        assert (res[k] == 0).all(), k
    assert (res['pratt'] == 1).all() and (res['n_both'] == res['n_obs']).all()

    case, ref = reference('empty_pred')                                  # an empty side: NaN, but Delta stays finite under the diagonal
    res = distance_from_sums(ref['counts'], ref['sums'], case['y'].shape, case['thresholds'])
    assert ref['counts'][0, 0, 4] == EMPTY and ref['counts'][0, 0, 5] == 0 and ref['sums'][0, 0, 0] == math.inf
    for k in ('hausdorff', 'med_obs_to_pred', 'med_pred_to_obs', 'rms_obs_to_pred', 'rms_pred_to_obs', 'pratt'):
        assert np.isnan(res[k]).all() and np.isnan(res[k + '_mean']).all(), k
    assert np.isfinite(res['baddeley1']).all() and (res['baddeley_max'] <= cutoff_of(case)).all() and (res['baddeley_max'] > 0).all()

    case, ref = reference('empty_both_infinite_cutoff')                  # inf - inf: NaN sums, NaN scores
    res = distance_from_sums(ref['counts'], ref['sums'], case['y'].shape, case['thresholds'])
    assert np.isnan(ref['sums'][0, 0, 4:]).all()
    assert all(np.isnan(res[k]).all() for k in ('baddeley1', 'baddeley2', 'baddeley_max'))
    case, ref = reference('empty_both')
    res = distance_from_sums(ref['counts'], ref['sums'], case['y'].shape, case['thresholds'])
    assert all((res[k] == 0).all() for k in ('baddeley1', 'baddeley2', 'baddeley_max')) and np.isnan(res['hausdorff']).all()

    case, ref = reference('one_cell')                                    # means over the fields skip NaN
    res = distance_from_sums(ref['counts'], ref['sums'], case['y'].shape, case['thresholds'])
    assert res['hausdorff'][:, 0, 0].tolist()[0] == 0 and np.isnan(res['hausdorff'][1:, 0, 0]).all()
    assert res['hausdorff_mean'].tolist() == [0.0] and res['pratt_mean'].tolist() == [1.0]
    assert res['baddeley_max'][:, 0, 0].tolist() == [0.0, 1.0, 0.0]     # (the cutoff of a one-cell field is 1)


@pytest.fixture(scope='module')
def host_check(tmp_path_factory):
    """the host program, built with the plain host compiler (no sanitizer, nothing preloaded)"""
    cxx = shutil.which(os.environ.get('CXX', 'c++')) or shutil.which('g++') or shutil.which('clang++')
    assert cxx, 'no host C++ compiler'
    exe = str(tmp_path_factory.mktemp('distance_host') / 'distance_host_check')
    subprocess.run([cxx, '-std=c++17', '-O1', '-Wall', '-ffp-contract=off', '-o', exe,
                    os.path.join(ROOT, 'tools', 'distance_host_check.cpp')], check=True)
    return exe


def run_host(exe, tmp, case, seg):
    """-> the host program's outputs in the layout of distance_ref.distance"""
    y, p, thr = case['y'], case['p'], case['thresholds']
    N, H, W, C = y.shape
    F, T = N * C, len(thr)
    src, out = os.path.join(tmp, 'case.bin'), os.path.join(tmp, 'out.bin')
    with open(src, 'wb') as f:
        f.write(np.array([N, H, W, C, T, seg], np.int32).tobytes())
        f.write(np.array([cutoff_of(case), case['alpha']], np.float64).tobytes())
        f.write(np.asarray(thr, np.float32).tobytes())
        f.write(np.ascontiguousarray(y, np.float32).tobytes())
        f.write(np.ascontiguousarray(p, np.float32).tobytes())
    r = subprocess.run([exe, src, out], capture_output=True, text=True)
    assert r.returncode == 0, (r.returncode, r.stderr)
    raw = open(out, 'rb').read()
    pos, got = 0, {}
    for name, dtype, shape in (('counts', np.int64, (F, T, 8)), ('sums', np.float64, (F, T, 7)), ('d2_obs', np.int32, (F, T, H, W)),
                               ('d2_pred', np.int32, (F, T, H, W))):
        n = int(np.prod(shape))
        got[name] = np.frombuffer(raw, dtype, n, pos).reshape(shape)
        pos += n * np.dtype(dtype).itemsize
    assert pos == len(raw)
    return got


@pytest.mark.parametrize('name', sorted(CASES))
def test_host_program_against_restatement(host_check, tmp_path, name):
    case, ref = reference(name)
    results = [run_host(host_check, str(tmp_path), case, seg) for seg in (1024, 64, 1)]
    for got in results:
        distance_ref.same(got, ref)
    for got in results[1:]:                                              # the segment length changes no bit
        assert all(got[k].tobytes() == results[0][k].tobytes() for k in got)


def test_exports_and_header():
    import dl4ds_amd as dds
    import dl4ds_amd._lib as L
    from dl4ds_amd import distance
    for name in ('distance_transform', 'distance_scores', 'distance_from_sums', 'check_distance_args'):
        assert getattr(dds, name) is getattr(distance, name)
    assert list(inspect.signature(distance.check_distance_args).parameters) == ['shape', 'thresholds', 'cutoff', 'alpha', 'batch_size']
    assert list(inspect.signature(distance.distance_from_sums).parameters) == ['counts', 'sums', 'shape', 'thresholds']
    assert list(inspect.signature(distance.distance_transform).parameters) == ['x', 'threshold', 'squared', 'batch_size', 'mask']
    sig = inspect.signature(distance.distance_scores)
    assert list(sig.parameters) == ['obs', 'pred', 'thresholds', 'cutoff', 'alpha', 'scaler', 'mask', 'batch_size', 'return_maps']
    assert sig.parameters['alpha'].default == 1 / 9 and sig.parameters['cutoff'].default is None
    assert inspect.signature(distance.distance_transform).parameters['squared'].default is True
    protos = L.parse_header()
    assert len(protos['dl4ds_distance_scores'][1]) == 14
    core = open(os.path.join(ROOT, 'dl4ds_amd', 'csrc', 'distance_core.h')).read()
    assert f'DC_DIST_EMPTY = {distance.DIST_EMPTY}' in core and distance.DIST_EMPTY == EMPTY


def test_check_distance_args_fills_in_and_casts():
    from dl4ds_amd.distance import check_distance_args
    thr, cutoff, alpha = check_distance_args((2, 4, 5, 1), [0.1, 0.05], None, 0.25, 2)
    assert thr.dtype == np.float32 and thr.tolist() == [np.float32(0.1), np.float32(0.05)] and cutoff == 5.0 and alpha == 0.25
    assert check_distance_args((1, 1, 1, 1), 0.5)[1:] == (1.0, 1 / 9)
    assert check_distance_args((1, 3, 3, 1), np.float32(2), math.inf, 1)[1:] == (math.inf, 1.0)
    assert check_distance_args((1, 46341, 1, 1), 0.0)[1] == 46340.0      # 46340^2 < 2^31 - 1


def _no_library(monkeypatch):
    import dl4ds_amd._lib as L

    def boom(*a, **k):
        raise AssertionError('the library was touched')
    monkeypatch.setattr(L, 'lib', boom)
    monkeypatch.setattr(L, 'load', boom)


X = np.random.default_rng(0).random((2, 6, 5, 1)).astype(np.float32)


@pytest.mark.parametrize('kw', [dict(thresholds=np.nan), dict(thresholds=np.inf), dict(thresholds=1e39), dict(thresholds=[]),
                                dict(thresholds='a'), dict(thresholds=True), dict(thresholds=np.zeros((2, 2))),
                                dict(thresholds=[0.5, None]), dict(cutoff=0), dict(cutoff=-1.0), dict(cutoff=np.nan),
                                dict(cutoff='x'), dict(cutoff=True), dict(alpha=0), dict(alpha=-1.0), dict(alpha=np.inf),
                                dict(alpha=np.nan), dict(alpha=None), dict(alpha='x'), dict(batch_size=0), dict(batch_size=1.5),
                                dict(mask=np.ones((3, 3), bool))])
def test_distance_scores_refusals_without_a_library_call(monkeypatch, kw):
    from dl4ds_amd.distance import distance_scores
    _no_library(monkeypatch)
    with pytest.raises(ValueError):
        distance_scores(X, X, **dict(dict(thresholds=0.5), **kw))


@pytest.mark.parametrize('kw', [dict(threshold=np.nan), dict(threshold=np.inf), dict(threshold=[0.1, 0.2]), dict(threshold='a'),
                                dict(threshold=None), dict(batch_size=0), dict(batch_size=-2), dict(mask=np.ones((3, 3), bool))])
def test_distance_transform_refusals_without_a_library_call(monkeypatch, kw):
    from dl4ds_amd.distance import distance_transform
    _no_library(monkeypatch)
    with pytest.raises(ValueError):
        distance_transform(X, **dict(dict(threshold=0.5), **kw))


def test_shape_and_size_refusals_without_a_library_call(monkeypatch):
    from dl4ds_amd.distance import check_distance_args, distance_scores, distance_transform
    _no_library(monkeypatch)
    with pytest.raises(ValueError):
        distance_transform(np.zeros((0, 6, 5, 1), np.float32), 0.5)
    with pytest.raises(ValueError, match='shape'):
        distance_scores(X, X[:, :5], 0.5)
    for shape, what in (((1, 46342, 1, 1), r'2\^31 - 1'), ((1, 1, 46342, 1), r'2\^31 - 1'), ((1, 32769, 32769, 1), r'2\^31 - 1')):
        big = np.lib.stride_tricks.as_strided(np.zeros(1, np.float32), shape, (0, 0, 0, 0))      # (no memory behind it)
        with pytest.raises(ValueError, match=what):
            distance_transform(big, 0.5)
        with pytest.raises(ValueError, match=what):
            check_distance_args(shape, 0.5)
    for shape in ((1, 4, 5), (1, 0, 5, 1), (1, 4, 5, 1, 1)):
        with pytest.raises(ValueError):
            check_distance_args(shape, 0.5)


def test_device_arrays_take_no_mask_and_no_scaler(monkeypatch):
    """refused before any library call (the stand-in below has no buffer behind it)"""
    from dl4ds_amd.device import DeviceArray
    from dl4ds_amd.distance import distance_scores, distance_transform
    _no_library(monkeypatch)
    d = DeviceArray.__new__(DeviceArray)
    d.shape, d.dtype, d.ptr = (2, 6, 5, 1), np.dtype(np.float32), None
    m = np.ones((6, 5), bool)
    with pytest.raises(ValueError, match='mask'):
        distance_transform(d, 0.5, mask=m)
    with pytest.raises(ValueError, match='mask'):
        distance_scores(d, d, 0.5, mask=m)
    with pytest.raises(ValueError, match='scaler'):
        distance_scores(d, d, 0.5, scaler=object())
    with pytest.raises(ValueError, match='both'):
        distance_scores(d, X, 0.5)
    with pytest.raises(ValueError):
        distance_scores(d, d, np.nan)
