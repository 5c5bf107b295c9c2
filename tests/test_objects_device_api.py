"""CPU checks of the device object labelling: tools/objects_host_check.cpp runs the kernels' five steps cell
by cell through dl4ds_amd/csrc/objects_core.h, the header the kernels take every index from, and must agree with the sequential
restatement tests/objects_ref.py on every case of tests/objects_cases.py; the exports, the header's declarations and the refusals
of label_objects / sal_scores / object_scores with the library made unreachable."""
import inspect
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests.objects_cases import CASES
from tests.objects_shared import capped, reference, same_objects

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope='module')
def host_check(tmp_path_factory):
    """the host program, built with the plain host compiler (no sanitizer, nothing preloaded)"""
    cxx = shutil.which(os.environ.get('CXX', 'c++')) or shutil.which('g++') or shutil.which('clang++')
    assert cxx, 'no host C++ compiler'
    exe = str(tmp_path_factory.mktemp('objects_host') / 'objects_host_check')
    subprocess.run([cxx, '-std=c++17', '-O1', '-Wall', '-o', exe, os.path.join(ROOT, 'tools', 'objects_host_check.cpp')], check=True)
    return exe


def run_host(exe, tmp, x, thr, connectivity, cap):
    """-> the host program's outputs in the layout of objects_ref.objects (cap None: the largest count)"""
    N, H, W, C = x.shape
    F = N * C
    case, out = os.path.join(tmp, 'case.bin'), os.path.join(tmp, 'out.bin')
    with open(case, 'wb') as f:
        f.write(np.array([N, H, W, C, connectivity, -1 if cap is None else cap], np.int32).tobytes())
        f.write(np.asarray(thr, np.float32).tobytes())
        f.write(np.ascontiguousarray(x, np.float32).tobytes())
    r = subprocess.run([exe, case, out], capture_output=True, text=True)
    assert r.returncode == 0, (r.returncode, r.stderr)
    raw = open(out, 'rb').read()
    K = int(np.frombuffer(raw, np.int32, 1)[0])
    pos, got = 4, {}
    for name, dtype, shape in (('labels', np.int32, (F, H, W)), ('count', np.int32, (F,)), ('nvalid', np.int64, (F,)),
                               ('field_sums', np.float64, (F, 3)), ('sums', np.int64, (F, K, 6)), ('bbox', np.int32, (F, K, 4)),
                               ('first', np.int32, (F, K)), ('vmax', np.float32, (F, K)), ('mass', np.float64, (F, K, 3))):
        n = int(np.prod(shape))
        got[name] = np.frombuffer(raw, dtype, n, pos).reshape(shape)
        pos += n * np.dtype(dtype).itemsize
    assert pos == len(raw)
    return got


@pytest.mark.parametrize('connectivity', [1, 2])
@pytest.mark.parametrize('name', sorted(CASES))
def test_host_program_against_restatement(host_check, tmp_path, name, connectivity):
    x, thr, full = reference(name, connectivity)
    biggest = int(full['count'].max())
    for cap in dict.fromkeys((None, 0, 1, max(biggest - 1, 0))):
        same_objects(run_host(host_check, str(tmp_path), x, thr, connectivity, cap), capped(full, cap))


def test_core_run_arithmetic_by_hand(host_check, tmp_path):
    """a row of 130 cells with runs that cross both unit boundaries (columns 60..70 and 120..129) and a threshold that is not
    finite: sum j and sum j*j of the runs in closed form against the definition; no event under a NaN threshold"""
    x = np.zeros((2, 1, 130, 1), np.float32)
    x[:, 0, 60:71, 0], x[:, 0, 120:, 0], x[:, 0, 3, 0] = 2.0, 3.0, 1.0
    got = run_host(host_check, str(tmp_path), x, np.array([0.5, np.nan], np.float32), 1, None)
    assert got['count'].tolist() == [3, 0] and got['nvalid'].tolist() == [130, 130] and not got['labels'][1].any()
    j = [np.arange(3, 4), np.arange(60, 71), np.arange(120, 130)]
    assert got['sums'][0].tolist() == [[len(a), 0, a.sum(), 0, (a * a).sum(), 0] for a in j]
    assert got['bbox'][0].tolist() == [[0, 0, a[0], a[-1]] for a in j] and got['first'][0].tolist() == [3, 60, 120]
    assert got['vmax'][0].tolist() == [1.0, 2.0, 3.0] and got['mass'][0, :, 0].tolist() == [1.0, 22.0, 30.0]


def test_exports_and_header():
    import dl4ds_amd as dds
    import dl4ds_amd._lib as L
    from dl4ds_amd import objects
    for name in ('label_objects', 'sal_scores', 'object_scores'):
        assert getattr(dds, name) is getattr(objects, name)
    assert list(inspect.signature(objects.label_objects).parameters) == \
        ['x', 'threshold', 'factor', 'connectivity', 'cap', 'batch_size', 'mask', 'return_labels']
    assert list(inspect.signature(objects.sal_scores).parameters) == \
        ['obs', 'pred', 'threshold', 'factor', 'connectivity', 'cap', 'batch_size', 'mask']
    assert inspect.signature(objects.sal_scores).parameters['factor'].default == objects.SAL_DEFAULT_FACTOR
    assert list(inspect.signature(objects.object_scores).parameters)[:4] == ['obs', 'pred', 'threshold', 'connectivity']
    protos = L.parse_header()
    assert len(protos['dl4ds_label_objects'][1]) == 17 and len(protos['dl4ds_object_thresholds'][1]) == 7


def _no_library(monkeypatch):
    import dl4ds_amd._lib as L

    def boom(*a, **k):
        raise AssertionError('the library was touched')
    monkeypatch.setattr(L, 'lib', boom)
    monkeypatch.setattr(L, 'load', boom)


X = np.random.default_rng(0).random((2, 6, 5, 1)).astype(np.float32)


@pytest.mark.parametrize('kw', [dict(), dict(threshold=0.5, factor=0.1), dict(threshold=np.nan), dict(threshold=np.inf),
                                dict(threshold=1e39), dict(threshold=(0.1, 0.2, 0.3)), dict(threshold='a'), dict(threshold=True),
                                dict(threshold=np.zeros((1, 2))), dict(factor=0.0), dict(factor=-1.0), dict(factor=np.nan),
                                dict(factor='x'), dict(threshold=0.5, connectivity=0), dict(threshold=0.5, connectivity=3),
                                dict(threshold=0.5, connectivity=1.0), dict(threshold=0.5, connectivity=True),
                                dict(threshold=0.5, cap=-1), dict(threshold=0.5, cap=1.5), dict(threshold=0.5, cap=2 ** 31),
                                dict(threshold=0.5, batch_size=0), dict(threshold=0.5, batch_size=1.5),
                                dict(threshold=0.5, mask=np.ones((3, 3), bool))])
def test_label_objects_refusals_without_a_library_call(monkeypatch, kw):
    from dl4ds_amd.objects import label_objects
    _no_library(monkeypatch)
    with pytest.raises(ValueError):
        label_objects(X, **kw)


def test_shape_and_size_refusals_without_a_library_call(monkeypatch):
    from dl4ds_amd.objects import label_objects, object_scores, sal_scores
    _no_library(monkeypatch)
    with pytest.raises(ValueError):
        label_objects(np.zeros((0, 6, 5, 1), np.float32), threshold=0.5)
    for shape, what in (((1, 2 ** 16, 2 ** 15, 1), r'2\^31'), ((1, 1, 2 ** 29, 1), r'2\^29'), ((1, 4, 2 ** 28, 1), r'2\^62')):
        big = np.lib.stride_tricks.as_strided(np.zeros(1, np.float32), shape, (0, 0, 0, 0))      # (no memory behind it)
        with pytest.raises(ValueError, match=what):
            label_objects(big, threshold=0.5)
        with pytest.raises(ValueError, match=what):
            sal_scores(big, big)
    for fn, kw in ((sal_scores, {}), (object_scores, dict(threshold=0.5))):
        with pytest.raises(ValueError, match='shape'):
            fn(X, X[:, :5], **kw)
        with pytest.raises(ValueError):
            fn(X, X, **dict(kw, connectivity=3))
    with pytest.raises(ValueError):
        sal_scores(X, X, threshold=0.5, factor=0.1)
    with pytest.raises(ValueError):
        sal_scores(X, X, factor=None)
    with pytest.raises(ValueError):
        object_scores(X, X, threshold=np.nan)
    with pytest.raises(ValueError):
        object_scores(X, X, threshold=None)


def test_mask_on_a_device_array_is_refused(monkeypatch):
    """a DeviceArray cannot take a mask: refused before any library call (the stand-in below has no buffer behind it)"""
    from dl4ds_amd.device import DeviceArray
    from dl4ds_amd.objects import label_objects, object_scores, sal_scores
    _no_library(monkeypatch)
    d = DeviceArray.__new__(DeviceArray)
    d.shape, d.dtype, d.ptr = (2, 6, 5, 1), np.dtype(np.float32), None
    m = np.ones((6, 5), bool)
    with pytest.raises(ValueError, match='mask'):
        label_objects(d, threshold=0.5, mask=m)
    with pytest.raises(ValueError, match='mask'):
        sal_scores(d, d, mask=m)
    with pytest.raises(ValueError, match='mask'):
        object_scores(d, d, threshold=0.5, mask=m)
