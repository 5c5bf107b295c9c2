"""CPU checks of the regridding kernels' arithmetic: tools/regrid_host_check.cpp, which runs the walk, the
choice of form and of the x-table's place and the summation order of dl4ds_amd/csrc/regrid_core.h lane by lane with every access
checked, against the restatement tests/regrid_ref.py, bit for bit, on every case of tests/regrid_cases.py and in both forms where
the channel count allows the 16-byte one."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests import regrid_ref
from tests.regrid_cases import CASES, reference

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope='module')
def host_check(tmp_path_factory):
    """the host program, built with the plain host compiler (no sanitizer, nothing preloaded)"""
    cxx = shutil.which(os.environ.get('CXX', 'c++')) or shutil.which('g++') or shutil.which('clang++')
    assert cxx, 'no host C++ compiler'
    exe = str(tmp_path_factory.mktemp('regrid_host') / 'regrid_host_check')
    subprocess.run([cxx, '-std=c++17', '-O1', '-Wall', '-ffp-contract=off', '-o', exe,
                    os.path.join(ROOT, 'tools', 'regrid_host_check.cpp')], check=True)
    return exe


def run_host(exe, tmp, case, form):
    x, ref = case['x'], case['ref']
    (yp, yi, yw), (xp, xi, xw), ay, ax = case['tables']
    N, H, W, C = x.shape
    Ho, Wo = ref.shape[1:3]
    kw = case['kw']
    src, out = os.path.join(tmp, 'case.bin'), os.path.join(tmp, 'out.bin')
    with open(src, 'wb') as f:
        f.write(np.array([N, H, W, C, Ho, Wo, int(kw['skipna']), form, len(yi), len(xi)], np.int32).tobytes())
        f.write(np.array([kw['min_valid']], np.float64).tobytes())
        for a, dt in ((yp, np.int32), (yi, np.int32), (xp, np.int32), (xi, np.int32), (yw, np.float64), (xw, np.float64),
                      (ay, np.float64), (ax, np.float64), (x, np.float32), (ref, np.float32)):
            f.write(np.ascontiguousarray(a, dt).tobytes())
    r = subprocess.run([exe, src, out], capture_output=True, text=True)
    assert r.returncode == 0, (r.returncode, r.stderr)
    raw = open(out, 'rb').read()
    pos, got = 0, {}
    for name, dtype, shape in (('out', np.float32, ref.shape), ('sums', np.float64, (N, C, 6)), ('counts', np.int64, (N, C, 2)),
                               ('resid', np.float32, ref.shape)):
        n = int(np.prod(shape))
        got[name] = np.frombuffer(raw, dtype, n, pos).reshape(shape)
        pos += n * np.dtype(dtype).itemsize
    assert pos == len(raw)
    return got


@pytest.mark.parametrize('name', CASES)
def test_host_program_against_restatement(host_check, tmp_path, name):
    case, ref = reference(name)
    forms = (1, 4) if case['x'].shape[3] % 4 == 0 else (1,)
    for form in forms:
        got = run_host(host_check, str(tmp_path), case, form)
        for k in ('out', 'sums', 'resid'):
            regrid_ref.same_bits(got[k], ref[k], (name, form, k))
        np.testing.assert_array_equal(got['counts'], ref['counts'])


def test_cases_reach_what_they_are_for():
    """the properties the case list promises, read from the restatement"""
    core = open(os.path.join(ROOT, 'dl4ds_amd', 'csrc', 'regrid_core.h')).read()
    assert 'RG_LDS_TAPS = 2048;' in core and 'RG_THREADS = 256;' in core
    case, _ = reference('long_taps_2400_4')
    assert len(case['tables'][1][1]) == 2400 > 2048                      # the x-taps of its one slab do not fit the stage
    case, ref = reference('wide_bilinear_520')
    assert ref['out'].shape[2] == 520 > 2 * 256                          # three slabs per row, lanes with three cells
    case, ref = reference('skipna_min_half')
    out0, out1 = reference('skipna_min0')[1]['out'], reference('skipna_min1')[1]['out']
    n0, nh, n1 = (int(np.isnan(o).sum()) for o in (out0, ref['out'], out1))
    assert 0 < n0 < nh < n1                                              # all-NaN cells; partly covered ones fall with min_valid
    assert np.isfinite(out1[~np.isnan(out1)]).all() and np.isinf(case['x']).sum() == 2
    case, ref = reference('nan_propagates')
    (yp, yi, _), (xp, xi, _), _, _ = case['tables']
    touched = np.array([[3 in yi[yp[i]:yp[i + 1]] and 4 in xi[xp[j]:xp[j + 1]] for j in range(len(xp) - 1)] for i in range(len(yp) - 1)])
    assert touched.any() and not touched.all()
    np.testing.assert_array_equal(np.isnan(ref['out'][0, :, :, 0]), touched)   # exactly the outputs whose taps touch the NaN
    for name in CASES:
        c = reference(name)[1]['counts']
        assert c[..., 0].min() > 0 and c[..., 1].sum() > 0 or name in ('cons_8x8_2x2_planar', 'long_taps_2400_4'), name
    assert reference('cons_64x96_17x23_c3')[1]['out'].shape[2] * 3 % 2 == 1     # an odd W'C
