"""CPU checks of dl4ds_amd/csrc/conv_route.h -- the one statement of which convolution family takes a layer -- through the host
program tools/conv_route_check.cpp (host code only: no device call, no sanitizer, nothing preloaded).  The expected side is never the
code under test:

* every cell of tests/conv_view_cases.py's outcome table (the kernel tag or refusal that tests/test_gpu_conv_views.py pins on the
  device) gives the family the route must name for the same views;
* the hand-over cases of tests/attention_cases.py: the three planner decisions of ChAttOp::on_prepare, as questions put to the routes,
  against ``expected_flags``;
* edge views whose expected routes are written out by hand from the dispatch code this header replaced (commit 0ee1293; every entry
  names the file:line of the deciding condition there);
* conv2d_wgrad_workspace_bytes against values recorded from that commit's library.
"""
import importlib.util
import os
import subprocess

import pytest

from tests import attention_cases as K
from tests import conv_view_cases as CV

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, 'dl4ds_amd')


def _hipcc():
    spec = importlib.util.spec_from_file_location('_dl4ds_csrc_build', os.path.join(PKG, 'csrc', 'build.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.HIPCC


def _build(tmp, name, extra=()):
    """conv_route.h includes common.h and with it the HIP headers: the host side of hipcc, as csrc/build.py finds it"""
    exe = str(tmp / name)
    subprocess.run([_hipcc(), '-std=c++17', '-x', 'hip', '--offload-host-only', '-O1', '-Wall', '-o', exe,
                    os.path.join(ROOT, 'tools', 'conv_route_check.cpp'), *extra], check=True)
    return exe


@pytest.fixture(scope='module')
def route_check(tmp_path_factory):
    return _build(tmp_path_factory.mktemp('conv_route'), 'conv_route_check')


def ask(exe, tmp_path, lines):
    """-> one tuple per line: ('fwd', family, refusal | None), ('wgrad', family, slabs, refusal | None), ('ws', bytes)"""
    src = tmp_path / 'calls.txt'
    src.write_text('\n'.join(lines) + '\n')
    r = subprocess.run([exe, str(src)], capture_output=True, text=True)
    assert r.returncode == 0, (r.returncode, r.stderr)
    out = []
    for ln in r.stdout.splitlines():
        f = ln.split(' ', 3 if ln.startswith('wgrad') else 2)
        if f[0] == 'fwd':
            out.append(('fwd', f[1], None if f[2] == '-' else f[2]))
        elif f[0] == 'wgrad':
            out.append(('wgrad', f[1], int(f[2]), None if f[3] == '-' else f[3]))
        else:
            out.append(('ws', int(f[1])))
    assert len(out) == len(lines), (len(out), len(lines))
    return out


def view(n, h, w, c, form='dense', d2s=0, aff=0, null=False, ld=None, off=None):
    """a view token of tools/conv_route_check.cpp for a logical (n, h, w, c) tensor placed as dl4ds_amd.ops.View places ``form``;
    ld / off: a pitch and base offset (floats) given directly"""
    r = max(d2s, 1)
    pld, coff, framed = CV.placement(form, c // (r * r))
    if ld is None:
        ld = pld
    if off is None:
        off = coff + (CV.T_PICK * h * r * w * r * ld if framed else 0)
    return f'{n},{h},{w},{c},{ld},{d2s},{"n" if null else off},{aff}'


def fwd(ks, x, y, add='-', mask='-', pool=0, bias='0'):
    return f'fwd {ks} {x} {y} {add} {mask} {pool} {bias}'


# ---- the outcome table ------------------------------------------------------------------------------------------------------------
def fwd_family_of(tag):
    if tag.startswith('conv_direct<'):
        return 'Direct'
    if tag.startswith('conv_narrow_pair_ws<'):
        return 'NarrowPair'
    if tag.startswith(('conv_narrow<', 'conv_narrow16_ws<', 'conv_narrow_pair16')):
        return 'Narrow'
    return 'Rest'                # split, wino, gemm, stream, point, igemm: the chain behind the route


FWD_REFUSALS = {CV.R_DIRECT: 'Direct', CV.R_NARROW: 'Narrow', CV.R_CONV: 'Rest'}


def wgrad_family_of(tag, cin):
    if tag.startswith('conv_direct_wgrad<'):
        return 'Direct'
    if tag.startswith('conv_narrow_wgrad<'):
        return 'NarrowSlices' if cin == 13 else 'Narrow'
    return 'General'             # (the Winograd weight gradient is a try ahead of the route)


WGRAD_REFUSALS = {CV.R_WGRAD: 'General', CV.R_DIRECT_WG: 'Direct'}


def expect_of(fam, role, form, epi=None):
    """tests/test_gpu_conv_views.py expect_tags"""
    kind, what = fam.outcome(role, form) if role != 'all' else ('run', fam.tag if form == 'dense' else fam.all_tag)
    if kind == 'run' and epi is not None and epi in fam.epi_tags and what == fam.tag:
        what = fam.epi_tags[epi]
    return kind, what


def fwd_cell_line(fam, role, form, epi):
    """the views tests/test_gpu_conv_views.py run_fwd hands to conv2d_views"""
    n, h, w, ci, co, ks = fam.shape
    place = form if form in CV.PLACEMENTS else 'dense'
    aff = {'affine_s': 1, 'affine_sh': 2}.get(form, 0)
    r = fam.d2s[1] if fam.d2s else 0
    v = {k: view(n, h, w, ci if k == 'x' else co, place if role in (k, 'all') else 'dense', d2s=(r if k != 'x' else 0),
                 aff=(aff if k == 'x' else 0)) for k in CV.FWD_ROLES}
    return fwd(ks, v['x'], v['y'], v['add'] if epi & 1 else '-', v['mask'] if epi & 4 else '-')


def fwd_table():
    rows = []                    # (what, line, family, refusal)
    for fam in (f for f in CV.FAMILIES if f.kind == 'fwd'):
        n, h, w, ci, co, ks = fam.shape
        for role, form in fam.cells():
            epi = CV.ROLE_EPI[role]
            kind, want = expect_of(fam, role, form, epi)
            if kind == 'refused' and want == CV.R_ENTRY:
                continue         # (the entry point refuses a y / add / mask descriptor with an affine before any route is asked)
            fam_want, msg = (FWD_REFUSALS[want], want) if kind == 'refused' else (fwd_family_of(want), None)
            rows.append((f'{fam.name} {role}:{form}', fwd_cell_line(fam, role, form, epi), fam_want, msg))
        for epi in range(16):
            for form in ('dense',) + (('frame+slice4',) if fam.grid else ()):
                rows.append((f'{fam.name} all:{form} epi {epi}', fwd_cell_line(fam, 'all', form, epi),
                             fwd_family_of(expect_of(fam, 'all', form, epi)[1]), None))
        if fam.grid:             # the layer backwards: dz (co channels) -> dx (ci), a ReLU mask, no bias, every operand in `form`
            for form, tag in (('dense', fam.dgrad_tag), ('frame+slice4', fam.dgrad_view_tag), ('slice1', fam.dgrad_slice1_tag)):
                rows.append((f'{fam.name} dgrad {form}', fwd(ks, view(n, h, w, co, form), view(n, h, w, ci, form), '-',
                                                             view(n, h, w, ci, form), bias='-'), fwd_family_of(tag), None))
    return rows


def wgrad_table():
    rows = []
    for fam in (f for f in CV.FAMILIES if f.kind == 'wgrad'):
        n, h, w, ci, co, ks = fam.shape
        r = fam.d2s[1] if fam.d2s else 0
        for role, form in fam.cells():
            kind, want = expect_of(fam, role, form)
            place = form if form in CV.PLACEMENTS else 'dense'
            aff = {'affine_s': 1, 'affine_sh': 2}.get(form, 0)
            x = view(n, h, w, ci, place if role in ('x', 'all') else 'dense', aff=(aff if role == 'x' else 0))
            dz = view(n, h, w, co, place if role in ('dz', 'all') else 'dense', d2s=r, aff=(aff if role == 'dz' else 0))
            fam_want, msg = (WGRAD_REFUSALS[want], want) if kind == 'refused' else (wgrad_family_of(want, ci), None)
            rows.append((f'{fam.name} {role}:{form}', f'wgrad {ks} {x} {dz}', fam_want, msg))
    return rows


def check_rows(got, rows):
    for g, (what, line, family, msg) in zip(got, rows):
        refusal = g[-1]
        assert g[1] == family, (what, line, g)
        assert (refusal is None) if msg is None else (refusal is not None and msg in refusal), (what, line, g)


def test_forward_route_names_the_family_of_every_outcome_cell(route_check, tmp_path):
    rows = fwd_table()
    assert {r[2] for r in rows} == {'Direct', 'NarrowPair', 'Narrow', 'Rest'}
    assert {r[3] for r in rows} >= {None, CV.R_DIRECT, CV.R_CONV}
    check_rows(ask(route_check, tmp_path, [r[1] for r in rows]), rows)


def test_wgrad_route_names_the_family_of_every_outcome_cell(route_check, tmp_path):
    rows = wgrad_table()
    assert {r[2] for r in rows} == {'Direct', 'Narrow', 'NarrowSlices', 'General'}
    assert {r[3] for r in rows} == {None, CV.R_WGRAD, CV.R_DIRECT_WG}
    check_rows(ask(route_check, tmp_path, [r[1] for r in rows]), rows)


# ---- the attention hand-over ------------------------------------------------------------------------------------------------------
def test_planner_decisions_on_the_handover_cases(route_check, tmp_path):
    """ChAttOp::on_prepare's three questions (tests/test_attention_cases.py pins their wording in graph.hip) on dense, aligned views"""
    lines = []
    for c in K.HANDOVER:
        b = max(c.batches)
        p_in, p_out, y = view(b, c.h, c.w, c.ci), view(b, c.h, c.w, c.c), view(b, c.h, c.w, c.co, null=True)
        lines += [fwd(3, p_in, p_out),                                                        # pool: the producer, with its bias
                  fwd(3, view(b, c.h, c.w, c.c, aff=1), y, bias='-'),                         # scale: the consumer on the affine view
                  f'wgrad 3 {p_in} {view(b, c.h, c.w, c.c, aff=2)}',                          # dx: the producer's weight gradient ...
                  fwd(3, view(b, c.h, c.w, c.c, aff=2), p_in, bias='-')]                      # ... and its dgrad
    got = ask(route_check, tmp_path, lines)
    for i, c in enumerate(K.HANDOVER):
        pool, scale, wg, dg = got[4 * i:4 * i + 4]
        flags = (c.c <= 8 and pool[1] == 'NarrowPair',
                 scale[1] == 'Direct' and scale[2] is None,
                 wg[1] == 'Narrow' and dg[2] is None and dg[1] in ('Direct', 'NarrowPair'))
        assert flags == K.expected_flags(c.ci, c.c, c.co), (c.id, flags, got[4 * i:4 * i + 4])
        if not c.no_fusion:
            assert flags == (c.pool, c.scale, c.dx), c.id


# ---- edge views, expected values by hand ------------------------------------------------------------------------------------------
# Line numbers: commit 0ee1293.  D = conv_direct.hip (eligible 825-831, affine_ok 908, conv2d_direct_forward 912-926,
# conv2d_direct_wgrad_slabs 928-933), N = conv_narrow.hip (narrow_wgrad_eligible 1746-1750, conv2d_narrow_wgrad_slabs 1754-1758,
# the pair kernel's conditions 1792-1797, conv2d_narrow_forward 1800-1827), C = conv.hip (conv2d_forward 1524-1555,
# narrow_wgrad_split_slabs 1647-1652, conv2d_wgrad 1664-1729).
def _v(c, n=2, h=16, w=16, **k):
    return view(n, h, w, c, **k)


M20 = 1 << 20
FWD_EDGES = [
    # in.C / out.C at 8 | 9 and 16 | 17
    ('8->8', fwd(3, _v(8), _v(8)), 'NarrowPair', None),                  # N:1795 holds; D:830 8 * 8 > 8
    ('9->8', fwd(3, _v(9), _v(8)), 'Narrow', None),                      # N:1795 in.C <= 8 fails; N:1806 unaligned_ok (C > 8) passes N:1807
    ('8->9', fwd(3, _v(8), _v(9)), 'Narrow', None),                      # N:1795 (out.C & 3) fails; in.vec passes N:1807
    ('16->16', fwd(3, _v(16), _v(16)), 'Narrow', None),                  # N:1802 passes, N:1795 fails
    ('17->16', fwd(3, _v(17), _v(16)), 'Rest', None),                    # N:1802 in.C > 16
    ('16->17', fwd(3, _v(16), _v(17)), 'Rest', None),                    # N:1802 out.C > 16
    # pad_pow2 products 8 | 16
    ('2->4', fwd(3, _v(2), _v(4)), 'Direct', None),                      # D:830 2 * 4 = 8
    ('3->4', fwd(3, _v(3), _v(4)), 'NarrowPair', None),                  # D:830 4 * 4 = 16; N:1795 holds (Cin % 4 != 0 is the pair kernel's)
    ('5->1', fwd(3, _v(5), _v(1)), 'Direct', None),                      # D:830 8 * 1
    ('8->1', fwd(3, _v(8), _v(1)), 'Direct', None),
    ('8->2', fwd(3, _v(8), _v(2)), 'Narrow', None),                      # D:830 8 * 2 = 16; N:1795 (out.C & 3); in.vec
    ('1->8', fwd(3, _v(1), _v(8)), 'Direct', None),
    ('1->9', fwd(3, _v(1), _v(9)), 'Rest', None),                        # D:830 1 * 16; N:1807 !in.vec, no pair, C <= 8: declined
    ('2->4 5x5', fwd(5, _v(2), _v(4)), 'Rest', None),                    # D:826, N:1802 KS != 3
    # Cout in {4, 6, 8}
    ('8->4', fwd(3, _v(8), _v(4)), 'NarrowPair', None),
    ('8->6', fwd(3, _v(8), _v(6)), 'Narrow', None),                      # N:1795 (out.C & 3)
    ('8->8 bias at +4 bytes', fwd(3, _v(8), _v(8), bias='4'), 'Narrow', None),                     # N:1796 bias & 15
    ('8->8 out at pitch 13', fwd(3, _v(8), _v(8, form='slice1')), 'Narrow', None),                 # N:1795 out.vec
    ('5->8 x at pitch 10', fwd(3, _v(5, form='slice1'), _v(8)), 'NarrowPair', None),               # N:1795 asks nothing of a plain input
    # a residual / mask in depth_to_space layout on a direct-eligible layer: D:916 steps aside after D:915 has refused
    ('2->4 add', fwd(3, _v(2), _v(4), add=_v(4)), 'Direct', None),
    ('2->4 add d2s', fwd(3, _v(2), _v(4), add=_v(4, d2s=2)), 'Rest', None),                        # D:916; N:1795 add.vec (cp = 1), N:1807 declines
    ('2->4 mask d2s', fwd(3, _v(2), _v(4), mask=_v(4, d2s=2)), 'Rest', None),
    ('4->2 add at pitch 7', fwd(3, _v(4), _v(2), add=_v(2, form='slice1')), 'Direct', None),       # (a plain add at any pitch stays)
    ('2->4 affine, add d2s', fwd(3, _v(2, aff=1), _v(4), add=_v(4, d2s=2)), 'Direct', CV.R_DIRECT),   # D:915 comes before D:916
    ('4->2 affine, add', fwd(3, _v(4, aff=1), _v(2), add=_v(2)), 'Direct', None),                  # D:908 holds on four channels
    ('out d2s', fwd(3, _v(2), _v(4, d2s=2)), 'Rest', None),                                        # D:827; N:1795 out.vec (cp = 1); N:1807
    # channel affine / pooling partials: who refuses
    ('16->16 affine', fwd(3, _v(16, aff=1), _v(16)), 'Narrow', CV.R_NARROW),                       # in.vec passes N:1807, N:1809 refuses
    ('8->8 affine_sh', fwd(3, _v(8, aff=2), _v(8)), 'NarrowPair', None),                           # N:1796 in.vec && Cin % 4 == 0
    ('5->8 affine', fwd(3, _v(5, aff=1), _v(8)), 'Rest', CV.R_CONV),                               # N:1796 fails, N:1807 declines, C:1530
    ('2->4 pool', fwd(3, _v(2), _v(4), pool=1), 'Direct', CV.R_DIRECT),                            # D:915 !ep.pool
    ('8->8 pool', fwd(3, _v(8), _v(8), pool=1), 'NarrowPair', None),
    ('16->16 pool', fwd(3, _v(16), _v(16), pool=1), 'Narrow', CV.R_NARROW),                        # N:1809
    ('13->8 pool', fwd(3, _v(13), _v(8), pool=1), 'Rest', CV.R_CONV),                              # N:1806 !ep.pool, N:1807 declines, C:1530
    ('48->48 pool', fwd(3, _v(48), _v(48), pool=1), 'Rest', CV.R_CONV),                            # C:1530
    # a tile count of 2^20 against one below, through N
    ('direct tiles 2^20 - 1', fwd(3, view(M20 - 1, 8, 32, 1), view(M20 - 1, 8, 32, 1)), 'Direct', None),     # D:829: 1 x 1 x N tiles
    ('direct tiles 2^20', fwd(3, view(M20, 8, 32, 1), view(M20, 8, 32, 1)), 'Rest', None),         # D:829; N:1794 (2N tiles), N:1807
    ('narrow tiles 2^20 - 1', fwd(3, view(M20 - 1, 32, 16, 8), view(M20 - 1, 32, 16, 8)), 'NarrowPair', None),  # N:1794: N tiles
    ('narrow tiles 2^20', fwd(3, view(M20, 32, 16, 8), view(M20, 32, 16, 8)), 'Rest', None),       # N:1794, then N:1808
    ('narrow16 tiles 2^20', fwd(3, view(M20, 32, 16, 16), view(M20, 32, 16, 16)), 'Rest', None),   # N:1808
]


def _wg(x, dz, ks=3):
    return f'wgrad {ks} {x} {dz}'


def _w(c, n=2, h=20, w=33, **k):          # direct: 2 x 3 x 2 = 12 tiles of 32 x 8; narrow: 3 x 1 x 2 = 6 tiles of 16 x 32
    return view(n, h, w, c, **k)


WGRAD_EDGES = [
    # x.C at 8 | 9 and 16 | 17 with eight outputs; dz.C at 8 | 9 and 16 | 20
    ('8->8', _wg(_w(8), _w(8)), 'Narrow', 6, None),                          # N:1748, N:1756-1757
    ('9->8', _wg(_w(9), _w(8)), 'NarrowSlices', 6, None),                    # C:1649 passes, C:1651 on the slice [0, 8)
    ('16->8', _wg(_w(16), _w(8)), 'NarrowSlices', 6, None),
    ('17->8', _wg(_w(17), _w(8)), 'General', 0, None),                       # C:1649 x.C > 16
    ('13->9', _wg(_w(13), _w(9)), 'General', 0, None),                       # C:1649 dz.C > 8
    ('13->12', _wg(_w(13), _w(12)), 'General', 0, None),
    ('8->16', _wg(_w(8), _w(16)), 'Narrow', 6, None),
    ('8->20', _wg(_w(8), _w(20)), 'General', 0, None),                       # N:1748 dz.C > 16
    ('8->8 5x5', _wg(_w(8), _w(8), 5), 'General', 0, None),                  # N:1748 KS != 3
    # pad_pow2 products 8 | 16
    ('2->4', _wg(_w(2), _w(4)), 'Direct', 12, None),                         # D:830, D:931-932
    ('3->4', _wg(_w(3), _w(4)), 'Narrow', 6, None),                          # D:830 16; N:1748 (x may have any channel count <= 8)
    ('8->2', _wg(_w(8), _w(2)), 'General', 0, None),                         # D:830 16; N:1748 !dz.vec
    # a dz slice at pitch 13
    ('8->8 dz pitch 13', _wg(_w(8), _w(8, form='slice1')), 'General', 0, None),                    # N:1748 !dz.vec
    ('8->8 dz pitch 13 at +0', _wg(_w(8), _w(8, ld=13, off=0)), 'General', 0, None),               # (the pitch alone: make_pitched_view)
    ('13->8 dz pitch 13', _wg(_w(13), _w(8, form='slice1')), 'General', 0, None),                  # C:1649 !dz.vec
    ('8->8 dz pitch 24', _wg(_w(8), _w(8, form='slice4')), 'Narrow', 6, None),
    ('8->8 x pitch 13', _wg(_w(8, form='slice1'), _w(8)), 'Narrow', 6, None),                      # N:1748: x may be unaligned
    ('8->1 dz pitch 6', _wg(_w(8), _w(1, form='slice1')), 'Direct', 12, None),                     # D:825-831 ask nothing of the pitch
    ('8->8 dz d2s', _wg(_w(8), _w(8, d2s=2)), 'General', 0, None),                                 # N:1748 dz.d2s
    # channel affines: who takes them, who refuses
    ('8->1 x affine', _wg(_w(8, aff=1), _w(1)), 'Direct', 12, None),                               # D:930 affine_ok(x)
    ('2->4 x affine', _wg(_w(2, aff=1), _w(4)), 'Direct', 12, CV.R_DIRECT_WG),                     # D:930, D:908 C < 4
    ('2->4 dz affine', _wg(_w(2), _w(4, aff=2)), 'Direct', 12, CV.R_DIRECT_WG),                    # D:930 !dz.sc
    ('8->8 dz affine', _wg(_w(8), _w(8, aff=2)), 'Narrow', 6, None),
    ('8->8 x affine', _wg(_w(8, aff=1), _w(8)), 'General', 0, CV.R_WGRAD),                         # N:1747, C:1694
    ('13->8 dz affine', _wg(_w(13), _w(8, aff=1)), 'NarrowSlices', 6, None),
    ('13->8 x affine', _wg(_w(13, aff=1), _w(8)), 'General', 0, CV.R_WGRAD),                       # C:1649 x.sc, C:1694
    ('8->20 dz affine', _wg(_w(8), _w(20, aff=1)), 'General', 0, CV.R_WGRAD),                      # C:1694
    # slab counts: min(tiles, 1024), and a tile count of 2^20 against one below
    ('direct 512 slabs', _wg(view(8, 128, 128, 8), view(8, 128, 128, 1)), 'Direct', 512, None),    # 4 x 16 x 8 tiles
    ('direct 1024 slabs', _wg(view(32, 128, 128, 8), view(32, 128, 128, 1)), 'Direct', 1024, None),   # 2048 tiles: D:932 caps
    ('narrow 256 slabs', _wg(view(8, 128, 128, 8), view(8, 128, 128, 8)), 'Narrow', 256, None),    # 8 x 4 x 8
    ('direct tiles 2^20 - 1', _wg(view(M20 - 1, 8, 32, 1), view(M20 - 1, 8, 32, 1)), 'Direct', 1024, None),   # D:829
    ('direct tiles 2^20', _wg(view(M20, 8, 32, 1), view(M20, 8, 32, 1)), 'General', 0, None),      # D:829; N:1748 !dz.vec
    ('narrow tiles 2^20 - 1', _wg(view(M20 - 1, 32, 16, 8), view(M20 - 1, 32, 16, 8)), 'Narrow', 1024, None),  # N:1749
    ('narrow tiles 2^20', _wg(view(M20, 32, 16, 8), view(M20, 32, 16, 8)), 'General', 0, None),
    ('slices tiles 2^20', _wg(view(M20, 32, 16, 13), view(M20, 32, 16, 8)), 'General', 0, None),   # C:1651 -> N:1749
]


def test_forward_route_on_edge_views(route_check, tmp_path):
    check_rows(ask(route_check, tmp_path, [e[1] for e in FWD_EDGES]), FWD_EDGES)


def test_wgrad_route_on_edge_views(route_check, tmp_path):
    got = ask(route_check, tmp_path, [e[1] for e in WGRAD_EDGES])
    check_rows(got, [(e[0], e[1], e[2], e[4]) for e in WGRAD_EDGES])
    for g, e in zip(got, WGRAD_EDGES):
        assert g[2] == e[3], (e[0], e[1], g)


# ---- workspace sizes --------------------------------------------------------------------------------------------------------------
# conv2d_wgrad_workspace_bytes of commit 0ee1293, recorded by a program linked against that commit's library (no device is needed: the
# function reads none); x on an aligned base, dz on a null pointer as the graph sizes, or the slice the call may bring.
_NULL = dict(null=True)
WORKSPACE = [
    ('direct 3->1', 3, view(2, 9, 33, 3), view(2, 9, 33, 1, **_NULL), 896),
    ('direct 8->1, 1024 slabs', 3, view(64, 512, 512, 8), view(64, 512, 512, 1, **_NULL), 299008),
    ('narrow 8->8: the general plan is larger', 3, view(2, 21, 70, 8), view(2, 21, 70, 8, **_NULL), 70080),
    ('narrow 8->16, 1024 slabs', 3, view(16, 256, 256, 8), view(16, 256, 256, 16, **_NULL), 4784128),
    ('two slices 13->8: the general plan is larger', 3, view(2, 20, 33, 13), view(2, 20, 33, 8, **_NULL), 67968),
    ('two slices 16->8, 2 x 256 slabs', 3, view(8, 128, 128, 16), view(8, 128, 128, 8, **_NULL), 2375680),
    ('narrow 8->8, dz at pitch 13', 3, view(2, 21, 70, 8), view(2, 21, 70, 8, form='slice1'), 70080),
    ('two slices 13->8, dz at pitch 13', 3, view(2, 20, 33, 13), view(2, 20, 33, 8, form='slice1'), 67968),
    ('general 1x1 8->48', 1, view(4, 64, 64, 8), view(4, 64, 64, 48, **_NULL), 221184),
    ('general 1x1 13->26', 1, view(2, 33, 17, 13), view(2, 33, 17, 26, **_NULL), 29120),
    ('general 3x3 50->40', 3, view(2, 24, 24, 50), view(2, 24, 24, 40, **_NULL), 865920),
    ('general 3x3 48->192, dz depth_to_space', 3, view(2, 34, 20, 48), view(2, 34, 20, 192, d2s=2, **_NULL), 6650880),
    ('general 5x5 6->12', 5, view(2, 16, 16, 6), view(2, 16, 16, 12, **_NULL), 28992),
    ('general 5x5 8->32', 5, view(4, 64, 64, 8), view(4, 64, 64, 32, **_NULL), 3293184),
]


def test_wgrad_workspace_bytes_are_those_of_the_dispatch_code_before(tmp_path_factory, tmp_path):
    lib = os.path.join(PKG, 'libdl4ds_hip.so')
    assert os.path.exists(lib), 'build the library first (python dl4ds_amd/csrc/build.py)'
    exe = _build(tmp_path_factory.mktemp('conv_route_ws'), 'conv_route_check_ws',
                 ['-DCONV_ROUTE_WITH_LIBRARY', '-L' + PKG, '-ldl4ds_hip', '-Wl,-rpath,' + PKG])
    lines = [f'ws {ks} {x} {dz}' for _, ks, x, dz, _ in WORKSPACE] + [f'wgrad {ks} {x} {dz}' for _, ks, x, dz, _ in WORKSPACE]
    got = ask(exe, tmp_path, lines)
    for g, (what, ks, x, dz, want) in zip(got, WORKSPACE):
        assert g == ('ws', want), (what, g, want)
    assert {g[1] for g in got[len(WORKSPACE):]} == {'Direct', 'Narrow', 'NarrowSlices', 'General'}
