"""CPU checks of conv_route.h's Pointwise family (csrc/conv_pointwise.hip) through tools/conv_route_check.cpp, beside
tests/test_conv_route.py (whose helpers build and ask the host program): the 1x1 layers of the headline configuration -- the projected
skips 8 -> 16 ... 40 -> 48 and TransitionSkip 8 -> 48 of the residual backbone at 64 x 128^2, forward and dgrad -- are the family's,
and every form its scope leaves out goes on to the kernels behind the route.  The expected side is written out from the scope stated
in conv_route.h's comment, not computed by the code under test."""
import pytest

from tests import conv_view_cases as CV
from tests.test_conv_route import _build, ask, fwd, view

B, H, W = 64, 128, 128
SKIPS = [(8, 16), (16, 24), (24, 32), (32, 40), (40, 48)]


@pytest.fixture(scope='module')
def route_check(tmp_path_factory):
    return _build(tmp_path_factory.mktemp('conv_route_pointwise'), 'conv_route_check')


def v(c, **kw):
    return view(B, H, W, c, **kw)


def test_headline_1x1_layers_are_pointwise(route_check, tmp_path):
    lines = []
    for ci, co in SKIPS:
        lines += [fwd(1, v(ci), v(co)),                                        # the projection, with its bias
                  fwd(1, v(ci), v(co), add=v(co)),                             # ... written with the block's residual added
                  fwd(1, v(co), v(ci), bias='-'),                              # its dgrad
                  fwd(1, v(co), v(ci), mask=v(ci), bias='-')]                  # ... behind a ReLU
    lines += [fwd(1, v(8), v(48)), fwd(1, v(48), v(8), bias='-')]              # TransitionSkip and its dgrad
    # channel slices of wider buffers (pitch > C, 16-byte aligned base)
    lines += [fwd(1, v(16, ld=24, off=4), v(24, ld=32, off=8)), fwd(1, v(48, ld=96, off=48), v(8), bias='-')]
    got = ask(route_check, tmp_path, lines)
    for ln, g in zip(lines, got):
        assert g == ('fwd', 'Pointwise', None), (ln, g)


def test_forms_outside_the_scope_keep_their_kernels(route_check, tmp_path):
    rows = [
        ('3x3', fwd(3, v(16), v(24)), None),
        ('Cin 26', fwd(1, v(26), v(16)), None),
        ('Cout 13', fwd(1, v(24), v(13)), None),
        ('Cin 52', fwd(1, v(52), v(16)), None),
        ('Cout 64', fwd(1, v(16), v(64)), None),
        ('depth_to_space output', fwd(1, v(16), v(32, d2s=2)), None),
        ('depth_to_space input', fwd(1, v(32, d2s=2), v(16)), None),
        ('pooling epilogue', fwd(1, v(8), v(8), pool=1), CV.R_CONV),
        ('channel-affine input', fwd(1, v(16, aff=1), v(16)), CV.R_CONV),
        ('unaligned slice', fwd(1, v(16, ld=24, off=1), v(16)), None),
        ('odd pitch', fwd(1, v(16, ld=18, off=0), v(16)), None),
        ('unaligned bias', fwd(1, v(16), v(16), bias='4'), None),
        ('residual of another width', fwd(1, v(16), v(16), add=v(24)), None),
        ('residual + mask', fwd(1, v(16), v(16), add=v(16), mask=v(16)), None),
        ('depth_to_space residual', fwd(1, v(16), v(16), add=v(16, d2s=2)), None),
    ]
    got = ask(route_check, tmp_path, [r[1] for r in rows])
    for (what, ln, msg), g in zip(rows, got):
        assert g[1] == 'Rest', (what, ln, g)
        assert (g[2] is None) if msg is None else (g[2] is not None and msg in g[2]), (what, ln, g)


def test_the_test_hooks_switch_the_family_off(route_check, tmp_path, monkeypatch):
    """DL4DS_NO_POINTWISE (the A/B comparison) and DL4DS_STREAM_FORCE_WS (which forces conv_stream_ws_kernel) are test hooks: read
    only while DL4DS_TEST_HOOKS=1"""
    import os
    import subprocess
    src = tmp_path / 'one.txt'
    src.write_text(fwd(1, v(16), v(24)) + '\n')

    def family(**env):
        e = {k: val for k, val in os.environ.items() if k not in ('DL4DS_NO_POINTWISE', 'DL4DS_STREAM_FORCE_WS', 'DL4DS_TEST_HOOKS')}
        e.update(env)
        return subprocess.run([route_check, str(src)], capture_output=True, text=True, env=e, check=True).stdout.split()[1]

    assert family() == 'Pointwise'
    assert family(DL4DS_TEST_HOOKS='1') == 'Pointwise'
    assert family(DL4DS_TEST_HOOKS='1', DL4DS_NO_POINTWISE='1') == 'Rest'
    assert family(DL4DS_TEST_HOOKS='1', DL4DS_STREAM_FORCE_WS='1') == 'Rest'
    assert family(DL4DS_NO_POINTWISE='1') == 'Pointwise'
