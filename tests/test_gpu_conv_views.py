"""The convolution kernels on the operand forms the graph passes -- channel slices, frame views, channel-affine read views -- and the
bias gradient of every weight-gradient family, op by op against float64 (tests/conv_view_cases.py holds the table and the references).

Per cell of the table: (1) the view's contents against the float64 reference at the conv kernels' bar (`close` of test_gpu_ops:
max abs error < 2e-4 of the reference's max magnitude), (2) bit-identity with the dense call of the same logical operands where
both report the same kernel tags, (3) every byte outside the view -- of the output buffer, of every input buffer and of the slack
behind each -- as uploaded, (4) the kernel tags of the table, (5) refusals: error status, the table's message, no launch, nothing
written, (6) weight gradients bitwise repeatable.

Measured on an MI355X (max abs error / max |reference|, the bar is 2e-4; every family ran dense, slice4, slice1, tail, frame and
frame+slice4 on each operand role, all roles at once with all 16 epilogue forms, and as a dgrad; affine forms ran where the table
says the kernel honours them and were refused everywhere else):
  forward / dgrad  direct_3_1 1.8e-7, direct_1_3 1.0e-7, direct_8_1 3.5e-7 (affine 2.6e-7), pair_8_8 4.0e-7 (affine 3.3e-7),
                   pair_5_8 3.0e-7, narrow16 4.4e-7, pair16 4.2e-7, stream 8.7e-7, stream_ws 9.5e-7, wino_24_32 4.6e-7,
                   wino_28_36 4.9e-7, split 6.2e-7, gemm 4.4e-7, point 2.0e-7, igemm3 4.4e-7, igemm5 2.5e-7, igemm7 2.5e-7,
                   stream_d2s 7.3e-7
  wgrad (dw, db)   wg_general_1 3.0e-7, wg_general_3 1.6e-7, wg_general_5 1.9e-7, wg_direct 1.1e-7, wg_direct2 1.4e-7 (affine x
                   1.4e-7), wg_narrow8 2.4e-7 (affine dz 2.4e-7), wg_two_slice 3.2e-7 (affine dz 2.2e-7), wg_rows 2.8e-7,
                   wg_wino 2.1e-7, wg_d2s 3.4e-7; attention entry (dw, db, ds) below 1e-6
Same bits as dense: EVERY view cell that reported the dense call's kernel tags was bit-identical to it, in all families, with one
tabulated exception -- wg_direct2 x:slice1, where the first-generation stencil kernel runs under the second generation's tag
(conv_view_cases: why['bits']).  No kernel wrote outside its view; no defect was found in the kernels.
Wall time of the module: 7.3 s (79 tests, the slowest 0.8 s).
"""
import numpy as np
import pytest

from tests import conv_view_cases as CV

pytestmark = pytest.mark.gpu
TOL = 2e-4


@pytest.fixture(scope='module')
def ops():
    import dl4ds_amd.ops as o
    return o


def rel_err(a, ref):
    ref = np.asarray(ref, np.float64)
    a = np.asarray(a, np.float64)
    assert a.shape == ref.shape, (a.shape, ref.shape)
    return float(np.abs(a - ref).max() / max(np.abs(ref).max(), 1e-6))


def conv_tags(tags):
    """the convolution kernels among the launched tags (not the filter transposes / slab reductions around them)"""
    return sorted(t for t in tags if t.startswith('conv_') or t.startswith('att_'))


def set_env(monkeypatch, fam):
    for k in ('DL4DS_STREAM_FORCE_WS', 'DL4DS_WINO_FORCE', 'DL4DS_SPLIT_FORCE'):
        monkeypatch.delenv(k, raising=False)
    for k, v in fam.env.items():
        monkeypatch.setenv(k, v)


def untouched(bufs, sent, form_of, cmem_of):
    """every element outside each view, and the slack behind each buffer, is bit for bit what was uploaded"""
    from dl4ds_amd.ops import slack_values
    bad = []
    for name, (after, slack) in bufs.items():
        _, inside = CV.extract(after, form_of[name], cmem_of[name])
        keep_all = name != 'y' and name != 'out'
        same = after.view(np.uint32) == sent[name].view(np.uint32)
        if not (same | (inside & (not keep_all))).all():
            bad.append(name)
        if not np.array_equal(slack.view(np.uint32), slack_values().view(np.uint32)):
            bad.append(name + '.slack')
    return bad


# ---- forward / dgrad ------------------------------------------------------------------------------------------------------------------
def fwd_forms(role, form):
    """-> {operand: placement form}, the affine form of x"""
    place = form if form in CV.PLACEMENTS else 'dense'
    forms = {r: (place if role in (r, 'all') else 'dense') for r in CV.FWD_ROLES}
    return forms, (form if form.startswith('affine') else '')


def run_fwd(ops, fam, role, form, epi):
    """One call of conv2d_views -> dict(tags, y (the view's contents), outside (names of buffers written outside the view), error)."""
    from tests.parity import kernel_tags
    from dl4ds_amd._lib import Dl4dsHipError
    forms, affine = fwd_forms(role, form)
    arole = role if affine else None
    d = CV.fwd_case(fam.name, affine if arole == 'x' else '')
    n, h, w, ci, co, ks = fam.shape
    r = fam.d2s[1] if fam.d2s else 0
    mem = dict(x=d['x'], y=d['old'], add=d['add'], mask=d['mask'])
    if r:
        from oracle import np_ops as N
        mem = {k: (np.ascontiguousarray(N.depth_to_space(v, r)) if k != 'x' else v) for k, v in mem.items()}
    views, sent, cmem = {}, {}, {}
    for k in CV.FWD_ROLES:
        buf, kw = CV.embed(mem[k], forms[k], CV.seed_of(fam.name, role, form, k))
        sent[k], cmem[k] = buf, mem[k].shape[-1]
        sc = sh = None
        if arole == k:
            sc, sh = (d['sc'], d['sh']) if k == 'x' else CV.affine_of(affine, n, co, 1)
        views[k] = ops.View(buf, C=(ci if k == 'x' else co), d2s=(r if k != 'x' else 0), sc=sc, sh=sh, **kw)
    use = dict(add=views['add'] if epi & 1 or arole == 'add' else None, mask=views['mask'] if epi & 4 or arole == 'mask' else None)
    out = dict(error=None)

    def call():
        try:
            return ops.conv2d_views(views['x'], d['w'], views['y'], b=d['b'], relu=bool(epi & 2), accumulate=bool(epi & 8), **use), None
        except Dl4dsHipError as e:
            return e.buffers, str(e)
    (bufs, out['error']), tags = kernel_tags(call)
    if out['error'] is not None:
        # nothing may have been launched or written anywhere, the output view included
        out['outside'] = [k for k, (after, slack) in bufs.items() if not np.array_equal(after.view(np.uint32), sent[k].view(np.uint32))]
        out['tags'] = sorted(tags)
        return out
    out['tags'] = conv_tags(tags)
    out['y'] = np.array(CV.extract(bufs['y'][0], forms['y'], cmem['y'])[0])
    if r:
        from oracle import np_ops as N
        out['y'] = N.space_to_depth(out['y'], r) if hasattr(N, 'space_to_depth') else _s2d(out['y'], r)
    out['outside'] = untouched(bufs, sent, forms, cmem)
    out['ref'] = CV.fwd_reference(d, epi)
    return out


def _s2d(y, r):
    n, hh, ww, cp = y.shape
    return y.reshape(n, hh // r, r, ww // r, r, cp).transpose(0, 1, 3, 2, 4, 5).reshape(n, hh // r, ww // r, r * r * cp)


def run_dgrad(ops, fam, form):
    """the family's layer backwards, dx = old + where(mask > 0, dgrad(dz, w), 0), every operand in `form`"""
    from tests.parity import kernel_tags
    d = CV.dgrad_case(fam.name)
    n, h, w, ci, co, ks = fam.shape
    mem = dict(x=d['dz'], y=d['old'], mask=d['mask'])
    views, sent, cmem, forms = {}, {}, {}, {}
    for k in mem:
        buf, kw = CV.embed(mem[k], form, CV.seed_of(fam.name, 'dgrad', form, k))
        sent[k], cmem[k], forms[k] = buf, mem[k].shape[-1], form
        views[k] = ops.View(buf, C=mem[k].shape[-1], **kw)
    bufs, tags = kernel_tags(lambda: ops.conv2d_views(views['x'], d['w'], views['y'], mask=views['mask'], accumulate=True, dgrad=True))
    return dict(tags=conv_tags(tags), y=np.array(CV.extract(bufs['y'][0], form, ci)[0]), outside=untouched(bufs, sent, forms, cmem),
                ref=d['ref'], error=None)


# ---- weight gradient ------------------------------------------------------------------------------------------------------------------
def run_wgrad(ops, fam, role, form, acc=(0, 0), want_db=True):
    from tests.parity import kernel_tags
    from dl4ds_amd._lib import Dl4dsHipError
    place = form if form in CV.PLACEMENTS else 'dense'
    affine = form if form.startswith('affine') else ''
    d = CV.wgrad_case(fam.name, role if affine else '', affine)
    n, h, w, ci, co, ks = fam.shape
    r = fam.d2s[1] if fam.d2s else 0
    mem = dict(x=d['x'], dz=d['dz'])
    views, sent, cmem, forms = {}, {}, {}, {}
    for k in mem:
        forms[k] = place if role in (k, 'all') else 'dense'
        buf, kw = CV.embed(mem[k], forms[k], CV.seed_of(fam.name, role, form, k))
        sent[k], cmem[k] = buf, mem[k].shape[-1]
        aff = dict(sc=d['sc'], sh=d['sh']) if (affine and role == k) else {}
        views[k] = ops.View(buf, C=(ci if k == 'x' else co), d2s=(r if k == 'dz' else 0), **aff, **kw)
    out = dict(error=None)
    dw0 = d['dw0'] if acc[0] else None
    db0 = d['db0'] if acc[1] else None

    def call():
        try:
            return ops.conv2d_wgrad_views(views['x'], views['dz'], ks, dw0=dw0, db0=db0, want_db=want_db), None
        except Dl4dsHipError as e:
            return (None, None, e.buffers), str(e)
    ((dw, db, bufs), out['error']), tags = kernel_tags(call)
    if out['error'] is not None:
        out['tags'] = sorted(tags)
        out['outside'] = [k for k, (after, slack) in bufs.items() if not np.array_equal(after.view(np.uint32), sent[k].view(np.uint32))]
        return out
    forms_all = dict(forms)
    out.update(tags=conv_tags(tags), all_tags=dict(tags), dw=dw, db=db, outside=[k for k, (after, slack) in bufs.items()
                                                                                 if not np.array_equal(after.view(np.uint32), sent[k].view(np.uint32))]
               + [k for k in untouched(bufs, sent, forms_all, cmem) if k.endswith('.slack')])
    out['dw_ref'] = d['dw64'] + (d['dw0'] if acc[0] else 0.0)
    out['db_ref'] = d['db64'] + (d['db0'] if acc[1] else 0.0)
    return out


# ---- the tests --------------------------------------------------------------------------------------------------------------------
FWD = [f for f in CV.FAMILIES if f.kind == 'fwd']
WG = [f for f in CV.FAMILIES if f.kind == 'wgrad']
_dense = {}


def dense_of(ops, fam, epi, runner=run_fwd):
    key = (fam.name, epi, runner.__name__)
    if key not in _dense:
        _dense[key] = runner(ops, fam, 'all', 'dense', epi)
    return _dense[key]


def expect_tags(fam, role, form, epi=None):
    kind, what = fam.outcome(role, form) if role != 'all' else ('run', fam.tag if form == 'dense' else fam.all_tag)
    if kind == 'run' and epi is not None and epi in fam.epi_tags and what == fam.tag:
        what = fam.epi_tags[epi]
    return kind, what


def check_run(got, dense, want_tag, what, bits_may_differ=False):
    assert got['error'] is None, (what, got['error'])
    assert any(t.startswith(want_tag) for t in got['tags']), (what, want_tag, got['tags'])
    assert not got['outside'], f'{what}: written outside the view: {got["outside"]}'
    err = rel_err(got['y'], got['ref'])
    assert err < TOL, f'{what}: max rel err {err:.3e}'
    if dense is not None and got['tags'] == dense['tags'] and not bits_may_differ:
        np.testing.assert_array_equal(got['y'].view(np.uint32), dense['y'].view(np.uint32), err_msg=f'{what}: bits differ from the dense call')
    return err


def check_refused(got, msg, what):
    assert got['error'] is not None and msg in got['error'], (what, msg, got['error'])
    assert got['tags'] == [] and not got['outside'], (what, got['tags'], got['outside'])


@pytest.mark.parametrize('fam', FWD, ids=lambda f: f.name)
def test_forward_cells(ops, monkeypatch, fam):
    """every (role, form) cell of a forward family with the role's epilogue (conv_view_cases.ROLE_EPI)"""
    set_env(monkeypatch, fam)
    for role, form in fam.cells():
        if form == 'dense':
            continue
        epi = CV.ROLE_EPI[role]
        kind, want = expect_tags(fam, role, form, epi)
        got = run_fwd(ops, fam, role, form, epi)
        what = f'{fam.name} {role}:{form} epi {epi}'
        if kind == 'refused':
            check_refused(got, want, what)
        else:
            dense = None if form.startswith('affine') else dense_of(ops, fam, epi)
            check_run(got, dense, want, what, (role, form) in fam.bits_differ)


@pytest.mark.parametrize('fam', FWD, ids=lambda f: f.name)
def test_forward_every_epilogue_form_on_views(ops, monkeypatch, fam):
    """all 16 (residual, ReLU, mask, accumulate) forms, dense and with every operand a frame+slice4 view: one reference per form"""
    set_env(monkeypatch, fam)
    for epi in range(16):
        kind, want = expect_tags(fam, 'all', 'dense', epi)
        dense = dense_of(ops, fam, epi)
        check_run(dense, None, want, f'{fam.name} dense epi {epi}')
        if fam.grid:
            check_run(run_fwd(ops, fam, 'all', 'frame+slice4', epi), dense, expect_tags(fam, 'all', 'frame+slice4', epi)[1],
                      f'{fam.name} all:frame+slice4 epi {epi}',
                      ('all', 'frame+slice4') in fam.bits_differ)


@pytest.mark.parametrize('fam', [f for f in FWD if f.grid], ids=lambda f: f.name)
def test_dgrad_on_views(ops, monkeypatch, fam):
    set_env(monkeypatch, fam)
    dense = run_dgrad(ops, fam, 'dense')
    check_run(dense, None, fam.dgrad_tag, f'{fam.name} dgrad dense')
    d = CV.dgrad_case(fam.name)                # the existing entry point on the same operands: the same bits
    ci, co = fam.shape[3:5]
    old = ops.conv2d_epilogue(d['dz'], np.ascontiguousarray(d['w'][::-1, ::-1].transpose(0, 1, 3, 2)), mask=d['mask'], accumulate_into=d['old'])
    np.testing.assert_array_equal(old.view(np.uint32), dense['y'].view(np.uint32))
    for form, want in (('frame+slice4', fam.dgrad_view_tag), ('slice1', fam.dgrad_slice1_tag)):
        check_run(run_dgrad(ops, fam, form), dense, want, f'{fam.name} dgrad {form}')


def check_wgrad(got, dense, want_tag, what, bits_may_differ=False):
    assert got['error'] is None, (what, got['error'])
    assert any(t.startswith(want_tag) for t in got['tags']), (what, want_tag, got['tags'])
    assert not got['outside'], f'{what}: an input buffer was written: {got["outside"]}'
    ew, eb = rel_err(got['dw'], got['dw_ref']), rel_err(got['db'], got['db_ref'])
    assert ew < TOL and eb < TOL, f'{what}: max rel err dw {ew:.3e} db {eb:.3e}'
    if dense is not None and got['tags'] == dense['tags'] and not bits_may_differ:
        np.testing.assert_array_equal(got['dw'].view(np.uint32), dense['dw'].view(np.uint32), err_msg=f'{what}: dw bits differ from the dense call')
        np.testing.assert_array_equal(got['db'].view(np.uint32), dense['db'].view(np.uint32), err_msg=f'{what}: db bits differ from the dense call')
    return ew, eb


@pytest.mark.parametrize('fam', WG, ids=lambda f: f.name)
def test_wgrad_cells(ops, monkeypatch, fam):
    set_env(monkeypatch, fam)
    dense = run_wgrad(ops, fam, 'all', 'dense')
    check_wgrad(dense, None, fam.tag, f'{fam.name} dense')
    for role, form in fam.cells():
        if form == 'dense':
            continue
        kind, want = expect_tags(fam, role, form)
        got = run_wgrad(ops, fam, role, form)
        what = f'{fam.name} {role}:{form}'
        if kind == 'refused':
            check_refused(got, want, what)
            continue
        check_wgrad(got, None if form.startswith('affine') else dense, want, what, (role, form) in fam.bits_differ)
        again = run_wgrad(ops, fam, role, form)                      # bitwise repeatable
        np.testing.assert_array_equal(got['dw'].view(np.uint32), again['dw'].view(np.uint32))
        np.testing.assert_array_equal(got['db'].view(np.uint32), again['db'].view(np.uint32))


@pytest.mark.parametrize('fam', WG, ids=lambda f: f.name)
def test_wgrad_bias_gradient_accumulate_pairs(ops, monkeypatch, fam):
    """db rides along in every family: the four (accumulate, accumulate_db) pairs on the dense and the all-roles view call, and a
    call without db whose dw must equal, bit for bit, both the call with db and the existing entry point's."""
    set_env(monkeypatch, fam)
    n, h, w, ci, co, ks = fam.shape
    base = run_wgrad(ops, fam, 'all', 'dense')
    for acc in ((0, 0), (1, 0), (0, 1), (1, 1)):
        dense = run_wgrad(ops, fam, 'all', 'dense', acc)
        check_wgrad(dense, None, fam.tag, f'{fam.name} dense acc {acc}')
        if not acc[0]:
            np.testing.assert_array_equal(dense['dw'].view(np.uint32), base['dw'].view(np.uint32))
        if not acc[1]:
            np.testing.assert_array_equal(dense['db'].view(np.uint32), base['db'].view(np.uint32))
        check_wgrad(run_wgrad(ops, fam, 'all', 'frame+slice4', acc), dense, fam.tag, f'{fam.name} all:frame+slice4 acc {acc}',
                    ('all', 'frame+slice4') in fam.bits_differ)
    nodb = run_wgrad(ops, fam, 'all', 'dense', want_db=False)
    assert nodb['db'] is None and nodb['tags'] == base['tags']
    np.testing.assert_array_equal(nodb['dw'].view(np.uint32), base['dw'].view(np.uint32))
    d = CV.wgrad_case(fam.name)
    old = ops.conv2d_wgrad(d['x'], d['dz'], ks, d2s=(fam.d2s[1] if fam.d2s else 0))
    np.testing.assert_array_equal(old.view(np.uint32), base['dw'].view(np.uint32))
    if fam.name == 'wg_two_slice':
        assert base['all_tags'].get('conv_narrow_wgrad<8>') == 2, base['all_tags']       # both slices ran; db written exactly once (checked above)


@pytest.mark.parametrize('form', ['dense', 'slice4', 'slice1', 'tail', 'frame', 'frame+slice4'])
def test_wgrad_attention(ops, form):
    """conv2d_direct_wgrad_attention (att_wgrad_per_image_kernel, att_wgrad_combine_kernel): dw, db and the attention's ds with the
    raw input in every placement form (the scale is applied by the combine kernel, so x itself carries no affine and a pitch of 13
    floats is taken too, by the first-generation stencil kernel); accumulate and accumulate_db independently; ds never accumulates."""
    from tests.parity import kernel_tags
    d = CV.attention_case()
    views, sent = {}, {}
    for k in ('x', 'dz'):
        buf, kw = CV.embed(d[k], form if k == 'x' else 'dense', CV.seed_of('attention', form, k))
        sent[k] = buf
        views[k] = ops.View(buf, C=d[k].shape[-1], **kw)
    first = None
    for acc in ((0, 0), (1, 0), (0, 1), (1, 1)):
        (dw, db, ds, ok), tags = kernel_tags(lambda: ops.conv2d_wgrad_attention(views['x'], views['dz'], d['s'], d['w'],
                                                                                dw0=d['dw0'] if acc[0] else None, db0=d['db0'] if acc[1] else None))
        assert ok and any(t.startswith('conv_direct_wgrad<3,8,1>') for t in tags), tags
        assert rel_err(dw, d['dw64'] + (d['dw0'] if acc[0] else 0.0)) < TOL
        assert rel_err(db, d['db64'] + (d['db0'] if acc[1] else 0.0)) < TOL
        assert rel_err(ds, d['ds64']) < TOL
        if first is None:
            first = ds
        np.testing.assert_array_equal(ds.view(np.uint32), first.view(np.uint32))
