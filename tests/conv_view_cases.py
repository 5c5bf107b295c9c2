"""Case table and float64 references of the convolution kernels on the operand forms the graph passes (not a test module).

The op tests of tests/test_gpu_ops.py hand every convolution dense, contiguous, 16-byte aligned operands.  The graph hands them
channel slices of wider buffers (Graph::view), frames of (B, T, H, W, C) buffers, per-image channel-affine read views (TView::sc /
sh) and asks every weight-gradient family for the bias gradient on the side.  This module tabulates, per kernel FAMILY (a shape
and the test hooks at which tests/test_gpu_ops.py already pins the kernel), per operand ROLE and per view FORM, what the
dispatcher does with the call -- runs it on the family's kernel, routes it to another kernel, or refuses it -- as read from the
dispatch code (the file:line of the deciding condition is in each entry's reason), and builds the inputs and references:

* one set of LOGICAL operands per family (N(0,1) data, 0.2 N(0,1) filters, fixed seed per case id), shared by every cell: a view
  form changes where the values live, not what they are, so one float64 reference per epilogue form serves all of a family's cells;
* the bytes of a wide / framed buffer outside the view are independent finite random values (zeros would hide a read at the wrong
  pitch); `embed` places a logical tensor into such a buffer, `extract` reads the view back;
* channel-affine cells have their own logical input mem * sc[n, c] + sh[n, c] (per-image values differ between images);
* ReLU kinks: an input pixel whose float64 pre-activation (with or without the residual) lies within KINK * max|v| of zero is
  redrawn from the case's own stream, looking at the reference alone, until none is left; nothing is excluded from a comparison;
* weight gradients: dz carries a per-channel offset of order one, so a lost or doubled slab moves db = sum dz visibly.
"""
import functools
import zlib

import numpy as np

from oracle import np_ops as N

KINK = 1e-4
FORMS = ('slice4', 'slice1', 'tail', 'frame', 'frame+slice4', 'affine_s', 'affine_sh')
PLACEMENTS = FORMS[:5]
FWD_ROLES = ('x', 'y', 'add', 'mask')
WG_ROLES = ('x', 'dz')
T_FRAMES, T_PICK = 3, 1

# refusal messages (substrings of dl4ds_last_error)
R_ENTRY = 'only a read operand'                               # capi.cpp desc_view: y / add / mask descriptors with sc
R_DIRECT = 'conv_direct: channel-affine input needs float4-loadable channels'       # conv_route.h conv2d_forward_route
R_NARROW = 'conv_narrow: channel-affine input / pooling partials need the pair kernel'  # conv_route.h conv2d_forward_route
R_CONV = 'conv2d: channel-affine input / pooling partials are only implemented'     # conv_route.h conv2d_forward_route
R_WGRAD = 'wgrad: channel-affine operands are only implemented'                     # conv_route.h conv2d_wgrad_route
R_DIRECT_WG = 'conv_direct wgrad: only a float4-loadable x operand may carry a channel affine'   # conv_route.h conv2d_wgrad_route


def run(tag):
    return ('run', tag)


def refused(msg):
    return ('refused', msg)


class Family:
    """kind 'fwd' | 'wgrad'; shape (N, H, W, Cin, Cout, KS); env: test hooks; tag: the kernel tag prefix of the dense call.
    outcomes: {(role, form): ('run', tag prefix) | ('refused', message)} where the dispatcher does NOT run the family's kernel,
    with `why` holding the code-level reason; every other placement cell runs on `tag`.  bits_differ: same-tag cells whose bits
    may legitimately differ from the dense call's (reason in `why['bits']`).  d2s: (role, r) -- that operand's memory is depth_to_space."""

    def __init__(self, name, kind, shape, tag, env=None, outcomes=None, why=None, bits_differ=(), d2s=None, grid=True, dgrad_tag=None,
                 epi_tags=None, dgrad_slice1_tag=None, dgrad_view_tag=None, all_tag=None):
        self.name, self.kind, self.shape, self.tag, self.env = name, kind, shape, tag, dict(env or {})
        self.outcomes, self.why, self.bits_differ, self.d2s, self.grid = dict(outcomes or {}), dict(why or {}), set(bits_differ), d2s, grid
        self.dgrad_tag, self.epi_tags = dgrad_tag or tag, dict(epi_tags or {})
        # dgrad with every operand a frame+slice4 / slice1 view; forward with every operand a frame+slice4 view
        self.dgrad_view_tag, self.dgrad_slice1_tag, self.all_tag = dgrad_view_tag or self.dgrad_tag, dgrad_slice1_tag or self.dgrad_tag, all_tag or tag

    @property
    def roles(self):
        return FWD_ROLES if self.kind == 'fwd' else WG_ROLES

    def outcome(self, role, form):
        if (role, form) in self.outcomes:
            return self.outcomes[(role, form)]
        if form.startswith('affine'):
            raise KeyError(f'{self.name}: no outcome tabulated for {(role, form)}')
        return run(self.tag)

    def cells(self):
        """-> [(role, form)]: 'dense' baseline, every role x form, and all roles at once (frame+slice4: float4 access survives)."""
        out = [('all', 'dense')]
        if self.grid:
            out += [(r, f) for r in self.roles for f in FORMS] + [('all', 'frame+slice4')]
        else:
            out += sorted(self.outcomes)
        return out



def _affine_all(fwd_msg_x):
    """forward families that take no channel affine at all: x refused by the dispatcher, y / add / mask by the entry point"""
    o = {}
    for f in ('affine_s', 'affine_sh'):
        o[('x', f)] = refused(fwd_msg_x)
        for r in ('y', 'add', 'mask'):
            o[(r, f)] = refused(R_ENTRY)
    return o


def _merge(*ds):
    out = {}
    for d in ds:
        out.update(d)
    return out


# ---- the table ----------------------------------------------------------------------------------------------------------------
# Filled from the dispatch code: conv.hip conv2d_forward / conv2d_wgrad try the families in a fixed order and each family's
# *_forward / *_ok function states what it needs of a view (vec, ld, nstride, sc).  N is at least 2 everywhere (frame and affine
# forms mean nothing on one image); the other dimensions are those of tests/test_gpu_ops.py.
FAMILIES = []


def _fam(*a, **k):
    FAMILIES.append(Family(*a, **k))


def family(name):
    return next(f for f in FAMILIES if f.name == name)


# ---- placement of a logical tensor into the buffer of a view form ------------------------------------------------------------------
def seed_of(*what):
    return zlib.crc32(repr(what).encode())


def placement(form, c_mem):
    """-> (ld, coff, framed) of a view of c_mem channels per pixel in memory"""
    base = form.replace('frame+', '')
    framed = form.startswith('frame')
    if base == 'slice4':
        return c_mem + 16, 8, framed
    if base == 'slice1':
        return c_mem + 5, 3, framed
    if base == 'tail':
        return c_mem + 8, 8, framed
    return c_mem, 0, framed            # dense, frame, affine_*


def embed(mem, form, seed):
    """mem: (N, H', W', c_mem) float32, the view's contents in memory layout -> (buffer, dict(coff=, t=)) with everything outside the
    view drawn from N(0,1) under `seed`."""
    n, h, w, c = mem.shape
    ld, coff, framed = placement(form, c)
    g = np.random.default_rng(seed)
    shape = (n, T_FRAMES, h, w, ld) if framed else (n, h, w, ld)
    buf = g.standard_normal(shape).astype(np.float32)
    if framed:
        buf[:, T_PICK, :, :, coff:coff + c] = mem
    else:
        buf[..., coff:coff + c] = mem
    return buf, dict(coff=coff, t=T_PICK if framed else None)


def extract(buf, form, c_mem):
    """-> (the view's contents, a boolean array marking the elements of `buf` that belong to the view)"""
    ld, coff, framed = placement(form, c_mem)
    inside = np.zeros(buf.shape, bool)
    if framed:
        inside[:, T_PICK, :, :, coff:coff + c_mem] = True
        return buf[:, T_PICK, :, :, coff:coff + c_mem], inside
    inside[..., coff:coff + c_mem] = True
    return buf[..., coff:coff + c_mem], inside


def affine_of(form, n, c, seed):
    """per-image channel scale (and shift): images differ, values of order one, bounded away from zero"""
    if not form.startswith('affine'):
        return None, None
    g = np.random.default_rng(seed)
    sc = (0.5 + g.random((n, c)) + 0.25 * np.arange(n)[:, None]).astype(np.float32)
    sh = (g.standard_normal((n, c)) * 0.5 + 0.3 * np.arange(n)[:, None]).astype(np.float32) if form == 'affine_sh' else None
    return sc, sh


def logical(mem, sc, sh):
    """float64 logical value of a read view: mem * sc[n, c] + sh[n, c] (plain: mem)"""
    x = mem.astype(np.float64)
    if sc is not None:
        x = x * sc.astype(np.float64)[:, None, None, :]
    if sh is not None:
        x = x + sh.astype(np.float64)[:, None, None, :]
    return x


# ---- forward ----------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def fwd_case(name, affine=''):
    """Logical operands of a forward family (float32 dicts) and the float64 convolution conv64 = conv(x) + b; `affine`: '' |
    'affine_s' | 'affine_sh' (x read as mem * sc + sh).  Inputs are redrawn until no ReLU argument sits on its kink."""
    fam = family(name)
    n, h, w, ci, co, ks = fam.shape
    g = np.random.default_rng(seed_of(name, affine))
    d = dict(x=g.standard_normal((n, h, w, ci)).astype(np.float32), w=(g.standard_normal((ks, ks, ci, co)) * 0.2).astype(np.float32),
             b=g.standard_normal(co).astype(np.float32), add=g.standard_normal((n, h, w, co)).astype(np.float32),
             mask=g.standard_normal((n, h, w, co)).astype(np.float32), old=g.standard_normal((n, h, w, co)).astype(np.float32))
    d['sc'], d['sh'] = affine_of(affine, n, ci, seed_of(name, affine, 'sc'))
    w64, b64 = d['w'].astype(np.float64), d['b'].astype(np.float64)
    for rounds in range(60):
        conv = N.conv2d(logical(d['x'], d['sc'], d['sh']), w64, b64)
        bad = kink_offenders(conv, d['add'])
        if not bad.any():
            break
        px = bad.any(axis=-1)                                   # (n, h, w): redraw the centre input pixel and the residual there
        d['x'][px] = g.standard_normal((int(px.sum()), ci)).astype(np.float32)
        d['add'][px] = g.standard_normal((int(px.sum()), co)).astype(np.float32)
    else:
        raise AssertionError(f'{name}: pre-activations on the kink after 60 rounds')
    d['conv64'], d['rounds'] = conv, rounds
    for v in d.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return d


def kink_offenders(conv, add):
    """elements whose ReLU argument -- without or with the residual -- lies within KINK * max|v| of zero"""
    v1 = conv + add.astype(np.float64)
    return (np.abs(conv) < KINK * np.abs(conv).max()) | (np.abs(v1) < KINK * np.abs(v1).max())


def fwd_reference(d, epi):
    """epi: bit 0 residual, 1 ReLU, 2 mask, 3 accumulate -> y = [old +] where(mask > 0, [relu](conv + b + add), 0) in float64"""
    v = d['conv64']
    if epi & 1:
        v = v + d['add'].astype(np.float64)
    if epi & 2:
        v = np.maximum(v, 0.0)
    if epi & 4:
        v = np.where(d['mask'] > 0, v, 0.0)
    if epi & 8:
        v = v + d['old'].astype(np.float64)
    return v


@functools.lru_cache(maxsize=None)
def dgrad_case(name):
    """The family's layer run backwards: dz (N, H, W, Cout) -> dx (N, H, W, Cin) = dgrad(dz, w), in the graph's form
    dx = old + where(mask > 0, dgrad, 0) (epilogue 12: the ReLU backward of the layer below and gradient accumulation)."""
    import torch
    from oracle import torch_ops as T
    fam = family(name)
    n, h, w, ci, co, ks = fam.shape
    g = np.random.default_rng(seed_of(name, 'dgrad'))
    d = dict(dz=g.standard_normal((n, h, w, co)).astype(np.float32), w=(g.standard_normal((ks, ks, ci, co)) * 0.2).astype(np.float32),
             mask=g.standard_normal((n, h, w, ci)).astype(np.float32), old=g.standard_normal((n, h, w, ci)).astype(np.float32))
    xt = torch.zeros((n, h, w, ci), dtype=torch.float64, requires_grad=True)
    (T.conv2d(xt, torch.tensor(d['w'], dtype=torch.float64)) * torch.tensor(d['dz'], dtype=torch.float64)).sum().backward()
    d['ref'] = np.where(d['mask'] > 0, xt.grad.numpy(), 0.0) + d['old'].astype(np.float64)
    return d


# ---- weight gradient ----------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def wgrad_case(name, affine_role='', affine=''):
    """-> dict(x, dz (memory layout when the family reads dz through depth_to_space), sc, sh, dw0, db0, dw64, db64).  dz carries a
    per-channel offset of order one."""
    import torch
    from oracle import torch_ops as T
    fam = family(name)
    n, h, w, ci, co, ks = fam.shape
    g = np.random.default_rng(seed_of(name, affine_role, affine))
    off = (1.0 + 0.5 * np.cos(np.arange(co))) * np.where(np.arange(co) % 2, -1.0, 1.0)
    d = dict(x=g.standard_normal((n, h, w, ci)).astype(np.float32), dz=(g.standard_normal((n, h, w, co)) + off).astype(np.float32),
             dw0=g.standard_normal((ks, ks, ci, co)).astype(np.float32), db0=g.standard_normal(co).astype(np.float32))
    c_aff = ci if affine_role == 'x' else co
    d['sc'], d['sh'] = affine_of(affine, n, c_aff, seed_of(name, affine_role, affine, 'sc'))
    x64 = logical(d['x'], *((d['sc'], d['sh']) if affine_role == 'x' else (None, None)))
    dz64 = logical(d['dz'], *((d['sc'], d['sh']) if affine_role == 'dz' else (None, None)))
    xt = torch.tensor(x64, requires_grad=False)
    wt = torch.zeros((ks, ks, ci, co), dtype=torch.float64, requires_grad=True)
    (T.conv2d(xt, wt) * torch.tensor(dz64)).sum().backward()
    d['dw64'], d['db64'] = wt.grad.numpy(), dz64.sum(axis=(0, 1, 2))
    if fam.d2s:                                   # dz lives in depth_to_space layout: (N, H*r, W*r, Cout / r^2)
        d['dz'] = np.ascontiguousarray(N.depth_to_space(d['dz'], fam.d2s[1]))
    for v in d.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return d


@functools.lru_cache(maxsize=None)
def attention_case(n=3, h=19, w=45, ci=8, co=1):
    """conv2d_direct_wgrad_attention: y = conv(x * s[n, ci]); -> dw = wgrad(x * s, dz), db = sum dz, ds[n, ci] = sum_p x * dgrad(dz)"""
    import torch
    from oracle import torch_ops as T
    g = np.random.default_rng(seed_of('attention', n, h, w, ci, co))
    d = dict(x=g.standard_normal((n, h, w, ci)).astype(np.float32), dz=(g.standard_normal((n, h, w, co)) + 1.0).astype(np.float32),
             w=(g.standard_normal((3, 3, ci, co)) * 0.2).astype(np.float32), s=(0.25 + g.random((n, ci))).astype(np.float32),
             dw0=g.standard_normal((3, 3, ci, co)).astype(np.float32), db0=g.standard_normal(co).astype(np.float32))
    st = torch.tensor(d['s'].astype(np.float64), requires_grad=True)
    wt = torch.tensor(d['w'].astype(np.float64), requires_grad=True)
    xs = torch.tensor(d['x'].astype(np.float64)) * st[:, None, None, :]
    (T.conv2d(xs, wt) * torch.tensor(d['dz'].astype(np.float64))).sum().backward()
    d['dw64'], d['ds64'], d['db64'] = wt.grad.numpy(), st.grad.numpy(), d['dz'].astype(np.float64).sum(axis=(0, 1, 2))
    return d


# ---- the families -----------------------------------------------------------------------------------------------------------------
# Epilogue of a role cell: the operand under test must be read / written -- x: residual + ReLU (3), y: the same accumulated into the
# view's old contents (11), add: 3, mask: ReLU mask + accumulate (12, the dgrad form).  The 16-form sweep runs on the 'all roles' cell.
ROLE_EPI = {'x': 3, 'y': 11, 'add': 3, 'mask': 12, 'all': 15}
IGEMM = 'conv_igemm<'
OUT_SIDE = ('y', 'add', 'mask')
PITCHED = ('slice4', 'slice1', 'tail', 'frame+slice4')            # forms whose pixel pitch differs from the dense operands'


def _cells(roles, forms, outcome):
    return {(r, f): outcome for r in roles for f in forms}


_fam('direct_3_1', 'fwd', (2, 9, 33, 3, 1, 3), 'conv_direct<3,4,1>', outcomes=_affine_all(R_DIRECT), dgrad_tag='conv_direct<3,1,4>',
     why={'affine': 'conv_route.h affine_ok (conv2d_forward_route requires it): Cin = 3 is not float4-loadable'})
_fam('direct_1_3', 'fwd', (2, 8, 32, 1, 3, 3), 'conv_direct<3,1,4>', outcomes=_affine_all(R_DIRECT), dgrad_tag='conv_direct<3,4,1>',
     why={'affine': 'conv_route.h affine_ok: Cin = 1 is not float4-loadable'})
# (not in test_gpu_ops' CONV_CASES as a forward shape: test_conv2d_fused_epilogues_stencil_path's 8 -> 1 grid, the one stencil
# shape whose input a channel affine can ride on)
_fam('direct_8_1', 'fwd', (2, 19, 45, 8, 1, 3), 'conv_direct<3,8,1>', dgrad_tag='conv_direct<3,1,8>',
     outcomes=_merge(_affine_all(R_DIRECT), _cells('x', ('affine_s', 'affine_sh'), run('conv_direct<3,8,1>'))),
     why={'affine': 'conv_route.h affine_ok holds (Cin = 8, float4-loadable): conv_direct_kernel / conv_direct2_kernel apply sc / sh'})
_fam('pair_8_8', 'fwd', (2, 21, 70, 8, 8, 3), 'conv_narrow_pair_ws<', dgrad_slice1_tag=IGEMM,
     outcomes=_merge(_affine_all(R_CONV), _cells('x', ('affine_s', 'affine_sh'), run('conv_narrow_pair_ws<')),
                     _cells(OUT_SIDE, ('slice1',), run('conv_narrow<8>'))),
     why={'affine': 'conv_route.h narrow_pair_ok / conv_narrow.hip narrow_pair_ws_ok: float4-loadable input with Cin % 4 == 0 -> PAIR_EPI_AFF forms',
          'slice1': 'conv_route.h narrow_pair_ok: out / add / mask must be float4-accessible -> conv_narrow_kernel<8>; as a '
                    'dgrad with every operand at that pitch the input is not float4-loadable either and the narrow path declines'})
_fam('pair_5_8', 'fwd', (2, 21, 70, 5, 8, 3), 'conv_narrow_pair_ws<', dgrad_tag='conv_narrow16_ws<', dgrad_slice1_tag=IGEMM,
     outcomes=_merge(_affine_all(R_CONV), _cells(OUT_SIDE, ('slice1',), run(IGEMM))),
     why={'affine': 'conv_route.h narrow_pair_ok: sc needs Cin % 4 == 0; conv2d_forward_route then passes the narrow family by (no float4 input, '
                    'not the pair kernel) and refuses',
          'slice1': 'conv_route.h conv2d_forward_route: !in.vec && !pair && Cin <= 8 -> not the narrow family; no other family takes 5 channels'})
_fam('narrow16', 'fwd', (2, 17, 16, 15, 16, 3), 'conv_narrow16_ws<',
     outcomes=_merge(_affine_all(R_CONV), _cells(OUT_SIDE, PITCHED, run('conv_narrow<16>'))),
     why={'affine': 'conv_narrow.hip narrow16_ws_ok / conv_route.h conv2d_forward_route: no channel affine outside the pair kernel',
          'pitched': 'conv_narrow.hip narrow16_ws_ok: add and mask must share the output\'s layout (same_layout); with ONE of the three '
                     'at another pitch the older conv_narrow_kernel<16> runs.  All three at one pitch (the all-roles cell) stay.'})
_fam('pair16', 'fwd', (2, 20, 33, 13, 8, 3), 'conv_narrow_pair16_ws<', dgrad_tag='conv_narrow16_ws<', dgrad_slice1_tag=IGEMM,
     outcomes=_merge(_affine_all(R_CONV), _cells(OUT_SIDE, ('slice1',), run('conv_narrow<16>'))),
     why={'affine': 'conv_narrow.hip launch_narrow_pair16: p.in.sc declines', 'slice1': 'conv_narrow.hip launch_narrow_pair16: out / add / mask need vec'})
_VEC = {'slice1': 'the family needs float4 access on every operand (its *_forward checks in.vec, out.vec, add.vec, mask.vec): conv_igemm'}
_fam('stream', 'fwd', (2, 16, 16, 48, 48, 3), 'conv_stream<', dgrad_slice1_tag=IGEMM,
     outcomes=_merge(_affine_all(R_CONV), _cells(FWD_ROLES, ('slice1',), run(IGEMM))), why=dict(_VEC, affine='conv.hip conv2d_forward'))
_fam('stream_ws', 'fwd', (2, 33, 20, 48, 48, 3), 'conv_stream_ws<', env={'DL4DS_STREAM_FORCE_WS': '1'}, dgrad_slice1_tag=IGEMM,
     outcomes=_merge(_affine_all(R_CONV), _cells(OUT_SIDE, PITCHED, run('conv_stream<')), _cells(FWD_ROLES, ('slice1',), run(IGEMM))),
     why=dict(_VEC, affine='conv.hip conv2d_forward',
              pitched='conv_stream.hip (producer / consumer form): add / mask must share the output\'s layout (same_layout) -> conv_stream_kernel'))
_WINO_EPI = {e: 'conv_stream<' for e in (5, 7, 9, 11, 13, 15)}      # conv_wino.hip: a residual together with a mask or an accumulation is declined
_WINO_OUT = _merge(_affine_all(R_CONV), _cells(('add', 'mask'), PITCHED, run('conv_stream<')), _cells(FWD_ROLES, ('slice1',), run(IGEMM)))
_WINO_WHY = dict(_VEC, affine='conv.hip conv2d_forward', pitched='conv_wino.hip conv2d_wino_forward like_out: add / mask must share the output\'s layout')
_fam('wino_24_32', 'fwd', (2, 17, 19, 24, 32, 3), 'conv_wino<', env={'DL4DS_WINO_FORCE': 'all'}, outcomes=_WINO_OUT, why=_WINO_WHY,
     epi_tags=_WINO_EPI, dgrad_slice1_tag=IGEMM)
_fam('wino_28_36', 'fwd', (2, 16, 16, 28, 36, 3), 'conv_wino<', env={'DL4DS_WINO_FORCE': 'all'}, outcomes=_WINO_OUT, why=_WINO_WHY,
     epi_tags=_WINO_EPI, dgrad_slice1_tag=IGEMM)
_fam('split', 'fwd', (2, 40, 33, 48, 48, 3), 'conv_split<3,3>', env={'DL4DS_SPLIT_FORCE': 'all'}, dgrad_slice1_tag=IGEMM,
     outcomes=_merge(_affine_all(R_CONV), _cells(FWD_ROLES, ('slice1',), run(IGEMM))), why=dict(_VEC, affine='conv_split.hip / conv.hip'))
_fam('gemm', 'fwd', (5, 7, 9, 80, 68, 3), 'conv_gemm<3>', dgrad_tag=IGEMM,         # (dgrad: 68 input channels, not a multiple of 16)
     outcomes=_merge(_affine_all(R_CONV), _cells('x', ('slice1',), run(IGEMM))),
     why={'slice1': 'conv_gemm.hip conv2d_gemm_forward: !in.vec declines (the output side is stored channel-wise)', 'affine': 'conv.hip'})
_fam('point', 'fwd', (2, 33, 17, 13, 26, 1), 'conv_point', dgrad_slice1_tag=IGEMM, dgrad_view_tag=IGEMM, all_tag=IGEMM,
     outcomes=_merge(_affine_all(R_CONV), _cells(OUT_SIDE, PLACEMENTS, run(IGEMM)),
                     _cells('x', ('slice4', 'slice1', 'frame', 'frame+slice4'), run(IGEMM))),
     why={'placed': 'conv_point.hip: out / add / mask must be plain (ld == C, contiguous images, 16-byte base); the input may be a '
                    'slice with contiguous images, a 16-byte aligned base and ld <= 24 (tail: 21), not a frame view',
          'affine': 'conv_point.hip !in.sc, conv.hip conv2d_forward'})
_fam('igemm3', 'fwd', (2, 24, 24, 50, 40, 3), 'conv_igemm<3,', outcomes=_affine_all(R_CONV), why={'affine': 'conv.hip conv2d_forward'})
_fam('igemm5', 'fwd', (2, 16, 16, 6, 12, 5), 'conv_igemm<5,', outcomes=_affine_all(R_CONV), why={'affine': 'conv.hip conv2d_forward'})
_fam('igemm7', 'fwd', (2, 13, 19, 2, 8, 7), 'conv_igemm<7,', outcomes=_affine_all(R_CONV), why={'affine': 'conv.hip conv2d_forward'})
# supplementary (not a grid family): the output stored through depth_to_space with the input a channel slice
_fam('stream_d2s', 'fwd', (2, 16, 18, 48, 192, 3), 'conv_stream<', d2s=('y', 2), grid=False, outcomes={('x', 'slice4'): run('conv_stream<')})


def _wg_affine(x, dz):
    return _merge(_cells('x', ('affine_s', 'affine_sh'), x), _cells(('dz',), ('affine_s', 'affine_sh'), dz))


_WG_NONE = _wg_affine(refused(R_WGRAD), refused(R_WGRAD))
_WG_WHY = {'affine': 'conv.hip conv2d_wgrad: only the direct (x) and narrow (dz) kernels take a channel affine'}
# 128 slabs of 432 values: reduce_slabs_kernel<4>; the others below: reduce_slabs_kernel<16>
_fam('wg_general_1', 'wgrad', (4, 64, 64, 8, 48, 1), 'conv_wgrad_rows<1,', outcomes=_WG_NONE, why=_WG_WHY)
_fam('wg_general_3', 'wgrad', (2, 24, 24, 50, 40, 3), 'conv_wgrad_rows<3,3,', outcomes=_WG_NONE, why=_WG_WHY)
_fam('wg_general_5', 'wgrad', (2, 16, 16, 6, 12, 5), 'conv_wgrad_rows<5,', outcomes=_WG_NONE, why=_WG_WHY)
_fam('wg_direct', 'wgrad', (2, 9, 33, 3, 1, 3), 'conv_direct_wgrad<3,4,1>', outcomes=_wg_affine(refused(R_DIRECT_WG), refused(R_DIRECT_WG)),
     why={'affine': 'conv_route.h conv2d_wgrad_route: affine_ok(x) fails on Cin = 3; dz never takes one'})
_fam('wg_direct2', 'wgrad', (2, 19, 45, 8, 1, 3), 'conv_direct_wgrad<3,8,1>', bits_differ=[('x', 'slice1')],
     outcomes=_wg_affine(run('conv_direct_wgrad<3,8,1>'), refused(R_DIRECT_WG)),
     why={'affine': 'conv_route.h conv2d_wgrad_route: a float4-loadable x may carry one, dz never',
          'bits': 'conv_direct.hip direct2_ok: Cin >= 4 needs in.vec, so x at a pitch of 13 floats runs conv_direct_wgrad_kernel (first '
                  'generation, other tile height and summation order) under the SAME tag as conv_direct2_wgrad_kernel'})
_fam('wg_narrow8', 'wgrad', (2, 21, 70, 8, 8, 3), 'conv_narrow_wgrad<8>',
     outcomes=_merge(_wg_affine(refused(R_WGRAD), run('conv_narrow_wgrad<8>')), {('dz', 'slice1'): run('conv_wgrad_rows<3,1,')}),
     why={'affine': 'conv_route.h narrow_wgrad_eligible: x.sc declines, dz.sc is applied in the staging loads',
          'slice1': 'conv_route.h narrow_wgrad_eligible: !dz.vec declines -> the general kernel'})
_fam('wg_two_slice', 'wgrad', (2, 20, 33, 13, 8, 3), 'conv_narrow_wgrad<8>',
     outcomes=_merge(_wg_affine(refused(R_WGRAD), run('conv_narrow_wgrad<8>')), {('dz', 'slice1'): run('conv_wgrad_rows<3,1,')}),
     why={'affine': 'conv_route.h conv2d_wgrad_route (NarrowSlices): x.sc declines; dz.sc goes through conv_narrow_wgrad_kernel<8> of both slices',
          'slice1': 'conv_route.h conv2d_wgrad_route (NarrowSlices): !dz.vec declines -> the general kernel'})
_fam('wg_rows', 'wgrad', (2, 17, 16, 8, 32, 3), 'conv_wgrad_rows<3,1,', outcomes=_WG_NONE, why=_WG_WHY)
_fam('wg_wino', 'wgrad', (2, 17, 19, 24, 32, 3), 'conv_wino_wgrad<', env={'DL4DS_WINO_FORCE': 'all'},
     outcomes=_merge(_WG_NONE, _cells(WG_ROLES, ('slice1',), run('conv_wgrad_rows<3,2,'))),
     why=dict(_WG_WHY, slice1='conv_wino_wgrad.hip conv2d_wino_wgrad: !x.vec || !dy.vec declines -> the general kernel'))
_fam('wg_d2s', 'wgrad', (2, 34, 20, 48, 192, 3), 'conv_wgrad_rows<3,3,', d2s=('dz', 2), outcomes=_WG_NONE, why=_WG_WHY)
