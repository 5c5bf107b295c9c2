"""Tiny two-input discriminators for the CGAN step's adversarial-gradient routes (csrc/cgan.hip, "pass 2"), each defined TWICE:
as a GraphBuilder graph (``build_discriminator`` / ``build_generator``: need the library, imported inside the functions) and as a
plain torch function over the oracle's layer definitions (``discriminator_ref`` / ``generator_ref``: oracle/models.py and
oracle/torch_ops.py, autograd, any dtype), plus the reference step and the seeded cases shared by tests/test_cgan_route_cases.py
(CPU) and tests/test_gpu_cgan_routes.py.  Not a test module; importable without a GPU; the reference imports nothing of the product.

The graphs are the forms residual_discriminator never produces (all without a normalisation op, so the ratio route is eligible):
  frames           both inputs carry T = 3 frames per sample: conv on each input, concat, conv + ReLU, pooling over (T, H, W).  With
                   B = 3 the image index n, n // T, n % B and n // B all differ, so a factor looked up by anything but n // T is wrong
  two_readers      the HR input feeds a 3x3 (ReLU) and a 1x1 convolution, both concatenated with the conditioning branch
  pool_reader      the HR input feeds max-pooling, only then a convolution: the reader is no convolution and the rescaled tensor is
                   the pooled one
  relu_reader_add  the reader is a convolution with fused ReLU whose output feeds two residual blocks AND the ``add=`` of the
                   convolution behind them (branch2_in of residual_discriminator on a deeper chain, with the ReLU it never has)
  attention        two_readers with a channel-attention block behind the merge convolution (refuses partial batches)
  chained_readers  two_readers whose 1x1 reader takes the 3x3 reader's output as its fused ``add=``: running the 1x1 reader's backward
                   again adds its output gradient to the 3x3 reader's a second time, so rescaling the readers one by one is not the
                   second backward pass here and the ratio route has to refuse the graph
every one followed by GlobalAveragePooling, Dropout(0.4) with an injected keep-mask and two sigmoid Dense layers.

The step (reference cgan.py:575-639): gen = G(cond); p_real = D(cond, hr), p_fake = D(cond, gen);
  gen_gan = BCE(1, p_fake), gen_px = MAE(hr, gen) [weighted: sum w |d| / sum w], gen_total = gen_gan + lam * gen_px,
  disc = BCE(1, p_real) + BCE(0, p_fake), BCE on clip(p, 1e-7, 1 - 1e-7) as Keras does; gradients of gen_total w.r.t. G's and of
  disc w.r.t. D's parameters.
"""
import functools

import numpy as np
import torch

from oracle import models as M
from oracle import torch_ops as T
from tests.parity import banded_reference, first_quiet, is_quiet, targets_clear_of_the_kink

TOPOLOGIES = ['frames', 'two_readers', 'pool_reader', 'relu_reader_add', 'attention', 'chained_readers']
READERS = {'frames': 1, 'two_readers': 2, 'pool_reader': 1, 'relu_reader_add': 1, 'attention': 2, 'chained_readers': 2}     # ops reading the HR input
RATIO_REFUSED = ('chained_readers',)          # the ratio route must not take these: the second backward pass runs instead
NF, N_COND, DENSE1, T_FRAMES, RATE = 4, 2, 8, 3, 0.4
# lam: at the trainer's default of 100 the adversarial term is 1e-4 .. 6e-3 of every generator gradient tensor on these graphs (from
# the float64 reference alone: lam = 0 against lam = 100), i.e. below the 1e-3 bar -- a wrong per-sample factor would pass.  At 0.02
# it is the larger part of most tensors; the pixel-weight case, which is about the OTHER term, takes 1.
LAMBDA, LAMBDA_WEIGHTED = 0.02, 1.0
GRIDS = {'frames': (8, 10), 'two_readers': (10, 12), 'pool_reader': (10, 12), 'relu_reader_add': (9, 11), 'attention': (10, 12),
         'chained_readers': (9, 12)}
GEN_CFG = dict(backbone_block='convnet', n_filters=4, n_blocks=1)          # net_pin, the generator of the spatial topologies
FIRST_SEED = 300           # inputs: the first of the seeds FIRST_SEED + 100 * k, ... (+ parity.QUIET_SEEDS = 8) with a quiet reference
EPS = 1e-7
# Keras clips in the dtype of p: in float32 the upper bound 1 - 1e-7 is 1 - 2^-23.  A probability that saturates to 1.0f takes
# -log(1 - bound) = 15.94 there and 16.12 under the float64 bound, so the cases WITH such samples are referred to the float32 bound
CLIP_HI32 = float(np.float32(1.0) - np.float32(EPS))
LOGIT_EDGE = float(np.log((1 - EPS) / EPS))          # 16.118: |logit| at which p leaves [1e-7, 1 - 1e-7]
LOGIT_MARGIN = 5.0


def frames_of(topology):
    return T_FRAMES if topology == 'frames' else 1


def merge_channels(topology):
    return {'frames': 2 * NF, 'two_readers': 3 * NF, 'pool_reader': 2 * NF, 'relu_reader_add': 2 * NF, 'attention': 3 * NF,
            'chained_readers': 3 * NF}[topology]


# ---- the product's graphs ------------------------------------------------------------------------------------------------------------
def build_discriminator(topology):
    from dl4ds_amd.graph import GraphBuilder, Model
    from dl4ds_amd.models.blocks import residual_block
    (h, w), t = GRIDS[topology], frames_of(topology)
    g = GraphBuilder()
    x_in = g.input(h, w, N_COND, nmul=t)
    x_ref = g.input(h, w, 1, nmul=t, requires_grad=True)
    if topology == 'frames':
        a = g.conv2d(x_ref, 'hr_conv', NF, 3)
        b = g.conv2d(x_in, 'cond_conv', NF, 3)
        x = g.concat([b, a], 'concat')
    elif topology in ('two_readers', 'attention'):
        a = g.conv2d(x_ref, 'hr_conv3', NF, 3, activation='relu')
        c = g.conv2d(x_ref, 'hr_conv1', NF, 1)
        b = g.conv2d(x_in, 'cond_conv', NF, 3, activation='relu')
        x = g.concat([b, a, c], 'concat')
    elif topology == 'chained_readers':
        a = g.conv2d(x_ref, 'hr_conv3', NF, 3, activation='relu')
        c = g.conv2d(x_ref, 'hr_conv1', NF, 1, add=a)
        b = g.conv2d(x_in, 'cond_conv', NF, 3, activation='relu')
        x = g.concat([b, a, c], 'concat')
    elif topology == 'pool_reader':
        a = g.conv2d(g.maxpool2(x_ref, 'hr_pool'), 'hr_conv', NF, 3, activation='relu')
        b = g.maxpool2(g.conv2d(x_in, 'cond_conv', NF, 3, activation='relu'), 'cond_pool')
        x = g.concat([b, a], 'concat')
    elif topology == 'relu_reader_add':
        x2 = g.conv2d(x_ref, 'hr_in', NF, 3, activation='relu')
        c = residual_block(g, 'hr_res1', x2, NF)
        c = residual_block(g, 'hr_res2', c, NF)
        a = g.conv2d(c, 'hr_out', NF, 3, add=x2)
        b = g.conv2d(x_in, 'cond_conv', NF, 3, activation='relu')
        x = g.concat([b, a], 'concat')
    else:
        raise ValueError(topology)
    x = g.conv2d(x, 'merge_conv', x.C, 3, activation='relu')
    if topology == 'attention':
        x = g.channel_attention(x, 'att', x.C)
    x = g.gap(x, 'gap', over_time=t > 1)
    x = g.dropout(x, RATE, 'dropout')
    x = g.dense(x, 'dense1', DENSE1, activation='sigmoid')
    x = g.dense(x, 'dense2', 1, activation='sigmoid')
    g.finalize(x, 0)
    lead = (t,) if t > 1 else ()
    return Model(g, 'discriminator_' + topology, [lead + (h, w, N_COND), lead + (h, w, 1)])


def build_generator(topology):
    (h, w), t = GRIDS[topology], frames_of(topology)
    if t == 1:
        import dl4ds_amd.models as PM
        return PM.net_pin(n_channels=N_COND, n_aux_channels=0, hr_size=(h, w), seed=0, **GEN_CFG)
    from dl4ds_amd.graph import GraphBuilder, Model
    g = GraphBuilder()                                    # frame-wise: its output carries T frames per sample, as D's HR input does
    x = g.input(h, w, N_COND, nmul=t)
    y = g.conv2d(x, 'gen_conv1', NF, 3, activation='relu')
    y = g.conv2d(y, 'gen_conv2', 1, 3)
    g.finalize(y, 0)
    return Model(g, 'frame_generator', [(t, h, w, N_COND)])


# ---- the same graphs over the oracle's layers ---------------------------------------------------------------------------------------
def discriminator_ref(topology, P, x_in, x_ref, mask, ops=T, parts=False):
    """-> p (N, 1); ``parts``: (p, logit, dense1's output).  5-D inputs are (B, T, H, W, C): Conv2D takes the leading axes as batch."""
    conv = lambda name, x, f, k: M._conv(ops, P, name, x, f, k)
    if topology == 'frames':
        x = ops.concat([conv('cond_conv', x_in, NF, 3), conv('hr_conv', x_ref, NF, 3)])
    elif topology in ('two_readers', 'attention'):
        a = ops.relu(conv('hr_conv3', x_ref, NF, 3))
        c = conv('hr_conv1', x_ref, NF, 1)
        x = ops.concat([ops.relu(conv('cond_conv', x_in, NF, 3)), a, c])
    elif topology == 'chained_readers':
        a = ops.relu(conv('hr_conv3', x_ref, NF, 3))
        c = ops.add(conv('hr_conv1', x_ref, NF, 1), a)
        x = ops.concat([ops.relu(conv('cond_conv', x_in, NF, 3)), a, c])
    elif topology == 'pool_reader':
        a = ops.relu(conv('hr_conv', ops.max_pool2(x_ref), NF, 3))
        x = ops.concat([ops.max_pool2(ops.relu(conv('cond_conv', x_in, NF, 3))), a])
    elif topology == 'relu_reader_add':
        x2 = ops.relu(conv('hr_in', x_ref, NF, 3))
        c = M.residual_block(ops, P, 'hr_res1', x2, NF)
        c = M.residual_block(ops, P, 'hr_res2', c, NF)
        a = ops.add(conv('hr_out', c, NF, 3), x2)
        x = ops.concat([ops.relu(conv('cond_conv', x_in, NF, 3)), a])
    else:
        raise ValueError(topology)
    x = ops.relu(conv('merge_conv', x, x.shape[-1], 3))
    if topology == 'attention':
        x = M.channel_attention(ops, P, 'att', x, x.shape[-1])
    x = ops.global_avg_pool(x)
    if mask is not None:
        x = ops.dropout_apply(x, mask, RATE)
    h1 = ops.sigmoid(ops.dense(x, P.get(ops, 'dense1/kernel', (x.shape[-1], DENSE1)), P.get(ops, 'dense1/bias', (DENSE1,), 'zeros')))
    logit = ops.dense(h1, P.get(ops, 'dense2/kernel', (DENSE1, 1)), P.get(ops, 'dense2/bias', (1,), 'zeros'))
    p = ops.sigmoid(logit)
    return (p, logit, h1) if parts else p


def generator_ref(topology, P, x, ops=T):
    if frames_of(topology) == 1:
        return M.net_pin(ops, P, x, None, **GEN_CFG)
    y = ops.relu(M._conv(ops, P, 'gen_conv1', x, NF, 3))
    return M._conv(ops, P, 'gen_conv2', y, 1, 3)


def bce(label, p, clip_hi=1 - EPS):
    """Keras binary_crossentropy of a constant label: mean over the samples of -(y log q + (1 - y) log(1 - q)), q = clip(p, eps, hi)."""
    q = torch.clamp(p, EPS, clip_hi)
    return -(label * torch.log(q) + (1 - label) * torch.log(1 - q)).mean()


def pixel_loss(hr, gen, weights=None):
    if weights is None:
        return T.mae(hr, gen)
    w = torch.as_tensor(np.asarray(weights), dtype=gen.dtype)[..., None].expand(gen.shape)       # one (H, W) map for every image
    return (w * T._shifted(gen - hr).abs()).sum() / w.sum()


def _tensors(P, dt):
    Q = M.Params()
    for k, v in P.items():
        Q[k] = torch.from_numpy(np.asarray(v, dt)).clone().requires_grad_(True)
    return Q


def reference_step(topology, gw, dw, cond, hr, mask, dt=np.float64, lam=LAMBDA, weights=None, clip_hi=1 - EPS):
    """One step in ``dt`` -> dict(losses=[gen_total, gen_gan, gen_px, disc], gradsG, gradsD, gen, p_real, p_fake)."""
    PG, PD = _tensors(gw, dt), _tensors(dw, dt)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a, dt))
    cond, hr, mask = t(cond), t(hr), t(mask)
    B = cond.shape[0]
    gen = generator_ref(topology, PG, cond)
    p_real = discriminator_ref(topology, PD, cond, hr, mask[:B])
    p_fake = discriminator_ref(topology, PD, cond, gen, mask[B:])
    gan, px = bce(1.0, p_fake, clip_hi), pixel_loss(hr, gen, weights)
    total = gan + lam * px
    disc = bce(1.0, p_real, clip_hi) + bce(0.0, p_fake, clip_hi)
    gG = torch.autograd.grad(total, list(PG.values()), retain_graph=True, allow_unused=True)
    gD = torch.autograd.grad(disc, list(PD.values()), allow_unused=True)
    zero = lambda g, v: (torch.zeros_like(v) if g is None else g).detach().numpy()
    return dict(losses=[float(total.detach()), float(gan.detach()), float(px.detach()), float(disc.detach())],
                gradsG={k: zero(g, v) for (k, v), g in zip(PG.items(), gG)}, gradsD={k: zero(g, v) for (k, v), g in zip(PD.items(), gD)},
                gen=gen.detach().numpy(), p_real=p_real.detach().numpy(), p_fake=p_fake.detach().numpy())


# ---- weights and inputs --------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def weights(topology):
    """-> (generator weights, discriminator weights) as {name: float32 array}: Keras initialisers, biases drawn non-zero."""
    (h, w), t = GRIDS[topology], frames_of(topology)
    lead = (1, t) if t > 1 else (1,)
    PG, PD = M.Params(create=True, seed=41, dtype=np.float64), M.Params(create=True, seed=42, dtype=np.float64)
    z = lambda c: torch.zeros(lead + (h, w, c), dtype=torch.float64)
    with torch.no_grad():
        generator_ref(topology, PG, z(N_COND))
        discriminator_ref(topology, PD, z(N_COND), z(1), None)
    rng = np.random.default_rng(43)
    out = []
    for P in (PG, PD):
        d = {}
        for k, v in P.items():
            a = v.numpy()
            d[k] = (rng.standard_normal(a.shape) * 0.05 if k.endswith('bias') else a).astype(np.float32)
        out.append(d)
    return tuple(out)


def _draw(topology, B, seed, offsets=None):
    """cond in U[0, 1) (+ a per-sample offset), hr = G(cond) +- (0.5 .. 1.5) (no MAE residual near its sign change), keep-mask."""
    (h, w), t = GRIDS[topology], frames_of(topology)
    lead = (B, t) if t > 1 else (B,)
    rng = np.random.default_rng(seed)
    cond = rng.random(lead + (h, w, N_COND))
    if offsets is not None:
        cond = cond + np.asarray(offsets, np.float64).reshape((B,) + (1,) * (cond.ndim - 1))
    cond = cond.astype(np.float32)
    gw, _ = weights(topology)
    with torch.no_grad():
        pred = generator_ref(topology, _tensors(gw, np.float64), torch.from_numpy(cond.astype(np.float64))).numpy()
    hr = targets_clear_of_the_kink(pred, rng)
    mask = (rng.random((2 * B, merge_channels(topology))) > RATE).astype(np.float32)
    return cond, hr, mask


def loss_weight_map(topology):
    """(H, W) weights of the pixel loss: U[0.5, 2) with about a fifth exact zeros."""
    rng = np.random.default_rng(77)
    w = rng.uniform(0.5, 2.0, GRIDS[topology])
    w[rng.random(w.shape) < 0.2] = 0.0
    return w.astype(np.float32)


def _banded(topology, gw, dw, cond, hr, mask, **kw):
    def call(dt):
        r = reference_step(topology, gw, dw, cond, hr, mask, dt=dt, **kw)
        g = {'G:' + k: v for k, v in r['gradsG'].items()}
        g.update({'D:' + k: v for k, v in r['gradsD'].items()})
        return r['losses'], g, None
    return banded_reference(call)


@functools.lru_cache(maxsize=None)
def case(topology, B=3, weighted=False):
    """-> dict(gw, dw, cond, hr, mask, weights, ref, seed): the first seed (of parity.QUIET_SEEDS) on which the reference has no unit
    next to a kink; ``ref`` is tests/parity.py's banded reference with the gradients under 'G:<name>' / 'D:<name>'."""
    gw, dw = weights(topology)
    wmap, lam = (loss_weight_map(topology), LAMBDA_WEIGHTED) if weighted else (None, LAMBDA)

    def attempt(seed):
        cond, hr, mask = _draw(topology, B, seed)
        return seed, cond, hr, mask, _banded(topology, gw, dw, cond, hr, mask, weights=wmap, lam=lam)
    seed, cond, hr, mask, ref = first_quiet(attempt, FIRST_SEED + 100 * TOPOLOGIES.index(topology) + 10 * B)
    return dict(gw=gw, dw=dw, cond=cond, hr=hr, mask=mask, weights=wmap, ref=ref, seed=seed, lam=lam, clip_hi=1 - EPS)


# ---- probabilities outside Keras' clip range -----------------------------------------------------------------------------------------
def _with_logits(topology, dw, cond, hr, mask, targets):
    """dw with dense2 set so that the 2B samples' logits (real rows first) are ``targets``: the minimum-norm solution of
    [h1, 1] x = targets over dense1's outputs of the float64 reference.  -> (dw', logits of the float32-rounded solution)."""
    gw, _ = weights(topology)
    B = cond.shape[0]
    with torch.no_grad():
        PG, PD = _tensors(gw, np.float64), _tensors(dw, np.float64)
        t = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.float64))
        gen = generator_ref(topology, PG, t(cond))
        h1 = torch.cat([discriminator_ref(topology, PD, t(cond), x, t(m), parts=True)[2]
                        for x, m in ((t(hr), mask[:B]), (gen, mask[B:]))]).numpy()
    A = np.concatenate([h1, np.ones((2 * B, 1))], axis=1)
    x = (np.linalg.pinv(A) @ np.asarray(targets, np.float64)).astype(np.float32)
    out = dict(dw)
    out['dense2/kernel'], out['dense2/bias'] = x[:-1].reshape(DENSE1, 1), x[-1:].copy()
    return out, A @ x.astype(np.float64)


@functools.lru_cache(maxsize=None)
def clipped_case(only_clipped=False):
    """two_readers with the samples' logits spread across the clip range by a per-sample offset of the conditioning input and a
    dense2 solved for them.  Generated samples: logit -30 (p < 1e-7), +1, +30 (p rounds to 1.0f); real samples -27, -0.5, +26.
    ``only_clipped``: B = 2, generated logits -30 and +30, real ones inside the range, lam = 0.  Every logit keeps LOGIT_MARGIN from
    +-LOGIT_EDGE (asserted), so the float32 and the float64 decisions agree.  -> case dict with ``logits`` (2B, real rows first)."""
    topology = 'two_readers'
    gw, dw0 = weights(topology)
    dw0 = dict(dw0)
    dw0['dense1/kernel'] = dw0['dense1/kernel'] * np.float32(16.0)          # dense1's outputs differ more from sample to sample
    if only_clipped:
        B, offsets, targets, lam = 2, [-2.0, 2.0], [-0.5, 0.8, -30.0, 30.0], 0.0
    else:
        B, offsets, targets, lam = 3, [-2.0, 0.0, 2.0], [-27.0, -0.5, 26.0, -30.0, 1.0, 30.0], LAMBDA

    def attempt(seed):
        cond, hr, mask = _draw(topology, B, seed, offsets)
        dw, logits = _with_logits(topology, dw0, cond, hr, mask, targets)
        return seed, cond, hr, mask, dw, logits, _banded(topology, gw, dw, cond, hr, mask, lam=lam, clip_hi=CLIP_HI32)
    seed, cond, hr, mask, dw, logits, ref = first_quiet(attempt, FIRST_SEED + 700 + 10 * B)
    away = np.abs(np.abs(logits) - LOGIT_EDGE)
    assert away.min() >= LOGIT_MARGIN and np.abs(logits - targets).max() < 0.01, (logits, targets)
    return dict(gw=gw, dw=dw, cond=cond, hr=hr, mask=mask, weights=None, ref=ref, seed=seed, lam=lam, clip_hi=CLIP_HI32, logits=logits,
                clipped=np.abs(logits) > LOGIT_EDGE)


def quiet(c):
    return is_quiet(c['ref'])
