"""The reference of tests/test_gpu_cgan_routes.py checked on its own (no GPU, nothing of the product): tests/cgan_route_cases.py's
float64 step against central finite differences, its two discriminator calls against one call on [real ; fake], the exact zeros
of samples outside Keras' clip range, and the input selection (the reference alone stays inside tests/parity.py's caps)."""
import numpy as np
import pytest
import torch

from tests import cgan_route_cases as C
from tests.parity import QUIET_SEEDS, assert_matches_reference

ALL_CASES = [(tp, 3, False) for tp in C.TOPOLOGIES] + [(tp, b, False) for tp in ('frames', 'two_readers') for b in (4, 2)] + \
            [('two_readers', 3, True)]


def _fp32_grads(tp, c):
    r = C.reference_step(tp, c['gw'], c['dw'], c['cond'], c['hr'], c['mask'], dt=np.float32, lam=c['lam'], weights=c['weights'],
                         clip_hi=c['clip_hi'])
    return {'G:' + k: v for k, v in r['gradsG'].items()} | {'D:' + k: v for k, v in r['gradsD'].items()}, r


@pytest.mark.parametrize('tp,B,weighted', ALL_CASES)
def test_selected_inputs_keep_the_reference_inside_the_caps(tp, B, weighted):
    """The inputs are the first of QUIET_SEEDS = 8 consecutive seeds on which the oracle grants no entry more than QUIET_LIMIT: one must
    exist, and the oracle's own float32 evaluation must then pass the criterion AND the caps on slack-reliant entries."""
    c = C.case(tp, B, weighted)
    first = C.FIRST_SEED + 100 * C.TOPOLOGIES.index(tp) + 10 * B
    assert first <= c['seed'] < first + QUIET_SEEDS
    assert C.quiet(c), (tp, B, c['seed'])
    got, r = _fp32_grads(tp, c)
    assert_matches_reference(got, c['ref'])
    np.testing.assert_allclose(r['losses'], c['ref']['losses'], rtol=1e-4)


@pytest.mark.parametrize('only_clipped', [False, True])
def test_clipped_case_is_quiet_and_spread(only_clipped):
    c = C.clipped_case(only_clipped)
    assert C.quiet(c), c['seed']
    B = c['cond'].shape[0]
    fake = c['logits'][B:]
    assert (fake < -C.LOGIT_EDGE - C.LOGIT_MARGIN).any() and (fake > C.LOGIT_EDGE + C.LOGIT_MARGIN).any()
    assert only_clipped or (np.abs(fake) < C.LOGIT_EDGE - C.LOGIT_MARGIN).any()
    r = C.reference_step('two_readers', c['gw'], c['dw'], c['cond'], c['hr'], c['mask'], lam=c['lam'], clip_hi=c['clip_hi'])
    p = r['p_fake'].ravel()
    assert (p < 1e-7).any() and (p.astype(np.float32) == np.float32(1.0)).any()          # below the range / rounds to 1.0f
    got, _ = _fp32_grads('two_readers', c)
    assert_matches_reference(got, c['ref'])


def test_reference_gradients_match_central_differences():
    """d gen_total / d G's parameters and d disc / d D's parameters in float64 against (f(x + h) - f(x - h)) / 2h, h = 1e-5, on three
    entries of every tensor (two_readers: concat of two readers, net_pin generator).  Bound 1e-6 of the tensor's largest gradient
    entry + 1e-9: the truncation term is h^2 f''' / 6 ~ 1e-10, the rounding term 1e-16 |f| / h ~ 1e-11."""
    tp = 'two_readers'
    c = C.case(tp)
    f64 = lambda d: {k: np.asarray(v, np.float64) for k, v in d.items()}
    gw, dw = f64(c['gw']), f64(c['dw'])
    step = lambda g, d: C.reference_step(tp, g, d, c['cond'], c['hr'], c['mask'], lam=c['lam'])
    ref = step(gw, dw)
    rng = np.random.default_rng(5)
    h = 1e-5
    for which, params, grads, li in (('G', gw, ref['gradsG'], 0), ('D', dw, ref['gradsD'], 3)):
        for k, v in params.items():
            scale = np.abs(grads[k]).max()
            for idx in rng.choice(v.size, size=min(3, v.size), replace=False):
                vals = []
                for sgn in (+1, -1):
                    p2 = dict(params)
                    p2[k] = v.copy()
                    p2[k].flat[idx] += sgn * h
                    vals.append(step(p2, dw)['losses'][li] if which == 'G' else step(gw, p2)['losses'][li])
                fd = (vals[0] - vals[1]) / (2 * h)
                assert abs(fd - grads[k].flat[idx]) <= 1e-6 * scale + 1e-9, (which, k, int(idx), fd, grads[k].flat[idx])


@pytest.mark.parametrize('tp', C.TOPOLOGIES)
def test_two_discriminator_calls_equal_one_call_on_the_joined_batch(tp):
    """The samples of D are independent: D(cond, hr) and D(cond, gen) are the halves of D([cond ; cond], [hr ; gen])."""
    c = C.case(tp)
    B = c['cond'].shape[0]
    t = lambda a: torch.from_numpy(np.asarray(a, np.float64))
    with torch.no_grad():
        PG, PD = C._tensors(c['gw'], np.float64), C._tensors(c['dw'], np.float64)
        cond, hr, mask = t(c['cond']), t(c['hr']), t(c['mask'])
        gen = C.generator_ref(tp, PG, cond)
        two = torch.cat([C.discriminator_ref(tp, PD, cond, hr, mask[:B]), C.discriminator_ref(tp, PD, cond, gen, mask[B:])])
        one = C.discriminator_ref(tp, PD, torch.cat([cond, cond]), torch.cat([hr, gen]), mask)
    assert one.shape == (2 * B, 1)
    np.testing.assert_allclose(one.numpy(), two.numpy(), rtol=0, atol=1e-14)


def test_clipped_samples_carry_no_gradient():
    """Outside [1e-7, 1 - 1e-7] the clip cuts the gradient: with only such generated samples and lam = 0 every generator gradient and
    D's generated-term gradient are exactly 0; in the mixed batch the adversarial gradient w.r.t. the clipped samples' images is 0."""
    c = C.clipped_case(True)
    r = C.reference_step('two_readers', c['gw'], c['dw'], c['cond'], c['hr'], c['mask'], lam=0.0, clip_hi=c['clip_hi'])
    assert all(np.all(v == 0.0) for v in r['gradsG'].values())
    c = C.clipped_case(False)
    B = c['cond'].shape[0]
    t = lambda a: torch.from_numpy(np.asarray(a, np.float64))
    PG, PD = C._tensors(c['gw'], np.float64), C._tensors(c['dw'], np.float64)
    gen = C.generator_ref('two_readers', PG, t(c['cond'])).detach().requires_grad_(True)
    p = C.discriminator_ref('two_readers', PD, t(c['cond']), gen, t(c['mask'])[B:])
    for label in (1.0, 0.0):
        g_gen, *g_par = torch.autograd.grad(C.bce(label, p, c['clip_hi']), [gen] + list(PD.values()), retain_graph=True)
        clipped = c['clipped'][B:]
        assert clipped.sum() == 2 and np.all(g_gen.numpy()[clipped] == 0.0) and np.all(g_gen.numpy()[~clipped].any(axis=(1, 2, 3)))
    only = torch.autograd.grad(C.bce(0.0, p[torch.from_numpy(clipped)], c['clip_hi']), list(PD.values()), allow_unused=True)
    assert all(g is None or bool((g == 0).all()) for g in only)
