"""The CGAN step's adversarial gradient through the discriminator (csrc/cgan.hip, pass 2) on the graphs of tests/cgan_route_cases.py,
by each of its routes, against the float64 reference step of that module:
  ratio            (default, unless the eligibility scan refuses the graph: cases.RATIO_REFUSED) cgan_ratio_kernel + one scale_samples_kernel launch per op that reads D's HR input, tag cgan_scale_samples
  second backward  (DL4DS_NO_CGAN_RATIO=1) over the generated half, tag cgan_pass2_partial; over the whole batch with a zeroed real half
                   where an op refuses partial batches (channel attention), tag cgan_pass2_zero_filled
The route is decided once per trainer, so every engine is built after the variable is set, and the launch tags of the step are asserted:
a test that fell onto another route fails.  Losses to rel 1e-4 and gradients by tests/parity.py's per-element criterion and caps, as the
CGAN tests of test_gpu_models.py; the two routes against each other to 2e-5 * scale + 1e-9, as the switch test there.  Inputs: the
first of parity.QUIET_SEEDS = 8 consecutive seeds on which the reference has no unit next to a kink (tests/test_cgan_route_cases.py
asserts on the CPU that one exists and that the reference's own float32 evaluation stays inside the caps)."""
import numpy as np
import pytest

from tests import cgan_route_cases as C
from tests.parity import assert_matches_reference, kernel_tags

pytestmark = pytest.mark.gpu

ROUTES = ['ratio', 'second_backward']
LOSSES = ('gen_total', 'gen_gan', 'gen_px', 'disc')


def _engine(tp, c, route, monkeypatch):
    from dl4ds_amd.training import CGANEngine
    if route == 'ratio':
        monkeypatch.delenv('DL4DS_NO_CGAN_RATIO', raising=False)
    else:
        monkeypatch.setenv('DL4DS_NO_CGAN_RATIO', '1')
    gen, disc = C.build_generator(tp), C.build_discriminator(tp)
    for m, w in ((gen, c['gw']), (disc, c['dw'])):
        have = m.get_weights()
        assert set(have) == set(w) and all(have[k].shape == w[k].shape for k in w), sorted(set(have) ^ set(w))
        m.set_weights(w)
    return CGANEngine(gen, disc, loss='mae', learning_rate=2e-4, beta_1=0.5, lambda_scaling_factor=c['lam']), gen, disc


def _step(eng, gen, disc, c):
    out, tags = kernel_tags(lambda: eng.step([c['cond']], c['hr'], dropout_keep=c['mask'], apply_update=False))
    return out, gen.get_gradients(), disc.get_gradients(), tags


def _assert_route(tp, route, tags):
    got = tuple(tags.get(k, 0) for k in ('cgan_scale_samples', 'cgan_pass2_partial', 'cgan_pass2_zero_filled'))
    ratio = route == 'ratio' and tp not in C.RATIO_REFUSED
    want = (C.READERS[tp], 0, 0) if ratio else (0, 0, 1) if tp == 'attention' else (0, 1, 0)
    assert got == want, (tp, route, got, want)


def _assert_reference(out, gg, gd, c, what, losses=LOSSES):
    for i, k in enumerate(LOSSES):
        print(what, k, out[i], c['ref']['losses'][i])
        if k in losses:
            assert out[i] == pytest.approx(c['ref']['losses'][i], rel=1e-4), (what, k)
    rows = assert_matches_reference({'G:' + k: v for k, v in gg.items()} | {'D:' + k: v for k, v in gd.items()}, c['ref'], what=what)
    print(what, 'worst gradient error / tensor size', max(r['err'] for r in rows), 'entries on slack', sum(r['n_slack'] for r in rows))


def _assert_routes_agree(a, b):
    (o0, g0, d0, _), (o1, g1, d1, _) = a, b
    for x, y in zip(o0, o1):
        assert x == pytest.approx(y, rel=1e-5)
    for name, (x, y) in [('G', (g0, g1)), ('D', (d0, d1))]:
        for k in x:
            scale = max(np.abs(y[k]).max(), 1e-12)
            assert np.abs(x[k] - y[k]).max() <= 2e-5 * scale + 1e-9, (name, k)


def _bitwise(a, b):
    return a[0] == b[0] and all(np.array_equal(a[i][k], b[i][k]) for i in (1, 2) for k in a[i])


@pytest.mark.parametrize('tp', C.TOPOLOGIES)
def test_routes_match_the_reference(monkeypatch, tp):
    """B = 3: the four losses and every gradient of G and D by each route against the reference, the route that ran by its tags (two
    rescaling launches for the two readers), the routes against each other.  chained_readers: the default falls to the second backward
    pass -- rescaling its two readers one after the other counted the 1x1 reader's gradient twice in the 3x3 reader's (measured before
    the eligibility scan refused the graph: see the summary of the change that added this test)."""
    c = C.case(tp)
    res = {}
    for route in ROUTES:
        eng, gen, disc = _engine(tp, c, route, monkeypatch)
        res[route] = _step(eng, gen, disc, c)
        _assert_route(tp, route, res[route][3])
        _assert_reference(*res[route][:3], c, (tp, route))
    _assert_routes_agree(res['ratio'], res['second_backward'])
    same = all(np.array_equal(res['ratio'][1][k], res['second_backward'][1][k]) for k in res['ratio'][1])
    assert same == (tp in C.RATIO_REFUSED)                 # (another evaluation, unless the graph is one the ratio route refuses)


def test_clipped_probabilities(monkeypatch):
    """two_readers with generated samples at p < 1e-7, inside the range and at p = 1.0f (every logit 5 away from the thresholds): both
    routes match the reference, whose BCE clips at float32's 1 - 1e-7 (cgan_route_cases.CLIP_HI32)."""
    tp, c = 'two_readers', C.clipped_case(False)
    res = {}
    for route in ROUTES:
        eng, gen, disc = _engine(tp, c, route, monkeypatch)
        res[route] = _step(eng, gen, disc, c)
        _assert_route(tp, route, res[route][3])
        _assert_reference(*res[route][:3], c, ('clipped', route))
    _assert_routes_agree(res['ratio'], res['second_backward'])


@pytest.mark.parametrize('route', ROUTES)
def test_only_clipped_samples_give_exact_zeros(monkeypatch, route):
    """lam = 0 and a batch whose generated samples all lie outside the clip range: every generator gradient is exactly 0.0 (no NaN, no
    -0 * inf), D's gradients are those of its real term.  (gen_total and gen_px are not compared: the step reports the pixel loss as
    (lam * px) / lam, which is 0 / 0 at lam = 0.)"""
    tp, c = 'two_readers', C.clipped_case(True)
    eng, gen, disc = _engine(tp, c, route, monkeypatch)
    out, gg, gd, tags = _step(eng, gen, disc, c)
    _assert_route(tp, route, tags)
    for k, v in gg.items():
        assert np.all(v == 0.0), (k, v.ravel()[:4])
    assert all(np.isfinite(v).all() for v in gd.values())
    _assert_reference(out, gg, gd, c, ('only_clipped', route), losses=('gen_gan', 'disc'))


@pytest.mark.parametrize('route', ROUTES)
@pytest.mark.parametrize('tp', ['frames', 'two_readers'])
def test_batch_changes_on_one_engine(monkeypatch, tp, route):
    """B = 4, 2, 4 on one trainer: the ratio buffer is sized for 8 rows and then used with 4, p_fake sits at row B of the current batch.
    Every step matches its reference, the third equals the first bit for bit."""
    big, small = C.case(tp, 4), C.case(tp, 2)
    eng, gen, disc = _engine(tp, big, route, monkeypatch)
    res = []
    for i, c in enumerate((big, small, big)):
        res.append(_step(eng, gen, disc, c))
        _assert_route(tp, route, res[-1][3])
        _assert_reference(*res[-1][:3], c, (tp, route, 'step', i, 'B', c['cond'].shape[0]))
    assert _bitwise(res[0], res[2])


@pytest.mark.parametrize('route', ROUTES)
def test_pixel_loss_weights_leave_the_adversarial_terms_alone(monkeypatch, route):
    """set_loss_weights on the engine: gen_gan, disc and D's gradients are bitwise those of the unweighted step, G's gradients and the
    losses match the reference with sum w |d| / sum w as its pixel term."""
    tp, c = 'two_readers', C.case('two_readers', 3, True)
    eng, gen, disc = _engine(tp, c, route, monkeypatch)
    plain = _step(eng, gen, disc, c)
    eng.set_loss_weights(c['weights'])
    weighted = _step(eng, gen, disc, c)
    _assert_route(tp, route, weighted[3])
    assert weighted[0][1] == plain[0][1] and weighted[0][3] == plain[0][3]
    assert all(np.array_equal(weighted[2][k], plain[2][k]) for k in plain[2])
    assert weighted[0][2] != plain[0][2]
    _assert_reference(*weighted[:3], c, ('weighted', route))
