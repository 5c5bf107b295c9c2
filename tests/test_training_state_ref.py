"""CPU checks of tests/training_state_ref.py: the restatement against hand-worked numbers, a float32 evaluation of a correct
trajectory inside its bounds, and the proof that the bounds DISCRIMINATE -- a restatement whose schedule boundary or whose bias
correction step is off by one fails them on at least 90 % of the entries with a non-zero gradient."""
import numpy as np

from tests import training_state_ref as R

LR0, LR1, BOUNDARY, STEPS = 1e-3, 1e-4, 2, 6


def _trajectory(n=4000, seed=0):
    """A float32 Adam trajectory of STEPS updates under the schedule, on synthetic gradients with a persistent sign (a mean plus
    30 % noise per step, like a loss that keeps falling: |m| / sqrt(v) stays of order one, so every entry moves by about lr) ->
    list of (before, g, after, iterations)."""
    rng = np.random.default_rng(seed)
    w = rng.standard_normal(n).astype(np.float32)
    g0 = rng.standard_normal(n).astype(np.float32)
    g0[::50] = 0                                                  # entries no gradient reaches
    m, v = np.zeros(n, np.float32), np.zeros(n, np.float32)
    out = []
    for it in range(STEPS):
        g = (g0 * (1 + 0.3 * rng.standard_normal(n))).astype(np.float32)
        lr = R.scheduled_lr(it, LR0, LR1, BOUNDARY)
        w1, m1, v1 = R.adam32(w, g, m, v, it, lr)
        out.append(((w, m, v), g, (w1, m1, v1), it))
        w, m, v = w1, m1, v1
    return out


def test_schedule_is_keras_piecewise_constant_decay():
    assert [R.scheduled_lr(i, LR0, LR1, BOUNDARY) for i in range(STEPS)] == [LR0, LR0, LR0, LR1, LR1, LR1]
    assert R.scheduled_lr(0, 5e-4, 1e-5, 0) == 5e-4 and R.scheduled_lr(1, 5e-4, 1e-5, 0) == 1e-5


def test_first_updates_by_hand():
    # t = 1: m = 0.1 g, v = 0.001 g^2, lr_t = lr sqrt(0.001) / 0.1  ->  dw = -lr g / (|g| + eps sqrt(1000))  ~ -lr sign(g)
    r = R.adam_step([1.0, -2.0], [0.5, -0.25], [0, 0], [0, 0], 0, 1e-3)
    b1, b2, eps = R.consts32(0.9, 0.999, 1e-7)
    np.testing.assert_allclose(r['m'], (1 - b1) * np.array([0.5, -0.25]), rtol=1e-15)
    np.testing.assert_allclose(r['v'], (1 - b2) * np.array([0.25, 0.0625]), rtol=1e-15)
    np.testing.assert_allclose(r['dw'], [-1e-3, 1e-3], rtol=2e-5)
    # t = 2 from that state with the same gradient: m = 0.19 g, v = 0.001999 g^2, lr_t = lr sqrt(1 - b2^2) / (1 - b1^2)
    r2 = R.adam_step(r['w'], [0.5, -0.25], r['m'], r['v'], 1, 1e-3)
    np.testing.assert_allclose(r2['m'], (1 - b1 * b1) * np.array([0.5, -0.25]), rtol=1e-12)
    np.testing.assert_allclose(r2['dw'], [-1e-3, 1e-3], rtol=2e-5)
    # decoupled decay uses the plain lr: w (1 - lr wd) before the Adam term; the clipping factor scales g
    r3 = R.adam_step([1.0], [0.0], [0], [0], 7, 1e-4, decay=0.5)
    np.testing.assert_allclose(r3['w'], [1.0 - 1e-4 * 0.5], rtol=1e-15)
    r4 = R.adam_step([1.0], [2.0], [0], [0], 0, 1e-3, grad_factor=0.25)
    np.testing.assert_allclose(r4['m'], [(1 - b1) * 0.5], rtol=1e-15)
    c, norm = R.clip_factor({'a': np.array([3.0]), 'b': np.array([4.0])}, 2.5)
    assert norm == 5.0 and c == 0.5
    assert R.clip_factor([np.array([3.0, 4.0])], 10.0)[0] == 1.0
    e, _ = R.ema_step([1.0], [2.0], 0.75)
    np.testing.assert_allclose(e, [1.25], rtol=1e-15)


def test_float32_trajectory_is_inside_the_bounds_and_reads_back_its_rate():
    for before, g, after, it in _trajectory():
        lr = R.scheduled_lr(it, LR0, LR1, BOUNDARY)
        c = R.check_step(before, g, after, it, lr)
        assert not c['m_bad'].any() and not c['v_bad'].any() and not c['w_bad'].any(), (it, c['m_ulps'], c['v_ulps'], c['w_over_lr'])
        assert c['m_ulps'] <= 2.0 and c['v_ulps'] <= 3.0                               # (the bounds leave room, and not orders of it)
        assert c['w_over_lr'] <= 2.0 ** -24 * 5 / lr + 1e-6          # (half an ulp of the subtraction at |w| < 5: the step itself is exact to 1e-7)
        assert abs(R.implied_lr(before[0], after, it) / lr - 1) < 1e-3
        idle = g == 0
        if it == 0:
            assert np.array_equal(after[0][idle], before[0][idle])


def test_a_restatement_shifted_by_one_step_fails_the_bounds():
    traj = _trajectory()
    for before, g, after, it in traj:
        live = g != 0
        # (a) the boundary one step late or early: the update at which the two schedules differ is 10 x off
        for wrong in (BOUNDARY + 1, BOUNDARY - 1):
            lr_wrong = R.scheduled_lr(it, LR0, LR1, wrong)
            if lr_wrong == R.scheduled_lr(it, LR0, LR1, BOUNDARY):
                continue
            c = R.check_step(before, g, after, it, lr_wrong)
            assert c['w_bad'][live].mean() >= 0.9, (it, wrong, c['w_bad'][live].mean())
        # (b) the bias correction lr_t taken from t + 1 or t - 1 (3 % off at t = 6, 25 % at t = 1)
        lr = R.scheduled_lr(it, LR0, LR1, BOUNDARY)
        for shift in (1, -1):
            if it + 1 + shift < 1:
                continue
            c = R.check_step(before, g, after, it, lr, t_shift=shift)
            assert c['w_bad'][live].mean() >= 0.9, (it, shift, c['w_bad'][live].mean())
    # both boundary shifts met an update at which they differ
    assert any(R.scheduled_lr(it, LR0, LR1, BOUNDARY + 1) != R.scheduled_lr(it, LR0, LR1, BOUNDARY) for it in range(STEPS))
    assert any(R.scheduled_lr(it, LR0, LR1, BOUNDARY - 1) != R.scheduled_lr(it, LR0, LR1, BOUNDARY) for it in range(STEPS))
    # (c) moments carried wrongly: the previous m dropped (as if every step were the first) fails m on the live entries after step 1
    before, g, after, it = traj[2]
    c = R.check_step((before[0], np.zeros_like(before[1]), before[2]), g, after, it, LR0)
    assert c['m_bad'][g != 0].mean() >= 0.9
    c = R.check_step((before[0], before[1], np.zeros_like(before[2])), g, after, it, LR0)
    assert c['v_bad'][g != 0].mean() >= 0.9
