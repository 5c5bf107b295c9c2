"""The optimiser extensions without a GPU: argument validation, the default decayed set on the parameter lists of one model of
every builder family (traced by the numpy oracle, which creates the same variables), the range table, the CGAN pair forms, the
launch figures tests/optimizer_cases.py restates, and the float64 reference tests/optimizer_ref.py against hand-worked cases."""
import inspect

import numpy as np
import pytest

from tests import optimizer_cases as C
from tests import optimizer_ref as R
from tests import step_kernels_cases as S
from dl4ds_amd.ops import merge_ranges
from dl4ds_amd.training.engine import (check_optimizer_args, cgan_optimizer_pair, decayed_parameters, default_decay_filter)

F32, F64 = np.float32, np.float64


# ---------------------------------------------------------------------------------------------------------------- arguments
def test_check_optimizer_args_accepts():
    assert check_optimizer_args() == (None, None, None)
    assert check_optimizer_args(1, 0, 0) == (1.0, 0.0, 0.0)
    assert check_optimizer_args(np.float32(0.5), np.float64(1e-4), 0.999) == (0.5, 1e-4, 0.999)
    assert check_optimizer_args(global_clipnorm=1e-30, weight_decay=None, ema_momentum=np.nextafter(1.0, 0.0))[0] == 1e-30
    assert all(isinstance(v, float) for v in check_optimizer_args(1, np.int64(2), np.float32(0.5)))


@pytest.mark.parametrize('kw', [dict(global_clipnorm=0), dict(global_clipnorm=-1.0), dict(global_clipnorm=np.inf),
                                dict(global_clipnorm=np.nan), dict(weight_decay=-1e-9), dict(weight_decay=np.inf),
                                dict(weight_decay=np.nan), dict(ema_momentum=1.0), dict(ema_momentum=-0.1),
                                dict(ema_momentum=np.nan), dict(ema_momentum=1.5)])
def test_check_optimizer_args_rejects_values(kw):
    with pytest.raises(ValueError):
        check_optimizer_args(**kw)


@pytest.mark.parametrize('kw', [dict(global_clipnorm='1'), dict(global_clipnorm=(1.0, 2.0)), dict(weight_decay=[1e-4]),
                                dict(weight_decay=True), dict(ema_momentum='0.99'), dict(ema_momentum=False),
                                dict(global_clipnorm=np.ones(2))])
def test_check_optimizer_args_rejects_types(kw):
    with pytest.raises(TypeError):
        check_optimizer_args(**kw)


def test_cgan_pair_forms():
    assert cgan_optimizer_pair('global_clipnorm', None) == (None, None)
    assert cgan_optimizer_pair('global_clipnorm', 2.0) == (2.0, 2.0)
    assert cgan_optimizer_pair('global_clipnorm', [2.0]) == (2.0, 2.0)
    assert cgan_optimizer_pair('weight_decay', (1e-4, None)) == (1e-4, None)
    assert cgan_optimizer_pair('weight_decay', [0.0, 1e-3]) == (0.0, 1e-3)
    with pytest.raises(ValueError):
        cgan_optimizer_pair('weight_decay', (1.0, 2.0, 3.0))
    with pytest.raises(ValueError):
        cgan_optimizer_pair('weight_decay', ())
    with pytest.raises(TypeError):                       # each side goes through check_optimizer_args
        check_optimizer_args(*[cgan_optimizer_pair('global_clipnorm', ('a', 1.0))[0]])


def test_new_keyword_arguments_are_trailing_and_default_to_none():
    from dl4ds_amd.training import SupervisedEngine, CGANEngine, SupervisedTrainer, CGANTrainer
    for cls in (SupervisedEngine, CGANEngine, SupervisedTrainer, CGANTrainer):
        p = inspect.signature(cls.__init__).parameters
        for k in ('global_clipnorm', 'weight_decay', 'ema_momentum'):
            assert k in p and p[k].default is None, (cls.__name__, k)
    for cls in (SupervisedEngine, CGANEngine):
        assert inspect.signature(cls.__init__).parameters['decay_filter'].default is None
        for meth in ('optimizer_stats', 'swap_ema', 'ema_weights', 'set_optimizer_ext', 'ema_state'):
            assert callable(getattr(cls, meth))


def test_trainers_validate_at_construction():
    from dl4ds_amd.training import SupervisedTrainer, CGANTrainer
    data = np.zeros((8, 16, 16, 1), np.float32)
    topo = np.zeros((16, 16), np.float32)
    with pytest.raises(ValueError):
        SupervisedTrainer('resnet', 'spc', data, data, data, scale=4, global_clipnorm=0.0, verbose=False)
    with pytest.raises(TypeError):
        SupervisedTrainer('resnet', 'spc', data, data, data, scale=4, ema_momentum='0.9', verbose=False)
    with pytest.raises(ValueError):
        CGANTrainer('resnet', 'spc', data, data, scale=4, static_vars=[topo], weight_decay=(1e-4, -1.0), verbose=False)
    t = CGANTrainer('resnet', 'spc', data, data, scale=4, static_vars=[topo], global_clipnorm=(1.0, 2.0), ema_momentum=0.99, verbose=False)
    assert t.global_clipnorm == (1.0, 2.0) and t.ema_momentum == 0.99


# ---------------------------------------------------------------------------------------------------------------- decayed set
def _oracle_params(model, xs, ss=None, **cfg):
    from oracle import models as M
    norm = cfg.pop('normalization', None)                   # the oracle takes normalization through its Ctx
    if norm is not None:
        cfg['ctx'] = M.Ctx(training=True, normalization=norm)
    return {k: tuple(np.shape(v)) for k, v in M.init_params(model, xs, ss, **cfg).items()}


FAMILIES = [
    ('net_postupsampling', (1, 8, 8, 1), None, dict(backbone_block='resnet', upsampling='spc', scale=4, n_blocks=2)),
    ('net_postupsampling', (1, 8, 8, 1), (1, 16, 16, 1), dict(backbone_block='convnext', upsampling='rc', scale=2, n_blocks=2, normalization='bn')),
    ('net_pin', (1, 8, 8, 2), (1, 8, 8, 1), dict(backbone_block='densenet', n_blocks=2, attention=True, localcon_layer=True, normalization='ln')),
    ('unet_pin', (1, 16, 16, 3), (1, 16, 16, 1), dict(n_filters=4, n_blocks=2, decoder_upsampling='dc')),
    ('recnet_postupsampling', (1, 3, 6, 6, 1), (1, 12, 12, 1), dict(backbone_block='densenet', upsampling='rc', scale=2, time_window=3, n_filters=4, n_blocks=1, attention=True, localcon_layer=True)),
    ('recnet_pin', (1, 2, 6, 6, 2), None, dict(backbone_block='resnet', time_window=2, n_filters=4, n_blocks=1)),
]


@pytest.mark.parametrize('model,xs,ss,cfg', FAMILIES)
def test_default_decayed_set(model, xs, ss, cfg):
    params = _oracle_params(model, xs, ss, **dict(cfg))
    dec = decayed_parameters(params)
    assert dec and len(dec) == len(set(dec))                             # nothing twice
    for k in dec:
        assert len(params[k]) >= 2, k
        leaf = k.rsplit('/', 1)[-1]
        assert leaf not in ('bias', 'gamma', 'beta', 'moving_mean', 'moving_variance'), k
    for k, shape in params.items():
        if k not in dec:                                                 # every kernel IS decayed: what is left out has one
            assert len(shape) <= 1 or k.endswith('/bias'), (k, shape)    # dimension or is the (H, W, F) bias of a localized conv
    assert [k for k in params if k in dec] == dec                        # parameter order


def test_decayed_set_trainable_flag_and_filter():
    params = {'c/kernel': dict(shape=(3, 3, 1, 8), trainable=True), 'c/bias': dict(shape=(8,), trainable=True),
              'bn/gamma': dict(shape=(8,)), 'bn/moving_mean': dict(shape=(8,), trainable=False),
              'frozen/kernel': dict(shape=(1, 1, 8, 8), trainable=False), 'd/kernel': dict(shape=(8, 4)),
              'loc/bias': dict(shape=(4, 4, 2))}
    assert decayed_parameters(params) == ['c/kernel', 'd/kernel']
    assert default_decay_filter('x', (3, 3)) and not default_decay_filter('x', (3,)) and not default_decay_filter('x', ())
    assert not default_decay_filter('LocalizedConvBlock/localconv/bias', (4, 4, 2))
    seen = []
    only_dense = decayed_parameters(params, lambda name, shape: seen.append((name, shape)) or len(shape) == 2)
    assert only_dense == ['d/kernel'] and ('c/bias', (8,)) in seen
    assert decayed_parameters(params, lambda name, shape: True) == ['c/kernel', 'c/bias', 'bn/gamma', 'd/kernel', 'loc/bias']


def test_range_table_is_sorted_and_merged():
    assert merge_ranges([]) == []
    assert merge_ranges([(7, 1022), (0, 5)]) == [(0, 5), (7, 1022)]
    assert merge_ranges([(0, 4), (4, 8), (8, 9)]) == [(0, 9)]                      # adjacent
    assert merge_ranges([(0, 6), (2, 4), (5, 10), (12, 12)]) == [(0, 10)]          # nested, overlapping, empty
    assert merge_ranges([(3, 4), (1, 2)]) == [(1, 2), (3, 4)]
    with pytest.raises(ValueError):
        merge_ranges([(4, 2)])
    # parameters of an arena whose slices are padded to four elements touch only where the size is a multiple of four
    assert merge_ranges([(0, 72), (72, 80), (84, 90)]) == [(0, 80), (84, 90)]
    for n in C.SIZES:
        for s in C.decay_range_sets(n):
            assert merge_ranges(s) == s and all(0 <= b < e <= n for b, e in s)


def test_launch_figures_match_the_source():
    assert C.norm_figures_in_source() == (C.NORM_THREADS, C.NORM_BLOCK_CAP)
    per_pass = 4 * C.NORM_THREADS * C.NORM_BLOCK_CAP
    assert per_pass < C.NORM_LARGEST < per_pass + 4 * C.NORM_THREADS * 4 and C.NORM_LARGEST % 4 == 3
    assert C.norm_blocks(C.NORM_LARGEST) == C.NORM_BLOCK_CAP and C.norm_blocks(1) == 1 and C.norm_blocks(1025) == 2
    assert C.SIZES[:8] == (1, 2, 3, 4, 5, 1023, 1025, 2051)
    src = S._src('adam.hip')
    assert 'adam_ext' not in src                                         # the old kernel's file is what it was


# ---------------------------------------------------------------------------------------------------------------- reference
def test_reference_clip_one_element():
    """g = 3, clip = 1: norm 3, c = fl32(1 / 3); the first Adam step moves w by lr_t * m' / (sqrt(v') + eps) with gr = 3 c = 1."""
    assert R.global_norm64(np.array([3.0], F32), 1.0) == 3.0
    c = R.clip_factor32(3.0, 1.0)
    assert c == F32(1.0) / F32(3.0) and R.clip_factor32(0.5, 1.0) == 1.0 and R.clip_factor32(1.0, 1.0) == 1.0
    z = np.zeros(1, F32)
    out = R.step_ref(np.array([2.0], F32), np.array([3.0], F32), z, z, None, 1, 1.0, c, 0.0, None, 0.0)
    b1, b2, eps, lr_t = R.adam_consts(1)
    gr = 3.0 * F64(c)
    assert abs(gr - 1.0) < 1e-7
    assert out['m'][0][0] == (1 - b1) * gr and out['v'][0][0] == (1 - b2) * gr * gr
    want = 2.0 - lr_t * (1 - b1) * gr / (np.sqrt((1 - b2) * gr * gr) + eps)
    assert abs(out['w'][0][0] - want) < 1e-15
    assert abs((2.0 - out['w'][0][0]) - S.ADAM_LR) < 1e-8                 # the first Adam step is lr * sign(g) up to eps
    assert 'ema' not in out and out['w'][1][0] > 0


def test_reference_decay_only_step():
    """g = m = v = 0: Adam moves nothing, the decayed element becomes w (1 - lr wd), the other stays w with a zero bound."""
    w = np.array([2.0, -4.0], F32)
    z = np.zeros(2, F32)
    out = R.step_ref(w, z, z, z, None, 5, 1.0, F32(1), 0.5, np.array([True, False]), 0.0)
    lw = F64(F32(F32(S.ADAM_LR) * F32(0.5)))
    assert out['w'][0][0] == 2.0 - lw * 2.0 and out['w'][0][1] == -4.0
    assert abs(out['w'][0][0] - 2.0 * (1 - 0.5e-3)) < 1e-9
    assert out['w'][1][0] > 0 and out['w'][1][1] == S.ADAM_BOUND * 4.0     # no decay term outside the set
    assert (out['m'][0] == 0).all() and (out['v'][0] == 0).all()


def test_reference_ema_after_two_steps():
    """mu = 0.5, the average starts at w0 = 1: after weights 3 then 5 it is 0.5 (0.5 * 1 + 0.5 * 3) + 0.5 * 5 = 3.5."""
    e0 = np.array([1.0], F32)
    e1, b1 = R.ema_ref(e0, np.array([3.0], F32), 0.5)
    e2, b2 = R.ema_ref(e1, np.array([5.0], F32), 0.5)
    assert e1[0] == 2.0 and e2[0] == 3.5
    assert b1[0] == S.ADAM_BOUND * 2.0 and b2[0] == S.ADAM_BOUND * 3.5
    z = np.zeros(1, F32)
    out = R.step_ref(e0, z, z, z, e0, 1, 1.0, F32(1), 0.0, None, 0.5)
    assert out['ema'][0][0] == 1.0                                       # nothing moves: the average of equal values


def test_reference_ratios_zero_bound_must_be_exact():
    ref = {'w': (np.array([1.0, 2.0]), np.array([0.0, 0.5]))}
    assert R.ratios({'w': np.array([1.0, 2.25])}, ref)['w'] == 0.5
    assert R.ratios({'w': np.array([1.0 + 1e-9, 2.0])}, ref)['w'] == np.inf
    assert R.decay_mask(6, [(1, 2), (4, 6)]).tolist() == [False, True, False, False, True, True]
