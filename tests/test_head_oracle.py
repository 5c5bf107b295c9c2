"""CPU checks of tests/head_ref.py and tests/head_cases.py: the references against independent evaluations (torch autograd in fp64,
explicit loops, known splitmix64 outputs), the dispatch restated in the case tables against the source, and every condition the GPU
tests of tests/test_gpu_head.py rely on -- so that those are verified without a GPU."""
import numpy as np
import pytest
import torch

from tests import head_cases as K
from tests import head_ref as R

F32, F64 = np.float32, np.float64


# ------------------------------------------------------------------------------------------------------------------- noise
def test_splitmix64_known_answers():
    """The first outputs of the SplitMix64 generator seeded with 0 are the hashes of GOLDEN, 2 * GOLDEN, 3 * GOLDEN."""
    want = [0xE220A8397B1DCDAF, 0x6E789E6AA1B965F4, 0x06C45D188009454F]
    assert [R.op_seed(0, i) for i in range(3)] == want
    z = np.array([R.GOLDEN * (i + 1) & (2 ** 64 - 1) for i in range(3)], np.uint64)
    assert [int(v) for v in R.splitmix64(z)] == want


def test_scheme_constants_match_the_source():
    graph_h, ops2, head, capi = (K.source(f) for f in ('graph.h', 'graph_ops2.hip', 'head.hip', 'capi.cpp'))
    assert f'DROPOUT_BUILTIN_SEED = 0x{R.BUILTIN_SEED:X}ull' in graph_h
    assert f'0x{R.GOLDEN:X}ull * (unsigned long long)(index + 1)' in graph_h
    assert f'(++counter) * 0x{R.DRAW_STEP:X}ull' in ops2
    assert f'seed + 0x{R.GOLDEN:X}ull * (e + 1)' in head
    # one helper seeds both the un-reseeded ops and the reseeded ones
    assert 'dropout_op_seed(DROPOUT_BUILTIN_SEED, g.dropout_ops.size())' in ops2
    assert 'reseed(dropout_op_seed(seed, i))' in capi
    assert K.noise_grid_threads_in_source() == K.NOISE_GRID_THREADS
    assert K.mask_size(K.LARGE_MASK) > K.NOISE_GRID_THREADS > K.mask_size(K.INDEP_MASK)
    assert K.RESEEDS[1] >> 63 == 1 and K.RESEEDS[0] >> 63 == 0


@pytest.mark.parametrize('rate', K.RATES + (0.05, 0.25, 0.3))
def test_keep_threshold(rate):
    """The float32 comparison u >= rate is the integer comparison m >= ceil(float32(rate) * 2^24).  The double value of the rate gives
    the same threshold or the next one (0.9: float32(0.9) * 2^24 is the integer 15099494): 2^-24 in the keep probability, four
    orders below the frequency test's bound."""
    thr = R.keep_threshold(rate)
    assert 0 <= int(np.ceil(rate * 2.0 ** 24)) - thr <= 1
    for m in (thr - 1, thr):
        assert (F32(m) * F32(2.0 ** -24) >= F32(rate)) == (m >= thr)
    assert R.keep_probability(0.5) == 0.5 and R.gaussian_sigma(0.5) == 1.0


def test_replica_frequencies():
    n = K.mask_size(K.LARGE_MASK)
    for i, rate in enumerate(K.RATES):
        p, sigma = R.keep_probability(rate), R.gaussian_sigma(rate)
        keep = R.keep_mask(R.builtin_seed(i), 1, n, rate)
        assert abs(keep.mean() - p) <= 6.0 * np.sqrt(p * (1 - p) / n)
        z = R.gaussian_mask(R.builtin_seed(i), 1, n, rate)
        assert abs(z.mean() - 1.0) <= 6.0 * sigma / np.sqrt(n)
        assert abs(z.var() - sigma ** 2) <= 6.0 * sigma ** 2 * np.sqrt(2.0 / n)


@pytest.mark.parametrize('gaussian', [False, True], ids=['keep', 'gaussian'])
def test_fixed_scheme_meets_the_independence_bounds(gaussian):
    """The replica of the scheme, for exactly the seeds tests/test_gpu_head.py::test_noise_streams_are_independent uses (fixed seeds:
    a deterministic check): built-in and reseeded, nine streams each, 612 comparisons."""
    n = K.mask_size(K.INDEP_MASK)
    check = R.correlation_violations if gaussian else R.agreement_violations
    for seed_of_op in (R.builtin_seed, lambda i: R.op_seed(K.INDEP_RESEED, i)):
        bad, count = check(K.replica_streams(seed_of_op, n, K.INDEP_RATE, gaussian))
        assert count == 612 and not bad, bad[:6]


@pytest.mark.parametrize('gaussian', [False, True], ids=['keep', 'gaussian'])
def test_old_builtin_scheme_violates_them(gaussian):
    """What was fixed: with s_i = BUILTIN + GOLDEN * (i + 1) the mask of op i + 1 is the mask of op i shifted by one element, at every
    draw -- agreement 1.0 (correlation 1.0) one element apart between neighbouring ops, two apart between ops 0 and 2."""
    n = K.mask_size(K.INDEP_MASK)
    streams = K.replica_streams(R.old_builtin_seed, n, K.INDEP_RATE, gaussian)
    nd = len(K.DRAWS)
    for i in range(K.N_OPS - 1):
        for k in range(nd):
            np.testing.assert_array_equal(streams[(i + 1) * nd + k][:-1], streams[i * nd + k][1:])
    bad, count = (R.correlation_violations if gaussian else R.agreement_violations)(streams)
    assert count == 612
    shifted = {(i, j, lag) for i, j, lag, score, _ in bad if abs(score - 1.0) < 1e-12}
    # (stream a at element e against stream b at element e + lag: op b holds op a's mask b - a elements EARLIER, lag = a - b)
    assert shifted == {(a * nd + k, b * nd + k, a - b) for a in range(K.N_OPS) for b in range(a + 1, K.N_OPS) for k in range(nd)}
    # the issue's own example
    m0, m1 = (R.keep_mask(R.old_builtin_seed(i), 1, 4096, 0.4) for i in (0, 1))
    np.testing.assert_array_equal(m1[:-1], m0[1:])


def test_draws_of_one_op_cannot_line_up():
    """Two draws of one op read the same hash inputs only at the element shift s = dk * DRAW_STEP / GOLDEN (mod 2^64): for every
    distance dk below 2 000 000 draws |s| is beyond 2^43 elements (csrc/graph.h quotes the figures)."""
    s = R.draw_alignment_shifts(1_999_999)
    assert s.min() == 8924847125489.0 and int(np.argmin(s)) + 1 == 98199 and s.min() > 2.0 ** 43
    assert s[:65535].min() > 1.8e14
    # and the offset is what the replica applies: draw k of seed s is draw 1 of seed s + (k - 1) * DRAW_STEP
    np.testing.assert_array_equal(R.hash_bits(12345, 3, 64), R.hash_bits(12345 + 2 * R.DRAW_STEP, 1, 64))


# ------------------------------------------------------------------------------------------------------------------- dropout apply
def test_dropout_apply_references():
    shape = (2, 3, 2, 2, 5)
    b, t, h, w, c = shape
    for dim, mshape in ((2, (b * t, c)), (3, (b, c))):
        mask = np.arange(np.prod(mshape), dtype=F32).reshape(mshape)
        full = R.broadcast_mask(mask, shape, dim)
        # dropout_apply_bcast_kernel's indexing: element e of block q = e / (inner * C) uses mask[q * C + e % C]
        inner = h * w * (t if dim == 3 else 1)
        e = np.arange(np.prod(shape))
        np.testing.assert_array_equal(full.ravel(), mask.ravel()[(e // (inner * c)) * c + e % c])
    assert R.dropout_scale(0.4, False) == F32(1.0) / (F32(1.0) - F32(0.4)) and R.dropout_scale(0.4, True) == 1.0
    x = np.random.default_rng(0).standard_normal(shape).astype(F32)
    keep = K.irregular_keep(shape, 1, 0.4)
    assert 0.4 < keep.mean() < 0.8 and R.dropout_forward(x, keep, R.dropout_scale(0.4, False)).dtype == F32
    assert (K.gaussian_noise((3, 1, 9, 11, 5), 4, 0.05) > 0).all()          # the accumulate case of the GPU test: positive noise


# ------------------------------------------------------------------------------------------------------------------- bound
def test_sum_bound_holds_for_a_float32_chain_and_catches_a_lost_term():
    r = np.random.default_rng(0)
    for k in (1, 7, 40, 300):
        a, b = r.standard_normal((64, k)).astype(F32), r.standard_normal((64, k)).astype(F32)
        s = np.zeros(64, F32)
        for j in range(k):
            s = s + a[:, j] * b[:, j]
        terms = np.abs(a.astype(F64) * b.astype(F64))
        ref = (a.astype(F64) * b.astype(F64)).sum(axis=1)
        bound = R.sum_bound(k, terms.sum(axis=1), ref)
        assert (np.abs(s.astype(F64) - ref) <= bound).all()
        if k > 1:                # one term of typical size left out is far outside
            j = np.argmax(terms, axis=1)
            lost = ref - (a.astype(F64) * b.astype(F64))[np.arange(64), j]
            assert (np.abs(lost - ref) > 100 * bound).all()
    assert R.worst(np.array([1.0, 0.0]), np.array([1.0, 0.0]), np.array([0.0, 0.0]))[0] == 0.0
    assert R.worst(np.array([1.0, 1e-30]), np.array([1.0, 0.0]), np.array([0.0, 0.0]))[0] > 1.0


# ------------------------------------------------------------------------------------------------------------------- Dense
def _t(a):
    return torch.tensor(np.asarray(a, F64), requires_grad=True)


def _torch_act(z, act):
    return {None: lambda v: v, 'sigmoid': torch.sigmoid, 'relu': torch.relu, 'tanh': torch.tanh}[act](z)


@pytest.mark.parametrize('act', R.ACTS)
@pytest.mark.parametrize('case', K.DENSE_CASES)
def test_dense_reference_and_inputs(case, act):
    """The fp64 reference against torch autograd, and the condition of the ReLU cases: no pre-activation within 1e-4 of 0."""
    b, cin, f, nmul = case
    x, w, bias, _ = K.dense_case_inputs(case)
    assert x.shape == (b * nmul, cin) and w.shape == (cin, f)
    z, y, bound = R.dense_forward(x, w, bias, act)
    assert np.abs(z).min() >= K.KINK_MARGIN
    if f * b * nmul >= 6:
        assert (z > 0).any() and (z < 0).any()
    tx, tw, tb = _t(x), _t(w), _t(bias)
    ty = _torch_act(tx @ tw + tb, act)
    np.testing.assert_allclose(y, ty.detach().numpy(), rtol=1e-13, atol=1e-300)
    _, dy = R.mse_targets(y.astype(F32), 5)
    ty.backward(torch.tensor(dy))
    ref = R.dense_backward(x, w, y, dy, act)
    for name, t in (('dW', tw), ('db', tb), ('dX', tx)):
        np.testing.assert_allclose(ref[name][0], t.grad.numpy(), rtol=1e-11, atol=1e-18)
        assert (ref[name][1] > 0).all()
    # the float32 forward of numpy itself stays inside the forward bound
    y32 = R.act_fwd((x @ w + bias).astype(F64), act)
    assert (np.abs(y32 - y) <= bound).all()


@pytest.mark.parametrize('case', K.DENSE_SHARED_CASES)
def test_dense_shared_inputs(case):
    x, heads, _ = K.dense_shared_inputs(case)
    for w, bias in heads:
        assert np.abs(x.astype(F64) @ w.astype(F64) + bias.astype(F64)).min() >= K.KINK_MARGIN


def test_mse_targets():
    y = np.random.default_rng(1).standard_normal((9, 32)).astype(F32)
    t, dy = R.mse_targets(y, 5)
    assert t.dtype == F32 and 0.4 < np.abs(y - t).min() and np.abs(y - t).max() < 1.6
    np.testing.assert_array_equal(dy, 2.0 * (y - t).astype(F64) / y.size)
    assert (dy > 0).any() and (dy < 0).any()


# ------------------------------------------------------------------------------------------------------------------- GAP
def test_gap_dispatch_restated():
    assert K.gap_dispatch_in_source() == (K.GAP_CHUNKS, 256, K.GAP_CHUNKED_MIN_HW)
    paths = {case: K.gap_path(case[2] * case[3] * (case[1] if case[5] else 1), case[4]) for case in K.GAP_FWD_CASES}
    assert paths[(2, 1, 64, 64, 20, False)] == ('partial4', (5, 51, 1))            # float4 packs, CP = 5, one idle thread
    assert paths[(2, 1, 64, 64, 7, False)] == ('partial1', (7, 36, 4))             # scalar packs, four idle threads
    assert paths[(2, 1, 64, 64, 260, False)] == ('partial4', (65, 3, 61))
    assert paths[(2, 1, 64, 64, 1028, False)] == ('per_nc', None)                  # CP = 257
    assert paths[(2, 3, 48, 40, 8, True)][0] == 'partial4'
    for c in (20, 7, 260):
        assert paths[(2, 1, 63, 65, c, False)] == ('per_nc', None)                 # HW = 4095
    assert paths[(2, 1, 3, 2, 5, False)] == ('per_nc', None)
    used = {(K.gap_bwd_kernel_of(c[5], c[6]), c[6], c[8]) for c in K.GAP_BWD_CASES}
    for kernel, relu in (('gap_bwd4_kernel', True), ('gap_bwd4_kernel', False), ('gap_bwd_masked_kernel', True), ('gap_bwd_kernel', False)):
        assert (kernel, relu, False) in used and (kernel, relu, True) in used      # every kernel with and without accumulate
    assert any(c[7] and c[6] for c in K.GAP_BWD_CASES)                             # an over_time masked case


@pytest.mark.parametrize('case', K.GAP_FWD_CASES)
def test_gap_forward_inputs(case):
    n, t, h, w, c, over_time = case
    x = K.gap_fwd_input(case)
    ref = R.gap_forward(x, over_time)
    assert ref.shape == ((n, c) if over_time else (n, t, c)) and 9.0 < ref.min() and ref.max() < 101.0
    np.testing.assert_allclose(ref, torch.tensor(x, dtype=torch.float64).mean(dim=(1, 2, 3) if over_time else (2, 3)).numpy(), rtol=1e-13)


@pytest.mark.parametrize('case', K.GAP_BWD_CASES)
def test_gap_backward_reference_and_inputs(case):
    """The fp64 reference against torch autograd, and the condition of the masked cases: no value of xW + b within 1e-4 of 0."""
    n, t, h, w, cin, c, relu, over_time, twice = case
    x, wk, bias, _ = K.gap_bwd_inputs(case)
    z, feat = R.gap_feat(x, wk, bias, relu)
    assert np.abs(z).min() >= K.KINK_MARGIN and 0.2 < (z > 0).mean() < 0.8
    tx, tw, tb = _t(x), _t(wk), _t(bias)
    tf = tx @ tw + tb
    tf = torch.relu(tf) if relu else tf
    pooled = tf.mean(dim=(1, 2, 3) if over_time else (2, 3))
    np.testing.assert_allclose(R.gap_forward(feat, over_time), pooled.detach().numpy(), rtol=1e-12)
    out = torch.cat([pooled, pooled], dim=-1) if twice else pooled
    _, dy = R.mse_targets(out.detach().numpy().astype(F32), 7)
    out.backward(torch.tensor(dy))
    ref = R.gap_backward(x, wk, z, [dy[..., :c], dy[..., c:]] if twice else [dy], over_time, relu)
    for name, tt in (('dW', tw), ('db', tb), ('dX', tx)):
        np.testing.assert_allclose(ref[name][0], tt.grad.numpy(), rtol=1e-10, atol=1e-18)
        assert ref[name][1].shape == ref[name][0].shape
    if relu:                     # a masked element of dfeat is exactly 0: dX is exactly 0 where every channel is masked
        dead = (z <= 0).all(axis=-1)
        assert (ref['dX'][0][dead] == 0).all()
