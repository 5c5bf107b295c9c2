"""Data-parallel path on real hardware: the fail-safe (a rank without a communicator refuses to train), host-side
reductions on a 1-rank communicator, bench.py's self-launcher, and -- when the box has two or more GPUs -- two real
ranks over RCCL: the reduced gradient is the mean of the per-rank gradients and the replicas stay bit-identical.
Every case runs in child processes so that communicators and WORLD_SIZE never leak into the other tests."""
import json
import os
import subprocess
import sys
import textwrap

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(code, env=None, timeout=900):
    e = {k: v for k, v in os.environ.items() if k not in ('WORLD_SIZE', 'RANK', 'LOCAL_RANK', 'DL4DS_ALLOW_UNSYNCED')}
    e.update(env or {})
    return subprocess.run([sys.executable, '-c', textwrap.dedent(code) % {'root': ROOT}], capture_output=True, text=True,
                          timeout=timeout, env=e)


def _device_count():
    import ctypes
    import dl4ds_amd._lib as L
    n = ctypes.c_int()
    try:
        L.check(L.load().dl4ds_device_count(ctypes.byref(n)))
    except L.Dl4dsHipError:          # no device visible: the skipif below is evaluated on machines without a GPU, too
        return 0
    return n.value


STEP = '''
    import sys, numpy as np
    sys.path.insert(0, %(root)r)
    import dl4ds_amd.models as PM
    from dl4ds_amd.training import SupervisedEngine, CGANEngine
    from dl4ds_amd import parallel, _lib
    rng = np.random.default_rng(0)
    x = rng.standard_normal((2, 16, 16, 1)).astype(np.float32)
    y = rng.standard_normal((2, 64, 64, 1)).astype(np.float32)
    m = PM.net_postupsampling('resnet', 'spc', 4, 1, 0, (16, 16), n_blocks=2, seed=5)
    e = SupervisedEngine(m, loss='mae', learning_rate=1e-3)
'''


def test_step_without_communicator_is_refused_when_launched_as_one_of_several_ranks():
    """VERDICT r1 'missing' #2: WORLD_SIZE=2 and nobody created the communicator -> dl4ds_trainer_step, dl4ds_cgan_step
    and dl4ds_dist_broadcast_trainer return an error (they used to fall back to silent local training)."""
    r = _run(STEP + '''
    for name, call in (('step', lambda: e.step([x], y)), ('broadcast', lambda: parallel.broadcast_trainer(e))):
        try:
            call()
        except _lib.Dl4dsHipError as err:
            assert 'WORLD_SIZE=2' in str(err) and 'no RCCL communicator' in str(err), str(err)
            print('REFUSED', name)
    print('LOSS-OK', e.loss_and_grads([x], y)[0] > 0)          # local gradients (no update) are still allowed
    H = 16
    gen = PM.unet_pin('unet', 2, 1, hr_size=(H, H), n_filters=4, n_blocks=2, decoder_upsampling='dc', seed=3)
    disc = PM.residual_discriminator(2, 'pin', False, 8, (H // 8, H // 8), n_filters=4, n_res_blocks=1, hr_size=(H, H), seed=4)
    c = CGANEngine(gen, disc, loss='mae')
    lr, st, hr = (rng.random((2, H, H, k)).astype(np.float32) for k in (2, 1, 1))
    try:
        c.step([lr, st], hr)
    except _lib.Dl4dsHipError as err:
        print('REFUSED cgan')
    print('NOUPDATE-OK', len(c.step([lr, st], hr, apply_update=False)) == 4)
    ''', env={'WORLD_SIZE': '2', 'RANK': '0', 'LOCAL_RANK': '0'})
    out = r.stdout + r.stderr
    for tag in ('REFUSED step', 'REFUSED broadcast', 'LOSS-OK True', 'REFUSED cgan', 'NOUPDATE-OK True'):
        assert tag in r.stdout, out[-3000:]


def test_unsynced_replicas_are_an_explicit_opt_in():
    r = _run(STEP + '''
    print('STEP-OK', np.isfinite(e.step([x], y)))
    ''', env={'WORLD_SIZE': '2', 'RANK': '1', 'LOCAL_RANK': '0', 'DL4DS_ALLOW_UNSYNCED': '1'})
    assert 'STEP-OK True' in r.stdout, (r.stdout + r.stderr)[-3000:]


def test_trainer_constructor_brings_up_the_communicator_like_hvd_init():
    """Trainer.__init__ calls parallel.init_from_env (training/base.py:97-107 calls hvd.init()): a one-rank 'job'
    (WORLD_SIZE=1) stays local; the communicator checks run in the 2-GPU test below."""
    r = _run('''
    import sys, numpy as np
    sys.path.insert(0, %(root)r)
    from dl4ds_amd.training import SupervisedTrainer
    from dl4ds_amd import parallel
    rng = np.random.default_rng(0)
    d = lambda n: rng.random((n, 16, 16, 1)).astype(np.float32)
    t = SupervisedTrainer('resnet', 'spc', d(8), d(4), d(4), scale=2, batch_size=2, epochs=1, verbose=False, n_blocks=1,
                          n_filters=4, save=False)
    assert (t.rank, t.world) == (0, 1) and not parallel.is_initialized()
    t.run()
    print('LOCAL-OK', np.isfinite(t.test_loss))
    ''', env={'WORLD_SIZE': '1', 'RANK': '0'})
    assert 'LOCAL-OK True' in r.stdout, (r.stdout + r.stderr)[-3000:]


def test_host_reductions_and_comm_info_on_a_one_rank_communicator():
    r = _run('''
    import sys
    sys.path.insert(0, %(root)r)
    from dl4ds_amd import parallel
    assert parallel.allreduce_host([1.5, -2.0], 'max') == [1.5, -2.0]          # identity without a communicator
    assert parallel.comm_info()['nranks'] == 0
    parallel.init_with_id(0, 1, parallel.unique_id())
    info = parallel.comm_info()
    assert info['nranks'] == 1 and info['rank'] == 0 and info['device'] >= 0, info
    for op in ('sum', 'max', 'min', 'mean'):
        assert parallel.allreduce_host([1.5, -2.0, 3.0], op) == [1.5, -2.0, 3.0], op
    parallel.barrier()
    parallel.finalize()
    assert not parallel.is_initialized()
    print('HOST-RED-OK')
    ''')
    assert 'HOST-RED-OK' in r.stdout, (r.stdout + r.stderr)[-3000:]


def test_bench_runs_when_invoked_directly_with_gpus_flag():
    """`python bench.py --gpus N` must work without torch.distributed.run (VERDICT r1 'missing' #3): N = 1 always, N = 2
    through the self-launcher when the box has two GPUs."""
    env = {k: v for k, v in os.environ.items() if k not in ('WORLD_SIZE', 'RANK', 'LOCAL_RANK')}
    for n in ([1, 2] if _device_count() >= 2 else [1]):
        r = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py'), '--gpus', str(n), '--steps', '2', '--warmup', '1',
                            '--batch', '4', '--full', '--no-cpu-baseline', '--no-unfolded'], capture_output=True, text=True,
                           timeout=1200, env=env)
        assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
        line = [l for l in r.stdout.splitlines() if l.startswith('{')][-1]
        out = json.loads(line)
        assert out['n_gpus'] == n and out['value'] > 0 and out['config']['global_batch'] == 4 * n
        assert out['roofline'] and out['roofline']['frac'] > 0 and 'reference_equivalent_tflops' not in out
        assert out['hbm_kernels'], out
        if n > 1:
            assert out['rccl']['nranks'] == n


def test_plain_bench_run_times_the_steps_only_and_dumps_what_the_last_step_returned(tmp_path):
    """A plain run (no --full): the K timed steps and nothing else on the line; --dump-outputs writes the loss and the updated
    weights of the last timed step as float32 .npy files."""
    env = {k: v for k, v in os.environ.items() if k not in ('WORLD_SIZE', 'RANK', 'LOCAL_RANK')}
    d = tmp_path / 'out'
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py'), '--gpus', '1', '--steps', '3', '--warmup', '1',
                        '--batch', '4', '--dump-outputs', str(d)], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    out = json.loads([l for l in r.stdout.splitlines() if l.startswith('{')][-1])
    assert out['steps'] == 3 and out['warmup'] == 1 and out['ms_per_step'] > 0
    assert abs(out['value'] - 4 / (out['ms_per_step'] * 1e-3)) < 1e-6 * out['value']
    assert out['roofline'] is None and out['steady_state'] is None and out['cpu_baseline'] is None and out['hbm_kernels'] is None
    assert 'b16' not in out and 'unfolded_graph' not in out
    files = sorted(os.listdir(d))
    assert set(files) == set(out['dump_outputs']['arrays']) and len(files) == 1 + 56, files
    assert sum(os.path.getsize(d / f) for f in files) < 64 << 20
    loss = np.load(d / 'loss.npy')
    assert loss.dtype == np.float32 and loss.shape == (1,) and loss[0] == np.float32(out['config']['loss_after_run'])
    for f in files:
        a = np.load(d / f)
        assert a.dtype == np.float32 and np.isfinite(a).all(), f
    assert np.load(d / 'weights.stem.kernel.npy').shape == tuple(out['dump_outputs']['arrays']['weights.stem.kernel.npy']['shape'])


TWO_RANK = '''
    import os, sys, numpy as np
    sys.path.insert(0, %(root)r)
    import dl4ds_amd.models as PM
    from dl4ds_amd.training import SupervisedEngine
    from dl4ds_amd import parallel, _lib
    rank, world = parallel.init_from_env()
    assert parallel.comm_info() == {'nranks': 2, 'rank': rank, 'device': rank}
    rng = np.random.default_rng(100 + rank)                       # a different batch on every rank
    x = rng.standard_normal((2, 16, 16, 1)).astype(np.float32)
    y = rng.standard_normal((2, 64, 64, 1)).astype(np.float32)
    m = PM.net_postupsampling('resnet', 'spc', 4, 1, 0, (16, 16), n_blocks=2, seed=5 + rank)    # different init, too
    e = SupervisedEngine(m, loss='mae', learning_rate=1e-3)
    parallel.broadcast_trainer(e)                                 # rank 0's weights everywhere
    w0 = m.get_weights()
    _, g_local = e.loss_and_grads([x], y)                         # this rank's gradients, no update
    import ctypes
    wp, gp, n_arena, n_par = ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_size_t(), ctypes.c_int()
    L = _lib.lib()
    _lib.check(L.dl4ds_graph_arena_ptrs(m.graph.h, ctypes.byref(wp), ctypes.byref(gp)))
    _lib.check(L.dl4ds_graph_param_count(m.graph.h, ctypes.byref(n_arena), ctypes.byref(n_par)))
    _lib.check(L.dl4ds_dist_allreduce_sum(gp, n_arena.value))     # the collective the train step issues per bucket
    _lib.check(L.dl4ds_sync())
    g_sum = m.get_gradients()
    out = os.environ['OUT_DIR']
    losses = [e.step([x], y)]
    w1 = m.get_weights()
    losses += [e.step([x], y) for _ in range(2)]
    np.savez(os.path.join(out, f'rank{rank}.npz'), **{'w0/' + k: v for k, v in w0.items()},
             **{'g/' + k: v for k, v in g_local.items()}, **{'w3/' + k: v for k, v in m.get_weights().items()},
             **{'gsum/' + k: v for k, v in g_sum.items()}, **{'w1/' + k: v for k, v in w1.items()})
    assert parallel.allreduce_host([float(rank + 1)], 'sum') == [3.0]
    assert parallel.allreduce_host([float(rank + 1)], 'max') == [2.0]
    parallel.barrier()
    parallel.finalize()
    print('RANK-OK', rank)
'''


@pytest.mark.skipif('_device_count() < 2', reason='needs two GPUs (RCCL refuses two ranks on one device)')
def test_two_real_ranks_average_gradients_and_stay_identical(tmp_path):
    import socket
    s = socket.socket()
    s.bind(('127.0.0.1', 0))
    port = s.getsockname()[1]
    s.close()
    procs = []
    for r in range(2):
        env = {k: v for k, v in os.environ.items() if k != 'DL4DS_ALLOW_UNSYNCED'}
        env.update(RANK=str(r), LOCAL_RANK=str(r), WORLD_SIZE='2', MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port),
                   OUT_DIR=str(tmp_path), HSA_ENABLE_IPC_MODE_LEGACY='0')
        procs.append(subprocess.Popen([sys.executable, '-c', textwrap.dedent(TWO_RANK) % {'root': ROOT}], env=env,
                                      stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True))
    outs = [p.communicate(timeout=900)[0] for p in procs]
    assert all(p.returncode == 0 for p in procs), '\n'.join(o[-2000:] for o in outs)
    z = [np.load(tmp_path / f'rank{r}.npz') for r in range(2)]
    names = [k[3:] for k in z[0].files if k.startswith('w0/')]
    for k in names:
        np.testing.assert_array_equal(z[0]['w0/' + k], z[1]['w0/' + k], err_msg='broadcast ' + k)
        np.testing.assert_array_equal(z[0]['w3/' + k], z[1]['w3/' + k], err_msg='replicas diverged: ' + k)
        assert not np.array_equal(z[0]['g/' + k], z[1]['g/' + k]) or not z[0]['g/' + k].any()
    lr, b1, b2, eps = 2e-3, 0.9, 0.999, 1e-7                      # supervised LR is scaled by world in the trainers; the
    for k in names:                                               # engine here was created with 1e-3 -> see below
        g0, g1 = z[0]['g/' + k].astype(np.float32), z[1]['g/' + k].astype(np.float32)
        for r in range(2):                                        # sum all-reduce: exact in fp32 for two ranks
            np.testing.assert_array_equal(z[r]['gsum/' + k], g0 + g1, err_msg='reduced gradient: ' + k)
        # first Keras-Adam step on the MEAN gradient (1/world folded into the Adam kernel)
        g = (g0.astype(np.float64) + g1) / 2
        m_ = (1 - b1) * g
        v_ = (1 - b2) * g * g
        lr_t = 1e-3 * np.sqrt(1 - b2) / (1 - b1)
        w1 = z[0]['w0/' + k] - lr_t * m_ / (np.sqrt(v_) + eps)
        np.testing.assert_allclose(z[0]['w1/' + k], w1, rtol=0, atol=2e-6, err_msg='Adam on the averaged gradient: ' + k)


def test_watchdog_polling_path_on_a_one_rank_communicator():
    """The host-side waits poll the stream (instead of blocking) when several ranks take part, so that a stranded peer fails
    loudly.  DL4DS_FORCE_WATCHDOG=1 takes that path with a 1-rank communicator: train steps with loss read-back, host
    reductions and dl4ds_sync must work through it -- in particular hipStreamQuery's hipErrorNotReady must not linger as the
    thread's last error and surface at the next kernel launch."""
    r = _run('''
        import sys, numpy as np
        sys.path.insert(0, %(root)r)
        from dl4ds_amd import parallel
        import dl4ds_amd.models as PM
        from dl4ds_amd.training import SupervisedEngine
        parallel.init_with_id(0, 1, parallel.unique_id())
        m = PM.net_postupsampling('resnet', 'spc', 2, 1, 0, (16, 16), n_blocks=1, n_filters=4, seed=1)
        eng = SupervisedEngine(m, loss='mae', learning_rate=1e-3)
        rng = np.random.default_rng(0)
        x = rng.standard_normal((2, 16, 16, 1)).astype(np.float32); y = rng.standard_normal((2, 32, 32, 1)).astype(np.float32)
        losses = [eng.step([x], y) for _ in range(5)]
        assert all(np.isfinite(losses)) and losses[-1] < losses[0], losses
        assert parallel.allreduce_host([3.0], 'max') == [3.0]
        parallel.barrier()
        parallel.finalize()
        print('WATCHDOG-OK')
    ''', env={'DL4DS_FORCE_WATCHDOG': '1'})
    assert r.returncode == 0 and 'WATCHDOG-OK' in r.stdout, r.stdout[-1500:] + r.stderr[-1500:]


def test_bucket_plans_of_the_benchmark_models_are_the_plan_of_survey_8e():
    """SURVEY section 8e as an invariant: the gradient arena goes out in buckets ordered by backward completion.
    cfg2 (0.82 MB): at least two buckets, and the one holding the arena's head -- the parameters the backward pass reaches last, i.e.
    the collective nothing is left to hide -- is cut at the first parameter boundary past 256 KB.  cfg5's generator (54.3 MB): seven buckets of a few MB (two hold one large deconvolution kernel each),
    the first one final while most of the backward pass is still to run; its discriminator (65 KB) is one small bucket.  The plan
    depends on the parameter arena only: cfg2's model is built on a small grid, cfg5's at its own size (no forward is run)."""
    import bench
    import dl4ds_amd.models as PM
    m2 = PM.net_postupsampling('resnet', 'spc', 4, 1, 0, (16, 16), seed=7)
    p2 = bench.bucket_plan(m2)
    assert m2.count_params() == 204405 and 4 * 204405 <= sum(p2['bytes']) <= 4 * 204405 + 16 * 64        # (16-byte aligned arena entries)
    assert p2['buckets'] >= 2
    ready = p2['final_after_backward_of_op']
    assert ready == sorted(ready) or ready == sorted(ready, reverse=True), ready        # buckets are contiguous arena ranges in op order
    head = ready.index(min(ready))                                            # the bucket the backward pass completes LAST
    assert p2['bytes'][head] <= 384 * 1024                                    # ... closes the step with a small message: it is cut at the
    #     first parameter boundary past 256 KB (Graph::plan_buckets; cfg2: 302 KB = stem ... ResidualBlock6)
    gen = PM.unet_pin('unet', 5, 1, hr_size=(512, 512), n_filters=8, n_blocks=6, decoder_upsampling='dc', seed=7)      # (no buffers until a forward)
    pg = bench.bucket_plan(gen)
    assert gen.count_params() == 13566325 and 4 * 13566325 <= sum(pg['bytes']) <= 4 * 13566325 + 16 * 256
    assert 5 <= pg['buckets'] <= 16, pg                                        # (7: 1.2 / 4.7 / 4.7 / 13.0 / 23.6 / 6.8 / ... MB)
    assert max(pg['bytes']) <= 24 * 2 ** 20                                   # (Dec1's 21.2 MB deconvolution kernel is one tensor)
    big = [b for b in pg['bytes'] if b >= 2 ** 20]
    assert len(big) >= 5 and 2.5e6 <= float(np.median(big)) <= 8e6, pg['bytes']
    ready = pg['final_after_backward_of_op']
    assert ready == sorted(ready) or ready == sorted(ready, reverse=True), ready
    assert max(ready) > 0.5 * pg['forward_ops']                               # the first collective starts in the first half of the backward pass
    disc = PM.residual_discriminator(5, 'pin', False, 8, (64, 64), n_filters=8, hr_size=(512, 512), seed=8)
    pd = bench.bucket_plan(disc)
    assert 4 * disc.count_params() <= sum(pd['bytes']) <= 80 * 1024 and pd['buckets'] <= 2


def test_persistent_convlstm_beside_collective_standins_does_not_time_out():
    """The persistent ConvLSTM recurrence needs all of its workgroups co-resident while kernels of the communication stream hold
    CUs (csrc/convlstm_seq.hip reserves CUs when a communicator exists).  No second rank is reachable from one GPU, so the
    collectives are played by DL4DS_DIST_STANDIN=1's stand-in kernels: every bucket launch of a 1-rank communicator is followed on
    the communication stream by a kernel that reads and rewrites the bucket, concurrent with the rest of the backward pass.  Five
    steps of a recurrent net: no spin gives up (the sticky device error word would fail a host wait), and losses and weights equal
    the local run bit for bit."""
    r = _run('''
        import sys, numpy as np
        sys.path.insert(0, %(root)r)
        import dl4ds_amd.models as PM
        from dl4ds_amd.training import SupervisedEngine
        from dl4ds_amd import parallel, _lib
        rng = np.random.default_rng(0)
        B, T, h, s = 4, 4, 32, 2
        x = rng.standard_normal((B, T, h, h, 1)).astype(np.float32)
        aux = rng.standard_normal((B, h * s, h * s, 1)).astype(np.float32)
        y = rng.standard_normal((B, T, h * s, h * s, 1)).astype(np.float32)
        def run(dist):
            m = PM.recnet_postupsampling('densenet', 'rc', s, 1, 1, (h, h), time_window=T, attention=True, localcon_layer=True,
                                         n_blocks=2, seed=7)
            e = SupervisedEngine(m, loss='mae', learning_rate=1e-3)
            if dist:
                parallel.broadcast_trainer(e)
            losses = [e.step([x, aux], y) for _ in range(5)]
            _lib.check(_lib.lib().dl4ds_sync())          # (a spin that gave up raises the sticky error word here)
            return losses, m.get_weights()
        l0, w0 = run(False)
        parallel.init_with_id(0, 1, parallel.unique_id())
        l1, w1 = run(True)
        parallel.finalize()
        assert l0 == l1, (l0, l1)
        for k in w0:
            np.testing.assert_array_equal(w0[k], w1[k], err_msg=k)
        print('SEQ-STANDIN-OK')
    ''', env={'DL4DS_DIST_STANDIN': '1'})
    assert 'SEQ-STANDIN-OK' in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
