#!/usr/bin/env python
"""Headline benchmark: HR samples/s of one full train step (forward + MAE + backward + [RCCL gradient
all-reduce] + Keras-Adam) of dl4ds's 4x residual-backbone sub-pixel SR model at 128->512 grids
(BASELINE.json configs[1]; configs[2] when run on N GPUs).

    python bench.py [--gpus N] [--steps K] [--warmup W] [--batch B_per_gpu] [--config cfg2|cfg4|cfg5] [--full]
                    [--dump-outputs DIR]

A plain run sets up, warms up (W steps), times the K steps and prints the line: `value` = HR samples/s over the K steps,
`ms_per_step` = milliseconds per timed step.  `--full` adds everything else the line can carry: the library profiler's per-kernel
figures (`roofline`, `step_roofline`, `hbm_kernels`, DL4DS_BENCH_BREAKDOWN=1's `breakdown`), the >= 2 s `steady_state` window and,
for cfg2 on one GPU, the unfolded graph, the per-GPU-batch-16 line and the CPU baseline (`--no-*` switch those off one by one).
`--dump-outputs DIR` writes what the last timed step returned to its caller -- the loss and the updated weights (cfg5: both
models' weights; `--predict`: the HR fields) -- as DIR/<name>.npy in float32; inputs and initial weights are seeded, so two
builds can be compared output for output.

`python bench.py --gpus N` (N > 1) starts the N ranks itself -- one process per GPU with RANK / LOCAL_RANK /
WORLD_SIZE / MASTER_ADDR / MASTER_PORT set -- and works just as well under a launcher that already did
(`python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 --master-port P bench.py
--gpus N ...`).  Rank bring-up is dl4ds_amd.parallel.init_from_env (RCCL id over a TCP socket); barriers and the
max-over-ranks time are RCCL collectives.  torch is imported only by the CPU baseline (the oracle) on rank 0 at N=1.

One JSON line on rank 0.  Inputs are synthetic, resident in HBM before the timed
region; weights are random-init (glorot) -- there is no dataset / checkpoint access.  fp32 throughout.
`--config cfg4` / `cfg5` time BASELINE.json configs[3] / configs[4] at their full sizes on one GPU (secondary
lines, same fields; the default and the driver's line is cfg2).
"""
import argparse
import ctypes
import json
import os
import socket
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

PEAK_FP32_MFMA_TFLOPS = 157.3          # MI355X_MICROARCH.md: v_mfma_f32_16x16x4_f32 dense peak
PEAK_HBM_GBPS = 8000.0                 # MI355X_MICROARCH.md: HBM3E spec (about 6.3 TB/s is achievable)
PEAK_BF16_MFMA_TFLOPS = 2500.0         # MI355X_MICROARCH.md: dense bf16 MFMA peak (only the opt-in conv_split kernel runs there)
ACHIEVABLE_HBM_GBPS = 6300.0           # MI355X_MICROARCH.md: measured float4 copy, the bandwidth term of the step-level bound
WINOGRAD_SAVING = 2.25                 # F(2x2,3x3): 16 multiplies per 2x2 tile and (cin, cout) pair instead of 36
MIN_STEADY_S = 2.0                     # the second timing window (`steady_state`) runs at least this long
# the cfg2 graph AS THE REFERENCE EVALUATES IT (layer by layer) is 18.336 GFLOP forward and
# 55.0 GFLOP per train step and sample.  The product composes spc.conv2x#2 (48 -> 4x48 at 256^2) with TransitionLast
# (1x1, 48 -> 8) into one 48 -> 4x8 convolution (csrc/graph_ops3.hip; DL4DS_NO_FOLD=1 disables it), which removes 27.2
# of those GFLOP.  Utilisation figures below use the FLOPs the kernels actually execute (library profiler).

# tags (prefixes) of the kernels north_star calls memory-bound: upsampling / attention / stencil tail / losses / Adam
HBM_KERNEL_PREFIXES = ('chatt', 'conv_direct', 'conv_narrow', 'resize', 'maxpool', 'localconv', 'pixel_loss', 'dssim',
                       'msdssim', 'bce', 'adam', 'relu_mask', 'view_axpy', 'masked_axpy', 'add_act', 'act_', 'bias_act',
                       'convlstm_gates', 'layernorm', 'batchnorm', 'gap', 'tail_')


def box_blur_fields(rng, shape_bhw, channels=1):
    """U[0,1) fields smoothed by a 5x5 box blur: (B,H,W,C) float64."""
    b, h, w = shape_bhw
    raw = rng.random((b, h + 4, w + 4, channels))
    cs = np.pad(raw.cumsum(axis=1).cumsum(axis=2), ((0, 0), (1, 0), (1, 0), (0, 0)))
    return (cs[:, 5:, 5:] - cs[:, :-5, 5:] - cs[:, 5:, :-5] + cs[:, :-5, :-5]) / 25.0


def block_mean(a, s):
    b, h, w, c = a.shape
    return a.reshape(b, h // s, s, w // s, s, c).mean(axis=(2, 4))


def synthetic_batch(seed, batch, hr=512, scale=4):
    """cfg2: HR y in U[0,1) box-blurred 5x5; LR x = scale x scale block mean."""
    y = box_blur_fields(np.random.default_rng(seed), (batch, hr, hr))
    return block_mean(y, scale).astype(np.float32), y.astype(np.float32)


def synthetic_batch_cfg4(seed, batch, T=8, h=64, s=4):
    """cfg4: T box-blurred HR frames per sample, LR = their block means, one HR auxiliary field -> (x, aux, y)."""
    rng = np.random.default_rng(seed)
    y = np.stack([box_blur_fields(rng, (batch, h * s, h * s)) for _ in range(T)], axis=1)          # (B,T,256,256,1)
    x = np.stack([block_mean(y[:, t], s) for t in range(T)], axis=1)
    aux = box_blur_fields(rng, (batch, h * s, h * s))
    return x.astype(np.float32), aux.astype(np.float32), y.astype(np.float32)


def synthetic_batch_cfg5(seed, batch, H=512):
    """cfg5 ('pin'): five 64^2 fields (block means of box-blurred 512^2 ones) re-expanded x 8, one HR static field, the HR target."""
    rng = np.random.default_rng(seed)
    y = box_blur_fields(rng, (batch, H, H))
    f = box_blur_fields(rng, (batch, H, H), channels=5)
    x = np.repeat(np.repeat(block_mean(f, 8), 8, axis=1), 8, axis=2)
    aux = box_blur_fields(rng, (batch, H, H))
    return x.astype(np.float32), aux.astype(np.float32), y.astype(np.float32)


DUMP_MAX_ELEMS = 1 << 22               # --dump-outputs: a larger array is stored as a fixed, seeded sample of this many elements


def dump_outputs(out_dir, arrays):
    """--dump-outputs: {name: array} -> out_dir/<name>.npy (float32; float64 stays float64), '/' in a name -> '.'.  An array of more
    than DUMP_MAX_ELEMS elements is replaced by the elements at DUMP_MAX_ELEMS flat indices drawn without replacement by
    np.random.default_rng(0), in increasing order (the same indices for the same shape in every run).  -> {name: description}."""
    os.makedirs(out_dir, exist_ok=True)
    written = {}
    for name, a in arrays.items():
        a = np.asarray(a)
        a = a.astype(np.float64 if a.dtype == np.float64 else np.float32, copy=False)
        desc = {'shape': list(a.shape)}
        if a.size > DUMP_MAX_ELEMS:
            idx = np.sort(np.random.default_rng(0).choice(a.size, DUMP_MAX_ELEMS, replace=False))
            a = a.reshape(-1)[idx]
            desc['sample'] = f'{DUMP_MAX_ELEMS} elements at seeded flat indices (default_rng(0), sorted)'
        fname = name.replace('/', '.') + '.npy'
        np.save(os.path.join(out_dir, fname), a)
        written[fname] = desc
    return written


def csrc_sha():
    """Fingerprint of the kernel sources this run's library was built from (dl4ds_amd/csrc/*.{hip,cpp,h} + the C header), 16 hex
    digits.  profiles/traffic.json carries the fingerprint of the tree its PMC passes ran on: counters collected before a kernel
    changed are not this kernel's traffic.  (.git does not travel to the GPU box; the sources do.)"""
    import hashlib
    h = hashlib.sha256()
    d = os.path.join(ROOT, 'dl4ds_amd', 'csrc')
    for f in sorted(os.listdir(d)):
        if f.endswith(('.hip', '.cpp', '.h')):
            h.update(f.encode())
            h.update(open(os.path.join(d, f), 'rb').read())
    h.update(open(os.path.join(ROOT, 'include', 'dl4ds_hip.h'), 'rb').read())
    return h.hexdigest()[:16]


def one_socket_cpus():
    """The hardware threads of ONE socket, one per physical core (sysfs topology) -- the CPU baseline is pinned to them: spread
    over both sockets of the 2 x 64-core host with first-touch memory placement the same step ANTI-scaled (round 4: 9.9 / 7.2 /
    3.5 samples/s at 32 / 64 / 128 threads).  Falls back to the current affinity mask where sysfs is not readable."""
    try:
        allowed = sorted(os.sched_getaffinity(0))
    except AttributeError:
        return None
    cores = {}
    for c in allowed:
        base = f'/sys/devices/system/cpu/cpu{c}/topology/'
        try:
            pkg = int(open(base + 'physical_package_id').read())
            core = int(open(base + 'core_id').read())
        except (OSError, ValueError):
            return allowed
        cores.setdefault(pkg, {}).setdefault(core, c)            # first hardware thread of each core
    pkg = max(cores, key=lambda k: len(cores[k]))
    return sorted(cores[pkg].values())


def cgroup_cpu_quota():
    """CPUs' worth of time the container may use (cgroup v2 cpu.max / v1 cfs quota), or None when unlimited / unreadable.  Found in
    round 6: the GPU box's container has 16 (cpu.max = 1600000 100000) of the host's 256 hardware threads -- which is why the baseline
    is fastest at 16 threads, collapses at 64 (throttled) and why concurrent replicas share what one process already uses."""
    try:
        q, per = open('/sys/fs/cgroup/cpu.max').read().split()[:2]
        return None if q == 'max' else float(q) / float(per)
    except (OSError, ValueError):
        pass
    try:
        q = float(open('/sys/fs/cgroup/cpu/cpu.cfs_quota_us').read())
        per = float(open('/sys/fs/cgroup/cpu/cpu.cfs_period_us').read())
        return None if q <= 0 else q / per
    except (OSError, ValueError):
        return None


def physical_cores_by_socket():
    """{socket: [one hardware thread per physical core]} from sysfs; None where it is not readable."""
    try:
        allowed = sorted(os.sched_getaffinity(0))
    except AttributeError:
        return None
    cores = {}
    for c in allowed:
        base = f'/sys/devices/system/cpu/cpu{c}/topology/'
        try:
            pkg = int(open(base + 'physical_package_id').read())
            core = int(open(base + 'core_id').read())
        except (OSError, ValueError):
            return None
        cores.setdefault(pkg, {}).setdefault(core, c)
    return {k: sorted(v.values()) for k, v in cores.items()}


def cpu_replica_worker(path):
    """One of the concurrent replicas of cpu_baseline's second phase: pinned to ITS core set, the same oracle step at the job's batch;
    waits for the go file so that all replicas time the same wall-clock window; prints its timed interval."""
    job = np.load(path)
    cpus = [int(c) for c in job['cpus']]
    os.sched_setaffinity(0, cpus)
    import torch
    from oracle import torch_ops as T  # noqa: F401
    from oracle import models as M
    from oracle import train as TR
    torch.set_num_threads(len(cpus))
    b, nsteps = int(job['B']), int(job['nsteps'])
    cfg = dict(backbone_block='resnet', upsampling='spc', scale=4)
    P = M.Params()
    for k in job.files:
        if k.startswith('w/'):
            P[k[2:]] = torch.from_numpy(np.array(job[k], np.float32)).requires_grad_(True)
    opt = TR.Adam(P, lr=1e-3)
    x, y = synthetic_batch(4242 + int(job['index']), b)
    xt, yt = torch.from_numpy(x), torch.from_numpy(y)
    TR.supervised_step('net_postupsampling', cfg, P, xt, None, yt, loss='mae', opt=opt)          # warm-up (first touch)
    ready, go = str(job['ready']), str(job['go'])
    open(ready, 'w').close()
    t_wait = time.time()
    while not os.path.exists(go) and time.time() - t_wait < 120:
        time.sleep(0.005)
    t0 = time.time()
    for _ in range(nsteps):
        TR.supervised_step('net_postupsampling', cfg, P, xt, None, yt, loss='mae', opt=opt)
    print(json.dumps({'t0': t0, 't1': time.time(), 'steps': nsteps, 'B': b, 'cpus': len(cpus)}), flush=True)


def cpu_baseline_worker(path):
    """Child process of cpu_baseline: pins itself to one socket BEFORE torch creates its thread pool, times the oracle, prints JSON."""
    cpus = one_socket_cpus()
    if cpus:
        os.sched_setaffinity(0, cpus)
    import torch
    from oracle import torch_ops as T  # noqa: F401
    from oracle import models as M
    from oracle import train as TR
    ncpu = os.cpu_count() or 1
    threads = len(cpus) if cpus else ncpu
    torch.set_num_threads(threads)
    job = np.load(path)
    b, budget_s = int(job['B']), float(job['budget_s'])
    cfg = dict(backbone_block='resnet', upsampling='spc', scale=4)
    P = M.Params()
    for k in job.files:
        if k.startswith('w/'):
            P[k[2:]] = torch.from_numpy(np.array(job[k], np.float32)).requires_grad_(True)
    opt = TR.Adam(P, lr=1e-3)
    x, y = synthetic_batch(4242, b)
    xt, yt = torch.from_numpy(x), torch.from_numpy(y)

    def step():
        t0 = time.perf_counter()
        TR.supervised_step('net_postupsampling', cfg, P, xt, None, yt, loss='mae', opt=opt)
        return time.perf_counter() - t0
    # thread counts inside the socket: the graph's 8-channel 512^2 layers stop scaling well before 64 cores (measured on the GPU box,
    # round 5: 4.7 samples/s with all 64 cores of a socket at B = 64, ~10 with 16-32 threads) -- the best count is reported with the sweep
    t_all = time.perf_counter()
    sweep, best = {}, None
    quota = cgroup_cpu_quota()
    counts = sorted({min(threads, t) for t in (16, 32, threads)})
    if quota:                                              # threads beyond the container's CPU quota are only throttled: one such count stays in the sweep as the evidence
        counts = sorted({min(threads, t) for t in (max(1, int(quota)), max(1, int(2 * quota)))} | {c for c in counts if c <= quota})
    for n in counts:
        if best is not None and time.perf_counter() - t_all > budget_s:
            sweep[str(n)] = 'skipped (time budget)'
            continue
        torch.set_num_threads(n)
        times = [step()]                                   # warm-up (first touch of every activation buffer)
        while len(times) < 3 and (time.perf_counter() - t_all) + times[-1] < budget_s:
            times.append(step())
        dt = min(times[1:]) if len(times) > 1 else times[0]
        sweep[str(n)] = round(b / dt, 2)
        if best is None or dt < best[1]:
            best = (n, dt, times)
    n, dt, times = best
    print(json.dumps({'value': b / dt, 'unit': 'HR samples/s', 'cores': n, 'cores_total': ncpu, 'kind': 'port', 'cgroup_cpu_quota': quota,
                      'socket_cores': threads, 'sweep_samples_per_s_by_threads': sweep, 'step_seconds': [round(t, 3) for t in times],
                      'sample': f'oracle torch-CPU (oneDNN) fp32 train step (fwd+MAE+bwd+Adam) of the same graph and weights, B={b} at '
                                f'128->512, process pinned to the {threads} physical cores of ONE socket (os.sched_setaffinity; the host '
                                f'has {ncpu} hardware threads' + (f'; the container\'s cgroup CPU quota is {quota:g} CPUs' if quota else '') +
                                f'), thread counts {" / ".join(str(c) for c in counts)} swept, {n} threads fastest: best of '
                                f'{max(len(times) - 1, 1)} step(s) after a warm-up step, {budget_s:.0f} s budget'}), flush=True)


def cpu_replicas(weights, tmp, batch, per=16, nsteps=2):
    """Second phase of the CPU baseline (round 6): the single process anti-scales beyond 16-32 threads (the graph's
    8-channel 512^2 layers), which says nothing about what the HOST can do -- so: as many concurrent replicas of the same step as there
    are disjoint sets of `per` physical cores (both sockets), each pinned to its set with its own batch, no gradient exchange between
    them (optimistic for the CPU: a data-parallel CPU job would pay an all-reduce on top).  value = all replicas' samples over the
    common wall-clock window (first start .. last end)."""
    by_socket = physical_cores_by_socket()
    if not by_socket:
        return None
    quota = cgroup_cpu_quota()
    if quota is not None and quota < 2 * per:
        return {'skipped': f'the container\'s cgroup CPU quota is {quota:g} CPUs: fewer than two sets of {per} cores -- concurrent replicas would share what '
                           f'the single process already uses (measured once on the GPU box: 8 replicas 11.2 samples/s in aggregate against 13.2 of one)'}
    sets = []
    for pkg in sorted(by_socket):
        cs = by_socket[pkg]
        sets += [cs[i:i + per] for i in range(0, len(cs) - per + 1, per)]
    if len(sets) < 2:
        return None
    procs = []
    go = os.path.join(tmp, 'go')
    for i, cpus in enumerate(sets):
        path = os.path.join(tmp, f'rep{i}.npz')
        np.savez(path, B=np.asarray(batch), nsteps=np.asarray(nsteps), index=np.asarray(i), cpus=np.asarray(cpus),
                 ready=np.asarray(os.path.join(tmp, f'ready{i}')), go=np.asarray(go),
                 **{'w/' + k: np.asarray(v, np.float32) for k, v in weights.items()})
        procs.append(subprocess.Popen([sys.executable, os.path.abspath(__file__), '--cpu-replica-worker', path], stdout=subprocess.PIPE,
                                      stderr=subprocess.PIPE, text=True, env=dict(os.environ, PYTHONPATH=ROOT)))
    t_wait = time.time()
    while not all(os.path.exists(os.path.join(tmp, f'ready{i}')) for i in range(len(sets))) and time.time() - t_wait < 180:
        if any(p.poll() is not None for p in procs):
            break
        time.sleep(0.05)
    open(go, 'w').close()
    outs = []
    for p in procs:
        o, e = p.communicate(timeout=600)
        lines = [ln for ln in o.splitlines() if ln.startswith('{')]
        if p.returncode != 0 or not lines:
            raise RuntimeError(f'cpu replica failed (rc {p.returncode}): {e[-300:]}')
        outs.append(json.loads(lines[-1]))
    window = max(o['t1'] for o in outs) - min(o['t0'] for o in outs)
    total = sum(o['steps'] * o['B'] for o in outs)
    return {'value': total / window, 'unit': 'HR samples/s', 'replicas': len(sets), 'cores_per_replica': per, 'cores': per * len(sets),
            'per_replica_samples_per_s': [round(o['steps'] * o['B'] / (o['t1'] - o['t0']), 2) for o in outs],
            'window_s': round(window, 3),
            'sample': f'{len(sets)} concurrent replicas of the same oracle step (B = {batch} each, {nsteps} steps after a warm-up step), each pinned '
                      f'to its own {per} physical cores (both sockets), started together, no gradient exchange: all samples / the common window'}


def cpu_baseline(weights, budget_s=30.0, batch=16):
    """The oracle (torch-CPU restatement of the identical graph, fp32, oneDNN convolutions) timed on a bounded sample of the same
    workload -- B = 16 at 128 -> 512 (the metric is samples/s; B = 64 was slower per sample), one socket's physical cores, in a CHILD process so that the affinity mask
    is in place before torch's thread pool exists and nothing of it leaks into this process.  A reported baseline, never a target
    (cores stated -- `cores`, `cores_total`).  Round 6: a second phase runs concurrent replicas on disjoint
    16-core sets of BOTH sockets (cpu_replicas); the larger of the two is `value`, both are reported."""
    import tempfile
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, 'job.npz')
        np.savez(path, B=np.asarray(batch), budget_s=np.asarray(budget_s), **{'w/' + k: np.asarray(v, np.float32) for k, v in weights.items()})
        r = subprocess.run([sys.executable, os.path.abspath(__file__), '--cpu-baseline-worker', path], capture_output=True, text=True,
                           timeout=4 * budget_s + 120, env=dict(os.environ, PYTHONPATH=ROOT))
        lines = [ln for ln in r.stdout.splitlines() if ln.startswith('{')]
        if r.returncode != 0 or not lines:
            raise RuntimeError(f'cpu baseline worker failed (rc {r.returncode}): {r.stderr[-500:]}')
        single = json.loads(lines[-1])
        try:
            rep = cpu_replicas(weights, tmp, batch)
        except Exception as e:
            rep = {'error': repr(e)}
    out = dict(single)
    out['single_process'] = {k: single[k] for k in ('value', 'cores', 'sweep_samples_per_s_by_threads') if k in single}
    out['replicas'] = rep
    if rep and 'value' in rep and rep['value'] > single['value']:
        out.update({'value': rep['value'], 'cores': rep['cores'],
                    'sample': rep['sample'] + ' (the single process pinned to one socket: ' + f"{single['value']:.1f} samples/s at {single['cores']} threads)"})
    return out


def split_roofs(roofline, achieved):
    """A conv_split tag computes fp32 products as six bf16 MFMA terms: BOTH roofs -- `peak` / `frac` = the pipe it runs on
    (dense bf16 MFMA peak / 6 bf16 products per fp32 product = 417 TFLOP/s of fp32 products), `fp32_mfma_roof` = what the same layer is
    priced at on the fp32 pipe (a fraction above 1 there is the point of the form, not an error)."""
    pipe = PEAK_BF16_MFMA_TFLOPS / 6.0
    roofline['arith'] = 'fp32 products as 6 bf16 MFMA terms, fp32 accumulate'
    roofline['fp32_mfma_roof'] = {'achieved': achieved, 'peak': PEAK_FP32_MFMA_TFLOPS, 'unit': 'TFLOP/s', 'frac': achieved / PEAK_FP32_MFMA_TFLOPS}
    roofline.update({'peak': pipe, 'unit': 'TFLOP/s of fp32 products', 'frac': achieved / pipe,
                     'peak_note': 'v_mfma_f32_16x16x32_bf16 dense peak 2 500 TFLOP/s / six bf16 products per fp32 product'})


def arith_text():
    """What the matrix pipes multiply (a six-term split counts as f32 only if the line says so and prints both roofs)."""
    if os.environ.get('DL4DS_NO_SPLIT'):
        return 'fp32 MFMA (v_mfma_f32_16x16x4_f32) / fp32 VALU, fp32 accumulate (DL4DS_NO_SPLIT=1)'
    which = ('every eligible 40/48-channel shape: DL4DS_SPLIT=1' if os.environ.get('DL4DS_SPLIT') else
             'default dispatch: one pass of <= 48 input channels, <= 48 output channels, grids of >= 1 strip segment per CU')
    return ('fp32 products as 6 bf16 MFMA terms, fp32 accumulate, on the 3x3 layers tagged conv_split<3,3> (' + which + '; same error as the '
            'fp32 MFMA, profiles/conv_split_r06.txt; DL4DS_NO_SPLIT=1 is the A/B switch); every other layer fp32 MFMA '
            '(v_mfma_f32_16x16x4_f32) / fp32 VALU, fp32 accumulate')


def step_roofline(rep, nprof, ms_step):
    """How far the whole STEP is from its own roofline.  Every profiled launch class k (a kernel tag = one shape class) is priced
    at the larger of its matrix time and its memory time, lower_bound = sum_k max(flops_k / 157.3 TFLOP/s, bytes_k / 6.3 TB/s):
    flops_k = the multiply-adds the layer NEEDS in the form the kernel computes it (Winograd launches: the direct form / 2.25,
    no channel padding, no transform additions), bytes_k = one read of every input + one write of every output.  frac =
    lower_bound / measured step time.  Launches without a profiler tag (a few memsets / copies) add nothing to the bound."""
    lb = mfma = hbm = 0.0
    for k, v in rep.items():
        fl = v.get('direct_flops', v['flops']) / WINOGRAD_SAVING if k.startswith('conv_wino') else v['flops']
        # (the opt-in six-term kernel is priced at the roof of the pipe it runs on: 2 500 / 6 TFLOP/s of fp32 products)
        peak = PEAK_BF16_MFMA_TFLOPS / 6.0 if k.startswith('conv_split') else PEAK_FP32_MFMA_TFLOPS
        t_m = fl / (peak * 1e12) * 1e3 / nprof
        t_b = v['bytes'] / (ACHIEVABLE_HBM_GBPS * 1e9) * 1e3 / nprof
        lb += max(t_m, t_b)
        if t_m >= t_b:
            mfma += t_m
        else:
            hbm += t_b
    tagged = sum(v['ms'] for v in rep.values()) / nprof
    return {'lower_bound_ms': round(lb, 4), 'frac': round(lb / ms_step, 4), 'mfma_ms': round(mfma, 4), 'hbm_ms': round(hbm, 4),
            'tagged_kernel_ms': round(tagged, 4), 'ms_per_step': round(ms_step, 4),
            'peaks': {'fp32_mfma_tflops': PEAK_FP32_MFMA_TFLOPS, 'hbm_gbps': ACHIEVABLE_HBM_GBPS},
            'note': 'sum over kernel tags of max(useful flops / MFMA peak, algorithmic bytes / achievable HBM rate) over the '
                    'measured step; Winograd layers at their useful multiplies (direct form / 2.25)'}


# ------------------------------------------------------------------------------------------------ workloads
def supervised_outputs(eng, model):
    """What a supervised train step returns to its caller: the batch loss and the updated weights (by variable name)."""
    return dict([('loss', np.asarray([eng.last_loss()], np.float32))] + [('weights/' + k, v) for k, v in model.get_weights().items()])


def make_workload(name, B, rank, world):
    """-> dict(step=callable, describe=str, engine=..., model=..., metric=str, loss=callable, outputs=callable -> {name: array})."""
    import dl4ds_amd.models as PM
    from dl4ds_amd.device import DeviceArray
    from dl4ds_amd.training import SupervisedEngine, CGANEngine
    if name == 'cfg2':
        model = PM.net_postupsampling('resnet', 'spc', 4, 1, 0, (128, 128), seed=7)
        eng = SupervisedEngine(model, loss='mae', learning_rate=(1e-3 * world, 1e-4 * world), lr_decay_after=1e5)
        x, y = synthetic_batch(1002 + rank, B)
        dx, dy = DeviceArray.from_numpy(x), DeviceArray.from_numpy(y)
        return dict(step=lambda: eng.step_device([dx.ptr], dy.ptr, B), engine=eng, model=model, keep=(dx, dy),
                    metric='HR samples/s (train step) at 4x 128->512 residual SR',
                    describe=('configs[1]: net_postupsampling(resnet, spc, scale=4, lr 128x128 -> hr 512x512, 204405 '
                              'params), MAE, Adam' if world == 1 else 'configs[2]: same model, data-parallel over RCCL'),
                    loss=lambda: eng.last_loss(), outputs=lambda: supervised_outputs(eng, model))
    if name == 'cfg4':
        T, h, s = 8, 64, 4
        model = PM.recnet_postupsampling('densenet', 'rc', s, 1, 1, (h, h), time_window=T, attention=True,
                                         localcon_layer=True, seed=7)
        eng = SupervisedEngine(model, loss='mae', learning_rate=1e-3 * world)
        x, aux, y = synthetic_batch_cfg4(1004 + rank, B, T, h, s)
        dx, da, dy = (DeviceArray.from_numpy(a) for a in (x, aux, y))
        return dict(step=lambda: eng.step_device([dx.ptr, da.ptr], dy.ptr, B), engine=eng, model=model, keep=(dx, da, dy),
                    metric='HR samples/s (train step), spatio-temporal dense + attention + LCB, resize-conv 4x, T=8, 64->256',
                    describe=f'configs[3]: recnet_postupsampling(densenet, rc, scale=4, lr 64x64, T=8, attention, LCB, 1 aux; '
                             f'{model.count_params()} params), MAE, Adam',
                    loss=lambda: eng.last_loss(), outputs=lambda: supervised_outputs(eng, model))
    if name == 'cfg5':
        H = 512
        gen = PM.unet_pin('unet', 5, 1, hr_size=(H, H), n_filters=8, n_blocks=6, decoder_upsampling='dc', seed=7)
        disc = PM.residual_discriminator(5, 'pin', False, 8, (H // 8, H // 8), n_filters=8, hr_size=(H, H), seed=8)
        eng = CGANEngine(gen, disc, loss='mae', learning_rate=(2e-4, 2e-4))
        x, aux, y = synthetic_batch_cfg5(1005 + rank, B, H)
        dx, da, dy = (DeviceArray.from_numpy(a) for a in (x, aux, y))
        return dict(step=lambda: eng.step_device([dx.ptr, da.ptr], dy.ptr, B), engine=eng, model=gen, keep=(dx, da, dy),
                    metric='HR samples/s (CGAN train step), U-Net(deconv) generator + residual discriminator, 8x 64->512',
                    describe=f'configs[4]: unet_pin(unet, dc, 5+1 channels, hr 512x512; G {gen.count_params()} + '
                             f'D {disc.count_params()} params), CGAN step (MAE x100 + BCE), 2 x Adam(2e-4, beta1 0.5)',
                    loss=lambda: None,
                    outputs=lambda: dict([('generator/' + k, v) for k, v in gen.get_weights().items()] +
                                         [('discriminator/' + k, v) for k, v in disc.get_weights().items()]))
    raise SystemExit(f'unknown --config {name}')


# ------------------------------------------------------------------------------------------------ predict line
def predict_line(args):
    """`python bench.py --predict`: forward-only HR samples/s of configs[1] (north_star: the Predictor API, inference.py:109-255) --
    `value` with the LR batch and the HR output resident in HBM (dl4ds_graph_forward), `host_arrays` the same through Model.predict
    with numpy arrays in and out (one PCIe copy each way per batch), the dominant kernel with its roofline and the forward pass's
    distance from its own roofline; one JSON line (kept as profiles/bench_predict_rNN.json)."""
    import dl4ds_amd._lib as L
    import dl4ds_amd.models as PM
    from dl4ds_amd.device import DeviceArray
    lib = L.lib()
    B = args.batch or 64
    model = PM.net_postupsampling('resnet', 'spc', 4, 1, 0, (128, 128), seed=7)
    x_host, _ = synthetic_batch(1002, B)
    x = DeviceArray.from_numpy(x_host)
    y = DeviceArray.zeros((B, 512, 512, 1))
    ptrs = (ctypes.c_void_p * 1)(x.ptr)
    fwd = lambda: L.check(lib.dl4ds_graph_forward(model.graph.h, ptrs, 1, B, 0, 0, y.ptr))
    for _ in range(max(args.warmup, 3)):
        fwd()
    L.check(lib.dl4ds_profile_filter(b''))
    L.check(lib.dl4ds_profile_enable(1))
    nprof = 3
    for _ in range(nprof):
        fwd()
    buf = ctypes.create_string_buffer(1 << 17)
    L.check(lib.dl4ds_profile_report(buf, len(buf)))
    rep = json.loads(buf.value.decode())
    L.check(lib.dl4ds_profile_enable(0))
    L.check(lib.dl4ds_sync())
    t0 = time.perf_counter()
    for _ in range(args.steps):
        fwd()
    L.check(lib.dl4ds_sync())
    dt = (time.perf_counter() - t0) / args.steps
    outputs = {'pred': y.numpy()} if args.dump_outputs else None          # the HR fields of the last timed forward pass
    n2 = int(np.ceil(MIN_STEADY_S / dt))
    t0 = time.perf_counter()
    for _ in range(n2):
        fwd()
    L.check(lib.dl4ds_sync())
    dt2 = (time.perf_counter() - t0) / n2
    # through the reference's call: numpy in, numpy out (4 batches per call, batch_size = B)
    xs = np.concatenate([x_host] * 4, axis=0)
    model.predict(xs[:B], batch_size=B)
    t0 = time.perf_counter()
    reps_h = 3
    for _ in range(reps_h):
        out_h = model.predict(xs, batch_size=B)
    dth = (time.perf_counter() - t0) / (reps_h * 4)
    assert out_h.shape == (4 * B, 512, 512, 1)
    dom = max((k for k in rep if rep[k]['flops'] > 0), key=lambda k: rep[k]['ms'])
    d = rep[dom]
    wino = dom.startswith('conv_wino')
    achieved = (d.get('direct_flops', d['flops']) / WINOGRAD_SAVING if wino else d['flops']) / (d['ms'] * 1e-3) / 1e12
    tot = sum(v['ms'] for v in rep.values())
    top = {k: {'ms_per_batch': round(v['ms'] / nprof, 4), 'launches': v['n'] / nprof,
               'tflops_issued': round(v['flops'] / (v['ms'] * 1e-3) / 1e12, 1) if v['flops'] else None,
               'gbps': round(v['bytes'] / (v['ms'] * 1e-3) / 1e9, 1)}
           for k, v in sorted(rep.items(), key=lambda kv: -kv[1]['ms'])[:8]}
    out = {'metric': 'HR samples/s (predict: forward only) at 4x 128->512 residual SR', 'value': B / dt, 'unit': 'HR samples/s',
           'n_gpus': 1, 'steps': args.steps, 'warmup': max(args.warmup, 3), 'ms_per_step': 1e3 * dt, 'higher_is_better': True,
           'scaling': 'weak', 'vs_baseline': None, 'dtype': 'f32', 'data': 'synthetic', 'arith': arith_text(),
           'config': {'workload': 'configs[1] forward only: net_postupsampling(resnet, spc, scale=4, lr 128x128 -> hr 512x512, 204405 params), '
                                  'dl4ds_graph_forward with the LR batch and the HR output resident in HBM', 'per_gpu_batch': B},
           'steady_state': {'steps': n2, 'ms_per_step': 1e3 * dt2, 'value': B / dt2},
           'host_arrays': {'value': B / dth, 'ms_per_batch': 1e3 * dth, 'unit': 'HR samples/s',
                           'note': 'Model.predict(numpy (4 B, 128, 128, 1), batch_size=B) -> numpy (4 B, 512, 512, 1): one host-to-device '
                                   'copy of the LR batch and one device-to-host copy of the HR fields (67 MB) per batch, pageable memory'},
           'roofline': {'bound': 'mfma', 'kernel': dom, 'achieved': achieved, 'peak': PEAK_FP32_MFMA_TFLOPS, 'unit': 'TFLOP/s',
                        'frac': achieved / PEAK_FP32_MFMA_TFLOPS, 'traffic': None, 'winograd': wino,
                        'avg_launch_ms': d['ms'] / d['n'], 'launches_per_batch': d['n'] / nprof, 'share_of_forward_time': d['ms'] / tot,
                        'algorithmic_bytes_per_launch': d['bytes'] / d['n'],
                        'measured': 'HIP events around every launch of three profiled forward passes right before the timed ones'},
           'step_roofline': step_roofline(rep, nprof, 1e3 * dt),
           'executed_gflop_per_sample': sum(v['flops'] for v in rep.values()) / nprof / 1e9 / B,
           'direct_form_gflop_per_sample': sum(v.get('direct_flops', v['flops']) for v in rep.values()) / nprof / 1e9 / B,
           'kernels': top, 'cpu_baseline': None}
    if dom.startswith('conv_split'):
        split_roofs(out['roofline'], achieved)
    if outputs is not None:
        out['dump_outputs'] = {'dir': args.dump_outputs, 'arrays': dump_outputs(args.dump_outputs, outputs)}
    print(json.dumps(out), flush=True)


# ------------------------------------------------------------------------------------------------ launcher
def _free_port_pair():
    for _ in range(64):
        s = socket.socket()
        s.bind(('127.0.0.1', 0))
        p = s.getsockname()[1]
        s2 = socket.socket()
        try:
            s2.bind(('127.0.0.1', p + 1))
        except OSError:
            continue
        finally:
            s.close()
            s2.close()
        return p
    raise RuntimeError('no free port pair found')


def spawn_ranks(n, argv, script=None, device_count=None):
    """One child per GPU (rank i -> LOCAL_RANK i); rank 0's stdout is this process's stdout (the JSON line).
    ``script`` / ``device_count``: stand-ins for this file and the library's device count (tests/test_rendezvous.py runs the
    launcher for N = 8 without a GPU)."""
    if device_count is None:
        import dl4ds_amd._lib as L
        cnt = ctypes.c_int(0)
        device_count = cnt.value if L.load().dl4ds_device_count(ctypes.byref(cnt)) == 0 else 0
    if device_count < n:
        raise SystemExit(f'bench.py --gpus {n}: only {device_count} HIP device(s) visible (one process per GPU: '
                         f'run with --gpus {max(device_count, 1)} or on a node with {n} GPUs)')
    port = _free_port_pair()
    procs = []
    for r in range(n):
        env = dict(os.environ, RANK=str(r), LOCAL_RANK=str(r), WORLD_SIZE=str(n), LOCAL_WORLD_SIZE=str(n),
                   MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port), HSA_ENABLE_IPC_MODE_LEGACY='0')
        procs.append(subprocess.Popen([sys.executable, script or os.path.abspath(__file__)] + argv, env=env,
                                      stdout=None if r == 0 else subprocess.DEVNULL))
    rc = 0
    try:
        while procs:
            for p in list(procs):
                code = p.poll()
                if code is None:
                    continue
                procs.remove(p)
                if code != 0:
                    rc = rc or code
                    for q in procs:              # one rank failed: the others would wait in a collective for ever
                        q.terminate()
            time.sleep(0.05)
    finally:
        for q in procs:
            q.kill()
    return rc


def bucket_plan(model):
    """The gradient buckets of the model's arena in launch order (dl4ds_graph_bucket_plan)."""
    import dl4ds_amd._lib as L
    buf = ctypes.create_string_buffer(1 << 16)
    L.check(L.lib().dl4ds_graph_bucket_plan(model.graph.h, buf, len(buf)))
    plan = json.loads(buf.value.decode())
    return {'buckets': len(plan), 'bytes': [b['bytes'] for b in plan],
            'final_after_backward_of_op': [b['final_after_backward_of_op'] for b in plan], 'forward_ops': plan[0]['of_ops'] if plan else 0}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--gpus', type=int, default=1)
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--batch', type=int, default=None,
                    help='per-GPU batch (weak scaling); default 64 for cfg2 (the reference default, '
                         'training/supervised.py:49) and 16 for cfg4 / cfg5 (training/cgan.py:48)')
    ap.add_argument('--config', default='cfg2', choices=['cfg2', 'cfg4', 'cfg5'])
    ap.add_argument('--predict', action='store_true', help='the forward-only line of configs[1] (Predictor API) instead of the train step')
    ap.add_argument('--full', action='store_true',
                    help='also the per-kernel profile and rooflines, the steady-state window and (cfg2, one GPU) the unfolded graph, '
                         'the per-GPU-batch-16 line and the CPU baseline; a plain run times the K steps only')
    ap.add_argument('--dump-outputs', default=None, metavar='DIR',
                    help='write what the last timed step returned (loss, updated weights) as DIR/<name>.npy')
    ap.add_argument('--no-cpu-baseline', action='store_true')
    ap.add_argument('--no-profile', action='store_true')
    ap.add_argument('--no-unfolded', action='store_true', help='skip the 5-step comparison run of the unfolded graph')
    ap.add_argument('--no-b16', action='store_true', help='skip the per-GPU-batch-16 line (SURVEY.md section 8d: "best and B=16")')
    ap.add_argument('--cpu-baseline-worker', default=None, help=argparse.SUPPRESS)
    ap.add_argument('--cpu-replica-worker', default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.cpu_baseline_worker:
        return cpu_baseline_worker(args.cpu_baseline_worker)
    if args.cpu_replica_worker:
        return cpu_replica_worker(args.cpu_replica_worker)

    if args.predict:
        return predict_line(args)
    if 'WORLD_SIZE' not in os.environ and args.gpus > 1:
        raise SystemExit(spawn_ranks(args.gpus, sys.argv[1:]))
    rank = int(os.environ.get('RANK', '0'))
    world = int(os.environ.get('WORLD_SIZE', '1'))
    os.environ.setdefault('HSA_ENABLE_IPC_MODE_LEGACY', '0')

    import dl4ds_amd._lib as L
    from dl4ds_amd import parallel

    if world > 1:
        cnt = ctypes.c_int(0)
        if L.load().dl4ds_device_count(ctypes.byref(cnt)) != 0 or cnt.value < int(os.environ.get('LOCAL_WORLD_SIZE', world)):
            raise SystemExit(f'bench.py: rank {rank} of {world} sees {cnt.value} HIP device(s), the launcher asked for '
                             f'{os.environ.get("LOCAL_WORLD_SIZE", world)} ranks on this node (one GPU per rank)')
    lib = L.lib()                       # binds LOCAL_RANK -> device, fails loudly without a GPU
    force_dist = bool(os.environ.get('DL4DS_FORCE_DIST'))      # exercise the RCCL path even with one rank
    if world > 1:
        parallel.init_from_env()
    elif force_dist:
        parallel.init_with_id(0, 1, parallel.unique_id())
    comm = parallel.comm_info()
    dist_on = comm['nranks'] > 0

    B = args.batch or (64 if args.config == 'cfg2' else 16)
    wl = make_workload(args.config, B, rank, world)
    eng, model, step = wl['engine'], wl['model'], wl['step']
    if dist_on:
        parallel.broadcast_trainer(eng)
    is_cfg2 = args.config == 'cfg2'
    full = args.full
    w0 = model.get_weights() if (full and rank == 0 and world == 1 and is_cfg2 and not args.no_cpu_baseline) else None

    def barrier():
        L.check(lib.dl4ds_sync())
        if dist_on:
            parallel.barrier()

    # ---- warm-up; on rank 0 its last steps are timed per launch (HIP events on the library stream) to find the kernel
    #      with the largest share of step time and to provide the per-kernel figures
    prof_on = full and rank == 0 and not args.no_profile
    nprof = min(3, args.warmup) if prof_on else 0
    if prof_on and nprof == 0:
        nprof = 2            # --warmup 0: two extra (untimed) steps are needed to pick the kernel to instrument
    # every rank runs the SAME number of steps (each step is a sequence of collectives): the ranks that do not profile make up
    # for rank 0's extra steps of a --warmup 0 run
    extra_other = (2 if (args.warmup == 0 and full and not args.no_profile) else 0) if (world > 1 and rank != 0) else 0
    for _ in range(max(args.warmup - nprof, 0) + extra_other):
        step()
    breakdown, dom, dom_share, rep_all = None, None, None, None
    executed_gflop_per_step = mfma_gflop_per_step = direct_gflop_per_step = None
    winograd = None           # (known from the profile of a --full run)
    hbm_kernels = None

    def report():
        buf = ctypes.create_string_buffer(1 << 17)
        L.check(lib.dl4ds_profile_report(buf, len(buf)))
        return json.loads(buf.value.decode())

    if nprof:
        L.check(lib.dl4ds_profile_filter(b''))
        L.check(lib.dl4ds_profile_enable(1))
        for _ in range(nprof):
            step()
        rep = rep_all = report()
        L.check(lib.dl4ds_profile_enable(0))
        tot = sum(v['ms'] for v in rep.values())
        breakdown = {k: {'launches_per_step': v['n'] / nprof, 'ms_per_step': v['ms'] / nprof,
                         'tflops': (v['flops'] / (v['ms'] * 1e-3) / 1e12) if v['flops'] else None,
                         'gbps': v['bytes'] / (v['ms'] * 1e-3) / 1e9}
                     for k, v in sorted(rep.items(), key=lambda kv: -kv[1]['ms'])}
        # (issued work: the Winograd launches count the multiply-adds they issue -- 4 per output and (cin, cout) pair on the
        #  padded operands plus the transforms' additions -- not the 9 of the direct form; `direct_form_gflop_per_sample` is
        #  the same step priced as the direct kernels would execute it)
        executed_gflop_per_step = sum(v['flops'] for v in rep.values()) / nprof / 1e9
        direct_gflop_per_step = sum(v.get('direct_flops', v['flops']) for v in rep.values()) / nprof / 1e9
        winograd = any(k.startswith('conv_wino') for k in rep)
        mfma_gflop_per_step = sum(v['flops'] for k, v in rep.items()
                                  if k.startswith(('conv_stream', 'conv_wgrad', 'conv_igemm', 'conv_narrow', 'conv_pack', 'conv_wino'))
                                  ) / nprof / 1e9
        # memory-bound kernels (north_star: "achieved HBM GB/s for the memory-bound upsampling/attention kernels"):
        # algorithmic bytes (one read of each input + one write of each output) / HIP-event duration, vs the 8 TB/s spec
        hbm_kernels = {}
        for k, v in sorted(rep.items(), key=lambda kv: -kv[1]['ms']):
            if k.startswith(HBM_KERNEL_PREFIXES) and v['bytes'] > 0 and v['ms'] / nprof >= 0.02:
                gbps = v['bytes'] / (v['ms'] * 1e-3) / 1e9
                hbm_kernels[k] = {'gbps': round(gbps, 1), 'frac_of_8TBps': round(gbps / PEAK_HBM_GBPS, 3),
                                  'ms_per_step': round(v['ms'] / nprof, 4), 'launches_per_step': v['n'] / nprof}
        dom = max((k for k in rep if rep[k]['flops'] > 0), key=lambda k: rep[k]['ms'])
        dom_share = rep[dom]['ms'] / tot
        # ---- the dominant kernel alone stays instrumented during the timed region (two events per launch of that one
        #      kernel: a handful of launches per step)
        L.check(lib.dl4ds_profile_filter(dom.encode()))
        L.check(lib.dl4ds_profile_enable(1))
    barrier()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        step()
    L.check(lib.dl4ds_sync())
    dt = time.perf_counter() - t0
    barrier()
    dt_own = dt
    dt_min = dt
    if dist_on:
        dt = parallel.allreduce_host([dt_own], 'max')[0]        # slowest rank
        dt_min = parallel.allreduce_host([dt_own], 'min')[0]
    loss = wl['loss']()
    # (taken before the steady-state window of --full trains the same model further)
    outputs = wl['outputs']() if (args.dump_outputs and rank == 0) else None

    roofline = None
    if dom is not None:
        d = report().get(dom)               # (the K timed steps only: the steady-state window below runs un-instrumented)
        L.check(lib.dl4ds_profile_enable(0))
        L.check(lib.dl4ds_profile_filter(b''))
        if d and d['n']:
            wino = dom.startswith('conv_wino')
            issued = d['flops'] / (d['ms'] * 1e-3) / 1e12
            # ALGORITHMIC work over the kernel's time: for a Winograd tag the multiplies the layer needs in
            # F(2x2,3x3) form -- direct form / 2.25, no channel padding, no transform additions (`issued_*` keeps what
            # rounds 3-4 printed as `frac`: the padded operands and the transforms' additions the kernel actually issues)
            achieved = (d.get('direct_flops', d['flops']) / WINOGRAD_SAVING / (d['ms'] * 1e-3) / 1e12) if wino else issued
            traffic, traffic_source = None, None
            tfile = os.path.join(ROOT, 'profiles', 'traffic.json')
            if os.path.exists(tfile):
                try:
                    tj = json.load(open(tfile))
                    # keyed by config, then by kernel tag: PMC bytes of ANOTHER config's launch of a same-named kernel
                    # (another shape) are not this kernel's traffic -- no entry, no number; and counters collected on OTHER
                    # kernel sources than this build's are not this kernel's either -- fingerprint mismatch, no number
                    here = csrc_sha()
                    if os.environ.get('DL4DS_NO_SPLIT') or os.environ.get('DL4DS_SPLIT'):
                        # the counters were collected in the default dispatch: with it switched the same tag covers other layers
                        traffic_source = 'profiles/traffic.json holds the default dispatch; this run has DL4DS_NO_SPLIT / DL4DS_SPLIT set: not reported'
                    elif tj.get('_csrc_sha') != here:
                        traffic_source = (f'profiles/traffic.json was collected on kernel sources {tj.get("_csrc_sha")} (commit '
                                          f'{tj.get("_commit")}), this build is {here}: stale, not reported')
                    else:
                        traffic = (tj.get(args.config) or {}).get(dom)
                        if traffic is not None:
                            traffic_source = ('profiles/traffic.json: rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE passes of this command '
                                              '(--config ' + args.config + ') on the same kernel sources (' + here + ', commit ' +
                                              str(tj.get('_commit')) + ', ' + str(tj.get('_round')) + '), not measured in this run; per '
                                              'call of the layer, like achieved (a Winograd layer with more than 48 input channels '
                                              'is several kernel launches per call)')
                except Exception:
                    traffic = None
            roofline = {'bound': 'mfma', 'kernel': dom, 'achieved': achieved, 'peak': PEAK_FP32_MFMA_TFLOPS,
                        'unit': 'TFLOP/s', 'frac': achieved / PEAK_FP32_MFMA_TFLOPS, 'traffic': traffic,
                        'traffic_source': traffic_source,
                        'algorithmic_bytes_per_launch': d['bytes'] / d['n'],
                        'launches': d['n'], 'calls_per_step': d['n'] / args.steps, 'avg_launch_ms': d['ms'] / d['n'],
                        'algorithmic_gflop_per_launch': (d.get('direct_flops', d['flops']) / WINOGRAD_SAVING if wino else d['flops']) / d['n'] / 1e9,
                        **({'winograd': True,
                            'note': 'achieved / frac = the multiplies the layer NEEDS in F(2x2,3x3) form (direct form / 2.25: 4 per output '
                                    'and (cin, cout) pair) over the kernel time; issued_* adds the channel padding and the transforms\' '
                                    'additions the kernel executes; direct_form_* is the same layer at the 9 of the direct form',
                            'issued_tflops': issued, 'issued_frac': issued / PEAK_FP32_MFMA_TFLOPS,
                            'issued_gflop_per_launch': d['flops'] / d['n'] / 1e9,
                            'direct_form_gflop_per_launch': d.get('direct_flops', d['flops']) / d['n'] / 1e9,
                            'direct_form_tflops': d.get('direct_flops', d['flops']) / (d['ms'] * 1e-3) / 1e12}
                           if wino else {}),
                        'share_of_step_time': dom_share,
                        'measured': 'HIP events around every launch of this kernel inside the timed region'}
            if dom.startswith('conv_split'):
                split_roofs(roofline, achieved)
            # the roof that binds: a narrow-channel layer's algorithmic bytes / 8 TB/s can be the larger fraction
            gbps = d['bytes'] / (d['ms'] * 1e-3) / 1e9
            if gbps / PEAK_HBM_GBPS > roofline['frac']:
                roofline['mfma_roof'] = {'achieved': achieved, 'peak': PEAK_FP32_MFMA_TFLOPS, 'unit': 'TFLOP/s',
                                         'frac': achieved / PEAK_FP32_MFMA_TFLOPS}
                roofline.update({'bound': 'hbm', 'achieved': gbps, 'peak': PEAK_HBM_GBPS, 'unit': 'GB/s',
                                 'frac': gbps / PEAK_HBM_GBPS})
            else:
                roofline['hbm_roof'] = {'achieved': gbps, 'peak': PEAK_HBM_GBPS, 'unit': 'GB/s', 'frac': gbps / PEAK_HBM_GBPS}

    # ---- a second, longer window: the driver's K steps may be a fraction of a second (cfg2: 20 x 14 ms), during which the
    #      clock is still settling; `value` stays the K-step figure the contract asks for, `steady_state` reports both
    steady = None
    ms_first = 1e3 * dt / args.steps
    if full and ms_first * args.steps < 1e3 * MIN_STEADY_S:
        n2 = int(np.ceil(1e3 * MIN_STEADY_S / ms_first))
        barrier()
        t2 = time.perf_counter()
        for _ in range(n2):
            step()
        L.check(lib.dl4ds_sync())
        dt2s = time.perf_counter() - t2
        barrier()
        if dist_on:
            dt2s = parallel.allreduce_host([dt2s], 'max')[0]
        steady = {'steps': n2, 'seconds': round(dt2s, 3), 'ms_per_step': 1e3 * dt2s / n2, 'value': world * B * n2 / dt2s,
                  'note': f'{n2} further steps (>= {MIN_STEADY_S} s) timed the same way right after the {args.steps} steps of `value`'}
    devname = L.device_name()
    per_rank = None
    if dist_on:
        # every rank's own view, gathered through the host reductions (one slot per rank, summed)
        slots = [0.0] * world
        slots[rank] = 1e3 * dt_own / args.steps
        per_rank = parallel.allreduce_host(slots, 'sum')

    split_on = not os.environ.get('DL4DS_NO_SPLIT')          # (the default dispatch: conv_split for the single-pass <= 48 x <= 48 channel 3x3 layers)
    if rank == 0:
        value = world * B * args.steps / dt
        ms_step = 1e3 * dt / args.steps
        out = {
            'metric': wl['metric'],
            'value': value, 'unit': 'HR samples/s', 'n_gpus': world, 'steps': args.steps, 'warmup': args.warmup,
            'ms_per_step': ms_step, 'higher_is_better': True, 'scaling': 'weak',
            'vs_baseline': None, 'dtype': 'f32', 'data': 'synthetic',
            'config': {'workload': wl['describe'], 'per_gpu_batch': B, 'global_batch': B * world,
                       'parallelism': f'dp{world}', 'loss_after_run': loss},
            'rccl': {'nranks': comm['nranks'], 'launcher_world': world, 'bucket_plan': bucket_plan(model),
                     'ms_per_step_by_rank': [round(v, 4) for v in per_rank] if per_rank else None,
                     'ms_per_step_min_max': [1e3 * dt_min / args.steps, ms_step],
                     'device': devname, 'local_rank_to_device': 'LOCAL_RANK i -> HIP device i (one process per GPU)'} if dist_on else None,
            'steady_state': steady,
            'step_roofline': step_roofline(rep_all, nprof, ms_step) if rep_all else None,
            # executed FLOPs (library profiler, rank 0) over the measured step time
            'step_tflops_per_gpu': (executed_gflop_per_step / ms_step) if executed_gflop_per_step else None,
            'mfma_conv_frac_of_peak': (mfma_gflop_per_step / ms_step / PEAK_FP32_MFMA_TFLOPS) if mfma_gflop_per_step else None,
            'executed_gflop_per_sample': (executed_gflop_per_step / B) if executed_gflop_per_step else None,
            'direct_form_gflop_per_sample': (direct_gflop_per_step / B) if direct_gflop_per_step else None,
            'conv_folding': not bool(os.environ.get('DL4DS_NO_FOLD')),
            'winograd': winograd,
            # what the matrix pipes multiply (a six-term split counts as f32 only if it says so and prints both roofs)
            'arith': arith_text(),
            'roofline': roofline,
            'hbm_kernels': hbm_kernels,
            'cpu_baseline': None,
        }
        if breakdown is not None and os.environ.get('DL4DS_BENCH_BREAKDOWN'):
            out['breakdown'] = breakdown
        if full and world == 1 and is_cfg2 and not os.environ.get('DL4DS_NO_FOLD') and not args.no_unfolded:
            # the same step with every layer evaluated separately (the reference's evaluation order, DL4DS_NO_FOLD=1),
            # measured in the same run so that both figures sit side by side; `value` above is the product path
            try:
                os.environ['DL4DS_NO_FOLD'] = '1'
                wl2 = make_workload('cfg2', B, rank, world)
                for _ in range(2):
                    wl2['step']()
                L.check(lib.dl4ds_sync())
                t1 = time.perf_counter()
                for _ in range(5):
                    wl2['step']()
                L.check(lib.dl4ds_sync())
                dt2 = (time.perf_counter() - t1) / 5
                out['unfolded_graph'] = {'value': B / dt2, 'ms_per_step': 1e3 * dt2, 'steps': 5,
                                         'note': 'DL4DS_NO_FOLD=1: conv2x#2 and TransitionLast as two layers (55 GFLOP/sample)'}
                del wl2
            except Exception as e:
                out['unfolded_graph'] = {'error': repr(e)}
            finally:
                os.environ.pop('DL4DS_NO_FOLD', None)
        if full and world == 1 and is_cfg2 and not args.no_b16 and B != 16:
            # "B per GPU in {8,16,32,64}, report best and B=16" -- the same step at per-GPU batch 16, timed the
            # same way (warm-up, K steps fenced by device syncs, then a >= 1 s window) in this run; `value` stays the B = 64 figure
            try:
                wl3 = make_workload('cfg2', 16, rank, world)
                for _ in range(max(args.warmup, 3)):
                    wl3['step']()
                L.check(lib.dl4ds_sync())
                n3 = max(args.steps, 20)
                t1 = time.perf_counter()
                for _ in range(n3):
                    wl3['step']()
                L.check(lib.dl4ds_sync())
                dt3 = (time.perf_counter() - t1) / n3
                n4 = int(np.ceil(1.0 / dt3))
                t1 = time.perf_counter()
                for _ in range(n4):
                    wl3['step']()
                L.check(lib.dl4ds_sync())
                dt4 = (time.perf_counter() - t1) / n4
                out['b16'] = {'per_gpu_batch': 16, 'value': 16 / dt3, 'ms_per_step': 1e3 * dt3, 'steps': n3,
                              'steady_state': {'value': 16 / dt4, 'ms_per_step': 1e3 * dt4, 'steps': n4}, 'unit': 'HR samples/s'}
                del wl3
            except Exception as e:
                out['b16'] = {'error': repr(e)}
        if w0 is not None:
            try:
                out['cpu_baseline'] = cpu_baseline(w0)
                out['gpu_over_cpu'] = value / out['cpu_baseline']['value']
            except Exception as e:          # the baseline must never kill the GPU number
                out['cpu_baseline'] = {'error': repr(e)}
        if outputs is not None:
            out['dump_outputs'] = {'dir': args.dump_outputs, 'arrays': dump_outputs(args.dump_outputs, outputs)}
        print(json.dumps(out), flush=True)
    if dist_on:
        parallel.barrier()
        parallel.finalize()


if __name__ == '__main__':
    main()
