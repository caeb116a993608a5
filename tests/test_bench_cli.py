"""bench.py plumbing: the multi-GPU launch command (`--gpus N` on its own starts the ranks as a CHILD
`python -m torch.distributed.run`, before anything touches the GPU) and the argument contract of the driver."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_launch_ranks_dry_run_prints_the_launcher_command():
    env = dict(os.environ, RANK='3', LOCAL_RANK='3')          # stale launcher variables must not leak into the child's environment
    env.pop('WORLD_SIZE', None)
    out = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py'), '--gpus', '4', '--steps', '5', '--warmup', '2', '--dry-run'],
                         env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300, cwd=ROOT)
    assert out.returncode == 0, out.stderr.decode()[-2000:]
    d = json.loads(out.stdout.decode().strip().splitlines()[-1])
    cmd = d['cmd']
    assert d['dry_run'] is True and d['cwd'] == ROOT
    assert cmd[1:3] == ['-m', 'torch.distributed.run'] and '--nnodes=1' in cmd
    assert cmd[cmd.index('--nproc-per-node') + 1] == '4'
    assert cmd[cmd.index('--master-addr') + 1] == '127.0.0.1'
    assert 0 < int(cmd[cmd.index('--master-port') + 1]) < 65536
    i = cmd.index(os.path.join(ROOT, 'bench.py'))
    assert cmd[i + 1:] == ['--gpus', '4', '--steps', '5', '--warmup', '2']            # same arguments, --dry-run dropped
    assert d['env']['HSA_ENABLE_IPC_MODE_LEGACY'] == '0'                              # dmabuf IPC: RCCL needs it on this pool


def test_world_size_mismatch_is_refused_before_any_gpu_call():
    env = dict(os.environ, WORLD_SIZE='2', RANK='0', LOCAL_RANK='0')
    out = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py'), '--gpus', '4'], env=env, stdout=subprocess.PIPE,
                         stderr=subprocess.PIPE, timeout=300, cwd=ROOT)
    assert out.returncode != 0 and b'WORLD_SIZE=2' in out.stderr


@pytest.mark.gpu
def test_one_rank_rehearsal_of_the_multi_gpu_bench_on_rccl():
    """The driver's N > 1 runs happen on hardware this repository never sees; this is their rehearsal on the 1-GPU box: bench.py under the
    driver's own launcher with ONE rank and MMSEG_BENCH_FORCE_DIST=1 goes through every line of the data-parallel branch on the real
    backend -- RCCL process group, weight broadcast, per-arena gradient all-reduces overlapped with the backward pass, barrier + max over
    ranks, the replica check -- and must print the contract's JSON line with the dp block."""
    import socket
    s = socket.socket()
    s.bind(('127.0.0.1', 0))
    port = s.getsockname()[1]
    s.close()
    env = dict(os.environ, MMSEG_BENCH_FORCE_DIST='1', HSA_ENABLE_IPC_MODE_LEGACY='0')
    for k in ('RANK', 'LOCAL_RANK', 'WORLD_SIZE'):
        env.pop(k, None)
    cmd = [sys.executable, '-m', 'torch.distributed.run', '--nnodes=1', '--nproc-per-node', '1', '--master-addr', '127.0.0.1',
           '--master-port', str(port), os.path.join(ROOT, 'bench.py'), '--gpus', '1', '--size', '64', '--steps', '2', '--warmup', '1',
           '--no-cpu-baseline']
    out = subprocess.run(cmd, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=900, cwd=ROOT)
    assert out.returncode == 0, out.stderr.decode()[-3000:]
    lines = [l for l in out.stdout.decode().splitlines() if l.startswith('{')]
    assert len(lines) == 1, out.stdout.decode()[-2000:]
    d = json.loads(lines[0])
    assert d['n_gpus'] == 1 and d['rccl_ranks'] == 1 and d['steps'] == 2 and d['warmup'] == 1
    assert d['value'] > 0 and d['scaling'] == 'weak' and d['config']['parallelism'] == 'dp1'
    assert len(d['per_rank_ms_per_step']) == 1
    dp = d['dp']
    assert dp['replicas_identical_after_timed_region'] is True
    assert dp['collectives_per_iteration'] > 0 and 0 < dp['overlapped_with_backward_per_iteration'] <= dp['collectives_per_iteration']
    assert d['roofline']['frac'] > 0


def _dafnet_for_dump(H=64):
    from multimodal_segmentation_amd import nn
    from multimodal_segmentation_amd.configuration import dafnet_config_chaos
    from multimodal_segmentation_amd.models.dafnet import DAFNet
    from tests import helpers as Hh
    nn.set_default_device('cpu')
    model = DAFNet(Hh.make_conf(dafnet_config_chaos, H))
    model.build()
    return model


def test_dump_outputs_writes_the_last_step_within_the_budget(cpu_backend, tmp_path, monkeypatch):
    """--dump-outputs: the losses of the LAST timed step only (a step appends a fixed number of entries per name), every component
    model's state, a seeded sample of it when the whole does not fit the budget -- the same sample from one run to the next"""
    import numpy as np
    import torch
    import bench
    from multimodal_segmentation_amd.models.trainer import nn_total
    model = _dafnet_for_dump()
    losses = {'rec_X': [torch.tensor(9.0)], 'dis_M': [torch.tensor(9.0), torch.tensor(9.0)], 'unused': []}     # warm-up entries
    n_before = {k: len(v) for k, v in losses.items()}
    for step in range(3):                                   # three timed steps: one rec_X and two dis_M entries each
        losses['rec_X'].append(torch.tensor(float(step)))
        losses['dis_M'] += [torch.tensor(step + 0.25), nn_total([(1.0, torch.tensor(float(step))), (0.25, torch.tensor(2.0))])]
    budget = 4 << 20
    monkeypatch.setattr(bench, 'DUMP_WEIGHT_BYTES', budget)
    bench.dump_outputs(str(tmp_path / 'a'), model, losses, n_before, 3)
    bench.dump_outputs(str(tmp_path / 'b'), model, losses, n_before, 3)

    rec, dis = np.load(str(tmp_path / 'a' / 'loss_rec_X.npy')), np.load(str(tmp_path / 'a' / 'loss_dis_M.npy'))
    assert rec.dtype == np.float64 and rec.tolist() == [2.0]
    assert dis.tolist() == [2.25, 2.5]
    assert not (tmp_path / 'a' / 'loss_unused.npy').exists()

    models = bench.component_models(model)
    names = [m.name for m in models]
    assert len(set(names)) == len(names) and {'D_Mask', 'D_Image1', 'D_Image2', 'Segmentor', 'Decoder'} <= set(names)
    total = sum(m.arena.numel() + m.state_arena.numel() for m in models)
    assert total * 4 > budget                               # this case does sample
    files = sorted(os.listdir(str(tmp_path / 'a')))
    assert files == sorted(['loss_rec_X.npy', 'loss_dis_M.npy'] + ['weights_%s.npy' % n for n in names])
    assert sum(os.path.getsize(str(tmp_path / 'a' / f)) for f in files) <= budget + 128 * len(files)
    for m in models:
        a = np.load(str(tmp_path / 'a' / ('weights_%s.npy' % m.name)))
        b = np.load(str(tmp_path / 'b' / ('weights_%s.npy' % m.name)))
        full = np.concatenate([m.arena.numpy(), m.state_arena.numpy()])
        assert a.dtype == np.float32 and a.ndim == 1 and np.array_equal(a, b)
        assert a.size == int(full.size * budget / 4.0 / total) and np.isin(a, full).all()

    monkeypatch.setattr(bench, 'DUMP_WEIGHT_BYTES', 1 << 40)
    bench.dump_outputs(str(tmp_path / 'c'), model, losses, n_before, 3)
    m = models[0]
    assert np.array_equal(np.load(str(tmp_path / 'c' / ('weights_%s.npy' % m.name))), np.concatenate([m.arena.numpy(), m.state_arena.numpy()]))


def test_steps_below_one_are_refused():
    out = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py'), '--steps', '0'], stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                         timeout=300, cwd=ROOT)
    assert out.returncode != 0 and b'--steps' in out.stderr


def test_launcher_passes_an_absolute_dump_directory(tmp_path):
    env = dict(os.environ)
    for k in ('RANK', 'LOCAL_RANK', 'WORLD_SIZE'):
        env.pop(k, None)
    out = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py'), '--gpus', '2', '--dump-outputs', 'outs', '--dry-run'],
                         env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300, cwd=str(tmp_path))
    assert out.returncode == 0, out.stderr.decode()[-2000:]
    cmd = json.loads(out.stdout.decode().strip().splitlines()[-1])['cmd']
    assert cmd[cmd.index('--dump-outputs') + 1] == str(tmp_path / 'outs')


@pytest.mark.gpu
def test_bench_dumps_the_last_timed_step(tmp_path):
    """bench.py --steps K runs K timed steps, reports ms_per_step and, with --dump-outputs, writes the last step's outputs: finite
    float32 / float64 arrays, 64 MB at most"""
    import numpy as np
    out_dir = tmp_path / 'outs'
    cmd = [sys.executable, os.path.join(ROOT, 'bench.py'), '--gpus', '1', '--size', '64', '--steps', '3', '--warmup', '1',
           '--no-cpu-baseline', '--no-multi-stream-region', '--dump-outputs', str(out_dir)]
    env = dict(os.environ)
    for k in ('RANK', 'LOCAL_RANK', 'WORLD_SIZE'):
        env.pop(k, None)
    out = subprocess.run(cmd, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=900, cwd=ROOT)
    assert out.returncode == 0, out.stderr.decode()[-3000:]
    lines = [l for l in out.stdout.decode().splitlines() if l.startswith('{')]
    assert len(lines) == 1, out.stdout.decode()[-2000:]
    d = json.loads(lines[0])
    assert d['steps'] == 3 and d['ms_per_step'] > 0
    files = sorted(os.listdir(str(out_dir)))
    assert 'loss_rec_X.npy' in files and 'loss_dis_M.npy' in files and 'weights_D_Mask.npy' in files
    assert sum(os.path.getsize(str(out_dir / f)) for f in files) <= 64 << 20
    for f in files:
        a = np.load(str(out_dir / f))
        assert f.endswith('.npy') and a.dtype in (np.float32, np.float64) and a.size > 0 and np.isfinite(a).all(), f
    assert np.load(str(out_dir / 'loss_dis_M.npy')).size == 2          # two mask-discriminator fits per DAFNet step


def test_launcher_passes_full_to_the_ranks():
    env = dict(os.environ)
    for k in ('RANK', 'LOCAL_RANK', 'WORLD_SIZE'):
        env.pop(k, None)
    out = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py'), '--gpus', '2', '--full', '--dry-run'],
                         env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300, cwd=ROOT)
    assert out.returncode == 0, out.stderr.decode()[-2000:]
    cmd = json.loads(out.stdout.decode().strip().splitlines()[-1])['cmd']
    assert cmd[cmd.index(os.path.join(ROOT, 'bench.py')) + 1:] == ['--gpus', '2', '--full']


@pytest.mark.gpu
def test_plain_run_is_lean_and_full_adds_the_rest():
    """A plain run carries only what its own timed region measures; --full adds the CPU baseline and the informational
    multi-stream region on top of the same headline fields"""
    env = dict(os.environ)
    for k in ('RANK', 'LOCAL_RANK', 'WORLD_SIZE'):
        env.pop(k, None)
    lines = {}
    for extra in ([], ['--full']):
        cmd = [sys.executable, os.path.join(ROOT, 'bench.py'), '--gpus', '1', '--size', '64', '--steps', '2', '--warmup', '1'] + extra
        out = subprocess.run(cmd, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=900, cwd=ROOT)
        assert out.returncode == 0, out.stderr.decode()[-3000:]
        got = [l for l in out.stdout.decode().splitlines() if l.startswith('{')]
        assert len(got) == 1, out.stdout.decode()[-2000:]
        lines[bool(extra)] = json.loads(got[0])
    plain, full = lines[False], lines[True]
    for d in (plain, full):
        assert d['steps'] == 2 and d['warmup'] == 1 and d['value'] > 0 and d['ms_per_step'] > 0 and d['roofline']['frac'] > 0
        assert d['higher_is_better'] is True and d['dtype'] == 'f32' and d['unit'] == 'paired slices/s'
    assert plain['metric'] == full['metric']
    assert 'cpu_baseline' not in plain and 'multi_stream' not in plain
    assert full['cpu_baseline']['value'] > 0 and full['cpu_baseline']['kind'] == 'port'
    assert full['multi_stream']['value'] > 0 and full['multi_stream']['steps'] == 2
