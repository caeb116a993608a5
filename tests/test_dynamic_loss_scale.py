"""Dynamic fp16 loss scaling (conf.loss_scale = 'dynamic', loss_scaler.py): GradScaler semantics with the scale, the skip flag, the
counters and the Adam iteration count in device memory.

GPU: the three new kernels at op level (unscale + non-finite check, guarded Adam, the scaler state machine), transparency (a dynamic
run that never overflows is bitwise the static-1024 run), the overflow path (skipped steps leave weights and moments bitwise
untouched, the scale backs off, training then proceeds), hipGraph replays with recurring skips, and an executor epoch.
CPU (torch-CPU stand-ins registered here for the new entry points): conf validation, bf16 / fp32 carry no scaler, and a gloo world-2
run where one rank's local gradient overflows: both ranks skip and the replicas stay identical."""
import logging
import os
import socket

import numpy as np
import pytest
import torch

from tests import helpers as Hh

H = 64


# ---- torch-CPU stand-ins of the new entry points (the CPU backend lives in tests/cpu_backend.py; registered from here) ----------
def _cpu_segloss_grad_s(pred, target, coef, dpred, B, HW, C, nm, scale, scale_dev, use_bce):
    from tests import cpu_backend as cb
    s = float(torch.tensor(scale, dtype=torch.float32) * scale_dev[0])
    return cb._TABLE['mmseg_segloss_grad'](pred, target, coef, dpred, B, HW, C, nm, s, use_bce)


def _cpu_diffloss_grad_s(p, t, tconst, n, mode, scale, scale_dev, dp):
    from tests import cpu_backend as cb
    s = float(torch.tensor(scale, dtype=torch.float32) * scale_dev[0])
    return cb._TABLE['mmseg_diffloss_grad'](p, t, tconst, n, mode, s, dp)


def _cpu_spectral_grad4_s(w0, w1, w2, w3, sgn, dw0, dw1, dw2, dw3, n, n0, n1, n2, n3, scale, scale_dev):
    from tests import cpu_backend as cb
    s = float(torch.tensor(scale, dtype=torch.float32) * scale_dev[0])
    return cb._TABLE['mmseg_spectral_grad4'](w0, w1, w2, w3, sgn, dw0, dw1, dw2, dw3, n, n0, n1, n2, n3, s)


def _cpu_unscale_check8(g0, g1, g2, g3, g4, g5, g6, g7, n0, n1, n2, n3, n4, n5, n6, n7, count, scale, st):
    inv = 1.0 / scale[0]
    for g, n in list(zip((g0, g1, g2, g3, g4, g5, g6, g7), (n0, n1, n2, n3, n4, n5, n6, n7)))[:count]:
        v = g.view(-1)[:n]
        if not bool(torch.isfinite(v).all()):
            st[0] = 1
        v.mul_(inv)
    return 0


def _cpu_adam_guarded(p, g, m, v, n, table, tlen, st, b1, b2, eps):
    from tests import cpu_backend as cb
    if int(st[0]):
        return 0
    k = min(int(st[3]) + 1, tlen)
    return cb._TABLE['mmseg_adam'](p, g, m, v, n, float(table[k - 1]), b1, b2, eps)


def _cpu_loss_scale_update(scale, st, interval):
    s, found, count, skipped, it = _host_update(float(scale[0]), int(st[0]), int(st[1]), int(st[2]), int(st[3]), interval)
    scale[0] = s
    st.copy_(torch.tensor([0, count, skipped, it], dtype=torch.int32))
    return 0


STANDINS = {'mmseg_segloss_grad_s': _cpu_segloss_grad_s, 'mmseg_diffloss_grad_s': _cpu_diffloss_grad_s,
            'mmseg_spectral_grad4_s': _cpu_spectral_grad4_s, 'mmseg_unscale_check8': _cpu_unscale_check8,
            'mmseg_adam_guarded': _cpu_adam_guarded, 'mmseg_loss_scale_update': _cpu_loss_scale_update}


def _host_update(scale, found, count, skipped, it, interval):
    """host restatement of loss_scale_update_kernel -> (scale, 0, growth count, skipped, iterations)"""
    if found:
        return max(scale * 0.5, 1.0), 0, 0, skipped + 1, it
    count += 1
    if count >= interval:
        return (scale * 2.0 if scale < 2.0 ** 127 else scale), 0, 0, skipped, it + 1
    return scale, 0, count, skipped, it + 1


@pytest.fixture
def cpu_dynamic(cpu_backend, monkeypatch):
    for k, fn in STANDINS.items():
        monkeypatch.setitem(cpu_backend._TABLE, k, fn)
    from multimodal_segmentation_amd import nn
    nn.set_default_device('cpu')
    yield cpu_backend


# ================================================ CPU ==================================================================
def test_conf_validation():
    from multimodal_segmentation_amd import loss_scaler as L
    C = dict
    assert L.parse_conf(C()) is None and L.parse_conf(C(loss_scale=512.0)) is None
    assert L.parse_conf(C(loss_scale='dynamic')) == (1024.0, 2000)
    assert L.parse_conf(C(loss_scale='dynamic', loss_scale_init=2.0 ** 40, loss_scale_growth_interval=1)) == (2.0 ** 40, 1)
    for bad in [dict(loss_scale='Dynamic'), dict(loss_scale='auto'), dict(loss_scale='dynamic', loss_scale_init=1000.0),
                dict(loss_scale='dynamic', loss_scale_init=0.5), dict(loss_scale='dynamic', loss_scale_init=float('inf')),
                dict(loss_scale='dynamic', loss_scale_init=-1024.0), dict(loss_scale='dynamic', loss_scale_init='big'),
                dict(loss_scale='dynamic', loss_scale_growth_interval=0), dict(loss_scale='dynamic', loss_scale_growth_interval=2.5)]:
        with pytest.raises(ValueError):
            L.parse_conf(C(**bad))
    t = L.lr_table(1e-4, 0.9, 0.999)
    import math
    for k in (1, 2, 10, 1000, len(t)):
        assert t[k - 1] == 1e-4 * math.sqrt(1. - 0.999 ** k) / (1. - 0.9 ** k)
    assert t[-1] == 1e-4 and t[-2] != 1e-4


@pytest.mark.parametrize('dtype', ['fp32', 'bf16', 'fp16'])
def test_only_fp16_dynamic_carries_scalers(cpu_dynamic, dtype):
    from multimodal_segmentation_amd import ops as P
    from multimodal_segmentation_amd.configuration import dafnet_config_chaos
    from multimodal_segmentation_amd.models.dafnet import DAFNet
    from multimodal_segmentation_amd.loss_scaler import LossScaler
    try:
        model = DAFNet(Hh.make_conf(dafnet_config_chaos, 48, compute_dtype=dtype, loss_scale='dynamic', loss_scale_init=2.0 ** 12))
        model.build()
        trainers = [getattr(model, n) for n in model._TRAINERS if getattr(model, n, None) is not None]
        assert len(trainers) >= 5
        for t in trainers:
            assert t.loss_scale == 1.0
            if dtype == 'fp16':
                assert isinstance(t.scaler, LossScaler) and t.scaler.scale() == 2.0 ** 12 and t.scaler.iterations() == 0
            else:
                assert t.scaler is None
        assert len(set(id(t.scaler) for t in trainers)) == (len(trainers) if dtype == 'fp16' else 1)
        assert [n for n, _ in model.loss_scalers()] == ([n for n in model._TRAINERS if getattr(model, n, None) is not None]
                                                        if dtype == 'fp16' else [])
        # the static default is untouched
        static = DAFNet(Hh.make_conf(dafnet_config_chaos, 48, compute_dtype=dtype))
        static.build()
        assert static.supervised_trainer.scaler is None
        assert static.supervised_trainer.loss_scale == (1024.0 if dtype == 'fp16' else 1.0)
        with pytest.raises(ValueError):
            DAFNet(Hh.make_conf(dafnet_config_chaos, 48, compute_dtype=dtype, loss_scale='dynamic', loss_scale_init=1000.0)).build()
    finally:
        P.set_conv_precision('fp32')
        P.set_activation_storage(False)


def test_discriminator_step_dynamic_equals_static_on_cpu(cpu_dynamic):
    """the Spectral regulariser's gradient follows the device scale: three D_Mask steps with a dynamic scaler at 1024 are bitwise
    the static-1024 steps (stand-in arithmetic)"""
    from multimodal_segmentation_amd.configuration import dafnet_config_chaos
    from multimodal_segmentation_amd.models.dafnet import DAFNet
    from multimodal_segmentation_amd.loss_scaler import LossScaler
    conf = Hh.make_conf(dafnet_config_chaos, 48)
    model = DAFNet(conf)
    model.build()
    d = Hh.make_step_data(2, 48, 48)
    w0 = model.D_Mask.get_weights()
    out = {}
    for mode in ('static', 'dynamic'):
        model.D_Mask.set_weights(w0)
        tr = model._d_trainer(model.D_Mask, 'D_Mask_' + mode, conf.d_mask_params.lr)
        if mode == 'static':
            tr.loss_scale = 1024.0
        else:
            tr.scaler = LossScaler(tr.optimizer, 'cpu', 1024.0, 2000)
        losses = [tr.fit([d['dm_m1'], d['dm_m2']], [1.0, 0.0]).history['loss'][0] for _ in range(3)]
        st = tr.optimizer.state[model.D_Mask.uid]
        out[mode] = (losses, model.D_Mask.arena.clone(), st[0].clone(), st[1].clone())
    assert out['static'][0] == out['dynamic'][0]
    for a, b in zip(out['static'][1:], out['dynamic'][1:]):
        assert torch.equal(a, b)
    assert tr.scaler.iterations() == 3 and tr.scaler.skipped_steps() == 0


def _free_port():
    s = socket.socket()
    s.bind(('127.0.0.1', 0))
    p = s.getsockname()[1]
    s.close()
    return p


class _Poison(torch.autograd.Function):
    """identity whose backward puts +inf into the first gradient element when asked (a local fp16 overflow on one rank)"""

    @staticmethod
    def forward(ctx, x, on):
        ctx.on = on
        return x

    @staticmethod
    def backward(ctx, g):
        if ctx.on:
            g = g.clone()
            g.view(-1)[0] = float('inf')
        return g, None


def _dp_worker(rank, world, port, q):
    try:
        _dp_worker_body(rank, world, port, q)
    except BaseException as exc:          # surface the failure instead of letting the parent wait for its timeout
        import traceback
        q.put((rank, 'error', traceback.format_exc(), repr(exc)))
        raise


def _dp_worker_body(rank, world, port, q):
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    torch.set_num_threads(2)
    dist.init_process_group('gloo', rank=rank, world_size=world)
    from tests import cpu_backend as cb
    cb.install()
    cb._TABLE.update(STANDINS)                      # (a fresh spawned process: nothing to restore)
    from multimodal_segmentation_amd import nn, ops
    from multimodal_segmentation_amd.loss_scaler import LossScaler
    from multimodal_segmentation_amd.models.trainer import Trainer, OutputSpec
    from multimodal_segmentation_amd.parallel import dp
    nn.set_default_device('cpu')
    dp.enable(True)

    class Tiny(nn.Model):
        def __init__(self):
            super(Tiny, self).__init__('TinySeg')
            nn.conv_params(self, 'c', 1, 8, 5)
            self.finalize(np.random.RandomState(3))

        def forward(self, x, training=False):
            return ops.softmax(nn.conv(self, 'c', x))
    m = Tiny()
    poison = {'on': False}
    tr = Trainer('tiny', lambda ins, training=True: [_Poison.apply(m(ins[0]), poison['on'])], [OutputSpec('Segmentor', 'dice_bce', 10.0)],
                 [m], nn.Adam(1e-3), num_masks=4)
    tr.scaler = LossScaler(tr.optimizer, 'cpu', 2.0 ** 10, 2)
    dp.broadcast_models([m])
    d = Hh.make_step_data(2, H // 2, H // 2, seed=5)
    x = np.random.RandomState(11 + rank).standard_normal((1, H // 2, H // 2, 8)).astype(np.float32)   # per-rank data
    rec = []
    for step in range(5):
        poison['on'] = (step == 2 and rank == 1)
        before = (m.arena.clone(), [t.clone() for t in tr.optimizer.state.get(m.uid, ())])
        tr.fit([x], [d['m1'][rank:rank + 1]])
        sc = tr.scaler
        unchanged = torch.equal(before[0], m.arena) and all(torch.equal(a, b) for a, b in zip(before[1], tr.optimizer.state[m.uid]))
        ok, cs = dp.replicas_identical([m])
        rec.append((sc.scale(), sc.skipped_steps(), sc.iterations(), sc.growth_count(), unchanged, ok))
    q.put((rank, rec))
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.timeout(600)
def test_dp_gloo_world2_overflow_on_one_rank_skips_on_both():
    import torch.multiprocessing as mp
    ctx = mp.get_context('spawn')
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_dp_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = {}
    try:
        for _ in range(2):
            item = q.get(timeout=500)
            assert item[1] != 'error', item[2]
            res[item[0]] = item[1]
    finally:
        for p in procs:
            p.join(timeout=60)
            if p.is_alive():
                p.terminate()
    assert res[0] == res[1], res                     # same scale / counters / skip decision on both ranks
    rec = res[0]
    # growth interval 2: 1024 -> 2048 after steps 0, 1; step 2 overflows on rank 1 -> skipped on both, back to 1024; then 2 applied
    assert [r[:4] for r in rec] == [(1024.0, 0, 1, 1), (2048.0, 0, 2, 0), (1024.0, 1, 2, 0), (1024.0, 1, 3, 1), (2048.0, 1, 4, 0)], rec
    assert [r[4] for r in rec] == [False, False, True, False, False]
    assert all(r[5] for r in rec)


# ================================================ GPU ==================================================================
def _scaler_state(device='cuda:0'):
    return torch.full((1,), 1024.0, device=device), torch.zeros(4, dtype=torch.int32, device=device)


@pytest.mark.gpu
def test_unscale_check_kernel_flags_every_non_finite_position():
    from multimodal_segmentation_amd import ops
    dev = torch.device('cuda:0')
    lens = [7, 1030, 4099, 5, 262147, 1, 33, 70001]          # none a multiple of 4 except by accident of the tail: all have tails
    rng = np.random.RandomState(0)
    base = [torch.from_numpy(rng.standard_normal(n).astype(np.float32) * 1e3).to(dev) for n in lens]
    S = 2.0 ** 10
    # clean: flag clear, bitwise axpby(g, g, 1/S, 0)
    for k in (1, 3, 8):
        scale, st = _scaler_state()
        scale.fill_(S)
        gs = [b.clone() for b in base[:k]]
        ops.unscale_check(gs, scale, st)
        assert int(st[0].item()) == 0
        for g, b in zip(gs, base):
            assert torch.equal(g, ops.axpby(b, b, 1.0 / S, 0.0))
    cases = [(0, 0), (7, lens[7] - 1), (1, 1029), (1, 1028), (4, lens[4] - 3), (2, 2050), (2, 0), (5, 0), (6, 32)]
    vals = [float('inf'), float('-inf'), float('nan')]
    for ci, (a, i) in enumerate(cases):
        for v in vals:
            scale, st = _scaler_state()
            scale.fill_(S)
            gs = [b.clone() for b in base]
            gs[a][i] = v
            ops.unscale_check(gs, scale, st)
            assert int(st[0].item()) == 1, (a, i, v)
            assert int(st[1:].abs().sum().item()) == 0          # only the flag is touched
    # a flag already set is never cleared by a clean pass
    scale, st = _scaler_state()
    st[0] = 1
    ops.unscale_check([b.clone() for b in base[:2]], scale, st)
    assert int(st[0].item()) == 1


@pytest.mark.gpu
def test_guarded_adam_is_adam_p_or_nothing():
    from multimodal_segmentation_amd import ops, loss_scaler as L
    from multimodal_segmentation_amd import _native as N
    dev = torch.device('cuda:0')
    rng = np.random.RandomState(1)
    n = 4099
    mk = lambda s=1.0: torch.from_numpy((rng.standard_normal(n) * s).astype(np.float32)).to(dev)
    p0, g, m0, v0 = mk(), mk(1e-2), mk(1e-3), mk(1e-4).abs()
    table = torch.tensor(L.lr_table(1e-4, 0.9, 0.999), dtype=torch.float32, device=dev)
    for it in (0, 4, 999, table.numel() - 1, table.numel() + 500):
        _, st = _scaler_state()
        st[3] = it
        p, m, v = p0.clone(), m0.clone(), v0.clone()
        ops.adam_guarded(p, g, m, v, table, st, 0.9, 0.999, 1e-7)
        lr = table[min(it + 1, table.numel()) - 1:min(it + 1, table.numel())].clone()
        pr, mr, vr = p0.clone(), m0.clone(), v0.clone()
        N.call('mmseg_adam_p', pr, g, mr, vr, n, lr, 0.9, 0.999, 1e-7)
        assert torch.equal(p, pr) and torch.equal(m, mr) and torch.equal(v, vr), it
        assert not torch.equal(p, p0)
        assert st.tolist() == [0, 0, 0, it]             # the count advances in the scaler update, not here
        st[0] = 1
        p, m, v = p0.clone(), m0.clone(), v0.clone()
        ops.adam_guarded(p, g, m, v, table, st, 0.9, 0.999, 1e-7)
        assert torch.equal(p, p0) and torch.equal(m, m0) and torch.equal(v, v0)
        assert st.tolist() == [1, 0, 0, it]


@pytest.mark.gpu
@pytest.mark.parametrize('init,interval', [(8.0, 3), (2.0 ** 126, 1)])
def test_scaler_state_machine_matches_the_host_restatement(init, interval):
    from multimodal_segmentation_amd import ops
    flags = [0, 0, 0, 1, 0, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 1, 0, 0, 0, 0]
    scale, st = _scaler_state()
    scale.fill_(init)
    host = (init, 0, 0, 0, 0)
    for f in flags:
        st[0] = f
        ops.loss_scale_update(scale, st, interval)
        host = _host_update(host[0], f, host[2], host[3], host[4], interval)
        assert (float(scale.item()),) + tuple(st.tolist()) == host, (f, scale.item(), st.tolist(), host)
    assert host[3] == sum(flags) and host[4] == len(flags) - sum(flags)
    assert 1.0 <= float(scale.item()) <= 2.0 ** 127


def _build(which, dtype='fp16', **extra):
    from multimodal_segmentation_amd import nn
    nn.set_default_device('cuda:0')
    if which == 'dafnet':
        from multimodal_segmentation_amd.configuration import dafnet_config_chaos
        from multimodal_segmentation_amd.models.dafnet import DAFNet
        conf = Hh.make_conf(dafnet_config_chaos, H, batch_size=2, compute_dtype=dtype, decoder_type='film', **extra)
        model = DAFNet(conf)
    else:
        from multimodal_segmentation_amd.configuration import mmsdnet3_config_chaos
        from multimodal_segmentation_amd.models.mmsdnet import MMSDNet
        conf = Hh.make_conf(mmsdnet3_config_chaos, H, batch_size=2, compute_dtype=dtype, **extra)
        model = MMSDNet(conf)
    model.build()
    return conf, model


def _models(model):
    ms = list(model._generator_models())
    for n in ('D_Mask', 'D_Image1', 'D_Image2', 'Balancer'):
        m = getattr(model, n, None)
        if m is not None and m not in ms:
            ms.append(m)
    return ms


def _moments(model):
    out = []
    for n in model._TRAINERS:
        t = getattr(model, n, None)
        if t is not None:
            for m in t.train_models:
                st = t.optimizer.state.get(m.uid)
                out += [x.detach().cpu().numpy().copy() for x in st] if st is not None else [None]
    return out


def _reset_precision():
    from multimodal_segmentation_amd import ops as P
    P.set_activation_storage(False)
    P.set_conv_precision('fp32')


@pytest.mark.gpu
@pytest.mark.parametrize('which', ['dafnet', 'mmsdnet3'])
def test_dynamic_without_overflow_is_bitwise_static_1024(which):
    """'dynamic' from 1024 with a growth interval longer than the run == the static 1024 scale: every loss of five executor
    iterations (each several trainer fits), every weight and both Adam moments of every trainer, bitwise"""
    runs, ref_w = {}, None
    try:
        for mode in ('static', 'dynamic'):
            np.random.seed(123)
            extra = {} if mode == 'static' else dict(loss_scale='dynamic', loss_scale_init=1024.0, loss_scale_growth_interval=10 ** 6)
            conf, model = _build(which, **extra)
            ms = _models(model)
            if ref_w is None:
                ref_w = [m.get_weights() for m in ms]
            else:
                for m, w in zip(ms, ref_w):
                    m.set_weights(w)
            model.Enc_Modality._eps_rng = None
            if which == 'dafnet':
                from multimodal_segmentation_amd.model_executors.dafnet_executor import DAFNetExecutor as Ex
            else:
                from multimodal_segmentation_amd.model_executors.mmsdnet_executor import MMSDNetExecutor as Ex
            ex = Ex(conf, model)
            np.random.seed(321)
            ex.init_train_data(slices_per_volume=3)
            losses = {n: [] for n in ex.get_loss_names()}
            for _ in range(5):
                ex.train_batch(losses)
            if mode == 'dynamic':
                scs = model.loss_scalers()
                assert len(scs) >= 3
                for name, sc in scs:
                    assert sc.skipped_steps() == 0 and sc.scale() == 1024.0, name
                    assert getattr(model, name).optimizer.iterations == 0            # the count lives on the device
                iters = {name: sc.iterations() for name, sc in scs}
                assert iters['supervised_trainer'] >= 5 and iters['D_Mask_trainer'] >= 5, iters
            else:
                iters = {n: getattr(model, n).optimizer.iterations for n in model._TRAINERS if getattr(model, n, None) is not None}
            runs[mode] = ({k: [float(v.item()) if hasattr(v, 'item') else float(v) for v in vs] for k, vs in losses.items()},
                          [w.copy() for m in ms for w in m.get_weights()], _moments(model), iters)
    finally:
        _reset_precision()
    (l0, w0, m0, i0), (l1, w1, m1, i1) = runs['static'], runs['dynamic']
    assert sum(len(v) for v in l0.values()) > 0
    assert l0 == l1, 'losses differ between the static and the dynamic loss scale'
    assert i0 == i1
    assert len(w0) == len(w1) and all(np.array_equal(a, b) for a, b in zip(w0, w1))
    assert len(m0) == len(m1) and all((a is None and b is None) or np.array_equal(a, b) for a, b in zip(m0, m1))


def _fixed_generator_batch(model, seed=9):
    d = Hh.make_step_data(2, H, H, seed=seed)
    B1 = np.ones((2, 1), np.float32)
    tg = [d['m1'], d['m2'], d['m1'], d['m2']] + [B1] * 4 + [d['x1'], d['x2'], d['x1'], d['x2']] + [B1] * 4 + \
         [np.zeros(2, np.float32)] * 2 + [d['z1'], d['z2']]
    return d, tg


@pytest.mark.gpu
def test_overflowing_scale_skips_steps_then_trains():
    """init 2^40 overflows the fp16 data-gradient operands: each skipped step leaves weights and Adam moments bitwise unchanged and
    halves the scale; once the scale fits, steps apply, weights stay finite and the fixed-batch objective decreases"""
    try:
        conf, model = _build('dafnet', loss_scale='dynamic', loss_scale_init=2.0 ** 40)
        tr = model.supervised_trainer
        sc = tr.scaler
        d, tg = _fixed_generator_batch(model)
        eps = [d['eps1'], d['eps2']]
        applied, skips = [], 0
        for step in range(60):
            w_before = [m.arena.clone() for m in tr.train_models]
            mo_before = [x.clone() for m in tr.train_models for x in tr.optimizer.state.get(m.uid, ())]
            s_before, k_before, it_before = sc.scale(), sc.skipped_steps(), sc.iterations()
            loss = tr.fit([d['x1'], d['x2'], d['z1'], d['z2']], tg, eps=eps).history['loss'][0]
            if sc.skipped_steps() == k_before + 1:
                skips += 1
                assert sc.scale() == max(s_before / 2, 1.0) and sc.iterations() == it_before
                assert all(torch.equal(a, m.arena) for a, m in zip(w_before, tr.train_models))
                mo_after = [x for m in tr.train_models for x in tr.optimizer.state.get(m.uid, ())]
                if not mo_before:                    # the very first step creates the (zero) moments
                    assert mo_after and all(not bool(x.any()) for x in mo_after)
                else:
                    assert len(mo_after) == len(mo_before) and all(torch.equal(a, b) for a, b in zip(mo_before, mo_after))
            else:
                assert sc.skipped_steps() == k_before and sc.iterations() == it_before + 1 and sc.scale() == s_before
                applied.append(loss)
            if len(applied) >= 8:
                break
        assert skips > 0 and sc.skipped_steps() == skips, skips
        assert sc.scale() < 2.0 ** 40
        assert len(applied) >= 8, (skips, applied)
        for m in tr.train_models:
            assert bool(torch.isfinite(m.arena).all()), m.name
        assert all(np.isfinite(v) for v in applied) and applied[-1] < applied[0], applied
    finally:
        _reset_precision()


@pytest.mark.gpu
def test_graph_replays_with_recurring_skips_are_bitwise_the_eager_dynamic_run():
    """conf.hip_graphs with init 2^36 and growth interval 1: the scale keeps growing into overflow, so skips recur during the
    replays; twelve generator + discriminator fits are bitwise the eager dynamic run (losses, weights, moments, scaler state)"""
    steps = 12
    runs, ref_w = {}, None
    try:
        for graphs_on in (False, True):
            conf, model = _build('dafnet', hip_graphs=graphs_on, loss_scale='dynamic', loss_scale_init=2.0 ** 36,
                                 loss_scale_growth_interval=1)
            ms = _models(model)
            if ref_w is None:
                ref_w = [m.get_weights() for m in ms]
            else:
                for m, w in zip(ms, ref_w):
                    m.set_weights(w)
            model.Enc_Modality._eps_rng = None
            assert model.supervised_trainer.use_graph == graphs_on
            rng = np.random.RandomState(3)
            losses, skipped = [], []
            for i in range(steps):
                d, tg = _fixed_generator_batch(model, seed=40 + i)
                h = model.D_Mask_trainer.fit([d['m1'][..., :4].copy(), rng.rand(2, H, H, 4).astype(np.float32)], [1.0, 0.0])
                losses.append(h.history['loss'][0])
                h = model.supervised_trainer.fit([d['x1'], d['x2'], d['z1'], d['z2']], tg)
                losses += [h.history[k][0] for k in h.history.keys()]
                skipped.append(model.supervised_trainer.scaler.skipped_steps())
            if graphs_on:
                g = model.supervised_trainer._graphs
                assert len(g) == 1 and list(g.values())[0].graph is not None, 'the generator step was not recorded'
            scs = [(sc.scale(), sc.skipped_steps(), sc.iterations(), sc.growth_count()) for _, sc in model.loss_scalers()]
            runs[graphs_on] = (losses, [w.copy() for m in ms for w in m.get_weights()], _moments(model), scs, skipped)
    finally:
        _reset_precision()
    (l0, w0, m0, s0, k0), (l1, w1, m1, s1, k1) = runs[False], runs[True]
    assert k0 == k1 and s0 == s1
    assert k0[-1] > k0[3], 'no step was skipped during the replays (steps 4..12): %r' % k0
    assert l0 == l1
    assert all(np.array_equal(a, b) for a, b in zip(w0, w1))
    assert all((a is None and b is None) or np.array_equal(a, b) for a, b in zip(m0, m1))


@pytest.mark.gpu
def test_mmsdnet3_executor_epoch_logs_the_scalers(tmp_path, caplog):
    """a short epoch of the 3-modality MMSDNet executor in dynamic fp16 mode runs, keeps its csv columns and logs every trainer's
    scale and skipped-step count"""
    from multimodal_segmentation_amd.model_executors.mmsdnet_executor import MMSDNetExecutor
    try:
        conf, model = _build('mmsdnet3', loss_scale='dynamic', epochs=1, slices_per_volume=2, folder=str(tmp_path / 'dyn_mmsdnet3'))
        ex = MMSDNetExecutor(conf, model)
        with caplog.at_level(logging.INFO):
            total = ex.train()
        names = [n for n, _ in model.loss_scalers()]
        assert {'supervised_trainer', 'D_Mask_trainer'} <= set(names), names
        for n, sc in model.loss_scalers():
            assert sc.iterations() + sc.skipped_steps() > 0 or n == 'unsupervised_trainer', n
            assert any(('%s loss scale' % n) in r.getMessage() and 'skipped steps' in r.getMessage() for r in caplog.records), n
        assert ex.log_loss_scalers() == {n: (sc.scale(), sc.skipped_steps()) for n, sc in model.loss_scalers()}
        with open(conf.folder + '/training.csv') as f:
            assert f.readline().strip() == 'epoch,' + ','.join(ex.get_loss_names())
        for k in ('supervised_Mask', 'adv_M', 'rec_X', 'dis_M'):
            assert np.isfinite(total[k][0]), (k, total[k])
    finally:
        _reset_precision()
