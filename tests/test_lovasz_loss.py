"""Lovasz-Softmax loss (conf.w_lovasz; csrc/lovasz.hip, lovasz.py, models/trainer.py): the restatement of tests/lovasz_ref.py against
Berman's algorithm under torch fp64 autograd, the device map against the restatement (order exact, values to one fp32 ulp), the term
and its gradient against fp64 / the documented fp32 sequence, the refusals, and the trainer wiring -- off by default and bit-neutral,
the History entries and the CSV column, the epoch ramp, boundary and Lovasz together, hipGraph replays that follow the device weight,
fp16 with the dynamic loss scale, the command line.  Host logic runs on the CPU through the stand-ins of lovasz_ref; kernels run on the
GPU."""
import json
import os
import shutil

import numpy as np
import pytest
import torch

from tests import boundary_ref as BR
from tests import helpers as Hh
from tests import lovasz_ref as R

gpu = pytest.mark.gpu

# (B, H, W, C, nm).  The issue's shapes, then this kernel family's own edges (csrc/lovasz.hip): a wave of the scatter takes LV_WAVE = 512
# records (8 rows of 64), a block LV_TILE = 2048, and a segment gets ceil(HW / 2048) blocks -- so HW = 511 / 512 / 513 are one below, at
# and one above the wave's share, 2047 / 2048 / 2049 the block tile and the step from one block per segment to two, 4095 / 4096 / 4097
# the step from two blocks to three (a full last tile against a last tile of one record).
SHAPES = [(1, 1, 1, 2, 1), (1, 1, 63, 2, 1), (1, 1, 64, 2, 1), (1, 1, 65, 2, 1), (2, 37, 70, 4, 3), (3, 64, 64, 2, 1), (2, 65, 129, 8, 8),
          (9, 16, 257, 5, 4), (1, 300, 520, 5, 4),
          (1, 1, 511, 2, 1), (2, 1, 512, 3, 2), (1, 1, 513, 2, 1),
          (1, 1, 2047, 2, 1), (2, 1, 2048, 3, 2), (1, 1, 2049, 2, 1),
          (1, 1, 4095, 2, 1), (2, 1, 4096, 3, 2), (1, 1, 4097, 2, 1)]
HEADLINE = (8, 256, 256, 5, 4)
_ids = lambda s: 'x'.join(str(v) for v in s)


@pytest.fixture(params=['cpu', pytest.param('cuda', marks=gpu)])
def backend(request, monkeypatch):
    """'cpu': the C-ABI calls go to the torch-CPU stand-ins (tests/cpu_backend.py plus the boundary and Lovasz stand-ins, added here and
    removed afterwards); 'cuda': the real library"""
    from multimodal_segmentation_amd import _native, nn
    if request.param == 'cpu':
        from tests import cpu_backend as cb
        for table in (BR.STANDINS, R.STANDINS):
            for k, fn in table.items():
                monkeypatch.setitem(cb._TABLE, k, fn)
        monkeypatch.setattr(_native, 'call', cb._call)
        nn.set_default_device('cpu')
        yield 'cpu'
    else:
        nn.set_default_device('cuda:0')
        yield 'cuda:0'


class CallLog(object):
    """wrapper around _native.call: counts the entry points by name and keeps a copy of every loss value just before a combine adds
    a weighted term to it, with the term"""

    def __init__(self, monkeypatch):
        from multimodal_segmentation_amd import _native
        self.names, self.combines = [], []
        inner = _native.call

        def call(name, *args):
            if name == 'mmseg_boundary_combine':
                self.combines.append((float(args[0].item()), float(args[1].item()), float(args[2].item())))
            rc = inner(name, *args)
            self.names.append(name)
            return rc
        monkeypatch.setattr(_native, 'call', call)

    def count(self, name):
        return self.names.count(name)

    def lovasz_calls(self):
        return [n for n in self.names if n.startswith('mmseg_lovasz_')]


def _dev(a, dtype=torch.float32):
    return torch.as_tensor(np.array(a), dtype=dtype).to('cuda:0')


# ================================================ 1. the restatement =====================================================
def _berman(p, y):
    """Berman's lovasz_grad + lovasz_softmax_flat for one class, torch fp64: -> (loss, order); differentiable in p"""
    e = (y - p).abs()
    es, perm = torch.sort(e, stable=True, dim=0, descending=True)
    ys = y[perm]
    gts = ys.sum()
    inter = gts - ys.cumsum(0)
    union = gts + (1 - ys).cumsum(0)
    jac = 1.0 - inter / union
    if len(ys) > 1:
        jac = torch.cat([jac[:1], jac[1:] - jac[:-1]])
    return torch.dot(es, jac), perm


def _berman_cases():
    rng = np.random.RandomState(3)
    P = 97
    out = []
    for name in ('random', 'ties', 'exact01', 'G0', 'G1', 'GP', 'constant'):
        p = rng.rand(2, P, 3).astype(np.float32)
        t = (rng.rand(2, P, 3) > 0.5).astype(np.float32)
        if name == 'ties':
            p = (rng.randint(0, 5, (2, P, 3)) * 0.25).astype(np.float32)
        if name == 'exact01':
            p = rng.choice(np.array([0.0, 1.0, 0.5, 0.125], np.float32), (2, P, 3))
        if name == 'G0':
            t[0, :, 1] = 0
            t[1] = 0                                       # a sample without a class
        if name == 'G1':
            t[:, :, 0] = 0
            t[0, 17, 0] = t[1, 96, 0] = 1
        if name == 'GP':
            t[:, :, 2] = 1
        if name == 'constant':
            p[:] = 0.3
        out.append((name, p.reshape(2, 1, P, 3), t.reshape(2, 1, P, 3)))
    return out


@pytest.mark.parametrize('classes_all', [False, True], ids=['present', 'all'])
def test_the_restatement_is_bermans_algorithm(classes_all):
    """order, loss and gradient of the closed form against cumsum-Jaccard differences under torch fp64 autograd, to 1e-12.  The
    prediction enters torch as the fp64 image of the fp32 numbers, so |y - p| has the restatement's ties whenever they are exact."""
    nm = 3
    for name, p, t in _berman_cases():
        r = R.map_ref(p, t, nm, classes_all)
        B, P = p.shape[0], p.shape[2]
        pt = torch.tensor(r['e'].astype(np.float64), dtype=torch.float64)        # errors as the device sees them (fp32 values)
        y = torch.tensor(r['y'].astype(np.float64))
        # p64 such that |y - p64| is exactly the fp32 error: p64 = y -/+ e
        p64 = torch.where(y > 0.5, 1.0 - pt, pt).clone().requires_grad_(True)
        total = torch.zeros((), dtype=torch.float64)
        for b in range(B):
            G = y[b].sum(0)
            ks = [k for k in range(nm) if classes_all or G[k] > 0]
            for k in ks:
                loss, perm = _berman(p64[b, :, k], y[b, :, k])
                assert np.array_equal(perm.numpy(), r['order'][b, k]), (name, b, k)
                assert abs(float(loss.detach()) - r['term'][b, k]) <= 1e-12, (name, b, k)
                total = total + loss / (B * len(ks))
        want_L = float((r['term'] * r['q'][:, None] * (np.ones((B, nm)) if classes_all else (r['y'].sum(1) > 0))).sum())
        assert abs(float(total.detach()) - want_L) <= 1e-12, name
        got_L, _ = R.loss_ref(np.where(r['y'], 1.0 - r['e'].astype(np.float64), r['e'].astype(np.float64)), r['y'].astype(np.float32), r['m'], nm)
        assert abs(got_L - want_L) <= 1e-12, name
        if total.requires_grad:
            total.backward()
            assert np.abs(p64.grad.numpy() - r['m']).max() <= 1e-12, name
        else:
            assert not r['m'].any(), name
        assert np.all(r['m'][r['e'] == 0] == 0) and 0.0 <= want_L <= 1.0 + 1e-12


def test_closed_form_edge_values():
    g = R.lovasz_grad_closed(np.array([0, 0, 0], bool))
    assert g.tolist() == [1.0, 0.0, 0.0]
    g = R.lovasz_grad_closed(np.array([1, 1, 1], bool))
    assert np.allclose(g, [1 / 3.0] * 3, rtol=1e-15) and abs(g.sum() - 1) < 1e-15
    g = R.lovasz_grad_closed(np.array([0, 1, 0, 1], bool))             # J: 1-2/3, 1-1/3, 1-1/4, 1
    assert np.allclose(np.cumsum(g), [1 / 3.0, 2 / 3.0, 3 / 4.0, 1.0], rtol=1e-15)


# ================================================ 2. the map on the device ================================================
def _check_map(shape, pkind, mkind, classes_all):
    from multimodal_segmentation_amd import ops
    B, H, W, C, nm = shape
    c = R.case(shape, pkind, mkind, classes_all)
    p, t = _dev(c['pred']), _dev(c['target'])
    m_dev = ops.lovasz_map(p, t, nm, classes_all)
    again = ops.lovasz_map(p, t, nm, classes_all)
    assert m_dev.shape == (B, H, W, nm) and m_dev.dtype == torch.float32
    assert torch.equal(m_dev, again), 'two runs differ'
    m = m_dev.cpu().numpy().astype(np.float64).reshape(B, H * W, nm)
    ref, e, y = c['m'], c['e'], c['y']
    assert np.all(m[e == 0] == 0.0), 'm must be exactly 0 where the error is 0'
    assert np.all(m[y] <= 0.0) and np.all(m[~y] >= 0.0), 'sign: negative on the positives, positive on the negatives'
    assert np.all((m != 0) == (ref != 0)), 'zeros of the map differ from the restatement'
    # the device evaluates the same integer expression in fp64 (a quotient, q_b = 1 / (B |K_b|), their product: three roundings of
    # 2^-53) and rounds to fp32 once: at most one fp32 ulp from the rounded reference, 2^-23 |m_ref|; every element is compared
    err, lim = np.abs(m - ref), 2.0 ** -23 * np.abs(ref)
    assert err.size == B * H * W * nm and np.all(err <= lim), 'max excess %g at %s' % (float((err - lim).max()), np.argwhere(err > lim)[:5].tolist())


@gpu
@pytest.mark.parametrize('pkind', R.PRED_KINDS)
@pytest.mark.parametrize('shape', SHAPES, ids=_ids)
def test_map_is_the_stable_sort_and_the_closed_form(shape, pkind):
    for mkind in R.MASK_KINDS:
        for classes_all in (False, True):
            _check_map(shape, pkind, mkind, classes_all)


@gpu
def test_map_at_the_headline_geometry():
    _check_map(HEADLINE, 'softmax_like', 'mixed', False)


@gpu
def test_non_finite_predictions_terminate_and_write_every_element():
    from multimodal_segmentation_amd import ops
    shape = (2, 37, 70, 4, 3)
    c = R.case(shape, 'uniform', 'mixed')
    p = np.array(c['pred'])
    p.reshape(-1)[::7] = np.nan
    p.reshape(-1)[3::11] = np.inf
    p.reshape(-1)[5::13] = -np.inf
    from multimodal_segmentation_amd import _native as N
    B, H, W, C, nm = shape
    m = torch.full((B, H, W, nm), 123.0, device='cuda:0')
    ws = torch.empty((N.call('mmseg_lovasz_workspace_bytes', B, H * W, nm) + 3) // 4, dtype=torch.int32, device='cuda:0')
    N.call('mmseg_lovasz_map', _dev(p), _dev(c['target']), m, ws, B, H * W, C, nm, 0)
    torch.cuda.synchronize()
    assert not bool((m == 123.0).any()), 'an element was not written'


# ================================================ 3. term and gradient =====================================================
TERM_SHAPES = [(1, 1, 1, 2, 1), (2, 37, 70, 4, 3), (2, 65, 129, 8, 8), (9, 16, 257, 5, 4), (1, 300, 520, 5, 4)]


@gpu
@pytest.mark.parametrize('pkind', ('uniform', 'softmax_like'))
@pytest.mark.parametrize('shape', TERM_SHAPES, ids=_ids)
def test_term_against_fp64(shape, pkind):
    from multimodal_segmentation_amd import ops
    B, H, W, C, nm = shape
    c = R.case(shape, pkind, 'mixed')
    want, abs_sum = R.loss_ref(c['pred'], c['target'], c['m32'], nm)
    bound = R.loss_bound(B, H * W, nm, want, abs_sum)
    args = (_dev(c['pred']), _dev(c['target']), _dev(c['m32'].reshape(B, H, W, nm)), nm)
    ll, again = ops.lovasz_term(*args), ops.lovasz_term(*args)
    got = float(ll.item())
    print('L %r, fp64 %r, |diff| %.3g, bound %.3g' % (got, want, abs(got - want), bound))
    assert ll.shape == (1,) and got == float(again.item())
    assert abs(got - want) <= bound
    assert 0.0 <= got <= 1.0 + 2.0 ** -20
    # and the term of the device's own map is the mean of the per-pair dot products of the restatement
    m_dev = ops.lovasz_map(args[0], args[1], nm)
    got2 = float(ops.lovasz_term(args[0], args[1], m_dev, nm).item())
    want2 = float((c['term'] * c['q'][:, None] * (c['y'].sum(1) > 0)).sum())
    # (all terms >= 0: relative errors add up -- 2^-23 of the device map, 2^-24 of the restatement's fp32 e, 2^-24 of the final rounding,
    # the fp64 sum far below: 2^-22, doubled for the second-order terms)
    assert abs(got2 - want2) <= 2.0 ** -21 * want2


@gpu
@pytest.mark.parametrize('with_scale_dev', [False, True], ids=['static', 'scale_dev'])
@pytest.mark.parametrize('shape', TERM_SHAPES, ids=_ids)
def test_gradient_is_added_in_the_documented_order(shape, with_scale_dev):
    from multimodal_segmentation_amd import ops
    B, H, W, C, nm = shape
    m32 = R.case(shape, 'uniform', 'mixed')['m32'].reshape(B, H, W, nm)
    scale_host, sd, w = 1.7, (1024.0 if with_scale_dev else None), 0.37
    d0 = np.random.RandomState(11).standard_normal((B, H, W, C)).astype(np.float32)
    w_dev = _dev([w])
    sd_dev = _dev([sd]) if with_scale_dev else None
    dpred = _dev(d0)
    ops.lovasz_grad_add(_dev(m32), dpred, nm, scale_host, w_dev, scale_dev=sd_dev)
    got = dpred.cpu().numpy()
    want = R.grad_add_f32(m32, d0, nm, scale_host, sd, w)
    assert np.array_equal(got[..., nm:], d0[..., nm:]), 'channels >= num_masks were touched'
    assert np.array_equal(got[..., :nm], want[..., :nm]), 'not the fp32 sequence ((scale_host * scale_dev) * weight) * m, then the addition'


# ================================================ 4. refusals =============================================================
def test_workspace_queries_run_without_a_gpu_and_return_0_for_refused_arguments():
    from multimodal_segmentation_amd import _native as N
    assert N.call('mmseg_lovasz_workspace_bytes', 2, 37 * 70, 3) == R.lovasz_workspace_bytes(2, 37 * 70, 3) >= 2 * 6 * 37 * 70 * 8
    assert N.call('mmseg_lovasz_workspace_bytes', 1, 1 << 22, 8) == R.lovasz_workspace_bytes(1, 1 << 22, 8)
    for bad in (dict(nm=0), dict(nm=9), dict(HW=0), dict(HW=(1 << 22) + 1), dict(B=0), dict(B=65536)):
        a = dict(B=2, HW=256, nm=2)
        a.update(bad)
        assert N.call('mmseg_lovasz_workspace_bytes', a['B'], a['HW'], a['nm']) == 0, bad
    assert N.call('mmseg_lovasz_loss_workspace_floats', 3) >= 3 and N.call('mmseg_lovasz_loss_workspace_floats', 0) == 0


@gpu
def test_refused_arguments_return_the_error_and_write_nothing():
    from multimodal_segmentation_amd import _native as N
    sentinel = 123.0
    n = 16 * 16 * 2
    p = torch.full((n,), 0.25, device='cuda:0')
    t = torch.ones(n, device='cuda:0')
    m = torch.full((n,), sentinel, device='cuda:0')
    ws = torch.full((65536,), 77, dtype=torch.int32, device='cuda:0')
    ok = dict(B=1, HW=256, C=2, nm=2)
    for bad in [dict(nm=3), dict(nm=0), dict(C=9, nm=2), dict(HW=0), dict(HW=(1 << 22) + 1), dict(B=65536), dict(B=0),
                'null_pred', 'null_target', 'null_m', 'null_ws']:
        a = dict(ok)
        if isinstance(bad, dict):
            a.update(bad)
        args = [None if bad == 'null_pred' else p, None if bad == 'null_target' else t, None if bad == 'null_m' else m, None if bad == 'null_ws' else ws]
        with pytest.raises(N.NativeLibraryError):
            N.call('mmseg_lovasz_map', args[0], args[1], args[2], args[3], a['B'], a['HW'], a['C'], a['nm'], 0)
        torch.cuda.synchronize()
        assert bool((m == sentinel).all()) and bool((ws == 77).all()), bad
    one, w = torch.full((1,), sentinel, device='cuda:0'), torch.ones(1, device='cuda:0')
    wsf = torch.zeros(1024, device='cuda:0')
    for C, nm, ll in ((2, 0, one), (2, 3, one), (9, 2, one), (2, 2, None)):
        with pytest.raises(N.NativeLibraryError):
            N.call('mmseg_lovasz_loss', p, t, p, ll, wsf, 1, 256, C, nm)
    d = torch.full((n,), sentinel, device='cuda:0')
    for C, nm, wd in ((2, 0, w), (2, 3, w), (9, 2, w), (2, 2, None)):
        with pytest.raises(N.NativeLibraryError):
            N.call('mmseg_lovasz_grad_add', p, d, 1, 256, C, nm, 1.0, None, wd)
    torch.cuda.synchronize()
    assert float(one.item()) == sentinel and bool((d == sentinel).all())


# ================================================ 5. configuration ========================================================
def test_parse_conf_and_its_refusals():
    from multimodal_segmentation_amd import lovasz as Lv
    assert Lv.parse_conf({}) is None and Lv.parse_conf({'w_lovasz': 0}) is None
    assert Lv.parse_conf({'w_lovasz': 0.0, 'lovasz_ramp_epochs': 0, 'lovasz_classes': 'all'}) is None
    assert Lv.parse_conf({'w_lovasz': 0.5}) == (0.5, 0, 'present')
    assert Lv.parse_conf({'w_lovasz': 2, 'lovasz_ramp_epochs': 4, 'lovasz_classes': 'all'}) == (2.0, 4, 'all')
    for bad in [{'w_lovasz': -0.1}, {'w_lovasz': float('nan')}, {'w_lovasz': float('inf')}, {'w_lovasz': 'big'}, {'w_lovasz': True},
                {'lovasz_ramp_epochs': 4}, {'w_lovasz': 0, 'lovasz_ramp_epochs': 2}, {'w_lovasz': 0.5, 'lovasz_ramp_epochs': -1},
                {'w_lovasz': 0.5, 'lovasz_ramp_epochs': 2.5}, {'w_lovasz': 0.5, 'lovasz_classes': 'some'}, {'lovasz_classes': None},
                {'w_lovasz': 0.5, 'lovasz_classes': 1}]:
        with pytest.raises(ValueError):
            Lv.parse_conf(bad)


def test_command_line_overrides_the_configuration_and_is_recorded(tmp_path, monkeypatch):
    from multimodal_segmentation_amd.experiment import Experiment, parse_arguments
    monkeypatch.chdir(tmp_path)
    plain = Experiment().get_config(0, parse_arguments(['--config', 'dafnet_config_chaos', '--split', '0']))
    assert all(k not in plain for k in ('w_lovasz', 'lovasz_ramp_epochs', 'lovasz_classes'))
    args = parse_arguments(['--config', 'dafnet_config_chaos', '--split', '0', '--w_lovasz', '0.25', '--lovasz_ramp_epochs', '3',
                            '--lovasz_classes', 'all'])
    assert args.w_lovasz == 0.25 and args.lovasz_ramp_epochs == 3 and args.lovasz_classes == 'all'
    conf = Experiment().get_config(0, args)
    assert conf.w_lovasz == 0.25 and conf.lovasz_ramp_epochs == 3 and conf.lovasz_classes == 'all'
    assert conf.folder == plain.folder == "dafnet_chaos_l1_['t1', 't2']_split0", 'the option does not rename the run folder'
    dumped = json.load(open(os.path.join(conf.folder, 'experiment_configuration.json')))
    assert dumped['w_lovasz'] == 0.25 and dumped['lovasz_ramp_epochs'] == 3 and dumped['lovasz_classes'] == 'all'
    with pytest.raises(SystemExit):
        parse_arguments(['--config', 'dafnet_config_chaos', '--split', '0', '--lovasz_classes', 'some'])


# ================================================ 6. trainer level ========================================================
def _dafnet(size, **extra):
    from multimodal_segmentation_amd.configuration import dafnet_config_chaos
    from multimodal_segmentation_amd.models.dafnet import DAFNet
    conf = Hh.make_conf(dafnet_config_chaos, size, **extra)
    model = DAFNet(conf)
    model.build()
    return conf, model


def _gen_models(model):
    return model._generator_models() + [model.D_Mask, model.D_Image1, model.D_Image2]


def _targets(d, B):
    ones = np.ones((B, 1), np.float32)
    return [d['m1'], d['m2'], d['m1'], d['m2']] + [ones] * 4 + [d['x1'], d['x2'], d['x1'], d['x2']] + [ones] * 4 + \
           [np.zeros(B, np.float32)] * 2 + [d['z1'], d['z2']]


def _supervised_steps(model, data, B, ref_w, eps=True, after=None):
    """-> (histories as dicts, weights) of len(data) supervised steps from the weights ref_w"""
    ms = _gen_models(model)
    for m, w in zip(ms, ref_w):
        m.set_weights(w)
    model.Enc_Modality._eps_rng = None
    hs = []
    for i, d in enumerate(data):
        kw = {'eps': [d['eps1'], d['eps2']]} if eps else {}
        h = model.supervised_trainer.fit([d['x1'], d['x2'], d['z1'], d['z2']], _targets(d, B), **kw)
        hs.append({k: h.history[k][0] for k in h.history.keys()})
        if after is not None:
            after(i)
    return hs, [w.copy() for m in ms for w in m.get_weights()]


def test_off_by_default_and_bit_neutral_at_weight_zero(backend, monkeypatch):
    size, B = (48, 2) if backend == 'cpu' else (64, 2)
    data = [Hh.make_step_data(B, size, size, seed=70)]
    log = CallLog(monkeypatch)
    runs, ref_w = [], None
    for extra in ({}, {'w_lovasz': 0.0, 'lovasz_classes': 'all'}):
        conf, model = _dafnet(size, **extra)
        assert model.lovasz is None and model.supervised_trainer.lovasz is None and model.unsupervised_trainer.lovasz is None
        model.set_lovasz_epoch(3)                              # nothing to set: no launch, no error
        if ref_w is None:
            ref_w = [m.get_weights() for m in _gen_models(model)]
        runs.append(_supervised_steps(model, data, B, ref_w))
    assert log.lovasz_calls() == [] and log.count('mmseg_boundary_combine') == 0, 'no entry point of the term may be launched when it is off'
    for hs, ws in runs[1:]:
        assert hs == runs[0][0] and all('Segmentor_lovasz' not in h for h in hs)
        for a, b in zip(ws, runs[0][1]):
            assert np.array_equal(a, b)


def test_weighted_term_enters_the_loss_the_history_and_the_gradient(backend, monkeypatch):
    size, B = (48, 2) if backend == 'cpu' else (64, 2)
    data = [Hh.make_step_data(B, size, size, seed=70)]
    conf0, model0 = _dafnet(size)
    ref_w = [m.get_weights() for m in _gen_models(model0)]
    hs0, ws0 = _supervised_steps(model0, data, B, ref_w)
    conf, model = _dafnet(size, w_lovasz=0.5)
    assert model.lovasz is not None and model.supervised_trainer.lovasz is model.unsupervised_trainer.lovasz is model.lovasz
    assert model.D_Mask_trainer.lovasz is None and float(model.lovasz.weight_dev.item()) == 0.5 and model.boundary is None
    assert model.supervised_trainer.lovasz_all is False
    log = CallLog(monkeypatch)
    hs, ws = _supervised_steps(model, data, B, ref_w)
    h = hs[0]
    # four Segmentor outputs, each with its own prediction: four maps, four terms, four gradients, four combines
    assert log.count('mmseg_lovasz_map') == log.count('mmseg_lovasz_loss') == log.count('mmseg_lovasz_grad_add') == 4, log.lovasz_calls()
    assert log.count('mmseg_boundary_combine') == 4 and log.count('mmseg_boundary_map') == 0
    assert 'Segmentor_lovasz' in h and np.isfinite(h['Segmentor_lovasz']) and 0.0 <= h['Segmentor_lovasz'] <= 1.0 + 1e-6
    # the forward pass is the parent's (same weights, same data): what seg_loss wrote for the last Segmentor output IS the parent's loss
    before, term, w = log.combines[-1]
    assert before == hs0[0]['Segmentor_loss'] and term == h['Segmentor_lovasz'] and w == 0.5
    want = float(np.float32(before) + np.float32(np.float32(0.5) * np.float32(term)))
    assert h['Segmentor_loss'] == want, (h['Segmentor_loss'], before, term)
    assert h['Segmentor_loss'] > hs0[0]['Segmentor_loss']
    assert any(not np.array_equal(a, b) for a, b in zip(ws, ws0)), 'the Lovasz term did not reach the weights'
    d = data[0]
    hu = model.unsupervised_trainer.fit([d['x1'], d['x2'], d['z1'], d['z2']], Hh.dafnet_targets(d, False), eps=[d['eps1'], d['eps2']])
    assert log.count('mmseg_lovasz_map') == 4 + 2 and 'Segmentor_lovasz' in hu.history


def test_boundary_and_lovasz_together(backend, monkeypatch):
    size, B = (48, 2) if backend == 'cpu' else (64, 2)
    data = [Hh.make_step_data(B, size, size, seed=71)]
    conf0, model0 = _dafnet(size, w_boundary=0.25)
    ref_w = [m.get_weights() for m in _gen_models(model0)]
    hs0, _ = _supervised_steps(model0, data, B, ref_w)
    conf, model = _dafnet(size, w_boundary=0.25, w_lovasz=0.5, lovasz_classes='all')
    assert model.boundary is not None and model.lovasz is not None and model.lovasz is not model.boundary
    assert model.supervised_trainer.lovasz_all is True
    log = CallLog(monkeypatch)
    hs, _ = _supervised_steps(model, data, B, ref_w)
    h = hs[0]
    assert log.count('mmseg_boundary_map') == 2 and log.count('mmseg_lovasz_map') == 4 and log.count('mmseg_boundary_combine') == 8
    # per output: seg_loss, the boundary entry points, then the Lovasz ones
    seq = [n for n in log.names if n.startswith(('mmseg_lovasz_', 'mmseg_boundary_')) and 'workspace' not in n and n != 'mmseg_boundary_map']
    assert seq[:8] == ['mmseg_boundary_loss', 'mmseg_boundary_grad_add', 'mmseg_boundary_combine',
                       'mmseg_lovasz_map', 'mmseg_lovasz_loss', 'mmseg_lovasz_grad_add', 'mmseg_boundary_combine', 'mmseg_boundary_loss'], seq[:8]
    assert h['Segmentor_boundary'] == hs0[0]['Segmentor_boundary']
    before, term, w = log.combines[-1]
    assert before == hs0[0]['Segmentor_loss'] and term == h['Segmentor_lovasz'] and w == 0.5
    assert h['Segmentor_loss'] == float(np.float32(before) + np.float32(np.float32(0.5) * np.float32(term)))


def test_mmsdnet_dice_outputs_carry_the_term_and_the_executor_logs_it(backend, monkeypatch):
    from multimodal_segmentation_amd.configuration import mmsdnet_config_chaos
    from multimodal_segmentation_amd.models.mmsdnet import MMSDNet
    from multimodal_segmentation_amd.model_executors.mmsdnet_executor import MMSDNetExecutor
    size = 48 if backend == 'cpu' else 64
    np.random.seed(123)
    conf = Hh.make_conf(mmsdnet_config_chaos, size, batch_size=2, l_mix=1.0, w_lovasz=0.25, multi_stream=False)
    model = MMSDNet(conf)
    model.build()
    assert model.supervised_trainer.lovasz is not None
    ex = MMSDNetExecutor(conf, model)
    ex.init_train_data(slices_per_volume=2)
    losses = {n: [] for n in ex.get_loss_names() + ['lovasz']}
    log = CallLog(monkeypatch)
    ex.train_batch(losses)
    n_seg = sum(1 for s in model.supervised_trainer.specs if s.name == 'Segmentor')
    assert log.count('mmseg_lovasz_map') == log.count('mmseg_lovasz_loss') == n_seg == 2 + 2 * 2 * 1
    assert len(losses['lovasz']) == 1 and np.isfinite(float(losses['lovasz'][0])) and 'boundary' not in losses


def test_invalid_values_raise_when_the_model_is_built_and_the_ramp_sets_the_weight(backend):
    from multimodal_segmentation_amd.configuration import dafnet_config_chaos
    from multimodal_segmentation_amd.models.dafnet import DAFNet
    for bad in (dict(w_lovasz=-1.0), dict(lovasz_ramp_epochs=3), dict(w_lovasz=float('nan')), dict(w_lovasz=0.5, lovasz_classes='some')):
        with pytest.raises(ValueError):
            DAFNet(Hh.make_conf(dafnet_config_chaos, 48, **bad)).build()
    conf, model = _dafnet(48, w_lovasz=0.4, lovasz_ramp_epochs=4)
    buf = model.lovasz.weight_dev
    assert float(buf.item()) == float(np.float32(0.1))         # epoch 0
    for e, want in enumerate((0.1, 0.2, 0.4 * 3 / 4, 0.4, 0.4)):
        model.set_lovasz_epoch(e)
        assert float(model.lovasz.weight_dev.item()) == float(np.float32(want))
    assert model.lovasz.weight_dev is buf, 'the ramp must write into the one buffer the recorded kernels read'


def test_executor_writes_the_csv_column_and_sets_the_epoch(backend, monkeypatch):
    """two tiny epochs of the DAFNet executor's own loop with a ramp of 2 (validation and checkpoints, which the term has no part in,
    left out): the weight the combines read goes w/2 -> w, training.csv ends with a `lovasz` column"""
    from multimodal_segmentation_amd.model_executors.dafnet_executor import DAFNetExecutor
    size = 48 if backend == 'cpu' else 64
    np.random.seed(123)
    conf, model = _dafnet(size, batch_size=2, l_mix=1.0, epochs=2, slices_per_volume=1, w_lovasz=0.2, lovasz_ramp_epochs=2)
    ex = DAFNetExecutor(conf, model)
    monkeypatch.setattr(ex, 'validate', lambda epoch_loss: None)
    monkeypatch.setattr(ex, 'save_models', lambda *a, **k: None)
    init = ex.init_train_data

    def one_batch_per_epoch(*a, **k):
        init(*a, **k)
        ex.batches = 1
    monkeypatch.setattr(ex, 'init_train_data', one_batch_per_epoch)
    log = CallLog(monkeypatch)
    shutil.rmtree(conf.folder, ignore_errors=True)
    total = ex.train()
    rows = open(os.path.join(conf.folder, 'training.csv')).read().strip().split('\n')
    head = rows[0].split(',')
    assert head[-1] == 'lovasz' and 'boundary' not in head and len(rows) == 3
    assert all(np.isfinite(float(r.split(',')[-1])) for r in rows[1:]) and len(total['lovasz']) == 2
    ws = sorted(set(w for _, _, w in log.combines))
    assert ws == [float(np.float32(0.1)), float(np.float32(0.2))], ws
    shutil.rmtree(conf.folder, ignore_errors=True)


@gpu
def test_graph_replays_follow_a_weight_changed_after_the_capture():
    """five steps eager and five recorded (two eager warm-ups, the capture, two replays); the weight goes from w/2 to w after step 4,
    after the capture: a weight baked into the recording would leave step 5 at w/2"""
    from multimodal_segmentation_amd import nn
    nn.set_default_device('cuda:0')
    B, size, steps = 2, 64, 5
    data = [Hh.make_step_data(B, size, size, seed=40 + i) for i in range(steps)]
    runs, ref_w = {}, None
    for mode in (False, True):
        conf, model = _dafnet(size, hip_graphs=mode, w_lovasz=0.5, lovasz_ramp_epochs=2)
        if ref_w is None:
            ref_w = [m.get_weights() for m in _gen_models(model)]
        assert model.supervised_trainer.use_graph == mode and float(model.lovasz.weight_dev.item()) == 0.25

        def after(i, model=model):
            if i == 3:
                model.set_lovasz_epoch(1)
        runs[mode] = _supervised_steps(model, data, B, ref_w, eps=False, after=after)
        assert float(model.lovasz.weight_dev.item()) == 0.5
        if mode:
            g = model.supervised_trainer._graphs
            assert len(g) == 1 and list(g.values())[0].graph is not None, 'the step was not recorded'
    (h0, w0), (h1, w1) = runs[False], runs[True]
    assert all('Segmentor_lovasz' in h for h in h1)
    assert h0 == h1, 'losses differ between the eager and the replayed steps'
    for a, b in zip(w0, w1):
        assert np.array_equal(a, b)
    conf, model = _dafnet(size, hip_graphs=True, w_lovasz=0.5, lovasz_ramp_epochs=2)
    h2, _ = _supervised_steps(model, data, B, ref_w, eps=False)
    assert h2[3] == h1[3] and h2[4]['Segmentor_loss'] != h1[4]['Segmentor_loss']


@gpu
def test_fp16_with_the_dynamic_loss_scale_runs_a_step_without_a_skip():
    from multimodal_segmentation_amd import nn, ops as P
    nn.set_default_device('cuda:0')
    try:
        conf, model = _dafnet(64, compute_dtype='fp16', loss_scale='dynamic', w_lovasz=0.5)
        d = Hh.make_step_data(2, 64, 64, seed=70)
        h = model.supervised_trainer.fit([d['x1'], d['x2'], d['z1'], d['z2']], _targets(d, 2), eps=[d['eps1'], d['eps2']])
        vals = {k: h.history[k][0] for k in h.history.keys()}
        assert all(np.isfinite(v) for v in vals.values()), vals
        assert 'Segmentor_lovasz' in vals
        sc = model.supervised_trainer.scaler
        assert sc is not None and sc.skipped_steps() == 0 and sc.iterations() == 1
    finally:
        P.set_conv_precision('fp32')
        P.set_activation_storage(False)
