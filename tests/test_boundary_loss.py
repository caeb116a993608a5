"""Boundary loss (conf.w_boundary; csrc/boundary.hip, boundary.py, models/trainer.py): the signed distance map against the scipy
restatement of tests/boundary_ref.py (exact squared distances, fp32 rounding of the root), the term and its gradient against fp64 with
bounds derived from the kernels as written, the refusals, and the trainer wiring -- off by default and bit-neutral, the History
entries, the epoch ramp, one map per distinct target, hipGraph replays that follow the device weight, fp16 with the dynamic loss
scale, the command line.  Host logic runs on the CPU through the stand-ins of boundary_ref; kernels run on the GPU."""
import os
import shutil

import numpy as np
import pytest
import torch

from tests import boundary_ref as R
from tests import helpers as Hh

gpu = pytest.mark.gpu

# (B, H, W, C, nm).  The last of the first eight is larger than a column tile and an LDS stage in both axes; the odd extents cross wave
# and tile edges.  The two after it are this kernel family's own edges: H = 2048 forces a one-column tile whose LDS stage is the
# largest the column pass ever asks for (64 KiB), W = 2048 the largest row stage and the longest per-lane runs of the row pass; the
# column tile grows beyond its least width only once B * W reaches 2048: B * W = 2313 gives two-column tiles and, W being odd, a
# narrower last one.
SHAPES = [(1, 1, 1, 2, 1), (1, 1, 130, 2, 1), (1, 130, 1, 2, 1), (2, 37, 70, 4, 3), (3, 64, 64, 2, 1), (2, 65, 129, 8, 8),
          (2, 256, 256, 5, 4), (1, 300, 520, 5, 4), (1, 2048, 5, 8, 8), (1, 3, 2048, 8, 8), (9, 16, 257, 5, 4)]
_ids = lambda s: 'x'.join(str(v) for v in s)


@pytest.fixture(params=['cpu', pytest.param('cuda', marks=gpu)])
def backend(request, monkeypatch):
    """'cpu': the C-ABI calls go to the torch-CPU stand-ins (tests/cpu_backend.py plus the boundary stand-ins, added here and removed
    afterwards); 'cuda': the real library"""
    from multimodal_segmentation_amd import _native, nn
    if request.param == 'cpu':
        from tests import cpu_backend as cb
        for k, fn in R.STANDINS.items():
            monkeypatch.setitem(cb._TABLE, k, fn)
        monkeypatch.setattr(_native, 'call', cb._call)         # what cb.install() does; undone with the table entries, in reverse order
        nn.set_default_device('cpu')
        yield 'cpu'
    else:
        nn.set_default_device('cuda:0')
        yield 'cuda:0'


class CallLog(object):
    """wrapper around _native.call: counts the entry points by name and keeps a copy of the loss mmseg_segloss_finalize wrote"""

    def __init__(self, monkeypatch):
        from multimodal_segmentation_amd import _native
        self.names, self.seg_losses = [], []
        inner = _native.call

        def call(name, *args):
            rc = inner(name, *args)
            self.names.append(name)
            if name == 'mmseg_segloss_finalize':
                self.seg_losses.append(args[1].clone())
            return rc
        monkeypatch.setattr(_native, 'call', call)

    def count(self, name):
        return self.names.count(name)

    def boundary_calls(self):
        return [n for n in self.names if n.startswith('mmseg_boundary_')]


def _dev(a, dtype=torch.float32):
    return torch.as_tensor(np.array(a), dtype=dtype).to('cuda:0')


# ================================================ 1. the map ==============================================================
@gpu
@pytest.mark.parametrize('kind', R.CONTENTS)
@pytest.mark.parametrize('shape', SHAPES, ids=_ids)
def test_map_is_the_exact_distance_transform(shape, kind):
    from multimodal_segmentation_amd import ops
    B, H, W, C, nm = shape
    c = R.case(shape, kind)
    t = _dev(c['target'])
    phi_dev = ops.boundary_map(t, nm)
    again = ops.boundary_map(t, nm)
    assert phi_dev.shape == (B, H, W, nm) and phi_dev.dtype == torch.float32
    assert torch.equal(phi_dev, again), 'two runs differ'
    phi = phi_dev.cpu().numpy().astype(np.float64)
    sq, fg, ref = c['sq'], c['fg'], c['phi']
    none = sq < 0                                              # the mask of this (b, k) is empty or full
    assert np.all(phi[none] == 0.0), 'an empty or a full mask must give exactly 0'
    got_sq = np.where(fg, np.rint((1.0 - phi) ** 2), np.rint(phi ** 2)).astype(np.int64)
    bad = (got_sq != sq) & ~none
    assert not bad.any(), 'squared distances differ at %s: got %s, scipy %s' % (np.argwhere(bad)[:5].tolist(), got_sq[bad][:5], sq[bad][:5])
    assert np.all((phi[~none] > 0) == ~fg[~none]), 'sign: negative or zero inside, positive outside'
    ref32 = ref.astype(np.float32).astype(np.float64)
    err = np.abs(phi - ref32)
    lim = 2.0 ** -23 * np.maximum(1.0, np.abs(ref))
    assert np.all(err <= lim), 'max excess %g' % float((err - lim).max())
    assert np.array_equal(phi.astype(np.float32), c['phi32']), 'not the fp32 sequence sqrtf, then - 1'


def test_the_restatement_is_one_hot2dist():
    """the restatement against the paper's expression on scipy's fp64 distances, and its own fp32 sequence against the bound the GPU
    test uses"""
    from scipy.ndimage import distance_transform_edt as edt
    for kind in R.CONTENTS:
        c = R.case((2, 37, 70, 4, 3), kind)
        for b in range(2):
            for k in range(3):
                pos = c['fg'][b, ..., k]
                want = np.zeros(pos.shape)
                if pos.any() and not pos.all():
                    want = edt(~pos) * ~pos - (edt(pos) - 1) * pos
                assert np.allclose(c['phi'][b, ..., k], want, rtol=1e-14, atol=0), kind
        assert np.all(np.abs(c['phi32'].astype(np.float64) - c['phi'].astype(np.float32)) <= 2.0 ** -23 * np.maximum(1.0, np.abs(c['phi'])))
    t = R.case((1, 1, 130, 2, 1), 'threshold_049_051')['target']
    assert set(np.unique(t[..., 0])) <= {np.float32(0.49), np.float32(0.5), np.float32(0.51)} and not R.case((1, 1, 130, 2, 1), 'threshold_049_051')['fg'][0, 0, 0, 0]


# ================================================ 2. term and gradient =====================================================
LOSS_KINDS = ('smooth_noise', 'far_blobs', 'centre_hole')


@gpu
@pytest.mark.parametrize('kind', LOSS_KINDS)
@pytest.mark.parametrize('shape', SHAPES, ids=_ids)
def test_term_against_fp64(shape, kind):
    from multimodal_segmentation_amd import ops
    B, H, W, C, nm = shape
    phi32, p = R.case(shape, kind)['phi32'], R.softmax_pred(shape)
    want, abs_mean = R.loss_ref(p, phi32, nm)
    # (sequential fused multiply-adds per thread + 12 levels of block_sum, twice: per chunk and over the 128 B partials, + 1 for the division)
    # * 2^-24 * sum |p * phi| / N; the counts are derived from the kernels as written in boundary_ref.loss_bound
    bound = R.loss_bound(B, H * W, nm, abs_mean)
    lb = ops.boundary_term(_dev(p), _dev(phi32), nm)
    again = ops.boundary_term(_dev(p), _dev(phi32), nm)
    got = float(lb.item())
    print('L_B %r, fp64 %r, |diff| %.3g, bound %.3g' % (got, want, abs(got - want), bound))
    assert lb.shape == (1,) and got == float(again.item())
    assert abs(got - want) <= bound


@gpu
@pytest.mark.parametrize('with_scale_dev', [False, True], ids=['static', 'scale_dev'])
@pytest.mark.parametrize('shape', SHAPES, ids=_ids)
def test_gradient_is_added_in_the_documented_order(shape, with_scale_dev):
    from multimodal_segmentation_amd import ops
    B, H, W, C, nm = shape
    phi32, p = R.case(shape, 'smooth_noise')['phi32'], R.softmax_pred(shape)
    scale_host, sd, w = 1.7, (1024.0 if with_scale_dev else None), 0.37
    d0 = np.random.RandomState(11).standard_normal((B, H, W, C)).astype(np.float32)
    w_dev = _dev([w])
    sd_dev = _dev([sd]) if with_scale_dev else None
    dpred = _dev(d0)
    ops.boundary_grad_add(_dev(phi32), dpred, nm, scale_host, w_dev, scale_dev=sd_dev)
    got = dpred.cpu().numpy()
    want = R.grad_add_f32(phi32, d0, nm, scale_host, sd, w)
    assert np.array_equal(got[..., nm:], d0[..., nm:]), 'channels >= num_masks were touched'
    ulp = np.spacing(np.abs(want[..., :nm]))
    assert np.all(np.abs(got[..., :nm].astype(np.float64) - want[..., :nm]) <= 2 * ulp)
    # linearity: sum p * (gradient from a zeroed dpred) = weight * scale * L_B, within the bound of the term times that factor
    z = torch.zeros_like(dpred)
    ops.boundary_grad_add(_dev(phi32), z, nm, scale_host, w_dev, scale_dev=sd_dev)
    lhs = float((p.astype(np.float64) * z.cpu().numpy().astype(np.float64)).sum())
    lb, abs_mean = R.loss_ref(p, phi32, nm)
    factor = float(np.float32(w)) * float(np.float32(scale_host)) * (sd or 1.0)
    assert abs(lhs - factor * lb) <= factor * R.loss_bound(B, H * W, nm, abs_mean)


@gpu
def test_combine_adds_the_weighted_term_and_keeps_the_raw_one():
    from multimodal_segmentation_amd import ops
    loss, lb, w = _dev([0.8125]), _dev([-3.3]), _dev([0.3])
    ops.boundary_combine(loss, lb, w)
    assert float(loss.item()) == float(np.float32(0.8125) + np.float32(0.3) * np.float32(-3.3)) and float(lb.item()) == float(np.float32(-3.3))


# ================================================ 3. properties ===========================================================
def test_truth_scores_below_zero_and_a_shifted_truth_scores_worse(backend):
    from multimodal_segmentation_amd import nn, ops
    H = W = 64
    ii, jj = np.indices((H, W))
    m = ((ii - 30) ** 2 + (jj - 24) ** 2 <= 11 ** 2).astype(np.float32)
    target = np.stack([m, 1 - m], -1)[None]
    dev = torch.device(backend)
    phi = ops.boundary_map(nn.to_device(target, dev), 1)
    vals = []
    for shift in (0, 1, 3, 9):
        p = np.roll(target, shift, axis=2)
        vals.append(float(ops.boundary_term(nn.to_device(p, dev), phi, 1).item()))
    assert vals[0] <= 0.0, vals
    assert vals[0] < vals[1] < vals[2] < vals[3], vals


# ================================================ 4. refusals =============================================================
BAD = [dict(nm=0), dict(nm=3, C=2), dict(C=9, nm=9), dict(C=9, nm=2), dict(H=2049), dict(W=2049), dict(B=0)]


def test_workspace_queries_run_without_a_gpu_and_return_0_for_refused_arguments():
    from multimodal_segmentation_amd import _native as N
    assert N.call('mmseg_boundary_workspace_bytes', 2, 37, 70, 3) == 2 * 37 * 70 * 3 * 4
    assert N.call('mmseg_boundary_workspace_bytes', 1, 2048, 2048, 8) == 2048 * 2048 * 8 * 4
    for bad in (dict(nm=0), dict(nm=9), dict(H=2049), dict(W=2049), dict(H=0), dict(B=0)):
        a = dict(B=2, H=16, W=16, nm=2)
        a.update(bad)
        assert N.call('mmseg_boundary_workspace_bytes', a['B'], a['H'], a['W'], a['nm']) == 0, bad
    assert N.call('mmseg_boundary_loss_workspace_floats', 3) >= 3 and N.call('mmseg_boundary_loss_workspace_floats', 0) == 0


@gpu
def test_refused_arguments_return_the_error_and_write_nothing():
    from multimodal_segmentation_amd import _native as N
    ok = dict(B=1, H=16, W=16, C=2, nm=2)
    sentinel = 123.0
    for bad in BAD + ['null_target', 'null_phi', 'null_ws']:
        a = dict(ok)
        if isinstance(bad, dict):
            a.update(bad)
        n_t = max(a['B'], 1) * a['H'] * a['W'] * a['C']
        t = torch.ones(n_t, device='cuda:0')
        phi = torch.full((max(a['B'], 1) * a['H'] * a['W'] * max(a['nm'], 1),), sentinel, device='cuda:0')
        ws = torch.full((phi.numel(),), 77, dtype=torch.int32, device='cuda:0')
        args = [None if bad == 'null_target' else t, None if bad == 'null_phi' else phi, None if bad == 'null_ws' else ws]
        with pytest.raises(N.NativeLibraryError):
            N.call('mmseg_boundary_map', args[0], args[1], args[2], a['B'], a['H'], a['W'], a['C'], a['nm'])
        torch.cuda.synchronize()
        assert bool((phi == sentinel).all()) and bool((ws == 77).all()), bad
    one, w = torch.full((1,), sentinel, device='cuda:0'), torch.ones(1, device='cuda:0')
    p = torch.ones(16 * 16 * 2, device='cuda:0')
    wsf = torch.zeros(1024, device='cuda:0')
    for C, nm, lb in ((2, 0, one), (2, 3, one), (9, 2, one), (2, 2, None)):
        with pytest.raises(N.NativeLibraryError):
            N.call('mmseg_boundary_loss', p, p, lb, wsf, 1, 256, C, nm)
    d = torch.full((16 * 16 * 2,), sentinel, device='cuda:0')
    for C, nm, wd in ((2, 0, w), (2, 3, w), (9, 2, w), (2, 2, None)):
        with pytest.raises(N.NativeLibraryError):
            N.call('mmseg_boundary_grad_add', p, d, 1, 256, C, nm, 1.0, None, wd)
    with pytest.raises(N.NativeLibraryError):
        N.call('mmseg_boundary_combine', one, one, None)
    torch.cuda.synchronize()
    assert float(one.item()) == sentinel and bool((d == sentinel).all())


# ================================================ 5. trainer level ========================================================
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
    data = [Hh.make_step_data(B, size, size, seed=70 + i) for i in range(2)]
    log = CallLog(monkeypatch)
    runs, ref_w = [], None
    for extra in ({}, {"w_boundary": 0}):
        conf, model = _dafnet(size, **extra)
        assert model.boundary is None and model.supervised_trainer.boundary is None and model.unsupervised_trainer.boundary is None
        model.set_boundary_epoch(3)                            # nothing to set: no launch, no error
        if ref_w is None:
            ref_w = [m.get_weights() for m in _gen_models(model)]
        runs.append(_supervised_steps(model, data, B, ref_w))
    assert log.boundary_calls() == [], 'the boundary entry points must not be launched when the option is off'
    assert log.count('mmseg_segloss_finalize') == 2 * 2 * 4
    for hs, ws in runs[1:]:
        assert hs == runs[0][0] and all('Segmentor_boundary' not in h for h in hs)
        for a, b in zip(ws, runs[0][1]):
            assert np.array_equal(a, b)


def test_weighted_term_enters_the_loss_the_history_and_the_gradient(backend, monkeypatch):
    size, B = (48, 2) if backend == 'cpu' else (64, 2)
    data = [Hh.make_step_data(B, size, size, seed=70)]
    conf0, model0 = _dafnet(size)
    ref_w = [m.get_weights() for m in _gen_models(model0)]
    hs0, ws0 = _supervised_steps(model0, data, B, ref_w)
    conf, model = _dafnet(size, w_boundary=0.5)
    assert model.boundary is not None and model.supervised_trainer.boundary is model.unsupervised_trainer.boundary is model.boundary
    assert model.D_Mask_trainer.boundary is None and float(model.boundary.weight_dev.item()) == 0.5
    log = CallLog(monkeypatch)
    hs, ws = _supervised_steps(model, data, B, ref_w)
    h = hs[0]
    # four Segmentor outputs against two distinct targets (m1, m2): two maps, four terms, four gradients, four combines
    assert log.count('mmseg_boundary_map') == 2, log.boundary_calls()
    assert log.count('mmseg_boundary_loss') == log.count('mmseg_boundary_grad_add') == log.count('mmseg_boundary_combine') == 4
    assert 'Segmentor_boundary' in h and np.isfinite(h['Segmentor_boundary'])
    dice_bce = float(log.seg_losses[-1].item())                # what seg_loss wrote for the last Segmentor output, before the combine
    want = dice_bce + 0.5 * h['Segmentor_boundary']
    tol = 2.0 ** -23 * max(abs(dice_bce), abs(0.5 * h['Segmentor_boundary']), abs(want))
    assert abs(h['Segmentor_loss'] - want) <= tol, (h['Segmentor_loss'], dice_bce, h['Segmentor_boundary'])
    assert h['Segmentor_loss'] != hs0[0]['Segmentor_loss']
    assert any(not np.array_equal(a, b) for a, b in zip(ws, ws0)), 'the boundary term did not reach the weights'
    # the unsupervised trainer: both Segmentor outputs train against m1 -> one map
    d = data[0]
    n0 = log.count('mmseg_boundary_map')
    hu = model.unsupervised_trainer.fit([d['x1'], d['x2'], d['z1'], d['z2']], Hh.dafnet_targets(d, False), eps=[d['eps1'], d['eps2']])
    assert log.count('mmseg_boundary_map') == n0 + 1 and 'Segmentor_boundary' in hu.history


@pytest.mark.parametrize('nmod', [2, 3])
def test_mmsdnet_dice_outputs_carry_the_term_one_map_per_modality(backend, monkeypatch, nmod):
    from multimodal_segmentation_amd.configuration import mmsdnet_config_chaos, mmsdnet3_config_chaos
    from multimodal_segmentation_amd.models.mmsdnet import MMSDNet
    from multimodal_segmentation_amd.model_executors.mmsdnet_executor import MMSDNetExecutor
    size = 48 if backend == "cpu" else 64
    np.random.seed(123)
    conf = Hh.make_conf(mmsdnet_config_chaos if nmod == 2 else mmsdnet3_config_chaos, size, batch_size=2, l_mix=1.0, w_boundary=0.25,
                        multi_stream=False)
    model = MMSDNet(conf)
    model.build()
    assert model.supervised_trainer.boundary is not None
    ex = MMSDNetExecutor(conf, model)
    ex.init_train_data(slices_per_volume=2)
    losses = {n: [] for n in ex.get_loss_names() + ['boundary']}
    log = CallLog(monkeypatch)
    ex.train_batch(losses)
    n_seg = sum(1 for s in model.supervised_trainer.specs if s.name == 'Segmentor')
    assert log.count('mmseg_boundary_map') == nmod, 'one map per distinct target (one per modality)'
    assert log.count('mmseg_boundary_loss') == n_seg == nmod + 2 * nmod * (nmod - 1)
    assert len(losses['boundary']) == 1 and np.isfinite(float(losses['boundary'][0]))


def test_ramp_and_validation():
    from multimodal_segmentation_amd import boundary as Bd
    assert Bd.parse_conf({}) is None and Bd.parse_conf({'w_boundary': 0}) is None and Bd.parse_conf({'w_boundary': 0.0, 'boundary_ramp_epochs': 0}) is None
    assert Bd.parse_conf({'w_boundary': 0.5}) == (0.5, 0) and Bd.parse_conf({'w_boundary': 2, 'boundary_ramp_epochs': 4}) == (2.0, 4)
    for bad in [{'w_boundary': -0.1}, {'w_boundary': float('nan')}, {'w_boundary': float('inf')}, {'w_boundary': 'big'},
                {'boundary_ramp_epochs': 4}, {'w_boundary': 0, 'boundary_ramp_epochs': 2}, {'w_boundary': 0.5, 'boundary_ramp_epochs': -1},
                {'w_boundary': 0.5, 'boundary_ramp_epochs': 2.5}, {'w_boundary': True}]:
        with pytest.raises(ValueError):
            Bd.parse_conf(bad)
    w = 0.8
    bw = Bd.BoundaryWeight('cpu', w, 4)
    buf = bw.weight_dev
    got = []
    for e in range(5):
        bw.set_epoch(e)
        got.append(float(bw.weight_dev.item()))
    assert bw.weight_dev is buf, 'set() must write into the one buffer the recorded kernels read'
    assert got == [float(np.float32(v)) for v in (w / 4, w / 2, 3 * w / 4, w, w)]
    flat = Bd.BoundaryWeight('cpu', w, 0)
    assert float(flat.weight_dev.item()) == float(np.float32(w))
    flat.set(0.125)
    assert float(flat.weight_dev.item()) == 0.125 and flat.value == 0.125


def test_invalid_values_raise_when_the_model_is_built_and_the_executor_sets_the_epoch(backend):
    from multimodal_segmentation_amd.configuration import dafnet_config_chaos
    from multimodal_segmentation_amd.models.dafnet import DAFNet
    for bad in (dict(w_boundary=-1.0), dict(boundary_ramp_epochs=3), dict(w_boundary=float('nan'))):
        with pytest.raises(ValueError):
            DAFNet(Hh.make_conf(dafnet_config_chaos, 48, **bad)).build()
    conf, model = _dafnet(48, w_boundary=0.4, boundary_ramp_epochs=4)
    assert float(model.boundary.weight_dev.item()) == float(np.float32(0.1))         # epoch 0
    for e, want in enumerate((0.1, 0.2, 0.4 * 3 / 4, 0.4, 0.4)):
        model.set_boundary_epoch(e)
        assert float(model.boundary.weight_dev.item()) == float(np.float32(want))


def test_command_line_overrides_the_configuration(tmp_path, monkeypatch):
    from multimodal_segmentation_amd.experiment import Experiment, parse_arguments
    monkeypatch.chdir(tmp_path)
    args = parse_arguments(['--config', 'dafnet_config_chaos', '--split', '0', '--w_boundary', '0.1', '--boundary_ramp_epochs', '2'])
    assert args.w_boundary == 0.1 and args.boundary_ramp_epochs == 2
    conf = Experiment().get_config(0, args)
    assert conf.w_boundary == 0.1 and conf.boundary_ramp_epochs == 2
    plain = Experiment().get_config(0, parse_arguments(['--config', 'dafnet_config_chaos', '--split', '0']))
    assert 'w_boundary' not in plain and 'boundary_ramp_epochs' not in plain


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
        conf, model = _dafnet(size, hip_graphs=mode, w_boundary=0.5, boundary_ramp_epochs=2)
        if ref_w is None:
            ref_w = [m.get_weights() for m in _gen_models(model)]
        assert model.supervised_trainer.use_graph == mode and float(model.boundary.weight_dev.item()) == 0.25

        def after(i, model=model):
            if i == 3:
                model.set_boundary_epoch(1)
        runs[mode] = _supervised_steps(model, data, B, ref_w, eps=False, after=after)
        assert float(model.boundary.weight_dev.item()) == 0.5
        if mode:
            g = model.supervised_trainer._graphs
            assert len(g) == 1 and list(g.values())[0].graph is not None, 'the step was not recorded'
    (h0, w0), (h1, w1) = runs[False], runs[True]
    assert all('Segmentor_boundary' in h for h in h1)
    assert h0 == h1, 'losses differ between the eager and the replayed steps'
    for a, b in zip(w0, w1):
        assert np.array_equal(a, b)
    # and the change is visible at all: step 5 with the weight left at w/2 gives another loss
    conf, model = _dafnet(size, hip_graphs=True, w_boundary=0.5, boundary_ramp_epochs=2)
    h2, _ = _supervised_steps(model, data, B, ref_w, eps=False)
    assert h2[3] == h1[3] and h2[4]['Segmentor_loss'] != h1[4]['Segmentor_loss']


@gpu
def test_fp16_with_the_dynamic_loss_scale_runs_a_step_without_a_skip():
    from multimodal_segmentation_amd import nn, ops as P
    nn.set_default_device('cuda:0')
    try:
        conf, model = _dafnet(64, compute_dtype='fp16', loss_scale='dynamic', w_boundary=0.5)
        d = Hh.make_step_data(2, 64, 64, seed=70)
        h = model.supervised_trainer.fit([d['x1'], d['x2'], d['z1'], d['z2']], _targets(d, 2), eps=[d['eps1'], d['eps2']])
        vals = {k: h.history[k][0] for k in h.history.keys()}
        assert all(np.isfinite(v) for v in vals.values()), vals
        assert 'Segmentor_boundary' in vals
        sc = model.supervised_trainer.scaler
        assert sc is not None and sc.skipped_steps() == 0 and sc.iterations() == 1
    finally:
        P.set_conv_precision('fp32')
        P.set_activation_storage(False)


@gpu
def test_experiment_with_the_boundary_loss_runs_end_to_end(tmp_path, monkeypatch):
    from multimodal_segmentation_amd import nn
    from multimodal_segmentation_amd.configuration import _chaos
    from multimodal_segmentation_amd.experiment import Experiment
    nn.set_default_device('cuda:0')
    monkeypatch.chdir(tmp_path)
    real = _chaos.assemble

    def tiny(*a, **k):
        p = real(*a, **k)
        shp = (64, 64, 1)
        p.update(input_shape=shp, epochs=1, batch_size=4, slices_per_volume=2)
        p['anatomy_encoder'].update(input_shape=shp, output_shape=(64, 64, 8))
        p['d_mask_params']['input_shape'] = (64, 64, 4)
        p['d_image_params']['input_shape'] = shp
        return p
    monkeypatch.setattr(_chaos, 'assemble', tiny)
    Experiment().run(['--config', 'dafnet_config_chaos', '--split', '0', '--w_boundary', '0.1', '--boundary_ramp_epochs', '2'])
    folder = "dafnet_chaos_l1_['t1', 't2']_split0"
    rows = open(os.path.join(folder, 'training.csv')).read().strip().split('\n')
    head = rows[0].split(',')
    assert head[-1] == 'boundary' and len(rows) == 2
    assert np.isfinite(float(rows[1].split(',')[-1]))
    assert 'boundary Loss = ' in open(os.path.join(folder, 'logfile.log')).read()
    import json
    dumped = json.load(open(os.path.join(folder, 'experiment_configuration.json')))
    assert dumped['w_boundary'] == 0.1 and dumped['boundary_ramp_epochs'] == 2
    shutil.rmtree(folder, ignore_errors=True)
