"""Winograd F(2x2,3x3) route of the inference forward (ops.conv2d_bn_infer: Conv2D -> folded BatchNorm [-> ReLU]) of the 3x3 'same' fp32
layers: weight image U = G w G^T, input transform V = B^T d B, sixteen products M[p] = V[p] U[p]^T in one launch of the fast-path body
(family 25: conv_fast_planes_kernel, M tile and N tile in the code), output transform A^T M A with scale, bias and ReLU.

Every case forces mmseg_conv2d_wino_mode 2 (the default admits only deep batch-8 layers of the flagship workload), compares with the fp64
oracle (oracle.ops.conv2d, then scale, bias and ReLU in fp64) at the op-level bar of tests/test_ops_parity.py (RTOL = 2e-4 of the largest
magnitude) and asserts the family id of the launch.  Outputs whose pre-activation lies within 1e-4 of the ReLU kink are masked.

Shapes (B x H x W, C1[+C2] -> Cout), the smallest where each piece can go wrong:
  2x2x4   32 -> 64      every tile touches two borders; T = 4; one ragged M tile
  1x6x10  32+32 -> 96   concat read; ragged N tile (96 = 64 + 32); no ReLU
  3x16x16 64 -> 128     T = 192 = 128 + 64, ragged second M tile; ReLU; a non-trivial oscale and bias
  2x8x8   256 -> 64     K loop of 8 tiles; tile choice below the 384-tile bar
"""
import contextlib
import functools

import numpy as np
import pytest
import torch

from oracle import ops as O
from multimodal_segmentation_amd import ops as P
from multimodal_segmentation_amd import _native as N
from tests.test_ops_parity import _close, rnd

# B, H, W, C1, C2, Cout, relu | kernel code of the route
SHAPES = [
    pytest.param(2, 2, 4, 32, 0, 64, True, 25064064, id='2x2x4-32to64-all-borders'),
    pytest.param(1, 6, 10, 32, 32, 96, False, 25064064, id='1x6x10-32+32to96-concat-ragged-n'),
    pytest.param(3, 16, 16, 64, 0, 128, True, 25064064, id='3x16x16-64to128-ragged-m-relu'),
    pytest.param(2, 8, 8, 256, 0, 64, True, 25064064, id='2x8x8-256to64-k8-below-bar'),
]


@contextlib.contextmanager
def _wino_mode(mode, precision='fp32'):
    prevp = P.set_conv_precision(precision)
    prev = N.call('mmseg_conv2d_wino_mode', mode)
    try:
        yield
    finally:
        N.call('mmseg_conv2d_wino_mode', prev)
        P.set_conv_precision(prevp)


def _last():
    return N.call('mmseg_conv2d_last_kernel')


def _inputs(B, H, W, C1, C2, Cout, wseed=2):
    x1 = torch.relu(rnd(B, H, W, C1, seed=1))                       # post-ReLU activations, as the layers see them
    x2 = torch.relu(rnd(B, H, W, C2, seed=8)) if C2 else None
    w = rnd(3, 3, C1 + C2, Cout, seed=wseed, scale=(2.0 / (9 * (C1 + C2))) ** 0.5)
    cb, gamma, beta = rnd(Cout, seed=4, scale=0.1), torch.rand(Cout, generator=torch.Generator().manual_seed(11)) + 0.5, rnd(Cout, seed=5, scale=0.2)
    mm, mv = rnd(Cout, seed=6, scale=0.3), torch.rand(Cout, generator=torch.Generator().manual_seed(12)) + 0.3
    return x1, x2, w, (cb, gamma, beta, mm, mv)


def _oracle(x1, x2, w, bn, relu, upsample=False):
    """fp64: convolution, then the inference BatchNorm as scale and bias, then ReLU; returns (y, pre-activation)"""
    cb, gamma, beta, mm, mv = [v.double() for v in bn]
    x = x1.double() if x2 is None else torch.cat([x1.double(), x2.double()], dim=3)
    if upsample:
        x = O.upsample2(x)
    conv = O.conv2d(x, w.double(), cb, stride=1, padding='same')
    Pd = {'bn/gamma': gamma, 'bn/beta': beta, 'bn/moving_mean': mm, 'bn/moving_variance': mv}
    pre = O.batchnorm(conv, Pd, 'bn', False)
    return (torch.relu(pre) if relu else pre), pre


@functools.lru_cache(maxsize=None)
def _reference(B, H, W, C1, C2, Cout, relu):
    x1, x2, w, bn = _inputs(B, H, W, C1, C2, Cout)
    return _oracle(x1, x2, w, bn, relu)


def _run(x1, x2, w, bn, relu, upsample=False, wkey=None, dev='cuda'):
    t = lambda v: None if v is None else v.to(dev)
    with torch.no_grad():
        return P.conv2d_bn_infer(t(x1), t(w), *[t(v) for v in bn], relu=relu, x2=t(x2), upsample=upsample, wkey=wkey)


def _close_off_kink(y, y_ref, pre, relu, name):
    keep = (pre.abs() > 1e-4).double() if relu else torch.ones_like(pre)
    _close(y.detach().cpu().double() * keep, y_ref * keep, name)


@pytest.mark.gpu
@pytest.mark.parametrize('B,H,W,C1,C2,Cout,relu,code', SHAPES)
def test_wino_route_against_the_oracle(B, H, W, C1, C2, Cout, relu, code):
    x1, x2, w, bn = _inputs(B, H, W, C1, C2, Cout)
    y_ref, pre = _reference(B, H, W, C1, C2, Cout, relu)
    with _wino_mode(2):
        assert N.call('mmseg_conv2d_wino_ok', B, H, W, C1, C2, Cout) == 1
        y = _run(x1, x2, w, bn, relu)
        assert _last() == code
        err = ((y.cpu().double() - y_ref).abs() * (pre.abs() > 1e-4)).max().item() / y_ref.abs().max().item()
        print('wino %dx%dx%d %d+%d->%d: max err %.3e of the largest magnitude' % (B, H, W, C1, C2, Cout, err))
        _close_off_kink(y, y_ref, pre, relu, 'winograd conv+bn(infer)')


@pytest.mark.gpu
@pytest.mark.parametrize('Cin,Cout', [(32, 64), (64, 96)])
def test_weight_image_is_G_w_Gt(Cin, Cout):
    """mmseg_conv2d_wprep_wino against a numpy construction to 1e-6 of the largest weight (sums of at most nine fp32 values)"""
    G = np.array([[1, 0, 0], [.5, .5, .5], [.5, -.5, .5], [0, 0, 1]], np.float64)
    w = rnd(3, 3, Cin, Cout, seed=2).numpy().astype(np.float64)
    ref = np.einsum('ia,abck,jb->ijkc', G, w, G).reshape(16, Cout, Cin)
    with _wino_mode(2):
        out = torch.full((16 * Cin * Cout,), float('nan'), device='cuda')
        N.call('mmseg_conv2d_wprep_wino', torch.from_numpy(w.astype(np.float32)).cuda(), out, Cin, Cout)
    err = np.abs(out.cpu().numpy().astype(np.float64).reshape(16, Cout, Cin) - ref).max()
    print('wprep_wino: max err %.3e' % err)
    assert err <= 1e-6 * np.abs(w).max()


@pytest.mark.gpu
def test_deterministic_and_rebuilt_after_a_weight_version_bump():
    B, H, W, C1, C2, Cout = 3, 16, 16, 64, 0, 128
    x1, x2, w, bn = _inputs(B, H, W, C1, C2, Cout)
    wkey = ('test_wino_w', 'test_wino_model')
    with _wino_mode(2):
        wd = w.cuda()
        a = _run(x1, x2, wd, bn, True, wkey=wkey)
        assert _last() == 25064064
        b = _run(x1, x2, wd, bn, True, wkey=wkey)
        assert torch.equal(a, b)
        # new weights in the same storage: the cached image is stale until the version moves
        _, _, w2, _ = _inputs(B, H, W, C1, C2, Cout, wseed=9)
        wd.copy_(w2)
        P.bump_weight_version()
        c = _run(x1, x2, wd, bn, True, wkey=wkey)
        assert _last() == 25064064
        y_ref, pre = _oracle(x1, x2, w2, bn, True)
        _close_off_kink(c, y_ref, pre, True, 'after the weight-version bump')
        assert not torch.equal(a, c)


@pytest.mark.gpu
def test_refusals_keep_the_old_route():
    cases = [   # B, H, W, C1, C2, Cout, mode, precision, upsample
        (2, 5, 8, 32, 0, 64, 2, 'fp32', False),       # odd H
        (2, 8, 5, 32, 0, 64, 2, 'fp32', False),       # odd W
        (2, 8, 8, 48, 0, 64, 2, 'fp32', False),       # C1 % 32 != 0
        (2, 8, 8, 32, 0, 48, 2, 'fp32', False),       # Cout % 32 != 0
        (2, 8, 8, 32, 16, 64, 2, 'fp32', False),      # C2 % 32 != 0
        (2, 8, 8, 32, 0, 64, 0, 'fp32', False),       # mode 0
        (2, 4, 4, 32, 0, 64, 2, 'fp32', True),        # up-sampling
    ]
    for B, H, W, C1, C2, Cout, mode, prec, ups in cases:
        x1, x2, w, bn = _inputs(B, H, W, C1, C2, Cout)
        y_ref, pre = _oracle(x1, x2, w, bn, True, upsample=ups)
        with _wino_mode(mode, prec):
            Hc, Wc = (2 * H, 2 * W) if ups else (H, W)
            t = lambda v: None if v is None else v.cuda()
            assert not P._wino_ok(t(x1), t(x2), t(w), ups, torch.float32)
            if not ups:
                assert N.call('mmseg_conv2d_wino_ok', B, Hc, Wc, C1, C2, Cout) == 0
            y = _run(x1, x2, w, bn, True, upsample=ups)
            assert _last() // 1000000 != 25
            _close_off_kink(y, y_ref, pre, True, 'old route %r' % ((B, H, W, C1, C2, Cout, mode, ups),))
    # the 16-bit modes stay on their kernels: the oracle on operands rounded to the 16-bit type, as tests/test_ops_parity.py compares them
    B, H, W, C1, C2, Cout = 2, 8, 8, 32, 0, 64
    x1, x2, w, bn = _inputs(B, H, W, C1, C2, Cout)
    for prec, tdt in (('bf16', torch.bfloat16), ('fp16', torch.float16)):
        y_ref, pre = _oracle(x1.to(tdt).float(), x2, w.to(tdt).float(), bn, True)
        with _wino_mode(2, prec):
            assert N.call('mmseg_conv2d_wino_ok', B, H, W, C1, C2, Cout) == 0
            y = _run(x1, x2, w, bn, True)
            assert _last() // 1000000 != 25
            _close_off_kink(y, y_ref, pre, True, '%s route' % prec)


@pytest.mark.gpu
def test_default_mode_keeps_shapes_outside_the_table_on_their_kernels():
    B, H, W, C1, C2, Cout = 3, 16, 16, 64, 0, 128
    x1, x2, w, bn = _inputs(B, H, W, C1, C2, Cout)
    y_ref, pre = _reference(B, H, W, C1, C2, Cout, True)
    with _wino_mode(1):
        for s in SHAPES:
            assert N.call('mmseg_conv2d_wino_ok', *s.values[:6]) == 0
        y = _run(x1, x2, w, bn, True)
        assert _last() == 1064064
        _close_off_kink(y, y_ref, pre, True, 'default mode, direct launch')
    with _wino_mode(0):
        assert N.call('mmseg_conv2d_wino_ok', 8, 32, 32, 512, 0, 512) == 0
    with _wino_mode(2):
        assert N.call('mmseg_conv2d_wino_ok', 8, 32, 32, 512, 0, 512) == 1


@pytest.mark.gpu
def test_anatomy_encoder_predict_agrees_across_the_rounding_layer():
    """an anatomy encoder at 64 x 64, batch 2, filters as configured, predicted with mode 0 and mode 2: the soft-max agrees within 1e-5, and
    a rounded output may differ only where the mode-0 soft-max is within 1e-5 of 1/2"""
    from multimodal_segmentation_amd import nn
    from multimodal_segmentation_amd.configuration import dafnet_config_chaos
    from multimodal_segmentation_amd.model_components import anatomy_encoder
    from tests import helpers as Hh
    nn.set_default_device('cuda:0')
    H, B = 64, 2
    conf = Hh.make_conf(dafnet_config_chaos, H).anatomy_encoder
    enc = anatomy_encoder.build(conf, 'Enc_Anatomy_wino', rng=np.random.RandomState(7))
    rng = np.random.RandomState(1)
    for p in enc.params.values():
        if 'gamma' in p.name or 'beta' in p.name or 'bias' in p.name or 'moving_mean' in p.name:
            p.data.copy_(torch.from_numpy((p.data.cpu().numpy() + 0.1 * rng.standard_normal(p.shape)).astype(np.float32)).to(p.data.device))
    P.bump_weight_version()              # (also makes the folded BatchNorm parameters stale)
    x = nn.to_device(Hh.smooth_field(rng, B, H, H), enc.device)
    res = {}
    for mode in (0, 2):
        with _wino_mode(mode):
            r = enc.predict(x)
            res[mode] = (enc.last_soft.detach().cpu().double(), r.detach().cpu())
    s0, r0 = res[0]
    s2, r2 = res[2]
    err = (s0 - s2).abs().max().item()
    diff = r0 != r2
    print('encoder soft-max: max difference %.3e; rounded outputs that differ: %d of %d' % (err, int(diff.sum()), diff.numel()))
    assert err <= 1e-5
    assert bool(((s0 - 0.5).abs()[diff] <= 1e-5).all())
