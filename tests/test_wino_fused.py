"""Fused Winograd F(2x2,3x3) route of the inference forward (ops.conv2d_bn_infer(rounded=True): Conv2D -> folded BatchNorm [-> ReLU]) of the
wide 3x3 'same' fp32 layers: ONE launch of winof_kernel (family 26; a block = 8 image rows x 32 columns x 64 output channels, K in chunks
of 16 input channels), weight image U = G w G^T shared with the un-fused route of tests/test_wino.py.

Every case compares with the fp64 oracle (oracle.ops.conv2d, then scale, bias and ReLU in fp64) at the op-level bar of
tests/test_ops_parity.py (RTOL = 2e-4 of the largest magnitude), outputs within 1e-4 of the ReLU kink masked, and prints the fused route's
error next to the un-fused route's on the same inputs.

Shapes (B x H x W, C1[+C2] -> Cout):
  1x8x32  32 -> 64       exactly one block, all four image borders inside it, two K chunks (one 32-channel group)
  2x16x64 32+32 -> 64    2 x 2 blocks per image, two images, the concat boundary at a chunk edge; each image alone gives the same bits
  1x8x64  96 -> 128      six K chunks (an odd number of 32-channel groups), two N blocks; with / without ReLU, with / without scale and bias
  3x8x32  64 -> 96       Cout % 64 != 0: the kernel has no ragged N block, mmseg_conv2d_winof_ok answers 0, the layer keeps its kernel
"""
import numpy as np
import pytest
import torch

from oracle import ops as O
from multimodal_segmentation_amd import ops as P
from multimodal_segmentation_amd import _native as N
from tests.test_wino import _inputs, _oracle, _close_off_kink, _wino_mode, _last

FUSED = 26064064
INVALID = 1          # hipErrorInvalidValue


def _run(x1, x2, w, bn, relu, rounded=True, wkey=None):
    t = lambda v: None if v is None else v.cuda()
    with torch.no_grad():
        return P.conv2d_bn_infer(t(x1), t(w), *[t(v) for v in bn], relu=relu, x2=t(x2), wkey=wkey, rounded=rounded)


def _err(y, y_ref, pre):
    return ((y.cpu().double() - y_ref).abs() * (pre.abs() > 1e-4)).max().item() / y_ref.abs().max().item()


def _fused_and_unfused(shape, relu):
    """the layer through the fused and through the un-fused route (mode 2) -> (fused y, oracle y, oracle pre-activation); prints both errors"""
    x1, x2, w, bn = _inputs(*shape)
    y_ref, pre = _oracle(x1, x2, w, bn, relu)
    with _wino_mode(2):
        assert N.call('mmseg_conv2d_winof_ok', *shape) == 1
        y = _run(x1, x2, w, bn, relu)
        assert _last() == FUSED
        yu = _run(x1, x2, w, bn, relu, rounded=False)
        assert _last() // 1000000 == 25
    print('winof %dx%dx%d %d+%d->%d: max err fused %.3e, un-fused %.3e of the largest magnitude' % (shape + (_err(y, y_ref, pre), _err(yu, y_ref, pre))))
    return y, y_ref, pre


@pytest.mark.gpu
def test_one_block_with_all_four_borders():
    y, y_ref, pre = _fused_and_unfused((1, 8, 32, 32, 0, 64), True)
    _close_off_kink(y, y_ref, pre, True, 'fused winograd, one block')


@pytest.mark.gpu
def test_several_blocks_concat_and_image_boundaries():
    shape = (2, 16, 64, 32, 32, 64)
    y, y_ref, pre = _fused_and_unfused(shape, True)
    _close_off_kink(y, y_ref, pre, True, 'fused winograd, 2 x 2 blocks x 2 images, concat')
    # a block on an image's last (first) rows must not read the next (previous) image: each image alone gives the same bits
    x1, x2, w, bn = _inputs(*shape)
    with _wino_mode(2):
        for b in range(2):
            yb = _run(x1[b:b + 1], x2[b:b + 1], w, bn, True)
            assert _last() == FUSED
            assert torch.equal(yb[0], y[b]), 'image %d alone' % b


@pytest.mark.gpu
@pytest.mark.parametrize('relu', [True, False])
def test_odd_chunk_groups_and_two_n_blocks(relu):
    y, y_ref, pre = _fused_and_unfused((1, 8, 64, 96, 0, 128), relu)
    _close_off_kink(y, y_ref, pre, relu, 'fused winograd, 96 -> 128')


@pytest.mark.gpu
@pytest.mark.parametrize('relu', [True, False])
def test_entry_point_without_scale_and_bias(relu):
    B, H, W, C1, C2, Cout = 1, 8, 64, 96, 0, 128
    x1, _, w, _ = _inputs(B, H, W, C1, C2, Cout)
    pre = O.conv2d(x1.double(), w.double(), None, stride=1, padding='same')
    y_ref = torch.relu(pre) if relu else pre
    with _wino_mode(2):
        xd, wd = x1.cuda(), w.cuda()
        U = torch.empty(16 * C1 * Cout, device='cuda')
        N.call('mmseg_conv2d_wprep_wino', wd, U, C1, Cout)
        y = torch.full((B, H, W, Cout), float('nan'), device='cuda')
        N.call('mmseg_conv2d_fwd_winof', xd, None, U, None, None, y, B, H, W, C1, C2, Cout, 1 if relu else 0, 0.0)
        assert _last() == FUSED
    print('winof entry point, no scale / bias, relu %s: max err %.3e' % (relu, _err(y, y_ref, pre)))
    _close_off_kink(y, y_ref, pre, relu, 'fused winograd without scale and bias')


@pytest.mark.gpu
def test_ragged_output_channels_keep_their_kernel():
    shape = (3, 8, 32, 64, 0, 96)
    x1, x2, w, bn = _inputs(*shape)
    y_ref, pre = _oracle(x1, x2, w, bn, True)
    with _wino_mode(2):
        assert N.call('mmseg_conv2d_winof_ok', *shape) == 0
        y = _run(x1, x2, w, bn, True)
        code = _last()
        assert code // 1000000 != 26
        y0 = _run(x1, x2, w, bn, True, rounded=False)
        assert _last() == code and torch.equal(y, y0)
    _close_off_kink(y, y_ref, pre, True, '64 -> 96 on its old kernel')


@pytest.mark.gpu
def test_deterministic_and_rebuilt_after_a_weight_version_bump():
    shape = (2, 16, 64, 32, 32, 64)
    x1, x2, w, bn = _inputs(*shape)
    wkey = ('test_winof_w', 'test_winof_model')
    with _wino_mode(2):
        wd = w.cuda()
        a = _run(x1, x2, wd, bn, True, wkey=wkey)
        assert _last() == FUSED
        b = _run(x1, x2, wd, bn, True, wkey=wkey)
        assert torch.equal(a, b)
        # new weights in the same storage: the cached image is stale until the version moves
        _, _, w2, _ = _inputs(*shape, wseed=9)
        wd.copy_(w2)
        P.bump_weight_version()
        c = _run(x1, x2, wd, bn, True, wkey=wkey)
        assert _last() == FUSED
        y_ref, pre = _oracle(x1, x2, w2, bn, True)
        _close_off_kink(c, y_ref, pre, True, 'after the weight-version bump')
        assert not torch.equal(a, c)


@pytest.mark.gpu
def test_refusals_launch_nothing():
    """hipErrorInvalidValue before anything is queued: the output keeps its sentinel and the last-kernel code does not move"""
    def attempt(B, H, W, C1, C2, Cout, misalign=False):
        n = B * H * W * C1
        buf = torch.zeros(n + 4, device='cuda')
        x1 = buf[1:1 + n] if misalign else buf[:n]
        x2 = torch.zeros(B * H * W * C2, device='cuda') if C2 else None
        U = torch.zeros(16 * (C1 + C2) * Cout, device='cuda')
        y = torch.full((B * H * W * Cout,), float('nan'), device='cuda')
        before = _last()
        with pytest.raises(N.NativeLibraryError, match='hipError_t %d' % INVALID):
            N.call('mmseg_conv2d_fwd_winof', x1, x2, U, None, None, y, B, H, W, C1, C2, Cout, 1, 0.0)
        torch.cuda.synchronize()
        assert _last() == before and bool(torch.isnan(y).all())

    with _wino_mode(2):
        attempt(1, 9, 32, 32, 0, 64)                     # odd H
        attempt(1, 8, 48, 32, 0, 64)                     # W not a multiple of the block's 32 columns
        attempt(1, 8, 32, 16, 0, 64)                     # C1 = 16
        attempt(1, 8, 32, 32, 16, 64)                    # C2 % 32 != 0
        attempt(1, 8, 32, 32, 0, 96)                     # Cout % 64 != 0
        attempt(1, 8, 32, 32, 0, 64, misalign=True)      # x1 four bytes off a 16-byte boundary
        for shape in ((1, 9, 32, 32, 0, 64), (1, 8, 48, 32, 0, 64), (1, 8, 32, 16, 0, 64), (1, 8, 32, 32, 0, 96)):
            assert N.call('mmseg_conv2d_winof_ok', *shape) == 0
    for prec in ('bf16', 'fp16'):
        with _wino_mode(2, prec):
            assert N.call('mmseg_conv2d_winof_ok', 1, 8, 32, 32, 0, 64) == 0
            attempt(1, 8, 32, 32, 0, 64)


@pytest.mark.gpu
def test_never_without_the_keyword():
    shape = (1, 8, 32, 64, 0, 64)
    x1, x2, w, bn = _inputs(*shape)
    y_ref, pre = _oracle(x1, x2, w, bn, True)
    for mode in (0, 1, 2):
        with _wino_mode(mode):
            y = _run(x1, x2, w, bn, True, rounded=False)
            assert _last() // 1000000 != 26, mode
            _close_off_kink(y, y_ref, pre, True, 'without the keyword, mode %d' % mode)
    with _wino_mode(2):
        y = _run(x1, x2, w, bn, True, rounded=True)
        assert _last() == FUSED
        _close_off_kink(y, y_ref, pre, True, 'with the keyword, mode 2')
    for mode in (0, 1):                                  # (mode 1: one block is far outside the table of profiles/winof_ab.txt)
        with _wino_mode(mode):
            assert N.call('mmseg_conv2d_winof_ok', *shape) == 0
            y = _run(x1, x2, w, bn, True, rounded=True)
            assert _last() // 1000000 != 26, mode
            _close_off_kink(y, y_ref, pre, True, 'with the keyword, mode %d' % mode)


@pytest.mark.gpu
def test_segmentor_predict_never_takes_the_fused_route(monkeypatch):
    """the segmentor's 64 -> 64 layer has the fused route's shape, but its masks feed the mask discriminator unrounded"""
    from multimodal_segmentation_amd import nn
    from multimodal_segmentation_amd.configuration import dafnet_config_chaos
    from multimodal_segmentation_amd.model_components import segmentor
    from tests import helpers as Hh
    nn.set_default_device('cuda:0')
    conf = Hh.make_conf(dafnet_config_chaos, 16, 32)
    seg = segmentor.build(conf, rng=np.random.RandomState(3))
    s = (np.random.RandomState(4).rand(2, 16, 32, conf.anatomy_encoder.output_shape[-1]) > 0.5).astype(np.float32)
    names, families = [], []
    real = N.call

    def counting(name, *args):
        rc = real(name, *args)
        names.append(name)
        if name.startswith('mmseg_conv2d_fwd'):
            families.append(real('mmseg_conv2d_last_kernel') // 1000000)
        return rc
    monkeypatch.setattr(N, 'call', counting)
    with _wino_mode(2):
        assert real('mmseg_conv2d_winof_ok', 2, 16, 32, 64, 0, 64) == 1      # (the shape alone would be admitted)
        out = seg.predict(nn.to_device(s, seg.device))
    assert tuple(out.shape) == (2, 16, 32, conf.num_masks + 1)
    assert len(families) >= 3 and 26 not in families, families
    assert 'mmseg_conv2d_fwd_winof' not in names and 'mmseg_conv2d_winof_ok' not in names


ENCODER_SEED = 4          # (the closest mode-0 soft-max value to 1/2 is 0.12 away; seeds 1, 5 and 10 come within 1e-3)


@pytest.mark.gpu
def test_anatomy_encoder_predict_agrees_across_the_rounding_layer():
    """an anatomy encoder at 64 x 64, batch 2, filters as configured, predicted with mode 0 and mode 2 (where its 64 -> 64, 64+64 -> 64,
    64 -> 128, 128 -> 128 and 128+128 -> 128 layers take the fused kernel): no rounded output flips.  Precondition, asserted: in mode 0
    no soft-max value lies within 1e-5 of 1/2 (the seed is chosen for that), so the test neither passes by luck nor fails on a borderline
    pixel."""
    from multimodal_segmentation_amd import nn
    from multimodal_segmentation_amd.configuration import dafnet_config_chaos
    from multimodal_segmentation_amd.model_components import anatomy_encoder
    from tests import helpers as Hh
    nn.set_default_device('cuda:0')
    H, B = 64, 2
    conf = Hh.make_conf(dafnet_config_chaos, H).anatomy_encoder
    assert conf.rounding
    enc = anatomy_encoder.build(conf, 'Enc_Anatomy_winof', rng=np.random.RandomState(7))
    rng = np.random.RandomState(ENCODER_SEED)
    for p in enc.params.values():
        if 'gamma' in p.name or 'beta' in p.name or 'bias' in p.name or 'moving_mean' in p.name:
            p.data.copy_(torch.from_numpy((p.data.cpu().numpy() + 0.1 * rng.standard_normal(p.shape)).astype(np.float32)).to(p.data.device))
    P.bump_weight_version()              # (also makes the folded BatchNorm parameters stale)
    x = nn.to_device(Hh.smooth_field(rng, B, H, H), enc.device)
    res, fused = {}, {}
    real = N.call
    for mode in (0, 2):
        n = [0]

        def counting(name, *args):
            n[0] += name == 'mmseg_conv2d_fwd_winof'
            return real(name, *args)
        N.call = counting
        try:
            with _wino_mode(mode):
                r = enc.predict(x)
                res[mode] = (enc.last_soft.detach().cpu().double(), r.detach().cpu())
        finally:
            N.call = real
        fused[mode] = n[0]
    assert fused[0] == 0 and fused[2] >= 6, fused
    s0, r0 = res[0]
    s2, r2 = res[2]
    margin = (s0 - 0.5).abs().min().item()
    err = (s0 - s2).abs().max().item()
    diff = r0 != r2
    print('encoder soft-max: %d fused launches; max difference %.3e; closest mode-0 value to 1/2: %.3e; rounded outputs that differ: %d of %d'
          % (fused[2], err, margin, int(diff.sum()), diff.numel()))
    assert margin > 1e-5, 'precondition: choose another ENCODER_SEED'
    assert err <= 1e-5
    assert int(diff.sum()) == 0


def test_winof_ok_is_pure_host_logic():
    """mmseg_conv2d_winof_ok over a grid of shapes and the three modes, without a device: mode 0 never; mode 2 exactly the structural
    conditions; mode 1 a subset of mode 2; the 16-bit precision modes never"""
    N.build()
    lib = N.load()
    ok = lambda *s: lib.mmseg_conv2d_winof_ok(*s)
    structural = lambda B, H, W, C1, C2, Cout: (B >= 1 and H >= 8 and H % 8 == 0 and W >= 32 and W % 32 == 0 and C1 >= 32 and C1 % 32 == 0 and
                                                C2 % 32 == 0 and Cout >= 64 and Cout % 64 == 0)
    grid = [(B, H, W, C1, C2, Cout) for B in (1, 8) for H in (4, 8, 9, 12, 16, 256) for W in (16, 32, 48, 64, 256)
            for C1 in (16, 32, 48, 64, 128) for C2 in (0, 16, 32, 64) for Cout in (32, 64, 96, 128, 256)]
    prev_mode = lib.mmseg_conv2d_wino_mode(-1)
    prev_prec = lib.mmseg_get_conv_precision()
    try:
        lib.mmseg_set_conv_precision(0)
        admitted = {}
        for mode in (0, 1, 2):
            lib.mmseg_conv2d_wino_mode(mode)
            assert lib.mmseg_conv2d_wino_mode(-1) == mode
            admitted[mode] = set(s for s in grid if ok(*s))
            assert all(ok(*s) in (0, 1) for s in grid[:50])
        assert admitted[0] == set()
        assert admitted[2] == set(s for s in grid if structural(*s))
        assert admitted[1] <= admitted[2]
        assert (1, 8, 32, 64, 0, 64) not in admitted[1]                       # one block: far outside the measured table
        # the offset limits: a tensor of 2^31 bytes or more is refused in every mode
        assert ok(64, 1024, 1024, 32, 0, 64) == 0 and ok(1, 1024, 1024, 32, 0, 64) == 1
        assert ok(0, 8, 32, 32, 0, 64) == 0 and ok(1, 8, 32, 32, -32, 64) == 0
        for prec in (1, 2):
            lib.mmseg_set_conv_precision(prec)
            assert not any(ok(*s) for s in grid)
    finally:
        lib.mmseg_set_conv_precision(prev_prec)
        lib.mmseg_conv2d_wino_mode(prev_mode)
