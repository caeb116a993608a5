"""The 16-bit storage kernels of csrc/act16.hip (BatchNorm, 2x2 max pooling, the up-sampling gradient, the activation gradient with
its bias gradient, the typed column sums and the 8-channel im2col) where their launch arithmetic changes.

Continues tests/test_act16.py (one shape per kernel, compared with the fp32-storage kernel only) with the conventions of
tests/test_ops_edges.py: the id or the comment of a case gives the arithmetic it exercises, recomputed from the launchers:

  csrc/act16.hip  rows16(M, C) = min(512, 1024 / (C / 64), ceil(M / 64)) row blocks of rpb = ceil(M / blocks) rows, grid (row blocks,
                  C / 64), 16 float4 column lanes x 16 row lanes (bn16_partial_kernel, act16_bwd_kernel, colsum16_partial_kernel; the
                  same function as v4_row_blocks of csrc/norm.hip).  Blocks with r0 = blockIdx.x * rpb >= M run an empty row loop and
                  write zero partials, which the final kernels sum.  grid16(n) = min(4096, ceil(n / 256)) blocks of 256, so a
                  grid-stride loop wraps above 1 048 576 work items of four elements (bn16_apply_kernel, bn16_bwd_apply_kernel,
                  maxpool16_*_kernel, upsample16_bwd_kernel, act16_bwd_flat_kernel; im2col8_kernel: items of one (pixel, tap) pair,
                  12 per pixel).  colsum16_final_kernel: one block of 256 threads per channel walks the row blocks, a second trip
                  above 256 row blocks.  reduce_partials_64 (csrc/common.hpp): 16 lanes per channel walk the row blocks.

Inputs are random fp32 tensors rounded to the 16-bit type (bf16 / fp16: the `mode` fixture), so they are exactly representable.
Every check has two legs:
  1. independent reference: the fp64 oracle (oracle.ops, or the same formula in fp64 torch) on the widened inputs, against the fp32
     outputs of the typed kernels and against the fp32-storage kernel at the same shape, RTOL = 5e-4 of the tensor's largest
     magnitude (the value of _batchnorm_train_case and the InstanceNorm cases of tests/test_ops_parity.py);
  2. storage: a 16-bit output is bit for bit `.to(mode)` of the fp32-storage kernel's output, an fp32 output bit for bit the same
     (what tests/test_act16.py asserts at its one shape).
Pooling, the routing of the pooling gradient and im2col move or select data: exact (`torch.equal`) against the reference after the
single rounding.  Output buffers start as NaN, so an element that a kernel does not write fails; dgamma / dbeta / bias-gradient
buffers start from gbuf_pattern with accumulate = 1 and from NaN with accumulate = 0.

Where the code differs from the plan these cases were drawn up from:
  * mmseg_colsum (csrc/pointwise.hip) ends in colsum_fold_final_kernel (wave shuffles), mmseg_colsum_t in colsum16_final_kernel (an LDS
    tree): another association of the same partials, so the two are NOT bit for bit equal by construction.  The fp32-storage kernel of
    the storage leg is therefore mmseg_colsum_t / mmseg_act_bwd_bias_t with element code 0 on the widened tensor (bit for bit);
    mmseg_colsum is compared at the neighbour's bound (1e-5, test_spade_gamma_beta_tensor_in_16_bits).
  * the up-sampling gradient adds four terms: its fp32 output is compared with the fp64 sum at RTOL, and bit for bit with the fp32
    left-to-right sum in plain torch (the kernel's order); only its 16-bit output is a rounding of that.
The grid-wrap cases of pooling and up-sampling (34 MB in 16 bits, 68 MB widened) run in bf16 only, once per kernel; their reference is
plain fp32 torch on the widened tensor, bit for bit, as in test_maxpool2_grid_wrap.  The BatchNorm, activation-gradient and im2col wrap
cases (<= 17 MB) run in both modes.

Tolerances:
  case                          | tolerance | differs from the neighbour
  ------------------------------+-----------+---------------------------
  (none)                        |           | no case needed another tolerance
"""
import functools

import pytest
import torch

from oracle import ops as O
from multimodal_segmentation_amd import _native as N
from tests.test_act16 import DEV, mode, rnd  # noqa: F401 (mode: fixture)
from tests.test_ops_edges import _plant_ties
from tests.test_ops_parity import _close, gbuf_pattern

pytestmark = pytest.mark.gpu
RTOL = 5e-4
NAN = float('nan')
ALPHA = 0.2


def _hc(mode, on=True):
    """element code of the `_t` entry points: 0 fp32, 1 bf16, 2 fp16"""
    return (1 if mode == torch.bfloat16 else 2) if on else 0


def _nan(shape, dtype=torch.float32):
    return torch.full(tuple(shape), NAN, device=DEV, dtype=dtype)


def _pat(C):
    return gbuf_pattern(torch.empty(C)).to(DEV)


# ======================================================================================================================
# BatchNorm
# ======================================================================================================================
# M, C, shifted (mean 50, sd 0.5)
BN_CASES = [
    pytest.param(1311, 64, False, id='M1311-21-blocks-of-63-last-51'),           # min(512, ceil(1311 / 64)) = 21 blocks, rpb = 63
    pytest.param(65, 64, False, id='M65-two-blocks-33+32'),
    pytest.param(9, 64, False, id='M9-fewer-rows-than-lanes'),                   # one block, 9 rows for 16 row lanes
    pytest.param(1, 64, False, id='M1-variance-0'),                              # dx exactly 0, moving variance takes the M = 1 branch
    pytest.param(512, 192, False, id='C192-three-column-blocks'),                # blockIdx.y = 0..2, 8 blocks of 64 rows
    # 1 x 145 x 113 pixels: min(512, 1024 / 4, 257) = 256 blocks, rpb = ceil(16385 / 256) = 65: blocks 0..251 full, block 252 holds 5
    # rows, blocks 253..255 are EMPTY (r0 >= M).  n4 = 16385 * 64 = 1 048 640 > 4096 * 256: the apply kernels wrap by 64 items
    pytest.param(16385, 256, False, id='M16385-C256-rpb65-3-empty-blocks-apply-wraps-by-64'),
    pytest.param(1311, 64, True, id='M1311-mean50-sd0.5-shifted-sums'),          # the shift x[0][c] is read through ld1<HX> / ld4<HX>
]


@functools.lru_cache(maxsize=4)
def _bn_case(M, C, shifted, mode, relu):
    """inputs (fp32, representable in `mode`) and the fp64 oracle's results of one case; shared by the (hx, hy) pairs, never written"""
    x = (rnd(M, C, seed=21) * (0.5 if shifted else 1.5) + (50.0 if shifted else 0.3)).to(mode).float()
    gamma, beta = rnd(C, seed=22) * 0.2 + 1, rnd(C, seed=23) * 0.1
    mm0, mv0 = rnd(C, seed=24) * 0.1, torch.rand(C, generator=torch.Generator().manual_seed(9)) + 0.5
    dy = rnd(M, C, seed=25).to(mode).float()
    xr, gr, br = x.double().requires_grad_(True), gamma.double().requires_grad_(True), beta.double().requires_grad_(True)
    Pd = {'n/gamma': gr, 'n/beta': br, 'n/moving_mean': mm0.double(), 'n/moving_variance': mv0.double()}
    upd = []
    y = O.batchnorm(xr.reshape(1, 1, M, C), Pd, 'n', True, upd).reshape(M, C)
    O.apply_bn_updates(Pd, upd)
    if relu:       # no cotangent where the kink could flip between fp32 and fp64 (as tests.test_ops_parity.check does)
        dy = dy * (y.detach().abs() > 1e-4).float()
    (torch.relu(y) if relu else y).backward(dy.double())
    mean, var = x.double().mean(0), x.double().var(0, unbiased=False)
    invstd = torch.rsqrt(var + O.BN_EPS)
    scale = gamma.double() * invstd
    return dict(x=x, gamma=gamma, beta=beta, mm0=mm0, mv0=mv0, dy=dy, mean=mean, invstd=invstd, scale=scale,
                shift=beta.double() - mean * scale, mm=Pd['n/moving_mean'].detach(), mv=Pd['n/moving_variance'].detach(),
                y=(torch.relu(y) if relu else y).detach(), dx=xr.grad, dgamma=gr.grad, dbeta=br.grad)


@pytest.mark.parametrize('hx,hy', [(0, 1), (1, 1), (1, 0)])
@pytest.mark.parametrize('relu', [1, 0])
@pytest.mark.parametrize('M,C,shifted', BN_CASES)
def test_batchnorm_typed_boundaries(M, C, shifted, relu, hx, hy, mode):
    """mmseg_bn_stats_t / mmseg_bn_apply_t / mmseg_bn_bwd_t (x, dx stored with code hx; y, dy with code hy) against mmseg_bn_stats /
    mmseg_bn_apply / mmseg_bn_bwd on the widened tensors (bit for bit) and against the fp64 oracle (RTOL)"""
    ref = _bn_case(M, C, shifted, mode, relu)
    tx, ty = (mode if hx else torch.float32), (mode if hy else torch.float32)
    x = ref['x'].to(DEV)
    xin = x.to(tx)
    gamma, beta = ref['gamma'].to(DEV), ref['beta'].to(DEV)
    wsn = torch.empty(N.call('mmseg_norm_workspace_floats', C), device=DEV)
    eps, mom = float(O.BN_EPS), float(O.BN_MOMENTUM)
    # ---- statistics
    st_ref, st = _nan((4, C)), _nan((4, C))
    mm, mv = ref['mm0'].to(DEV), ref['mv0'].to(DEV)
    mm2, mv2 = mm.clone(), mv.clone()
    N.call('mmseg_bn_stats', x, gamma, beta, st_ref[0], st_ref[1], st_ref[2], st_ref[3], mm, mv, wsn, M, C, eps, mom)
    N.call('mmseg_bn_stats_t', xin, gamma, beta, st[0], st[1], st[2], st[3], mm2, mv2, wsn, M, C, eps, mom, _hc(mode, hx))
    assert torch.equal(st, st_ref), 'mean / invstd / scale / shift'
    assert torch.equal(mm2, mm) and torch.equal(mv2, mv), 'moving statistics'
    for k, name in enumerate(('mean', 'invstd', 'scale', 'shift')):
        _close(st[k], ref[name], name, RTOL)
    _close(mm2, ref['mm'], 'moving_mean', RTOL)
    _close(mv2, ref['mv'], 'moving_variance', RTOL)
    if M == 1:
        assert torch.equal(st[0], x[0]), 'the mean of one row is the row (shift + 0)'
        # var + eps = 1 / invstd^2: rsqrtf is good to 2 ulp -> 5e-10 absolute here; a variance from cancellation would be >= 1e-7 * x^2
        assert float((1.0 / st[1].double() ** 2 - eps).abs().max()) <= 1e-9, 'batch variance of one row is exactly 0'
    # ---- normalisation
    y_ref, y = _nan((M, C)), _nan((M, C), ty)
    N.call('mmseg_bn_apply', x, st[2], st[3], y_ref, M, C, relu)
    N.call('mmseg_bn_apply_t', xin, st[2], st[3], y, M, C, relu, _hc(mode, hx), _hc(mode, hy))
    assert torch.equal(y, y_ref.to(ty)), 'y'
    _close(y_ref, ref['y'], 'y (fp32 storage)', RTOL)
    # ---- backward: what it sees as y is the (possibly rounded) stored output
    dy = ref['dy'].to(DEV)
    yq = y.float()
    for acc in (1, 0):
        fill = (lambda: _pat(C)) if acc else (lambda: _nan((C,)))
        dx_ref, dg_ref, db_ref, coef_ref = _nan((M, C)), fill(), fill(), _nan((3 * C,))
        N.call('mmseg_bn_bwd', dy, yq, x, gamma, st[0], st[1], dx_ref, dg_ref, db_ref, coef_ref, wsn, M, C, relu, acc)
        dx, dg, db, coef = _nan((M, C), tx), fill(), fill(), _nan((3 * C,))
        N.call('mmseg_bn_bwd_t', dy.to(ty), y, xin, gamma, st[0], st[1], dx, dg, db, coef, wsn, M, C, relu, acc, _hc(mode, hx), _hc(mode, hy))
        assert torch.equal(dg, dg_ref) and torch.equal(db, db_ref), 'dgamma / dbeta (accumulate = %d)' % acc
        assert torch.equal(dx, dx_ref.to(tx)), 'dx (accumulate = %d)' % acc
        off = _pat(C) if acc else 0.0
        _close(dg - off, ref['dgamma'], 'dgamma (accumulate = %d)' % acc, RTOL)
        _close(db - off, ref['dbeta'], 'dbeta (accumulate = %d)' % acc, RTOL)
        _close(dx_ref, ref['dx'], 'dx (fp32 storage)', RTOL)
        if M == 1:
            assert torch.count_nonzero(dx.float()) == 0, 'dx of a one-row batch is exactly 0'


def test_batchnorm_typed_rejects_what_its_kernels_cannot_index(mode):
    h, other = _hc(mode), 3 - _hc(mode)
    M = 8
    z = lambda C, dt=torch.float32: torch.zeros(M, C, device=DEV, dtype=dt)
    v = lambda C: torch.ones(C, device=DEV)
    ws = torch.empty(N.call('mmseg_norm_workspace_floats', 96), device=DEV)
    stats = lambda C, hx: N.call('mmseg_bn_stats_t', z(C, mode if hx else torch.float32), v(C), v(C), v(C), v(C), v(C), v(C), None, None, ws,
                                 M, C, 1e-3, 0.99, hx)
    bwd = lambda C, hx, hy: N.call('mmseg_bn_bwd_t', z(C, mode), z(C, mode), z(C, mode), v(C), v(C), v(C), z(C, mode), v(C), v(C), v(3 * C), ws,
                                   M, C, 1, 1, hx, hy)
    apply = lambda C, hx, hy: N.call('mmseg_bn_apply_t', z(C, mode), v(C), v(C), z(C, mode), M, C, 1, hx, hy)
    stats(64, h), bwd(64, h, h), apply(4, h, h)                                   # (the accepted neighbours of what follows)
    for bad in (lambda: stats(96, h), lambda: bwd(96, h, h),                      # C % 64 != 0: the column lanes cover 64 channels
                lambda: apply(6, h, h),                                           # C % 4 != 0
                lambda: stats(64, 3), lambda: bwd(64, 3, h), lambda: apply(64, 3, h), lambda: apply(64, h, 3),      # no such element code
                lambda: bwd(64, h, other), lambda: apply(64, h, other), lambda: apply(64, 1, 2)):   # both 16-bit types in one call
        with pytest.raises(N.NativeLibraryError):
            bad()


# ======================================================================================================================
# 2x2 max pooling, gradient of nearest x2 up-sampling
# ======================================================================================================================
POOL_SHAPES = [
    pytest.param(1, 2, 2, 4, id='one-work-item'),
    pytest.param(3, 6, 10, 4, id='C4-1-45-windows'),
    pytest.param(2, 14, 18, 132, id='C4-33-4158-quads-17-blocks-last-62'),       # 2 * 7 * 9 * 33 = 4158 = 16 * 256 + 62
]


def _pool_ref(x, dy):
    """plain torch: pooled values and the routed gradient (first maximum in row-major window order), both exact in any precision"""
    xr = x.clone().requires_grad_(True)
    yr = O.maxpool2(xr)
    (g,) = torch.autograd.grad(yr, xr, dy)
    return yr.detach(), g


def _first_max_routing(x, dy):
    """the tie rule itself, from the definition: per window and channel the cotangent at the first maximum, exactly 0 behind it"""
    B, H, W, C = x.shape
    xw = x.reshape(B, H // 2, 2, W // 2, 2, C).permute(0, 1, 3, 5, 2, 4).reshape(-1, 4)
    first = (xw == xw.amax(1, keepdim=True)).to(torch.float32).argmax(1)
    gw = torch.nn.functional.one_hot(first, 4).to(dy.dtype) * dy.reshape(-1, 1)
    return gw.reshape(B, H // 2, W // 2, C, 2, 2).permute(0, 1, 4, 2, 5, 3).reshape(B, H, W, C)


@pytest.mark.parametrize('ties', ['none', '00', '01', '10', '11', 'all'])
@pytest.mark.parametrize('B,H,W,C', POOL_SHAPES)
def test_maxpool2_typed_boundaries(B, H, W, C, ties, mode):
    """mmseg_maxpool2_fwd_t / _bwd_t / _bwd_add_t with 16-bit tensors and with element code 0.  Rounding to 16 bits makes natural ties
    frequent; planted ties cover every window position"""
    h = _hc(mode)
    x = _plant_ties(rnd(B, H, W, C, seed=45).to(mode).float(), ties)
    dy = rnd(B, H // 2, W // 2, C, seed=46).to(mode).float()
    add = rnd(B, H, W, C, seed=47).to(mode).float()
    y_want, g_want = _pool_ref(x.double(), dy.double())
    assert torch.equal(g_want, _first_max_routing(x.double(), dy.double())), 'the reference follows the first-maximum rule'
    y_want, g_want = y_want.float(), g_want.float()                              # moved values: exact
    xd, dyd, addd = x.to(DEV), dy.to(DEV), add.to(DEV)
    x16, dy16, add16 = xd.to(mode), dyd.to(mode), addd.to(mode)
    # forward
    p_ref, p = _nan(y_want.shape), _nan(y_want.shape, mode)
    N.call('mmseg_maxpool2_fwd', xd, p_ref, B, H, W, C)
    N.call('mmseg_maxpool2_fwd_t', x16, p, B, H, W, C, h)
    assert torch.equal(p, p_ref.to(mode))
    assert torch.equal(p_ref.cpu(), y_want) and torch.equal(p.float().cpu(), y_want)
    p0 = _nan(y_want.shape)
    N.call('mmseg_maxpool2_fwd_t', xd, p0, B, H, W, C, 0)
    assert torch.equal(p0, p_ref)
    # gradient
    g_ref, g = _nan(x.shape), _nan(x.shape, mode)
    N.call('mmseg_maxpool2_bwd', xd, p_ref, dyd, g_ref, B, H, W, C)
    N.call('mmseg_maxpool2_bwd_t', x16, p, dy16, g, B, H, W, C, h)
    assert torch.equal(g, g_ref.to(mode))
    assert torch.equal(g_ref.cpu(), g_want) and torch.equal(g.float().cpu(), g_want)
    # gradient + the skip connection's gradient: `add` lands on all four window positions, rounded once
    for with_add in (False, True):
        want = g_want + add if with_add else g_want                              # one fp32 addition, as in the kernel
        g0, g1 = _nan(x.shape), _nan(x.shape, mode)
        N.call('mmseg_maxpool2_bwd_add_t', xd, p_ref, dyd, addd if with_add else None, g0, B, H, W, C, 0)
        N.call('mmseg_maxpool2_bwd_add_t', x16, p, dy16, add16 if with_add else None, g1, B, H, W, C, h)
        assert torch.equal(g0.cpu(), want), 'h = 0, add = %s' % with_add
        assert torch.equal(g1, g0.to(mode)) and torch.equal(g1.cpu(), want.to(mode)), 'h = %d, add = %s' % (h, with_add)


def test_maxpool2_fp32_code_on_unrounded_input():
    """mmseg_maxpool2_bwd_add_t with element code 0 (the pooling gradient of EVERY configuration) on fp32 values that no 16-bit type
    holds: planted ties at every position in turn, with and without `add`"""
    B, H, W, C = 2, 14, 18, 132
    for ties in ('none', '00', '01', '10', '11', 'all'):
        x = _plant_ties(rnd(B, H, W, C, seed=48), ties)
        dy, add = rnd(B, H // 2, W // 2, C, seed=49), rnd(B, H, W, C, seed=50)
        y_want, g_want = _pool_ref(x, dy)
        assert torch.equal(g_want, _first_max_routing(x, dy))
        for with_add in (False, True):
            g0 = _nan(x.shape)
            N.call('mmseg_maxpool2_bwd_add_t', x.to(DEV), y_want.to(DEV), dy.to(DEV), add.to(DEV) if with_add else None, g0, B, H, W, C, 0)
            assert torch.equal(g0.cpu(), g_want + add if with_add else g_want), (ties, with_add)


def _upsample2_bwd_torch(dy):
    """2x2 block sums, added left to right in row-major window order (the kernels' order) in dy's precision"""
    B, H2, W2, C = dy.shape
    d = dy.reshape(B, H2 // 2, 2, W2 // 2, 2, C)
    return ((d[:, :, 0, :, 0] + d[:, :, 0, :, 1]) + d[:, :, 1, :, 0]) + d[:, :, 1, :, 1]


@pytest.mark.parametrize('B,H,W,C', POOL_SHAPES)          # the shape of dy; dx is [B, H / 2, W / 2, C]
def test_upsample2_bwd_typed_boundaries(B, H, W, C, mode):
    h = _hc(mode)
    dy = rnd(B, H, W, C, seed=51).to(mode).float()
    want32 = _upsample2_bwd_torch(dy)
    dyd = dy.to(DEV)
    u_ref, u0, u = _nan(want32.shape), _nan(want32.shape), _nan(want32.shape, mode)
    N.call('mmseg_upsample2_bwd', dyd, u_ref, B, H // 2, W // 2, C)
    N.call('mmseg_upsample2_bwd_t', dyd, u0, B, H // 2, W // 2, C, 0)
    N.call('mmseg_upsample2_bwd_t', dyd.to(mode), u, B, H // 2, W // 2, C, h)
    assert torch.equal(u0, u_ref) and torch.equal(u, u_ref.to(mode))
    _close(u_ref, _upsample2_bwd_torch(dy.double()), 'upsample2 grad (fp32 storage)', RTOL)
    assert torch.equal(u_ref.cpu(), want32) and torch.equal(u.cpu(), want32.to(mode))


def test_maxpool2_typed_grid_wrap():
    """(1, 260, 254, 256) in bf16: 130 * 127 * 64 = 1 056 640 quads > 4096 * 256 = 1 048 576: maxpool16_fwd_kernel<1>, maxpool16_bwd_kernel<1>
    (with and without `add`) and maxpool16_bwd_kernel<0> wrap by 8064 items.  Bit for bit against plain fp32 torch on the widened tensor"""
    B, H, W, C = 1, 260, 254, 256
    mode = torch.bfloat16
    x = rnd(B, H, W, C, seed=52).to(mode).float()
    x[0, :4, :4] = 0.0                                                    # ties in the first block
    x[0, -4:, -4:] = 0.0                                                  # ... and among the wrapped work items (the last windows)
    dy = rnd(B, H // 2, W // 2, C, seed=53).to(mode).float()
    add = rnd(B, H, W, C, seed=54).to(mode).float()
    y_want, g_want = _pool_ref(x, dy)
    x16, dy16, add16 = x.to(DEV).to(mode), dy.to(DEV).to(mode), add.to(DEV).to(mode)
    p = _nan(y_want.shape, mode)
    N.call('mmseg_maxpool2_fwd_t', x16, p, B, H, W, C, 1)
    assert torch.equal(p.float().cpu(), y_want)
    g = _nan(x.shape, mode)
    N.call('mmseg_maxpool2_bwd_t', x16, p, dy16, g, B, H, W, C, 1)
    assert torch.equal(g.float().cpu(), g_want)
    g.fill_(NAN)
    N.call('mmseg_maxpool2_bwd_add_t', x16, p, dy16, add16, g, B, H, W, C, 1)
    want = g_want + add
    assert torch.equal(g.cpu(), want.to(mode))
    del g, x16
    g0 = _nan(x.shape)
    N.call('mmseg_maxpool2_bwd_add_t', x.to(DEV), y_want.to(DEV), dy.to(DEV), add.to(DEV), g0, B, H, W, C, 0)
    assert torch.equal(g0.cpu(), want)


def test_upsample2_bwd_typed_grid_wrap():
    """low-res (1, 130, 127, 256): 1 056 640 quads: upsample16_bwd_kernel<1> and <0> wrap.  Bit for bit against the fp32 left-to-right
    sums of plain torch on the widened tensor"""
    B, H, W, C = 1, 130, 127, 256
    mode = torch.bfloat16
    dy = rnd(B, 2 * H, 2 * W, C, seed=55).to(mode).float()
    want = _upsample2_bwd_torch(dy)
    u = _nan(want.shape, mode)
    N.call('mmseg_upsample2_bwd_t', dy.to(DEV).to(mode), u, B, H, W, C, 1)
    assert torch.equal(u.cpu(), want.to(mode))
    u0 = _nan(want.shape)
    N.call('mmseg_upsample2_bwd_t', dy.to(DEV), u0, B, H, W, C, 0)
    assert torch.equal(u0.cpu(), want)


def test_pooling_typed_rejects_what_its_kernels_cannot_index(mode):
    h = _hc(mode)
    z = lambda *s: torch.zeros(*s, device=DEV, dtype=mode)
    for B, H, W, C, hh in [(1, 3, 4, 4, h), (1, 4, 3, 4, h), (1, 4, 4, 6, h), (1, 4, 4, 4, 3)]:       # odd H, odd W, C = 6, h = 3
        x, y = z(B, H, W, C), z(B, max(H // 2, 1), max(W // 2, 1), C)
        with pytest.raises(N.NativeLibraryError):
            N.call('mmseg_maxpool2_fwd_t', x, y, B, H, W, C, hh)
        with pytest.raises(N.NativeLibraryError):
            N.call('mmseg_maxpool2_bwd_t', x, y, y, x, B, H, W, C, hh)
        with pytest.raises(N.NativeLibraryError):
            N.call('mmseg_maxpool2_bwd_add_t', x, y, y, x, x, B, H, W, C, hh)
    for C, hh in [(6, h), (4, 3)]:
        with pytest.raises(N.NativeLibraryError):
            N.call('mmseg_upsample2_bwd_t', z(1, 4, 4, C), z(1, 2, 2, C), 1, 2, 2, C, hh)


# ======================================================================================================================
# activation gradient (+ bias gradient), typed column sums
# ======================================================================================================================
ROW_CASES = [
    # min(512, 1024, ceil(16400 / 64) = 257) = 257 row blocks of 64 rows, the last holds 16; colsum16_final_kernel: thread 0 takes blocks
    # 0 and 256
    pytest.param(16400, 64, id='M16400-257-blocks-last-16-final-second-trip'),
    pytest.param(65, 64, id='M65-two-blocks-33+32'),
    pytest.param(1, 64, id='M1-one-row'),
    # min(512, 1024 / 8, 129) = 128 blocks, rpb = 65: blocks 0..125 full, block 126 holds 3 rows, block 127 is EMPTY
    pytest.param(8193, 512, id='M8193-C512-rpb65-one-empty-block'),
    pytest.param(130, 192, id='M130-C192-3-blocks-44+44+42-three-column-blocks'),
]


def _act_grad64(dy, y, act):
    g = {1: (y > 0).double(), 2: torch.where(y >= 0, torch.ones_like(y), torch.full_like(y, ALPHA)), 3: 1.0 - y * y}[act]
    return dy * g


def _act_inputs(M, C, act, mode):
    y = rnd(M, C, seed=21)
    y = (torch.tanh(y) if act == 3 else y).to(mode).float()
    dy = rnd(M, C, seed=22).to(mode).float()
    return y, dy, _act_grad64(dy.double(), y.double(), act)


@pytest.mark.parametrize('act', [1, 2, 3])
@pytest.mark.parametrize('M,C', ROW_CASES)
def test_act_bwd_bias_typed_row_form(M, C, act, mode):
    """mmseg_act_bwd_bias_t with a bias gradient (act16_bwd_kernel<H, true> + colsum16_final_kernel): dx bit for bit the rounding of the
    fp32 result; the bias gradient sums the STORED (rounded) values: 2e-4 against their fp64 column sums (test_activation_gradient_16bit)"""
    h = _hc(mode)
    y, dy, ref64 = _act_inputs(M, C, act, mode)
    yd, dyd = y.to(DEV), dy.to(DEV)
    ref = _nan((M, C))
    N.call('mmseg_act_bwd', dyd, yd, ref, M * C, act, ALPHA)
    _close(ref, ref64, 'act_bwd (fp32 storage)', RTOL)
    ws = torch.empty(N.call('mmseg_colsum_workspace_floats', M, C), device=DEV)
    # element code 0: the fp32-storage instance of the same kernel
    dx0, bg0 = _nan((M, C)), _nan((C,))
    N.call('mmseg_act_bwd_bias_t', dyd, yd, dx0, bg0, ws, M, C, act, ALPHA, 0, 0)
    _close(dx0, ref64, 'dx (h = 0)', RTOL)
    _close(bg0, ref64.sum(0), 'bias gradient (h = 0)', RTOL)
    stored = ref.to(mode).double().sum(0).cpu()
    for acc in (1, 0):
        dx = _nan((M, C), mode)
        bg = _pat(C) if acc else _nan((C,))
        N.call('mmseg_act_bwd_bias_t', dyd.to(mode), yd.to(mode), dx, bg, ws, M, C, act, ALPHA, acc, h)
        assert torch.equal(dx, ref.to(mode)) and torch.equal(dx, dx0.to(mode)), 'accumulate = %d' % acc
        want = stored + (_pat(C).double().cpu() if acc else 0.0)
        assert (bg.double().cpu() - want).abs().max() <= 2e-4 * max(1.0, float(want.abs().max())), 'accumulate = %d' % acc


@pytest.mark.parametrize('M,C', ROW_CASES)
def test_colsum_typed_boundaries(M, C, mode):
    """mmseg_colsum_t: 16-bit loads against element code 0 on the widened tensor (bit for bit), the fp64 column sums (RTOL) and mmseg_colsum
    (another final kernel: the neighbour's 1e-5)"""
    h = _hc(mode)
    x = rnd(M, C, seed=23).to(mode).float()
    xd = x.to(DEV)
    ws = torch.empty(N.call('mmseg_colsum_workspace_floats', M, C), device=DEV)
    want = x.double().sum(0)
    for acc in (1, 0):
        o16, o0, o32 = (_pat(C) if acc else _nan((C,)) for _ in range(3))
        N.call('mmseg_colsum_t', xd.to(mode), o16, ws, M, C, acc, h)
        N.call('mmseg_colsum_t', xd, o0, ws, M, C, acc, 0)
        N.call('mmseg_colsum', xd, o32, ws, M, C, 1.0, acc)
        assert torch.equal(o16, o0), 'accumulate = %d' % acc
        off = _pat(C) if acc else 0.0
        _close(o16 - off, want, 'column sums (accumulate = %d)' % acc, RTOL)
        _close(o32 - off, want, 'column sums (fp32 storage, accumulate = %d)' % acc, RTOL)
        assert (o16 - o32).abs().max() <= 1e-5 * max(1.0, float(o32.abs().max()))


@pytest.mark.parametrize('M,C,act', [
    pytest.param(1, 4, 1, id='n4-one-item-relu'), pytest.param(1, 4, 2, id='n4-one-item-leaky'), pytest.param(1, 4, 3, id='n4-one-item-tanh'),
    pytest.param(7, 12, 1, id='7x12-21-items-relu'), pytest.param(7, 12, 2, id='7x12-21-items-leaky'), pytest.param(7, 12, 3, id='7x12-21-items-tanh'),
    pytest.param(1048577, 4, 2, id='n4-1048577-wraps-by-one-item-leaky'),          # grid16 = 4096 blocks x 256 = 1 048 576 threads
])
def test_act_bwd_typed_flat_form(M, C, act, mode):
    """mmseg_act_bwd_bias_t without a bias gradient (act16_bwd_flat_kernel): any M * C % 4 == 0"""
    h = _hc(mode)
    y, dy, ref64 = _act_inputs(M, C, act, mode)
    yd, dyd = y.to(DEV), dy.to(DEV)
    ref, dx0, dx = _nan((M, C)), _nan((M, C)), _nan((M, C), mode)
    N.call('mmseg_act_bwd', dyd, yd, ref, M * C, act, ALPHA)
    N.call('mmseg_act_bwd_bias_t', dyd, yd, dx0, None, None, M, C, act, ALPHA, 0, 0)
    N.call('mmseg_act_bwd_bias_t', dyd.to(mode), yd.to(mode), dx, None, None, M, C, act, ALPHA, 0, h)
    _close(ref, ref64, 'act_bwd (fp32 storage)', RTOL)
    _close(dx0, ref64, 'dx (h = 0)', RTOL)
    assert torch.equal(dx, ref.to(mode)) and torch.equal(dx, dx0.to(mode))


def test_act_bwd_bias_and_colsum_typed_reject_what_their_kernels_cannot_index(mode):
    h = _hc(mode)
    z = lambda M, C: torch.zeros(M, C, device=DEV, dtype=mode)
    ws = torch.empty(N.call('mmseg_colsum_workspace_floats', 8, 128), device=DEV)
    bg = torch.zeros(128, device=DEV)
    N.call('mmseg_act_bwd_bias_t', z(3, 4), z(3, 4), z(3, 4), None, None, 3, 4, 1, ALPHA, 0, h)           # (accepted: 12 elements)
    N.call('mmseg_act_bwd_bias_t', z(8, 64), z(8, 64), z(8, 64), bg, ws, 8, 64, 1, ALPHA, 0, h)           # (accepted: C = 64 with a workspace)
    for bad in (lambda: N.call('mmseg_act_bwd_bias_t', z(3, 5), z(3, 5), z(3, 5), None, None, 3, 5, 1, ALPHA, 0, h),     # M * C % 4 != 0
                lambda: N.call('mmseg_act_bwd_bias_t', z(8, 96), z(8, 96), z(8, 96), bg, ws, 8, 96, 1, ALPHA, 0, h),     # C % 64 != 0
                lambda: N.call('mmseg_act_bwd_bias_t', z(8, 64), z(8, 64), z(8, 64), bg, None, 8, 64, 1, ALPHA, 0, h),   # no workspace
                lambda: N.call('mmseg_act_bwd_bias_t', z(8, 64), z(8, 64), z(8, 64), bg, ws, 8, 64, 1, ALPHA, 0, 3),     # no such element code
                lambda: N.call('mmseg_colsum_t', z(8, 96), bg, ws, 8, 96, 0, h),
                lambda: N.call('mmseg_colsum_t', z(8, 64), bg, None, 8, 64, 0, h),
                lambda: N.call('mmseg_colsum_t', z(8, 64), bg, ws, 8, 64, 0, 3)):
        with pytest.raises(N.NativeLibraryError):
            bad()


# ======================================================================================================================
# im2col of an 8-channel tensor
# ======================================================================================================================
def _im2col8_ref(x, dtype):
    """rows of 96: columns tap * 8 + c = x[p + delta(tap)][c] for the 9 taps of a 3x3 'same' window (zero outside), 72..95 zero; built
    from explicit shifts of the zero-padded source and rounded once"""
    B, H, W, _ = x.shape
    xp = torch.nn.functional.pad(x, (0, 0, 1, 1, 1, 1))
    cols = [xp[:, kh:kh + H, kw:kw + W, :] for kh in range(3) for kw in range(3)] + [torch.zeros(B, H, W, 24)]
    return torch.cat(cols, -1).reshape(B * H * W, 96).to(dtype)


@pytest.mark.parametrize('x16', [False, True], ids=['fp32-source', '16bit-source'])
@pytest.mark.parametrize('B,H,W', [
    pytest.param(1, 1, 1, id='1x1-every-tap-but-the-centre-outside'),
    pytest.param(2, 1, 5, id='H1-no-row-above-or-below'),
    pytest.param(2, 5, 1, id='W1-no-column-left-or-right'),
    pytest.param(3, 5, 7, id='3x5x7-1260-items-5-blocks-last-236'),
    pytest.param(1, 296, 296, id='296x296-1051392-items-wraps'),                 # 87 616 pixels * 12 > 4096 * 256 = 1 048 576
])
def test_im2col8_typed_boundaries(B, H, W, x16, mode):
    """mmseg_im2col8_t called directly (through a convolution a wrong tap at a border hides inside the bound of a sum of 72 products):
    an fp32 source is rounded once, a 16-bit source is moved"""
    h = _hc(mode)
    x = rnd(B, H, W, 8, seed=61)
    x = x.to(mode).float() if x16 else x
    # the source lies one image row into a buffer of NaN: a tap that wraps to the neighbouring row's pixel instead of reading zero reads
    # NaN at the first and the last pixel as well (and stays inside the allocation)
    buf = _nan(((B * H + 2) * W * 8,), mode if x16 else torch.float32)
    xd = buf[W * 8:(B * H + 1) * W * 8].view(B, H, W, 8)
    xd.copy_(x.to(DEV))
    out = _nan((B * H * W, 96), mode)
    N.call('mmseg_im2col8_t', xd, out, B, H, W, h if x16 else 0, h)
    want = _im2col8_ref(x, mode)
    assert torch.count_nonzero(out[:, 72:].float()) == 0 and not torch.isnan(out.float()).any()
    assert torch.equal(out.cpu(), want)


def test_im2col8_typed_rejects_what_it_does_not_take(mode):
    h, other = _hc(mode), 3 - _hc(mode)
    x32, x16 = torch.zeros(1, 2, 2, 8, device=DEV), torch.zeros(1, 2, 2, 8, device=DEV, dtype=mode)
    out = torch.zeros(4, 96, device=DEV, dtype=mode)
    for bad in (lambda: N.call('mmseg_im2col8_t', x32, torch.zeros(4, 96, device=DEV), 1, 2, 2, 0, 0),       # hy = 0: the output is an MFMA operand
                lambda: N.call('mmseg_im2col8_t', x16, out, 1, 2, 2, other, h),                              # the other 16-bit type
                lambda: N.call('mmseg_im2col8_t', x16, out, 1, 2, 2, 3, h),
                lambda: N.call('mmseg_im2col8_t', x16, out, 0, 2, 2, h, h)):                                 # B = 0
        with pytest.raises(N.NativeLibraryError):
            bad()
