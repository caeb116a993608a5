"""The dense, resampling, pooling, slicing, axpby and spectral-penalty kernels where their launch arithmetic changes.

Continues the boundary tests at the end of tests/test_ops_parity.py with the same conventions: every case runs on the device
(`-m gpu`) and through tests/cpu_backend.py, values and gradients are compared with the fp64 oracle on the same seeded fp32
inputs, and the id or the comment of a case gives the arithmetic it exercises, recomputed from the launchers:

  csrc/dense.hip      forward: ks = min(1024, ceil(K / 128)) K slices of kper = ceil(K / ks) (rounded up to 4 on the 16-byte path,
                      K % 4 == 0), grid (ceil(N / 64), ks), RB = 8 / 16 / 32 rows in registers; N <= 4 and (R <= 16 or N == 1) and
                      K >= 4096: blocks of 1024 k along K.  Data gradient: K <= 16 and N >= 1024 -> one block per row, otherwise
                      ceil(K / 64) blocks that walk N in chunks of 128.  Weight gradient: min(8192, ceil(K * N / 256)) blocks.
                      ops._Dense: row groups of 32.
  csrc/pointwise.hip  grid_for: min(4096, ceil(n / 256)) blocks of 256, so a grid-stride loop wraps above 1 048 576 work items;
                      act_bwd / axpby: float4 body + a scalar tail of n % 4 run by one thread.
  csrc/optim.hip      spectral penalty: 32 K slices of kper = ceil(K / 32), column blocks of 256, one block of 1024 threads
                      normalises, gradient on min(4096, ceil(n / 256)) blocks (2048 in the batched launch).
  csrc/act16.hip      batch plumbing (last section): grid16(n) = min(4096, ceil(n / 256)) blocks of 256, so a grid-stride loop wraps
                      above 1 048 576 work items.  sum_n_kernel: grid16(numel / 4 + 1), groups of four elements + a scalar tail of
                      numel % 4 run by one thread, at most 8 operands per launch (ops._sum_n chains launches).  cat_words_kernel:
                      grid16(words / 4 + 1); per part 16-byte copies + a scalar tail of words % 4 when source AND destination are
                      16-byte aligned, else one 4-byte word per thread; at most 8 parts per launch.  gather_rows_kernel: grid
                      (min(1024, ceil(words / 4 / 256)), min(4096, rows)), 16-byte copies when words % 4 == 0.  add_residual_kernel:
                      grid16(M), one row per thread.

Tolerances: those of the neighbouring tests (RTOL = 2e-4 of the tensor's largest magnitude for values and gradients, 1e-4 / 1e-5
for the spectral loss / gradient), exact equality where an op only moves or selects data (and for the fp32 sums of sum_n_kernel, which
are left-to-right additions that plain torch repeats bit for bit).
  case                          | tolerance | differs from the neighbour
  ------------------------------+-----------+---------------------------
  (none)                        |           | no case needed another tolerance
"""
import functools

import pytest
import torch

from oracle import ops as O
from multimodal_segmentation_amd import ops as P
from tests.test_ops_parity import RTOL, _anchor, _close, _native_error, check, device, gbuf_pattern, rnd  # noqa: F401 (device: fixture)


# ======================================================================================================================
# dense
# ======================================================================================================================
# R, K, N, act.  Every case starts from NON-ZERO gradient buffers (gbuf_pattern): the weight and bias gradients must be added.
DENSE_EDGES = [
    # ---- scalar forward (dense_fwd_partial_kernel: K % 4 != 0 outside the small-N path)
    pytest.param(8, 1001, 100, 'tanh', id='fwd-scalar-ks8-kper126-last119'),        # N = 100: second column block has 36 live lanes
    # RB = 32 with 15 masked rows; ks = 3, kper = 86, last slice 85; N = 65: the second column block has ONE live lane;
    # data gradient: 5 blocks of 64 rows of W, the last holds one row
    pytest.param(17, 257, 65, None, id='fwd-scalar-RB32-15-masked-rows-N65'),
    pytest.param(1, 130, 64, None, id='fwd-scalar-R1-ks2-kper65'),                  # K % 4 = 2; one row in RB = 8
    # ---- the small-N threshold (N <= 4, K >= 4096)
    pytest.param(8, 4095, 1, None, id='K4095-below-smalln-scalar-ks32-kper128-last127'),   # 63 of 64 column lanes dead
    pytest.param(8, 4096, 1, None, id='K4096-smalln-8x1-four-full-blocks-16B'),     # 4 blocks x 256 threads x 4 k = 4096
    pytest.param(8, 4097, 1, None, id='K4097-smalln-8x1-scalar-fifth-block-one-k'),
    pytest.param(3, 4096, 2, None, id='smalln-8x4-N2-two-dummy-columns'),
    pytest.param(8, 4100, 4, 'leaky', id='smalln-8x4-N4-fifth-block-4k'),
    pytest.param(9, 4100, 3, None, id='smalln-16x4-7-masked-rows'),
    # R > 16 and N > 1: not the small-N path.  k4 kernel, RB = 32, ks = 33, kper = ceil(4100 / 33) = 125 -> 128, the last slice holds
    # 4 k; N = 3: 61 dead column lanes
    pytest.param(20, 4100, 3, None, id='R20-N3-not-smalln-k4-ks33-kper128-last4'),
    # ---- capped slices: ceil(K / 128) = 1025 > 1024
    # k4 kernel: kper = ceil(131076 / 1024) = 129 -> 132; 993 * 132 = 131076, so slices 993..1023 are empty and write zeros (W: 4 MB)
    pytest.param(8, 131076, 8, None, id='K131076-k4-ks1024-kper132-slices-993-on-empty'),
    # scalar kernel: kper = 129; slice 1016 holds 131073 - 1016 * 129 = 9 k, slices 1017..1023 are empty (W: 2.6 MB)
    pytest.param(3, 131073, 5, None, id='K131073-scalar-ks1024-kper129-slices-1017-on-empty'),
    # ---- generic data gradient (dense_dgrad_kernel)
    # N chunks of 128, 128, 44; second block holds 36 rows of W; bias gradient: generic column-sum kernel, cw = 256, two passes
    pytest.param(8, 100, 300, None, id='dgrad-chunks-128-128-44-second-block-36-rows'),
    pytest.param(32, 70, 129, 'leaky', id='dgrad-R32-all-8-slots-last-chunk-1'),    # K % 4 = 2: scalar forward; second block 6 rows
    pytest.param(29, 64, 128, None, id='dgrad-R29-one-block-one-full-chunk'),       # slot 7 live in row lane 0 only (b = 28)
    pytest.param(4, 17, 1024, None, id='dgrad-K17-above-smallk-limit-8-chunks'),
    pytest.param(4, 16, 1024, None, id='dgrad-K16-N1024-smallk-exactly'),           # 16 accumulators, 4 full trips over N
    pytest.param(4, 8, 1023, None, id='dgrad-N1023-below-smallk-limit-last-chunk-127'),
    # ---- weight-gradient wrap: K * N = 2 099 200 > 8192 * 256 = 2 097 152, 2048 elements make a second trip
    pytest.param(4, 4100, 512, None, id='wgrad-2099200-wraps'),
    # ---- row groups of ops._Dense (the weight gradient accumulates across the groups)
    pytest.param(33, 64, 10, 'tanh', id='rows-32+1-act-tail-2'),                     # R * N = 330: n % 4 = 2 in act_bwd_kernel
    pytest.param(70, 36, 5, None, id='rows-32+32+6'),
    # ---- scalar tail of act_bwd_kernel (n = R * N, n % 4 != 0)
    pytest.param(3, 40, 7, 'leaky', id='act-tail-n21-rem1'),
    pytest.param(2, 40, 7, 'leaky', id='act-tail-n14-rem2'),
    pytest.param(5, 40, 7, 'tanh', id='act-tail-n35-rem3'),
    pytest.param(1, 40, 3, 'tanh', id='act-tail-n3-tail-only'),
    # ---- bias gradient through mmseg_colsum: N = 300 is neither a multiple of 64 nor a divisor of 64 -> colsum_partial_kernel with
    # cw = 256 channels per pass, the second pass holds 44
    pytest.param(8, 32, 300, None, id='bgrad-colsum-generic-two-passes-44'),
]


@pytest.mark.parametrize('R,K,N,act', DENSE_EDGES)
def test_dense_boundaries(R, K, N, act, device):
    x, w, b = rnd(R, K, seed=12), rnd(K, N, seed=13, scale=K ** -0.5), rnd(N, seed=14, scale=0.1)

    def f_ref(x, w, b):
        y = O.dense(x, w, b)
        f_ref.pre = y if act == 'leaky' else None
        return O.leaky_relu(y, 0.3) if act == 'leaky' else (torch.tanh(y) if act == 'tanh' else y)

    check(lambda x, w, b: P.dense(x, w, b, act, 0.3, wgrad=w.gbuf, bgrad=b.gbuf, anchor=_anchor(x)), f_ref, [x, w, b], device,
          param_idx=(1, 2), gbuf_fill=gbuf_pattern)


@pytest.mark.parametrize('R', [0, 33])
def test_dense_entry_points_reject_row_counts_their_registers_cannot_hold(R, device):
    """mmseg_dense_fwd / _dgrad / _wgrad keep <= 32 rows in registers (and LDS): R = 0 and R = 33 are refused before any launch.
    (ops._Dense never passes them: it walks larger batches in row groups.)"""
    from multimodal_segmentation_amd import _native as N
    K, Nn = 8, 8
    z = lambda *s: torch.zeros(*s, device=device)
    x, w, bias, y, ws = z(33, K), z(K, Nn), z(Nn), z(33, Nn), z(4096)
    with pytest.raises(_native_error()):
        N.call('mmseg_dense_fwd', x, w, bias, y, ws, R, K, Nn, 0, 0.0)
    with pytest.raises(_native_error()):
        N.call('mmseg_dense_dgrad', y, w, x, R, K, Nn)
    with pytest.raises(_native_error()):
        N.call('mmseg_dense_wgrad', x, y, w, R, K, Nn, 1)


# ======================================================================================================================
# nearest resampling
# ======================================================================================================================
@pytest.mark.parametrize('B,H,W,C', [
    pytest.param(2, 5, 7, 4, id='C4-1'),                                  # one float4 per pixel
    pytest.param(3, 9, 6, 12, id='C4-3'),                                 # C4 = 3: the index split is a real division
    pytest.param(1, 130, 129, 64, id='fwd-1073280-quads-wraps'),          # 260 * 258 * 16 = 1 073 280 output quads > 1 048 576
    pytest.param(2, 130, 129, 128, id='bwd-1073280-quads-wraps'),         # 2 * 130 * 129 * 32 = 1 073 280 input quads (forward: 4 trips)
])
def test_upsample2(B, H, W, C, device):
    """ops.upsample2 (upsample2_fwd_kernel / upsample2_bwd_kernel) against the oracle: the forward moves data -> bit for bit;
    the gradient sums four terms -> RTOL"""
    x0 = rnd(B, H, W, C, seed=41)
    x = x0.clone().to(device).requires_grad_(True)
    y = P.upsample2(x)
    assert torch.equal(y.detach().cpu(), O.upsample2(x0)), 'nearest up-sampling copies its input bit for bit'
    xr = x0.double().requires_grad_(True)
    yr = O.upsample2(xr)
    cot = rnd(*yr.shape, seed=42)
    y.backward(cot.to(device))
    yr.backward(cot.double())
    _close(x.grad, xr.grad, 'upsample2 grad')


def test_upsample2_rejects_channels_that_are_no_float4(device):
    with pytest.raises(_native_error()):
        P.upsample2(rnd(1, 2, 2, 6).to(device))


# B, H, W, C -> Ho, Wo.  The issue's wrap example (1, 1128, 940, 2) -> (564, 470) has 564 * 470 * 2 = 530 160 OUTPUT elements, below
# the 1 048 576 at which subsample_fwd_kernel wraps (1 060 320 is its count of input PIXELS); C = 4 gives the 1 060 320 outputs
# asked for, and C = 1 gives 1 060 320 INPUT elements for a gradient that wraps while its forward (265 080) does not.
SUBSAMPLE_CASES = [
    pytest.param(2, 16, 24, 5, 8, 12, id='f2-C5'),
    pytest.param(1, 32, 32, 3, 8, 8, id='f4-C3'),
    pytest.param(2, 64, 64, 1, 8, 8, id='f8-C1'),
    pytest.param(1, 1128, 940, 4, 564, 470, id='f2-fwd-1060320-outputs-wraps'),         # its gradient: 4 241 280 inputs, 5 trips
    pytest.param(1, 1128, 940, 1, 564, 470, id='f2-bwd-1060320-inputs-wraps'),
]


@pytest.mark.parametrize('B,H,W,C,Ho,Wo', SUBSAMPLE_CASES)
def test_resize_nearest_down(B, H, W, C, Ho, Wo, device):
    """ops.resize_nearest_down (subsample_fwd_kernel / subsample_bwd_kernel) == tf.image.resize_nearest_neighbor of the oracle, bit
    for bit; the gradient is the cotangent on the sampled lattice (bit for bit) and exactly 0 off it"""
    f = H // Ho
    x0 = rnd(B, H, W, C, seed=43)
    x = x0.clone().to(device).requires_grad_(True)
    y = P.resize_nearest_down(x, Ho, Wo)
    assert torch.equal(y.detach().cpu(), O.resize_nearest(x0, Ho, Wo))
    cot = rnd(B, Ho, Wo, C, seed=44)
    cot[cot == 0] = 1.0
    y.backward(cot.to(device))
    g = x.grad.cpu()
    assert torch.equal(g[:, ::f, ::f], cot), 'the sampled positions receive the cotangent'
    assert torch.count_nonzero(g) == cot.numel(), 'every other position has gradient exactly 0'
    xr = x0.double().requires_grad_(True)
    O.resize_nearest(xr, Ho, Wo).backward(cot.double())
    assert torch.equal(g.double(), xr.grad)


def test_resize_nearest_down_shortcut_and_refusals(device):
    x = rnd(2, 16, 24, 5, seed=43).to(device)
    assert P.resize_nearest_down(x, 16, 24) is x                         # same size: no launch, the tensor itself
    for Ho, Wo in [(5, 8), (8, 5), (8, 6), (32, 48)]:                    # no integer factor / two different factors / up-sampling
        with pytest.raises(NotImplementedError):
            P.resize_nearest_down(x, Ho, Wo)


# ======================================================================================================================
# 2x2 max pooling
# ======================================================================================================================
def _plant_ties(x, where):
    """where = '00' | '01' | '10' | '11': position (dh, dw) of every 2x2 window gets the value of the window's maximum, so it ties with
    the maximum wherever that was (a random one of the four positions); 'all': all four positions hold the maximum; 'none': no ties"""
    if where == 'none':
        return x
    B, H, W, C = x.shape
    xw = x.reshape(B, H // 2, 2, W // 2, 2, C).clone()
    m = xw.amax(dim=(2, 4))
    if where == 'all':
        xw[:] = m[:, :, None, :, None, :]
    else:
        xw[:, :, int(where[0]), :, int(where[1]), :] = m
    return xw.reshape(B, H, W, C)


@pytest.mark.parametrize('ties', ['none', '00', '01', '10', '11', 'all'])
@pytest.mark.parametrize('B,H,W,C', [
    pytest.param(1, 2, 2, 4, id='one-work-item'),
    pytest.param(3, 6, 10, 4, id='C4-1-75-windows'),
    pytest.param(2, 14, 18, 132, id='C4-33-not-a-power-of-two'),          # 2 * 7 * 9 * 33 = 4158 quads: 17 blocks, the last holds 62
])
def test_maxpool2_boundaries(B, H, W, C, ties, device):
    """ops.maxpool2: values, and the gradient goes to the FIRST maximum of a window in row-major order (TF MaxPoolGrad)"""
    x = _plant_ties(rnd(B, H, W, C, seed=45), ties)
    check(P.maxpool2, O.maxpool2, [x], device)
    if ties != 'none':         # the tie rule itself, not only agreement with the oracle: nothing arrives behind the first maximum
        xd = x.clone().to(device).requires_grad_(True)
        y = P.maxpool2(xd)
        y.backward(torch.ones_like(y))
        gw = xd.grad.cpu().reshape(B, H // 2, 2, W // 2, 2, C).permute(0, 1, 3, 5, 2, 4).reshape(-1, 4)
        xw = x.reshape(B, H // 2, 2, W // 2, 2, C).permute(0, 1, 3, 5, 2, 4).reshape(-1, 4)
        first = (xw == xw.amax(1, keepdim=True)).float().argmax(1)
        assert torch.equal(gw, torch.nn.functional.one_hot(first, 4).float())


def test_maxpool2_grid_wrap(device):
    """(2, 258, 256, 128): 2 * 129 * 128 * 32 = 1 056 768 quads > 1 048 576: maxpool2_fwd_kernel and maxpool2_bwd_kernel wrap.  Maximum
    and routing are exact, so the reference is plain fp32 torch (no fp64 copy of a 68 MB tensor) and the comparison is bit for bit"""
    x0 = rnd(2, 258, 256, 128, seed=46)
    x0[0, :4, :4] = 0.0                                                   # ties, also in the first block
    x0[1, -4:, -4:] = 0.0                                                 # ... and among the wrapped work items
    x = x0.clone().to(device).requires_grad_(True)
    y = P.maxpool2(x)
    xr = x0.clone().requires_grad_(True)
    yr = O.maxpool2(xr)
    assert torch.equal(y.detach().cpu(), yr.detach())
    cot = rnd(*yr.shape, seed=47)
    y.backward(cot.to(device))
    yr.backward(cot)
    assert torch.equal(x.grad.cpu(), xr.grad)


@pytest.mark.parametrize('shape', [pytest.param((1, 3, 4, 4), id='odd-H'), pytest.param((1, 4, 3, 4), id='odd-W'),
                                   pytest.param((1, 4, 4, 6), id='C6-no-float4')])
def test_maxpool2_rejects_what_its_kernels_cannot_index(shape, device):
    with pytest.raises(_native_error()):
        P.maxpool2(rnd(*shape).to(device))


# ======================================================================================================================
# channel slices, axpby
# ======================================================================================================================
@pytest.mark.parametrize('shape,c0,cs', [
    pytest.param((2, 8, 8, 5), 1, 3, id='C5-1+3'),
    pytest.param((2, 8, 8, 5), 4, 1, id='C5-4+1-last-channel'),
    pytest.param((3, 7, 5, 8), 2, 6, id='C8-2+6'),
    # M = 175 000: forward M * Cs = 1 050 000 > 1 048 576 (1424 elements make a second trip), backward M * C = 1 400 000
    pytest.param((2, 250, 350, 8), 2, 6, id='C8-2+6-M175000-both-wrap'),
])
def test_slice_channels(shape, c0, cs, device):
    """ops.slice_channels (slice_fwd_kernel / slice_bwd_kernel): the slice bit for bit; its gradient is the cotangent inside the slice
    and exactly 0 outside"""
    x0 = rnd(*shape, seed=48)
    x = x0.clone().to(device).requires_grad_(True)
    y = P.slice_channels(x, c0, cs)
    assert torch.equal(y.detach().cpu(), x0[..., c0:c0 + cs])
    cot = rnd(*y.shape, seed=49)
    cot[cot == 0] = 1.0
    y.backward(cot.to(device))
    g = x.grad.cpu()
    assert torch.equal(g[..., c0:c0 + cs], cot)
    assert torch.count_nonzero(g) == cot.numel(), 'the gradient outside the slice is exactly 0'


def test_slice_channels_rejects_a_slice_past_the_last_channel(device):
    x = rnd(2, 4, 4, 5).to(device)
    with pytest.raises(_native_error()):
        P.slice_channels(x, 3, 3)
    with pytest.raises(_native_error()):
        P.slice_channels(x, -1, 2)


@pytest.mark.parametrize('n', [
    pytest.param(1, id='n1-tail-only'), pytest.param(3, id='n3-tail-only'), pytest.param(5, id='n5-one-quad-tail-1'),
    pytest.param(4099, id='n4099-1024-quads-tail-3'),
    pytest.param(4194309, id='n4194309-1048577-quads-wrap-tail-1'),      # grid_for(n / 4 + 1) = 4096 blocks: one quad makes a second trip
])
def test_axpby_tail_and_wrap(n, device):
    """ops.axpby (axpby_kernel): float4 body + the scalar tail of n % 4 elements.  The output starts as NaN: an element the kernel does
    not write stays NaN"""
    a, b = rnd(n, seed=50), rnd(n, seed=51)
    out = torch.full((n,), float('nan')).to(device)
    got = P.axpby(a.to(device), b.to(device), 0.75, -1.5, out=out)
    assert got is out
    _close(out, a.double() * 0.75 + b.double() * -1.5, 'axpby')


# ======================================================================================================================
# spectral penalty
# ======================================================================================================================
# KH, KW, Cin, Cout -> W is [K = KH * KW * Cin][N = Cout]
SPEC_SHAPES = [
    (4, 4, 1, 64),        # K = 16 (the discriminators' first layer): kper = 1, K slices 16..31 are empty
    (1, 1, 100, 70),      # K = 100: kper = 4, 25 live slices; N = 70 is no multiple of 64 (gemv_n lanes) nor of 256 (gemv_t block)
    (4, 4, 256, 512),     # K = 4096 > 1024 threads of spec_normalize_kernel (4 trips); N = 512: two column blocks; n = 2 097 152:
                          # 8192 blocks > 4096 -> spec_grad_kernel wraps (4 trips on the 2048 blocks of the batched launch)
    (3, 3, 5, 300),       # K = 45: kper = 2, 23 live slices, the last holds one k; N = 300: column blocks of 256 + 44
]
SPEC_IDS = ['K16-N64', 'K100-N70', 'K4096-N512', 'K45-N300']


@functools.lru_cache(maxsize=None)
def _spec_case(i, regime):
    """-> (w, u0, loss_ref[1], grad_ref) of SPEC_SHAPES[i], computed once and shared (nobody writes to them).  The entries are scaled so
    that the largest singular value is about 0.5 ('below': 1 - 1/sigma < 0) or about 2 ('above': > 0); every 7th weight is exactly 0"""
    shp = SPEC_SHAPES[i]
    K, Nn = shp[0] * shp[1] * shp[2], shp[3]
    target = 0.5 if regime == 'below' else 2.0
    w = rnd(*shp, seed=60 + i, scale=target / (K ** 0.5 + Nn ** 0.5))
    w.view(-1)[::7] = 0.0
    u0 = torch.rand(K, 1, generator=torch.Generator().manual_seed(70 + i)) * 2 - 1
    wr = w.clone().double().requires_grad_(True)
    ref = O.spectral_reg(wr, u0.double(), 10.0)
    (gref,) = torch.autograd.grad(ref, wr)
    # |1 - 1/sigma| and its sign, read back from the reference: loss = alpha * |d| * mean|W|, grad = alpha / n * sign(d) * sign(W)
    d = ref.item() / (10.0 * w.double().abs().mean().item())
    assert d > 0.05, 'sigma too close to 1: the sign of 1 - 1/sigma could flip between fp32 and fp64'
    sign = torch.sign((gref * torch.sign(w.double())).sum()).item()
    assert sign == (-1.0 if regime == 'below' else 1.0)
    return w, u0, ref.detach().reshape(1), gref


@pytest.mark.parametrize('regime', ['below', 'above'])
@pytest.mark.parametrize('i', range(len(SPEC_SHAPES)), ids=SPEC_IDS)
def test_spectral_reg_boundaries(i, regime, device):
    """ops.spectral_reg / spectral_reg_grad, one matrix per call: both signs of 1 - 1/sigma, gradient exactly 0 at weights that are 0"""
    w, u0, ref, gref = _spec_case(i, regime)
    loss, sgn = P.spectral_reg(w.to(device), u0.to(device), 10.0)
    _close(loss, ref, 'loss', 1e-4)
    g = P.spectral_reg_grad(w.to(device), sgn)
    _close(g, gref, 'grad', 1e-5)
    assert torch.count_nonzero(g.cpu()[w == 0]) == 0
    assert torch.count_nonzero(g.cpu()[w != 0]) == (w != 0).sum()


@pytest.mark.parametrize('members', [
    pytest.param(((0, 'below'), (1, 'above'), (2, 'below'), (3, 'above')), id='four-mixed-signs'),
    pytest.param(((3, 'below'), (2, 'above'), (0, 'above')), id='three-largest-in-the-middle'),
    pytest.param(((2, 'above'),), id='one-K4096-N512'),
    pytest.param(((0, 'below'),), id='one-K16-N64'),
])
def test_spectral_reg_multi_boundaries(members, device):
    """ops.spectral_reg_multi / spectral_reg_grad_accumulate: the same matrices in one batch of launches (grids sized by the largest
    member, smaller members leave early), accumulated into NON-ZERO gradients"""
    cases = [_spec_case(i, regime) for i, regime in members]
    ws_ = [c[0].to(device) for c in cases]
    loss, sgn = P.spectral_reg_multi(ws_, [c[1].to(device) for c in cases], 10.0)
    _close(loss, torch.cat([c[2] for c in cases]), 'losses', 1e-4)
    for k, c in enumerate(cases):                                         # each member within ITS OWN magnitude
        _close(loss[k:k + 1], c[2], 'loss %d' % k, 1e-4)
    grads = [torch.full_like(w, 0.5) for w in ws_]
    P.spectral_reg_grad_accumulate(ws_, sgn, grads)
    for g, c in zip(grads, cases):
        _close(g - 0.5, c[3], 'grad', 1e-5)
        assert torch.equal(g.cpu()[c[0] == 0], torch.full((int((c[0] == 0).sum()),), 0.5)), 'a weight that is 0 adds exactly 0'
        assert torch.count_nonzero((g.cpu() - 0.5)[c[0] != 0]) == (c[0] != 0).sum()


# ======================================================================================================================
# batch plumbing of csrc/act16.hip: sums of fan-out gradients, batch concatenation, row gather, background channel
# ======================================================================================================================
# Where the code differs from the plan these cases were drawn up from: ops._cat_words hands the second launch of more than 8 parts the
# destination out[8 * B:], 8 * words * 4 = 32 * words bytes behind the first: a multiple of 16 for ANY words, so a second launch never
# starts unaligned through cat_batch / split_batch (words = 7, n = 15: byte 224).  Inside each launch parts 1, 2, 3, 5, 6, 7 of 7 words
# are unaligned; a destination that itself starts unaligned is covered by the direct calls below (`off` = 1 word).
NAN = float('nan')
SENTINEL = -77.0


def _N():
    from multimodal_segmentation_amd import _native as N
    return N


def _left_to_right(ts):
    acc = ts[0].clone()
    for t in ts[1:]:
        acc = acc + t
    return acc


# n operands, numel.  n4 = numel // 4 groups of four + numel % 4 tail elements; n = 9: two launches (8 operands, then the sum + the 9th)
SUM_N_CASES = [pytest.param(n, numel, id='n%d-numel%d-%s' % (n, numel, 'tail-only' if numel < 4 else 'one-quad-tail-%d' % (numel % 4)))
               for numel in (3, 5, 6, 7) for n in (1, 2, 8, 9)] + [
    # grid16(n4 + 1) = 4096 blocks x 256 threads = 1 048 576: one quad makes a second trip, and three tail elements follow
    pytest.param(2, 4194311, id='n2-numel4194311-1048577-quads-wrap-tail-3')]


@pytest.mark.parametrize('n,numel', SUM_N_CASES)
def test_sum_n_tail_and_wrap(n, numel, device):
    """mmseg_sum_n_t with element code 0 (sum_n_kernel<0>) through ops._sum_n, ops.share and by direct call into a NaN buffer: the fp64
    sum at RTOL, and bit for bit the left-to-right fp32 sum of plain torch"""
    ts = [rnd(numel, seed=80 + k) for k in range(n)]
    want, exact = sum(t.double() for t in ts), _left_to_right(ts)
    ds = [t.to(device) for t in ts]
    got = P._sum_n(ds, ds[0])
    _close(got, want, 'sum of %d' % n)
    assert torch.equal(got.cpu(), exact)
    if n <= 8:
        out = torch.full((numel,), NAN).to(device)
        _N().call('mmseg_sum_n_t', *(ds + [None] * (8 - n)), n, out, numel, 0)
        _close(out, want, 'direct sum of %d' % n)
        assert torch.equal(out.cpu(), exact)
    if n > 1 and numel < 100:
        x = rnd(numel, seed=79).to(device).requires_grad_(True)
        torch.autograd.backward(P.share(x, n), ds)
        _close(x.grad, want, 'shared grad')


@pytest.mark.gpu
@pytest.mark.parametrize('dtype,h', [(torch.bfloat16, 1), (torch.float16, 2)], ids=['bf16', 'fp16'])
@pytest.mark.parametrize('n,numel', SUM_N_CASES)
def test_sum_n_16bit_codes(n, numel, dtype, h):
    """sum_n_kernel<1> / <2> on the device: bit for bit the rounding of the fp32 left-to-right sum of the widened operands (n = 9: the
    first launch's sum is rounded to 16 bits before the ninth operand is added)"""
    ts = [rnd(numel, seed=80 + k).to(dtype) for k in range(n)]
    ds = [t.to('cuda') for t in ts]
    if n <= 8:
        out = torch.full((numel,), NAN, dtype=dtype, device='cuda')
        _N().call('mmseg_sum_n_t', *(ds + [None] * (8 - n)), n, out, numel, h)
        assert torch.equal(out.cpu(), _left_to_right([t.float() for t in ts]).to(dtype))
        want = out.cpu()
    else:
        first = _left_to_right([t.float() for t in ts[:8]]).to(dtype)
        want = _left_to_right([first.float()] + [t.float() for t in ts[8:]]).to(dtype)
    got = P._sum_n(ds, ds[0])
    assert got.dtype == dtype and torch.equal(got.cpu(), want)


def test_sum_n_rejects_operand_counts_and_null_operands(device):
    a = rnd(8, seed=1).to(device)
    out = torch.zeros(8).to(device)
    N = _N()
    N.call('mmseg_sum_n_t', a, a, a, None, None, None, None, None, 3, out, 8, 0)                # (accepted)
    with pytest.raises(_native_error()):
        N.call('mmseg_sum_n_t', a, None, None, None, None, None, None, None, 0, out, 8, 0)      # n = 0
    with pytest.raises(_native_error()):
        N.call('mmseg_sum_n_t', a, a, a, a, a, a, a, a, 9, out, 8, 0)                           # n = 9
    with pytest.raises(_native_error()):
        N.call('mmseg_sum_n_t', a, None, a, None, None, None, None, None, 3, out, 8, 0)         # a NULL operand below n


# n parts, shape of a part, dtype
CAT_CASES = [
    # 24 bytes per part: part 0 takes the 16-byte branch with a 2-word tail, part 1 starts at byte 24 (one word per thread), part 2 at
    # byte 48 is aligned again
    pytest.param(3, (1, 6), torch.float32, id='words6-n3-vector-tail-2-scalar-vector'),
    pytest.param(8, (1, 1), torch.float32, id='words1-n8-w4-0-parts-0-and-4-tail-only'),
    pytest.param(15, (1, 7), torch.float32, id='words7-n15-two-launches-8+7'),
    pytest.param(2, (1, 4194308), torch.float32, id='words4194308-n2-1048577-quads-wrap'),      # grid16(w4 + 1) = 4096 blocks: one quad wraps
    pytest.param(4, (3, 10), torch.bfloat16, id='bf16-30-elements-15-words-n4'),                # part k starts at byte 60 * k
    pytest.param(3, (2, 4), torch.float16, id='fp16-8-elements-4-words-n3'),
]


@pytest.mark.parametrize('n,shape,dtype', CAT_CASES)
def test_cat_and_split_batch_boundaries(n, shape, dtype, device):
    """ops.cat_batch and the gradient of ops.split_batch (mmseg_cat_words) move bytes: bit for bit; an unused split (a NULL part, written
    as zeros) in the first, a middle and the last position"""
    B = shape[0]
    parts = [rnd(*shape, seed=20 + i).to(dtype) for i in range(n)]
    y = P.cat_batch([t.to(device) for t in parts])
    assert y.dtype == dtype and torch.equal(y.cpu(), torch.cat(parts, 0))
    for unused in sorted({0, n // 2, n - 1}):
        big = rnd(n * B, *shape[1:], seed=6).to(dtype).to(device).requires_grad_(True)
        sp = P.split_batch(big, n)
        use = [i for i in range(n) if i != unused]
        torch.autograd.backward([sp[i] for i in use], [parts[i].to(device) for i in use])
        want = torch.cat([torch.zeros(shape, dtype=dtype) if i == unused else parts[i] for i in range(n)], 0)
        assert torch.equal(big.grad.cpu(), want), 'unused split %d' % unused


def test_cat_batch_of_views_that_start_4_bytes_into_a_buffer(device):
    """ops._c keeps a contiguous view, so the kernel gets sources that are NOT 16-byte aligned for aligned destinations (parts of 24
    words): one word per thread"""
    shape = (2, 3, 4)
    bufs = [rnd(28, seed=30 + i).to(device) for i in range(3)]
    xs = [b[1:25].view(shape) for b in bufs]
    if device == 'cuda':
        assert all(x.data_ptr() % 16 == 4 for x in xs)
    y = P.cat_batch(xs)
    assert torch.equal(y.cpu(), torch.cat([b.cpu()[1:25].view(shape) for b in bufs], 0))


@pytest.mark.parametrize('n,words,off,nulls', [
    pytest.param(3, 6, 0, (), id='words6-n3'),
    pytest.param(3, 6, 0, (0,), id='words6-n3-null-first'),
    pytest.param(3, 6, 0, (1,), id='words6-n3-null-middle-unaligned-part'),
    pytest.param(3, 6, 0, (2,), id='words6-n3-null-last'),
    pytest.param(8, 1, 0, (), id='words1-n8'),
    pytest.param(7, 7, 0, (3,), id='words7-n7-null-middle'),
    pytest.param(4, 8, 1, (), id='words8-n4-destination-starts-at-byte-4-all-scalar'),
    pytest.param(2, 9, 3, (1,), id='words9-n2-destination-starts-at-byte-12-part-1-aligned-null'),   # 12 + 36 = 48
    pytest.param(2, 4194308, 0, (), id='words4194308-n2-wraps'),
])
def test_cat_words_writes_its_range_and_nothing_else(n, words, off, nulls, device):
    """mmseg_cat_words by direct call into a buffer full of a sentinel: the n * words words are written, the words in front (`off`) and
    the row behind keep the sentinel"""
    buf = torch.full((off + (n + 1) * words,), SENTINEL).to(device)
    out = buf[off:off + n * words].view(n, words)
    parts = [None if k in nulls else rnd(1, words, seed=30 + k) for k in range(n)]
    _N().call('mmseg_cat_words', *([None if t is None else t.to(device) for t in parts] + [None] * (8 - n)), n, out, words)
    want = torch.cat([torch.zeros(1, words) if t is None else t for t in parts], 0)
    got = buf.cpu()
    assert torch.equal(got[off:off + n * words].view(n, words), want)
    assert bool((got[:off] == SENTINEL).all()) and bool((got[off + n * words:] == SENTINEL).all()), 'written outside the range'


def test_cat_words_rejects_part_counts(device):
    a = rnd(1, 4, seed=1).to(device)
    N = _N()
    with pytest.raises(_native_error()):
        N.call('mmseg_cat_words', a, None, None, None, None, None, None, None, 0, torch.zeros(1, 4).to(device), 4)
    with pytest.raises(_native_error()):
        N.call('mmseg_cat_words', a, a, a, a, a, a, a, a, 9, torch.zeros(9, 4).to(device), 4)


def _idx(rows, src_rows, seed):
    return torch.randint(0, src_rows, (rows,), generator=torch.Generator().manual_seed(seed), dtype=torch.int64)


GATHER_CASES = [
    # gridDim.y = min(4096, rows): row 4096 is taken by the block of row 0 on its second trip
    pytest.param((50, 4), _idx(4097, 50, 1), id='rows4097-of-4-words-gridy-4096-row-4096-second-trip'),
    pytest.param((10, 6), torch.tensor([9, 8, 7, 7, 6, 5, 4, 3, 3, 2, 1, 0, 0]), id='6-words-scalar-branch-descending-repeated'),
    pytest.param((5, 1028), torch.tensor([4, 4, 0, 2]), id='1028-words-257-quads-two-x-blocks-second-holds-1'),
    # words / 4 = 1 048 578 quads for min(1024, 4097) = 1024 x blocks of 256: every thread makes 4 trips, two make a fifth
    pytest.param((2, 4194312), torch.tensor([1, 0]), id='2-rows-of-4194312-words-bx-capped-at-1024-wraps'),
    pytest.param((5, 8), torch.zeros(0, dtype=torch.int64), id='rows0-no-launch'),
    pytest.param((5, 0), torch.tensor([1, 2]), id='words0-no-launch'),
    pytest.param((12, 2, 3), torch.tensor([11, 0, 11]), id='bf16-rows-of-6-elements-3-words'),
]


@pytest.mark.parametrize('src_shape,idx', GATHER_CASES)
def test_gather_rows_boundaries(src_shape, idx, device):
    """ops.gather_rows and mmseg_gather_rows into a NaN buffer == index_select along the leading axis, bit for bit"""
    src = rnd(*src_shape, seed=3)
    if len(src_shape) == 3:
        src = src.to(torch.bfloat16)
    want = src.index_select(0, idx)
    sd, idd = src.to(device), idx.to(device)
    assert torch.equal(P.gather_rows(sd, idd).cpu(), want)
    out = torch.full(want.shape, NAN, dtype=src.dtype).to(device)
    words = (src.numel() // src_shape[0]) * src.element_size() // 4
    _N().call('mmseg_gather_rows', sd, idd, out, idx.numel(), words, src_shape[0])
    assert torch.equal(out.cpu(), want)


@pytest.mark.gpu
@pytest.mark.parametrize('words', [8, 6], ids=['16-byte-branch', 'scalar-branch'])
def test_gather_rows_skips_indices_outside_the_source(words):
    """by direct call on the device (ops.gather_rows' callers validate their indices): an index of -1 or of src_rows leaves the output
    row as it was and reads nothing (the kernel `continue`s in front of the row's address)"""
    src = rnd(4, words, seed=4).to('cuda')
    idx = torch.tensor([2, -1, 4, 0, 3], dtype=torch.int64, device='cuda')
    out = torch.full((5, words), SENTINEL, device='cuda')
    _N().call('mmseg_gather_rows', src, idx, out, 5, words, 4)
    got, s = out.cpu(), src.cpu()
    assert torch.equal(got[[0, 3, 4]], s[[2, 0, 3]])
    assert bool((got[[1, 2]] == SENTINEL).all())


@pytest.mark.parametrize('M,C', [
    pytest.param(1, 1, id='M1-C1'), pytest.param(1, 4, id='M1-C4'), pytest.param(7, 4, id='M7-C4'), pytest.param(300, 1, id='M300-C1-two-blocks'),
    pytest.param(1048577, 1, id='M1048577-C1-wraps-by-one-row'),                 # grid16(M) = 4096 blocks x 256 rows = 1 048 576
])
def test_add_residual_boundaries(M, C, device):
    """ops.add_residual and mmseg_add_residual into a NaN buffer: the background channel is 1 unless some mask equals 1 EXACTLY.  The
    neighbours of 1 in fp32, 1, -1 and 0 are planted in the first row, the last row of the first trip and the first wrapped row"""
    import numpy as np
    base = (torch.rand(M, C, generator=torch.Generator().manual_seed(3)) > 0.8).float()
    anchors = sorted({0, min(M, 1048576) - 1, M - 1})
    vals = [float(np.nextafter(np.float32(1), np.float32(0))), float(np.nextafter(np.float32(1), np.float32(2))), 1.0, -1.0, 0.0]
    for j, v in enumerate(vals):
        m = base.clone()
        for r in anchors:
            m[r] = 0.5
            m[r, j % C] = v
        assert m[0, j % C].item() == v
        want = torch.cat([m, 1.0 - (m == 1).any(-1, keepdim=True).float()], -1)
        for r in anchors:
            assert want[r, C].item() == (0.0 if v == 1.0 else 1.0)
        md = m.to(device)
        assert torch.equal(P.add_residual(md).cpu(), want), 'planted %r' % v
        out = torch.full((M, C + 1), NAN).to(device)
        _N().call('mmseg_add_residual', md, out, M, C)
        assert torch.equal(out.cpu(), want), 'planted %r (direct)' % v


def test_add_residual_rejects_zero_channels(device):
    with pytest.raises(_native_error()):
        _N().call('mmseg_add_residual', torch.zeros(4, 1).to(device), torch.zeros(4, 1).to(device), 4, 0)
