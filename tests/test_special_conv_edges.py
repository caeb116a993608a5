"""The special-purpose convolution kernels (csrc/conv.hip, csrc/smallconv.hpp, csrc/s2conv.hpp) where their grids wrap.

Continues tests/test_conv_edges.py with the same conventions: every operator case runs on the device (`-m gpu`) and through
tests/cpu_backend.py against the fp64 oracle on the same seeded fp32 inputs, gradient buffers start NON-ZERO (gbuf_pattern), the id of a
case gives the arithmetic it exercises, and on the device every case asserts the kernel codes of its three launches
(mmseg_conv2d_last_kernel: family * 1000000 + 1000 * a + b, see MMSEG_SET_LAST at each launcher).  fp32, mmseg_conv16_mode 1 (the default).
These are the families that test_conv_edges.py lists as "outside this stack": until this file their only value tests were the small
CONV_CASES, none of which reaches a capped grid, a second trip of a tile loop or a two-level slab reduction.

Launch arithmetic, recomputed from the launchers (M = B * Ho * Wo output pixels):

  conv_dispatch, 8 -> 8   conv_direct_mfma_kernel<3> (family 3): ceil(M / 256) blocks through xcd_remap, a lane = a pixel, a 4x4x1 MFMA block = 4
                          consecutive pixels (index order: they may lie in two rows or two samples); lanes >= M are not `live`: no taps, no store.
                          The data gradient is the same launch on the flipped kernel.
  smallconv_dispatch      pw_reduce_kernel<LANES, COUT, VPL> (family 10, code LANES / COUT): 64 -> 5 <16,5>, 64 -> 8 <8,8,2>, 16 -> 1 <4,1>, 8 -> 1 <2,1>;
                          nb = min(ceil(M / (64 * 64 / LANES)), 2048) blocks, a wave takes 4 / VPL groups of 64 / LANES pixels per trip.
                          smallk_conv_kernel<KS, CIN, L> (family 11, code KS * 20 + L / CIN), L = Cout / 4 in {16, 4, 2} lanes per pixel:
                          nb = min(ceil(M * L / 1024), 2048) blocks, pixel = thread / L, step = gridDim.x * 256 / L pixels -- capped when
                          M * L > 2097152, then step = 524288 / L (32768 pixels at L = 16).
  s2conv_dispatch         s2k3c9_fwd_kernel (family 21): a wave = a 16-pixel tile, blocks = min(ceil(ceil(M / 16) / 4), 2048), tile += 4 * gridDim.x --
                          taken only when M > 131072.  s2k3c9_dgrad_kernel (21, b = 9): gridDim.y = the four parity classes of the input pixels,
                          blocks = min(ceil(ceil(Mc / 16) / 4), 1024) for the largest class Mc = B * ceil(H / 2) * ceil(W / 2): the loop wraps when Mc > 65536.
                          locnet5_fwd_kernel<PREC> (16-bit modes) / locnet5_f32_kernel<CA, CB, NOUT, PREC> (family 23, code Cin / Cout): tiles of 8 x 64
                          output pixels, min(B * ceil(Ho / 8) * ceil(Wo / 64), 512) blocks, a block walks tiles bid, bid + gridDim.x, ... and restages
                          its LDS patch behind a barrier; <8,8,20> first layer, <20,0,20> second / third layer and their padding-4 data gradients,
                          <20,0,16> the first layer's data gradient (16 outputs stored 8 + 8).
  ops._Conv2d.backward    4x4 stride 2 'valid', Cout = 64, Cin in {1, 4}: conv_dgrad_s2k4_smallc_kernel<Cin> (family 5), 16 lanes per 2 x 2 input
                          pixels, ceil(B * ceil(H / 2) * ceil(W / 2) / 16) blocks.
  conv2d_wgrad_impl       cap = min(wgrad_splits(M, K, Cout), 1024) with wgrad_splits = min(ceil(3072 / (ceil(K / 128) * ceil(Cout / BN))), ceil(M / 512)).
                          pw_reduce_wgrad_kernel (family 12): nblk = min(ceil(M / (256 * 64 / LANES)), cap) slabs.
                          smallk_wgrad_kernel<KS, 1, L> (13): nblk = min(ceil(M * L / 4096), cap).
                          s2k3c9_wgrad_kernel (22): nsteps = ceil(M / 4) groups of 4 pixels, nb = min(cap, 512), steps = ceil(nsteps / (4 nb)) per wave,
                          nblk = ceil(nsteps / (4 steps)); the last block's waves may hold fewer (or no) steps.
                          locnet5_wgrad_kernel (24): tiles of 4 x 64, nblk = min(B * ceil(Ho / 4) * ceil(Wo / 64), 512), a block walks its tiles as above.
                          All four stage nblk slabs (also for nblk = 1) and launch_slab_reduce adds them: nblk > 64 -> ceil(nblk / 32) groups of 32 (the
                          last partial) into ws[nblk * K * Cout ...], then those; accumulate = 1 adds to dW.

Every instantiation of these families that the dispatchers can select, the case that reaches it and the edge (old = CONV_CASES of tests/test_ops_parity.py;
new = SPECIAL_EDGES below, direct = the direct calls of sections 2 and 3):
  conv_direct_mfma_kernel<3>        old 2x16x16, 2x128x128, 3x16x192 (M % 256 == 0, W % 4 == 0)   new 3x17x19: 4 blocks (xcd_remap with nwg % 8 = 4), 201 live lanes
                                    in the last, M % 4 = 1, W % 4 = 3   new 1x5x3: one wave, last quad 3 live pixels   new 2x9x64: W % 4 = 0, M % 256 = 128
  conv_dgrad_s2k4_smallc_kernel     <1> old 2x33x31, new 1x729x729: 8327 blocks, odd input (last row and column: one tap)   <4> old 2x34x30, 1x446x446 of test_conv_edges.py
  pw_reduce_kernel                  <16,5> new 1x363x363: 515 blocks, last wave partial   <8,8,2> new 1x363x363: 258 blocks   <4,1> new 1x513x513: 258 blocks
                                    <2,1> new 1x725x725: 257 blocks (all below the 2048 cap: it needs M > 2097152 pixels at 64 channels, 537 MB)
  pw_reduce_wgrad_kernel            <16,5> new 1x363x363: 129 slabs, groups 32 x 4 + 1; direct 1 / 33 / 129 slabs   <8,8,2> new 1x363x363: 65 slabs (32, 32, 1)
                                    <4,1> new 1x513x513: 65 slabs, the first M with more than 64   <2,1> new 1x725x725: 65 slabs, likewise
  smallk_conv_kernel                <3,1,16> new 1x363x363: capped, 4 trips of 32768 pixels + 697   <4,1,16> new 1x729x729: capped, same M
                                    <1,5,16> / <1,8,16> new 1x363x363 64 -> 5 / 64 -> 8 (data gradient): capped   <1,1,4> / <1,1,2> new 1x513x513 / 1x725x725
                                    (data gradient): 1029 / 1027 blocks, M * L just above 2 ^ 20   <1,5,2> old 3x17x19 8 -> 5   <3,1,4> old 2x19x23 1 -> 16
                                    <1,1,16> new 3x17x19 1 -> 64 1x1   <1,5,4> new 3x17x19 5 -> 16   <1,8,4> new 3x17x19 8 -> 16   <1,8,2> new 3x17x19 8 -> 8 1x1
                                    <3,1,2> new 2x19x23 1 -> 8   <4,1,4> new 2x37x41 1 -> 16   <4,1,2> new 2x37x41 1 -> 8 (no case before: ragged last wave)
  smallk_wgrad_kernel               <3,1,16> new 1x363x363: cap 258 < nb 515 -> 258 slabs (32 x 8 + 2); direct 1 / 20 / 258   <4,1,16> new 1x729x729: 258 slabs;
                                    direct 65 (32, 32, 1)   <3,1,4> old 2x19x23   <3,1,2> new 2x19x23 1 -> 8   <4,1,4> / <4,1,2> new 2x37x41 (one slab each)
  s2k3c9_fwd_kernel                 new 1x727x726: M = 131406, 8213 tiles, 2054 -> 2048 blocks, waves 0 .. 20 take a second tile, the last tile holds 14 pixels
  s2k3c9_dgrad_kernel               new 1x727x726: classes 132132, 132132, 131769, 131769 > 65536: 1024 blocks, 8259 / 8236 tiles on 4096 waves (2 - 3 each);
                                    column 725 is reached by no tap and is exactly 0
  s2k3c9_wgrad_kernel               new 1x727x726: cap 257, steps 32, 257 slabs (32 x 8 + 1), the last block holds 84 of its 128 steps; direct 1 / 20 / 257
  locnet5_f32_kernel<8,8,20,0>      new 130x13x69: Ho x Wo = 9 x 65, 520 tiles on 512 blocks, blocks 0 .. 7 two trips, second row tile 1 live row, second column
                                    tile 1 live column   new 530x6x70: 2 x 66, 1060 tiles, blocks 0 .. 35 three trips, every tile ragged in both directions
  locnet5_f32_kernel<20,0,20,0>     new 130x13x69 20 -> 20: forward 520 tiles; data gradient (padding 4, 9 x 65 -> 13 x 69) 520 tiles
  locnet5_f32_kernel<20,0,16,0>     new 130x13x69 / 530x6x70 (data gradient of the first layer, padding 4, stored 8 + 8): output 13 x 69 / 6 x 70, 2 x 2 /
                                    1 x 2 tiles per sample, 520 / 1060 tiles (blocks 0 .. 7 two trips / blocks 0 .. 35 three trips, as the forward pass)
  locnet5_wgrad_kernel              new 130x13x69: 780 tiles of 4 x 64 on 512 blocks -> 512 slabs, 16 groups of 32   new 530x6x70: 1060 tiles, 512 slabs;
                                    direct 1 / 18 / 66 (32, 32, 2) / 512
  locnet5_fwd_kernel<1>, <2> and locnet5_f32_kernel<..., PREC 1 / 2> (16-bit modes): tests/test_act16.py, which this change gives the 520-tile geometry
                                    (the first layer on locnet5_fwd_kernel; <20,0,20,PREC> forward and padding-4 data gradient, <20,0,16,PREC> with
                                    the split store).

Mutants (scratch copies of csrc/, one at a time, each run once on the device against this file and the older conv tests, which stayed green) and
what they did to the tests of this file (1 = test_special_conv2d_boundaries, 2 = test_special_wgrad_slabs_direct, 3 = test_special_forward_direct_...):
  single trip instead of `bid += gridDim.x` / `tile += nw`   locnet5_f32_kernel: 1 failed on the three locnet5 cases, 3 on both locnet5 cases (and
      the six 130-sample cases of tests/test_act16.py's other-layers test); locnet5_wgrad_kernel: 1 on both locnet5-first cases, 2 on
      locnet5-780-tiles-capped-512-slabs; locnet5_fwd_kernel: tests/test_act16.py's first-layer test at 130x13x69, both modes; s2k3c9_fwd_kernel: 1 and 3
      on the s2k3c9 case; s2k3c9_dgrad_kernel: 1 on the s2k3c9 case
  first barrier of the tile loop moved behind the patch stores   locnet5_f32_kernel: 1 failed on the data gradients of locnet5-first-520-tiles,
      locnet5-first-1060-tiles and locnet5-20to20-520-tiles (the forward launches and 3 passed in that run: a race, it need not show);
      locnet5_wgrad_kernel: 1 locnet5-first-520-tiles and 2 locnet5-780-tiles-capped-512-slabs failed; locnet5_fwd_kernel: nothing failed in the one
      run, also not tests/test_act16.py's 130x13x69 -- the race did not show, and the run was not repeated to make it show
  smallk step taken from the uncapped block count (the cap then skips pixels)   1 failed on the four capped smallk launches (smallk-3x3-1to64,
      smallk-4x4s2-1to64, pw_reduce-16x5 and pw_reduce-8x8x2 through their data gradients), 3 on smallk-3x3-capped-2048-blocks, and test_conv2d_bf16_precision at 1x363x363
  SMK1's cap 2048 -> 1024 alone   survives: the kernel takes its step from gridDim.x, every pixel is still computed with the same arithmetic
  tmp2 = nullptr for nblk > 64   values unchanged (one level adds the same slabs); 2 failed on all seven geometries above 64 slabs, both
      accumulate settings: the first-level partial sums behind the slabs stayed NaN
  `accumulate` ignored by the special families' reduction   2 failed on all 15 geometries with accumulate = 1; 1 failed on the 12 cases whose weight
      gradient runs on families 12, 13, 22, 24 (gbuf_pattern: the gradient buffers start non-zero)
  `live` dropped from the store of conv_direct_mfma_kernel   3 failed on its three cases: the guard behind the output lost its NaN (run on 2 and 3
      only -- in 1 the stray stores would leave the test's own buffers)
  `live` dropped from its tap predicate   survives: a dead lane then loads values of pixels that exist (or zeros), but row q of a 4x4x1 block depends
      on lane q's A operand alone and the dead lane still stores nothing

Size: no case holds more than about 70 MB of operands, results and gradients on the device (the 64-channel cases: 33.7 MB per tensor) or costs the
oracle more than 1.6 GFLOP per pass (130x13x69 20 -> 20: 1.52).

Tolerances: those of the neighbours -- RTOL = 2e-4 of the tensor's largest magnitude through `check` and for the direct forward calls, 2e-5 of the
largest magnitude for the direct weight-gradient calls.  The weight-gradient sums are up to 131769 terms long, but slab-wise: no fp32 accumulator of
these kernels adds more than 4 * 32 = 128 products (s2k3c9), 64 (pw_reduce), ceil(M / (nblk * 256 / L)) (smallk: its trips; 32 at the capped
258-slab cases, step 258 * 16 = 4128 pixels, M = 131769) or 3 x 256 (locnet5) before the fixed-order tree.
  case                          | tolerance | differs from the neighbour
  ------------------------------+-----------+---------------------------
  (none)                        |           | no case needed another tolerance
"""
import pytest
import torch

from oracle import ops as O
from multimodal_segmentation_amd import ops as P
from multimodal_segmentation_amd import _native as N
from tests.test_ops_parity import RTOL, _anchor, _native_error, check, device, gbuf_pattern, rnd  # noqa: F401 (device: fixture)
from tests.test_conv_edges import _conv_inputs, _fp32_default_mode, _last, _launch_codes, _untouched, _wgrad_geometry, _wgrad_problem


def _groups(S):
    return (S + 31) // 32 if S > 64 else 0


# ======================================================================================================================
# 1. operator level, both backends
# ======================================================================================================================
# B, H, W, C1, C2, Cout, k, stride, padding, act, alpha | kernel codes: forward, weight gradient, data gradient (asserted on the device)
SPECIAL_EDGES = [
    # ---- modality encoder first layer (s2conv.hpp: families 21 / 22) -------------------------------------------------------------------------
    # Ho x Wo = 363 x 362, M = 131406 > 131072: 8213 tiles -> 2054 blocks, capped to 2048, the first 21 waves take a second tile, the last tile has 14
    # live pixels.  Data gradient: classes 364x363, 364x363, 363x363, 363x363 = 132132 .. 131769 > 65536 -> 1024 blocks x 4 classes, 2 - 3 tiles per wave.
    # Weight gradient: cap = min(ceil(3072 / 1), ceil(M / 512)) = 257, nsteps = 32852, steps = 32, 257 slabs -> 9 groups (the last of 1)
    pytest.param(1, 727, 726, 8, 1, 16, 3, 2, 'valid', 'leaky', 0.2, 21016016, 22016016, 21016009,
                 id='s2k3c9-M131406-fwd-capped-2048-dgrad-classes>65536-wgrad-257-slabs'),
    # ---- localisation network first layer (families 23 / 24) ------------------------------------------------------------------------------------
    # Ho x Wo = 9 x 65: 2 x 2 tiles of 8 x 64 per sample, 520 tiles on 512 blocks (blocks 0 .. 7 twice); weight gradient 3 x 2 tiles of 4 x 64 per
    # sample, 780 tiles -> 512 slabs, 16 groups; data gradient <20,0,16> padding 4 -> 13 x 69, 520 tiles, stored 8 + 8
    pytest.param(130, 13, 69, 8, 8, 20, 5, 1, 'valid', 'leaky', 0.3, 23016020, 24016020, 23020016,
                 id='locnet5-first-520-tiles-on-512-blocks-wgrad-780-tiles-512-slabs'),
    # Ho x Wo = 2 x 66: 1 x 2 tiles per sample, 1060 > 2 * 512 tiles (blocks 0 .. 35 three times), 2 live rows of 8 / 4, second column tile 2 columns
    pytest.param(530, 6, 70, 8, 8, 20, 5, 1, 'valid', 'leaky', 0.3, 23016020, 24016020, 23020016,
                 id='locnet5-first-1060-tiles-three-trips-all-tiles-ragged'),
    # ---- second / third layer <20,0,20>: forward 520 tiles, its padding-4 data gradient 9 x 65 -> 13 x 69 likewise.  Weight gradient: Wo % 4 = 1 ->
    # conv_wgrad_fast_kernel <128,32>, S = min(ceil(3072 / 4), ceil(76050 / 512)) = 149
    pytest.param(130, 13, 69, 20, 0, 20, 5, 1, 'valid', 'leaky', 0.2, 23020020, 7128032, 23020020,
                 id='locnet5-20to20-520-tiles-and-padding4-dgrad-520-tiles'),
    # ---- smallk_conv_kernel at the 2048-block cap -------------------------------------------------------------------------------------------
    # M = 131769, M * 16 = 2108304 > 2097152: 2059 -> 2048 blocks, step 32768: four full trips and 697 pixels.  Weight gradient: cap =
    # min(3072, ceil(M / 512)) = 258 < nb = 515 -> 258 slabs (8 groups of 32 + 2).  Data gradient 64 -> 1 3x3: flipped kernel, generic 16-byte <128,32>
    pytest.param(1, 363, 363, 1, 0, 64, 3, 1, 'same', 'relu', 0.0, 11076001, 13076001, 2628032,
                 id='smallk-3x3-1to64-capped-2048-step32768-last697-wgrad-258-slabs'),
    # Ho = Wo = 363: the same cap and slabs on the 4x4 stride-2 instance; data gradient conv_dgrad_s2k4_smallc_kernel<1>: ceil(365 * 365 / 16) = 8327
    # blocks, odd input: the last row and column of 2 x 2 groups hold one pixel
    pytest.param(1, 729, 729, 1, 0, 64, 4, 2, 'valid', 'leaky', 0.2, 11096001, 13096001, 5001064,
                 id='smallk-4x4s2-1to64-capped-2048-dgrad-s2k4-8327-blocks-odd-input'),
    # ---- pw_reduce heads: M = 131769 ---------------------------------------------------------------------------------------------------------
    # forward ceil(M / 256) = 515 blocks, the last wave partial; weight gradient ceil(M / 1024) = 129 slabs (32, 32, 32, 32, 1); data gradient
    # smallk<1,5,16> capped as above
    pytest.param(1, 363, 363, 64, 0, 5, 1, 1, 'same', None, 0.0, 10016005, 12016005, 11036005,
                 id='pw_reduce-16x5-515-blocks-wgrad-129-slabs-last-group-1-dgrad-capped'),
    # <8,8,2>: forward ceil(M / 512) = 258 blocks; weight gradient ceil(M / 2048) = 65 slabs (32, 32, 1); data gradient smallk<1,8,16> capped
    pytest.param(1, 363, 363, 64, 0, 8, 1, 1, 'same', None, 0.0, 10008008, 12008008, 11036008,
                 id='pw_reduce-8x8x2-258-blocks-wgrad-65-slabs-dgrad-capped'),
    # the first sizes with 65 slabs: ceil(M / 4096) with M = 263169 > 262144 and ceil(M / 8192) with M = 525625 > 524288 (cap 515 / 1024).
    # Data gradients smallk<1,1,4> (1029 blocks) / smallk<1,1,2> (1027 blocks)
    pytest.param(1, 513, 513, 16, 0, 1, 1, 1, 'same', 'tanh', 0.0, 10004001, 12004001, 11024001, id='pw_reduce-4x1-M263169-wgrad-65-slabs'),
    pytest.param(1, 725, 725, 8, 0, 1, 1, 1, 'same', 'tanh', 0.0, 10002001, 12002001, 11022001, id='pw_reduce-2x1-M525625-wgrad-65-slabs'),
    # ---- conv_direct_mfma_kernel off its round sizes (the data gradient is the same kernel on the flipped weights; weight gradient: H % 8 != 0 ->
    # conv_wgrad_fast_kernel <128,32>) ---------------------------------------------------------------------------------------------------------
    pytest.param(3, 17, 19, 8, 0, 8, 3, 1, 'same', 'leaky', 0.2, 3008008, 7128032, 3008008,
                 id='direct-mfma-M969-4-blocks-last-201-live-M%4=1-W%4=3-quads-straddle-rows-and-samples'),
    pytest.param(1, 5, 3, 8, 0, 8, 3, 1, 'same', None, 0.0, 3008008, 7128032, 3008008, id='direct-mfma-M15-one-wave-last-quad-3-live'),
    pytest.param(2, 9, 64, 8, 0, 8, 3, 1, 'same', 'relu', 0.0, 3008008, 7128032, 3008008, id='direct-mfma-M1152-W%4=0-M%256=128-5-blocks'),
    # ---- the smallk_conv_kernel / smallk_wgrad_kernel instances no case selected before: ragged last waves, grids that wrap uncapped --------------
    # M = 969 1x1 layers: weight gradients on the generic / fast kernels (KS = 1 has no smallk_wgrad instance), data gradients 1x1 with the flipped kernel
    pytest.param(3, 17, 19, 1, 0, 64, 1, 1, 'same', None, 0.0, 11036001, 8128064, 2628032, id='smallk-1x1-1to64-L16-M969'),
    pytest.param(3, 17, 19, 5, 0, 16, 1, 1, 'same', 'relu', 0.0, 11024005, 8128032, 2628032, id='smallk-1x1-5to16-L4-M969'),
    pytest.param(3, 17, 19, 8, 0, 16, 1, 1, 'same', None, 0.0, 11024008, 7128032, 2628032, id='smallk-1x1-8to16-L4-M969'),
    pytest.param(3, 17, 19, 8, 0, 8, 1, 1, 'same', 'leaky', 0.2, 11022008, 7128032, 11022008, id='smallk-1x1-8to8-L2-M969-dgrad-same-kernel'),
    pytest.param(2, 19, 23, 1, 0, 8, 3, 1, 'same', 'leaky', 0.2, 11062001, 13062001, 2628032, id='smallk-3x3-1to8-L2-M874-one-slab'),
    pytest.param(2, 37, 41, 1, 0, 16, 4, 2, 'valid', None, 0.0, 11084001, 13084001, 2628032, id='smallk-4x4s2-1to16-L4-M646-one-slab'),
    pytest.param(2, 37, 41, 1, 0, 8, 4, 2, 'valid', 'relu', 0.0, 11082001, 13082001, 2628032, id='smallk-4x4s2-1to8-L2-M646-one-slab'),
]


@pytest.mark.parametrize('B,H,W,C1,C2,Cout,k,stride,padding,act,alpha,k_fwd,k_wgrad,k_dgrad', SPECIAL_EDGES)
def test_special_conv2d_boundaries(B, H, W, C1, C2, Cout, k, stride, padding, act, alpha, k_fwd, k_wgrad, k_dgrad, device):
    seen, held = [], {}

    def f_prod(x1, w, b, x2=None):
        held['x1'], held['x2'] = x1, x2
        y = P.conv2d(x1, w, b, stride=stride, padding=padding, act=act, alpha=alpha, x2=x2, wgrad=w.gbuf, bgrad=b.gbuf, anchor=_anchor(x1))
        if device == 'cuda':
            seen.append(_last())
        return y

    def f_ref(x1, w, b, x2=None):
        xin = x1 if x2 is None else torch.cat([x1, x2], -1)
        y = O.conv2d(xin, w, b, stride=stride, padding=padding)
        f_ref.pre = y
        if act == 'relu':
            y = torch.relu(y)
        elif act == 'leaky':
            y = O.leaky_relu(y, alpha)
        elif act == 'tanh':
            y = torch.tanh(y)
        return y

    with _fp32_default_mode():
        check(f_prod, f_ref, _conv_inputs(B, H, W, C1, C2, Cout, k, False), device, param_idx=(1, 2), gbuf_fill=gbuf_pattern)
        if stride == 2 and (W - k) % 2:
            # the last input column is reached by no tap: its gradient is exactly zero, not a rounded sum
            assert not held['x1'].grad[:, :, W - 1].any()
            assert held['x2'] is None or not held['x2'].grad[:, :, W - 1].any()
        if device == 'cuda':
            seen.append(_last())       # the backward of `check` wants the input gradient: its last launch is the data gradient
            assert tuple(seen) == (k_fwd, k_dgrad), 'forward / data gradient ran on %s' % (seen,)
            got = _launch_codes(B, H, W, C1, C2, Cout, k, stride, padding, act, False)
            assert got == (k_fwd, k_wgrad, k_dgrad), 'forward / weight gradient / data gradient ran on %s' % (got,)


# ======================================================================================================================
# 2. direct weight-gradient calls: one slab, several, the two-level reduction, accumulation (device only)
# ======================================================================================================================
# B, H, W, C1, C2, Cout, k, stride, padding | family, nblk (slabs the launch stages)
SPECIAL_WGRAD_DIRECT = [
    # ---- pw_reduce_wgrad_kernel<16,5>: nblk = ceil(M / 1024) below its cap
    pytest.param(2, 7, 9, 64, 0, 5, 1, 1, 'same', 12, 1, id='pw_reduce-16x5-M126-one-slab'),
    pytest.param(1, 182, 182, 64, 0, 5, 1, 1, 'same', 12, 33, id='pw_reduce-16x5-M33124-33-slabs'),
    pytest.param(1, 363, 363, 64, 0, 5, 1, 1, 'same', 12, 129, id='pw_reduce-16x5-M131769-129-slabs-groups-32x4+1'),
    pytest.param(1, 363, 363, 64, 0, 8, 1, 1, 'same', 12, 65, id='pw_reduce-8x8x2-M131769-65-slabs-groups-32-32-1'),
    # ---- smallk_wgrad_kernel: nblk = min(ceil(M * 16 / 4096), cap)
    pytest.param(2, 7, 9, 1, 0, 64, 3, 1, 'same', 13, 1, id='smallk-3x3-M126-one-slab'),
    pytest.param(1, 100, 100, 1, 0, 64, 3, 1, 'same', 13, 20, id='smallk-3x3-M10000-cap20-below-nb40'),
    pytest.param(1, 363, 363, 1, 0, 64, 3, 1, 'same', 13, 258, id='smallk-3x3-M131769-cap258-below-nb515-groups-32x8+2'),
    pytest.param(1, 366, 366, 1, 0, 64, 4, 2, 'valid', 13, 65, id='smallk-4x4s2-M33124-cap65-groups-32-32-1'),
    # ---- s2k3c9_wgrad_kernel: 2x7x9 -> M = 24, 6 steps on one block (waves 0 .. 2, two each; wave 3 none); 1x200x200 -> M = 9801, cap 20, steps 31,
    # the last block 95 of 124 steps; 1x727x726 -> 257 slabs
    pytest.param(2, 7, 9, 8, 1, 16, 3, 2, 'valid', 22, 1, id='s2k3c9-M24-one-slab-wave3-empty'),
    pytest.param(1, 200, 200, 8, 1, 16, 3, 2, 'valid', 22, 20, id='s2k3c9-M9801-20-slabs-steps31'),
    pytest.param(1, 727, 726, 8, 1, 16, 3, 2, 'valid', 22, 257, id='s2k3c9-M131406-257-slabs-groups-32x8+1'),
    # ---- locnet5_wgrad_kernel: one slab per block, 4 x 64 tiles
    pytest.param(1, 7, 9, 8, 8, 20, 5, 1, 'valid', 24, 1, id='locnet5-3x5-one-tile-one-slab'),
    pytest.param(1, 40, 70, 8, 8, 20, 5, 1, 'valid', 24, 18, id='locnet5-36x66-18-slabs'),
    pytest.param(11, 13, 69, 8, 8, 20, 5, 1, 'valid', 24, 66, id='locnet5-66-tiles-66-slabs-groups-32-32-2'),
    pytest.param(130, 13, 69, 8, 8, 20, 5, 1, 'valid', 24, 512, id='locnet5-780-tiles-capped-512-slabs-16-groups'),
]


@pytest.mark.gpu
@pytest.mark.parametrize('acc', [0, 1], ids=['overwrite', 'accumulate'])
@pytest.mark.parametrize('B,H,W,C1,C2,Cout,k,stride,padding,family,nblk', SPECIAL_WGRAD_DIRECT)
def test_special_wgrad_slabs_direct(B, H, W, C1, C2, Cout, k, stride, padding, family, nblk, acc):
    """mmseg_conv2d_wgrad on the four special weight-gradient families against the fp64 oracle's autograd: NaN-filled workspace of exactly
    mmseg_conv2d_wgrad_workspace floats, dW NaN (accumulate 0) or a known non-zero base (accumulate 1).  These kernels stage one slab per block --
    also a single one -- and the reduction gets nblk slabs, not the S of wgrad_splits: exactly nblk slabs (+ ceil(nblk / 32) partial sums above
    64) are finite afterwards, everything behind them is still NaN.  A second call is bitwise equal to the first."""
    dev = 'cuda'
    Ho, Wo, ph, pw = _wgrad_geometry(H, W, k, stride, padding)
    x1c, x2c, dyc, basec, ref = _wgrad_problem(B, H, W, C1, C2, Cout, k, stride, padding, 0)
    x1, dy, base = x1c.to(dev), dyc.to(dev), basec.to(dev)
    x2 = x2c.to(dev) if C2 else None
    Cin = C1 + C2
    KN = k * k * Cin * Cout
    with _fp32_default_mode():
        need = N.call('mmseg_conv2d_wgrad_workspace', B, Ho, Wo, Cin, Cout, k, k)
        staged = (nblk + _groups(nblk)) * KN
        assert need >= staged
        outs = []
        for _ in range(2):
            ws = torch.full((need,), float('nan'), device=dev)
            dw = base.clone() if acc else torch.full_like(base, float('nan'))
            N.call('mmseg_conv2d_wgrad', x1, x2, dy, dw.view(-1), ws, ws.numel(), B, H, W, C1, C2, Ho, Wo, Cout, k, k, stride, ph, pw, 0, acc)
            fam = _last() // 1000000
            assert fam == family, 'launch went to kernel family %d' % fam
            outs.append(dw)
        nan = torch.isnan(ws)
        assert not nan[:staged].any(), 'a staged slab (or first-level partial sum) was not written'
        assert nan[staged:].all(), 'the launch wrote behind its %d slabs' % nblk
        want = ref + (basec.double() if acc else 0.0)
        scale = float(want.abs().max())
        err = float((outs[0].cpu().double() - want).abs().max())
        print('special wgrad direct: max err %.3e, bound %.3e' % (err, 2e-5 * scale))
        assert not torch.isnan(outs[0]).any()
        assert err <= 2e-5 * scale
        assert torch.equal(outs[0], outs[1]), 'one slab per block and a fixed-order reduction: bitwise reproducible'


# B, H, W, C1, C2, Cout, k, stride, padding | family
WGRAD_REFUSALS = [
    pytest.param(2, 7, 9, 64, 0, 5, 1, 1, 'same', 12, id='pw_reduce'),
    pytest.param(2, 7, 9, 1, 0, 64, 3, 1, 'same', 13, id='smallk'),
    pytest.param(2, 7, 9, 8, 1, 16, 3, 2, 'valid', 22, id='s2k3c9'),
    pytest.param(1, 40, 70, 8, 8, 20, 5, 1, 'valid', 24, id='locnet5'),
]


@pytest.mark.gpu
@pytest.mark.parametrize('B,H,W,C1,C2,Cout,k,stride,padding,family', WGRAD_REFUSALS)
def test_special_wgrad_refuses_a_short_workspace(B, H, W, C1, C2, Cout, k, stride, padding, family):
    """a workspace one float short of mmseg_conv2d_wgrad_workspace is refused with hipErrorInvalidValue (1) before anything is queued: dW and
    the workspace keep their NaN; the same call with the full workspace then runs on the family's kernel"""
    dev = 'cuda'
    Ho, Wo, ph, pw = _wgrad_geometry(H, W, k, stride, padding)
    x1 = rnd(B, H, W, C1, seed=1).to(dev)
    x2 = rnd(B, H, W, C2, seed=2).to(dev) if C2 else None
    dy = rnd(B, Ho, Wo, Cout, seed=3).to(dev)
    with _fp32_default_mode():
        need = N.call('mmseg_conv2d_wgrad_workspace', B, Ho, Wo, C1 + C2, Cout, k, k)
        ws = torch.full((need,), float('nan'), device=dev)
        dw = torch.full((k, k, C1 + C2, Cout), float('nan'), device=dev)
        for acc in (0, 1):
            with pytest.raises(_native_error(), match='hipError_t 1$'):
                N.call('mmseg_conv2d_wgrad', x1, x2, dy, dw.view(-1), ws[:need - 1], need - 1, B, H, W, C1, C2, Ho, Wo, Cout, k, k, stride, ph, pw, 0, acc)
            torch.cuda.synchronize()
            assert _untouched(dw) and _untouched(ws)
        N.call('mmseg_conv2d_wgrad', x1, x2, dy, dw.view(-1), ws, need, B, H, W, C1, C2, Ho, Wo, Cout, k, k, stride, ph, pw, 0, 0)
        assert _last() // 1000000 == family
        assert not torch.isnan(dw).any()


# ======================================================================================================================
# 3. direct forward calls: every output pixel is written, nothing behind the last one; misaligned operands leave for the generic kernel
# ======================================================================================================================
GUARD = 4096       # floats behind the output: more than the 255 dead lanes of a conv_direct_mfma_kernel block (8 floats each) could reach


def _fwd_problem(B, H, W, C1, C2, Cout, k, stride, padding, act, alpha):
    """operands (CPU, fp32) and the fp64 oracle's output"""
    Ho, Wo, ph, pw = _wgrad_geometry(H, W, k, stride, padding)
    x1 = rnd(B, H, W, C1, seed=1)
    x2 = rnd(B, H, W, C2, seed=2) if C2 else None
    w = rnd(k, k, C1 + C2, Cout, seed=3, scale=(2.0 / (k * k * (C1 + C2))) ** 0.5)
    b = rnd(Cout, seed=4, scale=0.1)
    a = x1.double() if x2 is None else torch.cat([x1.double(), x2.double()], -1)
    ref = O.conv2d(a, w.double(), b.double(), stride=stride, padding=padding)
    ref = torch.relu(ref) if act == 1 else (O.leaky_relu(ref, alpha) if act == 2 else ref)
    return x1, x2, w, b, ref, (Ho, Wo, ph, pw)


def _offset_by_one_float(t, dev):
    """a contiguous device copy of `t` whose first element lies 4 bytes behind a 16-byte boundary"""
    buf = torch.empty(t.numel() + 4, device=dev)
    assert buf.data_ptr() % 16 == 0
    v = buf[1:1 + t.numel()].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 16 == 4 and v.is_contiguous()
    return v


# B, H, W, C1, C2, Cout, k, stride, padding, act, alpha | kernel code
FWD_DIRECT = [
    pytest.param(1, 727, 726, 8, 1, 16, 3, 2, 'valid', 2, 0.2, 21016016, id='s2k3c9-capped-2048-blocks-second-tile-last-tile-14-live'),
    pytest.param(130, 13, 69, 8, 8, 20, 5, 1, 'valid', 2, 0.3, 23016020, id='locnet5-520-tiles-on-512-blocks'),
    pytest.param(530, 6, 70, 8, 8, 20, 5, 1, 'valid', 2, 0.3, 23016020, id='locnet5-1060-tiles-three-trips'),
    pytest.param(1, 363, 363, 1, 0, 64, 3, 1, 'same', 1, 0.0, 11076001, id='smallk-3x3-capped-2048-blocks-step32768'),
    pytest.param(3, 17, 19, 8, 0, 8, 3, 1, 'same', 2, 0.2, 3008008, id='direct-mfma-4-blocks-201-live-lanes-in-the-last'),
    pytest.param(1, 5, 3, 8, 0, 8, 3, 1, 'same', 0, 0.0, 3008008, id='direct-mfma-15-live-lanes'),
    pytest.param(2, 9, 64, 8, 0, 8, 3, 1, 'same', 1, 0.0, 3008008, id='direct-mfma-5-blocks-128-live-lanes-in-the-last'),
]


@pytest.mark.gpu
@pytest.mark.parametrize('B,H,W,C1,C2,Cout,k,stride,padding,act,alpha,code', FWD_DIRECT)
def test_special_forward_direct_writes_every_pixel_and_nothing_else(B, H, W, C1, C2, Cout, k, stride, padding, act, alpha, code):
    """mmseg_conv2d_fwd on the wrapped geometries into an output pre-filled with NaN that is followed by a NaN guard: no NaN survives in the output
    (a tile, trip or pixel range that is skipped shows), the guard keeps its NaN (a dead lane that stores shows, inside the test's own buffer), the
    values match the oracle and a second call is bitwise equal"""
    dev = 'cuda'
    x1c, x2c, wc, bc, ref, (Ho, Wo, ph, pw) = _fwd_problem(B, H, W, C1, C2, Cout, k, stride, padding, act, alpha)
    x1, w, b = x1c.to(dev), wc.to(dev), bc.to(dev)
    x2 = x2c.to(dev) if C2 else None
    n = B * Ho * Wo * Cout
    with _fp32_default_mode():
        outs = []
        for _ in range(2):
            buf = torch.full((n + GUARD,), float('nan'), device=dev)
            y = buf[:n].view(B, Ho, Wo, Cout)
            N.call('mmseg_conv2d_fwd', x1, x2, w, None, b, y, None, B, H, W, C1, C2, Ho, Wo, Cout, k, k, stride, ph, pw, 0, 0, act, alpha, 0)
            assert _last() == code, 'launch went to kernel %d' % _last()
            assert torch.isnan(buf[n:]).all(), 'the launch stored behind its last output pixel'
            outs.append(y)
        assert not torch.isnan(outs[0]).any(), 'output pixels were not written'
        scale = float(ref.abs().max())
        err = float((outs[0].cpu().double() - ref).abs().max())
        print('special forward direct: max err %.3e, bound %.3e' % (err, RTOL * scale))
        assert err <= RTOL * scale
        assert torch.equal(outs[0], outs[1])


# B, H, W, C1, C2, Cout, k, stride, padding | which operand is offset, the aligned launch's code, the generic kernel's code
MISALIGNED = [
    # smallconv_dispatch wants x1 and y on 16-byte boundaries
    pytest.param(2, 20, 12, 1, 0, 64, 3, 1, 'same', 'x1', 11076001, 2064064, id='smallk-x-offset-generic-scalar-64x64'),
    pytest.param(2, 20, 12, 1, 0, 64, 3, 1, 'same', 'y', 11076001, 2064064, id='smallk-y-offset-generic-scalar-64x64'),
    pytest.param(3, 17, 19, 64, 0, 5, 1, 1, 'same', 'x1', 10016005, 2128032, id='pw_reduce-x-offset-generic-scalar-128x32'),
    pytest.param(3, 17, 19, 64, 0, 5, 1, 1, 'same', 'y', 10016005, 2628032, id='pw_reduce-y-offset-generic-vec-128x32'),
    # s2conv_dispatch: s2k3c9_fwd_kernel reads x1 with 8-byte loads and stores 16 bytes; the locnet5 kernels read and store 16 bytes
    pytest.param(2, 33, 33, 8, 1, 16, 3, 2, 'valid', 'x1', 21016016, 2128032, id='s2k3c9-x1-offset-generic-scalar-128x32'),
    pytest.param(2, 33, 33, 8, 1, 16, 3, 2, 'valid', 'y', 21016016, 2128032, id='s2k3c9-y-offset-generic-scalar-128x32'),
    pytest.param(2, 20, 20, 8, 8, 20, 5, 1, 'valid', 'x2', 23016020, 2128032, id='locnet5-x2-offset-generic-scalar-128x32'),
    pytest.param(2, 20, 20, 8, 8, 20, 5, 1, 'valid', 'y', 23016020, 2628032, id='locnet5-y-offset-generic-vec-128x32'),
]


@pytest.mark.gpu
@pytest.mark.parametrize('B,H,W,C1,C2,Cout,k,stride,padding,which,k_special,k_generic', MISALIGNED)
def test_special_forward_misaligned_operands_fall_through_to_the_generic_kernel(B, H, W, C1, C2, Cout, k, stride, padding, which, k_special, k_generic):
    """an input or output that starts one float behind a 16-byte boundary cannot run on the vector loads and stores of the special kernels:
    smallconv_dispatch and s2conv_dispatch pass the launch on to conv_fwd_kernel (scalar gather when an input is offset, scalar stores when the
    output is) -- the kernel code changes, the values stay within tolerance of the oracle"""
    dev = 'cuda'
    x1c, x2c, wc, bc, ref, (Ho, Wo, ph, pw) = _fwd_problem(B, H, W, C1, C2, Cout, k, stride, padding, 0, 0.0)
    w, b = wc.to(dev), bc.to(dev)
    scale = float(ref.abs().max())
    with _fp32_default_mode():
        for off, want in ((None, k_special), (which, k_generic)):
            x1 = _offset_by_one_float(x1c, dev) if off == 'x1' else x1c.to(dev)
            x2 = None if not C2 else (_offset_by_one_float(x2c, dev) if off == 'x2' else x2c.to(dev))
            y = torch.full((B, Ho, Wo, Cout), float('nan'), device=dev)
            if off == 'y':
                y = _offset_by_one_float(y, dev)
            N.call('mmseg_conv2d_fwd', x1, x2, w, None, b, y, None, B, H, W, C1, C2, Ho, Wo, Cout, k, k, stride, ph, pw, 0, 0, 0, 0.0, 0)
            assert _last() == want, 'operand offset %s: launch went to kernel %d' % (off, _last())
            assert not torch.isnan(y).any()
            assert float((y.cpu().double() - ref).abs().max()) <= RTOL * scale
