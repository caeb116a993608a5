"""The 16-bit and patch-resident convolutions (csrc/conv16.hpp, csrc/wgrad32h.hpp, the 16-bit instances of csrc/conv.hip) at their plan and grid edges.

Continues tests/test_conv_edges.py, tests/test_special_conv_edges.py and tests/test_ups_fold.py with their conventions: the id of a case gives the
arithmetic it exercises ("holeN" = the gap of the list below it closes), every launch asserts the FULL kernel code (mmseg_conv2d_last_kernel: family *
1000000 + M-tile field * 1000 + N tile, see MMSEG_SET_LAST at each launcher), outputs and workspaces start as NaN, dW starts non-zero when accumulating,
precision mode and mmseg_conv16_mode are restored in `finally` blocks, and the 16-bit cases run in both modes through the `mode` fixture.  Device only
(16-bit storage has no CPU backend).  Until this file the only value tests of these kernels were the friendly shapes of tests/test_act16.py, forced
onto small problems with mmseg_conv16_mode 2.

Holes closed (numbers quoted by the ids): 1 the product's own dispatch (mode 1) on both sides of every threshold; 2 the pixel-major block order
(w_major == false) with more than one N tile, grids with nblk % 8 != 0; 3 conv16_kernel with stride 2, its raster form across samples, its 2-D tiles with
B = 3; 4 up-sampled x1 concatenated with x2 (the UNet decoder layer) on families 16 - 19; 5 the weight-gradient plans (ragged last block, sample
crossings, odd tpb > 3, S > 64 with and without accumulation, grids that xcd_remap mixes); 6 second and third trips of conv8h_kernel's walk;
7 the 16-bit instances of the register-staged kernels (families 1, 4, 6) at tile edges.

Launch arithmetic, recomputed from the launchers (and restated as code below: _fast_tile .. _tr_plan; M = B * Ho * Wo, K = KH * KW * Cin):

  conv16_tile             applicable: 16-bit inputs, C1 % 64 == C2 % 64 == 0, Cout % 8 == 0, at most 30 taps, no output mapping, y (and y2) 8-byte aligned
                          for 16-bit / 16-byte for fp32 stores, nsplit1 % 4 == 0; any stride and padding.  bn = 256 / 128 / 64 for Cout > 128 / > 64 / else,
                          mt = ceil(M / 256); mode 1 wants mt * ceil(Cout / bn) >= 192 and bn != 64; mode 2 takes everything applicable.  Code 16256<bn>.
  conv16_body             nblk = mt * ntn blocks through xcd_remap (the identity per XCD only when nblk % 8 == 0); w_major = K * Cout > M * Cin
                          (3x3: 9 * Cout > M; 1x1: Cout > M, i.e. never above 264 pixels; 5x5: 25 * Cout > M): w_major ? (mt = lb % ntm, n0 = lb / ntm) :
                          (mt = lb / ntn, n0 = lb % ntn).  tile2d (16 x 16 pixel tiles) when Wo % 16 == 0 and Ho % 16 == 0, else 256 raster pixels that may
                          cross rows and samples; rows >= M load nothing and store nothing.
  conv16h_tile / _rows    3x3 'same' stride 1 with W % 32 == 0, H % 8 == 0 and conv16_applicable (fp32: C % 32, Cout % 8, io == 0).  bn as above;
                          grid_ok(blocks) = mode 2 or (blocks >= 192 and blocks / (ceil(blocks / 256) * 256) >= 0.8): 205 .. 256 and 410 .. 512 pass, 192 .. 204
                          and 257 .. 409 do not (the first condition never decides: a fill of 0.8 needs 205 blocks).  bn 64: H % 16 == 0 and grid_ok(M / 512),
                          16 rows x 32 columns per block (code 17512064).  bn 128: 16 rows (17512128) where H % 16 == 0 and grid_ok(M / 512 * ntn), else 8 rows
                          (17256128) where grid_ok(M / 256 * ntn).  bn 256: 8 rows (17256256) where grid_ok(M / 256 * ntn).  fp32 and mode 1: Cout <= 32 excluded.
                          Block order as conv16_body with ntm = M / (32 TH); a block's sample is mt / tpi, tpi = (H / TH) * (W / 32), tpr = W / 32.
  wgrad32h_plan           fp32, 3x3 'same', W % 32 == 0, H % 2 == 0, channels % 32: <1,4> when Cout % 128 == 0, else <2,2> when Cout, C1, C2 % 64 == 0, else
                          <4,1> when C1, C2 % 128 == 0 -- so Cout is always a multiple of 32 nco: NO instance ever sees a partly filled output group (the issue
                          that asked for this file expected Cout = 160 on <1,4>; it runs on <4,1>, five full groups, or not at all).  ntiles = B * (H / 2) *
                          (W / 32), nbk = Cin / (32 nci) * Cout / (32 nco), S0 = max(1, min(ceil(256 / nbk), ntiles / 8)); mode 1 wants nbk * S0 >= 192;
                          tpb = ceil(ntiles / S0), S = ceil(ntiles / tpb); grid nbk * S through xcd_remap, block -> (channel blocks fastest, share s);
                          share s walks tiles [s tpb, min(ntiles, (s + 1) tpb)), double buffered by (t - t0) & 1.  Code 1800<nci>00<nco>.
  wgrad16h_plan           16-bit x and dy (io 5), W % 32 == 0, H % 8 == 0, C1, C2 % 64 == 0, Cout % 32 == 0 (Cout % 64 == 32: the waves of the last output
                          half plane idle).  ntiles = B * (H / 8) * (W / 32), nbk = Cin / 64 * ceil(Cout / 64), S0 = max(1, min(ceil(256 / nbk), ntiles / 2)),
                          the rest as above.  So tpb is 2 or 3 unless nbk caps S0: tpb = 5 needs S0 * nbk ~ 256 and ntiles = 5 S0, e.g. nbk 32, 40 tiles
                          (24 GFLOP for the oracle: it checks 32 of the 512 output channels there).  Code 19064064.
  workspace               mmseg_conv2d_wgrad_workspace covers both plans with Sh = min(512, B * (Ho / 2) * (Wo / 32) / 8) slabs (= ntiles16 / 2, and S <= 256):
                          a launch whose slabs did not fit would fall back to family 6 WITHOUT an error -- every direct case passes exactly that many floats
                          and asserts the code.  S slabs, plus ceil(S / 32) first-level sums behind them when S > 64; a single overwriting slab goes to dW.
  mmseg_conv8h_fwd_t      items = B * H * (W / 32) * ceil(Cout / 128), blocks = min(ceil(items / 4), 512); wave g = 4 block + wid keeps column group g % ntn
                          and walks segments g / ntn + i * nslots, nslots = (4 blocks + ntn - 1 - g % ntn) / ntn; the next segment's operands are requested
                          before the epilogue.  `if (blocks * 4 < ntn) blocks = (ntn + 3) / 4` cannot be taken: blocks * 4 >= min(items, 2048) >= ntn unless
                          Cout > 262144, so it has no case.  Code 20<x16 | 2 y16 | 4 relu>128.
  launch_fast             family 1 + 500000 for 16-bit inputs, + 250000 more where their K tiles are 64 channels deep (tile >= 128 x 64 and C % 64 == 0).
  launch_wgrad_tr         family 6 + 500000 with two inputs; tiles and S / chunk from wgrad_tr_splits (ported below operation for operation).
  launch_fast_batched     family 4: mmseg_conv2d_dgrad_parity_all takes fp32 tensors only (io = 0), so ops._Conv2d.backward cannot reach the IN16 instance
                          of conv_fast_batched_kernel in 16-bit storage (a 16-bit gradient does not pass the binding); the PREC 1 / 2 instances on fp32
                          tensors are what the 16-bit modes run, and what section 5 tests.

Every instantiation the dispatchers can select in the 16-bit modes (and on PREC 0 for families 17 and 18), and the case that reaches it (PREC 1 and 2:
the `mode` fixture):
  conv16_kernel     <256,256,2,4,2>   hole2-16-256-* (1x1, 5x5), hole3+4-16-256-raster-*, hole3-16-256-k4s2-*, epilogues 16-256-*; mode 1: hole1-64to192-B96
                    <256,128,4,2,3>   hole4-16-128-tile2d-*, hole3-16-128-*; mode 1: hole1-64to128-B204, -B96, hole1-1x1-64to128-B96
                    <256,64,4,1,3>    16-64-tile2d-B2-two-chunks, 16-64-raster-M720-Cout56 (mode 2 only: mode 1 never picks the 64-wide tile)
  conv16h_kernel    <256,2,4,2,P> (8 rows)             P 1, 2: hole2-17-256-*, 17-256-TH8-B2-*, hole4-17-256-*, epilogue 17-256-split196+68; P 0: *-prec0-* of the same
                    <128,4,2,3,P,1,16,1> (16 rows)     17-128-TH16-PB1-*, hole4-17-128-TH16-*; mode 1: hole1-64to128-B205; P 0: *-prec0-*, hole1-fp32-64to128
                    <128,4,2,3,P> (8 rows)             17-128-TH8-H%16=8-*; mode 1: hole1-64to128-B128; P 0: 17-128-TH8-prec0-*
                    <64,8,1,3,P,1,16,1>                17-64-TH16-PB1-*, hole4-17-64-*; mode 1: hole1-64to64-B205; P 0: 17-64-*-prec0-*, hole1-fp32-64to64
  wgrad32h_kernel   <1,4> <2,2> <4,1>                  hole5-18-* (each: ragged + crossing, S = 65), hole4-18-*; mode 1: hole1-18-*
  wgrad16h_kernel   <1> <2>                            hole5-19-*, hole4-19-*, 19-Cout96-*; mode 1: hole1-19-*
  conv8h_kernel     <P,4,X16,Y16,RELU>                 hole6-20-* (X16 and Y16 both ways in every case; RELU: the ntn1-items2049 case)
  conv_fast_kernel  <.,.,P,true,64> 128x128, 128x64    mode 1: hole1-64to192-B95 (128x128), hole1-64to128-B95 and hole1-64to64-B204 (128x64)
                    <.,.,P,true> and <.,.,P> (32-channel K tiles; 16-bit / fp32 tensors) 128x128, 128x64, 64x64, 128x32: hole7-1-*
  conv_fast_batched_kernel <.,.,P> 128x128, 128x64, 64x64, 128x32: hole7-4-* (fp32 tensors; <.,.,P,true>: unreachable, see launch_fast_batched above)
  conv_wgrad_tr_kernel <192|128, 128|64|32, P, TWO>    hole7-6-* (five tiles, one and two inputs, io 1, 4 and 5)

Where the issue's derivation did not hold (recomputed from the code): Cout = 160 on wgrad32h_kernel (above); the `blocks * 4 < ntn` branch of
mmseg_conv8h_fwd_t (unreachable, above); "an output row 8-byte but not 16-byte aligned when Cout * 2 % 16 == 8" -- these kernels want Cout % 8 == 0, so
whole outputs are offset by 8 bytes instead (_guarded) and the split output 196 + 68 gives y rows of 392 bytes; the 16-bit-storage form of family 4 (above).

Mutants (scratch copies of csrc/, one at a time, each run once on the device against this file; only changes of WHICH values are summed or stored inside
the same buffers -- every load of these kernels is a bounds-checked buffer load, no guard or store address was touched, stores are at most dropped) and the
tests that failed (F16 = test_forced_16bit_forward_kernels, F32 = test_forced_fp32_patch_resident_forward, EPI = ..._forward_epilogues, W19 / W18 =
test_forced_16bit / fp32_patch_resident_wgrad, C8 = test_conv_of_8_channels_beyond_one_trip, D = the test_mode1_dispatch_* tests; 16-bit cases: both modes):
  the w_major orders swapped for n0 only (both bodies)      F16 hole2-17-256-w_major0 (ntm 10 and 12), hole2-16-256-1x1 (both), hole4-17-256-TH8-ups64+128
      (w_major1, ntm 4); F32 hole2-17-256-prec0-w_major0, hole4-17-256-TH8-prec0; EPI both split196+68 cases.  The first version of the mirrored cases
      (w_major1 with ntm = 9 on family 17, ntm = 3 on family 16: ntm and ntn coprime) SURVIVED: lb -> (lb % ntm, lb % ntn) is then a bijection.  They now
      use ntm = 6; run again, all three fail as well: F16 hole2-17-256-w_major1-ntm6, hole2-16-256-5x5-w_major1-ntm6; F32 hole2-17-256-prec0-w_major1-ntm6
  the up-sampling parity bits dropped (conv16_body)         F16 hole3+4-16-256-raster-ups64+128, hole3-16-128-raster-5x5-ups, hole4-16-128-tile2d-ups128+64
  x2 chunks read at x1's resolution (16, 17, 18, 19)         every hole4 case of F16 (5), F32 (3), W19 (2 x 2) and W18 (2 x 2)
  the stage parity of the wgrad double buffer fixed to 0    every case of W19 and W18 (tpb >= 2 everywhere) and the two accepted D weight-gradient cases
  a tile's sample taken from the block's first tile (18, 19)  exactly the cases whose blocks cross a sample: W19 ntiles7-B7, ntiles40-tpb5; W18 the three
      ntiles21-tpb11 cases and hole4-18-2x2-ups64+64 (20 tiles per sample, tpb 8)
  the per-channel scale ignored by both epilogues            all four EPI cases
  a single trip in conv8h_kernel                            all three C8 cases
  the row wrap `if (yy >= H) yy -= H` of its walk dropped   C8 hole6-20-ntn1-items4097 only: in the two 2049-item cases the second trip lands on row 682 < H = 683, no wrap
  `accumulate` ignored by the reduction of families 18, 19  every accumulate case of W19 (9) and W18 (9), the accepted D weight-gradient cases (they accumulate)
  first-level group size 32 -> 16 in the reduction, S > 64  W19 ntiles130-S65 (both), ntiles512-S256; W18 the three ntiles520-S65 cases; overwrite and
      accumulate alike; the accepted D weight-gradient cases (S = 96)
  the stride ignored by conv16_body's gather                F16 the three hole3-16-*-k4s2 cases
  the thresholds 192 -> 128 (all four)                      D hole1-64to128-B95, hole1-1x1-64to128-B95, hole1-64to192-B95 (conv16_tile), hole1-19-...-nbk*S=190,
      hole1-18-...-nbk*S=190 (the plans).  The fourth, `blocks >= 192` of conv16h_grid_ok, survives by arithmetic: a fill of 0.8 needs 205 blocks
  the fill 0.8 -> 0.7                                       section 4 only: D hole1-64to128-B204 and hole1-64to64-B204 (204 / 256 = 0.797), hole1-64to128-B96 and
      hole1-64to192-B96 (192 / 256 = 0.75)
  conv16h_rows never 16                                     every 17-128-TH16 case of F16, F32 and EPI and the D cases of 64 -> 128 (the code field changes)
  fp32 Cout <= 32 no longer excluded in mode 1              D hole1-fp32-64to32-B205

Size: the largest case on the device is hole5-19-ntiles40-nbk32 (the only way to tpb = 5: a 94 MB workspace of 20 slabs of 9 x 256 x 512 floats, about
105 MB in all); the dispatch cases at B = 205 hold 54 MB of fp32 output + 17 MB of the mode-0 reference (run 64 samples at a time) + 13 MB of input.
No oracle pass costs more than 2 GFLOP: weight-gradient cases above that check every 2nd / 4th / ... output channel against the oracle (_co_subset) and
the whole tensor against mode 0.

Tolerances: those of tests/test_act16.py, all relative to the largest magnitude of the reference tensor.
  comparison                                          | tolerance | differs from the neighbour
  ----------------------------------------------------+-----------+---------------------------
  mode 2 / mode 1 vs mode 0, fp32 output              | 1e-5      | no (measured here at most 6.8e-7 forced, 1.0e-6 in the dispatch cases)
  16-bit outputs, mode 2 vs mode 0                    | 2^-7      | no (at most 2.2e-3)
  16-bit kernels vs the oracle on rounded operands    | 4e-4      | no (at most 6.2e-7 over all cases, the 16-tap stride-2 sums with K = 2048 included; mode 0: 4.0e-7)
  PREC 0 vs the oracle and vs mode 0                  | 5e-6      | no (at most 1.7e-6)
  weight gradients vs the oracle and vs mode 0        | 2e-5      | no (at most 9.9e-7 over all cases, the 256-slab reductions included; mode 0: 3.3e-7)
  conv8h_kernel vs the oracle                         | 2e-5      | no (at most 1.9e-7)
  bitwise: 16-bit output = rounding of the fp32 output of the same kernel; 16-bit storage = fp32 storage of the same mode; repeated weight gradient
  (none)                                              |           | no case needed another tolerance
"""
import functools

import pytest
import torch

from oracle import ops as O
from multimodal_segmentation_amd import ops as P
from multimodal_segmentation_amd import _native as N

pytestmark = pytest.mark.gpu
DEV = 'cuda'
NAN = float('nan')


# ======================================================================================================================
# the launch arithmetic of the header, as code: the tests assert the kernel code AND that these plans are the ones their ids state
# ======================================================================================================================
def _cdiv(a, b):
    return -(-a // b)


def _fast_tile(M, Cout):
    """conv_dispatch / launch_fast: tile of conv_fast_kernel"""
    tm = _cdiv(M, 128)
    if Cout > 64 and tm * _cdiv(Cout, 128) >= 384:
        return 128, 128
    if Cout > 32:
        return (128, 64) if tm * _cdiv(Cout, 64) >= 384 else (64, 64)
    return 128, 32


def _fast_code(M, Cout, C1, C2, in16):
    """family 1: + 500000 for the 16-bit-input instance, + 250000 more for its 64-channel K tiles"""
    bm, bn = _fast_tile(M, Cout)
    code = 1000000 + bm * 1000 + bn
    if in16:
        code += 500000
        if bm * bn >= 128 * 64 and C1 % 64 == 0 and C2 % 64 == 0:
            code += 250000
    return code


def _grid_ok(blocks, mode2):
    """conv16h_grid_ok"""
    return mode2 or (blocks >= 192 and blocks / (_cdiv(blocks, 256) * 256.0) >= 0.8)


def _plan17(B, H, W, Cout, mode2, fp32=False):
    """conv16h_tile + conv16h_rows for a 3x3 'same' layer whose channel counts fit: kernel code or 0"""
    if W % 32 or H % 8:
        return 0
    M = B * H * W
    bn = 256 if Cout > 128 else (128 if Cout > 64 else 64)
    ntn = _cdiv(Cout, bn)
    if not mode2 and fp32 and Cout <= 32:
        return 0
    if bn == 64:
        return 17512064 if H % 16 == 0 and _grid_ok(M // 512, mode2) else 0
    if bn == 128 and H % 16 == 0 and _grid_ok(M // 512 * ntn, mode2):
        return 17512128
    return 17256000 + bn if _grid_ok(M // 256 * ntn, mode2) else 0


def _plan16(M, Cout, mode2):
    """conv16_tile: kernel code or 0"""
    bn = 256 if Cout > 128 else (128 if Cout > 64 else 64)
    if not mode2 and (_cdiv(M, 256) * _cdiv(Cout, bn) < 192 or bn == 64):
        return 0
    return 16256000 + bn


def _plan_h(ntiles, nbk, min_tiles, mode2):
    """the common tail of wgrad32h_plan (min_tiles 8) and wgrad16h_plan (2): (S, tpb) or None"""
    S = min(_cdiv(256, nbk), ntiles // min_tiles)
    S = max(S, 1)
    if not mode2 and nbk * S < 192:
        return None
    tpb = _cdiv(ntiles, S)
    return _cdiv(ntiles, tpb), tpb


def _plan19(B, H, W, Cin, Cout, mode2=True):
    return _plan_h(B * (H // 8) * (W // 32), (Cin // 64) * _cdiv(Cout, 64), 2, mode2)


def _plan18(B, H, W, C1, C2, Cout, mode2=True):
    """-> (nci, S, tpb) or None"""
    if Cout % 128 == 0:
        nci = 1
    elif Cout % 64 == 0 and C1 % 64 == 0 and C2 % 64 == 0:
        nci = 2
    elif C1 % 128 == 0 and C2 % 128 == 0:
        nci = 4
    else:
        return None
    nco = 4 // nci
    pl = _plan_h(B * (H // 2) * (W // 32), ((C1 + C2) // (32 * nci)) * _cdiv(Cout, 32 * nco), 8, mode2)
    return None if pl is None else (nci,) + pl


def _tr_plan(M, K, Cout):
    """wgrad_tr_bkt / wgrad_tr_bnt / wgrad_tr_splits (the cost model, operation for operation): (K tile, N tile, S, chunk)"""
    bnt = 128 if Cout > 64 else (64 if Cout > 32 else 32)
    bkt = 192 if (K % 128 != 0 and K % 192 == 0 and Cout > 32) else 128
    bpc = 2 if bkt == 192 else (2 if bnt == 128 else (3 if bnt == 64 else 4))
    tiles = _cdiv(K, bkt) * _cdiv(Cout, bnt)
    cu_rate = 4.0 * 64.0 * 2.4e9
    eff = (0.0, 0.55, 0.75, 0.82, 0.85)
    maxS = max(1, min(M // 128, 4096))
    best, bestS, bestChunk = 1e30, 1, _cdiv(M, 32) * 32
    for S in range(1, maxS + 1):
        chunk = _cdiv(_cdiv(M, S), 32) * 32
        Se = _cdiv(M, chunk)
        if Se != S:
            continue
        blocks, slots = tiles * Se, 256 * bpc
        full, rem = divmod(blocks, slots)
        blk_flop = float(chunk) * bkt * bnt * 2.0
        t = full * (blk_flop * bpc / (cu_rate * eff[bpc]) + 3e-6)
        if rem:
            r = _cdiv(rem, 256)
            t += blk_flop * r / (cu_rate * eff[r]) + 3e-6
        t += float(Se) * K * Cout * 8.0 / 4.5e12 + 2e-6
        if t < best:
            best, bestS, bestChunk = t, Se, chunk
    return bkt, bnt, bestS, bestChunk


def _staged(S, KN, acc):
    """floats of the workspace a weight-gradient launch with S slabs writes: nothing for a single overwriting slab, else the slabs and, above
    64, the ceil(S / 32) first-level partial sums behind them"""
    return 0 if (S == 1 and not acc) else (S + (_cdiv(S, 32) if S > 64 else 0)) * KN


def _xcd_remap(orig, nwg):
    q, r, xcd = nwg >> 3, nwg & 7, orig & 7
    return (xcd * (q + 1) if xcd < r else r * (q + 1) + (xcd - r) * q) + (orig >> 3)


def _last():
    return N.call('mmseg_conv2d_last_kernel')


def rnd(*shape, seed=0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g)


@pytest.fixture(params=['bf16', 'fp16'])
def mode(request):
    prev = P.set_conv_precision(request.param)
    try:
        yield (torch.bfloat16 if request.param == 'bf16' else torch.float16)
    finally:
        P.set_conv_precision(prev)


def _geometry(H, W, k, stride, padding):
    return P._conv_geometry(H, W, k, k, stride, padding)


def _act(ref, act, alpha=0.2):
    return torch.relu(ref) if act == 1 else (O.leaky_relu(ref, alpha) if act == 2 else ref)


def _oracle_input(x1, x2, ups):
    a = x1.float().cpu().double()
    if ups:
        a = O.upsample2(a)
    if x2 is not None:
        a = torch.cat([a, x2.float().cpu().double()], -1)
    return a


def _guarded(shape, dtype):
    """a NaN-filled tensor of `shape` that starts 4 elements into a NaN-filled buffer (16 bytes for fp32; 8 bytes for a 16-bit type: rows of
    Cout % 8 == 0 channels are then 8-byte but not 16-byte aligned) and ends 4 elements before its end -> (buffer, view)"""
    n = 1
    for s in shape:
        n *= s
    buf = torch.full((n + 8,), NAN, device=DEV, dtype=dtype)
    v = buf[4:4 + n].view(shape)
    assert buf.data_ptr() % 16 == 0 and v.is_contiguous() and v.data_ptr() % 16 == (0 if dtype == torch.float32 else 8)
    return buf, v


def _guards_intact(buf):
    return bool(torch.isnan(buf[:4].float()).all() and torch.isnan(buf[-4:].float()).all())


def test_the_plans_of_the_header_are_what_the_ids_state():
    """the arithmetic the case ids quote, evaluated by the plan functions above (no device work)"""
    # conv16h_grid_ok: 205 .. 256 and 410 .. 512 pass, 192 .. 204 and 257 .. 409 do not
    assert [b for b in range(150, 520) if _grid_ok(b, False)] == list(range(205, 257)) + list(range(410, 513))
    # section 4, 64 -> 128 on 16 x 32 images
    assert [_plan17(B, 16, 32, 128, False) or _plan16(B * 512, 128, False) for B in (205, 204, 128, 96, 95)] == \
        [17512128, 16256128, 17256128, 16256128, 0]
    assert [_plan17(B, 16, 32, 64, False) or _plan16(B * 512, 64, False) for B in (205, 204)] == [17512064, 0]
    assert _plan17(205, 16, 32, 32, False, fp32=True) == 0 and _plan17(205, 16, 32, 32, True, fp32=True) == 17512064
    # weight gradients: nbk * S on both sides of 192
    assert _plan19(6, 64, 128, 64, 128, False) == (96, 2) and _plan19(19, 40, 64, 64, 128, False) is None
    assert _plan18(3, 128, 128, 64, 0, 128, False) == (1, 96, 8) and _plan18(5, 76, 128, 64, 0, 128, False) is None
    # xcd_remap is the identity inside an XCD only when the grid is a multiple of 8: with 20 blocks XCD 1 starts at logical id 3
    assert [_xcd_remap(i, 24) for i in (0, 1, 8, 9)] == [0, 3, 1, 4] and [_xcd_remap(i, 20) for i in (0, 1, 4, 5, 8)] == [0, 3, 12, 14, 1]


# ======================================================================================================================
# 1. forward, families 16 and 17 forced onto small problems (mmseg_conv16_mode 2)
# ======================================================================================================================
# B, H, W, C1, C2, Cout, k, stride, padding, ups, act | the mode-2 kernel code
FWD16 = [
    # ---- hole 2: block order with more than one N tile.  w_major = K * Cout > M * Cin, for 3x3: 9 * Cout > M ------------------------------------
    # family 17 <256, TH 8>: 264 channels = 2 N tiles (the second holds 8 channels: one 8-row weight piece), M = 2560 >= 2376 -> pixel-major,
    # ntm = 10, 20 blocks, 20 % 8 = 4: xcd_remap is not the identity
    pytest.param(10, 8, 32, 64, 0, 264, 3, 1, 'same', 0, 0, 17256256, id='hole2-17-256-w_major0-ntn2-ntm10-nblk20%8=4-Cout264'),
    pytest.param(12, 8, 32, 64, 0, 264, 3, 1, 'same', 0, 1, 17256256, id='hole2-17-256-w_major0-ntn2-ntm12-nblk24%8=0'),
    # the mirrored order (M = 1536 < 2376): ntm = 6 and ntn = 2 share a factor -- with coprime counts (ntm 9) lb -> (lb % ntm, lb % ntn) is itself a
    # bijection and a block that takes its N tile from the other order's formula still covers every tile once
    pytest.param(6, 8, 32, 64, 0, 264, 3, 1, 'same', 0, 2, 17256256, id='hole2-17-256-w_major1-ntn2-ntm6-nblk12%8=4-M1536<2376'),
    # family 16 <256,256>: 1x1 -> w_major needs Cout > M: never; 3 x 16 x 16: tile2d, ntm 3, 6 blocks; 1 x 24 x 40: raster, M = 960, ntm 4, 8 blocks, the
    # last tile holds 192 pixels; 5x5: 25 * 264 = 6600 > 1536 -> weight-major (ntm 6: see above)
    pytest.param(3, 16, 16, 64, 0, 264, 1, 1, 'same', 0, 0, 16256256, id='hole2-16-256-1x1-w_major0-ntn2-ntm3-nblk6-tile2d'),
    pytest.param(1, 24, 40, 128, 0, 264, 1, 1, 'same', 0, 2, 16256256, id='hole2-16-256-1x1-w_major0-ntn2-ntm4-nblk8-raster-M960'),
    pytest.param(6, 16, 16, 64, 0, 264, 5, 1, 'same', 0, 1, 16256256, id='hole2-16-256-5x5-w_major1-ntn2-ntm6-nblk12%8=4'),
    # ---- every family-17 instance with B > 1 (mt / tpi changes sample inside the grid) and tpr = W / 32 > 1 -------------------------------------
    pytest.param(2, 16, 64, 64, 0, 136, 3, 1, 'same', 0, 1, 17256256, id='17-256-TH8-B2-tpr2-tpi4-Cout136-partly-filled-weight-piece'),
    pytest.param(2, 32, 64, 128, 0, 72, 3, 1, 'same', 0, 0, 17512128, id='17-128-TH16-PB1-B2-tpr2-tpi4-Cout72-two-chunks'),
    pytest.param(2, 24, 64, 64, 0, 128, 3, 1, 'same', 0, 2, 17256128, id='17-128-TH8-H%16=8-B2-tpr2-tpi6'),
    pytest.param(3, 16, 64, 128, 0, 40, 3, 1, 'same', 0, 1, 17512064, id='17-64-TH16-PB1-B3-tpr2-tpi2-Cout40-patch-reloaded'),
    # ---- hole 4: the UNet decoder layer, up-sampled x1 (chunks at half resolution) then x2 (full resolution); the halo rows y = -1 and y = H map
    # through y >> 1 to -1 and H1 (out of range, masked by `ok`), x likewise ---------------------------------------------------------------------------
    pytest.param(2, 16, 32, 128, 64, 128, 3, 1, 'same', 1, 1, 17512128, id='hole4-17-128-TH16-ups128+64-H1=8-W1=16'),
    pytest.param(2, 8, 64, 64, 128, 264, 3, 1, 'same', 1, 0, 17256256, id='hole4-17-256-TH8-ups64+128-H1=4-W1=32-ntn2'),
    pytest.param(2, 16, 64, 64, 128, 64, 3, 1, 'same', 1, 2, 17512064, id='hole4-17-64-TH16-ups64+128-three-chunks'),
    pytest.param(2, 16, 16, 128, 64, 128, 3, 1, 'same', 1, 1, 16256128, id='hole4-16-128-tile2d-ups128+64'),
    # hole 3, raster form: Wo % 16 != 0, M = 720 = 2.8 tiles of 256, 240 pixels per sample: tiles 0 and 1 cross a sample boundary, the last holds 208;
    # up-sampled x1 with hb = ho - 1 and wb = wo - 1 of both parities
    pytest.param(3, 12, 20, 64, 128, 192, 3, 1, 'same', 1, 0, 16256256, id='hole3+4-16-256-raster-M720%256=208-crosses-samples-ups64+128'),
    pytest.param(3, 12, 20, 128, 0, 72, 5, 1, 'same', 1, 2, 16256128, id='hole3-16-128-raster-5x5-ups-odd-parities'),
    # ---- hole 3: family 16 tile2d with three samples; stride 2 (the discriminators' 4x4 'valid' layers) -------------------------------------------
    pytest.param(3, 16, 48, 64, 0, 128, 3, 1, 'same', 0, 1, 16256128, id='hole3-16-128-tile2d-B3-Ho16-Wo48-tpr3'),
    # 34 x 34 -> 16 x 16: tile2d, the last input column 33 is reached by tap kw = 3 of wo = 15 alone
    pytest.param(2, 34, 34, 64, 0, 128, 4, 2, 'valid', 0, 2, 16256128, id='hole3-16-128-k4s2-64to128-even-34x34-tile2d-last-column-one-tap'),
    # 35 x 33 -> 16 x 15: raster, M = 480; input row 34 is reached by no tap, column 32 by kw = 2 .. 3 of wo = 14 / 15 only
    pytest.param(2, 35, 33, 128, 0, 256, 4, 2, 'valid', 0, 2, 16256256, id='hole3-16-256-k4s2-128to256-odd-35x33-raster-M480'),
    pytest.param(1, 21, 37, 64, 0, 128, 4, 2, 'valid', 0, 0, 16256128, id='hole3-16-128-k4s2-64to128-odd-21x37-M153-one-tile'),
    # ---- the 64-wide tile of family 16 (4 waves; mode 1 never picks it) ------------------------------------------------------------------------------
    pytest.param(2, 16, 48, 128, 0, 64, 3, 1, 'same', 0, 1, 16256064, id='16-64-tile2d-B2-two-chunks'),
    pytest.param(3, 12, 20, 64, 0, 56, 3, 1, 'same', 0, 2, 16256064, id='16-64-raster-M720-Cout56-crosses-samples'),
]


@pytest.mark.parametrize('B,H,W,C1,C2,Cout,k,stride,padding,ups,act,code', FWD16)
def test_forced_16bit_forward_kernels(B, H, W, C1, C2, Cout, k, stride, padding, ups, act, code, mode):
    """conv16_kernel / conv16h_kernel (mode 2) against conv_fast_kernel's 16-bit instance (mode 0) on the same 16-bit operands, fp32 and 16-bit
    output, and against the fp64 oracle on the operands as the MFMA sees them"""
    Ho, Wo, ph, pw = _geometry(H, W, k, stride, padding)
    M = B * Ho * Wo
    if code // 1000000 == 17:
        assert _plan17(B, H, W, Cout, True) == code
    else:
        assert not (k == 3 and stride == 1 and _plan17(B, H, W, Cout, True)) and _plan16(M, Cout, True) == code
    H1, W1 = (H // 2, W // 2) if ups else (H, W)
    x1 = rnd(B, H1, W1, C1, seed=1).to(mode).to(DEV)
    x2 = rnd(B, H, W, C2, seed=2).to(mode).to(DEV) if C2 else None
    Cin = C1 + C2
    w = (rnd(k, k, Cin, Cout, seed=3) * (2.0 / (k * k * Cin)) ** 0.5).to(DEV)
    b = rnd(Cout, seed=4).to(DEV)
    wp = torch.empty(w.numel(), device=DEV)
    N.call('mmseg_conv2d_wprep', w, wp, k, k, Cin, Cout, 0)
    io_in = 1 | (2 if C2 else 0)
    prev = N.call('mmseg_conv16_mode', 0)
    try:
        outs = {}
        for m16 in (0, 2):
            N.call('mmseg_conv16_mode', m16)
            for out16 in (False, True):
                y = torch.full((B, Ho, Wo, Cout), NAN, device=DEV, dtype=mode if out16 else torch.float32)
                N.call('mmseg_conv2d_fwd_t', x1, x2, w, wp, b, y, None, B, H, W, C1, C2, Ho, Wo, Cout, k, k, stride, ph, pw, ups, 0, act, 0.2, 0,
                       io_in | (4 if out16 else 0))
                want = code if m16 == 2 else _fast_code(M, Cout, C1, C2, True)
                assert _last() == want, 'mode %d: launch went to kernel %d, not %d' % (m16, _last(), want)
                outs[(m16, out16)] = y
    finally:
        N.call('mmseg_conv16_mode', prev)
    ref = _act(O.conv2d(_oracle_input(x1, x2, ups), w.to(mode).float().cpu().double(), b.cpu().double(), stride=stride, padding=padding), act)
    scale = float(ref.abs().max())
    e2 = float((outs[(2, False)].cpu().double() - ref).abs().max()) / scale
    e0 = float((outs[(0, False)].cpu().double() - ref).abs().max()) / scale
    d32 = float((outs[(0, False)] - outs[(2, False)]).abs().max()) / scale
    d16 = float((outs[(0, True)].float() - outs[(2, True)].float()).abs().max()) / scale
    print('forced forward: oracle err mode 2 %.3e, mode 0 %.3e; mode 2 vs mode 0 fp32 %.3e, 16-bit %.3e' % (e2, e0, d32, d16))
    assert not torch.isnan(outs[(2, False)]).any() and not torch.isnan(outs[(2, True)].float()).any()
    assert d32 <= 1e-5
    assert d16 <= 2.0 ** -7
    assert torch.equal(outs[(2, True)], outs[(2, False)].to(mode)), 'a 16-bit output is the rounding of the fp32 output'
    assert e2 < 4e-4


# B, H, W, C1, C2, Cout, ups, act | code
FWD17_FP32 = [
    pytest.param(10, 8, 32, 32, 0, 264, 0, 0, 17256256, id='hole2-17-256-prec0-w_major0-ntn2-nblk20%8=4-Cin32'),
    pytest.param(6, 8, 32, 96, 0, 264, 0, 1, 17256256, id='hole2-17-256-prec0-w_major1-ntn2-ntm6-nblk12-Cin96-three-chunks'),
    pytest.param(2, 32, 64, 96, 0, 72, 0, 2, 17512128, id='17-128-TH16-PB1-prec0-B2-tpr2-Cin96-Cout72'),
    pytest.param(2, 24, 64, 32, 0, 136, 0, 1, 17256256, id='17-256-TH8-prec0-B2-tpr2-Cin32-Cout136'),
    pytest.param(2, 24, 64, 32, 0, 128, 0, 0, 17256128, id='17-128-TH8-prec0-H%16=8-B2-tpr2'),
    pytest.param(3, 16, 64, 96, 0, 40, 0, 2, 17512064, id='17-64-TH16-PB1-prec0-B3-tpr2-Cin96-Cout40'),
    pytest.param(2, 16, 32, 128, 64, 128, 1, 1, 17512128, id='hole4-17-128-TH16-prec0-ups128+64-six-chunks'),
    pytest.param(2, 8, 64, 64, 128, 264, 1, 0, 17256256, id='hole4-17-256-TH8-prec0-ups64+128-ntn2'),
    pytest.param(2, 16, 64, 32, 96, 32, 1, 2, 17512064, id='hole4-17-64-prec0-ups32+96-Cout32-taken-in-mode2-only'),
]


@pytest.mark.parametrize('B,H,W,C1,C2,Cout,ups,act,code', FWD17_FP32)
def test_forced_fp32_patch_resident_forward(B, H, W, C1, C2, Cout, ups, act, code):
    """conv16h_kernel<..., PREC 0, ...> (mode 2) against conv_fast_kernel (mode 0) and the fp64 oracle, fp32 throughout"""
    assert _plan17(B, H, W, Cout, True, fp32=True) == code
    prevp = P.set_conv_precision('fp32')
    prev = N.call('mmseg_conv16_mode', 0)
    try:
        H1, W1 = (H // 2, W // 2) if ups else (H, W)
        x1 = rnd(B, H1, W1, C1, seed=1).to(DEV)
        x2 = rnd(B, H, W, C2, seed=2).to(DEV) if C2 else None
        Cin, M = C1 + C2, B * H * W
        w = (rnd(3, 3, Cin, Cout, seed=3) * (2.0 / (9 * Cin)) ** 0.5).to(DEV)
        b = rnd(Cout, seed=4).to(DEV)
        wp = torch.empty(w.numel(), device=DEV)
        N.call('mmseg_conv2d_wprep', w, wp, 3, 3, Cin, Cout, 0)
        outs = {}
        for m16 in (0, 2):
            N.call('mmseg_conv16_mode', m16)
            y = torch.full((B, H, W, Cout), NAN, device=DEV)
            N.call('mmseg_conv2d_fwd', x1, x2, w, wp, b, y, None, B, H, W, C1, C2, H, W, Cout, 3, 3, 1, 1, 1, ups, 0, act, 0.2, 0)
            want = code if m16 == 2 else _fast_code(M, Cout, C1, C2, False)
            assert _last() == want, 'mode %d: launch went to kernel %d, not %d' % (m16, _last(), want)
            outs[m16] = y
    finally:
        N.call('mmseg_conv16_mode', prev)
        P.set_conv_precision(prevp)
    ref = _act(O.conv2d(_oracle_input(x1, x2, ups), w.cpu().double(), b.cpu().double()), act)
    scale = float(ref.abs().max())
    e2 = float((outs[2].cpu().double() - ref).abs().max()) / scale
    d = float((outs[2] - outs[0]).abs().max()) / scale
    print('forced fp32 forward: oracle err %.3e, mode 2 vs mode 0 %.3e' % (e2, d))
    assert not torch.isnan(outs[2]).any()
    assert e2 <= 5e-6
    assert d <= 5e-6


# B, H, W, C1, Cout, nsplit1, k | code
EPILOGUES = [
    # 264 channels on the 256-wide tile, split 196 + 68: the second N tile (channels 256 .. 263) stores into y2 at column 60, and the rows of y hold
    # 392 bytes in 16 bits: every other row is 8-byte but not 16-byte aligned even without the offset view
    pytest.param(2, 8, 32, 64, 264, 196, 3, 17256256, id='17-256-split196+68-tile-boundary-256-rows-392-bytes'),
    pytest.param(2, 16, 32, 64, 72, 36, 3, 17512128, id='17-128-TH16-split36+36-rows-72-bytes'),
    pytest.param(2, 12, 20, 64, 264, 196, 3, 16256256, id='16-256-raster-split196+68'),
    pytest.param(2, 16, 16, 128, 136, 128, 1, 16256256, id='16-256-tile2d-1x1-split128+8'),
]


@pytest.mark.parametrize('B,H,W,C1,Cout,nsplit1,k,code', EPILOGUES)
def test_forced_16bit_forward_epilogues(B, H, W, C1, Cout, nsplit1, k, code, mode):
    """the two-output store (y: channels [0, nsplit1), y2: the rest), the per-channel scale of the BatchNorm-folded inference convolution, and outputs
    that start 4 elements into their buffers -- 8-byte but not 16-byte aligned rows of a 16-bit y: the elements in front of and behind every output
    keep their NaN.  Mode 2 against mode 0 and the oracle."""
    x = rnd(B, H, W, C1, seed=1).to(mode).to(DEV)
    w = (rnd(k, k, C1, Cout, seed=3) * (2.0 / (k * k * C1)) ** 0.5).to(DEV)
    wp = torch.empty(w.numel(), device=DEV)
    N.call('mmseg_conv2d_wprep', w, wp, k, k, C1, Cout, 0)
    sc, sh = (rnd(Cout, seed=5) * 0.1 + 1).to(DEV), rnd(Cout, seed=6).to(DEV)
    p, M, n2 = k // 2, B * H * W, Cout - nsplit1
    prev = N.call('mmseg_conv16_mode', 0)
    try:
        res = {}
        for m16 in (0, 2):
            N.call('mmseg_conv16_mode', m16)
            want = code if m16 == 2 else _fast_code(M, Cout, C1, 0, True)
            for out16 in (False, True):
                dt = mode if out16 else torch.float32
                io = 1 | (4 if out16 else 0)
                b1, y1 = _guarded((B, H, W, nsplit1), dt)
                b2, y2 = _guarded((B, H, W, n2), dt)
                N.call('mmseg_conv2d_fwd_t', x, None, w, wp, None, y1, y2, B, H, W, C1, 0, H, W, Cout, k, k, 1, p, p, 0, 0, 0, 0.0, nsplit1, io)
                assert _last() == want, 'split, mode %d: kernel %d, not %d' % (m16, _last(), want)
                b3, ys = _guarded((B, H, W, Cout), dt)
                N.call('mmseg_conv2d_fwd_scaled_t', x, None, w, wp, sh, sc, ys, B, H, W, C1, 0, H, W, Cout, k, k, 1, p, p, 0, 1, 0.0, io)
                assert _last() == want, 'scaled, mode %d: kernel %d, not %d' % (m16, _last(), want)
                assert _guards_intact(b1) and _guards_intact(b2) and _guards_intact(b3), 'a store left its output (mode %d, out16 %s)' % (m16, out16)
                res[(m16, out16)] = (torch.cat([y1, y2], -1), ys)
    finally:
        N.call('mmseg_conv16_mode', prev)
    lin = O.conv2d(x.float().cpu().double(), w.to(mode).float().cpu().double(), None)
    refs = (lin, torch.relu(lin * sc.cpu().double() + sh.cpu().double()))
    for i, ref in enumerate(refs):
        scale = float(ref.abs().max())
        a32, c32, a16, c16 = res[(0, False)][i], res[(2, False)][i], res[(0, True)][i], res[(2, True)][i]
        assert not torch.isnan(c32).any() and not torch.isnan(c16.float()).any()
        assert float((a32 - c32).abs().max()) <= 1e-5 * scale
        assert float((a16.float() - c16.float()).abs().max()) <= 2.0 ** -7 * scale
        assert torch.equal(c16, c32.to(mode)), 'a 16-bit output is the rounding of the fp32 output'
        assert float((c32.cpu().double() - ref).abs().max()) < 4e-4 * scale


# ======================================================================================================================
# 2. weight gradients, families 18 and 19: direct calls in mode 2
# ======================================================================================================================
def _co_subset(M, Cin, Cout):
    """the output channels the oracle computes: all, or every 2nd / 4th / ... while a pass would cost more than 2 GFLOP"""
    step = 1
    while 2.0 * M * 9 * Cin * _cdiv(Cout, step) > 2.0e9:
        step *= 2
    return list(range(0, Cout, step))


@functools.lru_cache(maxsize=None)
def _wgrad_problem(B, H, W, C1, C2, Cout, ups, dtype):
    """operands (CPU; rounded to `dtype` when it is a 16-bit type) and the fp64 oracle's weight gradient on them, for the output channels `co`"""
    H1, W1 = (H // 2, W // 2) if ups else (H, W)
    x1 = rnd(B, H1, W1, C1, seed=1).to(dtype)
    x2 = rnd(B, H, W, C2, seed=2).to(dtype) if C2 else None
    dy = rnd(B, H, W, Cout, seed=3).to(dtype)
    base = rnd(3, 3, C1 + C2, Cout, seed=4) * 0.1
    co = _co_subset(B * H * W, C1 + C2, Cout)
    wref = torch.zeros(3, 3, C1 + C2, len(co), dtype=torch.float64, requires_grad=True)
    O.conv2d(_oracle_input(x1, x2, ups), wref, None).backward(dy.float().double()[..., co].contiguous())
    return x1, x2, dy, base, co, wref.grad


def _wgrad_direct(B, H, W, C1, C2, Cout, ups, acc, dtype, code, S):
    """one geometry on the patch-resident kernel (mode 2) and on conv_wgrad_tr_kernel (mode 0): NaN workspace of exactly
    mmseg_conv2d_wgrad_workspace floats, dW NaN or a non-zero base; the S slabs (+ first-level partial sums) are finite afterwards and everything
    behind them is NaN; values against the oracle and mode 0; a second launch is bitwise equal"""
    h16 = dtype != torch.float32
    x1c, x2c, dyc, basec, co, ref = _wgrad_problem(B, H, W, C1, C2, Cout, ups, dtype)
    x1, dy, base = x1c.to(DEV), dyc.to(DEV), basec.to(DEV)
    x2 = x2c.to(DEV) if C2 else None
    Cin = C1 + C2
    KN = 9 * Cin * Cout
    need = N.call('mmseg_conv2d_wgrad_workspace', B, H, W, Cin, Cout, 3, 3)
    staged = _staged(S, KN, acc)
    assert need >= max(staged, KN), 'mmseg_conv2d_wgrad_workspace (%d floats) does not hold the %d slabs of this plan' % (need, S)
    ws = torch.empty(need, device=DEV)

    def launch():
        ws.fill_(NAN)
        dw = base.clone() if acc else torch.full_like(base, NAN)
        if h16:
            N.call('mmseg_conv2d_wgrad_t', x1, x2, dy, dw.view(-1), ws, need, B, H, W, C1, C2, H, W, Cout, 3, 3, 1, 1, 1, ups, acc, 5)
        else:
            N.call('mmseg_conv2d_wgrad', x1, x2, dy, dw.view(-1), ws, need, B, H, W, C1, C2, H, W, Cout, 3, 3, 1, 1, 1, ups, acc)
        return dw

    prev = N.call('mmseg_conv16_mode', 0)
    try:
        d0 = launch()
        assert _last() // 1000000 == 6, 'mode 0: launch went to kernel %d' % _last()
        N.call('mmseg_conv16_mode', 2)
        outs = []
        for _ in range(2):
            outs.append(launch())
            assert _last() == code, 'launch went to kernel %d, not %d' % (_last(), code)
        nan = torch.isnan(ws)
        assert not nan[:staged].any(), 'a staged slab (or first-level partial sum) was not written'
        assert nan[staged:].all(), 'the launch wrote behind its %d slabs' % S
    finally:
        N.call('mmseg_conv16_mode', prev)
    want = ref + (basec.double()[..., co] if acc else 0.0)
    full_scale = float(d0.abs().max())
    scale = float(want.abs().max())
    err = float((outs[0].cpu().double()[..., co] - want).abs().max()) / scale
    err0 = float((d0.cpu().double()[..., co] - want).abs().max()) / scale
    d = float((outs[0] - d0).abs().max()) / full_scale
    print('forced wgrad: oracle err %.3e (mode 0: %.3e) on %d of %d output channels; mode 2 vs mode 0 %.3e' % (err, err0, len(co), Cout, d))
    assert not torch.isnan(outs[0]).any()
    assert err <= 2e-5
    assert d <= 2e-5
    assert torch.equal(outs[0], outs[1]), 'fixed tile order per block and a fixed-order slab reduction: bitwise reproducible'


# B, H, W, C1, C2, Cout, ups | S, tpb  (ntiles = B * (H / 8) * (W / 32) tiles of 8 x 32 pixels, nbk = Cin / 64 * ceil(Cout / 64) channel blocks,
# S0 = min(ceil(256 / nbk), ntiles / 2), tpb = ceil(ntiles / S0), S = ceil(ntiles / tpb), grid = nbk * S through xcd_remap)
WGRAD19 = [
    pytest.param(1, 40, 32, 64, 0, 64, 0, 2, 3, id='hole5-19-ntiles5-S2-tpb3-last-block-2-tiles'),
    pytest.param(7, 8, 32, 64, 0, 64, 0, 3, 3, id='hole5-19-ntiles7-B7-S3-tpb3-last-1-every-tile-another-sample'),
    # nbk = 4 * 8 = 32 -> S0 = 8, 40 tiles (8 per sample) -> tpb 5: odd and > 3; blocks 1, 3, 4, 6 cross a sample; grid 256
    pytest.param(5, 16, 128, 256, 0, 512, 0, 8, 5, id='hole5-19-ntiles40-nbk32-S8-tpb5-odd-crosses-samples'),
    # the first S above 64: 130 tiles, S0 = 65, tpb 2; two-level reduction over 32 + 32 + 1 slabs; grid 65 (65 % 8 = 1: xcd_remap mixes the shares)
    pytest.param(13, 80, 32, 64, 0, 64, 0, 65, 2, id='hole5-19-ntiles130-S65-groups-32-32-1-grid65%8=1'),
    # nbk = 3: S0 = min(86, 65) = 65 on 3 channel blocks: grid 195 (195 % 8 = 3), pixel shares of different XCD rounds interleave
    pytest.param(13, 80, 32, 64, 0, 160, 0, 65, 2, id='hole5-19-ntiles130-nbk3-Cout160-S65-grid195%8=3-idle-half-plane'),
    pytest.param(16, 64, 128, 64, 0, 64, 0, 256, 2, id='hole5-19-ntiles512-S256-eight-groups-of-32'),
    pytest.param(2, 16, 32, 64, 0, 96, 0, 2, 2, id='19-Cout96-idle-half-plane-nbk2-S2-grid4'),
    pytest.param(3, 24, 64, 64, 64, 64, 1, 9, 2, id='hole4-19-ups64+64-ntiles18-nbk2-S9-grid18%8=2'),
    pytest.param(1, 40, 64, 128, 64, 96, 1, 5, 2, id='hole4-19-ups128+64-Cout96-ntiles10-nbk6-S5-grid30%8=6'),
]


@pytest.mark.parametrize('acc', [0, 1], ids=['overwrite', 'accumulate'])
@pytest.mark.parametrize('B,H,W,C1,C2,Cout,ups,S,tpb', WGRAD19)
def test_forced_16bit_patch_resident_wgrad(B, H, W, C1, C2, Cout, ups, S, tpb, acc, mode):
    assert _plan19(B, H, W, C1 + C2, Cout) == (S, tpb)
    _wgrad_direct(B, H, W, C1, C2, Cout, ups, acc, mode, 19064064, S)


# B, H, W, C1, C2, Cout, ups | nci, S, tpb  (ntiles = B * (H / 2) * (W / 32) tiles of 2 x 32 pixels, nbk = Cin / (32 nci) * Cout / (32 nco),
# S0 = min(ceil(256 / nbk), ntiles / 8), tpb = ceil(ntiles / S0), S = ceil(ntiles / tpb))
WGRAD18 = [
    # 21 tiles, 7 per sample: S0 = 2, tpb 11 (odd, > 3), block 0 walks tiles 0 .. 10 across samples 0 -> 1, block 1 the remaining 10 (ragged)
    pytest.param(3, 14, 32, 32, 0, 128, 0, 1, 2, 11, id='hole5-18-1x4-ntiles21-S2-tpb11-odd-last10-crosses-samples'),
    pytest.param(3, 14, 32, 64, 0, 64, 0, 2, 2, 11, id='hole5-18-2x2-ntiles21-S2-tpb11-odd-last10-crosses-samples'),
    pytest.param(3, 14, 32, 128, 0, 32, 0, 4, 2, 11, id='hole5-18-4x1-ntiles21-S2-tpb11-odd-last10-crosses-samples'),
    # Cout = 160 is neither a multiple of 128 nor of 64: only <4,1> takes it (five 32-channel output blocks; no instance ever sees a partly
    # filled output group: the plan wants Cout % (32 nco) == 0); nbk = 5, 36 tiles, S0 = 4, tpb 9, grid 20 (20 % 8 = 4)
    pytest.param(2, 36, 32, 128, 0, 160, 0, 4, 4, 9, id='hole5-18-4x1-Cout160-nbk5-ntiles36-S4-tpb9-grid20%8=4'),
    # S > 64 needs ntiles / 8 > 64: 520 tiles, S0 = 65, tpb 8, 65 slabs (32 + 32 + 1), grid 65
    pytest.param(13, 80, 32, 32, 0, 128, 0, 1, 65, 8, id='hole5-18-1x4-ntiles520-S65-groups-32-32-1-grid65%8=1'),
    pytest.param(13, 80, 32, 64, 0, 64, 0, 2, 65, 8, id='hole5-18-2x2-ntiles520-S65-groups-32-32-1-grid65%8=1'),
    pytest.param(13, 80, 32, 128, 0, 32, 0, 4, 65, 8, id='hole5-18-4x1-ntiles520-S65-groups-32-32-1-grid65%8=1'),
    # the decoder layer: planes walk x1 at half resolution, then x2
    pytest.param(2, 20, 64, 64, 64, 64, 1, 2, 5, 8, id='hole4-18-2x2-ups64+64-ntiles40-nbk2-S5-tpb8-grid10%8=2'),
    pytest.param(2, 20, 32, 32, 96, 128, 1, 1, 2, 10, id='hole4-18-1x4-ups32+96-ntiles20-nbk4-S2-tpb10'),
]


@pytest.mark.parametrize('acc', [0, 1], ids=['overwrite', 'accumulate'])
@pytest.mark.parametrize('B,H,W,C1,C2,Cout,ups,nci,S,tpb', WGRAD18)
def test_forced_fp32_patch_resident_wgrad(B, H, W, C1, C2, Cout, ups, nci, S, tpb, acc):
    assert _plan18(B, H, W, C1, C2, Cout) == (nci, S, tpb)
    prevp = P.set_conv_precision('fp32')
    try:
        _wgrad_direct(B, H, W, C1, C2, Cout, ups, acc, torch.float32, 18000000 + nci * 1000 + 4 // nci, S)
    finally:
        P.set_conv_precision(prevp)


# ======================================================================================================================
# 3. conv8h_kernel: second and third trips of the grid-stride walk
# ======================================================================================================================
@functools.lru_cache(maxsize=None)
def _conv8h_problem(B, H, W, Cout, act, dtype):
    x = rnd(B, H, W, 8, seed=1).to(dtype)
    w = rnd(3, 3, 8, Cout, seed=2) * (2.0 / 72) ** 0.5
    b = rnd(Cout, seed=3)
    ref = _act(O.conv2d(x.float().double(), w.to(dtype).float().double(), b.double()), act)
    return x, w, b, ref


# B, H, W, Cout, act | items = B * H * (W / 32) * ceil(Cout / 128) on min(ceil(items / 4), 512) blocks = at most 2048 waves; a wave keeps the column
# group nt = wave % ntn and walks the row segments wslot, wslot + nslots, ... with wslot = wave / ntn, nslots = (2048 + ntn - 1 - nt) / ntn
CONV8H = [
    # 683 segments x 3 groups = 2049 items: groups 0 and 1 have 683 slots, group 2 has 682 -> its slot 0 (wave 2) walks segments 0 and 682, alone
    pytest.param(1, 683, 32, 320, 2, id='hole6-20-ntn3-items2049-first-above-2048-one-wave-walks-twice'),
    # 2049 segments, one group: wave 0 takes segments 0 and 2048; the second trip starts in sample 2
    pytest.param(3, 683, 32, 128, 1, id='hole6-20-ntn1-items2049-wave0-walks-twice'),
    # 4097 segments: wave 0 walks three times, every other wave twice; 40 channels: Cout % 8 == 0 only, 88 masked columns
    pytest.param(17, 241, 32, 40, 0, id='hole6-20-ntn1-items4097-third-trip-Cout40'),
]


@pytest.mark.parametrize('B,H,W,Cout,act', CONV8H)
def test_conv_of_8_channels_beyond_one_trip(B, H, W, Cout, act, mode):
    """fp32 and 16-bit input, fp32 and 16-bit output, against the oracle on the whole tensor (at most 1.2 GFLOP); bitwise against launches of the
    same data in pieces of at most 2048 items -- a wave's sums for a pixel do not depend on where in its walk the pixel comes"""
    xc, wc, bc, ref = _conv8h_problem(B, H, W, Cout, act, mode)
    ntn = _cdiv(Cout, 128)
    assert B * H * (W // 32) * ntn > 2048
    w, b = wc.to(DEV), bc.to(DEV)
    hm = 1 if mode == torch.bfloat16 else 2
    scale = float(ref.abs().max())
    for x16 in (False, True):
        xd = (xc if x16 else xc.float()).to(DEV)
        ys = {}
        for out16 in (False, True):
            buf, y = _guarded((B, H, W, Cout), mode if out16 else torch.float32)
            N.call('mmseg_conv8h_fwd_t', xd, w, b, y, B, H, W, Cout, act, 0.2, hm if x16 else 0, hm if out16 else 0)
            want = 20000128 + 1000 * ((1 if x16 else 0) | (2 if out16 else 0) | (4 if act == 1 else 0))
            assert _last() == want, 'launch went to kernel %d, not %d' % (_last(), want)
            assert _guards_intact(buf)
            ys[out16] = y
        assert not torch.isnan(ys[False]).any(), 'pixels of a later trip were not written'
        assert torch.equal(ys[True], ys[False].to(mode)), 'a 16-bit output is the rounding of the fp32 output'
        err = float((ys[False].cpu().double() - ref).abs().max()) / scale
        print('conv8h x16=%s: oracle err %.3e' % (x16, err))
        assert err < 2e-5
        # the same data in single-trip launches: per sample, or (one sample) two overlapping row ranges compared away from the cut
        if B > 1:
            assert H * (W // 32) * ntn <= 2048
            parts = torch.empty_like(ys[False])
            for s in range(B):
                N.call('mmseg_conv8h_fwd_t', xd[s:s + 1], w, b, parts[s:s + 1], 1, H, W, Cout, act, 0.2, hm if x16 else 0, 0)
            assert torch.equal(parts, ys[False])
        else:
            h0 = H // 2 + 1
            assert h0 * (W // 32) * ntn <= 2048
            top, bot = torch.empty(1, h0, W, Cout, device=DEV), torch.empty(1, h0, W, Cout, device=DEV)
            N.call('mmseg_conv8h_fwd_t', xd[:, :h0].contiguous(), w, b, top, 1, h0, W, Cout, act, 0.2, hm if x16 else 0, 0)
            N.call('mmseg_conv8h_fwd_t', xd[:, H - h0:].contiguous(), w, b, bot, 1, h0, W, Cout, act, 0.2, hm if x16 else 0, 0)
            assert torch.equal(top[:, :h0 - 1], ys[False][:, :h0 - 1]) and torch.equal(bot[:, 1:], ys[False][:, H - h0 + 1:])


# ======================================================================================================================
# 4. the product's own dispatch (mode 1) on both sides of every threshold
# ======================================================================================================================
def _dispatch_forward(B, H, W, Cin, Cout, k, dtype, want1, want2):
    """mode 1 takes kernel `want1`, mode 2 `want2` (0: the layer stays on conv_fast_kernel); every output is written; values against mode 0, run
    on at most 64 samples at a time (the whole batch twice in fp32 would not fit the size limit)"""
    h16 = dtype != torch.float32
    x = rnd(B, H, W, Cin, seed=1).to(dtype).to(DEV)
    w = (rnd(k, k, Cin, Cout, seed=3) * (2.0 / (k * k * Cin)) ** 0.5).to(DEV)
    b = rnd(Cout, seed=4).to(DEV)
    wp = torch.empty(w.numel(), device=DEV)
    N.call('mmseg_conv2d_wprep', w, wp, k, k, Cin, Cout, 0)
    p = k // 2

    def launch(xs, y):
        n = xs.shape[0]
        if h16:
            N.call('mmseg_conv2d_fwd_t', xs, None, w, wp, b, y, None, n, H, W, Cin, 0, H, W, Cout, k, k, 1, p, p, 0, 0, 1, 0.0, 0, 1)
        else:
            N.call('mmseg_conv2d_fwd', xs, None, w, wp, b, y, None, n, H, W, Cin, 0, H, W, Cout, k, k, 1, p, p, 0, 0, 1, 0.0, 0)
        return _last()

    fast = _fast_code(B * H * W, Cout, Cin, 0, h16)
    prev = N.call('mmseg_conv16_mode', 1)
    try:
        y = torch.full((B, H, W, Cout), NAN, device=DEV)
        got = launch(x, y)
        assert got == (want1 or fast), 'mode 1: launch went to kernel %d, not %d' % (got, want1 or fast)
        assert not torch.isnan(y).any()
        N.call('mmseg_conv16_mode', 0)
        worst, scale = 0.0, float(y.abs().max())
        for s in range(0, B, 64):
            y0 = torch.full((min(64, B - s), H, W, Cout), NAN, device=DEV)
            assert launch(x[s:s + 64], y0) // 1000000 == 1
            worst = max(worst, float((y[s:s + 64] - y0).abs().max()))
        del y0
        N.call('mmseg_conv16_mode', 2)
        got = launch(x[:1], torch.empty(1, H, W, Cout, device=DEV))
        assert got == (want2 or _fast_code(H * W, Cout, Cin, 0, h16)), 'mode 2: launch went to kernel %d' % got
    finally:
        N.call('mmseg_conv16_mode', prev)
    print('dispatch forward: mode 1 vs mode 0 %.3e of the largest magnitude' % (worst / scale))
    assert worst <= (1e-5 if h16 else 5e-6) * scale


# B, Cout, k | mode-1 kernel (0 = conv_fast_kernel), mode-2 kernel; 64 input channels, 16 x 32 images: M = 512 B
DISPATCH16 = [
    pytest.param(205, 128, 3, 17512128, 17512128, id='hole1-64to128-B205-205-blocks-of-512-fill-0.801-17-16rows'),
    pytest.param(204, 128, 3, 16256128, 17512128, id='hole1-64to128-B204-204-and-408-blocks-fail-the-fill-16-at-mt408'),
    pytest.param(128, 128, 3, 17256128, 17512128, id='hole1-64to128-B128-128-blocks-too-few-256-of-256-pixels-17-8rows'),
    pytest.param(96, 128, 3, 16256128, 17512128, id='hole1-64to128-B96-192-blocks-fill-0.75-17-refused-16-at-mt192'),
    pytest.param(95, 128, 3, 0, 17512128, id='hole1-64to128-B95-mt190-below-192-conv_fast'),
    pytest.param(96, 128, 1, 16256128, 16256128, id='hole1-1x1-64to128-B96-mt192-16'),
    pytest.param(95, 128, 1, 0, 16256128, id='hole1-1x1-64to128-B95-mt190-one-sample-fewer-conv_fast'),
    pytest.param(205, 64, 3, 17512064, 17512064, id='hole1-64to64-B205-205-blocks-17-64'),
    pytest.param(204, 64, 3, 0, 17512064, id='hole1-64to64-B204-fill-fails-conv_fast-never-16'),
    # 192 channels: one 256-wide N tile; 192 blocks fail the fill -> conv16_kernel<256,256> at mt = 192; one sample fewer -> conv_fast_kernel
    # <128,128> with 64-channel K tiles (tiles_big = 380 * 2)
    pytest.param(96, 192, 3, 16256256, 17256256, id='hole1-64to192-B96-192-blocks-fill-0.75-16-256-at-mt192'),
    pytest.param(95, 192, 3, 0, 17256256, id='hole1-64to192-B95-mt190-conv_fast-128x128-k64'),
]


@pytest.mark.parametrize('B,Cout,k,want1,want2', DISPATCH16)
def test_mode1_dispatch_of_the_16bit_forward_kernels(B, Cout, k, want1, want2, mode):
    H, W = 16, 32
    plan = lambda m2: (_plan17(B if not m2 else 1, H, W, Cout, m2) if k == 3 else 0) or _plan16((B if not m2 else 1) * H * W, Cout, m2)
    assert plan(False) == want1 and plan(True) == want2
    _dispatch_forward(B, H, W, 64, Cout, k, mode, want1, want2)


@pytest.mark.parametrize('Cout,want1,want2', [pytest.param(32, 0, 17512064, id='hole1-fp32-64to32-B205-Cout32-excluded-in-mode1'),
                                              pytest.param(64, 17512064, 17512064, id='hole1-fp32-64to64-B205-17-64-prec0'),
                                              pytest.param(128, 17512128, 17512128, id='hole1-fp32-64to128-B205-17-128-16rows-prec0')])
def test_mode1_dispatch_of_the_fp32_patch_resident_kernel(Cout, want1, want2):
    assert _plan17(205, 16, 32, Cout, False, fp32=True) == want1 and _plan17(1, 16, 32, Cout, True, fp32=True) == want2
    prevp = P.set_conv_precision('fp32')
    try:
        _dispatch_forward(205, 16, 32, 64, Cout, 3, torch.float32, want1, want2)
    finally:
        P.set_conv_precision(prevp)


def _dispatch_wgrad(B, H, W, Cin, Cout, dtype, want1):
    """mode 1 -> `want1`; values against mode 0 (conv_wgrad_tr_kernel <192,128>), accumulating into a non-zero dW; a second launch bitwise equal"""
    h16 = dtype != torch.float32
    x = rnd(B, H, W, Cin, seed=1).to(dtype).to(DEV)
    dy = rnd(B, H, W, Cout, seed=3).to(dtype).to(DEV)
    base = (rnd(3, 3, Cin, Cout, seed=4) * 0.1).to(DEV)
    need = N.call('mmseg_conv2d_wgrad_workspace', B, H, W, Cin, Cout, 3, 3)
    ws = torch.empty(need, device=DEV)

    def launch():
        ws.fill_(NAN)
        dw = base.clone()
        if h16:
            N.call('mmseg_conv2d_wgrad_t', x, None, dy, dw.view(-1), ws, need, B, H, W, Cin, 0, H, W, Cout, 3, 3, 1, 1, 1, 0, 1, 5)
        else:
            N.call('mmseg_conv2d_wgrad', x, None, dy, dw.view(-1), ws, need, B, H, W, Cin, 0, H, W, Cout, 3, 3, 1, 1, 1, 0, 1)
        return dw, _last()

    prev = N.call('mmseg_conv16_mode', 1)
    try:
        d1, got = launch()
        assert got == want1, 'mode 1: launch went to kernel %d, not %d' % (got, want1)
        d1b, _ = launch()
        N.call('mmseg_conv16_mode', 0)
        d0, got0 = launch()
        assert got0 == 6192128
    finally:
        N.call('mmseg_conv16_mode', prev)
    assert not torch.isnan(d1).any() and torch.equal(d1, d1b)
    diff = float((d1 - d0).abs().max()) / float(d0.abs().max())
    print('dispatch wgrad: mode 1 vs mode 0 %.3e' % diff)
    assert diff <= 2e-5


@pytest.mark.parametrize('B,H,W,want1', [pytest.param(6, 64, 128, 19064064, id='hole1-19-64to128-ntiles192-nbk2-S96-nbk*S=192'),
                                         pytest.param(19, 40, 64, 6192128, id='hole1-19-64to128-ntiles190-nbk2-S95-nbk*S=190-refused')])
def test_mode1_dispatch_of_the_16bit_patch_resident_wgrad(B, H, W, want1, mode):
    assert (_plan19(B, H, W, 64, 128, False) is not None) == (want1 == 19064064)
    _dispatch_wgrad(B, H, W, 64, 128, mode, want1)


@pytest.mark.parametrize('B,H,W,want1', [pytest.param(3, 128, 128, 18001004, id='hole1-18-64to128-3x128x128-ntiles768-S96-nbk*S=192'),
                                         pytest.param(5, 76, 128, 6192128, id='hole1-18-64to128-5x76x128-ntiles760-S95-nbk*S=190-refused')])
def test_mode1_dispatch_of_the_fp32_patch_resident_wgrad(B, H, W, want1):
    assert (_plan18(B, H, W, 64, 0, 128, False) is not None) == (want1 == 18001004)
    prevp = P.set_conv_precision('fp32')
    try:
        _dispatch_wgrad(B, H, W, 64, 128, torch.float32, want1)
    finally:
        P.set_conv_precision(prevp)


# ======================================================================================================================
# 5. the 16-bit instances of the register-staged kernels (families 1, 4, 6) at their tile edges, default mode 1
# ======================================================================================================================
# B, H, W, C1, C2, Cout, k, ups, act | conv_fast_kernel tile.  Channel counts are multiples of 32 but not of 64: conv16_applicable refuses them in
# every mode, and the 16-bit-input instance keeps its 32-channel K tiles (code + 500000, never + 250000)
FAST16 = [
    # M = 24640 = 192.5 tiles of 128 (the last holds 64 rows); 132 channels: 2 N tiles, the second holds 4; tiles_big = 193 * 2 = 386
    pytest.param(2, 280, 44, 32, 0, 132, 3, 0, 2, 128128, id='hole7-1-128x128-M24640%128=64-Cout132%4-Wo44-tiles_big386'),
    # tiles_big = 193 < 384, tiles_mid = 193 * 2 = 386
    pytest.param(2, 280, 44, 32, 0, 72, 3, 0, 1, 128064, id='hole7-1-128x64-M24640%128=64-Cout72-tiles_mid386'),
    pytest.param(2, 13, 20, 32, 96, 40, 3, 0, 0, 64064, id='hole7-1-64x64-32+96-M520%64=8-Cout40-Wo20'),
    pytest.param(2, 12, 20, 32, 96, 68, 3, 1, 2, 64064, id='hole7-1-64x64-ups32+96-Cout68%4-second-N-tile-4-columns'),
    pytest.param(3, 17, 12, 96, 0, 24, 3, 0, 1, 128032, id='hole7-1-128x32-Cin96-M612%128=100-Cout24'),
    pytest.param(3, 17, 12, 32, 0, 12, 1, 0, 0, 128032, id='hole7-1-128x32-1x1-Cin32-Cout12%4'),
]


@pytest.mark.parametrize('B,H,W,C1,C2,Cout,k,ups,act,tile', FAST16)
def test_register_staged_forward_with_16bit_tensors_at_tile_edges(B, H, W, C1, C2, Cout, k, ups, act, tile, mode):
    """every input / output storage combination of conv_fast_kernel's 16-bit instances: bitwise the fp32-storage call of the same precision mode
    on representable inputs (a 16-bit output: its rounding), and the oracle on the rounded operands.  A 16-bit output wants Cout % 8 == 0."""
    M, p = B * H * W, k // 2
    assert _fast_tile(M, Cout) == (tile // 1000, tile % 1000)
    H1, W1 = (H // 2, W // 2) if ups else (H, W)
    x1 = rnd(B, H1, W1, C1, seed=1).to(mode).to(DEV)
    x2 = rnd(B, H, W, C2, seed=2).to(mode).to(DEV) if C2 else None
    Cin = C1 + C2
    w = (rnd(k, k, Cin, Cout, seed=3) * (2.0 / (k * k * Cin)) ** 0.5).to(DEV)
    b = rnd(Cout, seed=4).to(DEV)
    wp = torch.empty(w.numel(), device=DEV)
    N.call('mmseg_conv2d_wprep', w, wp, k, k, Cin, Cout, 0)
    prev = N.call('mmseg_conv16_mode', 1)
    try:
        y32 = torch.full((B, H, W, Cout), NAN, device=DEV)
        N.call('mmseg_conv2d_fwd', x1.float(), x2.float() if C2 else None, w, wp, b, y32, None, B, H, W, C1, C2, H, W, Cout, k, k, 1, p, p, ups, 0,
               act, 0.2, 0)
        assert _last() == 1000000 + tile
        for in16 in (True, False):
            for out16 in ((False, True) if Cout % 8 == 0 else (False,)):
                buf, y = _guarded((B, H, W, Cout), mode if out16 else torch.float32)
                a1 = x1 if in16 else x1.float()
                a2 = (x2 if in16 else x2.float()) if C2 else None
                io = ((1 | (2 if C2 else 0)) if in16 else 0) | (4 if out16 else 0)
                N.call('mmseg_conv2d_fwd_t', a1, a2, w, wp, b, y, None, B, H, W, C1, C2, H, W, Cout, k, k, 1, p, p, ups, 0, act, 0.2, 0, io)
                want = 1000000 + tile + (500000 if in16 else 0)
                assert _last() == want, 'in16=%s out16=%s: kernel %d, not %d' % (in16, out16, _last(), want)
                assert _guards_intact(buf)
                assert torch.equal(y, y32.to(mode) if out16 else y32), 'in16=%s out16=%s' % (in16, out16)
    finally:
        N.call('mmseg_conv16_mode', prev)
    ref = _act(O.conv2d(_oracle_input(x1, x2, ups), w.to(mode).float().cpu().double(), b.cpu().double()), act)
    err = float((y32.cpu().double() - ref).abs().max()) / float(ref.abs().max())
    print('register-staged forward: oracle err %.3e' % err)
    assert not torch.isnan(y32).any() and err < 4e-4


# B, H, W, C1, C2, Cout, ups | K tile, N tile, S, chunk (wgrad_tr_splits); W % 4 == 0 but W % 32 != 0: families 18 / 19 cannot take them
TR16 = [
    pytest.param(2, 18, 20, 64, 0, 136, 0, 192, 128, 5, 160, id='hole7-6-192x128-M720-S5-chunk160-last80-Cout136'),
    pytest.param(2, 18, 20, 32, 32, 72, 0, 192, 128, 5, 160, id='hole7-6-192x128-two-inputs-32+32-Cout72-S5-last80'),
    pytest.param(1, 22, 36, 64, 0, 40, 0, 192, 64, 5, 160, id='hole7-6-192x64-M792-S5-chunk160-last152-Cout40'),
    pytest.param(1, 22, 36, 32, 32, 64, 0, 192, 64, 5, 160, id='hole7-6-192x64-two-inputs-S5-last152'),
    pytest.param(2, 22, 12, 96, 0, 72, 0, 128, 128, 4, 160, id='hole7-6-128x128-Cin96-M528-S4-chunk160-last48'),
    pytest.param(2, 22, 12, 32, 96, 136, 1, 128, 128, 4, 160, id='hole7-6-128x128-ups32+96-Cout136-S4-last48'),
    pytest.param(2, 22, 12, 96, 0, 40, 0, 128, 64, 4, 160, id='hole7-6-128x64-Cin96-Cout40-S4-last48'),
    pytest.param(2, 22, 12, 32, 96, 64, 1, 128, 64, 4, 160, id='hole7-6-128x64-ups32+96-S4-last48'),
    pytest.param(2, 22, 12, 96, 0, 24, 0, 128, 32, 4, 160, id='hole7-6-128x32-Cin96-Cout24-S4-last48'),
    pytest.param(2, 22, 12, 32, 96, 8, 0, 128, 32, 4, 160, id='hole7-6-128x32-two-inputs-32+96-Cout8-S4-last48'),
]


@pytest.mark.parametrize('acc', [0, 1], ids=['overwrite', 'accumulate'])
@pytest.mark.parametrize('B,H,W,C1,C2,Cout,ups,bkt,bnt,S,chunk', TR16)
def test_register_staged_wgrad_with_16bit_tensors_at_tile_edges(B, H, W, C1, C2, Cout, ups, bkt, bnt, S, chunk, acc, mode):
    """conv_wgrad_tr_kernel's 16-bit instances with 16-bit x (io 1), 16-bit dy (io 4) and both (io 5): bitwise the fp32-storage call of the same
    precision mode on representable operands; the fp64 oracle on the rounded operands; S slabs staged, nothing behind them"""
    Cin, M = C1 + C2, B * H * W
    K = 9 * Cin
    KN = K * Cout
    assert _tr_plan(M, K, Cout) == (bkt, bnt, S, chunk) and (S - 1) * chunk < M < S * chunk, 'the last slab is shorter than the chunk'
    x1c, x2c, dyc, basec, co, ref = _wgrad_problem(B, H, W, C1, C2, Cout, ups, mode)
    assert len(co) == Cout
    x1, dy, base = x1c.to(DEV), dyc.to(DEV), basec.to(DEV)
    x2 = x2c.to(DEV) if C2 else None
    need = N.call('mmseg_conv2d_wgrad_workspace', B, H, W, Cin, Cout, 3, 3)
    staged = _staged(S, KN, acc)
    assert need >= max(staged, KN)
    code = 6000000 + (500000 if C2 else 0) + bkt * 1000 + bnt
    prev = N.call('mmseg_conv16_mode', 1)
    try:
        ws = torch.full((need,), NAN, device=DEV)
        d32 = base.clone() if acc else torch.full_like(base, NAN)
        N.call('mmseg_conv2d_wgrad', x1.float(), x2.float() if C2 else None, dy.float(), d32.view(-1), ws, need, B, H, W, C1, C2, H, W, Cout,
               3, 3, 1, 1, 1, ups, acc)
        assert _last() == code, 'fp32 storage: kernel %d, not %d' % (_last(), code)
        for io in (5, 1, 4):
            ws.fill_(NAN)
            got = base.clone() if acc else torch.full_like(base, NAN)
            a1 = x1 if io & 1 else x1.float()
            a2 = (x2 if io & 1 else x2.float()) if C2 else None
            g = dy if io & 4 else dy.float()
            N.call('mmseg_conv2d_wgrad_t', a1, a2, g, got.view(-1), ws, need, B, H, W, C1, C2, H, W, Cout, 3, 3, 1, 1, 1, ups, acc, io)
            assert _last() == code, 'io=%d: kernel %d, not %d' % (io, _last(), code)
            nan = torch.isnan(ws)
            assert not nan[:staged].any() and nan[staged:].all(), 'io=%d: %d slabs should be staged' % (io, S)
            assert torch.equal(got, d32), 'io=%d: max diff %g' % (io, float((got - d32).abs().max()))
    finally:
        N.call('mmseg_conv16_mode', prev)
    want = ref + (basec.double() if acc else 0.0)
    err = float((d32.cpu().double() - want).abs().max()) / float(want.abs().max())
    print('register-staged wgrad: oracle err %.3e' % err)
    assert not torch.isnan(d32).any() and err <= 2e-5


# B, H, W, Cin, Cout | conv_fast_batched_kernel tile (N = Cin); 4x4 stride 2 'valid'
PARITY16 = [
    pytest.param(2, 31, 31, 64, 128, 4064064, id='hole7-4-64x64-2x31x31-64to128-odd-input-classes-of-different-size'),
    pytest.param(2, 33, 30, 32, 64, 4128032, id='hole7-4-128x32-2x33x30-32to64'),
    pytest.param(1, 223, 223, 64, 32, 4128064, id='hole7-4-128x64-1x223x223-64to32-classes-12544-12432-12432-12321'),
    pytest.param(1, 221, 221, 96, 32, 4128128, id='hole7-4-128x128-1x221x221-96to32-Cin96-32-dead-columns'),
]


@pytest.mark.parametrize('B,H,W,Cin,Cout,code', PARITY16)
def test_parity_class_data_gradient_in_the_16bit_modes(B, H, W, Cin, Cout, code, mode):
    """conv_fast_batched_kernel<..., PREC 1 / 2> through ops._Conv2d.backward: the stride-2 data gradient in the 16-bit COMPUTE modes.  Its entry
    point mmseg_conv2d_dgrad_parity_all takes fp32 tensors only (io = 0: the IN16 instance of this kernel is never launched), so there is no
    16-bit STORAGE form to test -- the operands are rounded on their way into the MFMA.  Against the fp64 oracle on the rounded operands."""
    Ho, Wo = (H - 4) // 2 + 1, (W - 4) // 2 + 1
    x = rnd(B, H, W, Cin, seed=1).to(DEV).requires_grad_(True)
    w = (rnd(4, 4, Cin, Cout, seed=2) * (2.0 / (16 * Cin)) ** 0.5).to(DEV)
    dy = rnd(B, Ho, Wo, Cout, seed=3).to(mode).float()
    prev = N.call('mmseg_conv16_mode', 1)
    try:
        y = P.conv2d(x, w, None, stride=2, padding='valid')
        y.backward(dy.to(DEV))
        assert _last() == code, 'data gradient ran on kernel %d, not %d' % (_last(), code)
    finally:
        N.call('mmseg_conv16_mode', prev)
    xr = torch.zeros(B, H, W, Cin, dtype=torch.float64, requires_grad=True)
    O.conv2d(xr, w.to(mode).float().cpu().double(), None, stride=2, padding='valid').backward(dy.double())
    scale = float(xr.grad.abs().max())
    err = float((x.grad.cpu().double() - xr.grad).abs().max()) / scale
    print('parity classes: oracle err %.3e' % err)
    assert err < 4e-4
    if (W - 4) % 2:
        assert not x.grad[:, :, W - 1].any(), 'the last input column is reached by no tap'
    if (H - 4) % 2:
        assert not x.grad[:, H - 1].any(), 'the last input row is reached by no tap'
