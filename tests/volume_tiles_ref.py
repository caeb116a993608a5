"""Yardstick of tests/test_volume_tiles.py: an fp64 numpy restatement of the tile plan, the tile weights and the blend of INTEGRATION.md
section 5 ("Frames larger than the input").  Build-defined: the reference predicts the cropped frame only.  It shares no code with
loaders/volume_folder.py or csrc/postprocess.hip.

    plan      R <= O: one tile, the padded centre window (0, R, (O - R) // 2).  R > O: n = ceil((R - overlap) / (O - overlap)) tiles
              (a_i, O, 0), a_i = (i * (R - O)) // (n - 1).  More than 8 tiles is refused.
    weights   container index j of tile i: min(l, r), l = j + 1 with a left neighbour else O, r = O - j with a right neighbour else O
    others    the window of tile i on another modality's frame starts at s_i - c(R_m) + c(R_j): s_i the signed start of the tile on
              the planned frame (lo - before), c(R) the signed start of the centre crop (ceil((R - O) / 2) for R > O, else
              -((O - R) // 2)); container index u reads frame index clamp(start + u, 0, R_j - 1)
    blend     out = sum of W p / sum of W over the tiles that cover the pixel, W = wr * wc, in fp64; no covering tile gives 0

Also here: the TEST-ONLY CPU stand-in of mmseg_blend_tiles (installed into tests/cpu_backend._TABLE by the test's fixture): fp32, the
tiles in ascending order, a singly covered pixel copied."""
import numpy as np
import torch

MAX_TILES = 8
MAP_BAR = 1e-5          # (64 + 2) * 2^-24 = 3.9e-6 for probabilities in [0, 1], with margin
LABEL_BAND = 2e-5       # volume_predict_ref.UNDECIDABLE + MAP_BAR


def plan(R, O, overlap):
    if R <= O:
        return [(0, R, (O - R) // 2)]
    n = 1
    while n * (O - overlap) + overlap < R:          # the least n whose tiles, sharing `overlap`, reach R
        n += 1
    if n > MAX_TILES:
        raise ValueError('%d tiles' % n)
    return [((i * (R - O)) // (n - 1), O, 0) for i in range(n)]


def weights(tiles, O):
    out = np.zeros((len(tiles), O), np.float64)
    for i in range(len(tiles)):
        for j in range(O):
            left = j + 1 if i > 0 else O
            right = O - j if i + 1 < len(tiles) else O
            out[i, j] = min(left, right)
    return out


def centre(R, O):
    return -(-(R - O) // 2) if R > O else -((O - R) // 2)


def other_starts(tiles, R_m, R_j, O):
    """signed starts of the windows on the other frame"""
    return [lo - before - centre(R_m, O) + centre(R_j, O) for lo, kept, before in tiles]


def window_indices(start, R, O):
    """the frame index every container index reads: edge padding"""
    return np.clip(start + np.arange(O), 0, R - 1)


def map_indices(lo, kept, before, O):
    """the frame index every container index reads under the contract of mmseg_preprocess_image"""
    return lo + np.clip(np.arange(O) - before, 0, kept - 1)


def contract_ok(lo, kept, before, R, O):
    return 0 <= lo and kept >= 1 and lo + kept <= R and 0 <= before < O


def blend(prob, rows, cols, wr, wc, S, RH, RW, K):
    """prob [TR*TC*S,OH,OW,C] -> (fp64 [S,RH,RW,K], the number of covering tiles [RH,RW])"""
    prob = np.asarray(prob)
    OH, OW = prob.shape[1:3]
    wr, wc = np.asarray(wr, np.float64), np.asarray(wc, np.float64)
    num, den = np.zeros((S, RH, RW, K), np.float64), np.zeros((RH, RW), np.float64)
    count = np.zeros((RH, RW), np.int64)
    for tr, (lo_r, kept_r, before_r) in enumerate(rows):
        for tc, (lo_c, kept_c, before_c) in enumerate(cols):
            t = tr * len(cols) + tc
            tile = prob[t * S:(t + 1) * S, before_r:before_r + kept_r, before_c:before_c + kept_c, :K].astype(np.float64)
            W = np.outer(wr[tr, before_r:before_r + kept_r], wc[tc, before_c:before_c + kept_c])
            num[:, lo_r:lo_r + kept_r, lo_c:lo_c + kept_c] += W[None, :, :, None] * tile
            den[lo_r:lo_r + kept_r, lo_c:lo_c + kept_c] += W
            count[lo_r:lo_r + kept_r, lo_c:lo_c + kept_c] += 1
    out = np.where(den[None, :, :, None] > 0, num / np.where(den > 0, den, 1.0)[None, :, :, None], 0.0)
    return out, count


# ---- CPU stand-in of the entry point (argument list of include/mmseg_hip.h without the stream) -------------------------------------------
def standin_blend_tiles(prob, rows, cols, wr, wc, out, S, TR, TC, OH, OW, C, K, RH, RW):
    if not (1 <= TR <= MAX_TILES and 1 <= TC <= MAX_TILES and 1 <= K <= min(C, 16) and min(OH, OW, RH, RW) >= 1 and S >= 0):
        return 1
    p = prob.numpy().reshape(TR * TC, S, OH, OW, C)
    ar, ac = rows.numpy().reshape(TR, 3), cols.numpy().reshape(TC, 3)
    fr, fc = wr.numpy().reshape(TR, OH), wc.numpy().reshape(TC, OW)
    num, first = np.zeros((S, RH, RW, K), np.float32), np.zeros((S, RH, RW, K), np.float32)
    den, count = np.zeros((RH, RW), np.float32), np.zeros((RH, RW), np.int64)
    for tr in range(TR):
        for tc in range(TC):
            (lo_r, kept_r, before_r), (lo_c, kept_c, before_c) = (int(v) for v in ar[tr]), (int(v) for v in ac[tc])
            ys, xs = slice(lo_r, lo_r + kept_r), slice(lo_c, lo_c + kept_c)
            tile = p[tr * TC + tc, :, before_r:before_r + kept_r, before_c:before_c + kept_c, :K]
            W = (fr[tr, before_r:before_r + kept_r][:, None] * fc[tc, before_c:before_c + kept_c][None, :]).astype(np.float32)
            first[:, ys, xs] = np.where((count[ys, xs] == 0)[None, :, :, None], tile, first[:, ys, xs])
            num[:, ys, xs] = num[:, ys, xs] + W[None, :, :, None] * tile
            den[ys, xs] = den[ys, xs] + W
            count[ys, xs] += 1
    with np.errstate(invalid='ignore', divide='ignore'):
        mean = num / den[None, :, :, None]
    c = count[None, :, :, None]
    out.copy_(torch.from_numpy(np.where(c == 1, first, np.where(c == 0, np.float32(0), mean)).astype(np.float32)))
    return 0


STANDINS = {'mmseg_blend_tiles': standin_blend_tiles}
