"""Yardstick of tests/test_volume_tta.py: an fp64 numpy / scipy restatement of the views of test-time augmentation and of their merge
("Views of a slice, merged").  Build-defined: the reference predicts every slice once.  It shares no code
with volume_predictor.py or csrc/postprocess.hip.

    matrices  per token the two 2 x 3 matrices F (view pixel -> the image pixel it shows) and B (image pixel -> the view pixel that shows
              it), written out from the table; a matrix m takes (r, c) to (m0*r + m1*c + m2, m3*r + m4*c + m5)
    merge     per view the fp64 coordinate (b0*r + b1*c) + b2, (b3*r + b4*c) + b5; the view covers the pixel iff the coordinate lies in
              [0, OH-1] x [0, OW-1]; scipy.ndimage.map_coordinates(order=1, mode='nearest', prefilter=False) samples the view's map
              there; out = the mean over the covering views, 0 where there is none

Also here: the TEST-ONLY CPU stand-in of mmseg_merge_views (installed into tests/cpu_backend._TABLE by the test's fixture): fp32, the
views in ascending order, a zero fraction skipping its taps, a singly covered pixel copied."""
import math

import numpy as np
import torch
from scipy import ndimage as ndi

MAX_VIEWS = 16
EXACT = ('id', 'fliplr', 'flipud', 'rot180', 'transpose', 'antitranspose', 'rot90', 'rot270')
PRESETS = {'flips': ['id', 'fliplr', 'flipud', 'rot180'], 'd4': list(EXACT)}


def expand(text):
    out = []
    for t in text.split(','):
        out += PRESETS.get(t, [t])
    return out


def matrices(token, OH, OW):
    """(F, B), each [6] fp64"""
    h, w = OH - 1.0, OW - 1.0
    if token == 'id':
        F = B = [1, 0, 0, 0, 1, 0]
    elif token == 'fliplr':          # (r, OW-1-c)
        F = B = [1, 0, 0, 0, -1, w]
    elif token == 'flipud':          # (OH-1-r, c)
        F = B = [-1, 0, h, 0, 1, 0]
    elif token == 'rot180':          # (OH-1-r, OW-1-c)
        F = B = [-1, 0, h, 0, -1, w]
    elif token == 'transpose':          # (c, r)
        F = B = [0, 1, 0, 1, 0, 0]
    elif token == 'antitranspose':          # (OW-1-c, OH-1-r)
        F = B = [0, -1, w, -1, 0, h]
    elif token == 'rot90':          # F (c, OW-1-r), B (OH-1-c, r)
        F, B = [0, 1, 0, -1, 0, w], [0, -1, h, 1, 0, 0]
    elif token == 'rot270':          # F (OH-1-c, r), B (c, OW-1-r)
        F, B = [0, -1, h, 1, 0, 0], [0, 1, 0, -1, 0, w]
    else:
        cy, cx = h / 2, w / 2
        out = []
        for theta in (float(token[3:]) * math.pi / 180, -(float(token[3:]) * math.pi / 180)):
            cos, sin = math.cos(theta), math.sin(theta)
            out.append([cos, -sin, cy - cos * cy + sin * cx, sin, cos, cx - sin * cy - cos * cx])
        F, B = out
    return np.asarray(F, np.float64), np.asarray(B, np.float64)


def tables(text, OH, OW):
    """-> (tokens, F [V,6], B [V,6])"""
    tokens = expand(text)
    pairs = [matrices(t, OH, OW) for t in tokens]
    return tokens, np.stack([p[0] for p in pairs]), np.stack([p[1] for p in pairs])


def apply(m, r, c):
    return (m[0] * r + m[1] * c) + m[2], (m[3] * r + m[4] * c) + m[5]


def coverage(back, OH, OW):
    """[V,OH,OW] bool, and the fp64 coordinates [V,2,OH,OW]"""
    r, c = np.meshgrid(np.arange(OH, dtype=np.float64), np.arange(OW, dtype=np.float64), indexing='ij')
    coords = np.stack([np.stack(apply(b, r, c)) for b in np.asarray(back, np.float64)])
    with np.errstate(invalid='ignore'):
        cov = (coords[:, 0] >= 0) & (coords[:, 0] <= OH - 1) & (coords[:, 1] >= 0) & (coords[:, 1] <= OW - 1)
    return cov, coords


def merge(prob, back, N, K):
    """prob [V*N,OH,OW,C] -> (fp64 [N,OH,OW,K], the number of covering views [OH,OW])"""
    prob = np.asarray(prob, np.float64)
    OH, OW = prob.shape[1:3]
    cov, coords = coverage(back, OH, OW)
    num = np.zeros((N, OH, OW, K), np.float64)
    for v in range(cov.shape[0]):
        at = np.where(cov[v][None], coords[v], 0.0)
        for n in range(N):
            for k in range(K):
                s = ndi.map_coordinates(prob[v * N + n, :, :, k], at, order=1, mode='nearest', prefilter=False)
                num[n, :, :, k] += np.where(cov[v], s, 0.0)
    count = cov.sum(0)
    return num / np.maximum(count, 1)[None, :, :, None], count


def views_in(x, forward):
    """x [N,OH,OW] -> fp64 [V,N,OH,OW]: view v of slice n is x[n] read at F_v (r, c), bilinear, the edge repeated
    (scipy.ndimage.affine_transform(order=1, mode='nearest'))"""
    x = np.asarray(x, np.float64)
    out = np.zeros((len(forward),) + x.shape, np.float64)
    for v, f in enumerate(np.asarray(forward, np.float64)):
        for n in range(x.shape[0]):
            out[v, n] = ndi.affine_transform(x[n], f.reshape(2, 3)[:, :2], f.reshape(2, 3)[:, 2], order=1, mode='nearest')
    return out


# ---- CPU stand-in of the entry point (argument list of include/mmseg_hip.h without the stream) -------------------------------------------
def standin_merge_views(prob, back, out, V, N, OH, OW, C, K):
    if N == 0:
        return 0
    if not (1 <= V <= MAX_VIEWS and 1 <= K <= min(C, 16) and min(OH, OW) >= 1 and N > 0 and N * OH * OW < 2 ** 29):
        return 1
    p = prob.numpy().reshape(V, N, OH, OW, C)
    b = back.numpy().reshape(V, 6)
    r, c = np.meshgrid(np.arange(OH, dtype=np.float64), np.arange(OW, dtype=np.float64), indexing='ij')
    one = np.float32(1)
    num, first = np.zeros((N, OH, OW, K), np.float32), np.zeros((N, OH, OW, K), np.float32)
    count = np.zeros((OH, OW), np.int64)
    for v in range(V):
        sr, sc = (b[v, 0] * r + b[v, 1] * c) + b[v, 2], (b[v, 3] * r + b[v, 4] * c) + b[v, 5]
        with np.errstate(invalid='ignore'):
            cov = (sr >= 0) & (sr <= OH - 1) & (sc >= 0) & (sc <= OW - 1)
        sr, sc = np.where(cov, sr, 0.0), np.where(cov, sc, 0.0)
        r0, c0 = np.floor(sr).astype(np.int64), np.floor(sc).astype(np.int64)
        r1, c1 = np.minimum(r0 + 1, OH - 1), np.minimum(c0 + 1, OW - 1)
        fy, fx = (sr - np.floor(sr)).astype(np.float32)[None, :, :, None], (sc - np.floor(sc)).astype(np.float32)[None, :, :, None]
        a00, a01, a10, a11 = (p[v][:, i, j, :K] for i, j in ((r0, c0), (r0, c1), (r1, c0), (r1, c1)))
        top = np.where(fx != 0, (one - fx) * a00 + fx * a01, a00)
        bot = np.where(fx != 0, (one - fx) * a10 + fx * a11, a10)
        val = np.where(fy != 0, (one - fy) * top + fy * bot, top).astype(np.float32)
        m = cov[None, :, :, None]
        first = np.where(m & (count == 0)[None, :, :, None], val, first)
        num = np.where(m, num + val, num)
        count += cov
    cnt = count[None, :, :, None]
    mean = num / np.maximum(cnt, 1).astype(np.float32)
    out.copy_(torch.from_numpy(np.where(cnt == 1, first, np.where(cnt == 0, np.float32(0), mean)).astype(np.float32)))
    return 0


STANDINS = {'mmseg_merge_views': standin_merge_views}
