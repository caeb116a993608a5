"""Yardstick of tests/test_volume_uncertainty.py: an fp64 numpy / scipy restatement of the ensemble's mean map, of its uncertainty planes,
of their way back to a volume's own grid and of the calibration scores ("Several models, their mean and its
uncertainty").  Build-defined: the reference predicts with one model and writes no probability.  It shares no code with
volume_predictor.py or csrc/postprocess.hip; the sampling is that of tests/volume_tta_ref.py (views) and tests/volume_predict_ref.py
(the way back).

    members      per member r (a model: prob [V*N,OH,OW,C], back [V,6]) and view v the sample q of tests/volume_tta_ref.merge; over all
                 covering (r, v): sum += q, sh += h(q), cnt += 1, h(q) = sum of t over the K organs and rest = max(0, 1 - sum q),
                 t(x) = -x ln x (0 for x <= 0).  mean = sum / cnt, Hraw = h(mean), H = min(1, Hraw / ln(K+1)),
                 I = max(0, Hraw - sh / cnt) / ln(K+1); cnt == 0 gives (0, 0, 0)
    levels       plane u sampled as tests/volume_predict_ref.sample samples an organ channel, limited to [0, 1], times 255, rounded half
                 up; 0 outside the window.  UNDECIDABLE where 255 v lies within 1e-3 of k + 0.5
    scores       from a table (bins [K,B,2], sums [K,B+2]): n = sum of n_b, conf_b = sum p / n_b, freq_b = positives / n_b,
                 ECE = sum n_b / n |freq_b - conf_b|, MCE = the largest |freq_b - conf_b| of a bin that holds a pixel, Brier and NLL = their
                 sums / n; nan for an organ without pixels

Also here: the fp32 numpy rule of the five entry points, statement by statement in the expression order of include/mmseg_hip.h, as the
TEST-ONLY CPU stand-ins (installed into tests/cpu_backend._TABLE by the test's fixture) and, for the calibration table, as the fp32 side of
the comparison (`table32`): the bins of a pixel are decided in fp32, so only an fp32 restatement can be held to equality."""
import numpy as np
import torch

from tests import volume_predict_ref as P
from tests import volume_tta_ref as A

LEVEL_BAND = 1e-3          # of 255 v around k + 0.5: a quarter of one level is 1e-3 of the value, this is 4e-6 of it
LEVEL_CAP = 5e-3           # share of a case's pixels that may be undecidable
MAX_PLANES, MAX_BINS, MAX_MEMBERS = 4, 64, 7


# ---- fp64 ---------------------------------------------------------------------------------------------------------------------------------
def xlogx(x):
    x = np.asarray(x, np.float64)
    with np.errstate(divide='ignore', invalid='ignore'):
        return np.where(x > 0, -x * np.log(np.where(x > 0, x, 1.0)), 0.0)


def entropy(q):
    """q [...,K] -> [...] in nats: the K organs and the rest"""
    q = np.asarray(q, np.float64)
    rest = np.maximum(0.0, 1.0 - q.sum(-1))
    return xlogx(q).sum(-1) + xlogx(rest)


def view_samples(prob, back, N, K):
    """prob [V*N,OH,OW,C] -> (q [V,N,OH,OW,K] fp64, cov [V,OH,OW]): tests/volume_tta_ref.merge's sample of every view"""
    from scipy import ndimage as ndi
    prob = np.asarray(prob, np.float64)
    OH, OW = prob.shape[1:3]
    cov, coords = A.coverage(back, OH, OW)
    q = np.zeros((cov.shape[0], N, OH, OW, K), np.float64)
    for v in range(cov.shape[0]):
        at = np.where(cov[v][None], coords[v], 0.0)
        for n in range(N):
            for k in range(K):
                q[v, n, :, :, k] = ndi.map_coordinates(prob[v * N + n, :, :, k], at, order=1, mode='nearest', prefilter=False)
    return q, cov


def members(probs, backs, N, K):
    """probs / backs: one (prob [V*N,OH,OW,C], back [V,6]) per member -> (mean [N,OH,OW,K], H [N,OH,OW], I [N,OH,OW], cnt [OH,OW])"""
    total = sh = cnt = None
    for prob, back in zip(probs, backs):
        q, cov = view_samples(prob, back, N, K)
        m = cov[:, None, :, :]
        s, h, c = np.where(m[..., None], q, 0.0).sum(0), np.where(m, entropy(q), 0.0).sum(0), cov.sum(0)
        total, sh, cnt = (s, h, c) if total is None else (total + s, sh + h, cnt + c)
    div = np.maximum(cnt, 1)[None]
    mean = total / div[..., None]
    raw = entropy(mean)
    norm = np.log(K + 1.0)
    H = np.where(cnt[None] > 0, np.minimum(1.0, raw / norm), 0.0)
    I = np.where(cnt[None] > 0, np.maximum(0.0, raw - sh / div) / norm, 0.0)
    return mean, H, I, cnt


def levels(planes, u, raw_hw, resampled, rows, cols, order):
    """planes [S,OH,OW,U] -> (level [S,H,W] uint8, undecidable [S,H,W] bool)"""
    planes = np.asarray(planes, np.float64)
    v = P.sample(planes[..., u:u + 1], 1, raw_hw, resampled, rows, cols, order)[..., 0]
    inside = np.broadcast_to(P.window_mask(raw_hw, resampled, rows, cols)[None], v.shape)
    x = np.clip(v, 0.0, 1.0) * 255.0 + 0.5
    level = np.where(inside, np.floor(x), 0.0).astype(np.uint8)
    undecidable = inside & (np.abs(x - np.round(x)) < LEVEL_BAND) & (order == 1)
    return level, undecidable


def scores(bins, sums):
    """bins [K,B,2], sums [K,B+2] -> [K,5] = ECE, MCE, Brier, NLL, n"""
    bins, sums = np.asarray(bins, np.float64), np.asarray(sums, np.float64)
    K, B = bins.shape[:2]
    out = np.full((K, 5), np.nan)
    for k in range(K):
        n_b, pos = bins[k, :, 0], bins[k, :, 1]
        n = n_b.sum()
        out[k, 4] = n
        if n == 0:
            continue
        some = n_b > 0
        gap = np.abs(pos[some] / n_b[some] - sums[k, :B][some] / n_b[some])
        out[k, :4] = (n_b[some] / n * gap).sum(), gap.max(), sums[k, B] / n, sums[k, B + 1] / n
    return out


def by_error(pred, truth, planes):
    """planes: a list of uint8 arrays of pred's shape -> int64 [2,1+U]"""
    wrong = np.asarray(pred) != np.asarray(truth)
    return np.asarray([[int(np.count_nonzero(m))] + [int(np.asarray(l, np.int64)[m].sum()) for l in planes] for m in (~wrong, wrong)], np.int64)


# ---- fp32, the rule's expression order -----------------------------------------------------------------------------------------------------
ONE, ZERO = np.float32(1), np.float32(0)


def _xlogx32(x):
    with np.errstate(divide='ignore', invalid='ignore'):
        return np.where(x > 0, -x * np.log(np.where(x > 0, x, ONE), dtype=np.float32), ZERO).astype(np.float32)


def entropy32(q):
    """q [...,K] fp32 -> [...] fp32: total = ((q0 + q1) + ..), h = (((0 + t(q0)) + t(q1)) + ..) + t(rest)"""
    total, h = q[..., 0], np.zeros(q.shape[:-1], np.float32)
    for k in range(q.shape[-1]):
        if k:
            total = total + q[..., k]
        h = h + _xlogx32(q[..., k])
    return (h + _xlogx32(np.maximum(ZERO, ONE - total))).astype(np.float32)


def _view32(p, b, OH, OW, K):
    """one view: p [N,OH,OW,C] fp32, b [6] -> (sample [N,OH,OW,K] fp32, cov [OH,OW]); tests/volume_tta_ref.standin_merge_views's steps"""
    r, c = np.meshgrid(np.arange(OH, dtype=np.float64), np.arange(OW, dtype=np.float64), indexing='ij')
    sr, sc = (b[0] * r + b[1] * c) + b[2], (b[3] * r + b[4] * c) + b[5]
    with np.errstate(invalid='ignore'):
        cov = (sr >= 0) & (sr <= OH - 1) & (sc >= 0) & (sc <= OW - 1)
    sr, sc = np.where(cov, sr, 0.0), np.where(cov, sc, 0.0)
    r0, c0 = np.floor(sr).astype(np.int64), np.floor(sc).astype(np.int64)
    r1, c1 = np.minimum(r0 + 1, OH - 1), np.minimum(c0 + 1, OW - 1)
    fy, fx = (sr - np.floor(sr)).astype(np.float32)[None, :, :, None], (sc - np.floor(sc)).astype(np.float32)[None, :, :, None]
    a00, a01, a10, a11 = (p[:, i, j, :K] for i, j in ((r0, c0), (r0, c1), (r1, c0), (r1, c1)))
    top = np.where(fx != 0, (ONE - fx) * a00 + fx * a01, a00)
    bot = np.where(fx != 0, (ONE - fx) * a10 + fx * a11, a10)
    return np.where(fy != 0, (ONE - fy) * top + fy * bot, top).astype(np.float32), cov


def _pixels_ok(N, OH, OW):
    return N > 0 and min(OH, OW) >= 1 and N * OH * OW < 2 ** 29


def standin_members_accumulate(prob, back, total, aux, first, V, N, OH, OW, C, K):
    if N == 0:
        return 0
    if not (1 <= V <= A.MAX_VIEWS and 1 <= K <= min(C, 16) and _pixels_ok(N, OH, OW) and N * OH * OW * V * C * 4 < 2 ** 31):
        return 1
    p, b = prob.numpy().reshape(V, N, OH, OW, C), back.numpy().reshape(V, 6)
    acc = np.zeros((N, OH, OW, K), np.float32) if first else total.numpy().copy()
    sh = np.zeros((N, OH, OW), np.float32) if first else aux.numpy()[..., 0].copy()
    cnt = np.zeros((N, OH, OW), np.float32) if first else aux.numpy()[..., 1].copy()
    for v in range(V):
        q, cov = _view32(p[v], b[v], OH, OW, K)
        m = np.broadcast_to(cov[None], sh.shape)
        acc = np.where(m[..., None], acc + q, acc)
        sh = np.where(m, sh + entropy32(q), sh)
        cnt = np.where(m, cnt + ONE, cnt)
    total.copy_(torch.from_numpy(acc.astype(np.float32)))
    aux.copy_(torch.from_numpy(np.stack([sh, cnt], axis=-1).astype(np.float32)))
    return 0


def standin_members_finish(total, aux, N, OH, OW, K):
    if N == 0:
        return 0
    if not (1 <= K <= 16 and _pixels_ok(N, OH, OW)):
        return 1
    acc, sh, cnt = total.numpy().copy(), aux.numpy()[..., 0].copy(), aux.numpy()[..., 1].copy()
    div = np.where(cnt == 0, ONE, cnt)
    c = cnt[..., None]
    mean = np.where(c == 1, acc, np.where(c == 0, ZERO, acc / div[..., None])).astype(np.float32)
    raw = entropy32(mean)
    e = np.where(cnt == 1, sh, sh / div).astype(np.float32)
    inv = np.float32(1.0 / np.log(K + 1.0))
    H = np.where(cnt == 0, ZERO, np.minimum(ONE, raw * inv))
    I = np.where(cnt == 0, ZERO, np.maximum(ZERO, raw - e) * inv)
    total.copy_(torch.from_numpy(mean))
    aux.copy_(torch.from_numpy(np.stack([H, I], axis=-1).astype(np.float32)))
    return 0


def _axis32(n_raw, R, lo, kept, before, order):
    """one axis of mmseg_restore_label: (inside [n], i0 [n], i1 [n], f [n] fp32)"""
    s = P.raw_coordinates(n_raw, R)
    inside = (s >= lo) & (s <= lo + kept - 1)
    if order == 0:
        i0 = np.clip(np.floor(s + 0.5).astype(np.int64), lo, lo + kept - 1) - lo + before
        return inside, np.where(inside, i0, before), np.where(inside, i0, before), np.zeros(n_raw, np.float32)
    w = s - lo
    fl = np.floor(w)
    i = fl.astype(np.int64)
    i0, i1 = np.where(inside, i + before, before), np.where(inside, np.minimum(i + 1, kept - 1) + before, before)
    return inside, i0, i1, np.where(inside, (w - fl).astype(np.float32), ZERO).astype(np.float32)


def sample32(src, channels, raw_hw, resampled, rows, cols, order):
    """src [S,OH,OW,C] fp32 -> (v [S,H,W,len(channels)] fp32, inside [H,W]): the taps and po_mix's expression, in fp32"""
    iy, r0, r1, fy = _axis32(raw_hw[0], resampled[0], rows[0], rows[1], rows[2], order)
    ix, c0, c1, fx = _axis32(raw_hw[1], resampled[1], cols[0], cols[1], cols[2], order)
    src = np.asarray(src, np.float32)[..., list(channels)]
    a00 = src[:, r0][:, :, c0]
    if order == 0:
        return a00, iy[:, None] & ix[None, :]
    a01, a10, a11 = src[:, r0][:, :, c1], src[:, r1][:, :, c0], src[:, r1][:, :, c1]
    fy, fx = fy[None, :, None, None], fx[None, None, :, None]
    top = (ONE - fx) * a00 + fx * a01
    bot = (ONE - fx) * a10 + fx * a11
    return ((ONE - fy) * top + fy * bot).astype(np.float32), iy[:, None] & ix[None, :]


def _geometry_ok(S, H, W, RH, RW, OH, OW, rows, cols):
    def axis(lo, kept, before, R, O):
        return lo >= 0 and kept >= 1 and lo + kept <= R and 0 <= before < O and before + kept <= O
    return 0 < S <= 65535 and min(H, W, RH, RW, OH, OW) >= 1 and axis(*(tuple(rows) + (RH, OH))) and axis(*(tuple(cols) + (RW, OW)))


def standin_restore_map(planes, out, S, H, W, RH, RW, OH, OW, lo_r, kept_r, before_r, lo_c, kept_c, before_c, U, u, order):
    if S <= 0:
        return 0
    rows, cols = (lo_r, kept_r, before_r), (lo_c, kept_c, before_c)
    if not (1 <= U <= MAX_PLANES and 0 <= u < U and order in (0, 1) and _geometry_ok(S, H, W, RH, RW, OH, OW, rows, cols)):
        return 1
    v, inside = sample32(planes.numpy(), [u], (H, W), (RH, RW), rows, cols, order)
    level = (np.fmin(np.fmax(v[..., 0], ZERO), ONE) * np.float32(255) + np.float32(0.5)).astype(np.uint8)          # fmaxf: a NaN gives 0
    out.copy_(torch.from_numpy(np.where(inside[None], level, 0).astype(np.uint8)))
    return 0


def table32(prob, truth, values, raw_hw, resampled, rows, cols, B, order):
    """the rule of mmseg_calibration_table: (bins [K,B,2] int64, sums [K,B+2] fp64)"""
    K = len(values)
    p, inside = sample32(prob, range(K), raw_hw, resampled, rows, cols, order)
    bins, sums = np.zeros((K, B, 2), np.int64), np.zeros((K, B + 2), np.float64)
    m = np.broadcast_to(inside[None], p.shape[:3])
    for k in range(K):
        pk, y = p[..., k][m], (np.asarray(truth) == values[k])[m]
        b = np.minimum(B - 1, np.maximum(0, (pk * np.float32(B)).astype(np.int64)))
        bins[k, :, 0] = np.bincount(b, minlength=B)
        bins[k, :, 1] = np.bincount(b[y], minlength=B)
        sums[k, :B] = np.bincount(b, weights=pk.astype(np.float64), minlength=B)
        sums[k, B] = ((pk.astype(np.float64) - y) ** 2).sum()
        sums[k, B + 1] = (-np.log(np.maximum(np.where(y, pk, ONE - pk), np.float32(1e-6)), dtype=np.float32)).astype(np.float64).sum()
    return bins, sums


def _table_ok(S, H, W, K, B):
    return S >= 1 and min(H, W) >= 1 and S * H * W < 2 ** 31 - 1 and 1 <= K <= 16 and 2 <= B <= MAX_BINS


def standin_calibration_table_workspace_bytes(S, H, W, K, B):
    return 8 * min(-(-S * H * W // 256), 1024) * K * (B + 2) if _table_ok(S, H, W, K, B) else 0


def standin_calibration_table(prob, truth, values, bins, sums, ws, S, H, W, RH, RW, OH, OW, lo_r, kept_r, before_r, lo_c, kept_c, before_c,
                              C, K, B, order):
    if S == 0:
        return 0
    rows, cols = (lo_r, kept_r, before_r), (lo_c, kept_c, before_c)
    if not (_table_ok(S, H, W, K, B) and K <= C and order in (0, 1) and _geometry_ok(S, H, W, RH, RW, OH, OW, rows, cols)):
        return 1
    b, s = table32(prob.numpy(), truth.numpy(), [int(v) for v in values], (H, W), (RH, RW), rows, cols, B, order)
    bins.copy_(torch.from_numpy(b.astype(np.int32)))
    sums.copy_(torch.from_numpy(s))
    return 0


def standin_uncertainty_by_error(pred, truth, levels_, out, n, U):
    if n == 0:
        return 0
    if not (1 <= U <= MAX_PLANES and 0 < n < 2 ** 31 - 1):
        return 1
    l = levels_.numpy().reshape(U, n)
    out.copy_(torch.from_numpy(by_error(pred.numpy().reshape(n), truth.numpy().reshape(n), list(l))))
    return 0


STANDINS = {'mmseg_members_accumulate': standin_members_accumulate, 'mmseg_members_finish': standin_members_finish,
            'mmseg_restore_map': standin_restore_map, 'mmseg_calibration_table': standin_calibration_table,
            'mmseg_calibration_table_workspace_bytes': standin_calibration_table_workspace_bytes,
            'mmseg_uncertainty_by_error': standin_uncertainty_by_error}
