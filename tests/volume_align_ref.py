"""Yardstick of tests/test_volume_align.py: a numpy restatement of the alignment of a volume's modalities by mutual information (the rule is
in include/mmseg_hip.h), on top of the resampling of tests/volume_loader_ref.py and the order statistics of tests/volume_intensity_ref.py.
It shares no code with loaders/volume_folder.py, ops.py or csrc/align.hip.

    quantise     the resampled frames in fp32, binned between two order statistics of the volume; `position` is the same expression in fp64
    pairs        brute force: every window coordinate of a generous range is tested against both frames and against the stride (Python's
                 floor-mod), nothing is derived from interval lengths -- n_full_closed, the closed form, is checked against it
    score        Studholme's (H(A) + H(B)) / H(A,B) in fp64, p = count / N, natural log, empty bins skipped
    select       a sort under the tie rule
    search       the lattice at stride 2^(L-1), then +-1 slice x +-t pixels around the best, down to stride 1

Also here: the TEST-ONLY CPU stand-ins of the mmseg_align_* entry points, installed into tests/cpu_backend._TABLE by the test's fixture.

The bar of the scores (score_bar).  u = 2^-53.  A term t = -(p log p): p = count / N carries a relative error <= u (one division), log one of
<= 1 ulp of its result plus the error of p passed on, |d log p| <= u, i.e. an ABSOLUTE error of p u in the term; the product adds u.  So
|dt| <= 3 u |t| + u p, and over a table, sum p = 1:  |dH| <= (3 + n - 1) u H + u, n the number of terms added (any order; all terms have one
sign, so the sum of their magnitudes is H itself).  Relative: (n + 2) u + u / H.  The joint entropy adds n = B^2 terms, a marginal n = B.
score = (H(A) + H(B)) / H(A,B): one addition and one division more, so its relative error is at most
    (B + 2) u + u / min(H(A), H(B)) + u   +   (B^2 + 2) u + u / H(A,B)   +   u   <=   (B^2 + B + 6 + 2 / h_min) u
for tables whose three entropies are all >= h_min, and the score is at most 2.  The device and this restatement may each be that far from
the true value: bar = 2 * 2 * (B^2 + B + 6 + 2 / h_min) * 2^-53, i.e. B^2 + 2 B terms of a few ulp, twice.  About 1.9e-12 at 64 bins."""
import numpy as np
import torch

from tests import volume_intensity_ref as I

MODE_LIST, MODE_LATTICE, MODE_REFINE = 0, 1, 2
UNDECIDABLE = 1e-4
CAP = 5e-3          # share of the pixels of a quantise case that may be undecidable: a condition on the inputs, not a measurement
U = 2.0 ** -53


def centre_start(R, O):
    return (R - O + 1) // 2 if R > O else -((O - R) // 2)


# ---- 1 quantise ------------------------------------------------------------------------------------------------------------------------
def quantise_frames(fr, lo, hi, bins):
    """(q uint8, position fp64) of resampled frames fr (fp32) between the fp32 values lo, hi"""
    fr = fr.astype(np.float32)
    lo, hi = np.float32(lo), np.float32(hi)
    if not hi > lo:
        return np.zeros(fr.shape, np.uint8), np.zeros(fr.shape, np.float64)
    scale = np.float32(np.float32(bins) / np.float32(hi - lo))
    inner = np.minimum(bins - 1, np.floor(((fr - lo).astype(np.float32) * scale).astype(np.float32))).astype(np.int64)
    q = np.where(fr <= lo, 0, np.where(fr >= hi, bins - 1, inner)).astype(np.uint8)
    position = (fr.astype(np.float64) - float(lo)) * float(bins) / (float(hi) - float(lo))
    return q, position


def quantise(image, RH, RW, bins, percentiles=(0.5, 99.5)):
    """(q [S,RH,RW] uint8, position, (lo, hi)) of the raw slices image [S,H,W]"""
    fr = I.frames(image, RH, RW, np.float32)
    lo, hi = I.knots(fr, I.ranks(fr.size, percentiles), True)[0]
    q, position = quantise_frames(fr, lo, hi, bins)
    return q, position, (lo, hi)


def undecidable(position, bins):
    """pixels whose fp64 position lies within UNDECIDABLE of one of the decision points 1 .. bins - 1.  (0 and bins are no decision points:
    the bins on both sides of them are the same, 0 and bins - 1.)"""
    near = np.abs(position - np.round(position)) < UNDECIDABLE
    return near & (np.round(position) >= 1) & (np.round(position) <= bins - 1)


# ---- 2 pairing ---------------------------------------------------------------------------------------------------------------------------
def _axis_pairs(Ra, Rb, O, d, t):
    """(indices into A, indices into B) of one axis, by testing every window coordinate"""
    ca, cb = centre_start(Ra, O), centre_start(Rb, O)
    span = Ra + Rb + abs(d) + abs(ca) + abs(cb) + t + 1
    o = np.array([v for v in range(-span, span + 1) if v % t == 0 and 0 <= v + ca < Ra and 0 <= v + cb + d < Rb], np.int64)
    return o + ca, o + cb + d


def _window(window):
    return (int(window), int(window)) if np.isscalar(window) else (int(window[0]), int(window[1]))


def pairs(qa, qb, window, cand, t):
    """(a values, b values) of every sampled pair of candidate (dz, dy, dx), flattened"""
    dz, dy, dx = cand
    OH, OW = _window(window)
    ia = np.array([i for i in range(qa.shape[0]) if 0 <= i + dz < qb.shape[0]], np.int64)
    ya, yb = _axis_pairs(qa.shape[1], qb.shape[1], OH, dy, t)
    xa, xb = _axis_pairs(qa.shape[2], qb.shape[2], OW, dx, t)
    if not (len(ia) and len(ya) and len(xa)):
        return np.zeros(0, np.int64), np.zeros(0, np.int64)
    return qa[np.ix_(ia, ya, xa)].reshape(-1).astype(np.int64), qb[np.ix_(ia + dz, yb, xb)].reshape(-1).astype(np.int64)


def histogram(qa, qb, window, cand, t, bins):
    a, b = pairs(qa, qb, window, cand, t)
    a, b = np.minimum(a, bins - 1), np.minimum(b, bins - 1)
    return np.bincount(a * bins + b, minlength=bins * bins).reshape(bins, bins)


def histograms(qa, qb, window, cands, t, bins):
    """[C,B,B] int64; a candidate None (outside the range) has an empty table"""
    return np.stack([np.zeros((bins, bins), np.int64) if c is None else histogram(qa, qb, window, c, t, bins) for c in cands])


def n_full_brute(shape_a, shape_b, window, cand):
    a, _ = pairs(np.zeros(shape_a, np.uint8), np.zeros(shape_b, np.uint8), window, cand, 1)
    return int(a.size)


def n_full_closed(shape_a, shape_b, window, cand):
    """the product of the three overlap lengths"""
    OH, OW = _window(window)
    dz, dy, dx = cand
    n = max(0, min(shape_a[0], shape_b[0] - dz) - max(0, -dz))
    for Ra, Rb, O, d in ((shape_a[1], shape_b[1], OH, dy), (shape_a[2], shape_b[2], OW, dx)):
        ca, cb = centre_start(Ra, O), centre_start(Rb, O)
        n *= max(0, min(Ra - ca, Rb - cb - d) - max(-ca, -cb - d))
    return n


# ---- 3 score -------------------------------------------------------------------------------------------------------------------------------
def entropy(counts, n):
    c = np.asarray(counts, np.float64).reshape(-1)
    p = c[c > 0] / float(n)
    return float(-(p * np.log(p)).sum())


def entropies(h):
    n = int(h.sum())
    return entropy(h.sum(1), n), entropy(h.sum(0), n), entropy(h, n)


def score(h, admissible=True):
    """(score, N) of one table"""
    n = int(h.sum())
    if n == 0 or not admissible:
        return -1.0, n
    ha, hb, hab = entropies(h)
    return (-1.0 if hab == 0.0 else (ha + hb) / hab), n


def admissible(shape_a, shape_b, window, cand, min_overlap):
    return float(n_full_closed(shape_a, shape_b, window, cand)) >= min_overlap * float(n_full_closed(shape_a, shape_b, window, (0, 0, 0)))


def scores(h, shape_a, shape_b, window, cands, min_overlap):
    """[C,2] fp64"""
    return np.array([score(t, c is not None and admissible(shape_a, shape_b, window, c, min_overlap)) for t, c in zip(h, cands)], np.float64)


def score_bar(bins, h_min):
    """see the module's docstring; holds for tables whose three entropies are all >= h_min"""
    return 2 * 2 * (bins * bins + bins + 6 + 2.0 / h_min) * U


# ---- 4 search -------------------------------------------------------------------------------------------------------------------------------
def stage_candidates(mode, t, Z, Py, Px, centre=(0, 0, 0)):
    """the candidates of a lattice or refinement stage in the header's index order, None where one leaves the range; the zero-shift probe last"""
    if mode == MODE_LATTICE:
        my, mx = Py // t, Px // t
        out = [(dz, iy * t, ix * t) for dz in range(-Z, Z + 1) for iy in range(-my, my + 1) for ix in range(-mx, mx + 1)]
    else:
        out = [(centre[0] + jz, centre[1] + jy * t, centre[2] + jx * t) for jz in (-1, 0, 1) for jy in (-1, 0, 1) for jx in (-1, 0, 1)]
        out = [c if abs(c[0]) <= Z and abs(c[1]) <= Py and abs(c[2]) <= Px else None for c in out]
    return out + [(0, 0, 0)]


def tie_key(s, c):
    return (-s, c[0] * c[0], c[1] * c[1] + c[2] * c[2], c)


def select(sc, cands, probe):
    """(shift, score, N, found, lead): the best of the selectable candidates under the tie rule, (0, 0, 0) where none scores >= 0; lead = the
    best score minus the runner-up's (inf with one candidate)"""
    n_sel = len(cands) - 1 if probe else len(cands)
    ranked = sorted((tie_key(sc[i, 0], cands[i]), i) for i in range(n_sel) if cands[i] is not None)
    best = ranked[0][1]
    lead = sc[best, 0] - sc[ranked[1][1], 0] if len(ranked) > 1 else np.inf
    if sc[best, 0] >= 0:
        return tuple(cands[best]), sc[best, 0], int(sc[best, 1]), True, lead
    if probe:
        return (0, 0, 0), sc[-1, 0], int(sc[-1, 1]), False, lead
    return (0, 0, 0), -1.0, 0, False, lead


def search(qa, qb, window, Z, Py, Px, bins, levels, min_overlap):
    """-> dict(shift, score, zero, n, found, leads): `leads` holds every stage's lead of the best over the runner-up"""
    centre, leads, rec = (0, 0, 0), [], None
    for s in range(levels - 1, -1, -1):
        t = 1 << s
        cands = stage_candidates(MODE_LATTICE if s == levels - 1 else MODE_REFINE, t, Z, Py, Px, centre)
        sc = scores(histograms(qa, qb, window, cands, t, bins), qa.shape, qb.shape, window, cands, min_overlap)
        centre, best, n, found, lead = select(sc, cands, True)
        leads.append(float(lead))
        rec = dict(shift=centre, score=float(best), zero=float(sc[-1, 0]), n=n, found=found)
    rec['leads'] = leads
    return rec


def align(a, res_a, b, res_b, target_resolution, input_shape, params):
    """the whole of ops.align_volumes for raw volumes a, b [S,H,W]: search's record"""
    from tests import volume_loader_ref as R
    qs = []
    for x, res in ((a, res_a), (b, res_b)):
        RH, RW = R.out_extent(x.shape[1], res[0], target_resolution[0]), R.out_extent(x.shape[2], res[1], target_resolution[1])
        qs.append(quantise(x, RH, RW, params['bins'], params.get('percentiles', (0.5, 99.5)))[0])
    Py, Px = (int(np.floor(params['max_shift_mm'] / t)) for t in target_resolution)
    return search(qs[0], qs[1], input_shape[:2], params['max_slices'], Py, Px, params['bins'], params['levels'], params['min_overlap'])


# ---- CPU stand-ins of the entry points (argument lists of include/mmseg_hip.h without the stream) ----------------------------------------
CALLS = []          # one (entry point, mode, stride, C) per launch: the tests count them


def _count(mode, t, Z, Py, Px):
    if mode == MODE_REFINE:
        return 28
    if mode != MODE_LATTICE:
        return 0
    return (2 * Z + 1) * (2 * (Py // t) + 1) * (2 * (Px // t) + 1) + 1


def standin_stage_candidates(mode, t, Z, Py, Px):
    c = _count(mode, t, Z, Py, Px)
    return c if c <= 65535 else 0


def standin_workspace_bytes(C, bins):
    if not 1 <= C <= 65535 or not 2 <= bins <= 64:
        return 0
    return (C * bins * bins * 4 + 7) // 8 * 8 + C * 16


def _cands(cand, state, mode, t, Z, Py, Px, C):
    if mode == MODE_LIST:
        return [tuple(int(v) for v in row) for row in cand.numpy().reshape(-1, 3)[:C]]
    centre = tuple(int(v) for v in state[:3].tolist()) if mode == MODE_REFINE else (0, 0, 0)
    return stage_candidates(mode, t, Z, Py, Px, centre)


def standin_quantise(img, knots, q, S, H, W, RH, RW, bins):
    if not 2 <= bins <= 64:
        return 1
    lo, hi = knots.reshape(-1).tolist()
    q.copy_(torch.from_numpy(quantise_frames(I.frames(img.numpy(), RH, RW, np.float32), lo, hi, bins)[0]))
    return 0


def standin_histograms(qa, qb, cand, state, h, Sa, RHa, RWa, Sb, RHb, RWb, OH, OW, mode, t, Z, Py, Px, C, bins, aggregate):
    if mode != MODE_LIST and _count(mode, t, Z, Py, Px) != C:
        return 1
    CALLS.append(('histograms', mode, t, C))
    cands = _cands(cand, state, mode, t, Z, Py, Px, C)
    h.view(-1)[:C * bins * bins].copy_(torch.from_numpy(histograms(qa.numpy(), qb.numpy(), (OH, OW), cands, t, bins).astype(np.int32)).view(-1))
    return 0


def standin_scores(h, cand, state, out, Sa, RHa, RWa, Sb, RHb, RWb, OH, OW, mode, t, Z, Py, Px, C, bins, min_overlap):
    if not 0 <= min_overlap <= 1:
        return 1
    CALLS.append(('scores', mode, t, C))
    cands = _cands(cand, state, mode, t, Z, Py, Px, C)
    tables = h.numpy().reshape(-1)[:C * bins * bins].reshape(C, bins, bins).astype(np.int64)
    out.copy_(torch.from_numpy(scores(tables, (Sa, RHa, RWa), (Sb, RHb, RWb), (OH, OW), cands, min_overlap)))
    return 0


def standin_select(sc, cand, state, mode, t, Z, Py, Px, C):
    CALLS.append(('select', mode, t, C))
    cands = _cands(cand, state, mode, t, Z, Py, Px, C)
    s = sc.numpy()
    shift, best, n, found, _ = select(s, cands, mode != MODE_LIST)
    zero = float(state[4]) if mode == MODE_LIST else float(s[-1, 0])
    state.copy_(torch.tensor([shift[0], shift[1], shift[2], best, zero, n, float(found), float(state[7]) + 1.0], dtype=torch.float64))
    return 0


STANDINS = {'mmseg_align_stage_candidates': standin_stage_candidates, 'mmseg_align_workspace_bytes': standin_workspace_bytes,
            'mmseg_align_quantise': standin_quantise, 'mmseg_align_histograms': standin_histograms, 'mmseg_align_scores': standin_scores,
            'mmseg_align_select': standin_select}
