"""Yardstick of tests/test_volume_robust.py: HD(q), a percentile of the surface distances, and NSD(tau), the surface Dice at a tolerance,
of a predicted label volume, written from numpy / scipy alone, in fp64.  Build-defined: the rules are those of INTEGRATION.md section 5,
and no code is shared with the product (csrc/postprocess.hip, multimodal_segmentation_amd/volume_predictor.py); `problems`, `surface` and
`distance_map` are those of tests/volume_metrics_ref.py.

    D              per binary problem the distances d(v, T) over surface(P) and d(v, P) over surface(T), one multiset; N = |D|
    robust_table   [K+1,8] = metrics_table's six columns, |{x in D : x <= tau}|, numpy.percentile(D, q); the last two nan when either
                   surface is empty
    robust_scores  [K+1,2] = HD(q) = column 8, NSD(tau) = column 7 / N
    order_stats    what mmseg_masked_select returns for a list: N, the count, numpy.percentile, D_(lo), D_(hi) with
                   h = (N - 1) * (q / 100), lo = floor(h), hi = min(lo + 1, N - 1) over numpy.sort

Also here: the TEST-ONLY CPU stand-ins of the four entry points (installed into tests/cpu_backend._TABLE by the test's fixture) so that
the host logic above the C ABI runs without a GPU."""
import math

import numpy as np
import torch

from tests import volume_metrics_ref as M


def distances(p, t, spacing):
    """the multiset D of one binary problem (masks p, t), or None when either surface is empty"""
    sp, st = M.surface(p), M.surface(t)
    if not (sp.any() and st.any()):
        return None
    return np.concatenate([M.distance_map(st, spacing)[sp], M.distance_map(sp, spacing)[st]])


def robust_table(pred, truth, values, spacing, percentile, tolerance):
    out = np.full((len(values) + 1, 8), np.nan)
    out[:, :6] = M.metrics_table(pred, truth, values, spacing)
    for k, (p, t) in enumerate(zip(M.problems(pred, values), M.problems(truth, values))):
        d = distances(p, t, spacing)
        if d is not None:
            out[k, 6], out[k, 7] = np.count_nonzero(d <= tolerance), np.percentile(d, percentile)
    return out


def robust_scores(pred, truth, values, spacing, percentile, tolerance):
    """[K+1,2] = HD(percentile) in mm, NSD(tolerance); the union of the organs is the last row"""
    t = robust_table(pred, truth, values, spacing, percentile, tolerance)
    with np.errstate(divide='ignore', invalid='ignore'):
        return np.stack([t[:, 7], t[:, 6] / (t[:, 2] + t[:, 3])], axis=1)


def ranks(n, percentile):
    """(lo, hi, h - lo) of the percentile's linear rule over n values"""
    h = (n - 1) * (float(percentile) / 100.0)          # numpy's order of evaluation: the quantile q / 100 first
    lo = min(int(math.floor(h)), n - 1)
    return lo, min(lo + 1, n - 1), h - lo


def order_stats(d, percentile, tolerance):
    """fp64 [5] = N, |{x <= tolerance}|, numpy.percentile(d), D_(lo), D_(hi); nan for an empty list"""
    d = np.sort(np.asarray(d, np.float64).reshape(-1))
    if d.size == 0:
        return np.asarray([0.0, 0.0, np.nan, np.nan, np.nan])
    lo, hi, _ = ranks(d.size, percentile)
    return np.asarray([d.size, np.count_nonzero(d <= tolerance), np.percentile(d, percentile), d[lo], d[hi]], np.float64)


# ---- CPU stand-ins of the entry points (argument lists of include/mmseg_hip.h without the stream) ----------------------------------------
def standin_masked_select_workspace_doubles(n):
    return 2 * n + 1 if 0 <= n < 2 ** 31 else 0


def standin_masked_select(a, ma, b, mb, n, percentile, tolerance, out, ws):
    a, ma, b, mb = (x.numpy().reshape(-1) for x in (a, ma, b, mb))
    out.copy_(torch.from_numpy(order_stats(np.concatenate([a[ma != 0], b[mb != 0]]), percentile, tolerance)))
    return 0


def standin_surface_scores_workspace_doubles(S, H, W, K):
    return 1


def standin_surface_scores(pred, truth, values, table, ws, S, H, W, K, dz, dy, dx, percentile, tolerance):
    t = robust_table(pred.numpy().reshape(S, H, W), truth.numpy().reshape(S, H, W), [int(v) for v in values], (dz, dy, dx), percentile,
                     tolerance)
    table.copy_(torch.from_numpy(t))
    return 0


STANDINS = {'mmseg_masked_select_workspace_doubles': standin_masked_select_workspace_doubles,
            'mmseg_masked_select': standin_masked_select,
            'mmseg_surface_scores_workspace_doubles': standin_surface_scores_workspace_doubles,
            'mmseg_surface_scores': standin_surface_scores}
