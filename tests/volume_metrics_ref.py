"""Yardstick of tests/test_volume_metrics.py: the scores in mm of a predicted label volume (RAVD, ASSD, MSSD), written from scipy
alone, in fp64.  Build-defined: the reference scores Dice only, so this restates the rules of INTEGRATION.md section 5, and shares no
code with the product (csrc/postprocess.hip, multimodal_segmentation_amd/volume_predictor.py).

    problems    K + 1 per volume: k < K is `volume == values[k]`, K is "equals any of values" (every other grey value is background)
    surface     m & ~binary_erosion(m, generate_binary_structure(3, 1), border_value=0): a foreground voxel with a face neighbour that
                is background or outside the volume
    distance    distance_transform_edt(~surface, sampling=(dz, dy, dx)): mm to the nearest surface voxel; +inf without one
    table       [K+1,6] = nP, nT, |surface(P)|, |surface(T)|, sum and max of d(v, T) over surface(P) and d(v, P) over surface(T); the
                last two nan when either surface is empty
    chaos       RAVD = 100 |nP - nT| / nT (nan when nT = 0), ASSD = sum / (|surface(P)| + |surface(T)|), MSSD = max

Also here: the TEST-ONLY CPU stand-ins of the entry points (installed into tests/cpu_backend._TABLE by the test's fixture) so that the
host logic above the C ABI runs without a GPU."""
import numpy as np
import torch
from scipy import ndimage as ndi

STRUCTURE = ndi.generate_binary_structure(3, 1)


def problems(volume, values):
    """[K+1,S,H,W] bool"""
    volume = np.asarray(volume)
    return np.stack([volume == v for v in values] + [np.isin(volume, list(values))], axis=0)


def surface(mask):
    mask = np.asarray(mask, bool)
    return mask & ~ndi.binary_erosion(mask, STRUCTURE, border_value=0)


def distance_map(sites, spacing):
    """fp64 [S,H,W]: mm to the nearest True voxel of `sites`"""
    sites = np.asarray(sites, bool)
    if not sites.any():
        return np.full(sites.shape, np.inf)
    return ndi.distance_transform_edt(~sites, sampling=tuple(float(s) for s in spacing))


def metrics_table(pred, truth, values, spacing):
    out = np.zeros((len(values) + 1, 6), np.float64)
    for k, (p, t) in enumerate(zip(problems(pred, values), problems(truth, values))):
        sp, st = surface(p), surface(t)
        out[k, :4] = p.sum(), t.sum(), sp.sum(), st.sum()
        if sp.any() and st.any():
            d = np.concatenate([distance_map(st, spacing)[sp], distance_map(sp, spacing)[st]])
            out[k, 4], out[k, 5] = d.sum(), d.max()
        else:
            out[k, 4:] = np.nan
    return out


def chaos_metrics(pred, truth, values, spacing):
    """[K+1,3] = RAVD (%), ASSD (mm), MSSD (mm); the union of the organs is the last row"""
    t = metrics_table(pred, truth, values, spacing)
    with np.errstate(divide='ignore', invalid='ignore'):
        ravd = np.where(t[:, 1] > 0, 100.0 * np.abs(t[:, 0] - t[:, 1]) / t[:, 1], np.nan)
        assd = t[:, 4] / (t[:, 2] + t[:, 3])
    return np.stack([ravd, assd, t[:, 5]], axis=1)


# ---- CPU stand-ins of the entry points (argument lists of include/mmseg_hip.h without the stream) ----------------------------------------
def standin_label_surface(label, values, surf, counts, S, H, W, K):
    p = problems(label.numpy().reshape(S, H, W), [int(v) for v in values])
    s = np.stack([surface(m) for m in p], axis=0)
    surf.copy_(torch.from_numpy(s.astype(np.uint8)).reshape(surf.shape))
    if counts is not None:
        counts.copy_(torch.from_numpy(np.stack([p.reshape(K + 1, -1).sum(1), s.reshape(K + 1, -1).sum(1)], axis=1).astype(np.int32)))
    return 0


def standin_distance_to_sites(sites, out, tmp, S, H, W, dz, dy, dx):
    out.copy_(torch.from_numpy(distance_map(sites.numpy().reshape(S, H, W) != 0, (dz, dy, dx))).reshape(out.shape))
    return 0


def standin_workspace_doubles(S, H, W, K):
    return 1


def standin_surface_metrics(pred, truth, values, table, ws, S, H, W, K, dz, dy, dx):
    t = metrics_table(pred.numpy().reshape(S, H, W), truth.numpy().reshape(S, H, W), [int(v) for v in values], (dz, dy, dx))
    table.copy_(torch.from_numpy(t))
    return 0


STANDINS = {'mmseg_label_surface': standin_label_surface, 'mmseg_distance_to_sites': standin_distance_to_sites,
            'mmseg_surface_metrics_workspace_doubles': standin_workspace_doubles, 'mmseg_surface_metrics': standin_surface_metrics}
