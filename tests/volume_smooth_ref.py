"""Yardstick of tests/test_volume_smooth.py: every organ of a label volume opened, closed or smoothed by a ball in mm, written from
scipy and exact rational arithmetic alone.  Build-defined: the reference writes no segmentation, so this restates the rule of
INTEGRATION.md section 5, and shares no code with the product (csrc/postprocess.hip, multimodal_segmentation_amd/volume_predictor.py).

    ball        B = { o : (dx ox)^2 + (dy oy)^2 + (dz oz)^2 <= r^2 }, every term an exact fraction of the fp64 spacings and radius; with
                extent '2d' only oz == 0.  `margin` is the smallest relative distance of any t(o) within reach + 1 to r^2: where it is
                above 1e-9, no rounding of the product's fp64 evaluation can decide a membership
    erode       ndimage.binary_erosion(X, B, border_value=1): what lies outside the volume is no background
    dilate      ndimage.binary_dilation(X, B)
    open, close dilate(erode(X)), a subset of X; erode(dilate(X)), a superset of X
    labels      open: a voxel of values[k] outside open(volume == values[k]) becomes 0.  close: fill = close(volume == values[k]) &
                (volume == 0) & (out == 0) becomes values[k], for k ascending; out starts as a copy of the volume.  smooth: open, then
                close with the opened volume as its input
    stats       [K,3] = (voxels of values[k] in the input, voxels removed, voxels added)

Also here: the TEST-ONLY CPU stand-ins of the entry points (installed into tests/cpu_backend._TABLE by the test's fixture) so that the
host logic above the C ABI runs without a GPU."""
import itertools
import math
from fractions import Fraction

import numpy as np
import torch
from scipy import ndimage as ndi

OPS = ('open', 'close', 'smooth')
EXTENTS = ('2d', '3d')
MAX_REACH = 32


def _axes(spacing, extent):
    """the spacings as fractions, None for the slice axis with extent '2d'"""
    assert extent in EXTENTS and len(spacing) == 3
    return [None if (extent == '2d' and i == 0) else Fraction(float(s)) for i, s in enumerate(spacing)]


def reach(spacing, r, extent):
    """floor(r / spacing) per axis (0 for the slice axis with '2d'), in exact arithmetic"""
    return tuple(0 if s is None else int(Fraction(float(r)) / s) for s in _axes(spacing, extent))


def _t(axes, o):
    return sum(((s * n) ** 2 for s, n in zip(axes, o) if s is not None), Fraction(0))


def ball(spacing, r, extent):
    """bool [2 rz + 1, 2 ry + 1, 2 rx + 1], centred"""
    axes, rr = _axes(spacing, extent), Fraction(float(r)) ** 2
    n = reach(spacing, r, extent)
    B = np.zeros(tuple(2 * m + 1 for m in n), bool)
    for o in itertools.product(*(range(-m, m + 1) for m in n)):
        B[tuple(a + m for a, m in zip(o, n))] = _t(axes, o) <= rr
    assert B[n] and np.array_equal(B, B[::-1, ::-1, ::-1])
    return B


def margin(spacing, r, extent):
    """the smallest |t(o) - r^2| / r^2 over the offsets within reach + 1 per axis in use"""
    axes, rr = _axes(spacing, extent), Fraction(float(r)) ** 2
    n = [0 if s is None else m + 1 for s, m in zip(axes, reach(spacing, r, extent))]
    return float(min(abs(_t(axes, o) - rr) / rr for o in itertools.product(*(range(0, m + 1) for m in n))))


def erode(X, B):
    return ndi.binary_erosion(X, B, border_value=1) if X.size else X.copy()


def dilate(X, B):
    return ndi.binary_dilation(X, B) if X.size else X.copy()


def opened(X, B):
    return dilate(erode(X, B), B)


def closed(X, B):
    return erode(dilate(X, B), B)


def open_label(volume, values, B):
    volume = np.asarray(volume)
    out, stats = volume.copy(), np.zeros((len(values), 3), np.int32)
    for k, v in enumerate(values):
        X = volume == v
        gone = X & ~opened(X, B)
        out[gone] = 0
        stats[k] = (np.count_nonzero(X), np.count_nonzero(gone), 0)
    return out, stats


def close_label(volume, values, B):
    volume = np.asarray(volume)
    out, stats = volume.copy(), np.zeros((len(values), 3), np.int32)
    for k, v in enumerate(values):
        X = volume == v
        fill = closed(X, B) & (volume == 0) & (out == 0)
        out[fill] = v
        stats[k] = (np.count_nonzero(X), 0, np.count_nonzero(fill))
    return out, stats


def smooth_label(volume, values, spacing, r, op, extent):
    """(uint8 [S,H,W], stats int32 [K,3])"""
    assert op in OPS
    B = ball(spacing, r, extent)
    if op == 'open':
        return open_label(volume, values, B)
    if op == 'close':
        return close_label(volume, values, B)
    first, s1 = open_label(volume, values, B)
    out, s2 = close_label(first, values, B)
    return out, np.stack([s1[:, 0], s1[:, 1], s2[:, 2]], axis=1).astype(np.int32)


def claims(volume, values, spacing, r, extent):
    """int [S,H,W]: by how many organs' closings a zero of the volume is claimed"""
    B = ball(spacing, r, extent)
    volume = np.asarray(volume)
    return sum((closed(volume == v, B) & (volume == 0)).astype(np.int32) for v in values)


def edt_within(X, spacing, r, extent):
    """bool: the voxels within r mm of a voxel of X, by scipy's exact Euclidean transform; X must hold a voxel (per slice with '2d')"""
    if extent == '3d':
        return ndi.distance_transform_edt(~X, sampling=[float(s) for s in spacing]) <= r
    return np.stack([ndi.distance_transform_edt(~x, sampling=[float(s) for s in spacing[1:]]) <= r if x.any() else np.zeros_like(x)
                     for x in X])


# ---- CPU stand-ins of the entry points (argument lists of include/mmseg_hip.h without the stream) ----------------------------------------
def standin_workspace_bytes(S, H, W, K):
    return 8


def standin_smooth_label(label, values, out, stats, ws, S, H, W, K, dz, dy, dx, radius, op, per_slice):
    extent = '2d' if per_slice else '3d'
    used = (dy, dx) if per_slice else (dz, dy, dx)
    if not all(math.isfinite(s) and s > 0 for s in used + (radius,)) or max(reach((dz, dy, dx), radius, extent)) > MAX_REACH:
        return 1
    o, s = smooth_label(label.numpy().reshape(S, H, W), [int(v) for v in values], (dz, dy, dx), radius, OPS[op], extent)
    out.copy_(torch.from_numpy(o).reshape(out.shape))
    stats.copy_(torch.from_numpy(s))
    return 0


STANDINS = {'mmseg_smooth_label_workspace_bytes': standin_workspace_bytes, 'mmseg_smooth_label': standin_smooth_label}
