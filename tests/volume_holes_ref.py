"""Yardstick of tests/test_volume_holes.py: the enclosed holes of every organ of a label volume and the pass that fills them, written
from scipy alone.  Build-defined: the reference writes no segmentation, so this restates the rule of INTEGRATION.md section 5, and
shares no code with the product (csrc/postprocess.hip, multimodal_segmentation_amd/volume_predictor.py).

    mask        per organ k: M_k = (volume == values[k]); its complement is everything else, zeros, other organs and foreign grey
                values alike
    hole        ndimage.binary_fill_holes(M_k) & ~M_k with the default structure (faces only): the components of the complement that
                hold no border voxel.  mode '3d': on the volume, six neighbours, the border is the six faces; mode '2d': slice by
                slice, four neighbours, the border is the four edges of the slice
    fill        hole & (volume == 0) & (out == 0) becomes values[k], for k ascending; out starts as a copy of the volume.  Holes are
                those of the input; only zeros change; the lowest k wins
    stats       [K,3] = (ndimage.label(hole, faces)[1], voxels of values[k] before, voxels added); the structure is the in-plane one
                with mode '2d', so that a hole is counted once per slice

Also here: the TEST-ONLY CPU stand-ins of the entry points (installed into tests/cpu_backend._TABLE by the test's fixture) so that the
host logic above the C ABI runs without a GPU."""
import numpy as np
import torch
from scipy import ndimage as ndi

MODES = ('2d', '3d')
FACES = ndi.generate_binary_structure(3, 1)
IN_PLANE = FACES.copy()
IN_PLANE[0], IN_PLANE[2] = False, False


def holes(volume, v, mode):
    """bool [S,H,W]: the voxels of the complement of (volume == v) that organ v encloses"""
    assert mode in MODES
    mask = np.asarray(volume) == v
    if mode == '3d':
        filled = ndi.binary_fill_holes(mask)
    else:
        filled = np.stack([ndi.binary_fill_holes(m) for m in mask]) if mask.shape[0] else mask.copy()
    return filled & ~mask


def count(hole, mode):
    return int(ndi.label(hole, FACES if mode == '3d' else IN_PLANE)[1])


def fill_holes(volume, values, mode):
    """(filled uint8 [S,H,W], stats int32 [K,3])"""
    volume = np.asarray(volume)
    out = volume.copy()
    stats = np.zeros((len(values), 3), np.int32)
    for k, v in enumerate(values):
        hole = holes(volume, v, mode)
        fill = hole & (volume == 0) & (out == 0)
        out[fill] = v
        stats[k] = (count(hole, mode), np.count_nonzero(volume == v), np.count_nonzero(fill))
    return out, stats


# ---- CPU stand-ins of the entry points (argument lists of include/mmseg_hip.h without the stream) ----------------------------------------
def standin_workspace_bytes(S, H, W, K):
    return 8


def standin_fill_label_holes(label, values, out, stats, ws, S, H, W, K, per_slice):
    o, s = fill_holes(label.numpy().reshape(S, H, W), [int(v) for v in values], '2d' if per_slice else '3d')
    out.copy_(torch.from_numpy(o).reshape(out.shape))
    stats.copy_(torch.from_numpy(s))
    return 0


STANDINS = {'mmseg_fill_label_holes_workspace_bytes': standin_workspace_bytes, 'mmseg_fill_label_holes': standin_fill_label_holes}
