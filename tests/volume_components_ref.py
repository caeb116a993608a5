"""Yardstick of tests/test_volume_components.py: the connected components of every organ of a label volume and the filter that keeps
each organ's largest one, written from scipy alone.  Build-defined: the reference writes no segmentation, so this restates the rule
of INTEGRATION.md section 5, and shares no code with the product (csrc/postprocess.hip, multimodal_segmentation_amd/volume_predictor.py).

    neighbours  generate_binary_structure(3, 1) for connectivity 6 (faces), generate_binary_structure(3, 3) for 26 (faces, edges, corners)
    components  per organ v: ndimage.label(volume == v, structure); a voxel whose grey value is no organ's gets 0
    canonical   component id -> 1 + the smallest linear index (s * H * W + y * W + x) of its voxels
    largest     sizes from bincount; the largest component wins, of equally large ones the one with the smallest canonical id
    filter      organ voxels outside their organ's winner become 0, everything else is copied
    stats       [K,3] = (number of components, voxels of the organ before, voxels kept); (0, 0, 0) for an organ without voxels

Also here: the TEST-ONLY CPU stand-ins of the entry points (installed into tests/cpu_backend._TABLE by the test's fixture) so that the
host logic above the C ABI runs without a GPU."""
import numpy as np
import torch
from scipy import ndimage as ndi


def structure(connectivity):
    return ndi.generate_binary_structure(3, {6: 1, 26: 3}[connectivity])


def organ_components(volume, v, connectivity):
    """(canonical int64 [S,H,W] with 0 outside the organ, sizes {canonical id: voxels})"""
    volume = np.asarray(volume)
    lab, n = ndi.label(volume == v, structure(connectivity))
    canon = np.zeros(volume.shape, np.int64)
    if n == 0:
        return canon, {}
    flat = lab.reshape(-1)
    index = np.arange(flat.size, dtype=np.int64)
    first = np.full(n + 1, flat.size, np.int64)
    np.minimum.at(first, flat, index)
    ids = first + 1
    ids[0] = 0
    canon = ids[flat].reshape(volume.shape)
    sizes = np.bincount(flat, minlength=n + 1)
    return canon, {int(ids[i]): int(sizes[i]) for i in range(1, n + 1)}


def components(volume, values, connectivity):
    """int32 [S,H,W]: 0, or 1 + the smallest linear index of the voxel's component"""
    out = np.zeros(np.asarray(volume).shape, np.int64)
    for v in values:
        canon, _ = organ_components(volume, v, connectivity)
        out = np.where(canon > 0, canon, out)
    return out.astype(np.int32)


def sorted_sizes(volume, v, connectivity):
    """component sizes of one organ, largest first"""
    return sorted(organ_components(volume, v, connectivity)[1].values(), reverse=True)


def keep_largest(volume, values, connectivity):
    """(filtered uint8 [S,H,W], stats int32 [K,3])"""
    volume = np.asarray(volume)
    out = volume.copy()
    stats = np.zeros((len(values), 3), np.int32)
    for k, v in enumerate(values):
        canon, sizes = organ_components(volume, v, connectivity)
        if not sizes:
            continue
        winner = min(sizes, key=lambda i: (-sizes[i], i))
        out[(canon > 0) & (canon != winner)] = 0
        stats[k] = (len(sizes), sum(sizes.values()), sizes[winner])
    return out, stats


# ---- CPU stand-ins of the entry points (argument lists of include/mmseg_hip.h without the stream) ----------------------------------------
def standin_label_components(label, values, comp, S, H, W, K, connectivity):
    c = components(label.numpy().reshape(S, H, W), [int(v) for v in values], connectivity)
    comp.copy_(torch.from_numpy(c).reshape(comp.shape))
    return 0


def standin_workspace_bytes(S, H, W, K):
    return 8


def standin_keep_largest_components(label, values, out, stats, ws, S, H, W, K, connectivity):
    o, s = keep_largest(label.numpy().reshape(S, H, W), [int(v) for v in values], connectivity)
    out.copy_(torch.from_numpy(o).reshape(out.shape))
    stats.copy_(torch.from_numpy(s))
    return 0


STANDINS = {'mmseg_label_components': standin_label_components, 'mmseg_keep_largest_workspace_bytes': standin_workspace_bytes,
            'mmseg_keep_largest_components': standin_keep_largest_components}
