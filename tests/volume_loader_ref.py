"""Yardstick of tests/test_volume_loader.py: an fp64 numpy / scipy restatement of the volume preprocessing of the reference's CHAOS
loader (loaders/chaos.py:242-246, 248-264, 303-319, 324-343), built on scipy.ndimage.map_coordinates and on the project's own
utils/data_utils.rescale / crop_same, which tests/test_data_pipeline.py pins to reference-generated fixtures.  It shares no code
with loaders/volume_folder.py or csrc/preprocess.hip.

`skimage.transform.rescale(order, mode='constant', preserve_range=True)` without anti-aliasing, as the reference's era had it,
restated from memory: output extent round(in * scale) (numpy's round, half to even); resampled pixel d reads source coordinate
(d + 0.5) * (in / out) - 0.5; order 1 is bilinear, order 0 takes the nearest pixel with half rounded away from zero; everything
outside the source is 0.  map_coordinates(mode='constant') decides "outside" on the coordinate: outside [0, in - 1] gives 0.

Also here: the TEST-ONLY CPU stand-ins of the mmseg_preprocess_* entry points (installed into tests/cpu_backend._TABLE by the test's
fixture), so that the host logic above the C ABI runs without a GPU.  They apply the index map the host passes to the kernels, on
top of the restatement's resampling."""
import importlib.util
import os

import numpy as np
import torch
from scipy import ndimage as ndi

from multimodal_segmentation_amd.utils import data_utils

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def tool():
    """tools/make_volume_folder.py as a module (tools/ is a folder of scripts, not a package)"""
    spec = importlib.util.spec_from_file_location('make_volume_folder', os.path.join(ROOT, 'tools', 'make_volume_folder.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


# ---- the restatement ---------------------------------------------------------------------------------------------------------------
def out_extent(n, old_res, new_res):
    return int(np.round(n * (old_res / new_res)))


def source_coordinates(n_in, n_out):
    return (np.arange(n_out, dtype=np.float64) + 0.5) * (n_in / n_out) - 0.5


def resample(slice2d, old_res, new_res, order):
    H, W = slice2d.shape
    rows = source_coordinates(H, out_extent(H, old_res[0], new_res[0]))
    cols = source_coordinates(W, out_extent(W, old_res[1], new_res[1]))
    grid = np.meshgrid(rows, cols, indexing='ij')
    return ndi.map_coordinates(slice2d.astype(np.float64), grid, order=order, mode='constant', cval=0.0, prefilter=False)


def preprocess(image, label, old_res, new_res, label_values, out_hw):
    """image, label [S,H,W] -> (images [S,OH,OW,1], masks [S,OH,OW,K]) in fp64, in the reference's order: resample, split the labels,
    rescale every slice to [-1, 1] over its whole resampled frame, crop / pad"""
    imgs = np.stack([resample(s, old_res, new_res, 1) for s in image])[..., None]
    labs = np.stack([resample(s, old_res, new_res, 0) for s in label])
    masks = np.stack([(labs == v).astype(np.float64) for v in label_values], axis=-1)
    imgs = np.concatenate([data_utils.rescale(imgs[i:i + 1], -1, 1) for i in range(imgs.shape[0])])
    [imgs], [masks] = data_utils.crop_same([imgs], [masks], tuple(out_hw))
    return imgs, masks


def undecidable_pixels(n_in, n_out, tol=1e-6):
    """number of resampled indices along one axis whose source coordinate lies within `tol` of a decision point without sitting on
    it exactly where exactness is well defined: a half-integer (the nearest-neighbour tie) or, unless in == out (exact integer
    coordinates), the borders 0 and in - 1 of the strict inside test"""
    c = source_coordinates(n_in, n_out)
    ties = np.abs((c - np.floor(c)) - 0.5) < tol
    border = np.zeros_like(ties) if n_in == n_out else (np.abs(c) < tol) | (np.abs(c - (n_in - 1)) < tol)
    return int(np.count_nonzero(ties | border))


# ---- CPU stand-ins of the entry points (argument lists of include/mmseg_hip.h without the stream) ----------------------------------------
def _resample_to(slice2d, RH, RW, order):
    H, W = slice2d.shape
    grid = np.meshgrid(source_coordinates(H, RH), source_coordinates(W, RW), indexing='ij')
    return ndi.map_coordinates(slice2d.astype(np.float64), grid, order=order, mode='constant', cval=0.0, prefilter=False)


def _index_map(lo, kept, before, n_out):
    return lo + np.clip(np.arange(n_out) - before, 0, kept - 1)


def standin_workspace_floats(S, RH, RW):
    return 2 * S


def standin_minmax(img, ws, S, H, W, RH, RW):
    x = img.numpy()
    for s in range(S):
        r = _resample_to(x[s], RH, RW, 1).astype(np.float32)
        ws[2 * s], ws[2 * s + 1] = float(r.min()), float(r.max())
    return 0


def standin_image(img, ws, out, S, H, W, RH, RW, OH, OW, lo_r, kept_r, before_r, lo_c, kept_c, before_c, C, ch):
    x = img.numpy()
    ir, ic = _index_map(lo_r, kept_r, before_r, OH), _index_map(lo_c, kept_c, before_c, OW)
    for s in range(S):
        r = _resample_to(x[s], RH, RW, 1).astype(np.float32)
        lo, hi = np.float32(float(ws[2 * s])), np.float32(float(ws[2 * s + 1]))
        v = r[ir][:, ic]
        out[s, :, :, ch] = torch.from_numpy(np.full_like(v, -1) if hi == lo else np.float32(2) * (v - lo) / (hi - lo) - np.float32(1))
    return 0


def standin_label(lab, values, out, S, H, W, RH, RW, OH, OW, lo_r, kept_r, before_r, lo_c, kept_c, before_c, C, ch0, K):
    x = lab.numpy()
    ir, ic = _index_map(lo_r, kept_r, before_r, OH), _index_map(lo_c, kept_c, before_c, OW)
    for s in range(S):
        g = _resample_to(x[s], RH, RW, 0)[ir][:, ic]
        for k in range(K):
            out[s, :, :, ch0 + k] = torch.from_numpy((g == int(values[k])).astype(np.float32))
    return 0


STANDINS = {'mmseg_preprocess_workspace_floats': standin_workspace_floats, 'mmseg_preprocess_minmax': standin_minmax,
            'mmseg_preprocess_image': standin_image, 'mmseg_preprocess_label': standin_label}
