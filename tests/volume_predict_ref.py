"""Yardstick of tests/test_volume_predict.py: an fp64 numpy / scipy restatement of the way back from the network's frame to a volume's
own grid (csrc/postprocess.hip, multimodal_segmentation_amd/volume_predictor.py).  Build-defined: the reference writes no segmentation,
so this restates the rule of INTEGRATION.md section 5, and shares no code with the product.

    coordinate   raw index d of n -> (d + 0.5) * (R / n) - 0.5 in fp64, clamped into [0, R - 1].  IEEE multiplication, division and
                 subtraction are correctly rounded here and on the device (which forbids contraction), so the window test and the
                 order-0 tap floor(coord + 0.5) agree bit for bit, half-integer ties included.
    window       coord outside [lo, lo + kept - 1] on either axis -> 0
    order 0      the container is indexed with the taps (limited to the window): the sampled value is an input value
    order 1      per organ channel the crop / pad is undone by index (before, kept) and scipy.ndimage.map_coordinates(order=1,
                 mode='nearest', prefilter=False) samples the kept window at coord - lo, in fp64
    0.5 rule     the lowest organ k whose sampled probability is > 0.5 gives values[k]; none -> 0
A pixel inside the window is UNDECIDABLE (order 1 only) when an organ's fp64 probability lies within 1e-5 of 0.5: the device's fp32
bilinear expression differs from fp64 by a few 1e-7 on values in [0, 1].

Also here: the TEST-ONLY CPU stand-ins of mmseg_restore_label / mmseg_label_overlap (installed into tests/cpu_backend._TABLE by the
test's fixture) so that the host logic above the C ABI runs without a GPU."""
import numpy as np
import torch
from scipy import ndimage as ndi

from multimodal_segmentation_amd import costs

UNDECIDABLE = 1e-5
CAP = 1e-3          # share of the raw pixels of a case that may be undecidable: a condition on the inputs, not a measurement


def raw_coordinates(n_raw, R):
    c = (np.arange(n_raw, dtype=np.float64) + 0.5) * (R / n_raw) - 0.5
    return np.clip(c, 0.0, float(R - 1))


def window_mask(raw_hw, resampled, rows, cols):
    """[H,W] bool: raw pixels whose clamped coordinate lies inside the kept window on both axes"""
    cy, cx = raw_coordinates(raw_hw[0], resampled[0]), raw_coordinates(raw_hw[1], resampled[1])
    iy = (cy >= rows[0]) & (cy <= rows[0] + rows[1] - 1)
    ix = (cx >= cols[0]) & (cx <= cols[0] + cols[1] - 1)
    return iy[:, None] & ix[None, :]


def sample(prob, K, raw_hw, resampled, rows, cols, order):
    """prob [S,OH,OW,C] -> fp64 [S,H,W,K]: the organ channels sampled at every raw pixel (meaningless outside the window)"""
    prob = np.asarray(prob, np.float64)
    cy, cx = raw_coordinates(raw_hw[0], resampled[0]), raw_coordinates(raw_hw[1], resampled[1])
    (lo_r, kept_r, before_r), (lo_c, kept_c, before_c) = rows, cols
    out = np.zeros((prob.shape[0], raw_hw[0], raw_hw[1], K), np.float64)
    if order == 0:
        ty = np.clip(np.floor(cy + 0.5).astype(np.int64), lo_r, lo_r + kept_r - 1) - lo_r + before_r
        tx = np.clip(np.floor(cx + 0.5).astype(np.int64), lo_c, lo_c + kept_c - 1) - lo_c + before_c
        return prob[:, ty][:, :, tx][..., :K]
    grid = np.meshgrid(cy - lo_r, cx - lo_c, indexing='ij')
    for s in range(prob.shape[0]):
        for k in range(K):
            kept = prob[s, before_r:before_r + kept_r, before_c:before_c + kept_c, k]
            out[s, ..., k] = ndi.map_coordinates(kept, grid, order=1, mode='nearest', prefilter=False)
    return out


def restore(prob, values, raw_hw, resampled, rows, cols, order):
    """-> (label [S,H,W] uint8, undecidable [S,H,W] bool)"""
    K = len(values)
    v = sample(prob, K, raw_hw, resampled, rows, cols, order)
    inside = window_mask(raw_hw, resampled, rows, cols)[None]
    label = np.zeros(v.shape[:3], np.uint8)
    for k in reversed(range(K)):          # the lowest k above 0.5 is written last
        label[v[..., k] > 0.5] = values[k]
    label[np.broadcast_to(~inside, label.shape)] = 0
    undecidable = np.zeros(label.shape, bool)
    if order == 1:
        undecidable = (np.abs(v - 0.5) < UNDECIDABLE).any(-1) & inside
    return label, undecidable


def one_hot(label, values):
    return np.stack([(label == v).astype(np.float64) for v in values], axis=-1)


def dice(truth, pred, values):
    """(joint, [per organ]) of two uint8 volumes [S,H,W]: costs.dice on one-hot arrays"""
    t, p = one_hot(truth, values), one_hot(pred, values)
    return costs.dice(t, p), [costs.dice(t[..., k:k + 1], p[..., k:k + 1]) for k in range(len(values))]


def overlap_counts(pred, truth, values):
    out = np.zeros((pred.shape[0], len(values), 3), np.int64)
    for k, v in enumerate(values):
        p, t = pred == v, truth == v
        out[:, k, 0], out[:, k, 1], out[:, k, 2] = p.sum((1, 2)), t.sum((1, 2)), (p & t).sum((1, 2))
    return out


# ---- CPU stand-ins of the entry points (argument lists of include/mmseg_hip.h without the stream) ----------------------------------------
def standin_restore_label(prob, values, out, S, H, W, RH, RW, OH, OW, lo_r, kept_r, before_r, lo_c, kept_c, before_c, C, K, order):
    label, _ = restore(prob.numpy(), [int(v) for v in values], (H, W), (RH, RW), (lo_r, kept_r, before_r), (lo_c, kept_c, before_c), order)
    out.copy_(torch.from_numpy(label))
    return 0


def standin_label_overlap(pred, truth, values, counts, S, n, K):
    c = overlap_counts(pred.numpy().reshape(S, 1, n), truth.numpy().reshape(S, 1, n), [int(v) for v in values])
    counts.copy_(torch.from_numpy(c.astype(np.int32)))
    return 0


STANDINS = {'mmseg_restore_label': standin_restore_label, 'mmseg_label_overlap': standin_label_overlap}
