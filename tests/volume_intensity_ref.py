"""Yardstick of tests/test_volume_intensity.py: a numpy restatement of the percentile-window and landmark intensity normalisation
(the definition is in include/mmseg_hip.h), on top of the resampling of tests/volume_loader_ref.py.  It shares no code with
loaders/volume_folder.py or csrc/preprocess.hip.

Population of a (volume, modality): the bilinearly resampled values over the whole RH x RW frame of every slice.  A segment is one
slice (G = S segments of N = RH * RW values) or the volume (G = 1, N = S * RH * RW).  Knot x_k of a segment is its order statistic of
rank floor((N - 1) * (q_k / 100)) -- np.sort(segment)[rank], no interpolation.  A value v maps through its segment's knots x and the
shared targets y: v <= x_0 -> y_0, v >= x_{K-1} -> y_{K-1}, otherwise with k the largest index that has x_k < v:
min(y_k + (v - x_k) * ((y_{k+1} - y_k) / (x_{k+1} - x_k)), y_{k+1}).  Everything is evaluated in the dtype asked for (fp64: the
yardstick; fp32: what the arithmetic of the kernels amounts to).

Also here: the TEST-ONLY CPU stand-ins of the three mmseg_preprocess_quantiles* / _image_map entry points, installed into
tests/cpu_backend._TABLE by the test's fixture on top of the existing ones."""
import numpy as np
import torch

from tests import volume_loader_ref as R

WINDOW_PERCENTILES = (0.5, 99.5)
LANDMARK_PERCENTILES = (1, 10, 20, 30, 40, 50, 60, 70, 80, 90, 99)


def ranks(n, percentiles):
    return [int(np.floor((n - 1) * (q / 100.0))) for q in percentiles]


def frames(image, RH, RW, dtype=np.float64):
    """[S,RH,RW]: every slice resampled (fp64 interpolation), rounded to `dtype`"""
    return np.stack([R._resample_to(s, RH, RW, 1) for s in image]).astype(dtype)


def knots(fr, rk, per_volume):
    """[G,K] of frames fr [S,RH,RW], in fr's dtype"""
    segments = fr.reshape(1, -1) if per_volume else fr.reshape(fr.shape[0], -1)
    return np.stack([np.sort(seg)[np.asarray(rk)] for seg in segments])


def apply_map(v, x, y):
    """the map of the definition, element-wise, in v's dtype; x [K] the segment's knots, y [K] the targets"""
    dt = v.dtype
    x, y = np.asarray(x, dt), np.asarray(y, dt)
    K = len(x)
    k = np.clip(np.searchsorted(x, v, side='left') - 1, 0, K - 2)          # the largest k with x_k < v, where one exists below K - 1
    with np.errstate(divide='ignore', invalid='ignore'):
        slope = ((y[1:] - y[:-1]) / (x[1:] - x[:-1])).astype(dt)
        inner = np.minimum(y[k] + (v - x[k]) * slope[k], y[k + 1]).astype(dt)
    return np.where(v <= x[0], y[0], np.where(v >= x[-1], y[-1], inner)).astype(dt)


def normalise(fr, rk, y, per_volume):
    """(frames mapped [S,RH,RW], knots [G,K]) in fr's dtype"""
    x = knots(fr, rk, per_volume)
    return np.stack([apply_map(fr[s], x[0 if per_volume else s], y) for s in range(fr.shape[0])]), x


def crop_pad(fr, rows, cols, out_hw):
    """[S,OH,OW] of [S,RH,RW] by the per-axis index maps (lo, kept, before)"""
    ir, ic = R._index_map(rows[0], rows[1], rows[2], out_hw[0]), R._index_map(cols[0], cols[1], cols[2], out_hw[1])
    return fr[:, ir][:, :, ic]


def setting_parts(setting, modality, n_slice, S):
    """(ranks, targets, per_volume) of a normalised `intensity` setting other than minmax"""
    per_volume = setting.get('scope', 'volume') == 'volume'
    q = setting.get('percentiles', WINDOW_PERCENTILES if setting['mode'] == 'window' else LANDMARK_PERCENTILES)
    y = setting['standard'][modality] if setting['mode'] == 'landmarks' else (-1.0, 1.0)
    return ranks((S if per_volume else 1) * n_slice, q), y, per_volume


def preprocess(image, old_res, new_res, out_hw, setting, modality, dtype=np.float64):
    """image [S,H,W] -> [S,OH,OW,1]: the loader's image path under an `intensity` setting, crop / pad by the project's crop_same"""
    from multimodal_segmentation_amd.utils import data_utils
    RH, RW = R.out_extent(image.shape[1], old_res[0], new_res[0]), R.out_extent(image.shape[2], old_res[1], new_res[1])
    fr = frames(image, RH, RW, dtype)
    rk, y, per_volume = setting_parts(setting, modality, RH * RW, image.shape[0])
    mapped, _ = normalise(fr, rk, y, per_volume)
    [out], _ = data_utils.crop_same([mapped[..., None]], [mapped[..., None].copy()], tuple(out_hw))
    return out


def standard_scale(landmarks):
    """landmarks [V,K] fp64 of the training volumes -> the mean of their linear images with x_0 -> -1, x_{K-1} -> 1"""
    x = np.asarray(landmarks, np.float64)
    y = (-1.0 + 2.0 * (x - x[:, :1]) / (x[:, -1:] - x[:, :1])).mean(axis=0)
    y[0], y[-1] = -1.0, 1.0
    return y


# ---- CPU stand-ins of the entry points (argument lists of include/mmseg_hip.h without the stream) ----------------------------------------
CALLS = []          # one (S, K, per_volume) per selection: the tests count them


def standin_quantiles_workspace_bytes(S, K, per_volume):
    return 0 if S < 1 or not 2 <= K <= 16 else 4 * K


def standin_quantiles(img, rk, ws, x, S, H, W, RH, RW, K, per_volume):
    if not 2 <= K <= 16 or (S if per_volume else 1) * RH * RW >= 2 ** 31:
        return 1
    CALLS.append((S, K, int(per_volume)))
    fr = frames(img.numpy(), RH, RW, np.float32)
    x.copy_(torch.from_numpy(knots(fr, [int(r) for r in rk[:K]], bool(per_volume))))
    return 0


def standin_image_map(img, x, y, out, S, H, W, RH, RW, OH, OW, lo_r, kept_r, before_r, lo_c, kept_c, before_c, C, ch, K, per_volume):
    if not 2 <= K <= 16:
        return 1
    fr = frames(img.numpy(), RH, RW, np.float32)
    xs, ys = x.numpy(), y.numpy()
    mapped = np.stack([apply_map(fr[s], xs[0 if per_volume else s], ys) for s in range(S)])
    out[:, :, :, ch] = torch.from_numpy(crop_pad(mapped, (lo_r, kept_r, before_r), (lo_c, kept_c, before_c), (OH, OW)))
    return 0


STANDINS = {'mmseg_preprocess_quantiles_workspace_bytes': standin_quantiles_workspace_bytes,
            'mmseg_preprocess_quantiles': standin_quantiles, 'mmseg_preprocess_image_map': standin_image_map}
