"""Predicted label volumes for a folder of exported volumes, written in each volume's own geometry (build-defined: the reference
writes no segmentation; its `plot_images` PNG dumps are visualisation).

For every volume of the folder (loaders/volume_folder.py; labels are optional) and every modality m:
    images (device)  = loader.load_volume_for_prediction(volume)            resampled, rescaled, cropped / padded on the device
    prob   (device)  = model.predict_mask(m, mode, images)                   in batches of conf.batch_size slices
    label  (device)  = ops.restore_label(prob, label_values, geometry, order)   uint8 grey values on the raw H x W grid
and the selected slices are scattered back to their positions in a zero [S_file,H,W] array, so that the output lines up with the
input file.  The raw arrays cross the bus once each way: the image up, 1 byte per pixel down; no probability map reaches the host.

    <out>/<file name of the input>.npz     label [S_file,H,W] uint8 (0 and the grey values of `label_values`), resolution (copied)
    <out>/predictions.json                 settings only: source folder, mode, order, model folder, per file the selected slices
    <out>/results_native_<modality>.csv    where the input files carry a `label`: Dice on the raw grid, header and row format of
                                           model_tester.write_results, one row per labelled volume

Dice is costs.dice's formula applied to pixel counts (ops.label_overlap): per slice (2 I + 1e-12) / (P + T + 1e-12), the joint score
from the counts summed over the organs, then the mean over the selected slices."""
import json
import logging
import os

import numpy as np
import torch

from . import nn, ops
from .loaders.volume_folder import VolumeFolderLoader
from .model_tester import FUSION_MODES, write_results

log = logging.getLogger('volume_predictor')

SMOOTH = 1e-12          # costs.dice


def checkpoint_of(folder):
    """the checkpoint a run folder holds (models/dafnet.py, models/mmsdnet.py `load_models`), or None"""
    for path in (os.path.join(folder, 'models', 'D_Mask'), os.path.join(folder, 'supervised_trainer')):
        if os.path.exists(path):
            return path
    return None


def dice_from_counts(counts):
    """counts [S,K,3] = (|pred|, |truth|, |both|) per slice and organ -> (joint, [per organ]) as model_tester.volume_scores"""
    c = np.asarray(counts, np.float64)

    def score(x):          # x [S,3]
        return float(np.mean((2 * x[:, 2] + SMOOTH) / (x[:, 1] + x[:, 0] + SMOOTH)))
    return score(c.sum(axis=1)), [score(c[:, k]) for k in range(c.shape[1])]


class VolumePredictor(object):
    def __init__(self, model, conf):
        self.model, self.conf = model, conf

    def predict_volume(self, modality_index, mode, images):
        """predict_mask over the slices of one volume in batches of conf.batch_size: device tensors in, one device tensor out"""
        S = images[0].shape[0]
        step = max(1, int(self.conf.get('batch_size', S) or S))
        parts = [self.model.predict_mask(modality_index, mode, [x[i:i + step] for x in images]) for i in range(0, S, step)]
        parts = [p if isinstance(p, torch.Tensor) else nn.host_to_device(p, images[0].device) for p in parts]
        return parts[0] if len(parts) == 1 else torch.cat(parts, dim=0)

    def run(self, folder, out_folder, volumes=None, mode='simple', order=1):
        if mode not in FUSION_MODES:
            raise ValueError('Unknown mode: %r (expected one of %s)' % (mode, ', '.join(FUSION_MODES)))
        if order not in (0, 1):
            raise ValueError('order must be 0 (nearest) or 1 (bilinear), got %r' % (order,))
        loader = VolumeFolderLoader(folder)
        if len(loader.modalities) != len(self.model.modalities):
            raise ValueError('%s holds %d modalities, the model is built for %d'
                             % (folder, len(loader.modalities), len(self.model.modalities)))
        if tuple(loader.input_shape[:2]) != tuple(self.conf.input_shape[:2]) or loader.num_masks != self.conf.num_masks:
            raise ValueError('%s is prepared for input_shape %s and %d organs, the model is built for %s and %d'
                             % (folder, loader.input_shape[:2], loader.num_masks, tuple(self.conf.input_shape[:2]),
                                self.conf.num_masks))
        volumes = list(loader.manifest['volumes']) if volumes is None else [str(v) for v in volumes]
        for v in volumes:
            if v not in loader.manifest['volumes']:
                raise ValueError('%s describes no volume %r' % (folder, v))
        os.makedirs(out_folder, exist_ok=True)
        device = nn.default_device()
        values = nn.host_to_device(np.asarray(loader.label_values), device, np.int32)
        rows = [[] for _ in loader.modalities]
        files = {}
        for v in volumes:
            images, geometry = loader.load_volume_for_prediction(v)
            for m, geo in enumerate(geometry):
                prob = self.predict_volume(m, mode, images)
                pred = ops.restore_label(prob, values, geo['raw_shape'][1:], geo['resampled'], geo['rows'], geo['cols'], order)
                if geo['label'] is not None:
                    counts = ops.label_overlap(pred, nn.host_to_device(geo['label'], device, np.uint8), values)
                    joint, per_organ = dice_from_counts(nn.to_numpy(counts))
                    rows[m].append((v, joint, per_organ))
                    log.info('volume %s, %s: Dice on the raw grid %.3f' % (v, loader.modalities[m], joint))
                label = np.zeros(geo['raw_shape'], np.uint8)
                label[geo['slices']] = pred.cpu().numpy()
                np.savez_compressed(os.path.join(out_folder, geo['file']), label=label, resolution=geo['resolution'])
                files[geo['file']] = dict(volume=v, modality=loader.modalities[m], slices=geo['slices'])
        for m, name in enumerate(loader.modalities):
            if rows[m]:
                write_results(os.path.join(out_folder, 'results_native_%s.csv' % name), rows[m], loader.num_masks)
        with open(os.path.join(out_folder, 'predictions.json'), 'w') as f:
            json.dump(dict(source_folder=folder, mode=mode, order=order, model_folder=self.conf.get('folder'),
                           label_values=loader.label_values, files=files), f, indent=1)
        return {name: rows[m] for m, name in enumerate(loader.modalities)}
