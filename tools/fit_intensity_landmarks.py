#!/usr/bin/env python
"""Learn the standard intensity scale of a volume folder (Nyul and Udupa's landmark standardisation) and write it into the folder's
dataset.json as its `intensity` block (multimodal_segmentation_amd/loaders/volume_folder.py; INTEGRATION.md, "Volume folders").

For every training volume of the split and every modality the landmarks -- the order statistics of the configured percentiles among
the resampled values of the whole volume -- are selected on the device (ops.preprocess_quantiles), mapped linearly so that the lowest
lands on -1 and the highest on 1 (fp64, on the host) and averaged over the volumes.  The loader then maps every volume's own landmarks
onto that scale, piecewise linearly.  The block is also written to the folders named with --copy-to, so that test and predict folders
share the scale.

    python tools/fit_intensity_landmarks.py FOLDER [--split 0] [--percentiles 1,10,20,30,40,50,60,70,80,90,99] [--copy-to OTHER ...]
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

from multimodal_segmentation_amd import nn
from multimodal_segmentation_amd.loaders import volume_folder as vf


def volume_landmarks(loader, volume, modality, percentiles):
    """fp64 [K]: the landmarks of one (volume, modality), selected on the device over its whole resampled frame"""
    from multimodal_segmentation_amd import ops
    image, _, res = loader.read_volume(volume, modality, require_label=False)
    resampled, _, _ = loader.geometry(image.shape[1], image.shape[2], res)
    x = nn.host_to_device(image, nn.default_device(), np.float32)
    ranks = vf.quantile_ranks(x.shape[0] * resampled[0] * resampled[1], percentiles)
    return nn.to_numpy(ops.preprocess_quantiles(x, resampled, ranks, True))[0].astype(np.float64)


def fit(folder, split=0, percentiles=vf.LANDMARK_PERCENTILES):
    """the `intensity` block of `folder`: mode landmarks, the percentiles and per modality the mean over the split's training volumes
    of their landmarks brought to [-1, 1]"""
    manifest = vf.read_manifest(folder)
    probe = dict(mode='landmarks', percentiles=list(percentiles),
                 standard={m: [-1.0] + [0.0] * (len(percentiles) - 2) + [1.0] for m in manifest['modalities']})
    percentiles = vf.check_intensity(probe, manifest['modalities'], '--percentiles')['percentiles']
    loader = vf.VolumeFolderLoader(folder)
    volumes = loader.get_volumes_for_split(split, 'training')
    if not volumes:
        raise ValueError('%s: split %s has no training volumes' % (folder, split))
    standard = {}
    for mod in loader.modalities:
        scales = []
        for v in volumes:
            x = volume_landmarks(loader, v, mod, percentiles)
            if x[0] == x[-1]:
                raise ValueError('volume %s, modality %s: its lowest and highest landmarks are equal (%r): a constant volume has no '
                                 'scale' % (v, mod, float(x[0])))
            scales.append(-1.0 + 2.0 * (x - x[0]) / (x[-1] - x[0]))
        y = np.mean(np.stack(scales), axis=0)
        y[0], y[-1] = -1.0, 1.0
        standard[mod] = [float(t) for t in y]
    return dict(mode='landmarks', percentiles=[float(q) for q in percentiles], standard=standard)


def write_block(folder, block):
    """set the `intensity` key of the folder's dataset.json (validated against that folder's modalities first)"""
    path = os.path.join(folder, vf.MANIFEST)
    manifest = vf.read_manifest(folder)
    vf.check_intensity(block, manifest['modalities'], path)
    manifest['intensity'] = block
    with open(path, 'w') as f:
        json.dump(manifest, f, indent=1)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('folder')
    ap.add_argument('--split', type=int, default=0)
    ap.add_argument('--percentiles', default=','.join(str(q) for q in vf.LANDMARK_PERCENTILES), metavar='LIST',
                    help='2 to 16 increasing percentiles, comma separated')
    ap.add_argument('--copy-to', nargs='*', default=[], metavar='OTHER_FOLDER', help='folders that get the same block (test, predict)')
    a = ap.parse_args(argv)
    try:
        percentiles = [float(q) for q in a.percentiles.split(',')]
    except ValueError:
        ap.error('--percentiles must be a comma separated list of numbers, got %r' % a.percentiles)
    block = fit(a.folder, a.split, percentiles)
    for folder in [a.folder] + list(a.copy_to):
        write_block(folder, block)
    print('wrote the standard scale of %s (split %d, %d landmarks) to %s'
          % (', '.join(sorted(block['standard'])), a.split, len(percentiles), ', '.join([a.folder] + list(a.copy_to))))
    return block


if __name__ == '__main__':
    main()
