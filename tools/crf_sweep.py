#!/usr/bin/env python
"""Score a grid of CRF settings (`--predict_crf`, ops.crf_refine) on a labelled folder of volumes: how a user replaces the defaults,
which are starting values that nobody has tuned.

The folder is predicted ONCE with the checkpoint of the run folder and the probability maps stay on the device; every setting of the
grid then goes through crf, restore_label and the scorers of volume_predictor.py (score_volume): Dice on the raw grid and, where the
files hold `slice_spacing`, RAVD (%), ASSD, MSSD and HD95 (mm) and NSD of the union of the organs.  One table row per setting, the
first one without the refinement; every figure is the mean over the labelled volumes and modalities.

    python tools/crf_sweep.py FOLDER --run RUN [--grid radius=3,5 w_a=2,4,8 theta_beta=0.05,0.1] [--mode simple] [--order 1]
                              [--percentile 95] [--tolerance 1.0]

RUN is a run folder of experiment.py (experiment_configuration.json and the checkpoint).  Every --grid item is key=v1,v2,... over
the keys of --predict_crf; the settings are the product of the items over the defaults.
"""
import argparse
import itertools
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

from multimodal_segmentation_amd import nn, ops
from multimodal_segmentation_amd.loaders.volume_folder import VolumeFolderLoader
from multimodal_segmentation_amd.volume_predictor import CRF_DEFAULTS, VolumePredictor, check_crf, checkpoint_of, score_volume

DEFAULT_GRID = ('radius=3,5', 'w_a=2,4,8', 'theta_beta=0.05,0.1,0.2')
COLUMNS = (('dice', 'Dice', '%.4f'), ('ravd', 'RAVD %', '%.2f'), ('assd', 'ASSD mm', '%.3f'), ('mssd', 'MSSD mm', '%.2f'),
           ('hd', 'HD mm', '%.2f'), ('nsd', 'NSD', '%.4f'))


def parse_grid(items):
    """['radius=3,5', 'w_a=2'] -> the settings, each a tuple of (key, value) pairs in the order given: the product of the items"""
    axes = []
    for item in items:
        key, eq, values = item.partition('=')
        key = key.strip().lower()
        if not eq or key not in CRF_DEFAULTS._fields or key in [k for k, _ in axes]:
            raise ValueError('--grid: expected key=v1,v2,... with a key of %s, each once, got %r' % (', '.join(CRF_DEFAULTS._fields), item))
        axes.append((key, [check_crf('%s=%s' % (key, v.strip()))._asdict()[key] for v in values.split(',')]))
    return [tuple(zip([k for k, _ in axes], combo)) for combo in itertools.product(*[v for _, v in axes])]


def name_of(setting):
    return ','.join('%s=%g' % kv for kv in setting) if setting else 'none'


def sweep(model, conf, folder, grid, mode='simple', order=1, robust=(95.0, 1.0)):
    """-> one dictionary per setting (None first, then those of `grid`): setting, volumes, dice and, where the files allow, the scores in mm"""
    loader = VolumeFolderLoader(folder)
    predictor = VolumePredictor(model, conf)
    device = nn.default_device()
    values = nn.host_to_device(np.asarray(loader.label_values), device, np.int32)
    kept = []
    for v in loader.manifest['volumes']:
        images, geometry = loader.load_volume_for_prediction(v)
        for m, geo in enumerate(geometry):
            if geo['label'] is not None:
                kept.append((predictor.predict_volume(m, mode, images), images[m], geo, nn.host_to_device(geo['label'], device, np.uint8)))
    if not kept:
        raise ValueError('%s holds no labelled volume to score against' % folder)
    rows = []
    for setting in [None] + list(grid):
        params = None if setting is None else check_crf(CRF_DEFAULTS._replace(**dict(setting)))
        scores = []
        for prob, image, geo, label in kept:
            refined = prob if params is None else ops.crf_refine(prob, image, loader.num_masks, params)
            pred = ops.restore_label(refined, values, geo['raw_shape'][1:], geo['resampled'], geo['rows'], geo['cols'], order)
            scores.append(score_volume(pred, label, values, geo, True, robust))
        row = dict(setting=name_of(setting), volumes=len(scores), dice=float(np.mean([s[0] for s in scores])))
        in_mm = [s[2][-1] for s in scores if s[2] is not None]          # the union of the organs
        if in_mm:
            row.update(zip(('ravd', 'assd', 'mssd'), (float(x) for x in np.nanmean(np.asarray(in_mm), axis=0))))
            row.update(zip(('hd', 'nsd'), (float(x) for x in np.nanmean(np.asarray([s[3][-1] for s in scores if s[3] is not None]), axis=0))))
        rows.append(row)
    return rows


def print_table(rows):
    shown = [c for c in COLUMNS if c[0] in rows[0]]
    width = max(len(r['setting']) for r in rows)
    print('%-*s  %s' % (width, 'setting', '  '.join('%9s' % title for _, title, _ in shown)))
    print('-' * (width + 11 * len(shown)))
    for r in rows:
        print('%-*s  %s' % (width, r['setting'], '  '.join('%9s' % (fmt % r[key]) for key, _, fmt in shown)))


def load_model(run):
    """(model, conf) of a run folder: the configuration it recorded, the model built from it, the checkpoint loaded as --test does"""
    from multimodal_segmentation_amd.experiment import resolve
    from multimodal_segmentation_amd.utils.config import EasyDict
    path = os.path.join(run, 'experiment_configuration.json')
    if not os.path.isfile(path) or checkpoint_of(run) is None:
        raise SystemExit('%s is no run folder with a checkpoint (experiment_configuration.json and the models)' % run)
    with open(path) as f:
        conf = EasyDict(json.load(f))
    conf.folder = run
    model = resolve('models', conf.model)(conf)
    model.build()
    return model, conf


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('folder', help='a labelled folder of exported volumes')
    ap.add_argument('--run', required=True, help='run folder of experiment.py with a checkpoint')
    ap.add_argument('--grid', nargs='+', default=list(DEFAULT_GRID), metavar='KEY=V1,V2', help='default: %s' % ' '.join(DEFAULT_GRID))
    ap.add_argument('--mode', default='simple')
    ap.add_argument('--order', type=int, choices=[0, 1], default=1)
    ap.add_argument('--percentile', type=float, default=95.0)
    ap.add_argument('--tolerance', type=float, default=1.0)
    a = ap.parse_args(argv)
    grid = parse_grid(a.grid)
    model, conf = load_model(a.run)
    print_table(sweep(model, conf, a.folder, grid, a.mode, a.order, (a.percentile, a.tolerance)))


if __name__ == '__main__':
    main()
