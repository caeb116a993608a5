#!/usr/bin/env python
"""Score label volumes that were written earlier -- by `experiment.py --predict_folder` or by another program -- against a labelled
folder of volumes (loaders/volume_folder.py), without a model: Dice on the raw grid (results_native_<modality>.csv) and, for files
that carry `slice_spacing`, RAVD, ASSD and MSSD in mm (results_surface_<modality>.csv), through the code path of the predictor
(volume_predictor.score_folder, on the device).

PRED_FOLDER holds one `<file name of the input>.npz` with `label` [S_file,H,W] uint8 per scored file; files that are missing there, or
that carry no label in DATA_FOLDER, are left out.

`--predict_robust true` also writes HD (the `--predict_percentile` of the surface distances, default 95) and NSD (the share of them
within `--predict_tolerance` mm, default 1.0) into results_robust_<modality>.csv, for the files the surface file scores.

`--components largest` keeps each organ's largest 3-D connected component in every volume read from PRED_FOLDER before it is scored
(`--connectivity 6|26`): the scores that `--predict_components largest` would have given, for volumes written without it.
`--fill_holes 2d|3d` then fills the zeros that an organ encloses, slice by slice or in the volume, as `--predict_fill_holes` does;
with both options the filter runs first.
`--smooth open|close|smooth --smooth_radius MM` (`--smooth_extent 2d|3d`, default 2d) opens, closes or opens and then closes every
organ by a ball of that radius in mm before either, as `--predict_smooth` does.

    python tools/score_predictions.py PRED_FOLDER DATA_FOLDER [--out OUT] [--surface true|false] [--components largest]
                                      [--connectivity 6|26] [--fill_holes 2d|3d] [--smooth open|close|smooth] [--smooth_radius MM]
                                      [--smooth_extent 2d|3d] [--predict_robust true|false] [--predict_percentile Q]
                                      [--predict_tolerance MM]
"""
import argparse
import logging
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from multimodal_segmentation_amd.experiment import true_or_false
from multimodal_segmentation_amd.volume_predictor import score_folder


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('pred_folder')
    ap.add_argument('data_folder')
    ap.add_argument('--out', help='where to write the CSV files (default: PRED_FOLDER)')
    ap.add_argument('--surface', type=true_or_false, default=True, metavar='true|false', help='also the scores in mm')
    ap.add_argument('--components', choices=['largest'], help="filter the predicted volumes first: each organ's largest component")
    ap.add_argument('--connectivity', type=int, choices=[6, 26], default=6, help='neighbours of --components')
    ap.add_argument('--fill_holes', choices=['2d', '3d'], help='then fill the holes of every organ: slice by slice / in the volume')
    ap.add_argument('--smooth', choices=['open', 'close', 'smooth'],
                    help='before --components and --fill_holes: open / close / open and then close every organ by a ball')
    ap.add_argument('--smooth_radius', type=float, metavar='MM', help='radius of the ball of --smooth in mm, above 0; no default')
    ap.add_argument('--smooth_extent', choices=['2d', '3d'], default='2d', help='the ball lies in the slice / reaches across slices')
    ap.add_argument('--predict_robust', type=true_or_false, default=False, metavar='true|false', help='also HD and NSD')
    ap.add_argument('--predict_percentile', type=float, default=95.0, metavar='Q', help='percentile of --predict_robust, 0 to 100')
    ap.add_argument('--predict_tolerance', type=float, default=1.0, metavar='MM', help='tolerance of --predict_robust in mm, 0 or more')
    a = ap.parse_args(argv)
    if not 0.0 <= a.predict_percentile <= 100.0:
        ap.error('--predict_percentile must lie in [0, 100], got %r' % a.predict_percentile)
    if not 0.0 <= a.predict_tolerance < float('inf'):
        ap.error('--predict_tolerance must be a finite number of mm >= 0, got %r' % a.predict_tolerance)
    if a.smooth is not None and a.smooth_radius is None:
        ap.error('--smooth %s needs --smooth_radius MM: there is no default radius' % a.smooth)
    if a.smooth_radius is not None and not 0.0 < a.smooth_radius < float('inf'):
        ap.error('--smooth_radius must be a finite number of mm > 0, got %r' % a.smooth_radius)
    logging.basicConfig(level=logging.INFO, format='%(message)s')
    robust = (a.predict_percentile, a.predict_tolerance) if a.predict_robust else None
    tables = score_folder(a.pred_folder, a.data_folder, a.out, a.surface, a.components, a.connectivity, robust, a.fill_holes,
                          a.smooth, a.smooth_radius, a.smooth_extent)
    rows, surface_rows = tables[:2]
    for name in rows:
        print('%s: %d volumes scored, %d of them in mm' % (name, len(rows[name]), len(surface_rows[name])))
        if robust is not None:
            print('%s: %d volumes scored by HD(%g) and NSD(%g mm)' % ((name, len(tables[2][name])) + robust))


if __name__ == '__main__':
    main()
