#!/usr/bin/env python
"""Load time of a CHAOS-sized volume folder: loaders/volume_folder.py on the device (csrc/preprocess.hip) beside the fp64 scipy
restatement of the same preprocessing (tests/volume_loader_ref.py) on the host it runs on.

Writes the folder with tools/make_volume_folder.py (20 volumes x 2 modalities x about 30 slices of 256..320 pixels a side,
input_shape 192 x 192), then loads all of it (`load_all_modalities_concatenated(0, 'all', 1)`):
  device   wall time of the whole call (read + decompress the .npz files, pinned upload, kernels, download), the first call and
           the median of the next `--repeats`; and the share spent reading the files
  host     the restatement over the same raw arrays, files already read
The images must agree within 2e-4 or the tool fails; the number of differing mask pixels is reported.  Prints one JSON line.

    python tools/volume_loader_bench.py [--volumes 20] [--slices 30] [--repeats 3] [--keep DIR]
"""
import argparse
import json
import os
import shutil
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from multimodal_segmentation_amd import nn
from multimodal_segmentation_amd.loaders.volume_folder import VolumeFolderLoader
from tests import volume_loader_ref as R


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('--volumes', type=int, default=20)
    ap.add_argument('--slices', type=int, default=30)
    ap.add_argument('--repeats', type=int, default=3)
    ap.add_argument('--keep', help='write the folder here and keep it')
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit('volume_loader_bench needs a GPU: a load time measured without one says nothing')
    nn.set_default_device('cuda:0')
    root = a.keep or tempfile.mkdtemp(prefix='volume_folder_')
    try:
        R.tool().write_folder(root, volumes=a.volumes, size=192, slices=a.slices, raw_size=(256, 320), seed=1)
        loader = VolumeFolderLoader(root)

        def load():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            d = loader.load_all_modalities_concatenated(0, 'all', 1)        # ends in a device -> host copy, i.e. synchronised
            return time.perf_counter() - t0, d
        first, data = load()
        times = [load()[0] for _ in range(a.repeats)]
        t0 = time.perf_counter()
        raw = [[loader.read_volume(v, m) for m in loader.modalities] for v in loader.get_volumes_for_split(0, 'all')]
        t_read = time.perf_counter() - t0
        t0 = time.perf_counter()
        err, differing, n = 0.0, 0, 0
        for per_mod in raw:
            S = per_mod[0][0].shape[0]
            for m, (image, label, res) in enumerate(per_mod):
                want_i, want_m = R.preprocess(image, label, res, loader.target_resolution, loader.label_values, loader.input_shape[:2])
                err = max(err, float(np.abs(data.get_images_modi(m)[n:n + S] - want_i).max()))
                differing += int(np.count_nonzero(data.get_masks_modi(m)[n:n + S] != want_m))
            n += S
        t_host = time.perf_counter() - t0
        out = dict(volumes=a.volumes, modalities=len(loader.modalities), slices=int(n), raw_pixels=[256, 320], input_shape=[192, 192],
                   device_first_s=round(first, 3), device_s=[round(t, 3) for t in times], device_median_s=round(float(np.median(times)), 3),
                   read_files_s=round(t_read, 3), host_restatement_s=round(t_host, 3), image_max_abs_error=err,
                   mask_pixels_differing=differing, device=torch.cuda.get_device_name(0))
        print(json.dumps(out))
        if err > 2e-4:
            raise SystemExit('device and host preprocessing disagree')
    finally:
        if not a.keep:
            shutil.rmtree(root, ignore_errors=True)


if __name__ == '__main__':
    main()
