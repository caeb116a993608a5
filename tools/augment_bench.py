#!/usr/bin/env python
"""Isolated timings of the batch-assembly augmentation kernels (csrc/augment.hip) at the training geometry: mmseg_affine_gather
(rotation only) beside mmseg_augment_gather (every ImageDataGenerator key, without and with the channel shift), B slices of
H x H x C gathered from a resident set of N.  Algorithmic bytes = B*H*H*C*4 read + the same written (+ the same again read and
written by the channel-shift pass); HBM-bound.  Run it under `rocprofv3 --kernel-trace --stats -- python tools/augment_bench.py`
for the per-kernel table.

    python tools/augment_bench.py [B=8] [H=256]
"""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from multimodal_segmentation_amd import ops
from multimodal_segmentation_amd.utils import augment


def bench(fn, reps=50):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(reps):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / reps * 1e3      # us


def main():
    B = int(sys.argv[1]) if len(sys.argv) > 1 else 8
    H = int(sys.argv[2]) if len(sys.argv) > 2 else 256
    n = 32
    params = dict(rotation_range=20., width_shift_range=0.1, height_shift_range=0.1, shear_range=10., zoom_range=0.1,
                  channel_shift_range=0.2, fill_mode='reflect', horizontal_flip=True, vertical_flip=True)
    for C in (1, 4):
        data = torch.randn(n, H, H, C, device='cuda')
        stream = augment.KerasTransformStream(n, B, 5, params, H, H, C)
        rows, mats, _, _, shifts = stream.next()
        rows_d = torch.as_tensor(rows.astype(np.int32)).cuda()
        mat64 = torch.as_tensor(mats).cuda()
        mat32 = mat64.float()
        shift_d = torch.as_tensor(shifts.astype(np.float32)).cuda()
        nbytes = B * H * H * C * 4 * 2
        t_rot = bench(lambda: ops.affine_gather(data, rows_d, mat32, 1))
        t_aug = bench(lambda: ops.augment_gather(data, rows_d, mat64, None, 1, 'reflect', 0.))
        t_shift = bench(lambda: ops.augment_gather(data, rows_d, mat64, shift_d, 1, 'reflect', 0.))
        print(json.dumps(dict(B=B, H=H, C=C, algorithmic_MB=nbytes / 1e6, affine_gather_us=round(t_rot, 2),
                              augment_gather_us=round(t_aug, 2), augment_gather_shift_us=round(t_shift, 2),
                              augment_gather_GBs=round(nbytes / t_aug / 1e3, 1),
                              augment_gather_shift_GBs=round(2 * nbytes / t_shift / 1e3, 1))))


if __name__ == '__main__':
    main()
