#!/usr/bin/env python
"""Time of the hole filling of one predicted label volume: ops.fill_label_holes on the device (csrc/postprocess.hip) in both modes,
beside ops.keep_largest_components and ops.surface_metrics on the same volume (the steps before and after it in volume_predictor.py)
and beside the scipy restatement (tests/volume_holes_ref.py) on the host it runs on.

Workload: the volumes of tools/volume_components_bench.py, four organs: 36 x 320 x 320 (a CHAOS MR volume) and, where the device's
memory allows, 100 x 512 x 512 (a CT volume).  The prediction is the arg-max over smooth random fields with `--salt` of its voxels
replaced by a random organ's grey value and `--pepper` of them by 0 (pin-holes inside the organs).
  device   event time of ops.fill_label_holes ('2d' and '3d'), ops.keep_largest_components (connectivity 6) and ops.surface_metrics
           (the filled prediction against the truth), each after `--warmup` calls, median of `--repeats`
  host     the restatement (ndimage.binary_fill_holes per organ, on the volume or slice by slice), timed once; its volume and stats
           must equal the device's or the tool fails
Prints one JSON line and writes the write-up to `--out`.

    python tools/volume_holes_bench.py [--repeats 20] [--warmup 3] [--salt 0.002] [--pepper 0.002] [--out profiles/volume_holes_bench.md]
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from multimodal_segmentation_amd import nn, ops
from tests import helpers as Hh
from tests import volume_holes_ref as F

VALUES = [63, 126, 189, 252]
SHAPES = (((36, 320, 320), (7.7, 1.6, 1.6)), ((100, 512, 512), (3.0, 0.8, 0.8)))
BYTES_PER_VOXEL = 60          # of ops.surface_metrics, the largest workspace of the three (two fp64 maps, ten surface volumes)


def make_pair(rng, shape, salt, pepper):
    """(pred, truth) uint8: fields of 12 distinct slices, cycled along the volume; salt and pepper noise on the prediction"""
    S, H, W = shape
    f = np.concatenate([Hh.smooth_field(rng, 12, H, W, sigma=H / 16.0) for _ in range(5)], axis=-1).astype(np.float32)
    g = np.concatenate([Hh.smooth_field(rng, 12, H, W, sigma=H / 16.0) for _ in range(5)], axis=-1).astype(np.float32)
    grey = np.asarray([0] + VALUES, np.uint8)
    which = np.arange(S) % 12
    pred, truth = grey[np.argmax(f + 0.35 * g, axis=-1)][which], grey[np.argmax(f, axis=-1)][which]
    noisy = rng.rand(*shape) < salt
    pred[noisy] = np.asarray(VALUES, np.uint8)[rng.randint(0, len(VALUES), size=int(noisy.sum()))]
    pred[rng.rand(*shape) < pepper] = 0
    return pred, truth


def time_calls(fn, warmup, repeats):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(repeats):
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        fn()
        stop.record()
        stop.synchronize()
        times.append(start.elapsed_time(stop) * 1e-3)
    return float(np.median(times)), float(np.min(times)), float(np.max(times))


def measure(a, shape, spacing):
    pred, truth = make_pair(np.random.RandomState(11), shape, a.salt, a.pepper)
    dev = [nn.host_to_device(x, 'cuda:0', np.uint8) for x in (pred, truth)]
    values = nn.host_to_device(np.asarray(VALUES), 'cuda:0', np.int32)
    out = {}
    for mode in F.MODES:
        filled, stats = ops.fill_label_holes(dev[0], values, mode)
        t0 = time.perf_counter()
        want, want_stats = F.fill_holes(pred, VALUES, mode)
        t_host = time.perf_counter() - t0
        if not np.array_equal(filled.cpu().numpy(), want) or not np.array_equal(stats.cpu().numpy(), want_stats):
            raise SystemExit('device and host disagree in mode %s on %s' % (mode, shape))
        t = time_calls(lambda: ops.fill_label_holes(dev[0], values, mode), a.warmup, a.repeats)
        out[mode] = dict(fill_s=t[0], fill_min_max_s=t[1:], host_s=t_host, stats=want_stats.tolist())
    t_keep = time_calls(lambda: ops.keep_largest_components(dev[0], values, 6), a.warmup, a.repeats)
    filled, _ = ops.fill_label_holes(dev[0], values, '3d')
    t_metrics = time_calls(lambda: ops.surface_metrics(filled, dev[1], values, spacing), a.warmup, a.repeats)
    return dict(shape=shape, voxels=int(pred.size), salt=a.salt, pepper=a.pepper, by_mode=out, keep_largest_s=t_keep[0],
                keep_largest_min_max_s=t_keep[1:], surface_metrics_s=t_metrics[0], surface_metrics_min_max_s=t_metrics[1:])


def write_up(path, a, results, skipped, device):
    lines = ['# Hole filling of one predicted label volume: ops.fill_label_holes', '',
             'Four organs, smooth-field labels with %.2g of the voxels replaced by a random organ (salt) and %.2g by 0 (pepper).'
             % (a.salt, a.pepper),
             'Device: event time, %d warm-up calls, median of %d calls (min .. max in brackets).  Host: the scipy restatement'
             % (a.warmup, a.repeats),
             '(tests/volume_holes_ref.py), timed once on the same machine; its volume and stats equal the device\'s.  %s.' % device,
             'Command: `python tools/volume_holes_bench.py`', '']
    for r in results:
        lines += ['## %s (%d voxels)' % (' x '.join(str(v) for v in r['shape']), r['voxels']), '',
                  '| step | device | host (scipy) |', '|---|---|---|']
        for mode in F.MODES:
            m = r['by_mode'][mode]
            lines.append('| fill_label_holes %s | %.3f ms (%.3f .. %.3f) | %.1f ms |'
                         % (mode, 1e3 * m['fill_s'], 1e3 * m['fill_min_max_s'][0], 1e3 * m['fill_min_max_s'][1], 1e3 * m['host_s']))
        lines.append('| keep_largest_components, connectivity 6 | %.3f ms (%.3f .. %.3f) | |'
                     % (1e3 * r['keep_largest_s'], 1e3 * r['keep_largest_min_max_s'][0], 1e3 * r['keep_largest_min_max_s'][1]))
        lines.append('| surface_metrics (filled prediction against the truth) | %.3f ms (%.3f .. %.3f) | |'
                     % (1e3 * r['surface_metrics_s'], 1e3 * r['surface_metrics_min_max_s'][0], 1e3 * r['surface_metrics_min_max_s'][1]))
        lines.append('')
        for mode in F.MODES:
            m = r['by_mode'][mode]
            ratio = m['fill_s'] / r['surface_metrics_s']
            lines.append('Mode %s: per organ (holes, voxels before, voxels added) %s; %.2f times the time of surface_metrics: it costs %s '
                         'than the scores in mm.' % (mode, m['stats'], ratio, 'MORE' if ratio > 1 else 'less'))
        lines.append('')
    for shape, why in skipped:
        lines += ['## %s' % ' x '.join(str(v) for v in shape), '', 'NOT MEASURED: %s' % why, '']
    with open(path, 'w') as f:
        f.write('\n'.join(lines))


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('--repeats', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--salt', type=float, default=0.002)
    ap.add_argument('--pepper', type=float, default=0.002)
    ap.add_argument('--out', default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'profiles',
                                                  'volume_holes_bench.md'))
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit('volume_holes_bench needs a GPU: a time measured without one says nothing')
    if a.repeats < 10:
        raise SystemExit('at least 10 repeats')
    nn.set_default_device('cuda:0')
    results, skipped = [], []
    for shape, spacing in SHAPES:
        need = BYTES_PER_VOXEL * int(np.prod(shape))
        free = torch.cuda.mem_get_info(0)[0]
        if need > free // 2:
            skipped.append((shape, 'needs about %d MB, %d MB are free' % (need >> 20, free >> 20)))
            continue
        results.append(measure(a, shape, spacing))
    device = torch.cuda.get_device_name(0)
    print(json.dumps(dict(device=device, results=results, skipped=skipped)))
    write_up(a.out, a, results, skipped, device)


if __name__ == '__main__':
    main()
