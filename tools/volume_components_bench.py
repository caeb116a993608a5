#!/usr/bin/env python
"""Time of the component filter of one predicted label volume: ops.keep_largest_components on the device (csrc/postprocess.hip) beside
the scipy restatement (tests/volume_components_ref.py) on the host it runs on, and beside ops.surface_metrics on the same volume, the
step that follows the filter in volume_predictor.py.

Workload: a 36 x 320 x 320 volume (a CHAOS MR volume), four organs.  The truth is the arg-max over five smooth random fields, the
prediction the arg-max of the same fields plus 0.35 times a second set, with `--salt` of its voxels replaced by a random organ's grey
value (stray islands of one voxel).
  device   event time of ops.keep_largest_components, ops.label_components and ops.surface_metrics (prediction after the filter
           against the truth), each after `--warmup` calls, median of `--repeats`
  host     the restatement of the filter (ndimage.label per organ, bincount, the winner), timed once; its volume and stats must equal
           the device's or the tool fails
Prints one JSON line and writes the write-up to `--out`.

    python tools/volume_components_bench.py [--repeats 20] [--warmup 3] [--salt 0.002] [--out profiles/components_bench.txt]
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
from tests import volume_components_ref as C

VALUES = [63, 126, 189, 252]
SHAPE, SPACING = (36, 320, 320), (7.7, 1.6, 1.6)


def make_pair(rng, shape, salt):
    """(pred, truth) uint8: fields of 12 distinct slices, cycled along the volume; salt noise on the prediction"""
    S, H, W = shape
    f = np.concatenate([Hh.smooth_field(rng, 12, H, W, sigma=H / 16.0) for _ in range(5)], axis=-1).astype(np.float32)
    g = np.concatenate([Hh.smooth_field(rng, 12, H, W, sigma=H / 16.0) for _ in range(5)], axis=-1).astype(np.float32)
    grey = np.asarray([0] + VALUES, np.uint8)
    which = np.arange(S) % 12
    pred, truth = grey[np.argmax(f + 0.35 * g, axis=-1)][which], grey[np.argmax(f, axis=-1)][which]
    noisy = rng.rand(*shape) < salt
    pred[noisy] = np.asarray(VALUES, np.uint8)[rng.randint(0, len(VALUES), size=int(noisy.sum()))]
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


def measure(a):
    pred, truth = make_pair(np.random.RandomState(11), SHAPE, a.salt)
    dev = [nn.host_to_device(x, 'cuda:0', np.uint8) for x in (pred, truth)]
    values = nn.host_to_device(np.asarray(VALUES), 'cuda:0', np.int32)
    out = {}
    for connectivity in (6, 26):
        kept, stats = ops.keep_largest_components(dev[0], values, connectivity)
        t0 = time.perf_counter()
        want, want_stats = C.keep_largest(pred, VALUES, connectivity)
        t_host = time.perf_counter() - t0
        if not np.array_equal(kept.cpu().numpy(), want) or not np.array_equal(stats.cpu().numpy(), want_stats):
            raise SystemExit('device and host disagree at connectivity %d' % connectivity)
        t_keep = time_calls(lambda: ops.keep_largest_components(dev[0], values, connectivity), a.warmup, a.repeats)
        t_label = time_calls(lambda: ops.label_components(dev[0], values, connectivity), a.warmup, a.repeats)
        out[connectivity] = dict(keep_largest_s=t_keep[0], keep_largest_min_max_s=t_keep[1:], label_components_s=t_label[0],
                                 host_s=t_host, stats=want_stats.tolist())
    kept, _ = ops.keep_largest_components(dev[0], values, 6)
    t_metrics = time_calls(lambda: ops.surface_metrics(kept, dev[1], values, SPACING), a.warmup, a.repeats)
    return dict(shape=SHAPE, voxels=int(pred.size), salt=a.salt, by_connectivity=out, surface_metrics_s=t_metrics[0],
                surface_metrics_min_max_s=t_metrics[1:])


def write_up(path, a, r, device):
    lines = ['Component filter of one predicted label volume: ops.keep_largest_components', '',
             'Workload: %s voxels, four organs, smooth-field labels with %.2g of the voxels replaced by a random organ (salt).'
             % (' x '.join(str(v) for v in r['shape']), r['salt']),
             'Device: event time, %d warm-up calls, median of %d calls (min .. max in brackets).  Host: the scipy restatement'
             % (a.warmup, a.repeats),
             '(tests/volume_components_ref.py), timed once on the same machine; its volume and stats equal the device\'s.  %s.' % device,
             'Command: python tools/volume_components_bench.py', '']
    for connectivity in (6, 26):
        c = r['by_connectivity'][connectivity]
        lines += ['connectivity %d' % connectivity,
                  '  keep_largest_components (device)   %.3f ms (%.3f .. %.3f)'
                  % (1e3 * c['keep_largest_s'], 1e3 * c['keep_largest_min_max_s'][0], 1e3 * c['keep_largest_min_max_s'][1]),
                  '  label_components alone (device)    %.3f ms' % (1e3 * c['label_components_s']),
                  '  scipy restatement (host)           %.1f ms' % (1e3 * c['host_s']),
                  '  per organ (components, voxels before, voxels kept): %s' % c['stats'], '']
    ratio = r['by_connectivity'][6]['keep_largest_s'] / r['surface_metrics_s']
    lines += ['surface_metrics on the same volume (device, the filtered prediction against the truth)   %.3f ms (%.3f .. %.3f)'
              % (1e3 * r['surface_metrics_s'], 1e3 * r['surface_metrics_min_max_s'][0], 1e3 * r['surface_metrics_min_max_s'][1]),
              'The filter at connectivity 6 takes %.3f times the time of surface_metrics: it costs %s than the scores in mm.'
              % (ratio, 'MORE' if ratio > 1 else 'less'), '']
    with open(path, 'w') as f:
        f.write('\n'.join(lines))


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('--repeats', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--salt', type=float, default=0.002)
    ap.add_argument('--out', default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'profiles',
                                                  'components_bench.txt'))
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit('volume_components_bench needs a GPU: a time measured without one says nothing')
    if a.repeats < 10:
        raise SystemExit('at least 10 repeats')
    nn.set_default_device('cuda:0')
    result = measure(a)
    device = torch.cuda.get_device_name(0)
    print(json.dumps(dict(device=device, result=result)))
    write_up(a.out, a, result, device)


if __name__ == '__main__':
    main()
