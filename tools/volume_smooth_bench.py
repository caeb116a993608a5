#!/usr/bin/env python
"""Time of the opening, closing and smoothing of one predicted label volume by a ball in mm: ops.smooth_label on the device
(csrc/postprocess.hip), the three ops at several radii and both extents, beside ops.keep_largest_components, ops.fill_label_holes and
ops.surface_metrics on the same volume (the steps after it in volume_predictor.py) and beside the scipy restatement
(tests/volume_smooth_ref.py) on the host it runs on.

Workload: the volumes of tools/volume_holes_bench.py, four organs: 36 x 320 x 320 (a CHAOS MR volume) and, where the device's memory
allows, 100 x 512 x 512 (a CT volume).  The prediction is the arg-max over smooth random fields with `--salt` of its voxels replaced by
a random organ's grey value and `--pepper` of them by 0.
  device   event time of ops.smooth_label per op, radius and extent, and of the three other steps, each after `--warmup` calls, median
           of `--repeats`
  host     the restatement (ndimage.binary_erosion / binary_dilation per organ with the exact ball), timed once per configuration on
           the first volume and once in all on the others; its volume and stats must equal the device's or the tool fails
  traffic  the bytes that a configuration has to move per voxel if every kernel reads and writes each of its volumes once (the rows of
           the ball that a voxel visits come from the caches), and the share of the HBM peak that this model reaches in the measured
           time: per organ and erosion or dilation 2 bytes for the map of runs along x (none when the ball is one voxel wide there) and
           3 or 4 for the pass over the rows of the ball
Prints one JSON line and writes the write-up to `--out`.

    python tools/volume_smooth_bench.py [--repeats 20] [--warmup 3] [--salt 0.002] [--pepper 0.002] [--out profiles/volume_smooth_bench.md]
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
from tests import volume_smooth_ref as F
from tools.volume_holes_bench import BYTES_PER_VOXEL, SHAPES, VALUES, make_pair, time_calls

RADII = (2.5, 4.5)           # mm: 1 and 2 voxels in the plane of the MR volume, 3 and 5 in that of the CT volume (and 1 slice at 4.5 mm)
HBM_PEAK = 8.0e12            # bytes per second, MI355X


def model_bytes(op, reach, K):
    """bytes per voxel by the model of the module docstring; reach = (rz, ry, rx)"""
    run = 2 if reach[2] > 0 else 0
    half = (run + 3) + (run + 4)          # erosion or dilation into the mask, then the pass that writes the volume
    return K * half * (2 if op == 'smooth' else 1)


def measure(a, shape, spacing, check_all):
    pred, truth = make_pair(np.random.RandomState(11), shape, a.salt, a.pepper)
    dev = [nn.host_to_device(x, 'cuda:0', np.uint8) for x in (pred, truth)]
    values = nn.host_to_device(np.asarray(VALUES), 'cuda:0', np.int32)
    rows, checked = [], 0
    for r in RADII:
        for extent in F.EXTENTS:
            if F.margin(spacing, r, extent) <= 1e-9:
                raise SystemExit('radius %r at spacing %r: an offset lies on the rim of the ball' % (r, spacing))
            reach = F.reach(spacing, r, extent)
            for op in F.OPS:
                t_host = None
                if check_all or (checked == 0 and op == 'smooth'):
                    out, stats = ops.smooth_label(dev[0], values, spacing, r, op, extent)
                    t0 = time.perf_counter()
                    want, want_stats = F.smooth_label(pred, VALUES, spacing, r, op, extent)
                    t_host = time.perf_counter() - t0
                    if not np.array_equal(out.cpu().numpy(), want) or not np.array_equal(stats.cpu().numpy(), want_stats):
                        raise SystemExit('device and host disagree: %s, %r mm, %s on %s' % (op, r, extent, shape))
                    checked += 1
                t = time_calls(lambda: ops.smooth_label(dev[0], values, spacing, r, op, extent), a.warmup, a.repeats)
                _, stats = ops.smooth_label(dev[0], values, spacing, r, op, extent)
                print('%s: %s, %g mm, %s: %.3f ms' % (shape, op, r, extent, 1e3 * t[0]), file=sys.stderr, flush=True)
                nbytes = model_bytes(op, reach, len(VALUES))
                rows.append(dict(op=op, radius_mm=r, extent=extent, reach=reach, ball=int(F.ball(spacing, r, extent).sum()), smooth_s=t[0],
                                 smooth_min_max_s=t[1:], host_s=t_host, bytes_per_voxel=nbytes,
                                 hbm_share=nbytes * pred.size / t[0] / HBM_PEAK, stats=stats.cpu().numpy().tolist()))
    t_keep = time_calls(lambda: ops.keep_largest_components(dev[0], values, 6), a.warmup, a.repeats)
    t_fill = time_calls(lambda: ops.fill_label_holes(dev[0], values, '2d'), a.warmup, a.repeats)
    smoothed, _ = ops.smooth_label(dev[0], values, spacing, RADII[0], 'smooth', '2d')
    t_metrics = time_calls(lambda: ops.surface_metrics(smoothed, dev[1], values, spacing), a.warmup, a.repeats)
    return dict(shape=shape, spacing=spacing, voxels=int(pred.size), salt=a.salt, pepper=a.pepper, rows=rows, keep_largest_s=t_keep[0],
                keep_largest_min_max_s=t_keep[1:], fill_holes_s=t_fill[0], fill_holes_min_max_s=t_fill[1:],
                surface_metrics_s=t_metrics[0], surface_metrics_min_max_s=t_metrics[1:])


def write_up(path, a, results, skipped, device):
    lines = ['# Opening, closing and smoothing of one predicted label volume: ops.smooth_label', '',
             'Four organs, smooth-field labels with %.2g of the voxels replaced by a random organ (salt) and %.2g by 0 (pepper).'
             % (a.salt, a.pepper),
             'Device: event time, %d warm-up calls, median of %d calls (min .. max in brackets).  Host: the scipy restatement'
             % (a.warmup, a.repeats),
             '(tests/volume_smooth_ref.py), timed once on the same machine where a time is given; its volume and stats equal the',
             'device\'s.  Bytes per voxel: what the kernels of the configuration read and write if every volume crosses the memory bus',
             'once per kernel (2 per map of runs along x, 3 or 4 per pass over the rows of the ball, per organ and erosion or dilation);',
             'HBM share: those bytes over the measured time, against %.0f TB/s.  %s.' % (HBM_PEAK / 1e12, device),
             'Command: `python tools/volume_smooth_bench.py`', '']
    for r in results:
        lines += ['## %s at %s mm (%d voxels)' % (' x '.join(str(v) for v in r['shape']), ' x '.join('%g' % s for s in r['spacing']),
                                                r['voxels']), '',
                  '| step | reach (z, y, x), voxels of the ball | device | host (scipy) | bytes per voxel | HBM share |', '|---|---|---|---|---|---|']
        for m in r['rows']:
            lines.append('| smooth_label %s, %g mm, %s | %s, %d | %.3f ms (%.3f .. %.3f) | %s | %d | %.1f %% |'
                         % (m['op'], m['radius_mm'], m['extent'], tuple(m['reach']), m['ball'], 1e3 * m['smooth_s'],
                            1e3 * m['smooth_min_max_s'][0], 1e3 * m['smooth_min_max_s'][1],
                            '' if m['host_s'] is None else '%.0f ms' % (1e3 * m['host_s']), m['bytes_per_voxel'], 100 * m['hbm_share']))
        for name, key in (('keep_largest_components, connectivity 6', 'keep_largest'), ('fill_label_holes 2d', 'fill_holes'),
                          ('surface_metrics (smoothed prediction against the truth)', 'surface_metrics')):
            lines.append('| %s | | %.3f ms (%.3f .. %.3f) | | | |' % (name, 1e3 * r[key + '_s'], 1e3 * r[key + '_min_max_s'][0],
                                                                     1e3 * r[key + '_min_max_s'][1]))
        lines.append('')
        worst = max(r['rows'], key=lambda m: m['smooth_s'])
        ratio = worst['smooth_s'] / r['surface_metrics_s']
        lines.append('The slowest configuration (%s, %g mm, %s) takes %.2f times the time of surface_metrics on the same volume: it '
                     'costs %s than the scores in mm.' % (worst['op'], worst['radius_mm'], worst['extent'], ratio,
                                                           'MORE' if ratio > 1 else 'less'))
        first = r['rows'][0]
        lines.append('Per organ (voxels before, removed, added) of %s, %g mm, %s: %s.' % (first['op'], first['radius_mm'], first['extent'],
                                                                                       first['stats']))
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
                                                  'volume_smooth_bench.md'))
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit('volume_smooth_bench needs a GPU: a time measured without one says nothing')
    if a.repeats < 10:
        raise SystemExit('at least 10 repeats')
    nn.set_default_device('cuda:0')
    results, skipped = [], []
    for i, (shape, spacing) in enumerate(SHAPES):
        need = BYTES_PER_VOXEL * int(np.prod(shape))
        free = torch.cuda.mem_get_info(0)[0]
        if need > free // 2:
            skipped.append((shape, 'needs about %d MB, %d MB are free' % (need >> 20, free >> 20)))
            continue
        results.append(measure(a, shape, spacing, check_all=i == 0))
    device = torch.cuda.get_device_name(0)
    print(json.dumps(dict(device=device, results=results, skipped=skipped)))
    write_up(a.out, a, results, skipped, device)


if __name__ == '__main__':
    main()
