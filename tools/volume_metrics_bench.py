#!/usr/bin/env python
"""Time of the scores in mm of one predicted label volume: ops.surface_metrics on the device (csrc/postprocess.hip) beside the scipy
restatement (tests/volume_metrics_ref.py) on the host it runs on.

Workload: a 36 x 320 x 320 pair (a CHAOS MR volume) and a 100 x 512 x 512 pair (a CT volume), four organs and their union.  The truth
is the arg-max over five smooth random fields, the prediction the arg-max of the same fields plus 0.35 times a second set.
  device   event time of ops.surface_metrics, ops.label_surface and ops.distance_to_sites, each after `--warmup` calls, median of
           `--repeats`; beside it the bytes the passes have to move (every map read once and written once) over that time
  host     the restatement over the first `--host_problems` binary problems, scaled to all five; its table must agree with the
           device's (counts equal, maximum to 1e-12, sum to 1e-9 relative) or the tool fails
Prints one JSON line and writes the write-up to `--out`.

    python tools/volume_metrics_bench.py [--repeats 10] [--warmup 2] [--host_problems 1] [--out profiles/volume_metrics_bench.md]
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
from tests import volume_metrics_ref as M
from tests.volume_metrics_ref import problems, surface

VALUES = [63, 126, 189, 252]
HBM_BYTES_PER_S = 8e12
SHAPES = (((36, 320, 320), (7.7, 1.6, 1.6)), ((100, 512, 512), (3.0, 0.8, 0.8)))


def make_pair(rng, shape):
    """(pred, truth) uint8: fields of 12 distinct slices, cycled along the volume"""
    S, H, W = shape
    f = np.concatenate([Hh.smooth_field(rng, 12, H, W, sigma=H / 16.0) for _ in range(5)], axis=-1).astype(np.float32)
    g = np.concatenate([Hh.smooth_field(rng, 12, H, W, sigma=H / 16.0) for _ in range(5)], axis=-1).astype(np.float32)
    grey = np.asarray([0] + VALUES, np.uint8)
    which = np.arange(S) % 12
    return grey[np.argmax(f + 0.35 * g, axis=-1)][which], grey[np.argmax(f, axis=-1)][which]


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


def measure(shape, spacing, a):
    pred, truth = make_pair(np.random.RandomState(11), shape)
    n, K = pred.size, len(VALUES)
    dev = [nn.host_to_device(x, 'cuda:0', np.uint8) for x in (pred, truth)]
    values = nn.host_to_device(np.asarray(VALUES), 'cuda:0', np.int32)
    sites = ops.label_surface(dev[1], values)[K].contiguous()
    t_all = time_calls(lambda: ops.surface_metrics(dev[0], dev[1], values, spacing), a.warmup, a.repeats)
    t_surface = time_calls(lambda: ops.label_surface(dev[1], values), a.warmup, a.repeats)
    t_distance = time_calls(lambda: ops.distance_to_sites(sites, spacing), a.warmup, a.repeats)
    table = ops.surface_metrics(dev[0], dev[1], values, spacing).cpu().numpy()
    # the host restatement of the first problems (the union last, so it is timed when all are), and agreement in the same run
    order = list(range(K + 1))[:a.host_problems]
    t0 = time.perf_counter()
    want = []
    for k in order:
        p, t = problems(pred, VALUES)[k], problems(truth, VALUES)[k]
        sp, st = surface(p), surface(t)
        d = np.concatenate([M.distance_map(st, spacing)[sp], M.distance_map(sp, spacing)[st]])
        want.append([p.sum(), t.sum(), sp.sum(), st.sum(), d.sum(), d.max()])
    t_host = (time.perf_counter() - t0) * (K + 1) / float(len(order))
    want = np.asarray(want, np.float64)
    got = table[order]
    if not np.array_equal(got[:, :4], want[:, :4]):
        raise SystemExit('device and host counts disagree')
    rel_sum = float(np.max(np.abs(got[:, 4] - want[:, 4]) / want[:, 4]))
    rel_max = float(np.max(np.abs(got[:, 5] - want[:, 5]) / want[:, 5]))
    if rel_sum > 1e-9 or rel_max > 1e-12:
        raise SystemExit('device and host distances disagree: sum %.3g, max %.3g relative' % (rel_sum, rel_max))
    # bytes every pass has to move: a map read once, written once
    b_surface = n + (K + 1) * n
    b_distance = (n + 8 * n) + 16 * n + 16 * n                      # W pass from bytes, H pass, S pass
    b_all = 2 * b_surface + 2 * (K + 1) * (b_distance + 9 * n)       # + the reduction: a surface and a distance map
    return dict(shape=shape, spacing=spacing, voxels=n, surface_metrics_s=t_all[0], surface_metrics_min_max_s=t_all[1:],
                label_surface_s=t_surface[0], distance_to_sites_s=t_distance[0], bytes_surface=b_surface, bytes_distance=b_distance,
                bytes_all=b_all, candidates_per_voxel=sum(shape), host_s=t_host, host_problems_timed=len(order), rel_sum=rel_sum,
                rel_max=rel_max, assd_mm=float(table[K, 4] / (table[K, 2] + table[K, 3])), mssd_mm=float(table[K, 5]))


def write_up(path, a, results, device):
    lines = ['# Scores in mm of one predicted label volume: `ops.surface_metrics`', '',
             'Workload: a predicted and a true label volume, four organs and their union (five binary problems): surfaces of both',
             'volumes in one sweep each, then per problem two exact distance transforms (three per-axis fp64 minimum passes each) and two',
             'fixed-order reductions; only the [5,6] table leaves the device.  Device: event time, %d warm-up calls, median of %d calls'
             % (a.warmup, a.repeats),
             '(min .. max in brackets).  Host: the scipy restatement (`tests/volume_metrics_ref.py`: `binary_erosion`, two',
             '`distance_transform_edt` per problem) on the same machine, timed on %d of the 5 problems and scaled.  %s.' % (a.host_problems, device), '',
             'Command: `python tools/volume_metrics_bench.py`', '',
             '| volume | spacing mm | surface_metrics | bytes to move | achieved | of 8 TB/s | label_surface | achieved | distance_to_sites | achieved | host (scipy) |',
             '|---|---|---|---|---|---|---|---|---|---|---|']
    for r in results:
        lines.append('| %s | %s | %.2f ms (%.2f .. %.2f) | %.0f MB | %.2f TB/s | %.1f %% | %.3f ms | %.2f TB/s | %.3f ms | %.2f TB/s | %.1f s |'
                     % (' x '.join(str(v) for v in r['shape']), ', '.join('%g' % v for v in r['spacing']), 1e3 * r['surface_metrics_s'],
                        1e3 * r['surface_metrics_min_max_s'][0], 1e3 * r['surface_metrics_min_max_s'][1], r['bytes_all'] / 1e6,
                        r['bytes_all'] / r['surface_metrics_s'] / 1e12, 100 * r['bytes_all'] / r['surface_metrics_s'] / HBM_BYTES_PER_S,
                        1e3 * r['label_surface_s'], r['bytes_surface'] / r['label_surface_s'] / 1e12, 1e3 * r['distance_to_sites_s'],
                        r['bytes_distance'] / r['distance_to_sites_s'] / 1e12, r['host_s']))
    lines += ['', 'Bytes to move, per voxel: `label_surface` 1 in + 5 out; one distance transform 1 + 8 (pass along W, from the byte mask),',
              '8 + 8 (along H), 8 + 8 (along S) = 41; one reduction 1 + 8; the whole op 2 x 6 + 10 x (41 + 9) = 512.  The distance passes',
              'are bound by arithmetic, not by memory: every output takes the minimum over the whole line, %s candidates per voxel'
              % ' and '.join('%d' % r['candidates_per_voxel'] for r in results),
              '(W + H + S) of one fp64 multiply, fused multiply-add and minimum each, and a block of the strided passes reads its line',
              'once per 64 outputs, so the achieved rate above says how far the op is from streaming, not how fast it streams.  No target',
              'was set for this path: the parent commit had none to compare with.', '',
              'Agreement in the same run (the problems the host timed): %s.'
              % '; '.join('%s: counts equal, sum %.2g and maximum %.2g relative; union ASSD %.3f mm, MSSD %.3f mm'
                          % (' x '.join(str(v) for v in r['shape']), r['rel_sum'], r['rel_max'], r['assd_mm'], r['mssd_mm']) for r in results), '']
    with open(path, 'w') as f:
        f.write('\n'.join(lines))


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('--repeats', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--host_problems', type=int, default=1)
    ap.add_argument('--out', default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'profiles',
                                                  'volume_metrics_bench.md'))
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit('volume_metrics_bench needs a GPU: a time measured without one says nothing')
    if a.repeats < 10:
        raise SystemExit('at least 10 repeats')
    nn.set_default_device('cuda:0')
    a.host_problems = max(1, min(a.host_problems, len(VALUES) + 1))
    results = [measure(shape, spacing, a) for shape, spacing in SHAPES]
    device = torch.cuda.get_device_name(0)
    print(json.dumps(dict(device=device, results=results)))
    write_up(a.out, a, results, device)


if __name__ == '__main__':
    main()
