#!/usr/bin/env python
"""Time of HD(q) and NSD(tau) of one predicted label volume: ops.surface_scores beside ops.surface_metrics on the device
(csrc/postprocess.hip), and the numpy / scipy restatement (tests/volume_robust_ref.py) on the host it runs on.

Workload: the volumes of tools/volume_metrics_bench.py (a 36 x 320 x 320 MR pair and a 100 x 512 x 512 CT pair, four organs and their
union), q = 95, tau = 1 mm.
  device   event time of ops.surface_scores and of ops.surface_metrics at the same commit, each after `--warmup` calls, median of
           `--repeats`; their difference is what compaction and selection cost.  Beside it ops.masked_select alone on the union's
           two distance maps and surfaces.
  host     the restatement over the first `--host_problems` binary problems, scaled to all five; its count and percentile must agree
           with the device's (count equal, percentile to 2e-12 relative) or the tool fails
Prints one JSON line and writes the write-up to `--out`.

    python tools/volume_robust_bench.py [--repeats 10] [--warmup 2] [--host_problems 1] [--out profiles/volume_robust_bench.md]
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np
import torch

from multimodal_segmentation_amd import nn, ops
from tests import volume_metrics_ref as M
from tests import volume_robust_ref as B
from volume_metrics_bench import SHAPES, VALUES, make_pair, time_calls

Q, TAU = 95.0, 1.0


def measure(shape, spacing, a):
    pred, truth = make_pair(np.random.RandomState(11), shape)
    K = len(VALUES)
    dev = [nn.host_to_device(x, 'cuda:0', np.uint8) for x in (pred, truth)]
    values = nn.host_to_device(np.asarray(VALUES), 'cuda:0', np.int32)
    t_metrics = time_calls(lambda: ops.surface_metrics(dev[0], dev[1], values, spacing), a.warmup, a.repeats)
    t_scores = time_calls(lambda: ops.surface_scores(dev[0], dev[1], values, spacing, Q, TAU), a.warmup, a.repeats)
    table = ops.surface_scores(dev[0], dev[1], values, spacing, Q, TAU).cpu().numpy()
    if not np.array_equal(table[:, :6].view(np.uint64), ops.surface_metrics(dev[0], dev[1], values, spacing).cpu().numpy().view(np.uint64)):
        raise SystemExit('the first six columns differ from ops.surface_metrics')
    # the selection alone, on the union's maps
    surf = [ops.label_surface(x, values)[K].contiguous() for x in dev]
    maps = [ops.distance_to_sites(surf[1], spacing), ops.distance_to_sites(surf[0], spacing)]          # to T over P, to P over T
    t_select = time_calls(lambda: ops.masked_select(maps[0], surf[0], maps[1], surf[1], Q, TAU), a.warmup, a.repeats)
    alone = ops.masked_select(maps[0], surf[0], maps[1], surf[1], Q, TAU).cpu().numpy()
    if alone[1] != table[K, 6] or alone[2] != table[K, 7]:
        raise SystemExit('ops.masked_select and ops.surface_scores disagree on the union')
    order = list(range(K + 1))[:a.host_problems]
    t0 = time.perf_counter()
    want = []
    for k in order:
        d = B.distances(M.problems(pred, VALUES)[k], M.problems(truth, VALUES)[k], spacing)
        want.append([np.count_nonzero(d <= TAU), np.percentile(d, Q)])
    t_host = (time.perf_counter() - t0) * (K + 1) / float(len(order))
    want = np.asarray(want, np.float64)
    got = table[order][:, 6:]
    rel = float(np.max(np.abs(got[:, 1] - want[:, 1]) / want[:, 1]))
    if not np.array_equal(got[:, 0], want[:, 0]) or rel > 2e-12:
        raise SystemExit('device and host disagree: counts %s / %s, percentile %.3g relative' % (got[:, 0], want[:, 0], rel))
    n_list = float(table[K, 2] + table[K, 3])
    return dict(shape=shape, spacing=spacing, voxels=pred.size, surface_scores_s=t_scores[0], surface_scores_min_max_s=t_scores[1:],
                surface_metrics_s=t_metrics[0], surface_metrics_min_max_s=t_metrics[1:], masked_select_s=t_select[0],
                union_list=n_list, union_list_share=n_list / (2.0 * pred.size), host_s=t_host, host_problems_timed=len(order), rel_hd=rel,
                hd_mm=float(table[K, 7]), mssd_mm=float(table[K, 5]), nsd=float(table[K, 6] / n_list))


def write_up(path, a, results, device):
    lines = ['# HD(q) and NSD(tau) of one predicted label volume: `ops.surface_scores`', '',
             'Workload: the volumes of `tools/volume_metrics_bench.py`, four organs and their union, q = %g, tau = %g mm.  `surface_scores`' % (Q, TAU),
             'is `surface_metrics` plus, per problem, two compaction sweeps (a byte mask and the selected doubles) and eight radix passes',
             'over the list of surface distances.  Device: event time, %d warm-up calls, median of %d calls (min .. max in brackets).' % (a.warmup, a.repeats),
             '`masked_select` alone: the union\'s two maps and surfaces.  Host: the numpy / scipy restatement (`tests/volume_robust_ref.py`)',
             'timed on %d of the 5 problems and scaled.  %s.' % (a.host_problems, device), '',
             'Command: `python tools/volume_robust_bench.py`', '',
             '| volume | surface_metrics | surface_scores | difference | per problem | masked_select (union) | union list | host (scipy) |',
             '|---|---|---|---|---|---|---|---|']
    for r in results:
        extra = r['surface_scores_s'] - r['surface_metrics_s']
        lines.append('| %s | %.2f ms (%.2f .. %.2f) | %.2f ms (%.2f .. %.2f) | %.2f ms (%.1f %%) | %.3f ms | %.3f ms | %d values, %.1f %% of 2 n | %.1f s |'
                     % (' x '.join(str(v) for v in r['shape']), 1e3 * r['surface_metrics_s'], 1e3 * r['surface_metrics_min_max_s'][0],
                        1e3 * r['surface_metrics_min_max_s'][1], 1e3 * r['surface_scores_s'], 1e3 * r['surface_scores_min_max_s'][0],
                        1e3 * r['surface_scores_min_max_s'][1], 1e3 * extra, 100 * extra / r['surface_metrics_s'], 1e3 * extra / 5.0,
                        1e3 * r['masked_select_s'], r['union_list'], 100 * r['union_list_share'], r['host_s']))
    lines += ['', 'Agreement in the same run (the problems the host timed): %s.'
              % '; '.join('%s: count equal, percentile %.2g relative; union HD95 %.3f mm beside MSSD %.3f mm, NSD %.3f'
                          % (' x '.join(str(v) for v in r['shape']), r['rel_hd'], r['hd_mm'], r['mssd_mm'], r['nsd']) for r in results), '']
    with open(path, 'w') as f:
        f.write('\n'.join(lines))


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('--repeats', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--host_problems', type=int, default=1)
    ap.add_argument('--out', default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'profiles',
                                                  'volume_robust_bench.md'))
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit('volume_robust_bench needs a GPU: a time measured without one says nothing')
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
