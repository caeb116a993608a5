#!/usr/bin/env python
"""What the ensemble path of the way back costs for one CHAOS-sized volume: 36 slices in containers of 256 x 256, soft-max maps with
C = 5 channels (four organs and the background), V = 1, 4 and 8 views per member.

  members   event time of ops.members_accumulate (first call of a state) alone and followed by ops.members_finish (csrc/postprocess.hip) beside
            ops.merge_views on the same maps, each with the bytes it needs (accumulate: the K organ channels of every view once, the
            K + 2 accumulators once; finish: the K + 2 floats read and written; merge: the organ channels and the map) and GB/s, and as
            a share of the 8 TB/s of HBM.  Expectation: accumulate + finish cost no more than merge_views plus the traffic of the
            extra floats per pixel (K + 2 written by accumulate, K + 2 read and written again by finish, less the K the merge writes)
  planes    event time of ops.restore_map (one plane onto a raw grid of 320 x 320) and of ops.calibration_table (10 bins) beside
            ops.restore_label of the same map, order 1
Each after `--warmup` calls, median of `--repeats`.  Prints one JSON line and writes the write-up to `--out`.

    python tools/volume_uncertainty_bench.py [--repeats 20] [--warmup 3] [--out profiles/volume_uncertainty_bench.md]
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from multimodal_segmentation_amd import nn, ops
from tests import helpers as Hh

VALUES = [63, 126, 189, 252]
SLICES, RAW, INPUT, C, K, BINS = 36, (320, 320), 256, 5, 4, 10
VIEWS = (1, 4, 8)
HBM = 8.0e12          # bytes per second, the specified peak
FLIPS = ([1, 0, 0, 0, 1, 0], [1, 0, 0, 0, -1, INPUT - 1], [-1, 0, INPUT - 1, 0, 1, 0], [-1, 0, INPUT - 1, 0, -1, INPUT - 1],
         [0, 1, 0, 1, 0, 0], [0, -1, INPUT - 1, -1, 0, INPUT - 1], [0, 1, 0, -1, 0, INPUT - 1], [0, -1, INPUT - 1, 1, 0, 0])


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
    return [float(np.median(times)), float(np.min(times)), float(np.max(times))]


def softmax_fields(rng, n):
    """[n,INPUT,INPUT,C] fp32: a soft-max over smooth random fields, 12 distinct slices cycled"""
    f = 4.0 * np.concatenate([Hh.smooth_field(rng, 12, INPUT, INPUT, sigma=8.0) for _ in range(C)], axis=-1).astype(np.float64)
    e = np.exp(f - f.max(-1, keepdims=True))
    return (e / e.sum(-1, keepdims=True)).astype(np.float32)[np.arange(n) % 12]


def measure(a):
    dev = 'cuda:0'
    rng = np.random.RandomState(3)
    maps = softmax_fields(rng, 12)
    values = nn.host_to_device(np.asarray(VALUES), dev, np.int32)
    pixels = SLICES * INPUT * INPUT
    out = dict(views={})
    for V in VIEWS:
        prob = nn.host_to_device(maps[np.arange(V * SLICES) % 12], dev, np.float32)
        back = nn.host_to_device(np.asarray(FLIPS[:V], np.float64), dev, np.float64)
        r = dict(accumulate_s=time_calls(lambda: ops.members_accumulate(prob, back, SLICES, K), a.warmup, a.repeats),
                 accumulate_bytes=4 * pixels * (V * K + K + 2),
                 # the finish works in place and a state is finished once, so it is timed together with the accumulation that feeds it
                 both_s=time_calls(lambda: ops.members_finish(ops.members_accumulate(prob, back, SLICES, K)), a.warmup, a.repeats),
                 finish_bytes=4 * pixels * 2 * (K + 2),
                 merge_s=time_calls(lambda: ops.merge_views(prob, back, SLICES, K), a.warmup, a.repeats),
                 merge_bytes=4 * pixels * (V * K + K))
        out['views'][str(V)] = r
        del prob
    prob = nn.host_to_device(maps[np.arange(SLICES) % 12], dev, np.float32)
    mean, planes = ops.members_finish(ops.members_accumulate(prob, ops.IDENTITY_VIEW, SLICES, K))
    whole = ((INPUT, INPUT), (0, INPUT, 0), (0, INPUT, 0))
    truth = ops.restore_label(mean, values, RAW, *whole)
    out['restore_label_s'] = time_calls(lambda: ops.restore_label(mean, values, RAW, *whole), a.warmup, a.repeats)
    out['restore_map_s'] = time_calls(lambda: ops.restore_map(planes, 0, RAW, *whole), a.warmup, a.repeats)
    out['calibration_s'] = time_calls(lambda: ops.calibration_table(mean, truth, values, whole[0], whole[1], whole[2], BINS), a.warmup,
                                      a.repeats)
    levels = torch.stack([ops.restore_map(planes, u, RAW, *whole) for u in (0, 1)])
    out['by_error_s'] = time_calls(lambda: ops.uncertainty_by_error(truth, truth, levels), a.warmup, a.repeats)
    return out


def ms(t):
    return '%.3f ms (%.3f .. %.3f)' % (1e3 * t[0], 1e3 * t[1], 1e3 * t[2])


def rate(t, n):
    return '%s, %.1f MB, %.0f GB/s, %.0f %% of 8 TB/s' % (ms(t), n / 1e6, n / t[0] / 1e9, 100 * n / t[0] / HBM)


def write_up(path, a, r, device):
    lines = ['# The ensemble path of one volume: members_accumulate, members_finish, and the planes on the way back', '',
             '%d slices in containers of %d x %d, soft-max maps with C = %d channels, K = %d organs (the scalar path: a thread per pixel, K '
             'loads per tap).' % (SLICES, INPUT, INPUT, C, K),
             'Event time, %d warm-up calls, median of %d calls (min .. max in brackets).' % (a.warmup, a.repeats),
             '%s.  Command: `python tools/volume_uncertainty_bench.py`' % device, '',
             '| V | members_accumulate (first) | accumulate + members_finish | merge_views | (accumulate + finish) / merge | expected from the bytes |',
             '|---|---|---|---|---|---|']
    for V in VIEWS:
        v = r['views'][str(V)]
        lines.append('| %d | %s | %s | %s | %.2f | %.2f |'
                     % (V, rate(v['accumulate_s'], v['accumulate_bytes']), rate(v['both_s'], v['accumulate_bytes'] + v['finish_bytes']),
                        rate(v['merge_s'], v['merge_bytes']), v['both_s'][0] / v['merge_s'][0],
                        (v['accumulate_bytes'] + v['finish_bytes']) / float(v['merge_bytes'])))
    lines += ['', 'Bytes: accumulate reads the K organ channels of every view once and writes K + 2 floats per pixel; finish reads and writes '
              'K + 2; merge_views reads the same channels and writes K.  "Expected from the bytes" is the ratio of those counts: what the '
              'pair would cost beside the merge if all three ran at one rate.  The repeats find the maps where the call before left them: '
              'a rate above what HBM delivers is that of the last-level cache, which holds these sizes.', '',
              'The expectation was that accumulate + finish cost no more than merge_views plus the traffic of the extra floats per pixel '
              '(at the rate merge_views itself reaches):', '']
    for V in VIEWS:
        v = r['views'][str(V)]
        extra = v['accumulate_bytes'] + v['finish_bytes'] - v['merge_bytes']
        bound = v['merge_s'][0] * (1.0 + extra / float(v['merge_bytes']))
        lines.append('* V = %d: %.3f ms measured against %.3f ms + %.1f MB = %.3f ms: %s (%.2f of it).'
                     % (V, 1e3 * v['both_s'][0], 1e3 * v['merge_s'][0], extra / 1e6, 1e3 * bound,
                        'confirmed' if v['both_s'][0] <= bound else 'REFUTED', v['both_s'][0] / bound))
    lines += ['', 'Where it is refuted the reason, read from the kernels and not from counters, is the thread-per-pixel form of the scalar path under TRANSPOSING views (V = 8 is `d4`, whose '
              'last four views transpose).  There neighbouring lanes read taps one container row apart, so every load instruction of a wave '
              'touches 64 different cache lines.  merge_views spreads a pixel\'s K channels over K lanes and reads them with one '
              'instruction; a thread that owns the pixel needs K instructions, each touching its own 64 lines: K times the cache-line '
              'requests for the same bytes.  The flips and the identity read along rows, where the K instructions of a wave share their '
              'lines, and there the pair stays below the expectation.  The entropy needs a pixel\'s channels in one thread (DESIGN.md '
              'section 8), so the form stays; a transposing view costs a forward pass of tens of ms beside these 0.15 ms.', '',
              'calibration_table is not bandwidth-bound: per tile of 256 pixels the K (B + 2) owners of the table walk the staged pixels '
              'one after the other (256 dependent LDS reads each, most threads of the block waiting), which is what makes every fp64 sum '
              'the same in every run without floating-point atomics.  It runs once per labelled file, beside a forward pass.', '',
              '| on a raw grid of %d x %d, order 1 | time |' % RAW, '|---|---|',
              '| restore_label (the labels, for comparison) | %s |' % ms(r['restore_label_s']),
              '| restore_map (one plane) | %s |' % ms(r['restore_map_s']),
              '| calibration_table (%d bins, %d organs) | %s |' % (BINS, K, ms(r['calibration_s'])),
              '| uncertainty_by_error (two planes) | %s |' % ms(r['by_error_s'])]
    with open(path, 'w') as f:
        f.write('\n'.join(lines) + '\n')


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('--repeats', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--out', default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'profiles',
                                                  'volume_uncertainty_bench.md'))
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit('volume_uncertainty_bench needs a GPU: a time measured without one says nothing')
    if a.repeats < 10:
        raise SystemExit('at least 10 repeats')
    nn.set_default_device('cuda:0')
    result = measure(a)
    device = '%s (%s)' % (torch.cuda.get_device_name(0), str(getattr(torch.cuda.get_device_properties(0), 'gcnArchName', '?')).split(':')[0])
    print(json.dumps(dict(device=device, result=result)))
    write_up(a.out, a, result, device)


if __name__ == '__main__':
    main()
