#!/usr/bin/env python
"""What the CRF refinement of predicted maps costs for one CHAOS-sized volume: 30 slices of 256 x 256, soft-max maps with C = 5 channels
(four organs and the background), 5 mean-field iterations, window radius 3, 5 (the default) and 8.

  refine    event time of ops.crf_refine (csrc/crf.hip: the table, Q^0 and one launch per iteration), with the neighbour visits per
            second it reaches (pixels x ((2r + 1)^2 - 1) x iterations / time) and the bytes one pixel reads per iteration
  restore   event time of ops.restore_label of the refined map onto a raw grid of 320 x 320
  numpy     wall time of the fp64 numpy restatement (tests/volume_crf_ref.py) on ONE slice
  model     event time of DAFNet.predict_mask(0, 'simple') over the 30 slices in batches of `--batch`.  Skipped with --no-model
  errors    per case of tests/test_volume_crf.py the largest difference of the device map from the fp64 restatement, beside e32 (the
            restatement's own lines in fp32) and the bar max(8 e32, 2e-6)
Each time after `--warmup` calls, median of `--repeats`.  Prints one JSON line and writes the write-up to `--out`.

    python tools/volume_crf_bench.py [--repeats 20] [--warmup 3] [--batch 10] [--no-model] [--out profiles/volume_crf_bench.md]
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

VALUES = [63, 126, 189, 252]
SLICES, INPUT, RAW, C, K, ITERATIONS = 30, 256, (320, 320), 5, 4, 5
RADII = (3, 5, 8)
TILE = (8, 32)          # the output tile of a block of csrc/crf.hip


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


def bytes_per_pixel(r):
    """what one pixel reads in one iteration: its share of the staged image and Q planes (tile and halo), its own channels of prob"""
    halo = (TILE[0] + 2 * r) * (TILE[1] + 2 * r) / float(TILE[0] * TILE[1])
    return 4.0 * (halo * (1 + K + 1) + C)


def inputs(rng):
    """(prob [SLICES,INPUT,INPUT,C], image [SLICES,INPUT,INPUT,1]) fp32: a soft-max over smooth fields and a smooth image, 10 distinct slices"""
    f = 4.0 * np.concatenate([Hh.smooth_field(rng, 10, INPUT, INPUT, sigma=8.0) for _ in range(C)], axis=-1).astype(np.float64)
    e = np.exp(f - f.max(-1, keepdims=True))
    prob = (e / e.sum(-1, keepdims=True)).astype(np.float32)[np.arange(SLICES) % 10]
    image = np.clip(Hh.smooth_field(rng, 10, INPUT, INPUT, sigma=6.0), -1, 1).astype(np.float32)[np.arange(SLICES) % 10]
    return prob, image


def errors(dev):
    from tests import test_volume_crf as cases
    from tests import volume_crf_ref as A
    out = {}
    for name in sorted(cases.CASES):
        (H, W), c, k, r, _ = cases.CASES[name]
        prob, image = cases._inputs(name)
        want, e32 = cases._want(name)
        got = ops.crf_refine(nn.host_to_device(np.array(prob), dev, np.float32), nn.host_to_device(np.array(image), dev, np.float32), k,
                             A.with_defaults(radius=r))
        out[name] = dict(C=c, K=k, radius=r, device=float(np.abs(got.cpu().numpy().astype(np.float64) - want).max()), e32=e32,
                         bar=max(A.MARGIN * e32, A.FLOOR_BAR))
    return out


def measure(a):
    from tests import volume_crf_ref as A
    dev = 'cuda:0'
    prob_h, image_h = inputs(np.random.RandomState(3))
    prob, image = nn.host_to_device(prob_h, dev, np.float32), nn.host_to_device(image_h, dev, np.float32)
    values = nn.host_to_device(np.asarray(VALUES), dev, np.int32)
    out = dict(radii={}, errors=errors(dev))
    pixels = SLICES * INPUT * INPUT
    for r in RADII:
        params = ops.CRF_DEFAULTS._replace(radius=r, iterations=ITERATIONS)
        t = time_calls(lambda: ops.crf_refine(prob, image, K, params), a.warmup, a.repeats)
        start = time.time()
        A.refine(prob_h[:1], image_h[:1], K, tuple(params))
        out['radii'][r] = dict(refine_s=t, visits_per_s=pixels * ((2 * r + 1) ** 2 - 1) * ITERATIONS / t[0], bytes_per_pixel=bytes_per_pixel(r),
                               numpy_one_slice_s=time.time() - start)
    refined = ops.crf_refine(prob, image, K)
    out['restore_s'] = time_calls(lambda: ops.restore_label(refined, values, RAW, (INPUT, INPUT), (0, INPUT, 0), (0, INPUT, 0), 1), a.warmup,
                                  a.repeats)
    if not a.no_model:
        from multimodal_segmentation_amd.configuration import dafnet_config_chaos
        from multimodal_segmentation_amd.models.dafnet import DAFNet
        from multimodal_segmentation_amd.volume_predictor import VolumePredictor
        conf = Hh.make_conf(dafnet_config_chaos, INPUT, batch_size=a.batch)
        model = DAFNet(conf)
        model.build()
        predictor = VolumePredictor(model, conf)
        few = max(1, a.repeats // 4)
        out['model_s'] = time_calls(lambda: predictor.predict_volume(0, 'simple', [image, image]), 1, few)
        out['model_batch'], out['model_repeats'] = a.batch, few
    return out


def ms(t):
    return '%.3f ms (%.3f .. %.3f)' % (1e3 * t[0], 1e3 * t[1], 1e3 * t[2])


def write_up(path, a, r, device):
    lines = ['# CRF refinement of one volume\'s probability maps: ops.crf_refine beside the forward pass and the way back', '',
             '%d slices of %d x %d, C = %d channels, K = %d organs (L = %d labels), %d iterations; weights and theta at their defaults.'
             % (SLICES, INPUT, INPUT, C, K, K + 1, ITERATIONS),
             'Event time, %d warm-up calls, median of %d calls (min .. max in brackets).' % (a.warmup, a.repeats),
             '%s.  Command: `python tools/volume_crf_bench.py`' % device, '',
             '| radius | neighbours | crf_refine, %d iterations | per iteration | neighbour visits / s | bytes read per pixel and iteration | numpy '
             'restatement, ONE slice |' % ITERATIONS, '|---|---|---|---|---|---|---|']
    for radius in RADII:
        v = r['radii'][radius] if radius in r['radii'] else r['radii'][str(radius)]
        lines.append('| %d | %d | %s | %.3f ms | %.3g | %.0f | %.2f s |' % (radius, (2 * radius + 1) ** 2 - 1, ms(v['refine_s']),
                                                                          1e3 * v['refine_s'][0] / ITERATIONS, v['visits_per_s'],
                                                                          v['bytes_per_pixel'], v['numpy_one_slice_s']))
    at5 = r['radii'][5] if 5 in r['radii'] else r['radii']['5']
    lines += ['', 'A back-of-envelope count (about 120 neighbours x 18 lane operations x 2 M pixels) had put an iteration at radius 5 near '
              '0.1 ms; measured: %.3f ms.' % (1e3 * at5['refine_s'][0] / ITERATIONS),
              'The time per iteration includes a fifth of the two launches that come once per call (the table, Q^0).  Bytes: the staged '
              'image and Q planes of the 8 x 32 tile with its halo, shared among the tile\'s pixels, and the pixel\'s own channels of prob; '
              'they come from the last-level cache, which holds these sizes.  The kernel is bound by its arithmetic and LDS reads, not '
              'by these bytes: per neighbour one exp2, L LDS reads and 2 L multiply-adds.',
              '', '`restore_label` of the refined map onto %d x %d, order 1: %s.' % (RAW[0], RAW[1], ms(r['restore_s']))]
    if 'model_s' in r:
        default = r['radii'][5] if 5 in r['radii'] else r['radii']['5']
        ratio = default['refine_s'][0] / r['model_s'][0]
        lines += ['', 'DAFNet.predict_mask(0, \'simple\') over the %d slices, batches of %d, median of %d: %s.  The refinement at the defaults '
                  '(radius 5) takes %.2f times that.' % (SLICES, r['model_batch'], r['model_repeats'], ms(r['model_s']), ratio)]
        if ratio > 1:
            lines += ['It costs more than the forward pass it follows: every pixel visits 120 neighbours for each of 5 labels in each of 5 '
                      'iterations, 3000 multiply-add pairs per pixel, where the network spends its arithmetic on the matrix cores.']
    else:
        lines += ['', 'The model\'s forward: NOT MEASURED (--no-model).']
    lines += ['', '## Errors against the fp64 restatement', '',
              'The cases of tests/test_volume_crf.py, 3 slices each, defaults but the radius.  e32: the restatement\'s own lines in fp32.', '',
              '| case | C | K | radius | device | e32 | bar max(8 e32, 2e-6) | device / e32 |', '|---|---|---|---|---|---|---|---|']
    for name in sorted(r['errors']):
        e = r['errors'][name]
        lines.append('| %s | %d | %d | %d | %.2e | %.2e | %.2e | %s |' % (name, e['C'], e['K'], e['radius'], e['device'], e['e32'], e['bar'],
                                                                        '%.1f' % (e['device'] / e['e32']) if e['e32'] > 0 else '-'))
    with open(path, 'w') as f:
        f.write('\n'.join(lines) + '\n')


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('--repeats', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--batch', type=int, default=10)
    ap.add_argument('--no-model', dest='no_model', action='store_true')
    ap.add_argument('--out', default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'profiles',
                                                  'volume_crf_bench.md'))
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit('volume_crf_bench needs a GPU: a time measured without one says nothing')
    if a.repeats < 10:
        raise SystemExit('at least 10 repeats')
    nn.set_default_device('cuda:0')
    result = measure(a)
    device = '%s (%s)' % (torch.cuda.get_device_name(0), str(getattr(torch.cuda.get_device_properties(0), 'gcnArchName', '?')).split(':')[0])
    print(json.dumps(dict(device=device, result=result)))
    write_up(a.out, a, result, device)


if __name__ == '__main__':
    main()
