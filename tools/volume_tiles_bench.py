#!/usr/bin/env python
"""What whole-slice prediction costs for one CHAOS-sized volume: 36 slices of 256 x 256 raw pixels at 1.89 mm, whose resampled frame is
256 x 256 and needs 2 x 2 tiles of 192 x 192 (overlap: half the input extent).

  blend     event time of ops.blend_tiles (csrc/postprocess.hip) on the 4 x 36 soft-max containers [192,192,5], beside ops.restore_label
            of the blended map onto the raw grid and beside ops.restore_label of one container (the way back without the option)
  tiles in  event time of the 4 ops.preprocess_images calls of loader.load_volume_tiles (each repeats the min-max pass over the whole
            resampled frame), beside the one call of the centre window
  model     event time of DAFNet.predict_mask(0, 'simple') over the 4 x 36 tiles in batches of `--batch`, beside the 36 centre windows;
            skipped with --no-model
Each after `--warmup` calls, median of `--repeats`.  Prints one JSON line and writes the write-up to `--out`.

    python tools/volume_tiles_bench.py [--repeats 20] [--warmup 3] [--batch 12] [--no-model] [--out profiles/volume_tiles_bench.md]
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from multimodal_segmentation_amd import nn, ops
from multimodal_segmentation_amd.loaders.volume_folder import crop_pad_map, tile_axis, tile_weights
from tests import helpers as Hh

VALUES = [63, 126, 189, 252]
SLICES, RAW, FRAME, INPUT, C = 36, (256, 256), (256, 256), 192, 5


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
    rows, cols = tile_axis(FRAME[0], INPUT, INPUT // 2), tile_axis(FRAME[1], INPUT, INPUT // 2)
    T = len(rows) * len(cols)
    assert T == 4
    wr, wc = tile_weights(rows, INPUT), tile_weights(cols, INPUT)
    centre = crop_pad_map(FRAME[0], INPUT), crop_pad_map(FRAME[1], INPUT)
    values = nn.host_to_device(np.asarray(VALUES), dev, np.int32)
    prob = nn.host_to_device(softmax_fields(rng, T * SLICES), dev, np.float32)
    tables = [torch.as_tensor(x, device=dev) for x in (np.asarray(rows, np.int32), np.asarray(cols, np.int32), wr, wc)]
    blended = ops.blend_tiles(prob, *tables, SLICES, FRAME, 4)
    whole = (0, FRAME[0], 0), (0, FRAME[1], 0)
    out = dict(tiles=[len(rows), len(cols)], rows=rows, cols=cols)
    out['blend_tiles_s'] = time_calls(lambda: ops.blend_tiles(prob, *tables, SLICES, FRAME, 4), a.warmup, a.repeats)
    out['restore_blended_s'] = time_calls(lambda: ops.restore_label(blended, values, RAW, FRAME, whole[0], whole[1], 1), a.warmup, a.repeats)
    out['restore_centre_s'] = time_calls(lambda: ops.restore_label(prob[:SLICES], values, RAW, FRAME, centre[0], centre[1], 1), a.warmup,
                                         a.repeats)
    out['blend_bytes'] = int(prob.numel() * 4 * 4 // 5 + blended.numel() * 4)          # the organ channels read once, the map written
    raw = nn.host_to_device(np.round(700 * (Hh.smooth_field(rng, SLICES, RAW[0], RAW[1])[..., 0] + 1.5)), dev, np.float32)
    tiles_in = torch.zeros((T * SLICES, INPUT, INPUT, 1), device=dev)

    def load_tiles():
        for tr, r in enumerate(rows):
            for tc, c in enumerate(cols):
                t = tr * len(cols) + tc
                ops.preprocess_images(raw, tiles_in[t * SLICES:(t + 1) * SLICES], FRAME, r, c, 0)
    out['preprocess_tiles_s'] = time_calls(load_tiles, a.warmup, a.repeats)
    out['preprocess_centre_s'] = time_calls(lambda: ops.preprocess_images(raw, tiles_in[:SLICES], FRAME, centre[0], centre[1], 0), a.warmup,
                                            a.repeats)
    if not a.no_model:
        from multimodal_segmentation_amd.configuration import dafnet_config_chaos
        from multimodal_segmentation_amd.models.dafnet import DAFNet
        from multimodal_segmentation_amd.volume_predictor import VolumePredictor
        conf = Hh.make_conf(dafnet_config_chaos, INPUT, batch_size=a.batch)
        model = DAFNet(conf)
        model.build()
        predictor = VolumePredictor(model, conf)
        images = [tiles_in, tiles_in]
        few = max(1, a.repeats // 4)
        out['model_tiles_s'] = time_calls(lambda: predictor.predict_volume(0, 'simple', images), 1, few)
        out['model_centre_s'] = time_calls(lambda: predictor.predict_volume(0, 'simple', [x[:SLICES] for x in images]), 1, few)
        out['model_batch'], out['model_repeats'] = a.batch, few
    return out


def ms(t):
    return '%.3f ms (%.3f .. %.3f)' % (1e3 * t[0], 1e3 * t[1], 1e3 * t[2])


def write_up(path, a, r, device):
    lines = ['# Whole-slice prediction of one volume: tiles in, ops.blend_tiles, the way back', '',
             '%d slices, raw %d x %d, resampled frame %d x %d, input %d x %d: %d x %d tiles at origins %s (rows) and %s (columns), overlap %d.'
             % (SLICES, RAW[0], RAW[1], FRAME[0], FRAME[1], INPUT, INPUT, r['tiles'][0], r['tiles'][1], [t[0] for t in r['rows']],
                [t[0] for t in r['cols']], INPUT // 2),
             'Soft-max containers with %d channels, four organs.  Event time, %d warm-up calls, median of %d calls (min .. max in brackets).'
             % (C, a.warmup, a.repeats), '%s.  Command: `python tools/volume_tiles_bench.py`' % device, '',
             '| step | with tiles | centre window only |', '|---|---|---|',
             '| preprocess_images (min-max + image, per tile) | %s, %d calls | %s, 1 call |'
             % (ms(r['preprocess_tiles_s']), r['tiles'][0] * r['tiles'][1], ms(r['preprocess_centre_s'])),
             '| blend_tiles | %s | |' % ms(r['blend_tiles_s']),
             '| restore_label, order 1 | %s (the blended map, the whole frame) | %s (one container) |'
             % (ms(r['restore_blended_s']), ms(r['restore_centre_s']))]
    if 'model_tiles_s' in r:
        lines.append('| DAFNet.predict_mask, batches of %d, median of %d | %s | %s |'
                     % (r['model_batch'], r['model_repeats'], ms(r['model_tiles_s']), ms(r['model_centre_s'])))
    else:
        lines.append('| the model\'s forward | NOT MEASURED (--no-model) | |')
    gbs = r['blend_bytes'] / r['blend_tiles_s'][0] / 1e9
    lines += ['', 'blend_tiles moves %.1f MB (the organ channels of every tile once, the map once): %.0f GB/s.  The %d preprocess_images '
              'calls repeat the min-max pass over the whole resampled frame: %.2f times the time of the one call of the centre window.'
              % (r['blend_bytes'] / 1e6, gbs, r['tiles'][0] * r['tiles'][1], r['preprocess_tiles_s'][0] / r['preprocess_centre_s'][0])]
    if 'model_tiles_s' in r:
        lines += ['The forward passes over the tiles take %.1f times those over the centre windows; blend_tiles is %.2f %% of them.'
                  % (r['model_tiles_s'][0] / r['model_centre_s'][0], 100 * r['blend_tiles_s'][0] / r['model_tiles_s'][0])]
    with open(path, 'w') as f:
        f.write('\n'.join(lines) + '\n')


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('--repeats', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--batch', type=int, default=12)
    ap.add_argument('--no-model', dest='no_model', action='store_true')
    ap.add_argument('--out', default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'profiles',
                                                  'volume_tiles_bench.md'))
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit('volume_tiles_bench needs a GPU: a time measured without one says nothing')
    if a.repeats < 10:
        raise SystemExit('at least 10 repeats')
    nn.set_default_device('cuda:0')
    result = measure(a)
    device = '%s (%s)' % (torch.cuda.get_device_name(0), str(getattr(torch.cuda.get_device_properties(0), 'gcnArchName', '?')).split(':')[0])
    print(json.dumps(dict(device=device, result=result)))
    write_up(a.out, a, result, device)


if __name__ == '__main__':
    main()
