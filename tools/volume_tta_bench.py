#!/usr/bin/env python
"""What test-time augmentation costs for one CHAOS-sized volume: 36 slices in containers of 192 x 192, soft-max maps with C = 5
channels (four organs and the background: the scalar path of the merge) and with C = K = 4 (its 16-byte path), under the view lists
`flips` (4 views), `d4` (8) and `id,rot10,rot-10` (3).

  views in  event time of the ops.augment_gather call that makes the V x 36 views of one modality's containers
  merge     event time of ops.merge_views (csrc/postprocess.hip) on the V x 36 maps, with the bytes it moves (the organ channels of
            every view once, the merged map once) and GB/s
  restore   event time of ops.restore_label of the merged map onto the raw grid (the same with and without the option)
  model     event time of DAFNet.predict_mask(0, 'simple') over the V x 36 views in batches of `--batch`, beside the 36 slices; the
            merge as a share of the former.  Skipped with --no-model
Each after `--warmup` calls, median of `--repeats`.  Prints one JSON line and writes the write-up to `--out`.

    python tools/volume_tta_bench.py [--repeats 20] [--warmup 3] [--batch 12] [--no-model] [--out profiles/volume_tta_bench.md]
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from multimodal_segmentation_amd import nn, ops
from multimodal_segmentation_amd.loaders.volume_folder import crop_pad_map
from multimodal_segmentation_amd.volume_predictor import check_tta, views_in
from tests import helpers as Hh

VALUES = [63, 126, 189, 252]
SLICES, RAW, FRAME, INPUT, K = 36, (256, 256), (256, 256), 192, 4
VIEW_LISTS = ('flips', 'd4', 'id,rot10,rot-10')
CHANNELS = (5, 4)


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


def softmax_fields(rng, n, C):
    """[n,INPUT,INPUT,C] fp32: a soft-max over smooth random fields, 12 distinct slices cycled"""
    f = 4.0 * np.concatenate([Hh.smooth_field(rng, 12, INPUT, INPUT, sigma=8.0) for _ in range(C)], axis=-1).astype(np.float64)
    e = np.exp(f - f.max(-1, keepdims=True))
    return (e / e.sum(-1, keepdims=True)).astype(np.float32)[np.arange(n) % 12]


def measure(a):
    dev = 'cuda:0'
    rng = np.random.RandomState(3)
    centre = crop_pad_map(FRAME[0], INPUT), crop_pad_map(FRAME[1], INPUT)
    values = nn.host_to_device(np.asarray(VALUES), dev, np.int32)
    images = nn.host_to_device(Hh.smooth_field(rng, SLICES, INPUT, INPUT), dev, np.float32)
    maps = {C: softmax_fields(rng, 12, C) for C in CHANNELS}
    out = dict(views={})
    for text in VIEW_LISTS:
        views = check_tta(text, (INPUT, INPUT, 1))
        V = len(views.tokens)
        back = nn.host_to_device(views.back, dev, np.float64)
        r = dict(V=V, views_in_s=time_calls(lambda: views_in([images], views), a.warmup, a.repeats))
        for C in CHANNELS:
            prob = nn.host_to_device(maps[C][np.arange(V * SLICES) % 12], dev, np.float32)
            merged = ops.merge_views(prob, back, SLICES, K)
            r['merge_c%d_s' % C] = time_calls(lambda: ops.merge_views(prob, back, SLICES, K), a.warmup, a.repeats)
            r['merge_c%d_bytes' % C] = int(prob.numel() * 4 * K // C + merged.numel() * 4)
            if C == 5:
                r['restore_s'] = time_calls(lambda: ops.restore_label(merged, values, RAW, FRAME, centre[0], centre[1], 1), a.warmup,
                                            a.repeats)
            del prob, merged
        out['views'][text] = r
    if not a.no_model:
        from multimodal_segmentation_amd.configuration import dafnet_config_chaos
        from multimodal_segmentation_amd.models.dafnet import DAFNet
        from multimodal_segmentation_amd.volume_predictor import VolumePredictor
        conf = Hh.make_conf(dafnet_config_chaos, INPUT, batch_size=a.batch)
        model = DAFNet(conf)
        model.build()
        predictor = VolumePredictor(model, conf)
        few = max(1, a.repeats // 4)
        out['model_once_s'] = time_calls(lambda: predictor.predict_volume(0, 'simple', [images, images]), 1, few)
        for text in VIEW_LISTS:
            turned = views_in([images], check_tta(text, (INPUT, INPUT, 1)))[0]
            out['views'][text]['model_s'] = time_calls(lambda: predictor.predict_volume(0, 'simple', [turned, turned]), 1, few)
            del turned
        out['model_batch'], out['model_repeats'] = a.batch, few
    return out


def ms(t):
    return '%.3f ms (%.3f .. %.3f)' % (1e3 * t[0], 1e3 * t[1], 1e3 * t[2])


def write_up(path, a, r, device):
    lines = ['# Test-time augmentation of one volume: views in, ops.merge_views, the way back', '',
             '%d slices in containers of %d x %d, raw %d x %d, four organs.  Soft-max maps with C = 5 channels (the scalar path of the merge: '
             'a thread per output float) and C = K = 4 (a thread per pixel, 16-byte loads and stores).' % (SLICES, INPUT, INPUT, RAW[0], RAW[1]),
             'Event time, %d warm-up calls, median of %d calls (min .. max in brackets).' % (a.warmup, a.repeats),
             '%s.  Command: `python tools/volume_tta_bench.py`' % device, '',
             '| views | V | views in (augment_gather, one modality) | merge_views, C = 5 | merge_views, C = K = 4 | restore_label, order 1 |',
             '|---|---|---|---|---|---|']
    for text in VIEW_LISTS:
        v = r['views'][text]
        cells = ['%s, %.1f MB, %.0f GB/s' % (ms(v['merge_c%d_s' % C]), v['merge_c%d_bytes' % C] / 1e6,
                                            v['merge_c%d_bytes' % C] / v['merge_c%d_s' % C][0] / 1e9) for C in CHANNELS]
        lines.append('| `%s` | %d | %s | %s | %s | %s |' % (text, v['V'], ms(v['views_in_s']), cells[0], cells[1], ms(v['restore_s'])))
    lines += ['', 'Bytes: the K organ channels of every view once and the merged map once.  `d4` holds the four transposing views, whose '
              'reads have a stride of one container row between neighbouring lanes; the rotations read four taps per view where they cover.  '
              'The repeats find the maps where the call before left them: a rate above what HBM delivers is that of the last-level cache, '
              'which holds these sizes, as it holds maps that the network has just written.']
    if 'model_once_s' in r:
        lines += ['', 'DAFNet.predict_mask(0, \'simple\'), batches of %d, median of %d: %s over the %d slices without the option.'
                  % (r['model_batch'], r['model_repeats'], ms(r['model_once_s']), SLICES), '',
                  '| views | forward over V x %d slices | times the forward without | merge_views (C = 5) as a share of it |' % SLICES,
                  '|---|---|---|---|']
        for text in VIEW_LISTS:
            v = r['views'][text]
            lines.append('| `%s` | %s | %.2f | %.3f %% |' % (text, ms(v['model_s']), v['model_s'][0] / r['model_once_s'][0],
                                                              100 * v['merge_c5_s'][0] / v['model_s'][0]))
    else:
        lines += ['', 'The model\'s forward: NOT MEASURED (--no-model).']
    with open(path, 'w') as f:
        f.write('\n'.join(lines) + '\n')


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('--repeats', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--batch', type=int, default=12)
    ap.add_argument('--no-model', dest='no_model', action='store_true')
    ap.add_argument('--out', default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'profiles',
                                                  'volume_tta_bench.md'))
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit('volume_tta_bench needs a GPU: a time measured without one says nothing')
    if a.repeats < 10:
        raise SystemExit('at least 10 repeats')
    nn.set_default_device('cuda:0')
    result = measure(a)
    device = '%s (%s)' % (torch.cuda.get_device_name(0), str(getattr(torch.cuda.get_device_properties(0), 'gcnArchName', '?')).split(':')[0])
    print(json.dumps(dict(device=device, result=result)))
    write_up(a.out, a, result, device)


if __name__ == '__main__':
    main()
