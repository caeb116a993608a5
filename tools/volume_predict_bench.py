#!/usr/bin/env python
"""Time of the way back to the raw grid for a CHAOS-sized folder: ops.restore_label + ops.label_overlap on the device
(csrc/postprocess.hip) beside the fp64 scipy restatement (tests/volume_predict_ref.py) on the host it runs on.

Workload: `--volumes` x 2 modalities, `--slices` slices each, raw slices of 256 / 288 / 320 pixels a side (the CHAOS MR sizes; all
multiples of 4, so a lane stores a packed dword) at 1.2..2.4 mm, brought back from 192 x 192 x 5 softmax containers at 1.89 mm; and the
same with every extent reduced by one pixel (per-byte stores).  Probabilities are a softmax over smooth random fields, the truth is
the restatement's own label of another draw.
  device   event time of one pass over all (volume, modality) pairs, after `--warmup` passes, median of `--repeats`; the bytes the
           algorithm needs (the kept window of the container once, 1 byte per raw pixel out) over that time
  host     the restatement over the first `--host_pairs` pairs, scaled to all of them; its labels must equal the device's on every
           decidable pixel, its counts the device's exactly, or the tool fails
Prints one JSON line and writes the write-up to `--out`.

    python tools/volume_predict_bench.py [--volumes 20] [--slices 30] [--repeats 20] [--warmup 3] [--host_pairs 4]
                                         [--out profiles/volume_predict_bench.md]
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
from multimodal_segmentation_amd.loaders.volume_folder import crop_pad_map, resampled_size
from tests import helpers as Hh
from tests import volume_predict_ref as P

TARGET, OUT, C, VALUES = 1.89, 192, 5, [63, 126, 189, 252]
HBM_BYTES_PER_S = 8e12


def make_pairs(rng, n, slices, shrink):
    """per (volume, modality): raw size, geometry, a container of probabilities and a truth volume on the device"""
    base = np.stack([Hh.smooth_field(rng, 8, OUT, OUT, sigma=8.0)[..., 0] for _ in range(C)], axis=-1).astype(np.float64) * 4.0
    e = np.exp(base - base.max(-1, keepdims=True))
    base = (e / e.sum(-1, keepdims=True)).astype(np.float32)
    pairs = []
    for i in range(n):
        H, W = [int(rng.choice([256, 288, 320])) - shrink for _ in range(2)]
        res = rng.uniform(1.2, 2.4, size=2)
        RH, RW = resampled_size(H, res[0], TARGET), resampled_size(W, res[1], TARGET)
        prob = base[(np.arange(slices) + i) % base.shape[0]]
        if i % 2:
            prob = prob[:, ::-1, :, :]
        truth = np.ascontiguousarray(np.asarray([0] + VALUES, np.uint8)[rng.randint(0, 5, size=(slices, H // 16 + 1, W // 16 + 1))]
                                     .repeat(16, 1).repeat(16, 2)[:, :H, :W])
        pairs.append(dict(raw=(H, W), resampled=(RH, RW), rows=crop_pad_map(RH, OUT), cols=crop_pad_map(RW, OUT),
                          prob_host=np.ascontiguousarray(prob), truth_host=truth))
    return pairs


def needed_bytes(pairs, slices):
    window = sum(p['rows'][1] * p['cols'][1] * C * 4 for p in pairs) * slices
    raw = sum(p['raw'][0] * p['raw'][1] for p in pairs) * slices
    return window, raw


def time_passes(fn, warmup, repeats):
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


def measure(pairs, slices, a, order):
    values = nn.host_to_device(np.asarray(VALUES), 'cuda:0', np.int32)
    for p in pairs:
        p['prob'] = nn.host_to_device(p['prob_host'], 'cuda:0', np.float32)
        p['truth'] = nn.host_to_device(p['truth_host'], 'cuda:0', np.uint8)
    preds = [None] * len(pairs)

    def restore():
        for i, p in enumerate(pairs):
            preds[i] = ops.restore_label(p['prob'], values, p['raw'], p['resampled'], p['rows'], p['cols'], order)

    def overlap():
        return [ops.label_overlap(preds[i], p['truth'], values) for i, p in enumerate(pairs)]
    t_restore = time_passes(restore, a.warmup, a.repeats)
    t_overlap = time_passes(overlap, a.warmup, a.repeats)
    counts = [c.cpu().numpy() for c in overlap()]
    # the host restatement on the first pairs, and agreement in the same run
    t0 = time.perf_counter()
    host = [P.restore(p['prob_host'], VALUES, p['raw'], p['resampled'], p['rows'], p['cols'], order) for p in pairs[:a.host_pairs]]
    t_host_restore = time.perf_counter() - t0
    t0 = time.perf_counter()
    host_counts = [P.overlap_counts(h[0], p['truth_host'], VALUES) for h, p in zip(host, pairs)]
    t_host_overlap = time.perf_counter() - t0
    differing = undecidable = compared = 0
    for i, (want, und) in enumerate(host):
        got = preds[i].cpu().numpy()
        differing += int(np.count_nonzero((got != want) & ~und))
        undecidable += int(np.count_nonzero(und))
        compared += want.size
        flips = int(np.count_nonzero(got != want))
        if np.abs(counts[i].astype(np.int64) - host_counts[i]).max() > flips:
            raise SystemExit('device and host counts disagree')
    if differing:
        raise SystemExit('device and host labels disagree on %d decidable pixels' % differing)
    window, raw = needed_bytes(pairs, slices)
    scale = len(pairs) / float(a.host_pairs)
    return dict(order=order, restore_s=t_restore[0], restore_min_max_s=t_restore[1:], overlap_s=t_overlap[0],
                overlap_min_max_s=t_overlap[1:], restore_bytes=window + raw, overlap_bytes=2 * raw,
                restore_bytes_per_s=(window + raw) / t_restore[0], overlap_bytes_per_s=2 * raw / t_overlap[0],
                host_restore_s=t_host_restore * scale, host_overlap_s=t_host_overlap * scale, host_pairs_timed=a.host_pairs,
                compared_pixels=compared, undecidable_pixels=undecidable, differing_pixels=differing,
                foreground_share=float(np.mean([np.count_nonzero(h[0]) / float(h[0].size) for h in host])))


def write_up(path, a, results, device, launches):
    lines = ['# Restoring predicted labels to the raw grid: a CHAOS-sized folder', '',
             'Workload: %d volumes x 2 modalities x %d slices; raw slices of 256 / 288 / 320 pixels a side (the CHAOS MR sizes) at' % (a.volumes, a.slices),
             '1.2..2.4 mm, brought back from 192 x 192 x 5 softmax containers at 1.89 mm with `ops.restore_label`, then scored against a',
             'label volume with `ops.label_overlap` (4 organs).  "odd" rows: every raw extent one pixel smaller, so `W % 4 != 0` and the',
             'kernel stores single bytes.  One pass = %d launches of each kernel (one per volume and modality).  Device: event time,' % launches,
             '%d warm-up passes, median of %d passes (min .. max in brackets).  Host: the fp64 scipy restatement' % (a.warmup, a.repeats),
             '(`tests/volume_predict_ref.py`) on the same machine, timed on %d of the %d pairs and scaled.  %s.' % (a.host_pairs, launches, device), '',
             'Command: `python tools/volume_predict_bench.py`', '',
             '| raw widths | order | restore_label | needed bytes | achieved | of 8 TB/s | label_overlap | achieved | host restore | host counts |',
             '|---|---|---|---|---|---|---|---|---|---|']
    for name, r in results:
        lines.append('| %s | %d | %.3f ms (%.3f .. %.3f) | %.1f MB | %.2f TB/s | %.1f %% | %.3f ms (%.3f .. %.3f) | %.2f TB/s | %.1f s | %.2f s |'
                     % (name, r['order'], 1e3 * r['restore_s'], 1e3 * r['restore_min_max_s'][0], 1e3 * r['restore_min_max_s'][1],
                        r['restore_bytes'] / 1e6, r['restore_bytes_per_s'] / 1e12, 100 * r['restore_bytes_per_s'] / HBM_BYTES_PER_S,
                        1e3 * r['overlap_s'], 1e3 * r['overlap_min_max_s'][0], 1e3 * r['overlap_min_max_s'][1],
                        r['overlap_bytes_per_s'] / 1e12, r['host_restore_s'], r['host_overlap_s']))
    r = results[0][1]
    lines += ['', 'Needed bytes = the kept window of every container once (fp32, 5 channels) plus 1 byte per raw pixel; the bilinear taps of',
              'neighbouring raw pixels overlap and are served by the caches.  Per launch the kernels move %.1f MB and %.1f MB: at that size a'
              % (r['restore_bytes'] / launches / 1e6, r['overlap_bytes'] / launches / 1e6),
              'launch is a large part of the time (%.1f us and %.1f us per launch in the first row), so the achieved rate says how far a'
              % (1e6 * r['restore_s'] / launches, 1e6 * r['overlap_s'] / launches),
              'per-volume call is from the HBM bound, not how fast the kernel streams.  No target was set for this path.', '',
              'Agreement in the same run (the pairs the host timed): %s.'
              % '; '.join('%s order %d: %d differing of %d compared pixels, %d undecidable left out, foreground %.0f %%'
                          % (n, x['order'], x['differing_pixels'], x['compared_pixels'] - x['undecidable_pixels'], x['undecidable_pixels'],
                             100 * x['foreground_share']) for n, x in results), '']
    with open(path, 'w') as f:
        f.write('\n'.join(lines))


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('--volumes', type=int, default=20)
    ap.add_argument('--slices', type=int, default=30)
    ap.add_argument('--repeats', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--host_pairs', type=int, default=4)
    ap.add_argument('--out', default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'profiles',
                                                  'volume_predict_bench.md'))
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit('volume_predict_bench needs a GPU: a time measured without one says nothing')
    nn.set_default_device('cuda:0')
    a.host_pairs = max(1, min(a.host_pairs, 2 * a.volumes))
    results = []
    for name, shrink in (('256 / 288 / 320', 0), ('odd: 255 / 287 / 319', 1)):
        pairs = make_pairs(np.random.RandomState(7), 2 * a.volumes, a.slices, shrink)
        for order in ((1, 0) if shrink == 0 else (1,)):
            results.append((name, measure(pairs, a.slices, a, order)))
    device = torch.cuda.get_device_name(0)
    print(json.dumps(dict(volumes=a.volumes, slices=a.slices, device=device, results=[dict(r, widths=n) for n, r in results])))
    write_up(a.out, a, results, device, 2 * a.volumes)


if __name__ == '__main__':
    main()
