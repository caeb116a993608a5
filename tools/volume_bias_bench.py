#!/usr/bin/env python
"""Device time of the bias-field correction (csrc/biasfield.hip, ops.bias_correct) for one CHAOS-sized volume, with the split over its
stages, beside the rest of the loader's device work on the same upload (the min / max path of ops.preprocess_images) and -- with --host --
beside the numpy restatement (tests/volume_bias_ref.py) on the host it runs on.  No speed target is set: the numbers are recorded, not
asserted.

Device events around the Python ops, warmed up, median of `--repeats` windows of `--calls` calls each:
  correct      ops.bias_correct at the defaults (sigma 40 mm, 3 levels x 20 iterations, 3d): 5 + 3 * (4 + 20 * 8) + 1 launches
  stages       the stage entry points on the same volume at the radii of every level: Otsu (extremes, histogram, threshold), the 200-bin
               histogram (extremes + counts), the one-block sharpen, the three passes (3d), the two in-plane passes (2d; the difference is
               the pass along S), the update.  The residual and the final multiply are element-wise like the update and not split out.
  loader       ops.preprocess_images() on the same upload: what a (volume, modality) costs on the device without the correction
Also recorded, because the tests' bars refer to them (tests/test_volume_bias.py): the largest error of the sharpen table against numpy.fft
beside its derived bar, and the distance of the end-to-end fp32 output from the restatement in fp32 spacings, for the tests' cases.
Writes a markdown report (default profiles/volume_bias_bench.md) and prints one JSON line per record.

    python tools/volume_bias_bench.py [--repeats 5] [--calls 3] [--host] [--out profiles/volume_bias_bench.md]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

from multimodal_segmentation_amd import nn, ops
from multimodal_segmentation_amd.loaders.volume_folder import crop_pad_map
from tests import volume_bias_ref as B

SHAPE, SPACINGS = (30, 256, 256), (6.0, 1.6, 1.6)
OUT = (192, 192)


def device_ms(fn, calls, repeats):
    fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(repeats):
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        for _ in range(calls):
            fn()
        stop.record()
        stop.synchronize()
        times.append(start.elapsed_time(stop) / calls)
    return float(np.median(times)), float(min(times)), float(max(times))


def accuracy_records():
    """the figures the bars of tests/test_volume_bias.py refer to, for its own cases"""
    from tests import test_volume_bias as T
    recs = []
    for name in ('bimodal', 'one-bin'):
        h, vmin, vmax = T._sharpen_input(name)
        want = B.sharpen(h, vmin, vmax)
        bar, e_nd = B.sharpen_bar(h, vmin, vmax)
        got = ops.bias_sharpen(T._dev(h.astype(np.int32)), T._dev(np.array([vmin, vmax]))).cpu().numpy()
        err, stated = np.abs(got - want), np.isfinite(bar)
        recs.append(dict(kind='sharpen', case=name, largest_relative_error=float((err / np.abs(want))[stated].max()),
                         largest_error_over_bar=float((err / bar)[stated].max()), smallest_relative_bar=float((bar / np.abs(want))[stated].min()),
                         largest_relative_bar=float((bar / np.abs(want))[stated].max()), entries_bounded=int(stated.sum())))
    for name in sorted(T.E2E_CASES):
        case = T.E2E_CASES[name]
        x, _, _, res = T._e2e(name)
        out, f, info = ops.bias_correct(T._dev(x), case['spacings'], case['params'], field=True)
        recs.append(dict(kind='end-to-end', case=name, fp32_spacings_from_restatement=B.spacings_apart(out.cpu().numpy(), res['out']),
                         log_field_max_abs_error=float(np.abs(f.cpu().numpy() - res['field'])[res['mask']].max()),
                         smallest_bin_edge_distance=float(res['margin']), bar_in_the_test=T.E2E_BAR))
    x, field, tissue = B.phantom()
    for where, (out, f, m) in (('restatement', (lambda r: (r['out'], r['field'], r['mask']))(B.correct(x, T.SPACINGS))),
                               ('device', (lambda o: (o[0].cpu().numpy(), o[1].cpu().numpy(), B.otsu(x)[2] < x.astype(np.float64)))(
                                   ops.bias_correct(T._dev(x), T.SPACINGS, field=True)))):
        recs.append(dict(kind='corrects', where=where, cv_before=B.tissue_cv(x, tissue), cv_after=B.tissue_cv(out, tissue),
                         field_correlation=float(np.corrcoef(f[m], field[m])[0, 1])))
    return recs


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--calls', type=int, default=3)
    ap.add_argument('--host', action='store_true', help='also time the numpy restatement on the same volume (about a minute)')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'volume_bias_bench.md'))
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit('volume_bias_bench needs a GPU: a time measured without one says nothing')
    nn.set_default_device('cuda:0')
    dev = 'cuda:0'
    S, H, W = SHAPE
    image, _, _ = B.phantom(SHAPE, SPACINGS, seed=1)
    x = nn.host_to_device(image, dev, np.float32)
    params = ops.bias_params()
    levels = ops.bias_sigmas(SPACINGS, params)
    recs = []

    def note(rec):
        recs.append(rec)
        print(json.dumps(rec), flush=True)

    out = torch.empty_like(x)
    t = device_ms(lambda: ops.bias_correct(x, SPACINGS, params, out=out), a.calls, a.repeats)
    note(dict(kind='correct', shape=list(SHAPE), spacings=list(SPACINGS), params=params, radii=[[R for _, R in lv] for lv in levels],
              ms=round(t[0], 3), ms_range=[round(t[1], 3), round(t[2], 3)], device=torch.cuda.get_device_name(0)))
    container = torch.zeros((S, OUT[0], OUT[1], 1), device=dev)
    rows, cols = crop_pad_map(H, OUT[0]), crop_pad_map(W, OUT[1])
    t = device_ms(lambda: ops.preprocess_images(x, container, (H, W), rows, cols, 0), 20, a.repeats)
    note(dict(kind='loader', what='preprocess_images (min / max + image) on the same upload', ms=round(t[0], 4)))
    # the stages, on inputs of the iteration's kind
    x64 = image.astype(np.float64)
    m = x64 > B.otsu(image)[2]
    v = np.where(m, np.log(np.maximum(x64, 1e-30)), 0.0)
    dv, dm = torch.from_numpy(v).to(dev), torch.from_numpy(m.astype(np.uint8)).to(dev)
    hist, rng = ops.bias_histogram(dv, dm)
    f = torch.zeros_like(dv)
    stage = {}
    stage['otsu'] = device_ms(lambda: ops.bias_otsu(x), 20, a.repeats)[0]
    stage['histogram'] = device_ms(lambda: ops.bias_histogram(dv, dm), 20, a.repeats)[0]
    stage['sharpen'] = device_ms(lambda: ops.bias_sharpen(hist, rng), 20, a.repeats)[0]
    stage['update'] = device_ms(lambda: ops.bias_update(f, dv, dv), 20, a.repeats)[0]
    note(dict(kind='stages', ms={k: round(val, 4) for k, val in stage.items()}))
    for l, lv in enumerate(levels):
        t3 = device_ms(lambda: ops.bias_smooth(dv, lv), 10, a.repeats)[0]
        t2 = device_ms(lambda: ops.bias_smooth(dv, [(0.0, 0)] + list(lv[1:])), 10, a.repeats)[0]
        taps = sum(2 * R + 1 for _, R in lv)
        note(dict(kind='smooth', level=l, radii=[R for _, R in lv], ms_3d=round(t3, 4), ms_in_plane=round(t2, 4), ms_along_s=round(t3 - t2, 4),
                  g_taps_per_s=round(S * H * W * taps / (t3 * 1e-3) / 1e9, 1)))
    if a.host:
        t0 = time.perf_counter()
        res = B.correct(image, SPACINGS)
        host_s = time.perf_counter() - t0
        apart = B.spacings_apart(out.cpu().numpy(), res['out'])
        note(dict(kind='host', what='numpy restatement at the defaults on the same volume', s=round(host_s, 2),
                  device_output_fp32_spacings_from_it=apart, smallest_bin_edge_distance=float(res['margin'])))
    for rec in accuracy_records():
        note(rec)
    with open(a.out, 'w') as fh:
        fh.write('# Bias-field correction: device time and the figures behind the tests\' bars\n\n')
        fh.write('Written by `tools/volume_bias_bench.py%s`; see its docstring for what each record is.  One %s.  No speed target is set.\n\n'
                 % (' --host' if a.host else '', torch.cuda.get_device_name(0)))
        fh.write('```\n')
        for rec in recs:
            fh.write(json.dumps(rec) + '\n')
        fh.write('```\n')
    print('wrote', a.out)


if __name__ == '__main__':
    main()
