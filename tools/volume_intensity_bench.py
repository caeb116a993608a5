#!/usr/bin/env python
"""Device time of the percentile / landmark intensity normalisation (csrc/preprocess.hip: mmseg_preprocess_quantiles, four radix
passes that each recompute the resampling, and mmseg_preprocess_image_map) beside the min / max path it replaces (mmseg_preprocess_minmax
+ mmseg_preprocess_image) on the same upload, and beside the numpy restatement (tests/volume_intensity_ref.py) on the host it runs on.

Per geometry (S x H x W raw slices resampled by a factor, cropped to 192 x 192), scope (slice / volume) and K (2: window, 11:
landmarks): device events around the Python ops, warmed up, median of `--repeats` windows of `--calls` calls each;
  select       ops.preprocess_quantiles (memset + 4 x (histogram + pick))
  map          ops.preprocess_images(knots=...)
  minmax+image ops.preprocess_images() -- the parent's two launches
  raw bytes per pass = 4 * S * H * W, and the rate select achieves: 4 passes x raw bytes / select time (a whole-op rate over the
  least traffic the algorithm needs, not a kernel's share of peak), against 6.3 TB/s achievable HBM bandwidth
With --host the restatement's sort and map over the same resampled frames are timed too, and the knots must equal its knots within
2^-20 * max|raw| or the tool fails.  Prints one JSON line per case.

    python tools/volume_intensity_bench.py [--repeats 5] [--calls 20] [--host]
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
from multimodal_segmentation_amd.loaders.volume_folder import LANDMARK_PERCENTILES, WINDOW_PERCENTILES, crop_pad_map, quantile_ranks
from tests import volume_intensity_ref as I

GEOMETRIES = [(30, 256, 256, 1.0), (90, 320, 320, 1.3)]
OUT = (192, 192)
HBM_ACHIEVABLE = 6.3e12          # bytes / s


def raw_volume(S, H, W, seed):
    """MR-like: smooth tissue, 30 % air, int16 range"""
    rng = np.random.RandomState(seed)
    coarse = rng.rand(S, H // 16 + 2, W // 16 + 2).astype(np.float32)
    image = np.kron(coarse, np.ones((1, 16, 16), np.float32))[:, :H, :W] * 1200.0 + rng.rand(S, H, W).astype(np.float32) * 100.0
    image[:, :int(0.3 * H)] = 0.0
    return np.round(image).astype(np.float32)


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


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--calls', type=int, default=20)
    ap.add_argument('--host', action='store_true', help='also time the numpy restatement (slow at the larger geometry)')
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit('volume_intensity_bench needs a GPU: a time measured without one says nothing')
    nn.set_default_device('cuda:0')
    for S, H, W, factor in GEOMETRIES:
        RH, RW = int(np.round(H * factor)), int(np.round(W * factor))
        rows, cols = crop_pad_map(RH, OUT[0]), crop_pad_map(RW, OUT[1])
        image = raw_volume(S, H, W, S)
        x = nn.host_to_device(image, 'cuda:0', np.float32)
        out = torch.zeros((S, OUT[0], OUT[1], 1), device='cuda:0')
        t_plain = device_ms(lambda: ops.preprocess_images(x, out, (RH, RW), rows, cols, 0), a.calls, a.repeats)
        fr = I.frames(image, RH, RW) if a.host else None
        for per_volume in (False, True):
            for q in (WINDOW_PERCENTILES, LANDMARK_PERCENTILES):
                K = len(q)
                ranks = quantile_ranks((S if per_volume else 1) * RH * RW, q)
                y = nn.host_to_device(np.linspace(-1.0, 1.0, K), 'cuda:0', np.float32)
                knots = ops.preprocess_quantiles(x, (RH, RW), ranks, per_volume)
                t_select = device_ms(lambda: ops.preprocess_quantiles(x, (RH, RW), ranks, per_volume), a.calls, a.repeats)
                t_map = device_ms(lambda: ops.preprocess_images(x, out, (RH, RW), rows, cols, 0, knots=(knots, y)), a.calls, a.repeats)
                raw_bytes = 4 * S * H * W
                rate = 4 * raw_bytes / (t_select[0] * 1e-3)
                rec = dict(raw=[S, H, W], resampled=[RH, RW], scope='volume' if per_volume else 'slice', K=K,
                           select_ms=round(t_select[0], 4), select_ms_range=[round(t_select[1], 4), round(t_select[2], 4)],
                           map_ms=round(t_map[0], 4), minmax_image_ms=round(t_plain[0], 4),
                           minmax_image_ms_range=[round(t_plain[1], 4), round(t_plain[2], 4)], raw_bytes_per_pass=raw_bytes,
                           select_gb_per_s=round(rate / 1e9, 1), share_of_achievable_hbm=round(rate / HBM_ACHIEVABLE, 4),
                           device=torch.cuda.get_device_name(0))
                if a.host:
                    t0 = time.perf_counter()
                    mapped, want = I.normalise(fr, ranks, np.linspace(-1.0, 1.0, K), per_volume)
                    rec['host_restatement_s'] = round(time.perf_counter() - t0, 3)          # sort + map; the resampling is not counted
                    err = float(np.abs(knots.cpu().numpy().astype(np.float64) - want).max())
                    rec['knot_max_abs_error'] = err
                    if err > 2.0 ** -20 * float(np.abs(image).max()):
                        print(json.dumps(rec))
                        raise SystemExit('device and host knots disagree')
                print(json.dumps(rec), flush=True)


if __name__ == '__main__':
    main()
