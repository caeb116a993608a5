#!/usr/bin/env python
"""Timings of the boundary loss (csrc/boundary.hip; conf.w_boundary, build-defined).

  python tools/boundary_bench.py ops [--markdown] [--no-host]
      device time of ops.boundary_map, of the term + gradient + combine (ops.boundary_term, boundary_grad_add, boundary_combine) and of
      ops.seg_loss alone (Dice + 0.01 BCE with its gradient), at the CHAOS geometry (num_masks 4, C = 5) for batch 8 at 256 x 256 and at
      512 x 512, on masks of random ellipses; beside the scipy restatement of the map on the host (one distance_transform_edt pair per
      sample and channel).  Device events around 50 calls after 3 warm-up calls: the times include what the host adds between launches.
      Algorithmic bytes per pixel of one sample: the row pass reads the C target floats and writes nm words, the column pass reads nm
      words and writes nm floats: 4 C + 12 nm (68 B at C = 5, nm = 4).
  python tools/boundary_bench.py step [--steps K --warmup W --rounds R]
      one supervised DAFNet trainer step (batch 8, 256 x 256) with w_boundary 0 and 1, eager and with hip_graphs: R rounds alternating
      the four models, K steps per block timed with a host clock around a device synchronise; the median per-step time of each.

One JSON line per measurement.  For the kernels alone: `rocprofv3 --kernel-trace --stats -- python tools/boundary_bench.py ops --no-host`.
"""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import numpy as np
import torch

NM, C = 4, 5


def ellipse_target(rng, B, H, W):
    """NM disjoint random ellipses per slice + the residual channel -> [B,H,W,C] fp32 in {0, 1}"""
    yy, xx = np.mgrid[:H, :W]
    out = np.zeros((B, H, W, C), np.float32)
    for b in range(B):
        taken = np.zeros((H, W), bool)
        for k in range(NM):
            cy, cx = rng.uniform(0.2, 0.8) * H, rng.uniform(0.2, 0.8) * W
            ry, rx = rng.uniform(0.06, 0.18) * H, rng.uniform(0.06, 0.18) * W
            m = (((yy - cy) / ry) ** 2 + ((xx - cx) / rx) ** 2 <= 1.0) & ~taken
            taken |= m
            out[b, ..., k] = m
        out[b, ..., NM] = ~taken
    return out


def bench(fn, reps=50):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(reps):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / reps * 1e3      # us


def host_map(target):
    from scipy.ndimage import distance_transform_edt as edt
    t0 = time.perf_counter()
    B = target.shape[0]
    out = np.zeros(target.shape[:3] + (NM,), np.float32)
    for b in range(B):
        for k in range(NM):
            pos = target[b, ..., k] > 0.5
            if pos.any() and not pos.all():
                out[b, ..., k] = edt(~pos) * ~pos - (edt(pos) - 1) * pos
    return time.perf_counter() - t0, out


def cmd_ops(a):
    from multimodal_segmentation_amd import ops
    lines = []
    for B, H in ((8, 256), (8, 512)):
        rng = np.random.RandomState(3)
        host = ellipse_target(rng, B, H, H)
        target = torch.as_tensor(host).cuda()
        pred = torch.softmax(torch.randn(B, H, H, C, device='cuda'), -1).contiguous()
        w = torch.ones(1, device='cuda')
        phi = ops.boundary_map(target, NM)
        t_map = bench(lambda: ops.boundary_map(target, NM))

        def term():
            loss, dpred = torch.zeros(1, device='cuda'), state['dpred']
            lb = ops.boundary_term(pred, phi, NM)
            ops.boundary_grad_add(phi, dpred, NM, 1.0, w)
            ops.boundary_combine(loss, lb, w)
        state = {'dpred': torch.zeros_like(pred)}
        t_term = bench(term)
        t_seg = bench(lambda: ops.seg_loss(pred, target, NM, 0.01, 1.0))
        t_host, ref = (float('nan'), None) if a.no_host else host_map(host)
        if ref is not None:
            assert float((phi.cpu() - torch.as_tensor(ref)).abs().max()) <= 2.0 ** -23 * max(1.0, float(np.abs(ref).max())), 'map differs from scipy'
        px = B * H * H
        lines.append(dict(B=B, H=H, C=C, num_masks=NM, boundary_map_us=round(t_map, 2), term_grad_combine_us=round(t_term, 2),
                          seg_loss_us=round(t_seg, 2), map_over_seg_loss=round(t_map / t_seg, 2),
                          map_bytes_per_pixel=4 * C + 12 * NM, map_GBs=round(px * (4 * C + 12 * NM) / t_map / 1e3, 1),
                          max_abs_phi=round(float(phi.abs().max()), 2), host_scipy_ms=round(t_host * 1e3, 1)))
        print(json.dumps(lines[-1]), flush=True)
    if a.markdown:
        keys = ('B', 'H', 'boundary_map_us', 'term_grad_combine_us', 'seg_loss_us', 'map_over_seg_loss', 'map_GBs', 'host_scipy_ms')
        print('| ' + ' | '.join(keys) + ' |')
        print('|' + '---|' * len(keys))
        for ln in lines:
            print('| ' + ' | '.join(str(ln[k]) for k in keys) + ' |')


def build_step(w_boundary, hip_graphs, ref=None, B=8, S=256):
    from multimodal_segmentation_amd import nn
    from multimodal_segmentation_amd.configuration import dafnet_config_chaos
    from multimodal_segmentation_amd.models.dafnet import DAFNet
    from multimodal_segmentation_amd.utils.config import EasyDict
    nn.set_default_device('cuda:0')
    conf = EasyDict(dafnet_config_chaos.get())
    shp = (S, S, 1)
    conf.input_shape = shp
    conf.anatomy_encoder['input_shape'] = shp
    conf.anatomy_encoder['output_shape'] = (S, S, conf.anatomy_encoder['out_channels'])
    conf.d_mask_params['input_shape'] = (S, S, conf.num_masks)
    conf.d_image_params['input_shape'] = shp
    conf.n_pairs, conf.batch_size = 1, B
    conf.hip_graphs, conf.w_boundary = hip_graphs, w_boundary
    conf.folder = tempfile.mkdtemp(prefix='boundary_bench_')
    model = DAFNet(conf)
    model.build()
    ms = model._generator_models()
    if ref is not None:
        for m, w in zip(ms, ref):
            m.set_weights(w)
    rng = np.random.RandomState(5)
    x1, x2 = [torch.as_tensor(np.tanh(rng.standard_normal((B, S, S, 1))).astype(np.float32)).cuda() for _ in range(2)]
    m1, m2 = [torch.as_tensor(ellipse_target(rng, B, S, S)).cuda() for _ in range(2)]
    z1, z2 = [torch.as_tensor(rng.standard_normal((B, 8)).astype(np.float32)).cuda() for _ in range(2)]
    ones, zeros = np.ones((B, 1), np.float32), np.zeros(B, np.float32)
    tg = [m1, m2, m1, m2] + [ones] * 4 + [x1, x2, x1, x2] + [ones] * 4 + [zeros] * 2 + [z1, z2]
    tr = model.supervised_trainer

    def step():
        return tr.fit([x1, x2, z1, z2], tg)
    return model, step, [m.get_weights() for m in ms]


def cmd_step(a):
    variants = [(0.0, False), (1.0, False), (0.0, True), (1.0, True)]
    steps, ref = {}, None
    for v in variants:
        model, step, w = build_step(v[0], v[1], ref)
        ref = ref or w
        for _ in range(a.warmup):
            step()
        torch.cuda.synchronize()
        steps[v] = (model, step)
    times = {v: [] for v in variants}
    for _ in range(a.rounds):
        for v in variants:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(a.steps):
                h = steps[v][1]()
            torch.cuda.synchronize()
            times[v].append((time.perf_counter() - t0) / a.steps * 1e3)
    out = {}
    for (wb, g), ts in times.items():
        out['%s_w%d_ms' % ('graph' if g else 'eager', int(wb))] = round(statistics.median(ts), 3)
        out['%s_w%d_spread_ms' % ('graph' if g else 'eager', int(wb))] = round(max(ts) - min(ts), 3)
    out['eager_overhead_ms'] = round(out['eager_w1_ms'] - out['eager_w0_ms'], 3)
    out['graph_overhead_ms'] = round(out['graph_w1_ms'] - out['graph_w0_ms'], 3)
    out.update(batch=8, size=256, steps=a.steps, rounds=a.rounds, warmup=a.warmup)
    print(json.dumps(out), flush=True)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    sub = ap.add_subparsers(dest='cmd', required=True)
    p = sub.add_parser('ops')
    p.add_argument('--markdown', action='store_true')
    p.add_argument('--no-host', dest='no_host', action='store_true')
    p = sub.add_parser('step')
    p.add_argument('--steps', type=int, default=10)
    p.add_argument('--warmup', type=int, default=4)
    p.add_argument('--rounds', type=int, default=5)
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit('boundary_bench: needs a GPU (the kernels have no CPU path)')
    (cmd_ops if a.cmd == 'ops' else cmd_step)(a)


if __name__ == '__main__':
    main()
