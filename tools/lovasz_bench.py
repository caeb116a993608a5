#!/usr/bin/env python
"""Timings of the Lovasz-Softmax loss (csrc/lovasz.hip; conf.w_lovasz, build-defined).

  python tools/lovasz_bench.py ops [--markdown] [--no-host]
      device time of ops.lovasz_map, of the term + gradient + combine (ops.lovasz_term, lovasz_grad_add, boundary_combine), of
      ops.seg_loss alone (Dice + 0.01 BCE with its gradient) and of ops.boundary_map, at the CHAOS geometry (num_masks 4, C = 5) for
      batch 8 at 256 x 256 and at 512 x 512, on a soft-max of Gaussian logits against masks of random ellipses; beside the numpy
      restatement of the map on the host (one stable argsort per sample and channel).  Device events around 50 calls after 3 warm-up
      calls: the times include what the host adds between launches.
      Algorithmic bytes per record (one pixel of one organ channel; 8-byte records): the build reads 8 C / nm bytes of pred and target
      and writes 8; each of the four passes reads 8 for the histogram (the first histogram is taken while building), reads 8 and
      writes 8 for the scatter; the count reads 8, the final pass reads 8 and writes 4: 8 C / nm + 8 + 3 * 24 + 16 + 20 = 126 B at
      C = 5, nm = 4 (histograms and tile counts are 0.5 B per record).
      For the time per kernel (per pass): `rocprofv3 --kernel-trace --stats -- python tools/lovasz_bench.py ops --no-host`.
  python tools/lovasz_bench.py step [--steps K --warmup W --rounds R --weights 0,1 --root TREE]
      one supervised DAFNet trainer step (batch 8, 256 x 256, fp32) with w_lovasz 0 and 1, eager and with hip_graphs: R rounds
      alternating the models, K steps per block timed with a host clock around a device synchronise; the median per-step time of each.
      --root TREE imports the package from another checkout (the parent commit, say, with --weights 0: a tree without the option
      ignores the key), so that its step can be timed by the same script in the same session.

One JSON line per measurement.
"""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for i, arg in enumerate(sys.argv):
    if arg == '--root' and i + 1 < len(sys.argv):
        ROOT = os.path.abspath(sys.argv[i + 1])
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


def host_map(pred, target):
    """the numpy restatement: e in fp32, a stable argsort, the closed form of lovasz_grad in fp64; 'present' classes"""
    t0 = time.perf_counter()
    B = pred.shape[0]
    p = pred.reshape(B, -1, C)[..., :NM]
    y = target.reshape(B, -1, C)[..., :NM] > 0.5
    e = np.abs(y.astype(np.float32) - p)
    P = p.shape[1]
    out = np.zeros((B, P, NM), np.float64)
    for b in range(B):
        G = y[b].sum(0)
        nk = int((G > 0).sum())
        for k in range(NM):
            if G[k] == 0:
                continue
            o = np.argsort(-e[b, :, k], kind='stable')
            ys = y[b, o, k]
            c = np.cumsum(ys) - ys
            Gn = (G[k] + np.arange(P) - c).astype(np.float64)
            g = np.where(ys, -1.0 / Gn, (G[k] - c) / (Gn * (Gn + 1.0))) / (B * nk)
            g[e[b, o, k] == 0] = 0.0
            out[b, o, k] = g
    return time.perf_counter() - t0, out.reshape(pred.shape[:3] + (NM,))


def cmd_ops(a):
    from multimodal_segmentation_amd import ops
    lines = []
    bpr = 8.0 * C / NM + 8 + 3 * 24 + 16 + 20
    for B, H in ((8, 256), (8, 512)):
        rng = np.random.RandomState(3)
        host_t = ellipse_target(rng, B, H, H)
        target = torch.as_tensor(host_t).cuda()
        pred = torch.softmax(3.0 * torch.randn(B, H, H, C, device='cuda'), -1).contiguous()
        w = torch.ones(1, device='cuda')
        m = ops.lovasz_map(pred, target, NM)
        t_map = bench(lambda: ops.lovasz_map(pred, target, NM))

        def term():
            loss, dpred = torch.zeros(1, device='cuda'), state['dpred']
            ll = ops.lovasz_term(pred, target, m, NM)
            ops.lovasz_grad_add(m, dpred, NM, 1.0, w)
            ops.boundary_combine(loss, ll, w)
        state = {'dpred': torch.zeros_like(pred)}
        t_term = bench(term)
        t_seg = bench(lambda: ops.seg_loss(pred, target, NM, 0.01, 1.0))
        t_bnd = bench(lambda: ops.boundary_map(target, NM))
        t_host, ref = (float('nan'), None) if a.no_host else host_map(pred.cpu().numpy(), host_t)
        if ref is not None:
            err = np.abs(m.cpu().numpy().astype(np.float64) - ref)
            assert np.all(err <= 2.0 ** -23 * np.abs(ref)), 'map differs from the restatement'
        recs = B * H * H * NM
        lines.append(dict(B=B, H=H, C=C, num_masks=NM, lovasz_map_us=round(t_map, 2), term_grad_combine_us=round(t_term, 2),
                          seg_loss_us=round(t_seg, 2), boundary_map_us=round(t_bnd, 2), map_over_seg_loss=round(t_map / t_seg, 2),
                          map_over_boundary_map=round(t_map / t_bnd, 2), map_bytes_per_record=bpr,
                          map_GBs=round(recs * bpr / t_map / 1e3, 1), lovasz_term=round(float(ops.lovasz_term(pred, target, m, NM).item()), 5),
                          host_numpy_ms=round(t_host * 1e3, 1)))
        print(json.dumps(lines[-1]), flush=True)
    if a.markdown:
        keys = ('B', 'H', 'lovasz_map_us', 'term_grad_combine_us', 'seg_loss_us', 'boundary_map_us', 'map_over_boundary_map', 'map_GBs',
                'host_numpy_ms')
        print('| ' + ' | '.join(keys) + ' |')
        print('|' + '---|' * len(keys))
        for ln in lines:
            print('| ' + ' | '.join(str(ln[k]) for k in keys) + ' |')


def build_step(w_lovasz, hip_graphs, ref=None, B=8, S=256):
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
    conf.hip_graphs, conf.w_lovasz = hip_graphs, w_lovasz
    conf.folder = tempfile.mkdtemp(prefix='lovasz_bench_')
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
    weights = [float(v) for v in a.weights.split(',')]
    variants = [(w, g) for g in (False, True) for w in weights]
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
                steps[v][1]()
            torch.cuda.synchronize()
            times[v].append((time.perf_counter() - t0) / a.steps * 1e3)
    out = {}
    for (wl, g), ts in times.items():
        out['%s_w%d_ms' % ('graph' if g else 'eager', int(wl))] = round(statistics.median(ts), 3)
        out['%s_w%d_spread_ms' % ('graph' if g else 'eager', int(wl))] = round(max(ts) - min(ts), 3)
    if 0.0 in weights and 1.0 in weights:
        out['eager_overhead_ms'] = round(out['eager_w1_ms'] - out['eager_w0_ms'], 3)
        out['graph_overhead_ms'] = round(out['graph_w1_ms'] - out['graph_w0_ms'], 3)
    out.update(batch=8, size=256, steps=a.steps, rounds=a.rounds, warmup=a.warmup, root=ROOT)
    print(json.dumps(out), flush=True)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--root', help='checkout to import the package from (default: the one this file is in)')
    sub = ap.add_subparsers(dest='cmd', required=True)
    p = sub.add_parser('ops')
    p.add_argument('--markdown', action='store_true')
    p.add_argument('--no-host', dest='no_host', action='store_true')
    p = sub.add_parser('step')
    p.add_argument('--steps', type=int, default=10)
    p.add_argument('--warmup', type=int, default=4)
    p.add_argument('--rounds', type=int, default=5)
    p.add_argument('--weights', default='0,1', help='comma-separated w_lovasz values to time (default 0,1)')
    p.add_argument('--root', help=argparse.SUPPRESS)
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit('lovasz_bench: needs a GPU (the kernels have no CPU path)')
    (cmd_ops if a.cmd == 'ops' else cmd_step)(a)


if __name__ == '__main__':
    main()
