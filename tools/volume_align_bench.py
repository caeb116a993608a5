#!/usr/bin/env python
"""Device time of the alignment of a volume's modalities by mutual information (csrc/align.hip, ops.align_*) for one CHAOS-sized pair,
36 x 256 x 256 against 40 x 264 x 250 at the target resolution, at the defaults (32 bins, 3 levels, +-4 slices, +-21 pixels = 40 mm), beside
the numpy restatement (tests/volume_align_ref.py) on the host it runs on.  No speed target is set: the numbers are recorded, not asserted.

The pair is a phantom with the air of an MR frame: a body ellipse over about half the frame, zero outside it, the moving modality with
inverted organ contrast, its own texture, and cut (2, 9, -6) off the reference.  Device events around the Python ops, warmed up, median of
`--repeats` windows of `--calls` calls each:
  quantise     ops.preprocess_quantiles (the two percentiles, 8 launches) and ops.align_quantise (1 launch), per volume
  stage s      ops.align_histograms with and without the wave aggregation (the A/B of DESIGN.md section 8), ops.align_scores and
               ops.align_select for the candidates of that stage; pairs = the sampled voxel pairs of all its candidates (the N the scores
               kernel reports, summed)
  search       ops.align_search: all stages, 9 launches and 3 memsets, no host synchronisation
  align        ops.align_volumes: everything, with its one copy to the host
  --host       the restatement's quantise and search on the same volumes

Writes a markdown report (default profiles/volume_align_bench.md) and prints one JSON line per record.

    python tools/volume_align_bench.py [--repeats 5] [--calls 3] [--host] [--out profiles/volume_align_bench.md]
"""
import argparse
import importlib.util
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

from multimodal_segmentation_amd import nn, ops
from tests import volume_align_ref as A

TARGET = (1.89, 1.89)
O = 256
TRUTH = (2, 9, -6)
SHAPE_A, SHAPE_B = (36, 256, 256), (40, 264, 250)


def _generator():
    spec = importlib.util.spec_from_file_location('make_volume_folder', os.path.join(ROOT, 'tools', 'make_volume_folder.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def phantom(seed=0):
    """(a, b): int16 volumes, windows of one canvas, b moved by TRUTH in the convention of the rule"""
    gen = _generator()
    rng = np.random.RandomState(seed)
    canvas = 320
    y, x = np.mgrid[0:canvas, 0:canvas]
    body = ((y - canvas / 2.0) ** 2 / (0.36 * canvas) ** 2 + (x - canvas / 2.0) ** 2 / (0.30 * canvas) ** 2) < 1
    out = []
    for mod, (S, H, W), (dz, dy, dx) in ((0, SHAPE_A, (0, 0, 0)), (1, SHAPE_B, TRUTH)):
        image, _ = gen.make_volume(rng, 1000 - dz, mod, S, canvas, canvas, gen.label_values(4))
        image = image * body[None]
        y0 = 32 - A.centre_start(H, O) - dy
        x0 = 32 - A.centre_start(W, O) - dx
        out.append(np.ascontiguousarray(image[:, y0:y0 + H, x0:x0 + W]).astype(np.int16))
    return out


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
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--calls', type=int, default=3)
    ap.add_argument('--host', action='store_true', help='also time the numpy restatement on this host')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'volume_align_bench.md'))
    args = ap.parse_args(argv)
    dev = torch.device('cuda:0')
    nn.set_default_device('cuda:0')
    p = ops.align_params()
    B, L, Z = p['bins'], p['levels'], p['max_slices']
    Py, Px = (int(np.floor(p['max_shift_mm'] / t)) for t in TARGET)
    a, b = phantom()
    air = float((a == 0).mean())
    xa, xb = (torch.from_numpy(v.astype(np.float32)).to(dev) for v in (a, b))
    records = []

    def record(**kw):
        records.append(kw)
        print(json.dumps(kw))

    def ranks(x):
        return [int(np.floor((x.numel() - 1) * (q / 100.0))) for q in p['percentiles']]

    knots = [ops.preprocess_quantiles(x, x.shape[1:], ranks(x), True) for x in (xa, xb)]
    qa, qb = (ops.align_quantise(x, x.shape[1:], k, B) for x, k in zip((xa, xb), knots))
    for name, x, k in (('reference', xa, knots[0]), ('moving', xb, knots[1])):
        ms = device_ms(lambda: ops.preprocess_quantiles(x, x.shape[1:], ranks(x), True), args.calls, args.repeats)
        record(step='quantiles', volume=name, shape=list(x.shape), ms=ms[0], ms_min=ms[1], ms_max=ms[2])
        ms = device_ms(lambda: ops.align_quantise(x, x.shape[1:], k, B), args.calls, args.repeats)
        record(step='quantise', volume=name, shape=list(x.shape), ms=ms[0], ms_min=ms[1], ms_max=ms[2], voxels_per_s=x.numel() / ms[0] * 1e3)

    # the stages, each from the state the stages before it left
    state = torch.zeros(ops.ALIGN_STATE, dtype=torch.float64, device=dev)
    total = {False: 0.0, True: 0.0}
    for s in range(L - 1, -1, -1):
        t = 1 << s
        stage = ('lattice', Z, Py, Px) if s == L - 1 else ('refine', Z, Py, Px, state)
        h = ops.align_histograms(qa, qb, O, stage, t, B)
        sc = ops.align_scores(h, qa.shape, qb.shape, O, stage, t, p['min_overlap'])
        pairs = float(sc[:, 1].sum())
        C = int(h.shape[0])
        for agg in (False, True):
            other = ops.align_histograms(qa, qb, O, stage, t, B, aggregate=agg)
            assert torch.equal(other, h)
            ms = device_ms(lambda: ops.align_histograms(qa, qb, O, stage, t, B, aggregate=agg, out=h), args.calls, args.repeats)
            total[agg] += ms[0]
            record(step='histograms', stride=t, candidates=C, aggregate=agg, pairs=pairs, ms=ms[0], ms_min=ms[1], ms_max=ms[2],
                   pairs_per_s=pairs / ms[0] * 1e3)
        ms = device_ms(lambda: ops.align_scores(h, qa.shape, qb.shape, O, stage, t, p['min_overlap'], out=sc), args.calls, args.repeats)
        record(step='scores', stride=t, candidates=C, ms=ms[0], ms_min=ms[1], ms_max=ms[2])
        scratch = state.clone()
        sel_stage = stage if s == L - 1 else ('refine', Z, Py, Px, scratch)
        ms = device_ms(lambda: (scratch.copy_(state), ops.align_select(sc, sel_stage, t, scratch)), args.calls, args.repeats)
        record(step='select', stride=t, candidates=C, ms=ms[0], ms_min=ms[1], ms_max=ms[2])
        ops.align_select(sc, stage, t, state)
    record(step='histograms, all stages', aggregate=False, ms=total[False])
    record(step='histograms, all stages', aggregate=True, ms=total[True])
    for agg in (False, True):
        ms = device_ms(lambda: ops.align_search(qa, qb, O, Z, Py, Px, B, L, p['min_overlap'], aggregate=agg), args.calls, args.repeats)
        record(step='search', aggregate=agg, ms=ms[0], ms_min=ms[1], ms_max=ms[2])
    found = state.cpu().tolist()
    ms = device_ms(lambda: ops.align_volumes(xa, TARGET, xb, TARGET, TARGET, (O, O, 1)), args.calls, args.repeats)
    shift, rec = ops.align_volumes(xa, TARGET, xb, TARGET, TARGET, (O, O, 1))
    record(step='align', ms=ms[0], ms_min=ms[1], ms_max=ms[2], shift=list(shift), truth=list(TRUTH), score=rec[0], zero_score=rec[1], pairs=rec[2],
           default_aggregate=ops.ALIGN_AGGREGATE, air=air)
    host = None
    if args.host:
        t0 = time.time()
        ha = A.quantise(a, a.shape[1], a.shape[2], B)[0]
        hb = A.quantise(b, b.shape[1], b.shape[2], B)[0]
        t1 = time.time()
        want = A.search(ha, hb, O, Z, Py, Px, B, L, p['min_overlap'])
        t2 = time.time()
        host = dict(step='host restatement', quantise_s=t1 - t0, search_s=t2 - t1, shift=list(want['shift']), score=want['score'],
                    leads=want['leads'], quantised_equal=[float((ha == qa.cpu().numpy()).mean()), float((hb == qb.cpu().numpy()).mean())])
        record(**host)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, 'w') as f:
        f.write('# Alignment by mutual information: device time for one 36 x 256 x 256 pair\n\n')
        f.write('`python tools/volume_align_bench.py%s` on %s.  Defaults: %d bins, %d levels, +-%d slices, +-%d x %d pixels; %.0f %% of the '
                'reference volume is air (0).  Device events around the Python ops, median (min .. max) of %d windows of %d calls.\n\n'
                % (' --host' if args.host else '', torch.cuda.get_device_name(0), B, L, Z, Py, Px, 100 * air, args.repeats, args.calls))
        f.write('| step | detail | ms | rate |\n|---|---|---|---|\n')
        for r in records:
            if 'ms' not in r:
                continue
            detail = ', '.join('%s %s' % (k, r[k]) for k in ('volume', 'stride', 'candidates', 'aggregate') if k in r)
            rate = '%.3g pairs/s' % r['pairs_per_s'] if 'pairs_per_s' in r else ('%.3g voxels/s' % r['voxels_per_s'] if 'voxels_per_s' in r else '')
            span = ' (%.3f .. %.3f)' % (r['ms_min'], r['ms_max']) if 'ms_min' in r else ''
            f.write('| %s | %s | %.3f%s | %s |\n' % (r['step'], detail, r['ms'], span, rate))
        f.write('\nFound %s (truth %s), score %.6f against %.6f at zero shift, %d voxel pairs at stride 1; state block %s.\n'
                % (shift, TRUTH, rec[0], rec[1], rec[2], found))
        if host is not None:
            f.write('\nThe numpy restatement on this host: quantise %.2f s, search %.2f s, shift %s, score %.12f (device %.12f), stage leads %s; '
                    'share of equal quantised bytes %s.\n' % (host['quantise_s'], host['search_s'], host['shift'], host['score'], rec[0],
                                                              ['%.1e' % v for v in host['leads']], host['quantised_equal']))
    print('wrote', args.out)


if __name__ == '__main__':
    main()
