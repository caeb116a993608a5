#!/usr/bin/env python
"""Static vs dynamic fp16 loss scale on BASELINE config #5 (3-modality MMSDNet, 320 x 320, batch 16, fp16 MFMA operands).

  python tools/loss_scale_bench.py time [--rounds R --steps K --warmup W]
      builds one model per mode (same weights), then alternates timed blocks of K generator steps (supervised_trainer.fit on one
      fixed batch) static, dynamic, static, ... R rounds; prints one JSON line with the per-step times of both modes, the median
      ratio, and the dynamic scalers' state (a skipped step is cheaper than an applied one: the count is reported).
  python tools/loss_scale_bench.py trace --mode static|dynamic [--steps K]
      K generator steps of one mode, for `rocprofv3 --kernel-trace --stats -- python tools/loss_scale_bench.py trace ...`.
  python tools/loss_scale_bench.py report STATIC_TRACE_DIR DYNAMIC_TRACE_DIR [--steps K]
      from the two kernel traces: per step, the static mode's unscale (axpby_kernel) and the dynamic mode's unscale_check_kernel,
      adam_kernel vs adam_guarded_kernel, with achieved HBM bandwidth (8 B per gradient element: one read, one write).
"""
import argparse
import csv
import glob
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

S, BATCH = 320, 16


def build(mode, ref=None):
    import numpy as np
    from multimodal_segmentation_amd import nn
    from multimodal_segmentation_amd.configuration import mmsdnet3_config_chaos
    from multimodal_segmentation_amd.models.mmsdnet import MMSDNet
    from multimodal_segmentation_amd.model_executors.mmsdnet_executor import MMSDNetExecutor
    from multimodal_segmentation_amd.utils.config import EasyDict
    import tempfile
    nn.set_default_device('cuda:0')
    conf = EasyDict(mmsdnet3_config_chaos.get())
    shp = (S, S, 1)
    conf.input_shape = shp
    conf.anatomy_encoder['input_shape'] = shp
    conf.anatomy_encoder['output_shape'] = (S, S, conf.anatomy_encoder['out_channels'])
    conf.d_mask_params['input_shape'] = (S, S, conf.num_masks)
    conf.n_pairs, conf.batch_size, conf.compute_dtype = 1, BATCH, 'fp16'
    conf.folder = tempfile.mkdtemp(prefix='loss_scale_bench_')
    if mode == 'dynamic':
        conf.loss_scale = 'dynamic'
    model = MMSDNet(conf)
    model.build()
    ms = model._all_component_models()
    if ref is not None:
        for m, w in zip(ms, ref):
            m.set_weights(w)
    ex = MMSDNetExecutor(conf, model)
    np.random.seed(5)
    ex.init_train_data(slices_per_volume=2)
    batch = next(ex.gen_labelled)
    x_list = [b for b in batch[:3]]
    m_list = [ex._five(b) for b in batch[3:]]
    tg = ex.generator_targets(x_list, m_list, True)
    n_out = model.n_out()
    eps = [np.random.RandomState(5 + i).standard_normal((BATCH, 8)).astype(np.float32) for i in range(n_out)]
    tr = model.supervised_trainer

    def step():
        return tr.fit(x_list, tg, eps=eps)
    return model, step, [m.get_weights() for m in ms]


def cmd_time(a):
    import torch
    runs = {}
    ref = None
    for mode in ('static', 'dynamic'):
        model, step, w = build(mode, ref)
        ref = ref or w
        for _ in range(a.warmup):
            step()
        runs[mode] = (model, step)
    torch.cuda.synchronize()
    per = {'static': [], 'dynamic': []}
    for _ in range(a.rounds):
        for mode in ('static', 'dynamic'):
            step = runs[mode][1]
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(a.steps):
                step()
            torch.cuda.synchronize()
            per[mode].append((time.perf_counter() - t0) / a.steps * 1e3)
    ratios = [d / s for s, d in zip(per['static'], per['dynamic'])]
    scalers = {n: dict(scale=sc.scale(), skipped=sc.skipped_steps(), iterations=sc.iterations())
               for n, sc in runs['dynamic'][0].loss_scalers()}
    print(json.dumps(dict(workload='config #5: 3-modality MMSDNet %dx%d bs%d fp16, supervised_trainer.fit' % (S, S, BATCH),
                          rounds=a.rounds, steps_per_block=a.steps, ms_per_step=per,
                          median_ms=dict(static=statistics.median(per['static']), dynamic=statistics.median(per['dynamic'])),
                          median_ratio_dynamic_over_static=statistics.median(ratios), dynamic_scalers=scalers)))


def cmd_trace(a):
    import torch
    model, step, _ = build(a.mode)
    for _ in range(a.steps):
        step()
    torch.cuda.synchronize()
    arenas = [m.grad_arena.numel() for m in model.supervised_trainer.train_models]
    print(json.dumps(dict(mode=a.mode, steps=a.steps, grad_floats=sum(arenas), arenas=arenas)))


def _kernels(d):
    files = glob.glob(os.path.join(d, '**', '*kernel_trace.csv'), recursive=True)
    out = {}
    for f in files:
        for r in csv.DictReader(open(f)):
            name = r['Kernel_Name'].split('(')[0]
            out.setdefault(name, []).append((int(r['End_Timestamp']) - int(r['Start_Timestamp'])) / 1e3)
    return out


def cmd_report(a):
    st, dy = _kernels(a.static_dir), _kernels(a.dynamic_dir)
    pick = lambda k, pat: next((v for n, v in k.items() if n.endswith(pat)), [])
    rows = {}
    for label, k, pat in (('static unscale (axpby_kernel)', st, 'axpby_kernel'), ('dynamic unscale+check (unscale_check_kernel)', dy, 'unscale_check_kernel'),
                          ('static adam_kernel', st, 'adam_kernel'), ('dynamic adam_guarded_kernel', dy, 'adam_guarded_kernel'),
                          ('dynamic loss_scale_update_kernel', dy, 'loss_scale_update_kernel')):
        v = pick(k, pat)
        rows[label] = dict(launches=len(v), total_us=round(sum(v), 1), median_us=round(statistics.median(v), 2) if v else None)
    print(json.dumps(rows, indent=1))


def main():
    ap = argparse.ArgumentParser()
    sub = ap.add_subparsers(dest='cmd', required=True)
    p = sub.add_parser('time')
    p.add_argument('--rounds', type=int, default=6)
    p.add_argument('--steps', type=int, default=5)
    p.add_argument('--warmup', type=int, default=3)
    p = sub.add_parser('trace')
    p.add_argument('--mode', choices=['static', 'dynamic'], required=True)
    p.add_argument('--steps', type=int, default=4)
    p = sub.add_parser('report')
    p.add_argument('static_dir')
    p.add_argument('dynamic_dir')
    a = ap.parse_args()
    {'time': cmd_time, 'trace': cmd_trace, 'report': cmd_report}[a.cmd](a)


if __name__ == '__main__':
    main()
