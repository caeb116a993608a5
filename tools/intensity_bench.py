#!/usr/bin/env python
"""Isolated timings of the MR intensity augmentation of a training batch (csrc/intensity.hip): the plain mmseg_augment_gather of B slices of
H x H x C from a resident set of 32, then the gather followed by each intensity operation alone (blur, bias field, contrast, gamma, noise;
every sample on) and by all of them, as AugmentFlow launches them for ONE image array: the host draws and tables, their uploads,
mmseg_intensity_stats, mmseg_intensity_blur, the bias field's mmseg_elastic_field and mmseg_intensity_apply.  Beside them the numpy + scipy
restatement of all operations on the host.  One JSON line per case, and a markdown table with --markdown.

    python tools/intensity_bench.py [--markdown] [--no-host] [B=8] [H=256] [C=1]

The times are device events around 50 calls and include what the host adds between launches; for the kernels alone run
`rocprofv3 --kernel-trace --stats -- python tools/intensity_bench.py --no-host`.
"""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from multimodal_segmentation_amd import nn, ops
from multimodal_segmentation_amd.utils import augment

GEOMETRY = dict(rotation_range=20., width_shift_range=0.1, height_shift_range=0.1, shear_range=10., zoom_range=0.1, fill_mode='reflect',
                horizontal_flip=True, vertical_flip=True)
CASES = (('blur', dict(blur_sigma_range=(0.5, 1.5))),
         ('bias', dict(bias_field_strength=0.3, bias_field_sigma=32.)),
         ('contrast', dict(contrast_range=(0.75, 1.25))),
         ('gamma', dict(gamma_range=(0.7, 1.5), gamma_invert_prob=0.5)),
         ('noise', dict(noise_std_max=0.1)))
CASES += (('all', {k: v for _, p in CASES for k, v in p.items()}),)
FP32_ITERATION_MS = 128.          # the fp32 training iteration of the flagship benchmark, for the share column


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


def host_restatement(x, params, seed, batch):
    """every operation of `params` on the host batch x [B,H,W,C]: numpy + scipy + vectorised Philox; seconds"""
    from scipy import ndimage as ndi
    B, H, W, C = x.shape
    t0 = time.perf_counter()
    d = augment.intensity_draws(params, seed, batch, B, 1)
    p = augment.intensity_params(params, seed)
    m32, u64 = np.uint64(0xffffffff), np.uint64

    def philox(c, k):
        c = [np.asarray(v, np.uint64) * np.ones(len(c[0]), np.uint64) for v in c]
        k = [u64(k[0] & 0xffffffff), u64(k[1] & 0xffffffff)]
        for _ in range(10):
            p0, p1 = u64(0xD2511F53) * c[0], u64(0xCD9E8D57) * c[2]
            c = [(p1 >> u64(32)) ^ c[1] ^ k[0], p1 & m32, (p0 >> u64(32)) ^ c[3] ^ k[1], p0 & m32]
            k = [(k[0] + u64(0x9E3779B9)) & m32, (k[1] + u64(0xBB67AE85)) & m32]
        return c

    out = np.zeros_like(x)
    for b in range(B):
        v = x[b].astype(np.float64)
        lo, hi, mean = v.min(), v.max(), v.mean()
        if d['blur'][0, b]:
            v = np.stack([ndi.gaussian_filter(v[..., ch], d['sigma'][0, b], mode='reflect', truncate=4.0) for ch in range(C)], -1)
            v = v.astype(np.float32).astype(np.float64)
        if d['bias'][0, b]:
            P = philox((np.arange(H * W), b, 0, 0), (p['seed'] + 0x9E3779B9, batch))
            u = ((P[0] >> u64(8)).astype(np.float64) * 2.0 ** -23 - 1.0).reshape(H, W)
            f = p['bias_strength'] * p['bias_sigma'] * np.sqrt(12 * np.pi) * ndi.gaussian_filter(u, p['bias_sigma'], mode='reflect', truncate=4.0)
            v = lo + (v - lo) * np.exp(f.astype(np.float32).astype(np.float64))[..., None]
        if d['contrast'][0, b]:
            v = mean + (v - mean) * d['c'][0, b]
        if d['bias'][0, b] or d['contrast'][0, b]:
            v = np.clip(v, lo, hi)
        if d['gamma'][0, b] and hi > lo:
            t = np.clip((v - lo) / (hi - lo), 0, 1)
            t = 1 - (1 - t) ** d['g'][0, b] if d['invert'][0, b] else t ** d['g'][0, b]
            v = lo + t * (hi - lo)
        if d['noise'][0, b]:
            P = philox((np.arange(H * W * C), b, 0, 3), (p['seed'], batch))
            u1, u2 = ((P[0] >> u64(8)).astype(np.float64) + 1) * 2.0 ** -24, (P[1] >> u64(8)).astype(np.float64) * 2.0 ** -24
            v = v + d['std'][0, b] * (np.sqrt(-2 * np.log(u1)) * np.cos(2 * np.pi * u2)).reshape(H, W, C)
        out[b] = v
    return time.perf_counter() - t0


def main(argv=None):
    argv = list(sys.argv[1:] if argv is None else argv)
    markdown, no_host = '--markdown' in argv, '--no-host' in argv
    argv = [a for a in argv if a not in ('--markdown', '--no-host')]
    if not torch.cuda.is_available():
        raise SystemExit('intensity_bench: needs a GPU (the kernels have no CPU path)')
    B = int(argv[0]) if len(argv) > 0 else 8
    H = int(argv[1]) if len(argv) > 1 else 256
    C = int(argv[2]) if len(argv) > 2 else 1
    n, seed = 32, 5
    nn.set_default_device('cuda:0')
    data = torch.rand(n, H, H, C, device='cuda') * 2 - 1
    plain = augment.AugmentFlow([data], B, seed, 'cuda', GEOMETRY)
    t_plain = bench(lambda: next(plain))
    lines = [dict(case='gather', B=B, H=H, C=C, flow_us=round(t_plain, 2), added_us=0.0, share_of_fp32_iteration_pct=0.0,
                  host_scipy_ms=float('nan'))]
    print(json.dumps(lines[-1]), flush=True)
    for name, keys in CASES:
        params = dict(GEOMETRY, **keys)
        flow = augment.AugmentFlow([data], B, seed, 'cuda', params, n_images=1)
        t = bench(lambda: next(flow))
        t_host = float('nan') if no_host else host_restatement(next(plain).cpu().numpy(), params, seed, 0)
        lines.append(dict(case=name, B=B, H=H, C=C, flow_us=round(t, 2), added_us=round(t - t_plain, 2),
                          share_of_fp32_iteration_pct=round((t - t_plain) / (FP32_ITERATION_MS * 1e3) * 100, 3),
                          host_scipy_ms=round(t_host * 1e3, 1)))
        print(json.dumps(lines[-1]), flush=True)
    if markdown:
        keys = ('case', 'flow_us', 'added_us', 'share_of_fp32_iteration_pct', 'host_scipy_ms')
        print('| ' + ' | '.join(keys) + ' |')
        print('|' + '---|' * len(keys))
        for ln in lines:
            print('| ' + ' | '.join(str(ln[k]) for k in keys) + ' |')


if __name__ == '__main__':
    main()
