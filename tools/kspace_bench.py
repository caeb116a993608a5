#!/usr/bin/env python
"""Isolated timings of the MR k-space artefact augmentation of a training batch (csrc/kspace.hip): the plain mmseg_augment_gather of B
slices of H x H x C from a resident set of 32, then the gather followed by each k-space operation alone (motion, ghosting, Gibbs, spikes,
Rician noise; every sample on) and by all of them, as AugmentFlow launches them for ONE image array: the host draws and table, its upload,
mmseg_intensity_stats, mmseg_kspace_forward, mmseg_kspace_apply and mmseg_kspace_inverse.  Beside them the intensity stage with all of its
operations on (tools/intensity_bench.py's `all`), the five k-space launches alone on a resident batch (no gather, no host work), and the
numpy.fft restatement of all operations on the host.  One JSON line per case, and a markdown table with --markdown.

    python tools/kspace_bench.py [--markdown] [--no-host] [B=8] [H=256] [C=1]

The stage moves BYTES_PER_PIXEL = 136 bytes per pixel and channel: the forward pass along W reads 4 and writes 16, the pass along H, the
rule and the inverse pass along H read and write 16 each, the inverse pass along W reads 16 and writes 4.  `launches_GBps` is that traffic
over the time of the five launches alone.

The times are device events around 50 calls and include what the host adds between launches; for the kernels alone run
`rocprofv3 --kernel-trace --stats -- python tools/kspace_bench.py --no-host`.
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
CASES = (('motion', dict(motion_shift_max=3., motion_segments=4)),
         ('ghost', dict(ghost_count_range=(2, 4), ghost_intensity_range=(0.2, 0.6))),
         ('gibbs', dict(gibbs_cutoff_range=(0.4, 0.8))),
         ('spike', dict(spike_count_max=3, spike_intensity_range=(0.05, 0.2))),
         ('rician', dict(rician_std_max=0.05)))
CASES += (('all', {k: v for _, p in CASES for k, v in p.items()}),)
INTENSITY_ALL = dict(gamma_range=(0.7, 1.5), gamma_invert_prob=0.5, contrast_range=(0.75, 1.25), noise_std_max=0.1,
                     blur_sigma_range=(0.5, 1.5), bias_field_strength=0.3, bias_field_sigma=32.)
BYTES_PER_PIXEL = 4 + 8 * 16 + 4
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
    """every operation of `params` on the host batch x [B,H,W,C] with numpy.fft, written out from the table; seconds"""
    B, H, W, C = x.shape
    t0 = time.perf_counter()
    table = augment.kspace_tables(augment.kspace_draws(params, seed, batch, B, 1, H, W), 0, H, W)
    fy, fx = np.fft.fftfreq(H) * H, np.fft.fftfreq(W) * W
    ky, kx = np.meshgrid(fy, fx, indexing='ij')
    out = x.copy()
    for b in range(B if table is not None else 0):
        row = table[b]
        flags = int(row[0])
        if not flags:
            continue
        v = x[b].astype(np.float64)
        lo = v.min()
        X = np.fft.fft2(np.moveaxis(v - lo, -1, 0), axes=(1, 2))
        kp, P = (kx, W) if row[1] else (ky, H)
        if flags & 1:
            seg = (row[3:3 + int(row[2])][None, None, :] <= (kp + P // 2)[..., None]).sum(-1)
            X = X * np.exp(-2j * np.pi * (ky * row[10 + 2 * seg] / H + kx * row[11 + 2 * seg] / W))
        if flags & 2:
            X = X * np.where((kp % row[26] == 0) & (kp != 0), row[27], 1.0)
        if flags & 4:
            X = X * (4.0 * (ky * ky * W * W + kx * kx * H * H) <= row[28])
        if flags & 8:
            A = (v - lo).sum() / C
            for i in range(int(row[29])):
                u, w, c, s = row[30 + 4 * i:34 + 4 * i]
                X[:, int(u), int(w)] += A * (c + 1j * s)
                X[:, -int(u) % H, -int(w) % W] += A * (c - 1j * s)
        z = np.fft.ifft2(X, axes=(1, 2))
        if flags & 16:
            rs = np.random.RandomState(b)          # the device draws Philox words; the host's cost is about the same with any generator
            z = z + row[46] * (rs.standard_normal(z.shape) + 1j * rs.standard_normal(z.shape))
        out[b] = np.moveaxis(lo + np.abs(z), 0, -1)
    return time.perf_counter() - t0


def main(argv=None):
    argv = list(sys.argv[1:] if argv is None else argv)
    markdown, no_host = '--markdown' in argv, '--no-host' in argv
    argv = [a for a in argv if a not in ('--markdown', '--no-host')]
    if not torch.cuda.is_available():
        raise SystemExit('kspace_bench: needs a GPU (the kernels have no CPU path)')
    B = int(argv[0]) if len(argv) > 0 else 8
    H = int(argv[1]) if len(argv) > 1 else 256
    C = int(argv[2]) if len(argv) > 2 else 1
    n, seed = 32, 5
    nn.set_default_device('cuda:0')
    data = torch.rand(n, H, H, C, device='cuda') * 2 - 1
    plain = augment.AugmentFlow([data], B, seed, 'cuda', GEOMETRY)
    t_plain = bench(lambda: next(plain))
    nan = float('nan')
    lines = [dict(case='gather', B=B, H=H, C=C, flow_us=round(t_plain, 2), added_us=0.0, launches_us=nan, launches_GBps=nan,
                  share_of_fp32_iteration_pct=0.0, host_numpy_ms=nan)]
    print(json.dumps(lines[-1]), flush=True)
    inten = augment.AugmentFlow([data], B, seed, 'cuda', dict(GEOMETRY, **INTENSITY_ALL), n_images=1)
    t = bench(lambda: next(inten))
    lines.append(dict(case='intensity-all', B=B, H=H, C=C, flow_us=round(t, 2), added_us=round(t - t_plain, 2), launches_us=nan,
                      launches_GBps=nan, share_of_fp32_iteration_pct=round((t - t_plain) / (FP32_ITERATION_MS * 1e3) * 100, 3),
                      host_numpy_ms=nan))
    print(json.dumps(lines[-1]), flush=True)
    x = next(plain).clone()
    stats = ops.intensity_stats(x)
    for name, keys in CASES:
        params = dict(GEOMETRY, **keys)
        flow = augment.AugmentFlow([data], B, seed, 'cuda', params, n_images=1)
        t = bench(lambda: next(flow))
        table = nn.host_to_device(augment.kspace_tables(augment.kspace_draws(params, seed, 0, B, 1, H, H), 0, H, H), 'cuda', np.float64)
        spec = ops.kspace_spectrum_buffer(x)

        def launches():
            ops.kspace_forward(x, table, stats, spec)
            ops.kspace_apply(spec, table, stats)
            ops.kspace_inverse(spec, table, stats, x, seed, 0, 0)

        t_k = bench(launches)
        t_host = nan if no_host else host_restatement(next(plain).cpu().numpy(), params, seed, 0)
        lines.append(dict(case=name, B=B, H=H, C=C, bytes_per_pixel=BYTES_PER_PIXEL, flow_us=round(t, 2), added_us=round(t - t_plain, 2),
                          launches_us=round(t_k, 2),
                          launches_GBps=round(BYTES_PER_PIXEL * B * H * H * C / (t_k * 1e-6) / 1e9, 1),
                          share_of_fp32_iteration_pct=round((t - t_plain) / (FP32_ITERATION_MS * 1e3) * 100, 3),
                          host_numpy_ms=round(t_host * 1e3, 1)))
        print(json.dumps(lines[-1]), flush=True)
    if markdown:
        keys = ('case', 'flow_us', 'added_us', 'launches_us', 'launches_GBps', 'share_of_fp32_iteration_pct', 'host_numpy_ms')
        print('| ' + ' | '.join(keys) + ' |')
        print('|' + '---|' * len(keys))
        for ln in lines:
            print('| ' + ' | '.join(str(ln[k]) for k in keys) + ' |')


if __name__ == '__main__':
    main()
