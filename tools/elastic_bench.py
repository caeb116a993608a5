#!/usr/bin/env python
"""Isolated timings of the elastic deformation of a training batch (csrc/augment.hip): mmseg_elastic_field (two launches: Philox noise
blurred along each row into an fp64 scratch, then blurred along each column) and mmseg_elastic_gather, beside plain mmseg_augment_gather on the same
batch and beside the numpy + scipy restatement on the host.  B slices of H x H x C from a resident set of 32, sigma 4 / 8 / 32 (blur
radius 16 / 32 / 128).  Algorithmic bytes per output element: the gather reads and writes 4 B each (+ 8 B of field per pixel, shared by
its C channels); the field writes 16 B and reads 16 B of scratch per pixel and writes 8 B -- its cost is the (2R + 1)-tap fp64 sums,
not memory.  One JSON line per (C, sigma), and a markdown table with --markdown.

    python tools/elastic_bench.py [--markdown] [--sigma S] [--no-host] [B=8] [H=256]

The times are device events around 50 calls and include what the host adds between launches; for the kernels alone run one sigma under
`rocprofv3 --kernel-trace --stats -- python tools/elastic_bench.py --sigma S --no-host`.
"""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from multimodal_segmentation_amd import ops
from multimodal_segmentation_amd.utils import augment

SIGMAS = (4.0, 8.0, 32.0)
CHANNELS = (1, 4)
PARAMS = dict(rotation_range=20., width_shift_range=0.1, height_shift_range=0.1, shear_range=10., zoom_range=0.1, fill_mode='reflect',
              horizontal_flip=True, vertical_flip=True)


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


def host_noise(seed, batch, b, H, W):
    """the field's noise in vectorised numpy: Philox4x32-10 on uint64 words -> u [2,H,W] fp64"""
    m32, u64 = np.uint64(0xffffffff), np.uint64
    c = [np.arange(H * W, dtype=np.uint64), np.full(H * W, b, np.uint64), np.zeros(H * W, np.uint64), np.zeros(H * W, np.uint64)]
    k = [u64(seed & 0xffffffff), u64(batch & 0xffffffff)]
    for _ in range(10):
        p0, p1 = u64(0xD2511F53) * c[0], u64(0xCD9E8D57) * c[2]
        c = [(p1 >> u64(32)) ^ c[1] ^ k[0], p1 & m32, (p0 >> u64(32)) ^ c[3] ^ k[1], p0 & m32]
        k = [(k[0] + u64(0x9E3779B9)) & m32, (k[1] + u64(0xBB67AE85)) & m32]
    return np.stack([(c[a] >> u64(8)).astype(np.float64) * 2.0 ** -23 - 1.0 for a in (0, 1)]).reshape(2, H, W)


def host_restatement(x, rows, mats, scale, sigma, seed, batch):
    """the same batch on the host: Philox + scipy gaussian_filter + map_coordinates per channel; seconds"""
    from scipy import ndimage as ndi
    B, (_, H, W, C) = len(rows), x.shape
    t0 = time.perf_counter()
    r, c = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing='ij')
    out = np.zeros((B, H, W, C), np.float32)
    for b in range(B):
        u = host_noise(seed, batch, b, H, W)
        d = [scale[b] * ndi.gaussian_filter(u[a], sigma, mode='reflect', truncate=4.0) for a in (0, 1)]
        m = mats[b]
        pr, pc = r + d[0], c + d[1]
        coords = np.stack([m[0] * pr + m[1] * pc + m[2], m[3] * pr + m[4] * pc + m[5]])
        for ch in range(C):
            out[b, ..., ch] = ndi.map_coordinates(x[rows[b], ..., ch], coords, order=1, mode='reflect')
    return time.perf_counter() - t0


def main(argv=None):
    argv = list(sys.argv[1:] if argv is None else argv)
    markdown = '--markdown' in argv
    no_host = '--no-host' in argv
    sigmas = SIGMAS
    if '--sigma' in argv:
        i = argv.index('--sigma')
        sigmas = (float(argv[i + 1]),)
        del argv[i:i + 2]
    argv = [a for a in argv if a not in ('--markdown', '--no-host')]
    if not torch.cuda.is_available():
        raise SystemExit('elastic_bench: needs a GPU (the kernels have no CPU path)')
    B = int(argv[0]) if len(argv) > 0 else 8
    H = int(argv[1]) if len(argv) > 1 else 256
    n, seed = 32, 5
    lines = []
    for C in CHANNELS:
        data = torch.randn(n, H, H, C, device='cuda')
        host = data.cpu().numpy()
        rows, mats, _, _, _ = augment.KerasTransformStream(n, B, seed, PARAMS, H, H, C).next()
        rows_d = torch.as_tensor(rows.astype(np.int32)).cuda()
        mat_d = torch.as_tensor(mats).cuda()
        t_plain = bench(lambda: ops.augment_gather(data, rows_d, mat_d, None, 1, 'reflect', 0.))
        for sigma in sigmas:
            alpha = 10. * sigma
            scale = torch.full((B,), alpha, dtype=torch.float64, device='cuda')
            disp = ops.elastic_field(scale, sigma, seed, 0, H, H)
            t_field = bench(lambda: ops.elastic_field(scale, sigma, seed, 0, H, H))
            t_gather = bench(lambda: ops.elastic_gather(data, rows_d, mat_d, disp, None, 1, 'reflect', 0.))
            t_host = float('nan') if no_host else host_restatement(host, rows, mats, np.full(B, alpha), sigma, seed, 0)
            elems = B * H * H * C
            lines.append(dict(B=B, H=H, C=C, sigma=sigma, R=ops.elastic_radius(sigma), rms_px=round(float(disp.double().pow(2).mean().sqrt()), 2),
                              augment_gather_us=round(t_plain, 2), elastic_field_us=round(t_field, 2),
                              elastic_gather_us=round(t_gather, 2), field_plus_gather_us=round(t_field + t_gather, 2),
                              gather_bytes_per_element=round(8 + 8. / C, 1), field_bytes_per_element=round(40. / C, 1),
                              elastic_gather_GBs=round(elems * (8 + 8. / C) / t_gather / 1e3, 1), host_scipy_ms=round(t_host * 1e3, 1)))
            print(json.dumps(lines[-1]), flush=True)
    if markdown:
        keys = ('C', 'sigma', 'R', 'augment_gather_us', 'elastic_field_us', 'elastic_gather_us', 'field_plus_gather_us',
                'gather_bytes_per_element', 'field_bytes_per_element', 'host_scipy_ms')
        print('| ' + ' | '.join(keys) + ' |')
        print('|' + '---|' * len(keys))
        for ln in lines:
            print('| ' + ' | '.join(str(ln[k]) for k in keys) + ' |')


if __name__ == '__main__':
    main()
