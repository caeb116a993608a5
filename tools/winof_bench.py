#!/usr/bin/env python
"""A/B of the predict-mode 3x3 'same' layers (Conv2D -> folded BatchNorm -> ReLU, fp32) of the anatomy encoders at the benchmark's shapes,
batch 8 (level L of the UNet = 256 / 2^L pixels; a = first, b = second convolution of a block, cat = the one that reads the skip): the parent's route against the fused Winograd F(2x2,3x3) kernel (mmseg_conv2d_fwd_winof, one launch, no workspace).  The parent's
route is the single direct launch (mmseg_conv2d_fwd_scaled) for the six wide layers and the un-fused Winograd sequence
(mmseg_conv2d_fwd_wino) where mmseg_conv2d_wino_ok admits the layer in its default mode; both are timed.  The weight images are cached per
weight version in the product and therefore outside the timed sequences.  The routes alternate in ONE process on random post-ReLU data;
ROUNDS rounds of ITERS launches each; the table gives the minimum and the spread (max - min) of the rounds.  A shape is admitted to the
default mode only if even the slowest round of the fused kernel beats the fastest round of the parent's route.  err = largest deviation
from an fp64 convolution computed on the device (nine shifted matrix products), relative to the largest magnitude, for the fused and the
un-fused route on the same inputs.  The last shape is the segmentor's layer: for information, never routed.

Each shape runs in a child process of its own under a time limit; after a child that fails no further one is started.

    python tools/winof_bench.py [OUT]      (default OUT: profiles/winof_ab.txt)"""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

# layer, B, H, C1, C2, Cout
SHAPES = [('L0 b', 8, 256, 64, 0, 64), ('L0 cat', 8, 256, 64, 64, 64), ('L1 b', 8, 128, 128, 0, 128), ('L1 cat', 8, 128, 128, 128, 128),
          ('L1 a', 8, 128, 64, 0, 128), ('L2 a', 8, 64, 128, 0, 256),
          # the deep layers of the un-fused route (tools/wino_bench.py); the two layers at 16 x 16 are narrower than a block of the fused kernel
          ('L2 b', 8, 64, 256, 0, 256), ('L2 cat', 8, 64, 256, 256, 256), ('L3 b', 8, 32, 512, 0, 512), ('L3 cat', 8, 32, 512, 512, 512),
          ('L3 a', 8, 32, 256, 0, 512), ('seg c1', 32, 256, 64, 0, 64)]
ROUNDS, ITERS = 5, 20
CHILD_LIMIT_S = 150
HEADER = '%-8s %-20s %-7s %9s %8s %9s %8s %9s %8s %8s %9s %9s %9s %6s' % (
    'layer', 'B,H,C1,C2,Cout', 'parent', 'direct ms', 'sprd', 'unfused', 'sprd', 'fused ms', 'sprd', 'speedup', 'saved ms', 'err fused', 'err unf.', 'admit')


def timeit(fn, iters):
    import torch
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(iters):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / iters


def reference64(x, w, b, sc):
    """relu(conv3x3_same(x) * sc + b) in fp64 on the device, image by image: nine shifted matrix products"""
    import torch
    B, H, W, C = x.shape
    out = []
    for i in range(B):
        xp = torch.nn.functional.pad(x[i].double(), (0, 0, 1, 1, 1, 1))
        acc = torch.zeros(H * W, w.shape[3], dtype=torch.float64, device=x.device)
        for kh in range(3):
            for kw in range(3):
                acc += xp[kh:kh + H, kw:kw + W].reshape(H * W, C) @ w[kh, kw].double()
        out.append(torch.relu(acc * sc.double() + b.double()).reshape(H, W, -1))
    return torch.stack(out)


def run_shape(i):
    import torch
    from multimodal_segmentation_amd import _native as N, ops as P
    name, B, H, C1, C2, Cout = SHAPES[i]
    P.set_conv_precision('fp32')
    dev = torch.device('cuda')
    Cin = C1 + C2
    x1 = torch.relu(torch.randn(B, H, H, C1, device=dev))
    x2 = torch.relu(torch.randn(B, H, H, C2, device=dev)) if C2 else None
    w = torch.randn(3, 3, Cin, Cout, device=dev) * (2.0 / (9 * Cin)) ** 0.5
    b, sc = torch.randn(Cout, device=dev) * 0.1, torch.rand(Cout, device=dev) + 0.5
    wp = torch.empty(w.numel(), device=dev)
    N.call('mmseg_conv2d_wprep', w, wp, 3, 3, Cin, Cout, 0)
    U = torch.empty(16 * Cin * Cout, device=dev)
    N.call('mmseg_conv2d_wprep_wino', w, U, Cin, Cout)
    unf_is_parent = bool(N.call('mmseg_conv2d_wino_ok', B, H, H, C1, C2, Cout))      # (default mode)
    need = N.call('mmseg_conv2d_wino_workspace', B, H, H, C1, C2, Cout)
    with_unf = need * 4 <= (6 << 30)
    ws = torch.empty(need if with_unf else 4, device=dev)
    ys = [torch.empty(B, H, H, Cout, device=dev) for _ in range(3)]
    direct = lambda: N.call('mmseg_conv2d_fwd_scaled', x1, x2, w, wp, b, sc, ys[0], B, H, H, C1, C2, H, H, Cout, 3, 3, 1, 1, 1, 0, 1, 0.0)
    unfused = lambda: N.call('mmseg_conv2d_fwd_wino', x1, x2, U, b, sc, ys[1], B, H, H, C1, C2, Cout, 1, 0.0, ws, ws.numel())
    fused = lambda: N.call('mmseg_conv2d_fwd_winof', x1, x2, U, b, sc, ys[2], B, H, H, C1, C2, Cout, 1, 0.0)
    fns = [direct, unfused if with_unf else None, fused]
    for fn in fns:
        if fn is not None:
            fn()
    torch.cuda.synchronize()
    nb = min(B, 2)                                   # the fp64 reference of two images
    xr = x1[:nb] if x2 is None else torch.cat([x1[:nb], x2[:nb]], dim=3)
    ref = reference64(xr, w, b, sc)
    err = lambda y: ((y[:nb].double() - ref).abs().max() / ref.abs().max()).item()
    ef, eu = err(ys[2]), (err(ys[1]) if with_unf else float('nan'))
    del ref, xr
    t = {0: [], 1: [], 2: []}
    for _ in range(ROUNDS):
        for k, fn in enumerate(fns):
            if fn is not None:
                t[k].append(timeit(fn, ITERS))
    mn = lambda k: min(t[k]) if t[k] else float('nan')
    sp = lambda k: max(t[k]) - min(t[k]) if t[k] else float('nan')
    pk = 1 if (unf_is_parent and with_unf) else 0
    admit = max(t[2]) < min(t[pk])
    print('%-8s %-20s %-7s %9.3f %8.3f %9.3f %8.3f %9.3f %8.3f %7.2fx %9.3f %9.1e %9.1e %6s' % (
        name, '%d,%d,%d,%d,%d' % (B, H, C1, C2, Cout), 'unfused' if pk else 'direct', mn(0), sp(0), mn(1), sp(1), mn(2), sp(2),
        mn(pk) / mn(2), mn(pk) - mn(2), ef, eu, 'yes' if admit else 'no'))


def main():
    if len(sys.argv) > 2 and sys.argv[1] == '--shape':
        run_shape(int(sys.argv[2]))
        return 0
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, 'profiles', 'winof_ab.txt')
    lines = ['# tools/winof_bench.py: direct = mmseg_conv2d_fwd_scaled, unfused = mmseg_conv2d_fwd_wino (three launches, workspace), fused =',
             '# mmseg_conv2d_fwd_winof (one launch); parent = the route of the parent commit; weight images cached, not timed; ms per layer, min and',
             '# spread (max - min) of %d rounds x %d launches, alternating; speedup and saved ms against the parent route; err against fp64 relative' % (ROUNDS, ITERS),
             '# to the largest magnitude; admit = the slowest fused round beats the fastest round of the parent route', HEADER]
    for i in range(len(SHAPES)):
        try:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), '--shape', str(i)], stdout=subprocess.PIPE, timeout=CHILD_LIMIT_S)
        except subprocess.TimeoutExpired:
            lines.append('# %s: no result within %d s; stopped' % (SHAPES[i][0], CHILD_LIMIT_S))
            break
        if r.returncode != 0:
            lines.append('# %s: exit status %d; stopped' % (SHAPES[i][0], r.returncode))
            break
        lines.append(r.stdout.decode().strip().splitlines()[-1])
        print(lines[-1], flush=True)
    text = '\n'.join(lines) + '\n'
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, 'w') as f:
        f.write(text)
    return 0 if len(lines) == 5 + len(SHAPES) else 1


if __name__ == '__main__':
    sys.exit(main())
