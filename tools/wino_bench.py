#!/usr/bin/env python
"""A/B of the predict-mode 3x3 'same' layers (Conv2D -> folded BatchNorm -> ReLU, fp32) of the anatomy encoders' deep levels at the
benchmark's shapes, batch 8: today's single direct launch (mmseg_conv2d_fwd_scaled) against the Winograd F(2x2,3x3) sequence
(mmseg_conv2d_fwd_wino: input transform, sixteen products in one launch, output transform; the weight image is cached per weight version
and therefore outside the timed sequence, its launch is timed separately in the last column).  Old and new alternate in ONE process on
random post-ReLU data; ROUNDS rounds of ITERS launches each; the table gives the minimum and the spread (max - min) of the rounds.  A shape
is admitted to the default mode only if even the slowest round of the new sequence beats the fastest round of the old launch.

Each shape runs in a child process of its own under a time limit; after a child that fails no further one is started.

    python tools/wino_bench.py [OUT]      (default OUT: profiles/wino_ab.txt)"""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

# layer, B, H, C1, C2, Cout
SHAPES = [('d3b/u2b', 8, 32, 512, 0, 512), ('u2a', 8, 32, 512, 512, 512), ('d3a', 8, 32, 256, 0, 512), ('d4b', 8, 16, 1024, 0, 1024),
          ('d4a', 8, 16, 512, 0, 1024), ('d2b/u1b', 8, 64, 256, 0, 256), ('u1a', 8, 64, 256, 256, 256), ('d2a', 8, 64, 128, 0, 256)]
ROUNDS, ITERS = 5, 20
CHILD_LIMIT_S = 120
HEADER = '%-8s %-22s %9s %9s %9s %9s %8s %9s %9s %9s %6s' % ('layer', 'B,H,C1,C2,Cout', 'old ms', 'old sprd', 'new ms', 'new sprd', 'speedup',
                                                          'saved ms', 'err', 'wprep ms', 'admit')


def timeit(fn, iters):
    import torch
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(iters):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / iters


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
    wprep = lambda: N.call('mmseg_conv2d_wprep_wino', w, U, Cin, Cout)
    wprep()
    ws = torch.empty(N.call('mmseg_conv2d_wino_workspace', B, H, H, C1, C2, Cout), device=dev)
    y0, y1 = torch.empty(B, H, H, Cout, device=dev), torch.empty(B, H, H, Cout, device=dev)
    old = lambda: N.call('mmseg_conv2d_fwd_scaled', x1, x2, w, wp, b, sc, y0, B, H, H, C1, C2, H, H, Cout, 3, 3, 1, 1, 1, 0, 1, 0.0)
    new = lambda: N.call('mmseg_conv2d_fwd_wino', x1, x2, U, b, sc, y1, B, H, H, C1, C2, Cout, 1, 0.0, ws, ws.numel())
    old(); new()
    torch.cuda.synchronize()
    err = ((y1 - y0).abs().max() / y0.abs().max()).item()
    t = {0: [], 1: []}
    for _ in range(ROUNDS):
        for k, fn in enumerate((old, new)):
            t[k].append(timeit(fn, ITERS))
    tw = min(timeit(wprep, ITERS) for _ in range(3))
    o, n = min(t[0]), min(t[1])
    admit = max(t[1]) < o
    print('%-8s %-22s %9.3f %9.3f %9.3f %9.3f %7.2fx %9.3f %9.1e %9.3f %6s' % (name, '%d,%d,%d,%d,%d' % (B, H, C1, C2, Cout), o, max(t[0]) - o, n,
                                                                           max(t[1]) - n, o / n, o - n, err, tw, 'yes' if admit else 'no'))


def main():
    if len(sys.argv) > 2 and sys.argv[1] == '--shape':
        run_shape(int(sys.argv[2]))
        return 0
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, 'profiles', 'wino_ab.txt')
    lines = ['# tools/wino_bench.py: old = mmseg_conv2d_fwd_scaled (one direct launch), new = mmseg_conv2d_fwd_wino (input transform, 16 products, output',
             '# transform; weight image cached, timed apart); ms per sequence, min and spread (max - min) of %d rounds x %d launches, alternating' % (ROUNDS, ITERS),
             '# err = max |new - old| / max |old|; admit = the slowest new round beats the fastest old round', HEADER]
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
    sys.stdout.write(text)
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, 'w') as f:
        f.write(text)
    return 0 if len(lines) == 4 + len(SHAPES) else 1


if __name__ == '__main__':
    sys.exit(main())
