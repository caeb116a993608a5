#!/usr/bin/env python
"""Device time of the non-local means denoising (csrc/denoise.hip, ops.nlm_sigma / ops.nlm_denoise) for one CHAOS-sized volume, 36 x 256 x
256, beside the bias-field correction at its defaults on the same upload and -- with --host -- beside the numpy restatement
(tests/volume_denoise_ref.py) on a cropped volume on the host it runs on.  No speed target is set: the numbers are recorded, not asserted.

Device events around the Python ops, warmed up, median of `--repeats` windows of `--calls` calls each:
  sigma        ops.nlm_sigma: Immerkaer's estimate, 2 launches
  denoise      ops.nlm_denoise with a given sigma (1 launch) at the defaults (Rs 5, Rp 1) and at the largest radii (Rs 10, Rp 3), each for
               extent 2d and 3d (Rz 1 at the defaults, 4 at the largest radii).  The rate is voxel x offset x patch-tap per second, the
               offsets counted as the kernel walks them (all in-plane offsets; a dz only where the slice exists); a tap is one subtraction
               and one fused multiply-add, so `share_of_fp32_vector_peak` = 3 x taps / s over the 157.3 TFLOP/s of MI355X_MICROARCH.md --
               a whole-call figure from device events, launch included, not a kernel's counter.
  bias         ops.bias_correct at its defaults on the same volume: the step that follows in the chain
  --other_form LIB   a shared library that exports another mmseg_nlm_denoise (a kernel form under evaluation): timed in alternation with
               the built one on the same inputs, outputs compared.  This is how the two forms of DESIGN.md section 8 were compared.
Also recorded: the figures the tests' bar refers to (tests/test_volume_denoise.py), measured on the device for the tests' own cases.

--lds needs no GPU: it enumerates the LDS bank of every lane for the kernel's reads and stores under the model of MI355X_MICROARCH.md (LDS
table: ds_read_b32 / ds_write_b32 are served in the lane groups {0-31}, {32-63}, bank = (addr / 4) mod 32) and prints the worst number of
distinct words on one bank in a group: 1 = conflict-free.

Writes a markdown report (default profiles/volume_denoise_bench.md) and prints one JSON line per record.

    python tools/volume_denoise_bench.py [--repeats 5] [--calls 3] [--host] [--other_form LIB] [--out profiles/volume_denoise_bench.md]
    python tools/volume_denoise_bench.py --lds
"""
import argparse
import ctypes
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

from multimodal_segmentation_amd import nn, ops
from tests import volume_denoise_ref as D

SHAPE, SPACINGS = (36, 256, 256), (6.0, 1.6, 1.6)
SIGMA = 10.0
PEAK_FP32_VECTOR = 157.3e12
CONFIGS = (('defaults-2d', dict()), ('defaults-3d', dict(extent='3d')),
           ('largest-2d', dict(search_radius=10, patch_radius=3)), ('largest-3d', dict(search_radius=10, patch_radius=3, extent='3d', search_radius_z=4)))


# ---- LDS layout by enumeration (no GPU) -------------------------------------------------------------------------------------------------------
TH, TW = ops.NLM_TILE
GROUPS = (range(0, 32), range(32, 64))          # ds_read_b32, ds_write_b32


def ways(addresses):
    """worst number of distinct words of one lane group on one of the 32 banks"""
    worst = 1
    for g in GROUPS:
        banks = {}
        for lane in g:
            a = addresses[lane]
            if a is not None:
                banks.setdefault(a % 32, set()).add(a)
        worst = max([worst] + [len(v) for v in banks.values()])
    return worst


def lds_check(Rs, Rp):
    """(worst ways of a tap read over every wave, offset and tap; worst ways of a staging store) for the unpadded planes [SH, SW]"""
    halo = Rs + Rp
    SW, SH = TW + 2 * halo, TH + 2 * halo
    read = 1
    for wave in range(TH * TW // 64):
        for dy in range(-Rs, Rs + 1):
            for dx in range(-Rs, Rs + 1):
                for a in range(-Rp, Rp + 1):
                    for b in range(-Rp, Rp + 1):
                        adr = []
                        for lane in range(64):
                            t = wave * 64 + lane
                            lx, ly = t % TW, t // TW
                            adr.append((ly + halo + dy + a) * SW + lx + halo + dx + b)
                        read = max(read, ways(adr))
    store = 1
    for i0 in range(0, SW * SH, 64):          # thread t of a sweep stores word i0 + t: consecutive words
        store = max(store, ways([i0 + lane if i0 + lane < SW * SH else None for lane in range(64)]))
    return read, store, SW, SH


def lds_notes():
    lines = []
    for Rs, Rp in ((5, 1), (1, 1), (3, 2), (10, 3), (7, 2)):
        read, store, SW, SH = lds_check(Rs, Rp)
        lines.append('Rs %2d Rp %d: plane %2d x %2d floats, rows not padded; worst ways of a tap read %d, of a staging store %d'
                     % (Rs, Rp, SH, SW, read, store))
    return lines


# ---- timing -------------------------------------------------------------------------------------------------------------------------------
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


def taps(shape, p):
    """voxel x offset x patch-tap of one call, the offsets as the kernel walks them"""
    S, H, W = shape
    Rs, Rp, Rz = p['search_radius'], p['patch_radius'], p['search_radius_z']
    planes = sum(1 for s in range(S) for dz in range(-Rz, Rz + 1) if 0 <= s + dz < S)
    return (planes * (2 * Rs + 1) ** 2 - S) * H * W * (2 * Rp + 1) ** 2


def other_form(path, x, out, p):
    """a call of mmseg_nlm_denoise of the library at `path` with the arguments ops.nlm_denoise passes"""
    lib = ctypes.CDLL(path)
    fn = lib.mmseg_nlm_denoise
    fn.restype = ctypes.c_int
    fn.argtypes = [ctypes.c_void_p] * 3 + [ctypes.c_double] + [ctypes.c_int] * 6 + [ctypes.c_float, ctypes.c_int, ctypes.c_void_p]
    S, H, W = x.shape

    def call():
        rc = fn(x.data_ptr(), out.data_ptr(), None, p['sigma'], S, H, W, p['search_radius'], p['patch_radius'], p['search_radius_z'], p['h'],
                int(p['noise'] == 'rician'), torch.cuda.current_stream().cuda_stream)
        if rc:
            raise RuntimeError('%s: mmseg_nlm_denoise returned %d' % (path, rc))
    return call


def accuracy_records():
    """the figures the bar of tests/test_volume_denoise.py refers to, for its own cases"""
    from tests import test_volume_denoise as T
    recs = []
    for noise in T.NOISES:
        for name in sorted(T.CASES):
            x, ref = T._case(name), T._ref(name, noise)
            params = dict(T.CASES[name][1], noise=noise, sigma=T.SIGMA)
            if params.get('search_radius_z'):
                params['extent'] = '3d'
            got = ops.nlm_denoise(T._dev(x), params).cpu().numpy().astype(np.float64)
            if noise == 'gaussian':
                err = np.abs(got - ref['out']).max() / np.abs(x).max()
            else:
                err = np.abs(got * got - np.maximum(ref['pre'], 0.0)).max() / np.square(x.astype(np.float64)).max()
            recs.append(dict(kind='parity', case=name, noise=noise, device_error_of_scale=float(err), fp32_restatement_error_of_scale=T._gap(name, noise),
                             bar=T.BAR))
    x, clean = D.phantom((2, 64, 64), seed=0, sigma=T.SIGMA)
    out, sigma = ops.nlm_denoise(T._dev(x), sigma_out=True)
    recs.append(dict(kind='denoises', sigma_true=T.SIGMA, sigma_estimated=float(sigma.item()), sigma_restatement=D.immerkaer(x),
                     rmse_in=D.rmse(x, clean), rmse_out_device=D.rmse(out.cpu().numpy(), clean), rmse_out_restatement=D.rmse(D.nlm(x, D.immerkaer(x))['out'], clean)))
    return recs


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--calls', type=int, default=3)
    ap.add_argument('--host', action='store_true', help='also time the numpy restatement at the defaults on a 2 x 64 x 64 crop')
    ap.add_argument('--other_form', metavar='LIB', help='a library exporting another mmseg_nlm_denoise, timed in alternation with the built one')
    ap.add_argument('--lds', action='store_true', help='print the LDS bank enumeration and stop (needs no GPU)')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'volume_denoise_bench.md'))
    a = ap.parse_args(argv)
    notes = lds_notes()
    if a.lds:
        print('\n'.join(notes))
        return
    if not torch.cuda.is_available():
        raise SystemExit('volume_denoise_bench needs a GPU: a time measured without one says nothing')
    nn.set_default_device('cuda:0')
    dev = 'cuda:0'
    image = D.phantom(SHAPE, seed=1, sigma=SIGMA)[0]
    x = nn.host_to_device(image, dev, np.float32)
    out, out2 = torch.empty_like(x), torch.empty_like(x)
    recs = []

    def note(rec):
        recs.append(rec)
        print(json.dumps(rec), flush=True)

    t = device_ms(lambda: ops.nlm_sigma(x), 20, a.repeats)
    note(dict(kind='sigma', shape=list(SHAPE), ms=round(t[0], 4), ms_range=[round(t[1], 4), round(t[2], 4)], sigma=float(ops.nlm_sigma(x).item()),
              device=torch.cuda.get_device_name(0)))
    for name, given in CONFIGS:
        p = ops.nlm_params(dict(given, sigma=SIGMA))
        n = taps(SHAPE, p)
        calls = a.calls if 'largest' in name else 10 * a.calls
        t = device_ms(lambda: ops.nlm_denoise(x, p, out=out), calls, a.repeats)
        note(dict(kind='denoise', config=name, params=p, ms=round(t[0], 4), ms_range=[round(t[1], 4), round(t[2], 4)], taps=n,
                  tera_taps_per_s=round(n / (t[0] * 1e-3) / 1e12, 3), share_of_fp32_vector_peak=round(3.0 * n / (t[0] * 1e-3) / PEAK_FP32_VECTOR, 4)))
        if not a.other_form:
            continue
        kept, other = (lambda: ops.nlm_denoise(x, p, out=out)), other_form(a.other_form, x, out2, p)
        ms = {'kept': [], 'other': []}
        for _ in range(a.repeats):          # alternating windows of the two forms
            ms['kept'].append(device_ms(kept, calls, 1)[0])
            ms['other'].append(device_ms(other, calls, 1)[0])
        torch.cuda.synchronize()
        diff = float((out - out2).abs().max().item())
        note(dict(kind='forms', config=name, params=p, ms_kept=round(float(np.median(ms['kept'])), 4), ms_other=round(float(np.median(ms['other'])), 4),
                  ms_kept_range=[round(min(ms['kept']), 4), round(max(ms['kept']), 4)], ms_other_range=[round(min(ms['other']), 4), round(max(ms['other']), 4)],
                  largest_output_difference=diff, taps=n))
    bias_out = torch.empty_like(x)
    t = device_ms(lambda: ops.bias_correct(x, SPACINGS, out=bias_out), a.calls, a.repeats)
    note(dict(kind='bias', what='ops.bias_correct at its defaults on the same volume', ms=round(t[0], 3)))
    if a.host:
        crop = np.ascontiguousarray(image[:2, 96:160, 96:160])
        t0 = time.perf_counter()
        ref = D.nlm(crop, SIGMA, dtype=np.float32)
        host_s = time.perf_counter() - t0
        p = ops.nlm_params(dict(sigma=SIGMA))
        note(dict(kind='host', what='numpy restatement (fp32) at the defaults on a 2 x 64 x 64 crop', s=round(host_s, 3),
                  tera_taps_per_s=round(taps(crop.shape, p) / host_s / 1e12, 6),
                  largest_difference_from_device=float(np.abs(ops.nlm_denoise(nn.host_to_device(crop, dev, np.float32), p).cpu().numpy() - ref['out']).max())))
    for rec in accuracy_records():
        note(rec)
    with open(a.out, 'w') as fh:
        fh.write('# Non-local means denoising: device time and the figures behind the tests\' bar\n\n')
        fh.write('Written by `tools/volume_denoise_bench.py%s%s`; see its docstring for what each record is.  One %s.  No speed target is set.\n\n'
                 % (' --host' if a.host else '', ' --other_form LIB' if a.other_form else '', torch.cuda.get_device_name(0)))
        fh.write('```\n')
        for rec in recs:
            fh.write(json.dumps(rec) + '\n')
        fh.write('```\n\nLDS layout by enumeration (`--lds`, no GPU):\n\n```\n%s\n```\n' % '\n'.join(notes))
    print('wrote', a.out)


if __name__ == '__main__':
    main()
