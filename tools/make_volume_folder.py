#!/usr/bin/env python
"""Write a folder of volumes in the format of multimodal_segmentation_amd/loaders/volume_folder.py from the synthetic generator
(loaders/synthetic.py) -- the fixture of tests/test_volume_loader.py and a worked example of the format for users who export their
own data ("Volume folders").

Every (volume, modality) gets its own slice size, pixel spacing and slice count, like acquisitions of different scanners: the raw
extent is drawn so that the resampled slice is sometimes larger than input_shape (cropped) and sometimes smaller (edge-padded).
Images are int16 "scanner" intensities, labels uint8 grey values (label_values; 0 is background).  Modalities of a volume show the
same anatomy; the later modalities carry extra leading / trailing slices, and the manifest's `slices` ranges select the matching
ones.

    python tools/make_volume_folder.py OUT [--volumes 4] [--size 64] [--slices 6] [--modalities t1 t2] [--masks 4] [--seed 0]
                                       [--raw_size LO HI] [--name chaos] [--unlabelled] [--slice_spacing LO HI] [--hot_voxels N]
                                       [--bias_field STRENGTH] [--rician_noise STD] [--misalign PIXELS [--misalign_aligned]]
    python experiment.py --config dafnet_config_chaos --split 0 --data_folder OUT
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

from multimodal_segmentation_amd.loaders import synthetic

TARGET_RESOLUTION = (1.89, 1.89)          # the CHAOS loader's common pixel spacing (chaos.py:331)


def label_values(num_masks):
    """evenly spaced grey values as in the CHAOS ground-truth PNGs: 63, 126, 189, 252 for four organs"""
    step = 252 // num_masks
    return [step * (k + 1) for k in range(num_masks)]


def make_volume(rng, anatomy_seed, mod, S, H, W, values):
    """S slices [S,H,W]: int16 image and uint8 grey-value label; slice i of every modality draws its organs from the same seed"""
    K = len(values)
    image = np.zeros((S, H, W), np.int16)
    label = np.zeros((S, H, W), np.uint8)
    weights = np.linspace(0.4, 1.0, K)
    sign = np.where(np.arange(K) % 2 == 0, 1.0, -1.0)
    for i in range(S):
        m = synthetic.ellipse_masks(np.random.RandomState(anatomy_seed + i), H, W, K)
        organ = (m * (weights * (1.0 if mod == 0 else (-1.0 if mod == 1 else sign)))[None, None]).sum(-1)
        img = 0.5 * synthetic.smooth_field(rng, H, W, max(H / 32.0, 1.0)) + organ
        image[i] = np.round((img - img.min()) / (img.max() - img.min() + 1e-12) * rng.uniform(800, 1600))
        label[i] = (m * np.asarray(values, np.float32)[None, None]).sum(-1).astype(np.uint8)
    return image, label


def add_hot_voxels(rng, image, count):
    """image [S,H,W] int16 times a gain from [0.5, 2], then `count` voxels per slice at 8 .. 16 times the slice's maximum (within int16)"""
    out = image.astype(np.float64) * rng.uniform(0.5, 2.0)
    S, H, W = out.shape
    for i in range(S):
        top = out[i].max()
        for _ in range(count):
            out[i, rng.randint(0, H), rng.randint(0, W)] = min(top * rng.uniform(8.0, 16.0), 32767.0)
    return np.round(out).astype(np.int16)


def add_bias_field(rng, image, strength, res, spacing):
    """image [S,H,W] int16 lifted by 10 % of its maximum (tissue must be brighter than air for the shading to show) and multiplied by
    exp(f), f a smooth field in mm of amplitude `strength` (a plane plus a bowl, drawn per file): coil shading, what the `bias_field`
    block of dataset.json removes.  Rounded back to int16."""
    S, H, W = image.shape
    z, y, x = np.meshgrid((np.arange(S) - (S - 1) / 2.0) * (spacing or 1.0), (np.arange(H) - (H - 1) / 2.0) * res[0],
                          (np.arange(W) - (W - 1) / 2.0) * res[1], indexing='ij')
    a = rng.uniform(-1.0, 1.0, 5)
    half = max(H * res[0], W * res[1]) / 2.0
    f = (a[0] * y + a[1] * x + a[2] * z) / half + a[3] * (y * y - x * x) / half ** 2 + a[4] * (y * y + x * x) / half ** 2
    f = strength * f / max(np.abs(f).max(), 1e-12)
    out = (image.astype(np.float64) + 0.1 * image.max()) * np.exp(f)
    return np.round(np.minimum(out, 32767.0)).astype(np.int16)


def add_rician_noise(rng, image, std):
    """image [S,H,W] int16 through a Rician channel: sqrt((image + n1)^2 + n2^2) with n1, n2 ~ N(0, std^2), the magnitude of a complex
    signal with Gaussian noise in both parts -- what the `denoise` block of dataset.json removes.  Rounded back to int16."""
    clean = image.astype(np.float64)
    n1, n2 = rng.normal(0.0, std, clean.shape), rng.normal(0.0, std, clean.shape)
    return np.round(np.minimum(np.sqrt((clean + n1) ** 2 + n2 ** 2), 32767.0)).astype(np.int16)


def default_splits(ids):
    """70 / 15 / 15 like CHAOS's 14 / 3 / 3 (at least one volume each), rotated for a second split"""
    n = len(ids)
    n_val = n_test = max(1, int(round(0.15 * n)))
    out = []
    for shift in (0, n_val):
        r = ids[shift:] + ids[:shift]
        out.append({'training': r[:n - n_val - n_test], 'validation': r[n - n_val - n_test:n - n_test], 'test': r[n - n_test:]})
    return out


def misaligned_volume(rng, align_rng, anatomy_seed, modalities, slices, size, pixels, values, aligned):
    """One volume whose modalities are windows of ONE canvas drawn at TARGET_RESOLUTION (a raw pixel is a resampled pixel): per modality
    (image, label, leading extra slices) and, per later modality, the truth (dz, dy, dx) in the convention of the alignment rule
    (include/mmseg_hip.h) against the first: its slice i + dz and its centre window moved by (dy, dx) show what slice i and the centre
    window of the first modality show.  A window's extent is size + 0..8 per axis; the first modality's is centred on the canvas, a later
    one's is cut `offset` pixels off centre, offset from [-pixels, pixels] per axis (so |dy|, |dx| <= pixels), and carries 0..2 extra
    leading / trailing slices (dz = the leading ones).  aligned: the same draws, but every offset is 0."""
    margin = pixels + 4
    canvas = size + 2 * pixels + 12
    out, truth = [], []
    for mod in range(len(modalities)):
        H, W = (size + int(align_rng.randint(0, 9)) for _ in range(2))
        off = (0, 0) if mod == 0 else tuple(int(align_rng.randint(-pixels, pixels + 1)) for _ in range(2))
        before, after = (0, 0) if mod == 0 else (int(align_rng.randint(0, 3)), int(align_rng.randint(0, 3)))
        if aligned:
            off = (0, 0)
        image, label = make_volume(rng, anatomy_seed - before, mod, before + slices + after, canvas, canvas, values)
        y0, x0 = (margin - (n - size + 1) // 2 + o for n, o in zip((H, W), off))          # centre_start(n, size) = (n - size + 1) // 2
        out.append((image[:, y0:y0 + H, x0:x0 + W].copy(), label[:, y0:y0 + H, x0:x0 + W].copy(), before))
        if mod:
            truth.append((before, -off[0], -off[1]))
    return out, truth


def write_folder(out, volumes=4, size=64, slices=6, modalities=('t1', 't2'), masks=4, seed=0, raw_size=None, name='chaos', unlabelled=False,
                 slice_spacing=None, hot_voxels=0, bias_field=0.0, rician_noise=0.0, misalign=None, misalign_aligned=False):
    """unlabelled: the files carry no `label` array (scans to be segmented: experiment.py --predict_folder); everything else, the random
    draws included, is as without it.  slice_spacing = (LO, HI): every file also stores `slice_spacing`, mm between its slices, drawn
    from [LO, HI] by a generator of its own, so that every other draw is as without it.  hot_voxels = N > 0: every file is multiplied
    by a gain of its own from [0.5, 2] (scanners differ) and every slice gets N voxels of 8 to 16 times its maximum (vessels, fold-over
    artefacts): what the `intensity` modes of the loader are for.  These draws too come from a generator of their own.  bias_field =
    STRENGTH > 0: every file carries a smooth multiplicative field exp(f), |f| <= STRENGTH (add_bias_field; a generator of its own), and the
    manifest gets "bias_field": {"mode": "n3"} so that the loader removes it.  rician_noise = STD > 0: every file, after all of the above,
    passes through a Rician channel of that standard deviation in grey values (add_rician_noise; a generator of its own), and the
    manifest gets "denoise": {"mode": "nlm", "sigma": STD} so that the loader removes it.  misalign = PIXELS >= 0: the modalities of a
    volume are windows of one canvas at TARGET_RESOLUTION, cut off centre by up to PIXELS and with extra slices at both ends
    (misaligned_volume; the new draws come from a generator of their own), the manifest states NO `slices` but "align": {"mode": "mi",
    "max_shift_mm": PIXELS pixels in mm, "max_slices": 3, "bins": 16}, and the truth goes to misalignment.json ({volume: {modality: [dz, dy,
    dx]}}).  misalign_aligned: the same canvases with every offset 0, `slices` stated and no "align" key: what alignment should arrive at."""
    if volumes < 3:
        raise ValueError('need at least 3 volumes (training, validation, test)')
    os.makedirs(out, exist_ok=True)
    rng = np.random.RandomState(seed)
    spacing_rng = np.random.RandomState(seed + 1000003)
    if slice_spacing is not None and not 0 < slice_spacing[0] <= slice_spacing[1]:
        raise ValueError('slice_spacing must be 0 < LO <= HI, got %r' % (slice_spacing,))
    if hot_voxels < 0:
        raise ValueError('hot_voxels must be 0 or more, got %r' % (hot_voxels,))
    hot_rng = np.random.RandomState(seed + 2000003)
    if bias_field < 0:
        raise ValueError('bias_field must be 0 or more, got %r' % (bias_field,))
    bias_rng = np.random.RandomState(seed + 3000003)
    if not rician_noise >= 0:
        raise ValueError('rician_noise must be 0 or more, got %r' % (rician_noise,))
    noise_rng = np.random.RandomState(seed + 4000003)
    if misalign is not None and (misalign < 0 or raw_size is not None or slice_spacing is not None or hot_voxels or bias_field or rician_noise):
        raise ValueError('misalign must be 0 or more pixels and goes without raw_size, slice_spacing, hot_voxels, bias_field and '
                         'rician_noise, got %r' % (misalign,))
    align_rng = np.random.RandomState(seed + 5000003)
    truths = {}
    values = label_values(masks)
    ids = list(range(1, volumes + 1))
    manifest = dict(name=name, modalities=list(modalities), label_values=values, target_resolution=list(TARGET_RESOLUTION),
                    input_shape=[size, size, 1], splits=default_splits(ids), volumes={})
    for v in ids:
        entry = {}
        if misalign is not None:
            windows, truth = misaligned_volume(rng, align_rng, 1000 * (seed + 1) * v, modalities, slices, size, misalign, values, misalign_aligned)
            truths[str(v)] = {mod_name: list(t) for mod_name, t in zip(modalities[1:], truth)}
            for mod_name, (image, label, before) in zip(modalities, windows):
                fname = 'vol%02d_%s.npz' % (v, mod_name)
                arrays = dict(image=image, resolution=np.asarray(TARGET_RESOLUTION, np.float64))
                if not unlabelled:
                    arrays['label'] = label
                np.savez_compressed(os.path.join(out, fname), **arrays)
                entry[mod_name] = {'file': fname}
                if misalign_aligned and image.shape[0] != slices:
                    entry[mod_name]['slices'] = [[before, before + slices]]
            manifest['volumes'][str(v)] = entry
            continue
        for mod, mod_name in enumerate(modalities):
            res = rng.uniform(1.2, 2.4, size=2)
            if raw_size is None:      # field of view of 0.85 .. 1.2 input extents: crop on some axes, pad on others
                H, W = [max(8, int(round(size * rng.uniform(0.85, 1.2) * TARGET_RESOLUTION[a] / res[a]))) for a in range(2)]
            else:
                H, W = [int(rng.randint(raw_size[0], raw_size[1] + 1)) for _ in range(2)]
            before, after = (0, 0) if mod == 0 else (int(rng.randint(0, 3)), int(rng.randint(0, 3)))
            image, label = make_volume(rng, 1000 * (seed + 1) * v - before, mod, before + slices + after, H, W, values)
            if hot_voxels:
                image = add_hot_voxels(hot_rng, image, hot_voxels)
            fname = 'vol%02d_%s.npz' % (v, mod_name)
            arrays = dict(image=image, resolution=res.astype(np.float64)) if unlabelled else dict(image=image, label=label,
                                                                                                   resolution=res.astype(np.float64))
            spacing = None if slice_spacing is None else float(spacing_rng.uniform(slice_spacing[0], slice_spacing[1]))
            if bias_field:
                arrays['image'] = add_bias_field(bias_rng, image, bias_field, res, spacing)
            if rician_noise:
                arrays['image'] = add_rician_noise(noise_rng, arrays['image'], rician_noise)
            if spacing is not None:
                arrays['slice_spacing'] = np.float64(spacing)
            np.savez_compressed(os.path.join(out, fname), **arrays)
            entry[mod_name] = {'file': fname}
            if before or after:
                entry[mod_name]['slices'] = [[before, before + slices]]
        manifest['volumes'][str(v)] = entry
    if bias_field:
        manifest['bias_field'] = {'mode': 'n3'}
    if rician_noise:
        manifest['denoise'] = {'mode': 'nlm', 'sigma': float(rician_noise)}
    if misalign is not None:
        if not misalign_aligned:
            manifest['align'] = {'mode': 'mi', 'max_shift_mm': (misalign + 0.5) * min(TARGET_RESOLUTION), 'max_slices': 3,
                                 'bins': 16}
        with open(os.path.join(out, 'misalignment.json'), 'w') as f:
            json.dump(truths, f, indent=1)
    with open(os.path.join(out, 'dataset.json'), 'w') as f:
        json.dump(manifest, f, indent=1)
    return manifest


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('out')
    ap.add_argument('--volumes', type=int, default=4)
    ap.add_argument('--size', type=int, default=64, help='input_shape is size x size')
    ap.add_argument('--slices', type=int, default=6, help='paired slices per volume')
    ap.add_argument('--modalities', nargs='+', default=['t1', 't2'])
    ap.add_argument('--masks', type=int, default=4)
    ap.add_argument('--seed', type=int, default=0)
    ap.add_argument('--raw_size', type=int, nargs=2, metavar=('LO', 'HI'), help='draw the raw slice extents from [LO, HI]')
    ap.add_argument('--name', default='chaos')
    ap.add_argument('--unlabelled', action='store_true', help='write files without a label array (a folder to predict on)')
    ap.add_argument('--slice_spacing', type=float, nargs=2, metavar=('LO', 'HI'),
                    help='store a slice spacing in mm per file, drawn from [LO, HI] (what the scores in mm need)')
    ap.add_argument('--hot_voxels', type=int, default=0, metavar='N',
                    help='a gain per file and N very bright voxels per slice (what the intensity modes of dataset.json are for)')
    ap.add_argument('--bias_field', type=float, default=0.0, metavar='STRENGTH',
                    help='a smooth multiplicative field exp(f), |f| <= STRENGTH, per file, and "bias_field": {"mode": "n3"} in dataset.json '
                         '(what the bias-field correction of the loader is for)')
    ap.add_argument('--rician_noise', type=float, default=0.0, metavar='STD',
                    help='pass every file through a Rician channel of this standard deviation in grey values, and "denoise": {"mode": "nlm", '
                         '"sigma": STD} in dataset.json (what the denoising of the loader is for)')
    ap.add_argument('--misalign', type=int, default=None, metavar='PIXELS',
                    help='cut the modalities of a volume from one canvas, up to PIXELS off centre and with extra slices, state no "slices" '
                         'but "align": {"mode": "mi"} in dataset.json, and write the truth to misalignment.json (what the alignment of the '
                         'loader is for)')
    ap.add_argument('--misalign_aligned', action='store_true', help='with --misalign: the same canvases, offsets 0, "slices" stated, no "align"')
    a = ap.parse_args(argv)
    m = write_folder(a.out, a.volumes, a.size, a.slices, a.modalities, a.masks, a.seed, a.raw_size, a.name, a.unlabelled, a.slice_spacing,
                     a.hot_voxels, a.bias_field, a.rician_noise, a.misalign, a.misalign_aligned)
    print('wrote %d volumes x %d modalities to %s' % (len(m['volumes']), len(m['modalities']), a.out))


if __name__ == '__main__':
    main()
