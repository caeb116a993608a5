"""Percentile-window and landmark intensity normalisation of volumes read from a folder: csrc/preprocess.hip
(mmseg_preprocess_quantiles*, mmseg_preprocess_image_map), ops.preprocess_quantiles / preprocess_images(knots=...), the `intensity`
block of loaders/volume_folder.py, tools/fit_intensity_landmarks.py and the `--intensity_*` options of experiment.py, against the
numpy restatement in tests/volume_intensity_ref.py (the definition is in include/mmseg_hip.h)."""
import importlib.util
import json
import logging
import os

import numpy as np
import pytest
import torch

from multimodal_segmentation_amd import loaders, nn
from multimodal_segmentation_amd.loaders import loader_factory
from tests import helpers as Hh
from tests import volume_intensity_ref as I
from tests import volume_loader_ref as R

TARGET = (1.89, 1.89)

# the geometries of the op-level scenarios of tests/test_volume_loader.py: (H, W, resolution) per modality
GEOMETRIES = {
    'up,down': [(41, 41, (2.5, 2.5)), (91, 91, (1.2, 1.2))],
    'aniso,nonsquare,oddcrop+pad': [(61, 59, (1.3, 2.2)), (51, 37, (1.7, 1.7)), (45, 40, (1.89, 1.5))],
    'pad-both,constant': [(29, 34, (1.6, 2.0)), (79, 70, (1.4, 1.5)), (50, 44, (1.89, 1.89))],
}

SCALE11 = [-1.0, -0.8, -0.65, -0.5, -0.3, -0.1, 0.1, 0.35, 0.6, 0.8, 1.0]

# Image-level cases: raw (H, W) -> resampled -> out with the index maps crop_pad_map gives, the two quirky ones among them: rows
# (3, 39, 0) (an odd surplus: 39 kept, the last repeated) and rows (0, 25, 11) (padding by an odd amount)
MAP_CASES = {
    'window-volume': dict(raw=(45, 40), resampled=(45, 32), out=(40, 40), rows=(3, 39, 0), cols=(0, 32, 4), per_volume=True,
                          percentiles=I.WINDOW_PERCENTILES, y=(-1.0, 1.0), zero_slice=None, air_rows=0),
    'window-slice': dict(raw=(29, 34), resampled=(25, 36), out=(48, 48), rows=(0, 25, 11), cols=(0, 36, 6), per_volume=False,
                         percentiles=I.WINDOW_PERCENTILES, y=(-1.0, 1.0), zero_slice=1, air_rows=0),
    # 12 of 45 rows are air (the rows are not resampled, so they stay exact zeros below positive tissue): the landmarks at 1, 10 and
    # 20 % are all 0
    'landmarks': dict(raw=(45, 40), resampled=(45, 32), out=(40, 40), rows=(3, 39, 0), cols=(0, 32, 4), per_volume=True,
                      percentiles=I.LANDMARK_PERCENTILES, y=SCALE11, zero_slice=None, air_rows=12),
}


def _raw_image(rng, S, H, W, positive=False):
    """the generator of tests/test_volume_loader.py without its labels: smooth texture of +-1000 and a bright and a dark blob of
    +-3000, which spread the percentiles of a slice widely"""
    yy, xx = np.mgrid[:H, :W]
    sig = 0.05 * min(H, W)
    image = np.zeros((S, H, W), np.float64)
    for s in range(S):
        f = 1000.0 * Hh.smooth_field(rng, 1, H, W, sigma=3.0)[0, ..., 0]
        for sign, cy, cx in ((3000.0, 0.45 + 0.02 * s, 0.45), (-3000.0, 0.56, 0.55 - 0.02 * s)):
            f = f + sign * np.exp(-((yy - cy * H) ** 2 + (xx - cx * W) ** 2) / (2 * sig * sig))
        image[s] = f - f.min() + 50.0 if positive else f
    return image.astype(np.float32)


def _case_data(name, S=3):
    case = MAP_CASES[name]
    H, W = case['raw']
    image = _raw_image(np.random.RandomState(len(name)), S, H, W, positive=case['air_rows'] > 0)
    if case['zero_slice'] is not None:
        image[case['zero_slice']] = 0.0
    image[:, :case['air_rows']] = 0.0
    return case, image


def _case_want(case, image, dtype):
    RH, RW = case['resampled']
    fr = I.frames(image, RH, RW, dtype)
    rk = I.ranks((image.shape[0] if case['per_volume'] else 1) * RH * RW, case['percentiles'])
    mapped, x = I.normalise(fr, rk, case['y'], case['per_volume'])
    return fr, x, mapped, rk


@pytest.fixture(autouse=True)
def _clean_registries():
    saved = dict(loaders.data_conf), dict(loaders.intensity_conf)
    yield
    for registry, old in zip((loaders.data_conf, loaders.intensity_conf), saved):
        registry.clear()
        registry.update(old)


def _install(monkeypatch):
    from tests import cpu_backend as cb
    for table in (R.STANDINS, I.STANDINS):
        for name, fn in table.items():
            monkeypatch.setitem(cb._TABLE, name, fn)
    monkeypatch.setattr(I, 'CALLS', [])
    cb.install()
    nn.set_default_device('cpu')
    return cb


@pytest.fixture
def standin(monkeypatch):
    """the CPU stand-in of the C ABI with the stand-ins of the preprocessing entry points, old and new, added to its table"""
    cb = _install(monkeypatch)
    yield cb
    cb.uninstall()


@pytest.fixture(params=[pytest.param('cpu', id='cpu-standin'), pytest.param('cuda', marks=pytest.mark.gpu, id='mi355x')])
def device(request, monkeypatch):
    if request.param == 'cpu':
        cb = _install(monkeypatch)
        yield 'cpu'
        cb.uninstall()
    else:
        nn.set_default_device('cuda:0')
        yield 'cuda'


@pytest.fixture
def folder(tmp_path):
    out = str(tmp_path / 'volumes')
    R.tool().write_folder(out, volumes=4, size=64, slices=4, seed=3)
    return out


def _set_intensity(folder, block):
    path = os.path.join(folder, 'dataset.json')
    manifest = json.load(open(path))
    if block is None:
        manifest.pop('intensity', None)
    else:
        manifest['intensity'] = block
    json.dump(manifest, open(path, 'w'))


def _fit_tool():
    spec = importlib.util.spec_from_file_location('fit_intensity_landmarks', os.path.join(R.ROOT, 'tools', 'fit_intensity_landmarks.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


# ---- the definition and the test inputs (no GPU) ------------------------------------------------------------------------------------
def test_rank_rule_is_numpy_lower():
    """floor((N - 1) * (q / 100)) in fp64 selects what np.percentile(method='lower') selects"""
    from multimodal_segmentation_amd.loaders.volume_folder import quantile_ranks
    rng = np.random.RandomState(0)
    for n in (1, 2, 3, 7, 100, 2691):
        values = rng.permutation(n).astype(np.float64)          # distinct: the value identifies the rank
        for q in (0, 0.5, 1, 25, 50, 99, 99.5, 100):
            [rank] = quantile_ranks(n, [q])
            assert [rank] == I.ranks(n, [q]) and 0 <= rank <= n - 1
            assert np.sort(values)[rank] == np.percentile(values, q, method='lower'), (n, q)


@pytest.mark.parametrize('name', sorted(MAP_CASES))
def test_image_cases_are_decidable(name):
    """the restatement evaluated in fp32 and in fp64 agrees within 5e-5 on every image-level case: the condition under which the
    2e-4 bar of the GPU test tests the kernel and not the inputs"""
    case, image = _case_data(name)
    _, x32, m32, _ = _case_want(case, image, np.float32)
    _, x64, m64, _ = _case_want(case, image, np.float64)
    gap = float(np.abs(m32.astype(np.float64) - m64).max())
    print('%s: fp32 against fp64 restatement %.3e, knots %s' % (name, gap, x64[0].tolist()))
    assert m32.dtype == np.float32 and gap <= 5e-5
    assert m64.min() == -1.0 and m64.max() == 1.0
    if name == 'landmarks':
        assert x64[0, 0] == x64[0, 1] == x64[0, 2] == 0.0 < x64[0, 3]
    if case['zero_slice'] is not None:
        assert np.all(m64[case['zero_slice']] == -1.0)


# ---- selection ------------------------------------------------------------------------------------------------------------------------
def _exact_volumes(rng, H, W):
    """name -> [3,H,W] fp32, every slice from another distribution; normal numbers or zero only"""
    n = H * W
    low = np.float32(1000.0).view(np.uint32) + rng.randint(0, 256, size=n).astype(np.uint32)      # differ in the last key digit only
    low = low.view(np.float32)
    zeros = np.where(rng.rand(n) < 0.6, 0.0, rng.randn(n) * 30.0)
    return {
        'mixed signs': np.stack([rng.randn(n) * 1000.0, rng.uniform(-1.0, 1.0, n) * 1e-3, rng.randn(n) + 5e4]),
        '+-0, 60 % zeros, constant': np.stack([np.where(rng.rand(n) < 0.5, -0.0, 0.0), zeros, np.full(n, 3.5)]),
        'uint8-like, last digit, negative last digit': np.stack([rng.randint(0, 7, size=n) * 37.0, low, -low]),
    }


def _exact_ranks(n):
    sixteen = sorted(min(max(r, 0), n - 1) for r in (0, 0, 1, n // 7, n // 7 + 1, n // 3, n // 3, n // 2 - 1, n // 2, n // 2 + 1,
                                                     (2 * n) // 3, (7 * n) // 8, n - 3, n - 2, n - 1, n - 1))
    return [[0, n - 1], sixteen]


@pytest.mark.gpu
@pytest.mark.parametrize('per_volume', [False, True], ids=['slice', 'volume'])
@pytest.mark.parametrize('frame', [(1, 1), (5, 7), (37, 41), (131, 127)], ids=lambda f: '%dx%d' % f)
def test_selection_is_exact(frame, per_volume):
    """identity geometry, where the resampling returns the raw value (up to the sign of a zero: 1 * (-0) + 0 * a is +0 unless a is
    negative, so a raw -0 may enter the population as +0; np.sort does not tell the two apart either): the knots are
    np.sort(segment)[ranks] bit for bit, for K = 2 and K = 16 with repeated and adjacent ranks, and two runs are bitwise equal"""
    from multimodal_segmentation_amd import ops
    H, W = frame
    rng = np.random.RandomState(H * W)
    for name, vol in _exact_volumes(rng, H, W).items():
        vol = vol.astype(np.float32).reshape(3, H, W)
        assert np.all((vol == 0) | (np.abs(vol) >= np.finfo(np.float32).tiny))
        x = nn.host_to_device(vol, 'cuda:0', np.float32)
        segments = vol.reshape(1, -1) if per_volume else vol.reshape(3, -1)
        for rk in _exact_ranks(segments.shape[1]):
            got = ops.preprocess_quantiles(x, (H, W), rk, per_volume)
            again = ops.preprocess_quantiles(x, (H, W), rk, per_volume)
            assert torch.equal(got.view(torch.int32), again.view(torch.int32))
            got = got.cpu().numpy()
            assert got.shape == (segments.shape[0], len(rk))
            for g, seg in enumerate(segments):
                assert np.array_equal(got[g], np.sort(seg)[rk]), (name, g, rk)
                assert np.array_equal(_bits(got[g] + np.float32(0)), _bits(np.sort(seg)[rk] + np.float32(0))), (name, g, rk)


@pytest.mark.gpu
@pytest.mark.parametrize('name', sorted(GEOMETRIES))
def test_selection_under_resampling(name):
    """|x_got - x_want| <= 2^-20 * max|raw| against the fp64 restatement: order statistics are 1-Lipschitz in the sup norm, and the
    fp32 interpolation makes at most nine roundings of quantities <= max|raw| and three weight roundings, each multiplying a
    difference <= 2 * max|raw|: 15 * 2^-24 < 2^-20"""
    from multimodal_segmentation_amd import ops
    rng = np.random.RandomState(len(name))
    worst = 0.0
    for H, W, res in GEOMETRIES[name]:
        image = _raw_image(rng, 3, H, W)
        RH, RW = R.out_extent(H, res[0], TARGET[0]), R.out_extent(W, res[1], TARGET[1])
        x = nn.host_to_device(image, 'cuda:0', np.float32)
        fr = I.frames(image, RH, RW, np.float64)
        bound = 2.0 ** -20 * float(np.abs(image).max())
        for per_volume in (False, True):
            n = (3 if per_volume else 1) * RH * RW
            for q in (I.WINDOW_PERCENTILES, I.LANDMARK_PERCENTILES):
                rk = I.ranks(n, q)
                got = ops.preprocess_quantiles(x, (RH, RW), rk, per_volume).cpu().numpy().astype(np.float64)
                err = float(np.abs(got - I.knots(fr, rk, per_volume)).max())
                worst = max(worst, err / bound)
                assert err <= bound, (name, H, W, per_volume, q, err, bound)
    print('%s: largest knot error %.3f of the bound 2^-20 * max|raw|' % (name, worst))


# ---- the map --------------------------------------------------------------------------------------------------------------------------
def _run_map(image, case, rows, cols, out_hw, C=3, ch=1):
    from multimodal_segmentation_amd import ops
    S = image.shape[0]
    RH, RW = case['resampled']
    x = nn.host_to_device(image, 'cuda:0', np.float32)
    rk = I.ranks((S if case['per_volume'] else 1) * RH * RW, case['percentiles'])
    knots = ops.preprocess_quantiles(x, (RH, RW), rk, case['per_volume'])
    y = nn.host_to_device(np.asarray(case['y']), 'cuda:0', np.float32)
    out = torch.full((S, out_hw[0], out_hw[1], C), float('nan'), device='cuda:0')
    ops.preprocess_images(x, out, (RH, RW), rows, cols, ch, knots=(knots, y))
    return out, knots


@pytest.mark.gpu
@pytest.mark.parametrize('name', sorted(MAP_CASES))
def test_map_matches_restatement(name):
    """Within 2e-4 of the fp64 restatement (the op-level bar; the outputs span [-1, 1]); inside [-1, 1]; only the addressed channel
    of a NaN-filled container is written, all of it; two runs bitwise equal; exact ends: a pixel below x_0 by more than the rounding
    of the resampling (twice the knot bound of test_selection_under_resampling: value and knot) is exactly y_0, likewise above
    x_{K-1}, and over the whole frame at least r_0 + 1 pixels are exactly y_0 and at least N - r_{K-1} exactly y_{K-1} per segment."""
    case, image = _case_data(name)
    S = image.shape[0]
    RH, RW = case['resampled']
    fr, x64, m64, rk = _case_want(case, image, np.float64)
    out, knots = _run_map(image, case, case['rows'], case['cols'], case['out'])
    out2, _ = _run_map(image, case, case['rows'], case['cols'], case['out'])
    assert torch.equal(out.view(torch.int32), out2.view(torch.int32))
    out = out.cpu().numpy()
    assert np.isnan(out[..., 0]).all() and np.isnan(out[..., 2]).all() and np.isfinite(out[..., 1]).all()
    got = out[..., 1]
    want = I.crop_pad(m64, case['rows'], case['cols'], case['out'])
    err = float(np.abs(got - want).max() / np.abs(want).max())
    tol = 2.0 * 2.0 ** -20 * float(np.abs(image).max())
    v = I.crop_pad(fr, case['rows'], case['cols'], case['out'])
    xs = x64[[0] * S] if case['per_volume'] else x64
    below, above = v < xs[:, :1, None] - tol, v > xs[:, -1:, None] + tol
    below |= (v == 0.0) & (xs[:, :1, None] == 0.0)          # air under a knot of 0: zeros resample to exact zeros in any precision
    near = int(np.count_nonzero((np.abs(v - xs[:, :1, None]) <= tol) | (np.abs(v - xs[:, -1:, None]) <= tol)))
    print('%s: error %.3e of the maximum, %d pixels at y_0, %d at y_K-1, %d within the rounding of a window end'
          % (name, err, np.count_nonzero(below), np.count_nonzero(above), near))
    assert err <= 2e-4
    assert got.min() >= -1.0 and got.max() <= 1.0
    assert below.any() and np.all(got[below] == np.float32(case['y'][0]))
    assert above.any() and np.all(got[above] == np.float32(case['y'][-1]))
    if case['zero_slice'] is not None:
        assert np.all(got[case['zero_slice']] == -1.0)
    # the whole resampled frame, uncropped: the counts that the ranks guarantee
    full, _ = _run_map(image, case, (0, RH, 0), (0, RW, 0), (RH, RW), C=1, ch=0)
    full = full.cpu().numpy()[..., 0]
    segments = full.reshape(1, -1) if case['per_volume'] else full.reshape(S, -1)
    for seg, xg in zip(segments, knots.cpu().numpy()):
        assert np.count_nonzero(seg == np.float32(case['y'][0])) >= rk[0] + 1
        if xg[0] < xg[-1]:          # a constant segment is y_0 everywhere
            assert np.count_nonzero(seg == np.float32(case['y'][-1])) >= seg.size - rk[-1]


@pytest.mark.gpu
@pytest.mark.parametrize('per_volume', [False, True], ids=['slice', 'volume'])
def test_constant_segment_maps_to_minus_one(per_volume):
    case = dict(resampled=(9, 11), per_volume=per_volume, percentiles=I.WINDOW_PERCENTILES, y=(-1.0, 1.0))
    image = np.full((3, 9, 11), 7.0, np.float32)          # identity geometry: interpolating a constant other than 0 is exact there only
    out, knots = _run_map(image, case, (0, 9, 0), (0, 11, 0), (9, 11), C=1, ch=0)
    assert np.all(knots.cpu().numpy() == 7.0) and np.all(out.cpu().numpy() == -1.0)


# ---- what the feature is for: one hot voxel does not move the scale ---------------------------------------------------------------------
ROBUST = dict(raw=(81, 81), resampled=(107, 107), res=(2.5, 2.5), S=3)


def _robust_pair():
    """a volume whose brightest region is a broad smooth bump per slice, and a copy with the voxel at the top of every bump set to
    50 x the volume's maximum.  The bump is broad enough for the bilinear footprint of that voxel (at most 3 x 3 resampled pixels at
    this scale) to lie among the 0.5 % of the volume above the upper knot, so the knots of the pair are the same values."""
    H, W = ROBUST['raw']
    rng = np.random.RandomState(7)
    yy, xx = np.mgrid[:H, :W]
    image = np.zeros((ROBUST['S'], H, W), np.float64)
    hot = []
    for s in range(ROBUST['S']):
        cy, cx = 30 + 7 * s, 45 - 6 * s
        image[s] = 100.0 * Hh.smooth_field(rng, 1, H, W, sigma=3.0)[0, ..., 0] + 3000.0 * np.exp(-((yy - cy) ** 2 + (xx - cx) ** 2) / (2 * 8.0 ** 2))
        hot.append(np.unravel_index(np.argmax(image[s]), (H, W)))
    image = image.astype(np.float32)
    spiked = image.copy()
    for s, (r, c) in enumerate(hot):
        spiked[s, r, c] = 50.0 * image.max()
    cap = 4 * ROBUST['S'] * int(np.ceil(ROBUST['resampled'][0] / H)) * int(np.ceil(ROBUST['resampled'][1] / W))
    return image, spiked, cap


def _minmax64(fr):
    lo, hi = fr.min(axis=(1, 2), keepdims=True), fr.max(axis=(1, 2), keepdims=True)
    return 2.0 * (fr - lo) / (hi - lo) - 1.0


def test_restatement_is_robust_to_a_hot_voxel():
    image, spiked, cap = _robust_pair()
    RH, RW = ROBUST['resampled']
    assert (RH, RW) == (R.out_extent(81, 2.5, TARGET[0]),) * 2
    rk = I.ranks(image.shape[0] * RH * RW, I.WINDOW_PERCENTILES)
    fa, fb = I.frames(image, RH, RW), I.frames(spiked, RH, RW)
    (a, xa), (b, xb) = I.normalise(fa, rk, (-1.0, 1.0), True), I.normalise(fb, rk, (-1.0, 1.0), True)
    touched = int(np.count_nonzero(fa != fb))
    differing = int(np.count_nonzero(a != b))
    print('the hot voxels touch %d resampled pixels, %d window outputs differ, cap %d' % (touched, differing, cap))
    assert np.array_equal(xa, xb) and 0 < touched <= cap and differing <= cap
    same = int(np.count_nonzero(_minmax64(fa) == _minmax64(fb)))          # min / max: all but the two extremes of a slice move
    assert same <= 2 * image.shape[0]


@pytest.mark.gpu
def test_window_is_robust_to_a_hot_voxel_and_minmax_is_not():
    """window / volume: the outputs of the pair differ in at most the pixels the bilinear footprints of the hot voxels touch, capped
    at 4 * S * ceil(RH / H) * ceil(RW / W) (here they all lie above the window and stay 1: none differs); min / max: every
    pixel but the two extremes of its slice differs"""
    from multimodal_segmentation_amd import ops
    image, spiked, cap = _robust_pair()
    RH, RW = ROBUST['resampled']
    case = dict(resampled=(RH, RW), per_volume=True, percentiles=I.WINDOW_PERCENTILES, y=(-1.0, 1.0))
    (a, xa), (b, xb) = [_run_map(v, case, (0, RH, 0), (0, RW, 0), (RH, RW), C=1, ch=0) for v in (image, spiked)]
    differing = int(torch.count_nonzero(a != b))
    print('window / volume: %d of %d outputs differ (cap %d), knots %s and %s' % (differing, a.numel(), cap, xa.tolist(), xb.tolist()))
    assert torch.equal(xa, xb) and differing <= cap
    plain = []
    for v in (image, spiked):
        out = torch.full((image.shape[0], RH, RW, 1), float('nan'), device='cuda:0')
        ops.preprocess_images(nn.host_to_device(v, 'cuda:0', np.float32), out, (RH, RW), (0, RH, 0), (0, RW, 0), 0)
        plain.append(out.cpu().numpy()[..., 0])
    same = int(np.count_nonzero(plain[0] == plain[1]))
    print('min / max: all but %d of %d outputs differ' % (same, plain[0].size))
    assert same <= 2 * image.shape[0]          # the two extremes of every slice stay -1 and 1


# ---- the loader (CPU through the stand-ins, and the same on the GPU) ------------------------------------------------------------------
SETTINGS = {
    'window-volume': {'mode': 'window'},
    'window-slice': {'mode': 'window', 'scope': 'slice', 'percentiles': [1, 99]},
    'landmarks': {'mode': 'landmarks', 'standard': {'t1': SCALE11, 't2': [-1.0, -0.9, -0.7, -0.5, -0.3, 0.0, 0.2, 0.4, 0.6, 0.9, 1.0]}},
}


def _count_selections(monkeypatch):
    from multimodal_segmentation_amd import ops
    real, seen = ops.preprocess_quantiles, []

    def counted(img, resampled, ranks, per_volume):
        seen.append((tuple(img.shape), tuple(resampled), len(ranks), bool(per_volume)))
        return real(img, resampled, ranks, per_volume)
    monkeypatch.setattr(ops, 'preprocess_quantiles', counted)
    return seen


@pytest.mark.parametrize('name', sorted(SETTINGS))
def test_loader_applies_the_intensity_block(name, device, folder, monkeypatch):
    """training data, prediction and tiles of a folder with an `intensity` block equal the restatement volume by volume (2e-4, the
    outputs span [-1, 1]); the knots are selected once per (volume, modality) and shared by the tiles"""
    from multimodal_segmentation_amd.loaders.volume_folder import VolumeFolderLoader
    _set_intensity(folder, SETTINGS[name])
    loaders.data_conf['chaos'] = folder
    loader = loader_factory.init_loader('chaos')
    setting = loader.intensity
    assert setting['mode'] == SETTINGS[name]['mode'] and setting['scope'] == SETTINGS[name].get('scope', 'volume')
    seen = _count_selections(monkeypatch)
    data = loader.load_all_modalities_concatenated(0, 'training', 1)
    assert len(seen) == 2 * 2 and (device != 'cpu' or len(I.CALLS) == 4)          # volumes 1, 2 x t1, t2
    want = {}
    for v in (1, 2):
        for m, mod in enumerate(loader.modalities):
            image, label, res = loader.read_volume(v, mod)
            want[v, m] = I.preprocess(image, res, loader.target_resolution, (64, 64), setting, mod)
            got = data.get_volume_images_modi(m, v)
            assert np.abs(got - want[v, m]).max() <= 2e-4, (v, mod)
            assert got.min() >= -1.0 and got.max() <= 1.0
            _, want_m = R.preprocess(image, label, res, loader.target_resolution, loader.label_values, (64, 64))
            assert np.array_equal(data.get_volume_masks_modi(m, v), want_m)          # the label path is untouched
    del seen[:]
    images, geometry = loader.load_volume_for_prediction(1)
    assert len(seen) == 2
    for m in range(2):
        assert np.abs(nn.to_numpy(images[m]) - want[1, m]).max() <= 2e-4
    # tiles: a frame larger than the input on at least one axis, two predicted modalities from one upload
    del seen[:]
    uploaded = loader.upload_volume(1)
    assert len(seen) == 2 and all(g['knots'] is not None for g in uploaded[1])
    tiles_seen = 0
    for m in range(2):
        tiles, geo, plan = loader.load_volume_tiles(1, m, (16, 16), uploaded)
        for j, mod in enumerate(loader.modalities):
            image, _, res = loader.read_volume(1, mod)
            S = image.shape[0]
            RH, RW = geo[j]['resampled']
            rk, y, per_volume = I.setting_parts(setting, mod, RH * RW, S)
            mapped, _ = I.normalise(I.frames(image, RH, RW), rk, y, per_volume)
            rows, cols = plan[j]
            tiles_seen = max(tiles_seen, len(rows) * len(cols))
            got = nn.to_numpy(tiles[j])
            for tr, r in enumerate(rows):
                for tc, c in enumerate(cols):
                    t = tr * len(cols) + tc
                    assert np.abs(got[t * S:(t + 1) * S, ..., 0] - I.crop_pad(mapped, r, c, (64, 64))).max() <= 2e-4, (m, mod, tr, tc)
    assert len(seen) == 2 and tiles_seen > 1          # no selection per tile, nor per predicted modality


def test_folder_without_the_block_takes_the_three_launches(device, folder, monkeypatch):
    """absent key and {"mode": "minmax"}: bit for bit what the three existing ops give when called directly; nothing is selected"""
    from multimodal_segmentation_amd import ops
    from multimodal_segmentation_amd.loaders.volume_folder import VolumeFolderLoader, crop_pad_map, resampled_size
    dev = 'cuda:0' if device == 'cuda' else 'cpu'
    seen = _count_selections(monkeypatch)
    called = []
    from multimodal_segmentation_amd import _native
    real_call = _native.call          # the stand-in's dispatcher on the CPU; put back here, before the fixture removes the stand-in
    _native.call = lambda name, *a: (called.append(name), real_call(name, *a))[1]
    results = []
    try:
        for block in (None, {'mode': 'minmax'}):
            _set_intensity(folder, block)
            loader = VolumeFolderLoader(folder)
            assert loader.intensity == {'mode': 'minmax'}
            del called[:]
            data = loader.load_all_modalities_concatenated(0, 'validation', 1)
            assert [c for c in called if c.startswith('mmseg_preprocess')] == [
                'mmseg_preprocess_workspace_floats', 'mmseg_preprocess_minmax', 'mmseg_preprocess_image', 'mmseg_preprocess_label'] * 2
            pred, _ = loader.load_volume_for_prediction(3)
            results.append((data, pred))
    finally:
        _native.call = real_call
    assert not seen
    loader = VolumeFolderLoader(folder)
    values = nn.host_to_device(np.asarray(loader.label_values), dev, np.int32)
    images = torch.zeros((4, 64, 64, 2), device=dev)
    masks = torch.zeros((4, 64, 64, 8), device=dev)
    for m, mod in enumerate(loader.modalities):
        image, label, res = loader.read_volume(3, mod)
        RH, RW = resampled_size(image.shape[1], res[0], TARGET[0]), resampled_size(image.shape[2], res[1], TARGET[1])
        ops.preprocess_volume(nn.host_to_device(image, dev, np.float32), nn.host_to_device(label, dev, np.uint8), values, images, masks,
                              (RH, RW), crop_pad_map(RH, 64), crop_pad_map(RW, 64), m)
    images, masks = nn.to_numpy(images), nn.to_numpy(masks)
    for data, pred in results:
        for m in range(2):
            assert np.array_equal(_bits(data.get_volume_images_modi(m, 3)), _bits(images[..., m:m + 1]))
            assert np.array_equal(data.get_volume_masks_modi(m, 3), masks[..., 4 * m:4 * m + 4])
            assert np.array_equal(_bits(nn.to_numpy(pred[m])), _bits(images[..., m:m + 1]))


@pytest.mark.parametrize('block, message', [
    ({'mode': 'zscore'}, 'mode must be one of'),
    ({'mode': 'window', 'scope': 'organ'}, 'scope must be one of'),
    ({'mode': 'window', 'percentiles': [1, 50, 99]}, 'two percentiles'),
    ({'mode': 'window', 'percentiles': [99.5, 0.5]}, 'increase strictly'),
    ({'mode': 'window', 'percentiles': [0.5, 101]}, r'in \[0, 100\]'),
    ({'mode': 'landmarks', 'percentiles': [50], 'standard': {'t1': [-1], 't2': [1]}}, r'2\.\.16 percentiles'),
    ({'mode': 'landmarks', 'percentiles': list(range(17)), 'standard': {}}, r'2\.\.16 percentiles'),
    ({'mode': 'landmarks', 'percentiles': [1, 50, 40, 99], 'standard': {}}, 'increase strictly'),
    ({'mode': 'landmarks'}, 'needs "standard"'),
    ({'mode': 'landmarks', 'standard': {'t1': SCALE11}}, "modality 't2' must hold 11 values"),
    ({'mode': 'landmarks', 'standard': {'t1': SCALE11, 't2': SCALE11[:-1]}}, "modality 't2' must hold 11 values"),
    ({'mode': 'landmarks', 'standard': {'t1': SCALE11, 't2': [-0.9] + SCALE11[1:]}}, 'begin with -1 and end with 1'),
    ({'mode': 'landmarks', 'standard': {'t1': SCALE11, 't2': SCALE11[:-1] + [0.99]}}, 'begin with -1 and end with 1'),
    ({'mode': 'landmarks', 'standard': {'t1': SCALE11, 't2': [-1.0, -0.2, -0.5] + SCALE11[3:]}}, 'must not decrease'),
    ({'mode': 'landmarks', 'scope': 'slice', 'standard': {'t1': SCALE11, 't2': SCALE11}}, 'works per volume'),
    ({'mode': 'minmax', 'scope': 'volume'}, 'takes no other key'),
    ({'mode': 'window', 'percentile': [1, 99]}, 'unknown key'),
])
def test_manifest_errors_name_the_problem(block, message, folder):
    from multimodal_segmentation_amd.loaders.volume_folder import read_manifest
    assert 'intensity' not in read_manifest(folder)
    _set_intensity(folder, block)
    with pytest.raises(ValueError, match='dataset.json.*intensity.*' + message):
        read_manifest(folder)


def test_ops_refuse_bad_ranks_and_knots(standin):
    from multimodal_segmentation_amd import ops
    x = torch.zeros(2, 4, 5)
    for ranks, per_volume in (([0], False), ([0] * 17, False), ([0, 20], False), ([-1, 3], True), ([0, 40], True)):
        with pytest.raises(ValueError, match='preprocess_quantiles'):
            ops.preprocess_quantiles(x, (4, 5), ranks, per_volume)
    assert tuple(ops.preprocess_quantiles(x, (4, 5), [0, 19], False).shape) == (2, 2)
    assert tuple(ops.preprocess_quantiles(x, (4, 5), [0, 39], True).shape) == (1, 2)
    out = torch.zeros(2, 4, 5, 1)
    with pytest.raises(ValueError, match='knots'):
        ops.preprocess_images(x, out, (4, 5), (0, 4, 0), (0, 5, 0), 0, knots=(torch.zeros(3, 2), torch.zeros(2)))
    with pytest.raises(ValueError, match='knots'):
        ops.preprocess_images(x, out, (4, 5), (0, 4, 0), (0, 5, 0), 0, knots=(torch.zeros(2, 3), torch.zeros(2)))


# ---- the fit tool -----------------------------------------------------------------------------------------------------------------------
def test_fit_tool_reproduces_the_scale_and_copies_it(device, folder, tmp_path):
    """the scale written by tools/fit_intensity_landmarks.py = the restatement's (landmarks of the training volumes in fp64, brought
    to [-1, 1], averaged).  A landmark on the device lies within d = 2^-20 * max|raw| of the restatement's
    (test_selection_under_resampling), and y = -1 + 2 (x - x_0) / (x_K-1 - x_0) moves by at most 8 d / (x_K-1 - x_0)."""
    other = str(tmp_path / 'other')
    R.tool().write_folder(other, volumes=3, size=64, slices=2, seed=5, name='site_b')
    tool = _fit_tool()
    q = [2, 25, 50, 75, 98]
    block = tool.main([folder, '--split', '1', '--percentiles', ','.join(str(v) for v in q), '--copy-to', other])
    from multimodal_segmentation_amd.loaders.volume_folder import VolumeFolderLoader, read_manifest
    assert read_manifest(folder)['intensity'] == block == read_manifest(other)['intensity']
    assert block['mode'] == 'landmarks' and block['percentiles'] == [float(v) for v in q] and sorted(block['standard']) == ['t1', 't2']
    loader = VolumeFolderLoader(folder)
    assert loader.intensity['standard'] == block['standard'] and VolumeFolderLoader(other).intensity['mode'] == 'landmarks'
    volumes = loader.get_volumes_for_split(1, 'training')
    assert len(volumes) == 2
    for mod in loader.modalities:
        marks, bound = [], 0.0
        for v in volumes:
            image, _, res = loader.read_volume(v, mod)
            (RH, RW), _, _ = loader.geometry(image.shape[1], image.shape[2], res)
            x = I.knots(I.frames(image, RH, RW), I.ranks(image.shape[0] * RH * RW, q), True)[0]
            marks.append(x)
            bound = max(bound, 8.0 * 2.0 ** -20 * float(np.abs(image).max()) / (x[-1] - x[0]))
        want = I.standard_scale(marks)
        got = np.asarray(block['standard'][mod])
        print('%s: scale %s, largest difference %.3e (bound %.3e)' % (mod, got.tolist(), np.abs(got - want).max(), bound))
        assert got[0] == -1.0 and got[-1] == 1.0 and np.all(np.diff(got) >= 0)
        assert np.abs(got - want).max() <= bound


def test_fit_tool_refuses_a_constant_volume(standin, folder):
    manifest = json.load(open(os.path.join(folder, 'dataset.json')))
    path = os.path.join(folder, manifest['volumes']['2']['t1']['file'])
    arrays = dict(np.load(path))
    arrays['image'] = np.zeros_like(arrays['image'])
    np.savez_compressed(path, **arrays)
    with pytest.raises(ValueError, match='volume 2, modality t1.*equal'):
        _fit_tool().fit(folder, 0)


# ---- the override of a run ------------------------------------------------------------------------------------------------------------
def test_cli_override_reaches_the_loader_and_the_recorded_configuration(folder, tmp_path, monkeypatch):
    from multimodal_segmentation_amd.experiment import Experiment, parse_arguments
    monkeypatch.chdir(tmp_path)
    _set_intensity(folder, SETTINGS['landmarks'])
    base = ['--config', 'dafnet_config_chaos', '--split', '0', '--data_folder', folder]
    conf = Experiment().get_config(0, parse_arguments(base))
    assert loaders.intensity_conf == {} and conf.intensity['mode'] == 'landmarks'          # no override: the folder's own block
    conf = Experiment().get_config(0, parse_arguments(base + ['--intensity_norm', 'window', '--intensity_scope', 'slice',
                                                               '--intensity_percentiles', '2,98']))
    want = {'mode': 'window', 'scope': 'slice', 'percentiles': [2.0, 98.0]}
    assert loaders.intensity_conf == {'chaos': want} and conf.intensity == want
    assert loader_factory.init_loader('chaos').intensity == want
    dumped = json.load(open(os.path.join(conf.folder, 'experiment_configuration.json')))
    assert dumped['intensity'] == want and dumped['data_folder'] == folder
    conf = Experiment().get_config(0, parse_arguments(base + ['--intensity_norm', 'minmax']))
    assert conf.intensity == {'mode': 'minmax'} == loader_factory.init_loader('chaos').intensity
    # a later run without the options follows dataset.json again
    conf = Experiment().get_config(0, parse_arguments(base))
    assert loaders.intensity_conf == {} and loader_factory.init_loader('chaos').intensity['mode'] == 'landmarks'
    with pytest.raises(SystemExit):
        parse_arguments(base + ['--intensity_scope', 'slice'])
    with pytest.raises(SystemExit):
        parse_arguments(base + ['--intensity_norm', 'landmarks'])


def test_override_applies_to_the_loaded_arrays(standin, folder, tmp_path, monkeypatch):
    """the registry changes what a loader computes, not only what it reports"""
    loaders.data_conf['chaos'] = folder
    loaders.intensity_conf['chaos'] = {'mode': 'window', 'percentiles': [5, 95]}
    loader = loader_factory.init_loader('chaos')
    data = loader.load_all_modalities_concatenated(0, 'test', 1)
    image, _, res = loader.read_volume(4, 't2')
    want = I.preprocess(image, res, loader.target_resolution, (64, 64), {'mode': 'window', 'percentiles': [5, 95]}, 't2')
    assert np.abs(data.get_volume_images_modi(1, 4) - want).max() <= 2e-4
    assert np.count_nonzero(want == 1.0) > 0.04 * want.size


def test_predict_folder_with_another_setting_logs_a_warning(folder, tmp_path, caplog):
    from multimodal_segmentation_amd.utils.config import EasyDict
    from multimodal_segmentation_amd.experiment import warn_predict_stages
    other = str(tmp_path / 'scans')
    R.tool().write_folder(other, volumes=3, size=64, slices=2, seed=5, name='site_b', unlabelled=True)
    log = logging.getLogger('test_volume_intensity')
    conf = EasyDict(folder='run', intensity={'mode': 'window', 'scope': 'volume', 'percentiles': [0.5, 99.5]})
    with caplog.at_level(logging.WARNING):
        assert warn_predict_stages(conf, other, log) == ['intensity']
    assert 'minmax' in caplog.text and 'window' in caplog.text and other in caplog.text
    caplog.clear()
    _set_intensity(other, {'mode': 'window'})
    with caplog.at_level(logging.WARNING):
        assert not warn_predict_stages(conf, other, log)
        assert not warn_predict_stages(EasyDict(folder='run'), folder, log)          # neither records nor asks for anything
    assert caplog.text == ''
    loaders.intensity_conf['site_b'] = {'mode': 'minmax'}                                # the override counts
    with caplog.at_level(logging.WARNING):
        assert warn_predict_stages(conf, other, log) == ['intensity']


# ---- the example folder -----------------------------------------------------------------------------------------------------------------
def test_example_folder_with_hot_voxels(tmp_path):
    tool = R.tool()
    plain, hot = str(tmp_path / 'plain'), str(tmp_path / 'hot')
    assert tool.write_folder(plain, volumes=3, size=32, slices=2, seed=1) == tool.write_folder(hot, volumes=3, size=32, slices=2, seed=1,
                                                                                               hot_voxels=2)
    for name in sorted(os.listdir(plain)):
        if not name.endswith('.npz'):
            continue
        a, b = np.load(os.path.join(plain, name)), np.load(os.path.join(hot, name))
        assert np.array_equal(a['label'], b['label']) and np.array_equal(a['resolution'], b['resolution'])
        assert a['image'].shape == b['image'].shape and b['image'].dtype == np.int16
        ratio = b['image'].reshape(b['image'].shape[0], -1).max(axis=1) / np.percentile(b['image'], 99)
        assert np.all(ratio > 4)          # every slice carries voxels far above the bulk


# ---- ABI --------------------------------------------------------------------------------------------------------------------------------
def test_entry_points_declared_and_arguments_checked():
    """the header declares the three entry points; the launchers refuse K = 1, K = 17, a segment of 2^31 values or more and null
    pointers, without launching"""
    from multimodal_segmentation_amd import _native
    protos = _native.parse_header()
    for name in I.STANDINS:
        assert name in protos, name
    _native.build()
    lib = _native.load()
    assert lib.mmseg_preprocess_quantiles_workspace_bytes(3, 2, 0) == 4 * (3 * 2 * 2 + 4 * 3 * 2 * 256)
    assert lib.mmseg_preprocess_quantiles_workspace_bytes(3, 16, 1) == 4 * (2 * 16 + 4 * 16 * 256)
    for S, K in ((0, 2), (3, 1), (3, 17)):
        assert lib.mmseg_preprocess_quantiles_workspace_bytes(S, K, 0) == 0
    one = 1          # stands for a non-null pointer: a refused call launches nothing and touches no memory
    geo = [3, 10, 10, 12, 12]
    assert lib.mmseg_preprocess_quantiles(one, one, one, one, *(geo + [1, 0, None])) != 0
    assert lib.mmseg_preprocess_quantiles(one, one, one, one, *(geo + [17, 1, None])) != 0
    assert lib.mmseg_preprocess_quantiles(one, one, one, one, 65535, 8, 8, 256, 256, 2, 1, None) != 0          # 2^32 values in one segment
    for null in range(4):
        ptrs = [None if i == null else one for i in range(4)]
        assert lib.mmseg_preprocess_quantiles(*(ptrs + geo + [2, 0, None])) != 0
    tail = [8, 8, 2, 8, 0, 2, 8, 0, 2, 0]
    assert lib.mmseg_preprocess_image_map(one, one, one, one, *(geo + tail + [1, 0, None])) != 0
    assert lib.mmseg_preprocess_image_map(one, one, one, one, *(geo + tail + [17, 0, None])) != 0
    assert lib.mmseg_preprocess_image_map(one, one, one, one, 65535, 8, 8, 256, 256, *(tail + [2, 1, None])) != 0
    assert lib.mmseg_preprocess_image_map(one, one, one, one, *(geo + [8, 8, 6, 8, 0, 2, 8, 0, 2, 0] + [2, 0, None])) != 0      # lo + kept > RH
    for null in range(4):
        ptrs = [None if i == null else one for i in range(4)]
        assert lib.mmseg_preprocess_image_map(*(ptrs + geo + tail + [2, 0, None])) != 0
