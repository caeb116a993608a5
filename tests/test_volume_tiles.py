"""Whole-slice prediction: frames larger than the network's input cut into tiles, predicted and blended on the device.  The tile plan
and weights (loaders/volume_folder.py tile_axis / tile_weights / tiles_of_other), `load_volume_tiles`, csrc/postprocess.hip
(mmseg_blend_tiles), ops.blend_tiles, `tiles=` / `tile_overlap=` of VolumePredictor.run and `--predict_tiles` /
`--predict_tile_overlap`, against the fp64 restatement of tests/volume_tiles_ref.py.

Comparison rules (set by the feature's issue).
  map     the blended map differs from the fp64 restatement by at most 1e-5 (T.MAP_BAR: at most 64 covering tiles, (64 + 2) * 2^-24 =
          3.9e-6 for probabilities in [0, 1], with margin); a pixel that one tile covers is a bit-exact copy; NaN in a container's
          padding reaches no output; two runs are bitwise equal; `prob` is left alone.
  labels  restore_label of the blended map equals the restatement on every decidable pixel (0 differing), orders 0 and 1; a pixel is
          undecidable when an organ's fp64 blended-and-sampled probability lies within 2e-5 of 0.5 (P.UNDECIDABLE + the map bar), and
          at most P.CAP (0.1 %) of a case's pixels may be (test_inputs_are_decidable_and_not_vacuous)."""
import functools
import importlib.util
import json
import os

import numpy as np
import pytest
import torch

from multimodal_segmentation_amd import nn
from tests import helpers as Hh
from tests import volume_holes_ref as F
from tests import volume_loader_ref as R
from tests import volume_predict_ref as P
from tests import volume_tiles_ref as T
from tests.test_volume_loader import VALUES
from tests.volume_fixtures import _clean_registry, _dev, _up, device  # noqa: F401

S = 3
GRID_CAP = 1024 * 256          # PO_SURF_MAXBLK * PO_BLOCK of csrc/postprocess.hip: where the grid-stride loop of the blend wraps
CHANNELS = ((5, 4), (4, 4), (3, 2))          # (C, K): a soft-max with background, the 16-byte path, two organs of three channels
# name -> (frame (RH, RW), O, overlap, raw (H, W)): the raw sizes are no multiple of anything and differ from the frame on both axes
GEOMETRIES = {
    '77x53-3x2': ((77, 53), 32, 8, (91, 47)),          # 3 x 2 tiles, nothing divides
    '40x90-padded-rows': ((40, 90), 48, 24, (37, 101)),          # one padded tile on the rows (before = 4), 3 tiles on the columns
    '33x33-o-plus-1': ((33, 33), 32, 31, (41, 29)),          # R = O + 1: two tiles per axis that overlap by O - 1
    '32x32-one-tile': ((32, 32), 32, 16, (45, 38)),
    '96x64-mosaic': ((96, 64), 32, 0, (83, 72)),          # overlap 0: an exact 3 x 2 mosaic
}
PAST_CAP = ('77x53-3x2', 66)          # 66 * 77 * 53 = 269346 frame pixels: past the cap on both paths of the kernel


@pytest.fixture
def dev(device, monkeypatch):
    """the shared `device` fixture, with the stand-ins of the blend and (for the chain) of the hole filling on top of its table"""
    if device == 'cpu':
        from tests import cpu_backend as cb
        for name, fn in list(T.STANDINS.items()) + list(F.STANDINS.items()):
            monkeypatch.setitem(cb._TABLE, name, fn)
    return _dev(device)


# ---- the inputs --------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _case(name, C, K, slices=S):
    """(prob [T*slices,O,O,C] fp32 with NaN in every container's padding, rows, cols, the restatement's blended map and coverage): a
    soft-max over smooth random fields on the frame (as tests/test_volume_predict._case_data makes them), every tile its window of it
    plus a smooth field of its own, so that the tiles of a pixel differ and the blend has something to do.  More slices than S repeat
    the S slices."""
    (RH, RW), O, overlap, _ = GEOMETRIES[name]
    rng = np.random.RandomState(7000 + 10 * sorted(GEOMETRIES).index(name) + C)
    rows, cols = T.plan(RH, O, overlap), T.plan(RW, O, overlap)
    frame = 4.0 * np.concatenate([Hh.smooth_field(rng, S, RH, RW, sigma=3.0) for _ in range(C)], axis=-1).astype(np.float64)
    tiles = []
    for lo_r, kept_r, before_r in rows:
        for lo_c, kept_c, before_c in cols:
            own = 0.6 * np.concatenate([Hh.smooth_field(rng, S, kept_r, kept_c, sigma=3.0) for _ in range(C)], axis=-1)
            f = frame[:, lo_r:lo_r + kept_r, lo_c:lo_c + kept_c] + own
            e = np.exp(f - f.max(-1, keepdims=True))
            tile = np.full((S, O, O, C), np.nan, np.float32)
            tile[:, before_r:before_r + kept_r, before_c:before_c + kept_c] = e / e.sum(-1, keepdims=True)
            reps = -(-slices // S)
            tiles.append(np.tile(tile, (reps, 1, 1, 1))[:slices])
    prob = np.concatenate(tiles, axis=0)
    want, count = T.blend(prob, rows, cols, T.weights(rows, O), T.weights(cols, O), slices, RH, RW, K)
    for a in (prob, want, count):
        a.setflags(write=False)
    return prob, rows, cols, want, count


def _labels(want, values, raw_hw, order):
    """the restatement's labels of a blended fp64 map [S,RH,RW,K] on the raw grid, and the undecidable pixels: the whole frame is the
    window"""
    RH, RW = want.shape[1:3]
    v = P.sample(want, len(values), raw_hw, (RH, RW), (0, RH, 0), (0, RW, 0), order)
    label = np.zeros(v.shape[:3], np.uint8)
    for k in reversed(range(len(values))):
        label[v[..., k] > 0.5] = values[k]
    return label, (np.abs(v - 0.5) < T.LABEL_BAND).any(-1)


def _blend(prob, rows, cols, O, slices, frame, K, dev):
    """ops.blend_tiles twice (the runs must be bitwise equal, `prob` untouched) -> the map as numpy"""
    from multimodal_segmentation_amd import ops
    from multimodal_segmentation_amd.loaders.volume_folder import tile_weights
    p = nn.host_to_device(np.array(prob), dev, np.float32)
    args = (rows, cols, tile_weights(rows, O), tile_weights(cols, O), slices, frame, K)
    out, again = ops.blend_tiles(p, *args), ops.blend_tiles(p, *args)
    assert out.dtype == torch.float32 and tuple(out.shape) == (slices,) + tuple(frame) + (K,)
    assert torch.equal(out, again) and not torch.isnan(out).any()
    assert np.array_equal(p.cpu().numpy(), prob, equal_nan=True)
    return out


# ---- 1. the plan (no GPU) ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('O', (8, 32))
def test_plan_covers_every_frame_and_matches_the_restatement(O):
    from multimodal_segmentation_amd.loaders.volume_folder import crop_pad_map, tile_axis, tile_weights
    refused = 0
    for overlap in sorted({0, 1, O // 4, O // 2, O - 2, O - 1}):
        for Rr in range(1, 4 * O + 1):
            try:
                want = T.plan(Rr, O, overlap)
            except ValueError:
                with pytest.raises(ValueError, match='tile_overlap'):
                    tile_axis(Rr, O, overlap)
                refused += 1
                continue
            tiles = tile_axis(Rr, O, overlap)
            assert [tuple(t) for t in tiles] == want and 1 <= len(tiles) <= 8
            if Rr <= O:
                assert tiles == [crop_pad_map(Rr, O)] == [(0, Rr, (O - Rr) // 2)]
            else:
                lo = [t[0] for t in tiles]
                assert all(t[1:] == (O, 0) for t in tiles) and lo[0] == 0 and lo[-1] == Rr - O and lo == sorted(lo)
                assert all(a + O - b >= overlap for a, b in zip(lo, lo[1:]))
                covered = np.zeros(Rr, int)
                for a in lo:
                    covered[a:a + O] += 1
                assert covered.min() >= 1
            w = tile_weights(tiles, O)
            assert w.dtype == np.float32 and w.shape == (len(tiles), O) and np.array_equal(w, T.weights(tiles, O))
            assert (w >= 1).all() and np.array_equal(w, np.round(w))
            if len(tiles) > 1:          # tapering towards a neighbour only
                assert w[0, 0] == O and w[0, -1] == 1 and w[-1, 0] == 1 and w[-1, -1] == O and (w[1:-1, [0, -1]] == 1).all()
            else:
                assert (w == O).all()
    assert refused > 0          # O - 1 of overlap advances one pixel per tile: more than 8 tiles from R = O + 8 on
    for bad in (-1, O, O + 3):
        with pytest.raises(ValueError, match='tile_overlap'):
            tile_axis(2 * O, O, bad)


@pytest.mark.parametrize('O', (8, 32))
def test_windows_of_the_other_modality_keep_the_preprocess_contract(O):
    from multimodal_segmentation_amd.loaders.volume_folder import crop_pad_map, tile_axis, tile_window, tiles_of_other
    outside = 0
    for overlap in (0, O // 2):
        for R_m in list(range(1, 4 * O + 1, 3)) + [O, O + 1]:
            tiles = tile_axis(R_m, O, overlap)
            for R_j in list(range(1, 5 * O, 5)) + [1, 2, O, O + 1, R_m]:
                got = tiles_of_other(tiles, R_m, R_j, O)
                starts = T.other_starts(tiles, R_m, R_j, O)
                assert len(got) == len(tiles)
                for (lo, kept, before), start in zip(got, starts):
                    assert T.contract_ok(lo, kept, before, R_j, O), (R_m, R_j, O, overlap, (lo, kept, before))
                    assert np.array_equal(T.map_indices(lo, kept, before, O), T.window_indices(start, R_j, O))
                    outside += start >= R_j or start + O <= 0
                # the tile that coincides with the centre crop of the planned frame coincides with the other frame's
                for (lo, kept, before), other in zip(tiles, got):
                    if lo - before == T.centre(R_m, O):
                        c = crop_pad_map(R_j, O)
                        assert other[0] - other[2] == (c[0] if R_j > O else -c[2])
                if R_j == R_m:
                    assert got == [tuple(t) for t in tiles]
    assert outside > 0          # windows wholly outside the other frame occurred: they repeat the nearest edge pixel
    assert tile_window(50, 10, O) == (9, 1, 0) and tile_window(-O - 3, 10, O) == (0, 1, 0)


# ---- 2. the inputs and the restatement alone (no GPU) ---------------------------------------------------------------------------------------
def test_inputs_are_decidable_and_not_vacuous():
    for name in sorted(GEOMETRIES):
        (RH, RW), O, overlap, raw_hw = GEOMETRIES[name]
        for C, K in CHANNELS:
            prob, rows, cols, want, count = _case(name, C, K)
            assert count.min() >= 1 and np.isfinite(want).all() and want.min() >= 0 and want.max() <= 1
            assert np.isnan(prob).any() == any(t[1] < O for t in rows + cols)
            for order in (0, 1):
                label, undecidable = _labels(want, VALUES[:K], raw_hw, order)
                fg = np.count_nonzero(label) / float(label.size)
                print('%s C %d K %d order %d: %d x %d tiles, coverage 1..%d, %d of %d raw pixels undecidable, foreground %.1f %%'
                      % (name, C, K, order, len(rows), len(cols), count.max(), np.count_nonzero(undecidable), label.size, 100 * fg))
                assert np.count_nonzero(undecidable) <= P.CAP * label.size
                assert 0.02 < fg < 0.98
    assert [len(T.plan(n, 32, 8)) for n in (77, 53)] == [3, 2] and [len(T.plan(n, 48, 24)) for n in (40, 90)] == [1, 3]
    assert T.plan(40, 48, 24) == [(0, 40, 4)] and T.plan(33, 32, 31) == [(0, 32, 0), (1, 32, 0)]
    assert _case('96x64-mosaic', 5, 4)[4].max() == 1 and _case('33x33-o-plus-1', 5, 4)[4].max() == 4
    name, slices = PAST_CAP
    assert slices * np.prod(GEOMETRIES[name][0]) > GRID_CAP


# ---- 3. the blend, op level -----------------------------------------------------------------------------------------------------------------
def _check_map(name, C, K, slices, dev):
    (RH, RW), O, overlap, raw_hw = GEOMETRIES[name]
    prob, rows, cols, want, count = _case(name, C, K, slices)
    out = _blend(prob, rows, cols, O, slices, (RH, RW), K, dev)
    got = out.cpu().numpy()
    worst = float(np.abs(got - want).max())
    print('%s C %d K %d, %d slices: largest difference from the fp64 restatement %.3g (bar %.0e), coverage 1..%d'
          % (name, C, K, slices, worst, T.MAP_BAR, count.max()))
    assert worst <= T.MAP_BAR
    # a pixel that one tile covers is that tile's value, bit for bit
    single = np.zeros((slices, RH, RW, K), np.float32)
    for tr, (lo_r, kept_r, before_r) in enumerate(rows):
        for tc, (lo_c, kept_c, before_c) in enumerate(cols):
            t = tr * len(cols) + tc
            single[:, lo_r:lo_r + kept_r, lo_c:lo_c + kept_c] = prob[t * slices:(t + 1) * slices, before_r:before_r + kept_r,
                                                                     before_c:before_c + kept_c, :K]
    once = count == 1
    assert np.array_equal(got[:, once].view(np.uint32), single[:, once].view(np.uint32))
    return out, want, once


@pytest.mark.parametrize('C,K', CHANNELS)
@pytest.mark.parametrize('name', sorted(GEOMETRIES))
def test_blended_map_and_labels_match_the_restatement(name, C, K, dev):
    from multimodal_segmentation_amd import ops
    (RH, RW), O, overlap, raw_hw = GEOMETRIES[name]
    out, want, once = _check_map(name, C, K, S, dev)
    if name in ('96x64-mosaic', '32x32-one-tile'):
        assert once.all()          # the whole map is a copy
    else:
        assert once.any() or name == '33x33-o-plus-1'
        assert not once.all()
    values = _up(np.asarray(VALUES[:K]), dev, np.int32)
    for order in (0, 1):
        label, undecidable = _labels(want, VALUES[:K], raw_hw, order)
        got = ops.restore_label(out, values, raw_hw, (RH, RW), (0, RH, 0), (0, RW, 0), order).cpu().numpy()
        differing = int(np.count_nonzero((got != label) & ~undecidable))
        print('%s C %d K %d order %d: %d differing pixels of %d compared (%d undecidable left out), foreground %d'
              % (name, C, K, order, differing, label.size - np.count_nonzero(undecidable), np.count_nonzero(undecidable),
                 np.count_nonzero(label)))
        assert np.count_nonzero(undecidable) <= P.CAP * label.size
        assert differing == 0


@pytest.mark.parametrize('C,K', CHANNELS[:2])
def test_a_frame_past_the_grid_cap(C, K, dev):
    name, slices = PAST_CAP
    _check_map(name, C, K, slices, dev)


def test_a_pixel_that_no_tile_covers_gets_zero_and_every_element_is_written(dev):
    """the planner never leaves a gap; the kernel defines it anyway.  The entry point itself, on a pre-filled output"""
    from multimodal_segmentation_amd import _native
    O, RH, RW, C, K = 8, 20, 9, 5, 4
    rows, cols = [(0, 8, 0), (12, 8, 0)], [(0, 8, 0), (1, 8, 0)]          # frame rows 8 .. 11 are covered by no tile
    rng = np.random.RandomState(5)
    prob = rng.uniform(0, 1, size=(4 * S, O, O, C)).astype(np.float32)
    wr, wc = T.weights(rows, O).astype(np.float32), T.weights(cols, O).astype(np.float32)
    want, count = T.blend(prob, rows, cols, wr, wc, S, RH, RW, K)
    assert count[8:12].max() == 0 and count[:8].min() >= 1
    out = torch.full((S, RH, RW, K), 7.0, device=dev)
    rc = _native.call('mmseg_blend_tiles', _up(prob, dev, np.float32), _up(np.asarray(rows), dev, np.int32), _up(np.asarray(cols), dev, np.int32),
                      _up(wr, dev, np.float32), _up(wc, dev, np.float32), out, S, 2, 2, O, O, C, K, RH, RW)
    got = out.cpu().numpy()
    assert rc == 0 and not (got[:, 8:12] != 0).any() and np.abs(got - want).max() <= T.MAP_BAR and (got[:, :8] != 7.0).all()


# ---- 4. tiles in: the loader ----------------------------------------------------------------------------------------------------------------
TARGET = (2.0, 2.0)
O_FOLDER = 32
# volume -> per modality (raw H, W, resolution): frames 64 x 63 and 72 x 75 (larger on both axes), 68 x 24 and 50 x 24 (larger on one,
# short on the other), 30 x 29 and 30 x 30 (fit)
FOLDER = {'1': ((80, 70, (1.6, 1.8)), (60, 100, (2.4, 1.5))),
          '2': ((90, 30, (1.5, 1.6)), (50, 40, (2.0, 1.2))),
          '3': ((40, 36, (1.5, 1.6)), (30, 30, (2.0, 2.0)))}
FRAMES = {'1': ((64, 63), (72, 75)), '2': ((68, 24), (50, 24)), '3': ((30, 29), (30, 30))}
CENTRES = (-0.6, -0.2, 0.2, 0.6)


def organ_probabilities(x):
    """pointwise: intensity x in [-1, 1] [...,1] -> [...,5], organ k where x lies within 0.18 of CENTRES[k] (a smooth band), then the
    background.  Reads no neighbourhood, so every tile of a frame pixel gives the same value."""
    c = torch.as_tensor(CENTRES, dtype=x.dtype, device=x.device)
    p = torch.sigmoid(12.0 * (0.18 - (x - c).abs()))
    return torch.cat([p, (1 - p.sum(-1, keepdim=True)).clamp(min=0)], dim=-1).contiguous()


class Pointwise(object):
    """predict_mask(m, 'simple'): organ_probabilities of the image of modality m; mode 'def': of the OTHER modality's image"""
    modalities = ['t1', 't2']

    def __init__(self):
        self.batches = []

    def predict_mask(self, modality_index, mode, image_list):
        assert len(image_list) == 2 and all(x.shape == image_list[0].shape for x in image_list)
        self.batches.append(image_list[0].shape[0])
        return organ_probabilities(image_list[modality_index if mode == 'simple' else 1 - modality_index])


def _conf(batch_size=5):
    from multimodal_segmentation_amd.utils.config import EasyDict
    return EasyDict(dict(batch_size=batch_size, input_shape=(O_FOLDER, O_FOLDER, 1), num_masks=4, folder='nowhere'))


def _texture(rng, slices, H, W):
    """a smooth field under a fine oblique pattern, int16: a tile misplaced by one pixel shows"""
    y, x = np.mgrid[0:H, 0:W]
    base = Hh.smooth_field(rng, slices, H, W, sigma=max(H, W) / 10.0)[..., 0]
    fine = 0.25 * np.sin(0.9 * y + 0.5 * x)[None] * np.cos(0.35 * x - 0.2 * y)[None]
    return np.round(700.0 * (base + fine + 1.5)).astype(np.int16)


@pytest.fixture
def wide_folder(tmp_path):
    """three volumes, two modalities with different raw sizes and resolutions, zero labels for now"""
    out = str(tmp_path / 'wide')
    os.makedirs(out)
    rng = np.random.RandomState(21)
    manifest = dict(name='wide', modalities=['t1', 't2'], label_values=VALUES, target_resolution=list(TARGET),
                    input_shape=[O_FOLDER, O_FOLDER, 1], splits=[{'training': [1], 'validation': [2], 'test': [3]}], volumes={})
    for v, mods in sorted(FOLDER.items()):
        entry = {}
        for name, (H, W, res) in zip(('t1', 't2'), mods):
            slices = S + (1 if name == 't2' else 0)
            fname = 'wide%s_%s.npz' % (v, name)
            np.savez_compressed(os.path.join(out, fname), image=_texture(rng, slices, H, W), label=np.zeros((slices, H, W), np.uint8),
                                resolution=np.asarray(res, np.float64))
            entry[name] = dict(file=fname, **({'slices': [[1, 1 + S]]} if name == 't2' else {}))
        manifest['volumes'][v] = entry
    json.dump(manifest, open(os.path.join(out, 'dataset.json'), 'w'))
    return out


def _whole_frames(loader, volume):
    """per modality the whole preprocessed frame [S,RH,RW,1] on the device: the frame itself as the container"""
    from multimodal_segmentation_amd import ops
    raw, geometry = loader.upload_volume(volume)
    frames = []
    for x, geo in zip(raw, geometry):
        RH, RW = geo['resampled']
        frame = torch.zeros((x.shape[0], RH, RW, 1), device=x.device)
        ops.preprocess_images(x, frame, (RH, RW), (0, RH, 0), (0, RW, 0), 0)
        frames.append(frame)
    return frames, geometry


def test_tiles_show_every_modality_at_the_offsets_of_the_plan(wide_folder, dev):
    """every tile of every modality is the whole preprocessed frame read at the restatement's window, edge-padded: exact, since a
    tile is the same resampled pixels under another index map and the rescale is per whole frame"""
    from multimodal_segmentation_amd.loaders.volume_folder import VolumeFolderLoader
    loader = VolumeFolderLoader(wide_folder)
    padded = 0
    for v in sorted(FOLDER):
        frames, geometry = _whole_frames(loader, v)
        assert [g['resampled'] for g in geometry] == list(FRAMES[v])
        for m in (0, 1):
            for overlap in ((16, 16), (5, 0)):
                images, geo2, plan = loader.load_volume_tiles(v, m, overlap)
                RH, RW = FRAMES[v][m]
                rows, cols = T.plan(RH, O_FOLDER, overlap[0]), T.plan(RW, O_FOLDER, overlap[1])
                assert [tuple(t) for t in plan[m][0]] == rows and [tuple(t) for t in plan[m][1]] == cols
                assert [g['file'] for g in geo2] == [g['file'] for g in geometry]
                for j in (0, 1):
                    RHj, RWj = FRAMES[v][j]
                    sr, sc = T.other_starts(rows, RH, RHj, O_FOLDER), T.other_starts(cols, RW, RWj, O_FOLDER)
                    assert tuple(images[j].shape) == (len(rows) * len(cols) * S, O_FOLDER, O_FOLDER, 1)
                    frame = frames[j].cpu().numpy()
                    got = images[j].cpu().numpy()
                    for tr, a in enumerate(sr):
                        for tc, b in enumerate(sc):
                            iy, ix = T.window_indices(a, RHj, O_FOLDER), T.window_indices(b, RWj, O_FOLDER)
                            t = tr * len(cols) + tc
                            assert np.array_equal(got[t * S:(t + 1) * S], frame[:, iy][:, :, ix]), (v, m, j, overlap, tr, tc)
                            padded += a < 0 or b < 0 or a + O_FOLDER > RHj or b + O_FOLDER > RWj
    assert padded > 0


def test_other_modality_through_the_predictor(wide_folder, dev):
    """mode 'def' with a model that reads the OTHER modality: the blended map equals the restatement's blend of that modality's
    windows"""
    from multimodal_segmentation_amd.loaders.volume_folder import VolumeFolderLoader
    from multimodal_segmentation_amd.volume_predictor import VolumePredictor
    loader = VolumeFolderLoader(wide_folder)
    predictor = VolumePredictor(Pointwise(), _conf())
    for v in ('1', '2'):
        frames, geometry = _whole_frames(loader, v)
        for m in (0, 1):
            (RH, RW), (RHj, RWj) = FRAMES[v][m], FRAMES[v][1 - m]
            rows, cols = T.plan(RH, O_FOLDER, 16), T.plan(RW, O_FOLDER, 16)
            other = organ_probabilities(frames[1 - m]).cpu().numpy()
            tiles = []
            for a in T.other_starts(rows, RH, RHj, O_FOLDER):
                for b in T.other_starts(cols, RW, RWj, O_FOLDER):
                    tiles.append(other[:, T.window_indices(a, RHj, O_FOLDER)][:, :, T.window_indices(b, RWj, O_FOLDER)])
            want, count = T.blend(np.concatenate(tiles), rows, cols, T.weights(rows, O_FOLDER), T.weights(cols, O_FOLDER), S, RH, RW, 4)
            got = predictor.predict_tiled(loader, v, m, 'def', (16, 16), loader.upload_volume(v)).cpu().numpy()
            worst = float(np.abs(got - want).max())
            print('volume %s modality %d reads modality %d: %d x %d tiles, largest difference %.3g' % (v, m, 1 - m, len(rows), len(cols), worst))
            assert count.min() >= 1 and worst <= T.MAP_BAR and want.max() > 0.5


# ---- 5. offsets, end to end without training ------------------------------------------------------------------------------------------------
def _yardstick(loader, volume, values, order):
    """per modality (the labels that restore_label gives the pointwise function of the WHOLE preprocessed frame, undecidable pixels)"""
    from multimodal_segmentation_amd import ops
    frames, geometry = _whole_frames(loader, volume)
    out = []
    for frame, geo in zip(frames, geometry):
        RH, RW = geo['resampled']
        prob = organ_probabilities(frame)
        label = ops.restore_label(prob, values, geo['raw_shape'][1:], (RH, RW), (0, RH, 0), (0, RW, 0), order).cpu().numpy()
        _, undecidable = _labels(prob.cpu().numpy().astype(np.float64)[..., :4], VALUES, geo['raw_shape'][1:], order)
        out.append((label, undecidable, geo))
    return out


@pytest.mark.parametrize('order', (1, 0))
def test_tiled_prediction_reaches_the_pixels_outside_the_centre_window(order, wide_folder, tmp_path, dev):
    from multimodal_segmentation_amd.loaders.volume_folder import VolumeFolderLoader
    from multimodal_segmentation_amd.volume_predictor import VolumePredictor
    loader = VolumeFolderLoader(wide_folder)
    values = _up(np.asarray(VALUES), dev, np.int32)
    truth = {}
    for v in sorted(FOLDER):          # the truth of every file: the full-frame yardstick
        for (label, undecidable, geo) in _yardstick(loader, v, values, order):
            path = os.path.join(wide_folder, geo['file'])
            with np.load(path) as z:
                arrays = {k: z[k] for k in z.files}
            arrays['label'][geo['slices']] = label
            np.savez_compressed(path, **arrays)
            truth[geo['file']] = (arrays['label'], undecidable, geo)
    plain, tiled = str(tmp_path / 'plain'), str(tmp_path / 'tiled')
    model = Pointwise()
    VolumePredictor(model, _conf()).run(wide_folder, plain, order=order)
    untiled_batches, model.batches = model.batches, []
    VolumePredictor(model, _conf()).run(wide_folder, tiled, order=order, tiles=True)
    assert set(untiled_batches) == {S} and max(model.batches) == 5 and sum(model.batches) > sum(untiled_batches)
    settings = [json.load(open(os.path.join(d, 'predictions.json'))) for d in (plain, tiled)]
    assert sorted(settings[1]) == sorted(list(settings[0]) + ['tiles', 'tile_overlap'])
    assert settings[1]['tiles'] is True and settings[1]['tile_overlap'] == [16, 16]
    rows = {d: {mod: _dice_rows(os.path.join(d, 'results_native_%s.csv' % mod)) for mod in ('t1', 't2')} for d in (plain, tiled)}
    for v in sorted(FOLDER):
        for m, mod in enumerate(('t1', 't2')):
            fname = loader.manifest['volumes'][v][mod]['file']
            want, undecidable, geo = truth[fname]
            sel = geo['slices']
            entry = settings[1]['files'][fname]
            assert 'tile_origins' not in settings[0]['files'][fname]
            assert sorted(entry) == sorted(list(settings[0]['files'][fname]) + ['tile_origins'])
            RH, RW = geo['resampled']
            assert entry['tile_origins'] == dict(rows=[t[0] for t in T.plan(RH, O_FOLDER, 16)], cols=[t[0] for t in T.plan(RW, O_FOLDER, 16)])
            raw_a, raw_b = open(os.path.join(plain, fname), 'rb').read(), open(os.path.join(tiled, fname), 'rb').read()
            with np.load(os.path.join(plain, fname)) as z:
                before = z['label']
            with np.load(os.path.join(tiled, fname)) as z:
                after = z['label']
            if v == '3':          # the file fits: the old path ran, the output is byte for byte that of tiles=False
                assert raw_a == raw_b
                continue
            inside = P.window_mask(geo['raw_shape'][1:], geo['resampled'], geo['rows'], geo['cols'])
            outside = np.broadcast_to(~inside, want[sel].shape)
            differing = int(np.count_nonzero((after[sel] != want[sel]) & ~undecidable))
            print('volume %s %s order %d: frame %s, %d raw pixels per slice outside the centre window, truth foreground there %d, untiled %d, '
                  'tiled %d; %d differing pixels (%d undecidable left out); Dice %.3f -> %.3f'
                  % (v, mod, order, geo['resampled'], np.count_nonzero(~inside), np.count_nonzero(want[sel][outside]),
                     np.count_nonzero(before[sel][outside]), np.count_nonzero(after[sel][outside]), differing,
                     np.count_nonzero(undecidable), rows[plain][mod][v], rows[tiled][mod][v]))
            assert np.count_nonzero(undecidable) <= P.CAP * undecidable.size
            assert differing == 0          # every tile in its place: the texture would show a shift of one pixel
            assert (~inside).any() and want[sel][outside].any() and not before[sel][outside].any()          # what fails without the feature
            assert after[sel][outside].any()
            assert rows[tiled][mod][v] > rows[plain][mod][v]
            assert not after[np.setdiff1d(np.arange(after.shape[0]), sel)].any()


def _dice_rows(path):
    lines = open(path).read().strip().split('\n')
    return {l.split(',')[0]: float(l.split(',')[1]) for l in lines[1:]}


def test_overlap_argument(wide_folder, tmp_path, dev):
    from multimodal_segmentation_amd.volume_predictor import VolumePredictor, check_tile_overlap
    assert check_tile_overlap(None, (32, 48, 1)) == (16, 24) and check_tile_overlap(8, (32, 48, 1)) == (8, 8)
    assert check_tile_overlap((0, 47), (32, 48, 1)) == (0, 47)
    for bad in (-1, 32, (8, 48), 2.5, 'x', (1, 2, 3), True):
        with pytest.raises((ValueError, TypeError), match='tile_overlap'):
            check_tile_overlap(bad, (32, 48, 1))
    with pytest.raises(ValueError, match='tile_overlap'):
        VolumePredictor(Pointwise(), _conf()).run(wide_folder, str(tmp_path / 'no'), tiles=True, tile_overlap=32)
    assert not os.path.exists(str(tmp_path / 'no'))
    with pytest.raises(ValueError, match='tile_overlap'):          # 31 of overlap: 75 columns need 44 tiles
        VolumePredictor(Pointwise(), _conf()).run(wide_folder, str(tmp_path / 'many'), tiles=True, tile_overlap=31)


# ---- 6. the chain: experiment.py ------------------------------------------------------------------------------------------------------------
def test_experiment_predicts_tiles_then_filters_and_fills(tmp_path, dev, monkeypatch):
    from tests.test_volume_holes import _experiment
    folder = str(tmp_path / 'volumes')
    manifest = R.tool().write_folder(folder, volumes=3, size=64, slices=3, seed=6, slice_spacing=(4.0, 9.0))
    exp = _experiment(monkeypatch, Pointwise(), str(tmp_path / 'run'))
    out = str(tmp_path / 'out')
    exp.run(['--config', 'dafnet_config_chaos', '--split', '0', '--test', 'true', '--predict_folder', folder, '--predict_out', out,
             '--predict_tiles', 'true', '--predict_tile_overlap', '8', '--predict_components', 'largest', '--predict_fill_holes', '2d'])
    files = [e[mod]['file'] for e in manifest['volumes'].values() for mod in ('t1', 't2')]
    csvs = ['results_%s_%s.csv' % (a, b) for a in ('native', 'surface', 'components', 'holes') for b in ('t1', 't2')]
    assert sorted(os.listdir(out)) == sorted(['predictions.json'] + csvs + files)
    settings = json.load(open(os.path.join(out, 'predictions.json')))
    assert settings['tiles'] is True and settings['tile_overlap'] == [8, 8] and settings['fill_holes'] == '2d'
    several = 0
    for fname in files:
        origins = settings['files'][fname]['tile_origins']
        several += len(origins['rows']) * len(origins['cols']) > 1
        with np.load(os.path.join(folder, fname)) as z, np.load(os.path.join(out, fname)) as p:
            assert p['label'].shape == z['image'].shape and p['label'].dtype == np.uint8 and p['label'].any()
            assert set(np.unique(p['label']).tolist()) <= {0} | set(VALUES)
    assert several >= 2          # the tool draws fields of view of 0.85 to 1.2 input extents


def test_cli_options(monkeypatch, capsys):
    from multimodal_segmentation_amd import experiment
    from tests.test_volume_predict import _stub_conf
    base = ['--config', 'dafnet_config_chaos', '--split', '0']
    a = experiment.parse_arguments(base)
    assert a.predict_tiles is False and a.predict_tile_overlap is None
    a = experiment.parse_arguments(base + ['--predict_tiles', 'true', '--predict_tile_overlap', '8'])
    assert a.predict_tiles is True and a.predict_tile_overlap == 8

    def no_model(*args, **kwargs):
        raise AssertionError('the run went on past the options')
    conf = _stub_conf(3)
    conf.folder = 'nowhere'
    monkeypatch.setattr(experiment.Experiment, 'get_config', lambda self, split, args: conf)
    monkeypatch.setattr(experiment.Experiment, 'init_logging', lambda self, conf: None)
    monkeypatch.setattr(experiment.Experiment, 'get_executor', no_model)
    monkeypatch.setattr(experiment, 'resolve', no_model)
    capsys.readouterr()
    with pytest.raises(SystemExit):          # negative: refused with the other options
        experiment.Experiment().run(base + ['--predict_folder', 'G', '--predict_tiles', 'true', '--predict_tile_overlap', '-1'])
    assert '--predict_tile_overlap' in capsys.readouterr().err
    for bad in ('64', '200'):          # the input extent of the configuration is 64
        with pytest.raises(ValueError, match='--predict_tile_overlap'):
            experiment.Experiment().run(base + ['--predict_folder', 'G', '--predict_tiles', 'true', '--predict_tile_overlap', bad])


# ---- 7. ABI and arguments -----------------------------------------------------------------------------------------------------------------
def test_entry_point_declared_and_bad_arguments_refused():
    from multimodal_segmentation_amd import _native, ops
    protos = _native.parse_header()
    for name in T.STANDINS:
        assert name in protos and protos[name][1][-1] == 'void*', name
    assert len(protos['mmseg_blend_tiles'][1]) == 16 and callable(ops.blend_tiles)
    _native.build()
    lib = _native.load()
    blend = lib.mmseg_blend_tiles
    ptrs, bad = [16, 32, 48, 64, 80, 96], 1          # non-null pointers (a refused call launches nothing and touches no memory); hipErrorInvalidValue
    ok = [3, 2, 2, 32, 32, 5, 4, 77, 53]             # S, TR, TC, OH, OW, C, K, RH, RW
    for i, v in ((1, 0), (1, 9), (2, 0), (2, 9), (6, 6), (6, 0), (3, 0), (4, -1), (7, 0), (8, 0), (0, -1)):
        a = list(ok)
        a[i] = v
        assert blend(*(ptrs + a + [None])) == bad, a
    assert blend(*(ptrs + [3, 2, 2, 32, 32, 40, 17, 77, 53, None])) == bad                 # K > 16
    assert blend(*(ptrs + [4096, 8, 8, 64, 64, 5, 4, 8, 8, None])) == bad                  # prob: 2^31 bytes or more
    assert blend(*(ptrs + [64, 1, 1, 8, 8, 4, 4, 2048, 1024, None])) == bad                # out: exactly 2^31 bytes
    assert blend(*(ptrs + [30000, 8, 8, 30000, 30000, 5, 4, 8, 8, None])) == bad           # a product past 2^63
    for i in range(6):
        p = list(ptrs)
        p[i] = None
        assert blend(*(p + ok + [None])) == bad
    assert blend(*(ptrs + [0] + ok[1:] + [None])) == 0          # S = 0: nothing to do
    prob = torch.zeros(4 * 2, 8, 8, 5)
    rows, cols, w = [(0, 8, 0), (4, 8, 0)], [(0, 8, 0), (2, 8, 0)], np.ones((2, 8), np.float32)
    with pytest.raises(ValueError, match='blend_tiles'):
        ops.blend_tiles(prob, rows, cols, w, w, 3, (12, 10), 4)                 # 8 containers are not 2 x 2 tiles of 3 slices
    with pytest.raises(ValueError, match='blend_tiles'):
        ops.blend_tiles(prob, rows, cols, w, w, 2, (12, 10), 6)                 # K > C
    with pytest.raises(ValueError, match='blend_tiles'):
        ops.blend_tiles(prob, rows * 5, cols, np.ones((10, 8), np.float32), w, 2, (12, 10), 4)          # 10 tiles on an axis
    with pytest.raises(ValueError, match='blend_tiles'):
        ops.blend_tiles(prob, rows, cols, np.ones((2, 9), np.float32), w, 2, (12, 10), 4)               # weights of another extent
    with pytest.raises(ValueError, match='blend_tiles'):
        ops.blend_tiles(prob.double(), rows, cols, w, w, 2, (12, 10), 4)


def test_tiles_bench_tool_is_importable():
    """tools/volume_tiles_bench.py refuses to time anything without a GPU, and says so"""
    spec = importlib.util.spec_from_file_location('volume_tiles_bench', os.path.join(R.ROOT, 'tools', 'volume_tiles_bench.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    assert callable(mod.main)
    if not torch.cuda.is_available():
        with pytest.raises(SystemExit, match='GPU'):
            mod.main([])
