"""Predicted label volumes in each volume's own geometry: csrc/postprocess.hip (mmseg_restore_label, mmseg_label_overlap),
ops.restore_label / ops.label_overlap, loaders/volume_folder.py `load_volume_for_prediction`, volume_predictor.py, the `--predict_*`
options of experiment.py and `tools/make_volume_folder.py --unlabelled`, against the fp64 restatement of tests/volume_predict_ref.py.

Comparison rule (set by the feature's issue): order 0 and every decidable pixel of order 1 must equal the restatement exactly (0
differing pixels); a pixel of order 1 is undecidable when an organ's fp64 probability lies within 1e-5 of 0.5, and at most 0.1 % of
the raw pixels of a case may be (test_restore_inputs_are_decidable)."""
import json
import os

import numpy as np
import pytest
import torch
from scipy import ndimage as ndi

from multimodal_segmentation_amd import nn
from tests import helpers as Hh
from tests import volume_loader_ref as R
from tests import volume_predict_ref as P
from tests.test_volume_loader import SCENARIOS, TARGET, VALUES
from tests.volume_fixtures import device, _clean_registry  # noqa: F401

S = 3


def _cases():
    """name -> (H, W, resolution, (OH, OW), K, C): the eight geometries of SCENARIOS, one with W % 4 != 0 on a 53 x 47 grid, K = 2 of
    C = 3, and K = 4 of C = 8 (organ channels read as one 16-byte load)"""
    out = {}
    for name in sorted(SCENARIOS):
        for i, (H, W, res, _) in enumerate(SCENARIOS[name]['mods']):
            out['%s#%d' % (name, i)] = (H, W, res, SCENARIOS[name]['out'], 4, 5)
    out['53x47'] = (53, 47, (1.5, 2.1), (48, 48), 4, 5)
    out['k2-of-c3'] = (64, 48, (1.6, 1.6), (48, 48), 2, 3)
    out['k4-of-c8'] = (60, 56, (2.2, 1.4), (48, 48), 4, 8)
    return out


CASES = _cases()


def _geometry(H, W, res, out_hw):
    from multimodal_segmentation_amd.loaders.volume_folder import crop_pad_map, resampled_size
    RH, RW = resampled_size(H, res[0], TARGET[0]), resampled_size(W, res[1], TARGET[1])
    return (RH, RW), crop_pad_map(RH, out_hw[0]), crop_pad_map(RW, out_hw[1])


def _case_data(name):
    """a softmax over smooth random fields, fp32 [S,OH,OW,C], seeded per case"""
    H, W, res, out_hw, K, C = CASES[name]
    rng = np.random.RandomState(1000 + sorted(CASES).index(name))
    f = 4.0 * np.concatenate([Hh.smooth_field(rng, S, out_hw[0], out_hw[1], sigma=3.0) for _ in range(C)], axis=-1).astype(np.float64)
    e = np.exp(f - f.max(-1, keepdims=True))
    prob = (e / e.sum(-1, keepdims=True)).astype(np.float32)
    return prob, VALUES[:K], (H, W), _geometry(H, W, res, out_hw)


# ---- the test inputs (no GPU) ----------------------------------------------------------------------------------------------------------
def test_restore_inputs_are_decidable():
    """the restatement alone: per committed case at most 0.1 % of the raw pixels are undecidable, and foreground is neither rare nor
    everything, so the comparison is not vacuous"""
    assert len(CASES) == 11 and any(c[1] % 4 for c in CASES.values()) and any(c[1] % 4 == 0 for c in CASES.values())
    for name in sorted(CASES):
        prob, values, raw_hw, (resampled, rows, cols) = _case_data(name)
        label, undecidable = P.restore(prob, values, raw_hw, resampled, rows, cols, 1)
        label0, undecidable0 = P.restore(prob, values, raw_hw, resampled, rows, cols, 0)
        inside = P.window_mask(raw_hw, resampled, rows, cols)
        fg = np.count_nonzero(label) / float(S * np.count_nonzero(inside))
        print('%s: raw %s -> resampled %s, rows %s cols %s: %d of %d pixels undecidable, %d inside the window per slice, foreground '
              '%.1f %% of them' % (name, raw_hw, resampled, rows, cols, np.count_nonzero(undecidable), label.size,
                                   np.count_nonzero(inside), 100 * fg))
        assert np.count_nonzero(undecidable) <= P.CAP * label.size
        assert not undecidable0.any()
        assert 0.1 < fg < 0.9 and set(np.unique(label).tolist()) <= {0} | set(values)
        assert not label[:, ~inside].any() and not label0[:, ~inside].any()


def test_half_integer_tie_of_the_centre_row():
    """41 -> 54: the centre raw row 20 sits exactly on 26.5 and floor(coord + 0.5) takes 27; 91 -> 58: the outermost raw pixels fall
    outside the resampled frame and are clamped onto its edge"""
    c = P.raw_coordinates(41, 54)
    assert c[20] == 26.5 and np.floor(c[20] + 0.5) == 27
    c = P.raw_coordinates(91, 58)
    assert c[0] == 0.0 and c[90] == 57.0 and 0.0 < c[1] < c[89] < 57.0


# ---- op level -------------------------------------------------------------------------------------------------------------------------
def _restore_on_device(prob, values, raw_hw, geo, order, fill=7):
    """ops.restore_label, and the entry point itself on an output pre-filled with a grey value that is neither 0 nor a label value"""
    from multimodal_segmentation_amd import _native, ops
    resampled, rows, cols = geo
    p = nn.host_to_device(prob, 'cuda:0', np.float32)
    v = nn.host_to_device(np.asarray(values), 'cuda:0', np.int32)
    got = ops.restore_label(p, v, raw_hw, resampled, rows, cols, order)
    out = torch.full((prob.shape[0], raw_hw[0], raw_hw[1]), fill, dtype=torch.uint8, device='cuda:0')
    _native.call('mmseg_restore_label', p, v, out, prob.shape[0], raw_hw[0], raw_hw[1], resampled[0], resampled[1], prob.shape[1],
                 prob.shape[2], *(list(rows) + list(cols) + [prob.shape[3], len(values), order]))
    return got, out


@pytest.mark.gpu
@pytest.mark.parametrize('order', [0, 1])
@pytest.mark.parametrize('name', sorted(CASES))
def test_restore_label_matches_restatement(name, order):
    """0 differing pixels outside the undecidable ones (none for order 0), every output byte written, two runs bitwise equal"""
    prob, values, raw_hw, geo = _case_data(name)
    want, undecidable = P.restore(prob, values, raw_hw, geo[0], geo[1], geo[2], order)
    assert np.count_nonzero(undecidable) <= P.CAP * want.size and (order == 1 or not undecidable.any())
    got, prefilled = _restore_on_device(prob, values, raw_hw, geo, order)
    assert got.dtype == torch.uint8 and tuple(got.shape) == want.shape
    assert torch.equal(got, prefilled)                    # no byte of the pre-filled output survived, and two runs agree
    got = got.cpu().numpy()
    assert set(np.unique(got).tolist()) <= {0} | set(values)
    differing = int(np.count_nonzero((got != want) & ~undecidable))
    print('%s order %d: %d differing pixels of %d compared (%d undecidable left out), foreground %d'
          % (name, order, differing, want.size - np.count_nonzero(undecidable), np.count_nonzero(undecidable), np.count_nonzero(want)))
    assert differing == 0


@pytest.mark.gpu
@pytest.mark.parametrize('order', [0, 1])
def test_constant_probability_gives_a_constant_window(order):
    for name in sorted(CASES):
        H, W, res, out_hw, K, C = CASES[name]
        geo = _geometry(H, W, res, out_hw)
        prob = np.full((2, out_hw[0], out_hw[1], C), 0.1, np.float32)
        prob[..., 1] = 0.7
        got, prefilled = _restore_on_device(prob, VALUES[:K], (H, W), geo, order)
        inside = P.window_mask((H, W), *geo)
        want = np.broadcast_to(np.where(inside, VALUES[1], 0).astype(np.uint8), (2, H, W))
        assert np.array_equal(got.cpu().numpy(), want) and torch.equal(got, prefilled), name
        assert inside.any()


@pytest.mark.gpu
@pytest.mark.parametrize('name', sorted(SCENARIOS))
def test_label_round_trip(name):
    """a raw label through mmseg_preprocess_label and back through restore_label (order 0) is reproduced on every pixel inside the
    window whose 3 x 3 raw neighbourhood carries one label (more than one raw pixel away from a label boundary).  The count compared
    is stated per modality and must exceed half the raw pixels of the scenario: a single geometry cannot always meet that alone (the
    first one of the anisotropic scenario keeps 39 of 69 resampled columns, so only 52 % of its raw pixels lie inside the window)."""
    from multimodal_segmentation_amd import ops
    from tests.test_volume_loader import _run_op, _scenario_data
    sc, raw = _scenario_data(name)
    K = len(VALUES)
    _, masks = _run_op(raw, sc['out'], 'cuda:0')
    values = nn.host_to_device(np.asarray(VALUES), 'cuda:0', np.int32)
    n_compared = n_pixels = 0
    for mod, (image, label, res) in enumerate(raw):
        H, W = label.shape[1:]
        geo = _geometry(H, W, res, sc['out'])
        got = ops.restore_label(masks[..., mod * K:(mod + 1) * K].contiguous(), values, (H, W), geo[0], geo[1], geo[2], 0).cpu().numpy()
        uniform = ndi.maximum_filter(label, size=(1, 3, 3), mode='nearest') == ndi.minimum_filter(label, size=(1, 3, 3), mode='nearest')
        compared = uniform & P.window_mask((H, W), *geo)[None]
        differing = int(np.count_nonzero((got != label) & compared))
        print('%s modality %d: %d differing of %d compared pixels (%d in all), foreground among them %d'
              % (name, mod, differing, np.count_nonzero(compared), label.size, np.count_nonzero(label[compared])))
        assert np.count_nonzero(label[compared]) > 0
        assert differing == 0
        n_compared, n_pixels = n_compared + np.count_nonzero(compared), n_pixels + label.size
    print('%s: %d of %d raw pixels compared' % (name, n_compared, n_pixels))
    assert n_compared > 0.5 * n_pixels


@pytest.mark.gpu
def test_label_overlap_matches_numpy_counts():
    from multimodal_segmentation_amd import ops
    rng = np.random.RandomState(5)
    for (H, W), K in (((53, 47), 4), ((64, 48), 2), ((320, 320), 4), ((37, 61), 16)):
        values = VALUES[:K] if K <= 4 else list(range(10, 10 + K))
        pool = np.asarray([0] + values + [5], np.uint8)                      # 5: a grey value that is no organ
        pred = pool[rng.randint(0, len(pool), size=(4, H, W))]
        truth = pool[rng.randint(0, len(pool), size=(4, H, W))]
        truth[1][truth[1] == values[0]] = 0                                  # a slice with an empty organ ...
        pred[2][pred[2] == values[-1]] = 0                                   # ... on either side
        truth[3] = pred[3]
        v = nn.host_to_device(np.asarray(values), 'cuda:0', np.int32)
        dev = [nn.host_to_device(a, 'cuda:0', np.uint8) for a in (pred, truth)]
        got = ops.label_overlap(dev[0], dev[1], v)
        again = ops.label_overlap(dev[0], dev[1], v)
        want = P.overlap_counts(pred, truth, values)
        assert got.dtype == torch.int32 and torch.equal(got, again)
        assert np.array_equal(got.cpu().numpy(), want), (H, W, K)
        assert want[1, 0, 1] == 0 and want[2, -1, 0] == 0 and np.array_equal(want[3, :, 0], want[3, :, 2])


def test_entry_points_declared_and_bad_geometry_refused():
    """the C ABI declares both entry points, ops exposes them, and the launchers refuse without launching: an axis map that leaves the
    resampled frame or the container, K > C, K > 16, an order outside {0, 1}, sizes beyond the 31-bit index range"""
    from multimodal_segmentation_amd import _native, ops
    protos = _native.parse_header()
    for name in P.STANDINS:
        assert name in protos and protos[name][1][-1] == 'void*', name
    assert 'postprocess.hip' in _native.SOURCES and callable(ops.restore_label) and callable(ops.label_overlap)
    _native.build()
    lib = _native.load()
    one = 1          # stands for a non-null pointer: a refused call launches nothing and touches no memory
    head = [one, one, one, 2, 10, 10, 12, 12, 8, 8]          # S, H, W, RH, RW, OH, OW
    ok_geo = [2, 8, 0, 2, 8, 0]
    bad = hipErrorInvalidValue = 1
    assert lib.mmseg_restore_label(*(head + [6, 8, 0, 2, 8, 0, 5, 4, 1, None])) == bad      # lo + kept > RH
    assert lib.mmseg_restore_label(*(head + [2, 8, 0, -1, 8, 0, 5, 4, 1, None])) == bad     # lo < 0
    assert lib.mmseg_restore_label(*(head + [2, 8, 8, 2, 8, 0, 5, 4, 1, None])) == bad      # before >= OH
    assert lib.mmseg_restore_label(*(head + [2, 8, 0, 2, 8, 1, 5, 4, 1, None])) == bad      # before + kept > OW: outside the container
    assert lib.mmseg_restore_label(*(head + [2, 0, 0, 2, 8, 0, 5, 4, 1, None])) == bad      # nothing kept
    assert lib.mmseg_restore_label(*(head + ok_geo + [3, 4, 1, None])) == bad               # K > C
    assert lib.mmseg_restore_label(*(head + ok_geo + [40, 17, 1, None])) == bad             # K > 16
    assert lib.mmseg_restore_label(*(head + ok_geo + [5, 4, 2, None])) == bad               # order 2
    assert lib.mmseg_restore_label(*(head + ok_geo + [5, 4, -1, None])) == bad
    assert lib.mmseg_restore_label(*([one, one, one, 2, 50000, 50000, 12, 12, 8, 8] + ok_geo + [5, 4, 1, None])) == bad   # H * W >= 2^31
    assert lib.mmseg_restore_label(*([one, one, one, 70000, 10, 10, 12, 12, 8, 8] + ok_geo + [5, 4, 1, None])) == bad     # S > 65535
    assert lib.mmseg_restore_label(*([0, one, one] + head[3:] + ok_geo + [5, 4, 1, None])) == bad                         # null input
    assert lib.mmseg_label_overlap(one, one, one, one, 2, 100, 17, None) == bad
    assert lib.mmseg_label_overlap(one, one, one, one, 2, 0x7fffffff, 4, None) == bad
    assert lib.mmseg_label_overlap(one, one, one, one, 2, 0, 4, None) == bad
    assert lib.mmseg_restore_label(*([one, one, one, 0] + head[4:] + ok_geo + [5, 4, 1, None])) == 0                       # S = 0: nothing to do
    with pytest.raises(ValueError, match='restore_label'):
        ops.restore_label(torch.zeros(1, 8, 8, 3), torch.zeros(4, dtype=torch.int32), (10, 10), (12, 12), (2, 8, 0), (2, 8, 0), 1)
    with pytest.raises(ValueError, match='restore_label'):
        ops.restore_label(torch.zeros(1, 8, 8, 5), torch.zeros(4, dtype=torch.int32), (10, 10), (12, 12), (2, 8, 0), (2, 8, 0), 2)
    with pytest.raises(ValueError, match='label_overlap'):
        ops.label_overlap(torch.zeros(1, 8, 8, dtype=torch.uint8), torch.zeros(1, 8, 9, dtype=torch.uint8), torch.zeros(4, dtype=torch.int32))


# ---- host logic: loader, predictor, tool (CPU stand-in and GPU) ------------------------------------------------------------------------
@pytest.fixture
def folder(tmp_path):
    out = str(tmp_path / 'volumes')
    R.tool().write_folder(out, volumes=4, size=64, slices=4, seed=3)
    return out


@pytest.fixture
def unlabelled(tmp_path):
    """a folder that is only predicted on: files without `label`, no volume in any split"""
    out = str(tmp_path / 'scans')
    R.tool().write_folder(out, volumes=3, size=64, slices=3, seed=11, name='site_c', unlabelled=True)
    path = os.path.join(out, 'dataset.json')
    manifest = json.load(open(path))
    manifest['splits'] = [{'training': [], 'validation': [], 'test': []}]
    json.dump(manifest, open(path, 'w'))
    return out


def test_tool_default_output_is_unchanged_and_unlabelled_drops_the_label(tmp_path):
    """without --unlabelled the tool writes what it wrote before the option existed: the arrays are regenerated here from make_volume
    with the draws in the old order; with it the files lose `label` and nothing else changes"""
    tool = R.tool()
    a, b = str(tmp_path / 'a'), str(tmp_path / 'b')
    m = tool.write_folder(a, volumes=3, size=48, slices=3, seed=4)
    assert m == json.load(open(os.path.join(a, 'dataset.json')))
    assert sorted(m) == ['input_shape', 'label_values', 'modalities', 'name', 'splits', 'target_resolution', 'volumes']
    assert m['name'] == 'chaos' and m['label_values'] == VALUES and m['splits'] == tool.default_splits([1, 2, 3])
    rng = np.random.RandomState(4)
    for v in (1, 2, 3):
        for mod, mod_name in enumerate(('t1', 't2')):
            res = rng.uniform(1.2, 2.4, size=2)
            H, W = [max(8, int(round(48 * rng.uniform(0.85, 1.2) * tool.TARGET_RESOLUTION[i] / res[i]))) for i in range(2)]
            before, after = (0, 0) if mod == 0 else (int(rng.randint(0, 3)), int(rng.randint(0, 3)))
            image, label = tool.make_volume(rng, 1000 * 5 * v - before, mod, before + 3 + after, H, W, VALUES)
            entry = m['volumes'][str(v)][mod_name]
            assert entry == dict({'file': 'vol%02d_%s.npz' % (v, mod_name)}, **({'slices': [[before, before + 3]]} if before or after else {}))
            with np.load(os.path.join(a, entry['file'])) as z:
                assert sorted(z.files) == ['image', 'label', 'resolution']
                assert np.array_equal(z['image'], image) and z['image'].dtype == np.int16
                assert np.array_equal(z['label'], label) and z['label'].dtype == np.uint8
                assert np.array_equal(z['resolution'], res) and z['resolution'].dtype == np.float64
    tool.main([b, '--volumes', '3', '--size', '48', '--slices', '3', '--seed', '4', '--unlabelled'])
    assert json.load(open(os.path.join(b, 'dataset.json'))) == m
    for name in sorted(os.listdir(a)):
        if name.endswith('.npz'):
            with np.load(os.path.join(a, name)) as za, np.load(os.path.join(b, name)) as zb:
                assert sorted(zb.files) == ['image', 'resolution']
                assert np.array_equal(za['image'], zb['image']) and np.array_equal(za['resolution'], zb['resolution'])


def test_unlabelled_folder_loads_for_prediction(unlabelled, folder, device):
    from multimodal_segmentation_amd.loaders.volume_folder import VolumeFolderLoader, read_manifest
    assert read_manifest(unlabelled)['splits'] == [{'training': [], 'validation': [], 'test': []}]
    loader = VolumeFolderLoader(unlabelled)
    assert loader.volumes == [] and sorted(loader.manifest['volumes']) == ['1', '2', '3']
    for v in (1, 2, 3):
        images, geometry = loader.load_volume_for_prediction(v)
        assert len(images) == len(geometry) == 2
        for mod, (x, geo) in enumerate(zip(images, geometry)):
            entry = loader.manifest['volumes'][str(v)][loader.modalities[mod]]
            with np.load(os.path.join(unlabelled, entry['file'])) as z:
                raw, res = z['image'], z['resolution']
            a, b = entry.get('slices', [[0, raw.shape[0]]])[0]
            assert isinstance(x, torch.Tensor) and x.device.type == device and tuple(x.shape) == (3, 64, 64, 1)
            assert geo['file'] == entry['file'] and geo['raw_shape'] == raw.shape and geo['slices'] == list(range(a, b)) and geo['label'] is None
            assert (geo['resampled'], geo['rows'], geo['cols']) == _geometry(raw.shape[1], raw.shape[2], res, (64, 64))
            want, _ = R.preprocess(raw[a:b], np.zeros(raw[a:b].shape, np.uint8), res, TARGET, VALUES, (64, 64))
            assert np.abs(x.cpu().numpy() - want).max() <= 2e-4
            image, label, res2 = loader.read_volume(v, loader.modalities[mod], require_label=False)
            assert label is None and np.array_equal(image, raw[a:b]) and np.array_equal(res2, res)
            with pytest.raises(ValueError, match="no array 'label'"):
                loader.read_volume(v, loader.modalities[mod])
    # the training surface still refuses files without labels, with the error it always gave
    manifest = json.load(open(os.path.join(unlabelled, 'dataset.json')))
    manifest['splits'] = [{'training': [1], 'validation': [2], 'test': [3]}]
    json.dump(manifest, open(os.path.join(unlabelled, 'dataset.json'), 'w'))
    with pytest.raises(ValueError, match="no array 'label'"):
        VolumeFolderLoader(unlabelled).load_all_modalities_concatenated(0, 'training', 1)
    # a labelled folder: the raw label of the selected slices comes along
    lab = VolumeFolderLoader(folder)
    images, geometry = lab.load_volume_for_prediction(2)
    for mod, geo in enumerate(geometry):
        image, label, res = lab.read_volume(2, lab.modalities[mod])
        assert np.array_equal(geo['label'], label) and geo['label'].dtype == np.uint8 and len(geo['slices']) == 4


class StubModel(object):
    """predict_mask returns the preprocessed ground truth of the slices it is shown (organ channels, then background), found by
    matching the images against the containers of every volume; it records the batch sizes it was called with"""

    def __init__(self, loader, device, volumes):
        from multimodal_segmentation_amd import ops
        from multimodal_segmentation_amd.loaders.volume_folder import crop_pad_map
        self.modalities = list(loader.modalities)
        self.known, self.batches = [], []
        values = nn.host_to_device(np.asarray(loader.label_values), device, np.int32)
        K, M = loader.num_masks, len(loader.modalities)
        for v in volumes:
            raw = [loader.read_volume(v, mod) for mod in loader.modalities]
            n = raw[0][0].shape[0]
            images = torch.zeros((n, 64, 64, M), device=device)
            masks = torch.zeros((n, 64, 64, M * K), device=device)
            for mod, (image, label, res) in enumerate(raw):
                resampled, rows, cols = loader.geometry(image.shape[1], image.shape[2], res)
                ops.preprocess_volume(nn.host_to_device(image, device, np.float32), nn.host_to_device(label, device, np.uint8), values,
                                      images, masks, resampled, rows, cols, mod)
            self.known.append((images, masks))
        self.K = K

    def predict_mask(self, modality_index, mode, image_list):
        x = image_list[modality_index]
        assert isinstance(x, torch.Tensor) and mode == 'simple'
        self.batches.append(x.shape[0])
        for images, masks in self.known:
            for off in range(images.shape[0] - x.shape[0] + 1):
                if torch.equal(images[off:off + x.shape[0], ..., modality_index], x[..., 0]):
                    m = masks[off:off + x.shape[0], ..., modality_index * self.K:(modality_index + 1) * self.K]
                    return torch.cat([m, 1 - m.sum(-1, keepdim=True)], dim=-1).contiguous()
        raise AssertionError('slices of no known volume')


def _stub_conf(batch_size=3):
    from multimodal_segmentation_amd.utils.config import EasyDict
    return EasyDict(dict(batch_size=batch_size, input_shape=(64, 64, 1), num_masks=4, folder='nowhere'))


@pytest.mark.parametrize('order', [1, 0])
def test_predictor_writes_volumes_on_their_own_grid_and_scores_them(order, folder, tmp_path, device):
    """one .npz per input file with the file's own shape; slices outside `slices` stay 0 and the selected ones land at their file
    positions, also for out-of-order ranges; the Dice rows equal what the restatement computes for the same stub on the CPU (as printed,
    +- 0.001 for a flipped undecidable pixel) and beat the same prediction rolled by 5 raw pixels along each axis"""
    from multimodal_segmentation_amd.loaders.volume_folder import VolumeFolderLoader
    from multimodal_segmentation_amd.volume_predictor import VolumePredictor
    path = os.path.join(folder, 'dataset.json')
    manifest = json.load(open(path))
    for mod in ('t1', 't2'):          # volume 1: out-of-order ranges of 2 + 2 slices in both modalities
        n = np.load(os.path.join(folder, manifest['volumes']['1'][mod]['file']))['image'].shape[0]
        manifest['volumes']['1'][mod]['slices'] = [[n - 2, n], [0, 2]]
    json.dump(manifest, open(path, 'w'))
    loader = VolumeFolderLoader(folder)
    dev = 'cuda:0' if device == 'cuda' else 'cpu'
    stub = StubModel(loader, dev, [1, 2, 3, 4])
    out = str(tmp_path / 'pred')
    VolumePredictor(stub, _stub_conf(3)).run(folder, out, order=order)
    assert set(stub.batches) == {3, 1}                   # 4 slices in batches of conf.batch_size = 3
    written = json.load(open(os.path.join(out, 'predictions.json')))
    assert written['source_folder'] == folder and written['mode'] == 'simple' and written['order'] == order
    assert written['model_folder'] == 'nowhere'
    npz = sorted(f for f in os.listdir(out) if f.endswith('.npz'))
    assert npz == sorted(e[mod]['file'] for e in manifest['volumes'].values() for mod in ('t1', 't2')) and len(npz) == 8
    rows = {}
    for mod in ('t1', 't2'):
        lines = open(os.path.join(out, 'results_native_%s.csv' % mod)).read().strip().split('\n')
        assert lines[0] == 'Vol, Dice, Dice0, Dice1, Dice2, Dice3' and [l.split(',')[0] for l in lines[1:]] == ['1', '2', '3', '4']
        rows[mod] = {l.split(',')[0]: [float(x) for x in l.split(',')[1:]] for l in lines[1:]}
    for v in ('1', '2', '3', '4'):
        for m, mod in enumerate(('t1', 't2')):
            entry = manifest['volumes'][v][mod]
            with np.load(os.path.join(folder, entry['file'])) as z:
                raw_image, raw_label, res = z['image'], z['label'], z['resolution']
            with np.load(os.path.join(out, entry['file'])) as z:
                assert sorted(z.files) == ['label', 'resolution']
                got, got_res = z['label'], z['resolution']
            assert got.shape == raw_label.shape and got.dtype == np.uint8 and np.array_equal(got_res, res)
            assert set(np.unique(got).tolist()) <= {0} | set(VALUES)
            ranges = entry.get('slices', [[0, raw_label.shape[0]]])
            selected = np.concatenate([np.arange(a, b) for a, b in ranges])
            assert written['files'][entry['file']]['slices'] == selected.tolist()
            rest = np.setdiff1d(np.arange(raw_label.shape[0]), selected)
            assert not got[rest].any() and got[selected].any()
            # the same stub on the CPU: the restatement there (volume_loader_ref) and back (volume_predict_ref)
            geo = _geometry(raw_label.shape[1], raw_label.shape[2], res, (64, 64))
            _, masks = R.preprocess(raw_image[selected], raw_label[selected], res, TARGET, VALUES, (64, 64))
            prob = np.concatenate([masks, 1 - masks.sum(-1, keepdims=True)], axis=-1)
            want, undecidable = P.restore(prob, VALUES, raw_label.shape[1:], geo[0], geo[1], geo[2], order)
            flipped = int(np.count_nonzero(got[selected] != want))
            assert flipped <= np.count_nonzero(undecidable)          # positions too: file position = position of the selected slice
            joint, per_organ = P.dice(raw_label[selected], want, VALUES)
            rolled, _ = P.dice(raw_label[selected], np.roll(got[selected], (5, 5), axis=(1, 2)), VALUES)
            print('volume %s %s order %d: Dice on the raw grid %.3f (restatement %.3f, rolled by 5 pixels %.3f), organs %s, %d pixels '
                  'differ, %d undecidable' % (v, mod, order, rows[mod][v][0], joint, rolled, rows[mod][v][1:], flipped,
                                              np.count_nonzero(undecidable)))
            for a, b in zip(rows[mod][v], [joint] + per_organ):
                assert abs(a - float('%.3f' % b)) <= 0.001 + 1e-9
            assert rows[mod][v][0] > rolled


def test_predictor_on_an_unlabelled_folder_writes_no_scores(unlabelled, folder, tmp_path, device):
    from multimodal_segmentation_amd.loaders.volume_folder import VolumeFolderLoader
    from multimodal_segmentation_amd.volume_predictor import VolumePredictor

    class Blank(object):
        modalities = ['t1', 't2']

        def predict_mask(self, modality_index, mode, image_list):
            p = torch.full(tuple(image_list[0].shape[:3]) + (5,), 0.05, device=image_list[0].device)
            p[..., 2] = 0.8
            return p
    out = str(tmp_path / 'pred')
    VolumePredictor(Blank(), _stub_conf(2)).run(unlabelled, out, volumes=[2, 3], mode='def', order=0)
    assert sorted(os.listdir(out)) == ['predictions.json', 'vol02_t1.npz', 'vol02_t2.npz', 'vol03_t1.npz', 'vol03_t2.npz']
    loader = VolumeFolderLoader(unlabelled)
    for name in ('vol02_t1.npz', 'vol03_t2.npz'):
        with np.load(os.path.join(unlabelled, name)) as z, np.load(os.path.join(out, name)) as p:
            assert p['label'].shape == z['image'].shape and VALUES[2] in p['label'] and set(np.unique(p['label']).tolist()) <= {0, VALUES[2]}
    with pytest.raises(ValueError, match='Unknown mode'):
        VolumePredictor(Blank(), _stub_conf(2)).run(unlabelled, out, mode='maxnostn')
    with pytest.raises(ValueError, match='no volume'):
        VolumePredictor(Blank(), _stub_conf(2)).run(unlabelled, out, volumes=[9])
    assert loader.volumes == []


# ---- end to end: experiment.py --predict_folder ------------------------------------------------------------------------------------------
def test_cli_options():
    from multimodal_segmentation_amd.experiment import parse_arguments
    base = ['--config', 'dafnet_config_chaos', '--split', '0']
    a = parse_arguments(base)
    assert a.predict_folder is None and a.predict_out is None and a.predict_mode == 'simple' and a.predict_order == 1
    a = parse_arguments(base + ['--predict_folder', 'G', '--predict_out', 'O', '--predict_mode', 'max', '--predict_order', '0'])
    assert (a.predict_folder, a.predict_out, a.predict_mode, a.predict_order) == ('G', 'O', 'max', 0)
    with pytest.raises(SystemExit):
        parse_arguments(base + ['--predict_order', '2'])


def test_experiment_predicts_after_training_and_again_from_the_checkpoint(device, folder, unlabelled, tmp_path, monkeypatch):
    from multimodal_segmentation_amd.experiment import Experiment
    from tests.test_volume_loader import _short_run
    monkeypatch.chdir(tmp_path)
    _short_run(monkeypatch)
    base = ['--config', 'dafnet_config_chaos', '--split', '0', '--data_folder', folder]
    run = "dafnet_chaos_l1_['t1', 't2']_split0"
    # a run without the option creates no predictions folder; without a checkpoint --test --predict_folder says so
    Experiment().run(base + ['--test', 'true'])
    assert os.path.isdir(run) and not [f for f in os.listdir(run) if f.startswith('predictions')]
    with pytest.raises(FileNotFoundError, match='no checkpoint'):
        Experiment().run(base + ['--test', 'true', '--predict_folder', unlabelled])
    assert not [f for f in os.listdir(run) if f.startswith('predictions')]
    # the same run folder with the option: train one epoch, test, predict
    Experiment().run(base + ['--predict_folder', unlabelled])
    out = os.path.join(run, 'predictions_site_c')
    names = sorted(os.listdir(out))
    assert names == ['predictions.json'] + ['vol%02d_%s.npz' % (v, m) for v in (1, 2, 3) for m in ('t1', 't2')]
    first = {}
    for name in names[1:]:
        with np.load(os.path.join(unlabelled, name)) as z, np.load(os.path.join(out, name)) as p:
            assert p['label'].shape == z['image'].shape and p['label'].dtype == np.uint8
            assert set(np.unique(p['label']).tolist()) <= {0} | set(VALUES) and np.array_equal(p['resolution'], z['resolution'])
            first[name] = p['label'].copy()
    settings = json.load(open(os.path.join(out, 'predictions.json')))
    assert settings['source_folder'] == unlabelled and settings['model_folder'] == run and settings['mode'] == 'simple'
    os.rename(out, out + '_first')
    Experiment().run(base + ['--test', 'true', '--predict_folder', unlabelled])
    for name in names[1:]:
        with np.load(os.path.join(out, name)) as p:
            assert np.array_equal(p['label'], first[name]), name
    # labelled volumes and another place to write to
    other = str(tmp_path / 'elsewhere')
    Experiment().run(base + ['--test', 'true', '--predict_folder', folder, '--predict_out', other, '--predict_order', '0'])
    rows = open(os.path.join(other, 'results_native_t2.csv')).read().strip().split('\n')
    assert rows[0] == 'Vol, Dice, Dice0, Dice1, Dice2, Dice3' and [r.split(',')[0] for r in rows[1:]] == ['1', '2', '3', '4']
    assert all(0.0 <= float(x) <= 1.0 for r in rows[1:] for x in r.split(',')[1:])
