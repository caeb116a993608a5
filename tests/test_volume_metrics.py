"""Scores in mm of predicted label volumes (RAVD, ASSD, MSSD): csrc/postprocess.hip (mmseg_label_surface, mmseg_distance_to_sites,
mmseg_surface_metrics), ops.label_surface / ops.distance_to_sites / ops.surface_metrics, the `slice_spacing` key of
loaders/volume_folder.py, volume_predictor.py, `--predict_surface`, tools/make_volume_folder.py --slice_spacing and
tools/score_predictions.py, against the scipy restatement of tests/volume_metrics_ref.py.

Comparison rules (set by the feature's issue).  Surfaces and counts are integers: 0 differing voxels, equal counts.  A distance: both
sides take the square root of a sum of three fp64 squares of the same index differences, a few ulp apart, so 1e-12 relative per voxel and
exactly 0 at the sites; the same bar for the maximum.  The sum: at most about 1e6 fp64 terms in another order give at most n * 2^-53,
about 1e-10; the bar sits ten times above that, 1e-9 relative.  Two runs are bitwise equal."""
import json
import os

import numpy as np
import pytest
import torch

from tests import helpers as Hh
from tests import volume_loader_ref as R
from tests import volume_metrics_ref as M
from tests.test_volume_loader import VALUES
from tests.volume_fixtures import _clean_registry, _csv_rows, _dev, _score_tool, _up, device  # noqa: F401

REL_DISTANCE = 1e-12
REL_SUM = 1e-9

# name -> ((S, H, W), (dz, dy, dx) mm, K, classes of the arg-max, sigma).  classes = K + 1 (background and the organs); one class more
# puts a grey value that is no organ into the volume
CASES = {
    '7x40x36': ((7, 40, 36), (5.5, 1.4, 1.7), 4, 5, 3.0),
    '12x53x47': ((12, 53, 47), (7.7, 1.89, 1.2), 4, 5, 3.5),
    '5x64x48': ((5, 64, 48), (9.0, 1.6, 1.6), 4, 5, 4.0),
    'one-slice': ((1, 48, 40), (6.0, 1.5, 1.5), 4, 5, 3.0),
    'odd-45x38': ((6, 45, 38), (6.5, 1.3, 1.9), 4, 5, 3.2),          # H odd, W % 4 = 2
    'k2': ((6, 44, 52), (8.0, 1.7, 1.5), 2, 3, 3.4),
    'other-grey': ((6, 48, 44), (7.0, 1.5, 1.8), 4, 6, 3.6),          # class 5 -> grey value 5, which is background
    '24x160x144': ((24, 160, 144), (3.0, 1.2, 1.2), 4, 5, 4.0),      # H and W longer than one 64-wide tile of a strided pass
}
OTHER_GREY = 5


def _case_data(name):
    """(pred, truth) uint8 [S,H,W], values, spacing: truth from the arg-max over smooth random fields, the prediction from the same
    fields plus 0.35 times a second set"""
    (S, H, W), spacing, K, classes, sigma = CASES[name]
    rng = np.random.RandomState(2000 + sorted(CASES).index(name))
    f = np.concatenate([Hh.smooth_field(rng, S, H, W, sigma=sigma) for _ in range(classes)], axis=-1).astype(np.float64)
    g = np.concatenate([Hh.smooth_field(rng, S, H, W, sigma=sigma) for _ in range(classes)], axis=-1).astype(np.float64)
    values = VALUES[:K]
    grey = np.asarray([0] + values + [OTHER_GREY] * (classes - K - 1), np.uint8)
    return grey[np.argmax(f + 0.35 * g, axis=-1)], grey[np.argmax(f, axis=-1)], values, spacing


def _rel(got, want):
    """largest relative difference; 0 where both are 0 or both +inf"""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    same = (got == want)
    with np.errstate(invalid='ignore', divide='ignore'):
        r = np.where(same, 0.0, np.abs(got - want) / np.abs(want))
    return float(np.max(r)) if r.size else 0.0


# ---- 1, 6: the inputs and the yardstick alone (no GPU) ----------------------------------------------------------------------------------
def test_inputs_are_not_vacuous():
    assert any(c[0][0] == 1 for c in CASES.values()) and any(c[0][2] % 4 and c[0][1] % 2 for c in CASES.values())
    assert any(c[2] == 2 for c in CASES.values()) and any(c[3] > c[2] + 1 for c in CASES.values())
    for name in sorted(CASES):
        pred, truth, values, spacing = _case_data(name)
        table, scores = M.metrics_table(pred, truth, values, spacing), M.chaos_metrics(pred, truth, values, spacing)
        print('%s spacing %s\n%s\nRAVD, ASSD, MSSD:\n%s' % (name, spacing, table, np.round(scores, 3)))
        assert table.shape == (len(values) + 1, 6) and (table[:, 2:4] > 0).all()
        assert (table[:, :2] > 0).all()
        joint = table[-1, :2] / pred.size
        assert (joint > 0.1).all() and (joint < 0.9).all()
        assert np.isfinite(scores).all() and (scores[:, 1] > 0).all() and (scores[:, 2] >= scores[:, 1]).all()
        if CASES[name][3] > CASES[name][2] + 1:
            assert (truth == OTHER_GREY).any() and (pred == OTHER_GREY).any()


def test_a_dropped_axis_is_caught():
    """the yardstick with dz replaced by dy moves ASSD by more than 10 % on every problem of every case with S > 1: no bar of this
    file could hide a kernel that ignores the slice spacing"""
    for name in sorted(CASES):
        pred, truth, values, (dz, dy, dx) = _case_data(name)
        if pred.shape[0] == 1:
            continue
        right, wrong = M.chaos_metrics(pred, truth, values, (dz, dy, dx)), M.chaos_metrics(pred, truth, values, (dy, dy, dx))
        moved = np.abs(wrong[:, 1] - right[:, 1]) / right[:, 1]
        print('%s: ASSD moves by %s %%, MSSD by %s %%' % (name, np.round(100 * moved, 1),
                                                       np.round(100 * np.abs(wrong[:, 2] - right[:, 2]) / right[:, 2], 1)))
        assert (moved > 0.1).all()


# ---- 2, 3: op level on the GPU --------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize('name', sorted(CASES))
def test_label_surface_equals_yardstick(name):
    from multimodal_segmentation_amd import ops
    pred, truth, values, _ = _case_data(name)
    v = _up(np.asarray(values), 'cuda:0', np.int32)
    for volume in (truth, pred):
        got = ops.label_surface(_up(volume, 'cuda:0'), v)
        assert got.dtype == torch.uint8 and tuple(got.shape) == (len(values) + 1,) + volume.shape
        got = got.cpu().numpy()
        want = np.stack([M.surface(m) for m in M.problems(volume, values)], axis=0)
        differing = int(np.count_nonzero(got != want.astype(np.uint8)))
        print('%s: %d differing voxels of %d, surface voxels per problem %s' % (name, differing, want.size, want.reshape(len(want), -1).sum(1)))
        assert differing == 0


def _check_distance(sites, spacing, what):
    from multimodal_segmentation_amd import ops
    got = ops.distance_to_sites(_up(sites.astype(np.uint8), 'cuda:0'), spacing)
    assert got.dtype == torch.float64 and tuple(got.shape) == sites.shape
    got = got.cpu().numpy()
    want = M.distance_map(sites, spacing)
    worst = _rel(got, want)
    print('%s: largest relative difference %.3g over %d voxels, largest distance %.6f mm' % (what, worst, want.size, want.max()))
    assert (got[sites] == 0).all()
    assert worst <= REL_DISTANCE
    return worst


@pytest.mark.gpu
@pytest.mark.parametrize('name', sorted(CASES))
def test_distance_to_sites_equals_edt(name):
    pred, truth, values, spacing = _case_data(name)
    for k, m in enumerate(M.problems(truth, values)):
        _check_distance(M.surface(m), spacing, '%s problem %d' % (name, k))


@pytest.mark.gpu
def test_distance_to_sites_corner_slice_row_and_empty():
    from multimodal_segmentation_amd import ops
    for shape, spacing in (((9, 70, 300), (5.5, 1.4, 1.7)), ((3, 37, 41), (7.7, 1.89, 1.2)), ((1, 20, 530), (2.0, 0.9, 0.7))):
        corner = np.zeros(shape, bool)
        corner[0, 0, 0] = True
        _check_distance(corner, spacing, '%s, one site in a corner' % (shape,))
        far = np.zeros(shape, bool)
        far[-1, -1, -1] = True
        _check_distance(far, spacing, '%s, one site in the far corner' % (shape,))
        rng = np.random.RandomState(7)
        one_slice = np.zeros(shape, bool)
        one_slice[shape[0] // 2] = rng.rand(*shape[1:]) < 0.02
        _check_distance(one_slice, spacing, '%s, sites in one slice' % (shape,))
        one_row = np.zeros(shape, bool)
        one_row[shape[0] - 1, shape[1] // 3] = rng.rand(shape[2]) < 0.2
        _check_distance(one_row, spacing, '%s, sites in one row' % (shape,))
        empty = ops.distance_to_sites(torch.zeros(shape, dtype=torch.uint8, device='cuda:0'), spacing).cpu().numpy()
        assert np.isposinf(empty).all()


# ---- 4, 5: the table and what the host derives from it ----------------------------------------------------------------------------------
def _scores(pred, truth, values, spacing, dev):
    from multimodal_segmentation_amd import ops
    from multimodal_segmentation_amd.volume_predictor import chaos_from_table
    v = _up(np.asarray(values), dev, np.int32)
    table = ops.surface_metrics(_up(pred, dev), _up(truth, dev), v, spacing)
    assert table.dtype == torch.float64 and tuple(table.shape) == (len(values) + 1, 6)
    return table, chaos_from_table(table.cpu().numpy())


@pytest.mark.parametrize('name', sorted(CASES))
def test_surface_metrics_against_yardstick(name, device):
    pred, truth, values, spacing = _case_data(name)
    table, scores = _scores(pred, truth, values, spacing, _dev(device))
    again, _ = _scores(pred, truth, values, spacing, _dev(device))
    assert torch.equal(table, again)                     # two runs, bitwise
    got, want = table.cpu().numpy(), M.metrics_table(pred, truth, values, spacing)
    print('%s: counts\n%s\nsum: relative difference %.3g, max: %.3g' % (name, got[:, :4], _rel(got[:, 4], want[:, 4]), _rel(got[:, 5], want[:, 5])))
    assert np.array_equal(got[:, :4], want[:, :4])
    assert _rel(got[:, 5], want[:, 5]) <= REL_DISTANCE
    assert _rel(got[:, 4], want[:, 4]) <= REL_SUM
    ref = M.chaos_metrics(pred, truth, values, spacing)
    assert _rel(scores[:, 0], ref[:, 0]) <= REL_DISTANCE and _rel(scores[:, 1], ref[:, 1]) <= REL_SUM
    assert _rel(scores[:, 2], ref[:, 2]) <= REL_DISTANCE


def test_known_answers(device):
    dev = _dev(device)
    values, spacing = VALUES[:2], (4.5, 1.25, 1.75)
    pred, truth, _, _ = _case_data('7x40x36')
    _, same = _scores(truth, truth, VALUES, spacing, dev)
    assert np.array_equal(same, np.zeros_like(same))
    box = np.zeros((20, 40, 44), np.uint8)
    box[6:12, 10:22, 12:26] = values[0]
    for shift in ((2, 3, 4), (0, 0, 5), (3, 0, 0), (0, 4, 0)):
        moved = np.roll(box, shift, axis=(0, 1, 2))
        table, scores = _scores(moved, box, values, spacing, dev)
        want = float(np.sqrt(sum((n * s) ** 2 for n, s in zip(shift, spacing))))
        print('shift %s: RAVD %s, ASSD %s, MSSD %s (expected MSSD %.12f)' % (shift, scores[:, 0], scores[:, 1], scores[:, 2], want))
        for k in (0, 2):          # organ 0 and the union; organ 1 is empty on both sides
            assert abs(scores[k, 2] - want) <= REL_DISTANCE * want and scores[k, 0] == 0.0
            if sum(1 for n in shift if n) == 1:
                assert 0.0 < scores[k, 1] < scores[k, 2]
        assert np.isnan(scores[1]).all() and np.array_equal(table.cpu().numpy()[1, :4], np.zeros(4))
    _, empty_pred = _scores(np.zeros_like(box), box, values, spacing, dev)
    assert empty_pred[0, 0] == 100.0 and empty_pred[2, 0] == 100.0 and np.isnan(empty_pred[:, 1:]).all()
    _, empty_truth = _scores(box, np.zeros_like(box), values, spacing, dev)
    assert np.isnan(empty_truth).all()


# ---- 7: ABI ------------------------------------------------------------------------------------------------------------------------------
def test_entry_points_declared_and_bad_arguments_refused():
    from multimodal_segmentation_amd import _native, ops
    protos = _native.parse_header()
    for name in M.STANDINS:
        assert name in protos, name
        assert name.endswith('workspace_doubles') or protos[name][1][-1] == 'void*', name
    assert callable(ops.label_surface) and callable(ops.distance_to_sites) and callable(ops.surface_metrics)
    _native.build()
    lib = _native.load()
    for name in M.STANDINS:
        assert hasattr(lib, name)
    one, bad = 1, 1          # a non-null pointer (a refused call launches nothing and touches no memory); hipErrorInvalidValue
    nan, inf = float('nan'), float('inf')
    assert lib.mmseg_label_surface(one, one, one, None, 2, 8, 8, 17, None) == bad                      # K > 16
    assert lib.mmseg_label_surface(one, one, one, None, 2, 8, 8, 0, None) == bad
    assert lib.mmseg_label_surface(one, one, one, None, 2048, 1024, 1024, 4, None) == bad              # S * H * W = 2^31
    assert lib.mmseg_label_surface(one, one, one, None, 2, 0, 8, 4, None) == bad
    assert lib.mmseg_label_surface(None, one, one, None, 2, 8, 8, 4, None) == bad
    assert lib.mmseg_label_surface(one, None, one, None, 2, 8, 8, 4, None) == bad
    assert lib.mmseg_label_surface(one, one, None, None, 2, 8, 8, 4, None) == bad
    assert lib.mmseg_label_surface(one, one, one, None, 0, 8, 8, 4, None) == 0                         # S = 0: nothing to do
    for spacing in ((0.0, 1.0, 1.0), (1.0, -1.0, 1.0), (1.0, 1.0, nan), (inf, 1.0, 1.0)):
        assert lib.mmseg_distance_to_sites(one, one, one, 2, 8, 8, *(spacing + (None,))) == bad
        assert lib.mmseg_surface_metrics(one, one, one, one, one, 2, 8, 8, 4, *(spacing + (None,))) == bad
    assert lib.mmseg_distance_to_sites(one, one, one, 2048, 1024, 1024, 1.0, 1.0, 1.0, None) == bad
    assert lib.mmseg_distance_to_sites(None, one, one, 2, 8, 8, 1.0, 1.0, 1.0, None) == bad
    assert lib.mmseg_distance_to_sites(one, None, one, 2, 8, 8, 1.0, 1.0, 1.0, None) == bad
    assert lib.mmseg_distance_to_sites(one, one, None, 2, 8, 8, 1.0, 1.0, 1.0, None) == bad
    assert lib.mmseg_distance_to_sites(one, one, one, 0, 8, 8, 1.0, 1.0, 1.0, None) == 0
    assert lib.mmseg_surface_metrics(one, one, one, one, one, 2, 8, 8, 17, 1.0, 1.0, 1.0, None) == bad
    assert lib.mmseg_surface_metrics(one, one, one, one, one, 2048, 1024, 1024, 4, 1.0, 1.0, 1.0, None) == bad
    for i in range(5):
        ptrs = [one] * 5
        ptrs[i] = None
        assert lib.mmseg_surface_metrics(*(ptrs + [2, 8, 8, 4, 1.0, 1.0, 1.0, None])) == bad
    assert lib.mmseg_surface_metrics(one, one, one, one, one, 0, 8, 8, 4, 1.0, 1.0, 1.0, None) == 0
    n = 36 * 320 * 320
    assert lib.mmseg_surface_metrics_workspace_doubles(36, 320, 320, 4) >= 2 * n + (2 * 5 * n + 7) // 8
    assert lib.mmseg_surface_metrics_workspace_doubles(36, 320, 320, 17) == 0
    u8, i32 = torch.zeros(2, 8, 8, dtype=torch.uint8), torch.zeros(4, dtype=torch.int32)
    with pytest.raises(ValueError, match='label_surface'):
        ops.label_surface(torch.zeros(2, 8, 8), i32)
    with pytest.raises(ValueError, match='label_surface'):
        ops.label_surface(u8, torch.zeros(17, dtype=torch.int32))
    with pytest.raises(ValueError, match='distance_to_sites'):
        ops.distance_to_sites(torch.zeros(8, 8, dtype=torch.uint8), (1.0, 1.0, 1.0))
    with pytest.raises(ValueError, match='distance_to_sites'):
        ops.distance_to_sites(u8, (1.0, 0.0, 1.0))
    with pytest.raises(ValueError, match='surface_metrics'):
        ops.surface_metrics(u8, torch.zeros(2, 8, 9, dtype=torch.uint8), i32, (1.0, 1.0, 1.0))
    with pytest.raises(ValueError, match='surface_metrics'):
        ops.surface_metrics(u8, u8, i32.float(), (1.0, 1.0, 1.0))
    with pytest.raises(ValueError, match='surface_metrics'):
        ops.surface_metrics(u8, u8, i32, (1.0, float('nan'), 1.0))


# ---- 8: loader ---------------------------------------------------------------------------------------------------------------------------
@pytest.fixture
def folder(tmp_path):
    out = str(tmp_path / 'volumes')
    R.tool().write_folder(out, volumes=4, size=64, slices=4, seed=3, slice_spacing=(4.0, 9.0))
    return out


@pytest.fixture
def plain_folder(tmp_path):
    out = str(tmp_path / 'plain')
    R.tool().write_folder(out, volumes=4, size=64, slices=4, seed=3)
    return out


def test_loader_reads_slice_spacing(folder, plain_folder, device):
    from multimodal_segmentation_amd.loaders.volume_folder import VolumeFolderLoader
    loader = VolumeFolderLoader(folder)
    seen = []
    for v in (1, 2, 3, 4):
        _, geometry = loader.load_volume_for_prediction(v)
        for mod, geo in zip(loader.modalities, geometry):
            with np.load(os.path.join(folder, geo['file'])) as z:
                assert z['slice_spacing'].dtype == np.float64 and geo['slice_spacing'] == float(z['slice_spacing'])
            assert isinstance(geo['slice_spacing'], float) and 4.0 <= geo['slice_spacing'] <= 9.0
            seen.append(geo['slice_spacing'])
    assert len(set(seen)) == 8
    _, geometry = VolumeFolderLoader(plain_folder).load_volume_for_prediction(1)
    assert [geo['slice_spacing'] for geo in geometry] == [None, None]
    # training ignores the key: the same containers with and without it
    a = VolumeFolderLoader(folder).load_all_modalities_concatenated(0, 'training', 1)
    b = VolumeFolderLoader(plain_folder).load_all_modalities_concatenated(0, 'training', 1)
    assert np.array_equal(a.get_images_modi(0), b.get_images_modi(0)) and np.array_equal(a.get_masks_modi(1), b.get_masks_modi(1))
    name = loader.manifest['volumes']['2']['t2']['file']
    with np.load(os.path.join(folder, name)) as z:
        arrays = {k: z[k] for k in z.files}
    for value in (0.0, -2.5, float('nan'), float('inf')):
        arrays['slice_spacing'] = np.float64(value)
        np.savez_compressed(os.path.join(folder, name), **arrays)
        with pytest.raises(ValueError, match=name.replace('.', r'\.') + '.*slice_spacing'):
            VolumeFolderLoader(folder).load_volume_for_prediction(2)


# ---- 9: end to end -------------------------------------------------------------------------------------------------------------------------
def test_predictor_scores_in_mm(folder, plain_folder, tmp_path, device):
    from multimodal_segmentation_amd.loaders.volume_folder import VolumeFolderLoader
    from multimodal_segmentation_amd.volume_predictor import VolumePredictor
    from tests.test_volume_predict import StubModel, _stub_conf
    K = len(VALUES)
    loader = VolumeFolderLoader(folder)
    manifest = loader.manifest
    assert any('slices' in e[mod] for e in manifest['volumes'].values() for mod in ('t1', 't2'))          # unselected slices occur
    stub = StubModel(loader, _dev(device), [1, 2, 3, 4])

    class Rolled(object):
        modalities = stub.modalities

        def predict_mask(self, modality_index, mode, image_list):
            return torch.roll(stub.predict_mask(modality_index, mode, image_list), 5, dims=2)

    out, out_rolled = str(tmp_path / 'pred'), str(tmp_path / 'rolled')
    VolumePredictor(stub, _stub_conf(3)).run(folder, out)
    VolumePredictor(Rolled(), _stub_conf(3)).run(folder, out_rolled)
    written = json.load(open(os.path.join(out, 'predictions.json')))
    header = 'Vol, RAVD, ASSD, MSSD, ' + ', '.join('%s%d' % (n, k) for k in range(K) for n in ('RAVD', 'ASSD', 'MSSD'))
    for mod in ('t1', 't2'):
        head, rows = _csv_rows(os.path.join(out, 'results_surface_%s.csv' % mod))
        _, rolled = _csv_rows(os.path.join(out_rolled, 'results_surface_%s.csv' % mod))
        assert head == header and len(head.split(', ')) == 3 * (K + 1) + 1
        assert list(rows) == ['1', '2', '3', '4'] and all(len(r) == 3 * (K + 1) for r in rows.values())
        for v in ('1', '2', '3', '4'):
            entry = manifest['volumes'][v][mod]
            with np.load(os.path.join(folder, entry['file'])) as z:
                truth, res, dz = z['label'].copy(), z['resolution'], float(z['slice_spacing'])
            with np.load(os.path.join(out, entry['file'])) as z:
                assert sorted(z.files) == ['label', 'resolution', 'slice_spacing'] and float(z['slice_spacing']) == dz
                pred = z['label']
            assert written['files'][entry['file']]['slice_spacing'] == dz
            a, b = entry.get('slices', [[0, truth.shape[0]]])[0]
            truth[:a], truth[b:] = 0, 0
            want = M.chaos_metrics(pred, truth, VALUES, (dz, res[0], res[1]))
            want = np.concatenate([want[-1:], want[:-1]], axis=0).reshape(-1)          # the union first
            print('volume %s %s, dz %.3f mm: csv %s | yardstick %s | rolled ASSD %s' % (v, mod, dz, rows[v], np.round(want, 4), rolled[v][1]))
            assert rows[v] == ['%.3f' % x for x in want]
            assert float(rolled[v][1]) > float(rows[v][1]) > 0.0
        assert open(os.path.join(out, 'results_native_%s.csv' % mod)).readline().strip() == 'Vol, Dice, Dice0, Dice1, Dice2, Dice3'
    # surface=False, or a folder without slice_spacing: no such file, and the listing of today
    today = sorted(['predictions.json', 'results_native_t1.csv', 'results_native_t2.csv']
                   + [e[mod]['file'] for e in manifest['volumes'].values() for mod in ('t1', 't2')])
    assert sorted(os.listdir(out)) == sorted(today + ['results_surface_t1.csv', 'results_surface_t2.csv'])
    off = str(tmp_path / 'off')
    VolumePredictor(stub, _stub_conf(3)).run(folder, off, surface=False)
    assert sorted(os.listdir(off)) == today
    plain = str(tmp_path / 'plain_pred')
    VolumePredictor(StubModel(VolumeFolderLoader(plain_folder), _dev(device), [1, 2, 3, 4]), _stub_conf(3)).run(plain_folder, plain)
    assert sorted(os.listdir(plain)) == today
    with np.load(os.path.join(plain, 'vol01_t1.npz')) as z:
        assert sorted(z.files) == ['label', 'resolution']
    assert all(sorted(f) == ['modality', 'slices', 'volume'] for f in json.load(open(os.path.join(plain, 'predictions.json')))['files'].values())
    for mod in ('t1', 't2'):          # Dice does not depend on the new key
        assert open(os.path.join(plain, 'results_native_%s.csv' % mod)).read() == open(os.path.join(out, 'results_native_%s.csv' % mod)).read()
    # the tool scores the written folder again, without a model: both files, byte for byte
    again = str(tmp_path / 'again')
    _score_tool().main([out, folder, '--out', again])
    assert sorted(os.listdir(again)) == ['results_native_t1.csv', 'results_native_t2.csv', 'results_surface_t1.csv', 'results_surface_t2.csv']
    for name in sorted(os.listdir(again)):
        assert open(os.path.join(again, name), 'rb').read() == open(os.path.join(out, name), 'rb').read(), name


# ---- 10: options ---------------------------------------------------------------------------------------------------------------------------
def test_cli_options(tmp_path):
    from multimodal_segmentation_amd.experiment import parse_arguments
    base = ['--config', 'dafnet_config_chaos', '--split', '0']
    assert parse_arguments(base).predict_surface is True
    assert parse_arguments(base + ['--predict_surface', 'false']).predict_surface is False
    assert parse_arguments(base + ['--predict_surface', 'true']).predict_surface is True
    with pytest.raises(SystemExit):
        parse_arguments(base + ['--predict_surface', 'perhaps'])
    tool = R.tool()
    a, b = str(tmp_path / 'a'), str(tmp_path / 'b')
    tool.main([a, '--volumes', '3', '--size', '48', '--slices', '3', '--seed', '4'])
    tool.main([b, '--volumes', '3', '--size', '48', '--slices', '3', '--seed', '4', '--slice_spacing', '4', '9'])
    assert json.load(open(os.path.join(a, 'dataset.json'))) == json.load(open(os.path.join(b, 'dataset.json')))
    for name in sorted(os.listdir(a)):
        if name.endswith('.npz'):
            with np.load(os.path.join(a, name)) as za, np.load(os.path.join(b, name)) as zb:
                assert sorted(za.files) == ['image', 'label', 'resolution'] and sorted(zb.files) == sorted(za.files + ['slice_spacing'])
                assert all(np.array_equal(za[k], zb[k]) for k in za.files) and 4.0 <= float(zb['slice_spacing']) <= 9.0
    with pytest.raises(ValueError, match='slice_spacing'):
        tool.write_folder(str(tmp_path / 'c'), volumes=3, slice_spacing=(0.0, 2.0))
