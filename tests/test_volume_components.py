"""Each organ's largest connected component in predicted label volumes: csrc/postprocess.hip (mmseg_label_components,
mmseg_keep_largest_components), ops.label_components / ops.keep_largest_components, `components='largest'` of volume_predictor.py,
`--predict_components` / `--predict_connectivity` and tools/score_predictions.py --components, against the scipy restatement of
tests/volume_components_ref.py.

Comparison rule (set by the feature's issue).  Everything is an integer: 0 differing voxels in `comp` and `out`, equal `stats`, and two
runs are bitwise equal."""
import functools
import json
import os
import zipfile

import numpy as np
import pytest
import torch

from tests import volume_components_ref as C
from tests import volume_loader_ref as R
from tests import volume_metrics_ref as M
from tests.test_volume_loader import VALUES
from tests.test_volume_metrics import CASES, OTHER_GREY, _case_data
from tests.volume_fixtures import _clean_registry, _csv_rows, _dev, _score_tool, _up, device  # noqa: F401

CONNECTIVITIES = (6, 26)
KNOWN_SHAPES = ((12, 53, 47), (3, 37, 41))          # no tile size divides them


@functools.lru_cache(maxsize=None)
def _volume(name):
    """the `pred` side of tests.test_volume_metrics._case_data"""
    pred, _, values, _ = _case_data(name)
    pred.setflags(write=False)
    return pred, tuple(values)


@functools.lru_cache(maxsize=None)
def _reference(name, connectivity):
    """(comp, out, stats) of the yardstick, computed once per case and connectivity and never written to"""
    pred, values = _volume(name)
    comp = C.components(pred, values, connectivity)
    out, stats = C.keep_largest(pred, values, connectivity)
    for a in (comp, out, stats):
        a.setflags(write=False)
    return comp, out, stats


def _run(volume, values, connectivity, dev):
    """(comp, out, stats) as numpy through the two ops, each run twice: the second run must be bitwise equal"""
    from multimodal_segmentation_amd import ops
    x, v = _up(volume, dev), _up(np.asarray(values), dev, np.int32)
    comp, again = ops.label_components(x, v, connectivity), ops.label_components(x, v, connectivity)
    assert comp.dtype == torch.int32 and tuple(comp.shape) == volume.shape and torch.equal(comp, again)
    out, stats = ops.keep_largest_components(x, v, connectivity)
    out2, stats2 = ops.keep_largest_components(x, v, connectivity)
    assert out.dtype == torch.uint8 and tuple(out.shape) == volume.shape and torch.equal(out, out2)
    assert stats.dtype == torch.int32 and tuple(stats.shape) == (len(values), 3) and torch.equal(stats, stats2)
    return comp.cpu().numpy(), out.cpu().numpy(), stats.cpu().numpy()


# ---- the inputs and the yardstick alone (no GPU) ----------------------------------------------------------------------------------------
def test_inputs_are_not_vacuous():
    """every organ of every case has at least 3 components, a strict winner and something to remove, at both connectivities; and the
    yardstick with the wrong connectivity labels every case with S > 1 differently, so a kernel that ignores the argument cannot pass"""
    assert any(c[0][0] == 1 for c in CASES.values()) and any(c[0][2] % 4 == 2 and c[0][1] % 2 for c in CASES.values())
    assert any(c[2] == 2 for c in CASES.values()) and any(c[3] > c[2] + 1 for c in CASES.values())
    assert any(c[0][0] > 4 and c[0][1] > 16 and c[0][2] > 64 for c in CASES.values())          # several tiles on every axis
    for name in sorted(CASES):
        pred, values = _volume(name)
        if CASES[name][3] > CASES[name][2] + 1:
            assert (pred == OTHER_GREY).any() and OTHER_GREY not in values
        for connectivity in CONNECTIVITIES:
            _, out, stats = _reference(name, connectivity)
            for k, v in enumerate(values):
                sizes = C.sorted_sizes(pred, v, connectivity)
                print('%s organ %d, connectivity %d: %d components, largest %d, second %d, %d of %d voxels removed'
                      % (name, v, connectivity, len(sizes), sizes[0], sizes[1], stats[k, 1] - stats[k, 2], stats[k, 1]))
                assert len(sizes) >= 3 and sizes[0] > sizes[1]
                assert tuple(stats[k]) == (len(sizes), sum(sizes), sizes[0]) and stats[k, 1] - stats[k, 2] >= 1
                assert int(np.count_nonzero(out == v)) == sizes[0]
            assert np.array_equal(out[~np.isin(pred, values)], pred[~np.isin(pred, values)])
        if pred.shape[0] > 1:
            assert not np.array_equal(_reference(name, 6)[0], _reference(name, 26)[0])


# ---- the random volumes: all eight cases, both connectivities ------------------------------------------------------------------------
@pytest.mark.parametrize('connectivity', CONNECTIVITIES)
@pytest.mark.parametrize('name', sorted(CASES))
def test_components_and_filter_equal_yardstick(name, connectivity, device):
    pred, values = _volume(name)
    want_comp, want_out, want_stats = _reference(name, connectivity)
    comp, out, stats = _run(pred, values, connectivity, _dev(device))
    d_comp, d_out = int(np.count_nonzero(comp != want_comp)), int(np.count_nonzero(out != want_out))
    print('%s, connectivity %d: %d differing voxels in comp, %d in out, of %d; stats\n%s\nyardstick\n%s'
          % (name, connectivity, d_comp, d_out, pred.size, stats, want_stats))
    assert d_comp == 0
    assert d_out == 0
    assert np.array_equal(stats, want_stats)


# ---- known answers ---------------------------------------------------------------------------------------------------------------------
def _serpentine(shape, v):
    """even slices: even rows full, odd rows one voxel at alternating ends; odd slices: one voxel that joins its two neighbours"""
    S, H, W = shape
    vol = np.zeros(shape, np.uint8)
    for s in range(0, S, 2):
        vol[s, 0::2, :] = v
        for y in range(1, H, 2):
            vol[s, y, W - 1 if (y // 2) % 2 == 0 else 0] = v
    for s in range(1, S, 2):
        if (s // 2) % 2 == 0:
            vol[s, H - 1, W - 1] = v
        else:
            vol[s, 0, 0] = v
    return vol


@pytest.mark.parametrize('shape', KNOWN_SHAPES)
def test_serpentine_is_one_component(shape, device):
    """one long thin body through every tile: a propagation scheme with a cap on its rounds, or a broken merge across tiles, splits it"""
    v = VALUES[1]
    vol = _serpentine(shape, v)
    n = int(np.count_nonzero(vol))
    assert shape[1] % 2 == 1 and n > shape[0] // 2 * (shape[1] // 2) * shape[2]
    for connectivity in CONNECTIVITIES:
        comp, out, stats = _run(vol, VALUES, connectivity, _dev(device))
        assert np.array_equal(comp, (vol == v).astype(np.int32))          # 1 everywhere on it, 0 elsewhere
        assert np.array_equal(out, vol)
        assert np.array_equal(stats, np.asarray([[0, 0, 0], [1, n, n], [0, 0, 0], [0, 0, 0]], np.int32))


@pytest.mark.parametrize('shape', KNOWN_SHAPES)
def test_checkerboard(shape, device):
    v = VALUES[0]
    s, y, x = np.indices(shape)
    vol = np.where((s + y + x) % 2 == 0, v, 0).astype(np.uint8)
    n = int(np.count_nonzero(vol))
    index = np.arange(vol.size, dtype=np.int32).reshape(shape)
    comp, out, stats = _run(vol, VALUES[:2], 6, _dev(device))
    assert np.array_equal(comp, np.where(vol == v, index + 1, 0))          # every voxel its own component
    only_first = np.zeros(shape, np.uint8)
    only_first[0, 0, 0] = v                                                # all of size 1: the smallest index stays
    assert np.array_equal(out, only_first)
    assert np.array_equal(stats, np.asarray([[n, n, 1], [0, 0, 0]], np.int32))
    comp, out, stats = _run(vol, VALUES[:2], 26, _dev(device))
    assert np.array_equal(comp, (vol == v).astype(np.int32))
    assert np.array_equal(out, vol)
    assert np.array_equal(stats, np.asarray([[1, n, n], [0, 0, 0]], np.int32))


@pytest.mark.parametrize('shape', KNOWN_SHAPES)
def test_of_two_equal_boxes_the_one_with_the_smaller_index_stays(shape, device):
    v = VALUES[2]
    size = (1, 5, 6)
    for axis in range(3):
        first, second = [0, 3, 4], [0, 3, 4]
        second[axis] = shape[axis] - size[axis] - (0 if axis == 0 else 2)          # the same box, moved along `axis` only
        a, b = np.zeros(shape, bool), np.zeros(shape, bool)
        a[tuple(slice(o, o + n) for o, n in zip(first, size))] = True
        b[tuple(slice(o, o + n) for o, n in zip(second, size))] = True
        assert a.sum() == b.sum() == 30 and not (a & b).any()
        assert C.components((a | b).astype(np.uint8), [1], 26).max() > 1          # apart: two components at either connectivity
        for flipped in (False, True):
            boxes = [np.flip(m, axis) if flipped else m for m in (a, b)]
            vol = np.where(boxes[0] | boxes[1], v, 0).astype(np.uint8)
            stays = min(boxes, key=lambda m: int(np.flatnonzero(m)[0]))
            assert stays is (boxes[1] if flipped else boxes[0])
            for connectivity in CONNECTIVITIES:
                comp, out, stats = _run(vol, VALUES, connectivity, _dev(device))
                assert np.array_equal(out, np.where(stays, v, 0).astype(np.uint8))
                assert np.array_equal(stats[2], (2, 60, 30)) and not stats[[0, 1, 3]].any()
                assert sorted(np.unique(comp)) == sorted([0] + [int(np.flatnonzero(m)[0]) + 1 for m in boxes])


@pytest.mark.parametrize('shape', KNOWN_SHAPES)
def test_two_organs_face_to_face_and_a_foreign_grey_value(shape, device):
    va, vb = VALUES[0], VALUES[3]
    vol = np.zeros(shape, np.uint8)
    vol[0:3, 5:15, 5:12] = va
    vol[0:3, 5:15, 12:20] = vb          # touches organ a along a whole face: another grey value, so no merge
    na, nb = 3 * 10 * 7, 3 * 10 * 8
    for connectivity in CONNECTIVITIES:
        comp, out, stats = _run(vol, VALUES, connectivity, _dev(device))
        assert np.array_equal(out, vol)
        assert np.array_equal(stats, np.asarray([[1, na, na], [0, 0, 0], [0, 0, 0], [1, nb, nb]], np.int32))
        want = np.zeros(shape, np.int32)
        want[vol == va] = int(np.flatnonzero(vol == va)[0]) + 1
        want[vol == vb] = int(np.flatnonzero(vol == vb)[0]) + 1
        assert np.array_equal(comp, want)
    # a grey value that is no organ between an organ's body and its island: copied, no bridge, comp 0
    vol = np.zeros(shape, np.uint8)
    vol[1:3, 20:34, 3:18] = va
    vol[1:3, 24:30, 18:22] = OTHER_GREY
    vol[1:3, 25:28, 22:25] = va
    body, island = 2 * 14 * 15, 2 * 3 * 3
    for connectivity in CONNECTIVITIES:
        comp, out, stats = _run(vol, VALUES, connectivity, _dev(device))
        want = vol.copy()
        want[1:3, 25:28, 22:25] = 0
        assert np.array_equal(out, want) and (out == OTHER_GREY).sum() == 2 * 6 * 4
        assert (comp[vol == OTHER_GREY] == 0).all() and (comp[vol == 0] == 0).all() and (comp[vol == va] > 0).all()
        assert len(np.unique(comp[vol == va])) == 2
        assert np.array_equal(stats, np.asarray([[2, body + island, body], [0, 0, 0], [0, 0, 0], [0, 0, 0]], np.int32))


def test_empty_cases(device):
    from multimodal_segmentation_amd import ops
    dev = _dev(device)
    for shape in KNOWN_SHAPES:
        comp, out, stats = _run(np.zeros(shape, np.uint8), VALUES, 6, dev)
        assert not comp.any() and not out.any() and not stats.any()
        vol = np.full(shape, VALUES[1], np.uint8)          # one organ fills the volume, the others are empty
        comp, out, stats = _run(vol, VALUES, 26, dev)
        assert (comp == 1).all() and np.array_equal(out, vol)
        assert np.array_equal(stats, np.asarray([[0, 0, 0], [1, vol.size, vol.size], [0, 0, 0], [0, 0, 0]], np.int32))
    v = _up(np.asarray(VALUES), dev, np.int32)
    none = torch.zeros((0, 8, 9), dtype=torch.uint8, device=dev)
    comp = ops.label_components(none, v)
    out, stats = ops.keep_largest_components(none, v, 26)
    assert tuple(comp.shape) == (0, 8, 9) and comp.dtype == torch.int32
    assert tuple(out.shape) == (0, 8, 9) and out.dtype == torch.uint8
    assert tuple(stats.shape) == (4, 3) and stats.dtype == torch.int32 and not stats.any()


@pytest.mark.parametrize('shape', KNOWN_SHAPES)
def test_a_component_through_the_slice_axis(shape, device):
    """one voxel per slice, stacked: S voxels on the file grid, against S - 1 voxels side by side in one slice"""
    from multimodal_segmentation_amd.volume_predictor import keep_largest
    dev = _dev(device)
    S, H, W = shape
    v = VALUES[3]
    vol = np.zeros(shape, np.uint8)
    vol[:, H - 2, W - 3] = v
    vol[0, 1, 2:2 + S - 1] = v
    want = vol.copy()
    want[0, 1, :] = 0
    for connectivity in CONNECTIVITIES:
        comp, out, stats = _run(vol, VALUES, connectivity, dev)
        assert np.array_equal(out, want) and np.array_equal(stats[3], (2, 2 * S - 1, S))
    # the same slices with a gap in the file: the stack falls into pieces smaller than the row, which then stays
    for gap in range(1, S):
        slices = list(range(gap)) + list(range(gap + 1, S + 1))
        pieces = max(gap, S - gap)
        geometry = dict(raw_shape=(S + 1, H, W), slices=slices)
        kept, stats = keep_largest(_up(vol, dev), _up(np.asarray(VALUES), dev, np.int32), geometry, 6)
        kept, stats = kept.cpu().numpy(), stats.cpu().numpy()
        on_grid = np.zeros((S + 1, H, W), np.uint8)
        on_grid[slices] = vol
        ref, ref_stats = C.keep_largest(on_grid, VALUES, 6)
        assert np.array_equal(kept, ref[slices]) and np.array_equal(stats, ref_stats)
        if pieces < S - 1:
            assert np.array_equal(kept, np.where(want, 0, vol)) and np.array_equal(stats[3], (3, 2 * S - 1, S - 1))


# ---- end to end -----------------------------------------------------------------------------------------------------------------------
@pytest.fixture
def folder(tmp_path):
    """the folder of test_volume_metrics, with every organ of the truth made one body (the tool draws the ellipses of every slice
    anew, so its organs come in pieces, and a filter that drops a true piece is then scored worse for it): unselected slices are
    zeroed, which no score reads, and the yardstick's filter is applied to what is left"""
    out = str(tmp_path / 'volumes')
    manifest = R.tool().write_folder(out, volumes=4, size=64, slices=4, seed=3, slice_spacing=(4.0, 9.0))
    for entry in manifest['volumes'].values():
        for e in entry.values():
            with np.load(os.path.join(out, e['file'])) as z:
                arrays = {k: z[k] for k in z.files}
            a, b = e.get('slices', [[0, arrays['label'].shape[0]]])[0]
            arrays['label'][:a], arrays['label'][b:] = 0, 0
            arrays['label'] = C.keep_largest(arrays['label'], VALUES, 6)[0]
            np.savez_compressed(os.path.join(out, e['file']), **arrays)
    return out


def _file_contents(path):
    """the bytes of a file; of an .npz the names and the bytes of its members (the archive itself also stores the time of writing)"""
    if path.endswith('.npz'):
        with zipfile.ZipFile(path) as z:
            return [(i.filename, z.read(i.filename)) for i in z.infolist()]
    return open(path, 'rb').read()


def _with_islands(stub, K):
    """the stub's probabilities plus two small far-away blobs per organ, in every slice"""
    class Islands(object):
        modalities = stub.modalities

        def predict_mask(self, modality_index, mode, image_list):
            p = stub.predict_mask(modality_index, mode, image_list).clone()
            for k in range(K):
                for r0 in (9, 53):
                    p[:, r0:r0 + 2, 9 + 12 * k:11 + 12 * k, :] = 0.0
                    p[:, r0:r0 + 2, 9 + 12 * k:11 + 12 * k, k] = 1.0
            return p
    return Islands()


def test_predictor_keeps_the_largest_components(folder, tmp_path, device):
    from multimodal_segmentation_amd.loaders.volume_folder import VolumeFolderLoader
    from multimodal_segmentation_amd.volume_predictor import VolumePredictor
    from tests.test_volume_predict import StubModel, _stub_conf
    K = len(VALUES)
    loader = VolumeFolderLoader(folder)
    manifest = loader.manifest
    assert any('slices' in e[mod] for e in manifest['volumes'].values() for mod in ('t1', 't2'))          # unselected slices occur
    model = _with_islands(StubModel(loader, _dev(device), [1, 2, 3, 4]), K)
    plain, omitted, kept = str(tmp_path / 'plain'), str(tmp_path / 'omitted'), str(tmp_path / 'kept')
    VolumePredictor(model, _stub_conf(3)).run(folder, plain, components=None)
    VolumePredictor(model, _stub_conf(3)).run(folder, omitted)
    VolumePredictor(model, _stub_conf(3)).run(folder, kept, components='largest')
    # components=None: the listing and every file of a run without the argument; no new key
    today = sorted(['predictions.json'] + ['results_%s_%s.csv' % (a, b) for a in ('native', 'surface') for b in ('t1', 't2')]
                   + [e[mod]['file'] for e in manifest['volumes'].values() for mod in ('t1', 't2')])
    assert sorted(os.listdir(plain)) == sorted(os.listdir(omitted)) == today
    for name in today:
        if name != 'predictions.json':
            assert _file_contents(os.path.join(plain, name)) == _file_contents(os.path.join(omitted, name)), name
    settings = [json.load(open(os.path.join(d, 'predictions.json'))) for d in (plain, omitted, kept)]
    assert sorted(settings[0]) == sorted(settings[1]) == ['files', 'label_values', 'mode', 'model_folder', 'order', 'source_folder']
    assert settings[0] == settings[1]
    assert sorted(settings[2]) == sorted(list(settings[0]) + ['components', 'connectivity'])
    assert settings[2]['components'] == 'largest' and settings[2]['connectivity'] == 6 and settings[2]['files'] == settings[0]['files']
    # components='largest': one more file per modality, and everything follows from the yardstick's filter of the plain run's volumes
    assert sorted(os.listdir(kept)) == sorted(today + ['results_components_t1.csv', 'results_components_t2.csv'])
    header = 'Vol, ' + ', '.join('%s%d' % (n, k) for k in range(K) for n in ('N', 'Before', 'Kept'))
    for mod in ('t1', 't2'):
        head, comps = _csv_rows(os.path.join(kept, 'results_components_%s.csv' % mod))
        _, surface = _csv_rows(os.path.join(kept, 'results_surface_%s.csv' % mod))
        _, surface_plain = _csv_rows(os.path.join(plain, 'results_surface_%s.csv' % mod))
        assert head == header and list(comps) == list(surface) == ['1', '2', '3', '4']
        for v in ('1', '2', '3', '4'):
            entry = manifest['volumes'][v][mod]
            with np.load(os.path.join(folder, entry['file'])) as z:
                truth, res, dz = z['label'].copy(), z['resolution'], float(z['slice_spacing'])
            with np.load(os.path.join(plain, entry['file'])) as z:
                before = z['label']
            with np.load(os.path.join(kept, entry['file'])) as z:
                assert sorted(z.files) == ['label', 'resolution', 'slice_spacing']
                after = z['label']
            want, stats = C.keep_largest(before, VALUES, 6)
            assert after.dtype == np.uint8 and np.array_equal(after, want)
            assert (stats[:, 0] >= 2).all() and (stats[:, 2] < stats[:, 1]).all()          # the blobs are there, and they go
            assert comps[v] == ['%d' % x for x in stats.reshape(-1)]
            a, b = entry.get('slices', [[0, truth.shape[0]]])[0]
            truth[:a], truth[b:] = 0, 0
            scores = M.chaos_metrics(want, truth, VALUES, (dz, res[0], res[1]))
            scores = np.concatenate([scores[-1:], scores[:-1]], axis=0).reshape(-1)          # the union first
            print('volume %s %s: components %s | MSSD %s mm, without the filter %s mm' % (v, mod, comps[v], surface[v][2], surface_plain[v][2]))
            assert surface[v] == ['%.3f' % x for x in scores]
            assert float(surface[v][2]) < float(surface_plain[v][2])
    # the tool filters the volumes written without the filter and scores them: the filtered run's two files, byte for byte
    again = str(tmp_path / 'again')
    _score_tool().main([plain, folder, '--out', again, '--components', 'largest'])
    assert sorted(os.listdir(again)) == ['results_%s_%s.csv' % (a, b) for a in ('native', 'surface') for b in ('t1', 't2')]
    for name in sorted(os.listdir(again)):
        assert open(os.path.join(again, name), 'rb').read() == open(os.path.join(kept, name), 'rb').read(), name
    with pytest.raises(ValueError, match='components'):
        VolumePredictor(model, _stub_conf(3)).run(folder, str(tmp_path / 'no'), components='all')
    with pytest.raises(ValueError, match='connectivity'):
        VolumePredictor(model, _stub_conf(3)).run(folder, str(tmp_path / 'no'), components='largest', connectivity=18)
    assert not os.path.exists(str(tmp_path / 'no'))


def test_cli_options():
    from multimodal_segmentation_amd.experiment import parse_arguments
    base = ['--config', 'dafnet_config_chaos', '--split', '0']
    a = parse_arguments(base)
    assert a.predict_components == 'none' and a.predict_connectivity == 6
    a = parse_arguments(base + ['--predict_components', 'largest', '--predict_connectivity', '26'])
    assert a.predict_components == 'largest' and a.predict_connectivity == 26
    for bad in (['--predict_components', 'all'], ['--predict_connectivity', '18'], ['--predict_connectivity', 'faces']):
        with pytest.raises(SystemExit):
            parse_arguments(base + bad)
    tool = _score_tool()
    for bad in (['--components', 'none'], ['--connectivity', '18']):
        with pytest.raises(SystemExit):
            tool.main(['a', 'b'] + bad)


# ---- ABI ----------------------------------------------------------------------------------------------------------------------------------
def test_entry_points_declared_and_bad_arguments_refused():
    from multimodal_segmentation_amd import _native, ops
    protos = _native.parse_header()
    for name in C.STANDINS:
        assert name in protos, name
        assert name.endswith('workspace_bytes') or protos[name][1][-1] == 'void*', name
    assert callable(ops.label_components) and callable(ops.keep_largest_components)
    _native.build()
    lib = _native.load()
    for name in C.STANDINS:
        assert hasattr(lib, name)
    one, bad = 8, 1          # a non-null pointer (a refused call launches nothing and touches no memory); hipErrorInvalidValue
    label, keep = lib.mmseg_label_components, lib.mmseg_keep_largest_components
    for S, H, W, K, conn in ((2, 8, 8, 17, 6), (2, 8, 8, 0, 6), (2, 0, 8, 4, 6), (2, 8, 0, 4, 26), (2048, 1024, 1024, 4, 6),
                             (1, 2 ** 31 - 1, 1, 4, 6), (2, 8, 8, 4, 18), (2, 8, 8, 4, 0), (2, 8, 8, 4, 8)):
        assert label(one, one, one, S, H, W, K, conn, None) == bad, (S, H, W, K, conn)
        assert keep(one, one, one, one, one, S, H, W, K, conn, None) == bad, (S, H, W, K, conn)
    for i in range(3):
        ptrs = [one] * 3
        ptrs[i] = None
        assert label(*(ptrs + [2, 8, 8, 4, 6, None])) == bad
    for i in range(5):
        ptrs = [one] * 5
        ptrs[i] = None
        assert keep(*(ptrs + [2, 8, 8, 4, 26, None])) == bad
    assert label(one, one, one, 0, 8, 8, 4, 6, None) == 0                          # S = 0: nothing to do
    assert keep(one, one, one, one, one, 0, 8, 8, 4, 6, None) == 0
    n = 36 * 320 * 320
    assert lib.mmseg_keep_largest_workspace_bytes(36, 320, 320, 4) >= 4 * n
    assert lib.mmseg_keep_largest_workspace_bytes(36, 320, 320, 17) == 0
    assert lib.mmseg_keep_largest_workspace_bytes(2048, 1024, 1024, 4) == 0
    assert lib.mmseg_keep_largest_workspace_bytes(2, 0, 8, 4) == 0
    u8, i32 = torch.zeros(2, 8, 8, dtype=torch.uint8), torch.zeros(4, dtype=torch.int32)
    for name, op in (('label_components', ops.label_components), ('keep_largest_components', ops.keep_largest_components)):
        with pytest.raises(ValueError, match=name):
            op(torch.zeros(2, 8, 8), i32)
        with pytest.raises(ValueError, match=name):
            op(torch.zeros(8, 8, dtype=torch.uint8), i32)
        with pytest.raises(ValueError, match=name):
            op(u8, i32.float())
        with pytest.raises(ValueError, match=name):
            op(u8, torch.zeros(17, dtype=torch.int32))
        with pytest.raises(ValueError, match=name):
            op(u8, i32, 18)
