"""The enclosed holes of every organ of a predicted label volume, filled on the device: csrc/postprocess.hip (mmseg_fill_label_holes),
ops.fill_label_holes, volume_predictor.fill_holes, `fill_holes='2d' | '3d'` of VolumePredictor.run and score_folder,
`--predict_fill_holes` and tools/score_predictions.py --fill_holes, against the scipy restatement of tests/volume_holes_ref.py.

Comparison rule (set by the feature's issue).  Everything is an integer: 0 differing voxels in `out`, equal `stats`, and the second of
two runs is bitwise equal to the first.  No tolerance and no excluded voxels."""
import functools
import importlib.util
import json
import logging
import os

import numpy as np
import pytest
import torch
from scipy import ndimage as ndi

from tests import volume_components_ref as C
from tests import volume_holes_ref as F
from tests import volume_loader_ref as R
from tests import volume_metrics_ref as M
from tests import volume_predict_ref as P
from tests.test_volume_components import _file_contents, _serpentine, folder  # noqa: F401
from tests.test_volume_loader import VALUES
from tests.test_volume_metrics import CASES, OTHER_GREY, _case_data
from tests.volume_fixtures import _clean_registry, _csv_rows, _dev, _score_tool, _up, device  # noqa: F401

KNOWN_SHAPES = ((12, 53, 47), (3, 37, 41))          # no tile size divides them
DENSE = ('24x160x144', 'k2')
GRID_CAP = 4096 * 256                               # CC_MAXBLK * PO_BLOCK of csrc/postprocess.hip: where the grid-stride loops wrap
PAST_CAP = (23, 230, 219)
PREFILL = 7                                         # neither 0 nor a label value nor OTHER_GREY


@pytest.fixture
def dev(device, monkeypatch):
    """the shared `device` fixture, with the stand-ins of the hole filling on top of its table"""
    if device == 'cpu':
        from tests import cpu_backend as cb
        for name, fn in F.STANDINS.items():
            monkeypatch.setitem(cb._TABLE, name, fn)
    return _dev(device)


# ---- the inputs --------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _punched(name):
    """the `pred` side of tests.test_volume_metrics._case_data with random small boxes erased (every eighth one to OTHER_GREY) and, per
    organ, up to six sealed cavities: a voxel whose 3 x 5 x 5 neighbourhood (1 x 5 x 5 in a single slice) is the organ, that
    neighbourhood sealed again and a 1 x (1..3) x (1..3) box punched at its centre, one in three with a foreign grey value, one in
    three with a voxel of the next organ in the middle"""
    pred, _, values, _ = _case_data(name)
    rng = np.random.RandomState(4000 + sorted(CASES).index(name))
    vol = pred.copy()
    S, H, W = vol.shape
    for i in range(max(8, vol.size // 150)):
        d = (rng.randint(1, 3), rng.randint(1, 4), rng.randint(1, 4))
        o = [rng.randint(0, n - min(n, e) + 1) for n, e in zip(vol.shape, d)]
        vol[o[0]:o[0] + d[0], o[1]:o[1] + d[1], o[2]:o[2] + d[2]] = OTHER_GREY if i % 8 == 7 else 0
    hz = 1 if S >= 3 else 0
    for k, v in enumerate(values):
        core = np.argwhere(ndi.binary_erosion(vol == v, np.ones((2 * hz + 1, 5, 5), bool)))
        for j in range(min(6, len(core))):
            z, y, x = core[rng.randint(len(core))]
            vol[z - hz:z + hz + 1, y - 2:y + 3, x - 2:x + 3] = v
            h, w = rng.randint(1, 4), rng.randint(1, 4)
            y0, x0 = y - h // 2, x - w // 2
            vol[z, y0:y0 + h, x0:x0 + w] = OTHER_GREY if j % 3 == 1 else 0
            if j % 3 == 2:
                vol[z, y, x] = values[(k + 1) % len(values)]
    vol.setflags(write=False)
    return vol, tuple(values)


@functools.lru_cache(maxsize=None)
def _reference(name, mode):
    """(out, stats) of the yardstick, computed once per case and mode and never written to"""
    vol, values = _punched(name)
    out, stats = F.fill_holes(vol, values, mode)
    out.setflags(write=False)
    stats.setflags(write=False)
    return out, stats


@functools.lru_cache(maxsize=None)
def _past_cap():
    """the punched `k2` tiled over PAST_CAP, and one sealed cavity in the last slice but one, past the grid cap in linear index"""
    vol, values = _punched('k2')
    reps = [-(-n // m) for n, m in zip(PAST_CAP, vol.shape)]
    big = np.tile(vol, reps)[:PAST_CAP[0], :PAST_CAP[1], :PAST_CAP[2]].copy()
    z = PAST_CAP[0] - 2
    big[z - 1:z + 2, 199:206, 188:195] = values[0]
    big[z, 201:204, 190:193] = 0
    big[z, 202, 191] = OTHER_GREY
    big.setflags(write=False)
    refs = {mode: F.fill_holes(big, values, mode) for mode in F.MODES}
    return big, values, refs


def _run(volume, values, mode, dev):
    """(out, stats) as numpy through ops.fill_label_holes, run twice: the second run must be bitwise equal"""
    from multimodal_segmentation_amd import ops
    x, v = _up(volume, dev), _up(np.asarray(values), dev, np.int32)
    out, stats = ops.fill_label_holes(x, v, mode)
    out2, stats2 = ops.fill_label_holes(x, v, mode)
    assert out.dtype == torch.uint8 and tuple(out.shape) == volume.shape and torch.equal(out, out2)
    assert stats.dtype == torch.int32 and tuple(stats.shape) == (len(values), 3) and torch.equal(stats, stats2)
    assert torch.equal(x.cpu(), torch.from_numpy(np.array(volume)))          # the input is left alone
    return out.cpu().numpy(), stats.cpu().numpy()


def _check(volume, values, dev, modes=F.MODES):
    """both modes against the yardstick -> {mode: (out, stats)}"""
    got = {}
    for mode in modes:
        want, want_stats = F.fill_holes(volume, values, mode)
        out, stats = _run(volume, values, mode, dev)
        differ = int(np.count_nonzero(out != want))
        print('mode %s: %d differing voxels of %d; stats %s, yardstick %s' % (mode, differ, volume.size, stats.tolist(), want_stats.tolist()))
        assert differ == 0
        assert np.array_equal(stats, want_stats)
        got[mode] = (out, stats)
    return got


# ---- 1. the inputs and the yardstick alone (no GPU) --------------------------------------------------------------------------------------
def test_inputs_are_not_vacuous():
    assert set(DENSE) <= set(CASES) and 'one-slice' in CASES
    for name in sorted(CASES):
        vol, values = _punched(name)
        ref = {mode: _reference(name, mode) for mode in F.MODES}
        hole = {mode: [F.holes(vol, v, mode) for v in values] for mode in F.MODES}
        for mode in F.MODES:
            out, stats = ref[mode]
            print('%s %s: holes, before, added per organ %s' % (name, mode, stats.tolist()))
            assert np.array_equal(out[vol != 0], vol[vol != 0])                                                  # 6
            assert np.array_equal(out != vol, (vol == 0) & (out != 0)) and set(np.unique(out[out != vol]).tolist()) <= set(values)
        assert np.count_nonzero(ref['2d'][1][:, 0] > 0) >= 2 and ref['2d'][1][:, 2].sum() >= 1                    # 1
        if name in DENSE:
            for mode in F.MODES:
                assert (ref[mode][1][:, 0] >= 3).all() and (ref[mode][1][:, 2] >= 1).all(), (name, mode)          # 2
                inside = np.logical_or.reduce(hole[mode]) & (vol != 0)
                assert inside.any() and np.array_equal(ref[mode][0][inside], vol[inside])                         # 3
        if vol.shape[0] > 1:
            assert not np.array_equal(ref['2d'][0], ref['3d'][0])                                                 # 4
            for h2, h3 in zip(hole['2d'], hole['3d']):
                assert not (h3 & ~h2).any()
        else:
            assert np.array_equal(ref['3d'][0], vol) and not ref['3d'][1][:, [0, 2]].any()                        # 5
            assert not np.array_equal(ref['2d'][0], vol)
    big, values, refs = _past_cap()
    assert big.size > GRID_CAP and all(n % t for n, t in zip(big.shape, (4, 8, 32)))
    for mode in F.MODES:
        changed = np.flatnonzero(refs[mode][0] != big)
        print('past the cap, %s: %d voxels filled, %d of them past index %d; stats %s'
              % (mode, changed.size, np.count_nonzero(changed >= GRID_CAP), GRID_CAP, refs[mode][1].tolist()))
        assert (changed >= GRID_CAP).any() and (changed < GRID_CAP).any()


# ---- 2. all eight punched cases, both modes ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize('mode', F.MODES)
@pytest.mark.parametrize('name', sorted(CASES))
def test_filled_volume_equals_yardstick(name, mode, dev, monkeypatch):
    from multimodal_segmentation_amd import _native, ops
    vol, values = _punched(name)
    want, want_stats = _reference(name, mode)
    new = ops._new

    def prefilled(*args, **kwargs):          # what ops allocates for the result holds PREFILL before the call
        t = new(*args, **kwargs)
        return t.fill_(PREFILL) if t.dtype == torch.uint8 else t
    monkeypatch.setattr(ops, '_new', prefilled)
    out, stats = _run(vol, values, mode, dev)
    differ = int(np.count_nonzero(out != want))
    print('%s %s: %d differing voxels of %d; stats\n%s\nyardstick\n%s' % (name, mode, differ, vol.size, stats, want_stats))
    assert differ == 0
    assert np.array_equal(stats, want_stats)
    # the raw entry point: every byte of out and stats is written
    S, H, W = vol.shape
    x, v = _up(vol, dev), _up(np.asarray(values), dev, np.int32)
    raw = torch.full((S, H, W), PREFILL, dtype=torch.uint8, device=dev)
    raw_stats = torch.full((len(values), 3), -1, dtype=torch.int32, device=dev)
    ws = torch.empty((_native.call('mmseg_fill_label_holes_workspace_bytes', S, H, W, len(values)) + 3) // 4, device=dev)
    assert _native.call('mmseg_fill_label_holes', x, v, raw, raw_stats, ws, S, H, W, len(values), int(mode == '2d')) == 0
    assert np.array_equal(raw.cpu().numpy(), want) and np.array_equal(raw_stats.cpu().numpy(), want_stats)


# ---- 3. known answers -----------------------------------------------------------------------------------------------------------------------
def _box(shape, v, wall=1):
    """a box three slices thick (one slice of interior) in the middle of the volume -> (solid box, its interior as a mask)"""
    S, H, W = shape
    z = S // 2 - 1
    vol, inner = np.zeros(shape, np.uint8), np.zeros(shape, bool)
    vol[z:z + 3, 5:30, 4:36] = v
    inner[z + 1, 5 + wall:30 - wall, 4 + wall:36 - wall] = True
    return vol, inner, z


@pytest.mark.parametrize('shape', KNOWN_SHAPES)
def test_hollow_box_cup_and_tube(shape, dev):
    v = VALUES[1]
    solid, inner, z = _box(shape, v)
    before, interior = int(solid.sum() // v - inner.sum()), int(inner.sum())
    hollow = np.where(inner, 0, solid).astype(np.uint8)
    for mode, (out, stats) in _check(hollow, VALUES, dev).items():
        assert np.array_equal(out, solid)
        assert np.array_equal(stats, np.asarray([[0, 0, 0], [1, before, interior], [0, 0, 0], [0, 0, 0]], np.int32))
    cup = hollow.copy()
    cup[z, 17, 20] = 0          # one voxel of the top face
    got = _check(cup, VALUES, dev)
    assert np.array_equal(got['3d'][0], cup) and not got['3d'][1][:, [0, 2]].any() and got['3d'][1][1, 1] == before - 1
    assert np.array_equal(got['2d'][0], solid)          # the ring slice, and the missing voxel: in its slice the wall encloses it
    assert np.array_equal(got['2d'][1][1], (2, before - 1, interior + 1))
    tube = np.zeros(shape, np.uint8)
    tube[:, 5:30, 4:36] = v
    tube[:, 6:29, 5:35] = 0          # open at both ends along the slice axis
    got = _check(tube, VALUES, dev)
    assert np.array_equal(got['3d'][0], tube) and not got['3d'][1][:, [0, 2]].any()
    assert (got['2d'][0][:, 5:30, 4:36] == v).all() and np.array_equal(got['2d'][1][1], (shape[0], shape[0] * (25 * 32 - 23 * 30), shape[0] * 23 * 30))


@pytest.mark.parametrize('shape', KNOWN_SHAPES)
def test_a_cavity_joined_to_the_outside_across_an_edge_is_enclosed(shape, dev):
    """walls two voxels thick in the plane; two removed wall voxels on the diagonal of a corner: the inner one shares only an edge with
    the cavity and with the outer one, which faces the outside.  With faces only the cavity stays closed and the inner voxel is a hole
    of its own; a background joined through edges or corners would open both."""
    v = VALUES[0]
    solid, inner, z = _box(shape, v, wall=2)
    vol = np.where(inner, 0, solid).astype(np.uint8)
    assert inner[z + 1, 7, 6] and not inner[z + 1, 6, 5]
    vol[z + 1, 6, 5] = 0
    vol[z + 1, 5, 4] = 0          # the corner of the box: its row and column neighbours lie outside
    want = solid.copy()
    want[z + 1, 5, 4] = 0
    assert ndi.label(vol == 0, np.ones((3, 3, 3)))[1] == 1 and ndi.label(vol == 0, F.FACES)[1] == 3
    for mode, (out, stats) in _check(vol, VALUES, dev).items():
        assert np.array_equal(out, want)
        assert np.array_equal(stats[0], (2, solid.sum() // v - inner.sum() - 2, inner.sum() + 1)) and not stats[1:].any()


@pytest.mark.parametrize('shape', KNOWN_SHAPES)
def test_serpentine_cavity_open_at_its_far_end(shape, dev):
    """a cavity one voxel wide through every tile of a solid block: open to the border through one voxel next to its last voxel, the
    far end seen from the root of its set; sealed, it is one hole"""
    v = VALUES[2]
    S, H, W = shape
    cavity = np.zeros(shape, bool)
    cavity[1:-1, 1:-1, 1:-1] = _serpentine((S - 2, H - 2, W - 2), 1) != 0
    assert ndi.label(cavity, F.FACES)[1] == 1 and cavity[-2, -2, -2] and np.flatnonzero(cavity)[-1] == np.ravel_multi_index((S - 2, H - 2, W - 2), shape)
    tiles = {(z // 4, y // 8, x // 32) for z, y, x in np.argwhere(cavity)}
    assert len(tiles) == -(-S // 4) * -(-H // 8) * -(-W // 32)          # it passes through every tile
    sealed = np.where(cavity, 0, v).astype(np.uint8)
    n = int(cavity.sum())
    got = _check(sealed, VALUES, dev)
    assert (got['3d'][0] == v).all() and np.array_equal(got['3d'][1][2], (1, sealed.size - n, n)) and not got['3d'][1][[0, 1, 3]].any()
    opened = sealed.copy()
    opened[S - 2, H - 2, W - 1] = 0
    got = _check(opened, VALUES, dev)
    assert np.array_equal(got['3d'][0], opened) and np.array_equal(got['3d'][1][2], (0, sealed.size - n - 1, 0))


def _nested(shape, outer, inner):
    """a shell of `outer` around a zero gap around a shell of `inner` around a zero core; nested along the slice axis too where the
    volume has the slices for it -> (volume, gap, core, closed in 3-D)"""
    S = shape[0]
    deep = S >= 11
    vol = np.zeros(shape, np.uint8)
    boxes = []
    for i in range(4):
        zs = slice(1 + i, 10 - i) if deep else slice(0, S)
        boxes.append((zs, slice(3 + 2 * i, 33 - 2 * i), slice(4 + 2 * i, 40 - 2 * i)))
    vol[boxes[0]] = outer
    vol[boxes[1]] = 0
    vol[boxes[2]] = inner
    vol[boxes[3]] = 0
    gap, core = np.zeros(shape, bool), np.zeros(shape, bool)
    gap[boxes[1]] = True
    gap[boxes[2]] = False
    core[boxes[3]] = True
    return vol, gap, core, deep


@pytest.mark.parametrize('shape', KNOWN_SHAPES)
def test_shell_inside_a_shell_the_lowest_k_wins(shape, dev):
    a, b = VALUES[0], VALUES[1]
    vol, gap, core, deep = _nested(shape, a, b)
    both = _check(vol, [a, b], dev)
    swapped = _check(vol, [b, a], dev)
    for mode in F.MODES if deep else ('2d',):
        out, stats = both[mode]
        assert (out[gap] == a).all() and (out[core] == a).all() and np.array_equal(out[vol != 0], vol[vol != 0])
        assert stats[0, 2] == gap.sum() + core.sum() and stats[1, 0] >= 1 and stats[1, 2] == 0          # organ 1: a hole, nothing added
        out, stats = swapped[mode]
        assert (out[gap] == a).all() and (out[core] == b).all() and np.array_equal(out[vol != 0], vol[vol != 0])
        assert stats[0, 2] == core.sum() and stats[1, 2] == gap.sum()
    if not deep:
        assert np.array_equal(both['3d'][0], vol) and not both['3d'][1][:, [0, 2]].any()


@pytest.mark.parametrize('shape', KNOWN_SHAPES)
def test_other_grey_values_in_a_hole_and_organs_face_to_face(shape, dev):
    a, b = VALUES[0], VALUES[3]
    solid, inner, z = _box(shape, a)
    vol = np.where(inner, 0, solid).astype(np.uint8)
    vol[z + 1, 10, 10:13] = OTHER_GREY
    vol[z + 1, 15:17, 20] = b
    want = np.where((vol == 0) & inner, a, vol)
    for mode, (out, stats) in _check(vol, VALUES, dev).items():
        assert np.array_equal(out, want) and (out == OTHER_GREY).sum() == 3 and (out == b).sum() == 2
        assert np.array_equal(stats[0], (1, (vol == a).sum(), inner.sum() - 5))
        assert np.array_equal(stats[3], (0, 2, 0)) and not stats[1:3].any()
    # organ a closes one half of the cavity and organ b the other half: a hole of neither
    halves = np.where(inner, 0, solid).astype(np.uint8)
    halves[:, :, 20:][halves[:, :, 20:] == a] = b
    assert (halves == a).any() and (halves == b).any() and (halves[inner] == 0).all()
    for mode, (out, stats) in _check(halves, VALUES, dev).items():
        assert np.array_equal(out, halves) and not stats[:, [0, 2]].any()


def test_no_organ_voxel_and_no_slice(dev):
    from multimodal_segmentation_amd import ops
    for shape in KNOWN_SHAPES:
        vol = np.zeros(shape, np.uint8)
        vol[:, 3:9, 4:11] = OTHER_GREY
        vol[:, 5, 6] = 0
        for mode, (out, stats) in _check(vol, VALUES, dev).items():
            assert np.array_equal(out, vol) and not stats.any()
    v = _up(np.asarray(VALUES), dev, np.int32)
    none = torch.zeros((0, 8, 9), dtype=torch.uint8, device=dev)
    for mode in F.MODES:
        out, stats = ops.fill_label_holes(none, v, mode)
        assert tuple(out.shape) == (0, 8, 9) and out.dtype == torch.uint8
        assert tuple(stats.shape) == (4, 3) and stats.dtype == torch.int32 and not stats.any()


@pytest.mark.parametrize('axis', (0, 1, 2))
def test_nothing_depends_on_the_scan_direction(axis, dev):
    vol, values = _punched('12x53x47')
    flipped = np.ascontiguousarray(np.flip(vol, axis))
    for mode in F.MODES:
        want, want_stats = _reference('12x53x47', mode)
        out, stats = _run(flipped, values, mode, dev)
        assert np.array_equal(out, np.flip(want, axis)) and np.array_equal(stats, want_stats)


# ---- 4. one case past the grid cap -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('mode', F.MODES)
def test_a_volume_past_the_grid_cap(mode, dev):
    big, values, refs = _past_cap()
    out, stats = _run(big, values, mode, dev)
    differ = int(np.count_nonzero(out != refs[mode][0]))
    print('%s: %d differing voxels of %d (cap %d); stats %s, yardstick %s' % (mode, differ, big.size, GRID_CAP, stats.tolist(), refs[mode][1].tolist()))
    assert differ == 0
    assert np.array_equal(stats, refs[mode][1])


# ---- 5. the chain: on the file grid ----------------------------------------------------------------------------------------------------
def test_holes_are_those_of_the_file_grid(dev):
    from multimodal_segmentation_amd.volume_predictor import fill_holes
    v = VALUES[1]
    H, W = 37, 41
    packed = np.zeros((4, H, W), np.uint8)
    packed[0:3, 5:20, 6:25] = v
    packed[1, 8:12, 9:15] = 0          # the cavity; its lids are the packed slices 0 and 2
    packed[3, 20:30, 20:30] = v
    packed[3, 22, 23:26] = 0           # closed in its slice only
    slices = [0, 1, 3, 4]              # the file holds a slice between the cavity and its lower lid
    geometry = dict(raw_shape=(5, H, W), slices=slices)
    on_grid = np.zeros((5, H, W), np.uint8)
    on_grid[slices] = packed
    values = _up(np.asarray(VALUES), dev, np.int32)
    for mode in F.MODES:
        got, stats = fill_holes(_up(packed, dev), values, geometry, mode)
        got, stats = got.cpu().numpy(), stats.cpu().numpy()
        want, want_stats = F.fill_holes(on_grid, VALUES, mode)
        assert np.array_equal(got, want[slices]) and np.array_equal(stats, want_stats)
        closed, _ = F.fill_holes(packed, VALUES, mode)
        if mode == '3d':
            assert np.array_equal(got, packed) and not np.array_equal(closed, packed)          # open in the file, closed when packed
        else:
            assert np.array_equal(got, closed) and np.array_equal(stats[1], (2, (packed == v).sum(), 24 + 3))


# ---- 6. end to end -------------------------------------------------------------------------------------------------------------------------
@pytest.fixture
def solid_folder(folder):
    """the folder of test_volume_components (every organ of the truth one body), with the holes that the truth's own organs have in a
    slice filled by the yardstick: a filling that closes a true hole is scored worse for it, which is not what this test is about"""
    manifest = json.load(open(os.path.join(folder, 'dataset.json')))
    for entry in manifest['volumes'].values():
        for e in entry.values():
            with np.load(os.path.join(folder, e['file'])) as z:
                arrays = {k: z[k] for k in z.files}
            arrays['label'] = F.fill_holes(arrays['label'], VALUES, '2d')[0]
            np.savez_compressed(os.path.join(folder, e['file']), **arrays)
    return folder


def _with_cavities(stub, K):
    """the stub's probabilities with two cavities punched into every organ of every slice (background there), and one far-away blob
    per organ"""
    class Cavities(object):
        modalities = stub.modalities

        def predict_mask(self, modality_index, mode, image_list):
            t = stub.predict_mask(modality_index, mode, image_list)
            p = t.cpu().numpy().copy()
            for s in range(p.shape[0]):
                for k in range(K):
                    organ = p[s, :, :, k] > 0.5
                    core, n = np.argwhere(ndi.binary_erosion(organ, np.ones((5, 5), bool))), 2
                    if not len(core):          # a small organ: one pixel inside a 3 x 3 neighbourhood
                        core, n = np.argwhere(ndi.binary_erosion(organ, np.ones((3, 3), bool))), 1
                    for y, x in (core[0], core[-1]) if len(core) else ():
                        p[s, y + 1 - n:y + 1, x + 1 - n:x + 1, :] = 0.0
                        p[s, y + 1 - n:y + 1, x + 1 - n:x + 1, K] = 1.0
                    p[s, 3:5, 3 + 12 * k:5 + 12 * k, :] = 0.0
                    p[s, 3:5, 3 + 12 * k:5 + 12 * k, k] = 1.0
            return torch.from_numpy(p).to(t.device)
    return Cavities()


def _experiment(monkeypatch, model, run_folder):
    """Experiment whose configuration, training and model are the stub's: what is left is the command line and run_prediction"""
    from multimodal_segmentation_amd import experiment, volume_predictor
    from tests.test_volume_predict import _stub_conf
    conf = _stub_conf(3)
    conf.folder, conf.model = run_folder, 'stub.Stub'

    class Built(object):
        def __new__(cls, conf):
            return model
    model.build = lambda: None

    def init_logging(self, conf):
        self.log = logging.getLogger()
    monkeypatch.setattr(experiment.Experiment, 'get_config', lambda self, split, args: conf)
    monkeypatch.setattr(experiment.Experiment, 'init_logging', init_logging)
    monkeypatch.setattr(experiment.Experiment, 'run_experiment', lambda self, conf, test: None)
    monkeypatch.setattr(experiment, 'resolve', lambda subpackage, dotted: Built)
    monkeypatch.setattr(volume_predictor, 'checkpoint_of', lambda folder: folder)
    return experiment.Experiment()


def test_experiment_fills_holes_after_the_component_filter(solid_folder, tmp_path, dev, monkeypatch):
    folder = solid_folder
    from multimodal_segmentation_amd.loaders.volume_folder import VolumeFolderLoader
    from tests.test_volume_predict import StubModel
    K = len(VALUES)
    loader = VolumeFolderLoader(folder)
    manifest = loader.manifest
    assert any('slices' in e[mod] for e in manifest['volumes'].values() for mod in ('t1', 't2'))          # unselected slices occur
    model = _with_cavities(StubModel(loader, dev, [1, 2, 3, 4]), K)
    exp = _experiment(monkeypatch, model, str(tmp_path / 'run'))
    plain, kept, filled = str(tmp_path / 'plain'), str(tmp_path / 'kept'), str(tmp_path / 'filled')
    base = ['--config', 'dafnet_config_chaos', '--split', '0', '--predict_folder', folder]
    exp.run(base + ['--predict_out', plain])
    exp.run(base + ['--predict_out', kept, '--predict_components', 'largest'])
    exp.run(base + ['--predict_out', filled, '--predict_components', 'largest', '--predict_fill_holes', '2d'])
    # without the option: no new file, no new key
    files = [e[mod]['file'] for e in manifest['volumes'].values() for mod in ('t1', 't2')]
    scores = ['results_%s_%s.csv' % (a, b) for a in ('native', 'surface') for b in ('t1', 't2')]
    comps = ['results_components_t1.csv', 'results_components_t2.csv']
    assert sorted(os.listdir(plain)) == sorted(['predictions.json'] + scores + files)
    assert sorted(os.listdir(kept)) == sorted(['predictions.json'] + scores + comps + files)
    assert sorted(os.listdir(filled)) == sorted(['predictions.json'] + scores + comps + files + ['results_holes_t1.csv', 'results_holes_t2.csv'])
    settings = [json.load(open(os.path.join(d, 'predictions.json'))) for d in (plain, kept, filled)]
    assert 'fill_holes' not in settings[0] and 'fill_holes' not in settings[1]
    assert sorted(settings[2]) == sorted(list(settings[1]) + ['fill_holes']) and settings[2]['fill_holes'] == '2d'
    header = 'Vol, ' + ', '.join('%s%d' % (n, k) for k in range(K) for n in ('N', 'Before', 'Added'))
    for mod in ('t1', 't2'):
        head, holes = _csv_rows(os.path.join(filled, 'results_holes_%s.csv' % mod))
        _, comp_rows = _csv_rows(os.path.join(filled, 'results_components_%s.csv' % mod))
        _, surface = _csv_rows(os.path.join(filled, 'results_surface_%s.csv' % mod))
        _, surface_kept = _csv_rows(os.path.join(kept, 'results_surface_%s.csv' % mod))
        lines = open(os.path.join(filled, 'results_native_%s.csv' % mod)).read().strip().split('\n')
        native = {l.split(',')[0]: [float(x) for x in l.split(',')[1:]] for l in lines[1:]}
        assert head == header and list(holes) == list(surface) == list(native) == ['1', '2', '3', '4']
        for v in ('1', '2', '3', '4'):
            entry = manifest['volumes'][v][mod]
            with np.load(os.path.join(folder, entry['file'])) as z:
                truth, res, dz = z['label'].copy(), z['resolution'], float(z['slice_spacing'])
            with np.load(os.path.join(plain, entry['file'])) as z:
                before = z['label']
            with np.load(os.path.join(filled, entry['file'])) as z:
                assert sorted(z.files) == ['label', 'resolution', 'slice_spacing']
                after = z['label']
            # the yardstick chain on the unprocessed prediction: filter, then fill, then scores
            largest, comp_stats = C.keep_largest(before, VALUES, 6)
            want, stats = F.fill_holes(largest, VALUES, '2d')
            assert after.dtype == np.uint8 and np.array_equal(after, want)
            # the blobs are there, and cavities in every organ with room for one (the folder's smallest organ is often absent)
            assert (comp_stats[:, 0] >= 2).all() and (stats[:, 0] >= 2).sum() >= 2 and (stats[:, 2] >= 2).sum() >= 2
            assert comp_rows[v] == ['%d' % x for x in comp_stats.reshape(-1)]
            assert holes[v] == ['%d' % x for x in stats.reshape(-1)]
            a, b = entry.get('slices', [[0, truth.shape[0]]])[0]
            truth[:a], truth[b:] = 0, 0
            in_mm = M.chaos_metrics(want, truth, VALUES, (dz, res[0], res[1]))
            in_mm = np.concatenate([in_mm[-1:], in_mm[:-1]], axis=0).reshape(-1)          # the union first
            assert surface[v] == ['%.3f' % x for x in in_mm]
            sel = np.arange(a, b)
            joint, per_organ = P.dice(truth[sel], want[sel], VALUES)
            for got, ref in zip(native[v], [joint] + per_organ):          # as printed; the two sums round the same quotient
                assert abs(got - float('%.3f' % ref)) <= 0.001 + 1e-9
            print('volume %s %s: holes %s | ASSD %s mm, without the filling %s mm' % (v, mod, holes[v], surface[v][1], surface_kept[v][1]))
            assert float(surface[v][1]) < float(surface_kept[v][1])
    # the tool filters and fills the volumes written without either and scores them: the same score files, byte for byte
    again = str(tmp_path / 'again')
    _score_tool().main([plain, folder, '--out', again, '--components', 'largest', '--fill_holes', '2d'])
    assert sorted(os.listdir(again)) == sorted(scores)
    for name in scores:
        assert open(os.path.join(again, name), 'rb').read() == open(os.path.join(filled, name), 'rb').read(), name
    # and the files of the run with the filter alone are those of a run that never heard of the option
    from multimodal_segmentation_amd.volume_predictor import VolumePredictor
    from tests.test_volume_predict import _stub_conf
    direct = str(tmp_path / 'direct')
    VolumePredictor(model, _stub_conf(3)).run(folder, direct, components='largest')
    for name in scores + comps + files:
        assert _file_contents(os.path.join(direct, name)) == _file_contents(os.path.join(kept, name)), name
    with pytest.raises(ValueError, match='fill_holes'):
        VolumePredictor(model, _stub_conf(3)).run(folder, str(tmp_path / 'no'), fill_holes='4d')
    assert not os.path.exists(str(tmp_path / 'no'))


# ---- 7. ABI and arguments -----------------------------------------------------------------------------------------------------------------
def test_cli_options(monkeypatch, capsys):
    from multimodal_segmentation_amd import experiment
    base = ['--config', 'dafnet_config_chaos', '--split', '0']
    assert experiment.parse_arguments(base).predict_fill_holes == 'none'
    for mode in F.MODES:
        assert experiment.parse_arguments(base + ['--predict_fill_holes', mode]).predict_fill_holes == mode

    def no_model(*args, **kwargs):
        raise AssertionError('the run went on past the options')
    monkeypatch.setattr(experiment.Experiment, 'get_config', no_model)
    monkeypatch.setattr(experiment.Experiment, 'get_executor', no_model)
    capsys.readouterr()
    with pytest.raises(SystemExit):
        experiment.Experiment().run(base + ['--predict_fill_holes', '4d'])
    assert '--predict_fill_holes' in capsys.readouterr().err
    tool = _score_tool()
    for bad in ('4d', 'none'):
        with pytest.raises(SystemExit):
            tool.main(['a', 'b', '--fill_holes', bad])
        assert '--fill_holes' in capsys.readouterr().err


def test_entry_points_declared_and_bad_arguments_refused():
    from multimodal_segmentation_amd import _native, ops, volume_predictor
    protos = _native.parse_header()
    for name in F.STANDINS:
        assert name in protos, name
        assert name.endswith('workspace_bytes') or protos[name][1][-1] == 'void*', name
    assert callable(ops.fill_label_holes) and callable(volume_predictor.fill_holes) and callable(volume_predictor.check_fill_holes)
    _native.build()
    lib = _native.load()
    for name in F.STANDINS:
        assert hasattr(lib, name)
    ptrs, bad = [8, 16, 24, 32, 40], 1          # non-null pointers (a refused call launches nothing and touches no memory); hipErrorInvalidValue
    fill, query = lib.mmseg_fill_label_holes, lib.mmseg_fill_label_holes_workspace_bytes
    for S, H, W, K, per_slice in ((2, 8, 8, 17, 0), (2, 8, 8, 0, 1), (2, 0, 8, 4, 0), (2, 8, 0, 4, 1), (2048, 1024, 1024, 4, 0),
                                  (1, 2 ** 31 - 1, 1, 4, 1), (2, 8, 8, 4, 2), (2, 8, 8, 4, -1)):
        assert fill(*(ptrs + [S, H, W, K, per_slice, None])) == bad, (S, H, W, K, per_slice)
    for i in range(5):
        p = list(ptrs)
        p[i] = None
        assert fill(*(p + [2, 8, 8, 4, 0, None])) == bad
    assert fill(8, 16, 8, 32, 40, 2, 8, 8, 4, 0, None) == bad          # out is label
    for per_slice in (0, 1):
        assert fill(*(ptrs + [0, 8, 8, 4, per_slice, None])) == 0          # S = 0: nothing to do
    n = 36 * 320 * 320
    assert query(36, 320, 320, 4) >= 4 * n
    assert query(36, 320, 320, 17) == 0 and query(2048, 1024, 1024, 4) == 0 and query(2, 0, 8, 4) == 0
    u8, i32 = torch.zeros(2, 8, 8, dtype=torch.uint8), torch.zeros(4, dtype=torch.int32)
    name = 'fill_label_holes'
    for mode in ('4d', None, 2, '2D'):
        with pytest.raises(ValueError, match=name):
            ops.fill_label_holes(u8, i32, mode)
    with pytest.raises(ValueError, match=name):
        ops.fill_label_holes(torch.zeros(2, 8, 8), i32)
    with pytest.raises(ValueError, match=name):
        ops.fill_label_holes(torch.zeros(8, 8, dtype=torch.uint8), i32, '2d')
    with pytest.raises(ValueError, match=name):
        ops.fill_label_holes(u8, i32.float())
    with pytest.raises(ValueError, match=name):
        ops.fill_label_holes(u8, torch.zeros(17, dtype=torch.int32))
    for bad_mode in ('4d', 3, True):
        with pytest.raises(ValueError, match='fill_holes'):
            volume_predictor.check_fill_holes(bad_mode)


def test_holes_bench_tool_is_importable():
    """tools/volume_holes_bench.py refuses to time anything without a GPU, and says so"""
    spec = importlib.util.spec_from_file_location('volume_holes_bench', os.path.join(R.ROOT, 'tools', 'volume_holes_bench.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    assert callable(mod.main) and mod.SHAPES
    if not torch.cuda.is_available():
        with pytest.raises(SystemExit, match='GPU'):
            mod.main([])
