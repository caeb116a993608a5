"""Ensemble prediction with voxel-wise uncertainty and calibration scores: csrc/postprocess.hip (mmseg_members_accumulate,
mmseg_members_finish, mmseg_restore_map, mmseg_calibration_table, mmseg_uncertainty_by_error), their ops wrappers, `members=` /
`uncertainty=` / `calibration_bins=` of volume_predictor.VolumePredictor and `--predict_ensemble`, `--predict_uncertainty`,
`--predict_calibration_bins`, against the fp64 restatement of tests/volume_uncertainty_ref.py.

Comparison rules (set by the feature's issue).
  mean     one model: accumulate(first) + finish is ops.merge_views's map bit for bit, on every case and channel pair.
  stream   R = 3 models accumulated in three calls equal the restatement (T.MAP_BAR for the mean, PLANE_BAR for the planes) and, bit for
           bit, one call on the 3 V maps with the table of views repeated (3 V <= 16).
  planes   H and I differ from fp64 by at most PLANE_BAR (derived at test_planes_match_fp64).
  zeros    one member: I == 0 bit for bit; a model and its copy: the single model's mean bit for bit, I == 0; no view: (0, 0, 0).
  levels   restore_map equals the fp64 restatement on every decidable pixel and differs by at most 1 elsewhere; undecidable: 255 v within
           U.LEVEL_BAND of k + 0.5, at most U.LEVEL_CAP of a case's pixels; order 0 exact; cropped-away pixels 0.
  table    bins equal the fp32 numpy rule exactly; sums within 1e-9 relative (sum of p, Brier) and 1e-5 (NLL: logf is
           implementation-defined); every organ's bins add up to the window's pixels; p == y gives ECE = Brier = 0.
  by error exact integers."""
import functools
import json
import os

import numpy as np
import pytest
import torch

from multimodal_segmentation_amd import nn
from tests import volume_crf_ref as Q
from tests import volume_holes_ref as F
from tests import volume_loader_ref as R
from tests import volume_predict_ref as P
from tests import volume_tiles_ref as T
from tests import volume_tta_ref as A
from tests import volume_uncertainty_ref as U
from tests.test_augment_full import _standin_augment_gather
from tests.test_volume_loader import VALUES
from tests.test_volume_tiles import CENTRES, Pointwise, _conf, _whole_frames, wide_folder  # noqa: F401
from tests.test_volume_tta import CASES, CHANNELS, PAST_CAP, S, _case
from tests.volume_fixtures import _clean_registry, _dev, _up, device  # noqa: F401

PLANE_BAR = 2e-4          # see test_planes_match_fp64
RESTORE_CAP = 256 * 256          # PO_MAXBLK * PO_BLOCK: where the loops of mmseg_restore_map wrap (per slice; / 4 on the packed path)
TABLE_CAP = 1024 * 256           # CT_MAXBLK * PO_BLOCK: where the tile loop of mmseg_calibration_table wraps
# name -> (raw (H, W), resampled (RH, RW), rows, cols) for containers of 45 x 37
GEOMETRIES = {
    'whole-53x41': ((53, 41), (45, 37), (0, 45, 0), (0, 37, 0)),          # odd, W % 4 != 0: a byte per lane
    'crop-64x52': ((64, 52), (50, 44), (3, 45, 0), (4, 37, 0)),           # W % 4 == 0: packed dwords; a frame cropped on both axes
    'pad-47x36': ((47, 36), (40, 30), (0, 40, 2), (0, 30, 5)),            # a frame smaller than the container
    'cap-260x253': ((260, 253), (45, 37), (0, 45, 0), (0, 37, 0)),        # H W = 65780 > RESTORE_CAP on the byte path
    'cap-516x512': ((516, 512), (50, 44), (3, 45, 0), (4, 37, 0)),        # H W / 4 = 66048 > RESTORE_CAP packed; 3 H W > TABLE_CAP
}


@pytest.fixture
def dev(device, monkeypatch):
    """the shared `device` fixture with the stand-ins of the five new entry points, of the merge, the blend, the CRF, the views in and
    the hole filling on top of its table"""
    if device == 'cpu':
        from tests import cpu_backend as cb
        for table in (U.STANDINS, A.STANDINS, T.STANDINS, F.STANDINS, Q.STANDINS):
            for name, fn in table.items():
                monkeypatch.setitem(cb._TABLE, name, fn)
        monkeypatch.setitem(cb._TABLE, 'mmseg_augment_gather', _standin_augment_gather)
        monkeypatch.setitem(cb._TABLE, 'mmseg_augment_workspace_floats', lambda B, H, W, C: 2 * B)
    return _dev(device)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _members(probs, backs, N, K, dev):
    """every (prob, back) accumulated in turn, then finished -> (mean, planes) as numpy; the accumulation is run twice and must be
    bitwise equal, and `prob` is left alone"""
    from multimodal_segmentation_amd import ops
    outs = []
    for _ in range(2):
        state = None
        for prob, back in zip(probs, backs):
            p = nn.host_to_device(np.array(prob), dev, np.float32)
            state = ops.members_accumulate(p, np.array(back), N, K, state)
            assert np.array_equal(p.cpu().numpy(), prob)
        mean, planes = ops.members_finish(state)
        assert mean is state[0] and planes is state[1] and mean.dtype == planes.dtype == torch.float32
        outs.append((mean.cpu().numpy(), planes.cpu().numpy()))
    assert np.array_equal(_bits(outs[0][0]), _bits(outs[1][0])) and np.array_equal(_bits(outs[0][1]), _bits(outs[1][1]))
    assert np.isfinite(outs[0][0]).all() and np.isfinite(outs[0][1]).all()
    return outs[0]


@functools.lru_cache(maxsize=None)
def _three(name, C, K):
    """R = 3 models on case `name`: the case's maps and two variants of them (a soft-max sharpened and flattened, so that the models
    disagree) -> (probs, backs, the restatement's (mean, H, I, cnt))"""
    shape, text, _ = CASES[name]
    prob, back = _case(shape, text, C, K)[:2]
    probs = [prob]
    for power in (2.0, 0.5):
        p = prob.astype(np.float64) ** power
        probs.append((p / p.sum(-1, keepdims=True)).astype(np.float32))
    want = U.members(probs, [back] * 3, S, K)
    for a in probs + list(want):
        a.setflags(write=False)
    return probs, [back] * 3, want


# ---- 1. the mean is the merge ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('C,K', CHANNELS)
@pytest.mark.parametrize('name', sorted(CASES))
def test_one_model_mean_equals_merge_views(name, C, K, dev):
    from multimodal_segmentation_amd import ops
    shape, text, _ = CASES[name]
    prob, back, _, count = _case(shape, text, C, K)
    merged = ops.merge_views(_up(prob, dev, np.float32), np.array(back), S, K).cpu().numpy()
    mean, planes = _members([prob], [back], S, K, dev)
    assert np.array_equal(_bits(mean), _bits(merged))
    assert planes.min() >= 0 and planes.max() <= 1          # the views of one model are members like any other: I > 0 where they differ
    if name == '32x32':
        assert (count == 1).any()


def test_pixels_that_one_view_or_no_view_covers(dev):
    """a NaN matrix covers nothing: pixels with cnt 0, 1 and 2.  The mean is the merge bit for bit, (0, 0, 0) where nothing covers;
    the entry points themselves, on pre-filled accumulators that first != 0 must not read"""
    from multimodal_segmentation_amd import _native, ops
    OH, OW, C, K = 32, 32, 5, 4
    back = np.array(A.tables('id,rot20,rot45', OH, OW)[2])
    back[0] = np.nan
    rng = np.random.RandomState(5)
    prob = rng.uniform(0, 0.25, size=(3 * S, OH, OW, C)).astype(np.float32)
    count = A.merge(prob, back, S, K)[1]
    assert count.min() == 0 and count.max() == 2 and (count == 1).any()
    p, b = _up(prob, dev, np.float32), _up(back, dev, np.float64)
    merged = ops.merge_views(p, b, S, K).cpu().numpy()
    total, aux = torch.full((S, OH, OW, K), np.nan, device=dev), torch.full((S, OH, OW, 2), np.nan, device=dev)
    assert _native.call('mmseg_members_accumulate', p, b, total, aux, 1, 3, S, OH, OW, C, K) == 0
    assert np.array_equal(aux.cpu().numpy()[..., 1], np.broadcast_to(count[None].astype(np.float32), (S, OH, OW)))
    assert _native.call('mmseg_members_finish', total, aux, S, OH, OW, K) == 0
    mean, planes = total.cpu().numpy(), aux.cpu().numpy()
    assert np.array_equal(_bits(mean), _bits(merged))
    assert not mean[:, count == 0].any() and not planes[:, count == 0].any()
    want = U.members([prob], [back], S, K)
    assert np.abs(planes[..., 0] - want[1]).max() <= PLANE_BAR and np.abs(planes[..., 1] - want[2]).max() <= PLANE_BAR
    assert (planes[:, count == 1][..., 1] == 0).all()          # one covering view: nothing to disagree with


# ---- 2. streaming, and 3. the planes against fp64 ----------------------------------------------------------------------------------------------
def test_inputs_are_not_vacuous():
    """on case 45x37 with six members (the six views of one model) the restatement has I > 0.02 on at least 5 % and H > 0.5 on at least
    30 % of the pixels (11.6 % and 67.3 % when this was written); the numpy fp32 rule is within a quarter of PLANE_BAR of fp64 (5.2e-7
    when this was written: a few ulp of an entropy between 1 and 2 nats)"""
    shape, text, _ = CASES['45x37']
    prob, back = _case(shape, text, 5, 4)[:2]
    V = back.shape[0]
    probs = [prob[v * S:(v + 1) * S] for v in range(V)]
    backs = [back[v:v + 1] for v in range(V)]
    mean, H, I, cnt = U.members(probs, backs, S, 4)
    share_i, share_h = float(np.mean(I > 0.02)), float(np.mean(H > 0.5))
    print('45x37, six members: I > 0.02 on %.1f %%, H > 0.5 on %.1f %% of the pixels' % (100 * share_i, 100 * share_h))
    assert share_i >= 0.05 and share_h >= 0.30
    total, aux = torch.zeros((S,) + shape + (4,)), torch.zeros((S,) + shape + (2,))
    for i, (p, b) in enumerate(zip(probs, backs)):
        assert U.standin_members_accumulate(torch.from_numpy(np.array(p)), torch.from_numpy(np.array(b)), total, aux, int(i == 0), 1, S,
                                            shape[0], shape[1], 5, 4) == 0
    assert U.standin_members_finish(total, aux, S, shape[0], shape[1], 4) == 0
    worst = max(float(np.abs(aux.numpy()[..., 0] - H).max()), float(np.abs(aux.numpy()[..., 1] - I).max()))
    print('the numpy fp32 rule against fp64: largest difference of a plane %.3g' % worst)
    assert 4 * worst <= PLANE_BAR and np.abs(total.numpy() - mean).max() <= T.MAP_BAR


@pytest.mark.parametrize('C,K', CHANNELS)
@pytest.mark.parametrize('name', sorted(CASES))
def test_planes_match_fp64(name, C, K, dev):
    """Three models streamed through one pair of buffers against the fp64 restatement, and against one call on all their maps.

    PLANE_BAR.  A sample is bilinear: about 6 roundings of values in [0, 1], 6 * 2^-24 = 3.6e-7; a mean of at most 48 of them is good to
    T.MAP_BAR's count, (48 + 8) * 2^-24 = 3.3e-6 at the very worst and 1.4e-6 for 16.  t(x) = -x ln x turns an error d of x into at most
    d |ln d| + d (its slope is unbounded at 0, where t(d) = d |ln d|): 1.4e-6 -> 2.0e-5 per organ term, and the rest, which carries the K
    organs' errors (5.6e-6 for K = 4), 7.3e-5; logf's own ulp adds 1e-7.  K = 4: Hraw is good to 4 * 2.0e-5 + 7.3e-5 = 1.5e-4 nats, the
    mean E of the members' entropies (samples: d = 3.6e-7 -> 5.7e-6 per term, 2.3e-5 for the rest) to 4.6e-5 + 48 * 2^-24 * ln 5 = 5.1e-5.
    Over ln 5 = 1.61: H within 9.5e-5, I within 1.3e-4.  K = 2 (over ln 3): H within 7e-5, I within 1.1e-4.  Every term at its worst
    point at once cannot happen, so this is an upper bound: PLANE_BAR = 2e-4, below 1e-3, a quarter of one uint8 level (1 / 255).
    Largest difference measured over the fifteen cases: H 2.9e-6, I 2.8e-6, on the MI355X and with the numpy fp32 rule alike (the bar is
    69 times that)."""
    from multimodal_segmentation_amd import ops
    probs, backs, (w_mean, w_h, w_i, cnt) = _three(name, C, K)
    mean, planes = _members(probs, backs, S, K, dev)
    worst_m = float(np.abs(mean - w_mean).max())
    worst_h, worst_i = float(np.abs(planes[..., 0] - w_h).max()), float(np.abs(planes[..., 1] - w_i).max())
    print('%s C %d K %d, 3 models x %d views: largest difference from fp64: mean %.3g (bar %.0e), H %.3g, I %.3g (bar %.0e); I up to %.3f'
          % (name, C, K, backs[0].shape[0], worst_m, T.MAP_BAR, worst_h, worst_i, PLANE_BAR, w_i.max()))
    assert worst_m <= T.MAP_BAR and worst_h <= PLANE_BAR and worst_i <= PLANE_BAR
    assert planes.min() >= 0 and planes.max() <= 1 and 4 * max(worst_h, worst_i) <= PLANE_BAR < 1e-3
    assert w_i.max() > 0.01 or name == '1x1'
    V = backs[0].shape[0]
    if 3 * V <= A.MAX_VIEWS:          # one call on the 3 V maps, the table repeated: the same additions in the same order
        both = np.concatenate(probs, axis=0)
        state = ops.members_accumulate(_up(both, dev, np.float32), np.tile(backs[0], (3, 1)), S, K)
        once_mean, once_planes = (t.cpu().numpy() for t in ops.members_finish(state))
        assert np.array_equal(_bits(once_mean), _bits(mean)) and np.array_equal(_bits(once_planes), _bits(planes))


@pytest.mark.parametrize('C,K', CHANNELS[:2])
def test_a_volume_past_the_grid_cap(C, K, dev):
    """160 x 45 x 37 pixels: the grid-stride loops of both kernels wrap"""
    from multimodal_segmentation_amd import ops
    shape, text, slices = PAST_CAP
    prob, back, want, count = _case(shape, text, C, K, slices)
    assert slices * shape[0] * shape[1] > 1024 * 256
    mean, planes = _members([prob], [back], slices, K, dev)
    merged = ops.merge_views(_up(prob, dev, np.float32), np.array(back), slices, K).cpu().numpy()
    assert np.array_equal(_bits(mean), _bits(merged)) and np.abs(mean - want).max() <= T.MAP_BAR
    w = U.members([np.concatenate([prob[v * slices:v * slices + S] for v in range(4)], axis=0)], [back], S, K)
    reps = -(-slices // S)
    for u, plane in enumerate(w[1:3]):          # more slices than S repeat the S slices
        assert np.abs(planes[..., u] - np.tile(plane, (reps, 1, 1))[:slices]).max() <= PLANE_BAR


# ---- 4. exact zeros ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('C,K', CHANNELS)
def test_one_member_and_a_model_with_its_copy_disagree_about_nothing(C, K, dev):
    OH, OW = 45, 37
    prob = _case((OH, OW), 'flips', C, K)[0][:S]
    ident = A.tables('id', OH, OW)[2]
    mean, planes = _members([prob], [ident], S, K, dev)
    assert np.array_equal(_bits(mean), _bits(prob[..., :K])) and np.array_equal(_bits(planes[..., 1]), np.zeros((S, OH, OW), np.uint32))
    assert planes[..., 0].max() > 0.5
    twice, planes2 = _members([prob, prob], [ident, ident], S, K, dev)
    assert np.array_equal(_bits(twice), _bits(mean)) and np.array_equal(_bits(planes2), _bits(planes))


# ---- 5. the planes on a volume's own grid ---------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _planes45():
    """planes to bring back: (H, I) of the three models on 45x37 (U = 2) and their mean map (U = 4), fp32 as the rule's numpy form
    makes them"""
    probs, backs, _ = _three('45x37', 5, 4)
    total, aux = torch.zeros((S, 45, 37, 4)), torch.zeros((S, 45, 37, 2))
    for i, (p, b) in enumerate(zip(probs, backs)):
        assert U.standin_members_accumulate(torch.from_numpy(np.array(p)), torch.from_numpy(np.array(b)), total, aux, int(i == 0),
                                            b.shape[0], S, 45, 37, 5, 4) == 0
    assert U.standin_members_finish(total, aux, S, 45, 37, 4) == 0
    out = aux.numpy().copy(), total.numpy().copy()
    for a in out:
        a.setflags(write=False)
    return out


@pytest.mark.parametrize('name', sorted(GEOMETRIES))
def test_restore_map_matches_fp64(name, dev):
    from multimodal_segmentation_amd import ops
    raw_hw, resampled, rows, cols = GEOMETRIES[name]
    if name.startswith('cap'):
        assert raw_hw[0] * raw_hw[1] // (4 if raw_hw[1] % 4 == 0 else 1) > RESTORE_CAP
    inside = P.window_mask(raw_hw, resampled, rows, cols)
    assert inside.any() and inside.all() != name.startswith(('crop', 'cap-516'))          # only the cropped frames lose raw pixels
    for planes, us in zip(_planes45(), ((0, 1), (3,))):
        x = _up(planes, dev, np.float32)
        for u in us:
            for order in (0, 1):
                got = ops.restore_map(x, u, raw_hw, resampled, rows, cols, order)
                assert got.dtype == torch.uint8 and torch.equal(got, ops.restore_map(x, u, raw_hw, resampled, rows, cols, order))
                got = got.cpu().numpy()
                want, undecidable = U.levels(planes, u, raw_hw, resampled, rows, cols, order)
                off = np.abs(got.astype(np.int64) - want)
                share = np.count_nonzero(undecidable) / float(want.size)
                print('%s U %d u %d order %d: %d differing decidable pixels, %d undecidable (%.2f %%), levels up to %d'
                      % (name, planes.shape[-1], u, order, np.count_nonzero(off[~undecidable]), np.count_nonzero(undecidable),
                         100 * share, want.max()))
                assert not off[~undecidable].any() and off.max() <= 1 and share <= U.LEVEL_CAP
                assert not got[:, ~inside].any() and want.max() > 10
                if order == 0:
                    assert not undecidable.any()


def test_restore_map_rounds_and_limits(dev):
    """identity geometry, order 0: level = (unsigned char)(min(max(v, 0), 1) * 255 + 0.5f) value by value, NaN and the infinities
    included; every byte of a pre-filled output is written"""
    from multimodal_segmentation_amd import _native
    v = np.array([0.0, 1.0, 0.5, 0.25, 1 / 255.0, 0.5 / 255.0, np.nextafter(np.float32(0.5 / 255), np.float32(0)), 254.5 / 255, -0.3, 1.7,
                  np.inf, -np.inf, np.nan, 1e-30, 0.999, 0.0019], np.float32).reshape(1, 4, 4, 1)
    want = (np.minimum(np.maximum(np.nan_to_num(v, nan=0.0), np.float32(0)), np.float32(1)) * np.float32(255) + np.float32(0.5)).astype(np.uint8)
    out = torch.full((1, 4, 4), 77, dtype=torch.uint8, device=dev)
    assert _native.call('mmseg_restore_map', _up(v, dev, np.float32), out, 1, 4, 4, 4, 4, 4, 4, 0, 4, 0, 0, 4, 0, 1, 0, 0) == 0
    assert np.array_equal(out.cpu().numpy(), want[..., 0])
    assert want.reshape(-1)[:4].tolist() == [0, 255, 128, 64] and want.reshape(-1)[8:13].tolist() == [0, 255, 255, 0, 0]


# ---- 6. the calibration table -----------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _truth(name, K):
    """a label volume on the raw grid of geometry `name`: the labels of the case's first view, with a tenth of the pixels redrawn"""
    raw_hw, resampled, rows, cols = GEOMETRIES[name]
    prob = _case((45, 37), CASES['45x37'][1], 5, 4)[0][:S]
    label = P.restore(prob, VALUES[:K], raw_hw, resampled, rows, cols, 1)[0]
    rng = np.random.RandomState(77)
    noise = rng.choice(np.asarray([0] + list(VALUES[:K]), np.uint8), size=label.shape)
    label = np.where(rng.uniform(size=label.shape) < 0.1, noise, label).astype(np.uint8)
    label.setflags(write=False)
    return label


def _check_table(prob, truth, values, geometry, B, order, dev):
    from multimodal_segmentation_amd import ops
    raw_hw, resampled, rows, cols = geometry
    K = len(values)
    x, t, v = _up(prob, dev, np.float32), _up(truth, dev), _up(np.asarray(values), dev, np.int32)
    bins, sums = ops.calibration_table(x, t, v, resampled, rows, cols, B, order)
    again = ops.calibration_table(x, t, v, resampled, rows, cols, B, order)
    assert torch.equal(bins, again[0]) and np.array_equal(sums.cpu().numpy().view(np.uint64), again[1].cpu().numpy().view(np.uint64))
    assert bins.dtype == torch.int32 and tuple(bins.shape) == (K, B, 2) and sums.dtype == torch.float64 and tuple(sums.shape) == (K, B + 2)
    bins, sums = bins.cpu().numpy(), sums.cpu().numpy()
    w_bins, w_sums = U.table32(prob, truth, values, raw_hw, resampled, rows, cols, B, order)
    window = int(np.count_nonzero(P.window_mask(raw_hw, resampled, rows, cols))) * prob.shape[0]
    assert np.array_equal(bins, w_bins) and (bins[..., 0].sum(1) == window).all() and (bins[..., 1] <= bins[..., 0]).all()
    rel = np.abs(sums - w_sums) / np.maximum(np.abs(w_sums), 1e-300)
    rel[w_sums == 0] = np.abs(sums)[w_sums == 0]
    print('B %d order %d: %d window pixels, largest relative difference of the sums: p and Brier %.3g, NLL %.3g'
          % (B, order, window, rel[:, :B + 1].max(), rel[:, B + 1].max()))
    assert rel[:, :B + 1].max() <= 1e-9 and rel[:, B + 1].max() <= 1e-5
    return bins, sums


@pytest.mark.parametrize('B', (2, 10, 64))
@pytest.mark.parametrize('name', ('whole-53x41', 'crop-64x52', 'pad-47x36'))
def test_calibration_table_matches_the_fp32_rule(name, B, dev):
    for C, K in CHANNELS:
        prob = _case((45, 37), CASES['45x37'][1], C, K)[0][:S]
        for order in (0, 1):
            bins, sums = _check_table(prob, _truth(name, K), VALUES[:K], GEOMETRIES[name], B, order, dev)
            assert (bins[..., 1].sum(1) > 0).all() and np.count_nonzero(bins[..., 0]) > K          # positives, and more than one bin in use
            scores = U.scores(bins, sums)
            assert np.isfinite(scores).all() and (scores[:, 0] <= scores[:, 1]).all() and (scores[:, 0] > 0).all()


def test_calibration_table_past_the_grid_cap(dev):
    name = 'cap-516x512'
    raw_hw = GEOMETRIES[name][0]
    assert S * raw_hw[0] * raw_hw[1] > TABLE_CAP
    prob = _case((45, 37), CASES['45x37'][1], 5, 4)[0][:S]
    _check_table(prob, _truth(name, 4), VALUES[:4], GEOMETRIES[name], 10, 1, dev)


def test_a_map_that_equals_the_truth_is_perfectly_calibrated(dev):
    H, W, K = 23, 19, 4
    rng = np.random.RandomState(3)
    truth = rng.choice(np.asarray([0] + list(VALUES[:K]), np.uint8), size=(S, H, W))
    prob = np.stack([(truth == v) for v in VALUES[:K]] + [truth == 0], axis=-1).astype(np.float32)
    for order in (0, 1):
        bins, sums = _check_table(prob, truth, VALUES[:K], ((H, W), (H, W), (0, H, 0), (0, W, 0)), 10, order, dev)
        scores = U.scores(bins, sums)
        assert not scores[:, :3].any() and (scores[:, 4] == S * H * W).all() and not bins[:, 1:9].any()
        assert np.array_equal(bins[:, 9, 0], bins[:, 9, 1]) and not bins[:, 0, 1].any()


# ---- 7. uncertainty by error ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('n_shape', ((3, 41, 29), (1, 1, 1), (2, 300, 301)))          # the last: more than PO_MAXBLK * PO_BLOCK pixels
@pytest.mark.parametrize('planes', (1, 2, 4))
def test_uncertainty_by_error_counts_exactly(n_shape, planes, dev):
    from multimodal_segmentation_amd import ops
    rng = np.random.RandomState(planes)
    truth = rng.choice(np.asarray([0] + list(VALUES), np.uint8), size=n_shape)
    pred = np.where(rng.uniform(size=n_shape) < 0.3, rng.choice(np.asarray([0] + list(VALUES), np.uint8), size=n_shape), truth).astype(np.uint8)
    levels = rng.randint(0, 256, size=(planes,) + n_shape).astype(np.uint8)
    got = ops.uncertainty_by_error(_up(pred, dev), _up(truth, dev), _up(levels, dev))
    assert got.dtype == torch.int64 and tuple(got.shape) == (2, 1 + planes)
    assert np.array_equal(got.cpu().numpy(), U.by_error(pred, truth, list(levels)))
    same = ops.uncertainty_by_error(_up(truth, dev), _up(truth, dev), _up(levels, dev)).cpu().numpy()
    assert not same[1].any() and same[0, 0] == truth.size and np.array_equal(same[0, 1:], levels.reshape(planes, -1).astype(np.int64).sum(1))


# ---- 8. refusals --------------------------------------------------------------------------------------------------------------------------------
def test_entry_points_declared_and_bad_arguments_refused():
    from multimodal_segmentation_amd import _native, ops
    protos = _native.parse_header()
    geo = ['int'] * 13
    assert protos['mmseg_members_accumulate'] == ('int', ['const float*', 'const double*', 'float*', 'float*'] + ['int'] * 7 + ['void*'])
    assert protos['mmseg_members_finish'] == ('int', ['float*', 'float*'] + ['int'] * 4 + ['void*'])
    assert protos['mmseg_restore_map'] == ('int', ['const float*', 'unsigned char*'] + geo + ['int'] * 3 + ['void*'])
    assert protos['mmseg_calibration_table'] == ('int', ['const float*', 'const unsigned char*', 'const int*', 'int*', 'double*', 'double*']
                                                 + geo + ['int'] * 4 + ['void*'])
    assert protos['mmseg_calibration_table_workspace_bytes'] == ('long', ['int'] * 5)
    assert protos['mmseg_uncertainty_by_error'] == ('int', ['const unsigned char*'] * 3 + ['long long*', 'long', 'int', 'void*'])
    _native.build()
    lib = _native.load()
    bad = 1          # hipErrorInvalidValue; a refused call launches nothing and touches no memory, so the pointers need not be real

    def refuses(fn, ptrs, ok, changes, zero=None):
        assert all(fn(*(ptrs[:i] + [None] + ptrs[i + 1:] + ok + [None])) == bad for i in range(len(ptrs)))
        for i, v in changes:
            a = list(ok)
            a[i] = v
            assert fn(*(ptrs + a + [None])) == bad, (fn.__name__, a)
        if zero is not None:
            a = list(ok)
            a[zero] = 0
            assert fn(*(ptrs + a + [None])) == 0
    # first, V, N, OH, OW, C, K
    refuses(lib.mmseg_members_accumulate, [16, 32, 48, 64], [1, 4, 3, 32, 32, 5, 4],
            ((6, 6), (6, 0), (6, 17), (1, 17), (1, 0), (2, -1), (3, 0), (4, 0), (5, 0)), zero=2)
    assert lib.mmseg_members_accumulate(16, 32, 48, 64, 1, 1, 1 << 15, 128, 128, 4, 4, None) == bad          # exactly 2^29 pixels
    assert lib.mmseg_members_accumulate(16, 32, 48, 48, 1, 1, 3, 32, 32, 5, 4, None) == bad                   # sum and aux alias
    refuses(lib.mmseg_members_finish, [16, 32], [3, 32, 32, 4], ((3, 0), (3, 17), (0, -1), (1, 0), (2, 0)), zero=0)
    g = [3, 53, 41, 45, 37, 45, 37, 0, 45, 0, 0, 37, 0]          # S, H, W, RH, RW, OH, OW, rows, cols
    refuses(lib.mmseg_restore_map, [16, 32], g + [2, 1, 1], ((13, 5), (13, 0), (14, 2), (14, -1), (15, 2), (8, 46), (12, 1), (1, 0)), zero=0)
    # C, K, B, order
    refuses(lib.mmseg_calibration_table, [16, 32, 48, 64, 80, 96], g + [5, 4, 10, 1],
            ((14, 6), (14, 0), (14, 17), (15, 1), (15, 65), (16, 2), (8, 46), (2, 0)), zero=0)
    query = lib.mmseg_calibration_table_workspace_bytes
    assert query(3, 53, 41, 4, 10) == 8 * 26 * 4 * 12 and query(3, 516, 512, 4, 10) == 8 * 1024 * 4 * 12          # ceil(6519 / 256) = 26 blocks
    assert query(3, 53, 41, 4, 1) == query(3, 53, 41, 4, 65) == query(3, 53, 41, 17, 10) == query(3, 0, 41, 4, 10) == query(0, 53, 41, 4, 10) == 0
    refuses(lib.mmseg_uncertainty_by_error, [16, 32, 48, 64], [100, 2], ((1, 5), (1, 0), (0, -1), (0, 2 ** 31 - 1)), zero=0)
    # the wrappers name themselves
    prob, back = torch.zeros(4 * 2, 8, 8, 5), A.tables('flips', 8, 8)[2]
    for args in ((prob.double(), back, 2, 4), (prob, back, 2, 6), (torch.zeros(17, 8, 8, 5), np.zeros((17, 6)), 1, 4), (prob, back, 3, 4),
                 (prob, back[:3], 2, 4), (prob, back, 2, 4, (torch.zeros(2, 8, 8, 3), torch.zeros(2, 8, 8, 2)))):
        with pytest.raises(ValueError, match='members_accumulate'):
            ops.members_accumulate(*args)
    for state in ((torch.zeros(2, 8, 8, 4), torch.zeros(2, 8, 8, 3)), (torch.zeros(2, 8, 8, 17), torch.zeros(2, 8, 8, 2)),
                  (torch.zeros(2, 8, 8, 4).double(), torch.zeros(2, 8, 8, 2))):
        with pytest.raises(ValueError, match='members_finish'):
            ops.members_finish(state)
    for planes, u, order in ((torch.zeros(2, 8, 8, 5), 0, 1), (torch.zeros(2, 8, 8, 2), 2, 1), (torch.zeros(2, 8, 8, 2), 0, 2)):
        with pytest.raises(ValueError, match='restore_map'):
            ops.restore_map(planes, u, (9, 9), (8, 8), (0, 8, 0), (0, 8, 0), order)
    truth, values = torch.zeros(8, 9, 9, dtype=torch.uint8), torch.as_tensor(VALUES, dtype=torch.int32)
    for p, t, v, B in ((prob, truth, values, 1), (prob, truth, values, 65), (prob[..., :3], truth, values, 10), (prob, truth[:3], values, 10),
                       (prob, truth.int(), values, 10)):
        with pytest.raises(ValueError, match='calibration_table'):
            ops.calibration_table(p, t, v, (8, 8), (0, 8, 0), (0, 8, 0), B)
    for p, t, l in ((truth, truth, torch.zeros(5, 8, 9, 9, dtype=torch.uint8)), (truth, truth[:3], torch.zeros(2, 8, 9, 9, dtype=torch.uint8)),
                    (truth, truth, torch.zeros(2, 8, 9, 9))):
        with pytest.raises(ValueError, match='uncertainty_by_error'):
            ops.uncertainty_by_error(p, t, l)
    assert tuple(ops.members_accumulate(torch.zeros(0, 8, 8, 5), back, 0, 4)[1].shape) == (0, 8, 8, 2)


# ---- 9. the predictor ---------------------------------------------------------------------------------------------------------------------------
SHIFTS = (0.0, 0.1, -0.12)          # of CENTRES, per member
HARD_CAP = 5e-3          # share of a file's pixels whose label may be undecidable (the mean of three sigmoids, refined or not)


def shifted_probabilities(x, shift):
    """tests/test_volume_tiles.organ_probabilities with every centre moved by `shift`: members that disagree at the organs' edges"""
    c = torch.as_tensor(CENTRES, dtype=x.dtype, device=x.device) + shift
    p = torch.sigmoid(12.0 * (0.18 - (x - c).abs()))
    return torch.cat([p, (1 - p.sum(-1, keepdim=True)).clamp(min=0)], dim=-1).contiguous()


class Member(Pointwise):
    def __init__(self, shift):
        Pointwise.__init__(self)
        self.shift = shift

    def predict_mask(self, modality_index, mode, image_list):
        self.batches.append(image_list[0].shape[0])
        return shifted_probabilities(image_list[modality_index], self.shift)


@pytest.fixture
def labelled_wide(wide_folder, dev):
    """wide_folder with the labels of the unshifted model as every file's truth"""
    from multimodal_segmentation_amd.volume_predictor import VolumePredictor
    clean = wide_folder + '_clean'
    VolumePredictor(Pointwise(), _conf()).run(wide_folder, clean)
    for name in sorted(os.listdir(clean)):
        if name.endswith('.npz'):
            with np.load(os.path.join(wide_folder, name)) as z, np.load(os.path.join(clean, name)) as c:
                arrays = dict({k: z[k] for k in z.files}, label=c['label'])
            np.savez_compressed(os.path.join(wide_folder, name), **arrays)
    return wide_folder


def _expected(loader, volume, m, tta, tiles, crf, dev):
    """the restatement for one file -> (labels, label-undecidable, levels [2], level-undecidable [2], the map the labels come from, its
    window).  With tiles the members are pointwise, so every tile shows a frame pixel alike and the blend of the tiles is the map of the
    whole frame (tests/test_volume_tiles._yardstick's argument)."""
    from multimodal_segmentation_amd.volume_predictor import check_tta, views_in
    rows, cols = loader.tile_plan(loader.upload_volume(volume)[1], m, (16, 16))[m]          # the default overlap: half of 32
    if tiles and len(rows) * len(cols) > 1:
        images, geometry = _whole_frames(loader, volume)
        RH, RW = geometry[m]['resampled']
        window = ((RH, RW), (0, RH, 0), (0, RW, 0))
    else:
        images, geometry = loader.load_volume_for_prediction(volume)
        window = (geometry[m]['resampled'], geometry[m]['rows'], geometry[m]['cols'])
    geo, N = geometry[m], int(images[m].shape[0])
    OH, OW = images[m].shape[1:3]
    views = check_tta(tta, (OH, OW, 1)) if tta and OH == OW == 32 else None
    shown = images if views is None else views_in(images, views)
    back = np.asarray(A.tables('id', OH, OW)[2] if views is None else views.back)
    probs = [shifted_probabilities(shown[m], s).cpu().numpy() for s in SHIFTS]
    mean, H, I, cnt = U.members(probs, [back] * len(SHIFTS), N, 4)
    planes = np.stack([H, I], axis=-1)
    if crf:
        mean = Q.refine(mean, images[m].cpu().numpy(), 4, Q.DEFAULTS)
    raw_hw = geo['raw_shape'][1:]
    label, _ = P.restore(mean, VALUES, raw_hw, window[0], window[1], window[2], 1)
    inside = P.window_mask(raw_hw, window[0], window[1], window[2])
    hard = (np.abs(P.sample(mean, 4, raw_hw, window[0], window[1], window[2], 1) - 0.5) < (Q.LABEL_BAND if crf else T.LABEL_BAND)).any(-1) & inside[None]
    levels = [U.levels(planes, u, raw_hw, window[0], window[1], window[2], 1) for u in (0, 1)]
    return label, hard, [l[0] for l in levels], [l[1] for l in levels], mean, window, geo


def _rows(path):
    lines = open(path).read().strip().split('\n')
    return lines[0], {l.split(', ')[0]: [float(x) for x in l.split(', ')[1:]] for l in lines[1:]}


@pytest.mark.parametrize('tta,tiles,crf', ((None, False, None), ('flips', False, None), (None, True, None), (None, False, 'default')),
                         ids=('plain', 'flips', 'tiles', 'crf'))
def test_predictor_matches_the_chained_restatement(tta, tiles, crf, labelled_wide, tmp_path, dev):
    from multimodal_segmentation_amd.loaders.volume_folder import VolumeFolderLoader
    from multimodal_segmentation_amd.volume_predictor import VolumePredictor
    out = str(tmp_path / 'out')
    models = [Member(s) for s in SHIFTS]
    VolumePredictor(models[0], _conf(), members=models[1:]).run(labelled_wide, out, tta=tta, tiles=tiles, crf=crf, calibration_bins=10)
    assert all(sum(mod.batches) == sum(models[0].batches) for mod in models)
    settings = json.load(open(os.path.join(out, 'predictions.json')))
    assert settings['ensemble'] == ['nowhere', None, None] and settings['uncertainty'] is False and settings['calibration_bins'] == 10
    loader = VolumeFolderLoader(labelled_wide)
    B, tiled_files, reliability = 10, 0, {}
    for m, mod in enumerate(loader.modalities):
        cal = _rows(os.path.join(out, 'results_calibration_%s.csv' % mod))
        unc = _rows(os.path.join(out, 'results_uncertainty_%s.csv' % mod))
        assert cal[0] == 'Vol, ' + ', '.join('%s%d' % (n, k) for k in range(4) for n in ('ECE', 'MCE', 'Brier', 'NLL', 'N'))
        assert unc[0] == 'Vol, NCorrect, EntropyCorrect, MICorrect, NWrong, EntropyWrong, MIWrong'
        for v in sorted(loader.manifest['volumes']):
            fname = loader.manifest['volumes'][v][mod]['file']
            label, hard, levels, soft, mean, window, geo = _expected(loader, v, m, tta, tiles, crf, dev)
            tiled_files += window[1] == (0, window[0][0], 0) and tiles
            sel = geo['slices']
            with np.load(os.path.join(out, fname)) as z:
                got = z['label']
            with np.load(os.path.join(out, 'uncertainty', fname)) as z:
                planes = [z['entropy'], z['mutual_information']]
                assert sorted(z.files) == ['entropy', 'mutual_information', 'resolution'] and np.array_equal(z['resolution'], geo['resolution'])
            rest = np.setdiff1d(np.arange(got.shape[0]), sel)
            assert not got[rest].any() and not planes[0][rest].any() and not planes[1][rest].any()
            differing = int(np.count_nonzero((got[sel] != label) & ~hard))
            assert differing == 0 and np.count_nonzero(hard) <= HARD_CAP * hard.size and got[sel].any()
            worst = 0
            for u in (0, 1):
                assert planes[u].dtype == np.uint8 and planes[u].shape == got.shape
                off = np.abs(planes[u][sel].astype(np.int64) - levels[u])
                worst = max(worst, int(off.max()))
                assert not off[~soft[u]].any() and off.max() <= 1 and np.count_nonzero(soft[u]) <= U.LEVEL_CAP * off.size
            assert planes[1].max() > 10 and planes[0].max() > 100          # the members disagree somewhere, and are unsure somewhere
            # calibration: the restatement's table of the map that the labels come from, against this file's truth
            truth = geo['label']
            p = P.sample(mean, 4, geo['raw_shape'][1:], window[0], window[1], window[2], 1)
            inside = np.broadcast_to(P.window_mask(geo['raw_shape'][1:], window[0], window[1], window[2])[None], truth.shape)
            near = 0
            bins, sums = np.zeros((4, B, 2), np.int64), np.zeros((4, B + 2))
            for k in range(4):
                pk, y = p[..., k][inside], (truth == VALUES[k])[inside]
                b = np.minimum(B - 1, (pk * B).astype(np.int64))
                edge = pk * B
                near += int(np.count_nonzero((np.abs(edge - np.round(edge)) < 1e-4) & (np.round(edge) >= 1) & (np.round(edge) <= B - 1)))
                bins[k, :, 0], bins[k, :, 1] = np.bincount(b, minlength=B), np.bincount(b[y], minlength=B)
                sums[k, :B] = np.bincount(b, weights=pk, minlength=B)
                sums[k, B], sums[k, B + 1] = ((pk - y) ** 2).sum(), (-np.log(np.maximum(np.where(y, pk, 1 - pk), 1e-6))).sum()
            held = reliability.setdefault(mod, [np.zeros_like(bins), np.zeros_like(sums), 0])
            held[0] += bins
            held[1] += sums
            held[2] += near
            want = U.scores(bins, sums)
            row = np.asarray(cal[1][v]).reshape(4, 5)
            print('volume %s %s: %d label and up to %d level pixels undecidable, levels off by at most %d, %d probabilities near a bin edge; '
                  'ECE %s' % (v, mod, np.count_nonzero(hard), max(np.count_nonzero(s) for s in soft), worst, near,
                              ' '.join('%.4f' % e for e in row[:, 0])))
            assert np.array_equal(row[:, 4], want[:, 4]) and (row[:, 4] == np.count_nonzero(inside)).all()
            assert np.abs(row[:, [0, 2, 3]] - want[:, [0, 2, 3]]).max() <= 1e-3          # a pixel that changes its bin moves these by 1 / n
            if near == 0:
                assert np.abs(row[:, 1] - want[:, 1]).max() <= 1e-3          # MCE may rest on a bin of one pixel
            # uncertainty by error, on the final labels
            wrong = label != truth
            total = np.asarray(unc[1][v]).reshape(2, 3)
            assert total[0, 0] + total[1, 0] == label.size and abs(total[1, 0] - np.count_nonzero(wrong)) <= np.count_nonzero(hard)
            for r, mask in enumerate((~wrong, wrong)):
                for u in (0, 1):
                    if np.count_nonzero(mask) > 50 * max(1, np.count_nonzero(hard)):
                        assert abs(total[r, 1 + u] - levels[u][mask].mean() / 255.0) <= 2e-3
    assert (tiled_files >= 1) == bool(tiles)
    for mod, (bins, sums, near) in reliability.items():
        lines = open(os.path.join(out, 'reliability_%s.csv' % mod)).read().strip().split('\n')
        assert lines[0] == 'Organ, Bin, Lo, Hi, N, Confidence, Frequency' and len(lines) == 1 + 4 * B
        table = np.asarray([[float(x) for x in l.split(', ')] for l in lines[1:]]).reshape(4, B, 7)
        assert np.array_equal(table[..., 4].sum(1), bins[..., 0].sum(1))
        if near == 0:
            assert np.array_equal(table[..., 4], bins[..., 0])
            some = bins[..., 0] > 20
            assert np.abs(table[..., 5][some] - (sums[:, :B] / np.maximum(bins[..., 0], 1))[some]).max() <= 1e-3
            assert np.abs(table[..., 6][some] - (bins[..., 1] / np.maximum(bins[..., 0], 1.0))[some]).max() <= 1e-3


def test_nothing_new_requested_writes_the_same_bytes(labelled_wide, tmp_path, dev):
    """the parent's code path: VolumePredictor without members and run without uncertainty write what a predictor that knows neither
    writes (the options' defaults are spelled out in the second run), file by file; one model with uncertainty=True keeps the labels"""
    from multimodal_segmentation_amd import ops
    from multimodal_segmentation_amd.volume_predictor import VolumePredictor
    base, again, unsure = (str(tmp_path / d) for d in ('base', 'again', 'unsure'))
    model = Pointwise()

    def new_op(*args, **kwargs):
        raise AssertionError('an op of the ensemble path ran')
    with pytest.MonkeyPatch.context() as mp:          # nothing new is launched
        for name in ('members_accumulate', 'members_finish', 'restore_map', 'calibration_table', 'uncertainty_by_error'):
            mp.setattr(ops, name, new_op)
        VolumePredictor(model, _conf()).run(labelled_wide, base, tta='flips')
    launched, model.batches = list(model.batches), []
    VolumePredictor(model, _conf(), members=None).run(labelled_wide, again, tta='flips', uncertainty=False, calibration_bins=10)
    assert model.batches == launched
    want = {name: open(os.path.join(base, name), 'rb').read() for name in sorted(os.listdir(base))}
    assert {name: open(os.path.join(again, name), 'rb').read() for name in sorted(os.listdir(again))} == want
    assert not any(key in json.loads(want['predictions.json']) for key in ('ensemble', 'uncertainty', 'calibration_bins'))
    assert not any(name.startswith(('uncertainty', 'reliability', 'results_calibration', 'results_uncertainty')) for name in want)
    VolumePredictor(Pointwise(), _conf()).run(labelled_wide, unsure, uncertainty=True, calibration_bins=5)
    settings = json.load(open(os.path.join(unsure, 'predictions.json')))
    assert settings['ensemble'] == ['nowhere'] and settings['uncertainty'] is True and settings['calibration_bins'] == 5
    plain = str(tmp_path / 'plain')
    VolumePredictor(Pointwise(), _conf()).run(labelled_wide, plain)
    for name in sorted(os.listdir(plain)):
        if name.endswith('.npz'):
            assert open(os.path.join(plain, name), 'rb').read() == open(os.path.join(unsure, name), 'rb').read()
            with np.load(os.path.join(unsure, 'uncertainty', name)) as z:
                assert not z['mutual_information'].any() and z['entropy'].any()
    assert len(open(os.path.join(unsure, 'reliability_t1.csv')).read().strip().split('\n')) == 1 + 4 * 5
    for bad in (1, 65, 2.5, True, None):
        with pytest.raises(ValueError, match='calibration_bins'):
            VolumePredictor(Pointwise(), _conf()).run(labelled_wide, str(tmp_path / 'no'), uncertainty=True, calibration_bins=bad)
    with pytest.raises(ValueError, match='members'):
        VolumePredictor(Pointwise(), _conf(), members=[Pointwise()] * 8)
    assert not os.path.exists(str(tmp_path / 'no'))


# ---- 10. the command line -----------------------------------------------------------------------------------------------------------------------
def test_cli_options_are_checked_before_a_model_is_built(monkeypatch, tmp_path):
    from multimodal_segmentation_amd import experiment
    from tests.test_volume_predict import _stub_conf
    base = ['--config', 'dafnet_config_chaos', '--split', '0']
    args = experiment.parse_arguments(base)
    assert args.predict_ensemble is None and args.predict_uncertainty is False and args.predict_calibration_bins == 10
    args = experiment.parse_arguments(base + ['--predict_ensemble', 'a, b', '--predict_uncertainty', 'true', '--predict_calibration_bins', '20'])
    assert experiment.ensemble_folders(args.predict_ensemble) == ['a', 'b'] and args.predict_uncertainty is True
    assert args.predict_calibration_bins == 20

    def no_model(*args, **kwargs):
        raise AssertionError('the run went on past the options')
    conf = _stub_conf(3)
    conf.folder, conf.model = str(tmp_path / 'run'), 'stub.Stub'
    monkeypatch.setattr(experiment.Experiment, 'get_config', lambda self, split, args: conf)
    monkeypatch.setattr(experiment.Experiment, 'init_logging', lambda self, conf: None)
    monkeypatch.setattr(experiment.Experiment, 'get_executor', no_model)
    monkeypatch.setattr(experiment, 'resolve', no_model)
    for bins in ('1', '65'):
        with pytest.raises(ValueError, match='--predict_calibration_bins'):
            experiment.Experiment().run(base + ['--predict_folder', 'G', '--predict_calibration_bins', bins])
    for listed in ('a,,b', ','.join('r%d' % i for i in range(8))):
        with pytest.raises(ValueError, match='--predict_ensemble'):
            experiment.Experiment().run(base + ['--predict_folder', 'G', '--predict_ensemble', listed])
    with pytest.raises(FileNotFoundError, match='--predict_ensemble'):          # a member folder without a checkpoint
        experiment.Experiment().run(base + ['--predict_folder', 'G', '--predict_ensemble', str(tmp_path / 'empty')])
    member = tmp_path / 'member'
    (member / 'models').mkdir(parents=True)
    (member / 'models' / 'D_Mask').write_text('')
    for key, theirs in (('num_masks', 3), ('input_shape', [32, 32, 1]), ('model', 'mmsdnet.MMSDNet')):
        (member / 'experiment_configuration.json').write_text(json.dumps({key: theirs}))
        conf.model = 'stub.Stub'
        with pytest.raises(ValueError, match='--predict_ensemble.*%s' % key):
            experiment.Experiment().run(base + ['--predict_folder', 'G', '--predict_ensemble', str(member)])
    (member / 'experiment_configuration.json').write_text(json.dumps(dict(num_masks=4, input_shape=[64, 64, 1], model='stub.Stub')))
    with pytest.raises(AssertionError, match='past the options'):          # this member passes, and the run goes on to build the model
        experiment.Experiment().run(base + ['--predict_folder', 'G', '--predict_ensemble', str(member)])


def test_experiment_with_its_own_copy_as_the_only_member(tmp_path, dev, monkeypatch, caplog):
    from tests.test_volume_holes import _experiment
    folder = str(tmp_path / 'volumes')
    R.tool().write_folder(folder, volumes=3, size=64, slices=3, seed=6)
    model = Pointwise()
    run = str(tmp_path / 'run')
    exp = _experiment(monkeypatch, model, run)
    copy = str(tmp_path / 'copy')
    os.makedirs(copy)
    json.dump(dict(num_masks=4, input_shape=[64, 64, 1], intensity=dict(mode='window')), open(os.path.join(copy, 'experiment_configuration.json'), 'w'))
    plain, both = str(tmp_path / 'plain'), str(tmp_path / 'both')
    base = ['--config', 'dafnet_config_chaos', '--split', '0', '--test', 'true', '--predict_folder', folder]
    exp.run(base + ['--predict_out', plain])
    once, model.batches = sum(model.batches), []
    with caplog.at_level('WARNING'):
        exp.run(base + ['--predict_out', both, '--predict_ensemble', copy])
    assert sum(model.batches) == 2 * once
    assert any(copy in r.getMessage() and 'records' in r.getMessage() for r in caplog.records)          # warn_predict_stages about the member
    settings = json.load(open(os.path.join(both, 'predictions.json')))
    assert settings['ensemble'] == [run, None] and settings['uncertainty'] is False
    for name in sorted(os.listdir(plain)):
        if name.endswith('.npz'):
            assert open(os.path.join(plain, name), 'rb').read() == open(os.path.join(both, name), 'rb').read()
            with np.load(os.path.join(both, 'uncertainty', name)) as z:
                assert not z['mutual_information'].any() and z['entropy'].any()


def test_uncertainty_bench_tool_is_importable():
    """tools/volume_uncertainty_bench.py refuses to time anything without a GPU, and says so"""
    import importlib.util
    spec = importlib.util.spec_from_file_location('volume_uncertainty_bench', os.path.join(R.ROOT, 'tools', 'volume_uncertainty_bench.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    assert callable(mod.main)
    if not torch.cuda.is_available():
        with pytest.raises(SystemExit, match='GPU'):
            mod.main([])
