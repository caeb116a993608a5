"""Alignment of a volume's modalities by mutual information: csrc/align.hip (mmseg_align_*), ops.align_*, the `align` block of
loaders/volume_folder.py and tools/make_volume_folder.py --misalign, against the numpy restatement in tests/volume_align_ref.py (the rule is
in include/mmseg_hip.h).  Every measured figure is printed before it is asserted (pytest -s shows them)."""
import json
import os

import numpy as np
import pytest
import torch

from multimodal_segmentation_amd import loaders, nn, ops
from multimodal_segmentation_amd.loaders import volume_folder as VF
from tests import volume_align_ref as A
from tests import volume_bias_ref as B
from tests import volume_denoise_ref as D
from tests import volume_intensity_ref as I
from tests import volume_loader_ref as R
from tests import volume_predict_ref as P

gpu = pytest.mark.gpu
DEV = 'cuda:0'
PIXELS = 12
SEARCH = dict(bins=16, levels=3, max_slices=3, min_overlap=0.5)
LEAD = 1e-6          # the restatement's best must lead its runner-up by this at every stage, or the fixture is a bad one

_cache = {}


@pytest.fixture(autouse=True)
def _clean_registries():
    saved = dict(loaders.data_conf), dict(loaders.align_conf)
    yield
    for registry, old in zip((loaders.data_conf, loaders.align_conf), saved):
        registry.clear()
        registry.update(old)


def _install(monkeypatch):
    from tests import cpu_backend as cb
    for table in (R.STANDINS, I.STANDINS, B.STANDINS, D.STANDINS, P.STANDINS, A.STANDINS):
        for name, fn in table.items():
            monkeypatch.setitem(cb._TABLE, name, fn)
    monkeypatch.setattr(A, 'CALLS', [])
    cb.install()
    nn.set_default_device('cpu')
    return cb


@pytest.fixture(params=[pytest.param('cpu', id='cpu-standin'), pytest.param('cuda', marks=pytest.mark.gpu, id='mi355x')])
def device(request, monkeypatch):
    if request.param == 'cpu':
        cb = _install(monkeypatch)
        yield 'cpu'
        cb.uninstall()
    else:
        nn.set_default_device(DEV)
        yield 'cuda'


def _folders(tmp_path_factory, modalities=('t1', 't2'), seed=0):
    """(misaligned folder, the same canvases written aligned, truth), written once per (modalities, seed)"""
    key = ('folders', tuple(modalities), seed)
    if key not in _cache:
        root = tmp_path_factory.mktemp('align')
        mis, ali = str(root / 'misaligned'), str(root / 'aligned')
        R.tool().write_folder(mis, volumes=3, size=64, slices=6, seed=seed, modalities=modalities, misalign=PIXELS)
        R.tool().write_folder(ali, volumes=3, size=64, slices=6, seed=seed, modalities=modalities, misalign=PIXELS, misalign_aligned=True)
        truth = json.load(open(os.path.join(mis, 'misalignment.json')))
        _cache[key] = mis, ali, truth
    return _cache[key]


@pytest.fixture
def folders(tmp_path_factory):
    return _folders(tmp_path_factory)


def _volume(folder, volume, modality):
    m = json.load(open(os.path.join(folder, 'dataset.json')))
    z = np.load(os.path.join(folder, m['volumes'][str(volume)][modality]['file']))
    return z['image'], z['label'], z['resolution'], m


def _set_block(folder, block, key='align'):
    path = os.path.join(folder, 'dataset.json')
    m = json.load(open(path))
    m.pop(key, None)
    if block is not None:
        m[key] = block
    json.dump(m, open(path, 'w'))


# ---- 1 histograms, exact ------------------------------------------------------------------------------------------------------------------
SHAPE_A, SHAPE_B = (5, 37, 41), (7, 33, 46)
# c_a = (3, 5), c_b = (1, 7) at O = 32: rows of A at o in [-3, 34), of B at o in [-1 - dy, 32 - dy)
CANDIDATES = [(0, 0, 0), (-1, -5, 7), (2, 9, -8), (1, 3, 40), (0, -30, -38),          # window coordinates below 0 on both sides
              (6, 1, 1), (-4, 0, 2),                                                   # one slice left
              (7, 0, 0), (-5, 0, 0),                                                   # none left: N = 0
              (0, 34, 0), (0, -34, 1), (0, -33, 0),                                    # a single row (o = -3; 33; 32 and 33)
              (0, 0, 45)]                                                              # 13 candidates: no multiple of a wave, a block or a slab
WINDOWS = {'O=32': 32, 'O=(40,44)': (40, 44)}                                          # frames larger than O; smaller on rows, mixed on columns


def _bytes(bins, seed):
    rng = np.random.RandomState(seed)
    return rng.randint(0, bins, SHAPE_A).astype(np.uint8), rng.randint(0, bins, SHAPE_B).astype(np.uint8)


@gpu
@pytest.mark.parametrize('window', sorted(WINDOWS))
@pytest.mark.parametrize('stride', [1, 2, 4])
@pytest.mark.parametrize('bins', [2, 16, 64])
def test_histograms_equal_the_restatement_exactly(bins, stride, window):
    qa, qb = _bytes(bins, bins + stride)
    want = A.histograms(qa, qb, WINDOWS[window], CANDIDATES, stride, bins)
    n = want.reshape(len(CANDIDATES), -1).sum(1)
    print('pairs per candidate', n.tolist())
    for aggregate in (False, True):
        got = ops.align_histograms(torch.from_numpy(qa).to(DEV), torch.from_numpy(qb).to(DEV), WINDOWS[window], CANDIDATES, stride, bins,
                                   aggregate=aggregate)
        assert got.dtype == torch.int32 and tuple(got.shape) == (len(CANDIDATES), bins, bins)
        assert np.array_equal(got.cpu().numpy().astype(np.int64), want), aggregate


@gpu
@pytest.mark.parametrize('aggregate', [False, True])
def test_histogram_of_constant_frames_lands_in_one_bin(aggregate):
    """the contention path: every pair of a candidate meets the same LDS word"""
    qa, qb = np.full(SHAPE_A, 3, np.uint8), np.full(SHAPE_B, 9, np.uint8)
    got = ops.align_histograms(torch.from_numpy(qa).to(DEV), torch.from_numpy(qb).to(DEV), 32, CANDIDATES, 1, 16, aggregate=aggregate).cpu().numpy()
    for c, cand in enumerate(CANDIDATES):
        n = A.n_full_brute(SHAPE_A, SHAPE_B, 32, cand)
        assert got[c, 3, 9] == n and got[c].sum() == n, cand


def test_histogram_cases_are_what_their_comments_say():
    n = [A.n_full_brute(SHAPE_A, SHAPE_B, 32, c) for c in CANDIDATES]
    assert n[7] == 0 and n[8] == 0 and n[12] == 0 and n[5] == n[6] == 1 * 33 * 41          # one slice: the overlap of the frames, 33 x 41
    assert n[9] == n[10] == 5 * 1 * 41 and n[11] == 5 * 2 * 41                              # one row, two rows
    assert A.histogram(*_bytes(16, 1), 32, CANDIDATES[11], 2, 16).sum() == 5 * 1 * 20       # of which stride 2 samples row o = 32 alone, 20 columns
    assert len(CANDIDATES) == 13


def test_closed_form_pair_count_equals_the_brute_force_count():
    rng = np.random.RandomState(3)
    cands = CANDIDATES + [tuple(int(v) for v in rng.randint(-50, 51, 3)) for _ in range(40)]
    for window in WINDOWS.values():
        for cand in cands:
            assert A.n_full_closed(SHAPE_A, SHAPE_B, window, cand) == A.n_full_brute(SHAPE_A, SHAPE_B, window, cand), (window, cand)


# ---- 2 scores -----------------------------------------------------------------------------------------------------------------------------------
H_MIN = 0.1


def _tables(bins, seed):
    """random tables with entropies above H_MIN, then the -1 cases: an empty table, a single occupied bin, and (the last candidate) a
    healthy table of a shift that keeps less than min_overlap"""
    rng = np.random.RandomState(seed)
    cands = [(0, 0, 0), (1, 2, -3), (-1, 4, 4), (0, -6, 1), (2, 0, 0), (0, 1, 0), (0, 0, 0), (0, 0, 0), (-3, 0, 0)]
    keep = 0.7 if bins > 2 else 1.0          # empty bins among the occupied ones; a 2 x 2 table would lose its entropy with them
    h = np.stack([rng.randint(1, 2000, (bins, bins)) * (rng.uniform(size=(bins, bins)) < keep) for _ in cands]).astype(np.int64)
    h[5] = rng.randint(1, 3, (bins, bins))                     # nearly uniform: the largest entropies
    h[6] = 0
    h[7] = 0
    h[7, bins - 1, 0] = 12345
    return h, cands


@pytest.mark.parametrize('bins', [2, 16, 64])
def test_score_tables_are_what_the_bar_assumes(bins):
    h, cands = _tables(bins, bins)
    assert not A.admissible(SHAPE_A, SHAPE_B, 32, cands[8], 0.5) and A.admissible(SHAPE_A, SHAPE_B, 32, cands[4], 0.5)          # 2 and 5 slices of 5
    for t in list(h[:6]) + [h[8]]:
        assert min(A.entropies(t)) >= H_MIN
    want = A.scores(h, SHAPE_A, SHAPE_B, 32, cands, 0.5)
    assert (want[6:, 0] == -1).all() and (want[:6, 0] > 0).all() and want[6, 1] == 0 and want[7, 1] == 12345


@gpu
@pytest.mark.parametrize('bins', [2, 16, 64])
def test_scores_against_the_fp64_restatement(bins):
    h, cands = _tables(bins, bins)
    min_overlap = 0.5
    want = A.scores(h, SHAPE_A, SHAPE_B, 32, cands, min_overlap)
    got = ops.align_scores(torch.from_numpy(h.astype(np.int32)).to(DEV), SHAPE_A, SHAPE_B, 32, cands, 1, min_overlap).cpu().numpy()
    bar = A.score_bar(bins, H_MIN)
    err = np.abs(got[:, 0] - want[:, 0]).max()
    print('bins %d: largest score error %.3e, bar %.3e; scores %s' % (bins, err, bar, np.round(want[:, 0], 6).tolist()))
    assert np.array_equal(got[:, 1], want[:, 1])          # N
    assert (want[6:, 0] == -1).all() and (got[6:, 0] == -1).all() and (want[:6, 0] > 0).all()
    assert err <= bar
    free = ops.align_scores(torch.from_numpy(h.astype(np.int32)).to(DEV), SHAPE_A, SHAPE_B, 32, cands, 1, 0.0).cpu().numpy()
    assert free[8, 0] > 0 and free[6, 0] == -1          # without the floor the last candidate scores


def test_score_bar_is_about_1e_minus_12():
    assert 1e-12 < A.score_bar(64, H_MIN) < 3e-12 and A.score_bar(2, H_MIN) < 2e-14


# ---- 3 quantise --------------------------------------------------------------------------------------------------------------------------------
QUANTISE = {'identity': ((1.89, 1.89), (3, 40, 52)), 'up': ((2.4, 2.1), (3, 31, 45)), 'down': ((1.3, 1.5), (2, 58, 50))}


def _scan(shape, seed):
    """int16 over most of its range (so that few grey values sit on a decision point), a third of it air"""
    rng = np.random.RandomState(seed)
    S, H, W = shape
    y, x = np.mgrid[0:H, 0:W]
    body = ((y - H / 2.0) ** 2 / (0.4 * H) ** 2 + (x - W / 2.0) ** 2 / (0.42 * W) ** 2) < 1
    img = rng.uniform(2000, 30000, shape) * body[None] * (0.6 + 0.4 * np.sin(x / 7.0 + rng.uniform(0, 3)))[None]
    return np.round(img).astype(np.int16)


def _quantise_case(name, bins):
    res, shape = QUANTISE[name]
    image = _scan(shape, len(name))
    RH, RW = R.out_extent(shape[1], res[0], 1.89), R.out_extent(shape[2], res[1], 1.89)
    q, position, knots = A.quantise(image, RH, RW, bins)
    return image, (RH, RW), q, A.undecidable(position, bins), knots


@pytest.mark.parametrize('bins', [16, 64])
@pytest.mark.parametrize('name', sorted(QUANTISE))
def test_quantise_inputs_stay_inside_the_cap(name, bins):
    image, resampled, q, left_out, knots = _quantise_case(name, bins)
    print('%s, %d bins: %d of %d pixels undecidable, levels used %d' % (name, bins, left_out.sum(), left_out.size, len(np.unique(q))))
    assert left_out.mean() <= A.CAP and len(np.unique(q)) == bins and knots[1] > knots[0]


@gpu
@pytest.mark.parametrize('bins', [16, 64])
@pytest.mark.parametrize('name', sorted(QUANTISE))
def test_quantise_against_the_restatement(name, bins):
    image, resampled, want, left_out, knots = _quantise_case(name, bins)
    x = torch.from_numpy(image.astype(np.float32)).to(DEV)
    n = image.shape[0] * resampled[0] * resampled[1]
    dev_knots = ops.preprocess_quantiles(x, resampled, I.ranks(n, (0.5, 99.5)), True)
    got = ops.align_quantise(x, resampled, dev_knots, bins).cpu().numpy()
    wrong = (got != want) & ~left_out
    print('%s, %d bins: knots %s (restatement %s), %d undecidable, %d wrong' % (name, bins, dev_knots.cpu().numpy().tolist(), list(knots),
                                                                                   left_out.sum(), wrong.sum()))
    assert left_out.mean() <= A.CAP
    assert got.dtype == np.uint8 and got.shape == want.shape and not wrong.any()


@gpu
def test_quantise_of_a_constant_volume_is_zero():
    x = torch.full((2, 9, 11), 7.0, device=DEV)
    knots = ops.preprocess_quantiles(x, (9, 11), I.ranks(2 * 99, (0.5, 99.5)), True)
    assert float(knots[0, 0]) == float(knots[0, 1])
    assert not ops.align_quantise(x, (9, 11), knots, 32).any()


# ---- 4 selection --------------------------------------------------------------------------------------------------------------------------------
def _select(scores, stage, stride=1, state=None):
    sc = torch.tensor([[s, 10.0 + i] for i, s in enumerate(scores)], dtype=torch.float64, device=DEV)
    return ops.align_select(sc, stage, stride, state).cpu().numpy()


@gpu
def test_selection_follows_the_tie_rule():
    cands = [(2, 0, 0), (-1, 3, 0), (1, 0, 3), (1, -3, 0), (1, 0, -3), (0, 5, 5), (0, 9, 9)]
    table = [1.5, 1.5, 1.5, 1.5, 1.5, 1.2, -1.0]
    want = A.select(np.array([[s, 0] for s in table]), cands, False)[0]
    st = _select(table, cands)
    assert tuple(st[:3]) == want == (-1, 3, 0) and st[3] == 1.5 and st[5] == 11.0 and st[6] == 1.0 and st[7] == 1.0
    assert tuple(_select(table[1:5], cands[1:5])[:3]) == (-1, 3, 0)          # dz^2 ties: then dy^2 + dx^2 ties: then lexicographic, dz first
    assert tuple(_select(table[2:5], cands[2:5])[:3]) == (1, -3, 0)
    assert tuple(_select(table[:1] + [1.5], [(2, 0, 0), (-2, 0, 0)])[:3]) == (-2, 0, 0)
    assert tuple(_select([1.2, 1.5 + 1e-15], [(0, 0, 0), (3, 9, 9)])[:3]) == (3, 9, 9)          # the score comes first, by any margin
    many = [(0, i, -i) for i in range(700)]                      # more candidates than threads: the best sits in a later round
    assert tuple(_select([1.0] * 650 + [1.25] + [1.0] * 49, many)[:3]) == (0, 650, -650)


@gpu
def test_selection_without_an_admissible_candidate_is_the_zero_shift():
    st = _select([-1.0, -1.0, -1.0], [(1, 2, 3), (0, 1, 0), (2, 2, 2)])
    assert st[:7].tolist() == [0, 0, 0, -1.0, 0.0, 0.0, 0.0]
    state = torch.tensor([1, 4, -4, 0, 0, 0, 0, 0], dtype=torch.float64, device=DEV)
    st = _select([-1.0] * 27 + [1.01], ('refine', 3, 12, 12, state), 2)          # the probe's record is reported, and it is never selected
    assert st[:7].tolist() == [0, 0, 0, 1.01, 1.01, 37.0, 0.0]


@gpu
def test_selection_keeps_to_the_range():
    """a refinement stage centred on the corner of the range: the candidates beyond it hold the highest scores and are skipped"""
    Z, Py, Px, t = 3, 12, 10, 2
    centre = (3, 12, -10)
    cands = A.stage_candidates(A.MODE_REFINE, t, Z, Py, Px, centre)
    raw = [(centre[0] + jz, centre[1] + jy * t, centre[2] + jx * t) for jz in (-1, 0, 1) for jy in (-1, 0, 1) for jx in (-1, 0, 1)]
    table = [2.0 if c is None else 1.0 + 0.01 * i for i, c in enumerate(cands[:-1])] + [1.9]
    assert sum(c is None for c in cands) == 27 - 8
    state = torch.tensor(list(centre) + [0] * 5, dtype=torch.float64, device=DEV)
    st = _select(table, ('refine', Z, Py, Px, state), t)
    best = max((i for i in range(27) if cands[i] is not None), key=lambda i: table[i])
    assert tuple(st[:3]) == raw[best] == A.select(np.array([[s, 0] for s in table]), cands, True)[0]
    assert st[3] == table[best] and st[4] == 1.9 and abs(st[0]) <= Z and abs(st[1]) <= Py and abs(st[2]) <= Px
    lattice = A.stage_candidates(A.MODE_LATTICE, 4, 1, 9, 5)          # 3 x 5 x 3 and the probe
    assert len(lattice) == 46 and lattice[0] == (-1, -8, -4) and lattice[44] == (1, 8, 4)
    st = _select([1.0 + 0.001 * i for i in range(45)] + [3.0], ('lattice', 1, 9, 5), 4)
    assert tuple(st[:3]) == (1, 8, 4) and st[4] == 3.0


# ---- 5 the search recovers a known shift ------------------------------------------------------------------------------------------------------
def _params(manifest, **over):
    p = {k: v for k, v in manifest['align'].items() if k != 'mode'}
    p.update(SEARCH)
    p.update(over)
    return p


def _reference_record(folder, volume, ref, moving, params):
    key = ('record', folder, volume, ref, moving, json.dumps(params, sort_keys=True))
    if key not in _cache:
        a, _, res_a, m = _volume(folder, volume, ref)
        b, _, res_b, _ = _volume(folder, volume, moving)
        _cache[key] = A.align(a, res_a, b, res_b, m['target_resolution'], m['input_shape'], params)
    return _cache[key]


def _device_record(folder, volume, ref, moving, params):
    a, _, res_a, m = _volume(folder, volume, ref)
    b, _, res_b, _ = _volume(folder, volume, moving)
    dev = nn.default_device()
    return ops.align_volumes(nn.host_to_device(a, dev, np.float32), res_a, nn.host_to_device(b, dev, np.float32), res_b,
                             m['target_resolution'], m['input_shape'], params)


@pytest.mark.parametrize('volume', [1, 2])
def test_search_recovers_the_known_shift(device, folders, volume):
    mis, _, truth = folders
    m = json.load(open(os.path.join(mis, 'dataset.json')))
    params = _params(m)
    assert int(params['max_shift_mm'] // m['target_resolution'][0]) == PIXELS
    for ref, moving, sign in (('t1', 't2', 1), ('t2', 't1', -1)):          # the other way round: the shift changes its sign (dz < 0)
        want = _reference_record(mis, volume, ref, moving, params)
        print('volume %d, %s against %s: restatement %s, leads %s' % (volume, moving, ref, want['shift'], want['leads']))
        assert min(want['leads']) >= LEAD, 'bad fixture: a near-tie in the restatement'
        shift, (score, zero, n) = _device_record(mis, volume, ref, moving, params)
        print('    device %s score %.12f (restatement %.12f) zero %.12f (%.12f) N %d' % (shift, score, want['score'], zero, want['zero'], n))
        assert shift == want['shift'] == tuple(sign * v for v in truth[str(volume)]['t2'])
        assert n == want['n'] and abs(score - want['score']) <= A.score_bar(16, H_MIN) and abs(zero - want['zero']) <= A.score_bar(16, H_MIN)
        assert score > zero


def test_truth_outside_the_range_comes_back_clamped(device, folders):
    mis, _, truth = folders
    m = json.load(open(os.path.join(mis, 'dataset.json')))
    volume, limit = 1, 4
    t = truth[str(volume)]['t2']
    assert abs(t[1]) > limit and abs(t[2]) <= limit, 'bad fixture: rows beyond the range, columns within it'
    params = _params(m, max_shift_mm=(limit + 0.5) * m['target_resolution'][0])
    want = _reference_record(mis, volume, 't1', 't2', params)
    assert min(want['leads']) >= LEAD, 'bad fixture: a near-tie in the restatement'
    shift, _ = _device_record(mis, volume, 't1', 't2', params)
    print('truth %s, range %d: %s (restatement %s)' % (t, limit, shift, want['shift']))
    assert shift == want['shift'] == (t[0], int(np.sign(t[1])) * limit, t[2])


def test_two_runs_are_bitwise_equal(device, folders):
    mis = folders[0]
    a, _, res, m = _volume(mis, 3, 't1')
    b = _volume(mis, 3, 't2')[0]
    dev = nn.default_device()
    states = []
    for _ in range(2):
        qs = []
        for x in (a, b):
            xd = nn.host_to_device(x, dev, np.float32)
            knots = ops.preprocess_quantiles(xd, x.shape[1:], I.ranks(x.size, (0.5, 99.5)), True)
            qs.append(ops.align_quantise(xd, x.shape[1:], knots, 16))
        states.append((ops.align_search(qs[0], qs[1], 64, 3, PIXELS, PIXELS, 16, 3, 0.5).clone(), qs))
    assert torch.equal(states[0][0], states[1][0]) and states[0][0][7] == 3 and states[0][0][6] == 1
    assert all(torch.equal(p, q) for p, q in zip(states[0][1], states[1][1]))
    if device == 'cpu':          # three stages of three launches: the lattice of 7 x 7 x 7 and the probe, then twice 27 and the probe
        assert [c[1:] for c in A.CALLS[-9:]] == [(1, 4, 344)] * 3 + [(2, 2, 28)] * 3 + [(2, 1, 28)] * 3


# ---- 6 the loader ----------------------------------------------------------------------------------------------------------------------------------
def _common(a, b):
    """the two [S,h,w] arrays, every slice rescaled by its own extremes: equal for two affine images of the same values (the containers
    are scaled per slice by the extremes of the whole frame, and the two frames are different windows of the canvas)"""
    out = []
    for v in (a.astype(np.float64), b.astype(np.float64)):
        lo, hi = v.min(axis=(1, 2), keepdims=True), v.max(axis=(1, 2), keepdims=True)
        out.append((v - lo) / np.maximum(hi - lo, 1e-30))
    return out


def test_misaligned_folder_loads_as_the_aligned_one(device, folders):
    """no `slices`, unequal counts: the kept runs and the windows are the ones the truth implies, and what the moving modality shows is what
    it shows in the folder written aligned, wherever both windows lie inside their frames"""
    mis, ali, truth = folders
    lm, la = VF.VolumeFolderLoader(mis), VF.VolumeFolderLoader(ali)
    assert lm.align['mode'] == 'mi' and lm.align['reference'] == 't1' and la.align == {'mode': 'off'}
    for volume in (1, 2):
        dz, dy, dx = truth[str(volume)]['t2']
        images, geo = lm.load_volume_for_prediction(volume)
        want_images, want_geo = la.load_volume_for_prediction(volume)
        assert geo[0]['shift'] == (0, 0, 0) and geo[1]['shift'] == (dz, dy, dx) and 'shift' not in want_geo[0]
        assert geo[0]['slices'] == want_geo[0]['slices'] == list(range(6))
        assert geo[1]['slices'] == want_geo[1]['slices'] == list(range(dz, dz + 6))
        assert [i.shape[0] for i in images] == [6, 6]
        assert geo[0]['rows'] == want_geo[0]['rows'] and geo[0]['cols'] == want_geo[0]['cols']          # the reference keeps crop_pad_map
        assert torch.equal(images[0], want_images[0])
        RH, RW = geo[1]['resampled']
        for axis, (R_, d) in enumerate(((RH, dy), (RW, dx))):
            key = ('rows', 'cols')[axis]
            assert geo[1][key] == (VF.tile_window(VF.centre_start(R_, 64) + d, R_, 64) if d else VF.crop_pad_map(R_, 64))
        # container index o of the misaligned frame reads what o reads in the aligned frame, where neither is padded
        inside = []
        for key in ('rows', 'cols'):
            (lo, kept, before), (lo2, kept2, before2) = geo[1][key], want_geo[1][key]
            inside.append(slice(max(before, before2), min(before + kept, before2 + kept2)))
        got, want = _common(nn.to_numpy(images[1])[:, inside[0], inside[1], 0], nn.to_numpy(want_images[1])[:, inside[0], inside[1], 0])
        print('volume %d: common window %s, largest difference %.2e' % (volume, inside, np.abs(got - want).max()))
        assert inside[0].stop - inside[0].start >= 64 - PIXELS - 1 and np.abs(got - want).max() <= 1e-5
        assert np.array_equal(geo[1]['label'][:, :, :], _volume(mis, volume, 't2')[1][dz:dz + 6])
    # the training surface: the same pairing, labels included
    data = lm.load_all_modalities_concatenated(0, 'test', 1)
    want_data = la.load_all_modalities_concatenated(0, 'test', 1)
    v = lm.get_volumes_for_split(0, 'test')[0]
    g, wg = lm.load_volume_for_prediction(v)[1][1], la.load_volume_for_prediction(v)[1][1]
    inside = [slice(max(g[k][2], wg[k][2]), min(g[k][2] + g[k][1], wg[k][2] + wg[k][1])) for k in ('rows', 'cols')]
    assert data.get_masks_modi(1).shape == want_data.get_masks_modi(1).shape
    assert np.array_equal(data.get_masks_modi(1)[:, inside[0], inside[1]], want_data.get_masks_modi(1)[:, inside[0], inside[1]])
    assert np.array_equal(data.get_masks_modi(0), want_data.get_masks_modi(0)) and data.get_masks_modi(1).any()
    assert len(lm._alignments) == 3 or device == 'cuda'          # cached per volume


def test_without_the_key_nothing_changes(device, folders, tmp_path, monkeypatch):
    """`align` absent: no mmseg_align_* entry point is called and the containers of the existing fixture are what the preprocessing
    entry points give when called directly, as before; the misaligned folder is refused with the message it always got"""
    from multimodal_segmentation_amd import _native
    plain = str(tmp_path / 'plain')
    R.tool().write_folder(plain, volumes=3, size=32, slices=3, seed=1)
    loader = VF.VolumeFolderLoader(plain)
    assert loader.align == {'mode': 'off'} and loader.alignment(1, [], []) is None
    called = []
    real_call = _native.call
    _native.call = lambda name, *a: (called.append(name), real_call(name, *a))[1]
    try:
        images, geometry = loader.load_volume_for_prediction(1)
        raw, geometry2 = loader.upload_volume(1)
        data = loader.load_all_modalities_concatenated(0, 'training', 1)
    finally:
        _native.call = real_call
    assert called and not [n for n in called if n.startswith('mmseg_align')]
    dev = nn.default_device()
    values = nn.host_to_device(np.asarray(loader.label_values), dev, np.int32)
    v = loader.get_volumes_for_split(0, 'training')[0]
    for m, mod in enumerate(loader.modalities):
        image, label, res = loader.read_volume(1, mod)
        x = nn.host_to_device(image, dev, np.float32)
        RH, RW = VF.resampled_size(image.shape[1], res[0], 1.89), VF.resampled_size(image.shape[2], res[1], 1.89)
        rows, cols = VF.crop_pad_map(RH, 32), VF.crop_pad_map(RW, 32)
        container = torch.zeros((x.shape[0], 32, 32, 1), device=dev)
        ops.preprocess_images(x, container, (RH, RW), rows, cols, 0)
        assert torch.equal(images[m], container) and torch.equal(raw[m], x)
        assert geometry[m]['rows'] == rows and geometry[m]['cols'] == cols and 'shift' not in geometry[m] and 'shift' not in geometry2[m]
        image, label, res = loader.read_volume(v, mod)
        S = image.shape[0]
        RH, RW = VF.resampled_size(image.shape[1], res[0], 1.89), VF.resampled_size(image.shape[2], res[1], 1.89)
        im, ma = torch.zeros((S, 32, 32, 2), device=dev), torch.zeros((S, 32, 32, 8), device=dev)
        ops.preprocess_volume(nn.host_to_device(image, dev, np.float32), nn.host_to_device(label, dev, np.uint8), values, im, ma, (RH, RW),
                              VF.crop_pad_map(RH, 32), VF.crop_pad_map(RW, 32), m)
        assert np.array_equal(data.get_volume_images_modi(m, v)[..., 0], nn.to_numpy(im)[..., m])
        assert np.array_equal(data.get_volume_masks_modi(m, v), nn.to_numpy(ma)[..., 4 * m:4 * m + 4])
    mis = folders[0]
    copy = str(tmp_path / 'copy')
    os.makedirs(copy)
    for name in os.listdir(mis):
        os.symlink(os.path.join(mis, name), os.path.join(copy, name)) if name != 'dataset.json' else None
    json.dump(json.load(open(os.path.join(mis, 'dataset.json'))), open(os.path.join(copy, 'dataset.json'), 'w'))
    _set_block(copy, None)
    refused = VF.VolumeFolderLoader(copy)
    for load in (lambda: refused.load_volume_for_prediction(1), lambda: refused.load_all_modalities_concatenated(0, 'training', 1),
                 lambda: refused.upload_volume(1)):
        with pytest.raises(ValueError) as e:
            load()
        assert 'the modalities hold different numbers of slices after selection' in str(e.value) and 'state the matching' in str(e.value)


def test_training_load_launches_what_prediction_launches(device, tmp_path):
    """with denoise, bias_field and align on, a training load denoises and bias-corrects every (volume, modality) once, as prediction
    does: the same mmseg_nlm_* and mmseg_bias_* entry points, each as often"""
    from multimodal_segmentation_amd import _native
    folder = str(tmp_path / 'staged')
    R.tool().write_folder(folder, volumes=3, size=32, slices=3, seed=1)
    _set_block(folder, {'mode': 'nlm'}, 'denoise')
    _set_block(folder, {'mode': 'n3', 'extent': '2d', 'levels': 1, 'iterations': 1}, 'bias_field')
    _set_block(folder, {'mode': 'mi'})

    def recorded(load):
        loader, called = VF.VolumeFolderLoader(folder), []
        real_call = _native.call
        _native.call = lambda name, *a: (called.append(name), real_call(name, *a))[1]
        try:
            load(loader)
        finally:
            _native.call = real_call
        return sorted(n for n in called if n.startswith(('mmseg_nlm_', 'mmseg_bias_')))

    training = recorded(lambda loader: loader.load_all_modalities_concatenated(0, 'all', 1))
    prediction = recorded(lambda loader: [loader.load_volume_for_prediction(v) for v in loader.get_volumes_for_split(0, 'all')])
    print('training', len(training), 'prediction', len(prediction))
    assert [n for n in prediction if n.startswith('mmseg_nlm_')] and [n for n in prediction if n.startswith('mmseg_bias_')]
    assert training == prediction


def test_labels_return_to_the_file_grid(device, folders):
    """load_volume_for_prediction's record is all the way back needs: label containers written with its windows and pushed through
    mmseg_restore_label reproduce the file's own label on the file grid, inside the window"""
    mis, _, truth = folders
    loader = VF.VolumeFolderLoader(mis)
    dev = nn.default_device()
    values = nn.host_to_device(np.asarray(loader.label_values), dev, np.int32)
    for volume in (1, 2):
        images, geometry = loader.load_volume_for_prediction(volume)
        for m, g in enumerate(geometry):
            file_image, file_label = _volume(mis, volume, loader.modalities[m])[:2]
            S = len(g['slices'])
            assert np.array_equal(g['label'], file_label[g['slices']]) and images[m].shape[0] == S
            im, ma = torch.zeros((S, 64, 64, 1), device=dev), torch.zeros((S, 64, 64, 4), device=dev)
            ops.preprocess_volume(nn.host_to_device(file_image[g['slices']], dev, np.float32), nn.host_to_device(g['label'], dev, np.uint8),
                                  values, im, ma, g['resampled'], g['rows'], g['cols'], 0)
            assert torch.equal(im, images[m])
            back = nn.to_numpy(ops.restore_label(ma, values, g['raw_shape'][1:], g['resampled'], g['rows'], g['cols'], order=0))
            window = P.window_mask(g['raw_shape'][1:], g['resampled'], g['rows'], g['cols'])
            assert window.sum() >= (64 - PIXELS) ** 2 and g['label'][:, window].any()
            assert np.array_equal(back[:, window], g['label'][:, window]) and not back[:, ~window].any()


def test_tile_plan_follows_the_shift(device, folders, tmp_path):
    """in a window wide enough for every frame a plan is one tile, and the shifted modality's is load_volume_for_prediction's window"""
    mis = folders[0]
    wide = str(tmp_path / 'wide')
    os.makedirs(wide)
    for name in os.listdir(mis):
        os.symlink(os.path.join(mis, name), os.path.join(wide, name)) if name != 'dataset.json' else None
    m = json.load(open(os.path.join(mis, 'dataset.json')))
    m['input_shape'] = [80, 80, 1]
    json.dump(m, open(os.path.join(wide, 'dataset.json'), 'w'))
    loader = VF.VolumeFolderLoader(wide)
    images, geometry = loader.load_volume_for_prediction(2)
    shift = geometry[1]['shift']
    assert shift[1] and shift[2]
    raw, geometry2 = loader.upload_volume(2)
    assert geometry2[1]['shift'] == shift and [x.shape[0] for x in raw] == [i.shape[0] for i in images]
    plan = loader.tile_plan(geometry2, 0, (40, 40))
    assert plan[0] == ([geometry[0]['rows']], [geometry[0]['cols']]) and plan[1] == ([geometry[1]['rows']], [geometry[1]['cols']])
    tiles, _, _ = loader.load_volume_tiles(2, 0, (40, 40), uploaded=(raw, geometry2))
    assert all(torch.equal(t, i) for t, i in zip(tiles, images))
    back = loader.tile_plan(geometry2, 1, (40, 40))          # predicted from the moving side: the reference moves the other way
    RH, RW = geometry2[0]['resampled']
    assert back[0] == ([VF.tile_window(VF.centre_start(RH, 80) - shift[1], RH, 80)], [VF.tile_window(VF.centre_start(RW, 80) - shift[2], RW, 80)])


def test_three_modalities_keep_the_intersection(device, tmp_path_factory, monkeypatch):
    mis, _, truth = _folders(tmp_path_factory, ('t1', 't2', 't3'), seed=4)
    loader = VF.VolumeFolderLoader(mis)
    counts = [_volume(mis, 1, mod)[0].shape[0] for mod in loader.modalities]
    calls = []

    def fake(a, res_a, b, res_b, target, shape, params):
        calls.append(b.shape[0])
        return ((2, 1, 0) if len(calls) % 2 else (-1, 0, -2)), (1.1, 1.0, 100)

    monkeypatch.setattr(ops, 'align_volumes', fake)
    images, geometry = loader.load_volume_for_prediction(1)
    # reference slices [max(0, -2, 1), min(6, S_2 - 2, S_3 + 1)) = [1, min(6, S_2 - 2))
    hi = min(6, counts[1] - 2, counts[2] + 1)
    assert geometry[0]['slices'] == list(range(1, hi)) and geometry[1]['slices'] == list(range(3, hi + 2))
    assert geometry[2]['slices'] == list(range(0, hi - 1)) and [i.shape[0] for i in images] == [hi - 1] * 3
    loader.load_volume_for_prediction(1)
    assert len(calls) == 2          # cached per volume
    del calls[:]

    def apart(a, res_a, b, res_b, target, shape, params):
        calls.append(b.shape[0])
        return ((4, 0, 0) if len(calls) % 2 else (-6, 0, 0)), (1.1, 1.0, 100)

    monkeypatch.setattr(ops, 'align_volumes', apart)
    with pytest.raises(ValueError) as e:
        VF.VolumeFolderLoader(mis).load_volume_for_prediction(1)
    assert 'volume 1' in str(e.value) and 'no slice' in str(e.value) and '-6' in str(e.value)


def test_three_modalities_align_on_their_own(device, tmp_path_factory):
    mis, _, truth = _folders(tmp_path_factory, ('t1', 't2', 't3'), seed=4)
    loader = VF.VolumeFolderLoader(mis)
    _, geometry = loader.load_volume_for_prediction(2)
    print('truth', truth['2'], 'found', [g['shift'] for g in geometry])
    assert [list(g['shift']) for g in geometry[1:]] == [truth['2']['t2'], truth['2']['t3']]


# ---- settings ----------------------------------------------------------------------------------------------------------------------------------------
def test_settings_are_validated_with_the_key_named(folders, tmp_path):
    mis = folders[0]
    copy = str(tmp_path / 'copy')
    os.makedirs(copy)
    for name in os.listdir(mis):
        os.symlink(os.path.join(mis, name), os.path.join(copy, name)) if name != 'dataset.json' else None
    json.dump(json.load(open(os.path.join(mis, 'dataset.json'))), open(os.path.join(copy, 'dataset.json'), 'w'))
    full = dict(mode='mi', reference='t1', max_shift_mm=40.0, max_slices=4, bins=32, levels=3, min_overlap=0.5, percentiles=[0.5, 99.5])
    _set_block(copy, {'mode': 'mi'})
    assert VF.effective_setting(copy, 'align') == full
    _set_block(copy, {'mode': 'mi', 'reference': 't2', 'bins': 64})
    assert VF.effective_setting(copy, 'align') == dict(full, reference='t2', bins=64)
    for block, word in (({'mode': 'ncc'}, 'mode'), ({'mode': 'mi', 'reference': 'ct'}, 'reference'), ({'mode': 'mi', 'bins': 65}, 'bins'),
                        ({'mode': 'mi', 'bins': 1}, 'bins'), ({'mode': 'mi', 'levels': 0}, 'levels'), ({'mode': 'mi', 'max_slices': -1}, 'max_slices'),
                        ({'mode': 'mi', 'max_shift_mm': -1}, 'max_shift_mm'), ({'mode': 'mi', 'min_overlap': 0}, 'min_overlap'),
                        ({'mode': 'mi', 'min_overlap': 1.5}, 'min_overlap'), ({'mode': 'mi', 'percentiles': [99, 1]}, 'percentiles'),
                        ({'mode': 'mi', 'stride': 2}, 'stride'), ({'mode': 'off', 'bins': 8}, 'bins'), ('mi', 'object')):
        _set_block(copy, block)
        with pytest.raises(ValueError) as e:
            VF.VolumeFolderLoader(copy)
        assert '"align"' in str(e.value) and word in str(e.value) and 'dataset.json' in str(e.value), block
    _set_block(copy, {'mode': 'off'})
    loaders.align_conf['chaos'] = {'mode': 'mi', 'levels': 2}
    assert VF.VolumeFolderLoader(copy).align == dict(full, levels=2)
    loaders.align_conf['chaos'] = {'mode': 'mi', 'levels': 99}
    with pytest.raises(ValueError) as e:
        VF.VolumeFolderLoader(copy)
    assert "loaders.align_conf['chaos']" in str(e.value)


_GOLDEN_PLAIN = (698122, (2, 30, 28))          # (sum, shape) of vol01_t1 of write_folder(volumes=3, size=32, slices=2, seed=1) before --misalign existed


def test_generator_writes_the_same_bytes_without_the_option(tmp_path):
    """--misalign draws from a generator of its own: a folder written without it is what it was"""
    tool = R.tool()
    a, b = str(tmp_path / 'a'), str(tmp_path / 'b')
    tool.write_folder(a, volumes=3, size=32, slices=2, seed=1)
    assert tool.main([b, '--volumes', '3', '--size', '32', '--slices', '2', '--seed', '1']) is None
    for name in sorted(os.listdir(a)):
        if name.endswith('.npz'):
            p, s = np.load(os.path.join(a, name)), np.load(os.path.join(b, name))
            assert all(np.array_equal(p[k], s[k]) for k in p.files)
    assert not os.path.exists(os.path.join(a, 'misalignment.json'))
    image = np.load(os.path.join(a, 'vol01_t1.npz'))['image']
    assert (int(image.sum()), image.shape) == _GOLDEN_PLAIN          # the bytes of the parent commit's generator
    with pytest.raises(ValueError):
        tool.write_folder(str(tmp_path / 'bad'), misalign=-1)
    assert tool.main([str(tmp_path / 'cli'), '--volumes', '3', '--misalign', '5']) is None
    m = json.load(open(os.path.join(str(tmp_path / 'cli'), 'dataset.json')))
    t = json.load(open(os.path.join(str(tmp_path / 'cli'), 'misalignment.json')))
    assert m['align']['mode'] == 'mi' and all('slices' not in e for v in m['volumes'].values() for e in v.values())
    assert all(0 <= s[0] <= 2 and abs(s[1]) <= 5 and abs(s[2]) <= 5 for v in t.values() for s in v.values())




# ---- ABI ------------------------------------------------------------------------------------------------------------------------------------------
def test_entry_points_declared():
    from multimodal_segmentation_amd import _native
    protos = _native.parse_header()
    for name in A.STANDINS:
        assert name in protos, name
    _native.build()
    lib = _native.load()
    assert all(hasattr(lib, n) for n in protos if n.startswith('mmseg_align'))
    assert _native.call('mmseg_align_stage_candidates', 1, 4, 4, 21, 21) == 9 * 11 * 11 + 1
    assert _native.call('mmseg_align_stage_candidates', 2, 1, 4, 21, 21) == 28
    assert _native.call('mmseg_align_workspace_bytes', 1090, 32) == 1090 * 32 * 32 * 4 + 1090 * 16
    assert _native.call('mmseg_align_workspace_bytes', 70000, 32) == 0 and _native.call('mmseg_align_workspace_bytes', 10, 65) == 0
