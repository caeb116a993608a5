"""HD(q) and NSD(tau) of predicted label volumes: csrc/postprocess.hip (mmseg_masked_select, mmseg_surface_scores), ops.masked_select /
ops.surface_scores, `robust=(percentile, tolerance)` of volume_predictor.py, `--predict_robust` / `--predict_percentile` /
`--predict_tolerance` and tools/score_predictions.py, against the numpy / scipy restatement of tests/volume_robust_ref.py.

Comparison rules (set by the feature's issue).  The selection is exact: N, the count within the tolerance and the two order statistics
D_(lo), D_(hi) equal numpy.sort's bit for bit; the interpolated value is a few fp64 roundings from numpy's lerp, so 8 ulp of D_(hi).  On
volumes the distance maps are held to 1e-12 relative (REL_DISTANCE of test_volume_metrics.py) and an order statistic moves by no more
than the largest change of any element, so HD sits within 2e-12 * D_(hi) of the yardstick; the count equals it exactly (the inputs keep
every distance 5 % away from the tolerance); the first six columns are those of ops.surface_metrics bit for bit.  Two runs are bitwise
equal.

Grid-stride loops: the compaction and histogram kernels run at most 512 blocks of 256 threads, so their loops wrap from 131 073
elements on; the longest list, n = 200 003, is above that for the inputs and, with every content that selects more than 65 % of the
2 n values, for the list as well."""
import functools
import importlib.util
import json
import os

import numpy as np
import pytest
import torch

from tests import volume_loader_ref as R
from tests import volume_metrics_ref as M
from tests import volume_robust_ref as B
from tests.test_volume_loader import VALUES
from tests.test_volume_metrics import CASES, REL_DISTANCE, _case_data
from tests.volume_fixtures import _clean_registry, _csv_rows, _dev, _score_tool, _up, device  # noqa: F401

Q, TAU = 95.0, 2.0
COMBINED = ('7x40x36', 'one-slice', 'odd-45x38', 'k2', 'other-grey', '24x160x144')
LENGTHS = (1, 2, 63, 64, 65, 257, 200003)
WRAP = 512 * 256          # elements one sweep of the grid covers
PERCENTILES = (0.0, 50.0, 95.0, 99.9, 100.0)
CONTENTS = ('uniform', 'equal', 'lowest-bit', 'exponent', 'zeros', 'only-a', 'only-b', 'none', 'one-each')


def _bits(x):
    return np.ascontiguousarray(np.asarray(x, np.float64)).view(np.uint64)


@functools.lru_cache(maxsize=None)
def _yardstick(name, percentile=Q, tolerance=TAU):
    """(robust_table [K+1,8], per problem the sorted multiset D) of a case, computed once and never written to"""
    pred, truth, values, spacing = _case_data(name)
    table = B.robust_table(pred, truth, values, spacing, percentile, tolerance)
    lists = [np.sort(B.distances(p, t, spacing)) for p, t in zip(M.problems(pred, values), M.problems(truth, values))]
    table.setflags(write=False)
    return table, lists


# ---- the inputs and the yardstick alone (no GPU) -----------------------------------------------------------------------------------------
def test_robust_inputs_are_not_vacuous():
    for name in sorted(CASES):
        table, lists = _yardstick(name)
        hd, mssd, nsd = table[:, 7], table[:, 5], table[:, 6] / (table[:, 2] + table[:, 3])
        nearest = min(float(np.min(np.abs(d - TAU) / TAU)) for d in lists)
        ties = [d[B.ranks(d.size, Q)[0]] == d[B.ranks(d.size, Q)[1]] for d in lists]
        print('%s: HD95 %s mm, MSSD %s mm, ratio %s, NSD(%g) %s, nearest distance to the tolerance %.3g relative, D_(lo) == D_(hi): %s, '
              'zeros %s' % (name, np.round(hd, 3), np.round(mssd, 3), np.round(hd / mssd, 2), TAU, np.round(nsd, 3), nearest, ties,
                            np.round([np.mean(d == 0) for d in lists], 2)))
        assert np.isfinite(table).all() and all(d.size == table[k, 2] + table[k, 3] for k, d in enumerate(lists))
        assert (hd < 0.8 * mssd).all()                      # a kernel that returns the maximum is caught
        assert (nsd > 0.5).all() and (nsd < 1.0).all()
        assert nearest > 1e-6                               # rounding cannot flip a count


def test_a_dropped_axis_moves_the_percentile():
    """the yardstick with dz replaced by dy moves HD95 on at least one problem of every case with S > 1, by far more than the bar of the
    comparison could hide"""
    for name in sorted(CASES):
        pred, truth, values, (dz, dy, dx) = _case_data(name)
        if pred.shape[0] == 1:
            continue
        right = _yardstick(name)[0][:, 7]
        wrong = B.robust_table(pred, truth, values, (dy, dy, dx), Q, TAU)[:, 7]
        moved = np.abs(wrong - right) / right
        print('%s: HD95 moves by %s %%' % (name, np.round(100 * moved, 2)))
        assert float(np.max(moved)) > 100 * REL_DISTANCE


# ---- crafted lists -----------------------------------------------------------------------------------------------------------------------
def _crafted(content, n):
    """a, ma, b, mb of length n and the percentiles to ask for.  Unselected values are nan, negative or infinite: they must not count."""
    rng = np.random.RandomState(4000 + 31 * CONTENTS.index(content) + n % 1009)
    a, b = rng.rand(n) * 100.0, rng.rand(n) * 1e-3
    ma, mb = (rng.rand(n) < 0.7).astype(np.uint8), (rng.rand(n) < 0.7).astype(np.uint8)
    ma[0] = 1
    qs = list(PERCENTILES)
    if content == 'equal':
        a[:], b[:] = 3.25, 3.25
    elif content == 'lowest-bit':          # the last digit pass decides
        x = np.float64(1.75)          # an even bit pattern: the neighbour above differs in bit 0 alone
        a, b = np.where(rng.rand(n) < 0.5, x, np.nextafter(x, np.inf)), np.where(rng.rand(n) < 0.3, x, np.nextafter(x, np.inf))
    elif content == 'exponent':            # the first two passes decide: powers of two from 2^-1000 to 2^1000
        a, b = np.ldexp(1.0, rng.randint(-1000, 1001, n)), np.ldexp(1.0, rng.randint(-1000, 1001, n))
    elif content == 'zeros':               # 75 % exact zeros; one more percentile puts lo on the last zero and hi on the first positive value
        ma[:], mb[:] = 1, 1
        a[rng.rand(n) < 0.75], b[rng.rand(n) < 0.75] = 0.0, 0.0
        a[0] = 0.0
        zeros, total = int(np.count_nonzero(a == 0) + np.count_nonzero(b == 0)), 2 * n
        if zeros < total:
            qs.append(100.0 * (zeros - 0.5) / (total - 1))
    elif content == 'only-a':
        ma[:], mb[:] = 1, 0
    elif content == 'only-b':
        ma[:], mb[:] = 0, 1
    elif content == 'none':
        ma[:], mb[:] = 0, 0
    elif content == 'one-each':
        ma[:], mb[:] = 0, 0
        ma[n // 3], mb[(2 * n) // 3] = 1, 1
    a, b = a.astype(np.float64), b.astype(np.float64)
    junk = np.asarray([np.nan, -1.0, np.inf, -np.inf])
    a = np.where(ma != 0, a, junk[np.arange(n) % 4])
    b = np.where(mb != 0, b, junk[(np.arange(n) + 1) % 4])
    return a, ma, b, mb, qs


def _selected(a, ma, b, mb):
    return np.concatenate([a[ma != 0], b[mb != 0]])


def test_crafted_lists_exercise_interpolation_and_every_pass():
    """the volumes tie at lo and hi (lattice distances), so the crafted lists must exercise the interpolation: a case with D_(lo) < D_(hi)
    and 0 < h - lo < 1, among them the step from the last zero to the first positive value; and the longest list wraps the loops"""
    open_steps, zero_steps = 0, 0
    for content in CONTENTS:
        for n in LENGTHS:
            a, ma, b, mb, qs = _crafted(content, n)
            d = np.sort(_selected(a, ma, b, mb))
            assert d.size == 0 or (np.isfinite(d).all() and (d >= 0).all())
            if content == 'none':
                assert d.size == 0
            if content == 'one-each':
                assert d.size == 2
            if content == 'zeros' and n > 2:
                assert 0.6 < np.mean(d == 0) < 0.9 and len(qs) == len(PERCENTILES) + 1
            if n == LENGTHS[-1] and content in ('uniform', 'equal', 'lowest-bit', 'exponent', 'zeros'):
                assert n > WRAP and d.size > WRAP
            for q in qs:
                if d.size:
                    lo, hi, frac = B.ranks(d.size, q)
                    if d[lo] < d[hi] and 0.0 < frac < 1.0:
                        open_steps += 1
                        zero_steps += int(d[lo] == 0.0 and content == 'zeros' and q == qs[-1])
    print('%d (content, length, percentile) cases interpolate between two different values, %d of them from the last zero' % (open_steps, zero_steps))
    assert open_steps >= 10 and zero_steps >= len(LENGTHS) - 2
    a, ma, b, mb, _ = _crafted('lowest-bit', 257)
    assert len(set(_bits(_selected(a, ma, b, mb)) >> np.uint64(1))) == 1 and len(set(_bits(_selected(a, ma, b, mb)))) == 2
    a, ma, b, mb, _ = _crafted('exponent', 257)
    assert not (_bits(_selected(a, ma, b, mb)) & np.uint64((1 << 52) - 1)).any()


def _check_selection(content, n, dev):
    from multimodal_segmentation_amd import ops
    a, ma, b, mb, qs = _crafted(content, n)
    d = np.sort(_selected(a, ma, b, mb))
    tol = float(d[d.size // 2]) if d.size else 1.0          # a value of the list itself: ties with the tolerance count
    up = [_up(a, dev, np.float64), _up(ma, dev), _up(b, dev, np.float64), _up(mb, dev)]
    for q in qs:
        got = ops.masked_select(up[0], up[1], up[2], up[3], q, tol)
        again = ops.masked_select(up[0], up[1], up[2], up[3], q, tol)
        assert got.dtype == torch.float64 and tuple(got.shape) == (5,)
        got, again, want = got.cpu().numpy(), again.cpu().numpy(), B.order_stats(d, q, tol)
        assert np.array_equal(_bits(got), _bits(again)), (content, n, q)          # two runs, bitwise
        if d.size == 0:
            assert got[0] == 0 and got[1] == 0 and np.isnan(got[2:]).all()
            continue
        assert np.array_equal(_bits(got[[0, 1, 3, 4]]), _bits(want[[0, 1, 3, 4]])), (content, n, q, got, want)
        assert abs(got[2] - want[2]) <= 8 * np.spacing(want[4]), (content, n, q, got, want)


@pytest.mark.gpu
@pytest.mark.parametrize('content', CONTENTS)
def test_masked_select_equals_sort(content):
    for n in LENGTHS:
        _check_selection(content, n, 'cuda:0')


def test_masked_select_host_path(device):
    """the op's own checks and shapes, with the stand-in below it on the CPU"""
    from multimodal_segmentation_amd import ops
    for content in ('uniform', 'zeros', 'none'):
        _check_selection(content, 257, _dev(device))
    a, ma, b, mb, _ = _crafted('uniform', 65)
    dev = _dev(device)
    out = ops.masked_select(_up(a.reshape(5, 13), dev, np.float64), _up(ma.reshape(5, 13), dev), _up(b.reshape(5, 13), dev, np.float64),
                            _up(mb.reshape(5, 13), dev), 50.0, 0.0)          # any one shape; tolerance 0 is allowed
    assert np.array_equal(_bits(out.cpu().numpy()[[0, 1, 3, 4]]), _bits(B.order_stats(_selected(a, ma, b, mb), 50.0, 0.0)[[0, 1, 3, 4]]))
    empty = ops.masked_select(torch.zeros(0, dtype=torch.float64, device=dev), torch.zeros(0, dtype=torch.uint8, device=dev),
                              torch.zeros(0, dtype=torch.float64, device=dev), torch.zeros(0, dtype=torch.uint8, device=dev), 95.0, 1.0)
    empty = empty.cpu().numpy()
    assert empty[0] == 0 and empty[1] == 0 and np.isnan(empty[2:]).all()
    if device == 'cuda':          # the entry point itself with n = 0: it writes N = 0 and the nans
        from multimodal_segmentation_amd import _native
        x, m = torch.ones(1, dtype=torch.float64, device=dev), torch.ones(1, dtype=torch.uint8, device=dev)
        out = torch.full((5,), 7.0, dtype=torch.float64, device=dev)
        ws = torch.empty(_native.call('mmseg_masked_select_workspace_doubles', 0), dtype=torch.float64, device=dev)
        _native.call('mmseg_masked_select', x, m, x, m, 0, 95.0, 1.0, out, ws)
        out = out.cpu().numpy()
        assert out[0] == 0 and out[1] == 0 and np.isnan(out[2:]).all()


# ---- the combined call ------------------------------------------------------------------------------------------------------------------
def _scores_table(pred, truth, values, spacing, dev, percentile=Q, tolerance=TAU):
    from multimodal_segmentation_amd import ops
    v = _up(np.asarray(values), dev, np.int32)
    table = ops.surface_scores(_up(pred, dev), _up(truth, dev), v, spacing, percentile, tolerance)
    assert table.dtype == torch.float64 and tuple(table.shape) == (len(values) + 1, 8)
    return table


@pytest.mark.parametrize('name', COMBINED)
def test_surface_scores_against_yardstick(name, device):
    from multimodal_segmentation_amd import ops
    dev = _dev(device)
    pred, truth, values, spacing = _case_data(name)
    table = _scores_table(pred, truth, values, spacing, dev)
    again = _scores_table(pred, truth, values, spacing, dev)
    got = table.cpu().numpy()
    assert np.array_equal(_bits(got), _bits(again.cpu().numpy()))                     # two runs, bitwise
    want, lists = _yardstick(name)
    d_hi = np.asarray([d[B.ranks(d.size, Q)[1]] for d in lists])
    print('%s: count %s (yardstick %s), HD95 %s mm, difference %s, bar %s' % (name, got[:, 6], want[:, 6], got[:, 7],
                                                                                np.abs(got[:, 7] - want[:, 7]), 2 * REL_DISTANCE * d_hi))
    if device == 'cuda':
        v = _up(np.asarray(values), dev, np.int32)
        six = ops.surface_metrics(_up(pred, dev), _up(truth, dev), v, spacing).cpu().numpy()
        assert np.array_equal(_bits(got[:, :6]), _bits(six))
    assert np.array_equal(got[:, :4], want[:, :4])
    assert np.array_equal(got[:, 6], want[:, 6])
    assert (np.abs(got[:, 7] - want[:, 7]) <= 2 * REL_DISTANCE * d_hi).all()
    full = _scores_table(pred, truth, values, spacing, dev, 100.0, TAU).cpu().numpy()
    assert np.array_equal(_bits(full[:, 7]), _bits(full[:, 5]))                        # HD(100) is MSSD
    assert np.array_equal(_bits(full[:, :7]), _bits(got[:, :7]))


def test_surface_scores_of_an_erased_organ(device):
    pred, truth, values, spacing = _case_data('7x40x36')
    erased = np.where(pred == values[1], 0, pred).astype(np.uint8)
    got = _scores_table(erased, truth, values, spacing, _dev(device)).cpu().numpy()
    assert np.isnan(got[1, 4:]).all() and got[1, 0] == 0 and got[1, 2] == 0 and got[1, 3] > 0
    rest = np.delete(got, 1, axis=0)
    assert np.isfinite(rest).all() and (rest[:, 7] > 0).all()
    want = B.robust_table(erased, truth, values, spacing, Q, TAU)
    assert np.array_equal(rest[:, 6], np.delete(want, 1, axis=0)[:, 6])
    swapped = _scores_table(truth, erased, values, spacing, _dev(device)).cpu().numpy()          # the empty surface on the other side
    assert np.isnan(swapped[1, 4:]).all() and np.isfinite(np.delete(swapped, 1, axis=0)).all()


# ---- refusals and declarations (no GPU) ----------------------------------------------------------------------------------------------------
def test_robust_entry_points_declared_and_bad_arguments_refused():
    from multimodal_segmentation_amd import _native, ops
    protos = _native.parse_header()
    for name in B.STANDINS:
        assert name in protos, name
        assert name.endswith('workspace_doubles') or protos[name][1][-1] == 'void*', name
        assert all(t in _native._CTYPES for t in protos[name][1]), name
    assert callable(ops.masked_select) and callable(ops.surface_scores)
    _native.build()
    lib = _native.load()
    for name in B.STANDINS:
        assert hasattr(lib, name)
    one, bad = 8, 1          # a non-null pointer (a refused call launches nothing and touches no memory); hipErrorInvalidValue
    nan, inf = float('nan'), float('inf')
    query = lib.mmseg_masked_select_workspace_doubles
    assert query(0) > 0 and query(1000) >= 2000 + query(0) and query(2 ** 31 - 1) >= 2 * (2 ** 31 - 1)
    assert query(-1) == 0 and query(2 ** 31) == 0
    n = 36 * 320 * 320
    both = lib.mmseg_surface_scores_workspace_doubles
    assert both(36, 320, 320, 4) >= lib.mmseg_surface_metrics_workspace_doubles(36, 320, 320, 4) + 2 * n
    assert both(36, 320, 320, 17) == 0 and both(36, 320, 320, 0) == 0 and both(2048, 1024, 1024, 4) == 0 and both(2, 0, 8, 4) == 0
    assert both(0, 8, 8, 4) == 0
    select, scores = lib.mmseg_masked_select, lib.mmseg_surface_scores
    for q, tau in ((-1.0, 1.0), (100.5, 1.0), (nan, 1.0), (inf, 1.0), (95.0, -0.1), (95.0, -1.0), (95.0, nan), (95.0, inf)):
        assert select(one, one, one, one, 16, q, tau, one, one, None) == bad, (q, tau)
        assert scores(one, one, one, one, one, 2, 8, 8, 4, 1.0, 1.0, 1.0, q, tau, None) == bad, (q, tau)
    assert select(one, one, one, one, -1, 95.0, 1.0, one, one, None) == bad
    assert select(one, one, one, one, 2 ** 31, 95.0, 1.0, one, one, None) == bad
    for i in (0, 1, 2, 3, 7, 8):          # the six pointers of mmseg_masked_select
        args = [one, one, one, one, 16, 95.0, 1.0, one, one, None]
        args[i] = None
        assert select(*args) == bad, i
    for i in range(5):
        ptrs = [one] * 5
        ptrs[i] = None
        assert scores(*(ptrs + [2, 8, 8, 4, 1.0, 1.0, 1.0, 95.0, 1.0, None])) == bad
    assert scores(one, one, one, one, one, 2, 8, 8, 17, 1.0, 1.0, 1.0, 95.0, 1.0, None) == bad
    assert scores(one, one, one, one, one, 2048, 1024, 1024, 4, 1.0, 1.0, 1.0, 95.0, 1.0, None) == bad
    assert scores(one, one, one, one, one, 2, 8, 8, 4, 1.0, 0.0, 1.0, 95.0, 1.0, None) == bad
    assert scores(one, one, one, one, one, 0, 8, 8, 4, 1.0, 1.0, 1.0, 95.0, 1.0, None) == 0          # S = 0: nothing to do
    u8, i32, f64 = torch.zeros(2, 8, 8, dtype=torch.uint8), torch.zeros(4, dtype=torch.int32), torch.zeros(16, dtype=torch.float64)
    m8 = torch.zeros(16, dtype=torch.uint8)
    for q, tau in ((-1, 1.0), (100.5, 1.0), (nan, 1.0), (inf, 1.0), (95.0, -0.1), (95.0, nan), (95.0, inf)):
        with pytest.raises(ValueError, match='surface_scores'):
            ops.surface_scores(u8, u8, i32, (1.0, 1.0, 1.0), q, tau)
        with pytest.raises(ValueError, match='masked_select'):
            ops.masked_select(f64, m8, f64, m8, q, tau)
    with pytest.raises(ValueError, match='surface_scores'):
        ops.surface_scores(u8, torch.zeros(2, 8, 9, dtype=torch.uint8), i32, (1.0, 1.0, 1.0))
    with pytest.raises(ValueError, match='surface_scores'):
        ops.surface_scores(u8, u8, i32, (1.0, float('nan'), 1.0))
    with pytest.raises(ValueError, match='masked_select'):
        ops.masked_select(f64.float(), m8, f64, m8, 95.0, 1.0)
    with pytest.raises(ValueError, match='masked_select'):
        ops.masked_select(f64, m8, f64, m8[:15], 95.0, 1.0)
    with pytest.raises(ValueError, match='masked_select'):
        ops.masked_select(f64, m8.int(), f64, m8, 95.0, 1.0)


# ---- predictor, tool and CLI ------------------------------------------------------------------------------------------------------------------
@pytest.fixture
def folder(tmp_path):
    out = str(tmp_path / 'volumes')
    R.tool().write_folder(out, volumes=4, size=64, slices=4, seed=3, slice_spacing=(4.0, 9.0))
    return out


def _model(loader, dev, islands=False):
    """the stub's probabilities (the preprocessed truth) rolled by five columns, so that the surfaces differ; optionally with two small
    far-away blobs per organ, in every slice, for the component filter to remove"""
    from tests.test_volume_predict import StubModel
    stub = StubModel(loader, dev, [1, 2, 3, 4])
    K = loader.num_masks

    class Rolled(object):
        modalities = stub.modalities

        def predict_mask(self, modality_index, mode, image_list):
            p = torch.roll(stub.predict_mask(modality_index, mode, image_list), 5, dims=2).clone()
            if islands:
                for k in range(K):
                    for r0 in (9, 53):
                        p[:, r0:r0 + 2, 9 + 12 * k:11 + 12 * k, :] = 0.0
                        p[:, r0:r0 + 2, 9 + 12 * k:11 + 12 * k, k] = 1.0
            return p
    return Rolled()


def _expected_rows(folder, out, manifest, mod, percentile, tolerance):
    """per volume the yardstick's HD, NSD (the union first) of the written .npz against the file's label, as the CSV prints them"""
    rows = {}
    for v in ('1', '2', '3', '4'):
        entry = manifest['volumes'][v][mod]
        with np.load(os.path.join(folder, entry['file'])) as z:
            truth, res, dz = z['label'].copy(), z['resolution'], float(z['slice_spacing'])
        with np.load(os.path.join(out, entry['file'])) as z:
            pred = z['label']
        a, b = entry.get('slices', [[0, truth.shape[0]]])[0]
        truth[:a], truth[b:] = 0, 0
        want = B.robust_scores(pred, truth, VALUES, (dz, res[0], res[1]), percentile, tolerance)
        rows[v] = ['%.3f' % x for x in np.concatenate([want[-1:], want[:-1]], axis=0).reshape(-1)]
    return rows


def test_predictor_writes_robust_scores(folder, tmp_path, device):
    from multimodal_segmentation_amd.loaders.volume_folder import VolumeFolderLoader
    from multimodal_segmentation_amd.volume_predictor import VolumePredictor
    from tests.test_volume_predict import _stub_conf
    K = len(VALUES)
    loader = VolumeFolderLoader(folder)
    manifest = loader.manifest
    model = _model(loader, _dev(device))
    plain, omitted, both, alone = (str(tmp_path / name) for name in ('plain', 'omitted', 'both', 'alone'))
    VolumePredictor(model, _stub_conf(3)).run(folder, plain, robust=None)
    VolumePredictor(model, _stub_conf(3)).run(folder, omitted)
    VolumePredictor(model, _stub_conf(3)).run(folder, both, robust=(Q, TAU))
    VolumePredictor(model, _stub_conf(3)).run(folder, alone, surface=False, robust=(Q, TAU))
    volumes = [e[mod]['file'] for e in manifest['volumes'].values() for mod in ('t1', 't2')]
    today = sorted(['predictions.json'] + ['results_%s_%s.csv' % (a, b) for a in ('native', 'surface') for b in ('t1', 't2')] + volumes)
    robust_files = ['results_robust_t1.csv', 'results_robust_t2.csv']
    # robust=None: the folder of today, and no new key
    assert sorted(os.listdir(plain)) == sorted(os.listdir(omitted)) == today
    settings = [json.load(open(os.path.join(d, 'predictions.json'))) for d in (plain, omitted, both, alone)]
    assert sorted(settings[0]) == ['files', 'label_values', 'mode', 'model_folder', 'order', 'source_folder'] and settings[0] == settings[1]
    for name in today:
        if name.endswith('.csv'):
            assert open(os.path.join(plain, name), 'rb').read() == open(os.path.join(omitted, name), 'rb').read(), name
    # robust on: one more file per modality, everything else as before; with surface=False only the new file
    assert sorted(os.listdir(both)) == sorted(today + robust_files)
    assert sorted(os.listdir(alone)) == sorted(['predictions.json', 'results_native_t1.csv', 'results_native_t2.csv'] + robust_files + volumes)
    for s in settings[2:]:
        assert sorted(s) == sorted(list(settings[0]) + ['percentile', 'tolerance_mm']) and s['percentile'] == Q and s['tolerance_mm'] == TAU
        assert s['files'] == settings[0]['files']
    for name in today:
        if name.endswith('.csv'):          # one ops.surface_scores call serves both files: the surface file does not change
            assert open(os.path.join(both, name), 'rb').read() == open(os.path.join(plain, name), 'rb').read(), name
    header = 'Vol, HD, NSD, ' + ', '.join('%s%d' % (n, k) for k in range(K) for n in ('HD', 'NSD'))
    for mod in ('t1', 't2'):
        head, rows = _csv_rows(os.path.join(both, 'results_robust_%s.csv' % mod))
        assert head == header and list(rows) == ['1', '2', '3', '4'] and all(len(r) == 2 * (K + 1) for r in rows.values())
        want = _expected_rows(folder, both, manifest, mod, Q, TAU)
        print('%s: csv %s\nyardstick %s' % (mod, rows, want))
        assert rows == want
        assert all(float(r[0]) > 0.0 and 0.0 < float(r[1]) < 1.0 for r in rows.values())          # the roll is seen
        assert open(os.path.join(alone, 'results_robust_%s.csv' % mod), 'rb').read() == open(os.path.join(both, 'results_robust_%s.csv' % mod), 'rb').read()
    # the tool scores the written folder again, without a model: the same files, byte for byte
    again, again_alone = str(tmp_path / 'again'), str(tmp_path / 'again_alone')
    _score_tool().main([both, folder, '--out', again, '--predict_robust', 'true', '--predict_percentile', '%r' % Q, '--predict_tolerance', '%r' % TAU])
    assert sorted(os.listdir(again)) == sorted(['results_%s_%s.csv' % (a, b) for a in ('native', 'surface', 'robust') for b in ('t1', 't2')])
    for name in sorted(os.listdir(again)):
        assert open(os.path.join(again, name), 'rb').read() == open(os.path.join(both, name), 'rb').read(), name
    _score_tool().main([both, folder, '--out', again_alone, '--surface', 'false', '--predict_robust', 'true', '--predict_tolerance', '%r' % TAU])
    assert sorted(os.listdir(again_alone)) == sorted(['results_native_t1.csv', 'results_native_t2.csv'] + robust_files)
    for name in robust_files:
        assert open(os.path.join(again_alone, name), 'rb').read() == open(os.path.join(both, name), 'rb').read(), name
    # another percentile and tolerance change the file
    other = str(tmp_path / 'other')
    _score_tool().main([both, folder, '--out', other, '--predict_robust', 'true', '--predict_percentile', '50', '--predict_tolerance', '0.5'])
    assert _csv_rows(os.path.join(other, 'results_robust_t1.csv'))[1] == _expected_rows(folder, both, manifest, 't1', 50.0, 0.5)
    for bad in ((101, 1.0), (-1, 1.0), (95, -0.1), (float('nan'), 1.0), (95, float('inf')), (95,), 95):
        with pytest.raises(ValueError, match='robust'):
            VolumePredictor(model, _stub_conf(3)).run(folder, str(tmp_path / 'no'), robust=bad)
    assert not os.path.exists(str(tmp_path / 'no'))


def test_predictor_robust_skips_files_without_spacing_or_label(tmp_path, device, caplog):
    import logging
    from multimodal_segmentation_amd.loaders.volume_folder import VolumeFolderLoader
    from multimodal_segmentation_amd.volume_predictor import VolumePredictor
    from tests.test_volume_predict import _stub_conf
    plain = str(tmp_path / 'plain')
    R.tool().write_folder(plain, volumes=4, size=64, slices=4, seed=3)          # no slice_spacing
    out = str(tmp_path / 'out')
    with caplog.at_level(logging.INFO, logger='volume_predictor'):
        VolumePredictor(_model(VolumeFolderLoader(plain), _dev(device)), _stub_conf(3)).run(plain, out, surface=False, robust=(Q, TAU))
    assert not [f for f in os.listdir(out) if f.startswith('results_robust') or f.startswith('results_surface')]
    assert 'results_native_t1.csv' in os.listdir(out)
    lines = [r.getMessage() for r in caplog.records if 'slice_spacing' in r.getMessage()]
    assert len(lines) == 8 and len(set(lines)) == 8          # one line per skipped file


def test_robust_scores_the_filtered_volume(folder, tmp_path, device):
    """--predict_components largest with --predict_robust true: the component filter runs first, and what is scored is what is written"""
    from multimodal_segmentation_amd.experiment import parse_arguments, robust_of
    from multimodal_segmentation_amd.loaders.volume_folder import VolumeFolderLoader
    from multimodal_segmentation_amd.volume_predictor import VolumePredictor
    from tests.test_volume_predict import _stub_conf
    args = parse_arguments(['--config', 'dafnet_config_chaos', '--split', '0', '--predict_components', 'largest', '--predict_robust', 'true',
                            '--predict_tolerance', '%r' % TAU])
    components = {'largest': 'largest'}.get(args.predict_components)
    assert components == 'largest' and robust_of(args) == (Q, TAU)
    loader = VolumeFolderLoader(folder)
    model = _model(loader, _dev(device), islands=True)
    kept, unfiltered = str(tmp_path / 'kept'), str(tmp_path / 'unfiltered')
    VolumePredictor(model, _stub_conf(3)).run(folder, kept, components=components, connectivity=args.predict_connectivity, robust=robust_of(args))
    VolumePredictor(model, _stub_conf(3)).run(folder, unfiltered, robust=robust_of(args))
    differ = 0
    for mod in ('t1', 't2'):
        rows = _csv_rows(os.path.join(kept, 'results_robust_%s.csv' % mod))[1]
        assert rows == _expected_rows(folder, kept, loader.manifest, mod, Q, TAU)
        differ += int(rows != _csv_rows(os.path.join(unfiltered, 'results_robust_%s.csv' % mod))[1])
    assert differ == 2          # the blobs moved the scores of the unfiltered run
    settings = json.load(open(os.path.join(kept, 'predictions.json')))
    assert settings['components'] == 'largest' and settings['percentile'] == Q and settings['tolerance_mm'] == TAU
    # the tool, on the unfiltered volumes, with the filter: the same file
    again = str(tmp_path / 'again')
    _score_tool().main([unfiltered, folder, '--out', again, '--components', 'largest', '--predict_robust', 'true', '--predict_tolerance', '%r' % TAU])
    for mod in ('t1', 't2'):
        name = 'results_robust_%s.csv' % mod
        assert open(os.path.join(again, name), 'rb').read() == open(os.path.join(kept, name), 'rb').read()


def test_robust_cli_options(monkeypatch, capsys):
    from multimodal_segmentation_amd import experiment
    base = ['--config', 'dafnet_config_chaos', '--split', '0']
    a = experiment.parse_arguments(base)
    assert a.predict_robust is False and a.predict_percentile == 95.0 and a.predict_tolerance == 1.0 and experiment.robust_of(a) is None
    a = experiment.parse_arguments(base + ['--predict_robust', 'true', '--predict_percentile', '90', '--predict_tolerance', '2.5'])
    assert a.predict_robust is True and experiment.robust_of(a) == (90.0, 2.5)
    assert experiment.robust_of(experiment.parse_arguments(base + ['--predict_percentile', '90'])) is None

    def no_model(*args, **kwargs):
        raise AssertionError('the run went on past the options')
    monkeypatch.setattr(experiment.Experiment, 'get_config', no_model)
    monkeypatch.setattr(experiment.Experiment, 'get_executor', no_model)
    tool = _score_tool()
    for option, value in (('--predict_percentile', '101'), ('--predict_percentile', '-1'), ('--predict_percentile', 'nan'),
                          ('--predict_tolerance', '-0.1'), ('--predict_tolerance', 'inf'), ('--predict_robust', 'perhaps'),
                          ('--predict_percentile', 'many')):
        capsys.readouterr()
        with pytest.raises(SystemExit):
            experiment.Experiment().run(base + ['--predict_robust', 'true', option, value])
        assert option in capsys.readouterr().err          # the message names the option
        with pytest.raises(SystemExit):
            tool.main(['a', 'b', option, value])
        assert option in capsys.readouterr().err


def test_robust_bench_tool_is_importable():
    """tools/volume_robust_bench.py refuses to time anything without a GPU, and says so"""
    spec = importlib.util.spec_from_file_location('volume_robust_bench', os.path.join(R.ROOT, 'tools', 'volume_robust_bench.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    assert callable(mod.main) and mod.SHAPES
    if not torch.cuda.is_available():
        with pytest.raises(SystemExit, match='GPU'):
            mod.main([])
