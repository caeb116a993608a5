"""Bias-field correction of volumes read from a folder: csrc/biasfield.hip (mmseg_bias_*), ops.bias_correct and its stages, the `bias_field`
block of loaders/volume_folder.py, tools/make_volume_folder.py --bias_field and the `--bias_*` options of experiment.py, against the
numpy restatement in tests/volume_bias_ref.py (the rule is in include/mmseg_hip.h; the bars are derived in the restatement's docstring).
Every measured figure is printed before it is asserted (pytest -s shows them; profiles/volume_bias_bench.md records them)."""
import json
import logging
import os

import numpy as np
import pytest
import torch

from multimodal_segmentation_amd import loaders, nn, ops
from multimodal_segmentation_amd.loaders import loader_factory
from tests import volume_bias_ref as B
from tests import volume_intensity_ref as I
from tests import volume_loader_ref as R

gpu = pytest.mark.gpu
DEV = 'cuda:0'
SPACINGS = (6.0, 1.6, 1.6)
SHORT = dict(levels=2, iterations=3)

# End to end, the fp32 output against the restatement in fp32 spacings.  Measured on the MI355X: 0 spacings in all three cases
# (profiles/volume_bias_bench.md), as the fp64 experiment of the issue predicts; the bar is that plus one spacing.
E2E_BAR = 1.0


@pytest.fixture(autouse=True)
def _clean_registries():
    saved = dict(loaders.data_conf), dict(loaders.intensity_conf), dict(loaders.bias_conf)
    yield
    for registry, old in zip((loaders.data_conf, loaders.intensity_conf, loaders.bias_conf), saved):
        registry.clear()
        registry.update(old)


def _install(monkeypatch):
    from tests import cpu_backend as cb
    for table in (R.STANDINS, I.STANDINS, B.STANDINS):
        for name, fn in table.items():
            monkeypatch.setitem(cb._TABLE, name, fn)
    monkeypatch.setattr(B, 'CALLS', [])
    cb.install()
    nn.set_default_device('cpu')
    return cb


@pytest.fixture
def standin(monkeypatch):
    """the CPU stand-in of the C ABI with the stand-ins of the preprocessing and bias entry points added to its table"""
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
        nn.set_default_device(DEV)
        yield 'cuda'


FOLDER_BLOCK = {'mode': 'n3', 'levels': 2, 'iterations': 4}


@pytest.fixture
def folder(tmp_path):
    """a shaded example folder: +-0.35 in the logarithm, slice spacings in the files, so the default extent is 3d"""
    out = str(tmp_path / 'volumes')
    R.tool().write_folder(out, volumes=4, size=64, slices=4, seed=3, slice_spacing=(5.0, 8.0), bias_field=0.35)
    _set_block(out, FOLDER_BLOCK)
    return out


def _set_block(folder, block, key='bias_field'):
    path = os.path.join(folder, 'dataset.json')
    manifest = json.load(open(path))
    if block is None:
        manifest.pop(key, None)
    else:
        manifest[key] = block
    json.dump(manifest, open(path, 'w'))


def _dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a))
    return (t if dtype is None else t.to(dtype)).to(DEV)


# ---- 1. the stages ------------------------------------------------------------------------------------------------------------------------
def _otsu_volume(name):
    rng = np.random.RandomState(11)
    if name == '3x20x24':
        return B.phantom((3, 20, 24), seed=2)[0]
    if name == '1x7x5':
        return rng.uniform(-3.0, 40.0, (1, 7, 5)).astype(np.float32)
    if name == 'two-valued':
        return np.where(rng.rand(2, 9, 11) < 0.3, 7.5, 120.25).astype(np.float32)
    return np.full((2, 6, 7), 3.25, np.float32)


@gpu
@pytest.mark.parametrize('name', ['3x20x24', '1x7x5', 'two-valued', 'constant'])
def test_otsu_threshold_equals_the_restatement(name):
    x = _otsu_volume(name)
    lo, hi, thr, constant = B.otsu(x)
    got = ops.bias_otsu(_dev(x)).cpu().numpy()
    print('otsu %s: lo %r hi %r threshold %r (device %r)' % (name, lo, hi, thr, got[2]))
    assert got[0] == lo and got[1] == hi and got[2] == thr and bool(got[3]) == constant


def _histogram_input(seed):
    rng = np.random.RandomState(seed)
    v = np.log(rng.uniform(40.0, 900.0, 5000)) + 0.1 * rng.standard_normal(5000)
    m = rng.rand(5000) < 0.7
    return v, m


@gpu
@pytest.mark.parametrize('seed', [0, 1, 2])
def test_histogram_counts_equal_the_restatement(seed):
    v, m = _histogram_input(seed)
    want, vmin, vmax, c, margin = B.histogram(v, m)
    assert margin > B.MARGIN, 'seed %d puts a value within %g of a bin edge: choose another' % (seed, margin)
    hist, rng = ops.bias_histogram(_dev(v), _dev(m.astype(np.uint8)))
    assert np.array_equal(rng.cpu().numpy(), [vmin, vmax])
    assert np.array_equal(hist.cpu().numpy(), want) and int(hist.sum()) == int(m.sum())


def _sharpen_input(name):
    if name == 'one-bin':
        h = np.zeros(B.BINS, np.int64)
        h[77] = 5000
        return h, 1.0, 3.0
    rng = np.random.RandomState(5)
    v = np.concatenate([5.5 + 0.08 * rng.standard_normal(6000), 6.6 + 0.12 * rng.standard_normal(9000)])
    h, vmin, vmax, _, _ = B.histogram(v, np.ones(v.shape, bool))
    return h, vmin, vmax


@gpu
@pytest.mark.parametrize('name', ['bimodal', 'one-bin'])
def test_sharpen_table_within_the_derived_bar(name):
    """E against numpy.fft, entry by entry within sharpen_bar (Higham section 24.1 through the five transforms and the quotient)"""
    h, vmin, vmax = _sharpen_input(name)
    want = B.sharpen(h, vmin, vmax)
    bar, e_nd = B.sharpen_bar(h, vmin, vmax)
    got = ops.bias_sharpen(_dev(h.astype(np.int32)), _dev(np.array([vmin, vmax]))).cpu().numpy()
    err = np.abs(got - want)
    stated = np.isfinite(bar)
    print('sharpen %s: largest relative error %.3e, largest error / bar %.3e, the bar speaks about %d of %d entries, e_nd %.3e'
          % (name, (err / np.abs(want))[stated].max(), (err / bar)[stated].max(), stated.sum(), B.BINS, e_nd))
    assert stated.sum() >= 150          # the bound must say something about most of the table
    assert np.all(np.isfinite(got)) and np.all(err[stated] <= bar[stated])


SMOOTH_CASES = {
    'R>S': ((4, 33, 29), (6.75, 2.25, 2.25)),                  # R = (27, 9, 9): the slice radius exceeds the 4 slices
    'W=130': ((2, 9, 130), (0.6, 0.8, 1.3)),                   # one column past a tile of 128; R = (2, 3, 5)
    'R=128': ((5, 140, 12), (32.0, 32.0, 32.0)),               # the largest radius on every axis
    '2d': ((3, 20, 17), (None, 2.0, 1.5)),                     # no pass along S
    'S=1': ((1, 21, 19), (0.6, 0.6, 0.6)),
    'H=33': ((2, 33, 37), (None, 5.0, 0.7)),                   # one line past a tile of 32
}


def _level(sig):
    return [(0.0, 0) if s is None else (float(s), B.radius(s)) for s in sig]


@gpu
@pytest.mark.parametrize('name', sorted(SMOOTH_CASES))
def test_masked_gaussian_within_a_few_ulps_of_the_tap_sum(name):
    shape, sig = SMOOTH_CASES[name]
    assert name != 'R>S' or tuple(B.radius(s) for s in sig) == (27, 9, 9)
    assert name != 'R=128' or tuple(B.radius(s) for s in sig) == (128, 128, 128)
    rng = np.random.RandomState(len(name))
    y = rng.standard_normal(shape) * (rng.rand(*shape) < 0.6)
    want, bar = B.smooth(y, sig), B.smooth_bar(y, sig)
    got = ops.bias_smooth(_dev(y), _level(sig)).cpu().numpy()
    again = ops.bias_smooth(_dev(y), _level(sig)).cpu().numpy()
    err = np.abs(got - want)
    print('smooth %s: largest error %.3e, largest error / bar %.3e' % (name, err.max(), (err / np.maximum(bar, 1e-300)).max()))
    assert np.all(err <= bar) and np.array_equal(got, again)


@gpu
def test_update_keeps_the_field_where_the_denominator_is_zero():
    """a mask with a region farther than R from any masked voxel: den = 0 there exactly, and f stays as it was, bit for bit"""
    shape, sig = (2, 40, 50), (0.3, 0.8, 0.8)                  # R = (1, 3, 3)
    rng = np.random.RandomState(4)
    m = np.zeros(shape, bool)
    m[:, :12, :15] = rng.rand(2, 12, 15) < 0.8
    r = rng.standard_normal(shape) * m
    f0 = rng.standard_normal(shape)
    den, num = B.smooth(m.astype(np.float64), sig), B.smooth(r, sig)
    far = den == 0
    assert far.sum() > 1000 and (~far).sum() > 300
    f = _dev(f0.copy())
    d_den, d_num = ops.bias_smooth(_dev(m.astype(np.float64)), _level(sig)), ops.bias_smooth(_dev(r), _level(sig))
    ops.bias_update(f, d_num, d_den)
    got = f.cpu().numpy()
    assert np.array_equal(d_den.cpu().numpy() == 0, far) and np.array_equal(got[far], f0[far])
    q = num[~far] / den[~far]
    bar = (B.smooth_bar(r, sig)[~far] + np.abs(q) * B.smooth_bar(m.astype(np.float64), sig)[~far]) / den[~far] + 4 * B.U64 * (np.abs(q) + np.abs(f0[~far]))
    assert np.all(np.abs(got[~far] - (f0[~far] + q)) <= bar)


# ---- 2. end to end against the restatement ------------------------------------------------------------------------------------------------
E2E_CASES = {
    'phantom-3d': dict(shape=(6, 64, 56), spacings=SPACINGS, seed=0, params=dict(SHORT, extent='3d')),
    'phantom-2d': dict(shape=(6, 64, 56), spacings=SPACINGS, seed=0, params=dict(SHORT, extent='2d')),
    'odd-aniso': dict(shape=(5, 37, 41), spacings=(7.5, 1.4, 1.9), seed=3, params=dict(SHORT, extent='3d')),
}
_e2e_cache = {}


def _e2e(name):
    """the case's input and the restatement's result, computed once and shared"""
    if name not in _e2e_cache:
        case = E2E_CASES[name]
        x, field, tissue = B.phantom(case['shape'], case['spacings'], seed=case['seed'])
        _e2e_cache[name] = (x, field, tissue, B.correct(x, case['spacings'], case['params']))
    return _e2e_cache[name]


@pytest.mark.parametrize('name', sorted(E2E_CASES))
def test_restatement_keeps_its_distance_from_the_bin_edges(name):
    """the precondition of the end-to-end comparison, asserted on the reference side over all iterations"""
    res = _e2e(name)[3]
    print('%s: smallest distance to a bin edge %.3e over %d iterations' % (name, res['margin'], res['updates']))
    assert res['updates'] == 6 and not res['frozen'] and res['margin'] > B.MARGIN


@gpu
@pytest.mark.parametrize('name', sorted(E2E_CASES))
def test_correction_equals_the_restatement(name):
    case = E2E_CASES[name]
    x, _, _, res = _e2e(name)
    assert res['margin'] > B.MARGIN
    xd = _dev(x)
    out, f, info = ops.bias_correct(xd, case['spacings'], case['params'], field=True)
    again = ops.bias_correct(xd, case['spacings'], case['params'])
    got = out.cpu().numpy()
    apart = B.spacings_apart(got, res['out'])
    m = res['mask']
    print('%s: output %.2f fp32 spacings from the restatement; log-field within %.3e of it on the mask; info %s'
          % (name, apart, np.abs(f.cpu().numpy() - res['field'])[m].max(), info.cpu().tolist()))
    assert info.cpu().tolist() == [0, 6]
    assert torch.equal(out, again)                                   # two device runs, bit for bit
    assert np.array_equal(xd.cpu().numpy(), x)                       # the input is left alone
    assert apart <= E2E_BAR
    assert not np.array_equal(got, x)


@gpu
@pytest.mark.parametrize('name', ['constant', 'empty-mask', 'one-masked-value'])
def test_volumes_the_rule_leaves_alone_keep_their_bits(name):
    rng = np.random.RandomState(8)
    if name == 'constant':
        x = np.full((3, 10, 12), 41.5, np.float32)
    elif name == 'empty-mask':
        x = -rng.uniform(0.0, 5.0, (3, 10, 12)).astype(np.float32)          # nothing above max(threshold, 0)
    else:
        x = np.where(rng.rand(3, 10, 12) < 0.4, 0.0, 250.0).astype(np.float32)
    res = B.correct(x, SPACINGS, SHORT)
    assert res['updates'] == 0 and np.array_equal(res['out'].view(np.uint32), x.view(np.uint32))
    out, f, info = ops.bias_correct(_dev(x), SPACINGS, SHORT, field=True)
    assert np.array_equal(out.cpu().numpy().view(np.uint32), x.view(np.uint32))
    assert info.cpu().tolist() == [1, 0] and not f.cpu().numpy().any()


def test_host_logic_on_the_standin(standin):
    """ops.bias_correct drives the stand-ins level by level to the restatement's result: radii, weight rows, order of the calls"""
    x, _, _, res = _e2e('odd-aniso')
    case = E2E_CASES['odd-aniso']
    out, f, info = ops.bias_correct(torch.from_numpy(x), case['spacings'], case['params'], field=True)
    assert B.CALLS == [(5, 37, 41)] and info.tolist() == [0, 6]
    assert B.spacings_apart(out.numpy(), res['out']) <= 1.0 and np.abs(f.numpy() - res['field']).max() < 1e-9
    levels = ops.bias_sigmas(case['spacings'], ops.bias_params(case['params']))
    assert [[R_ for _, R_ in lv] for lv in levels] == [[B.radius(s) for s in sig] for sig in B.level_sigmas(case['spacings'], 40.0, 2, '3d')]
    rows = ops.bias_weight_rows(levels[1])
    for a in range(3):
        R_ = levels[1][a][1]
        assert abs(rows[a, 0] + 2 * rows[a, 1:R_ + 1].sum() - 1.0) < 1e-14 and not rows[a, R_ + 1:].any()


# ---- 3. it corrects ---------------------------------------------------------------------------------------------------------------------------
def _corrects(x, field, tissue, out, f, mask, where):
    before, after = B.tissue_cv(x, tissue), B.tissue_cv(out, tissue)
    corr = float(np.corrcoef(f[mask], field[mask])[0, 1])
    print('%s: coefficient of variation per tissue %s -> %s; correlation of the log-field with the true one %.4f'
          % (where, ['%.4f' % v for v in before], ['%.4f' % v for v in after], corr))
    assert all(a < b for a, b in zip(after, before)) and corr > 0


def test_restatement_corrects_the_phantom_at_the_defaults():
    x, field, tissue = B.phantom()
    res = B.correct(x, SPACINGS)
    _corrects(x, field, tissue, res['out'], res['field'], res['mask'], 'restatement')


@gpu
def test_device_corrects_the_phantom_at_the_defaults():
    x, field, tissue = B.phantom()
    out, f, info = ops.bias_correct(_dev(x), SPACINGS, field=True)
    assert info.cpu().tolist() == [0, 60]
    _corrects(x, field, tissue, out.cpu().numpy(), f.cpu().numpy(), B.otsu(x)[2] < x.astype(np.float64), 'MI355X')


# ---- 4. loader and command line -----------------------------------------------------------------------------------------------------------
def test_manifest_validation_messages(folder):
    from multimodal_segmentation_amd.loaders.volume_folder import check_bias, read_manifest
    assert check_bias(None, 'x') == {'mode': 'off'} == check_bias({}, 'x') == check_bias({'mode': 'off'}, 'x')
    assert check_bias({'mode': 'n3'}, 'x') == dict(mode='n3', sigma_mm=40.0, levels=3, iterations=20, extent=None)
    assert check_bias({'mode': 'n3', 'extent': '2d', 'sigma_mm': 25}, 'x')['extent'] == '2d'
    for block, text in (([1], 'must be an object'), ({'mode': 'n4'}, 'mode must be one of off, n3'), ({'mode': 'n3', 'bins': 5}, 'unknown key(s) bins'),
                        ({'mode': 'off', 'levels': 2}, 'mode off takes no other key'), ({'mode': 'n3', 'sigma_mm': 0}, 'sigma_mm must be'),
                        ({'mode': 'n3', 'sigma_mm': 'wide'}, 'sigma_mm must be'), ({'mode': 'n3', 'levels': 0}, 'levels must be a whole number in 1..8'),
                        ({'mode': 'n3', 'levels': 2.5}, 'levels must be'), ({'mode': 'n3', 'iterations': 1001}, 'iterations must be a whole number in 1..1000'),
                        ({'mode': 'n3', 'extent': '4d'}, 'extent must be one of 2d, 3d')):
        _set_block(folder, block)
        with pytest.raises(ValueError) as e:
            read_manifest(folder)
        assert text in str(e.value) and 'dataset.json' in str(e.value) and 'bias_field' in str(e.value), (block, str(e.value))


def test_bias_conf_overrides_the_folder(standin, folder):
    loaders.data_conf['chaos'] = folder
    assert loader_factory.init_loader('chaos').bias_field == dict(mode='n3', sigma_mm=40.0, levels=2, iterations=4, extent=None)
    loaders.bias_conf['chaos'] = {'mode': 'off'}
    loader = loader_factory.init_loader('chaos')
    assert loader.bias_field == {'mode': 'off'}
    loader.load_volume_for_prediction(1)
    assert B.CALLS == []                                             # the registry changes what is computed, not only what is reported
    loaders.bias_conf['chaos'] = {'mode': 'n3', 'levels': 1, 'iterations': 1, 'extent': '2d'}
    loader_factory.init_loader('chaos').load_volume_for_prediction(1)
    assert len(B.CALLS) == 2
    loaders.bias_conf['chaos'] = {'mode': 'n3', 'levels': 99}
    with pytest.raises(ValueError) as e:
        loader_factory.init_loader('chaos')
    assert "loaders.bias_conf['chaos']" in str(e.value)


def _strip_spacing(folder, name):
    path = os.path.join(folder, name)
    with np.load(path) as z:
        arrays = {k: z[k] for k in z.files if k != 'slice_spacing'}
    np.savez_compressed(path, **arrays)


def test_3d_needs_a_slice_spacing_and_one_run_of_slices(standin, folder):
    from multimodal_segmentation_amd.loaders.volume_folder import VolumeFolderLoader
    _set_block(folder, dict(FOLDER_BLOCK, extent='3d'))
    _strip_spacing(folder, 'vol01_t2.npz')
    loader = VolumeFolderLoader(folder)
    for load in (lambda: loader.load_volume_for_prediction(1), lambda: loader.upload_volume(1),
                 lambda: loader.load_all_modalities_concatenated(0, 'training', 1)):
        with pytest.raises(ValueError) as e:
            load()
        assert 'extent 3d needs a slice_spacing' in str(e.value) and 'volume 1, modality t2' in str(e.value)
    _set_block(folder, FOLDER_BLOCK)                                 # no extent named: that file alone falls back to 2d
    loader = VolumeFolderLoader(folder)
    loader.load_volume_for_prediction(1)
    assert loader.bias_extent(None, None, 'x') == '2d' and loader.bias_extent(6.0, np.arange(3), 'x') == '3d'
    manifest = json.load(open(os.path.join(folder, 'dataset.json')))
    first = manifest['volumes']['2']['t2'].get('slices', [[0, 4]])[0][0]
    manifest['volumes']['2']['t1']['slices'] = [[0, 2], [3, 4]]          # three slices with a gap (the file holds four)
    manifest['volumes']['2']['t2']['slices'] = [[first, first + 3]]      # three in one run
    json.dump(manifest, open(os.path.join(folder, 'dataset.json'), 'w'))
    with pytest.raises(ValueError) as e:
        VolumeFolderLoader(folder).load_volume_for_prediction(2)
    assert 'one contiguous run of slices' in str(e.value) and 'volume 2, modality t1' in str(e.value)
    _set_block(folder, dict(FOLDER_BLOCK, extent='2d'))
    VolumeFolderLoader(folder).load_volume_for_prediction(2)         # 2d takes any selection


def test_radius_refusal_names_axis_spacing_and_the_sigma_that_fits(standin):
    x = torch.zeros(3, 8, 8)
    with pytest.raises(ValueError) as e:
        ops.bias_correct(x, (6.0, 0.25, 1.5), dict(sigma_mm=40.0))
    text = str(e.value)
    assert 'row spacing of 0.25 mm' in text and 'radius of 640 voxels' in text and 'sigma_mm <= 8 fits' in text
    assert ops.bias_sigmas((6.0, 0.25, 1.5), ops.bias_params(dict(sigma_mm=8.0, levels=1)))[0][1] == (32.0, 128)
    with pytest.raises(ValueError) as e:
        ops.bias_correct(x, (6.0, 1.5, 1.5), dict(sigma_mm=2.0, levels=3))
    assert 'slice spacing of 6 mm' in str(e.value) and 'radius of 0 voxels at level 2' in str(e.value) and 'sigma_mm >= 3 fits' in str(e.value)
    ops.bias_correct(x, (6.0, 1.5, 1.5), dict(sigma_mm=2.0, levels=3, extent='2d'))          # the slice axis is not smoothed
    with pytest.raises(ValueError):
        ops.bias_correct(x, (6.0, 1.5), None)
    with pytest.raises(ValueError):
        ops.bias_correct(x, SPACINGS, dict(bins=100))
    from multimodal_segmentation_amd import _native
    _native.build()
    lib, one = _native.load(), 1          # `one` stands for a non-null pointer: a refused call launches nothing and touches no memory
    assert lib.mmseg_bias_workspace_doubles(30, 256, 256) == 512 + 6 * 30 * 256 * 256 + 30 * 256 * 256 // 8
    assert lib.mmseg_bias_workspace_doubles(0, 8, 8) == 0 and lib.mmseg_bias_workspace_doubles(65535, 65535, 2) == 0
    for radii in ((129, 9, 9), (1, 129, 9), (1, 9, 129), (1, 0, 9), (1, 9, 0), (-1, 9, 9)):
        assert lib.mmseg_bias_level(one, one, one, 4, 33, 29, *(radii + (1, None))) != 0
        assert lib.mmseg_bias_smooth(one, one, one, one, 4, 33, 29, *(radii + (None,))) != 0
    assert lib.mmseg_bias_level(one, one, one, 4, 33, 29, 27, 9, 9, 0, None) != 0
    assert lib.mmseg_bias_level(None, one, one, 4, 33, 29, 27, 9, 9, 1, None) != 0
    assert lib.mmseg_bias_begin(None, one, 4, 33, 29, None) != 0 and lib.mmseg_bias_finish(one, None, 4, 33, 29, None) != 0


def test_cli_override_reaches_the_loader_and_the_recorded_configuration(folder, tmp_path, monkeypatch):
    from multimodal_segmentation_amd.experiment import Experiment, parse_arguments
    monkeypatch.chdir(tmp_path)
    base = ['--config', 'dafnet_config_chaos', '--split', '0', '--data_folder', folder]
    own = dict(mode='n3', sigma_mm=40.0, levels=2, iterations=4, extent=None)
    conf = Experiment().get_config(0, parse_arguments(base))
    assert loaders.bias_conf == {} and conf.bias_field == own          # no override: the folder's own block
    conf = Experiment().get_config(0, parse_arguments(base + ['--bias_correction', 'n3', '--bias_sigma_mm', '30', '--bias_levels', '2',
                                                               '--bias_iterations', '5', '--bias_extent', '2d']))
    want = dict(mode='n3', sigma_mm=30.0, levels=2, iterations=5, extent='2d')
    assert loaders.bias_conf == {'chaos': want} and conf.bias_field == want
    assert loader_factory.init_loader('chaos').bias_field == want
    dumped = json.load(open(os.path.join(conf.folder, 'experiment_configuration.json')))
    assert dumped['bias_field'] == want and dumped['data_folder'] == folder
    conf = Experiment().get_config(0, parse_arguments(base + ['--bias_correction', 'off']))
    assert conf.bias_field == {'mode': 'off'} == loader_factory.init_loader('chaos').bias_field
    conf = Experiment().get_config(0, parse_arguments(base))          # a later run without the options follows dataset.json again
    assert loaders.bias_conf == {} and loader_factory.init_loader('chaos').bias_field == own
    for bad in (['--bias_levels', '2'], ['--bias_correction', 'off', '--bias_sigma_mm', '30'], ['--bias_correction', 'n4']):
        with pytest.raises(SystemExit):
            parse_arguments(base + bad)
    with pytest.raises(ValueError):
        Experiment().get_config(0, parse_arguments(base + ['--bias_correction', 'n3', '--bias_levels', '0']))


def test_predict_folder_with_another_setting_logs_a_warning(folder, tmp_path, caplog):
    from multimodal_segmentation_amd.utils.config import EasyDict
    from multimodal_segmentation_amd.experiment import warn_predict_stages
    other = str(tmp_path / 'scans')
    R.tool().write_folder(other, volumes=3, size=64, slices=2, seed=5, name='site_b', unlabelled=True)
    plain = str(tmp_path / 'plain')
    R.tool().write_folder(plain, volumes=3, size=32, slices=2, seed=1)
    log = logging.getLogger('test_volume_bias')
    conf = EasyDict(folder='run', bias_field=dict(mode='n3', sigma_mm=40.0, levels=3, iterations=20, extent=None))
    with caplog.at_level(logging.WARNING):
        assert warn_predict_stages(conf, other, log) == ['bias_field']
    assert '"off"' in caplog.text and '"n3"' in caplog.text and other in caplog.text
    caplog.clear()
    _set_block(other, {'mode': 'n3'})
    with caplog.at_level(logging.WARNING):
        assert not warn_predict_stages(conf, other, log)
        assert not warn_predict_stages(EasyDict(folder='run'), plain, log)          # neither records nor asks for anything
    assert caplog.text == ''
    loaders.bias_conf['site_b'] = {'mode': 'off'}                    # the override counts
    with caplog.at_level(logging.WARNING):
        assert warn_predict_stages(conf, other, log) == ['bias_field']


def _minmax_frames(image, RH, RW):
    fr = I.frames(image, RH, RW)
    lo, hi = fr.min(axis=(1, 2), keepdims=True), fr.max(axis=(1, 2), keepdims=True)
    return 2.0 * (fr - lo) / (hi - lo) - 1.0


def test_loader_applies_the_correction(device, folder):
    """training data, prediction and tiles of a shaded folder equal the restatement's correction followed by the existing loader
    restatement (2e-4, the bar of tests/test_volume_loader.py on outputs that span [-1, 1]), and differ from the uncorrected load"""
    from multimodal_segmentation_amd.loaders.volume_folder import VolumeFolderLoader
    loaders.data_conf['chaos'] = folder
    loader = loader_factory.init_loader('chaos')
    params = dict(sigma_mm=40.0, levels=2, iterations=4, extent='3d')
    data = loader.load_all_modalities_concatenated(0, 'training', 1)
    assert device != 'cpu' or len(B.CALLS) == 4                      # volumes 1, 2 x t1, t2: once per uploaded (volume, modality)
    loaders.bias_conf['chaos'] = {'mode': 'off'}
    plain = loader_factory.init_loader('chaos').load_all_modalities_concatenated(0, 'training', 1)
    del loaders.bias_conf['chaos']
    want, corrected = {}, {}
    for v in (1, 2):
        for m, mod in enumerate(loader.modalities):
            image, label, res, selected, spacing = loader._read_file(v, mod, True)
            if selected is not None:
                image, label = image[selected], label[selected]
            ref = B.correct(image.astype(np.float32), (spacing, res[0], res[1]), params)
            assert ref['updates'] == 8
            corrected[v, m] = ref['out']
            want[v, m], want_m = R.preprocess(ref['out'], label, res, loader.target_resolution, loader.label_values, (64, 64))
            got = data.get_volume_images_modi(m, v)
            assert np.abs(got - want[v, m]).max() <= 2e-4, (v, mod)
            assert np.array_equal(data.get_volume_masks_modi(m, v), want_m)          # the label path is untouched
            assert np.abs(got - plain.get_volume_images_modi(m, v)).max() > 0.02, (v, mod)
            assert np.array_equal(plain.get_volume_masks_modi(m, v), want_m)
    images, geometry = loader.load_volume_for_prediction(1)
    for m in range(2):
        assert np.abs(nn.to_numpy(images[m]) - want[1, m]).max() <= 2e-4
    if device == 'cpu':
        del B.CALLS[:]
    uploaded = loader.upload_volume(1)
    tiles_seen = 0
    for m in range(2):
        tiles, geo, plan = loader.load_volume_tiles(1, m, (16, 16), uploaded)
        for j in range(2):
            S = corrected[1, j].shape[0]
            RH, RW = geo[j]['resampled']
            mapped = _minmax_frames(corrected[1, j], RH, RW)
            rows, cols = plan[j]
            tiles_seen = max(tiles_seen, len(rows) * len(cols))
            got = nn.to_numpy(tiles[j])
            for tr, r in enumerate(rows):
                for tc, c in enumerate(cols):
                    t = tr * len(cols) + tc
                    assert np.abs(got[t * S:(t + 1) * S, ..., 0] - I.crop_pad(mapped, r, c, (64, 64))).max() <= 2e-4, (m, j, tr, tc)
    assert tiles_seen > 1 and (device != 'cpu' or len(B.CALLS) == 2)          # no correction per tile, nor per predicted modality


def test_folder_without_the_key_launches_nothing_new(device, folder, monkeypatch):
    """absent key and {"mode": "off"}: no mmseg_bias_* entry point is called, the arrays of the two are bitwise equal, and the volume that
    reaches the preprocessing kernels is the uploaded tensor itself"""
    from multimodal_segmentation_amd import _native
    from multimodal_segmentation_amd.loaders.volume_folder import VolumeFolderLoader
    called = []
    real_call = _native.call          # the stand-in's dispatcher on the CPU; put back here, before the fixture removes the stand-in
    _native.call = lambda name, *a: (called.append(name), real_call(name, *a))[1]
    results = []
    try:
        for block in (None, {'mode': 'off'}):
            _set_block(folder, block)
            loader = VolumeFolderLoader(folder)
            assert loader.bias_field == {'mode': 'off'}
            x = torch.zeros(2, 4, 4)
            assert loader.bias_corrected(x, (1.5, 1.5)) is x
            data = loader.load_all_modalities_concatenated(0, 'training', 1)
            images, _ = loader.load_volume_for_prediction(3)
            results.append([data.get_images_modi(0), data.get_masks_modi(1)] + [nn.to_numpy(i) for i in images])
    finally:
        _native.call = real_call
    assert called and not [n for n in called if n.startswith('mmseg_bias')]
    for a, b in zip(*results):
        assert np.array_equal(a, b)


# ---- the example folder -------------------------------------------------------------------------------------------------------------------------
def test_example_folder_with_a_bias_field(tmp_path):
    tool = R.tool()
    plain, shaded = str(tmp_path / 'plain'), str(tmp_path / 'shaded')
    a = tool.write_folder(plain, volumes=3, size=32, slices=2, seed=1, slice_spacing=(5.0, 8.0))
    b = tool.write_folder(shaded, volumes=3, size=32, slices=2, seed=1, slice_spacing=(5.0, 8.0), bias_field=0.3)
    assert b.pop('bias_field') == {'mode': 'n3'} and a == b
    for name in sorted(os.listdir(plain)):
        if not name.endswith('.npz'):
            continue
        p, s = np.load(os.path.join(plain, name)), np.load(os.path.join(shaded, name))
        assert np.array_equal(p['label'], s['label']) and np.array_equal(p['resolution'], s['resolution']) and p['slice_spacing'] == s['slice_spacing']
        assert s['image'].dtype == np.int16 and s['image'].shape == p['image'].shape
        ratio = np.log(s['image'].astype(np.float64) / (p['image'].astype(np.float64) + 0.1 * p['image'].max()))
        assert 0.25 < np.abs(ratio).max() < 0.35 and np.abs(np.diff(ratio, axis=2)).max() < 0.05          # a field of the strength asked for, and smooth
    with pytest.raises(ValueError):
        tool.write_folder(str(tmp_path / 'bad'), bias_field=-1.0)


# ---- ABI --------------------------------------------------------------------------------------------------------------------------------------
def test_entry_points_declared():
    from multimodal_segmentation_amd import _native
    protos = _native.parse_header()
    for name in list(B.STANDINS) + ['mmseg_bias_otsu', 'mmseg_bias_histogram', 'mmseg_bias_sharpen', 'mmseg_bias_smooth', 'mmseg_bias_update']:
        assert name in protos, name
    _native.build()
    lib = _native.load()
    assert all(hasattr(lib, n) for n in protos if n.startswith('mmseg_bias'))
