"""Non-local means denoising of volumes read from a folder: csrc/denoise.hip (mmseg_nlm_*), ops.nlm_sigma / ops.nlm_denoise, the `denoise`
block of loaders/volume_folder.py, tools/make_volume_folder.py --rician_noise and the `--denoise*` options of experiment.py, against the
numpy restatement in tests/volume_denoise_ref.py (the rule is in include/mmseg_hip.h).  Every measured figure is printed before it is
asserted (pytest -s shows them; profiles/volume_denoise_bench.md records them)."""
import json
import logging
import os

import numpy as np
import pytest
import torch

from multimodal_segmentation_amd import loaders, nn, ops
from multimodal_segmentation_amd.loaders import loader_factory
from tests import volume_bias_ref as B
from tests import volume_denoise_ref as D
from tests import volume_intensity_ref as I
from tests import volume_loader_ref as R

gpu = pytest.mark.gpu
DEV = 'cuda:0'
SIGMA = 10.0
TH, TW = ops.NLM_TILE

# ---- the parity cases: each the smallest that exercises its edge ----------------------------------------------------------------------------
CASES = {
    'window>slice': ((1, 7, 5), dict(search_radius=5, patch_radius=1)),                     # every patch is clamped
    'defaults': ((2, 48, 56), dict()),                                                      # full windows, several tiles
    'odd-2.5d': ((3, 20, 37), dict(search_radius=3, patch_radius=2, search_radius_z=1)),    # partial tiles, slices missing at both ends
    'largest-radii': ((1, 40, 33), dict(search_radius=10, patch_radius=3)),
    'Rz>S': ((2, 9, 9), dict(search_radius=2, patch_radius=1, search_radius_z=4)),
    'seam+1': ((1, TH + 1, TW + 1), dict()),                                                # one pixel past a seam on both axes
    'exact-tiles': ((1, 2 * TH, 2 * TW), dict()),
}
NOISES = ('gaussian', 'rician')

# The bar.  GAP is the largest difference between the restatement run in fp32 and in fp64 over CASES x NOISES, relative to max |x|
# (Gaussian outputs) or max x^2 (Rician, before the square root), measured with numpy on the host:
#     gaussian 1.32e-6, rician 1.70e-6, both at 'largest-radii' (49 taps: the largest patch distances, so the largest arguments of exp2,
#     whose fp32 rounding is what moves a weight); 4.8e-7 and 6.5e-7 at the defaults; below 3e-7 elsewhere
# GAP is that rounded up; test_bar_rests_on_the_measured_gap measures it again and holds it under GAP.  The device gets 16 times that (the
# hardware exp2 and another association of the sums are the only legitimate sources of more) but never more than 1e-5 of the scale, which
# is what binds here: BAR = 1e-5, 6 times the fp32 restatement's own distance.  A dropped or doubled tap moves an output by about
# 1 / (number of offsets) of a local contrast, orders of magnitude above that.
GAP = 2e-6
BAR = min(16 * GAP, 1e-5)

_cache = {}


def _case(name):
    """the case's noisy phantom, computed once and shared"""
    if ('x', name) not in _cache:
        shape = CASES[name][0]
        _cache['x', name] = D.phantom(shape, seed=len(name), sigma=SIGMA)[0]
    return _cache['x', name]


def _ref(name, noise, dtype=np.float64):
    key = ('ref', name, noise, dtype)
    if key not in _cache:
        _cache[key] = D.nlm(_case(name), SIGMA, dict(CASES[name][1], noise=noise), dtype)
    return _cache[key]


def _gap(name, noise):
    x = _case(name)
    a, b = _ref(name, noise, np.float32), _ref(name, noise)
    if noise == 'gaussian':
        return float(np.abs(a['out'].astype(np.float64) - b['out']).max() / np.abs(x).max())
    return float(np.abs(np.maximum(a['pre'].astype(np.float64), 0) - np.maximum(b['pre'], 0)).max() / np.square(x.astype(np.float64)).max())


@pytest.fixture(autouse=True)
def _clean_registries():
    saved = dict(loaders.data_conf), dict(loaders.intensity_conf), dict(loaders.bias_conf), dict(loaders.denoise_conf)
    yield
    for registry, old in zip((loaders.data_conf, loaders.intensity_conf, loaders.bias_conf, loaders.denoise_conf), saved):
        registry.clear()
        registry.update(old)


def _install(monkeypatch):
    from tests import cpu_backend as cb
    for table in (R.STANDINS, I.STANDINS, B.STANDINS, D.STANDINS):
        for name, fn in table.items():
            monkeypatch.setitem(cb._TABLE, name, fn)
    monkeypatch.setattr(B, 'CALLS', [])
    monkeypatch.setattr(D, 'CALLS', [])
    cb.install()
    nn.set_default_device('cpu')
    return cb


@pytest.fixture
def standin(monkeypatch):
    """the CPU stand-in of the C ABI with the stand-ins of the preprocessing, bias and denoising entry points added to its table"""
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


FOLDER_BLOCK = {'mode': 'nlm', 'sigma': 25.0, 'search_radius': 3}


@pytest.fixture
def folder(tmp_path):
    """a noisy example folder (a Rician channel of 25 grey values), slice spacings in the files"""
    out = str(tmp_path / 'volumes')
    R.tool().write_folder(out, volumes=4, size=64, slices=4, seed=3, slice_spacing=(5.0, 8.0), rician_noise=25.0)
    _set_block(out, FOLDER_BLOCK)
    return out


def _set_block(folder, block, key='denoise'):
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


# ---- 1. parity with the fp64 restatement ------------------------------------------------------------------------------------------------
def test_bar_rests_on_the_measured_gap():
    """fp32 against fp64 on the restatement's side, over every case and both noise models: what GAP above records"""
    worst = {}
    for noise in NOISES:
        gaps = {name: _gap(name, noise) for name in sorted(CASES)}
        top = max(gaps, key=gaps.get)
        worst[noise] = gaps[top]
        print('%s: fp32 restatement within %.2e of the fp64 one (largest at %s)' % (noise, gaps[top], top))
    assert 1e-8 < max(worst.values()) <= GAP and BAR <= 1e-5


@gpu
@pytest.mark.parametrize('noise', NOISES)
@pytest.mark.parametrize('name', sorted(CASES))
def test_device_equals_the_restatement(name, noise):
    x, ref = _case(name), _ref(name, noise)
    params = dict(CASES[name][1], noise=noise, sigma=SIGMA)
    if params.get('search_radius_z'):
        params['extent'] = '3d'
    xd = _dev(x)
    got = ops.nlm_denoise(xd, params).cpu().numpy().astype(np.float64)
    assert np.all(np.isfinite(got)) and np.array_equal(xd.cpu().numpy(), x)          # every element written, the input left alone
    if noise == 'gaussian':
        err = np.abs(got - ref['out']).max() / np.abs(x).max()
        print('%s gaussian: largest error %.3e of max |x| (bar %.2e)' % (name, err, BAR))
        assert err <= BAR
        return
    # Rician: before the square root, where an fp32 rounding in a background voxel is not magnified
    scale = np.square(x.astype(np.float64)).max()
    err = np.abs(got * got - np.maximum(ref['pre'], 0.0)).max() / scale
    print('%s rician: largest error of out^2 %.3e of max x^2 (bar %.2e)' % (name, err, BAR))
    assert err <= BAR
    # and after it where the value is away from 0.  |sqrt(a) - sqrt(b)| = |a - b| / (sqrt(a) + sqrt(b)) <= |a - b| / sqrt(a): per voxel
    # BAR scale / sqrt(pre), plus the root's own rounding
    away = ref['pre'] > (SIGMA / 4.0) ** 2
    root_bar = BAR * scale / np.sqrt(ref['pre'][away]) + 2.0 ** -23 * np.abs(x).max()
    err = np.abs(got - ref['out'])[away]
    print('%s rician: largest error of out %.3e, largest error / bar %.3e over %d voxels above (sigma / 4)^2'
          % (name, err.max(), (err / root_bar).max(), away.sum()))
    assert away.sum() > 0.5 * away.size and np.all(err <= root_bar)


# ---- 2. properties -----------------------------------------------------------------------------------------------------------------------
@gpu
def test_two_runs_and_both_ways_of_passing_sigma_give_equal_bits():
    x = _dev(_case('odd-2.5d'))
    params = dict(CASES['odd-2.5d'][1], extent='3d')
    out, sigma = ops.nlm_denoise(x, params, sigma_out=True)          # auto: the kernel reads the device scalar
    again, sigma2 = ops.nlm_denoise(x, params, sigma_out=True)
    assert torch.equal(out, again) and torch.equal(sigma, sigma2) and sigma.dtype == torch.float64
    by_value = ops.nlm_denoise(x, dict(params, sigma=float(sigma.item())))
    assert torch.equal(out, by_value) and not torch.equal(out, x)


@gpu
def test_slices_are_independent_without_a_search_across_them():
    x = _dev(D.phantom((3, 20, 37), seed=5, sigma=SIGMA)[0])
    params = dict(search_radius=3, patch_radius=2, sigma=SIGMA)
    whole = ops.nlm_denoise(x, params)
    for s in range(3):
        assert torch.equal(whole[s:s + 1], ops.nlm_denoise(x[s:s + 1].contiguous(), params)), s
    assert not torch.equal(whole, ops.nlm_denoise(x, dict(params, extent='3d')))          # the 2.5-D search does read the neighbours


@gpu
@pytest.mark.parametrize('shape', [(3, 20, 24), (1, 3, 3)])
def test_sigma_equals_the_restatement(shape):
    x = D.phantom(shape, seed=2, sigma=SIGMA)[0]
    want = D.immerkaer(x)
    got = [float(ops.nlm_sigma(_dev(x)).item()) for _ in range(2)]
    print('sigma %s: %.15g (restatement %.15g)' % (shape, got[0], want))
    assert got[0] == got[1] and want > 0 and abs(got[0] - want) <= 1e-12 * want


@gpu
@pytest.mark.parametrize('name', ['1x2x9', 'constant'])
def test_volumes_without_an_estimate_keep_their_bits(name):
    x = D.phantom((1, 2, 9), seed=1)[0] if name == '1x2x9' else np.full((2, 9, 11), 41.5, np.float32)
    assert D.immerkaer(x) == 0.0
    xd = _dev(x)
    assert float(ops.nlm_sigma(xd).item()) == 0.0
    out, sigma = ops.nlm_denoise(xd, sigma_out=True)
    assert float(sigma.item()) == 0.0 and np.array_equal(out.cpu().numpy().view(np.uint32), x.view(np.uint32))


def _refusals(x_ptr, out_ptr, sigma_ptr, n_bytes):
    """(entry point, arguments) that the rule refuses, for S, H, W = 2, 9, 11"""
    good = dict(x=x_ptr, out=out_ptr, sd=None, sigma=10.0, S=2, H=9, W=11, Rs=5, Rp=1, Rz=0, h=1.0, ric=1)
    order = ('x', 'out', 'sd', 'sigma', 'S', 'H', 'W', 'Rs', 'Rp', 'Rz', 'h', 'ric')
    bad = [dict(Rs=0), dict(Rs=11), dict(Rp=0), dict(Rp=4), dict(Rz=-1), dict(Rz=5), dict(h=0.0), dict(h=float('inf')), dict(h=float('nan')),
           dict(ric=2), dict(x=None), dict(out=None), dict(out=x_ptr), dict(out=x_ptr + n_bytes - 4), dict(S=65536, H=32768, W=1),
           dict(S=-1), dict(H=0), dict(W=0)]
    calls = [('mmseg_nlm_denoise', [dict(good, **b)[k] for k in order] + [None]) for b in bad]
    for b in (dict(x=None), dict(ws=None), dict(out=None), dict(S=65536, H=32768, W=1), dict(H=0)):
        a = dict(dict(x=x_ptr, ws=out_ptr, out=sigma_ptr, S=2, H=9, W=11), **b)
        calls.append(('mmseg_nlm_sigma', [a[k] for k in ('x', 'ws', 'out', 'S', 'H', 'W')] + [None]))
    return calls


def test_refusals_return_the_error_before_anything_is_launched():
    """on any machine: a refused call launches nothing and touches no memory, so made-up pointers do"""
    from multimodal_segmentation_amd import _native
    _native.build()
    lib = _native.load()
    for name, args in _refusals(4096, 8192, 16384, 2 * 9 * 11 * 4):
        assert getattr(lib, name)(*args) == 1, (name, args)          # hipErrorInvalidValue
    assert lib.mmseg_nlm_workspace_bytes(36, 256, 256) == 8 * 1024
    assert lib.mmseg_nlm_workspace_bytes(0, 8, 8) == 0 and lib.mmseg_nlm_workspace_bytes(65536, 32768, 1) == 0
    assert lib.mmseg_nlm_denoise(None, None, None, 10.0, 0, 9, 11, 5, 1, 0, 1.0, 1, None) == 0          # S = 0 does nothing
    assert lib.mmseg_nlm_sigma(None, None, None, 0, 9, 11, None) == 0
    src = open(os.path.join(_native.CSRC_DIR, 'denoise.hip')).read()
    assert 'NLM_TW = %d, NLM_TH = %d' % (TW, TH) in src          # ops.NLM_TILE is the kernel's tile


@gpu
def test_refusals_leave_the_output_unchanged():
    from multimodal_segmentation_amd import _native
    lib = _native.load()
    x = _dev(D.phantom((2, 9, 11), seed=3)[0])
    out, sigma = torch.full_like(x, -7.0), torch.full((1,), -7.0, dtype=torch.float64, device=DEV)
    for name, args in _refusals(x.data_ptr(), out.data_ptr(), sigma.data_ptr(), x.numel() * 4):
        assert getattr(lib, name)(*args) == 1, (name, args)
    torch.cuda.synchronize()
    assert bool((out == -7.0).all()) and float(sigma.item()) == -7.0
    with pytest.raises(ValueError):
        ops.nlm_denoise(x, out=x)


def test_restatement_denoises_the_phantom_at_the_defaults():
    x, clean = D.phantom((2, 64, 64), seed=0, sigma=SIGMA)
    sigma = D.immerkaer(x)
    out = D.nlm(x, sigma)['out']
    before, after = D.rmse(x, clean), D.rmse(out, clean)
    print('restatement: sigma estimated %.2f (true %.0f), RMSE against the clean phantom %.2f -> %.2f' % (sigma, SIGMA, before, after))
    assert after < 0.5 * before


@gpu
def test_device_denoises_the_phantom_at_the_defaults():
    x, clean = D.phantom((2, 64, 64), seed=0, sigma=SIGMA)
    out, sigma = ops.nlm_denoise(_dev(x), sigma_out=True)          # sigma = auto
    before, after = D.rmse(x, clean), D.rmse(out.cpu().numpy(), clean)
    print('MI355X: sigma estimated %.2f (true %.0f), RMSE against the clean phantom %.2f -> %.2f' % (float(sigma.item()), SIGMA, before, after))
    assert after < 0.5 * before


# ---- 3. host logic --------------------------------------------------------------------------------------------------------------------------
def test_host_logic_on_the_standin(standin):
    """ops.nlm_denoise drives the stand-ins to the restatement's result: defaults, the estimate under auto, the order of the calls"""
    x = _case('odd-2.5d')
    t = torch.from_numpy(x)
    out, sigma = ops.nlm_denoise(t, sigma_out=True)
    assert D.CALLS == [('mmseg_nlm_sigma', 3, 20, 37), ('mmseg_nlm_denoise', 3, 20, 37)] and float(sigma) == D.immerkaer(x)
    assert np.array_equal(out.numpy(), D.nlm(x, D.immerkaer(x), dtype=np.float32)['out'])
    del D.CALLS[:]
    out = ops.nlm_denoise(t, dict(sigma=SIGMA, extent='3d', noise='gaussian', search_radius=2))
    assert D.CALLS == [('mmseg_nlm_denoise', 3, 20, 37)]
    assert np.array_equal(out.numpy(), D.nlm(x, SIGMA, dict(search_radius=2, search_radius_z=1, noise='gaussian'), np.float32)['out'])
    assert ops.nlm_denoise(torch.zeros(0, 4, 4)).shape == (0, 4, 4)
    assert ops.nlm_params() == dict(search_radius=5, patch_radius=1, search_radius_z=0, h=1.0, noise='rician', sigma='auto', extent='2d')
    assert ops.nlm_params(dict(extent='3d'))['search_radius_z'] == 1
    for bad, text in ((dict(search_radius=0), 'search_radius must be a whole number in 1..10'), (dict(patch_radius=4), 'patch_radius must be'),
                      (dict(search_radius_z=2), 'goes with extent 3d'), (dict(extent='3d', search_radius_z=5), 'search_radius_z must be'),
                      (dict(h=0), 'h must be'), (dict(noise='poisson'), 'noise must be one of rician, gaussian'),
                      (dict(sigma=-1.0), 'sigma must be'), (dict(sigma='high'), 'sigma must be'), (dict(window=3), 'unknown key(s) window')):
        with pytest.raises(ValueError) as e:
            ops.nlm_denoise(t, bad)
        assert text in str(e.value), (bad, str(e.value))
    with pytest.raises(ValueError):
        ops.nlm_denoise(t, out=t)


def test_manifest_validation_messages(folder):
    from multimodal_segmentation_amd.loaders.volume_folder import check_denoise, read_manifest
    mods = ['t1', 't2']
    assert check_denoise(None, mods, 'x') == {'mode': 'off'} == check_denoise({}, mods, 'x') == check_denoise({'mode': 'off'}, mods, 'x')
    assert check_denoise({'mode': 'nlm'}, mods, 'x') == dict(mode='nlm', search_radius=5, patch_radius=1, search_radius_z=0, h=1.0,
                                                              noise='rician', sigma='auto', extent='2d')
    assert check_denoise({'mode': 'nlm', 'sigma': {'t1': 8, 't2': 12.5}}, mods, 'x')['sigma'] == {'t1': 8.0, 't2': 12.5}
    for block, text in (([1], 'must be an object'), ({'mode': 'bm3d'}, 'mode must be one of off, nlm'), ({'mode': 'nlm', 'window': 5}, 'unknown key(s) window'),
                        ({'mode': 'off', 'h': 2}, 'mode off takes no other key'), ({'mode': 'nlm', 'search_radius': 11}, 'search_radius must be a whole number in 1..10'),
                        ({'mode': 'nlm', 'patch_radius': 0}, 'patch_radius must be a whole number in 1..3'), ({'mode': 'nlm', 'h': -1}, 'h must be'),
                        ({'mode': 'nlm', 'sigma': 0}, 'sigma must be'), ({'mode': 'nlm', 'sigma': {'t1': 8}}, "no value for modality 't2'"),
                        ({'mode': 'nlm', 'sigma': {'t1': 8, 't2': 9, 'pd': 3}}, "'pd', which is no modality"),
                        ({'mode': 'nlm', 'sigma': {'t1': 8, 't2': 'auto'}}, "modality 't2' must be a number"),
                        ({'mode': 'nlm', 'search_radius_z': 1}, 'goes with extent 3d'), ({'mode': 'nlm', 'extent': '4d'}, 'extent must be one of 2d, 3d'),
                        ({'mode': 'nlm', 'noise': 'white'}, 'noise must be one of rician, gaussian')):
        _set_block(folder, block)
        with pytest.raises(ValueError) as e:
            read_manifest(folder)
        assert text in str(e.value) and 'dataset.json' in str(e.value) and 'denoise' in str(e.value), (block, str(e.value))


def test_3d_needs_one_run_of_slices_and_no_slice_spacing(standin, folder):
    from multimodal_segmentation_amd.loaders.volume_folder import VolumeFolderLoader
    _set_block(folder, dict(FOLDER_BLOCK, extent='3d'))
    path = os.path.join(folder, 'vol01_t2.npz')
    with np.load(path) as z:
        arrays = {k: z[k] for k in z.files if k != 'slice_spacing'}
    np.savez_compressed(path, **arrays)
    VolumeFolderLoader(folder).load_volume_for_prediction(1)          # no slice_spacing needed: the rule has no mm in it
    manifest = json.load(open(os.path.join(folder, 'dataset.json')))
    first = manifest['volumes']['2']['t2'].get('slices', [[0, 4]])[0][0]
    manifest['volumes']['2']['t1']['slices'] = [[0, 2], [3, 4]]          # three slices with a gap (the file holds four)
    manifest['volumes']['2']['t2']['slices'] = [[first, first + 3]]      # three in one run
    json.dump(manifest, open(os.path.join(folder, 'dataset.json'), 'w'))
    loader = VolumeFolderLoader(folder)
    for load in (lambda: loader.load_volume_for_prediction(2), lambda: loader.upload_volume(2)):
        with pytest.raises(ValueError) as e:
            load()
        assert '"denoise" extent 3d needs one contiguous run of slices' in str(e.value) and 'volume 2, modality t1' in str(e.value)
    _set_block(folder, dict(FOLDER_BLOCK, extent='2d'))
    VolumeFolderLoader(folder).load_volume_for_prediction(2)          # 2d takes any selection


def test_denoise_conf_overrides_the_folder(standin, folder):
    loaders.data_conf['chaos'] = folder
    own = dict(mode='nlm', search_radius=3, patch_radius=1, search_radius_z=0, h=1.0, noise='rician', sigma=25.0, extent='2d')
    assert loader_factory.init_loader('chaos').denoise == own
    loaders.denoise_conf['chaos'] = {'mode': 'off'}
    loader = loader_factory.init_loader('chaos')
    assert loader.denoise == {'mode': 'off'}
    loader.load_volume_for_prediction(1)
    assert D.CALLS == []                                             # the registry changes what is computed, not only what is reported
    loaders.denoise_conf['chaos'] = {'mode': 'nlm', 'search_radius': 1, 'sigma': {'t1': 20.0, 't2': 30.0}}
    loader_factory.init_loader('chaos').load_volume_for_prediction(1)
    assert [c[0] for c in D.CALLS] == ['mmseg_nlm_denoise'] * 2      # one per modality, no estimate: sigma is given
    loaders.denoise_conf['chaos'] = {'mode': 'nlm', 'search_radius': 99}
    with pytest.raises(ValueError) as e:
        loader_factory.init_loader('chaos')
    assert "loaders.denoise_conf['chaos']" in str(e.value)


def test_cli_override_reaches_the_loader_and_the_recorded_configuration(folder, tmp_path, monkeypatch):
    from multimodal_segmentation_amd.experiment import Experiment, parse_arguments
    monkeypatch.chdir(tmp_path)
    base = ['--config', 'dafnet_config_chaos', '--split', '0', '--data_folder', folder]
    own = dict(mode='nlm', search_radius=3, patch_radius=1, search_radius_z=0, h=1.0, noise='rician', sigma=25.0, extent='2d')
    conf = Experiment().get_config(0, parse_arguments(base))
    assert loaders.denoise_conf == {} and conf.denoise == own          # no override: the folder's own block
    conf = Experiment().get_config(0, parse_arguments(base + ['--denoise', 'nlm', '--denoise_sigma', '12.5', '--denoise_h', '0.8', '--denoise_search', '4',
                                                               '--denoise_patch', '2', '--denoise_search_z', '2', '--denoise_extent', '3d',
                                                               '--denoise_noise', 'gaussian']))
    want = dict(mode='nlm', search_radius=4, patch_radius=2, search_radius_z=2, h=0.8, noise='gaussian', sigma=12.5, extent='3d')
    assert loaders.denoise_conf == {'chaos': want} and conf.denoise == want
    assert loader_factory.init_loader('chaos').denoise == want
    dumped = json.load(open(os.path.join(conf.folder, 'experiment_configuration.json')))
    assert dumped['denoise'] == want and dumped['data_folder'] == folder
    conf = Experiment().get_config(0, parse_arguments(base + ['--denoise', 'nlm', '--denoise_sigma', 'auto']))
    assert conf.denoise['sigma'] == 'auto' and conf.denoise['search_radius'] == 5
    conf = Experiment().get_config(0, parse_arguments(base + ['--denoise', 'off']))
    assert conf.denoise == {'mode': 'off'} == loader_factory.init_loader('chaos').denoise
    conf = Experiment().get_config(0, parse_arguments(base))          # a later run without the options follows dataset.json again
    assert loaders.denoise_conf == {} and loader_factory.init_loader('chaos').denoise == own
    for bad in (['--denoise_h', '2'], ['--denoise', 'off', '--denoise_sigma', '30'], ['--denoise', 'bm3d'], ['--denoise', 'nlm', '--denoise_sigma', 'high']):
        with pytest.raises(SystemExit):
            parse_arguments(base + bad)
    with pytest.raises(ValueError):
        Experiment().get_config(0, parse_arguments(base + ['--denoise', 'nlm', '--denoise_search', '0']))


def test_predict_folder_with_another_setting_logs_a_warning(folder, tmp_path, caplog):
    from multimodal_segmentation_amd.utils.config import EasyDict
    from multimodal_segmentation_amd.experiment import warn_predict_stages
    other = str(tmp_path / 'scans')
    R.tool().write_folder(other, volumes=3, size=64, slices=2, seed=5, name='site_b', unlabelled=True)
    plain = str(tmp_path / 'plain')
    R.tool().write_folder(plain, volumes=3, size=32, slices=2, seed=1)
    log = logging.getLogger('test_volume_denoise')
    trained = dict(mode='nlm', search_radius=5, patch_radius=1, search_radius_z=0, h=1.0, noise='rician', sigma='auto', extent='2d')
    conf = EasyDict(folder='run', denoise=trained)
    with caplog.at_level(logging.WARNING):
        assert warn_predict_stages(conf, other, log) == ['denoise']
    assert '"off"' in caplog.text and '"nlm"' in caplog.text and other in caplog.text
    caplog.clear()
    _set_block(other, {'mode': 'nlm'})
    with caplog.at_level(logging.WARNING):
        assert not warn_predict_stages(conf, other, log)
        assert not warn_predict_stages(EasyDict(folder='run'), plain, log)          # neither records nor asks for anything
    assert caplog.text == ''
    loaders.denoise_conf['site_b'] = {'mode': 'off'}                 # the override counts
    with caplog.at_level(logging.WARNING):
        assert warn_predict_stages(conf, other, log) == ['denoise']


def test_loader_denoises_before_it_corrects_the_bias(device, folder):
    """with both keys set, what reaches the preprocessing kernels is exactly ops.bias_correct(ops.nlm_denoise(x)); the three upload sites
    agree, and each (volume, modality) is denoised once"""
    from multimodal_segmentation_amd.loaders.volume_folder import VolumeFolderLoader
    bias = {'mode': 'n3', 'levels': 1, 'iterations': 2}
    _set_block(folder, bias, 'bias_field')
    loader = VolumeFolderLoader(folder)
    dev = nn.default_device()
    raw, geometry = loader.upload_volume(1)
    assert device != 'cpu' or ([c[0] for c in D.CALLS] == ['mmseg_nlm_denoise'] * 2 and len(B.CALLS) == 2)
    want = []
    for m, mod in enumerate(loader.modalities):
        image, label, res, selected, spacing = loader._read_file(1, mod, False)
        x = nn.host_to_device(image if selected is None else image[selected], dev, np.float32)
        den = ops.nlm_denoise(x, dict(sigma=25.0, search_radius=3))
        want.append(ops.bias_correct(den, (spacing, float(res[0]), float(res[1])), dict(levels=1, iterations=2, extent='3d')))
        assert torch.equal(raw[m], want[m]), mod
        assert not torch.equal(raw[m], ops.bias_correct(x, (spacing, float(res[0]), float(res[1])), dict(levels=1, iterations=2, extent='3d')))
        assert D.rmse(nn.to_numpy(den), nn.to_numpy(x)) > 5.0          # the denoising changed the volume by about the noise it removed
    images, _ = loader.load_volume_for_prediction(1)
    for m in range(2):
        container = torch.zeros_like(images[m])
        g = geometry[m]
        ops.preprocess_images(want[m], container, g['resampled'], g['rows'], g['cols'], 0)
        assert torch.equal(images[m], container)
    data = loader.load_all_modalities_concatenated(0, 'test', 1)
    v = loader.get_volumes_for_split(0, 'test')[0]
    again, _ = loader.load_volume_for_prediction(v)
    for m in range(2):          # the training surface writes through another kernel: 2e-4, the bar of tests/test_volume_loader.py
        assert np.abs(data.get_volume_images_modi(m, v) - nn.to_numpy(again[m])).max() <= 2e-4


def test_folder_without_the_key_launches_nothing_new(device, folder, monkeypatch):
    """absent key and {"mode": "off"}: no mmseg_nlm_* entry point is called, the arrays of the two are bitwise equal, and the volume that
    reaches the rest of the loader is the uploaded tensor itself"""
    from multimodal_segmentation_amd import _native
    from multimodal_segmentation_amd.loaders.volume_folder import VolumeFolderLoader
    called = []
    real_call = _native.call          # the stand-in's dispatcher on the CPU; put back here, before the fixture removes the stand-in
    _native.call = lambda name, *a: (called.append(name), real_call(name, *a))[1]
    results = []
    try:
        for block in (None, {'mode': 'off'}, FOLDER_BLOCK):
            _set_block(folder, block)
            loader = VolumeFolderLoader(folder)
            if block is not FOLDER_BLOCK:
                assert loader.denoise == {'mode': 'off'}
                x = torch.zeros(2, 4, 4)
                assert loader.denoised(x, 't1') is x
            data = loader.load_all_modalities_concatenated(0, 'training', 1)
            images, _ = loader.load_volume_for_prediction(3)
            results.append([data.get_images_modi(0), data.get_masks_modi(1)] + [nn.to_numpy(i) for i in images])
            if block is not FOLDER_BLOCK:
                assert called and not [n for n in called if n.startswith('mmseg_nlm')]
    finally:
        _native.call = real_call
    assert [n for n in called if n.startswith('mmseg_nlm')]          # the count does see the entry points once the key is there
    for a, b in zip(results[0], results[1]):
        assert np.array_equal(a, b)
    assert not np.array_equal(results[0][0], results[2][0]) and np.array_equal(results[0][1], results[2][1])          # images change, labels do not


# ---- the example folder -------------------------------------------------------------------------------------------------------------------------
def test_example_folder_with_rician_noise_loads(standin, tmp_path):
    tool = R.tool()
    plain, noisy = str(tmp_path / 'plain'), str(tmp_path / 'noisy')
    a = tool.write_folder(plain, volumes=3, size=32, slices=2, seed=1)
    b = tool.write_folder(noisy, volumes=3, size=32, slices=2, seed=1, rician_noise=30.0)
    assert b.pop('denoise') == {'mode': 'nlm', 'sigma': 30.0} and a == b
    for name in sorted(os.listdir(plain)):
        if not name.endswith('.npz'):
            continue
        p, s = np.load(os.path.join(plain, name)), np.load(os.path.join(noisy, name))
        assert np.array_equal(p['label'], s['label']) and np.array_equal(p['resolution'], s['resolution'])
        assert s['image'].dtype == np.int16 and s['image'].shape == p['image'].shape and s['image'].min() >= 0
        diff = s['image'].astype(np.float64) - p['image'].astype(np.float64)
        assert 20.0 < diff.std() < 40.0                               # noise of the strength asked for
    with pytest.raises(ValueError):
        tool.write_folder(str(tmp_path / 'bad'), rician_noise=-1.0)
    assert tool.main([str(tmp_path / 'cli'), '--volumes', '3', '--size', '32', '--slices', '2', '--rician_noise', '15']) is None
    from multimodal_segmentation_amd.loaders.volume_folder import VolumeFolderLoader
    loader = VolumeFolderLoader(str(tmp_path / 'cli'))
    assert loader.denoise['sigma'] == 15.0
    images, _ = loader.load_volume_for_prediction(1)
    assert len(D.CALLS) == 2 and all(np.isfinite(nn.to_numpy(i)).all() for i in images)


# ---- ABI --------------------------------------------------------------------------------------------------------------------------------------
def test_entry_points_declared():
    from multimodal_segmentation_amd import _native
    protos = _native.parse_header()
    for name in D.STANDINS:
        assert name in protos, name
    _native.build()
    lib = _native.load()
    assert all(hasattr(lib, n) for n in protos if n.startswith('mmseg_nlm'))
