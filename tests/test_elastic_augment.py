"""Elastic deformation of training batches on the device: mmseg_elastic_field / mmseg_elastic_gather (csrc/augment.hip), ops.elastic_field /
ops.elastic_gather, the ELASTIC_KEYS of conf.datagen_params and AugmentFlow (utils/augment.py) against the numpy + scipy restatement in
tests/elastic_ref.py."""
import numpy as np
import pytest
import torch

from multimodal_segmentation_amd import nn
from multimodal_segmentation_amd.configuration import dafnet_config_chaos
from tests import elastic_ref as E
from tests import helpers as Hh
from tests import keras_datagen_ref as KR
from tests.test_augment_full import (_GEOMS, _check, _executor, _folded, _geom_matrix, _light_executor, _smooth,
                                     _standin_augment_gather)

TILE_W, TILE_H, TILE_C = 128, 64, 8          # EL_TW, EL_TH, EL_TC of csrc/augment.hip: columns per block of the first pass, rows x columns of the second
FIELD_SHAPES = (                             # (H, W, sigma)
    (5, 7, 3.0),                             # radius 12 exceeds both extents: the reflection wraps several times
    (37, 30, 2.5),                           # odd extents, R = 10
    (40, 33, 32.0),                          # R = 128, the cap
    (2 * TILE_H + 11, 2 * TILE_W + 13, 2.5),        # three tiles of either pass on each axis, the last one partial
)
SEEDS = ((11, 0), (0xfedcba98, 0x80000003))          # (seed, batch); the second pair has the top bit set in both words
SCALES = (60.0, 0.0, 7.25)
BASE = dict(rotation_range=20., zoom_range=0.2, horizontal_flip=True, vertical_flip=True)
ELASTIC = dict(BASE, elastic_alpha=40., elastic_sigma=3.)


def _dev(a):
    return torch.as_tensor(np.ascontiguousarray(a)).to('cuda')


@pytest.fixture
def standin(monkeypatch):
    """the CPU stand-ins of the gather (tests/test_augment_full.py) and of the new entry points over cpu_backend's table; `calls` records
    the arguments of every field and gather call"""
    from tests import cpu_backend as cb
    calls = []

    def recorded(name, fn):
        def run(*args):
            calls.append((name, args))
            return fn(*args)
        return run

    table = dict(E.STANDINS, mmseg_augment_gather=_standin_augment_gather,
                 mmseg_augment_workspace_floats=lambda B, H, W, C: 2 * B)
    for name, fn in table.items():
        monkeypatch.setitem(cb._TABLE, name, recorded(name, fn) if name.endswith(('_gather', '_field')) else fn)
    cb.install()
    nn.set_default_device('cpu')
    yield calls
    cb.uninstall()


# ---- host: the generator and the dict -------------------------------------------------------------------------------------------------
def test_host_philox_reproduces_the_known_answers():
    from multimodal_segmentation_amd.utils.augment import philox4x32
    for counter, key, out in E.KNOWN_ANSWERS:
        assert tuple(philox4x32(counter, key)) == out
        assert tuple(int(v) for v in E.philox4x32(counter, key)) == out


def test_restated_noise_and_blur_rule():
    """the noise is exact in fp32 and in [-1, 1 - 2^-23]; the product's weights are scipy's; the period-2n reflection rule, restated, is
    gaussian_filter where the radius exceeds the extent"""
    from multimodal_segmentation_amd import ops
    u = E.noise(5, 2, 2, 9, 11)
    assert np.array_equal(u.astype(np.float32).astype(np.float64), u) and u.min() >= -1 and u.max() <= 1 - 2.0 ** -23
    assert abs(u.mean()) < 0.1 and 0.2 < u.var() < 0.45
    H, W, sigma = 5, 7, 3.0
    R, w = ops.elastic_radius(sigma), ops.elastic_weights(sigma)
    assert R == 12 and len(w) == 13 and abs(w[0] + 2 * w[1:].sum() - 1) < 1e-15

    def reflect(i, n):
        t = i % (2 * n)
        return 2 * n - 1 - t if t >= n else t

    x = u[0, :H, :W, 0]
    rows = np.array([[sum(w[abs(k)] * x[reflect(r + k, H), c] for k in range(-R, R + 1)) for c in range(W)] for r in range(H)])
    both = np.array([[sum(w[abs(k)] * rows[r, reflect(c + k, W)] for k in range(-R, R + 1)) for c in range(W)] for r in range(H)])
    from scipy.ndimage import gaussian_filter
    assert np.abs(both - gaussian_filter(x, sigma, mode='reflect', truncate=4.0)).max() < 1e-15


@pytest.mark.parametrize('bad,word', [
    (dict(elastic_alpha='3'), 'elastic_alpha'), (dict(elastic_alpha=-1., elastic_sigma=2.), 'elastic_alpha'),
    (dict(elastic_alpha=None), 'elastic_alpha'), (dict(elastic_alpha=True, elastic_sigma=2.), 'elastic_alpha'),
    (dict(elastic_alpha=float('nan'), elastic_sigma=2.), 'elastic_alpha'),
    (dict(elastic_alpha=10.), 'elastic_sigma'), (dict(elastic_alpha=10., elastic_sigma=0.), 'elastic_sigma'),
    (dict(elastic_alpha=10., elastic_sigma=-2.), 'elastic_sigma'), (dict(elastic_sigma='wide'), 'elastic_sigma'),
    (dict(elastic_alpha=10., elastic_sigma=0.12), 'elastic_sigma'),           # int(4 sigma + 0.5) = 0
    (dict(elastic_alpha=10., elastic_sigma=32.2), 'elastic_sigma'),           # 129
    (dict(elastic_alpha=10., elastic_sigma=2., elastic_prob=1.5), 'elastic_prob'),
    (dict(elastic_prob=-0.1), 'elastic_prob'), (dict(elastic_prob='often'), 'elastic_prob'),
    (dict(elastic_prob=float('nan')), 'elastic_prob'),
    (dict(elastic_seed=1.5), 'elastic_seed'),
    (dict(elastic_alhpa=10.), 'unknown datagen parameter'),
])
def test_elastic_keys_validate(bad, word):
    from multimodal_segmentation_amd.utils.augment import DATAGEN_KEYS, ELASTIC_KEYS, check_datagen_params
    assert ELASTIC_KEYS == ('elastic_alpha', 'elastic_sigma', 'elastic_prob', 'elastic_seed') and not set(ELASTIC_KEYS) & set(DATAGEN_KEYS)
    p = dict(rotation_range=20., zoom_range=0)
    for good in (dict(elastic_alpha=0), dict(elastic_alpha=30, elastic_sigma=4), dict(elastic_alpha=30., elastic_sigma=32.1),
                 dict(elastic_alpha=30., elastic_sigma=0.125), dict(elastic_sigma=3.),
                 dict(elastic_alpha=np.float32(30.), elastic_sigma=np.float64(4.), elastic_prob=0, elastic_seed=np.int64(4))):
        assert check_datagen_params(dict(p, **good)) == dict(p, **good)
    with pytest.raises(ValueError, match=word):
        check_datagen_params(dict(p, **bad))


def test_rotation_only_is_false_with_elastic_on_and_unchanged_with_it_off():
    from multimodal_segmentation_amd.utils.augment import AugmentFlow, RotationFlow, rotation_only
    rot = dict(rotation_range=20., zoom_range=0, horizontal_flip=False)
    assert rotation_only(rot)
    assert not rotation_only(dict(rot, elastic_alpha=30., elastic_sigma=4.))
    assert not rotation_only(dict(rot, elastic_alpha=30., elastic_sigma=4., elastic_prob=0.5))
    for off in (dict(elastic_alpha=0), dict(elastic_alpha=0., elastic_sigma=4.), dict(elastic_alpha=30., elastic_sigma=4., elastic_prob=0),
                dict(elastic_sigma=4., elastic_seed=3)):
        assert rotation_only(dict(rot, **off))
        assert not rotation_only(dict(rot, horizontal_flip=True, **off))
    imgs = [np.zeros((3, 64, 64, 1), np.float32)]
    on = Hh.make_conf(dafnet_config_chaos, 64, batch_size=2, datagen_params=dict(elastic_alpha=30., elastic_sigma=4.))
    gen = _light_executor(on).get_data_generator(train_images=imgs)
    assert isinstance(gen, AugmentFlow) and gen.elastic == (30., 4., 1., on.seed)
    off = Hh.make_conf(dafnet_config_chaos, 64, batch_size=2, datagen_params=dict(elastic_alpha=0., elastic_sigma=4.))
    assert isinstance(_light_executor(off).get_data_generator(train_images=imgs), RotationFlow)
    bad = Hh.make_conf(dafnet_config_chaos, 64, batch_size=2, datagen_params=dict(elastic_alpha=30.))
    with pytest.raises(ValueError, match='elastic_sigma'):
        _light_executor(bad).get_data_generator(train_images=imgs)


# ---- host: the flow through the stand-ins ------------------------------------------------------------------------------------------------
def _gathers(calls):
    return [c for c in calls if c[0].endswith('_gather')]


@pytest.mark.parametrize('shift', [0., 0.2], ids=['one-stream', 'channel-shift'])
def test_flow_with_elastic_draws_what_the_flow_without_draws(standin, shift):
    """same rows and matrices, the same global RNG state after every next(), one field per batch keyed by 0, 1, 2, ... and handed to every
    array of the batch -- also where the channel shift gives image and masks their own matrices"""
    from multimodal_segmentation_amd.utils.augment import AugmentFlow
    n, H, W, B, seed = 7, 20, 24, 3, 6
    img, msk = _smooth(n, H, W, 1, 1), (_smooth(n, H, W, 4, 2) > 0).astype(np.float32)
    base = dict(BASE, channel_shift_range=shift)
    on = AugmentFlow([img, msk], B, seed, 'cpu', dict(base, elastic_alpha=40., elastic_sigma=3., elastic_seed=21))
    off = AugmentFlow([img, msk], B, seed, 'cpu', base)
    assert off.elastic is None and on.elastic == (40., 3., 1., 21)
    for k in range(4):
        del standin[:]
        a, m = next(on)
        state_on = np.random.get_state()
        calls_on = list(standin)
        del standin[:]
        a0, m0 = next(off)
        state_off = np.random.get_state()
        calls_off = list(standin)
        assert all(np.array_equal(p, q) for p, q in zip(state_on, state_off))
        assert [c[0] for c in calls_on] == ['mmseg_elastic_field'] + ['mmseg_elastic_gather'] * 2
        assert [c[0] for c in calls_off] == ['mmseg_augment_gather'] * 2
        (scale, _, disp, _, fseed, fbatch, fB, fH, fW, fR), = [c[1] for c in calls_on if c[0] == 'mmseg_elastic_field']
        nb = a.shape[0]
        assert (fseed, fbatch, fB, fH, fW, fR) == (21, k, nb, H, W, 12) and scale.dtype == torch.float64
        assert np.array_equal(scale.numpy(), np.full(nb, 40.))
        for g_on, g_off in zip(_gathers(calls_on), _gathers(calls_off)):
            assert g_on[1][3] is disp                                              # the same tensor for the image and the masks
            assert torch.equal(g_on[1][1], g_off[1][1]) and torch.equal(g_on[1][2], g_off[1][2])          # rows, matrices
            assert (g_on[1][4] is None) == (g_off[1][3] is None) and (g_on[1][4] is None or torch.equal(g_on[1][4], g_off[1][3]))
        if shift:
            assert not torch.equal(_gathers(calls_on)[0][1][2], _gathers(calls_on)[1][1][2]) or nb == 1
        assert a.shape == a0.shape and m.shape == m0.shape and not torch.equal(a, a0)
        ref = E.gather(img, _gathers(calls_on)[0][1][1].numpy(), _gathers(calls_on)[0][1][2].numpy(),
                       E.field(np.full(nb, 40.), 3., 21, k, H, W), None if not shift else _gathers(calls_on)[0][1][4].numpy())
        assert np.abs(a.numpy() - ref).max() < 1e-5


def test_flow_prob_draw_excludes_samples_with_a_zero_scale(standin):
    """scale[b] = alpha where the host's Philox word falls below prob, else 0; the default seed of the elastic stream is the flow's; an
    excluded sample is the plain affine sample"""
    from multimodal_segmentation_amd.utils.augment import AugmentFlow, elastic_scales
    n, H, W, B, seed = 8, 16, 18, 8, 3
    img = _smooth(n, H, W, 2, 5)
    on = AugmentFlow([img], B, seed, 'cpu', dict(BASE, elastic_alpha=25., elastic_sigma=2., elastic_prob=0.5))
    off = AugmentFlow([img], B, seed, 'cpu', BASE)
    seen = []
    for k in range(3):
        del standin[:]
        a = next(on).numpy()
        scale = [c[1][0] for c in standin if c[0] == 'mmseg_elastic_field'][0].numpy()
        assert [c[1][4:6] for c in standin if c[0] == 'mmseg_elastic_field'] == [(seed, k)]
        a0 = next(off).numpy()
        want = E.scales(25., 0.5, seed, k, B)
        assert np.array_equal(scale, want) and np.array_equal(elastic_scales(25., 0.5, seed, k, B), want)
        for b in range(B):
            assert (np.abs(a[b] - a0[b]).max() < 1e-5) == (want[b] == 0) and (want[b] == 0 or np.abs(a[b] - a0[b]).max() > 1e-2)
        seen += list(want)
    assert set(seen) == {0., 25.} and 6 <= seen.count(0.) <= 18
    assert np.array_equal(elastic_scales(25., 1.0, seed, 0, B), np.full(B, 25.))
    assert np.array_equal(elastic_scales(25., 0.0, seed, 0, B), np.zeros(B))


def test_ops_refuse_host_tensors_and_bad_arguments():
    """without the stand-ins: host tensors raise like every op; a sigma outside the kernel's radii and a field of the wrong shape raise"""
    from multimodal_segmentation_amd import _native, ops
    scale = torch.ones(2, dtype=torch.float64)
    with pytest.raises(_native.NativeLibraryError, match='device tensors'):
        ops.elastic_field(scale, 2.0, 1, 0, 8, 8)
    x, mat = torch.zeros(2, 8, 8, 1), torch.tensor([[1., 0., 0., 0., 1., 0.]] * 2, dtype=torch.float64)
    with pytest.raises(_native.NativeLibraryError, match='device tensors'):
        ops.elastic_gather(x, None, mat, torch.zeros(2, 8, 8, 2))
    for sigma in (0.1, 32.2, 0., -1.):
        with pytest.raises(ValueError, match='elastic_field'):
            ops.elastic_field(scale, sigma, 1, 0, 8, 8)
    with pytest.raises(ValueError, match='disp'):
        ops.elastic_gather(x, None, mat, torch.zeros(2, 8, 8))
    with pytest.raises(ValueError, match='fill_mode'):
        ops.elastic_gather(x, None, mat, torch.zeros(2, 8, 8, 2), fill_mode='mirror')
    assert ops._i32(0xfedcba98) == 0xfedcba98 - 2 ** 32 and ops._i32(-1) == -1 and ops._i32(2 ** 32 + 5) == 5


def test_entry_points_declared_and_bad_arguments_refused():
    """every new prototype uses types the binder knows and is exported; R = 129, R = 0 and unusable shapes return hipErrorInvalidValue,
    B = 0 returns 0, and none of them launches anything (the pointers are never dereferenced)"""
    from multimodal_segmentation_amd import _native
    protos = _native.parse_header()
    for name in E.STANDINS:
        assert name in protos and all(t in _native._CTYPES for t in protos[name][1]), name
    assert protos['mmseg_elastic_field'][1] == ['const double*', 'const double*', 'float*', 'double*'] + ['int'] * 6 + ['void*']
    aug, ela = protos['mmseg_augment_gather'][1], protos['mmseg_elastic_gather'][1]
    assert ela == aug[:3] + ['const float*'] + aug[3:]
    _native.build()
    lib = _native.load()
    run, query, gather = lib.mmseg_elastic_field, lib.mmseg_elastic_workspace_doubles, lib.mmseg_elastic_gather
    ptrs, bad = [8, 16, 24, 32], 1
    assert run(*(ptrs + [1, 0, 2, 8, 8, 129, None])) == bad
    assert run(*(ptrs + [1, 0, 2, 8, 8, 0, None])) == bad
    assert run(*(ptrs + [1, 0, 2, 8, 8, -3, None])) == bad
    assert run(*(ptrs + [1, 0, 0, 8, 8, 129, None])) == bad          # the radius is checked before the empty batch
    assert run(*(ptrs + [1, 0, 0, 8, 8, 128, None])) == 0
    assert run(*(ptrs + [1, 0, 0, 8, 8, 1, None])) == 0
    for B, H, W in ((2, 0, 8), (2, 8, 0), (65536, 8, 8), (2, 65536, 8), (2, 32768, 32768)):
        assert run(*(ptrs + [1, 0, B, H, W, 4, None])) == bad, (B, H, W)
        assert query(B, H, W) == 0
    for i in range(4):
        p = list(ptrs)
        p[i] = None
        assert run(*(p + [1, 0, 2, 8, 8, 4, None])) == bad
    assert query(8, 256, 256) == 2 * 8 * 256 * 256 and query(3, 5, 7) == 210 and query(0, 8, 8) == 0
    args = [8, 16, 24, 32, None, 40, None, 4]          # data, rows, mat, disp, shift, out, ws, N
    assert gather(*(args + [0, 8, 8, 1, 1, 0, 0.0, None])) == 0
    no_field = list(args)
    no_field[3] = None
    assert gather(*(no_field + [2, 8, 8, 1, 1, 0, 0.0, None])) == bad
    for tail in ([2, 0, 8, 1, 1, 0], [2, 8, 8, 0, 1, 0], [2, 8, 8, 1, 2, 0], [2, 8, 8, 1, 1, 4], [65536, 8, 8, 1, 1, 0]):
        assert gather(*(args + tail + [0.0, None])) == bad, tail


def test_elastic_bench_tool_is_importable():
    """tools/elastic_bench.py refuses to time anything without a GPU, and says so"""
    import importlib.util
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location('elastic_bench', os.path.join(root, 'tools', 'elastic_bench.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    assert callable(mod.main) and mod.SIGMAS == (4.0, 8.0, 32.0) and mod.CHANNELS == (1, 4)
    if not torch.cuda.is_available():
        with pytest.raises(SystemExit, match='GPU'):
            mod.main([])


# ---- device: the field --------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize('seed,batch', SEEDS)
@pytest.mark.parametrize('H,W,sigma', FIELD_SHAPES, ids=['5x7-R12', '37x30-R10', '40x33-R128', 'tiles'])
def test_field_matches_restatement(H, W, sigma, seed, batch):
    """|got - ref| <= 2^-23 |ref| + 1e-12 |scale|: one fp32 rounding plus a tie flipped by fp64 noise, and 16 x the 6e-14 bound on two
    257-term fp64 sums of products bounded by 1.  The sample with scale 0 is +0.0 exactly; a second run gives the same bits."""
    from multimodal_segmentation_amd import ops as P
    scale = np.array(SCALES, np.float64)
    ref = E.field64(scale, sigma, seed, batch, H, W)
    got_d = P.elastic_field(_dev(scale), sigma, seed, batch, H, W)
    again = P.elastic_field(_dev(scale), sigma, seed, batch, H, W)
    torch.cuda.synchronize()
    assert got_d.dtype == torch.float32 and tuple(got_d.shape) == (3, H, W, 2)
    got = got_d.cpu().numpy()
    assert np.array_equal(got.view(np.uint32), again.cpu().numpy().view(np.uint32))
    assert np.array_equal(got[1].view(np.uint32), np.zeros((H, W, 2), np.uint32))
    excess = np.abs(got.astype(np.float64) - ref) - (2.0 ** -23 * np.abs(ref) + 1e-12 * np.abs(scale)[:, None, None, None])
    print('field %dx%d sigma %g: max |got - ref| %.3e, worst excess over the bar %.3e, rms %.3f px'
          % (H, W, sigma, np.abs(got - ref).max(), excess.max(), np.sqrt((ref[0] ** 2).mean())))
    assert excess.max() <= 0
    assert np.abs(ref[0]).max() > 0.05 and not np.array_equal(got[0, ..., 0], got[0, ..., 1])
    other = P.elastic_field(_dev(scale), sigma, seed, batch + 1, H, W).cpu().numpy()
    assert not np.array_equal(other[0], got[0])


# ---- device: the gather -------------------------------------------------------------------------------------------------------------------
def _gather_case(H, W, C, order, seed=0):
    x = _smooth(4, H, W, C, seed) if order == 1 else np.random.RandomState(seed).rand(4, H, W, C).astype(np.float32)
    rows = np.array([3, 0, 2, 1, 3, 0], np.int32)
    mats = np.stack([_folded(dict(matrix=_geom_matrix(g, H, W), hflip=g[6], vflip=g[7]), H, W) for g in _GEOMS])
    disp = E.field(np.full(len(rows), 60.), 3.0, 17, 4, H, W)
    return x, rows, mats, disp


@pytest.mark.gpu
@pytest.mark.parametrize('order', [1, 0])
@pytest.mark.parametrize('fill_mode', ['nearest', 'constant', 'reflect', 'wrap'])
@pytest.mark.parametrize('C', [1, 3, 5])
def test_elastic_gather_matches_restatement(fill_mode, order, C):
    """the geometry cases of tests/test_augment_full.py with a field of sigma 3, alpha 60 (RMS about 4 px), the same fp32 field for the
    kernel and the yardstick; that file's bars"""
    from multimodal_segmentation_amd import ops as P
    H, W = 37, 30
    x, rows, mats, disp = _gather_case(H, W, C, order)
    assert 3. < np.sqrt((disp.astype(np.float64) ** 2).mean()) < 5. and np.abs(disp).max() > 8.
    ref = E.gather(x, rows, mats, disp, None, order, fill_mode, -0.75)
    got = P.elastic_gather(_dev(x), _dev(rows), _dev(mats), _dev(disp), None, order, fill_mode, -0.75).cpu().numpy()
    plain = P.augment_gather(_dev(x), _dev(rows), _dev(mats), None, order, fill_mode, -0.75).cpu().numpy()
    for i in range(len(rows)):
        _check(got[i], ref[i], order)
    assert np.abs(got[0] - plain[0]).max() > 1e-2                              # the field moves the sample (a pure flip without it)


@pytest.mark.gpu
def test_elastic_gather_channel_shift_with_clip():
    from multimodal_segmentation_amd import ops as P
    H, W, C = 41, 29, 5
    x, rows, mats, disp = _gather_case(H, W, C, 1, seed=3)
    shifts = np.random.RandomState(5).uniform(-1.5, 1.5, (len(rows), C)).astype(np.float32)
    unshifted = E.gather(x, rows, mats, disp, None, 1, 'nearest', 0.2)
    exp = E.gather(x, rows, mats, disp, shifts, 1, 'nearest', 0.2)
    for i in range(len(rows)):
        assert (exp[i] == unshifted[i].min()).any() and (exp[i] == unshifted[i].max()).any()          # the clip bites
    a = P.elastic_gather(_dev(x), _dev(rows), _dev(mats), _dev(disp), _dev(shifts), 1, 'nearest', 0.2)
    b = P.elastic_gather(_dev(x), _dev(rows), _dev(mats), _dev(disp), _dev(shifts), 1, 'nearest', 0.2)
    torch.cuda.synchronize()
    assert torch.equal(a, b)
    got = a.cpu().numpy()
    for i in range(len(rows)):
        assert np.abs(got[i] - exp[i]).max() < 2e-5 * max(1.0, np.abs(exp[i]).max())


@pytest.mark.gpu
@pytest.mark.parametrize('fill_mode', ['nearest', 'constant', 'reflect', 'wrap'])
def test_zero_field_is_the_plain_gather_bit_for_bit(fill_mode):
    from multimodal_segmentation_amd import ops as P
    H, W, C = 33, 47, 3
    x = np.random.RandomState(1).standard_normal((3, H, W, C)).astype(np.float32)
    x[0, 0, 0, 0] = -0.0
    rows = np.array([2, 0, 1], np.int32)
    zero = torch.zeros(3, H, W, 2, device='cuda')
    ident = np.tile(np.array([1., 0., 0., 0., 1., 0.]), (3, 1))
    mats = np.stack([_folded(dict(matrix=_geom_matrix(g, H, W), hflip=g[6], vflip=g[7]), H, W) for g in _GEOMS[1:4]])
    shifts = np.random.RandomState(2).uniform(-0.5, 0.5, (3, C)).astype(np.float32)
    for order in (0, 1):
        got = P.elastic_gather(_dev(x), _dev(rows), _dev(ident), zero, None, order, fill_mode, 5.).cpu().numpy()
        assert np.array_equal(got.view(np.uint32), x[rows].view(np.uint32))
        for sh in (None, _dev(shifts)):
            a = P.elastic_gather(_dev(x), _dev(rows), _dev(mats), zero, sh, order, fill_mode, 0.3)
            b = P.augment_gather(_dev(x), _dev(rows), _dev(mats), sh, order, fill_mode, 0.3)
            assert torch.equal(a.view(torch.int32), b.view(torch.int32))


# ---- device: the flow and the executor ----------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_flow_matches_zipped_restated_iterators_composed_with_the_restated_field():
    """rotation + zoom + flips + elastic over 3 batches of an image array (C = 1) and a mask array (C = 4) at 32 x 40: keras' restated draws
    (rows, matrices, flips) composed with the restated field, at the gather's bars; two flows of one seed give the same bits; the global
    RNG is where the flow without elastic leaves it"""
    from multimodal_segmentation_amd.utils.augment import AugmentFlow
    n, H, W, B, seed, alpha, sigma = 7, 32, 40, 3, 10, 40., 3.
    img = _smooth(n, H, W, 1, 1)
    msk = (_smooth(n, H, W, 4, 2) > 0).astype(np.float32)
    flow, twin = (AugmentFlow([img, msk], B, seed, 'cuda', ELASTIC) for _ in range(2))
    plain = AugmentFlow([img, msk], B, seed, 'cuda', BASE)
    o_img, o_msk = KR.NumpyArrayIteratorRef(img, B, seed, BASE), KR.NumpyArrayIteratorRef(msk, B, seed, BASE)
    for k in range(3):
        a, m = next(flow)
        state = np.random.get_state()
        a2, m2 = next(twin)
        assert torch.equal(a, a2) and torch.equal(m, m2)
        next(plain)
        state_plain = np.random.get_state()
        next(o_img), next(o_msk)
        state_ref = np.random.get_state()
        for other in (state_plain, state_ref):
            assert all(np.array_equal(p, q) for p, q in zip(state, other))
        assert np.array_equal(o_img.rows, o_msk.rows)
        nb = len(o_img.rows)
        disp = E.field(E.scales(alpha, 1.0, seed, k, nb), sigma, seed, k, H, W)
        for got, x, it in ((a, img, o_img), (m, msk, o_msk)):
            mats = np.stack([_folded(rec, H, W) for rec in it.records])
            ref = E.gather(x, it.rows, mats, disp, None, 1, 'nearest', 0.)
            assert tuple(got.shape) == ref.shape
            for i in range(nb):
                _check(got[i].cpu().numpy(), ref[i], 1)


@pytest.mark.gpu
def test_dafnet_executor_trains_with_elastic_on():
    from multimodal_segmentation_amd.utils.augment import AugmentFlow
    nn.set_default_device('cuda:0')
    conf = Hh.make_conf(dafnet_config_chaos, 64, batch_size=2, datagen_params=dict(elastic_alpha=30., elastic_sigma=4.))
    np.random.seed(conf.seed)
    torch.manual_seed(conf.seed)
    ex = _executor(conf)
    ex.init_train_data(slices_per_volume=2)
    assert isinstance(ex.gen_labelled, AugmentFlow) and ex.gen_labelled.elastic == (30., 4., 1., conf.seed)
    losses = {k: [] for k in ex.get_loss_names()}
    for _ in range(2):
        ex.train_batch(losses)
    vals = {k: [float(v) for v in vs] for k, vs in losses.items() if vs}
    assert vals and all(np.isfinite(v).all() for v in vals.values())
    assert ex.gen_labelled.elastic_batch == 2


@pytest.mark.gpu
def test_without_the_keys_the_executor_keeps_rotation_flow():
    from multimodal_segmentation_amd.utils.augment import RotationFlow
    nn.set_default_device('cuda:0')
    ex = _executor(Hh.make_conf(dafnet_config_chaos, 64, batch_size=2))
    assert isinstance(ex.get_data_generator(train_images=[np.zeros((3, 64, 64, 1), np.float32)]), RotationFlow)
