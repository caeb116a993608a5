"""The full ImageDataGenerator pixel surface of the reference's get_datagen_params() (model_executors/base_executor.py:37-78,
103-110) on the device: KerasTransformStream / AugmentFlow (utils/augment.py) and mmseg_augment_gather (csrc/augment.hip)
against the keras 2.1.6 restatement in tests/keras_datagen_ref.py."""
import numpy as np
import pytest
import torch

from multimodal_segmentation_amd import nn
from multimodal_segmentation_amd.configuration import dafnet_config_chaos
from tests import helpers as Hh
from tests import keras_datagen_ref as KR

ALL_KEYS = dict(rotation_range=20., width_shift_range=0.2, height_shift_range=3.5, shear_range=15., zoom_range=(0.8, 1.3),
                channel_shift_range=0.3, fill_mode='reflect', cval=0., horizontal_flip=True, vertical_flip=True)
SINGLE_KEYS = [dict(rotation_range=20.), dict(width_shift_range=0.25), dict(height_shift_range=4.0), dict(shear_range=30.),
               dict(zoom_range=0.2), dict(zoom_range=[0.5, 1.5]), dict(channel_shift_range=0.5), dict(horizontal_flip=True),
               dict(vertical_flip=True)]


def _smooth(n, H, W, C, seed):
    from scipy.ndimage import gaussian_filter
    rs = np.random.RandomState(seed)
    return np.stack([gaussian_filter(rs.standard_normal((H, W, C)), (2, 2, 0)) for _ in range(n)]).astype(np.float32)


def _folded(rec, H, W):
    """the restatement's draws as the product's single matrix: transform (or identity), then the flips as right factors"""
    m = np.eye(3) if rec['matrix'] is None else rec['matrix']
    if rec['hflip']:
        m = m @ np.array([[1, 0, 0], [0, -1, W - 1], [0, 0, 1]])
    if rec['vflip']:
        m = m @ np.array([[-1, 0, H - 1], [0, 1, 0], [0, 0, 1]])
    return m[:2].reshape(6)


def _standin_augment_gather(data, rows, mat, shift, out, ws, N, B, H, W, C, order, fill_mode, cval):
    """test-only CPU stand-in of mmseg_augment_gather: scipy's affine_transform with the kernel's matrix per channel"""
    from scipy import ndimage as ndi
    mode = ('nearest', 'constant', 'reflect', 'wrap')[fill_mode]
    x = data.numpy()
    idx = rows.numpy() if rows is not None else np.arange(B)
    m = mat.numpy().reshape(B, 2, 3)
    res = np.zeros((B, H, W, C), np.float32)
    for b in range(B):
        for c in range(C):
            res[b, ..., c] = ndi.affine_transform(x[idx[b], ..., c], m[b, :, :2], m[b, :, 2], order=order, mode=mode, cval=cval)
        if shift is not None:
            lo, hi = res[b].min(), res[b].max()
            res[b] = np.clip(res[b] + shift[b].numpy()[None, None, :], lo, hi)
    out.copy_(torch.from_numpy(res))
    return 0


@pytest.fixture
def standin(monkeypatch):
    from tests import cpu_backend as cb
    monkeypatch.setitem(cb._TABLE, 'mmseg_augment_gather', _standin_augment_gather)
    monkeypatch.setitem(cb._TABLE, 'mmseg_augment_workspace_floats', lambda B, H, W, C: 2 * B)
    cb.install()
    nn.set_default_device('cpu')
    yield cb
    cb.uninstall()


# ---- host: the draw sequence ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('params', SINGLE_KEYS + [ALL_KEYS], ids=[','.join(sorted(p)) for p in SINGLE_KEYS] + ['all'])
def test_transform_stream_matches_restatement(params):
    """same rows, matrices, flips and channel shifts as keras' iterator, over > 2 passes incl. the short last batch, and the same
    global RNG state after every batch"""
    from multimodal_segmentation_amd.utils.augment import KerasTransformStream
    n, H, W, C, B, seed = 7, 37, 30, 3, 3, 11
    x = _smooth(n, H, W, C, 0)
    stream = KerasTransformStream(n, B, seed, params, H, W, C)
    ref = KR.NumpyArrayIteratorRef(x, B, seed, params)
    sizes = []
    for k in range(7):
        rows, mats, hf, vf, shifts = stream.next()
        z_mine = np.random.standard_normal(4)
        next(ref)
        z_ref = np.random.standard_normal(4)
        assert np.array_equal(rows, ref.rows)
        sizes.append(len(rows))
        for i, rec in enumerate(ref.records):
            assert np.abs(mats[i] - _folded(rec, H, W)).max() < 1e-12, (k, i)
            assert bool(hf[i]) == rec['hflip'] and bool(vf[i]) == rec['vflip']
            if rec['shifts'] is None:
                assert shifts is None
            else:
                assert np.array_equal(shifts[i], rec['shifts'])
        assert np.array_equal(z_mine, z_ref)
    assert sizes == [3, 3, 1, 3, 3, 1, 3]


def test_channel_shift_streams_diverge_per_channel_count(standin):
    """keras' quirk, reproduced: with channel_shift_range != 0 an image (C = 1) and its 4-channel mask consume different numbers of
    draws, so from the second sample of a batch on their geometry differs; the global RNG ends in the LAST array's state"""
    from multimodal_segmentation_amd.utils.augment import AugmentFlow
    n, H, W, B, seed = 6, 24, 20, 3, 4
    p = dict(rotation_range=20., zoom_range=0.1, channel_shift_range=0.2, horizontal_flip=True)
    img = _smooth(n, H, W, 1, 1)
    msk = (_smooth(n, H, W, 4, 2) > 0).astype(np.float32)
    flow = AugmentFlow([img, msk], B, seed, 'cpu', p)
    o_img, o_msk = KR.NumpyArrayIteratorRef(img, B, seed, p), KR.NumpyArrayIteratorRef(msk, B, seed, p)
    for k in range(4):
        a, m = next(flow)
        z_mine = np.random.standard_normal(4)
        ra, rm = next(o_img), next(o_msk)
        z_ref = np.random.standard_normal(4)
        assert np.array_equal(o_img.rows, o_msk.rows)                      # the shuffle is the first draw: shared
        assert np.array_equal(o_img.records[0]['matrix'], o_msk.records[0]['matrix'])
        if len(o_img.records) > 1:
            assert not np.allclose(o_img.records[1]['matrix'], o_msk.records[1]['matrix'])
        assert np.abs(a.numpy() - ra).max() < 1e-4
        assert np.abs(m.numpy() - rm).max() < 1e-4
        assert np.array_equal(z_mine, z_ref)
    # the order of the zip decides the final state: masks first, image last
    flow = AugmentFlow([msk, img], B, seed, 'cpu', p)
    next(flow)
    z_mine = np.random.standard_normal(4)
    o_msk, o_img = KR.NumpyArrayIteratorRef(msk, B, seed, p), KR.NumpyArrayIteratorRef(img, B, seed, p)
    next(o_msk), next(o_img)
    assert np.array_equal(z_mine, np.random.standard_normal(4))


def test_without_channel_shift_one_stream_serves_every_array(standin):
    from multimodal_segmentation_amd.utils.augment import AugmentFlow
    n, H, W, B, seed = 5, 16, 18, 2, 9
    p = dict(ALL_KEYS, channel_shift_range=0., fill_mode='constant', cval=-1.)
    img, msk = _smooth(n, H, W, 1, 3), _smooth(n, H, W, 4, 4)
    flow = AugmentFlow([img, msk], B, seed, 'cpu', p)
    assert len(flow.streams) == 1
    o_img, o_msk = KR.NumpyArrayIteratorRef(img, B, seed, p), KR.NumpyArrayIteratorRef(msk, B, seed, p)
    for k in range(4):
        a, m = next(flow)
        z_mine = np.random.standard_normal(4)
        ra, rm = next(o_img), next(o_msk)
        z_ref = np.random.standard_normal(4)
        assert [r['matrix'] is None for r in o_img.records] == [r['matrix'] is None for r in o_msk.records]
        assert np.abs(a.numpy() - ra).max() < 1e-4 and np.abs(m.numpy() - rm).max() < 1e-4
        assert np.array_equal(z_mine, z_ref)


# ---- host: the dict ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('bad,msg', [
    (dict(rotation_rnage=20.), 'unknown datagen parameter'),
    (dict(brightness_range=(0.5, 1.5)), 'not supported'),
    (dict(featurewise_center=True), 'not supported'),
    (dict(zca_whitening=True), 'not supported'),
    (dict(rescale=1. / 255), 'not supported'),
    (dict(preprocessing_function=abs), 'not supported'),
    (dict(fill_mode='mirror'), 'fill_mode'),
    (dict(width_shift_range=[-2, 0, 2]), 'width_shift_range'),
    (dict(height_shift_range=(0.1, 0.2)), 'height_shift_range'),
    (dict(width_shift_range=3), 'width_shift_range'),
    (dict(zoom_range=(0.5, 1.0, 1.5)), 'zoom_range'),
])
def test_datagen_dict_validation(bad, msg):
    from multimodal_segmentation_amd.utils.augment import check_datagen_params
    p = dict(horizontal_flip=False, vertical_flip=False, rotation_range=20., width_shift_range=0, height_shift_range=0, zoom_range=0)
    check_datagen_params(dict(p))
    check_datagen_params(dict(p, featurewise_center=False, rescale=None, brightness_range=None, data_format='channels_last'))
    with pytest.raises(ValueError, match=msg):
        check_datagen_params(dict(p, **bad))


def _light_executor(conf):
    """the base Executor on a stand-in model: enough for get_data_generator"""
    import types
    from multimodal_segmentation_amd.model_executors.base_executor import Executor
    ex = Executor(conf, types.SimpleNamespace(loader=None))
    ex.device = torch.device('cpu')
    return ex


def _executor(conf):
    from multimodal_segmentation_amd.models.dafnet import DAFNet
    from multimodal_segmentation_amd.model_executors.dafnet_executor import DAFNetExecutor
    model = DAFNet(conf)
    model.build()
    return DAFNetExecutor(conf, model)


def test_executor_with_flips_shifts_and_zoom_builds_generators(standin):
    """an executor whose get_datagen_params() turns on flips, shifts and zoom (the reference's switches) gets AugmentFlow
    generators; conf.datagen_params (build-defined) is merged over the method's dict"""
    from multimodal_segmentation_amd.model_executors.dafnet_executor import DAFNetExecutor
    from multimodal_segmentation_amd.utils.augment import AugmentFlow, RotationFlow

    class Augmenting(DAFNetExecutor):
        def get_datagen_params(self):
            return dict(horizontal_flip=True, vertical_flip=True, rotation_range=20., width_shift_range=0.1,
                        height_shift_range=0.1, zoom_range=0.1)

    from multimodal_segmentation_amd.models.dafnet import DAFNet
    conf = Hh.make_conf(dafnet_config_chaos, 64, batch_size=2)
    model = DAFNet(conf)
    model.build()
    ex = Augmenting(conf, model)
    ex.init_train_data(slices_per_volume=1)
    assert isinstance(ex.gen_labelled, AugmentFlow)
    batch = next(ex.gen_labelled)
    assert len(batch) == 4 and tuple(batch[0].shape) == (2, 64, 64, 1) and tuple(batch[2].shape)[:3] == (2, 64, 64)
    assert all(np.isfinite(t.numpy()).all() for t in batch)
    # the configuration-file route: the default executor with conf.datagen_params
    conf2 = Hh.make_conf(dafnet_config_chaos, 64, batch_size=2, datagen_params=dict(fill_mode='constant', shear_range=10.))
    ex2 = _light_executor(conf2)
    assert ex2.datagen_params()['shear_range'] == 10. and ex2.datagen_params()['rotation_range'] == 20.
    imgs = [np.zeros((3, 64, 64, 1), np.float32)]
    assert isinstance(ex2.get_data_generator(train_images=imgs), AugmentFlow)
    conf3 = Hh.make_conf(dafnet_config_chaos, 64, batch_size=2, datagen_params=dict(fill_mode='wrapped'))
    with pytest.raises(ValueError, match='fill_mode'):
        _light_executor(conf3).get_data_generator(train_images=imgs)
    # the reference's default dict keeps the rotation-only path
    assert isinstance(_light_executor(Hh.make_conf(dafnet_config_chaos, 64, batch_size=2)).get_data_generator(train_images=imgs),
                      RotationFlow)


# ---- device ---------------------------------------------------------------------------------------------------------------------
_GEOMS = [  # (theta deg, tx, ty, shear deg, zx, zy, hflip, vflip)
    (0., 0., 0., 0., 1., 1., True, False),
    (17., -6., 9., 0., 1., 1., False, True),           # whole borders shifted out of the image
    (0., 40., -35.5, 0., 1., 1., False, False),         # beyond the extent: a full wrap / reflection period
    (-12., 2.3, -1.7, 25., 1., 1., True, True),         # shear
    (8., 0., 0., 0., 1.45, 1.3, False, False),          # zoom out
    (0., 0., 0., -10., 0.7, 0.85, True, False),         # zoom in + shear
]


def _geom_matrix(g, H, W):
    th, tx, ty, sh, zx, zy = (np.deg2rad(g[0]), g[1], g[2], np.deg2rad(g[3]), g[4], g[5])
    m = np.array([[np.cos(th), -np.sin(th), 0], [np.sin(th), np.cos(th), 0], [0, 0, 1]])
    m = m @ np.array([[1, 0, tx], [0, 1, ty], [0, 0, 1]]) @ np.array([[1, -np.sin(sh), 0], [0, np.cos(sh), 0], [0, 0, 1]])
    m = m @ np.array([[zx, 0, 0], [0, zy, 0], [0, 0, 1]])
    return KR.transform_matrix_offset_center(m, H, W)


def _geom_case(H, W, C, fill_mode, order, cval, seed=0):
    x = _smooth(4, H, W, C, seed) if order == 1 else np.random.RandomState(seed).rand(4, H, W, C).astype(np.float32)
    rows = np.array([3, 0, 2, 1, 3, 0], np.int32)
    mats, refs = [], []
    for i, g in enumerate(_GEOMS):
        m = _geom_matrix(g, H, W)
        ref = KR.apply_transform(x[rows[i]], m, 2, fill_mode, cval, order)
        if g[6]:
            ref = KR.flip_axis(ref, 1)
        if g[7]:
            ref = KR.flip_axis(ref, 0)
        mats.append(_folded(dict(matrix=m, hflip=g[6], vflip=g[7]), H, W))
        refs.append(ref)
    return x, rows, np.stack(mats), np.stack(refs).astype(np.float32)


def _dev(a):
    return torch.as_tensor(np.ascontiguousarray(a)).to('cuda')


def _check(got, ref, order):
    if order == 1:
        assert np.abs(got - ref).max() < 2e-5 * max(1.0, np.abs(ref).max())
    else:       # nearest tap: fp rounding of the coordinates may pick the other tap exactly at half-way points
        assert (np.abs(got - ref) > 1e-6).mean() < 2e-3


@pytest.mark.gpu
@pytest.mark.parametrize('order', [1, 0])
@pytest.mark.parametrize('fill_mode', ['nearest', 'constant', 'reflect', 'wrap'])
@pytest.mark.parametrize('C', [1, 3, 5])
def test_augment_gather_matches_restatement(fill_mode, order, C):
    from multimodal_segmentation_amd import ops as P
    H, W = 37, 30
    x, rows, mats, refs = _geom_case(H, W, C, fill_mode, order, cval=-0.75)
    got = P.augment_gather(_dev(x), _dev(rows), _dev(mats), None, order, fill_mode, -0.75).cpu().numpy()
    for i in range(len(rows)):
        _check(got[i], refs[i], order)


@pytest.mark.gpu
@pytest.mark.parametrize('fill_mode', ['nearest', 'constant'])
def test_augment_gather_channel_shift_with_clip(fill_mode):
    """random_channel_shift: clip(x_c + s_c, min, max) with min / max of the transformed sample; shifts large enough that the clip
    bites on every sample (checked); two launches give the same bits"""
    from multimodal_segmentation_amd import ops as P
    H, W, C = 41, 29, 5
    x, rows, mats, refs = _geom_case(H, W, C, fill_mode, 1, cval=0.2, seed=3)
    shifts = np.random.RandomState(5).uniform(-1.5, 1.5, (len(rows), C)).astype(np.float32)
    exp = np.stack([np.clip(refs[i] + shifts[i][None, None, :], refs[i].min(), refs[i].max()) for i in range(len(rows))])
    for i in range(len(rows)):
        assert (exp[i] == refs[i].min()).any() and (exp[i] == refs[i].max()).any()
    a = P.augment_gather(_dev(x), _dev(rows), _dev(mats), _dev(shifts), 1, fill_mode, 0.2)
    b = P.augment_gather(_dev(x), _dev(rows), _dev(mats), _dev(shifts), 1, fill_mode, 0.2)
    torch.cuda.synchronize()
    assert torch.equal(a, b)
    got = a.cpu().numpy()
    for i in range(len(rows)):
        assert np.abs(got[i] - exp[i]).max() < 2e-5 * max(1.0, np.abs(exp[i]).max())


@pytest.mark.gpu
@pytest.mark.parametrize('fill_mode', ['nearest', 'constant', 'reflect', 'wrap'])
def test_augment_gather_identity_is_bitwise_and_reproducible(fill_mode):
    from multimodal_segmentation_amd import ops as P
    H, W, C = 33, 47, 3
    x = np.random.RandomState(1).standard_normal((3, H, W, C)).astype(np.float32)
    x[0, 0, 0, 0] = -0.0
    rows = np.array([2, 0, 1], np.int32)
    ident = np.tile(np.array([1., 0., 0., 0., 1., 0.]), (3, 1))
    for order in (0, 1):
        got = P.augment_gather(_dev(x), _dev(rows), _dev(ident), None, order, fill_mode, 5.).cpu().numpy()
        assert np.array_equal(got.view(np.uint32), x[rows].view(np.uint32))
    mats = np.stack([_folded(dict(matrix=_geom_matrix(g, H, W), hflip=g[6], vflip=g[7]), H, W) for g in _GEOMS[:3]])
    a = P.augment_gather(_dev(x), _dev(rows), _dev(mats), None, 1, fill_mode, 0.)
    b = P.augment_gather(_dev(x), _dev(rows), _dev(mats), None, 1, fill_mode, 0.)
    assert torch.equal(a, b)


@pytest.mark.gpu
@pytest.mark.parametrize('params', [ALL_KEYS, dict(ALL_KEYS, channel_shift_range=0., fill_mode='wrap'),
                                    dict(ALL_KEYS, fill_mode='constant', cval=0.5)], ids=['all', 'no-channel-shift', 'constant'])
def test_augment_flow_matches_zipped_restated_iterators(params):
    """AugmentFlow over zipped images + masks: the pixels of zipped keras iterators for 7 batches (> 2 passes, short last batch)
    and the same global RNG state after each"""
    from multimodal_segmentation_amd.utils.augment import AugmentFlow
    n, H, W, B, seed = 7, 32, 28, 3, 10
    img = _smooth(n, H, W, 1, 1)
    msk = (_smooth(n, H, W, 4, 2) > 0).astype(np.float32)
    flow = AugmentFlow([img, msk], B, seed, 'cuda', params)
    o_img, o_msk = KR.NumpyArrayIteratorRef(img, B, seed, params), KR.NumpyArrayIteratorRef(msk, B, seed, params)
    sizes = []
    for k in range(7):
        a, m = next(flow)
        z_mine = np.random.standard_normal(4)
        ra, rm = next(o_img), next(o_msk)
        z_ref = np.random.standard_normal(4)
        assert a.shape == ra.shape and m.shape == rm.shape
        sizes.append(a.shape[0])
        assert np.abs(a.cpu().numpy() - ra).max() < 5e-5
        assert np.abs(m.cpu().numpy() - rm).max() < 2e-3
        assert np.array_equal(z_mine, z_ref)
    assert sizes == [3, 3, 1, 3, 3, 1, 3]


@pytest.mark.gpu
def test_dafnet_executor_trains_with_every_key_on():
    """a 64x64 DAFNet executor with every pixel key on (conf.datagen_params): finite losses over a few train_batch calls, the same
    losses again from the same seed"""
    from multimodal_segmentation_amd.utils.augment import AugmentFlow
    nn.set_default_device('cuda:0')
    runs = []
    for _ in range(2):
        conf = Hh.make_conf(dafnet_config_chaos, 64, batch_size=2, datagen_params=dict(ALL_KEYS, fill_mode='constant'))
        np.random.seed(conf.seed)
        torch.manual_seed(conf.seed)
        ex = _executor(conf)
        ex.init_train_data(slices_per_volume=2)
        assert isinstance(ex.gen_labelled, AugmentFlow)
        losses = {k: [] for k in ex.get_loss_names()}
        for _ in range(3):
            ex.train_batch(losses)
        vals = {k: [float(v) for v in vs] for k, vs in losses.items() if vs}
        assert vals and all(np.isfinite(v).all() for v in vals.values())
        runs.append(vals)
    assert runs[0] == runs[1]


@pytest.mark.gpu
def test_default_dict_keeps_rotation_flow():
    from multimodal_segmentation_amd.utils.augment import RotationFlow
    nn.set_default_device('cuda:0')
    conf = Hh.make_conf(dafnet_config_chaos, 64, batch_size=2)
    ex = _executor(conf)
    assert isinstance(ex.get_data_generator(train_images=[np.zeros((3, 64, 64, 1), np.float32)]), RotationFlow)
