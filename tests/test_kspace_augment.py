"""MR k-space artefact augmentation of training batches on the device: mmseg_kspace_forward / _apply / _inverse (csrc/kspace.hip),
ops.kspace_*, the KSPACE_KEYS of conf.datagen_params, kspace_draws / kspace_tables and AugmentFlow (utils/augment.py) against the fp64
numpy.fft restatement in tests/kspace_ref.py."""
import numpy as np
import pytest
import torch

from multimodal_segmentation_amd import nn
from multimodal_segmentation_amd.configuration import dafnet_config_chaos
from tests import elastic_ref as E
from tests import helpers as Hh
from tests import intensity_ref as RI
from tests import kspace_ref as R
from tests.test_augment_full import _executor, _light_executor, _smooth, _standin_augment_gather

SEEDS = ((11, 0), (0xfedcba98, 0x80000003))          # (seed, batch) as tests/test_intensity_augment.py
BASE = dict(rotation_range=20., zoom_range=0.2, horizontal_flip=True, vertical_flip=True)
ALL_ON = dict(motion_shift_max=3., motion_segments=4, ghost_count_range=(2, 4), ghost_intensity_range=(0.2, 0.6),
              gibbs_cutoff_range=(0.4, 0.8), spike_count_max=3, spike_intensity_range=(0.05, 0.2), rician_std_max=0.05)
# (H, W, C) of the transform alone: one radix-2 pass; 4 . 2; radices 4 . 3 and 2 . 5; no factor 2; three channels; 192 rows of 24 columns
# in three tiles of 8; the length limit on either axis, with the narrowest column tile (2 columns at H = 1024); W = 27 is no multiple of
# the 16-column tile of H = 40
FFT_SHAPES = ((2, 2, 1), (8, 8, 1), (12, 10, 1), (9, 25, 1), (30, 16, 3), (192, 24, 1), (1024, 6, 1), (6, 1024, 1), (40, 27, 1))
OP_SHAPES = ((12, 10, 1), (48, 40, 1), (30, 16, 3))


def _dev(a):
    return torch.as_tensor(np.ascontiguousarray(a)).to('cuda')


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _row(flags=0, axis=0, breaks=(), shifts=(), n=0, a=0., T=0., spikes=(), std=0.):
    """one table row by hand: spikes = [(u, v, s, phi)] with u, v already reduced mod H, W"""
    t = np.zeros(R.P_COLS)
    t[0], t[1], t[2] = flags, axis, len(breaks)
    t[3:3 + len(breaks)] = breaks
    for i, sh in enumerate(shifts):
        t[10 + 2 * i:12 + 2 * i] = sh
    t[26], t[27], t[28], t[29] = n, 1.0 - a, T, len(spikes)
    for i, (u, v, s, phi) in enumerate(spikes):
        t[30 + 4 * i:34 + 4 * i] = (u, v, s * np.cos(phi), s * np.sin(phi))
    t[46] = std
    return t


@pytest.fixture
def standin(monkeypatch):
    """the CPU stand-ins of the gather, the elastic field, the intensity and the k-space entry points over cpu_backend's table; `calls`
    records every call of a kernel entry point"""
    from tests import cpu_backend as cb
    calls = []

    def recorded(name, fn):
        def run(*args):
            calls.append((name, args))
            return fn(*args)
        return run

    table = dict(E.STANDINS, mmseg_augment_gather=_standin_augment_gather, mmseg_augment_workspace_floats=lambda B, H, W, C: 2 * B)
    table.update(RI.STANDINS)
    table.update(R.STANDINS)
    for name, fn in table.items():
        monkeypatch.setitem(cb._TABLE, name, fn if 'workspace' in name else recorded(name, fn))
    cb.install()
    nn.set_default_device('cpu')
    yield calls
    cb.uninstall()


# ---- host: the dict -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('bad,word', [
    (dict(motion_shift_max=-1.), 'motion_shift_max'), (dict(motion_shift_max='3'), 'motion_shift_max'),
    (dict(motion_shift_max=float('nan')), 'motion_shift_max'), (dict(motion_shift_max=True), 'motion_shift_max'),
    (dict(motion_segments=1), 'motion_segments'), (dict(motion_segments=9), 'motion_segments'), (dict(motion_segments=3.5), 'motion_segments'),
    (dict(motion_prob=1.5), 'motion_prob'), (dict(motion_prob='often'), 'motion_prob'),
    (dict(ghost_count_range=(1, 4), ghost_intensity_range=(0.2, 0.6)), 'ghost_count_range'),
    (dict(ghost_count_range=(4, 2), ghost_intensity_range=(0.2, 0.6)), 'ghost_count_range'),
    (dict(ghost_count_range=(2.5, 4), ghost_intensity_range=(0.2, 0.6)), 'ghost_count_range'),
    (dict(ghost_count_range=3, ghost_intensity_range=(0.2, 0.6)), 'ghost_count_range'),
    (dict(ghost_count_range=(2, 4)), 'ghost_intensity_range'), (dict(ghost_intensity_range=(0.2, 1.0)), 'ghost_intensity_range'),
    (dict(ghost_intensity_range=(-0.1, 0.5)), 'ghost_intensity_range'), (dict(ghost_intensity_range=(0.6, 0.2)), 'ghost_intensity_range'),
    (dict(ghost_prob=-0.1), 'ghost_prob'),
    (dict(gibbs_cutoff_range=(0., 0.5)), 'gibbs_cutoff_range'), (dict(gibbs_cutoff_range=(0.5, 1.1)), 'gibbs_cutoff_range'),
    (dict(gibbs_cutoff_range=0.5), 'gibbs_cutoff_range'), (dict(gibbs_cutoff_range=(0.5, float('nan'))), 'gibbs_cutoff_range'),
    (dict(gibbs_prob=2), 'gibbs_prob'),
    (dict(spike_count_max=5, spike_intensity_range=(0.05, 0.2)), 'spike_count_max'), (dict(spike_count_max=-1), 'spike_count_max'),
    (dict(spike_count_max=1.5, spike_intensity_range=(0.05, 0.2)), 'spike_count_max'), (dict(spike_count_max=2), 'spike_intensity_range'),
    (dict(spike_count_max=2, spike_intensity_range=(0., 0.2)), 'spike_intensity_range'),
    (dict(spike_intensity_range=(0.2, 0.05)), 'spike_intensity_range'), (dict(spike_prob=float('nan')), 'spike_prob'),
    (dict(rician_std_max=-0.1), 'rician_std_max'), (dict(rician_std_max=None), 'rician_std_max'), (dict(rician_prob=1.01), 'rician_prob'),
    (dict(kspace_phase_axis=2), 'kspace_phase_axis'), (dict(kspace_phase_axis='rows'), 'kspace_phase_axis'),
    (dict(kspace_phase_axis=True), 'kspace_phase_axis'), (dict(kspace_phase_axis=0.5), 'kspace_phase_axis'),
    (dict(kspace_seed=1.5), 'kspace_seed'), (dict(kspace_seed=True), 'kspace_seed'),
    (dict(motion_shift=3.), 'unknown datagen parameter'),
])
def test_kspace_keys_validate(bad, word):
    from multimodal_segmentation_amd.utils.augment import (DATAGEN_KEYS, ELASTIC_KEYS, INTENSITY_KEYS, KSPACE_KEYS, check_datagen_params,
                                                           kspace_on, kspace_params, rotation_only)
    assert len(KSPACE_KEYS) == 15 and not set(KSPACE_KEYS) & (set(DATAGEN_KEYS) | set(ELASTIC_KEYS) | set(INTENSITY_KEYS))
    p = dict(rotation_range=20., zoom_range=0)
    for good in (ALL_ON, dict(ALL_ON, kspace_phase_axis='random', kspace_seed=np.int64(4)), dict(motion_shift_max=2, motion_segments=8),
                 dict(ghost_count_range=[2, 2], ghost_intensity_range=np.array([0., 0.])), dict(gibbs_cutoff_range=(1, 1)),
                 dict(spike_count_max=4, spike_intensity_range=(0.1, 0.1), spike_prob=0), dict(rician_std_max=np.float32(0.1)),
                 dict(kspace_phase_axis=1), dict(ghost_intensity_range=(0.2, 0.6))):
        assert check_datagen_params(dict(p, **good)) is not None
    assert check_datagen_params(dict(p, **ALL_ON)) == dict(p, **ALL_ON)
    with pytest.raises(ValueError, match=word):
        check_datagen_params(dict(p, **bad))
    d = kspace_params({}, 7)          # everything off, probabilities 1.0, the flow's seed
    assert d['seed'] == 7 and d['motion_prob'] == d['rician_prob'] == 1.0 and d['motion_shift_max'] == 0 and d['ghost_count'] is None
    assert kspace_params(dict(kspace_seed=3), 7)['seed'] == 3
    off = dict(p, motion_shift_max=0, motion_segments=5, ghost_count_range=None, gibbs_cutoff_range=None, spike_count_max=0,
               rician_std_max=0, kspace_phase_axis='random', kspace_seed=3)
    assert check_datagen_params(off) == off and rotation_only(off) and not kspace_on(off)
    for dead in (dict(motion_shift_max=3., motion_prob=0), dict(rician_std_max=0.1, rician_prob=0.),
                 dict(gibbs_cutoff_range=(0.4, 0.8), gibbs_prob=0)):
        assert rotation_only(dict(p, **dead)) and not kspace_on(dict(p, **dead))
    for keys in (('motion_shift_max',), ('ghost_count_range', 'ghost_intensity_range'), ('gibbs_cutoff_range',),
                 ('spike_count_max', 'spike_intensity_range'), ('rician_std_max',)):
        on = dict(p, **{k: ALL_ON[k] for k in keys})
        assert kspace_on(on) and not rotation_only(on)


# ---- host: the draws ------------------------------------------------------------------------------------------------------------------
def test_kspace_draws_follow_their_probabilities_and_ranges():
    """192 samples per image array (24 batches of 8); an operation of probability p is on in 192 p +- 5 sqrt(192 p (1 - p)) of them
    (5 sigma of the binomial count): [62, 130] at 0.5, [26, 89] at 0.3, [112, 172] at 0.74.  The product's tables are the restatement's."""
    from multimodal_segmentation_amd.utils.augment import kspace_draws, kspace_tables
    H, W = 12, 10
    probs = dict(motion_prob=0.5, ghost_prob=0.3, gibbs_prob=0.74, spike_prob=0.5, rician_prob=0.3)
    params = dict(ALL_ON, kspace_seed=77, kspace_phase_axis='random', **probs)
    state = np.random.get_state()
    tables = [kspace_draws(params, 5, k, 8, 2, H, W) for k in range(24)]
    assert all(np.array_equal(p, q) for p, q in zip(state, np.random.get_state()))          # numpy's global RNG is untouched
    for k, d in enumerate(tables):
        ref = R.draws(params, 5, k, 8, 2, H, W)
        assert set(d) == set(ref)
        for key in ref:
            assert d[key].shape == ref[key].shape and np.array_equal(d[key], ref[key]), (k, key)
        for a in range(2):
            t = kspace_tables(d, a, H, W)
            assert t.shape == (8, 48) and np.array_equal(t, R.table(ref, a, H, W)), (k, a)
    cat = {key: np.concatenate([d[key] for d in tables], axis=1) for key in tables[0]}
    bounds = {0.5: (62, 130), 0.3: (26, 89), 0.74: (112, 172)}
    for a in range(2):
        for key in ('motion', 'ghost', 'gibbs', 'spike', 'rician'):
            lo, hi = bounds[probs[key + '_prob']]
            assert lo <= cat[key][a].sum() <= hi, (key, a, cat[key][a].sum())
        lo, hi = bounds[0.5]
        assert lo <= cat['axis'][a].sum() <= hi and set(cat['axis'][a]) == {0, 1}
        on = cat['motion'][a]
        P = np.where(cat['axis'][a] == 1, W, H)
        br, sh = cat['breaks'][a], cat['shifts'][a]
        assert (np.diff(br, axis=1) >= 0).all() and (br[on] >= 0).all() and (br[on] < P[on, None]).all() and not br[~on].any()
        assert (np.abs(sh) <= 3.0).all() and not sh[~on].any() and np.abs(sh[on]).max() > 2.0
        home = (br <= (P // 2)[:, None]).sum(1)
        assert not sh[np.arange(len(home)), home].any()                                       # the segment of k_p = 0 does not move
        assert ((sh[on] != 0).any(axis=2).sum(axis=1) == 3).all()                             # every other of the 4 segments does
        g = cat['ghost'][a]
        assert set(cat['n'][a][g]) == {2, 3, 4} and not cat['n'][a][~g].any()
        assert (cat['a'][a][g] >= 0.2).all() and (cat['a'][a][g] <= 0.6).all() and np.ptp(cat['a'][a][g]) > 0.2
        gb = cat['gibbs'][a]
        assert (cat['f'][a][gb] >= 0.4).all() and (cat['f'][a][gb] <= 0.8).all() and np.ptp(cat['f'][a][gb]) > 0.2 and not cat['f'][a][~gb].any()
        s = cat['spike'][a]
        assert set(cat['K'][a][s]) == {1, 2, 3} and not cat['K'][a][~s].any()
        sp = cat['spikes'][a]
        used = np.arange(4)[None, :] < cat['K'][a][:, None]
        assert not sp[~used].any()
        assert (sp[used][:, 0] >= -(H // 2)).all() and (sp[used][:, 0] < H - H // 2).all()
        assert (sp[used][:, 1] >= -(W // 2)).all() and (sp[used][:, 1] < W - W // 2).all()
        assert (sp[used][:, 2] >= 0.05).all() and (sp[used][:, 2] <= 0.2).all() and (sp[used][:, 3] >= 0).all() and (sp[used][:, 3] < 2 * np.pi).all()
        r = cat['rician'][a]
        assert (cat['std'][a][r] <= 0.05).all() and cat['std'][a][r].max() > 0.025 and not cat['std'][a][~r].any()
    assert not np.array_equal(cat['f'][0], cat['f'][1])          # one draw per array
    every = kspace_draws(ALL_ON, 5, 0, 8, 2, H, W)
    none = kspace_draws(dict(ALL_ON, motion_prob=0, ghost_prob=0, gibbs_prob=0, spike_prob=0, rician_prob=0), 5, 0, 8, 2, H, W)
    for key in ('motion', 'ghost', 'gibbs', 'spike', 'rician'):
        assert every[key].all() and not none[key].any()
    assert kspace_tables(none, 0, H, W) is None and not every['axis'].any() and kspace_draws(dict(ALL_ON, kspace_phase_axis=1), 5, 0, 8, 2, H, W)['axis'].all()
    assert np.array_equal(kspace_draws(ALL_ON, 5, 3, 8, 1, H, W)['f'], kspace_draws(dict(ALL_ON, kspace_seed=5), 9, 3, 8, 1, H, W)['f'])
    assert not np.array_equal(kspace_draws(ALL_ON, 5, 3, 8, 1, H, W)['f'], kspace_draws(ALL_ON, 5, 4, 8, 1, H, W)['f'])


# ---- host: the restated rule on inputs one can check by hand -----------------------------------------------------------------------------
def test_restated_rule_by_hand():
    H, W = 8, 12
    r, c = np.meshgrid(np.arange(H), np.arange(W), indexing='ij')
    # a single spike on an empty spectrum is a cosine of amplitude 2 A / (H W)
    A, ky, kx, s, phi = 5.0, -3, 2, 1.0, 0.7
    X = R.rule(np.zeros((1, H, W), complex), _row(8, spikes=[(ky % H, kx % W, s, phi)]), A)
    assert np.count_nonzero(X) == 2
    z = np.fft.ifft2(X[0])
    assert np.abs(z.imag).max() < 1e-15
    assert np.abs(z.real - 2 * A / (H * W) * np.cos(2 * np.pi * (ky * r / H + kx * c / W) + phi)).max() < 1e-15
    # a spike that is its own mirror (DC, or the Nyquist corner of even extents) gets both adds: 2 A cos(phi)
    for u, v in ((0, 0), (H // 2, W // 2)):
        X = R.rule(np.zeros((1, H, W), complex), _row(8, spikes=[(u, v, s, phi)]), A)
        assert np.count_nonzero(X) == 1 and abs(X[0, u, v] - 2 * A * np.cos(phi)) < 1e-15
    # gibbs with f = 1 on an even square keeps the inscribed circle ky^2 + kx^2 <= (n / 2)^2, its rim included
    n = 8
    X = R.rule(np.ones((1, n, n), complex), _row(4, T=1.0 * 1.0 * (n * n * n * n)), 0.)
    ky2, kx2 = np.meshgrid(R.freqs(n), R.freqs(n), indexing='ij')
    assert np.array_equal(X[0] != 0, ky2 ** 2 + kx2 ** 2 <= (n // 2) ** 2)
    assert X[0, n // 2, 0] == 1 and X[0, n // 2, 1] == 0 and X[0, 3, 3] == 0 and X[0, 2, 3] == 1
    assert list(R.freqs(8)) == [0, 1, 2, 3, -4, -3, -2, -1] and list(R.freqs(5)) == [0, 1, 2, -2, -1]
    # ... and on H x W the inscribed ellipse (ky / (H/2))^2 + (kx / (W/2))^2 <= f^2
    f = 0.6
    X = R.rule(np.ones((1, H, W), complex), _row(4, T=f * f * (H * H * W * W)), 0.)
    kyr, kxr = np.meshgrid(R.freqs(H), R.freqs(W), indexing='ij')
    assert np.array_equal(X[0] != 0, (kyr / (H / 2)) ** 2 + (kxr / (W / 2)) ** 2 <= f * f + 1e-12)
    # motion with zero shifts is the identity, bit for bit; with one shift for every line it is a circular translation
    rs = np.random.RandomState(0)
    y = rs.uniform(0, 2, (1, H, W))
    X0 = np.fft.fft2(y, axes=(1, 2))
    assert np.array_equal(R.rule(X0, _row(1, breaks=(2, 5, 6), shifts=[(0, 0)] * 4), 0.), X0)
    for axis in (0, 1):
        X = R.rule(X0, _row(1, axis=axis, breaks=(0,), shifts=[(0, 0), (2.0, -3.0)]), 0.)          # break 0: every line is segment 1
        assert np.abs(np.fft.ifft2(X, axes=(1, 2)) - np.roll(y, (2, -3), axis=(1, 2))).max() < 1e-14
    # segments: lines k_p + floor(P/2) below the break keep their values, the others turn
    X = R.rule(X0, _row(1, axis=0, breaks=(H // 2 + 1,), shifts=[(0, 0), (1.0, 0.)]), 0.)
    same = R.freqs(H) + H // 2 < H // 2 + 1
    assert np.array_equal(X[0, same], X0[0, same]) and not np.isclose(X[0, ~same], X0[0, ~same]).all()
    # ghosting: every n-th line but k_p = 0 is scaled by 1 - a
    for axis, k in ((0, kyr), (1, kxr)):
        X = R.rule(np.ones((1, H, W), complex), _row(2, axis=axis, n=3, a=0.25), 0.)
        assert np.array_equal(X[0].real, np.where((k % 3 == 0) & (k != 0), 0.75, 1.0))
    # the restated image: magnitude about the minimum; a Rician draw of std 0 changes nothing
    x = rs.uniform(-1, 1, (H, W, 2)).astype(np.float32)
    X, lo = R.spectrum(x)
    img, _ = R.image(X, lo, R.rician_draw(3, 4, 0, 0, H, W, 2, 0.0))
    assert lo == x.min() and np.abs(img - x).max() <= 2.0 ** -23


@pytest.mark.parametrize('seed,batch', SEEDS)
def test_restated_rician_draw_is_a_complex_normal(seed, batch):
    """4096 complex draws of std 1: |mean| < 0.08 and |var - 1| < 0.11 per part (5 standard errors: 5 / sqrt(4096), 5 sqrt(2 / 4096)),
    |correlation| < 0.08; counter word 3 = 5 keeps them apart from the intensity noise (3)"""
    z = R.rician_draw(seed, batch, 1, 0, 64, 64, 1, 1.0)
    for part in (z.real, z.imag):
        assert np.isfinite(part).all() and abs(part.mean()) < 0.08 and abs(part.var() - 1) < 0.11
    assert abs((z.real * z.imag).mean()) < 0.08
    assert not np.array_equal(z.real[0], RI.normals(seed, batch, 1, 0, 64, 64, 1)[..., 0])
    assert not np.array_equal(z, R.rician_draw(seed, batch, 1, 1, 64, 64, 1, 1.0))


# ---- host: the flow through the stand-ins ------------------------------------------------------------------------------------------------
def test_flow_changes_images_only_runs_first_and_counts_batches(standin):
    """two image arrays and a mask array with the k-space AND the intensity keys on: the masks and the global RNG are those of the flow
    without the keys, every image array gets its own draws, the k-space launches of the batch precede the intensity ones, whose statistics
    are taken on the k-space output, and both batch counters reach the kernels in order"""
    from multimodal_segmentation_amd.utils.augment import AugmentFlow
    n, H, W, B, seed = 7, 20, 24, 3, 6
    t1, t2, msk = _smooth(n, H, W, 1, 1), _smooth(n, H, W, 1, 4), (_smooth(n, H, W, 4, 2) > 0).astype(np.float32)
    inten = dict(contrast_range=(0.75, 1.25), noise_std_max=0.05, intensity_seed=21)
    params = dict(BASE, kspace_seed=33, **ALL_ON)
    on = AugmentFlow([t1, t2, msk], B, seed, 'cpu', dict(params, **inten), n_images=2)
    konly = AugmentFlow([t1, t2, msk], B, seed, 'cpu', params, n_images=2)
    off = AugmentFlow([t1, t2, msk], B, seed, 'cpu', BASE)
    default = AugmentFlow([t1, t2, msk], B, seed, 'cpu', params)          # n_images = 0: nothing is an image
    assert off.kspace is None and default.kspace is None and on.kspace is not None and on.intensity is not None
    for k in range(3):
        del standin[:]
        a1, a2, m = next(on)
        state_on = np.random.get_state()
        calls_on = list(standin)
        k1, k2, mk = next(konly)
        del standin[:]
        b1, b2, m0 = next(off)
        state_off = np.random.get_state()
        calls_off = [c[0] for c in standin]
        d1, d2, md = next(default)
        assert all(np.array_equal(p, q) for p, q in zip(state_on, state_off))
        assert calls_off == ['mmseg_augment_gather'] * 3
        assert torch.equal(m, m0) and torch.equal(mk, m0) and torch.equal(md, m0) and torch.equal(d1, b1) and torch.equal(d2, b2)
        assert not torch.equal(k1, b1) and not torch.equal(k2, b2) and not torch.equal(k1 - b1, k2 - b2)
        names = [c[0] for c in calls_on]
        assert names[:3] == ['mmseg_augment_gather'] * 3
        assert names[3:13] == ['mmseg_intensity_stats', 'mmseg_kspace_forward', 'mmseg_kspace_apply', 'mmseg_kspace_inverse'] * 2 + \
            ['mmseg_intensity_stats', 'mmseg_intensity_apply']                                  # all of k-space, then the intensity stage
        inverses = [c[1] for c in calls_on if c[0] == 'mmseg_kspace_inverse']
        assert [(c[5], c[6], c[7]) for c in inverses] == [(33, k, 0), (33, k, 1)]
        assert [(c[1][4], c[1][5], c[1][6]) for c in calls_on if c[0] == 'mmseg_intensity_apply'] == [(21, k, 0), (21, k, 1)]
        nb = a1.shape[0]
        d = R.draws(params, seed, k, nb, 2, H, W)
        di = RI.draws(inten, seed, k, nb, 2)
        for a, (got, mid, plain) in enumerate(((a1, k1, b1), (a2, k2, b2))):
            t = R.table(d, a, H, W)
            assert np.array_equal([c[1] for c in calls_on if c[0] == 'mmseg_kspace_apply'][a][1].numpy(), t)
            ref, _ = R.augment(plain.numpy(), t, 33, k, a)
            assert np.abs(mid.numpy() - ref).max() < 1e-5 and np.abs(ref - plain.numpy()).max() > 0.02
            after, _ = RI.augment(mid.numpy(), di, a, 21, k)          # the intensity stage measured and changed the k-space output
            assert np.abs(got.numpy() - after).max() < 1e-5
    assert on.kspace_batch == 3 and on.intensity_batch == 3 and konly.kspace_batch == 3 and off.kspace_batch == 0


def test_flow_skips_the_launches_nothing_needs(standin):
    """only Rician noise at probability 0.5: a batch in which no sample is flagged launches nothing but the gather, and a sample with
    nothing on is the gathered sample bit for bit"""
    from multimodal_segmentation_amd.utils.augment import AugmentFlow
    n, H, W, B, seed = 8, 12, 10, 2, 3
    img = _smooth(n, H, W, 2, 5)
    params = dict(BASE, rician_std_max=0.2, rician_prob=0.5)
    on, off = AugmentFlow([img], B, seed, 'cpu', params, n_images=1), AugmentFlow([img], B, seed, 'cpu', BASE)
    seen = []
    for k in range(8):
        del standin[:]
        a, a0 = next(on).numpy(), next(off).numpy()
        names = [c[0] for c in standin]
        noisy = R.draws(params, seed, k, B, 1, H, W)['rician'][0]
        assert names.count('mmseg_kspace_forward') == names.count('mmseg_kspace_apply') == names.count('mmseg_kspace_inverse') == \
            names.count('mmseg_intensity_stats') == int(noisy.any())
        for b in range(B):
            assert np.array_equal(_bits(a[b]), _bits(a0[b])) == (not noisy[b])
        seen.append(int(noisy.sum()))
    assert 0 in seen and 2 in seen and on.kspace_batch == 8


def test_flow_refuses_extents_the_transform_cannot_take():
    from multimodal_segmentation_amd.utils.augment import AugmentFlow
    for H, W, word in ((7, 192, 'H = 7'), (2048, 8, 'H = 2048'), (8, 14, 'W = 14')):
        x = np.zeros((2, H, W, 1), np.float32)
        with pytest.raises(ValueError, match=word + '.*2, 3 and 5'):
            AugmentFlow([x], 2, 1, 'cpu', dict(BASE, rician_std_max=0.1), n_images=1)
        assert AugmentFlow([x], 2, 1, 'cpu', dict(BASE, rician_std_max=0.1)).kspace is None          # no image array: nothing to refuse
        assert AugmentFlow([x], 2, 1, 'cpu', dict(BASE, noise_std_max=0.1), n_images=1).kspace is None
    flow = AugmentFlow([np.zeros((2, 192, 1000, 1), np.float32)], 2, 1, 'cpu', dict(BASE, rician_std_max=0.1), n_images=1)
    assert flow.kspace is not None


def test_executor_hands_the_image_count_to_the_flow():
    from multimodal_segmentation_amd.utils.augment import AugmentFlow, RotationFlow
    imgs, msks = [np.zeros((3, 16, 16, 1), np.float32)] * 2, [np.zeros((3, 16, 16, 4), np.float32)]
    on = _light_executor(Hh.make_conf(dafnet_config_chaos, 64, batch_size=2, datagen_params=dict(gibbs_cutoff_range=(0.4, 0.8))))
    gen = on.get_data_generator(train_images=imgs, train_labels=msks)
    assert isinstance(gen, AugmentFlow) and gen.n_images == 2 and gen.kspace is not None and gen.intensity is None
    assert on.get_data_generator(train_labels=msks).kspace is None
    off = _light_executor(Hh.make_conf(dafnet_config_chaos, 64, batch_size=2, datagen_params=dict(gibbs_cutoff_range=None)))
    assert isinstance(off.get_data_generator(train_images=imgs, train_labels=msks), RotationFlow)


def test_ops_refuse_host_tensors_and_bad_arguments():
    from multimodal_segmentation_amd import _native, ops
    x, t, st = torch.zeros(2, 8, 8, 1), torch.zeros(2, 48, dtype=torch.float64), torch.zeros(2, 3, dtype=torch.float64)
    spec = torch.zeros(2, 1, 8, 8, 2, dtype=torch.float64)
    with pytest.raises(_native.NativeLibraryError, match='device tensors'):
        ops.kspace_forward(x, t, st)
    with pytest.raises(_native.NativeLibraryError, match='device tensors'):
        ops.kspace_apply(spec, t, st)
    with pytest.raises(_native.NativeLibraryError, match='device tensors'):
        ops.kspace_inverse(spec, t, st, x, 1, 0, 0)
    with pytest.raises(ValueError, match='table'):
        ops.kspace_forward(x, torch.zeros(2, 47, dtype=torch.float64), st)
    with pytest.raises(ValueError, match='stats'):
        ops.kspace_apply(spec, t, torch.zeros(3, 3, dtype=torch.float64))
    with pytest.raises(ValueError, match='spec'):
        ops.kspace_forward(x, t, st, torch.zeros(2, 8, 8, 1, 2, dtype=torch.float64))
    with pytest.raises(ValueError, match='spec'):
        ops.kspace_inverse(spec.float(), t, st, x, 1, 0, 0)
    with pytest.raises(ValueError, match='spec'):
        ops.kspace_apply(spec[..., 0], t, st)
    with pytest.raises(ValueError, match='fp32'):
        ops.kspace_forward(x.double(), t, st)
    with pytest.raises(ValueError, match='limits'):
        ops.kspace_forward(torch.zeros(2, 7, 8, 1), t, st)
    with pytest.raises(ValueError, match='2, 3 and 5'):
        ops.kspace_twiddles(8, 22, 'cpu')
    tw = ops.kspace_twiddles(12, 10, 'cpu')
    assert tw is ops.kspace_twiddles(12, 10, 'cpu') and tuple(tw.shape) == (22, 2) and tw.dtype == torch.float64          # kept per (H, W, device)
    k = np.arange(10)
    assert np.array_equal(tw[12:].numpy(), np.stack([np.cos(2 * np.pi * k / 10), np.sin(2 * np.pi * k / 10)], axis=1))
    assert [n for n in range(1, 41) if ops.kspace_extent_ok(n)] == [2, 3, 4, 5, 6, 8, 9, 10, 12, 15, 16, 18, 20, 24, 25, 27, 30, 32, 36, 40]
    assert ops.kspace_extent_ok(1024) and ops.kspace_extent_ok(192) and not ops.kspace_extent_ok(1080) and not ops.kspace_extent_ok(1025)
    assert ops.KSPACE_FLAGS == R.FLAGS and ops.KSPACE_PARAMS == R.P_COLS


def test_entry_points_declared_and_bad_arguments_refused():
    """every new prototype uses types the binder knows and is exported; unusable shapes and null pointers return hipErrorInvalidValue,
    B = 0 returns 0, and none of them launches anything (the pointers are never dereferenced)"""
    from multimodal_segmentation_amd import _native
    protos = _native.parse_header()
    for name in R.STANDINS:
        assert name in protos and all(t in _native._CTYPES for t in protos[name][1]), name
    assert 'kspace.hip' in _native.SOURCES
    assert protos['mmseg_kspace_forward'][1] == ['const float*'] + ['const double*'] * 3 + ['double*'] + ['int'] * 4 + ['void*']
    assert protos['mmseg_kspace_apply'][1] == ['double*', 'const double*', 'const double*'] + ['int'] * 4 + ['void*']
    assert protos['mmseg_kspace_inverse'][1] == ['double*'] + ['const double*'] * 3 + ['float*'] + ['int'] * 7 + ['void*']
    _native.build()
    lib = _native.load()
    query, fwd, run, inv = lib.mmseg_kspace_workspace_doubles, lib.mmseg_kspace_forward, lib.mmseg_kspace_apply, lib.mmseg_kspace_inverse
    bad = 1
    assert query(8, 256, 256, 1) == 2 * 8 * 256 * 256 and query(3, 2, 2, 1) == 24 and query(2, 1024, 6, 3) == 2 * 2 * 3 * 1024 * 6
    assert query(0, 8, 8, 1) == 0
    for B, H, W, C in ((2, 7, 192, 1), (2, 2048, 8, 1), (2, 8, 1, 1), (2, 0, 8, 1), (2, 8, 14, 1), (2, 8, 8, 0), (65536, 8, 8, 1),
                       (300, 8, 8, 300), (-1, 8, 8, 1), (2, 1080, 8, 1)):
        assert query(B, H, W, C) == 0
        if B > 0:
            assert fwd(16, 32, 48, 64, 80, B, H, W, C, None) == bad and run(16, 32, 48, B, H, W, C, None) == bad
            assert inv(16, 32, 48, 64, 80, 1, 0, 0, B, H, W, C, None) == bad
    assert fwd(16, 32, 48, 64, 80, 0, 8, 8, 1, None) == 0 and run(16, 32, 48, 0, 8, 8, 1, None) == 0
    assert inv(16, 32, 48, 64, 80, 1, 0, 0, 0, 8, 8, 1, None) == 0
    for i in range(5):
        p = [16, 32, 48, 64, 80]
        p[i] = None
        assert fwd(*(p + [2, 8, 8, 1, None])) == bad and inv(*(p + [1, 0, 0, 2, 8, 8, 1, None])) == bad
    for i in range(3):
        p = [16, 32, 48]
        p[i] = None
        assert run(*(p + [2, 8, 8, 1, None])) == bad
    assert fwd(16, 32, 48, 64, 88, 2, 8, 8, 1, None) == bad and fwd(16, 32, 48, 72, 80, 2, 8, 8, 1, None) == bad          # 16-byte alignment
    assert run(24, 32, 48, 2, 8, 8, 1, None) == bad and inv(24, 32, 48, 64, 80, 1, 0, 0, 2, 8, 8, 1, None) == bad


def test_kspace_bench_tool_is_importable():
    """tools/kspace_bench.py refuses to time anything without a GPU, and says so"""
    import importlib.util
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location('kspace_bench', os.path.join(root, 'tools', 'kspace_bench.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    assert callable(mod.main) and [name for name, _ in mod.CASES] == ['motion', 'ghost', 'gibbs', 'spike', 'rician', 'all']
    assert mod.BYTES_PER_PIXEL == 4 + 8 * 16 + 4
    if not torch.cuda.is_available():
        with pytest.raises(SystemExit, match='GPU'):
            mod.main([])


def test_lds_layout_enumeration_says_what_the_kernel_header_says():
    """tools/kspace_lds_check.py under the guide's bank rule: every read of every pass is conflict-free; the stores of the passes along H
    are conflict-free for H <= 256 (tiles of 16 and 8 columns), 2-way in the first pass of a 4-column tile and 4-way in the first pass of
    a 2-column tile; along W 4-way in a first radix-4 pass, 2-way while Ns < 8"""
    import importlib.util
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location('kspace_lds_check', os.path.join(root, 'tools', 'kspace_lds_check.py'))
    K = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(K)
    assert [K.tile_columns(h) for h in (2, 128, 129, 256, 257, 512, 513, 1024)] == [16, 16, 8, 8, 4, 4, 2, 2]
    assert K.radices(192) == [4, 4, 4, 3] and K.radices(250) == [2, 5, 5, 5] and K.radices(1024) == [4] * 5
    for N in (6, 12, 40, 100, 128, 192, 256, 360, 512, 1024):
        along_h, along_w = K.check(N, K.tile_columns(N), 256), K.check(N, 1, 64)
        assert all(rd == 1 for _, _, rd, _ in along_h + along_w), N
        if N <= 256:
            assert all(wr == 1 for _, _, _, wr in along_h), N
        assert all(wr == 1 for _, Ns, _, wr in along_h if Ns >= 4) and all(wr == 1 for _, Ns, _, wr in along_w if Ns >= 8), N
    assert [wr for _, _, _, wr in K.check(512, 4, 256)] == [2, 1, 1, 1, 1] and [wr for _, _, _, wr in K.check(1024, 2, 256)] == [4, 1, 1, 1, 1]
    assert [wr for _, _, _, wr in K.check(256, 1, 64)] == [4, 2, 1, 1]


# ---- device: the transform alone ------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize('H,W,C', FFT_SHAPES, ids=['%dx%dx%d' % s for s in FFT_SHAPES])
def test_forward_matches_numpy_fft2(H, W, C):
    """mmseg_kspace_forward against numpy.fft.fft2 of x - lo in fp64, B = 3 with the middle sample's flags 0: its slot of the spectrum keeps
    a sentinel.  The bar (kspace_ref): C_FFT eps64 log2(H W) ||y||_2 on the root mean square of the error, which is what Higham's bound
    gives, and on every element.  Two runs are bitwise equal.  Then the inverse of the forward returns the input within one fp32 spacing
    plus E (kspace_ref.image_bound) < 2^-30."""
    from multimodal_segmentation_amd import ops as P
    x = np.random.RandomState(H * W + C).uniform(-1, 1, (3, H, W, C)).astype(np.float32)
    t = np.stack([_row(1), _row(0), _row(16)])          # a flag with nothing to do: the transform alone
    xd, td = _dev(x), _dev(t)
    stats = P.intensity_stats(xd)
    specs = []
    for _ in range(2):
        spec = torch.full((3, C, H, W, 2), 7.25, dtype=torch.float64, device='cuda')
        assert P.kspace_forward(xd, td, stats, spec) is spec
        specs.append(spec.cpu().numpy())
    got = specs[0]
    assert np.array_equal(got.view(np.uint64), specs[1].view(np.uint64))
    assert (got[1] == 7.25).all()
    for b in (0, 2):
        ref, lo = R.spectrum(x[b])
        y = x[b].astype(np.float64) - lo
        err = np.abs(got[b, ..., 0] + 1j * got[b, ..., 1] - ref)
        for ch in range(C):
            bar = R.spectrum_bound(y[..., ch], H, W)
            rms = np.sqrt((err[ch] ** 2).mean())
            print('fft2 %dx%dx%d sample %d channel %d: max |got - ref| %.3e, rms %.3e, bar %.3e' % (H, W, C, b, ch, err[ch].max(), rms, bar))
            assert rms <= bar and err[ch].max() <= bar, (b, ch, err[ch].max(), rms, bar)
        assert np.abs(ref).max() > 1.0
    spec = _dev(got)
    back = xd.clone()
    assert P.kspace_apply(spec, td, stats) is spec
    assert np.array_equal(spec.cpu().numpy().view(np.uint64), got.view(np.uint64))          # zero shifts, and no spectrum flag: untouched
    assert P.kspace_inverse(spec, td, stats, back, 1, 0, 0) is back
    back = back.cpu().numpy()
    assert np.array_equal(_bits(back[1]), _bits(x[1]))
    for b in (0, 2):
        y = x[b].astype(np.float64) - x[b].min()
        E_ = R.image_bound(np.sqrt((y ** 2).sum(axis=(0, 1))).max(), t[b], 0., H, W, 2.0, 0.)
        excess = np.abs(back[b].astype(np.float64) - x[b]) - (np.spacing(np.abs(x[b])).astype(np.float64) + E_)
        print('ifft2(fft2) %dx%dx%d sample %d: max |got - x| %.3e, E %.3e, bit-exact share %.4f'
              % (H, W, C, b, np.abs(back[b] - x[b]).max(), E_, (back[b] == x[b]).mean()))
        assert E_ < 2.0 ** -30 and excess.max() <= 0, (b, excess.max(), E_)


# ---- device: the operations -------------------------------------------------------------------------------------------------------------------
def _device(x, t, seed, batch, a):
    """the product's launches for one image array -> the result (x is left alone)"""
    from multimodal_segmentation_amd import ops as P
    xd, td = _dev(x), _dev(t)
    stats = P.intensity_stats(xd)
    spec = P.kspace_forward(xd, td, stats)
    P.kspace_apply(spec, td, stats)
    out = P.kspace_inverse(spec, td, stats, xd, seed, batch, a)
    assert out is xd
    return xd.cpu().numpy()


def _cases(H, W, axis):
    """table rows per case for samples 0 (on), 2 (on, other values) and 3 (on, a constant sample); sample 1 has nothing on"""
    P = W if axis else H
    T = lambda f: f * f * (H * H * W * W)
    motion = [dict(breaks=(1, P // 2 + 1, P - 1), shifts=[(1.5, -2.25), (0, 0), (-0.75, 3.0), (2.0, 0.5)]),
              dict(breaks=(P // 2,), shifts=[(0.6, 0.4), (0, 0)]), dict(breaks=(0, 0, 2), shifts=[(0, 0), (0, 0), (1, 1), (0, 0)])]
    ghost = [dict(n=2, a=0.5), dict(n=3, a=0.2), dict(n=4, a=0.9)]
    gibbs = [dict(T=T(0.5)), dict(T=T(1.0)), dict(T=T(0.3))]
    spike = [dict(spikes=[(3 % H, (W - 2) % W, 0.2, 0.7), (0, 0, 0.05, 2.0)]), dict(spikes=[(H // 2, W // 2, 0.1, 4.0)] * 4),
             dict(spikes=[(1, 1, 0.15, 0.3)])]
    rician = [dict(std=0.1), dict(std=0.03), dict(std=0.05)]
    one = lambda flag, rows: [dict(flags=flag, axis=axis, **r) for r in rows]
    every = [dict(flags=31, axis=axis, **{k: v for part in parts for k, v in part.items()}) for parts in zip(motion, ghost, gibbs, spike, rician)]
    return dict(motion=one(1, motion), ghost=one(2, ghost), gibbs=one(4, gibbs), spike=one(8, spike), rician=one(16, rician), all=every)


@pytest.mark.gpu
@pytest.mark.parametrize('seed,batch', SEEDS)
@pytest.mark.parametrize('axis', [0, 1])
@pytest.mark.parametrize('H,W,C', OP_SHAPES)
@pytest.mark.parametrize('case', ['motion', 'ghost', 'gibbs', 'spike', 'rician', 'all'])
def test_operations_match_restatement(case, H, W, C, axis, seed, batch):
    """Each operation alone and all together on B = 4 samples with mixed flags, as image array 1 of the batch, on either phase-encode
    axis.  |got - ref| <= one fp32 spacing at the reference value + E (kspace_ref.image_bound), E < 2^-30.  The sample with nothing on
    is the input bit for bit; two runs are bitwise equal."""
    a = 1
    rows = _cases(H, W, axis)[case]
    t = np.stack([_row(**rows[0]), _row(0), _row(**rows[1]), _row(**rows[2])])
    x = np.clip(_smooth(4, H, W, C, 7) * 3, -1, 1)
    x[1, 0, 0, 0] = -0.0
    x[3] = np.float32(0.25)
    got, again = _device(x, t, seed, batch, a), _device(x, t, seed, batch, a)
    assert np.array_equal(_bits(got), _bits(again))
    ref, bound = R.augment(x, t, seed, batch, a)
    assert np.array_equal(_bits(got[1]), _bits(x[1])) and np.array_equal(_bits(ref[1]), _bits(x[1]))
    assert np.isfinite(got).all()
    for b in (0, 2):
        assert np.abs(ref[b] - x[b]).max() > 1e-2
    E_ = (bound - np.spacing(np.abs(ref)).astype(np.float64)).max()
    excess = np.abs(got.astype(np.float64) - ref.astype(np.float64)) - bound
    print('%s %dx%dx%d axis %d seed %#x: max |got - ref| %.3e, E %.3e, worst excess over the bound %.3e, bit-exact share %.5f'
          % (case, H, W, C, axis, seed, np.abs(got - ref).max(), E_, excess.max(), (_bits(got) == _bits(ref)).mean()))
    assert E_ < 2.0 ** -30
    assert excess.max() <= 0
    if case == 'rician':
        assert not np.array_equal(_device(x, t, seed, batch, 0)[0], got[0])          # the array index is in the counter
        assert (got[3] >= 0.25).all() and got[3].max() > 0.26                        # magnitude about the minimum: the noise folds up


# ---- device: the flow and the executor ----------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_flow_end_to_end_on_the_device():
    """two image arrays and two mask arrays at 30 x 32, every k-space operation on at probability 0.6 and a random phase axis: the masks
    are those of the flow without the keys bit for bit, the images are the restatement of that flow's images within the bound where a
    sample is flagged and its bits where not, and a rebuilt flow reproduces every batch bit for bit"""
    from multimodal_segmentation_amd.utils.augment import AugmentFlow
    n, H, W, B, seed = 6, 30, 32, 3, 10
    arrays = [_smooth(n, H, W, 1, 1), _smooth(n, H, W, 1, 2), (_smooth(n, H, W, 4, 3) > 0).astype(np.float32),
              (_smooth(n, H, W, 1, 4) > 0).astype(np.float32)]
    params = dict(BASE, kspace_phase_axis='random', motion_prob=0.6, ghost_prob=0.6, gibbs_prob=0.6, spike_prob=0.6, rician_prob=0.6, **ALL_ON)
    flow, twin = (AugmentFlow(arrays, B, seed, 'cuda', params, n_images=2) for _ in range(2))
    plain = AugmentFlow(arrays, B, seed, 'cuda', BASE, n_images=2)
    flagged, batches = [], []
    for k in range(3):
        out = next(flow)
        state = np.random.get_state()
        again = next(twin)
        base = next(plain)
        assert all(np.array_equal(p, q) for p, q in zip(state, np.random.get_state()))
        assert all(torch.equal(p, q) for p, q in zip(out, again))
        assert torch.equal(out[2], base[2]) and torch.equal(out[3], base[3])
        d = R.draws(params, seed, k, out[0].shape[0], 2, H, W)
        for a in (0, 1):
            t = R.table(d, a, H, W)
            got, x = out[a].cpu().numpy(), base[a].cpu().numpy()
            ref, bound = R.augment(x, t, seed, k, a)
            excess = np.abs(got.astype(np.float64) - ref) - bound
            print('flow batch %d array %d flags %s: max |got - ref| %.3e, worst excess %.3e' % (k, a, t[:, 0], np.abs(got - ref).max(), excess.max()))
            assert excess.max() <= 0
            for b in range(len(t)):
                assert np.array_equal(_bits(got[b]), _bits(x[b])) == (t[b, 0] == 0)
            flagged += list(t[:, 0])
        batches.append(out)
    assert 0 in flagged and len(set(flagged)) > 3 and flow.kspace_batch == 3
    assert not torch.equal(batches[0][0], batches[1][0])


@pytest.mark.gpu
def test_executor_trains_on_kspace_batches():
    """a 64 x 64 DAFNet executor whose conf.datagen_params carries k-space keys: its batches are finite with the masks of the same executor
    without the keys, and train_batch runs on them with finite losses"""
    from multimodal_segmentation_amd.utils.augment import AugmentFlow
    nn.set_default_device('cuda:0')
    imgs, msks = [_smooth(5, 32, 32, 1, 1)], [(_smooth(5, 32, 32, 4, 2) > 0).astype(np.float32)]
    gens = []
    for extra in (dict(ALL_ON), {}):
        ex = _light_executor(Hh.make_conf(dafnet_config_chaos, 64, batch_size=2, datagen_params=dict(horizontal_flip=True, **extra)))
        ex.device = torch.device('cuda:0')
        gens.append(ex.get_data_generator(train_images=imgs, train_labels=msks))
    assert all(isinstance(g, AugmentFlow) for g in gens) and gens[0].n_images == 1 and gens[0].kspace is not None
    for _ in range(2):
        (a, m), (a0, m0) = next(gens[0]), next(gens[1])
        assert torch.isfinite(a).all() and torch.equal(m, m0) and not torch.equal(a, a0)
    conf = Hh.make_conf(dafnet_config_chaos, 64, batch_size=2, datagen_params=dict(ALL_ON))
    np.random.seed(conf.seed)
    torch.manual_seed(conf.seed)
    ex = _executor(conf)
    ex.init_train_data(slices_per_volume=2)
    assert isinstance(ex.gen_labelled, AugmentFlow) and ex.gen_labelled.kspace is not None
    losses = {k: [] for k in ex.get_loss_names()}
    ex.train_batch(losses)
    vals = {k: [float(v) for v in vs] for k, vs in losses.items() if vs}
    assert vals and all(np.isfinite(v).all() for v in vals.values())
    assert ex.gen_labelled.kspace_batch >= 1
