"""Training-batch iterators with the reference's augmentation (model_executors/base_executor.py:37-78,103-110).

The reference wraps every training array in keras `ImageDataGenerator(rotation_range=20., <everything else off>)
.flow(array, batch_size=conf.batch_size, seed=conf.seed)` and zips the iterators, relying on the shared seed to apply
the SAME shuffle and the SAME rotation to images and masks.  Keras 2.1.6 (un-vendored; restated from its published
source, unverifiable here -- see DESIGN.md) does, for batch number k of one iterator:

    np.random.seed(seed + k)                              # the GLOBAL numpy RNG
    if this batch starts a pass: order = np.random.permutation(n)
    rows = order[i*B : (i+1)*B]                           # last batch of a pass may be short
    for each row: theta = deg2rad(np.random.uniform(-20, 20)); rotate about the centre with
                  scipy.ndimage.affine_transform(channel, R, offset, order=1, mode='nearest')

`RotationFlow` draws exactly that stream once per batch (every zipped keras iterator would redraw the identical numbers,
leaving the global RNG in the same state -- which matters, because the executors draw z samples and pool indices from
the global RNG right after `next(gen)`), keeps the arrays resident in HBM and produces the rotated batch with one
`mmseg_affine_gather` launch per array.

`AugmentFlow` does the same for every other pixel key of ImageDataGenerator (shift, shear, zoom, flips, channel shift, fill
modes; `KerasTransformStream` is keras' full random_transform draw sequence) with one `mmseg_augment_gather` launch per array.

Elastic deformation (ELASTIC_KEYS; build-defined, not keras) adds a random smooth displacement field to the coordinates of that
same resampling: one field per batch, computed on the device from (seed, batch number, sample, pixel) and shared by every array.

MR intensity augmentation (INTENSITY_KEYS; build-defined, not keras) then changes the grey values of the IMAGE arrays of the gathered batch
on the device: blur, bias field, contrast, gamma and noise, every image array with its own Philox draws (csrc/intensity.hip).

MR k-space artefacts (KSPACE_KEYS; build-defined, not keras) come between the two: the image arrays of the gathered batch go to their 2-D
spectrum on the device, get motion, ghosting, Gibbs truncation, spikes and Rician noise there and come back as magnitude images
(csrc/kspace.hip); the intensity stage then works on that output.
"""
import numpy as np
import torch

from .. import nn, ops


def rotation_matrices(thetas, H, W):
    """[B,6] fp32 rows (m0..m5): src_row = m0*r + m1*c + m2, src_col = m3*r + m4*c + m5 -- keras' rotation about
    (H/2 + 0.5, W/2 + 0.5) (transform_matrix_offset_center), composed on the host in fp64."""
    thetas = np.asarray(thetas, np.float64)
    cos, sin = np.cos(thetas), np.sin(thetas)
    oh, ow = H / 2.0 + 0.5, W / 2.0 + 0.5
    m = np.stack([cos, -sin, oh - cos * oh + sin * ow, sin, cos, ow - sin * oh - cos * ow], axis=1)
    return m.astype(np.float32)


class KerasFlowStream(object):
    """The (rows, thetas) stream of keras' NumpyArrayIterator(shuffle=True, seed=s) with only rotation enabled."""

    def __init__(self, n, batch_size, seed, rotation_range):
        self.n, self.batch_size, self.seed, self.rotation_range = int(n), int(batch_size), seed, float(rotation_range)
        self.total_batches_seen = 0
        self.batch_index = 0
        self.order = None

    def next(self):
        if self.seed is not None:
            np.random.seed(self.seed + self.total_batches_seen)
        if self.batch_index == 0:
            self.order = np.random.permutation(self.n)
        start = (self.batch_index * self.batch_size) % self.n
        self.batch_index = self.batch_index + 1 if self.n > start + self.batch_size else 0
        self.total_batches_seen += 1
        rows = self.order[start:start + self.batch_size]
        r = self.rotation_range
        thetas = [np.deg2rad(np.random.uniform(-r, r)) if r else 0.0 for _ in rows]
        return rows, np.asarray(thetas, np.float64)


class RotationFlow(object):
    """Iterator over aligned arrays [N,H,W,C_i] -> tuple of rotated device batches [B,H,W,C_i] (a single array yields a
    bare tensor, like the reference's single-generator case)."""

    def __init__(self, arrays, batch_size, seed, device, rotation_range=20., order=1):
        self.device = torch.device(device)
        self.arrays = [a if isinstance(a, torch.Tensor) else
                       torch.as_tensor(np.ascontiguousarray(a, dtype=np.float32)).to(self.device) for a in arrays]
        n = self.arrays[0].shape[0]
        assert all(a.shape[0] == n for a in self.arrays), [tuple(a.shape) for a in self.arrays]
        self.H, self.W = int(self.arrays[0].shape[1]), int(self.arrays[0].shape[2])
        self.stream = KerasFlowStream(n, batch_size, seed, rotation_range)
        self.order = order

    def __iter__(self):
        return self

    def __next__(self):
        rows, thetas = self.stream.next()
        rows_d = nn.host_to_device(rows, self.device, np.int32)
        mat_d = nn.host_to_device(rotation_matrices(thetas, self.H, self.W), self.device, np.float32)
        out = tuple(ops.affine_gather(a, rows_d, mat_d, self.order) for a in self.arrays)
        return out if len(out) > 1 else out[0]

    next = __next__


# ---- the full ImageDataGenerator pixel surface ----------------------------------------------------------------------------------
# keys of keras 2.1.6 ImageDataGenerator(**d) that this pipeline implements (the reference's dict, base_executor.py:103-110, sets
# the first six); brightness_range (PIL), the feature/sample-wise statistics, zca_whitening, rescale and preprocessing_function
# are not on the device path
DATAGEN_KEYS = ('rotation_range', 'width_shift_range', 'height_shift_range', 'shear_range', 'zoom_range', 'channel_shift_range',
                'fill_mode', 'cval', 'horizontal_flip', 'vertical_flip')


# build-defined keys (not keras'): elastic deformation in the Simard 2003 / albumentations convention,
#     displacement = elastic_alpha * gaussian_filter(uniform(-1, 1), elastic_sigma)   per axis, in pixels;
# its RMS is about alpha / (sigma * sqrt(12 pi)) pixels (measured on 64 x 64: 0.0856 alpha at sigma 2, 0.0273 alpha at sigma 8, against
# the formula's 0.0814 and 0.0204 -- the formula neglects the reflecting border, whose share grows with sigma / extent).
#   elastic_alpha  0 (off)          elastic_sigma  required when alpha != 0; int(4 sigma + 0.5) in [1, 128]
#   elastic_prob   1.0: the probability that a sample is deformed          elastic_seed  the flow's seed: seed of the elastic stream
ELASTIC_KEYS = ('elastic_alpha', 'elastic_sigma', 'elastic_prob', 'elastic_seed')


# build-defined keys (not keras'): MR intensity augmentation of the image arrays after the gather, in the spirit of nnU-Net's gamma /
# contrast / noise / blur transforms and TorchIO's RandomBiasField.  Every operation is drawn per sample and per image array and is on
# where its Philox uniform falls below its probability (intensity_draws); the order is blur, bias field, contrast, clip, gamma, noise and
# the sample's minimum, maximum and mean are measured ONCE, before all of them (the definition: include/mmseg_hip.h).  Unlike nnU-Net,
# contrast keeps the mean and gamma the range of the UNAUGMENTED sample, and the noise is drawn by standard deviation, not variance.
#   gamma_range (lo, hi)  None (off): exponent g uniform in [lo, hi], 0 < lo <= hi      gamma_prob  1.0
#   gamma_invert_prob  0: the probability that the curve is applied to the inverted sample (nnU-Net's invert_image)
#   contrast_range (lo, hi)  None (off): factor c about the sample's mean                 contrast_prob  1.0
#   noise_std_max  0 (off): the sample's standard deviation is u * noise_std_max, in units of the [-1, 1] images      noise_prob  1.0
#   blur_sigma_range (lo, hi)  None (off): Gaussian sigma in pixels, int(4 hi + 0.5) in [1, 32]      blur_prob  1.0
#   bias_field_strength  0 (off): about the RMS of the log of the smooth multiplicative field (it is an elastic_field of scale
#                        strength * sigma * sqrt(12 pi), by the RMS relation above)       bias_field_sigma  required with a strength;
#                        elastic_sigma's bounds       bias_field_prob  1.0
#   intensity_seed  the flow's seed: seed of the intensity stream
INTENSITY_KEYS = ('gamma_range', 'gamma_prob', 'gamma_invert_prob', 'contrast_range', 'contrast_prob', 'noise_std_max', 'noise_prob',
                  'blur_sigma_range', 'blur_prob', 'bias_field_strength', 'bias_field_sigma', 'bias_field_prob', 'intensity_seed')


# build-defined keys (not keras'): MR k-space artefacts of the image arrays, made in the 2-D spectrum of every slice after the gather and
# BEFORE the intensity stage (csrc/kspace.hip; the rule: include/mmseg_hip.h), after TorchIO's RandomMotion / RandomGhosting / RandomSpike
# and MONAI's GibbsNoise / KSpaceSpikeNoise / RicianNoise.  Drawn per sample and per image array (kspace_draws); everything is off by
# default.  Unlike TorchIO, motion is an in-plane translation between segments of the acquisition (no rotated copies), and the output is the
# magnitude about the sample's own minimum, lo + |ifft2(X)|, not the real part (TorchIO) or abs of the raw image (MONAI).
#   motion_shift_max  0 (off): a segment is shifted by (2u - 1) * motion_shift_max pixels per axis      motion_segments  4, in [2, 8]
#   ghost_count_range (lo, hi)  None (off): integers, 2 <= lo <= hi; every n-th phase-encode line is scaled by 1 - a
#   ghost_intensity_range (lo, hi)  required with a count: a, 0 <= lo <= hi < 1
#   gibbs_cutoff_range (lo, hi)  None (off): the kept fraction f of the spectrum's radius, 0 < lo <= hi <= 1
#   spike_count_max  0 (off), in [0, 4]: 1 .. spike_count_max spikes, each with its mirror
#   spike_intensity_range (lo, hi)  required with a count: the amplitude relative to the DC term, 0 < lo <= hi
#   rician_std_max  0 (off): the std of the complex Gaussian is u * rician_std_max, in units of the [-1, 1] images
#   motion_prob, ghost_prob, gibbs_prob, spike_prob, rician_prob  1.0
#   kspace_phase_axis  0 (rows), 1 (columns) or 'random'          kspace_seed  the flow's seed: seed of the k-space stream
KSPACE_KEYS = ('motion_shift_max', 'motion_segments', 'motion_prob', 'ghost_count_range', 'ghost_intensity_range', 'ghost_prob',
               'gibbs_cutoff_range', 'gibbs_prob', 'spike_count_max', 'spike_intensity_range', 'spike_prob', 'rician_std_max', 'rician_prob',
               'kspace_phase_axis', 'kspace_seed')


# keras arguments outside the device path: accepted only at a value that switches them off
_OFF_PATH_KEYS = ('brightness_range', 'featurewise_center', 'samplewise_center', 'featurewise_std_normalization',
                  'samplewise_std_normalization', 'zca_whitening', 'zca_epsilon', 'rescale', 'preprocessing_function', 'data_format')


def check_datagen_params(params):
    """ValueError with a clear message for a dict the device pipeline cannot honour exactly; returns the dict."""
    for k, v in params.items():
        if k in DATAGEN_KEYS or k in ELASTIC_KEYS or k in INTENSITY_KEYS or k in KSPACE_KEYS:
            continue
        if k in _OFF_PATH_KEYS:
            if k == 'zca_epsilon' or v is None or v is False or (k == 'data_format' and v == 'channels_last') or \
                    (not isinstance(v, str) and np.isscalar(v) and v == 0):
                continue
            raise ValueError('datagen parameter %s=%r is not supported on the device augmentation path (supported: %s)'
                             % (k, v, ', '.join(DATAGEN_KEYS)))
        raise ValueError('unknown datagen parameter %r (supported: %s)' % (k, ', '.join(DATAGEN_KEYS)))
    for k in ('width_shift_range', 'height_shift_range'):
        v = params.get(k, 0.)
        if isinstance(v, bool) or not np.isscalar(v) or isinstance(v, str) or \
                (isinstance(v, (int, np.integer)) and v != 0):
            raise ValueError('%s must be a float (keras 2.1.6: below 1 a fraction of the extent, otherwise pixels), got %r'
                             % (k, v))
    for k in ('rotation_range', 'shear_range', 'channel_shift_range', 'cval'):
        v = params.get(k, 0.)
        if isinstance(v, bool) or not np.isscalar(v) or isinstance(v, str):
            raise ValueError('%s must be a number, got %r' % (k, v))
    zoom_bounds(params.get('zoom_range', 0.))
    fm = params.get('fill_mode', 'nearest')
    if fm not in ops.FILL_MODES:
        raise ValueError('fill_mode must be one of %s, got %r' % (', '.join(ops.FILL_MODES), fm))
    elastic_params(params)
    intensity_params(params)
    kspace_params(params)
    return params


def _number(v):
    return not isinstance(v, (bool, str)) and np.isscalar(v) and isinstance(v, (int, float, np.integer, np.floating))


def elastic_params(params, seed=None):
    """(alpha, sigma, prob, seed) of the ELASTIC_KEYS of a datagen dict, validated: ValueError naming the key"""
    alpha, sigma = params.get('elastic_alpha', 0), params.get('elastic_sigma', None)
    prob, eseed = params.get('elastic_prob', 1.0), params.get('elastic_seed', None)
    if not _number(alpha) or not np.isfinite(alpha) or alpha < 0:
        raise ValueError('elastic_alpha must be a number >= 0 (pixels times the blurred noise), got %r' % (alpha,))
    if sigma is not None:
        if not _number(sigma) or not np.isfinite(sigma) or sigma <= 0:
            raise ValueError('elastic_sigma must be a number > 0, got %r' % (sigma,))
        if not 1 <= ops.elastic_radius(sigma) <= ops.ELASTIC_MAX_RADIUS:
            raise ValueError('elastic_sigma=%r gives a blur radius int(4*sigma + 0.5) = %d outside [1, %d]'
                             % (sigma, ops.elastic_radius(sigma), ops.ELASTIC_MAX_RADIUS))
    elif alpha != 0:
        raise ValueError('elastic_sigma is required when elastic_alpha != 0')
    if not _number(prob) or not 0 <= prob <= 1:
        raise ValueError('elastic_prob must be a number in [0, 1], got %r' % (prob,))
    if eseed is not None and (isinstance(eseed, bool) or not isinstance(eseed, (int, np.integer))):
        raise ValueError('elastic_seed must be an integer, got %r' % (eseed,))
    eseed = (0 if seed is None else seed) if eseed is None else eseed
    return float(alpha), (None if sigma is None else float(sigma)), float(prob), int(eseed)


def elastic_on(params):
    """alpha != 0 and prob != 0"""
    return bool(params.get('elastic_alpha', 0)) and bool(params.get('elastic_prob', 1.0))


def philox4x32(counter, key, rounds=10):
    """Philox4x32-10 in plain Python: 4 counter words, 2 key words -> 4 output words (the generator of the device's elastic noise)"""
    c0, c1, c2, c3 = (int(v) & 0xffffffff for v in counter)
    k0, k1 = (int(v) & 0xffffffff for v in key)
    for _ in range(rounds):
        p0, p1 = 0xD2511F53 * c0, 0xCD9E8D57 * c2
        c0, c1, c2, c3 = (p1 >> 32) ^ c1 ^ k0, p1 & 0xffffffff, (p0 >> 32) ^ c3 ^ k1, p0 & 0xffffffff
        k0, k1 = (k0 + 0x9E3779B9) & 0xffffffff, (k1 + 0xBB67AE85) & 0xffffffff
    return c0, c1, c2, c3


def elastic_scales(alpha, prob, seed, batch, B):
    """scale[b] = alpha where u01 < prob, else 0; u01 = (Q[0] >> 8) * 2^-24, Q = Philox(counter (b, 0, 0, 1), key (seed, batch)) --
    counter word 3 keeps these draws apart from the field's noise, and numpy's global RNG is not touched"""
    return np.array([alpha if (philox4x32((b, 0, 0, 1), (seed, batch))[0] >> 8) * 2.0 ** -24 < prob else 0.0 for b in range(B)],
                    np.float64)


def _range(params, key):
    """a (lo, hi) key: None, or a pair of finite numbers with 0 < lo <= hi"""
    v = params.get(key, None)
    if v is None:
        return None
    if not isinstance(v, (list, tuple, np.ndarray)) or len(v) != 2 or not all(_number(t) and np.isfinite(t) for t in v) or \
            not 0 < v[0] <= v[1]:
        raise ValueError('%s must be None or a pair (lo, hi) of numbers with 0 < lo <= hi, got %r' % (key, v))
    return float(v[0]), float(v[1])


def _prob(params, key, default):
    v = params.get(key, default)
    if not _number(v) or not 0 <= v <= 1:
        raise ValueError('%s must be a number in [0, 1], got %r' % (key, v))
    return float(v)


def intensity_params(params, seed=None):
    """the INTENSITY_KEYS of a datagen dict as a dict with every default filled in, validated: ValueError naming the key"""
    p = dict(gamma=_range(params, 'gamma_range'), gamma_prob=_prob(params, 'gamma_prob', 1.0),
             invert_prob=_prob(params, 'gamma_invert_prob', 0.), contrast=_range(params, 'contrast_range'),
             contrast_prob=_prob(params, 'contrast_prob', 1.0), noise_prob=_prob(params, 'noise_prob', 1.0),
             blur=_range(params, 'blur_sigma_range'), blur_prob=_prob(params, 'blur_prob', 1.0),
             bias_prob=_prob(params, 'bias_field_prob', 1.0))
    std = params.get('noise_std_max', 0)
    if not _number(std) or not np.isfinite(std) or std < 0:
        raise ValueError('noise_std_max must be a number >= 0 (in units of the [-1, 1] images), got %r' % (std,))
    if p['blur'] is not None and not 1 <= ops.elastic_radius(p['blur'][1]) <= ops.INTENSITY_BLUR_MAX_RADIUS:
        raise ValueError('blur_sigma_range=%r gives a blur radius int(4*hi + 0.5) = %d outside [1, %d]'
                         % (params['blur_sigma_range'], ops.elastic_radius(p['blur'][1]), ops.INTENSITY_BLUR_MAX_RADIUS))
    s, sigma = params.get('bias_field_strength', 0), params.get('bias_field_sigma', None)
    if not _number(s) or not np.isfinite(s) or s < 0:
        raise ValueError('bias_field_strength must be a number >= 0 (RMS of the log of the field), got %r' % (s,))
    if sigma is not None:
        if not _number(sigma) or not np.isfinite(sigma) or sigma <= 0:
            raise ValueError('bias_field_sigma must be a number > 0, got %r' % (sigma,))
        if not 1 <= ops.elastic_radius(sigma) <= ops.ELASTIC_MAX_RADIUS:
            raise ValueError('bias_field_sigma=%r gives a blur radius int(4*sigma + 0.5) = %d outside [1, %d]'
                             % (sigma, ops.elastic_radius(sigma), ops.ELASTIC_MAX_RADIUS))
    elif s != 0:
        raise ValueError('bias_field_sigma is required when bias_field_strength != 0')
    iseed = params.get('intensity_seed', None)
    if iseed is not None and (isinstance(iseed, bool) or not isinstance(iseed, (int, np.integer))):
        raise ValueError('intensity_seed must be an integer, got %r' % (iseed,))
    p.update(noise_std_max=float(std), bias_strength=float(s), bias_sigma=None if sigma is None else float(sigma),
             seed=int((0 if seed is None else seed) if iseed is None else iseed))
    return p


def intensity_on(params):
    """some intensity operation has a switched-on value and a non-zero probability"""
    ranges = any(params.get(k) is not None and bool(params.get(pk, 1.0)) for k, pk in (
        ('gamma_range', 'gamma_prob'), ('contrast_range', 'contrast_prob'), ('blur_sigma_range', 'blur_prob')))
    return ranges or any(bool(params.get(k, 0)) and bool(params.get(pk, 1.0)) for k, pk in (
        ('noise_std_max', 'noise_prob'), ('bias_field_strength', 'bias_field_prob')))


def intensity_draws(params, seed, batch, B, n_images):
    """The intensity draws of batch number `batch` (counted from 0) for B samples of n_images image arrays, as numpy tables [n_images, B]:
    blur / bias / contrast / noise / gamma / invert (bool: the operation is on) and sigma / c / std / g (fp64, 0 where off).
    Q_j = Philox(counter (b, a, j, 2), key (intensity_seed, batch)), u(w) = (w >> 8) * 2^-24:
        Q_0 = (p_blur, u_blur, p_bias, -)   Q_1 = (p_contrast, u_contrast, p_noise, u_noise)   Q_2 = (p_gamma, u_gamma, p_invert, -)
    on iff p < prob; a value is lo + u * (hi - lo), the noise's std u * noise_std_max.  Counter word 3 = 2 keeps these apart from the
    elastic field (0) and the elastic scales (1); numpy's global RNG is not touched."""
    p = intensity_params(params, seed)
    u = np.array([[[[(w >> 8) * 2.0 ** -24 for w in philox4x32((b, a, j, 2), (p['seed'], batch))] for j in range(3)]
                   for b in range(B)] for a in range(n_images)], np.float64).reshape(n_images, B, 3, 4)
    d = {}

    def draw(name, value, rng, prob, pw, uw):
        on = (u[:, :, pw[0], pw[1]] < prob) & (rng is not None)
        lo, hi = rng if rng is not None else (0., 0.)
        d[name], d[value] = on, np.where(on, lo + u[:, :, uw[0], uw[1]] * (hi - lo), 0.)

    draw('blur', 'sigma', p['blur'], p['blur_prob'], (0, 0), (0, 1))
    draw('contrast', 'c', p['contrast'], p['contrast_prob'], (1, 0), (1, 1))
    draw('noise', 'std', (0., p['noise_std_max']) if p['noise_std_max'] else None, p['noise_prob'], (1, 2), (1, 3))
    draw('gamma', 'g', p['gamma'], p['gamma_prob'], (2, 0), (2, 1))
    d['bias'] = (u[:, :, 0, 2] < p['bias_prob']) & (p['bias_strength'] != 0)
    d['invert'] = d['gamma'] & (u[:, :, 2, 2] < p['invert_prob'])
    return d


def intensity_tables(params, seed, draws, a):
    """the host tables of image array a for one batch, from intensity_draws' `draws`: (radius [B] int32, weight rows [B,33] fp64) or None
    when no sample is blurred; the [B,5] fp64 table of ops.intensity_apply or None when nothing else is on; (scale [B] fp64, sigma,
    seed) of the bias field's ops.elastic_field or None when no sample is biased"""
    p = intensity_params(params, seed)
    F = ops.INTENSITY_FLAGS
    blur = ops.intensity_weight_rows(draws['sigma'][a]) if draws['blur'][a].any() else None
    flags = sum(F[k] * draws[k][a].astype(np.int64) for k in ('bias', 'contrast', 'gamma', 'noise'))
    table = np.stack([flags.astype(np.float64), draws['c'][a], draws['g'][a], draws['invert'][a].astype(np.float64), draws['std'][a]],
                     axis=1) if flags.any() else None
    field = None
    if draws['bias'][a].any():
        scale = np.where(draws['bias'][a], p['bias_strength'] * p['bias_sigma'] * np.sqrt(12.0 * np.pi), 0.0)
        field = (scale, p['bias_sigma'], (p['seed'] + 0x9E3779B9 * (a + 1)) % 2 ** 32)
    return blur, table, field


def _pair(params, key, rule, ok):
    """a (lo, hi) key with its own bounds: None, or a pair of finite numbers that `ok(lo, hi)` accepts"""
    v = params.get(key, None)
    if v is None:
        return None
    if not isinstance(v, (list, tuple, np.ndarray)) or len(v) != 2 or not all(_number(t) and np.isfinite(t) for t in v) or \
            not ok(v[0], v[1]):
        raise ValueError('%s must be None or a pair (lo, hi) of numbers with %s, got %r' % (key, rule, v))
    return v[0], v[1]


def kspace_params(params, seed=None):
    """the KSPACE_KEYS of a datagen dict as a dict with every default filled in, validated: ValueError naming the key"""
    p = dict(motion_prob=_prob(params, 'motion_prob', 1.0), ghost_prob=_prob(params, 'ghost_prob', 1.0),
             gibbs_prob=_prob(params, 'gibbs_prob', 1.0), spike_prob=_prob(params, 'spike_prob', 1.0),
             rician_prob=_prob(params, 'rician_prob', 1.0))
    for key, unit in (('motion_shift_max', 'pixels'), ('rician_std_max', 'in units of the [-1, 1] images')):
        v = params.get(key, 0)
        if not _number(v) or not np.isfinite(v) or v < 0:
            raise ValueError('%s must be a number >= 0 (%s), got %r' % (key, unit, v))
        p[key] = float(v)
    S = params.get('motion_segments', 4)
    if isinstance(S, bool) or not isinstance(S, (int, np.integer)) or not 2 <= S <= ops.KSPACE_MAX_SEGMENTS:
        raise ValueError('motion_segments must be an integer in [2, %d], got %r' % (ops.KSPACE_MAX_SEGMENTS, S))
    p['motion_segments'] = int(S)
    cnt = _pair(params, 'ghost_count_range', 'integers 2 <= lo <= hi', lambda lo, hi: 2 <= lo <= hi and all(
        isinstance(t, (int, np.integer)) for t in (lo, hi)))
    p['ghost_count'] = None if cnt is None else (int(cnt[0]), int(cnt[1]))
    gi = _pair(params, 'ghost_intensity_range', '0 <= lo <= hi < 1', lambda lo, hi: 0 <= lo <= hi < 1)
    p['ghost_intensity'] = None if gi is None else (float(gi[0]), float(gi[1]))
    if cnt is not None and gi is None:
        raise ValueError('ghost_intensity_range is required with a ghost_count_range')
    gb = _pair(params, 'gibbs_cutoff_range', '0 < lo <= hi <= 1', lambda lo, hi: 0 < lo <= hi <= 1)
    p['gibbs'] = None if gb is None else (float(gb[0]), float(gb[1]))
    K = params.get('spike_count_max', 0)
    if isinstance(K, bool) or not isinstance(K, (int, np.integer)) or not 0 <= K <= ops.KSPACE_MAX_SPIKES:
        raise ValueError('spike_count_max must be an integer in [0, %d], got %r' % (ops.KSPACE_MAX_SPIKES, K))
    p['spike_count_max'] = int(K)
    si = _pair(params, 'spike_intensity_range', '0 < lo <= hi', lambda lo, hi: 0 < lo <= hi)
    p['spike_intensity'] = None if si is None else (float(si[0]), float(si[1]))
    if K and si is None:
        raise ValueError('spike_intensity_range is required when spike_count_max != 0')
    axis = params.get('kspace_phase_axis', 0)
    if isinstance(axis, bool) or not (axis == 'random' if isinstance(axis, str) else (isinstance(axis, (int, np.integer)) and axis in (0, 1))):
        raise ValueError("kspace_phase_axis must be 0 (rows), 1 (columns) or 'random', got %r" % (axis,))
    p['axis'] = axis if isinstance(axis, str) else int(axis)
    kseed = params.get('kspace_seed', None)
    if kseed is not None and (isinstance(kseed, bool) or not isinstance(kseed, (int, np.integer))):
        raise ValueError('kspace_seed must be an integer, got %r' % (kseed,))
    p['seed'] = int((0 if seed is None else seed) if kseed is None else kseed)
    return p


def kspace_on(params):
    """some k-space operation has a switched-on value and a non-zero probability"""
    return any(bool(params.get(pk, 1.0)) and (params.get(k) is not None if k.endswith('range') else bool(params.get(k, 0))) for k, pk in (
        ('motion_shift_max', 'motion_prob'), ('ghost_count_range', 'ghost_prob'), ('gibbs_cutoff_range', 'gibbs_prob'),
        ('spike_count_max', 'spike_prob'), ('rician_std_max', 'rician_prob')))


def kspace_draws(params, seed, batch, B, n_images, H, W):
    """The k-space draws of batch number `batch` (counted from 0) for B samples of n_images image arrays of H x W, as numpy tables whose
    first two axes are [n_images, B]: motion / ghost / gibbs / spike / rician (bool: the operation is on), axis (0 rows, 1 columns), breaks
    [.., S-1] (sorted, int) and shifts [.., S, 2] (dy, dx in pixels; (0, 0) in the segment that holds k_p = 0), n and a of the ghosts,
    f of the Gibbs cut, K and spikes [.., 4, 4] = (ky, kx, s, phi), std; values are 0 where their operation is off.
    Q_j = Philox(counter (b, a, j, 4), key (kspace_seed, batch)), u(w) = (w >> 8) * 2^-24, P the extent of the phase-encode axis:
        Q_0 = (p_motion, p_ghost, p_gibbs, p_spike)      Q_1 = (p_rician, u_std, u_axis, u_n)      Q_2 = (u_a, u_f, u_K, -)
        Q_3, Q_4: the breaks, u_s = word (s - 1) % 4 of Q_{3 + (s - 1) // 4}, s = 1 .. S - 1; break = floor(u_s P)
        Q_{5 + s // 2}: words 2 (s % 2), 2 (s % 2) + 1 = (u_dy, u_dx) of segment s = 0 .. S - 1; a shift is (2u - 1) motion_shift_max
        Q_{9 + i} = (u_ky, u_kx, u_s, u_phi) of spike i < K: ky = floor(u H) - floor(H/2), kx likewise, phi = 2 pi u
    on iff p < prob; axis = floor(2 u) when 'random'; n = lo + floor(u (hi - lo + 1)); a, f, s = lo + u (hi - lo); K = 1 + floor(u
    spike_count_max); std = u rician_std_max.  Counter word 3 = 4 keeps these apart from the elastic field (0), the elastic scales (1),
    the intensity draws (2) and the intensity noise (3); 5 is the Rician noise on the device.  numpy's global RNG is not touched."""
    p = kspace_params(params, seed)
    S = p['motion_segments']
    d = dict({k: np.zeros((n_images, B), bool) for k in ('motion', 'ghost', 'gibbs', 'spike', 'rician')},
             axis=np.zeros((n_images, B), np.int64), breaks=np.zeros((n_images, B, S - 1), np.int64), shifts=np.zeros((n_images, B, S, 2)),
             n=np.zeros((n_images, B), np.int64), a=np.zeros((n_images, B)), f=np.zeros((n_images, B)), K=np.zeros((n_images, B), np.int64),
             spikes=np.zeros((n_images, B, ops.KSPACE_MAX_SPIKES, 4)), std=np.zeros((n_images, B)))
    for a in range(n_images):
        for b in range(B):
            words = {}

            def u(j, w):
                if j not in words:
                    words[j] = philox4x32((b, a, j, 4), (p['seed'], batch))
                return (words[j][w] >> 8) * 2.0 ** -24

            axis = int(2 * u(1, 2)) if p['axis'] == 'random' else p['axis']
            d['axis'][a, b] = axis
            P = W if axis else H
            if p['motion_shift_max'] and u(0, 0) < p['motion_prob']:
                d['motion'][a, b] = True
                d['breaks'][a, b] = sorted(int(np.floor(u(3 + (s - 1) // 4, (s - 1) % 4) * P)) for s in range(1, S))
                zero = int((d['breaks'][a, b] <= P // 2).sum())
                for s in range(S):
                    if s != zero:
                        d['shifts'][a, b, s] = [(2 * u(5 + s // 2, 2 * (s % 2) + i) - 1) * p['motion_shift_max'] for i in (0, 1)]
            if p['ghost_count'] is not None and u(0, 1) < p['ghost_prob']:
                (lo, hi), (alo, ahi) = p['ghost_count'], p['ghost_intensity']
                d['ghost'][a, b], d['n'][a, b], d['a'][a, b] = True, lo + int(np.floor(u(1, 3) * (hi - lo + 1))), alo + u(2, 0) * (ahi - alo)
            if p['gibbs'] is not None and u(0, 2) < p['gibbs_prob']:
                d['gibbs'][a, b], d['f'][a, b] = True, p['gibbs'][0] + u(2, 1) * (p['gibbs'][1] - p['gibbs'][0])
            if p['spike_count_max'] and u(0, 3) < p['spike_prob']:
                K, (lo, hi) = 1 + int(np.floor(u(2, 2) * p['spike_count_max'])), p['spike_intensity']
                d['spike'][a, b], d['K'][a, b] = True, K
                for i in range(K):
                    d['spikes'][a, b, i] = [int(np.floor(u(9 + i, 0) * H)) - H // 2, int(np.floor(u(9 + i, 1) * W)) - W // 2,
                                            lo + u(9 + i, 2) * (hi - lo), 2.0 * np.pi * u(9 + i, 3)]
            if p['rician_std_max'] and u(1, 0) < p['rician_prob']:
                d['rician'][a, b], d['std'][a, b] = True, u(1, 1) * p['rician_std_max']
    return d


def kspace_tables(draws, a, H, W):
    """the [B,48] fp64 table of ops.kspace_forward / kspace_apply / kspace_inverse for image array a of one batch, from kspace_draws'
    `draws` (the columns: include/mmseg_hip.h), or None when no sample has an operation on"""
    F = ops.KSPACE_FLAGS
    flags = sum(F[k] * draws[k][a].astype(np.int64) for k in F)
    if not flags.any():
        return None
    B, S = len(flags), draws['shifts'].shape[2]
    t = np.zeros((B, ops.KSPACE_PARAMS), np.float64)
    t[:, 0], t[:, 1] = flags, draws['axis'][a]
    t[:, 2] = np.where(draws['motion'][a], S - 1, 0)
    t[:, 3:3 + S - 1] = draws['breaks'][a]
    t[:, 10:10 + 2 * S] = draws['shifts'][a].reshape(B, 2 * S)
    t[:, 26], t[:, 27] = draws['n'][a], 1.0 - draws['a'][a]
    t[:, 28] = draws['f'][a] * draws['f'][a] * (float(H) * H * W * W)
    t[:, 29] = draws['K'][a]
    sp = draws['spikes'][a]
    t[:, 30:46] = np.stack([np.mod(sp[..., 0], H), np.mod(sp[..., 1], W), sp[..., 2] * np.cos(sp[..., 3]), sp[..., 2] * np.sin(sp[..., 3])],
                           axis=-1).reshape(B, 16)
    t[:, 46] = draws['std'][a]
    return t


def rotation_only(params):
    """True when RotationFlow reproduces the dict exactly: nothing but rotation_range, 'nearest' edges, no elastic deformation and no
    intensity or k-space augmentation"""
    return not elastic_on(params) and not intensity_on(params) and not kspace_on(params) and params.get('fill_mode', 'nearest') == 'nearest' and not any(
        params.get(k) for k in ('width_shift_range', 'height_shift_range', 'shear_range', 'channel_shift_range',
                                'horizontal_flip', 'vertical_flip')) and zoom_bounds(params.get('zoom_range', 0.) or 0.) == (1., 1.)


def zoom_bounds(zoom_range):
    """keras: a scalar z -> [1 - z, 1 + z], a pair -> itself"""
    if np.isscalar(zoom_range) and not isinstance(zoom_range, str):
        return 1. - zoom_range, 1. + zoom_range
    if isinstance(zoom_range, (list, tuple, np.ndarray)) and len(zoom_range) == 2:
        return float(zoom_range[0]), float(zoom_range[1])
    raise ValueError('zoom_range should be a float or a tuple or list of two floats, got %r' % (zoom_range,))


class KerasTransformStream(object):
    """keras 2.1.6 NumpyArrayIterator(shuffle=True, seed=s) + random_transform of ImageDataGenerator(**params) for arrays of
    [N, H, W, C]: per batch the rows, and per sample the resampling matrix (fp64 [B, 6], flips folded in), the flip flags and
    the channel shifts ([B, C] or None).  Per sample keras draws, each only when its key is non-zero: theta, tx, ty, shear,
    (zx, zy), one channel shift per channel, the horizontal flip, the vertical flip -- all from the GLOBAL numpy RNG."""

    def __init__(self, n, batch_size, seed, params, H, W, C):
        self.n, self.batch_size, self.seed = int(n), int(batch_size), seed
        self.H, self.W, self.C = int(H), int(W), int(C)
        p = params
        self.rotation = float(p.get('rotation_range', 0.) or 0.)
        self.hshift = float(p.get('height_shift_range', 0.) or 0.)
        self.wshift = float(p.get('width_shift_range', 0.) or 0.)
        self.shear = float(p.get('shear_range', 0.) or 0.)
        self.zoom = zoom_bounds(p.get('zoom_range', 0.) or 0.)
        self.channel_shift = float(p.get('channel_shift_range', 0.) or 0.)
        self.hflip, self.vflip = bool(p.get('horizontal_flip', False)), bool(p.get('vertical_flip', False))
        self.total_batches_seen = 0
        self.batch_index = 0
        self.order = None

    def _rows(self):
        if self.seed is not None:
            np.random.seed(self.seed + self.total_batches_seen)
        if self.batch_index == 0:
            self.order = np.random.permutation(self.n)
        start = (self.batch_index * self.batch_size) % self.n
        self.batch_index = self.batch_index + 1 if self.n > start + self.batch_size else 0
        self.total_batches_seen += 1
        return self.order[start:start + self.batch_size]

    def _transform(self):
        """one sample: (3x3 fp64 matrix or None, channel shifts or None, hflip, vflip), in keras' draw order"""
        H, W = self.H, self.W
        theta = np.deg2rad(np.random.uniform(-self.rotation, self.rotation)) if self.rotation else 0
        tx = ty = 0
        if self.hshift:
            tx = np.random.uniform(-self.hshift, self.hshift)
            if self.hshift < 1:
                tx *= H
        if self.wshift:
            ty = np.random.uniform(-self.wshift, self.wshift)
            if self.wshift < 1:
                ty *= W
        shear = np.deg2rad(np.random.uniform(-self.shear, self.shear)) if self.shear else 0
        if self.zoom[0] == 1 and self.zoom[1] == 1:
            zx, zy = 1, 1
        else:
            zx, zy = np.random.uniform(self.zoom[0], self.zoom[1], 2)
        m = None
        if theta != 0:
            m = np.array([[np.cos(theta), -np.sin(theta), 0], [np.sin(theta), np.cos(theta), 0], [0, 0, 1]])
        if tx != 0 or ty != 0:
            t = np.array([[1, 0, tx], [0, 1, ty], [0, 0, 1]])
            m = t if m is None else np.dot(m, t)
        if shear != 0:
            t = np.array([[1, -np.sin(shear), 0], [0, np.cos(shear), 0], [0, 0, 1]])
            m = t if m is None else np.dot(m, t)
        if zx != 1 or zy != 1:
            t = np.array([[zx, 0, 0], [0, zy, 0], [0, 0, 1]])
            m = t if m is None else np.dot(m, t)
        if m is not None:                                  # transform_matrix_offset_center
            ox, oy = float(H) / 2 + 0.5, float(W) / 2 + 0.5
            m = np.dot(np.dot(np.array([[1, 0, ox], [0, 1, oy], [0, 0, 1]]), m), np.array([[1, 0, -ox], [0, 1, -oy], [0, 0, 1]]))
        shifts = None
        if self.channel_shift != 0:
            shifts = [np.random.uniform(-self.channel_shift, self.channel_shift) for _ in range(self.C)]
        hf = bool(self.hflip and np.random.random() < 0.5)
        vf = bool(self.vflip and np.random.random() < 0.5)
        return m, shifts, hf, vf

    def next(self):
        """-> rows [B], mats fp64 [B, 6], hflips [B], vflips [B], shifts fp64 [B, C] or None"""
        rows = self._rows()
        B, H, W = len(rows), self.H, self.W
        mats = np.zeros((B, 6), np.float64)
        hfl, vfl = np.zeros(B, bool), np.zeros(B, bool)
        shifts = np.zeros((B, self.C), np.float64) if self.channel_shift != 0 else None
        for i in range(B):
            m, sh, hfl[i], vfl[i] = self._transform()
            m = np.eye(3) if m is None else m
            # flips act on the transformed sample: out[r, c] = t[H-1-r, W-1-c] -> right factors of the matrix (integer entries: exact)
            if hfl[i]:
                m = np.dot(m, np.array([[1, 0, 0], [0, -1, W - 1], [0, 0, 1]]))
            if vfl[i]:
                m = np.dot(m, np.array([[-1, 0, H - 1], [0, 1, 0], [0, 0, 1]]))
            mats[i] = m[:2].reshape(6)
            if sh is not None:
                shifts[i] = sh
        return rows, mats, hfl, vfl, shifts


class AugmentFlow(object):
    """RotationFlow for the whole ImageDataGenerator(**params) pixel surface: iterator over aligned arrays [N,H,W,C_i] -> tuple
    of augmented device batches (a single array yields a bare tensor).

    Keras gives every array its own iterator, reseeded with seed + k, and random_transform draws one channel shift PER CHANNEL:
    with channel_shift_range != 0 an image (C = 1) and its masks (C = num_masks) consume different numbers of draws and, from the
    second sample of a batch on, get different geometry and flips (the shuffle, the first draw after the reseed, stays shared).
    So one KerasTransformStream runs per distinct channel count (a single one when channel_shift_range == 0), and the stream of
    the LAST array in zip order runs last: the global RNG is left where keras' zipped next() leaves it.

    With elastic deformation on (ELASTIC_KEYS) batch k, counted from 0, gets one displacement field from ops.elastic_field(scale, sigma,
    elastic_seed, k, H, W), scale = elastic_scales(...): every array of the batch is gathered through that same field (images and masks
    are deformed alike even where the channel-shift quirk gives them different matrices), and its draws are Philox words on the host
    and the device -- the global numpy RNG sees exactly the draws it sees with elastic off.

    With intensity augmentation on (INTENSITY_KEYS) the first n_images arrays are images: after the gather each of them is changed on the
    device with its own draws of batch k (intensity_draws: Philox, the global numpy RNG is untouched); the other arrays (masks) are not.
    n_images = 0 (the default) leaves every array as gathered.

    With k-space augmentation on (KSPACE_KEYS) the same image arrays first pass through csrc/kspace.hip with their own draws of batch k
    (kspace_draws; its own batch counter): the intensity stage then measures its statistics on the k-space output.  An (H, W) the
    transform cannot take is refused here, at construction."""

    def __init__(self, arrays, batch_size, seed, device, params, order=1, n_images=0):
        self.device = torch.device(device)
        self.arrays = [a if isinstance(a, torch.Tensor) else
                       torch.as_tensor(np.ascontiguousarray(a, dtype=np.float32)).to(self.device) for a in arrays]
        n = self.arrays[0].shape[0]
        assert all(a.shape[0] == n for a in self.arrays), [tuple(a.shape) for a in self.arrays]
        assert all(a.dim() == 4 for a in self.arrays), [tuple(a.shape) for a in self.arrays]
        self.H, self.W = int(self.arrays[0].shape[1]), int(self.arrays[0].shape[2])
        self.fill_mode, self.cval = params.get('fill_mode', 'nearest'), float(params.get('cval', 0.))
        if self.fill_mode not in ops.FILL_MODES:
            raise ValueError('fill_mode must be one of %s, got %r' % (ops.FILL_MODES, self.fill_mode))
        per_channel = float(params.get('channel_shift_range', 0.) or 0.) != 0
        chans = [int(a.shape[3]) for a in self.arrays]
        self.keys = [c if per_channel else 0 for c in chans]
        last = self.keys[-1]
        distinct = []
        for k in self.keys:
            if k not in distinct and k != last:
                distinct.append(k)
        self.streams = [(k, KerasTransformStream(n, batch_size, seed, params, self.H, self.W, k or 1)) for k in distinct + [last]]
        self.order = order
        self.elastic = elastic_params(params, seed) if elastic_on(params) else None
        self.elastic_batch = 0
        if not 0 <= int(n_images) <= len(self.arrays):
            raise ValueError('n_images must lie in [0, %d], got %r' % (len(self.arrays), n_images))
        self.n_images = int(n_images)
        self.intensity = (dict(params), seed) if intensity_on(params) and self.n_images else None
        self.intensity_batch = 0
        if self.intensity is not None:
            intensity_params(*self.intensity)
        self.kspace = (dict(params), seed) if kspace_on(params) and self.n_images else None
        self.kspace_batch = 0
        if self.kspace is not None:
            kspace_params(*self.kspace)
            for name, n in (('H', self.H), ('W', self.W)):
                if not ops.kspace_extent_ok(n):
                    raise ValueError('k-space augmentation: the extent %s = %d of the arrays cannot be transformed: an extent must lie in '
                                     '[2, %d] and have no prime factor but 2, 3 and 5' % (name, n, ops.KSPACE_MAX_EXTENT))

    def __iter__(self):
        return self

    def _kspace(self, out):
        """motion, ghosting, Gibbs ringing, spikes and Rician noise on the leading image arrays of one gathered batch, in place"""
        (params, seed), k = self.kspace, self.kspace_batch
        self.kspace_batch += 1
        draws = kspace_draws(params, seed, k, int(out[0].shape[0]), self.n_images, self.H, self.W)
        kseed = kspace_params(params, seed)['seed']
        for a in range(self.n_images):
            table = kspace_tables(draws, a, self.H, self.W)
            if table is None:          # no sample of this array is flagged: nothing is launched
                continue
            x, table = out[a], nn.host_to_device(table, self.device, np.float64)
            stats = ops.intensity_stats(x)
            spec = ops.kspace_forward(x, table, stats, ops.kspace_spectrum_buffer(x))
            ops.kspace_apply(spec, table, stats)
            ops.kspace_inverse(spec, table, stats, x, kseed, k, a)
        return out

    def _intensity(self, out):
        """blur, bias field, contrast, gamma and noise on the leading image arrays of one gathered batch"""
        (params, seed), k = self.intensity, self.intensity_batch
        self.intensity_batch += 1
        up = lambda a, dtype: nn.host_to_device(a, self.device, dtype)
        draws = intensity_draws(params, seed, k, int(out[0].shape[0]), self.n_images)
        iseed = intensity_params(params, seed)['seed']
        for a in range(self.n_images):
            blur, table, field = intensity_tables(params, seed, draws, a)
            x = out[a]
            stats = ops.intensity_stats(x) if table is not None else None          # of the sample as gathered: before the blur
            if blur is not None:
                x = ops.intensity_blur(x, up(blur[0], np.int32), up(blur[1], np.float64))
            if table is not None:
                if field is not None:
                    field = ops.elastic_field(up(field[0], np.float64), field[1], field[2], k, self.H, self.W)
                ops.intensity_apply(x, up(table, np.float64), stats, field, iseed, k, a)
            out[a] = x
        return out

    def __next__(self):
        rows_d, mats, shifts = None, {}, {}
        for k, s in self.streams:
            rows, m, _, _, sh = s.next()
            if rows_d is None:
                rows_d = nn.host_to_device(rows, self.device, np.int32)
            mats[k] = nn.host_to_device(m, self.device, np.float64)
            shifts[k] = None if sh is None else nn.host_to_device(sh, self.device, np.float32)
        if self.elastic is None:
            gather = ops.augment_gather
        else:
            alpha, sigma, prob, eseed = self.elastic
            scale = elastic_scales(alpha, prob, eseed, self.elastic_batch, len(rows))
            disp = ops.elastic_field(nn.host_to_device(scale, self.device, np.float64), sigma, eseed, self.elastic_batch, self.H, self.W)
            self.elastic_batch += 1
            gather = lambda a, r, m, *rest: ops.elastic_gather(a, r, m, disp, *rest)      # one field for every array of the batch
        out = tuple(gather(a, rows_d, mats[k], shifts[k], self.order, self.fill_mode, self.cval) for a, k in zip(self.arrays, self.keys))
        if self.kspace is not None:
            out = tuple(self._kspace(list(out)))
        if self.intensity is not None:
            out = tuple(self._intensity(list(out)))
        return out if len(out) > 1 else out[0]

    next = __next__
