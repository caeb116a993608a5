"""TEST HELPER (numpy + scipy): the MR intensity augmentation of training batches restated in fp64 -- the yardstick of
tests/test_intensity_augment.py.

  * `draws`: the per-sample, per-image-array Philox draws (counter (b, a, j, 2), key (seed, batch)) with the Philox of tests/elastic_ref.py,
    written apart from utils/augment.intensity_draws.
  * `normals`: the Box-Muller noise of one sample, `blur`: scipy.ndimage.gaussian_filter per channel, `bias_field`: component 0 of
    elastic_ref's field.
  * `sample` / `augment`: blur, bias field, contrast, clip, gamma, noise in fp64 with one rounding to fp32 -- and, beside every value,
    a bound on what a second correct fp64 implementation may differ by before that rounding (see `sample`).
  * `STANDINS`: CPU stand-ins of the new entry points for tests/cpu_backend._TABLE (the argument lists of include/mmseg_hip.h without
    the stream).
"""
import numpy as np
import torch
from scipy import ndimage as ndi

from tests import elastic_ref as E

MAX_RADIUS = 32
FLAGS = dict(bias=1, contrast=2, gamma=4, noise=8)
U64 = 2.0 ** -52
# fp64 ulps allowed per libm call or short arithmetic chain: ROCm's device library documents at most 2 ulp for fp64 exp / log / pow / cos
# (sqrt is correctly rounded), glibc stays below 1, and the device contracts a*b + c into one rounding where numpy takes two -- at most 4
# roundings per step of the definition.  16 covers both libraries and the chain with room; it is not fitted to any kernel.
K_ULPS = 16


def _u01(w):
    return (w >> np.uint64(8)).astype(np.float64) * 2.0 ** -24


def draws(params, seed, batch, B, n_images):
    """tables [n_images, B] of a raw datagen dict: blur / bias / contrast / noise / gamma / invert (bool), sigma / c / std / g (fp64)"""
    iseed = params.get('intensity_seed', seed)
    b, a = np.meshgrid(np.arange(B), np.arange(n_images))
    Q = [[_u01(w) for w in E.philox4x32((b, a, j, 2), (iseed, batch))] for j in range(3)]

    def one(rng, prob, p, u):
        on = (p < prob) & (rng is not None)
        lo, hi = rng if rng is not None else (0., 0.)
        return on, np.where(on, lo + u * (hi - lo), 0.)

    d = {}
    d['blur'], d['sigma'] = one(params.get('blur_sigma_range'), params.get('blur_prob', 1.0), Q[0][0], Q[0][1])
    d['bias'] = (Q[0][2] < params.get('bias_field_prob', 1.0)) & bool(params.get('bias_field_strength', 0))
    d['contrast'], d['c'] = one(params.get('contrast_range'), params.get('contrast_prob', 1.0), Q[1][0], Q[1][1])
    smax = params.get('noise_std_max', 0)
    d['noise'], d['std'] = one((0., smax) if smax else None, params.get('noise_prob', 1.0), Q[1][2], Q[1][3])
    d['gamma'], d['g'] = one(params.get('gamma_range'), params.get('gamma_prob', 1.0), Q[2][0], Q[2][1])
    d['invert'] = d['gamma'] & (Q[2][2] < params.get('gamma_invert_prob', 0.))
    return d


def uniforms(seed, batch, b, a, H, W, C):
    """(u1 in (0, 1], u2 in [0, 1)) [H,W,C] of the noise of sample b of image array a"""
    e = np.arange(H * W * C).reshape(H, W, C)
    P = E.philox4x32((e, b, a, 3), (seed, batch))
    return ((P[0] >> np.uint64(8)).astype(np.float64) + 1.0) * 2.0 ** -24, _u01(P[1])


def normals(seed, batch, b, a, H, W, C):
    u1, u2 = uniforms(seed, batch, b, a, H, W, C)
    return np.sqrt(-2.0 * np.log(u1)) * np.cos(2.0 * np.pi * u2)


def blur64(x, sigma):
    """x [H,W,C] -> fp64 gaussian_filter over the two spatial axes, per channel"""
    x = np.asarray(x, np.float64)
    return np.stack([ndi.gaussian_filter(x[..., ch], sigma, mode='reflect', truncate=4.0) for ch in range(x.shape[-1])], axis=-1)


def blur(x, sigma):
    return blur64(x, sigma).astype(np.float32)


def bias_scale(params, on):
    return np.where(on, params['bias_field_strength'] * params['bias_field_sigma'] * np.sqrt(12.0 * np.pi), 0.0)


def bias_seed(seed, a):
    return (seed + 0x9E3779B9 * (a + 1)) % 2 ** 32


def bias_field(params, seed, batch, a, on, H, W):
    """[B,H,W] fp32: component 0 of elastic_ref's field of image array a"""
    return E.field(bias_scale(params, on), params['bias_field_sigma'], bias_seed(params.get('intensity_seed', seed), a), batch, H, W)[..., 0]


def measure(x):
    """(lo, hi, mean, elements) of one sample in fp64"""
    s = np.asarray(x, np.float64)
    return s.min(), s.max(), s.sum() / s.size, s.size


def sample(x, st, f=None, c=None, g=None, invert=False, std=None, n=None, df=None):
    """One sample after the blur: x [H,W,C] fp32 (the blurred sample), st = measure(the sample as gathered), f [H,W] the log bias field
    or None, c the contrast factor or None, g the exponent or None, std and n [H,W,C] the noise or None.
    -> (fp32 result, bound): bound >= |fp32(other) - result| for any `other` that evaluates the same formulas in fp64 with K_ULPS ulps
    per step, a mean from another summation order (|d mean| <= 2 per 2^-53 max|x|: two recursive-sum bounds) and, with df [H,W], a field
    that differs by at most df.  The bound follows the error through each step's derivative; for g < 1, where pow's derivative is
    unbounded at 0, it uses |a^g - b^g| <= |a - b|^g.  It ends with one fp32 spacing of the result for the final rounding."""
    lo, hi, mean, per = st
    A = max(abs(lo), abs(hi))
    dmean = 2.0 * per * 2.0 ** -53 * A
    k = K_ULPS * U64
    v = np.asarray(x, np.float64).copy()
    err = np.zeros_like(v)
    if f is not None:
        ef = np.exp(np.asarray(f, np.float64))[..., None]
        v1 = lo + (v - lo) * ef
        err = err * ef + np.abs(v - lo) * ef * (k + (0. if df is None else np.asarray(df, np.float64)[..., None])) + k * np.maximum(A, np.abs(v1))
        v = v1
    if c is not None:
        v1 = mean + (v - mean) * c
        err = c * err + abs(1. - c) * dmean + k * np.maximum(np.maximum(A, np.abs(v1)), np.abs(v) * c)
        v = v1
    if f is not None or c is not None:
        v = np.minimum(np.maximum(v, lo), hi)
    if g is not None and hi > lo:
        t = np.minimum(np.maximum((v - lo) / (hi - lo), 0.), 1.)
        dt = err / (hi - lo) + k
        t = 1. - np.power(1. - t, g) if invert else np.power(t, g)
        err = (hi - lo) * ((g * dt if g >= 1 else dt ** g) + 2 * k) + k * A
        v = lo + t * (hi - lo)
    if std is not None:
        v1 = v + std * n
        err = err + std * k * (np.abs(n) + 8.) + k * np.maximum(np.abs(v), np.abs(v1))
        v = v1
    out = v.astype(np.float32)
    return out, err + np.spacing(np.abs(out)).astype(np.float64)


def augment(x, d, a, seed, batch, field=None, dfield=None, blurred=None):
    """x [B,H,W,C] fp32 as gathered, d = draws(...), image array a, field [B,H,W] (bias_field) -> (fp32 [B,H,W,C], bound); a sample with
    nothing on is x's bits.  blurred: the blurred batch to use in place of the restated blur (so a test can hand over the device's)."""
    x = np.asarray(x, np.float32)
    B, H, W, C = x.shape
    out, bound = x.copy(), np.zeros(x.shape, np.float64)
    for b in range(B):
        v = x[b]
        if d['blur'][a, b] and int(4.0 * d['sigma'][a, b] + 0.5) >= 1:
            v = blur(x[b], d['sigma'][a, b]) if blurred is None else np.asarray(blurred[b], np.float32)
        out[b] = v
        if d['bias'][a, b] or d['contrast'][a, b] or d['gamma'][a, b] or d['noise'][a, b]:
            out[b], bound[b] = sample(v, measure(x[b]), field[b] if d['bias'][a, b] else None, d['c'][a, b] if d['contrast'][a, b] else None,
                                      d['g'][a, b] if d['gamma'][a, b] else None, bool(d['invert'][a, b]),
                                      d['std'][a, b] if d['noise'][a, b] else None,
                                      normals(seed, batch, b, a, H, W, C) if d['noise'][a, b] else None,
                                      None if dfield is None else dfield[b])
    return out, bound


def weight_rows(sigmas):
    """(radius [B] int32, weights [B,33] fp64) as scipy computes gaussian_filter's kernel"""
    radius, rows = np.zeros(len(sigmas), np.int32), np.zeros((len(sigmas), MAX_RADIUS + 1), np.float64)
    for b, s in enumerate(sigmas):
        R = int(4.0 * s + 0.5) if s else 0
        if R:
            w = np.exp(-0.5 / (s * s) * np.arange(-R, R + 1) ** 2)
            radius[b], rows[b, :R + 1] = R, (w / w.sum())[R:]
    return radius, rows


# ---- stand-ins of the C entry points ------------------------------------------------------------------------------------------------
def _ok(B, H, W, C):
    return min(B, H, W, C) >= 1 and B <= 65535 and H * W * C <= 2 ** 31 - 1 - 65536


def _workspace_doubles(B, H, W, C):
    per = H * W * C
    return B * max(per, 3 * min(-(-per // 256), 256)) if _ok(B, H, W, C) else 0


def _stats(x, stats, ws, B, H, W, C):
    if B <= 0:
        return 0
    if not _ok(B, H, W, C):
        return 1
    v = x.numpy().astype(np.float64).reshape(B, -1)
    stats.copy_(torch.from_numpy(np.stack([v.min(1), v.max(1), v.sum(1)], axis=1)))
    return 0


def _blur(x, radius, weights, out, ws, B, H, W, C):
    if B <= 0:
        return 0
    if not _ok(B, H, W, C):
        return 1
    res = x.numpy().copy()
    for b in range(B):
        R = min(int(radius[b]), MAX_RADIUS)
        if R > 0:
            w = weights.numpy()[b, :R + 1]
            full = np.concatenate([w[:0:-1], w])
            v = res[b].astype(np.float64)
            res[b] = ndi.correlate1d(ndi.correlate1d(v, full, axis=1, mode='reflect'), full, axis=0, mode='reflect')
    out.copy_(torch.from_numpy(res))
    return 0


def _apply(x, params, stats, field, seed, batch, array, B, H, W, C):
    if B <= 0:
        return 0
    if not _ok(B, H, W, C):
        return 1
    v, p, st = x.numpy(), params.numpy(), stats.numpy()
    for b in range(B):
        flags = int(p[b, 0])
        if not flags & 15:
            continue
        n = normals(seed, batch, b, array, H, W, C) if flags & 8 else None
        v[b], _ = sample(v[b], (st[b, 0], st[b, 1], st[b, 2] / v[b].size, v[b].size), field.numpy()[b, ..., 0] if flags & 1 and field is not None else None,
                         p[b, 1] if flags & 2 else None, p[b, 2] if flags & 4 else None, p[b, 3] != 0, p[b, 4] if flags & 8 else None, n)
    return 0


STANDINS = {'mmseg_intensity_workspace_doubles': _workspace_doubles, 'mmseg_intensity_stats': _stats, 'mmseg_intensity_blur': _blur,
            'mmseg_intensity_apply': _apply}
