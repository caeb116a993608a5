"""TEST HELPER (numpy + scipy): the elastic deformation of training batches restated -- the yardstick of tests/test_elastic_augment.py.

  * `philox4x32`: Philox4x32-10 on numpy arrays of words (uint64 arithmetic, masked), written apart from the product's host generator.
  * `noise` / `field64` / `field`: u_a = (P[a] >> 8) * 2^-23 - 1 from P = Philox(counter (r*W + c, b, 0, 0), key (seed, batch)), then
    scale[b] * scipy.ndimage.gaussian_filter(u_a[b], sigma, mode='reflect', truncate=4.0) in fp64; `field` rounds to fp32.
  * `gather`: out[b](p) = x[rows[b]](M_b (p + d_b(p))) as scipy.ndimage.map_coordinates(channel, coords, order, mode, cval) on
    coordinates composed in fp64 (map_coordinates applies affine_transform's boundary rules in all four modes at both orders), then
    keras' random_channel_shift.
  * `STANDINS`: CPU stand-ins of the new entry points for tests/cpu_backend._TABLE (the argument lists of include/mmseg_hip.h without
    the stream).
"""
import numpy as np
import torch
from scipy import ndimage as ndi

MODES = ('nearest', 'constant', 'reflect', 'wrap')
KNOWN_ANSWERS = (          # (counter, key, output) of Philox4x32-10
    ((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
)
_M32 = np.uint64(0xffffffff)


def philox4x32(counter, key):
    """counter: 4 arrays (or ints) of words, key: 2 -> 4 uint64 arrays holding 32-bit words"""
    c = [np.asarray(v, np.uint64) & _M32 for v in np.broadcast_arrays(*[np.asarray(v, np.uint64) for v in counter])]
    k = [np.uint64(int(v) & 0xffffffff) for v in key]
    for _ in range(10):
        p0 = np.uint64(0xD2511F53) * c[0]
        p1 = np.uint64(0xCD9E8D57) * c[2]
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ k[0], p1 & _M32, (p0 >> np.uint64(32)) ^ c[3] ^ k[1], p0 & _M32]
        k = [(k[0] + np.uint64(0x9E3779B9)) & _M32, (k[1] + np.uint64(0xBB67AE85)) & _M32]
    return c


def noise(seed, batch, B, H, W):
    """u [B,H,W,2] fp64, every value a multiple of 2^-23 in [-1, 1 - 2^-23]"""
    b, r, c = np.meshgrid(np.arange(B), np.arange(H), np.arange(W), indexing='ij')
    P = philox4x32((r * W + c, b, 0, 0), (seed, batch))
    return np.stack([(P[a] >> np.uint64(8)).astype(np.float64) * 2.0 ** -23 - 1.0 for a in (0, 1)], axis=-1)


def field64(scale, sigma, seed, batch, H, W):
    """[B,H,W,2] fp64: scale[b] * gaussian_filter(u_a[b], sigma, mode='reflect', truncate=4.0)"""
    scale = np.asarray(scale, np.float64)
    u = noise(seed, batch, len(scale), H, W)
    out = np.zeros_like(u)
    for b in range(len(scale)):
        for a in (0, 1):
            out[b, ..., a] = scale[b] * ndi.gaussian_filter(u[b, ..., a], sigma, mode='reflect', truncate=4.0)
    return out


def field(scale, sigma, seed, batch, H, W):
    return field64(scale, sigma, seed, batch, H, W).astype(np.float32)


def scales(alpha, prob, seed, batch, B):
    """the flow's per-sample scale: alpha where (Q[0] >> 8) * 2^-24 < prob, Q = Philox(counter (b, 0, 0, 1), key (seed, batch))"""
    Q = philox4x32((np.arange(B), 0, 0, 1), (seed, batch))
    u01 = (Q[0] >> np.uint64(8)).astype(np.float64) * 2.0 ** -24
    return np.where(u01 < prob, float(alpha), 0.0)


def gather(x, rows, mats, disp, shifts=None, order=1, mode='nearest', cval=0.):
    """x [N,H,W,C], rows [B] or None, mats [B,6] fp64, disp [B,H,W,2] -> [B,H,W,C] fp32"""
    x = np.asarray(x, np.float32)
    B, (_, H, W, C) = len(mats), x.shape
    rows = np.arange(B) if rows is None else np.asarray(rows)
    r, c = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing='ij')
    out = np.zeros((B, H, W, C), np.float32)
    for b in range(B):
        m = np.asarray(mats[b], np.float64)
        pr, pc = r + np.asarray(disp[b, ..., 0], np.float64), c + np.asarray(disp[b, ..., 1], np.float64)
        coords = np.stack([m[0] * pr + m[1] * pc + m[2], m[3] * pr + m[4] * pc + m[5]])
        for ch in range(C):
            out[b, ..., ch] = ndi.map_coordinates(x[rows[b], ..., ch], coords, order=order, mode=mode, cval=cval)
        if shifts is not None:
            lo, hi = out[b].min(), out[b].max()
            out[b] = np.clip(out[b] + np.asarray(shifts[b], np.float32)[None, None, :], lo, hi)
    return out


# ---- stand-ins of the C entry points ------------------------------------------------------------------------------------------------
def _workspace_doubles(B, H, W):
    return 2 * B * H * W if min(B, H, W) >= 1 else 0


def _elastic_field(scale, weights, disp, ws, seed, batch, B, H, W, R):
    if R < 1 or R > 128:
        return 1
    if B <= 0:
        return 0
    w = weights.numpy()[:R + 1]
    full = np.concatenate([w[:0:-1], w])
    u = noise(seed, batch, B, H, W)
    res = np.zeros((B, H, W, 2), np.float32)
    for b, s in enumerate(scale.numpy()[:B]):
        if s != 0:
            for a in (0, 1):
                g = ndi.correlate1d(ndi.correlate1d(u[b, ..., a], full, axis=0, mode='reflect'), full, axis=1, mode='reflect')
                res[b, ..., a] = s * g
    disp.copy_(torch.from_numpy(res))
    return 0


def _elastic_gather(data, rows, mat, disp, shift, out, ws, N, B, H, W, C, order, fill_mode, cval):
    if B <= 0:
        return 0
    res = gather(data.numpy(), None if rows is None else rows.numpy(), mat.numpy().reshape(B, 6), disp.numpy(),
                 None if shift is None else shift.numpy(), order, MODES[fill_mode], cval)
    out.copy_(torch.from_numpy(res))
    return 0


STANDINS = {'mmseg_elastic_workspace_doubles': _workspace_doubles, 'mmseg_elastic_field': _elastic_field,
            'mmseg_elastic_gather': _elastic_gather}
