"""Yardstick of tests/test_volume_denoise.py: a numpy restatement of the non-local means denoising of volumes (the rule is in
include/mmseg_hip.h, "non-local means denoising").  It shares no code with ops.py, loaders/volume_folder.py or csrc/denoise.hip, and
works on whole arrays: one shifted copy of the edge-padded volume per offset, the patch distance as a sum of shifted copies of the
squared differences.  `dtype` is the type of every operation (np.float64: the reference; np.float32: what the rule asks of the device,
used to measure how far fp32 alone moves the result -- the tests' bar is 16 times that).

Also here: the Rician phantom of the tests, Immerkaer's estimator in fp64, and the TEST-ONLY CPU stand-ins of the mmseg_nlm_* entry
points (STANDINS), installed into tests/cpu_backend._TABLE by the test's fixture, so that the host logic of ops.nlm_denoise and of the
loader runs without a GPU."""
import numpy as np
import torch

DEFAULTS = dict(search_radius=5, patch_radius=1, search_radius_z=0, h=1.0, noise='rician')
LOG2E = 1.4426950408889634


def constants(sigma, h, dtype):
    """(sigma, 2 sigma^2, c) in `dtype` from sigma and h rounded to fp32 once, or None for a volume that keeps its bits"""
    with np.errstate(all='ignore'):
        sig, hh = dtype(np.float32(sigma)), dtype(np.float32(h))
        two_s2 = dtype(2) * sig * sig
        g = (hh * sig) * (hh * sig)
        if not (np.isfinite(sig) and sig > 0 and np.isfinite(two_s2) and g > 0 and np.isfinite(g)):
            return None
        c = dtype(-LOG2E) / g
        if not np.isfinite(c):
            return None
    return sig, two_s2, c


def nlm(x, sigma, params=None, dtype=np.float64):
    """x [S,H,W] -> dict(out, pre, sw): `out` the rule's output in `dtype`; `pre` = m - 2 sigma^2 before the clamp and the square root
    (Rician) or m (Gaussian), the voxel's own value (squared for Rician) where sw = 0; `sw` the sum of the weights."""
    p = dict(DEFAULTS, **(params or {}))
    Rs, Rp, Rz, rician = p['search_radius'], p['patch_radius'], p['search_radius_z'], p['noise'] == 'rician'
    u = np.asarray(x, np.float32).astype(dtype)
    S, H, W = u.shape
    k = constants(sigma, p['h'], dtype)
    if k is None:
        return dict(out=u.copy(), pre=None, sw=None)
    sig, two_s2, c = k
    P, T = Rs + Rp, (2 * Rp + 1) ** 2
    up = np.pad(u, ((0, 0), (P, P), (P, P)), mode='edge')          # up[s, P + y, P + x] = u(s, clamp(y), clamp(x))
    ys, xs = np.arange(H)[:, None], np.arange(W)[None, :]
    sw, sv, wmax = np.zeros(u.shape, dtype), np.zeros(u.shape, dtype), np.zeros(u.shape, dtype)
    value = (lambda a: a * a) if rician else (lambda a: a)
    # the centre plane over the tile and its rim of Rp: rows and columns -Rp .. H + Rp - 1
    rim = up[:, Rs:Rs + H + 2 * Rp, Rs:Rs + W + 2 * Rp]
    for dz in range(-Rz, Rz + 1):
        lo, hi = max(0, -dz), min(S, S - dz)          # slices s with s + dz inside
        if hi <= lo:
            continue
        for dy in range(-Rs, Rs + 1):
            for dx in range(-Rs, Rs + 1):
                if dz == 0 and dy == 0 and dx == 0:
                    continue
                nb = up[lo + dz:hi + dz, Rs + dy:Rs + dy + H + 2 * Rp, Rs + dx:Rs + dx + W + 2 * Rp]
                e = rim[lo:hi] - nb
                D = e * e
                d = np.zeros((hi - lo, H, W), dtype)
                for a in range(2 * Rp + 1):
                    for b in range(2 * Rp + 1):
                        d = d + D[:, a:a + H, b:b + W]
                d2 = d * (dtype(1) / dtype(T))
                arg = np.maximum(d2 - two_s2, dtype(0)) * c
                w = np.where(arg >= -126, np.exp2(np.maximum(arg, dtype(-126))), dtype(0)).astype(dtype)          # no weight below 2^-126
                inside = ((ys + dy >= 0) & (ys + dy < H) & (xs + dx >= 0) & (xs + dx < W))[None]
                w = np.where(inside, w, dtype(0))
                uq = nb[:, Rp:Rp + H, Rp:Rp + W]
                wmax[lo:hi] = np.maximum(wmax[lo:hi], w)
                sw[lo:hi] += w
                sv[lo:hi] += w * value(uq)
    sw = sw + wmax
    sv = sv + wmax * value(u)
    some = sw > 0
    m = np.where(some, sv / np.where(some, sw, dtype(1)), value(u))
    if not rician:
        return dict(out=m.astype(dtype), pre=m.astype(dtype), sw=sw)
    pre = np.where(some, m - two_s2, u * u)          # a voxel that keeps its value: its square, so that out = sqrt(max(pre, 0)) everywhere
    out = np.where(some, np.sqrt(np.maximum(pre, dtype(0))), u)
    return dict(out=out.astype(dtype), pre=pre.astype(dtype), sw=sw)


def immerkaer(x):
    """sigma = sqrt(pi / 2) / (6 S (H - 2) (W - 2)) sum |L * x| over the interior pixels of every slice, in fp64; 0 for H < 3 or W < 3"""
    u = np.asarray(x, np.float32).astype(np.float64)
    S, H, W = u.shape
    if H < 3 or W < 3 or S < 1:
        return 0.0
    L = ((1, -2, 1), (-2, 4, -2), (1, -2, 1))
    r = np.zeros((S, H - 2, W - 2))
    for a in range(3):
        for b in range(3):
            r += L[a][b] * u[:, a:a + H - 2, b:b + W - 2]
    return float(np.sqrt(np.pi / 2.0) / (6.0 * S * (H - 2) * (W - 2)) * np.abs(r).sum())


# ---- the phantom: nested ellipses of 100 / 200 / 300 on a background of 0 with a little smooth shading, through a Rician channel ------
def phantom(shape=(2, 64, 64), seed=0, sigma=10.0):
    """(noisy fp32, clean fp64): noisy = sqrt((clean + n1)^2 + n2^2), n1, n2 ~ N(0, sigma^2)"""
    S, H, W = shape
    rng = np.random.RandomState(seed)
    s, r, c = np.meshgrid(np.arange(S), np.arange(H), np.arange(W), indexing='ij')
    zr, zc = (r - (H - 1) / 2.0) / max(H / 2.0, 1.0), (c - (W - 1) / 2.0) / max(W / 2.0, 1.0)
    clean = np.zeros(shape)
    clean[np.sqrt(zr ** 2 + zc ** 2) < 0.9] = 100.0
    clean[np.sqrt((zr + 0.2) ** 2 + (zc - 0.1) ** 2) < 0.55] = 200.0
    clean[np.sqrt((zr - 0.35) ** 2 + (zc + 0.3) ** 2) < 0.25] = 300.0
    clean = clean * (1.0 + 0.05 * zr - 0.04 * zc + 0.02 * (s - (S - 1) / 2.0))
    n1, n2 = rng.normal(0.0, sigma, shape), rng.normal(0.0, sigma, shape)
    return np.sqrt((clean + n1) ** 2 + n2 ** 2).astype(np.float32), clean


def rmse(a, b):
    return float(np.sqrt(np.mean((np.asarray(a, np.float64) - np.asarray(b, np.float64)) ** 2)))


# ---- CPU stand-ins of the entry points (argument lists of include/mmseg_hip.h without the stream) -----------------------------------------
CALLS = []          # (name, S, H, W) per launch entry point that got as far as launching


def _shape_ok(S, H, W):
    return S >= 0 and H >= 1 and W >= 1 and S * H * W < 2 ** 31 - 1


def standin_workspace_bytes(S, H, W):
    return 8 * 1024 if S >= 1 and _shape_ok(S, H, W) else 0


def standin_sigma(x, ws, sigma_out, S, H, W):
    if not _shape_ok(S, H, W) or (S and (x is None or ws is None or sigma_out is None)):
        return 1
    if S:
        CALLS.append(('mmseg_nlm_sigma', S, H, W))
        sigma_out[0] = immerkaer(x.numpy().reshape(S, H, W))
    return 0


def standin_denoise(x, out, sigma_dev, sigma, S, H, W, Rs, Rp, Rz, h, rician):
    if (not _shape_ok(S, H, W) or not 1 <= Rs <= 10 or not 1 <= Rp <= 3 or not 0 <= Rz <= 4 or not (0 < h < float('inf'))
            or rician not in (0, 1)):
        return 1
    if S == 0:
        return 0
    if x is None or out is None or x.data_ptr() == out.data_ptr():
        return 1
    CALLS.append(('mmseg_nlm_denoise', S, H, W))
    s = float(sigma_dev[0]) if sigma_dev is not None else float(sigma)
    res = nlm(x.numpy().reshape(S, H, W), s, dict(search_radius=Rs, patch_radius=Rp, search_radius_z=Rz, h=h,
                                                   noise='rician' if rician else 'gaussian'), np.float32)
    out.copy_(torch.from_numpy(res['out'].astype(np.float32)).reshape(out.shape))
    return 0


STANDINS = {'mmseg_nlm_workspace_bytes': standin_workspace_bytes, 'mmseg_nlm_sigma': standin_sigma, 'mmseg_nlm_denoise': standin_denoise}
