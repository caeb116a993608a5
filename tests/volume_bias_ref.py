"""Yardstick of tests/test_volume_bias.py: a numpy restatement of the bias-field correction (the rule is in include/mmseg_hip.h), in fp64
with numpy.fft and scipy.ndimage.gaussian_filter1d(mode='constant').  It shares no code with ops.py, loaders/volume_folder.py or
csrc/biasfield.hip.

The bars.
  Otsu, histogram   the same IEEE operations in the same order on both sides: equality.  The histogram's inputs are chosen so that the
                    smallest distance of c + 0.5 to an integer exceeds MARGIN = 1e-9, which the tests assert on this side first.
  masked Gaussian   one pass is a sum of 2R + 1 products; the kernel and scipy add them in different orders, each within gamma_(2R+2) of the
                    sum of the moduli (Higham, section 4.2), and the three passes add: smooth_bar = 2 u (2 (Rs + Rr + Rc) + 9) G * |y|.
  sharpen           Higham section 24.1 as in tests/kspace_ref.py: two implementations of one 512-point transform differ by at most
                    T = C_FFT eps64 log2 512 relative to the 2-norm of the result.  sharpen_bar carries 2-norm bounds through the five
                    steps (F^, V^ Re G, U, fft(U b + i U), its product with F^ and the way back) to one number e_nd that bounds the error of
                    every numerator and denominator entry, and then bounds the quotient entry by entry:
                        |dE_j| <= e_nd (1 + |E_j|) / (|den_j| - e_nd) + 4 u |E_j|      where |den_j| > 2 e_nd, no statement elsewhere.
                    The bound is loose (the multiplication by Re G is bounded through 1 / noise and max |V^| = the number of voxels);
                    profiles/volume_bias_bench.md records what was measured beside it.
  end to end        the fp32 output in fp32 spacings; the bar is in the test, beside the measurement it came from.

Also here: the phantom of the issue, and the TEST-ONLY CPU stand-ins of the mmseg_bias_* entry points (STANDINS), installed into
tests/cpu_backend._TABLE by the test's fixture, so that the host logic of ops.bias_correct and the loader runs without a GPU."""
import numpy as np
import torch
from scipy.ndimage import gaussian_filter1d

BINS, PAD, OFFSET = 200, 512, 156
FWHM, NOISE, TRUNCATE = 0.15, 0.01, 4.0
LN2X4 = 2.772588722239781          # 4 ln 2
GNORM = 0.9394372786996513         # 2 sqrt(ln 2 / pi)
DEFAULTS = dict(sigma_mm=40.0, levels=3, iterations=20, extent='3d')
MARGIN = 1e-9
U64 = 2.0 ** -53
EPS64 = 2.0 ** -52
C_FFT = 12.0                       # tests/kspace_ref.py


def otsu(x):
    """(lo, hi, threshold, constant) of x fp32, every step in fp64 on integer counts"""
    x = np.asarray(x, np.float32)
    lo, hi = np.float64(x.min()), np.float64(x.max())
    if not hi > lo:
        return lo, hi, lo, True
    b = np.minimum(np.floor((x.astype(np.float64) - lo) * (256.0 / (hi - lo))), 255).astype(np.int64)
    n = np.bincount(b.ravel(), minlength=256).astype(np.int64)
    j = np.arange(256, dtype=np.int64)
    total, first = int(n.sum()), int((j * n).sum())
    best, cut, w0, s0 = -1.0, 0, 0, 0
    for t in range(255):
        w0 += int(n[t])
        s0 += t * int(n[t])
        w1 = total - w0
        var = 0.0
        if w0 > 0 and w1 > 0:
            d = np.float64(s0) / np.float64(w0) - np.float64(first - s0) / np.float64(w1)
            var = (np.float64(w0) * np.float64(w1)) * (d * d)
        if var > best:
            best, cut = var, t
    thr = lo + (np.float64(cut + 1) * (hi - lo)) / 256.0
    return lo, hi, max(thr, 0.0), False


def level_sigmas(spacings, sigma_mm, levels, extent):
    """per level (sigma_s or None, sigma_r, sigma_c) in voxels"""
    out = []
    for l in range(levels):
        s = [sigma_mm / 2.0 ** l / float(d) if (a > 0 or extent == '3d') else None for a, d in enumerate(spacings)]
        out.append(tuple(s))
    return out


def radius(sigma):
    return 0 if sigma is None else int(TRUNCATE * sigma + 0.5)


def smooth(y, sig):
    """G * y: along W, then H, then S (where sig[0] is not None), zero outside the volume"""
    y = np.asarray(y, np.float64)
    for axis in (2, 1, 0):
        if sig[axis] is not None:
            y = gaussian_filter1d(y, sig[axis], axis=axis, mode='constant', cval=0.0, truncate=TRUNCATE)
    return y


def smooth_bar(y, sig):
    """the bar on |got - ref| of smooth(y, sig), element-wise (module docstring)"""
    k = 2 * sum(radius(s) for s in sig) + 9
    return 2.0 * U64 * k * smooth(np.abs(y), sig)


def histogram(v, m):
    """(hist [200] int64, vmin, vmax, c over the mask, the smallest distance of c + 0.5 to an integer); v fp64, m bool"""
    vm = np.asarray(v, np.float64)[m]
    vmin, vmax = vm.min(), vm.max()
    slope = (vmax - vmin) / (BINS - 1)
    c = (vm - vmin) / slope
    q = c + 0.5
    margin = np.abs(q - np.round(q)).min()
    hist = np.bincount(np.floor(q).astype(np.int64), minlength=BINS)
    return hist, vmin, vmax, c, margin


def sharpen(hist, vmin, vmax, parts=False):
    """E [200] fp64 of the rule; parts=True adds the padded numerator and denominator and the intermediate arrays sharpen_bar needs"""
    slope = (vmax - vmin) / (BINS - 1)
    w = FWHM / slope
    V = np.zeros(PAD)
    V[OFFSET:OFFSET + BINS] = hist
    n = np.arange(PAD)
    m = np.minimum(n, PAD - n).astype(np.float64)
    arg = (m * m * LN2X4) / (w * w)
    F = (GNORM / w) * np.exp(-arg)
    Fh = np.fft.fft(F)
    Vh = np.fft.fft(V)
    G = np.conj(Fh) / (np.abs(Fh) ** 2 + NOISE)
    U = np.maximum(np.fft.ifft(Vh * G.real).real, 0.0)
    b = vmin + (n - OFFSET) * slope
    num = np.fft.ifft(np.fft.fft(U * b) * Fh).real
    den = np.fft.ifft(np.fft.fft(U) * Fh).real
    with np.errstate(divide='ignore', invalid='ignore'):
        E = np.where(den != 0.0, num / den, 0.0)
    if parts:
        return E[OFFSET:OFFSET + BINS], dict(F=F, arg=arg, Fh=Fh, Vh=Vh, g=G.real, U=U, b=b, num=num, den=den)
    return E[OFFSET:OFFSET + BINS]


def sharpen_bar(hist, vmin, vmax):
    """(bar [200] on |E_got - E_ref|, inf where the bound makes no statement; e_nd) -- the chain of the module docstring"""
    E, p = sharpen(hist, vmin, vmax, parts=True)
    T = C_FFT * EPS64 * np.log2(PAD)
    rt = np.sqrt(PAD)
    nrm = np.linalg.norm
    e_F = nrm(8.0 * U64 * (1.0 + p['arg']) * p['F'])               # w, the argument (relative error -> absolute arg * u), exp, the product
    e_Fh = rt * e_F + T * nrm(p['Fh'])
    e_Vh = T * nrm(p['Vh'])
    e_g = e_Fh / NOISE + 4.0 * U64 * nrm(p['g'])                   # |grad of Re z / (|z|^2 + noise)| <= 1 / noise
    Wv = p['Vh'] * p['g']
    e_W = np.abs(p['g']).max() * e_Vh + np.abs(p['Vh']).max() * e_g + 2.0 * U64 * nrm(Wv)
    e_U = e_W / rt + T * nrm(Wv) / rt                              # the clamp is 1-Lipschitz
    z = p['U'] * p['b'] + 1j * p['U']
    e_z = np.sqrt(np.abs(p['b']).max() ** 2 + 1.0) * e_U + 4.0 * U64 * nrm(z)
    Zh = np.fft.fft(z)
    e_Zh = rt * e_z + T * nrm(Zh)
    Q = Zh * p['Fh']
    e_Q = np.abs(p['Fh']).max() * e_Zh + np.abs(Zh).max() * e_Fh + 4.0 * U64 * nrm(Q)
    e_nd = e_Q / rt + T * nrm(Q) / rt
    den = np.abs(p['den'][OFFSET:OFFSET + BINS])
    with np.errstate(divide='ignore', invalid='ignore'):
        bar = np.where(den > 2.0 * e_nd, e_nd * (1.0 + np.abs(E)) / (den - e_nd) + 4.0 * U64 * np.abs(E), np.inf)
    return bar, e_nd


def interpolate(E, c):
    i = np.minimum(np.floor(c), BINS - 2).astype(np.int64)
    return E[i] + (c - i) * (E[i + 1] - E[i])


def correct(x, spacings, params=None):
    """The rule on x [S,H,W] fp32 -> dict(out fp32, field fp64, mask, margin (smallest bin-edge distance over all iterations), updates
    (iterations that updated the field), frozen)"""
    p = dict(DEFAULTS)
    p.update(params or {})
    x = np.ascontiguousarray(x, np.float32)
    res = dict(out=x.copy(), field=np.zeros(x.shape), mask=np.zeros(x.shape, bool), margin=np.inf, updates=0, frozen=True)
    lo, hi, thr, constant = otsu(x)
    if constant:
        return res
    x64 = x.astype(np.float64)
    m = x64 > thr
    res['mask'] = m
    if not m.any():
        return res
    v0 = np.zeros(x.shape)
    v0[m] = np.log(x64[m])
    f = np.zeros(x.shape)
    frozen = False
    for sig in level_sigmas(spacings, p['sigma_mm'], p['levels'], p['extent']):
        if frozen:
            break
        den = smooth(m.astype(np.float64), sig)
        for _ in range(p['iterations']):
            v = v0 - f
            if not v[m].max() > v[m].min():
                frozen = True
                break
            hist, vmin, vmax, c, margin = histogram(v, m)
            res['margin'] = min(res['margin'], margin)
            E = sharpen(hist, vmin, vmax)
            r = np.zeros(x.shape)
            r[m] = v[m] - interpolate(E, c)
            num = smooth(r, sig)
            pos = den > 0
            f[pos] += num[pos] / den[pos]
            res['updates'] += 1
    res['frozen'] = frozen
    if res['updates']:
        res['out'] = (x64 * np.exp(-f)).astype(np.float32)
        res['field'] = f
    return res


# ---- the phantom: three tissues, noise and a smooth multiplicative field --------------------------------------------------------------
def phantom(shape=(6, 64, 56), spacings=(6.0, 1.6, 1.6), seed=0, strength=0.4, noise=0.03):
    """(x fp32, true log-field fp64, tissue [S,H,W] int: 0 background, 1..3) -- nested ellipsoids of grey values 300 / 600 / 1000 on a dark
    background, `noise` relative noise, times exp(field), field = a low-order polynomial in mm of amplitude about +-strength"""
    S, H, W = shape
    rng = np.random.RandomState(seed)
    s, r, c = np.meshgrid(np.arange(S), np.arange(H), np.arange(W), indexing='ij')
    zs, zr, zc = ((s - (S - 1) / 2.0) / max(S / 2.0, 1.0), (r - (H - 1) / 2.0) / (H / 2.0), (c - (W - 1) / 2.0) / (W / 2.0))
    rad = np.sqrt((0.6 * zs) ** 2 + zr ** 2 + zc ** 2)
    tissue = np.zeros(shape, np.int64)
    tissue[rad < 0.9] = 1
    tissue[np.sqrt((0.6 * zs) ** 2 + (zr + 0.2) ** 2 + (zc - 0.1) ** 2) < 0.55] = 2
    tissue[np.sqrt((0.6 * zs) ** 2 + (zr - 0.35) ** 2 + (zc + 0.3) ** 2) < 0.25] = 3
    grey = np.array([20.0, 300.0, 600.0, 1000.0])[tissue]
    grey = grey * (1.0 + noise * rng.standard_normal(shape))
    a = rng.uniform(-1, 1, 6)
    field = a[0] * zr + a[1] * zc + a[2] * zs * 0.5 + a[3] * zr * zc + a[4] * (zr ** 2 - 0.33) + a[5] * (zc ** 2 - 0.33)
    field = strength * field / np.abs(field).max()
    x = np.maximum(grey * np.exp(field), 0.0).astype(np.float32)
    return x, field, tissue


def tissue_cv(x, tissue):
    """coefficient of variation of x within tissues 1..3"""
    return [float(np.std(x[tissue == t], dtype=np.float64) / np.mean(x[tissue == t], dtype=np.float64)) for t in (1, 2, 3)]


def spacings_apart(got, want):
    """largest |got - want| in fp32 spacings (ulps) of `want`"""
    got, want = np.asarray(got, np.float32), np.asarray(want, np.float32)
    sp = np.spacing(np.abs(want)).astype(np.float64)
    return float((np.abs(got.astype(np.float64) - want.astype(np.float64)) / sp).max())


# ---- CPU stand-ins of the entry points (argument lists of include/mmseg_hip.h without the stream) -----------------------------------------
CALLS = []          # one (S, H, W) per mmseg_bias_begin: the tests count the corrections
_state = {}         # workspace pointer -> the volume under way


def _shape_ok(S, H, W):
    return 1 <= S <= 65535 and 1 <= H <= 65535 and 1 <= W <= 65535 and S * H * W < 2 ** 31 - 1


def standin_workspace_doubles(S, H, W):
    return 512 + 6 * S * H * W + (S * H * W + 7) // 8 if _shape_ok(S, H, W) else 0


def _sig_of(weights, radii):
    """the sigmas behind weight rows [3,129]: w_1 / w_0 = exp(-0.5 / sigma^2)"""
    w = weights.numpy()
    return tuple(None if R == 0 else float(np.sqrt(-0.5 / np.log(w[a, 1] / w[a, 0]))) for a, R in enumerate(radii))


def standin_begin(x, ws, S, H, W):
    if not _shape_ok(S, H, W):
        return 1
    CALLS.append((S, H, W))
    xv = x.numpy().reshape(S, H, W).copy()
    st = dict(x=xv, f=np.zeros(xv.shape), updates=0, frozen=False, m=None, v0=None)
    lo, hi, thr, constant = otsu(xv)
    if constant:
        st['frozen'] = True
    else:
        st['m'] = xv.astype(np.float64) > thr
        st['v0'] = np.zeros(xv.shape)
        st['v0'][st['m']] = np.log(xv.astype(np.float64)[st['m']])
    _state[ws.data_ptr()] = st
    return 0


def standin_level(ws, roots, weights, S, H, W, Rs, Rr, Rc, iterations):
    if not (_shape_ok(S, H, W) and 0 <= Rs <= 128 and 1 <= Rr <= 128 and 1 <= Rc <= 128 and 1 <= iterations <= 1000):
        return 1
    st = _state[ws.data_ptr()]
    if st['frozen']:
        return 0
    m, sig = st['m'], _sig_of(weights, (Rs, Rr, Rc))
    den = smooth(m.astype(np.float64), sig)
    for _ in range(iterations):
        v = st['v0'] - st['f']
        if not m.any() or not v[m].max() > v[m].min():
            st['frozen'] = True
            return 0
        hist, vmin, vmax, c, _ = histogram(v, m)
        r = np.zeros(v.shape)
        r[m] = v[m] - interpolate(sharpen(hist, vmin, vmax), c)
        num = smooth(r, sig)
        pos = den > 0
        st['f'][pos] += num[pos] / den[pos]
        st['updates'] += 1
    return 0


def standin_finish(x, ws, S, H, W):
    st = _state[ws.data_ptr()]
    if st['updates']:
        x.copy_(torch.from_numpy((st['x'].astype(np.float64) * np.exp(-st['f'])).astype(np.float32)).reshape(x.shape))
    return 0


def standin_field(ws, field, info, S, H, W):
    st = _state[ws.data_ptr()]
    field.copy_(torch.from_numpy(st['f'] if st['updates'] else np.zeros(st['f'].shape)).reshape(field.shape))
    if info is not None:
        info.copy_(torch.tensor([int(st['frozen']), st['updates']], dtype=torch.int32))
    return 0


STANDINS = {'mmseg_bias_workspace_doubles': standin_workspace_doubles, 'mmseg_bias_begin': standin_begin, 'mmseg_bias_level': standin_level,
            'mmseg_bias_finish': standin_finish, 'mmseg_bias_field': standin_field}
