"""TEST HELPER (numpy fp64, numpy.fft): the MR k-space artefact augmentation of training batches restated -- the yardstick of
tests/test_kspace_augment.py.

  * `draws`: the per-sample, per-image-array Philox draws (counter (b, a, j, 4), key (seed, batch)) with the Philox of
    tests/elastic_ref.py, written apart from utils/augment.kspace_draws.
  * `table`: the [B,48] table of include/mmseg_hip.h from those draws.
  * `spectrum` / `rule` / `image` / `augment`: fft2 of x - lo, the rule on the spectrum, lo + |ifft2 + Rician draw|, and all three on a
    batch, in fp64 with one rounding to fp32.
  * `spectrum_bound` / `image_bound`: what two correct implementations may differ by (below).
  * `STANDINS`: CPU stand-ins of the new entry points for tests/cpu_backend._TABLE (the argument lists of include/mmseg_hip.h without
    the stream).

The bounds.  Higham, Accuracy and Stability of Numerical Algorithms, section 24.1 (theorem 24.2): a radix-2 Cooley-Tukey transform of
length N = 2^t computed with roots of relative error mu satisfies ||X^ - X||_2 <= t eta / (1 - t eta) ||X||_2, eta = mu + gamma_4 (sqrt 2 +
mu): every stage is a unitary butterfly times sqrt 2 whose rounding errors add eta relative to the norm it carries.  The same argument
stage by stage, with u = 2^-53 and mu = u (fp64 cos / sin of the table, correctly rounded or nearly so):
    radix 2    eta_2 = u + 4 u (sqrt 2 + u) < 6.7 u                                                      for 1 stage,        6.7 u a stage
    radix 4    two radix-2 stages whose inner roots (+-1, +-i) are exact: at most 2 eta_2                 for 2 stages,       6.7 u a stage
    radix 3    root product (sqrt 2 gamma_2 + mu < 3.9 u), then y_p = sum of 3 products with roots (3.9 u each, 2 additions: + 2 u):
               |dy_p| <= 9.7 u sum_q |v_q| <= 9.7 u sqrt 3 ||v||, the 3 outputs: 29.1 u ||v|| = 16.8 u ||F_3 v||  for log2 3 = 1.58 stages, 10.6 u
    radix 5    the same with 5 products and 4 additions: 11.7 u * 5 ||v|| = 26.2 u ||F_5 v||               for log2 5 = 2.32 stages, 11.3 u
so a transform of length N, whatever the radices, is within 11.3 u log2 N = 5.65 eps64 log2 N of the exact one relative to ||X||_2 (first
order; t eta < 1e-13), and the two axes of fft2 add: log2 H + log2 W = log2 (H W).  Two implementations (the kernel; numpy's pocketfft,
radix 4 / 2 / 3 / 5 passes as well) differ by twice that: C_FFT = 12 >= 2 * 5.65.
  spectrum   ||got - ref||_2 <= C_FFT eps64 log2(H W) ||X||_2 = C_FFT eps64 log2(H W) sqrt(H W) ||y||_2 is what the theorem gives: a bound on
             the ROOT MEAN SQUARE error, rms(got - ref) <= C_FFT eps64 log2(H W) ||y||_2.  The tests assert that and, as the stricter
             statement, the same bar on EVERY element: max |got - ref| <= C_FFT eps64 log2(H W) ||y||_2.
  image      z = ifft2(X) is unitary up to 1 / sqrt(H W), so an error dX of the spectrum arrives as ||dz||_2 = ||dX||_2 / sqrt(H W)
             <= C_FFT eps64 log2(H W) ||y||_2, and the inverse adds as much again relative to ||X||_2 / sqrt(H W); every element is
             within the 2-norm.  The rule in between multiplies by factors of modulus <= 1 (they carry the error on unchanged) and adds
             the spikes, which join the norm: Y = ||y||_2 + sum of the spike amplitudes |A| (each spike twice).  Its own arithmetic -- the
             motion phase, whose argument |theta| <= 2 pi (|dy| + |dx|) / 2 turns an argument error of eps64 |theta| into a phase error,
             the products and the Rician draw's log / sqrt / sincos -- is K_ULPS fp64 ulps per step:
                 E = eps64 ((2 C_FFT log2(H W) + K_ULPS (1 + pi (|dy| + |dx|)_max)) Y + K_ULPS (|z| + |draw|)_max)
             and |got - ref| <= one fp32 spacing at the reference value + E.  With inputs in [-1, 1] and the tested shapes E < 2^-30.
"""
import numpy as np
import torch

from tests import elastic_ref as E

C_FFT = 12
K_ULPS = 16          # as tests/intensity_ref.py: fp64 ulps per libm call or short chain (ROCm documents <= 2 ulp for log / sincos / hypot)
EPS64 = 2.0 ** -52
FLAGS = dict(motion=1, ghost=2, gibbs=4, spike=8, rician=16)
P_COLS = 48
MAX_EXTENT = 1024


def extent_ok(n):
    if not 2 <= n <= MAX_EXTENT:
        return False
    for f in (2, 3, 5):
        while n % f == 0:
            n //= f
    return n == 1


def _u(w):
    return float(int(w) >> 8) * 2.0 ** -24


def draws(params, seed, batch, B, n_images, H, W):
    """the tables of utils/augment.kspace_draws from a raw datagen dict, written apart"""
    kseed = params.get('kspace_seed', seed)
    S = params.get('motion_segments', 4)
    smax, kmax, rmax = params.get('motion_shift_max', 0), params.get('spike_count_max', 0), params.get('rician_std_max', 0)
    d = dict({k: np.zeros((n_images, B), bool) for k in FLAGS}, axis=np.zeros((n_images, B), np.int64),
             breaks=np.zeros((n_images, B, S - 1), np.int64), shifts=np.zeros((n_images, B, S, 2)), n=np.zeros((n_images, B), np.int64),
             a=np.zeros((n_images, B)), f=np.zeros((n_images, B)), K=np.zeros((n_images, B), np.int64), spikes=np.zeros((n_images, B, 4, 4)),
             std=np.zeros((n_images, B)))
    for a in range(n_images):
        for b in range(B):
            Q = [[_u(w) for w in E.philox4x32((b, a, j, 4), (kseed, batch))] for j in range(13)]
            axis = params.get('kspace_phase_axis', 0)
            axis = int(2 * Q[1][2]) if axis == 'random' else axis
            P = W if axis else H
            d['axis'][a, b] = axis
            if smax and Q[0][0] < params.get('motion_prob', 1.0):
                flat = Q[3] + Q[4]
                br = sorted(int(flat[s - 1] * P) for s in range(1, S))
                home = sum(1 for t in br if t <= P // 2)
                d['motion'][a, b], d['breaks'][a, b] = True, br
                for s in range(S):
                    if s != home:
                        q = Q[5 + s // 2]
                        d['shifts'][a, b, s] = ((2 * q[2 * (s % 2)] - 1) * smax, (2 * q[2 * (s % 2) + 1] - 1) * smax)
            if params.get('ghost_count_range') is not None and Q[0][1] < params.get('ghost_prob', 1.0):
                (lo, hi), (alo, ahi) = params['ghost_count_range'], params['ghost_intensity_range']
                d['ghost'][a, b], d['n'][a, b], d['a'][a, b] = True, lo + int(Q[1][3] * (hi - lo + 1)), alo + Q[2][0] * (ahi - alo)
            if params.get('gibbs_cutoff_range') is not None and Q[0][2] < params.get('gibbs_prob', 1.0):
                lo, hi = params['gibbs_cutoff_range']
                d['gibbs'][a, b], d['f'][a, b] = True, lo + Q[2][1] * (hi - lo)
            if kmax and Q[0][3] < params.get('spike_prob', 1.0):
                lo, hi = params['spike_intensity_range']
                d['spike'][a, b], d['K'][a, b] = True, 1 + int(Q[2][2] * kmax)
                for i in range(d['K'][a, b]):
                    q = Q[9 + i]
                    d['spikes'][a, b, i] = (int(q[0] * H) - H // 2, int(q[1] * W) - W // 2, lo + q[2] * (hi - lo), 2.0 * np.pi * q[3])
            if rmax and Q[1][0] < params.get('rician_prob', 1.0):
                d['rician'][a, b], d['std'][a, b] = True, Q[1][1] * rmax
    return d


def table(d, a, H, W):
    """[B,48] fp64 of image array a (include/mmseg_hip.h)"""
    B, S = d['axis'].shape[1], d['shifts'].shape[2]
    t = np.zeros((B, P_COLS))
    for b in range(B):
        t[b, 0] = sum(v for k, v in FLAGS.items() if d[k][a, b])
        t[b, 1] = d['axis'][a, b]
        if d['motion'][a, b]:
            t[b, 2] = S - 1
            t[b, 3:3 + S - 1] = d['breaks'][a, b]
            t[b, 10:10 + 2 * S] = d['shifts'][a, b].ravel()
        t[b, 26], t[b, 27] = d['n'][a, b], 1.0 - d['a'][a, b]
        t[b, 28] = d['f'][a, b] * d['f'][a, b] * (H * H * W * W)
        t[b, 29] = d['K'][a, b]
        for i in range(4):
            ky, kx, s, phi = d['spikes'][a, b, i]
            t[b, 30 + 4 * i:34 + 4 * i] = (ky % H, kx % W, s * np.cos(phi), s * np.sin(phi))
        t[b, 46] = d['std'][a, b]
    return t


def freqs(n):
    """signed frequencies: u < ceil(n / 2) ? u : u - n"""
    k = np.arange(n)
    return np.where(k < (n + 1) // 2, k, k - n)


def spectrum(x):
    """x [H,W,C] fp32 -> (X [C,H,W] complex fp64 = fft2(x - lo), lo)"""
    v = np.asarray(x, np.float64)
    lo = v.min()
    return np.fft.fft2(np.moveaxis(v - lo, -1, 0), axes=(1, 2)), lo


def rule(X, row, A):
    """the rule of one sample on X [C,H,W] (a copy is returned): row = its 48 table columns, A the spikes' amplitude unit"""
    X = np.array(X, np.complex128)
    C, H, W = X.shape
    flags, axis = int(row[0]), int(row[1])
    ky, kx = np.meshgrid(freqs(H), freqs(W), indexing='ij')
    kp, P = (kx, W) if axis else (ky, H)
    if flags & FLAGS['motion']:
        breaks = row[3:3 + int(row[2])]
        seg = (breaks[None, None, :] <= (kp + P // 2)[..., None]).sum(-1)
        dy, dx = row[10 + 2 * seg], row[11 + 2 * seg]
        X = X * np.exp(-2j * np.pi * (ky * dy / H + kx * dx / W))[None]
    if flags & FLAGS['ghost']:
        n = int(row[26])
        X = X * np.where((kp % n == 0) & (kp != 0), row[27], 1.0)[None]
    if flags & FLAGS['gibbs']:
        X = X * (~(4.0 * (ky.astype(np.float64) ** 2 * W * W + kx.astype(np.float64) ** 2 * H * H) > row[28]))[None]
    if flags & FLAGS['spike']:
        for i in range(int(row[29])):
            u, v, c, s = row[30 + 4 * i:34 + 4 * i]
            u, v = int(u), int(v)
            X[:, u, v] += A * c + 1j * (A * s)
            X[:, (-u) % H, (-v) % W] += A * c - 1j * (A * s)
    return X


def rician_draw(seed, batch, b, a, H, W, C, std):
    """[C,H,W] complex: std sqrt(-2 ln u1) (cos 2 pi u2 + i sin 2 pi u2), counter (e, b, a, 5), e = (r W + c) C + ch"""
    e = np.moveaxis(np.arange(H * W * C).reshape(H, W, C), -1, 0)
    P = E.philox4x32((e, b, a, 5), (seed, batch))
    u1 = ((P[0] >> np.uint64(8)).astype(np.float64) + 1.0) * 2.0 ** -24
    u2 = (P[1] >> np.uint64(8)).astype(np.float64) * 2.0 ** -24
    r = std * np.sqrt(-2.0 * np.log(u1))
    return r * np.cos(2.0 * np.pi * u2) + 1j * (r * np.sin(2.0 * np.pi * u2))


def image(X, lo, draw=None):
    """X [C,H,W] -> (fp32 [H,W,C] = lo + |ifft2(X) + draw|, the fp64 |z| [H,W,C])"""
    z = np.fft.ifft2(X, axes=(1, 2))
    if draw is not None:
        z = z + draw
    mag = np.moveaxis(np.abs(z), 0, -1)
    return (lo + mag).astype(np.float32), mag


def spectrum_bound(y, H, W):
    """the bar on |got - ref| of a spectrum of y (any shape holding H W values per transform): C_FFT eps64 log2(H W) ||y||_2"""
    return C_FFT * EPS64 * np.log2(H * W) * np.sqrt((np.asarray(y, np.float64) ** 2).sum())


def image_bound(ynorm, row, A, H, W, mag_max, draw_max):
    """E of the module docstring for one sample: ynorm = max over the channels of ||y||_2"""
    flags = int(row[0])
    Y = ynorm + (2.0 * abs(A) * sum(np.hypot(row[32 + 4 * i], row[33 + 4 * i]) for i in range(int(row[29]))) if flags & FLAGS['spike'] else 0.)
    theta = np.pi * np.abs(row[10:26]).reshape(8, 2).sum(1).max() if flags & FLAGS['motion'] else 0.
    return EPS64 * ((2 * C_FFT * np.log2(H * W) + K_ULPS * (1 + theta)) * Y + K_ULPS * (mag_max + draw_max))


def augment(x, t, seed, batch, a):
    """x [B,H,W,C] fp32 as gathered, t = table(...) of image array a -> (fp32 [B,H,W,C], bound [B,H,W,C]); a sample whose flags are 0
    is x's bits"""
    x = np.asarray(x, np.float32)
    B, H, W, C = x.shape
    out, bound = x.copy(), np.zeros(x.shape, np.float64)
    for b in range(B):
        flags = int(t[b, 0])
        if not flags:
            continue
        X, lo = spectrum(x[b])
        y = x[b].astype(np.float64) - lo
        A = y.sum() / C
        X = rule(X, t[b], A)
        draw = rician_draw(seed, batch, b, a, H, W, C, t[b, 46]) if flags & FLAGS['rician'] else None
        out[b], mag = image(X, lo, draw)
        ynorm = np.sqrt((y ** 2).sum(axis=(0, 1))).max()
        e = image_bound(ynorm, t[b], A, H, W, mag.max(), 0. if draw is None else np.abs(draw).max())
        bound[b] = e + np.spacing(np.abs(out[b])).astype(np.float64)
    return out, bound


# ---- stand-ins of the C entry points ------------------------------------------------------------------------------------------------
def _ok(B, H, W, C):
    return B >= 1 and C >= 1 and B * C <= 65535 and extent_ok(H) and extent_ok(W) and H * W * C <= 2 ** 31 - 1


def _workspace_doubles(B, H, W, C):
    return 2 * B * C * H * W if _ok(B, H, W, C) else 0


def _forward(x, t, stats, tw, spec, B, H, W, C):
    if B <= 0:
        return 0
    if not _ok(B, H, W, C):
        return 1
    for b in range(B):
        if int(t[b, 0]):
            y = x[b].numpy().astype(np.float64) - float(stats[b, 0])
            X = np.fft.fft2(np.moveaxis(y, -1, 0), axes=(1, 2))
            spec[b].copy_(torch.from_numpy(np.stack([X.real, X.imag], axis=-1)))
    return 0


def _apply(spec, t, stats, B, H, W, C):
    if B <= 0:
        return 0
    if not _ok(B, H, W, C):
        return 1
    for b in range(B):
        if int(t[b, 0]) & 15:
            s = spec[b].numpy()
            A = (float(stats[b, 2]) - H * W * C * float(stats[b, 0])) / C
            X = rule(s[..., 0] + 1j * s[..., 1], t[b].numpy(), A)
            spec[b].copy_(torch.from_numpy(np.stack([X.real, X.imag], axis=-1)))
    return 0


def _inverse(spec, t, stats, tw, x, seed, batch, array, B, H, W, C):
    if B <= 0:
        return 0
    if not _ok(B, H, W, C):
        return 1
    for b in range(B):
        flags = int(t[b, 0])
        if flags:
            s = spec[b].numpy()
            draw = rician_draw(seed, batch, b, array, H, W, C, float(t[b, 46])) if flags & FLAGS['rician'] else None
            res, _ = image(s[..., 0] + 1j * s[..., 1], float(stats[b, 0]), draw)
            x[b].copy_(torch.from_numpy(res))
    return 0


STANDINS = {'mmseg_kspace_workspace_doubles': _workspace_doubles, 'mmseg_kspace_forward': _forward, 'mmseg_kspace_apply': _apply,
            'mmseg_kspace_inverse': _inverse}
