"""Yardstick of tests/test_volume_crf.py: a numpy restatement of the windowed mean-field CRF that refines predicted probability maps
against the image ("Maps refined against the image").  Build-defined: the reference writes no segmentation.
It shares no code with volume_predictor.py, ops.py or csrc/crf.hip.

    labels     L = K + 1: the K organ channels of prob and rest = max(0, 1 - their sum); u = log(max(P, 1e-6)); Q^0 = softmax(u)
    iteration  for every offset (dy, dx) of the (2r + 1)^2 window but the centre, over the pixels p whose neighbour q = p + (dy, dx)
               lies in the slice: a = exp(-|d|^2 / (2 theta_alpha^2) - (I_p - I_q)^2 / (2 theta_beta^2)), s = exp(-|d|^2 / (2 theta_gamma^2));
               m = w_a * sum(a Q(q)) / sum(a) + w_s * sum(s Q(q)) / sum(s), a term without neighbours being 0; Q = softmax(u + m)
    result     the K organ channels of Q^T

`refine` runs in the dtype it is given: fp64 is the yardstick, and the same lines in fp32 give e32, the error that plain fp32
arithmetic makes on a case, from which the test takes its bar.

Also here: the TEST-ONLY CPU stand-in of mmseg_crf_refine and of its workspace size (installed into tests/cpu_backend._TABLE by the
test's fixture): the fp32 restatement behind the argument checks of the entry point."""
import math

import numpy as np
import torch

FLOOR = 1e-6
PARAMS = ('radius', 'iterations', 'w_a', 'theta_alpha', 'theta_beta', 'w_s', 'theta_gamma')
DEFAULTS = (5, 5, 4.0, 3.0, 0.1, 1.0, 1.5)
LABEL_BAND = 2e-5          # an organ's fp64 value this close to 0.5 makes a pixel undecidable
FLOOR_BAR = 2e-6           # the map never needs to be better than this
MARGIN = 8.0               # times e32: another order of summation, hardware exp / log


def with_defaults(**kw):
    return tuple(kw.get(name, DEFAULTS[i]) for i, name in enumerate(PARAMS))


def labels_of(prob, K, dtype=np.float64):
    """prob [N,H,W,C] -> [N,H,W,K+1]: the organ channels and the rest"""
    organs = np.asarray(prob)[..., :K].astype(dtype)
    rest = np.maximum(dtype(0), dtype(1) - organs.sum(-1, keepdims=True, dtype=dtype))
    return np.concatenate([organs, rest], axis=-1)


def softmax(x):
    e = np.exp(x - x.max(-1, keepdims=True))
    return e / e.sum(-1, keepdims=True)


def unary(prob, K, dtype=np.float64):
    return np.log(np.maximum(labels_of(prob, K, dtype), dtype(FLOOR)))


def messages(Q, I, params, dtype=np.float64):
    """Q [N,H,W,L], I [N,H,W] -> m [N,H,W,L] of one iteration"""
    r, _, w_a, t_a, t_b, w_s, t_g = params
    N, H, W, L = Q.shape
    num_a, num_s = np.zeros(Q.shape, dtype), np.zeros(Q.shape, dtype)
    den_a, den_s = np.zeros((N, H, W), dtype), np.zeros((N, H, W), dtype)
    for dy in range(-r, r + 1):
        for dx in range(-r, r + 1):
            if (dy == 0 and dx == 0) or abs(dy) >= H or abs(dx) >= W:
                continue
            p = (slice(None), slice(max(0, -dy), H - max(0, dy)), slice(max(0, -dx), W - max(0, dx)))
            q = (slice(None), slice(max(0, dy), H + min(0, dy)), slice(max(0, dx), W + min(0, dx)))
            d2 = dtype(dy * dy + dx * dx)
            a = np.exp(-d2 / dtype(2 * t_a * t_a) - (I[p] - I[q]) ** 2 / dtype(2 * t_b * t_b))
            s = np.exp(-d2 / dtype(2 * t_g * t_g))
            num_a[p] += a[..., None] * Q[q]
            den_a[p] += a
            num_s[p] += s * Q[q]
            den_s[p] += s
    with np.errstate(invalid='ignore', divide='ignore'):
        m_a = np.where(den_a[..., None] > 0, num_a / den_a[..., None], dtype(0))
        m_s = np.where(den_s[..., None] > 0, num_s / den_s[..., None], dtype(0))
    return (dtype(w_a) * m_a + dtype(w_s) * m_s).astype(dtype)


def refine(prob, image, K, params, dtype=np.float64):
    """prob [N,H,W,C], image [N,H,W,1] -> [N,H,W,K] in `dtype`: the organ channels of Q^T"""
    u = unary(prob, K, dtype)
    I = np.asarray(image)[..., 0].astype(dtype)
    Q = softmax(u)
    for _ in range(params[1]):
        Q = softmax(u + messages(Q, I, params, dtype))
    assert Q.dtype == dtype
    return Q[..., :K]


# ---- CPU stand-in of the entry points (argument lists of include/mmseg_hip.h without the stream) -----------------------------------------
def _sizes_ok(N, H, W, C, K):
    return N >= 1 and H >= 1 and W >= 1 and 1 <= K <= min(C, 16) and 4 * N * H * W * C < 2 ** 31


def standin_workspace_bytes(N, H, W, K):
    return 4 * (1024 + 2 * N * H * W * (K + 1)) if _sizes_ok(N, H, W, K, K) else 0


def standin_crf_refine(prob, image, out, ws, N, H, W, C, K, radius, iterations, w_a, theta_alpha, theta_beta, w_s, theta_gamma):
    if N == 0:
        return 0
    reals = [float(np.float32(v)) for v in (w_a, theta_alpha, theta_beta, w_s, theta_gamma)]
    ok = (all(t is not None for t in (prob, image, out, ws)) and _sizes_ok(N, H, W, C, K) and 1 <= radius <= 8 and 1 <= iterations <= 20
          and all(math.isfinite(v) for v in reals) and min(reals[1], reals[2], reals[4]) > 0 and min(reals[0], reals[3]) >= 0
          and max(reals[0], reals[3]) > 0)
    if not ok or out.data_ptr() in (prob.data_ptr(), image.data_ptr()) or ws.numel() * ws.element_size() < standin_workspace_bytes(N, H, W, K):
        return 1
    params = (int(radius), int(iterations), reals[0], reals[1], reals[2], reals[3], reals[4])
    got = refine(prob.numpy().reshape(N, H, W, C), image.numpy().reshape(N, H, W, 1), K, params, np.float32)
    out.copy_(torch.from_numpy(np.ascontiguousarray(got)).reshape(out.shape))
    return 0


STANDINS = {'mmseg_crf_refine_workspace_bytes': standin_workspace_bytes, 'mmseg_crf_refine': standin_crf_refine}
