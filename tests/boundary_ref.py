"""numpy / scipy restatement (fp64) of the boundary loss of csrc/boundary.hip -- the signed distance map phi, the term L_B and its
gradient -- the mask contents the tests run on, and TEST-ONLY torch-CPU stand-ins of the new entry points (registered into
tests.cpu_backend._TABLE by a fixture of tests/test_boundary_loss.py; never a fallback of the product).

phi is `one_hot2dist` of the code of Kervadec et al. (MIDL 2019) over scipy.ndimage.distance_transform_edt:
    phi = edt(~mask) * ~mask - (edt(mask) - 1) * mask,   0 everywhere for an empty mask (theirs) and for a full one (defined here:
scipy's result without any background pixel is meaningless).  The squared distances are taken from the feature indices scipy returns,
so they are exact integers whatever the rounding of its fp64 distances."""
import functools

import numpy as np
import torch
from scipy.ndimage import distance_transform_edt, gaussian_filter

MAXC, MAXHW, CHUNKS = 8, 2048, 128

CONTENTS = ('empty', 'full', 'corner_pixel', 'centre_hole', 'checkerboard', 'half_plane', 'smooth_noise', 'blob_two_edges',
            'far_blobs', 'threshold_049_051')


# ---- the map --------------------------------------------------------------------------------------------------------------------------
def squared_distance_to_zero(mask):
    """per pixel of a 2-D bool array the squared distance to the nearest False pixel, as int64 (the array must hold one)"""
    idx = distance_transform_edt(mask, return_distances=False, return_indices=True)
    ii, jj = np.indices(mask.shape)
    return (idx[0].astype(np.int64) - ii) ** 2 + (idx[1].astype(np.int64) - jj) ** 2


def phi_one(mask):
    """2-D bool -> (phi fp64, squared distance int64 to the nearest pixel of the OTHER class; -1 where there is none)"""
    mask = np.asarray(mask, bool)
    if not mask.any() or mask.all():
        return np.zeros(mask.shape, np.float64), np.full(mask.shape, -1, np.int64)
    sq_bg = squared_distance_to_zero(mask)          # of the foreground pixels: to the nearest background pixel
    sq_fg = squared_distance_to_zero(~mask)         # of the background pixels: to the nearest foreground pixel
    sq = np.where(mask, sq_bg, sq_fg)
    d = np.sqrt(sq.astype(np.float64))
    return np.where(mask, -(d - 1.0), d), sq


def phi_ref(target, nm):
    """target [B,H,W,C] -> (phi [B,H,W,nm] fp64, sq [B,H,W,nm] int64, fg [B,H,W,nm] bool)"""
    target = np.asarray(target)
    B, H, W, C = target.shape
    phi = np.zeros((B, H, W, nm), np.float64)
    sq = np.zeros((B, H, W, nm), np.int64)
    fg = target[..., :nm] > 0.5
    for b in range(B):
        for k in range(nm):
            phi[b, ..., k], sq[b, ..., k] = phi_one(fg[b, ..., k])
    return phi, sq, fg


def phi_f32(target, nm):
    """what the kernel computes, step by step in fp32: the rounded root of the exact integer, then the '- 1'"""
    _, sq, fg = phi_ref(target, nm)
    r = np.sqrt(np.maximum(sq, 0).astype(np.float64)).astype(np.float32)      # fp32 sqrt == rounded fp64 sqrt for integers < 2^24
    out = np.where(fg, -(r - np.float32(1.0)), r).astype(np.float32)
    out[sq < 0] = 0.0
    return out


# ---- the term and its gradient --------------------------------------------------------------------------------------------------------
def loss_ref(pred, phi, nm):
    """-> (L_B, sum |p * phi| / N) in fp64"""
    p = np.asarray(pred, np.float64)[..., :nm]
    f = np.asarray(phi, np.float64)
    n = float(f.size)
    return float((p * f).sum() / n), float(np.abs(p * f).sum() / n)


def loss_bound(B, HW, nm, abs_mean):
    """the rounding bound of mmseg_boundary_loss as written, to first order in u = 2^-24:
       stage 1: a thread takes ceil(ceil(HW / 128) / 256) pixels of its chunk, nm fused multiply-adds each (one rounding per element);
                block_sum is a 6-level butterfly over the wave and a 6-level butterfly over the (at most 64) wave sums: depth 12;
       stage 2: a thread adds ceil(128 B / 256) partials, the same 12-level block_sum, and one division by N.
       Every element passes through at most that many roundings, each relative to a partial sum bounded by sum |p * phi|."""
    per = -(-HW // CHUNKS)
    seq1 = -(-per // 256) * nm
    seq2 = -(-(B * CHUNKS) // 256)
    return (seq1 + 12 + seq2 + 12 + 1) * 2.0 ** -24 * abs_mean


def grad_scale_f32(scale_host, scale_dev, weight, count):
    """s of mmseg_boundary_grad_add in its documented order, every step rounded to fp32"""
    s = np.float32(scale_host)
    if scale_dev is not None:
        s = np.float32(s * np.float32(scale_dev))
    s = np.float32(s * np.float32(weight))
    return np.float32(s / np.float32(count))


def grad_add_f32(phi, dpred, nm, scale_host, scale_dev, weight):
    out = np.array(dpred, np.float32, copy=True)
    s = grad_scale_f32(scale_host, scale_dev, weight, phi.size)
    out[..., :nm] = out[..., :nm] + (s * np.asarray(phi, np.float32)).astype(np.float32)
    return out


# ---- mask contents --------------------------------------------------------------------------------------------------------------------
def mask_content(kind, H, W, rng, variant=0):
    """one 2-D bool mask of the named kind; `variant` moves the feature between the slots of a batch"""
    ii, jj = np.indices((H, W))
    if kind == 'empty':
        return np.zeros((H, W), bool)
    if kind == 'full':
        return np.ones((H, W), bool)
    if kind == 'corner_pixel':
        m = np.zeros((H, W), bool)
        m[(0, H - 1, 0, H - 1)[variant % 4], (0, W - 1, W - 1, 0)[variant % 4]] = True
        return m
    if kind == 'centre_hole':
        m = np.ones((H, W), bool)
        m[H // 2, W // 2] = False
        return m
    if kind == 'checkerboard':
        return (ii + jj + variant) % 2 == 0
    if kind == 'half_plane':
        return (jj < W // 2) if variant % 2 == 0 else (ii >= H // 2)
    if kind in ('smooth_noise', 'threshold_049_051'):
        return gaussian_filter(rng.standard_normal((H, W)), 3) > 0.05
    if kind == 'blob_two_edges':
        r = 0.6 * min(H, W) + 1.0
        ci, cj = ((0, 0), (H - 1, W - 1), (0, W - 1), (H - 1, 0))[variant % 4]
        return (ii - ci) ** 2 + (jj - cj) ** 2 <= r * r
    if kind == 'far_blobs':
        m = np.zeros((H, W), bool)
        s = 1 + variant % 3
        if variant % 2 == 0:
            m[:s, :s] = True
            m[H - s:, W - s:] = True
        else:
            m[:s, W - s:] = True
            m[H - s:, :s] = True
        return m
    raise ValueError(kind)


@functools.lru_cache(maxsize=None)
def case(shape, kind):
    """-> dict(target fp32 [B,H,W,C], phi fp64, sq, fg, phi32) for one (B,H,W,C,nm) and content; computed once and shared (read-only)"""
    B, H, W, C, nm = shape
    rng = np.random.RandomState(1000 + CONTENTS.index(kind) * 97 + (H * 31 + W * 7 + C + nm) % 89)
    t = (rng.rand(B, H, W, C) > 0.5).astype(np.float32)          # channels >= nm: anything, they are not read
    for b in range(B):
        for k in range(nm):
            t[b, ..., k] = mask_content(kind, H, W, rng, b * nm + k)
    if kind == 'threshold_049_051':
        t = np.where(t > 0.5, np.float32(0.51), np.float32(0.49)).astype(np.float32)
        t[0, 0, 0, 0] = 0.5                                       # exactly 0.5 is background
    phi, sq, fg = phi_ref(t, nm)
    out = dict(target=t, phi=phi, sq=sq, fg=fg, phi32=phi_f32(t, nm))
    for v in out.values():
        v.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def softmax_pred(shape, seed=5):
    B, H, W, C, nm = shape
    x = np.random.RandomState(seed).standard_normal((B, H, W, C))
    e = np.exp(x - x.max(-1, keepdims=True))
    p = (e / e.sum(-1, keepdims=True)).astype(np.float32)
    p.setflags(write=False)
    return p


# ---- torch-CPU stand-ins of the entry points (same argument lists, tensors instead of pointers) ----------------------------------------
def _map_ok(B, H, W, nm):
    return 1 <= B <= 65535 and 1 <= H <= MAXHW and 1 <= W <= MAXHW and 1 <= nm <= MAXC


def boundary_workspace_bytes(B, H, W, nm):
    return B * H * W * nm * 4 if _map_ok(B, H, W, nm) else 0


def boundary_map(target, phi, ws, B, H, W, C, nm):
    if target is None or phi is None or ws is None or not _map_ok(B, H, W, nm) or nm > C or C > MAXC:
        return 1
    phi.copy_(torch.from_numpy(phi_f32(target.reshape(B, H, W, C).numpy(), nm)).reshape(phi.shape)); return 0


def boundary_loss_workspace_floats(B):
    return B * CHUNKS if 1 <= B <= 65535 else 0


def boundary_loss(pred, phi, loss_b, ws, B, HW, C, nm):
    if pred is None or phi is None or loss_b is None or ws is None or B < 1 or HW < 1 or nm < 1 or nm > C or C > MAXC:
        return 1
    v = (pred.reshape(B, HW, C)[..., :nm].double() * phi.reshape(B, HW, nm).double()).sum() / float(B * HW * nm)
    loss_b.copy_(v.float().reshape(1)); return 0


def boundary_grad_add(phi, dpred, B, HW, C, nm, scale_host, scale_dev, weight_dev):
    if phi is None or dpred is None or weight_dev is None or B < 1 or HW < 1 or nm < 1 or nm > C or C > MAXC:
        return 1
    s = torch.tensor(scale_host, dtype=torch.float32)
    if scale_dev is not None:
        s = s * scale_dev[0]
    s = (s * weight_dev[0]) / torch.tensor(float(B * HW * nm), dtype=torch.float32)
    d = dpred.reshape(B, HW, C)
    d[..., :nm] += s * phi.reshape(B, HW, nm)
    return 0


def boundary_combine(loss, loss_b, weight_dev):
    if loss is None or loss_b is None or weight_dev is None:
        return 1
    loss.add_(weight_dev * loss_b); return 0


STANDINS = {'mmseg_' + f.__name__: f for f in (boundary_workspace_bytes, boundary_map, boundary_loss_workspace_floats, boundary_loss,
                                               boundary_grad_add, boundary_combine)}
