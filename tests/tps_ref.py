"""References for tests/test_tps_edges.py: the stages of the thin-plate-spline warp (csrc/tps.hip) in fp64, each with the error
budget that the stage's own sums give, and a numpy emulator of the fixed-point scatter that predicts d_vol bit for bit.

Every function takes the kernel's own fp32 inputs of that stage (cast to double here), so no stage inherits another one's rounding:
in particular `loc` is always the array the kernel wrote, and both sides take the same floor().  Nothing in this file calls the
product package.
"""
import numpy as np
import torch

from oracle import ops as O

EPS = 2.0 ** -24            # unit round-off of fp32
FX_BITS = 36                # csrc/tps.hip: TPS_FX_SCALE = 2^36
FX_RANGE = 2.0 ** 27        # the 64-bit sum is exact below this magnitude


def loc_reference(Mb, theta, H, W):
    """loc (x, y) in pixels, [B, HW, 2] fp64, from the fp32 basis and offsets, and its tolerance per sample [B, 1, 1] (pixels).

    The kernel adds 25 products to row / (H - 1) and scales: the terms are bounded by 1 + rowsum * max|theta| (normalised units),
    32 roundings of that cover the division, the 25-term dot product, the addition and the scaling by (W - 1) or (H - 1)."""
    B = theta.shape[0]
    Mb, th = Mb.double(), theta.double().reshape(B, 25, 2)
    q = O.nd_grid((H, W), torch.float64)[0]
    ln = q[None] + torch.einsum('pj,bjk->bpk', Mb, th)
    loc = torch.flip(ln, dims=[-1]) * torch.tensor([W - 1, H - 1], dtype=torch.float64)
    rowsum = Mb.abs().sum(1).max()
    tol = 32 * EPS * (1 + rowsum * th.abs().amax(dim=(1, 2))) * (max(H, W) - 1)
    return loc, tol.reshape(B, 1, 1)


def _taps(loc, H, W):
    """the four taps of every pixel, in the kernel's order: [(index [B, N] into H*W, valid [B, N], wx, wy)] in fp64.
    The oracle's rule: floor in int64 (no clamp needed), a tap outside the image contributes nothing."""
    x, y = loc[..., 0], loc[..., 1]
    fx, fy = torch.floor(x), torch.floor(y)
    ax, ay = x - fx, y - fy
    fxi, fyi = fx.long(), fy.long()
    taps = []
    for t in range(4):
        xi, yi = fxi + (t & 1), fyi + (t >> 1)
        ok = (xi >= 0) & (xi < W) & (yi >= 0) & (yi < H)
        idx = yi.clamp(0, H - 1) * W + xi.clamp(0, W - 1)
        taps.append((idx, ok, ax if t & 1 else 1 - ax, ay if t >> 1 else 1 - ay))
    return taps


def gather_reference(vol, loc):
    """out [B, HW, C] fp64 = resampler(vol, loc) and sum_taps w * |src| per element (the magnitude the fp32 products and the four
    additions of the kernel round against)."""
    v, l = vol.double(), loc.double()
    return O.resampler(v, l), O.resampler(v.abs(), l)


def backward_reference(vol, loc, dout):
    """fp64 autograd of the resampler at the kernel's loc -> dict with
      dvol [B, H, W, C], dloc [B, HW, 2],
      dloc_mag [B, HW, 1]  : sum_taps sum_c |g_c * src_c|  (valid taps)
      dvol_n   [B, H, W, C]: number of valid taps landing on the element (a scatter of ones)
      dvol_mag [B, H, W, C]: sum of |g * wx * wy| over those taps"""
    B, H, W, C = vol.shape
    v = vol.double().clone().requires_grad_(True)
    l = loc.double().clone().requires_grad_(True)
    g = dout.double().reshape(B, H * W, C)
    gv, gl = torch.autograd.grad(O.resampler(v, l), [v, l], g)
    flat = vol.double().reshape(B, H * W, C)
    mag = torch.zeros(B, H * W, 1, dtype=torch.float64)
    n = torch.zeros(B, H * W, C, dtype=torch.float64)
    cm = torch.zeros(B, H * W, C, dtype=torch.float64)
    for idx, ok, wx, wy in _taps(loc.double(), H, W):
        okf = ok.double()[..., None]
        ix = idx[..., None].expand(-1, -1, C)
        mag += (g * torch.gather(flat, 1, ix)).abs().sum(-1, keepdim=True) * okf
        n.scatter_add_(1, ix, okf.expand(-1, -1, C).contiguous())
        cm.scatter_add_(1, ix, (g * (wx * wy)[..., None]).abs() * okf)
    return dict(dvol=gv, dloc=gl, dloc_mag=mag, dvol_n=n.reshape(B, H, W, C), dvol_mag=cm.reshape(B, H, W, C))


def dvol_tolerance(ref):
    """n roundings of a contribution to 2^-36 (2^-37 each) + the two fp32 multiplications of every contribution and the final
    rounding to fp32 (3 * 2^-24 of the sum of magnitudes)"""
    return ref['dvol_n'] * 2.0 ** -(FX_BITS + 1) + 3 * EPS * ref['dvol_mag']


def scatter_emulator(loc, dout, H, W):
    """tps_warp_bwd_tiled_kernel + tps_fx_to_float_kernel in numpy: fp32 loc [B, HW, 2] and dout [B, H, W, C] -> fp32 d_vol
    [B, H, W, C], the bits the device must produce.

    Per valid tap (g * wx) * wy in fp32 (two multiplications, nothing to contract), widened to fp64, scaled by 2^36 (exact),
    rounded to nearest-even, added into int64 (order-free), then int64 -> fp64 -> * 2^-36 -> fp32.  The floor is clamped to
    [-2, W] x [-2, H] before the conversion to an integer, as in the kernel."""
    loc = loc.detach().cpu().numpy().astype(np.float32, copy=False)
    B = loc.shape[0]
    C = dout.shape[-1]
    g = dout.detach().cpu().numpy().astype(np.float32, copy=False).reshape(B, H * W, C)
    x, y = loc[..., 0], loc[..., 1]
    fxf, fyf = np.floor(x), np.floor(y)
    ax, ay = (x - fxf).astype(np.float32), (y - fyf).astype(np.float32)
    fx = np.clip(fxf, np.float32(-2), np.float32(W)).astype(np.int64)
    fy = np.clip(fyf, np.float32(-2), np.float32(H)).astype(np.int64)
    one = np.float32(1)
    acc = np.zeros(B * H * W * C, np.int64)
    bi = np.broadcast_to(np.arange(B, dtype=np.int64)[:, None], fx.shape)
    ch = np.arange(C, dtype=np.int64)
    for t in range(4):
        xi, yi = fx + (t & 1), fy + (t >> 1)
        ok = (xi >= 0) & (xi < W) & (yi >= 0) & (yi < H)
        wx = (ax if t & 1 else one - ax).astype(np.float32)
        wy = (ay if t >> 1 else one - ay).astype(np.float32)
        v = ((g * wx[..., None]).astype(np.float32) * wy[..., None]).astype(np.float32)
        fixed = np.rint(v.astype(np.float64) * 2.0 ** FX_BITS).astype(np.int64)
        base = ((bi * H + yi) * W + xi) * C
        np.add.at(acc, (base[ok][:, None] + ch[None]).ravel(), fixed[ok].ravel())
    out = (acc.astype(np.float64) * 2.0 ** -FX_BITS).astype(np.float32)
    return torch.from_numpy(out.reshape(B, H, W, C))


def dtheta_reference(Mb, dloc, H, W, per):
    """dtheta [B, 25, 2] fp64 from the kernel's dloc, and its tolerance per entry: a chunk is walked sequentially (per terms), the
    final stage adds 16 + 16 terms -> (per + 32) roundings of the sum of magnitudes"""
    Mb = Mb.double()
    glr = torch.flip(dloc.double() * torch.tensor([W - 1, H - 1], dtype=torch.float64), dims=[-1])
    ref = torch.einsum('pj,bpk->bjk', Mb, glr)
    mag = torch.einsum('pj,bpk->bjk', Mb.abs(), glr.abs())
    return ref, (per + 32) * EPS * mag
