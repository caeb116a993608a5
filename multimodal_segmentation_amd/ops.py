"""Operators of the DAFNet/MMSDNet step: thin autograd nodes around the gfx950 kernels of libmmseg_hip.so.

torch is used for device memory (torch.empty), the stream and the autograd tape that stitches the nodes; every
arithmetic operation on activations, gradients and weights is a kernel of csrc/*.hip reached through
_native.call (C ABI, include/mmseg_hip.h).  Layout: NHWC fp32 (the reference's layout), weights in Keras
layout (conv HWIO, dense [in, out]).
"""
import collections
import math

import numpy as np
import torch

from . import _native as N
from .parallel import dp

ACT = {None: 0, 'linear': 0, 'relu': 1, 'leaky': 2, 'tanh': 3}
BN_EPS = 1e-3        # keras BatchNormalization default
BN_MOMENTUM = 0.99   # keras BatchNormalization default
IN_EPS = 1e-3        # keras_contrib InstanceNormalization default

_workspaces = {}


def _sid(device):
    """identity of the stream the next launches go to: scratch buffers and cached weight images are per stream, so that independent
    phases of an iteration may run on concurrent streams (conf.multi_stream) without sharing mutable scratch memory"""
    if device.type != 'cuda':
        return 0
    from . import graphs
    st = graphs._recording
    if st is not None and st.mode == 'capture':
        return ('graph', st.uid)       # a recorded step owns its scratch: torch records every graph on one shared capture stream,
                                       # and two recorded steps may later be replayed on concurrent streams
    return torch.cuda.current_stream(device).cuda_stream


def _ws(tag, n, device, dtype=torch.float32):
    """Grow-only scratch buffer of at least n elements per (tag, device, stream); a tag keeps to one dtype.  The kernels of one stream
    run in order, so a buffer can be handed to the next kernel as soon as the previous launch has been queued."""
    key = (tag, device, _sid(device))
    buf = _workspaces.get(key)
    n = max(int(n), 1)
    if buf is None or buf.numel() < n:
        buf = torch.empty(max(n, 1024), dtype=dtype, device=device)
        _workspaces[key] = buf
    return buf


def _new(shape, like, dtype=torch.float32):
    return torch.empty(shape, dtype=dtype, device=like.device)


# ---- reduced-precision STORAGE of the convolutional trunk (build-defined; BASELINE configs #3 / #5) ------------------------------
_act16 = [None]      # torch.bfloat16 / torch.float16 while 16-bit activation storage is on, else None
_HCODE = {torch.float32: 0, torch.bfloat16: 1, torch.float16: 2}


def set_activation_storage(on):
    """conf.act_storage = 'half': the activations and gradients of the MFMA trunk (UNet conv - BatchNorm - ReLU chains incl. pooling,
    up-sampling and skips; the segmentor's first block) live in HBM in the 16-bit type of the active precision mode.  Master
    weights, weight gradients, statistics, softmax / rounding, losses, Adam and the all-reduce stay fp32.  Needs
    set_conv_precision('bf16' | 'fp16') first.  Returns the previous setting."""
    old = _act16[0]
    if not on:
        _act16[0] = None
        return old is not None
    mode = N.call('mmseg_get_conv_precision')
    if mode == 0:
        raise ValueError("16-bit activation storage needs compute_dtype 'bf16' or 'fp16'")
    _act16[0] = torch.bfloat16 if mode == 1 else torch.float16
    return old is not None


def act16_dtype():
    return _act16[0]


def _h(t):
    """element code of a tensor for the `_t` entry points: 0 fp32, 1 bf16, 2 fp16"""
    return 0 if t is None else _HCODE[t.dtype]


def _c(t):
    return t if t.is_contiguous() else t.contiguous()


# ------------------------------------------------------------------------------------------------------
# convolution
# ------------------------------------------------------------------------------------------------------
_PRECISIONS = ['fp32', 'bf16', 'fp16']


def set_conv_precision(mode):
    """'fp32' (default), 'bf16' or 'fp16': precision of the MFMA products of the fast-path convolutions (operands
    rounded to the 16-bit type, fp32 accumulation; tensors in HBM, weight gradients, normalisation, losses and the optimiser
    stay fp32).  Returns the previous mode."""
    old = N.call('mmseg_set_conv_precision', _PRECISIONS.index(mode))
    if _PRECISIONS[old] != mode:
        bump_weight_version()           # the fast-path weight images hold elements of the operand type: cached ones are stale
    return _PRECISIONS[old]


class precision_scope(object):
    """`with precision_scope((compute_dtype, act16)):` -- run the enclosed launches in the precision of ONE model: the kernel library's
    mode (and the storage type of the trunk) is set on entry and put back on exit.  Trainers and `predict` enter the scope of the
    model they belong to, so models of different precisions can live in one process without the caller juggling the library-wide
    switch (round-2 review); `None` leaves whatever is set."""

    def __init__(self, precision):
        self.precision = precision

    def __enter__(self):
        self.prev = None
        if self.precision is not None:
            mode, act16 = self.precision
            cur = (_PRECISIONS[N.call('mmseg_get_conv_precision')], _act16[0] is not None)
            if cur != (mode, bool(act16)):
                self.prev = cur
                set_conv_precision(mode)
                set_activation_storage(bool(act16))
        return self

    def __exit__(self, *exc):
        if self.prev is not None:
            set_activation_storage(False)
            set_conv_precision(self.prev[0])
            set_activation_storage(self.prev[1])
        return False


def _conv_geometry(H, W, KH, KW, stride, padding):
    if padding == 'same':
        if stride != 1 or KH % 2 == 0 or KW % 2 == 0:
            raise ValueError("'same' is implemented for stride 1 and odd kernels (all the reference uses)")
        return H, W, KH // 2, KW // 2
    if padding == 'valid':
        return (H - KH) // stride + 1, (W - KW) // stride + 1, 0, 0
    raise ValueError(padding)


_weight_version = [0]
_wprep_cache = {}


_bn_state_version = [0]      # bumped whenever BatchNorm moving statistics may have changed (training-mode forward)
_bnfold_cache = {}


_owner_version = {}          # nn.Model.uid -> version of that model's weights (bumped by its optimiser steps only)


_wprep_batch = {}            # nn.Model.uid -> {'ents': {cache key: (src ptr, image, taps, Cin, Cout, mode, wkey)}, 'table': tensor | None, 'blocks': int}
_wprep_batch_on = [True]     # False: every image is re-laid out lazily by its own launch again (tests compare the two)


def _wprep_register(key, wkey, w, out, ntaps, Cin, Cout, mode):
    """remember a cached mode 0 / 1 image of a model's parameter: the model's next optimiser step refreshes all of them in ONE launch"""
    if not (isinstance(wkey, tuple) and len(wkey) == 2 and isinstance(wkey[0], int) and mode in (0, 1) and w.is_cuda):
        return
    b = _wprep_batch.setdefault(wkey[1], {'ents': {}, 'table': None, 'blocks': 0})
    ent = b['ents'].get(key)
    if ent is None or ent[0] != w.data_ptr() or ent[1] is not out:
        b['ents'][key] = (w.data_ptr(), out, ntaps, Cin, Cout, mode, wkey)
        b['table'] = None


def _wprep_refresh(owner):
    """all registered images of `owner`'s parameters in one launch (mmseg_conv2d_wprep_batch), stamped with the current version"""
    b = _wprep_batch.get(owner)
    if not b or not b['ents'] or not _wprep_batch_on[0]:
        return
    if torch.cuda.is_current_stream_capturing():
        return
    ents = list(b['ents'].items())
    dev = ents[0][1][1].device
    if b['table'] is None:
        rows, blk = [], 0
        for _, (src, out, ntaps, Cin, Cout, mode, _wk) in ents:
            rows.append([src, out.data_ptr(), ntaps, Cin, Cout, mode, blk, 0])
            blk += ntaps * ((Cin + 31) // 32) * ((Cout + 31) // 32)
        rows.append([0, 0, 0, 0, 0, 0, blk, 0])
        b['table'] = torch.tensor(rows, dtype=torch.int64).to(dev)
        b['blocks'] = blk
    N.call('mmseg_conv2d_wprep_batch', b['table'], len(ents), b['blocks'])
    for key, ent in ents:
        _wprep_cache[key] = (_wver(ent[6]), ent[1])


def bump_weight_version(owner=None):
    """Invalidate the cached weight re-layouts (called whenever weights change: optimiser step, set_weights).  `owner` = id of the
    nn.Model whose arena changed: only the images of ITS parameters become stale -- a discriminator's Adam step no longer makes the
    generator's ~100 forward images stale (they were re-laid out three times per iteration: after the generator step and again
    after the mask- and image-discriminator steps).  Without `owner` everything is invalidated (set_weights, precision switch,
    graph capture, broadcast)."""
    if owner is None:
        _weight_version[0] += 1
        _wprep_batch.clear()         # arenas may have moved (set_weights, broadcast): the images re-register as they are re-laid out
    else:
        _owner_version[owner] = _owner_version.get(owner, 0) + 1
        _wprep_refresh(owner)
    _bn_state_version[0] += 1


def _key_owner(key):
    """Model.uid a cache key belongs to, or None (keys start with the wkey = (Param.uid | ('pair', Param.uid), Model.uid))"""
    wk = key[0]
    return wk[1] if isinstance(wk, tuple) and len(wk) == 2 else None


def evict_owner(owner):
    """Drop every cached weight image / fused operand / BatchNorm fold of the model with this uid (nn.Model registers this as its
    finaliser): a process that builds many models does not keep the images of the dead ones in HBM."""
    for cache in (_wprep_cache, _pair_cache, _bnfold_cache):
        for k in [k for k in cache if _key_owner(k) == owner]:
            del cache[k]
    _wprep_batch.pop(owner, None)
    _owner_version.pop(owner, None)


def release_caches(workspaces=True):
    """Forget every cached weight image, fused operand and BatchNorm fold (they are rebuilt on demand) and, optionally, the
    grow-only scratch buffers of all streams.  Must not be called while a recorded hipGraph that owns scratch is alive."""
    _wprep_cache.clear()
    _pair_cache.clear()
    _bnfold_cache.clear()
    _wprep_batch.clear()
    _elastic_weights.clear()
    if workspaces:
        _workspaces.clear()


def release_graph_workspaces(uid):
    """the scratch buffers a recorded step owned (graphs.FitGraph registers this as its finaliser)"""
    sid = ('graph', uid)
    for k in [k for k in _workspaces if k[2] == sid]:
        del _workspaces[k]
    for cache in (_wprep_cache, _pair_cache, _bnfold_cache):       # ... and the weight images written inside the recording
        for k in [k for k in cache if k[-1] == sid]:
            del cache[k]
    for b in _wprep_batch.values():
        stale = [k for k in b['ents'] if k[-1] == sid]
        for k in stale:
            del b['ents'][k]
        if stale:
            b['table'] = None


def cache_footprint():
    """(entries, bytes) held by the caches and the scratch buffers -- for leak checks"""
    n = b = 0
    for cache in (_wprep_cache, _pair_cache, _bnfold_cache):
        for ent in cache.values():
            for t in ent[1:]:
                if isinstance(t, torch.Tensor):
                    n, b = n + 1, b + t.numel() * t.element_size()
    for t in _workspaces.values():
        n, b = n + 1, b + t.numel() * t.element_size()
    return n, b


def _wver(wkey):
    """version stamp of a cached image: (global version, version of the owning model); wkey = (Param.uid, Model.uid) -- serial
    numbers that are never reused (object ids are recycled by the interpreter, device addresses by the caching allocator)"""
    if isinstance(wkey, tuple):
        return (_weight_version[0], _owner_version.get(wkey[1], 0))
    return (_weight_version[0], 0)


def _wprep(w, KH, KW, Cin, Cout, mode, wkey=None):
    """[N][K] re-layout of a conv kernel for the fast path (mode 0: forward, 1: data gradient).  Cached per weight
    version when the caller identifies the weight (`wkey`, a parameter of an nn.Model whose arena is stable and whose
    every update bumps the version); anonymous weights are re-laid out on every call."""
    if wkey is None:
        out = _ws('wprep%d' % mode, w.numel(), w.device)[:w.numel()]
        N.call('mmseg_conv2d_wprep', w, out, KH, KW, Cin, Cout, mode)
        return out
    key = (wkey, w.data_ptr(), mode, _sid(w.device))
    ent = _wprep_cache.get(key)
    if ent is not None and ent[0] == _wver(wkey) and ent[1].numel() == w.numel():
        return ent[1]
    out = ent[1] if (ent is not None and ent[1].numel() == w.numel()) else torch.empty(w.numel(), dtype=torch.float32, device=w.device)
    N.call('mmseg_conv2d_wprep', w, out, KH, KW, Cin, Cout, mode)
    _wprep_cache[key] = (_wver(wkey), out)
    _wprep_register(key, wkey, w, out, KH * KW, Cin, Cout, mode)
    return out


def _wprep_col8(w, Cout, wkey=None):
    """fast-path weight image of a 3x3 kernel with 8 input channels read as a 1x1 kernel over the 96-column im2col rows of
    mmseg_im2col8_t: [72][Cout] + 24 zero rows -> [Cout][96]; cached per weight version like _wprep"""
    key = (wkey, w.data_ptr(), 'col8', _sid(w.device))
    ent = _wprep_cache.get(key) if wkey is not None else None
    if ent is not None and ent[0] == _wver(wkey):
        return ent[1]
    if ent is not None:
        pad, out = ent[2], ent[1]
    else:
        pad = torch.zeros(96 * Cout, dtype=torch.float32, device=w.device)
        out = torch.empty(96 * Cout, dtype=torch.float32, device=w.device)
    pad[:72 * Cout].copy_(w.reshape(-1))
    N.call('mmseg_conv2d_wprep', pad, out, 1, 1, 96, Cout, 0)
    if wkey is not None:
        _wprep_cache[key] = (_wver(wkey), out, pad)
    return out


def _wprep_parity_all(w, KH, KW, Cin, Cout, stride, taps, wkey=None):
    """The sub-kernels of all stride x stride parity classes back to back in (ph, pw) raster order (the operand of
    mmseg_conv2d_dgrad_parity_all); cached per weight version like _wprep."""
    sizes = [taps[0][qh] * taps[1][qw] * Cin * Cout for qh in range(stride) for qw in range(stride)]
    n = sum(sizes)
    key = (wkey, w.data_ptr(), 'parity_all', stride, _sid(w.device))
    ent = _wprep_cache.get(key) if wkey is not None else None
    if ent is not None and ent[0] == _wver(wkey) and ent[1].numel() == n:
        return ent[1]
    if wkey is None:
        out = _ws('wprep_parity_all', n, w.device)[:n]
    else:
        out = ent[1] if (ent is not None and ent[1].numel() == n) else torch.empty(n, dtype=torch.float32, device=w.device)
    N.call('mmseg_conv2d_wprep_parity_all', w, out, KH, KW, Cin, Cout, stride)
    if wkey is not None:
        _wprep_cache[key] = (_wver(wkey), out)
    return out


def _wprep_ups(w, C1, Cout, which, wkey=None):
    """Weight images of an up-sampled 3x3 layer with the up-sampling folded in (mmseg_conv2d_wprep_ups): which 0 = the four forward
    class images (operand of mmseg_conv2d_fwd_ups_parity), which 1 = the 4x4 stride-2 data-gradient image; cached per weight version
    like _wprep_parity_all."""
    n = 16 * C1 * Cout
    key = (wkey, w.data_ptr(), 'ups', which, _sid(w.device))
    ent = _wprep_cache.get(key) if wkey is not None else None
    if ent is not None and ent[0] == _wver(wkey) and ent[1].numel() == n:
        return ent[1]
    if wkey is None:
        out = _ws('wprep_ups%d' % which, n, w.device)[:n]
    else:
        out = ent[1] if (ent is not None and ent[1].numel() == n) else torch.empty(n, dtype=torch.float32, device=w.device)
    N.call('mmseg_conv2d_wprep_ups', w, out, C1, Cout, which)
    if wkey is not None:
        _wprep_cache[key] = (_wver(wkey), out)
    return out


def _ups_fold(x1, x2, w, stride, padding, ups, out_dtype):
    """the layer is one the folded up-sampling route may take (UpSampling2D(2) -> 3x3 'same' convolution, one fp32 input on the MFMA
    fast path); mmseg_conv2d_ups_fold_ok then decides per direction"""
    if not (ups and x2 is None and stride == 1 and padding == 'same' and tuple(w.shape[:2]) == (3, 3)):
        return False
    if not (x1.dtype == w.dtype == out_dtype == torch.float32):
        return False
    return bool(N.call('mmseg_conv2d_fast_path', x1.shape[3], 0, w.shape[3], 0))


def _ups_fold_ok(x1, Cout, direction):
    B, H1, W1, C1 = x1.shape
    return bool(N.call('mmseg_conv2d_ups_fold_ok', B, H1, W1, C1, Cout, direction))


def _wprep_wino(w, Cin, Cout, wkey=None):
    """Winograd F(2x2,3x3) weight image U [16][Cout][Cin] of a 3x3 layer (mmseg_conv2d_wprep_wino, 16/9 of the layer's weights); cached
    per weight version like _wprep_ups."""
    n = 16 * Cin * Cout
    key = (wkey, w.data_ptr(), 'wino', _sid(w.device))
    ent = _wprep_cache.get(key) if wkey is not None else None
    if ent is not None and ent[0] == _wver(wkey) and ent[1].numel() == n:
        return ent[1]
    if wkey is None:
        out = _ws('wprep_wino', n, w.device)[:n]
    else:
        out = ent[1] if (ent is not None and ent[1].numel() == n) else torch.empty(n, dtype=torch.float32, device=w.device)
    N.call('mmseg_conv2d_wprep_wino', w, out, Cin, Cout)
    if wkey is not None:
        _wprep_cache[key] = (_wver(wkey), out)
    return out


def _wino_ok(x1, x2, w, ups, out_dtype):
    """the inference forward of this layer takes the Winograd route: a 3x3 'same' fp32 layer without up-sampling that
    mmseg_conv2d_wino_ok admits (mode, precision, shape)"""
    if ups or tuple(w.shape[:2]) != (3, 3):
        return False
    if not (x1.dtype == w.dtype == out_dtype == torch.float32) or (x2 is not None and x2.dtype != torch.float32):
        return False
    B, H, W, C1 = x1.shape
    C2 = x2.shape[3] if x2 is not None else 0
    if not N.call('mmseg_conv2d_fast_path', C1, C2, w.shape[3], 0):      # the products run on the fast path's body
        return False
    return bool(N.call('mmseg_conv2d_wino_ok', B, H, W, C1, C2, w.shape[3]))


def _winof_ok(x1, x2, w, ups, out_dtype):
    """the inference forward of this layer, whose caller opted in (`rounded`), takes the fused Winograd route: a 3x3 'same' fp32 layer
    without up-sampling that mmseg_conv2d_winof_ok admits (mode, precision, shape)"""
    if ups or tuple(w.shape[:2]) != (3, 3):
        return False
    if not (x1.dtype == w.dtype == out_dtype == torch.float32) or (x2 is not None and x2.dtype != torch.float32):
        return False
    B, H, W, C1 = x1.shape
    C2 = x2.shape[3] if x2 is not None else 0
    if not N.call('mmseg_conv2d_fast_path', C1, C2, w.shape[3], 0):      # (a backend without the MFMA fast path has no fused route either)
        return False
    return bool(N.call('mmseg_conv2d_winof_ok', B, H, W, C1, C2, w.shape[3]))


def _conv_fwd_raw(x1, x2, w, wt, bias, y, y2, B, H, W, C1, C2, Ho, Wo, Cout, KH, KW, stride, ph, pw, ups, transposed,
                  act, alpha, nsplit1):
    # host-side shape checks: the kernel trusts these numbers
    assert x1.numel() == B * (H >> ups) * (W >> ups) * C1, 'x1 shape/geometry mismatch'
    assert (x2 is None and C2 == 0) or x2.numel() == B * H * W * C2, 'x2 shape/geometry mismatch'
    assert (w if w is not None else wt).numel() == KH * KW * (C1 + C2) * Cout, 'kernel shape mismatch'
    assert bias is None or bias.numel() == Cout
    if y2 is None:
        assert y.numel() == B * Ho * Wo * Cout
    else:
        assert y.numel() == B * Ho * Wo * nsplit1 and y2.numel() == B * Ho * Wo * (Cout - nsplit1)
    io = (1 if _h(x1) else 0) | (2 if _h(x2) else 0) | (4 if _h(y) else 0)
    if io:      # 16-bit tensors in HBM (reduced-precision storage)
        assert y2 is None or _h(y2) == _h(y)
        N.call('mmseg_conv2d_fwd_t', x1, x2, w, wt, bias, y, y2, B, H, W, C1, C2, Ho, Wo, Cout, KH, KW, stride, ph, pw,
               ups, transposed, act, float(alpha), nsplit1, io)
        return
    N.call('mmseg_conv2d_fwd', x1, x2, w, wt, bias, y, y2, B, H, W, C1, C2, Ho, Wo, Cout, KH, KW, stride, ph, pw,
           ups, transposed, act, float(alpha), nsplit1)


def _grad_done(*grads):
    """Tell the data-parallel tracker that the launches accumulating into these gradient-arena views have been queued
    (parallel/dp.py: the arena's all-reduce starts when its last accumulation is in the stream)."""
    tr = dp.current_tracker()
    if tr is None:
        return
    for t in grads:
        owner = getattr(t, '_owner', None) if t is not None else None
        if owner is not None:
            tr.done(owner, getattr(t, '_seg', 0))


def _accumulate(dst, src):
    """dst += src (weight-gradient accumulation into the gradient arena)."""
    N.call('mmseg_axpby', dst, src, dst, dst.numel(), 1.0, 1.0)


def _wgrad_launch(x1, x2, g, dw_flat, B, H, W, C1, C2, Ho, Wo, Cout, KH, KW, stride, ph, pw, ups, accumulate):
    """dW (+)= weight gradient of a convolution; x1 / x2 / g as they are stored (fp32 or the 16-bit storage type)"""
    need = N.call('mmseg_conv2d_wgrad_workspace', B, Ho, Wo, C1 + C2, Cout, KH, KW)
    ws = _ws('wgrad', need, g.device)
    if (_h(x1) or _h(x2) or _h(g)) and N.call('mmseg_conv2d_wgrad_t_supported', Ho, Wo, stride, C1, C2, Cout):
        # 16-bit operands in HBM: the transposed-staging kernel reads them as they are
        assert x2 is None or _h(x2) == _h(x1)
        N.call('mmseg_conv2d_wgrad_t', x1, x2, g, dw_flat, ws, ws.numel(), B, H, W, C1, C2, Ho, Wo, Cout, KH, KW,
               stride, ph, pw, ups, accumulate, (1 if _h(x1) else 0) | (4 if _h(g) else 0))
    elif _h(x1) or _h(x2) or _h(g):
        # geometry the 16-bit kernel does not take (tiny planes): widen the operands (a copy, no arithmetic)
        f = lambda t: t if t is None or _h(t) == 0 else t.float()
        N.call('mmseg_conv2d_wgrad', f(x1), f(x2), f(g), dw_flat, ws, ws.numel(), B, H, W, C1, C2, Ho, Wo, Cout, KH, KW,
               stride, ph, pw, ups, accumulate)
    else:
        N.call('mmseg_conv2d_wgrad', x1, x2, g, dw_flat, ws, ws.numel(), B, H, W, C1, C2, Ho, Wo, Cout, KH, KW,
               stride, ph, pw, ups, accumulate)


class _Conv2d(torch.autograd.Function):
    """inputs: activations x1 [, x2], the tape anchor, then non-differentiable arguments.  Weight / bias gradients
    are accumulated into `wgrad` / `bgrad` (views of the owner's gradient arena) instead of being returned."""

    @staticmethod
    def forward(ctx, x1, x2, anchor, w, bias, stride, padding, act, alpha, ups, wgrad, bgrad, wkey, out_dtype=torch.float32):
        x1 = _c(x1)
        x2 = _c(x2) if x2 is not None else None
        B, H1, W1, C1 = x1.shape
        H, W = (H1 * 2, W1 * 2) if ups else (H1, W1)
        C2 = 0 if x2 is None else x2.shape[3]
        if x2 is not None:
            assert x2.shape[:3] == (B, H, W)
        KH, KW, Cin, Cout = w.shape
        assert Cin == C1 + C2, 'kernel expects %d input channels, got %d' % (Cin, C1 + C2)
        Ho, Wo, ph, pw = _conv_geometry(H, W, KH, KW, stride, padding)
        y = _new((B, Ho, Wo, Cout), x1, out_dtype)
        prec = N.call('mmseg_get_conv_precision')
        fold = _ups_fold(x1, x2, w, stride, padding, ups, out_dtype)
        if fold and _ups_fold_ok(x1, Cout, 0):
            # nearest x2 + 3x3: four parity classes, each a 2x2 convolution of x with summed weights -- 4 of the 9 multiplications
            N.call('mmseg_conv2d_fwd_ups_parity', x1, _wprep_ups(w, C1, Cout, 0, wkey), bias, None, y, B, H1, W1, C1, Cout,
                   ACT[act], float(alpha))
        elif prec and C1 == 8 and C2 == 0 and KH == 3 and KW == 3 and stride == 1 and not ups and (Ho, Wo, ph, pw) == (H, W, 1, 1) \
                and Cout % 64 == 0 and _h(x1) in (0, prec) and B * H * W * 96 * 2 < (1 << 31) - 64:
            # reduced-precision modes, 8 input channels (the SPADE units' shared convolution, the segmentor's first): K = 72 is three
            # gathers of the generic kernel per output tile; instead the 72 (+24 zero) operand columns of every pixel are written
            # once as 16-bit rows and the product runs as a 1x1 convolution on the 16-bit MFMA fast path
            if W % 32 == 0 and _h(y) in (0, prec) and ACT[act] <= 2 and N.call('mmseg_conv16_mode', -1) != 0:
                # round 4: one launch, no im2col tensor -- a lane's MFMA operand is one pixel's 8 channels of one tap, read as it lies;
                # the weights stay in registers (conv8h_kernel, csrc/conv16.hpp)
                assert w.numel() == 72 * Cout and (bias is None or bias.numel() == Cout) and y.numel() == B * H * W * Cout
                N.call('mmseg_conv8h_fwd_t', x1, w, bias, y, B, H, W, Cout, ACT[act], float(alpha), _h(x1), _h(y))
            else:
                half = torch.bfloat16 if prec == 1 else torch.float16
                xcol = torch.empty((B, H, W, 96), dtype=half, device=x1.device)
                N.call('mmseg_im2col8_t', x1, xcol, B, H, W, _h(x1), prec)
                _conv_fwd_raw(xcol, None, None, _wprep_col8(w, Cout, wkey), bias, y, None, B, H, W, 96, 0, Ho, Wo, Cout, 1, 1, 1, 0, 0, 0, 0,
                              ACT[act], alpha, 0)
        else:
            wt = _wprep(w, KH, KW, Cin, Cout, 0, wkey) if N.call('mmseg_conv2d_fast_path', C1, C2, Cout, 0) else None
            _conv_fwd_raw(x1, x2, w, wt, bias, y, None, B, H, W, C1, C2, Ho, Wo, Cout, KH, KW, stride, ph, pw, int(ups), 0,
                          ACT[act], alpha, 0)
        ctx.geom = (B, H, W, C1, C2, Ho, Wo, Cout, KH, KW, stride, ph, pw, int(ups), ACT[act], alpha)
        ctx.wgrad, ctx.bgrad, ctx.wkey = wgrad, bgrad, wkey
        ctx.fold = fold
        ctx.w = w     # plain (non-leaf) weight view: not tracked by autograd
        ctx.save_for_backward(x1, x2, y if ACT[act] else None)
        return y

    @staticmethod
    def backward(ctx, dy):
        x1, x2, y = ctx.saved_tensors
        w = ctx.w
        B, H, W, C1, C2, Ho, Wo, Cout, KH, KW, stride, ph, pw, ups, act, alpha = ctx.geom
        dy = _c(dy)
        M = B * Ho * Wo
        bias_done = False
        if act:
            assert _h(dy) == _h(y), 'the gradient of a tensor is stored like the tensor'
            g = _new(dy.shape, dy, dy.dtype)      # act16_bwd_kernel stores dx with dy's element type
            if ctx.bgrad is not None and Cout % 64 == 0:
                # activation gradient and bias gradient (column sums of g) in one pass over dy / y
                ws = _ws('colsum', N.call('mmseg_colsum_workspace_floats', M, Cout), dy.device)
                N.call('mmseg_act_bwd_bias_t', dy, y, g, ctx.bgrad, ws, M, Cout, act, float(alpha), 1, _h(dy))
                bias_done = True
            elif _h(dy):
                N.call('mmseg_act_bwd_bias_t', dy, y, g, None, None, M, Cout, act, float(alpha), 0, _h(dy))
            else:
                N.call('mmseg_act_bwd', dy, y, g, dy.numel(), act, float(alpha))
        else:
            g = dy
        need_x1, need_x2 = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        dx1 = dx2 = None
        if ctx.bgrad is not None and not bias_done:
            ws = _ws('colsum', N.call('mmseg_colsum_workspace_floats', M, Cout), dy.device)
            N.call('mmseg_colsum', g if _h(g) == 0 else g.float(), ctx.bgrad, ws, M, Cout, 1.0, 1)
        fold = ctx.fold and g.dtype == torch.float32
        if ctx.wgrad is not None and fold and _ups_fold_ok(x1, Cout, 2):
            # folded up-sampling: the weight gradient of the 4x4 stride-2 convolution g -> dx (x in the role of its output gradient)
            # into scratch, then folded onto the 3x3 kernel and added to the gradient-arena view
            dwe = _ws('ups_dwe', 16 * C1 * Cout, g.device)[:16 * C1 * Cout]
            _wgrad_launch(g, None, x1, dwe, B, H, W, Cout, 0, H // 2, W // 2, C1, 4, 4, 2, 1, 1, 0, 0)
            N.call('mmseg_conv2d_ups_wgrad_fold', dwe, ctx.wgrad.view(-1), C1, Cout)
        elif ctx.wgrad is not None:
            # accumulates straight into the gradient-arena view (the final slab reduction adds to it)
            _wgrad_launch(x1, x2, g, ctx.wgrad.view(-1), B, H, W, C1, C2, Ho, Wo, Cout, KH, KW, stride, ph, pw, ups, 1)
        _grad_done(ctx.wgrad, ctx.bgrad)
        if need_x1 and fold and _ups_fold_ok(x1, Cout, 1):
            # folded up-sampling: dx at the low resolution directly, one 4x4 stride-2 convolution over g with summed weights (no
            # full-resolution gradient, no pooling pass)
            dx1 = _new((B, H // 2, W // 2, C1), dy, x1.dtype)
            _conv_fwd_raw(g, None, None, _wprep_ups(w, C1, Cout, 1, ctx.wkey), None, dx1, None, B, H, W, Cout, 0, H // 2, W // 2, C1,
                          4, 4, 2, 1, 1, 0, 0, 0, 0.0, 0)
            return (dx1, None) + (None,) * 12
        if need_x1 or (x2 is not None and need_x2):
            Cin = C1 + C2
            tr = 1 if stride > 1 else 0
            d1 = _new((B, H, W, C1), dy, x1.dtype)          # a gradient is stored like its tensor
            d2 = _new((B, H, W, C2), dy, x2.dtype) if C2 else None
            assert d2 is None or d2.dtype == d1.dtype
            taps = [[N.call('mmseg_conv2d_parity_taps', k, stride, q) for q in range(stride)] for k in (KH, KW)] if tr else None
            if tr and stride == 2 and KH == 4 and KW == 4 and ph == 0 and pw == 0 and C2 == 0 and not ups and Cout == 64 and \
                    Cin in (1, 4) and N.call('mmseg_conv2d_fast_path', 64, 0, 64, 0):
                # first layer of a discriminator: N = Cin GEMM -> direct kernel
                N.call('mmseg_conv2d_dgrad_s2k4_smallc', g, w, d1, B, H, W, Cin, Ho, Wo, Cout)
            elif stride == 1 and C2 == 0 and not ups and Cin % 4 == 0 and Cin <= 16 and KH * KW > 1 and KH * KW * Cin <= 256 and \
                    not (Cin == 8 and Cout == 8) and N.call('mmseg_conv2d_fast_path', Cout, 0, KH * KW * Cin, 0):
                # few input channels: ONE 1x1 GEMM of the gradient against all taps (N = taps * Cin instead of a 32-wide tile
                # that is mostly padding, dy read once instead of once per tap), then the shifted planes are summed
                nt = KH * KW * Cin
                T = _ws('dgrad_taps', B * Ho * Wo * nt, dy.device)[:B * Ho * Wo * nt]
                # the Keras kernel [KH, KW, Cin, Cout] read as [taps * Cin][Cout] IS the fast layout of that 1x1 convolution
                # (in the reduced-precision modes the image holds 16-bit elements: converted copy, cached like the other images)
                wimg = w.reshape(-1) if N.call('mmseg_get_conv_precision') == 0 else _wprep(w, KH, KW, Cin, Cout, 2, ctx.wkey)
                _conv_fwd_raw(g, None, None, wimg, None, T, None, B, Ho, Wo, Cout, 0, Ho, Wo, nt, 1, 1, 1, 0, 0, 0, 0, 0, 0.0, 0)
                N.call('mmseg_conv2d_dgrad_tapsum', T, d1, B, H, W, Ho, Wo, Cin, KH, KW, ph, pw)
            elif tr and stride == 2 and C2 == 0 and not ups and N.call('mmseg_conv2d_fast_path', Cout, 0, Cin, 0) and \
                    min(taps[0] + taps[1]) > 0:
                # strided convolution: the parity classes of the input pixels, each an exact stride-1 convolution, batched
                # into one launch (a single class does not fill the chip)
                wp = _wprep_parity_all(w, KH, KW, Cin, Cout, stride, taps, ctx.wkey)
                N.call('mmseg_conv2d_dgrad_parity_all', g, wp, d1, B, Ho, Wo, Cout, H, W, Cin, KH, KW, stride)
            else:
                if N.call('mmseg_conv2d_fast_path', Cout, 0, Cin, tr):
                    wf, wt = None, _wprep(w, KH, KW, Cin, Cout, 1, ctx.wkey)     # [Cin][flipped taps][Cout]
                else:
                    wf, wt = _ws('wflip', w.numel(), dy.device)[:w.numel()], None
                    N.call('mmseg_conv2d_wflip', w, wf, KH, KW, Cin, Cout)
                # data gradient = convolution of g with the flipped kernel; fractionally strided when stride > 1
                _conv_fwd_raw(g, None, wf, wt, None, d1, d2, B, Ho, Wo, Cout, 0, H, W, Cin, KH, KW, stride, KH - 1 - ph,
                              KW - 1 - pw, 0, tr, 0, 0.0, C1 if C2 else 0)
            if ups:
                dx1 = _new((B, H // 2, W // 2, C1), dy, d1.dtype)
                if _h(d1):
                    N.call('mmseg_upsample2_bwd_t', d1, dx1, B, H // 2, W // 2, C1, _h(d1))
                else:
                    N.call('mmseg_upsample2_bwd', d1, dx1, B, H // 2, W // 2, C1)
            else:
                dx1 = d1
            dx2 = d2
        return (dx1, dx2) + (None,) * 12


def conv2d_bn_infer(x, w, cbias, gamma, beta, mov_mean, mov_var, relu=False, x2=None, upsample=False, wkey=None,
                    out_dtype=torch.float32, rounded=False):
    """`predict` of Conv2D -> BatchNormalization [-> ReLU] as ONE launch: the moving statistics are folded into a
    per-channel scale and bias of the convolution epilogue (no tape: inference only).
    `rounded`: the caller's promise that every consumer sees this output only through a Rounding layer (the anatomy encoders'
    `predict`), so that last-bit differences reach no loss and no weight; only then may the fused Winograd kernel
    (mmseg_conv2d_fwd_winof) take the layer."""
    x1 = _c(x)
    x2 = _c(x2) if x2 is not None else None
    B, H1, W1, C1 = x1.shape
    H, W = (2 * H1, 2 * W1) if upsample else (H1, W1)
    C2 = x2.shape[3] if x2 is not None else 0
    KH, KW, Cin, Cout = w.shape
    assert Cin == C1 + C2
    Ho, Wo, ph, pw = _conv_geometry(H, W, KH, KW, 1, 'same')
    # folded scale / bias: cached per layer until the weights or the moving statistics change (a pool evaluates every
    # encoder layer four times per iteration with the same parameters)
    key = (wkey, gamma.data_ptr(), 'bnfold', _sid(gamma.device))
    ent = _bnfold_cache.get(key) if wkey is not None else None
    if ent is not None and ent[0] == (_wver(wkey), _bn_state_version[0]):
        ss = ent[1]
    else:
        ss = ent[1] if ent is not None else _new((2, Cout), x1)
        N.call('mmseg_bn_infer_fold', gamma, beta, mov_mean, mov_var, cbias, ss[0], ss[1], Cout, BN_EPS)
        if wkey is not None:
            _bnfold_cache[key] = ((_wver(wkey), _bn_state_version[0]), ss)
    y = _new((B, Ho, Wo, Cout), x1, out_dtype)
    if _ups_fold(x1, x2, w, 1, 'same', upsample, out_dtype) and _ups_fold_ok(x1, Cout, 3):
        N.call('mmseg_conv2d_fwd_ups_parity', x1, _wprep_ups(w, C1, Cout, 0, wkey), ss[1], ss[0], y, B, H1, W1, C1, Cout,
               ACT['relu' if relu else None], 0.0)
        return y
    if rounded and _winof_ok(x1, x2, w, upsample, out_dtype):
        N.call('mmseg_conv2d_fwd_winof', x1, x2, _wprep_wino(w, Cin, Cout, wkey), ss[1], ss[0], y, B, H, W, C1, C2, Cout,
               ACT['relu' if relu else None], 0.0)
        return y
    if _wino_ok(x1, x2, w, upsample, out_dtype):
        need = N.call('mmseg_conv2d_wino_workspace', B, H, W, C1, C2, Cout)
        ws = _ws('wino', need, x1.device)
        N.call('mmseg_conv2d_fwd_wino', x1, x2, _wprep_wino(w, Cin, Cout, wkey), ss[1], ss[0], y, B, H, W, C1, C2, Cout,
               ACT['relu' if relu else None], 0.0, ws, ws.numel())
        return y
    wt = _wprep(w, KH, KW, Cin, Cout, 0, wkey) if N.call('mmseg_conv2d_fast_path', C1, C2, Cout, 0) else None
    io = (1 if _h(x1) else 0) | (2 if _h(x2) else 0) | (4 if _h(y) else 0)
    if io:
        N.call('mmseg_conv2d_fwd_scaled_t', x1, x2, w, wt, ss[1], ss[0], y, B, H, W, C1, C2, Ho, Wo, Cout, KH, KW, 1, ph, pw,
               int(bool(upsample)), ACT['relu' if relu else None], 0.0, io)
    else:
        N.call('mmseg_conv2d_fwd_scaled', x1, x2, w, wt, ss[1], ss[0], y, B, H, W, C1, C2, Ho, Wo, Cout, KH, KW, 1, ph, pw,
               int(bool(upsample)), ACT['relu' if relu else None], 0.0)
    return y


def conv2d(x, w, bias=None, stride=1, padding='same', act=None, alpha=0.0, x2=None, upsample=False,
           wgrad=None, bgrad=None, anchor=None, wkey=None, out_dtype=torch.float32):
    """keras Conv2D on NHWC (+ fused nearest x2 up-sampling of x, + fused channel concat with x2, + fused
    bias/activation epilogue).  `wgrad`/`bgrad`: gradient-arena views to accumulate into (None = frozen)."""
    if upsample and (x.shape[3] % 4 != 0):
        raise ValueError('fused up-sampling needs C % 4 == 0')
    if wgrad is None and bgrad is None:
        anchor = None
    return _Conv2d.apply(x, x2, anchor, w, bias, stride, padding, act, alpha, bool(upsample), wgrad, bgrad, wkey, out_dtype)


# ------------------------------------------------------------------------------------------------------
# batch norm (+ReLU)
# ------------------------------------------------------------------------------------------------------
class _BatchNormTrain(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, anchor, gamma, beta, mov_mean, mov_var, relu, ggrad, bgrad, out_dtype=torch.float32):
        _bn_state_version[0] += 1          # the moving statistics are about to change: folded inference parameters are stale
        x = _c(x)
        C = x.shape[-1]
        M = x.numel() // C
        stats = _new((4, C), x)  # mean, invstd, scale, shift
        ws = _ws('norm', N.call('mmseg_norm_workspace_floats', C), x.device)
        ctx.sync = dp.sync_bn()
        hx, hy = _h(x), _HCODE[out_dtype]
        ctx.h = (hx, hy)
        if hx or hy:       # 16-bit storage of the input and / or the output (csrc/act16.hip): same arithmetic, 8-byte accesses
            assert not ctx.sync, 'sync_bn and 16-bit activation storage are not combined'
            N.call('mmseg_bn_stats_t', x, gamma, beta, stats[0], stats[1], stats[2], stats[3], mov_mean, mov_var, ws, M, C,
                   BN_EPS, BN_MOMENTUM, hx)
            y = _new(x.shape, x, out_dtype)
            N.call('mmseg_bn_apply_t', x, stats[2], stats[3], y, M, C, int(relu), hx, hy)
            ctx.relu = bool(relu)
            ctx.gamma, ctx.ggrad, ctx.bgrad = gamma, ggrad, bgrad
            ctx.save_for_backward(x, y if relu else None, stats)
            return y
        if ctx.sync:
            # statistics over the global batch: (mean, biased variance) of this rank's rows, gathered in rank order, combined
            local = _new((2, C), x)
            N.call('mmseg_bn_stats_local', x, local, ws, M, C)
            gathered = dp.all_gather_rows(local.reshape(-1))
            N.call('mmseg_bn_stats_combine', gathered, dp.world_size(), gamma, beta, stats[0], stats[1], stats[2], stats[3],
                   mov_mean, mov_var, M * dp.world_size(), C, BN_EPS, BN_MOMENTUM)
        else:
            N.call('mmseg_bn_stats', x, gamma, beta, stats[0], stats[1], stats[2], stats[3], mov_mean, mov_var, ws, M, C,
                   BN_EPS, BN_MOMENTUM)
        y = _new(x.shape, x)
        N.call('mmseg_bn_apply', x, stats[2], stats[3], y, M, C, int(relu))
        ctx.relu = bool(relu)
        ctx.gamma, ctx.ggrad, ctx.bgrad = gamma, ggrad, bgrad
        ctx.save_for_backward(x, y if (relu and ctx.sync) else None, stats)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, y, stats = ctx.saved_tensors
        dy = _c(dy)
        C = x.shape[-1]
        M = x.numel() // C
        dx = _new(x.shape, x, x.dtype)
        coef = _ws('bn_coef', 3 * C, x.device)
        ws = _ws('norm', N.call('mmseg_norm_workspace_floats', C), x.device)
        if ctx.h != (0, 0):
            assert (ctx.ggrad is None) == (ctx.bgrad is None), 'BatchNorm gamma and beta are trained or frozen together'
            N.call('mmseg_bn_bwd_t', dy, y, x, ctx.gamma, stats[0], stats[1], dx, ctx.ggrad, ctx.bgrad, coef, ws, M, C, int(ctx.relu), 1,
                   ctx.h[0], ctx.h[1])
            _grad_done(ctx.ggrad, ctx.bgrad)
            return (dx,) + (None,) * 9
        if ctx.sync:
            # sums of this rank -> dgamma / dbeta (averaged over ranks with the other weight gradients); sums over all ranks -> dx
            local = _new((2, C), x)
            N.call('mmseg_bn_bwd_sums', dy, y, x, stats[0], stats[1], local, ws, M, C, int(ctx.relu))
            glob = dp.all_reduce_sum(local.clone())
            if ctx.ggrad is not None and ctx.bgrad is not None:
                N.call('mmseg_bn_bwd_finish', local, glob, ctx.gamma, stats[0], stats[1], ctx.ggrad, ctx.bgrad, coef, C,
                       M * dp.world_size(), 1)
            else:
                assert ctx.ggrad is None and ctx.bgrad is None, 'BatchNorm gamma and beta are trained or frozen together'
                N.call('mmseg_bn_bwd_finish', local, glob, ctx.gamma, stats[0], stats[1], None, None, coef, C, M * dp.world_size(), 0)
            N.call('mmseg_bn_bwd_apply', dy, y, x, coef, dx, M, C, int(ctx.relu))
            _grad_done(ctx.ggrad, ctx.bgrad)
            return (dx,) + (None,) * 9
        # (the ReLU mask is recomputed from x with the forward pass's scale / shift: the saved output is not read again)
        if ctx.ggrad is not None and ctx.bgrad is not None:
            # the final reduction adds dgamma / dbeta straight into the gradient-arena views
            N.call('mmseg_bn_bwd_x', dy, x, stats[2], stats[3], ctx.gamma, stats[0], stats[1], dx, ctx.ggrad, ctx.bgrad, coef, ws, M, C,
                   int(ctx.relu), 1)
        else:
            tmp = _ws('bn_dgb', 2 * C, x.device)
            dgamma, dbeta = tmp[:C], tmp[C:2 * C]
            N.call('mmseg_bn_bwd_x', dy, x, stats[2], stats[3], ctx.gamma, stats[0], stats[1], dx, dgamma, dbeta, coef, ws, M, C,
                   int(ctx.relu), 0)
            if ctx.ggrad is not None:
                _accumulate(ctx.ggrad, dgamma)
            if ctx.bgrad is not None:
                _accumulate(ctx.bgrad, dbeta)
        _grad_done(ctx.ggrad, ctx.bgrad)
        return (dx,) + (None,) * 9


def batchnorm(x, gamma, beta, mov_mean, mov_var, training, relu=False, ggrad=None, bgrad=None, anchor=None,
              out_dtype=torch.float32):
    """keras BatchNormalization(axis=-1) [+ ReLU].  training: batch statistics and in-place moving-average update
    (what `fit` does); otherwise the moving statistics (what `predict` does)."""
    if training:
        if ggrad is None and bgrad is None:
            anchor = None
        return _BatchNormTrain.apply(x, anchor, gamma, beta, mov_mean, mov_var, relu, ggrad, bgrad, out_dtype)
    x = _c(x)
    C = x.shape[-1]
    M = x.numel() // C
    ss = _new((2, C), x)
    N.call('mmseg_bn_infer_prep', gamma, beta, mov_mean, mov_var, ss[0], ss[1], C, BN_EPS)
    y = _new(x.shape, x, out_dtype)
    if _h(x) or _h(y):
        N.call('mmseg_bn_apply_t', x, ss[0], ss[1], y, M, C, int(relu), _h(x), _h(y))
    else:
        N.call('mmseg_bn_apply', x, ss[0], ss[1], y, M, C, int(relu))
    return y


# ------------------------------------------------------------------------------------------------------
# pooling / softmax / rounding
# ------------------------------------------------------------------------------------------------------
class _MaxPool2(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        x = _c(x)
        B, H, W, C = x.shape
        y = _new((B, H // 2, W // 2, C), x, x.dtype)
        if _h(x):
            N.call('mmseg_maxpool2_fwd_t', x, y, B, H, W, C, _h(x))
        else:
            N.call('mmseg_maxpool2_fwd', x, y, B, H, W, C)
        ctx.save_for_backward(x, y)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, y = ctx.saved_tensors
        B, H, W, C = x.shape
        dx = _new(x.shape, x, x.dtype)
        if _h(x):
            N.call('mmseg_maxpool2_bwd_t', x, y, _c(dy), dx, B, H, W, C, _h(x))
        else:
            N.call('mmseg_maxpool2_bwd', x, y, _c(dy), dx, B, H, W, C)
        return dx


def maxpool2(x):
    return _MaxPool2.apply(x)


class _MaxPool2Skip(torch.autograd.Function):
    """-> (MaxPooling2D(2)(x), x): a down-path activation of the UNet feeds the pooling AND the skip Concatenate (reference
    models/unet.py:39-51,69-84).  Handing out the second use from the same node lets the backward pass add the two gradients inside
    the pooling-gradient kernel (one pass) instead of the autograd engine adding them with a torch kernel afterwards."""

    @staticmethod
    def forward(ctx, x):
        ctx.set_materialize_grads(False)
        x = _c(x)
        B, H, W, C = x.shape
        y = _new((B, H // 2, W // 2, C), x, x.dtype)
        if _h(x):
            N.call('mmseg_maxpool2_fwd_t', x, y, B, H, W, C, _h(x))
        else:
            N.call('mmseg_maxpool2_fwd', x, y, B, H, W, C)
        ctx.save_for_backward(x, y)
        return y, x.view_as(x)

    @staticmethod
    def backward(ctx, dy, dskip):
        if dy is None:
            return dskip
        x, y = ctx.saved_tensors
        B, H, W, C = x.shape
        dx = _new(x.shape, x, x.dtype)
        add = _c(dskip) if dskip is not None else None
        assert add is None or add.dtype == x.dtype, 'the gradient of a tensor is stored like the tensor'
        N.call('mmseg_maxpool2_bwd_add_t', x, y, _c(dy), add, dx, B, H, W, C, _h(x))
        return dx


def maxpool2_skip(x):
    """-> (pooled, skip): `skip` is x for its second consumer (see _MaxPool2Skip)"""
    return _MaxPool2Skip.apply(x)


class _Upsample2(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        x = _c(x)
        B, H, W, C = x.shape
        y = _new((B, 2 * H, 2 * W, C), x)
        N.call('mmseg_upsample2_fwd', x, y, B, H, W, C)
        ctx.shape = (B, H, W, C)
        return y

    @staticmethod
    def backward(ctx, dy):
        B, H, W, C = ctx.shape
        dx = _new(ctx.shape, dy)
        N.call('mmseg_upsample2_bwd', _c(dy), dx, B, H, W, C)
        return dx


def upsample2(x):
    """keras UpSampling2D(size=2) (nearest)."""
    return _Upsample2.apply(x)


class _Subsample(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, f):
        x = _c(x)
        B, H, W, C = x.shape
        assert H % f == 0 and W % f == 0
        y = _new((B, H // f, W // f, C), x)
        N.call('mmseg_subsample_fwd', x, y, B, H // f, W // f, C, f)
        ctx.meta = (B, H, W, C, f)
        return y

    @staticmethod
    def backward(ctx, dy):
        B, H, W, C, f = ctx.meta
        dx = _new((B, H, W, C), dy)
        N.call('mmseg_subsample_bwd', _c(dy), dx, B, H // f, W // f, C, f)
        return dx, None


def resize_nearest_down(x, Ho, Wo):
    """tf.image.resize_nearest_neighbor(x, [Ho, Wo]) for integer down-sampling factors (src = dst * f)."""
    B, H, W, C = x.shape
    if (H, W) == (Ho, Wo):
        return x
    if H % Ho or W % Wo or H // Ho != W // Wo:
        raise NotImplementedError('nearest resize: only integer down-sampling factors (%dx%d -> %dx%d)' % (H, W, Ho, Wo))
    return _Subsample.apply(x, H // Ho)


class _SoftmaxRound(torch.autograd.Function):
    """-> (p, s): channel softmax and its half-to-even rounding with the straight-through gradient of
    layers/rounding.py:40-42 (the gradient reaching s is passed to p unchanged)."""

    @staticmethod
    def forward(ctx, x, want_round):
        x = _c(x)
        C = x.shape[-1]
        p = _new(x.shape, x)
        s = _new(x.shape, x) if want_round else None
        N.call('mmseg_softmax_fwd', x, p, s, x.numel() // C, C)
        ctx.save_for_backward(p)
        return p, s

    @staticmethod
    def backward(ctx, dp, ds):
        (p,) = ctx.saved_tensors
        C = p.shape[-1]
        if dp is None:
            g = _c(ds)
        elif ds is None:
            g = _c(dp)
        else:
            g = _new(p.shape, p)
            N.call('mmseg_axpby', _c(dp), _c(ds), g, p.numel(), 1.0, 1.0)
        dx = _new(p.shape, p)
        N.call('mmseg_softmax_bwd', g, p, dx, p.numel() // C, C)
        return dx, None


def softmax(x):
    return _SoftmaxRound.apply(x, False)[0]


def softmax_round(x):
    """-> (softmax, rounded softmax)"""
    return _SoftmaxRound.apply(x, True)


# ------------------------------------------------------------------------------------------------------
# dense
# ------------------------------------------------------------------------------------------------------
_DENSE_ROWS = 32


class _Dense(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, anchor, w, bias, act, alpha, wgrad, bgrad):
        x = _c(x)
        R, K = x.shape
        K2, Nn = w.shape
        assert K == K2, 'dense: input has %d features, kernel expects %d' % (K, K2)
        y = _new((R, Nn), x)
        for r0 in range(0, R, _DENSE_ROWS):          # the kernels keep <= 32 rows in registers: larger batches go in row groups
            r = min(_DENSE_ROWS, R - r0)
            ws = _ws('dense', N.call('mmseg_dense_workspace_floats', r, K, Nn), x.device)
            N.call('mmseg_dense_fwd', x[r0:r0 + r], w, bias, y[r0:r0 + r], ws, r, K, Nn, ACT[act], float(alpha))
        ctx.act, ctx.alpha = ACT[act], alpha
        ctx.w, ctx.wgrad, ctx.bgrad = w, wgrad, bgrad
        ctx.save_for_backward(x, y if ACT[act] else None)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, y = ctx.saved_tensors
        w = ctx.w
        R, K = x.shape
        Nn = w.shape[1]
        dy = _c(dy)
        if ctx.act:
            g = _new(dy.shape, dy)
            N.call('mmseg_act_bwd', dy, y, g, dy.numel(), ctx.act, float(ctx.alpha))
        else:
            g = dy
        dx = None
        if ctx.needs_input_grad[0]:
            dx = _new(x.shape, x)
            for r0 in range(0, R, _DENSE_ROWS):
                r = min(_DENSE_ROWS, R - r0)
                N.call('mmseg_dense_dgrad', g[r0:r0 + r], w, dx[r0:r0 + r], r, K, Nn)
        if ctx.wgrad is not None:
            for r0 in range(0, R, _DENSE_ROWS):          # accumulates straight into the gradient-arena view
                r = min(_DENSE_ROWS, R - r0)
                N.call('mmseg_dense_wgrad', x[r0:r0 + r], g[r0:r0 + r], ctx.wgrad.view(-1), r, K, Nn, 1)
        if ctx.bgrad is not None:
            ws = _ws('colsum', N.call('mmseg_colsum_workspace_floats', R, Nn), x.device)
            N.call('mmseg_colsum', g, ctx.bgrad, ws, R, Nn, 1.0, 1)
        _grad_done(ctx.wgrad, ctx.bgrad)
        return (dx,) + (None,) * 7


def dense(x, w, bias=None, act=None, alpha=0.0, wgrad=None, bgrad=None, anchor=None):
    if wgrad is None and bgrad is None:
        anchor = None
    return _Dense.apply(x, anchor, w, bias, act, alpha, wgrad, bgrad)


# ------------------------------------------------------------------------------------------------------
# FiLM (+LeakyReLU + residual add)
# ------------------------------------------------------------------------------------------------------
class _Film(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, gamma, beta, res, alpha):
        x, gamma, beta = _c(x), _c(gamma), _c(beta)
        B, H, W, C = x.shape
        assert gamma.shape == (B, C) and beta.shape == (B, C)
        y = _new(x.shape, x)
        N.call('mmseg_film_fwd', x, gamma, beta, _c(res) if res is not None else None, y, B, H * W, C, float(alpha))
        ctx.alpha, ctx.has_res = alpha, res is not None
        ctx.save_for_backward(x, gamma, beta)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, gamma, beta = ctx.saved_tensors
        B, H, W, C = x.shape
        dy = _c(dy)
        dx = _new(x.shape, x)
        dg, db = _new((B, C), x), _new((B, C), x)
        ws = _ws('film', N.call('mmseg_film_bwd_workspace', B, C), x.device)
        N.call('mmseg_film_bwd', dy, x, gamma, beta, dx, dg, db, ws, B, H * W, C, float(ctx.alpha))
        return dx, dg, db, (dy if ctx.has_res else None), None


def film(x, gamma, beta, res=None, alpha=0.3):
    """leaky_relu(x * gamma + beta, alpha) [+ res]  (layers/film.py:26-36 + decoder.py:50-53)."""
    return _Film.apply(x, gamma, beta, res, alpha)


# ------------------------------------------------------------------------------------------------------
# thin-plate-spline warp, maximum, slice, sampling
# ------------------------------------------------------------------------------------------------------
class _TpsWarp(torch.autograd.Function):
    @staticmethod
    def forward(ctx, vol, theta, Mb):
        vol, theta = _c(vol), _c(theta)
        B, H, W, C = vol.shape
        assert theta.numel() == B * 50 and Mb.shape == (H * W, 25)
        # the kernels read Mb as raw fp32 rows of 25: anything else would be read as garbage, so refuse it instead of converting
        if Mb.dtype != torch.float32 or not Mb.is_contiguous() or Mb.device != vol.device:
            raise ValueError('tps_warp: the basis Mb must be a contiguous float32 tensor on %s (got %s on %s, contiguous=%s)'
                             % (vol.device, Mb.dtype, Mb.device, Mb.is_contiguous()))
        out = _new(vol.shape, vol)
        loc = _new((B, H * W, 2), vol)
        N.call('mmseg_tps_warp_fwd', vol, theta, Mb, out, loc, B, H, W, C)
        ctx.save_for_backward(vol, loc, Mb)
        ctx.theta_shape = theta.shape
        return out

    @staticmethod
    def backward(ctx, dout):
        vol, loc, Mb = ctx.saved_tensors
        B, H, W, C = vol.shape
        dout = _c(dout)
        dvol = dtheta = None
        acc = None
        if ctx.needs_input_grad[0]:
            dvol = _new(vol.shape, vol)
            acc = _ws('tps_acc', N.call('mmseg_tps_scatter_workspace_floats', B, H, W, C), vol.device)
        dloc = None
        ws = None
        if ctx.needs_input_grad[1]:
            dtheta = _new(ctx.theta_shape, vol)
            dloc = _ws('tps_dloc', B * H * W * 2, vol.device)
            ws = _ws('tps', N.call('mmseg_tps_workspace_floats', B), vol.device)
        N.call('mmseg_tps_warp_bwd', vol, loc, Mb, dout, dvol, dtheta, dloc, ws, acc, B, H, W, C)
        return dvol, dtheta, None


def tps_warp(vol, theta, Mb):
    return _TpsWarp.apply(vol, theta, Mb)


class _Maximum(torch.autograd.Function):
    @staticmethod
    def forward(ctx, a, b):
        a, b = _c(a), _c(b)
        y = _new(a.shape, a)
        N.call('mmseg_maximum_fwd', a, b, y, a.numel())
        ctx.save_for_backward(a, b)
        return y

    @staticmethod
    def backward(ctx, dy):
        a, b = ctx.saved_tensors
        da = _new(a.shape, a) if ctx.needs_input_grad[0] else None
        db = _new(a.shape, a) if ctx.needs_input_grad[1] else None
        N.call('mmseg_maximum_bwd', a, b, _c(dy), da, db, a.numel())
        return da, db


def maximum(a, b):
    return _Maximum.apply(a, b)


class _SliceChannels(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, c0, cs):
        x = _c(x)
        C = x.shape[-1]
        y = _new(x.shape[:-1] + (cs,), x)
        N.call('mmseg_slice_fwd', x, y, x.numel() // C, C, c0, cs)
        ctx.meta = (x.shape, c0, cs)
        return y

    @staticmethod
    def backward(ctx, dy):
        shape, c0, cs = ctx.meta
        dx = _new(shape, dy)
        N.call('mmseg_slice_bwd', _c(dy), dx, dx.numel() // shape[-1], shape[-1], c0, cs)
        return dx, None, None


def slice_channels(x, c0, cs):
    return _SliceChannels.apply(x, c0, cs)


class _SamplingKL(torch.autograd.Function):
    @staticmethod
    def forward(ctx, mu, lv, eps):
        mu, lv, eps = _c(mu), _c(lv), _c(eps)
        B, Z = mu.shape
        z, kl = _new((B, Z), mu), _new((B, 1), mu)
        N.call('mmseg_sampling_kl_fwd', mu, lv, eps, z, kl, B, Z)
        ctx.save_for_backward(mu, lv, eps)
        return z, kl

    @staticmethod
    def backward(ctx, dz, dkl):
        mu, lv, eps = ctx.saved_tensors
        B, Z = mu.shape
        dmu, dlv = _new((B, Z), mu), _new((B, Z), mu)
        N.call('mmseg_sampling_kl_bwd', mu, lv, eps, _c(dz) if dz is not None else None,
               _c(dkl) if dkl is not None else None, dmu, dlv, B, Z)
        return dmu, dlv, None


def sampling_kl(z_mean, z_log_var, eps):
    """-> (z, kl[B,1])  (utils/sdnet_utils.py:9-21 with explicit eps, costs.py:186-189)."""
    return _SamplingKL.apply(z_mean, z_log_var, eps)


class _Add(torch.autograd.Function):
    @staticmethod
    def forward(ctx, a, b):
        a, b = _c(a), _c(b)
        y = _new(a.shape, a)
        N.call('mmseg_axpby', a, b, y, a.numel(), 1.0, 1.0)
        return y

    @staticmethod
    def backward(ctx, dy):
        return dy, dy


def add(a, b):
    return _Add.apply(a, b)


# ------------------------------------------------------------------------------------------------------
# instance norm + SPADE modulation + LeakyReLU
# ------------------------------------------------------------------------------------------------------
class _InstNormSpade(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, gamma, beta, act_alpha):
        x = _c(x)
        B = x.shape[0]
        per = x.numel() // B
        gamma = _c(gamma) if gamma is not None else None
        beta = _c(beta) if beta is not None else None
        y = _new(x.shape, x)
        stat = _new((B, 2), x)
        ws = _ws('instnorm', N.call('mmseg_in_workspace_floats', B), x.device)
        N.call('mmseg_instnorm_spade_fwd', x, gamma, beta, y, stat, ws, B, per, IN_EPS, float(act_alpha))
        ctx.act_alpha = act_alpha
        ctx.save_for_backward(x, stat, gamma, beta)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, stat, gamma, beta = ctx.saved_tensors
        B = x.shape[0]
        per = x.numel() // B
        dx = _new(x.shape, x)
        dg = _new(x.shape, x) if gamma is not None else None
        db = _new(x.shape, x) if gamma is not None else None
        dxn = _ws('instnorm_dxn', x.numel(), x.device)
        ws = _ws('instnorm', N.call('mmseg_in_workspace_floats', B), x.device)
        N.call('mmseg_instnorm_spade_bwd', _c(dy), x, stat, gamma, beta, dx, dg, db, dxn, ws, B, per, IN_EPS,
               float(ctx.act_alpha))
        return dx, dg, db, None


# ------------------------------------------------------------------------------------------------------
# two convolutions of the same input as ONE (the gamma and beta convolutions of a SPADE unit)
# ------------------------------------------------------------------------------------------------------
_pair_cache = {}


def _pair_operands(wa, ba, wb, bb, wkey):
    """[KH, KW, Cin, Ca + Cb] kernel and [Ca + Cb] bias of the fused convolution: the two Keras kernels side by side.  Parameters of
    an nn.Model (`wkey`): a copy per weight version into buffers that live as long as the layer, so that the cached weight images
    keyed on them stay valid.  Anonymous weights (`wkey` None) are NEVER cached -- neither an address nor an object id identifies a
    tensor once the caching allocator has recycled it (round-3 review: a later weight of the same byte size got the previous
    layer's operands): they are concatenated on every call into scratch of the stream, like _wprep does."""
    KH, KW, Cin, Ca = wa.shape
    Cb = wb.shape[3]
    assert wb.shape == (KH, KW, Cin, Cb) and ba.numel() == Ca and bb.numel() == Cb
    nw, nb = KH * KW * Cin * (Ca + Cb), Ca + Cb
    if wkey is None:
        buf = _ws('pair_operands', nw + nb + 4, wa.device)
        wcat = buf[:nw].view(KH, KW, Cin, Ca + Cb)
        bcat = buf[(nw + 3) // 4 * 4:(nw + 3) // 4 * 4 + nb]
        N.call('mmseg_concat_cols', wa, wb, wcat, KH * KW * Cin, Ca, Cb)
        N.call('mmseg_concat_cols', ba, bb, bcat, 1, Ca, Cb)
        return wcat, bcat
    key = (wkey, wa.data_ptr(), wb.data_ptr(), _sid(wa.device))
    ent = _pair_cache.get(key)
    if ent is not None and (tuple(ent[1].shape) != (KH, KW, Cin, Ca + Cb) or ent[2].numel() != nb):
        ent = None           # never hand out operands of another geometry
    if ent is not None and ent[0] == _wver(wkey):
        return ent[1], ent[2]
    if ent is None:
        wcat = torch.empty((KH, KW, Cin, Ca + Cb), dtype=torch.float32, device=wa.device)
        bcat = torch.empty((Ca + Cb,), dtype=torch.float32, device=wa.device)
    else:
        wcat, bcat = ent[1], ent[2]
    N.call('mmseg_concat_cols', wa, wb, wcat, KH * KW * Cin, Ca, Cb)
    N.call('mmseg_concat_cols', ba, bb, bcat, 1, Ca, Cb)
    _pair_cache[key] = (_wver(wkey), wcat, bcat)
    return wcat, bcat


class _Conv2dPair(torch.autograd.Function):
    """y[..., :Ca] = conv(x, wa) + ba, y[..., Ca:] = conv(x, wb) + bb (3x3 'same', stride 1) as ONE convolution with Ca + Cb output
    channels: x is read once, the 32-wide tiles of two narrow convolutions become one 64-wide tile, and in the backward pass one
    weight-gradient and one data-gradient launch replace two of each (plus the addition of the two data gradients).  Per output
    channel the arithmetic is that of the separate convolutions."""

    @staticmethod
    def forward(ctx, x, anchor, wa, ba, wb, bb, grads, wkey, out_dtype=torch.float32):
        x = _c(x)
        B, H, W, Cin = x.shape
        KH, KW, Cin2, Ca = wa.shape
        Cb = wb.shape[3]
        assert Cin == Cin2 and wb.shape[:3] == wa.shape[:3] and KH % 2 == 1 and KW % 2 == 1
        Cout = Ca + Cb
        wcat, bcat = _pair_operands(wa, ba, wb, bb, wkey)
        pkey = (('pair',) + tuple(wkey[:1]), wkey[1]) if isinstance(wkey, tuple) else None
        wt = _wprep(wcat, KH, KW, Cin, Cout, 0, pkey) if N.call('mmseg_conv2d_fast_path', Cin, 0, Cout, 0) else None
        # 16-bit outputs need the fast path in BOTH directions: the backward pass reads the 16-bit dy and writes a 16-bit dx through
        # the fast path of the Cout -> Cin convolution (advisor, round 3: 2f % 32 != 0 sent a 16-bit dy to the generic kernel)
        bwd_fast = bool(N.call('mmseg_conv2d_fast_path', Cout, 0, Cin, 0))
        y = _new((B, H, W, Cout), x, out_dtype if (wt is not None and bwd_fast) else torch.float32)
        _conv_fwd_raw(x, None, wcat, wt, bcat, y, None, B, H, W, Cin, 0, H, W, Cout, KH, KW, 1, KH // 2, KW // 2, 0, 0, 0, 0.0, 0)
        ctx.geom = (B, H, W, Cin, Ca, Cb, KH, KW)
        ctx.grads, ctx.pkey = grads, pkey
        ctx.operands = (wa, ba, wb, bb, wkey)     # plain (non-leaf) weight views: not tracked by autograd
        ctx.save_for_backward(x)
        return y

    @staticmethod
    def backward(ctx, dy):
        (x,) = ctx.saved_tensors
        B, H, W, Cin, Ca, Cb, KH, KW = ctx.geom
        Cout, M, K = Ca + Cb, B * H * W, KH * KW * Cin
        dy = _c(dy)
        wga, bga, wgb, bgb = ctx.grads
        if bga is not None:
            tmp = _ws('pair_db', Cout, dy.device)[:Cout]
            ws = _ws('colsum', N.call('mmseg_colsum_workspace_floats', M, Cout), dy.device)
            if _h(dy) and Cout % 64 == 0:
                N.call('mmseg_colsum_t', dy, tmp, ws, M, Cout, 0, _h(dy))
            else:
                N.call('mmseg_colsum', dy if _h(dy) == 0 else dy.float(), tmp, ws, M, Cout, 1.0, 0)
            N.call('mmseg_split_cols_acc', tmp, bga, bgb, 1, Ca, Cb)
        if wga is not None:
            tmp = _ws('pair_dw', K * Cout, dy.device)[:K * Cout]
            _wgrad_launch(x, None, dy, tmp, B, H, W, Cin, 0, H, W, Cout, KH, KW, 1, KH // 2, KW // 2, 0, 0)
            N.call('mmseg_split_cols_acc', tmp, wga.view(-1), wgb.view(-1), K, Ca, Cb)
        _grad_done(wga, bga, wgb, bgb)
        dx = None
        if ctx.needs_input_grad[0]:
            # (a model's operands come out of the cache; anonymous ones are concatenated again: their scratch may have been reused)
            wcat = _pair_operands(*ctx.operands)[0]
            fastb = bool(N.call('mmseg_conv2d_fast_path', Cout, 0, Cin, 0))
            if not fastb and _h(dy):
                dy = dy.float()                             # (unreachable with the forward's choice of out_dtype; kept as a guard)
            dx = _new((B, H, W, Cin), dy, x.dtype if (fastb or _h(x) == 0) else torch.float32)      # a gradient is stored like its tensor
            if fastb:
                wf, wt = None, _wprep(wcat, KH, KW, Cin, Cout, 1, ctx.pkey)
            else:
                wf, wt = _ws('wflip', wcat.numel(), dy.device)[:wcat.numel()], None
                N.call('mmseg_conv2d_wflip', wcat, wf, KH, KW, Cin, Cout)
            _conv_fwd_raw(dy, None, wf, wt, None, dx, None, B, H, W, Cout, 0, H, W, Cin, KH, KW, 1, KH - 1 - KH // 2, KW - 1 - KW // 2,
                          0, 0, 0, 0.0, 0)
        return (dx,) + (None,) * 8


def conv2d_pair(x, wa, ba, wb, bb, grads=(None, None, None, None), anchor=None, wkey=None, out_dtype=torch.float32):
    if all(g is None for g in grads):
        anchor = None
    return _Conv2dPair.apply(x, anchor, wa, ba, wb, bb, tuple(grads), wkey, out_dtype)


class _InstNormSpadeGB(torch.autograd.Function):
    """instnorm_spade with gamma and beta as the halves of one tensor gb [B, H, W, 2C] (the output of conv2d_pair)"""

    @staticmethod
    def forward(ctx, x, gb, act_alpha, out_dtype=torch.float32):
        x, gb = _c(x), _c(gb)
        B, C = x.shape[0], x.shape[-1]
        assert gb.shape == x.shape[:-1] + (2 * C,)
        per = x.numel() // B
        y = _new(x.shape, x, out_dtype)
        stat = _new((B, 2), x)
        ws = _ws('instnorm', N.call('mmseg_in_workspace_floats', B), x.device)
        N.call('mmseg_instnorm_spade_fwd_gb_t', x, gb, y, stat, ws, B, per, C, IN_EPS, float(act_alpha), _h(gb), _h(y))
        ctx.act_alpha = act_alpha
        ctx.save_for_backward(x, stat, gb)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, stat, gb = ctx.saved_tensors
        B, C = x.shape[0], x.shape[-1]
        per = x.numel() // B
        dx, dgb = _new(x.shape, x), _new(gb.shape, gb, gb.dtype)          # a gradient is stored like its tensor
        dxn = _ws('instnorm_dxn', x.numel(), x.device)
        ws = _ws('instnorm', N.call('mmseg_in_workspace_floats', B), x.device)
        dy = _c(dy)
        N.call('mmseg_instnorm_spade_bwd_gb_t', dy, x, stat, gb, dx, dgb, dxn, ws, B, per, C, IN_EPS, float(ctx.act_alpha), _h(gb), _h(dy))
        return dx, dgb, None, None


def instnorm_spade_gb(x, gb, act_alpha=-1.0, out_dtype=torch.float32):
    """act( IN(x) * (1 + gb[..., :C]) + gb[..., C:] ); `out_dtype`: storage type of the result (and of its gradient)"""
    return _InstNormSpadeGB.apply(x, gb, act_alpha, out_dtype)


class _ExpandScalar(torch.autograd.Function):
    """A 1-element parameter (the scalar gamma / beta of keras_contrib InstanceNormalization(axis=None)) as a [B, C] table
    for the FiLM kernel; the backward pass sums the table's gradient into the parameter's gradient-arena slot."""

    @staticmethod
    def forward(ctx, anchor, p, B, C, grad):
        ctx.grad = grad
        return p.reshape(1, 1).expand(B, C).contiguous()

    @staticmethod
    def backward(ctx, dg):
        if ctx.grad is not None:
            dg = _c(dg)
            ws = _ws('colsum', N.call('mmseg_colsum_workspace_floats', dg.numel(), 1), dg.device)
            N.call('mmseg_colsum', dg.reshape(-1), ctx.grad, ws, dg.numel(), 1, 1.0, 1)
        _grad_done(ctx.grad)
        return (None,) * 5


def expand_scalar(p, B, C, grad=None, anchor=None):
    return _ExpandScalar.apply(anchor if grad is not None else None, p, B, C, grad)


def instnorm_spade(x, gamma=None, beta=None, act_alpha=-1.0):
    """act( IN(x) * (1 + gamma) + beta ); act_alpha < 0: no activation (layers/spade.py:7-33,51-54)."""
    return _InstNormSpade.apply(x, gamma, beta, act_alpha)


# ------------------------------------------------------------------------------------------------------
# losses: value (device scalar) + gradient w.r.t. the prediction, no autograd node
# ------------------------------------------------------------------------------------------------------
def seg_loss(pred, target, num_masks, lambda_bce, scale, class_sum_hook=None, n_pix_global=None, want_grad=True, scale_dev=None):
    """make_combined_dice_bce (lambda_bce = 0.01) or make_dice_loss_fnc (lambda_bce = 0) of costs.py.
    `class_sum_hook(t)` may all-reduce the batch-global class sums in place (data-parallel training).
    -> (loss[1], dpred or None); dpred already multiplied by `scale` (loss weight) and, if given, by the device scalar `scale_dev`
    (the dynamic loss scale, loss_scaler.py)."""
    pred, target = _c(pred), _c(target)
    B, H, W, C = pred.shape
    dev = pred.device
    stats = _new((N.call('mmseg_segloss_stats_floats', B),), pred)
    ws = _ws('segloss', N.call('mmseg_segloss_workspace_floats', B), dev)
    N.call('mmseg_segloss_stats', pred, target, stats, ws, B, H * W, C, num_masks)
    if class_sum_hook is not None and lambda_bce != 0.0:
        class_sum_hook(stats[N.call('mmseg_segloss_class_offset', B):])
    loss = _new((1,), pred)
    coef = _new((N.call('mmseg_segloss_coef_floats', B, C),), pred)
    npl = float(B * H * W)
    npg = npl if n_pix_global is None else float(n_pix_global)
    # loss value over the global pixel count; gradient seeds over the LOCAL one (the DP all-reduce averages over ranks)
    N.call('mmseg_segloss_finalize', stats, loss, coef, B, C, npg, npl, float(lambda_bce))
    dpred = None
    if want_grad:
        dpred = _new(pred.shape, pred)
        if scale_dev is None:
            N.call('mmseg_segloss_grad', pred, target, coef, dpred, B, H * W, C, num_masks, float(scale),
                   int(lambda_bce != 0.0))
        else:
            N.call('mmseg_segloss_grad_s', pred, target, coef, dpred, B, H * W, C, num_masks, float(scale), scale_dev,
                   int(lambda_bce != 0.0))
    return loss, dpred


# ------------------------------------------------------------------------------------------------------
# boundary loss of the segmentor (csrc/boundary.hip; build-defined, conf.w_boundary): no autograd node either
# ------------------------------------------------------------------------------------------------------
def boundary_map(target, num_masks):
    """Signed distance map of the first `num_masks` channels of target [B,H,W,C] (foreground: > 0.5) -> phi [B,H,W,num_masks]:
    the distance to the nearest foreground pixel outside an organ, -(distance to the nearest background pixel - 1) inside, 0 for an
    empty or a full mask.  Exact (include/mmseg_hip.h)."""
    target = _c(target)
    B, H, W, C = target.shape
    phi = _new((B, H, W, num_masks), target)
    ws = _ws('boundary_map', (N.call('mmseg_boundary_workspace_bytes', B, H, W, num_masks) + 3) // 4, target.device, torch.int32)
    N.call('mmseg_boundary_map', target, phi, ws, B, H, W, C, num_masks)
    return phi


def boundary_term(pred, phi, num_masks):
    """L_B = mean over (b, pixel, k < num_masks) of pred * phi -> loss_b[1] (a fixed-order two-stage reduction)"""
    pred, phi = _c(pred), _c(phi)
    B, H, W, C = pred.shape
    loss_b = _new((1,), pred)
    ws = _ws('boundary_loss', N.call('mmseg_boundary_loss_workspace_floats', B), pred.device)
    N.call('mmseg_boundary_loss', pred, phi, loss_b, ws, B, H * W, C, num_masks)
    return loss_b


def boundary_grad_add(phi, dpred, num_masks, scale, weight_dev, scale_dev=None):
    """dpred[..., :num_masks] += scale [* scale_dev[0]] * weight_dev[0] * phi / phi.numel(), in place on what seg_loss wrote"""
    B, H, W, C = dpred.shape
    N.call('mmseg_boundary_grad_add', _c(phi), dpred, B, H * W, C, num_masks, float(scale), scale_dev, weight_dev)
    return dpred


def boundary_combine(loss, loss_b, weight_dev):
    """loss[0] += weight_dev[0] * loss_b[0] on the device (loss_b keeps the raw term)"""
    N.call('mmseg_boundary_combine', loss, loss_b, weight_dev)
    return loss


# ------------------------------------------------------------------------------------------------------
# Lovasz-Softmax loss of the segmentor (csrc/lovasz.hip; build-defined, conf.w_lovasz): no autograd node either
# ------------------------------------------------------------------------------------------------------
def lovasz_map(pred, target, num_masks, classes_all=False):
    """The signed Lovasz map m [B,H,W,num_masks] of pred against target (both [B,H,W,C], foreground: target > 0.5): per sample and
    class the pixels sorted by |y - p| on the device, m = +-lovasz_grad / (B * classes counted), 0 where the error is 0
    (include/mmseg_hip.h).  The loss is sum m * (p - y) and m is its gradient with respect to pred."""
    pred, target = _c(pred), _c(target)
    B, H, W, C = pred.shape
    m = _new((B, H, W, num_masks), pred)
    ws = _ws('lovasz_map', (N.call('mmseg_lovasz_workspace_bytes', B, H * W, num_masks) + 3) // 4, pred.device, torch.int32)
    N.call('mmseg_lovasz_map', pred, target, m, ws, B, H * W, C, num_masks, 1 if classes_all else 0)
    return m


def lovasz_term(pred, target, m, num_masks):
    """L = sum over (b, pixel, k < num_masks) of m * (pred - y) -> loss_l[1] (fp64, a fixed-order two-stage reduction, rounded once)"""
    pred, target, m = _c(pred), _c(target), _c(m)
    B, H, W, C = pred.shape
    loss_l = _new((1,), pred)
    ws = _ws('lovasz_loss', N.call('mmseg_lovasz_loss_workspace_floats', B), pred.device)
    N.call('mmseg_lovasz_loss', pred, target, m, loss_l, ws, B, H * W, C, num_masks)
    return loss_l


def lovasz_grad_add(m, dpred, num_masks, scale, weight_dev, scale_dev=None):
    """dpred[..., :num_masks] += scale [* scale_dev[0]] * weight_dev[0] * m, in place on what seg_loss (and the boundary term) wrote"""
    B, H, W, C = dpred.shape
    N.call('mmseg_lovasz_grad_add', _c(m), dpred, B, H * W, C, num_masks, float(scale), scale_dev, weight_dev)
    return dpred


# ------------------------------------------------------------------------------------------------------
# in-graph per-sample loss terms of the automated-pairing trainers (csrc/pairloss.hip)
# ------------------------------------------------------------------------------------------------------
class _OverlapDice(torch.autograd.Function):
    """balancer.dice of one reference anatomy against J others -> [B, J] (model_components/balancer.py:21-22,33-38)"""

    @staticmethod
    def forward(ctx, ref, *others):
        ref = _c(ref)
        others = [_c(o) for o in others]
        B, J = ref.shape[0], len(others)
        per = ref.numel() // B
        out = _new((B, J), ref)
        stats = _new((J, B, 3), ref)
        ws = _ws('pairloss', N.call('mmseg_pairloss_workspace_floats', B), ref.device)
        for j, o in enumerate(others):
            N.call('mmseg_pair_dice_fwd', ref, o, stats[j], _col(out, j),
                   J, ws, B, per)
        ctx.save_for_backward(ref, stats, *others)
        return out

    @staticmethod
    def backward(ctx, g):
        ref, stats = ctx.saved_tensors[:2]
        others = ctx.saved_tensors[2:]
        g = _c(g)
        B, J = g.shape
        per = ref.numel() // B
        dref = _new(ref.shape, ref)
        douts = []
        for j, o in enumerate(others):
            do = _new(o.shape, o) if ctx.needs_input_grad[1 + j] else None
            N.call('mmseg_pair_dice_bwd', ref, o, stats[j], _col(g, j), J, dref, do, int(j > 0), B, per)
            douts.append(do)
        return (dref if ctx.needs_input_grad[0] else None,) + tuple(douts)


def _col(t, j):
    """view of t[:, j:] flattened so that element [b, j] sits at offset b * row_stride (used with an explicit ld)"""
    flat = t.reshape(-1)
    return flat[j:]


def overlap_dice(ref, others):
    return _OverlapDice.apply(ref, *others)


class _RowMAE(torch.autograd.Function):
    """costs.mae_single_input: mean |x - y| over all but the batch axis -> [B]; gradient to y only (x is data)"""

    @staticmethod
    def forward(ctx, x, y):
        x, y = _c(x), _c(y)
        B = y.shape[0]
        per = y.numel() // B
        out = _new((B,), y)
        ws = _ws('pairloss', N.call('mmseg_pairloss_workspace_floats', B), y.device)
        N.call('mmseg_row_mae_fwd', x, y, out, ws, B, per)
        ctx.save_for_backward(x, y)
        return out

    @staticmethod
    def backward(ctx, g):
        x, y = ctx.saved_tensors
        B = y.shape[0]
        dy = _new(y.shape, y)
        N.call('mmseg_row_mae_bwd', x, y, _c(g), dy, B, y.numel() // B)
        return None, dy


def row_mae(x, y):
    return _RowMAE.apply(x, y)


class _SegLossPerSample(torch.autograd.Function):
    """costs.make_combined_dice_bce_perbatch(num_masks)(y_true, y_pred) -> [B] (costs.py:138-143), including the
    swapped-argument cross-entropy (class weights from the prediction over the whole batch, log-softmax of the labels)."""

    @staticmethod
    def forward(ctx, target, pred, num_masks, lambda_bce, class_sum_hook):
        target, pred = _c(target), _c(pred)
        B, H, W, C = pred.shape
        stats = _new((N.call('mmseg_segpb_stats_floats', B),), pred)
        ws = _ws('pairloss', N.call('mmseg_pairloss_workspace_floats', B), pred.device)
        N.call('mmseg_segpb_stats', pred, target, stats, ws, B, H * W, C, num_masks)
        if class_sum_hook is not None:
            class_sum_hook(stats[N.call('mmseg_segpb_class_offset', B):])
        loss = _new((B,), pred)
        N.call('mmseg_segpb_loss', stats, loss, B, H * W, C, float(lambda_bce))
        ctx.save_for_backward(target, stats)
        ctx.meta = (B, H * W, C, num_masks, float(lambda_bce), class_sum_hook)
        return loss

    @staticmethod
    def backward(ctx, g):
        target, stats = ctx.saved_tensors
        B, HW, C, nm, lam, hook = ctx.meta
        g = _c(g)
        A = _new((8,), g)
        N.call('mmseg_segpb_classgrad', stats, g, A, B)
        if hook is not None:
            hook(A)
        dpred = _new(target.shape, target)
        N.call('mmseg_segpb_grad', target, stats, g, A, dpred, B, HW, C, nm, lam)
        return None, dpred, None, None, None


def seg_loss_per_sample(target, pred, num_masks, lambda_bce=0.01, class_sum_hook=None):
    return _SegLossPerSample.apply(target, pred, num_masks, lambda_bce, class_sum_hook)


class _RowDot(torch.autograd.Function):
    """sum_j w[:, j] * l_j -> [B, 1]: keras Multiply + Add over the candidate pairs (models/dafnet.py:293-312)"""

    @staticmethod
    def forward(ctx, w, *ls):
        w = _c(w)
        B, J = w.shape
        l = torch.stack([x.reshape(B) for x in ls], dim=1).contiguous()      # [B, J] gather of J*B scalars
        out = _new((B, 1), w)
        N.call('mmseg_rowdot_fwd', w, l, out, B, J)
        ctx.save_for_backward(w, l)
        ctx.shapes = [tuple(x.shape) for x in ls]
        return out

    @staticmethod
    def backward(ctx, g):
        w, l = ctx.saved_tensors
        B, J = w.shape
        dw, dl = _new(w.shape, w), _new(l.shape, l)
        N.call('mmseg_rowdot_bwd', w, l, _c(g), dw, dl, B, J)
        return (dw,) + tuple(dl[:, j].reshape(shp) for j, shp in enumerate(ctx.shapes))


def row_dot(w, ls):
    return _RowDot.apply(w, *ls)


_DIFF_MODE = {'mae': 0, 'mse': 1, 'mean': 2}


def diff_loss(pred, target, mode, scale, want_grad=True, scale_dev=None):
    """keras 'mae' / 'mse' (target tensor or python float) or mean(pred) (costs.ypred).
    -> (loss[1], dpred or None), dpred = scale [* scale_dev[0]] * dloss/dpred."""
    pred = _c(pred)
    n = pred.numel()
    t, tc = (None, float(target)) if not isinstance(target, torch.Tensor) else (_c(target), 0.0)
    if t is not None:
        assert t.numel() == n
    loss = _new((1,), pred)
    ws = _ws('diffloss', N.call('mmseg_diffloss_workspace_floats'), pred.device)
    N.call('mmseg_diffloss', pred, t, tc, n, _DIFF_MODE[mode], loss, ws)
    dpred = None
    if want_grad:
        dpred = _new(pred.shape, pred)
        g = {0: 1.0 / n, 1: 1.0 / n, 2: 1.0 / n}[_DIFF_MODE[mode]] * scale
        if scale_dev is None:
            N.call('mmseg_diffloss_grad', pred, t, tc, n, _DIFF_MODE[mode], float(g), dpred)
        else:
            N.call('mmseg_diffloss_grad_s', pred, t, tc, n, _DIFF_MODE[mode], float(g), scale_dev, dpred)
    return loss, dpred


def spectral_reg(w, u0, alpha=10.0):
    """layers/spectralnorm.py:216-239 -> (loss[1], sgn[1]); gradient via spectral_reg_grad."""
    K = w.numel() // w.shape[-1]
    Nn = w.shape[-1]
    assert u0.numel() == K
    loss, sgn = _new((1,), w), _new((1,), w)
    ws = _ws('spectral', N.call('mmseg_spectral_workspace_floats', K, Nn), w.device)
    N.call('mmseg_spectral_fwd', w, u0, loss, sgn, ws, K, Nn, float(alpha))
    return loss, sgn


def spectral_reg_multi(ws_, u0s, alpha=10.0):
    """The Spectral penalties of up to 4 kernels in one batch of launches -> (loss[n], sgn[n])."""
    n = len(ws_)
    assert 1 <= n <= 4 and len(u0s) == n
    dims = [(w.numel() // w.shape[-1], w.shape[-1]) for w in ws_]
    loss, sgn = _new((n,), ws_[0]), _new((n,), ws_[0])
    need = sum(N.call('mmseg_spectral_workspace_floats', K, Nn) for K, Nn in dims)
    ws = _ws('spectral', need, ws_[0].device)
    pad = lambda lst, fill: list(lst) + [fill] * (4 - n)
    flat = [v for d in pad(dims, dims[0]) for v in d]
    N.call('mmseg_spectral_fwd4', *pad(ws_, ws_[0]), *pad(u0s, u0s[0]), loss, sgn, ws, n, *flat, float(alpha))
    return loss, sgn


def spectral_reg_grad_accumulate(ws_, sgn, grads, scale=1.0, scale_dev=None):
    """grads[i] += scale [* scale_dev[0]] * d penalty_i / d W_i  (one launch)"""
    n = len(ws_)
    pad = lambda lst, fill: list(lst) + [fill] * (4 - n)
    if scale_dev is None:
        N.call('mmseg_spectral_grad4', *pad(ws_, ws_[0]), sgn, *pad(grads, grads[0]), n, *pad([w.numel() for w in ws_], 0), float(scale))
    else:
        N.call('mmseg_spectral_grad4_s', *pad(ws_, ws_[0]), sgn, *pad(grads, grads[0]), n, *pad([w.numel() for w in ws_], 0),
               float(scale), scale_dev)


def spectral_reg_grad(w, sgn, scale=1.0):
    dw = _new(w.shape, w)
    N.call('mmseg_spectral_grad', w, sgn, float(scale), w.numel(), dw)
    return dw


def adam_step(p, g, m, v, lr_t, beta_1=0.9, beta_2=0.999, eps=1e-7, owner=None):
    """Keras 2.1.6 Adam over flat arenas (p, g, m, v: 1-D views of equal length).  `owner`: id of the nn.Model that owns the arena
    (its cached weight images become stale; None: all of them)."""
    assert p.numel() == g.numel() == m.numel() == v.numel()
    if isinstance(lr_t, torch.Tensor):       # a device scalar: the launch stays valid when replayed from a captured graph
        N.call('mmseg_adam_p', p, g, m, v, p.numel(), lr_t, float(beta_1), float(beta_2), float(eps))
    else:
        N.call('mmseg_adam', p, g, m, v, p.numel(), float(lr_t), float(beta_1), float(beta_2), float(eps))
    bump_weight_version(owner)


def unscale_check(arenas, scale_dev, state):
    """dynamic loss scale (loss_scaler.py): arenas[i] *= 1 / scale_dev[0] in place, state[0] = 1 if any element is non-finite.
    Up to 8 flat fp32 arenas in one launch."""
    n = len(arenas)
    assert 1 <= n <= 8
    pad = lambda lst, fill: list(lst) + [fill] * (8 - n)
    N.call('mmseg_unscale_check8', *pad(arenas, arenas[0]), *pad([a.numel() for a in arenas], 0), n, scale_dev, state)


def adam_guarded(p, g, m, v, lr_table, state, beta_1=0.9, beta_2=0.999, eps=1e-7, owner=None):
    """adam_step skipped on the device when state[0] (found_inf) is set; lr_t from lr_table at the device iteration count state[3] + 1"""
    assert p.numel() == g.numel() == m.numel() == v.numel()
    N.call('mmseg_adam_guarded', p, g, m, v, p.numel(), lr_table, lr_table.numel(), state, float(beta_1), float(beta_2), float(eps))
    bump_weight_version(owner)


def loss_scale_update(scale_dev, state, growth_interval):
    N.call('mmseg_loss_scale_update', scale_dev, state, int(growth_interval))


def fill_(t, value):
    N.call('mmseg_fill', t, t.numel(), float(value))
    return t


def axpby(a, b, sa=1.0, sb=1.0, out=None):
    out = _new(a.shape, a) if out is None else out
    N.call('mmseg_axpby', _c(a), _c(b), out, a.numel(), float(sa), float(sb))
    return out


def affine_gather(data, rows, mat, order=1):
    """out[b] = affine resample (order 0/1, edge-clamped) of data[rows[b]] with the 2x3 matrix mat[b] in (row, col)
    coordinates -- batch assembly + augmentation in one launch (csrc/augment.hip).  No gradient (input pipeline)."""
    B = mat.shape[0]
    out = _new((B,) + tuple(data.shape[1:]), data)
    N.call('mmseg_affine_gather', data, rows, _c(mat), out, B, data.shape[1], data.shape[2], data.shape[3], int(order))
    return out


FILL_MODES = ('nearest', 'constant', 'reflect', 'wrap')


def _gather(data, rows, mat, disp, shift, order, fill_mode, cval):
    """mmseg_augment_gather, or with a displacement field mmseg_elastic_gather"""
    if fill_mode not in FILL_MODES:
        raise ValueError('fill_mode must be one of %s, got %r' % (FILL_MODES, fill_mode))
    B, (Nd, H, W, C) = mat.shape[0], data.shape
    if disp is not None and tuple(disp.shape) != (B, H, W, 2):
        raise ValueError('elastic_gather: disp must be [B,H,W,2] = %r, got %r' % ((B, H, W, 2), tuple(disp.shape)))
    out = _new((B, H, W, C), data)
    ws = None
    if shift is not None:
        shift = _c(shift)
        ws = _ws('augment', N.call('mmseg_augment_workspace_floats', B, H, W, C), data.device)
    tail = (shift, out, ws, Nd, B, H, W, C, int(order), FILL_MODES.index(fill_mode), float(cval))
    if disp is None:
        N.call('mmseg_augment_gather', data, rows, _c(mat), *tail)
    else:
        N.call('mmseg_elastic_gather', data, rows, _c(mat), _c(disp), *tail)
    return out


def augment_gather(data, rows, mat, shift=None, order=1, fill_mode='nearest', cval=0.):
    """out[b] = resample of data[rows[b]] with the fp64 2x3 matrix mat[b] in (row, col) coordinates, scipy.ndimage boundary rule
    `fill_mode` (FILL_MODES; 'constant' fills with cval), order 0/1; with shift [B,C] then keras' random_channel_shift
    clip(x_c + shift[b,c], min(x), max(x)) over the transformed sample (csrc/augment.hip).  No gradient (input pipeline)."""
    return _gather(data, rows, mat, None, shift, order, fill_mode, cval)


ELASTIC_MAX_RADIUS = 128          # EL_MAXR of csrc/augment.hip
_elastic_weights = {}


def elastic_radius(sigma):
    """the blur radius of scipy.ndimage.gaussian_filter(truncate=4.0)"""
    return int(4.0 * float(sigma) + 0.5)


def elastic_weights(sigma):
    """w_0 .. w_R of gaussian_filter's normalised kernel, fp64, as scipy computes them"""
    R, s2 = elastic_radius(sigma), float(sigma) * float(sigma)
    x = np.arange(-R, R + 1)
    w = np.exp(-0.5 / s2 * x ** 2)
    return (w / w.sum())[R:]


def _i32(v):
    """the low 32 bits of an int as a C int"""
    return ((int(v) & 0xffffffff) ^ 0x80000000) - 0x80000000


def elastic_field(scale, sigma, seed, batch, H, W):
    """disp [B,H,W,2] fp32 = scale[b] * gaussian_filter(u, sigma, mode='reflect') per axis (0 row, 1 column), u in [-1, 1) Philox4x32-10
    noise keyed by (seed, batch) and counted by (pixel, sample); scale [B] fp64 on the device, a zero leaves its sample's field +0.0
    (csrc/augment.hip; the definition is in include/mmseg_hip.h).  No gradient (input pipeline)."""
    R = elastic_radius(sigma)
    if not (float(sigma) > 0) or R < 1 or R > ELASTIC_MAX_RADIUS:
        raise ValueError('elastic_field: int(4*sigma + 0.5) must lie in [1, %d], got sigma=%r' % (ELASTIC_MAX_RADIUS, sigma))
    B, H, W = int(scale.shape[0]), int(H), int(W)
    key = (float(sigma), scale.device)
    wts = _elastic_weights.get(key)
    if wts is None:
        wts = _elastic_weights[key] = torch.from_numpy(elastic_weights(sigma)).to(scale.device)          # once per sigma
    disp = _new((B, H, W, 2), scale)
    ws = _ws('elastic', N.call('mmseg_elastic_workspace_doubles', B, H, W), scale.device, torch.float64)
    N.call('mmseg_elastic_field', _c(scale), wts, disp, ws, _i32(seed), _i32(batch), B, H, W, R)
    return disp


def elastic_gather(data, rows, mat, disp, shift=None, order=1, fill_mode='nearest', cval=0.):
    """augment_gather with the displacement field disp [B,H,W,2] (elastic_field) added to the output pixel before the matrix:
    out[b](p) = data[rows[b]](mat[b] (p + disp[b](p))), one interpolation, the boundary rule applied once.  No gradient (input pipeline)."""
    if disp is None:
        raise ValueError('elastic_gather: disp must be a [B,H,W,2] tensor, got None')
    return _gather(data, rows, mat, disp, shift, order, fill_mode, cval)


INTENSITY_BLUR_MAX_RADIUS = 32          # IN_MAXR of csrc/intensity.hip
INTENSITY_FLAGS = dict(bias=1, contrast=2, gamma=4, noise=8)          # column 0 of intensity_apply's table
INTENSITY_PARAMS = 5                                                  # its columns: flags, c, g, invert, std


def intensity_weight_rows(sigmas):
    """(radius [B] int32, weights [B, INTENSITY_BLUR_MAX_RADIUS + 1] fp64) of per-sample blur sigmas, on the host; sigma 0, or one so
    small that gaussian_filter's kernel is the single weight 1, gives radius 0: the sample is copied"""
    radius = np.zeros(len(sigmas), np.int32)
    rows = np.zeros((len(sigmas), INTENSITY_BLUR_MAX_RADIUS + 1), np.float64)
    for b, s in enumerate(sigmas):
        R = elastic_radius(s) if s else 0
        if R > INTENSITY_BLUR_MAX_RADIUS:
            raise ValueError('intensity blur: int(4*sigma + 0.5) must not exceed %d, got sigma=%r' % (INTENSITY_BLUR_MAX_RADIUS, s))
        if R:
            radius[b] = R
            rows[b, :R + 1] = elastic_weights(s)
    return radius, rows


def _intensity_ws(x):
    B, H, W, C = x.shape
    if x.dtype != torch.float32 or not x.is_contiguous():
        raise ValueError('intensity: x must be a contiguous fp32 [B,H,W,C] tensor, got %s %s' % (x.dtype, tuple(x.shape)))
    n = N.call('mmseg_intensity_workspace_doubles', B, H, W, C)
    if B and not n:
        raise ValueError('intensity: shape %r is outside the kernels\' limits (H*W*C < 2^31 - 65536, B <= 65535)' % (tuple(x.shape),))
    return _ws('intensity', n, x.device, torch.float64)


def intensity_stats(x):
    """[B,3] fp64 (min, max, sum) of every sample of x [B,H,W,C], on the device (csrc/intensity.hip; fixed summation order)"""
    B, H, W, C = x.shape
    stats = _new((B, 3), x, torch.float64)
    N.call('mmseg_intensity_stats', x, stats, _intensity_ws(x), B, H, W, C)
    return stats


def intensity_blur(x, radius, weights):
    """scipy.ndimage.gaussian_filter(x[b], sigma_b, mode='reflect', truncate=4.0) over H and W with a radius and a weight row per sample
    (intensity_weight_rows, uploaded by the caller); radius[b] == 0 copies the sample bit for bit.  A new tensor.  No gradient."""
    B, H, W, C = x.shape
    if tuple(radius.shape) != (B,) or tuple(weights.shape) != (B, INTENSITY_BLUR_MAX_RADIUS + 1):
        raise ValueError('intensity_blur: radius must be [B] and weights [B, %d], got %r and %r'
                         % (INTENSITY_BLUR_MAX_RADIUS + 1, tuple(radius.shape), tuple(weights.shape)))
    out = _new(x.shape, x)
    N.call('mmseg_intensity_blur', x, radius, weights, out, _intensity_ws(x), B, H, W, C)
    return out


def intensity_apply(x, params, stats, field, seed, batch, array):
    """bias field, contrast, clip, gamma and noise IN PLACE on x [B,H,W,C] (the definition is in include/mmseg_hip.h): params [B,5] fp64
    (INTENSITY_FLAGS, c, g, invert, std), stats from intensity_stats, field [B,H,W,2] (elastic_field) or None.  Returns x.  No gradient."""
    B, H, W, C = x.shape
    if tuple(params.shape) != (B, INTENSITY_PARAMS) or tuple(stats.shape) != (B, 3):
        raise ValueError('intensity_apply: params must be [B,%d] and stats [B,3], got %r and %r'
                         % (INTENSITY_PARAMS, tuple(params.shape), tuple(stats.shape)))
    if field is not None and tuple(field.shape) != (B, H, W, 2):
        raise ValueError('intensity_apply: field must be [B,H,W,2] = %r, got %r' % ((B, H, W, 2), tuple(field.shape)))
    if x.dtype != torch.float32 or not x.is_contiguous():
        raise ValueError('intensity_apply: x must be a contiguous fp32 tensor, got %s' % (x.dtype,))
    N.call('mmseg_intensity_apply', x, params, stats, None if field is None else _c(field), _i32(seed), _i32(batch), _i32(array),
           B, H, W, C)
    return x


KSPACE_FLAGS = dict(motion=1, ghost=2, gibbs=4, spike=8, rician=16)          # column 0 of the k-space table
KSPACE_PARAMS = 48                                                          # KS_P of csrc/kspace.hip; the columns: include/mmseg_hip.h
KSPACE_MAX_EXTENT = 1024                                                    # KS_MAXN
KSPACE_MAX_SEGMENTS, KSPACE_MAX_SPIKES = 8, 4
_kspace_twiddles = {}


def kspace_extent_ok(n):
    """the transform of csrc/kspace.hip takes a length 2 <= n <= 1024 with no prime factor but 2, 3 and 5"""
    n = int(n)
    if not 2 <= n <= KSPACE_MAX_EXTENT:
        return False
    for f in (2, 3, 5):
        while n % f == 0:
            n //= f
    return n == 1


def kspace_roots(n):
    """[n, 2] fp64 on the host: (cos, sin)(2 pi k / n), k < n -- the roots the device multiplies by"""
    t = 2.0 * np.pi * np.arange(int(n), dtype=np.float64) / float(n)
    return np.stack([np.cos(t), np.sin(t)], axis=1)


def kspace_twiddles(H, W, device):
    """the [H + W, 2] fp64 root table of an (H, W) transform on `device`: made by the host once per (H, W, device) and kept"""
    device = torch.device(device)
    key = (int(H), int(W), device)
    tw = _kspace_twiddles.get(key)
    if tw is None:
        if not (kspace_extent_ok(H) and kspace_extent_ok(W)):
            raise ValueError('kspace: the extents (%d, %d) must lie in [2, %d] and have no prime factor but 2, 3 and 5' % (H, W, KSPACE_MAX_EXTENT))
        tw = _kspace_twiddles[key] = torch.from_numpy(np.concatenate([kspace_roots(H), kspace_roots(W)])).to(device)
    return tw


def _kspace_check(name, x, table, stats):
    if x.dim() != 4 or x.dtype != torch.float32 or not x.is_contiguous():
        raise ValueError('%s: x must be a contiguous fp32 [B,H,W,C] tensor, got %s %s' % (name, x.dtype, tuple(x.shape)))
    B, H, W, C = x.shape
    if tuple(table.shape) != (B, KSPACE_PARAMS) or tuple(stats.shape) != (B, 3):
        raise ValueError('%s: table must be [B,%d] and stats [B,3], got %r and %r' % (name, KSPACE_PARAMS, tuple(table.shape), tuple(stats.shape)))
    if B and not N.call('mmseg_kspace_workspace_doubles', B, H, W, C):
        raise ValueError('%s: shape %r is outside the transform\'s limits (H, W in [2, %d] with no prime factor but 2, 3, 5; B*C <= 65535)'
                         % (name, tuple(x.shape), KSPACE_MAX_EXTENT))
    return B, H, W, C


def kspace_forward(x, table, stats, spec=None):
    """spec [B,C,H,W,2] fp64 (re, im) = numpy.fft.fft2(x[b, :, :, ch] - lo_b) of the samples whose table[b, 0] (KSPACE_FLAGS) is not 0;
    the slots of the others are left as they are (csrc/kspace.hip; the definition is in include/mmseg_hip.h).  x [B,H,W,C] fp32, table
    [B,48] fp64, stats from intensity_stats(x), all on the device.  spec: a tensor to fill, else a new one.  No gradient."""
    B, H, W, C = _kspace_check('kspace_forward', x, table, stats)
    if spec is None:
        spec = _new((B, C, H, W, 2), x, torch.float64)
    elif tuple(spec.shape) != (B, C, H, W, 2):
        raise ValueError('kspace_forward: spec must be [B,C,H,W,2] = %r, got %r' % ((B, C, H, W, 2), tuple(spec.shape)))
    N.call('mmseg_kspace_forward', x, table, stats, kspace_twiddles(H, W, x.device), spec, B, H, W, C)
    return spec


def kspace_apply(spec, table, stats):
    """motion, ghosting, Gibbs truncation and spikes IN PLACE on spec [B,C,H,W,2] fp64 (the rule: include/mmseg_hip.h).  Returns spec."""
    if spec.dim() != 5 or spec.shape[4] != 2 or spec.dtype != torch.float64 or not spec.is_contiguous():
        raise ValueError('kspace_apply: spec must be a contiguous fp64 [B,C,H,W,2] tensor, got %s %s' % (spec.dtype, tuple(spec.shape)))
    B, C, H, W = spec.shape[:4]
    if tuple(table.shape) != (B, KSPACE_PARAMS) or tuple(stats.shape) != (B, 3):
        raise ValueError('kspace_apply: table must be [B,%d] and stats [B,3], got %r and %r'
                         % (KSPACE_PARAMS, tuple(table.shape), tuple(stats.shape)))
    N.call('mmseg_kspace_apply', spec, table, stats, B, H, W, C)
    return spec


def kspace_inverse(spec, table, stats, x, seed, batch, array):
    """x[b] = fp32(lo_b + |numpy.fft.ifft2(spec[b]) + the Rician draw|) IN PLACE on x [B,H,W,C] for the flagged samples; the others are
    neither read nor written.  spec [B,C,H,W,2] fp64 is overwritten (it is left half transformed).  Returns x.  No gradient."""
    B, H, W, C = _kspace_check('kspace_inverse', x, table, stats)
    if tuple(spec.shape) != (B, C, H, W, 2) or spec.dtype != torch.float64 or not spec.is_contiguous():
        raise ValueError('kspace_inverse: spec must be a contiguous fp64 [B,C,H,W,2] = %r tensor, got %s %r'
                         % ((B, C, H, W, 2), spec.dtype, tuple(spec.shape)))
    N.call('mmseg_kspace_inverse', spec, table, stats, kspace_twiddles(H, W, x.device), x, _i32(seed), _i32(batch), _i32(array), B, H, W, C)
    return x


def kspace_spectrum_buffer(x):
    """the [B,C,H,W,2] fp64 spectrum of x [B,H,W,C] as a view of the grow-only 'kspace' workspace: AugmentFlow's, one array at a time"""
    B, H, W, C = x.shape
    n = 2 * B * C * H * W
    return _ws('kspace', n, x.device, torch.float64)[:n].view(B, C, H, W, 2)


BIAS_DEFAULTS = dict(sigma_mm=40.0, levels=3, iterations=20, extent='3d')          # untuned starting values (README)
BIAS_EXTENTS = ('2d', '3d')
BIAS_BINS, BIAS_PAD = 200, 512                                                     # BF_BINS, BF_PAD of csrc/biasfield.hip
BIAS_MAX_RADIUS = 128                                                              # BF_MAXR
BIAS_TRUNCATE = 4.0
BIAS_MAX_LEVELS, BIAS_MAX_ITERATIONS = 8, 1000
BIAS_AXES = ('slice', 'row', 'column')
_bias_tables = {}


def bias_params(params=None, what='bias_correct'):
    """BIAS_DEFAULTS overlaid with `params`, validated: sigma_mm finite > 0, levels in 1..8, iterations in 1..1000, extent 2d | 3d"""
    p = dict(BIAS_DEFAULTS)
    unknown = sorted(set(params or {}) - set(p))
    if unknown:
        raise ValueError('%s: unknown key(s) %s (known: %s)' % (what, ', '.join(unknown), ', '.join(sorted(p))))
    p.update(params or {})
    s = p['sigma_mm']
    if isinstance(s, bool) or not isinstance(s, (int, float, np.integer, np.floating)) or not np.isfinite(s) or s <= 0:
        raise ValueError('%s: sigma_mm must be a finite number of mm > 0, got %r' % (what, s))
    for key, top in (('levels', BIAS_MAX_LEVELS), ('iterations', BIAS_MAX_ITERATIONS)):
        v = p[key]
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or not 1 <= v <= top:
            raise ValueError('%s: %s must be a whole number in 1..%d, got %r' % (what, key, top, v))
    if p['extent'] not in BIAS_EXTENTS:
        raise ValueError('%s: extent must be one of %s, got %r' % (what, ', '.join(BIAS_EXTENTS), p['extent']))
    return dict(sigma_mm=float(s), levels=int(p['levels']), iterations=int(p['iterations']), extent=p['extent'])


def bias_sigmas(spacings, params):
    """per level the (sigma, radius) in voxels of the slice, row and column axis: sigma_mm / 2^l / d_axis and int(4 sigma + 0.5); the slice
    axis of extent 2d gets (0.0, 0).  A radius outside 1..128 is refused with the sigma_mm that would fit."""
    d = [float('nan') if v is None else float(v) for v in spacings]
    if len(d) != 3 or any(not np.isfinite(v) or v <= 0 for v in d[(1 if params['extent'] == '2d' else 0):]):
        raise ValueError('bias_correct: spacings must be three finite numbers of mm > 0 (slices, rows, columns), got %r' % (spacings,))
    out = []
    for l in range(params['levels']):
        level = []
        for a in range(3):
            if a == 0 and params['extent'] == '2d':
                level.append((0.0, 0))
                continue
            sigma = params['sigma_mm'] / 2.0 ** l / d[a]
            R = int(BIAS_TRUNCATE * sigma + 0.5)
            if R > BIAS_MAX_RADIUS:
                raise ValueError('bias_correct: sigma_mm %g at a %s spacing of %g mm needs a radius of %d voxels at level %d, more than the '
                                 '%d the kernels take: sigma_mm <= %g fits' % (params['sigma_mm'], BIAS_AXES[a], d[a], R, l, BIAS_MAX_RADIUS,
                                                                               2.0 ** l * 32.0 * d[a]))
            if R < 1:
                raise ValueError('bias_correct: sigma_mm %g at a %s spacing of %g mm leaves a radius of 0 voxels at level %d of %d: '
                                 'sigma_mm >= %g fits (or fewer levels)' % (params['sigma_mm'], BIAS_AXES[a], d[a], l, params['levels'],
                                                                           2.0 ** l * 0.125 * d[a]))
            level.append((sigma, R))
        out.append(level)
    return out


def bias_weight_rows(level):
    """[3, 129] fp64 on the host: per axis w_0 .. w_R of scipy.ndimage's normalised Gaussian kernel, zeros beyond R (and for R = 0)"""
    rows = np.zeros((3, BIAS_MAX_RADIUS + 1), np.float64)
    for a, (sigma, R) in enumerate(level):
        if R:
            k = np.arange(-R, R + 1)
            w = np.exp(-0.5 / (sigma * sigma) * k ** 2)
            rows[a, :R + 1] = (w / w.sum())[R:]
    return rows


def bias_roots(device):
    """the [512, 2] fp64 root table of the sharpen's transforms on `device`, made by the host once per device and kept"""
    device = torch.device(device)
    key = ('roots', device)
    if key not in _bias_tables:
        _bias_tables[key] = torch.from_numpy(kspace_roots(BIAS_PAD)).to(device)
    return _bias_tables[key]


def bias_weights(level, device):
    """bias_weight_rows(level) on `device`, kept per (level, device)"""
    device = torch.device(device)
    key = (tuple(level), device)
    if key not in _bias_tables:
        _bias_tables[key] = torch.from_numpy(bias_weight_rows(level)).to(device)
    return _bias_tables[key]


def _bias_ws(S, H, W, device):
    n = N.call('mmseg_bias_workspace_doubles', S, H, W)
    if not n:
        raise ValueError('bias_correct: a volume of %d x %d x %d is outside the kernels\' limits (extents in 1..65535, fewer than 2^31 - 1 '
                         'voxels)' % (S, H, W))
    return _ws('bias', n, device, torch.float64)


def bias_correct(x, spacings, params=None, out=None, field=False):
    """Bias-field correction of x [S,H,W] fp32 on the device (csrc/biasfield.hip; the rule is in include/mmseg_hip.h): spacings = mm
    between slices, rows, columns (the first is not read with extent 2d); params: keys of BIAS_DEFAULTS.  The result is written into
    `out` (a new tensor by default; out=x corrects in place) and returned; a volume the rule leaves alone keeps its bits.  field=True
    returns (out, f [S,H,W] fp64, (frozen, updates)) with the estimated log-field.  No host synchronisation, no gradient."""
    p = bias_params(params)
    if x.dim() != 3 or x.dtype != torch.float32 or not x.is_contiguous():
        raise ValueError('bias_correct: x must be a contiguous fp32 [S,H,W] tensor, got %s %s' % (x.dtype, tuple(x.shape)))
    S, H, W = x.shape
    levels = bias_sigmas(spacings, p)
    if out is None:
        out = x.clone()
    elif out is not x:
        if out.shape != x.shape or out.dtype != x.dtype or not out.is_contiguous():
            raise ValueError('bias_correct: out must be like x, got %s %s' % (out.dtype, tuple(out.shape)))
        out.copy_(x)
    if S * H * W == 0:
        return (out, _new(x.shape, x, torch.float64), (1, 0)) if field else out
    ws = _bias_ws(S, H, W, x.device)
    roots = bias_roots(x.device)
    N.call('mmseg_bias_begin', out, ws, S, H, W)
    for level in levels:
        N.call('mmseg_bias_level', ws, roots, bias_weights(level, x.device), S, H, W, level[0][1], level[1][1], level[2][1], p['iterations'])
    N.call('mmseg_bias_finish', out, ws, S, H, W)
    if not field:
        return out
    f, info = _new(x.shape, x, torch.float64), _new((2,), x, torch.int32)
    N.call('mmseg_bias_field', ws, f, info, S, H, W)
    return out, f, info


def bias_otsu(x):
    """[4] fp64 on the device: lo, hi, the Otsu threshold of x [S,H,W] fp32 after max(., 0), and 1 when x is constant"""
    S, H, W = x.shape
    out = _new((4,), x, torch.float64)
    N.call('mmseg_bias_otsu', _c(x), _bias_ws(S, H, W, x.device), out, S, H, W)
    return out


def bias_histogram(v, mask):
    """(hist [200] int32, range [2] fp64 = vmin, vmax) of the fp64 values v under the uint8 mask: nearest bin of (v - vmin) / slope"""
    n = v.numel()
    hist, rng = _new((BIAS_BINS,), v, torch.int32), _new((2,), v, torch.float64)
    N.call('mmseg_bias_histogram', _c(v), _c(mask), _ws('bias', 512, v.device, torch.float64), hist, rng, n)
    return hist, rng


def bias_sharpen(hist, rng):
    """E [200] fp64: the sharpened histogram's expectation per bin (the rule's `E`), from the counts and (vmin, vmax)"""
    E = _new((BIAS_BINS,), hist, torch.float64)
    N.call('mmseg_bias_sharpen', hist, rng, bias_roots(hist.device), _ws('bias', 512, hist.device, torch.float64), E)
    return E


def bias_smooth(y, level):
    """G * y for y [S,H,W] fp64 and one level of bias_sigmas: a new tensor"""
    S, H, W = y.shape
    out, tmp = _new(y.shape, y, torch.float64), _new((2,) + tuple(y.shape), y, torch.float64)
    for a in range(3):
        if not (0 if a == 0 else 1) <= level[a][1] <= BIAS_MAX_RADIUS:
            raise ValueError('bias_smooth: the %s radius must lie in %d..%d, got %d' % (BIAS_AXES[a], 0 if a == 0 else 1, BIAS_MAX_RADIUS, level[a][1]))
    N.call('mmseg_bias_smooth', _c(y), out, tmp, bias_weights(level, y.device), S, H, W, level[0][1], level[1][1], level[2][1])
    return out


def bias_update(f, num, den):
    """f += num / den where den > 0, in place on f (fp64); returns f"""
    N.call('mmseg_bias_update', f, _c(num), _c(den), f.numel())
    return f


NLM_DEFAULTS = dict(search_radius=5, patch_radius=1, search_radius_z=None, h=1.0, noise='rician', sigma='auto',
                    extent='2d')                                                   # untuned starting values (README)
NLM_EXTENTS = ('2d', '3d')
NLM_NOISES = ('rician', 'gaussian')
NLM_MAX_SEARCH, NLM_MAX_PATCH, NLM_MAX_SEARCH_Z = 10, 3, 4                         # NLM_MAX_RS, _RP, _RZ of csrc/denoise.hip
NLM_TILE = (8, 32)                                                                 # NLM_TH, NLM_TW: rows x columns one block owns


def _is_number(v):
    return not isinstance(v, bool) and isinstance(v, (int, float, np.integer, np.floating))


def nlm_params(params=None, what='nlm_denoise'):
    """NLM_DEFAULTS overlaid with `params`, validated: search_radius in 1..10, patch_radius in 1..3, extent 2d | 3d, search_radius_z in
    0..4 (None: 0 for 2d, 1 for 3d; 2d takes no other), h finite > 0, noise rician | gaussian, sigma 'auto' or a finite number > 0"""
    p = dict(NLM_DEFAULTS)
    unknown = sorted(set(params or {}) - set(p))
    if unknown:
        raise ValueError('%s: unknown key(s) %s (known: %s)' % (what, ', '.join(unknown), ', '.join(sorted(p))))
    p.update(params or {})
    for key, low, top in (('search_radius', 1, NLM_MAX_SEARCH), ('patch_radius', 1, NLM_MAX_PATCH)):
        v = p[key]
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or not low <= v <= top:
            raise ValueError('%s: %s must be a whole number in %d..%d, got %r' % (what, key, low, top, v))
    if p['extent'] not in NLM_EXTENTS:
        raise ValueError('%s: extent must be one of %s, got %r' % (what, ', '.join(NLM_EXTENTS), p['extent']))
    rz = p['search_radius_z']
    if rz is None:
        rz = 0 if p['extent'] == '2d' else 1
    if isinstance(rz, bool) or not isinstance(rz, (int, np.integer)) or not 0 <= rz <= NLM_MAX_SEARCH_Z:
        raise ValueError('%s: search_radius_z must be a whole number in 0..%d, got %r' % (what, NLM_MAX_SEARCH_Z, rz))
    if p['extent'] == '2d' and rz != 0:
        raise ValueError('%s: search_radius_z %d goes with extent 3d; extent 2d searches within the slice' % (what, rz))
    if not _is_number(p['h']) or not np.isfinite(p['h']) or p['h'] <= 0:
        raise ValueError('%s: h must be a finite number > 0 (the smoothing strength in units of sigma), got %r' % (what, p['h']))
    if p['noise'] not in NLM_NOISES:
        raise ValueError('%s: noise must be one of %s, got %r' % (what, ', '.join(NLM_NOISES), p['noise']))
    s = p['sigma']
    if s != 'auto' and (not _is_number(s) or not np.isfinite(s) or s <= 0):
        raise ValueError('%s: sigma must be "auto" or a finite number > 0 in the volume\'s grey values, got %r' % (what, s))
    return dict(search_radius=int(p['search_radius']), patch_radius=int(p['patch_radius']), search_radius_z=int(rz), h=float(p['h']),
                noise=p['noise'], sigma='auto' if s == 'auto' else float(s), extent=p['extent'])


def _nlm_volume(x, what):
    if x.dim() != 3 or x.dtype != torch.float32 or not x.is_contiguous():
        raise ValueError('%s: x must be a contiguous fp32 [S,H,W] tensor, got %s %s' % (what, x.dtype, tuple(x.shape)))
    S, H, W = x.shape
    if S and H and W and not N.call('mmseg_nlm_workspace_bytes', S, H, W):
        raise ValueError('%s: a volume of %d x %d x %d is outside the kernels\' limits (fewer than 2^31 - 1 voxels)' % (what, S, H, W))
    return S, H, W


def nlm_sigma(x):
    """Immerkaer's estimate of the noise of x [S,H,W] fp32, in-plane (csrc/denoise.hip; the rule is in include/mmseg_hip.h): one fp64
    scalar [1] on the device, 0 for slices narrower than 3 pixels.  It reads anatomy edges as noise, so it runs high on small or busy
    slices.  No host synchronisation."""
    S, H, W = _nlm_volume(x, 'nlm_sigma')
    sigma = _new((1,), x, torch.float64)
    if S * H * W == 0:
        return sigma.zero_()
    ws = _ws('nlm', N.call('mmseg_nlm_workspace_bytes', S, H, W) // 8, x.device, torch.float64)
    N.call('mmseg_nlm_sigma', x, ws, sigma, S, H, W)
    return sigma


def nlm_denoise(x, params=None, out=None, sigma_out=False):
    """Non-local means denoising of x [S,H,W] fp32 on the device (csrc/denoise.hip; the rule is in include/mmseg_hip.h); params: keys of
    NLM_DEFAULTS.  The result is written into `out` (a new tensor by default; it may not be x) and returned; sigma_out=True returns
    (out, sigma) with the fp64 device scalar [1] the kernel read.  A volume whose sigma is not > 0 (a constant one under 'auto') keeps
    its bits.  No host synchronisation, no gradient."""
    p = nlm_params(params)
    S, H, W = _nlm_volume(x, 'nlm_denoise')
    if out is None:
        out = torch.empty_like(x)
    elif out is x or out.shape != x.shape or out.dtype != x.dtype or not out.is_contiguous() or out.device != x.device:
        raise ValueError('nlm_denoise: out must be another tensor like x, got %s %s' % (out.dtype, tuple(out.shape)))
    auto = p['sigma'] == 'auto'
    if S * H * W == 0:
        return (out, _new((1,), x, torch.float64).zero_()) if sigma_out else out
    sigma = nlm_sigma(x) if auto else None
    N.call('mmseg_nlm_denoise', x, out, sigma, 0.0 if auto else p['sigma'], S, H, W, p['search_radius'], p['patch_radius'],
           p['search_radius_z'], p['h'], int(p['noise'] == 'rician'))
    if not sigma_out:
        return out
    return out, (sigma if auto else torch.full((1,), p['sigma'], dtype=torch.float64, device=x.device))


def preprocess_volume(img, lab, values, images, masks, resampled, rows, cols, mod, knots=None):
    """The S raw slices of one (volume, modality) -> channel `mod` of images [S,OH,OW,M] and channels mod*K .. of masks [S,OH,OW,M*K]
    (csrc/preprocess.hip): resample to `resampled` = (RH, RW), split the grey label values `values` [K] into binary channels,
    rescale every slice to [-1, 1] by the extremes of its whole resampled frame, crop / pad with the per-axis index maps
    rows / cols = (lo, kept, before).  img [S,H,W] fp32, lab [S,H,W] uint8, values int32, all on the device of `images`.  With
    knots = (x [G,K], y [K]) (preprocess_quantiles; build-defined) the rescale is the clamped piecewise-linear map through the
    knots instead, one launch in place of two; G = S: a row per slice, G = 1: one row for the volume.  No gradient (input pipeline)."""
    S, H, W = img.shape
    RH, RW = int(resampled[0]), int(resampled[1])
    K = int(values.numel())
    OH, OW, M = images.shape[1:]
    if (img.dtype != torch.float32 or lab.dtype != torch.uint8 or tuple(lab.shape) != (S, H, W) or images.shape[0] != S
            or tuple(masks.shape) != (S, OH, OW, M * K) or not 0 <= mod < M or not images.is_contiguous() or not masks.is_contiguous()):
        raise ValueError('preprocess_volume: img %s %s, lab %s %s, images %s, masks %s, K = %d, modality %d'
                         % (tuple(img.shape), img.dtype, tuple(lab.shape), lab.dtype, tuple(images.shape), tuple(masks.shape), K, mod))
    geo = [int(v) for v in tuple(rows) + tuple(cols)]
    if knots is None:
        ws = _ws('preprocess', N.call('mmseg_preprocess_workspace_floats', S, RH, RW), images.device)
        N.call('mmseg_preprocess_minmax', _c(img), ws, S, H, W, RH, RW)
        N.call('mmseg_preprocess_image', _c(img), ws, images, S, H, W, RH, RW, OH, OW, *(geo + [M, mod]))
    else:
        _image_map(img, images, knots, S, H, W, RH, RW, OH, OW, geo, M, mod)
    N.call('mmseg_preprocess_label', _c(lab), values, masks, S, H, W, RH, RW, OH, OW, *(geo + [M * K, mod * K, K]))


def preprocess_images(img, images, resampled, rows, cols, mod, knots=None):
    """The image half of preprocess_volume, for a volume without labels: channel `mod` of images [S,OH,OW,M] is written and no label
    kernel is launched."""
    S, H, W = img.shape
    RH, RW = int(resampled[0]), int(resampled[1])
    OH, OW, M = images.shape[1:]
    if img.dtype != torch.float32 or images.shape[0] != S or not 0 <= mod < M or not images.is_contiguous():
        raise ValueError('preprocess_images: img %s %s, images %s, modality %d' % (tuple(img.shape), img.dtype, tuple(images.shape), mod))
    geo = [int(v) for v in tuple(rows) + tuple(cols)]
    if knots is not None:
        return _image_map(img, images, knots, S, H, W, RH, RW, OH, OW, geo, M, mod)
    ws = _ws('preprocess', N.call('mmseg_preprocess_workspace_floats', S, RH, RW), images.device)
    N.call('mmseg_preprocess_minmax', _c(img), ws, S, H, W, RH, RW)
    N.call('mmseg_preprocess_image', _c(img), ws, images, S, H, W, RH, RW, OH, OW, *(geo + [M, mod]))


PREPROCESS_MAX_KNOTS = 16          # csrc/preprocess.hip


def _image_map(img, images, knots, S, H, W, RH, RW, OH, OW, geo, M, mod):
    """mmseg_preprocess_image_map with knots = (x [G,K], y [K]) fp32 on the device; G = 1 (one scale for the volume) or S"""
    x, y = knots
    K = int(y.numel())
    if (x.dim() != 2 or x.dtype != torch.float32 or y.dtype != torch.float32 or x.shape[1] != K or x.shape[0] not in (1, S)
            or not 2 <= K <= PREPROCESS_MAX_KNOTS):
        raise ValueError('preprocess: knots must be (x [1 or %d, K], y [K]) fp32 with K in 2..%d, got %s %s and %s %s'
                         % (S, PREPROCESS_MAX_KNOTS, tuple(x.shape), x.dtype, tuple(y.shape), y.dtype))
    per_volume = 1 if x.shape[0] == 1 and S > 1 else 0          # one slice: both scopes read row 0
    if per_volume and S * RH * RW >= 2 ** 31:
        raise ValueError('preprocess: a volume of %d x %d x %d resampled values (2^31 or more) cannot share one scale' % (S, RH, RW))
    N.call('mmseg_preprocess_image_map', _c(img), _c(x), _c(y), images, S, H, W, RH, RW, OH, OW, *(geo + [M, mod, K, per_volume]))


def preprocess_quantiles(img, resampled, ranks, per_volume):
    """x [G,K] fp32 on the device: the order statistics of rank ranks[k] (0-based, a host sequence of K = 2..16 integers) of every
    segment of the raw slices img [S,H,W] fp32 resampled to `resampled` = (RH, RW) -- one segment per slice (G = S, N = RH * RW values)
    or, with per_volume, the whole volume (G = 1, N = S * RH * RW).  Exact: every x is an element of the resampled population that
    preprocess_images(knots=...) meets again bit for bit (csrc/preprocess.hip; the definition is in include/mmseg_hip.h).  No gradient."""
    S, H, W = img.shape
    RH, RW = int(resampled[0]), int(resampled[1])
    ranks = [int(r) for r in ranks]
    K, per_volume = len(ranks), bool(per_volume)
    n = (S if per_volume else 1) * RH * RW
    if img.dtype != torch.float32 or S < 1 or RH < 1 or RW < 1 or not 2 <= K <= PREPROCESS_MAX_KNOTS:
        raise ValueError('preprocess_quantiles: img %s %s, resampled %s, %d ranks (2..%d)'
                         % (tuple(img.shape), img.dtype, (RH, RW), K, PREPROCESS_MAX_KNOTS))
    if n >= 2 ** 31:
        raise ValueError('preprocess_quantiles: a segment of %d values (2^31 or more)' % n)
    if any(not 0 <= r <= n - 1 for r in ranks):
        raise ValueError('preprocess_quantiles: ranks must lie in [0, %d], got %r' % (n - 1, ranks))
    G = 1 if per_volume else S
    x = _new((G, K), img)
    nbytes = N.call('mmseg_preprocess_quantiles_workspace_bytes', S, K, int(per_volume))
    ws = _ws('preprocess_quantiles', (nbytes + 3) // 4, img.device, torch.int32)
    N.call('mmseg_preprocess_quantiles', _c(img), torch.tensor(ranks, dtype=torch.int32).to(img.device), ws, x, S, H, W, RH, RW, K,
           int(per_volume))
    return x


ALIGN_DEFAULTS = dict(max_shift_mm=40.0, max_slices=4, bins=32, levels=3, min_overlap=0.5,
                      percentiles=(0.5, 99.5))                                     # untuned starting values (README)
ALIGN_MAX_BINS, ALIGN_MAX_LEVELS, ALIGN_MAX_SLICES, ALIGN_MAX_SHIFT = 64, 8, 64, 1 << 20          # csrc/align.hip
ALIGN_STATE = 8                    # fp64 words of the state block (include/mmseg_hip.h)
ALIGN_AGGREGATE = True             # the histogram kernel's wave aggregation (DESIGN.md section 8 has the measurement)
ALIGN_WORKSPACE_CAP = 512 << 20


def align_params(params=None, what='align_volumes'):
    """ALIGN_DEFAULTS overlaid with `params`, validated: max_shift_mm finite >= 0, max_slices a whole number in 0..64, bins in 2..64,
    levels in 1..8, min_overlap in (0, 1], percentiles two numbers 0 <= lo < hi <= 100"""
    p = dict(ALIGN_DEFAULTS)
    unknown = sorted(set(params or {}) - set(p))
    if unknown:
        raise ValueError('%s: unknown key(s) %s (known: %s)' % (what, ', '.join(unknown), ', '.join(sorted(p))))
    p.update(params or {})
    if not _is_number(p['max_shift_mm']) or not np.isfinite(p['max_shift_mm']) or p['max_shift_mm'] < 0:
        raise ValueError('%s: max_shift_mm must be a finite number >= 0, got %r' % (what, p['max_shift_mm']))
    for key, low, top in (('max_slices', 0, ALIGN_MAX_SLICES), ('bins', 2, ALIGN_MAX_BINS), ('levels', 1, ALIGN_MAX_LEVELS)):
        v = p[key]
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or not low <= v <= top:
            raise ValueError('%s: %s must be a whole number in %d..%d, got %r' % (what, key, low, top, v))
    if not _is_number(p['min_overlap']) or not 0 < p['min_overlap'] <= 1:
        raise ValueError('%s: min_overlap must be a number in (0, 1] (the share of the zero shift\'s overlap a candidate must keep), '
                         'got %r' % (what, p['min_overlap']))
    q = p['percentiles']
    if (not isinstance(q, (list, tuple)) or len(q) != 2 or any(not _is_number(v) or not np.isfinite(v) for v in q)
            or not 0 <= q[0] < q[1] <= 100):
        raise ValueError('%s: percentiles must be two numbers [lo, hi] with 0 <= lo < hi <= 100, got %r' % (what, q))
    return dict(max_shift_mm=float(p['max_shift_mm']), max_slices=int(p['max_slices']), bins=int(p['bins']), levels=int(p['levels']),
                min_overlap=float(p['min_overlap']), percentiles=[float(q[0]), float(q[1])])


def align_quantise(x, resampled, knots, bins):
    """q [S,RH,RW] uint8 on the device: the raw slices x [S,H,W] fp32 resampled to `resampled` = (RH, RW) as preprocess_images resamples
    them, binned between knots = (lo, hi) (fp32 [2] or [1,2] on the device: preprocess_quantiles' result, per volume) into `bins` = 2..64
    levels (csrc/align.hip; the rule is in include/mmseg_hip.h).  No host synchronisation."""
    if x.dim() != 3 or x.dtype != torch.float32:
        raise ValueError('align_quantise: x must be an fp32 [S,H,W] tensor, got %s %s' % (x.dtype, tuple(x.shape)))
    S, H, W = x.shape
    RH, RW = int(resampled[0]), int(resampled[1])
    if isinstance(bins, bool) or not isinstance(bins, (int, np.integer)) or not 2 <= bins <= ALIGN_MAX_BINS:
        raise ValueError('align_quantise: bins must be a whole number in 2..%d, got %r' % (ALIGN_MAX_BINS, bins))
    if knots.dtype != torch.float32 or knots.numel() != 2 or knots.device != x.device:
        raise ValueError('align_quantise: knots must be the two fp32 values (lo, hi) on %s, got %s %s' % (x.device, knots.dtype, tuple(knots.shape)))
    if S < 1 or H < 1 or W < 1 or RH < 1 or RW < 1 or S * RH * RW >= 2 ** 31 - 1 or H * W >= 2 ** 31 - 1 or S > 65535:
        raise ValueError('align_quantise: a volume of %d x %d x %d resampled to %d x %d is outside the kernel\'s limits' % (S, H, W, RH, RW))
    q = _new((S, RH, RW), x, torch.uint8)
    N.call('mmseg_align_quantise', _c(x), _c(knots), q, S, H, W, RH, RW, int(bins))
    return q


def _align_frames(op, qa, qb, window):
    for name, q in (('qa', qa), ('qb', qb)):
        if q.dim() != 3 or q.dtype != torch.uint8 or not q.is_contiguous() or min(q.shape) < 1 or q.numel() >= 2 ** 31 - 1:
            raise ValueError('%s: %s must be a contiguous, non-empty uint8 [S,RH,RW] tensor of fewer than 2^31 - 1 bytes, got %s %s'
                             % (op, name, q.dtype, tuple(q.shape)))
    if qb.device != qa.device:
        raise ValueError('%s: qa is on %s, qb on %s' % (op, qa.device, qb.device))
    return _align_shapes(op, tuple(qa.shape), tuple(qb.shape), window)


def _align_shapes(op, shape_a, shape_b, window):
    geo = [int(v) for v in tuple(shape_a) + tuple(shape_b)]
    O = (int(window), int(window)) if _is_number(window) else (int(window[0]), int(window[1]))
    if len(geo) != 6 or min(geo) < 1 or min(O) < 1:
        raise ValueError('%s: shapes %s and %s with a window of %s' % (op, tuple(shape_a), tuple(shape_b), O))
    return geo + list(O)


def _align_stage(op, stage, stride, device):
    """(cand, state, [mode, stride, Z, Py, Px, C]) of a stage description: a sequence / int array [C,3] of (dz, dy, dx) (mode 0), or
    ('lattice', Z, Py, Px) (mode 1), or ('refine', Z, Py, Px, state) with the fp64 [8] state block on the device (mode 2)"""
    t = int(stride)
    if not 1 <= t <= 1 << 16:
        raise ValueError('%s: stride must lie in 1..65536, got %r' % (op, stride))
    if isinstance(stage, tuple) and stage and stage[0] in ('lattice', 'refine'):
        mode = 1 if stage[0] == 'lattice' else 2
        Z, Py, Px = (int(v) for v in stage[1:4])
        state = stage[4] if mode == 2 else None
        if mode == 2 and (not isinstance(state, torch.Tensor) or state.dtype != torch.float64 or state.numel() != ALIGN_STATE):
            raise ValueError('%s: a refinement stage needs the fp64 [%d] state block on the device' % (op, ALIGN_STATE))
        C = N.call('mmseg_align_stage_candidates', mode, t, Z, Py, Px) if min(Z, Py, Px) >= 0 else 0
        if not C:
            raise ValueError('%s: a %s stage of %d slices x %d x %d pixels at stride %d is outside the kernels\' limits (65535 candidates)'
                             % (op, stage[0], Z, Py, Px, t))
        return None, state, [mode, t, Z, Py, Px, int(C)]
    cand = np.asarray(stage.cpu() if isinstance(stage, torch.Tensor) else stage)
    if cand.ndim != 2 or cand.shape[1] != 3 or not 1 <= cand.shape[0] <= 65535 or cand.dtype.kind not in 'iu':
        raise ValueError('%s: candidates must be 1..65535 whole-number rows (dz, dy, dx), got %s %s' % (op, cand.dtype, cand.shape))
    if np.abs(cand).max() > ALIGN_MAX_SHIFT:
        raise ValueError('%s: a candidate shift beyond %d' % (op, ALIGN_MAX_SHIFT))
    dev = torch.from_numpy(np.ascontiguousarray(cand, np.int32)).to(device)
    return dev, None, [0, t, 0, 0, 0, int(cand.shape[0])]


def _align_bins(op, bins):
    if isinstance(bins, bool) or not isinstance(bins, (int, np.integer)) or not 2 <= bins <= ALIGN_MAX_BINS:
        raise ValueError('%s: bins must be a whole number in 2..%d, got %r' % (op, ALIGN_MAX_BINS, bins))
    return int(bins)


def align_histograms(qa, qb, window, stage, stride, bins, aggregate=None, out=None):
    """h [C,bins,bins] int32 on the device: per candidate of `stage` (see _align_stage: a list of (dz, dy, dx), or a lattice /
    refinement description) the joint histogram of the quantised frames qa [Sa,RHa,RWa], qb [Sb,RHb,RWb] (uint8; a byte >= bins counts as
    bins - 1) over the overlap of the frames at `stride`, `window` = the network's input extent O or (OH, OW) that defines the zero
    shift (csrc/align.hip; the rule is in include/mmseg_hip.h).  Exact integer counts; aggregate chooses the kernel's way of adding
    them (None: ALIGN_AGGREGATE) and does not change them.  No host synchronisation."""
    geo = _align_frames('align_histograms', qa, qb, window)
    B = _align_bins('align_histograms', bins)
    cand, state, st = _align_stage('align_histograms', stage, stride, qa.device)
    C = st[-1]
    if out is None:
        out = _new((C, B, B), qa, torch.int32)
    elif out.dtype != torch.int32 or out.numel() != C * B * B or not out.is_contiguous() or out.device != qa.device:
        raise ValueError('align_histograms: out must be a contiguous int32 [%d,%d,%d] tensor on %s' % (C, B, B, qa.device))
    agg = ALIGN_AGGREGATE if aggregate is None else bool(aggregate)
    N.call('mmseg_align_histograms', qa, qb, cand, state, out, *(geo + st + [B, int(agg)]))
    return out


def align_scores(h, shape_a, shape_b, window, stage, stride, min_overlap, out=None):
    """scores [C,2] fp64 on the device = (score, N) per candidate from its table in h [C,bins,bins] int32: Studholme's normalised mutual
    information in fp64, -1 where N == 0, H(A,B) == 0 or the candidate keeps less than min_overlap of the zero shift's overlap
    (shape_a, shape_b = the (S, RH, RW) of the two frames; the rule is in include/mmseg_hip.h)"""
    if h.dim() != 3 or h.dtype != torch.int32 or h.shape[1] != h.shape[2] or not h.is_contiguous():
        raise ValueError('align_scores: h must be a contiguous int32 [C,bins,bins] tensor, got %s %s' % (h.dtype, tuple(h.shape)))
    geo = _align_shapes('align_scores', shape_a, shape_b, window)
    B = _align_bins('align_scores', int(h.shape[1]))
    cand, state, st = _align_stage('align_scores', stage, stride, h.device)
    if st[-1] != h.shape[0]:
        raise ValueError('align_scores: h holds %d tables, the stage has %d candidates' % (h.shape[0], st[-1]))
    if not _is_number(min_overlap) or not 0 <= min_overlap <= 1:
        raise ValueError('align_scores: min_overlap must lie in [0, 1], got %r' % (min_overlap,))
    if out is None:
        out = _new((st[-1], 2), h, torch.float64)
    N.call('mmseg_align_scores', h, cand, state, out, *(geo + st + [B, float(min_overlap)]))
    return out


def align_select(scores, stage, stride, state=None):
    """The stage's best candidate under the tie rule, written into the fp64 [8] state block on the device (a zeroed new one by default)
    and returned: (dz, dy, dx), its score, the zero-shift probe's score, its N, admissible?, stages run (include/mmseg_hip.h)"""
    if scores.dim() != 2 or scores.shape[1] != 2 or scores.dtype != torch.float64 or not scores.is_contiguous():
        raise ValueError('align_select: scores must be a contiguous fp64 [C,2] tensor, got %s %s' % (scores.dtype, tuple(scores.shape)))
    cand, st_state, st = _align_stage('align_select', stage, stride, scores.device)
    if st[-1] != scores.shape[0]:
        raise ValueError('align_select: %d scores, the stage has %d candidates' % (scores.shape[0], st[-1]))
    if state is None:
        state = st_state if st_state is not None else torch.zeros(ALIGN_STATE, dtype=torch.float64, device=scores.device)
    if state.dtype != torch.float64 or state.numel() != ALIGN_STATE or (st_state is not None and state.data_ptr() != st_state.data_ptr()):
        raise ValueError('align_select: state must be the fp64 [%d] block the refinement stage reads' % ALIGN_STATE)
    N.call('mmseg_align_select', scores, cand, state, *st)
    return state


def align_search(qa, qb, window, Z, Py, Px, bins, levels, min_overlap, aggregate=None):
    """The search of include/mmseg_hip.h over quantised frames: the lattice at stride 2^(levels-1), then refinement down to stride 1, every
    stage enumerated, scored and selected on the device -> the fp64 [8] state block on the device.  No host synchronisation."""
    geo = _align_frames('align_search', qa, qb, window)
    B = _align_bins('align_search', bins)
    state = torch.zeros(ALIGN_STATE, dtype=torch.float64, device=qa.device)
    for s in range(int(levels) - 1, -1, -1):
        stage = ('lattice', Z, Py, Px) if s == int(levels) - 1 else ('refine', Z, Py, Px, state)
        C = _align_stage('align_search', stage, 1 << s, qa.device)[2][-1]
        nbytes = N.call('mmseg_align_workspace_bytes', C, B)
        if not nbytes or nbytes > ALIGN_WORKSPACE_CAP:
            raise ValueError('align_search: %d candidates of %d x %d bins need %d MB of histograms (cap %d MB): raise levels, or lower '
                             'max_shift_mm / max_slices / bins' % (C, B, B, (C * B * B * 4) >> 20, ALIGN_WORKSPACE_CAP >> 20))
        ws = _ws('align', nbytes // 8, qa.device, torch.float64)
        words = (C * B * B * 4 + 7) // 8
        h = ws[:words].view(torch.int32)[:C * B * B].view(C, B, B)
        scores = ws[words:words + 2 * C].view(C, 2)
        align_histograms(qa, qb, geo[6:], stage, 1 << s, B, aggregate, out=h)
        align_scores(h, geo[:3], geo[3:6], geo[6:], stage, 1 << s, min_overlap, out=scores)
        align_select(scores, stage, 1 << s, state)
    return state


def align_volumes(a, res_a, b, res_b, target_resolution, input_shape, params=None):
    """The translation that pairs the moving volume b [Sb,Hb,Wb] with the reference volume a [Sa,Ha,Wa] (fp32 raw slices on the device,
    res_x = mm per pixel along rows and columns): ((dz, dy, dx), (score, zero-shift score, N)) -- reference slice i shows the anatomy of
    moving slice i + dz, and the centre window of b's resampled frame moves by (dy, dx) pixels of target_resolution.  params: keys of
    ALIGN_DEFAULTS.  Both volumes are quantised on their resampled grids between their own percentiles and the search maximises
    Studholme's normalised mutual information (csrc/align.hip; the rule is in include/mmseg_hip.h).  One device-to-host copy, at the end."""
    p = align_params(params)
    tr = (float(target_resolution[0]), float(target_resolution[1]))
    qs = []
    for x, res in ((a, res_a), (b, res_b)):
        if x.dim() != 3 or x.dtype != torch.float32 or min(x.shape) < 1:
            raise ValueError('align_volumes: a volume must be a non-empty fp32 [S,H,W] tensor, got %s %s' % (x.dtype, tuple(x.shape)))
        R = tuple(int(np.round(n * (float(r) / t))) for n, r, t in zip(x.shape[1:], res, tr))
        if min(R) < 1:
            raise ValueError('align_volumes: a %d x %d slice at %s mm resamples to nothing at %s mm' % (x.shape[1], x.shape[2], tuple(res), tr))
        n = x.shape[0] * R[0] * R[1]
        ranks = [int(np.floor((n - 1) * (q / 100.0))) for q in p['percentiles']]
        qs.append(align_quantise(x, R, preprocess_quantiles(x, R, ranks, True), p['bins']))
    Py, Px = (int(np.floor(p['max_shift_mm'] / t)) for t in tr)
    state = align_search(qs[0], qs[1], input_shape[:2], p['max_slices'], Py, Px, p['bins'], p['levels'], p['min_overlap'])
    rec = state.cpu().tolist()
    return (int(rec[0]), int(rec[1]), int(rec[2])), (rec[3], rec[4], int(rec[5]))


def restore_label(prob, values, raw_hw, resampled, rows, cols, order=1):
    """prob [S,OH,OW,C] fp32 (a segmentor's output on the device, organ channels first) -> uint8 grey values [S,H,W] on the raw grid
    raw_hw = (H, W) of the volume that preprocess_volume brought to [OH,OW] with `resampled` = (RH, RW) and the per-axis index maps
    rows / cols = (lo, kept, before) (csrc/postprocess.hip): the crop / pad is undone, every organ channel is resampled (order 1:
    bilinear, order 0: nearest) and the pixel gets values[k] of the organ whose probability is > 0.5, or 0; pixels that were cropped
    away get 0.  values [K] int32 on the device, K <= C.  No gradient."""
    H, W = int(raw_hw[0]), int(raw_hw[1])
    RH, RW = int(resampled[0]), int(resampled[1])
    K = int(values.numel())
    if (prob.dim() != 4 or prob.dtype != torch.float32 or values.dtype != torch.int32 or not 1 <= K <= min(16, prob.shape[3])
            or order not in (0, 1) or H < 1 or W < 1):
        raise ValueError('restore_label: prob %s %s, values %s %s, raw size %s, order %r'
                         % (tuple(prob.shape), prob.dtype, tuple(values.shape), values.dtype, (H, W), order))
    S, OH, OW, C = prob.shape
    geo = [int(v) for v in tuple(rows) + tuple(cols)]
    out = _new((S, H, W), prob, torch.uint8)
    N.call('mmseg_restore_label', _c(prob), values, out, S, H, W, RH, RW, OH, OW, *(geo + [C, K, int(order)]))
    return out


def label_overlap(pred, truth, values):
    """pred, truth [S,H,W] uint8 grey values on the device, values [K] int32 -> int32 [S,K,3]: per slice and organ the pixel counts
    |pred == v|, |truth == v| and |both| (csrc/postprocess.hip), what a per-slice Dice on the raw grid is made of"""
    K = int(values.numel())
    if (pred.dim() != 3 or pred.dtype != torch.uint8 or truth.dtype != torch.uint8 or tuple(truth.shape) != tuple(pred.shape)
            or values.dtype != torch.int32 or not 1 <= K <= 16):
        raise ValueError('label_overlap: pred %s %s, truth %s %s, values %s %s'
                         % (tuple(pred.shape), pred.dtype, tuple(truth.shape), truth.dtype, tuple(values.shape), values.dtype))
    S, H, W = pred.shape
    counts = _new((S, K, 3), pred, torch.int32)
    N.call('mmseg_label_overlap', _c(pred), _c(truth), values, counts, S, H * W, K)
    return counts


def _volume_args(op, label, values, others=()):
    """shared checks of the scores in mm: uint8 [S,H,W] volumes of one shape on one device, values [K] int32, 1 <= K <= 16"""
    K = int(values.numel())
    vols = (label,) + tuple(others)
    if (label.dim() != 3 or any(v.dtype != torch.uint8 or tuple(v.shape) != tuple(label.shape) or v.device != label.device for v in vols)
            or values.dtype != torch.int32 or not 1 <= K <= 16 or label.numel() >= 2 ** 31 - 1):
        raise ValueError('%s: volumes %s, values %s %s (expected uint8 [S,H,W] of one shape with fewer than 2^31 voxels and 1..16 int32 '
                         'values)' % (op, ', '.join('%s %s' % (tuple(v.shape), v.dtype) for v in vols), tuple(values.shape), values.dtype))
    return K


def _spacing_args(op, spacing):
    sp = [float(v) for v in spacing]
    if len(sp) != 3 or any(not (v > 0 and v < float('inf')) for v in sp):
        raise ValueError('%s: spacing must be three finite positive numbers (mm between slices, rows, columns), got %r' % (op, spacing))
    return sp


def label_surface(label, values):
    """label [S,H,W] uint8 grey values on the device, values [K] int32 -> uint8 [K+1,S,H,W], 0 or 1: the surface voxels of the K + 1
    binary problems "== values[k]" and, last, "equals any of values" (csrc/postprocess.hip).  A surface voxel is a foreground voxel
    with at least one of its six face neighbours in the background or outside the volume."""
    K = _volume_args('label_surface', label, values)
    S, H, W = label.shape
    surf = _new((K + 1, S, H, W), label, torch.uint8)
    N.call('mmseg_label_surface', _c(label), values, surf, None, S, H, W, K)
    return surf


def distance_to_sites(sites, spacing):
    """sites [S,H,W] uint8 on the device, spacing (dz, dy, dx) in mm -> fp64 [S,H,W]: the exact Euclidean distance in mm to the
    nearest non-zero voxel, +inf everywhere when there is none (csrc/postprocess.hip: three per-axis minimum passes over fp64
    squared distances, one square root)"""
    if sites.dim() != 3 or sites.dtype != torch.uint8 or sites.numel() >= 2 ** 31 - 1:
        raise ValueError('distance_to_sites: sites %s %s (expected uint8 [S,H,W] with fewer than 2^31 voxels)'
                         % (tuple(sites.shape), sites.dtype))
    dz, dy, dx = _spacing_args('distance_to_sites', spacing)
    S, H, W = sites.shape
    out = _new((S, H, W), sites, torch.float64)
    N.call('mmseg_distance_to_sites', _c(sites), out, _ws('edt', sites.numel(), sites.device, torch.float64), S, H, W, dz, dy, dx)
    return out


def surface_metrics(pred, truth, values, spacing):
    """pred, truth [S,H,W] uint8 grey values on the device, values [K] int32, spacing (dz, dy, dx) in mm -> fp64 [K+1,6] per binary
    problem (the K organs, then their union): nP, nT, |surface(P)|, |surface(T)|, the sum and the maximum over both surfaces of the
    distance in mm to the other surface; the last two are nan when either surface is empty (csrc/postprocess.hip).  RAVD, ASSD and
    MSSD follow on the host (volume_predictor.chaos_from_table)."""
    return _surface_table('surface_metrics', pred, truth, values, spacing)


def _robust_args(op, percentile, tolerance):
    q, tau = float(percentile), float(tolerance)
    if not 0.0 <= q <= 100.0:          # false for nan as well
        raise ValueError('%s: percentile must lie in [0, 100], got %r' % (op, percentile))
    if not 0.0 <= tau < float('inf'):
        raise ValueError('%s: tolerance must be a finite number of mm >= 0, got %r' % (op, tolerance))
    return q, tau


def _surface_table(op, pred, truth, values, spacing, robust=None):
    """the body of surface_metrics (robust None -> [K+1,6]) and of surface_scores (robust = (percentile, tolerance) -> [K+1,8]); `op`
    names the C entry point mmseg_<op>, its workspace query and the errors.  Both share one scratch buffer, which the larger sizes."""
    K = _volume_args(op, pred, values, (truth,))
    dz, dy, dx = _spacing_args(op, spacing)
    extra = () if robust is None else _robust_args(op, *robust)
    S, H, W = pred.shape
    table = torch.zeros((K + 1, 6 + len(extra)), dtype=torch.float64, device=pred.device)
    if S == 0:
        table[:, 4:] = float('nan')
        return table
    ws = _ws('surface_metrics', N.call('mmseg_%s_workspace_doubles' % op, S, H, W, K), pred.device, torch.float64)
    N.call('mmseg_' + op, _c(pred), _c(truth), values, table, ws, S, H, W, K, dz, dy, dx, *extra)
    return table


def masked_select(a, ma, b, mb, percentile, tolerance):
    """a, b fp64 and ma, mb uint8, all of one shape on the device -> fp64 [5] = N, |{x <= tolerance}|, the percentile, D_(lo), D_(hi) of
    the multiset D = {a[e] : ma[e] != 0} + {b[e] : mb[e] != 0} (csrc/postprocess.hip: an exact radix selection on the bit patterns).
    The selected values must be finite and >= 0.  numpy.percentile's linear rule: h = (N - 1) * (percentile / 100), lo = floor(h),
    hi = min(lo + 1, N - 1), D_(lo) + (h - lo) * (D_(hi) - D_(lo)); the last three are nan when nothing is selected."""
    q, tau = _robust_args('masked_select', percentile, tolerance)
    if (a.dtype != torch.float64 or b.dtype != torch.float64 or ma.dtype != torch.uint8 or mb.dtype != torch.uint8
            or any(tuple(t.shape) != tuple(a.shape) or t.device != a.device for t in (ma, b, mb)) or a.numel() >= 2 ** 31):
        raise ValueError('masked_select: values %s %s, %s %s, masks %s %s, %s %s (expected fp64 values and uint8 masks of one shape with '
                         'fewer than 2^31 elements)' % (tuple(a.shape), a.dtype, tuple(b.shape), b.dtype, tuple(ma.shape), ma.dtype,
                                                        tuple(mb.shape), mb.dtype))
    n = a.numel()
    out = torch.zeros(5, dtype=torch.float64, device=a.device)
    if n == 0:          # empty tensors have no storage to point at
        out[2:] = float('nan')
        return out
    ws = _ws('masked_select', N.call('mmseg_masked_select_workspace_doubles', n), a.device, torch.float64)
    N.call('mmseg_masked_select', _c(a), _c(ma), _c(b), _c(mb), n, q, tau, out, ws)
    return out


def surface_scores(pred, truth, values, spacing, percentile=95.0, tolerance=1.0):
    """surface_metrics with two more columns -> fp64 [K+1,8]: nP, nT, |surface(P)|, |surface(T)|, sum, max (bit for bit those of
    surface_metrics), then |{x in D : x <= tolerance}| and numpy.percentile(D, percentile), where D holds the distances in mm of
    surface(P) to surface(T) and of surface(T) to surface(P) together; columns 5 to 8 are nan when either surface is empty.  Every
    distance transform runs once.  HD(q) and NSD(tau) follow on the host (volume_predictor.robust_from_table)."""
    return _surface_table('surface_scores', pred, truth, values, spacing, (percentile, tolerance))


def _component_args(op, label, values, connectivity):
    if connectivity not in (6, 26):
        raise ValueError('%s: connectivity must be 6 (faces) or 26 (faces, edges, corners), got %r' % (op, connectivity))
    return _volume_args(op, label, values)


def label_components(label, values, connectivity=6):
    """label [S,H,W] uint8 grey values on the device, values [K] int32 -> int32 [S,H,W]: 0 where the grey value is none of `values`,
    else 1 + the smallest linear index of the voxel's connected component (csrc/postprocess.hip).  Two voxels are joined when they
    hold the same grey value and are neighbours: connectivity 6 (faces) or 26 (faces, edges, corners)."""
    K = _component_args('label_components', label, values, connectivity)
    S, H, W = label.shape
    comp = _new((S, H, W), label, torch.int32)
    if S:
        N.call('mmseg_label_components', _c(label), values, comp, S, H, W, K, int(connectivity))
    return comp


def keep_largest_components(label, values, connectivity=6):
    """label [S,H,W] uint8 on the device, values [K] int32 -> (uint8 [S,H,W], int32 [K,3]): the volume with every organ voxel outside
    its organ's largest connected component set to 0 (of equally large ones the component with the smallest linear index stays;
    other grey values are copied), and per organ (number of components, voxels before, voxels kept) (csrc/postprocess.hip)"""
    K = _component_args('keep_largest_components', label, values, connectivity)
    S, H, W = label.shape
    out = _new((S, H, W), label, torch.uint8)
    stats = torch.zeros((K, 3), dtype=torch.int32, device=label.device)
    if S:
        ws = _ws('keep_largest', (N.call('mmseg_keep_largest_workspace_bytes', S, H, W, K) + 3) // 4, label.device, torch.int32)
        N.call('mmseg_keep_largest_components', _c(label), values, out, stats, ws, S, H, W, K, int(connectivity))
    return out, stats


HOLE_MODES = ('2d', '3d')


def fill_label_holes(label, values, mode='3d'):
    """label [S,H,W] uint8 on the device, values [K] int32 -> (uint8 [S,H,W], int32 [K,3]): the volume with the zeros that organ k
    encloses set to values[k], and per organ (number of holes, voxels before, voxels added) (csrc/postprocess.hip).  A hole of organ k
    is a connected component of the complement of (label == values[k]), joined through faces only, that holds no border voxel: of
    the volume with mode '3d', of its slice with mode '2d', where every slice is a problem of its own.  Holes are those of the
    input; only zeros are filled, and where several organs enclose a voxel the lowest k wins."""
    if mode not in HOLE_MODES:
        raise ValueError("fill_label_holes: mode must be '2d' (every slice on its own) or '3d', got %r" % (mode,))
    K = _volume_args('fill_label_holes', label, values)
    S, H, W = label.shape
    out = _new((S, H, W), label, torch.uint8)
    stats = torch.zeros((K, 3), dtype=torch.int32, device=label.device)
    if S:
        ws = _ws('fill_holes', (N.call('mmseg_fill_label_holes_workspace_bytes', S, H, W, K) + 3) // 4, label.device)
        N.call('mmseg_fill_label_holes', _c(label), values, out, stats, ws, S, H, W, K, int(mode == '2d'))
    return out, stats


MAX_TILES = 8          # per axis (csrc/postprocess.hip)


def blend_tiles(prob, rows, cols, wr, wc, S, resampled, K):
    """prob [TR*TC*S,OH,OW,C] fp32 on the device: a segmentor's output for the tiles of one volume, tile-major (tile tr * TC + tc holds
    S slices), organ channels first -> fp32 [S,RH,RW,K], the blended map on the resampled frame `resampled` = (RH, RW)
    (csrc/postprocess.hip).  rows [TR,3] / cols [TC,3]: per tile and axis (lo, kept, before) as given to preprocess_images; wr [TR,OH] /
    wc [TC,OW]: the weights along each axis (loaders/volume_folder.tile_weights).  Host sequences or device tensors.  Every frame pixel
    gets the mean of the tiles that cover it, weighted by wr * wc; one covering tile is copied as it is.  No gradient."""
    RH, RW = int(resampled[0]), int(resampled[1])
    S, K = int(S), int(K)

    def table(x, dtype, width):
        t = x if isinstance(x, torch.Tensor) else torch.as_tensor(x, dtype=dtype)
        if t.dim() != 2 or t.dtype != dtype or t.shape[1] != width or not 1 <= t.shape[0] <= MAX_TILES:
            raise ValueError('blend_tiles: expected a [1..%d, %d] %s table, got %s %s' % (MAX_TILES, width, dtype, tuple(t.shape), t.dtype))
        return _c(t.to(prob.device))
    if prob.dim() != 4 or prob.dtype != torch.float32 or S < 0 or RH < 1 or RW < 1 or not 1 <= K <= min(16, prob.shape[3]):
        raise ValueError('blend_tiles: prob %s %s, S = %d, resampled %s, K = %d' % (tuple(prob.shape), prob.dtype, S, (RH, RW), K))
    N_, OH, OW, C = prob.shape
    rows, cols = table(rows, torch.int32, 3), table(cols, torch.int32, 3)
    wr, wc = table(wr, torch.float32, OH), table(wc, torch.float32, OW)
    TR, TC = rows.shape[0], cols.shape[0]
    if wr.shape[0] != TR or wc.shape[0] != TC or N_ != TR * TC * S:
        raise ValueError('blend_tiles: prob %s does not hold %d x %d tiles of %d slices (weights %s, %s)'
                         % (tuple(prob.shape), TR, TC, S, tuple(wr.shape), tuple(wc.shape)))
    if max(prob.numel(), S * RH * RW * K) * 4 >= 2 ** 31:
        raise ValueError('blend_tiles: prob %s or the map %s holds 2^31 bytes or more' % (tuple(prob.shape), (S, RH, RW, K)))
    out = _new((S, RH, RW, K), prob)
    if S:
        N.call('mmseg_blend_tiles', _c(prob), rows, cols, wr, wc, out, S, TR, TC, OH, OW, C, K, RH, RW)
    return out


MAX_VIEWS = 16          # csrc/postprocess.hip


def merge_views(prob, back, N_, K):
    """prob [V*N,OH,OW,C] fp32 on the device: a segmentor's output for V views of N slices, view-major (view v holds slices v * N ..),
    organ channels first -> fp32 [N,OH,OW,K], at every pixel the mean over the views that cover it of the view's map sampled at
    back[v] (r, c) (csrc/postprocess.hip).  back [V,6] fp64: per view the matrix from an image pixel to the view pixel that shows it,
    in augment_gather's convention; a host array or a device tensor.  A pixel that one view covers is that view's sample as it is, a
    pixel that none covers gets 0, and an integer coordinate is a copy.  No gradient."""
    n, K = int(N_), int(K)
    b = back if isinstance(back, torch.Tensor) else torch.as_tensor(back, dtype=torch.float64)
    if b.dim() != 2 or b.dtype != torch.float64 or b.shape[1] != 6 or not 1 <= b.shape[0] <= MAX_VIEWS:
        raise ValueError('merge_views: expected a [1..%d, 6] float64 table of views, got %s %s' % (MAX_VIEWS, tuple(b.shape), b.dtype))
    if prob.dim() != 4 or prob.dtype != torch.float32 or n < 0 or not 1 <= K <= min(16, prob.shape[3]):
        raise ValueError('merge_views: prob %s %s, N = %d, K = %d' % (tuple(prob.shape), prob.dtype, n, K))
    V, (M, OH, OW, C) = b.shape[0], prob.shape
    if M != V * n:
        raise ValueError('merge_views: prob %s does not hold %d views of %d slices' % (tuple(prob.shape), V, n))
    if prob.numel() * 4 >= 2 ** 31:
        raise ValueError('merge_views: prob %s holds 2^31 bytes or more' % (tuple(prob.shape),))
    out = _new((n, OH, OW, K), prob)
    if n:
        N.call('mmseg_merge_views', _c(prob), _c(b.to(prob.device)), out, V, n, OH, OW, C, K)
    return out


IDENTITY_VIEW = ((1.0, 0.0, 0.0, 0.0, 1.0, 0.0),)          # `back` of a model that predicts every slice once
MAX_PLANES = 4          # csrc/postprocess.hip
MAX_CALIBRATION_BINS = 64


def members_accumulate(prob, back, N_, K, state=None):
    """One member of an ensemble.  prob [V*N,OH,OW,C] fp32 on the device: ONE model's output for V views of N slices, as for merge_views
    (back [V,6] fp64; IDENTITY_VIEW for a plain model) -> state = (sum [N,OH,OW,K], aux [N,OH,OW,2]) fp32 (csrc/postprocess.hip): per
    pixel the sum of the covering views' samples, the sum of their entropies and their number.  state=None starts from 0 in new
    buffers; otherwise the call continues from `state`, in place, and returns it: one call per model, any number of models.
    members_finish turns the state into the mean map and the uncertainty planes.  No gradient."""
    n, K = int(N_), int(K)
    b = back if isinstance(back, torch.Tensor) else torch.as_tensor(back, dtype=torch.float64)
    if b.dim() != 2 or b.dtype != torch.float64 or b.shape[1] != 6 or not 1 <= b.shape[0] <= MAX_VIEWS:
        raise ValueError('members_accumulate: expected a [1..%d, 6] float64 table of views, got %s %s' % (MAX_VIEWS, tuple(b.shape), b.dtype))
    if prob.dim() != 4 or prob.dtype != torch.float32 or n < 0 or not 1 <= K <= min(16, prob.shape[3]):
        raise ValueError('members_accumulate: prob %s %s, N = %d, K = %d' % (tuple(prob.shape), prob.dtype, n, K))
    V, (M, OH, OW, C) = b.shape[0], prob.shape
    if M != V * n:
        raise ValueError('members_accumulate: prob %s does not hold %d views of %d slices' % (tuple(prob.shape), V, n))
    if prob.numel() * 4 >= 2 ** 31:
        raise ValueError('members_accumulate: prob %s holds 2^31 bytes or more' % (tuple(prob.shape),))
    if state is None:
        total, aux = _new((n, OH, OW, K), prob), _new((n, OH, OW, 2), prob)
    else:
        total, aux = state
        for t, last in ((total, K), (aux, 2)):
            if (not isinstance(t, torch.Tensor) or t.dtype != torch.float32 or tuple(t.shape) != (n, OH, OW, last) or not t.is_contiguous()
                    or t.device != prob.device):
                raise ValueError('members_accumulate: the state does not belong to %d slices of %d x %d with K = %d' % (n, OH, OW, K))
    if n:
        N.call('mmseg_members_accumulate', _c(prob), _c(b.to(prob.device)), total, aux, int(state is None), V, n, OH, OW, C, K)
    return total, aux


def members_finish(state):
    """state = (sum, aux) of members_accumulate -> (mean [N,OH,OW,K], planes [N,OH,OW,2]) fp32, IN PLACE (the same two tensors): the mean
    over every covering view of every member (one member: merge_views's map bit for bit), and per pixel (H, I) in [0, 1]: the entropy
    of the mean over the K organs and the rest, and the mutual information (H minus the mean of the members' entropies), both divided
    by ln(K + 1).  A pixel that nothing covers gets 0 everywhere.  A state is finished once."""
    total, aux = state
    if (not isinstance(total, torch.Tensor) or not isinstance(aux, torch.Tensor) or total.dim() != 4 or total.dtype != torch.float32
            or aux.dtype != torch.float32 or not 1 <= total.shape[3] <= 16 or tuple(aux.shape) != tuple(total.shape[:3]) + (2,)
            or not total.is_contiguous() or not aux.is_contiguous() or aux.device != total.device):
        raise ValueError('members_finish: expected the (sum [N,OH,OW,K], aux [N,OH,OW,2]) fp32 pair of members_accumulate')
    n, OH, OW, K = total.shape
    if n:
        N.call('mmseg_members_finish', total, aux, n, OH, OW, K)
    return total, aux


def restore_map(planes, u, raw_hw, resampled, rows, cols, order=1):
    """planes [S,OH,OW,U] fp32 on the device (U <= 4 maps with values in [0, 1], such as the planes of members_finish) -> plane u as
    uint8 levels [S,H,W] on the raw grid, level = round(255 * value), by the geometry and the taps of restore_label
    (csrc/postprocess.hip); pixels that were cropped away get 0.  No gradient."""
    H, W = int(raw_hw[0]), int(raw_hw[1])
    RH, RW = int(resampled[0]), int(resampled[1])
    if (planes.dim() != 4 or planes.dtype != torch.float32 or not 1 <= planes.shape[3] <= MAX_PLANES or not 0 <= int(u) < planes.shape[3]
            or order not in (0, 1) or H < 1 or W < 1):
        raise ValueError('restore_map: planes %s %s, plane %r, raw size %s, order %r' % (tuple(planes.shape), planes.dtype, u, (H, W), order))
    S, OH, OW, U = planes.shape
    geo = [int(v) for v in tuple(rows) + tuple(cols)]
    out = _new((S, H, W), planes, torch.uint8)
    N.call('mmseg_restore_map', _c(planes), out, S, H, W, RH, RW, OH, OW, *(geo + [U, int(u), int(order)]))
    return out


def calibration_table(prob, truth, values, resampled, rows, cols, bins=10, order=1):
    """prob [S,OH,OW,C] fp32 and truth [S,H,W] uint8 on the device, values [K] int32 -> (counts int32 [K,B,2], sums fp64 [K,B+2])
    (csrc/postprocess.hip): every organ channel is sampled at every raw pixel inside the window exactly as restore_label samples it and
    falls into bin min(B - 1, int(p * B)); counts = (pixels, pixels whose truth is values[k]) per bin; sums = the sum of p per bin, then
    the sum of (p - y)^2 and of -log(max(p of what is true, 1e-6)).  ECE, MCE, the Brier score and the NLL follow on the host
    (volume_predictor.calibration_scores).  Integer counts and fixed-order fp64 sums: two runs are bitwise equal."""
    B, K = int(bins), int(values.numel())
    RH, RW = int(resampled[0]), int(resampled[1])
    if (prob.dim() != 4 or prob.dtype != torch.float32 or truth.dim() != 3 or truth.dtype != torch.uint8 or truth.shape[0] != prob.shape[0]
            or values.dtype != torch.int32 or not 1 <= K <= min(16, prob.shape[3]) or not 2 <= B <= MAX_CALIBRATION_BINS
            or order not in (0, 1) or min(truth.shape[1:]) < 1):
        raise ValueError('calibration_table: prob %s %s, truth %s %s, values %s %s, bins %r, order %r'
                         % (tuple(prob.shape), prob.dtype, tuple(truth.shape), truth.dtype, tuple(values.shape), values.dtype, bins, order))
    S, OH, OW, C = prob.shape
    H, W = truth.shape[1:]
    geo = [int(v) for v in tuple(rows) + tuple(cols)]
    counts = torch.zeros((K, B, 2), dtype=torch.int32, device=prob.device)
    sums = torch.zeros((K, B + 2), dtype=torch.float64, device=prob.device)
    if S:
        ws = _ws('calibration', (N.call('mmseg_calibration_table_workspace_bytes', S, H, W, K, B) + 7) // 8, prob.device, torch.float64)
        N.call('mmseg_calibration_table', _c(prob), _c(truth), values, counts, sums, ws, S, H, W, RH, RW, OH, OW, *(geo + [C, K, B, int(order)]))
    return counts, sums


def uncertainty_by_error(pred, truth, levels):
    """pred, truth uint8 of one shape and levels uint8 [U, that shape] (U <= 4 planes of restore_map) on the device -> int64 [2,1+U]
    (csrc/postprocess.hip): row 0 over the pixels with pred == truth, row 1 over the others; a row holds the number of pixels and per
    plane the sum of their levels.  sum / (255 * count) is the mean uncertainty where the labels are right, or wrong."""
    if (pred.dtype != torch.uint8 or truth.dtype != torch.uint8 or levels.dtype != torch.uint8 or tuple(truth.shape) != tuple(pred.shape)
            or levels.dim() != pred.dim() + 1 or not 1 <= levels.shape[0] <= MAX_PLANES or tuple(levels.shape[1:]) != tuple(pred.shape)
            or pred.numel() >= 2 ** 31 - 1):
        raise ValueError('uncertainty_by_error: pred %s %s, truth %s %s, levels %s %s'
                         % (tuple(pred.shape), pred.dtype, tuple(truth.shape), truth.dtype, tuple(levels.shape), levels.dtype))
    U, n = levels.shape[0], pred.numel()
    out = torch.zeros((2, 1 + U), dtype=torch.int64, device=pred.device)
    if n:
        N.call('mmseg_uncertainty_by_error', _c(pred), _c(truth), _c(levels), out, n, U)
    return out


# the parameters of crf_refine, in the order of the entry point; the defaults are starting values that nobody has tuned
CrfParams = collections.namedtuple('CrfParams', ('radius', 'iterations', 'w_a', 'theta_alpha', 'theta_beta', 'w_s', 'theta_gamma'))
CRF_DEFAULTS = CrfParams(radius=5, iterations=5, w_a=4.0, theta_alpha=3.0, theta_beta=0.1, w_s=1.0, theta_gamma=1.5)
CRF_MAX_RADIUS, CRF_MAX_ITERATIONS = 8, 20          # csrc/crf.hip
CRF_WORKSPACE_CAP = 256 << 20


def crf_params(params, what='crf_refine'):
    """params: a CrfParams or a sequence in its order -> a CrfParams of two ints and five floats within the limits of the rule: radius
    1..8, iterations 1..20, the three theta finite and > 0, w_a and w_s finite and >= 0 and not both 0.  Raises ValueError otherwise."""
    def refuse(why):
        raise ValueError('%s: %s, got %r' % (what, why, params))
    try:
        p = CrfParams(*params)
    except TypeError:
        refuse('expected (%s)' % ', '.join(CrfParams._fields))
    whole = all(isinstance(v, (int, np.integer)) and not isinstance(v, bool) for v in p[:2])
    if not whole or not 1 <= p.radius <= CRF_MAX_RADIUS or not 1 <= p.iterations <= CRF_MAX_ITERATIONS:
        refuse('radius must be a whole number in 1..%d and iterations one in 1..%d' % (CRF_MAX_RADIUS, CRF_MAX_ITERATIONS))
    try:
        reals = [float(v) for v in p[2:]]
    except (TypeError, ValueError):
        refuse('the weights and the theta must be numbers')
    if any(isinstance(v, bool) for v in p[2:]) or not all(math.isfinite(v) for v in reals):
        refuse('the weights and the theta must be finite numbers')
    # what the kernel sees is fp32: a value that rounds to 0 or to inf there is refused here as well
    with np.errstate(over='ignore', under='ignore'):
        seen = CrfParams(0, 0, *(float(np.float32(v)) for v in reals))
    if not all(0 < v < float('inf') for v in (seen.theta_alpha, seen.theta_beta, seen.theta_gamma)):
        refuse('theta_alpha, theta_beta and theta_gamma must be finite and > 0 in fp32')
    if not all(0 <= v < float('inf') for v in (seen.w_a, seen.w_s)) or (seen.w_a == 0 and seen.w_s == 0):
        refuse('w_a and w_s must be finite and >= 0 in fp32, and not both 0')
    return CrfParams(int(p.radius), int(p.iterations), *reals)


def crf_refine(prob, image, K, params=CRF_DEFAULTS, max_workspace_bytes=CRF_WORKSPACE_CAP):
    """prob [N,H,W,C] fp32 on the device: a segmentor's output, the K organ channels first; image [N,H,W,1] fp32: the slices it saw, in
    [-1, 1] -> fp32 [N,H,W,K], the organ channels after `params.iterations` mean-field iterations of the windowed CRF of INTEGRATION.md
    section 5 (csrc/crf.hip): K + 1 labels (the organs and the rest), an appearance and a smoothness kernel over the (2 radius + 1)^2
    window, each normalised by its own sum.  Slices are independent; they run in chunks whose workspace (two Q buffers of K + 1 planes)
    stays under max_workspace_bytes (one slice at least), with bitwise the result of one call.  No gradient."""
    p = crf_params(params)
    K = int(K)
    if (prob.dim() != 4 or prob.dtype != torch.float32 or image.dtype != torch.float32 or image.device != prob.device
            or tuple(image.shape) != tuple(prob.shape[:3]) + (1,) or not 1 <= K <= min(16, prob.shape[3]) or min(prob.shape[1:3]) < 1):
        raise ValueError('crf_refine: prob %s %s, image %s %s on %s and %s, K = %d: expected fp32 [N,H,W,C] and [N,H,W,1] on one device, '
                         '1 <= K <= min(C, 16)' % (tuple(prob.shape), prob.dtype, tuple(image.shape), image.dtype, prob.device, image.device, K))
    n, H, W, C = (int(v) for v in prob.shape)
    if prob.numel() * 4 >= 2 ** 31:
        raise ValueError('crf_refine: prob %s holds 2^31 bytes or more' % (tuple(prob.shape),))
    if isinstance(max_workspace_bytes, bool) or not isinstance(max_workspace_bytes, (int, np.integer)) or max_workspace_bytes < 1:
        raise ValueError('crf_refine: max_workspace_bytes must be a whole number of bytes >= 1, got %r' % (max_workspace_bytes,))
    out = _new((n, H, W, K), prob)
    if n == 0:
        return out
    prob, image = _c(prob), _c(image)
    one, two = (N.call('mmseg_crf_refine_workspace_bytes', s, H, W, K) for s in (1, 2))
    if one <= 0:
        raise ValueError('crf_refine: a slice of %d x %d with %d channels is more than one call holds' % (H, W, C))
    per_slice = two - one if two > 0 else one
    step = int(min(n, max(1, (int(max_workspace_bytes) - (one - per_slice)) // per_slice)))
    ws = _ws('crf_refine', (N.call('mmseg_crf_refine_workspace_bytes', step, H, W, K) + 3) // 4, prob.device)
    for i in range(0, n, step):
        s = min(step, n - i)
        N.call('mmseg_crf_refine', prob[i:i + s], image[i:i + s], out[i:i + s], ws, s, H, W, C, K, p.radius, p.iterations, p.w_a,
               p.theta_alpha, p.theta_beta, p.w_s, p.theta_gamma)
    return out


SMOOTH_OPS = ('open', 'close', 'smooth')
SMOOTH_EXTENTS = ('2d', '3d')
SMOOTH_MAX_REACH = 32


def smooth_reach(spacing, radius, extent='2d'):
    """the reach of the ball in voxels per axis in use, floor(radius / spacing): (rows, columns) with extent '2d', (slices, rows,
    columns) with '3d'; spacing = (mm between slices, rows, columns)"""
    return tuple(int(math.floor(min(radius / s, 2.0 ** 31))) for s in (spacing[1:] if extent == '2d' else spacing))


def smooth_label(label, values, spacing, radius, op='smooth', extent='2d'):
    """label [S,H,W] uint8 on the device, values [K] int32, spacing (mm between slices, rows, columns), radius in mm -> (uint8 [S,H,W],
    int32 [K,3]): every organ opened ('open'), closed ('close') or opened and then closed ('smooth') by the ball of that radius on the
    volume's grid, and per organ (voxels before, removed, added) (csrc/postprocess.hip; the rule is in INTEGRATION.md section 5).  The
    ball holds the offsets o with (dx ox)^2 + (dy oy)^2 + (dz oz)^2 <= radius^2; with extent '2d' it lies in the slice and the first
    spacing is not read (it may be None).  Erosion does not see beyond the volume: open(X) = dilate(erode(X)) is a subset of X,
    close(X) = erode(dilate(X)) a superset.  'open' zeroes the voxels of values[k] outside the opened organ; 'close' gives the input's
    zeros inside the closed organ to it, the lowest k first, and overwrites nothing else.  At most 32 voxels of reach per axis."""
    name = 'smooth_label'
    if op not in SMOOTH_OPS:
        raise ValueError("%s: op must be one of %s, got %r" % (name, ', '.join(SMOOTH_OPS), op))
    if extent not in SMOOTH_EXTENTS:
        raise ValueError("%s: extent must be '2d' (the ball lies in the slice) or '3d', got %r" % (name, extent))
    K = _volume_args(name, label, values)
    try:
        sp = [0.0 if (extent == '2d' and i == 0) else float(v) for i, v in enumerate(spacing)]
        r = float(radius)
    except (TypeError, ValueError):
        raise ValueError('%s: spacing must be three numbers and radius one, got %r and %r' % (name, spacing, radius))
    used = sp[1:] if extent == '2d' else sp
    if len(sp) != 3 or any(not (v > 0 and v < float('inf')) for v in used):
        raise ValueError('%s: spacing must be three finite positive numbers (mm between slices, rows, columns; the first is not read '
                         "with extent '2d'), got %r" % (name, spacing))
    if not (r > 0 and r < float('inf')):
        raise ValueError('%s: radius must be a finite number of mm > 0, got %r' % (name, radius))
    reach = smooth_reach(sp, r, extent)
    if max(reach) > SMOOTH_MAX_REACH:
        raise ValueError('%s: a radius of %r mm at spacing %r reaches %s voxels per axis, at most %d'
                         % (name, radius, tuple(spacing), reach, SMOOTH_MAX_REACH))
    S, H, W = label.shape
    out = _new((S, H, W), label, torch.uint8)
    stats = torch.zeros((K, 3), dtype=torch.int32, device=label.device)
    if S:
        ws = _ws('smooth_label', (N.call('mmseg_smooth_label_workspace_bytes', S, H, W, K) + 3) // 4, label.device)
        N.call('mmseg_smooth_label', _c(label), values, out, stats, ws, S, H, W, K, sp[0], sp[1], sp[2], r, SMOOTH_OPS.index(op),
               int(extent == '2d'))
    return out, stats


def _sum_n(gs, like):
    """sum of 1..n same-shaped tensors in as few launches as possible (8 operands per launch, left to right)"""
    gs = [_c(g) for g in gs]
    while len(gs) > 1:
        grp, rest = gs[:8], gs[8:]
        out = _new(like.shape, like, grp[0].dtype)
        assert all(g.dtype == grp[0].dtype and g.shape == grp[0].shape for g in grp)
        N.call('mmseg_sum_n_t', *(grp + [None] * (8 - len(grp))), len(grp), out, out.numel(), _h(out))
        gs = [out] + rest
    return gs[0]


class _Share(torch.autograd.Function):
    """n aliases of x for n consumers.  The autograd engine adds the gradients of a tensor with several consumers pairwise with torch
    kernels (46 additions per DAFNet generator step; 6 of them chained for the anatomy factor alone); consumers that take their
    own alias meet again HERE, where one launch adds all of them (mmseg_sum_n_t)."""

    @staticmethod
    def forward(ctx, x, n):
        ctx.set_materialize_grads(False)
        return tuple(x.view_as(x) for _ in range(n))

    @staticmethod
    def backward(ctx, *gs):
        gs = [g for g in gs if g is not None]
        if not gs:
            return None, None
        return _sum_n(gs, gs[0]), None


class Shared(object):
    """`s = Shared(x, n)`; every consumer calls `s.use()` (the n-th use hands out the last alias; more uses raise).  Without a tape
    (inference) it hands out x itself."""

    def __init__(self, x, n):
        self.x, self.n, self.i = x, n, 0
        self.parts = _Share.apply(x, n) if (n > 1 and torch.is_grad_enabled() and x.requires_grad) else None

    def use(self):
        if self.parts is None:
            return self.x
        if self.i >= self.n:
            raise RuntimeError('Shared tensor declared for %d consumers is used a %d-th time' % (self.n, self.i + 1))
        self.i += 1
        return self.parts[self.i - 1]


def share(x, n):
    """-> list of n aliases of x, one per consumer (see _Share)"""
    sh = Shared(x, n)
    return [sh.use() for _ in range(n)]


def _cat_words(parts, out):
    """out (contiguous, n * len(part) rows) <- parts stacked on the leading axis; a None part is written as zeros"""
    n = len(parts)
    B = out.shape[0] // n
    words = (out.numel() // n) * out.element_size()
    assert words % 4 == 0, 'batch concatenation moves 4-byte words'
    words //= 4
    for k0 in range(0, n, 8):
        grp = parts[k0:k0 + 8]
        N.call('mmseg_cat_words', *(list(grp) + [None] * (8 - len(grp))), len(grp), out[k0 * B:(k0 + len(grp)) * B], words)


class _CatBatch(torch.autograd.Function):
    @staticmethod
    def forward(ctx, *ts):
        ts = [_c(t) for t in ts]
        t0 = ts[0]
        assert all(t.shape == t0.shape and t.dtype == t0.dtype for t in ts), 'cat_batch: equally shaped parts'
        out = _new((len(ts) * t0.shape[0],) + tuple(t0.shape[1:]), t0, t0.dtype)
        _cat_words(ts, out)
        ctx.n, ctx.B = len(ts), t0.shape[0]
        return out

    @staticmethod
    def backward(ctx, g):
        g = _c(g)
        return tuple(g[i * ctx.B:(i + 1) * ctx.B] for i in range(ctx.n))      # contiguous row blocks: views, nothing is copied


class _SplitBatch(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, n):
        ctx.set_materialize_grads(False)
        x = _c(x)
        assert x.shape[0] % n == 0
        B = x.shape[0] // n
        ctx.meta = (tuple(x.shape), x.dtype, n)
        return tuple(x[i * B:(i + 1) * B] for i in range(n))

    @staticmethod
    def backward(ctx, *gs):
        shape, dtype, n = ctx.meta
        like = next((g for g in gs if g is not None), None)
        if like is None:
            return None, None
        out = torch.empty(shape, dtype=dtype, device=like.device)
        _cat_words([_c(g) if g is not None else None for g in gs], out)
        return out, None


def cat_batch(tensors):
    """Stack independent calls of a per-sample component on the batch axis (pure data movement in one launch, mmseg_cat_words; the
    backward pass hands every producer its row block of the gradient as a view).  Components without batch statistics --
    discriminators, FiLM / SPADE decoders, the anatomy fuser, inference-mode BatchNorm -- give identical per-sample results, with
    1/n of the launches and GEMMs large enough to fill the chip."""
    tensors = list(tensors)
    if len(tensors) == 1:
        return tensors[0]
    return _CatBatch.apply(*tensors)


def split_batch(t, n):
    """inverse of cat_batch for n equal parts (views; their gradients are gathered into one tensor by one launch)"""
    if n == 1:
        return [t]
    return list(_SplitBatch.apply(t, n))


def gather_rows(src, idx):
    """src[idx] along the leading axis (idx: int64 device tensor): sampling a fake pool (utils/data_utils.py sample of the reference)"""
    src = _c(src)
    rows = idx.numel()
    out = _new((rows,) + tuple(src.shape[1:]), src, src.dtype)
    row_bytes = (src.numel() // max(src.shape[0], 1)) * src.element_size()
    assert row_bytes % 4 == 0
    N.call('mmseg_gather_rows', src, idx, out, rows, row_bytes // 4, src.shape[0])
    return out


def add_residual(m):
    """[..., C] masks -> [..., C + 1]: background channel = 1 unless some mask equals 1 exactly (base_executor.py:83-87)"""
    m = _c(m)
    C = m.shape[-1]
    out = _new(tuple(m.shape[:-1]) + (C + 1,), m)
    N.call('mmseg_add_residual', m, out, m.numel() // C, C)
    return out
