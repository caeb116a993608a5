"""numpy restatement (fp64) of the Lovasz-Softmax loss of csrc/lovasz.hip -- the signed map m, the term and the gradient added into
dpred -- the prediction / mask contents the tests run on, and TEST-ONLY torch-CPU stand-ins of the new entry points (registered into
tests.cpu_backend._TABLE by a fixture of tests/test_lovasz_loss.py; never a fallback of the product).

Definition (include/mmseg_hip.h).  Per sample b and organ channel k < nm, over the P = H * W pixels:
    y_i = target > 0.5,   e_i = |y_i - p_i| computed in float32 (one subtraction: the ties are the device's ties)
    order: e descending, equal e by pixel index ascending = numpy.argsort(-e, kind='stable')
    G = sum y;  c / n = positives / negatives strictly before a sorted position
    g = 1 / (G + n)  (y = 1);   (G - c) / ((G + n) (G + n + 1))  (y = 0, G > 0);   G = 0: 1 at the first position, 0 elsewhere
    m = s g q_b, s = +1 (y = 0) / -1 (y = 1), m = 0 where e == 0, q_b = 1 / (B |K_b|), K_b = classes with G > 0 ('present') or all nm
    L = sum m (p - y),  dL/dp = m.
Everything after e is fp64 from exact integers."""
import functools

import numpy as np
import torch

MAXC, MAXHW, CHUNKS, TILE, WAVE = 8, 1 << 22, 128, 2048, 512

PRED_KINDS = ('uniform', 'softmax_like', 'constant', 'quantised', 'low_bits', 'all_exponents')
MASK_KINDS = ('mixed', 'edges')          # 'edges': per (b, k) in turn empty, full, a single positive pixel, mixed


# ---- the map --------------------------------------------------------------------------------------------------------------------------
def errors_f32(pred, target, nm):
    """-> (e float32 [B,P,nm], y bool [B,P,nm])"""
    p = np.asarray(pred, np.float32)
    B, C = p.shape[0], p.shape[-1]
    p = p.reshape(B, -1, C)[..., :nm]
    y = np.asarray(target).reshape(B, -1, C)[..., :nm] > 0.5
    e = np.abs(y.astype(np.float32) - p)
    assert e.dtype == np.float32
    return e, y


def lovasz_grad_closed(ys):
    """sorted labels (bool [P]) -> g fp64 [P], the closed form of J_k - J_{k-1}"""
    ys = np.asarray(ys, bool)
    P = ys.size
    G = int(ys.sum())
    c = np.cumsum(ys) - ys                       # positives strictly before
    n = np.arange(P) - c                         # negatives strictly before
    if G == 0:
        g = np.zeros(P, np.float64)
        g[0] = 1.0
        return g
    Gn = (G + n).astype(np.float64)
    return np.where(ys, 1.0 / Gn, (G - c).astype(np.float64) / (Gn * (Gn + 1.0)))


def map_ref(pred, target, nm, classes_all=False):
    """-> dict(m fp64 [B,P,nm], order int64 [B,nm,P], e float32, y bool, term fp64 [B,nm] = L_{b,k}, q fp64 [B])"""
    e, y = errors_f32(pred, target, nm)
    B, P, _ = e.shape
    m = np.zeros((B, P, nm), np.float64)
    order = np.zeros((B, nm, P), np.int64)
    term = np.zeros((B, nm), np.float64)
    q = np.zeros(B, np.float64)
    for b in range(B):
        G = y[b].sum(0)
        nk = nm if classes_all else int((G > 0).sum())
        q[b] = 1.0 / (float(B) * nk) if nk > 0 else 0.0
        for k in range(nm):
            o = np.argsort(-e[b, :, k], kind='stable')
            order[b, k] = o
            ys = y[b, o, k]
            g = lovasz_grad_closed(ys)
            term[b, k] = float(np.dot(e[b, o, k].astype(np.float64), g))
            v = np.where(ys, -g, g) * (q[b] if classes_all or G[k] > 0 else 0.0)      # a class outside K_b pays nothing
            v[e[b, o, k] == 0] = 0.0
            m[b, o, k] = v
    return dict(m=m, order=order, e=e, y=y, term=term, q=q)


def loss_ref(pred, target, m, nm):
    """-> sum m (p - y) in fp64 (every term >= 0 for an m of map_ref)"""
    p = np.asarray(pred, np.float64)
    B, C = p.shape[0], p.shape[-1]
    p = p.reshape(B, -1, C)[..., :nm]
    y = (np.asarray(target).reshape(B, -1, C)[..., :nm] > 0.5).astype(np.float64)
    t = np.asarray(m, np.float64).reshape(B, -1, nm) * (p - y)
    return float(t.sum()), float(np.abs(t).sum())


def loss_bound(B, HW, nm, want, abs_sum):
    """the rounding bound of mmseg_lovasz_loss as written: fp64 throughout, one rounding to fp32 at the end.
       stage 1: a thread takes ceil(ceil(HW / 128) / 256) pixels of its chunk, per element one subtraction, one product and one addition
                (3 roundings, or 2 when the compiler fuses); a 6-level butterfly over the wave, then 3 additions over the 4 wave sums;
       stage 2: a thread adds ceil(128 B / 256) partials, the same 6 + 3 levels; then (float).
       Every element passes through at most that many fp64 roundings, each relative to a partial sum bounded by sum |m (p - y)|."""
    per = -(-HW // CHUNKS)
    seq1 = -(-per // 256) * nm * 3
    seq2 = -(-(B * CHUNKS) // 256)
    return (seq1 + 9 + seq2 + 9) * 2.0 ** -53 * abs_sum + 2.0 ** -24 * abs(want) * (1 + 2.0 ** -20)


def grad_scale_f32(scale_host, scale_dev, weight):
    """s of mmseg_lovasz_grad_add in its documented order, every step rounded to fp32"""
    s = np.float32(scale_host)
    if scale_dev is not None:
        s = np.float32(s * np.float32(scale_dev))
    return np.float32(s * np.float32(weight))


def grad_add_f32(m, dpred, nm, scale_host, scale_dev, weight):
    out = np.array(dpred, np.float32, copy=True)
    s = grad_scale_f32(scale_host, scale_dev, weight)
    out[..., :nm] = out[..., :nm] + (s * np.asarray(m, np.float32).reshape(out[..., :nm].shape)).astype(np.float32)
    return out


# ---- contents ---------------------------------------------------------------------------------------------------------------------------
def pred_content(kind, shape, rng):
    """fp32 [B,H,W,C]; only channels < nm matter"""
    B, H, W, C, nm = shape
    P = H * W
    if kind == 'uniform':
        p = rng.rand(B, P, C)
    elif kind == 'softmax_like':                 # most pixels saturated, exact 0.0 and 1.0 among them
        x = rng.standard_normal((B, P, C)) * 40.0
        ex = np.exp((x - x.max(-1, keepdims=True)).astype(np.float32))
        p = ex / ex.sum(-1, keepdims=True)
    elif kind == 'constant':                     # the whole order is decided by the pixel index (and the label)
        p = np.full((B, P, C), 0.3)
    elif kind == 'quantised':                    # five values in runs longer than any tile, so ties cross every tile edge; labels mixed
        run = max(1, min(3 * TILE // 2, -(-P // 3)))
        p = np.broadcast_to((((np.arange(P) // run) % 5) * 0.25)[None, :, None], (B, P, C))
    elif kind == 'low_bits':                     # keys differ in the lowest digit only
        p = 0.5 + (rng.randint(0, 256, (B, P, C)) * 2.0 ** -24)
    elif kind == 'all_exponents':                # denormals to 1: every key digit varies
        bits = rng.randint(0, 0x3F800000 + 1, (B, P, C)).astype(np.uint32)
        p = bits.view(np.float32)
    else:
        raise ValueError(kind)
    return np.ascontiguousarray(np.asarray(p, np.float32).reshape(B, H, W, C))


def mask_content(kind, shape, rng):
    B, H, W, C, nm = shape
    P = H * W
    t = (rng.rand(B, P, C) > 0.6).astype(np.float32)
    if kind == 'edges':
        for b in range(B):
            for k in range(nm):
                v = (b * nm + k + b) % 4
                if v == 0:
                    t[b, :, k] = 0
                elif v == 1:
                    t[b, :, k] = 1
                elif v == 2:
                    t[b, :, k] = 0
                    t[b, rng.randint(P), k] = 1
        if B > 1:
            t[B - 1, :, :nm] = 0                 # a sample without any organ: K_b is empty under 'present'
    return t.reshape(B, H, W, C)


@functools.lru_cache(maxsize=None)
def case(shape, pkind, mkind, classes_all=False):
    """-> dict(pred, target fp32 [B,H,W,C]) + map_ref(...); computed once and shared (read-only)"""
    B, H, W, C, nm = shape
    rng = np.random.RandomState(2000 + PRED_KINDS.index(pkind) * 97 + MASK_KINDS.index(mkind) * 13 + (H * 31 + W * 7 + C + nm) % 89)
    pred, target = pred_content(pkind, shape, rng), mask_content(mkind, shape, rng)
    out = dict(pred=pred, target=target)
    out.update(map_ref(pred, target, nm, classes_all))
    out['m32'] = out['m'].astype(np.float32)
    for v in out.values():
        v.setflags(write=False)
    return out


# ---- torch-CPU stand-ins of the entry points (same argument lists, tensors instead of pointers) ----------------------------------------
def _map_ok(B, HW, nm):
    return 1 <= B <= 65535 and 1 <= HW <= MAXHW and 1 <= nm <= MAXC


def lovasz_workspace_bytes(B, HW, nm):
    if not _map_ok(B, HW, nm):
        return 0
    S, nblk = B * nm, -(-HW // TILE)
    return 2 * S * HW * 8 + S * nblk * 256 * 4 + S * nblk * 4


def lovasz_map(pred, target, m, ws, B, HW, C, nm, classes_all):
    if pred is None or target is None or m is None or ws is None or not _map_ok(B, HW, nm) or nm > C or C > MAXC:
        return 1
    r = map_ref(pred.detach().reshape(B, HW, C).numpy(), target.reshape(B, HW, C).numpy(), nm, bool(classes_all))
    m.copy_(torch.from_numpy(r['m'].astype(np.float32)).reshape(m.shape)); return 0


def lovasz_loss_workspace_floats(B):
    return 2 * B * CHUNKS if 1 <= B <= 65535 else 0


def lovasz_loss(pred, target, m, loss_l, ws, B, HW, C, nm):
    if pred is None or target is None or m is None or loss_l is None or ws is None or B < 1 or B > 65535 or HW < 1 or nm < 1 or nm > C or C > MAXC:
        return 1
    y = (target.reshape(B, HW, C)[..., :nm] > 0.5).double()
    v = (m.reshape(B, HW, nm).double() * (pred.detach().reshape(B, HW, C)[..., :nm].double() - y)).sum()
    loss_l.copy_(v.float().reshape(1)); return 0


def lovasz_grad_add(m, dpred, B, HW, C, nm, scale_host, scale_dev, weight_dev):
    if m is None or dpred is None or weight_dev is None or B < 1 or HW < 1 or nm < 1 or nm > C or C > MAXC:
        return 1
    s = torch.tensor(scale_host, dtype=torch.float32)
    if scale_dev is not None:
        s = s * scale_dev[0]
    s = s * weight_dev[0]
    d = dpred.reshape(B, HW, C)
    d[..., :nm] += s * m.reshape(B, HW, nm)
    return 0


STANDINS = {'mmseg_' + f.__name__: f for f in (lovasz_workspace_bytes, lovasz_map, lovasz_loss_workspace_floats, lovasz_loss, lovasz_grad_add)}
