"""Synchronised BatchNorm's split kernels (csrc/norm.hip: mmseg_bn_stats_local / _stats_combine / _bwd_sums / _bwd_finish / _bwd_apply,
the `ctx.sync` branches of ops._BatchNormTrain) with SEVERAL shards on one device, against fp64 torch on the concatenated batch.

The collectives of the data-parallel step are a concatenation (all-gather of the [2][C] statistics) and a sum (all-reduce of the [2][C]
backward sums), so `_sync_bn_by_hand` plays R ranks by doing both by hand between the kernel calls.  tests/test_dp_rccl.py runs these
kernels with one rank (the combine adds one term and divides by 1, local == global), tests/test_dp_gloo.py runs several ranks on the
torch stand-ins; here R = 2, 3, 8 meet the kernels themselves, at the launch edges tests/test_ops_parity.py::BN_EDGES pins for the
fused path.  Every case runs on the device (`-m gpu`) and through tests/cpu_backend.py.

Launch arithmetic (recomputed from csrc/norm.hip; M = rows of ONE shard):
  generic partial kernel (C % 64 != 0): min(1024, ceil(M / 512)) row blocks of ceil(M / blocks) rows, 256 threads = cw = min(C, 256)
      columns x rl = 256 / cw row lanes, column passes of cw;
  float4 partial kernel (C % 64 == 0): min(512, 1024 / (C / 64), ceil(M / 64)) row blocks x C / 64 column blocks, 16 row lanes;
  the "final" kernels (stats_local_final, bwd_sums_final): ceil(C / 64) blocks, 16 lanes per channel over the row blocks;
  combine / finish: ceil(C / 256) blocks of 256 threads, one channel per thread;
  bn_apply / bn_bwd_apply: min(4096, ceil(M * C / 4 / 256)) blocks of 256 float4 lanes, grid-stride above 1 048 576 float4.

Tolerances.  y, dx and the gradients: 5e-4 of the tensor's largest magnitude, as the fused BatchNorm tests.  The per-channel statistics,
the per-rank sums and the dx coefficients: TIGHT = 1e-5 -- a wrong M_total in the unbiased factor moves the moving variance by only
1 / (M_total - 1) (3.8e-4 at 2622 rows, 3e-5 at 32770), so the fused tests' 2e-4 would let it pass.  The longest fp32 addition chain
of these shapes (rows per lane, row lanes, nblk / 16, the 16 lanes of reduce_partials_64, R) has under 100 roundings of 2^-24, about
6e-6 of the sum of magnitudes (C = 300 excepted: one row lane, 437 rows per chain).  `test_fp32_emulation_...` below repeats the
kernels' shifted two-stage sums in fp32 torch (no kernel involved) and holds every quantity of every case to a third of its bound;
the quantities that fp32 itself cannot hold to 1e-5 / 3 on the special inputs are listed in EMULATION_WORST with their figures.
"""
import functools
import types

import pytest
import torch

from oracle import ops as O
from multimodal_segmentation_amd import _native as N
from multimodal_segmentation_amd import ops as P
from multimodal_segmentation_amd.ops import BN_EPS, BN_MOMENTUM
from multimodal_segmentation_amd.parallel import dp
from tests.test_ops_parity import RTOL, _anchor, _close, _native_error, device, gbuf_pattern, rnd  # noqa: F401 (device: fixture)

# Bound of the per-channel statistics, per-rank sums and dx coefficients (see the module docstring): error / largest magnitude of the
# reference tensor.  The fp32 emulation stays within a third of it (worst: 2.9e-6, unb_var of (1311, 300, 2); the kernels on the MI355X
# measure 3.0e-6 there, stat2_var), except where fp32 itself cannot.  There the bound is 3 x the emulation's worst figure (the table's
# value; the kernels measure the same figures to two digits), for that quantity of that input only:
#   C300: rl = 256 / 256 = 1 row lane, so a lane chains all 437 rows of its block (not the < 100 additions of the other shapes);
#   common-mean: mean ~ 50 is known to half an fp32 ulp (1.9e-6), 4e-6 of the standard deviation 0.5; xhat carries it into sum g * xhat;
#   opposite-means-R2: the global mean of shards at +50 and -50 is ~ 0.02, the two rounded shard means leave up to 3.8e-6 of error in it;
#   constant-shard: shard 0 has xhat = (3 - mean) * invstd with mean ~ 3.0 +- 0.03, a cancellation of 100 in front of sum g.
TIGHT = 1e-5
EMULATION_WORST = {('C300', 'stat2_var'): 5.6e-6,
                   ('common-mean', 'sums_gxhat'): 6.8e-6, ('common-mean', 'coef_B'): 6.1e-6, ('common-mean', 'coef_C'): 6.1e-6,
                   ('opposite-means-R2', 'mean'): 9.1e-5, ('opposite-means-R2', 'unb_mean'): 9.1e-5,
                   ('constant-shard', 'sums_gxhat'): 9.5e-6}
LOOSE = 5e-4
SENTINEL = -777.0


def _bound(label, name):
    return 3 * EMULATION_WORST[(label, name)] if (label, name) in EMULATION_WORST else TIGHT


def _measure(a, b, name, rtol):
    """_close, after printing the figure it judges (error / largest reference magnitude), so that a run with `-s` records it"""
    a64, b64 = a.detach().cpu().double(), b.detach().cpu().double()
    scale = max(b64.abs().max().item(), 1e-6)
    print('sync-bn figure %-11s %.3e (bound %.1e)' % (name, (a64 - b64).abs().max().item() / scale, rtol))
    _close(a, b, name, rtol)


# ======================================================================================================================
# inputs and the fp64 reference on the concatenated batch (computed once per case, never written to)
# ======================================================================================================================
def _inputs(M, C, R, kind):
    Mt = R * M
    z = rnd(Mt, C, seed=5)
    if kind == 'normal':
        X = z * 2 + 3.0                                   # non-zero mean: exercises the shifted sums
    elif kind == 'common-mean':
        X = z * 0.5 + 50.0                                # mean_r - mean is rounding noise: the local shifted sums carry the variance
    elif kind == 'opposite-means':
        sign = torch.tensor([(-1.0) ** r for r in range(R)]).repeat_interleave(M).reshape(Mt, 1)
        X = z * 0.5 + 50.0 * sign                         # (mean_r - mean)^2 is 10^4 times the local variance
    elif kind == 'constant-shard':
        X = z * 2 + 3.0
        X[:M] = 3.0                                       # shard 0: local variance exactly 0
    else:
        raise ValueError(kind)
    return X.contiguous()


@functools.lru_cache(maxsize=2)
def _case(M, C, R, relu, kind='normal'):
    """fp32 CPU inputs of R shards of [M, C] and the fp64 reference of one training step of BatchNorm (+ReLU) on the [R * M, C] batch"""
    Mt = R * M
    X = _inputs(M, C, R, kind)
    gamma, beta = rnd(C, seed=6) * 0.2 + 1, rnd(C, seed=7) * 0.2
    mm0, mv0 = rnd(C, seed=8) * 0.1, torch.rand(C, generator=torch.Generator().manual_seed(9)) + 0.5
    x64 = X.double().reshape(1, 1, Mt, C).requires_grad_(True)
    g64, b64 = gamma.double().requires_grad_(True), beta.double().requires_grad_(True)
    Pd = {'n/gamma': g64, 'n/beta': b64, 'n/moving_mean': mm0.double(), 'n/moving_variance': mv0.double()}
    upd = []
    pre = O.batchnorm(x64, Pd, 'n', True, upd)
    O.apply_bn_updates(Pd, upd)
    y = torch.relu(pre) if relu else pre
    # no cotangent where the ReLU kink could flip between fp32 and fp64 (as test_ops_parity.check)
    cot = rnd(Mt, C, seed=11) * (pre.detach().reshape(Mt, C).abs() > 1e-4).float()
    y.backward(cot.double().reshape(y.shape))
    with torch.no_grad():
        Xd = X.double()
        mean, var = Xd.mean(0), Xd.var(0, unbiased=False)
        invstd = torch.rsqrt(var + BN_EPS)
        scale = gamma.double() * invstd
        g = cot.double() * (pre.reshape(Mt, C) > 0) if relu else cot.double()
        xhat = (Xd - mean) * invstd
        rows = [slice(r * M, (r + 1) * M) for r in range(R)]
        sums = [torch.stack([g[s].sum(0), (g[s] * xhat[s]).sum(0)]) for s in rows]        # (dbeta_r, dgamma_r)
        glob = torch.stack(sums).sum(0)
        # the per-rank gradients add up to autograd's gradients of the global batch
        _close(glob[0], b64.grad, 'sum of per-rank dbeta', 1e-12)
        _close(glob[1], g64.grad, 'sum of per-rank dgamma', 1e-12)
        A = scale
        Bc = -gamma.double() * invstd * invstd * glob[1] / Mt
        ref = {'mean': mean, 'invstd': invstd, 'scale': scale, 'shift': beta.double() - mean * scale,
               'mov_mean': Pd['n/moving_mean'].detach(), 'mov_var': Pd['n/moving_variance'].detach(),
               'unb_mean': mean, 'unb_var': var * (Mt / max(Mt - 1, 1)),
               'stat2': [torch.stack([Xd[s].mean(0), Xd[s].var(0, unbiased=False)]) for s in rows],
               'y': y.detach().reshape(Mt, C), 'sums': sums, 'coef': torch.stack([A, Bc, -A * glob[0] / Mt - Bc * mean]),
               'dx': x64.grad.reshape(Mt, C)}
    label = 'C300' if C == 300 else kind + ('-R2' if (kind, R) == ('opposite-means', 2) else '')
    return types.SimpleNamespace(M=M, C=C, R=R, relu=relu, label=label, xs=[X[s].contiguous() for s in rows], dys=[cot[s].contiguous() for s in rows],
                                 gamma=gamma, beta=beta, mm0=mm0, mv0=mv0, ref=ref)


def _compare(got, case, frac=1.0):
    ref, tight = case.ref, lambda name: _bound(case.label, name) * frac
    for k in ('mean', 'invstd', 'scale', 'shift', 'mov_mean', 'mov_var', 'unb_mean', 'unb_var'):
        _measure(got[k], ref[k], k, tight(k))
    for a, b in zip(got['stat2'], ref['stat2']):
        _measure(a[0], b[0], 'stat2_mean', tight('stat2_mean'))
        _measure(a[1], b[1], 'stat2_var', tight('stat2_var'))
    for a, b in zip(got['sums'], ref['sums']):
        _measure(a[0], b[0], 'sums_g', tight('sums_g'))
        _measure(a[1], b[1], 'sums_gxhat', tight('sums_gxhat'))
    for i, name in enumerate(('coef_A', 'coef_B', 'coef_C')):
        _measure(got['coef'][i], ref['coef'][i], name, tight(name))
    if 'y' in got:
        _measure(torch.cat(got['y']), ref['y'], 'y', LOOSE)
        _measure(torch.cat(got['dx']), ref['dx'], 'dx', LOOSE)


# ======================================================================================================================
# 1. R ranks on one device
# ======================================================================================================================
def _workspace(C, dev):
    return torch.empty(max(int(N.call('mmseg_norm_workspace_floats', C)), 1), device=dev)


def _sync_bn_by_hand(shards_x, shards_dy, gamma, beta, mov_mean, mov_var, relu, accumulate, train_affine):
    """The kernel sequence of ops._BatchNormTrain's sync branches for every rank, with the all-gather done as a concatenation and the
    all-reduce as a torch sum, both in rank order.  `mov_mean` / `mov_var` are updated in place (one update: every rank's copy is the
    same, which the repeated combine asserts).  Gradient buffers: gbuf_pattern (accumulate), SENTINEL (overwrite), none (frozen)."""
    dev, R = shards_x[0].device, len(shards_x)
    M, C = shards_x[0].shape
    ws = _workspace(C, dev)

    def new(*shape):
        return torch.empty(*shape, device=dev)

    stat2 = []
    for x in shards_x:
        stat2.append(new(2, C))
        N.call('mmseg_bn_stats_local', x, stat2[-1], ws, M, C)
    gathered = torch.cat([s.reshape(-1) for s in stat2])                      # the all-gather: [R][2][C]

    def combine(mm, mv, momentum=BN_MOMENTUM):
        st = new(4, C)       # mean, invstd, scale, shift
        N.call('mmseg_bn_stats_combine', gathered, R, gamma, beta, st[0], st[1], st[2], st[3], mm, mv, M * R, C, BN_EPS, momentum)
        return st
    mm2, mv2, mm3, mv3 = mov_mean.clone(), mov_var.clone(), mov_mean.clone(), mov_var.clone()
    stats = combine(mov_mean, mov_var)
    again = combine(mm2, mv2)                                                 # what another rank computes from the same gathered rows
    assert torch.equal(stats, again) and torch.equal(mm2, mov_mean) and torch.equal(mv2, mov_var)
    # momentum 0 lays the UNBIASED global variance bare (mov - (mov - unb) * 1): in the real update its M_total / (M_total - 1) is
    # damped by 1 - momentum = 0.01, which would hide a wrong M_total at 2622 rows behind the bound
    assert torch.equal(combine(mm3, mv3, 0.0), stats)

    ys, sums = [], []
    for x in shards_x:
        ys.append(new(M, C))
        N.call('mmseg_bn_apply', x, stats[2], stats[3], ys[-1], M, C, int(relu))
    for x, dy, y in zip(shards_x, shards_dy, ys):
        sums.append(new(2, C))
        N.call('mmseg_bn_bwd_sums', dy, y if relu else None, x, stats[0], stats[1], sums[-1], ws, M, C, int(relu))
    glob = sums[0].clone()
    for s in sums[1:]:
        glob = glob + s                                                       # the all-reduce
    dgammas, dbetas, coefs, dxs = [], [], [], []
    for x, dy, y, s in zip(shards_x, shards_dy, ys, sums):
        if train_affine:
            fill = gbuf_pattern(gamma) if accumulate else torch.full(gamma.shape, SENTINEL)
            dgammas.append(fill.clone().to(dev))
            dbetas.append(fill.clone().to(dev))
        coefs.append(new(3 * C))
        N.call('mmseg_bn_bwd_finish', s, glob, gamma, stats[0], stats[1], dgammas[-1] if train_affine else None,
               dbetas[-1] if train_affine else None, coefs[-1], C, M * R, int(accumulate))
        dxs.append(new(M, C))
        N.call('mmseg_bn_bwd_apply', dy, y if relu else None, x, coefs[-1], dxs[-1], M, C, int(relu))
    for c in coefs[1:]:
        assert torch.equal(c, coefs[0]), 'the dx coefficients depend on the global sums only'
    return {'mean': stats[0], 'invstd': stats[1], 'scale': stats[2], 'shift': stats[3], 'mov_mean': mov_mean, 'mov_var': mov_var,
            'unb_mean': mm3, 'unb_var': mv3,
            'stat2': stat2, 'y': ys, 'sums': sums, 'glob': glob, 'dgamma': dgammas, 'dbeta': dbetas, 'coef': coefs[0].reshape(3, C), 'dx': dxs}


def _by_hand(case, dev, accumulate=1, train_affine=True):
    to = lambda t: t.clone().to(dev)
    return _sync_bn_by_hand([to(x) for x in case.xs], [to(d) for d in case.dys], to(case.gamma), to(case.beta), to(case.mm0), to(case.mv0),
                            case.relu, accumulate, train_affine)


def _check_by_hand(case, dev):
    """the three gradient-buffer modes of mmseg_bn_bwd_finish; the statistics, sums, coefficients, y and dx are compared in the first"""
    got = _by_hand(case, dev, 1, True)
    _compare(got, case)
    fill = gbuf_pattern(case.gamma).double()
    for r in range(case.R):                                                   # added to what the buffer held
        _measure(got['dgamma'][r].cpu().double() - fill, case.ref['sums'][r][1], 'dgamma_r', LOOSE)
        _measure(got['dbeta'][r].cpu().double() - fill, case.ref['sums'][r][0], 'dbeta_r', LOOSE)
    over = _by_hand(case, dev, 0, True)
    for r in range(case.R):                                                   # the sentinel is overwritten by THIS rank's sums, bit for bit
        assert torch.equal(over['dbeta'][r], over['sums'][r][0]) and torch.equal(over['dgamma'][r], over['sums'][r][1])
        _measure(over['dgamma'][r], case.ref['sums'][r][1], 'dgamma_r', LOOSE)
        _measure(over['dbeta'][r], case.ref['sums'][r][0], 'dbeta_r', LOOSE)
    frozen = _by_hand(case, dev, 0, False)
    for k in ('coef', 'glob'):
        assert torch.equal(over[k], got[k]) and torch.equal(frozen[k], got[k]), k
    for r in range(case.R):
        assert torch.equal(over['dx'][r], got['dx'][r]) and torch.equal(frozen['dx'][r], got['dx'][r])
    return got


# ======================================================================================================================
# 2. shapes: the smallest that reach each edge.  M (rows of one shard), C, R
# ======================================================================================================================
SHAPES = [
    # generic kernel (C % 64 != 0).  M = 1311: 3 row blocks of exactly 437 rows
    pytest.param(1311, 20, 2, id='generic-C20-rl12-16-idle-threads'),           # cw = 20, rl = 12: threads 240..255 idle
    pytest.param(1312, 20, 3, id='generic-M1312-short-last-block'),             # rows_per_block = 438, the last block holds 436
    pytest.param(1311, 8, 2, id='generic-C8-rl32'),
    # second column pass of 44 columns; final kernels: 5 blocks, the last with 44 live channels; combine / finish: 2 blocks, 44 live threads
    pytest.param(1311, 300, 2, id='generic-C300-two-column-passes'),
    # float4 kernel (C % 64 == 0)
    pytest.param(1311, 64, 2, id='v4-M1311-21-blocks-of-63-last-51'),
    pytest.param(9, 64, 3, id='v4-M9-fewer-rows-than-lanes'),
    # one row per shard: every local variance is exactly 0, the batch variance is all (mean_r - mean)^2; R = 2: M_total = 2, unbiased factor 2
    pytest.param(1, 64, 2, id='v4-M1-R2-variance-between-shards-only'),
    pytest.param(1, 64, 8, id='v4-M1-R8-variance-between-shards-only'),
    pytest.param(512, 192, 2, id='v4-C192-three-column-blocks'),
    pytest.param(64, 512, 2, id='v4-C512-combine-finish-two-full-blocks'),
]
# M = 16385: min(512, 1024 / 4, 257) = 256 row blocks of 65 rows: blocks 0..251 full, block 252 holds 5 rows, blocks 253..255 are EMPTY and
# write zero partials that the sync final kernels sum; n4 = 1 048 640 wraps bn_apply / bn_bwd_apply by 64.  34 MB per tensor: ReLU on only
BIG = pytest.param(16385, 256, 2, id='v4-M16385-rpb65-three-empty-row-blocks-apply-wraps')


def _with_relu(shapes, big):
    out = [pytest.param(*p.values, relu, id='%s-%s' % (p.id, 'relu' if relu else 'linear')) for p in shapes for relu in (True, False)]
    return out + [pytest.param(*big.values, True, id=big.id + '-relu')]


@pytest.mark.parametrize('M,C,R,relu', _with_relu(SHAPES, BIG))
def test_sync_batchnorm_kernels_with_several_shards(M, C, R, relu, device):
    case = _case(M, C, R, relu)
    got = _check_by_hand(case, device)
    if M == 1:
        for s in got['stat2']:
            assert torch.equal(s[1], torch.zeros_like(s[1])), 'the variance of one row is exactly 0'


# ======================================================================================================================
# 3. inputs where the combine can lose the variance
# ======================================================================================================================
@pytest.mark.parametrize('C', [64, 20], ids=['v4', 'generic'])
@pytest.mark.parametrize('kind,R', [('common-mean', 2), ('opposite-means', 2), ('opposite-means', 3), ('constant-shard', 3)])
def test_sync_batchnorm_combine_keeps_the_variance(kind, R, C, device):
    case = _case(1311, C, R, True, kind)
    got = _check_by_hand(case, device)
    if kind == 'constant-shard':
        # x - x[0][c] is exactly 0 in every row: both shifted sums are 0.0 before the clamp is reached
        assert torch.equal(got['stat2'][0][1], torch.zeros_like(got['stat2'][0][1]))
        assert torch.equal(got['stat2'][0][0], torch.full_like(got['stat2'][0][0], 3.0))


# ======================================================================================================================
# the bound itself: an fp32 torch emulation of the kernels' shifted two-stage sums against the fp64 reference (no kernel involved)
# ======================================================================================================================
def _chain(t):
    """left-to-right fp32 sum over the first dimension"""
    acc = torch.zeros_like(t[0])
    for k in range(t.shape[0]):
        acc = acc + t[k]
    return acc


def _two_stage_sum(v):
    """column sums of v [M, C] in the kernels' order: per row block and row lane a chain over the lane's rows, a chain over the lanes,
    then reduce_partials_64: lane l chains the blocks l, l + 16, ..., and a chain over the 16 lanes"""
    M, C = v.shape
    if C % 64 == 0:
        nb, lanes = max(1, min(512, 1024 // (C // 64), (M + 63) // 64)), 16
    else:
        nb, lanes = max(1, min(1024, (M + 511) // 512)), 256 // min(C, 256)
    rpb = -(-M // nb)
    nj = -(-rpb // lanes)
    buf = torch.zeros(nb * rpb, C)
    buf[:M] = v
    buf = torch.cat([buf.reshape(nb, rpb, C), torch.zeros(nb, nj * lanes - rpb, C)], 1).reshape(nb, nj, lanes, C)
    part = _chain(_chain(buf.permute(1, 2, 0, 3)))                            # [nb, C]
    nl = -(-nb // 16)
    return _chain(_chain(torch.cat([part, torch.zeros(nl * 16 - nb, C)]).reshape(nl, 16, C)))


def _emulate(case):
    M, C, R = case.M, case.C, case.R
    invM, one_m = 1.0 / M, 1.0 - BN_MOMENTUM
    stat2 = []
    for x in case.xs:
        d = x - x[0]
        dd = _two_stage_sum(d) * invM
        stat2.append(torch.stack([x[0] + dd, (_two_stage_sum(d * d) * invM - dd * dd).clamp_min(0.0)]))
    mu = _chain(torch.stack([s[0] for s in stat2])) / R
    var = _chain(torch.stack([s[1] + (s[0] - mu) * (s[0] - mu) for s in stat2])) / R
    invstd = torch.rsqrt(var + BN_EPS)
    scale = case.gamma * invstd
    shift = case.beta - mu * scale
    Mt = M * R
    unb = var * (Mt / (Mt - 1.0)) if Mt > 1 else var
    sums = []
    for x, dy in zip(case.xs, case.dys):
        g = dy * (torch.addcmul(shift, x, scale) > 0) if case.relu else dy
        sums.append(torch.stack([_two_stage_sum(g), _two_stage_sum(g * (x - mu) * invstd)]))
    glob = _chain(torch.stack(sums))
    A = scale
    Bc = -case.gamma * invstd * invstd * glob[1] * (1.0 / Mt)
    out = {'mean': mu, 'invstd': invstd, 'scale': scale, 'shift': shift, 'mov_mean': case.mm0 - (case.mm0 - mu) * one_m,
           'mov_var': case.mv0 - (case.mv0 - unb) * one_m, 'unb_mean': case.mm0 - (case.mm0 - mu), 'unb_var': case.mv0 - (case.mv0 - unb),
           'stat2': stat2, 'sums': sums,
           'coef': torch.stack([A, Bc, -A * glob[0] * (1.0 / Mt) - Bc * mu])}
    assert all(t.dtype == torch.float32 for t in (mu, invstd, shift, glob, out['coef'], out['mov_var']))
    return out


SPECIAL = [pytest.param(1311, C, R, True, kind, id='%s-R%d-C%d' % (kind, R, C)) for C in (64, 20)
           for kind, R in (('common-mean', 2), ('opposite-means', 2), ('opposite-means', 3), ('constant-shard', 3))]


@pytest.mark.parametrize('M,C,R,relu,kind', [pytest.param(*p.values, 'normal', id=p.id) for p in _with_relu(SHAPES, BIG)] + SPECIAL)
def test_fp32_emulation_of_the_two_stage_sums_stays_within_a_third_of_the_bound(M, C, R, relu, kind):
    case = _case(M, C, R, relu, kind)
    _compare(_emulate(case), case, 1.0 / 3)


# ======================================================================================================================
# 4. R = 1 must be the fused path, bit for bit
# ======================================================================================================================
def _same(a, b, name, dev):
    if dev == 'cuda':
        assert torch.equal(a, b), '%s: %d elements differ' % (name, (a != b).sum().item())
    else:                 # the stand-ins of the fused and of the split entry points are not written to be bit-equal
        _close(a, b, name, 1e-6)


ONE_SHARD = [pytest.param(*p.values[:2], 1, id=p.id) for p in SHAPES if p.values != (1, 64, 8)]      # (1, 64) once


@pytest.mark.parametrize('M,C,R,relu', _with_relu(ONE_SHARD, pytest.param(*BIG.values[:2], 1, id=BIG.id)))
def test_sync_batchnorm_kernels_with_one_shard_are_the_fused_kernels_bit_for_bit(M, C, R, relu, device):
    """mmseg_bn_stats_local + combine == mmseg_bn_stats, mmseg_bn_bwd_sums + finish + bwd_apply == mmseg_bn_bwd (saved output) ==
    mmseg_bn_bwd_x (mask recomputed from x: bn_apply_kernel's own fused multiply-add, the same bits).  bn_bwd_finish_kernel and
    bn_bwd_final_kernel compile `-A * s1 * invM - Bc * mu` to the same fused multiply-add, so coef and dx are compared bitwise too."""
    case = _case(M, C, 1, relu)
    to = lambda t: t.clone().to(device)
    x, dy, gamma, beta = to(case.xs[0]), to(case.dys[0]), to(case.gamma), to(case.beta)
    ws = _workspace(C, device)
    st, mm, mv = torch.empty(4, C, device=device), to(case.mm0), to(case.mv0)
    N.call('mmseg_bn_stats', x, gamma, beta, st[0], st[1], st[2], st[3], mm, mv, ws, M, C, BN_EPS, BN_MOMENTUM)
    y = torch.empty(M, C, device=device)
    N.call('mmseg_bn_apply', x, st[2], st[3], y, M, C, int(relu))
    for accumulate in (0, 1):
        got = _by_hand(case, device, accumulate, True)
        for i, k in enumerate(('mean', 'invstd', 'scale', 'shift')):
            _same(got[k], st[i], k, device)
        _same(got['mov_mean'], mm, 'mov_mean', device)
        _same(got['mov_var'], mv, 'mov_var', device)
        _same(got['y'][0], y, 'y', device)
        assert torch.equal(got['glob'], got['sums'][0])
        for saved in (True, False):
            fill = gbuf_pattern(case.gamma) if accumulate else torch.full((C,), SENTINEL)
            dx, dg, db, coef = torch.empty(M, C, device=device), to(fill), to(fill), torch.empty(3 * C, device=device)
            if saved:
                N.call('mmseg_bn_bwd', dy, y if relu else None, x, gamma, st[0], st[1], dx, dg, db, coef, ws, M, C, int(relu), accumulate)
            else:
                N.call('mmseg_bn_bwd_x', dy, x, st[2], st[3], gamma, st[0], st[1], dx, dg, db, coef, ws, M, C, int(relu), accumulate)
            tag = ' (saved y)' if saved else ' (mask from x)'
            _same(got['dgamma'][0], dg, 'dgamma' + tag, device)
            _same(got['dbeta'][0], db, 'dbeta' + tag, device)
            if not accumulate:
                _same(got['sums'][0], torch.stack([db, dg]), 'sums' + tag, device)
            _same(got['coef'], coef.reshape(3, C), 'coef' + tag, device)
            _same(got['dx'][0], dx, 'dx' + tag, device)


# ======================================================================================================================
# 5. the op-level sync branch on one device, with a fake parallel.dp
# ======================================================================================================================
class _FakeRanks(object):
    """parallel.dp's collectives for rank `self.rank` of R: the other ranks' contributions are computed here, with the same kernels on
    the other shards and a workspace of its own, and merged in rank order"""

    def __init__(self, case, dev):
        to = lambda t: t.clone().to(dev)
        self.case, self.dev, self.rank = case, dev, 0
        self.xs, self.dys = [to(x) for x in case.xs], [to(d) for d in case.dys]
        self.gamma, self.beta = to(case.gamma), to(case.beta)
        self.ys = [None] * case.R                  # the saved outputs, filled in by the forward passes
        self.ws = _workspace(case.C, dev)
        self.gathered = None

    def install(self, m):
        m.setattr(dp, 'sync_bn', lambda: True)
        m.setattr(dp, 'world_size', lambda: self.case.R)
        m.setattr(dp, 'all_gather_rows', self.all_gather_rows)
        m.setattr(dp, 'all_reduce_sum', self.all_reduce_sum)

    def all_gather_rows(self, local):
        M, C, R = self.case.M, self.case.C, self.case.R
        out = torch.empty(R, 2 * C, device=self.dev)
        for r in range(R):
            if r == self.rank:
                out[r] = local
            else:
                s = torch.empty(2, C, device=self.dev)
                N.call('mmseg_bn_stats_local', self.xs[r], s, self.ws, M, C)
                out[r] = s.reshape(-1)
        self.gathered = out
        return out

    def all_reduce_sum(self, t):
        M, C, R, relu = self.case.M, self.case.C, self.case.R, self.case.relu
        st = torch.empty(4, C, device=self.dev)    # the shared statistics: the combine is bit-identical on every rank
        N.call('mmseg_bn_stats_combine', self.gathered.reshape(-1), R, self.gamma, self.beta, st[0], st[1], st[2], st[3], None, None,
               M * R, C, BN_EPS, BN_MOMENTUM)
        total = None
        for r in range(R):
            if r == self.rank:
                s = t
            else:
                s = torch.empty(2, C, device=self.dev)
                N.call('mmseg_bn_bwd_sums', self.dys[r], self.ys[r] if relu else None, self.xs[r], st[0], st[1], s, self.ws, M, C, int(relu))
            total = s.clone() if total is None else total + s.reshape(total.shape)
        return total.reshape(t.shape).contiguous()


@pytest.mark.parametrize('trained', [True, False], ids=['trained', 'frozen'])
@pytest.mark.parametrize('relu', [True, False], ids=['relu', 'linear'])
@pytest.mark.parametrize('M,C,R', [pytest.param(1311, 64, 2, id='v4-M1311-R2'), pytest.param(1312, 20, 3, id='generic-M1312-R3')])
def test_batchnorm_op_sync_branch_with_several_ranks(M, C, R, relu, trained, device, monkeypatch):
    case = _case(M, C, R, relu)
    to = lambda t: t.clone().to(device)
    fake = _FakeRanks(case, device)
    mms, mvs = [to(case.mm0) for _ in range(R)], [to(case.mv0) for _ in range(R)]
    ggs = [to(gbuf_pattern(case.gamma)) if trained else None for _ in range(R)]
    bgs = [to(gbuf_pattern(case.beta)) if trained else None for _ in range(R)]
    xs = [x.clone().requires_grad_(True) for x in fake.xs]
    with monkeypatch.context() as m:
        fake.install(m)
        ys = []
        for r in range(R):                         # every rank's forward pass first: the backward passes need every saved output
            fake.rank = r
            ys.append(P.batchnorm(xs[r], fake.gamma, fake.beta, mms[r], mvs[r], True, relu, ggrad=ggs[r], bgrad=bgs[r], anchor=_anchor(xs[r])))
            fake.ys[r] = ys[r].detach()
        for r in range(R):
            fake.rank = r
            ys[r].backward(fake.dys[r])
    for r in range(1, R):                          # every rank ends with the same moving statistics
        assert torch.equal(mms[r], mms[0]) and torch.equal(mvs[r], mvs[0])
    ref = case.ref
    _measure(mms[0], ref['mov_mean'], 'mov_mean', TIGHT)
    _measure(mvs[0], ref['mov_var'], 'mov_var', TIGHT)
    _measure(torch.cat(fake.ys), ref['y'], 'y', LOOSE)
    _measure(torch.cat([x.grad for x in xs]), ref['dx'], 'dx', LOOSE)
    hand = _by_hand(case, device, 1, trained)
    assert torch.equal(mms[0], hand['mov_mean']) and torch.equal(mvs[0], hand['mov_var'])
    for r in range(R):
        assert torch.equal(fake.ys[r], hand['y'][r]), 'y of rank %d' % r
        assert torch.equal(xs[r].grad, hand['dx'][r]), 'dx of rank %d' % r
        if trained:
            fill = gbuf_pattern(case.gamma).double()
            _measure(ggs[r].cpu().double() - fill, ref['sums'][r][1], 'dgamma_r', LOOSE)
            _measure(bgs[r].cpu().double() - fill, ref['sums'][r][0], 'dbeta_r', LOOSE)
            assert torch.equal(ggs[r], hand['dgamma'][r]) and torch.equal(bgs[r], hand['dbeta'][r]), 'gradients of rank %d' % r


def test_batchnorm_op_sync_branch_refuses_16_bit_storage(device, monkeypatch):
    """out_dtype = bfloat16 under sync_bn: the branch's AssertionError, before any kernel has run"""
    case = _case(1311, 64, 2, True)
    fake = _FakeRanks(case, device)
    launched = []
    with monkeypatch.context() as m:
        fake.install(m)
        inner = N.call
        m.setattr(N, 'call', lambda name, *a: (launched.append(name), inner(name, *a))[1])
        with pytest.raises(AssertionError, match='sync_bn'):
            P.batchnorm(fake.xs[0], fake.gamma, fake.beta, fake.gamma.clone(), fake.gamma.clone(), True, True, out_dtype=torch.bfloat16)
    assert [n for n in launched if n != 'mmseg_norm_workspace_floats'] == []


# ======================================================================================================================
# 6. refusals
# ======================================================================================================================
@pytest.mark.parametrize('entry', ['mmseg_bn_apply', 'mmseg_bn_bwd_apply'])
def test_bn_apply_kernels_refuse_channels_that_are_no_multiple_of_four(entry, device):
    """C = 6: the element-wise kernels move float4; refused before the launch, the output stays as it was"""
    M, C = 4, 6
    x, dy, v = rnd(M, C, seed=1).to(device), rnd(M, C, seed=2).to(device), rnd(3 * C, seed=3).to(device)
    out = torch.full((M, C), SENTINEL, device=device)
    with pytest.raises(_native_error()):
        if entry == 'mmseg_bn_apply':
            N.call(entry, x, v[:C].contiguous(), v[C:2 * C].contiguous(), out, M, C, 1)
        else:
            N.call(entry, dy, x, x, v, out, M, C, 1)
    assert torch.equal(out, torch.full_like(out, SENTINEL))


def test_bn_stats_combine_refuses_zero_ranks(device):
    C = 64
    gathered, gamma, beta = rnd(2 * C, seed=1).to(device), rnd(C, seed=2).to(device), rnd(C, seed=3).to(device)
    outs = [torch.full((C,), SENTINEL, device=device) for _ in range(6)]       # mean, invstd, scale, shift, moving mean, moving variance
    with pytest.raises(_native_error()):
        N.call('mmseg_bn_stats_combine', gathered, 0, gamma, beta, outs[0], outs[1], outs[2], outs[3], outs[4], outs[5], 0, C, BN_EPS, BN_MOMENTUM)
    for o in outs:
        assert torch.equal(o, torch.full_like(o, SENTINEL))
