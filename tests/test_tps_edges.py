"""The thin-plate-spline warp kernels (csrc/tps.hip) at their window, border, staging and batch-group edges.

Same conventions as tests/test_ops_parity.py: every case runs on the device (`-m gpu`) and through tests/cpu_backend.py.  The raw
entry points are called (mmseg_tps_warp_fwd with a loc buffer, mmseg_tps_warp_bwd with dvol / dtheta / dloc / ws / acc sized by the
two *_workspace_floats calls), and the comparison is SPLIT so that every stage is judged on the kernel's own inputs:

  1. loc     vs fp64 grid + Mb theta                      32 eps (1 + rowsum max|theta|) (max(H, W) - 1)  pixels
  2. out     vs fp64 resampler at the KERNEL's loc        16 eps sum_taps w |src|                      (same floor on both sides)
  3. dloc    vs fp64 autograd at the kernel's loc         16 eps sum_taps sum_c |g_c src_c|
  4. dvol    vs the numpy emulator of the fixed-point scatter fed the kernel's loc: torch.equal  (device only)
  5. dvol    vs fp64 autograd                             n(e) 2^-37 + 3 eps sum |contribution|        (also the emulator itself)
  6. dtheta  vs fp64 einsum of Mb with the KERNEL's dloc  (per + 32) eps sum_p |Mb dloc scale|
  7. ops.tps_warp + autograd end to end vs oracle.tps_warp, rtol 1e-3 as test_tps_warp

with eps = 2^-24; Mb is the fp32 basis cast to double in every reference.  Every tolerance is computed by tests/tps_ref.py from the
reference's own sums; no pixel is excluded anywhere.  The launch arithmetic the cases are built from:

  tps_warp_fwd_kernel / tps_warp_bwd_kernel   grid (ceil(HW / 256), B); floor clamped to [-2, W] x [-2, H] before (int)
  tps_warp_bwd_tiled_kernel (dvol requested)  grid (ceil(W / 16), ceil(H / 16), B); 32 x 32 LDS window starting 8 pixels before the
                                              tile; a valid tap outside the window goes to a global atomic
  tps_dtheta_partial_kernel                   256 chunks of per = ceil(HW / 256) pixels, staged 128 at a time; batch groups of 8,
                                              a thread owns combinations tid and tid + 256 of the group's nb * 50
  tps_dtheta_final_kernel                     16 lanes x 16 chunks each, then 16 terms
"""
import functools

import pytest
import torch

from oracle import ops as O
from multimodal_segmentation_amd import _native as N
from multimodal_segmentation_amd import ops as P
from tests import tps_ref as R
from tests.test_ops_parity import _native_error, check, device, rnd  # noqa: F401 (device: fixture)

C = 8
GARBAGE = -1.2345e30          # what every scratch and guard word holds before a launch
SENTINEL = 7.0e22             # prefill of a dloc buffer that must not be written
GUARD = 64                    # floats around ws and acc that must keep their content


@functools.lru_cache(maxsize=None)
def _basis(H, W):
    return O.tps_basis(H, W).float().contiguous()


def _vol(B, H, W, seed):
    """binary + 0.1 * noise, as test_tps_warp"""
    return (torch.rand(B, H, W, C, generator=torch.Generator().manual_seed(seed)) > 0.5).float() + rnd(B, H, W, C, seed=seed + 1) * 0.1


def _translation(H, W, dy, dx):
    """all 25 control points move by (dy, dx) pixels: the rows of Mb sum to 1, so every pixel does"""
    th = torch.zeros(1, 25, 2)
    th[..., 0] = dy / (H - 1)
    th[..., 1] = dx / (W - 1)
    return th


def _collapse(c=(0.37, 0.61)):
    """theta_j = c - cp_j: the spline reproduces affine maps, so every pixel samples the point c"""
    cp = O.nd_grid((5, 5), torch.float64)[0]
    return (torch.tensor(c, dtype=torch.float64)[None] - cp).float()[None]


# name -> (B, H, W, theta builder, dout scale).  The seeds are per case; theta is N(0, 1) * scale unless built otherwise.
def _case(name):
    if name.startswith('translate-'):
        _, axis, s = name.split('-', 2)
        H, W = 24, 20
        px = {'m0.5': -0.5, 'm1.5': -1.5, 'm2.5': -2.5, 'p0.5': 0.5, 'n-1.5': (W if axis == 'x' else H) - 1.5,
              'n-0.5': (W if axis == 'x' else H) - 0.5}[s]
        return 1, H, W, _translation(H, W, px if axis == 'y' else 0.0, px if axis == 'x' else 0.0), 1.0
    table = {
        # 58 % of the taps land in the window of their tile, 15 % are valid but outside it (global fallback), 27 % leave the image
        # (test_cases_reach_their_branches); tiles overhang in both axes (40 = 2 * 16 + 8, 36 = 2 * 16 + 4)
        'window-mix': (2, 40, 36, 0.3, 1.0),
        'window-mix-tiny-dout': (2, 40, 36, 0.3, 1e-9),        # resolution: contributions near 2^-36
        'small-warp': (2, 40, 36, 0.05, 1.0),                  # at most ~5 px: all in window, clipped windows on the edge tiles
        'one-tile-16x16': (1, 16, 16, 0.3, 1.0),
        'one-tile-17x15': (1, 17, 15, 0.3, 1.0),               # 2 x 1 tiles: one with a single live row, one idle column of threads
        'minimal-2x2': (1, 2, 2, 0.3, 1.0),                    # H - 1 = W - 1 = 1; HW = 4: per = 1, chunks 4..255 empty
        'minimal-2x129': (1, 2, 129, 0.3, 1.0),                # HW = 258: per = 2, chunks 129..255 start past the end
        'collapse': (1, 40, 36, 'collapse', 1.0),              # 1440 pixels on 4 x 8 accumulators: 1024 via LDS, 416 via the fallback
        'collapse-big-dout': (1, 40, 36, 'collapse', 1e4),     # range: sums of ~1e7, below 2^27
        'wild': (2, 24, 20, 'wild', 1.0),                      # sample 0: offsets of 1e12 -> loc ~ 2e13 px, beyond int32
        # second LDS staging round of tps_dtheta_partial_kernel: per = 129 (1 pixel), 130 (2 pixels), 128 (none, exact fit)
        'staging-B1-181x182': (1, 181, 182, 0.02, 1.0), 'staging-B9-181x182': (9, 181, 182, 0.02, 1.0),
        'staging-B1-182x182': (1, 182, 182, 0.02, 1.0), 'staging-B9-182x182': (9, 182, 182, 0.02, 1.0),
        'staging-B1-128x256': (1, 128, 256, 0.02, 1.0), 'staging-B9-128x256': (9, 128, 256, 0.02, 1.0),
        # batch groups of 8 at HW = 63 < 256 (per = 1, 193 empty chunks): B = 9 -> tail group of one sample (nloc = 50 < 256: no second
        # combination), B = 17 -> two full groups + tail
        'groups-B1-9x7': (1, 9, 7, 0.3, 1.0), 'groups-B8-9x7': (8, 9, 7, 0.3, 1.0),
        'groups-B9-9x7': (9, 9, 7, 0.3, 1.0), 'groups-B17-9x7': (17, 9, 7, 0.3, 1.0),
    }
    B, H, W, th, gs = table[name]
    if th == 'collapse':
        theta = _collapse()
    elif th == 'wild':
        theta = torch.cat([torch.full((1, 25, 2), 1e12), rnd(1, 25, 2, seed=41, scale=0.05)])
    else:
        theta = rnd(B, 25, 2, seed=31, scale=th)
    return B, H, W, theta, gs


TRANSLATIONS = ['translate-%s-%s' % (a, s) for a in 'xy' for s in ('m0.5', 'm1.5', 'm2.5', 'p0.5', 'n-1.5', 'n-0.5')]
FULL = ['window-mix', 'small-warp', 'one-tile-16x16', 'one-tile-17x15', 'minimal-2x2', 'minimal-2x129'] + TRANSLATIONS + \
       ['collapse', 'wild', 'window-mix-tiny-dout', 'collapse-big-dout']
DTHETA_ONLY = ['staging-B%d-%s' % (b, s) for s in ('181x182', '182x182', '128x256') for b in (1, 9)] + \
              ['groups-B%d-9x7' % b for b in (1, 8, 9, 17)]


@functools.lru_cache(maxsize=None)
def _inputs(name):
    B, H, W, theta, gs = _case(name)
    return _vol(B, H, W, 50), theta, rnd(B, H, W, C, seed=60) * gs, _basis(H, W)


def _filled(n, value, dev):
    return torch.full((n,), value, dtype=torch.float32, device=dev)


def run_fwd(dev, vol, theta, Mb):
    B, H, W, _ = vol.shape
    out = _filled(vol.numel(), float('nan'), dev).reshape(vol.shape)
    loc = _filled(B * H * W * 2, float('nan'), dev).reshape(B, H * W, 2)
    N.call('mmseg_tps_warp_fwd', vol.to(dev), theta.to(dev).contiguous(), Mb.to(dev), out, loc, B, H, W, C)
    return out.cpu(), loc.cpu()


def run_bwd(dev, vol, loc, Mb, dout, want_dvol=True, want_dtheta=True):
    """-> dvol, dtheta, dloc (CPU; dloc is the whole buffer, prefilled with SENTINEL).  ws and acc are cut out of buffers full of
    garbage with guard words on both sides: the launcher has to zero acc itself and nothing may be written outside either."""
    B, H, W, _ = vol.shape
    nws, nacc = N.call('mmseg_tps_workspace_floats', B), N.call('mmseg_tps_scatter_workspace_floats', B, H, W, C)
    wsbuf, accbuf = _filled(nws + 2 * GUARD, GARBAGE, dev), _filled(nacc + 2 * GUARD, GARBAGE, dev)
    ws, acc = wsbuf[GUARD:GUARD + nws], accbuf[GUARD:GUARD + nacc]
    assert acc.data_ptr() % 8 == 0
    dvol = _filled(vol.numel(), float('nan'), dev).reshape(vol.shape) if want_dvol else None
    dtheta = _filled(B * 50, float('nan'), dev).reshape(B, 25, 2) if want_dtheta else None
    dloc = _filled(B * H * W * 2, SENTINEL, dev).reshape(B, H * W, 2)
    N.call('mmseg_tps_warp_bwd', vol.to(dev), loc.to(dev), Mb.to(dev), dout.to(dev), dvol, dtheta, dloc,
           ws if want_dtheta else None, acc if want_dvol else None, B, H, W, C)
    for buf, n in ((wsbuf, nws), (accbuf, nacc)):
        assert (buf[:GUARD] == GARBAGE).all() and (buf[GUARD + n:] == GARBAGE).all(), 'a guard word around ws / acc was written'
    return (None if dvol is None else dvol.cpu()), (None if dtheta is None else dtheta.cpu()), dloc.cpu()


_runs = {}


def _run(name, dev):
    """forward (+ backward) of a case on `dev`, launched once and shared by the tests of the case; read-only"""
    if (name, dev) not in _runs:
        vol, theta, dout, Mb = _inputs(name)
        out, loc = run_fwd(dev, vol, theta, Mb)
        dvol, dtheta, dloc = run_bwd(dev, vol, loc, Mb, dout, want_dvol=name in FULL)
        _runs[name, dev] = dict(out=out, loc=loc, dvol=dvol, dtheta=dtheta, dloc=dloc)
    return _runs[name, dev]


@functools.lru_cache(maxsize=None)
def _bwd_ref(name, dev):
    vol, _, dout, _ = _inputs(name)
    return R.backward_reference(vol, _run(name, dev)['loc'], dout)


def _within(got, ref, tol, what):
    """|got - ref| <= tol element by element; prints the worst figure before it asserts"""
    assert got.shape == ref.shape, '%s: shape %s vs %s' % (what, tuple(got.shape), tuple(ref.shape))
    assert torch.isfinite(got).all(), '%s: not finite (an element was never written?)' % what
    err = (got.double() - ref).abs()
    tol = tol.expand_as(err)
    worst = (err / tol.clamp_min(1e-300)).max().item()
    print('%s: max err %.3e, worst err / tolerance %.3f' % (what, err.max().item(), worst))
    bad = err > tol
    assert not bad.any(), '%s: %d of %d elements beyond their tolerance, worst err / tolerance %.3g (max err %.3e)' % (
        what, int(bad.sum()), bad.numel(), worst, err.max().item())


# ======================================================================================================================
# stages 1 and 2: every case
# ======================================================================================================================
@pytest.mark.parametrize('name', FULL + DTHETA_ONLY)
def test_forward(name, device):
    """loc against fp64 grid + Mb theta; the gather against the fp64 resampler at the kernel's own loc"""
    vol, theta, _, Mb = _inputs(name)
    B, H, W, _ = vol.shape
    r = _run(name, device)
    ref, tol = R.loc_reference(Mb, theta, H, W)
    _within(r['loc'], ref, tol, 'loc')
    ref, mag = R.gather_reference(vol, r['loc'])
    _within(r['out'].reshape(B, H * W, C), ref, 16 * R.EPS * mag, 'out')


# ======================================================================================================================
# stages 3, 5, 6 (both devices) and 4 (device only)
# ======================================================================================================================
def _per(H, W):
    return (H * W + 255) // 256


@pytest.mark.parametrize('name', FULL + DTHETA_ONLY)
def test_dloc_and_dtheta(name, device):
    """dloc against fp64 autograd at the kernel's loc (the one-sided derivative at ax == 0 is the same on both sides); dtheta against
    the fp64 reduction of the kernel's own dloc.  The DTHETA_ONLY cases pass dvol = NULL: the untiled kernel, no scatter."""
    vol, _, _, Mb = _inputs(name)
    B, H, W, _ = vol.shape
    r, ref = _run(name, device), _bwd_ref(name, device)
    _within(r['dloc'], ref['dloc'], 16 * R.EPS * ref['dloc_mag'], 'dloc')
    want, tol = R.dtheta_reference(Mb, r['dloc'], H, W, _per(H, W))
    _within(r['dtheta'], want, tol, 'dtheta')


@pytest.mark.parametrize('name', FULL)
def test_dvol_magnitude(name, device):
    """dvol against fp64 autograd: n(e) roundings to 2^-36 + the fp32 products"""
    ref = _bwd_ref(name, device)
    _within(_run(name, device)['dvol'], ref['dvol'], R.dvol_tolerance(ref), 'dvol')


@pytest.mark.parametrize('name', FULL)
def test_scatter_emulator_against_fp64(name, device):
    """the emulator that test_dvol_bits trusts meets the same bound as the kernel, on the loc of either backend"""
    vol, _, dout, _ = _inputs(name)
    ref = _bwd_ref(name, device)
    _within(R.scatter_emulator(_run(name, device)['loc'], dout, vol.shape[1], vol.shape[2]), ref['dvol'], R.dvol_tolerance(ref),
            'emulated dvol')


@pytest.mark.gpu
@pytest.mark.parametrize('name', FULL)
def test_dvol_bits(name):
    """the fixed-point scatter is integer arithmetic, so dvol is predicted bit for bit: one lost, doubled or misplaced tap or window
    flush changes it"""
    vol, _, dout, _ = _inputs(name)
    r = _run(name, 'cuda')
    want = R.scatter_emulator(r['loc'], dout, vol.shape[1], vol.shape[2])
    diff = (r['dvol'] != want)
    print('dvol: %d of %d elements differ from the emulator' % (int(diff.sum()), diff.numel()))
    assert torch.equal(r['dvol'], want), 'dvol: %d of %d elements differ from the emulator, largest difference %.3e' % (
        int(diff.sum()), diff.numel(), (r['dvol'].double() - want.double()).abs().max().item())


# ======================================================================================================================
# the wild offsets, the skipped gradients
# ======================================================================================================================
def test_wild_offsets_are_clamped_and_stay_in_their_sample(device):
    """loc ~ 2e13 px would overflow the int conversion without the clamp: sample 0 samples nothing, so its out, dvol and dloc are
    exactly zero, and sample 1 is what it is when it runs alone (bit for bit on the device, where a sample's arithmetic does not
    depend on the batch; the stage tests hold it to the fp64 reference on both backends)"""
    vol, theta, dout, Mb = _inputs('wild')
    r = _run('wild', device)
    assert r['loc'][0].abs().min() > 2.0 ** 31
    for k in ('out', 'dvol', 'dloc', 'dtheta'):
        assert (r[k][0] == 0).all(), '%s of the wild sample is not exactly zero' % k
    assert r['out'][1].abs().max() > 0.5 and r['dvol'][1].abs().max() > 0.1
    if device == 'cuda':
        out1, loc1 = run_fwd(device, vol[1:], theta[1:], Mb)
        dvol1, dtheta1, dloc1 = run_bwd(device, vol[1:], loc1, Mb, dout[1:])
        for k, v in (('out', out1), ('loc', loc1), ('dvol', dvol1), ('dtheta', dtheta1), ('dloc', dloc1)):
            assert torch.equal(r[k][1:], v), '%s of sample 1 depends on sample 0' % k


def test_dvol_without_dtheta(device):
    """dtheta = NULL: the tiled kernel runs with dloc = NULL -- same dvol bits, and the dloc buffer keeps its content"""
    vol, _, dout, Mb = _inputs('window-mix')
    r = _run('window-mix', device)
    dvol, dtheta, dloc = run_bwd(device, vol, r['loc'], Mb, dout, want_dtheta=False)
    assert dtheta is None and (dloc == SENTINEL).all()
    assert torch.equal(dvol, r['dvol'])


# ======================================================================================================================
# the fixed-point accumulator
# ======================================================================================================================
@pytest.mark.parametrize('name', ['window-mix', 'collapse'])
def test_backward_is_repeatable(name, device):
    vol, _, dout, Mb = _inputs(name)
    r = _run(name, device)
    dvol, dtheta, dloc = run_bwd(device, vol, r['loc'], Mb, dout)
    assert torch.equal(dvol, r['dvol']) and torch.equal(dtheta, r['dtheta']) and torch.equal(dloc, r['dloc'])


def test_dvol_of_a_sample_does_not_depend_on_the_batch(device):
    vol, _, dout, Mb = _inputs('window-mix')
    r = _run('window-mix', device)
    dvol, _, _ = run_bwd(device, vol[1:], r['loc'][1:], Mb, dout[1:], want_dtheta=False)
    assert torch.equal(dvol, r['dvol'][1:])


def test_accumulator_resolution(device):
    """cotangents of 1e-9: contributions of a few 2^-36, the n 2^-37 term of the bound dominates -- and they are not flushed to zero.
    (The bound and, on the device, the bits: test_dvol_magnitude / test_dvol_bits[window-mix-tiny-dout].)  The bound is tight
    here by construction: an element with one tap whose contribution falls next to half a unit is off by almost 2^-37."""
    ref = _bwd_ref('window-mix-tiny-dout', device)
    tol = R.dvol_tolerance(ref)
    assert (ref['dvol_n'] * 2.0 ** -37 > 3 * R.EPS * ref['dvol_mag'])[ref['dvol_n'] > 0].all()
    dvol = _run('window-mix-tiny-dout', device)['dvol']
    _within(dvol, ref['dvol'], tol, 'dvol')
    assert (dvol != 0).any()
    assert ((dvol != 0) | (ref['dvol'].abs() <= tol)).all(), 'an element of dvol was flushed to zero'


def test_accumulator_range(device):
    """cotangents of 1e4 on the collapsed warp: per-element sums of ~1e7, inside the exact range of 2^27 (checked on the fp64
    reference first).  (The bound and the bits: test_dvol_magnitude / test_dvol_bits[collapse-big-dout].)"""
    ref = _bwd_ref('collapse-big-dout', device)
    assert 1e6 < ref['dvol_mag'].max() < R.FX_RANGE
    _within(_run('collapse-big-dout', device)['dvol'], ref['dvol'], R.dvol_tolerance(ref), 'dvol')


# ======================================================================================================================
# the inputs reach what the cases are named after (computed from the fp64 reference alone)
# ======================================================================================================================
def test_cases_reach_their_branches():
    def taps(name):
        """-> fractions of the 4 * B * HW taps that are valid and land in / outside the 32 x 32 window of their pixel's tile"""
        _, H, W, theta, _ = _case(name)
        loc = R.loc_reference(_basis(H, W), theta, H, W)[0]
        p = torch.arange(H * W)
        wy0, wx0 = (p // W) // 16 * 16 - 8, (p % W) // 16 * 16 - 8
        fx, fy = loc[..., 0].floor().long(), loc[..., 1].floor().long()
        inw = outw = 0
        for t in range(4):
            xi, yi = fx + (t & 1), fy + (t >> 1)
            ok = (xi >= 0) & (xi < W) & (yi >= 0) & (yi < H)
            win = (yi >= wy0) & (yi < wy0 + 32) & (xi >= wx0) & (xi < wx0 + 32)
            inw, outw = inw + (ok & win).sum().item(), outw + (ok & ~win).sum().item()
        n = 4.0 * fx.numel()
        print('%s: %.3f of the taps in window, %.3f global fallback, %.3f outside the image' % (name, inw / n, outw / n, 1 - (inw + outw) / n))
        return inw / n, outw / n

    inw, outw = taps('window-mix')
    assert inw > 0.1 and outw > 0.1 and inw + outw < 0.9      # all three kinds of tap, none of them rare
    inw, outw = taps('small-warp')
    assert outw == 0 and inw > 0.9                             # everything in window
    inw, outw = taps('collapse')
    # the point (14.4, 21.4) is in the windows of the 2 x 2 tiles at the top left (1024 pixels) and in none of the other five
    # (416 pixels): LDS contention for the former, 416 * 8 global atomics on each of the 4 x 8 accumulators for the latter
    assert inw == 1024 / 1440 and outw == 416 / 1440
    _, H, W, theta, _ = _case('collapse')
    loc = R.loc_reference(_basis(H, W), theta, H, W)[0]
    assert (loc - loc[:, :1]).abs().max() < 1e-4               # one sample point for all 1440 pixels
    for name in TRANSLATIONS:
        _, H, W, theta, _ = _case(name)
        loc = R.loc_reference(_basis(H, W), theta, H, W)[0]
        q = torch.flip(O.nd_grid((H, W), torch.float64)[0], dims=[-1]) * torch.tensor([W - 1, H - 1], dtype=torch.float64)
        s = loc - q[None]
        assert (s - s[:, :1]).abs().max() < 1e-4 and s.abs().max() > 0.49        # a pure translation
    for name, per in (('staging-B1-181x182', 129), ('staging-B1-182x182', 130), ('staging-B1-128x256', 128)):
        _, H, W, _, _ = _case(name)
        assert _per(H, W) == per


# ======================================================================================================================
# stage 7: through ops.tps_warp and autograd; what is refused
# ======================================================================================================================
LARGE_WARP_SEED = 0


def test_tps_warp_large_warp_end_to_end(device):
    """ops.tps_warp and its autograd node against oracle.tps_warp in the style of test_tps_warp, with a warp of many pixels.  fp32
    and fp64 may floor a coordinate differently only within the loc tolerance of an integer: the seed is one for which no coordinate
    that touches the image is that close (asserted on the fp64 oracle), so the comparison needs no mask."""
    B, H, W = 1, 24, 20
    vol, theta, Mb = _vol(B, H, W, 70), rnd(B, 25, 2, seed=LARGE_WARP_SEED, scale=0.3), _basis(H, W)
    loc, tol = R.loc_reference(Mb, theta, H, W)
    near = (loc - loc.round()).abs() <= tol
    touches = (loc[..., 0] > -1.5) & (loc[..., 0] < W + 0.5) & (loc[..., 1] > -1.5) & (loc[..., 1] < H + 0.5)
    assert not (near & touches[..., None]).any(), 'choose another seed: a coordinate lies on a grid line'
    q = torch.flip(O.nd_grid((H, W), torch.float64)[0], dims=[-1]) * torch.tensor([W - 1, H - 1], dtype=torch.float64)
    assert (loc - q[None]).abs().max() > 8
    check(lambda v, t: P.tps_warp(v, t, Mb.to(v.device)), lambda v, t: O.tps_warp(v, t), [vol, theta], device, rtol=1e-3)


def test_tps_rejects_what_its_kernels_cannot_hold(device):
    """C != 8 and H < 2 or W < 2 (the normalisation divides by H - 1 and W - 1) are refused by both entry points before any launch"""
    for B, H, W, Cc in ((1, 4, 4, 7), (1, 1, 4, 8), (1, 4, 1, 8)):
        vol, theta, Mb = torch.zeros(B, H, W, Cc).to(device), torch.zeros(B, 25, 2).to(device), torch.zeros(H * W, 25).to(device)
        with pytest.raises(_native_error()):
            P.tps_warp(vol, theta, Mb)
        loc, dout = torch.zeros(B, H * W, 2).to(device), torch.zeros(B, H, W, Cc).to(device)
        dvol, dtheta, dloc = torch.zeros_like(vol), torch.zeros_like(theta), torch.zeros_like(loc)
        ws = torch.zeros(N.call('mmseg_tps_workspace_floats', B)).to(device)
        acc = torch.zeros(max(2, 2 * vol.numel())).to(device)
        with pytest.raises(_native_error()):
            N.call('mmseg_tps_warp_bwd', vol, loc, Mb, dout, dvol, dtheta, dloc, ws, acc, B, H, W, Cc)


def test_tps_warp_refuses_a_basis_the_kernel_would_misread(cpu_backend):
    """ops.tps_warp hands Mb to the kernel as a raw pointer: fp64, non-contiguous or on another device is refused, not converted"""
    B, H, W = 1, 4, 5
    vol, theta, Mb = _vol(B, H, W, 80), torch.zeros(B, 25, 2), _basis(H, W)
    P.tps_warp(vol, theta, Mb)
    for bad in (Mb.double(), Mb.t().contiguous().t(), torch.empty(H * W, 25, device='meta')):
        assert bad.shape == Mb.shape
        with pytest.raises(ValueError, match='basis'):
            P.tps_warp(vol, theta, bad)
