"""Predicted label volumes for a folder of exported volumes, written in each volume's own geometry (build-defined: the reference
writes no segmentation; its `plot_images` PNG dumps are visualisation).

For every volume of the folder (loaders/volume_folder.py; labels are optional) and every modality m:
    images (device)  = loader.load_volume_for_prediction(volume)            resampled, rescaled, cropped / padded on the device
    prob   (device)  = model.predict_mask(m, mode, images)                   in batches of conf.batch_size slices
    label  (device)  = ops.restore_label(prob, label_values, geometry, order)   uint8 grey values on the raw H x W grid
and the selected slices are scattered back to their positions in a zero [S_file,H,W] array, so that the output lines up with the
input file.  The raw arrays cross the bus once each way: the image up, 1 byte per pixel down; no probability map reaches the host.

    <out>/<file name of the input>.npz     label [S_file,H,W] uint8 (0 and the grey values of `label_values`), resolution (copied)
    <out>/predictions.json                 settings only: source folder, mode, order, model folder, per file the selected slices
    <out>/results_native_<modality>.csv    where the input files carry a `label`: Dice on the raw grid, header and row format of
                                           model_tester.write_results, one row per labelled volume
    <out>/results_surface_<modality>.csv   where they also carry `slice_spacing`: RAVD (%), ASSD and MSSD (mm) of the union of the
                                           organs and of every organ, one row per scored volume
    <out>/results_robust_<modality>.csv    with robust=(percentile, tolerance in mm), for the files the surface file scores: HD (the
                                           percentile of the surface distances, mm) and NSD (the share of them within the tolerance)
                                           of the union of the organs and of every organ, one row per scored volume
    <out>/results_components_<modality>.csv   with components='largest': per organ the number of connected components, its voxels
                                           before the filter and the voxels kept, one row per volume
    <out>/results_holes_<modality>.csv     with fill_holes='2d' or '3d': per organ the number of enclosed holes, its voxels before
                                           the filling and the voxels added, one row per volume
    <out>/results_smooth_<modality>.csv    with smooth='open', 'close' or 'smooth': per organ its voxels before, the voxels removed
                                           and the voxels added, one row per volume
    <out>/results_crf_<modality>.csv       with crf='default' or 'key=value,...': per organ its voxels on the file grid before the
                                           refinement, the voxels removed and the voxels added, one row per volume

crf='default' | 'key=value,...' (build-defined, off by default; the rule is in INTEGRATION.md section 5) refines the probability map of
modality m against the slices of that modality as the network saw them, before anything else: a mean-field CRF over the (2 radius + 1)^2
window with an appearance and a smoothness kernel (ops.crf_refine, csrc/crf.hip), the one step of the way back that looks at the image
again.  With tta it follows the merge, against the unturned slices; with tiles it runs tile by tile before the blend.  The order is
crf, restore_label, smoothing, filter, filling, then scores and file.  predictions.json then carries `crf`, the seven parameters in
force.  The defaults are untuned starting values (tools/crf_sweep.py scores a grid of settings on a labelled folder).

components='largest' (build-defined, off by default; the rule is in INTEGRATION.md section 5) keeps, per organ, the largest 3-D connected
component: the prediction is scattered to the file grid [S_file,H,W] on the device and filtered there (ops.keep_largest_components),
so that neighbours across slices are those of the file; the filtered volume is what is scored and written.

fill_holes='2d' | '3d' (build-defined, off by default; the rule is in INTEGRATION.md section 5) then sets the zeros that an organ
encloses to that organ's grey value (ops.fill_label_holes, on the file grid as well): slice by slice with '2d', in the volume with
'3d'.  It runs after the component filter, so that an island which the filter turned into zeros inside an organ is closed again.

smooth='open' | 'close' | 'smooth' with smooth_radius in mm (build-defined, off by default, no default radius; the rule is in
INTEGRATION.md section 5) opens, closes or opens and then closes every organ by a ball of that radius (ops.smooth_label, on the file
grid as well, with the file's own spacings: `resolution` in the slice and, with smooth_extent='3d', `slice_spacing` across slices;
'2d', the default, keeps the ball in the slice).  Unselected slices of the file are zero there and count as background with '3d'.
It runs FIRST, before the component filter and the hole filling: restore_label, smoothing, filter, filling, then scores and file.  An
opening cuts a neck narrower than the ball before the filter looks, so that the filter drops the blob behind it; a fragment that a
closing joins to its organ survives the filter.  What is scored is what is written.

tiles=True (build-defined, off by default; the rule is in INTEGRATION.md section 5) predicts the whole resampled frame instead of its
centre input_shape window: per volume and predicted modality the frame is cut into overlapping tiles (loaders/volume_folder.tile_axis,
tile_overlap pixels at least, default half the input extent), the tiles of every modality go through predict_mask as one batch of
TR*TC*S slices, ops.blend_tiles blends the probability maps on the frame and ops.restore_label takes the whole frame as its window, so
that no raw pixel is cropped away.  A frame that one tile holds takes the path without the option.  predictions.json then carries
`tiles`, `tile_overlap` and per file `tile_origins`.

tta='id,fliplr,...' (build-defined, off by default; the rule and the table of views are in INTEGRATION.md section 5) predicts every
slice under several views (flips, right-angle turns, small rotations: the transformations the models are trained under), brings every
view's probability map back and averages them: ops.augment_gather makes the V*N views of the N containers of every modality,
predict_mask runs over them in batches, ops.merge_views merges the maps on the device, and the way back goes on from the merged map.
With tiles=True the views act on the tile containers, and the merged tiles are blended.  predictions.json then carries `tta`.

members=[further models] of VolumePredictor and uncertainty=True of run (build-defined, off by default; the rule is in INTEGRATION.md
section 5) predict with several models together, as the folds of a cross-validation are used, and keep what a mean throws away.  Every
model (the run folder's first, then the list) predicts the volume, under every view with tta; ops.members_accumulate adds each model's
maps into one pair of buffers and ops.members_finish leaves the mean map over all models and views and two planes in [0, 1]: the
entropy H of the mean over the organs and the rest, and the mutual information I, the part of H that is disagreement between the
members.  The way back goes on from the mean: crf (on the mean), restore_label, smoothing, filter, filling.  The planes are those
BEFORE the crf; with tiles=True the tiles' planes are blended like the maps (ops.blend_tiles), and a blend of entropies only
approximates the entropy of the blend.  One model alone and uncertainty=True gives the same labels as without, I == 0, and H.
    <out>/uncertainty/<file name>.npz      entropy, mutual_information [S_file,H,W] uint8 (level / 255; ops.restore_map, 1 byte per pixel
                                           down each), resolution and, where the file carries it, slice_spacing
    <out>/results_calibration_<modality>.csv   where the files carry a `label`: per volume and organ ECE, MCE, Brier score, NLL and the
                                           number of pixels, from ops.calibration_table with calibration_bins bins on the map that the
                                           labels come from (after the crf if it is on).  EVERY raw pixel inside the window counts, so
                                           the scores are dominated by the background
    <out>/reliability_<modality>.csv       per organ and bin, summed over the volumes: pixels, mean confidence, observed frequency; for
                                           anyone who wants another convention than the one above
    <out>/results_uncertainty_<modality>.csv   per volume the mean entropy and mutual information over the correctly and over the wrongly
                                           labelled pixels of the selected slices (ops.uncertainty_by_error), on the final prediction,
                                           after every filter
predictions.json then carries `ensemble` (the members' run folders), `uncertainty` and `calibration_bins`.

Dice is costs.dice's formula applied to pixel counts (ops.label_overlap): per slice (2 I + 1e-12) / (P + T + 1e-12), the joint score
from the counts summed over the organs, then the mean over the selected slices.

The scores in mm (build-defined: the reference scores Dice only; the rules restate the metric set of the CHAOS challenge from memory,
INTEGRATION.md section 5) are taken on the whole file grid [S_file,H,W]: the prediction is scattered to its file positions on the
device, the truth slices that `slices` does not select are zero, and ops.surface_metrics returns one [K+1,6] table per volume, the only
thing that leaves the device.  With robust=(percentile, tolerance) (build-defined, off by default; HD(q) and NSD(tau) of INTEGRATION.md
section 5) ops.surface_scores takes its place: the same table with two more columns, from the same distance transforms, so that one
call serves both CSV files.  `score_volume` and `ScoreSheet` are shared with tools/score_predictions.py, which scores label
volumes written earlier (`score_folder`)."""
import collections
import json
import logging
import math
import os

import numpy as np
import torch

from . import nn, ops
from .loaders.volume_folder import VolumeFolderLoader, tile_weights
from .model_tester import FUSION_MODES, write_results

log = logging.getLogger('volume_predictor')

SMOOTH = 1e-12          # costs.dice


def checkpoint_of(folder):
    """the checkpoint a run folder holds (models/dafnet.py, models/mmsdnet.py `load_models`), or None"""
    for path in (os.path.join(folder, 'models', 'D_Mask'), os.path.join(folder, 'supervised_trainer')):
        if os.path.exists(path):
            return path
    return None


def dice_from_counts(counts):
    """counts [S,K,3] = (|pred|, |truth|, |both|) per slice and organ -> (joint, [per organ]) as model_tester.volume_scores"""
    c = np.asarray(counts, np.float64)

    def score(x):          # x [S,3]
        return float(np.mean((2 * x[:, 2] + SMOOTH) / (x[:, 1] + x[:, 0] + SMOOTH)))
    return score(c.sum(axis=1)), [score(c[:, k]) for k in range(c.shape[1])]


def chaos_from_table(table):
    """table [K+1,6] = nP, nT, |surface(P)|, |surface(T)|, sum, max of ops.surface_metrics -> [K+1,3] = RAVD (%), ASSD (mm), MSSD (mm):
    RAVD = 100 |nP - nT| / nT (nan when nT = 0), ASSD = sum / (|surface(P)| + |surface(T)|), MSSD = max; the last two are nan
    where the table says so (an empty surface)"""
    t = np.asarray(table, np.float64)
    out = np.full((t.shape[0], 3), np.nan)
    for k, (n_p, n_t, s_p, s_t, total, largest) in enumerate(t):
        if n_t > 0:
            out[k, 0] = 100.0 * abs(n_p - n_t) / n_t
        if s_p > 0 and s_t > 0:
            out[k, 1], out[k, 2] = total / (s_p + s_t), largest
    return out


def check_robust(robust):
    """robust: None or (percentile in [0, 100], tolerance in mm >= 0) -> None or the pair as floats (the ranges are those of the op)"""
    if robust is None:
        return None
    try:
        q, tau = (float(v) for v in robust)
    except (TypeError, ValueError):
        raise ValueError('robust must be None or (percentile, tolerance in mm), got %r' % (robust,))
    return ops._robust_args('robust', q, tau)


def robust_from_table(table):
    """table [K+1,8] of ops.surface_scores -> [K+1,2] = HD (mm: column 8, the percentile of the surface distances of both directions
    together), NSD = column 7 / (|surface(P)| + |surface(T)|); both nan where the table says so (an empty surface)"""
    t = np.asarray(table, np.float64)
    out = np.full((t.shape[0], 2), np.nan)
    for k, row in enumerate(t):
        if row[2] > 0 and row[3] > 0:
            out[k] = row[7], row[6] / (row[2] + row[3])
    return out


def _on_file_grid(x, geometry):
    """x: uint8 [S,H,W] on the device, the selected slices of one file in order -> (x on the zero file grid [S_file,H,W], its positions)"""
    where = torch.as_tensor(np.asarray(geometry['slices'], np.int64), device=x.device)
    grid = tuple(int(n) for n in geometry['raw_shape'])
    return torch.zeros(grid, dtype=torch.uint8, device=x.device).index_copy_(0, where, x), where


def score_volume(pred, label, values, geometry, surface=True, robust=None):
    """pred, label: uint8 [S,H,W] on the device, the selected slices of one file in order; geometry: the record of
    loader.load_volume_for_prediction (raw_shape, slices, resolution, slice_spacing are read) -> (joint Dice, [per organ], scores in
    mm [K+1,3], HD and NSD [K+1,2]), the tables with the union LAST.  The third is None when surface is off, the fourth without robust =
    (percentile, tolerance in mm), both for a file without slice_spacing; otherwise both come from one ops.surface_scores call."""
    robust = check_robust(robust)
    joint, per_organ = dice_from_counts(nn.to_numpy(ops.label_overlap(pred, label, values)))
    if (not surface and robust is None) or geometry.get('slice_spacing') is None:
        return joint, per_organ, None, None
    on_grid = [_on_file_grid(x, geometry)[0] for x in (pred, label)]
    spacing = (float(geometry['slice_spacing']), float(geometry['resolution'][0]), float(geometry['resolution'][1]))
    if robust is None:
        table = ops.surface_metrics(on_grid[0], on_grid[1], values, spacing)
        return joint, per_organ, chaos_from_table(nn.to_numpy(table)), None
    table = nn.to_numpy(ops.surface_scores(on_grid[0], on_grid[1], values, spacing, robust[0], robust[1]))
    return joint, per_organ, (chaos_from_table(table[:, :6]) if surface else None), robust_from_table(table)


COMPONENTS = (None, 'largest')


def check_components(components, connectivity):
    if components not in COMPONENTS:
        raise ValueError("components must be None or 'largest', got %r" % (components,))
    if connectivity not in (6, 26):
        raise ValueError('connectivity must be 6 (faces) or 26 (faces, edges, corners), got %r' % (connectivity,))


def keep_largest(pred, values, geometry, connectivity=6):
    """pred: uint8 [S,H,W] on the device, the selected slices of one file in order -> (the same slices after the filter, stats [K,3]
    on the device).  The filter runs on the file grid [S_file,H,W] (unselected slices are zero), so that two voxels are neighbours
    along the slice axis when they are in the file."""
    on_grid, where = _on_file_grid(pred, geometry)
    kept, stats = ops.keep_largest_components(on_grid, values, connectivity)
    return kept.index_select(0, where), stats


FILL_HOLES = (None,) + ops.HOLE_MODES


def check_fill_holes(fill_holes):
    if fill_holes not in FILL_HOLES:
        raise ValueError("fill_holes must be None, '2d' or '3d', got %r" % (fill_holes,))


def fill_holes(pred, values, geometry, mode):
    """pred: uint8 [S,H,W] on the device, the selected slices of one file in order -> (the same slices with the enclosed zeros of
    every organ filled, stats [K,3] on the device).  Like keep_largest on the file grid [S_file,H,W] (unselected slices are zero): a
    cavity whose lid is a slice that the file holds but the selection skips is open."""
    on_grid, where = _on_file_grid(pred, geometry)
    filled, stats = ops.fill_label_holes(on_grid, values, mode)
    return filled.index_select(0, where), stats


SMOOTH_OPS = (None,) + ops.SMOOTH_OPS


def check_smooth(smooth, radius, extent='2d'):
    """smooth: None or one of ops.SMOOTH_OPS, radius: mm, finite and > 0 (there is no default), extent: '2d' or '3d' -> the radius as a
    float, None without smooth"""
    if smooth not in SMOOTH_OPS:
        raise ValueError("smooth (--predict_smooth) must be None, 'open', 'close' or 'smooth', got %r" % (smooth,))
    if extent not in ops.SMOOTH_EXTENTS:
        raise ValueError("smooth_extent (--predict_smooth_extent) must be '2d' or '3d', got %r" % (extent,))
    if smooth is None:
        return None
    if radius is None:
        raise ValueError('smooth=%r needs smooth_radius (--predict_smooth_radius), the radius of the ball in mm: there is no default'
                         % (smooth,))
    try:
        r = float(radius)
    except (TypeError, ValueError):
        r = float('nan')
    if isinstance(radius, bool) or not (r > 0 and r < float('inf')):
        raise ValueError('smooth_radius (--predict_smooth_radius) must be a finite number of mm > 0, got %r' % (radius,))
    return r


def smooth(pred, values, geometry, op, radius, extent='2d'):
    """pred: uint8 [S,H,W] on the device, the selected slices of one file in order -> (the same slices with every organ opened, closed
    or smoothed by the ball of `radius` mm, stats [K,3] = (before, removed, added) on the device).  Like keep_largest on the file grid
    [S_file,H,W] with the file's spacings: geometry['resolution'] in the slice and, with extent '3d', geometry['slice_spacing'] across
    slices.  Unselected slices are zero: with '3d' they are background to an erosion and empty to a dilation; '2d' never looks at
    them."""
    r = check_smooth(op, radius, extent)
    dz = geometry.get('slice_spacing')
    if extent == '3d' and dz is None:
        raise ValueError("%s holds no 'slice_spacing': smooth_extent='3d' (--predict_smooth_extent 3d) needs the mm between slices"
                         % (geometry.get('file'),))
    spacing = (None if dz is None else float(dz), float(geometry['resolution'][0]), float(geometry['resolution'][1]))
    in_use = spacing[1:] if extent == '2d' else spacing
    if all(s > 0 and s < float('inf') for s in in_use) and max(ops.smooth_reach(spacing, r, extent)) > ops.SMOOTH_MAX_REACH:
        raise ValueError('%s: smooth_radius=%r mm (--predict_smooth_radius) reaches %s voxels at spacing %r, at most %d per axis'
                         % (geometry.get('file'), r, ops.smooth_reach(spacing, r, extent), in_use, ops.SMOOTH_MAX_REACH))
    on_grid, where = _on_file_grid(pred, geometry)
    done, stats = ops.smooth_label(on_grid, values, spacing, r, op, extent)
    return done.index_select(0, where), stats


def check_tile_overlap(tile_overlap, input_shape):
    """tile_overlap: None (half the input extent per axis), one number of pixels for both axes or (rows, columns) -> (rows, columns);
    0 <= overlap < the input extent of its axis"""
    extent = (int(input_shape[0]), int(input_shape[1]))
    if tile_overlap is None:
        return extent[0] // 2, extent[1] // 2
    pair = tuple(tile_overlap) if isinstance(tile_overlap, (tuple, list)) else (tile_overlap, tile_overlap)
    whole = len(pair) == 2 and all(isinstance(o, (int, np.integer)) and not isinstance(o, bool) for o in pair)
    if not whole or any(not 0 <= int(o) < n for o, n in zip(pair, extent)):
        raise ValueError('tile_overlap (--predict_tile_overlap) must be a whole number of pixels in [0, input extent) per axis: the input '
                         'is %d x %d, got %r' % (extent[0], extent[1], tile_overlap))
    return int(pair[0]), int(pair[1])


MAX_VIEWS = ops.MAX_VIEWS
EXACT_VIEWS = ('id', 'fliplr', 'flipud', 'rot180', 'transpose', 'antitranspose', 'rot90', 'rot270')
TRANSPOSING_VIEWS = EXACT_VIEWS[4:]
VIEW_PRESETS = dict(flips=EXACT_VIEWS[:4], d4=EXACT_VIEWS)
# tokens: the expanded list; forward / back: [V,6] fp64, per view the matrices F (view pixel -> the image pixel it shows) and B (image pixel
# -> the view pixel that shows it) in ops.augment_gather's convention (m0*r + m1*c + m2, m3*r + m4*c + m5)
Views = collections.namedtuple('Views', ('tokens', 'forward', 'back'))


def _rotation(theta, cy, cx):
    """the turn by theta about the centre (cy, cx) of the container"""
    cos, sin = math.cos(theta), math.sin(theta)
    return [cos, -sin, cy - cos * cy + sin * cx, sin, cos, cx - sin * cy - cos * cx]


def view_matrices(token, OH, OW):
    """(F, B) of one token (the table of INTEGRATION.md section 5), each six floats; written out per token, never inverted numerically.
    The eight exact tokens hold 0, +-1 and whole offsets only.  Raises ValueError for a token the table does not have."""
    h, w = float(OH - 1), float(OW - 1)
    same = dict(id=[1., 0., 0., 0., 1., 0.], fliplr=[1., 0., 0., 0., -1., w], flipud=[-1., 0., h, 0., 1., 0.],
                rot180=[-1., 0., h, 0., -1., w], transpose=[0., 1., 0., 1., 0., 0.], antitranspose=[0., -1., w, -1., 0., h])
    if token in same:
        return same[token], list(same[token])
    quarter, three = [0., 1., 0., -1., 0., w], [0., -1., h, 1., 0., 0.]          # (c, OW-1-r) and (OH-1-c, r)
    if token == 'rot90':
        return quarter, three
    if token == 'rot270':
        return three, quarter
    try:
        if not token.startswith('rot'):
            raise ValueError(token)
        degrees = float(token[3:])
    except ValueError:
        raise ValueError('unknown view %r' % (token,))
    if not math.isfinite(degrees) or math.fmod(degrees, 360.0) == 0.0:
        raise ValueError('view %r: the angle must be finite and no multiple of 360 degrees' % (token,))
    theta = degrees * math.pi / 180
    return _rotation(theta, h / 2, w / 2), _rotation(-theta, h / 2, w / 2)


def check_tta(tta, input_shape):
    """tta: None, 'none' or 'id' (off) -> None; else a comma-separated list or a sequence of tokens and presets (EXACT_VIEWS, 'rotA' with A
    in degrees, VIEW_PRESETS) -> Views for containers of input_shape: 1 to 16 distinct views, the identity first (it covers every
    pixel, so the mean over the covering views never divides by nothing), transposing views on square inputs only"""
    OH, OW = int(input_shape[0]), int(input_shape[1])

    def refuse(why):
        raise ValueError('tta (--predict_tta) must be a list of views (%s, rotA with A in degrees; presets %s) that begins with id: the '
                         'input is %d x %d, got %r: %s' % (', '.join(EXACT_VIEWS), ', '.join(sorted(VIEW_PRESETS)), OH, OW, tta, why))
    if tta is None:
        return None
    if isinstance(tta, str):
        listed = tta.split(',')
    else:
        try:
            listed = list(tta)
        except TypeError:
            refuse('neither a string nor a sequence')
    tokens = []
    for t in listed:
        if not isinstance(t, str):
            refuse('%r is no token' % (t,))
        t = t.strip().lower()
        tokens.extend(VIEW_PRESETS.get(t, (t,)))
    if tokens in (['none'], ['id']):
        return None
    if not tokens or tokens[0] != 'id':
        refuse('the first view must be id')
    if len(tokens) > MAX_VIEWS:
        refuse('%d views, at most %d' % (len(tokens), MAX_VIEWS))
    forward, back, seen = [], [], set()
    for t in tokens:
        try:
            F, B = view_matrices(t, OH, OW)
        except ValueError as e:
            refuse(str(e))
        key = t if t in EXACT_VIEWS else float(t[3:])
        if key in seen:
            refuse('view %r is listed twice' % (t,))
        seen.add(key)
        if t in TRANSPOSING_VIEWS and OH != OW:
            refuse('view %r needs a square input' % (t,))
        forward.append(F)
        back.append(B)
    return Views(tuple(tokens), np.asarray(forward, np.float64), np.asarray(back, np.float64))


def views_in(images, views):
    """images: per modality a container [N,OH,OW,1] on the device -> per modality [V*N,OH,OW,1], view-major: every modality under the
    same views (ops.augment_gather with F, order 1, edge repeated).  The exact views are permutations of the input, bit for bit."""
    N, OH, OW = (int(n) for n in images[0].shape[:3])
    V = len(views.tokens)
    if V * N > 65535 or max(V * x.numel() for x in images) * 4 >= 2 ** 31:
        raise ValueError('tta (--predict_tta): %d views of %d slices of %d x %d make %d containers: at most 65535, of less than 2^31 '
                         'bytes together, go through the network at once' % (V, N, OH, OW, V * N))
    device = images[0].device
    rows = nn.host_to_device(np.tile(np.arange(N), V), device, np.int32)
    mats = nn.host_to_device(np.repeat(views.forward, N, axis=0), device, np.float64)
    return [ops.augment_gather(ops._c(x), rows, mats, None, 1, 'nearest') for x in images]


CrfParams, CRF_DEFAULTS = ops.CrfParams, ops.CRF_DEFAULTS


def check_crf(spec):
    """spec: None or 'none' (off) -> None; 'default' -> CRF_DEFAULTS; 'key=value,...' with the keys of CrfParams (radius, iterations, w_a,
    theta_alpha, theta_beta, w_s, theta_gamma) -> the defaults with those values; a CrfParams or a sequence in its order -> itself.  The
    result is within the limits of ops.crf_refine (ops.crf_params).  The defaults are starting values that nobody has tuned:
    tools/crf_sweep.py scores a grid of settings on a labelled folder."""
    what = 'crf (--predict_crf)'

    def refuse(why):
        raise ValueError("%s must be 'none', 'default' or key=value,... over the defaults (%s), got %r: %s"
                         % (what, ', '.join('%s=%g' % kv for kv in CRF_DEFAULTS._asdict().items()), spec, why))
    if spec is None:
        return None
    if not isinstance(spec, str):
        if isinstance(spec, (bool, int, float, dict)):
            refuse('neither a string nor a sequence of the seven parameters')
        return ops.crf_params(spec, what)
    text = spec.strip().lower()
    if text == 'none':
        return None
    values = CRF_DEFAULTS._asdict()
    if text != 'default':
        seen = set()
        for item in text.split(','):
            key, eq, value = (s.strip() for s in item.partition('='))
            if not eq or key not in values:
                refuse('%r is no key=value of these' % (item,))
            if key in seen:
                refuse('%s is given twice' % key)
            seen.add(key)
            try:
                values[key] = int(value) if key in ('radius', 'iterations') else float(value)
            except ValueError:
                refuse('%r is no %s' % (value, 'whole number' if key in ('radius', 'iterations') else 'number'))
    return ops.crf_params(CrfParams(**values), what)


_fill_holes, _smooth = fill_holes, smooth          # for score_folder and VolumePredictor.run, whose keywords carry the functions' names


def _write_table(path, rows, names, num_masks, fmt, union_first):
    """rows: (volume, one row of len(names) values per organ, then with union_first the union's) -> Vol, [names,] names of organ 0, ..."""
    cols = ['Vol'] + list(names if union_first else ()) + ['%s%d' % (name, k) for k in range(num_masks) for name in names]
    with open(path, 'w') as f:
        f.write(', '.join(cols) + '\n')
        for vol, table in rows:
            table = np.asarray(table)
            if union_first:
                table = np.concatenate([table[-1:], table[:-1]], axis=0)
            f.write(', '.join([str(vol)] + [fmt % v for v in table.reshape(-1)]) + '\n')


def write_component_results(path, rows, num_masks):
    """rows: (volume, stats [K,3]) -> Vol, N0, Before0, Kept0, N1, ..."""
    _write_table(path, rows, ('N', 'Before', 'Kept'), num_masks, '%d', False)


def write_hole_results(path, rows, num_masks):
    """rows: (volume, stats [K,3]) -> Vol, N0, Before0, Added0, N1, ..."""
    _write_table(path, rows, ('N', 'Before', 'Added'), num_masks, '%d', False)


def write_smooth_results(path, rows, num_masks):
    """rows: (volume, stats [K,3]) -> Vol, Before0, Removed0, Added0, Before1, ..."""
    _write_table(path, rows, ('Before', 'Removed', 'Added'), num_masks, '%d', False)


def write_crf_results(path, rows, num_masks):
    """rows: (volume, stats [K,3]) -> Vol, Before0, Removed0, Added0, Before1, ..."""
    _write_table(path, rows, ('Before', 'Removed', 'Added'), num_masks, '%d', False)


def write_surface_results(path, rows, num_masks):
    """rows: (volume, [K+1,3] with the union last) -> Vol, RAVD, ASSD, MSSD, RAVD0, ASSD0, MSSD0, ...: the union first"""
    _write_table(path, rows, ('RAVD', 'ASSD', 'MSSD'), num_masks, '%.3f', True)


def write_robust_results(path, rows, num_masks):
    """rows: (volume, [K+1,2] with the union last) -> Vol, HD, NSD, HD0, NSD0, ...: the union first"""
    _write_table(path, rows, ('HD', 'NSD'), num_masks, '%.3f', True)


MAX_MEMBERS = 7          # further models beside the run folder's own
CALIBRATION_NAMES = ('ECE', 'MCE', 'Brier', 'NLL', 'N')


def check_calibration_bins(bins):
    if isinstance(bins, bool) or not isinstance(bins, (int, np.integer)) or not 2 <= int(bins) <= ops.MAX_CALIBRATION_BINS:
        raise ValueError('calibration_bins (--predict_calibration_bins) must be a whole number in [2, %d], got %r'
                         % (ops.MAX_CALIBRATION_BINS, bins))
    return int(bins)


def calibration_scores(counts, sums):
    """counts [K,B,2] = (n, positives) and sums [K,B+2] of ops.calibration_table (host arrays) -> [K,5] = ECE, MCE, Brier, NLL, n per
    organ: over the bins that hold a pixel, gap_b = |positives_b / n_b - (sum of p)_b / n_b|; ECE = sum of n_b / n * gap_b, MCE = the
    largest gap; Brier and NLL are their sums over n.  An organ without a pixel inside the window gets nan."""
    counts, sums = np.asarray(counts, np.float64), np.asarray(sums, np.float64)
    K, B = counts.shape[:2]
    out = np.full((K, 5), np.nan)
    for k in range(K):
        n_b, positives = counts[k, :, 0], counts[k, :, 1]
        n = n_b.sum()
        out[k, 4] = n
        if n > 0:
            held = n_b > 0
            gap = np.abs(positives[held] / n_b[held] - sums[k, :B][held] / n_b[held])
            out[k, :4] = np.sum(n_b[held] / n * gap), gap.max(), sums[k, B] / n, sums[k, B + 1] / n
    return out


def uncertainty_means(table):
    """table [2,3] int64 of ops.uncertainty_by_error on (entropy, mutual information) -> [2,3] = (pixels, mean H, mean I) over the correctly
    and over the wrongly labelled pixels; the means are nan where there is no such pixel"""
    t = np.asarray(table, np.float64)
    with np.errstate(invalid='ignore', divide='ignore'):
        return np.concatenate([t[:, :1], t[:, 1:] / (255.0 * t[:, :1])], axis=1)


def write_calibration_results(path, rows, num_masks):
    """rows: (volume, [K,5]) -> Vol, ECE0, MCE0, Brier0, NLL0, N0, ECE1, ..."""
    with open(path, 'w') as f:
        f.write(', '.join(['Vol'] + ['%s%d' % (name, k) for k in range(num_masks) for name in CALIBRATION_NAMES]) + '\n')
        for vol, table in rows:
            f.write(', '.join([str(vol)] + ['%.6f, %.6f, %.6f, %.6f, %d' % (r[0], r[1], r[2], r[3], int(r[4])) for r in table]) + '\n')


def write_uncertainty_results(path, rows, num_masks):
    """rows: (volume, [2,3]) -> Vol, NCorrect, EntropyCorrect, MICorrect, NWrong, EntropyWrong, MIWrong"""
    with open(path, 'w') as f:
        f.write(', '.join(['Vol'] + [name + which for which in ('Correct', 'Wrong') for name in ('N', 'Entropy', 'MI')]) + '\n')
        for vol, table in rows:
            f.write(', '.join([str(vol)] + ['%d, %.6f, %.6f' % (int(r[0]), r[1], r[2]) for r in table]) + '\n')


def write_reliability(path, counts, sums):
    """counts [K,B,2] and sums [K,B+2] summed over the volumes -> Organ, Bin, Lo, Hi, N, Confidence, Frequency (nan in an empty bin)"""
    K, B = counts.shape[:2]
    with open(path, 'w') as f:
        f.write('Organ, Bin, Lo, Hi, N, Confidence, Frequency\n')
        for k in range(K):
            for b in range(B):
                n = int(counts[k, b, 0])
                conf, freq = (sums[k, b] / n, counts[k, b, 1] / float(n)) if n else (float('nan'), float('nan'))
                f.write('%d, %d, %.6f, %.6f, %d, %.6f, %.6f\n' % (k, b, b / float(B), (b + 1) / float(B), n, conf, freq))


class ScoreSheet(object):
    """the rows of one run's results_<kind>_<modality>.csv files: rows[kind][m] holds those of modality m; `scores` is score_volume's"""
    WRITERS = (('native', write_results), ('surface', write_surface_results), ('robust', write_robust_results),
               ('components', write_component_results), ('holes', write_hole_results), ('smooth', write_smooth_results),
               ('crf', write_crf_results), ('calibration', write_calibration_results), ('uncertainty', write_uncertainty_results))

    def __init__(self, modalities, num_masks, in_mm):
        self.modalities, self.num_masks, self.in_mm = list(modalities), num_masks, in_mm
        self.rows = {kind: [[] for _ in self.modalities] for kind, _ in self.WRITERS}
        self.reliability = {}          # modality index -> (counts, sums) of the calibration tables, summed over the volumes

    def add(self, m, volume, scores, geometry):
        modality, (joint, per_organ, in_mm, robust) = self.modalities[m], scores
        self.rows['native'][m].append((volume, joint, per_organ))
        log.info('volume %s, %s: Dice on the raw grid %.3f' % (volume, modality, joint))
        if in_mm is not None:
            self.rows['surface'][m].append((volume, in_mm))
            log.info('volume %s, %s: RAVD %.3f %%, ASSD %.3f mm, MSSD %.3f mm' % ((volume, modality) + tuple(in_mm[-1])))
        if robust is not None:
            self.rows['robust'][m].append((volume, robust))
            log.info('volume %s, %s: HD %.3f mm, NSD %.3f' % ((volume, modality) + tuple(robust[-1])))
        if geometry.get('slice_spacing') is None and self.in_mm:          # scores in mm were asked for
            log.info("volume %s, %s: %s holds no 'slice_spacing', so no scores in mm" % (volume, modality, geometry['file']))

    def add_components(self, m, volume, stats):
        self.rows['components'][m].append((volume, nn.to_numpy(stats)))

    def add_holes(self, m, volume, stats):
        self.rows['holes'][m].append((volume, nn.to_numpy(stats)))

    def add_smooth(self, m, volume, stats):
        self.rows['smooth'][m].append((volume, nn.to_numpy(stats)))

    def add_crf(self, m, volume, counts):
        """counts [S,K,3] of ops.label_overlap(labels of the refined map, labels of the map before): per organ the voxels before the
        refinement, those it removed and those it added"""
        after, before, both = nn.to_numpy(counts).astype(np.int64).sum(axis=0).T
        self.rows['crf'][m].append((volume, np.stack([before, before - both, after - both], axis=1)))

    def add_calibration(self, m, volume, counts, sums):
        """the table of ops.calibration_table, on the host: a row of scores, and the table is added to the modality's reliability table"""
        counts, sums = np.asarray(counts, np.int64), np.asarray(sums, np.float64)
        self.rows['calibration'][m].append((volume, calibration_scores(counts, sums)))
        held = self.reliability.get(m)
        self.reliability[m] = (counts, sums) if held is None else (held[0] + counts, held[1] + sums)

    def add_uncertainty(self, m, volume, table):
        self.rows['uncertainty'][m].append((volume, uncertainty_means(nn.to_numpy(table))))

    def write(self, out_folder):
        """one file per kind and modality that has rows"""
        for m, (counts, sums) in sorted(self.reliability.items()):
            write_reliability(os.path.join(out_folder, 'reliability_%s.csv' % self.modalities[m]), counts, sums)
        for kind, writer in self.WRITERS:
            for m, name in enumerate(self.modalities):
                if self.rows[kind][m]:
                    writer(os.path.join(out_folder, 'results_%s_%s.csv' % (kind, name)), self.rows[kind][m], self.num_masks)

    def by_name(self, kind):
        return {name: self.rows[kind][m] for m, name in enumerate(self.modalities)}


def score_folder(pred_folder, data_folder, out_folder=None, surface=True, components=None, connectivity=6, robust=None,
                 fill_holes=None, smooth=None, smooth_radius=None, smooth_extent='2d'):
    """Score label volumes written earlier (by VolumePredictor.run or by another program: <file name of the input>.npz with `label`
    [S_file,H,W] uint8) against the labelled files of `data_folder`; writes the CSV files of VolumePredictor.run into out_folder
    (default: pred_folder).  Volumes in the order of pred_folder/predictions.json where there is one, else of dataset.json.
    components='largest' filters every volume first (keep_largest), fill_holes='2d' | '3d' then fills the enclosed holes of every
    organ (fill_holes): the scores that post-processing would give.  smooth='open' | 'close' | 'smooth' with smooth_radius in mm (and
    smooth_extent) comes before both, as in VolumePredictor.run.
    robust=(percentile, tolerance in mm) also writes results_robust_<modality>.csv, and a third dictionary with its rows is returned."""
    check_components(components, connectivity)
    check_fill_holes(fill_holes)
    smooth_radius = check_smooth(smooth, smooth_radius, smooth_extent)
    robust = check_robust(robust)
    loader = VolumeFolderLoader(data_folder)
    out_folder = out_folder or pred_folder
    os.makedirs(out_folder, exist_ok=True)
    volumes = list(loader.manifest['volumes'])
    settings = os.path.join(pred_folder, 'predictions.json')
    if os.path.isfile(settings):
        with open(settings) as f:
            listed = [str(e['volume']) for e in json.load(f)['files'].values()]
        volumes = [v for i, v in enumerate(listed) if v not in listed[:i] and v in loader.manifest['volumes']]
    device = nn.default_device()
    values = nn.host_to_device(np.asarray(loader.label_values), device, np.int32)
    sheet = ScoreSheet(loader.modalities, loader.num_masks, surface or robust is not None)
    for v in volumes:
        for m, mod in enumerate(loader.modalities):
            entry = loader.manifest['volumes'][v][mod]
            path = os.path.join(pred_folder, entry['file'])
            if not os.path.isfile(path):
                continue
            image, label, res, selected, spacing = loader._read_file(v, mod, False)
            if label is None:
                continue
            with np.load(path) as z:
                pred = z['label']
            if pred.shape != label.shape or pred.dtype != np.uint8:
                raise ValueError('%s: expected label %s uint8 (the grid of %s), got %s %s'
                                 % (path, label.shape, entry['file'], pred.shape, pred.dtype))
            selected = np.arange(label.shape[0]) if selected is None else selected
            geo = dict(file=entry['file'], raw_shape=label.shape, slices=[int(i) for i in selected], resolution=res, slice_spacing=spacing)
            pred = nn.host_to_device(np.ascontiguousarray(pred[selected]), device, np.uint8)
            if smooth:
                pred, _ = _smooth(pred, values, geo, smooth, smooth_radius, smooth_extent)
            if components:
                pred, _ = keep_largest(pred, values, geo, connectivity)
            if fill_holes:
                pred, _ = _fill_holes(pred, values, geo, fill_holes)
            scores = score_volume(pred, nn.host_to_device(np.ascontiguousarray(label[selected]), device, np.uint8), values, geo, surface,
                                  robust)
            sheet.add(m, v, scores, geo)
    sheet.write(out_folder)
    return tuple(sheet.by_name(kind) for kind in (('native', 'surface') if robust is None else ('native', 'surface', 'robust')))


class VolumePredictor(object):
    def __init__(self, model, conf, members=None):
        """members: further models that predict together with `model` (an ensemble; at most MAX_MEMBERS), built for the same
        modalities, input_shape and organs"""
        self.model, self.conf = model, conf
        self.members = list(members or ())
        if len(self.members) > MAX_MEMBERS:
            raise ValueError('members (--predict_ensemble): %d further models, at most %d' % (len(self.members), MAX_MEMBERS))
        for member in self.members:
            if len(member.modalities) != len(model.modalities):
                raise ValueError('members (--predict_ensemble): a member is built for %d modalities, the model for %d'
                                 % (len(member.modalities), len(model.modalities)))

    def predict_volume(self, modality_index, mode, images, model=None):
        """predict_mask of `model` (default: the run folder's) over the slices of one volume in batches of conf.batch_size: device tensors
        in, one device tensor out"""
        model = self.model if model is None else model
        S = images[0].shape[0]
        step = max(1, int(self.conf.get('batch_size', S) or S))
        parts = [model.predict_mask(modality_index, mode, [x[i:i + step] for x in images]) for i in range(0, S, step)]
        parts = [p if isinstance(p, torch.Tensor) else nn.host_to_device(p, images[0].device) for p in parts]
        return parts[0] if len(parts) == 1 else torch.cat(parts, dim=0)

    def predict_views(self, modality_index, mode, images, views):
        """the merged probability map [N,OH,OW,K] of the N slices of `images` (per modality a container [N,OH,OW,1]): every slice is
        shown to the network under each of the V views (views_in; all modalities alike), predict_volume runs over the V*N slices, and
        ops.merge_views brings every view's map back and averages them.  views: check_tta's."""
        N = int(images[0].shape[0])
        prob = self.predict_volume(modality_index, mode, views_in(images, views))
        if prob.numel() * 4 >= 2 ** 31:
            raise ValueError('tta (--predict_tta): the maps of %d views of %d slices, %s, hold 2^31 bytes or more'
                             % (len(views.tokens), N, tuple(prob.shape)))
        return ops.merge_views(prob, views.back, N, int(self.conf.num_masks))

    def predict_members(self, modality_index, mode, images, views=None):
        """(mean map [N,OH,OW,K], planes [N,OH,OW,2] = (H, I)) of the N slices of `images` over the run folder's model and every member,
        in that order, each under every view of `views` (check_tta's; None: every slice once): one predict_volume and one
        ops.members_accumulate per model into one pair of buffers, then ops.members_finish."""
        N, K = int(images[0].shape[0]), int(self.conf.num_masks)
        shown = images if views is None else views_in(images, views)
        back = ops.IDENTITY_VIEW if views is None else views.back
        state = None
        for model in [self.model] + self.members:
            prob = self.predict_volume(modality_index, mode, shown, model)
            if prob.numel() * 4 >= 2 ** 31:
                raise ValueError('members (--predict_ensemble): the maps of %d views of %d slices, %s, hold 2^31 bytes or more'
                                 % (len(back), N, tuple(prob.shape)))
            state = ops.members_accumulate(prob, back, N, K, state)
        return ops.members_finish(state)

    def predict_tiled(self, loader, volume, m, mode, overlap, uploaded, views=None, crf=None, ensemble=False):
        """the blended probability map [S,RH,RW,K] of modality m on its whole resampled frame: the tiles are loaded
        (loader.load_volume_tiles), predicted as one batch of TR*TC*S slices and blended (ops.blend_tiles).  overlap = (rows, columns);
        uploaded: loader.upload_volume(volume).  With views (check_tta's) every tile is predicted under each view, turned about its own
        centre, and merged (predict_views) before the blend, which then sees the K organ channels alone.  With crf (check_crf's) every
        tile's map is refined against the tile's image of modality m (ops.crf_refine) before the blend, and the result is the pair
        (blend of the refined tiles, blend of the tiles as predicted).  With ensemble every tile's map is the members' mean
        (predict_members), and the blend of the tiles' planes (H, I) [S,RH,RW,2] is appended to whatever the call returns otherwise: an
        approximation, since the entropy of a blend is not the blend of the entropies."""
        images, geometry, plan = loader.load_volume_tiles(volume, m, overlap, uploaded)
        rows, cols = plan[m]
        OH, OW = loader.input_shape[:2]
        planes = None
        if ensemble:
            prob, planes = self.predict_members(m, mode, images, views)
        else:
            prob = self.predict_volume(m, mode, images) if views is None else self.predict_views(m, mode, images, views)
        S = images[m].shape[0] // (len(rows) * len(cols))

        def blend(p, channels=loader.num_masks):
            return ops.blend_tiles(p, rows, cols, tile_weights(rows, OH), tile_weights(cols, OW), S, geometry[m]['resampled'], channels)
        extra = () if planes is None else (blend(planes, 2),)
        if crf is None:
            return blend(prob) if planes is None else (blend(prob),) + extra
        return (blend(ops.crf_refine(prob, images[m], loader.num_masks, crf)), blend(prob)) + extra

    def run(self, folder, out_folder, volumes=None, mode='simple', order=1, surface=True, components=None, connectivity=6, robust=None,
            fill_holes=None, tiles=False, tile_overlap=None, tta=None, smooth=None, smooth_radius=None, smooth_extent='2d', crf=None,
            uncertainty=False, calibration_bins=10):
        crf = check_crf(crf)
        calibration_bins = check_calibration_bins(calibration_bins)
        ensemble = bool(self.members) or bool(uncertainty)          # off: the path below is the one without the option, launch for launch
        check_components(components, connectivity)
        check_fill_holes(fill_holes)
        smooth_radius = check_smooth(smooth, smooth_radius, smooth_extent)
        robust = check_robust(robust)
        if mode not in FUSION_MODES:
            raise ValueError('Unknown mode: %r (expected one of %s)' % (mode, ', '.join(FUSION_MODES)))
        if order not in (0, 1):
            raise ValueError('order must be 0 (nearest) or 1 (bilinear), got %r' % (order,))
        loader = VolumeFolderLoader(folder)
        if len(loader.modalities) != len(self.model.modalities):
            raise ValueError('%s holds %d modalities, the model is built for %d'
                             % (folder, len(loader.modalities), len(self.model.modalities)))
        if tuple(loader.input_shape[:2]) != tuple(self.conf.input_shape[:2]) or loader.num_masks != self.conf.num_masks:
            raise ValueError('%s is prepared for input_shape %s and %d organs, the model is built for %s and %d'
                             % (folder, loader.input_shape[:2], loader.num_masks, tuple(self.conf.input_shape[:2]),
                                self.conf.num_masks))
        overlap = check_tile_overlap(tile_overlap, loader.input_shape) if tiles else None
        views = check_tta(tta, loader.input_shape)
        volumes = list(loader.manifest['volumes']) if volumes is None else [str(v) for v in volumes]
        for v in volumes:
            if v not in loader.manifest['volumes']:
                raise ValueError('%s describes no volume %r' % (folder, v))
        os.makedirs(out_folder, exist_ok=True)
        device = nn.default_device()
        values = nn.host_to_device(np.asarray(loader.label_values), device, np.int32)
        sheet = ScoreSheet(loader.modalities, loader.num_masks, surface or robust is not None)
        files = {}
        for v in volumes:
            if tiles:
                uploaded = loader.upload_volume(v)
                images, geometry = None, uploaded[1]
            else:
                images, geometry = loader.load_volume_for_prediction(v)
            for m, geo in enumerate(geometry):
                origins = None
                if tiles:
                    rows, cols = loader.tile_plan(geometry, m, overlap)[m]
                    origins = dict(rows=[t[0] for t in rows], cols=[t[0] for t in cols])
                if tiles and len(rows) * len(cols) > 1:
                    RH, RW = geo['resampled']
                    window = ((RH, RW), (0, RH, 0), (0, RW, 0))
                    prob = self.predict_tiled(loader, v, m, mode, overlap, uploaded, views, crf, ensemble)
                    if ensemble:
                        prob, planes = (prob[0], prob[1]) if crf is None else (prob[:2], prob[2])
                    prob, unrefined = prob if crf is not None else (prob, None)
                else:          # one tile: the centre window of crop_pad_map, the path without the option
                    if images is None:
                        images, _ = loader.load_volume_for_prediction(v)
                    window = (geo['resampled'], geo['rows'], geo['cols'])
                    if ensemble:
                        prob, planes = self.predict_members(m, mode, images, views)
                    else:
                        prob = self.predict_volume(m, mode, images) if views is None else self.predict_views(m, mode, images, views)
                    if crf is not None:          # against the slices as the network saw them, unturned
                        prob, unrefined = ops.crf_refine(prob, images[m], loader.num_masks, crf), prob
                pred = ops.restore_label(prob, values, geo['raw_shape'][1:], window[0], window[1], window[2], order)
                if crf is not None:
                    before = ops.restore_label(unrefined, values, geo['raw_shape'][1:], window[0], window[1], window[2], order)
                    sheet.add_crf(m, v, ops.label_overlap(pred, before, values))
                if smooth:
                    pred, stats = _smooth(pred, values, geo, smooth, smooth_radius, smooth_extent)
                    sheet.add_smooth(m, v, stats)
                if components:
                    pred, stats = keep_largest(pred, values, geo, connectivity)
                    sheet.add_components(m, v, stats)
                if fill_holes:
                    pred, stats = _fill_holes(pred, values, geo, fill_holes)
                    sheet.add_holes(m, v, stats)
                truth = None if geo['label'] is None else nn.host_to_device(geo['label'], device, np.uint8)
                if truth is not None:
                    scores = score_volume(pred, truth, values, geo, surface, robust)
                    sheet.add(m, v, scores, geo)
                label = np.zeros(geo['raw_shape'], np.uint8)
                label[geo['slices']] = pred.cpu().numpy()
                extra = {} if geo['slice_spacing'] is None else dict(slice_spacing=float(geo['slice_spacing']))
                np.savez_compressed(os.path.join(out_folder, geo['file']), label=label, resolution=geo['resolution'], **extra)
                if ensemble:
                    levels = torch.stack([ops.restore_map(planes, u, geo['raw_shape'][1:], window[0], window[1], window[2], order)
                                          for u in (0, 1)])
                    if truth is not None:          # the map that the labels come from; the prediction after every filter
                        table = ops.calibration_table(prob, truth, values, window[0], window[1], window[2], calibration_bins, order)
                        sheet.add_calibration(m, v, nn.to_numpy(table[0]), nn.to_numpy(table[1]))
                        sheet.add_uncertainty(m, v, ops.uncertainty_by_error(pred, truth, levels))
                    on_grid = np.zeros((2,) + tuple(geo['raw_shape']), np.uint8)
                    on_grid[:, geo['slices']] = levels.cpu().numpy()
                    os.makedirs(os.path.join(out_folder, 'uncertainty'), exist_ok=True)
                    np.savez_compressed(os.path.join(out_folder, 'uncertainty', geo['file']), entropy=on_grid[0],
                                        mutual_information=on_grid[1], resolution=geo['resolution'], **extra)
                files[geo['file']] = dict(volume=v, modality=loader.modalities[m], slices=geo['slices'], **extra)
                if origins is not None:
                    files[geo['file']]['tile_origins'] = origins
        sheet.write(out_folder)
        settings = dict(source_folder=folder, mode=mode, order=order, model_folder=self.conf.get('folder'),
                        label_values=loader.label_values, files=files)
        if components:
            settings.update(components=components, connectivity=connectivity)
        if fill_holes:
            settings.update(fill_holes=fill_holes)
        if smooth:
            settings.update(smooth=smooth, smooth_radius=smooth_radius, smooth_extent=smooth_extent)
        if robust is not None:
            settings.update(percentile=robust[0], tolerance_mm=robust[1])
        if tiles:
            settings.update(tiles=True, tile_overlap=list(overlap))
        if views is not None:
            settings.update(tta=list(views.tokens))
        if crf is not None:
            settings.update(crf=dict(crf._asdict()))
        if ensemble:
            folders = [self.conf.get('folder')] + [(getattr(member, 'conf', None) or {}).get('folder') for member in self.members]
            settings.update(ensemble=folders, uncertainty=bool(uncertainty), calibration_bins=calibration_bins)
        with open(os.path.join(out_folder, 'predictions.json'), 'w') as f:
            json.dump(settings, f, indent=1)
        return sheet.by_name('native')
