"""Loader of volumes exported to a folder, with the surface of the reference's `Loader` (loaders/base_loader.py:10-89) and the
preprocessing of its CHAOS loader (loaders/chaos.py `_load_volume`, `resample`, `load_all_modalities_concatenated`), run on the
device (csrc/preprocess.hip).  Reading DICOM / PNG stays out of scope: a folder holds arrays ("Volume folders").

    <root>/dataset.json      settings only: name, modalities (2 or 3), label_values (one grey value per organ; everything else is
                             background, chaos.py:303-319), target_resolution [mm, mm], input_shape, splits (a list of
                             {training, validation, test} lists of volume ids, chaos.py:32-48) and
                             volumes: {"<id>": {"<modality>": {"file": "<name>.npz", "slices": [[start, stop], ...]}}}
    <root>/<name>.npz        image [S,H,W] (any integer or float dtype), label [S,H,W] uint8 grey values, resolution [2] mm per
                             pixel along rows and columns.  `label` may be missing in a folder that is only predicted on
                             (load_volume_for_prediction, volume_predictor.py); the training surface then refuses the file.
                             `slice_spacing` (optional): one positive float, mm between consecutive slices of the file.  The
                             scores in mm of volume_predictor.py and a 3-D `bias_field` use it; nothing else does.

`slices` (optional) lists [start, stop) ranges applied in order: how a user states which slices of the acquisitions show the same
anatomy (what chaos.py:110-240 hard-codes per subject).  After selection all modalities of a volume must hold the same number of
slices.  S, H, W and the resolution may differ between volumes and between modalities.

Per (volume, modality) the raw slices are uploaded once through pinned memory (`_upload`: the one way from a file to device slices,
for training, validation, testing, prediction, tiles and TTA alike) and three launches write the volume's share of the NHWC containers
[N,H,W,M] / [N,H,W,M*num_masks]; the host only decides the geometry (resampled size, crop / pad index map).

Four optional keys of dataset.json, the load-time stages, change what is loaded.  STAGES lists them with their registries, modes and
keys; check_stage validates a block of any of them, and effective_setting gives the one in force for a folder (a registry of
loaders.stage_conf overrides the key for a run).

`intensity` (optional key of dataset.json; build-defined) chooses how grey values reach [-1, 1].  Absent or {"mode": "minmax"}: every
slice by the extremes of its resampled frame, the reference's rule and the three launches above.  {"mode": "window", "scope":
"volume" | "slice", "percentiles": [lo, hi]} (defaults "volume", [0.5, 99.5]): clip to the two percentiles of the volume's (or the
slice's) resampled values and rescale.  {"mode": "landmarks", "percentiles": [...], "standard": {"<modality>": [y_0 .. y_K-1]}}
(default percentiles 1, 10, 20 .. 90, 99; per volume): Nyul and Udupa's standardisation, the volume's own landmarks mapped piecewise
linearly onto the scale that tools/fit_intensity_landmarks.py learned from the training volumes.  The percentiles are exact order
statistics selected on the device (ops.preprocess_quantiles, once per uploaded volume and modality: `intensity_knots`); the
definition is in include/mmseg_hip.h.  loaders.intensity_conf overrides the key for a run (experiment.py --intensity_norm).

`bias_field` (optional key of dataset.json; build-defined) removes coil shading before the grey values are normalised.  Absent or
{"mode": "off"}: the slices are used as exported.  {"mode": "n3", "sigma_mm": 40, "levels": 3, "iterations": 20, "extent": "3d" | "2d"}
(the defaults are untuned starting values; `extent` defaults to "3d" where a file holds `slice_spacing`, else "2d"): an N3 / N4-family
correction (ops.bias_correct; the rule is in include/mmseg_hip.h) of the selected raw slices, once per uploaded (volume, modality), in
`bias_corrected` -- before `intensity_knots`, so the percentiles are those of the corrected volume, and training, validation, testing,
prediction, tiles and TTA all see the same volume.  "3d" needs `slice_spacing` and one contiguous run of slices.
loaders.bias_conf overrides the key for a run (experiment.py --bias_correction).

`denoise` (optional key of dataset.json; build-defined) removes acquisition noise before all of the above.  Absent or {"mode": "off"}:
nothing is launched.  {"mode": "nlm", "sigma": "auto" | number | {modality: number}, "h": 1.0, "search_radius": 5, "patch_radius": 1,
"extent": "2d" | "3d", "search_radius_z": 0 | 1..4, "noise": "rician" | "gaussian"} (the defaults are untuned starting values; `extent`
defaults to "2d"): voxel-wise non-local means with in-plane patches (ops.nlm_denoise; the rule is in include/mmseg_hip.h) of the selected
raw slices, once per uploaded (volume, modality), in `denoised` -- immediately before `bias_corrected`, so the bias field, the percentiles
and everything after them see the denoised volume.  "3d" lets the search reach the neighbouring slices and needs one contiguous run of
slices.  `sigma` is in the file's raw grey values; "auto" estimates it per (volume, modality) on the device and runs high on small or busy
slices.  loaders.denoise_conf overrides the key for a run (experiment.py --denoise).

`align` (optional key of dataset.json; build-defined) pairs the modalities of a volume by themselves.  Absent or {"mode": "off"}: nothing is
launched, the pairing is the one `slices` states and the centre windows of the resampled frames.  {"mode": "mi", "reference": modality
(default the first), "max_shift_mm": 40, "max_slices": 4, "bins": 32, "levels": 3, "min_overlap": 0.5, "percentiles": [0.5, 99.5]} (the
defaults are untuned starting values): every other modality is translated against the reference -- a whole number of slices and of pixels
of target_resolution along rows and columns -- so that Studholme's normalised mutual information of the two quantised volumes is largest
(ops.align_volumes; the rule is in include/mmseg_hip.h), once per uploaded volume, in `alignment` -- after `bias_corrected` and before
`intensity_knots`.  The slices without a partner in every modality are dropped (so the modalities may hold different numbers of slices
after `slices`), a shifted modality reads a shifted window of its frame, images and labels alike, and the geometry record of a volume
carries the kept `slices`, the windows and `shift`, so the way back, the scores, tiles and TTA follow.  loaders.align_conf overrides the
key for a run (experiment.py --align).

For whole-slice prediction (volume_predictor.py `tiles=True`; build-defined) the host also plans the tiles of a
frame larger than input_shape (tile_axis, tile_weights, tiles_of_other) and `load_volume_tiles` writes them with the same kernels."""
import collections
import json
import logging
import os

import numpy as np
import torch

from .. import nn, ops
from .MultimodalPairedData import MultimodalPairedData
from .data import Data

log = logging.getLogger('volume_folder')

SPLIT_TYPES = ('training', 'validation', 'test', 'all')
MANIFEST = 'dataset.json'


def resampled_size(n, old_res, new_res):
    """np.round(n * scale), scale = old_res / new_res: skimage.transform.rescale's output extent (half to even)"""
    return int(np.round(n * (float(old_res) / float(new_res))))


def crop_pad_map(resampled, target):
    """(lo, kept, before) of utils/data_utils.crop_same(mode='equal', pad_mode='edge') along one axis: final index o reads
    resampled index lo + clamp(o - before, 0, kept - 1).  A surplus removes ceil(diff / 2) pixels from BOTH ends
    (data_utils._crop), so an odd surplus keeps target - 1 pixels and the last one is repeated (_pad: floor(1 / 2) = 0 before)."""
    r, n = int(resampled), int(target)
    if r > n:
        lo = int(np.ceil((r - n) / 2))
        if r - 2 * lo < 1:
            raise ValueError('cropping %d pixels to %d leaves nothing (%d are removed from both ends)' % (r, n, lo))
        return lo, r - 2 * lo, 0
    return 0, r, int((n - r) / 2)


MAX_TILES = ops.MAX_TILES          # per axis


def tile_window(start, resampled, target):
    """(lo, kept, before) of the window [start, start + target) of a frame of extent `resampled`, edge-padded where it leaves the frame
    (pad_mode='edge'): container index o reads frame index clamp(start + o, 0, resampled - 1).  It satisfies the contract of
    mmseg_preprocess_image: 0 <= lo, kept >= 1, lo + kept <= resampled, 0 <= before < target.  A window entirely outside the frame
    repeats the nearest edge pixel."""
    w, r, n = int(start), int(resampled), int(target)
    if w >= r:
        return r - 1, 1, 0
    if w + n <= 0:
        return 0, 1, 0
    lo = max(w, 0)
    return lo, min(w + n, r) - lo, max(-w, 0)


def centre_start(resampled, target):
    """signed start of crop_pad_map's centre window: lo when resampled > target, else -before"""
    r, n = int(resampled), int(target)
    return (r - n + 1) // 2 if r > n else -((n - r) // 2)


def tile_axis(resampled, target, overlap):
    """The tiles of one axis, a list of (lo, kept, before): one tile, crop_pad_map's padded one, when the frame fits the network's
    extent; else n = ceil((R - overlap) / (O - overlap)) full tiles (a_i, O, 0) with a_i = (i * (R - O)) // (n - 1), so that the first
    starts at 0, the last ends at R and neighbours share at least `overlap` pixels.  Integer arithmetic throughout."""
    r, n, ov = int(resampled), int(target), int(overlap)
    if r < 1 or n < 1 or not 0 <= ov < n:
        raise ValueError('tile_overlap must lie in [0, %d) for an extent of %d pixels (frame %d), got %d' % (n, n, r, ov))
    if r <= n:
        return [crop_pad_map(r, n)]
    count = -(-(r - ov) // (n - ov))
    if count > MAX_TILES:
        raise ValueError('a frame of %d pixels needs %d tiles of %d with tile_overlap %d (--predict_tile_overlap), more than the %d an '
                         'axis may have: lower the overlap' % (r, count, n, ov, MAX_TILES))
    return [((i * (r - n)) // (count - 1), n, 0) for i in range(count)]


def tile_weights(tiles, target):
    """fp32 [T, O], indexed by container index j: min(l, r) with l = j + 1 where the tile has a left neighbour, else O, and r = O - j
    where it has a right neighbour, else O.  Integers (exact in fp32), strictly positive, tapering towards a neighbour only."""
    n = int(target)
    j = np.arange(n)
    out = np.empty((len(tiles), n), np.float32)
    for i in range(len(tiles)):
        left = j + 1 if i > 0 else np.full(n, n)
        right = n - j if i < len(tiles) - 1 else np.full(n, n)
        out[i] = np.minimum(left, right)
    return out


def tiles_of_other(tiles, resampled, other_resampled, target, shift=0):
    """The windows of another modality (extent other_resampled) for the tiles planned on the predicted one (extent resampled): tile
    i, whose window starts at s_i = lo - before on the predicted frame, reads the other frame from s_i - c(R_m) + c(R_j) + shift, c =
    centre_start, so that the tile which coincides with the centre crop of one frame coincides with the centre crop of the other: the
    pairing the model was trained on.  shift: the `align` shift of the other modality minus that of the predicted one, in pixels."""
    shift = centre_start(other_resampled, target) - centre_start(resampled, target) + int(shift)
    return [tile_window(lo - before + shift, other_resampled, target) for lo, kept, before in tiles]


def has_data(name):
    """True when a folder is registered for data set `name` (loaders.data_conf)"""
    from . import data_conf
    return bool(name) and bool(data_conf.get(name))


INTENSITY_SCOPES = ('volume', 'slice')
WINDOW_PERCENTILES = (0.5, 99.5)                                        # nnU-Net's clip
LANDMARK_PERCENTILES = (1, 10, 20, 30, 40, 50, 60, 70, 80, 90, 99)      # Nyul and Udupa's deciles between the 1st and 99th
MAX_KNOTS = ops.PREPROCESS_MAX_KNOTS


def quantile_ranks(n, percentiles):
    """rank floor((n - 1) * (q / 100)) of every percentile q among n values, in fp64 in that order: numpy's method='lower'"""
    return [int(np.floor((int(n) - 1) * (float(q) / 100.0))) for q in percentiles]


def _intensity_block(block, modalities, where):
    """an `intensity` block of mode 'window' or 'landmarks': mode, scope and percentiles, and for 'landmarks' additionally `standard`
    {modality: [y_0 .. y_{K-1}]}"""
    mode = block['mode']
    scope = block.get('scope', 'volume')
    if scope not in INTENSITY_SCOPES:
        raise ValueError('%s: "intensity" scope must be one of %s, got %r' % (where, ', '.join(INTENSITY_SCOPES), scope))
    q = block.get('percentiles', WINDOW_PERCENTILES if mode == 'window' else LANDMARK_PERCENTILES)
    if (not isinstance(q, (list, tuple)) or any(isinstance(v, bool) or not isinstance(v, (int, float)) for v in q)
            or any(not np.isfinite(v) or not 0 <= v <= 100 for v in q)):
        raise ValueError('%s: "intensity" percentiles must be a list of numbers in [0, 100], got %r' % (where, q))
    if mode == 'window' and len(q) != 2:
        raise ValueError('%s: "intensity" mode window takes two percentiles [lo, hi], got %r' % (where, q))
    if not 2 <= len(q) <= MAX_KNOTS:
        raise ValueError('%s: "intensity" takes 2..%d percentiles, got %d' % (where, MAX_KNOTS, len(q)))
    if any(b <= a for a, b in zip(q[:-1], q[1:])):
        raise ValueError('%s: "intensity" percentiles must increase strictly, got %r' % (where, q))
    out = {'mode': mode, 'scope': scope, 'percentiles': [float(v) for v in q]}
    if mode == 'window':
        if 'standard' in block:
            raise ValueError('%s: "intensity" mode window takes no "standard" scale (its targets are -1 and 1)' % where)
        return out
    if scope != 'volume':
        raise ValueError('%s: "intensity" mode landmarks works per volume; scope %r is not available' % (where, scope))
    std = block.get('standard')
    if not isinstance(std, dict):
        raise ValueError('%s: "intensity" mode landmarks needs "standard": {modality: scale} (tools/fit_intensity_landmarks.py '
                         'writes it)' % where)
    out['standard'] = {}
    for mod in modalities:
        y = std.get(mod)
        if not isinstance(y, (list, tuple)) or len(y) != len(q):
            raise ValueError('%s: "intensity" standard scale of modality %r must hold %d values, one per percentile, got %r'
                             % (where, mod, len(q), y))
        y = [float(v) for v in y]
        if y[0] != -1.0 or y[-1] != 1.0:
            raise ValueError('%s: "intensity" standard scale of modality %r must begin with -1 and end with 1, got %r' % (where, mod, y))
        if any(b < a for a, b in zip(y[:-1], y[1:])):
            raise ValueError('%s: "intensity" standard scale of modality %r must not decrease, got %r' % (where, mod, y))
        out['standard'][mod] = y
    return out


def _bias_block(block, modalities, where):
    """a `bias_field` block of mode 'n3': 'sigma_mm', 'levels', 'iterations' and 'extent' with ops.BIAS_DEFAULTS filled in -- except
    `extent`, which stays None when the block names none: the loader takes '3d' where the files hold a slice_spacing, else '2d'"""
    given = {k: v for k, v in block.items() if k != 'mode' and not (k == 'extent' and v is None)}
    p = ops.bias_params(given, '%s: "bias_field"' % where)
    if 'extent' not in given:
        p['extent'] = None
    return dict(mode='n3', **p)


def _denoise_block(block, modalities, where):
    """a `denoise` block of mode 'nlm': 'sigma', 'h', 'search_radius', 'patch_radius', 'search_radius_z', 'extent' and 'noise' with
    ops.NLM_DEFAULTS filled in.  `sigma` is 'auto', a number or {modality: number}; a mapping must name every modality of `modalities`
    (None: the folder is not known yet, as for a command-line override)."""
    given = {k: v for k, v in block.items() if k != 'mode' and not (k == 'search_radius_z' and v is None)}
    per_modality = given.get('sigma') if isinstance(given.get('sigma'), dict) else None
    if per_modality is not None:
        del given['sigma']
        for mod, s in sorted(per_modality.items()):
            ops.nlm_params({'sigma': s}, '%s: "denoise" (modality %r)' % (where, mod))
            if s == 'auto':
                raise ValueError('%s: "denoise" sigma of modality %r must be a number; "auto" goes in place of the mapping' % (where, mod))
        if modalities is not None:
            missing = [mod for mod in modalities if mod not in per_modality]
            if missing:
                raise ValueError('%s: "denoise" sigma names no value for modality %s (a mapping must name every one of %s)'
                                 % (where, ', '.join(repr(mod) for mod in missing), ', '.join(modalities)))
            extra = sorted(set(per_modality) - set(modalities))
            if extra:
                raise ValueError('%s: "denoise" sigma names %s, which is no modality of the folder (%s)'
                                 % (where, ', '.join(repr(mod) for mod in extra), ', '.join(modalities)))
    p = ops.nlm_params(given, '%s: "denoise"' % where)
    if per_modality is not None:
        p['sigma'] = {str(mod): float(s) for mod, s in per_modality.items()}
    return dict(mode='nlm', **p)


def _align_block(block, modalities, where):
    """an `align` block of mode 'mi': 'reference', 'max_shift_mm', 'max_slices', 'bins', 'levels', 'min_overlap' and 'percentiles' with
    ops.ALIGN_DEFAULTS filled in.  `reference` is a modality's name; None stands for the folder's first (a command-line override may
    not know the folder yet: modalities = None)."""
    reference = block.get('reference')
    if reference is not None and (not isinstance(reference, str) or (modalities is not None and reference not in modalities)):
        raise ValueError('%s: "align" reference must be one of the modalities%s, got %r'
                         % (where, '' if modalities is None else ' (%s)' % ', '.join(modalities), reference))
    if reference is None and modalities is not None:
        reference = modalities[0]
    p = ops.align_params({k: v for k, v in block.items() if k not in ('mode', 'reference')}, '%s: "align"' % where)
    return dict(mode='mi', reference=reference, **p)


Stage = collections.namedtuple('Stage', 'key registry off modes keys validate')

# The load-time stages, in the order experiment.py registers and records them.  key: the key of dataset.json, of the configuration and of
# the loader's attribute; registry: the override's name in loaders (loaders.stage_conf[key] is the dict); off: the block that None and {}
# stand for (the first of `modes`), which takes no other key; keys: what a block may hold beside `mode`; validate(block, modalities,
# where): the normalised form of a block of any other mode.
STAGES = collections.OrderedDict((stage.key, stage) for stage in (
    Stage('intensity', 'intensity_conf', {'mode': 'minmax'}, ('minmax', 'window', 'landmarks'), ('scope', 'percentiles', 'standard'),
          _intensity_block),
    Stage('bias_field', 'bias_conf', {'mode': 'off'}, ('off', 'n3'), ('sigma_mm', 'levels', 'iterations', 'extent'), _bias_block),
    Stage('denoise', 'denoise_conf', {'mode': 'off'}, ('off', 'nlm'), tuple(ops.NLM_DEFAULTS), _denoise_block),
    Stage('align', 'align_conf', {'mode': 'off'}, ('off', 'mi'), ('reference',) + tuple(ops.ALIGN_DEFAULTS), _align_block)))


def check_stage(key, block, modalities, where):
    """The normalised form of the block of stage `key` (dataset.json, conf.<key>, loaders.stage_conf[key]): the stage's `off` block, or
    what its validator makes of a block of another mode, defaults filled in.  None and {} mean off."""
    stage = STAGES[key]
    off = stage.off['mode']
    if block is None:
        return dict(stage.off)
    if not isinstance(block, dict):
        raise ValueError('%s: "%s" must be an object, got %r' % (where, key, block))
    mode = block.get('mode', off)
    if mode not in stage.modes:
        raise ValueError('%s: "%s" mode must be one of %s, got %r' % (where, key, ', '.join(stage.modes), mode))
    unknown = sorted(set(block) - {'mode'} - set(stage.keys))
    if unknown:
        raise ValueError('%s: "%s" has unknown key(s) %s' % (where, key, ', '.join(unknown)))
    if mode == off:
        if set(block) - {'mode'}:
            raise ValueError('%s: "%s" mode %s takes no other key, got %s' % (where, key, off, ', '.join(sorted(set(block) - {'mode'}))))
        return dict(stage.off)
    return stage.validate(block, modalities, where)


def check_intensity(block, modalities, where):
    return check_stage('intensity', block, modalities, where)


def check_bias(block, where):
    return check_stage('bias_field', block, None, where)


def check_denoise(block, modalities, where):
    return check_stage('denoise', block, modalities, where)


def check_align(block, modalities, where):
    return check_stage('align', block, modalities, where)


def effective_setting(root, key, manifest=None):
    """the normalised setting of stage `key` for the folder `root`: the override registered in the stage's registry under a data set
    name that loaders.data_conf maps to this folder, or under the folder's own `name`; else its dataset.json's"""
    from . import data_conf, stage_conf
    m = read_manifest(root) if manifest is None else manifest
    here = os.path.abspath(root)
    names = [n for n, f in data_conf.items() if f and os.path.abspath(f) == here] + [m['name']]
    for n in names:
        if stage_conf[key].get(n) is not None:
            return check_stage(key, stage_conf[key][n], m['modalities'], 'loaders.%s[%r]' % (STAGES[key].registry, n))
    return check_stage(key, m.get(key), m['modalities'], os.path.join(root, MANIFEST))


def read_manifest(root):
    path = os.path.join(root, MANIFEST)
    if not os.path.isfile(path):
        raise FileNotFoundError('%s: no %s (see INTEGRATION.md, "Volume folders")' % (root, MANIFEST))
    with open(path) as f:
        m = json.load(f)
    for key in ('name', 'modalities', 'label_values', 'target_resolution', 'input_shape', 'splits', 'volumes'):
        if key not in m:
            raise ValueError('%s: missing key %r' % (path, key))
    if len(m['modalities']) not in (2, 3) or len(set(m['modalities'])) != len(m['modalities']):
        raise ValueError('%s: "modalities" must list 2 or 3 distinct names, got %r' % (path, m['modalities']))
    if not m['label_values'] or len(m['label_values']) > 16 or any(not 0 <= int(v) <= 255 for v in m['label_values']):
        raise ValueError('%s: "label_values" must hold 1..16 grey values in 0..255, got %r' % (path, m['label_values']))
    if len(m['target_resolution']) != 2 or min(m['target_resolution']) <= 0:
        raise ValueError('%s: "target_resolution" must be two positive numbers, got %r' % (path, m['target_resolution']))
    if len(m['input_shape']) not in (2, 3) or min(m['input_shape'][:2]) < 1:
        raise ValueError('%s: "input_shape" must be [H, W] or [H, W, 1], got %r' % (path, m['input_shape']))
    if not isinstance(m['splits'], list) or not m['splits']:
        raise ValueError('%s: "splits" must be a non-empty list' % path)
    for i, s in enumerate(m['splits']):
        for t in SPLIT_TYPES[:3]:
            if t not in s:
                raise ValueError('%s: split %d has no %r list' % (path, i, t))
            for v in s[t]:
                if str(v) not in m['volumes']:
                    raise ValueError('%s: split %d (%s) names volume %r, which "volumes" does not describe' % (path, i, t, v))
    for v, entry in m['volumes'].items():
        for mod in m['modalities']:
            if mod not in entry or 'file' not in entry[mod]:
                raise ValueError('%s: volume %s has no file for modality %r' % (path, v, mod))
    for key in STAGES:
        check_stage(key, m.get(key), m['modalities'], path)
    return m


class VolumeFolderLoader(object):
    def __init__(self, root):
        self.data_folder = root
        self.manifest = m = read_manifest(root)
        self.name = m['name']
        self.modalities = list(m['modalities'])
        self.label_values = [int(v) for v in m['label_values']]
        self.num_masks = len(self.label_values)
        self.target_resolution = (float(m['target_resolution'][0]), float(m['target_resolution'][1]))
        self.input_shape = (int(m['input_shape'][0]), int(m['input_shape'][1]), 1)
        self.volumes = sorted(set(v for s in m['splits'] for t in SPLIT_TYPES[:3] for v in s[t]))
        self.num_volumes = len(self.volumes)
        self.processed_folder = None
        self.log = log
        for key in STAGES:          # build-defined: self.intensity, .bias_field, .denoise, .align; a stage's `off` block is the reference's loading
            setattr(self, key, effective_setting(root, key, m))
        self._alignments = {}                                  # volume -> alignment()'s result

    # ---- splits (base_loader.py:27-32,80-89) --------------------------------------------------------------------------------
    def splits(self):
        return [{t: list(s[t]) for t in SPLIT_TYPES[:3]} for s in self.manifest['splits']]

    def get_volumes_for_split(self, split, split_type):
        if split_type not in SPLIT_TYPES:
            raise ValueError('Unknown split_type: %r (expected one of %s)' % (split_type, ', '.join(SPLIT_TYPES)))
        all_splits = self.splits()
        if not 0 <= int(split) < len(all_splits):
            raise ValueError('%s defines %d split(s), got split %r' % (self.data_folder, len(all_splits), split))
        s = all_splits[int(split)]
        if split_type == 'all':
            return sorted(s['training'] + s['validation'] + s['test'])
        return s[split_type]

    # ---- files --------------------------------------------------------------------------------------------------------------
    def read_volume(self, volume, modality, require_label=True):
        """raw (image [S,H,W], label [S,H,W] uint8, resolution (2,)) of one volume and modality, `slices` applied.  With
        require_label=False a file without a `label` array yields label = None (a scan to be segmented)."""
        image, label, res, selected, _ = self._read_file(volume, modality, require_label)
        if selected is not None:
            image = image[selected]
            label = None if label is None else label[selected]
        return image, label, res

    def _read_file(self, volume, modality, require_label):
        """the arrays as stored (all slices of the file), the indices that `slices` selects, in order (None: every slice), and the
        file's `slice_spacing` in mm (None when the file holds none)"""
        entry = self.manifest['volumes'][str(volume)][modality]
        path = os.path.join(self.data_folder, entry['file'])
        if not os.path.isfile(path):
            raise FileNotFoundError('volume %s, modality %s: %s does not exist' % (volume, modality, path))
        with np.load(path) as z:
            for key in ('image', 'label', 'resolution'):
                if key not in z.files and (require_label or key != 'label'):
                    raise ValueError('%s: no array %r' % (path, key))
            image, res = z['image'], np.asarray(z['resolution'], np.float64).reshape(-1)
            label = z['label'] if 'label' in z.files else None
            spacing = np.asarray(z['slice_spacing'], np.float64).reshape(-1) if 'slice_spacing' in z.files else None
        if spacing is not None:
            if spacing.shape != (1,) or not np.isfinite(spacing[0]) or spacing[0] <= 0:
                raise ValueError('%s: slice_spacing must be one finite number > 0 (mm between consecutive slices), got %s' % (path, spacing))
            spacing = float(spacing[0])
        if (image.ndim != 3 or res.shape != (2,) or res.min() <= 0
                or (label is not None and (label.shape != image.shape or label.dtype != np.uint8))):
            raise ValueError('%s: expected image [S,H,W], label [S,H,W] uint8 and resolution [2] > 0, got %s %s, %s %s, %s'
                             % (path, image.shape, image.dtype, getattr(label, 'shape', None), getattr(label, 'dtype', None), res))
        ranges = entry.get('slices')
        selected = None
        if ranges is not None:
            for a, b in ranges:
                if not 0 <= a < b <= image.shape[0]:
                    raise ValueError('volume %s, modality %s: slice range [%d, %d) outside the %d slices of %s'
                                     % (volume, modality, a, b, image.shape[0], path))
            selected = np.concatenate([np.arange(a, b) for a, b in ranges])
        return image, label, res, selected, spacing

    def geometry(self, H, W, res):
        """(RH, RW), rows, cols: the resampled extent of an H x W slice at `res` mm and its crop / pad index maps to input_shape"""
        RH = resampled_size(H, res[0], self.target_resolution[0])
        RW = resampled_size(W, res[1], self.target_resolution[1])
        if RH < 1 or RW < 1:
            raise ValueError('a %d x %d slice at %s mm resamples to nothing at %s mm' % (H, W, res, self.target_resolution))
        return (RH, RW), crop_pad_map(RH, self.input_shape[0]), crop_pad_map(RW, self.input_shape[1])

    def intensity_knots(self, x, resampled, modality):
        """The normalisation of one (volume, modality) whose raw slices x [S,H,W] are on the device: None for 'minmax' (the kernels
        rescale every slice by its extremes), else (knots [G,K], targets [K]) for ops.preprocess_images / preprocess_volume -- the
        ranks of the configured percentiles among the resampled values of a slice or of the volume, and their order statistics,
        selected on the device (ops.preprocess_quantiles).  The one place where this is decided: training, validation, testing,
        prediction and tiles call it once per uploaded (volume, modality)."""
        setting = self.intensity
        if setting['mode'] == 'minmax':
            return None
        per_volume = setting['scope'] == 'volume'
        n = (x.shape[0] if per_volume else 1) * int(resampled[0]) * int(resampled[1])
        knots = ops.preprocess_quantiles(x, resampled, quantile_ranks(n, setting['percentiles']), per_volume)
        y = setting['standard'][modality] if setting['mode'] == 'landmarks' else (-1.0, 1.0)
        return knots, nn.host_to_device(np.asarray(y), x.device, np.float32)

    def bias_extent(self, spacing, selected, what):
        """'2d' or '3d' for one file under the folder's bias_field setting: the configured extent, else '3d' where the file holds a
        slice_spacing.  '3d' needs that spacing and one contiguous run of slices, and says so."""
        extent = self.bias_field['extent'] or ('3d' if spacing is not None else '2d')
        if extent == '3d':
            if spacing is None:
                raise ValueError('%s: "bias_field" extent 3d needs a slice_spacing (mm between slices) in every file; this one holds '
                                 'none -- add it, or set "extent": "2d"' % what)
            if selected is not None and len(selected) > 1 and np.any(np.diff(selected) != 1):
                raise ValueError('%s: "bias_field" extent 3d needs one contiguous run of slices, but "slices" selects %d that are not '
                                 'consecutive -- set "extent": "2d"' % (what, len(selected)))
        return extent

    def bias_corrected(self, x, res, spacing=None, selected=None, what='volume'):
        """The raw slices x [S,H,W] of one (volume, modality) on the device, as the rest of the loader shall see them: x itself when
        bias_field is off, else a corrected copy (ops.bias_correct; the selected slices only).  The one place where this is decided:
        `_upload` calls it once per (volume, modality), before intensity_knots."""
        setting = self.bias_field
        if setting['mode'] == 'off' or x.shape[0] == 0:
            return x
        extent = self.bias_extent(spacing, selected, what)
        params = dict(sigma_mm=setting['sigma_mm'], levels=setting['levels'], iterations=setting['iterations'], extent=extent)
        return ops.bias_correct(x, (spacing if extent == '3d' else 1.0, float(res[0]), float(res[1])), params)

    def denoised(self, x, modality, selected=None, what='volume'):
        """The raw slices x [S,H,W] of one (volume, modality) on the device after the folder's `denoise` setting: x itself when it is off
        (nothing is launched), else a denoised copy (ops.nlm_denoise).  The one place where this is decided: `_upload` calls
        it once per (volume, modality), immediately before bias_corrected.  Extent 3d searches
        the neighbouring slices too and therefore needs one contiguous run of slices (no slice_spacing: the rule has no mm in it)."""
        setting = self.denoise
        if setting['mode'] == 'off' or x.shape[0] == 0:
            return x
        if setting['extent'] == '3d' and selected is not None and len(selected) > 1 and np.any(np.diff(selected) != 1):
            raise ValueError('%s: "denoise" extent 3d needs one contiguous run of slices, but "slices" selects %d that are not '
                             'consecutive -- set "extent": "2d"' % (what, len(selected)))
        params = {k: v for k, v in setting.items() if k != 'mode'}
        if isinstance(params['sigma'], dict):
            params['sigma'] = params['sigma'][modality]
        return ops.nlm_denoise(x, params)

    def alignment(self, volume, xs, geometries):
        """The folder's `align` setting applied to one volume whose modalities' raw slices xs (per modality [S,H,W] fp32 on the device,
        after `denoised` and `bias_corrected`) and geometries (per modality a record with `resolution` and `resampled`) are at hand: None
        when it is off (nothing is launched), else per modality dict(shift=(dz, dy, dx), keep=(start, stop), rows, cols, record).
        shift: ops.align_volumes' against the reference modality, (0, 0, 0) for the reference itself.  keep: the run of this modality's
        selected slices that stays -- the reference keeps the intersection over the moving modalities of [max(0, -dz), min(S_a, S_b - dz)),
        a moving one the same run moved by its dz.  rows / cols: the (lo, kept, before) windows -- crop_pad_map's, bit for bit, for the
        reference and on every axis without a shift; tile_window(centre_start(R, O) + d, R, O) on an axis shifted by d (a plain window:
        where crop_pad_map removes ceil(surplus / 2) pixels from BOTH ends of an odd surplus and repeats the last pixel, the shifted
        window keeps all O).  The one place where this is decided: `_upload` calls it once per volume, after bias_corrected and before
        intensity_knots; the result is cached per volume (None: not cached)."""
        setting = self.align
        if setting['mode'] == 'off':
            return None
        if volume is not None and volume in self._alignments:
            return self._alignments[volume]
        OH, OW = self.input_shape[:2]
        ref = self.modalities.index(setting['reference'])
        params = {k: v for k, v in setting.items() if k not in ('mode', 'reference')}
        out = [None] * len(self.modalities)
        lo, hi = 0, int(xs[ref].shape[0])
        for j, mod in enumerate(self.modalities):
            if j == ref:
                shift, record = (0, 0, 0), None
            else:
                shift, record = ops.align_volumes(xs[ref], geometries[ref]['resolution'], xs[j], geometries[j]['resolution'],
                                                  self.target_resolution, self.input_shape, params)
                lo, hi = max(lo, -shift[0]), min(hi, int(xs[j].shape[0]) - shift[0])
                self.log.info('volume %s: %s against %s: shift (%d slices, %d, %d pixels) = (%.1f, %.1f) mm in plane, score %.6f, %.6f at '
                              'zero shift, %d voxel pairs' % (volume, mod, setting['reference'], shift[0], shift[1], shift[2],
                                                              shift[1] * self.target_resolution[0], shift[2] * self.target_resolution[1],
                                                              record[0], record[1], record[2]))
            RH, RW = geometries[j]['resampled']
            rows = tile_window(centre_start(RH, OH) + shift[1], RH, OH) if shift[1] else crop_pad_map(RH, OH)
            cols = tile_window(centre_start(RW, OW) + shift[2], RW, OW) if shift[2] else crop_pad_map(RW, OW)
            out[j] = dict(shift=shift, rows=rows, cols=cols, record=record)
        if hi <= lo:
            raise ValueError('volume %s: after alignment no slice of %s has a partner in every other modality (slice shifts %s for %s '
                             'slices); check the files, or lower "max_slices" of "align"'
                             % (volume, setting['reference'], ', '.join('%s: %d' % (m, a['shift'][0]) for m, a in zip(self.modalities, out)),
                                ', '.join('%s: %d' % (m, x.shape[0]) for m, x in zip(self.modalities, xs))))
        for a in out:
            a['keep'] = (lo + a['shift'][0], hi + a['shift'][0])
        if volume is not None:
            self._alignments[volume] = out
        return out

    def _upload(self, volume, require_label):
        """per modality of one volume: (x, record) -- the selected raw slices [S,H,W] fp32 on the device after denoised and bias_corrected,
        and the geometry record of load_volume_for_prediction; then the volume's alignment applied to both (slices, label, rows, cols,
        shift), or the equal-counts check when `align` is off"""
        device = nn.default_device()
        xs, geometry = [], []
        for mod in self.modalities:
            image, label, res, selected, spacing = self._read_file(volume, mod, require_label)
            S_file, H, W = image.shape
            if selected is None:
                selected = np.arange(S_file)
            resampled, rows, cols = self.geometry(H, W, res)
            what = 'volume %s, modality %s' % (volume, mod)
            x = self.denoised(nn.host_to_device(image[selected], device, np.float32), mod, selected, what)
            xs.append(self.bias_corrected(x, res, spacing, selected, what))
            geometry.append(dict(file=self.manifest['volumes'][str(volume)][mod]['file'], raw_shape=(S_file, H, W),
                                 slices=[int(i) for i in selected], resolution=res, resampled=resampled, rows=rows, cols=cols,
                                 label=None if label is None else np.ascontiguousarray(label[selected]), slice_spacing=spacing))
        aligned = self.alignment(volume, xs, geometry)
        if aligned is None:
            self._same_counts(volume, [x.shape[0] for x in xs])
            return xs, geometry
        for j, (a, g) in enumerate(zip(aligned, geometry)):
            k0, k1 = a['keep']
            xs[j] = xs[j][k0:k1]
            g.update(slices=g['slices'][k0:k1], rows=a['rows'], cols=a['cols'], shift=a['shift'],
                     label=None if g['label'] is None else np.ascontiguousarray(g['label'][k0:k1]))
        return xs, geometry

    def load_volume_for_prediction(self, volume):
        """One volume, labelled or not, for volume_predictor.py: (images, geometry).  images: per modality the preprocessed container
        [S,OH,OW,1] on the device (ops.preprocess_images: no label kernel is launched).  geometry: per modality a record with what the
        way back needs -- file, raw_shape (S_file, H, W), slices (the selected file indices, in order), resolution, resampled (RH, RW),
        rows / cols (lo, kept, before), label (the selected raw slices [S,H,W] uint8, or None) and slice_spacing (mm between the file's
        slices, or None).  Under `align`, slices and label hold the kept run only, rows / cols are the shifted windows and `shift` is
        the modality's (dz, dy, dx)."""
        OH, OW = self.input_shape[:2]
        xs, geometry = self._upload(volume, False)
        images = []
        for mod, x, g in zip(self.modalities, xs, geometry):
            container = torch.zeros((x.shape[0], OH, OW, 1), dtype=torch.float32, device=x.device)
            ops.preprocess_images(x, container, g['resampled'], g['rows'], g['cols'], 0, knots=self.intensity_knots(x, g['resampled'], mod))
            images.append(container)
        return images, geometry

    def _same_counts(self, volume, counts):
        if len(set(counts)) != 1:
            raise ValueError('volume %s: the modalities hold different numbers of slices after selection (%s); state the matching '
                             'ranges under "slices" in %s' % (volume, ', '.join('%s: %d' % mc for mc in zip(self.modalities, counts)),
                                                               MANIFEST))

    def upload_volume(self, volume):
        """(raw, geometry) of one volume: per modality the selected raw slices [S,H,W] fp32 on the device, uploaded once, and the
        record of load_volume_for_prediction plus `knots`: intensity_knots' result, selected once here and shared by every tile.
        What load_volume_tiles builds its containers from, for every predicted modality."""
        raw, geometry = self._upload(volume, False)
        for mod, x, g in zip(self.modalities, raw, geometry):
            g['knots'] = self.intensity_knots(x, g['resampled'], mod)
        return raw, geometry

    def tile_plan(self, geometry, m, overlap):
        """per modality (rows, cols): the tiles of the frame of the predicted modality m (tile_axis with overlap = (rows, columns)), and
        for every other modality the windows that go with them (tiles_of_other, moved by the difference of the records' `shift`s)"""
        OH, OW = self.input_shape[:2]
        RH, RW = geometry[m]['resampled']
        rows, cols = tile_axis(RH, OH, overlap[0]), tile_axis(RW, OW, overlap[1])
        own = geometry[m].get('shift', (0, 0, 0))
        plan = []
        for j, g in enumerate(geometry):
            d = g.get('shift', (0, 0, 0))
            plan.append((rows, cols) if j == m else (tiles_of_other(rows, RH, g['resampled'][0], OH, d[1] - own[1]),
                                                     tiles_of_other(cols, RW, g['resampled'][1], OW, d[2] - own[2])))
        return plan

    def load_volume_tiles(self, volume, m, overlap, uploaded=None):
        """One volume cut into the tiles that cover the whole resampled frame of modality m: (images, geometry, plan).  images: per
        modality a container [TR*TC*S,OH,OW,1] on the device, tile-major (tile tr * TC + tc is a contiguous [S,OH,OW,1] written by
        ops.preprocess_images with that tile's index maps; the rescale is per whole resampled frame, so the tiles of a slice share
        one intensity scale).  geometry: as load_volume_for_prediction.  plan: tile_plan's.  overlap = (rows, columns) in pixels;
        uploaded: upload_volume's result, when the caller loads tiles for several modalities of one volume."""
        raw, geometry = self.upload_volume(volume) if uploaded is None else uploaded
        OH, OW = self.input_shape[:2]
        plan = self.tile_plan(geometry, m, overlap)
        images = []
        for x, geo, (rows, cols) in zip(raw, geometry, plan):
            S = x.shape[0]
            container = torch.zeros((len(rows) * len(cols) * S, OH, OW, 1), dtype=torch.float32, device=x.device)
            for tr, r in enumerate(rows):
                for tc, c in enumerate(cols):
                    t = tr * len(cols) + tc
                    ops.preprocess_images(x, container[t * S:(t + 1) * S], geo['resampled'], r, c, 0, knots=geo.get('knots'))
            images.append(container)
        return images, geometry, plan

    # ---- the reference's loading surface --------------------------------------------------------------------------------------
    def load_all_modalities_concatenated(self, split, split_type, downsample=1):
        """every volume of the split through `_upload`, as prediction loads it; their counts of slices (under `align` the kept runs) size
        one pair of device containers [n,OH,OW,M] / [n,OH,OW,M*num_masks], each volume's share of which ops.preprocess_volume writes per
        modality.  One copy brings them to the host: a copy per volume and a concatenation there measured a tenth slower."""
        device = nn.default_device()
        OH, OW = self.input_shape[:2]
        M, K = len(self.modalities), self.num_masks
        volumes = self.get_volumes_for_split(split, split_type)
        uploaded = [self._upload(v, True) for v in volumes]
        counts = [xs[0].shape[0] for xs, _ in uploaded]
        images = torch.zeros((sum(counts), OH, OW, M), dtype=torch.float32, device=device)
        masks = torch.zeros((sum(counts), OH, OW, M * K), dtype=torch.float32, device=device)
        values = nn.host_to_device(np.asarray(self.label_values), device, np.int32)
        n0 = 0
        for (xs, geometry), S in zip(uploaded, counts):
            for m, (mod, x, g) in enumerate(zip(self.modalities, xs, geometry)):
                ops.preprocess_volume(x, nn.host_to_device(g['label'], device, np.uint8), values, images[n0:n0 + S], masks[n0:n0 + S],
                                      g['resampled'], g['rows'], g['cols'], m, knots=self.intensity_knots(x, g['resampled'], mod))
            n0 += S
        index = np.concatenate([np.array([v] * S) for v, S in zip(volumes, counts)], axis=0) if volumes else np.zeros((0,), np.int64)
        return MultimodalPairedData(nn.to_numpy(images), nn.to_numpy(masks), index, downsample=downsample,
                                    num_modalities=len(self.modalities))

    def load_labelled_data(self, split, split_type, modality, normalise=True, downsample=1, root_folder=None):
        """one modality by name, or 'all': the modalities stacked along the slice axis (chaos.py:57-99)"""
        data = self.load_all_modalities_concatenated(split, split_type, downsample)
        if modality == 'all':
            mods = range(len(self.modalities))
        elif modality in self.modalities:
            mods = [self.modalities.index(modality)]
        else:
            raise ValueError('Unknown modality: %r (%s has %s)' % (modality, self.data_folder, ', '.join(self.modalities)))
        images = np.concatenate([data.get_images_modi(m) for m in mods], axis=0)
        masks = np.concatenate([data.get_masks_modi(m) for m in mods], axis=0)
        index = np.concatenate([data.index for _ in mods], axis=0)
        return Data(images, masks, index, 1)

    def load_unlabelled_data(self, split, split_type, modality, normalise=True, downsample=1):
        return self.load_labelled_data(split, split_type, modality, normalise, downsample)

    def load_all_data(self, split, split_type, modality, normalise=True, downsample=1):
        return self.load_labelled_data(split, split_type, modality, normalise, downsample)
