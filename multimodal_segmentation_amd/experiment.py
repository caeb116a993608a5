"""Command-line entry point with the reference's interface (experiment.py:100-111):

    python experiment.py --config <module in configuration/> --split <int> [--l_mix f] [--test b]
                         [--test_dataset chaos] [--automatedpairing b] [--randomise b]
                         [--data_folder PATH] [--test_data_folder PATH]
                         [--intensity_norm minmax|window] [--intensity_scope slice|volume] [--intensity_percentiles LO,HI]
                         [--bias_correction off|n3] [--bias_sigma_mm MM] [--bias_levels N] [--bias_iterations N] [--bias_extent 2d|3d]
                         [--denoise off|nlm] [--denoise_sigma auto|V] [--denoise_h K] [--denoise_search N] [--denoise_patch N]
                         [--denoise_search_z N] [--denoise_extent 2d|3d] [--denoise_noise rician|gaussian]
                         [--align off|mi] [--align_reference MOD] [--align_max_shift_mm MM] [--align_max_slices N] [--align_bins B]
                         [--align_levels L] [--align_min_overlap F]
                         [--predict_folder PATH] [--predict_out PATH] [--predict_mode simple|def|max] [--predict_order 0|1]
                         [--predict_surface true|false] [--predict_components none|largest] [--predict_connectivity 6|26]
                         [--predict_fill_holes none|2d|3d]
                         [--predict_smooth open|close|smooth] [--predict_smooth_radius MM] [--predict_smooth_extent 2d|3d]
                         [--predict_robust true|false] [--predict_percentile Q] [--predict_tolerance MM]
                         [--predict_tiles true|false] [--predict_tile_overlap PIXELS] [--predict_tta LIST]
                         [--predict_crf SPEC]
                         [--predict_ensemble RUN[,RUN...]] [--predict_uncertainty true|false] [--predict_calibration_bins B]

`--data_folder` (build-defined, like `conf.data_folder`) names a folder of exported volumes (loaders/volume_folder.py); without it
every configuration trains and tests on the synthetic volumes.  `--intensity_norm` and its two companions (build-defined, like
`conf.intensity`) override the `intensity` block of every folder of the run (loaders.intensity_conf).  `--predict_folder`
(build-defined) names a folder of exported volumes, labelled or not, for which the checkpoint of the run folder writes label volumes on each volume's own grid (volume_predictor.py): after
the test pass, or instead of training with `--test`.

The run folder name and the config mutations follow Experiment.get_config (experiment.py:31-72):
`<folder>[_randomise][_automatedpairing]_l<l_mix>_<modality>_split<split>` with dots stripped, n_pairs = 3 under automated
pairing else 1, `<folder>/experiment_configuration.json` written before and after training (74-78, 93-97).
"""
import argparse
import collections
import importlib
import json
import logging
import os
import subprocess

import numpy as np

from .parallel import dp
from .utils.config import EasyDict

_PKG = __package__


def true_or_false(text):
    """`true` / `false` of --predict_surface (argparse's type=bool reads every non-empty string as True)"""
    if text.lower() in ('true', '1', 'yes'):
        return True
    if text.lower() in ('false', '0', 'no'):
        return False
    raise argparse.ArgumentTypeError('expected true or false, got %r' % text)


def parse_arguments(argv=None):
    ap = argparse.ArgumentParser(description='multimodal segmentation experiment')
    ap.add_argument('--config', required=True, help='module name under configuration/')
    ap.add_argument('--split', required=True, help='data split index')
    ap.add_argument('--test', type=bool, help='only evaluate on the test volumes')
    ap.add_argument('--test_dataset', choices=['chaos'], help='override the configured test dataset')
    ap.add_argument('--l_mix', help='fraction of labelled volumes')
    ap.add_argument('--w_boundary', type=float, metavar='W',
                    help='weight of the boundary loss on the segmentation outputs, 0 or more (overrides the configuration; 0 = off)')
    ap.add_argument('--boundary_ramp_epochs', type=int, metavar='N',
                    help='epochs over which that weight rises linearly to --w_boundary (overrides the configuration; 0 = at once)')
    ap.add_argument('--w_lovasz', type=float, metavar='W',
                    help='weight of the Lovasz-Softmax loss on the segmentation outputs, 0 or more (overrides the configuration; 0 = off)')
    ap.add_argument('--lovasz_ramp_epochs', type=int, metavar='N',
                    help='epochs over which that weight rises linearly to --w_lovasz (overrides the configuration; 0 = at once)')
    ap.add_argument('--lovasz_classes', choices=['present', 'all'],
                    help="classes a sample's Lovasz-Softmax loss averages over: those it holds, or all (overrides the configuration)")
    ap.add_argument('--automatedpairing', type=bool, help='learn the pairing weights (n_pairs = 3)')
    ap.add_argument('--randomise', type=bool, help='randomise the multimodal pairs')
    ap.add_argument('--data_folder', help='folder of exported volumes (dataset.json + .npz) to train, validate and test on')
    ap.add_argument('--test_data_folder', help='another folder of exported volumes for the test pass')
    ap.add_argument('--intensity_norm', choices=['minmax', 'window'],
                    help='intensity normalisation of every volume folder of the run, instead of what their dataset.json say: every '
                         'slice by its extremes / clipped to a percentile window')
    ap.add_argument('--intensity_scope', choices=['slice', 'volume'], help='the window of --intensity_norm window is taken per slice / '
                                                                           'per volume (default: volume)')
    ap.add_argument('--intensity_percentiles', metavar='LO,HI', help='the window of --intensity_norm window (default: 0.5,99.5)')
    ap.add_argument('--bias_correction', choices=['off', 'n3'],
                    help='bias-field correction of every volume folder of the run at load time, instead of what their dataset.json say '
                         '(n3: log-domain histogram sharpening with a masked Gaussian smoother, on the device)')
    ap.add_argument('--bias_sigma_mm', type=float, help='width of the smoothing Gaussian of --bias_correction n3 at the first level, in mm '
                                                        '(default 40, an untuned starting value)')
    ap.add_argument('--bias_levels', type=int, help='levels of --bias_correction n3, each halving the width (default 3, untuned)')
    ap.add_argument('--bias_iterations', type=int, help='iterations per level of --bias_correction n3 (default 20, untuned)')
    ap.add_argument('--bias_extent', choices=['2d', '3d'], help='--bias_correction n3 smooths within slices / also across them (default: 3d '
                                                                'where the files hold slice_spacing)')
    ap.add_argument('--denoise', choices=['off', 'nlm'],
                    help='denoising of every volume folder of the run at load time, before the bias-field correction, instead of what '
                         'their dataset.json say (nlm: voxel-wise non-local means with in-plane patches, on the device)')
    ap.add_argument('--denoise_sigma', metavar='auto|V', help='noise level of --denoise nlm in raw grey values, or auto: estimated per '
                                                              'volume and modality on the device (default auto)')
    ap.add_argument('--denoise_h', type=float, help='smoothing strength of --denoise nlm in units of sigma (default 1, an untuned '
                                                    'starting value)')
    ap.add_argument('--denoise_search', type=int, help='in-plane search radius of --denoise nlm, 1..10 (default 5, untuned)')
    ap.add_argument('--denoise_patch', type=int, help='in-plane patch radius of --denoise nlm, 1..3 (default 1, untuned)')
    ap.add_argument('--denoise_search_z', type=int, help='slices before and after that --denoise_extent 3d also searches, 0..4 (default 1)')
    ap.add_argument('--denoise_extent', choices=['2d', '3d'], help='--denoise nlm searches within the slice / also in the neighbouring '
                                                                   'slices (default: 2d)')
    ap.add_argument('--denoise_noise', choices=['rician', 'gaussian'], help='noise model of --denoise nlm (default: rician)')
    ap.add_argument('--align', choices=['off', 'mi'],
                    help='alignment of the modalities of every volume of the run\'s volume folders at load time, instead of what their '
                         'dataset.json say (mi: a translation by whole slices and pixels that maximises normalised mutual information '
                         'against the reference modality, on the device)')
    ap.add_argument('--align_reference', metavar='MOD', help='the modality the others are aligned to (default: the folder\'s first)')
    ap.add_argument('--align_max_shift_mm', type=float, metavar='MM', help='largest in-plane shift of --align mi in mm (default 40, untuned)')
    ap.add_argument('--align_max_slices', type=int, metavar='N', help='largest slice shift of --align mi, 0..64 (default 4, untuned)')
    ap.add_argument('--align_bins', type=int, metavar='B', help='grey levels per volume of --align mi, 2..64 (default 32, untuned)')
    ap.add_argument('--align_levels', type=int, metavar='L', help='strides 2^(L-1) .. 1 of the search of --align mi, 1..8 (default 3, untuned)')
    ap.add_argument('--align_min_overlap', type=float, metavar='F',
                    help='share of the unshifted overlap a shift of --align mi must keep, in (0, 1] (default 0.5, untuned)')
    ap.add_argument('--predict_folder', help='folder of exported volumes (labels optional) to write predicted label volumes for')
    ap.add_argument('--predict_out', help='where to write them (default: <run folder>/predictions_<name in its dataset.json>)')
    ap.add_argument('--predict_mode', choices=['simple', 'def', 'max'], default='simple', help='predict_mask fusion mode')
    ap.add_argument('--predict_order', type=int, choices=[0, 1], default=1, help='resampling back to the raw grid: nearest / bilinear')
    ap.add_argument('--predict_surface', type=true_or_false, default=True, metavar='true|false',
                    help='also score labelled files that carry slice_spacing in mm (RAVD, ASSD, MSSD: results_surface_<modality>.csv)')
    ap.add_argument('--predict_components', choices=['none', 'largest'], default='none',
                    help="largest: keep each organ's largest 3-D connected component in the predicted label volumes")
    ap.add_argument('--predict_connectivity', type=int, choices=[6, 26], default=6,
                    help='neighbours of --predict_components: faces / faces, edges and corners')
    ap.add_argument('--predict_fill_holes', choices=['none', '2d', '3d'], default='none',
                    help='fill the zeros that an organ encloses, after --predict_components: slice by slice / in the volume '
                         '(results_holes_<modality>.csv)')
    ap.add_argument('--predict_smooth', choices=['open', 'close', 'smooth'], default=None,
                    help='open, close or open and then close every organ by a ball of --predict_smooth_radius mm, before '
                         '--predict_components and --predict_fill_holes (results_smooth_<modality>.csv)')
    ap.add_argument('--predict_smooth_radius', type=float, default=None, metavar='MM',
                    help='radius of the ball of --predict_smooth in mm, finite and above 0; there is no default')
    ap.add_argument('--predict_smooth_extent', choices=['2d', '3d'], default='2d',
                    help='the ball of --predict_smooth lies in the slice / reaches across slices (needs slice_spacing in the files)')
    ap.add_argument('--predict_robust', type=true_or_false, default=False, metavar='true|false',
                    help='also score them by HD (a percentile of the surface distances) and NSD (surface Dice at a tolerance): '
                         'results_robust_<modality>.csv')
    ap.add_argument('--predict_percentile', type=float, default=95.0, metavar='Q', help='percentile of --predict_robust, 0 to 100')
    ap.add_argument('--predict_tolerance', type=float, default=1.0, metavar='MM', help='tolerance of --predict_robust in mm, 0 or more')
    ap.add_argument('--predict_tiles', type=true_or_false, default=False, metavar='true|false',
                    help='predict the whole resampled frame of every slice: tiles of the input shape at several offsets, blended, '
                         'instead of its centre window alone')
    ap.add_argument('--predict_tile_overlap', type=int, default=None, metavar='PIXELS',
                    help='least overlap of neighbouring tiles of --predict_tiles, 0 or more and below the input extent (default: half '
                         'the input extent per axis)')
    ap.add_argument('--predict_tta', default='none', metavar='LIST',
                    help='test-time augmentation: predict every slice under these views and average the maps brought back, e.g. '
                         'id,fliplr,flipud,rot180 (= flips), d4 (the eight flips and right-angle turns) or id,rot10,rot-10 (degrees); '
                         'the first view is id')
    ap.add_argument('--predict_crf', default='none', metavar='SPEC',
                    help='refine every probability map against its image by a windowed mean-field CRF before the labels are taken: '
                         'none, default, or key=value,... over the defaults radius=5,iterations=5,w_a=4,theta_alpha=3,theta_beta=0.1,'
                         'w_s=1,theta_gamma=1.5, which are untuned starting values (tools/crf_sweep.py scores a grid of settings; '
                         'results_crf_<modality>.csv)')
    ap.add_argument('--predict_ensemble', default=None, metavar='RUN[,RUN...]',
                    help='further run folders (at most 7, e.g. the other splits of a cross-validation) whose checkpoints predict '
                         'together with this run: the mean of the models, its entropy and their disagreement '
                         '(<out>/uncertainty/, results_calibration_, reliability_ and results_uncertainty_<modality>.csv)')
    ap.add_argument('--predict_uncertainty', type=true_or_false, default=False, metavar='true|false',
                    help='write the uncertainty and calibration files of --predict_ensemble for this run alone (with --predict_tta '
                         'the views are the members)')
    ap.add_argument('--predict_calibration_bins', type=int, default=10, metavar='B',
                    help='bins of the reliability table of --predict_ensemble / --predict_uncertainty, 2 to 64')
    args = ap.parse_args(argv)
    if (args.intensity_scope or args.intensity_percentiles) and args.intensity_norm != 'window':
        ap.error('--intensity_scope and --intensity_percentiles go with --intensity_norm window')
    for cli in STAGE_CLI.values():          # `on` is None for intensity: its companions are checked above
        if cli.on is not None and any(getattr(args, a) is not None for a, _ in cli.companions) and getattr(args, cli.flag) != cli.on:
            ap.error('%s go with --%s %s' % (cli.listing or ', '.join('--' + a for a, _ in cli.companions), cli.flag, cli.on))
    if args.align:
        try:
            stage_override('align', {}, args)
        except ValueError as e:
            ap.error(str(e))
    if args.denoise_sigma is not None and args.denoise_sigma != 'auto':
        try:
            args.denoise_sigma = float(args.denoise_sigma)
        except ValueError:
            ap.error('--denoise_sigma takes auto or a number, got %r' % args.denoise_sigma)
    if args.intensity_percentiles is not None:
        try:
            args.intensity_percentiles = [float(v) for v in args.intensity_percentiles.split(',')]
        except ValueError:
            ap.error('--intensity_percentiles must be two numbers LO,HI, got %r' % args.intensity_percentiles)
    if args.predict_tile_overlap is not None and args.predict_tile_overlap < 0:
        ap.error('--predict_tile_overlap must be a number of pixels >= 0, got %r' % args.predict_tile_overlap)
    if not 0.0 <= args.predict_percentile <= 100.0:          # here, so that a bad value stops the run before the model is built
        ap.error('--predict_percentile must lie in [0, 100], got %r' % args.predict_percentile)
    if not 0.0 <= args.predict_tolerance < float('inf'):
        ap.error('--predict_tolerance must be a finite number of mm >= 0, got %r' % args.predict_tolerance)
    if args.predict_smooth is not None and args.predict_smooth_radius is None:
        ap.error('--predict_smooth %s needs --predict_smooth_radius MM: there is no default radius' % args.predict_smooth)
    if args.predict_smooth_radius is not None and not 0.0 < args.predict_smooth_radius < float('inf'):
        ap.error('--predict_smooth_radius must be a finite number of mm > 0, got %r' % args.predict_smooth_radius)
    return args


def robust_of(args):
    """(percentile, tolerance in mm) of --predict_robust true, else None"""
    if not getattr(args, 'predict_robust', False):
        return None
    return float(getattr(args, 'predict_percentile', 95.0)), float(getattr(args, 'predict_tolerance', 1.0))


def _flag(config, args, name):
    return bool(config.get(name, False)) or bool(getattr(args, name, None))


def folder_name(base, randomise, automatedpairing, l_mix, modality, split):
    parts = [base]
    if randomise:
        parts.append('randomise')
    if automatedpairing:
        parts.append('automatedpairing')
    parts += ['l%s' % l_mix, str(modality), 'split%s' % split]
    return '_'.join(parts).replace('.', '')


def git_hash():
    try:
        return subprocess.check_output(['git', 'rev-parse', 'HEAD'], stderr=subprocess.DEVNULL).decode().strip()
    except Exception:
        return ''


def _jsonable(o):
    if isinstance(o, np.integer):
        return int(o)
    if isinstance(o, np.floating):
        return float(o)
    raise TypeError(type(o))


def resolve(subpackage, dotted):
    """'dafnet.DAFNet' under models/ or model_executors/ -> class (experiment.py:115-123)"""
    module, cls = dotted.split('.')
    return getattr(importlib.import_module('%s.%s.%s' % (_PKG, subpackage, module)), cls)


def register_data_folders(module, args):
    """Fill loaders.data_conf (data set name -> folder, the reference's loaders/base_loader.py:5-7) from `--data_folder` /
    `--test_data_folder` or the configuration's `data_folder` / `test_data_folder`.  The folder is registered under the configured
    dataset_name and test_dataset.  A separate test folder whose configured name is the training data set's is registered under
    the `name` of its own dataset.json, which is returned as the test_dataset to use (else None)."""
    from .loaders import data_conf
    from .loaders.volume_folder import read_manifest
    named = module.get()                  # without a registered folder: only the names and folders are read from it
    folder = getattr(args, 'data_folder', None) or named.get('data_folder')
    test_folder = getattr(args, 'test_data_folder', None) or named.get('test_data_folder')
    train_name = named['dataset_name']
    test_name = getattr(args, 'test_dataset', None) or named.get('test_dataset', train_name)
    if folder:
        data_conf[train_name] = folder
    if not test_folder or (folder and os.path.abspath(test_folder) == os.path.abspath(folder)):
        if folder:
            data_conf[test_name] = folder
        return None
    if test_name != train_name:
        data_conf[test_name] = test_folder
        return None
    own_name = read_manifest(test_folder)['name']
    if own_name == train_name:
        raise ValueError('the test folder %s carries the name of the training data set (%r): give its dataset.json a "name" of its '
                         'own' % (test_folder, own_name))
    data_conf[own_name] = test_folder
    return own_name


CliStage = collections.namedtuple('CliStage', 'flag companions subject tail on listing modalities refused drop_none',
                                  defaults=(None, None, None, (), ()))

# The command-line side of the load-time stages, keyed and ordered like loaders/volume_folder.py's STAGES.  flag: the option that names
# the mode; companions: (option, key of the block) pairs that go with mode `on` (listing: how the refusal words them, else comma-separated; None
# for intensity, whose refusal parse_arguments words itself);
# subject and tail: the two phrases of the predict warning; modalities: what an override is validated against, which knows no folder yet;
# refused: modes an override may not name, with the reason; drop_none: keys registered only when set, so that the folder decides them.
STAGE_CLI = collections.OrderedDict((
    ('intensity', CliStage('intensity_norm', (('intensity_scope', 'scope'), ('intensity_percentiles', 'percentiles')),
                           '%s is normalised by %s', 'other grey levels', modalities=(),
                           refused=(('landmarks', 'landmarks are configured in the dataset.json of a folder '
                                                  '(tools/fit_intensity_landmarks.py), not as an override'),))),
    ('bias_field', CliStage('bias_correction', (('bias_sigma_mm', 'sigma_mm'), ('bias_levels', 'levels'), ('bias_iterations', 'iterations'),
                                                ('bias_extent', 'extent')),
                            'the bias field of %s is set to %s', 'other shading', on='n3',
                            listing='--bias_sigma_mm, --bias_levels, --bias_iterations and --bias_extent')),
    ('denoise', CliStage('denoise', (('denoise_sigma', 'sigma'), ('denoise_h', 'h'), ('denoise_search', 'search_radius'),
                                     ('denoise_patch', 'patch_radius'), ('denoise_search_z', 'search_radius_z'), ('denoise_extent', 'extent'),
                                     ('denoise_noise', 'noise')),
                         'the denoising of %s is set to %s', 'other noise', on='nlm')),
    ('align', CliStage('align', (('align_reference', 'reference'), ('align_max_shift_mm', 'max_shift_mm'), ('align_max_slices', 'max_slices'),
                                 ('align_bins', 'bins'), ('align_levels', 'levels'), ('align_min_overlap', 'min_overlap')),
                       'the alignment of %s is set to %s', 'modalities paired otherwise', on='mi', drop_none=('reference',)))))


def stage_override(stage, named, args):
    """the block of stage `stage` (a key of STAGE_CLI) from its mode option and companions, else the configuration's, else None: no
    override, every folder follows its own dataset.json"""
    from .loaders.volume_folder import check_stage
    cli = STAGE_CLI[stage]
    block, where = named.get(stage), 'conf.%s' % stage
    if getattr(args, cli.flag, None):
        block, where = {'mode': getattr(args, cli.flag)}, '--' + cli.flag
        for arg, key in cli.companions:
            if getattr(args, arg, None) is not None:
                block[key] = getattr(args, arg)
    if block is None:
        return None
    for mode, reason in cli.refused:
        if isinstance(block, dict) and block.get('mode') == mode:
            raise ValueError('%s: %s' % (where, reason))
    return check_stage(stage, dict(block), cli.modalities, where)


def register_stages(named, args, names):
    """Fill the registries of loaders.stage_conf for the data set names of this run; without an override their entries are removed"""
    from .loaders import stage_conf
    for stage, cli in STAGE_CLI.items():
        block = stage_override(stage, named, args)
        for name in names:
            if block is None:
                stage_conf[stage].pop(name, None)
            else:
                stage_conf[stage][name] = {k: v for k, v in block.items() if not (k in cli.drop_none and v is None)}


def warn_predict_stages(conf, folder, log):
    """a warning for every stage whose setting in force for the predict folder differs from the one the run folder records (conf.<key>; a
    run on the synthetic volumes records none: the stage's `off` block).  The keys of the stages it warned about."""
    from .loaders.volume_folder import STAGES, effective_setting, read_manifest
    manifest, warned = read_manifest(folder), []
    for stage, cli in STAGE_CLI.items():
        trained, here = conf.get(stage) or dict(STAGES[stage].off), effective_setting(folder, stage, manifest)
        if here != trained:
            log.warning('--predict_folder: %s, the run folder %s records %s: the model sees %s than it was trained on'
                        % (cli.subject % (folder, json.dumps(here, sort_keys=True)), conf.folder, json.dumps(trained, sort_keys=True), cli.tail))
            warned.append(stage)
    return warned


MEMBER_KEYS = ('model', 'input_shape', 'num_masks', 'modality')          # what a member of --predict_ensemble must share with the run


def ensemble_folders(text):
    """--predict_ensemble RUN[,RUN...] -> the folders; None or '' -> []"""
    from .volume_predictor import MAX_MEMBERS
    if text is None or not str(text).strip():
        return []
    folders = [f.strip() for f in str(text).split(',')]
    if not all(folders) or len(folders) > MAX_MEMBERS:
        raise ValueError('--predict_ensemble takes 1 to %d run folders RUN[,RUN...], got %r' % (MAX_MEMBERS, text))
    return folders


def member_conf(conf, folder):
    """the configuration a member of --predict_ensemble is built on: a copy of `conf` whose folder is that run.  The run must hold a
    checkpoint (FileNotFoundError), and what its experiment_configuration.json records of MEMBER_KEYS must be the run's (ValueError);
    a run folder without that file is taken at its word."""
    from . import volume_predictor
    if volume_predictor.checkpoint_of(folder) is None:
        raise FileNotFoundError('--predict_ensemble: the run folder %s holds no checkpoint to predict with' % folder)
    member = EasyDict(dict(conf.items()))
    member.folder = folder
    theirs = member_record(folder)
    for key in MEMBER_KEYS:
        if key in theirs and key in conf and json.loads(json.dumps(conf[key], default=_jsonable)) != theirs[key]:
            raise ValueError('--predict_ensemble: the run folder %s records %s = %r, this run has %r: the members of an ensemble '
                             'share model, input_shape, num_masks and modalities' % (folder, key, theirs[key], conf[key]))
    return member


def member_record(folder):
    """what the experiment_configuration.json of a run folder records, {} without one"""
    recorded = os.path.join(folder, 'experiment_configuration.json')
    if not os.path.isfile(recorded):
        return {}
    with open(recorded) as f:
        return json.load(f)


class Experiment(object):
    def __init__(self):
        self.log = None

    # ---- configuration --------------------------------------------------------------------------------------------
    def get_config(self, split, args):
        module = importlib.import_module('%s.configuration.%s' % (_PKG, args.config))
        test_dataset = register_data_folders(module, args)      # before get(): the configuration reads shapes from the loader
        conf = EasyDict(module.get())
        if test_dataset is not None:
            conf.test_dataset = test_dataset
        from .loaders import data_conf
        names = set(data_conf)
        if getattr(args, 'predict_folder', None):
            from .loaders.volume_folder import read_manifest
            names.add(read_manifest(args.predict_folder)['name'])
        register_stages(conf, args, sorted(names))         # before a loader that loads volumes is built: it reads its settings then
        if data_conf.get(conf.dataset_name):
            conf.data_folder = data_conf[conf.dataset_name]        # recorded in experiment_configuration.json
            from .loaders.volume_folder import effective_setting
            for stage in STAGE_CLI:                                 # the settings in force, override or dataset.json: recorded too
                conf[stage] = effective_setting(conf.data_folder, stage)
        conf.split = split
        conf.randomise = _flag(conf, args, 'randomise')
        conf.automatedpairing = _flag(conf, args, 'automatedpairing')
        conf.n_pairs = 3 if conf.automatedpairing else 1
        shown = conf.l_mix                       # the folder carries the string as typed on the command line
        if getattr(args, 'l_mix', None) is not None:
            conf.l_mix, shown = float(args.l_mix), args.l_mix
        for key in ('w_boundary', 'boundary_ramp_epochs', 'w_lovasz', 'lovasz_ramp_epochs', 'lovasz_classes'):   # build-defined keys; validated when the model is built
            if getattr(args, key, None) is not None:
                conf[key] = getattr(args, key)
        conf.folder = folder_name(conf.folder, conf.randomise, conf.automatedpairing, shown, conf.modality, split)
        if getattr(args, 'test_dataset', None):
            conf.test_dataset = args.test_dataset
        conf.githash = git_hash()
        self.save_config(conf)
        return conf


    def save_config(self, conf):
        if not dp.is_main():                      # data parallel: rank 0 owns the run folder
            return
        os.makedirs(conf.folder, exist_ok=True)
        with open(os.path.join(conf.folder, 'experiment_configuration.json'), 'w') as f:
            json.dump(dict(conf.items()), f, default=_jsonable)

    def init_logging(self, conf):
        """<folder>/logfile.log at DEBUG level + the console (experiment.py:21-29).  Handlers are attached explicitly, so the
        log file also appears when the embedding process has configured the root logger already."""
        os.makedirs(conf.folder, exist_ok=True)
        root = logging.getLogger()
        root.setLevel(logging.DEBUG)
        if dp.is_main():
            fh = logging.FileHandler(os.path.join(conf.folder, 'logfile.log'))
            fh.setFormatter(logging.Formatter('%(asctime)s %(message)s'))
            root.addHandler(fh)
            root.addHandler(logging.StreamHandler())
        self.log = root
        root.debug(conf.items())
        root.info('---- Setting up experiment at ' + conf.folder + '----')

    # ---- run ----------------------------------------------------------------------------------------------------
    def get_executor(self, conf, test=False):
        model = resolve('models', conf.model)(conf)
        model.build()
        dp.sync_model(model)                      # data parallel: every replica starts from rank 0's weights
        return resolve('model_executors', conf.executor)(conf, model)

    def run_experiment(self, conf, test):
        executor = self.get_executor(conf, test)
        if not test:
            executor.train()
            self.save_config(conf)               # training adds keys (e.g. unlabelled counts)
        if dp.is_main():                          # replicas are identical after training: one rank evaluates and writes
            executor.test()
        dp.host_barrier()                         # not a GPU collective: the other ranks may wait longer than RCCL's watchdog allows

    def run_prediction(self, conf, args):
        """`--predict_folder`: label volumes from the CHECKPOINT of the run folder (a freshly built model loads it, as `--test` does),
        so that a run that has just trained and a later `--test` run write the same arrays"""
        from .loaders.volume_folder import read_manifest
        from .volume_predictor import VolumePredictor, checkpoint_of
        if checkpoint_of(conf.folder) is None:
            raise FileNotFoundError('--predict_folder: the run folder %s holds no checkpoint to predict with (train first, without '
                                    '--test)' % conf.folder)
        if dp.is_main():
            warn_predict_stages(conf, args.predict_folder, self.log)
            out = args.predict_out or os.path.join(conf.folder, 'predictions_%s' % read_manifest(args.predict_folder)['name'])
            members = []
            for folder in ensemble_folders(getattr(args, 'predict_ensemble', None)):
                theirs = member_conf(conf, folder)
                record = member_record(folder)          # the stages the member was trained under are the ones its folder records
                warn_predict_stages(EasyDict(dict(theirs.items(), **{s: record[s] for s in STAGE_CLI if s in record})),
                                    args.predict_folder, self.log)
                members.append(theirs)
            model = resolve('models', conf.model)(conf)
            model.build()
            for i, theirs in enumerate(members):
                members[i] = resolve('models', conf.model)(theirs)
                members[i].build()
            VolumePredictor(model, conf, members).run(args.predict_folder, out, mode=args.predict_mode, order=args.predict_order,
                                              uncertainty=bool(getattr(args, 'predict_uncertainty', False)),
                                              calibration_bins=getattr(args, 'predict_calibration_bins', 10),
                                              surface=getattr(args, 'predict_surface', True),
                                              components={'largest': 'largest'}.get(getattr(args, 'predict_components', 'none')),
                                              connectivity=getattr(args, 'predict_connectivity', 6), robust=robust_of(args),
                                              fill_holes={'2d': '2d', '3d': '3d'}.get(getattr(args, 'predict_fill_holes', 'none')),
                                              tiles=bool(getattr(args, 'predict_tiles', False)),
                                              tile_overlap=getattr(args, 'predict_tile_overlap', None),
                                              tta=getattr(args, 'predict_tta', None),
                                              crf=getattr(args, 'predict_crf', None),
                                              smooth=getattr(args, 'predict_smooth', None),
                                              smooth_radius=getattr(args, 'predict_smooth_radius', None),
                                              smooth_extent=getattr(args, 'predict_smooth_extent', '2d'))
            self.log.info('Predicted label volumes of %s written to %s' % (args.predict_folder, out))
        dp.host_barrier()

    def run(self, argv=None):
        args = parse_arguments(argv)
        # one process per GPU under `python -m torch.distributed.run` (RANK / LOCAL_RANK / WORLD_SIZE): join the RCCL group and
        # shard the slice pairs across ranks (parallel/dp.py); a plain `python experiment.py` run is single-GPU
        dp.init_from_env()
        conf = self.get_config(int(args.split), args)
        self.init_logging(conf)
        if getattr(args, 'predict_tiles', False) or getattr(args, 'predict_tile_overlap', None) is not None:      # before the model is built
            from .volume_predictor import check_tile_overlap
            check_tile_overlap(getattr(args, 'predict_tile_overlap', None), conf.input_shape)
        if getattr(args, 'predict_tta', 'none') not in (None, 'none'):          # before the model is built as well
            from .volume_predictor import check_tta
            check_tta(args.predict_tta, conf.input_shape)
        if getattr(args, 'predict_crf', 'none') not in (None, 'none'):          # and so is this
            from .volume_predictor import check_crf
            check_crf(args.predict_crf)
        if getattr(args, 'predict_ensemble', None) or getattr(args, 'predict_calibration_bins', 10) != 10:          # and these
            from .volume_predictor import check_calibration_bins
            check_calibration_bins(getattr(args, 'predict_calibration_bins', 10))
            for folder in ensemble_folders(getattr(args, 'predict_ensemble', None)):
                member_conf(conf, folder)
        if getattr(args, 'predict_folder', None) and args.test:
            from .volume_predictor import checkpoint_of
            if checkpoint_of(conf.folder) is None:          # before the test pass evaluates an untrained model
                raise FileNotFoundError('--test --predict_folder: the run folder %s holds no checkpoint (train first, without --test)'
                                        % conf.folder)
        self.run_experiment(conf, args.test)
        if getattr(args, 'predict_folder', None):
            self.run_prediction(conf, args)

    read_console_parameters = staticmethod(parse_arguments)


if __name__ == '__main__':
    Experiment().run()
