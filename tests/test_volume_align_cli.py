"""The `--align*` options of experiment.py: the override reaches the loader and experiment_configuration.json, a predict folder with another
setting is warned about, and bad values are refused with messages that name the option or the key.  No GPU: nothing is loaded."""
import json
import logging
import os

import pytest

from multimodal_segmentation_amd import loaders
from multimodal_segmentation_amd.loaders import loader_factory
from tests import volume_loader_ref as R

FULL = dict(mode='mi', reference='t1', max_shift_mm=40.0, max_slices=4, bins=32, levels=3, min_overlap=0.5, percentiles=[0.5, 99.5])


@pytest.fixture(autouse=True)
def _clean_registries():
    saved = dict(loaders.data_conf), dict(loaders.align_conf)
    yield
    for registry, old in zip((loaders.data_conf, loaders.align_conf), saved):
        registry.clear()
        registry.update(old)


@pytest.fixture
def folder(tmp_path):
    out = str(tmp_path / 'volumes')
    R.tool().write_folder(out, volumes=3, size=32, slices=2, seed=1)
    return out


def test_cli_override_reaches_the_loader_and_the_recorded_configuration(folder, tmp_path, monkeypatch):
    from multimodal_segmentation_amd.experiment import Experiment, parse_arguments
    monkeypatch.chdir(tmp_path)
    base = ['--config', 'dafnet_config_chaos', '--split', '0', '--data_folder', folder]
    conf = Experiment().get_config(0, parse_arguments(base))
    assert loaders.align_conf == {} and conf.align == {'mode': 'off'}          # no override, no key: off
    conf = Experiment().get_config(0, parse_arguments(base + ['--align', 'mi']))
    assert conf.align == FULL and loader_factory.init_loader('chaos').align == FULL
    dumped = json.load(open(os.path.join(conf.folder, 'experiment_configuration.json')))
    assert dumped['align'] == FULL and dumped['data_folder'] == folder
    conf = Experiment().get_config(0, parse_arguments(base + ['--align', 'mi', '--align_reference', 't2', '--align_max_shift_mm', '25', '--align_max_slices',
                                                               '2', '--align_bins', '64', '--align_levels', '2', '--align_min_overlap', '0.75']))
    want = dict(FULL, reference='t2', max_shift_mm=25.0, max_slices=2, bins=64, levels=2, min_overlap=0.75)
    assert conf.align == want and loader_factory.init_loader('chaos').align == want
    assert json.load(open(os.path.join(conf.folder, 'experiment_configuration.json')))['align'] == want
    conf = Experiment().get_config(0, parse_arguments(base + ['--align', 'off']))
    assert conf.align == {'mode': 'off'} == loader_factory.init_loader('chaos').align and loaders.align_conf == {'chaos': {'mode': 'off'}}
    Experiment().get_config(0, parse_arguments(base))          # a later run without the options follows dataset.json again
    assert loaders.align_conf == {}


def test_bad_values_are_refused_with_their_names(folder, tmp_path, monkeypatch, capsys):
    from multimodal_segmentation_amd.experiment import Experiment, parse_arguments
    monkeypatch.chdir(tmp_path)
    base = ['--config', 'dafnet_config_chaos', '--split', '0', '--data_folder', folder]
    for bad, word in ((['--align_bins', '16'], '--align_bins'), (['--align', 'off', '--align_levels', '2'], 'go with --align mi'),
                      (['--align', 'ncc'], 'invalid choice'), (['--align', 'mi', '--align_bins', '65'], 'bins must be a whole number in 2..64'),
                      (['--align', 'mi', '--align_bins', '1'], 'bins'), (['--align', 'mi', '--align_levels', '0'], 'levels must be a whole number in 1..8'),
                      (['--align', 'mi', '--align_max_slices', '-1'], 'max_slices'), (['--align', 'mi', '--align_max_shift_mm', '-3'], 'max_shift_mm'),
                      (['--align', 'mi', '--align_min_overlap', '0'], 'min_overlap must be a number in (0, 1]'),
                      (['--align', 'mi', '--align_min_overlap', '1.5'], 'min_overlap'), (['--align', 'mi', '--align_bins', 'many'], '--align_bins')):
        with pytest.raises(SystemExit):
            parse_arguments(base + bad)
        assert word in capsys.readouterr().err, bad
    with pytest.raises(ValueError) as e:          # the folder is known only here
        Experiment().get_config(0, parse_arguments(base + ['--align', 'mi', '--align_reference', 'ct']))
    assert 'reference' in str(e.value) and "'ct'" in str(e.value) and 't1, t2' in str(e.value)


def test_predict_folder_with_another_setting_logs_a_warning(folder, tmp_path, caplog):
    from multimodal_segmentation_amd.experiment import warn_predict_stages
    from multimodal_segmentation_amd.utils.config import EasyDict
    other = str(tmp_path / 'scans')
    R.tool().write_folder(other, volumes=3, size=64, slices=2, seed=5, name='site_b', unlabelled=True, misalign=4)
    log = logging.getLogger('test_volume_align_cli')
    own = json.load(open(os.path.join(other, 'dataset.json')))['align']
    trained = dict(FULL, **{k: v for k, v in own.items() if k != 'mode'})
    with caplog.at_level(logging.WARNING):
        assert not warn_predict_stages(EasyDict(folder='run', align=trained), other, log)          # the same setting: silence
        assert not warn_predict_stages(EasyDict(folder='run'), folder, log)                        # neither records nor asks for anything
    assert caplog.text == ''
    with caplog.at_level(logging.WARNING):
        assert warn_predict_stages(EasyDict(folder='run'), other, log) == ['align']                # trained unaligned, predicts aligned
    assert '"off"' in caplog.text and '"mi"' in caplog.text and other in caplog.text and 'alignment' in caplog.text
    caplog.clear()
    loaders.align_conf['site_b'] = {'mode': 'off'}                                                # the override counts
    with caplog.at_level(logging.WARNING):
        assert warn_predict_stages(EasyDict(folder='run', align=trained), other, log) == ['align']
        assert not warn_predict_stages(EasyDict(folder='run'), other, log)
