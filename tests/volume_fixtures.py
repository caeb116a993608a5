"""What the tests/test_volume_*.py files share: the `device` fixture (the CPU stand-ins of the C ABI, or the MI355X), the registry guard
and the small helpers around the predictor's output.  A plain module: a test file imports the names it uses, fixtures included."""
import importlib.util
import os

import numpy as np
import pytest

from multimodal_segmentation_amd import loaders, nn
from tests import volume_components_ref as C
from tests import volume_loader_ref as R
from tests import volume_metrics_ref as M
from tests import volume_predict_ref as P
from tests import volume_robust_ref as B


@pytest.fixture(params=[pytest.param('cpu', id='cpu-standin'), pytest.param('cuda', marks=pytest.mark.gpu, id='mi355x')])
def device(request, monkeypatch):
    if request.param == 'cpu':
        from tests import cpu_backend as cb
        for table in (R.STANDINS, P.STANDINS, M.STANDINS, C.STANDINS, B.STANDINS):
            for name, fn in table.items():
                monkeypatch.setitem(cb._TABLE, name, fn)
        cb.install()
        nn.set_default_device('cpu')
        yield 'cpu'
        cb.uninstall()
    else:
        nn.set_default_device('cuda:0')
        yield 'cuda'


@pytest.fixture(autouse=True)
def _clean_registry():
    saved = dict(loaders.data_conf)
    yield
    loaders.data_conf.clear()
    loaders.data_conf.update(saved)


def _dev(device):
    return 'cuda:0' if device == 'cuda' else 'cpu'


def _up(a, dev, dtype=np.uint8):
    """a copy of `a` on the device: on the CPU a tensor shares the memory of the array it is made from, and some inputs are cached"""
    return nn.host_to_device(np.array(a), dev, dtype)


def _score_tool():
    spec = importlib.util.spec_from_file_location('score_predictions', os.path.join(R.ROOT, 'tools', 'score_predictions.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _csv_rows(path):
    lines = open(path).read().strip().split('\n')
    return lines[0], {l.split(', ')[0]: l.split(', ')[1:] for l in lines[1:]}
