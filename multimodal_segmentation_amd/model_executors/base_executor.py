"""Base class of the executors (reference model_executors/base_executor.py): batch alignment, the background
("residual") mask channel, and the augmenting data generators (keras ImageDataGenerator with +-20 degree rotations,
base_executor.py:37-78,103-110 -> utils/augment.RotationFlow: shuffle, gather and rotate on the device; any other pixel
augmentation of the dict -> utils/augment.AugmentFlow)."""
import logging

import numpy as np

log = logging.getLogger('executor')


class Executor(object):
    def __init__(self, conf, model):
        self.conf = conf
        self.model = model
        self.loader = model.loader
        self.epoch = 0
        self.batch = 0
        self.batches = 0

    def add_residual(self, data):
        """reference base_executor.py:83-87"""
        residual = np.ones(data.shape[:-1] + (1,))
        for i in range(data.shape[-1]):
            residual[data[..., i:i + 1] == 1] = 0
        return np.concatenate([data, residual], axis=-1)

    def align_batches(self, array_list):
        """reference base_executor.py:112-119"""
        mn = np.min([x.shape[0] for x in array_list])
        return [x[0:mn] + 0. for x in array_list]

    def get_datagen_params(self):
        """augmentation switches of base_executor.py:103-110: only rotation_range is non-trivial"""
        return dict(horizontal_flip=False, vertical_flip=False, rotation_range=20., width_shift_range=0, height_shift_range=0,
                    zoom_range=0)

    def datagen_params(self):
        """get_datagen_params() with the build-defined conf.datagen_params (a dict) merged over it, validated"""
        from ..utils.augment import check_datagen_params
        p = dict(self.get_datagen_params())
        extra = self.conf.get('datagen_params', None)
        if extra:
            if not isinstance(extra, dict):
                raise ValueError('conf.datagen_params must be a dict, got %r' % (extra,))
            p.update(extra)
        return check_datagen_params(p)

    def get_data_generator(self, train_images=None, train_labels=None):
        """Iterator over (images..., labels...) batches, all shuffled and augmented as keras does (base_executor.py:37-78: one
        keras flow per array with a shared seed, zipped).  A single array yields bare batches instead of 1-tuples.
        RotationFlow when the dict sets nothing but rotation_range (the reference's default), AugmentFlow otherwise."""
        from ..utils.augment import AugmentFlow, RotationFlow, rotation_only
        arrays, n_images = [], 0
        for group in (train_images, train_labels):
            if group is not None:
                arrays += list(group) if isinstance(group, (list, tuple)) else [group]
            if group is train_images:
                n_images = len(arrays)          # the leading arrays are images: intensity augmentation (INTENSITY_KEYS) changes only them
        if not arrays:
            raise Exception('No data to iterate.')
        p = self.datagen_params()
        # data parallel: rank r reseeds the global numpy stream with conf.seed + 7919 r (+ batch index), so shuffles, rotation
        # angles and the z / pool-index draws that follow a batch differ between replicas; rank 0 follows the reference stream
        from ..parallel import dp
        seed = self.conf.seed + 7919 * dp.rank()
        order = self.conf.get('augment_interpolation_order', 1)
        if rotation_only(p):
            return RotationFlow(arrays, self.conf.batch_size, seed, self.device, rotation_range=p.get('rotation_range', 0.),
                                order=order)
        return AugmentFlow(arrays, self.conf.batch_size, seed, self.device, p, order=order, n_images=n_images)

    def validate(self, epoch_loss):
        pass

    def stop_criterion(self, es, logs):
        es.on_epoch_end(self.epoch, logs)
        return es.stopped_epoch > 0


class EarlyStopping(object):
    """keras.callbacks.EarlyStopping(monitor, min_delta, patience), mode 'min' (dafnet_executor.py:222)"""

    def __init__(self, monitor, min_delta=0., patience=0):
        self.monitor, self.min_delta, self.patience = monitor, min_delta, patience
        self.best = np.inf
        self.wait = 0
        self.stopped_epoch = 0

    def on_epoch_end(self, epoch, logs):
        cur = logs.get(self.monitor)
        if cur is None:
            return
        if cur < self.best - self.min_delta:
            self.best, self.wait = cur, 0
        else:
            self.wait += 1
            if self.wait >= self.patience:
                self.stopped_epoch = epoch
