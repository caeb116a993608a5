"""TEST HELPER (numpy + scipy; PARITY UNPINNED): keras 2.1.6 `ImageDataGenerator(**d).flow(x, batch_size, seed)` for every pixel
argument the reference's dict can set (model_executors/base_executor.py:37-78,103-110), restated from keras' published source.
Keras 2.1.6 cannot be imported here, so none of the rules below has been checked against it -- UNVERIFIED, like
oracle/augment.py, which this extends:

  * Iterator._flow_index: per batch np.random.seed(seed + total_batches_seen) (the GLOBAL RNG); a new permutation when
    batch_index == 0; rows = index_array[cur : cur + B], the last batch of a pass may be short.
  * random_transform(x) (channels_last: row axis 0, column axis 1, channel axis 2), each value drawn only when its key is
    non-zero, in this order:
      1. theta = deg2rad(uniform(-rotation_range, rotation_range))
      2. tx = uniform(-height_shift_range, height_shift_range), times H if height_shift_range < 1  (tx moves rows)
      3. ty = uniform(-width_shift_range, width_shift_range), times W if width_shift_range < 1    (ty moves columns)
      4. shear = deg2rad(uniform(-shear_range, shear_range))
      5. zx, zy = uniform(zoom_range[0], zoom_range[1], 2) unless zoom_range == [1, 1]; a scalar z means [1 - z, 1 + z]
      then transform = rotation @ shift @ shear @ zoom (only the non-trivial factors) with
           rotation [[cos, -sin, 0], [sin, cos, 0]], shift [[1, 0, tx], [0, 1, ty]], shear [[1, -sin(s), 0], [0, cos(s), 0]],
           zoom [[zx, 0, 0], [0, zy, 0]];
      if any factor exists: transform_matrix_offset_center (about (H/2 + 0.5, W/2 + 0.5)) and apply_transform =
           ndi.affine_transform(channel, M[:2, :2], M[:2, 2], order=1, mode=fill_mode, cval=cval) per channel;
           otherwise the sample is not resampled.
      6. channel_shift_range != 0: random_channel_shift -- min, max of the whole (transformed) sample, then per channel
           clip(x_c + uniform(-i, i), min, max)
      7. horizontal_flip and random() < 0.5: flip the column axis
      8. vertical_flip and random() < 0.5: flip the row axis
  * apply_transform's `order` is 1 in keras; it is a parameter here so that the product's order-0 variant can be checked too.

Boundary handling is whatever the installed scipy does (the product's kernel rules were probed against scipy 1.15.3).
"""
import numpy as np
from scipy import ndimage as ndi


def transform_matrix_offset_center(matrix, x, y):
    o_x = float(x) / 2 + 0.5
    o_y = float(y) / 2 + 0.5
    offset_matrix = np.array([[1, 0, o_x], [0, 1, o_y], [0, 0, 1]])
    reset_matrix = np.array([[1, 0, -o_x], [0, 1, -o_y], [0, 0, 1]])
    return np.dot(np.dot(offset_matrix, matrix), reset_matrix)


def apply_transform(x, transform_matrix, channel_axis=2, fill_mode='nearest', cval=0., order=1):
    x = np.rollaxis(x, channel_axis, 0)
    final_affine_matrix = transform_matrix[:2, :2]
    final_offset = transform_matrix[:2, 2]
    channel_images = [ndi.affine_transform(x_channel, final_affine_matrix, final_offset, order=order, mode=fill_mode, cval=cval)
                      for x_channel in x]
    x = np.stack(channel_images, axis=0)
    return np.rollaxis(x, 0, channel_axis + 1)


def random_channel_shift(x, intensity, channel_axis=2):
    x = np.rollaxis(x, channel_axis, 0)
    min_x, max_x = np.min(x), np.max(x)
    shifts = []
    channel_images = []
    for x_channel in x:
        s = np.random.uniform(-intensity, intensity)
        shifts.append(s)
        channel_images.append(np.clip(x_channel + s, min_x, max_x))
    x = np.stack(channel_images, axis=0)
    return np.rollaxis(x, 0, channel_axis + 1), shifts


def flip_axis(x, axis):
    x = np.asarray(x).swapaxes(axis, 0)
    x = x[::-1, ...]
    return x.swapaxes(0, axis)


class ImageDataGeneratorRef(object):
    def __init__(self, rotation_range=0., width_shift_range=0., height_shift_range=0., shear_range=0., zoom_range=0.,
                 channel_shift_range=0., fill_mode='nearest', cval=0., horizontal_flip=False, vertical_flip=False, order=1):
        self.rotation_range = rotation_range
        self.width_shift_range = width_shift_range
        self.height_shift_range = height_shift_range
        self.shear_range = shear_range
        self.channel_shift_range = channel_shift_range
        self.fill_mode = fill_mode
        self.cval = cval
        self.horizontal_flip = horizontal_flip
        self.vertical_flip = vertical_flip
        self.order = order
        if np.isscalar(zoom_range):
            self.zoom_range = [1 - zoom_range, 1 + zoom_range]
        elif len(zoom_range) == 2:
            self.zoom_range = [zoom_range[0], zoom_range[1]]
        else:
            raise ValueError('zoom_range')

    def random_transform(self, x):
        """-> (transformed x, record of the draws: matrix (3x3 or None), shifts (list or None), hflip, vflip)"""
        img_row_axis, img_col_axis, img_channel_axis = 0, 1, 2
        if self.rotation_range:
            theta = np.deg2rad(np.random.uniform(-self.rotation_range, self.rotation_range))
        else:
            theta = 0
        if self.height_shift_range:
            tx = np.random.uniform(-self.height_shift_range, self.height_shift_range)
            if self.height_shift_range < 1:
                tx *= x.shape[img_row_axis]
        else:
            tx = 0
        if self.width_shift_range:
            ty = np.random.uniform(-self.width_shift_range, self.width_shift_range)
            if self.width_shift_range < 1:
                ty *= x.shape[img_col_axis]
        else:
            ty = 0
        if self.shear_range:
            shear = np.deg2rad(np.random.uniform(-self.shear_range, self.shear_range))
        else:
            shear = 0
        if self.zoom_range[0] == 1 and self.zoom_range[1] == 1:
            zx, zy = 1, 1
        else:
            zx, zy = np.random.uniform(self.zoom_range[0], self.zoom_range[1], 2)

        transform_matrix = None
        if theta != 0:
            rotation_matrix = np.array([[np.cos(theta), -np.sin(theta), 0], [np.sin(theta), np.cos(theta), 0], [0, 0, 1]])
            transform_matrix = rotation_matrix
        if tx != 0 or ty != 0:
            shift_matrix = np.array([[1, 0, tx], [0, 1, ty], [0, 0, 1]])
            transform_matrix = shift_matrix if transform_matrix is None else np.dot(transform_matrix, shift_matrix)
        if shear != 0:
            shear_matrix = np.array([[1, -np.sin(shear), 0], [0, np.cos(shear), 0], [0, 0, 1]])
            transform_matrix = shear_matrix if transform_matrix is None else np.dot(transform_matrix, shear_matrix)
        if zx != 1 or zy != 1:
            zoom_matrix = np.array([[zx, 0, 0], [0, zy, 0], [0, 0, 1]])
            transform_matrix = zoom_matrix if transform_matrix is None else np.dot(transform_matrix, zoom_matrix)
        if transform_matrix is not None:
            h, w = x.shape[img_row_axis], x.shape[img_col_axis]
            transform_matrix = transform_matrix_offset_center(transform_matrix, h, w)
            x = apply_transform(x, transform_matrix, img_channel_axis, fill_mode=self.fill_mode, cval=self.cval, order=self.order)
        shifts = None
        if self.channel_shift_range != 0:
            x, shifts = random_channel_shift(x, self.channel_shift_range, img_channel_axis)
        hflip = vflip = False
        if self.horizontal_flip:
            if np.random.random() < 0.5:
                x = flip_axis(x, img_col_axis)
                hflip = True
        if self.vertical_flip:
            if np.random.random() < 0.5:
                x = flip_axis(x, img_row_axis)
                vflip = True
        return x, dict(matrix=transform_matrix, shifts=shifts, hflip=hflip, vflip=vflip)


class NumpyArrayIteratorRef(object):
    """ImageDataGenerator(**params).flow(x, batch_size, shuffle=True, seed).  `records` holds the draws of the last batch."""

    def __init__(self, x, batch_size, seed, params, order=1):
        self.x = np.asarray(x, np.float32)
        self.gen = ImageDataGeneratorRef(order=order, **params)
        self.n, self.batch_size, self.seed = self.x.shape[0], batch_size, seed
        self.batch_index = 0
        self.total_batches_seen = 0
        self.index_array = None
        self.records = []

    def next_rows(self):
        if self.seed is not None:
            np.random.seed(self.seed + self.total_batches_seen)
        if self.batch_index == 0:
            self.index_array = np.random.permutation(self.n)
        cur = (self.batch_index * self.batch_size) % self.n
        if self.n > cur + self.batch_size:
            self.batch_index += 1
        else:
            self.batch_index = 0
        self.total_batches_seen += 1
        return self.index_array[cur:cur + self.batch_size]

    def __next__(self):
        rows = self.next_rows()
        out = np.zeros((len(rows),) + self.x.shape[1:], np.float32)
        self.records = []
        for i, j in enumerate(rows):
            out[i], rec = self.gen.random_transform(self.x[j].astype(np.float32))
            self.records.append(rec)
        self.rows = rows
        return out

    next = __next__
