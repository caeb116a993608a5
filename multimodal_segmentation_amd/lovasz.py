"""Configuration of the Lovasz-Softmax loss (conf.w_lovasz, conf.lovasz_ramp_epochs, conf.lovasz_classes; build-defined: the reference's
losses hold no sort).

The supervised segmentation loss gets the term w * L of Berman et al. (CVPR 2018), the convex surrogate of the Jaccard index, here per
image and over the organ channels only: per sample and class the pixels are sorted by their error |y - p| on the device and the sorted
errors are weighted by the discrete derivative of the Jaccard loss (csrc/lovasz.hip, include/mmseg_hip.h).  lovasz_classes = 'present'
(the default, and Berman's) averages over the classes a sample holds, 'all' over every organ channel.  The weight is a
boundary.BoundaryWeight -- a ramped scalar in device memory that recorded hipGraph steps follow: the weight of epoch e is
w * min(1, (e + 1) / ramp), or w when ramp is 0."""
import math

import numpy as np

CLASSES = ('present', 'all')


def parse_conf(conf):
    """-> None (off: w_lovasz absent or 0) or (w_lovasz, lovasz_ramp_epochs, lovasz_classes); ValueError for values that mean nothing"""
    w = conf.get('w_lovasz', 0)
    ramp = conf.get('lovasz_ramp_epochs', 0)
    classes = conf.get('lovasz_classes', 'present')
    if isinstance(w, bool) or not isinstance(w, (int, float, np.integer, np.floating)) or not math.isfinite(float(w)) or float(w) < 0:
        raise ValueError('w_lovasz must be a finite number >= 0, got %r' % (w,))
    if isinstance(ramp, bool) or not isinstance(ramp, (int, np.integer)) or int(ramp) < 0:
        raise ValueError('lovasz_ramp_epochs must be an integer >= 0, got %r' % (ramp,))
    if not isinstance(classes, str) or classes not in CLASSES:
        raise ValueError("lovasz_classes must be 'present' or 'all', got %r" % (classes,))
    if float(w) == 0.0:
        if int(ramp) != 0:
            raise ValueError('lovasz_ramp_epochs = %r needs w_lovasz > 0' % (ramp,))
        return None
    return float(w), int(ramp), classes
