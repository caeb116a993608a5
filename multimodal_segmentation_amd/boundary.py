"""Weight of the boundary loss (conf.w_boundary, conf.boundary_ramp_epochs; build-defined: the reference's losses hold no distance).

The supervised segmentation loss gets the term w * L_B of Kervadec et al. (MIDL 2019), L_B = mean(p * phi) over the organ channels with
phi the signed distance map of the ground truth (csrc/boundary.hip).  The weight lives in device memory: the kernels read it, so a step
recorded into a hipGraph follows a weight the host changes between replays.  The paper's "increase" schedule: the weight of epoch e is
w * min(1, (e + 1) / ramp), or w when ramp is 0 -- a large boundary weight from the first step does not train."""
import math

import numpy as np
import torch


def parse_conf(conf):
    """-> None (off: w_boundary absent or 0) or (w_boundary, boundary_ramp_epochs); ValueError for values that mean nothing"""
    w = conf.get('w_boundary', 0)
    ramp = conf.get('boundary_ramp_epochs', 0)
    if isinstance(w, bool) or not isinstance(w, (int, float, np.integer, np.floating)) or not math.isfinite(float(w)) or float(w) < 0:
        raise ValueError('w_boundary must be a finite number >= 0, got %r' % (w,))
    if isinstance(ramp, bool) or not isinstance(ramp, (int, np.integer)) or int(ramp) < 0:
        raise ValueError('boundary_ramp_epochs must be an integer >= 0, got %r' % (ramp,))
    if float(w) == 0.0:
        if int(ramp) != 0:
            raise ValueError('boundary_ramp_epochs = %r needs w_boundary > 0' % (ramp,))
        return None
    return float(w), int(ramp)


class BoundaryWeight(object):
    def __init__(self, device, w_boundary, ramp_epochs=0):
        self.w, self.ramp = float(w_boundary), int(ramp_epochs)
        self.device = torch.device(device)
        self.weight_dev = torch.zeros(1, dtype=torch.float32, device=self.device)
        self.value = None
        self.set_epoch(0)

    def weight_of_epoch(self, epoch):
        return self.w if self.ramp == 0 else self.w * min(1.0, (epoch + 1) / float(self.ramp))

    def set(self, value):
        """asynchronous copy of the value into the one buffer the kernels read"""
        from . import nn
        self.value = float(value)
        self.weight_dev.copy_(nn.host_to_device(np.asarray([self.value], np.float32), self.device), non_blocking=True)

    def set_epoch(self, epoch):
        self.set(self.weight_of_epoch(int(epoch)))
