"""Dynamic loss scaling of the fp16 compute mode (`conf.loss_scale = 'dynamic'`; build-defined, the reference trains in fp32).

torch.cuda.amp.GradScaler semantics with power-of-two factors, so that scaling the seed gradients and unscaling the gradient arenas
stay exact: a step whose gradients hold a non-finite value is skipped (no weight update, Adam moments and iteration count unchanged)
and the scale halves (never below 1); after `growth_interval` consecutive applied steps it doubles.  BatchNorm moving statistics
updated by a skipped step's forward pass are kept, as under torch AMP.

Everything a step reads or writes lives in device memory (csrc/optim.hip, mmseg_unscale_check8 .. mmseg_loss_scale_update):
  * scale[1]  fp32, read by the seed-gradient kernels (the `_s` entry points) and the unscale pass;
  * st[4]     int32 {found_inf, growth counter, skipped steps, Adam iterations};
  * lr_table  lr_t(k) of Keras' Adam for k = 1 .. T, computed on the host in fp64 exactly as nn.Adam._lr_t and rounded to fp32 once;
              T is the first iteration from which lr_t(k) == lr in fp64, so that one table serves every iteration count.
So a step never waits for the device, and a step recorded into a hipGraph (graphs.py) replays the same state machine.
The host accessors (`scale()`, `skipped_steps()`, `iterations()`) synchronise: logging only."""
import math

import torch

from . import ops

DEFAULT_INIT = 1024.0
DEFAULT_GROWTH_INTERVAL = 2000
MAX_SCALE = 2.0 ** 127          # the largest finite power of two of fp32 (growth stops there)
_MAX_TABLE = 1 << 22


def is_power_of_two(x):
    m, _ = math.frexp(x)
    return math.isfinite(x) and x > 0 and m == 0.5


def parse_conf(conf):
    """-> None (static scale: conf.loss_scale absent or a number) or (init, growth_interval) for 'dynamic'.  Raises ValueError on
    an unknown string, an initial scale that is not a power of two in [1, 2^127], or a growth interval below 1."""
    v = conf.get('loss_scale', None)
    if not isinstance(v, str):
        return None
    if v != 'dynamic':
        raise ValueError("conf.loss_scale: %r is not a number or 'dynamic'" % (v,))
    try:
        init = float(conf.get('loss_scale_init', DEFAULT_INIT))
    except (TypeError, ValueError):
        raise ValueError('conf.loss_scale_init must be a number, got %r' % (conf.get('loss_scale_init'),))
    if not (is_power_of_two(init) and 1.0 <= init <= MAX_SCALE):
        raise ValueError('conf.loss_scale_init must be a power of two in [1, 2^127] (scaling and unscaling stay exact), got %r' % (init,))
    interval = conf.get('loss_scale_growth_interval', DEFAULT_GROWTH_INTERVAL)
    if isinstance(interval, bool) or not isinstance(interval, int) or not 1 <= interval < 2 ** 31:
        raise ValueError('conf.loss_scale_growth_interval must be a positive integer, got %r' % (interval,))
    return init, interval


def lr_table(lr, beta_1, beta_2):
    """[lr_t(1), ..., lr_t(T)] in fp64 (nn.Adam._lr_t), T = the first k with 1 - beta^k == 1 for both betas, where lr_t(k) == lr"""
    out = []
    t = 1
    while True:
        out.append(lr * math.sqrt(1. - beta_2 ** t) / (1. - beta_1 ** t))
        if 1. - beta_2 ** t == 1. and 1. - beta_1 ** t == 1.:
            return out
        t += 1
        if t > _MAX_TABLE:
            raise ValueError('Adam betas (%r, %r): the step size does not reach lr within %d iterations' % (beta_1, beta_2, _MAX_TABLE))


class LossScaler(object):
    """the device-resident scaler of one trainer (one per Adam state)"""

    def __init__(self, optimizer, device, init=DEFAULT_INIT, growth_interval=DEFAULT_GROWTH_INTERVAL):
        self.optimizer = optimizer
        self.device = torch.device(device)
        self.growth_interval = int(growth_interval)
        self.scale_dev = torch.full((1,), float(init), dtype=torch.float32, device=self.device)
        self.state = torch.zeros(4, dtype=torch.int32, device=self.device)
        # written once, here (the optimiser's lr and betas are fixed at compile time): a recorded step keeps reading this buffer
        self.lr_table = torch.tensor(lr_table(optimizer.lr, optimizer.beta_1, optimizer.beta_2), dtype=torch.float32, device=self.device)

    # ---- one step: after the gradient all-reduce, in place of the static unscale + Adam ------------------------------------------
    def unscale_(self, models):
        """every model's gradient arena *= 1 / scale; found_inf set if any element is non-finite (one launch per 8 arenas)"""
        arenas = [m.grad_arena for m in models if m.grad_arena is not None and m.grad_arena.numel() > 0]
        for i in range(0, len(arenas), 8):
            ops.unscale_check(arenas[i:i + 8], self.scale_dev, self.state)

    def step(self, models):
        """guarded Adam over every model's arena, then the scaler update"""
        opt = self.optimizer
        for m in models:
            mm, vv = opt.moments(m)
            ops.adam_guarded(m.arena, m.grad_arena, mm, vv, self.lr_table, self.state, opt.beta_1, opt.beta_2, opt.epsilon, owner=m.uid)
        ops.loss_scale_update(self.scale_dev, self.state, self.growth_interval)

    # ---- host accessors (synchronise: for logging and tests) ----------------------------------------------------------------------
    def scale(self):
        return float(self.scale_dev.item())

    def found_inf(self):
        return int(self.state[0].item())

    def growth_count(self):
        return int(self.state[1].item())

    def skipped_steps(self):
        return int(self.state[2].item())

    def iterations(self):
        return int(self.state[3].item())
