"""A compiled Keras "trainer" model: a forward graph over shared component models + a per-output loss table + one
Adam state.  `fit(inputs, targets)` performs exactly what `keras.Model.fit(..., epochs=1)` does for one batch
(batch_size 32 >= the batch, so one optimiser step): forward in training mode (BatchNorm batch statistics, moving
averages updated), weighted sum of the per-output losses (+ the layers' regulariser losses), gradients of the
trainable weights collected at compile time, one Adam update, History with '<output_name>_loss' entries.

Loss kinds (reference costs.py / keras): 'dice_bce' (make_combined_dice_bce), 'dice' (make_dice_loss_fnc), 'mse',
'mae', 'ypred' (mean of the output).
"""
import torch

from .. import graphs, nn, ops
from ..parallel import dp


class OutputSpec(object):
    __slots__ = ('name', 'kind', 'weight')

    def __init__(self, name, kind, weight):
        self.name, self.kind, self.weight = name, kind, float(weight)


class Trainer(object):
    def __init__(self, name, graph_fn, output_specs, train_models, optimizer, num_masks=None, regularised=(),
                 all_models=()):
        """graph_fn(inputs: list of device tensors) -> list of output tensors (len == len(output_specs)).
        train_models: nn.Models whose arenas this trainer updates (the weights that were trainable at compile time).
        regularised: DiscriminatorModels whose Spectral penalties are part of this trainer's total loss."""
        self.name = name
        self.graph_fn = graph_fn
        self.specs = list(output_specs)
        self.train_models = list(train_models)
        self.optimizer = optimizer
        self.num_masks = num_masks
        self.regularised = list(regularised)
        self.all_models = list(all_models) or self.train_models
        self.device = self.train_models[0].device
        self.last_outputs = None
        # conf.hip_graphs: record the step into a hipGraph after two eager warm-up steps and replay it from then on (graphs.py)
        self.use_graph = False
        self._graphs = {}
        # static loss scale (fp16 compute mode): every seed gradient is multiplied by it, the gradient arenas are divided by it
        # before the optimiser step; 1.0 = off
        self.loss_scale = 1.0
        # conf.loss_scale = 'dynamic' (fp16): a loss_scaler.LossScaler owning the device-resident scale, the skipped-step logic and
        # this trainer's Adam iteration count; the seeds are then multiplied by its device scale (loss_scale stays 1.0).  None = static
        self.scaler = None
        # (compute_dtype, 16-bit activation storage) of the model wrapper this trainer belongs to: every fit / predict runs inside
        # ops.precision_scope(self.precision); None = whatever the library is set to
        self.precision = None
        # conf.w_boundary > 0 (build-defined): the boundary.BoundaryWeight whose device weight the boundary term of every Dice output is
        # multiplied with (csrc/boundary.hip); None = off, none of those kernels is launched
        self.boundary = None
        self._prepared, self._phi = None, None            # per fit: targets by identity -> device tensor -> distance map
        # conf.w_lovasz > 0 (build-defined): the device weight (a boundary.BoundaryWeight, the generic ramped device scalar) of the
        # Lovasz-Softmax term of every Dice output (csrc/lovasz.hip), and conf.lovasz_classes == 'all'; None = off, no launch
        self.lovasz = None
        self.lovasz_all = False

    # keras API used by the executors ---------------------------------------------------------------------------
    @property
    def output_names(self):
        return [s.name for s in self.specs]

    def summary(self, print_fn=print):
        print_fn('Trainer %s: %d outputs, trainable models: %s' % (self.name, len(self.specs),
                                                                   ', '.join(m.name for m in self.train_models)))

    def _loss_and_grad(self, spec, pred, target, hist=None):
        gs = spec.weight * self.loss_scale            # scale of the returned gradient only; the loss value is unscaled
        sd = self.scaler.scale_dev if self.scaler is not None else None     # dynamic: times the device scale
        if spec.kind == 'dice_bce':
            out = ops.seg_loss(pred, target, self.num_masks, 0.01, gs, class_sum_hook=dp.class_sum_hook(),
                               n_pix_global=pred.numel() // pred.shape[-1] * dp.world_size(), scale_dev=sd)
            return self._add_terms(spec, pred, target, out, gs, sd, hist)
        if spec.kind == 'dice':
            out = ops.seg_loss(pred, target, self.num_masks, 0.0, gs, scale_dev=sd)
            return self._add_terms(spec, pred, target, out, gs, sd, hist)
        if spec.kind == 'mse':
            return ops.diff_loss(pred, target, 'mse', gs, scale_dev=sd)
        if spec.kind == 'mae':
            return ops.diff_loss(pred, target, 'mae', gs, scale_dev=sd)
        if spec.kind == 'ypred':
            return ops.diff_loss(pred, 0.0, 'mean', gs, scale_dev=sd)
        raise ValueError(spec.kind)

    def _add_terms(self, spec, pred, target, out, gs, sd, hist):
        """the optional terms of a Dice output, in a fixed order: boundary, then Lovasz (each nothing when off)"""
        if self.boundary is not None:
            out = self._add_boundary(spec, pred, target, out, gs, sd, hist)
        if self.lovasz is not None:
            out = self._add_lovasz(spec, pred, target, out, gs, sd, hist)
        return out

    def _add_lovasz(self, spec, pred, target, out, gs, sd, hist):
        """+ weight * L of the Lovasz-Softmax loss (per image, organ channels): the signed map m of this prediction (a device sort per
        sample and class; it depends on the prediction, so it is built per output), the term sum m (p - y), its gradient m added into
        what seg_loss (and the boundary term) wrote, the weighted term added into the loss value; the raw term goes into the History
        as '<name>_lovasz'.  q_b holds the local batch size (the data-parallel all-reduce averages over ranks) and the recorded term is
        rank-local, as for the boundary term."""
        loss, dpred = out
        w = self.lovasz.weight_dev
        m = ops.lovasz_map(pred, target, self.num_masks, self.lovasz_all)
        loss_l = ops.lovasz_term(pred, target, m, self.num_masks)
        if dpred is not None:
            ops.lovasz_grad_add(m, dpred, self.num_masks, gs, w, scale_dev=sd)
        ops.boundary_combine(loss, loss_l, w)
        if hist is not None:
            hist.record(spec.name + '_lovasz', loss_l)
        return loss, dpred

    def _add_boundary(self, spec, pred, target, out, gs, sd, hist):
        """the segmentation loss of one output + weight * L_B: the map of the target (built once per distinct target of a fit), the term,
        its gradient added into what seg_loss wrote, the weighted term added into the loss value; the raw term goes into the History
        as '<name>_boundary'.  The gradient is normalised by the local element count (the data-parallel all-reduce averages over ranks)
        and the recorded term is rank-local, as for 'mae' / 'mse'."""
        loss, dpred = out
        cache = self._phi if self._phi is not None else {}
        ent = cache.get(id(target))
        if ent is None:
            ent = cache[id(target)] = (target, ops.boundary_map(target, self.num_masks))      # (the target is held: its id stays its own)
        phi = ent[1]
        w = self.boundary.weight_dev
        loss_b = ops.boundary_term(pred, phi, self.num_masks)
        if dpred is not None:
            ops.boundary_grad_add(phi, dpred, self.num_masks, gs, w, scale_dev=sd)
        ops.boundary_combine(loss, loss_b, w)
        if hist is not None:
            hist.record(spec.name + '_boundary', loss_b)
        return loss, dpred

    def _prep_target(self, t, pred):
        if isinstance(t, (int, float)):
            return float(t)
        if self._prepared is not None:                # boundary loss: outputs that share a target object share its device tensor
            key = (id(t), tuple(pred.shape))
            ent = self._prepared.get(key)
            if ent is None:
                ent = self._prepared[key] = (t, self._prep_tensor(t, pred))
            return ent[1]
        return self._prep_tensor(t, pred)

    def _prep_tensor(self, t, pred):
        t = nn.to_device(t, self.device)
        if t.numel() != pred.numel():
            # keras broadcasts e.g. zeros(batch) targets against [batch, 1] outputs
            t = t.reshape(-1, *([1] * (pred.dim() - 1))).expand_as(pred).contiguous()
        return t

    def fit(self, inputs, targets, epochs=1, verbose=0, **graph_kw):
        assert epochs == 1
        inputs = list(inputs) if isinstance(inputs, (list, tuple)) else [inputs]
        targets = list(targets) if isinstance(targets, (list, tuple)) else [targets]
        graph_kw = {k: v for k, v in graph_kw.items() if v is not None}      # (eps=None etc.: the graph functions' defaults)
        with ops.precision_scope(self.precision):
            if self.use_graph and not graph_kw and not dp.enabled() and self.device.type == 'cuda':
                key = graphs.signature(inputs, targets)
                if self.boundary is not None:         # which targets are one object: the recording shares their buffer (and their map)
                    key = key + (graphs.aliases(targets),)
                st = self._graphs.get(key)
                if st is None:
                    st = self._graphs[key] = graphs.FitGraph(self)
                return st.run(inputs, targets)
            return self._fit_eager(inputs, targets, graph_kw)

    @staticmethod
    def _total(terms):
        return nn_total(terms)

    def _fit_eager(self, inputs, targets, graph_kw, lr_dev=None):
        ins = [nn.to_device(x, self.device) for x in inputs]
        assert len(targets) == len(self.specs), '%s: %d targets for %d outputs' % (self.name, len(targets), len(self.specs))
        for m in self.train_models:
            m.zero_grad_own()
        # data parallel: arenas are all-reduced as soon as their last gradient kernel is queued (overlap with backward);
        # models that also receive regulariser gradients after the backward pass are reduced at the end
        tracker = dp.begin(self.train_models, defer=[d for d in self.regularised if d in self.train_models])
        if self.boundary is not None:
            self._prepared, self._phi = {}, {}
        with torch.enable_grad():
            outs = self.graph_fn(ins, **graph_kw)
            assert len(outs) == len(self.specs)
            hist = nn.History()
            grads, terms = [], []
            for spec, pred, tgt in zip(self.specs, outs, targets):
                loss, dpred = self._loss_and_grad(spec, pred, self._prep_target(tgt, pred), hist)
                grads.append(dpred)
                terms.append((spec.weight, loss))
                hist.record(spec.name + '_loss', loss)
            torch.autograd.backward(outs, grads)
        self._prepared, self._phi = None, None
        for d in self.regularised:
            kw = {} if self.scaler is None else {'grad_scale_dev': self.scaler.scale_dev}
            for loss in d.regulariser_losses(accumulate_grad=d in self.train_models, grad_scale=self.loss_scale, **kw):
                terms.append((1.0, loss))
        dp.finish(tracker)
        if self.scaler is not None:
            # dynamic loss scale: unscale + non-finite check AFTER the all-reduce (every rank sees the same arenas and skips together),
            # then Adam guarded by the device flag and the scaler update -- no host read
            self.scaler.unscale_(self.train_models)
            self.scaler.step(self.train_models)
        else:
            if self.loss_scale != 1.0:
                for m in self.train_models:
                    ops.axpby(m.grad_arena, m.grad_arena, 1.0 / self.loss_scale, 0.0, out=m.grad_arena)
            self.optimizer.step(self.train_models, lr_dev=lr_dev)
        hist.record('loss', nn_total(terms))
        self.last_outputs = [o.detach() for o in outs]
        return hist

    def predict(self, inputs, **graph_kw):
        ins = [nn.to_device(x, self.device) for x in (inputs if isinstance(inputs, (list, tuple)) else [inputs])]
        with torch.no_grad(), ops.precision_scope(self.precision):
            outs = self.graph_fn(ins, training=False, **graph_kw)
        return [nn.to_numpy(o) for o in outs]


class nn_total(object):
    """Lazy weighted sum of device scalars (read with .item(), like a 0-d tensor)."""

    def __init__(self, terms):
        self.terms = terms

    def item(self):
        return float(sum(w * float(t.item()) for w, t in self.terms))
