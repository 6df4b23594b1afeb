"""Drop-in for the adversarial channel-classifier branch of the reference (``--ADV_AUG``):
``model.GradientReversal`` / ``model.ChannelClassifier`` (model.py:976-1023), ``nn.CrossEntropyLoss``
as used at main_train.py:251, and the two-phase step of main_train.py:377-403 + :420-453.

Same constructors, ``state_dict`` keys (``classifier.0.*``, ``classifier.3.*``) and forward
semantics; every device computation is a HIP kernel behind the C-ABI (csrc/adv_head.hip plus the
linear kernels), one ``autograd.Function`` per module.  ``nn.Dropout(0.3)`` draws its mask on the
device (Philox4x32-10, seeded per module); tests pass an explicit mask to replay the reference's.
"""
import ctypes

import torch
import torch.distributed as td
import torch.nn as nn
import torch.nn.init as init

from . import _hip, ops
from . import dist as air_dist
from ._hip import ci, cf, csz, dptr, stream
from .hip_model import HipModel
from .train import Trainer, adjust_learning_rate


def _n(t):
    return csz(t.numel())


def dropout_mask(shape, p, seed, offset, device):
    keep = torch.empty(shape, device=device, dtype=torch.float32)
    _hip.check(_hip.lib().air_dropout_mask(dptr(keep), _n(keep), cf(p), ctypes.c_uint64(seed),
                                           ctypes.c_uint64(offset), stream()), "air_dropout_mask")
    return keep


def _mask_relu_fwd(x, keep):
    y = torch.empty_like(x)
    _hip.check(_hip.lib().air_mask_relu_fwd(dptr(x), dptr(keep, allow_none=True), _n(x), dptr(y), stream()),
               "air_mask_relu_fwd")
    return y


def _mask_relu_bwd(dy, y, keep, alpha=1.0):
    dx = torch.empty_like(dy)
    _hip.check(_hip.lib().air_mask_relu_bwd(dptr(dy), dptr(y), dptr(keep, allow_none=True), _n(dy), cf(alpha),
                                            dptr(dx), stream()), "air_mask_relu_bwd")
    return dx


def scale_(x, alpha):
    _hip.check(_hip.lib().air_scale(dptr(x), _n(x), cf(alpha), stream()), "air_scale")
    return x


class _GRLFn(torch.autograd.Function):
    """model.py:976-995: identity forward, dx = -lambda * dy."""

    @staticmethod
    def forward(ctx, x, lambda_):
        ctx.lambda_ = float(lambda_)
        return x.clone()

    @staticmethod
    def backward(ctx, g):
        return scale_(g.contiguous().clone(), -ctx.lambda_), None


class GradientReversal(nn.Module):
    def __init__(self, lambda_=1):
        super().__init__()
        self.lambda_ = lambda_

    def forward(self, x):
        if not x.is_cuda:
            raise _hip.AirError("GradientReversal HIP path needs a GPU tensor; there is no CPU fallback")
        return _GRLFn.apply(x, self.lambda_)


class _ClassifierFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, w1, b1, w2, b2, keep, lambda_):
        x = x.contiguous()
        h = _mask_relu_fwd(ops.linear_fwd(x, w1.detach(), b1.detach()), keep)  # Linear -> Dropout -> ReLU
        o = ops.linear_fwd(h, w2.detach(), b2.detach(), relu=True)            # Linear -> ReLU
        ctx.save_for_backward(x, w1, w2, h, o)
        ctx.keep, ctx.lambda_ = keep, float(lambda_)
        return o

    @staticmethod
    def backward(ctx, do):
        x, w1, w2, h, o = ctx.saved_tensors
        do_pre = _mask_relu_bwd(do.contiguous(), o, None)
        dh, dw2, db2 = ops.linear_bwd(h, w2.detach(), do_pre)
        dh_pre = _mask_relu_bwd(dh, h, ctx.keep)
        dx, dw1, db1 = ops.linear_bwd(x, w1.detach(), dh_pre)
        scale_(dx, -ctx.lambda_)  # gradient reversal (model.py:993)
        return dx, dw1, db1, dw2, db2, None, None


class ChannelClassifier(nn.Module):
    """model.py:998-1023.

    ``flatten()`` re-seats the four parameters as views of ONE fp32 block ([w1 | b1 | w2 | b2], the layout of
    air_adv_heads) with a gradient block beside it: ``state_dict`` keys, shapes and the whole-module pickle are
    unchanged, the fused heads read and write the blocks, and ``TensorAdam`` steps a head in one launch.
    ``counter(device)`` is the dropout draw's Philox offset as a device-side counter (HipModel.device_counter's rules:
    one per device, never replaced once made, folded to its value in pickles); once it exists the module forward
    draws through it too, so that fused and unfused calls, eager launches and replays walk one sequence."""

    _flat = None       # class-level defaults: a pickle of any age loads without them
    _flat_grad = None
    _grad_views = None
    _ctr = None
    _ctrs = None

    def __init__(self, enc_dim, nclasses, lambda_):
        super().__init__()
        self.grl = GradientReversal(lambda_)
        self.classifier = nn.Sequential(nn.Linear(enc_dim, enc_dim // 2),
                                        nn.Dropout(0.3),
                                        nn.ReLU(),
                                        nn.Linear(enc_dim // 2, nclasses),
                                        nn.ReLU())
        self._seed = int(torch.initial_seed()) & 0x7FFFFFFFFFFFFFFF
        self._offset = 0

    def initialize_params(self):
        for layer in self.modules():
            if isinstance(layer, torch.nn.Linear):
                init.kaiming_uniform_(layer.weight)

    def forward(self, x, keep=None):
        """x (B, enc_dim) GPU features.  ``keep``: optional explicit dropout keep-mask (B, enc_dim//2),
        already scaled by 1/(1-p); default: drawn on the device in training mode, none in eval."""
        if not x.is_cuda:
            raise _hip.AirError("ChannelClassifier HIP path needs a GPU tensor; there is no CPU fallback")
        l1, l2 = self.classifier[0], self.classifier[3]
        if x.dim() != 2 or x.shape[1] != l1.in_features:
            raise ValueError("expected (B, %d) features, got %s" % (l1.in_features, tuple(x.shape)))
        p = self.classifier[1].p
        if keep is None and self.training and p > 0:
            if self._ctr is not None:
                keep = ops.dropout_mask_ctr((x.shape[0], l1.out_features), p, self._seed, self.counter(x.device), x.device)
            else:
                keep = dropout_mask((x.shape[0], l1.out_features), p, self._seed, self._offset, x.device)
                self._offset += (x.shape[0] * l1.out_features + 3) // 4
        return _ClassifierFn.apply(x.float(), l1.weight, l1.bias, l2.weight, l2.bias, keep, self.grl.lambda_)


    # ------------------------------------------------------------------ flat storage, device counter
    def _flat_params(self):
        l1, l2 = self.classifier[0], self.classifier[3]
        return [l1.weight, l1.bias, l2.weight, l2.bias]

    def flatten(self):
        """The parameter block (built on first use, rebuilt when .to() moved the parameters)."""
        params = self._flat_params()
        flat, off, ok = self._flat, 0, self._flat is not None
        for p in params:
            ok = ok and p.device == flat.device and p.data_ptr() == flat.data_ptr() + 4 * off and p.is_contiguous()
            off += p.numel()
        if ok:
            return flat
        flat = torch.cat([p.detach().reshape(-1).float() for p in params])
        off = 0
        for p in params:
            p.data = flat[off:off + p.numel()].view(p.shape)
            off += p.numel()
        self._flat, self._flat_grad, self._grad_views = flat, None, None
        return flat

    def flat_grad(self, block=None):
        """The gradient block (``block``: a slice of a larger one - the trainer keeps all heads' in one tensor for
        one all-reduce)."""
        flat = self.flatten()
        if block is not None or self._flat_grad is None or self._flat_grad.device != flat.device:
            self._flat_grad = block if block is not None else torch.zeros_like(flat)
            off, views = 0, []
            for p in self._flat_params():
                views.append(self._flat_grad[off:off + p.numel()].view(p.shape))
                off += p.numel()
            self._grad_views = views
        return self._flat_grad

    def point_grads(self):
        """p.grad = the views of the gradient block (what the fused heads wrote)."""
        self.flat_grad()
        for p, v in zip(self._flat_params(), self._grad_views):
            if p.grad is not v:
                p.grad = v

    def grads_are_flat(self):
        return self._grad_views is not None and all(p.grad is v for p, v in zip(self._flat_params(), self._grad_views))

    def counter(self, device):
        return HipModel.device_counter(self, "", torch.device(device))

    def head(self):
        """This classifier as ``ops.adv_heads`` takes it; the dropout probability is the one in force (0 in eval mode)."""
        flat = self.flatten()
        p = float(self.classifier[1].p) if self.training else 0.0
        return ops.AdvHead(flat, self.flat_grad(), self.classifier[3].out_features, p=p, seed=self._seed,
                           counter=self.counter(flat.device) if p > 0 else None)

    def _apply(self, fn, *args, **kw):
        was_flat = self._flat is not None
        out = super()._apply(fn, *args, **kw)
        if was_flat:
            self.flatten()
        return out

    def __getstate__(self):
        st = dict(self.__dict__)
        HipModel.fold_counter(st, "")
        st["_flat_grad"] = st["_grad_views"] = None
        return st


class _CEFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logits, labels, owner):
        logits = logits.contiguous()
        B, C = logits.shape
        probs = torch.empty_like(logits)
        loss = torch.empty((), device=logits.device, dtype=torch.float32)
        correct = torch.empty((), device=logits.device, dtype=torch.int32)
        _hip.check(_hip.lib().air_softmax_ce_fwd(dptr(logits), dptr(labels, torch.int64), ci(B), ci(C), dptr(probs),
                                                 dptr(loss), dptr(correct, torch.int32), stream()),
                   "air_softmax_ce_fwd")
        ctx.save_for_backward(probs, labels)
        owner.last_correct = correct
        return loss

    @staticmethod
    def backward(ctx, g):
        probs, labels = ctx.saved_tensors
        B, C = probs.shape
        d = torch.empty_like(probs)
        _hip.check(_hip.lib().air_softmax_ce_bwd(dptr(probs), dptr(labels, torch.int64), ci(B), ci(C),
                                                 dptr(g.reshape(1).float().contiguous()), dptr(d), stream()),
                   "air_softmax_ce_bwd")
        return d, None, None


class CrossEntropyLoss(nn.Module):
    """nn.CrossEntropyLoss() with default arguments (main_train.py:251): mean over the batch.
    ``last_correct`` holds #(argmax == label) of the last call as a GPU scalar (the accuracy
    counters of main_train.py:383-385 without a second pass over the logits)."""

    def __init__(self):
        super().__init__()
        self.last_correct = None

    def forward(self, logits, labels):
        if not logits.is_cuda:
            raise _hip.AirError("CrossEntropyLoss HIP path needs GPU tensors; there is no CPU fallback")
        if logits.dim() != 2:
            raise ValueError("expected (B, C) logits")
        labels = labels.to(device=logits.device, dtype=torch.int64).contiguous()
        return _CEFn.apply(logits.float(), labels, self)


class TensorAdam:
    """torch.optim.Adam(module.parameters(), lr, betas, eps, weight_decay) as configured for the
    classifiers at main_train.py:215-216 (lr_d = 1e-4, coupled L2 5e-4): one fused launch per tensor."""

    def __init__(self, module, lr=1e-4, betas=(0.9, 0.999), eps=1e-8, weight_decay=5e-4):
        self.params = list(module.parameters())
        self.module = module if isinstance(module, ChannelClassifier) else None
        self.flat_state = None
        self.param_groups = [{"lr": lr, "betas": betas, "eps": eps, "weight_decay": weight_decay}]
        self.step_count = 0
        self.state = {}

    def zero_grad(self, set_to_none=True):
        for p in self.params:
            p.grad = None

    def step(self, grad_scale=1.0):
        g = self.param_groups[0]
        self.step_count += 1
        mod = self.module
        if mod is not None and mod._flat is not None:
            # flat storage: the moments are one block too; a head whose gradients are the views of its gradient block
            # (the fused heads) is stepped in ONE launch - the same per-element arithmetic as one launch per tensor
            flat = mod.flatten()
            if self.flat_state is None or self.flat_state[0].device != flat.device:
                self._adopt_flat(flat)
            if mod.grads_are_flat():
                ops.adam_step(flat, mod._flat_grad, self.flat_state[0], self.flat_state[1], self.step_count, g["lr"],
                              g["betas"][0], g["betas"][1], g["eps"], g["weight_decay"], grad_scale)
                return
        for p in self.params:
            if p.grad is None:
                continue
            st = self.state.get(id(p))
            if st is None:
                st = self.state[id(p)] = (torch.zeros_like(p.data).view(-1), torch.zeros_like(p.data).view(-1))
            ops.adam_step(p.data.view(-1), p.grad.contiguous().view(-1), st[0], st[1], self.step_count, g["lr"],
                          g["betas"][0], g["betas"][1], g["eps"], g["weight_decay"], grad_scale)

    def _adopt_flat(self, flat):
        """Moments as one block laid out like the parameters; ``state`` holds views of it (what was there is kept)."""
        m, v = torch.zeros_like(flat), torch.zeros_like(flat)
        off = 0
        for p in self.params:
            n = p.numel()
            old = self.state.get(id(p))
            if old is not None:
                m[off:off + n].copy_(old[0])
                v[off:off + n].copy_(old[1])
            self.state[id(p)] = (m[off:off + n], v[off:off + n])
            off += n
        self.flat_state = (m, v)


class AdversarialTrainer(Trainer):
    """The ``--ADV_AUG`` train step (main_train.py:375-409 + :420-453).

    ``n_channels``: int (LA_aug / DF_aug: one classifier over ``channels (B,)``) or a tuple
    (LAPA_aug / DFPA_aug: codec and device classifiers over ``channels (B, 2)``).
    ``recompute=True`` is the reference's behaviour: after the encoder update the batch goes
    through the encoder AGAIN (train mode: BatchNorm statistics are updated a second time) to
    train the classifiers on detached features.  ``recompute=False`` trains them on the detached
    features of the first forward (one encoder forward per step instead of two: a deliberate,
    documented deviation).

    ``fused_heads``: all classifier heads of a phase in ONE ``air_adv_heads`` launch (forward, cross-entropy, accuracy
    count, backward, the reversed gradient) instead of the module chain under autograd.  ``None``: fused exactly when
    ``enable_graph()`` is on - the step is then two hipGraph replays, phase 1 (front-end, encoder forward, OC-Softmax
    head, the heads with their reversed gradient, encoder backward) and phase 2 (second forward, the heads), with the
    optimisers between and behind them; ``True``: fused on the eager step too; ``False``: never (``enable_graph()``
    then leaves steps with ``channels`` eager).  The fused path serves the ``ang_iso`` head, the only one the
    reference applies ``--ADV_AUG`` to (main_train.py:374-377).

    ``last``: ``adv_loss``, ``classifier_loss``, and ``correct_m`` / ``correct_c`` - head 0's #(argmax == channel) of
    phase 1 / phase 2 as device int32 scalars; ``epoch_accuracy()`` is their running percentage since ``set_epoch``."""

    def __init__(self, model, n_channels, lambda_=0.05, lr_d=1e-4, recompute=True, fused_heads=None, **kw):
        super().__init__(model, **kw)
        counts = (n_channels,) if isinstance(n_channels, int) else tuple(n_channels)
        if fused_heads and self.add_loss != "ang_iso":
            raise ValueError("fused_heads serves the ang_iso head only")
        enc_dim = self.loss.feat_dim
        self.classifiers = [ChannelClassifier(enc_dim, n, lambda_).to(self.device) for n in counts]
        if self.world > 1:  # same classifier replicas everywhere (the encoder is synchronised by Trainer)
            for c in self.classifiers:
                for t in list(c.parameters()) + list(c.buffers()):
                    td.broadcast(t.data, src=0)
        # flat storage: one parameter block per classifier, and ONE gradient tensor for all of them (one all-reduce)
        sizes = [c.flatten().numel() for c in self.classifiers]
        self._cls_grad = torch.zeros(sum(sizes), device=self.device, dtype=torch.float32)
        off = 0
        for c, n in zip(self.classifiers, sizes):
            c.flat_grad(self._cls_grad[off:off + n])
            off += n
        self.classifier_optimizers = [TensorAdam(c, lr=lr_d) for c in self.classifiers]
        self.criterion = CrossEntropyLoss()
        self.lr_d = lr_d
        self.recompute = recompute
        self.fused_heads = fused_heads
        self.last = {}
        # running #(argmax == channel) per phase and head on the device (the fused heads add to it in-kernel), and the
        # rows they were counted over on the host
        self._run = torch.zeros(2, len(counts), dtype=torch.int64, device=self.device)
        self._seen = [0, 0]
        self._adv_ctx = None   # (channels, adversarial term on) of the step _graphed_step is serving
        self._cap1 = None

    def set_epoch(self, epoch_num, lr_decay=0.5, interval=30):
        super().set_epoch(epoch_num, lr_decay, interval)
        for opt in self.classifier_optimizers:  # main_train.py:301-306
            adjust_learning_rate(self.lr_d, opt, epoch_num, lr_decay, interval)
        self._run.zero_()  # correct_m / correct_c, total_m / total_c start over (main_train.py:383-385, :427-429)
        self._seen = [0, 0]

    def epoch_accuracy(self):
        """(acc_1, acc_2) in percent: head 0's 100 * correct / total of phase 1 and phase 2 since ``set_epoch`` - the two
        accuracy columns of main_train.py:475-476.  One synchronisation, only when called."""
        run = self._run[:, 0].cpu()
        return tuple(100.0 * int(run[ph]) / self._seen[ph] if self._seen[ph] else 0.0 for ph in (0, 1))

    def _fused(self):
        if self.fused_heads is None:
            return self.use_graph and self.add_loss == "ang_iso"
        return bool(self.fused_heads)

    def _targets(self, channels):
        channels = channels.to(self.device)
        if len(self.classifiers) == 1:
            return [channels.reshape(-1)]
        return [channels[:, i].contiguous() for i in range(len(self.classifiers))]

    def step_features(self, feat, labels, channels=None, epoch_num=1):
        if channels is None:
            return super().step_features(feat, labels)
        if self._fused():
            return self._fused_step_features(feat, labels, channels, epoch_num)
        targets = self._targets(channels)
        self.model.train()
        for c in self.classifiers:
            c.train()
        self.feat_optimizer.zero_grad()
        self.loss_optimizer.zero_grad()
        feats, _ = self.model(feat)
        loss, neg_scores = self.loss(feats, labels)
        feat_loss = loss * self.weight_loss
        adv = None
        correct_m = None
        if epoch_num > 0:  # main_train.py:377
            for c, tgt in zip(self.classifiers, targets):
                l = self.criterion(c(feats), tgt)
                if correct_m is None:
                    correct_m = self.criterion.last_correct
                adv = l if adv is None else adv + l
            feat_loss = feat_loss + adv
        feat_loss.backward()
        scale = 1.0
        if self.world > 1:  # encoder + centre gradients are averaged over ranks
            air_dist.allreduce_grads(self.model, self.loss)
            scale = 1.0 / self.world
        self.feat_optimizer.step(grad_scale=scale)
        self.loss_optimizer.step(grad_scale=scale)
        # phase 2 (main_train.py:420-453): train the classifiers on detached features
        if self.recompute:
            with torch.no_grad():
                feats2 = self.model(feat)[0]
        else:
            feats2 = feats.detach()
        closs = []
        correct_c = None
        for c, opt, tgt in zip(self.classifiers, self.classifier_optimizers, targets):
            lc = self.criterion(c(feats2.detach()), tgt)
            if correct_c is None:
                correct_c = self.criterion.last_correct
            opt.zero_grad()
            lc.backward()
            if self.world > 1:
                # the classifiers are replicas too: without this every rank would train its own, and the
                # gradient-reversal term each rank feeds its encoder would drift apart
                works = [td.all_reduce(p.grad, op=td.ReduceOp.SUM, async_op=True)
                         for p in c.parameters() if p.grad is not None]
                for w in works:
                    w.wait()
            opt.step(grad_scale=scale)
            closs.append(lc.detach())
        if correct_m is None:
            correct_m = torch.zeros_like(correct_c)
        else:
            self._run[0, 0] += correct_m
            self._seen[0] += feat.shape[0]
        self._run[1, 0] += correct_c
        self._seen[1] += feat.shape[0]
        self.last = {"adv_loss": None if adv is None else adv.detach(), "classifier_loss": closs,
                     "correct_m": correct_m, "correct_c": correct_c}
        return loss.detach(), neg_scores

    # ------------------------------------------------------------------ fused heads: the two phases as plain calls
    def _heads(self):
        for c in self.classifiers:
            if not c.training:
                c.train()
        return [c.head() for c in self.classifiers]

    def _phase1(self, feat, labels, targets, adv_on):
        """Encoder forward, OC-Softmax head, the fused heads with their reversed gradient (``adv_on``: epoch_num > 0,
        main_train.py:377), encoder backward - in THIS thread, without autograd around the model (capturable)."""
        model = self.model
        feats, saved = model.forward_saved(feat)
        leaf = feats.detach().requires_grad_(True)
        loss, bwd, neg = self._head(leaf, None, labels)
        bwd.backward()  # the head only: weight_loss * d(ocsoftmax) / d(feats) and the centre's gradient
        dfeat = leaf.grad
        adv = correct = None
        if adv_on:
            losses, correct, dx = ops.adv_heads(leaf.detach(), self._heads(), targets, self.classifiers[0].grl.lambda_,
                                                True, run_correct=self._run[0])
            ops.add_(dfeat, dx)
            adv = losses[0]
            for k in range(1, len(self.classifiers)):
                adv = adv + losses[k]
        grads = model.backward_saved(saved, dfeat)
        pairs = []
        for (n, p, _, _), gr in zip(model.arena().entries, grads):
            if gr is not None:
                p.grad = gr
                pairs.append((p, gr))
        pairs += [(p, p.grad) for p in self._loss_params() if p.grad is not None]
        return dict(loss=loss.detach(), neg=neg, adv=adv, correct=correct, feat=feat, feats=leaf.detach(), pairs=pairs)

    def _phase2(self, feat, feats1, targets):
        """main_train.py:420-453 up to the classifier optimisers: the second train-mode forward (``recompute``) or the
        detached features of phase 1, then the fused heads without the reversed gradient."""
        if self.recompute:
            with torch.no_grad():
                feats2 = self.model(feat)[0]
        else:
            feats2 = feats1
        losses, correct, _ = ops.adv_heads(feats2.float().contiguous(), self._heads(), targets,
                                           self.classifiers[0].grl.lambda_, False, run_correct=self._run[1])
        return dict(losses=losses, correct=correct)

    def _exchange_and_optimise(self):
        scale = 1.0
        if self.world > 1:
            air_dist.allreduce_grads(self.model, self.loss)
            scale = 1.0 / self.world
        self._optimise(scale)
        return scale

    def _step_classifiers(self, scale):
        """Behind phase 2: ONE all-reduce over all heads' gradients (world > 1), one Adam launch per head."""
        if self.world > 1:
            td.all_reduce(self._cls_grad, op=td.ReduceOp.SUM)
        for c, opt in zip(self.classifiers, self.classifier_optimizers):
            c.point_grads()
            opt.step(grad_scale=scale)

    def _set_last(self, p1, p2, rows, copy):
        keep = (lambda t: t.clone()) if copy else (lambda t: t)  # (a replay's outputs are overwritten by the next)
        n = len(self.classifiers)
        zero = None
        if p1["correct"] is None:
            zero = torch.zeros((), dtype=torch.int32, device=self.device)
        else:
            self._seen[0] += rows
        self._seen[1] += rows
        losses = keep(p2["losses"])
        self.last = {"adv_loss": None if p1["adv"] is None else keep(p1["adv"]),
                     "classifier_loss": [losses[k] for k in range(n)],
                     "correct_m": zero if zero is not None else keep(p1["correct"])[0],
                     "correct_c": keep(p2["correct"])[0]}

    def _fused_step_features(self, feat, labels, channels, epoch_num):
        if self.add_loss != "ang_iso":
            raise ValueError("fused_heads serves the ang_iso head only")
        targets = self._targets(channels)
        if not self.model.training:
            self.model.train()
        self._zero_grads()
        p1 = self._phase1(feat, labels, targets, epoch_num > 0)
        scale = self._exchange_and_optimise()
        p2 = self._phase2(feat, p1["feats"], targets)
        self._step_classifiers(scale)
        self._set_last(p1, p2, feat.shape[0], copy=False)
        return p1["loss"], p1["neg"]

    # ------------------------------------------------------------------ hipGraph replay (Trainer's machinery, two phases)
    def _graph_key(self, pcm, labels, ragged=False):
        key = super()._graph_key(pcm, labels, ragged)
        ctx = self._adv_ctx
        if ctx is None:
            return key
        channels, adv_on = ctx
        return key + ("adv", tuple(c.classifier[3].out_features for c in self.classifiers),
                      tuple(float(c.grl.lambda_) for c in self.classifiers),
                      tuple(float(c.classifier[1].p) for c in self.classifiers), bool(self.recompute), bool(adv_on),
                      tuple(channels.shape))

    def _static_targets(self, channels):
        """The captured step's channel labels: an int64 (heads, B) buffer (one contiguous row per head)."""
        channels = channels.to(self.device, non_blocking=True)
        return channels.reshape(1, -1) if len(self.classifiers) == 1 else channels.t()

    def _capture(self, key, pcm, labels, lengths=None, start=None):
        if self._adv_ctx is not None:
            self._adv_static = self._static_targets(self._adv_ctx[0]).to(torch.int64).contiguous().clone()
        return super()._capture(key, pcm, labels, lengths, start)

    def _fwd_bwd_direct(self, pcm, labels, lengths=None, start=None):
        ctx = self._adv_ctx
        if ctx is None:
            return super()._fwd_bwd_direct(pcm, labels, lengths, start)
        targets = [self._adv_static[k] for k in range(len(self.classifiers))]
        p1 = self._cap1 = self._phase1(self.features(pcm, start, lengths), labels, targets, ctx[1])
        return p1["loss"], p1["neg"], p1["pairs"]

    def _capture_tail(self, captured):
        if self._adv_ctx is None:
            return None
        p1, self._cap1 = self._cap1, None
        targets = [self._adv_static[k] for k in range(len(self.classifiers))]
        graph, p2 = captured(lambda: self._phase2(p1["feat"], p1["feats"], targets))
        return dict(graph=graph, p1=p1, p2=p2, channels=self._adv_static)

    def _refresh_tail(self, g):
        if g["tail"] is not None:
            g["tail"]["channels"].copy_(self._static_targets(self._adv_ctx[0]), non_blocking=True)

    def _replay_tail(self, g, scale):
        tail = g["tail"]
        if tail is None:
            return
        tail["graph"].replay()
        self._step_classifiers(scale)
        self._set_last(tail["p1"], tail["p2"], g["pcm"].shape[0], copy=True)

    def step(self, pcm, labels, channels=None, start=None, epoch_num=1, lengths=None):
        """``lengths``: int32 (B,), a ragged batch as in ``Trainer.step``.  With ``enable_graph()`` and fused heads a
        step with ``channels`` replays two captured phases (the augmentation stays in front of the captured region; a
        ``start`` without ``lengths`` forces the eager step, as in ``Trainer.step``); a step without ``channels`` is
        ``Trainer``'s eager step."""
        self._refuse_ragged_augment(lengths)
        if lengths is not None and self.augment is not None:
            lengths = self._ragged_lengths(lengths, pcm)
        pcm = self._augment(pcm, lengths)
        if channels is not None and self.use_graph and self._fused() and (start is None or lengths is not None):
            self._adv_ctx = (torch.as_tensor(channels), epoch_num > 0)
            try:
                out = self._graphed_step(pcm, labels, lengths, start)
            finally:
                self._adv_ctx = None
            if out is not None:
                return out
        return self.step_features(self.features(pcm, start, lengths), labels, channels, epoch_num)
