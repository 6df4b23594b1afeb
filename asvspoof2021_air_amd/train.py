"""Train step of the hot path (main_train.py:310-415):

    PCM --fused HIP LFCC (+repeat-pad/chop, transposed)--> (B,1,60,feat_len)
        --ResNet / ECAPA / LCNN / Res2Net forward--> (feat, logits) --loss head--> loss
        --backward--> gradient arena --[RCCL all-reduce]--> Adam(model) + SGD(head parameter)

``Trainer`` sequences the drop-in modules exactly like the reference's loop:
zero_grad x2, loss.backward(), feat_optimizer.step(), <head>_optimizer.step()
(main_train.py:352-415), LR = lr0 * decay^(epoch // interval) (main_train.py:144-147).

The head is ``add_loss`` (main_train.py:66-67, :250-300): ``"ang_iso"`` (OC-Softmax, the default here),
``None`` (the reference's default: cross-entropy on the model's logits, no loss module), ``"isolate"`` /
``"iso_sq"`` (IsolateLoss / IsolateSquareLoss on the features) or ``"p2sgrad"`` (P2SGradLoss on the features).
"""
import collections
import os

import numpy as np
import torch
import torch.distributed as td

from . import dist as air_dist
from .feature_extraction import LFCC
from .hip_model import HipModel
from .loss import AngularIsoLoss, IsolateLoss, IsolateSquareLoss, P2SGradLoss
from .optim import FusedAdam, FusedSGD
from .ragged import device_lengths


def adjust_learning_rate(lr0, optimizer, epoch_num, lr_decay=0.5, interval=30):
    """main_train.py:144-147."""
    lr = lr0 * (lr_decay ** (epoch_num // interval))
    for group in optimizer.param_groups:
        group["lr"] = lr
    return lr


# what Trainer.evaluate returns: the monitored loss, the EER (min over both polarities), the min t-DCF (None without
# ``tdcf``) and the pass's scores and labels, still on the device
class EvalResult(collections.namedtuple("EvalResult", ("loss", "eer", "min_tdcf", "scores", "labels"))):
    """Five fields, as callers unpack it; ``by_group`` hangs off it as an attribute: None, or with
    ``evaluate(n_groups=...)`` one GroupResult per group (None for a group without bona fide or without spoof trials);
    ``feats`` likewise: None, or with ``evaluate(keep_feats=True)`` the pass's embeddings, fp32 (trials, enc_dim), on
    the device."""
    by_group = None
    feats = None


# one row of the breakdown: the group's name (its index without ``group_names``), the EER of (scores, -scores), and the
# EER and min t-DCF (None without ``tdcf``) in the polarity that wins the POOLED EER - a system has one polarity
GroupResult = collections.namedtuple("GroupResult", ("name", "eers", "eer", "min_tdcf"))

ADD_LOSSES = (None, "isolate", "iso_sq", "ang_iso", "p2sgrad")
# the head a given loss module stands for (any other module: the OC-Softmax head's interface, as before)
_HEAD_OF_MODULE = ((IsolateSquareLoss, "iso_sq"), (IsolateLoss, "isolate"), (P2SGradLoss, "p2sgrad"))


def _make_head(add_loss, enc_dim, r_real, r_fake, alpha):
    """The loss module main_train.py:255-277 builds for ``--add_loss`` (None: none, the CE head has no parameter)."""
    if add_loss == "isolate":
        return IsolateLoss(2, enc_dim, r_real=r_real, r_fake=r_fake)
    if add_loss == "iso_sq":
        return IsolateSquareLoss(2, enc_dim, r_real=r_real, r_fake=r_fake)
    if add_loss == "p2sgrad":
        return P2SGradLoss(in_dim=enc_dim, out_dim=2, smooth=0.0)
    if add_loss == "ang_iso":
        return AngularIsoLoss(enc_dim, r_real=r_real, r_fake=r_fake, alpha=alpha)
    return None


class Trainer:
    add_loss = "ang_iso"  # (class defaults: the head of a Trainer made without __init__)
    ce = None

    def __init__(self, model, enc_dim=256, lr=5e-4, betas=(0.9, 0.999), eps=1e-8, r_real=0.9,
                 r_fake=0.2, alpha=20.0, weight_loss=1.0, feat_len=750, device="cuda", ecapa=False,
                 loss_module=None, augment=None, padding="repeat", add_loss="ang_iso", frontend=None):
        """add_loss: the training head (module docstring).  An explicit ``loss_module`` of one of the head classes
        selects its head; any other module is driven as the OC-Softmax head."""
        if add_loss not in ADD_LOSSES:
            raise ValueError("add_loss must be one of %s, got %r" % (ADD_LOSSES, add_loss))
        if loss_module is not None:
            if add_loss is None:
                raise ValueError("add_loss=None trains cross-entropy on the logits and takes no loss_module")
            add_loss = next((h for cls, h in _HEAD_OF_MODULE if isinstance(loss_module, cls)), add_loss)
        self.add_loss = add_loss
        self.device = torch.device(device)
        self.model = model.to(self.device)
        head = loss_module if loss_module is not None else _make_head(add_loss, enc_dim, r_real, r_fake, alpha)
        self.loss = head.to(self.device) if head is not None else None
        if add_loss is None:
            from .adversarial import CrossEntropyLoss
            self.ce = CrossEntropyLoss()  # main_train.py:251
        # the front-end of features() / score() / the captured step: None = the reference's LFCC (dataset.py:13); a given
        # module (feature_extraction.STFT / Melspec) takes its place - (B, out_dim, feat_len) from forward_padded / _ragged
        # (forward_padded / forward_ragged, the only entry points used here, never mutate the waveforms)
        if frontend is None:
            frontend = LFCC(320, 160, 512, 16000, 20, with_energy=False)
            frontend.mutate_input = False
        self.lfcc = frontend.to(self.device)
        self.lr0 = lr
        self.feat_optimizer = FusedAdam(self.model, lr=lr, betas=betas, eps=eps, weight_decay=0.0005)
        self.loss_optimizer = FusedSGD(self.loss, lr=lr) if self.loss is not None else None
        self.weight_loss = weight_loss
        self.feat_len = feat_len
        self.ecapa = ecapa
        self.world = air_dist.world_size()
        self.padding = padding
        self.out_fold = None
        self.prev_loss = 1e8       # best validation loss so far (main_train.py:280)
        self.early_stop_cnt = 0    # main_train.py:279
        if self.world > 1:
            self.sync_from_rank0()
        # data parallel: start the gradient all-reduce inside backward where the model supports it
        if self.world > 1 and hasattr(self.model, "enable_ddp_overlap") and os.environ.get("AIR_DDP_OVERLAP", "1") == "1":
            self.model.enable_ddp_overlap()
        # optional augment.ChannelAugment: on-the-fly IR convolution of the TRAINING batches ahead
        # of the LFCC kernel (BASELINE configs[4]; replaces channel_simulation/*.py's offline pass)
        self.augment = augment
        # optional hipGraph replay of the fused front-end + forward + loss + backward (enable_graph)
        self._graph = None
        self._graph_warm = 0
        self.use_graph = False
        self._overlap_saved = None
        # world > 1 under hipGraph replay: the step is captured as SEGMENTS cut where backward has finished a bucket of
        # the gradient arena; that bucket's all-reduce is launched between two replays (enable_graph)
        self.graph_segments = False
        self.segment_bytes = int(os.environ.get("AIR_SEGMENT_BYTES", str(air_dist.BUCKET_BYTES)))
        self._seg_bucketer = None

    # ------------------------------------------------------------------ data parallel
    def sync_from_rank0(self):
        """Same replica everywhere: broadcast rank 0's parameter arena, the loss parameters and every module
        buffer (BatchNorm running statistics, num_batches_tracked).  Called at construction when world > 1 -
        ranks that built their model from a different seed or checkpoint would otherwise train diverged
        replicas without any error.  (save_checkpoint runs NO collective: rank 0 saves its own statistics.)"""
        if self.world == 1:
            return
        td.broadcast(self.model.arena().flat, src=0)
        for p in self._loss_params():
            td.broadcast(p.data, src=0)
        self.sync_buffers_from_rank0()

    def sync_buffers_from_rank0(self):
        """Per-rank BatchNorm statistics are the reference's semantics (per-GPU batch == its batch, no SyncBN:
        SURVEY.md 8e); what is SAVED is rank 0's running statistics."""
        if self.world == 1:
            return
        for b in self.model.buffers():
            td.broadcast(b.data, src=0)

    def _loss_params(self):
        return list(self.loss.parameters()) if self.loss is not None else []

    # ------------------------------------------------------------------ logs and checkpoints
    def set_out_fold(self, out_fold, fresh=True):
        """main_train.py:104-121: the output folder with its ``checkpoint`` sub-folder.  ``fresh``: start the
        logs over (the reference deletes and recreates the folder on a new run)."""
        self.out_fold = out_fold
        if air_dist.rank() == 0:
            os.makedirs(os.path.join(out_fold, "checkpoint"), exist_ok=True)
            if fresh:
                for name in ("train_loss.log", "dev_loss.log", "test_loss.log"):
                    path = os.path.join(out_fold, name)
                    if os.path.exists(path):
                        os.remove(path)
        return self

    def log_step(self, epoch_num, i, loss, adv=None):
        """One line of ``train_loss.log`` exactly as main_train.py:479-481 appends it per iteration:
        ``str(epoch) \\t str(i) \\t str(loss) \\n`` with ``loss`` the Python float of ``.item()`` - the head's own
        loss before ``weight_loss`` (trainlossDict[monitor_loss][-1], main_train.py:287-290, :359-415), as step returns it.  ``adv``:
        the (adv_loss, acc_1, acc_2) triple of the ``--ADV_AUG`` variant (main_train.py:470-476)."""
        if self.out_fold is None or air_dist.rank() != 0:
            return
        val = float(loss.item()) if torch.is_tensor(loss) else float(loss)
        with open(os.path.join(self.out_fold, "train_loss.log"), "a") as log:
            if adv is not None and epoch_num > 0:
                log.write(str(epoch_num) + "\t" + str(i) + "\t" + str(float(adv[0])) + "\t" + str(float(adv[1])) +
                          "\t" + str(float(adv[2])) + "\t" + str(val) + "\n")
            else:
                log.write(str(epoch_num) + "\t" + str(i) + "\t" + str(val) + "\n")

    def log_eval(self, epoch_num, losses, eer, name="test_loss.log"):
        """``str(epoch) \\t str(np.nanmean(losses)) \\t str(eer) \\n`` (main_train.py:666-667; the dev log of
        :596-598 has the same layout)."""
        if self.out_fold is None or air_dist.rank() != 0:
            return
        with open(os.path.join(self.out_fold, name), "a") as log:
            log.write(str(epoch_num) + "\t" + str(np.nanmean(losses)) + "\t" + str(eer) + "\n")

    def save_checkpoint(self, epoch_num, val_loss=None):
        """End-of-epoch checkpoints with the reference's file names and whole-module pickles
        (main_train.py:671-709): ``checkpoint/anti-spoofing_feat_model_%d.pt`` and
        ``checkpoint/anti-spoofing_loss_model_%d.pt`` every epoch (numbered epoch_num + 1), and
        ``anti-spoofing_feat_model.pt`` / ``anti-spoofing_loss_model.pt`` whenever the validation loss
        improves.  The CE head (add_loss=None) has no loss module and writes no loss-model file.  generate_score.py:46-48 loads these with torch.load.  Returns True when the best pair
        was written.

        No collective runs in here, so the usual ``if rank == 0: trainer.save_checkpoint(...)`` is safe with
        world > 1 (round 2 broadcast the buffers first and deadlocked under that pattern): rank 0 writes its
        OWN BatchNorm running statistics, which is what SURVEY.md 8e asks for, and the other ranks keep
        theirs.  When every rank calls it, pass the same ``val_loss`` everywhere (``dist.all_mean``) so that
        ``prev_loss`` / ``early_stop_cnt`` stay in step; either way take the early-stop decision through
        ``should_stop()``, which adopts rank 0's counter everywhere."""
        if self.out_fold is None:
            raise RuntimeError("call set_out_fold() first")
        improved = val_loss is not None and val_loss < self.prev_loss
        if air_dist.rank() == 0:
            ck = os.path.join(self.out_fold, "checkpoint")
            torch.save(self.model, os.path.join(ck, "anti-spoofing_feat_model_%d.pt" % (epoch_num + 1)))
            if self.loss is not None:
                torch.save(self.loss, os.path.join(ck, "anti-spoofing_loss_model_%d.pt" % (epoch_num + 1)))
            if improved:
                torch.save(self.model, os.path.join(self.out_fold, "anti-spoofing_feat_model.pt"))
                if self.loss is not None:
                    torch.save(self.loss, os.path.join(self.out_fold, "anti-spoofing_loss_model.pt"))
        if improved:
            self.prev_loss = val_loss
            self.early_stop_cnt = 0
        elif val_loss is not None:
            self.early_stop_cnt += 1
        return improved

    def should_stop(self, patience=500):
        """main_train.py:711-715's early stop (``early_stop_cnt == 500 -> break``) as a decision EVERY rank takes
        alike: under ``if rank == 0: save_checkpoint(...)`` only rank 0's counter advances, and a rank that left
        the loop alone would leave the others blocked in the next all-reduce.  Rank 0 is authoritative: its counter
        is broadcast and adopted everywhere (a MAX over the ranks would hand a stale count back to rank 0 after it
        reset on an improvement - the reference counts CONSECUTIVE epochs without improvement, main_train.py:705-711).
        Collective when world > 1 - call it on every rank, once per epoch."""
        cnt = self.early_stop_cnt
        if self.world > 1:
            dev = self.device if td.get_backend() == "nccl" else "cpu"
            t = torch.tensor([cnt], dtype=torch.int64, device=dev)
            td.broadcast(t, src=0)
            cnt = int(t.item())
            self.early_stop_cnt = cnt
        return cnt >= patience

    def set_epoch(self, epoch_num, lr_decay=0.5, interval=30):
        """main_train.py:287-300.  Quirk kept: the reference never decays the ``iso_sq`` head's SGD learning rate
        (its adjust_learning_rate calls name isolate, ang_iso and p2sgrad only)."""
        adjust_learning_rate(self.lr0, self.feat_optimizer, epoch_num, lr_decay, interval)
        if self.loss_optimizer is not None and self.add_loss != "iso_sq":
            adjust_learning_rate(self.lr0, self.loss_optimizer, epoch_num, lr_decay, interval)

    def features(self, pcm, start=None, lengths=None):
        """(B, L) PCM -> model input, fused on the GPU (dataset.py:66-79 + main_train.py:338,:347).  ``lengths``: int32
        (B,), the batch is ragged - row b of ``pcm`` holds lengths[b] samples (LFCC.forward_ragged).  Never augments (step does)."""
        if lengths is not None:
            self._refuse_ragged_augment(lengths)
            feat = self.lfcc.forward_ragged(pcm, lengths, self.feat_len, start, self.padding)
        else:
            feat = self.lfcc.forward_padded(pcm, self.feat_len, start, self.padding)  # (B, out_dim, feat_len)
        return feat if self.ecapa else feat.unsqueeze(1)

    def _refuse_ragged_augment(self, lengths):
        """A ragged batch needs an augment that is told the rows' lengths (``supports_lengths``: augment.ChannelAugment
        convolves and peak-normalises each row over its own samples).  Any other - a plain callable of one argument -
        would work over the whole row, and scale an utterance by, and convolve it into, its padding."""
        if lengths is not None and self.augment is not None and not getattr(self.augment, "supports_lengths", False):
            raise NotImplementedError("ragged batches (lengths=...) are not supported together with augment")

    def _augment(self, pcm, lengths=None):
        """The augmentation in front of the (captured) step; ragged: fp32 or int16 rows in, fp32 rows with zero tails out."""
        if self.augment is None:
            return pcm
        return self.augment(pcm) if lengths is None else self.augment(pcm, lengths=lengths)

    def _head(self, feats, logits, labels):
        """The head's forward: (loss as logged, the loss backward() starts from, second output).  Second output:
        -scores (ang_iso, p2sgrad), the logits (CE), None (isolate / iso_sq: the reference's head returns a bare loss)."""
        if self.add_loss is None:
            loss = self.ce(logits, labels)
            return loss, loss, logits.detach()  # main_train.py:352-362: no weight_loss
        if self.add_loss in ("isolate", "iso_sq"):
            loss, second = self.loss(feats, labels), None
        else:
            loss, second = self.loss(feats, labels)
        if self.add_loss == "p2sgrad" or self.weight_loss == 1.0:  # main_train.py:411-415: p2sgrad has no weight_loss
            return loss, loss, second
        return loss, loss * self.weight_loss, second  # main_train.py:365-366, :376

    def _zero_grads(self):
        self.feat_optimizer.zero_grad()
        if self.loss_optimizer is not None:
            self.loss_optimizer.zero_grad()

    def _optimise(self, scale):
        self.feat_optimizer.step(grad_scale=scale)
        if self.loss_optimizer is not None:
            self.loss_optimizer.step(grad_scale=scale)

    def step_features(self, feat, labels):
        """One optimisation step on model-layout features.  Returns (loss, second output of the head: -scores for
        ang_iso / p2sgrad, the logits for the CE head, None for isolate / iso_sq)."""
        if not self.model.training:  # (Module.train() walks every submodule: 1 ms of host time per step)
            self.model.train()
        self._zero_grads()
        feats, logits = self.model(feat)
        loss, bwd, second = self._head(feats, logits, labels)
        bwd.backward()  # main_train.py:356-415
        scale = 1.0
        if self.world > 1:
            air_dist.allreduce_grads(self.model, self.loss)
            scale = 1.0 / self.world
        self._optimise(scale)
        return loss.detach(), second

    @torch.no_grad()
    def eval_batch(self, pcm, labels, start=None, lengths=None):
        """The dev pass of main_train.py:526-575 for one batch: (loss, score) with the reference's score of each head -
        softmax(logits)[:, 0] (None), |feats - center| (isolate / iso_sq), the head's second output (ang_iso, p2sgrad).
        Eval-mode model; feeds ``save_checkpoint(val_loss=...)`` for any head."""
        return self._eval_batch(pcm, labels, start, lengths)[:2]

    def _eval_batch(self, pcm, labels, start=None, lengths=None):
        """eval_batch plus the embeddings the model returned: (loss, score, feats)."""
        from . import ops
        self.model.eval()
        feats, logits = self.model(self.features(pcm, start, lengths))
        labels = labels.to(device=feats.device, dtype=torch.int64).contiguous()
        if self.add_loss is None:
            return self.ce(logits, labels), ops.softmax_rows(logits)[:, 0], feats
        if self.add_loss in ("isolate", "iso_sq"):
            lm = self.loss
            return ops.isolate_fwd(feats.float().contiguous(), lm.center.detach().contiguous(), labels, float(lm.r_real),
                                   float(lm.r_fake), self.add_loss == "iso_sq", want_dist=True) + (feats,)
        loss, score = self.loss(feats, labels)
        return loss, score, feats

    @torch.no_grad()
    def evaluate(self, batches, epoch_num=None, log=None, capacity=None, tdcf=None, n_groups=None, group_names=None,
                 keep_feats=False):
        """The dev / eval half of the reference's epoch (main_train.py:484-668) over ``batches``, an iterable of
        ``(pcm, labels[, start[, lengths]])`` as eval_batch takes them, without a host synchronisation inside the
        loop: per batch eval_batch, the loss into a device vector, scores and labels into device buffers
        (preallocated for ``capacity`` trials, or from ``len(batches)`` where it has one; grown by device-side copies
        otherwise).  Behind the loop the EER of both score polarities (main_train.py:662-664) and, with
        ``tdcf=(Pfa_asv, Pmiss_asv, Pmiss_spoof_asv, cost_model)``, the min t-DCF of the polarity with the lower
        EER (evaluate_tDCF_asvspoof19.py:53-67) are found on the device (eval_metrics.DeviceGroupedMinima) and fetched
        with the loss vector in ONE copy; the monitored loss is ``np.nanmean`` of the per-batch losses on the host
        (main_train.py:671 - a device mean would not reproduce numpy's summation order).  ``log``: "dev_loss.log" or
        "test_loss.log" - the line log_eval writes for ``epoch_num``.  Bit-equal to the per-batch loop
        (``eval_batch`` + ``.item()``, ``np.nanmean``, ``eval_metrics.eer_both_polarities``).  Up to 2^20 trials.
        world > 1: every rank evaluates what it is given; no collective runs.  Returns an EvalResult
        (loss, eer, min_tdcf or None, the device score and label tensors).

        ``n_groups=G``: the breakdown by attack or by channel condition.  A batch is then
        ``(pcm, labels, start, lengths, groups)`` (``start`` / ``lengths`` may be None) with one integer group per trial,
        0 .. G - 1 or -1 for "member of every group" (eval_metrics, "breakdown"); the groups go into a third device
        buffer, both polarities are sorted once each for the pooled curve and all groups
        (eval_metrics.DeviceGroupedMinima), and the records still come back with the losses in the one copy.  The
        result's ``by_group`` is a list of GroupResult (``group_names``: G names for them), None where a group lacks a
        class.  ``tdcf`` may carry a fifth element, one (Pfa_asv, Pmiss_asv, Pmiss_spoof_asv) per group; without it
        every group takes the pooled rates.  Without ``n_groups`` the same kernel chain runs on the pooled record alone
        (as many launches as the pass had before the breakdown, and nothing uploaded); ``by_group`` is None.

        ``keep_feats=True``: each batch's embeddings - the fp32 (B, enc_dim) tensor the model hands the head - go into
        a fourth device buffer, preallocated and grown like the others, and come back as the result's ``feats``
        (trials, enc_dim): what visualize.get_features projects, without a second pass or a ``.cpu()`` per batch.  No
        synchronisation is added and every other field is bit-equal to the pass without the keyword, which allocates
        no such buffer and launches what it launched before."""
        from .devbuf import DeviceVector
        from .eval_metrics import DeviceGroupedMinima, _rates_of_group, tdcf_weights
        from .ops import EVAL_MAX_GROUPS, EVAL_RECORD_WORDS
        if log not in (None, "dev_loss.log", "test_loss.log"):
            raise ValueError("log must be None, 'dev_loss.log' or 'test_loss.log', got %r" % (log,))
        weights = tdcf_weights(*tdcf[:4]) if tdcf is not None else None  # (refused before the pass, not after it)
        grouped = n_groups is not None
        if not grouped and (group_names is not None or (tdcf is not None and len(tdcf) > 4)):
            raise ValueError("group_names and per-group t-DCF rates need n_groups")
        if grouped:
            n_groups = int(n_groups)
            if n_groups < 1 or n_groups > EVAL_MAX_GROUPS:
                raise ValueError("n_groups must be 1 .. %d, got %d" % (EVAL_MAX_GROUPS, n_groups))
            if group_names is not None and len(group_names) != n_groups:
                raise ValueError("group_names must name %d groups, got %d" % (n_groups, len(group_names)))
            if weights is not None:  # row 0: the pooled weights; per group its own rates, or the pooled ones
                rates = _rates_of_group(tdcf[4] if len(tdcf) > 4 else tdcf[:3], n_groups)
                weights = [weights] + [tdcf_weights(*r, tdcf[3]) for r in rates]
        n_batches = len(batches) if hasattr(batches, "__len__") else None
        losses = scores = labs = grps = embs = None
        enc_dim = 0
        for batch in batches:
            if grouped and len(batch) != 5:
                raise ValueError("with n_groups a batch is (pcm, labels, start, lengths, groups), got %d items" % len(batch))
            pcm = batch[0]
            labels = batch[1].to(device=self.device, dtype=torch.int64, non_blocking=True).contiguous()
            loss, score, feats = self._eval_batch(pcm, labels, batch[2] if len(batch) > 2 else None,
                                                  batch[3] if len(batch) > 3 else None)
            if losses is None:
                trials = capacity if capacity is not None else (n_batches or 0) * pcm.shape[0]
                losses = DeviceVector(torch.float32, self.device, n_batches or 64)
                scores = DeviceVector(torch.float32, self.device, trials)
                labs = DeviceVector(torch.int64, self.device, trials)
                grps = DeviceVector(torch.int64, self.device, trials) if grouped else None
                if keep_feats:
                    enc_dim = feats.shape[1]
                    embs = DeviceVector(torch.float32, self.device, trials * enc_dim)
            losses.append(loss)
            scores.append(score)
            labs.append(labels)
            if keep_feats:
                embs.append(feats)
            if grouped:
                grps.append(batch[4].to(device=self.device, dtype=torch.int64, non_blocking=True))
        if losses is None:
            raise ValueError("evaluate() needs at least one batch")
        if grouped and grps.n != scores.n:
            raise ValueError("the batches gave %d groups for %d trials" % (grps.n, scores.n))
        words = 2 * ((n_groups or 0) + 1) * EVAL_RECORD_WORDS
        pack = torch.empty(words + losses.n, dtype=torch.int32, device=self.device)  # [records | losses]: one fetch
        minima = DeviceGroupedMinima(scores.view(), labs.view(), grps.view() if grouped else None, n_groups or 0,
                                     (False, True), weights, out=pack[:words])
        pack[words:].view(torch.float32).copy_(losses.view())
        host = pack.cpu().numpy()
        minima.fetch(host[:words])
        batch_losses = host[words:].view(np.float32).astype(np.float64)  # what .item() per batch would have listed
        eers = (minima.eer(0)[0], minima.eer(1)[0])
        eer = min(eers)
        win = 0 if eers[0] < eers[1] else 1
        min_tdcf = minima.min_tdcf(win)[0] if weights is not None else None
        if log is not None:
            self.log_eval(epoch_num, batch_losses, eer, name=log)
        out = EvalResult(float(np.nanmean(batch_losses)), eer, min_tdcf, scores.view(), labs.view())
        if keep_feats:
            out.feats = embs.view().view(-1, enc_dim)
        if grouped:
            out.by_group = []
            for g in range(n_groups):
                pair = (minima.eer(0, g), minima.eer(1, g))  # (a group lacks a class in both polarities or in neither)
                out.by_group.append(None if pair[0] is None else GroupResult(
                    g if group_names is None else group_names[g], (pair[0][0], pair[1][0]), pair[win][0],
                    minima.min_tdcf(win, g)[0] if weights is not None else None))
        return out

    def step(self, pcm, labels, start=None, lengths=None):
        """``lengths`` None: a batch of one length; a ``start`` forces the eager step.  ``lengths`` int32 (B,): a ragged
        batch - the crop offsets and the lengths are device data of the captured step, so it stays on hipGraph replay
        with or without ``start``, and every batch of one (B, Lcap) shape replays the same capture.  With an ``augment``
        that takes lengths (ChannelAugment) the rows are augmented over their own samples in front of the captured region,
        which then sees fp32 (B, Lcap) whatever the batch's dtype was."""
        self._refuse_ragged_augment(lengths)
        if lengths is not None and self.augment is not None:
            lengths = self._ragged_lengths(lengths, pcm)  # checked and uploaded once, for the augment and the front-end
        pcm = self._augment(pcm, lengths)
        if self.use_graph and (start is None or lengths is not None):
            out = self._graphed_step(pcm, labels, lengths, start)
            if out is not None:
                return out
        return self.step_features(self.features(pcm, start, lengths), labels)

    def train_epoch(self, batches, epoch_num):
        """The training half of the reference's epoch (main_train.py:287-481) over ``batches`` - an iterable of
        ``(pcm, labels[, start[, lengths]])``, e.g. ``corpus.CorpusSampler.epoch()`` - without a host synchronisation
        inside the loop: ``set_epoch``, then per batch ``step`` with the returned loss kept in a device vector.  Behind
        the loop the losses are fetched in ONE copy and ``train_loss.log`` gets the lines one ``log_step`` per batch
        would have written, byte for byte.  Returns the per-batch losses as a float32 host array.  The plain trainer
        only: the ``--ADV_AUG`` columns are log_step's."""
        from .devbuf import DeviceVector
        self.set_epoch(epoch_num)
        losses = DeviceVector(torch.float32, self.device, len(batches) if hasattr(batches, "__len__") else 64)
        for batch in batches:
            loss, _ = self.step(batch[0], batch[1], start=batch[2] if len(batch) > 2 else None,
                                lengths=batch[3] if len(batch) > 3 else None)
            losses.append(loss)
        host = losses.view().cpu().numpy()
        if self.out_fold is not None and air_dist.rank() == 0 and host.size:
            with open(os.path.join(self.out_fold, "train_loss.log"), "a") as log:
                # str(float(x)) of the float32 loss: what log_step makes of ``loss.item()``
                log.write("".join(str(epoch_num) + "\t" + str(i) + "\t" + str(float(v)) + "\n" for i, v in enumerate(host)))
        return host

    # ------------------------------------------------------------------ hipGraph replay
    def enable_graph(self, on=True, segments=None):
        """Capture front-end + forward + loss + backward of one fixed-shape batch in a hipGraph and replay it per
        step (the optimiser launches stay outside: Adam's step count is a kernel argument).  ECAPA's step is
        ~450 launches of 5 - 150 us each and the host cannot keep the queue full once the activations are bf16
        (13 % GPU idle, tools/gpu_idle.py); the ResNet step is ~330 launches behind 4 - 7 ms of host work, which a
        cold box (Python not yet warm, clocks not yet up) does not hide.  Replaying one graph removes the host from
        the step.  The ResNet's attention noise (resnet.py:38) is drawn from a device-side Philox offset that the
        draw itself advances (ops.randn_ctr), so every replay draws fresh noise and eager launches and replays walk
        the same sequence.

        world > 1: a captured chain holds no collective.  ``segments`` False: one graph, the gradient arena and the loss
        centre are all-reduced behind the replay (dist.allreduce_grads) - the whole exchange is exposed.  ``segments``
        True (round 6; default with world > 1, AIR_GRAPH_SEGMENTS=0 / 1 forces): the step is captured as SEVERAL graphs
        cut inside backward where a bucket (>= segment_bytes) of the gradient arena is final - ResNet-18: behind
        layer4.1 (24 MB), behind layer3.1 (19 MB), the rest - and each bucket's all-reduce is launched on the
        communication stream between two replays, underneath the next segment: replay's 0.2 - 0.4 ms of host time per
        step AND BASELINE configs[3]'s "all-reduce overlapped with backward".  Same kernels in the same order as the
        one-chain capture and as the eager step: bit-identical (tests/test_dist_gpu.py)."""
        self.use_graph = bool(on) and isinstance(self.model, HipModel)
        if segments is None:
            env = os.environ.get("AIR_GRAPH_SEGMENTS", "")
            segments = (env == "1") if env in ("0", "1") else self.world > 1
        self.graph_segments = bool(segments) and self.use_graph
        self._drop_graph()
        if self.use_graph:
            # captured as ONE chain: a graph with the side stream's fork / join pairs replays slower (profiles/r06_launch_modes.md)
            if self._overlap_saved is None:  # (a second enable_graph() must not save the already-forced False)
                self._overlap_saved = (self.model.overlap_wgrad, self.model._bucketer)
            self.model.overlap_wgrad, self.model._bucketer = False, None
        elif self._overlap_saved is not None:
            self.model.overlap_wgrad, self.model._bucketer = self._overlap_saved
            self._overlap_saved = None
        return self

    def _drop_graph(self):
        """Forget the capture and release the scratch buffers that were only kept alive for its replays."""
        from . import ops
        had = self._graph is not None
        self._graph = None
        self._graph_warm = 0
        if had:
            ops.unpin_workspaces(id(self))

    def _head_scalars(self):
        """The head's scalars that travel as kernel arguments (ang_iso: the tuple the key always held)."""
        if self.add_loss == "ang_iso":
            return (float(self.loss.r_real), float(self.loss.r_fake), float(self.loss.alpha))
        if self.add_loss in ("isolate", "iso_sq"):
            return (self.add_loss, float(self.loss.r_real), float(self.loss.r_fake))
        if self.add_loss == "p2sgrad":
            return ("p2sgrad", float(self.loss.smooth))
        return ("ce",)

    def _graph_key(self, pcm, labels, ragged=False):
        """Everything a capture freezes: shapes, the arithmetic mode and the scalars that travel as kernel
        arguments (loss weight and the head's own: OC-Softmax margins / scale, Isolate radii, P2SGrad smoothing).
        ``ragged``: the capture holds the ragged front-end (lengths and crop offsets are its device inputs, not its key)."""
        return (tuple(pcm.shape), pcm.dtype, tuple(labels.shape), getattr(self.model, "compute_dtype", "fp32"),
                self.feat_len, float(self.weight_loss)) + self._head_scalars() + (
                self.padding, getattr(self.model, "noise_mode", None), getattr(self.model, "noise_scale", None)) + (
                ("ragged",) if ragged else ()) + (
                () if type(self.lfcc) is LFCC else (type(self.lfcc).__name__, self.lfcc.out_dim, self.lfcc._flags()))

    def _graphed_step(self, pcm, labels, lengths=None, start=None):
        from . import ops
        if getattr(self.model, "noise_mode", None) == "tensor":
            return None  # an installed noise tensor (parity tests) is host state: eager
        ragged = lengths is not None
        if ragged:
            lengths = self._ragged_lengths(lengths, pcm)
        key = self._graph_key(pcm, labels, ragged)
        g = self._graph
        if g is not None and (g["key"] != key or g["ws_gen"] != ops.workspace_generation()):
            # another shape / hyper-parameter, or an eager step in between outgrew a scratch buffer the graph
            # points into (the old buffers are pinned until here, so nothing dangled; the capture is simply redone)
            self._drop_graph()
            g = None
        if g is None:
            # two eager steps first: arenas, workspaces, lazy kernel attributes, optimiser state, the side stream
            if self._graph_warm < 2:
                self._graph_warm += 1
                return None
            g = self._capture_or_fall_back(key, pcm, labels, lengths, start)
            if g is None:
                return None  # (every rank alike: the eager step takes over)
        if not self.model.training:  # an interleaved score() left eval mode behind
            self.model.train()
        # The captured kernels write the gradients into the tensors that were p.grad AT CAPTURE (arena views for the
        # model, a tensor of the graph's private pool for the loss head's parameter).  Any eager step or zero_grad() since then
        # replaced or dropped them: re-point every p.grad, or the optimisers would apply stale / no gradients.
        for p, gr in g["grads"]:
            if p.grad is not gr:
                p.grad = gr
        g["pcm"].copy_(pcm, non_blocking=True)
        g["labels"].copy_(labels, non_blocking=True)
        if ragged:
            g["lengths"].copy_(lengths, non_blocking=True)
            if start is None:
                g["start"].zero_()
            else:
                g["start"].copy_(torch.as_tensor(start), non_blocking=True)
        self._refresh_tail(g)
        # graph k's replay, then (world > 1, segments) the all-reduce of the arena slice it completed - launched on the
        # communication stream behind an event, so that the next replay is enqueued right away
        bucketer = None
        if self.world > 1 and g["segments"]:
            if self._seg_bucketer is None:
                self._seg_bucketer = air_dist.GradBucketer(self.segment_bytes)
            bucketer = self._seg_bucketer
            arena = self.model.arena()
            bucketer.reset(arena.grad, arena.head_total)
        main = torch.cuda.current_stream()
        for graph, lo in g["graphs"]:
            graph.replay()
            if bucketer is not None and lo is not None:
                ev = torch.cuda.Event()
                ev.record(main)
                bucketer.lo, bucketer.events = lo, [ev]
                bucketer.flush()
        scale = 1.0
        if self.world > 1:  # the remaining exchange of the step, behind the replay (no in-backward bucketer while the graph is on)
            self.model._bucketer = bucketer  # (allreduce_grads waits for what was sent and reduces the remaining head)
            try:
                air_dist.allreduce_grads(self.model, self.loss)
            finally:
                self.model._bucketer = None
            scale = 1.0 / self.world
        self._optimise(scale)
        self._replay_tail(g, scale)
        return g["loss"].detach().clone(), (g["neg"].clone() if g["neg"] is not None else None)

    # A subclass whose step goes on behind the optimisers (adversarial.AdversarialTrainer: the classifiers' phase)
    # captures that part as a graph of the same pool (``captured(fn) -> (graph, fn())``), refreshes its static inputs
    # before the replays and replays it behind ``_optimise``.
    def _capture_tail(self, captured):
        return None

    def _refresh_tail(self, g):
        pass

    def _replay_tail(self, g, scale):
        pass

    def _ragged_lengths(self, lengths, pcm):
        """``lengths`` as the int32 (B,) device tensor a replay copies into the capture's buffer; host values are checked
        (``ragged.device_lengths``)."""
        return device_lengths(lengths, pcm.shape[0], pcm.shape[1], pcm.device, non_blocking=True)

    def _capture_or_fall_back(self, key, pcm, labels, lengths=None, start=None):
        """The capture, guarded for world > 1: were it to fail on ANY rank (a runtime that refuses a call inside a
        capture, memory), EVERY rank drops the graph and goes on with the eager bucketed step - one rank replaying
        while another launches its all-reduces from inside backward would pair the wrong collectives.  The agreement
        costs one 4-byte all-reduce at capture time.  world 1: errors propagate as before."""
        if self.world == 1:
            return self._capture(key, pcm, labels, lengths, start)
        err = None
        try:
            g = self._capture(key, pcm, labels, lengths, start)
        except Exception as exc:  # noqa: BLE001
            g, err = None, exc
        dev = self.device if td.get_backend() == "nccl" else "cpu"
        ok = torch.tensor([0 if g is None else 1], dtype=torch.int32, device=dev)
        td.all_reduce(ok, op=td.ReduceOp.MIN)
        if int(ok.item()) == 1:
            return g
        import warnings
        warnings.warn("hipGraph capture of the train step failed on %s (%s): every rank continues with the eager step" % (
            "this rank" if err is not None else "another rank", repr(err)[:200] if err is not None else "-"))
        self._drop_graph()
        self.enable_graph(False)  # restores the side stream and the in-backward bucketer
        return None

    def _fwd_bwd_direct(self, pcm, labels, lengths=None, start=None):
        """front-end + forward + loss + backward as plain calls in THIS thread (what model(x) -> loss.backward() does
        through autograd, whose backward runs on a worker thread): (loss, second output, [(param, grad)])."""
        model = self.model
        feats, saved = model.forward_saved(self.features(pcm, start, lengths))
        if self.add_loss is None:  # the CE head: the gradient enters through the logits (fc_mu / fc7, bn7)
            leaf = saved["logits"].detach().requires_grad_(True)
            loss, bwd, second = self._head(None, leaf, labels)
            bwd.backward()
            grads = model.backward_saved(saved, None, dout=leaf.grad)
        else:
            leaf = feats.detach().requires_grad_(True)
            loss, bwd, second = self._head(leaf, None, labels)
            bwd.backward()  # the head only: d(loss) / d(feats) and its parameter's gradient
            grads = model.backward_saved(saved, leaf.grad)
        pairs = []
        for (n, p, _, _), gr in zip(model.arena().entries, grads):
            if gr is not None:
                p.grad = gr
                pairs.append((p, gr))
        pairs += [(p, p.grad) for p in self._loss_params() if p.grad is not None]
        return loss, second, pairs

    def _capture(self, key, pcm, labels, lengths=None, start=None):
        """The step recorded through _fwd_bwd_direct on a capture stream: one hipGraph, or (graph_segments) several sharing
        one memory pool, cut at backward's bucket boundaries (enable_graph).  A ragged capture (``lengths``) owns static
        int32 ``lengths`` and ``start`` buffers beside ``pcm`` and ``labels``; every replay refreshes them."""
        from . import ops
        self.model.train()
        s_pcm, s_labels = pcm.detach().clone(), labels.detach().clone()
        s_len = s_start = None
        if lengths is not None:
            s_len = lengths.detach().to(torch.int32).clone()
            s_start = torch.zeros(pcm.shape[0], dtype=torch.int32, device=pcm.device)
            if start is not None:
                s_start.copy_(torch.as_tensor(start))
        self._zero_grads()
        arena = self.model.arena()
        pool = torch.cuda.graph_pool_handle()
        state = {"g": None, "hi": arena.head_total}
        graphs = []  # (graph, lo): replaying it completes arena.grad[lo:hi]; lo None for the last one

        # world > 1: other threads of the process (the process group's watchdog polling its events) make runtime calls
        # while this thread captures; "thread_local" checks only the capturing thread's calls (the default, "global",
        # turns any other thread's event query into a capture error)
        mode = "thread_local" if self.world > 1 else "global"

        def begin():
            state["g"] = torch.cuda.CUDAGraph()
            state["g"].capture_begin(pool=pool, capture_error_mode=mode)

        def cut(lo):
            """backward reports: everything that writes arena.grad[lo:] has been enqueued"""
            if lo >= state["hi"] or (state["hi"] - lo) * 4 < self.segment_bytes:
                return
            state["g"].capture_end()
            graphs.append((state["g"], lo))
            state["hi"] = lo
            begin()

        import gc
        torch.cuda.synchronize()
        gc.collect()
        torch.cuda.empty_cache()
        cap = torch.cuda.Stream(device=self.device)
        cap.wait_stream(torch.cuda.current_stream())
        self.model._segment_cut = cut if self.graph_segments else None  # (no cut: one graph)
        try:
            with torch.cuda.stream(cap):
                begin()
                try:
                    loss, neg, grads = self._fwd_bwd_direct(s_pcm, s_labels, s_len, s_start)
                except BaseException:
                    try:  # leave the stream out of capture mode: the caller may go on eagerly (_capture_or_fall_back)
                        state["g"].capture_end()
                    except Exception:  # noqa: BLE001
                        pass
                    raise
                state["g"].capture_end()
                graphs.append((state["g"], None))  # the rest of the arena goes with the final all-reduce
                self.model._segment_cut = None

                def captured(fn):
                    graph = torch.cuda.CUDAGraph()
                    graph.capture_begin(pool=pool, capture_error_mode=mode)
                    try:
                        out = fn()
                    except BaseException:
                        try:
                            graph.capture_end()
                        except Exception:  # noqa: BLE001
                            pass
                        raise
                    graph.capture_end()
                    return graph, out
                tail = self._capture_tail(captured)
        finally:
            self.model._segment_cut = None
        torch.cuda.current_stream().wait_stream(cap)
        ops.pin_workspaces(id(self))
        if not getattr(self, "_pin_finalizer", None):
            import weakref
            self._pin_finalizer = weakref.finalize(self, ops.unpin_workspaces, id(self))
        # p.grad now ARE the tensors the captured kernels write (no zero_grad between replays - every gradient is
        # overwritten, none accumulated); kept in "grads" so _graphed_step can restore them after eager interludes
        self._graph = dict(key=key, graphs=graphs, segments=graphs if self.graph_segments else None, pool=pool, pcm=s_pcm,
                           labels=s_labels, lengths=s_len, start=s_start, loss=loss, neg=neg, grads=grads, tail=tail,
                           ws_gen=ops.workspace_generation())
        return self._graph

    @torch.no_grad()
    def score(self, pcm, start=None, lengths=None):
        """generate_score.py:91-110: the value written to the score file (+cos similarity for ang_iso and p2sgrad,
        softmax(logits)[:, 0] for the CE head - and for isolate / iso_sq, which generate_score.py has no branch for)."""
        from .generate_score import batch_scores
        self.model.eval()
        add = {"ang_iso": "ocsoftmax", "p2sgrad": "p2sgrad"}.get(self.add_loss)
        return -batch_scores(self.model, self.features(pcm, start, lengths), self.loss, add)
