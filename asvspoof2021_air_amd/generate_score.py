"""Scoring path of the reference (generate_score.py:37-119) on the HIP modules.

``test_on_dataset`` keeps the reference's loop - eval-mode model, per-item ``lfcc.transpose(2, 3)``
(``.squeeze(1)`` for ECAPA, :91-94), ``feats, outputs = model(lfcc)``, default score
``-softmax(outputs)[:, 0]`` (:102), ``--loss ocsoftmax`` / ``p2sgrad`` score = the loss module's second output
(:104-105, :109-110), ``--loss amsoftmax`` score = ``softmax(logits)[:, 0]`` of the module's cosines (:106-108) -
and the exact score-file text (:113-119): ``'%s %s %s\\n' % (name, -score, key)`` for the
ASVspoof2019 tasks, ``'%s %s\\n'`` for the 2021 evaluation sets.  Differences, both
arithmetic-neutral: any batch size (the reference uses 1; eval-mode BatchNorm makes utterances
independent, so one launch scores a whole batch) and one device->host copy per batch instead of
one ``.item()`` per utterance.

Quirk kept from the reference (:96): the dataset's labels are overwritten by zeros before the
key is written, so every 2019-task line ends in ``bonafide``; ``keep_dataset_labels=True`` writes
the true key instead.

``score_pcm`` is the on-the-fly variant: raw PCM -> fused HIP LFCC (+pad/chop, transposed) ->
model -> score, for corpora that were not pre-extracted by preprocess.py.

``test_on_dataset_ensemble`` / ``score_pcm_ensemble`` score K models in one pass - the batch is copied and transposed
(or its features computed) once for all of them - and fuse the K score vectors on the device as the reference's
score_fusion.py does on files (score_fusion.py here; ops.score_fuse).
"""
import os

import torch

from . import ops
from .devbuf import DeviceVector
from .feature_extraction import LFCC


def format_score_line(name, score, key=None):
    """One line of the score file (generate_score.py:113-119); ``score`` is the NEGATED loss
    score, i.e. the value the reference writes as ``-score[j].item()``."""
    if key is None:
        return "%s %s\n" % (name, score)
    return "%s %s %s\n" % (name, score, key)


@torch.no_grad()
def batch_scores(model, lfcc, loss_model=None, add_loss=None):
    """Scores of one batch of model-layout features, as a (B,) GPU tensor holding what the
    reference calls ``score`` (the file gets ``-score``)."""
    feats, outputs = model(lfcc)
    if add_loss is None:
        return -ops.softmax_rows(outputs)[:, 0]  # :102
    labels = torch.zeros(lfcc.shape[0], dtype=torch.int64, device=lfcc.device)  # :96
    if add_loss in ("ocsoftmax", "p2sgrad"):
        _, score = loss_model(feats, labels)  # :104-105, :109-110
        return score
    if add_loss == "amsoftmax":
        logits, _ = loss_model(feats, labels)  # :106-108
        return ops.softmax_rows(logits)[:, 0]
    raise NotImplementedError("scoring with add_loss=%r: generate_score.py knows ocsoftmax, amsoftmax and p2sgrad" % (
        add_loss,))


class GraphedScorer:
    """The eval-mode score of ONE fixed-shape batch captured in a hipGraph and replayed.

    generate_score.py scores with ``DataLoader(batch_size=1)`` (:73): ~150 kernel launches of a few
    microseconds each per utterance, i.e. launch-bound.  When the caller keeps that batch size, capture the
    whole forward (model + loss score) once for the feature shape and replay it per utterance: one graph
    launch instead of ~150 kernel launches.  The attention noise of resnet.py:38 comes from a device-side Philox offset
    that the captured draw advances (ops.randn_ctr): every replay draws fresh noise, like the reference's per-call
    ``torch.randn``; ``model.set_attention_noise(None)`` for none."""

    def __init__(self, model, example, loss_model=None, add_loss=None):
        if not example.is_cuda:
            raise ValueError("GraphedScorer needs a GPU example batch")
        self.model, self.loss_model, self.add_loss = model.eval(), loss_model, add_loss
        self.static_in = example.detach().clone().contiguous()
        with torch.no_grad():
            side = torch.cuda.Stream()
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):  # warm-up off the capture: arenas, workspaces, lazy module loads
                for _ in range(2):
                    batch_scores(self.model, self.static_in, loss_model, add_loss)
            torch.cuda.current_stream().wait_stream(side)
            self.graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(self.graph):
                self.static_out = batch_scores(self.model, self.static_in, loss_model, add_loss)

    @torch.no_grad()
    def __call__(self, lfcc):
        """lfcc: model-layout features of the captured shape.  Returns the (B,) ``score`` tensor (a static
        buffer: consume or clone it before the next call)."""
        if tuple(lfcc.shape) != tuple(self.static_in.shape):
            raise ValueError("GraphedScorer was captured for %s, got %s" % (tuple(self.static_in.shape), tuple(lfcc.shape)))
        self.static_in.copy_(lfcc, non_blocking=True)
        self.graph.replay()
        return self.static_out


@torch.no_grad()
def test_on_dataset(model, loader, score_file, loss_model=None, add_loss=None, task="19eval", ecapa=False,
                    device="cuda", keep_dataset_labels=False, use_graph=False, sync="batch"):
    """generate_score.py:75-119 over any iterable of dataset batches
    ``(lfcc:(B,1,feat_len,60), audio_fn, tag, labels[, channel])`` ('19' tasks) or
    ``(lfcc, audio_fn)`` (2021 LA/DF eval).  Returns the number of lines written.
    use_graph: replay a captured hipGraph per batch shape (GraphedScorer) - for the reference's batch size 1.
    sync: "batch" copies each batch's scores to the host before the next is launched (one device synchronisation per
    utterance at the reference's batch size 1); "end" keeps them in a device buffer and writes the file after ONE
    copy - the same text, byte for byte."""
    if sync not in ("batch", "end"):
        raise ValueError("sync must be 'batch' or 'end', got %r" % (sync,))
    model.eval()
    os.makedirs(os.path.dirname(os.path.abspath(score_file)), exist_ok=True)
    is19 = "19" in task
    n = 0
    graphs = {}
    held, rows = None, []  # sync="end": the scores on the device, (name, label) per line on the host
    with open(score_file, "w") as fh:
        for data in loader:
            if is19:
                lfcc, audio_fn, labels = data[0], data[1], data[3]
            else:
                lfcc, audio_fn = data[0], data[1]
                labels = None
            lfcc = lfcc.to(device).transpose(2, 3)
            if ecapa:
                lfcc = lfcc.squeeze(1)
            lfcc = lfcc.contiguous()
            if use_graph:
                key = tuple(lfcc.shape)
                if key not in graphs:
                    graphs[key] = GraphedScorer(model, lfcc, loss_model, add_loss)
                score = graphs[key](lfcc)
            else:
                score = batch_scores(model, lfcc, loss_model, add_loss)
            if sync == "end":
                if held is None:
                    held = DeviceVector(torch.float32, lfcc.device, (len(loader) if hasattr(loader, "__len__") else 64) * lfcc.shape[0])
                held.append((-score).float())  # (a copy: a GraphedScorer's output is overwritten by the next replay)
                rows.extend((audio_fn[j], (int(labels[j]) if keep_dataset_labels else 0) if is19 else None)
                            for j in range(lfcc.shape[0]))
                continue
            vals = (-score).float().cpu().tolist()
            for j, v in enumerate(vals):
                if is19:
                    lab = int(labels[j]) if keep_dataset_labels else 0
                    fh.write(format_score_line(audio_fn[j], v, "spoof" if lab else "bonafide"))
                else:
                    fh.write(format_score_line(audio_fn[j], v))
                n += 1
        if held is not None:
            for (name, lab), v in zip(rows, held.view().cpu().tolist()):
                fh.write(format_score_line(name, v, None if lab is None else ("spoof" if lab else "bonafide")))
                n += 1
    return n


@torch.no_grad()
def score_pcm(model, loss_model, pcm, feat_len=750, ecapa=False, add_loss="ocsoftmax", lfcc=None, lengths=None, start=None):
    """(B, L) raw PCM on the GPU -> (B,) scores as written to the file (``-score``).  ``lengths``: int32 (B,), a ragged
    batch - row b holds lengths[b] samples (LFCC.forward_ragged); ``start``: optional int32 (B,) crop offsets."""
    if lfcc is None:
        lfcc = LFCC(320, 160, 512, 16000, 20, with_energy=False).to(pcm.device)
        lfcc.mutate_input = False
    if lengths is not None:
        feat = lfcc.forward_ragged(pcm, lengths, feat_len, start)
    else:
        feat = lfcc.forward_padded(pcm, feat_len, start)
    model.eval()
    return -batch_scores(model, feat if ecapa else feat.unsqueeze(1), loss_model, add_loss)


# ------------------------------------------------------------------ K systems in one pass (score_fusion.py)
def _per_model(value, K, what):
    """One entry per model from a single value or a list of K."""
    if isinstance(value, (list, tuple)):
        if len(value) != K:
            raise ValueError("%s: %d entries for %d models" % (what, len(value), K))
        return list(value)
    return [value] * K


@torch.no_grad()
def score_pcm_ensemble(models, loss_models, pcm, feat_len=750, ecapa=False, add_loss="ocsoftmax", lfcc=None, lengths=None,
                       start=None):
    """score_pcm for K models on ONE front-end launch: (B, L) raw PCM -> (K, B) scores as written to the files, row k
    bit-equal to ``score_pcm(models[k], loss_models[k], pcm, ...)``.  ``loss_models`` / ``ecapa`` / ``add_loss``: one
    value for all models or a list of K; the feature tensor is computed once, a 2-d model gets ``unsqueeze(1)`` of it
    (a view)."""
    K = len(models)
    if K < 1:
        raise ValueError("score_pcm_ensemble needs at least one model")
    loss_models, ecapa, add_loss = (_per_model(v, K, n) for v, n in ((loss_models, "loss_models"), (ecapa, "ecapa"),
                                                                     (add_loss, "add_loss")))
    if lfcc is None:
        lfcc = LFCC(320, 160, 512, 16000, 20, with_energy=False).to(pcm.device)
        lfcc.mutate_input = False
    if lengths is not None:
        feat = lfcc.forward_ragged(pcm, lengths, feat_len, start)
    else:
        feat = lfcc.forward_padded(pcm, feat_len, start)
    feat4 = feat.unsqueeze(1)
    out = torch.empty((K, feat.shape[0]), dtype=torch.float32, device=feat.device)
    for k, model in enumerate(models):
        model.eval()
        out[k].copy_(-batch_scores(model, feat if ecapa[k] else feat4, loss_models[k], add_loss[k]))
    return out


@torch.no_grad()
def test_on_dataset_ensemble(models, loader, score_files, fused_file=None, method="avg", eers=None, loss_models=None,
                             add_loss=None, task="19eval", ecapa=False, device="cuda", keep_dataset_labels=False):
    """``test_on_dataset(..., sync="end")`` for K models in ONE pass over ``loader``, and their fusion.

    Per batch: one host-to-device copy and one transpose of the features, shared by the K models (an ECAPA model takes
    the ``squeeze(1)`` view of the same tensor), then K ``batch_scores`` calls whose results are copied device-side into
    a (K, capacity) buffer (capacity from ``len(loader)``, doubled by a device-side copy when outgrown).  Nothing inside
    the loop waits for the device.  Behind the loop ops.score_fuse fuses the K rows where they lie (aligned path:
    ``method`` "avg" = the sum, "wght" = the weighted mean with ``score_fusion.cal_weight(eers)``), and ONE
    device-to-host copy brings back the K vectors and the fused one.

    Written: ``score_files[k]`` with exactly the text ``test_on_dataset(models[k], ..., sync="end")`` writes;
    ``fused_file`` (optional, '19' tasks: the 2021 files carry no key to join on) with the text
    ``score_fusion.write_fused`` produces from ``avg_fuse`` / ``weighted_fuse`` over those K files - rows
    ``fname - key score`` sorted by name.  A name that the loader yields twice with one key is refused (ValueError): the
    file-based fusion would add the two.  ``loss_models`` / ``add_loss`` / ``ecapa``: one value for all models or a
    list of K.  Every model is put in eval mode.

    Returns (lines per file, FusionResult or None).  The FusionResult (score_fusion.fuse_device: the systems' EERs, the
    fused EER) is computed for '19' tasks with ``keep_dataset_labels``, where the keys are the true ones; it costs
    fuse_device's own copy of the records (two for "wght" without ``eers``, whose weights then come from the systems'
    own EERs).  Without it "wght" needs ``eers``.

    ``use_graph`` (GraphedScorer) is out of scope here: K captured graphs per batch shape would share one static input
    but not one replay."""
    from . import score_fusion as sf
    K = len(models)
    if K < 1 or len(score_files) != K:
        raise ValueError("%d score files for %d models" % (len(score_files), K))
    if method not in ("avg", "wght"):
        raise ValueError("method must be 'avg' or 'wght', got %r" % (method,))
    loss_models, ecapa, add_loss = (_per_model(v, K, n) for v, n in ((loss_models, "loss_models"), (ecapa, "ecapa"),
                                                                     (add_loss, "add_loss")))
    is19 = "19" in task
    evaluate = is19 and keep_dataset_labels
    if fused_file is not None and not is19:
        raise ValueError("a fused file needs the keys of a '19' task")
    if method == "wght" and eers is None and not evaluate:
        raise ValueError("method 'wght' needs eers (or a '19' task with keep_dataset_labels, whose EERs it then takes)")
    if eers is not None and (method != "wght" or len(eers) != K):
        raise ValueError("eers: %d EERs for method 'wght', one per model" % K)
    for m in models:
        m.eval()
    held, n, rows = None, 0, []
    for data in loader:
        lfcc4 = data[0].to(device).transpose(2, 3).contiguous()
        lfcc3 = lfcc4.squeeze(1)
        B = lfcc4.shape[0]
        if held is None:
            held = torch.empty((K, max(1, (len(loader) if hasattr(loader, "__len__") else 64) * B)), dtype=torch.float32,
                               device=lfcc4.device)
        if n + B > held.shape[1]:
            grown = torch.empty((K, max(n + B, 2 * held.shape[1])), dtype=torch.float32, device=held.device)
            grown[:, :n].copy_(held[:, :n])
            held = grown
        for k, model in enumerate(models):
            score = batch_scores(model, lfcc3 if ecapa[k] else lfcc4, loss_models[k], add_loss[k])
            held[k, n:n + B].copy_((-score).float())
        labels = data[3] if is19 else None
        rows.extend((data[1][j], (int(labels[j]) if keep_dataset_labels else 0) if is19 else None) for j in range(B))
        n += B
    if held is None:
        raise ValueError("test_on_dataset_ensemble needs at least one batch")
    per_system = held[:, :n]
    result = None
    if evaluate:
        labs = torch.tensor([lab for _, lab in rows], dtype=torch.int64).to(held.device)
        result = sf.fuse_device(per_system, labs, method, eers)
        fused = result.scores
    else:
        weights = None
        if method == "wght":
            weights = torch.tensor(sf.cal_weight(eers), dtype=torch.float64).to(torch.float32).to(held.device)
        fused = ops.score_fuse(per_system, None, weights, "mean" if method == "wght" else "sum")
    host = torch.cat((per_system.reshape(-1), fused)).cpu()  # [K vectors | fused]: the one copy
    keys = [None if lab is None else ("spoof" if lab else "bonafide") for _, lab in rows]
    for k, path in enumerate(score_files):
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        with open(path, "w") as fh:
            for (name, _), key, v in zip(rows, keys, host[k * n:(k + 1) * n].tolist()):
                fh.write(format_score_line(name, v, key))
    if fused_file is not None:
        joined = [(name, "-", key) for (name, _), key in zip(rows, keys)]
        order = sorted(range(n), key=joined.__getitem__)
        for a, b in zip(order, order[1:]):
            if joined[a] == joined[b]:
                raise ValueError("the loader yields %r twice: score_fusion would add the two scores" % (joined[a],))
        os.makedirs(os.path.dirname(os.path.abspath(fused_file)), exist_ok=True)
        sf.write_fused(fused_file, [joined[i] for i in order], host[K * n:].numpy()[order])
    return n, result


@torch.no_grad()
def test_on_dataset_gmm(backend, loader, score_file, task="19eval", device="cuda", keep_dataset_labels=False, sync="end"):
    """The score file of ``test_on_dataset`` for a ``gmm.GMMBackend``: the same loop over the same batches
    (``(lfcc:(B,1,feat_len,60), audio_fn, tag, labels[, channel])`` for the '19' tasks, ``(lfcc, audio_fn)`` for the 2021
    evaluation sets), the same ``format_score_line`` and the same label quirk; the value written is the back-end's
    log-likelihood ratio (higher = bona fide).  The first item may also be (B, Lcap) PCM, optionally followed by a sixth
    / third item with the int32 lengths: it then goes through the back-end's own front-end.  Pre-extracted features
    count every frame of the row - padding frames included, as the networks see them.  ``sync`` as there; returns the
    number of lines written."""
    if sync not in ("batch", "end"):
        raise ValueError("sync must be 'batch' or 'end', got %r" % (sync,))
    os.makedirs(os.path.dirname(os.path.abspath(score_file)), exist_ok=True)
    is19 = "19" in task
    held, rows, n = None, [], 0
    with open(score_file, "w") as fh:
        for data in loader:
            x, audio_fn = data[0].to(device), data[1]
            labels = data[3] if is19 else None
            if x.dim() == 2:
                extra = 5 if is19 else 2
                score = backend.score(x, data[extra] if len(data) > extra else None)
            else:
                feats = x.reshape(x.shape[0], x.shape[-2], x.shape[-1]).float()  # (B, feat_len, D): frame-major
                score = backend.score_frames(feats, None, "btd")
            keys = [(("spoof" if (int(labels[j]) if keep_dataset_labels else 0) else "bonafide") if is19 else None)
                    for j in range(x.shape[0])]
            if sync == "end":
                if held is None:
                    held = DeviceVector(torch.float32, score.device, (len(loader) if hasattr(loader, "__len__") else 64) * x.shape[0])
                held.append(score)
                rows.extend(zip(audio_fn, keys))
                continue
            for name, key, v in zip(audio_fn, keys, score.cpu().tolist()):
                fh.write(format_score_line(name, v, key))
                n += 1
        if held is not None:
            for (name, key), v in zip(rows, held.view().cpu().tolist()):
                fh.write(format_score_line(name, v, key))
                n += 1
    return n
