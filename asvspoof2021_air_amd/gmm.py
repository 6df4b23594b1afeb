"""Diagonal-covariance GMM back-end on the device: fp64 EM and log-likelihood-ratio scoring.

The ASVspoof baselines B01 / B02 are a pair of diagonal GMMs - bona fide and spoof - on LFCC or CQCC frames, scored by
the log-likelihood ratio; it is the number every paper reports beside its network and the usual second system of a
fusion.  ``DiagGMM`` is one such model, ``GMMBackend`` the pair behind a PCM front-end.  The arithmetic is the
specification in include/air_hip.h ("GMM back-end"): scikit-learn 1.7's ``GaussianMixture(covariance_type="diag")``
from a given initialisation, carried in fp64 on the matrix cores (csrc/gmm.hip) - in fp32 the ``E[x^2] - mu^2`` and
``x^2 p - 2 x mu p`` cancellations lose the covariances of LFCC-like frames within a few iterations.

Parity is claimed with scikit-learn's EM from a given initialisation (tests/gmm_oracle.py, tests/test_gmm_cpu.py); not
with its k-means initialisation, nor with the challenge's MATLAB / Python baseline scripts.  There is no CPU fallback.
"""
import ctypes

import numpy as np
import torch

from . import _hip
from .devbuf import DeviceVector
from .ragged import device_lengths

MAX_COMPONENTS, MAX_FEATURES = 1024, 128
LAYOUTS = {"btd": 0, "nd": 0, "bdt": 1}


_lib = _hip.lib


def ws_bytes(n_frames_cap, K, D):
    """``air_gmm_ws_bytes``: the scratch one accumulate / loglik call over ``n_frames_cap`` frame slots needs."""
    return _lib().air_gmm_ws_bytes(ctypes.c_int64(int(n_frames_cap)), _hip.ci(K), _hip.ci(D))


def frame_tile():
    return _lib().air_gmm_frame_tile()


def _check_shape(K, D):
    if not (1 <= K <= MAX_COMPONENTS):
        raise ValueError("n_components must be 1 .. %d, got %d" % (MAX_COMPONENTS, K))
    if not (1 <= D <= MAX_FEATURES):
        raise ValueError("n_features must be 1 .. %d, got %d" % (MAX_FEATURES, D))


def _frames(feats, n_frames, layout, D):
    """-> (contiguous fp32 feats, layout id, B, Tcap, int32 n_frames or None).  2-d feats are (N, D); 3-d feats are
    (B, D, Tcap) - what the front-ends write - unless ``layout="btd"`` says (B, Tcap, D)."""
    if layout is not None and layout not in LAYOUTS:
        raise ValueError("layout must be one of %s, got %r" % (sorted(LAYOUTS), layout))
    if not (torch.is_tensor(feats) and feats.is_cuda):
        raise _hip.AirError("the GMM back-end takes GPU tensors; there is no CPU fallback")
    if layout is None:
        layout = "nd" if feats.dim() == 2 else "bdt"
    if feats.dtype != torch.float32:
        raise ValueError("frames are float32, got %s" % feats.dtype)
    if feats.dim() == 2 and layout != "bdt":
        B, Tcap, d = 1, feats.shape[0], feats.shape[1]
    elif feats.dim() == 3:
        B = feats.shape[0]
        Tcap, d = (feats.shape[2], feats.shape[1]) if layout == "bdt" else (feats.shape[1], feats.shape[2])
    else:
        raise ValueError("frames are (N, D), (B, Tcap, D) or (B, D, Tcap), got %s as %r" % (tuple(feats.shape), layout))
    if d != D:
        raise ValueError("the model has %d features, the frames %d" % (D, d))
    if B < 1 or Tcap < 1:
        raise ValueError("an empty batch: %s" % (tuple(feats.shape),))
    if B * Tcap >= 1 << 31:
        raise ValueError("B * Tcap must stay below 2^31, got %d" % (B * Tcap))
    if n_frames is not None:
        if not (torch.is_tensor(n_frames) and n_frames.is_cuda):
            n_frames = torch.as_tensor(n_frames, dtype=torch.int32).to(feats.device)
        if n_frames.numel() != B:
            raise ValueError("n_frames must have %d entries, got %d" % (B, n_frames.numel()))
        n_frames = n_frames.to(torch.int32).contiguous()
    return feats.contiguous(), LAYOUTS[layout], B, Tcap, n_frames


class _StopRule:
    """scikit-learn's loop control (BaseMixture.fit): stop when abs(change of the lower bound) < tol."""

    def __init__(self, max_iter, tol):
        self.max_iter, self.tol = int(max_iter), float(tol)
        self.lower_bound, self.n_iter, self.converged = -np.inf, 0, False

    @property
    def done(self):
        return self.converged or self.n_iter >= self.max_iter

    def update(self, lower_bound):
        prev, self.lower_bound = self.lower_bound, float(lower_bound)
        self.n_iter += 1
        if abs(self.lower_bound - prev) < self.tol:
            self.converged = True


class DiagGMM:
    """``DiagGMM(n_components=512, n_features=60, reg_covar=1e-6, device="cuda")``: fp64 device tensors ``weights_``
    (K), ``means_`` (K, D), ``covariances_`` (K, D); ``lower_bound_``, ``n_iter_``, ``converged_`` as scikit-learn
    sets them.  ``begin()`` / ``accumulate(...)`` / ``m_step()`` are one EM iteration streamed over any number of
    batches, without a host synchronisation; ``fit`` runs them under scikit-learn's stop rule."""

    def __init__(self, n_components=512, n_features=60, reg_covar=1e-6, device="cuda"):
        K, D = int(n_components), int(n_features)
        _check_shape(K, D)
        if not reg_covar >= 0.0:
            raise ValueError("reg_covar must be non-negative, got %r" % (reg_covar,))
        self.n_components, self.n_features, self.reg_covar = K, D, float(reg_covar)
        self.device = torch.device(device)
        self.weights_ = self.means_ = self.covariances_ = None
        self.lower_bound_, self.n_iter_, self.converged_ = -np.inf, 0, False
        self._params = self._stats = self._ws = self._lb = None
        self._packed = False

    # ------------------------------------------------------------------------------------------------- parameters
    def set_params(self, weights, means, covariances):
        K, D = self.n_components, self.n_features

        def dev(a, shape, what):
            t = torch.as_tensor(a, dtype=torch.float64).to(self.device).contiguous().clone()
            if tuple(t.shape) != shape:
                raise ValueError("%s must be %s, got %s" % (what, shape, tuple(t.shape)))
            return t
        self.weights_ = dev(weights, (K,), "weights")
        self.means_ = dev(means, (K, D), "means")
        self.covariances_ = dev(covariances, (K, D), "covariances")
        self._packed = False
        return self

    def _need_model(self):
        if self.weights_ is None:
            raise RuntimeError("the model has no parameters yet: set_params, init_from_frames or load_state_dict first")

    def _operand(self):
        """The packed E-step operand of the current parameters (``air_gmm_prepare``), repacked when they changed."""
        self._need_model()
        L = _lib()
        K, D = self.n_components, self.n_features
        if self._params is None:
            self._params = torch.empty(L.air_gmm_params_doubles(_hip.ci(K), _hip.ci(D)), dtype=torch.float64,
                                       device=self.device)
        if not self._packed:
            _hip.check(L.air_gmm_prepare(_hip.dptr(self.weights_, torch.float64), _hip.dptr(self.means_, torch.float64),
                                         _hip.dptr(self.covariances_, torch.float64), _hip.ci(K), _hip.ci(D),
                                         _hip.dptr(self._params, torch.float64), _hip.stream()), "air_gmm_prepare")
            self._packed = True
        return self._params

    def _scratch(self, n):
        # the model's own scratch: growing the stream's shared workspace would make a trainer re-capture its step
        need = ws_bytes(n, self.n_components, self.n_features)
        if self._ws is None or self._ws.numel() < need:
            self._ws = torch.empty(need, dtype=torch.uint8, device=self.device)
        return self._ws

    # ------------------------------------------------------------------------------------------------------- EM
    def begin(self):
        """Start an EM iteration: zero statistics."""
        n = _lib().air_gmm_stats_doubles(_hip.ci(self.n_components), _hip.ci(self.n_features))
        if self._stats is None:
            self._stats = torch.zeros(n, dtype=torch.float64, device=self.device)
        else:
            self._stats.zero_()
        return self

    def accumulate(self, feats, n_frames=None, layout=None):
        """Add the batch's S0, S1, S2, LL and frame count under the current parameters (``air_gmm_accumulate``)."""
        if self._stats is None:
            self.begin()
        x, lay, B, Tcap, nf = _frames(feats, n_frames, layout, self.n_features)
        ws = self._scratch(B * Tcap)
        _hip.check(_lib().air_gmm_accumulate(_hip.dptr(x), _hip.ci(lay), _hip.ci(B), _hip.ci(Tcap),
                                             _hip.dptr(nf, torch.int32, True), _hip.dptr(self._operand(), torch.float64),
                                             _hip.ci(self.n_components), _hip.ci(self.n_features),
                                             _hip.dptr(self._stats, torch.float64), _hip.dptr(ws, torch.uint8),
                                             _hip.csz(ws.numel()), _hip.stream()), "air_gmm_accumulate")
        return self

    def statistics(self):
        """Views of the running statistics: (S0 (K), S1 (K, D), S2 (K, D), LL (), Nf () int64)."""
        K, D = self.n_components, self.n_features
        s = self._stats
        return (s[:K], s[K:K + K * D].view(K, D), s[K + K * D:K + 2 * K * D].view(K, D), s[K + 2 * K * D],
                s[K + 2 * K * D + 1:].view(torch.int64)[0])

    def m_step(self):
        """The M-step on the device (``air_gmm_mstep``); returns the iteration's lower bound as a device scalar."""
        if self._stats is None:
            raise RuntimeError("m_step() without begin() / accumulate()")
        K, D = self.n_components, self.n_features
        if self.weights_ is None:
            self.weights_ = torch.empty(K, dtype=torch.float64, device=self.device)
            self.means_ = torch.empty((K, D), dtype=torch.float64, device=self.device)
            self.covariances_ = torch.empty((K, D), dtype=torch.float64, device=self.device)
        if self._lb is None:
            self._lb = torch.empty(1, dtype=torch.float64, device=self.device)
        _hip.check(_lib().air_gmm_mstep(_hip.dptr(self._stats, torch.float64), _hip.ci(K), _hip.ci(D),
                                        ctypes.c_double(self.reg_covar), _hip.dptr(self.weights_, torch.float64),
                                        _hip.dptr(self.means_, torch.float64), _hip.dptr(self.covariances_, torch.float64),
                                        _hip.dptr(self._lb, torch.float64), _hip.stream()), "air_gmm_mstep")
        self._packed = False
        return self._lb[0]

    def fit(self, batches, max_iter=100, tol=1e-3):
        """EM from the current parameters.  ``batches``: a callable returning a fresh iterable of ``(feats, n_frames)``
        (or ``(feats, n_frames, layout)``) per iteration.  One 8-byte copy per iteration, none per batch."""
        self._need_model()
        rule = _StopRule(max_iter, tol)
        while not rule.done:
            self.begin()
            for batch in batches():
                self.accumulate(*batch)
            rule.update(self.m_step().item())
        self.lower_bound_, self.n_iter_, self.converged_ = rule.lower_bound, rule.n_iter, rule.converged
        return self

    def init_from_frames(self, feats, n_frames=None, layout=None, seed=0):
        """scikit-learn's ``random_from_data`` idea: the means are K distinct valid frames drawn with
        ``numpy.random.default_rng(seed)`` on the host (this synchronises; it runs once), every covariance row is the
        global variance of the given frames (from one accumulate of a K = 1 model, whose S0, S1, S2 are N, sum x,
        sum x^2) plus ``reg_covar``, the weights are uniform."""
        K, D = self.n_components, self.n_features
        x, lay, B, Tcap, nf = _frames(feats, n_frames, layout, D)
        counts = np.full(B, Tcap, dtype=np.int64) if nf is None else np.clip(nf.cpu().numpy().astype(np.int64), 0, Tcap)
        total = int(counts.sum())
        if total < K:
            raise ValueError("%d components need at least as many frames, got %d" % (K, total))
        pick = np.sort(np.random.default_rng(seed).choice(total, K, replace=False))
        ends = np.cumsum(counts)
        rows = np.searchsorted(ends, pick, side="right")
        ts = pick - (ends[rows] - counts[rows])
        rows_d, ts_d = torch.from_numpy(rows).to(self.device), torch.from_numpy(ts).to(self.device)
        means = (x[rows_d, :, ts_d] if lay == 1 else x.view(B, Tcap, D)[rows_d, ts_d]).double()
        one = DiagGMM(1, D, 0.0, self.device).set_params(torch.ones(1), torch.zeros(1, D), torch.ones(1, D))
        one.begin().accumulate(x, nf, layout or ("nd" if feats.dim() == 2 else "bdt"))
        S0, S1, S2, _, _ = one.statistics()
        mean = S1[0] / S0[0]
        var = S2[0] / S0[0] - mean * mean + self.reg_covar
        return self.set_params(torch.full((K,), 1.0 / K, dtype=torch.float64), means, var.expand(K, D))

    # ---------------------------------------------------------------------------------------------------- scores
    def _loglik(self, feats, n_frames, layout, want_frames, want_rows, out=None):
        x, lay, B, Tcap, nf = _frames(feats, n_frames, layout, self.n_features)
        ws = self._scratch(B * Tcap)
        frame_ll = row_ll = None
        if out is not None and (out.dtype != torch.float64 or out.numel() != (B * Tcap if want_frames else B)
                                or not out.is_contiguous() or out.device != x.device):
            raise ValueError("out must be a contiguous float64 device tensor of %d elements" % (B * Tcap if want_frames else B))
        if want_frames:
            frame_ll = out.view(-1) if out is not None else torch.empty(B * Tcap, dtype=torch.float64, device=self.device)
        if want_rows:
            row_ll = out.view(-1) if out is not None else torch.empty(B, dtype=torch.float64, device=self.device)
        _hip.check(_lib().air_gmm_loglik(_hip.dptr(x), _hip.ci(lay), _hip.ci(B), _hip.ci(Tcap),
                                         _hip.dptr(nf, torch.int32, True), _hip.dptr(self._operand(), torch.float64),
                                         _hip.ci(self.n_components), _hip.ci(self.n_features),
                                         _hip.dptr(frame_ll, torch.float64, True), _hip.dptr(row_ll, torch.float64, True),
                                         _hip.dptr(ws, torch.uint8), _hip.csz(ws.numel()), _hip.stream()), "air_gmm_loglik")
        if frame_ll is not None:
            frame_ll = frame_ll if feats.dim() == 2 else frame_ll.view(B, Tcap)
        return frame_ll, row_ll

    def score_samples(self, feats, n_frames=None, layout=None, out=None):
        """log p(x) per frame, fp64: (N,) for (N, D) frames, else (B, Tcap) with 0 behind each row's frames.  ``out``:
        an optional float64 device tensor of that many elements to write into."""
        return self._loglik(feats, n_frames, layout, True, False, out)[0]

    def score_rows(self, feats, n_frames=None, layout=None, out=None):
        """The mean of log p(x) over each row's frames, fp64 (B,); NaN for a row without frames."""
        return self._loglik(feats, n_frames, layout, False, True, out)[1]

    # ----------------------------------------------------------------------------------------------------- state
    def state_dict(self):
        self._need_model()
        return {"weights": self.weights_.clone(), "means": self.means_.clone(), "covariances": self.covariances_.clone(),
                "reg_covar": self.reg_covar, "lower_bound": self.lower_bound_, "n_iter": self.n_iter_,
                "converged": self.converged_}

    def load_state_dict(self, state):
        self.set_params(state["weights"], state["means"], state["covariances"])
        self.reg_covar = float(state.get("reg_covar", self.reg_covar))
        self.lower_bound_ = float(state.get("lower_bound", -np.inf))
        self.n_iter_, self.converged_ = int(state.get("n_iter", 0)), bool(state.get("converged", False))
        return self

    def to_sklearn(self):
        """A fitted ``sklearn.mixture.GaussianMixture`` holding these parameters (scikit-learn is imported here)."""
        from sklearn.mixture import GaussianMixture
        self._need_model()
        gm = GaussianMixture(n_components=self.n_components, covariance_type="diag", reg_covar=self.reg_covar)
        gm.weights_ = self.weights_.cpu().numpy()
        gm.means_ = self.means_.cpu().numpy()
        gm.covariances_ = self.covariances_.cpu().numpy()
        gm.precisions_cholesky_ = 1.0 / np.sqrt(gm.covariances_)
        gm.precisions_ = gm.precisions_cholesky_ ** 2
        gm.converged_, gm.n_iter_, gm.lower_bound_ = self.converged_, self.n_iter_, self.lower_bound_
        gm.n_features_in_ = self.n_features
        return gm

    @classmethod
    def from_sklearn(cls, gm, device="cuda"):
        """The model of a fitted diagonal ``GaussianMixture``; any other covariance type: ValueError."""
        if getattr(gm, "covariance_type", None) != "diag":
            raise ValueError("only covariance_type='diag' is served, got %r" % (getattr(gm, "covariance_type", None),))
        means = np.asarray(gm.means_, dtype=np.float64)
        m = cls(means.shape[0], means.shape[1], gm.reg_covar, device)
        m.set_params(np.asarray(gm.weights_, dtype=np.float64), means, np.asarray(gm.covariances_, dtype=np.float64))
        m.lower_bound_ = float(getattr(gm, "lower_bound_", -np.inf))
        m.n_iter_, m.converged_ = int(getattr(gm, "n_iter_", 0)), bool(getattr(gm, "converged_", False))
        return m


def _unpack(batch):
    """``(pcm, labels[, start[, lengths[, groups]]])`` as Trainer.step / Trainer.evaluate take it (a DeviceBatch's
    first four fields); the crop offsets do not apply: every frame of an utterance counts."""
    pcm, labels = batch[0], batch[1]
    lengths = batch[3] if len(batch) > 3 else None
    return pcm, labels, lengths


class GMMBackend:
    """``GMMBackend(n_components=512, frontend=None, reg_covar=1e-6, device="cuda")``: the models ``bona`` and ``spoof``
    behind a PCM front-end (default: the trainer's LFCC(320, 160, 512, 16000, 20), not mutating its input).  An
    utterance's score is mean log p_bona - mean log p_spoof over its own frames; higher means bona fide."""

    def __init__(self, n_components=512, frontend=None, reg_covar=1e-6, device="cuda"):
        if frontend is None:
            from .feature_extraction import LFCC
            frontend = LFCC(320, 160, 512, 16000, 20, with_energy=False)
            frontend.mutate_input = False
        # a caller's front-end is used as it is: forward_padded / forward_ragged, the only calls made, never mutate
        # their input whatever its mutate_input says
        self.frontend, self.device = frontend, torch.device(device)
        D = frontend.out_dim
        self.bona = DiagGMM(n_components, D, reg_covar, device)
        self.spoof = DiagGMM(n_components, D, reg_covar, device)

    def frames(self, pcm, lengths=None):
        """(B, Lcap) PCM -> (feats (B, D, Tcap) with Tcap = 1 + Lcap // hop, n_frames int32 (B,) on the device):
        utterance b owns min(1 + lengths[b] // hop, Tcap) frames; what follows them is zero padding no model reads."""
        B, Lcap = pcm.shape
        hop = self.frontend.fs
        Tcap = 1 + Lcap // hop
        if lengths is None:
            feats = self.frontend.forward_padded(pcm, feat_len=Tcap, padding="zero")
            return feats, torch.full((B,), Tcap, dtype=torch.int32, device=pcm.device)
        lengths = device_lengths(lengths, B, Lcap, pcm.device)
        feats = self.frontend.forward_ragged(pcm, lengths, feat_len=Tcap, padding="zero")
        n_frames = (1 + torch.div(lengths.clamp(1, Lcap), hop, rounding_mode="floor")).clamp(max=Tcap).to(torch.int32)
        return feats, n_frames

    def _routed(self, batch):
        pcm, labels, lengths = _unpack(batch)
        feats, nf = self.frames(pcm, lengths)
        labels = labels.to(device=self.device, non_blocking=True)
        zero = torch.zeros_like(nf)
        return feats, torch.where(labels == 0, nf, zero), torch.where(labels != 0, nf, zero)

    @staticmethod
    def _iterate(batches):
        if callable(batches):
            return batches()
        if hasattr(batches, "epoch"):
            return batches.epoch()
        return batches

    def fit(self, batches, max_iter=10, tol=1e-3, seed=0):
        """EM of both models over batches ``(pcm, labels[, start[, lengths]])`` - a list, a callable returning a fresh
        iterable per iteration, or a ``CorpusSampler`` (one ``epoch()`` per iteration).  Each batch's frames are computed
        once and feed both models; a row reaches the model of its label (0 = bona fide) by a zero frame count for the
        other, with no host synchronisation and no compaction.  Models without parameters are initialised from the first
        batch alone (``DiagGMM.init_from_frames``, which synchronises once): a first batch with fewer than
        ``n_components`` frames of a class raises its ValueError - use a larger batch for the fit, or initialise the
        models beforehand (``backend.bona.init_from_frames`` / ``set_params``), which ``fit`` then leaves as they are.  Each model stops on its own rule; the two lower
        bounds come back in one 16-byte copy per iteration."""
        models = (self.bona, self.spoof)
        if any(m.weights_ is None for m in models):
            for batch in self._iterate(batches):
                feats, nf_b, nf_s = self._routed(batch)
                for i, (m, nf) in enumerate(((self.bona, nf_b), (self.spoof, nf_s))):
                    if m.weights_ is None:
                        m.init_from_frames(feats, nf, "bdt", seed=seed + i)
                break
        rules = [_StopRule(max_iter, tol), _StopRule(max_iter, tol)]
        while not all(r.done for r in rules):
            live = [i for i in (0, 1) if not rules[i].done]
            for i in live:
                models[i].begin()
            for batch in self._iterate(batches):
                routed = self._routed(batch)
                for i in live:
                    models[i].accumulate(routed[0], routed[1 + i], "bdt")
            bounds = torch.stack([models[i].m_step() for i in live]).cpu().tolist()
            for i, lb in zip(live, bounds):
                rules[i].update(lb)
        for m, r in zip(models, rules):
            m.lower_bound_, m.n_iter_, m.converged_ = r.lower_bound, r.n_iter, r.converged
        return self

    def score_frames(self, feats, n_frames=None, layout=None):
        """The LLR of rows of frames, fp32 (B,)."""
        return (self.bona.score_rows(feats, n_frames, layout) - self.spoof.score_rows(feats, n_frames, layout)).float()

    def score(self, pcm, lengths=None):
        """The LLR of each utterance, fp32 (B,) on the device."""
        feats, nf = self.frames(pcm, lengths)
        return self.score_frames(feats, nf, "bdt")

    def state_dict(self):
        return {"bona": self.bona.state_dict(), "spoof": self.spoof.state_dict()}

    def load_state_dict(self, state):
        self.bona.load_state_dict(state["bona"])
        self.spoof.load_state_dict(state["spoof"])
        return self

    @torch.no_grad()
    def evaluate(self, batches, tdcf=None, n_groups=None, group_names=None, capacity=None):
        """The dev / eval pass of ``Trainer.evaluate`` for this back-end: scores and labels stay on the device, the EER
        of both polarities and, with ``tdcf``, the min t-DCF of the better one come from
        ``eval_metrics.DeviceGroupedMinima`` in ONE copy.  Returns the trainer's ``EvalResult`` (``loss`` is NaN: the
        back-end has none); its ``scores`` can go into ``score_fusion.fuse_device`` beside the networks'.  ``n_groups``,
        ``group_names`` and a five-element ``tdcf`` as there (batches then carry the groups as their fifth item)."""
        # (the argument checks, the buffers and the by_group assembly restate train.Trainer.evaluate, which this change
        # may not touch; a later change should move them into one helper both call)
        from .eval_metrics import DeviceGroupedMinima, _rates_of_group, tdcf_weights
        from .ops import EVAL_MAX_GROUPS, EVAL_RECORD_WORDS
        from .train import EvalResult, GroupResult
        weights = tdcf_weights(*tdcf[:4]) if tdcf is not None else None
        grouped = n_groups is not None
        if not grouped and (group_names is not None or (tdcf is not None and len(tdcf) > 4)):
            raise ValueError("group_names and per-group t-DCF rates need n_groups")
        if grouped:
            n_groups = int(n_groups)
            if n_groups < 1 or n_groups > EVAL_MAX_GROUPS:
                raise ValueError("n_groups must be 1 .. %d, got %d" % (EVAL_MAX_GROUPS, n_groups))
            if group_names is not None and len(group_names) != n_groups:
                raise ValueError("group_names must name %d groups, got %d" % (n_groups, len(group_names)))
            if weights is not None:
                rates = _rates_of_group(tdcf[4] if len(tdcf) > 4 else tdcf[:3], n_groups)
                weights = [weights] + [tdcf_weights(*r, tdcf[3]) for r in rates]
        scores = labs = grps = None
        for batch in self._iterate(batches):
            if grouped and len(batch) != 5:
                raise ValueError("with n_groups a batch is (pcm, labels, start, lengths, groups), got %d items" % len(batch))
            pcm, labels, lengths = _unpack(batch)
            if scores is None:
                trials = capacity if capacity is not None else 64 * pcm.shape[0]
                scores = DeviceVector(torch.float32, self.device, trials)
                labs = DeviceVector(torch.int64, self.device, trials)
                grps = DeviceVector(torch.int64, self.device, trials) if grouped else None
            scores.append(self.score(pcm, lengths))
            labs.append(labels.to(device=self.device, dtype=torch.int64, non_blocking=True))
            if grouped:
                grps.append(batch[4].to(device=self.device, dtype=torch.int64, non_blocking=True))
        if scores is None:
            raise ValueError("evaluate() needs at least one batch")
        if grouped and grps.n != scores.n:
            raise ValueError("the batches gave %d groups for %d trials" % (grps.n, scores.n))
        words = 2 * ((n_groups or 0) + 1) * EVAL_RECORD_WORDS
        pack = torch.empty(words, dtype=torch.int32, device=self.device)
        minima = DeviceGroupedMinima(scores.view(), labs.view(), grps.view() if grouped else None, n_groups or 0,
                                     (False, True), weights, out=pack)
        minima.fetch(pack.cpu().numpy())
        eers = (minima.eer(0)[0], minima.eer(1)[0])
        win = 0 if eers[0] < eers[1] else 1
        out = EvalResult(float("nan"), min(eers), minima.min_tdcf(win)[0] if weights is not None else None, scores.view(),
                         labs.view())
        if grouped:
            out.by_group = []
            for g in range(n_groups):
                pair = (minima.eer(0, g), minima.eer(1, g))
                out.by_group.append(None if pair[0] is None else GroupResult(
                    g if group_names is None else group_names[g], (pair[0][0], pair[1][0]), pair[win][0],
                    minima.min_tdcf(win, g)[0] if weights is not None else None))
        return out
