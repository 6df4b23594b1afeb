"""Drop-ins for the reference's loss heads (loss.py), one HIP launch per pass each.

``AngularIsoLoss`` / ``OCSoftmax`` (loss.py:62-97, :176-206): the OC-Softmax (``ang_iso``) head,
``forward(x, labels) -> (loss, -scores)``, attribute ``center`` (1, feat_dim) read by main_train.py:610
(csrc/ocsoftmax.hip).  ``P2SGradLoss`` (loss.py:244-335, ``--add_loss p2sgrad``), ``IsolateLoss`` /
``IsolateSquareLoss`` (loss.py:99-173, ``--add_loss isolate`` / ``iso_sq``) and the forward-only ``AMSoftmax``
(loss.py:209-234, scoring with ``--loss amsoftmax``) run on csrc/loss_heads.hip.  ``CrossEntropyLoss`` (the
default ``--add_loss None``, main_train.py:250-252) is adversarial.CrossEntropyLoss on air_softmax_ce_fwd/bwd.

Every module keeps the reference's constructor signature and defaults, attribute names, return types and seeded
construction (the same draws from the same generator), and pickles whole (main_train.py:676-706).
"""
import torch
import torch.nn as nn

from . import _hip, ops


def __getattr__(name):
    """``loss.CrossEntropyLoss`` is adversarial.CrossEntropyLoss (the ``--add_loss None`` head, main_train.py:251),
    resolved lazily: adversarial imports train, which imports this module."""
    if name == "CrossEntropyLoss":
        from .adversarial import CrossEntropyLoss
        return CrossEntropyLoss
    raise AttributeError(name)


def _gpu_rows(x, dim, what):
    if not x.is_cuda:
        raise _hip.AirError("%s HIP path needs GPU tensors; there is no CPU fallback" % what)
    if x.dim() != 2 or x.shape[1] != dim:
        raise ValueError("expected (B, %d) features, got %s" % (dim, tuple(x.shape)))


class _OCSoftmaxFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, center, labels, r_real, r_fake, alpha):
        x = x.contiguous()
        loss, neg = ops.ocsoftmax_fwd(x, center.detach().contiguous(), labels, r_real, r_fake, alpha)
        ctx.save_for_backward(x, center, labels)
        ctx.cfg = (r_real, r_fake, alpha)
        ctx.mark_non_differentiable(neg)
        return loss, neg

    @staticmethod
    def backward(ctx, dloss, _dneg):
        x, center, labels = ctx.saved_tensors
        r_real, r_fake, alpha = ctx.cfg
        g = dloss.reshape(1).float().contiguous()
        dx, dc = ops.ocsoftmax_bwd(x, center.detach().contiguous(), labels, r_real, r_fake, alpha, gscale=g)
        return dx, dc, None, None, None, None


class AngularIsoLoss(nn.Module):
    def __init__(self, feat_dim=2, r_real=0.9, r_fake=0.5, alpha=20.0):
        super().__init__()
        self.feat_dim = feat_dim
        self.r_real = r_real
        self.r_fake = r_fake
        self.alpha = alpha
        self.center = nn.Parameter(torch.randn(1, self.feat_dim))
        nn.init.kaiming_uniform_(self.center, 0.25)
        self.softplus = nn.Softplus()

    def forward(self, x, labels):
        """x: (B, feat_dim) GPU features; labels: (B,) 0 = bona fide, 1 = spoof."""
        if not x.is_cuda:
            raise _hip.AirError("OC-Softmax HIP path needs GPU tensors; there is no CPU fallback")
        if x.dim() != 2 or x.shape[1] != self.feat_dim:
            raise ValueError("expected (B, %d) features, got %s" % (self.feat_dim, tuple(x.shape)))
        labels = labels.to(device=x.device, dtype=torch.int64).contiguous()
        return _OCSoftmaxFn.apply(x.float(), self.center, labels, float(self.r_real),
                                  float(self.r_fake), float(self.alpha))


class OCSoftmax(AngularIsoLoss):
    """loss.py:176-206: identical arithmetic, kept under its second name."""


class _P2SGradFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight, labels, smooth):
        x = x.contiguous()
        w = weight.detach().contiguous()
        loss, neg = ops.p2sgrad_fwd(x, w, labels, smooth)
        ctx.save_for_backward(x, weight, labels)
        ctx.smooth = smooth
        ctx.mark_non_differentiable(neg)
        return loss, neg

    @staticmethod
    def backward(ctx, dloss, _dneg):
        x, weight, labels = ctx.saved_tensors
        g = dloss.reshape(1).float().contiguous()
        dx, dw = ops.p2sgrad_bwd(x, weight.detach().contiguous(), labels, ctx.smooth, gscale=g)
        return dx, dw, None, None


class P2SGradLoss(nn.Module):
    """loss.py:244-335: cos(x, renormed weight columns) against smoothed one-hot targets, MSE.
    ``forward(x, labels) -> (loss, -cos[:, 0])``; attribute ``weight`` (in_dim, out_dim).  main_train.py:274-277
    builds it as ``P2SGradLoss(enc_dim, 2, smooth=0.0)``.  out_dim <= 4 and in_dim <= 1024 on the HIP path."""

    def __init__(self, in_dim, out_dim, smooth=0.1):
        super().__init__()
        self.in_dim = in_dim
        self.out_dim = out_dim
        self.smooth = smooth
        self.weight = nn.Parameter(torch.Tensor(in_dim, out_dim))
        self.weight.data.uniform_(-1, 1).renorm_(2, 1, 1e-5).mul_(1e5)
        self.m_loss = nn.MSELoss()

    def forward(self, input_feat, target):
        _gpu_rows(input_feat, self.in_dim, "P2SGradLoss")
        labels = target.to(device=input_feat.device, dtype=torch.int64).contiguous()
        return _P2SGradFn.apply(input_feat.float(), self.weight, labels, float(self.smooth))


class _IsolateFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, center, labels, r_real, r_fake, square):
        x = x.contiguous()
        loss = ops.isolate_fwd(x, center.detach().contiguous(), labels, r_real, r_fake, square)
        ctx.save_for_backward(x, center, labels)
        ctx.cfg = (r_real, r_fake, square)
        return loss

    @staticmethod
    def backward(ctx, dloss):
        x, center, labels = ctx.saved_tensors
        g = dloss.reshape(1).float().contiguous()
        dx, dc = ops.isolate_bwd(x, center.detach().contiguous(), labels, *ctx.cfg, gscale=g)
        return dx, dc, None, None, None, None


class IsolateLoss(nn.Module):
    """loss.py:99-139: relu(|x - c| - r_real) over the bona fide rows + relu(r_fake - |x - c|) over the spoofed
    rows, each averaged over its rows.  Returns the bare scalar loss (NaN on a batch without one of the classes,
    as the reference).  Attribute ``center`` (1, feat_dim), drawn by randn with no further init."""
    SQUARE = False

    def __init__(self, num_classes=10, feat_dim=2, r_real=0.042, r_fake=1.638):
        super().__init__()
        self.num_classes = num_classes
        self.feat_dim = feat_dim
        self.r_real = r_real
        self.r_fake = r_fake
        self.center = nn.Parameter(torch.randn(1, self.feat_dim))

    def forward(self, x, labels):
        _gpu_rows(x, self.feat_dim, type(self).__name__)
        labels = labels.to(device=x.device, dtype=torch.int64).contiguous()
        return _IsolateFn.apply(x.float(), self.center, labels, float(self.r_real), float(self.r_fake), self.SQUARE)


class IsolateSquareLoss(IsolateLoss):
    """loss.py:141-173: IsolateLoss on squared norms against squared radii."""
    SQUARE = True


class AMSoftmax(nn.Module):
    """loss.py:209-234, forward only (the reference scores with it, ``--loss amsoftmax``, and never trains it):
    ``forward(feat, label) -> (logits, margin_logits)``.  Attribute ``centers`` (num_classes, enc_dim)."""

    def __init__(self, num_classes, enc_dim, s=20, m=0.9):
        super().__init__()
        self.enc_dim = enc_dim
        self.num_classes = num_classes
        self.s = s
        self.m = m
        self.centers = nn.Parameter(torch.randn(num_classes, enc_dim))

    def forward(self, feat, label):
        _gpu_rows(feat, self.enc_dim, "AMSoftmax")
        if torch.is_grad_enabled() and (feat.requires_grad or self.centers.requires_grad):
            raise NotImplementedError("AMSoftmax.forward is forward-only (use torch.no_grad()): the reference never "
                                      "trains through it")
        labels = label.to(device=feat.device, dtype=torch.int64).contiguous()
        return ops.amsoftmax_fwd(feat.float().contiguous(), self.centers.detach().contiguous(), labels, float(self.s),
                                 float(self.m))
