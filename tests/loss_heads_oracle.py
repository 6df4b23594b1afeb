"""Test helper: the reference's loss heads (loss.py:99-173 Isolate / IsolateSquare, :209-234 AMSoftmax, :244-335
P2SGrad, main_train.py:251 cross-entropy) restated in plain torch ops, in any dtype (fp64 for parity; gradients by
autograd), and the inputs every head test shares (regenerated from oracle.filler seeds)."""
import torch
import torch.nn.functional as F

from oracle.filler import fill_value, synth_feat

D = 256


def p2sgrad(x, weight, labels, smooth=0.0):
    """(loss, -cos[:, 0]) of P2SGradLoss.forward (loss.py:300-335)."""
    w = weight.renorm(2, 1, 1e-5).mul(1e5)
    x_modulus = x.pow(2).sum(1).pow(0.5)
    cos = (x.mm(w) / x_modulus.view(-1, 1)).clamp(-1, 1)
    C = w.shape[1]
    target = F.one_hot(labels.long(), C).to(x.dtype) * (1 - smooth) + smooth / C
    return F.mse_loss(cos, target), -cos[:, 0]


def isolate(x, center, labels, r_real=0.042, r_fake=1.638, square=False):
    """IsolateLoss.forward (loss.py:119-139); square: IsolateSquareLoss.forward (:155-173)."""
    n0 = torch.norm(x[labels == 0] - center, p=2, dim=1)
    n1 = torch.norm(x[labels == 1] - center, p=2, dim=1)
    if square:
        return F.relu(torch.pow(n0, 2) - r_real ** 2).mean() + F.relu(r_fake ** 2 - torch.pow(n1, 2)).mean()
    return F.relu(n0 - r_real).mean() + F.relu(r_fake - n1).mean()


def amsoftmax(feat, centers, labels, s=20, m=0.9):
    """(logits, margin_logits) of AMSoftmax.forward (loss.py:217-234)."""
    nfeat = feat / torch.norm(feat, p=2, dim=-1, keepdim=True)
    ncenters = centers / torch.norm(centers, p=2, dim=-1, keepdim=True)
    logits = nfeat @ ncenters.t()
    onehot = torch.zeros_like(logits).scatter_(1, labels.long().unsqueeze(-1), m)
    return logits, s * (logits - onehot)


def cross_entropy(logits, labels):
    return F.cross_entropy(logits, labels.long())


# ------------------------------------------------------------------------------------------------ shared inputs
SEED_X = 1301


def inputs(B, seed=SEED_X, scale=0.1):
    """x (B, 256) as the reference's features are scaled (|x| ~ 1.6), mixed labels 0, 1, 0, 1, ..."""
    x = synth_feat((B, D), seed=seed, scale=scale)
    labels = torch.arange(B) % 2
    return x, labels


def params():
    """The head parameters the fixtures use: P2SGrad weight (256, 2), Isolate centre (1, 256), AMSoftmax centres (2, 256)."""
    return {"p2s": fill_value("p2sgrad.weight", (D, 2)), "iso": 0.1 * fill_value("isolate.center", (1, D)),
            "ams": fill_value("amsoftmax.centers", (2, D))}


def grads(fn, *tensors):
    """fn(*leaves) -> loss (or (loss, ...)); returns (outputs, [grad of each leaf]) by autograd."""
    leaves = [t.detach().clone().requires_grad_(True) for t in tensors]
    out = fn(*leaves)
    loss = out[0] if isinstance(out, tuple) else out
    loss.backward()
    return out, [lf.grad for lf in leaves]
