"""Test infrastructure: the bf16-RESIDENT arithmetic of ``Res2Net2(context=, summed=)`` - what the HIP path computes
under ``set_compute_dtype("bf16", variants=True)`` - composed from oracle/ecapa.py's own pieces (``RF`` / ``RG`` /
``RB``, ``_Bf16Conv``, ``_Bf16Pointwise``, ``bottle2neck_resident``, ``_SoftmaxStored``, ``_bn``).  oracle/ecapa.py
states the resident arithmetic for the constructor defaults only (context=True, summed=False) and its module docstring
says which tensors are rounded where; this module adds the two options and, for the defaults, IS that statement
(tests/test_ecapa_resident_variants_cpu.py holds it to ``ecapa_forward(bf16="resident")`` bit for bit).

``summed=True`` (ecapa_tdnn.py:163-166).  Blocks k = 1..3, s_0 = h (the stored bn1 output):
    x_k = block_k(s_{k-1})            the block's residual is its input s_{k-1}
    s_k = bf16(s_{k-1} + x_k)         both addends stored bf16 tensors: autocast's bf16 + bf16 add (the SE pass of
                                      block k writes x_k into its concat slice and s_k into a tensor of its own)
Backward, g_k = slice k of the (stored, bf16) concat gradient:
    d x_3 = g_3
    d s_{k-1} = bf16(conv1_k's dgrad + d x_k + d s_k)   ONE rounding of the three-term sum (d s_3 = 0): the epilogue of
                                                        block k's last dgrad GEMM with acc = d x_k, acc2 = d s_k
    d x_{k-1} = bf16(g_{k-1} + d s_{k-1})               both operands stored bf16 (air_h_add, over the concat slice)
Here: ``s = RB(s + x_k)`` around the unchanged ``bottle2neck_resident`` - autograd sums the three contributions to s_{k-1}
in fp32 and RB's backward rounds the sum once; x_k's gradient g_k + d s_k is rounded by the RB that closes the block.
Where the kernels differ from this statement (both as for the default options, neither new):
  * d s_0 = d h enters bn1's backward as a STORED bf16 tensor on the GPU; here it stays fp32 (``h = RF(...)``: the default
    statement does not round that gradient either, and the default case must stay bit-equal to it);
  * the fp32 three-term sum is formed as (dgrad + acc) + acc2 in the GEMM epilogue and in autograd's accumulation order
    here: the same real number up to one fp32 rounding before the bf16 one.

``context=False`` (:126-129, :177-180).  No context statistics exist: attention.0 is the plain pointwise GEMM on the stored
x4 with the layer's own (128, 1536, 1) weight and bias.  d(x4) is built in TWO stored steps, bf16(bf16(pooling) +
attention.0's dgrad) (``_X4Fan2``, the two-way counterpart of oracle.ecapa._X4Fan), then layer4's ReLU mask;
attention.0.weight's gradient is the (128, 1536) contraction alone.
"""
import numpy as np
import torch
import torch.nn.functional as F

from oracle import ecapa as oe
from oracle.ecapa import RB, RF, RG, _Bf16Conv, _Bf16Pointwise, _SoftmaxStored, _bn, _conv, _rnd, bottle2neck_resident
from oracle.loss import ocsoftmax_forward


class _X4Fan2(torch.autograd.Function):
    """context=False: layer4's output feeds the pooling and attention.0 only; the HIP backward builds d(x4) in two
    stored steps: bf16(pooling) -> bf16(. + attention.0's dgrad) [ReLU mask upstream]."""

    @staticmethod
    def forward(ctx, x):
        return x.clone(), x.clone()

    @staticmethod
    def backward(ctx, g_pool, g_att):
        return _rnd(_rnd(g_pool) + g_att)


def ecapa_forward_resident(p, x, scale=8, training=True, updates=None, taps=None, context=True, summed=False, out_bn=True):
    """Res2Net2.forward (ecapa_tdnn.py:152-198), encoder_type 'ECA', with bf16-resident activations, for every
    (context, summed).  x: (B, n_mels, T).  Returns (feat (B, 256), out (B, nOut))."""
    def tap(name, t):
        if taps is not None:
            taps[name] = t
        return t

    b1 = _rnd(p["conv1.bias"]) if oe.AUTOCAST_BIAS else p["conv1.bias"]
    c1 = _Bf16Conv.apply(x, p["conv1.weight"], 1, 2) + b1[None, :, None]  # :159
    h = RF(_bn(RB(F.relu(c1)), p, "bn1", training, updates))  # :160-161
    tap("h0", h)
    if summed:  # :163-166
        x1 = tap("x1", bottle2neck_resident(h, p, "layer1", 2, scale, training, updates))
        s1 = tap("s1", RB(h + x1))
        x2 = tap("x2", bottle2neck_resident(s1, p, "layer2", 3, scale, training, updates))
        s2 = tap("s2", RB(s1 + x2))
        x3 = tap("x3", bottle2neck_resident(s2, p, "layer3", 4, scale, training, updates))
    else:  # :167-170
        x1 = tap("x1", bottle2neck_resident(h, p, "layer1", 2, scale, training, updates))
        x2 = tap("x2", bottle2neck_resident(x1, p, "layer2", 3, scale, training, updates))
        x3 = tap("x3", bottle2neck_resident(x2, p, "layer3", 4, scale, training, updates))
    x4 = RF(F.relu(_conv(RG(torch.cat((x1, x2, x3), 1)), p, "layer4", bf16=True)))  # :172-173
    tap("layer4", x4)
    w0, c = p["attention.0.weight"], x4.shape[1]
    if context:  # :177-178
        x_pool, x_att, x_stat = oe._X4Fan.apply(x4)
        mean = x_stat.mean(2, keepdim=True)
        std = torch.sqrt(x_stat.var(2, keepdim=True).clamp(min=1e-4))
        a0 = (_Bf16Pointwise.apply(x_att, w0[:, :c]) + F.conv1d(torch.cat((mean, std), 1), w0[:, c:])
              + p["attention.0.bias"][None, :, None])
    else:  # :179-180
        x_pool, x_att = _X4Fan2.apply(x4)
        a0 = _Bf16Pointwise.apply(x_att, w0) + p["attention.0.bias"][None, :, None]
    a = RF(_bn(RB(F.relu(a0)), p, "attention.2", training, updates))
    logits = RB(_conv(RG(a), p, "attention.3", bf16=True))
    w = _SoftmaxStored.apply(logits)  # :139-145
    tap("w", w)
    mu = torch.sum(x_pool * w, dim=2)  # :184
    sg = torch.sqrt((torch.sum((x_pool ** 2) * w, dim=2) - mu ** 2).clamp(min=1e-4))  # :185
    tap("mu", mu)
    tap("sg", sg)
    y = _bn(torch.cat((mu, sg), 1), p, "bn5", training, updates)  # :187-189
    feat = F.linear(y, p["fc6.weight"], p["fc6.bias"])  # :191
    out = F.linear(feat, p["fc7.weight"], p["fc7.bias"])  # :193
    if out_bn:
        out = _bn(out, p, "bn7", training, updates)  # :195-196
    return feat, out


def loss_and_grads(params, center, x, labels, context=True, summed=False, r_real=0.9, r_fake=0.2, alpha=20.0):
    """One forward + AngularIsoLoss + backward of the resident arithmetic, as oracle.train.OracleTrainer.loss_and_grads
    (main_train.py:376, :406) does for the other modes.  Returns (loss, feat, grads by name, centre gradient, updates)."""
    names = [k for k, v in params.items() if v.dtype.is_floating_point and not k.endswith(("running_mean", "running_var"))]
    p = dict(params)
    for k in names:
        p[k] = params[k].detach().clone().requires_grad_(True)
    c = center.detach().clone().requires_grad_(True)
    updates = {}
    feat, _ = ecapa_forward_resident(p, x, training=True, updates=updates, context=context, summed=summed)
    loss, _ = ocsoftmax_forward(feat, c, labels, r_real, r_fake, alpha)
    loss.backward()
    return loss.detach(), feat.detach(), {k: p[k].grad for k in names}, c.grad, updates


# the input of the gradient tests (GPU: the HIP step; CPU: the oracle's fp32 evaluation against its own band)
GRAD_SHAPE, GRAD_SEED = (8, 60, 64), 464


def grad_labels(B):
    return (torch.arange(B) % 3 != 0).long()


ZERO_GRADS = ("attention.2.bias", "attention.3.bias")  # analytically zero (softmax over T ignores a shift of a row)


def gradient_band(x, labels, got, context, summed, params32=None, center32=None):
    """oracle.train.bf16_gradient_band for this module's arithmetic: ``band`` = the oracle's own fp32-vs-fp64 relative-L2
    gradient spread on this input (max / median over the tensors, smallest cosine) and the fp64 loss; ``errs[name]`` =
    (relative L2, cosine) of ``got[name]`` (flat float64 arrays) against the fp64 evaluation.  got=None: the fp32
    evaluation stands in for the run under test (errs = the band's own samples)."""
    from oracle.filler import fill_state, fill_value
    p32 = fill_state(oe.ecapa_shapes(context=context)) if params32 is None else params32
    c32 = fill_value("center", (1, 256)) if center32 is None else center32
    p64 = {k: (v.double() if v.dtype.is_floating_point else v) for k, v in p32.items()}
    l64, _, g64, _, _ = loss_and_grads(p64, c32.double(), x.double(), labels, context, summed)
    _, _, g32, _, _ = loss_and_grads(p32, c32, x, labels, context, summed)
    own, own_cos, errs = [], [], {}
    for k, ref in g64.items():
        if ref is None or k in ZERO_GRADS:
            continue
        r = ref.numpy().ravel()
        nr = np.linalg.norm(r) + 1e-30
        o32 = g32[k].double().numpy().ravel()
        own.append(np.linalg.norm(o32 - r) / nr)
        own_cos.append(float(o32 @ r) / (np.linalg.norm(o32) * nr + 1e-30))
        g = o32 if got is None else got[k]
        errs[k] = (np.linalg.norm(g - r) / nr, float(g @ r) / (np.linalg.norm(g) * nr + 1e-30))
    return {"max": float(max(own)), "median": float(np.median(own)), "loss64": l64.item(),
            "min_cos": float(min(own_cos))}, errs
