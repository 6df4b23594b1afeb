"""Test helper: SE-Res2Net-50 (model.py:256-509) restated in plain torch ops (F.conv2d / batch_norm / avg_pool2d /
linear / log_softmax) over a name -> tensor parameter dict, in any dtype (fp64 for parity)."""
import math

import torch
import torch.nn.functional as F

LAYERS = ((16, 3, 1), (32, 4, 2), (64, 6, 2), (128, 3, 2))  # (planes, blocks, stride) of layer1 .. layer4


def blocks(layers=(3, 4, 6, 3), base_width=26, scale=4):
    """(name, inplanes, planes, stride, width, stage, downsample kernel or None) of every block, in order."""
    out, inplanes = [], 16
    for li, ((planes, _, stride), nb) in enumerate(zip(LAYERS, layers)):
        width = int(math.floor(planes * (base_width / 64.0)))
        for bi in range(nb):
            first = bi == 0
            ds = stride if first and (stride != 1 or inplanes != planes * 2) else None
            out.append(("layer%d.%d" % (li + 1, bi), inplanes, planes, stride if first else 1, width, first, ds))
            inplanes = planes * 2
    return out


def state_shapes(num_classes=2):
    """state_dict names and shapes of model.Res2Net(SEBottle2neck, [3, 4, 6, 3], 26, 4), in order."""
    out = {}

    def bn(n, c):
        for k in ("weight", "bias", "running_mean", "running_var"):
            out["%s.%s" % (n, k)] = (c,)
        out[n + ".num_batches_tracked"] = ()

    out["conv1.0.weight"] = (16, 1, 3, 3)
    bn("conv1.1", 16)
    out["conv1.3.weight"] = (16, 16, 3, 3)
    bn("conv1.4", 16)
    out["conv1.6.weight"] = (16, 16, 3, 3)
    bn("bn1", 16)
    for name, cin, planes, _, w, _, ds in blocks():
        out[name + ".conv1.weight"] = (4 * w, cin, 1, 1)
        bn(name + ".bn1", 4 * w)
        for i in range(3):
            out["%s.convs.%d.weight" % (name, i)] = (w, w, 3, 3)
        for i in range(3):
            bn("%s.bns.%d" % (name, i), w)
        out[name + ".conv3.weight"] = (2 * planes, 4 * w, 1, 1)
        bn(name + ".bn3", 2 * planes)
        out[name + ".se.fc.0.weight"] = (2 * planes // 16, 2 * planes)
        out[name + ".se.fc.2.weight"] = (2 * planes, 2 * planes // 16)
        if ds is not None:
            out[name + ".downsample.1.weight"] = (2 * planes, cin, 1, 1)
            bn(name + ".downsample.2", 2 * planes)
    out["cls_layer.weight"] = (num_classes, 256)
    out["cls_layer.bias"] = (num_classes,)
    return out


def forward(P, x, training, buffers=None, momentum=0.1, eps=1e-5):
    """(feat, log-probs).  P: parameters by state_dict name; buffers: running statistics by name (updated in place in
    training mode when given; eval mode needs them)."""
    def bn(n, t):
        rm = buffers.get(n + ".running_mean") if buffers is not None else None
        rv = buffers.get(n + ".running_var") if buffers is not None else None
        return F.batch_norm(t, rm, rv, P[n + ".weight"], P[n + ".bias"], training, momentum, eps)

    t = F.conv2d(x, P["conv1.0.weight"], padding=1)
    t = F.relu(bn("conv1.1", t))
    t = F.conv2d(t, P["conv1.3.weight"], padding=1)
    t = F.relu(bn("conv1.4", t))
    t = F.conv2d(t, P["conv1.6.weight"], padding=1)
    t = F.relu(bn("bn1", t))
    for name, _, _, stride, w, stage, ds in blocks():
        res = t
        out = F.relu(bn(name + ".bn1", F.conv2d(t, P[name + ".conv1.weight"])))
        spx = torch.split(out, w, 1)
        parts = []
        sp = None
        for i in range(3):
            sp = spx[i] if (i == 0 or stage) else sp + spx[i]
            sp = F.relu(bn("%s.bns.%d" % (name, i), F.conv2d(sp, P["%s.convs.%d.weight" % (name, i)], stride=stride,
                                                              padding=1)))
            parts.append(sp)
        parts.append(F.avg_pool2d(spx[3], 3, stride, 1) if stage else spx[3])
        o = bn(name + ".bn3", F.conv2d(torch.cat(parts, 1), P[name + ".conv3.weight"]))
        y = o.mean((2, 3))
        y = torch.sigmoid(F.linear(F.relu(F.linear(y, P[name + ".se.fc.0.weight"])), P[name + ".se.fc.2.weight"]))
        o = o * y[:, :, None, None]
        if ds is not None:
            r = res if ds == 1 else F.avg_pool2d(res, ds, ds, ceil_mode=True, count_include_pad=False)
            res = bn(name + ".downsample.2", F.conv2d(r, P[name + ".downsample.1.weight"]))
        t = F.relu(o + res)
    feat = t.mean((2, 3))
    return feat, F.log_softmax(F.linear(feat, P["cls_layer.weight"], P["cls_layer.bias"]), dim=-1)
