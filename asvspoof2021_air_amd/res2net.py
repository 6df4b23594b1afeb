"""Drop-in for the reference's ``model.Res2Net`` / ``model.SEBottle2neck`` / ``model.SELayer`` /
``model.se_res2net50_v1b`` (model.py:256-509): ``--model res2net`` of main_train.py:169-170 builds
``Res2Net(SEBottle2neck, [3, 4, 6, 3], baseWidth=26, scale=4, pretrained=False, num_classes=2)``.

Same constructors, ``forward(x:(B,1,F,T)) -> (feat:(B,256), out:(B,num_classes))`` with ``out`` the log-softmax of
``cls_layer`` (model.py:353), submodules, ``state_dict`` keys and construction order (a seeded construction draws the
reference's numbers: default inits as the modules are built, then the kaiming_normal_(fan_out) / BatchNorm loop of
model.py:284-291).  The forward and backward run in HIP kernels reached through the C-ABI; this file only sequences
them:
  * every 3x3 convolution and the 1x1 layers the generic kernels refuse: the narrow-channel kernels
    (csrc/conv_narrow.hip), which read and write channel slices, so torch.split / torch.cat of the Res2 chain cost no
    copy pass; the stem's BatchNorm + ReLU run as the next convolution's prologue;
  * the 1x1 layers with Cin % 8 == 0 and Cout % 64 == 0 (conv3 of layers 3 / 4, the downsample convolutions of
    layers 2 - 4): the generic convolutions (csrc/conv2d.hip);
  * the Res2 chain step with ReLU, the stage block's 3x3 pool and the downsample's 2x2 ceil-mode pool, the SE tail
    relu(x*sigmoid(z) + residual) and log_softmax: csrc/res2net.hip; the BatchNorm, row-statistics (SE squeeze,
    global average pool) and linear kernels for the rest.
Backward: the weight gradients run on the side stream of schedule.BackwardSchedule.  There is no CPU fallback.
"""
import math

import torch
import torch.nn as nn

from . import ops
from .hip_model import HipModel
from .schedule import BackwardSchedule


class SELayer(nn.Module):
    """model.py:493-507.  Its forward runs inside Res2Net.forward (squeeze, the two Linear layers and the gate)."""

    def __init__(self, channel, reduction=16):
        super().__init__()
        self.avg_pool = nn.AdaptiveAvgPool2d(1)
        self.fc = nn.Sequential(nn.Linear(channel, channel // reduction, bias=False),
                                nn.ReLU(inplace=True),
                                nn.Linear(channel // reduction, channel, bias=False),
                                nn.Sigmoid())

    def forward(self, x):
        raise NotImplementedError("SELayer runs inside Res2Net.forward (the SE gate is fused with the block's residual "
                                  "and ReLU)")


class SEBottle2neck(nn.Module):
    """model.py:376-490."""
    expansion = 2

    def __init__(self, inplanes, planes, stride=1, downsample=None, baseWidth=26, scale=4, stype='normal'):
        super().__init__()
        width = int(math.floor(planes * (baseWidth / 64.0)))
        self.conv1 = nn.Conv2d(inplanes, width * scale, kernel_size=1, bias=False)
        self.bn1 = nn.BatchNorm2d(width * scale)
        self.nums = 1 if scale == 1 else scale - 1
        if stype == 'stage':
            self.pool = nn.AvgPool2d(kernel_size=3, stride=stride, padding=1)
        self.convs = nn.ModuleList([nn.Conv2d(width, width, kernel_size=3, stride=stride, padding=1, bias=False)
                                    for _ in range(self.nums)])
        self.bns = nn.ModuleList([nn.BatchNorm2d(width) for _ in range(self.nums)])
        self.conv3 = nn.Conv2d(width * scale, planes * self.expansion, kernel_size=1, bias=False)
        self.bn3 = nn.BatchNorm2d(planes * self.expansion)
        self.se = SELayer(planes * self.expansion, reduction=16)
        self.relu = nn.ReLU(inplace=True)
        self.downsample = downsample
        self.stype = stype
        self.scale = scale
        self.width = width

    def forward(self, x):
        raise NotImplementedError("SEBottle2neck runs inside Res2Net.forward")


def se_res2net50_v1b(**kwargs):
    """model.py:365-370: Res2Net-50_v1b_26w_4s with SE blocks."""
    return Res2Net(SEBottle2neck, [3, 4, 6, 3], baseWidth=26, scale=4, **kwargs)


def _generic_1x1(cin, cout):
    """The generic conv2d kernels take this 1x1 shape (conv2d.hip: Cin % 8 == 0, Cout % 64 == 0)."""
    return cin % 8 == 0 and cout % 64 == 0


def _v3(t):
    """(B, C, H, W) channel slice -> the (B, C, H*W) view the BatchNorm / strided-add kernels take."""
    B, C, H, W = t.shape
    return t.view(B, C, H * W)


class Res2Net(HipModel):
    TAIL = ("cls_layer.weight", "cls_layer.bias")
    BUCKET_BYTES = 256 << 10  # buckets go out as the blocks of layer4 .. layer1 finish their weight gradients

    def __init__(self, block, layers, baseWidth=26, scale=4, m=0.35, num_classes=1000, loss='softmax', **kwargs):
        self.inplanes = 16
        super().__init__()
        self.loss = loss
        self.baseWidth = baseWidth
        self.scale = scale
        self.conv1 = nn.Sequential(nn.Conv2d(1, 16, 3, 1, 1, bias=False),
                                   nn.BatchNorm2d(16), nn.ReLU(inplace=True),
                                   nn.Conv2d(16, 16, 3, 1, 1, bias=False),
                                   nn.BatchNorm2d(16), nn.ReLU(inplace=True),
                                   nn.Conv2d(16, 16, 3, 1, 1, bias=False))
        self.bn1 = nn.BatchNorm2d(16)
        self.relu = nn.ReLU()
        self.layer1 = self._make_layer(block, 16, layers[0])
        self.layer2 = self._make_layer(block, 32, layers[1], stride=2)
        self.layer3 = self._make_layer(block, 64, layers[2], stride=2)
        self.layer4 = self._make_layer(block, 128, layers[3], stride=2)
        self.avgpool = nn.AdaptiveAvgPool2d(1)
        if self.loss == 'softmax':
            self.cls_layer = nn.Linear(128 * block.expansion, num_classes)
        else:
            raise NotImplementedError
        for mod in self.modules():
            if isinstance(mod, nn.Conv2d):
                nn.init.kaiming_normal_(mod.weight, mode='fan_out', nonlinearity='relu')
            elif isinstance(mod, nn.BatchNorm2d):
                nn.init.constant_(mod.weight, 1)
                nn.init.constant_(mod.bias, 0)

    def _make_layer(self, block, planes, blocks, stride=1):
        downsample = None
        if stride != 1 or self.inplanes != planes * block.expansion:
            downsample = nn.Sequential(
                nn.AvgPool2d(kernel_size=stride, stride=stride, ceil_mode=True, count_include_pad=False),
                nn.Conv2d(self.inplanes, planes * block.expansion, kernel_size=1, stride=1, bias=False),
                nn.BatchNorm2d(planes * block.expansion),
            )
        layers = [block(self.inplanes, planes, stride, downsample=downsample, stype='stage', baseWidth=self.baseWidth,
                        scale=self.scale)]
        self.inplanes = planes * block.expansion
        for _ in range(1, blocks):
            layers.append(block(self.inplanes, planes, baseWidth=self.baseWidth, scale=self.scale))
        return nn.Sequential(*layers)

    # ------------------------------------------------------------------ plumbing
    def blocks(self):
        """(name, block) of every SEBottle2neck in forward order."""
        return [("layer%d.%d" % (li, bi), blk) for li in range(1, 5)
                for bi, blk in enumerate(getattr(self, "layer%d" % li))]

    def check_supported(self):
        """The HIP path trains SEBottle2neck blocks with scale >= 2 whose convolutions the narrow kernels (<= 256
        channels) or, for 1x1 layers, the generic kernels take."""
        for name, blk in self.blocks():
            if type(blk) is not SEBottle2neck:
                raise NotImplementedError("Res2Net HIP path: %s is a %s; only SEBottle2neck blocks have kernels" % (
                    name, type(blk).__name__))
            if blk.scale < 2:
                raise NotImplementedError("Res2Net HIP path: scale = %d; the Res2 chain needs scale >= 2" % blk.scale)
            if blk.width > 256:
                raise NotImplementedError("Res2Net HIP path: %s's 3x3 branches are %d wide (the narrow-channel "
                                          "kernels take <= 256)" % (name, blk.width))
            convs = [blk.conv1, blk.conv3] + ([blk.downsample[1]] if blk.downsample is not None else [])
            for c in convs:
                cout, cin = c.weight.shape[:2]
                if max(cin, cout) > 256 and not _generic_1x1(cin, cout):
                    raise NotImplementedError("Res2Net HIP path: %s has a 1x1 convolution %d -> %d that neither the "
                                              "narrow (<= 256 channels) nor the generic kernels take" % (name, cin, cout))
            if blk.downsample is not None:
                k = blk.downsample[0].kernel_size
                if k not in (1, 2):
                    raise NotImplementedError("Res2Net HIP path: downsample pool of kernel %s" % (k,))

    def check_input(self, x):
        if x.dim() != 4 or x.shape[1] != 1:
            raise ValueError("Res2Net expects (B, 1, F, T), got %s" % (tuple(x.shape),))
        self.check_supported()

    def extract(self, x):
        """model.py:355-374: the pooled 256-dim embedding."""
        return self.forward(x)[0]

    # ------------------------------------------------------------------ layers
    @staticmethod
    def _c1_fwd(x, w):
        cout, cin = w.shape[:2]
        if _generic_1x1(cin, cout):
            return ops.conv2d_fwd(x, w, 1, 0)
        return ops.conv_narrow_fwd(x, w, 1)

    @staticmethod
    def _c1_dgrad(dy, w, x_shape, acc=None):
        """Data gradient of a 1x1 layer, + acc (then written into acc on the narrow kernels)."""
        cout, cin = w.shape[:2]
        if _generic_1x1(cin, cout):
            return ops.conv2d_dgrad(dy, w, x_shape, 1, 0, accumulate=acc)
        if acc is not None:
            return ops.conv_narrow_dgrad(dy, w, x_shape, 1, out=acc, accumulate=True)
        return ops.conv_narrow_dgrad(dy, w, x_shape, 1)

    @staticmethod
    def _c1_wgrad(x, dy, w_shape, out):
        cout, cin = w_shape[:2]
        if _generic_1x1(cin, cout):
            return ops.conv2d_wgrad(x, dy, w_shape, 1, 0, out=out)
        return ops.conv_narrow_wgrad(x, dy, w_shape, 1, out=out)

    def _block_fwd(self, blk, x, save):
        B = x.shape[0]
        w, nums, stage = blk.width, blk.nums, blk.stype == 'stage'
        s = blk.convs[0].stride[0]
        c1 = self._c1_fwd(x, blk.conv1.weight.detach())  # model.py:452-455
        st1 = ops.bn_coeffs(c1, blk.bn1, self.training)
        out1 = ops.bn_apply(c1, st1[2], st1[3], relu=True)
        H, W = out1.shape[2], out1.shape[3]
        Ho, Wo = (H - 1) // s + 1, (W - 1) // s + 1
        cat = torch.empty((B, w * blk.scale, Ho, Wo), device=x.device, dtype=torch.float32)
        branches = []
        sp = out1[:, 0:w]
        for i in range(nums):  # model.py:458-470
            ci = ops.conv_narrow_fwd(sp, blk.convs[i].weight.detach(), s)
            sti = ops.bn_coeffs(ci, blk.bns[i], self.training)
            sci, shi = sti[2], sti[3]
            nxt = None
            if not stage and i + 1 < nums:
                nxt = torch.empty((B, w, Ho, Wo), device=x.device, dtype=torch.float32)
                ops.res2_bn_relu_apply(ci, sci, shi, cat[:, i * w:(i + 1) * w], add=out1[:, (i + 1) * w:(i + 2) * w],
                                       y2=nxt)
            else:
                ops.res2_bn_relu_apply(ci, sci, shi, cat[:, i * w:(i + 1) * w])
            branches.append((sp, ci, sti))
            sp = nxt if nxt is not None else out1[:, (i + 1) * w:(i + 2) * w]
        last, cat_last = out1[:, nums * w:], cat[:, nums * w:]
        if stage:  # model.py:473-474
            ops.avgpool2d_fwd(last, 3, s, 1, False, True, out=cat_last)
        else:
            ops.add_strided(_v3(cat_last), _v3(last))
        c3 = self._c1_fwd(cat, blk.conv3.weight.detach())
        st3 = ops.bn_coeffs(c3, blk.bn3, self.training)
        u = ops.bn_apply(c3, st3[2], st3[3])
        m, _ = ops.row_stats(_v3(u), want_std=False)  # SELayer (model.py:499-505)
        fc1, fc2 = blk.se.fc[0], blk.se.fc[2]
        h = ops.linear_fwd(m, fc1.weight.detach(), None, relu=True)
        z = ops.linear_fwd(h, fc2.weight.detach(), None)
        ds = None
        if blk.downsample is not None:  # model.py:482-483
            k = blk.downsample[0].kernel_size
            xp = x if k == 1 else ops.avgpool2d_fwd(x, k, k, 0, True, False)
            cd = self._c1_fwd(xp, blk.downsample[1].weight.detach())
            std_ = ops.bn_coeffs(cd, blk.downsample[2], self.training)
            r = ops.bn_apply(cd, std_[2], std_[3])
            ds = (k, xp, cd, std_)
        else:
            r = x
        o = ops.se_relu_fwd(u, z, r)  # model.py:485-488
        S = None
        if save:
            S = dict(x=x, c1=c1, st1=st1, out1=out1, branches=branches, cat=cat, c3=c3, st3=st3, u=u, m=m, h=h, z=z,
                     ds=ds, o=o)
        return o, S

    def _forward_impl(self, x, save):
        if save and not self.training:
            raise NotImplementedError("backward through eval-mode BatchNorm is not on the hot path")
        S = {"x": x, "blocks": []} if save else None
        c = self.conv1
        # stem (model.py:261-266, :326-329): each BatchNorm + ReLU is the next convolution's prologue
        a0 = ops.conv_narrow_fwd(x, c[0].weight.detach(), 1)
        st0 = ops.bn_coeffs(a0, c[1], self.training)
        a1 = ops.conv_narrow_fwd(a0, c[3].weight.detach(), 1, in_scale=st0[2], in_shift=st0[3], relu=True)
        st1 = ops.bn_coeffs(a1, c[4], self.training)
        a2 = ops.conv_narrow_fwd(a1, c[6].weight.detach(), 1, in_scale=st1[2], in_shift=st1[3], relu=True)
        st2 = ops.bn_coeffs(a2, self.bn1, self.training)
        cur = ops.bn_apply(a2, st2[2], st2[3], relu=True)
        if save:
            S.update(a0=a0, a1=a1, a2=a2, stem=(st0, st1, st2))
        for name, blk in self.blocks():
            cur, bs = self._block_fwd(blk, cur, save)
            if save:
                S["blocks"].append((name, blk, bs))
        feat, _ = ops.row_stats(_v3(cur), want_std=False)  # AdaptiveAvgPool2d(1) + flatten (model.py:345-349)
        logits = ops.linear_fwd(feat, self.cls_layer.weight.detach(), self.cls_layer.bias.detach())
        out = ops.log_softmax_fwd(logits)  # model.py:352-353
        if save:
            S.update(top=cur, feat=feat, out=out)
        ops.bn_flush()
        return feat, out, S

    # ----------------------------------------------------------------- backward
    def _block_bwd(self, blk, name, S, do, sch):
        gv = sch.grad
        w, nums, stage = blk.width, blk.nums, blk.stype == 'stage'
        s = blk.convs[0].stride[0]
        x, u, z, o = S["x"], S["u"], S["z"], S["o"]
        du, dz, dres = ops.se_relu_bwd(u, z, o, do)
        fc1, fc2 = blk.se.fc[0], blk.se.fc[2]
        dh, _, _ = ops.linear_bwd(S["h"], fc2.weight.detach(), dz, True, dw=gv(name + ".se.fc.2.weight"),
                                  need_db=False)
        ops.relu_mask_(dh, S["h"])
        dm, _, _ = ops.linear_bwd(S["m"], fc1.weight.detach(), dh, True, dw=gv(name + ".se.fc.0.weight"),
                                  need_db=False)
        c3, st3 = S["c3"], S["st3"]
        Sp = c3.shape[2] * c3.shape[3]
        dc3, _, _ = ops.bn_bwd(c3, du, st3[0], st3[1], blk.bn3.weight.detach(), blk.bn3.bias.detach(),
                               dgamma=gv(name + ".bn3.weight"), dbeta=gv(name + ".bn3.bias"), rowbias=dm,
                               rowbias_scale=1.0 / Sp)
        cat = S["cat"]
        w3 = blk.conv3.weight.detach()
        g3 = gv(name + ".conv3.weight")
        sch.on_side(lambda: self._c1_wgrad(cat, dc3, w3.shape, g3), cat, dc3)
        dcat = self._c1_dgrad(dc3, w3, cat.shape)
        out1 = S["out1"]
        dout1 = torch.empty_like(out1)
        if stage:
            ops.avgpool2d_bwd(dcat[:, nums * w:], out1[:, nums * w:].shape, 3, s, 1, False, True,
                              out=dout1[:, nums * w:])
        else:
            ops.add_strided(_v3(dout1[:, nums * w:]), _v3(dcat[:, nums * w:]))
        for i in reversed(range(nums)):
            sp, ci, sti = S["branches"][i]
            dy2 = _v3(dout1[:, (i + 1) * w:(i + 2) * w]) if (not stage and i + 1 < nums) else None
            bn = blk.bns[i]
            dci, _, _ = ops.bn_bwd(ci, _v3(dcat[:, i * w:(i + 1) * w]), sti[0], sti[1], bn.weight.detach(),
                                   bn.bias.detach(), relu=True, dgamma=gv("%s.bns.%d.weight" % (name, i)),
                                   dbeta=gv("%s.bns.%d.bias" % (name, i)), dy2=dy2)
            wi = blk.convs[i].weight.detach()
            gwi = gv("%s.convs.%d.weight" % (name, i))
            sch.on_side(lambda sp=sp, dci=dci, wi=wi, gwi=gwi: ops.conv_narrow_wgrad(sp, dci, wi.shape, s, out=gwi),
                        sp, dci)
            ops.conv_narrow_dgrad(dci, wi, sp.shape, s, out=dout1[:, i * w:(i + 1) * w])
        c1, st1 = S["c1"], S["st1"]
        dc1, _, _ = ops.bn_bwd(c1, dout1, st1[0], st1[1], blk.bn1.weight.detach(), blk.bn1.bias.detach(), relu=True,
                               dgamma=gv(name + ".bn1.weight"), dbeta=gv(name + ".bn1.bias"))
        w1 = blk.conv1.weight.detach()
        g1 = gv(name + ".conv1.weight")
        sch.on_side(lambda: self._c1_wgrad(x, dc1, w1.shape, g1), x, dc1)
        if S["ds"] is None:
            dx = self._c1_dgrad(dc1, w1, x.shape, acc=dres)
        else:
            k, xp, cd, std_ = S["ds"]
            bnd = blk.downsample[2]
            dcd, _, _ = ops.bn_bwd(cd, dres, std_[0], std_[1], bnd.weight.detach(), bnd.bias.detach(),
                                   dgamma=gv(name + ".downsample.2.weight"), dbeta=gv(name + ".downsample.2.bias"))
            wd = blk.downsample[1].weight.detach()
            gd = gv(name + ".downsample.1.weight")
            sch.on_side(lambda: self._c1_wgrad(xp, dcd, wd.shape, gd), xp, dcd)
            if k == 1:
                dx = self._c1_dgrad(dcd, wd, x.shape)
            else:
                dx = ops.avgpool2d_bwd(self._c1_dgrad(dcd, wd, xp.shape), x.shape, k, k, 0, True, False)
            dx = self._c1_dgrad(dc1, w1, x.shape, acc=dx)
        return dx

    def _backward_impl(self, S, dfeat, dout):
        arena = self.arena()
        sch = BackwardSchedule(self, arena, self.overlap_wgrad, self._bucketer, side_when_accumulating=True)
        gv = sch.grad
        feat = S["feat"]
        if dout is not None:  # CE / base-loss branch (main_train.py:355): log_softmax, then cls_layer
            dlog = ops.log_softmax_bwd(S["out"], dout.contiguous())
            dfc, _, _ = ops.linear_bwd(feat, self.cls_layer.weight.detach(), dlog, True,
                                       dw=gv("cls_layer.weight"), db=gv("cls_layer.bias"))
            dfeat = dfc if dfeat is None else ops.add_(dfc, dfeat.contiguous())
        if dfeat is None:
            dfeat = torch.zeros_like(feat)
        dfeat = dfeat.contiguous()
        top = S["top"]
        dtop = torch.empty_like(top)
        ops.row_stats_bwd(_v3(top), feat, None, dfeat, None, _v3(dtop), accumulate=False)
        d = dtop
        for name, blk, bs in reversed(S["blocks"]):
            d = self._block_bwd(blk, name, bs, d, sch)
            sch.grads_final_from(name + ".conv1.weight")
        # stem
        c = self.conv1
        st0, st1, st2 = S["stem"]  # (mean, invstd, scale, shift) each
        (s0, h0), (s1, h1) = st0[2:], st1[2:]
        x, a0, a1, a2 = S["x"], S["a0"], S["a1"], S["a2"]
        da2, _, _ = ops.bn_bwd(a2, d, st2[0], st2[1], self.bn1.weight.detach(), self.bn1.bias.detach(), relu=True,
                               dgamma=gv("bn1.weight"), dbeta=gv("bn1.bias"))
        w2, g2 = c[6].weight.detach(), gv("conv1.6.weight")
        sch.on_side(lambda: ops.conv_narrow_wgrad(a1, da2, w2.shape, 1, in_scale=s1, in_shift=h1, relu=True, out=g2),
                    a1, da2, s1, h1)
        dact1 = ops.conv_narrow_dgrad(da2, w2, a1.shape, 1)
        da1, _, _ = ops.bn_bwd(a1, dact1, st1[0], st1[1], c[4].weight.detach(), c[4].bias.detach(), relu=True,
                               dgamma=gv("conv1.4.weight"), dbeta=gv("conv1.4.bias"))
        w1, g1 = c[3].weight.detach(), gv("conv1.3.weight")
        sch.on_side(lambda: ops.conv_narrow_wgrad(a0, da1, w1.shape, 1, in_scale=s0, in_shift=h0, relu=True, out=g1),
                    a0, da1, s0, h0)
        dact0 = ops.conv_narrow_dgrad(da1, w1, a0.shape, 1)
        da0, _, _ = ops.bn_bwd(a0, dact0, st0[0], st0[1], c[1].weight.detach(), c[1].bias.detach(), relu=True,
                               dgamma=gv("conv1.1.weight"), dbeta=gv("conv1.1.bias"))
        w0, g0 = c[0].weight.detach(), gv("conv1.0.weight")
        sch.on_side(lambda: ops.conv_narrow_wgrad(x, da0, w0.shape, 1, out=g0), x, da0)
        return sch.finish()
