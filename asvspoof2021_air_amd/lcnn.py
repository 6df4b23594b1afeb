"""Drop-in for the reference's ``model.LCNN`` / ``model.MaxFeatureMap2D`` (model.py:511-610), the default ``--model``
of main_train.py:49-50.

Same constructor, ``forward(x:(B,1,60,750)) -> (feat:(B,enc_dim), out:(B,nclasses))``, submodules, ``state_dict`` keys
and construction order (a seeded construction draws the reference's numbers).  The forward and backward run in HIP
kernels reached through the C-ABI; this file only sequences them:
  * conv1 (5x5, 1 -> 64) + bias + MFM + 2x2 max-pool: one fused kernel (csrc/lcnn.hip) that writes the pooled map
    and a route byte per output, never the 64-channel map;
  * conv2 .. conv9: the generic convolutions (csrc/conv2d.hip, bias-free), then one MFM (+ pool) pass that adds the
    bias on the way in and writes the route bytes; conv3 / conv4's 96 outputs run on weights zero-padded to 128 rows
    (the generic kernels tile 64 output channels);
  * BatchNorm2d(affine=False): the BatchNorm kernels with unit scale and zero shift;
  * Dropout(0.7): a keep-mask drawn on the device from a Philox counter that the draw advances (graph replays draw
    fresh masks); Linear / MFM / Linear / fc_mu on the linear and MFM kernels.
Backward: the route bytes send each post-MFM / post-pool gradient to its winner (zeros elsewhere) and give the conv
bias gradients; the weight gradients run on the side stream of schedule.BackwardSchedule.
"""
import torch
import torch.nn as nn

from . import _hip, ops
from .hip_model import HipModel
from .schedule import BackwardSchedule

# (name, Cin, Cout, kernel, padding, max-pool, BatchNorm) of conv2 .. conv9 (model.py:531-563)
LAYERS = (("conv2", 32, 64, 1, 0, False, True),
          ("conv3", 32, 96, 3, 1, True, True),
          ("conv4", 48, 96, 1, 0, False, True),
          ("conv5", 48, 128, 3, 1, True, False),
          ("conv6", 64, 128, 1, 0, False, True),
          ("conv7", 64, 64, 3, 1, False, True),
          ("conv8", 32, 64, 1, 0, False, True),
          ("conv9", 32, 64, 3, 1, True, False))
DROPOUT_P = 0.7


def _padded_cout(cout):
    return (cout + 63) // 64 * 64


class MaxFeatureMap2D(nn.Module):
    """model.py:512-545: the larger of channel c and c + C/2 (``view(B, 2, C/2, ...).max(1)``).  Forward only (the
    LCNN's training path runs through LCNN.forward); dims other than 1 are not on any reference path."""

    def __init__(self, max_dim=1):
        super().__init__()
        self.max_dim = max_dim

    def forward(self, inputs):
        if not inputs.is_cuda:
            raise _hip.AirError("MaxFeatureMap2D HIP path needs a GPU tensor; there is no CPU fallback")
        if self.max_dim != 1:
            raise NotImplementedError("MaxFeatureMap2D: only max_dim=1 (the channel axis) has a kernel")
        if inputs.shape[1] % 2:
            raise ValueError("MaxFeatureMap2D: channel dimension %d is odd" % inputs.shape[1])
        if torch.is_grad_enabled() and inputs.requires_grad:
            raise NotImplementedError("MaxFeatureMap2D.forward is forward-only (use torch.no_grad()); gradients flow "
                                      "through LCNN.forward")
        x = inputs.float().contiguous()
        shp = x.shape
        x4 = x.view(shp[0], shp[1], -1, 1)
        y, _ = ops.mfm_pool_fwd(x4)
        return y.view((shp[0], shp[1] // 2) + tuple(shp[2:]))


class LCNN(HipModel):
    TAIL = ("fc_mu.weight", "fc_mu.bias")
    # 3.5 MB of gradients (2.8 MB of them out.1): 256 KB buckets send out.1 + out.3, conv9 .. conv6 and conv5 .. conv3
    # from inside backward; the default 16 MB bucket would leave the whole exchange behind it
    BUCKET_BYTES = 256 << 10
    # the offset of the mask's Philox stream as a device-side counter (HipModel.device_counter)
    _mask_ctr = None
    _mask_ctrs = None

    def __init__(self, num_nodes, enc_dim, nclasses=2):
        super().__init__()
        self.num_nodes = num_nodes
        self.enc_dim = enc_dim
        self.nclasses = nclasses
        self.conv1 = nn.Sequential(nn.Conv2d(1, 64, (5, 5), 1, padding=(2, 2)),
                                   MaxFeatureMap2D(),
                                   nn.MaxPool2d((2, 2), (2, 2)))
        for name, cin, cout, k, pad, pool, bn in LAYERS:
            mods = [nn.Conv2d(cin, cout, (k, k), 1, padding=(pad, pad)), MaxFeatureMap2D()]
            if pool:
                mods.append(nn.MaxPool2d((2, 2), (2, 2)))
            if bn:
                mods.append(nn.BatchNorm2d(cout // 2, affine=False))
            setattr(self, name, nn.Sequential(*mods))
        self.out = nn.Sequential(nn.Dropout(DROPOUT_P),
                                 nn.Linear((750 // 16) * (num_nodes // 16) * 32, 160),
                                 MaxFeatureMap2D(),
                                 nn.Linear(80, self.enc_dim))
        self.fc_mu = nn.Linear(enc_dim, nclasses) if nclasses >= 2 else nn.Linear(enc_dim, 1)
        # dropout keep-mask: 'device' = Philox draw with a device-side offset, or 'tensor' = a mask installed with
        # set_dropout_mask() (parity tests replay the reference's draw; train.Trainer then steps eagerly)
        self.noise_mode = "device"
        self._mask_tensor = None
        self._mask_seed = int(torch.initial_seed()) & 0x7FFFFFFFFFFFFFFF
        self._mask_offset = 0
        self._unit = {}   # device -> (ones, zeros) of 64: the affine=False BatchNorms' scale and shift
        self._wpad = {}   # layer name -> weight zero-padded to a multiple of 64 rows (conv3, conv4)

    def __getstate__(self):
        """Also runtime state: the unit coefficients, the padded weights and an installed mask."""
        st = super().__getstate__()
        st["_unit"], st["_wpad"] = {}, {}
        st["_mask_tensor"] = None
        self.fold_counter(st, "_mask")
        if st.get("noise_mode") == "tensor":
            st["noise_mode"] = "device"
        return st

    # ------------------------------------------------------------------ plumbing
    def set_dropout_mask(self, mask):
        """Install the (B, 4416) scaled keep-mask nn.Dropout(0.7) would draw (values 0 and 1 / 0.3), or None to go
        back to the device draw."""
        self._mask_tensor = mask
        self.noise_mode = "tensor" if mask is not None else "device"

    def _draw_mask(self, B, N, device):
        if self.noise_mode == "tensor":
            m = self._mask_tensor
            if tuple(m.shape) != (B, N):
                raise _hip.AirError("dropout mask must be (B, %d), got %s" % (N, tuple(m.shape)))
            return m.to(device=device, dtype=torch.float32).contiguous()
        ctr = self.device_counter("_mask", device)
        return ops.dropout_mask_ctr((B, N), DROPOUT_P, self._mask_seed, ctr, device)

    def _units(self, device):
        u = self._unit.get(device)
        if u is None:
            u = self._unit[device] = (torch.ones(64, device=device), torch.zeros(64, device=device))
        return u

    def _weight(self, name):
        """The layer's conv weight as the generic kernels take it: rows zero-padded to a multiple of 64."""
        conv = getattr(self, name)[0]
        w = conv.weight.detach()
        cout = w.shape[0]
        cp = _padded_cout(cout)
        if cp == cout:
            return w
        buf = self._wpad.get(name)
        if buf is None or buf.device != w.device:
            buf = self._wpad[name] = torch.empty((cp,) + tuple(w.shape[1:]), device=w.device, dtype=torch.float32)
        return ops.copy_pad(buf, w)

    def check_input(self, x):
        if x.dim() != 4 or x.shape[1] != 1:
            raise ValueError("LCNN expects (B, 1, F, T), got %s" % (tuple(x.shape),))
        H, W = x.shape[2], x.shape[3]
        want = self.out[1].in_features
        got = (W // 16) * (H // 16) * 32
        if got != want:
            raise ValueError("LCNN: input (F=%d, T=%d) pools to %d x %d x 32 = %d features; out.1 = Linear(%d, 160) "
                             "needs T // 16 = %d and F // 16 = %d (model.py:601)" % (
                                 H, W, H // 16, W // 16, got, want, 750 // 16, self.num_nodes // 16))

    # ------------------------------------------------------------------ forward
    def _forward_impl(self, x, save):
        training = self.training
        dev = x.device
        ones, zeros = self._units(dev)
        S = {"x": x, "layers": []} if save else None
        c1 = self.conv1[0]
        cur, r1 = ops.lcnn_conv1_fwd(x, c1.weight.detach(), c1.bias.detach())  # model.py:528-530, :577
        if save:
            S["r1"] = r1
        for name, cin, cout, k, pad, pool, bn in LAYERS:
            seq = getattr(self, name)
            w = self._weight(name)
            pre = ops.conv2d_fwd(cur, w, 1, pad)
            m, route = ops.mfm_pool_fwd(pre, C=cout, bias=seq[0].bias.detach(), pool=pool)
            st, a = None, m
            if bn:
                C = cout // 2
                st = ops.bn_coeffs(m, seq[-1], training, affine=(ones[:C], zeros[:C]))
                a = ops.bn_apply(m, st[2], st[3])
            if save:
                S["layers"].append((name, cur, w, pre.shape, pool, route, m, st))
            cur = a
        B = x.shape[0]
        flat = cur.view(B, -1)  # model.py:586
        if training:
            keep = self._draw_mask(B, flat.shape[1], dev)
            drop = ops.mul(flat, keep)
        else:
            keep, drop = None, flat
        l1, l3 = self.out[1], self.out[3]
        h160 = ops.linear_fwd(drop, l1.weight.detach(), l1.bias.detach())
        h80, rh = ops.mfm_pool_fwd(h160.view(B, 160, 1, 1))
        h80 = h80.view(B, 80)
        feat = ops.linear_fwd(h80, l3.weight.detach(), l3.bias.detach())
        out = ops.linear_fwd(feat, self.fc_mu.weight.detach(), self.fc_mu.bias.detach())
        if save:
            if not training:
                raise NotImplementedError("backward through eval-mode BatchNorm is not on the hot path")
            S.update(a9=cur, keep=keep, drop=drop, h160_shape=h160.shape, rh=rh, h80=h80, feat=feat)
        ops.bn_flush()
        return feat, out, S

    # ----------------------------------------------------------------- backward
    def _backward_impl(self, S, dfeat, dout):
        arena = self.arena()
        sch = BackwardSchedule(self, arena, self.overlap_wgrad, self._bucketer, side_when_accumulating=True)
        gv = sch.grad
        dev = S["x"].device
        ones, zeros = self._units(dev)
        if dout is not None:  # CE / base-loss branch (main_train.py:355); dead under ang_iso
            dx_mu, _, _ = ops.linear_bwd(S["feat"], self.fc_mu.weight.detach(), dout.contiguous(), True,
                                         dw=gv("fc_mu.weight"), db=gv("fc_mu.bias"))
            dfeat = dx_mu if dfeat is None else ops.add_(dx_mu, dfeat.contiguous())
        if dfeat is None:
            dfeat = torch.zeros_like(S["feat"])
        dfeat = dfeat.contiguous()
        l1, l3 = self.out[1], self.out[3]
        B = dfeat.shape[0]
        dh80, _, _ = ops.linear_bwd(S["h80"], l3.weight.detach(), dfeat, True, dw=gv("out.3.weight"), db=gv("out.3.bias"))
        dh160 = ops.mfm_pool_bwd(dh80.view(B, 80, 1, 1), S["rh"], (B, 160, 1, 1)).view(B, 160)
        ddrop, _, _ = ops.linear_bwd(S["drop"], l1.weight.detach(), dh160, True, dw=gv("out.1.weight"),
                                     db=gv("out.1.bias"))
        sch.grads_final_from("out.1.weight")
        da = ops.mul(ddrop, S["keep"]).view(S["a9"].shape)
        for name, xin, w, pre_shape, pool, route, m, st in reversed(S["layers"]):
            conv = getattr(self, name)[0]
            cout = conv.weight.shape[0]
            if st is not None:  # BatchNorm2d(affine=False) backward: unit gamma, zero beta
                C = cout // 2
                dm, _, _ = ops.bn_bwd(m, da, st[0], st[1], ones[:C], zeros[:C])
            else:
                dm = da
            dpre = ops.mfm_pool_bwd(dm, route, pre_shape, C=cout, pool=pool)
            ops.mfm_bias_grad(dm, route, out=gv(name + ".0.bias"))
            gw = gv(name + ".0.weight")
            pad = conv.padding

            def wg(xin=xin, dpre=dpre, w=w, gw=gw, pad=pad):
                if w.shape[0] == gw.shape[0]:
                    ops.conv2d_wgrad(xin, dpre, w.shape, 1, pad, out=gw)
                else:  # zero-padded rows: the gradient of the real rows is the leading part of the padded one
                    ops.copy_pad(gw, ops.conv2d_wgrad(xin, dpre, w.shape, 1, pad))

            sch.on_side(wg, xin, dpre, w)
            da = ops.conv2d_dgrad(dpre, w, xin.shape, 1, pad)
            sch.grads_final_from(name + ".0.weight")
        c1 = self.conv1[0]
        x, r1 = S["x"], S["r1"]
        gw1, gb1 = gv("conv1.0.weight"), gv("conv1.0.bias")
        sch.on_side(lambda: ops.lcnn_conv1_wgrad(x, da, r1, gw1, gb1), x, da, r1)
        return sch.finish()
