"""Tensor-level wrappers over the C-ABI (include/air_hip.h).

Each function takes contiguous fp32 GPU tensors, allocates outputs with torch
(device memory is plumbing) and launches the HIP kernels on the current
stream.  Nothing here computes on the CPU or through ATen.
"""
import ctypes

import torch

from . import _hip
from ._hip import AirConv1d, AirConv2d, AirConvNarrow, ci, cf, csz, dptr, stream

_WS = {}
_WS_GEN = [0]     # bumped whenever a scratch buffer is (re)allocated
_WS_PINNED = {}   # capture owner -> buffers its hipGraph may still point into (kept alive until the capture is dropped)


def workspace_generation():
    """Changes whenever workspace() replaced a buffer.  A captured hipGraph holds raw pointers into the buffers
    that existed at capture time (train.Trainer compares this before every replay and re-captures)."""
    return _WS_GEN[0]


def pin_workspaces(owner=None):
    """Called when a hipGraph has been captured: from now on a buffer that is outgrown is kept alive instead of
    freed, so a replay can never write through a dangling scratch pointer - until ``unpin_workspaces(owner)``."""
    held = _WS_PINNED.setdefault(owner, [])
    for buf in _WS.values():
        if not any(buf is b for b in held):
            held.append(buf)


def unpin_workspaces(owner=None):
    """The capture that pinned the buffers is gone: release what was only kept alive for its replays."""
    _WS_PINNED.pop(owner, None)


def workspace(nbytes, device):
    """One growing scratch buffer per (device, stream): ops run back to back on a stream, and
    the weight-gradient side stream (resnet.py) must not share scratch with the main one."""
    cur = _hip._RAW_DEVICE() if _hip._RAW_DEVICE is not None else torch.cuda.current_device()
    key = (device.type, device.index,
           _hip.raw_stream() if device.index in (None, cur) else torch.cuda.current_stream(device).cuda_stream)
    buf = _WS.get(key)
    if buf is None or buf.numel() < nbytes:
        buf = torch.empty(max(int(nbytes), 1 << 20), dtype=torch.uint8, device=device)
        _WS[key] = buf
        _WS_GEN[0] += 1
    return buf


def _conv_desc(x_shape, w_shape, stride, padding):
    B, Cin, H, W = x_shape
    Cout, Cin2, KH, KW = w_shape
    if Cin2 != Cin:
        raise _hip.AirError("conv2d: weight expects %d input channels, got %d" % (Cin2, Cin))
    sh, sw = (stride, stride) if isinstance(stride, int) else stride
    ph, pw = (padding, padding) if isinstance(padding, int) else padding
    Ho = (H + 2 * ph - KH) // sh + 1
    Wo = (W + 2 * pw - KW) // sw + 1
    return AirConv2d(B, Cin, H, W, Cout, KH, KW, sh, sw, ph, pw, Ho, Wo)


def _conv_ws(desc, device):
    lib = _hip.lib()
    n = lib.air_conv2d_ws_bytes(ctypes.byref(desc))
    if n == 0:
        raise _hip.AirError("conv2d: unsupported configuration %s" %
                            ([getattr(desc, f[0]) for f in desc._fields_],))
    return workspace(n, device), n


def conv2d_prepack(w, x_shape, stride, padding, which, out=None):
    """Transformed (Winograd) weights of a 3x3 / stride 1 / pad 1 layer for ``which`` (0 forward, 1 dgrad) into a
    buffer the later conv2d_fwd / conv2d_dgrad call takes as ``w_packed``; None when the layer has no such form.
    Runs on the current stream: call it under a side stream and order it with events."""
    d = _conv_desc(x_shape, w.shape, stride, padding)
    n = int(_hip.lib().air_conv2d_prepack_bytes(ctypes.byref(d), ci(which)))
    if n == 0:
        return None
    if out is None or out.numel() < n:
        out = torch.empty(n, dtype=torch.uint8, device=w.device)
    _hip.check(_hip.lib().air_conv2d_prepack(ctypes.byref(d), dptr(w), ci(which), dptr(out, torch.uint8), csz(n),
                                             stream()), "air_conv2d_prepack")
    out._air_pack_layout = int(_hip.lib().air_conv2d_prepack_layout(ctypes.byref(d), ci(which)))
    return out


class prepack_batch:
    """``with ops.prepack_batch():`` the conv2d_prepack / conv2d_dgrad_s2_pair_prepack calls inside only record their
    transforms; leaving the block runs them on the current stream as one launch per 32 (air_conv2d_prepack_begin /
    _flush).  The buffers are valid behind the block in stream order."""

    def __enter__(self):
        _hip.check(_hip.lib().air_conv2d_prepack_begin(), "air_conv2d_prepack_begin")
        return self

    def __exit__(self, *exc):
        _hip.check(_hip.lib().air_conv2d_prepack_flush(stream()), "air_conv2d_prepack_flush")
        return False


def _check_packed(d, w_packed, which):
    """A prepacked weight buffer must be at least what the layer consumes under the CURRENT dispatch options
    (options can change between prepack and use; the library walks the buffer without a size)."""
    if w_packed is not None:
        #  the layouts differ in element type, not only in size: the tag conv2d_prepack left on the buffer
        # must be what the layer consumes now (f32 slabs / Winograd F2 / split-bf16 planes / Winograd F4)
        have = getattr(w_packed, "_air_pack_layout", None)
        now = int(_hip.lib().air_conv2d_prepack_layout(ctypes.byref(d), ci(which)))
        if have is not None and have != now:
            raise _hip.AirError("conv2d: w_packed was written in layout %d, the layer consumes layout %d under the current "
                                "dispatch options (prepack again after air_set_option)" % (have, now))
        need = int(_hip.lib().air_conv2d_prepack_bytes(ctypes.byref(d), ci(which)))
        if w_packed.numel() * w_packed.element_size() < need:
            raise _hip.AirError("conv2d: w_packed holds %d bytes, the layer consumes %d under the current dispatch "
                                "options (prepack again after air_set_option)" % (
                                    w_packed.numel() * w_packed.element_size(), need))


def conv2d_fwd(x, w, stride=1, padding=0, in_scale=None, in_shift=None, relu=False, residual=None, w_packed=None,
               stats=False):
    """y = conv2d(act(x), w) (+ residual); act = optional per-channel affine + ReLU.
    stats=True: returns (y, records) - BatchNorm statistics records of y from the convolution's epilogue for
    ``bn_stats(..., stats_in=records)``, or (y, None) when this layer has no fused statistics (the caller's BatchNorm
    then makes its own pass over y)."""
    d = _conv_desc(x.shape, w.shape, stride, padding)
    _check_packed(d, w_packed, 0)
    y = torch.empty((d.B, d.Cout, d.Ho, d.Wo), device=x.device, dtype=torch.float32)
    ws, n = _conv_ws(d, x.device)
    rec = None
    if stats and in_scale is None:
        nb = int(_hip.lib().air_conv2d_fwd_stats_bytes(ctypes.byref(d)))
        if nb > 0:
            rec = torch.empty(nb, dtype=torch.uint8, device=x.device)
    _hip.check(_hip.lib().air_conv2d_fwd_pre(
        ctypes.byref(d), dptr(x), dptr(w), dptr(w_packed, torch.uint8, allow_none=True), dptr(y),
        dptr(in_scale, allow_none=True),
        dptr(in_shift, allow_none=True), ci(1 if relu else 0), dptr(residual, allow_none=True),
        dptr(rec, torch.uint8, allow_none=True), dptr(ws, torch.uint8), csz(n), stream()), "air_conv2d_fwd_pre")
    return (y, rec) if stats else y


def conv2d_dgrad(dy, w, x_shape, stride=1, padding=0, accumulate=None, out=None, w_packed=None, bn=None):
    """dx = the data gradient of conv2d (+ accumulate).  bn = (bn_x, mean, invstd, gamma, beta): dx is the gradient
    with respect to the output of relu(batchnorm(bn_x)); returns (dx, sums) with ``sums`` the BatchNorm-backward
    records for ``bn_bwd(..., sums_in=sums)`` taken by the epilogue, or (dx, None) when this layer has no such form."""
    d = _conv_desc(x_shape, w.shape, stride, padding)
    _check_packed(d, w_packed, 1)
    dx = out if out is not None else torch.empty(tuple(x_shape), device=dy.device, dtype=torch.float32)
    ws, n = _conv_ws(d, dy.device)
    if bn is not None:
        nb = int(_hip.lib().air_conv2d_dgrad_bn_sums_bytes(ctypes.byref(d)))
        if nb > 0:
            bx, mean, invstd, gamma, beta = bn
            if tuple(bx.shape) != tuple(x_shape):
                raise _hip.AirError("conv2d_dgrad: bn_x must have dx's shape")
            sums = torch.empty(nb, dtype=torch.uint8, device=dy.device)
            _hip.check(_hip.lib().air_conv2d_dgrad_bn(
                ctypes.byref(d), dptr(dy), dptr(w), dptr(w_packed, torch.uint8, allow_none=True), dptr(dx),
                dptr(accumulate, allow_none=True), dptr(bx), dptr(mean), dptr(invstd), dptr(gamma), dptr(beta),
                dptr(sums, torch.uint8), dptr(ws, torch.uint8), csz(n), stream()), "air_conv2d_dgrad_bn")
            return dx, sums
    _hip.check(_hip.lib().air_conv2d_dgrad_pre(
        ctypes.byref(d), dptr(dy), dptr(w), dptr(w_packed, torch.uint8, allow_none=True), dptr(dx),
        dptr(accumulate, allow_none=True),
        dptr(ws, torch.uint8), csz(n), stream()), "air_conv2d_dgrad_pre")
    return (dx, None) if bn is not None else dx


def conv2d_dgrad_s2_pair_ok(w_shape, x_shape):
    """Whether a 3x3 / stride 2 / pad 1 convolution and the 1x1 / stride 2 shortcut beside it have the one-pass data
    gradient under the current dispatch options."""
    d = _conv_desc(x_shape, w_shape, 2, 1)
    return int(_hip.lib().air_conv2d_dgrad_s2_pair_prepack_bytes(ctypes.byref(d))) > 0


def conv2d_dgrad_s2_pair_prepack(w, w_sc, x_shape, out=None):
    """Both weights of a PreActBlock's stride-2 pair (3x3 conv1, 1x1 shortcut) in the layout conv2d_dgrad_s2_pair
    consumes; None when the pair has no one-pass data gradient under the current dispatch options."""
    d = _conv_desc(x_shape, w.shape, 2, 1)
    n = int(_hip.lib().air_conv2d_dgrad_s2_pair_prepack_bytes(ctypes.byref(d)))
    if n == 0:
        return None
    if out is None or out.numel() < n:
        out = torch.empty(n, dtype=torch.uint8, device=w.device)
    _hip.check(_hip.lib().air_conv2d_dgrad_s2_pair_prepack(ctypes.byref(d), dptr(w), dptr(w_sc), dptr(out, torch.uint8),
                                                           csz(n), stream()), "air_conv2d_dgrad_s2_pair_prepack")
    return out


def conv2d_dgrad_s2_pair(dy, w, dy_sc, w_sc, x_shape, accumulate=None, out=None, packed=None):
    """dx = dgrad(3x3 / stride 2 / pad 1 conv; dy, w) + dgrad(1x1 / stride 2 shortcut; dy_sc, w_sc) (+ accumulate) in one
    pass over the two output gradients (resnet.py:56-66).  Returns None when the pair has no such form under the current
    dispatch options (the caller then runs the two data gradients one after the other)."""
    d = _conv_desc(x_shape, w.shape, 2, 1)
    if tuple(w_sc.shape) != (w.shape[0], w.shape[1], 1, 1) or tuple(dy_sc.shape) != tuple(dy.shape):
        raise _hip.AirError("conv2d_dgrad_s2_pair: the shortcut must be the 1x1 / stride 2 convolution beside the 3x3 one")
    n = int(_hip.lib().air_conv2d_dgrad_s2_pair_prepack_bytes(ctypes.byref(d)))
    if n == 0:
        return None
    if packed is not None and packed.numel() * packed.element_size() < n:
        raise _hip.AirError("conv2d_dgrad_s2_pair: packed holds %d bytes, the pair consumes %d under the current "
                            "dispatch options" % (packed.numel() * packed.element_size(), n))
    dx = out if out is not None else torch.empty(tuple(x_shape), device=dy.device, dtype=torch.float32)
    ws = workspace(n, dy.device) if packed is None else None
    _hip.check(_hip.lib().air_conv2d_dgrad_s2_pair(
        ctypes.byref(d), dptr(dy), dptr(w), dptr(dy_sc), dptr(w_sc), dptr(packed, torch.uint8, allow_none=True), dptr(dx),
        dptr(accumulate, allow_none=True), dptr(ws, torch.uint8, allow_none=True), csz(n if packed is None else 0),
        stream()), "air_conv2d_dgrad_s2_pair")
    return dx


def conv2d_fwd_s2_pair_ok(w_shape, x_shape):
    """Whether a 3x3 / stride 2 / pad 1 convolution and the 1x1 / stride 2 shortcut on the same input have the one-launch
    forward under the current dispatch options."""
    d = _conv_desc(x_shape, w_shape, 2, 1)
    return int(_hip.lib().air_conv2d_fwd_s2_pair_prepack_bytes(ctypes.byref(d))) > 0


def conv2d_fwd_s2_pair_prepack(w, w_sc, x_shape, out=None):
    """Both weights of a PreActBlock's stride-2 pair in the layout conv2d_fwd_s2_pair consumes; None when the pair has
    no one-launch forward under the current dispatch options."""
    d = _conv_desc(x_shape, w.shape, 2, 1)
    n = int(_hip.lib().air_conv2d_fwd_s2_pair_prepack_bytes(ctypes.byref(d)))
    if n == 0:
        return None
    if out is None or out.numel() < n:
        out = torch.empty(n, dtype=torch.uint8, device=w.device)
    _hip.check(_hip.lib().air_conv2d_fwd_s2_pair_prepack(ctypes.byref(d), dptr(w), dptr(w_sc), dptr(out, torch.uint8),
                                                         csz(n), stream()), "air_conv2d_fwd_s2_pair_prepack")
    return out


def conv2d_fwd_s2_pair(x, w, w_sc, packed=None):
    """(conv2d(x, w, stride 2, pad 1), conv2d(x, w_sc, stride 2)) in one launch (resnet.py:56-66: both read the block's
    activated input); None when the pair has no such form under the current dispatch options."""
    d = _conv_desc(x.shape, w.shape, 2, 1)
    if tuple(w_sc.shape) != (w.shape[0], w.shape[1], 1, 1):
        raise _hip.AirError("conv2d_fwd_s2_pair: the shortcut must be the 1x1 / stride 2 convolution beside the 3x3 one")
    n = int(_hip.lib().air_conv2d_fwd_s2_pair_prepack_bytes(ctypes.byref(d)))
    if n == 0:
        return None
    if packed is not None and packed.numel() * packed.element_size() < n:
        raise _hip.AirError("conv2d_fwd_s2_pair: packed holds %d bytes, the pair consumes %d under the current dispatch "
                            "options" % (packed.numel() * packed.element_size(), n))
    y = torch.empty((d.B, d.Cout, d.Ho, d.Wo), device=x.device, dtype=torch.float32)
    ysc = torch.empty_like(y)
    ws = workspace(n, x.device) if packed is None else None
    _hip.check(_hip.lib().air_conv2d_fwd_s2_pair(
        ctypes.byref(d), dptr(x), dptr(w), dptr(w_sc), dptr(packed, torch.uint8, allow_none=True), dptr(y), dptr(ysc),
        dptr(ws, torch.uint8, allow_none=True), csz(n if packed is None else 0), stream()), "air_conv2d_fwd_s2_pair")
    return y, ysc


def conv2d_wgrad(x, dy, w_shape, stride=1, padding=0, in_scale=None, in_shift=None, relu=False,
                 out=None):
    d = _conv_desc(x.shape, w_shape, stride, padding)
    dw = out if out is not None else torch.empty(tuple(w_shape), device=x.device, dtype=torch.float32)
    ws, n = _conv_ws(d, x.device)
    _hip.check(_hip.lib().air_conv2d_wgrad(
        ctypes.byref(d), dptr(x), dptr(dy), dptr(dw), dptr(in_scale, allow_none=True),
        dptr(in_shift, allow_none=True), ci(1 if relu else 0), dptr(ws, torch.uint8), csz(n),
        stream()), "air_conv2d_wgrad")
    return dw


def _bcs(x):
    B, C = x.shape[0], x.shape[1]
    S = x.numel() // (B * C)
    return B, C, S


def bn_stats(x, gamma, beta, running_mean=None, running_var=None, eps=1e-5, momentum=0.1, stats_in=None):
    """Training-mode batch statistics.  Returns (mean, invstd, scale, shift); updates
    running stats in place when given.  stats_in: the records ``conv2d_fwd(..., stats=True)`` returned for THIS x
    (merged in fp64 instead of reading x)."""
    B, C, S = _bcs(x)
    coef = torch.empty((4, C), device=x.device, dtype=torch.float32)
    lib = _hip.lib()
    n = lib.air_bn_ws_bytes(ci(B), ci(C), ci(S))
    ws = workspace(n, x.device)
    _hip.check(lib.air_bn_stats(
        dptr(x), ci(B), ci(C), ci(S), dptr(stats_in, torch.uint8, allow_none=True), dptr(gamma), dptr(beta), cf(eps),
        cf(momentum), dptr(running_mean, allow_none=True), dptr(running_var, allow_none=True),
        dptr(coef[0]), dptr(coef[1]), dptr(coef[2]), dptr(coef[3]), dptr(ws, torch.uint8), csz(n),
        stream()), "air_bn_stats")
    return coef[0], coef[1], coef[2], coef[3]


def bn_eval_coeffs(gamma, beta, running_mean, running_var, eps=1e-5):
    C = gamma.numel()
    coef = torch.empty((2, C), device=gamma.device, dtype=torch.float32)
    _hip.check(_hip.lib().air_bn_eval_coeffs(dptr(gamma), dptr(beta), dptr(running_mean),
                                             dptr(running_var), cf(eps), ci(C), dptr(coef[0]),
                                             dptr(coef[1]), stream()), "air_bn_eval_coeffs")
    return coef[0], coef[1]


def bn_coeffs(x, bn, training, stats_in=None, affine=None):
    """(mean, invstd, scale, shift) of the BatchNorm module ``bn`` over x.  Training: batch statistics, the running
    statistics updated and num_batches_tracked queued for bn_flush().  Otherwise (None, None, scale, shift) from the
    running statistics.  stats_in: see bn_stats.  affine: the (gamma, beta) of a layer that has none of its own
    (BatchNorm2d(affine=False): unit scale, zero shift)."""
    gamma, beta = affine if affine is not None else (bn.weight.detach(), bn.bias.detach())
    if training:
        st = bn_stats(x, gamma, beta, bn.running_mean, bn.running_var, bn.eps, bn.momentum, stats_in=stats_in)
        bn_tick(bn.num_batches_tracked)
        return st
    scale, shift = bn_eval_coeffs(gamma, beta, bn.running_mean, bn.running_var, bn.eps)
    return None, None, scale, shift


def bn_apply(x, scale, shift, relu=False, out=None, rowmean=None, y_bf=None):
    """y = x * scale[c] + shift[c] (+ ReLU); rowmean (B, C), 32 <= S <= 1024: also the mean over s of every
    output plane (the SE squeeze taken on the way out)."""
    B, C, S = _bcs(x)
    y = out if out is not None else torch.empty_like(x)
    _hip.check(_hip.lib().air_bn_apply_ex(dptr(x), ci(B), ci(C), ci(S), dptr(scale), dptr(shift),
                                          ci(1 if relu else 0), dptr(y), dptr(rowmean, allow_none=True),
                                          dptr(y_bf, torch.int16, allow_none=True),
                                          ci(y_bf.shape[2] if y_bf is not None else 0), stream()),
               "air_bn_apply_ex")
    return y


def bn_bwd(x, dy, mean, invstd, gamma, beta, relu=False, dx=None, accumulate=False,
           dgamma=None, dbeta=None, relu_in=False, rowbias=None, rowbias_scale=1.0, dbias=None, dy2=None,
           dx_bf16=None, sums_in=None):
    """Backward of y = relu?(batchnorm_train(x)).  Returns (dx, dgamma, dbeta).
    relu_in: x is itself a ReLU output (conv -> ReLU -> BN); dx is then the gradient
    w.r.t. the pre-ReLU tensor.  rowbias (B, C): the incoming gradient is dy + rowbias_scale *
    rowbias[b, c] (broadcast over time).  dbias (C,): receives sum_{b,t} dx, the conv-bias gradient.
    dy (and the optional second gradient dy2, added on the fly) may be channel-slice views.
    dx_bf16: (B, C, Tp) int16 buffer from bf16_rows(): receives dx rounded to bf16, the operand of conv1d_wgrad."""
    B, C, S = _bcs(x)
    if dy.dim() == 3 and (dy2 is not None or not dy.is_contiguous()):
        dyp, dyb = vptr(dy)
        dy2p, dy2b = vptr(dy2) if dy2 is not None else (ctypes.c_void_p(0), 0)
    else:
        dyp, dyb, dy2p, dy2b = dptr(dy), 0, ctypes.c_void_p(0), 0
    if dx is None:
        if accumulate:
            raise _hip.AirError("bn_bwd: accumulate needs an existing dx")
        dx = torch.empty_like(x)
    if dgamma is None:
        dgamma = torch.empty(C, device=x.device, dtype=torch.float32)
    if dbeta is None:
        dbeta = torch.empty(C, device=x.device, dtype=torch.float32)
    lib = _hip.lib()
    n = lib.air_bn_ws_bytes(ci(B), ci(C), ci(S))
    ws = workspace(n, x.device)
    if dx_bf16 is not None and tuple(dx_bf16.shape[:2]) != (B, C):
        raise _hip.AirError("bn_bwd: dx_bf16 must be (B, C, Tp)")
    # sums_in: the records conv2d_dgrad(..., bn=...) took for THIS (x, dy): the pass that re-reads both is skipped
    _hip.check(lib.air_bn_bwd_ex3(dptr(x), dyp, csz(dyb), dy2p, csz(dy2b), dptr(rowbias, allow_none=True),
                                  cf(rowbias_scale), ci(B), ci(C), ci(S), dptr(mean), dptr(invstd), dptr(gamma),
                                  dptr(beta),
                                  ci((1 if relu else 0) | (2 if relu_in else 0)), dptr(dx),
                                  ci(1 if accumulate else 0), dptr(dgamma), dptr(dbeta),
                                  dptr(dbias, allow_none=True), dptr(dx_bf16, torch.int16, allow_none=True),
                                  ci(dx_bf16.shape[2] if dx_bf16 is not None else 0),
                                  dptr(sums_in, torch.uint8, allow_none=True),
                                  dptr(ws, torch.uint8), csz(n), stream()),
               "air_bn_bwd_ex3")
    return dx, dgamma, dbeta


def selfatt_pool_fwd(x, att_w, noise=None):
    """x: (B, C, T).  Returns (out (B, 2C), alpha (B, T))."""
    B, C, T = x.shape
    out = torch.empty((B, 2 * C), device=x.device, dtype=torch.float32)
    alpha = torch.empty((B, T), device=x.device, dtype=torch.float32)
    _hip.check(_hip.lib().air_selfatt_pool_fwd(dptr(x), ci(B), ci(C), ci(T), dptr(att_w),
                                               dptr(noise, allow_none=True), dptr(out), dptr(alpha),
                                               stream()), "air_selfatt_pool_fwd")
    return out, alpha


def selfatt_pool_bwd(x, att_w, noise, alpha, out, dout):
    """Returns (dx (B,C,T), datt_partial (B,C))."""
    B, C, T = x.shape
    dx = torch.empty_like(x)
    datt = torch.empty((B, C), device=x.device, dtype=torch.float32)
    _hip.check(_hip.lib().air_selfatt_pool_bwd(dptr(x), ci(B), ci(C), ci(T), dptr(att_w),
                                               dptr(noise, allow_none=True), dptr(alpha), dptr(out),
                                               dptr(dout), dptr(dx), dptr(datt), stream()),
               "air_selfatt_pool_bwd")
    return dx, datt


def linear_fwd(x, w, b=None, relu=False):
    M, K = x.shape
    N = w.shape[0]
    y = torch.empty((M, N), device=x.device, dtype=torch.float32)
    fn = _hip.lib().air_linear_relu_fwd if relu else _hip.lib().air_linear_fwd
    _hip.check(fn(dptr(x), dptr(w), dptr(b, allow_none=True), ci(M), ci(K), ci(N), dptr(y),
                  stream()), "air_linear_fwd")
    return y


def linear_bwd(x, w, dy, need_dx=True, dw=None, db=None, need_db=True):
    M, K = x.shape
    N = w.shape[0]
    dx = torch.empty_like(x) if need_dx else None
    if dw is None:
        dw = torch.empty_like(w)
    if db is None and need_db:
        db = torch.empty(N, device=x.device, dtype=torch.float32)
    _hip.check(_hip.lib().air_linear_bwd(dptr(x), dptr(w), dptr(dy), ci(M), ci(K), ci(N),
                                         dptr(dx, allow_none=True), dptr(dw),
                                         dptr(db, allow_none=True), stream()), "air_linear_bwd")
    return dx, dw, db


def ocsoftmax_fwd(x, center, labels, r_real, r_fake, alpha):
    B, D = x.shape
    loss = torch.empty((), device=x.device, dtype=torch.float32)
    neg = torch.empty(B, device=x.device, dtype=torch.float32)
    _hip.check(_hip.lib().air_ocsoftmax_fwd(dptr(x), dptr(center), dptr(labels, torch.int64), ci(B),
                                            ci(D), cf(r_real), cf(r_fake), cf(alpha), dptr(loss),
                                            dptr(neg), stream()), "air_ocsoftmax_fwd")
    return loss, neg


def ocsoftmax_bwd(x, center, labels, r_real, r_fake, alpha, gscale=None, dcenter=None):
    B, D = x.shape
    dx = torch.empty_like(x)
    if dcenter is None:
        dcenter = torch.empty_like(center)
    _hip.check(_hip.lib().air_ocsoftmax_bwd(dptr(x), dptr(center), dptr(labels, torch.int64), ci(B),
                                            ci(D), cf(r_real), cf(r_fake), cf(alpha),
                                            dptr(gscale, allow_none=True), dptr(dx), dptr(dcenter),
                                            stream()), "air_ocsoftmax_bwd")
    return dx, dcenter


def p2sgrad_fwd(x, weight, labels, smooth):
    B, D = x.shape
    C = weight.shape[1]
    loss = torch.empty((), device=x.device, dtype=torch.float32)
    neg = torch.empty(B, device=x.device, dtype=torch.float32)
    _hip.check(_hip.lib().air_p2sgrad_fwd(dptr(x), dptr(weight), dptr(labels, torch.int64), ci(B), ci(D), ci(C),
                                          cf(smooth), dptr(loss), dptr(neg), stream()), "air_p2sgrad_fwd")
    return loss, neg


def p2sgrad_bwd(x, weight, labels, smooth, gscale=None):
    B, D = x.shape
    C = weight.shape[1]
    dx = torch.empty_like(x)
    dw = torch.empty_like(weight)
    _hip.check(_hip.lib().air_p2sgrad_bwd(dptr(x), dptr(weight), dptr(labels, torch.int64), ci(B), ci(D), ci(C),
                                          cf(smooth), dptr(gscale, allow_none=True), dptr(dx), dptr(dw), stream()),
               "air_p2sgrad_bwd")
    return dx, dw


def isolate_fwd(x, center, labels, r_real, r_fake, square, want_dist=False):
    """r_real / r_fake as the module holds them (squared here for IsolateSquareLoss).  want_dist: also |x - c| per
    row -> (loss, dist)."""
    B, D = x.shape
    if square:
        r_real, r_fake = r_real ** 2, r_fake ** 2
    loss = torch.empty((), device=x.device, dtype=torch.float32)
    dist = torch.empty(B, device=x.device, dtype=torch.float32) if want_dist else None
    _hip.check(_hip.lib().air_isolate_fwd(dptr(x), dptr(center), dptr(labels, torch.int64), ci(B), ci(D), cf(r_real),
                                          cf(r_fake), ci(1 if square else 0), dptr(loss),
                                          dptr(dist, allow_none=True), stream()), "air_isolate_fwd")
    return (loss, dist) if want_dist else loss


def isolate_bwd(x, center, labels, r_real, r_fake, square, gscale=None):
    B, D = x.shape
    if square:
        r_real, r_fake = r_real ** 2, r_fake ** 2
    dx = torch.empty_like(x)
    dc = torch.empty_like(center)
    _hip.check(_hip.lib().air_isolate_bwd(dptr(x), dptr(center), dptr(labels, torch.int64), ci(B), ci(D), cf(r_real),
                                          cf(r_fake), ci(1 if square else 0), dptr(gscale, allow_none=True), dptr(dx),
                                          dptr(dc), stream()), "air_isolate_bwd")
    return dx, dc


def amsoftmax_fwd(x, centers, labels, s, m):
    B, D = x.shape
    C = centers.shape[0]
    logits = torch.empty(B, C, device=x.device, dtype=torch.float32)
    margin = torch.empty(B, C, device=x.device, dtype=torch.float32)
    _hip.check(_hip.lib().air_amsoftmax_fwd(dptr(x), dptr(centers), dptr(labels, torch.int64), ci(B), ci(D), ci(C),
                                            cf(s), cf(m), dptr(logits), dptr(margin), stream()), "air_amsoftmax_fwd")
    return logits, margin


def adam_step(p, g, m, v, step, lr=5e-4, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=5e-4,
              grad_scale=1.0):
    _hip.check(_hip.lib().air_adam_step(dptr(p), dptr(g), dptr(m), dptr(v), csz(p.numel()),
                                        ci(step), cf(lr), cf(beta1), cf(beta2), cf(eps),
                                        cf(weight_decay), cf(grad_scale), stream()), "air_adam_step")


def sgd_step(p, g, lr, grad_scale=1.0):
    _hip.check(_hip.lib().air_sgd_step(dptr(p), dptr(g), csz(p.numel()), cf(lr), cf(grad_scale),
                                       stream()), "air_sgd_step")


def add_(y, x):
    _hip.check(_hip.lib().air_add_inplace(dptr(y), dptr(x), csz(y.numel()), stream()),
               "air_add_inplace")
    return y


def sum_rows(x, out=None):
    M, N = x.shape
    if out is None:
        out = torch.empty(N, device=x.device, dtype=torch.float32)
    _hip.check(_hip.lib().air_sum_rows(dptr(x), ci(M), ci(N), dptr(out), stream()), "air_sum_rows")
    return out


def randn(shape, device, seed, offset, scale=1.0):
    out = torch.empty(shape, device=device, dtype=torch.float32)
    _hip.check(_hip.lib().air_randn(dptr(out), csz(out.numel()), ctypes.c_uint64(seed),
                                    ctypes.c_uint64(offset), cf(scale), stream()), "air_randn")
    return out


def randn_ctr(shape, device, seed, counter, scale=1.0):
    """randn() with the stream offset in device memory: ``counter`` is a 1-element int64 GPU tensor that the call reads
    and then advances by ceil(numel / 4) on the stream - capturable in a hipGraph, and the same sequence eagerly."""
    if counter.dtype != torch.int64 or not counter.is_cuda or counter.numel() != 1:
        raise _hip.AirError("randn_ctr: counter must be a 1-element int64 GPU tensor")
    out = torch.empty(shape, device=device, dtype=torch.float32)
    _hip.check(_hip.lib().air_randn_ctr(dptr(out), csz(out.numel()), ctypes.c_uint64(seed),
                                        dptr(counter, torch.int64), cf(scale), stream()), "air_randn_ctr")
    return out


# ------------------------------------------------------------------ LCNN (lcnn.py)
def lcnn_conv1_fwd(x, w, bias):
    """conv1 of model.py:528-530 fused: (pooled MFM output (B, 32, H/2, W/2), route bytes of the same shape)."""
    B, _, H, W = x.shape
    y = torch.empty((B, 32, H // 2, W // 2), device=x.device, dtype=torch.float32)
    route = torch.empty(y.shape, device=x.device, dtype=torch.uint8)
    _hip.check(_hip.lib().air_lcnn_conv1_fwd(dptr(x), dptr(w), dptr(bias), ci(B), ci(H), ci(W), dptr(y),
                                             dptr(route, torch.uint8), stream()), "air_lcnn_conv1_fwd")
    return y, route


def lcnn_conv1_wgrad(x, dy, route, dw, db):
    B, _, H, W = x.shape
    n = int(_hip.lib().air_lcnn_conv1_wgrad_ws_bytes())
    ws = workspace(n, x.device)
    _hip.check(_hip.lib().air_lcnn_conv1_wgrad(dptr(x), dptr(dy), dptr(route, torch.uint8), ci(B), ci(H), ci(W),
                                               dptr(dw), dptr(db), dptr(ws, torch.uint8), csz(n), stream()),
               "air_lcnn_conv1_wgrad")
    return dw, db


def mfm_pool_fwd(x, C=None, bias=None, pool=False):
    """MaxFeatureMap2D over channels [0, C) of x (B, Ctot, H, W) (+ bias), then an optional 2x2 floor-mode max-pool.
    Returns (y (B, C/2, Ho, Wo), route bytes)."""
    B, Ctot, H, W = x.shape
    C = Ctot if C is None else C
    Ho, Wo = (H // 2, W // 2) if pool else (H, W)
    y = torch.empty((B, C // 2, Ho, Wo), device=x.device, dtype=torch.float32)
    route = torch.empty(y.shape, device=x.device, dtype=torch.uint8)
    _hip.check(_hip.lib().air_mfm_pool_fwd(dptr(x), dptr(bias, allow_none=True), ci(B), ci(Ctot), ci(C), ci(H), ci(W),
                                           ci(1 if pool else 0), dptr(y), dptr(route, torch.uint8), stream()),
               "air_mfm_pool_fwd")
    return y, route


def mfm_pool_bwd(dy, route, x_shape, C=None, pool=False, out=None):
    """Gradient with respect to mfm_pool_fwd's x: dy where the element won, zero elsewhere."""
    B, Ctot, H, W = x_shape
    C = Ctot if C is None else C
    dx = out if out is not None else torch.empty(tuple(x_shape), device=dy.device, dtype=torch.float32)
    _hip.check(_hip.lib().air_mfm_pool_bwd(dptr(dy), dptr(route, torch.uint8), ci(B), ci(Ctot), ci(C), ci(H), ci(W),
                                           ci(1 if pool else 0), dptr(dx), stream()), "air_mfm_pool_bwd")
    return dx


def mfm_bias_grad(dy, route, out=None):
    """Bias gradient of the convolution in front of an MFM: (C,) from dy (B, C/2, ...) and its route bytes."""
    B, C2 = dy.shape[0], dy.shape[1]
    S = dy.numel() // (B * C2)
    db = out if out is not None else torch.empty(2 * C2, device=dy.device, dtype=torch.float32)
    n = int(_hip.lib().air_mfm_bias_grad_ws_bytes(ci(2 * C2)))
    ws = workspace(n, dy.device)
    _hip.check(_hip.lib().air_mfm_bias_grad(dptr(dy), dptr(route, torch.uint8), ci(B), ci(2 * C2), ci(S), dptr(db),
                                            dptr(ws, torch.uint8), csz(n), stream()), "air_mfm_bias_grad")
    return db


def copy_pad(dst, src):
    """dst[:n] = src[:n] (n = the smaller size), zeros behind src in dst."""
    _hip.check(_hip.lib().air_copy_pad(dptr(dst), csz(dst.numel()), dptr(src), csz(src.numel()), stream()),
               "air_copy_pad")
    return dst


def mul(a, b, out=None):
    y = out if out is not None else torch.empty_like(a)
    _hip.check(_hip.lib().air_mul(dptr(a), dptr(b), csz(a.numel()), dptr(y), stream()), "air_mul")
    return y


def dropout_mask_ctr(shape, p, seed, counter, device):
    """nn.Dropout(p)'s scaled keep-mask from Philox4x32-10 with the offset in ``counter`` (1-element int64 GPU
    tensor, advanced on the stream): capturable, and eager calls and replays walk one sequence."""
    if counter.dtype != torch.int64 or not counter.is_cuda or counter.numel() != 1:
        raise _hip.AirError("dropout_mask_ctr: counter must be a 1-element int64 GPU tensor")
    keep = torch.empty(shape, device=device, dtype=torch.float32)
    _hip.check(_hip.lib().air_dropout_mask_ctr(dptr(keep), csz(keep.numel()), cf(p), ctypes.c_uint64(seed),
                                               dptr(counter, torch.int64), stream()), "air_dropout_mask_ctr")
    return keep


class AdvHead:
    """One channel-classifier head as ``adv_heads`` takes it: ``flat`` = [w1 (H, D) | b1 (H) | w2 (C, H) | b2 (C)] in one
    fp32 block, ``grad`` the gradient block of the same layout, ``p`` the dropout probability in force (0: eval),
    ``seed`` / ``counter`` (1-element int64 GPU tensor) the in-kernel draw's Philox key and device-side offset."""

    def __init__(self, flat, grad, nclasses, p=0.0, seed=0, counter=None):
        self.flat, self.grad, self.nclasses, self.p, self.seed, self.counter = flat, grad, int(nclasses), float(p), int(seed), counter


def adv_head_numel(D, C):
    H = D // 2
    return H * D + H + C * H + C


def adv_heads(feats, heads, targets, lambda_, want_dx, keeps=None, run_correct=None):
    """Every classifier head of one phase of the --ADV_AUG step in one fused call (air_adv_heads): ``feats`` (B, D) fp32,
    ``heads`` 1 - 4 ``AdvHead``-like objects, ``targets`` one int64 (B,) tensor per head, ``keeps`` optional explicit
    scaled keep masks (B, D // 2) per head (None entries: the head's own draw, or none), ``run_correct`` optional int64
    (n,) running totals.  Returns (losses (n,), correct (n,) int32, dx (B, D) or None); the gradients are written
    into the heads' ``grad`` blocks."""
    n = len(heads)
    if not 1 <= n <= _hip.ADV_MAX_HEADS or len(targets) != n or (keeps is not None and len(keeps) != n):
        raise ValueError("adv_heads takes 1 - %d heads with one target tensor (and keep mask) each" % _hip.ADV_MAX_HEADS)
    if feats.dim() != 2:
        raise ValueError("expected (B, D) features")
    B, D = feats.shape
    H = D // 2
    dev = feats.device
    losses = torch.empty(n, device=dev, dtype=torch.float32)
    correct = torch.empty(n, device=dev, dtype=torch.int32)
    dx = torch.empty(B, D, device=dev, dtype=torch.float32) if want_dx else None
    if run_correct is not None and (run_correct.dtype != torch.int64 or run_correct.numel() != n):
        raise _hip.AirError("adv_heads: run_correct must be an int64 GPU tensor with one entry per head")
    d = _hip.AirAdvHeads()
    d.B, d.D, d.nheads, d.want_dx, d.lambda_ = B, D, n, int(bool(want_dx)), float(lambda_)
    d.feats = dptr(feats).value
    d.dx = dptr(dx, allow_none=True).value
    counts = (ctypes.c_int * n)(*[int(h.nclasses) for h in heads])
    nbytes = _hip.lib().air_adv_heads_ws_bytes(ci(B), ci(D), ci(n), counts, ci(d.want_dx))
    if nbytes == 0:
        raise _hip.AirError("adv_heads: unsupported shape B=%d D=%d classes=%s" % (B, D, list(counts)))
    ws = workspace(nbytes, dev)
    d.ws, d.ws_bytes = ws.data_ptr(), ws.numel()
    hold = []
    for k, h in enumerate(heads):
        C = int(h.nclasses)
        if h.flat.numel() != adv_head_numel(D, C) or h.grad.numel() != h.flat.numel():
            raise _hip.AirError("adv_heads: head %d's blocks do not hold a (%d -> %d -> %d) classifier" % (k, D, H, C))
        tgt = targets[k]
        if tgt.numel() != B:
            raise ValueError("adv_heads: head %d needs %d targets, got %d" % (k, B, tgt.numel()))
        base, gbase = dptr(h.flat).value, dptr(h.grad).value
        e = d.head[k]
        e.w1, e.b1, e.w2, e.b2 = base, base + 4 * H * D, base + 4 * (H * D + H), base + 4 * (H * D + H + C * H)
        e.targets = dptr(tgt, torch.int64).value
        keep = keeps[k] if keeps is not None else None
        if keep is not None:
            if tuple(keep.shape) != (B, H):
                raise ValueError("adv_heads: keep mask of head %d must be (%d, %d)" % (k, B, H))
            e.keep = dptr(keep).value
        ctr = getattr(h, "counter", None)
        if ctr is not None:
            if ctr.dtype != torch.int64 or not ctr.is_cuda or ctr.numel() != 1:
                raise _hip.AirError("adv_heads: counter must be a 1-element int64 GPU tensor")
            e.counter = ctr.data_ptr()
        e.seed, e.C, e.p = int(h.seed) & 0xFFFFFFFFFFFFFFFF, C, float(h.p)
        e.grads = gbase
        e.loss = losses.data_ptr() + 4 * k
        e.correct = correct.data_ptr() + 4 * k
        if run_correct is not None:
            e.run_correct = dptr(run_correct, torch.int64).value + 8 * k
        hold.append((tgt, keep, ctr))
    _hip.check(_hip.lib().air_adv_heads(ctypes.byref(d), stream()), "air_adv_heads")
    return losses, correct, dx


# ------------------------------------------------------------------ Res2Net (res2net.py)
def sptr(t):
    """(pointer, batch stride) of a (B, C, H, W) fp32 GPU tensor or channel-slice view whose (C, H, W) block is
    dense."""
    if t.dim() != 4 or not t.is_cuda or t.dtype != torch.float32:
        raise _hip.AirError("expected a (B, C, H, W) fp32 GPU tensor")
    B, C, H, W = t.shape
    if t.stride(3) != 1 or (H > 1 and t.stride(2) != W) or (C > 1 and t.stride(1) != H * W):
        raise _hip.AirError("channel-slice view must keep (C, H, W) dense")
    return ctypes.c_void_p(t.data_ptr()), (t.stride(0) if B > 1 else C * H * W)


def _narrow_desc(x_shape, cout, k, stride, x_bs=0, y_bs=0):
    B, Cin, H, W = x_shape
    if k not in (1, 3):
        raise _hip.AirError("conv_narrow: kernel %d (1 or 3 only)" % k)
    pad = k // 2
    Ho, Wo = (H + 2 * pad - k) // stride + 1, (W + 2 * pad - k) // stride + 1
    return AirConvNarrow(B, Cin, H, W, cout, k, stride, Ho, Wo, x_bs, y_bs)


def conv_narrow_fwd(x, w, stride=1, in_scale=None, in_shift=None, relu=False, out=None):
    """y = conv2d(act(x), w, stride, padding=k // 2) on the narrow-channel kernels; act = optional x*in_scale + in_shift
    (+ ReLU).  x and ``out`` may be channel-slice views."""
    xp, xb = sptr(x)
    d = _narrow_desc(x.shape, w.shape[0], w.shape[2], stride, xb)
    if out is None:
        out = torch.empty((d.B, d.Cout, d.Ho, d.Wo), device=x.device, dtype=torch.float32)
    if tuple(out.shape) != (d.B, d.Cout, d.Ho, d.Wo):
        raise _hip.AirError("conv_narrow_fwd: out is %s, want %s" % (tuple(out.shape), (d.B, d.Cout, d.Ho, d.Wo)))
    yp, yb = sptr(out)
    d.y_bstride = yb
    _hip.check(_hip.lib().air_conv_narrow_fwd(ctypes.byref(d), xp, dptr(w), dptr(in_scale, allow_none=True),
                                              dptr(in_shift, allow_none=True), ci(1 if relu else 0), yp, stream()),
               "air_conv_narrow_fwd")
    return out


def conv_narrow_dgrad(dy, w, x_shape, stride=1, out=None, accumulate=False):
    """Gradient with respect to conv_narrow_fwd's (activated) input; ``out`` (may be a channel-slice view) is written,
    or added to with accumulate."""
    d = _narrow_desc(tuple(x_shape), w.shape[0], w.shape[2], stride)
    if accumulate and out is None:
        raise _hip.AirError("conv_narrow_dgrad: accumulate needs out")
    if out is None:
        out = torch.empty(tuple(x_shape), device=dy.device, dtype=torch.float32)
    gp, gb = sptr(dy)
    xp, xb = sptr(out)
    if tuple(dy.shape) != (d.B, d.Cout, d.Ho, d.Wo) or tuple(out.shape) != tuple(x_shape):
        raise _hip.AirError("conv_narrow_dgrad: shapes dy %s / dx %s do not match" % (tuple(dy.shape), tuple(out.shape)))
    d.x_bstride, d.y_bstride = xb, gb
    _hip.check(_hip.lib().air_conv_narrow_dgrad(ctypes.byref(d), gp, dptr(w), xp, ci(1 if accumulate else 0),
                                                stream()), "air_conv_narrow_dgrad")
    return out


def conv_narrow_wgrad(x, dy, w_shape, stride=1, in_scale=None, in_shift=None, relu=False, out=None):
    """dw (Cout, Cin, k, k) of conv_narrow_fwd (same prologue); deterministic.  x and dy may be channel-slice views."""
    xp, xb = sptr(x)
    gp, gb = sptr(dy)
    d = _narrow_desc(x.shape, w_shape[0], w_shape[2], stride, xb, gb)
    if tuple(dy.shape) != (d.B, d.Cout, d.Ho, d.Wo):
        raise _hip.AirError("conv_narrow_wgrad: dy is %s, want %s" % (tuple(dy.shape), (d.B, d.Cout, d.Ho, d.Wo)))
    dw = out if out is not None else torch.empty(tuple(w_shape), device=x.device, dtype=torch.float32)
    n = int(_hip.lib().air_conv_narrow_wgrad_ws_bytes(ctypes.byref(d)))
    if n == 0:
        raise _hip.AirError("conv_narrow_wgrad: unsupported shape %s -> %s" % (tuple(x.shape), tuple(w_shape)))
    ws = workspace(n, x.device)
    _hip.check(_hip.lib().air_conv_narrow_wgrad(ctypes.byref(d), xp, gp, dptr(in_scale, allow_none=True),
                                                dptr(in_shift, allow_none=True), ci(1 if relu else 0), dptr(dw),
                                                dptr(ws, torch.uint8), csz(n), stream()), "air_conv_narrow_wgrad")
    return dw


def res2_bn_relu_apply(x, scale, shift, y1, add=None, y2=None):
    """y1 (channel-slice view) = relu(x*scale + shift); y2 (dense) = that + add (channel-slice view).  4-D tensors;
    x may be a channel slice too."""
    B, C, H, W = x.shape
    xp, xb = sptr(x)
    y1p, y1b = sptr(y1)
    ap, ab = sptr(add) if add is not None else (ctypes.c_void_p(0), 0)
    _hip.check(_hip.lib().air_res2_bn_relu_apply(xp, csz(xb), ci(B), ci(C), ci(H * W), dptr(scale), dptr(shift), y1p,
                                                 csz(y1b), ap, csz(ab), dptr(y2, allow_none=True), stream()),
               "air_res2_bn_relu_apply")
    return y2


def pool_out_size(n, k, stride, pad, ceil_mode):
    """PyTorch's pooling output size."""
    num = n + 2 * pad - k
    o = (-(-num // stride) if ceil_mode else num // stride) + 1
    if ceil_mode and (o - 1) * stride >= n + pad:
        o -= 1
    return o


def avgpool2d_fwd(x, k, stride, pad, ceil_mode, count_include_pad, out=None):
    """nn.AvgPool2d forward; x and ``out`` may be channel-slice views."""
    B, C, H, W = x.shape
    Ho, Wo = pool_out_size(H, k, stride, pad, ceil_mode), pool_out_size(W, k, stride, pad, ceil_mode)
    if out is None:
        out = torch.empty((B, C, Ho, Wo), device=x.device, dtype=torch.float32)
    xp, xb = sptr(x)
    yp, yb = sptr(out)
    _hip.check(_hip.lib().air_avgpool2d_fwd(xp, csz(xb), ci(B), ci(C), ci(H), ci(W), ci(k), ci(stride), ci(pad),
                                            ci(1 if ceil_mode else 0), ci(1 if count_include_pad else 0), ci(Ho),
                                            ci(Wo), yp, csz(yb), stream()), "air_avgpool2d_fwd")
    return out


def avgpool2d_bwd(dy, x_shape, k, stride, pad, ceil_mode, count_include_pad, out=None, accumulate=False):
    """Gradient of avgpool2d_fwd with respect to x (``out`` may be a channel-slice view; accumulate adds to it)."""
    B, C, H, W = x_shape
    Ho, Wo = dy.shape[2], dy.shape[3]
    if accumulate and out is None:
        raise _hip.AirError("avgpool2d_bwd: accumulate needs out")
    if out is None:
        out = torch.empty(tuple(x_shape), device=dy.device, dtype=torch.float32)
    gp, gb = sptr(dy)
    xp, xb = sptr(out)
    _hip.check(_hip.lib().air_avgpool2d_bwd(gp, csz(gb), ci(B), ci(C), ci(H), ci(W), ci(k), ci(stride), ci(pad),
                                            ci(1 if ceil_mode else 0), ci(1 if count_include_pad else 0), ci(Ho),
                                            ci(Wo), xp, csz(xb), ci(1 if accumulate else 0), stream()),
               "air_avgpool2d_bwd")
    return out


def se_relu_fwd(x, z, res, out=None):
    """out = relu(x * sigmoid(z[b, c]) + res), all dense (B, C, ...)."""
    B, C, S = _bcs(x)
    out = out if out is not None else torch.empty_like(x)
    _hip.check(_hip.lib().air_se_relu_fwd(dptr(x), dptr(z), dptr(res), ci(B), ci(C), ci(S), dptr(out), stream()),
               "air_se_relu_fwd")
    return out


def se_relu_bwd(x, z, out, dout, want_dres=True):
    """Returns (dx, dz, dres or None) of se_relu_fwd."""
    B, C, S = _bcs(x)
    dx = torch.empty_like(x)
    dz = torch.empty_like(z)
    dres = torch.empty_like(x) if want_dres else None
    _hip.check(_hip.lib().air_se_relu_bwd(dptr(x), dptr(z), dptr(out), dptr(dout), ci(B), ci(C), ci(S), dptr(dx),
                                          dptr(dz), dptr(dres, allow_none=True), stream()), "air_se_relu_bwd")
    return dx, dz, dres


def log_softmax_fwd(z):
    B, C = z.shape
    out = torch.empty_like(z)
    _hip.check(_hip.lib().air_log_softmax_fwd(dptr(z), ci(B), ci(C), dptr(out), stream()), "air_log_softmax_fwd")
    return out


def log_softmax_bwd(out, dout):
    B, C = out.shape
    dz = torch.empty_like(out)
    _hip.check(_hip.lib().air_log_softmax_bwd(dptr(out), dptr(dout), ci(B), ci(C), dptr(dz), stream()),
               "air_log_softmax_bwd")
    return dz


# ------------------------------------------------------------------ ECAPA (B, C, T) ops
def vptr(t):
    """(pointer, batch stride) of a (B, C, T) tensor or channel-slice view whose (C, T)
    block is dense."""
    if t.dim() != 3 or not t.is_cuda or t.dtype != torch.float32:
        raise _hip.AirError("expected a (B, C, T) fp32 GPU tensor")
    B, C, T = t.shape
    if t.stride(2) != 1 or (C > 1 and t.stride(1) != T):
        raise _hip.AirError("channel-slice view must keep (C, T) dense")
    return ctypes.c_void_p(t.data_ptr()), (t.stride(0) if B > 1 else C * T)


def _c1d(x, cout, K, dil, pad, y=None):
    B, Cin, T = x.shape
    xp, xb = vptr(x)
    yb = vptr(y)[1] if y is not None else cout * T
    d = AirConv1d(B, Cin, T, cout, K, dil, pad, xb, yb)
    n = _hip.lib().air_conv1d_ws_bytes(ctypes.byref(d))
    if n == 0:
        raise _hip.AirError("conv1d: unsupported configuration K=%d dil=%d pad=%d" % (K, dil, pad))
    return d, workspace(n, x.device), n


def _c1d_bf16(d, device, which):
    """Workspace for the bf16 kernels (pointwise layers; dilated K = 3 forward / dgrad), or None when the
    layer is not theirs (K = 5, ragged channel counts, K = 3 wgrad): the caller then runs the fp32 kernels."""
    lib = _hip.lib()
    if not lib.air_conv1d_bf16_supported(ctypes.byref(d), ci(which)):
        return None, 0
    n = lib.air_conv1d_bf16_ws_bytes(ctypes.byref(d))
    return workspace(n, device), n


def conv1d_tap_pack(weights, transpose, out=None):
    """bf16 operand blocks of a list of equally shaped K = 3 conv weights, packed in ONE launch when they sit at a
    regular stride in memory (the Res2 branch convs inside the parameter arena) and one launch per weight otherwise
    (parameters re-assigned outside the arena).  Returns an (n, 3*Cout*Cin) int16 tensor whose rows are the w_packed
    arguments of conv1d_fwd / conv1d_dgrad / ops_h.conv_tap; None only for shapes the tap kernels do not take."""
    w0 = weights[0]
    n = len(weights)
    Cout, Cin, K = w0.shape
    if K != 3 or any(w.shape != w0.shape or w.dtype != torch.float32 or not w.is_cuda for w in weights):
        return None
    weights = [w if w.is_contiguous() else w.contiguous() for w in weights]
    w0 = weights[0]
    stride = (weights[1].data_ptr() - w0.data_ptr()) // 4 if n > 1 else 0
    regular = n == 1 or (stride > 0 and all(w.data_ptr() == w0.data_ptr() + 4 * stride * i for i, w in enumerate(weights)))
    per = Cout * Cin * 3
    if out is None:
        out = torch.empty((n, per), device=w0.device, dtype=torch.int16)
    tr = ci(1 if transpose else 0)
    if regular:
        _hip.check(_hip.lib().air_conv1d_tap_pack_bf16(dptr(w0), csz(stride), ci(n), ci(Cout), ci(Cin), tr,
                                                       dptr(out, torch.int16), stream()), "air_conv1d_tap_pack_bf16")
    else:
        for i, w in enumerate(weights):
            _hip.check(_hip.lib().air_conv1d_tap_pack_bf16(dptr(w), csz(0), ci(1), ci(Cout), ci(Cin), tr,
                                                           dptr(out[i], torch.int16), stream()),
                       "air_conv1d_tap_pack_bf16")
    return out


def conv1d_fwd(x, w, bias=None, bias_bc=None, relu=False, dil=1, pad=0, out=None, bf16=False, y_bf=None,
               w_packed=None):
    """y = relu?(conv1d(x, w) + bias + bias_bc[b]); x / out may be channel-slice views.
    bf16: pointwise layers run on the bf16 matrix cores (operands rounded, fp32 accumulate); y_bf (bf16_rows
    buffer, bf16 path only) also receives y rounded to bf16 - the X operand of a later conv1d_wgrad."""
    Cout, Cin, K = w.shape
    B, _, T = x.shape
    y = out if out is not None else torch.empty((B, Cout, T), device=x.device, dtype=torch.float32)
    d, ws, n = _c1d(x, Cout, K, dil, pad, y)
    if bf16:
        wsb, nb = _c1d_bf16(d, x.device, 0)
        if wsb is not None:
            _hip.check(_hip.lib().air_conv1d_fwd_bf16_ex(
                ctypes.byref(d), vptr(x)[0], dptr(w), dptr(w_packed, torch.int16, allow_none=True),
                dptr(bias, allow_none=True),
                dptr(bias_bc, allow_none=True), ci(1 if relu else 0), vptr(y)[0],
                dptr(y_bf, torch.int16, allow_none=True),
                dptr(wsb, torch.uint8), csz(nb), stream()), "air_conv1d_fwd_bf16_ex")
            return y
    if y_bf is not None:
        raise _hip.AirError("conv1d_fwd: y_bf needs the bf16 path")
    _hip.check(_hip.lib().air_conv1d_fwd(ctypes.byref(d), vptr(x)[0], dptr(w), dptr(bias, allow_none=True),
                                         dptr(bias_bc, allow_none=True), ci(1 if relu else 0), vptr(y)[0],
                                         dptr(ws, torch.uint8), csz(n), stream()), "air_conv1d_fwd")
    return y


def conv1d_pointwise_kmajor(xb, w, T, dgrad=False, bias=None, bias_bc=None, relu=False, accumulate=None, out=None,
                            y_bf=None, accumulate2=None):
    """K = 1 forward (y = W . x) or data gradient (dx = W^T . dy + accumulate) straight from the bf16 copy ``xb``
    ((B, C, Tp) int16, or a channel slice of one) of the input operand.  Returns None when the layer does not fit the
    K-major GEMM (the caller falls back to conv1d_fwd / conv1d_dgrad on the fp32 tensor)."""
    Cout, Cin, K = w.shape
    B = xb.shape[0]
    Cy = Cin if dgrad else Cout
    if K != 1 or xb.shape[1] != (Cout if dgrad else Cin):
        return None
    y = out if out is not None else torch.empty((B, Cy, T), device=xb.device, dtype=torch.float32)
    yp, yb = vptr(y)
    d = AirConv1d(B, Cin, T, Cout, 1, 1, 0, yb if dgrad else 0, 0 if dgrad else yb)
    wsb, nb = _c1d_bf16(d, xb.device, 1 if dgrad else 0)
    if wsb is None:
        return None
    xp, xbs_ = _bf_view(xb)
    acc, accb = vptr(accumulate) if accumulate is not None else (ctypes.c_void_p(0), 0)
    acc2, acc2b = vptr(accumulate2) if accumulate2 is not None else (ctypes.c_void_p(0), 0)
    rc = _hip.lib().air_conv1d_pointwise_bf16_kmajor(
        ctypes.byref(d), xp, csz(xbs_), dptr(w), ci(1 if dgrad else 0), dptr(bias, allow_none=True),
        dptr(bias_bc, allow_none=True), ci(1 if relu else 0), acc, csz(accb), acc2, csz(acc2b), yp,
        dptr(y_bf, torch.int16, allow_none=True),
        dptr(wsb, torch.uint8), csz(nb), stream())
    if rc == -2:  # AIR_EUNSUPPORTED: shape outside the K-major kernel
        return None
    _hip.check(rc, "air_conv1d_pointwise_bf16_kmajor")
    return y


def conv1d_dgrad(dy, w, dil=1, pad=0, accumulate=None, out=None, bf16=False, accumulate2=None, w_packed=None):
    """dx = conv1d_transpose(dy, w) (+ accumulate, addressed like out).  bf16 pointwise path: accumulate may be a
    channel-slice view and a second operand accumulate2 (view or dense) is added in the same epilogue."""
    Cout, Cin, K = w.shape
    B, _, T = dy.shape
    dx = out if out is not None else torch.empty((B, Cin, T), device=dy.device, dtype=torch.float32)
    xp, xb = vptr(dx)
    yp, yb = vptr(dy)
    d = AirConv1d(B, Cin, T, Cout, K, dil, pad, xb, yb)
    acc, accb = vptr(accumulate) if accumulate is not None else (ctypes.c_void_p(0), 0)
    if bf16:
        wsb, nb = _c1d_bf16(d, dy.device, 1)
        if wsb is not None:
            acc2, acc2b = vptr(accumulate2) if accumulate2 is not None else (ctypes.c_void_p(0), 0)
            _hip.check(_hip.lib().air_conv1d_dgrad_bf16_ex(ctypes.byref(d), yp, dptr(w),
                                                           dptr(w_packed, torch.int16, allow_none=True), xp, acc,
                                                           csz(accb), acc2,
                                                           csz(acc2b), dptr(wsb, torch.uint8), csz(nb), stream()),
                       "air_conv1d_dgrad_bf16_ex")
            return dx
    if accumulate2 is not None or (accumulate is not None and accb != xb):
        raise _hip.AirError("conv1d_dgrad: a second / strided accumulate operand needs the bf16 pointwise path")
    n = _hip.lib().air_conv1d_ws_bytes(ctypes.byref(d))
    ws = workspace(n, dy.device)
    _hip.check(_hip.lib().air_conv1d_dgrad(ctypes.byref(d), yp, dptr(w), xp, acc, dptr(ws, torch.uint8),
                                           csz(n), stream()), "air_conv1d_dgrad")
    return dx


_BF_ROWS = {}


def bf16_rows(tag, B, C, T, device):
    """Zero-padded (B, C, Tp) int16 buffer for a bf16 operand copy (Tp = air_conv1d_bf16_tp(T)).  With a tag: one
    persistent buffer per (tag, shape), for copies made and consumed inside one backward pass - writers only
    touch frames < T, so the padding stays zero for as long as the buffer lives.  tag None: fresh memory."""
    Tp = int(_hip.lib().air_conv1d_bf16_tp(ci(T)))
    if tag is None:  # a copy that outlives the call sequence (saved for backward): its own memory, padding zeroed
        buf = torch.empty((B, C, Tp), device=device, dtype=torch.int16)
        if Tp > T:
            buf[:, :, T:].zero_()
        return buf
    key = (tag, B, C, Tp, device.type, device.index)
    buf = _BF_ROWS.get(key)
    if buf is None:
        buf = _BF_ROWS[key] = torch.zeros((B, C, Tp), device=device, dtype=torch.int16)
    return buf


def conv1d_cvt_bf16(x, out):
    """out (B, C, Tp) int16 <- bf16(x) for a (B, C, T) fp32 tensor or channel-slice view."""
    B, C, T = x.shape
    xp, xb = vptr(x)
    _hip.check(_hip.lib().air_conv1d_cvt_bf16(xp, csz(xb), ci(B), ci(C), ci(T), dptr(out, torch.int16), stream()),
               "air_conv1d_cvt_bf16")
    return out


def _bf_view(t):
    """(pointer, batch stride in elements) of a (B, C, Tp) int16 copy or a channel-slice view of one."""
    if t is None:
        return ctypes.c_void_p(0), 0
    if t.dtype != torch.int16 or not t.is_cuda or t.stride(2) != 1 or t.stride(1) != t.shape[2]:
        raise _hip.AirError("bf16 operand copy must be a (B, C, Tp) int16 GPU tensor (or a channel slice of one)")
    return ctypes.c_void_p(t.data_ptr()), t.stride(0)


def conv1d_wgrad(x, dy, w_shape, dil=1, pad=0, out=None, bf16=False, x_bf=None, dy_bf=None):
    """x_bf / dy_bf (bf16 path only): operand copies the caller already holds (bf16_rows buffers filled by
    bn_bwd(dx_bf16=...) or conv1d_cvt_bf16), skipping the conversion pass inside."""
    Cout, Cin, K = w_shape
    B, _, T = x.shape
    dw = out if out is not None else torch.empty(tuple(w_shape), device=x.device, dtype=torch.float32)
    xp, xb = vptr(x)
    yp, yb = vptr(dy)
    d = AirConv1d(B, Cin, T, Cout, K, dil, pad, xb, yb)
    if bf16:
        wsb, nb = _c1d_bf16(d, x.device, 2)
        if wsb is not None:
            xfp, xfb = _bf_view(x_bf)
            yfp, yfb = _bf_view(dy_bf)
            _hip.check(_hip.lib().air_conv1d_wgrad_bf16_pre(ctypes.byref(d), xp, yp, xfp, csz(xfb), yfp, csz(yfb),
                                                            dptr(dw), dptr(wsb, torch.uint8), csz(nb), stream()),
                       "air_conv1d_wgrad_bf16_pre")
            return dw
    n = _hip.lib().air_conv1d_ws_bytes(ctypes.byref(d))
    ws = workspace(n, x.device)
    _hip.check(_hip.lib().air_conv1d_wgrad(ctypes.byref(d), xp, yp, dptr(dw), dptr(ws, torch.uint8),
                                           csz(n), stream()), "air_conv1d_wgrad")
    return dw


def add_strided(out, a, b=None, out_bf=None):
    """out = a (+ b) over (B, C, T) tensors / channel-slice views; out_bf: (B, C, Tp) int16 copy (or a channel slice
    of one) that also receives the result as bf16."""
    B, C, T = out.shape
    op, ob = vptr(out)
    ap, ab = vptr(a)
    bp, bb = vptr(b) if b is not None else (ctypes.c_void_p(0), 0)
    fp, fb = _bf_view(out_bf)
    _hip.check(_hip.lib().air_add_strided_ex(op, csz(ob), ap, csz(ab), bp, csz(bb), ci(B), ci(C), ci(T), fp, csz(fb),
                                             ci(out_bf.shape[2] if out_bf is not None else 0), stream()),
               "air_add_strided_ex")
    return out


def res2_bn_apply(x, scale, shift, y1, add=None, y2=None, y1_bf=None):
    """y1 (channel-slice view) = x*scale + shift; y2 (dense) = that + add (channel-slice view); y1_bf: channel slice
    of a (B, C, Tp) int16 copy that also receives y1 as bf16."""
    B, C, T = x.shape
    y1p, y1b = vptr(y1)
    ap, ab = vptr(add) if add is not None else (ctypes.c_void_p(0), 0)
    fp, fb = _bf_view(y1_bf)
    _hip.check(_hip.lib().air_res2_bn_apply_ex(dptr(x), ci(B), ci(C), ci(T), dptr(scale), dptr(shift), y1p, csz(y1b),
                                               ap, csz(ab), dptr(y2, allow_none=True), fp, csz(fb),
                                               ci(y1_bf.shape[2] if y1_bf is not None else 0), stream()),
               "air_res2_bn_apply_ex")
    return y2


def channel_sum(x, out=None):
    B, C, T = x.shape
    xp, xb = vptr(x)
    if out is None:
        out = torch.empty(C, device=x.device, dtype=torch.float32)
    n = _hip.lib().air_channel_sum_ws_bytes(ci(B), ci(C))
    ws = workspace(n, x.device)
    _hip.check(_hip.lib().air_channel_sum(xp, ci(B), ci(C), ci(T), csz(xb), dptr(out), dptr(ws, torch.uint8),
                                          csz(n), stream()), "air_channel_sum")
    return out


def row_stats(x, want_std=True, clamp_min=1e-4, mean_out=None, std_out=None):
    B, C, T = x.shape
    mean = mean_out if mean_out is not None else torch.empty((B, C), device=x.device, dtype=torch.float32)
    std = None
    if want_std:
        std = std_out if std_out is not None else torch.empty((B, C), device=x.device, dtype=torch.float32)
    _hip.check(_hip.lib().air_row_stats(dptr(x), ci(B), ci(C), ci(T), dptr(mean), dptr(std, allow_none=True),
                                        cf(clamp_min), stream()), "air_row_stats")
    return mean, std


def row_stats_bwd(x, mean, std, dmean, dstd, dx, accumulate=True, clamp_min=1e-4, relu_mask=False, rowsum=None,
                  dx_bf16=None):
    """dx (+)= gradient of the per-row mean / std statistics; relu_mask zeroes the result where x == 0;
    rowsum (B, C) receives the time sums of the result rows; dx_bf16 (bf16_rows buffer) its bf16 copy."""
    B, C, T = x.shape
    _hip.check(_hip.lib().air_row_stats_bwd_ex(dptr(x), ci(B), ci(C), ci(T), dptr(mean), dptr(std, allow_none=True),
                                               dptr(dmean, allow_none=True), dptr(dstd, allow_none=True),
                                               cf(clamp_min), dptr(dx), ci(1 if accumulate else 0),
                                               ci(1 if relu_mask else 0), dptr(rowsum, allow_none=True),
                                               dptr(dx_bf16, torch.int16, allow_none=True),
                                               ci(dx_bf16.shape[2] if dx_bf16 is not None else 0), stream()),
               "air_row_stats_bwd_ex")
    return dx


def row_sum(x):
    B, C, T = x.shape
    out = torch.empty((B, C), device=x.device, dtype=torch.float32)
    _hip.check(_hip.lib().air_row_sum(dptr(x), ci(B), ci(C), ci(T), dptr(out), stream()), "air_row_sum")
    return out


def relu_mask_(dx, y):
    _hip.check(_hip.lib().air_relu_mask(dptr(dx), dptr(y), csz(dx.numel()), stream()), "air_relu_mask")
    return dx


def se_scale_fwd(x, z, res, out, out_bf=None):
    """out = x * sigmoid(z[b][c]) + res; out_bf: channel slice of a (B, C', Tp) int16 copy that also receives it as bf16."""
    B, C, T = x.shape
    rp, rb = vptr(res)
    op, ob = vptr(out)
    fp, fb = _bf_view(out_bf)
    _hip.check(_hip.lib().air_se_scale_fwd_ex(dptr(x), dptr(z), rp, csz(rb), ci(B), ci(C), ci(T), op, csz(ob), fp,
                                              csz(fb), ci(out_bf.shape[2] if out_bf is not None else 0), stream()),
               "air_se_scale_fwd_ex")
    return out


def se_scale_bwd(x, z, dout):
    B, C, T = x.shape
    dp, db = vptr(dout)
    dx = torch.empty_like(x)
    dz = torch.empty_like(z)
    _hip.check(_hip.lib().air_se_scale_bwd(dptr(x), dptr(z), dp, csz(db), ci(B), ci(C), ci(T), dptr(dx),
                                           dptr(dz), stream()), "air_se_scale_bwd")
    return dx, dz


def asp_fwd(x, logits):
    """Overwrites ``logits`` with the softmax weights; returns (B, 2C) = [mu | sg]."""
    B, C, T = x.shape
    out = torch.empty((B, 2 * C), device=x.device, dtype=torch.float32)
    _hip.check(_hip.lib().air_asp_fwd(dptr(x), dptr(logits), ci(B), ci(C), ci(T), dptr(out), stream()),
               "air_asp_fwd")
    return out


def asp_bwd(x, w, out, dout, dx, accumulate=False, rowsum=None, dlogits_bf16=None):
    """Overwrites ``w`` with d(logits); writes / accumulates dx; rowsum (B, C) receives sum_t d(logits);
    dlogits_bf16 (bf16_rows buffer) the bf16 copy of d(logits)."""
    B, C, T = x.shape
    _hip.check(_hip.lib().air_asp_bwd_ex(dptr(x), dptr(w), ci(B), ci(C), ci(T), dptr(out), dptr(dout), dptr(dx),
                                         ci(1 if accumulate else 0), dptr(rowsum, allow_none=True),
                                         dptr(dlogits_bf16, torch.int16, allow_none=True),
                                         ci(dlogits_bf16.shape[2] if dlogits_bf16 is not None else 0), stream()),
               "air_asp_bwd_ex")
    return dx


def softmax_rows(logits):
    """softmax over dim 1 of (B, C) logits (generate_score.py:102) on the softmax / cross-entropy kernel."""
    B, C = logits.shape
    logits = logits.float().contiguous()
    probs = torch.empty_like(logits)
    labels = torch.zeros(B, dtype=torch.int64, device=logits.device)
    loss = torch.empty((), device=logits.device, dtype=torch.float32)
    correct = torch.empty((), device=logits.device, dtype=torch.int32)
    _hip.check(_hip.lib().air_softmax_ce_fwd(_hip.dptr(logits), _hip.dptr(labels, torch.int64), _hip.ci(B), _hip.ci(C),
                                             _hip.dptr(probs), _hip.dptr(loss), _hip.dptr(correct, torch.int32),
                                             _hip.stream()), "air_softmax_ce_fwd")
    return probs


# ---------------------------------------------------------------- evaluation metrics (csrc/eval_metrics.hip)
EVAL_MAX_TRIALS = 1 << 20
EVAL_MAX_GROUPS = 128
EVAL_RECORD_WORDS = 16  # air_eval_record as int32 words


def eval_workspace_bytes(n):
    """Bytes of scratch the evaluation-metric calls without groups need for n trials (ValueError beyond
    EVAL_MAX_TRIALS)."""
    n = int(n)
    if n < 1 or n > EVAL_MAX_TRIALS:
        raise ValueError("device metrics take 1 .. %d trials, got %d" % (EVAL_MAX_TRIALS, n))
    return int(_hip.lib().air_eval_workspace_bytes(ci(n)))


def eval_workspace_bytes_grouped(n, n_groups):
    """Bytes of scratch eval_det_min_grouped needs for n trials in n_groups groups (ValueError beyond EVAL_MAX_TRIALS /
    EVAL_MAX_GROUPS)."""
    n_groups = int(n_groups)
    if n_groups < 1 or n_groups > EVAL_MAX_GROUPS:
        raise ValueError("device metrics take 1 .. %d groups, got %d" % (EVAL_MAX_GROUPS, n_groups))
    eval_workspace_bytes(n)  # (the range of n)
    return int(_hip.lib().air_eval_workspace_bytes_grouped(ci(int(n)), ci(n_groups)))


def _eval_args(scores, labels, ws, records=None, groups=None, n_groups=0):
    """The checks of both eval_det_min calls: ``groups`` None and ``n_groups`` 0 for the one without groups."""
    if not (torch.is_tensor(scores) and torch.is_tensor(labels)):
        raise _hip.AirError("scores and labels must be GPU tensors (the HIP path has no CPU fallback)")
    if scores.dim() != 1 or labels.dim() != 1 or labels.numel() != scores.numel():
        raise ValueError("scores and labels must be 1-d and of one length, got %s and %s" % (
            tuple(scores.shape), tuple(labels.shape)))
    if labels.dtype not in (torch.int32, torch.int64):
        raise _hip.AirError("labels must be int32 or int64, got %s" % labels.dtype)
    n = scores.numel()
    if groups is not None:
        if not torch.is_tensor(groups) or groups.dim() != 1 or groups.numel() != n:
            raise ValueError("groups must be 1-d and as long as the scores")
        if groups.dtype not in (torch.int32, torch.int64):
            raise _hip.AirError("groups must be int32 or int64, got %s" % groups.dtype)
    need = eval_workspace_bytes(n) if groups is None else eval_workspace_bytes_grouped(n, n_groups)
    if ws.dtype != torch.uint8 or ws.numel() < need:
        raise ValueError("workspace must be a uint8 tensor of >= %d bytes (eval_workspace_bytes%s)" % (
            need, "" if groups is None else "_grouped"))
    words = (n_groups + 1) * EVAL_RECORD_WORDS
    if records is not None and (records.dtype != torch.int32 or records.numel() != words):
        raise ValueError("records must be %d int32 words" % words)
    return n


def eval_det_min(scores, labels, record, ws, negate=False, c1=None, c2=None):
    """EER point (and, with the fp64 weights c1, c2, the min t-DCF point) of the DET curve of ``scores`` (fp32, (n,))
    and ``labels`` (int32 | int64, 0 = bona fide) into ``record`` (EVAL_RECORD_WORDS int32: air_eval_record), using the
    uint8 scratch ``ws``.  Enqueues only: nothing is allocated or synchronised."""
    n = _eval_args(scores, labels, ws, record)
    want = c1 is not None
    _hip.check(_hip.lib().air_eval_det_min(
        dptr(scores), dptr(labels, labels.dtype), ci(labels.element_size()), ci(n), ci(1 if negate else 0),
        ci(1 if want else 0), ctypes.c_double(c1 if want else 1.0), ctypes.c_double(c2 if want else 1.0),
        dptr(record, torch.int32), dptr(ws, torch.uint8), csz(ws.numel()), stream()), "air_eval_det_min")
    return record


def eval_det_min_grouped(scores, labels, groups, n_groups, records, ws, negate=False, c12=None):
    """eval_det_min for the pooled trials and for each of ``n_groups`` groups from ONE sort: ``groups`` (int32 | int64,
    (n,)) holds each trial's group, -1 = member of every group; ``records`` ((n_groups + 1) * EVAL_RECORD_WORDS int32)
    gets the pooled record and one per group, each what eval_det_min writes for that subset alone.  ``c12``: fp64
    (n_groups + 1, 2) GPU tensor of the t-DCF weights (C1, C2) per record, or None.  Ids outside -1 .. n_groups - 1
    are counted into reserved[0] of the pooled record.  Enqueues only: nothing is allocated or synchronised."""
    if groups is None:
        raise ValueError("groups must be 1-d and as long as the scores")
    n_groups = int(n_groups)
    n = _eval_args(scores, labels, ws, records, groups, n_groups)
    if c12 is not None and (c12.dtype != torch.float64 or c12.numel() != 2 * (n_groups + 1)):
        raise ValueError("c12 must be fp64 of shape (%d, 2)" % (n_groups + 1))
    _hip.check(_hip.lib().air_eval_det_min_grouped(
        dptr(scores), dptr(labels, labels.dtype), ci(labels.element_size()), dptr(groups, groups.dtype),
        ci(groups.element_size()), ci(n), ci(n_groups), ci(1 if negate else 0), ci(0 if c12 is None else 1),
        dptr(c12, torch.float64, allow_none=True), dptr(records, torch.int32), dptr(ws, torch.uint8), csz(ws.numel()),
        stream()), "air_eval_det_min_grouped")
    return records


def eval_sorted_keys(scores, labels, negate=False):
    """The n sorted composite keys ((ordered image of the score) << 9 | is_spoof << 8, no group code) as an int64 GPU
    tensor - the first two steps of eval_det_min, for tests of the sort."""
    ws = torch.empty(eval_workspace_bytes(scores.numel()), dtype=torch.uint8, device=scores.device)
    n = _eval_args(scores, labels, ws)
    L = _hip.lib()
    _hip.check(L.air_eval_keys(dptr(scores), dptr(labels, labels.dtype), ci(labels.element_size()), ci(n),
                               ci(1 if negate else 0), dptr(ws, torch.uint8), csz(ws.numel()), stream()), "air_eval_keys")
    _hip.check(L.air_eval_sort_keys(ci(n), dptr(ws, torch.uint8), csz(ws.numel()), stream()), "air_eval_sort_keys")
    return ws[:n * 8].view(torch.int64).clone()


# ---------------------------------------------------------------- score fusion (csrc/score_fusion.hip)
SCORE_FUSE_MODES = {"sum": 0, "mean": 1}


def score_fuse_max_systems():
    return int(_hip.lib().air_score_fuse_max_systems())


def score_fuse(scores, index=None, weights=None, mode="sum", out=None, n_present=None):
    """The fusion of K systems' scores (air_score_fuse): ``scores`` fp32 (K, L) on the GPU, rows of unit stride (the
    row stride may exceed L: rows of a wider buffer); ``index`` None - trial n is column n, N = L - or int32 (K, N), the
    position of trial n in row k, negative = absent (positions >= L are made absent by one elementwise launch before the
    kernel: nothing outside a row is read); ``weights`` None or fp32 (K,) on the GPU; ``mode`` "sum" (avg_fuse) or
    "mean" over the systems that have the trial (weighted_fuse).  Returns the fused fp32 (N,) tensor (``out``);
    ``n_present``: optional int32 (N,) that gets the number of terms per trial (0: the trial's score is NaN).
    Enqueues only: nothing is synchronised."""
    if not torch.is_tensor(scores) or not scores.is_cuda:
        raise _hip.AirError("scores must be a GPU tensor (the HIP path has no CPU fallback)")
    if mode not in SCORE_FUSE_MODES:
        raise ValueError("mode must be 'sum' or 'mean', got %r" % (mode,))
    if scores.dim() != 2 or scores.dtype != torch.float32:
        raise ValueError("scores must be fp32 of shape (K, L), got %s %s" % (scores.dtype, tuple(scores.shape)))
    K, L = scores.shape
    if K < 1 or K > score_fuse_max_systems():
        raise ValueError("score fusion takes 1 .. %d systems, got %d" % (score_fuse_max_systems(), K))
    if L > 0 and (scores.stride(1) != 1 or (K > 1 and scores.stride(0) < L)):
        scores = scores.contiguous()
    N = L
    if index is not None:
        if not torch.is_tensor(index) or not index.is_cuda or index.dtype != torch.int32 or index.dim() != 2 or index.shape[0] != K:
            raise ValueError("index must be an int32 GPU tensor of shape (%d, N)" % K)
        N = index.shape[1]
        index = torch.where(index < L, index, -1).contiguous()
    if weights is not None and (not torch.is_tensor(weights) or weights.numel() != K):
        raise ValueError("weights must be %d fp32 values on the GPU" % K)
    if out is None:
        out = torch.empty(N, dtype=torch.float32, device=scores.device)
    elif out.dim() != 1 or out.numel() != N:
        raise ValueError("out must be fp32 of shape (%d,)" % N)
    if n_present is not None and (n_present.dim() != 1 or n_present.numel() != N):
        raise ValueError("n_present must be int32 of shape (%d,)" % N)
    if N == 0:
        return out
    if L == 0:
        raise ValueError("the rows of scores are empty")
    _hip.check(_hip.lib().air_score_fuse(
        ctypes.c_void_p(scores.data_ptr()), ctypes.c_int64(scores.stride(0) if K > 1 else L),
        dptr(index, torch.int32, allow_none=True), dptr(weights, torch.float32, allow_none=True), ci(K), ctypes.c_int64(N),
        ci(SCORE_FUSE_MODES[mode]), dptr(out), dptr(n_present, torch.int32, allow_none=True), stream()), "air_score_fuse")
    return out


# ---------------------------------------------------------------- device corpus (csrc/corpus.hip)
CORPUS_ALIGN = 8                # every utterance of a store starts at a multiple of this many elements
CORPUS_KIND_CROP = 2            # stream = (generation << 2) | kind; kinds 0 and 1: the flows' permutations
CORPUS_MAX_GENERATION = (1 << 30) - 1
CORPUS_DTYPES = (torch.int16, torch.float32)


def corpus_copy_tile(dtype):
    """Elements one workgroup of the ragged row copy moves (the tile boundary of air_corpus_copy_rows)."""
    return int(_hip.lib().air_corpus_copy_tile(ci(torch.empty(0, dtype=dtype).element_size())))


def corpus_stream(generation, kind):
    generation, kind = int(generation), int(kind)
    if generation < 0 or generation > CORPUS_MAX_GENERATION or kind not in (0, 1, CORPUS_KIND_CROP):
        raise ValueError("stream of generation %d, kind %d" % (generation, kind))
    return (generation << 2) | kind


def corpus_permutation_ws_bytes(n):
    return eval_workspace_bytes(n)


def corpus_permutation(lo, n, seed, stream_id, out=None, ws=None):
    """The permutation of [lo, lo + n) that (seed, stream_id) names (air_corpus_permutation), as an int64 (n,) GPU tensor
    (``out``).  ValueError beyond EVAL_MAX_TRIALS.  Enqueues only; the scratch is ``ws`` (uint8, at least
    corpus_permutation_ws_bytes(n)) or the stream's workspace."""
    lo, n = int(lo), int(n)
    if n < 1 or n > EVAL_MAX_TRIALS:
        raise ValueError("a permutation takes 1 .. %d elements, got %d" % (EVAL_MAX_TRIALS, n))
    if lo < 0:
        raise ValueError("lo must not be negative, got %d" % lo)
    if out is None:
        out = torch.empty(n, dtype=torch.int64, device="cuda")
    elif out.dim() != 1 or out.numel() != n:
        raise ValueError("out must be int64 of shape (%d,)" % n)
    L = _hip.lib()
    need = int(L.air_corpus_permutation_ws_bytes(ci(n)))
    if ws is None:
        ws = workspace(need, out.device)
    elif ws.dtype != torch.uint8 or ws.numel() < need:
        raise ValueError("workspace must be a uint8 tensor of >= %d bytes (corpus_permutation_ws_bytes)" % need)
    _hip.check(L.air_corpus_permutation(ctypes.c_int64(lo), ci(n), ctypes.c_uint64(int(seed) & 0xFFFFFFFFFFFFFFFF),
                                        ctypes.c_uint32(int(stream_id) & 0xFFFFFFFF), dptr(out, torch.int64),
                                        dptr(ws, torch.uint8), csz(ws.numel()), stream()), "air_corpus_permutation")
    return out


def corpus_copy_rows(src, dst, lengths, max_len, src_off=None, src_stride=0, dst_off=None, dst_stride=0, dst_cap=0):
    """air_corpus_copy_rows over 1-d or 2-d GPU tensors of one dtype (int16 | float32): row r moves
    min(lengths[r], max_len) elements from ``src_off[r]`` (or r * src_stride) to ``dst_off[r]`` (or r * dst_stride);
    ``dst_cap``: zeros in [length, dst_cap).  ``lengths`` int32, the offsets int64, all on the GPU.  The CALLER vouches
    that every row lies inside both tensors: the rows' extents are device data."""
    if src.dtype != dst.dtype or src.dtype not in CORPUS_DTYPES:
        raise _hip.AirError("corpus rows are int16 or float32 on both sides, got %s -> %s" % (src.dtype, dst.dtype))
    rows = int(lengths.numel())
    for off in (src_off, dst_off):
        if off is not None and off.numel() != rows:
            raise ValueError("one offset per row")
    _hip.check(_hip.lib().air_corpus_copy_rows(
        dptr(src, src.dtype), dptr(src_off, torch.int64, allow_none=True), ctypes.c_int64(int(src_stride)),
        dptr(dst, dst.dtype), dptr(dst_off, torch.int64, allow_none=True), ctypes.c_int64(int(dst_stride)),
        dptr(lengths, torch.int32), ci(rows), ci(int(max_len)), ci(int(dst_cap)), ci(src.element_size()), stream()),
        "air_corpus_copy_rows")
    return dst


def corpus_gather(samples, offsets, lengths, labels, tags, index, channels, n, segments, seed, feat_len, hop, Lcap,
                  pcm=None):
    """One batch out of a store (air_corpus_gather).  ``samples``: the flat int16 | float32 store; ``offsets`` (int64),
    ``lengths`` (int32), ``labels`` / ``tags`` / ``index`` (int64) and ``channels`` ((n, C) int64 or None): its tables,
    of which the first ``n`` entries are read.  ``segments``: one or two ``(perm, first, count, generation)`` - ``perm``
    an int64 GPU tensor or None (the identity), of which rows [first, first + count) are drawn.  Returns freshly
    allocated (pcm (B, Lcap), labels, start, lengths, tags, channels | None, index); ``pcm``: a contiguous (B, Lcap)
    tensor of the store's dtype to write the samples into instead of a fresh one.  Enqueues only."""
    if samples.dtype not in CORPUS_DTYPES:
        raise _hip.AirError("a store is int16 or float32, got %s" % samples.dtype)
    n, Lcap = int(n), int(Lcap)
    if Lcap < CORPUS_ALIGN or Lcap % CORPUS_ALIGN:
        raise ValueError("Lcap must be a positive multiple of %d, got %d" % (CORPUS_ALIGN, Lcap))
    if not 1 <= len(segments) <= 2:
        raise ValueError("a batch has one or two segments")
    for t in (offsets, lengths, labels, tags, index):
        if t.numel() < n:
            raise ValueError("a table of the store holds fewer than n = %d entries" % n)
    C = 0
    if channels is not None:
        C = int(channels.shape[1])
        if channels.dim() != 2 or channels.shape[0] < n or C < 1:
            raise ValueError("channels must be (>= n, C)")
    segs = (_hip.AirCorpusSegment * 2)()
    B = 0
    for k, (perm, first, count, generation) in enumerate(segments):
        first, count = int(first), int(count)
        if count < 0 or first < 0 or first + count > (n if perm is None else perm.numel()):
            raise ValueError("segment %d draws rows [%d, %d) of %d" % (k, first, first + count,
                                                                      n if perm is None else perm.numel()))
        corpus_stream(generation, CORPUS_KIND_CROP)
        segs[k].perm = perm.data_ptr() if perm is not None else None
        if perm is not None:
            dptr(perm, torch.int64)
        segs[k].first, segs[k].count, segs[k].generation = first, count, int(generation)
        B += count
    if B < 1:
        raise ValueError("an empty batch")
    dev = samples.device
    view = _hip.AirCorpusView(samples.data_ptr(), dptr(offsets, torch.int64).value, dptr(lengths, torch.int32).value,
                              dptr(labels, torch.int64).value, dptr(tags, torch.int64).value,
                              dptr(index, torch.int64).value,
                              dptr(channels, torch.int64).value if channels is not None else None, n, C,
                              samples.element_size())
    if pcm is None:
        pcm = torch.empty((B, Lcap), dtype=samples.dtype, device=dev)
    elif tuple(pcm.shape) != (B, Lcap) or pcm.dtype != samples.dtype:
        raise ValueError("pcm must be a (%d, %d) %s tensor" % (B, Lcap, samples.dtype))
    o_len = torch.empty(B, dtype=torch.int32, device=dev)
    o_start = torch.empty(B, dtype=torch.int32, device=dev)
    o_lab = torch.empty(B, dtype=torch.int64, device=dev)
    o_tag = torch.empty(B, dtype=torch.int64, device=dev)
    o_idx = torch.empty(B, dtype=torch.int64, device=dev)
    o_ch = torch.empty((B, C), dtype=torch.int64, device=dev) if channels is not None else None
    _hip.check(_hip.lib().air_corpus_gather(
        ctypes.byref(view), segs, ci(len(segments)), ctypes.c_uint64(int(seed) & 0xFFFFFFFFFFFFFFFF), ci(int(feat_len)),
        ci(int(hop)), ci(Lcap), dptr(pcm, pcm.dtype), dptr(o_len, torch.int32), dptr(o_lab, torch.int64),
        dptr(o_tag, torch.int64), dptr(o_ch, torch.int64, allow_none=True), dptr(o_idx, torch.int64),
        dptr(o_start, torch.int32), stream()), "air_corpus_gather")
    return pcm, o_lab, o_start, o_len, o_tag, o_ch, o_idx


# ---------------------------------------------------------------- embedding projections (csrc/embed_vis.hip)
TSNE_STATUS_BYTES = 64  # air_tsne_status
TSNE_STATUS_DTYPE = [("stopped", "<i4"), ("reason", "<i4"), ("n_iter", "<i4"), ("best_iter", "<i4"),
                     ("best_error", "<f8"), ("kl", "<f8"), ("grad_norm", "<f8"), ("pad", "<f8", (3,))]


def vis_limits():
    """(largest N, largest D, most principal components) the projection kernels take."""
    L = _hip.lib()
    return int(L.air_vis_max_n()), int(L.air_vis_max_d()), int(L.air_pca_max_components())


def _vis_matrix(x, what, cols=None):
    if not torch.is_tensor(x) or not x.is_cuda:
        raise _hip.AirError("%s must be a GPU tensor (the HIP path has no CPU fallback)" % what)
    if x.dim() != 2 or x.dtype != torch.float32 or (cols is not None and x.shape[1] != cols):
        raise ValueError("%s must be fp32 of shape (N, %s), got %s %s" % (what, cols or "D", x.dtype, tuple(x.shape)))
    return x.contiguous()


def _vis_ws(nbytes, device, what):
    if nbytes == 0:
        raise _hip.AirError("%s: AIR_EUNSUPPORTED (2 <= N <= %d, D <= %d)" % ((what,) + vis_limits()[:2]))
    return torch.empty(nbytes, dtype=torch.uint8, device=device)


def pca_ws_bytes(n, d):
    return int(_hip.lib().air_pca_ws_bytes(ci(int(n)), ci(int(d))))


def tsne_ws_bytes(n):
    return int(_hip.lib().air_tsne_ws_bytes(ci(int(n))))


def pca_gram(x, ws=None):
    """(mean fp32 (D,), centred Gram matrix fp64 (D, D)) of ``x`` fp32 (N, D) on the GPU (air_pca_gram)."""
    x = _vis_matrix(x, "x")
    N, D = x.shape
    if ws is None:
        ws = _vis_ws(pca_ws_bytes(N, D), x.device, "air_pca_gram")
    mean = torch.empty(D, dtype=torch.float32, device=x.device)
    gram = torch.empty(D, D, dtype=torch.float64, device=x.device)
    _hip.check(_hip.lib().air_pca_gram(dptr(x), ci(N), ci(D), dptr(mean), dptr(gram, torch.float64), dptr(ws, torch.uint8),
                                       csz(ws.numel()), stream()), "air_pca_gram")
    return mean, gram


def pca_project(x, mean, comps):
    """(x - mean) comps^T as fp32 (N, K): ``comps`` fp32 (K, D) on the GPU (air_pca_project)."""
    x = _vis_matrix(x, "x")
    N, D = x.shape
    comps = _vis_matrix(comps, "comps", D)
    K = comps.shape[0]
    if mean.numel() != D:
        raise ValueError("mean must hold %d values" % D)
    out = torch.empty(N, K, dtype=torch.float32, device=x.device)
    _hip.check(_hip.lib().air_pca_project(dptr(x), ci(N), ci(D), dptr(mean), dptr(comps), ci(K), dptr(out), stream()),
               "air_pca_project")
    return out


def pairwise_sqdist(x, out=None):
    """Dense (N, N) fp32 squared Euclidean distances of the rows of ``x`` fp32 (N, D), summed as (x_i - x_j)^2."""
    x = _vis_matrix(x, "x")
    N, D = x.shape
    if out is None:
        out = torch.empty(N, N, dtype=torch.float32, device=x.device)
    elif tuple(out.shape) != (N, N):
        raise ValueError("out must be fp32 of shape (%d, %d)" % (N, N))
    _hip.check(_hip.lib().air_pairwise_sqdist(dptr(x), ci(N), ci(D), dptr(out), stream()), "air_pairwise_sqdist")
    return out


def tsne_affinities(dist, perplexity, out=None):
    """scikit-learn's _binary_search_perplexity over ``dist`` fp32 (N, N): (conditional P fp32 (N, N), beta fp32 (N,))."""
    dist = _vis_matrix(dist, "dist")
    N = dist.shape[0]
    if dist.shape[1] != N:
        raise ValueError("dist must be square, got %s" % (tuple(dist.shape),))
    if out is None:
        out = torch.empty(N, N, dtype=torch.float32, device=dist.device)
    elif tuple(out.shape) != (N, N) or out.data_ptr() == dist.data_ptr():
        raise ValueError("out must be another fp32 tensor of shape (%d, %d)" % (N, N))
    beta = torch.empty(N, dtype=torch.float32, device=dist.device)
    _hip.check(_hip.lib().air_tsne_affinities(dptr(dist), ci(N), cf(float(perplexity)), dptr(out), dptr(beta), stream()),
               "air_tsne_affinities")
    return out, beta


def _tsne_ws(N, device, ws, what):
    if ws is None:
        return _vis_ws(tsne_ws_bytes(N), device, what)
    return ws


def tsne_joint(cond, ws=None):
    """The joint distribution of the conditional ``cond`` fp32 (N, N), IN PLACE (air_tsne_joint); returns ``cond``."""
    if not torch.is_tensor(cond) or not cond.is_cuda:
        raise _hip.AirError("cond must be a GPU tensor (the HIP path has no CPU fallback)")
    N = cond.shape[0]
    if cond.dim() != 2 or cond.shape[1] != N or cond.dtype != torch.float32 or not cond.is_contiguous():
        raise ValueError("cond must be a contiguous fp32 (N, N) tensor")
    ws = _tsne_ws(N, cond.device, ws, "air_tsne_joint")
    _hip.check(_hip.lib().air_tsne_joint(dptr(cond), ci(N), dptr(ws, torch.uint8), csz(ws.numel()), stream()), "air_tsne_joint")
    return cond


def tsne_new_status(device):
    """A device status record (air_tsne_status) that says "running" with no best error yet."""
    import numpy as np
    rec = np.zeros(1, dtype=TSNE_STATUS_DTYPE)
    rec["best_error"] = np.finfo(np.float64).max
    rec["kl"] = rec["grad_norm"] = np.nan
    return torch.from_numpy(rec.view(np.uint8).copy()).to(device)


def tsne_read_status(status):
    """The status record on the host, as a dict (one device-to-host copy)."""
    rec = status.cpu().numpy().view(TSNE_STATUS_DTYPE)[0]
    return {k: rec[k].item() for k in ("stopped", "reason", "n_iter", "best_iter", "best_error", "kl", "grad_norm")}


def tsne_gradient_kl(P, y, exaggeration=1.0, ws=None):
    """(grad fp32 (N, 2), KL as a device fp64 scalar inside the returned status record) of _kl_divergence at the
    embedding ``y`` for the joint ``P``: air_tsne_pairs with the KL pass, air_tsne_gradient, air_tsne_check without rules.
    Returns (grad, status): ``tsne_read_status(status)["kl"]``."""
    P = _vis_matrix(P, "P")
    N = P.shape[0]
    y = _vis_matrix(y, "y", 2)
    if P.shape[1] != N or y.shape[0] != N:
        raise ValueError("P must be (N, N) and y (N, 2)")
    ws = _tsne_ws(N, P.device, ws, "air_tsne_pairs")
    status = tsne_new_status(P.device)
    grad = torch.empty(N, 2, dtype=torch.float32, device=P.device)
    L = _hip.lib()
    wsp, wsn = dptr(ws, torch.uint8), csz(ws.numel())
    _hip.check(L.air_tsne_pairs(dptr(P), dptr(y), ci(N), cf(float(exaggeration)), ci(1), dptr(status, torch.uint8), wsp, wsn,
                                stream()), "air_tsne_pairs")
    _hip.check(L.air_tsne_gradient(ci(N), dptr(grad), wsp, wsn, stream()), "air_tsne_gradient")
    # (the check kernel sums the norm partials an update leaves: a step of zero length on a scratch embedding writes them)
    scratch = y.clone()
    upd, gains = torch.zeros_like(y), torch.ones_like(y)
    _hip.check(L.air_tsne_update(dptr(scratch), dptr(upd), dptr(gains), ci(N), cf(0.0), cf(0.0), dptr(status, torch.uint8),
                                 wsp, wsn, stream()), "air_tsne_update")
    _hip.check(L.air_tsne_check(ci(N), ci(0), ci(1), ci(0), ci(0), ctypes.c_double(0.0), dptr(status, torch.uint8), wsp, wsn,
                                stream()), "air_tsne_check")
    return grad, status


def tsne_run(P, y, update, gains, status, max_iter=1000, exploration_iter=250, n_iter_check=50,
             n_iter_without_progress=300, min_grad_norm=1e-7, learning_rate=200.0, early_exaggeration=12.0, ws=None):
    """Enqueue the whole descent (air_tsne_run) on the joint ``P`` fp32 (N, N): ``y``, ``update``, ``gains`` fp32 (N, 2)
    are advanced in place (update and gains are initialised by the call), ``status`` (TSNE_STATUS_BYTES uint8 on the
    GPU) gets the record.  Nothing is synchronised."""
    P = _vis_matrix(P, "P")
    N = P.shape[0]
    for t, name in ((y, "y"), (update, "update"), (gains, "gains")):
        if not torch.is_tensor(t) or not t.is_cuda:
            raise _hip.AirError("%s must be a GPU tensor (the HIP path has no CPU fallback)" % name)
        if tuple(t.shape) != (N, 2) or t.dtype != torch.float32 or not t.is_contiguous():
            raise ValueError("%s must be a contiguous fp32 (%d, 2) tensor" % (name, N))
    if P.shape[1] != N:
        raise ValueError("P must be square")
    if status.dtype != torch.uint8 or status.numel() != TSNE_STATUS_BYTES:
        raise ValueError("status must be %d uint8" % TSNE_STATUS_BYTES)
    ws = _tsne_ws(N, P.device, ws, "air_tsne_run")
    sched = _hip.AirTsneSchedule(int(max_iter), int(exploration_iter), int(n_iter_check), int(n_iter_without_progress),
                                 float(learning_rate), float(early_exaggeration), float(min_grad_norm))
    _hip.check(_hip.lib().air_tsne_run(dptr(P), dptr(y), dptr(update), dptr(gains), ci(N), ctypes.byref(sched),
                                       dptr(status, torch.uint8), dptr(ws, torch.uint8), csz(ws.numel()), stream()),
               "air_tsne_run")
    return status


# BatchNorm's num_batches_tracked counters: one multi-tensor add per forward instead of one 4 us ATen launch per
# layer (34 per ECAPA step).  bn_tick() queues a counter, bn_flush() adds 1 to everything queued since the last flush.
_TICKS = []


def bn_tick(counter):
    _TICKS.append(counter)


def bn_flush():
    if _TICKS:
        torch._foreach_add_(_TICKS, 1)
        del _TICKS[:]


class ClockProbe:
    """Core clock of the GPU WHILE other kernels run (air_debug_clock_probe): one wave on a side stream samples
    {wall clock, core-clock counter} every ``interval_us``; ``mhz()`` after the measured work has been synchronised.
    Measurement instrumentation (bench.py "core_clock"), not part of the training path."""

    def __init__(self, device, n_samples=2000, interval_us=50.0):
        self.n = int(n_samples)
        self.buf = torch.zeros(2 * self.n, dtype=torch.int64, device=device)
        self.side = torch.cuda.Stream(device=device)
        self.interval_us = float(interval_us)

    def start(self):
        self.buf.zero_()
        torch.cuda.current_stream(self.buf.device).synchronize()
        _hip.check(_hip.lib().air_debug_clock_probe(ctypes.c_void_p(self.buf.data_ptr()), ci(self.n),
                                                    ctypes.c_double(self.interval_us),
                                                    ctypes.c_void_p(self.side.cuda_stream)), "air_debug_clock_probe")

    def samples(self):
        """(t_us, mhz) per sampling interval, after the probe has finished."""
        self.side.synchronize()
        raw = self.buf.cpu().numpy().reshape(self.n, 2)
        ok = raw[:, 0] > 0
        raw = raw[ok]
        dw = (raw[1:, 0] - raw[:-1, 0]).astype("float64")
        dc = (raw[1:, 1] - raw[:-1, 1]).astype("float64")
        keep = dw > 0
        t = (raw[1:, 0] - raw[0, 0])[keep] / 100.0
        return t, dc[keep] / dw[keep] * 100.0

    def mhz(self, t_lo_us=None, t_hi_us=None):
        """Median / min / max core clock over the samples whose time since the probe's start lies in [t_lo, t_hi]."""
        import numpy as np
        t, f = self.samples()
        if t_lo_us is not None:
            sel = (t >= t_lo_us) & (t <= t_hi_us)
            f = f[sel]
        if f.size == 0:
            return None
        return {"median": round(float(np.median(f)), 1), "min": round(float(f.min()), 1), "max": round(float(f.max()), 1),
                "samples": int(f.size), "interval_us": self.interval_us}

