"""What the stages between a file on disk and a ragged PCM batch on the device share on the host: the row capacity, the
``lengths`` check, the (fp32, int16) pointer pair of the kernels' entry points, the decoders' rings of output tensors and
their row status, and the pinned staging of what the host uploads per batch.  Imports ``_hip`` and ``torch`` only.
"""
import ctypes

import torch

from . import _hip

RAGGED_ROUND = 16000  # the default row capacity is the longest row rounded up to this
_NULL = ctypes.c_void_p(0)


def round_capacity(longest):
    """The default capacity of a batch whose longest row holds ``longest`` samples."""
    return -(-max(1, int(longest)) // RAGGED_ROUND) * RAGGED_ROUND


def device_lengths(lengths, B, Lcap, device, non_blocking=False, extra_check=None):
    """``lengths`` as the int32 (B,) device tensor the ragged kernels read: a GPU tensor is used as is (the kernels clamp
    it to [1, Lcap]), a host tensor or sequence is checked (ValueError; then ``extra_check(host, Lcap)``) and uploaded."""
    if not (torch.is_tensor(lengths) and lengths.is_cuda):
        host = torch.as_tensor(lengths).reshape(-1)
        if host.numel() != B or host.is_floating_point() or host.dtype == torch.bool:
            raise ValueError("lengths must be %d integers, got %s %s" % (B, tuple(host.shape), host.dtype))
        if B and (int(host.min()) < 1 or int(host.max()) > Lcap):
            raise ValueError("lengths must lie in [1, %d] (the row capacity), got [%d, %d]" % (
                Lcap, int(host.min()), int(host.max())))
        if extra_check is not None:
            extra_check(host, Lcap)
        lengths = host.to(torch.int32).to(device, non_blocking=non_blocking)
    elif lengths.numel() != B:
        raise ValueError("lengths must have %d entries, got %d" % (B, lengths.numel()))
    return lengths.to(torch.int32).contiguous()  # (no-op for what the dataset hands over)


def pcm_pointers(src):
    """(fp32 pointer, int16 pointer) of a contiguous float32 or int16 GPU tensor, the other one NULL: the argument pair
    every ragged entry point takes."""
    if src.dtype == torch.int16:
        return _NULL, _hip.dptr(src, torch.int16)
    return _hip.dptr(src), _NULL


class DeviceRing:
    """Output, status and workspace tensors out of a ring of ``depth`` slots per key: a replayed step sees stable
    addresses, and a result stays valid until ``depth - 1`` further calls of the same shape."""

    def __init__(self, device, depth):
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise _hip.AirError("%s runs on the GPU (the HIP path has no CPU fallback)" % type(self).__name__)
        self.depth = max(1, int(depth))
        self._ring, self._next = {}, {}

    def _slot(self, key, make):
        ring = self._ring.setdefault(key, [])
        j = self._next.get(key, 0)
        self._next[key] = (j + 1) % self.depth
        if j >= len(ring):
            ring.append(make())
        return ring[j]

    def _output(self, B, Lcap, dtype, out):
        """-> (pcm (B, Lcap) ``dtype`` - ``out`` or the ring's -, status (B,) int32, int16 pointer, fp32 pointer)."""
        if dtype not in (torch.int16, torch.float32):
            raise ValueError("dtype is torch.int16 or torch.float32")
        if out is not None:
            if tuple(out.shape) != (B, Lcap) or out.dtype != dtype or not out.is_contiguous():
                raise ValueError("out must be a contiguous (%d, %d) %s tensor" % (B, Lcap, dtype))
            pcm = out
        else:
            pcm = self._slot(("pcm", B, Lcap, dtype), lambda: torch.empty((B, Lcap), dtype=dtype, device=self.device))
        status = self._slot(("status", B), lambda: torch.empty(B, dtype=torch.int32, device=self.device))
        p32, p16 = pcm_pointers(pcm)
        return pcm, status, p16, p32


def check_status(status, ok, error):
    """Copy ``status`` to the host (synchronises) and raise ``error([(row, code), ...])`` for the rows that are not ``ok``."""
    bad = [(r, c) for r, c in enumerate(status.detach().cpu().reshape(-1).tolist()) if c != ok]
    if bad:
        raise error(bad)


class PinnedRing:
    """Pinned host buffers out of a ring of ``depth`` per key: allocating pinned memory per batch cost ~20 ms of host
    time per 16 MB batch (the from-dataset bench leg was host-bound at 0.48 of the resident rate).  A buffer stays valid
    until ``depth - 1`` further ``take``s of its key; ``DevicePrefetcher`` stores the event of the copy it issued from a
    buffer through its ``_air_ring`` tag, and a slot is reused only behind that event (normally long done)."""

    def __init__(self, depth):
        self.depth = int(depth)
        self._slots = {}

    def take(self, key, shape, dtype):
        if not torch.cuda.is_available():
            return torch.empty(shape, dtype=dtype)
        slot = self._slots.get(key)
        if slot is None:
            slot = self._slots[key] = {"bufs": [None] * self.depth, "events": [None] * self.depth, "next": 0}
        j = slot["next"]
        slot["next"] = (j + 1) % self.depth
        if slot["bufs"][j] is None:
            slot["bufs"][j] = torch.empty(shape, dtype=dtype, pin_memory=True)
        ev = slot["events"][j]
        if ev is not None:
            ev.synchronize()
            slot["events"][j] = None
        buf = slot["bufs"][j]
        buf._air_ring = (slot["events"], j)  # (the events list, not the slot: the slot holds the buffer - no reference cycle)
        return buf


class PinnedUpload:
    """``upload(host_array, device)`` of an instance: the asynchronous copy of a small numpy array from a pinned buffer
    kept per (shape, dtype) - a pageable ``.to(device)`` would synchronise the stream and drain the step's launch queue
    (measured: ~1 ms per step)."""

    def __init__(self):
        self._slots = {}

    def __call__(self, host, device):
        src = torch.from_numpy(host)
        key = (tuple(src.shape), src.dtype)
        slot = self._slots.get(key)
        if slot is None:
            slot = self._slots[key] = [torch.empty(src.shape, dtype=src.dtype).pin_memory(), None]
        if slot[1] is not None:
            slot[1].synchronize()  # the previous upload from this buffer has executed (one step of run-ahead)
        slot[0].copy_(src)
        dev = slot[0].to(device, non_blocking=True)
        slot[1] = torch.cuda.Event()
        slot[1].record()
        return dev
