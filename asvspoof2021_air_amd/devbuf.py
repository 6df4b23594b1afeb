"""A 1-d device buffer that a pass appends to without the host ever waiting: every append is a device-side copy at an
offset the host knows from the shapes, and a full buffer is doubled by one more device-side copy.  The dev / eval pass
(train.Trainer.evaluate) and end-synchronised scoring (generate_score.test_on_dataset(sync="end")) collect their
per-batch results in these instead of one ``.item()`` / ``.cpu()`` per batch (main_train.py:526-575,
generate_score.py:113-119)."""
import torch


class DeviceVector:
    def __init__(self, dtype, device, capacity=0):
        self.buf = torch.empty(max(int(capacity), 1), dtype=dtype, device=device)
        self.n = 0

    def append(self, t):
        """Copy the elements of the device tensor ``t`` (any shape, cast to the buffer's dtype) behind what is held."""
        t = t.reshape(-1)
        end = self.n + t.numel()
        if end > self.buf.numel():
            grown = torch.empty(max(end, 2 * self.buf.numel()), dtype=self.buf.dtype, device=self.buf.device)
            grown[:self.n].copy_(self.buf[:self.n])
            self.buf = grown
        self.buf[self.n:end].copy_(t, non_blocking=True)
        self.n = end

    def view(self):
        return self.buf[:self.n]
