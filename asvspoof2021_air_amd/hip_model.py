"""What every HIP-sequenced model owes autograd, train.Trainer, dist, optim and torch.save, written once.

A model file (resnet.py, ecapa_tdnn.py, lcnn.py, res2net.py) sequences kernels; ``HipModel`` is how that sequence
meets the rest: ONE ``torch.autograd.Function`` spans the model (``loss.backward()`` works as in main_train.py:406
while the per-layer bookkeeping stays out of the autograd engine), the parameters and gradients live in flat arenas
(arena.py), the gradient all-reduce may leave from inside backward (dist.GradBucketer), train.Trainer captures the
step through ``forward_saved`` / ``backward_saved``, and a whole-module pickle (main_train.py:675-704 ->
generate_score.py:46-48) carries no runtime state.

A subclass provides
  * ``TAIL``: the names of the parameters that get no gradient under ang_iso (placed last in the arenas);
  * ``check_input(x)``: raises for an input the kernels do not take;
  * ``_forward_impl(x, save) -> (feat, out, saved)``: saved is the dict backward needs (None unless ``save``);
  * ``_backward_impl(saved, dfeat, dout)``: the gradients of every arena entry in arena order
    (schedule.BackwardSchedule.finish), either of dfeat / dout may be None;
and may set ``BUCKET_BYTES`` and extend ``__getstate__`` for runtime state of its own.  The base has no ``__init__``:
it registers no parameter, buffer or submodule and draws no random number, so ``state_dict`` and a seeded
construction are the subclass's alone."""
import torch
import torch.nn as nn

from . import _hip
from .arena import ParamArena


class _ModelFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, model, x, *params):
        ctx.set_materialize_grads(False)
        feat, out, saved = model._forward_impl(x, save=True)
        ctx.model, ctx.saved = model, saved
        if model.keep_saved_for_test:  # parity tests read the ReLU decisions of the step
            model._last_saved_for_test = saved
        return feat, out

    @staticmethod
    def backward(ctx, dfeat, dout):
        model, saved = ctx.model, ctx.saved
        ctx.saved = None
        return (None, None) + tuple(model._backward_impl(saved, dfeat, dout))


class HipModel(nn.Module):
    TAIL = ()
    BUCKET_BYTES = None  # enable_ddp_overlap's bucket size; None: dist.BUCKET_BYTES
    # runtime state, rebuilt on first use and dropped from pickles: class-level defaults, so that a pickle of any age
    # loads without them
    _arena = None
    _side_stream = None
    _bucketer = None      # dist.GradBucketer when the all-reduce is overlapped with backward
    _segment_cut = None   # train.Trainer's capture-segment hook (schedule.BackwardSchedule)
    overlap_wgrad = True  # weight gradients on a side HIP stream (schedule.py); train.Trainer turns it off for its capture
    keep_saved_for_test = False
    RUNTIME = ("_arena", "_side_stream", "_bucketer", "_segment_cut", "_last_saved_for_test", "keep_saved_for_test")

    def __getstate__(self):
        st = dict(self.__dict__)
        for k in self.RUNTIME:
            st.pop(k, None)
        return st

    def arena(self):
        """Flat parameter/gradient arenas (built lazily, re-bound after .to(device)); TAIL goes last."""
        if self._arena is None:
            self._arena = ParamArena(list(self.named_parameters()), tail_names=self.TAIL)
        dev = self._arena.entries[0][1].device
        if not self._arena.bound() or self._arena.device != dev:
            self._arena.bind(dev)
        return self._arena

    def enable_ddp_overlap(self, bucket_bytes=None):
        """Launch the gradient all-reduce from inside backward (one process per GPU, world size > 1)."""
        from .dist import GradBucketer
        self._bucketer = GradBucketer(self.BUCKET_BYTES if bucket_bytes is None else bucket_bytes)
        return self

    def device_counter(self, name, device):
        """The Philox offset ``<name>_offset`` as a device-side counter on ``device`` (``<name>_ctr``; one per device in
        ``<name>_ctrs``).  The draw advances it there, so that a step captured in a hipGraph draws afresh on every
        replay and eager launches and replays walk one sequence.  ONE counter per device, never replaced once made: a
        captured hipGraph (train.Trainer, GraphedScorer) holds its address.  On a change of device the live count is
        carried over, so that the sequence goes on instead of restarting."""
        live, ctrs = getattr(self, name + "_ctr"), getattr(self, name + "_ctrs")
        if ctrs is None:
            ctrs = {}
            setattr(self, name + "_ctrs", ctrs)
        ctr = ctrs.get(device)
        if ctr is None:
            if live is not None:
                setattr(self, name + "_offset", int(live.item()))
            ctr = ctrs[device] = torch.tensor([getattr(self, name + "_offset")], dtype=torch.int64, device=device)
        elif live is not None and live is not ctr:
            ctr.copy_(live)  # back on a device used before: the count of the counter used in between (device-side copy)
        setattr(self, name + "_ctr", ctr)
        return ctr

    @staticmethod
    def fold_counter(st, name):
        """__getstate__: the device-side counter travels as its value."""
        if st.get(name + "_ctr") is not None:
            st[name + "_offset"] = int(st[name + "_ctr"].item())
        st[name + "_ctr"] = st[name + "_ctrs"] = None

    def forward(self, x):
        if not x.is_cuda:
            raise _hip.AirError("%s HIP path needs a GPU tensor; there is no CPU fallback" % type(self).__name__)
        self.check_input(x)
        x = x.float().contiguous()  # main_train.py:338 hands over a transposed view
        arena = self.arena()
        # eval-mode forward never records a graph (backward through running-stat BN is not on the hot path;
        # generate_score.py only scores)
        if self.training and torch.is_grad_enabled() and any(p.requires_grad for _, p, _, _ in arena.entries):
            return _ModelFn.apply(self, x, *[p for _, p, _, _ in arena.entries])
        feat, out, _ = self._forward_impl(x, save=False)
        return feat, out

    def forward_saved(self, x):
        """The train-mode forward WITHOUT autograd: (feat, saved).  With ``backward_saved`` this is what ``_ModelFn``
        does, callable from one Python thread - train.Trainer captures the step as several hipGraphs cut between
        backward's bucket boundaries (autograd would run backward on its own worker thread)."""
        self.check_input(x)
        x = x.float().contiguous()
        self.arena()
        feat, out, saved = self._forward_impl(x, save=True)
        saved["logits"] = out  # the CE head's input (train.Trainer, add_loss=None)
        return feat, saved

    def backward_saved(self, saved, dfeat, dout=None):
        """Gradients of every arena entry (views of the gradient arena, None where there is none), in arena order.
        dout: the gradient of saved["logits"] (the CE head), or None."""
        return self._backward_impl(saved, dfeat, dout)
