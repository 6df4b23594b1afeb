"""The stream schedule shared by the backward passes of every hip_model.HipModel (ResNet, Res2Net2's fp32 and
bf16-resident paths, LCNN, Res2Net).

Weight gradients feed nothing until the optimiser, so they may run on a SIDE stream: the MFMA-bound weight-gradient
kernels overlap the HBM-bound BatchNorm-backward passes and the dgrad chain of the main stream.  Ordering: a weight
gradient starts after an event of the main stream that marks its operands ready; the tensors it reads are kept alive
until the join (the caching allocator would hand their memory back to the main stream); the main stream joins the side
stream before the gradients are used.  The schedule also reports where a part of the gradient arena is final (a
segment cut of train.Trainer's hipGraph capture, a bucket of dist.GradBucketer), records which gradients a pass wrote
and folds an accumulating backward back into the old sums."""
import torch

from . import ops


def side_stream(model):
    """The model's side stream (``model._side_stream``), made on first use."""
    if model._side_stream is None:
        model._side_stream = torch.cuda.Stream(device=torch.cuda.current_stream().device)
    return model._side_stream


class BackwardSchedule:
    def __init__(self, model, arena, use_side, bucketer, side_when_accumulating):
        """use_side: weight gradients on the side stream.  bucketer: a dist.GradBucketer or None; an accumulating
        pass sends nothing from inside backward.  side_when_accumulating: False runs an accumulating pass as one chain."""
        self.arena, self.G = arena, arena.grad_views()
        # gradient accumulation (a second backward without zero_grad): p.grad already IS the arena view, so autograd's
        # "p.grad += returned view" would double the NEW gradient instead of adding the old one.  The old sums are kept
        # aside, folded back in by finish(), and None is returned for the aliased entries
        self.aliased = [p.grad is not None and p.grad.data_ptr() == self.G[n].data_ptr() for n, p, _, _ in arena.entries]
        self.accumulating = any(self.aliased)
        self.old = arena.grad.clone() if self.accumulating else None
        self.use_side = use_side and (side_when_accumulating or not self.accumulating)
        self.main = torch.cuda.current_stream()
        self.side = side_stream(model) if self.use_side else self.main
        self.keep = []  # tensors the side stream reads
        self.cut = model._segment_cut
        self.have = set()  # names handed out by grad()
        self.bucketer = None if self.accumulating else bucketer
        if self.bucketer is not None:
            self.bucketer.reset(arena.grad, arena.head_total)

    def grad(self, name):
        """The gradient-arena view of parameter ``name``, for a kernel to write; recorded as written for finish()."""
        self.have.add(name)
        return self.G[name]

    def on_side(self, fn, *reads, done=False):
        """Run fn() on the side stream once everything enqueued on main so far is done (inline without one).
        done: return an event marking fn's completion (None when fn ran inline)."""
        if not self.use_side:
            fn()
            return None
        self.keep.extend(reads)
        ready = torch.cuda.Event()
        ready.record(self.main)
        self.side.wait_event(ready)
        with torch.cuda.stream(self.side):
            fn()
        if not done:
            return None
        ev = torch.cuda.Event()
        ev.record(self.side)
        return ev

    def grads_final_from(self, name):
        """Everything that writes arena.grad[offset(name):] has been enqueued: a capture segment may end here (under
        capture the side stream is off, so nothing is forked at a cut), and that part may go to the bucketer."""
        lo = self.arena.offsets[name]
        if self.cut is not None:
            self.cut(lo)
        if self.bucketer is not None:
            evs = [torch.cuda.Event()]
            evs[0].record(self.main)
            if self.use_side:
                evs.append(torch.cuda.Event())
                evs[1].record(self.side)
            self.bucketer.ready(lo, evs)

    def join(self):
        if self.use_side:
            self.main.wait_stream(self.side)  # every weight gradient is in the arena
        self.keep.clear()

    def finish(self, has_grad=None, tail_has_grad=None, keep_old_tail=False):
        """Join, set arena.tail_has_grad and fold an accumulating pass's old sums back in.  Returns the gradients for
        autograd in arena order: None where has_grad(name) is False or where p.grad already is the arena view.
        Without arguments: what grad() recorded (the tail has gradients when one of its names was handed out); a pass
        that indexes G itself says which entries it wrote.
        keep_old_tail: an accumulating pass marks the tail live (its old sums), zeroing it first where this pass wrote
        none of it."""
        self.join()
        arena = self.arena
        if has_grad is None:
            has_grad, tail_has_grad = self.have.__contains__, not self.have.isdisjoint(arena.tail_names)
        arena.tail_has_grad = tail_has_grad
        if self.accumulating:
            if keep_old_tail:
                if not tail_has_grad:
                    arena.grad[arena.head_total:].zero_()
                arena.tail_has_grad = True
            ops.add_(arena.grad, self.old)
        return [None if a else (self.G[n] if has_grad(n) else None) for (n, _, _, _), a in zip(arena.entries, self.aliased)]
