"""A whole GAN train step captured once in a hipGraph and replayed.

Why: at small batches the step is bound by its ~340 kernel launches, not by the kernels (256x256 / B=1: 4.6 ms per
step for ~1.6 ms of kernel time; the reference ships batch 2, train.py:77).  A captured step replays all launches from
one hipGraphLaunch: no per-launch host work, back-to-back dispatch on the device.

What makes the step capturable: nothing in `train_step` synchronises with the host, every buffer the kernels touch is
either persistent (parameters, gradient buffers, Adam state, prepared weights, workspaces) or comes from torch's
graph-private memory pool, and the only kernel arguments that change from step to step -- Adam's two bias-correction
scalars, which carry the learning rate -- are read from device memory (tg_adam_multi_s) and refreshed before each replay from
the live param_groups (ops.AdamScalarArena).  Results are bit-identical to the eager step, also when the host changes weights,
learning rate or optimiser state between two replays (tests/test_hip_graph.py; GraphedTrainStep's docstring has the table).

Single-GPU only: the data-parallel path keeps the eager schedule (its collectives are launched by torch.distributed).
"""
import torch

from . import ops as O


class GraphedTrainStep:
    """step = GraphedTrainStep(G, D, criterion, optG, optD); out = step(real, mask)

    The first `warmup` calls run eagerly (they create the optimiser state, gradient buffers, workspaces, prepared-weight
    tables and per-kernel LDS opt-ins -- none of which may happen inside a capture); the next call captures; every call
    from then on copies the batch into the static input buffers and replays.  The returned dict holds STATIC tensors that
    the next call overwrites.  `flush()` brings the torch optimisers' host-side step counters up to date (state_dict(),
    checkpoints); it is cheap and idempotent.

    What the host may change between two calls, and what the next call does about it (host-side comparisons only: an
    unchanged step launches nothing more and never synchronises):
      weights       written in place through torch (load_state_dict, copy_, mul_ ...) or through `.data` followed by
                    ops.weights_updated(), eager forwards with other weights swapped in and out again: honoured -- the
                    prepared buffers the graph reads without preparing them itself are re-prepared when their stamp is
                    not their weight's (one launch, only then).
      learning rate param_groups[i]["lr"]: honoured, read at every replay.
      betas, eps, weight_decay / amsgrad / maximize: ValueError -- they are arguments of the captured launches.
      optimiser state replaced (optimizer.load_state_dict), parameters or gradient buffers moved: the captured pointers
                    are gone; flush(), drop the graph, `warmup` eager calls, capture again (`captures` counts).
      batch shape   ValueError."""

    def __init__(self, generator, discriminator, criterion, optimizer_G, optimizer_D, warmup=2, reuse_fake_forward=True):
        self.G, self.D, self.crit, self.oG, self.oD = generator, discriminator, criterion, optimizer_G, optimizer_D
        self.warmup, self.reuse = max(int(warmup), 1), reuse_fake_forward
        self.calls, self.graph, self.out, self.shape = 0, None, None, None
        self.replays, self.flushed, self.captures = 0, 0, 0
        self.eager_left, self.base = self.warmup, 0           # eager calls before the next capture; `replays` at that capture
        self.arena, self.states = None, []

    def _eager(self, real, mask):
        from mvp_gan.src.train import train_step
        return train_step(self.G, self.D, self.crit, self.oG, self.oD, real, mask, reuse_fake_forward=self.reuse)

    def _capture(self, real, mask):
        dev = real.device
        self.real_s, self.mask_s = torch.empty_like(real), torch.empty_like(mask)
        self.shape = (tuple(real.shape), tuple(mask.shape))
        self.arena = O.AdamScalarArena(dev)
        self.graph = torch.cuda.CUDAGraph()
        torch.cuda.synchronize(dev)
        O.adam_scalar_arena = self.arena
        self.arena.active = True
        O.wprep_capture = cap = O.WprepCapture()
        try:
            with torch.cuda.graph(self.graph):
                self.out = self._eager(self.real_s, self.mask_s)
        finally:
            self.arena.active = False
            O.adam_scalar_arena = None
            O.wprep_capture = None
        self.captures += 1
        self.base = self.replays
        # what a replay changes behind the host-side prepared-weight cache (ops.graph_replayed)
        self.wprep_keys = list(dict.fromkeys(cap.keys))
        self.wptrs = sorted({p.data_ptr() for m in (self.G, self.D) for p in m.parameters() if p.dim() == 4 and p.requires_grad})
        # the prepared buffers a replay reads as it finds them, with their entries (which keep the buffers alive), and the
        # device tables its launches read
        self.watched = [(key, O._wprep[key], O._wprep[key][2]) for key in dict.fromkeys(cap.keys + cap.hits)]
        self.refs = cap.refs
        self.gbufs = [(m, m.__dict__.get("_tg_gradbuf")) for m in (self.G, self.D)]
        # the capture executed hip_adam_step's HOST side (state["step"] += 1) without running a step on the device
        self.states = [st for opt in (self.oG, self.oD) for st in opt.state.values() if "step" in st]
        for st in self.states:
            st["step"] -= 1

    def _moved(self):
        """Hold what the graph has baked in against the live optimisers and modules.  Raises for a changed hyper-parameter;
        True when a captured pointer is no longer the live one (the graph must go)."""
        for launch, (_lr, b1, b2, _step) in zip(self.arena.launches, self.arena.slots):
            if launch is None or launch.owner is None:          # (an adam_multi_ call outside hip_adam_step: nothing live to read)
                continue
            opt, gi, _params = launch.owner
            group = opt.param_groups[gi]
            for name, was, now in (("betas", (b1, b2), tuple(group["betas"])), ("eps", launch.eps, float(group["eps"])),
                                   ("weight_decay", 0, group.get("weight_decay", 0)), ("amsgrad", False, group.get("amsgrad", False)),
                                   ("maximize", False, group.get("maximize", False))):
                if was != now:
                    raise ValueError(f"GraphedTrainStep: param_groups[{gi}]['{name}'] was {was} when the step was captured and is "
                                     f"{now} now: it is an argument of the captured Adam launch (make a new GraphedTrainStep)")
            if launch.live_ptrs() != launch.ptrs:
                return True
        for m, gb in self.gbufs:
            if m.__dict__.get("_tg_gradbuf") is not gb:
                return True
        for key, ent, buf in self.watched:
            if O._wprep.get(key) is not ent or ent[2] is not buf:
                return True
        return False

    def _drop(self):
        self.flush()
        self.graph = self.out = self.arena = None
        self.watched, self.refs, self.gbufs = [], [], []
        self.eager_left = self.warmup

    def __call__(self, real, mask):
        self.calls += 1
        if self.graph is not None and self._moved():
            self._drop()
        if self.graph is None:
            if self.eager_left > 0:
                self.eager_left -= 1
                return self._eager(real, mask)
            self._capture(real, mask)
        if (tuple(real.shape), tuple(mask.shape)) != self.shape:
            raise ValueError(f"GraphedTrainStep: captured for batch shape {self.shape[0]}, got {tuple(real.shape)}")
        stale = O.prepared_stale([key for key, _ent, _buf in self.watched])
        if stale:
            O.prepare_keys(stale)
        self.real_s.copy_(real, non_blocking=True)
        self.mask_s.copy_(mask, non_blocking=True)
        self.arena.refresh(self.replays - self.base)
        self.graph.replay()
        self.replays += 1
        O.graph_replayed(self.wptrs, self.wprep_keys)
        return self.out

    def flush(self):
        n = self.replays - self.flushed
        if n:
            # (the state entries the graph was captured on: one that optimizer.load_state_dict() replaced since carries its own count)
            for st in self.states:
                st["step"] += n
            self.flushed = self.replays
