"""Batch-sharded data parallelism for the IGN training step: one process per GPU, one flat fp32 gradient bucket,
one RCCL all-reduce per optimizer step.

The reference has only ``nn.DataParallel`` (IGN/exp/experiment_classification.py:279-281).  Here every rank owns
a full replica and a disjoint slice of each global batch; after backward the gradients -- laid out contiguously
in ONE buffer whose slices are the parameters' ``.grad`` views, so no flatten/unflatten copies exist -- are summed
over ranks with a single ``all_reduce`` (4.27 MB for IGN-default: a latency-bound message on xGMI, one launch
instead of one per tensor) and divided by the world size.  BatchNorm statistics stay per-rank, like DataParallel.
Device-agnostic on purpose: the gloo/CPU tests in tests/test_ddp_cpu.py run the same code.
"""
import ctypes

import torch
import torch.distributed as dist

from . import _lib


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr())


class FlatParamBucket:
    ALIGN = 64          # floats

    def __init__(self, module, world_size=None, process_group=None, force_collective=False):
        self.group = process_group
        # run the all-reduce even at world size 1 (a one-rank RCCL communicator: exercises initialisation, stream ordering with
        # the library's kernels and the timing fields on a one-GPU box; the result is unchanged -- sum over one rank, / 1)
        self.force_collective = bool(force_collective)
        self.world = world_size if world_size is not None else (dist.get_world_size(process_group) if dist.is_initialized() else 1)
        self.params = [p for p in module.parameters() if p.requires_grad]
        if not self.params:
            raise ValueError("module has no trainable parameters")
        dev, dt = self.params[0].device, self.params[0].dtype
        # every parameter starts on a 256-byte boundary of the flat buffer: the HIP kernels read parameters and write
        # gradients with 16-byte vector accesses (the zero padding in between is inert for the all-reduce and for Adam)
        self.offsets, n = [], 0
        for p in self.params:
            self.offsets.append(n)
            n += (p.numel() + self.ALIGN - 1) // self.ALIGN * self.ALIGN
        self.flat_grad = torch.zeros(n, device=dev, dtype=dt)
        self.views = []
        for p, off in zip(self.params, self.offsets):
            if p.device != dev or p.dtype != dt:
                raise ValueError("all parameters must share one device and dtype")
            self.views.append(self.flat_grad[off:off + p.numel()].view_as(p))
            p.grad = None if self.flat_grad.is_cuda else self.views[-1]
        # slots that may hold something other than zeros (`gather`): the buffer starts zero-filled, and a parameter that gets no
        # gradient step after step (three of the IGN model's) needs no fill kernel per step to keep its slot at zero
        self._dirty = [False] * len(self.params)
        self._held = False          # the slots hold a running sum of micro-batch gradients (`gather(accumulate=True)`)
        self._norm = None           # (out2, workspace) of ign_grad_norm_clip (`grad_norm`)
        self.module = module

    @property
    def nbytes(self):
        return self.flat_grad.numel() * self.flat_grad.element_size()

    def broadcast_state(self, src=0):
        """Make every replica identical to rank `src` (parameters and buffers) before the first step."""
        if self.world == 1:
            return
        for t in list(self.module.parameters()) + list(self.module.buffers()):
            dist.broadcast(t.data, src=src, group=self.group)

    def gather(self, accumulate=False):
        """Bring the gradients autograd produced into the flat buffer.

        On the GPU ``zero_grad`` leaves ``p.grad = None``, so autograd hands every parameter a fresh gradient tensor (no
        accumulate kernel); one ``ign_gather_flat`` launch copies them all into their slots and ``p.grad`` is pointed back
        at the slot, so clipping, the all-reduce and the optimizer see one buffer.  Parameters whose ``.grad`` already is
        the slot view (CPU path, or a second call) are left alone; parameters without a gradient get zeros -- by a fill only when
        their slot was written since it was last zero (the buffer starts zero-filled; scaling by clipping or averaging keeps
        zeros zero).

        ``accumulate=True`` (gradient accumulation, a later micro-step of a cycle): one ``ign_gather_flat_acc`` launch ADDS the
        fresh gradients into their slots and ``p.grad`` goes back to None, so autograd never runs its per-parameter accumulate
        kernels; a parameter without a gradient in this micro-step keeps what its slot holds.  The slots then hold the running sum
        (``_held``): the next plain ``gather()`` -- the one ``allreduce`` / ``FlatAdam.step`` make -- finds ``p.grad is None``, keeps
        the slot instead of zeroing it and points ``p.grad`` at it."""
        todo = []
        for i, (p, off, view) in enumerate(zip(self.params, self.offsets, self.views)):
            g = p.grad
            if g is view:
                self._dirty[i] = True                    # written in place by autograd (CPU path) or by the caller
                continue
            if accumulate:
                if g is not None:
                    todo.append((g.contiguous(), off, view))
                    self._dirty[i] = True
                    p.grad = None
                continue
            if g is None:
                if self._dirty[i] and not self._held:
                    view.zero_()
                    self._dirty[i] = False
            else:
                todo.append((g.contiguous(), off, view))
                self._dirty[i] = True
            p.grad = view
        held, self._held = self._held, bool(accumulate)
        if not todo:
            return
        if not self.flat_grad.is_cuda:
            for g, _, view in todo:
                if accumulate or held:
                    view.add_(g)
                else:
                    view.copy_(g)
            return
        n = len(todo)
        src = (ctypes.c_void_p * n)(*[g.data_ptr() for g, _, _ in todo])
        off = (ctypes.c_longlong * n)(*[o for _, o, _ in todo])
        cnt = (ctypes.c_longlong * n)(*[g.numel() for g, _, _ in todo])
        # held: fresh gradients on top of a running sum (a cycle closed by a plain gather()) add as well
        entry = "ign_gather_flat_acc" if accumulate or held else "ign_gather_flat"
        _lib.check(getattr(_lib.lib(), entry)(src, off, cnt, n, _ptr(self.flat_grad), _lib.stream()), entry)

    def clear(self):
        """Zero the whole buffer (one fill) and forget every running sum: the state a new bucket starts in."""
        self.flat_grad.zero_()
        self._dirty = [False] * len(self.params)
        self._held = False

    def grad_norm(self, max_norm):
        """-> (2,) device tensor [||g||_2 over the flat buffer, min(1, max_norm / (norm + 1e-6))] of the gathered gradients: one
        ``ign_grad_norm_clip`` launch, no host synchronisation.  The tensor is the bucket's own and is rewritten by the next call."""
        if not self.flat_grad.is_cuda:
            raise _lib.IgnError("FlatParamBucket.grad_norm runs on the GPU only")
        self.gather()
        return self._norm_into(self._norm_buffers()[0], max_norm)

    def _norm_buffers(self):
        """(out2, workspace) of ign_grad_norm_clip, allocated once; the workspace starts zero-filled (its ticket counter)."""
        if self._norm is None:
            n = self.flat_grad.numel()
            nbytes = int(_lib.lib().ign_grad_norm_workspace_bytes(n))
            self._norm = (torch.zeros(2, device=self.flat_grad.device, dtype=torch.float32),
                          torch.zeros((nbytes + 3) // 4, device=self.flat_grad.device, dtype=torch.float32))
        return self._norm

    def _norm_into(self, out2, max_norm):
        _lib.check(_lib.lib().ign_grad_norm_clip(_ptr(self.flat_grad), self.flat_grad.numel(), float(max_norm), _ptr(out2),
                                                 _ptr(self._norm_buffers()[1]), _lib.stream()), "ign_grad_norm_clip")
        return out2

    def clip_(self, max_norm):
        """``clip_grad_norm_`` on the flat buffer: the norm launch plus one ``ign_scale_flat`` launch that multiplies the
        gradients themselves by the coefficient -> the norm before clipping, a device scalar (no host synchronisation)."""
        out2 = self.grad_norm(max_norm)
        _lib.check(_lib.lib().ign_scale_flat(_ptr(self.flat_grad), self.flat_grad.numel(),
                                             ctypes.c_void_p(out2.data_ptr() + 4), _lib.stream()), "ign_scale_flat")
        return out2[0]

    def allreduce(self):
        """Average the gradients over ranks: one collective on the flat bucket."""
        self.gather()
        if self.world == 1 and not self.force_collective:
            return
        dist.all_reduce(self.flat_grad, op=dist.ReduceOp.SUM, group=self.group)
        if self.world > 1:
            self.flat_grad.div_(self.world)

    def zero_grad(self):
        """GPU: drop the gradients (``gather`` rebuilds the flat buffer at the next step, no zero-fill and no
        accumulate kernels).  CPU: zero in place, the gradients stay views of the flat buffer."""
        if self.flat_grad.is_cuda:
            for p in self.params:
                p.grad = None
        else:
            self.flat_grad.zero_()


def shard_indices(n, rank, world, epoch=0, seed=0, shuffle=True):
    """Global permutation from a shared seed; rank r takes the r-th contiguous slice of every global batch's worth.
    Trailing samples that do not fill all ranks evenly are dropped (equal shard sizes keep the CE means exact)."""
    if shuffle:
        g = torch.Generator().manual_seed(seed + epoch)
        perm = torch.randperm(n, generator=g)
    else:
        perm = torch.arange(n)
    per = n // world
    return perm[rank * per:(rank + 1) * per]


class FlatAdam(torch.optim.Optimizer):
    """Adam over ONE flat parameter buffer: a single `ign_adam_step` launch per optimizer step instead of torch's
    per-tensor (or multi-tensor) update -- torch.optim.Adam semantics (betas (0.9, 0.999), eps 1e-8, no weight decay),
    as constructed at IGN/exp/experiment_classification.py:136.

    Parameters become views into `flat_param` (same trick as the gradient bucket), so the model, its state_dict and
    checkpoints are unaffected.  Needs the bucket (its flat gradient is the kernel's input).  A torch Optimizer
    subclass, so lr schedulers (CosineAnnealingWarmRestarts at :137) attach to it; the learning rate is read from
    ``param_groups[0]['lr']`` at every step.

    ``weight_decay`` > 0, a ``schedule`` (an ``--lr_schedule`` text or utils.optim_rule.LrSchedule) other than none, or ``ema`` > 0
    select the AdamW path (``scheduled``): one ``ign_adamw_step_dev`` launch pair per step, always in device-count form.  Its tick
    kernel computes the step's learning rate (``param_groups[0]['lr']`` is the schedule's base) and EMA decay on the device and
    leaves them in ``hp_dev`` = [bc1, bc2_sqrt, lr_t, d_t]; the decay applies to the parameters utils.optim_rule.decays names (a
    byte per 64-float chunk, ``decay_mask``); ``ema_flat`` starts as a copy of ``flat_param`` and follows it by ``ema_update()``.
    The step count of that path lives in ``step_dev`` alone: ``lr_at(step)`` is the pure host rule and reads nothing back.
    With all three neutral (the default) this is the class as it was: the same entry points, the same host count.
    """

    def __init__(self, bucket, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, capturable=False, weight_decay=0.0, schedule=None,
                 total_steps=None, ema=0.0):
        ps = bucket.params
        if not ps[0].is_cuda:
            raise _lib.IgnError("FlatAdam runs on the GPU only")
        from utils.optim_rule import parse_lr_schedule
        self.weight_decay, self.schedule, self.ema = float(weight_decay), parse_lr_schedule(schedule), float(ema)
        self.scheduled = self.weight_decay > 0.0 or self.schedule.active or self.ema > 0.0
        if self.weight_decay < 0.0 or not 0.0 <= self.ema < 1.0:
            raise ValueError(f"FlatAdam: weight_decay {weight_decay} must be >= 0 and ema {ema} in [0, 1)")
        if self.schedule.kind == 'cosine' and total_steps is None:
            raise ValueError("FlatAdam: a cosine schedule needs total_steps, the run's number of optimizer steps")
        self.total_steps = int(total_steps or 0)
        capturable = capturable or self.scheduled
        super().__init__(ps, dict(lr=lr, betas=betas, eps=eps))
        self.bucket, self.lr, self.betas, self.eps = bucket, lr, betas, eps
        self.step_count = 0
        self.flat_param = torch.zeros_like(bucket.flat_grad)
        with torch.no_grad():
            for p, off in zip(ps, bucket.offsets):
                n = p.numel()
                self.flat_param[off:off + n].copy_(p.data.reshape(-1))
                p.data = self.flat_param[off:off + n].view_as(p)
        self.exp_avg = torch.zeros_like(self.flat_param)
        self.exp_avg_sq = torch.zeros_like(self.flat_param)
        # capturable: the step count lives on the device (ign_adam_step_dev), so the step can sit inside a hipGraph
        self.capturable = bool(capturable)
        self.step_dev = torch.zeros(1, device=self.flat_param.device, dtype=torch.int32) if capturable else None
        self.bc_dev = torch.zeros(2, device=self.flat_param.device, dtype=torch.float32) if capturable else None
        # step(max_norm): [gradient norm, clip coefficient] of the last clipped step, on the device (allocated at the first one)
        self.norm_dev = None
        self.last_grad_norm = None
        self.hp_dev = self.decay_mask = self.ema_flat = None
        if self.scheduled:
            from utils.optim_rule import decay_mask
            dev = self.flat_param.device
            self.hp_dev = torch.zeros(4, device=dev, dtype=torch.float32)
            self.bc_dev = self.hp_dev[:2]
            if self.weight_decay > 0.0:
                names = [k for k, p in bucket.module.named_parameters() if p.requires_grad]
                self.decay_mask = torch.from_numpy(decay_mask(names, ps, bucket.offsets, self.flat_param.numel(),
                                                              bucket.ALIGN)).to(dev)
            if self.ema > 0.0:
                self.ema_flat = self.flat_param.clone()

    def lr_at(self, step):
        """The learning rate optimizer step `step` = 1, 2, ... uses, in float64: the host statement of the rule the tick kernel
        evaluates (utils.optim_rule.lr_at); reads nothing from the device."""
        from utils.optim_rule import lr_at
        return lr_at(self.schedule, self.param_groups[0]["lr"], self.total_steps, step)

    def ema_update(self):
        """ema_flat += (1 - d_t) * (flat_param - ema_flat) with the decay the last step's tick left in hp_dev: one launch, to be
        made after whatever rewrites the parameters behind the optimizer (the --pos_weight clamp)."""
        if self.ema_flat is None:
            raise _lib.IgnError("FlatAdam.ema_update: constructed with ema = 0")
        _lib.check(_lib.lib().ign_ema_update(_ptr(self.ema_flat), _ptr(self.flat_param), self.flat_param.numel(), _ptr(self.hp_dev),
                                             _lib.stream()), "ign_ema_update")

    def swap_ema(self):
        """Exchange flat_param and ema_flat in place (one launch; no pointer changes, so parameter views and captured graphs stay
        valid): the model then computes with the averaged weights, a second call puts the live ones back."""
        if self.ema_flat is None:
            raise _lib.IgnError("FlatAdam.swap_ema: constructed with ema = 0")
        _lib.PARAM_GENERATION[0] += 1                # the parameters change behind autograd's back
        _lib.check(_lib.lib().ign_swap_flat(_ptr(self.flat_param), _ptr(self.ema_flat), self.flat_param.numel(), _lib.stream()),
                   "ign_swap_flat")

    def make_capturable(self):
        """Move the step count to the device (ign_adam_step_dev) so that the optimizer step can be captured into a hipGraph;
        the trajectory is unchanged (same update rule, the count continues where the host count stands)."""
        if not self.capturable:
            dev = self.flat_param.device
            self.step_dev = torch.full((1,), self.step_count, device=dev, dtype=torch.int32)
            self.bc_dev = torch.zeros(2, device=dev, dtype=torch.float32)
            self.capturable = True

    @torch.no_grad()
    def step(self, closure=None, max_norm=None):
        """One Adam step.  ``max_norm`` > 0: gradient clipping as ``clip_grad_norm_(parameters, max_norm)`` in front of the step --
        one ``ign_grad_norm_clip`` launch leaves [norm, coefficient] in ``last_grad_norm`` / ``norm_dev`` on the device and the
        ``_clip`` Adam entry point reads every gradient times that coefficient (the gradients themselves are not rewritten)."""
        loss = closure() if closure is not None else None
        self.bucket.gather()
        self.step_count += not self.scheduled        # the host count of ign_adam_step; the AdamW path counts in step_dev alone
        _lib.PARAM_GENERATION[0] += 1                # the kernel rewrites the parameters through raw pointers
        clip = max_norm is not None and max_norm > 0
        if clip:
            if self.norm_dev is None:
                self.norm_dev = torch.zeros(2, device=self.flat_param.device, dtype=torch.float32)
                self.last_grad_norm = self.norm_dev[0]
            self.bucket._norm_into(self.norm_dev, max_norm)
        g = self.param_groups[0]
        if self.scheduled:
            s = self.schedule
            _lib.check(_lib.lib().ign_adamw_step_dev(
                _ptr(self.flat_param), _ptr(self.bucket.flat_grad), _ptr(self.exp_avg), _ptr(self.exp_avg_sq), self.flat_param.numel(),
                g["betas"][0], g["betas"][1], g["eps"], self.weight_decay,
                None if self.decay_mask is None else _ptr(self.decay_mask), s.code, float(g["lr"]), s.warmup, s.min_lr,
                self.total_steps, self.ema, _ptr(self.step_dev), _ptr(self.hp_dev),
                ctypes.c_void_p(self.norm_dev.data_ptr() + 4) if clip else None, _lib.stream()), "ign_adamw_step_dev")
            return loss
        entry = "ign_adam_step" + ("_clip" if clip else "") + ("_dev" if self.capturable else "")
        args = [_ptr(self.flat_param), _ptr(self.bucket.flat_grad), _ptr(self.exp_avg), _ptr(self.exp_avg_sq),
                self.flat_param.numel(), g["lr"], g["betas"][0], g["betas"][1], g["eps"]]
        args += [_ptr(self.step_dev), _ptr(self.bc_dev)] if self.capturable else [self.step_count]
        if clip:
            args.append(ctypes.c_void_p(self.norm_dev.data_ptr() + 4))          # the coefficient, out2[1] of the norm launch
        _lib.check(getattr(_lib.lib(), entry)(*args, _lib.stream()), entry)
        return loss

    def zero_grad(self, set_to_none=False):
        self.bucket.zero_grad()
