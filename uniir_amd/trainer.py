"""Native optimizer + train step for the CLIP_SF in-batch contrastive path on MI355X.

Mirrors UniIR src/models/uniir_clip/engine.py:19-50 (forward, loss / accumulation_steps, backward, optimizer step every
accumulation_steps, scheduler.step) and clip_scorefusion/train.py:52-61,195-199,281-284 (AdamW lr 1e-5 betas
(0.9,0.98) eps 1e-6, weight decay 0 for gains / biases / logit_scale and 0.2 for the rest,
CosineAnnealingLR(T_max, eta_min=0)).  Differences, all result-preserving:
  * bf16 MFMA compute needs no GradScaler's loss scale (the reference's fp16 autocast does); the other half of scaler.step() -- a step
    whose gradients hold Inf / NaN is not applied -- is the opt-in GradGuard below, with clip_grad_norm_ on top;
  * gradients live in one flat fp32 buffer: DDP's bucketed all-reduce(mean) becomes RCCL all-reduce(sum) of ranges of
    that buffer, launched per finished residual block while backward still runs (comm.GradReducer; one blocking
    all-reduce of the remainder at step()), with the 1/world factor folded into the fused AdamW kernel;
  * AdamW is one fused kernel per weight-decay group and refreshes the bf16 weight shadow in the same pass.
"""
import bisect
import math
import os

import torch

from . import _lib, comm, ops


def guard_settings(max_grad_norm=None, skip_nonfinite=False, trainer_config=None):
    """-> (max_grad_norm or None, skip_nonfinite) of the gradient guard, both off unless something asks: an explicit argument, else
    the optional YAML keys trainer_config.max_grad_norm / trainer_config.skip_nonfinite_steps (absent in every reference YAML), else the
    environment, UNIIR_MAX_GRAD_NORM=<float> / UNIIR_SKIP_NONFINITE=1.  A norm of 0 or below means no clipping."""
    def cfg(key):
        if trainer_config is None:
            return None
        return trainer_config.get(key, None) if hasattr(trainer_config, "get") else getattr(trainer_config, key, None)

    if max_grad_norm is None:
        max_grad_norm = cfg("max_grad_norm")
    if max_grad_norm is None and os.environ.get("UNIIR_MAX_GRAD_NORM", "") != "":
        max_grad_norm = os.environ["UNIIR_MAX_GRAD_NORM"]
    if max_grad_norm is not None:
        max_grad_norm = float(max_grad_norm)
        if math.isnan(max_grad_norm):
            raise ValueError("max_grad_norm is NaN")
        if max_grad_norm <= 0:
            max_grad_norm = None
    if not skip_nonfinite:
        skip_nonfinite = cfg("skip_nonfinite_steps")
        if skip_nonfinite is None:
            skip_nonfinite = os.environ.get("UNIIR_SKIP_NONFINITE", "0") not in ("", "0")
    return max_grad_norm, bool(skip_nonfinite)


class GradGuard:
    """The device-side guard around the optimizer step (include/uniir_hip.h [OPT] gradient guard): one uniir_grad_guard call per step
    over the AdamW ranges of every store fills a 64-byte control block on the device -- the global norm of the gradient AdamW will
    consume, the clip_grad_norm_ coefficient, and whether the step is skipped because a gradient is Inf / NaN -- and the guarded AdamW
    launches read it there.  The host never reads device memory inside step(): the block is copied to a pinned mirror behind the
    step's launches and read one step later (resolve())."""

    def __init__(self, max_grad_norm=None, skip_nonfinite=False):
        self.max_grad_norm = max_grad_norm
        self.skip_nonfinite = bool(skip_nonfinite)
        self.steps_seen = self.steps_skipped = 0      # as of the last resolved step (or the checkpoint)
        self.ctl = self.mirror = self.event = self.workspace = self.plan = None
        self.pending = False
        self.stats = None                             # of the last resolved step
        self._where = []                              # (store, lo) of every range of the pending step

    def _device_state(self, dev):
        if self.ctl is None or self.ctl.device != dev:
            host = torch.zeros(8, dtype=torch.int64)
            host[5], host[6] = self.steps_seen, self.steps_skipped
            self.ctl = host.to(dev)                   # the allocator's blocks are 512-byte aligned
            self.mirror = torch.zeros(8, dtype=torch.int64).pin_memory()
            self.event = torch.cuda.Event()
            self.workspace = None

    def measure(self, ranges, grad_scale):
        """ranges: [(FlatStore, lo, hi)], every AdamW range of the step.  Launches the norm / scan kernels and the finish."""
        dev = ranges[0][0].dev
        self._device_state(dev)
        key = tuple((st.g32.data_ptr(), lo, hi) for st, lo, hi in ranges)
        if self.plan is None or self.plan.key != key:
            self.plan = ops.GradGuardPlan([(st.g32, lo, hi) for st, lo, hi in ranges])
        if self.workspace is None or self.workspace.numel() < self.plan.workspace_bytes:
            self.workspace = torch.empty(max(256, self.plan.workspace_bytes), dtype=torch.uint8, device=dev)
        self._where = [(st, lo) for st, lo, _ in ranges]
        self.plan.launch(grad_scale, self.max_grad_norm or 0.0, self.skip_nonfinite, self.ctl, self.workspace)

    def publish(self):
        """behind the step's launches: control block -> pinned mirror, asynchronously, and an event"""
        self.mirror.copy_(self.ctl, non_blocking=True)
        self.event.record()
        self.pending = True

    def resolve(self):
        """wait for the last published step and read its outcome; -> True when that step was skipped and not yet reported"""
        if not self.pending:
            return False
        self.event.synchronize()
        self.pending = False
        c = _lib.GradCtl.from_buffer_copy(self.mirror.numpy().tobytes())
        first_bad = None
        if c.first_bad_range >= 0:
            st, lo = self._where[c.first_bad_range]
            names, offs = list(st.off), list(st.off.values())
            first_bad = names[bisect.bisect_right(offs, lo + c.first_bad_index) - 1]
        self.steps_seen, self.steps_skipped = int(c.steps_seen), int(c.steps_skipped)
        self.stats = {"norm": float(c.norm), "coef": float(c.coef), "skipped": bool(c.skip), "nonfinite": bool(c.nonfinite),
                      "sumsq": float(c.sumsq), "steps_seen": self.steps_seen, "steps_skipped": self.steps_skipped,
                      "first_bad": first_bad}
        return bool(c.skip)

    def load_counters(self, seen, skipped):
        self.steps_seen, self.steps_skipped = int(seen), int(skipped)
        if self.ctl is not None:
            self.ctl[5:7] = torch.tensor([self.steps_seen, self.steps_skipped], dtype=torch.int64)


class NativeAdamW(torch.optim.Optimizer):
    """torch.optim.AdamW semantics over flat parameter stores (flat_store.FlatStore): the model's own store -- param group 0
    without weight decay, group 1 with -- and one param group per extra store.  Each store gets one fused AdamW launch per run of
    consecutive tensors of one group (FlatStore.ranges) and one pair of moment buffers; the launches write the masters and the bf16
    shadow, and FlatStore.kernel_wrote() after them brings the store's other copies along.  It is a real torch Optimizer
    (param_groups / lr schedulers / state_dict work)."""

    def __init__(self, clip_model, lr=1e-5, betas=(0.9, 0.98), eps=1e-6, weight_decay=0.2, allreduce=True, extra=None,
                 overlap=True, bucket_bytes=64 << 20, max_grad_norm=None, skip_nonfinite=False):
        """clip_model: the model that owns the main store (CLIP, BLIPFeatureFusion): _ensure_flat() -> its FlatStore,
        optimizer_groups() -> (no-decay params, decay params), adamw_group(name) -> 0 / 1, or None for a tensor that is not
        stepped (BLIP_SF's frozen cross-attention).
        extra: further flat parameter stores, each one param group of its own -- objects with .params (list of nn.Parameter),
        .store() (-> FlatStore), .weight_decay and .lr (CLIP_FF's T5 stack: clip_featurefusion/train.py:52-61 gives it weight
        decay 0.2 on everything and its own learning rate)
        max_grad_norm / skip_nonfinite: the gradient guard (GradGuard), off by default and then absent: step() issues the plain
        AdamW launches and nothing else.  max_grad_norm clips the global norm over every store like clip_grad_norm_; skip_nonfinite
        leaves a step out whose gradients hold Inf or NaN, as the reference's scaler.step(optimizer) does.  The environment
        (UNIIR_MAX_GRAD_NORM, UNIIR_SKIP_NONFINITE) is read here where the arguments are left at their defaults."""
        max_grad_norm, skip_nonfinite = guard_settings(max_grad_norm, skip_nonfinite)
        self.guard = GradGuard(max_grad_norm, skip_nonfinite) if (max_grad_norm is not None or skip_nonfinite) else None
        self.clip = clip_model
        self.extra = list(extra or [])
        nd, d = clip_model.optimizer_groups()
        groups = [{"params": nd, "weight_decay": 0.0}, {"params": d, "weight_decay": weight_decay}]
        groups += [{"params": e.params, "weight_decay": e.weight_decay, "lr": e.lr} for e in self.extra]
        super().__init__(groups, dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay))
        # (store getter, tensor name -> param group index) of every store, the model's own first
        self.sources = [(clip_model._ensure_flat, clip_model.adamw_group)]
        self.sources += [(e.store, lambda name, gi=2 + i: gi) for i, e in enumerate(self.extra)]
        self.mv = [None] * len(self.sources)            # (exp_avg, exp_avg_sq) of every store
        self._ranges = [(None, None)] * len(self.sources)      # (store, its AdamW ranges)
        self.allreduce = allreduce
        self.overlap, self.bucket_bytes = overlap, bucket_bytes
        self.reducer = None
        self.last_collectives = 0
        self.opt_step = 0

    def _moments(self, i, st):
        mv = self.mv[i]
        if mv is None or mv[0].numel() != st.total:
            mv = (torch.zeros_like(st.p32), torch.zeros_like(st.p32))
        elif mv[0].device != st.dev:          # resumed from a checkpoint mapped to the CPU
            mv = tuple(t.to(st.dev) for t in mv)
        self.mv[i] = mv
        return mv

    def _buffers(self):
        st = self.clip._ensure_flat()
        self._moments(0, st)
        if self.allreduce and self.overlap and comm.world() > 1:
            if self.reducer is None or self.reducer.flat.data_ptr() != st.g32.data_ptr():
                self.reducer = comm.GradReducer(st.g32, self.bucket_bytes)
        else:
            self.reducer = None
        return st

    def arm_overlap(self, last_micro_batch=True):
        """call before backward(): on the LAST micro-batch of an accumulation window the tower backward hands every finished
        residual block's weight gradients to the reducer (DDP's no_sync() on the earlier micro-batches)"""
        self._buffers()
        if self.reducer is not None:
            self.reducer.reset()           # an armed backward that never reached step() must not leak into this one
        self.clip._grad_reducer = self.reducer if last_micro_batch else None

    @torch.no_grad()
    def step(self, closure=None):
        main = self._buffers()
        if self.guard is not None:
            self._resolve_guard()          # the outcome of the step before this one: a skipped step does not count
        world = comm.world() if self.allreduce else 1
        reduced = set()                    # gradient buffers already all-reduced in this step
        if world > 1:
            self.last_collectives = 0
            if self.reducer is not None:           # blocks already reduced during backward; now the remainder + wait
                self.last_collectives, reduced = self.reducer.finish()
                reduced.add(main.g32.data_ptr())
        self.clip._grad_reducer = None
        self.opt_step += 1
        if self.guard is not None:
            return self._step_guarded(main, world, reduced)
        for i, (store, group_of) in enumerate(self.sources):
            st = main if i == 0 else store()
            m, v = self._moments(i, st)
            if world > 1 and st.g32.data_ptr() not in reduced:     # one all-reduce of the whole buffer
                comm.allreduce_sum_(st.g32)
                self.last_collectives += 1
            if self._ranges[i][0] is not st:
                self._ranges[i] = (st, st.ranges(group_of))
            for lo, hi, gi in self._ranges[i][1]:
                group = self.param_groups[gi]
                b1, b2 = group["betas"]
                ops.call("uniir_adamw_step", st.p32[lo:hi], st.g32[lo:hi], m[lo:hi], v[lo:hi], st.w16_buf[lo:hi], hi - lo,
                         float(group["lr"]), b1, b2, group["eps"], group["weight_decay"], self.opt_step, 1.0 / world)
            st.kernel_wrote()                  # the kernel wrote p32 and the bf16 shadow itself: the store's other copies follow

    def _step_guarded(self, main, world, reduced):
        """the rest of step() behind the gradient guard: the all-reduce of every store first, then ONE norm / scan over the AdamW
        ranges of all stores (a global norm, as clip_grad_norm_(model.parameters()) takes it; frozen tensors are in no range), then
        the guarded AdamW launches, which read the decision on the device"""
        work = []
        for i, (store, group_of) in enumerate(self.sources):
            st = main if i == 0 else store()
            m, v = self._moments(i, st)
            if world > 1 and st.g32.data_ptr() not in reduced:
                comm.allreduce_sum_(st.g32)
                self.last_collectives += 1
            if self._ranges[i][0] is not st:
                self._ranges[i] = (st, st.ranges(group_of))
            work.append((st, m, v, self._ranges[i][1]))
        self.guard.measure([(st, lo, hi) for st, _, _, rs in work for lo, hi, _ in rs], 1.0 / world)
        for st, m, v, rs in work:
            for lo, hi, gi in rs:
                group = self.param_groups[gi]
                b1, b2 = group["betas"]
                ops.call("uniir_adamw_step_guarded", st.p32[lo:hi], st.g32[lo:hi], m[lo:hi], v[lo:hi], st.w16_buf[lo:hi], hi - lo,
                         float(group["lr"]), b1, b2, group["eps"], group["weight_decay"], self.opt_step, 1.0 / world,
                         self.guard.ctl)
            st.kernel_wrote()
        self.guard.publish()

    def _resolve_guard(self):
        if self.guard.resolve():           # that step was skipped: bias correction counts applied steps only, as torch's does when
            self.opt_step -= 1             # scaler.step() leaves optimizer.step() out

    def grad_stats(self):
        """the guard's view of the last step(): {"norm", "coef", "skipped", "nonfinite", "sumsq", "steps_seen", "steps_skipped",
        "first_bad"}; first_bad is the name of the tensor (FlatStore.off) that holds the first non-finite gradient, None without one.
        Waits for that step's launches.  None without a guard or before the first step."""
        if self.guard is None:
            return None
        self._resolve_guard()
        return self.guard.stats

    def zero_grad(self, set_to_none=False):
        self.clip._ensure_flat()
        self.clip.zero_grad()
        for e in self.extra:
            e.store().g32.zero_()

    def state_dict(self):
        if self.guard is not None:
            self._resolve_guard()          # opt_step below counts applied steps
        exp_avg, exp_avg_sq = self.mv[0] or (None, None)
        sd = {"opt_step": self.opt_step, "exp_avg": exp_avg, "exp_avg_sq": exp_avg_sq, "extra": self.mv[1:],
              "param_groups": [{k: v for k, v in g.items() if k != "params"} for g in self.param_groups]}
        if self.guard is not None:
            sd.update(steps_seen=self.guard.steps_seen, steps_skipped=self.guard.steps_skipped,
                      max_grad_norm=self.guard.max_grad_norm, skip_nonfinite=self.guard.skip_nonfinite)
        return sd

    def load_state_dict(self, sd):
        self.opt_step = sd["opt_step"]
        main = None if sd["exp_avg"] is None else (sd["exp_avg"], sd["exp_avg_sq"])
        self.mv = [main] + list(sd.get("extra", self.mv[1:]))
        for g, s in zip(self.param_groups, sd["param_groups"]):
            g.update(s)
        if self.guard is not None:         # the counters travel; the settings are this run's own (a checkpoint without them: zeros)
            self.guard.pending = False
            self.guard.load_counters(sd.get("steps_seen", 0), sd.get("steps_skipped", 0))


class CosineLR:
    """closed form of torch CosineAnnealingLR(T_max=t_total, eta_min=0) driving NativeAdamW.param_groups"""

    def __init__(self, optimizer, t_total):
        self.opt, self.t_total, self.step_count = optimizer, max(1, t_total), 0
        self.base = [g["lr"] for g in optimizer.param_groups]

    def step(self):
        self.step_count += 1
        for g, b in zip(self.opt.param_groups, self.base):
            g["lr"] = b * (1 + math.cos(math.pi * self.step_count / self.t_total)) / 2

    def state_dict(self):
        return {"step_count": self.step_count, "base": self.base, "t_total": self.t_total}

    def load_state_dict(self, sd):
        self.step_count, self.base, self.t_total = sd["step_count"], sd["base"], sd["t_total"]
        self.step_count -= 1
        self.step()


class NativeTrainer:
    def __init__(self, model, lr=1e-5, betas=(0.9, 0.98), eps=1e-6, weight_decay=0.2, t_total=1000,
                 accumulation_steps=1, max_grad_norm=None, skip_nonfinite=False):
        self.model = model
        self.clip = model.clip_model
        extra = [model.t5_optimizer_group(lr=lr, weight_decay=weight_decay)] if hasattr(model, "t5_optimizer_group") else None
        self.opt = NativeAdamW(self.clip, lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, extra=extra,
                               max_grad_norm=max_grad_norm, skip_nonfinite=skip_nonfinite)
        self.sched = CosineLR(self.opt, t_total)
        self.accum = accumulation_steps
        self.micro = 0
        self._stash_reviewed = False

    def train_step(self, batch):
        """one micro-batch: returns the reference's outputs dict (loss un-scaled, as logged by engine.py:48)."""
        if self.micro == 0:
            self.opt.zero_grad()
        self.model.train()
        out = self.model(batch)
        self.opt.arm_overlap(self.micro == self.accum - 1)
        (out["loss"] / self.accum).backward()
        self.micro += 1
        if self.micro == self.accum:
            self.opt.step()
            self.sched.step()
            self.micro = 0
            if not self._stash_reviewed:          # once, after the first complete step (clip_model.CLIP.review_stash)
                self._stash_reviewed = True
                clip = getattr(self.model, "clip_model", None)
                if clip is not None and hasattr(clip, "review_stash"):
                    clip.review_stash(comm.all_reduce_min_float if comm.world() > 1 else None)
        return out
