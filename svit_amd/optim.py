"""Optimiser tail of the training step on the flat parameter buffers.

Replaces `scaler.unscale_ -> clip_grad_norm_(1.0) -> AdamW.step` (tools/train_net.py:136-151,
slowfast/models/optimizer.py:15-112) by three HBM-bound launches: one sum-of-squares reduction
over the flat grad buffer and one fused clip+AdamW kernel per weight-decay group.  No host
synchronisation: the clip coefficient is computed on the device from the reduced norm.

GuardedClipAdamW is the same tail with the other half of `scaler.step`: a step whose gradients hold an inf or a NaN
is dropped ON THE DEVICE (weights, moments and the step counter stay as they were).  Every scalar of the step lives
in a step record in device memory, so the tail can end a captured graph (graph.GraphedTrainStep(optimizer=...)).
"""
import math

import numpy as np
import torch

from . import freeze, hip, lrscale, ops
from .lrscale import lr_scale_from_cfg  # noqa: F401  (construct_optimizer's source of `lr_scale`)


def get_lr_at_epoch(cfg, cur_epoch):
    """slowfast/utils/lr_policy.py:9-96: the `cosine` and `steps_with_relative_lrs` policies with optional linear
    warm-up."""
    s = cfg.SOLVER

    def cosine(ep):
        offset = s.WARMUP_EPOCHS if s.COSINE_AFTER_WARMUP else 0.0
        assert s.COSINE_END_LR < s.BASE_LR
        return s.COSINE_END_LR + (s.BASE_LR - s.COSINE_END_LR) * (
            math.cos(math.pi * (ep - offset) / (s.MAX_EPOCH - offset)) + 1.0) * 0.5

    def steps_with_relative_lrs(ep):
        """LRS[i] * BASE_LR from epoch STEPS[i] on (lr_policy.py:69-96; past MAX_EPOCH the last entry of LRS)"""
        for ind, step in enumerate(list(s.STEPS) + [s.MAX_EPOCH]):
            if ep < step:
                break
        return s.LRS[ind - 1] * s.BASE_LR
    policies = {"cosine": cosine, "steps_with_relative_lrs": steps_with_relative_lrs}
    if s.LR_POLICY not in policies:
        raise NotImplementedError("svit_amd implements SOLVER.LR_POLICY 'cosine' and 'steps_with_relative_lrs', got %r"
                                  % (s.LR_POLICY,))
    policy = policies[s.LR_POLICY]
    lr = policy(cur_epoch)
    if cur_epoch < s.WARMUP_EPOCHS:
        lr_end = policy(s.WARMUP_EPOCHS)
        alpha = (lr_end - s.WARMUP_START_LR) / s.WARMUP_EPOCHS
        lr = cur_epoch * alpha + s.WARMUP_START_LR
    return {"lr": lr}


class FusedClipAdamW:
    """torch.optim-like surface (`param_groups`, `zero_grad`, `step`, `state_dict`) over the
    model's FlatParams.  Semantics = clip_grad_norm_(max_norm) + torch.optim.AdamW(eps=1e-8).

    Parameters with `requires_grad = False` (read here, once: svit_amd/freeze.py) are left out as the reference leaves
    them out (slowfast/models/optimizer.py:39-76): never decayed, no moments, not in the clip norm, not in
    `state_dict()`.  The kernels then run on `segments`, the trainable ranges of the flat buffers.

    lr_scale: a callable name -> float (svit_amd/lrscale.py: layer-wise lr decay, per-prefix multipliers).  An element
    is stepped with float32(lr of its group) * float32(scale of its parameter); `param_groups` stays the two entries
    `set_lr` writes, the scales live in `lr_segments` int64 [S, 2] / `lr_scales` float32 [S], fixed here.  None, or 1.0
    for every trainable parameter: no table, and the optimizer is the one it was without the argument."""

    # what a solver keeps per parameter, as its torch twin's checkpoint names it = the flat buffers of these names
    STATE = ("exp_avg", "exp_avg_sq")
    STEP_IN_STATE = True        # every state entry carries the solver's step counter

    def __init__(self, model, lr, weight_decay=1e-4, betas=(0.9, 0.999), eps=1e-8,
                 clip_grad_l2norm=None, grad_scale=1.0, lr_scale=None):
        core = model.module if hasattr(model, "module") else model
        self.model, self.flat = core, core.flat
        if self.flat is None:
            raise RuntimeError("FusedClipAdamW needs a finalized (on-GPU) SViT")
        # the frozen set the flags describe: NotImplementedError for an unsupported pattern, ValueError for none trainable
        # (a bare holder of flat buffers, as tools and tests build one, has no flags to read: nothing frozen)
        self.cut = core.frozen_cut() if hasattr(core, "frozen_cut") else 0
        self.segments = core.trainable_segments(self.cut) if self.cut else None
        self.lr_segments = self.lr_scales = self._name_scale = None
        if lr_scale is not None:
            scales = lrscale.name_scales(self.flat.slots, lr_scale)
            tab = lrscale.table(self.flat.slots, self.flat.n_decay, scales, self.segments)
            if tab is not None:
                self.lr_segments, self.lr_scales = tab
                self._name_scale = scales
        self.betas, self.eps = betas, eps
        self.clip = clip_grad_l2norm
        self.grad_scale = grad_scale
        n = self.flat.total
        dev = self.flat.data.device
        for key in self.STATE:
            setattr(self, key, torch.zeros(n, device=dev))
        self.sumsq = torch.zeros(1, device=dev)
        self.step_count = 0
        nd = self.flat.n_decay
        self.param_groups = [
            {"lr": lr, "weight_decay": weight_decay, "range": (0, nd)},
            {"lr": lr, "weight_decay": 0.0, "range": (nd, n)},
        ]

    def zero_grad(self, set_to_none=False):
        self.flat.grad.zero_()

    @torch.no_grad()
    def step(self):
        self.step_count += 1
        f = self.flat
        sumsq = None
        if self.clip is not None and self.clip > 0:
            self.sumsq.zero_()
            ops.sumsq(f.grad, self.sumsq)
            sumsq = self.sumsq      # (over the whole buffer also with frozen parameters: their gradients are zero)
        for g, a, b in self._launches():
            ops.adamw_step(f.data[a:b], f.grad[a:b], self.exp_avg[a:b], self.exp_avg_sq[a:b], sumsq,
                           float(self.clip or 0.0), g["lr"], self.betas[0], self.betas[1], self.eps,
                           g["weight_decay"], self.step_count, self.grad_scale)

    def _launches(self):
        """(param group, begin, end) of the AdamW launches of a step: one per weight-decay group, or -- with frozen
        parameters -- one per trainable segment (a segment never crosses the groups' boundary), or -- with learning-rate
        scales -- one per range of the table, the group's lr replaced by the fp32 product the guarded tail forms"""
        if self.lr_segments is not None:
            nd, out = self.flat.n_decay, []
            for (a, b), c in zip(self.lr_segments, self.lr_scales):
                g = self.param_groups[0 if a < nd else 1]
                out.append((dict(g, lr=float(np.float32(g["lr"]) * c)), int(a), int(b)))
            return out
        if self.segments is None:
            return [(g,) + tuple(g["range"]) for g in self.param_groups if g["range"][1] > g["range"][0]]
        nd = self.flat.n_decay
        return [(self.param_groups[0 if a < nd else 1], int(a), int(b)) for a, b in self.segments]

    def grad_norm(self):
        """host value of the last clipped step's global grad norm (forces a sync; logging only)."""
        return float(self.sumsq.sqrt()) * self.grad_scale

    # ---- checkpoint format of torch.optim.AdamW as the reference builds it -------------------
    def _order(self):
        """state index -> parameter name: the reference's two groups (decayed, then 1-D / bias;
        slowfast/models/optimizer.py:39-72), each in named_parameters() order."""
        named = [(n, tuple(p.shape)) for n, p in self.model.named_parameters()]
        if self.cut:        # the reference's optim_params: the trainable parameters alone
            depth = len(self.model.plan.blocks)
            named = [(n, s) for n, s in named if freeze.position(n, depth) >= self.cut]
        wd = self.model.weight_decayed       # same predicate that laid out the flat buffers
        dec = [n for n, s in named if wd(n, s)]
        return dec, [n for n, s in named if not wd(n, s)]

    def state_dict(self):
        """The dict torch.optim.AdamW.state_dict() yields for the reference's optimizer (what a
        released .pyth holds under "optimizer_state"): per-parameter step / exp_avg / exp_avg_sq
        (views of the flat moment buffers) and two param groups of indices."""
        dec, rest = self._order()
        state = {}
        if self.step_count > 0 and self.STATE:
            for j, n in enumerate(dec + rest):
                state[j] = {"step": torch.tensor(float(self.step_count))} if self.STEP_IN_STATE else {}
                for key in self.STATE:
                    state[j][key] = self.flat.view(getattr(self, key), n)
        groups, base = [], 0
        for g, names in zip(self.param_groups, (dec, rest)):
            if not names:
                continue
            # with learning-rate scales each group splits by distinct scale, in order of first appearance, into
            # torch-shaped groups: "lr" is the effective rate, "layer_decay" the scale
            split = {}
            for j, n in enumerate(names, base):
                split.setdefault(None if self._name_scale is None else self._name_scale[n], []).append(j)
            for c, idx in split.items():
                grp = self._group(g["lr"] if c is None else float(np.float32(g["lr"]) * c), g["weight_decay"])
                grp["params"] = idx
                if c is not None:
                    grp["layer_decay"] = float(c)
                groups.append(grp)
            base += len(names)
        return {"state": state, "param_groups": groups}

    def _group(self, lr, weight_decay):
        """a param group of torch.optim.AdamW.state_dict() but for "params", keys in torch's order"""
        return {"lr": lr, "betas": tuple(self.betas), "eps": self.eps, "weight_decay": weight_decay, "amsgrad": False,
                "maximize": False, "foreach": None, "capturable": False, "differentiable": False, "fused": None,
                "decoupled_weight_decay": True}

    def load_state_dict(self, sd):
        """either form of `param_groups` -- the reference's two groups or groups split by "layer_decay" -- whatever this
        optimizer's own scales are: moments go by index, the base lr of a weight-decay group is `lr / layer_decay` of its
        first subgroup"""
        dec, rest = self._order()
        order = dec + rest
        n_listed = sum(len(g["params"]) for g in sd["param_groups"])
        if n_listed != len(order):
            raise ValueError("optimizer state lists %d parameters, the model has %d" % (n_listed, len(order)))
        state = sd["state"]
        for key in self.STATE:
            getattr(self, key).zero_()
        step, found = 0, False
        for j, n in enumerate(order):
            ent = state.get(j, state.get(str(j)))
            if ent is None:
                continue
            want = self.flat.slots[n][2]
            for key in self.STATE:
                if key not in ent:
                    raise ValueError("optimizer state %d (%s) holds %s and no %s: it was written by another solver"
                                     % (j, n, sorted(ent), key))
                if tuple(ent[key].shape) != tuple(want):      # copy_ would silently broadcast [96] -> [1,1,96]
                    raise ValueError("optimizer state %d (%s): %s has shape %s, the parameter %s -- the "
                                     "checkpoint's parameter order / decay groups differ from this model's"
                                     % (j, n, key, tuple(ent[key].shape), tuple(want)))
                self.flat.view(getattr(self, key), n).copy_(ent[key])
            found = bool(self.STATE)
            if self.STEP_IN_STATE:
                step = max(step, int(ent["step"]))
        if self.STEP_IN_STATE:
            self.step_count = step
        elif found:             # loaded momentum buffers: the next step is not the one that initialises them
            self.step_count = max(self.step_count, 1)
        elif self.STATE:        # a state without buffers (torch: momentum_buffer None): zeroed above, the next step is "first"
            self.step_count = 0
        seen = set()
        for src in sd["param_groups"]:
            if not src["params"]:
                continue
            which = 0 if int(src["params"][0]) < len(dec) else 1
            if which not in seen:
                seen.add(which)
                self.param_groups[which]["lr"] = src["lr"] / src.get("layer_decay", 1.0)


def pack_step_host(lr, weight_decay, max_norm, clip_value, grad_scale):
    """the 32 bytes of svit_step_host (include/svit_hip.h) as float32 [8]; lr / weight_decay: (decayed group, the rest).
    A clip value switches norm clipping off, the reference's precedence (tools/train_net.py:139-147)."""
    clip_value = float(clip_value or 0.0)
    max_norm = 0.0 if clip_value > 0 else float(max_norm or 0.0)
    return np.array([lr[0], lr[1], weight_decay[0], weight_decay[1], max_norm, clip_value, grad_scale, 0.0],
                    dtype=np.float32)


class GuardedClipAdamW(FusedClipAdamW):
    """FusedClipAdamW whose step is dropped on the device when a gradient is not finite, as `GradScaler.step` drops
    it: weights, moments and `step_count` stay as they were, `skipped` counts it.  Two launches of the sum of squares
    (the second also takes the decision) and ONE AdamW launch over both weight-decay groups, every scalar read from
    the step record (svit_step_host uploaded by `upload()`, svit_step_dev owned by the kernels).  Nothing here
    synchronises except the read-outs: `step_count`, `stats()`, `grad_norm()`, `check()`, `state_dict()`.

    clip_grad_value: clip_grad_value_ bound (cfg.SOLVER.CLIP_GRAD_VAL); it replaces norm clipping when set.
    max_consecutive_skips: `check()` raises once that many steps in a row were dropped -- the deferred form of the
    reference's check_nan_losses (a NaN loss gives NaN gradients, thus a dropped step).  None: never raises."""

    RING = 16
    ema = None          # the ema.WeightEMA `attach_ema` hung behind the step: every enqueue() ends with its launch
    _averaged = None    # the ema.WeightEMA whose average stands in the weights' place (ema.average_weights()): no step
    monitor = None      # the monitor.TensorMonitor `attach_monitor` hung behind the guard: two launches before the solver's
    act_monitor = None  # the actmon.ActivationMonitor bound by model.attach_activation_monitor: check() asks it for the origin
    update_monitor = None   # the updmon.UpdateMonitor `attach_update_monitor` hung around the solver's launch: one launch in
    #                         front of it, two behind

    def __init__(self, model, lr, weight_decay=1e-4, betas=(0.9, 0.999), eps=1e-8, clip_grad_l2norm=None,
                 grad_scale=1.0, clip_grad_value=None, max_consecutive_skips=None, lr_scale=None):
        super().__init__(model, lr, weight_decay=weight_decay, betas=betas, eps=eps,
                         clip_grad_l2norm=clip_grad_l2norm, grad_scale=grad_scale, lr_scale=lr_scale)
        self.clip_value = clip_grad_value
        self.max_consecutive_skips = max_consecutive_skips
        dev = self.flat.data.device
        self._records()
        self.host_rec = torch.from_numpy(self._pack()).to(dev)
        # bias corrections of steps 1, 2, ...: tabulated once on the host, by the code the classic step runs per call
        self.bias_table = torch.from_numpy(self._bias_pairs()).to(dev)
        self._ws = torch.zeros(1024, device=dev)
        self._slots, self._events, self._next = None, [None] * self.RING, 0
        if dev.type == "cuda":
            self._warm()

    def _bias_pairs(self):
        return ops.adamw_bias_table(self.betas[0], self.betas[1])

    def _records(self):
        """svit_step_dev as int32 [12] (created on first use: the base constructor already assigns step_count)"""
        if "dev_rec" not in self.__dict__:
            self.dev_rec = torch.zeros(12, dtype=torch.int32, device=self.flat.data.device)
        return self.dev_rec

    def _warm(self):
        """one launch of each kernel on four dummy elements, so that a later stream capture meets loaded code; the
        optimizer's own record and buffers are not touched"""
        dev = self.flat.data.device
        z = torch.zeros(4, 4, device=dev)
        rec = torch.zeros(12, dtype=torch.int32, device=dev)
        ops.step_guard(z[1], self.host_rec, rec, self.bias_table, self._ws)
        ops.adamw_step_guarded(z[0], z[1], z[2], z[3], 2, self.host_rec, rec, self.betas[0], self.betas[1], self.eps)
        if self.segments is not None:
            seg = np.array([[0, 4]], dtype=np.int64)
            ops.step_guard_seg(z[1], seg, self.host_rec, rec, self.bias_table, self._ws)
            ops.adamw_step_guarded_seg(z[0], z[1], z[2], z[3], 4, seg, self.host_rec, rec, self.betas[0], self.betas[1],
                                       self.eps)
        if self.lr_segments is not None:
            ops.adamw_step_guarded_lr(z[0], z[1], z[2], z[3], 4, np.array([[0, 4]], dtype=np.int64),
                                      np.ones(1, dtype=np.float32), self.host_rec, rec, self.betas[0], self.betas[1],
                                      self.eps)

    def _pack(self):
        g = self.param_groups
        return pack_step_host((g[0]["lr"], g[1]["lr"]), (g[0]["weight_decay"], g[1]["weight_decay"]),
                              self.clip, self.clip_value, self.grad_scale)

    # ---- the step: upload() + enqueue(); a GraphedTrainStep holds enqueue() in its graph and calls upload() ------
    def upload(self):
        """send this step's lr / weight decay / clip bounds / grad scale, in stream order, without stalling the host:
        a ring of pinned slots, each guarded by the event of the copy that last read it"""
        if self._averaged is not None:
            raise RuntimeError("the weights hold their moving average (inside WeightEMA.average_weights()): an optimizer "
                               "step or a replay of the training step here would train the average -- leave the context "
                               "first")
        if self._slots is None:
            self._slots = torch.empty((self.RING, 8), dtype=torch.float32).pin_memory()
        i = self._next
        self._next = (i + 1) % self.RING
        if self._events[i] is not None:
            self._events[i].synchronize()
        self._slots[i].copy_(torch.from_numpy(self._pack()))
        self.host_rec.copy_(self._slots[i], non_blocking=True)
        ev = torch.cuda.Event()
        ev.record(torch.cuda.current_stream(self.host_rec.device))
        self._events[i] = ev

    def attach_ema(self, ema):
        """ema: an ema.WeightEMA built over this optimizer -- every `enqueue()` from now on ends with its launch (one
        more, behind the solver's), so the eager step, a GraphedTrainStep(optimizer=) captured AFTERWARDS and an
        AccumulatedTrainStep carry the average along; a step captured before refuses its replay.  None: detach."""
        if ema is not None and getattr(ema, "optimizer", None) is not self:
            raise ValueError("attach_ema: the WeightEMA was built over another optimizer (its update count is derived "
                             "from that optimizer's step record)")
        self.ema = ema

    def attach_monitor(self, monitor):
        """monitor: a monitor.TensorMonitor built over this optimizer -- every `enqueue()` from now on issues its two
        launches between the guard and the solver's launch, so the eager step, a GraphedTrainStep(optimizer=) captured
        AFTERWARDS and an AccumulatedTrainStep record the statistics; a step captured before refuses its replay.  None:
        detach."""
        if monitor is not None and getattr(monitor, "optimizer", None) is not self:
            raise ValueError("attach_monitor: the TensorMonitor was built over another optimizer (its step index is "
                             "derived from that optimizer's step record)")
        self.monitor = monitor

    def attach_update_monitor(self, monitor):
        """monitor: an updmon.UpdateMonitor built over this optimizer -- every `enqueue()` from now on issues its snapshot
        in front of the solver's launch and its two statistics launches directly behind it (in front of the average's), so
        the eager step, a GraphedTrainStep(optimizer=) captured AFTERWARDS and an AccumulatedTrainStep record what the
        solver did; a step captured before refuses its replay.  None: detach."""
        if monitor is not None and getattr(monitor, "optimizer", None) is not self:
            raise ValueError("attach_update_monitor: the UpdateMonitor was built over another optimizer (its step index is "
                             "derived from that optimizer's step record)")
        self.update_monitor = monitor

    def enqueue(self):
        """the three launches (with the attached monitor's two between the guard and the solver's, the attached update
        monitor's one in front of the solver's and two behind it, and the attached average's one last); allocation-free
        and capturable"""
        self._solve()
        if self.ema is not None:
            self.ema.enqueue()

    def _watch(self):
        """the attached monitor's launches: behind the guard, so the record is this step's, and in front of the solver, so
        the weights are those the gradient was taken at"""
        if self.monitor is not None:
            self.monitor.enqueue()

    def _snap(self):
        """the attached update monitor's snapshot: the weights in front of the solver's launch"""
        if self.update_monitor is not None:
            self.update_monitor.snapshot()

    def _measure(self):
        """the attached update monitor's two launches: directly behind the solver's launch"""
        if self.update_monitor is not None:
            self.update_monitor.enqueue()

    def _solve(self):
        """the guard, the monitors' launches and the solver's launch"""
        f = self.flat
        self._guard()
        self._watch()
        self._snap()
        if self.lr_segments is not None:    # learning-rate scales: AdamW over the scaled ranges
            ops.adamw_step_guarded_lr(f.data, f.grad, self.exp_avg, self.exp_avg_sq, f.n_decay, self.lr_segments,
                                      self.lr_scales, self.host_rec, self.dev_rec, self.betas[0], self.betas[1], self.eps)
        elif self.segments is not None:     # frozen parameters: over the trainable segments
            ops.adamw_step_guarded_seg(f.data, f.grad, self.exp_avg, self.exp_avg_sq, f.n_decay, self.segments,
                                       self.host_rec, self.dev_rec, self.betas[0], self.betas[1], self.eps)
        else:
            ops.adamw_step_guarded(f.data, f.grad, self.exp_avg, self.exp_avg_sq, f.n_decay, self.host_rec,
                                   self.dev_rec, self.betas[0], self.betas[1], self.eps)
        self._measure()

    def _guard(self):
        """the sum of squares and the step's decision, over the trainable segments when part of the buffer is frozen"""
        if self.segments is not None:
            ops.step_guard_seg(self.flat.grad, self.segments, self.host_rec, self.dev_rec, self.bias_table, self._ws)
        else:
            ops.step_guard(self.flat.grad, self.host_rec, self.dev_rec, self.bias_table, self._ws)

    def _ranges(self):
        """(segs int64 [S, 2], scales float32 [S] or None) for the solvers that always walk a table: the scaled ranges,
        else the trainable segments, else the extent of each weight-decay group"""
        if self.lr_segments is not None:
            return self.lr_segments, self.lr_scales
        if self.segments is not None:
            return self.segments, None
        nd, n = self.flat.n_decay, self.flat.total
        return np.array([r for r in ((0, nd), (nd, n)) if r[1] > r[0]], dtype=np.int64).reshape(-1, 2), None

    @torch.no_grad()
    def step(self):
        self.upload()
        self.enqueue()

    # ---- read-outs (each synchronises) ---------------------------------------------------------------------------
    @property
    def step_count(self):
        """applied steps = AdamW's step counter; dropped steps do not advance it"""
        return int(self._records().view(torch.int64)[0])

    @step_count.setter
    def step_count(self, value):
        self._records().view(torch.int64)[0:1].fill_(int(value))

    def stats(self):
        r = hip.StepDev.from_buffer_copy(self.dev_rec.cpu().numpy().tobytes())
        return {"applied": r.applied, "skipped": r.skipped, "consecutive_skipped": r.consecutive,
                "grad_norm": r.grad_norm, "clip_coef": r.coef}

    def grad_norm(self):
        """host value of the global grad norm of the last APPLIED step (forces a sync; logging only)"""
        return self.stats()["grad_norm"]

    def check(self):
        """call once per LOG_PERIOD: raises when `max_consecutive_skips` or more steps in a row were dropped"""
        if self.max_consecutive_skips is None:
            return
        s = self.stats()
        if s["consecutive_skipped"] >= self.max_consecutive_skips:
            culprits = self.monitor.culprit_line() if self.monitor is not None else ""
            # (the step that was dropped last is the last step: its forward passes carry that index)
            origin = (self.act_monitor.origin_line(s["applied"] + s["skipped"] - 1)
                      if self.act_monitor is not None and s["consecutive_skipped"] > 0 else "")
            culprits = "\n".join(x for x in (culprits, origin) if x)
            raise RuntimeError("the last %d optimizer steps were dropped for non-finite gradients (limit %d; %d applied, "
                               "%d dropped in all, last finite grad norm %g)%s"
                               % (s["consecutive_skipped"], self.max_consecutive_skips, s["applied"], s["skipped"],
                                  s["grad_norm"], "\n" + culprits if culprits else ""))


# ---- SGD and Adam on the guarded tail (csrc/solver.hip) -------------------------------------------------------------
def _solver_grad(p, g, coef, wd, clip_value):
    gi = g * np.float32(coef)
    cv = np.float32(clip_value or 0.0)
    if cv > 0:
        gi = np.minimum(np.maximum(gi, -cv), cv)
    wd = np.asarray(wd, dtype=np.float32)
    return np.where(wd != 0, gi + p * wd, gi)


def sgd_step_host(p, g, buf, coef, lr_eff, wd, momentum=0.0, dampening=0.0, nesterov=False, first=False,
                  clip_value=0.0):
    """svit_sgd_step_guarded restated in NumPy float32, the kernel's yardstick: the same formulas in the same order, each
    operation rounded once.  p, g, buf: float32 arrays (buf None with momentum == 0); lr_eff, wd: float32 scalars or
    per-element arrays; coef and `first` as the guard's record has them.  -> (p, buf), new arrays"""
    p, g = np.asarray(p, dtype=np.float32), np.asarray(g, dtype=np.float32)
    gi = _solver_grad(p, g, coef, wd, clip_value)
    if momentum != 0:
        mom, omd = np.float32(momentum), np.float32(1) - np.float32(dampening)
        buf = gi.copy() if first else np.asarray(buf, dtype=np.float32) * mom + gi * omd
        gi = gi + buf * mom if nesterov else buf
    return p - gi * np.asarray(lr_eff, dtype=np.float32), buf


def adam_step_host(p, g, m, v, coef, bc1, bc2_sqrt, lr_eff, wd, betas=(0.9, 0.999), eps=1e-8, clip_value=0.0):
    """svit_adam_step_guarded restated in NumPy float32 (see sgd_step_host); bc1, bc2_sqrt: the pair of the step from
    ops.adamw_bias_table, as the guard's record has it.  -> (p, m, v), new arrays"""
    p, g = np.asarray(p, dtype=np.float32), np.asarray(g, dtype=np.float32)
    b1, b2 = np.float32(betas[0]), np.float32(betas[1])
    gi = _solver_grad(p, g, coef, wd, clip_value)
    m = np.asarray(m, dtype=np.float32) * b1 + gi * (np.float32(1) - b1)
    v = np.asarray(v, dtype=np.float32) * b2 + (gi * gi) * (np.float32(1) - b2)
    denom = np.sqrt(v) / np.float32(bc2_sqrt) + np.float32(eps)
    return p - (np.asarray(lr_eff, dtype=np.float32) / np.float32(bc1)) * (m / denom), m, v


class _GuardedRangeSolver(GuardedClipAdamW):
    """What GuardedClipAdam and GuardedClipSGD share: a step is the guard, then ONE launch (`_launch`, the subclass's) over
    the range table of `_ranges()`.  Everything around the update -- the step record and its upload, the drop of a
    non-finite step, `stats()`, `check()`, `grad_scale`, clipping, `lr_scale`, the frozen cut -- is GuardedClipAdamW's;
    its own AdamW launches (`_warm`, `enqueue`) are replaced here."""

    def _warm(self):
        dev = self.flat.data.device
        z = torch.zeros(4, 4, device=dev)
        rec = torch.zeros(12, dtype=torch.int32, device=dev)
        seg = np.array([[0, 4]], dtype=np.int64)
        ops.step_guard(z[1], self.host_rec, rec, self.bias_table, self._ws)
        if self.segments is not None:
            ops.step_guard_seg(z[1], seg, self.host_rec, rec, self.bias_table, self._ws)
        self._launch(z[0], z[1], [z[2], z[3]], 4, seg, None, rec)

    def _launch(self, p, g, state, n_decay, segs, scales, rec):
        """the solver's launch on p, g and `state` (one buffer per entry of STATE) with the step record `rec`"""
        raise NotImplementedError

    def _solve(self):
        """the guard's two launches and the solver's one; allocation-free and capturable"""
        f = self.flat
        self._guard()
        self._watch()
        self._snap()
        segs, scales = self._ranges()
        self._launch(f.data, f.grad, [getattr(self, key) for key in self.STATE], f.n_decay, segs, scales, self.dev_rec)
        self._measure()


class GuardedClipAdam(_GuardedRangeSolver):
    """torch.optim.Adam (weight decay added to the gradient, no amsgrad) on the guarded tail: the guard, then ONE launch
    of svit_adam_step_guarded over the range table."""

    def _launch(self, p, g, state, n_decay, segs, scales, rec):
        ops.adam_step_guarded(p, g, state[0], state[1], n_decay, segs, scales, self.host_rec, rec, self.betas[0],
                              self.betas[1], self.eps)

    def _group(self, lr, weight_decay):
        """a param group of torch.optim.Adam.state_dict()"""
        return dict(super()._group(lr, weight_decay), decoupled_weight_decay=False)


class GuardedClipSGD(_GuardedRangeSolver):
    """torch.optim.SGD (momentum, dampening, nesterov, weight decay added to the gradient) on the guarded tail: the guard,
    then ONE launch of svit_sgd_step_guarded.  One state buffer, `momentum_buffer`, or none with momentum == 0.  The
    first APPLIED step copies the gradient into the buffer (the device reads that off the step record), also after
    dropped steps.  Loading a checkpoint's buffers makes the next step an ordinary one; loading a state without buffers
    (torch's `momentum_buffer` of None) zeroes them and makes the next step "first" again.  No betas, no eps: both are
    None."""

    STEP_IN_STATE = False

    def __init__(self, model, lr, momentum=0.0, dampening=0.0, nesterov=False, weight_decay=0.0, clip_grad_l2norm=None,
                 grad_scale=1.0, clip_grad_value=None, max_consecutive_skips=None, lr_scale=None):
        if momentum < 0.0:
            raise ValueError("Invalid momentum value: %s" % (momentum,))
        if nesterov and (momentum <= 0 or dampening != 0):          # torch.optim.SGD's refusal, in its words
            raise ValueError("Nesterov momentum requires a momentum and zero dampening")
        self.momentum, self.dampening, self.nesterov = momentum, dampening, bool(nesterov)
        self.STATE = ("momentum_buffer",) if momentum != 0 else ()
        self.momentum_buffer = None
        super().__init__(model, lr, weight_decay=weight_decay, betas=None, eps=None, clip_grad_l2norm=clip_grad_l2norm,
                         grad_scale=grad_scale, clip_grad_value=clip_grad_value,
                         max_consecutive_skips=max_consecutive_skips, lr_scale=lr_scale)

    def _bias_pairs(self):
        """no bias corrections: a table of 0 entries, the guard then records 1.0 for both"""
        return np.zeros((0, 2), dtype=np.float32)

    def _launch(self, p, g, state, n_decay, segs, scales, rec):
        ops.sgd_step_guarded(p, g, state[0] if self.STATE else None, n_decay, segs, scales, self.host_rec, rec,
                             self.momentum, self.dampening, self.nesterov)

    def _group(self, lr, weight_decay):
        """a param group of torch.optim.SGD.state_dict()"""
        return {"lr": lr, "momentum": self.momentum, "dampening": self.dampening, "weight_decay": weight_decay,
                "nesterov": self.nesterov, "maximize": False, "foreach": None, "differentiable": False, "fused": None}


def construct_optimizer(model, cfg):
    """slowfast/models/optimizer.py:15-112.  `adamw`: the fused tail, guarded with SOLVER.CLIP_GRAD_VAL, the opt-in
    SVIT.GUARDED_STEP, SVIT.EMA_DECAY, SVIT.MONITOR or SVIT.UPDATE_MONITOR (none a key of the default tree, like
    SVIT.REPRODUCIBLE).  `sgd`
    and `adam`: always the guarded tail (GuardedClipSGD / GuardedClipAdam)."""
    s = cfg.SOLVER
    if not s.ZERO_WD_1D_PARAM:
        raise NotImplementedError("svit_amd lays its flat buffers out for SOLVER.ZERO_WD_1D_PARAM: True")
    if s.OPTIMIZING_METHOD not in ("sgd", "adam", "adamw"):
        raise NotImplementedError("Does not support {} optimizer".format(s.OPTIMIZING_METHOD))
    lr_scale = lr_scale_from_cfg(cfg)       # SOLVER.LAYER_DECAY / SVIT.LR_MULT (svit_amd/lrscale.py); None without them
    if s.OPTIMIZING_METHOD != "adamw":
        common = dict(lr=s.BASE_LR, weight_decay=s.WEIGHT_DECAY, clip_grad_l2norm=s.CLIP_GRAD_L2NORM,
                      clip_grad_value=s.CLIP_GRAD_VAL, lr_scale=lr_scale,
                      max_consecutive_skips=getattr(cfg.SVIT, "MAX_CONSECUTIVE_SKIPS", None))
        if s.OPTIMIZING_METHOD == "sgd":
            return GuardedClipSGD(model, momentum=s.MOMENTUM, dampening=s.DAMPENING, nesterov=s.NESTEROV, **common)
        return GuardedClipAdam(model, betas=(0.9, 0.999), eps=1e-8, **common)
    # (SVIT.EMA_DECAY: the moving average's update count is derived from the guarded tail's step record, svit_amd/ema.py;
    #  SVIT.MONITOR / SVIT.UPDATE_MONITOR: so is the step index of the per-tensor statistics, svit_amd/monitor.py and
    #  svit_amd/updmon.py)
    if (getattr(cfg.SVIT, "GUARDED_STEP", False) or cfg.SOLVER.CLIP_GRAD_VAL
            or getattr(cfg.SVIT, "EMA_DECAY", None) is not None or getattr(cfg.SVIT, "MONITOR", False)
            or getattr(cfg.SVIT, "UPDATE_MONITOR", False)):
        return GuardedClipAdamW(model, lr=cfg.SOLVER.BASE_LR, weight_decay=cfg.SOLVER.WEIGHT_DECAY,
                                clip_grad_l2norm=cfg.SOLVER.CLIP_GRAD_L2NORM, clip_grad_value=cfg.SOLVER.CLIP_GRAD_VAL,
                                max_consecutive_skips=getattr(cfg.SVIT, "MAX_CONSECUTIVE_SKIPS", None),
                                lr_scale=lr_scale)
    return FusedClipAdamW(model, lr=cfg.SOLVER.BASE_LR, weight_decay=cfg.SOLVER.WEIGHT_DECAY,
                          clip_grad_l2norm=cfg.SOLVER.CLIP_GRAD_L2NORM, lr_scale=lr_scale)


def set_lr(optimizer, new_lr):
    for g in optimizer.param_groups:
        g["lr"] = new_lr["lr"] if isinstance(new_lr, dict) else new_lr
