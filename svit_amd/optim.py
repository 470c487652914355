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
    """slowfast/utils/lr_policy.py:9-66 (cosine policy with optional linear warm-up)."""
    s = cfg.SOLVER

    def cosine(ep):
        offset = s.WARMUP_EPOCHS if s.COSINE_AFTER_WARMUP else 0.0
        assert s.COSINE_END_LR < s.BASE_LR
        return s.COSINE_END_LR + (s.BASE_LR - s.COSINE_END_LR) * (
            math.cos(math.pi * (ep - offset) / (s.MAX_EPOCH - offset)) + 1.0) * 0.5
    if s.LR_POLICY != "cosine":
        raise NotImplementedError("svit_amd implements SOLVER.LR_POLICY == 'cosine'")
    lr = cosine(cur_epoch)
    if cur_epoch < s.WARMUP_EPOCHS:
        lr_end = cosine(s.WARMUP_EPOCHS)
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
        self.exp_avg = torch.zeros(n, device=dev)
        self.exp_avg_sq = torch.zeros(n, device=dev)
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
        if self.step_count > 0:
            for j, n in enumerate(dec + rest):
                state[j] = {"step": torch.tensor(float(self.step_count)),
                            "exp_avg": self.flat.view(self.exp_avg, n),
                            "exp_avg_sq": self.flat.view(self.exp_avg_sq, n)}
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
                grp = {"lr": g["lr"] if c is None else float(np.float32(g["lr"]) * c),
                       "betas": tuple(self.betas), "eps": self.eps,
                       "weight_decay": g["weight_decay"], "amsgrad": False, "maximize": False,
                       "foreach": None, "capturable": False, "differentiable": False,
                       "fused": None, "decoupled_weight_decay": True,
                       "params": idx}
                if c is not None:
                    grp["layer_decay"] = float(c)
                groups.append(grp)
            base += len(names)
        return {"state": state, "param_groups": groups}

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
        self.exp_avg.zero_()
        self.exp_avg_sq.zero_()
        step = 0
        for j, n in enumerate(order):
            ent = state.get(j, state.get(str(j)))
            if ent is None:
                continue
            want = self.flat.slots[n][2]
            for key in ("exp_avg", "exp_avg_sq"):     # copy_ would silently broadcast [96] -> [1,1,96]
                if tuple(ent[key].shape) != tuple(want):
                    raise ValueError("optimizer state %d (%s): %s has shape %s, the parameter %s -- the "
                                     "checkpoint's parameter order / decay groups differ from this model's"
                                     % (j, n, key, tuple(ent[key].shape), tuple(want)))
            self.flat.view(self.exp_avg, n).copy_(ent["exp_avg"])
            self.flat.view(self.exp_avg_sq, n).copy_(ent["exp_avg_sq"])
            step = max(step, int(ent["step"]))
        self.step_count = step
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
        self.bias_table = torch.from_numpy(ops.adamw_bias_table(betas[0], betas[1])).to(dev)
        self._ws = torch.zeros(1024, device=dev)
        self._slots, self._events, self._next = None, [None] * self.RING, 0
        if dev.type == "cuda":
            self._warm()

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

    def enqueue(self):
        """the three launches; allocation-free and capturable"""
        f = self.flat
        if self.lr_segments is not None:    # learning-rate scales: today's guard, then AdamW over the scaled ranges
            if self.segments is not None:
                ops.step_guard_seg(f.grad, self.segments, self.host_rec, self.dev_rec, self.bias_table, self._ws)
            else:
                ops.step_guard(f.grad, self.host_rec, self.dev_rec, self.bias_table, self._ws)
            ops.adamw_step_guarded_lr(f.data, f.grad, self.exp_avg, self.exp_avg_sq, f.n_decay, self.lr_segments,
                                      self.lr_scales, self.host_rec, self.dev_rec, self.betas[0], self.betas[1], self.eps)
            return
        if self.segments is not None:       # frozen parameters: the same two steps over the trainable segments
            ops.step_guard_seg(f.grad, self.segments, self.host_rec, self.dev_rec, self.bias_table, self._ws)
            ops.adamw_step_guarded_seg(f.data, f.grad, self.exp_avg, self.exp_avg_sq, f.n_decay, self.segments,
                                       self.host_rec, self.dev_rec, self.betas[0], self.betas[1], self.eps)
            return
        ops.step_guard(f.grad, self.host_rec, self.dev_rec, self.bias_table, self._ws)
        ops.adamw_step_guarded(f.data, f.grad, self.exp_avg, self.exp_avg_sq, f.n_decay, self.host_rec, self.dev_rec,
                               self.betas[0], self.betas[1], self.eps)

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
            raise RuntimeError("the last %d optimizer steps were dropped for non-finite gradients (limit %d; %d applied, "
                               "%d dropped in all, last finite grad norm %g)"
                               % (s["consecutive_skipped"], self.max_consecutive_skips, s["applied"], s["skipped"],
                                  s["grad_norm"]))


def construct_optimizer(model, cfg):
    """slowfast/models/optimizer.py:15-112 for the configuration the SViT recipe uses.  SOLVER.CLIP_GRAD_VAL, or the
    opt-in SVIT.GUARDED_STEP (not a key of the default tree, like SVIT.REPRODUCIBLE), selects the guarded tail."""
    if cfg.SOLVER.OPTIMIZING_METHOD != "adamw" or not cfg.SOLVER.ZERO_WD_1D_PARAM:
        raise NotImplementedError("svit_amd fuses the configs/ssv2.yaml solver (adamw, ZERO_WD_1D_PARAM)")
    lr_scale = lr_scale_from_cfg(cfg)       # SOLVER.LAYER_DECAY / SVIT.LR_MULT (svit_amd/lrscale.py); None without them
    if getattr(cfg.SVIT, "GUARDED_STEP", False) or cfg.SOLVER.CLIP_GRAD_VAL:
        return GuardedClipAdamW(model, lr=cfg.SOLVER.BASE_LR, weight_decay=cfg.SOLVER.WEIGHT_DECAY,
                                clip_grad_l2norm=cfg.SOLVER.CLIP_GRAD_L2NORM, clip_grad_value=cfg.SOLVER.CLIP_GRAD_VAL,
                                max_consecutive_skips=getattr(cfg.SVIT, "MAX_CONSECUTIVE_SKIPS", None),
                                lr_scale=lr_scale)
    return FusedClipAdamW(model, lr=cfg.SOLVER.BASE_LR, weight_decay=cfg.SOLVER.WEIGHT_DECAY,
                          clip_grad_l2norm=cfg.SOLVER.CLIP_GRAD_L2NORM, lr_scale=lr_scale)


def set_lr(optimizer, new_lr):
    for g in optimizer.param_groups:
        g["lr"] = new_lr["lr"] if isinstance(new_lr, dict) else new_lr
