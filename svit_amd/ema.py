"""Exponential moving average of the weights on the guarded optimizer tail (timm's ModelEma inside the captured step).

    optimizer = optim.construct_optimizer(model, cfg)       # the guarded tail when SVIT.EMA_DECAY is set
    ema = build_ema(cfg, model, optimizer)                  # None without the key; attached to the optimizer otherwise
    ...
    train.eval_epoch(val_loader, model, val_meter, epoch, cfg, ema=ema)
    checkpoint.save_checkpoint(job, model, optimizer, epoch, cfg, ema=ema)

The average is ONE flat fp32 buffer beside `flat.data`, updated by ONE launch (svit_ema_step_guarded, csrc/solver.hip)
that `optimizer.enqueue()` issues behind the solver's: part of the eager step, of a GraphedTrainStep's replay and of an
AccumulatedTrainStep alike.  A step the guard dropped does not move it: the kernel reads the guard's decision and its
count of applied steps from the step record, nothing here synchronises or counts on the host.  The reference has no
EMA: SVIT.EMA_DECAY / SVIT.EMA_WARMUP are read with getattr and are not keys of the default tree.
"""
import contextlib
from collections import OrderedDict

import numpy as np
import torch

from . import ops


def ema_step_host(e, p, d):
    """svit_ema_step_guarded restated in NumPy float32, the kernel's yardstick: e * d + p * (1 - d), every operation
    rounded once, 1 - d first.  e, p: float32 arrays; d: the update's decay -> the new average, a new array"""
    e, p = np.asarray(e, dtype=np.float32), np.asarray(p, dtype=np.float32)
    d = np.float32(d)
    omd = np.float32(1) - d
    return e * d + p * omd


def decay_at(k, decay, table=None):
    """the decay of update k (clamped to 1 from below, as the kernel clamps it): table[k - 1] inside the warm-up table,
    `decay` past it -> np.float32"""
    k = max(int(k), 1)
    if table is not None and k <= len(table):
        return np.float32(table[k - 1])
    return np.float32(decay)


def _check_decay(decay):
    if not (isinstance(decay, (int, float)) and 0.0 < float(np.float32(decay)) < 1.0):
        raise ValueError("the EMA decay lies in (0, 1), got %r" % (decay,))
    return float(decay)


class WeightEMA:
    """The moving average of `model`'s weights behind `optimizer`'s step.

    decay: d of `ema = ema * d + w * (1 - d)`, fixed here.  warmup: update k takes min(decay, (1 + k) / (10 + k)), timm's
    ModelEmaV2 warm-up, from a table built once on the host (ops.ema_decay_table).  The buffer starts as a copy of the
    weights; under a frozen cut only the optimizer's trainable segments are ever updated, the frozen ranges keep that
    copy (which IS the frozen weights).  Learning-rate scales play no part.

    The optimizer is an optim.GuardedClipAdamW or one of its subclasses: `num_updates` is its count of applied steps
    plus an offset kept here in device memory, so the device alone knows whether the average moves.  Nothing is
    attached by the constructor: `optimizer.attach_ema(ema)` (or `build_ema`) does that."""

    def __init__(self, model, optimizer, decay=0.9999, warmup=False):
        from .optim import GuardedClipAdamW
        if not isinstance(optimizer, GuardedClipAdamW):
            raise TypeError("WeightEMA needs an optim.GuardedClipAdamW or one of its subclasses, got %s: only the guarded "
                            "tail keeps the step's decision and its count of applied steps in device memory (set "
                            "SVIT.GUARDED_STEP or SVIT.EMA_DECAY before construct_optimizer)" % type(optimizer).__name__)
        core = model.module if hasattr(model, "module") else model
        if optimizer.flat is not core.flat:
            raise ValueError("WeightEMA: the optimizer was built over another model")
        self.model, self.flat, self.optimizer = core, core.flat, optimizer
        self.decay, self.warmup = _check_decay(decay), bool(warmup)
        flat = self.flat
        dev = flat.data.device
        self.buf = flat.data.detach().clone()
        self.table_host = ops.ema_decay_table(self.decay) if self.warmup else None
        self.table = None if self.table_host is None else torch.from_numpy(self.table_host).to(dev)
        # {offset, reserved}: num_updates = the optimizer's applied steps + offset; written here, by reset() and by
        # load_state_dict() only
        self.ema_rec = torch.zeros(2, dtype=torch.int64, device=dev)
        self.segments = optimizer.segments if optimizer.segments is not None else np.array([[0, flat.total]],
                                                                                           dtype=np.int64)
        self._set_updates(0)
        if dev.type == "cuda":
            self._warm()

    def _warm(self):
        """one launch on four dummy elements, so that a later stream capture meets loaded code; neither the average nor
        the optimizer's record is touched"""
        dev = self.flat.data.device
        z = torch.zeros(2, 4, device=dev)
        rec = torch.zeros(12, dtype=torch.int32, device=dev)
        ops.ema_step_guarded(z[0], z[1], np.array([[0, 4]], dtype=np.int64), self.table, self.decay,
                             torch.zeros(2, dtype=torch.int64, device=dev), rec)

    def enqueue(self):
        """the one launch, behind the solver's; allocation-free and capturable"""
        ops.ema_step_guarded(self.buf, self.flat.data, self.segments, self.table, self.decay, self.ema_rec,
                             self.optimizer.dev_rec)

    # ---- the update count (each of these synchronises) -------------------------------------------------------------
    def _set_updates(self, n):
        self.ema_rec[0:1].fill_(int(n) - self.optimizer.step_count)

    @property
    def num_updates(self):
        return max(self.optimizer.step_count + int(self.ema_rec[0]), 0)

    def stats(self):
        """{"num_updates", "decay"}: the updates so far and the decay the last of them took (the first one's before any)"""
        n = self.num_updates
        return {"num_updates": n, "decay": float(decay_at(n, self.decay, self.table_host))}

    def reset(self):
        """start over from the current weights: a copy of them, num_updates 0"""
        self._not_averaged("reset()")
        with torch.no_grad():
            self.buf.copy_(self.flat.data)
        self._set_updates(0)

    def _not_averaged(self, what):
        if self.optimizer._averaged is not None:
            raise RuntimeError("%s inside average_weights(): the buffers have exchanged their contents -- leave the context "
                               "first" % what)

    # ---- evaluating with the average ---------------------------------------------------------------------------------
    def _exchange(self):
        with torch.no_grad():
            tmp = self.flat.data.clone()
            self.flat.data.copy_(self.buf)
            self.buf.copy_(tmp)
            self.model.engine.refresh_weights()

    @contextlib.contextmanager
    def average_weights(self):
        """Inside, the model computes with the averaged weights: the CONTENTS of `flat.data` and of the average are
        exchanged in place (torch copies through one temporary) and the bf16 mirrors refreshed, on exit they are
        exchanged back -- bit for bit what they were.  No pointer moves, so captured graphs stay valid and the
        parameter views show the averaged values.  `optimizer.upload()` raises inside: neither an eager step nor a
        replay of the training step can train the average."""
        opt = self.optimizer
        if opt._averaged is not None:
            raise RuntimeError("average_weights(): the weights already hold a moving average (the context does not nest)")
        if self.model.engine is None:
            raise RuntimeError("average_weights() needs a finalized (on-GPU) SViT")
        self._exchange()
        opt._averaged = self
        try:
            yield self
        finally:
            opt._averaged = None
            self._exchange()

    # ---- state -------------------------------------------------------------------------------------------------------
    def state_dict(self):
        """{"decay", "warmup", "num_updates", "model_state"}; model_state: the model's own state_dict() names and shapes
        (frozen parameters included) over views of the average, so it loads into the model -- the reference's too"""
        own = self.model.state_dict()
        # (inside average_weights() the two buffers have exchanged their contents: the average lies in flat.data)
        avg = self.flat.data if self.optimizer._averaged is self else self.buf
        state = OrderedDict((k, self.flat.view(avg, k) if k in self.flat.slots else v) for k, v in own.items())
        return {"decay": self.decay, "warmup": self.warmup, "num_updates": self.num_updates, "model_state": state}

    def load_state_dict(self, sd):
        """copies the averaged tensors in and continues the count: offset = num_updates - the optimizer's applied steps
        as of now (so load the optimizer first).  The decay and the warm-up are this object's: a state written under
        others is refused, its count would point into another table."""
        self._not_averaged("load_state_dict()")
        if np.float32(sd["decay"]) != np.float32(self.decay) or bool(sd["warmup"]) != self.warmup:
            raise ValueError("the EMA state was written with decay %r, warmup %r; this WeightEMA was built with %r, %r"
                             % (sd["decay"], sd["warmup"], self.decay, self.warmup))
        state = sd["model_state"]
        missing = [k for k in self.flat.slots if k not in state]
        if missing:
            raise KeyError("the EMA state lacks %d of the model's parameters, the first is %s" % (len(missing), missing[0]))
        with torch.no_grad():
            for k, (_, _, shape) in self.flat.slots.items():
                if tuple(state[k].shape) != tuple(shape):
                    raise ValueError("the EMA state's %s has shape %s, the parameter %s"
                                     % (k, tuple(state[k].shape), tuple(shape)))
                self.flat.view(self.buf, k).copy_(state[k])
        self._set_updates(int(sd["num_updates"]))


def build_ema(cfg, model, optimizer):
    """SVIT.EMA_DECAY (and SVIT.EMA_WARMUP, default False) -> a WeightEMA attached to `optimizer`, or None without the
    key: no table, no buffer, not one launch more"""
    decay = getattr(cfg.SVIT, "EMA_DECAY", None)
    if decay is None:
        return None
    if not (isinstance(decay, (int, float)) and not isinstance(decay, bool) and 0.0 < decay < 1.0):
        raise ValueError("SVIT.EMA_DECAY lies in (0, 1), got %r" % (decay,))
    ema = WeightEMA(model, optimizer, decay=decay, warmup=bool(getattr(cfg.SVIT, "EMA_WARMUP", False)))
    optimizer.attach_ema(ema)
    return ema
