"""What the solver did to every tensor, measured inside the step, on the guarded optimizer tail.

    optimizer = optim.construct_optimizer(model, cfg)       # the guarded tail when SVIT.UPDATE_MONITOR is set
    monitor = build_update_monitor(cfg, optimizer)          # None without the key; attached to the optimizer otherwise
    ...
    rows = monitor.read()                                   # once per cfg.LOG_PERIOD: ONE device read
    monitor.by_layer(rows), monitor.stalled(rows)

Two launch groups (csrc/update.hip) bracket the solver's launch in `optimizer.enqueue()` -- in the eager step, in a
GraphedTrainStep's replay and in an AccumulatedTrainStep alike: svit_update_snapshot copies the weights of the trainable
segments into a shadow buffer in front of it, svit_update_stats' two launches behind it leave, per parameter tensor, the
fp64 sums of squares of the step Delta = p_new - p_old, of the new weights, of the gradient and of the first moment, the sum
of the second moment, the dot product of Delta and g, the largest |Delta| and two counts on the weights' bits -- the
elements that did not change at all and those that moved to an adjacent float -- in a row of a ring in device memory (the
layout: include/svit_hip.h).  No update rule is restated: the numbers are those of whatever solver ran in between.

Every `every`-th step is recorded when the guard applied it; on a dropped step nothing moves and nothing is recorded
(monitor.TensorMonitor records those).  The step index is TensorMonitor's, so rows of both join by step.  Nothing here
synchronises but `read()`, `reset()` and the constructor.  The reference has nothing like it: SVIT.UPDATE_MONITOR /
SVIT.UPDATE_MONITOR_EVERY are read with getattr and are not keys of the default tree.  Nothing is saved: no state_dict,
nothing in checkpoints.  The shadow buffer costs 4 bytes per parameter.
"""
import numpy as np
import torch

from . import ops
from .monitor import TensorRing, trainable_mask

HEADER = np.dtype([("step", "<i8"), ("flags", "<i4"), ("reserved", "<i4")])
ENTRY = np.dtype([("sumsq_d", "<f8"), ("sumsq_p", "<f8"), ("dot_dg", "<f8"), ("sumsq_g", "<f8"), ("sumsq_m", "<f8"),
                  ("sum_v", "<f8"), ("absmax_d", "<f4"), ("n_still", "<i4"), ("n_one_ulp", "<i4"), ("reserved", "<i4")])
SUMS = ("sumsq_d", "sumsq_p", "dot_dg", "sumsq_g", "sumsq_m", "sum_v")
HAS_M, HAS_V = 1, 2     # bits of the header's flags
MAX_STALLED = 8         # names in log_stats' line


def row_dtype(Tn):
    """a ring row of Tn tensors: 16 + 64 * Tn bytes"""
    return np.dtype([("head", HEADER), ("entry", ENTRY, (Tn,))])


def empty_ring(R, Tn):
    """the ring as the host writes it: no row written (step -1), no entry written (n_still -1)"""
    ring = np.zeros(R, dtype=row_dtype(Tn))
    ring["head"]["step"] = -1
    ring["entry"]["n_still"] = -1
    return ring


def ulp_key(x):
    """float32 -> int64 keys monotone in the float order, adjacent floats one apart: i ^ ((i >> 31) & 0x7fffffff) on the
    signed 32-bit image (-0.0 is the key below +0.0)"""
    i = np.ascontiguousarray(x, dtype=np.float32).view(np.int32)
    return (i ^ ((i >> 31) & np.int32(0x7fffffff))).astype(np.int64)


def _delta(p_old, p_new):
    return p_new.astype(np.float64) - p_old.astype(np.float64)


def update_host(p_old, p_new, g, m, v, table, segs=None, step=-1):
    """svit_update_stats restated in NumPy float64, the kernels' yardstick -> one ring row (row_dtype(Tn)): the header
    (`step` as given, the flags from m / v being there) and ENTRY [Tn].  m, v: arrays or None.  A frozen tensor keeps the
    entry of an empty ring."""
    f32 = lambda a: None if a is None else np.ascontiguousarray(a, dtype=np.float32)     # noqa: E731
    p_old, p_new, g, m, v = f32(p_old), f32(p_new), f32(g), f32(m), f32(v)
    table = np.asarray(table, dtype=np.int64).reshape(-1, 2)
    row = empty_ring(1, len(table))[0]
    row["head"] = (step, (HAS_M if m is not None else 0) | (HAS_V if v is not None else 0), 0)
    live = trainable_mask(table, segs)
    for t, (a, b) in enumerate(table):
        if not live[t]:
            continue
        po, pn = p_old[a:b], p_new[a:b]
        d, pd, gd = _delta(po, pn), pn.astype(np.float64), g[a:b].astype(np.float64)
        md = None if m is None else m[a:b].astype(np.float64)
        kd = ulp_key(pn) - ulp_key(po)
        row["entry"][t] = (float(np.sum(d * d)), float(np.sum(pd * pd)), float(np.sum(d * gd)), float(np.sum(gd * gd)),
                           0.0 if md is None else float(np.sum(md * md)),
                           0.0 if v is None else float(np.sum(v[a:b].astype(np.float64))),
                           np.abs(d).astype(np.float32).max(), int((pn.view(np.int32) == po.view(np.int32)).sum()),
                           int((np.abs(kd) == 1).sum()), 0)
    return row


def abs_terms_host(p_old, p_new, g, m, v, table, segs=None):
    """the sums of |term| the six sums of update_host are compared against -> ENTRY [Tn], its six doubles filled: only
    dot_dg's differs from the sum itself (sum |Delta * g|)"""
    row = update_host(p_old, p_new, g, m, v, table, segs)
    out = row["entry"].copy()
    p_old, p_new, g = (np.ascontiguousarray(a, dtype=np.float32) for a in (p_old, p_new, g))
    table = np.asarray(table, dtype=np.int64).reshape(-1, 2)
    live = trainable_mask(table, segs)
    for t, (a, b) in enumerate(table):
        if live[t]:
            out["dot_dg"][t] = float(np.sum(np.abs(_delta(p_old[a:b], p_new[a:b]) * g[a:b].astype(np.float64))))
    out["sum_v"] = np.abs(out["sum_v"])
    return out


class UpdateMonitor(TensorRing):
    """The shadow buffer and the statistics ring around `optimizer`'s solver launch.

    optimizer: an optim.GuardedClipAdamW or one of its subclasses (AdamW plain, over segments or with learning-rate
    scales; GuardedClipAdam; GuardedClipSGD).  period: rows of the ring, R -- cfg.LOG_PERIOD, the steps between two
    `read()`s.  every: a step is recorded when the guard applied it and its index (applied + dropped steps so far, from
    0) is a multiple of it.

    The moments are the optimizer's STATE buffers: (exp_avg, exp_avg_sq), (momentum_buffer,) or none.  Nothing is
    attached by the constructor: `optimizer.attach_update_monitor(monitor)` (or `build_update_monitor`) does that."""
    KEY = "UPDATE_MONITOR"
    row_dtype, empty_ring = staticmethod(row_dtype), staticmethod(empty_ring)
    workspace_bytes = staticmethod(ops.update_stats_workspace)

    def __init__(self, optimizer, period, every=1):
        super().__init__(optimizer, period, every)
        self.shadow = torch.zeros(self.flat.total, dtype=torch.float32, device=self.flat.data.device)

    def _moments(self):
        """(m, v): the optimizer's first and second state buffer, None where it keeps none"""
        state = [getattr(self.optimizer, key) for key in self.optimizer.STATE]
        return (state + [None, None])[:2]

    def _warm(self):
        """one call of each entry point on four dummy elements, so that a later stream capture meets loaded code; neither
        the ring nor the optimizer's record is touched (a record of zeros says: nothing is due)"""
        dev = self.flat.data.device
        z = torch.zeros(5, 4, device=dev)
        t = np.array([[0, 4]], dtype=np.int64)
        rec = torch.zeros(12, dtype=torch.int32, device=dev)
        m, v = self._moments()
        ops.update_snapshot(z[0], z[1], None, rec, 1)
        ops.update_stats(z[0], z[1], z[2], None if m is None else z[3], None if v is None else z[4],
                         torch.from_numpy(t).to(dev), t, None, rec, torch.zeros(16 + 64, dtype=torch.uint8, device=dev),
                         1, 1, torch.zeros(ops.update_stats_workspace(4, 1), dtype=torch.uint8, device=dev))

    def snapshot(self):
        """the launch in front of the solver's: shadow = the weights, when the step is due; allocation-free and capturable"""
        ops.update_snapshot(self.flat.data, self.shadow, self.segments, self.optimizer.dev_rec, self.every)

    def enqueue(self):
        """the two launches behind the solver's; allocation-free and capturable"""
        m, v = self._moments()
        ops.update_stats(self.flat.data, self.shadow, self.flat.grad, m, v, self.table_dev, self.table, self.segments,
                         self.optimizer.dev_rec, self.ring, self.period, self.every, self.workspace)

    def read(self):
        """the rows recorded since the last read, ordered by step, as a dict of arrays [rows, Tn] (frozen tensors masked):
        names, steps, flags, numel, update_norm = sqrt(sumsq_d), weight_norm = sqrt(sumsq_p), ratio = update_norm /
        weight_norm, cos_grad = -dot_dg / (update_norm * |g|) (1 for plain gradient descent), m_rms = sqrt(sumsq_m /
        numel), v_mean = sum_v / numel (both 0 without the moment: see flags), absmax, n_still, n_one_ulp, the six raw sums,
        and `lost`: how many multiples of `every` since the last read, up to the newest step the ring holds, have no row
        -- overwritten (R rows; an overrun is reported, not raised) or dropped by the guard, which a TensorMonitor's rows
        tell apart"""
        return super().read()

    def _dict(self, rows, lost):
        e, masked = rows["entry"], self._masked
        numel = self.numel.astype(np.float64)
        un, wn, gn = np.sqrt(e["sumsq_d"]), np.sqrt(e["sumsq_p"]), np.sqrt(e["sumsq_g"])
        with np.errstate(divide="ignore", invalid="ignore"):
            ratio, cos = un / wn, -e["dot_dg"] / (un * gn)
        out = {"names": list(self.names), "steps": rows["head"]["step"].copy(), "flags": rows["head"]["flags"].copy(),
               "numel": self.numel.copy(), "update_norm": masked(un), "weight_norm": masked(wn), "ratio": masked(ratio),
               "cos_grad": masked(cos), "m_rms": masked(np.sqrt(e["sumsq_m"] / numel)), "v_mean": masked(e["sum_v"] / numel),
               "absmax": masked(e["absmax_d"].copy()), "n_still": masked(e["n_still"].copy()),
               "n_one_ulp": masked(e["n_one_ulp"].copy()), "lost": lost}
        for key in SUMS:
            out[key] = masked(e[key].copy())
        return out

    def by_layer(self, rows):
        """rows (what `read()` gave) summed over lrscale's layer ids: depth + 2 groups -- 0 the stem, 1 + i block i,
        depth + 1 the rest -- of update_norm, weight_norm and ratio = update_norm / weight_norm, n_still and numel, each
        [rows, depth + 2]; a group whose tensors are all frozen is masked"""
        still = rows["n_still"].data
        (sd, sp, still, numel), mask = self._layer_sums(rows["sumsq_d"].data, rows["sumsq_p"].data, still,
                                                        np.broadcast_to(self.numel, still.shape))
        un, wn = np.sqrt(sd), np.sqrt(sp)
        with np.errstate(divide="ignore", invalid="ignore"):
            ratio = un / wn
        return {"steps": rows["steps"], "update_norm": np.ma.MaskedArray(un, mask=mask),
                "weight_norm": np.ma.MaskedArray(wn, mask=mask.copy()), "ratio": np.ma.MaskedArray(ratio, mask=mask.copy()),
                "n_still": np.ma.MaskedArray(still, mask=mask.copy()), "numel": np.ma.MaskedArray(numel, mask=mask.copy())}

    def stalled(self, rows, min_fraction=0.5):
        """[(step, name, n_still, numel)] for every watched tensor among the rows of which at least `min_fraction` of the
        elements kept their 32 bits through the step"""
        out = []
        for i, step in enumerate(rows["steps"]):
            still = np.ma.filled(rows["n_still"][i], -1)
            for t in np.flatnonzero((still >= 0) & (still >= min_fraction * self.numel)):
                out.append((int(step), self.names[t], int(still[t]), int(self.numel[t])))
        return out

    def log_stats(self, rows):
        """the JSON line train_epoch logs: the by_layer numbers of the last recorded step among `rows`, its stalled
        tensors (their number, the first MAX_STALLED by name) and the share of elements that did not move; None when there
        is no row"""
        if not len(rows["steps"]):
            return None
        layers, last = self.by_layer(rows), self._last
        step = int(rows["steps"][-1])
        stalled = [s for s in self.stalled(rows) if s[0] == step]
        live = ~self.frozen
        still = int(rows["n_still"].data[-1][live].sum())
        return {"_type": "train_update_stats", "step": step, "rows": int(len(rows["steps"])), "lost": int(rows["lost"]),
                "flags": int(rows["flags"][-1]), "update_norm": last(layers["update_norm"]),
                "weight_norm": last(layers["weight_norm"]), "ratio": last(layers["ratio"]),
                "still_fraction": float("%.6g" % (still / max(1, int(self.numel[live].sum())))),
                "n_stalled": len(stalled), "stalled": [[n, k, m] for _, n, k, m in stalled[:MAX_STALLED]]}

    update_host = staticmethod(update_host)


def build_update_monitor(cfg, optimizer):
    """SVIT.UPDATE_MONITOR (and SVIT.UPDATE_MONITOR_EVERY, default 1) -> an UpdateMonitor of cfg.LOG_PERIOD rows attached
    to `optimizer`, or None without the key: no shadow, no ring, not one launch more"""
    if not getattr(cfg.SVIT, "UPDATE_MONITOR", False):
        return None
    every = getattr(cfg.SVIT, "UPDATE_MONITOR_EVERY", 1)
    if isinstance(every, bool) or not isinstance(every, int) or every < 1:
        raise ValueError("SVIT.UPDATE_MONITOR_EVERY is a positive int, got %r" % (every,))
    if type(optimizer).__name__ == "FusedClipAdamW":
        raise TypeError("SVIT.UPDATE_MONITOR needs the guarded optimizer tail, got the classic FusedClipAdamW: build the "
                        "optimizer with optim.construct_optimizer(model, cfg) AFTER the key is set")
    mon = UpdateMonitor(optimizer, int(cfg.LOG_PERIOD), every=every)
    optimizer.attach_update_monitor(mon)
    return mon
