"""Per-tensor gradient and weight statistics inside the step, on the guarded optimizer tail.

    optimizer = optim.construct_optimizer(model, cfg)       # the guarded tail when SVIT.MONITOR is set
    monitor = build_monitor(cfg, optimizer)                 # None without the key; attached to the optimizer otherwise
    ...
    rows = monitor.read()                                   # once per cfg.LOG_PERIOD: ONE device read
    monitor.by_layer(rows), monitor.culprits(rows)

Two launches (svit_tensor_stats, csrc/monitor.hip) that `optimizer.enqueue()` issues between the guard and the solver's
launch -- part of the eager step, of a GraphedTrainStep's replay and of an AccumulatedTrainStep alike -- write, per
parameter tensor, the fp64 sums of squares of the gradient and of the weights, the largest finite |g|, the number of
non-finite gradient elements and the offset of the first one into a row of a ring in device memory (the layout:
include/svit_hip.h).  Every `every`-th step is recorded, and every step the guard dropped.  Nothing here synchronises but
`read()`, `reset()` and the constructor.  The reference has nothing like it: SVIT.MONITOR / SVIT.MONITOR_EVERY are read
with getattr and are not keys of the default tree.  Nothing is saved: no state_dict, nothing in checkpoints.
"""
import numpy as np
import torch

from . import lrscale, ops

HEADER = np.dtype([("step", "<i8"), ("apply", "<i4"), ("reserved", "<i4")])
ENTRY = np.dtype([("sumsq_g", "<f8"), ("sumsq_p", "<f8"), ("absmax_g", "<f4"), ("n_bad", "<i4"), ("first_bad", "<i4"),
                  ("reserved", "<i4")])
MAX_CULPRITS = 8        # names in check()'s message


def row_dtype(Tn):
    """a ring row of Tn tensors: 16 + 32 * Tn bytes"""
    return np.dtype([("head", HEADER), ("entry", ENTRY, (Tn,))])


def empty_ring(R, Tn):
    """the ring as the host writes it: no row written (step -1), no entry written (n_bad -1, first_bad -1)"""
    ring = np.zeros(R, dtype=row_dtype(Tn))
    ring["head"]["step"] = -1
    ring["entry"]["n_bad"] = -1
    ring["entry"]["first_bad"] = -1
    return ring


def trainable_mask(table, segs):
    """bool [Tn]: a tensor is trainable when its begin lies inside a segment; segs None or empty: all are"""
    table = np.asarray(table, dtype=np.int64).reshape(-1, 2)
    if segs is None or len(segs) == 0:
        return np.ones(len(table), dtype=bool)
    segs = np.asarray(segs, dtype=np.int64).reshape(-1, 2)
    b = table[:, 0][:, None]
    return ((b >= segs[None, :, 0]) & (b < segs[None, :, 1])).any(axis=1)


def stats_host(g, p, table, segs=None):
    """svit_tensor_stats restated in NumPy float64, the kernels' yardstick -> ENTRY [Tn] as a ring row holds them.  An
    element of g is non-finite when its exponent bits are all ones; it enters neither the sum nor the maximum.  A frozen
    tensor keeps the entry of an empty ring."""
    g, p = np.ascontiguousarray(g, dtype=np.float32), np.ascontiguousarray(p, dtype=np.float32)
    table = np.asarray(table, dtype=np.int64).reshape(-1, 2)
    out = empty_ring(1, len(table))["entry"][0]
    live = trainable_mask(table, segs)
    for t, (a, b) in enumerate(table):
        if not live[t]:
            continue
        gt, pt = g[a:b], p[a:b].astype(np.float64)
        bad = (gt.view(np.uint32) & np.uint32(0x7f800000)) == np.uint32(0x7f800000)
        fin = gt[~bad]
        where = np.flatnonzero(bad)
        f64 = fin.astype(np.float64)
        out[t] = (float(np.sum(f64 * f64)), float(np.sum(pt * pt)), np.abs(fin).max() if fin.size else np.float32(0.0),
                  int(bad.sum()), int(where[0]) if where.size else -1, 0)
    return out


class TensorRing:
    """What TensorMonitor and updmon.UpdateMonitor share: the tensor table of `optimizer`'s flat buffer, a ring of `period`
    rows in device memory that two launches per due step fill, and its reading.

    One tensor per parameter, in the order of the flat buffer: `names`, `shapes`, `numel`, `table` int64 [Tn, 2].  Under a
    frozen cut the optimizer's trainable segments decide which tensors are watched (`frozen`); the others come back
    masked.  A subclass names its config key (KEY), its module's row_dtype / empty_ring and its workspace query, and
    supplies `_warm`, `enqueue`, `_dict` (rows -> what `read()` returns) and, where a row is not one due step,
    `_due_rows`."""
    KEY = row_dtype = empty_ring = workspace_bytes = None

    def __init__(self, optimizer, period, every=1):
        from .optim import GuardedClipAdamW
        me = type(self).__name__
        if not isinstance(optimizer, GuardedClipAdamW):
            raise TypeError("%s needs an optim.GuardedClipAdamW or one of its subclasses, got %s: only the guarded tail "
                            "keeps the step's decision and its step counters in device memory (set SVIT.GUARDED_STEP or "
                            "SVIT.%s before construct_optimizer)" % (me, type(optimizer).__name__, self.KEY))
        for what, v in (("period", period), ("every", every)):
            if isinstance(v, bool) or not isinstance(v, int) or v < 1:
                raise ValueError("%s: %s is a positive int, got %r" % (me, what, v))
        self.optimizer, self.flat = optimizer, optimizer.flat
        self.period, self.every = period, every
        flat = self.flat
        self.names = sorted(flat.slots, key=lambda k: flat.slots[k][0])
        self.shapes = [tuple(flat.slots[k][2]) for k in self.names]
        self.table = np.ascontiguousarray(
            np.array([[flat.slots[k][0], flat.slots[k][0] + flat.slots[k][1]] for k in self.names], dtype=np.int64))
        ops.tensor_table_check(self.table, flat.total)
        self.numel = self.table[:, 1] - self.table[:, 0]
        self.segments = optimizer.segments              # None: nothing is frozen
        self.frozen = ~trainable_mask(self.table, self.segments)
        self.depth = flat.n_ranks - 2
        self.layer_ids = np.array([lrscale.layer_id(k, self.depth) for k in self.names], dtype=np.int64)
        dev = flat.data.device
        self.table_dev = torch.from_numpy(self.table).to(dev)
        self.workspace = torch.zeros(self.workspace_bytes(flat.total, len(self.names)), dtype=torch.uint8, device=dev)
        self.ring = self._empty().to(dev)
        self.last_read = self._step_now()
        if dev.type == "cuda":
            self._warm()

    def _empty(self):
        return torch.from_numpy(self.empty_ring(self.period, len(self.names)).view(np.uint8).reshape(-1).copy())

    def _step_now(self):
        """index of the optimizer's last step (-1 before the first); synchronises"""
        s = self.optimizer.stats()
        return s["applied"] + s["skipped"] - 1

    def reset(self):
        """forget every row: the ring as it was created, the next `read()` starts behind the optimizer's last step"""
        self.ring.copy_(self._empty())
        self.last_read = self._step_now()

    # ---- reading -----------------------------------------------------------------------------------------------------
    def _rows(self, since):
        """the ring's written rows of the steps after `since`, ordered by step (ONE device read)"""
        ring = self.ring.cpu().numpy().view(self.row_dtype(len(self.names)))
        rows = ring[ring["head"]["step"] > since]
        return rows[np.argsort(rows["head"]["step"], kind="stable")]

    def _masked(self, a):
        """a [rows, Tn] with the frozen tensors masked"""
        return np.ma.MaskedArray(a, mask=np.broadcast_to(self.frozen, a.shape).copy())

    def _due_rows(self, rows):
        """how many of the rows are steps that were due by `every`"""
        return len(rows)

    def read(self):
        """the rows recorded since the last read, ordered by step, as the subclass's `read` lists them; `lost`: how many
        multiples of `every` since the last read, up to the newest step the ring holds, have no row"""
        rows = self._rows(self.last_read)
        lost = 0
        if len(rows):
            now = int(rows["head"]["step"][-1])
            due = now // self.every - self.last_read // self.every          # multiples of `every` in (last_read, now]
            lost = due - self._due_rows(rows)
            self.last_read = now
        return self._dict(rows, lost)

    def _layer_sums(self, *arrays):
        """each [rows, Tn] array summed over lrscale's layer ids, frozen tensors left out: depth + 2 groups -- 0 the stem,
        1 + i block i, depth + 1 the rest -> ([rows, depth + 2] per array, the mask of the groups whose tensors are all
        frozen)"""
        G = self.depth + 2
        r = len(arrays[0])
        sums = [np.zeros((r, G), dtype=np.float64 if a.dtype.kind == "f" else np.int64) for a in arrays]
        seen = np.zeros(G, dtype=bool)
        for t, lid in enumerate(self.layer_ids):
            if self.frozen[t]:
                continue
            seen[lid] = True
            for s, a in zip(sums, arrays):
                s[:, lid] += a[:, t]
        return sums, np.broadcast_to(~seen, (r, G)).copy()

    @staticmethod
    def _last(a):
        """the last row of a by_layer array as log_stats prints it: six digits, None where masked or not finite"""
        return [None if x is np.ma.masked or not np.isfinite(x) else float("%.6g" % x) for x in a[-1]]


class TensorMonitor(TensorRing):
    """The statistics ring behind `optimizer`'s guard.

    optimizer: an optim.GuardedClipAdamW or one of its subclasses (AdamW plain, over segments or with learning-rate
    scales; GuardedClipAdam; GuardedClipSGD).  period: rows of the ring, R -- cfg.LOG_PERIOD, the steps between two
    `read()`s.  every: a step is recorded when its index (applied + dropped steps so far, from 0) is a multiple of it;
    a dropped step is always recorded.  Nothing is attached by the constructor: `optimizer.attach_monitor(monitor)` (or
    `build_monitor`) does that."""
    KEY = "MONITOR"
    row_dtype, empty_ring = staticmethod(row_dtype), staticmethod(empty_ring)
    workspace_bytes = staticmethod(ops.tensor_stats_workspace)

    def _warm(self):
        """one call on four dummy elements, so that a later stream capture meets loaded code; neither the ring nor the
        optimizer's record is touched (a record of zeros says step -1: nothing is recorded)"""
        dev = self.flat.data.device
        z = torch.zeros(2, 4, device=dev)
        t = np.array([[0, 4]], dtype=np.int64)
        ops.tensor_stats(z[0], z[1], torch.from_numpy(t).to(dev), t, None, torch.zeros(12, dtype=torch.int32, device=dev),
                         torch.zeros(48, dtype=torch.uint8, device=dev), 1, 1,
                         torch.zeros(ops.tensor_stats_workspace(4, 1), dtype=torch.uint8, device=dev))

    def enqueue(self):
        """the two launches, behind the guard and in front of the solver's; allocation-free and capturable"""
        ops.tensor_stats(self.flat.grad, self.flat.data, self.table_dev, self.table, self.segments,
                         self.optimizer.dev_rec, self.ring, self.period, self.every, self.workspace)

    def _due_rows(self, rows):
        """dropped steps are recorded too: only the multiples of `every` count (a dropped step between two due ones that
        was overwritten leaves no trace and is not counted as lost)"""
        return int((rows["head"]["step"] % self.every == 0).sum())

    def read(self):
        """the rows recorded since the last read, ordered by step, as a dict of arrays [rows, Tn] (frozen tensors masked):
        names, steps, applied, grad_norm = sqrt(sumsq_g) * optimizer.grad_scale, weight_norm, absmax, n_bad, first_bad,
        the raw sumsq_g / sumsq_p, and `lost`: how many steps that were due by `every` since the last read the ring no
        longer holds (R rows; an overrun is reported, not raised)"""
        return super().read()

    def _dict(self, rows, lost):
        e, masked = rows["entry"], self._masked
        return {"names": list(self.names), "steps": rows["head"]["step"].copy(), "applied": rows["head"]["apply"] != 0,
                "sumsq_g": masked(e["sumsq_g"].copy()), "sumsq_p": masked(e["sumsq_p"].copy()),
                "grad_norm": masked(np.sqrt(e["sumsq_g"]) * float(self.optimizer.grad_scale)),
                "weight_norm": masked(np.sqrt(e["sumsq_p"])), "absmax": masked(e["absmax_g"].copy()),
                "n_bad": masked(e["n_bad"].copy()), "first_bad": masked(e["first_bad"].copy()), "lost": lost}

    def by_layer(self, rows):
        """rows (what `read()` gave) summed over lrscale's layer ids: depth + 2 groups -- 0 the stem, 1 + i block i,
        depth + 1 the rest -- of grad_norm, weight_norm and ratio = grad_norm / weight_norm, each [rows, depth + 2]; a
        group whose tensors are all frozen is masked"""
        (sg, sp), mask = self._layer_sums(rows["sumsq_g"].data, rows["sumsq_p"].data)
        gn = np.sqrt(sg) * float(self.optimizer.grad_scale)
        wn = np.sqrt(sp)
        with np.errstate(divide="ignore", invalid="ignore"):
            ratio = gn / wn
        return {"steps": rows["steps"], "grad_norm": np.ma.MaskedArray(gn, mask=mask),
                "weight_norm": np.ma.MaskedArray(wn, mask=mask), "ratio": np.ma.MaskedArray(ratio, mask=mask.copy())}

    def culprits(self, rows):
        """[(step, name, n_bad, index)] for every dropped step among the rows: the tensors whose gradient held a
        non-finite element, `index` the first one's position unravelled into the tensor's shape"""
        out = []
        for i, step in enumerate(rows["steps"]):
            if rows["applied"][i]:
                continue
            nb, fb = rows["n_bad"][i], rows["first_bad"][i]
            for t in np.flatnonzero(np.ma.filled(nb, 0) > 0):
                shape = self.shapes[t] or (1,)
                idx = tuple(int(x) for x in np.unravel_index(int(fb.data[t]), shape))
                out.append((int(step), self.names[t], int(nb.data[t]), idx if self.shapes[t] else ()))
        return out

    def culprit_line(self):
        """one line on the most recent dropped step the ring holds, for the optimizer's check(); "" when it holds none.
        Reads the ring without moving `last_read`."""
        found = self.culprits(self._dict(self._rows(-1), 0))
        if not found:
            return ""
        last = found[-1][0]
        found = [c for c in found if c[0] == last]
        text = ", ".join("%s (%d non-finite, the first at %s)" % (name, nb, list(idx)) for _, name, nb, idx in
                         found[:MAX_CULPRITS])
        more = len(found) - MAX_CULPRITS
        return "non-finite gradients of step %d in %d tensor%s: %s%s" % (
            last, len(found), "" if len(found) == 1 else "s", text, " and %d more" % more if more > 0 else "")

    def log_stats(self, rows):
        """the JSON line train_epoch logs: the by_layer numbers of the last recorded step among `rows` and the culprits
        of its dropped steps; None when there is no row"""
        if not len(rows["steps"]):
            return None
        layers, last = self.by_layer(rows), self._last
        return {"_type": "train_tensor_stats", "step": int(rows["steps"][-1]), "applied": bool(rows["applied"][-1]),
                "rows": int(len(rows["steps"])), "lost": int(rows["lost"]), "grad_norm": last(layers["grad_norm"]),
                "weight_norm": last(layers["weight_norm"]), "ratio": last(layers["ratio"]),
                "culprits": [[s, n, nb, list(idx)] for s, n, nb, idx in self.culprits(rows)]}

    stats_host = staticmethod(stats_host)


def build_monitor(cfg, optimizer):
    """SVIT.MONITOR (and SVIT.MONITOR_EVERY, default 1) -> a TensorMonitor of cfg.LOG_PERIOD rows attached to `optimizer`,
    or None without the key: no ring, no table, not one launch more"""
    if not getattr(cfg.SVIT, "MONITOR", False):
        return None
    every = getattr(cfg.SVIT, "MONITOR_EVERY", 1)
    if isinstance(every, bool) or not isinstance(every, int) or every < 1:
        raise ValueError("SVIT.MONITOR_EVERY is a positive int, got %r" % (every,))
    mon = TensorMonitor(optimizer, int(cfg.LOG_PERIOD), every=every)
    optimizer.attach_monitor(mon)
    return mon
