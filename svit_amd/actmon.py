"""Per-block forward statistics inside the step: which block, branch, clip and token went non-finite first, and the
residual-stream RMS, the outlier token and the attention logits' level per block.

    monitor = build_actmon(cfg, model, optimizer)           # None without SVIT.ACT_MONITOR; attached to the model otherwise
    ...
    rows = monitor.read()                                   # once per cfg.LOG_PERIOD: ONE device read
    monitor.origin(rows), rows["rms"], rows["lse_max"]

A training forward keeps, for its backward, the per-row LayerNorm statistics in front of every block's attention branch
(mean1 / rstd1), in front of its MLP (mean2 / rstd2) and in front of the final norm, and the attention's log-sum-exp.
The LayerNorm kernel forms `mean` as a plain sum and `rstd` from the two-pass variance without a clamp, so a non-finite
element of a row shows in that row's statistics, and for a finite row mean^2 + 1 / rstd^2 - eps is its mean square.
Two launches (svit_act_stats, csrc/actmon.hip) at the end of every SAVING `Engine.forward` -- the eager training forward,
the body of a GraphedTrainStep, every micro-step of an accumulated step -- read those small arrays (about 13 MB at
B = 8, 16 x 224^2, against several GB of activations) and write one row of a ring in device memory (the layout:
include/svit_hip.h).  A pass that saves nothing (eval, the frames pass, a head-only cut) records nothing and launches
nothing.  Nothing here synchronises but `read()`, `reset()`, `origin_line()` and the constructor.  The reference has
nothing like it: SVIT.ACT_MONITOR is read with getattr and is not a key of the default tree.  Nothing is saved in
checkpoints.
"""
import math

import numpy as np
import torch

from . import arch, ops

HEADER = np.dtype([("pass", "<i8"), ("step", "<i8"), ("B", "<i4"), ("Tx", "<i4"), ("T0", "<i4"), ("H0", "<i4"),
                   ("W0", "<i4"), ("n_sites", "<i4"), ("reserved", "<i4", (2,))])
ENTRY = np.dtype([("sum", "<f8"), ("ext", "<f4"), ("ext2", "<f4"), ("arg", "<i4"), ("n_bad", "<i4"),
                  ("first_bad", "<i4"), ("rows", "<i4")])
assert HEADER.itemsize == 48 and ENTRY.itemsize == 32
MAX_SITES = 96
MAX_ROWS = 1 << 24
LN_EPS = 1e-6           # ops.layernorm_fwd's eps, the one every block norm and the final norm use
LN2 = math.log(2.0)
_EXP = np.uint32(0x7f800000)
_SIGN = np.uint32(0x80000000)


def row_dtype(n_slots):
    """a ring row of n_slots slots: 48 + 32 * n_slots bytes"""
    return np.dtype([("head", HEADER), ("entry", ENTRY, (n_slots,))])


def empty_entry():
    """the entry of a slot no site names: n_bad = -1, arg = first_bad = -1, zeros"""
    e = np.zeros((), dtype=ENTRY)
    e["arg"] = e["n_bad"] = e["first_bad"] = -1
    return e


def empty_ring(R, n_slots):
    """the ring as the host writes it: no row written (pass -1, step -1), every entry the empty entry"""
    ring = np.zeros(R, dtype=row_dtype(n_slots))
    ring["head"]["pass"] = -1
    ring["head"]["step"] = -1
    ring["entry"] = empty_entry()
    return ring


def slot_names(depth):
    """3 * depth + 1 names in network order: blocks.i.in, blocks.i.attn_lse, blocks.i.mid for every block, then norm.in"""
    out = []
    for i in range(depth):
        out += ["blocks.%d.in" % i, "blocks.%d.attn_lse" % i, "blocks.%d.mid" % i]
    return out + ["norm.in"]


def order_key(bits):
    """uint32 keys monotone in the float order of the finite values whose integer images are `bits`; -0.0 below +0.0"""
    bits = np.asarray(bits, dtype=np.uint32)
    return np.where(bits & _SIGN, ~bits, bits | _SIGN)


def bad_rows(a, b=None):
    """bool [rows]: the rows the kernels leave out.  LayerNorm (b given): mean or rstd with all exponent bits set, or
    rstd zero or negative (sign bit set); lse: all exponent bits set."""
    ab = np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)
    bad = (ab & _EXP) == _EXP
    if b is not None:
        bb = np.ascontiguousarray(b, dtype=np.float32).view(np.uint32)
        bad = bad | ((bb & _EXP) == _EXP) | ((bb & _SIGN) != 0) | (bb == 0)
    return bad


def acts_host(sites):
    """svit_act_stats restated in NumPy float64, the kernels' yardstick.  sites: [(a, b)] of float32 arrays, b None for
    an lse site -> (ENTRY [n_sites] as a ring row holds them, sum |term| per site: what the bar on `sum` scales with)."""
    out = np.zeros(len(sites), dtype=ENTRY)
    mass = np.zeros(len(sites))
    for i, (a, b) in enumerate(sites):
        a = np.ascontiguousarray(a, dtype=np.float32).reshape(-1)
        ln = b is not None
        if ln:
            b = np.ascontiguousarray(b, dtype=np.float32).reshape(-1)
            assert b.shape == a.shape
        bad = bad_rows(a, b)
        good = np.flatnonzero(~bad)
        where = np.flatnonzero(bad)
        ag = a[good].astype(np.float64)
        if ln:
            bg = b[good].astype(np.float64)
            with np.errstate(over="raise", divide="raise"):
                term = ag * ag + 1.0 / (bg * bg)
        else:
            term = ag
        e = out[i]
        e["sum"] = float(np.sum(term))
        mass[i] = float(np.sum(np.abs(term)))
        e["n_bad"], e["first_bad"], e["rows"] = len(where), (where[0] if len(where) else -1), len(a)
        if len(good) == 0:
            e["ext"], e["ext2"], e["arg"] = 0.0, 0.0, -1
            continue
        if ln:
            keys = b[good].view(np.uint32).astype(np.int64)                      # rstd > 0: the smallest wins
            k = int(np.argmin(keys))                                             # (the first among ties)
            e["ext"], e["ext2"] = b[good][k], np.abs(a[good]).max()
        else:
            keys = order_key(a[good].view(np.uint32)).astype(np.int64)           # the largest wins
            k = int(np.argmax(keys))
            e["ext"], e["ext2"] = a[good][k], 0.0
        e["arg"] = good[k]
    return out, mass


def slot_geometry(plan, Tx, T0, H0, W0):
    """per slot, in slot_names' order: (heads or None, (t, h, w) of the slot's token grid, n_obj) -- a LayerNorm slot has
    B * (1 + t h w + n_obj) rows, an lse slot B * heads * (1 + t h w + n_obj)"""
    n_obj, thw, out = Tx * plan.objects, (T0, H0, W0), []
    for blk in plan.blocks:
        sq = blk.stride_q[1]
        q_thw = (thw[0], arch.pooled(thw[1], sq), arch.pooled(thw[2], sq))
        out += [(None, thw, n_obj), (blk.heads, q_thw, n_obj), (None, q_thw, n_obj)]
        thw = q_thw
    return out + [(None, thw, n_obj)]


_BLAME = {"in": "the MLP of block %d", "attn_lse": "the q/k of block %d", "mid": "the attention branch of block %d"}


def culprit(name):
    """what to look at when `name` is the first slot in network order with a bad row"""
    if name == "blocks.0.in":
        return "the stem or the input"
    if name == "norm.in":
        return None
    _, i, kind = name.split(".")
    return _BLAME[kind] % (int(i) - 1 if kind == "in" else int(i))


class ActivationMonitor:
    """The forward-statistics ring of `model` (an SViT on the GPU, or its data-parallel wrapper).

    period: rows of the ring, R -- the saving forward passes between two `read()`s (cfg.LOG_PERIOD times the virtual
    ranks per GPU).  optimizer: an optim.GuardedClipAdamW or one of its subclasses, whose step record gives every row the
    index of the optimizer step the pass feeds (applied + dropped steps so far, what a TensorMonitor's rows carry), or
    None: step -1.  Nothing is attached by the constructor: `model.attach_activation_monitor(monitor)` (or
    `build_actmon`) does that."""

    def __init__(self, model, period, optimizer=None):
        core = model.module if hasattr(model, "module") else model
        if getattr(core, "flat", None) is None:
            raise ValueError("ActivationMonitor needs a finalized (on-GPU) SViT: the ring lives beside its flat buffers "
                             "and its engine's forward holds the launches")
        if optimizer is not None:
            from .optim import GuardedClipAdamW
            if not isinstance(optimizer, GuardedClipAdamW):
                raise TypeError("ActivationMonitor(optimizer=...) takes an optim.GuardedClipAdamW or one of its "
                                "subclasses, got %s: only the guarded tail keeps its step counters in device memory "
                                "(pass optimizer=None for rows without a step index)" % type(optimizer).__name__)
            if optimizer.flat is not core.flat:
                raise ValueError("ActivationMonitor: the optimizer was built over another model")
        if isinstance(period, bool) or not isinstance(period, int) or period < 1:
            raise ValueError("ActivationMonitor: period is a positive int, got %r" % (period,))
        self.model, self.plan, self.optimizer, self.period = core, core.plan, optimizer, period
        self.depth = len(self.plan.blocks)
        self.names = slot_names(self.depth)
        self.n_slots = len(self.names)
        if self.n_slots > MAX_SITES:
            raise ValueError("ActivationMonitor: depth %d gives %d sites, the site table holds %d"
                             % (self.depth, self.n_slots, MAX_SITES))
        self.is_lse = np.array([n.endswith("attn_lse") for n in self.names])
        self.window = ops.act_stats_window()
        dev = core.flat.data.device
        self.ring = torch.from_numpy(empty_ring(period, self.n_slots).view(np.uint8).reshape(-1).copy()).to(dev)
        self.state = torch.zeros(1, dtype=torch.int64, device=dev)
        self.workspace = torch.zeros(ops.act_stats_workspace(64), dtype=torch.uint8, device=dev)
        self._retired = []          # outgrown workspaces: a capture may hold their address
        self.last_read = -1
        if dev.type == "cuda":
            self._warm()

    def _warm(self):
        """one call on a dummy site, so that a later stream capture meets loaded code; ring and counter of its own"""
        dev = self.ring.device
        z = torch.ones(2, 4, device=dev)
        ops.act_stats([(z[0].data_ptr(), z[1].data_ptr(), 4)], [0], 1, (1, 1, 1, 1, 1), None,
                      torch.zeros(48 + 32, dtype=torch.uint8, device=dev), 1, torch.zeros(1, dtype=torch.int64, device=dev),
                      torch.zeros(ops.act_stats_workspace(1), dtype=torch.uint8, device=dev))
        torch.cuda.synchronize(dev)

    def sites_of(self, st):
        """(sites, slots, tensors) of a forward's saved state: blocks whose saved state is None or only the shapes of a
        frozen cut contribute nothing"""
        sites, slots, keep = [], [], []

        def put(slot, a, b=None):
            sites.append((a.data_ptr(), None if b is None else b.data_ptr(), a.numel()))
            slots.append(slot)
            keep.append((a, b))
        for i, sv in enumerate(st["blocks"]):
            if sv is None or "mean1" not in sv:
                continue
            put(3 * i, sv["mean1"], sv["rstd1"])
            put(3 * i + 1, sv["lse2"])
            put(3 * i + 2, sv["mean2"], sv["rstd2"])
        if st.get("mean") is not None:
            put(3 * self.depth, st["mean"], st["rstd"])
        return sites, slots, keep

    def enqueue(self, st):
        """the two launches over the statistics `st` (what Engine.forward returns beside the tokens) holds; capturable,
        and allocation-free unless the workspace has to grow, which only an uncaptured pass may do"""
        sites, slots, _ = self.sites_of(st)
        if not sites:
            return
        need = ops.act_stats_workspace(sum((s[2] + self.window - 1) // self.window for s in sites))
        if need > self.workspace.numel():
            if torch.cuda.is_current_stream_capturing():
                raise RuntimeError("ActivationMonitor: this pass needs a workspace of %d bytes, the monitor holds %d, and "
                                   "a stream capture cannot allocate: run the pass once outside a capture first"
                                   % (need, self.workspace.numel()))
            self._retired.append(self.workspace)
            self.workspace = torch.zeros(need, dtype=torch.uint8, device=self.ring.device)
        T0, H0, W0 = st["thw0"]
        ops.act_stats(sites, slots, self.n_slots, (st["B"], st["Tx"], T0, H0, W0),
                      None if self.optimizer is None else self.optimizer.dev_rec, self.ring, self.period, self.state,
                      self.workspace)

    def reset(self):
        """forget every row: the ring as it was created, the pass counter at 0"""
        self.ring.copy_(torch.from_numpy(empty_ring(self.period, self.n_slots).view(np.uint8).reshape(-1).copy()))
        self.state.zero_()
        self.last_read = -1

    # ---- reading -----------------------------------------------------------------------------------------------------
    def _ring_host(self):
        """the ring on the host as row_dtype rows: the ONE place that reads the device"""
        return self.ring.cpu().numpy().view(row_dtype(self.n_slots))

    def read(self):
        """the rows written since the last read, ordered by pass, as a dict: names, passes, steps, header (the rows'
        headers: B, Tx, T0, H0, W0 per pass), lost (passes since the last read the ring of R rows no longer holds: an
        overrun is reported, not raised) and arrays [rows, n_slots], masked where no site named the slot --
        mean_sq = sum / good rows - eps, rms = sqrt(mean_sq), widest_std (the std of the widest token, from the smallest
        rstd), max_abs_mean for the LayerNorm slots; lse_max, lse_mean (natural log) for the attn_lse slots; n_bad,
        first_bad, arg (the row of the widest token / of the largest lse), rows and the raw sum for all."""
        rows, lost, self.last_read = read_rows(self._ring_host(), self.last_read)
        return rows_dict(rows, self.names, self.is_lse, lost)

    def where(self, header, slot, r):
        """row index r of `slot` (an index or a name) in a pass with that header -> (sample, token, kind) for a LayerNorm
        slot, (sample, head, token, kind) for an attn_lse slot; kind is "cls", ("patch", t, h, w) or
        ("object", frame, o).  The geometry comes from the header: a video and an image micro-step share one ring."""
        return where(self.plan, header, slot, r)

    def origin(self, rows):
        """[(pass, step, name, n_bad, where(first_bad), culprit)] for every pass among the rows (what `read()` gave)
        that has a bad row: the first slot in network order with n_bad > 0 and what to look at -- blocks.0.in: the stem
        or the input; blocks.i.attn_lse: block i's q/k; blocks.i.mid: block i's attention branch; blocks.i+1.in or
        norm.in: the MLP of the block before"""
        return origin(self.plan, rows)

    def origin_line(self, step=None):
        """one line on the most recent pass with a bad row that the ring holds -- among the passes of optimizer step
        `step` when given -- for the optimizer's check(); "" when it holds none.  Reads the ring without moving
        `last_read`."""
        found = self.origin(rows_dict(rows_since(self._ring_host(), -1), self.names, self.is_lse))
        if step is not None:
            found = [f for f in found if f[1] == step]
        if not found:
            return ""
        p, step, name, nb, at, blame = found[-1]
        return ("non-finite activations in the forward of step %d (pass %d): first at %s, %d bad row%s, the first %s -- "
                "look at %s" % (step, p, name, nb, "" if nb == 1 else "s", describe(at), blame))

    def log_stats(self, rows):
        """the JSON line train_epoch logs: per block the residual-stream RMS in front of it, the widest token's std and
        the largest attention log-sum-exp of the last pass among `rows`, and the origins of the passes with bad rows;
        None when there is no row"""
        if not len(rows["passes"]):
            return None
        ln_in = [3 * i for i in range(self.depth)] + [3 * self.depth]
        lse = [3 * i + 1 for i in range(self.depth)]

        def last(a, cols):
            return [None if x is np.ma.masked or not np.isfinite(x) else float("%.6g" % x) for x in a[-1][cols]]
        return {"_type": "train_activation_stats", "pass": int(rows["passes"][-1]), "step": int(rows["steps"][-1]),
                "rows": int(len(rows["passes"])), "lost": int(rows["lost"]), "rms": last(rows["rms"], ln_in),
                "widest_std": last(rows["widest_std"], ln_in), "lse_max": last(rows["lse_max"], lse),
                "n_bad": int(np.ma.filled(rows["n_bad"], 0).clip(min=0).sum()),
                "origin": [[p, s, n, nb, list(_flat(at)), bl] for p, s, n, nb, at, bl in self.origin(rows)]}

    acts_host = staticmethod(acts_host)


def _flat(at):
    return [x if not isinstance(x, tuple) else list(x) for x in at]


def describe(at):
    """where()'s tuple as text"""
    kind = at[-1]
    tok = "the cls token" if kind == "cls" else "%s token %s" % (kind[0], list(kind[1:]))
    head = " head %d" % at[1] if len(at) == 4 else ""
    return "in sample %d%s at token %d (%s)" % (at[0], head, at[-2], tok)


def origin(plan, rows):
    """see ActivationMonitor.origin; needs no device"""
    depth = len(plan.blocks)
    names = slot_names(depth)
    out = []
    for i in range(len(rows["passes"])):
        nb = np.ma.filled(rows["n_bad"][i], 0)
        hit = np.flatnonzero(nb > 0)
        if not len(hit):
            continue
        s = int(hit[0])
        blame = culprit(names[s]) or "the MLP of block %d" % (depth - 1)
        out.append((int(rows["passes"][i]), int(rows["steps"][i]), names[s], int(nb[s]),
                    where(plan, rows["header"][i], s, int(rows["first_bad"].data[i][s])), blame))
    return out


def read_rows(ring, last_read):
    """a ring (row_dtype array) and the newest pass already read -> (the rows written since, ordered by pass; the passes
    in between that the ring no longer holds; the newest pass now read)"""
    rows = rows_since(ring, last_read)
    if not len(rows):
        return rows, 0, last_read
    now = int(rows["head"]["pass"][-1])
    return rows, now - last_read - len(rows), now


def rows_since(ring, since):
    """the written rows of a ring (row_dtype array) of the passes after `since`, ordered by pass"""
    rows = ring[ring["head"]["pass"] > since]
    return rows[np.argsort(rows["head"]["pass"], kind="stable")]


def rows_dict(rows, names, is_lse, lost=0):
    """ring rows -> the dict `ActivationMonitor.read()` returns"""
    e = rows["entry"]
    absent = e["n_bad"] < 0
    lse = np.broadcast_to(np.asarray(is_lse, dtype=bool), absent.shape)
    good = (e["rows"] - np.maximum(e["n_bad"], 0)).astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        mean = e["sum"] / good
        mean_sq = mean - LN_EPS
        rms = np.sqrt(np.maximum(mean_sq, 0.0))
        ext = e["ext"].astype(np.float64)
        widest = np.sqrt(np.maximum(1.0 / (ext * ext) - LN_EPS, 0.0))
    none = good <= 0

    def masked(a, m):
        return np.ma.MaskedArray(np.array(a), mask=np.array(m))
    ln_m, lse_m = absent | lse | none, absent | ~lse | none
    return {"names": list(names), "passes": rows["head"]["pass"].copy(), "steps": rows["head"]["step"].copy(),
            "header": rows["head"].copy(), "lost": int(lost),
            "sum": masked(e["sum"], absent), "mean_sq": masked(mean_sq, ln_m), "rms": masked(rms, ln_m),
            "widest_std": masked(widest, ln_m), "max_abs_mean": masked(e["ext2"], ln_m),
            "lse_max": masked(ext * LN2, lse_m), "lse_mean": masked(mean * LN2, lse_m),
            "n_bad": masked(e["n_bad"], absent), "first_bad": masked(e["first_bad"], absent),
            "arg": masked(e["arg"], absent), "rows": masked(e["rows"], absent)}


def where(plan, header, slot, r):
    """see ActivationMonitor.where; needs no device"""
    names = slot_names(len(plan.blocks))
    s = names.index(slot) if isinstance(slot, str) else int(slot)
    B, Tx = int(header["B"]), int(header["Tx"])
    heads, (t, h, w), n_obj = slot_geometry(plan, Tx, int(header["T0"]), int(header["H0"]), int(header["W0"]))[s]
    L = t * h * w
    N = 1 + L + n_obj
    total = B * N * (heads or 1)
    r = int(r)
    if not 0 <= r < total:
        raise ValueError("where: row %d outside the %d rows of %s in a pass of B = %d, Tx = %d, grid %s"
                         % (r, total, names[s], B, Tx, (t, h, w)))
    tok = r % N
    if tok == 0:
        kind = "cls"
    elif tok <= L:
        kind = ("patch",) + tuple(int(x) for x in np.unravel_index(tok - 1, (t, h, w)))
    else:
        kind = ("object", (tok - 1 - L) // plan.objects, (tok - 1 - L) % plan.objects)
    if heads is None:
        return (r // N, tok, kind)
    return (r // (heads * N), (r // N) % heads, tok, kind)


def build_actmon(cfg, model, optimizer=None, virtual_ranks=None):
    """SVIT.ACT_MONITOR -> an ActivationMonitor of cfg.LOG_PERIOD * k rows attached to `model` (k: the virtual ranks one
    GPU runs per iteration, cfg.NUM_GPUS // world size unless given), or None without the key: no ring, not one launch
    more"""
    if not getattr(cfg.SVIT, "ACT_MONITOR", False):
        return None
    period = cfg.LOG_PERIOD
    if isinstance(period, bool) or not isinstance(period, int) or period < 1:
        raise ValueError("SVIT.ACT_MONITOR: cfg.LOG_PERIOD is a positive int, got %r" % (period,))
    if virtual_ranks is None:
        import torch.distributed as dist
        world = dist.get_world_size() if dist.is_available() and dist.is_initialized() else 1
        virtual_ranks = max(1, int(cfg.NUM_GPUS) // world)
    if isinstance(virtual_ranks, bool) or not isinstance(virtual_ranks, int) or virtual_ranks < 1:
        raise ValueError("build_actmon: virtual_ranks is a positive int, got %r" % (virtual_ranks,))
    core = model.module if hasattr(model, "module") else model
    mon = ActivationMonitor(core, period * virtual_ranks, optimizer=optimizer)
    core.attach_activation_monitor(mon)
    return mon
