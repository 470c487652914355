"""Per-head attention statistics inside the step: the entropy of chosen query rows, their peak and how much of their
attention goes to the cls, the patch and the object keys -- per block, head and query group.

    monitor = build_attnmon(cfg, model, optimizer)          # None without SVIT.ATTN_MONITOR; attached to the model otherwise
    ...
    rows = monitor.read()                                   # once per cfg.LOG_PERIOD: ONE device read
    rows["entropy"], rows["mass_obj"], monitor.collapsed(rows, 0.05)
    maps = attnmon.probe_clip(model, video)                 # a trained checkpoint's maps, one no-grad forward

A training forward keeps, for its backward, `qa`, `ka` and `lse2` of every block, and by the operand convention of
svit_attn_fwd (include/svit_hip.h) `qa . ka^T` over columns [0, 96 + J) IS the score in the log2 domain with the
relative-position bias folded into the one-hot columns:  p[q, k] = exp2(qa[q] . ka[k] - lse2[q]).  Two launches
(svit_attn_stats, csrc/attnmon.hip) at the end of every SAVING `Engine.forward`, directly behind the activation
monitor's, recompute that for a few probe rows per (sample, head) -- "cls": row 0; "obj": the object rows; "patch:K": K
evenly spaced patch rows -- and write one row of a ring in device memory (the layout: include/svit_hip.h).  A pass that
saves nothing (eval, the frames pass, GraphedEvalStep) records nothing and launches nothing; a block without saved
state (a frozen cut) contributes no site.  Nothing here synchronises but `read()`, `maps()`, `reset()` and the
constructor.  The reference has nothing like it inside the step: SVIT.ATTN_MONITOR, SVIT.ATTN_MONITOR_EVERY,
SVIT.ATTN_MONITOR_ROWS and SVIT.ATTN_MONITOR_MAPS are read with getattr and are not keys of the default tree.  Nothing is
saved in checkpoints.
"""
import math

import numpy as np
import torch

from . import actmon, arch, ops

HEADER = np.dtype([("pass", "<i8"), ("step", "<i8"), ("B", "<i4"), ("Tx", "<i4"), ("T0", "<i4"), ("H0", "<i4"),
                   ("W0", "<i4"), ("n_sites", "<i4"), ("row", "<i4"), ("reserved", "<i4")])
ENTRY = np.dtype([("sum_H", "<f8"), ("sum_pmax", "<f8"), ("sum_cls", "<f8"), ("sum_obj", "<f8"), ("sum_p", "<f8"),
                  ("min_H", "<f4"), ("min_row", "<i4"), ("sum_dev", "<f4"), ("rows", "<i4"), ("n_bad", "<i4"),
                  ("first_bad", "<i4")])
assert HEADER.itemsize == 48 and ENTRY.itemsize == 64
MAX_SITES = 32
MAX_ENTRIES = 1024
MAX_K = 256
DEFAULT_ROWS = ("cls", "obj", "patch:32")
SUMS = ("sum_H", "sum_pmax", "sum_cls", "sum_obj", "sum_p")
_EXP = np.uint32(0x7f800000)


def row_dtype(ent_slots):
    """a ring row of ent_slots entries: 48 + 64 * ent_slots bytes"""
    return np.dtype([("head", HEADER), ("entry", ENTRY, (ent_slots,))])


def empty_entry():
    """the entry no site owns: n_bad = -1, min_row = first_bad = -1, zeros"""
    e = np.zeros((), dtype=ENTRY)
    e["min_row"] = e["n_bad"] = e["first_bad"] = -1
    return e


def empty_ring(R, ent_slots):
    """the ring as the host writes it: no row written (pass -1, step -1), every entry the empty entry"""
    ring = np.zeros(R, dtype=row_dtype(ent_slots))
    ring["head"]["pass"] = -1
    ring["head"]["step"] = -1
    ring["entry"] = empty_entry()
    return ring


def parse_rows(rows):
    """("cls", "obj", "patch:32") -> (group names, kinds as svit_attn_probe takes them, K): one to three distinct groups
    in entry order"""
    if isinstance(rows, str):
        rows = tuple(r.strip() for r in rows.split(","))
    names, kinds, K = [], [], 32
    for r in rows:
        if not isinstance(r, str):
            raise ValueError("attention monitor rows: %r is not one of \"cls\", \"obj\", \"patch:K\"" % (r,))
        base, _, arg = r.partition(":")
        if base not in ops.ATTN_GROUP_KINDS or (arg != "") != (base == "patch") or base in [n.split(":")[0] for n in names]:
            raise ValueError("attention monitor rows: %r -- the groups are \"cls\", \"obj\" and \"patch:K\", each at most "
                             "once" % (r,))
        if base == "patch":
            if not arg.isdigit() or not 1 <= int(arg) <= MAX_K:
                raise ValueError("attention monitor rows: %r -- K is an int in 1 .. %d" % (r, MAX_K))
            K = int(arg)
        names.append(r)
        kinds.append(ops.ATTN_GROUP_KINDS[base])
    if not names:
        raise ValueError("attention monitor rows: no group given")
    return names, kinds, K


def group_rows(kind, Lq, n_obj, K):
    """the probe rows (query tokens) of one group, ascending -- the kernel's selection in the same integer arithmetic"""
    if kind == 0:
        return np.zeros(1, dtype=np.int64)
    if kind == 1:
        return 1 + Lq + np.arange(n_obj, dtype=np.int64)
    if Lq <= K:
        return 1 + np.arange(Lq, dtype=np.int64)
    return 1 + ((2 * np.arange(K, dtype=np.int64) + 1) * Lq) // (2 * K)


def _f64(t):
    if torch.is_tensor(t):
        t = t.detach().float().cpu().numpy()
    return np.asarray(t, dtype=np.float64)


def bad_bits(a):
    """bool: float32 values with all exponent bits set (inf, NaN)"""
    return (np.ascontiguousarray(a, dtype=np.float32).view(np.uint32) & _EXP) == _EXP


def attn_host(qa, ka, lse2, Lq, Lk, n_obj, bias_cols, kinds, K, eps_exp=2.0 ** -23):
    """svit_attn_stats restated in NumPy float64 on one site, the kernels' yardstick.

    qa [B,h,Nq,DA], ka [B,h,Nk,DA] (bf16 tensors or float arrays of bf16 values), lse2 f32 [B,h,Nq] -> dict:
      entries  ENTRY [h * G] as a ring row holds them (head-major, group-minor)
      bars     the same shape, one float64 per sum field and for min_H / sum_dev: the derived bound on |kernel - host|
      rows     the probe rows, all groups in order;  group  the group of each
      P        float64 [B,h,n_probe,Nk], the probabilities (NaN rows where the row is bad)
      per_row  dict of [B,h,n_probe] arrays: H, pmax, argmax, cls, obj, sum_p, bad and their bars b_H, b_p (of pmax),
               b_cls, b_obj, b_sum; b_map [B,h,n_probe,Nk]: 2 e_p per element; d: the exponents
    The bars (tests/attnmon_cases.py derives them): per key |s^ - s| <= C * 2^-24 * sum_j |q_j k_j| (C = 96 + J fp32
    additions of exact products), the subtraction adds 2^-24 |d|, so e_d = C 2^-24 A + 2^-24 |d|; exp2 adds eps_exp
    relative, a flushed result 2^-126 absolute: e_p = p (ln 2 e_d + eps_exp) + 2^-126.  To first order, times 2:
    b_sum = 2 sum e_p, b_cls = 2 e_p[0], b_obj = 2 sum_{k > Lk} e_p, b_p = 2 max e_p, b_H = 2 sum (|d| e_p + p e_d)."""
    q, k = _f64(qa), _f64(ka)
    lse32 = np.ascontiguousarray(lse2.detach().cpu().numpy() if torch.is_tensor(lse2) else lse2, dtype=np.float32)
    B, h, Nq, DA = q.shape
    Nk = k.shape[2]
    assert k.shape == (B, h, Nk, DA) and lse32.shape == (B, h, Nq) and DA in (128, 160)
    assert Nq == 1 + Lq + n_obj and Nk == 1 + Lk + n_obj
    C = 96 + (bias_cols if bias_cols else DA - 96)
    groups = [group_rows(kind, Lq, n_obj, K) for kind in kinds]
    rows = np.concatenate(groups) if groups else np.zeros(0, dtype=np.int64)
    gid = np.concatenate([np.full(len(g), i) for i, g in enumerate(groups)]).astype(np.int64)
    G, npb = len(kinds), len(rows)
    qs, kc = q[:, :, rows, :C], k[:, :, :, :C]
    with np.errstate(all="ignore"):
        s = np.einsum("bhqc,bhkc->bhqk", qs, kc)
        A = np.einsum("bhqc,bhkc->bhqk", np.abs(qs), np.abs(kc))
        lse = lse32[:, :, rows].astype(np.float64)[..., None]
        bad = bad_bits(lse32[:, :, rows]) | bad_bits(s.astype(np.float32)).any(-1) | ~np.isfinite(s).all(-1)
        d = s - lse
        P = np.exp2(d)
        e_d = C * 2.0 ** -24 * A + 2.0 ** -24 * np.abs(d)
        e_p = P * (math.log(2.0) * e_d + eps_exp) + 2.0 ** -126
        pd = np.where(P > 0, P * d, 0.0)
        per = {"H": -pd.sum(-1), "pmax": P.max(-1), "argmax": P.argmax(-1), "cls": P[..., 0],
               "obj": P[..., 1 + Lk:].sum(-1), "sum_p": P.sum(-1), "bad": bad,
               "b_H": 2 * (np.abs(d) * e_p + P * e_d).sum(-1), "b_p": 2 * e_p.max(-1), "b_cls": 2 * e_p[..., 0],
               "b_obj": 2 * e_p[..., 1 + Lk:].sum(-1), "b_sum": 2 * e_p.sum(-1), "b_map": 2 * e_p, "d": d}
    P = np.where(bad[..., None], np.nan, P)
    entries = np.zeros((h, G), dtype=ENTRY)
    bars = np.zeros((h, G), dtype=[(n, "<f8") for n in SUMS + ("min_H", "sum_dev")])
    code = (np.arange(B)[:, None] * Nq + rows[None, :])                    # [B, n_probe]
    for hd in range(h):
        for g in range(G):
            sel = gid == g
            good = ~bad[:, hd][:, sel]                                      # [B, rows of the group]
            e, bar = entries[hd, g], bars[hd, g]
            for name, key, bk in (("sum_H", "H", "b_H"), ("sum_pmax", "pmax", "b_p"), ("sum_cls", "cls", "b_cls"),
                                  ("sum_obj", "obj", "b_obj"), ("sum_p", "sum_p", "b_sum")):
                e[name] = per[key][:, hd][:, sel][good].sum()
                bar[name] = per[bk][:, hd][:, sel][good].sum()
            cg = code[:, sel]
            e["rows"], e["n_bad"] = good.size, int((~good).sum())
            e["first_bad"] = cg[~good].min() if (~good).any() else -1
            if good.any():
                Hg = per["H"][:, hd][:, sel][good]
                i = int(np.argmin(Hg))                                      # (the first, i.e. the smallest code, among ties)
                e["min_H"], e["min_row"] = Hg[i], cg[good][i]
                bar["min_H"] = per["b_H"][:, hd][:, sel][good].max() + 2.0 ** -23 * np.abs(Hg).max()
                dev = np.abs(per["sum_p"][:, hd][:, sel][good] - 1.0)
                e["sum_dev"] = dev.max()
                bar["sum_dev"] = per["b_sum"][:, hd][:, sel][good].max() + 2.0 ** -23 * dev.max()
            else:
                e["min_H"], e["min_row"], e["sum_dev"] = 0.0, -1, 0.0
    return {"entries": entries.reshape(-1), "bars": bars.reshape(-1), "rows": rows, "group": gid, "P": P,
            "per_row": per, "code": code}


def block_geometry(plan, Tx, T0, H0, W0):
    """per block: (heads, q grid (t, h, w), k grid (t, h, w), n_obj) of a pass with that geometry"""
    n_obj, thw, out = Tx * plan.objects, (T0, H0, W0), []
    for blk in plan.blocks:
        sq, skv = blk.stride_q[1], blk.stride_kv[1]
        q_thw = (thw[0], arch.pooled(thw[1], sq), arch.pooled(thw[2], sq))
        k_thw = (thw[0], arch.pooled(thw[1], skv), arch.pooled(thw[2], skv))
        out.append((blk.heads, q_thw, k_thw, n_obj))
        thw = q_thw
    return out


def train_geometry(plan):
    """(Tx, T0, H0, W0) of the plan's training clip"""
    return (plan.num_frames, plan.num_frames // plan.patch_stride[0], plan.crop // plan.patch_stride[1],
            plan.crop // plan.patch_stride[2])


def _geom(header):
    if isinstance(header, (tuple, list)):
        return tuple(int(x) for x in header)
    return tuple(int(header[k]) for k in ("Tx", "T0", "H0", "W0"))


def unravel_key(plan, header, block, k):
    """key token k of `block` in a pass with that header (a ring row's, or (Tx, T0, H0, W0)) -> "cls",
    ("patch", t, h, w) on the block's KEY grid or ("object", frame, o)"""
    _, _, (t, h, w), n_obj = block_geometry(plan, *_geom(header))[block]
    L, k = t * h * w, int(k)
    if not 0 <= k < 1 + L + n_obj:
        raise ValueError("unravel_key: key %d outside the %d keys of block %d (key grid %s, %d object tokens)"
                         % (k, 1 + L + n_obj, block, (t, h, w), n_obj))
    if k == 0:
        return "cls"
    if k <= L:
        return ("patch",) + tuple(int(x) for x in np.unravel_index(k - 1, (t, h, w)))
    return ("object", (k - 1 - L) // plan.objects, (k - 1 - L) % plan.objects)


def where(plan, header, block, head, code):
    """row code b * Nq + q of (block, head) in a pass with that header -> (sample, head, token, kind), by actmon's
    unravelling of the block's attn_lse slot"""
    heads, (t, h, w), _, n_obj = block_geometry(plan, *_geom(header))[block]
    Nq = 1 + t * h * w + n_obj
    b, q = int(code) // Nq, int(code) % Nq
    return actmon.where(plan, header, 3 * block + 1, (b * heads + int(head)) * Nq + q)


def entry_index(plan, group_names):
    """[(block, head, group name)] in entry order, and each block's first entry"""
    index, base = [], []
    for i, blk in enumerate(plan.blocks):
        base.append(len(index))
        index += [(i, hd, g) for hd in range(blk.heads) for g in group_names]
    return index, base


def read_rows(ring, last_row):
    """a ring (row_dtype array) and the newest row counter already read -> (the rows written since, in order; the rows
    in between that the ring no longer holds; the newest row counter now read)"""
    rows = ring[(ring["head"]["pass"] >= 0) & (ring["head"]["row"] > last_row)]
    rows = rows[np.argsort(rows["head"]["row"], kind="stable")]
    if not len(rows):
        return rows, 0, last_row
    now = int(rows["head"]["row"][-1])
    return rows, now - last_row - len(rows), now


def rows_dict(plan, rows, group_names, lost=0):
    """ring rows -> the dict `AttentionMonitor.read()` returns"""
    index, _ = entry_index(plan, group_names)
    e = rows["entry"]
    absent = e["n_bad"] < 0
    good = (e["rows"] - np.maximum(e["n_bad"], 0)).astype(np.float64)
    none = absent | (good <= 0)
    log_nk = np.ones(e["n_bad"].shape)
    for r in range(len(rows)):
        geo = block_geometry(plan, *_geom(rows["head"][r]))
        log_nk[r] = [math.log2(1 + np.prod(geo[b][2]) + geo[b][3]) for b, _, _ in index]

    def masked(a, m):
        return np.ma.MaskedArray(np.array(a), mask=np.array(m))
    with np.errstate(divide="ignore", invalid="ignore"):
        mean = {k: e[k] / good for k in SUMS}
        out = {"index": index, "passes": rows["head"]["pass"].copy(), "steps": rows["head"]["step"].copy(),
               "header": rows["head"].copy(), "lost": int(lost),
               "entropy": masked(mean["sum_H"], none), "entropy_norm": masked(mean["sum_H"] / log_nk, none),
               "entropy_min": masked(e["min_H"], none), "min_row": masked(e["min_row"], none),
               "pmax": masked(mean["sum_pmax"], none), "mass_cls": masked(mean["sum_cls"], none),
               "mass_obj": masked(mean["sum_obj"], none),
               "mass_patch": masked(mean["sum_p"] - mean["sum_cls"] - mean["sum_obj"], none),
               "sum_dev": masked(e["sum_dev"], none), "n_bad": masked(e["n_bad"], absent),
               "first_bad": masked(e["first_bad"], absent), "rows": masked(e["rows"], absent)}
    return out


def collapsed(rows, max_fraction):
    """[(step, block, head, group, value)] for every entry among `rows` (what `read()` gave) whose mean entropy lies below
    max_fraction of log2 Nk -- heads whose probe rows have gone one-hot"""
    out = []
    norm = rows["entropy_norm"]
    for r in range(len(rows["passes"])):
        for e in np.flatnonzero(np.ma.filled(norm[r] < max_fraction, False)):
            b, hd, g = rows["index"][e]
            out.append((int(rows["steps"][r]), b, hd, g, float(norm[r][e])))
    return out


class AttentionMonitor:
    """The attention-statistics ring of `model` (an SViT on the GPU, or its data-parallel wrapper).

    period: rows of the ring, R -- the DUE saving passes between two `read()`s.  optimizer: an optim.GuardedClipAdamW or
    one of its subclasses, whose step record gives every row its step index and decides ON THE DEVICE which passes are
    due ((applied + skipped) % every == 0: stage 1 of a pass that is not returns before it loads an operand), or None:
    step -1, due when pass % every == 0 (then `every` only thins the ring).  rows: the query groups.  maps_samples: the
    leading samples whose probability rows are kept, per block, from the latest due pass (`maps()`).  Nothing is
    attached by the constructor: `model.attach_attention_monitor(monitor)` (or `build_attnmon`) does that."""

    def __init__(self, model, period, optimizer=None, rows=DEFAULT_ROWS, every=1, maps_samples=0):
        core = model.module if hasattr(model, "module") else model
        if getattr(core, "flat", None) is None:
            raise ValueError("AttentionMonitor needs a finalized (on-GPU) SViT: the ring lives beside its flat buffers "
                             "and its engine's forward holds the launches")
        if optimizer is not None:
            from .optim import GuardedClipAdamW
            if not isinstance(optimizer, GuardedClipAdamW):
                raise TypeError("AttentionMonitor(optimizer=...) takes an optim.GuardedClipAdamW or one of its "
                                "subclasses, got %s: only the guarded tail keeps its step counters in device memory "
                                "(pass optimizer=None for rows without a step index)" % type(optimizer).__name__)
            if optimizer.flat is not core.flat:
                raise ValueError("AttentionMonitor: the optimizer was built over another model")
        for name, v, lo in (("period", period, 1), ("every", every, 1), ("maps_samples", maps_samples, 0)):
            if isinstance(v, bool) or not isinstance(v, int) or v < lo:
                raise ValueError("AttentionMonitor: %s is an int >= %d, got %r" % (name, lo, v))
        self.model, self.plan, self.optimizer, self.period = core, core.plan, optimizer, period
        self.every, self.maps_samples = every, maps_samples
        self.group_names, self.kinds, self.K = parse_rows(rows)
        self.depth = len(self.plan.blocks)
        self.index, self.ent_base = entry_index(self.plan, self.group_names)
        self.ent_slots = len(self.index)
        if self.depth > MAX_SITES or self.ent_slots > MAX_ENTRIES:
            raise ValueError("AttentionMonitor: depth %d with %d (head, group) entries; the site table holds %d blocks "
                             "and a ring row %d entries" % (self.depth, self.ent_slots, MAX_SITES, MAX_ENTRIES))
        dev = core.flat.data.device
        self.ring = torch.from_numpy(empty_ring(period, self.ent_slots).view(np.uint8).reshape(-1).copy()).to(dev)
        self.state = torch.tensor([0, 0, -1, 0], dtype=torch.int64, device=dev)
        self.workspace = torch.zeros(ops.attn_stats_workspace(1024), dtype=torch.uint8, device=dev)
        self._retired = []          # outgrown workspaces: a capture may hold their address
        self._maps = {}             # (block, B', heads, n_probe, Nk) -> f32 buffer; a capture holds their addresses
        self._maps_now = {}         # block -> the buffer the latest enqueued pass writes
        self.last_row = -1
        if dev.type == "cuda":
            self._warm()

    def _warm(self):
        """one call on a dummy site, so that a later stream capture meets loaded code; ring and counters of its own"""
        dev = self.ring.device
        qa = torch.zeros(1, 1, 2, 128, dtype=torch.bfloat16, device=dev)
        lse = torch.ones(1, 1, 2, device=dev)
        site = dict(qa=qa.data_ptr(), ka=qa.data_ptr(), lse2=lse.data_ptr(), maps=None, B=1, heads=1, Nq=2, Nk=2, DA=128,
                    bias_cols=0, Lq=1, Lk=1, n_obj=0, slot=0, ent_base=0)
        ops.attn_stats([site], 1, 1, [0], 32, 1, 0, (1, 1, 1, 1, 1), None,
                       torch.zeros(48 + 64, dtype=torch.uint8, device=dev), 1,
                       torch.zeros(4, dtype=torch.int64, device=dev),
                       torch.zeros(ops.attn_stats_workspace(1), dtype=torch.uint8, device=dev))
        torch.cuda.synchronize(dev)

    def n_probe(self, Lq, n_obj):
        return sum(len(group_rows(k, Lq, n_obj, self.K)) for k in self.kinds)

    def sites_of(self, st):
        """(sites as ops.attn_stats takes them, without maps; the tensors) of a forward's saved state: blocks whose saved
        state is None or only the shapes of a frozen cut contribute nothing"""
        sites, keep = [], []
        for i, sv in enumerate(st["blocks"]):
            if sv is None or "pools" not in sv:
                continue
            qa, ka, lse2 = sv["pools"][0][0], sv["pools"][1][0], sv["lse2"]
            B, h, Nq, DA = qa.shape
            (qt, qh, qw), (kt, kh, kw) = sv["q_thw"], sv["k_thw"]
            sites.append(dict(qa=qa.data_ptr(), ka=ka.data_ptr(), lse2=lse2.data_ptr(), maps=None, B=B, heads=h, Nq=Nq,
                              Nk=ka.shape[2], DA=DA, bias_cols=kt + kh + kw, Lq=qt * qh * qw, Lk=kt * kh * kw,
                              n_obj=st["n_obj"], slot=i, ent_base=self.ent_base[i]))
            keep.append((qa, ka, lse2))
        return sites, keep

    def enqueue(self, st):
        """the two launches over the attention operands `st` (what Engine.forward returns beside the tokens) holds;
        capturable, and allocation-free unless the workspace or a map buffer has to be created, which only an uncaptured
        pass may do"""
        sites, _ = self.sites_of(st)
        if not sites:
            return
        capturing = torch.cuda.is_current_stream_capturing()
        need = ops.attn_stats_workspace(sum(s["B"] * s["heads"] * len(self.kinds) for s in sites))
        if need > self.workspace.numel():
            if capturing:
                raise RuntimeError("AttentionMonitor: this pass needs a workspace of %d bytes, the monitor holds %d, and "
                                   "a stream capture cannot allocate: run the pass once outside a capture first"
                                   % (need, self.workspace.numel()))
            self._retired.append(self.workspace)
            self.workspace = torch.zeros(need, dtype=torch.uint8, device=self.ring.device)
        if self.maps_samples:
            for s in sites:
                key = (s["slot"], min(self.maps_samples, s["B"]), s["heads"], self.n_probe(s["Lq"], s["n_obj"]), s["Nk"])
                if key not in self._maps:
                    if capturing:
                        raise RuntimeError("AttentionMonitor: block %d has no map buffer for this geometry and a stream "
                                           "capture cannot allocate: run the pass once outside a capture first" % key[0])
                    self._maps[key] = torch.zeros(key[1:], dtype=torch.float32, device=self.ring.device)
                self._maps_now[s["slot"]] = self._maps[key]
                s["maps"] = self._maps[key].data_ptr()
        T0, H0, W0 = st["thw0"]
        ops.attn_stats(sites, self.depth, self.ent_slots, self.kinds, self.K, self.every, self.maps_samples,
                       (st["B"], st["Tx"], T0, H0, W0), None if self.optimizer is None else self.optimizer.dev_rec,
                       self.ring, self.period, self.state, self.workspace)

    def reset(self):
        """forget every row: the ring as it was created, the counters at 0, no maps"""
        self.ring.copy_(torch.from_numpy(empty_ring(self.period, self.ent_slots).view(np.uint8).reshape(-1).copy()))
        self.state.copy_(torch.tensor([0, 0, -1, 0], dtype=torch.int64))
        self.last_row = -1

    # ---- reading -----------------------------------------------------------------------------------------------------
    def _ring_host(self):
        """the ring on the host as row_dtype rows: the ONE place `read()` reads the device"""
        return self.ring.cpu().numpy().view(row_dtype(self.ent_slots))

    def read(self):
        """the rows written since the last read, in order, as a dict: index ([(block, head, group)] per entry), passes,
        steps, header, lost (due passes since the last read the ring of R rows no longer holds: an overrun is reported,
        not raised) and arrays [rows, entries], masked where no site owned the entry or it has no good row -- entropy
        (mean over the good probe rows, bits), entropy_norm (the same / log2 Nk), entropy_min with min_row (`where()`
        unravels it), pmax (mean peak probability), mass_cls / mass_obj / mass_patch (mean attention on the cls, object
        and patch keys; patch = sum_p - cls - obj), sum_dev (the largest |sum_p - 1|: how far the probe lies from the
        fused kernel's lse2), n_bad, first_bad, rows."""
        rows, lost, self.last_row = read_rows(self._ring_host(), self.last_row)
        return rows_dict(self.plan, rows, self.group_names, lost)

    def where(self, header, block, head, code):
        """row code (min_row, first_bad) of (block, head) in a pass with that header -> (sample, head, token, kind)"""
        return where(self.plan, header, block, head, code)

    def unravel_key(self, block, k, header=None):
        """key k of `block` -> "cls", ("patch", t, h, w) or ("object", frame, o); header: a ring row's (default: the
        geometry of the model's training clip)"""
        return unravel_key(self.plan, train_geometry(self.plan) if header is None else header, block, k)

    def probe_rows(self, block, header=None, geom=None):
        """the probe rows (query tokens) of `block`, all groups in order, and the group of each, for a pass with that
        header (or geom = (Tx, T0, H0, W0); default: the geometry of the model's training clip)"""
        if header is None and geom is None:
            geom = train_geometry(self.plan)
        _, (t, h, w), _, n_obj = block_geometry(self.plan, *_geom(header if geom is None else geom))[block]
        groups = [group_rows(k, t * h * w, n_obj, self.K) for k in self.kinds]
        return (np.concatenate(groups),
                np.concatenate([np.full(len(g), i) for i, g in enumerate(groups)]).astype(np.int64))

    def maps(self):
        """(pass, {block: f32 tensor [samples, heads, n_probe, Nk]}): the probability rows of the latest pass that stored
        them (-1 and clones of zeros before the first); one synchronising read of the pass id"""
        p = int(self.state[2])
        return p, {b: t.clone() for b, t in sorted(self._maps_now.items())}

    def collapsed(self, rows, max_fraction):
        return collapsed(rows, max_fraction)

    def log_stats(self, rows):
        """the JSON line train_epoch logs: per block the mean over heads of the normalised entropy of each group, the
        smallest normalised entropy with its (block, head, group), the object-key mass per group and the largest sum_dev
        of the last row among `rows`; None when there is no row"""
        if not len(rows["passes"]):
            return None
        idx = rows["index"]

        def per_block(a, g):
            out = []
            for b in range(self.depth):
                v = np.ma.MaskedArray([a[-1][e] for e, (bb, _, gg) in enumerate(idx) if bb == b and gg == g]).compressed()
                out.append(None if not len(v) or not np.isfinite(v).all() else float("%.6g" % v.mean()))
            return out
        norm = rows["entropy_norm"][-1]
        low = None
        if norm.count():
            e = int(np.ma.argmin(norm))
            low = [float("%.6g" % norm[e])] + list(idx[e])
        dev = rows["sum_dev"][-1].compressed()
        return {"_type": "train_attention_stats", "pass": int(rows["passes"][-1]), "step": int(rows["steps"][-1]),
                "rows": int(len(rows["passes"])), "lost": int(rows["lost"]),
                "entropy_norm": {g: per_block(rows["entropy_norm"], g) for g in self.group_names},
                "mass_obj": {g: per_block(rows["mass_obj"], g) for g in self.group_names},
                "lowest": low, "sum_dev": float("%.6g" % dev.max()) if len(dev) else None,
                "n_bad": int(np.ma.filled(rows["n_bad"], 0).clip(min=0).sum())}

    attn_host = staticmethod(attn_host)


def probe_clip(model, video, rows=DEFAULT_ROWS, samples=None):
    """the attention maps of a (trained) model on one batch: ONE no-grad `engine.forward(video, save=True)` under a
    temporary monitor, whatever monitor was attached put back afterwards -> {block: (probe rows, f32 tensor
    [samples, heads, n_probe, Nk])}.  samples: the leading samples kept (default: all)."""
    core = model.module if hasattr(model, "module") else model
    B = video.shape[0]
    samples = B if samples is None else int(samples)
    mon = AttentionMonitor(core, 1, rows=rows, maps_samples=max(1, samples))
    old = core.engine.attn_monitor
    core.attach_attention_monitor(mon)
    try:
        with torch.no_grad():
            _, st = core.engine.forward(video, save=True)
    finally:
        core.attach_attention_monitor(old)
    _, maps = mon.maps()
    geom = (st["Tx"],) + tuple(st["thw0"])
    return {b: (mon.probe_rows(b, geom=geom)[0], m) for b, m in maps.items()}


def build_attnmon(cfg, model, optimizer=None, virtual_ranks=None):
    """SVIT.ATTN_MONITOR -> an AttentionMonitor of cfg.LOG_PERIOD * k rows attached to `model` (k: the virtual ranks one
    GPU runs per iteration, cfg.NUM_GPUS // world size unless given), or None without the key: no ring, not one launch
    more.  SVIT.ATTN_MONITOR_EVERY (1), SVIT.ATTN_MONITOR_ROWS (("cls", "obj", "patch:32")) and SVIT.ATTN_MONITOR_MAPS
    (0 samples) are read with getattr as well."""
    if not getattr(cfg.SVIT, "ATTN_MONITOR", False):
        return None
    period = cfg.LOG_PERIOD
    if isinstance(period, bool) or not isinstance(period, int) or period < 1:
        raise ValueError("SVIT.ATTN_MONITOR: cfg.LOG_PERIOD is a positive int, got %r" % (period,))
    every = getattr(cfg.SVIT, "ATTN_MONITOR_EVERY", 1)
    if isinstance(every, bool) or not isinstance(every, int) or every < 1:
        raise ValueError("SVIT.ATTN_MONITOR_EVERY is a positive int, got %r" % (every,))
    maps = getattr(cfg.SVIT, "ATTN_MONITOR_MAPS", 0)
    if isinstance(maps, bool) or not isinstance(maps, int) or maps < 0:
        raise ValueError("SVIT.ATTN_MONITOR_MAPS is a non-negative int (samples), got %r" % (maps,))
    rows = tuple(getattr(cfg.SVIT, "ATTN_MONITOR_ROWS", DEFAULT_ROWS))
    parse_rows(rows)
    if virtual_ranks is None:
        import torch.distributed as dist
        world = dist.get_world_size() if dist.is_available() and dist.is_initialized() else 1
        virtual_ranks = max(1, int(cfg.NUM_GPUS) // world)
    if isinstance(virtual_ranks, bool) or not isinstance(virtual_ranks, int) or virtual_ranks < 1:
        raise ValueError("build_attnmon: virtual_ranks is a positive int, got %r" % (virtual_ranks,))
    core = model.module if hasattr(model, "module") else model
    mon = AttentionMonitor(core, period * virtual_ranks, optimizer=optimizer, rows=rows, every=every, maps_samples=maps)
    core.attach_attention_monitor(mon)
    return mon
