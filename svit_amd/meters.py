"""Train / val meters whose per-iteration numbers stay on the device.

The reference's `train_epoch` reads every entry of the loss dict with `.item()` in every iteration
(tools/train_net.py:153-167) and its `eval_epoch` two top-k errors (tools/train_net.py:325-335): a host round trip per
step.  Here one launch per iteration (`svit_meter_push`, csrc/meter.hip) copies the 0-d loss tensors -- and, for
validation, counts the top-k hits of the batch -- into row `state[0] % W` of an fp32 ring in device memory, W =
cfg.LOG_PERIOD, and advances `state[0]` itself, so the launch can live inside a replayed graph
(graph.GraphedTrainStep(meter=)).  `log_iter_stats` reads ring and state ONCE per period -- the only synchronisation --
and feeds the rows, in push order, to host meters that do what the reference's do (slowfast/utils/meters.py:401-709,
793-866): `np.median` over the window, Python-double totals, and for validation `(1.0 - x / N) * 100.0` in fp32.  The
logged numbers equal the reference's.

Stated differences: `time_diff` is the wall time since the previous read divided by the iterations in it (no per-step
sync exists to time one iteration); `mem` / `gpu_mem` is torch.cuda.max_memory_allocated in GB; `RAM` is omitted where
psutil is absent.

Failures are raised at the read: a ring that overran (`log_iter_stats` must be called every iteration), a NaN `loss`
(check_nan_losses's message, naming the first bad iteration: a caller that uses the meter needs no misc.NanWatch);
labels outside [0, C) are counted into the epoch stats as `bad_labels`.

Data parallel: at the period the ranks' rings are gathered with ONE all_gather (device tensors where the default
group's backend takes them, host copies under gloo); column names are exchanged once.  Training merges per iteration
and key as tools/train_net.py:153-161 does (`sum(v) / len(v)` in Python double over the ranks that have the key, in rank
order: video and image ranks log different keys), validation as du.all_reduce does (slowfast/utils/distributed.py:
38-54: fp32 sum in rank order, times fp32 `1.0 / world`).
"""
import ctypes
import datetime
import json
import logging
import time
from collections import deque

import numpy as np
import torch
import torch.distributed as dist

from . import hip, misc

logger = logging.getLogger(__name__)
MAX_SCALARS = 16


class ScalarMeter(object):
    """slowfast/utils/meters.py:401-450: a window of the last `window_size` values plus a global total."""

    def __init__(self, window_size):
        self.deque = deque(maxlen=window_size)
        self.total = 0.0
        self.count = 0

    def reset(self):
        self.deque.clear()
        self.total = 0.0
        self.count = 0

    def add_value(self, value):
        if value is None:
            return
        self.deque.append(value)
        self.count += 1
        self.total += value

    def get_win_median(self):
        return np.median(self.deque)

    def get_win_avg(self):
        return np.mean(self.deque)

    def get_global_avg(self):
        return self.total / self.count


class MultiLossMeter(object):
    """slowfast/utils/meters.py:793-846: one ScalarMeter per key of the dicts it is fed (host floats here)."""

    def __init__(self, window_size, prefix=None):
        self.window_size = window_size
        self.prefix = prefix
        self.losses = dict()

    def add_prefix(self, d):
        if self.prefix is None:
            return d
        return {f"{self.prefix}_{k}": v for k, v in d.items()}

    def reset(self):
        for m in self.losses.values():
            m.reset()

    def add_value(self, value):
        if value is None:
            return
        for k, v in value.items():
            if torch.is_tensor(v):
                v = v.item()
            if k not in self.losses:
                self.losses[k] = ScalarMeter(self.window_size)
            self.losses[k].add_value(v)

    def get_win_median(self):
        return self.add_prefix({k: v.get_win_median() for k, v in self.losses.items()})

    def get_win_avg(self):
        return self.add_prefix({k: v.get_win_avg() for k, v in self.losses.items()})

    def get_global_avg(self):
        return self.add_prefix({k: v.get_global_avg() for k, v in self.losses.items()})


def log_json_stats(stats):
    """slowfast/utils/logging.py:89-101: one JSON line, floats with five decimals"""
    line = {k: float("{:.5f}".format(v)) if isinstance(v, float) else v for k, v in stats.items()}
    logger.info("json_stats: {:s}".format(json.dumps(line, sort_keys=True)))


def _gpu_mem_gb(device):
    if device.type != "cuda":
        return 0.0
    return torch.cuda.max_memory_allocated(device) / 1024 ** 3


def _label_hits(logits, labels, ks):
    """the kernel's counts with torch ops (CPU meters only): rank = classes with a larger score, or an equal score and a
    lower index; a label outside [0, C) reads nothing and counts as wrong -> ([hits k0, hits k1], bad labels)"""
    n, c = logits.shape
    ok = (labels >= 0) & (labels < c)
    lab = torch.where(ok, labels, torch.zeros_like(labels))
    s = logits.gather(1, lab[:, None])
    idx = torch.arange(c)[None, :]
    rank = ((logits > s) | ((logits == s) & (idx < lab[:, None]))).sum(1)
    return [int(((rank < k) & ok).sum()) for k in ks], int((~ok).sum())


class _DeviceMeter:
    """What TrainMeter and ValMeter share: the ring, the push, the one read per period, the data-parallel gather."""
    topk = False
    nan_key = None
    _label = ""                        # (a virtual rank's ring names itself in the NaN message)

    def __init__(self, cfg, device=None, force_collectives=False):
        if device is None:
            device = torch.device("cuda", torch.cuda.current_device()) if torch.cuda.is_available() else "cpu"
        self.device = torch.device(device)
        self._cfg = cfg
        self.window = int(cfg.LOG_PERIOD)
        if self.window <= 0:
            raise ValueError("cfg.LOG_PERIOD must be positive, got %r" % (cfg.LOG_PERIOD,))
        self.force_collectives = force_collectives
        self.names = None              # column names, fixed by the first update
        self.buf = self.state = self.ring = None
        self._read = 0                 # pushes the host has seen (state[0] at the last read)
        self._host = []                # the host half of every push since the last read
        self._rank_names = None
        self._t_read = time.time()
        self.time_diff = 0.0
        self.bad_labels = 0

    # ---- device half ---------------------------------------------------------------------------------------------
    def bind(self, scalars):
        """fix the column names and allocate ring and state (first update; a graph capture calls it while warming up,
        so that the capture itself allocates nothing)"""
        names = list(scalars)
        if self.names is not None:
            if names != self.names:
                raise ValueError("the meter's columns were fixed by the first update as %s, this update has %s"
                                 % (self.names, names))
            return
        if len(names) > MAX_SCALARS:
            raise ValueError("a meter row takes at most %d scalars, got %d" % (MAX_SCALARS, len(names)))
        self.names = names
        k = len(names) + (2 if self.topk else 0)
        if k == 0:
            raise ValueError("nothing to record: an empty loss dict")
        # state (int64 [2] = pushes, labels out of range) and ring (f32 [W, K]) in ONE buffer: one copy reads both
        self.buf = torch.zeros(4 + self.window * k, dtype=torch.int32, device=self.device)
        self.state = self.buf[:4].view(torch.int64)
        self.ring = self.buf[4:].view(torch.float32).view(self.window, k)
        self._ptrs = (ctypes.c_void_p * MAX_SCALARS)()

    def _scalars(self, scalars):
        out = []
        for k in self.names:
            v = scalars[k]
            if not torch.is_tensor(v):
                v = torch.tensor(float(v), dtype=torch.float32)
            v = v.detach()
            if v.numel() != 1:
                raise ValueError("meter entry %r is not a scalar: shape %s" % (k, tuple(v.shape)))
            if v.dtype != torch.float32 or v.device != self.device:
                v = v.to(self.device, torch.float32)
            out.append(v)
        return out

    def push(self, scalars, logits=None, labels=None, ks=(1, 5)):
        """record one iteration on the device: enqueue only (capturable on the GPU)"""
        self.bind(scalars)
        vals = self._scalars(scalars)
        w, k = self.ring.shape
        if self.topk:
            logits = logits.detach().to(self.device, torch.float32).contiguous()
            labels = labels.detach().to(self.device, torch.int64).contiguous()
            if logits.dim() != 2 or labels.shape != logits.shape[:1]:
                raise ValueError("update_stats: preds %s labels %s" % (tuple(logits.shape), tuple(labels.shape)))
        if self.device.type == "cuda":
            for i, v in enumerate(vals):
                self._ptrs[i] = v.data_ptr()
            n, c = logits.shape if self.topk else (0, 0)
            hip.call("svit_meter_push", hip.ptr(self.ring), w, k, hip.ptr(self.state), self._ptrs, len(vals),
                     hip.ptr(logits) if self.topk else None, hip.ptr(labels) if self.topk else None, n, c,
                     int(ks[0]), int(ks[1]))
            self._alive = (vals, logits, labels)      # (addresses a captured launch keeps reading)
            return
        r = int(self.state[0]) % w
        bits = self.ring.view(torch.int32)
        for i, v in enumerate(vals):
            bits[r, i] = v.reshape(()).view(torch.int32)
        if self.topk:
            if not all(1 <= kk <= logits.shape[1] for kk in ks):
                raise ValueError("ks %s outside [1, %d]" % (tuple(ks), logits.shape[1]))
            hits, bad = _label_hits(logits, labels, ks)
            self.ring[r, len(vals)] = float(hits[0])
            self.ring[r, len(vals) + 1] = float(hits[1])
            self.state[1] += bad
        self.state[0] += 1

    def host_update(self, *record):
        """the host half of an update (what never travels to the device: lr, mb_size, the batch's N)"""
        self._host.append(record)

    def _reset_device(self):
        if self.buf is not None:
            self.state.zero_()         # stream-ordered, no sync: pushes not yet read are discarded
        self._read = 0
        self._host = []
        self.bad_labels = 0
        self._t_read = time.time()

    # ---- the read ------------------------------------------------------------------------------------------------
    def _collective(self):
        if not (dist.is_available() and dist.is_initialized()):
            return False
        return dist.get_world_size() > 1 or self.force_collectives

    def _on_device(self):
        return self.device.type == "cuda" and "nccl" in str(dist.get_backend())

    def _payload(self, kmax):
        """what a rank sends at the period: state | the batch sizes of the rows (host knowledge the other ranks lack) |
        ring padded to kmax columns (host copies under gloo: the one synchronisation)"""
        w, k = self.ring.shape
        ns = [int(h[-1]) for h in self._host] if self.topk else []
        src = self.buf if self._on_device() else self.buf.cpu()
        payload = torch.zeros(4 + w + w * kmax, dtype=torch.int32, device=src.device)
        payload[:4] = src[:4]
        if ns:
            rows = [(self._read + i) % w for i in range(min(len(ns), w))]
            size = torch.zeros(w, dtype=torch.int32)
            size[rows] = torch.tensor(ns[:w], dtype=torch.int32)
            payload[4:4 + w] = size.to(src.device, non_blocking=True)
        payload[4 + w:].view(w, kmax)[:, :k] = src[4:].view(w, k)
        return payload

    def _all_gather(self, payload):
        """ONE all_gather -> the ranks' payloads on the host"""
        world = dist.get_world_size()
        if self._on_device():
            out = torch.empty(world * payload.numel(), dtype=torch.int32, device=payload.device)
            dist.all_gather_into_tensor(out, payload)
            return list(out.cpu().view(world, -1))                  # the one synchronisation
        parts = [torch.empty_like(payload) for _ in range(world)]
        dist.all_gather(parts, payload)
        return parts

    def _parse(self, names, p, kmax):
        """a rank's payload -> (its column names, its state + ring as it holds them, the batch sizes of its rows)"""
        w = self.window
        kr = len(names) + (2 if self.topk else 0)
        own = torch.cat((p[:4], p[4 + w:].view(w, kmax)[:, :kr].reshape(-1)))
        return names, own, p[4:4 + w]

    def _drain(self, ranks=None):
        """-> [(host record, [row of rank 0, row of rank 1, ...])] of the pushes since the last read, in push order; a
        rank's row is {name: python float} (+ "_hits": (fp32 count, fp32 count), "_n": rows of its batch).  ranks: what
        `_parse` gave for every rank, when the owner of several rings gathered them together"""
        if self.buf is None:
            return []
        w, k = self.ring.shape
        ns = [int(h[-1]) for h in self._host] if self.topk else []
        if ranks is not None:
            pass
        elif not self._collective():
            ranks = [(self.names, self.buf.cpu(), None)]            # the one synchronisation of the period
        else:
            if self._rank_names is None:                            # once
                got = [None] * dist.get_world_size()
                dist.all_gather_object(got, self.names)
                self._rank_names = got
            kmax = max(len(n) for n in self._rank_names) + (2 if self.topk else 0)
            parts = self._all_gather(self._payload(kmax))
            ranks = [self._parse(names, p, kmax) for names, p in zip(self._rank_names, parts)]
        out = None
        for rank, (names, host, sizes) in enumerate(ranks):
            pushes, bad = (int(v) for v in host[:4].view(torch.int64))
            new = pushes - self._read
            if new > w:
                raise RuntimeError("the meter's ring of cfg.LOG_PERIOD = %d rows overran: %d iterations were pushed "
                                   "since the last read -- log_iter_stats must be called every iteration" % (w, new))
            if new != len(self._host):
                raise RuntimeError("rank %d pushed %d iterations since the last read, the host half of update_stats "
                                   "ran %d times" % (rank, new, len(self._host)))
            if out is None:
                out = [(h, []) for h in self._host]
                self.bad_labels = 0
            self.bad_labels += bad
            ring = host[4:].view(torch.float32).view(w, -1)
            for i in range(new):
                r = (self._read + i) % w
                vals = ring[r].tolist()
                row = dict(zip(names, vals))
                if self.nan_key in row:
                    misc.check_nan_losses(row[self.nan_key], extra_msg="first at iteration %d of the epoch%s, %s" % (
                        self._read + i, ("" if len(ranks) == 1 else " (rank %d)" % rank) + self._label, row))
                if self.topk:
                    row["_hits"] = (vals[len(names)], vals[len(names) + 1])
                    row["_n"] = int(sizes[r]) if sizes is not None else ns[i]
                out[i][1].append(row)
        n_new = len(self._host)
        self._read += n_new
        self._host = []
        now = time.time()
        if n_new:
            self.time_diff = (now - self._t_read) / n_new
        self._t_read = now
        return out

    # timers of the reference's meters: no per-step sync exists to time, see `time_diff`
    def iter_tic(self):
        pass

    def iter_toc(self):
        pass

    def data_toc(self):
        pass


class _Ring(_DeviceMeter):
    """the ring of ONE virtual rank of a TrainMeter(virtual_ranks=k): its own column names, buffer and counter"""
    nan_key = "loss"

    def __init__(self, cfg, device, force_collectives, vrank):
        super().__init__(cfg, device, force_collectives)
        self._label = " (virtual rank %d)" % vrank


class TrainMeter(_DeviceMeter):
    """slowfast/utils/meters.py:454-560 with the loss dict left on the device.

    virtual_ranks=k (graph.AccumulatedTrainStep, train.accumulate_step): one real rank runs k recipe ranks per
    iteration, whose key sets differ (video and image ranks) -- the meter then keeps ONE RING PER VIRTUAL RANK, each with
    its own column names and push counter (`push(scalars, vrank=i)`; `svit_meter_push` as it is), and one host record
    per iteration.  At the period every ring is read as a plain meter's is (across real ranks: the ONE all_gather
    carries the k rings), and the rows of an iteration are merged in recipe-rank order -- real rank r, virtual rank i is recipe rank r*k + i --
    by the same `sum(v) / len(v)` over the recipe ranks that logged the key: what the k x world-rank job logs.  None:
    the one ring, buffer layout, payload and numbers of a plain meter."""
    nan_key = "loss"

    def __init__(self, epoch_iters, cfg, device=None, force_collectives=False, virtual_ranks=None):
        super().__init__(cfg, device, force_collectives)
        self.epoch_iters = epoch_iters
        self.multi_loss = MultiLossMeter(cfg.LOG_PERIOD)
        self.MAX_EPOCH = cfg.SOLVER.MAX_EPOCH * epoch_iters
        self.lr = None
        self.num_samples = 0
        self.virtual_ranks = None if virtual_ranks is None else int(virtual_ranks)
        self._rings = None
        if self.virtual_ranks is not None:
            if self.virtual_ranks < 1:
                raise ValueError("virtual_ranks must be positive, got %r" % (virtual_ranks,))
            self._rings = [_Ring(cfg, self.device, force_collectives, i) for i in range(self.virtual_ranks)]

    def reset(self):
        self.multi_loss.reset()
        self.lr = None
        self.num_samples = 0
        self._reset_device()
        for ring in self._rings or ():
            ring._reset_device()

    # ---- virtual ranks: the device half goes to the rank's ring, the host half to all of them -----------------------
    def _ring(self, vrank):
        if self._rings is None:
            if vrank is not None:
                raise ValueError("push(vrank=%r) on a TrainMeter built without virtual_ranks" % (vrank,))
            return None
        if vrank is None or not 0 <= int(vrank) < len(self._rings):
            raise ValueError("a TrainMeter(virtual_ranks=%d) takes push(scalars, vrank=i) with i in [0, %d), got %r"
                             % (len(self._rings), len(self._rings), vrank))
        return self._rings[int(vrank)]

    def bind(self, scalars, vrank=None):
        ring = self._ring(vrank)
        return super().bind(scalars) if ring is None else ring.bind(scalars)

    def push(self, scalars, vrank=None, **kw):
        ring = self._ring(vrank)
        return super().push(scalars, **kw) if ring is None else ring.push(scalars)

    def host_update(self, *record):
        super().host_update(*record)
        for ring in self._rings or ():
            ring.host_update(*record)

    def _drain(self):
        if self._rings is None:
            return super()._drain()
        host, self._host = self._host, []
        rings = self._rings
        if self._collective() and all(r.buf is not None for r in rings):
            # the one all_gather of a plain meter carries the k rings, every one padded to the widest of all ranks
            if self._rank_names is None:                            # once: per real rank, the k lists of column names
                got = [None] * dist.get_world_size()
                dist.all_gather_object(got, [r.names for r in rings])
                self._rank_names = got
            kmax = max(len(n) for names in self._rank_names for n in names)
            parts = self._all_gather(torch.cat([r._payload(kmax) for r in rings]))
            per = [ring._drain(ranks=[ring._parse(names[v], p.view(len(rings), -1)[v], kmax)
                                      for names, p in zip(self._rank_names, parts)])
                   for v, ring in enumerate(rings)]
        else:
            per = [ring._drain() for ring in rings]             # per ring: [(host record, [row of real rank 0, 1, ...])]
        for i, got in enumerate(per):
            if len(got) != len(host):
                raise RuntimeError("virtual rank %d pushed %d iterations since the last read, the host half of "
                                   "update_stats ran %d times" % (i, len(got), len(host)))
        out = []
        for it, h in enumerate(host):
            by_ring = [got[it][1] for got in per]
            world = len(by_ring[0])
            out.append((h, [by_ring[v][r] for r in range(world) for v in range(len(per))]))     # recipe-rank order
        self.time_diff = self._rings[0].time_diff
        return out

    def update_stats(self, lr, mb_size, dloss=None, is_video=True):
        """dloss: {name: 0-d device tensor}; nothing is read back here"""
        if self._rings is not None:
            raise ValueError("a TrainMeter(virtual_ranks=...) is fed by push(scalars, vrank=i) per micro-step and one "
                             "host_update(lr, mb_size) per iteration")
        if not isinstance(dloss, dict):
            dloss = {"loss": dloss}
        self.push(dloss)
        self.host_update(lr, mb_size)

    def _feed(self):
        for (lr, mb_size), rows in self._drain():
            merged = {}
            for d in rows:                                   # tools/train_net.py:153-161, ranks in order
                for k, v in d.items():
                    merged.setdefault(k, []).append(v)
            self.multi_loss.add_value({k: sum(v) / len(v) for k, v in merged.items()})
            self.lr = lr
            self.num_samples += mb_size

    def _stats(self, kind, cur_epoch, done):
        eta_sec = self.time_diff * (self.MAX_EPOCH - done)
        return {"_type": kind, "epoch": "{}/{}".format(cur_epoch + 1, self._cfg.SOLVER.MAX_EPOCH),
                "iter": "{}/{}".format(done - cur_epoch * self.epoch_iters, self.epoch_iters),
                "time_diff": self.time_diff, "eta": str(datetime.timedelta(seconds=int(eta_sec))), "lr": self.lr,
                "mem": int(np.ceil(_gpu_mem_gb(self.device)))}

    def log_iter_stats(self, cur_epoch, cur_iter):
        if (cur_iter + 1) % self._cfg.LOG_PERIOD != 0:
            return None
        self._feed()
        stats = self._stats("train_iter", cur_epoch, cur_epoch * self.epoch_iters + cur_iter + 1)
        stats.update(self.multi_loss.get_win_median())
        log_json_stats(stats)
        return stats

    def log_epoch_stats(self, cur_epoch):
        self._feed()                                         # what was pushed since the last period
        stats = self._stats("train_epoch", cur_epoch, (cur_epoch + 1) * self.epoch_iters)
        del stats["iter"]
        stats.update(self.multi_loss.get_global_avg())
        log_json_stats(stats)
        return stats


class ValMeter(_DeviceMeter):
    """slowfast/utils/meters.py:565-709 for single-label classification: the top-k hits of a batch are counted on the
    device, the errors formed from them on the host in fp32 as tools/train_net.py:328-330 forms them."""
    topk = True

    def __init__(self, max_iter, cfg, device=None, force_collectives=False):
        super().__init__(cfg, device, force_collectives)
        if cfg.DATA.MULTI_LABEL:
            raise NotImplementedError("multi-label (mAP) validation is not part of the SViT path")
        self.max_iter = max_iter
        self.ks = (1, 5) if cfg.MODEL.NUM_CLASSES > 5 else (1, 1)
        self.mb_top1_err = ScalarMeter(cfg.LOG_PERIOD)
        self.mb_top5_err = ScalarMeter(cfg.LOG_PERIOD)
        self.extra_metrices = MultiLossMeter(cfg.LOG_PERIOD, prefix="extra_meter")
        self.min_top1_err = 100.0
        self.min_top5_err = 100.0
        self.num_top1_mis = 0
        self.num_top5_mis = 0
        self.num_samples = 0
        self.output_dir = cfg.OUTPUT_DIR

    def reset(self):
        self.mb_top1_err.reset()
        self.mb_top5_err.reset()
        self.extra_metrices.reset()
        self.num_top1_mis = 0
        self.num_top5_mis = 0
        self.num_samples = 0
        self._reset_device()

    def update_stats(self, preds, labels, mb_size, extra_metrices={}):
        """preds f32 [N,C] logits and labels int64 [N] of this rank's batch, extra_metrices {name: 0-d tensor}: all
        left on the device"""
        self.push(dict(extra_metrices), preds, labels, self.ks)
        self.host_update(mb_size, int(preds.shape[0]))

    def _feed(self):
        one, hundred = np.float32(1.0), np.float32(100.0)
        for (mb_size, _n), rows in self._drain():
            world = len(rows)
            errs = []
            for j in range(2):
                per_rank = [(one - np.float32(d["_hits"][j]) / np.float32(d["_n"])) * hundred for d in rows]
                errs.append(self._mean(per_rank, world))
            extra = {}
            for k in self.names:
                if any(k not in d for d in rows):
                    raise RuntimeError("validation ranks log different extra metrics (%r): du.all_reduce has no such "
                                       "case" % k)
                extra[k] = self._mean([np.float32(d[k]) for d in rows], world)
            top1_err, top5_err = errs
            self.mb_top1_err.add_value(top1_err)
            self.mb_top5_err.add_value(top5_err)
            self.num_top1_mis += top1_err * mb_size
            self.num_top5_mis += top5_err * mb_size
            self.num_samples += mb_size
            self.extra_metrices.add_value(extra)

    @staticmethod
    def _mean(vals, world):
        """du.all_reduce (slowfast/utils/distributed.py:38-54) on fp32: sum in rank order, times fp32 1.0 / world"""
        if world == 1:
            return float(vals[0])
        acc = vals[0]
        for v in vals[1:]:
            acc = np.float32(acc + v)
        return float(np.float32(acc * np.float32(1.0 / world)))

    def _head(self, kind, cur_epoch):
        return {"_type": kind, "epoch": "{}/{}".format(cur_epoch + 1, self._cfg.SOLVER.MAX_EPOCH)}

    def log_iter_stats(self, cur_epoch, cur_iter):
        if (cur_iter + 1) % self._cfg.LOG_PERIOD != 0:
            return None
        self._feed()
        eta_sec = self.time_diff * (self.max_iter - cur_iter - 1)
        stats = self._head("val_iter", cur_epoch)
        stats.update({"iter": "{}/{}".format(cur_iter + 1, self.max_iter), "time_diff": self.time_diff,
                      "eta": str(datetime.timedelta(seconds=int(eta_sec))),
                      "gpu_mem": "{:.2f}G".format(_gpu_mem_gb(self.device)),
                      "top1_err": self.mb_top1_err.get_win_median(), "top5_err": self.mb_top5_err.get_win_median()})
        stats.update(self.extra_metrices.get_win_median())
        log_json_stats(stats)
        return stats

    def log_epoch_stats(self, cur_epoch):
        self._feed()                                         # what was pushed since the last period
        stats = self._head("val_epoch", cur_epoch)
        stats.update({"time_diff": self.time_diff, "gpu_mem": "{:.2f}G".format(_gpu_mem_gb(self.device))})
        try:
            import psutil
            vram = psutil.virtual_memory()
            stats["RAM"] = "{:.2f}/{:.2f}G".format((vram.total - vram.available) / 1024 ** 3, vram.total / 1024 ** 3)
        except ImportError:
            pass
        if self.num_samples > 0:
            top1_err = self.num_top1_mis / self.num_samples
            top5_err = self.num_top5_mis / self.num_samples
            self.min_top1_err = min(self.min_top1_err, top1_err)
            self.min_top5_err = min(self.min_top5_err, top5_err)
            stats.update({"top1_err": top1_err, "top5_err": top5_err, "min_top1_err": self.min_top1_err,
                          "min_top5_err": self.min_top5_err})
        stats.update(self.extra_metrices.get_global_avg())
        if self.bad_labels:
            stats["bad_labels"] = self.bad_labels
        log_json_stats(stats)
        return stats
