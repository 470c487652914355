"""The device side of the meters on a real MI355X: `svit_meter_push` through the C ABI (counts against torch.topk,
scalars bit for bit, ties, labels out of range, canaries, the ring walk, the 16-scalar limit, graph replay), the push
inside graph.GraphedTrainStep(meter=), the poisoned step, train.eval_epoch, and the data-parallel merge."""
import ctypes
import os
import socket
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import procedural as P
from tests import smoke_impl as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda"
CANARY = 0x5A5A5A5A
PAD = 8
TIMING = ("time_diff", "eta", "mem", "gpu_mem", "RAM")


class Arena:
    """ring and state between canary words: [PAD | state int64 [2] | PAD | ring f32 [W,K] | PAD] in one int32 buffer"""

    def __init__(self, W, K):
        self.W, self.K = W, K
        self.buf = torch.full((3 * PAD + 4 + W * K,), CANARY, dtype=torch.int32, device=DEV)
        self.state = self.buf[PAD:PAD + 4].view(torch.int64)
        self.ring_bits = self.buf[2 * PAD + 4:2 * PAD + 4 + W * K].view(W, K)
        self.ring = self.ring_bits.view(torch.float32)
        self.state.zero_()
        self.ring_bits.zero_()

    def canaries_intact(self):
        b = self.buf.cpu()
        pads = torch.cat((b[:PAD], b[PAD + 4:2 * PAD + 4], b[-PAD:]))
        return bool((pads == CANARY).all())


def raw_push(arena, scalars, logits=None, labels=None, ks=(1, 5), K=None, check=True):
    """-> the return code of svit_meter_push (raises on a non-zero one when `check`)"""
    from svit_amd import hip
    ptrs = (ctypes.c_void_p * max(len(scalars), 1))(*[t.data_ptr() for t in scalars])
    n, c = logits.shape if logits is not None else (0, 0)
    rc = hip.load().svit_meter_push(arena.ring.data_ptr(), arena.W, arena.K if K is None else K, arena.state.data_ptr(),
                                    ptrs, len(scalars), hip.ptr(logits), hip.ptr(labels), n, c, ks[0], ks[1],
                                    hip.stream())
    if check:
        hip.check(rc, "svit_meter_push")
    return rc


def bits(values):
    """fp32 scalars from bit patterns -> list of 0-d device tensors"""
    t = torch.tensor(values, dtype=torch.int64).to(torch.int32).to(DEV).view(torch.float32)
    return [t[i] for i in range(len(values))], t


def perm_logits(n, c, seed):
    """distinct scores per row (a permutation): torch.topk has no ties to break"""
    g = torch.Generator().manual_seed(seed)
    rows = torch.stack([torch.randperm(c, generator=g) for _ in range(n)]).float() / 7.0 - 3.0
    labels = torch.randint(0, c, (n,), generator=g)
    labels[0] = int(rows[0].argmax())
    return rows, labels


def topk_counts(logits, labels, ks):
    """metrics.topks_correct (slowfast/utils/metrics.py:9-50) on CPU tensors"""
    _, inds = torch.topk(logits, max(ks), dim=1, largest=True, sorted=True)
    correct = inds.t().eq(labels.view(1, -1).expand_as(inds.t()))
    return [float(correct[:k, :].float().sum()) for k in ks]


# NaN with a payload, -NaN, +inf, -inf, -0.0, a denormal, 1.5
SPECIAL = [0x7FC12345, 0xFFFFFFFF - (1 << 32), 0x7F800000, 0xFF800000 - (1 << 32), 0x80000000 - (1 << 32), 0x00000001,
           0x3FC00000]


@pytest.mark.parametrize("C", [2, 5, 6, 174, 1000])
@pytest.mark.parametrize("N", [1, 2, 7, 64, 257])
def test_push_counts_and_scalars(N, C):
    ks = (1, 5) if C > 5 else (1, 1)
    logits, labels = perm_logits(N, C, 1000 * N + C)
    scalars, packed = bits(SPECIAL)
    a = Arena(2, len(scalars) + 2)
    raw_push(a, scalars, logits.to(DEV), labels.to(DEV), ks)
    torch.cuda.synchronize()
    row = a.ring_bits[0].cpu()
    assert torch.equal(row[:len(scalars)], packed.view(torch.int32).cpu())          # bit-equal: NaN payload, -0.0
    assert a.ring[0, -2:].tolist() == topk_counts(logits, labels, ks)
    assert a.state.tolist() == [1, 0] and bool((a.ring_bits[1] == 0).all()) and a.canaries_intact()


@pytest.mark.parametrize("C", [6, 174])
def test_tie_rows(C):
    """all scores equal: the class with the lower index is ahead, so label L has rank L"""
    labs = [0, 4, 5, C - 1]
    labels = torch.tensor(labs, device=DEV)
    a = Arena(1, 2)
    for ks in ((1, 5), (5, 6), (6, C)):
        raw_push(a, [], torch.full((4, C), 0.25, device=DEV), labels, ks)
        assert a.ring[0].tolist() == [float(sum(l < k for l in labs)) for k in ks], ks
    assert a.state.tolist() == [3, 0]
    # equal scores among larger and smaller ones: 9 is ahead of every 2, and a 2 with a lower index ahead of a later 2
    x = torch.tensor([[0.0, 2.0, 9.0, 2.0, 2.0, -1.0]], device=DEV)
    for lab, rank in ((1, 1), (3, 2), (4, 3), (2, 0), (0, 4), (5, 5)):
        raw_push(a, [], x, torch.tensor([lab], device=DEV), (rank + 1, max(rank, 1)))
        assert a.ring[0].tolist() == [1.0, 1.0 if rank == 0 else 0.0], (lab, rank)
    assert a.canaries_intact()


def test_labels_out_of_range_read_nothing():
    N, C = 7, 6
    logits, labels = perm_logits(N, C, 5)
    labels[2], labels[5] = -1, C
    a = Arena(2, 3)
    # the logits sit between canaries too: a label outside [0, C) must not be used as an index
    box = torch.full((2 * PAD + N * C,), float("inf"), device=DEV)
    box[PAD:PAD + N * C] = logits.flatten().to(DEV)
    one, _ = bits([0x3F800000])
    for i in range(3):
        raw_push(a, one, box[PAD:PAD + N * C].view(N, C), labels.to(DEV), (1, 5))
    ok = (labels >= 0) & (labels < C)
    want = topk_counts(logits[ok], labels[ok], (1, 5))
    assert a.state.tolist() == [3, 6]
    assert a.ring[0].tolist() == [1.0] + want and a.ring[1].tolist() == [1.0] + want
    assert a.canaries_intact()
    assert bool(torch.isinf(box[:PAD]).all()) and bool(torch.isinf(box[-PAD:]).all())
    # every label bad: zero hits
    raw_push(a, one, logits.to(DEV), torch.full((N,), C + 5, device=DEV), (1, 5))
    assert a.ring[1].tolist() == [1.0, 0.0, 0.0] and a.state.tolist() == [4, 6 + N]


def test_rows_walk_the_ring_and_the_16_scalar_limit():
    W = 3
    a = Arena(W, 16)
    vals = torch.arange(16.0 * (2 * W + 3), device=DEV).view(-1, 16) + 0.5
    for i in range(2 * W + 3):
        raw_push(a, [vals[i, j] for j in range(16)])                 # 16 scalars: the most a row takes
        assert int(a.state[0]) == i + 1
        assert torch.equal(a.ring[i % W], vals[i]), i
        for r in range(W):                                           # the other rows keep their last push
            last = max((p for p in range(i + 1) if p % W == r), default=None)
            assert torch.equal(a.ring[r], vals[last] if last is not None else torch.zeros(16, device=DEV))
    before = a.buf.clone()
    b = Arena(W, 17)
    assert raw_push(b, [vals[0, j % 16] for j in range(17)], check=False) == -2         # refused ...
    assert raw_push(a, [vals[0, j] for j in range(16)], K=15, check=False) == -2
    torch.cuda.synchronize()
    assert b.state.tolist() == [0, 0] and torch.equal(a.buf, before)                    # ... without a launch
    assert a.canaries_intact() and b.canaries_intact()


def test_graph_replay_walks_the_rows_by_itself():
    W, N, C = 3, 7, 174
    s_static = torch.zeros(2, device=DEV)
    x_static = torch.zeros(N, C, device=DEV)
    y_static = torch.zeros(N, dtype=torch.int64, device=DEV)
    inputs = []
    for i in range(2 * W + 3):
        x, y = perm_logits(N, C, 77 + i)
        inputs.append((torch.tensor([i + 0.25, -i - 0.5]), x, y))
    eager, graphed = Arena(W, 4), Arena(W, 4)
    snaps = []
    for s, x, y in inputs:
        raw_push(eager, list(s.to(DEV)), x.to(DEV), y.to(DEV))
        snaps.append(eager.buf.clone())
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        raw_push(Arena(W, 4), [s_static[0], s_static[1]], x_static, y_static)        # code loaded before the capture
    torch.cuda.current_stream().wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        raw_push(graphed, [s_static[0], s_static[1]], x_static, y_static)
    torch.cuda.synchronize()
    assert graphed.state.tolist() == [0, 0]                          # a capture runs nothing
    for i, (s, x, y) in enumerate(inputs):
        s_static.copy_(s)
        x_static.copy_(x)
        y_static.copy_(y)
        g.replay()
        assert torch.equal(graphed.buf, snaps[i]), i
    assert graphed.state.tolist() == [2 * W + 3, 0] and graphed.canaries_intact()


# ------------------------------------------------------------------------------------------------- model level
def _tiny(period):
    cfg, model, _, _ = S.build_hip_model(4, 64)
    model.engine.reproducible = True
    cfg.LOG_PERIOD = period
    return cfg, model


def numbers(stats):
    return None if stats is None else {k: (float(v) if isinstance(v, float) else v) for k, v in stats.items()
                                       if k not in TIMING}


class _NoSync:
    """torch.cuda.set_sync_debug_mode("error") around everything but the meter's read"""

    def __init__(self, meter):
        self.meter, self.drain = meter, meter._drain

    def __enter__(self):
        self.mode = torch.cuda.get_sync_debug_mode()

        def drain():
            torch.cuda.set_sync_debug_mode(self.mode)
            try:
                return self.drain()
            finally:
                torch.cuda.set_sync_debug_mode("error")
        self.meter._drain = drain
        torch.cuda.synchronize()
        torch.cuda.set_sync_debug_mode("error")
        return self

    def __exit__(self, *exc):
        torch.cuda.set_sync_debug_mode(self.mode)
        self.meter._drain = self.drain


def test_push_inside_the_replayed_step():
    """arm A: GraphedTrainStep(optimizer=, meter=), one read per LOG_PERIOD = 3; arm B: the same step without a meter,
    float() on every entry after every replay, fed to the host meters.  Seven replays (2 periods + 1 drained by the
    epoch line): every logged number is ==, and so are the weights."""
    from svit_amd import losses, meters, optim
    from svit_amd.graph import GraphedTrainStep
    cfg, ma = _tiny(3)
    _, mb = _tiny(3)
    lam = torch.tensor(0.5, device=DEV)

    def loss_fun(p, e, y):
        ce = losses.cross_entropy(p, y)
        aux = e["obj_desc"].float().square().mean()
        return {"loss_ce": ce, "aux": aux, "loss": ce + lam * aux}

    x, y = P.frames(2, 4, 64).cuda(), P.labels(2).cuda()
    a = optim.GuardedClipAdamW(ma, lr=1e-3, weight_decay=0.05, clip_grad_l2norm=1.0)
    b = optim.GuardedClipAdamW(mb, lr=1e-3, weight_decay=0.05, clip_grad_l2norm=1.0)
    meter = meters.TrainMeter(7, cfg)
    step_a = GraphedTrainStep(ma, loss_fun, [x], y, optimizer=a, meter=meter)
    step_b = GraphedTrainStep(mb, loss_fun, [x], y, optimizer=b)
    torch.cuda.synchronize()
    assert meter.state.tolist() == [0, 0] and meter._host == [] and meter.names == ["loss_ce", "aux", "loss"]
    assert [k for k, _ in step_a.segments] == [k for k, _ in step_b.segments]
    assert torch.equal(ma.flat.data, mb.flat.data)
    xs = [x * (1.0 - 0.03 * i) for i in range(7)]
    lrs = [optim.get_lr_at_epoch(cfg, i / 7.0)["lr"] for i in range(7)]
    got = []
    with _NoSync(meter):
        for i in range(7):
            optim.set_lr(a, lrs[i])
            step_a([xs[i]], y)
            got.append(numbers(meter.log_iter_stats(0, i)))
        got.append(numbers(meter.log_epoch_stats(0)))
    host = meters.MultiLossMeter(3)
    want = []
    for i in range(7):
        optim.set_lr(b, lrs[i])
        step_b([xs[i]], y)
        host.add_value({k: float(v) for k, v in step_b.loss_dict.items()})
        line = None
        if (i + 1) % 3 == 0:
            line = {"_type": "train_iter", "epoch": "1/50", "iter": "%d/7" % (i + 1), "lr": lrs[i]}
            line.update({k: float(v) for k, v in host.get_win_median().items()})
        want.append(line)
    line = {"_type": "train_epoch", "epoch": "1/50", "lr": lrs[6]}
    line.update(host.get_global_avg())
    want.append(line)
    assert got == want
    assert len({w["loss"] for w in want if w}) == 3                  # the numbers move from line to line
    assert meter.num_samples == 14 and meter.state.tolist() == [7, 0]
    torch.cuda.synchronize()
    assert torch.equal(ma.flat.data, mb.flat.data)
    assert a.stats()["applied"] == b.stats()["applied"] == 7


def test_poisoned_step_is_named_at_the_period():
    """the device of test_tail_inside_the_replayed_step: a NaN loss in replay 4 raises at the read of iteration 5"""
    from svit_amd import losses, meters, optim
    from svit_amd.graph import GraphedTrainStep
    cfg, model = _tiny(3)
    poison = torch.ones(1, device=DEV)

    def loss_fun(p, e, y):
        return losses.cross_entropy(p, y) * poison

    x, y = P.frames(2, 4, 64).cuda(), P.labels(2).cuda()
    opt = optim.GuardedClipAdamW(model, lr=1e-3, weight_decay=0.05, clip_grad_l2norm=1.0)
    meter = meters.TrainMeter(9, cfg)
    step = GraphedTrainStep(model, loss_fun, [x], y, optimizer=opt, meter=meter)
    assert meter.names == ["loss"]
    for i in range(3):
        step([x], y)
        line = meter.log_iter_stats(0, i)
    assert line["iter"] == "3/9" and line["loss"] > 0
    for i in range(3, 6):
        poison.fill_(float("nan") if i == 4 else 1.0)
        step([x], y)
        if i < 5:
            assert meter.log_iter_stats(0, i) is None
    with pytest.raises(RuntimeError, match=r"Got NaN losses.*first at iteration 4 "):
        meter.log_iter_stats(0, 5)
    assert opt.stats()["skipped"] == 1


class _Recording:
    """the model, keeping what it returned (on the device) for the test's own arithmetic"""

    def __init__(self, model):
        self.model, self.seen = model, []

    def eval(self):
        self.model.eval()

    def __call__(self, inputs, meta):
        preds, extra = self.model(inputs, meta)
        self.seen.append(preds.detach().clone())
        return preds, extra


def test_eval_epoch_five_batches_the_last_one_short():
    from svit_amd import losses, meters, train
    cfg, model, _, _ = S.build_hip_model(4, 64, train=False)
    cfg.LOG_PERIOD = 2
    cfg.TRAIN.FORWARD_VIDEO_FRAMES = False
    x = P.frames(2, 4, 64).cuda()
    sizes = [2, 2, 2, 2, 1]
    g = torch.Generator().manual_seed(3)
    loader = [([(x * (1.0 - 0.1 * i))[:n].contiguous()], torch.randint(0, 174, (n,), generator=g).cuda(), None, {})
              for i, n in enumerate(sizes)]
    rec = _Recording(model)
    with torch.no_grad():                                            # the label of one clip per batch: its best class
        for i, (inp, lab, _, _) in enumerate(loader):
            top = model(inp, {})[0].topk(5, dim=1).indices
            lab[0] = top[0, 0] if i % 2 else top[0, 3]
    meter = meters.ValMeter(len(loader), cfg)
    lines = []
    log_iter = meter.log_iter_stats
    meter.log_iter_stats = lambda e, i: lines.append(numbers(log_iter(e, i)))
    with _NoSync(meter):                                             # no host read between the periods
        epoch = numbers(train.eval_epoch(loader, rec, meter, 0, cfg))
    assert [l is not None for l in lines] == [False, True, False, True, False]
    # the reference's arithmetic (tools/train_net.py:322-354, meters.py:628-641, 679-707) on the CPU copy of the logits
    top1s, top5s, ces, mis1, mis5, num = [], [], [], 0, 0, 0
    for (inp, lab, _, _), preds in zip(loader, rec.seen):
        preds, lab = preds.cpu(), lab.cpu()
        c1, c5 = [torch.tensor(c) for c in topk_counts(preds, lab, (1, 5))]
        e1, e5 = [((1.0 - c / preds.size(0)) * 100.0).item() for c in (c1, c5)]
        top1s.append(e1)
        top5s.append(e5)
        mis1 += e1 * preds.size(0)
        mis5 += e5 * preds.size(0)
        num += preds.size(0)
        ces.append(float(losses.cross_entropy(preds.cuda(), lab.cuda())))
    assert len({round(e) for e in top1s}) > 1 and top5s != top1s
    assert lines[3]["top1_err"] == float(np.median(top1s[2:4])) and lines[3]["top5_err"] == float(np.median(top5s[2:4]))
    assert lines[1]["iter"] == "2/5" and lines[1]["top1_err"] == float(np.median(top1s[:2]))
    assert epoch["top1_err"] == mis1 / num and epoch["top5_err"] == mis5 / num and num == 9
    assert epoch["min_top1_err"] == min(100.0, mis1 / num) and "bad_labels" not in epoch
    # the extra losses: the same fused cross entropy on the same logits, read per batch and averaged as the host meter does
    assert epoch["extra_meter_loss_ce"] == sum(ces) / 5 and epoch["extra_meter_loss"] == sum(ces) / 5
    assert lines[3]["extra_meter_loss_ce"] == float(np.median(ces[2:4]))
    assert meter.state.tolist() == [0, 0] and meter.num_samples == 0          # eval_epoch ends with reset()


def test_train_epoch_replayed_and_eager():
    """train.train_epoch over five batches at LOG_PERIOD 2.  Replayed step: the epoch line equals a twin step whose
    losses are read with float() after every replay, under the same lr schedule, with no host read between the periods.
    Eager step: the same loop around model / loss / backward / optimizer.step(); its first line is the first replay's
    loss within test_graph_gpu's bar for one step (1e-4 relative)."""
    from svit_amd import losses, meters, optim, train
    from svit_amd.graph import GraphedTrainStep
    cfg, ma = _tiny(2)
    _, mb = _tiny(2)
    fn, wl = losses.VideoImageLoss(cfg), losses.get_lambdas_dict(cfg)

    def loss_fun(p, e, y):
        d = fn(p, e, y, {})
        d["loss"] = sum(wl[k] * d[k] for k in d)
        return d

    x, y = P.frames(2, 4, 64).cuda(), P.labels(2).cuda()
    loader = [([x * (1.0 - 0.05 * i)], (y + i) % 174, None, {}) for i in range(5)]
    a = optim.GuardedClipAdamW(ma, lr=1e-3, weight_decay=0.05, clip_grad_l2norm=1.0)
    b = optim.GuardedClipAdamW(mb, lr=1e-3, weight_decay=0.05, clip_grad_l2norm=1.0)
    meter = meters.TrainMeter(len(loader), cfg)
    step_a = GraphedTrainStep(ma, loss_fun, [x], y, optimizer=a, meter=meter)
    step_b = GraphedTrainStep(mb, loss_fun, [x], y, optimizer=b)
    with pytest.raises(ValueError, match="meter="):
        train.train_epoch(loader, step_b, b, meter, 0, cfg)
    with _NoSync(meter):
        epoch = numbers(train.train_epoch(loader, step_a, a, meter, 0, cfg))
    host, lrs, seen = meters.MultiLossMeter(2), [], []
    for i, (inp, lab, _, _) in enumerate(loader):
        lrs.append(optim.get_lr_at_epoch(cfg, i / 5.0)["lr"])
        optim.set_lr(b, lrs[-1])
        step_b(inp, lab)
        host.add_value({k: float(v) for k, v in step_b.loss_dict.items()})
        seen.append(float(step_b.loss_dict["loss"]))
    want = {"_type": "train_epoch", "epoch": "1/50", "lr": lrs[-1]}
    want.update(host.get_global_avg())
    assert epoch == want and set(epoch) >= {"loss_ce", "loss"} and len(set(lrs)) == 5
    torch.cuda.synchronize()
    assert torch.equal(ma.flat.data, mb.flat.data) and a.stats()["applied"] == 5
    assert meter.state.tolist() == [0, 0] and meter.num_samples == 0             # train_epoch ends with reset()
    # the eager loop
    cfg1, mc = _tiny(1)
    c = optim.FusedClipAdamW(mc, lr=1e-3, weight_decay=0.05, clip_grad_l2norm=1.0)
    meter_c = meters.TrainMeter(len(loader), cfg1)
    lines = []
    log_iter = meter_c.log_iter_stats
    meter_c.log_iter_stats = lambda e, i: lines.append(log_iter(e, i))
    epoch_c = train.train_epoch(loader, mc, c, meter_c, 0, cfg1)
    assert [l["iter"] for l in lines] == ["%d/5" % (i + 1) for i in range(5)]
    assert meter_c.names == ["loss_ce", "loss"] and lines[0]["loss"] == lines[0]["loss_ce"]
    assert abs(lines[0]["loss"] - seen[0]) < 1e-4 * max(1.0, abs(seen[0])), (lines[0]["loss"], seen[0])
    assert c.step_count == 5 and epoch_c["lr"] == lrs[-1] and np.isfinite(epoch_c["loss"])


# ------------------------------------------------------------------------------------------------ data parallel
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _rank_values(rank, iters):
    g = torch.Generator().manual_seed(100 + rank)
    keys = ["loss_ce", "loss"] if rank == 0 else ["boxes_l1_loss", "loss_contact_state", "loss"]
    vals = torch.rand(iters, len(keys), generator=g) + 0.25
    n = 3 + rank
    logits = [torch.stack([torch.randperm(174, generator=g) for _ in range(n)]).float() / 7.0 for _ in range(iters)]
    labels = [torch.randint(0, 174, (n,), generator=g) for _ in range(iters)]
    for i in range(iters):
        labels[i][0] = int(logits[i][0].argmax()) if (i + rank) % 2 else int(logits[i][0].topk(3).indices[2])
    extra = torch.rand(iters, 1, generator=g) + 0.5
    return keys, vals, logits, labels, extra


def _dp_worker(rank, world, port, out, backend, force):
    import torch.distributed as dist
    sys.path.insert(0, ROOT)
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    torch.cuda.set_device(0)
    if backend == "nccl":
        dist.init_process_group("nccl", rank=rank, world_size=world, device_id=torch.device("cuda", 0))
    else:
        dist.init_process_group("gloo", rank=rank, world_size=world)
    from svit_amd import config, meters
    cfg = config.ssv2_cfg(4, 64)
    cfg.LOG_PERIOD = 3
    iters = 7
    keys, vals, logits, labels, extra = _rank_values(rank, iters)
    res = {}
    for arm in (["plain", "forced"] if force else ["merged"]):
        tm = meters.TrainMeter(iters, cfg, force_collectives=arm == "forced")
        vm = meters.ValMeter(iters, cfg, force_collectives=arm == "forced")
        if arm == "plain":
            tm._collective = vm._collective = lambda: False
        lines = []
        for i in range(iters):
            tm.update_stats(1e-3 * (i + 1), 2 * world, dloss={k: vals[i, j].cuda() for j, k in enumerate(keys)})
            vm.update_stats(logits[i].cuda(), labels[i].cuda(), 7, extra_metrices={"loss": extra[i, 0].cuda()})
            lines.append((numbers(tm.log_iter_stats(0, i)), numbers(vm.log_iter_stats(0, i))))
        lines.append((numbers(tm.log_epoch_stats(0)), numbers(vm.log_epoch_stats(0))))
        if arm == "forced":
            assert tm._rank_names == [keys] and "nccl" in str(dist.get_backend())
        res[arm] = lines
    torch.save(res, out % rank)
    dist.barrier()
    dist.destroy_process_group()


def _spawn(world, out, backend, force):
    import torch.multiprocessing as mp
    port = _free_port()
    ctx = mp.get_context("spawn")
    procs = [ctx.Process(target=_dp_worker, args=(r, world, port, out, backend, force)) for r in range(world)]
    for p in procs:
        p.start()
    for p in procs:
        p.join(300)
    assert all(p.exitcode == 0 for p in procs), [p.exitcode for p in procs]
    return [torch.load(out % r) for r in range(world)]


def test_two_ranks_on_one_gpu_over_gloo(tmp_path):
    """the merged lines equal the formulas on the two ranks' values: training tools/train_net.py:153-161 (Python double
    sum(v) / len(v) over the ranks that have the key), validation du.all_reduce (fp32 sum, times fp32 1 / world)"""
    from svit_amd import meters
    got = _spawn(2, str(tmp_path / "r%d.pt"), "gloo", False)
    assert got[0]["merged"] == got[1]["merged"]
    iters, f = 7, np.float32
    ranks = [_rank_values(r, iters) for r in range(2)]
    host = meters.MultiLossMeter(3)
    top1, top5, ex = meters.ScalarMeter(3), meters.ScalarMeter(3), meters.ScalarMeter(3)
    mis1 = mis5 = num = 0
    want = []
    for i in range(iters):
        merged = {}
        for keys, vals, _, _, _ in ranks:
            for j, k in enumerate(keys):
                merged.setdefault(k, []).append(vals[i, j].item())
        host.add_value({k: sum(v) / len(v) for k, v in merged.items()})
        errs = []
        for k in (1, 5):
            per = [f(f(1) - f(topk_counts(lg[i], lb[i], (k,))[0]) / f(lg[i].shape[0])) * f(100)
                   for _, _, lg, lb, _ in ranks]
            errs.append(float(f(f(per[0] + per[1]) * f(0.5))))
        top1.add_value(errs[0])
        top5.add_value(errs[1])
        ex.add_value(float(f(f(f(ranks[0][4][i, 0].item()) + f(ranks[1][4][i, 0].item())) * f(0.5))))
        mis1 += errs[0] * 7
        mis5 += errs[1] * 7
        num += 7
        if (i + 1) % 3:
            want.append((None, None))
            continue
        t = {"_type": "train_iter", "epoch": "1/50", "iter": "%d/7" % (i + 1), "lr": 1e-3 * (i + 1)}
        t.update({k: float(v) for k, v in host.get_win_median().items()})
        v = {"_type": "val_iter", "epoch": "1/50", "iter": "%d/7" % (i + 1), "top1_err": float(top1.get_win_median()),
             "top5_err": float(top5.get_win_median()), "extra_meter_loss": float(ex.get_win_median())}
        want.append((t, v))
    t = {"_type": "train_epoch", "epoch": "1/50", "lr": 1e-3 * iters}
    t.update(host.get_global_avg())
    v = {"_type": "val_epoch", "epoch": "1/50", "top1_err": mis1 / num, "top5_err": mis5 / num,
         "min_top1_err": min(100.0, mis1 / num), "min_top5_err": min(100.0, mis5 / num),
         "extra_meter_loss": ex.get_global_avg()}
    want.append((t, v))
    assert got[0]["merged"] == want
    assert set(want[2][0]) >= {"loss_ce", "boxes_l1_loss", "loss_contact_state", "loss"}


def test_one_rank_forced_collectives_equal_the_plain_run(tmp_path):
    """force_collectives=True on a one-rank RCCL group: the device-tensor all_gather runs and changes nothing"""
    got = _spawn(1, str(tmp_path / "f%d.pt"), "nccl", True)[0]
    assert got["forced"] == got["plain"] and got["plain"][2][0] is not None
