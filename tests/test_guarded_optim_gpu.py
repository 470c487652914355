"""The guarded optimizer tail on the GPU (optim.GuardedClipAdamW; svit_step_guard + svit_adamw_step_guarded): bit parity
with the classic kernels, a dropped step that leaves every buffer as it was, clip by value, the read-outs, the tail
inside the captured step (graph.GraphedTrainStep(optimizer=...)), checkpoints, and its place behind the last all-reduce
of a data-parallel step.  Needs a real MI355X."""
import os
import socket
import sys
import types

import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import procedural as P
from tests import smoke_impl as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda"
# n % 4 == 3: a scalar tail of three; the boundary between the two weight-decay groups is inside a 16-byte vector
N, N_DECAY = 4099, 2050


class _Flat:
    """what the optimizers touch of a model's FlatParams: flat fp32 buffers on the device"""

    def __init__(self, p):
        self.total, self.n_decay = p.numel(), N_DECAY
        self.data = p.clone()
        self.grad = torch.zeros_like(p)


def _rand(name, amp):
    return P.tensor("guard:" + name, (N,), amp).to(DEV)


def _pair(clip, clip_value=None, classic_clip="same", **kw):
    """(guarded, classic) over equal weights; lr and weight decay differ between the two groups"""
    from svit_amd import optim
    p0 = _rand("p", 0.1)
    a = optim.GuardedClipAdamW(types.SimpleNamespace(flat=_Flat(p0)), lr=1e-3, weight_decay=0.05,
                               clip_grad_l2norm=clip, clip_grad_value=clip_value, **kw)
    b = optim.FusedClipAdamW(types.SimpleNamespace(flat=_Flat(p0)), lr=1e-3, weight_decay=0.05,
                             clip_grad_l2norm=clip if classic_clip == "same" else classic_clip)
    for o in (a, b):
        o.param_groups[1]["lr"] = 3e-3
        o.param_groups[1]["weight_decay"] = 0.01
    return a, b


def _state(o):
    return o.flat.data.clone(), o.exp_avg.clone(), o.exp_avg_sq.clone()


def _assert_same(a, b, what):
    for name, x, y in zip(("p", "exp_avg", "exp_avg_sq"), _state(a), _state(b) if not isinstance(b, tuple) else b):
        assert torch.equal(x, y), (what, name, int((x != y).sum()), float((x - y).abs().max()))


def _both_step(a, b, g, what, classic_g=None):
    a.flat.grad.copy_(g)
    b.flat.grad.copy_(g if classic_g is None else classic_g)
    a.step()
    b.step()
    _assert_same(a, b, what)


@pytest.mark.parametrize("clip", [1.0, None])
def test_parity_with_the_classic_kernels(clip):
    """steps 1-3, then four steps from applied = 17 319: across the end of the (0.9, 0.999) bias table (17 321 pairs)"""
    a, b = _pair(clip)
    assert a.bias_table.shape == (17321, 2)
    for k in range(3):
        _both_step(a, b, _rand("g%d" % k, 1.0), "step %d" % (k + 1))
    s = a.stats()
    assert s["applied"] == 3 and s["skipped"] == 0 and b.step_count == 3
    if clip:
        assert 0.0 < s["clip_coef"] < 0.1          # |g| ~ 37 against max_norm 1: the clip is active
    else:
        assert s["clip_coef"] == 1.0
    a.step_count = 17319
    b.step_count = 17319
    for k in range(4):
        _both_step(a, b, _rand("h%d" % k, 1.0), "step %d" % (17320 + k))
    assert a.step_count == 17323 and b.step_count == 17323


@pytest.mark.parametrize("bad,index", [(float("inf"), N - 1), (float("nan"), 0)])
def test_non_finite_step_is_dropped(bad, index):
    a, b = _pair(1.0)
    for k in range(2):
        _both_step(a, b, _rand("g%d" % k, 1.0), "step %d" % (k + 1))
    before, s0 = _state(a), a.stats()
    g = _rand("gbad", 1.0)
    g[index] = bad
    a.flat.grad.copy_(g)
    a.step()
    _assert_same(a, before, "dropped step")
    s1 = a.stats()
    assert s1["applied"] == s0["applied"] == 2 and a.step_count == 2
    assert s1["skipped"] == s0["skipped"] + 1 == 1
    assert s1["consecutive_skipped"] == s0["consecutive_skipped"] + 1 == 1
    assert s1["grad_norm"] == s0["grad_norm"] and s1["clip_coef"] == s0["clip_coef"]      # nothing else changed
    # the next finite step is the classic kernel's step applied + 1 (b.step() counts 2 -> 3)
    _both_step(a, b, _rand("g2", 1.0), "step after the dropped one")
    s2 = a.stats()
    assert s2["applied"] == 3 and s2["skipped"] == 1 and s2["consecutive_skipped"] == 0 and b.step_count == 3


def test_clip_by_value():
    """clip_value = 0.01 on gradients of scale 0.05 == the classic kernel fed g.clamp(-0.01, 0.01), norm clipping off
    (the norm bound the guarded optimizer was also given is ignored: value before norm, as in the reference)"""
    a, b = _pair(1.0, clip_value=0.01, classic_clip=None)
    for k in range(3):
        g = _rand("v%d" % k, 0.05)
        assert float((g.abs() > 0.01).float().mean()) > 0.3 and float((g.abs() < 0.01).float().mean()) > 0.05
        _both_step(a, b, g, "value-clipped step %d" % (k + 1), classic_g=g.clamp(-0.01, 0.01))
    assert a.stats()["clip_coef"] == 1.0 and a.stats()["applied"] == 3


def test_read_outs_and_no_sync_in_step():
    a, b = _pair(1.0, max_consecutive_skips=2)
    g = _rand("g0", 1.0)
    _both_step(a, b, g, "step 1")
    norm = float(g.double().norm())
    s = a.stats()
    assert set(s) == {"applied", "skipped", "consecutive_skipped", "grad_norm", "clip_coef"}
    assert (s["applied"], s["skipped"], s["consecutive_skipped"]) == (1, 0, 0)
    assert abs(s["grad_norm"] - norm) < 1e-5 * norm and a.grad_norm() == s["grad_norm"]
    assert abs(s["clip_coef"] - 1.0 / (norm + 1e-6)) < 1e-5 / norm
    assert abs(a.grad_norm() - b.grad_norm()) < 1e-6 * norm      # the classic optimizer's read-out of the same step
    bad = g.clone()
    bad[7] = float("nan")
    a.flat.grad.copy_(bad)
    a.step()
    a.check()                                      # one dropped step: below the limit
    a.step()
    assert a.stats()["consecutive_skipped"] == 2 and a.stats()["skipped"] == 2 and a.stats()["applied"] == 1
    with pytest.raises(RuntimeError, match="dropped"):
        a.check()
    assert a.stats()["grad_norm"] == s["grad_norm"]          # still the last FINITE norm
    a.flat.grad.copy_(g)
    a.step()
    a.check()                                      # an applied step resets the run
    # step() never waits for the device: more steps than the upload ring has slots, under sync-debug "error"
    torch.cuda.synchronize()
    mode = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        for _ in range(a.RING + 2):
            a.step()
    finally:
        torch.cuda.set_sync_debug_mode(mode)
    assert a.stats()["applied"] == 2 + a.RING + 2


# ---------------------------------------------------------------------------------------- model level
def _tiny(reproducible=True):
    cfg, model, _, _ = S.build_hip_model(4, 64)
    model.engine.reproducible = reproducible
    return cfg, model


def test_tail_inside_the_replayed_step():
    """arm A: GraphedTrainStep(optimizer=guarded); arm B: GraphedTrainStep + the classic eager opt.step().  Four steps
    down the cosine schedule (a different lr every step: the uploaded lr reaches the replay), one poisoned step that
    moves nothing, one more clean step."""
    from svit_amd import losses, optim
    from svit_amd.graph import GraphedTrainStep
    cfg, ma = _tiny()
    _, mb = _tiny()
    assert torch.equal(ma.flat.data, mb.flat.data)
    w_init = ma.flat.data.clone()
    poison = torch.ones(1, device=DEV)

    def loss_fun(p, e, y):
        return losses.cross_entropy(p, y) * poison

    x, y = P.frames(2, 4, 64).cuda(), P.labels(2).cuda()
    a = optim.GuardedClipAdamW(ma, lr=1e-3, weight_decay=0.05, clip_grad_l2norm=1.0)
    b = optim.FusedClipAdamW(mb, lr=1e-3, weight_decay=0.05, clip_grad_l2norm=1.0)
    step_a = GraphedTrainStep(ma, loss_fun, [x], y, optimizer=a)
    step_b = GraphedTrainStep(mb, loss_fun, [x], y)
    torch.cuda.synchronize()
    assert torch.equal(ma.flat.data, mb.flat.data) and a.stats()["applied"] == 0       # building the step moved nothing
    assert [k for k, _ in step_a.segments] == [k for k, _ in step_b.segments]           # no data parallelism: no new cut
    with pytest.raises(Exception, match="GuardedClipAdamW"):
        GraphedTrainStep(mb, loss_fun, [x], y, optimizer=b)
    lrs = [optim.get_lr_at_epoch(cfg, 0.5 * i)["lr"] for i in range(5)]
    assert len(set(lrs)) == 5

    def clean(i):
        optim.set_lr(a, lrs[i])
        optim.set_lr(b, lrs[i])
        la, _ = step_a([x], y)
        lb, _ = step_b([x], y)
        b.step()
        torch.cuda.synchronize()
        assert float(la) == float(lb)
        _assert_same(a, b, "replayed step %d" % (i + 1))

    for i in range(4):
        clean(i)
    assert a.stats()["applied"] == 4 and not torch.equal(ma.flat.data, w_init)
    before = _state(a)
    poison.fill_(float("nan"))
    la, _ = step_a([x], y)
    torch.cuda.synchronize()
    assert la.isnan().all()
    _assert_same(a, before, "poisoned replay")
    s = a.stats()
    assert (s["applied"], s["skipped"], s["consecutive_skipped"]) == (4, 1, 1)
    poison.fill_(1.0)
    clean(4)
    s = a.stats()
    assert (s["applied"], s["skipped"], s["consecutive_skipped"]) == (5, 1, 0) and b.step_count == 5


def test_checkpoint_round_trip():
    """state_dict() after 3 applied + 1 dropped steps says step == 3 and loads into a guarded and a classic optimizer"""
    from svit_amd import optim
    _, model = _tiny()
    flat = model.flat
    kw = dict(lr=1e-3, weight_decay=0.05, clip_grad_l2norm=1.0)
    a = optim.GuardedClipAdamW(model, **kw)

    # the flat buffer pads every parameter to an aligned size; the padding never receives a gradient in training and
    # is no part of a checkpoint, so the synthetic gradients leave it zero as well
    live = torch.zeros(flat.total, device=DEV)
    for off, numel, _ in flat.slots.values():
        live[off:off + numel] = 1.0
    first = min(off for off, _, _ in flat.slots.values())

    def grad(k, poison=False):
        g = P.tensor("guard:ck%d" % k, (flat.total,), 1e-2).to(DEV) * live
        if poison:
            g[first] = float("inf")
        flat.grad.copy_(g)

    for k, poison in enumerate((False, False, True, False)):
        grad(k, poison)
        a.step()
    s = a.stats()
    assert (s["applied"], s["skipped"]) == (3, 1)
    sd = a.state_dict()
    n_params = len(list(model.named_parameters()))
    assert len(sd["state"]) == n_params and all(float(e["step"]) == 3.0 for e in sd["state"].values())
    assert "skipped" not in sd and all(set(e) == {"step", "exp_avg", "exp_avg_sq"} for e in sd["state"].values())
    w0 = flat.data.clone()
    outs = []
    for cls in (optim.GuardedClipAdamW, optim.FusedClipAdamW):
        flat.data.copy_(w0)
        o = cls(model, **kw)
        o.load_state_dict(sd)
        assert o.step_count == 3
        assert torch.equal(o.exp_avg, a.exp_avg) and torch.equal(o.exp_avg_sq, a.exp_avg_sq)
        grad(9)
        o.step()
        torch.cuda.synchronize()
        assert o.step_count == 4
        outs.append(_state(o))
    for name, u, v in zip(("p", "exp_avg", "exp_avg_sq"), *outs):
        assert torch.equal(u, v), (name, int((u != v).sum()))
    assert not torch.equal(outs[0][0], w0)
    assert optim.GuardedClipAdamW(model, **kw).stats()["skipped"] == 0      # the dropped-step counters are not checkpointed


# ------------------------------------------------------------------------------------- data parallel
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _dp_worker(port, out):
    """one rank on the RCCL group, set up as tests/test_dp_gpu.py::test_rccl_production_branch_with_one_rank does: three
    replayed guarded steps without and with DataParallel(force_collectives=True)"""
    import torch.distributed as dist
    sys.path.insert(0, ROOT)
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    torch.cuda.set_device(0)
    dist.init_process_group("nccl", rank=0, world_size=1, device_id=torch.device("cuda", 0))
    from oracle import svit_ref as R
    from svit_amd import config, optim
    from svit_amd.dp import DataParallel
    from svit_amd.graph import GraphedTrainStep
    from svit_amd.model import MODEL_REGISTRY
    x, y = P.frames(2, 4, 64).cuda(), P.labels(2).cuda()
    sd = P.state_dict(R.param_shapes(R.make_spec(4, 64, drop_path_rate=0.0, dropout_rate=0.0)))
    res = {}
    for arm in ("plain", "dp"):
        cfg = config.ssv2_cfg(num_frames=4, crop=64, num_gpus=1)
        cfg.MVIT.DROPPATH_RATE = 0.0
        cfg.MODEL.DROPOUT_RATE = 0.0
        model = MODEL_REGISTRY.get("SViT")(cfg).cuda()
        model.load_state_dict(sd)
        # bit-equality across a different cut of the step: every reduction that meets in fp32 atomics runs unsplit
        model.engine.deterministic = True
        dp = DataParallel(model, bucket_ranks=4, force_collectives=True) if arm == "dp" else model
        opt = optim.GuardedClipAdamW(dp, lr=1e-3, weight_decay=0.05, clip_grad_l2norm=1.0)
        step = GraphedTrainStep(dp, lambda p, e, l: torch.nn.functional.cross_entropy(p, l), [x], y, optimizer=opt)
        kinds = [k for k, _ in step.segments]
        if arm == "dp":
            assert dp.force_collectives and dist.get_backend() == "nccl"
            assert kinds.count("ready") == len(dp.launch_ranks())
            # the tail is the one segment behind the final bucket's all-reduce (whose _on_ready ends in finish())
            assert kinds[-2:] == ["ready", "graph"], kinds
            assert step.segments[-2][1][-1] == model.flat.n_ranks - 1
        else:
            assert "ready" not in kinds
        for i in range(3):
            optim.set_lr(opt, 1e-3 * (i + 1))
            step([x], y)
        torch.cuda.synchronize()
        if arm == "dp":
            assert not dp._works
        res[arm] = {"p": model.flat.data.cpu(), "m": opt.exp_avg.cpu(), "v": opt.exp_avg_sq.cpu(), "stats": opt.stats()}
    torch.save(res, out)
    dist.barrier()
    dist.destroy_process_group()


def test_tail_runs_behind_the_last_all_reduce(tmp_path):
    import torch.multiprocessing as mp
    out = str(tmp_path / "dp.pt")
    proc = mp.get_context("spawn").Process(target=_dp_worker, args=(_free_port(), out))
    proc.start()
    proc.join(600)
    assert proc.exitcode == 0, proc.exitcode
    res = torch.load(out)
    assert res["plain"]["stats"]["applied"] == res["dp"]["stats"]["applied"] == 3
    assert res["plain"]["stats"]["skipped"] == res["dp"]["stats"]["skipped"] == 0
    for k in ("p", "m", "v"):
        assert torch.equal(res["plain"][k], res["dp"][k]), (k, float((res["plain"][k] - res["dp"][k]).abs().max()))
    assert res["plain"]["stats"] == res["dp"]["stats"]
