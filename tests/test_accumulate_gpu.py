"""Virtual ranks on the GPU: k recipe ranks run one after another into the one flat gradient buffer, one exchange, one
guarded optimizer step (graph.AccumulatedTrainStep, its eager twin train.accumulate_step).

The tiny configuration of the data-parallel tests: a 4-frame model at 64^2, video micro-batches of 2 clips with cross
entropy, image micro-batches of 3 stills with the HAOG losses, inputs from oracle.procedural, drop rates 0 unless
stated.  Every value comparison is bit equality: fp32 addition of two numbers is commutative, doubling and halving are
exact, and `engine.deterministic` / `engine.reproducible` make every gradient a pure function of the batch."""
import os
import socket
import sys
import types

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

pytestmark = pytest.mark.gpu

from oracle import procedural as P
from oracle import svit_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FORMS = ["eager", "graphed"]
LR = 1e-3


# ------------------------------------------------------------------------------------------------ helpers ----
def build(droppath=0.0, mode=None, num_gpus=1):
    """the tiny model with the procedural weights, in train mode; mode: "deterministic" | "reproducible" | None"""
    from svit_amd import config
    from svit_amd.model import MODEL_REGISTRY
    cfg = config.ssv2_cfg(num_frames=4, crop=64, num_gpus=num_gpus)
    cfg.MVIT.DROPPATH_RATE = droppath
    cfg.MODEL.DROPOUT_RATE = 0.0
    cfg.IMAGE_TRAIN.GPU_IDS, cfg.IMAGE_TRAIN.BATCH_SIZE, cfg.TRAIN.BATCH_SIZE = [1], 3, 2
    model = MODEL_REGISTRY.get("SViT")(cfg).cuda()
    model.load_state_dict(P.state_dict(R.param_shapes(R.make_spec(4, 64, drop_path_rate=droppath, dropout_rate=0.0))))
    model.train()
    if mode is not None:
        setattr(model.engine, mode, True)
    return cfg, model


def optimizer_for(model, **kw):
    from svit_amd import optim
    return optim.GuardedClipAdamW(model, lr=LR, weight_decay=0.05, clip_grad_l2norm=1.0, **kw)


def video(tag=""):
    return [P.frames(2, 4, 64, tag="clip" + tag).cuda()], P.labels(2, tag="label" + tag).cuda()


def image(tag=""):
    return [P.frames(3, 1, 64, tag="clip" + tag).cuda()], {k: v.cuda() for k, v in P.haog_meta(3, tag="haog" + tag).items()}


def is_image(batch):
    return isinstance(batch[1], dict)


def loss_of(cfg, image_rank, seen=None):
    """loss_fun(preds, extra, labels) -> the dict the loop logs, "loss" = the weighted total (train_net.py:124);
    seen: a list that collects every dict returned (the eager twin's read-back)"""
    from svit_amd import losses
    fn = losses.VideoImageLoss(cfg, is_video_rank=not image_rank)

    def loss_fun(preds, extra, labels):
        d = fn(preds, extra, labels, labels)
        d["loss"] = fn.total(d)
        if seen is not None:
            seen.append({k: v.detach().clone() for k, v in d.items()})
        return d
    return loss_fun


def single_grad(cfg, model, batch):
    """one eager step over a zeroed buffer -> flat.grad (a copy)"""
    model.flat.grad.zero_()
    preds, extra = model(batch[0], {})
    loss_of(cfg, is_image(batch))(preds, extra, batch[1])["loss"].backward()
    torch.cuda.synchronize()
    return model.flat.grad.clone()


class Rig:
    """one accumulated step in either form over `batches` (their shapes and roles fix the micro-steps; equal roles share
    one capture)"""

    def __init__(self, form, cfg, model, opt, batches, meter=None, wrapper=None):
        from svit_amd.graph import AccumulatedTrainStep, GraphedTrainStep
        self.form, self.cfg, self.opt, self.meter = form, cfg, opt, meter
        self.model = model if wrapper is None else wrapper
        self.kinds = [is_image(b) for b in batches]
        self.step = None
        if form == "graphed":
            caps = {}
            for b, kind in zip(batches, self.kinds):
                if kind not in caps:
                    caps[kind] = GraphedTrainStep(self.model, loss_of(cfg, kind), b[0], b[1], accumulate=True)
            self.captures = caps
            self.step = AccumulatedTrainStep(self.model, [caps[kind] for kind in self.kinds], opt, meter=meter)

    def __call__(self, batches):
        """-> the k losses as host floats' bit patterns (a tensor of int32)"""
        from svit_amd import train
        if self.step is not None:
            losses = self.step(batches)
        else:
            losses = train.accumulate_step(self.model, [loss_of(self.cfg, kind) for kind in self.kinds], batches, self.opt,
                                           meter=self.meter)
        torch.cuda.synchronize()
        return torch.stack([l.detach().reshape(()) for l in losses]).cpu().view(torch.int32)


def snapshot(model, opt):
    rng = None if model._rng_state is None else model._rng_state.clone()
    return (model.flat.data.clone(), opt.exp_avg.clone(), opt.exp_avg_sq.clone(), opt.dev_rec.clone(), rng)


def restore(model, opt, snap):
    model.flat.data.copy_(snap[0])
    opt.exp_avg.copy_(snap[1])
    opt.exp_avg_sq.copy_(snap[2])
    opt.dev_rec.copy_(snap[3])
    if snap[4] is not None:
        model._rng_state.copy_(snap[4])


def state_bits(model, opt):
    torch.cuda.synchronize()
    return [t.clone().view(torch.int32) for t in (model.flat.grad, model.flat.data, opt.exp_avg, opt.exp_avg_sq)]


def assert_bits(got, want, what):
    for name, a, b in zip(("flat.grad", "weights", "exp_avg", "exp_avg_sq", "losses"), got, want):
        assert torch.equal(a, b), "%s: %s differs in %d elements" % (what, name, int((a != b).sum()))


def differing_names(model, got, want):
    """names of the parameters whose gradient slices differ bit for bit"""
    bad = []
    for name, _ in model.named_parameters():
        a, b = model.flat.view(got, name), model.flat.view(want, name)
        if not torch.equal(a.view(torch.int32), b.view(torch.int32)):
            bad.append(name)
    return bad


# ---------------------------------------------------------------------------------------- (a) additivity ----
@pytest.mark.parametrize("form", FORMS)
def test_a_accumulated_buffer_is_the_ordered_sum_and_the_tail_steps_on_it(form):
    from svit_amd import optim
    cfg, model = build(mode="deterministic")
    A, B, C = video(), video("B"), image()
    assert not torch.equal(A[0][0], B[0][0]) and not torch.equal(A[1], B[1])
    gA, gB, gC = (single_grad(cfg, model, b) for b in (A, B, C))
    assert float(gA.abs().max()) > 0 and float(gC.abs().max()) > 0 and not torch.equal(gA, gB)
    want = (gA + gB) + gC                                            # fp32, in recipe-rank order
    opt = optimizer_for(model)
    # the second model: the same initial weights and moments, its gradient SET to the sum, one guarded step at 1/3
    twin_flat = types.SimpleNamespace(total=model.flat.total, n_decay=model.flat.n_decay, data=model.flat.data.clone(),
                                      grad=want.clone())
    twin = optim.GuardedClipAdamW(types.SimpleNamespace(flat=twin_flat), lr=LR, weight_decay=0.05, clip_grad_l2norm=1.0,
                                  grad_scale=1.0 / 3)
    rig = Rig(form, cfg, model, opt, [A, B, C])
    rig([A, B, C])
    bad = differing_names(model, model.flat.grad, want)
    assert not bad, "gradients that are not ((gA + gB) + gC): %s" % bad
    assert torch.equal(model.flat.grad.view(torch.int32), want.view(torch.int32))
    twin.step()
    torch.cuda.synchronize()
    for name, a, b in (("weights", model.flat.data, twin_flat.data), ("exp_avg", opt.exp_avg, twin.exp_avg),
                       ("exp_avg_sq", opt.exp_avg_sq, twin.exp_avg_sq)):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32)), (name, int((a != b).sum()))
    s, t = opt.stats(), twin.stats()
    assert s["applied"] == 1 and s["skipped"] == 0 and opt.step_count == 1
    assert s["grad_norm"] == t["grad_norm"] and s["clip_coef"] == t["clip_coef"]
    assert opt.grad_scale == 1.0                                     # the 1/k lived in the step's record only


# -------------------------------------------------------------------------------- (b) no storing producer ----
@pytest.mark.parametrize("form", FORMS)
def test_b_every_gradient_producer_adds(form):
    """the same micro-batch twice: every one of the 405 named tensors must hold 2 * g_single (doubling is exact); a
    producer that stores over the buffer instead of adding leaves g_single and is named"""
    cfg, model = build(mode="deterministic")
    names = [n for n, _ in model.named_parameters()]
    assert len(names) == 405
    opt = optimizer_for(model)
    opt.param_groups[0]["lr"] = opt.param_groups[1]["lr"] = 0.0       # (the weights stay put between the two roles)
    for g in opt.param_groups:
        g["weight_decay"] = 0.0
    w0 = model.flat.data.clone()
    for batch in (video(), image()):
        single = single_grad(cfg, model, batch)
        live = [n for n in names if bool(model.flat.view(single, n).any())]
        assert len(live) > 200, len(live)         # the whole backbone and the role's heads
        Rig(form, cfg, model, opt, [batch, batch])([batch, batch])
        bad = differing_names(model, model.flat.grad, 2.0 * single)
        assert not bad, "%s micro-batch twice: gradients that are not 2 * g_single: %s" % (
            "image" if is_image(batch) else "video", bad)
        assert torch.equal(model.flat.data, w0)


# -------------------------------------------------------------------------------- (c) graphed equals eager ----
def test_c_graphed_equals_eager_and_replays():
    cfg, model = build(mode="reproducible")
    opt = optimizer_for(model)
    first = [video(), video("B"), image()]
    second = [video("C"), video(), image("B")]
    s0 = snapshot(model, opt)
    graphed = Rig("graphed", cfg, model, opt, first)
    assert len(graphed.captures) == 2 and graphed.step.micro_steps[0] is graphed.step.micro_steps[1]
    n_graphs = [c.n_graphs for c in graphed.captures.values()]

    def two_steps(rig):
        restore(model, opt, s0)
        out = []
        for batches in (first, second):
            losses = rig(batches)
            out.append(state_bits(model, opt) + [losses])
        return out
    g1 = two_steps(graphed)
    assert [c.n_graphs for c in graphed.captures.values()] == n_graphs          # replayed, not recaptured
    g2 = two_steps(graphed)
    e1 = two_steps(Rig("eager", cfg, model, opt, first))
    for i in range(2):
        assert_bits(g1[i], g2[i], "two graphed runs from the same state, step %d" % i)
        assert_bits(g1[i], e1[i], "graphed against eager, step %d" % i)
    assert not torch.equal(g1[0][4], g1[1][4]) and not torch.equal(g1[0][1], g1[1][1])
    assert len(set(g1[0][4].tolist())) == 3                                      # three different micro-step losses
    assert opt.stats()["applied"] == 2


# ------------------------------------------------------------------------------ (d) against the real exchange ----
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _exchange_worker(rank, world, port, out, form):
    """world 2: the 2-rank job (rank 0 clips, rank 1 stills, DataParallel over gloo) -> what it leaves in flat.grad;
    world 1: one process, the two roles as k = 2 virtual ranks -> the accumulated buffer"""
    sys.path.insert(0, ROOT)
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    torch.cuda.set_device(0)
    if world > 1:
        dist.init_process_group("gloo", rank=rank, world_size=world)
    from svit_amd.dp import DataParallel, rank_role, virtual_roles
    cfg, model = build(mode="deterministic", num_gpus=2)
    batch_of = lambda role: image() if role.is_image else video()
    if world > 1:
        dp = DataParallel(model, bucket_ranks=4)
        role = rank_role(cfg, rank)
        x, lab = batch_of(role)
        assert x[0].shape[0] == role.batch_size == (3 if role.is_image else 2)
        if form == "graphed":
            from svit_amd.graph import GraphedTrainStep
            GraphedTrainStep(dp, loss_of(cfg, role.is_image), x, lab)(x, lab)
        else:
            preds, extra = dp(x, {})
            loss = loss_of(cfg, role.is_image)(preds, extra, lab)["loss"]
            model.zero_grad()
            loss.backward()
        torch.cuda.synchronize()
        g = model.flat.grad.detach().cpu().clone()
        both = [torch.zeros_like(g) for _ in range(world)]
        dist.all_gather(both, g)
        assert torch.equal(both[0], both[1])
    else:
        roles = virtual_roles(cfg, 1, 0)
        assert [r.is_image for r in roles] == [False, True]
        batches = [batch_of(r) for r in roles]
        Rig(form, cfg, model, optimizer_for(model), batches)(batches)
        g = model.flat.grad.detach().cpu().clone()
    if rank == 0:
        torch.save(g, out)
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()


def _spawn(target, world, out, *args):
    port = _free_port()
    ctx = mp.get_context("spawn")      # fresh children, started before this process touches a GPU
    procs = [ctx.Process(target=target, args=(r, world, port, out) + args) for r in range(world)]
    for p in procs:
        p.start()
    for p in procs:
        p.join(600)
    assert all(p.exitcode == 0 for p in procs), [p.exitcode for p in procs]
    return torch.load(out)


@pytest.mark.parametrize("form", FORMS)
def test_d_two_rank_exchange_is_half_the_accumulated_buffer(tmp_path, form):
    one = _spawn(_exchange_worker, 1, str(tmp_path / "k2.pt"), form)
    two = _spawn(_exchange_worker, 2, str(tmp_path / "w2.pt"), form)
    assert float(one.abs().max()) > 0
    want = 0.5 * one                                                  # halving is exact
    assert torch.equal(two.view(torch.int32), want.view(torch.int32)), (
        int((two != want).sum()), float((two - want).abs().max()))


# ------------------------------------------------------------------------------------ (e) DP plus accumulation ----
def _dp_worker(rank, world, port, out, form, wrapped):
    """k = 2 video micro-steps; wrapped: over DataParallel(force_collectives=True) on a one-rank RCCL group"""
    sys.path.insert(0, ROOT)
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    torch.cuda.set_device(0)
    cfg, model = build(mode="deterministic")
    wrapper, calls = None, []
    if wrapped:
        from svit_amd.dp import DataParallel
        dist.init_process_group("nccl", rank=0, world_size=1, device_id=torch.device("cuda", 0))
        wrapper = DataParallel(model, bucket_ranks=4, force_collectives=True)
        reduce_slice = wrapper._reduce_slice
        wrapper._reduce_slice = lambda a, b: (calls.append((a, b)), reduce_slice(a, b))[1]
    batches = [video(), video("B")]
    plain = 0
    if wrapped:                              # one plain step: the launches of the exchange of ONE backward
        preds, extra = wrapper(batches[0][0], {})
        loss_of(cfg, False)(preds, extra, batches[0][1])["loss"].backward()
        torch.cuda.synchronize()
        plain = len(calls)
    opt = optimizer_for(model)
    rig = Rig(form, cfg, model, opt, batches, wrapper=wrapper)
    del calls[:]
    rig(batches)
    per_step = len(calls)
    rig(batches)
    torch.cuda.synchronize()
    assert len(calls) == 2 * per_step and (not wrapped or not wrapper._works)
    torch.save({"flat": model.flat.data.detach().cpu(), "grad": model.flat.grad.detach().cpu(), "plain": plain,
                "per_step": per_step, "applied": opt.stats()["applied"]}, out)
    if wrapped:
        dist.barrier()
        dist.destroy_process_group()


@pytest.mark.parametrize("form", FORMS)
def test_e_exchange_runs_in_the_last_micro_step_only(tmp_path, form):
    bare = _spawn(_dp_worker, 1, str(tmp_path / "bare.pt"), form, False)
    dp = _spawn(_dp_worker, 1, str(tmp_path / "dp.pt"), form, True)
    assert dp["plain"] > 0 and dp["per_step"] == dp["plain"], (dp["plain"], dp["per_step"])
    assert bare["per_step"] == 0 and bare["applied"] == dp["applied"] == 2
    assert torch.equal(bare["grad"].view(torch.int32), dp["grad"].view(torch.int32))
    assert torch.equal(bare["flat"].view(torch.int32), dp["flat"].view(torch.int32))


# ------------------------------------------------------------------------------------------- (f) dropped step ----
@pytest.mark.parametrize("form", FORMS)
def test_f_one_non_finite_micro_step_drops_the_whole_step(form):
    cfg, model = build(mode="reproducible")
    opt = optimizer_for(model)
    clean = [video(), video("B"), image()]
    poisoned = [clean[0], video("B"), clean[2]]
    poisoned[1][0][0][1, 2, 3, 17, 40] = float("nan")                 # the input clip of micro-step 2 of 3
    rig = Rig(form, cfg, model, opt, clean)
    before = [t.clone() for t in (model.flat.data, opt.exp_avg, opt.exp_avg_sq)]
    rig(poisoned)
    assert not bool(torch.isfinite(model.flat.grad).all())
    for name, a, b in zip(("weights", "exp_avg", "exp_avg_sq"), (model.flat.data, opt.exp_avg, opt.exp_avg_sq), before):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32)), name
    s = opt.stats()
    assert s["skipped"] == 1 and s["applied"] == 0 and opt.step_count == 0
    rig(clean)
    s = opt.stats()
    assert s["skipped"] == 1 and s["applied"] == 1 and s["consecutive_skipped"] == 0
    assert bool(torch.isfinite(model.flat.data).all()) and not torch.equal(model.flat.data, before[0])


# -------------------------------------------------------------------------------------------------- (g) meter ----
def test_g_meter_logs_the_per_key_mean_over_the_virtual_ranks():
    from svit_amd import train
    from svit_amd.meters import TrainMeter
    cfg, model = build(mode="reproducible")
    cfg.LOG_PERIOD = 2
    opt = optimizer_for(model)
    iters = [[video(t), image(t)] for t in ("", "B", "C", "D")]
    s0 = snapshot(model, opt)
    # the eager twin, read back separately: every micro-step's loss dict of every iteration
    want = []
    for batches in iters:
        seen = []
        train.accumulate_step(model, [loss_of(cfg, is_image(b), seen) for b in batches], batches, opt)
        torch.cuda.synchronize()
        assert len(seen) == 2 and set(seen[0]) == {"loss_ce", "loss"} and "boxes_giou_loss" in seen[1]
        per_key = {}
        for d in seen:                                                # recipe-rank order
            for k, v in d.items():
                per_key.setdefault(k, []).append(float(v))
        want.append({k: sum(v) / len(v) for k, v in per_key.items()})
    restore(model, opt, s0)
    meter = TrainMeter(4, cfg, virtual_ranks=2)
    rig = Rig("graphed", cfg, model, opt, iters[0], meter=meter)
    assert all(int(r.state[0]) == 0 for r in meter._rings if r.state is not None)       # empty after construction
    for it, batches in enumerate(iters):
        rig(batches)
        got = meter.log_iter_stats(0, it)
        assert (got is None) == (it % 2 == 0)
        if got is not None:
            assert set(want[it]) <= set(got) and len(want[it]) == 6
            for k in want[it]:
                assert float(got[k]) == float(np.median([want[it - 1][k], want[it][k]])), (it, k)
            assert got["lr"] == LR
    assert meter.num_samples == 4 * (2 + 3)                           # mb_size = sum of the micro-batches x 1 rank
    # a NaN loss raises check_nan_losses's message at the period and names the iteration
    meter.reset()
    bad = [video("B"), image("B")]
    bad[0][0][0][1, 0, 0, 5, 5] = float("nan")
    rig(iters[0])
    rig(bad)
    with pytest.raises(RuntimeError, match=r"Got NaN losses.*first at iteration 1 of the epoch \(virtual rank 0\)"):
        meter.log_iter_stats(0, 1)


# ------------------------------------------------------------------------ (h) draws advance per micro-step ----
@pytest.mark.parametrize("form", FORMS)
def test_h_every_micro_step_draws_its_own_drop_path(form):
    torch.manual_seed(1234)
    cfg, model = build(droppath=0.4, mode="reproducible")
    opt = optimizer_for(model)
    batch = video()
    rig = Rig(form, cfg, model, opt, [batch, batch])
    if model._rng_state is None:                  # (the eager form has not drawn yet)
        model.sample_drop_scales(2, "cuda", Tx=4)
    s0 = snapshot(model, opt)
    draws0 = int(s0[4][1])
    l1 = rig([batch, batch])
    assert int(l1[0]) != int(l1[1])                                   # the same clips, other DropPath draws
    assert int(model._rng_state[1]) == draws0 + 2
    first = state_bits(model, opt) + [l1]
    rig([batch, batch])
    assert int(model._rng_state[1]) == draws0 + 4
    restore(model, opt, s0)
    l2 = rig([batch, batch])
    assert_bits(state_bits(model, opt) + [l2], first, "two runs from the same seed and state")


# ---------------------------------------------------------------------------------------------- (i) refusals ----
def test_i_refusals():
    from svit_amd import hip, optim
    from svit_amd.graph import AccumulatedTrainStep, GraphedTrainStep
    cfg, model = build(mode="reproducible")
    opt = optimizer_for(model)
    A, C = video(), image()
    micro = GraphedTrainStep(model, loss_of(cfg, False), A[0], A[1], accumulate=True)
    step = AccumulatedTrainStep(model, [micro, micro], opt)
    w0 = model.flat.data.clone()
    with pytest.raises(hip.SvitHipError, match="2 micro-steps, got 3 batches"):
        step([A, A, A])
    with pytest.raises(hip.SvitHipError, match="micro-step 1.*captured for input"):
        step([A, C])
    with pytest.raises(hip.SvitHipError, match="micro-step"):
        GraphedTrainStep(model, loss_of(cfg, False), A[0], A[1], accumulate=True, optimizer=opt)
    with pytest.raises(hip.SvitHipError, match="its own optimizer"):
        AccumulatedTrainStep(model, [micro, GraphedTrainStep(model, loss_of(cfg, False), A[0], A[1], optimizer=opt)], opt)
    with pytest.raises(hip.SvitHipError, match="without accumulate=True"):
        AccumulatedTrainStep(model, [GraphedTrainStep(model, loss_of(cfg, False), A[0], A[1])], opt)
    with pytest.raises(hip.SvitHipError, match="GuardedClipAdamW"):
        AccumulatedTrainStep(model, [micro], optim.FusedClipAdamW(model, lr=LR))
    _, other = build(mode="reproducible")
    with pytest.raises(hip.SvitHipError, match="another model"):
        AccumulatedTrainStep(other, [micro], optimizer_for(other))
    with pytest.raises(hip.SvitHipError, match="another model"):
        AccumulatedTrainStep(model, [micro], optimizer_for(other))
    from svit_amd.meters import TrainMeter
    with pytest.raises(hip.SvitHipError, match="virtual_ranks=2"):
        AccumulatedTrainStep(model, [micro, micro], opt, meter=TrainMeter(4, cfg))
    model.eval()
    with pytest.raises(RuntimeError, match="train"):
        AccumulatedTrainStep(model, [micro], opt)
    with pytest.raises(RuntimeError, match="train"):
        step([A, A])
    from svit_amd import train
    with pytest.raises(RuntimeError, match="train"):
        train.accumulate_step(model, [loss_of(cfg, False)], [A], opt)
    model.train()
    torch.cuda.synchronize()
    assert torch.equal(model.flat.data, w0) and opt.stats()["applied"] == 0        # nothing refused moved a weight
    step([A, A])
    assert opt.stats()["applied"] == 1


# ------------------------------------------------------------------- (j) the keyword is inert when absent ----
def test_j_plain_graphed_step_is_unchanged():
    from svit_amd.graph import GraphedTrainStep
    cfg, model = build(mode="reproducible")
    opt = optimizer_for(model)
    A = video()
    s0 = snapshot(model, opt)
    fn = loss_of(cfg, False)
    preds, extra = model(A[0], {})
    loss = fn(preds, extra, A[1])["loss"]
    opt.zero_grad()
    loss.backward()
    opt.step()
    eager = state_bits(model, opt) + [loss.detach().reshape(1).cpu().view(torch.int32)]
    restore(model, opt, s0)
    step = GraphedTrainStep(model, fn, A[0], A[1], optimizer=opt)
    assert step.accumulate is False and step.n_graphs == 1 and [k for k, _ in step.segments] == ["graph"]
    got, _ = step(A[0], A[1])
    graphed = state_bits(model, opt) + [got.detach().reshape(1).cpu().view(torch.int32)]
    assert_bits(graphed, eager, "plain graphed step against the eager step")
    # the micro-step form is the same capture minus the prologue: as many graphs
    assert GraphedTrainStep(model, fn, A[0], A[1], accumulate=True).n_graphs == step.n_graphs


# ------------------------------------------------------------------------------------------------ the loop ----
def test_k_train_epoch_over_an_accumulated_step():
    """train.train_epoch with a loader that yields k (inputs, labels, idx, meta) per iteration, three iterations at
    LOG_PERIOD 2: the epoch line equals the per-key global average of an eager twin's losses under the same lr schedule,
    the weights after it are the twin's"""
    from svit_amd import optim, train
    from svit_amd.meters import TrainMeter
    cfg, model = build(mode="reproducible")
    cfg.LOG_PERIOD = 2
    opt = optimizer_for(model)
    host = lambda t: {k: v.cpu() for k, v in t.items()} if isinstance(t, dict) else t.cpu()
    loader = []
    for tag in ("", "B", "C"):
        (vx, vy), (ix, imeta) = video(tag), image(tag)
        loader.append([([vx[0].cpu()], host(vy), None, {}),
                       ([ix[0].cpu()], torch.zeros(3, dtype=torch.int64), None, host(imeta))])
    s0 = snapshot(model, opt)
    want, lrs = {}, []
    for it, micro in enumerate(loader):
        lrs.append(optim.get_lr_at_epoch(cfg, it / 3.0)["lr"])
        optim.set_lr(opt, lrs[-1])
        seen = []
        batches = [video(("", "B", "C")[it]), image(("", "B", "C")[it])]
        train.accumulate_step(model, [loss_of(cfg, is_image(b), seen) for b in batches], batches, opt)
        per_key = {}
        for d in seen:
            for k, v in d.items():
                per_key.setdefault(k, []).append(float(v))
        for k, v in per_key.items():
            want.setdefault(k, []).append(sum(v) / len(v))
    twin = state_bits(model, opt)[1:]
    restore(model, opt, s0)
    meter = TrainMeter(len(loader), cfg, virtual_ranks=2)
    rig = Rig("graphed", cfg, model, opt, [video(), image()], meter=meter)
    with pytest.raises(ValueError, match="meter="):
        train.train_epoch(loader, rig.step, opt, TrainMeter(len(loader), cfg, virtual_ranks=2), 0, cfg)
    with pytest.raises(ValueError, match="yielded 1 micro-batches"):
        train.train_epoch([loader[0][:1]], rig.step, opt, meter, 0, cfg)
    epoch = train.train_epoch(loader, rig.step, opt, meter, 0, cfg)
    assert epoch["_type"] == "train_epoch" and epoch["lr"] == lrs[-1] and len(set(lrs)) == 3
    assert len(want) == 6
    for k, v in want.items():
        assert float(epoch[k]) == sum(v) / 3, k
    for name, a, b in zip(("weights", "exp_avg", "exp_avg_sq"), state_bits(model, opt)[1:], twin):
        assert torch.equal(a, b), name
    assert opt.stats()["applied"] == 3 and meter.num_samples == 0            # train_epoch ends with reset()
