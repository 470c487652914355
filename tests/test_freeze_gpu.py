"""Frozen parameters on the GPU: the segment kernels of the guarded tail (svit_step_guard_seg /
svit_adamw_step_guarded_seg) against the plain pair, and the model under a cut -- forward, the shortened backward, the
optimizers, the captured and the accumulated step, a one-rank RCCL exchange and a checkpoint round trip.  Every
comparison is bit equality.  Needs a real MI355X."""
import os
import socket
import sys
import types

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import procedural as P
from oracle import svit_ref as R
from tests import freeze_cases as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda"
N, ND = 20000, 12296
BETAS, EPS = (0.9, 0.999), 1e-8


def bits(t):
    return t.contiguous().view(torch.int32)


def same(a, b):
    return torch.equal(bits(a), bits(b))


# ===================================================================================================== kernels ====
@pytest.fixture(scope="module")
def table():
    from svit_amd import ops
    return torch.from_numpy(ops.adamw_bias_table(*BETAS)).to(DEV)


class Tail:
    """p, g, m, v f32 [N] + the two step records; `run` is the plain pair, or the `_seg` pair over `segs`"""

    def __init__(self, table, g_amp=1.0, clip=1.0, clip_value=None, grad_scale=1.0, applied=5):
        from svit_amd.optim import pack_step_host
        self.table = table
        self.p = P.tensor("freeze:p", (N,), 0.1).to(DEV)
        self.g = P.tensor("freeze:g", (N,), g_amp).to(DEV)
        self.m = P.tensor("freeze:m", (N,), 0.01).to(DEV)
        self.v = P.tensor("freeze:v", (N,), 0.01).to(DEV).square()
        self.host = torch.from_numpy(pack_step_host((1e-3, 3e-3), (0.05, 0.01), clip, clip_value, grad_scale)).to(DEV)
        self.rec = torch.zeros(12, dtype=torch.int32, device=DEV)
        self.rec.view(torch.int64)[0:1].fill_(applied)
        self.ws = torch.zeros(1024, device=DEV)

    def twin(self):
        t = Tail.__new__(Tail)
        t.table, t.host, t.ws = self.table, self.host, torch.zeros(1024, device=DEV)
        t.p, t.g, t.m, t.v, t.rec = (x.clone() for x in (self.p, self.g, self.m, self.v, self.rec))
        return t

    def run(self, segs=None):
        from svit_amd import ops
        if segs is None:
            ops.step_guard(self.g, self.host, self.rec, self.table, self.ws)
            ops.adamw_step_guarded(self.p, self.g, self.m, self.v, ND, self.host, self.rec, *BETAS, EPS)
        else:
            segs = np.ascontiguousarray(np.array(segs, dtype=np.int64).reshape(-1, 2))
            ops.step_guard_seg(self.g, segs, self.host, self.rec, self.table, self.ws)
            ops.adamw_step_guarded_seg(self.p, self.g, self.m, self.v, ND, segs, self.host, self.rec, *BETAS, EPS)
        torch.cuda.synchronize()

    def stats(self):
        from svit_amd import hip
        return hip.StepDev.from_buffer_copy(self.rec.cpu().numpy().tobytes())


SEGS = [[0, 8], [4104, 4120], [ND - 8, ND], [ND, ND + 8], [13000, 19000], [N - 8, N]]


def _mask(segs):
    m = torch.zeros(N, dtype=torch.bool, device=DEV)
    for a, b in segs:
        m[a:b] = True
    return m


def _poison_outside(t, inside):
    """what a frozen range may hold: NaN / +-inf / 1e30 gradients, canaries in p, m, v"""
    out = ~inside
    bad = torch.tensor([float("nan"), float("inf"), -float("inf"), 1e30], device=DEV).repeat(N // 4)
    t.g[out] = bad[out]
    t.p[out], t.m[out], t.v[out] = 123.456, -7.0, 9.0e9


def test_a_whole_buffer_as_two_segments_is_the_plain_pair(table):
    a = Tail(table)
    b = a.twin()
    a.run([[0, ND], [ND, N]])
    b.run()
    for name in ("p", "m", "v", "rec"):
        assert same(getattr(a, name), getattr(b, name)), name
    assert a.stats().apply == 1 and a.stats().applied == 6


@pytest.mark.parametrize("case", ["norm clip", "clip by value", "grad_scale 0.5", "no clip"])
def test_b_d_segments_against_the_plain_pair_on_a_zeroed_twin(table, case):
    kw = {"norm clip": {}, "clip by value": dict(g_amp=0.05, clip_value=0.01), "grad_scale 0.5": dict(grad_scale=0.5),
          "no clip": dict(clip=None)}[case]
    a = Tail(table, **kw)
    inside = _mask(SEGS)
    assert int(inside.sum()) == 8 + 16 + 8 + 8 + 6000 + 8
    b = a.twin()
    b.g[~inside] = 0.0                       # the twin: frozen gradients are zero, the plain pair runs over everything
    _poison_outside(a, inside)
    before = [x.clone() for x in (a.p, a.m, a.v)]
    a.run(SEGS)
    b.run()
    s = a.stats()
    assert s.apply == 1 and s.applied == 6 and s.skipped == 0          # NaN / inf / 1e30 outside did not drop the step
    assert same(a.rec, b.rec)                                          # the whole record, coefficient included
    if case == "norm clip":
        assert 0.0 < s.coef < 1.0
    if case == "grad_scale 0.5":
        assert 0.0 < s.coef < 0.5
    if case == "clip by value":
        gi = a.g[inside]
        assert float((gi.abs() > 0.01).float().mean()) > 0.3 and float((gi.abs() < 0.01).float().mean()) > 0.05
    for name, x, y, x0 in zip("pmv", (a.p, a.m, a.v), (b.p, b.m, b.v), before):
        assert same(x[inside], y[inside]), (case, name, int((bits(x[inside]) != bits(y[inside])).sum()))
        assert same(x[~inside], x0[~inside]), (case, name, "a frozen element was written")
        assert not same(x[inside], x0[inside])


def test_c_a_nan_inside_a_segment_drops_the_step(table):
    a = Tail(table)
    inside = _mask(SEGS)
    _poison_outside(a, inside)
    a.g[13001] = float("nan")
    before = [x.clone() for x in (a.p, a.g, a.m, a.v)]
    r0 = a.stats()
    a.run(SEGS)
    for name, x, x0 in zip("pgmv", (a.p, a.g, a.m, a.v), before):
        assert same(x, x0), name
    s = a.stats()
    assert (s.apply, s.applied, s.skipped, s.consecutive) == (0, r0.applied, r0.skipped + 1, r0.consecutive + 1)
    assert (s.coef, s.sumsq, s.grad_norm) == (r0.coef, r0.sumsq, r0.grad_norm)


def test_wrappers_refuse_a_bad_table(table):
    from svit_amd import hip
    a = Tail(table)
    for bad in ([[8, 16], [0, 8]], [[0, 6]], [[0, N + 8]], [[16, 16]]):
        before = [x.clone() for x in (a.p, a.m, a.v, a.rec)]
        with pytest.raises(hip.SvitHipError):
            a.run(bad)
        assert all(same(x, y) for x, y in zip((a.p, a.m, a.v, a.rec), before))


# ======================================================================================================= model ====
LR = 1e-3


def build(droppath=0.0, mode="deterministic"):
    """the tiny model of the other step tests with the procedural weights, in train mode"""
    from svit_amd import config
    from svit_amd.model import MODEL_REGISTRY
    cfg = config.ssv2_cfg(num_frames=4, crop=64)
    cfg.MVIT.DROPPATH_RATE = droppath
    cfg.MODEL.DROPOUT_RATE = 0.0
    if mode == "reproducible":
        cfg.SVIT.REPRODUCIBLE = True
    model = MODEL_REGISTRY.get("SViT")(cfg).cuda()
    model.load_state_dict(P.state_dict(R.param_shapes(R.make_spec(4, 64, drop_path_rate=droppath, dropout_rate=0.0))))
    model.train()
    if mode == "deterministic":
        model.engine.deterministic = True
    assert len(model.plan.blocks) == F.DEPTH
    return cfg, model


def batch(tag=""):
    return P.frames(2, 4, 64, tag="clip" + tag).cuda(), P.labels(2, tag="label" + tag).cuda()


def fwd_bwd(model, x, y, ds=None):
    """one eager forward / backward after zero_grad(set_to_none=True) -> (logits, loss, flat.grad), copies"""
    for p in model.parameters():
        p.grad = None
    logits, _ = model([x], {}, drop_scales=ds)
    loss = torch.nn.functional.cross_entropy(logits, y)
    loss.backward()
    torch.cuda.synchronize()
    return logits.detach().clone(), loss.detach().clone(), model.flat.grad.clone()


def seg_mask(model, cut):
    m = torch.zeros(model.flat.total, dtype=torch.bool, device=DEV)
    for a, b in model.trainable_segments(cut):
        m[int(a):int(b)] = True
    return m


def explicit_drop_scales(model):
    """per block (attention branch, MLP branch) factors 0 or 1 / keep for the two samples, as DropPath draws them: in
    frozen and in trainable blocks samples are dropped, and both arms of a comparison get these very tensors"""
    ds = []
    for b in model.plan.blocks:
        if b.drop_path <= 0.0:
            ds.append(None)
            continue
        k = 1.0 / (1.0 - b.drop_path)
        ds.append((torch.tensor([k, 0.0 if b.index % 3 == 0 else k], device=DEV),
                   torch.tensor([0.0 if b.index % 4 == 1 else k, k], device=DEV)))
    assert sum(d is not None for d in ds) >= F.DEPTH - 1
    return ds


_REF = {}


def reference(mode, droppath):
    """the unfrozen model's pass, computed once per configuration and left unchanged"""
    key = (mode, droppath)
    if key not in _REF:
        cfg, model = build(droppath, mode)
        x, y = batch()
        ds = explicit_drop_scales(model) if droppath else None
        assert model.frozen_cut() == 0
        logits, loss, grad = fwd_bwd(model, x, y, ds)
        assert all(p.grad is not None for p in model.parameters())
        _REF[key] = dict(cfg=cfg, model=model, x=x, y=y, ds=ds, logits=logits, loss=loss, grad=grad,
                         w0=model.flat.data.clone())
    return _REF[key]


@pytest.mark.parametrize("cut", F.CUTS_GPU)
@pytest.mark.parametrize("mode,droppath", [("deterministic", 0.0), ("reproducible", 0.0), ("deterministic", 0.4)])
def test_forward_and_backward_under_a_cut(mode, droppath, cut):
    r = reference(mode, droppath)
    model = r["model"]
    assert same(model.flat.data, r["w0"])
    model.freeze_below(cut)
    try:
        logits, loss, grad = fwd_bwd(model, r["x"], r["y"], r["ds"])
        named = list(model.named_parameters())
    finally:
        model.freeze_below(0)
    assert same(logits, r["logits"]) and same(loss, r["loss"])
    inside = seg_mask(model, cut)
    assert 0 < int(inside.sum()) < model.flat.total
    bad = [n for n, _ in named if F.position(n) >= cut
           and not same(model.flat.view(grad, n), model.flat.view(r["grad"], n))]
    assert not bad, "trainable gradients that differ from the full backward's: %s" % bad[:8]
    assert same(grad[inside], r["grad"][inside])
    assert int(torch.count_nonzero(bits(grad[~inside]))) == 0, "a frozen range of flat.grad is not zero"
    assert float(r["grad"][~inside].abs().max()) > 0            # (the full backward does write there)


@pytest.mark.parametrize("cut", F.CUTS_GPU)
def test_frozen_parameters_keep_grad_none(cut):
    r = reference("deterministic", 0.0)
    model = r["model"]
    model.freeze_below(cut)
    try:
        fwd_bwd(model, r["x"], r["y"])
        for n, p in model.named_parameters():
            if F.position(n) >= cut:
                assert p.grad is not None and p.grad.data_ptr() == model.flat.g(n).data_ptr(), n
            else:
                assert p.grad is None, n
    finally:
        model.freeze_below(0)
        fwd_bwd(model, r["x"], r["y"])            # every view is back for the tests that follow


def test_unsupported_pattern_is_refused_by_the_training_forward():
    r = reference("deterministic", 0.0)
    model = r["model"]
    p = dict(model.named_parameters())["blocks.5.norm1.weight"]
    p.requires_grad_(False)
    try:
        with pytest.raises(NotImplementedError, match=r"blocks\.5\.norm1\.weight "):
            model([r["x"]], {})
        with torch.no_grad():
            model([r["x"]], {})                   # a pass that cannot be differentiated reads no flags
    finally:
        p.requires_grad_(True)
    # nothing trainable: a forward has nothing to differentiate (any torch module's behaviour), the optimizer refuses
    from svit_amd import optim
    for q in model.parameters():
        q.requires_grad_(False)
    try:
        logits, _ = model([r["x"]], {})
        assert not logits.requires_grad and same(logits, r["logits"])
        with pytest.raises(ValueError, match="empty parameter list"):
            optim.GuardedClipAdamW(model, lr=LR)
    finally:
        model.freeze_below(0)


@pytest.mark.parametrize("cut", F.CUTS_GPU)
@pytest.mark.parametrize("kind", ["classic", "guarded"])
def test_three_optimizer_steps(kind, cut):
    """frozen weights bit-unchanged and their moments zero (on the parent commit every weight moves); after step 1 the
    trainable weights and moments are the unfrozen optimizer's on the same gradient buffer"""
    from svit_amd import optim
    r = reference("deterministic", 0.0)
    model, flat = r["model"], r["model"].flat
    cls = optim.FusedClipAdamW if kind == "classic" else optim.GuardedClipAdamW
    kw = dict(lr=LR, weight_decay=0.05, clip_grad_l2norm=1.0)
    model.freeze_below(cut)
    try:
        opt = cls(model, **kw)
        assert opt.cut == cut
        inside = seg_mask(model, cut)
        for i in range(3):
            optim.set_lr(opt, LR * (i + 1))
            opt.zero_grad()
            logits, _ = model([r["x"]], {})
            torch.nn.functional.cross_entropy(logits, r["y"]).backward()
            if i == 0:
                twin_flat = types.SimpleNamespace(total=flat.total, n_decay=flat.n_decay, data=flat.data.clone(),
                                                  grad=flat.grad.clone())
                twin = cls(types.SimpleNamespace(flat=twin_flat), **kw)
                optim.set_lr(twin, LR)
                twin.step()
            opt.step()
            torch.cuda.synchronize()
            if i == 0:
                for name, a, b in (("weights", flat.data, twin_flat.data), ("exp_avg", opt.exp_avg, twin.exp_avg),
                                   ("exp_avg_sq", opt.exp_avg_sq, twin.exp_avg_sq)):
                    assert same(a[inside], b[inside]), (name, int((bits(a[inside]) != bits(b[inside])).sum()))
                assert not same(twin_flat.data[~inside], r["w0"][~inside])     # the unfrozen optimizer decays them
        assert opt.step_count == 3
        assert same(flat.data[~inside], r["w0"][~inside]), "a frozen weight moved"
        assert not same(flat.data[inside], r["w0"][inside])
        assert int(torch.count_nonzero(opt.exp_avg[~inside])) == 0 and int(torch.count_nonzero(opt.exp_avg_sq[~inside])) == 0
        assert int(torch.count_nonzero(opt.exp_avg[inside])) > 0
    finally:
        flat.data.copy_(r["w0"])
        model.freeze_below(0)
        fwd_bwd(model, r["x"], r["y"])


def _count_launches(monkeypatch, fn):
    """library launches issued while fn() runs (the captured body's kernel nodes are among them, the same number of
    warm-up bodies on every arm)"""
    from svit_amd import hip
    n = [0]
    real = hip.call

    def counting(name, *a, **k):
        n[0] += 1
        return real(name, *a, **k)
    monkeypatch.setattr(hip, "call", counting)
    try:
        out = fn()
    finally:
        monkeypatch.setattr(hip, "call", real)
    return out, n[0]


def test_graphed_step_at_cut_4(monkeypatch):
    from svit_amd import hip, optim
    from svit_amd.graph import GraphedTrainStep
    cut = 4
    kw = dict(lr=LR, weight_decay=0.05, clip_grad_l2norm=1.0)
    poison = torch.ones(1, device=DEV)

    def loss_fun(p, e, y):
        return torch.nn.functional.cross_entropy(p, y) * poison

    x, y = batch()
    _, mg = build()
    _, me = build()
    _, mf = build()
    w0 = mg.flat.data.clone()
    mg.freeze_below(cut)
    me.freeze_below(cut)
    og, oe, of = (optim.GuardedClipAdamW(m, **kw) for m in (mg, me, mf))
    full, n_full = _count_launches(monkeypatch, lambda: GraphedTrainStep(mf, loss_fun, [x], y, optimizer=of))
    step, n_cut = _count_launches(monkeypatch, lambda: GraphedTrainStep(mg, loss_fun, [x], y, optimizer=og))
    assert step.cut == cut and full.cut == 0
    assert n_cut < n_full, (n_cut, n_full)
    torch.cuda.synchronize()
    assert same(mg.flat.data, w0) and og.stats()["applied"] == 0

    def eager():
        oe.zero_grad()
        logits, extra = me([x], {})
        loss = loss_fun(logits, extra, y)
        loss.backward()
        oe.step()
        return loss.detach()

    def compare(what):
        torch.cuda.synchronize()
        for name, a, b in (("weights", mg.flat.data, me.flat.data), ("exp_avg", og.exp_avg, oe.exp_avg),
                           ("exp_avg_sq", og.exp_avg_sq, oe.exp_avg_sq), ("grad", mg.flat.grad, me.flat.grad)):
            assert same(a, b), (what, name, int((bits(a) != bits(b)).sum()))
        assert og.stats() == oe.stats(), what

    for i in range(3):
        optim.set_lr(og, LR * (i + 1))
        optim.set_lr(oe, LR * (i + 1))
        lg, _ = step([x], y)
        le = eager()
        assert same(lg, le)
        compare("step %d" % (i + 1))
    poison.fill_(float("nan"))
    before = mg.flat.data.clone()
    step([x], y)
    eager()
    compare("poisoned step")
    assert same(mg.flat.data, before) and og.stats()["skipped"] == 1 and og.stats()["applied"] == 3
    poison.fill_(1.0)
    inside = seg_mask(mg, cut)
    assert same(mg.flat.data[~inside], w0[~inside]) and not same(mg.flat.data[inside], w0[inside])
    # the flags are the truth: a replay after one changed is refused, and nothing is enqueued
    p = dict(mg.named_parameters())["blocks.2.norm1.weight"]
    p.requires_grad_(True)
    before = mg.flat.data.clone()
    with pytest.raises(hip.SvitHipError, match="rebuild"):
        step([x], y)
    torch.cuda.synchronize()
    assert same(mg.flat.data, before)
    p.requires_grad_(False)
    step([x], y)                                    # the old flags again: the capture fits
    # an optimizer built over other flags than the step
    mg.freeze_below(0)
    with pytest.raises(hip.SvitHipError, match="rebuild"):
        GraphedTrainStep(mg, loss_fun, [x], y, optimizer=og)
    torch.cuda.synchronize()


def test_unfrozen_capture_is_unchanged():
    """nothing frozen: the segments of a capture and its weights after a step are those of a model that never heard of
    cuts (the cut-0 calls take the entry points they always took)"""
    from svit_amd import optim
    from svit_amd.graph import GraphedTrainStep
    x, y = batch()
    _, ma = build()
    _, mb = build()
    mb.freeze_below(3)
    mb.freeze_below(0)
    kw = dict(lr=LR, weight_decay=0.05, clip_grad_l2norm=1.0)
    oa, ob = optim.GuardedClipAdamW(ma, **kw), optim.GuardedClipAdamW(mb, **kw)
    assert oa.segments is None and ob.segments is None
    f = lambda p, e, l: torch.nn.functional.cross_entropy(p, l)
    sa, sb = GraphedTrainStep(ma, f, [x], y, optimizer=oa), GraphedTrainStep(mb, f, [x], y, optimizer=ob)
    assert [k for k, _ in sa.segments] == [k for k, _ in sb.segments]
    sa([x], y)
    sb([x], y)
    torch.cuda.synchronize()
    assert same(ma.flat.data, mb.flat.data) and same(ma.flat.grad, mb.flat.grad)
    assert all(p.grad is not None for p in mb.parameters())


def test_accumulated_step_k2():
    from svit_amd import optim
    from svit_amd.graph import AccumulatedTrainStep, GraphedTrainStep
    cut = 4
    _, model = build()
    model.freeze_below(cut)
    A, B = batch(), batch("B")
    gA = fwd_bwd(model, *A)[2]
    gB = fwd_bwd(model, *B)[2]
    assert not same(gA, gB)
    inside = seg_mask(model, cut)
    opt = optim.GuardedClipAdamW(model, lr=LR, weight_decay=0.05, clip_grad_l2norm=1.0)
    f = lambda p, e, l: torch.nn.functional.cross_entropy(p, l)
    micro = GraphedTrainStep(model, f, [A[0]], A[1], accumulate=True)
    assert micro.cut == cut
    step = AccumulatedTrainStep(model, [micro, micro], opt)
    w0 = model.flat.data.clone()
    step([([A[0]], A[1]), ([B[0]], B[1])])
    torch.cuda.synchronize()
    want = gA + gB
    assert same(model.flat.grad[inside], want[inside])
    assert int(torch.count_nonzero(bits(model.flat.grad[~inside]))) == 0
    assert opt.stats()["applied"] == 1 and same(model.flat.data[~inside], w0[~inside])
    assert not same(model.flat.data[inside], w0[inside])
    # a micro-step captured over other flags than the optimizer's
    model.freeze_below(7)
    other = GraphedTrainStep(model, f, [A[0]], A[1], accumulate=True)
    from svit_amd import hip
    with pytest.raises(hip.SvitHipError, match="rebuild"):
        AccumulatedTrainStep(model, [other], opt)


def test_checkpoint_round_trip_under_a_cut(tmp_path):
    from svit_amd import checkpoint, optim
    cut = 7
    cfg, model = build()
    model.freeze_below(cut)
    opt = optim.GuardedClipAdamW(model, lr=LR, weight_decay=0.05, clip_grad_l2norm=1.0)
    x, y = batch()
    for _ in range(2):
        opt.zero_grad()
        logits, _ = model([x], {})
        torch.nn.functional.cross_entropy(logits, y).backward()
        opt.step()
    torch.cuda.synchronize()
    path = checkpoint.save_checkpoint(str(tmp_path), model, opt, 3, cfg)
    ck = torch.load(path, map_location="cpu", weights_only=False)
    n_train = sum(1 for p in model.parameters() if p.requires_grad)
    assert len(ck["model_state"]) == 405 and len(ck["optimizer_state"]["state"]) == n_train < 405
    cfg2, model2 = build()
    model2.flat.data.zero_()
    model2.freeze_below(cut)
    opt2 = optim.GuardedClipAdamW(model2, lr=LR, weight_decay=0.05, clip_grad_l2norm=1.0)
    assert checkpoint.load_checkpoint(path, model2, data_parallel=False, optimizer=opt2) == 3
    assert same(model2.flat.data, model.flat.data)
    assert same(opt2.exp_avg, opt.exp_avg) and same(opt2.exp_avg_sq, opt.exp_avg_sq) and opt2.step_count == 2
    # a model with other flags refuses the optimizer state (the weights themselves load as ever)
    cfg3, model3 = build()
    opt3 = optim.GuardedClipAdamW(model3, lr=LR, weight_decay=0.05, clip_grad_l2norm=1.0)
    with pytest.raises(ValueError, match="optimizer state lists %d parameters, the model has 405" % n_train):
        checkpoint.load_checkpoint(path, model3, data_parallel=False, optimizer=opt3)


# ------------------------------------------------------------------------------------- data parallel
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _dp_worker(port, out):
    """one rank on the RCCL group: three replayed guarded steps at cut 4 without and with
    DataParallel(force_collectives=True), and one unfrozen data-parallel step for its collective count"""
    import torch.distributed as dist
    sys.path.insert(0, ROOT)
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    torch.cuda.set_device(0)
    dist.init_process_group("nccl", rank=0, world_size=1, device_id=torch.device("cuda", 0))
    from svit_amd import optim
    from svit_amd.dp import DataParallel
    from svit_amd.graph import GraphedTrainStep
    x, y = batch()
    res = {}
    for arm, cut in (("plain", 4), ("dp", 4), ("dp_full", 0)):
        _, model = build()
        model.freeze_below(cut)
        dp = model if arm == "plain" else DataParallel(model, bucket_ranks=4, force_collectives=True)
        calls = []
        if arm != "plain":
            real = dp._reduce_slice
            dp._reduce_slice = lambda a, b, real=real, calls=calls: (calls.append((a, b)), real(a, b))[1]
        opt = optim.GuardedClipAdamW(dp, lr=LR, weight_decay=0.05, clip_grad_l2norm=1.0)
        step = GraphedTrainStep(dp, lambda p, e, l: torch.nn.functional.cross_entropy(p, l), [x], y, optimizer=opt)
        calls.clear()
        steps = 3 if cut else 1
        for i in range(steps):
            optim.set_lr(opt, LR * (i + 1))
            step([x], y)
        torch.cuda.synchronize()
        res[arm] = {"p": model.flat.data.cpu(), "m": opt.exp_avg.cpu(), "v": opt.exp_avg_sq.cpu(), "stats": opt.stats(),
                    "collectives": len(calls) // steps, "bytes": getattr(dp, "exchanged_bytes", None),
                    "slices": calls[:len(calls) // steps],
                    "trainable_bytes": 4 * int(sum(b - a for a, b in model.trainable_segments(cut))),
                    "total_bytes": 4 * model.flat.total}
    torch.save(res, out)
    dist.barrier()
    dist.destroy_process_group()


def test_one_rank_rccl_exchange_covers_the_trainable_ranges(tmp_path):
    import torch.multiprocessing as mp
    out = str(tmp_path / "dp.pt")
    proc = mp.get_context("spawn").Process(target=_dp_worker, args=(_free_port(), out))
    proc.start()
    proc.join(600)
    assert proc.exitcode == 0, proc.exitcode
    res = torch.load(out)
    plain, dp, full = res["plain"], res["dp"], res["dp_full"]
    assert plain["stats"]["applied"] == dp["stats"]["applied"] == 3
    for k in ("p", "m", "v"):
        assert torch.equal(plain[k].view(torch.int32), dp[k].view(torch.int32)), k
    assert plain["stats"] == dp["stats"]
    assert dp["bytes"] == dp["trainable_bytes"] < dp["total_bytes"]
    assert full["bytes"] == full["total_bytes"] == full["trainable_bytes"]
    assert 0 < dp["collectives"] <= full["collectives"]
    assert sum(b - a for a, b in dp["slices"]) * 4 == dp["trainable_bytes"]
