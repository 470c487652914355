"""Weight EMA on the guarded tail, on the GPU: svit_ema_step_guarded against its NumPy float32 restatement
(ema.ema_step_host), and the average carried through the optimizers -- the eager, the captured and the accumulated step, a
frozen cut, evaluation inside average_weights(), a checkpoint round trip.  Bit equality throughout.  Needs a real MI355X."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import procedural as P
from oracle import svit_ref as R
from tests import ema_cases as E

DEV = "cuda"
N, N4 = E.N, E.N4
DECAY = 0.9             # its warm-up table has 80 entries
NAN = float("nan")


def bits(t):
    return t.contiguous().view(torch.int32)


def same(a, b):
    return torch.equal(bits(a), bits(b))


# ===================================================================================================== kernel ====
@pytest.fixture(scope="module")
def table():
    from svit_amd import ops
    t = ops.ema_decay_table(DECAY)
    assert len(t) == 80 and t[-1] == np.float32(DECAY) and t[0] == np.float32(2.0 / 11.0)
    return t


class Avg:
    """ema and p f32 [n] with the two records: the guard's (applied, apply) and the average's (offset)"""

    def __init__(self, n=N, applied=1, offset=0, apply=1):
        self.n = n
        self.e = P.tensor("ema:e", (n,), 0.1).to(DEV)
        self.p = P.tensor("ema:p", (n,), 0.1).to(DEV)
        self.rec = torch.zeros(12, dtype=torch.int32, device=DEV)
        self.erec = torch.tensor([offset, 0], dtype=torch.int64, device=DEV)
        self.set(applied, apply)

    def set(self, applied, apply=1):
        self.rec.view(torch.int64)[0:1].fill_(applied)
        self.rec[5:6].fill_(apply)                     # svit_step_dev.apply, byte 20

    def poison_outside(self, inside):
        """canaries in ema outside every range; NaN / inf in p there: a load of either would show"""
        out = torch.from_numpy(~inside).to(DEV)
        self.e[out] = 123.456
        bad = torch.tensor([NAN, float("inf"), -float("inf"), 1e30], device=DEV).repeat(self.n // 4 + 1)[:self.n]
        self.p[out] = bad[out]

    def snapshot(self):
        return self.e.cpu().numpy().copy(), self.p.cpu().numpy().copy(), self.rec.cpu().numpy().copy(), \
            self.erec.cpu().numpy().copy()

    def launch(self, rows, table, decay=DECAY):
        from svit_amd import ops
        dev_table = None if table is None else torch.from_numpy(np.ascontiguousarray(table)).to(DEV)
        ops.ema_step_guarded(self.e, self.p, E.segs(rows), dev_table, decay, self.erec, self.rec)
        torch.cuda.synchronize()


def _check(a, before, rows, d, what):
    """the average is the restatement at decay d inside the ranges and untouched outside; nothing else was written"""
    from svit_amd import ema
    e0, p0, rec0, erec0 = before
    e1, p1, rec1, erec1 = a.snapshot()
    inside = E.inside(rows, a.n)
    want = e0.copy()
    want[inside] = ema.ema_step_host(e0[inside], p0[inside], d)
    assert E.same_np(e1[~inside], e0[~inside]), (what, "an element of the average outside the ranges was written")
    assert E.same_np(e1, want), (what, int((e1.view(np.int32) != want.view(np.int32)).sum()))
    assert E.same_np(p1, p0) and np.array_equal(rec1, rec0) and np.array_equal(erec1, erec0), (what, "p or a record moved")
    assert not E.same_np(e1[inside], e0[inside]), (what, "the average did not move")


@pytest.mark.parametrize("warm", [False, True])
@pytest.mark.parametrize("name", list(E.TABLES))
def test_a_kernel_is_the_restatement(table, name, warm):
    """every range table at n = 8 203, updates 1, 2 and 3 in a row (with the warm-up table each takes another decay),
    canaries outside every range"""
    from svit_amd import ema
    rows = E.TABLES[name]
    assert len(rows) <= 64 and (name != "64 ranges" or len(rows) == 64)
    a = Avg()
    a.poison_outside(E.inside(rows))
    seen = set()
    for k in (1, 2, 3):
        a.set(applied=k)
        d = ema.decay_at(k, DECAY, table if warm else None)
        seen.add(float(d))
        before = a.snapshot()
        a.launch(rows, table if warm else None)
        _check(a, before, rows, d, (name, "update %d" % k))
        a.p.mul_(0.5 + 0.25 * k)                        # another p for the next update (the canaries stay what they are)
    assert len(seen) == (3 if warm else 1)


# applied + offset -> the update number the kernel must take, against a table cut to 40 entries so that the entry past it
# (decay itself, 0.9) differs from the last one (41 / 50)
UPDATES = {
    "last table entry": (40, 0, 40),
    "one past the table": (41, 0, 41),
    "far past the table": (17, 100000, 100017),
    "an offset in front": (1, 2, 3),
    "an offset behind": (12, -9, 3),
    "sum zero clamps to 1": (5, -5, 1),
    "sum negative clamps to 1": (5, -9, 1),
}


@pytest.mark.parametrize("name", list(UPDATES))
def test_a_update_number_and_decay(table, name):
    from svit_amd import ema
    applied, offset, k = UPDATES[name]
    short = table[:40]
    assert short[39] == np.float32(41.0 / 50.0) != np.float32(DECAY)
    d = ema.decay_at(applied + offset, DECAY, short)
    assert d == (short[k - 1] if k <= 40 else np.float32(DECAY))
    rows = E.TABLES["three in a window"]
    a = Avg(applied=applied, offset=offset)
    a.poison_outside(E.inside(rows))
    before = a.snapshot()
    a.launch(rows, short)
    _check(a, before, rows, d, name)


def test_a_more_windows_than_the_grid_holds():
    """4096 workgroups at most: past 4096 x 1024 floats a workgroup takes a second window"""
    n = 4096 * 1024 + 3 * 1024 + 8
    edge = 4096 * 1024 + 512
    rows = [[0, 2048], [4096 * 1024 - 256, edge], [edge, edge + 1000], [n - 520, n]]
    a = Avg(n=n, applied=2)
    a.poison_outside(E.inside(rows, n))
    before = a.snapshot()
    a.launch(rows, None, decay=0.999)
    _check(a, before, rows, np.float32(0.999), "second window")


def test_b_a_dropped_step_returns_before_its_first_load(table):
    """apply == 0: the average is bit for bit what it was although p holds a NaN INSIDE a range (one update would carry
    it over) and the average NaNs outside"""
    rows = E.TABLES["touching"]
    inside = E.inside(rows)
    a = Avg(applied=3, apply=0)
    out = torch.from_numpy(~inside).to(DEV)
    a.e[out] = NAN
    a.p[torch.from_numpy(inside).to(DEV)] = NAN
    before = a.snapshot()
    for t in (None, table):
        a.launch(rows, t)
        assert all(x.tobytes() == x0.tobytes() for x, x0 in zip(a.snapshot(), before))
    # the same launch with apply == 1 does carry the NaN over: the kernel was not looking elsewhere
    a.set(applied=3, apply=1)
    a.launch(rows, None)
    assert bool(torch.isnan(a.e[torch.from_numpy(inside).to(DEV)]).all())


def test_c_wrapper_refuses_before_any_launch(table):
    from svit_amd import hip, ops
    a = Avg()
    before = a.snapshot()
    good = E.segs(E.TABLES["window edges"])
    t = torch.from_numpy(table).to(DEV)
    calls = {
        "unsorted": lambda: ops.ema_step_guarded(a.e, a.p, E.segs([[8, 16], [0, 8]]), t, DECAY, a.erec, a.rec),
        "a bound not a multiple of 4": lambda: ops.ema_step_guarded(a.e, a.p, E.segs([[0, 6]]), t, DECAY, a.erec, a.rec),
        "past n": lambda: ops.ema_step_guarded(a.e, a.p, E.segs([[0, N + 1]]), t, DECAY, a.erec, a.rec),
        "65 ranges": lambda: ops.ema_step_guarded(a.e, a.p, E.segs([[8 * i, 8 * i + 4] for i in range(65)]), t, DECAY,
                                                  a.erec, a.rec),
        "decay 1": lambda: ops.ema_step_guarded(a.e, a.p, good, t, 1.0, a.erec, a.rec),
        "decay 0": lambda: ops.ema_step_guarded(a.e, a.p, good, None, 0.0, a.erec, a.rec),
        "sizes differ": lambda: ops.ema_step_guarded(a.e[:N4], a.p, good, t, DECAY, a.erec, a.rec),
        "a float64 table": lambda: ops.ema_step_guarded(a.e, a.p, good, t.double(), DECAY, a.erec, a.rec),
        "an int32 ema_rec": lambda: ops.ema_step_guarded(a.e, a.p, good, t, DECAY, a.erec.int(), a.rec),
        "a host table": lambda: ops.ema_step_guarded(a.e, a.p, good, t.cpu(), DECAY, a.erec, a.rec),
        "a misaligned average": lambda: ops.ema_step_guarded(a.e[1:N4 + 1], a.p[1:N4 + 1], E.segs([[0, 8]]), t, DECAY,
                                                             a.erec, a.rec),
    }
    for label, fn in calls.items():
        with pytest.raises(hip.SvitHipError):
            fn()
        torch.cuda.synchronize()
        assert all(x.tobytes() == x0.tobytes() for x, x0 in zip(a.snapshot(), before)), label


# ======================================================================================================= model ====
LR = {"sgd": 0.05, "adam": 1e-3, "adamw": 1e-3}


def build(mode="deterministic"):
    """the tiny model of the other step tests with the procedural weights, in train mode"""
    from svit_amd import config
    from svit_amd.model import MODEL_REGISTRY
    cfg = config.ssv2_cfg(num_frames=4, crop=64)
    cfg.MVIT.DROPPATH_RATE = 0.0
    cfg.MODEL.DROPOUT_RATE = 0.0
    if mode == "reproducible":
        cfg.SVIT.REPRODUCIBLE = True
    model = MODEL_REGISTRY.get("SViT")(cfg).cuda()
    model.load_state_dict(P.state_dict(R.param_shapes(R.make_spec(4, 64, drop_path_rate=0.0, dropout_rate=0.0))))
    model.train()
    if mode == "deterministic":
        model.engine.deterministic = True
    return cfg, model


def batch(tag=""):
    return P.frames(2, 4, 64, tag="clip" + tag).cuda(), P.labels(2, tag="label" + tag).cuda()


def ce(p, e, y):
    return torch.nn.functional.cross_entropy(p, y)


def fwd_bwd(model, x, y):
    for p in model.parameters():
        p.grad = None
    model.flat.grad.zero_()
    logits, _ = model([x], {})
    torch.nn.functional.cross_entropy(logits, y).backward()
    torch.cuda.synchronize()


def with_ema(cfg, method, warmup=False, decay=DECAY):
    s = cfg.SOLVER
    s.OPTIMIZING_METHOD, s.BASE_LR, s.WEIGHT_DECAY, s.CLIP_GRAD_L2NORM = method, LR[method], 1e-4, 1.0
    s.MOMENTUM, s.DAMPENING, s.NESTEROV = 0.9, 0.0, True
    cfg.SVIT.EMA_DECAY = decay
    if warmup:
        cfg.SVIT.EMA_WARMUP = True
    return cfg


def make(method, warmup=False, mode="deterministic", cut=0):
    from svit_amd import ema, optim
    cfg, model = build(mode)
    if cut:
        model.freeze_below(cut)
    opt = optim.construct_optimizer(model, with_ema(cfg, method, warmup))
    av = ema.build_ema(cfg, model, opt)
    assert isinstance(opt, optim.GuardedClipAdamW) and opt.ema is av and av.warmup == warmup
    return cfg, model, opt, av


class HostAverage:
    """the restatement over a copy of the average: one update per applied step, from the weights the step left"""

    def __init__(self, av):
        self.av = av
        self.e = av.buf.cpu().numpy().copy()
        self.inside = E.inside(av.segments.tolist(), av.flat.total)
        self.k = 0

    def update(self):
        from svit_amd import ema
        self.k += 1
        m = self.inside
        w = self.av.flat.data.cpu().numpy()
        self.e[m] = ema.ema_step_host(self.e[m], w[m], ema.decay_at(self.k, self.av.decay, self.av.table_host))

    def check(self, what):
        got = self.av.buf.cpu().numpy()
        assert E.same_np(got, self.e), (what, int((got.view(np.int32) != self.e.view(np.int32)).sum()))


@pytest.mark.parametrize("method,warmup", [("adamw", False), ("adamw", True), ("adam", False), ("sgd", False)])
def test_d_three_steps_through_construct_optimizer(method, warmup):
    """(on the parent commit there is no svit_amd.ema)"""
    from svit_amd import optim
    x, y = batch()
    cfg, model, opt, av = make(method, warmup)
    assert type(opt) is {"adamw": optim.GuardedClipAdamW, "adam": optim.GuardedClipAdam, "sgd": optim.GuardedClipSGD}[method]
    assert same(av.buf, model.flat.data) and av.stats()["num_updates"] == 0
    host = HostAverage(av)
    assert bool(host.inside.all())
    w0 = model.flat.data.clone()
    for i in range(3):
        optim.set_lr(opt, LR[method] * (i + 1))
        fwd_bwd(model, x, y)
        opt.step()
        torch.cuda.synchronize()
        assert opt.stats()["applied"] == i + 1
        host.update()
        host.check("step %d" % (i + 1))
        want = float(np.float32((2.0 + i) / (11.0 + i))) if warmup else float(np.float32(DECAY))
        assert av.stats() == {"num_updates": i + 1, "decay": want}
    assert not same(av.buf, w0) and not same(av.buf, model.flat.data)


def test_d_a_poisoned_gradient_leaves_the_average_alone():
    x, y = batch()
    cfg, model, opt, av = make("sgd", warmup=True)
    host = HostAverage(av)
    for i in range(3):
        fwd_bwd(model, x, y)
        if i == 1:
            model.flat.grad[12345] = NAN
            before = av.buf.clone()
        opt.step()
        torch.cuda.synchronize()
        if i == 1:
            assert same(av.buf, before) and av.stats()["num_updates"] == 1 and opt.stats()["skipped"] == 1
        else:
            host.update()           # (update 2 takes the table's second entry: the dropped step was not counted)
        host.check("step %d" % (i + 1))
    assert av.stats()["num_updates"] == 2 and opt.stats()["applied"] == 2


def test_d_cut_4_frozen_ranges_stay_the_frozen_weights():
    x, y = batch()
    cfg, model, opt, av = make("adamw", cut=4)
    assert opt.cut == 4 and av.segments is opt.segments
    host = HostAverage(av)
    frozen = torch.from_numpy(~host.inside).to(DEV)
    assert 0 < int(frozen.sum()) < model.flat.total
    w0 = model.flat.data.clone()
    av.buf[frozen] += 1.0           # a marker: were the frozen ranges walked, it would decay towards the weights
    host.e[~host.inside] += np.float32(1.0)
    for i in range(3):
        fwd_bwd(model, x, y)
        opt.step()
        torch.cuda.synchronize()
        host.update()
        host.check("step %d" % (i + 1))
    assert same(model.flat.data[frozen], w0[frozen]) and same(av.buf[frozen], w0[frozen] + 1.0)
    sd = av.state_dict()["model_state"]
    assert list(sd) == list(model.state_dict()) and same(sd["cls_token"], model.cls_token.data + 1.0)


def _trace_names(monkeypatch, fn):
    """names of the library launches issued while fn() runs, in order"""
    from svit_amd import hip
    names = []
    real = hip.call

    def logging(name, *a, **k):
        names.append(name)
        return real(name, *a, **k)
    monkeypatch.setattr(hip, "call", logging)
    try:
        out = fn()
    finally:
        monkeypatch.setattr(hip, "call", real)
    return out, names


def _tail(names):
    """the optimizer tail's launches among `names`"""
    return [n for n in names if n.startswith(("svit_step_guard", "svit_adamw_step", "svit_sgd_", "svit_adam_", "svit_ema_"))]


def _state_pairs(a, b, ea, eb):
    return ([("weights", a.flat.data, b.flat.data), ("average", ea.buf, eb.buf)]
            + [(k, getattr(a, k), getattr(b, k)) for k in a.STATE])


def test_e_graphed_step_replays_the_average(monkeypatch):
    """the captured step over a poisoned first replay and three more with lr changes equals the eager step in weights,
    moments and average; a replay after the attached average changed is refused"""
    from svit_amd import hip, optim
    from svit_amd.graph import GraphedTrainStep
    poison = torch.ones(1, device=DEV)

    def loss_fun(p, e, y):
        return torch.nn.functional.cross_entropy(p, y) * poison

    x, y = batch()
    _, mg, og, eg = make("adamw", warmup=True)
    _, me, oe, ee = make("adamw", warmup=True)
    w0 = mg.flat.data.clone()
    step, names = _trace_names(monkeypatch, lambda: GraphedTrainStep(mg, loss_fun, [x], y, optimizer=og))
    assert _tail(names) == ["svit_step_guard", "svit_adamw_step_guarded", "svit_ema_step_guarded"]
    assert names[-1] == "svit_ema_step_guarded" and names[-2] == "svit_adamw_step_guarded"
    torch.cuda.synchronize()
    assert same(mg.flat.data, w0) and same(eg.buf, w0) and eg.stats()["num_updates"] == 0       # building moved nothing

    def eager():
        oe.zero_grad()
        logits, extra = me([x], {})
        loss = loss_fun(logits, extra, y)
        loss.backward()
        oe.step()
        return loss.detach()

    def compare(what):
        torch.cuda.synchronize()
        for name, a, b in _state_pairs(og, oe, eg, ee):
            assert same(a, b), (what, name, int((bits(a) != bits(b)).sum()))
        assert og.stats() == oe.stats() and eg.stats() == ee.stats(), what

    poison.fill_(NAN)
    step([x], y)
    eager()
    compare("poisoned step")
    assert same(eg.buf, w0) and eg.stats()["num_updates"] == 0 and og.stats()["skipped"] == 1
    poison.fill_(1.0)
    host = HostAverage(eg)
    for i in range(3):
        optim.set_lr(og, LR["adamw"] * (i + 1))
        optim.set_lr(oe, LR["adamw"] * (i + 1))
        lg, _ = step([x], y)
        le = eager()
        assert same(lg, le)
        compare("step %d" % (i + 1))
        host.update()
        host.check("replay %d" % (i + 1))
    assert eg.stats() == {"num_updates": 3, "decay": float(np.float32(4.0 / 13.0))} and not same(eg.buf, w0)
    # the capture holds the launch of the average attached THEN
    og.attach_ema(None)
    with pytest.raises(hip.SvitHipError, match="attached WeightEMA changed after this GraphedTrainStep was built"):
        step([x], y)
    og.attach_ema(eg)
    step([x], y)
    torch.cuda.synchronize()
    assert eg.stats()["num_updates"] == 4


def test_e_accumulated_step_k2_reproducible(monkeypatch):
    """AccumulatedTrainStep(k = 2) under SVIT.REPRODUCIBLE against the eager micro-steps + optimizer.step() on a second
    model: weights, momentum buffer and average bit for bit, ONE launch of the average per call"""
    from svit_amd import hip, optim, train
    from svit_amd.graph import AccumulatedTrainStep, GraphedTrainStep
    A, B, C = batch(), batch("B"), batch("C")
    _, mg, og, eg = make("sgd", mode="reproducible")
    _, me, oe, ee = make("sgd", mode="reproducible")
    micro = GraphedTrainStep(mg, ce, [A[0]], A[1], accumulate=True)
    step = AccumulatedTrainStep(mg, [micro, micro], og)
    w0 = mg.flat.data.clone()
    host = HostAverage(eg)
    for i, batches in enumerate(([A, B], [C, A], [B, C])):
        optim.set_lr(og, LR["sgd"] * (i + 1))
        optim.set_lr(oe, LR["sgd"] * (i + 1))
        batches = [([x], y) for x, y in batches]
        _, names = _trace_names(monkeypatch, lambda: step(batches))
        assert names.count("svit_ema_step_guarded") == 1 and names[-1] == "svit_ema_step_guarded"
        assert _tail(names) == ["svit_step_guard", "svit_sgd_step_guarded", "svit_ema_step_guarded"]
        train.accumulate_step(me, [ce, ce], batches, oe)
        torch.cuda.synchronize()
        for name, a, b in _state_pairs(og, oe, eg, ee):
            assert same(a, b), ("call %d" % (i + 1), name, int((bits(a) != bits(b)).sum()))
        assert og.stats() == oe.stats() and eg.stats() == ee.stats() == {"num_updates": i + 1, "decay": float(np.float32(DECAY))}
        host.update()
        host.check("call %d" % (i + 1))
    assert not same(eg.buf, w0)
    og.attach_ema(None)
    with pytest.raises(hip.SvitHipError, match="attached WeightEMA changed after this AccumulatedTrainStep was built"):
        step(batches)


def _trained(method="adamw", steps=2, **kw):
    x, y = batch()
    cfg, model, opt, av = make(method, **kw)
    for _ in range(steps):
        fwd_bwd(model, x, y)
        opt.step()
    torch.cuda.synchronize()
    return cfg, model, opt, av


def test_f_average_weights_exchanges_and_restores():
    from svit_amd.graph import GraphedTrainStep
    x, y = batch()
    cfg, model, opt, av = _trained()
    step = GraphedTrainStep(model, ce, [x], y, optimizer=opt)
    torch.cuda.synchronize()
    w, e, rec = model.flat.data.clone(), av.buf.clone(), opt.dev_rec.clone()
    assert not same(w, e)
    # a second model, loaded from the state the average writes
    _, twin = build()
    twin.load_state_dict(av.state_dict()["model_state"])
    twin.eval()
    assert same(twin.flat.data, e)
    with torch.no_grad():
        want = twin([x], {})
        want = want[0] if isinstance(want, tuple) else want
        model.eval()
        raw = model([x], {})
        raw = raw[0] if isinstance(raw, tuple) else raw
        with av.average_weights() as inside:
            assert inside is av and same(model.flat.data, e) and same(av.buf, w)
            assert same(model.cls_token.data, model.flat.view(e, "cls_token"))      # the parameter views show the average
            got = model([x], {})
            got = got[0] if isinstance(got, tuple) else got
            assert same(av.state_dict()["model_state"]["cls_token"], model.flat.view(e, "cls_token"))
            model.train()
            with pytest.raises(RuntimeError, match="the weights hold their moving average"):
                opt.step()
            with pytest.raises(RuntimeError, match="the weights hold their moving average"):
                step([x], y)
            with pytest.raises(RuntimeError, match="does not nest"):
                with av.average_weights():
                    pass
            with pytest.raises(RuntimeError, match=r"reset\(\) inside average_weights\(\)"):
                av.reset()
            model.eval()
    torch.cuda.synchronize()
    assert same(got, want) and not same(got, raw)
    assert same(model.flat.data, w) and same(av.buf, e) and torch.equal(opt.dev_rec, rec)
    with torch.no_grad():
        again = model([x], {})
        again = again[0] if isinstance(again, tuple) else again
    assert same(again, raw)                             # the bf16 mirrors are the raw weights' again
    # and the step goes on where it was
    model.train()
    step([x], y)
    torch.cuda.synchronize()
    assert av.stats()["num_updates"] == 3 and not same(model.flat.data, w)


class _Recording:
    """the model, keeping what it returned (on the device)"""

    def __init__(self, model):
        self.model, self.seen = model, []

    def eval(self):
        self.model.eval()

    def __call__(self, inputs, meta):
        out = self.model(inputs, meta)
        self.seen.append((out[0] if isinstance(out, tuple) else out).detach().clone())
        return out


def test_f_eval_loops_run_on_the_average():
    """train.eval_epoch(ema=) and evaluate.perform_test(ema=) see the averaged weights, and the raw ones are back after"""
    from svit_amd import evaluate, meters, train
    cfg, model, opt, av = _trained()
    cfg.LOG_PERIOD = 10
    cfg.TRAIN.FORWARD_VIDEO_FRAMES = False
    w, e = model.flat.data.clone(), av.buf.clone()
    _, twin = build()
    twin.load_state_dict(av.state_dict()["model_state"])
    twin.eval()
    x = P.frames(2, 4, 64).cuda()
    labels = P.labels(2).cuda()
    loader = [([x], labels, None, {}), ([(x * 0.9).contiguous()], labels, None, {})]
    with torch.no_grad():
        want = []
        for inp, _, _, _ in loader:
            out = twin(inp, {})
            want.append(out[0] if isinstance(out, tuple) else out)
    rec = _Recording(model)
    train.eval_epoch(loader, rec, meters.ValMeter(len(loader), cfg), 0, cfg, ema=av)
    torch.cuda.synchronize()
    assert len(rec.seen) == 2 and all(same(a, b) for a, b in zip(rec.seen, want))
    assert same(model.flat.data, w) and same(av.buf, e) and opt._averaged is None
    # two videos x the spatial crops, two clips per batch (the same clip stands in for every view)
    crops = cfg.TEST.NUM_SPATIAL_CROPS
    ids = torch.arange(2 * crops).cuda()
    tl = [([x], labels[ids[i:i + 2] // crops], ids[i:i + 2], {}) for i in range(0, 2 * crops, 2)]
    rec = _Recording(model)
    evaluate.perform_test(tl, rec, evaluate.TestMeter(2, crops, cfg.MODEL.NUM_CLASSES, len(tl)), cfg, dedupe=False, ema=av)
    torch.cuda.synchronize()
    assert len(rec.seen) == len(tl) and all(same(got, want[0]) for got in rec.seen)
    assert same(model.flat.data, w) and same(av.buf, e)


@pytest.mark.parametrize("method", ["sgd", "adamw"])
def test_g_checkpoint_round_trip(tmp_path, method):
    """the average and its count survive a resume -- SGD's own counter restarts at 1, the average's does not --, a file
    without the key makes the average start over, use_ema=True puts the average into the model"""
    from svit_amd import checkpoint
    x, y = batch()

    def one_step(model, opt):
        fwd_bwd(model, x, y)
        opt.step()
        torch.cuda.synchronize()

    cfg, model, opt, av = _trained(method, steps=3, warmup=True)
    path = checkpoint.save_checkpoint(str(tmp_path), model, opt, 3, cfg, ema=av)
    ck = torch.load(path, map_location="cpu", weights_only=False)
    assert list(ck) == ["epoch", "model_state", "optimizer_state", "cfg", "scaler_state", "ema_state"]
    assert list(ck["ema_state"]) == ["decay", "warmup", "num_updates", "model_state"]
    assert (ck["ema_state"]["decay"], ck["ema_state"]["warmup"], ck["ema_state"]["num_updates"]) == (DECAY, True, 3)
    assert list(ck["ema_state"]["model_state"]) == list(ck["model_state"]) and len(ck["model_state"]) == 405
    assert all(a.shape == b.shape and not a.is_cuda for a, b in zip(ck["ema_state"]["model_state"].values(),
                                                                     ck["model_state"].values()))
    cfg2, model2, opt2, av2 = make(method, warmup=True)
    model2.flat.data.zero_()
    assert checkpoint.load_checkpoint(path, model2, data_parallel=False, optimizer=opt2, ema=av2) == 3
    assert same(model2.flat.data, model.flat.data) and same(av2.buf, av.buf)
    assert opt2.step_count == (1 if method == "sgd" else 3)
    assert av2.stats() == av.stats() == {"num_updates": 3, "decay": float(np.float32(4.0 / 13.0))}
    one_step(model, opt)
    one_step(model2, opt2)
    assert same(model2.flat.data, model.flat.data)
    assert same(av2.buf, av.buf), "the update after the reload took another decay"
    assert av2.stats() == av.stats() == {"num_updates": 4, "decay": float(np.float32(5.0 / 14.0))}
    # a file without the key (written without ema=): the average starts over from the loaded weights
    plain = checkpoint.save_checkpoint(str(tmp_path / "plain"), model, opt, 4, cfg)
    assert "ema_state" not in torch.load(plain, map_location="cpu", weights_only=False)
    assert checkpoint.load_checkpoint(plain, model2, data_parallel=False, optimizer=opt2, ema=av2) == 4
    assert same(av2.buf, model2.flat.data) and same(model2.flat.data, model.flat.data) and av2.stats()["num_updates"] == 0
    with pytest.raises(KeyError) as refused:
        checkpoint.load_checkpoint(plain, model2, data_parallel=False, use_ema=True)
    assert refused.value.args[0].startswith("use_ema=True: '%s' holds no \"ema_state\"" % plain)      # names the file
    # use_ema: the model takes the averaged weights
    _, model3 = build()
    assert checkpoint.load_checkpoint(path, model3, data_parallel=False, use_ema=True) == 3
    assert all(same(model3.flat.p(k), v.cuda()) for k, v in ck["ema_state"]["model_state"].items())
    assert not same(model3.flat.data, ck_flat(model3, ck["model_state"]))


def ck_flat(model, state):
    """a checkpoint's model_state laid out as the model's flat buffer"""
    out = torch.zeros_like(model.flat.data)
    for k, v in state.items():
        model.flat.view(out, k).copy_(v)
    return out


def test_h_without_the_key_the_launches_are_the_parents(monkeypatch):
    """no SVIT.EMA_DECAY: build_ema gives None and a capture issues the body of a capture without an optimizer, then the
    guard and the plain guarded AdamW -- nothing of the average, no table, no buffer"""
    from svit_amd import ema, optim
    from svit_amd.graph import GraphedTrainStep
    x, y = batch()
    cfg, ma = build()
    _, mb = build()
    s = cfg.SOLVER
    s.BASE_LR, s.WEIGHT_DECAY, s.CLIP_GRAD_L2NORM = 1e-3, 0.05, 1.0
    cfg.SVIT.GUARDED_STEP = True
    opt = optim.construct_optimizer(ma, cfg)
    assert type(opt) is optim.GuardedClipAdamW and ema.build_ema(cfg, ma, opt) is None and opt.ema is None
    _, bare = _trace_names(monkeypatch, lambda: GraphedTrainStep(mb, ce, [x], y))
    step, names = _trace_names(monkeypatch, lambda: GraphedTrainStep(ma, ce, [x], y, optimizer=opt))
    assert _tail(bare) == [] and _tail(names) == ["svit_step_guard", "svit_adamw_step_guarded"]
    assert [n for n in names if n not in _tail(names)] == bare
    _, eager = _trace_names(monkeypatch, opt.step)
    assert eager == ["svit_step_guard", "svit_adamw_step_guarded"]
    assert list(opt.state_dict()) == ["state", "param_groups"]
