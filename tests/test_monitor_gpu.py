"""Per-tensor statistics on the guarded tail, on the GPU: svit_tensor_stats against its NumPy float64 restatement
(monitor.stats_host) on a synthetic buffer, and the monitor carried through the optimizers -- the eager, the captured and
the accumulated step, a frozen cut, an attached EMA.  Sums of squares inside 2^-30 relative (tests/monitor_cases.py),
everything else and every run-to-run comparison bit for bit.  Needs a real MI355X."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import procedural as P
from oracle import svit_ref as R
from tests import monitor_cases as M

DEV = "cuda"
NAN = float("nan")
CANARY = 0xA5
PAD = 256               # canary bytes on either side of a buffer


def bits(t):
    return t.contiguous().view(torch.int32)


def same(a, b):
    return torch.equal(bits(a), bits(b))


# ===================================================================================================== kernel ====
def guarded(nbytes, fill=CANARY):
    """(whole, inner): a uint8 buffer with PAD canary bytes on either side of `inner`"""
    whole = torch.full((PAD + nbytes + PAD,), fill, dtype=torch.uint8, device=DEV)
    return whole, whole[PAD:PAD + nbytes]


class Rig:
    """the synthetic buffer of tests/monitor_cases.py on the device, with the guard's record, the table, the ring and the
    workspace, the last three between canaries"""

    def __init__(self, R=4, every=1, segs=None, special=False):
        from svit_amd import monitor, ops
        self.W = ops.tensor_stats_window()
        self.table, self.n, self.where = M.layout(self.W)
        g, p = M.buffers(self.n)
        M.poison_gap(g, p, self.where)
        self.bad = M.special_values(g, self.table, self.where, self.W) if special else {}
        self.g, self.p = torch.from_numpy(g).to(DEV), torch.from_numpy(p).to(DEV)
        self.R, self.every, self.Tn = R, every, len(self.table)
        self.segs = None if segs is None else np.ascontiguousarray(np.array(segs, dtype=np.int64))
        self.rec = torch.zeros(12, dtype=torch.int32, device=DEV)
        self.ring_all, self.ring = guarded(R * (16 + 32 * self.Tn))
        self.ring.copy_(torch.from_numpy(monitor.empty_ring(R, self.Tn).view(np.uint8).reshape(-1).copy()))
        self.ws_all, self.ws = guarded(ops.tensor_stats_workspace(self.n, self.Tn))
        self.table_all, t = guarded(16 * self.Tn)
        self.table_dev = t.view(torch.int64).view(self.Tn, 2)
        self.table_dev.copy_(torch.from_numpy(self.table))
        self.table_bytes = self.table_all.cpu().numpy().copy()
        self.step = None

    def set(self, step, apply=1, skipped=0):
        """the record the guard leaves behind step `step` (counted from 0)"""
        self.step = step
        r = self.rec.view(torch.int64)
        r[0:1].fill_(step + 1 - skipped)
        r[1:2].fill_(skipped)
        self.rec[5:6].fill_(apply)

    def launch(self):
        from svit_amd import ops
        g0, p0, rec0 = self.g.clone(), self.p.clone(), self.rec.clone()
        ops.tensor_stats(self.g, self.p, self.table_dev, self.table, self.segs, self.rec, self.ring, self.R, self.every,
                         self.ws)
        torch.cuda.synchronize()
        assert same(self.g, g0) and same(self.p, p0) and torch.equal(self.rec, rec0), "g, p or the record was written"
        for name, whole in (("ring", self.ring_all), ("workspace", self.ws_all), ("table", self.table_all)):
            edge = torch.cat([whole[:PAD], whole[-PAD:]])
            assert bool((edge == CANARY).all()), "a canary beside the %s was overwritten" % name
        assert self.table_all.cpu().numpy().tobytes() == self.table_bytes.tobytes(), "the table was written"

    def rows(self):
        from svit_amd import monitor
        return self.ring.cpu().numpy().view(monitor.row_dtype(self.Tn)).copy()

    def host(self):
        from svit_amd import monitor
        return monitor.stats_host(self.g.cpu().numpy(), self.p.cpu().numpy(), self.table, self.segs)


def _empty_row(Tn):
    from svit_amd import monitor
    return monitor.empty_ring(1, Tn)[0]


def test_a_kernel_is_the_yardstick():
    """plain values: every tensor of the layout (sizes 1 .. 3 W + 5, 70 inside one window, a boundary on a window edge, an
    end at n with n % 4 = 1) against stats_host; the NaN in the gap is not counted; the other rows stay empty"""
    r = Rig()
    assert r.n % 4 == 1 and r.Tn == 80
    r.set(step=0)
    r.launch()
    rows = r.rows()
    assert rows[0]["head"].tolist() == (0, 1, 0)
    M.assert_entries(rows[0]["entry"], r.host(), "plain")
    assert (rows[0]["entry"]["n_bad"] == 0).all() and (rows[0]["entry"]["sumsq_g"] > 0).all()
    for k in (1, 2, 3):
        assert rows[k].tobytes() == _empty_row(r.Tn).tobytes(), k
    # a second run from the same state: bit for bit
    r.launch()
    assert r.rows().tobytes() == rows.tobytes()


def test_a_special_values_and_first_bad():
    """NaN, +inf, -inf, 1e30 and a denormal inside tensors; first_bad on a tensor's first and last element, on either side
    of a window edge and as the smaller of two in different windows"""
    r = Rig(special=True)
    r.set(step=5)
    r.launch()
    rows = r.rows()
    assert rows[5 % 4]["head"].tolist() == (5, 1, 0)
    e, want = rows[1]["entry"], r.host()
    M.assert_entries(e, want, "special")
    found = {int(t): (int(e["n_bad"][t]), int(e["first_bad"][t])) for t in np.flatnonzero(e["n_bad"] > 0)}
    assert found == r.bad and (e["first_bad"][e["n_bad"] == 0] == -1).all()
    t96 = r.where["size 96"]
    assert np.isfinite(e["sumsq_g"][t96]) and e["sumsq_g"][t96] > 9.9e59 and e["absmax_g"][t96] == np.float32(1e30)
    g32 = r.g[r.table[t96][0]:r.table[t96][1]]
    assert not bool(torch.isfinite((g32 * g32).sum()))          # where the guard's fp32 sum overflows
    t3 = r.where["size 3"]
    assert e["sumsq_g"][t3] > 0 and e["absmax_g"][t3] >= M.DENORMAL
    # a tensor that holds nothing but a denormal: the maximum is its bits
    lone = Rig()
    a = int(lone.table[lone.where["size 1"]][0])
    lone.g[a] = float(M.DENORMAL)
    lone.set(step=0)
    lone.launch()
    got = lone.rows()[0]["entry"][lone.where["size 1"]]
    assert got["absmax_g"].tobytes() == M.DENORMAL.tobytes() and got["n_bad"] == 0
    M.assert_entries(lone.rows()[0]["entry"], lone.host(), "lone denormal")


def test_b_every_3_records_steps_0_3_6_and_the_dropped_4():
    r = Rig(R=8, every=3)
    skipped, host = 0, {}
    for step in range(7):
        r.g.mul_(1.25)                                  # another gradient every step
        drop = step == 4
        if drop:
            r.g[int(r.table[r.where["W"]][0]) + 7] = NAN
            skipped = 1
        r.set(step, apply=0 if drop else 1, skipped=skipped)
        before = r.rows()
        r.launch()
        after = r.rows()
        if step in (0, 3, 4, 6):
            host[step] = r.host()
            assert after[step]["head"].tolist() == (step, 0 if drop else 1, 0), step
            for k in range(8):
                if k != step:
                    assert after[k].tobytes() == before[k].tobytes(), (step, k)
        else:
            assert after.tobytes() == before.tobytes(), step
        if drop:
            r.g[int(r.table[r.where["W"]][0]) + 7] = 0.5
    rows = r.rows()
    assert rows["head"]["step"].tolist() == [0, -1, -1, 3, 4, -1, 6, -1]
    for step, want in host.items():
        M.assert_entries(rows[step]["entry"], want, "step %d" % step)
    t = r.where["W"]
    assert (rows[4]["entry"]["n_bad"][t], rows[4]["entry"]["first_bad"][t]) == (1, 7) and rows[4]["entry"]["n_bad"].sum() == 1
    for k in (1, 2, 5, 7):
        assert rows[k].tobytes() == _empty_row(r.Tn).tobytes(), k


def test_b_a_dropped_step_is_recorded_whatever_every_says():
    r = Rig(R=2, every=1000)
    r.set(step=1, apply=0, skipped=2)
    r.launch()
    rows = r.rows()
    assert rows[1]["head"].tolist() == (1, 0, 0) and rows[0].tobytes() == _empty_row(r.Tn).tobytes()
    M.assert_entries(rows[1]["entry"], r.host(), "dropped")
    # ... an applied step that is not due is not; neither is a record the guard has not touched (step -1)
    for kw in (dict(step=3), dict(step=-1)):
        before = r.rows()
        r.set(**kw)
        r.launch()
        assert r.rows().tobytes() == before.tobytes(), kw


def test_c_two_segments_leave_tensors_out():
    """the tensors outside both segments are frozen: their entries keep what the host wrote (a marker here), the NaN and
    infinities in their gradients are not reported"""
    W = 4096
    r = Rig(special=True, segs=[[0, 108], [2 * W, 4 * W + 4]])
    assert r.W == W
    from svit_amd import monitor
    live = monitor.trainable_mask(r.table, r.segs)
    assert live.sum() == 6 and live[[r.where[k] for k in ("size 1", "size 3", "size 4", "size 96", "W", "W + 1")]].all()
    ring = r.rows()
    ring["entry"]["sumsq_g"][:, ~live] = 123.0
    ring["entry"]["absmax_g"][:, ~live] = 7.0
    r.ring.copy_(torch.from_numpy(ring.view(np.uint8).reshape(-1)))
    marked = r.rows()
    r.set(step=2)
    r.launch()
    rows = r.rows()
    want = r.host()
    assert rows[2]["head"].tolist() == (2, 1, 0)
    M.assert_entries(rows[2]["entry"][live], want[live], "two segments")
    assert rows[2]["entry"][~live].tobytes() == marked[2]["entry"][~live].tobytes()
    assert (want["n_bad"][~live] == -1).all() and (rows[2]["entry"]["n_bad"][~live] == -1).all()
    found = {int(t) for t in np.flatnonzero(rows[2]["entry"]["n_bad"] > 0)}
    assert found == {r.where["W"], r.where["W + 1"]}                    # not "to the edge", not "3 W + 5"
    for k in (0, 1, 3):
        assert rows[k].tobytes() == marked[k].tobytes(), k


def test_c_ring_of_two_rows_overrun_by_one_step():
    r = Rig(R=2)
    host = {}
    for step in range(3):
        r.g.mul_(0.5)
        r.set(step)
        r.launch()
        host[step] = r.host()
    rows = r.rows()
    assert rows["head"]["step"].tolist() == [2, 1] and rows["head"]["apply"].tolist() == [1, 1]
    M.assert_entries(rows[0]["entry"], host[2], "step 2")
    M.assert_entries(rows[1]["entry"], host[1], "step 1")
    assert rows[0]["entry"]["sumsq_g"].tobytes() != rows[1]["entry"]["sumsq_g"].tobytes()


def test_c_wrapper_refuses_before_any_launch():
    from svit_amd import hip, ops
    r = Rig()
    r.set(step=0)
    before = r.rows()
    args = dict(g=r.g, p=r.p, table_dev=r.table_dev, table_host=r.table, segs=None, dev_rec=r.rec, ring=r.ring, R=r.R,
                every=1, workspace=r.ws)
    cases = {
        "a ring of another size": dict(ring=r.ring[:-16]),
        "a host tensor": dict(g=r.g.cpu()),
        "a device table of another shape": dict(table_dev=r.table_dev[:-1]),
        "a record of floats": dict(dev_rec=r.rec.float()),
        "p of another size": dict(p=r.p[:-1].clone()),
        "a short workspace": dict(workspace=r.ws[:-32]),
        "every = 0": dict(every=0),
        "a misaligned g": dict(g=r.g[1:], p=r.p[1:], table_host=np.ascontiguousarray(r.table[:-1])),
    }
    for label, kw in cases.items():
        a = dict(args, **kw)
        if label == "a misaligned g":
            a["table_dev"] = r.table_dev[:-1].clone()
            a["ring"] = torch.zeros(r.R * (16 + 32 * (r.Tn - 1)), dtype=torch.uint8, device=DEV)
        with pytest.raises(hip.SvitHipError):
            ops.tensor_stats(**a)
        torch.cuda.synchronize()
        assert r.rows().tobytes() == before.tobytes(), label


# ======================================================================================================= model ====
LR = {"sgd": 0.05, "adam": 1e-3, "adamw": 1e-3}
CULPRIT = "blocks.3.attn.rel_pos_h"


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


def make(method, mode="deterministic", cut=0, monitor=True, period=4, every=1, ema=False, max_skips=None):
    from svit_amd import ema as ema_mod
    from svit_amd import monitor as mon_mod
    from svit_amd import optim
    cfg, model = build(mode)
    if cut:
        model.freeze_below(cut)
    s = cfg.SOLVER
    s.OPTIMIZING_METHOD, s.BASE_LR, s.WEIGHT_DECAY, s.CLIP_GRAD_L2NORM = method, LR[method], 1e-4, 1.0
    s.MOMENTUM, s.DAMPENING, s.NESTEROV = 0.9, 0.0, True
    cfg.LOG_PERIOD = period
    cfg.SVIT.GUARDED_STEP = True
    if monitor:
        cfg.SVIT.MONITOR = True
        cfg.SVIT.MONITOR_EVERY = every
    if ema:
        cfg.SVIT.EMA_DECAY = 0.9
    if max_skips is not None:
        cfg.SVIT.MAX_CONSECUTIVE_SKIPS = max_skips
    opt = optim.construct_optimizer(model, cfg)
    av = ema_mod.build_ema(cfg, model, opt)
    mon = mon_mod.build_monitor(cfg, opt)
    assert isinstance(opt, optim.GuardedClipAdamW) and opt.monitor is mon and (mon is not None) == monitor
    return cfg, model, opt, mon, av


def snapshot(model):
    """the gradient and the weights the next optimizer step will see, on the host"""
    torch.cuda.synchronize()
    return model.flat.grad.cpu().numpy().copy(), model.flat.data.cpu().numpy().copy()


def check_rows(mon, rows, seen, what):
    """every row against stats_host on the (g, p) of its step"""
    from svit_amd import monitor
    assert len(rows["steps"]) > 0
    for i, step in enumerate(rows["steps"].tolist()):
        g, p = seen[step]
        want = monitor.stats_host(g, p, mon.table, mon.segments)
        live = ~mon.frozen
        for key in ("sumsq_g", "sumsq_p"):
            k, h = rows[key].data[i][live], want[key][live]
            assert (np.abs(k - h) <= M.BAR * h).all(), (what, step, key)
        for key, src in (("absmax", "absmax_g"), ("n_bad", "n_bad"), ("first_bad", "first_bad")):
            assert rows[key].data[i].tobytes() == want[src].tobytes(), (what, step, key)
        assert np.array_equal(rows["grad_norm"].data[i], np.sqrt(rows["sumsq_g"].data[i]) * mon.optimizer.grad_scale)
        assert np.array_equal(np.ma.getmaskarray(rows["grad_norm"])[i], mon.frozen)


@pytest.mark.parametrize("method", ["adamw", "adam", "sgd"])
def test_d_three_steps_through_construct_optimizer(method):
    """(on the parent commit there is no svit_amd.monitor)"""
    from svit_amd import optim
    x, y = batch()
    cfg, model, opt, mon, _ = make(method)
    assert type(opt) is {"adamw": optim.GuardedClipAdamW, "adam": optim.GuardedClipAdam, "sgd": optim.GuardedClipSGD}[method]
    assert len(mon.names) == 405 and mon.period == 4 and not mon.frozen.any()
    seen = {}
    for i in range(3):
        optim.set_lr(opt, LR[method] * (i + 1))
        fwd_bwd(model, x, y)
        seen[i] = snapshot(model)
        opt.step()
    torch.cuda.synchronize()
    rows = mon.read()
    assert rows["steps"].tolist() == [0, 1, 2] and rows["applied"].tolist() == [True] * 3 and rows["lost"] == 0
    check_rows(mon, rows, seen, method)
    assert not np.array_equal(rows["sumsq_p"].data[0], rows["sumsq_p"].data[2])         # the weights moved
    assert (rows["n_bad"].data == 0).all() and mon.culprits(rows) == []
    layers = mon.by_layer(rows)
    assert layers["ratio"].shape == (3, cfg.MVIT.DEPTH + 2) and bool((layers["ratio"] > 0).all())
    again = mon.read()
    assert again["steps"].tolist() == [] and again["lost"] == 0
    assert mon.log_stats(rows)["step"] == 2 and mon.log_stats(again) is None


def test_d_a_nan_is_located_and_the_step_is_the_unwatched_one():
    """one NaN in blocks.3.attn.rel_pos_h's gradient in step 2: dropped, named with its index by culprits() and by
    check(); weights and moments are those of an optimizer without a monitor, bit for bit"""
    x, y = batch()
    _, mw, ow, mon, _ = make("adamw", max_skips=1)
    _, mb, ob, none, _ = make("adamw", monitor=False, max_skips=1)
    assert none is None and ob.monitor is None
    shape = mon.shapes[mon.names.index(CULPRIT)]
    idx = (min(2, shape[0] - 1), 5)
    for i in range(3):
        for model, opt in ((mw, ow), (mb, ob)):
            fwd_bwd(model, x, y)
            if i == 1:
                model.flat.view(model.flat.grad, CULPRIT)[idx] = NAN
            opt.step()
        torch.cuda.synchronize()
        if i == 1:
            assert ow.stats()["skipped"] == 1 and ob.stats()["skipped"] == 1
            with pytest.raises(RuntimeError) as told:
                ow.check()
            with pytest.raises(RuntimeError) as bare:
                ob.check()
            head, line = str(told.value).split("\n")
            assert head == str(bare.value) and "\n" not in str(bare.value)
            assert line == "non-finite gradients of step 1 in 1 tensor: %s (1 non-finite, the first at %s)" % (CULPRIT, list(idx))
        else:
            ow.check()
    rows = mon.read()
    assert rows["steps"].tolist() == [0, 1, 2] and rows["applied"].tolist() == [True, False, True]
    assert mon.culprits(rows) == [(1, CULPRIT, 1, idx)]
    assert int(rows["n_bad"].data.sum()) == 1
    assert mon.log_stats(rows)["culprits"] == [[1, CULPRIT, 1, list(idx)]]
    for name, a, b in [("weights", mw.flat.data, mb.flat.data)] + [(k, getattr(ow, k), getattr(ob, k)) for k in ow.STATE]:
        assert same(a, b), name
    assert ow.stats() == ob.stats() and list(ow.state_dict()) == list(ob.state_dict())


def test_d_cut_4_and_a_ring_of_two_rows():
    """a frozen cut at 4: the frozen tensors come back masked and untouched; period 2 overrun by one step is reported"""
    x, y = batch()
    cfg, model, opt, mon, _ = make("adamw", cut=4, period=2)
    assert opt.cut == 4 and mon.segments is opt.segments and 0 < int(mon.frozen.sum()) < 405
    seen = {}
    for i in range(3):
        fwd_bwd(model, x, y)
        if i == 2:      # a NaN in a frozen tensor's gradient is neither seen by the guard nor reported
            t = int(np.flatnonzero(mon.frozen)[0])
            model.flat.grad[int(mon.table[t][0])] = NAN
        seen[i] = snapshot(model)
        opt.step()
    torch.cuda.synchronize()
    assert opt.stats()["applied"] == 3
    rows = mon.read()
    assert rows["steps"].tolist() == [1, 2] and rows["lost"] == 1
    check_rows(mon, rows, seen, "cut 4")
    assert (rows["n_bad"].data[:, mon.frozen] == -1).all() and (rows["n_bad"].data[:, ~mon.frozen] == 0).all()
    assert bool(np.ma.getmaskarray(rows["weight_norm"])[:, mon.frozen].all())
    layers = mon.by_layer(rows)
    masked = np.ma.getmaskarray(layers["grad_norm"])[0]
    assert masked[0] and not masked[-1] and 0 < masked.sum() < len(masked)          # the stem's group is all frozen


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
    return [n for n in names if n.startswith(("svit_step_guard", "svit_adamw_step", "svit_sgd_", "svit_adam_", "svit_ema_",
                                              "svit_tensor_"))]


def _ring(mon):
    torch.cuda.synchronize()
    return mon.ring.cpu().numpy().tobytes()


def test_e_graphed_step_replays_the_monitor(monkeypatch):
    """the captured step over a poisoned first replay and three more with lr changes equals the eager step in the rows,
    the weights and the moments; a replay after the attached monitor changed is refused"""
    from svit_amd import hip, optim
    from svit_amd.graph import GraphedTrainStep
    poison = torch.ones(1, device=DEV)

    def loss_fun(p, e, y):
        return torch.nn.functional.cross_entropy(p, y) * poison

    x, y = batch()
    _, mg, og, ng, _ = make("adamw", period=8)
    _, me, oe, ne, _ = make("adamw", period=8)
    empty = _ring(ng)
    step, names = _trace_names(monkeypatch, lambda: GraphedTrainStep(mg, loss_fun, [x], y, optimizer=og))
    assert _tail(names) == ["svit_step_guard", "svit_tensor_stats", "svit_adamw_step_guarded"]
    assert names[-2:] == ["svit_tensor_stats", "svit_adamw_step_guarded"]
    assert _ring(ng) == empty and og.stats()["applied"] == 0                 # building recorded nothing

    def eager():
        oe.zero_grad()
        logits, extra = me([x], {})
        loss = loss_fun(logits, extra, y)
        loss.backward()
        oe.step()
        return loss.detach()

    def compare(what):
        torch.cuda.synchronize()
        for name, a, b in [("weights", mg.flat.data, me.flat.data)] + [(k, getattr(og, k), getattr(oe, k)) for k in og.STATE]:
            assert same(a, b), (what, name)
        assert og.stats() == oe.stats() and _ring(ng) == _ring(ne), what

    poison.fill_(NAN)
    step([x], y)
    eager()
    compare("poisoned step")
    poison.fill_(1.0)
    seen = {}
    for i in range(3):
        optim.set_lr(og, LR["adamw"] * (i + 1))
        optim.set_lr(oe, LR["adamw"] * (i + 1))
        p_before = mg.flat.data.cpu().numpy().copy()
        lg, _ = step([x], y)
        le = eager()
        assert same(lg, le)
        compare("step %d" % (i + 1))
        seen[i + 1] = (mg.flat.grad.cpu().numpy().copy(), p_before)       # (the step leaves the gradient where it was)
    rows = ng.read()
    assert rows["steps"].tolist() == [0, 1, 2, 3] and rows["applied"].tolist() == [False, True, True, True]
    assert int((rows["n_bad"].data[0] > 0).sum()) > 100 and len(ng.culprits(rows)) == int((rows["n_bad"].data[0] > 0).sum())
    poisoned = {k: v for k, v in rows.items()}
    for key in ("steps", "applied", "sumsq_g", "sumsq_p", "grad_norm", "weight_norm", "absmax", "n_bad", "first_bad"):
        poisoned[key] = rows[key][1:]
    check_rows(ng, poisoned, seen, "replay")
    # the capture holds the launches of the monitor attached THEN
    og.attach_monitor(None)
    with pytest.raises(hip.SvitHipError, match="attached TensorMonitor changed after this GraphedTrainStep was built"):
        step([x], y)
    og.attach_monitor(ng)
    step([x], y)
    torch.cuda.synchronize()
    assert ng.read()["steps"].tolist() == [4]


def test_e_accumulated_step_k2_reproducible(monkeypatch):
    """AccumulatedTrainStep(k = 2) under SVIT.REPRODUCIBLE: ONE pair of monitor launches per call, the rows are those of
    the summed gradient and equal the eager micro-steps + optimizer.step() on a second model bit for bit"""
    from svit_amd import hip, optim, train
    from svit_amd.graph import AccumulatedTrainStep, GraphedTrainStep
    A, B, C = batch(), batch("B"), batch("C")
    _, mg, og, ng, _ = make("sgd", mode="reproducible")
    _, me, oe, ne, _ = make("sgd", mode="reproducible")
    micro = GraphedTrainStep(mg, ce, [A[0]], A[1], accumulate=True)
    step = AccumulatedTrainStep(mg, [micro, micro], og)
    seen = {}
    for i, batches in enumerate(([A, B], [C, A], [B, C])):
        optim.set_lr(og, LR["sgd"] * (i + 1))
        optim.set_lr(oe, LR["sgd"] * (i + 1))
        batches = [([x], y) for x, y in batches]
        p_before = mg.flat.data.cpu().numpy().copy()
        _, names = _trace_names(monkeypatch, lambda: step(batches))
        assert names.count("svit_tensor_stats") == 1
        assert _tail(names) == ["svit_step_guard", "svit_tensor_stats", "svit_sgd_step_guarded"]
        train.accumulate_step(me, [ce, ce], batches, oe)
        torch.cuda.synchronize()
        assert same(mg.flat.data, me.flat.data) and same(og.momentum_buffer, oe.momentum_buffer) and _ring(ng) == _ring(ne)
        seen[i] = (mg.flat.grad.cpu().numpy().copy(), p_before)            # the gradient summed over the two micro-steps
    rows = ng.read()
    assert rows["steps"].tolist() == [0, 1, 2] and rows["lost"] == 0
    check_rows(ng, rows, seen, "accumulated")
    og.attach_monitor(None)
    with pytest.raises(hip.SvitHipError, match="attached TensorMonitor changed after this AccumulatedTrainStep was built"):
        step(batches)


def test_f_with_an_ema_attached_as_well(monkeypatch):
    """guard, the monitor's two launches, the solver's, the average's; the average is the one of a step without a monitor"""
    from svit_amd import optim
    x, y = batch()
    _, mw, ow, mon, aw = make("adam", ema=True)
    _, mb, ob, _, ab = make("adam", ema=True, monitor=False)
    assert aw is not None and ow.ema is aw and ob.monitor is None
    seen = {}
    for i in range(2):
        fwd_bwd(mw, x, y)
        fwd_bwd(mb, x, y)
        seen[i] = snapshot(mw)
        _, names = _trace_names(monkeypatch, ow.step)
        assert names == ["svit_step_guard", "svit_tensor_stats", "svit_adam_step_guarded", "svit_ema_step_guarded"]
        ob.step()
    torch.cuda.synchronize()
    assert same(aw.buf, ab.buf) and same(mw.flat.data, mb.flat.data) and not same(aw.buf, mw.flat.data)
    rows = mon.read()
    assert rows["steps"].tolist() == [0, 1]
    check_rows(mon, rows, seen, "with an EMA")


def test_h_without_the_key_the_launches_are_the_parents(monkeypatch):
    """no SVIT.MONITOR: build_monitor gives None and a capture issues the body of a capture without an optimizer, then the
    guard and the plain guarded AdamW -- nothing of the monitor, no ring, no table"""
    from svit_amd.graph import GraphedTrainStep
    x, y = batch()
    cfg, ma, opt, mon, _ = make("adamw", monitor=False)
    _, mb = build()
    assert mon is None and opt.monitor is None
    _, bare = _trace_names(monkeypatch, lambda: GraphedTrainStep(mb, ce, [x], y))
    step, names = _trace_names(monkeypatch, lambda: GraphedTrainStep(ma, ce, [x], y, optimizer=opt))
    assert _tail(bare) == [] and _tail(names) == ["svit_step_guard", "svit_adamw_step_guarded"]
    assert [n for n in names if n not in _tail(names)] == bare
    _, eager = _trace_names(monkeypatch, opt.step)
    assert eager == ["svit_step_guard", "svit_adamw_step_guarded"]
    assert list(opt.state_dict()) == ["state", "param_groups"]
