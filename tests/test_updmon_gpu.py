"""The update monitor on the GPU: svit_update_snapshot and svit_update_stats against their NumPy float64 restatement
(updmon.update_host) on the synthetic buffer of tests/monitor_cases.py, the stall of fp32 weights under a tiny learning rate
end to end, and the monitor carried through the optimizers -- the eager, the captured and the accumulated step, a frozen
cut, learning-rate scales, a TensorMonitor and an EMA beside it.  The six sums inside 2^-29 * sum |term|
(tests/update_cases.py), everything else and every run-to-run comparison bit for bit.  Needs a real MI355X."""
import types

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import procedural as P
from oracle import svit_ref as R
from tests import monitor_cases as M
from tests import update_cases as U

DEV = "cuda"
NAN = float("nan")
CANARY = 0xA5
PAD = 256               # canary bytes on either side of a buffer
W = 4096


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
    """the synthetic buffer of tests/monitor_cases.py on the device: the weights in front of the step (`old`), behind it
    (`p`), g, m, v, the guard's record, and the shadow, the ring, the workspace and the table between canaries; NaN in p
    and g in the 8-element gap"""

    def __init__(self, R=4, every=1, segs=None, flags=3):
        from svit_amd import ops, updmon
        assert ops.tensor_stats_window() == W
        self.table, self.n, self.where = M.layout(W)
        old, g, m, v = U.buffers(self.n)
        new, self.expect = U.perturb(old, self.table, self.where, W)
        a, b = self.where["gap"]
        for x in (old, new, g):
            x[a:b] = np.nan
        self.old, self.p, self.g = (torch.from_numpy(x).to(DEV) for x in (old, new, g))
        self.m = torch.from_numpy(m).to(DEV) if flags & 1 else None
        self.v = torch.from_numpy(v).to(DEV) if flags & 2 else None
        self.R, self.every, self.Tn = R, every, len(self.table)
        self.segs = None if segs is None else np.ascontiguousarray(np.array(segs, dtype=np.int64))
        self.rec = torch.zeros(12, dtype=torch.int32, device=DEV)
        self.ring_all, self.ring = guarded(R * (16 + 64 * self.Tn))
        self.ring.copy_(torch.from_numpy(updmon.empty_ring(R, self.Tn).view(np.uint8).reshape(-1).copy()))
        self.ws_all, self.ws = guarded(ops.update_stats_workspace(self.n, self.Tn))
        self.table_all, t = guarded(16 * self.Tn)
        self.table_dev = t.view(torch.int64).view(self.Tn, 2)
        self.table_dev.copy_(torch.from_numpy(self.table))
        self.table_bytes = self.table_all.cpu().numpy().copy()
        self.shadow_all, s = guarded(4 * self.n, fill=0x5A)
        self.shadow = s.view(torch.float32)

    def set(self, step, apply=1, skipped=0):
        """the record the guard leaves behind step `step` (counted from 0)"""
        r = self.rec.view(torch.int64)
        r[0:1].fill_(step + 1 - skipped)
        r[1:2].fill_(skipped)
        self.rec[5:6].fill_(apply)

    def canaries(self):
        for name, whole, fill in (("ring", self.ring_all, CANARY), ("workspace", self.ws_all, CANARY),
                                  ("table", self.table_all, CANARY), ("shadow", self.shadow_all, 0x5A)):
            edge = torch.cat([whole[:PAD], whole[-PAD:]])
            assert bool((edge == fill).all()), "a canary beside the %s was overwritten" % name
        assert self.table_all.cpu().numpy().tobytes() == self.table_bytes.tobytes(), "the table was written"

    def snapshot(self, src=None):
        """svit_update_snapshot of `src` (the weights in front of the step)"""
        from svit_amd import ops
        src = self.old if src is None else src
        before, rec0 = src.clone(), self.rec.clone()
        ops.update_snapshot(src, self.shadow, self.segs, self.rec, self.every)
        torch.cuda.synchronize()
        assert same(src, before) and torch.equal(self.rec, rec0), "p or the record was written"
        self.canaries()

    def stats(self):
        from svit_amd import ops
        ins = [x for x in (self.p, self.shadow, self.g, self.m, self.v, self.rec) if x is not None]
        before = [x.clone() for x in ins]
        ops.update_stats(self.p, self.shadow, self.g, self.m, self.v, self.table_dev, self.table, self.segs, self.rec,
                         self.ring, self.R, self.every, self.ws)
        torch.cuda.synchronize()
        for x, x0 in zip(ins, before):
            assert same(x, x0), "an input was written"
        self.canaries()

    def rows(self):
        from svit_amd import updmon
        return self.ring.cpu().numpy().view(updmon.row_dtype(self.Tn)).copy()

    def host(self, step, old=None):
        """(row, terms) of the yardstick on what the device holds"""
        from svit_amd import updmon
        args = [(self.old if old is None else old).cpu().numpy(), self.p.cpu().numpy(), self.g.cpu().numpy(),
                None if self.m is None else self.m.cpu().numpy(), None if self.v is None else self.v.cpu().numpy(),
                self.table, self.segs]
        return updmon.update_host(*args, step=step), updmon.abs_terms_host(*args)


def _empty_row(Tn):
    from svit_amd import updmon
    return updmon.empty_ring(1, Tn)[0]


def _in_segs(n, segs):
    inside = np.zeros(n, dtype=bool)
    for a, b in segs:
        inside[a:b] = True
    return inside


def test_a_snapshot_copies_the_segments_and_only_them():
    """a due step: the whole buffer (n % 4 == 1, the NaN of the gap bit for bit), two segments that cut a window (what lies
    outside keeps its bytes: the gap's NaN is not copied), 64 segments"""
    r = Rig()
    r.set(step=0)
    r.snapshot()
    assert r.n % 4 == 1 and same(r.shadow, r.old)
    cases = {"two segments cut a window": [[0, 108], [1000, W + 2000]],
             "a segment from edge to edge": [[W, 2 * W]],
             "64 segments": [[464 * k, 464 * k + 232] for k in range(64)]}
    gap = r.where["gap"]
    for label, segs in cases.items():
        r = Rig(segs=segs)
        fresh = r.shadow.clone()
        r.set(step=4)
        r.snapshot()
        inside = torch.from_numpy(_in_segs(r.n, segs)).to(DEV)
        assert same(r.shadow[inside], r.old[inside]), label
        assert same(r.shadow[~inside], fresh[~inside]), label
        if label != "64 segments":
            assert not inside[gap[0]:gap[1]].any() and not bool(torch.isnan(r.shadow).any()), label
        else:
            assert len(segs) == 64 and 7 * W < segs[-1][1] <= r.n


def test_a_snapshot_of_a_step_that_is_not_due_writes_nothing():
    for label, every, kw in (("every = 3, step 1", 3, dict(step=1)), ("every = 3, step 4, one dropped before", 3, dict(step=4, skipped=1)),
                             ("dropped", 1, dict(step=2, apply=0, skipped=1)), ("no step yet", 1, dict(step=-1)),
                             ("dropped on a multiple", 2, dict(step=2, apply=0, skipped=1))):
        for segs in (None, [[0, 108], [2 * W, 4 * W + 4]]):
            r = Rig(every=every, segs=segs)
            before = r.shadow_all.cpu().numpy().tobytes()
            r.set(**kw)
            r.snapshot()
            assert r.shadow_all.cpu().numpy().tobytes() == before, (label, segs)
    r = Rig(every=3)
    r.set(step=3, skipped=1)            # the index counts dropped steps: step 3 is due
    r.snapshot()
    assert same(r.shadow, r.old)


@pytest.mark.parametrize("flags", [3, 1, 0])
def test_b_stats_are_the_yardsticks(flags):
    """every tensor of the layout after the known perturbation, with both moments, the first alone and neither; the
    tensors laid out by hand report the counts written down beside them; a second run is bit-equal"""
    r = Rig(flags=flags)
    r.set(step=5)
    r.snapshot()
    r.stats()
    rows = r.rows()
    want, terms = r.host(step=5)
    assert rows[1]["head"].tolist() == (5, flags, 0)
    U.assert_row(rows[1], want, terms, "flags %d" % flags)
    e = rows[1]["entry"]
    for t, (still, one) in r.expect.items():
        assert (int(e["n_still"][t]), int(e["n_one_ulp"][t])) == (still, one), t
    numel = r.table[:, 1] - r.table[:, 0]
    big = numel >= 1000
    assert (e["n_still"][big] > 0.15 * numel[big]).all() and (e["n_one_ulp"][big] > 0.15 * numel[big]).all()
    assert (e["n_still"] + e["n_one_ulp"] <= numel).all() and (e["sumsq_d"][big] > 0).all()
    assert ((e["sumsq_m"] > 0) == bool(flags & 1)).all() and ((e["sum_v"] > 0) == bool(flags & 2)).all()
    t96 = r.where["size 96"]
    assert e["absmax_d"][t96] == np.float32(np.float64(np.float32(1.01)) - np.float64(np.float32(0.99)))
    for k in (0, 2, 3):
        assert rows[k].tobytes() == _empty_row(r.Tn).tobytes(), k
    r.ws.fill_(0xEE)                    # (what an earlier run left in the workspace does not matter)
    r.stats()
    assert r.rows().tobytes() == rows.tobytes()


def test_b_unchanged_elements_at_the_edges():
    """the unchanged elements U.perturb places on either side of the window edges W and 2 W, on a tensor's first and last
    element and on the buffer's last: moving one of them changes its tensor's n_still by exactly one"""
    r = Rig()
    r.set(step=0)
    r.snapshot()
    r.stats()
    base = r.rows()[0]["entry"]["n_still"].copy()
    a, b = (int(x) for x in r.table[r.where["W + 1"]])
    spots = {W - 1: "W - 1", W: "W - 1", 2 * W - 1: "to the edge", 2 * W: "W", a: "W + 1", b - 1: "W + 1", r.n - 1: "last"}
    assert b - 1 == 4 * W and r.table[r.where["W - 1"]][0] < W - 1 and r.table[r.where["W - 1"]][1] > W
    for i, name in spots.items():
        assert same(r.p[i:i + 1], r.old[i:i + 1])
        keep = r.p[i:i + 1].clone()
        r.p[i:i + 1] = r.p[i:i + 1] * 1.5
        r.stats()
        now = r.rows()[0]["entry"]["n_still"]
        t = r.where[name]
        assert now[t] == base[t] - 1 and np.array_equal(np.delete(now, t), np.delete(base, t)), (i, name)
        r.p[i:i + 1] = keep


def test_c_every_three_steps_with_a_dropped_one():
    """every = 3 over steps 0..6 with step 3 dropped: rows 0 and 6 are written, row 6 against the weights of step 6's
    own snapshot; the other rows keep their bytes"""
    r = Rig(R=8, every=3)
    empty = _empty_row(r.Tn).tobytes()
    host = {}
    for step in range(7):
        dropped = step == 3
        r.set(step, apply=0 if dropped else 1, skipped=1 if step >= 3 else 0)
        front = r.p.clone()
        r.snapshot(src=front)
        if not dropped:                 # "the solver": the weights move on an applied step
            r.p.mul_(1.0 + 2.0 ** -12)
            r.p[::3] = front[::3]
        r.stats()
        if step in (0, 6):
            assert same(r.shadow, front)
            host[step] = r.host(step, old=front)
        else:
            assert not same(r.shadow, front)
    rows = r.rows()
    assert rows["head"]["step"].tolist() == [0, -1, -1, -1, -1, -1, 6, -1]
    for step in (0, 6):
        U.assert_row(rows[step], host[step][0], host[step][1], "step %d" % step)
    for k in (1, 2, 3, 4, 5, 7):
        assert rows[k].tobytes() == empty, k
    numel = r.table[:, 1] - r.table[:, 0]
    assert (rows[6]["entry"]["n_still"] >= numel // 3).all()


def test_c_segments_leave_tensors_out():
    """the tensors outside both segments are frozen: their entries keep what the host wrote (a marker here) and
    n_still = -1; nothing of them is loaded (their shadow was never written)"""
    from svit_amd import monitor
    r = Rig(segs=[[0, 108], [2 * W, 4 * W + 4]])
    live = monitor.trainable_mask(r.table, r.segs)
    assert live.sum() == 6 and live[[r.where[k] for k in ("size 1", "size 3", "size 4", "size 96", "W", "W + 1")]].all()
    ring = r.rows()
    ring["entry"]["sumsq_d"][:, ~live] = 123.0
    ring["entry"]["absmax_d"][:, ~live] = 7.0
    r.ring.copy_(torch.from_numpy(ring.view(np.uint8).reshape(-1)))
    marked = r.rows()
    r.set(step=2)
    r.snapshot()
    r.stats()
    rows = r.rows()
    want, terms = r.host(step=2)
    assert rows[2]["head"].tolist() == (2, 3, 0)
    U.assert_row({"head": rows[2]["head"], "entry": rows[2]["entry"][live]},
                 {"head": want["head"], "entry": want["entry"][live]}, terms[live], "two segments")
    assert rows[2]["entry"][~live].tobytes() == marked[2]["entry"][~live].tobytes()
    assert (want["entry"]["n_still"][~live] == -1).all() and (rows[2]["entry"]["n_still"][~live] == -1).all()
    assert (rows[2]["entry"]["n_still"][live] >= 0).all()
    for k in (0, 1, 3):
        assert rows[k].tobytes() == marked[k].tobytes(), k


def test_c_ring_of_two_rows_overrun_by_one_step():
    r = Rig(R=2)
    host = {}
    for step in range(3):
        front = r.p.clone()
        r.set(step)
        r.snapshot(src=front)
        r.p.mul_(1.0 + 2.0 ** -(10 + step))
        r.stats()
        host[step] = r.host(step, old=front)
    rows = r.rows()
    assert rows["head"]["step"].tolist() == [2, 1] and rows["head"]["flags"].tolist() == [3, 3]
    U.assert_row(rows[0], host[2][0], host[2][1], "step 2")
    U.assert_row(rows[1], host[1][0], host[1][1], "step 1")
    assert rows[0]["entry"]["sumsq_d"].tobytes() != rows[1]["entry"]["sumsq_d"].tobytes()


def test_c_wrappers_refuse_before_any_launch():
    from svit_amd import hip, ops
    r = Rig()
    r.set(step=0)
    before, shadow = r.rows(), r.shadow.clone()
    args = dict(p=r.p, shadow=r.shadow, g=r.g, m=r.m, v=r.v, table_dev=r.table_dev, table_host=r.table, segs=None,
                dev_rec=r.rec, ring=r.ring, R=r.R, every=1, workspace=r.ws)
    cases = {"a ring of another size": dict(ring=r.ring[:-16]), "a host tensor": dict(g=r.g.cpu()),
             "a device table of another shape": dict(table_dev=r.table_dev[:-1]), "a record of floats": dict(dev_rec=r.rec.float()),
             "m of another size": dict(m=r.m[:-1].clone()), "a short workspace": dict(workspace=r.ws[:-64]),
             "every = 0": dict(every=0), "a shadow of halves": dict(shadow=r.shadow.half())}
    for label, kw in cases.items():
        with pytest.raises(hip.SvitHipError):
            ops.update_stats(**dict(args, **kw))
    for label, kw in {"every = 0": dict(every=0), "a shadow of another size": dict(shadow=r.shadow[:-1].clone()),
                      "a record of floats": dict(dev_rec=r.rec.float()), "a misaligned p": dict(p=r.p[1:], shadow=r.shadow[1:]),
                      "segments as a list": dict(segs=[[0, 8]])}.items():
        with pytest.raises(hip.SvitHipError):
            ops.update_snapshot(**dict(dict(p=r.p, shadow=r.shadow, segs=None, dev_rec=r.rec, every=1), **kw))
    torch.cuda.synchronize()
    assert r.rows().tobytes() == before.tobytes() and same(r.shadow, shadow)


# ============================================================================== the stall, on the synthetic buffer ====
class _Flat:
    """what the optimizer and the monitor touch of a model's FlatParams, over the synthetic layout"""

    def __init__(self, p, table, where):
        self.total, self.n_decay, self.n_ranks = p.numel(), int(table[where["W - 1"]][0]), 3
        self.data, self.grad = p.clone(), torch.zeros_like(p)
        names = {v: k for k, v in where.items() if k != "gap"}
        self.slots = {names[t]: (int(a), int(b - a), (int(b - a),)) for t, (a, b) in enumerate(table)}


def test_d_weights_of_one_stall_at_a_tiny_learning_rate():
    """ONE guarded AdamW step at lr = 1e-9, wd = 0, g = +-1: the tensor of weights 1.0 does not move a bit and is named by
    stalled(), the tensor of weights 0.01 moves by exactly one ulp everywhere; the whole row is the yardstick's"""
    from svit_amd import optim, updmon
    table, n, where = M.layout(W)
    rng = np.random.default_rng(3)
    p = (rng.standard_normal(n) * 0.05).astype(np.float32)
    g = np.where(rng.random(n) < 0.5, -1.0, 1.0).astype(np.float32)
    (a1, b1), (a2, b2) = table[where["W"]], table[where["W + 1"]]
    p[a1:b1] = 1.0
    p[a2:b2] = 0.01
    p[a2:b2:2] = -0.01
    flat = _Flat(torch.from_numpy(p).to(DEV), table, where)
    opt = optim.GuardedClipAdamW(types.SimpleNamespace(flat=flat), lr=1e-9, weight_decay=0.0)
    mon = updmon.UpdateMonitor(opt, period=2)
    opt.attach_update_monitor(mon)
    assert mon.names[where["W"]] == "W" and np.array_equal(mon.table, table) and not mon.frozen.any()
    flat.grad.copy_(torch.from_numpy(g))
    opt.step()
    torch.cuda.synchronize()
    assert opt.stats()["applied"] == 1 and same(mon.shadow, torch.from_numpy(p).to(DEV))
    p_new = flat.data.cpu().numpy()
    args = (p, p_new, g, opt.exp_avg.cpu().numpy(), opt.exp_avg_sq.cpu().numpy(), table, None)
    ring = mon.ring.cpu().numpy().view(updmon.row_dtype(80))
    U.assert_row(ring[0], updmon.update_host(*args, step=0), updmon.abs_terms_host(*args), "the stall")
    rows = mon.read()
    assert rows["steps"].tolist() == [0] and rows["flags"].tolist() == [3] and rows["lost"] == 0
    t1, t2 = where["W"], where["W + 1"]
    assert rows["n_still"][0, t1] == W and rows["n_one_ulp"][0, t1] == 0 and rows["update_norm"][0, t1] == 0
    assert rows["n_still"][0, t2] == 0 and rows["n_one_ulp"][0, t2] == W + 1
    assert np.array_equal(p_new[a1:b1], p[a1:b1]) and (p_new[a2:b2] != p[a2:b2]).all()
    named = mon.stalled(rows)
    assert (0, "W", W, W) in named and all(name != "W + 1" for _, name, _, _ in named)
    assert all(k >= 0.5 * m for _, _, k, m in named)
    # the first step moves every element against its gradient: the cosine is positive wherever something moved
    moved = rows["update_norm"].data[0] > 0
    assert moved.sum() >= 40 and (rows["cos_grad"].data[0][moved] > 0).all()


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


def make(method, mode="deterministic", cut=0, update=True, period=4, every=1, ema=False, monitor=False, layer_decay=None):
    from svit_amd import ema as ema_mod
    from svit_amd import monitor as mon_mod
    from svit_amd import optim, updmon
    cfg, model = build(mode)
    if cut:
        model.freeze_below(cut)
    s = cfg.SOLVER
    s.OPTIMIZING_METHOD, s.BASE_LR, s.WEIGHT_DECAY, s.CLIP_GRAD_L2NORM = method, LR[method], 1e-4, 1.0
    s.MOMENTUM, s.DAMPENING, s.NESTEROV = 0.9, 0.0, True
    if layer_decay is not None:
        s.LAYER_DECAY = layer_decay
    cfg.LOG_PERIOD = period
    if update:
        cfg.SVIT.UPDATE_MONITOR = True
        cfg.SVIT.UPDATE_MONITOR_EVERY = every
    else:
        cfg.SVIT.GUARDED_STEP = True
    if monitor:
        cfg.SVIT.MONITOR = True
    if ema:
        cfg.SVIT.EMA_DECAY = 0.9
    opt = optim.construct_optimizer(model, cfg)
    av = ema_mod.build_ema(cfg, model, opt)
    tm = mon_mod.build_monitor(cfg, opt)
    um = updmon.build_update_monitor(cfg, opt)
    assert isinstance(opt, optim.GuardedClipAdamW) and opt.update_monitor is um and (um is not None) == update
    return types.SimpleNamespace(cfg=cfg, model=model, opt=opt, um=um, tm=tm, ema=av)


def host(t):
    return None if t is None else t.detach().cpu().numpy().copy()


def weights(k):
    torch.cuda.synchronize()
    return host(k.model.flat.data)


def after(k, p_before):
    """what update_host takes of a step: the weights in front of it and behind it, the gradient and the moments behind it"""
    torch.cuda.synchronize()
    m, v = k.um._moments() if k.um is not None else (None, None)
    return p_before, host(k.model.flat.data), host(k.model.flat.grad), host(m), host(v)


def check_rows(um, rows, seen, what, flags):
    """every row `read()` gave against update_host on the buffers of its step"""
    from svit_amd import updmon
    assert len(rows["steps"]) > 0
    Tn = len(um.names)
    for i, step in enumerate(rows["steps"].tolist()):
        args = seen[step] + (um.table, um.segments)
        want, terms = updmon.update_host(*args, step=step), updmon.abs_terms_host(*args)
        got = np.zeros((), dtype=updmon.row_dtype(Tn))
        got["head"] = (step, int(rows["flags"][i]), 0)
        for key in U.SUMS + ("n_still", "n_one_ulp"):
            got["entry"][key] = rows[key].data[i]
        got["entry"]["absmax_d"] = rows["absmax"].data[i]
        assert int(rows["flags"][i]) == flags
        U.assert_row(got, want, terms, "%s, step %d" % (what, step))
        live = ~um.frozen
        assert np.array_equal(np.ma.getmaskarray(rows["ratio"])[i], um.frozen)
        e = want["entry"]
        assert np.array_equal(rows["update_norm"].data[i][live], np.sqrt(rows["sumsq_d"].data[i][live]))
        assert (rows["n_still"].data[i][live] >= 0).all() and (rows["n_still"].data[i][~live] == -1).all()
        assert (e["n_still"][live] + e["n_one_ulp"][live] <= um.numel[live]).all()


@pytest.mark.parametrize("method", ["adamw", "adam", "sgd"])
def test_e_three_steps_through_construct_optimizer(method):
    """three eager steps of each solver under cfg.SVIT.UPDATE_MONITOR, every row against update_host on copies of the
    weights taken before and after the step, of the gradient and of the moments after it.  FAILS ON THE PARENT COMMIT:
    there is no svit_amd.updmon there, and construct_optimizer does not know the key (adamw would get the classic tail,
    which has no attach_update_monitor)."""
    from svit_amd import optim, updmon
    x, y = batch()
    k = make(method)
    assert type(k.opt) is {"adamw": optim.GuardedClipAdamW, "adam": optim.GuardedClipAdam, "sgd": optim.GuardedClipSGD}[method]
    assert type(k.um) is updmon.UpdateMonitor and len(k.um.names) == 405 and k.um.period == 4 and not k.um.frozen.any()
    assert k.um.shadow.numel() == k.model.flat.total and k.opt.monitor is None
    seen = {}
    for i in range(3):
        optim.set_lr(k.opt, LR[method] * (i + 1))
        fwd_bwd(k.model, x, y)
        before = weights(k)
        k.opt.step()
        seen[i] = after(k, before)
        assert same(k.um.shadow, torch.from_numpy(before).to(DEV))
    rows = k.um.read()
    assert rows["steps"].tolist() == [0, 1, 2] and rows["lost"] == 0
    check_rows(k.um, rows, seen, method, flags={"adamw": 3, "adam": 3, "sgd": 1}[method])
    assert bool((rows["update_norm"][:, rows["numel"] > 100] > 0).all())
    if method == "sgd":
        assert bool((rows["v_mean"] == 0).all()) and bool((rows["m_rms"][:, rows["numel"] > 100] > 0).all())
        assert np.nanmedian(rows["cos_grad"].data[0]) > 0.99          # the first step is along the clipped gradient (+ decay)
    else:
        # (under decoupled decay a tensor whose gradient is all zeros -- there are some in this tiny model -- has v = 0)
        assert (rows["v_mean"].data > 0).mean() > 0.5 and (rows["v_mean"].data >= 0).all()
    layers = k.um.by_layer(rows)
    assert layers["ratio"].shape == (3, k.cfg.MVIT.DEPTH + 2) and bool((layers["ratio"] > 0).all())
    again = k.um.read()
    assert again["steps"].tolist() == [] and again["lost"] == 0
    stats = k.um.log_stats(rows)
    assert stats["_type"] == "train_update_stats" and stats["step"] == 2 and k.um.log_stats(again) is None


def test_e_the_step_is_the_unwatched_one_and_a_dropped_step_leaves_no_row():
    """a NaN in the gradient of step 1: dropped -- no row, the shadow keeps step 0's weights bit for bit; weights and
    moments are those of an optimizer without the monitor, bit for bit, as is the state_dict's layout"""
    x, y = batch()
    kw, kb = make("adamw"), make("adamw", update=False)
    assert kb.um is None and kb.opt.update_monitor is None
    seen = {}
    for i in range(3):
        for k in (kw, kb):
            fwd_bwd(k.model, x, y)
            if i == 1:
                k.model.flat.grad[12345] = NAN
        before, shadow = weights(kw), kw.um.shadow.clone()
        kw.opt.step()
        kb.opt.step()
        seen[i] = after(kw, before)
        if i == 1:
            assert kw.opt.stats()["skipped"] == 1 and same(kw.um.shadow, shadow)
            assert same(shadow, torch.from_numpy(seen[0][0]).to(DEV))           # step 0's weights, not step 1's
    rows = kw.um.read()
    assert rows["steps"].tolist() == [0, 2] and rows["lost"] == 1
    check_rows(kw.um, rows, seen, "around a dropped step", flags=3)
    for name, a, b in [("weights", kw.model.flat.data, kb.model.flat.data)] + [(s, getattr(kw.opt, s), getattr(kb.opt, s))
                                                                             for s in kw.opt.STATE]:
        assert same(a, b), name
    assert kw.opt.stats() == kb.opt.stats() and list(kw.opt.state_dict()) == list(kb.opt.state_dict()) == ["state", "param_groups"]


def test_e_cut_4_and_layer_decay():
    """a frozen cut at 4 (the `_seg` tail): the frozen tensors come back masked, their entries and their part of the shadow
    untouched; SOLVER.LAYER_DECAY = 0.75 (the `_lr` tail): the lower a layer, the smaller its step against its weights"""
    x, y = batch()
    k = make("adamw", cut=4, period=2)
    um = k.um
    assert k.opt.cut == 4 and um.segments is k.opt.segments and 0 < int(um.frozen.sum()) < 405
    um.shadow.fill_(7.0)
    seen = {}
    for i in range(3):
        fwd_bwd(k.model, x, y)
        before = weights(k)
        k.opt.step()
        seen[i] = after(k, before)
    rows = um.read()
    assert rows["steps"].tolist() == [1, 2] and rows["lost"] == 1
    check_rows(um, rows, seen, "cut 4", flags=3)
    assert bool(np.ma.getmaskarray(rows["update_norm"])[:, um.frozen].all())
    t = int(np.flatnonzero(um.frozen)[0])
    a, b = um.table[t]
    assert bool((um.shadow[a:b] == 7.0).all())
    masked = np.ma.getmaskarray(um.by_layer(rows)["ratio"])[0]
    assert masked[0] and not masked[-1] and 0 < masked.sum() < len(masked)          # the stem's group is all frozen

    k = make("adamw", layer_decay=0.75)
    assert k.opt.lr_segments is not None
    seen = {}
    fwd_bwd(k.model, x, y)
    before = weights(k)
    k.opt.step()
    seen[0] = after(k, before)
    rows = k.um.read()
    check_rows(k.um, rows, seen, "layer decay", flags=3)
    # AdamW's first step moves every element by lr_eff: |Delta| max per tensor follows the layer's scale
    depth = k.cfg.MVIT.DEPTH
    top = rows["absmax"].data[0][k.um.layer_ids == depth + 1].max()
    stem = rows["absmax"].data[0][k.um.layer_ids == 0].max()
    assert 0.9 * 0.75 ** (depth + 1) < stem / top < 1.1 * 0.75 ** (depth + 1)


def _trace_names(monkeypatch, fn):
    """names of the library launches issued while fn() runs, in order"""
    from svit_amd import hip
    names = []
    real = hip.call

    def logging(name, *a, **kw):
        names.append(name)
        return real(name, *a, **kw)
    monkeypatch.setattr(hip, "call", logging)
    try:
        out = fn()
    finally:
        monkeypatch.setattr(hip, "call", real)
    return out, names


def _tail(names):
    """the optimizer tail's launches among `names`"""
    return [n for n in names if n.startswith(("svit_step_guard", "svit_adamw_step", "svit_sgd_", "svit_adam_", "svit_ema_",
                                              "svit_tensor_", "svit_update_"))]


def _ring(mon):
    torch.cuda.synchronize()
    return mon.ring.cpu().numpy().tobytes()


def test_f_graphed_step_replays_the_monitor(monkeypatch):
    """the captured step, with a TensorMonitor and an EMA attached beside the update monitor, over a poisoned first replay
    and three more with lr changes equals the eager step in the rows of both monitors, the weights, the moments and the
    average; a replay after the attachment changed is refused"""
    from svit_amd import hip, optim
    from svit_amd.graph import GraphedTrainStep
    poison = torch.ones(1, device=DEV)

    def loss_fun(p, e, y):
        return torch.nn.functional.cross_entropy(p, y) * poison

    x, y = batch()
    kg = make("adamw", period=8, ema=True, monitor=True)
    ke = make("adamw", period=8, ema=True, monitor=True)
    empty = _ring(kg.um)
    step, names = _trace_names(monkeypatch, lambda: GraphedTrainStep(kg.model, loss_fun, [x], y, optimizer=kg.opt))
    assert _tail(names) == ["svit_step_guard", "svit_tensor_stats", "svit_update_snapshot", "svit_adamw_step_guarded",
                            "svit_update_stats", "svit_ema_step_guarded"]
    assert _ring(kg.um) == empty and kg.opt.stats()["applied"] == 0                 # building recorded nothing

    def eager():
        ke.opt.zero_grad()
        logits, extra = ke.model([x], {})
        loss = loss_fun(logits, extra, y)
        loss.backward()
        ke.opt.step()
        return loss.detach()

    def compare(what):
        torch.cuda.synchronize()
        pairs = [("weights", kg.model.flat.data, ke.model.flat.data), ("average", kg.ema.buf, ke.ema.buf),
                 ("shadow", kg.um.shadow, ke.um.shadow)]
        for name, a, b in pairs + [(s, getattr(kg.opt, s), getattr(ke.opt, s)) for s in kg.opt.STATE]:
            assert same(a, b), (what, name)
        assert kg.opt.stats() == ke.opt.stats() and _ring(kg.um) == _ring(ke.um) and _ring(kg.tm) == _ring(ke.tm), what

    poison.fill_(NAN)
    shadow = kg.um.shadow.clone()
    step([x], y)
    eager()
    compare("poisoned step")
    assert _ring(kg.um) == empty and same(kg.um.shadow, shadow)
    poison.fill_(1.0)
    seen = {}
    for i in range(3):
        optim.set_lr(kg.opt, LR["adamw"] * (i + 1))
        optim.set_lr(ke.opt, LR["adamw"] * (i + 1))
        before = weights(kg)
        lg, _ = step([x], y)
        le = eager()
        assert same(lg, le)
        compare("step %d" % (i + 1))
        seen[i + 1] = after(kg, before)
    rows = kg.um.read()
    assert rows["steps"].tolist() == [1, 2, 3] and rows["lost"] == 1                # step 0 was dropped: no row
    check_rows(kg.um, rows, seen, "replay", flags=3)
    assert kg.tm.read()["steps"].tolist() == [0, 1, 2, 3]                           # the TensorMonitor's rows join by step
    # the capture holds the launches of the monitor attached THEN
    kg.opt.attach_update_monitor(None)
    with pytest.raises(hip.SvitHipError, match="attached UpdateMonitor changed after this GraphedTrainStep was built"):
        step([x], y)
    kg.opt.attach_update_monitor(kg.um)
    step([x], y)
    torch.cuda.synchronize()
    assert kg.um.read()["steps"].tolist() == [4]


def test_f_accumulated_step_k2_reproducible(monkeypatch):
    """AccumulatedTrainStep(k = 2) under SVIT.REPRODUCIBLE: ONE snapshot and ONE statistics pair per call, around the one
    solver launch; rows, weights and momentum equal the eager micro-steps + optimizer.step() on a second model bit for bit"""
    from svit_amd import hip, optim, train
    from svit_amd.graph import AccumulatedTrainStep, GraphedTrainStep
    A, B, C = batch(), batch("B"), batch("C")
    kg, ke = make("sgd", mode="reproducible"), make("sgd", mode="reproducible")
    micro = GraphedTrainStep(kg.model, ce, [A[0]], A[1], accumulate=True)
    step = AccumulatedTrainStep(kg.model, [micro, micro], kg.opt)
    seen = {}
    for i, batches in enumerate(([A, B], [C, A], [B, C])):
        optim.set_lr(kg.opt, LR["sgd"] * (i + 1))
        optim.set_lr(ke.opt, LR["sgd"] * (i + 1))
        batches = [([x], y) for x, y in batches]
        before = weights(kg)
        _, names = _trace_names(monkeypatch, lambda: step(batches))
        assert names.count("svit_update_snapshot") == 1 and names.count("svit_update_stats") == 1
        assert _tail(names) == ["svit_step_guard", "svit_update_snapshot", "svit_sgd_step_guarded", "svit_update_stats"]
        train.accumulate_step(ke.model, [ce, ce], batches, ke.opt)
        torch.cuda.synchronize()
        assert same(kg.model.flat.data, ke.model.flat.data) and same(kg.opt.momentum_buffer, ke.opt.momentum_buffer)
        assert _ring(kg.um) == _ring(ke.um)
        seen[i] = after(kg, before)
    rows = kg.um.read()
    assert rows["steps"].tolist() == [0, 1, 2] and rows["lost"] == 0
    check_rows(kg.um, rows, seen, "accumulated", flags=1)
    kg.opt.attach_update_monitor(None)
    with pytest.raises(hip.SvitHipError, match="attached UpdateMonitor changed after this AccumulatedTrainStep was built"):
        step(batches)


def test_h_without_the_key_the_launches_are_the_parents(monkeypatch):
    """no SVIT.UPDATE_MONITOR: build_update_monitor gives None, there is no shadow, and a capture issues the body of a
    capture without an optimizer, then the guard and the plain guarded AdamW -- the parent commit's launch names"""
    from svit_amd.graph import GraphedTrainStep
    x, y = batch()
    k = make("adamw", update=False)
    _, mb = build()
    assert k.um is None and k.opt.update_monitor is None and not hasattr(k.opt, "shadow")
    _, bare = _trace_names(monkeypatch, lambda: GraphedTrainStep(mb, ce, [x], y))
    step, names = _trace_names(monkeypatch, lambda: GraphedTrainStep(k.model, ce, [x], y, optimizer=k.opt))
    assert _tail(bare) == [] and _tail(names) == ["svit_step_guard", "svit_adamw_step_guarded"]
    assert [n for n in names if n not in _tail(names)] == bare
    _, eager = _trace_names(monkeypatch, k.opt.step)
    assert eager == ["svit_step_guard", "svit_adamw_step_guarded"]
    assert list(k.opt.state_dict()) == ["state", "param_groups"]
