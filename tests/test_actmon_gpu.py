"""Activation monitor on the GPU: svit_act_stats against its NumPy float64 restatement (actmon.acts_host) on synthetic
sites, and the monitor carried through the tiny model -- the eager, the captured and the accumulated step, a frozen cut,
a NaN pixel and an infinite bias located, a TensorMonitor and an EMA beside it.  Sums inside 2^-27 of sum |term|
(tests/actmon_cases.py), everything else and every run-to-run comparison bit for bit.  Needs a real MI355X."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import procedural as P
from tests import actmon_cases as A
from tests.smoke_impl import build_hip_model

DEV = "cuda"
NAN = float("nan")
CANARY = 0xA5
PAD = 256               # canary bytes on either side of a buffer


def bits(t):
    return t.contiguous().view(torch.int32)


def same(a, b):
    return torch.equal(bits(a), bits(b))


# ===================================================================================================== kernel ====
def guarded(nbytes):
    """(whole, inner): a uint8 buffer with PAD canary bytes on either side of `inner`"""
    whole = torch.full((PAD + nbytes + PAD,), CANARY, dtype=torch.uint8, device=DEV)
    return whole, whole[PAD:PAD + nbytes]


class Rig:
    """host sites on the device, packed back to back in ONE buffer (so most arrays are 4-byte aligned and no more), with
    the ring, the workspace and the pass counter between canaries"""

    def __init__(self, sites, slots=None, n_slots=None, R=4, rec=None):
        from svit_amd import actmon, ops
        self.host = sites
        flat = np.concatenate([x for s in sites for x in s if x is not None])
        self.buf = torch.from_numpy(flat).to(DEV)
        self.sites, off = [], 0
        for a, b in sites:
            pa = self.buf.data_ptr() + 4 * off
            off += len(a)
            pb = None
            if b is not None:
                pb = self.buf.data_ptr() + 4 * off
                off += len(b)
            self.sites.append((pa, pb, len(a)))
        self.slots = list(range(len(sites))) if slots is None else list(slots)
        self.n_slots = len(sites) if n_slots is None else n_slots
        self.R = R
        self.rec = rec
        W = ops.act_stats_window()
        self.windows = sum((len(a) + W - 1) // W for a, _ in sites)
        self.ring_all, self.ring = guarded(R * (48 + 32 * self.n_slots))
        self.ring.copy_(torch.from_numpy(actmon.empty_ring(R, self.n_slots).view(np.uint8).reshape(-1).copy()))
        self.ws_all, self.ws = guarded(ops.act_stats_workspace(self.windows))
        self.state_all, st = guarded(8)
        self.state = st.view(torch.int64)
        self.state.zero_()
        self.geom = (3, 4, 2, 16, 16)

    def launch(self):
        from svit_amd import ops
        before = self.buf.clone()
        rec0 = None if self.rec is None else self.rec.clone()
        ops.act_stats(self.sites, self.slots, self.n_slots, self.geom, self.rec, self.ring, self.R, self.state, self.ws)
        torch.cuda.synchronize()
        assert same(self.buf, before), "a site was written"
        assert rec0 is None or torch.equal(self.rec, rec0), "the step record was written"
        for name, whole in (("ring", self.ring_all), ("workspace", self.ws_all), ("state", self.state_all)):
            edge = torch.cat([whole[:PAD], whole[-PAD:]])
            assert bool((edge == CANARY).all()), "a canary beside the %s was overwritten" % name

    def rows(self):
        from svit_amd import actmon
        return self.ring.cpu().numpy().view(actmon.row_dtype(self.n_slots)).copy()

    def want(self):
        from svit_amd import actmon
        return actmon.acts_host(self.host)


def head(row):
    """a ring row's header as ten ints: pass, step, B, Tx, T0, H0, W0, n_sites, reserved x 2"""
    h = row["head"]
    return tuple(int(h[k]) for k in ("pass", "step", "B", "Tx", "T0", "H0", "W0", "n_sites")) + tuple(
        int(v) for v in h["reserved"])


def _empty_row(n_slots):
    from svit_amd import actmon
    return actmon.empty_ring(1, n_slots)[0]


def test_a_kernel_is_the_yardstick():
    """plain values on sites of 1, 3, W - 1, W, W + 1 and 3 W + 5 rows of both kinds, with ties in the extremum; header,
    pass counter and the other rows; a second run from the same state bit for bit"""
    from svit_amd import ops
    W = ops.act_stats_window()
    s, where = A.sites(W)
    args = A.ties(s, where)
    r = Rig(s)
    r.launch()
    rows = r.rows()
    assert head(rows[0]) == (0, -1, 3, 4, 2, 16, 16, 12, 0, 0) and int(r.state[0]) == 1
    want, mass = r.want()
    A.assert_entries(rows[0]["entry"], want, mass, "plain")
    assert (rows[0]["entry"]["n_bad"] == 0).all() and (mass > 0).all()
    for i, arg in args.items():
        assert rows[0]["entry"]["arg"][i] == arg
    for k in (1, 2, 3):
        assert rows[k].tobytes() == _empty_row(r.n_slots).tobytes(), k
    first = rows[0]["entry"].tobytes()
    r.launch()                                                          # the second pass lands in row 1
    rows = r.rows()
    assert rows[1]["entry"].tobytes() == first and rows[0]["entry"].tobytes() == first
    assert rows[1]["head"]["pass"] == 1 and int(r.state[0]) == 2


def test_a_bad_rows_and_sites_without_a_good_row():
    """NaN, +inf, -inf, rstd 0, -0 and negative: on a site's first and last row, on either side of a window edge, in two
    windows at once; two sites with no good row; a denormal rstd is a good row"""
    from svit_amd import ops
    W = ops.act_stats_window()
    s, where = A.sites(W)
    A.ties(s, where)
    bad = A.bad_rows(s, where, W)
    s[where["ln W - 1"]][1][17] = np.float32(1e-41)
    r = Rig(s)
    r.launch()
    e = r.rows()[0]["entry"]
    want, mass = r.want()
    A.assert_entries(e, want, mass, "bad rows")
    assert {int(i): (int(e["n_bad"][i]), int(e["first_bad"][i])) for i in np.flatnonzero(e["n_bad"] > 0)} == bad
    assert (e["first_bad"][e["n_bad"] == 0] == -1).all()
    for name in ("ln 3", "lse 1"):
        z = e[where[name]]
        assert (z["sum"], z["ext"], z["ext2"], z["arg"]) == (0.0, 0.0, 0.0, -1) and z["n_bad"] == z["rows"]
    d = e[where["ln W - 1"]]
    assert d["arg"] == 17 and d["ext"].tobytes() == np.float32(1e-41).tobytes() and np.isfinite(d["sum"]) and d["sum"] > 1e81


def test_b_96_sites_an_absent_slot_and_97_refused():
    from svit_amd import hip, ops
    rng = np.random.default_rng(5)

    def make(n):
        return [[rng.standard_normal(4).astype(np.float32), None if i % 3 == 1 else
                 np.exp(rng.standard_normal(4)).astype(np.float32)] for i in range(n)]
    # 96 sites into 97 slots in reversed order: slot 40 is named by no site
    slots = [96 - i if 96 - i > 40 else 95 - i for i in range(96)]
    r = Rig(make(96), slots=slots, n_slots=97)
    marked = r.rows()
    marked["entry"]["sum"][:, 40] = 123.0                              # what an earlier pass left in the absent slot
    marked["entry"]["n_bad"][:, 40] = 0
    r.ring.copy_(torch.from_numpy(marked.view(np.uint8).reshape(-1)))
    r.launch()
    row = r.rows()[0]
    want, mass = r.want()
    A.assert_entries(row["entry"][slots], want, mass, "96 sites")
    assert row["entry"][40].tobytes() == _empty_row(97)["entry"][40].tobytes() and row["head"]["n_sites"] == 96
    assert r.rows()[1]["entry"]["sum"][40] == 123.0
    # 97 sites: refused before any launch
    big = Rig(make(97))
    before = big.rows().tobytes()
    with pytest.raises(hip.SvitHipError, match="svit_act_stats failed: bad argument"):
        ops.act_stats(big.sites, big.slots, big.n_slots, big.geom, None, big.ring, big.R, big.state, big.ws)
    torch.cuda.synchronize()
    assert big.rows().tobytes() == before and int(big.state[0]) == 0
    # the wrapper's own refusals
    cases = {"a ring of another size": dict(ring=r.ring[:-16]), "a host ring": dict(ring=r.ring.cpu()),
             "a state of int32": dict(state=torch.zeros(2, dtype=torch.int32, device=DEV)),
             "a record of floats": dict(dev_rec=torch.zeros(12, device=DEV)), "a short workspace": dict(workspace=r.ws[:-32]),
             "geom of four": dict(geom=(1, 2, 3, 4)), "a slot too few": dict(slots=r.slots[:-1])}
    args = dict(sites=r.sites, slots=r.slots, n_slots=r.n_slots, geom=r.geom, dev_rec=None, ring=r.ring, R=r.R,
                state=r.state, workspace=r.ws)
    before = r.rows().tobytes()
    for label, kw in cases.items():
        with pytest.raises(hip.SvitHipError):
            ops.act_stats(**dict(args, **kw))
        torch.cuda.synchronize()
        assert r.rows().tobytes() == before and int(r.state[0]) == 1, label


def test_c_ring_of_two_rows_overrun_and_the_step_record():
    """R = 2 overrun by one pass; dev_rec NULL gives step -1, a record of applied = 5, skipped = 2 gives step 7"""
    from svit_amd import ops
    W = ops.act_stats_window()
    s, _ = A.sites(W)
    s = s[4:8]
    rec = torch.zeros(12, dtype=torch.int32, device=DEV)
    rec.view(torch.int64)[0:1].fill_(5)
    rec.view(torch.int64)[1:2].fill_(2)
    r = Rig(s, R=2, rec=rec)
    host = {}
    for p in range(3):
        r.buf.mul_(1.25)
        r.host = [[x if x is None else (x * np.float32(1.25)) for x in site] for site in r.host]
        r.launch()
        host[p] = r.want()
    rows = r.rows()
    assert rows["head"]["pass"].tolist() == [2, 1] and rows["head"]["step"].tolist() == [7, 7] and int(r.state[0]) == 3
    A.assert_entries(rows[0]["entry"], *host[2], "pass 2")
    A.assert_entries(rows[1]["entry"], *host[1], "pass 1")
    assert rows[0]["entry"]["sum"].tobytes() != rows[1]["entry"]["sum"].tobytes()
    bare = Rig(s)
    bare.launch()
    assert bare.rows()[0]["head"]["step"] == -1


# ======================================================================================================= model ====
LR = 1e-3


def build(mode="deterministic"):
    cfg, model, _, _ = build_hip_model(4, 64)
    if mode == "reproducible":
        model.engine.reproducible = True
    else:
        model.engine.deterministic = True
    return cfg, model


def batch(tag=""):
    return P.frames(2, 4, 64, tag="clip" + tag).cuda(), P.labels(2, tag="label" + tag).cuda()


def ce(p, e, y):
    return torch.nn.functional.cross_entropy(p, y)


def make(mode="deterministic", cut=0, monitor=True, period=8, tensor_monitor=False, ema=False, max_skips=None,
         method="adamw", k=1):
    from svit_amd import actmon, optim
    from svit_amd import ema as ema_mod
    from svit_amd import monitor as mon_mod
    cfg, model = build(mode)
    if cut:
        model.freeze_below(cut)
    s = cfg.SOLVER
    s.OPTIMIZING_METHOD, s.BASE_LR, s.WEIGHT_DECAY, s.CLIP_GRAD_L2NORM = method, LR if method != "sgd" else 0.05, 1e-4, 1.0
    s.MOMENTUM, s.DAMPENING, s.NESTEROV = 0.9, 0.0, True
    cfg.LOG_PERIOD = period
    cfg.SVIT.GUARDED_STEP = True
    if monitor:
        cfg.SVIT.ACT_MONITOR = True
    if tensor_monitor:
        cfg.SVIT.MONITOR = True
    if ema:
        cfg.SVIT.EMA_DECAY = 0.9
    if max_skips is not None:
        cfg.SVIT.MAX_CONSECUTIVE_SKIPS = max_skips
    opt = optim.construct_optimizer(model, cfg)
    ema_mod.build_ema(cfg, model, opt)
    mon_mod.build_monitor(cfg, opt)
    mon = actmon.build_actmon(cfg, model, opt, virtual_ranks=k)
    assert (mon is not None) == monitor and model.engine.act_monitor is mon and opt.act_monitor is mon
    return cfg, model, opt, mon


class Spy:
    """keeps what every `mon.enqueue(st)` saw: the host copies of the pass's statistics, in pass order"""

    def __init__(self, mon):
        self.mon, self.seen, self.real = mon, [], mon.enqueue
        mon.enqueue = self

    def __call__(self, st):
        _, slots, keep = self.mon.sites_of(st)
        self.seen.append((slots, keep))
        return self.real(st)

    def host(self, i):
        slots, keep = self.seen[i]
        torch.cuda.synchronize()
        return slots, [(a.cpu().numpy().reshape(-1), None if b is None else b.cpu().numpy().reshape(-1)) for a, b in keep]


def check_pass(mon, ring_row, slots, sites, what):
    """one ring row against acts_host on the arrays of the forward's own saved state"""
    from svit_amd import actmon
    want, mass = actmon.acts_host(sites)
    A.assert_entries(ring_row["entry"][slots], want, mass, what)
    absent = np.setdiff1d(np.arange(mon.n_slots), slots)
    assert (ring_row["entry"]["n_bad"][absent] == -1).all(), what
    return want


def ring_rows(mon):
    from svit_amd import actmon
    torch.cuda.synchronize()
    return mon.ring.cpu().numpy().view(actmon.row_dtype(mon.n_slots)).copy()


def eager_step(model, opt, x, y, loss_fun=ce):
    opt.zero_grad()
    logits, extra = model([x], {})
    loss = loss_fun(logits, extra, y)
    loss.backward()
    opt.step()
    return loss.detach()


def test_d_three_eager_steps_through_construct_optimizer():
    """(on the parent commit there is no svit_amd.actmon)"""
    from svit_amd import optim
    x, y = batch()
    cfg, model, opt, mon = make()
    assert mon.n_slots == 49 and mon.period == 8 and type(opt) is optim.GuardedClipAdamW
    spy = Spy(mon)
    for i in range(3):
        eager_step(model, opt, x, y)
    rows = mon.read()
    assert rows["passes"].tolist() == [0, 1, 2] and rows["steps"].tolist() == [0, 1, 2] and rows["lost"] == 0
    raw = ring_rows(mon)
    for i in range(3):
        slots, sites = spy.host(i)
        assert slots == list(range(49))
        want = check_pass(mon, raw[i], slots, sites, "eager step %d" % i)
        assert head(raw[i]) == (i, i, 2, 4, 2, 16, 16, 49, 0, 0)
        assert want["rows"][0] == 2 * 529 and want["rows"][1] == 2 * 529 and want["rows"][-1] == 2 * (1 + 8 + 16)
    assert (rows["n_bad"].data == 0).all() and not np.ma.getmaskarray(rows["n_bad"]).any() and mon.origin(rows) == []
    ln, lse = ~mon.is_lse, mon.is_lse
    assert bool((rows["rms"][:, ln] > 0).all()) and bool((rows["widest_std"][:, ln] > 0).all())
    assert np.isfinite(rows["lse_max"][:, lse]).all() and bool((rows["lse_max"][:, lse] >= rows["lse_mean"][:, lse]).all())
    assert not np.array_equal(rows["sum"].data[0], rows["sum"].data[2])                 # the weights moved
    # the residual stream's mean square, from the statistics alone, against the activations themselves
    with torch.no_grad():
        _, st = model.engine.forward(x, None, save=True)
    torch.cuda.synchronize()
    x1 = st["blocks"][5]["x1"].double()
    direct = float((x1 * x1).mean())
    got = mon.read()
    assert got["passes"].tolist() == [3] and abs(got["mean_sq"].data[0][3 * 5 + 2] - direct) <= 1e-3 * direct
    assert mon.log_stats(got)["pass"] == 3 and mon.read()["passes"].tolist() == []


def _receptive_tokens(plan, T0, H0, W0, t, h, w):
    """tokens (1-based patch indices in the sequence) whose patch_kernel window at patch_stride / patch_pad holds input
    position (t, h, w)"""
    (kt, kh, kw), (st, sh, sw), (pt, ph, pw) = plan.patch_kernel, plan.patch_stride, plan.patch_pad
    out = []
    for a in range(T0):
        for b in range(H0):
            for c in range(W0):
                if (a * st - pt <= t < a * st - pt + kt and b * sh - ph <= h < b * sh - ph + kh
                        and c * sw - pw <= w < c * sw - pw + kw):
                    out.append(1 + (a * H0 + b) * W0 + c)
    return out


def test_d_a_nan_pixel_is_traced_to_the_stem():
    """a NaN pixel in clip 1: blocks.0.in is the first bad slot, first_bad is sample 1's smallest token whose 3 x 7 x 7
    window holds the pixel and n_bad the number of such tokens; origin() and check() name the stem; weights and moments
    are those of a run without the monitor, bit for bit"""
    x, y = batch()
    x = x.clone()
    x[1, 2, 2, 33, 18] = NAN
    _, mw, ow, mon = make(max_skips=1)
    _, mb, ob, none = make(monitor=False, max_skips=1)
    assert none is None and ob.act_monitor is None
    clean, _ = batch()
    for i, inp in enumerate((clean, x, clean)):
        for model, opt in ((mw, ow), (mb, ob)):
            eager_step(model, opt, inp, y)
        torch.cuda.synchronize()
        if i == 1:
            assert ow.stats()["skipped"] == 1 and ob.stats()["skipped"] == 1
            with pytest.raises(RuntimeError) as told:
                ow.check()
            with pytest.raises(RuntimeError) as bare:
                ob.check()
            head, line = str(told.value).split("\n")
            assert head == str(bare.value) and "\n" not in str(bare.value)
            assert line.startswith("non-finite activations in the forward of step 1 (pass 1): first at blocks.0.in, ")
            assert line.endswith("look at the stem or the input") and "in sample 1 at token" in line
        else:
            ow.check()
    rows = mon.read()
    assert rows["passes"].tolist() == [0, 1, 2] and rows["steps"].tolist() == [0, 1, 2]
    toks = _receptive_tokens(mw.plan, 2, 16, 16, 2, 33, 18)
    assert len(toks) > 1
    nb = rows["n_bad"].data
    assert (nb[0] == 0).all() and (nb[2] == 0).all() and nb[1][0] == len(toks) and (nb[1][2:] > 0).all()
    assert rows["first_bad"].data[1][0] == 529 + min(toks)
    found = mon.origin(rows)
    assert found == [(1, 1, "blocks.0.in", len(toks), mon.where(rows["header"][1], 0, 529 + min(toks)), "the stem or the input")]
    assert found[0][4][:2] == (1, min(toks)) and found[0][4][2][0] == "patch"
    # behind block 0's attention branch: those tokens and more (the residual and the pooled queries carry the NaN on), all
    # of them in sample 1
    assert len(toks) <= nb[1][2] <= 529 and 529 <= rows["first_bad"].data[1][2] < 2 * 529
    for name, a, b in [("weights", mw.flat.data, mb.flat.data)] + [(k, getattr(ow, k), getattr(ob, k)) for k in ow.STATE]:
        assert same(a, b), name
    assert ow.stats() == ob.stats()


def test_d_an_infinite_bias_is_traced_to_the_mlp_of_block_2():
    x, y = batch()
    _, model, opt, mon = make()
    with torch.no_grad():
        model.flat.p("blocks.2.mlp.fc2.bias")[5] = float("inf")
    eager_step(model, opt, x, y)
    rows = mon.read()
    nb = rows["n_bad"].data[0]
    names = mon.names
    upto = names.index("blocks.2.mid")
    assert (nb[:upto + 1] == 0).all() and nb[names.index("blocks.3.in")] > 0
    found = mon.origin(rows)
    assert len(found) == 1 and found[0][2] == "blocks.3.in" and found[0][5] == "the MLP of block 2"
    assert found[0][3] == rows["rows"].data[0][names.index("blocks.3.in")] and found[0][4] == (0, 0, "cls")
    assert opt.stats()["skipped"] == 1


def test_e_frozen_cut_4_masks_the_slots_below():
    x, y = batch()
    _, model, opt, mon = make(cut=4)
    spy = Spy(mon)
    eager_step(model, opt, x, y)
    rows = mon.read()
    slots, sites = spy.host(0)
    assert slots == list(range(9, 49))                                     # blocks 0, 1, 2 lie below position 4
    check_pass(mon, ring_rows(mon)[0], slots, sites, "cut 4")
    mask = np.ma.getmaskarray(rows["n_bad"])[0]
    assert mask[:9].all() and not mask[9:].any() and (rows["n_bad"].data[0][:9] == -1).all()
    assert rows["header"]["n_sites"].tolist() == [40] and bool(np.ma.getmaskarray(rows["rms"])[0][:9].all())


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


def _entries(mon, passes):
    raw = ring_rows(mon)
    by = {int(r["head"]["pass"]): r for r in raw}
    return [(int(by[p]["head"]["step"]), by[p]["entry"].tobytes(), by[p]["head"][["B", "Tx", "T0", "H0", "W0", "n_sites"]].tobytes())
            for p in passes]


def test_f_graphed_step_replays_the_monitor(monkeypatch):
    """the captured step over a poisoned first replay and three more equals the eager step in entries and steps (the
    capture's warm-up passes advance the pass counter, so both monitors are reset first); with a TensorMonitor and an
    EMA attached as well; a replay after the attached monitor changed is refused"""
    from svit_amd import hip, optim
    from svit_amd.graph import GraphedTrainStep
    poison = torch.ones(1, device=DEV)

    def loss_fun(p, e, y):
        return torch.nn.functional.cross_entropy(p, y) * poison

    x, y = batch()
    bad = x.clone()
    bad[0, 0, 1, 5, 7] = NAN
    _, mg, og, ng = make(period=8, tensor_monitor=True, ema=True)
    _, me, oe, ne = make(period=8, tensor_monitor=True, ema=True)
    step, names = _trace_names(monkeypatch, lambda: GraphedTrainStep(mg, loss_fun, [x], y, optimizer=og))
    # one pair of launches per forward (the warm-up bodies and the captured one), behind the last block and the final norm
    assert names.count("svit_act_stats") * 16 == names.count("svit_attn_fwd") > 0
    assert names.count("svit_tensor_stats") == 1 and "svit_ema_step_guarded" in names
    last = len(names) - 1 - names[::-1].index("svit_act_stats")
    assert names[last - 1] == "svit_layernorm_fwd" and last < names.index("svit_step_guard")
    assert og.stats()["applied"] == 0
    assert int(ng.state[0]) >= 1                                           # the warm-up passes ran and were recorded
    ng.reset()
    spy = Spy(ne)
    for i, inp in enumerate((bad, x, x, x)):
        optim.set_lr(og, LR * (i + 1))
        optim.set_lr(oe, LR * (i + 1))
        lg, _ = step([inp], y)
        le = eager_step(me, oe, inp, y, loss_fun)
        torch.cuda.synchronize()
        assert (i == 0 or same(lg, le)) and same(mg.flat.data, me.flat.data), i
    assert og.stats() == oe.stats() and og.stats()["skipped"] == 1
    assert _entries(ng, range(4)) == _entries(ne, range(4))
    raw = ring_rows(ng)
    for i in range(4):
        slots, sites = spy.host(i)
        check_pass(ng, raw[i], slots, sites, "replay %d" % i)
    rows = ng.read()
    assert rows["passes"].tolist() == [0, 1, 2, 3] and rows["steps"].tolist() == [0, 1, 2, 3]
    found = ng.origin(rows)
    assert len(found) == 1 and found[0][:3] == (0, 0, "blocks.0.in") and found[0][4][0] == 0
    # the TensorMonitor beside it carries the same step indices
    assert og.monitor.read()["steps"].tolist() == [0, 1, 2, 3]
    # the capture holds the launches of the monitor attached THEN
    mg.attach_activation_monitor(None)
    with pytest.raises(hip.SvitHipError, match="attached ActivationMonitor changed after this GraphedTrainStep was built"):
        step([x], y)
    mg.attach_activation_monitor(ng)
    step([x], y)
    assert ng.read()["passes"].tolist() == [4]


def test_f_accumulated_step_k2_gives_two_rows_per_call(monkeypatch):
    """AccumulatedTrainStep with k = 2 under SVIT.REPRODUCIBLE: two rows per call with the same step, equal to the eager
    micro-steps on a second model"""
    from svit_amd import hip, train
    from svit_amd.graph import AccumulatedTrainStep, GraphedTrainStep
    B0, B1, B2 = batch(), batch("B"), batch("C")
    _, mg, og, ng = make(mode="reproducible", method="sgd", period=4, k=2)
    _, me, oe, ne = make(mode="reproducible", method="sgd", period=4, k=2)
    assert ng.period == 8
    micro = GraphedTrainStep(mg, ce, [B0[0]], B0[1], accumulate=True)
    step = AccumulatedTrainStep(mg, [micro, micro], og)
    ng.reset()
    spy = Spy(ne)
    for i, batches in enumerate(([B0, B1], [B2, B0], [B1, B2])):
        batches = [([x], y) for x, y in batches]
        _, names = _trace_names(monkeypatch, lambda: step(batches))
        assert names.count("svit_act_stats") == 0                           # (inside the replays)
        train.accumulate_step(me, [ce, ce], batches, oe)
        torch.cuda.synchronize()
        assert same(mg.flat.data, me.flat.data), i
    assert _entries(ng, range(6)) == _entries(ne, range(6))
    rows = ng.read()
    assert rows["passes"].tolist() == [0, 1, 2, 3, 4, 5] and rows["steps"].tolist() == [0, 0, 1, 1, 2, 2] and rows["lost"] == 0
    raw = ring_rows(ng)
    for i in range(6):
        slots, sites = spy.host(i)
        check_pass(ng, raw[i], slots, sites, "micro-step %d" % i)
    mg.attach_activation_monitor(None)
    with pytest.raises(hip.SvitHipError, match="attached ActivationMonitor changed after this AccumulatedTrainStep was built"):
        step(batches)


def test_g_passes_that_save_nothing_launch_nothing(monkeypatch):
    """the frames pass of a captured step, a GraphedEvalStep and an eager no-grad forward add no launch and no row"""
    from svit_amd.graph import GraphedEvalStep, GraphedTrainStep
    x, y = batch()
    _, model, opt, mon = make()

    def loss_fun(p, e, y):
        return torch.nn.functional.cross_entropy(p, y)
    _, names = _trace_names(monkeypatch, lambda: GraphedTrainStep(model, loss_fun, [x], y, optimizer=opt, frames_pass=True))
    # the clip forward's pair per body, none for the frames pass: 16 + 16 attention launches to one pair
    assert names.count("svit_act_stats") * 32 == names.count("svit_attn_fwd") > 0
    before = int(mon.state[0])
    with torch.no_grad():
        _, names = _trace_names(monkeypatch, lambda: model([x], {}))
    assert "svit_act_stats" not in names
    model.eval()
    _, names = _trace_names(monkeypatch, lambda: GraphedEvalStep(model, [x], y))
    assert "svit_act_stats" not in names
    torch.cuda.synchronize()
    assert int(mon.state[0]) == before


def test_h_without_the_key_a_capture_holds_no_monitor_launch(monkeypatch):
    """no SVIT.ACT_MONITOR: build_actmon gives None, and a capture with the guarded optimizer issues the launches of a
    capture of a second, never-watched model of this tree plus the two of the tail -- no svit_act_* launch among them.
    (Two captures of this tree are compared; the parent's launch names are not recorded anywhere.)"""
    from svit_amd.graph import GraphedTrainStep
    x, y = batch()
    _, ma, opt, mon = make(monitor=False)
    _, mb = build()
    assert mon is None and ma.engine.act_monitor is None
    _, bare = _trace_names(monkeypatch, lambda: GraphedTrainStep(mb, ce, [x], y))
    _, names = _trace_names(monkeypatch, lambda: GraphedTrainStep(ma, ce, [x], y, optimizer=opt))
    tail = ["svit_step_guard", "svit_adamw_step_guarded"]
    assert names[-2:] == tail and names[:-2] == bare and not [n for n in names if n.startswith("svit_act_")]
