"""Attention monitor on the GPU: svit_attn_stats against its NumPy float64 restatement (attnmon.attn_host) on synthetic
sites in svit_attn_fwd's operand convention, with canaries around ring, workspace, counters and maps, and the monitor
carried through the tiny model -- the eager, the captured and the accumulated step, a frozen cut, probe_clip, the other
three monitors and an EMA beside it.  Every bar is derived from the operands (tests/attnmon_cases.py); counts, codes,
headers and every run-to-run comparison are exact.  Needs a real MI355X.

eps_exp as measured on an MI355X over these cases' exponents: see profiles/r26_attnmon_step.txt."""
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import attnmon_cases as A
from tests import test_actmon_gpu as AG          # the tiny model's rig: build, batch, ce, eager_step, _trace_names

DEV = "cuda"
CANARY = 0xA5
PAD = 256
ALL = ("cls", "obj", "patch:32")


def guarded(nbytes, dtype=torch.uint8):
    whole = torch.full((PAD + nbytes + PAD,), CANARY, dtype=torch.uint8, device=DEV)
    return whole, whole[PAD:PAD + nbytes].view(dtype)


class Rig:
    """synthetic sites on the device; ring, workspace, counters and maps between canaries"""

    def __init__(self, sites, rows=ALL, R=4, rec=None, every=1, maps_samples=0, n_slots=None, slots=None):
        from svit_amd import attnmon, ops
        self.host_sites = sites
        self.names, self.kinds, self.K = attnmon.parse_rows(rows)
        self.G = len(self.kinds)
        self.R, self.rec, self.every, self.maps_samples = R, rec, every, maps_samples
        self.slots = list(range(len(sites))) if slots is None else list(slots)
        self.n_slots = len(sites) if n_slots is None else n_slots
        self.dev, self.sites, self.maps, base = [], [], [], 0
        self.guards = []
        for s, slot in zip(sites, self.slots):
            qa, ka, lse = s["qa"].to(DEV), s["ka"].to(DEV), torch.from_numpy(s["lse2"]).to(DEV)
            self.dev.append((qa, ka, lse))
            d = {k: s[k] for k in ("B", "heads", "Nq", "Nk", "DA", "bias_cols", "Lq", "Lk", "n_obj")}
            d.update(qa=qa.data_ptr(), ka=ka.data_ptr(), lse2=lse.data_ptr(), maps=None, slot=slot, ent_base=base)
            base += s["heads"] * self.G
            if maps_samples:
                npb = sum(len(attnmon.group_rows(k, s["Lq"], s["n_obj"], self.K)) for k in self.kinds)
                shape = (min(maps_samples, s["B"]), s["heads"], npb, s["Nk"])
                whole, m = guarded(4 * int(np.prod(shape)), torch.float32)
                self.guards.append(("maps", whole))
                self.maps.append(m.view(shape))
                d["maps"] = m.data_ptr()
            self.sites.append(d)
        self.ent_slots = base
        self.wgs = ops.attn_sites_check(self.sites, self.n_slots, self.ent_slots, self.kinds, self.K, every, maps_samples)
        whole, self.ring = guarded(R * (48 + 64 * self.ent_slots))
        self.guards.append(("ring", whole))
        self.ring.copy_(torch.from_numpy(attnmon.empty_ring(R, self.ent_slots).view(np.uint8).reshape(-1).copy()))
        whole, self.ws = guarded(ops.attn_stats_workspace(self.wgs))
        self.guards.append(("workspace", whole))
        whole, self.state = guarded(32, torch.int64)
        self.guards.append(("state", whole))
        self.state.copy_(torch.tensor([0, 0, -1, 0]))
        self.geom = (sites[0]["B"], 4, 2, 16, 16)

    def launch(self):
        from svit_amd import ops
        before = [[t.clone() for t in d] for d in self.dev]
        rec0 = None if self.rec is None else self.rec.clone()
        ops.attn_stats(self.sites, self.n_slots, self.ent_slots, self.kinds, self.K, self.every, self.maps_samples,
                       self.geom, self.rec, self.ring, self.R, self.state, self.ws)
        torch.cuda.synchronize()
        for d, b in zip(self.dev, before):
            for t, u in zip(d, b):
                assert torch.equal(t.view(torch.uint8), u.view(torch.uint8)), "an operand was written"
        assert rec0 is None or torch.equal(self.rec, rec0), "the step record was written"
        for name, whole in self.guards:
            edge = torch.cat([whole[:PAD], whole[-PAD:]])
            assert bool((edge == CANARY).all()), "a canary beside the %s was overwritten" % name

    def rows(self):
        from svit_amd import attnmon
        return self.ring.cpu().numpy().view(attnmon.row_dtype(self.ent_slots)).copy()

    def entries(self, row, i):
        s = self.sites[i]
        return row["entry"][s["ent_base"]:s["ent_base"] + s["heads"] * self.G]

    def want(self, i):
        s = self.host_sites[i]
        eps = A.measure_eps(A.host_d(s, self.kinds, self.K), DEV)
        return A.host(s, self.kinds, self.K, eps), eps

    def check(self, row, what):
        eps_all = []
        for i in range(len(self.sites)):
            want, eps = self.want(i)
            eps_all.append(eps)
            A.assert_entries(self.entries(row, i), want, "%s, site %d" % (what, i))
            if self.maps_samples:
                A.assert_maps(self.maps[i].cpu().numpy(), want, min(self.maps_samples, self.host_sites[i]["B"]),
                              "%s, maps of site %d" % (what, i))
        print("eps_exp %s: %s" % (what, ["2^%.2f" % math.log2(e) for e in eps_all]))


def head(row):
    h = row["head"]
    return tuple(int(h[k]) for k in ("pass", "step", "B", "Tx", "T0", "H0", "W0", "n_sites", "row", "reserved"))


def rec_at(step, skipped=0):
    rec = torch.zeros(12, dtype=torch.int32, device=DEV)
    rec.view(torch.int64)[0], rec.view(torch.int64)[1] = step - skipped, skipped
    return rec


# ===================================================================================================== kernel ====
@pytest.mark.parametrize("DA,J", [(128, 20), (128, 0), (160, 41), (160, 64)])
def test_a_kernel_is_the_yardstick(DA, J):
    """both widths, bias columns that are and are not a multiple of 8; Nk of 27, 64, 65, 257 and 457 with n_obj 0 and
    8, Lq below, at and above K; every group; maps of every sample; a second run bit for bit"""
    sites = [A.site(2, 2, 26, 26, 0, DA, J, seed=1),            # Nk = 27, no objects, Lq < K
             A.site(2, 1, 55, 55, 8, DA, J, seed=2),            # Nk = 64
             A.site(2, 2, 32, 56, 8, DA, J, seed=3),            # Nk = 65, Lq = K
             A.site(2, 2, 248, 248, 8, DA, J, seed=4),          # Nk = 257
             A.site(2, 1, 100, 456, 0, DA, J, seed=5, sharp=3.0)]   # Nk = 457, sharper rows
    r = Rig(sites, maps_samples=2)
    r.launch()
    rows = r.rows()
    assert head(rows[0]) == (0, -1, 2, 4, 2, 16, 16, 5, 0, 0)
    assert r.state.tolist() == [1, 1, 0, 0]
    r.check(rows[0], "DA %d J %d" % (DA, J))
    assert (rows[0]["entry"]["n_bad"] == 0).all()
    from svit_amd import attnmon
    for k in (1, 2, 3):
        assert rows[k].tobytes() == attnmon.empty_ring(1, r.ent_slots)[0].tobytes(), k
    first, maps = rows[0]["entry"].tobytes(), [m.clone() for m in r.maps]
    r.launch()
    rows = r.rows()
    assert rows[1]["entry"].tobytes() == first and rows[0]["entry"].tobytes() == first
    assert head(rows[1])[:2] == (1, -1) and head(rows[1])[8] == 1 and r.state.tolist() == [2, 2, 1, 0]
    for a, b in zip(maps, r.maps):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))


def test_a_the_largest_key_count_of_the_recipe():
    """Nk = 1633 (16 x 224^2, block 0) at B = h = 1, all 97 probe rows, maps"""
    r = Rig([A.site(1, 1, 1568, 1568, 64, 160, 36, seed=6)], maps_samples=1)
    r.launch()
    row = r.rows()[0]
    r.check(row, "Nk 1633")
    assert row["entry"]["rows"].tolist() == [1, 64, 32]


@pytest.mark.parametrize("rows", [("cls",), ("patch:64",), ("obj", "cls"), ("patch:7", "obj", "cls")])
def test_a_groups(rows):
    """cls alone, patch:K with Lq < K, and other orders of the groups"""
    sites = [A.site(2, 2, 40, 12, 8, 128, 20, seed=7), A.site(2, 1, 9, 9, 0, 160, 0, seed=8)]
    r = Rig(sites, rows=rows, maps_samples=1)
    r.launch()
    r.check(r.rows()[0], "rows %s" % (rows,))


def test_a_closed_form_anchor():
    """qa = 0 and lse2 = log2 Nk: every p is 1 / Nk, so H = log2 Nk, m_cls = 1 / Nk and m_obj = n_obj / Nk -- held
    without the yardstick"""
    s = A.site(2, 2, 30, 50, 8, 128, 20, seed=9)
    s["qa"].zero_()
    Nk = s["Nk"]
    s["lse2"][:] = np.float32(math.log2(Nk))
    r = Rig([s], maps_samples=2)
    r.launch()
    e = r.rows()[0]["entry"]
    n = e["rows"].astype(np.float64)
    L = float(np.float32(math.log2(Nk)))                        # the exponent the kernel sees: d = -L exactly
    p = 2.0 ** -L
    tol = A.measure_eps(np.float32(-L), DEV)                    # the one exponent there is; floored at 2^-23
    assert np.allclose(e["sum_H"] / n, Nk * p * L, rtol=tol, atol=0) and abs(Nk * p * L - math.log2(Nk)) < 1e-5
    assert np.allclose(e["sum_cls"] / n, p, rtol=tol, atol=0) and abs(p * Nk - 1) < 1e-5
    assert np.allclose(e["sum_obj"] / n, 8 * p, rtol=tol, atol=0)
    assert np.allclose(e["sum_pmax"] / n, p, rtol=tol, atol=0)
    assert np.allclose(r.maps[0].cpu().numpy(), p, rtol=tol, atol=0)
    assert e["rows"].tolist() == [2, 16, 60] * 2 and (e["n_bad"] == 0).all()


def test_a_columns_past_the_bias_do_not_count():
    """NaN and inf in qa / ka columns >= 96 + J: the row of entries is bit for bit the one without them"""
    s = A.site(2, 2, 40, 40, 8, 128, 19, seed=10)
    r = Rig([s], maps_samples=2)
    r.launch()
    clean, maps = r.rows()[0]["entry"].tobytes(), r.maps[0].clone()
    t = {k: s[k] for k in s}
    t["qa"], t["ka"] = s["qa"].clone(), s["ka"].clone()
    t["qa"][..., 96 + 19:] = float("nan")
    t["ka"][..., 96 + 19:] = float("inf")
    t["ka"][0, 1, 3, 96 + 19] = float("nan")
    r2 = Rig([t], maps_samples=2)
    r2.launch()
    assert r2.rows()[0]["entry"].tobytes() == clean
    assert torch.equal(r2.maps[0].view(torch.int32), maps.view(torch.int32))
    assert (r2.rows()[0]["entry"]["n_bad"] == 0).all()


@pytest.mark.parametrize("where", ["first", "last"])
def test_a_bad_rows(where):
    """a NaN lse2, an inf lse2 and a NaN key, on the first and on the last probe row / key: n_bad and first_bad, and the
    other rows stay readable"""
    from svit_amd import attnmon
    s = A.site(2, 2, 40, 40, 8, 128, 20, seed=11)
    _, kinds, K = attnmon.parse_rows(ALL)
    probe = np.concatenate([attnmon.group_rows(k, 40, 8, K) for k in kinds])
    q = int(probe.min() if where == "first" else probe.max())          # the cls row / the last object row
    s["lse2"][0, 0, q] = np.nan
    s["lse2"][1, 1, q] = -np.inf if where == "first" else np.inf
    r = Rig([s])
    r.launch()
    row = r.rows()[0]
    r.check(row, "bad lse2, %s" % where)
    e = row["entry"].reshape(2, 3)                                       # [head, group]
    g = 0 if where == "first" else 1
    assert e["n_bad"][0, g] == 1 and e["first_bad"][0, g] == q and e["n_bad"][1, g] == 1 and e["first_bad"][1, g] == 49 + q
    assert e["n_bad"].sum() == 2
    # a NaN key spoils every probe row of its (sample, head) and no other
    t = A.site(2, 2, 40, 40, 8, 128, 20, seed=12)
    k = 0 if where == "first" else t["Nk"] - 1
    t["ka"][1, 0, k, 5] = float("nan")
    r = Rig([t])
    r.launch()
    row = r.rows()[0]
    r.check(row, "NaN key, %s" % where)
    e = row["entry"].reshape(2, 3)
    assert e["n_bad"].tolist() == [[1, 8, 32], [0, 0, 0]] and e["first_bad"][0].tolist() == [49, 49 + 41, 49 + 1]
    assert (e["rows"] - e["n_bad"] > 0).all() and np.isfinite(e["sum_H"]).all()


def test_a_exponents_below_the_normal_range():
    """rows whose every d lies below -126: the probabilities flush, the sums stay inside the bar's absolute term"""
    s = A.site(2, 1, 20, 20, 8, 128, 20, seed=13)
    s["lse2"][0] += np.float32(140.0)
    s["lse2"][1, 0, 0] += np.float32(300.0)
    r = Rig([s], maps_samples=2)
    r.launch()
    row = r.rows()[0]
    r.check(row, "d < -126")
    assert (row["entry"]["n_bad"] == 0).all() and row["entry"]["sum_dev"].max() <= 1.0


def test_a_every_3_with_a_dropped_step():
    """every = 3 over optimizer steps 0 .. 6, step 4 dropped (applied + skipped still advances): rows for steps 0, 3 and
    6 alone; the passes that are not due leave ring, rows-written counter and workspace untouched"""
    s = A.site(2, 2, 40, 40, 8, 128, 20, seed=14)
    rec = rec_at(0)
    r = Rig([s], rec=rec, every=3, R=4, maps_samples=1)
    want = None
    skipped = 0
    for step in range(7):
        skipped += step == 5                                     # (step 4 was dropped: the record says so from step 5 on)
        rec.copy_(rec_at(step, skipped))
        ring0, ws0 = r.ring.clone(), r.ws.clone()
        r.launch()
        if step % 3:
            assert torch.equal(r.ring, ring0) and torch.equal(r.ws, ws0), step
    rows = r.rows()
    assert [head(x)[:2] for x in rows] == [(0, 0), (3, 3), (6, 6), (-1, -1)]
    assert [head(x)[8] for x in rows[:3]] == [0, 1, 2] and r.state.tolist() == [7, 3, 6, 0]
    for k in range(3):
        r.check(rows[k], "every 3, row %d" % k)
    # without a record the due rule reads the pass counter
    bare = Rig([s], every=3, R=4)
    for _ in range(5):
        bare.launch()
    assert [head(x)[:2] for x in bare.rows()] == [(0, -1), (3, -1), (-1, -1), (-1, -1)] and bare.state.tolist() == [5, 2, -1, 0]


def test_a_ring_of_two_rows_overrun():
    from svit_amd import attnmon
    s = A.site(2, 2, 40, 40, 8, 128, 20, seed=15)
    r = Rig([s], R=2, rec=rec_at(7))
    for _ in range(3):
        r.launch()
    rows = r.rows()
    assert [head(x)[0] for x in rows] == [2, 1] and [head(x)[8] for x in rows] == [2, 1] and r.state.tolist()[:2] == [3, 3]
    got, lost, last = attnmon.read_rows(rows, -1)
    assert got["head"]["pass"].tolist() == [1, 2] and lost == 1 and last == 2


@pytest.mark.parametrize("samples", [0, 1, 2])
def test_a_maps_samples(samples):
    s = A.site(2, 2, 40, 40, 8, 128, 20, seed=16)
    r = Rig([s], maps_samples=samples)
    r.launch()
    r.check(r.rows()[0], "maps_samples %d" % samples)
    assert r.state.tolist()[2] == (0 if samples else -1)


def test_a_absent_slots_and_a_reused_row():
    """a pass whose table names fewer sites leaves the empty entry where the earlier pass of that ring row wrote"""
    from svit_amd import attnmon
    a, b = A.site(2, 2, 40, 40, 8, 128, 20, seed=17), A.site(2, 1, 20, 20, 8, 128, 20, seed=18)
    r = Rig([a, b], R=1)
    r.launch()
    full = r.rows()[0]["entry"].copy()
    assert (full["n_bad"] == 0).all()
    r.sites = r.sites[1:]
    r.launch()
    e = r.rows()[0]["entry"]
    assert e[:6].tobytes() == np.full(6, attnmon.empty_entry()).tobytes() and e[6:].tobytes() == full[6:].tobytes()


# ======================================================================================================= model ====
def make(rows=ALL, every=1, maps=0, cut=0, mode="deterministic", method="adamw", period=8, k=1, others=False):
    from svit_amd import actmon, attnmon, optim, updmon
    from svit_amd import ema as ema_mod
    from svit_amd import monitor as mon_mod
    cfg, model = AG.build(mode)
    if cut:
        model.freeze_below(cut)
    s = cfg.SOLVER
    s.OPTIMIZING_METHOD, s.BASE_LR, s.WEIGHT_DECAY, s.CLIP_GRAD_L2NORM = method, AG.LR if method != "sgd" else 0.05, 1e-4, 1.0
    s.MOMENTUM, s.DAMPENING, s.NESTEROV = 0.9, 0.0, True
    cfg.LOG_PERIOD = period
    cfg.SVIT.GUARDED_STEP = True
    cfg.SVIT.ATTN_MONITOR, cfg.SVIT.ATTN_MONITOR_ROWS = True, rows
    cfg.SVIT.ATTN_MONITOR_EVERY, cfg.SVIT.ATTN_MONITOR_MAPS = every, maps
    if others:
        cfg.SVIT.ACT_MONITOR = cfg.SVIT.MONITOR = cfg.SVIT.UPDATE_MONITOR = True
        cfg.SVIT.EMA_DECAY = 0.9
    opt = optim.construct_optimizer(model, cfg)
    if others:
        ema_mod.build_ema(cfg, model, opt)
        mon_mod.build_monitor(cfg, opt)
        updmon.build_update_monitor(cfg, opt)
        actmon.build_actmon(cfg, model, opt, virtual_ranks=k)
    mon = attnmon.build_attnmon(cfg, model, opt, virtual_ranks=k)
    assert model.engine.attn_monitor is mon
    return cfg, model, opt, mon


class Spy:
    """keeps the operands every `mon.enqueue(st)` saw, as host copies taken on the spot (the next pass reuses nothing,
    but a weight update must not be waited for), in pass order"""

    def __init__(self, mon):
        self.mon, self.seen, self.real = mon, [], mon.enqueue
        mon.enqueue = self

    def __call__(self, st):
        sites, keep = self.mon.sites_of(st)
        self.seen.append((sites, [(qa.detach().clone(), ka.detach().clone(), l.detach().clone()) for qa, ka, l in keep]))
        return self.real(st)


def ring_rows(mon):
    from svit_amd import attnmon
    torch.cuda.synchronize()
    return mon.ring.cpu().numpy().view(attnmon.row_dtype(mon.ent_slots)).copy()


def check_pass(mon, row, seen, what, maps=None):
    """one ring row against attn_host on the forward's own operands"""
    sites, keep = seen
    owned = np.zeros(mon.ent_slots, dtype=bool)
    for s, (qa, ka, lse) in zip(sites, keep):
        args = (qa.cpu(), ka.cpu(), lse.cpu().numpy(), s["Lq"], s["Lk"], s["n_obj"], s["bias_cols"], mon.kinds, mon.K)
        d = mon.attn_host(*args)["per_row"]["d"]
        want = mon.attn_host(*args, eps_exp=A.measure_eps(d, DEV))
        sl = slice(s["ent_base"], s["ent_base"] + s["heads"] * len(mon.kinds))
        owned[sl] = True
        A.assert_entries(row["entry"][sl], want, "%s, block %d" % (what, s["slot"]))
        if maps is not None:
            A.assert_maps(maps[s["slot"]].cpu().numpy(), want, maps[s["slot"]].shape[0], "%s, maps of block %d" % (what, s["slot"]))
    assert (row["entry"]["n_bad"][~owned] == -1).all() and (row["entry"]["n_bad"][owned] >= 0).all(), what


def test_d_three_eager_steps_every_entry_against_the_yardstick():
    """(on the parent commit there is no svit_amd.attnmon)"""
    x, y = AG.batch()
    cfg, model, opt, mon = make(maps=2)
    assert mon.depth == 16 and mon.period == 8 and mon.ent_slots == 3 * sum(b.heads for b in model.plan.blocks)
    spy = Spy(mon)
    for i in range(3):
        AG.eager_step(model, opt, x, y)
    raw = ring_rows(mon)
    p, maps = mon.maps()
    assert p == 2 and sorted(maps) == list(range(16))
    for i in range(3):
        assert len(spy.seen[i][0]) == 16
        check_pass(mon, raw[i], spy.seen[i], "eager step %d" % i, maps if i == 2 else None)
        assert head(raw[i]) == (i, i, 2, 4, 2, 16, 16, 16, i, 0)
    rows = mon.read()
    assert rows["passes"].tolist() == [0, 1, 2] and rows["steps"].tolist() == [0, 1, 2] and rows["lost"] == 0
    assert (rows["n_bad"].data == 0).all() and not np.ma.getmaskarray(rows["entropy"]).any()
    assert bool((rows["entropy_norm"] > 0).all()) and bool((rows["entropy_norm"] <= 1 + 1e-6).all())
    mass = rows["mass_cls"] + rows["mass_obj"] + rows["mass_patch"]
    # svit_attn_fwd sums its row on the matrix pipe from the bf16 P fragments: every term within 2^-9 of its p, so its
    # lse2 puts the probe's sum within 2^-9 (+ fp32 accumulation) of 1 -- and a layout mistake would put it far outside
    assert np.allclose(mass, 1.0, atol=2.0 ** -8) and float(rows["sum_dev"].max()) < 2.0 ** -8
    assert not np.array_equal(rows["entropy"].data[0], rows["entropy"].data[2])              # the weights moved
    assert mon.collapsed(rows, 0.0) == [] and len(mon.collapsed(rows, 2.0)) == 3 * mon.ent_slots
    line = mon.log_stats(rows)
    assert line["_type"] == "train_attention_stats" and line["pass"] == 2 and len(line["entropy_norm"]["cls"]) == 16
    b, hd, g = rows["index"][5]
    at = mon.where(rows["header"][0], b, hd, int(rows["min_row"][0][5]))
    assert at[1] == hd and 0 <= at[0] < 2
    assert mon.read()["passes"].tolist() == []


def test_d_maps_against_the_dense_float64_forward():
    """the independent anchor: the map rows of block 3 against P of tests/attn_reference.py's float64 dense forward on the
    same qa and ka, with lse2 from ops.attn_fwd"""
    from svit_amd import engine, ops
    from tests import attn_reference as R
    x, y = AG.batch()
    _, model, opt, mon = make(maps=2)
    with torch.no_grad():
        _, st = model.engine.forward(x, None, save=True)
    torch.cuda.synchronize()
    _, maps = mon.maps()
    for blk in (0, 3, 15):
        sv = st["blocks"][blk]
        qa, ka, v = sv["pools"][0][0], sv["pools"][1][0], sv["pools"][2][0]
        J = sum(sv["k_thw"])
        _, lse2 = ops.attn_fwd(qa, ka, v, engine.SCALE, bias_cols=J)
        assert torch.equal(lse2.view(torch.int32), sv["lse2"].view(torch.int32))
        _, _, lse_ref, P = R.reference_fwd(qa.cpu(), ka.cpu(), v.cpu(), J)
        probe, _ = mon.probe_rows(blk, geom=(st["Tx"],) + tuple(st["thw0"]))
        # the reference normalises by its own float64 log-sum-exp, the probe by the lse2 svit_attn_fwd stored
        want = (P * torch.exp2(lse_ref - lse2.cpu().double())[..., None])[:, :, probe, :].numpy()
        Lq, Lk = int(np.prod(sv["q_thw"])), int(np.prod(sv["k_thw"]))
        args = (qa.cpu(), ka.cpu(), lse2.cpu().numpy(), Lq, Lk, st["n_obj"], J, mon.kinds, mon.K)
        eps = A.measure_eps(mon.attn_host(*args)["per_row"]["d"], DEV)
        bound = mon.attn_host(*args, eps_exp=eps)["per_row"]["b_map"]
        got = maps[blk].cpu().numpy().astype(np.float64)
        assert got.shape == want.shape and (np.abs(got - want) <= bound).all(), (blk, float(np.abs(got - want).max()))


def test_e_frozen_cut_4_contributes_no_site_below():
    x, y = AG.batch()
    _, model, opt, mon = make(cut=4)
    spy = Spy(mon)
    AG.eager_step(model, opt, x, y)
    row = ring_rows(mon)[0]
    assert [s["slot"] for s in spy.seen[0][0]] == list(range(3, 16)) and row["head"]["n_sites"] == 13
    check_pass(mon, row, spy.seen[0], "cut 4")
    rows = mon.read()
    below = [e for e, (b, _, _) in enumerate(rows["index"]) if b < 3]
    assert np.ma.getmaskarray(rows["entropy"])[0][below].all() and (rows["n_bad"].data[0][below] == -1).all()


def _entries(mon, passes):
    raw = ring_rows(mon)
    by = {int(r["head"]["pass"]): r for r in raw if r["head"]["pass"] >= 0}
    return [(int(by[p]["head"]["step"]), by[p]["entry"].tobytes()) for p in passes]


def test_f_graphed_step_replays_the_monitor(monkeypatch):
    """the captured step over a poisoned first replay and two more equals the eager step in rows, maps, weights and
    moments, the other three monitors and an EMA attached beside it; a replay after the attachment changed is refused"""
    from svit_amd import hip, optim
    from svit_amd.graph import GraphedTrainStep
    poison = torch.ones(1, device=DEV)

    def loss_fun(p, e, y):
        return torch.nn.functional.cross_entropy(p, y) * poison

    x, y = AG.batch()
    bad = x.clone()
    bad[0, 0, 1, 5, 7] = float("nan")
    _, mg, og, ng = make(maps=1, others=True)
    _, me, oe, ne = make(maps=1, others=True)
    step, names = AG._trace_names(monkeypatch, lambda: GraphedTrainStep(mg, loss_fun, [x], y, optimizer=og))
    assert names.count("svit_attn_stats") == names.count("svit_act_stats") > 0
    for i, n in enumerate(names):
        if n == "svit_attn_stats":
            assert names[i - 1] == "svit_act_stats"                        # directly behind the activation monitor's
    ng.reset()
    og.act_monitor.reset()
    for i, inp in enumerate((bad, x, x)):
        optim.set_lr(og, AG.LR * (i + 1))
        optim.set_lr(oe, AG.LR * (i + 1))
        lg, _ = step([inp], y)
        le = AG.eager_step(me, oe, inp, y, loss_fun)
        torch.cuda.synchronize()
        assert (i == 0 or AG.same(lg, le)) and AG.same(mg.flat.data, me.flat.data), i
    assert og.stats() == oe.stats() and og.stats()["skipped"] == 1
    for k in og.STATE:
        assert AG.same(getattr(og, k), getattr(oe, k)), k
    assert _entries(ng, range(3)) == _entries(ne, range(3))
    (pg, mapg), (pe, mape) = ng.maps(), ne.maps()
    assert pg == pe == 2
    for b in mapg:
        assert torch.equal(mapg[b].view(torch.int32), mape[b].view(torch.int32)), b
    rows = ng.read()
    assert rows["passes"].tolist() == [0, 1, 2] and rows["steps"].tolist() == [0, 1, 2]
    assert rows["n_bad"].data[0].max() > 0 and (rows["n_bad"].data[1:] == 0).all()      # the NaN pixel's pass
    assert og.monitor.read()["steps"].tolist() == [0, 1, 2]
    mg.attach_attention_monitor(None)
    with pytest.raises(hip.SvitHipError, match="attached AttentionMonitor changed after this GraphedTrainStep was built"):
        step([x], y)
    mg.attach_attention_monitor(ng)
    step([x], y)
    assert ng.read()["passes"].tolist() == [3]


def test_f_accumulated_step_k2_gives_two_rows_per_call(monkeypatch):
    from svit_amd import hip, train
    from svit_amd.graph import AccumulatedTrainStep, GraphedTrainStep
    B0, B1, B2 = AG.batch(), AG.batch("B"), AG.batch("C")
    _, mg, og, ng = make(mode="reproducible", method="sgd", period=4, k=2)
    _, me, oe, ne = make(mode="reproducible", method="sgd", period=4, k=2)
    assert ng.period == 8
    micro = GraphedTrainStep(mg, AG.ce, [B0[0]], B0[1], accumulate=True)
    step = AccumulatedTrainStep(mg, [micro, micro], og)
    ng.reset()
    for i, batches in enumerate(([B0, B1], [B2, B0])):
        batches = [([x], y) for x, y in batches]
        _, names = AG._trace_names(monkeypatch, lambda: step(batches))
        assert names.count("svit_attn_stats") == 0                          # (inside the replays)
        train.accumulate_step(me, [AG.ce, AG.ce], batches, oe)
        torch.cuda.synchronize()
        assert AG.same(mg.flat.data, me.flat.data), i
    assert _entries(ng, range(4)) == _entries(ne, range(4))
    rows = ng.read()
    assert rows["passes"].tolist() == [0, 1, 2, 3] and rows["steps"].tolist() == [0, 0, 1, 1] and rows["lost"] == 0
    mg.attach_attention_monitor(None)
    with pytest.raises(hip.SvitHipError, match="attached AttentionMonitor changed after this AccumulatedTrainStep was built"):
        step(batches)


def test_g_passes_that_save_nothing_launch_nothing(monkeypatch):
    from svit_amd.graph import GraphedEvalStep, GraphedTrainStep
    x, y = AG.batch()
    _, model, opt, mon = make()
    _, names = AG._trace_names(monkeypatch, lambda: GraphedTrainStep(model, AG.ce, [x], y, optimizer=opt, frames_pass=True))
    assert names.count("svit_attn_stats") * 32 == names.count("svit_attn_fwd") > 0
    before = int(mon.state[0])
    with torch.no_grad():
        _, names = AG._trace_names(monkeypatch, lambda: model([x], {}))
    assert "svit_attn_stats" not in names
    model.eval()
    _, names = AG._trace_names(monkeypatch, lambda: GraphedEvalStep(model, [x], y))
    assert "svit_attn_stats" not in names
    torch.cuda.synchronize()
    assert int(mon.state[0]) == before


def test_g_probe_clip():
    from svit_amd import attnmon
    x, y = AG.batch()
    _, model = AG.build()
    assert model.engine.attn_monitor is None
    maps = attnmon.probe_clip(model, x, rows=("cls", "obj"), samples=1)
    assert model.engine.attn_monitor is None and sorted(maps) == list(range(16))
    for b, (probe, m) in maps.items():
        assert m.shape[0] == 1 and m.shape[2] == len(probe) == 1 + 16 and probe[0] == 0
        assert float((m.sum(-1) - 1).abs().max()) < 2.0 ** -8           # (svit_attn_fwd's bf16 row sum: see test_d)
    again = attnmon.probe_clip(model, x, rows=("cls", "obj"), samples=1)
    for b in maps:
        assert torch.equal(maps[b][1].view(torch.int32), again[b][1].view(torch.int32))


def test_h_without_the_key_a_capture_holds_no_monitor_launch(monkeypatch):
    from svit_amd import attnmon
    from svit_amd.graph import GraphedTrainStep
    x, y = AG.batch()
    cfg, ma, opt, _ = AG.make(monitor=False)
    assert attnmon.build_attnmon(cfg, ma, opt) is None and ma.engine.attn_monitor is None
    _, mb = AG.build()
    _, bare = AG._trace_names(monkeypatch, lambda: GraphedTrainStep(mb, AG.ce, [x], y))
    _, names = AG._trace_names(monkeypatch, lambda: GraphedTrainStep(ma, AG.ce, [x], y, optimizer=opt))
    assert names[:-2] == bare and not [n for n in names if n.startswith("svit_attn_stats")]
