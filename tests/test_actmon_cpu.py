"""Activation monitor, host side: the site-table validator and every argument refusal of svit_act_stats by error code,
the workspace query, the NumPy yardstick on hand-made sites, three mutants of it against the bar, slot names / where() /
origin() on the real plan at 16 x 224^2 and at T = 1, read() and `lost` on rings filled by hand, check()'s message and
build_actmon's refusals.  No GPU needed."""
import json
import os
import types

import numpy as np
import pytest
import torch

from tests import actmon_cases as A

NAN, INF = np.float32("nan"), np.float32("inf")


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__
    __graft_entry__.build()
    from svit_amd import hip
    return hip.load()


def f32(*v):
    return np.array(v, dtype=np.float32)


def golden_plan():
    """the plan of the recipe the golden config tree describes (16 x 224^2, depth 16)"""
    from svit_amd import arch, config
    ref = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "cfg.json")))["merged"]
    cfg = config.ssv2_cfg()
    assert cfg.DATA.NUM_FRAMES == ref["DATA"]["NUM_FRAMES"] == 16 and cfg.MVIT.DEPTH == ref["MVIT"]["DEPTH"] == 16
    assert cfg.DATA.TRAIN_CROP_SIZE == ref["DATA"]["TRAIN_CROP_SIZE"] == 224 and cfg.SVIT.O == ref["SVIT"]["O"]
    return cfg, arch.build_plan(cfg)


def _cpu_model():
    """an SViT that has not left the CPU, with the real FlatParams placement over untouched CPU memory and a stand-in for
    the engine's one attribute the monitor's attachment touches"""
    from svit_amd import arch, config
    from svit_amd.engine import FlatParams
    from svit_amd.model import MODEL_REGISTRY
    cfg = config.ssv2_cfg(num_frames=4, crop=64)
    model = MODEL_REGISTRY.get("SViT")(cfg)
    shapes = {n: tuple(p.shape) for n, p in model.named_parameters()}
    model.flat = FlatParams(shapes, model.weight_decayed, torch.device("cpu"), arch.readiness_rank)
    for n, p in model.named_parameters():
        model.flat.p(n).copy_(p.data)
        p.data = model.flat.p(n)
    model.engine = types.SimpleNamespace(act_monitor=None)
    return cfg, model


# ------------------------------------------------------------------------------------------------- the validator ----
P = 4096        # a made-up device address that is never followed


def _table(sites):
    from svit_amd import ops
    return ops.act_site_table([s[:3] for s in sites], [s[3] for s in sites])


def test_sites_check_by_error_code(lib):
    import ctypes

    def check(sites, n_slots=8, n_sites=None, null=False, null_slots=False):
        tab, sl = _table(sites)
        w = ctypes.c_int64(-7)
        rc = lib.svit_act_sites_check(None if null else tab, None if null_slots else sl.ctypes.data,
                                      len(sites) if n_sites is None else n_sites, n_slots, ctypes.byref(w))
        return rc, w.value

    good = [(P, P + 4, 1, 0), (P, None, 4096, 3), (P + 8, P, 4097, 1), (P, None, 1 << 24, 7)]
    assert check(good) == (0, 1 + 1 + 2 + 4096)
    assert check([(P, P, 4, i) for i in range(96)], n_slots=96) == (0, 96)            # the limit itself
    assert check([(P, P, 4, 1023)], n_slots=1024)[0] == 0
    bad_arg = {
        "NULL table": dict(sites=good, null=True), "NULL slots": dict(sites=good, null_slots=True),
        "no site": dict(sites=good, n_sites=0), "n_sites < 0": dict(sites=good, n_sites=-1),
        "97 sites": dict(sites=[(P, P, 4, i) for i in range(97)], n_slots=128),
        "n_slots = 0": dict(sites=good, n_slots=0), "n_slots = 1025": dict(sites=good, n_slots=1025),
        "NULL a": dict(sites=[(P, P, 4, 0), (None, P, 4, 1)]), "NULL a of an lse site": dict(sites=[(None, None, 4, 0)]),
        "rows = 0": dict(sites=[(P, P, 0, 0)]), "rows < 0": dict(sites=[(P, None, -4, 0)]),
        "rows = 2^24 + 1": dict(sites=[(P, P, (1 << 24) + 1, 0)]),
        "slot = n_slots": dict(sites=[(P, P, 4, 8)]), "slot < 0": dict(sites=[(P, P, 4, -1)]),
        "a slot twice": dict(sites=[(P, P, 4, 2), (P, None, 4, 2)]),
        "NULL a and misaligned b": dict(sites=[(None, P + 2, 4, 0)]),               # the argument error is reported first
    }
    for label, kw in bad_arg.items():
        assert check(**kw)[0] == -4, label
    for label, sites in {"a": [(P + 2, P, 4, 0)], "b": [(P, P + 1, 4, 0)], "a later site": good + [(P + 3, None, 4, 2)]}.items():
        assert check(sites)[0] == -3, label
    from svit_amd import hip, ops
    assert ops.act_sites_check([g[:3] for g in good], [g[3] for g in good], 8) == 4100
    with pytest.raises(hip.SvitHipError, match="svit_act_sites_check .* bad alignment"):
        ops.act_sites_check([(P + 2, P, 4)], [0], 8)
    with pytest.raises(hip.SvitHipError, match="svit_act_sites_check .* bad argument"):
        ops.act_sites_check([(P, P, 4), (P, P, 4)], [1, 1], 8)


def test_workspace_query(lib):
    from svit_amd import hip, ops
    assert ops.act_stats_window() == 4096
    q = lib.svit_act_stats_workspace
    assert q(1) == 32 and q(49) == 49 * 32 and q(96 * 4096) == 96 * 4096 * 32 and ops.act_stats_workspace(600) == 19200
    for w in (0, -1, 96 * 4096 + 1):
        assert q(w) == -4, w
    with pytest.raises(hip.SvitHipError, match="svit_act_stats_workspace .* bad argument"):
        ops.act_stats_workspace(0)


def test_entry_point_checks_its_arguments_without_a_gpu(lib):
    """refused before any HIP call: stream = None and made-up device addresses that are never followed"""
    good = [(P, P + 4, 5000, 0), (P, None, 4096, 2)]
    need = 3 * 32
    geom = np.array([2, 4, 2, 16, 16], dtype=np.int32)

    def stats(sites=good, n_slots=4, g=True, rec=P, ring=P, R=4, state=P, ws=P, ws_bytes=need):
        tab, sl = _table(sites)
        return lib.svit_act_stats(tab, sl.ctypes.data, len(sites), n_slots, geom.ctypes.data if g else None, rec, ring, R,
                                  state, ws, ws_bytes, None)

    bad_arg = {
        "NULL geom": dict(g=False), "NULL ring": dict(ring=None), "NULL state": dict(state=None),
        "NULL workspace": dict(ws=None), "R = 0": dict(R=0), "R < 0": dict(R=-1),
        "workspace one byte short": dict(ws_bytes=need - 1), "workspace negative": dict(ws_bytes=-1),
        "97 sites": dict(sites=[(P, P, 4, i) for i in range(97)], n_slots=128, ws_bytes=1 << 20),
        "NULL a": dict(sites=[(None, P, 4, 0)]), "rows = 0": dict(sites=[(P, P, 0, 0)]),
        "rows = 2^24 + 1": dict(sites=[(P, P, (1 << 24) + 1, 0)], ws_bytes=1 << 20),
        "slot outside": dict(sites=[(P, P, 4, 4)]), "a slot twice": dict(sites=[(P, P, 4, 1), (P, P, 4, 1)]),
    }
    for label, kw in bad_arg.items():
        assert stats(**kw) == -4, label
    bad_align = {"a": dict(sites=[(P + 1, P, 4, 0)]), "b": dict(sites=[(P, P + 2, 4, 0)]), "ring": dict(ring=P + 8),
                 "workspace": dict(ws=P + 8), "state": dict(state=P + 4), "dev_rec": dict(rec=P + 4)}
    for label, kw in bad_align.items():
        assert stats(**kw) == -3, label
    # the limits themselves pass the checks: shown through the one check that comes after them (a misaligned ring)
    for kw in (dict(), dict(rec=None), dict(R=1), dict(sites=[(P, P, 4, i) for i in range(96)], n_slots=96, ws_bytes=96 * 32),
               dict(sites=[(P, None, 1 << 24, 0)], ws_bytes=4096 * 32)):
        assert stats(ring=P + 8, **kw) == -3, kw


# ------------------------------------------------------------------------------------------------- the yardstick ----
def test_acts_host_on_hand_made_sites():
    from svit_amd import actmon
    denormal = np.float32(1e-41)
    sites = [
        (f32(0.5), f32(2.0)),                                               # 0 a single row
        (f32(3.0), None),                                                   # 1 a single lse row
        (f32(0.0, 1.0, -2.0, 0.25), f32(4.0, 0.5, 0.5, 1.0)),               # 2 a tie in ext: rows 1 and 2
        (f32(-1.0, 7.0, 7.0, -0.0, 0.0), None),                             # 3 a tie in ext; -0.0 below +0.0
        (f32(NAN, 1.0), f32(1.0, INF)),                                     # 4 all rows bad
        (f32(INF, -INF, NAN), None),                                        # 5 all rows bad
        (f32(NAN, INF, -INF, 1.0, 2.0, 3.0, 0.5), f32(1.0, 1.0, 1.0, NAN, INF, -INF, 0.5)),      # 6 NaN, +inf, -inf
        (f32(1.0, 1.0, 1.0, -3.0), f32(0.0, -0.0, -2.0, 0.25)),             # 7 rstd 0, -0 and negative
        (f32(0.0, 0.0), f32(denormal, 1.0)),                                # 8 a denormal rstd: a good, very wide row
        (f32(-0.0, 0.0), None),                                             # 9 the larger zero is +0.0
        (f32(-5.0, -INF, -7.0), None),                                      # 10 negative values
    ]
    e, mass = actmon.acts_host(sites)

    def row(i):
        return (float(e["sum"][i]), float(e["ext"][i]), float(e["ext2"][i]), int(e["arg"][i]), int(e["n_bad"][i]),
                int(e["first_bad"][i]), int(e["rows"][i]))
    assert row(0) == (0.5, 2.0, 0.5, 0, 0, -1, 1)
    assert row(1) == (3.0, 3.0, 0.0, 0, 0, -1, 1)
    assert row(2) == (0.0625 + 5.0 + 8.0 + 1.0625, 0.5, 2.0, 1, 0, -1, 4)
    assert row(3) == (13.0, 7.0, 0.0, 1, 0, -1, 5)
    assert row(4) == (0.0, 0.0, 0.0, -1, 2, 0, 2)
    assert row(5) == (0.0, 0.0, 0.0, -1, 3, 0, 3)
    assert row(6) == (4.25, 0.5, 0.5, 6, 6, 0, 7)
    assert row(7) == (25.0, 0.25, 3.0, 3, 3, 0, 4)
    d = float(denormal)
    assert row(8) == (1.0 / (d * d) + 1.0, d, 0.0, 0, 0, -1, 2) and np.isfinite(e["sum"][8]) and e["sum"][8] > 1e81
    assert row(9)[1:4] == (0.0, 0.0, 1) and not np.signbit(e["ext"][9])
    assert row(10) == (-12.0, -5.0, 0.0, 0, 1, 1, 3)
    assert mass[10] == 12.0 and mass[3] == 15.0 and mass[6] == 4.25 and mass[4] == 0.0
    assert e.dtype == actmon.ENTRY and actmon.ActivationMonitor.acts_host is actmon.acts_host
    # the empty entry and the empty ring
    ring = actmon.empty_ring(2, 3)
    assert ring.itemsize == 48 + 32 * 3 and (ring["head"]["pass"] == -1).all() and (ring["head"]["step"] == -1).all()
    z = ring["entry"][1][2]
    assert (z["sum"], z["ext"], z["ext2"], z["arg"], z["n_bad"], z["first_bad"], z["rows"]) == (0, 0, 0, -1, -1, -1, 0)


def test_three_mutants_miss_the_bar_by_ten_times():
    """on the synthetic case the GPU test runs: each mistake moves some site's sum by more than 10 x the bar"""
    from svit_amd import actmon
    W = 4096
    s, where = A.sites(W)
    A.ties(s, where)
    A.bad_rows(s, where, W)
    want, mass = actmon.acts_host(s)
    right = A.mutant_sums(s, None, W)
    assert (np.abs(right - want["sum"]) <= A.BAR * mass).all()               # the restatement's restatement agrees
    for which, sites in (("rstd", ["ln 1", "ln W", "ln 3 W + 5"]), ("zero_mean", ["ln 3 W + 5", "ln W + 1"]),
                         ("window", ["lse W + 1", "ln 3 W + 5", "lse 3 W + 5"])):       # (one row of 4097 suffices)
        got = A.mutant_sums(s, which, W)
        for name in sites:
            i = where[name]
            assert abs(got[i] - want["sum"][i]) >= 10 * A.BAR * mass[i], (which, name)


def test_cases_are_what_the_issue_lists():
    from svit_amd import actmon
    W = 4096
    s, where = A.sites(W)
    assert sorted(len(a) for a, _ in s) == sorted([1, 3, 4095, 4096, 4097, 3 * 4096 + 5] * 2)
    assert sum(b is None for _, b in s) == 6
    args = A.ties(s, where)
    bad = A.bad_rows(s, where, W)
    e, _ = actmon.acts_host(s)
    for i, arg in args.items():
        assert e["arg"][i] == arg
    assert {i: (int(e["n_bad"][i]), int(e["first_bad"][i])) for i in np.flatnonzero(e["n_bad"] > 0)} == bad
    none_good = [where["ln 3"], where["lse 1"]]
    assert (e["arg"][none_good] == -1).all() and (e["ext"][none_good] == 0).all() and (e["sum"][none_good] == 0).all()


# -------------------------------------------------------------------------------------------- names, where, origin ----
def header(B, Tx, T0, H0, W0):
    from svit_amd import actmon
    h = np.zeros((), dtype=actmon.HEADER)
    h["B"], h["Tx"], h["T0"], h["H0"], h["W0"] = B, Tx, T0, H0, W0
    return h


def test_slot_names_and_geometry_on_the_real_plan():
    from svit_amd import actmon
    cfg, plan = golden_plan()
    names = actmon.slot_names(len(plan.blocks))
    assert len(names) == 49 and names[:4] == ["blocks.0.in", "blocks.0.attn_lse", "blocks.0.mid", "blocks.1.in"]
    assert names[-2:] == ["blocks.15.mid", "norm.in"] and len(actmon.slot_names(24)) == 73
    O = plan.objects
    geo = actmon.slot_geometry(plan, 16, 8, 56, 56)
    assert geo[0] == (None, (8, 56, 56), 16 * O) and geo[1] == (1, (8, 56, 56), 16 * O)
    assert geo[3 * 1 + 1] == (2, (8, 28, 28), 16 * O) and geo[3 * 1] == (None, (8, 56, 56), 16 * O)
    assert geo[-1] == (None, (8, 7, 7), 16 * O) and geo[3 * 14 + 1][0] == 8
    # the statistics of a bench step: about 1.1 M LayerNorm rows and 1.0 M lse values
    rows = [8 * (h or 1) * (1 + t * hh * w + n) for h, (t, hh, w), n in geo]
    ln = sum(r for r, g in zip(rows, geo) if g[0] is None)
    lse = sum(r for r, g in zip(rows, geo) if g[0] is not None)
    assert 1.0e6 < ln < 1.25e6 and 0.9e6 < lse < 1.1e6 and max(rows) <= 1 << 24
    image = actmon.slot_geometry(plan, 1, 1, 56, 56)
    assert image[0] == (None, (1, 56, 56), O) and image[-1] == (None, (1, 7, 7), O)


def test_where_unravels_rows_at_16x224_and_at_t1():
    from svit_amd import actmon
    cfg, plan = golden_plan()
    O = plan.objects
    h = header(8, 16, 8, 56, 56)
    N0 = 1 + 8 * 56 * 56 + 16 * O
    assert actmon.where(plan, h, "blocks.0.in", 0) == (0, 0, "cls")
    assert actmon.where(plan, h, 0, 3 * N0 + 1) == (3, 1, ("patch", 0, 0, 0))
    assert actmon.where(plan, h, 0, 3 * N0 + 1 + (2 * 56 + 5) * 56 + 9) == (3, 1 + (2 * 56 + 5) * 56 + 9, ("patch", 2, 5, 9))
    assert actmon.where(plan, h, 0, 8 * N0 - 1) == (7, N0 - 1, ("object", 15, O - 1))
    assert actmon.where(plan, h, "blocks.0.mid", N0 + 1 + 8 * 56 * 56) == (1, 1 + 8 * 56 * 56, ("object", 0, 0))
    assert actmon.where(plan, h, 0, N0 + 1 + 8 * 56 * 56 + O + 2) == (1, 1 + 8 * 56 * 56 + O + 2, ("object", 1, 2))
    # block 1 pools its queries to 28 x 28 and has two heads: its lse is [B, 2, Nq]
    N1 = 1 + 8 * 28 * 28 + 16 * O
    assert actmon.where(plan, h, "blocks.1.in", N0 + 5) == (1, 5, ("patch", 0, 0, 4))
    assert actmon.where(plan, h, "blocks.1.attn_lse", (2 * 2 + 1) * N1 + 1 + 28 * 28 + 3) == (2, 1, 1 + 28 * 28 + 3, ("patch", 1, 0, 3))
    assert actmon.where(plan, h, "blocks.1.mid", N1) == (1, 0, "cls")
    assert actmon.where(plan, h, "norm.in", 1 + 8 * 49 + 16 * O + 1 + 50) == (1, 51, ("patch", 1, 0, 1))
    # an image micro-step in the same ring: T = 1, one frame of objects
    im = header(4, 1, 1, 56, 56)
    M0 = 1 + 56 * 56 + O
    assert actmon.where(plan, im, 0, 2 * M0 + 1 + 57) == (2, 58, ("patch", 0, 1, 1))
    assert actmon.where(plan, im, 0, 4 * M0 - 1) == (3, M0 - 1, ("object", 0, O - 1))
    assert actmon.where(plan, im, "norm.in", 1 + 49) == (0, 50, ("object", 0, 0))
    for slot, r in ((0, 8 * N0), (0, -1), ("blocks.1.attn_lse", 8 * 2 * N1)):
        with pytest.raises(ValueError, match="^where: row "):
            actmon.where(plan, h, slot, r)


def _rows(plan, passes):
    """read()'s dict over hand-made passes: [(pass, step, header, {slot name: (n_bad, first_bad)}, absent names)]"""
    from svit_amd import actmon
    names = actmon.slot_names(len(plan.blocks))
    ring = actmon.empty_ring(len(passes), len(names))
    for k, (p, step, h, bad, absent) in enumerate(passes):
        ring[k]["head"] = h
        ring[k]["head"]["pass"], ring[k]["head"]["step"] = p, step
        ring[k]["entry"]["n_bad"] = 0
        ring[k]["entry"]["rows"] = 100
        ring[k]["entry"]["sum"] = 400.0
        ring[k]["entry"]["ext"] = 0.5
        for n, (nb, fb) in bad.items():
            ring[k]["entry"][names.index(n)]["n_bad"], ring[k]["entry"][names.index(n)]["first_bad"] = nb, fb
        for n in absent:
            ring[k]["entry"][names.index(n)] = actmon.empty_entry()
    lse = np.array([n.endswith("attn_lse") for n in names])
    return ring, actmon.rows_dict(actmon.rows_since(ring, -1), names, lse)


def test_origin_names_the_first_slot_in_network_order():
    from svit_amd import actmon
    cfg, plan = golden_plan()
    O = plan.objects
    h = header(8, 16, 8, 56, 56)
    N0 = 1 + 8 * 56 * 56 + 16 * O
    later = {"blocks.%d.%s" % (i, k): (5, 0) for i in range(4, 16) for k in ("in", "attn_lse", "mid")}
    passes = [
        (0, 0, h, {}, []),
        (1, 1, h, dict(later, **{"blocks.0.in": (3, N0 + 2), "norm.in": (9, 0)}), []),
        (2, 2, h, dict(later, **{"blocks.3.attn_lse": (1, 4)}), []),
        (3, 3, h, dict(later, **{"blocks.3.mid": (2, 1)}), []),
        (4, 3, header(4, 1, 1, 56, 56), {"blocks.4.in": (7, 1 + 14 * 14 + O), "blocks.4.mid": (7, 0)}, []),
        (5, 4, h, {"norm.in": (1, 0)}, ["blocks.0.in", "blocks.0.attn_lse", "blocks.0.mid"]),
    ]
    _, rows = _rows(plan, passes)
    assert rows["passes"].tolist() == [0, 1, 2, 3, 4, 5] and rows["steps"].tolist() == [0, 1, 2, 3, 3, 4]
    assert actmon.origin(plan, rows) == [
        (1, 1, "blocks.0.in", 3, (1, 2, ("patch", 0, 0, 1)), "the stem or the input"),
        (2, 2, "blocks.3.attn_lse", 1, (0, 0, 4, ("patch", 0, 0, 3)), "the q/k of block 3"),
        (3, 3, "blocks.3.mid", 2, (0, 1, ("patch", 0, 0, 0)), "the attention branch of block 3"),
        (4, 3, "blocks.4.in", 7, (1, 0, "cls"), "the MLP of block 3"),
        (5, 4, "norm.in", 1, (0, 0, "cls"), "the MLP of block 15"),
    ]
    assert np.ma.getmaskarray(rows["n_bad"])[5, :3].all() and not np.ma.getmaskarray(rows["n_bad"])[5, 3:].any()
    assert actmon.culprit("blocks.1.in") == "the MLP of block 0" and actmon.culprit("blocks.0.in") == "the stem or the input"


# ---------------------------------------------------------------------------------------------------- read, lost ----
@pytest.fixture(scope="module")
def watched(lib):
    from svit_amd import actmon, optim
    cfg, model = _cpu_model()
    opt = optim.GuardedClipAdamW(model, lr=1e-3, max_consecutive_skips=1)
    return cfg, model, opt, actmon.ActivationMonitor(model, 4, optimizer=opt)


def _fill(mon, passes):
    """a ring of mon.period rows: (pass, step, {slot: (n_bad, first_bad)}) lands in row pass % period"""
    from svit_amd import actmon
    ring = actmon.empty_ring(mon.period, mon.n_slots)
    for p, step, bad in passes:
        r = ring[p % mon.period]
        r["head"] = header(2, 4, 2, 16, 16)
        r["head"]["pass"], r["head"]["step"], r["head"]["n_sites"] = p, step, mon.n_slots
        r["entry"]["n_bad"] = 0
        r["entry"]["rows"] = 50
        r["entry"]["sum"] = 200.0 + p
        r["entry"]["ext"] = 0.5
        r["entry"]["ext2"] = 0.75
        for n, (nb, fb) in bad.items():
            r["entry"][mon.names.index(n)]["n_bad"], r["entry"][mon.names.index(n)]["first_bad"] = nb, fb
    return torch.from_numpy(ring.view(np.uint8).reshape(-1).copy())


def test_read_selects_rows_and_counts_the_lost(watched):
    from svit_amd import actmon
    _, _, _, mon = watched
    assert (mon.n_slots, mon.period, mon.last_read) == (49, 4, -1) and mon.ring.numel() == 4 * (48 + 32 * 49)
    assert mon.names == actmon.slot_names(16) and int(mon.is_lse.sum()) == 16
    rows = mon.read()
    assert rows["passes"].tolist() == [] and rows["lost"] == 0 and mon.log_stats(rows) is None
    mon.ring.copy_(_fill(mon, [(0, 0, {}), (1, 1, {}), (2, 2, {})]))
    rows = mon.read()
    assert rows["passes"].tolist() == [0, 1, 2] and rows["steps"].tolist() == [0, 1, 2] and rows["lost"] == 0
    assert mon.last_read == 2 and rows["header"]["H0"].tolist() == [16, 16, 16]
    ln, lse = ~mon.is_lse, mon.is_lse
    assert np.allclose(rows["mean_sq"].data[1][ln], 201.0 / 50 - 1e-6) and np.ma.getmaskarray(rows["mean_sq"])[1][lse].all()
    assert np.allclose(rows["rms"].data[2][ln], np.sqrt(202.0 / 50 - 1e-6))
    assert np.allclose(rows["widest_std"].data[0][ln], np.sqrt(4.0 - 1e-6)) and (rows["max_abs_mean"].data[0][ln] == 0.75).all()
    assert np.allclose(rows["lse_max"].data[0][lse], 0.5 * np.log(2.0)) and np.ma.getmaskarray(rows["lse_max"])[0][ln].all()
    assert np.allclose(rows["lse_mean"].data[2][lse], 202.0 / 50 * np.log(2.0))
    assert mon.read()["passes"].tolist() == []
    # passes 3 .. 6 arrive: 3 was overwritten by nothing yet -- all four are there
    mon.ring.copy_(_fill(mon, [(3, 3, {}), (4, 3, {}), (5, 4, {}), (6, 4, {})]))
    rows = mon.read()
    assert rows["passes"].tolist() == [3, 4, 5, 6] and rows["steps"].tolist() == [3, 3, 4, 4] and rows["lost"] == 0
    # an overrun by three passes: 7, 8, 9 are gone
    mon.ring.copy_(_fill(mon, [(10, 6, {}), (11, 6, {}), (12, 7, {}), (13, 7, {})]))
    rows = mon.read()
    assert rows["passes"].tolist() == [10, 11, 12, 13] and rows["lost"] == 3 and mon.last_read == 13
    ring = actmon.empty_ring(4, 49)
    assert actmon.read_rows(ring, -1)[1:] == (0, -1)
    mon.reset()
    assert mon.last_read == -1 and int(mon.state[0]) == 0 and mon.read()["passes"].tolist() == []


def test_check_adds_the_origin_only_with_a_monitor(watched):
    """check()'s message: unchanged without an activation monitor, one more line with one bound to the optimizer -- on the
    passes of the step that was dropped last"""
    from svit_amd import actmon, monitor
    _, model, opt, mon = watched
    rec = opt.dev_rec.view(torch.int64)
    rec[0], rec[1] = 2, 1                  # two applied, one dropped: the last step is index 2
    opt.dev_rec[4] = 1                     # consecutive
    with pytest.raises(RuntimeError) as bare:
        opt.check()
    assert "\n" not in str(bare.value) and opt.act_monitor is None
    model.attach_activation_monitor(mon)
    try:
        assert opt.act_monitor is mon and model.engine.act_monitor is mon
        mon.reset()
        N0 = 1 + 2 * 16 * 16 + 4 * model.plan.objects
        mon.ring.copy_(_fill(mon, [(0, 1, {"blocks.5.mid": (9, 0)}), (1, 2, {}), (2, 2, {"blocks.0.in": (12, N0 + 1 + 16 + 3),
                                                                                     "blocks.0.mid": (N0, N0)})]))
        with pytest.raises(RuntimeError) as told:
            opt.check()
        head, line = str(told.value).split("\n")
        assert head == str(bare.value)
        assert line == ("non-finite activations in the forward of step 2 (pass 2): first at blocks.0.in, 12 bad rows, the "
                        "first in sample 1 at token 20 (patch token [0, 1, 3]) -- look at the stem or the input")
        assert mon.last_read == -1
        # the forward of the dropped step was clean (the backward went wrong): no line; with a TensorMonitor: its line alone
        mon.ring.copy_(_fill(mon, [(0, 1, {"blocks.5.mid": (9, 0)}), (1, 2, {})]))
        with pytest.raises(RuntimeError) as clean:
            opt.check()
        assert str(clean.value) == str(bare.value)
        assert mon.origin_line() == ("non-finite activations in the forward of step 1 (pass 0): first at blocks.5.mid, 9 bad "
                                     "rows, the first in sample 0 at token 0 (the cls token) -- look at the attention "
                                     "branch of block 5")
    finally:
        model.attach_activation_monitor(None)
    assert opt.act_monitor is None and model.engine.act_monitor is None


def test_refusals_by_message(lib):
    from svit_amd import actmon, config, optim
    cfg, model = _cpu_model()
    assert "ACT_MONITOR" not in config.get_cfg().SVIT
    classic = optim.FusedClipAdamW(model, lr=1e-3)
    opt = optim.GuardedClipAdamW(model, lr=1e-3)
    with pytest.raises(TypeError, match="GuardedClipAdamW or one of its subclasses, got FusedClipAdamW"):
        actmon.ActivationMonitor(model, 10, optimizer=classic)
    for period in (0, -1, 2.0, True, "4"):
        with pytest.raises(ValueError, match="^ActivationMonitor: period is a positive int, got"):
            actmon.ActivationMonitor(model, period)
    _, other = _cpu_model()
    with pytest.raises(ValueError, match="^ActivationMonitor: the optimizer was built over another model"):
        actmon.ActivationMonitor(other, 4, optimizer=opt)
    from svit_amd.model import MODEL_REGISTRY
    with pytest.raises(ValueError, match="^ActivationMonitor needs a finalized"):
        actmon.ActivationMonitor(MODEL_REGISTRY.get("SViT")(cfg), 4)
    with pytest.raises(ValueError, match="^attach_activation_monitor: the ActivationMonitor was built over another model"):
        model.attach_activation_monitor(actmon.ActivationMonitor(other, 4))
    assert model.engine.act_monitor is None
    # build_actmon: nothing without the key; LOG_PERIOD x virtual ranks rows with it
    assert actmon.build_actmon(cfg, model, opt) is None and model.engine.act_monitor is None and opt.act_monitor is None
    cfg.SVIT.ACT_MONITOR = True
    cfg.LOG_PERIOD = 7
    cfg.NUM_GPUS = 1
    mon = actmon.build_actmon(cfg, model, opt)
    assert type(mon) is actmon.ActivationMonitor and mon.period == 7 and model.engine.act_monitor is mon and opt.act_monitor is mon
    cfg.NUM_GPUS = 8                                                        # the 8-rank recipe on one GPU: k = 8
    assert actmon.build_actmon(cfg, model).period == 56 and opt.act_monitor is None     # (the new one has no optimizer)
    assert actmon.build_actmon(cfg, model, virtual_ranks=2).period == 14
    with pytest.raises(TypeError, match="got FusedClipAdamW"):
        actmon.build_actmon(cfg, model, classic)
    for bad in (0, -3, 2.5, True):
        cfg.LOG_PERIOD = bad
        with pytest.raises(ValueError, match="^SVIT.ACT_MONITOR: cfg.LOG_PERIOD is a positive int, got "):
            actmon.build_actmon(cfg, model, opt)
    cfg.LOG_PERIOD = 7
    for bad in (0, 1.5, True):
        with pytest.raises(ValueError, match="^build_actmon: virtual_ranks is a positive int, got "):
            actmon.build_actmon(cfg, model, opt, virtual_ranks=bad)
    model.attach_activation_monitor(None)


def test_train_epoch_logs_one_line_per_period(watched, caplog):
    """train._log_activation_stats, the call train_epoch makes behind log_iter_stats: nothing without a monitor or between
    periods, else ONE read and one json_stats line"""
    import logging
    from svit_amd import train
    cfg, model, opt, mon = watched
    cfg.LOG_PERIOD = 4
    assert model.engine.act_monitor is None and train._log_activation_stats(model, cfg, 3) is None
    model.attach_activation_monitor(mon)
    try:
        mon.reset()
        N2 = 1 + 2 * 8 * 8 + 4 * model.plan.objects         # block 2: two heads over the 8 x 8 grid block 1 pooled to
        mon.ring.copy_(_fill(mon, [(0, 0, {}), (1, 1, {"blocks.2.attn_lse": (3, 2 * N2 + 5)}), (2, 2, {}), (3, 3, {})]))
        assert train._log_activation_stats(model, cfg, 2) is None and mon.last_read == -1      # not the period's end: no read
        step = types.SimpleNamespace(core=model)                                              # a captured step holds .core
        with caplog.at_level(logging.INFO):
            stats = train._log_activation_stats(step, cfg, 3)
        assert mon.last_read == 3 and stats["_type"] == "train_activation_stats" and (stats["pass"], stats["step"]) == (3, 3)
        assert stats["rows"] == 4 and stats["lost"] == 0 and stats["n_bad"] == 3
        assert len(stats["rms"]) == 17 and len(stats["lse_max"]) == 16 and stats["rms"][0] == float("%.6g" % np.sqrt(203.0 / 50 - 1e-6))
        assert stats["origin"] == [[1, 1, "blocks.2.attn_lse", 3, [1, 0, 5, ["patch", 0, 0, 4]], "the q/k of block 2"]]
        lines = [r.getMessage() for r in caplog.records if "train_activation_stats" in r.getMessage()]
        assert len(lines) == 1 and json.loads(lines[0].split("json_stats: ")[1])["pass"] == 3
        assert train._log_activation_stats(model, cfg, 7) is None                              # nothing new: no line
    finally:
        model.attach_activation_monitor(None)
