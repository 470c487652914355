"""Attention monitor, host side: the site-table validator and every argument refusal of svit_attn_stats by error code, the
workspace query, the probe-row selection, the NumPy yardstick on hand-made rows, three mutants of it against the bar,
read() / `lost` / collapsed() on rings filled by hand, unravel_key on the real plan at 16 x 224^2 and at T = 1, and
build_attnmon's refusals.  No GPU needed."""
import ctypes
import math
import types

import numpy as np
import pytest
import torch

from tests import attnmon_cases as A
from tests.test_actmon_cpu import _cpu_model, golden_plan

P = 4096        # a made-up device address that is never followed
ALL = [0, 1, 2]


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__
    __graft_entry__.build()
    from svit_amd import hip
    return hip.load()


def S(**kw):
    """a site that passes: B 2, 2 heads, a 4 x 4 query grid over a 2 x 2 key grid, 8 objects, slot 0"""
    s = dict(qa=P, ka=P + 16, lse2=P + 4, maps=None, B=2, heads=2, Nq=25, Nk=13, DA=128, bias_cols=5, Lq=16, Lk=4,
             n_obj=8, slot=0, ent_base=0)
    s.update(kw)
    return s


# ------------------------------------------------------------------------------------------------- the validator ----
def _check(lib, sites, n_slots=4, ent_slots=64, groups=ALL, K=32, every=1, maps_samples=0, n_sites=None, null=False,
           null_probe=False):
    from svit_amd import ops
    tab, probe = ops.attn_site_table(sites, groups, K, every, maps_samples)
    w = ctypes.c_int64(-7)
    rc = lib.svit_attn_sites_check(None if null else tab, len(sites) if n_sites is None else n_sites, n_slots, ent_slots,
                                   None if null_probe else ctypes.byref(probe), ctypes.byref(w))
    return rc, w.value


def test_sites_check_by_error_code(lib):
    good = [S(), S(slot=3, ent_base=6, heads=1, DA=160, bias_cols=0, maps=P + 8)]
    assert _check(lib, good) == (0, 2 * 2 * 3 + 2 * 1 * 3)
    assert _check(lib, [S(slot=i, ent_base=6 * i) for i in range(32)], n_slots=32, ent_slots=192)[0] == 0    # the limits
    assert _check(lib, [S(ent_base=1018)], ent_slots=1024)[0] == 0 and _check(lib, [S(slot=1023)], n_slots=1024)[0] == 0
    assert _check(lib, [S(bias_cols=32)])[0] == 0 and _check(lib, [S(DA=160, bias_cols=64)])[0] == 0
    assert _check(lib, [S()], groups=[2], K=256)[0] == 0 and _check(lib, [S()], groups=[0], K=0) == (0, 4)
    bad_arg = {
        "NULL table": dict(sites=good, null=True), "NULL probe": dict(sites=good, null_probe=True),
        "no site": dict(sites=good, n_sites=0), "n_sites < 0": dict(sites=good, n_sites=-1),
        "33 sites": dict(sites=[S(slot=i, ent_base=6 * i) for i in range(33)], n_slots=64, ent_slots=256),
        "n_slots = 0": dict(sites=good, n_slots=0), "n_slots = 1025": dict(sites=good, n_slots=1025),
        "ent_slots = 0": dict(sites=good, ent_slots=0), "ent_slots = 1025": dict(sites=good, ent_slots=1025),
        "no group": dict(sites=good, groups=[]), "an unknown kind": dict(sites=good, groups=[0, 3]),
        "a kind twice": dict(sites=good, groups=[2, 0, 2]), "K = 0": dict(sites=good, K=0), "K = 257": dict(sites=good, K=257),
        "every = 0": dict(sites=good, every=0), "maps_samples < 0": dict(sites=good, maps_samples=-1),
        "NULL qa": dict(sites=[S(qa=None)]), "NULL ka": dict(sites=[S(ka=None)]), "NULL lse2": dict(sites=[S(lse2=None)]),
        "B = 0": dict(sites=[S(B=0)]), "heads = 0": dict(sites=[S(heads=0)]), "Lq = 0": dict(sites=[S(Lq=0, Nq=9)]),
        "Lk = 0": dict(sites=[S(Lk=0, Nk=9)]), "n_obj < 0": dict(sites=[S(n_obj=-1, Nq=16, Nk=4)]),
        "DA = 96": dict(sites=[S(DA=96)]), "DA = 144": dict(sites=[S(DA=144)]),
        "J = 33 at DA 128": dict(sites=[S(bias_cols=33)]), "J = 65 at DA 160": dict(sites=[S(DA=160, bias_cols=65)]),
        "J < 0": dict(sites=[S(bias_cols=-1)]),
        "Nq != 1 + Lq + n_obj": dict(sites=[S(Nq=26)]), "Nk != 1 + Lk + n_obj": dict(sites=[S(Nk=12)]),
        "rows past 2^31": dict(sites=[S(B=1 << 16, heads=1 << 12, Lq=8, Nq=17)]),
        "slot = n_slots": dict(sites=[S(slot=4)]), "slot < 0": dict(sites=[S(slot=-1)]),
        "a slot twice": dict(sites=[S(), S(ent_base=6)]),
        "entries past the row": dict(sites=[S(ent_base=59)]), "ent_base < 0": dict(sites=[S(ent_base=-1)]),
        "entries owned twice": dict(sites=[S(), S(slot=1, ent_base=5)]),
        "NULL qa and a misaligned ka": dict(sites=[S(qa=None, ka=P + 2)]),                # the argument error comes first
    }
    for label, kw in bad_arg.items():
        assert _check(lib, **kw)[0] == -4, label
    for label, kw in {"qa": dict(qa=P + 8), "ka": dict(ka=P + 4), "lse2": dict(lse2=P + 2), "maps": dict(maps=P + 1)}.items():
        assert _check(lib, [S(**kw)])[0] == -3, label
    assert _check(lib, good + [S(slot=1, ent_base=12, ka=P + 2)])[0] == -3                # a later site
    from svit_amd import hip, ops
    assert ops.attn_sites_check(good, 4, 64, ALL) == 18
    with pytest.raises(hip.SvitHipError, match="svit_attn_sites_check .* bad alignment"):
        ops.attn_sites_check([S(qa=P + 2)], 4, 64, ALL)
    with pytest.raises(hip.SvitHipError, match="svit_attn_sites_check .* bad argument"):
        ops.attn_sites_check([S(DA=96)], 4, 64, ALL)


def test_workspace_query(lib):
    from svit_amd import hip, ops
    q = lib.svit_attn_stats_workspace
    assert q(1) == 64 and q(1560) == 1560 * 64 and q(1 << 20) == 64 << 20 and ops.attn_stats_workspace(18) == 1152
    for w in (0, -1, (1 << 20) + 1):
        assert q(w) == -4, w
    with pytest.raises(hip.SvitHipError, match="svit_attn_stats_workspace .* bad argument"):
        ops.attn_stats_workspace(0)


def test_entry_point_checks_its_arguments_without_a_gpu(lib):
    """refused before any HIP call: stream = None and made-up device addresses that are never followed"""
    from svit_amd import ops
    good = [S(), S(slot=2, ent_base=6, heads=1)]
    need = 18 * 64
    geom = np.array([2, 4, 2, 16, 16], dtype=np.int32)

    def stats(sites=good, n_slots=4, ent_slots=16, groups=ALL, K=32, every=1, g=True, rec=P, ring=P, R=4, state=P, ws=P,
              ws_bytes=need, probe=True):
        tab, pr = ops.attn_site_table(sites, groups, K, every, 0)
        return lib.svit_attn_stats(tab, len(sites), n_slots, ent_slots, ctypes.byref(pr) if probe else None,
                                   geom.ctypes.data if g else None, rec, ring, R, state, ws, ws_bytes, None)

    bad_arg = {
        "NULL geom": dict(g=False), "NULL ring": dict(ring=None), "NULL state": dict(state=None), "NULL probe": dict(probe=False),
        "NULL workspace": dict(ws=None), "R = 0": dict(R=0), "R < 0": dict(R=-1),
        "workspace one byte short": dict(ws_bytes=need - 1), "workspace negative": dict(ws_bytes=-1),
        "DA = 96": dict(sites=[S(DA=96)]), "J too large": dict(sites=[S(bias_cols=40)]), "Nq": dict(sites=[S(Nq=24)]),
        "a slot twice": dict(sites=[S(), S(ent_base=6)]), "entries past the row": dict(ent_slots=8),
        "every = 0": dict(every=0), "K = 300": dict(K=300),
    }
    for label, kw in bad_arg.items():
        assert stats(**kw) == -4, label
    bad_align = {"qa": dict(sites=[S(qa=P + 2)]), "lse2": dict(sites=[S(lse2=P + 1)]), "ring": dict(ring=P + 8),
                 "workspace": dict(ws=P + 8), "state": dict(state=P + 4), "dev_rec": dict(rec=P + 4)}
    for label, kw in bad_align.items():
        assert stats(**kw) == -3, label
    # the limits themselves pass the checks: shown through the one check that comes after them (a misaligned ring)
    for kw in (dict(), dict(rec=None), dict(R=1), dict(groups=[0], ws_bytes=6 * 64),
               dict(sites=[S(slot=i, ent_base=6 * i) for i in range(32)], n_slots=32, ent_slots=192, ws_bytes=32 * 12 * 64)):
        assert stats(ring=P + 8, **kw) == -3, kw


# ------------------------------------------------------------------------------------------------- probe rows ----
def test_probe_rows_below_at_and_above_K():
    from svit_amd import attnmon
    g = attnmon.group_rows
    assert g(0, 40, 8, 32).tolist() == [0] and g(1, 40, 8, 32).tolist() == list(range(41, 49)) and g(1, 40, 0, 32).tolist() == []
    assert g(2, 5, 8, 32).tolist() == [1, 2, 3, 4, 5]                       # Lq < K: every patch row
    assert g(2, 32, 8, 32).tolist() == list(range(1, 33))                   # Lq = K
    above = g(2, 33, 0, 32)
    assert len(above) == 32 and above[0] == 1 and above[-1] == 1 + (63 * 33) // 64 == 33 and (np.diff(above) >= 1).all()
    big = g(2, 8 * 56 * 56, 64, 256)                                        # block 0 of the recipe, the largest K
    assert len(big) == 256 and big[0] == 1 + 25088 // 512 and big[-1] <= 25088 and (np.diff(big) == 98).all()
    assert g(2, 1568, 64, 32).tolist() == [1 + ((2 * i + 1) * 1568) // 64 for i in range(32)]
    names, kinds, K = attnmon.parse_rows(("patch:7", "cls"))
    assert (names, kinds, K) == (["patch:7", "cls"], [2, 0], 7) and attnmon.parse_rows("cls, obj")[1] == [0, 1]
    for bad in (("cls", "cls"), ("patch",), ("patch:0",), ("patch:257",), ("cls:3",), ("rows",), (), ("patch:x",), (3,)):
        with pytest.raises(ValueError, match="attention monitor rows"):
            attnmon.parse_rows(bad)


# ------------------------------------------------------------------------------------------------- the yardstick ----
def _hand(P_rows, Lk, n_obj, lse=None):
    """operands whose probe rows have exactly the given probabilities: one head, one sample, no patch queries but one;
    qa row q is e_q (a unit vector) scaled by 1 and ka[k, q] = log2 P[q][k] rounded to bf16 -- P is then recomputed
    from the rounded operands, and lse2 is their exact log-sum"""
    P_rows = np.asarray(P_rows, dtype=np.float64)
    Nq, Nk = P_rows.shape
    qa = np.zeros((1, 1, Nq, 128), dtype=np.float32)
    ka = np.zeros((1, 1, Nk, 128), dtype=np.float32)
    for q in range(Nq):
        qa[0, 0, q, q] = 1.0
        ka[0, 0, :, q] = np.log2(P_rows[q])
    ka = A.bf16(ka).float().numpy()
    s = ka[0, 0, :, :Nq].T.astype(np.float64)
    lse2 = np.log2(np.exp2(s).sum(-1)).astype(np.float32)[None, None] if lse is None else lse
    return qa, ka, lse2


def test_attn_host_on_hand_made_rows():
    """uniform, one-hot and two equal peaks, as the cls row and the two object rows of a site with 5 keys"""
    from svit_amd import attnmon
    tiny = 2.0 ** -40
    rows = [[0.125] * 8,                                                     # cls: uniform over 1 + 5 + 2 keys
            [1.0, tiny, tiny, tiny, tiny, tiny, tiny, tiny],                 # patch row 1: one-hot on cls
            [0.25] * 4 + [tiny] * 4, [0.125] * 8, [0.125] * 8, [0.125] * 8,  # patch rows 2 .. 5
            [tiny, tiny, 0.5, tiny, tiny, tiny, 0.5, tiny],                  # object row 0: two equal peaks, one an object key
            [tiny] * 7 + [1.0]]                                              # object row 1: one-hot on the last object key
    qa, ka, lse2 = _hand(rows, 5, 2)
    h = attnmon.attn_host(qa, ka, lse2, 5, 5, 2, 8, [0, 1, 2], 32)
    e, per = h["entries"], h["per_row"]
    assert h["rows"].tolist() == [0, 6, 7, 1, 2, 3, 4, 5] and h["group"].tolist() == [0, 1, 1, 2, 2, 2, 2, 2]
    assert e["rows"].tolist() == [1, 2, 5] and (e["n_bad"] == 0).all() and (e["first_bad"] == -1).all()
    near = dict(rel=0, abs=1e-9)
    assert e["sum_H"][0] == pytest.approx(3.0, **near) and e["sum_cls"][0] == pytest.approx(0.125, **near)
    assert e["sum_obj"][0] == pytest.approx(0.25, **near) and e["sum_pmax"][0] == pytest.approx(0.125, **near)
    # two equal peaks: 1 bit; one-hot: 0 bits; the object mass of the two rows: 0.5 + 1
    assert e["sum_H"][1] == pytest.approx(1.0, **near) and e["sum_obj"][1] == pytest.approx(1.5, **near)
    assert e["sum_pmax"][1] == pytest.approx(1.5, **near) and e["min_row"][1] == 7 and e["min_H"][1] == pytest.approx(0.0, abs=1e-9)
    assert per["argmax"][0, 0].tolist()[:3] == [0, 2, 7]                     # (the first among equal peaks)
    # patch rows: one-hot on cls (0 bits), four keys (2 bits), three uniform (3 bits)
    assert e["sum_H"][2] == pytest.approx(0 + 2 + 9, **near) and e["sum_cls"][2] == pytest.approx(1 + 0.25 + 0.375, **near)
    assert e["min_row"][2] == 1 and e["sum_p"][2] == pytest.approx(5.0, **near) and e["sum_dev"].max() < 1e-6
    assert (h["bars"]["sum_H"] > 0).all() and (h["bars"]["sum_H"] < 1e-3).all()
    # bad rows: a NaN lse2 on the cls row, an inf score on an object row
    lse_bad = lse2.copy()
    lse_bad[0, 0, 0] = np.nan
    qb = qa.copy()
    qb[0, 0, 7, 7] = np.inf
    hb = attnmon.attn_host(qb, ka, lse_bad, 5, 5, 2, 8, [0, 1, 2], 32)
    eb = hb["entries"]
    assert eb["n_bad"].tolist() == [1, 1, 0] and eb["first_bad"].tolist() == [0, 7, -1]
    assert eb["min_row"].tolist() == [-1, 6, 1] and eb["sum_H"][0] == 0.0 and eb["sum_H"][1] == pytest.approx(1.0, **near)
    assert eb[2].tobytes() == e[2].tobytes() and np.isnan(hb["P"][0, 0, 0]).all()
    # columns past 96 + J are never read
    qn, kn = qa.copy(), ka.copy()
    qn[..., 104:] = np.nan
    kn[..., 104:] = np.inf
    assert attnmon.attn_host(qn, kn, lse2, 5, 5, 2, 8, [0, 1, 2], 32)["entries"].tobytes() == e.tobytes()


def test_three_mutants_lie_ten_bars_out():
    for seed, (DA, J) in enumerate([(128, 20), (160, 41)]):
        s = A.site(2, 2, 40, 12, 8, DA, J, seed=40 + seed)
        h = A.host(s, ALL, 32)
        e, bars = h["entries"], h["bars"]
        for which, key in (("column", "sum_p"), ("obj", "sum_obj"), ("ln", "sum_H")):
            m = A.mutant(s, ALL, 32, which)
            ratio = np.abs(m[key] - e[key]) / bars[key]
            assert ratio.min() >= 10.0, (DA, which, float(ratio.min()))
        # and the yardstick itself, recomputed, sits at zero
        assert A.host(s, ALL, 32)["entries"].tobytes() == e.tobytes()


# ------------------------------------------------------------------------------------------------- reading ----
def _plan4():
    from svit_amd import arch, config
    return arch.build_plan(config.ssv2_cfg(num_frames=4, crop=64))


def _filled(plan, names, written):
    """a ring of 4 rows for `plan`: written = [(ring row, pass, step, row counter)], entropy of entry e = (e % 5) bits"""
    from svit_amd import attnmon
    index, _ = attnmon.entry_index(plan, names)
    ring = attnmon.empty_ring(4, len(index))
    for at, p, step, row in written:
        h = ring[at]["head"]
        h["pass"], h["step"], h["row"] = p, step, row
        h["B"], h["Tx"], h["T0"], h["H0"], h["W0"], h["n_sites"] = 2, 4, 2, 16, 16, len(plan.blocks)
        e = ring[at]["entry"]
        e["rows"], e["n_bad"], e["first_bad"], e["min_row"] = 4, 0, -1, 3
        e["sum_H"] = 4.0 * (np.arange(len(index)) % 5)
        e["sum_p"], e["sum_cls"], e["sum_obj"], e["sum_pmax"] = 4.0, 1.0, 2.0, 3.0
    return ring, index


def test_read_lost_and_collapsed_on_rings_filled_by_hand():
    from svit_amd import attnmon
    plan = _plan4()
    names = ["cls", "obj", "patch:32"]
    ring, index = _filled(plan, names, [(0, 8, 4, 4), (1, 10, 5, 5), (2, 4, 2, 2), (3, 6, 3, 3)])      # every = 2, wrapped once
    rows, lost, last = attnmon.read_rows(ring, -1)
    assert rows["head"]["pass"].tolist() == [4, 6, 8, 10] and lost == 2 and last == 5
    assert attnmon.read_rows(ring, 5) [1:] == (0, 5) and attnmon.read_rows(ring, 3)[0]["head"]["row"].tolist() == [4, 5]
    assert attnmon.read_rows(attnmon.empty_ring(4, len(index)), -1)[1:] == (0, -1)
    # an absent block and a group without a good row
    base = index.index((2, 0, "cls"))
    ring[1]["entry"][base:base + 3] = attnmon.empty_entry()
    e = ring[1]["entry"][0]
    e["n_bad"], e["first_bad"], e["min_row"] = 4, 0, -1
    d = attnmon.rows_dict(plan, rows[:0], names)
    assert len(d["passes"]) == 0 and d["entropy"].shape == (0, len(index))
    rows, lost, _ = attnmon.read_rows(ring, -1)
    d = attnmon.rows_dict(plan, rows, names, lost)
    assert d["lost"] == 2 and d["steps"].tolist() == [2, 3, 4, 5] and d["index"] == index
    assert d["entropy"][0].tolist() == [float(i % 5) for i in range(len(index))]
    mask = np.ma.getmaskarray(d["entropy"])
    assert mask[3][0] and mask[3][base:base + 3].all() and mask.sum() == 4
    assert np.ma.getmaskarray(d["n_bad"])[3][base] and not np.ma.getmaskarray(d["n_bad"])[3][0] and d["n_bad"][3][0] == 4
    assert d["mass_cls"][0][1] == 0.25 and d["mass_obj"][0][1] == 0.5 and d["mass_patch"][0][1] == 0.25 and d["pmax"][0][1] == 0.75
    # block 0 of the tiny plan: keys 1 + 2 * 4 * 4 + 4 * O
    geo = attnmon.block_geometry(plan, 4, 2, 16, 16)
    Nk0 = 1 + int(np.prod(geo[0][2])) + geo[0][3]
    assert d["entropy_norm"][0][1] == pytest.approx(1.0 / math.log2(Nk0))
    hit = attnmon.collapsed(d, 0.05)
    zeros = [i for i in range(len(index)) if i % 5 == 0]
    gone = len({0, base, base + 1, base + 2} & set(zeros))                        # (masked in the last row: not collapsed)
    assert len(hit) == 4 * len(zeros) - gone and hit[0] == (2, 0, 0, "cls", 0.0)
    assert {(b, hd, g) for _, b, hd, g, _ in hit} == {index[i] for i in zeros}
    assert attnmon.collapsed(d, 0.0) == []
    at = attnmon.where(plan, d["header"][0], 0, 0, 3)
    assert at == (0, 0, 3, ("patch", 0, 0, 2))


def test_unravel_key_on_the_real_plan():
    from svit_amd import attnmon
    cfg, plan = golden_plan()
    O = plan.objects
    video = attnmon.train_geometry(plan)
    assert video == (16, 8, 56, 56)
    geo = attnmon.block_geometry(plan, *video)
    heads, q0, k0, n_obj = geo[0]
    assert (heads, q0, k0, n_obj) == (1, (8, 56, 56), (8, 7, 7), 16 * O) and 1 + 392 + n_obj == 457
    u = lambda b, k, g=video: attnmon.unravel_key(plan, g, b, k)
    assert u(0, 0) == "cls" and u(0, 1) == ("patch", 0, 0, 0) and u(0, 392) == ("patch", 7, 6, 6)
    assert u(0, 1 + 7 * 7 + 8) == ("patch", 1, 1, 1) and u(0, 393) == ("object", 0, 0)
    assert u(0, 393 + O) == ("object", 1, 0) and u(0, 392 + 16 * O) == ("object", 15, O - 1)
    # the largest key count of the recipe: 1 + 8 * 14 * 14 + 64 = 1633
    assert max(1 + int(np.prod(g[2])) + g[3] for g in geo) == 1633
    last = len(plan.blocks) - 1
    kl = geo[last][2]
    assert u(last, int(np.prod(kl))) == ("patch", kl[0] - 1, kl[1] - 1, kl[2] - 1)
    with pytest.raises(ValueError, match="unravel_key: key"):
        u(0, 393 + 16 * O)
    # the frames pass / an image: T = 1, one frame's objects
    image = (1, 1, 56, 56)
    assert attnmon.block_geometry(plan, *image)[0][2:] == ((1, 7, 7), O)
    assert u(0, 49, image) == ("patch", 0, 6, 6) and u(0, 50, image) == ("object", 0, 0) and u(0, 49 + O, image) == ("object", 0, O - 1)
    with pytest.raises(ValueError, match="unravel_key: key"):
        u(0, 50 + O, image)
    # the header of a ring row works as well as the tuple
    head = np.zeros((), dtype=attnmon.HEADER)
    head["Tx"], head["T0"], head["H0"], head["W0"] = video
    assert attnmon.unravel_key(plan, head, 0, 392) == ("patch", 7, 6, 6)
    # 65 (block, head) pairs, 195 entries with the default groups: inside a ring row's 1024
    index, base = attnmon.entry_index(plan, ["cls", "obj", "patch:32"])
    assert len(index) == 3 * sum(b.heads for b in plan.blocks) <= attnmon.MAX_ENTRIES and base[1] == 3 * plan.blocks[0].heads


# ------------------------------------------------------------------------------------------------- building ----
def test_build_attnmon_refusals():
    from svit_amd import attnmon
    cfg, model = _cpu_model()
    model.engine.attn_monitor = None
    assert attnmon.build_attnmon(cfg, model) is None and "ATTN_MONITOR" not in cfg.SVIT
    cfg.SVIT.ATTN_MONITOR = True
    cfg.LOG_PERIOD = 0
    with pytest.raises(ValueError, match="SVIT.ATTN_MONITOR: cfg.LOG_PERIOD is a positive int"):
        attnmon.build_attnmon(cfg, model)
    cfg.LOG_PERIOD = 10
    for key, value, msg in (("ATTN_MONITOR_EVERY", 0, "SVIT.ATTN_MONITOR_EVERY is a positive int"),
                            ("ATTN_MONITOR_EVERY", True, "SVIT.ATTN_MONITOR_EVERY is a positive int"),
                            ("ATTN_MONITOR_MAPS", -1, "SVIT.ATTN_MONITOR_MAPS is a non-negative int"),
                            ("ATTN_MONITOR_ROWS", ("cls", "rows"), "attention monitor rows"),
                            ("ATTN_MONITOR_ROWS", ("patch:999",), "K is an int in 1 .. 256")):
        old = getattr(cfg.SVIT, key, None)
        setattr(cfg.SVIT, key, value)
        with pytest.raises(ValueError, match=msg):
            attnmon.build_attnmon(cfg, model)
        if old is None:
            del cfg.SVIT[key]
        else:
            setattr(cfg.SVIT, key, old)
    with pytest.raises(ValueError, match="build_attnmon: virtual_ranks is a positive int"):
        attnmon.build_attnmon(cfg, model, virtual_ranks=0)
    with pytest.raises(TypeError, match="takes an optim.GuardedClipAdamW"):
        attnmon.build_attnmon(cfg, model, optimizer=torch.optim.SGD(model.parameters(), lr=0.1), virtual_ranks=1)
    bare = types.SimpleNamespace(flat=None)
    with pytest.raises(ValueError, match="needs a finalized"):
        attnmon.AttentionMonitor(bare, 4)
    for kw, msg in ((dict(period=0), "period is an int >= 1"), (dict(period=4, every=0), "every is an int >= 1"),
                    (dict(period=4, maps_samples=-2), "maps_samples is an int >= 0")):
        with pytest.raises(ValueError, match=msg):
            attnmon.AttentionMonitor(model, **kw)
    # a monitor over the CPU stand-in: the ring as the host writes it, entries in plan order
    mon = attnmon.build_attnmon(cfg, model, virtual_ranks=2)
    assert model.engine.attn_monitor is mon and mon.period == 20 and mon.every == 1 and mon.maps_samples == 0
    assert mon.ent_slots == 3 * sum(b.heads for b in model.plan.blocks) and mon.state.tolist() == [0, 0, -1, 0]
    assert mon.read()["passes"].tolist() == [] and mon.log_stats(mon.read()) is None
    rows, group = mon.probe_rows(0)                                       # (the training clip's geometry by default)
    assert rows[0] == 0 and group.tolist()[:2] == [0, 1] and len(rows) == mon.n_probe(2 * 16 * 16, 4 * model.plan.objects)
    assert mon.unravel_key(0, 0) == "cls" and mon.unravel_key(0, 1) == ("patch", 0, 0, 0)
    other = _cpu_model()[1]
    with pytest.raises(ValueError, match="built over another model"):
        other.attach_attention_monitor(mon)
    model.attach_attention_monitor(None)
    assert model.engine.attn_monitor is None
