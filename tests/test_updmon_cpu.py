"""The update monitor, host side: every argument refusal of the three entry points and the workspace query by error code,
the NumPy yardstick on hand-made cases (the four weights of the stall among them) and three mutants of it that land far
above the bar, the key function, by_layer on the real 405-tensor layout, stalled(), read() and `lost` on rings filled by
hand, build_update_monitor's refusals and construct_optimizer's dispatch.  No GPU needed."""
import numpy as np
import pytest
import torch

from tests import monitor_cases as M
from tests import update_cases as U


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__
    __graft_entry__.build()
    from svit_amd import hip
    return hip.load()


def _cpu_model():
    """an SViT that has not left the CPU, with the real FlatParams placement over untouched CPU memory"""
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
    return cfg, model


def _tab(rows):
    return np.ascontiguousarray(np.array(rows, dtype=np.int64).reshape(-1, 2))


GOOD = [[0, 5], [8, 9], [12, 108], [108, 4000], [4096, 20000]]
N = 20000
SEG_ARG = {
    "S = 65": dict(segs=[[8 * i, 8 * i + 4] for i in range(65)]), "S < 0": dict(S=-1),
    "S > 0 without a table": dict(segs=[[0, 8]], seg_ptr=False),
    "segments unsorted": dict(segs=[[4104, 4120], [0, 8]]), "segments overlapping": dict(segs=[[0, 16], [8, 24]]),
    "segment empty": dict(segs=[[0, 8], [16, 16]]), "segment end > n": dict(segs=[[0, 8], [N - 8, N + 4]]),
}


# ----------------------------------------------------------------------------------------------- the entry points ----
def test_header_names_the_entry_points(lib):
    from svit_amd import build, hip
    for name in ("svit_update_snapshot", "svit_update_stats", "svit_update_stats_workspace"):
        assert name in hip.EXPORTS and hasattr(lib, name)
    assert "update.hip" in build.SOURCES and "update.hip" not in build.SOURCE_FLAGS and "-ffast-math" in build.flags_for("update.hip")


def test_workspace_query(lib):
    from svit_amd import hip, ops
    q = lib.svit_update_stats_workspace
    assert q(1, 1) == 2 * 64 and q(4096, 1) == 2 * 64 and q(4097, 1) == 3 * 64
    assert q(34_400_000, 405) == (8399 + 405) * 64 and ops.update_stats_workspace(5 * 4096, 80) == 85 * 64
    assert q(8, 4096) == 4097 * 64
    for n, Tn in ((0, 1), (-1, 1), (8, 0), (8, -1), (8, 4097)):
        assert q(n, Tn) == -4, (n, Tn)
    with pytest.raises(hip.SvitHipError, match="svit_update_stats_workspace .* bad argument"):
        ops.update_stats_workspace(0, 1)


def test_snapshot_checks_its_arguments_without_a_gpu(lib):
    """refused before any HIP call: stream = None and made-up device addresses that are never followed"""
    P = 4096

    def snap(p=P, shadow=2 * P, n=N, segs=None, S=None, rec=P, every=1, seg_ptr=True):
        keep = _tab(segs) if segs is not None else None
        sp = keep.ctypes.data if keep is not None and seg_ptr else None
        return lib.svit_update_snapshot(p, shadow, n, sp, (0 if keep is None else len(keep)) if S is None else S, rec,
                                        every, None)

    bad_arg = dict(SEG_ARG, **{"NULL p": dict(p=None), "NULL shadow": dict(shadow=None), "NULL dev_rec": dict(rec=None),
                               "n = 0": dict(n=0), "n < 0": dict(n=-4), "every = 0": dict(every=0), "every < 0": dict(every=-3)})
    for label, kw in bad_arg.items():
        assert snap(**kw) == -4, label
    for label, kw in {"a segment bound": dict(segs=[[0, 6]]), "a segment begin": dict(segs=[[2, 8]]), "p": dict(p=P + 4),
                      "shadow": dict(shadow=P + 8), "dev_rec": dict(rec=P + 4)}.items():
        assert snap(**kw) == -3, label
    # the limits themselves pass the checks: shown through the one check that comes after them (a misaligned p)
    for kw in (dict(), dict(segs=[[0, N]]), dict(segs=[[8 * i, 8 * i + 4] for i in range(64)]), dict(every=10 ** 9),
               dict(S=0, seg_ptr=False), dict(n=1)):
        assert snap(p=P + 4, **kw) == -3, kw


def test_stats_checks_its_arguments_without_a_gpu(lib):
    P = 4096
    need = lib.svit_update_stats_workspace(N, len(GOOD))

    def stats(rows=GOOD, n=N, Tn=None, host=True, segs=None, S=None, p=P, shadow=P, g=P, m=P, v=P, tdev=P, rec=P, ring=P,
              R=4, every=1, ws=P, ws_bytes=need, seg_ptr=True):
        t = _tab(rows)
        keep = _tab(segs) if segs is not None else None
        sp = keep.ctypes.data if keep is not None and seg_ptr else None
        return lib.svit_update_stats(p, shadow, g, m, v, n, tdev, t.ctypes.data if host else None,
                                     len(t) if Tn is None else Tn, sp, (0 if keep is None else len(keep)) if S is None else S,
                                     rec, ring, R, every, ws, ws_bytes, None)

    bad_arg = dict(SEG_ARG, **{
        "NULL p": dict(p=None), "NULL shadow": dict(shadow=None), "NULL g": dict(g=None), "NULL device table": dict(tdev=None),
        "NULL host table": dict(host=False), "NULL dev_rec": dict(rec=None), "NULL ring": dict(ring=None),
        "NULL workspace": dict(ws=None), "R = 0": dict(R=0), "R < 0": dict(R=-2), "every = 0": dict(every=0),
        "every < 0": dict(every=-1), "n = 0": dict(n=0), "Tn = 0": dict(Tn=0),
        "Tn = 4097": dict(rows=[[4 * i, 4 * i + 3] for i in range(4097)], n=4 * 4097, ws_bytes=1 << 30),
        "table unsorted": dict(rows=[[8, 12], [0, 4]]), "table overlapping": dict(rows=[[0, 9], [8, 12]]),
        "table empty tensor": dict(rows=[[0, 4], [8, 8]]), "table end > n": dict(rows=[[0, 4], [N - 4, N + 1]]),
        "workspace one byte short": dict(ws_bytes=need - 1), "workspace negative": dict(ws_bytes=-1),
        "the TensorMonitor's workspace": dict(ws_bytes=lib.svit_tensor_stats_workspace(N, len(GOOD)))})
    for label, kw in bad_arg.items():
        assert stats(**kw) == -4, label
    bad_align = {"a begin not a multiple of 4": dict(rows=[[0, 4], [9, 12]]), "a segment bound": dict(segs=[[0, 6]]),
                 "p": dict(p=P + 4), "shadow": dict(shadow=P + 8), "g": dict(g=P + 4), "m": dict(m=P + 8), "v": dict(v=P + 4),
                 "ring": dict(ring=P + 8), "workspace": dict(ws=P + 8), "device table": dict(tdev=P + 4),
                 "dev_rec": dict(rec=P + 4)}
    for label, kw in bad_align.items():
        assert stats(**kw) == -3, label
    # the limits themselves, and m / v left out, pass the checks: shown through the one that comes after them
    for kw in (dict(), dict(segs=[[0, N]]), dict(segs=[[8 * i, 8 * i + 4] for i in range(64)]), dict(R=1, every=10 ** 9),
               dict(rows=[[4 * i, 4 * i + 3] for i in range(4096)], n=4 * 4096, ws_bytes=(4 + 4096) * 64),
               dict(S=0, seg_ptr=False), dict(m=None), dict(v=None), dict(m=None, v=None)):
        assert stats(g=P + 4, **kw) == -3, kw


# ------------------------------------------------------------------------------------------------- the yardstick ----
def test_key_function():
    from svit_amd import updmon
    f = np.float32
    tiny = np.frombuffer(np.array([1, 2, 0x007fffff, 0x00800000], dtype=np.uint32).tobytes(), dtype=np.float32)
    x = np.array([0.0, -0.0, 1.0, U.neighbour1(1.0, up=False), U.neighbour1(1.0), -1.0, U.neighbour1(-1.0, up=False)], dtype=f)
    k = updmon.ulp_key(x)
    assert k.dtype == np.int64 and k[0] == 0 and k[1] == -1                         # +0.0 -> -0.0 is one step
    assert k[2] - k[3] == 1 and k[4] - k[2] == 1                                    # across the binade edge at 1.0
    assert x[3] == f(1.0) - f(2.0 ** -24) and x[4] == f(1.0) + f(2.0 ** -23)
    assert k[5] == -k[2] - 1 and k[5] - k[6] == 1 and x[6] == f(-1.0) - f(2.0 ** -23)
    kt = updmon.ulp_key(tiny)
    assert kt.tolist() == [1, 2, 0x007fffff, 0x00800000]                            # denormals, up to the first normal
    assert updmon.ulp_key(-tiny).tolist() == [-2, -3, -0x00800000, -0x00800001]
    # monotone, adjacent floats one apart, over a sweep through zero; from_key is the inverse
    keys = np.arange(-5000, 5000, dtype=np.int64)
    vals = U.from_key(keys)
    assert (np.diff(vals.astype(np.float64)) >= 0).all() and np.array_equal(updmon.ulp_key(vals), keys)
    big = np.array([np.finfo(f).max, -np.finfo(f).max], dtype=f)
    kb = updmon.ulp_key(big)
    assert kb[0] - kb[1] == 2 * 0x7f7fffff + 1                                      # the difference needs int64


def test_update_host_on_hand_made_cases():
    from svit_amd import updmon
    f = np.float32
    table = _tab([[0, 3], [4, 8], [8, 16], [20, 21], [24, 28]])
    po, pn, g = np.zeros(32, dtype=f), np.zeros(32, dtype=f), np.zeros(32, dtype=f)
    m, v = np.full(32, 0.5, dtype=f), np.full(32, 0.25, dtype=f)
    po[0:3], pn[0:3], g[0:3] = [1.0, 2.0, 2.0], [1.0, 1.5, 4.0], [3.0, -4.0, 12.0]
    po[3] = pn[3] = g[3] = np.nan                       # padding: never counted
    po[4:8], pn[4:8] = [0.0, -0.0, 0.0, 1.0], [-0.0, 0.0, 0.0, U.neighbour1(1.0, up=False)]
    po[8:16] = 0.25
    pn[8:16] = 0.25
    g[8:16] = -0.25
    po[20], pn[20], g[20] = 3.0, -1.0, 2.0
    po[24:28] = pn[24:28] = [1e-41, 1.0, -2.0, 0.0]
    pn[24] = U.neighbour1(1e-41)
    row = updmon.update_host(po, pn, g, m, v, table, step=7)
    e = row["entry"]
    assert row.dtype == updmon.row_dtype(5) and updmon.ENTRY.itemsize == 64 and updmon.HEADER.itemsize == 16
    assert row["head"].tolist() == (7, 3, 0) and updmon.row_dtype(5).itemsize == 16 + 64 * 5
    assert e["sumsq_d"][:4].tolist() == [4.25, 2.0 ** -48, 0.0, 16.0] and e["sumsq_d"][4] == float(f(1e-45)) ** 2
    assert e["sumsq_p"][:4].tolist() == [1.0 + 2.25 + 16.0, float(pn[7]) ** 2, 0.5, 1.0]
    assert e["dot_dg"].tolist() == [2.0 + 24.0, 0.0, 0.0, -8.0, 0.0] and e["sumsq_g"].tolist() == [169.0, 0.0, 0.5, 4.0, 0.0]
    assert e["sumsq_m"].tolist() == [0.75, 1.0, 2.0, 0.25, 1.0] and e["sum_v"].tolist() == [0.75, 1.0, 2.0, 0.25, 1.0]
    assert e["absmax_d"].tolist() == [2.0, 2.0 ** -24, 0.0, 4.0, float(f(1e-45))]
    assert e["n_still"].tolist() == [1, 1, 8, 0, 3] and e["n_one_ulp"].tolist() == [0, 3, 0, 0, 1]
    # without the moments: zeros and the flags say so
    for mm, vv, flags in ((m, None, 1), (None, None, 0), (None, v, 2)):
        r = updmon.update_host(po, pn, g, mm, vv, table)
        assert r["head"].tolist() == (-1, flags, 0)
        assert (r["entry"]["sumsq_m"] > 0).all() == (mm is not None) and (r["entry"]["sum_v"] > 0).all() == (vv is not None)
        assert not r["entry"]["sumsq_m"].any() or mm is not None
    # frozen tensors keep the empty ring's entry
    r = updmon.update_host(po, pn, g, m, v, table, segs=_tab([[0, 4], [8, 16]]))
    assert r["entry"]["n_still"].tolist() == [1, -1, 8, -1, -1] and r["entry"]["sumsq_d"].tolist() == [4.25, 0.0, 0.0, 0.0, 0.0]
    terms = updmon.abs_terms_host(po, pn, g, m, v, table)
    assert terms["dot_dg"].tolist() == [2.0 + 24.0, 0.0, 0.0, 8.0, 0.0] and terms["sumsq_d"].tolist() == e["sumsq_d"].tolist()
    assert updmon.UpdateMonitor.update_host is updmon.update_host
    ring = updmon.empty_ring(3, 5)
    assert ring.itemsize == 16 + 64 * 5 and (ring["head"]["step"] == -1).all() and (ring["entry"]["n_still"] == -1).all()
    assert not ring["entry"]["sumsq_d"].any() and not ring["entry"]["n_one_ulp"].any() and not ring["head"]["flags"].any()


def test_the_four_weights_of_the_stall():
    """one AdamW step at lr = 1e-9, wd = 0, g = +-1 in NumPy float32: weights of 1.0 and 0.5 do not change a bit, weights
    of +-0.01 move by exactly one ulp -- as update_host counts them"""
    from svit_amd import updmon
    p = np.array([1.0, 0.5, 0.01, -0.01] * 2, dtype=np.float32)
    g = np.array([1.0] * 4 + [-1.0] * 4, dtype=np.float32)
    p_new, m, v = U.adamw_first_step(p, g, lr=1e-9)
    table = _tab([[0, 1], [1, 2], [2, 3], [3, 4]])
    for half in (slice(0, 4), slice(4, 8)):
        e = updmon.update_host(p[half], p_new[half], g[half], m[half], v[half], _tab([[0, 2], [2, 4]]))["entry"]
        assert e["n_still"].tolist() == [2, 0] and e["n_one_ulp"].tolist() == [0, 2]
        assert e["sumsq_d"][0] == 0 and e["absmax_d"][1] == np.float32(2.0 ** -30)              # one ulp of 0.01
        assert abs(e["absmax_d"][1] - 1e-9) < 1e-10
    assert np.array_equal(p_new[[0, 1, 4, 5]], p[[0, 1, 4, 5]])
    assert (np.sign(p_new[2:4] - p[2:4]) == -1).all() and (np.sign(p_new[6:8] - p[6:8]) == 1).all()
    assert table.shape == (4, 2)


def _synthetic():
    table, n, where = M.layout(4096)
    po, g, m, v = U.buffers(n)
    pn, expect = U.perturb(po, table, where, 4096)
    return table, n, where, po, pn, g, m, v, expect


def test_perturbation_is_what_the_gpu_tests_say():
    from svit_amd import updmon
    table, n, where, po, pn, g, m, v, expect = _synthetic()
    e = updmon.update_host(po, pn, g, m, v, table)["entry"]
    for t, (still, one) in expect.items():
        assert (int(e["n_still"][t]), int(e["n_one_ulp"][t])) == (still, one), t
    W = 4096
    for i in (W - 1, W, 2 * W - 1, 2 * W, int(table[where["W + 1"]][0]), 4 * W, n - 1):
        assert pn[i] == po[i] and (pn[i - 1] != po[i - 1] or pn[i + 1 if i + 1 < n else i - 1] != po[i + 1 if i + 1 < n else i - 1])
    assert pn[W - 2] != po[W - 2] and pn[W + 1] != po[W + 1] and pn[2 * W - 2] != po[2 * W - 2] and pn[2 * W + 1] != po[2 * W + 1]
    a4 = int(table[where["size 4"]][0])
    assert np.signbit(pn[a4 + 2]) and not np.signbit(po[a4 + 2]) and pn[a4 + 2] == 0 == po[a4 + 2]
    a96 = int(table[where["size 96"]][0])
    assert po[a96 + 3] < 1.0 == pn[a96 + 3] and po[a96 + 4] < 1.0 < pn[a96 + 4]


def test_mutants_of_the_yardstick_miss_the_bar_tenfold():
    """fp32 accumulation, p_old in place of p_new in sumsq_p, a dropped last element per tensor: each lands at least ten
    times above the bar the kernels are held to; the yardstick against itself lands at zero"""
    from svit_amd import updmon
    table, n, where, po, pn, g, m, v, _ = _synthetic()
    want = updmon.update_host(po, pn, g, m, v, table)
    terms = updmon.abs_terms_host(po, pn, g, m, v, table)
    assert U.worst_excess(want, want, terms) == 0.0
    U.assert_row(want, want, terms, "itself")

    def seq32(x):                                   # a running fp32 sum, element after element
        return float(np.cumsum(x.astype(np.float32), dtype=np.float32)[-1])

    fp32 = want.copy()
    for t, (a, b) in enumerate(table):
        d = (pn[a:b].astype(np.float64) - po[a:b].astype(np.float64))
        fp32["entry"]["sumsq_d"][t] = seq32(d * d)
        fp32["entry"]["sumsq_p"][t] = seq32(pn[a:b].astype(np.float64) ** 2)
        fp32["entry"]["sumsq_g"][t] = seq32(g[a:b].astype(np.float64) ** 2)
    swapped = updmon.update_host(po, pn, g, m, v, table)
    swapped["entry"]["sumsq_p"] = updmon.update_host(pn, po, g, m, v, table)["entry"]["sumsq_p"]
    short = table.copy()
    short[:, 1] -= (short[:, 1] - short[:, 0]) > 1
    dropped = updmon.update_host(po, pn, g, m, v, short)
    for label, mutant in (("fp32 accumulation", fp32), ("p_old for p_new", swapped), ("a dropped last element", dropped)):
        assert U.worst_excess(mutant, want, terms) >= 10.0, (label, U.worst_excess(mutant, want, terms))
        with pytest.raises(AssertionError):
            U.assert_row(mutant, want, terms, label)
    # ... and on the big tensors alone, where a dropped element or a swapped operand weighs least
    big = np.flatnonzero(table[:, 1] - table[:, 0] >= 4096)
    for label, mutant in (("fp32 accumulation", fp32), ("p_old for p_new", swapped), ("a dropped last element", dropped)):
        pick = lambda r: {"entry": r["entry"][big]}          # noqa: E731
        assert U.worst_excess(pick(mutant), pick(want), terms[big]) >= 10.0, label


# ------------------------------------------------------------------------------------------------ the real layout ----
@pytest.fixture(scope="module")
def watched(lib):
    from svit_amd import optim, updmon
    cfg, model = _cpu_model()
    opt = optim.GuardedClipAdamW(model, lr=1e-3)
    return cfg, model, opt, updmon.UpdateMonitor(opt, period=4)


def _fill(mon, rows):
    """a ring's bytes: rows = [(slot, step, flags, entries or None)]"""
    from svit_amd import updmon
    ring = updmon.empty_ring(mon.period, len(mon.names))
    for slot, step, flags, entries in rows:
        ring[slot]["head"] = (step, flags, 0)
        ring[slot]["entry"]["n_still"] = 0
        if entries is not None:
            ring[slot]["entry"] = entries
    return ring.view(np.uint8).reshape(-1)


def _read(mon, rows):
    """read() over a ring filled by hand (the ring of a monitor built on the CPU is host memory)"""
    mon.ring.copy_(torch.from_numpy(_fill(mon, rows).copy()))
    return mon.read()


def test_monitor_over_the_real_405_tensors(watched):
    from svit_amd import lrscale, updmon
    cfg, model, opt, mon = watched
    flat = model.flat
    assert len(mon.names) == 405 and set(mon.names) == set(flat.slots)
    assert (mon.table[:, 0] % 4 == 0).all() and (np.diff(mon.table[:, 0]) > 0).all() and mon.table[-1, 1] <= flat.total
    assert mon.ring.numel() == 4 * (16 + 64 * 405) and mon.ring.dtype == torch.uint8 and not mon.frozen.any()
    assert mon.shadow.numel() == flat.total and mon.shadow.dtype == torch.float32
    assert mon.workspace.numel() == ((flat.total + 4095) // 4096 + 405) * 64
    assert mon.numel.tolist() == [flat.slots[k][1] for k in mon.names]
    assert mon.last_read == -1 and not hasattr(mon, "state_dict") and list(opt.state_dict()) == ["state", "param_groups"]
    m, v = mon._moments()
    assert m is opt.exp_avg and v is opt.exp_avg_sq
    depth = cfg.MVIT.DEPTH
    assert mon.depth == depth and mon.layer_ids.tolist() == [lrscale.layer_id(k, depth) for k in mon.names]
    rng = np.random.default_rng(5)
    po = rng.standard_normal(flat.total).astype(np.float32)
    pn = (po * (1 + 1e-3 * rng.standard_normal(flat.total))).astype(np.float32)
    g, mm = rng.standard_normal(flat.total).astype(np.float32), rng.standard_normal(flat.total).astype(np.float32)
    vv = mm * mm
    e = updmon.update_host(po, pn, g, mm, vv, mon.table)["entry"]
    rows = _read(mon, ([(1, 1, 3, e)]))
    assert rows["steps"].tolist() == [1] and rows["flags"].tolist() == [3] and rows["lost"] == 1           # step 0 never came
    assert rows["ratio"].shape == (1, 405) and not np.ma.is_masked(rows["ratio"])
    assert np.array_equal(rows["update_norm"].data[0], np.sqrt(e["sumsq_d"]))
    assert np.array_equal(rows["ratio"].data[0], np.sqrt(e["sumsq_d"]) / np.sqrt(e["sumsq_p"]))
    assert np.array_equal(rows["cos_grad"].data[0], -e["dot_dg"] / (np.sqrt(e["sumsq_d"]) * np.sqrt(e["sumsq_g"])))
    assert np.array_equal(rows["m_rms"].data[0], np.sqrt(e["sumsq_m"] / mon.numel))
    assert np.array_equal(rows["v_mean"].data[0], e["sum_v"] / mon.numel)
    assert np.array_equal(rows["absmax"].data[0], e["absmax_d"]) and np.array_equal(rows["n_one_ulp"].data[0], e["n_one_ulp"])
    assert abs(rows["ratio"].data[0]).max() < 0.01 and abs(rows["cos_grad"].data[0]).max() <= 1.0
    L = mon.by_layer(rows)
    assert L["ratio"].shape == (1, depth + 2) and not np.ma.is_masked(L["ratio"])
    for lid in range(depth + 2):
        own = [t for t, k in enumerate(mon.names) if lrscale.layer_id(k, depth) == lid]
        assert own, lid
        sd = sum(float(np.sum((pn[a:b].astype(np.float64) - po[a:b].astype(np.float64)) ** 2)) for a, b in mon.table[own])
        sp = sum(float(np.sum(pn[a:b].astype(np.float64) ** 2)) for a, b in mon.table[own])
        assert abs(L["update_norm"][0, lid] - np.sqrt(sd)) <= 1e-12 * np.sqrt(sd), lid
        assert abs(L["weight_norm"][0, lid] - np.sqrt(sp)) <= 1e-12 * np.sqrt(sp), lid
        assert L["ratio"][0, lid] == L["update_norm"][0, lid] / L["weight_norm"][0, lid]
        assert L["numel"][0, lid] == sum(int(mon.numel[t]) for t in own)
        assert L["n_still"][0, lid] == sum(int(e["n_still"][t]) for t in own)
    stats = mon.log_stats(rows)
    assert stats["_type"] == "train_update_stats" and stats["step"] == 1 and len(stats["ratio"]) == depth + 2
    assert stats["lost"] == 1 and stats["flags"] == 3 and stats["n_stalled"] == len(mon.stalled(rows))
    import json
    json.dumps(stats)
    mon.last_read = -1


def test_stalled_names_the_tensors_that_did_not_move(watched):
    from svit_amd import updmon
    cfg, model, opt, mon = watched
    mon.last_read = -1
    e = updmon.empty_ring(1, 405)["entry"][0]
    e["n_still"] = 0
    picks = {"blocks.0.norm1.weight": 1.0, "blocks.0.norm1.bias": 0.5, "blocks.3.attn.rel_pos_h": 0.49, "head.projection.bias": 0.75}
    picks = {k: f for k, f in picks.items() if k in mon.names}
    assert len(picks) >= 3
    want = {}
    for k, frac in picks.items():
        t = mon.names.index(k)
        e[t]["n_still"] = int(np.ceil(frac * mon.numel[t])) if frac >= 0.5 else int(np.floor(frac * mon.numel[t]))
        want[k] = (int(e[t]["n_still"]), int(mon.numel[t]))
    moving = e.copy()
    moving["n_still"] = 0
    rows = _read(mon, [(0, 4, 3, moving), (1, 5, 3, e)])
    found = mon.stalled(rows)
    assert sorted(found) == sorted((5, k, *want[k]) for k, f in picks.items() if f >= 0.5)
    assert all(s == 5 for s, _, _, _ in found)
    strict = mon.stalled(rows, min_fraction=0.9)
    assert [k for _, k, _, _ in strict] == [k for k in mon.names if picks.get(k, 0) >= 0.9]
    assert len(mon.stalled(rows, min_fraction=0.4)) == len(picks)
    stats = mon.log_stats(rows)
    assert stats["n_stalled"] == len(found) and sorted(x[0] for x in stats["stalled"]) == sorted(k for _, k, _, _ in found)
    # a frozen tensor (n_still -1, masked) is never named, whatever the fraction
    mon.frozen = mon.frozen.copy()
    mon.frozen[0] = True
    try:
        mon.last_read = -1
        unwritten = e.copy()
        unwritten[0]["n_still"] = -1
        assert all(name != mon.names[0] for _, name, _, _ in mon.stalled(_read(mon, [(0, 8, 3, unwritten)]), min_fraction=0.0))
    finally:
        mon.frozen[0] = False
        mon.last_read = -1


def test_read_selects_rows_and_counts_the_lost(watched):
    cfg, model, opt, mon = watched
    mon.last_read = -1
    rows = _read(mon, ([(0, 0, 3, None), (1, 1, 3, None), (2, 2, 3, None), (3, 3, 3, None)]))
    assert rows["steps"].tolist() == [0, 1, 2, 3] and rows["lost"] == 0 and mon.last_read == 3
    again = _read(mon, ([(0, 0, 3, None), (1, 1, 3, None), (2, 2, 3, None), (3, 3, 3, None)]))
    assert again["steps"].tolist() == [] and again["lost"] == 0 and again["ratio"].shape == (0, 405) and mon.last_read == 3
    # R = 4: steps 4..9 pass, rows hold 8, 9, 6, 7 -- steps 4 and 5 are lost
    rows = _read(mon, ([(0, 8, 3, None), (1, 9, 3, None), (2, 6, 3, None), (3, 7, 3, None)]))
    assert rows["steps"].tolist() == [6, 7, 8, 9] and rows["lost"] == 2 and mon.last_read == 9
    # a row older than the last read that was never overwritten is not returned again; a dropped step (11: no row, the
    # guard's doing) counts among the lost up to the newest row
    rows = _read(mon, ([(0, 12, 3, None), (1, 9, 3, None), (2, 10, 3, None), (3, 7, 3, None)]))
    assert rows["steps"].tolist() == [10, 12] and rows["lost"] == 1 and mon.last_read == 12
    # every = 5: due steps are the multiples
    mon.every, mon.last_read = 5, -1
    try:
        rows = _read(mon, ([(0, 20, 1, None), (1, 5, 1, None), (2, 10, 1, None), (3, 15, 1, None)]))
        assert rows["steps"].tolist() == [5, 10, 15, 20] and rows["lost"] == 1 and rows["flags"].tolist() == [1] * 4   # step 0
        rows = _read(mon, ([(0, 40, 1, None), (1, 25, 1, None), (2, 30, 1, None), (3, 15, 1, None)]))
        assert rows["steps"].tolist() == [25, 30, 40] and rows["lost"] == 1                                           # step 35
    finally:
        mon.every, mon.last_read = 1, -1
    # reset(): the ring as it was created
    from svit_amd import updmon
    mon.reset()
    assert mon.ring.numpy().tobytes() == updmon.empty_ring(4, 405).tobytes() and mon.last_read == -1


# ------------------------------------------------------------------------------------------------------ refusals ----
def test_refusals_by_message(lib):
    from svit_amd import optim, updmon
    cfg, model = _cpu_model()
    classic = optim.FusedClipAdamW(model, lr=1e-3)
    with pytest.raises(TypeError, match="GuardedClipAdamW or one of its subclasses, got FusedClipAdamW"):
        updmon.UpdateMonitor(classic, 10)
    opt = optim.GuardedClipAdamW(model, lr=1e-3)
    for kw in (dict(period=0), dict(period=-1), dict(period=2.0), dict(period=True), dict(period=4, every=0),
               dict(period=4, every="1")):
        with pytest.raises(ValueError, match="^UpdateMonitor: .* is a positive int, got"):
            updmon.UpdateMonitor(opt, **kw)
    assert updmon.build_update_monitor(cfg, opt) is None and opt.update_monitor is None          # no key
    assert updmon.build_update_monitor(cfg, classic) is None
    cfg.SVIT.UPDATE_MONITOR = True
    with pytest.raises(TypeError, match="^SVIT.UPDATE_MONITOR needs the guarded optimizer tail, got the classic FusedClipAdamW"):
        updmon.build_update_monitor(cfg, classic)
    for bad in (0, -1, 2.5, "3", True):
        cfg.SVIT.UPDATE_MONITOR_EVERY = bad
        with pytest.raises(ValueError, match="^SVIT.UPDATE_MONITOR_EVERY is a positive int, got "):
            updmon.build_update_monitor(cfg, opt)
    assert opt.update_monitor is None
    theirs = updmon.UpdateMonitor(optim.GuardedClipSGD(model, lr=0.1), 4)
    with pytest.raises(ValueError, match="^attach_update_monitor: the UpdateMonitor was built over another optimizer"):
        opt.attach_update_monitor(theirs)
    assert opt.update_monitor is None and not hasattr(classic, "attach_update_monitor")


def test_construct_optimizer_and_build_update_monitor_under_the_key(lib):
    from svit_amd import config, monitor, optim, updmon
    cfg, model = _cpu_model()
    assert "UPDATE_MONITOR" not in config.get_cfg().SVIT and "UPDATE_MONITOR_EVERY" not in config.get_cfg().SVIT
    s = cfg.SOLVER
    s.OPTIMIZING_METHOD, s.BASE_LR, s.WEIGHT_DECAY, s.CLIP_GRAD_L2NORM = "adamw", 1e-3, 0.05, 1.0
    plain = optim.construct_optimizer(model, cfg)
    assert type(plain) is optim.FusedClipAdamW and updmon.build_update_monitor(cfg, plain) is None
    cfg.SVIT.UPDATE_MONITOR = True
    cfg.LOG_PERIOD = 7
    opt = optim.construct_optimizer(model, cfg)
    assert type(opt) is optim.GuardedClipAdamW and opt.update_monitor is None and opt.monitor is None
    mon = updmon.build_update_monitor(cfg, opt)
    assert type(mon) is updmon.UpdateMonitor and opt.update_monitor is mon and (mon.period, mon.every) == (7, 1)
    assert monitor.build_monitor(cfg, opt) is None and opt.monitor is None                 # the other monitor has its own key
    cfg.SVIT.UPDATE_MONITOR_EVERY = 10
    assert updmon.build_update_monitor(cfg, opt).every == 10 and opt.update_monitor is not mon
    opt.attach_update_monitor(None)
    assert opt.update_monitor is None
    for method, cls, state in (("sgd", optim.GuardedClipSGD, 1), ("adam", optim.GuardedClipAdam, 2)):
        s.OPTIMIZING_METHOD = method
        s.MOMENTUM, s.DAMPENING, s.NESTEROV = 0.9, 0.0, True
        o = optim.construct_optimizer(model, cfg)
        um = updmon.build_update_monitor(cfg, o)
        assert type(o) is cls and um is o.update_monitor and um is not None
        assert [x is not None for x in um._moments()] == [True, state == 2]
    s.MOMENTUM, s.NESTEROV = 0.0, False
    s.OPTIMIZING_METHOD = "sgd"
    assert updmon.UpdateMonitor(optim.construct_optimizer(model, cfg), 4)._moments() == [None, None]
    # a frozen cut: the optimizer's segments decide what is watched
    s.OPTIMIZING_METHOD = "adamw"
    model.freeze_below(4)
    o = optim.construct_optimizer(model, cfg)
    um = updmon.build_update_monitor(cfg, o)
    assert um.segments is o.segments and 0 < int(um.frozen.sum()) < 405
    assert all(um.frozen[t] == (not p.requires_grad) for t, p in ((um.names.index(k), p) for k, p in model.named_parameters()))
    del cfg.SVIT["UPDATE_MONITOR"]
    assert updmon.build_update_monitor(cfg, o) is None
    assert type(optim.construct_optimizer(model, cfg)) is optim.FusedClipAdamW


def test_steps_remember_the_attachment():
    """graph._check_update_monitor, beside _check_monitor: the message names the step's class and what changed"""
    import types
    from svit_amd import graph, hip
    opt = types.SimpleNamespace(update_monitor=None)
    graph._check_update_monitor(opt, None, "GraphedTrainStep")
    mon = object()
    with pytest.raises(hip.SvitHipError, match="attached UpdateMonitor changed after this AccumulatedTrainStep was built "
                                               r"\(one then, none now\)"):
        graph._check_update_monitor(opt, mon, "AccumulatedTrainStep")
    opt.update_monitor = mon
    graph._check_update_monitor(opt, mon, "GraphedTrainStep")
    with pytest.raises(hip.SvitHipError, match=r"\(none then, one now\)"):
        graph._check_update_monitor(opt, None, "GraphedTrainStep")


def test_train_epoch_logs_one_line_per_period(watched, caplog):
    """train._log_update_stats, the call train_epoch makes behind _log_tensor_stats: nothing without a monitor or between
    periods, else ONE read and one json_stats line"""
    import json
    import logging
    from svit_amd import optim, train, updmon
    cfg, model, opt, mon = watched
    cfg.LOG_PERIOD = 4
    assert train._log_update_stats(optim.FusedClipAdamW(model, lr=1e-3), cfg, 3) is None
    assert opt.update_monitor is None and train._log_update_stats(opt, cfg, 3) is None
    opt.attach_update_monitor(mon)
    try:
        mon.last_read = -1
        e = updmon.empty_ring(1, 405)["entry"][0]
        e["n_still"], e["sumsq_d"], e["sumsq_p"] = 0, 4.0, 16.0
        t = mon.names.index("blocks.3.attn.rel_pos_h")
        e[t]["n_still"] = mon.numel[t]
        mon.ring.copy_(torch.from_numpy(_fill(mon, [(0, 0, 3, e), (2, 2, 3, e), (3, 3, 3, e)]).copy()))
        assert train._log_update_stats(opt, cfg, 2) is None and mon.last_read == -1          # not the period's end: no read
        with caplog.at_level(logging.INFO):
            stats = train._log_update_stats(opt, cfg, 3)
        assert mon.last_read == 3 and stats["_type"] == "train_update_stats" and stats["step"] == 3 and stats["rows"] == 3
        assert stats["lost"] == 1 and stats["ratio"] == [0.5] * (mon.depth + 2)
        assert stats["stalled"] == [[mon.names[t], int(mon.numel[t]), int(mon.numel[t])]] and stats["n_stalled"] == 1
        assert stats["still_fraction"] == float("%.6g" % (mon.numel[t] / mon.numel.sum()))
        lines = [r.getMessage() for r in caplog.records if "train_update_stats" in r.getMessage()]
        assert len(lines) == 1 and json.loads(lines[0].split("json_stats: ")[1])["step"] == 3
        assert train._log_update_stats(opt, cfg, 7) is None                                   # nothing new: no line
    finally:
        opt.attach_update_monitor(None)
        mon.last_read = -1
