"""Per-tensor statistics on the guarded tail, host side: the table validator and every argument refusal of the entry points
by error code, the workspace query, the NumPy yardstick on hand-made cases, by_layer on the real 405-tensor layout,
culprits' unravelling, build_monitor's refusals, and read()'s row selection and `lost` count on a ring filled by hand.
No GPU needed."""
import numpy as np
import pytest
import torch

from tests import monitor_cases as M


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


# ------------------------------------------------------------------------------------------------- the validator ----
GOOD = [[0, 5], [8, 9], [12, 108], [108, 4000], [4096, 20000]]
N = 20000


def test_table_validator_by_error_code(lib):
    def check(rows, n=N, Tn=None, null=False):
        t = _tab(rows)
        return lib.svit_tensor_table_check(None if null else t.ctypes.data, len(t) if Tn is None else Tn, n)

    assert check(GOOD) == 0
    assert check([[0, N]]) == 0 and check([[0, 1]]) == 0
    assert check([[4 * i, 4 * i + 3] for i in range(4096)], n=4 * 4096) == 0          # the limit itself
    bad_arg = {
        "NULL table": dict(rows=GOOD, null=True),
        "Tn = 0": dict(rows=GOOD, Tn=0),
        "Tn < 0": dict(rows=GOOD, Tn=-1),
        "Tn = 4097": dict(rows=[[4 * i, 4 * i + 3] for i in range(4097)], n=4 * 4097),
        "n = 0": dict(rows=GOOD, n=0),
        "unsorted": dict(rows=[[8, 12], [0, 4]]),
        "overlapping": dict(rows=[[0, 9], [8, 12]]),
        "empty": dict(rows=[[0, 4], [8, 8]]),
        "reversed": dict(rows=[[12, 8]]),
        "negative": dict(rows=[[-4, 4]]),
        "end > n": dict(rows=[[0, 4], [N - 4, N + 1]]),
        "2^31 elements": dict(rows=[[0, 2 ** 31 - 1]], n=2 ** 31),
    }
    for label, kw in bad_arg.items():
        assert check(**kw) == -4, label
    assert check([[0, 2 ** 31 - 2]], n=2 ** 31) == 0
    for label, rows in {"begin % 4": [[2, 8]], "a later begin": [[0, 4], [9, 12]], "begin = end of the last, odd": [[0, 5], [5, 8]]}.items():
        assert check(rows) == -3, label
    from svit_amd import hip, ops
    ops.tensor_table_check(_tab(GOOD), N)
    with pytest.raises(hip.SvitHipError, match="svit_tensor_table_check .* bad alignment"):
        ops.tensor_table_check(_tab([[2, 8]]), N)
    with pytest.raises(hip.SvitHipError, match="C-contiguous int64 numpy array"):
        ops.tensor_table_check(np.array(GOOD, dtype=np.int32), N)


def test_workspace_query(lib):
    from svit_amd import ops
    W = ops.tensor_stats_window()
    assert W == 4096
    q = lib.svit_tensor_stats_workspace
    assert q(1, 1) == 2 * 32 and q(W, 1) == 2 * 32 and q(W + 1, 1) == 3 * 32
    assert q(34_400_000, 405) == (8399 + 405) * 32 and ops.tensor_stats_workspace(5 * W, 80) == 85 * 32
    assert q(8, 4096) == 4097 * 32
    for n, Tn in ((0, 1), (-1, 1), (8, 0), (8, -1), (8, 4097)):
        assert q(n, Tn) == -4, (n, Tn)


def test_entry_point_checks_its_arguments_without_a_gpu(lib):
    """refused before any HIP call: stream = None and made-up device addresses that are never followed"""
    P = 4096
    need = lib.svit_tensor_stats_workspace(N, len(GOOD))

    def stats(rows=GOOD, n=N, Tn=None, host=True, segs=None, S=None, g=P, p=P, tdev=P, rec=P, ring=P, R=4, every=1,
              ws=P, ws_bytes=need, seg_ptr=True):
        t = _tab(rows)
        keep = _tab(segs) if segs is not None else None
        sp = keep.ctypes.data if keep is not None and seg_ptr else None
        return lib.svit_tensor_stats(g, p, n, tdev, t.ctypes.data if host else None, len(t) if Tn is None else Tn, sp,
                                     (0 if keep is None else len(keep)) if S is None else S, rec, ring, R, every, ws,
                                     ws_bytes, None)

    bad_arg = {
        "NULL g": dict(g=None), "NULL p": dict(p=None), "NULL device table": dict(tdev=None),
        "NULL host table": dict(host=False), "NULL dev_rec": dict(rec=None), "NULL ring": dict(ring=None),
        "NULL workspace": dict(ws=None), "R = 0": dict(R=0), "R < 0": dict(R=-2), "every = 0": dict(every=0),
        "every < 0": dict(every=-1), "n = 0": dict(n=0), "Tn = 0": dict(Tn=0),
        "Tn = 4097": dict(rows=[[4 * i, 4 * i + 3] for i in range(4097)], n=4 * 4097, ws_bytes=1 << 30),
        "table unsorted": dict(rows=[[8, 12], [0, 4]]), "table overlapping": dict(rows=[[0, 9], [8, 12]]),
        "table empty tensor": dict(rows=[[0, 4], [8, 8]]), "table end > n": dict(rows=[[0, 4], [N - 4, N + 1]]),
        "workspace one byte short": dict(ws_bytes=need - 1), "workspace negative": dict(ws_bytes=-1),
        "S = 65": dict(segs=[[8 * i, 8 * i + 4] for i in range(65)]), "S < 0": dict(S=-1),
        "S > 0 without a table": dict(segs=[[0, 8]], seg_ptr=False),
        "segments unsorted": dict(segs=[[4104, 4120], [0, 8]]), "segments overlapping": dict(segs=[[0, 16], [8, 24]]),
        "segment empty": dict(segs=[[0, 8], [16, 16]]), "segment end > n": dict(segs=[[0, 8], [N - 8, N + 4]]),
    }
    for label, kw in bad_arg.items():
        assert stats(**kw) == -4, label
    bad_align = {
        "a begin not a multiple of 4": dict(rows=[[0, 4], [9, 12]]), "a segment bound": dict(segs=[[0, 6]]),
        "g": dict(g=P + 4), "p": dict(p=P + 8), "ring": dict(ring=P + 8), "workspace": dict(ws=P + 8),
        "device table": dict(tdev=P + 4), "dev_rec": dict(rec=P + 4),
    }
    for label, kw in bad_align.items():
        assert stats(**kw) == -3, label
    # the limits themselves pass the checks: shown through the one check that comes after them (a misaligned g)
    for kw in (dict(), dict(segs=[[0, N]]), dict(segs=[[8 * i, 8 * i + 4] for i in range(64)]), dict(R=1, every=10 ** 9),
               dict(rows=[[4 * i, 4 * i + 3] for i in range(4096)], n=4 * 4096, ws_bytes=(4 + 4096) * 32),
               dict(S=0, seg_ptr=False)):
        assert stats(g=P + 4, **kw) == -3, kw


# ------------------------------------------------------------------------------------------------- the yardstick ----
def test_stats_host_on_hand_made_cases():
    from svit_amd import monitor
    g = np.zeros(32, dtype=np.float32)
    p = np.zeros(32, dtype=np.float32)
    table = _tab([[0, 3], [4, 8], [8, 16], [20, 21], [24, 31]])
    g[0:3] = [3.0, -4.0, 12.0]
    p[0:3] = [1.0, 2.0, 2.0]
    g[3] = np.nan                                    # padding: never counted
    g[4:8] = [1.0, np.nan, -7.0, np.inf]
    p[4:8] = 0.5
    g[8:16] = -0.25
    g[20] = -np.inf
    g[24:31] = [1e30, 0.0, -0.0, M.DENORMAL, 2e30, -1.0, 1.0]
    e = monitor.stats_host(g, p, table)
    assert e.dtype == monitor.ENTRY and e.shape == (5,) and monitor.ENTRY.itemsize == 32 and monitor.HEADER.itemsize == 16
    assert e["sumsq_g"].tolist() == [169.0, 50.0, 0.5, 0.0, float(np.float32(1e30)) ** 2 + float(np.float32(2e30)) ** 2
                                     + float(M.DENORMAL) ** 2 + 2.0]
    assert e["sumsq_p"].tolist() == [9.0, 1.0, 0.0, 0.0, 0.0]
    assert e["absmax_g"].tolist() == [12.0, 7.0, 0.25, 0.0, float(np.float32(2e30))]
    assert e["n_bad"].tolist() == [0, 2, 0, 1, 0] and e["first_bad"].tolist() == [-1, 1, -1, 0, -1]
    with np.errstate(over="ignore"):
        assert np.isfinite(e["sumsq_g"][4]) and not np.isfinite(np.float32(1e30) * np.float32(1e30))
    # frozen tensors keep the empty ring's entry; a NaN in them is not seen
    e = monitor.stats_host(g, p, table, segs=_tab([[0, 4], [8, 16]]))
    assert e["n_bad"].tolist() == [0, -1, 0, -1, -1] and e["first_bad"].tolist() == [-1] * 5
    assert e["sumsq_g"].tolist() == [169.0, 0.0, 0.5, 0.0, 0.0]
    assert monitor.trainable_mask(table, _tab([[0, 4], [8, 16]])).tolist() == [True, False, True, False, False]
    assert monitor.TensorMonitor.stats_host is monitor.stats_host
    ring = monitor.empty_ring(3, 5)
    assert ring.itemsize == 16 + 32 * 5 and (ring["head"]["step"] == -1).all() and (ring["entry"]["n_bad"] == -1).all()
    assert ring["entry"]["sumsq_g"].sum() == 0 and (ring["entry"]["first_bad"] == -1).all()


def test_cases_layout_is_what_the_issue_lists():
    W = 4096
    table, n, where = M.layout(W)
    sizes = (table[:, 1] - table[:, 0]).tolist()
    assert sizes[:4] == [1, 3, 4, 96] and sizes[4:74] == [4] * 70 and sizes[74] == W - 1 and sizes[76:79] == [W, W + 1, 3 * W + 5]
    assert (table[:, 0] % 4 == 0).all() and table[where["W"]].tolist() == [2 * W, 3 * W] and n % 4 == 1
    assert table[-1, 1] == n and 5 * W < n < 8 * W


# ------------------------------------------------------------------------------------------------ the real layout ----
@pytest.fixture(scope="module")
def watched(lib):
    from svit_amd import monitor, optim
    cfg, model = _cpu_model()
    opt = optim.GuardedClipAdamW(model, lr=1e-3, grad_scale=0.5)
    return cfg, model, opt, monitor.TensorMonitor(opt, period=4)


def _fill(mon, rows):
    """a ring's bytes: rows = [(slot, step, apply, entries or None)]"""
    from svit_amd import monitor
    ring = monitor.empty_ring(mon.period, len(mon.names))
    for slot, step, apply, entries in rows:
        ring[slot]["head"] = (step, apply, 0)
        if entries is not None:
            ring[slot]["entry"] = entries
    return ring.view(np.uint8).reshape(-1)


def _read(mon, rows):
    """read() over a ring filled by hand (the ring of a monitor built on the CPU is host memory)"""
    mon.ring.copy_(torch.from_numpy(_fill(mon, rows).copy()))
    return mon.read()


def test_monitor_over_the_real_405_tensors(watched):
    from svit_amd import lrscale, monitor
    cfg, model, opt, mon = watched
    flat = model.flat
    assert len(mon.names) == 405 and set(mon.names) == set(flat.slots)
    assert (mon.table[:, 0] % 4 == 0).all() and (np.diff(mon.table[:, 0]) > 0).all() and mon.table[-1, 1] <= flat.total
    assert [tuple(flat.slots[k][2]) for k in mon.names] == mon.shapes
    assert mon.ring.numel() == 4 * (16 + 32 * 405) and mon.ring.dtype == torch.uint8 and not mon.frozen.any()
    assert mon.table_dev.dtype == torch.int64 and mon.table_dev.numpy().tolist() == mon.table.tolist()
    assert mon.workspace.numel() == ((flat.total + 4095) // 4096 + 405) * 32
    assert mon.last_read == -1 and not hasattr(mon, "state_dict") and list(opt.state_dict()) == ["state", "param_groups"]
    depth = cfg.MVIT.DEPTH
    assert mon.depth == depth and mon.layer_ids.tolist() == [lrscale.layer_id(k, depth) for k in mon.names]
    # by_layer against the ids: random weights and gradients through the yardstick
    rng = np.random.default_rng(5)
    g = rng.standard_normal(flat.total).astype(np.float32)
    p = rng.standard_normal(flat.total).astype(np.float32)
    e = monitor.stats_host(g, p, mon.table)
    rows = _read(mon, ([(1, 1, 1, e)]))
    assert rows["steps"].tolist() == [1] and rows["applied"].tolist() == [True] and rows["lost"] == 1     # step 0 never came
    assert rows["grad_norm"].shape == (1, 405) and not np.ma.is_masked(rows["grad_norm"])
    assert np.array_equal(rows["grad_norm"].data[0], np.sqrt(e["sumsq_g"]) * 0.5)                          # grad_scale
    assert np.array_equal(rows["weight_norm"].data[0], np.sqrt(e["sumsq_p"]))
    L = mon.by_layer(rows)
    assert L["grad_norm"].shape == (1, depth + 2) and not np.ma.is_masked(L["ratio"])
    for lid in range(depth + 2):
        own = [t for t, k in enumerate(mon.names) if lrscale.layer_id(k, depth) == lid]
        assert own, lid
        sg = sum(float(np.sum(g[a:b].astype(np.float64) ** 2)) for a, b in mon.table[own])
        sp = sum(float(np.sum(p[a:b].astype(np.float64) ** 2)) for a, b in mon.table[own])
        assert abs(L["grad_norm"][0, lid] - 0.5 * np.sqrt(sg)) <= 1e-12 * np.sqrt(sg), lid
        assert abs(L["weight_norm"][0, lid] - np.sqrt(sp)) <= 1e-12 * np.sqrt(sp), lid
        assert L["ratio"][0, lid] == L["grad_norm"][0, lid] / L["weight_norm"][0, lid]
    stats = mon.log_stats(rows)
    assert stats["_type"] == "train_tensor_stats" and stats["step"] == 1 and len(stats["ratio"]) == depth + 2
    assert stats["culprits"] == [] and stats["lost"] == 1
    import json
    json.dumps(stats)
    mon.last_read = -1


def test_culprits_unravel_the_first_offset(watched):
    from svit_amd import monitor
    cfg, model, opt, mon = watched
    mon.last_read = -1
    name = "blocks.3.attn.rel_pos_h"
    t = mon.names.index(name)
    shape = mon.shapes[t]
    assert len(shape) == 2
    e = monitor.empty_ring(1, 405)["entry"][0]
    e["n_bad"] = 0
    e[t]["n_bad"], e[t]["first_bad"] = 3, 2 * shape[1] + 5
    t4 = [i for i, s in enumerate(mon.shapes) if len(s) >= 3 and min(s) >= 1][0]
    idx4 = tuple(min(j % 3, d - 1) for j, d in enumerate(mon.shapes[t4], 1))
    e[t4]["n_bad"], e[t4]["first_bad"] = 1, int(np.ravel_multi_index(idx4, mon.shapes[t4]))
    ok = e.copy()
    ok["n_bad"] = 0
    rows = _read(mon, ([(0, 4, 1, ok), (1, 5, 0, e), (2, 6, 1, ok)]))
    assert rows["steps"].tolist() == [4, 5, 6] and rows["applied"].tolist() == [True, False, True]
    found = mon.culprits(rows)
    first, second = sorted([t, t4])
    want = {t: (5, name, 3, (2, 5)), t4: (5, mon.names[t4], 1, idx4)}
    assert found == [want[first], want[second]]
    assert mon.log_stats(rows)["culprits"] == [[s, n, nb, list(i)] for s, n, nb, i in found]
    mon.last_read = -1


def test_read_selects_rows_and_counts_the_lost(watched):
    cfg, model, opt, mon = watched
    mon.last_read = -1
    # R = 4: steps 0..3 recorded, read; then steps 4..9 pass: rows hold 8, 9, 6, 7 -- steps 4 and 5 are lost
    rows = _read(mon, ([(0, 0, 1, None), (1, 1, 1, None), (2, 2, 0, None), (3, 3, 1, None)]))
    assert rows["steps"].tolist() == [0, 1, 2, 3] and rows["applied"].tolist() == [True, True, False, True]
    assert rows["lost"] == 0 and mon.last_read == 3
    again = _read(mon, ([(0, 0, 1, None), (1, 1, 1, None), (2, 2, 0, None), (3, 3, 1, None)]))
    assert again["steps"].tolist() == [] and again["lost"] == 0 and again["grad_norm"].shape == (0, 405) and mon.last_read == 3
    rows = _read(mon, ([(0, 8, 1, None), (1, 9, 1, None), (2, 6, 1, None), (3, 7, 0, None)]))
    assert rows["steps"].tolist() == [6, 7, 8, 9] and rows["lost"] == 2 and mon.last_read == 9
    # a row older than the last read that was never overwritten is not returned again
    rows = _read(mon, ([(0, 8, 1, None), (1, 9, 1, None), (2, 10, 1, None), (3, 7, 0, None)]))
    assert rows["steps"].tolist() == [10] and rows["lost"] == 0
    # every = 5: due steps are the multiples; a dropped step between them is a row of its own and not "due"
    mon.every, mon.last_read = 5, -1
    try:
        rows = _read(mon, ([(0, 20, 1, None), (1, 5, 1, None), (2, 10, 1, None), (3, 15, 1, None)]))
        assert rows["steps"].tolist() == [5, 10, 15, 20] and rows["lost"] == 1            # step 0
        rows = _read(mon, ([(0, 40, 1, None), (1, 25, 1, None), (2, 30, 1, None), (3, 27, 0, None)]))
        assert rows["steps"].tolist() == [25, 27, 30, 40] and rows["lost"] == 1           # step 35
    finally:
        mon.every, mon.last_read = 1, -1


# ------------------------------------------------------------------------------------------------------ refusals ----
def test_refusals_by_message(lib):
    from svit_amd import monitor, optim
    cfg, model = _cpu_model()
    classic = optim.FusedClipAdamW(model, lr=1e-3)
    with pytest.raises(TypeError, match="GuardedClipAdamW or one of its subclasses, got FusedClipAdamW"):
        monitor.TensorMonitor(classic, 10)
    opt = optim.GuardedClipAdamW(model, lr=1e-3)
    for kw in (dict(period=0), dict(period=-1), dict(period=2.0), dict(period=True), dict(period=4, every=0),
               dict(period=4, every="1")):
        with pytest.raises(ValueError, match="is a positive int, got"):
            monitor.TensorMonitor(opt, **kw)
    assert monitor.build_monitor(cfg, opt) is None and opt.monitor is None          # no key
    cfg.SVIT.MONITOR = True
    with pytest.raises(TypeError, match="got FusedClipAdamW"):
        monitor.build_monitor(cfg, classic)
    for bad in (0, -1, 2.5, "3", True):
        cfg.SVIT.MONITOR_EVERY = bad
        with pytest.raises(ValueError, match="^SVIT.MONITOR_EVERY is a positive int, got "):
            monitor.build_monitor(cfg, opt)
    assert opt.monitor is None
    theirs = monitor.TensorMonitor(optim.GuardedClipSGD(model, lr=0.1), 4)
    with pytest.raises(ValueError, match="^attach_monitor: the TensorMonitor was built over another optimizer"):
        opt.attach_monitor(theirs)
    assert opt.monitor is None


def test_construct_optimizer_and_build_monitor_under_the_key(lib):
    from svit_amd import config, monitor, optim
    cfg, model = _cpu_model()
    assert "MONITOR" not in config.get_cfg().SVIT and "MONITOR_EVERY" not in config.get_cfg().SVIT
    s = cfg.SOLVER
    s.OPTIMIZING_METHOD, s.BASE_LR, s.WEIGHT_DECAY, s.CLIP_GRAD_L2NORM = "adamw", 1e-3, 0.05, 1.0
    plain = optim.construct_optimizer(model, cfg)
    assert type(plain) is optim.FusedClipAdamW and monitor.build_monitor(cfg, plain) is None
    cfg.SVIT.MONITOR = True
    cfg.LOG_PERIOD = 7
    opt = optim.construct_optimizer(model, cfg)
    assert type(opt) is optim.GuardedClipAdamW and opt.monitor is None
    mon = monitor.build_monitor(cfg, opt)
    assert type(mon) is monitor.TensorMonitor and opt.monitor is mon and (mon.period, mon.every) == (7, 1)
    cfg.SVIT.MONITOR_EVERY = 10
    assert monitor.build_monitor(cfg, opt).every == 10 and opt.monitor is not mon
    opt.attach_monitor(None)
    assert opt.monitor is None
    for method, cls in (("sgd", optim.GuardedClipSGD), ("adam", optim.GuardedClipAdam)):
        s.OPTIMIZING_METHOD = method
        s.MOMENTUM, s.DAMPENING, s.NESTEROV = 0.9, 0.0, True
        o = optim.construct_optimizer(model, cfg)
        assert type(o) is cls and monitor.build_monitor(cfg, o) is o.monitor and o.monitor is not None
    # a frozen cut: the optimizer's segments decide what is watched
    model.freeze_below(4)
    o = optim.construct_optimizer(model, cfg)
    m = monitor.build_monitor(cfg, o)
    assert m.segments is o.segments and 0 < int(m.frozen.sum()) < 405
    assert all(m.frozen[t] == (not p.requires_grad) for t, p in ((m.names.index(k), p) for k, p in model.named_parameters()))
    del cfg.SVIT["MONITOR"]
    s.OPTIMIZING_METHOD = "adamw"
    assert monitor.build_monitor(cfg, o) is None


def test_check_names_the_culprits_only_with_a_monitor(lib):
    """check()'s message: unchanged without a monitor, one more line with one (the ring and the record filled by hand)"""
    from svit_amd import monitor, optim
    _, model = _cpu_model()
    opt = optim.GuardedClipAdamW(model, lr=1e-3, max_consecutive_skips=1)
    rec = opt.dev_rec.view(torch.int64)
    rec[0], rec[1] = 2, 1                  # two applied, one dropped: the last step is index 2
    opt.dev_rec[4] = 1                     # consecutive
    with pytest.raises(RuntimeError) as bare:
        opt.check()
    assert str(bare.value) == ("the last 1 optimizer steps were dropped for non-finite gradients (limit 1; 2 applied, 1 "
                               "dropped in all, last finite grad norm 0)")
    mon = monitor.TensorMonitor(opt, 4)
    assert mon.last_read == 2
    opt.attach_monitor(mon)
    e = monitor.empty_ring(1, 405)["entry"][0]
    e["n_bad"] = 0
    names = ["blocks.%d.attn.rel_pos_h" % i for i in range(10)]
    for k in names:
        t = mon.names.index(k)
        e[t]["n_bad"], e[t]["first_bad"] = 1, mon.shapes[t][1] + 2
    mon.ring.copy_(torch.from_numpy(_fill(mon, [(2, 2, 0, e), (1, 1, 1, None)]).copy()))
    with pytest.raises(RuntimeError) as told:
        opt.check()
    head, line = str(told.value).split("\n")
    assert head == str(bare.value)
    assert line.startswith("non-finite gradients of step 2 in 10 tensors: ") and line.endswith(" and 2 more")
    listed = [k for k in names if k + " (1 non-finite, the first at [1, 2])" in line]
    assert len(listed) == 8 and mon.last_read == 2


def test_train_epoch_logs_one_line_per_period(watched, caplog):
    """train._log_tensor_stats, the call train_epoch makes behind log_iter_stats: nothing without a monitor or between
    periods, else ONE read and one json_stats line with the by_layer numbers of the period's last recorded step"""
    import json
    import logging
    from svit_amd import monitor, optim, train
    cfg, model, opt, mon = watched
    cfg.LOG_PERIOD = 4
    assert train._log_tensor_stats(optim.FusedClipAdamW(model, lr=1e-3), cfg, 3) is None
    assert opt.monitor is None and train._log_tensor_stats(opt, cfg, 3) is None
    opt.attach_monitor(mon)
    try:
        mon.last_read = -1
        e = monitor.empty_ring(1, 405)["entry"][0]
        e["n_bad"], e["sumsq_g"], e["sumsq_p"] = 0, 4.0, 16.0
        bad = e.copy()
        t = mon.names.index("blocks.3.attn.rel_pos_h")
        bad[t]["n_bad"], bad[t]["first_bad"] = 2, 7
        mon.ring.copy_(torch.from_numpy(_fill(mon, [(0, 0, 1, e), (1, 1, 0, bad), (2, 2, 1, e), (3, 3, 1, e)]).copy()))
        assert train._log_tensor_stats(opt, cfg, 2) is None and mon.last_read == -1          # not the period's end: no read
        with caplog.at_level(logging.INFO):
            stats = train._log_tensor_stats(opt, cfg, 3)
        assert mon.last_read == 3 and stats["_type"] == "train_tensor_stats" and stats["step"] == 3 and stats["rows"] == 4
        assert stats["lost"] == 0 and stats["applied"] is True and stats["culprits"] == [[1, mon.names[t], 2, [0, 7]]]
        per_layer = np.bincount(mon.layer_ids, minlength=mon.depth + 2)
        assert stats["grad_norm"] == [float("%.6g" % (0.5 * np.sqrt(4.0 * k))) for k in per_layer]      # grad_scale 0.5
        assert stats["ratio"] == [0.25] * (mon.depth + 2)
        lines = [r.getMessage() for r in caplog.records if "train_tensor_stats" in r.getMessage()]
        assert len(lines) == 1 and json.loads(lines[0].split("json_stats: ")[1])["step"] == 3
        assert train._log_tensor_stats(opt, cfg, 7) is None                                   # nothing new: no line
    finally:
        opt.attach_monitor(None)
        mon.last_read = -1
