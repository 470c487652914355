"""Weight EMA on the guarded tail, host side: the NumPy restatement against float64, the warm-up table against its closed
form, every argument refusal of the two entry points, the state's names and shapes, build_ema's refusals and
construct_optimizer's dispatch under SVIT.EMA_DECAY.  No GPU needed."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import ema_cases as E


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
    for n, p in model.named_parameters():           # (as finalize() does: the parameters are views of the flat buffer)
        model.flat.p(n).copy_(p.data)
        p.data = model.flat.p(n)
    return cfg, model


# ------------------------------------------------------------------------------------- restatement against float64 ----
N_EL, STEPS = 65536, 200
DECAYS = {"decay 0.9999": (0.9999, False), "decay 0.999": (0.999, False), "warm-up table": (0.9999, True)}


@pytest.fixture(scope="module")
def inputs():
    rng = np.random.default_rng(22)
    e0 = (rng.standard_normal(N_EL) * 0.02).astype(np.float32)
    # a fresh p per update, off the average's mean so that the average has somewhere to go
    return e0, [(0.05 + rng.standard_normal(N_EL) * 0.02).astype(np.float32) for _ in range(STEPS)]


@pytest.mark.parametrize("name", list(DECAYS))
def test_restatement_against_float64(lib, inputs, name):
    """200 updates on 65 536 elements with a fresh random p per update.  The decay of an update is a float32 -- the
    kernel's argument or an entry of its float32 table -- so all three runs take that very number: float64 evaluates
    e d + p (1 - d) with it exactly, torch's fp32 `e.mul_(d).add_(p, alpha=1 - d)` and the restatement round.
    Bar, the solvers' own form: max |restatement - f64| <= 2 x max |torch fp32 - f64|.
    Measured, restatement / torch fp32: 1.00 in all three (errors 2.0e-7 at 0.9999, 1.1e-7 at 0.999, 2.2e-8 through the
    warm-up table, the same on both sides: torch's CPU kernel rounds as the restatement does; the run prints its own
    figures)."""
    from svit_amd import ema, ops
    decay, warmup = DECAYS[name]
    e0, ps = inputs
    table = ops.ema_decay_table(decay) if warmup else None
    ours = e0.copy()
    t32, t64 = torch.from_numpy(e0.copy()), torch.from_numpy(e0.astype(np.float64))
    for k, p in enumerate(ps, 1):
        d = ema.decay_at(k, decay, table)
        assert d.dtype == np.float32 and (warmup and d == E.warmup_closed_form(decay, k) or d == np.float32(decay))
        ours = ema.ema_step_host(ours, p, d)
        t32.mul_(float(d)).add_(torch.from_numpy(p), alpha=1.0 - float(d))
        t64.mul_(float(d)).add_(torch.from_numpy(p.astype(np.float64)), alpha=1.0 - float(d))
    assert ours.dtype == np.float32
    exact = t64.numpy()
    err = float(np.abs(ours.astype(np.float64) - exact).max())
    theirs = float(np.abs(t32.double().numpy() - exact).max())
    print("%s: max |restatement - f64| %.3e, max |torch fp32 - f64| %.3e, ratio %.2f" % (name, err, theirs, err / theirs))
    assert theirs > 0 and float(np.median(np.abs(exact - e0))) > 1e-4    # the updates moved the average
    assert err <= 2.0 * theirs, (name, err, theirs)


def test_restatement_is_the_formula_operation_by_operation():
    from svit_amd import ema
    e = np.array([1.0, -2.0, 3.0, 0.1], dtype=np.float32)
    p = np.array([0.5, 0.25, -4.0, 0.3], dtype=np.float32)
    d = np.float32(1.0 / 3.0)
    omd = np.float32(1) - d
    got = ema.ema_step_host(e, p, 1.0 / 3.0)            # (a double is taken to float32 first)
    assert got.dtype == np.float32 and np.array_equal(got, (e * d).astype(np.float32) + (p * omd).astype(np.float32))
    # not the fused form: somewhere in a random sample the once-rounded products differ from the exact ones
    rng = np.random.default_rng(3)
    e, p = rng.standard_normal(4096).astype(np.float32), rng.standard_normal(4096).astype(np.float32)
    fused = (e.astype(np.float64) * np.float64(d) + p.astype(np.float64) * np.float64(omd)).astype(np.float32)
    assert not np.array_equal(ema.ema_step_host(e, p, d), fused)
    assert ema.decay_at(0, 0.9) == ema.decay_at(-5, 0.9) == np.float32(0.9)
    t = np.array([0.25, 0.5], dtype=np.float32)
    assert [float(ema.decay_at(k, 0.9, t)) for k in (-1, 0, 1, 2, 3)] == [0.25, 0.25, 0.25, 0.5, float(np.float32(0.9))]


# ------------------------------------------------------------------------------------------------- decay table ----
@pytest.mark.parametrize("decay", [0.9999, 0.999, 0.9, 0.5, 0.1])
def test_decay_table_against_the_closed_form(lib, decay):
    from svit_amd import ops
    t = ops.ema_decay_table(decay)
    assert t.dtype == np.float32 and len(t) == E.warmup_length(decay)
    assert E.same_np(t, E.warmup_closed_form(decay, np.arange(1, len(t) + 1)))
    assert t[-1] == np.float32(decay) and (len(t) == 1 or t[-2] < np.float32(decay))
    assert bool((np.diff(t) >= 0).all())                 # (neighbours may round to one float32 near the end)
    if decay == 0.9999:
        assert len(t) == 89949              # "about 9 x 10^4"
    if decay == 0.999:
        assert len(t) == 8990


def test_decay_table_contract(lib):
    n = C.c_int64(-1)
    f = lib.svit_ema_decay_table
    assert f(0.999, None, 0, C.byref(n)) == 0 and n.value == 8990       # NULL table: the length alone
    buf = np.full(8990 + 8, -1.0, dtype=np.float32)
    assert f(0.999, buf.ctypes.data, 8989, C.byref(n)) == -4            # a table shorter than the length
    assert f(0.999, buf.ctypes.data, -1, C.byref(n)) == -4
    assert f(0.999, buf.ctypes.data, 8990, C.byref(n)) == 0 and n.value == 8990
    assert buf[8989] == np.float32(0.999) and bool((buf[8990:] == -1.0).all())      # nothing past the length is written
    assert f(0.999, None, 0, None) == -4                                 # nowhere to put the length
    # 9 / (1 - d) updates to reach d: above 2^20 from 0.99999142 on
    assert f(0.99999, None, 0, C.byref(n)) == 0 and 2 ** 19 < n.value <= 2 ** 20
    assert f(0.999999, None, 0, C.byref(n)) == -4
    for bad in (0.0, -0.0, 1.0, -0.5, 1.5, float("nan"), float("inf"), -float("inf")):
        assert f(bad, None, 0, C.byref(n)) == -4, bad


# ---------------------------------------------------------------------------------------------------- refusals ----
def test_entry_point_checks_its_arguments_without_a_gpu(lib):
    """refused before any HIP call: stream = None and made-up device addresses that are never followed"""
    P = 4096
    N = 20000
    good = [[0, 8], [4104, 4120], [13000, 19000], [N - 8, N]]

    def ema(segs=good, S=None, n=N, ptrs=(P, P), table=P, entries=100, decay=0.9999, recs=(P, P), seg_ptr=True):
        keep = np.array(segs, dtype=np.int64).reshape(-1, 2)
        return lib.svit_ema_step_guarded(*ptrs, n, keep.ctypes.data if seg_ptr else None, len(keep) if S is None else S,
                                         table, entries, decay, *recs, None)

    bad_arg = {
        "S = 0": dict(S=0),
        "S = 65": dict(segs=[[8 * i, 8 * i + 4] for i in range(65)]),
        "S < 0": dict(S=-1),
        "no table of ranges": dict(seg_ptr=False),
        "unsorted": dict(segs=[[4104, 4120], [0, 8]]),
        "overlapping": dict(segs=[[0, 16], [8, 24]]),
        "empty": dict(segs=[[0, 8], [16, 16]]),
        "reversed": dict(segs=[[24, 16]]),
        "negative": dict(segs=[[-8, 8]]),
        "end > n": dict(segs=[[0, 8], [N - 8, N + 4]]),
        "n = 0": dict(n=0),
        "entries < 0": dict(entries=-1),
        "entries > 2^20": dict(entries=2 ** 20 + 1),
        "NULL table with entries": dict(table=None, entries=1),
        "NULL ema": dict(ptrs=(None, P)),
        "NULL p": dict(ptrs=(P, None)),
        "NULL ema_rec": dict(recs=(None, P)),
        "NULL dev_rec": dict(recs=(P, None)),
    }
    for label, kw in bad_arg.items():
        assert ema(**kw) == -4, label
    for bad in (0.0, -0.0, 1.0, -0.5, 1.0000001, float("nan"), float("inf"), -float("inf")):
        assert ema(decay=bad) == -4, bad
        assert ema(decay=bad, table=None, entries=0) == -4, bad
    bad_align = {
        "a bound not a multiple of 4": dict(segs=[[0, 6]]),
        "a begin not a multiple of 4": dict(segs=[[2, 8]]),
        "a later bound": dict(segs=[[0, 8], [4105, 4121]]),
        "ema": dict(ptrs=(P + 4, P)),
        "p": dict(ptrs=(P, P + 8)),
        "ema_rec": dict(recs=(P + 4, P)),
        "dev_rec": dict(recs=(P, P + 4)),
    }
    for label, kw in bad_align.items():
        assert ema(**kw) == -3, label
    # the limits themselves pass the checks: with everything else in order the next thing would be the launch, so
    # they are shown through the one check that comes after them (a misaligned ema)
    for kw in (dict(entries=2 ** 20), dict(table=None, entries=0), dict(decay=float(np.float32(0.99999994))),
               dict(decay=1e-45), dict(segs=[[8 * i, 8 * i + 4] for i in range(64)]), dict(segs=[[0, N]])):
        assert ema(ptrs=(P + 4, P), **kw) == -3, kw


def test_refusals_by_message(lib):
    from svit_amd import ema, optim
    cfg, model = _cpu_model()
    classic = optim.FusedClipAdamW(model, lr=1e-3)
    with pytest.raises(TypeError, match="GuardedClipAdamW or one of its subclasses, got FusedClipAdamW"):
        ema.WeightEMA(model, classic)
    opt = optim.GuardedClipAdamW(model, lr=1e-3)
    for bad in (0.0, 1.0, -0.1, 1.5, float("nan")):
        with pytest.raises(ValueError, match=r"the EMA decay lies in \(0, 1\)"):
            ema.WeightEMA(model, opt, decay=bad)
    for bad in (0.0, 1.0, -0.1, 2, "0.999", True):
        cfg.SVIT.EMA_DECAY = bad
        with pytest.raises(ValueError, match=r"^SVIT.EMA_DECAY lies in \(0, 1\), got "):
            ema.build_ema(cfg, model, opt)
    assert opt.ema is None
    cfg.SVIT.EMA_DECAY = 0.999
    with pytest.raises(TypeError, match="got FusedClipAdamW"):
        ema.build_ema(cfg, model, classic)
    _, other = _cpu_model()
    with pytest.raises(ValueError, match="built over another model"):
        ema.WeightEMA(other, opt)
    theirs = ema.WeightEMA(model, optim.GuardedClipSGD(model, lr=0.1))
    with pytest.raises(ValueError, match="^attach_ema: the WeightEMA was built over another optimizer"):
        opt.attach_ema(theirs)
    assert opt.ema is None
    # a state written under another decay or warm-up
    mine = ema.WeightEMA(model, opt, decay=0.999)
    for kw in (dict(decay=0.9999), dict(decay=0.999, warmup=True)):
        with pytest.raises(ValueError, match="the EMA state was written with decay"):
            mine.load_state_dict(ema.WeightEMA(model, opt, **kw).state_dict())
    sd = mine.state_dict()
    del sd["model_state"]["cls_token"]
    with pytest.raises(KeyError, match="cls_token"):
        mine.load_state_dict(sd)


# ------------------------------------------------------------------------------------------------------- state ----
@pytest.mark.parametrize("cut", [0, 4])
def test_state_dict_has_the_models_names_and_shapes(lib, cut):
    from svit_amd import ema, optim
    cfg, model = _cpu_model()
    model.freeze_below(cut)
    opt = optim.GuardedClipSGD(model, lr=0.1, momentum=0.9)
    av = ema.WeightEMA(model, opt, decay=0.999, warmup=True)
    flat = model.flat
    if cut:
        assert av.segments is opt.segments and len(av.segments) > 1
    else:
        assert av.segments.tolist() == [[0, flat.total]] and av.segments.dtype == np.int64
    assert av.table.shape == (8990,) and av.table.dtype == torch.float32 and av.ema_rec.dtype == torch.int64
    assert av.buf.data_ptr() != flat.data.data_ptr() and torch.equal(av.buf, flat.data)
    sd = av.state_dict()
    assert list(sd) == ["decay", "warmup", "num_updates", "model_state"]
    assert (sd["decay"], sd["warmup"], sd["num_updates"]) == (0.999, True, 0)
    own = model.state_dict()
    assert list(sd["model_state"]) == list(own) and len(own) == 405
    for k, v in own.items():
        t = sd["model_state"][k]
        assert t.shape == v.shape and t.dtype == v.dtype, k
        assert torch.equal(t, v), k                      # frozen parameters included: the copy of the weights
    # the tensors are the average's, not the model's: moving the average shows in them alone
    av.buf.add_(1.0)
    sd = av.state_dict()
    assert all(torch.equal(sd["model_state"][k], v + 1.0) for k, v in own.items())
    # ... and they load into a model as they are
    _, twin = _cpu_model()
    twin.load_state_dict(sd["model_state"])
    assert all(torch.equal(a, b + 1.0) for a, b in zip(twin.state_dict().values(), own.values()))


def test_update_count_follows_the_optimizer_and_survives_an_sgd_resume(lib):
    """num_updates = the optimizer's applied steps + an offset only the host writes: zero when the average is created or
    reset whatever the optimizer has done before, continued across a load although SGD's own count restarts at 1"""
    from svit_amd import ema, optim
    _, model = _cpu_model()
    opt = optim.GuardedClipSGD(model, lr=0.1, momentum=0.9)
    opt.step_count = 7
    av = ema.WeightEMA(model, opt, decay=0.9, warmup=True)
    assert av.num_updates == 0 and int(av.ema_rec[0]) == -7 and int(av.ema_rec[1]) == 0
    assert av.stats() == {"num_updates": 0, "decay": float(E.warmup_closed_form(0.9, 1))}
    opt.step_count = 7 + 12                             # (what twelve applied steps leave in the record)
    assert av.stats() == {"num_updates": 12, "decay": float(E.warmup_closed_form(0.9, 12))}
    opt.step_count = 7 + 500
    assert av.stats() == {"num_updates": 500, "decay": float(np.float32(0.9))}
    opt.momentum_buffer.fill_(0.5)
    av.buf.mul_(3.0)
    state, opt_state = av.state_dict(), opt.state_dict()
    assert state["num_updates"] == 500
    # the resume: a fresh optimizer loads SGD's state (its count becomes 1), then the average
    _, model2 = _cpu_model()
    opt2 = optim.GuardedClipSGD(model2, lr=0.1, momentum=0.9)
    av2 = ema.WeightEMA(model2, opt2, decay=0.9, warmup=True)
    opt2.load_state_dict(opt_state)
    assert opt2.step_count == 1
    av2.load_state_dict(state)
    assert av2.num_updates == 500 and int(av2.ema_rec[0]) == 499 and torch.equal(av2.buf, av.buf)
    opt2.step_count = 2                                 # the next applied step is update 501
    assert av2.num_updates == 501
    av2.reset()
    assert av2.num_updates == 0 and int(av2.ema_rec[0]) == -2 and torch.equal(av2.buf, model2.flat.data)


# ---------------------------------------------------------------------------------------------------- dispatch ----
def test_construct_optimizer_and_build_ema_under_the_key(lib):
    from svit_amd import config, ema, optim
    cfg, model = _cpu_model()
    assert "EMA_DECAY" not in config.get_cfg().SVIT and "EMA_WARMUP" not in config.get_cfg().SVIT     # not keys of the default tree
    s = cfg.SOLVER
    s.OPTIMIZING_METHOD, s.BASE_LR, s.WEIGHT_DECAY, s.CLIP_GRAD_L2NORM = "adamw", 1e-3, 0.05, 1.0
    plain = optim.construct_optimizer(model, cfg)
    assert type(plain) is optim.FusedClipAdamW and ema.build_ema(cfg, model, plain) is None
    cfg.SVIT.EMA_DECAY = 0.999
    opt = optim.construct_optimizer(model, cfg)
    assert type(opt) is optim.GuardedClipAdamW and opt.ema is None and opt.clip == 1.0 and opt.clip_value is None
    av = ema.build_ema(cfg, model, opt)
    assert type(av) is ema.WeightEMA and opt.ema is av and av.optimizer is opt
    assert (av.decay, av.warmup, av.table, av.table_host) == (0.999, False, None, None)
    cfg.SVIT.EMA_WARMUP = True
    av = ema.build_ema(cfg, model, opt)
    assert opt.ema is av and av.warmup and av.table.shape == (8990,)
    opt.attach_ema(None)
    assert opt.ema is None
    for method, cls in (("sgd", optim.GuardedClipSGD), ("adam", optim.GuardedClipAdam)):
        s.OPTIMIZING_METHOD = method
        s.MOMENTUM, s.DAMPENING, s.NESTEROV = 0.9, 0.0, True
        o = optim.construct_optimizer(model, cfg)
        assert type(o) is cls and ema.build_ema(cfg, model, o) is o.ema and o.ema is not None
    # without the key: the state_dict of today
    del cfg.SVIT["EMA_DECAY"]
    s.OPTIMIZING_METHOD = "adamw"
    assert type(optim.construct_optimizer(model, cfg)) is optim.FusedClipAdamW
    assert list(plain.state_dict()) == ["state", "param_groups"]
