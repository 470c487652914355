"""SGD and Adam on the guarded tail, host side: the NumPy restatements against torch's own solvers, the checkpoint
format, the refusals, the lr policies against values recorded from the reference, construct_optimizer's dispatch.
No GPU needed."""
import json
import os
import types

import numpy as np
import pytest
import torch

from tests import layer_decay_cases as L


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
    return cfg, model


# ------------------------------------------------------------------------- restatements against torch's solvers ----
N_EL, STEPS = 65536, 5
CASES = {
    "sgd nesterov wd 1e-4": dict(kind="sgd", lr=0.1, wd=1e-4, momentum=0.9, dampening=0.0, nesterov=True),
    "sgd dampening 0.1": dict(kind="sgd", lr=0.1, wd=0.0, momentum=0.9, dampening=0.1, nesterov=False),
    "sgd momentum 0": dict(kind="sgd", lr=0.1, wd=0.0, momentum=0.0, dampening=0.0, nesterov=False),
    "adam wd 1e-4": dict(kind="adam", lr=2e-4, wd=1e-4),
    "adam wd 0": dict(kind="adam", lr=2e-4, wd=0.0),
}


@pytest.fixture(scope="module")
def inputs():
    rng = np.random.default_rng(20)
    w = (rng.standard_normal(N_EL) * 0.02).astype(np.float32)
    return w, [(rng.standard_normal(N_EL) * 0.01).astype(np.float32) for _ in range(STEPS)]


def _torch_run(case, w, grads, dtype):
    p = torch.nn.Parameter(torch.from_numpy(w.copy()).to(dtype))
    if case["kind"] == "sgd":
        opt = torch.optim.SGD([p], lr=case["lr"], momentum=case["momentum"], dampening=case["dampening"],
                              nesterov=case["nesterov"], weight_decay=case["wd"])
    else:
        opt = torch.optim.Adam([p], lr=case["lr"], betas=(0.9, 0.999), eps=1e-8, weight_decay=case["wd"])
    for g in grads:
        p.grad = torch.from_numpy(g.copy()).to(dtype)
        opt.step()
    return p.detach().double().numpy()


@pytest.mark.parametrize("name", list(CASES))
def test_restatement_against_torch_in_float64(lib, inputs, name):
    """Five steps on 65 536 elements; the yardstick is torch's own fp32 solver against its float64 one.
    Bar: max |ours - f64| <= 2 x max |torch fp32 - f64| (a different but equally valid rounding order may cost that).
    Measured, ours / torch fp32: sgd nesterov wd 1e-4 1.04; sgd dampening 0.1 1.01; sgd momentum 0 1.00;
    adam wd 1e-4 0.90; adam wd 0 1.00 (errors 9.5e-9 to 1.4e-8 on both sides; the run prints its own figures)."""
    from svit_amd import ops, optim
    case = CASES[name]
    w, grads = inputs
    p = w.copy()
    if case["kind"] == "sgd":
        buf = None
        for i, g in enumerate(grads):
            p, buf = optim.sgd_step_host(p, g, buf, 1.0, case["lr"], case["wd"], case["momentum"], case["dampening"],
                                         case["nesterov"], first=(i == 0))
        assert (buf is None) == (case["momentum"] == 0)
    else:
        table = ops.adamw_bias_table(0.9, 0.999)
        m, v = np.zeros_like(p), np.zeros_like(p)
        for i, g in enumerate(grads):
            p, m, v = optim.adam_step_host(p, g, m, v, 1.0, table[i, 0], table[i, 1], case["lr"], case["wd"])
    assert p.dtype == np.float32
    exact = _torch_run(case, w, grads, torch.float64)
    ours = float(np.abs(p.astype(np.float64) - exact).max())
    theirs = float(np.abs(_torch_run(case, w, grads, torch.float32) - exact).max())
    print("%s: max |ours - f64| %.3e, max |torch fp32 - f64| %.3e, ratio %.2f" % (name, ours, theirs, ours / theirs))
    assert theirs > 0 and float(np.abs(exact - w).max()) > 1e-4          # the steps moved the weights
    assert ours <= 2.0 * theirs, (name, ours, theirs)


def test_restatement_first_step_and_clamp():
    """the first applied step copies gi into the buffer whatever the dampening; clip by value clamps g * coef"""
    from svit_amd import optim
    p = np.array([1.0, -2.0, 3.0, 0.5], dtype=np.float32)
    g = np.array([0.5, -0.25, 4.0, -4.0], dtype=np.float32)
    stale = np.full(4, 7.0, dtype=np.float32)
    p1, b1 = optim.sgd_step_host(p, g, stale, 0.5, 0.1, 0.0, momentum=0.9, dampening=0.3, first=True)
    assert np.array_equal(b1, g * np.float32(0.5)) and np.array_equal(p1, p - b1 * np.float32(0.1))
    p2, b2 = optim.sgd_step_host(p, g, stale, 0.5, 0.1, 0.0, momentum=0.9, dampening=0.3, first=False)
    assert np.array_equal(b2, stale * np.float32(0.9) + (g * np.float32(0.5)) * (np.float32(1) - np.float32(0.3)))
    p3, _ = optim.sgd_step_host(p, g, None, 1.0, 1.0, 0.0, clip_value=1.0)
    assert np.array_equal(p3, p - np.array([0.5, -0.25, 1.0, -1.0], dtype=np.float32))
    # per-element rates: an element with wd == 0 takes no decay term
    p4, _ = optim.sgd_step_host(p, g, None, 1.0, np.array([1, 1, 2, 2], dtype=np.float32),
                                np.array([0.5, 0, 0.5, 0], dtype=np.float32))
    assert np.array_equal(p4, p - (g + p * np.array([0.5, 0, 0.5, 0], dtype=np.float32))
                          * np.array([1, 1, 2, 2], dtype=np.float32))


# --------------------------------------------------------------------------------------------- checkpoint format ----
def _torch_twin(model, kind, scale_of, lr, wd, momentum):
    """torch.optim.SGD / Adam over CPU parameters grouped as the reference groups the trainable ones (two weight-decay
    groups), each split by distinct scale in order of first appearance -> (optimizer, names per group)"""
    skip = set(model.no_weight_decay())
    groups = ({}, {})
    for name, p in model.named_parameters():
        if not p.requires_grad:
            continue
        which = 1 if (name in skip or p.dim() == 1 or name.endswith(".bias")) else 0
        groups[which].setdefault(scale_of(name), []).append((name, tuple(p.shape)))
    out, names = [], []
    for which, split in enumerate(groups):
        for c, members in split.items():
            out.append({"params": [torch.nn.Parameter(torch.zeros(s)) for _, s in members],
                        "weight_decay": wd if which == 0 else 0.0,
                        "lr": lr if c is None else float(np.float32(lr) * np.float32(c))})
            names.append([n for n, _ in members])
    if kind == "adam":
        return torch.optim.Adam(out, lr=lr, betas=(0.9, 0.999), weight_decay=wd), names
    return torch.optim.SGD(out, lr=lr, momentum=momentum, dampening=0.0, nesterov=momentum > 0, weight_decay=wd), names


@pytest.mark.parametrize("decayed", [False, True])
@pytest.mark.parametrize("cut", [0, 4])
@pytest.mark.parametrize("kind", ["sgd", "sgd momentum 0", "adam"])
def test_state_dict_against_the_torch_solver(lib, kind, cut, decayed):
    from svit_amd import optim
    cfg, model = _cpu_model()
    momentum = 0.0 if kind == "sgd momentum 0" else 0.9
    method = kind.split()[0]
    s = cfg.SOLVER
    s.OPTIMIZING_METHOD, s.BASE_LR, s.WEIGHT_DECAY, s.MOMENTUM, s.DAMPENING, s.NESTEROV = (method, 0.1, 1e-4, momentum, 0.0,
                                                                                            momentum > 0)
    if decayed:
        s.LAYER_DECAY = L.DECAY
        cfg.SVIT.LR_MULT = L.LR_MULT
    model.freeze_below(cut)
    opt = optim.construct_optimizer(model, cfg)
    assert type(opt) is (optim.GuardedClipAdam if method == "adam" else optim.GuardedClipSGD)
    assert (opt.lr_segments is not None) == decayed and len(opt.param_groups) == 2
    scale_of = (lambda n: L.scale(n, L.DECAY, L.LR_MULT)) if decayed else (lambda n: None)
    ref, ref_names = _torch_twin(model, method, scale_of, 0.1, 1e-4, momentum)
    n_train = sum(1 for p in model.parameters() if p.requires_grad)
    assert (n_train == 405) == (cut == 0)
    # before the first step: no state, as torch's
    assert opt.state_dict()["state"] == {} == ref.state_dict()["state"]
    # after two steps of the torch twin (zero gradients: the state's structure is what is compared)
    for _ in range(2):
        for g in ref.param_groups:
            for p in g["params"]:
                p.grad = torch.zeros_like(p)
        ref.step()
    opt.step_count = 2
    sd, rd = opt.state_dict(), ref.state_dict()
    order = sum(opt._order(), [])
    assert len(order) == n_train
    assert len(sd["param_groups"]) == len(rd["param_groups"]) and (len(sd["param_groups"]) > 2) == decayed
    extra = {"layer_decay"} if decayed else set()
    for ours, theirs, members in zip(sd["param_groups"], rd["param_groups"], ref_names):
        assert set(ours) == set(theirs) | extra
        assert [order[j] for j in ours["params"]] == members
        if not decayed:
            assert ours["params"] == theirs["params"]
        for key in theirs:
            if key != "params":
                assert ours[key] == theirs[key] and type(ours[key]) is type(theirs[key]), key
    # the state: same indices, same keys, the parameter's shape; empty for momentum 0
    assert sorted(sd["state"]) == sorted(rd["state"]) == ([] if momentum == 0 and method == "sgd" else list(range(n_train)))
    shapes = {n: tuple(p.shape) for n, p in model.named_parameters()}
    by_name = {n: rd["state"][j] for g, members in zip(rd["param_groups"], ref_names)
               for j, n in zip(g["params"], members) if j in rd["state"]}
    for j, ent in sd["state"].items():
        assert list(ent) == list(by_name[order[j]])
        assert list(ent) == (["step", "exp_avg", "exp_avg_sq"] if method == "adam" else ["momentum_buffer"])
        for key, t in ent.items():
            assert tuple(t.shape) == (() if key == "step" else shapes[order[j]])
        if method == "adam":
            assert float(ent["step"]) == 2.0 == float(by_name[order[j]]["step"])
    # a real torch optimizer takes our dict
    fresh, _ = _torch_twin(model, method, scale_of, 0.05, 1e-4, momentum)
    fresh.load_state_dict(sd)
    assert [g["lr"] for g in fresh.param_groups] == [g["lr"] for g in sd["param_groups"]]
    assert len(fresh.state_dict()["state"]) == len(sd["state"])
    # and either group form loads into either optimizer of the same solver
    other_cfg, _ = _cpu_model()
    plain = type(opt)(model, lr=0.05, **({} if method == "adam" else dict(momentum=momentum)))
    assert plain.lr_segments is None
    plain.load_state_dict(sd)
    assert all(np.float32(g["lr"]) == np.float32(0.1) for g in plain.param_groups)
    if method == "adam":
        assert plain.step_count == 2
    else:
        assert plain.step_count == (1 if momentum else 0)       # loaded buffers: the next step is not "first"
    plain.param_groups[0]["lr"] = plain.param_groups[1]["lr"] = 0.05
    two = plain.state_dict()
    assert len(two["param_groups"]) == 2 and all("layer_decay" not in g for g in two["param_groups"])
    opt.load_state_dict(two)
    assert [g["lr"] for g in opt.param_groups] == [0.05, 0.05]


def test_loaded_buffers_keep_a_later_step_count(lib):
    from svit_amd import optim
    _, model = _cpu_model()
    a = optim.GuardedClipSGD(model, lr=0.1, momentum=0.9)
    a.step_count = 7
    a.momentum_buffer.fill_(0.25)
    b = optim.GuardedClipSGD(model, lr=0.1, momentum=0.9)
    assert b.step_count == 0
    b.load_state_dict(a.state_dict())
    assert b.step_count == 1
    for name, (off, numel, _) in model.flat.slots.items():      # every slot arrived (the alignment padding is not state)
        assert bool((b.momentum_buffer[off:off + numel] == 0.25).all()), name
    b.step_count = 9
    b.load_state_dict(a.state_dict())
    assert b.step_count == 9
    # a state without buffers (torch's momentum_buffer of None, e.g. saved before the first step): the buffers are
    # zeroed and the counter returns to 0, so the next step copies its gradient into them as torch's would
    fresh = optim.GuardedClipSGD(model, lr=0.1, momentum=0.9, dampening=0.1)
    empty = fresh.state_dict()
    assert empty["state"] == {}
    b.load_state_dict(empty)
    assert b.step_count == 0 and int(torch.count_nonzero(b.momentum_buffer)) == 0
    # Adam's counter is the checkpoint's, as before
    adam = optim.GuardedClipAdam(model, lr=1e-3)
    adam.step_count = 5
    adam.load_state_dict(optim.GuardedClipAdam(model, lr=1e-3).state_dict())
    assert adam.step_count == 0


# ----------------------------------------------------------------------------------------------------- refusals ----
def test_refusals_by_message(lib):
    from svit_amd import optim
    cfg, model = _cpu_model()
    s = cfg.SOLVER
    s.OPTIMIZING_METHOD, s.MOMENTUM, s.DAMPENING, s.NESTEROV = "sgd", 0.0, 0.0, True
    with pytest.raises(ValueError, match="^Nesterov momentum requires a momentum and zero dampening$"):
        optim.construct_optimizer(model, cfg)
    s.MOMENTUM, s.DAMPENING = 0.9, 0.1
    with pytest.raises(ValueError, match="^Nesterov momentum requires a momentum and zero dampening$"):
        optim.construct_optimizer(model, cfg)
    with pytest.raises(ValueError, match="^Nesterov momentum requires a momentum and zero dampening$"):     # torch's own words
        torch.optim.SGD([torch.nn.Parameter(torch.zeros(1))], lr=0.1, momentum=0.9, dampening=0.1, nesterov=True)
    with pytest.raises(ValueError, match="Invalid momentum value: -0.5"):
        optim.GuardedClipSGD(model, lr=0.1, momentum=-0.5)
    s.DAMPENING = 0.0
    for method in ("sgd", "adam", "adamw"):
        s.OPTIMIZING_METHOD, s.ZERO_WD_1D_PARAM = method, False
        with pytest.raises(NotImplementedError, match="ZERO_WD_1D_PARAM") as e:
            optim.construct_optimizer(model, cfg)
        assert "adamw" not in str(e.value) and "ssv2.yaml" not in str(e.value)     # the layout is all it is about
        s.ZERO_WD_1D_PARAM = True
    s.OPTIMIZING_METHOD = "lars"
    with pytest.raises(NotImplementedError, match="^Does not support lars optimizer$"):
        optim.construct_optimizer(model, cfg)
    s.LR_POLICY = "exp"
    with pytest.raises(NotImplementedError, match="steps_with_relative_lrs.*'exp'"):
        optim.get_lr_at_epoch(cfg, 1.0)
    # a checkpoint of another solver
    adam = optim.GuardedClipAdam(model, lr=1e-3)
    adam.step_count = 1
    sgd = optim.GuardedClipSGD(model, lr=0.1, momentum=0.9)
    with pytest.raises(ValueError, match="no momentum_buffer: it was written by another solver"):
        sgd.load_state_dict(adam.state_dict())
    sgd.step_count = 1
    with pytest.raises(ValueError, match="no exp_avg: it was written by another solver"):
        adam.load_state_dict(sgd.state_dict())
    # the captured steps take the new classes by isinstance
    assert issubclass(optim.GuardedClipSGD, optim.GuardedClipAdamW) and issubclass(optim.GuardedClipAdam, optim.GuardedClipAdamW)
    assert not issubclass(optim.GuardedClipSGD, optim.GuardedClipAdam) and sgd.betas is None and sgd.eps is None


def test_entry_points_check_their_arguments_without_a_gpu(lib):
    """refused before any HIP call: stream = None and made-up device addresses that are never followed"""
    P = 4096
    N, ND = 20000, 12296
    good = [[0, 8], [4104, 4120], [ND - 8, ND], [ND, ND + 8], [13000, 19000], [N - 8, N]]

    def sgd(segs=good, scales=None, S=None, n=N, nd=ND, ptrs=(P, P, P), momentum=0.9, dampening=0.0, nesterov=0, seg_ptr=True):
        keep = np.array(segs, dtype=np.int64).reshape(-1, 2)
        sc = None if scales is None else np.array(scales, dtype=np.float32)
        return lib.svit_sgd_step_guarded(*ptrs, n, nd, keep.ctypes.data if seg_ptr else None,
                                         None if sc is None else sc.ctypes.data, len(keep) if S is None else S, P, P,
                                         momentum, dampening, nesterov, None)

    def adam(segs=good, scales=None, S=None, n=N, nd=ND, ptrs=(P, P, P, P), seg_ptr=True):
        keep = np.array(segs, dtype=np.int64).reshape(-1, 2)
        sc = None if scales is None else np.array(scales, dtype=np.float32)
        return lib.svit_adam_step_guarded(*ptrs, n, nd, keep.ctypes.data if seg_ptr else None,
                                          None if sc is None else sc.ctypes.data, len(keep) if S is None else S, P, P,
                                          0.9, 0.999, 1e-8, None)

    bad_arg = {
        "S = 0": dict(S=0),
        "S = 65": dict(segs=[[8 * i, 8 * i + 4] for i in range(65)]),
        "S < 0": dict(S=-1),
        "no table": dict(seg_ptr=False),
        "unsorted": dict(segs=[[4104, 4120], [0, 8]]),
        "overlapping": dict(segs=[[0, 16], [8, 24]]),
        "empty": dict(segs=[[0, 8], [16, 16]]),
        "reversed": dict(segs=[[24, 16]]),
        "negative": dict(segs=[[-8, 8]]),
        "end > n": dict(segs=[[0, 8], [N - 8, N + 4]]),
        "straddles n_decay": dict(segs=[[ND - 8, ND + 8]]),
        "n_decay > n": dict(nd=N + 1),
        "n_decay < 0": dict(nd=-1),
    }
    for fn, n_ptrs in ((sgd, 3), (adam, 4)):
        for label, kw in bad_arg.items():
            assert fn(**kw) == -4, (fn.__name__, label)
        for bad in (0.0, -0.0, -1.0, float("nan"), float("inf"), -float("inf")):
            for at in (0, 3, 5):
                sc = [1.0, 0.5, 2.0, 0.75 ** 17, 10.0, 1.0]
                sc[at] = bad
                assert fn(scales=sc) == -4, (fn.__name__, bad, at)
        for segs in ([[0, 6]], [[2, 8]], [[0, 8], [4105, 4121]]):
            assert fn(segs=segs) == -3, (fn.__name__, segs)
        for i in range(n_ptrs):
            ptrs = [P] * n_ptrs
            ptrs[i] = None
            assert fn(ptrs=ptrs) == -4, (fn.__name__, i)
            ptrs[i] = P + 4
            assert fn(ptrs=ptrs) == -3, (fn.__name__, i)
    # SGD's own: nesterov needs momentum > 0 and dampening == 0; a momentum needs its buffer, none does not
    assert sgd(nesterov=1, momentum=0.0) == -4 and sgd(nesterov=1, momentum=-0.5) == -4
    assert sgd(nesterov=1, momentum=0.9, dampening=0.1) == -4
    assert sgd(momentum=0.9, ptrs=(P, P, None)) == -4
    # (with momentum 0 and no buffer the arguments are fine: what is refused next is a misaligned gradient)
    assert sgd(momentum=0.0, ptrs=(P, P + 4, None)) == -3


# ---------------------------------------------------------------------------------------------------- lr policy ----
def test_lr_policies_against_the_recorded_reference_values(golden_dir):
    """tests/golden/lr_policy.json (tools/gen_lr_policy_golden.py): to the last bit of a Python double"""
    from svit_amd import optim
    rec = json.load(open(os.path.join(golden_dir, "lr_policy.json")))
    assert sorted(rec) == ["cosine_warmup", "steps", "steps_warmup"]
    for name, r in rec.items():
        cfg = types.SimpleNamespace(SOLVER=types.SimpleNamespace(**r["solver"]))
        assert len(r["epochs"]) == len(r["lr_hex"]) >= 20
        for ep, want in zip(r["epochs"], r["lr_hex"]):
            got = optim.get_lr_at_epoch(cfg, ep)["lr"]
            assert float(got).hex() == want, (name, ep, got, float.fromhex(want))
    # the step policy steps: four plateaus, and the warm-up ramps to the plateau that holds its last epoch
    lrs = [float.fromhex(h) for h in rec["steps"]["lr_hex"]]
    assert len(set(lrs)) == 4 and max(lrs) == 0.1 and lrs == sorted(lrs, reverse=True)
    w = rec["steps_warmup"]
    ramp = [float.fromhex(h) for e, h in zip(w["epochs"], w["lr_hex"]) if e < 3.5]
    assert ramp == sorted(ramp) and ramp[0] == 0.0003 and ramp[-1] < 0.3 * 0.03


# ----------------------------------------------------------------------------------------------------- dispatch ----
def test_construct_optimizer_dispatch(lib):
    from svit_amd import config, optim
    cfg, model = _cpu_model()
    s = cfg.SOLVER
    s.BASE_LR, s.WEIGHT_DECAY, s.CLIP_GRAD_L2NORM = 0.05, 5e-4, 1.0
    cfg.SVIT.MAX_CONSECUTIVE_SKIPS = 3
    # sgd with the default tree's momentum and nesterov
    d = config.get_cfg().SOLVER
    assert (d.OPTIMIZING_METHOD, d.MOMENTUM, d.DAMPENING, d.NESTEROV) == ("sgd", 0.9, 0.0, True)
    s.OPTIMIZING_METHOD, s.MOMENTUM, s.DAMPENING, s.NESTEROV = "sgd", d.MOMENTUM, d.DAMPENING, d.NESTEROV
    for guarded in (False, True):                       # returned whether or not SVIT.GUARDED_STEP is set
        if guarded:
            cfg.SVIT.GUARDED_STEP = True
        o = optim.construct_optimizer(model, cfg)
        assert type(o) is optim.GuardedClipSGD
        assert (o.momentum, o.dampening, o.nesterov, o.clip, o.clip_value, o.max_consecutive_skips) == (0.9, 0.0, True, 1.0,
                                                                                                      None, 3)
        assert [(g["lr"], g["weight_decay"]) for g in o.param_groups] == [(0.05, 5e-4), (0.05, 0.0)]
        assert o.STATE == ("momentum_buffer",) and o.momentum_buffer.shape == (model.flat.total,)
        assert not hasattr(o, "exp_avg") and o.bias_table.shape == (0, 2)
        segs, scales = o._ranges()
        nd, n = model.flat.n_decay, model.flat.total
        assert segs.tolist() == [[0, nd], [nd, n]] and scales is None and segs.dtype == np.int64
        s.OPTIMIZING_METHOD = "adam"
        o = optim.construct_optimizer(model, cfg)
        assert type(o) is optim.GuardedClipAdam and o.betas == (0.9, 0.999) and o.eps == 1e-8
        assert o.exp_avg.shape == o.exp_avg_sq.shape == (n,) and o.bias_table.shape == (17321, 2)
        s.OPTIMIZING_METHOD = "sgd"
    s.MOMENTUM, s.NESTEROV, s.CLIP_GRAD_VAL = 0.0, False, 0.5
    o = optim.construct_optimizer(model, cfg)
    assert o.STATE == () and o.momentum_buffer is None and o.clip_value == 0.5 and o.state_dict()["state"] == {}
    # a frozen cut: the table is the trainable segments; with LAYER_DECAY the scaled ranges
    model.freeze_below(4)
    o = optim.construct_optimizer(model, cfg)
    assert o.cut == 4 and o._ranges()[0] is o.segments and o._ranges()[1] is None
    s.LAYER_DECAY = L.DECAY
    o = optim.construct_optimizer(model, cfg)
    assert o._ranges()[0] is o.lr_segments and o._ranges()[1] is o.lr_scales and len(o.lr_scales) > 2
    model.freeze_below(0)
    del s["LAYER_DECAY"]
    # adamw: today's branch
    s.OPTIMIZING_METHOD, s.CLIP_GRAD_VAL = "adamw", None
    assert type(optim.construct_optimizer(model, cfg)) is optim.GuardedClipAdamW
    del cfg.SVIT["GUARDED_STEP"]
    assert type(optim.construct_optimizer(model, cfg)) is optim.FusedClipAdamW
    s.CLIP_GRAD_VAL = 0.5
    assert type(optim.construct_optimizer(model, cfg)) is optim.GuardedClipAdamW
