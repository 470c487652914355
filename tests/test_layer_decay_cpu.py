"""Layer-wise lr decay, host side (svit_amd/lrscale.py, the optimizers' range tables and state_dict, the argument checks
of svit_adamw_step_guarded_lr).  No GPU needed."""
import json
import os

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


def _layout(golden_dir, skip):
    from svit_amd import arch
    from svit_amd.engine import FlatParams
    from svit_amd.model import _weight_decayed
    layout = json.load(open(os.path.join(golden_dir, "layout.json")))
    shapes = {n: tuple(layout["shapes"][n]) for n in layout["named_parameters"]}
    assert len(shapes) == 405
    order, slots, n_decay, _, total, depth = FlatParams.layout(
        shapes, lambda n, s: _weight_decayed(n, s, skip), arch.readiness_rank)
    assert depth == L.DEPTH
    return list(shapes), slots, n_decay, total


@pytest.fixture(scope="module", params=["no_weight_decay names", "nothing skipped"])
def real_layout(request, golden_dir):
    """the flat placement of the reference's 405 tensors, with and without the no_weight_decay names"""
    skip = ("cls_token", "object_queries", "pos_embed_temporal") if request.param == "no_weight_decay names" else ()
    return _layout(golden_dir, skip)


def _cfg(decay=None, mult=None):
    from svit_amd import config
    cfg = config.ssv2_cfg()
    assert cfg.MVIT.DEPTH == L.DEPTH
    assert not hasattr(cfg.SOLVER, "LAYER_DECAY") and not hasattr(cfg.SVIT, "LR_MULT")      # not keys of the default tree
    if decay is not None:
        cfg.SOLVER.LAYER_DECAY = decay
    if mult is not None:
        cfg.SVIT.LR_MULT = mult
    return cfg


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


# ------------------------------------------------------------------------------------------------- the rule ----
def test_layer_ids_and_scales_of_named_parameters():
    from svit_amd import lrscale, optim
    fn = optim.lr_scale_from_cfg(_cfg(decay=L.DECAY))
    for name, lid in L.EXAMPLES.items():
        assert lrscale.layer_id(name, L.DEPTH) == lid == L.layer_id(name), name
        assert fn(name) == L.DECAY ** (L.DEPTH + 1 - lid), name
    assert fn("object_queries") == 1.0 and fn("head.contact_mlp.bias") == 1.0 and fn("norm.weight") == 1.0
    assert fn("cls_token") == 0.75 ** 17 and fn("blocks.0.norm1.weight") == 0.75 ** 16 and fn("blocks.15.mlp.fc2.bias") == 0.75
    # multipliers: the first matching prefix, on top of the layer's scale
    fn = optim.lr_scale_from_cfg(_cfg(decay=L.DECAY, mult=[["object_queries", 4.0], ["head.", 2.0], ["head.contact", 8.0],
                                                           ["blocks.3.", 0.5]]))
    assert fn("object_queries") == 4.0 and fn("head.contact_mlp.bias") == 2.0 and fn("norm.bias") == 1.0
    assert fn("blocks.3.attn.qkv.weight") == 0.75 ** 13 * 0.5 and fn("blocks.30.x") != fn("blocks.3.x")
    # multipliers alone
    fn = optim.lr_scale_from_cfg(_cfg(mult=[["head.", 2.0]]))
    assert fn("head.projection.weight") == 2.0 and fn("cls_token") == 1.0


def test_absent_keys_give_no_table():
    from svit_amd import optim
    assert optim.lr_scale_from_cfg(_cfg()) is None
    assert optim.lr_scale_from_cfg(_cfg(decay=1.0)) is None
    assert optim.lr_scale_from_cfg(_cfg(decay=1.0, mult=[])) is None
    _, model = _cpu_model()
    for kw in ({}, {"lr_scale": None}, {"lr_scale": lambda name: 1.0}):
        opt = optim.FusedClipAdamW(model, lr=1e-3, **kw)
        assert opt.lr_segments is None and opt.lr_scales is None


@pytest.mark.parametrize("bad", [0, 0.0, -0.5, 1.5, float("nan"), float("inf")])
def test_layer_decay_outside_0_1_is_refused(bad):
    from svit_amd import optim
    with pytest.raises(ValueError, match="LAYER_DECAY"):
        optim.lr_scale_from_cfg(_cfg(decay=bad))
    _, model = _cpu_model()
    cfg = _cfg(decay=bad)
    with pytest.raises(ValueError, match="LAYER_DECAY"):
        optim.construct_optimizer(model, cfg)


@pytest.mark.parametrize("bad", [0.0, -2.0, float("nan"), float("inf")])
def test_a_factor_that_is_not_positive_and_finite_is_refused(bad):
    from svit_amd import optim
    with pytest.raises(ValueError, match="LR_MULT"):
        optim.lr_scale_from_cfg(_cfg(mult=[["head.", 2.0], ["norm.", bad]]))
    _, model = _cpu_model()
    with pytest.raises(ValueError, match="finite and > 0"):
        optim.FusedClipAdamW(model, lr=1e-3, lr_scale=lambda name: bad if name == "norm.weight" else 1.0)


# ------------------------------------------------------------------------------------------------ the table ----
@pytest.mark.parametrize("mult", [(), L.LR_MULT], ids=["decay", "decay+mult"])
@pytest.mark.parametrize("cut", [0, 4, 17])
def test_range_table_on_the_real_layout(real_layout, cut, mult):
    from svit_amd import freeze, lrscale, optim
    names, slots, n_decay, total = real_layout
    fn = optim.lr_scale_from_cfg(_cfg(decay=L.DECAY, mult=list(mult)))
    scales = lrscale.name_scales(names, fn)
    assert all(scales[n] == L.scale(n, L.DECAY, mult) and scales[n].dtype == np.float32 for n in names)
    trainable = freeze.trainable_names(names, L.DEPTH, cut)
    tsegs = freeze.segments(slots, n_decay, trainable) if cut else None
    tab = lrscale.table(slots, n_decay, scales, tsegs)
    if cut == 17 and not mult:
        assert tab is None              # final norm and head alone: every trainable scale is 1.0
        return
    segs, sc = tab
    L.check_table(segs, sc, L.element_scales(slots, trainable, total, L.DECAY, mult), n_decay)
    if cut == 0 and not mult:
        assert len(segs) == 38          # 18 layer ids x 2 weight-decay groups + readiness order's two extra pieces
    if cut:                             # the intersection: nothing outside the trainable segments
        inside = np.zeros(total, dtype=bool)
        for a, b in tsegs:
            inside[a:b] = True
        assert all(inside[a:b].all() for a, b in segs) and sum(b - a for a, b in segs) == int(inside.sum())


def test_tables_merge_and_split():
    from svit_amd import lrscale
    f = np.float32
    slots = {"a": (0, 5, (5,)), "b": (8, 8, (8,)), "c": (16, 3, (3,)), "d": (24, 8, (8,))}
    segs, sc = lrscale.table(slots, 16, {"a": f(.5), "b": f(.5), "c": f(.5), "d": f(2)})
    assert segs.tolist() == [[0, 16], [16, 24], [24, 32]] and sc.tolist() == [.5, .5, 2.0]     # cut at n_decay
    segs, sc = lrscale.table(slots, 32, {"a": f(.5), "b": f(1), "c": f(1), "d": f(.5)})
    assert segs.tolist() == [[0, 8], [8, 24], [24, 32]] and sc.tolist() == [.5, 1.0, .5]
    segs, sc = lrscale.table(slots, 32, {"a": f(.5), "b": f(1), "c": f(1), "d": f(.5)}, trainable=[(8, 20), (24, 32)])
    assert segs.tolist() == [[8, 20], [24, 32]] and sc.tolist() == [1.0, .5]
    assert lrscale.table(slots, 32, {"a": f(.5), "b": f(1), "c": f(1), "d": f(.5)}, trainable=[(8, 24)]) is None
    assert lrscale.table(slots, 16, {n: f(1) for n in slots}) is None


def test_more_than_64_ranges_are_refused_with_the_count(real_layout):
    from svit_amd import lrscale
    names, slots, n_decay, total = real_layout
    by_offset = sorted(names, key=lambda n: slots[n][0])
    per_tensor = {n: 1.0 + i / 1024.0 for i, n in enumerate(by_offset)}         # a multiplier per tensor
    with pytest.raises(NotImplementedError, match=r"\b405 ranges.*\b64\b"):
        lrscale.table(slots, n_decay, lrscale.name_scales(names, per_tensor.__getitem__))
    _, model = _cpu_model()
    from svit_amd import optim
    with pytest.raises(NotImplementedError, match=r"\b405 ranges.*\b64\b"):
        optim.GuardedClipAdamW(model, lr=1e-3, lr_scale=per_tensor.__getitem__)
    # 64 still fit: the first 62 tensors of the buffer on their own, the rest together on either side of n_decay
    few = {n: (1.0 + i / 1024.0 if i < 62 else 3.0) for i, n in enumerate(by_offset)}
    segs, _ = lrscale.table(slots, n_decay, lrscale.name_scales(names, few.__getitem__))
    assert len(segs) == 64


# ------------------------------------------------------------------------------------------- optimizers -------
def _torch_adamw(model, scale_of, lr, wd):
    """torch.optim.AdamW over CPU parameters grouped as the issue says: the reference's two weight-decay groups of the
    trainable parameters, each split by distinct scale in order of first appearance -> (optimizer, names per group)"""
    skip = set(model.no_weight_decay())
    groups = ({}, {})
    for name, p in model.named_parameters():
        if not p.requires_grad:
            continue
        which = 1 if (name in skip or p.dim() == 1 or name.endswith(".bias")) else 0
        groups[which].setdefault(scale_of(name), []).append(name)
    out, names = [], []
    for which, split in enumerate(groups):
        for c, members in split.items():
            out.append({"params": [torch.nn.Parameter(torch.empty(0)) for _ in members],
                        "weight_decay": wd if which == 0 else 0.0, "lr": float(np.float32(lr) * c)})
            names.append(members)
    return torch.optim.AdamW(out, lr=lr), names


@pytest.mark.parametrize("cut", [0, 4])
@pytest.mark.parametrize("kind", ["classic", "guarded"])
def test_state_dict_groups_against_torch_adamw(lib, kind, cut):
    from svit_amd import optim
    cfg, model = _cpu_model()
    cfg.SOLVER.LAYER_DECAY = L.DECAY
    cfg.SVIT.LR_MULT = L.LR_MULT
    cfg.SOLVER.BASE_LR, cfg.SOLVER.WEIGHT_DECAY = 1e-3, 0.05
    if kind == "guarded":
        cfg.SVIT.GUARDED_STEP = True
    model.freeze_below(cut)
    opt = optim.construct_optimizer(model, cfg)
    assert type(opt) is (optim.GuardedClipAdamW if kind == "guarded" else optim.FusedClipAdamW)
    assert len(opt.param_groups) == 2 and opt.lr_segments is not None and len(opt.lr_segments) == len(opt.lr_scales)
    opt.step_count = 2
    sd = opt.state_dict()
    ref, ref_names = _torch_adamw(model, lambda n: L.scale(n, L.DECAY, L.LR_MULT), 1e-3, 0.05)
    ref = ref.state_dict()
    dec, rest = opt._order()
    order = dec + rest
    assert len(sd["param_groups"]) == len(ref["param_groups"]) > 2
    n_train = sum(1 for p in model.parameters() if p.requires_grad)
    assert sorted(sd["state"]) == list(range(n_train))
    assert sorted(j for g in sd["param_groups"] for j in g["params"]) == list(range(n_train))
    # torch numbers parameters group by group; ours keep their index in the reference's two-group order (the moments'
    # index), so the partition is compared through the names
    assert sorted(j for g in ref["param_groups"] for j in g["params"]) == list(range(n_train))
    for ours, theirs, members in zip(sd["param_groups"], ref["param_groups"], ref_names):
        assert set(ours) == set(theirs) | {"layer_decay"}
        assert [order[j] for j in ours["params"]] == members and len(theirs["params"]) == len(members)
        assert ours["weight_decay"] == theirs["weight_decay"] and ours["lr"] == theirs["lr"]
        assert ours["lr"] == float(np.float32(1e-3) * np.float32(ours["layer_decay"]))
    # state j is parameter j of the order: its scale is its group's, its shape the parameter's
    shapes = {n: tuple(p.shape) for n, p in model.named_parameters()}
    for g in sd["param_groups"]:
        for j in g["params"]:
            assert np.float32(g["layer_decay"]) == L.scale(order[j], L.DECAY, L.LR_MULT)
            assert tuple(sd["state"][j]["exp_avg"].shape) == shapes[order[j]]
    # either form loads, whatever the optimizer's own scales; the base lr comes back from lr / layer_decay
    plain = (optim.GuardedClipAdamW if kind == "guarded" else optim.FusedClipAdamW)(model, lr=5e-4, weight_decay=0.05)
    assert plain.lr_segments is None
    plain.step_count = 3
    two = plain.state_dict()
    assert len(two["param_groups"]) == 2 and all("layer_decay" not in g for g in two["param_groups"])
    opt.load_state_dict(two)
    assert opt.step_count == 3 and [g["lr"] for g in opt.param_groups] == [5e-4, 5e-4]
    plain.load_state_dict(sd)
    assert plain.step_count == 2
    assert all(np.float32(g["lr"]) == np.float32(1e-3) for g in plain.param_groups)
    assert len(plain.state_dict()["param_groups"]) == 2


def test_without_a_table_the_state_dict_is_the_old_one(lib):
    """the dict written out here is what the optimizer gave before it knew about scales"""
    from svit_amd import optim
    cfg, model = _cpu_model()
    for opt in (optim.construct_optimizer(model, cfg), optim.FusedClipAdamW(model, lr=1e-3, lr_scale=lambda n: 1.0)):
        opt.param_groups[0]["lr"] = opt.param_groups[1]["lr"] = 1e-3
        wd = opt.param_groups[0]["weight_decay"]
        dec, rest = opt._order()
        sd = opt.state_dict()
        common = {"lr": 1e-3, "betas": (0.9, 0.999), "eps": 1e-8, "amsgrad": False, "maximize": False, "foreach": None,
                  "capturable": False, "differentiable": False, "fused": None, "decoupled_weight_decay": True}
        assert sd == {"state": {}, "param_groups": [
            dict(common, weight_decay=wd, params=list(range(len(dec)))),
            dict(common, weight_decay=0.0, params=list(range(len(dec), 405)))]}
        assert [list(g) for g in sd["param_groups"]] == [
            ["lr", "betas", "eps", "weight_decay", "amsgrad", "maximize", "foreach", "capturable", "differentiable",
             "fused", "decoupled_weight_decay", "params"]] * 2


def test_classic_launches_are_one_per_range_at_the_fp32_product():
    from svit_amd import optim
    _, model = _cpu_model()
    opt = optim.FusedClipAdamW(model, lr=1e-3, weight_decay=0.05, lr_scale=lambda n: L.scale(n, L.DECAY, L.LR_MULT))
    optim.set_lr(opt, 3e-4)
    launches = opt._launches()
    assert [(a, b) for _, a, b in launches] == [tuple(r) for r in opt.lr_segments.tolist()]
    nd = model.flat.n_decay
    for (g, a, b), c in zip(launches, opt.lr_scales):
        assert g["lr"] == float(np.float32(3e-4) * np.float32(c))
        assert g["weight_decay"] == (0.05 if a < nd else 0.0)
    assert [g["lr"] for g in opt.param_groups] == [3e-4, 3e-4]          # set_lr's two entries stay what they are


# ----------------------------------------------------------------------- argument checks of the entry point ----
def test_lr_entry_point_checks_its_arguments_without_a_gpu(lib):
    """refused before any HIP call: stream = None and made-up device addresses that are never followed"""
    P = 4096
    N, ND = 20000, 12296
    a = (0.9, 0.999, 1e-8, None)

    def adamw(segs, scales=None, S=None, n=N, nd=ND, ptrs=(P, P, P, P), no_scales=False):
        keep = np.array(segs, dtype=np.int64).reshape(-1, 2)
        sc = np.ones(max(len(keep), 1), dtype=np.float32) if scales is None else np.array(scales, dtype=np.float32)
        return lib.svit_adamw_step_guarded_lr(*ptrs, n, nd, keep.ctypes.data, None if no_scales else sc.ctypes.data,
                                              len(keep) if S is None else S, P, P, *a)

    good = [[0, 8], [4104, 4120], [ND - 8, ND], [ND, ND + 8], [13000, 19000], [N - 8, N]]
    bad_arg = {
        "S = 0": dict(segs=good, S=0),
        "S = 65": dict(segs=[[8 * i, 8 * i + 4] for i in range(65)]),
        "S < 0": dict(segs=good, S=-1),
        "unsorted": dict(segs=[[4104, 4120], [0, 8]]),
        "overlapping": dict(segs=[[0, 16], [8, 24]]),
        "empty": dict(segs=[[0, 8], [16, 16]]),
        "reversed": dict(segs=[[24, 16]]),
        "negative": dict(segs=[[-8, 8]]),
        "end > n": dict(segs=[[0, 8], [N - 8, N + 4]]),
        "straddles n_decay": dict(segs=[[ND - 8, ND + 8]]),
        "no scales": dict(segs=good, no_scales=True),
    }
    for label, kw in bad_arg.items():
        assert adamw(**kw) == -4, label
    for bad in (0.0, -0.0, -1.0, float("nan"), float("inf"), -float("inf")):
        for at in (0, 3, 5):
            sc = [1.0, 0.5, 2.0, 0.75 ** 17, 10.0, 1.0]
            sc[at] = bad
            assert adamw(segs=good, scales=sc) == -4, (bad, at)
    assert adamw(segs=[[0, 6]]) == -3 and adamw(segs=[[2, 8]]) == -3 and adamw(segs=[[0, 8], [4105, 4121]]) == -3
    assert lib.svit_adamw_step_guarded_lr(P, P, P, P, N, ND, None, np.ones(1, dtype=np.float32).ctypes.data, 1, P, P,
                                          *a) == -4
    for i in range(4):
        ptrs = [P, P, P, P]
        ptrs[i] = None
        assert adamw(segs=good, ptrs=ptrs) == -4
        ptrs[i] = P + 4
        assert adamw(segs=good, ptrs=ptrs) == -3
    assert adamw(segs=good, nd=N + 1) == -4 and adamw(segs=good, nd=-1) == -4
