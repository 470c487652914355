"""Frozen parameters, host side (svit_amd/freeze.py, SViT.freeze_below, the optimizers' state_dict under a cut, the
argument checks of svit_step_guard_seg / svit_adamw_step_guarded_seg).  No GPU needed."""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

from tests import freeze_cases as F


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__
    __graft_entry__.build()
    from svit_amd import hip
    return hip.load()


@pytest.fixture(scope="module")
def real_layout(golden_dir):
    """the flat placement of the reference's 405 tensors (tests/golden/layout.json), as SViT.finalize lays them out"""
    from svit_amd import arch
    from svit_amd.engine import FlatParams
    from svit_amd.model import _weight_decayed
    layout = json.load(open(os.path.join(golden_dir, "layout.json")))
    shapes = {n: tuple(layout["shapes"][n]) for n in layout["named_parameters"]}
    assert len(shapes) == 405
    skip = ("cls_token", "object_queries", "pos_embed_temporal")
    order, slots, n_decay, _, total, depth = FlatParams.layout(
        shapes, lambda n, s: _weight_decayed(n, s, skip), arch.readiness_rank)
    assert depth == F.DEPTH
    return list(shapes), slots, n_decay, total


def _cpu_model(flat=False):
    """an SViT that has not left the CPU (flags and names are all the host logic reads); flat: with the real
    FlatParams placement over untouched CPU memory, which is what an optimizer's constructor and state_dict need"""
    from svit_amd import arch, config
    from svit_amd.engine import FlatParams
    from svit_amd.model import MODEL_REGISTRY
    cfg = config.ssv2_cfg(num_frames=4, crop=64)
    model = MODEL_REGISTRY.get("SViT")(cfg)
    if flat:
        shapes = {n: tuple(p.shape) for n, p in model.named_parameters()}
        model.flat = FlatParams(shapes, model.weight_decayed, torch.device("cpu"), arch.readiness_rank)
    return cfg, model


# ------------------------------------------------------------------------------------------ cut -> segments ----
@pytest.mark.parametrize("cut", F.CUTS_CPU)
def test_segments_of_a_cut_on_the_real_layout(real_layout, cut):
    from svit_amd import freeze
    names, slots, n_decay, total = real_layout
    trainable = [n for n in names if F.position(n) >= cut]
    assert freeze.trainable_names(names, F.DEPTH, cut) == trainable
    segs = freeze.segments(slots, n_decay, trainable)
    assert segs.dtype == np.int64 and segs.ndim == 2 and segs.shape[1] == 2 and 1 <= len(segs) <= 64
    # exactly the trainable slots with their alignment padding
    assert np.array_equal(F.seg_mask(segs, total), F.slot_mask(slots, trainable, total))
    # sorted, disjoint, non-empty, merged (two segments touch only at the weight-decay boundary), cut at n_decay
    for i, (a, b) in enumerate(segs):
        assert 0 <= a < b <= total and a % 4 == 0 and b % 4 == 0
        assert not (a < n_decay < b), "segment %d straddles n_decay" % i
        if i:
            assert a >= segs[i - 1][1]
            assert a > segs[i - 1][1] or a == n_decay, "segments %d and %d are adjacent and not merged" % (i - 1, i)
    if cut == 0:
        assert segs.tolist() == [[0, n_decay], [n_decay, total]]
    else:
        assert len(segs) == 2       # readiness order: the trainable part leads each weight-decay group
        assert segs[0][0] == 0 and segs[0][1] <= n_decay
        # (rank 0 holds the final norm IN FRONT of the head's biases: head-only starts behind norm.weight / norm.bias)
        assert segs[1][0] == (n_decay if cut <= F.DEPTH + 1 else slots["norm.bias"][0] + slots["norm.bias"][1])
    # what is left over is the frozen part
    comp = freeze.complement(segs, total)
    assert np.array_equal(F.seg_mask(comp, total), ~F.seg_mask(segs, total))


def test_segments_merge_and_limit():
    from svit_amd import freeze
    slots = {"a": (0, 5, (5,)), "b": (8, 8, (8,)), "c": (24, 3, (3,)), "d": (32, 8, (8,))}
    assert freeze.segments(slots, 16, ["a", "b", "c", "d"]).tolist() == [[0, 16], [24, 40]]
    assert freeze.segments(slots, 8, ["a", "b"]).tolist() == [[0, 8], [8, 16]]          # cut at n_decay
    assert freeze.segments(slots, 16, ["d", "a"]).tolist() == [[0, 8], [32, 40]]
    many = {"p%d" % i: (16 * i, 8, (8,)) for i in range(65)}
    with pytest.raises(NotImplementedError):
        freeze.segments(many, 16 * 65, list(many))
    assert len(freeze.segments(many, 16 * 65, list(many)[:64])) == 64
    assert freeze.intersect([(0, 10), (20, 30)], [(4, 24)]) == [(4, 10), (20, 24)]


# ------------------------------------------------------------------------------------- flags, cuts, refusals ----
def test_freeze_below_sets_the_flags_of_the_positions():
    _, model = _cpu_model()
    names = [n for n, _ in model.named_parameters()]
    assert model.frozen_cut() == 0
    for cut in F.CUTS_CPU:
        model.freeze_below(cut)
        got = {n: p.requires_grad for n, p in model.named_parameters()}
        assert got == F.flags_for_cut(names, cut), cut
        assert model.frozen_cut() == cut
    with pytest.raises(ValueError):
        model.freeze_below(F.DEPTH + 3)
    with pytest.raises(ValueError):
        model.freeze_below(-1)


def test_build_model_reads_freeze_below_from_the_cfg():
    from svit_amd import config
    from svit_amd.model import build_model
    cfg = config.ssv2_cfg(num_frames=4, crop=64)
    assert not hasattr(cfg.SVIT, "FREEZE_BELOW")            # not a key of the default tree
    cfg.NUM_GPUS = 0
    cfg.SVIT.FREEZE_BELOW = 4
    model = build_model(cfg)             # (NUM_GPUS 0: stays on the CPU, on any machine)
    assert model.frozen_cut() == 4


def test_unsupported_patterns_are_refused_by_name():
    from svit_amd import optim
    cfg, model = _cpu_model(flat=True)
    params = dict(model.named_parameters())
    for label, flags, offender in F.unsupported_patterns(list(params)):
        for n, p in params.items():
            p.requires_grad_(flags[n])
        with pytest.raises(NotImplementedError, match=offender.replace(".", r"\.") + " ") as e:
            model.frozen_cut()
        assert offender in str(e.value), label
        for build in (lambda: optim.construct_optimizer(model, cfg),
                      lambda: optim.GuardedClipAdamW(model, lr=1e-3)):
            with pytest.raises(NotImplementedError, match=offender.replace(".", r"\.") + " "):
                build()


def test_nothing_trainable_is_adamws_value_error():
    from svit_amd import optim
    cfg, model = _cpu_model(flat=True)
    for p in model.parameters():
        p.requires_grad_(False)
    with pytest.raises(ValueError) as ours:
        optim.construct_optimizer(model, cfg)
    with pytest.raises(ValueError) as torchs:
        torch.optim.AdamW([])
    assert str(ours.value) == str(torchs.value)
    with pytest.raises(ValueError):
        model.frozen_cut()


# ------------------------------------------------------------------------------------------ state_dict ----------
def _reference_adamw(model):
    """torch.optim.AdamW over the reference's grouping of the trainable parameters: frozen ones left out, the decayed
    group first, then the 1-D / bias / skip-listed one, empty groups dropped"""
    skip = set(model.no_weight_decay())
    dec, zero = [], []
    for name, p in model.named_parameters():
        if not p.requires_grad:
            continue
        (zero if (name in skip or p.dim() == 1 or name.endswith(".bias")) else dec).append(torch.nn.Parameter(torch.empty(0)))
    groups = [{"params": dec, "weight_decay": 0.05}, {"params": zero, "weight_decay": 0.0}]
    return torch.optim.AdamW([g for g in groups if g["params"]], lr=1e-3)


@pytest.mark.parametrize("cut", [1, 4, F.DEPTH + 1, F.DEPTH + 2])
def test_state_dict_lists_the_trainable_parameters_in_the_references_groups(lib, cut):
    from svit_amd import optim
    _, model = _cpu_model(flat=True)
    full = optim.FusedClipAdamW(model, lr=1e-3, weight_decay=0.05)
    full.step_count = 2
    full_sd = full.state_dict()
    assert sum(len(g["params"]) for g in full_sd["param_groups"]) == 405
    model.freeze_below(cut)
    for cls in (optim.FusedClipAdamW, optim.GuardedClipAdamW):
        opt = cls(model, lr=1e-3, weight_decay=0.05)
        assert opt.cut == cut and opt.segments is not None
        opt.step_count = 2
        sd = opt.state_dict()
        ref = _reference_adamw(model).state_dict()
        assert [g["params"] for g in sd["param_groups"]] == [g["params"] for g in ref["param_groups"]]
        assert [g["weight_decay"] for g in sd["param_groups"]] == [g["weight_decay"] for g in ref["param_groups"]]
        n_train = sum(1 for p in model.parameters() if p.requires_grad)
        assert sorted(sd["state"]) == list(range(n_train)) and n_train < 405
        # state j is the j-th trainable parameter of the groups' order: shapes say so
        dec, rest = opt._order()
        for j, n in enumerate(dec + rest):
            assert tuple(sd["state"][j]["exp_avg"].shape) == tuple(dict(model.named_parameters())[n].shape)
            assert dict(model.named_parameters())[n].requires_grad
        opt.load_state_dict(sd)                              # its own state loads
        assert opt.step_count == 2
        with pytest.raises(ValueError, match="optimizer state lists 405 parameters, the model has %d" % n_train):
            opt.load_state_dict(full_sd)                     # a full-model state is refused
    with pytest.raises(ValueError, match="the model has 405"):
        model.freeze_below(0)
        optim.FusedClipAdamW(model, lr=1e-3).load_state_dict(sd)


# ------------------------------------------------------------------------ argument checks of the entry points ----
def _segs(rows):
    a = np.array(rows, dtype=np.int64).reshape(-1, 2)
    return a, a.ctypes.data


def test_seg_entry_points_check_their_arguments_without_a_gpu(lib):
    """refused before any HIP call: stream = None and made-up device addresses that are never followed"""
    P = 4096
    N, ND = 20000, 12296
    a = (0.9, 0.999, 1e-8, None)

    def guard(segs, S=None, n=N, g=P):
        keep, p = _segs(segs)
        return lib.svit_step_guard_seg(g, n, p, len(keep) if S is None else S, P, P, P, 10, P, 1024, None)

    def adamw(segs, S=None, n=N, nd=ND, ptrs=(P, P, P, P)):
        keep, p = _segs(segs)
        return lib.svit_adamw_step_guarded_seg(*ptrs, n, nd, p, len(keep) if S is None else S, P, P, *a)

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
    }
    for fn in (guard, adamw):
        for label, kw in bad_arg.items():
            assert fn(**kw) == -4, (fn.__name__, label)
        assert fn(segs=[[0, 6]]) == -3 and fn(segs=[[2, 8]]) == -3 and fn(segs=[[0, 8], [4105, 4121]]) == -3
    assert lib.svit_step_guard_seg(P, N, None, 1, P, P, P, 10, P, 1024, None) == -4              # no table
    assert lib.svit_adamw_step_guarded_seg(P, P, P, P, N, ND, None, 1, P, P, *a) == -4
    assert adamw(segs=[[ND - 8, ND + 8]]) == -4               # straddles n_decay
    # the checks of the plain pair still hold in front of the table's
    keep, p = _segs(good)
    assert lib.svit_step_guard_seg(None, N, p, 6, P, P, P, 10, P, 1024, None) == -4
    assert lib.svit_step_guard_seg(P, 0, p, 6, P, P, P, 10, P, 1024, None) == -4
    assert lib.svit_step_guard_seg(P, N, p, 6, P + 4, P, P, 10, P, 1024, None) == -3
    assert lib.svit_step_guard_seg(P + 4, N, p, 6, P, P, P, 10, P, 1024, None) == -3               # g not 16-byte aligned
    assert lib.svit_step_guard_seg(P, N, p, 6, P, P, P, 10, P, 0, None) == -4                      # no room for one partial
    for i in range(4):
        ptrs = [P, P, P, P]
        ptrs[i] = None
        assert adamw(segs=good, ptrs=ptrs) == -4
        ptrs[i] = P + 4
        assert adamw(segs=good, ptrs=ptrs) == -3
    assert adamw(segs=good, nd=N + 1) == -4 and adamw(segs=good, nd=-1) == -4
    assert C.sizeof(C.c_int64) == 8


def test_slab_lead_checks_its_arguments_without_a_gpu(lib):
    """svit_gemm_tn_grouped_slab_lead: the leading-problem count and the whole list's checks, before any launch"""
    from svit_amd import hip
    arr = (hip.TnProblem * 3)()
    for t, (M, N, K) in zip(arr, ((512, 96, 96), (512, 288, 96), (2048, 96, 96))):
        t.A, t.B, t.dW, t.dbias = 1 << 20, 2 << 20, 3 << 20, None
        t.lda, t.ldb, t.lddw, t.M, t.N, t.K = N, K, K, M, N, K
    need = lib.svit_gemm_tn_grouped_workspace(arr, 3)
    assert need > 0
    P = 4096
    for lead in (0, -1, 4):
        assert lib.svit_gemm_tn_grouped_slab_lead(arr, 3, lead, P, need, None) == -4
    assert lib.svit_gemm_tn_grouped_slab_lead(arr, 3, 2, None, need, None) == -4         # no workspace
    assert lib.svit_gemm_tn_grouped_slab_lead(arr, 3, 2, P, need - 1, None) == -4        # sized for the WHOLE list
    assert lib.svit_gemm_tn_grouped_slab_lead(arr, 3, 2, P + 4, need, None) == -3
    arr[2].M = 0                                                                         # a follower is checked too
    assert lib.svit_gemm_tn_grouped_slab_lead(arr, 3, 2, P, need, None) == -2


def test_header_declares_the_segment_limit():
    from svit_amd import freeze
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = open(os.path.join(root, "include", "svit_hip.h")).read()
    assert "#define SVIT_MAX_SEGS %d" % freeze.MAX_SEGS in text
