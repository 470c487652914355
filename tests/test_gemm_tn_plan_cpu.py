"""Host side of the TN weight-gradient GEMMs (csrc/gemm_tn.hip), asked through svit_debug_gemm_tn_plan -- no GPU.  The query
runs tn_check, tn_plan / tn_single_plan and tn_chunks, the functions the launch entry points run, so what it answers is what a
launch runs: the plan of every TN GEMM call of the 16x224^2 training step and of the shape lists of the GPU tests is pinned, the
query is shown to agree with the workspace query and with its own grids, and the plans hold their invariants over a grid."""
import ctypes as C
import itertools
import json
import os
import random

import pytest

from tests.test_reproducible_wgrad_cpu import BLOCK0, SHAPES

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# tests/golden/gemm_tn_plans.json: "step_groups" / "step_singles" are the (M, N, K, has_bias) lists that Engine._flush_tn handed to
# ops.gemm_tn_grouped, in order, and the stand-alone ops.gemm_tn calls, in one eager 16x224^2 B = 8 training step on an MI355X
# (a wrapper around the three ops functions noted them).  "cases" are the plans of those and of the other pinned lists.  Every
# value in it was recorded from the planner as it stood BEFORE tn_chunks and the query existed (a build of that gemm_tn.hip
# with its launches replaced by recorders of grid, TnGroup and TnSlabs, its knob reads by a table), never from the code under
# test: the test pins that the rewrite planned nothing differently.  A case: name, mode (svit_debug_set_tn_tile), form,
# arg (splits, form 3), problems, ws (floats of slab workspace the old svit_gemm_tn_grouped_workspace answered; form 2) and per
# launch group grid, red (reduce grid) and a row of FIELDS per problem.
GOLDEN = json.load(open(os.path.join(ROOT, "tests", "golden", "gemm_tn_plans.json")))
CASES = GOLDEN["cases"]
FIELDS = ("tile_kind", "tiles_n", "tiles_k", "rows_per_split", "splits", "first_block", "w", "tile_off", "bias_off", "red_first")
TN_SINGLE = [(1000, 288, 96), (70, 96, 448), (4100, 384, 1536), (333, 96, 96), (64, 3072, 768)]      # test_kernels_gpu.test_gemm_tn
GROUP_MAX = 16


@pytest.fixture(scope="module")
def ops():
    import __graft_entry__
    __graft_entry__.build()
    from svit_amd import ops
    return ops


@pytest.fixture()
def lib(ops):
    from svit_amd import hip
    lib = hip.load()
    yield lib
    lib.svit_debug_reset()


def _with_bias(shapes):
    """every third problem without a bias, as _tn_grouped_case and test_reproducible_wgrad_cpu._problems build them"""
    return [[M, N, K, i % 3 != 2] for i, (M, N, K) in enumerate(shapes)]


def test_the_pinned_cases_are_the_ones_asked_for():
    step = GOLDEN["step_groups"]
    assert [len(g) for g in step] == [15, 14, 14, 14, 14, 14, 15, 15]      # two blocks per flush; three rel-pos tables a block
    assert step[0][0] == [3656, 768, 3072, True] and step[-1][-1] == [201224, 288, 96, True]
    assert GOLDEN["step_singles"] == [[200704, 96, 441, True]]             # the patch-embedding wgrad; no table is interpolated
    want = {("step%d" % i, mode, form): g for i, g in enumerate(step) for mode in (2, 1) for form in (0, 1, 2)}
    want.update({("shapes%d" % n, mode, form): _with_bias(SHAPES[:n]) for n in (1, 5, 11) for mode in range(4) for form in range(3)})
    for form in range(3):
        want[("block0", 2, form)] = _with_bias([BLOCK0])
        want[("shapes22", 2, form)] = _with_bias(SHAPES + SHAPES)
    grouped = {(c["name"], c["mode"], c["form"]): c["problems"] for c in CASES if c["form"] != 3}
    assert grouped == want
    single = sorted((tuple(c["problems"][0]), c["arg"]) for c in CASES if c["form"] == 3)
    assert single == sorted([((200704, 96, 441, True), 0)] + [((M, N, K, True), s) for M, N, K in TN_SINGLE for s in (0, 1, 3)])
    assert len(CASES) == len(grouped) + len(single) == 106


@pytest.mark.parametrize("case", CASES, ids=["%s-mode%d-form%d-arg%d" % (c["name"], c["mode"], c["form"], c["arg"]) for c in CASES])
def test_plans_are_the_ones_recorded_before_the_rewrite(ops, lib, case):
    from svit_amd import hip
    assert lib.svit_debug_set_tn_tile(case["mode"]) == 0
    problems = [tuple(p) for p in case["problems"]]
    plan = ops.gemm_tn_plan(problems, form=case["form"], splits=case["arg"])
    assert plan["form"] == ops.TN_FORMS[case["form"]]
    assert plan["workspace_floats"] == case["ws"]
    assert len(plan["groups"]) == len(case["groups"]) == -(-len(problems) // GROUP_MAX)
    for got, want in zip(plan["groups"], case["groups"]):
        assert (got["grid"], got["reduce_grid"]) == (want["grid"], want["red"])
        assert [[p[f] for f in FIELDS] for p in got["problems"]] == want["problems"]
        # the query's own arithmetic: the grid ends where the last problem's workgroups end
        last = got["problems"][-1]
        assert got["grid"] == last["first_block"] + last["tiles_n"] * last["tiles_k"] * last["splits"]
    if case["form"] == 2:      # ... and its workspace figure is the workspace query's, on the same array
        arr = (hip.TnProblem * len(problems))()
        for t, (M, N, K, bias) in zip(arr, problems):
            t.A, t.B, t.dW, t.dbias = 1 << 20, 2 << 20, 3 << 20, (4 << 20) if bias else None
            t.lda, t.ldb, t.lddw, t.M, t.N, t.K = (N + 7) // 8 * 8 + 16, (K + 7) // 8 * 8 + 8, K + 3, M, N, K      # (strided operands)
        assert lib.svit_gemm_tn_grouped_workspace(arr, len(problems)) == plan["workspace_floats"] > 0
    else:
        assert plan["workspace_floats"] == 0 and all(g["reduce_grid"] == 0 for g in plan["groups"])


def test_tile_kinds_of_the_training_step(ops, lib):
    """default mode (2): every problem of the step runs 128x192 tiles; mode 1 (the isolated-launch heuristic) reaches both"""
    def kinds():
        return {p["tile_kind"] for g in GOLDEN["step_groups"] for form in ops.TN_FORMS[:3]
                for grp in ops.gemm_tn_plan([tuple(p) for p in g], form=form)["groups"] for p in grp["problems"]}
    assert kinds() == {1}
    assert lib.svit_debug_set_tn_tile(1) == 0
    assert kinds() == {0, 1}


MS = (1, 20, 64, 65, 333, 4100, 13064, 201224)
NS = (40, 96, 128, 288, 3072)
KS = (96, 192, 384, 441, 1536)


def _groups_of(size):
    shapes = list(itertools.product(MS, NS, KS))
    random.Random(size).shuffle(shapes)
    return [_with_bias(shapes[i:i + size]) for i in range(0, len(shapes) - size + 1, size)]


@pytest.mark.parametrize("size", [1, 3, 16])
def test_plans_hold_their_invariants(ops, size):
    groups = _groups_of(size)
    assert len(groups) == 200 // size
    for problems, form in itertools.product(groups, (0, 1, 2)):
        plan = ops.gemm_tn_plan([tuple(p) for p in problems], form=form)
        (g,) = plan["groups"]
        where = "form %d %s: %s" % (form, problems, plan)
        block, regions, red = 0, [], 0
        for (M, N, K, bias), p in zip(problems, g["problems"]):
            tk, stage = (192, 32) if p["tile_kind"] else (96, 64)           # tile columns, reduction rows per stage
            assert p["tile_kind"] in (0, 1) and (p["tiles_n"], p["tiles_k"]) == (-(-N // 128), -(-K // tk)), where
            assert p["splits"] * p["rows_per_split"] >= M > (p["splits"] - 1) * p["rows_per_split"], where
            assert p["rows_per_split"] > 0 and p["rows_per_split"] % stage == 0, where
            assert form != 1 or p["splits"] == 1, where
            assert p["first_block"] == block, where
            block += p["tiles_n"] * p["tiles_k"] * p["splits"]
            if form == 2:
                assert p["w"] == min(tk, -(-K // 32) * 32) and p["red_first"] >= red, where
                red = p["red_first"]
                regions.append((p["tile_off"], p["tiles_n"] * p["tiles_k"] * p["splits"] * 128 * p["w"]))
                regions.append((p["bias_off"], p["splits"] * p["tiles_n"] * 128 if bias else 0))
            else:
                assert (p["w"], p["tile_off"], p["bias_off"], p["red_first"]) == (0, 0, 0, 0), where
        assert g["grid"] == block, where
        if form == 2:
            end = 0
            for off, floats in sorted(regions):                               # (an empty region may share its offset)
                assert off % 4 == 0 and floats % 4 == 0 and off >= end, where
                end = off + floats
            assert plan["workspace_floats"] == end > 0, where
            assert g["reduce_grid"] > red, where
    if size == 1:      # the stand-alone GEMM: 128x96 tiles, whole 64-row stages, the split count its chooser or the caller's
        for (M, N, K, bias), splits in itertools.product([p[0] for p in groups], (0, 1, 3)):
            (g,) = ops.gemm_tn_plan([(M, N, K, bias)], form="single", splits=splits)["groups"]
            (p,) = g["problems"]
            assert (p["tile_kind"], p["tiles_n"], p["tiles_k"]) == (0, -(-N // 128), -(-K // 96))
            assert p["splits"] * p["rows_per_split"] >= M > (p["splits"] - 1) * p["rows_per_split"] and p["rows_per_split"] % 64 == 0
            assert p["splits"] <= (splits or 512) and g["grid"] == p["tiles_n"] * p["tiles_k"] * p["splits"]


def test_errors_are_the_entry_points(ops, lib):
    """the cases of test_reproducible_wgrad_cpu.test_workspace_query_reports_argument_errors, through the query, in every form;
    SVIT_ERR_ARG (-4) for what only the query can be asked wrongly"""
    from svit_amd import hip
    from tests.test_reproducible_wgrad_cpu import _problems
    out = (C.c_int64 * 64)()
    for form in range(4):
        n = 1 if form == 3 else 2      # (form 3 takes one problem: the faulty one)
        assert lib.svit_debug_gemm_tn_plan(None, 1, form, 0, out, 64) == -4
        arr = _problems(hip, SHAPES[:2])
        assert lib.svit_debug_gemm_tn_plan(arr, 0, form, 0, out, 64) == -4
        arr[n - 1].A = None
        assert lib.svit_debug_gemm_tn_plan(arr, n, form, 0, out, 64) == -4
        arr = _problems(hip, SHAPES[:2])
        arr[0].M = 0
        assert lib.svit_debug_gemm_tn_plan(arr, n, form, 0, out, 64) == -2
        arr = _problems(hip, SHAPES[:2])
        arr[0].lda = arr[0].N + 3
        assert lib.svit_debug_gemm_tn_plan(arr, n, form, 0, out, 64) == -3
        arr = _problems(hip, SHAPES[:2])
        arr[0].lda, arr[0].M = arr[0].N + 3, -1                      # shape before alignment
        assert lib.svit_debug_gemm_tn_plan(arr, n, form, 0, out, 64) == -2
        arr = _problems(hip, SHAPES[:2])
        need = 2 + 3 + 10 * n
        assert lib.svit_debug_gemm_tn_plan(arr, n, form, 0, out, need) == need
        assert lib.svit_debug_gemm_tn_plan(arr, n, form, 0, out, need - 1) == -4
        assert lib.svit_debug_gemm_tn_plan(arr, n, form, 0, None, need) == -4
    arr = _problems(hip, SHAPES[:2])
    assert lib.svit_debug_gemm_tn_plan(arr, 2, 3, 0, out, 64) == -4      # the stand-alone form with two problems
    assert lib.svit_debug_gemm_tn_plan(arr, 2, 4, 0, out, 64) == -4 and lib.svit_debug_gemm_tn_plan(arr, 2, -1, 0, out, 64) == -4
    with pytest.raises(hip.SvitHipError):
        ops.gemm_tn_plan([(1000, 288, 96, True)] * 2, form="single")
    with pytest.raises(hip.SvitHipError):
        ops.gemm_tn_plan([], form="atomic")
