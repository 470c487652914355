"""Slab-reduced weight gradients (svit_gemm_tn_grouped_slab / svit_gemm_tn_grouped_workspace): what can be
checked without a GPU -- the two entry points exist on every layer, the workspace query is host-only arithmetic
that answers for every call the launch entry point accepts, and a missing or short workspace is refused before
any launch."""
import ctypes as C
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# the eleven shapes of tests/test_kernels_gpu.py::_tn_grouped_case (M, N, K) and the block-0 problem of the bench step
SHAPES = [(1000, 288, 96), (4100, 384, 1536), (70, 96, 441), (13064, 384, 384), (333, 40, 96),
          (64, 3072, 768), (2000, 1152, 384), (5000, 96, 96), (129, 128, 96), (8000, 64, 96),
          (700, 768, 768)]
BLOCK0 = (201224, 384, 96)
ERR_ARG = -4


def _lib():
    import __graft_entry__
    __graft_entry__.build()
    from svit_amd import hip
    return hip, hip.load()


def _problems(hip, shapes):
    """fake non-null, 16-byte aligned operand pointers (nothing is launched): row-strided a, padded ldb, every
    third problem without a bias, as the GPU case builds them"""
    arr = (hip.TnProblem * len(shapes))()
    for i, (t, (M, N, K)) in enumerate(zip(arr, shapes)):
        t.A, t.B, t.dW = 1 << 20, 2 << 20, 3 << 20
        t.dbias = (4 << 20) if i % 3 != 2 else None
        t.lda, t.ldb, t.lddw, t.M, t.N, t.K = N + 16, (K + 7) // 8 * 8, K, M, N, K
    return arr


def test_both_symbols_are_declared_bound_and_exported():
    hip, lib = _lib()
    header = open(os.path.join(ROOT, "include", "svit_hip.h")).read()
    for name in ("svit_gemm_tn_grouped_slab", "svit_gemm_tn_grouped_workspace"):
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert name in hip.EXPORTS
        assert hasattr(lib, name), name
    assert lib.svit_gemm_tn_grouped_workspace.restype is C.c_int64


def test_workspace_query_answers_without_a_gpu():
    hip, lib = _lib()
    sizes = []
    for count in range(1, len(SHAPES) + 1):
        need = lib.svit_gemm_tn_grouped_workspace(_problems(hip, SHAPES[:count]), count)
        assert need > 0, (count, need)
        sizes.append(need)
    # the size grows when a problem is added (not a law for every step: the planner re-cuts ALL problems of a group
    # when one joins, so a later group may be cut coarser -- these steps add a problem larger than the re-cut saves)
    assert sizes[-1] > sizes[0]
    for a, b in ((1, 2), (3, 4), (5, 6)):
        assert sizes[b - 1] > sizes[a - 1], sizes
    assert lib.svit_gemm_tn_grouped_workspace(_problems(hip, [BLOCK0]), 1) >= BLOCK0[1] * BLOCK0[2]
    # more problems than one launch group holds: the largest group's need, still positive
    many = SHAPES + SHAPES
    assert lib.svit_gemm_tn_grouped_workspace(_problems(hip, many), len(many)) >= sizes[-1]


def test_workspace_holds_at_least_one_tile_set():
    """a one-problem, one-split call: the slab of the only split holds every dW element"""
    hip, lib = _lib()
    for M, N, K in ((64, 96, 96), (32, 384, 96), (64, 3072, 768), (20, 40, 441)):
        need = lib.svit_gemm_tn_grouped_workspace(_problems(hip, [(M, N, K)]), 1)
        assert need >= N * K, (M, N, K, need)


def test_workspace_query_reports_argument_errors():
    hip, lib = _lib()
    assert lib.svit_gemm_tn_grouped_workspace(None, 1) == ERR_ARG
    arr = _problems(hip, SHAPES[:2])
    assert lib.svit_gemm_tn_grouped_workspace(arr, 0) == ERR_ARG
    arr[1].A = None
    assert lib.svit_gemm_tn_grouped_workspace(arr, 2) == ERR_ARG
    arr = _problems(hip, SHAPES[:2])
    arr[0].M = 0
    assert lib.svit_gemm_tn_grouped_workspace(arr, 2) == -2
    arr = _problems(hip, SHAPES[:2])
    arr[0].lda = arr[0].N + 3
    assert lib.svit_gemm_tn_grouped_workspace(arr, 2) == -3


def test_slab_entry_point_refuses_a_missing_or_short_workspace_before_any_launch():
    hip, lib = _lib()
    for shapes in (SHAPES, SHAPES[:1], [BLOCK0], SHAPES + SHAPES):
        arr = _problems(hip, shapes)
        n = len(shapes)
        need = lib.svit_gemm_tn_grouped_workspace(arr, n)
        assert need > 0
        assert lib.svit_gemm_tn_grouped_slab(arr, n, None, need, None) == ERR_ARG
        assert lib.svit_gemm_tn_grouped_slab(arr, n, 5 << 20, need - 1, None) == ERR_ARG
        assert lib.svit_gemm_tn_grouped_slab(arr, n, 5 << 20, 0, None) == ERR_ARG
    # and the problem checks of svit_gemm_tn_grouped come first
    arr = _problems(hip, SHAPES[:1])
    arr[0].dW = None
    assert lib.svit_gemm_tn_grouped_slab(arr, 1, 5 << 20, 1 << 30, None) == ERR_ARG


def test_engine_switch_is_not_a_key_of_the_default_tree():
    """cfg.SVIT.REPRODUCIBLE is read with getattr where the engine is created (like SVIT.CONSISTENCY's reader):
    the default config tree, and with it tests/golden/cfg.json, stay as they are"""
    from svit_amd import config
    cfg = config.ssv2_cfg(num_frames=4, crop=64)
    assert not hasattr(cfg.SVIT, "REPRODUCIBLE")
    src = open(os.path.join(ROOT, "svit_amd", "model.py")).read()
    assert re.search(r'getattr\(self\.cfg\.SVIT,\s*"REPRODUCIBLE",\s*False\)', src)
