"""Host side of the pooling kernels (csrc/pool.hip), asked through svit_debug_pool_plan -- no GPU: the chunk plans of the staged
conv forward and of the fused conv backward hold their invariants over a grid of geometries, and the forward chooser takes the
paths its comments promise at every block of the 16x224^2 training step and in a T = 1 pass."""
import itertools

import pytest

BHS = (1, 2, 8, 32, 64, 96)
TS = (1, 2, 3, 4, 8, 16)
PLANES = ((7, 7), (14, 14), (28, 28), (56, 56), (78, 78), (19, 26), (23, 17))
STRIDES = ((1, 1, 1), (1, 2, 2), (2, 2, 2), (2, 4, 4), (1, 8, 8), (1, 3, 3))
N_OBJ = 4
LDS_MAX = 79 * 1024


@pytest.fixture(scope="module")
def ops():
    import __graft_entry__
    __graft_entry__.build()
    from svit_amd import ops
    return ops


def _rows(kind, H, s):
    """extent a tensor is cut along y: output rows (staged forward); rows of units of the input plane (fused backward:
    one row at stride 1, two at stride 2, the stride's window from 3 on)"""
    Ho = (H - 1) // s + 1
    return Ho if kind == 1 or s >= 3 else H if s == 1 else (H + 1) // 2


@pytest.mark.parametrize("kind", [1, 2], ids=["staged_fwd", "fused_bwd"])
def test_chunk_plans_hold_their_invariants(ops, kind):
    plans = 0
    for BH, T, (H, W), strides in itertools.product(BHS, TS, PLANES, STRIDES):
        where = "kind %d BH %d T %d plane %dx%d strides %s" % (kind, BH, T, H, W, strides)
        p = ops.pool_plan(kind, BH, 1, (T, H, W), N_OBJ, strides)
        if kind == 2:       # the workspace query answers from the same plan
            need = ops.pool_conv_bwd_workspace(BH, 1, (T, H, W), N_OBJ, strides)
            assert need == (-1 if p is None else BH * p["max_chunks"] * 3 * 27 * 96), where
        if p is None:
            continue
        plans += 1
        for i in range(3):
            n, r, tc, yc, rows = p["n_per"][i], p["r_per"][i], p["t_chunks"][i], p["y_chunks"][i], _rows(kind, H, strides[i])
            # the chunks cover T and the rows exactly, and the last one is not empty
            assert 1 <= n <= T and tc == -(-T // n) and (tc - 1) * n < T, where
            assert 1 <= r <= rows and yc == -(-rows // r) and (yc - 1) * r < rows, where
        assert p["n_per"][1] == p["n_per"][2] and p["r_per"][1] == p["r_per"][2], where      # k and v share a choice
        assert 0 < p["lds"] <= LDS_MAX, where
        assert sorted(p["order"]) == [0, 1, 2], where
        assert p["first_item"][0] == 0, where
        for j, t in enumerate(p["order"]):
            assert p["first_item"][j + 1] - p["first_item"][j] == 3 * BH * p["t_chunks"][t] * p["y_chunks"][t] > 0, where
        assert p["max_chunks"] == max(p["t_chunks"][i] * p["y_chunks"][i] for i in range(3)), where
        if kind == 2:
            assert BH * p["max_chunks"] <= 4096, where
    assert plans > 1000         # (the 78x78 planes of the large batches have none)


def _step_geometries(num_frames, crop, frames_pass=False):
    """(block, heads, thw, n_obj, strides, sels given, relq_lpad) as Engine._block_fwd hands them to ops.pool_ln_fwd_qkv"""
    from svit_amd import arch, config
    from svit_amd.engine import FlatParams
    plan = arch.build_plan(config.ssv2_cfg(num_frames, crop))
    T = 1 if frames_pass else plan.num_frames // plan.patch_stride[0]
    thw = (T, crop // plan.patch_stride[1], crop // plan.patch_stride[2])
    n_obj = (1 if frames_pass else plan.num_frames) * plan.objects
    for blk in plan.blocks:
        sq, skv = blk.stride_q[1], blk.stride_kv[1]
        plane = thw[1] * thw[2]
        rows = 2 * blk.rel_sp_rows + (blk.rel_t_rows if not frames_pass else 1)
        yield (blk.index, blk.heads, thw, n_obj, (sq, skv, skv),
               plane >= FlatParams.TILED_MIN_PLANE or plane <= FlatParams.SLAB_MAX_PLANE, (rows + 95) // 96 * 96)
        thw = (thw[0], arch.pooled(thw[1], sq), arch.pooled(thw[2], sq))


def test_forward_paths_of_the_training_step(ops):
    """16x224^2, B = 8, pre / mean / rstd saved: staged conv at blocks 0-3 (planes past 14x14), MFMA slab conv at blocks 4-13
    (its 12 B heads workgroups are one round), VALU slab conv at blocks 14 / 15 (8 heads); pool_slab_ln_kernel writes q's
    rel-pos columns at every block."""
    want = ["staged"] * 4 + ["mfma"] * 10 + ["slab"] * 2
    conv = {"staged": "pool_fwd_staged", "mfma": "pool_mfma_fwd", "slab": "pool_slab_fwd"}
    geoms = list(_step_geometries(16, 224))
    assert [g[0] for g in geoms] == list(range(16)) and geoms[0][2] == (8, 56, 56) and geoms[15][2] == (8, 7, 7)
    for (idx, heads, thw, n_obj, strides, sels, lpad), path in zip(geoms, want):
        got, relq, launches = ops.pool_plan(0, 8, heads, thw, n_obj, strides, save=True, sels=sels, relq_lpad=lpad)
        assert (got, relq) == (path, "pool_slab_ln"), "block %d" % idx
        assert [l[0] for l in launches] == [conv[path], "pool_slab_ln"], "block %d" % idx
        assert launches[1][2:5] == (8 * heads, 3, 256) and all(l[5] <= 160 * 1024 for l in launches), "block %d" % idx


@pytest.mark.parametrize("save", [False, True])
def test_one_plane_pass_takes_the_frame_kernel(ops, save):
    """T = 1 (the frames pass; an image rank's training step with save): one pool_frame_fwd_kernel launch at every block, q's
    rel-pos columns from the trailing GEMM"""
    for idx, heads, thw, n_obj, strides, sels, lpad in _step_geometries(16, 224, frames_pass=True):
        got, relq, launches = ops.pool_plan(0, 8, heads, thw, n_obj, strides, save=save, sels=sels, relq_lpad=lpad)
        assert (got, relq) == ("frame", "gemm") and [l[0] for l in launches] == ["pool_frame_fwd"], "block %d" % idx
        assert launches[0][1] <= 256 and launches[0][4] == 512, "block %d" % idx
