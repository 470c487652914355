"""Host side of svit_gemm_nt (csrc/gemm_nt.hip), asked through svit_debug_gemm_nt_plan -- no GPU.  The query calls nt_choose,
the function the launch path calls, so what it answers is what a launch runs: the kernel of every NT GEMM of the 16x224^2
training step and of its frames pass is pinned, every named form of tests/gemm_reference.py is shown to be the kernel it
names at every shape the parity suite gives it, and the launch geometry holds its invariants over a grid of shapes."""
import itertools

import pytest

from tests import gemm_reference as G

EPI_BF16, EPI_GELU, EPI_RESID, EPI_F32, EPI_DGELU, EPI_RELQ = range(6)
FIELDS = ("family", "RB", "NB", "WM", "WN", "NL", "stages", "BK", "gx", "gy", "block", "lds")
LDS_MAX = 160 * 1024

# (M, N, K, epilogue) -> FIELDS, for every distinct NT GEMM call of _step_calls(16, 224, 8) and of its frames pass.  The values
# were recorded from the dispatcher as it stood BEFORE nt_choose existed (its launches replaced by recorders, default knobs),
# never from nt_choose: the test pins that the rewrite chose nothing differently.
STEP_CHOICES = {
    (200704, 96, 448, 3):      (0, 1, 3, 4, 1, 0, 2, 64, 1, 1568, 256, 57344),
    (201224, 288, 96, 0):      (0, 1, 3, 4, 1, 0, 2, 32, 3, 1573, 256, 32768),
    (201224, 96, 96, 2):       (0, 1, 3, 4, 1, 0, 2, 32, 1, 1573, 256, 32768),
    (201224, 384, 96, 1):      (0, 2, 3, 2, 2, 0, 2, 32, 2, 1573, 256, 40960),
    (201224, 96, 384, 2):      (0, 1, 3, 4, 1, 0, 2, 64, 1, 1573, 256, 57344),
    (201224, 384, 96, 4):      (0, 2, 3, 2, 2, 0, 2, 32, 2, 1573, 256, 40960),
    (201224, 96, 384, 0):      (0, 1, 3, 4, 1, 0, 2, 64, 1, 1573, 256, 57344),
    (201224, 96, 96, 0):       (0, 1, 3, 4, 1, 0, 2, 32, 1, 1573, 256, 32768),
    (201224, 96, 288, 0):      (0, 1, 3, 4, 1, 0, 2, 32, 1, 1573, 256, 32768),
    (201224, 576, 96, 0):      (0, 2, 3, 2, 2, 0, 2, 32, 3, 1573, 256, 40960),
    (201224, 192, 96, 3):      (0, 2, 3, 2, 2, 0, 2, 32, 1, 1573, 256, 40960),
    (50696, 192, 192, 2):      (0, 2, 3, 2, 2, 0, 2, 32, 1, 397, 256, 40960),
    (50696, 768, 192, 1):      (0, 2, 3, 2, 2, 0, 2, 32, 4, 397, 256, 40960),
    (50696, 192, 768, 2):      (0, 1, 3, 4, 1, 0, 2, 64, 2, 397, 256, 57344),
    (50696, 768, 192, 4):      (0, 2, 3, 2, 2, 0, 2, 32, 4, 397, 256, 40960),
    (50696, 192, 768, 0):      (0, 1, 3, 4, 1, 0, 2, 64, 2, 397, 256, 57344),
    (50696, 192, 192, 0):      (0, 2, 3, 2, 2, 0, 2, 32, 1, 397, 256, 40960),
    (201224, 96, 576, 3):      (0, 1, 3, 4, 1, 0, 2, 64, 1, 1573, 256, 57344),
    (201224, 96, 192, 3):      (0, 1, 3, 4, 1, 0, 2, 32, 1, 1573, 256, 32768),
    (50696, 576, 192, 0):      (0, 2, 3, 2, 2, 0, 2, 32, 3, 397, 256, 40960),
    (50696, 192, 576, 0):      (0, 1, 3, 4, 1, 0, 2, 64, 2, 397, 256, 57344),
    (50696, 1152, 192, 0):     (0, 2, 3, 2, 2, 0, 2, 32, 6, 397, 256, 40960),
    (50696, 384, 192, 3):      (0, 2, 3, 2, 2, 0, 2, 32, 2, 397, 256, 40960),
    (13064, 384, 384, 2):      (0, 1, 3, 4, 1, 0, 2, 64, 4, 103, 256, 57344),
    (13064, 1536, 384, 1):     (0, 5, 2, 1, 4, 0, 2, 32, 6, 82, 256, 57344),
    (13064, 384, 1536, 2):     (1, 2, 3, 2, 2, 4, 3, 64, 2, 103, 512, 122880),
    (13064, 1536, 384, 4):     (0, 5, 2, 1, 4, 0, 2, 32, 6, 82, 256, 57344),
    (13064, 384, 1536, 0):     (1, 2, 3, 2, 2, 4, 3, 64, 2, 103, 512, 122880),
    (13064, 384, 384, 0):      (0, 1, 3, 4, 1, 0, 2, 64, 4, 103, 256, 57344),
    (50696, 192, 1152, 3):     (1, 2, 3, 2, 2, 4, 3, 64, 1, 397, 512, 122880),
    (50696, 192, 384, 3):      (0, 1, 3, 4, 1, 0, 2, 64, 2, 397, 256, 57344),
    (13064, 1152, 384, 0):     (0, 3, 3, 2, 2, 0, 2, 32, 6, 69, 256, 49152),
    (13064, 384, 1152, 0):     (1, 2, 3, 2, 2, 4, 3, 64, 2, 103, 512, 122880),
    (13064, 2304, 384, 0):     (0, 2, 2, 2, 2, 0, 2, 32, 18, 103, 256, 32768),
    (13064, 768, 384, 3):      (0, 1, 3, 4, 1, 0, 2, 64, 8, 103, 256, 57344),
    (3656, 768, 768, 2):       (1, 1, 3, 4, 1, 4, 4, 64, 8, 29, 512, 114688),
    (3656, 3072, 768, 1):      (0, 2, 3, 2, 2, 0, 2, 32, 16, 29, 256, 40960),
    (3656, 768, 3072, 2):      (1, 1, 3, 4, 1, 4, 4, 64, 8, 29, 512, 114688),
    (3656, 3072, 768, 4):      (0, 2, 3, 2, 2, 0, 2, 32, 16, 29, 256, 40960),
    (3656, 768, 3072, 0):      (1, 1, 3, 4, 1, 4, 4, 64, 8, 29, 512, 114688),
    (3656, 768, 768, 0):       (1, 1, 3, 4, 1, 4, 4, 64, 8, 29, 512, 114688),
    (13064, 384, 2304, 3):     (1, 2, 3, 2, 2, 4, 3, 64, 2, 103, 512, 122880),
    (13064, 384, 768, 3):      (0, 1, 3, 4, 1, 0, 2, 64, 4, 103, 256, 57344),
    (3656, 2304, 768, 0):      (0, 2, 3, 2, 2, 0, 2, 32, 12, 29, 256, 40960),
    (3656, 768, 2304, 0):      (1, 1, 3, 4, 1, 4, 4, 64, 8, 29, 512, 114688),
    # the frames pass: B T = 128 one-frame clips, forward only
    (401408, 96, 448, 3):      (0, 1, 3, 4, 1, 0, 2, 64, 1, 3136, 256, 57344),
    (402048, 288, 96, 0):      (0, 1, 3, 4, 1, 0, 2, 32, 3, 3141, 256, 32768),
    (402048, 96, 96, 2):       (0, 1, 3, 4, 1, 0, 2, 32, 1, 3141, 256, 32768),
    (402048, 384, 96, 1):      (0, 2, 3, 2, 2, 0, 2, 32, 2, 3141, 256, 40960),
    (402048, 96, 384, 2):      (0, 1, 3, 4, 1, 0, 2, 64, 1, 3141, 256, 57344),
    (402048, 576, 96, 0):      (0, 2, 3, 2, 2, 0, 2, 32, 3, 3141, 256, 40960),
    (402048, 192, 96, 3):      (0, 2, 3, 2, 2, 0, 2, 32, 1, 3141, 256, 40960),
    (100992, 192, 192, 2):     (0, 2, 3, 2, 2, 0, 2, 32, 1, 789, 256, 40960),
    (100992, 768, 192, 1):     (0, 2, 3, 2, 2, 0, 2, 32, 4, 789, 256, 40960),
    (100992, 192, 768, 2):     (0, 1, 3, 4, 1, 0, 2, 64, 2, 789, 256, 57344),
    (100992, 576, 192, 0):     (0, 2, 3, 2, 2, 0, 2, 32, 3, 789, 256, 40960),
    (100992, 1152, 192, 0):    (0, 2, 3, 2, 2, 0, 2, 32, 6, 789, 256, 40960),
    (100992, 384, 192, 3):     (0, 2, 3, 2, 2, 0, 2, 32, 2, 789, 256, 40960),
    (25728, 384, 384, 2):      (0, 1, 3, 4, 1, 0, 2, 64, 4, 201, 256, 57344),
    (25728, 1536, 384, 1):     (0, 2, 3, 2, 2, 0, 2, 32, 8, 201, 256, 40960),
    (25728, 384, 1536, 2):     (1, 2, 3, 2, 2, 4, 3, 64, 2, 201, 512, 122880),
    (25728, 1152, 384, 0):     (0, 2, 2, 2, 2, 0, 2, 32, 9, 201, 256, 32768),
    (25728, 2304, 384, 0):     (0, 2, 3, 2, 2, 0, 2, 32, 12, 201, 256, 40960),
    (25728, 768, 384, 3):      (0, 1, 3, 4, 1, 0, 2, 64, 8, 201, 256, 57344),
    (6912, 768, 768, 2):       (0, 1, 3, 4, 1, 0, 2, 64, 8, 54, 256, 57344),
    (6912, 3072, 768, 1):      (0, 2, 3, 2, 2, 0, 2, 32, 16, 54, 256, 40960),
    (6912, 768, 3072, 2):      (1, 2, 3, 2, 2, 4, 3, 64, 4, 54, 512, 122880),
    (6912, 2304, 768, 0):      (0, 2, 3, 2, 2, 0, 2, 32, 12, 54, 256, 40960),
}
# Under default knobs the kernel names the rule: (family, RB, NB, WM, WN, K-step) -> rule.  (The 128x96 tile with K-step 64 is
# the K-step-64 shortcut: it returns before any tile rule is asked.)  "forced" is the one rule only the knobs reach.
RULE_OF_KERNEL = {(1, 1, 3, 4, 1, 64): "ring_few_long_tiles", (1, 2, 3, 2, 2, 64): "ring_long_k_narrow",
                  (0, 1, 3, 4, 1, 64): "bk64_narrow_long_k", (0, 5, 2, 1, 4, 32): "one_round_160x256",
                  (0, 3, 3, 2, 2, 32): "one_round_192x192", (0, 2, 2, 2, 2, 32): "square_128x128",
                  (0, 2, 3, 2, 2, 32): "big_128x192", (0, 1, 3, 4, 1, 32): "default_128x96"}


@pytest.fixture(scope="module")
def ops():
    import __graft_entry__
    __graft_entry__.build()
    from svit_amd import ops
    return ops


def _step_calls(num_frames, crop, batch, frames_pass=False):
    """(layer, M, N, K, epilogue) of every svit_gemm_nt call for a Linear layer, as Engine.forward / _block_fwd / _block_bwd
    issue them (the frames pass is a no-grad forward of batch * num_frames one-frame clips)"""
    from svit_amd import arch, config
    plan = arch.build_plan(config.ssv2_cfg(num_frames, crop))
    T = 1 if frames_pass else plan.num_frames // plan.patch_stride[0]
    thw = (T, crop // plan.patch_stride[1], crop // plan.patch_stride[2])
    n_obj = (1 if frames_pass else plan.num_frames) * plan.objects
    B = batch * plan.num_frames if frames_pass else batch
    calls = [("patch_embed", B * thw[0] * thw[1] * thw[2], plan.embed_dim, 448, EPI_F32)]
    for blk in plan.blocks:
        sq = blk.stride_q[1]
        q_thw = (thw[0], arch.pooled(thw[1], sq), arch.pooled(thw[2], sq))
        M = B * (1 + thw[0] * thw[1] * thw[2] + n_obj)
        Mq = B * (1 + q_thw[0] * q_thw[1] * q_thw[2] + n_obj)
        C, Co, hid, n = blk.dim_in, blk.dim_out, int(blk.dim_out * plan.mlp_ratio), "blocks.%d." % blk.index
        calls.append((n + "attn.qkv", M, 3 * Co, C, EPI_BF16))
        if blk.has_proj:
            calls.append((n + "proj", M, Co, C, EPI_F32))
        calls += [(n + "attn.proj", Mq, Co, Co, EPI_RESID), (n + "mlp.fc1", Mq, hid, Co, EPI_GELU),
                  (n + "mlp.fc2", Mq, Co, hid, EPI_RESID)]
        if not frames_pass:
            calls += [(n + "mlp.fc2 dgrad", Mq, hid, Co, EPI_DGELU), (n + "mlp.fc1 dgrad", Mq, Co, hid, EPI_BF16),
                      (n + "attn.proj dgrad", Mq, Co, Co, EPI_BF16),
                      (n + "attn.qkv dgrad", M, C, 3 * Co, EPI_F32 if blk.has_proj else EPI_BF16)]
            if blk.has_proj:
                calls.append((n + "proj dgrad", M, C, Co, EPI_F32))
        thw = q_thw
    return calls


def test_choices_of_the_training_step(ops):
    """16x224^2, B = 8, and its frames pass (128 frames): every Linear-layer GEMM runs the kernel, grid, block and LDS size the
    dispatcher chose before the rewrite; the step alone reaches every heuristic rule."""
    step, frames = _step_calls(16, 224, 8), _step_calls(16, 224, 8, frames_pass=True)
    assert len(step) == 1 + 16 * 8 + 3 * 2 and len(frames) == 1 + 16 * 4 + 3      # (three blocks change the width)
    assert step[0][1:4] == (8 * 25088, 96, 448) and step[1][1:4] == (201224, 288, 96) and step[-1][1:4] == (3656, 768, 2304)
    assert {c[1:] for c in step + frames} == set(STEP_CHOICES)
    for layer, M, N, K, epi in step + frames:
        p = ops.gemm_nt_plan(M, N, K, epi)
        want = STEP_CHOICES[(M, N, K, epi)]
        assert (ops.NT_FAMILIES.index(p["family"]),) + tuple(p[f] for f in FIELDS[1:]) == want, layer
        assert p["rule"] == RULE_OF_KERNEL[want[:5] + (want[7],)], layer
    assert {ops.gemm_nt_plan(*c[1:])["rule"] for c in step} == set(RULE_OF_KERNEL.values()) == set(ops.NT_RULES) - {"forced"}


# the tile (rows, columns) a forced configuration names (include/svit_hip.h, svit_debug_set key 1; gemm_reference.FORMS)
TILE_OF_CFG = {0: (128, 192), 2: (128, 96), 4: (128, 128), 5: (128, 192), 6: (128, 96), 7: (128, 128), 9: (160, 256),
               10: (192, 192)}
EPI_OF = {"bf16": EPI_BF16, "gelu": EPI_GELU, "resid": EPI_RESID, "f32": EPI_F32, "dgelu": EPI_DGELU}


@pytest.mark.parametrize("form", list(G.FORMS))
def test_every_named_form_is_the_form_it_names(ops, form):
    """the three knobs of a form of the parity suite select the kernel the form is named after, at every shape and epilogue
    the suite gives it (a forced tile that does not divide N, or a K-step of 64 on K % 64 != 0, would quietly be another)"""
    from svit_amd import hip
    lib, f = hip.load(), G.FORMS[form]
    try:
        assert lib.svit_debug_set(0, f["stages"]) == 0 and lib.svit_debug_set(1, f["cfg"]) == 0
        assert lib.svit_debug_set(2, f["bk"]) == 0
        for shape, lst in G.form_shapes(form):
            for epi in sorted({EPI_OF[kw["epi"]] for kw in lst}):
                p = ops.gemm_nt_plan(*shape, epi)
                where = "%s %s epilogue %d: %s" % (form, shape, epi, p)
                if form == "heuristic":      # what gemm_reference says of its three shapes
                    assert p["rule"] != "forced", where
                    if shape == G.MAIN_SHAPE:
                        assert (p["family"], p["RB"], p["NB"] * p["WN"] * 32, p["stages"], p["BK"]) == ("v2", f["rb"], 96, 2, 64), where
                    elif shape == G.HEURISTIC_SHAPES[0]:
                        assert p["family"] == "v2" and p["BK"] == 32, where            # K % 64 != 0
                    elif shape == G.HEURISTIC_SHAPES[1]:
                        assert p["stages"] == 4, where                                 # the long-K choice
                    continue
                assert p["rule"] == "forced", where
                assert p["family"] == ("ring" if f["cfg"] in (5, 6, 7) else "v2"), where
                assert p["RB"] == f["rb"] == G._RB[f["cfg"]], where
                assert (32 * p["RB"] * p["WM"], 32 * p["NB"] * p["WN"]) == TILE_OF_CFG[f["cfg"]], where
                assert p["stages"] == (f["stages"] or 2), where                        # (the one-round tiles: always 2)
                assert p["BK"] == (64 if p["family"] == "ring" else f["bk"] or 32), where
    finally:
        lib.svit_debug_reset()


MS = (1, 15, 130, 417, 3656, 13064, 50696, 201224)
NS = tuple(range(96, 3072 + 1, 96))
KS = (32, 64, 96, 192, 384, 448, 768, 1536, 2304, 3072)


def test_launch_geometry_holds_its_invariants(ops):
    import ctypes as C
    from svit_amd import hip
    lib, out = hip.load(), (C.c_int32 * 13)()
    seen = set()
    for M, N, K, epi in itertools.product(MS, NS, KS, range(6)):
        assert lib.svit_debug_gemm_nt_plan(M, N, K, epi, out, 13) == 13      # (an error here: a choice without a kernel)
        family, RB, NB, WM, WN, NL, stages, BK, gx, gy, block, lds, rule = out
        where = "%d x %d x %d epilogue %d: %s" % (M, N, K, epi, list(out))
        BM, BN = 32 * RB * WM, 32 * NB * WN
        assert (gx, gy) == (-(-N // BN), -(-M // BM)), where
        assert block == 64 * (WM * WN + NL) and NL == (4 if family else 0) and stages in (2, 3, 4), where
        assert 0 < lds <= LDS_MAX, where
        assert lds >= WM * WN * 16 * (32 * NB + 4) * 4, where                    # the epilogue's staging
        assert lds >= stages * (BM + BN) * BK * 2, where                          # the stages of the main loop
        if family:
            assert K % 64 == 0 and epi != EPI_RELQ and BK == 64, where
        assert BK == 32 or (BK == 64 and K % 64 == 0), where
        assert rule != 0, where                                                   # nothing is forced
        seen.add(ops.NT_RULES[rule])
    assert seen == set(ops.NT_RULES) - {"forced"}


@pytest.mark.parametrize("M,N,K,epi,err", [(0, 96, 32, 0, -2), (128, 0, 32, 0, -2), (128, 96, 0, 0, -2), (128, 96, 48, 0, -2),
                                           (128, 100, 32, 0, -2), (128, 128, 64, 0, -2), (-5, 96, 32, 3, -2),
                                           (128, 96, 32, 6, -4), (128, 96, 32, -1, -4)])
def test_shape_errors_are_the_entry_points(ops, M, N, K, epi, err):
    """SVIT_ERR_SHAPE (-2) for what svit_gemm_nt refuses as a shape, SVIT_ERR_ARG (-4) for an epilogue it has no kernel for"""
    import ctypes as C
    from svit_amd import hip
    out = (C.c_int32 * 13)()
    assert hip.load().svit_debug_gemm_nt_plan(M, N, K, epi, out, 13) == err
    assert hip.load().svit_debug_gemm_nt_plan(128, 96, 32, 0, out, 12) == -4        # room for 13 values is required
    with pytest.raises(hip.SvitHipError):
        ops.gemm_nt_plan(M, N, K, epi)
