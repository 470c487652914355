"""Input gradients without a GPU: the float64 restatement against autograd, mutants of it against the derived stage
bar, the entry point's argument refusals, the refusals under a frozen cut, and the plain-torch helpers."""
import ctypes as C

import pytest
import torch
import torch.nn.functional as F

from tests import input_grad_cases as K

ERR_SHAPE, ERR_ALIGN, ERR_ARG = -2, -3, -4


@pytest.mark.parametrize("T,H,W", K.SHAPES)
def test_dgrad_host_is_the_data_gradient_of_the_conv(T, H, W):
    """dgrad_host against float64 autograd of F.conv3d, to 1e-12 relative"""
    from svit_amd.saliency import dgrad_host
    g = torch.Generator().manual_seed(T * 10000 + H * 100 + W)
    To, Ho, Wo = K.out_dims(T, H, W)
    x = torch.randn((K.B, 3, T, H, W), generator=g, dtype=torch.float64, requires_grad=True)
    w = torch.randn((96, 3, 3, 7, 7), generator=g, dtype=torch.float64)
    dy = torch.randn((K.B, 96, To, Ho, Wo), generator=g, dtype=torch.float64)
    y = F.conv3d(x, w, stride=(2, 4, 4), padding=(1, 3, 3))
    assert tuple(y.shape) == tuple(dy.shape)
    want, = torch.autograd.grad(y, x, dy)
    dtok = dy.permute(0, 2, 3, 4, 1).reshape(-1, 96)
    w448 = torch.full((96, 448), float("nan"), dtype=torch.float64)      # the pad columns are never read
    w448[:, :441] = w.reshape(96, 441)
    got = dgrad_host(dtok, w448, K.B, T, H, W)
    assert got.dtype == torch.float64 and tuple(got.shape) == (K.B, 3, T, H, W)
    assert float((got - want).abs().max()) <= 1e-12 * float(want.abs().max())


@pytest.mark.parametrize("T,H,W", K.SHAPES)
def test_mutants_of_the_restatement_land_far_above_the_stage_bar(T, H, W):
    """what the bar is worth: each mistake is >= 10 x the bar away from dgrad_host on every shape where the mistake can
    exist -- with T <= 2 no input frame has a second temporal neighbour (To = 1), so that mutant IS the restatement
    there, which is asserted instead"""
    from svit_amd.saliency import dgrad_host
    dtok, w = K.operands(T, H, W, nan_pad=False)
    ref = dgrad_host(dtok, w, K.B, T, H, W)
    bar = K.stage_bar(dtok, w, K.B, T, H, W)
    for mutant in K.MUTANTS:
        got = K.dgrad_mutant(dtok, w, K.B, T, H, W, mutant)
        e = K.excess(got, ref, bar)
        print("(%d,%d,%d) %-18s %.3g x the stage bar" % (T, H, W, mutant, e))
        if mutant == "second_t_dropped" and T <= 2:
            assert e <= 1e-3, (mutant, e)
        else:
            assert e >= 10.0, (mutant, e)


def test_the_unmutated_pixel_loop_is_the_restatement():
    """the mutants' pixel loop with no mistake would be dgrad_host: checked through the one mutant that is the identity
    on a T = 1 shape, far inside the bar"""
    from svit_amd.saliency import dgrad_host
    T, H, W = 1, 8, 8
    dtok, w = K.operands(T, H, W)
    ref = dgrad_host(dtok, w, K.B, T, H, W)
    got = K.dgrad_mutant(dtok, w, K.B, T, H, W, "second_t_dropped")
    assert K.excess(got, ref, K.stage_bar(dtok, w, K.B, T, H, W)) <= 1e-3


def test_entry_point_refuses_bad_arguments_before_any_hip_call():
    import __graft_entry__
    __graft_entry__.build()
    from svit_amd import hip
    fn = hip.load().svit_patch_embed_dgrad
    P_ = 1 << 20

    def call(dtok=P_, w=P_, out=P_, B=2, T=4, H=64, W=64):
        return fn(dtok, w, out, B, T, H, W, None)

    assert call(dtok=None) == ERR_ARG
    assert call(w=None) == ERR_ARG
    assert call(out=None) == ERR_ARG
    for k in ("B", "T", "H", "W"):
        assert call(**{k: 0}) == ERR_ARG and call(**{k: -3}) == ERR_ARG
    assert call(dtok=P_ + 8) == ERR_ALIGN               # the operands are read in 16-byte pieces
    assert call(w=P_ + 2) == ERR_ALIGN
    assert call(out=P_ + 2) == ERR_ALIGN                # fp32 elements
    # B * To * Ho * Wo = 2^31 exactly: 2^10 * 2^7 * 2^7 * 2^7 rows
    assert call(B=1 << 10, T=(1 << 8) - 1, H=1 << 9, W=1 << 9) == ERR_SHAPE
    assert "svit_patch_embed_dgrad" in hip.EXPORTS


def test_engine_forward_refuses_the_request_under_a_cut():
    from svit_amd.engine import Engine
    from svit_amd.input import FramesView
    eng = Engine.__new__(Engine)            # the refusals come before anything of the engine is touched
    with pytest.raises(ValueError, match=r"frozen cut \(cut 3\)"):
        eng.forward(torch.zeros(1, 3, 4, 64, 64), save=True, cut=3, input_grad=True)
    with pytest.raises(ValueError, match="FramesView"):
        eng.forward(FramesView.__new__(FramesView), save=True, cut=0, input_grad=True)
    with pytest.raises(ValueError, match="saving forward"):
        eng.forward(torch.zeros(1, 3, 4, 64, 64), save=False, cut=0, input_grad=True)


def test_graphed_step_refuses_the_request_under_a_cut():
    from svit_amd import graph, hip
    graph._check_input_grad(0)
    with pytest.raises(hip.SvitHipError, match=r"input_grad=True\) under a frozen cut .*below position 5"):
        graph._check_input_grad(5)


def test_input_gradient_refuses_a_frozen_model():
    from svit_amd import config, saliency
    from svit_amd.model import MODEL_REGISTRY
    model = MODEL_REGISTRY.get("SViT")(config.ssv2_cfg(num_frames=4, crop=64))
    model.freeze_below(4)
    with pytest.raises(ValueError, match="frozen cut .*below position 4"):
        saliency.input_gradient(model, torch.zeros(1, 3, 4, 64, 64))
    with pytest.raises(ValueError, match="no-grad pass"):
        with torch.no_grad():
            model.engine = object()     # (past the "no CPU path" refusal: the request is checked before any launch)
            model([torch.zeros(1, 3, 4, 64, 64)], input_grad=True)


def test_saliency_helpers_on_hand_made_tensors():
    from svit_amd import saliency
    g = torch.zeros(1, 3, 2, 2, 2)
    g[0, 0, 0, 0, 0], g[0, 1, 0, 0, 0], g[0, 2, 0, 0, 0] = 1.0, -3.0, 2.0
    g[0, 2, 1, 1, 0] = -0.5
    m = saliency.saliency_map(g)
    assert tuple(m.shape) == (1, 2, 2, 2)
    assert float(m[0, 0, 0, 0]) == 3.0 and float(m[0, 1, 1, 0]) == 0.5 and float(m.sum()) == 3.5
    with pytest.raises(ValueError):
        saliency.saliency_map(g[:, :2])
    clip = torch.arange(24, dtype=torch.float32).reshape(1, 3, 2, 2, 2)
    gi = saliency.grad_times_input(g, clip)
    assert torch.equal(gi, g * clip) and float(gi[0, 1, 0, 0, 0]) == -3.0 * 8.0
    still = torch.ones(1, 3, 2, 2)
    assert tuple(saliency.grad_times_input(g[:, :, :1], still).shape) == (1, 3, 1, 2, 2)
    with pytest.raises(ValueError):
        saliency.grad_times_input(g, clip[:, :, :1])
    adv = saliency.fgsm(clip, g, 0.25)
    want = clip.clone()
    want[0, 0, 0, 0, 0] += 0.25
    want[0, 1, 0, 0, 0] -= 0.25
    want[0, 2, 0, 0, 0] += 0.25
    want[0, 2, 1, 1, 0] -= 0.25
    assert torch.equal(adv, want)                       # sign(0) = 0: untouched where the gradient is zero
    g4 = torch.ones(1, 3, 1, 2, 2)
    assert tuple(saliency.fgsm(still, g4, 0.5).shape) == (1, 3, 2, 2)
