"""Input gradients on the GPU: svit_patch_embed_dgrad alone against the float64 restatement and the derived stage bar
(tests/input_grad_cases.py), then the tiny model (4 frames, 64 x 64, batch 2, deterministic mode, no drop): clip.grad,
the bilinear identity with the stem's weight gradient, the chain against the fp32 oracle, bit equalities with the pass
that does not ask, the uint8 routes, stills, the captured step, the frozen cut, the launch lists, FGSM.  Needs a real
MI355X."""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from oracle import procedural as P
from oracle import svit_ref as R
from tests import input_grad_cases as K
from tests import smoke_impl as S

DEV = "cuda"
DGRAD = "svit_patch_embed_dgrad"


def bits(t):
    return t.contiguous().view(torch.int32)


def same(a, b):
    return a.shape == b.shape and torch.equal(bits(a), bits(b))


# ================================================================================================ kernel alone ====
def _run_kernel(dtok, w16, T, H, W, pad):
    """dvideo between two canary zones of `pad` floats, pre-filled with NaN -> (dvideo, canaries intact)"""
    from svit_amd import ops
    n = K.B * 3 * T * H * W
    buf = torch.full((n + 2 * pad,), 12345.0, device=DEV)
    buf[pad:pad + n] = float("nan")
    out = buf[pad:pad + n].view(K.B, 3, T, H, W)
    ops.patch_embed_dgrad(dtok, w16, K.B, T, H, W, out=out)
    torch.cuda.synchronize()
    intact = bool((buf[:pad] == 12345.0).all()) and bool((buf[pad + n:] == 12345.0).all())
    return out.clone(), intact


@pytest.mark.parametrize("T,H,W", K.SHAPES)
def test_kernel_meets_the_stage_bar(T, H, W):
    """(5,17,23): the pixel-by-pixel stores and every border; (1,8,8): T = 1, where only kt = 1 exists; the pad columns
    of w16 hold NaN"""
    from svit_amd.saliency import dgrad_host
    dtok, w16 = K.operands(T, H, W, nan_pad=True)
    d_dev, w_dev = dtok.to(DEV), w16.to(DEV)
    got, intact = _run_kernel(d_dev, w_dev, T, H, W, pad=1024)
    assert intact, "a canary next to dvideo was overwritten"
    assert not bool(torch.isnan(got).any()), "an element of dvideo was not stored (or a pad column was read)"
    ref = dgrad_host(d_dev, w_dev, K.B, T, H, W)            # on the operands the GPU read
    bar = K.stage_bar(dtok, w16, K.B, T, H, W)
    e = K.excess(got, ref, bar)
    print("(%d,%d,%d): max |kernel - dgrad_host| = %.3g x the stage bar" % (T, H, W, e))
    assert e <= 1.0, e
    again, intact = _run_kernel(d_dev, w_dev, T, H, W, pad=1024)
    assert intact and same(got, again), "two runs differ"
    # a base that is only 4-byte aligned takes the pixel-by-pixel stores at any W: the same bits
    odd, intact = _run_kernel(d_dev, w_dev, T, H, W, pad=1023)
    assert intact and same(got, odd)


# ================================================================================================== tiny model ====
def ce(p, e, y):
    return F.cross_entropy(p, y)


def run_step(model, x, y, loss=None, meta=None):
    """zeroed flat gradient, forward, loss, backward -> (logits, loss, flat gradient), detached copies"""
    model.flat.grad.zero_()
    logits, extra = model([x], {} if meta is None else meta)
    ls = F.cross_entropy(logits, y) if loss is None else loss(logits, extra)
    ls.backward()
    torch.cuda.synchronize()
    return logits.detach().clone(), ls.detach().clone(), model.flat.grad.clone()


def build(train=True):
    cfg, model, spec, sd = S.build_hip_model(4, 64, train=train)
    model.engine.deterministic = True
    return cfg, model, spec, sd


class Tiny:
    """one model and, computed once: the step that does not ask, the step whose clip requires grad with the operands
    its launches received, the two launch lists"""

    def __init__(self):
        from svit_amd import ops
        self.cfg, self.model, self.spec, self.sd = build()
        self.x, self.y = P.frames(K.B, 4, 64).to(DEV), P.labels(K.B).to(DEV)
        self.names_plain, self.names_asked = [], []
        with K.launch_names(self.names_plain):
            self.plain = run_step(self.model, self.x, self.y)
        self.clip = self.x.clone().requires_grad_(True)
        self.dgrad_calls, self.cast_calls = [], []
        with K.recording(ops, "patch_embed_dgrad", self.dgrad_calls), K.recording(ops, "scale_cast", self.cast_calls), \
                K.launch_names(self.names_asked):
            self.asked = run_step(self.model, self.clip, self.y)
        self.weight_grad = self.model.flat.g("patch_embed.proj.weight").clone().view(96, 441)


@pytest.fixture(scope="module")
def tiny():
    return Tiny()


def _held_to_the_bar(grad, call, shape5):
    """`grad` against dgrad_host on the operands the recorded launch received"""
    from svit_amd.saliency import dgrad_host
    (dtok, w16, Bn, T, H, W), _, result = call
    assert (Bn, 3, T, H, W) == tuple(shape5)
    assert dtok.dtype == torch.bfloat16 and w16.dtype == torch.bfloat16 and tuple(w16.shape) == (96, 448)
    ref = dgrad_host(dtok, w16, Bn, T, H, W)
    bar = K.stage_bar(dtok.cpu(), w16.cpu(), Bn, T, H, W)
    e = K.excess(grad.reshape(shape5), ref, bar)
    assert e <= 1.0, e
    return ref, e


def test_a_clip_grad_is_the_kernel_s_result_on_the_backward_s_operands(tiny):
    g = tiny.clip.grad
    assert g is not None, "clip.grad is None: the backward stops at the stem"
    assert g.shape == tiny.clip.shape and g.dtype == torch.float32
    assert len(tiny.dgrad_calls) == 1
    _, e = _held_to_the_bar(g, tiny.dgrad_calls[0], tiny.clip.shape)
    print("clip.grad: %.3g x the stage bar; |g| max %.3e" % (e, float(g.abs().max())))
    assert float(g.abs().max()) > 0.0


def test_b_bilinear_identity_with_the_stem_weight_gradient(tiny):
    """<clip.grad, bf16(clip)> = <dW, w16> = <dtok, cols w16^T>.  Bounds, from the operands in float64: an element of
    clip.grad is off by at most the stage bar, so its side by BAR * <dgrad_host(|dtok|, |w|), |clip16|>; an element of
    dW is an fp32 sum over M = B*L rows of exact products, off by at most 2 M 2^-24 sum|dtok cols|, and folded with
    |w16| that is, by the same bilinearity, 2 M 2^-24 <dgrad_host(|dtok|, |w|), |clip16|>."""
    from svit_amd.saliency import dgrad_host
    (dtok, w16, Bn, T, H, W), _, _ = tiny.dgrad_calls[0]
    clip16 = tiny.x.to(torch.bfloat16).double().cpu()
    w = w16.double().cpu()[:, :441]
    exact = float((dgrad_host(dtok, w16, Bn, T, H, W) * clip16).sum())
    mass = float((dgrad_host(dtok.double().abs(), w16.double()[:, :441].abs(), Bn, T, H, W) * clip16.abs()).sum())
    lhs = float((tiny.clip.grad.double().cpu() * clip16).sum())
    rhs = float((tiny.weight_grad.double().cpu() * w).sum())
    M = dtok.shape[0]
    tol_l, tol_r = K.BAR_FACTOR * mass, 2.0 * M * 2.0 ** -24 * mass
    print("<dvideo, clip> %.9e  <dW, w> %.9e  exact %.9e  bounds %.3e / %.3e" % (lhs, rhs, exact, tol_l, tol_r))
    assert abs(lhs - exact) <= tol_l and abs(rhs - exact) <= tol_r
    assert abs(lhs - rhs) <= tol_l + tol_r


def test_c_chain_against_the_fp32_oracle(tiny):
    """1 - c_kernel <= 1.1 (1 - c_chain) + 2e-4 per clip: c_chain is dgrad_host on the chain's fp32 dx rows and the fp32
    weights (no new code in it), c_kernel is clip.grad, both against the oracle's autograd gradient of the same loss"""
    from svit_amd.saliency import dgrad_host
    p = {k: v.clone().requires_grad_(True) for k, v in tiny.sd.items()}
    xr = tiny.x.cpu().clone().requires_grad_(True)
    lg, _ = R.forward(p, tiny.spec, xr, training=True)
    oracle, = torch.autograd.grad(R.video_loss(lg, tiny.y.cpu()), xr)
    L = 2 * 16 * 16
    casts = [c for c in tiny.cast_calls if c[1].get("gather") == (L, 1)]
    assert len(casts) == 1
    dx = casts[0][0][0]                                      # block 0's dx f32 [B, N, 96]
    rows = dx[:, 1:1 + L].reshape(K.B * L, 96)
    chain = dgrad_host(rows, tiny.sd["patch_embed.proj.weight"].reshape(96, 441), K.B, 4, 64, 64)
    for b in range(K.B):
        c_chain, c_kernel = S.cosine(chain[b], oracle[b]), S.cosine(tiny.clip.grad[b], oracle[b])
        print("clip %d: c_chain %.6f  c_kernel %.6f" % (b, c_chain, c_kernel))
        assert 1.0 - c_kernel <= 1.1 * (1.0 - c_chain) + S.YARD_FLOOR, (b, c_chain, c_kernel)


def test_d_asking_changes_nothing_else(tiny):
    for a, b, what in zip(tiny.plain, tiny.asked, ("logits", "loss", "flat gradient")):
        assert same(a, b), what


def _u8_inputs():
    from svit_amd.augment import AugClips, AugRecord
    from svit_amd.input import U8Clips
    g = torch.Generator().manual_seed(5)
    u8 = torch.randint(0, 256, (2, 4, 80, 96, 3), generator=g, dtype=torch.uint8).to(DEV)
    plain = U8Clips(u8, 64, torch.tensor([[0, 3, 5], [1, 16, 32]], dtype=torch.int32))
    recs = [AugRecord(0, 4, 8, 60, 72, 70, 80, 3, 9, 1, 1, 10, 12, 20, 16, 7),       # resize, flip, const erase
            AugRecord(1, 0, 0, 80, 96, 72, 90, 5, 20, 0, 2, 5, 5, 10, 10, 11)]       # resize, rand erase
    return plain, AugClips(u8, 64, recs)


def test_e_uint8_routes_equal_the_fp32_route_fed_their_render(tiny):
    from svit_amd.saliency import input_gradient
    for clips in _u8_inputs():
        got = input_gradient(tiny.model, clips, labels=tiny.y)
        assert float(tiny.model.flat.grad.abs().max()) == 0.0       # zeroed on exit
        assert tiny.model.last_input_grad is None
        want = input_gradient(tiny.model, clips.render(), labels=tiny.y)
        assert tuple(got.shape) == (K.B, 3, 4, 64, 64) and got.dtype == torch.float32
        assert float(got.abs().max()) > 0.0
        assert same(got, want), type(clips).__name__


def test_f_stills_with_the_image_rank_loss(tiny):
    from svit_amd import losses, ops
    meta = {k: v.to(DEV) for k, v in P.haog_meta(K.B).items()}
    fn = losses.VideoImageLoss(tiny.cfg, is_video_rank=False)
    still = P.frames(K.B, 1, 64).to(DEV).requires_grad_(True)
    calls = []
    with K.recording(ops, "patch_embed_dgrad", calls):
        run_step(tiny.model, still, None, loss=lambda p, e: fn.total(fn(p, e, None, meta)), meta=meta)
    assert still.grad is not None and still.grad.shape == still.shape
    assert len(calls) == 1 and calls[0][0][3] == 1               # T = 1
    _held_to_the_bar(still.grad, calls[0], still.shape)
    assert float(still.grad.abs().max()) > 0.0
    flat = P.frames(K.B, 1, 64).to(DEV)[:, :, 0].contiguous().requires_grad_(True)     # [B,3,S,S], as the engine unsqueezes
    run_step(tiny.model, flat, None, loss=lambda p, e: fn.total(fn(p, e, None, meta)), meta=meta)
    assert flat.grad.shape == flat.shape and same(flat.grad.unsqueeze(2), still.grad)


class Graphed:
    def __init__(self):
        from svit_amd.graph import GraphedTrainStep
        _, self.model, _, _ = build()
        self.x, self.y = P.frames(K.B, 4, 64).to(DEV), P.labels(K.B).to(DEV)
        self.names_bare, self.names_asked = [], []
        with K.launch_names(self.names_bare):
            self.bare = GraphedTrainStep(self.model, ce, [self.x], self.y)
        with K.launch_names(self.names_asked):
            self.step = GraphedTrainStep(self.model, ce, [self.x], self.y, input_grad=True)


@pytest.fixture(scope="module")
def graphed():
    return Graphed()


def test_g_captured_step_equals_the_eager_step(graphed):
    step, model = graphed.step, graphed.model
    assert graphed.bare.input_grad is None
    assert tuple(step.input_grad.shape) == (K.B, 3, 4, 64, 64) and step.input_grad.dtype == torch.float32
    static = step.input_grad
    for i in (1, 2):
        x = P.frames(K.B, 4, 64, tag="replay%d" % i).to(DEV)
        y = P.labels(K.B, tag="replay%d" % i).to(DEV)
        loss, _ = step([x], y)
        torch.cuda.synchronize()
        assert step.input_grad is static
        got = (static.clone(), loss.clone(), model.flat.grad.clone())
        clip = x.clone().requires_grad_(True)
        _, eager_loss, eager_flat = run_step(model, clip, y)
        assert same(got[0], clip.grad), "input_grad of replay %d" % i
        assert same(got[1], eager_loss) and same(got[2], eager_flat)
        assert float(clip.grad.abs().max()) > 0.0


def test_h_frozen_cut():
    from svit_amd.graph import GraphedTrainStep
    from svit_amd import hip
    from svit_amd.saliency import input_gradient
    _, model, _, _ = build()
    model.freeze_below(4)
    x, y = P.frames(K.B, 4, 64).to(DEV), P.labels(K.B).to(DEV)
    clip = x.clone().requires_grad_(True)
    run_step(model, clip, y)
    assert clip.grad is None
    with pytest.raises(ValueError, match="frozen cut"):
        input_gradient(model, x, labels=y)
    with pytest.raises(ValueError, match="frozen cut"):
        model([x], {}, input_grad=True)
    with pytest.raises(hip.SvitHipError, match="frozen cut"):
        GraphedTrainStep(model, ce, [x], y, input_grad=True)


def _without(names):
    return [n for n in names if n != DGRAD]


def test_i_without_the_request_not_one_launch_more(tiny, graphed):
    """the pass and the capture that do not ask never launch the kernel; asking adds exactly that launch, directly
    behind the cast that makes its operand, and moves nothing else"""
    assert DGRAD not in tiny.names_plain and DGRAD not in graphed.names_bare
    assert tiny.names_asked.count(DGRAD) == 1
    assert _without(tiny.names_asked) == tiny.names_plain
    assert tiny.names_asked[tiny.names_asked.index(DGRAD) - 1] == "svit_scale_cast"
    runs = graphed.names_asked.count(DGRAD)
    assert runs == 3                                             # two warm-up runs of the body and the captured one
    assert _without(graphed.names_asked) == graphed.names_bare
    assert all(graphed.names_asked[i - 1] == "svit_scale_cast" for i, n in enumerate(graphed.names_asked) if n == DGRAD)
    assert graphed.step.n_graphs == graphed.bare.n_graphs


def test_j_fgsm_moves_the_scalar_to_first_order():
    """eval mode, default scalar s (the sum of each sample's largest class probability): x - eps sign(g) moves s by
    -eps |g|_1 to first order; asserted within 50 % at eps = 1e-3 of the clip's range"""
    from svit_amd.saliency import fgsm, input_gradient, saliency_map
    _, model, _, _ = build(train=False)
    x = P.frames(K.B, 4, 64).to(DEV)

    def scalar(clip):
        with torch.no_grad():
            preds, _ = model([clip], {})
        return float(preds.double().max(dim=1).values.sum())

    g = input_gradient(model, x)
    m = saliency_map(g)
    assert tuple(m.shape) == (K.B, 4, 64, 64)
    assert bool(torch.isfinite(g).all()) and float(m.max()) > 0.0
    eps = 1e-3 * float(x.max() - x.min())
    s0, s1 = scalar(x), scalar(fgsm(x, g, -eps))
    first_order = eps * float(g.double().abs().sum())
    print("s %.9f -> %.9f: moved %.4e, first order -%.4e" % (s0, s1, s1 - s0, first_order))
    assert s1 < s0
    assert abs((s1 - s0) + first_order) <= 0.5 * first_order
