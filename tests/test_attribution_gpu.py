"""Attribution passes on the GPU: the two kernels of csrc/attrib.hip against their torch-CPU restatements bit for bit
(NaN canaries around every output, base pointers at +0 and +1 float), the noise against the erasing noise of
AugClips.render(), then the tiny model of tests/test_input_grad_gpu.py (4 frames, 64 x 64, batch 2): the
input-gradient-only pass leaves the training state alone and equals the full pass bit for bit, the launch lists, the
frozen cut, and SmoothGrad / integrated gradients against the chain of restatements.  No tolerance anywhere.  Needs a
real MI355X."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import procedural as P
from tests import input_grad_cases as K
from tests import smoke_impl as S

DEV = "cuda"
PAD = 64
SHAPES = [(1, 3, 1, 3, 5), (2, 3, 2, 8, 8), (2, 3, 4, 64, 64)]       # all head / tail; the vector body; the tiny model's
OFFSETS = [(0, 0, 0), (1, 1, 1), (1, 0, 0)]                           # floats in front of (out, x, base)


def bits(t):
    return t.contiguous().view(torch.int32)


def same(a, b):
    return a.shape == b.shape and torch.equal(bits(a.cpu()), bits(b.cpu()))


def record(alpha=1.0, weight=1.0, seed=0, k=0, squared=False):
    from svit_amd.attribution import pack_record
    return torch.frombuffer(bytearray(pack_record(alpha, weight, seed, k, squared)), dtype=torch.int32).to(DEV)


def guarded(shape, off):
    """a tensor of `shape`, `off` floats past a 16-byte boundary, between two zones of NaN canaries -> (buffer, view)"""
    n = int(torch.Size(shape).numel())
    buf = torch.full((n + 2 * PAD + 4,), float("nan"), device=DEV)
    assert buf.data_ptr() % 16 == 0
    return buf, buf[PAD + off:PAD + off + n].view(shape)


def intact(buf, view):
    lo = (view.data_ptr() - buf.data_ptr()) // 4
    return bool(torch.isnan(buf[:lo]).all()) and bool(torch.isnan(buf[lo + view.numel():]).all())


def placed(t, off):
    """a copy of `t` on the device whose base pointer sits `off` floats past a 16-byte boundary"""
    buf = torch.empty(t.numel() + 4, device=DEV)
    v = buf[off:off + t.numel()].view(t.shape)
    v.copy_(t)
    return v


def operand(shape, tag):
    g = torch.Generator().manual_seed(sum(shape) * 131 + len(tag) * 7 + ord(tag[0]))
    return torch.randn(shape, generator=g)


_noise = {}


def noise_field(B, T, H, W, seed):
    """the erasing noise, f32 [B,3,T,H,W] on the host: AugClips.render() of clips whose records erase the whole W x W
    window in pixel mode with this seed (the first H rows: the counter is y*W + x)"""
    key = (B, T, H, W, seed)
    if key not in _noise:
        from svit_amd.augment import AugClips, AugRecord
        assert H <= W
        u8 = torch.zeros((B, T, W, W, 3), dtype=torch.uint8, device=DEV)
        recs = [AugRecord(b, 0, 0, W, W, W, W, 0, 0, 0, 3, 0, 0, W, W, seed) for b in range(B)]
        _noise[key] = AugClips(u8, W, recs).render()[:, :, :, :H].contiguous().cpu()
    return _noise[key]


# ==================================================================================================== the kernels ====
@pytest.mark.parametrize("shape", SHAPES)
def test_perturb_equals_the_restatement(shape):
    from svit_amd import ops
    from svit_amd.attribution import perturb_host
    B, _, T, H, W = shape
    x, base = operand(shape, "x"), operand(shape, "base")
    sig = torch.tensor([0.5, 2.0][:B])
    seed = 1234567
    noise = noise_field(B, T, H, W, seed)
    for o_out, o_x, o_base in OFFSETS:
        xd, bd, sd = placed(x, o_x), placed(base, o_base), sig.to(DEV)
        for with_base in (True, False):
            for alpha in (0.0, 0.3, 1.0):
                for noisy in (False, True):
                    buf, out = guarded(shape, o_out)
                    ops.attr_perturb(xd, record(alpha=alpha, seed=seed), base=bd if with_base else None,
                                     sigma=sd if noisy else None, out=out)
                    torch.cuda.synchronize()
                    what = (shape, (o_out, o_x, o_base), with_base, alpha, noisy)
                    assert intact(buf, out), what
                    want = perturb_host(x, base if with_base else None, alpha, sig if noisy else None, noise)
                    assert same(out, want), what
    assert not same(perturb_host(x, base, 0.3, None, None), x)         # (an alpha for which the path does not end at x)


def test_the_noise_is_the_erasing_noise():
    from svit_amd import ops
    B, T, S = 2, 2, 8
    zero, one = torch.zeros((B, 3, T, S, S), device=DEV), torch.ones(B, device=DEV)
    a = ops.attr_perturb(zero, record(seed=77), sigma=one)
    assert same(a, noise_field(B, T, S, S, 77))
    assert same(ops.attr_perturb(zero, record(seed=77), sigma=one), a)          # the same record twice
    b = ops.attr_perturb(zero, record(seed=78), sigma=one)
    assert same(b, noise_field(B, T, S, S, 78)) and not same(a, b)
    big = ops.attr_perturb(torch.zeros((2, 3, 4, 64, 64), device=DEV), record(seed=5), sigma=one)
    assert float(big.abs().max()) <= 5.77 and float(big.std()) > 0.9


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("squared", [False, True])
def test_accumulate_equals_the_restatement(shape, squared):
    from svit_amd import ops
    from svit_amd.attribution import accumulate_host
    B, rows = shape[0], 3
    gs = [operand(shape, "g%d" % k) for k in range(4)]
    gs[0].view(-1)[1] = -0.0
    sc = [operand((B,), "s%d" % k) for k in range(4)]
    weights = (0.25, 1.0 / 3.0, 0.7, 0.5)
    for o_acc, o_g, _ in OFFSETS:
        runs = []
        for _ in range(2):
            buf, acc = guarded(shape, o_acc)
            sbuf, table = guarded((rows, B), 0)
            want = None
            for k in range(3):
                ops.attr_accumulate(placed(gs[k], o_g), acc, record(weight=weights[k], k=k, squared=squared),
                                    sc[k].to(DEV), table)
                want = accumulate_host(want, gs[k], weights[k], squared, k == 0)
            torch.cuda.synchronize()
            assert intact(buf, acc) and intact(sbuf, table), (shape, o_acc, o_g)
            assert same(acc, want), (shape, o_acc, o_g)
            assert same(table, torch.stack(sc[:3]))
            # a record whose pass number is `rows` writes no score: the table and its canaries stay
            ops.attr_accumulate(placed(gs[3], o_g), acc, record(weight=weights[3], k=rows, squared=squared),
                                sc[3].to(DEV), table)
            torch.cuda.synchronize()
            assert intact(sbuf, table) and same(table, torch.stack(sc[:3])) and intact(buf, acc)
            assert same(acc, accumulate_host(want, gs[3], weights[3], squared, False))
            runs.append(acc.clone())
        assert same(runs[0], runs[1])
    if not squared:     # the first pass stores: -0.0 survives a weight of 1
        buf, acc = guarded(shape, 0)
        ops.attr_accumulate(gs[0].to(DEV), acc, record())
        assert same(acc, gs[0])


# ===================================================================================================== tiny model ====
def ce(p, e, y):
    return torch.nn.functional.cross_entropy(p, y)


def build(train=True, deterministic=True, drop=False):
    cfg, model, spec, sd = S.build_hip_model(4, 64, drop=drop, train=train)
    model.engine.deterministic = deterministic
    return cfg, model


def clip(tag="clip"):
    return P.frames(K.B, 4, 64, tag=tag).to(DEV)


def labels():
    return P.labels(K.B).to(DEV)


def u8_inputs():
    from svit_amd.augment import AugClips, AugRecord
    from svit_amd.input import U8Clips
    g = torch.Generator().manual_seed(5)
    u8 = torch.randint(0, 256, (2, 4, 80, 96, 3), generator=g, dtype=torch.uint8).to(DEV)
    plain = U8Clips(u8, 64, torch.tensor([[0, 3, 5], [1, 16, 32]], dtype=torch.int32))
    recs = [AugRecord(0, 4, 8, 60, 72, 70, 80, 3, 9, 1, 1, 10, 12, 20, 16, 7),       # resize, flip, const erase
            AugRecord(1, 0, 0, 80, 96, 72, 90, 5, 20, 0, 2, 5, 5, 10, 10, 11)]       # resize, rand erase
    return plain, AugClips(u8, 64, recs)


def one_pass(model, x, y, mode, loss=None, meta=None):
    """forward(input_grad=mode), loss, backward -> last_input_grad (a copy)"""
    preds, extra = model([x], {} if meta is None else meta, input_grad=mode)
    (ce(preds, extra, y) if loss is None else loss(preds, extra)).backward()
    torch.cuda.synchronize()
    g = model.last_input_grad.clone()
    model.last_input_grad = None
    return g


def training_state(model, opt=None):
    s = {"grad": model.flat.grad.clone(), "data": model.flat.data.clone(),
         "rng": None if model._rng_state is None else model._rng_state.clone(),
         "torch_rng": torch.cuda.get_rng_state(), "ids": [id(p.grad) for p in model.parameters()]}
    if opt is not None:
        s["m"], s["v"] = opt.exp_avg.clone(), opt.exp_avg_sq.clone()
    return s


def assert_state_unchanged(model, before, opt=None):
    now = training_state(model, opt)
    assert now["ids"] == before["ids"], "a param.grad changed identity"
    for k in before:
        if k not in ("ids", "rng"):
            assert torch.equal(bits(now[k]) if now[k].dtype == torch.float32 else now[k],
                               bits(before[k]) if before[k].dtype == torch.float32 else before[k]), k
    assert (before["rng"] is None) == (now["rng"] is None)
    if before["rng"] is not None:
        assert torch.equal(before["rng"], now["rng"])


def pending_gradient(model, x, y):
    """a training backward whose gradient is left pending, then overwritten by a finite pattern"""
    model.flat.grad.zero_()
    preds, extra = model([x], {})
    ce(preds, extra, y).backward()
    n = model.flat.grad.numel()
    model.flat.grad.copy_(torch.arange(n, device=DEV, dtype=torch.float32).mul_(1e-3).sin_())


@pytest.mark.parametrize("drop", [False, True])
def test_a_the_only_pass_leaves_the_training_state_alone(drop):
    """fails on a tree without input_grad="only": the forward refuses the value"""
    from svit_amd import actmon, optim
    from svit_amd.graph import GraphedTrainStep
    cfg, model = build(drop=drop)
    opt = optim.GuardedClipAdamW(model, lr=1e-3)
    x, y = clip(), labels()
    pending_gradient(model, x, y)       # (with drop: the draw counter now exists)
    mon = actmon.ActivationMonitor(model, 4)
    model.attach_activation_monitor(mon)
    none_before = [p.grad is None for p in model.parameters()]
    before, ring = training_state(model, opt), mon.ring.clone()
    g = one_pass(model, x, y, "only")
    assert tuple(g.shape) == (K.B, 3, 4, 64, 64) and float(g.abs().max()) > 0.0
    assert_state_unchanged(model, before, opt)
    assert torch.equal(mon.ring, ring)
    step = GraphedTrainStep(model, ce, [x], y, input_grad="only")
    assert step.n_graphs == 1
    for i in range(3):
        step([clip("replay%d" % i)], y)
    torch.cuda.synchronize()
    assert_state_unchanged(model, before, opt)
    assert torch.equal(mon.ring, ring)
    assert [p.grad is None for p in model.parameters()] == none_before
    if not drop:
        assert same(step.input_grad, one_pass(model, clip("replay2"), y, "only"))


def test_a2_none_grads_stay_none():
    _, model = build()
    x, y = clip(), labels()
    assert all(p.grad is None for p in model.parameters())
    flat = model.flat.grad.clone()
    one_pass(model, x, y, "only")
    assert all(p.grad is None for p in model.parameters())
    assert torch.equal(bits(model.flat.grad), bits(flat))
    model.eval()        # the ATen head on detached weights
    one_pass(model, x, y, "only")
    assert all(p.grad is None for p in model.parameters())
    model.train()
    model.fused_head = False
    one_pass(model, x, y, "only")
    assert all(p.grad is None for p in model.parameters())


@pytest.mark.parametrize("deterministic", [True, False])
def test_b_only_equals_the_full_pass(deterministic):
    from svit_amd import losses
    cfg, model = build(deterministic=deterministic)
    y = labels()
    for x in (clip(),) + u8_inputs():
        full = one_pass(model, x, y, True)
        assert same(one_pass(model, x, y, "only"), full), type(x).__name__
        assert float(full.abs().max()) > 0.0
    meta = {k: v.to(DEV) for k, v in P.haog_meta(K.B).items()}
    fn = losses.VideoImageLoss(cfg, is_video_rank=False)
    still = P.frames(K.B, 1, 64).to(DEV)
    haog = lambda p, e: fn.total(fn(p, e, None, meta))
    full = one_pass(model, still, None, True, loss=haog, meta=meta)
    assert tuple(full.shape) == (K.B, 3, 1, 64, 64)
    assert same(one_pass(model, still, None, "only", loss=haog, meta=meta), full)


def test_c_launch_lists():
    _, model = build()
    x, y = clip(), labels()
    lists = {}
    for mode in (False, True, "only"):
        model.flat.grad.zero_()
        with K.launch_names(lists.setdefault(mode, [])):
            preds, extra = model([x], {}, input_grad=mode)
            ce(preds, extra, y).backward()
        torch.cuda.synchronize()
    plain, asked, only = lists[False], lists[True], lists["only"]
    dgrad = "svit_patch_embed_dgrad"
    assert not [n for n in only if n.startswith("svit_gemm_tn")] and "svit_special_token_grads" not in only
    assert only.count(dgrad) == 1 and asked.count(dgrad) == 1 and dgrad not in plain
    assert [n for n in asked if n != dgrad] == plain
    # the data-gradient chain: the full pass's launches in the full pass's order, minus the parameter-gradient ones
    assert only == [n for n in asked if not n.startswith("svit_gemm_tn") and n != "svit_special_token_grads"]
    assert any(n.startswith("svit_gemm_tn") for n in plain) and "svit_special_token_grads" in plain


@pytest.mark.parametrize("cut", [4, "head"])
def test_d_frozen_cut(cut):
    from svit_amd import hip
    from svit_amd.graph import GraphedTrainStep
    from svit_amd.saliency import input_gradient
    _, model = build()
    x, y = clip(), labels()
    free = one_pass(model, x, y, "only")
    model.freeze_below(len(model.plan.blocks) + 2 if cut == "head" else cut)
    flags = [p.requires_grad for p in model.parameters()]
    assert not all(flags)
    assert same(one_pass(model, x, y, "only"), free)
    assert same(input_gradient(model, x, scalar=lambda p, e: ce(p, e, y), param_grads=False), free)
    step = GraphedTrainStep(model, ce, [x], y, input_grad="only")
    step([x], y)
    torch.cuda.synchronize()
    assert same(step.input_grad, free)
    assert [p.requires_grad for p in model.parameters()] == flags
    with pytest.raises(ValueError, match="frozen cut"):
        model([x], {}, input_grad=True)
    with pytest.raises(ValueError, match="frozen cut"):
        input_gradient(model, x, labels=y)
    with pytest.raises(hip.SvitHipError, match="frozen cut"):
        GraphedTrainStep(model, ce, [x], y, input_grad=True)


class Attributed:
    """one model, one captured Attribution with a given target, and the parent's route to the same numbers"""

    def __init__(self):
        from svit_amd.attribution import Attribution
        _, self.model = build()
        self.x = clip()
        self.target = torch.tensor([3, 170], device=DEV)
        self.attr = Attribution(self.model, self.x, target=self.target)
        self.logits = []

    def scalar(self, preds, extra):
        s = preds.gather(1, self.target[:, None]).squeeze(1)
        self.logits.append(s.detach().clone())
        return s.sum()

    def full_route(self, x):
        """saliency.input_gradient on the full backward (the route of the parent commit), model in train mode"""
        from svit_amd.saliency import input_gradient
        assert self.model.training
        return input_gradient(self.model, x, scalar=self.scalar).clone()


@pytest.fixture(scope="module")
def attributed():
    return Attributed()


def test_e_gradient(attributed):
    from svit_amd import attribution
    a = attributed
    assert a.model.training
    got = a.attr.gradient()
    assert same(got, a.full_route(a.x)) and float(got.abs().max()) > 0.0
    for tag in ("second", "third"):
        x = clip(tag)
        a.attr.set_clip(x, target=a.target)
        assert same(a.attr.gradient(), attribution.gradient(a.model, x, target=a.target)), tag
    a.attr.set_clip(a.x, target=a.target)
    a.model.eval()          # the eager twin restores the mode it found
    attribution.gradient(a.model, a.x, target=a.target)
    assert not a.model.training
    a.model.train()


@pytest.mark.parametrize("squared", [False, True])
def test_f_smoothgrad(attributed, squared):
    from svit_amd.attribution import accumulate_host, passes, perturb_host
    a = attributed
    sigma = torch.tensor([0.5, 2.0])
    got = a.attr.smoothgrad(n=3, sigma=sigma, squared=squared, seed=2 ** 31 - 2).clone()      # (the seeds wrap)
    want = None
    for k, (alpha, weight, seed) in enumerate(passes("smoothgrad", 3, 2 ** 31 - 2)):
        noisy = perturb_host(a.x.cpu(), None, alpha, sigma, noise_field(K.B, 4, 64, 64, seed))
        want = accumulate_host(want, a.full_route(noisy.to(DEV)).cpu(), weight, squared, k == 0)
    assert same(got, want)
    assert float(got.abs().max()) > 0.0


def test_g_integrated_gradients(attributed):
    from svit_amd import attribution
    from svit_amd.attribution import accumulate_host, completeness, passes, perturb_host
    a = attributed
    base = 0.1 * clip("baseline")
    attr, delta = a.attr.integrated_gradients(steps=2, baseline=base)
    want, a.logits = None, []
    for k, (alpha, weight, _) in enumerate(passes("integrated_gradients", 2)):
        point = perturb_host(a.x.cpu(), base.cpu(), alpha, None, None)
        want = accumulate_host(want, a.full_route(point.to(DEV)).cpu(), weight, False, k == 0)
    assert same(a.attr.acc, want)
    table = torch.stack(a.logits)
    assert same(a.attr.scores, table)
    assert same(attr, a.attr.acc * (a.x - base))
    formula = attr.double().flatten(1).sum(1).cpu() - (table[2].double() - table[0].double()).cpu()
    assert torch.equal(delta.cpu(), formula) and torch.equal(delta, completeness(attr, a.attr.scores, 2))
    assert delta.dtype == torch.float64 and bool(torch.isfinite(delta).all())
    twin, twin_delta = attribution.integrated_gradients(a.model, a.x, target=a.target, steps=2, baseline=base)
    assert same(twin, attr) and torch.equal(twin_delta, delta)


def test_h_nothing_is_drawn_and_refresh_sees_new_weights():
    from svit_amd import attribution, optim
    from svit_amd.attribution import Attribution
    x, y = clip(), labels()
    target = torch.tensor([3, 170], device=DEV)
    _, calm = build(drop=False)
    _, model = build(drop=True)
    assert any(b.drop_path > 0 for b in model.plan.blocks)
    pending_gradient(model, x, y)                 # (a training pass: the draw counter exists from here on)
    before = training_state(model)
    attr = Attribution(model, x, target=target)
    g0 = attr.gradient().clone()
    assert same(g0, Attribution(calm, x, target=target).gradient())
    assert_state_unchanged(model, before)
    opt = optim.GuardedClipAdamW(model, lr=1e-2)
    model.flat.grad.zero_()
    preds, extra = model([x], {})
    ce(preds, extra, y).backward()
    opt.step()
    attr.refresh()
    g1 = attr.gradient().clone()
    assert not same(g1, g0)
    assert same(g1, attribution.gradient(model, x, target=target))
    auto = Attribution(calm, x)                   # the arg-max target: fixed on the device from the clean pass
    assert auto.target.dtype == torch.int64 and tuple(auto.target.shape) == (K.B,)
    with torch.no_grad():
        calm.eval()
        probs, _ = calm([x], {})
        calm.train()
    assert torch.equal(auto.target, probs.argmax(dim=1))


def test_i_a_training_step_does_not_notice_the_call():
    from svit_amd import optim
    from svit_amd.attribution import Attribution
    x, y = clip(), labels()
    results = []
    for call in (False, True):
        _, model = build()
        opt = optim.GuardedClipAdamW(model, lr=1e-2)
        model.flat.grad.zero_()
        preds, extra = model([x], {})
        ce(preds, extra, y).backward()                # the gradient is pending ...
        if call:
            Attribution(model, clip("other")).smoothgrad(n=2)
        opt.step()                                    # ... and stepped
        model.flat.grad.zero_()
        preds, extra = model([clip("next")], {})
        ce(preds, extra, y).backward()
        opt.step()
        torch.cuda.synchronize()
        results.append((model.flat.data.clone(), model.flat.grad.clone(), opt.exp_avg.clone(), opt.exp_avg_sq.clone()))
    for a, b, what in zip(results[0], results[1], ("weights", "gradient", "exp_avg", "exp_avg_sq")):
        assert same(a, b), what
