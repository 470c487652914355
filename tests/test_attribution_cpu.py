"""Attribution passes without a GPU: the schedule (`passes`), the driver on a float64 toy quadratic (trapezoid integrated
gradients are exact for a gradient linear in alpha), the restatements of the two kernels on hand-computed fp32 cases,
and every refusal of the two entry points and of the Python layer."""
import ctypes as C
import struct
import types

import pytest
import torch

from svit_amd import attribution as A

ERR_SHAPE, ERR_ALIGN, ERR_ARG = -2, -3, -4


# ======================================================================================================= schedule ====
def test_passes():
    assert A.passes("gradient") == [(1.0, 1.0, 0)]
    assert A.passes("gradient", seed=2 ** 31 + 5) == [(1.0, 1.0, 5)]
    assert A.passes("smoothgrad", 1, 9) == [(1.0, 1.0, 9)]
    p = A.passes("smoothgrad", 3, 2 ** 31 - 2)
    assert [a for a, _, _ in p] == [1.0] * 3 and [w for _, w, _ in p] == [1.0 / 3] * 3
    assert [s for _, _, s in p] == [2 ** 31 - 2, 2 ** 31 - 1, 0]                  # seed + k wraps at 2^31
    assert A.passes("integrated_gradients", 1) == [(0.0, 0.5, 0), (1.0, 0.5, 0)]
    p = A.passes("integrated_gradients", 4)
    assert [a for a, _, _ in p] == [0.0, 0.25, 0.5, 0.75, 1.0]
    assert [w for _, w, _ in p] == [0.125, 0.25, 0.25, 0.25, 0.125]
    for method, n in (("gradient", 1), ("smoothgrad", 1), ("smoothgrad", 3), ("smoothgrad", 7),
                      ("integrated_gradients", 1), ("integrated_gradients", 4), ("integrated_gradients", 7)):
        assert abs(sum(w for _, w, _ in A.passes(method, n)) - 1.0) <= 1e-15, (method, n)
    with pytest.raises(ValueError, match="n >= 1"):
        A.passes("smoothgrad", 0)
    with pytest.raises(ValueError, match="steps >= 1"):
        A.passes("integrated_gradients", 0)
    with pytest.raises(ValueError, match="method"):
        A.passes("gradcam")


def test_the_record_is_the_struct_of_the_header():
    raw = A.pack_record(0.3, 1.0 / 3, 2 ** 31 + 7, 5, True)
    assert len(raw) == 32
    alpha, weight, seed, k, flags, p0, p1, p2 = struct.unpack("<ffIIIIII", raw)
    assert alpha == torch.tensor(0.3, dtype=torch.float32).item() and weight == torch.tensor(1 / 3, dtype=torch.float32).item()
    assert (seed, k, flags, p0, p1, p2) == (7, 5, 1, 0, 0, 0)
    from svit_amd import hip
    assert C.sizeof(hip.AttrPass) == 32


# ============================================================================================ the driver on a toy ====
def quadratic(seed=0, dim=6):
    """F_c(x) = x . A_c x per class c, float64: the gradient (A_c + A_c^T) x is linear along a straight path"""
    g = torch.Generator().manual_seed(seed)
    mats = torch.randn((3, dim, dim), generator=g, dtype=torch.float64)

    def fn(clip):
        v = clip.flatten(1)
        return torch.einsum("bi,cij,bj->bc", v, mats, v)
    return fn, mats


def test_trapezoid_integrated_gradients_are_exact_on_a_quadratic():
    fn, mats = quadratic()
    g = torch.Generator().manual_seed(1)
    x = torch.randn((2, 3, 2), generator=g, dtype=torch.float64)
    base = torch.randn((2, 3, 2), generator=g, dtype=torch.float64)
    target = torch.tensor([2, 0])
    for steps in (1, 4):
        for b in (None, base):
            route = A.HostRoute(fn, x, target=target)
            attr, delta = route.integrated_gradients(steps=steps, baseline=b)
            zero = torch.zeros_like(x) if b is None else b
            gap = fn(x).gather(1, target[:, None]).squeeze(1) - fn(zero).gather(1, target[:, None]).squeeze(1)
            assert attr.shape == x.shape and delta.dtype == torch.float64 and tuple(delta.shape) == (2,)
            assert bool((delta.abs() <= 1e-9 * gap.abs()).all()), (steps, delta, gap)
            assert tuple(route.scores.shape) == (steps + 1, 2)
            assert torch.equal(route.scores[0], fn(zero).gather(1, target[:, None]).squeeze(1))


def test_smoothgrad_on_a_quadratic():
    fn, mats = quadratic()
    g = torch.Generator().manual_seed(2)
    x = torch.randn((2, 6), generator=g, dtype=torch.float64)
    target = torch.tensor([1, 2])
    noise = lambda seed: torch.randn(x.shape, generator=torch.Generator().manual_seed(seed), dtype=torch.float64)
    plain = A.HostRoute(fn, x, target=target).gradient()
    sym = mats + mats.transpose(1, 2)
    assert torch.allclose(plain, torch.einsum("bij,bj->bi", sym[target], x), rtol=1e-13, atol=0)
    # sigma = 0: every pass is the clean clip; n = 1 so that no rounding of the mean enters
    assert torch.equal(A.HostRoute(fn, x, target=target, noise=noise).smoothgrad(n=1, sigma=0.0), plain)
    got = A.HostRoute(fn, x, target=target, noise=noise).smoothgrad(n=4, sigma=0.0)
    assert torch.equal(got, plain)          # (weights 1/4: the four equal quarters sum exactly)
    assert torch.equal(A.HostRoute(fn, x, target=target, noise=noise).smoothgrad(n=1, sigma=0.0, squared=True), plain * plain)
    # with noise the mean of a LINEAR gradient is the gradient at the mean clip
    route = A.HostRoute(fn, x, target=target, noise=noise)
    got = route.smoothgrad(n=3, sigma=torch.tensor([0.5, 2.0], dtype=torch.float64), seed=2 ** 31 - 1)
    mean_noise = sum(noise(s) for s in (2 ** 31 - 1, 0, 1)) / 3
    mean_clip = x + torch.tensor([[0.5], [2.0]], dtype=torch.float64) * mean_noise
    assert torch.allclose(got, torch.einsum("bij,bj->bi", sym[target], mean_clip), rtol=1e-12, atol=1e-12)
    # the default sigma: noise_level x the clip's range, per clip
    route = A.HostRoute(fn, x, target=target, noise=noise)
    route.smoothgrad(n=1, noise_level=0.25)
    assert torch.equal(route.sigma, 0.25 * (x.amax(dim=1) - x.amin(dim=1)))


def test_the_target_is_fixed_by_the_clean_pass():
    """two classes whose order the noise swaps: score_0 = sum(x), score_1 = 1; clean sum(x) = 2 > 1, noisy sum(x) < 1"""
    def fn(clip):
        return torch.stack((clip.flatten(1).sum(dim=1), torch.ones(clip.shape[0], dtype=clip.dtype)), dim=1)
    x = torch.full((1, 4), 0.5, dtype=torch.float64)
    noise = lambda seed: torch.full((1, 4), -1.0, dtype=torch.float64)
    route = A.HostRoute(fn, x, noise=noise)
    assert route.target.tolist() == [0] and route.target.dtype == torch.int64
    noisy = A.perturb_host(x, None, 1.0, 1.0, noise(0))
    assert fn(noisy).argmax(dim=1).tolist() == [1]                  # the noisy pass would pick the other class
    got = route.smoothgrad(n=2, sigma=1.0)
    assert torch.equal(got, torch.ones_like(x))                      # d sum(x): class 0 in both passes (class 1: zeros)
    assert torch.equal(route.scores, torch.tensor([[-2.0], [-2.0]], dtype=torch.float64))


# ============================================================================================== the restatements ====
def f32(*v):
    return torch.tensor(v, dtype=torch.float32)


def test_perturb_host_hand_cases():
    x, base = f32(1.0, 0.1, -3.0), f32(0.5, 1e8, -0.0)
    a = torch.tensor(0.3, dtype=torch.float32)
    got = A.perturb_host(x, base, 0.3, None, None)
    assert torch.equal(got, base + a * (x - base)) and got.dtype == torch.float32
    # alpha = 1 does not give x back: 0.1 - 1e8 rounds to -1e8, and 1e8 + (-1e8) = 0
    one = A.perturb_host(x, base, 1.0, None, None)
    assert one.tolist() == [1.0, 0.0, -3.0] and one[1] != x[1]
    # 0.3: fp32(0.3) = 0x3E99999A, half of it is exact, 0.5 + 0.15000000596 lies midway between 0x3F266666 and
    # 0x3F266667 and rounds to the even one
    assert got[0].item() == (f32(0.5) + a * f32(0.5)).item() == 0.6499999761581421
    # base None is zeros; sigma None is no noise term; a per-clip sigma scales its clip
    xs = torch.stack((x, x))
    assert torch.equal(A.perturb_host(xs, None, 0.5, None, None), 0.5 * xs)
    n = torch.stack((f32(1.0, -1.0, 2.0), f32(1.0, -1.0, 2.0)))
    got = A.perturb_host(xs, None, 1.0, f32(0.5, 2.0), n)
    assert got.tolist() == [[1.5, -0.4000000059604645, -2.0], [3.0, -1.899999976158142, 1.0]]
    assert torch.equal(A.perturb_host(xs, None, 1.0, 0.0, n), xs)


def test_accumulate_host_hand_cases():
    g = f32(-0.0, 3.0, 1e-30, -2.0)
    nan = torch.full((4,), float("nan"))
    first = A.accumulate_host(nan, g, 1.0, False, True)             # the first pass stores: acc is never read
    assert torch.equal(first.view(torch.int32), g.view(torch.int32))               # ... and -0.0 survives
    assert A.accumulate_host(None, g, 0.5, False, True).tolist() == [-0.0, 1.5, f32(1e-30).item() / 2, -1.0]     # (halving is exact)
    sq = A.accumulate_host(None, g, 0.5, True, True)
    assert sq.tolist() == [0.0, 4.5, 0.0, 2.0]                       # (1e-30 squared underflows)
    w = torch.tensor(1.0 / 3, dtype=torch.float32)
    second = A.accumulate_host(first, f32(1.0, 1.0, 1.0, 1.0), 1.0 / 3, False, False)
    assert torch.equal(second, first + w * f32(1.0, 1.0, 1.0, 1.0))
    # 3 + fp32(1/3) = 3.33333334327 lies 0.9e-7 above 0x40555555 and 1.5e-7 below 0x40555556
    assert second[1].item() == 3.3333332538604736


def test_completeness():
    attr = torch.tensor([[[1.0, 2.0]], [[0.5, 0.25]]])
    scores = torch.tensor([[1.0, 0.0], [9.0, 9.0], [3.5, 1.0]])
    d = A.completeness(attr, scores, 2)
    assert d.dtype == torch.float64 and d.tolist() == [0.5, -0.25]


# ===================================================================================================== refusals ====
def test_entry_points_refuse_bad_arguments_without_a_gpu():
    from svit_amd import hip
    lib = hip.load()
    p = 64      # any non-null, 16-byte aligned address: every check comes before the first HIP call
    ok = dict(x=p, base=None, sigma=None, rec=p, out=p, B=2, T=4, H=8, W=8)

    def perturb(**kw):
        a = dict(ok, **kw)
        return lib.svit_attr_perturb(a["x"], a["base"], a["sigma"], a["rec"], a["out"], a["B"], a["T"], a["H"], a["W"], None)
    for name in ("x", "rec", "out"):
        assert perturb(**{name: None}) == ERR_ARG, name
    for name in ("B", "T", "H", "W"):
        assert perturb(**{name: 0}) == ERR_ARG, name
    assert perturb(B=-1) == ERR_ARG
    for name in ("x", "base", "sigma", "rec", "out"):
        assert perturb(**{name: p + 2}) == ERR_ALIGN, name
    assert perturb(H=1 << 16, W=1 << 15) == ERR_SHAPE and perturb(B=1 << 20, T=1 << 10) == ERR_SHAPE
    okc = dict(g=p, acc=p, rec=p, scores_in=None, scores=None, rows=0, n=100, B=2)

    def accumulate(**kw):
        a = dict(okc, **kw)
        return lib.svit_attr_accumulate(a["g"], a["acc"], a["rec"], a["scores_in"], a["scores"], a["rows"], a["n"], a["B"], None)
    for name in ("g", "acc", "rec"):
        assert accumulate(**{name: None}) == ERR_ARG, name
    assert accumulate(n=0) == ERR_ARG and accumulate(B=0) == ERR_ARG and accumulate(n=-5) == ERR_ARG
    assert accumulate(scores=p, rows=3) == ERR_ARG                       # a table without the pass's scores
    assert accumulate(scores=p, scores_in=p, rows=0) == ERR_ARG
    for name in ("g", "acc", "rec"):
        assert accumulate(**{name: p + 1}) == ERR_ALIGN, name
    assert accumulate(scores=p + 2, scores_in=p, rows=3) == ERR_ALIGN
    assert accumulate(scores=p, scores_in=p + 2, rows=3) == ERR_ALIGN


def test_the_python_layer_refuses():
    from svit_amd import hip
    from svit_amd.graph import GraphedTrainStep
    from svit_amd.input import FramesView
    x, y = torch.zeros((2, 3, 4, 64, 64)), torch.zeros(2, dtype=torch.int64)
    loss = lambda p, e, t: p.sum()
    for kw, what in ((dict(frames_pass=True), "frames_pass"), (dict(frames_pass="u8"), "frames_pass"),
                     (dict(optimizer=object()), "optimizer="), (dict(accumulate=True), "accumulate=True"),
                     (dict(meter=object()), "meter="), (dict(mixup=object()), "mixup=")):
        with pytest.raises(hip.SvitHipError, match="refuses " + what):
            GraphedTrainStep(None, loss, [x], y, input_grad="only", **kw)
    with pytest.raises(hip.SvitHipError, match="False, True or"):
        GraphedTrainStep(None, loss, [x], y, input_grad="all")
    view = FramesView.__new__(FramesView)
    view.clips = types.SimpleNamespace(shape=torch.Size((2, 3, 4, 64, 64)))
    model = types.SimpleNamespace(engine=None)
    for build in (lambda **kw: A.Attribution(model, **kw), lambda **kw: A.smoothgrad(model, **kw),
                  lambda **kw: A.integrated_gradients(model, **kw), lambda **kw: A.gradient(model, **kw)):
        with pytest.raises(ValueError, match="FramesView"):
            build(clips=view)
        with pytest.raises(ValueError, match="int64 \\[2\\]"):
            build(clips=x, target=torch.zeros(3, dtype=torch.int64))
        with pytest.raises(ValueError, match="int64 \\[2\\]"):
            build(clips=x, target=torch.zeros(2, dtype=torch.int32))
        with pytest.raises(ValueError, match="int64 \\[2\\]"):
            build(clips=x, target=[1, 2])
        with pytest.raises(ValueError, match="fp32 clip tensor"):
            build(clips="clip.mp4")
        with pytest.raises(hip.SvitHipError, match="finalized"):      # (the arguments pass: now the device is needed)
            build(clips=x, target=y)
    with pytest.raises(ValueError, match="steps >= 1"):
        A.integrated_gradients(model, x, steps=0)
    with pytest.raises(ValueError, match="n >= 1"):
        A.smoothgrad(model, x, n=0)
    with pytest.raises(ValueError, match="negative"):
        A.smoothgrad(model, x, sigma=-0.1)
    with pytest.raises(ValueError, match="negative"):
        A.smoothgrad(model, x, noise_level=-0.1)
    # the methods of a built route (the captured one shares them): through the host route
    fn = lambda c: torch.stack((c.flatten(1).sum(1), -c.flatten(1).sum(1)), dim=1)
    route = A.HostRoute(fn, torch.ones((2, 3), dtype=torch.float64), noise=lambda s: torch.zeros((2, 3), dtype=torch.float64))
    with pytest.raises(ValueError, match="steps >= 1"):
        route.integrated_gradients(steps=0)
    with pytest.raises(ValueError, match="n >= 1"):
        route.smoothgrad(n=0)
    with pytest.raises(ValueError, match="negative"):
        route.smoothgrad(sigma=-1.0)
    with pytest.raises(ValueError, match="negative"):
        route.smoothgrad(sigma=torch.tensor([0.5, -2.0]))
    with pytest.raises(ValueError, match="\\[2\\] tensor"):
        route.smoothgrad(sigma=torch.tensor([0.5, 1.0, 2.0]))
    with pytest.raises(ValueError, match="int64 \\[2\\]"):
        A.HostRoute(fn, torch.ones((2, 3)), target=torch.zeros((2, 1), dtype=torch.int64))


def test_only_is_the_one_string_the_model_takes():
    from svit_amd.engine import Engine
    with pytest.raises(ValueError, match="False, True or"):
        Engine.forward(types.SimpleNamespace(), torch.zeros((1, 3, 4, 8, 8)), input_grad="all")
