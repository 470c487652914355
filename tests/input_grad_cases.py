"""Shared pieces of tests/test_input_grad_cpu.py and tests/test_input_grad_gpu.py: the shapes, seeded bf16 operands,
the derived stage bar and three mutants of the float64 restatement.

The stage bar is derived, not measured: one element of dvideo is a sum of at most 2 x 2 x 2 x 96 = 768 products, each
bf16 x bf16 and hence exact in fp32, accumulated in fp32 in some fixed order, so by the standard bound
|fl(sum) - sum| <= gamma_n * sum|terms| with gamma_768 < 768 * 2^-24 * (1 + tiny):

    |kernel - dgrad_host| <= 2 * 768 * 2^-24 * sum|dtok * w|      per element,

the factor 2 being margin over gamma_n; sum|dtok * w| is dgrad_host on the absolute values.
"""
import contextlib

import torch

B = 2
SHAPES = [(1, 8, 8), (2, 12, 20), (5, 17, 23), (4, 64, 64)]     # (T, H, W)
BAR_FACTOR = 2.0 * 768.0 * 2.0 ** -24


def out_dims(T, H, W):
    return (T - 1) // 2 + 1, (H - 1) // 4 + 1, (W - 1) // 4 + 1


def operands(T, H, W, nan_pad=True, seed=0):
    """(dtok bf16 [B*To*Ho*Wo, 96], w16 bf16 [96, 448]) on the host; the pad columns 441..447 hold NaN (or, for the
    mutant that reads them, ordinary values)"""
    To, Ho, Wo = out_dims(T, H, W)
    g = torch.Generator().manual_seed(1000 * seed + 100 * T + 10 * H + W)
    dtok = torch.randn((B * To * Ho * Wo, 96), generator=g).to(torch.bfloat16)
    w = (0.1 * torch.randn((96, 448), generator=g))
    if nan_pad:
        w[:, 441:] = float("nan")
    return dtok, w.to(torch.bfloat16)


def stage_bar(dtok, w, Bn, T, H, W):
    """float64 [B,3,T,H,W]: the per-element bar above"""
    from svit_amd.saliency import dgrad_host
    return BAR_FACTOR * dgrad_host(dtok.double().abs(), w.double()[:, :441].abs(), Bn, T, H, W)


def excess(got, ref, bar):
    """max over the elements of |got - ref| / bar (an element whose bar is 0 must be met exactly: inf otherwise); a NaN
    counts as inf"""
    err = (got.double().cpu() - ref).abs()
    err = torch.where(torch.isnan(err), torch.full_like(err, float("inf")), err)
    ratio = torch.where(bar > 0, err / bar.clamp_min(1e-300), torch.where(err > 0, torch.full_like(err, float("inf")),
                                                                          torch.zeros_like(err)))
    return float(ratio.max())


MUTANTS = ("ky_shift", "second_t_dropped", "pad_as_taps")


def dgrad_mutant(dtok, w, Bn, T, H, W, mutant):
    """The restatement of svit_amd.saliency.dgrad_host pixel by pixel, with one deliberate mistake:
    ky_shift          the row a tap reaches is 4yo - 2 + ky instead of 4yo - 3 + ky;
    second_t_dropped  of the (up to two) output frames that reach an input frame only the first is summed;
    pad_as_taps       the pad columns 441 + i, i < 7, are summed as further taps (c 0, kt 1, ky 0, kx i)."""
    assert mutant in MUTANTS
    To, Ho, Wo = out_dims(T, H, W)
    d = dtok.double().reshape(Bn, To, Ho, Wo, 96)
    w = w.double()
    yoff = 2 if mutant == "ky_shift" else 3
    out = torch.zeros((Bn, 3, T, H, W), dtype=torch.float64)
    yks = [[(yo, ky) for ky in range(7) for yo in range(Ho) if 4 * yo - yoff + ky == y] for y in range(H)]
    xks = [[(xo, kx) for kx in range(7) for xo in range(Wo) if 4 * xo - 3 + kx == x] for x in range(W)]
    for t in range(T):
        tk = [(to, kt) for kt in range(3) for to in range(To) if 2 * to - 1 + kt == t]
        if mutant == "second_t_dropped":
            tk = tk[:1]
        for y, yk in enumerate(yks):
            for x, xk in enumerate(xks):
                for to, kt in tk:
                    for yo, ky in yk:
                        for xo, kx in xk:
                            cols = [((c * 3 + kt) * 7 + ky) * 7 + kx for c in range(3)]
                            out[:, :, t, y, x] += d[:, to, yo, xo] @ w[:, cols]
                            if mutant == "pad_as_taps" and (kt, ky) == (1, 0):
                                out[:, 0, t, y, x] += d[:, to, yo, xo] @ w[:, 441 + kx]
    return out


@contextlib.contextmanager
def recording(target, name, log):
    """while the block runs, `target.name(*a, **k)` appends (a, k, result) to `log`"""
    real = getattr(target, name)

    def wrapper(*a, **k):
        r = real(*a, **k)
        log.append((a, k, r))
        return r
    setattr(target, name, wrapper)
    try:
        yield log
    finally:
        setattr(target, name, real)


@contextlib.contextmanager
def launch_names(log):
    """while the block runs, the names of the library launches (hip.call) are appended to `log`, in order"""
    from svit_amd import hip
    real = hip.call

    def logging(name, *a, **k):
        log.append(name)
        return real(name, *a, **k)
    hip.call = logging
    try:
        yield log
    finally:
        hip.call = real
