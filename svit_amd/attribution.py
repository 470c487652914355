"""Attribution passes: SmoothGrad (Smilkov et al., 2017) and integrated gradients (Sundararajan et al., 2017) over the
input-gradient-only backward.

A raw gradient of a ViT is a noisy map; both methods average 16-50 gradient passes per clip.  One pass here is

    upload 32 bytes (the pass record)          alpha, weight, seed, pass number, flags
    svit_attr_perturb                          clip_k = base + alpha_k (x - base) + sigma[b] * noise(seed_k)
    the pass                                   forward, scalar, the backward that computes NO parameter gradient
    svit_attr_accumulate                       acc = (k == 0 ? 0 : acc) + weight_k * (g or g*g); scores[k] = the logits

and the pass is either the replay of ONE captured GraphedTrainStep(input_grad="only") (`Attribution`) or the eager
`saliency.input_gradient(..., param_grads=False)` (the module functions `smoothgrad` / `integrated_gradients`: the twins
the captured route is tested against, and the route for a clip seen once).  Neither touches flat.grad, a param.grad, a
weight, a moment, a meter, a monitor or a draw counter, and neither reads the requires_grad flags: they may be called
between a backward and its optimizer step, and under a frozen cut.

The scalar is the sum over the batch of the TRAIN-mode logit preds[b, target[b]] (no softmax; DropPath and dropout are
off in these passes whatever the cfg's rates).  `target` is fixed before the first pass -- given, or the arg-max logits
of one clean no-grad pass -- so a noisy pass cannot move it.  For a U8Clips / AugClips the clip is `clips.render()`,
rendered once: the attribution is with respect to that render, not to the uint8 pixels or through the resampling taps.

`passes`, `perturb_host`, `accumulate_host`, `completeness` and `HostRoute` are pure host code: the schedule both device
routes use, the torch-CPU restatements the two kernels equal bit for bit, and the same driver over any differentiable
torch function (tests/test_attribution_cpu.py runs it on a float64 quadratic).
"""
import struct

import torch

SEED_MASK = 0x7FFFFFFF      # the 31-bit seeds of the erasing noise (augment.AugRecord.seed)


# ======================================================================================= schedule and restatements ====
def passes(method, n=1, seed=0):
    """[(alpha, weight, seed)] of the passes of one call, in order.
    "gradient": one pass at the clip.  "smoothgrad": n passes at the clip, weight 1/n, seed_k = (seed + k) & 0x7FFFFFFF.
    "integrated_gradients": the trapezoid rule over n + 1 points of the straight path, alpha_k = k/n, weight 1/(2n) at
    both ends and 1/n between (no noise: seed 0)."""
    n, seed = int(n), int(seed)
    if method == "gradient":
        return [(1.0, 1.0, seed & SEED_MASK)]
    if method == "smoothgrad":
        if n < 1:
            raise ValueError("smoothgrad needs n >= 1 passes, got %d" % n)
        return [(1.0, 1.0 / n, (seed + k) & SEED_MASK) for k in range(n)]
    if method == "integrated_gradients":
        if n < 1:
            raise ValueError("integrated_gradients needs steps >= 1, got %d" % n)
        return [(k / n, (0.5 if k in (0, n) else 1.0) / n, 0) for k in range(n + 1)]
    raise ValueError("passes: method is \"gradient\", \"smoothgrad\" or \"integrated_gradients\", got %r" % (method,))


def _scalar_like(v, t):
    return torch.tensor(float(v), dtype=t.dtype, device=t.device)


def perturb_host(x, base, alpha, sigma, noise):
    """svit_attr_perturb restated in torch, in x's dtype (fp32: bit-equal to the kernel), one rounding per operation:
    d = x - base; p = base + alpha*d; out = p + sigma[b]*noise.  base None: zeros.  sigma None: no noise term (not a
    product with 0); else a float or a [B] tensor."""
    base = torch.zeros_like(x) if base is None else base.to(x.dtype)
    d = x - base
    p = base + _scalar_like(alpha, x) * d
    if sigma is None:
        return p
    s = torch.as_tensor(sigma, dtype=x.dtype, device=x.device)
    s = s.reshape((-1,) + (1,) * (x.dim() - 1)) if s.dim() else s
    return p + s * noise.to(x.dtype)


def accumulate_host(acc, g, weight, squared, first):
    """svit_attr_accumulate restated in torch, in g's dtype: v = squared ? g*g : g; t = weight*v; first ? t : acc + t
    (the first pass never reads acc)"""
    v = g * g if squared else g
    t = _scalar_like(weight, g) * v
    return t if first else acc + t


def completeness(attr, scores, steps):
    """float64 [B]: sum(attr[b]) - (score[steps][b] - score[0][b]), the completeness residual of integrated gradients
    from the score table of its passes (row k = the per-sample scalars at alpha_k) -- no extra forward"""
    sc = scores.double()
    return attr.double().flatten(1).sum(dim=1) - (sc[steps] - sc[0])


def fix_target(target, clean_scores, B, device):
    """the int64 [B] target of every pass: the given one (checked), or the arg-max of `clean_scores()` -- [B, classes] of
    ONE clean pass -- taken on the tensor's device with no host read"""
    if target is None:
        return clean_scores().argmax(dim=1).to(torch.int64)
    if not torch.is_tensor(target) or target.dtype != torch.int64 or tuple(target.shape) != (B,):
        raise ValueError("target must be an int64 [%d] tensor (one class per clip), got %s"
                         % (B, "%s %s" % (target.dtype, tuple(target.shape)) if torch.is_tensor(target) else type(target)))
    return target.to(device)


def _check_sigma(sigma, B):
    """a float or a [B] tensor, not negative (a tensor is read once on the host for that)"""
    if torch.is_tensor(sigma):
        if tuple(sigma.shape) != (B,):
            raise ValueError("sigma must be a float or a [%d] tensor, got %s" % (B, tuple(sigma.shape)))
        if bool((sigma < 0).any()):
            raise ValueError("sigma must not be negative")
    elif float(sigma) < 0.0:
        raise ValueError("sigma must not be negative, got %r" % (sigma,))


# ================================================================================================== the one driver ====
def drive(route, plan, noisy=False, squared=False):
    """every route's loop: pass k of `plan` perturbs, differentiates and folds -- `route.one_pass` -- and leaves the sum in
    `route.acc`, the per-sample scores in row k of `route.scores`"""
    route.begin(len(plan))
    for k, (alpha, weight, seed) in enumerate(plan):
        route.one_pass(k, alpha, weight, seed, noisy, squared)
    return route.acc


def _run_gradient(route):
    return drive(route, passes("gradient"))


def _run_smoothgrad(route, n, sigma, noise_level, squared, seed):
    plan = passes("smoothgrad", n, seed)
    if sigma is None:
        if float(noise_level) < 0.0:
            raise ValueError("noise_level must not be negative, got %r" % (noise_level,))
        x = route.x
        sigma = float(noise_level) * (x.flatten(1).amax(dim=1) - x.flatten(1).amin(dim=1))     # per clip, on its device
    else:
        _check_sigma(sigma, route.x.shape[0])
    route.set_sigma(sigma)
    return drive(route, plan, noisy=True, squared=squared)


def _run_integrated(route, steps, baseline):
    plan = passes("integrated_gradients", steps)
    route.set_base(baseline)
    acc = drive(route, plan)
    x = route.x
    attr = acc * (x if route.base is None else x - route.base)        # plain torch, once, outside the per-pass body
    return attr, completeness(attr, route.scores, int(steps))


class HostRoute:
    """The driver over any differentiable torch function, on any device and in any dtype -- the toy route of the CPU
    tests and a readable statement of what the device routes compute.  fn(clip [B, ...]) -> scores [B, classes];
    noise(seed) -> a tensor like x (N(0,1) of that seed)."""

    def __init__(self, fn, x, target=None, noise=None):
        self.fn, self.x, self.noise = fn, x.detach(), noise
        self.base = self.sigma = self.acc = self.scores = None
        with torch.no_grad():
            self.target = fix_target(target, lambda: fn(self.x), x.shape[0], x.device)

    def set_sigma(self, sigma):
        self.sigma = sigma

    def set_base(self, base):
        self.base = base

    def begin(self, rows):
        self.acc = None
        self.scores = torch.zeros((rows, self.x.shape[0]), dtype=self.x.dtype, device=self.x.device)

    def one_pass(self, k, alpha, weight, seed, noisy, squared):
        noise = self.noise(seed) if noisy else None
        clip = perturb_host(self.x, self.base, alpha, self.sigma if noisy else None, noise).requires_grad_(True)
        s = self.fn(clip).gather(1, self.target[:, None]).squeeze(1)
        g, = torch.autograd.grad(s.sum(), [clip])
        self.acc = accumulate_host(self.acc, g, weight, squared, k == 0)
        self.scores[k] = s.detach()

    def gradient(self):
        return _run_gradient(self)

    def smoothgrad(self, n=16, sigma=None, noise_level=0.15, squared=False, seed=0):
        return _run_smoothgrad(self, n, sigma, noise_level, squared, seed)

    def integrated_gradients(self, steps=16, baseline=None):
        return _run_integrated(self, steps, baseline)


# ================================================================================================ the device routes ====
def pack_record(alpha, weight, seed, k, squared):
    """the 32 bytes of svit_attr_pass (include/svit_hip.h): float alpha, weight; uint32 seed, pass, flags, pad[3]"""
    return struct.pack("<ffIIIIII", float(alpha), float(weight), int(seed) & SEED_MASK, int(k), 1 if squared else 0, 0, 0, 0)


def _core(model):
    return model.module if hasattr(model, "module") else model


class _DeviceRoute:
    """what both device routes share: the rendered fp32 clip, the fixed target, the record and its upload ring, the
    accumulator and the score table, sigma and the baseline as device tensors"""

    def __init__(self, model, clips, target):
        from . import hip
        from .input import FramesView
        self.model, self.core = model, _core(model)
        core = self.core
        x = clips[0] if isinstance(clips, (list, tuple)) else clips
        # (the arguments first: every refusal below is raised before the device is needed)
        if isinstance(x, FramesView):
            raise ValueError("attribution on a FramesView: the frames pass is a no-grad forward and is not attributed")
        if not torch.is_tensor(x) and not hasattr(x, "render"):
            raise ValueError("attribution takes an fp32 clip tensor, a U8Clips or an AugClips, got %s" % type(x).__name__)
        if target is not None:
            fix_target(target, None, x.shape[0], "cpu")
        if getattr(core, "engine", None) is None:
            raise hip.SvitHipError("attribution needs a finalized (on-GPU) SViT")
        if not torch.is_tensor(x):
            x = x.render()              # once: the attribution is with respect to this render
        x = x.detach().to(torch.float32)
        if x.dim() == 4:
            x = x.unsqueeze(2)
        if x.dim() != 5 or x.shape[1] != 3:
            raise ValueError("attribution takes a clip [B,3,T,S,S] (or stills [B,3,S,S]), got %s" % (tuple(x.shape),))
        self.x = x.contiguous().clone()
        dev, B = self.x.device, self.x.shape[0]
        self.target = fix_target(target, self._clean_logits, B, dev).clone()
        self.base = self.sigma = self.scores = self._pass_scores = None
        self.acc = torch.empty_like(self.x)
        self.rec = torch.zeros(8, dtype=torch.int32, device=dev)
        self._slots = torch.empty((16, 8), dtype=torch.int32).pin_memory()
        self._events, self._next = [None] * 16, 0

    @torch.no_grad()
    def _clean_logits(self):
        """the class logits of one clean pass: backbone without drops, the head's class projection on the cls token"""
        eng, head = self.core.engine, self.core.head
        eng.refresh_weights()
        y, _ = eng.forward(self.x, None, save=False)
        return torch.nn.functional.linear(y[:, 0], head.projection.weight, head.projection.bias)

    def _scalar(self, preds, extra=None, labels=None):
        """the differentiated scalar; the per-sample logits are the pass's scores"""
        target = self.target if labels is None else labels      # (a captured step: its own static copy)
        s = preds.gather(1, target[:, None]).squeeze(1)
        self._pass_scores = s.detach()
        return s.sum()

    def _upload(self, alpha, weight, seed, k, squared):
        # 32 bytes, in stream order, without stalling the host: a ring of pinned slots, each guarded by the event of the
        # copy that last read it (as GraphedTrainStep uploads its mix record)
        i = self._next
        self._next = (i + 1) % len(self._events)
        if self._events[i] is not None:
            self._events[i].synchronize()
        self._slots[i].copy_(torch.frombuffer(bytearray(pack_record(alpha, weight, seed, k, squared)), dtype=torch.int32))
        self.rec.copy_(self._slots[i], non_blocking=True)
        ev = torch.cuda.Event()
        ev.record(torch.cuda.current_stream(self.x.device))
        self._events[i] = ev

    def set_sigma(self, sigma):
        dev, B = self.x.device, self.x.shape[0]
        if torch.is_tensor(sigma):
            self.sigma = sigma.detach().to(dev, torch.float32).contiguous()
        else:
            self.sigma = torch.full((B,), float(sigma), dtype=torch.float32, device=dev)

    def set_base(self, base):
        if base is None:
            self.base = None
            return
        if not torch.is_tensor(base):
            raise ValueError("the baseline is None (zeros) or a tensor in the clip's shape, got %s" % type(base).__name__)
        base = base.detach().to(self.x.device, torch.float32)
        if base.dim() == 4:
            base = base.unsqueeze(2)
        if base.shape != self.x.shape:
            raise ValueError("the baseline %s and the clip %s differ in shape" % (tuple(base.shape), tuple(self.x.shape)))
        self.base = base.contiguous()

    def begin(self, rows):
        if self.scores is None or self.scores.shape[0] != rows:
            self.scores = torch.empty((rows, self.x.shape[0]), dtype=torch.float32, device=self.x.device)

    def gradient(self):
        """d sum_b logit[b, target[b]] / d clip, f32 [B,3,T,S,S]: one pass (alpha 1, no noise, weight 1).  Like every
        result here it is the route's accumulator: the next call overwrites it."""
        with self._mode():
            return _run_gradient(self)

    def smoothgrad(self, n=16, sigma=None, noise_level=0.15, squared=False, seed=0):
        """the mean over n passes of the gradient (squared: of its square) at clip + sigma[b] * N(0,1).  sigma: a float
        or f32 [B] in the clip's units; None: noise_level * (max - min) per clip.  Pass k draws the erasing-noise field
        of seed (seed + k) & 0x7FFFFFFF."""
        with self._mode():
            return _run_smoothgrad(self, n, sigma, noise_level, squared, seed)

    def integrated_gradients(self, steps=16, baseline=None):
        """-> (attr, delta): attr = (x - baseline) * the trapezoid mean of the gradient over steps + 1 points of the
        straight path from the baseline (None: zeros) to the clip; delta float64 [B] = sum(attr[b]) - (score at the
        clip - score at the baseline), the completeness residual, from the passes' own scores."""
        with self._mode():
            return _run_integrated(self, steps, baseline)


class _TrainMode:
    """the model in train mode (the passes differentiate the train-mode logits), its mode restored on exit"""

    def __init__(self, model):
        self.model = model

    def __enter__(self):
        self.was = self.model.training
        self.model.train()

    def __exit__(self, *exc):
        self.model.train(self.was)
        return False


class Attribution(_DeviceRoute):
    """The captured route: ONE GraphedTrainStep(input_grad="only") over a static fp32 clip, replayed per pass between the
    two kernels.

        attr = Attribution(model, clips, target=None)       # captures; the model's mode is restored
        g = attr.gradient()
        sg = attr.smoothgrad(n=16, noise_level=0.15)
        ig, delta = attr.integrated_gradients(steps=16)
        attr.refresh()                                      # after the weights moved (an optimizer step)

    clips: an fp32 tensor [B,3,T,S,S] (stills [B,3,S,S]), a U8Clips or an AugClips (rendered once).  target: int64 [B],
    or None for the arg-max logits of one clean pass.  A new clip of the same shape: `set_clip`."""

    def __init__(self, model, clips, target=None, warmup=2):
        from .graph import GraphedTrainStep
        super().__init__(model, clips, target)
        with _TrainMode(model):
            self.step = GraphedTrainStep(model, self._scalar, [self.x], self.target, warmup=warmup, input_grad="only")
        self.target = self.step.static_labels       # (the step's own copy: what the captured gather reads)

    def _mode(self):
        return _Nothing()       # (a replay does not look at the model's mode)

    def refresh(self):
        """the bf16 copies of the weights the captured pass reads: call after the weights moved"""
        self.step.refresh()

    def set_clip(self, clips, target=None):
        """another clip of the captured shape (and its target: given, or the arg-max logits of its clean pass)"""
        other = _DeviceRoute(self.model, clips, target)
        if other.x.shape != self.x.shape:
            raise ValueError("this Attribution was captured for a clip %s, got %s" % (tuple(self.x.shape), tuple(other.x.shape)))
        self.x.copy_(other.x)
        self.target.copy_(other.target)

    def one_pass(self, k, alpha, weight, seed, noisy, squared):
        from . import ops
        step = self.step
        self._upload(alpha, weight, seed, k, squared)
        ops.attr_perturb(self.x, self.rec, base=self.base, sigma=self.sigma if noisy else None, out=step.x)
        step([step.x], step.static_labels)           # (the static buffers themselves: nothing is copied)
        ops.attr_accumulate(step.input_grad, self.acc, self.rec, self._pass_scores, self.scores)


class _Nothing:
    def __enter__(self):
        return None

    def __exit__(self, *exc):
        return False


class _EagerRoute(_DeviceRoute):
    """the eager twin: every pass is `saliency.input_gradient(..., param_grads=False)` between the same two kernels"""

    def _mode(self):
        return _TrainMode(self.model)

    def one_pass(self, k, alpha, weight, seed, noisy, squared):
        from . import ops
        from .saliency import input_gradient
        self._upload(alpha, weight, seed, k, squared)
        clip = ops.attr_perturb(self.x, self.rec, base=self.base, sigma=self.sigma if noisy else None)
        g = input_gradient(self.model, clip, scalar=self._scalar, param_grads=False)
        ops.attr_accumulate(g, self.acc, self.rec, self._pass_scores, self.scores)


def _check_call(method, n, sigma=None, noise_level=0.0):
    """the refusals of a call that need no route: n / steps below 1, a negative float sigma or noise level"""
    passes(method, n)
    if sigma is not None and not torch.is_tensor(sigma):
        _check_sigma(sigma, 0)
    if sigma is None and float(noise_level) < 0.0:
        raise ValueError("noise_level must not be negative, got %r" % (noise_level,))


def gradient(model, clips, target=None):
    """`Attribution.gradient` without a capture"""
    return _EagerRoute(model, clips, target).gradient()


def smoothgrad(model, clips, target=None, n=16, sigma=None, noise_level=0.15, squared=False, seed=0):
    """`Attribution.smoothgrad` without a capture: n eager passes"""
    _check_call("smoothgrad", n, sigma, noise_level)
    return _EagerRoute(model, clips, target).smoothgrad(n, sigma, noise_level, squared, seed)


def integrated_gradients(model, clips, target=None, steps=16, baseline=None):
    """`Attribution.integrated_gradients` without a capture: steps + 1 eager passes -> (attr, delta)"""
    _check_call("integrated_gradients", steps)
    return _EagerRoute(model, clips, target).integrated_gradients(steps, baseline)
