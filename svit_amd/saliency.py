"""Input gradients: d loss / d clip out of the HIP backward, and what is built on it.

The backbone's backward ends at the stem; with a request it goes one launch further: `svit_patch_embed_dgrad`
(csrc/dgrad.hip) turns the bf16 patch rows of block 0's dx and the forward's bf16 weight operand into the gradient with
respect to the clip, f32 [B,3,T,S,S].  Three ways to ask:

    clip.requires_grad_(True); model([clip], meta); loss.backward(); clip.grad       # an fp32 tensor, as any module
    model([u8_clips], meta, input_grad=True); loss.backward(); model.last_input_grad # U8Clips / AugClips
    GraphedTrainStep(..., input_grad=True); step(...); step.input_grad               # inside the captured step

and `input_gradient` below does the first two for a scalar of choice.  For a U8Clips / AugClips the gradient is in the
coordinates of the S x S window the stem reads: d loss / d clips.render() (under cfg.MIXUP: d / d the mixed clip), not
with respect to the uint8 source pixels or through the resampling taps.  Nothing here works under a frozen cut
(svit_amd/freeze.py): the frozen blocks keep no activations -- except the pass that computes no parameter gradient
(`input_gradient(..., param_grads=False)`, `forward(..., input_grad="only")`), which saves every block and leaves the
training state alone; svit_amd/attribution.py builds SmoothGrad and integrated gradients on it.

`dgrad_host` is the float64 yardstick the kernel is held to (tests/test_input_grad_*.py).
"""
import torch


def dgrad_host(dtok, w, B, T, H, W):
    """float64 restatement of svit_patch_embed_dgrad, written out as index arithmetic over the taps:
        dvideo[b,c,t,y,x] = sum over (to,kt), (yo,ky), (xo,kx) of sum_n dtok[(b,to,yo,xo), n] * w[n, col(c,kt,ky,kx)]
    with t = 2to-1+kt, y = 4yo-3+ky, x = 4xo-3+kx, col = ((c*3+kt)*7+ky)*7+kx, kt in [0,3), ky, kx in [0,7) and
    (to,yo,xo) inside [0,To) x [0,Ho) x [0,Wo).  dtok [B*To*Ho*Wo, 96] and w [96, >= 441] (columns past 440 are never
    read) are tensors of any float type on any device -> float64 [B,3,T,H,W] on the host."""
    To, Ho, Wo = (T - 1) // 2 + 1, (H - 1) // 4 + 1, (W - 1) // 4 + 1
    d = torch.as_tensor(dtok).detach().to("cpu", torch.float64).reshape(B, To, Ho, Wo, -1)
    w = torch.as_tensor(w).detach().to("cpu", torch.float64)
    N = d.shape[-1]
    if w.dim() != 2 or w.shape[0] != N or w.shape[1] < 441:
        raise ValueError("dgrad_host: w must be [%d, >= 441], got %s" % (N, tuple(w.shape)))
    out = torch.zeros((B, 3, T, H, W), dtype=torch.float64)
    for kt in range(3):
        tos = [to for to in range(To) if 0 <= 2 * to - 1 + kt < T]
        for ky in range(7):
            yos = [yo for yo in range(Ho) if 0 <= 4 * yo - 3 + ky < H]
            for kx in range(7):
                xos = [xo for xo in range(Wo) if 0 <= 4 * xo - 3 + kx < W]
                if not (tos and yos and xos):
                    continue
                cols = [((c * 3 + kt) * 7 + ky) * 7 + kx for c in range(3)]
                # [B, to, yo, xo, n] x [n, c] for the output positions this tap reaches
                part = d[:, tos][:, :, yos][:, :, :, xos] @ w[:, cols]
                ts = torch.tensor([2 * to - 1 + kt for to in tos])
                ys = torch.tensor([4 * yo - 3 + ky for yo in yos])
                xs = torch.tensor([4 * xo - 3 + kx for xo in xos])
                # (one tap maps output positions to pixels one to one, so the indexed += meets no index twice)
                out[:, :, ts[:, None, None], ys[None, :, None], xs[None, None, :]] += part.permute(0, 4, 1, 2, 3)
    return out


def _core(model):
    return model.module if hasattr(model, "module") else model


def _default_scalar(preds, extra_preds):
    """the sum of each sample's largest logit (in eval mode: its largest class probability)"""
    return preds.max(dim=1).values.sum()


def input_gradient(model, clips, labels=None, meta=None, scalar=None, param_grads=True):
    """d scalar / d clip, f32 [B,3,T,S,S] (T = 1 for stills), from ONE saving forward and ONE full backward in the
    model's current mode (call model.eval() first for a checkpoint: no DropPath, no dropout, the head's softmax).
    clips: the fp32 clip tensor [B,3,T,S,S] (or stills [B,3,S,S]), an input.U8Clips or an augment.AugClips -- for those
    the gradient is with respect to `clips.render()`.  A one-element list, as the model takes it, is accepted.
    The scalar: with `labels` (or an image rank's `meta` holding "haog_bboxes") the step's loss, losses.VideoImageLoss
    over the model's cfg (cross entropy on a video rank, the HAOG losses with `meta`); otherwise
    `scalar(preds, extra_preds)`, by default the sum of each sample's largest logit.
    The backward accumulates parameter gradients like any other: `flat.grad` IS ZEROED ON EXIT, so call this between
    steps, not between a backward and its optimizer step.  Raises ValueError under a frozen cut.
    param_grads=False: the pass that computes the input gradient and NO parameter gradient (forward(...,
    input_grad="only")) -- the same gradient bit for bit where both routes run, but flat.grad and every param.grad are
    left as they are (nothing is zeroed on exit: it may be called between a backward and its optimizer step), frozen
    parameters do not matter, and in train mode DropPath and dropout are off and nothing is drawn."""
    core = _core(model)
    if not param_grads:
        return _input_gradient_only(model, core, clips, labels, meta, scalar)
    cut = core.frozen_cut()
    if cut > 0:
        raise ValueError("input_gradient under a frozen cut (the parameters' requires_grad flags freeze everything "
                         "below position %d): the backward stops above the frozen blocks, which keep no activations "
                         "-- unfreeze the model (freeze_below(0)) first" % cut)
    x = clips[0] if isinstance(clips, (list, tuple)) else clips
    image = meta is not None and "haog_bboxes" in meta
    try:
        with torch.enable_grad():
            if torch.is_tensor(x):
                leaf = x.detach().to(torch.float32).requires_grad_(True)
                preds, extra = model([leaf], meta)
            else:
                leaf = None
                preds, extra = model([x], meta, input_grad=True)
            if labels is not None or image:
                from .losses import VideoImageLoss
                fn = VideoImageLoss(core.cfg, is_video_rank=not image)
                s = fn.total(fn(preds, extra, labels, meta))
            else:
                s = (scalar or _default_scalar)(preds, extra)
            s.backward()
        grad = leaf.grad if leaf is not None else core.last_input_grad
        if grad is None:
            raise RuntimeError("input_gradient: the backward left no input gradient (does the scalar depend on the "
                               "model's outputs?)")
        return grad.unsqueeze(2) if grad.dim() == 4 else grad
    finally:
        core.last_input_grad = None
        if core.flat is not None:
            core.flat.grad.zero_()


def _input_gradient_only(model, core, clips, labels, meta, scalar):
    x = clips[0] if isinstance(clips, (list, tuple)) else clips
    image = meta is not None and "haog_bboxes" in meta
    try:
        with torch.enable_grad():
            if torch.is_tensor(x):
                x = x.detach().to(torch.float32)
            preds, extra = model([x], meta, input_grad="only")
            if labels is not None or image:
                from .losses import VideoImageLoss
                fn = VideoImageLoss(core.cfg, is_video_rank=not image)
                s = fn.total(fn(preds, extra, labels, meta))
            else:
                s = (scalar or _default_scalar)(preds, extra)
            s.backward()
        grad = core.last_input_grad
        if grad is None:
            raise RuntimeError("input_gradient: the backward left no input gradient (does the scalar depend on the "
                               "model's outputs?)")
        return grad.unsqueeze(2) if grad.dim() == 4 else grad
    finally:
        core.last_input_grad = None


def saliency_map(grad):
    """[B,3,T,S,S] -> [B,T,S,S]: the largest |gradient| over the channels of each pixel"""
    if grad.dim() != 5 or grad.shape[1] != 3:
        raise ValueError("saliency_map takes a gradient [B,3,T,S,S], got %s" % (tuple(grad.shape),))
    return grad.abs().amax(dim=1)


def grad_times_input(grad, clip):
    """gradient x input, elementwise, in the gradient's shape (a 4-D still is read as T = 1)"""
    if clip.dim() == 4 and grad.dim() == 5:
        clip = clip.unsqueeze(2)
    if clip.shape != grad.shape:
        raise ValueError("grad_times_input: gradient %s and clip %s differ" % (tuple(grad.shape), tuple(clip.shape)))
    return grad * clip.to(grad.dtype)


def fgsm(clip, grad, eps):
    """clip + eps * sign(grad) (Goodfellow et al., 2015), plain torch, in the clip's shape and dtype: the one-step
    adversarial clip of a robustness evaluation -- feed it to the existing eval loops.  eps is in the clip's own
    (normalised) units."""
    g = grad.reshape(clip.shape) if grad.shape != clip.shape else grad
    return clip + eps * torch.sign(g).to(clip.dtype)
