"""Batch-level mixup / CutMix with label smoothing (cfg.MIXUP; slowfast/datasets/mixup.py::MixUp, used by
tools/train_net.py:63-71,92-94 of the reference).

What is drawn per step is tiny -- a mode, a lambda, a box -- and is drawn on the HOST from the global `np.random`
stream in the reference's order, so after `np.random.seed(s)` a run here mixes exactly what the reference mixes (the
reference seeds every rank alike, so all ranks mix alike here too).  The draw is packed into a 32-byte RECORD that lives in
device memory; the three kernels of the feature read it there (include/svit_hip.h: `svit_mixup_clips`,
`svit_im2col_patch_u8_mix`, `svit_ce_loss_soft`), so a captured training step holds the same launches for every draw and
`GraphedTrainStep(..., mixup=...)` only rewrites 32 bytes between replays.

Two routes:

    samples, target = mixup_fn(inputs[0], labels)        # the reference's call: x mixed in place, dense [B,C] target
    samples, mixed = mixup_fn.mix(inputs[0], labels)     # fused: x mixed in place (or a U8Clips tagged), `MixedLabels`
                                                         # for losses.cross_entropy / VideoImageLoss -- no [B,C] target

Out of scope (a clear error where it can be hit): the image ranks' HAOG losses (VideoImageLoss refuses a soft target
there), dict-valued `num_classes` (the reference's Epic-Kitchens noun/verb heads), per-sample lambdas (one lambda per
batch, as the reference), and device-side random draws (the host draws; the device only reads the record).
"""
import collections
import math

import numpy as np
import torch

from . import hip

MODE_NONE, MODE_MIXUP, MODE_CUTMIX = 0, 1, 2


class MixRecord(collections.namedtuple("MixRecord", "mode lam yl yh xl xh")):
    """One draw on the host: mode (0 none, 1 mixup, 2 CutMix), lam (float64; for CutMix the area-corrected value, used by
    the target only) and the CutMix box.  `pack()` is the 8-word device record."""
    __slots__ = ()

    @property
    def use_cutmix(self):
        return self.mode == MODE_CUTMIX

    @property
    def box(self):
        return (self.yl, self.yh, self.xl, self.xh)

    def pack(self):
        """int32 [8]: mode | f32 lam | f32 (1.0 - lam), the subtraction in double as torch does with the Python scalar |
        yl yh xl xh | 0"""
        w = np.zeros(8, dtype=np.int32)
        w[0] = self.mode
        w[1:3] = np.array([self.lam, 1.0 - self.lam], dtype=np.float64).astype(np.float32).view(np.int32)
        w[3:7] = self.box
        return w


NO_MIX = MixRecord(MODE_NONE, 1.0, 0, 0, 0, 0)


def smoothed_one_hot_values(smoothing, num_classes):
    """(on, off) of the label-smoothed one-hot rows, in double (cast to fp32 where they are stored)."""
    off = smoothing / num_classes
    return 1.0 - smoothing + off, off


def dense_target(labels, num_classes, lam, oml, on, off):
    """[B,C] f32: one_hot(labels) * lam + one_hot(labels reversed) * oml over the smoothed values.  lam / oml: Python
    floats or 0-dim fp32 tensors (the device record's words) -- both multiply in fp32, bit for bit alike."""
    y = labels.long().view(-1, 1)
    t1 = torch.full((y.shape[0], num_classes), off, device=y.device, dtype=torch.float32).scatter_(1, y, on)
    t2 = torch.full((y.shape[0], num_classes), off, device=y.device, dtype=torch.float32).scatter_(1, y.flip(0), on)
    return t1 * lam + t2 * oml


class MixedLabels:
    """What the fused loss needs instead of a [B,C] target: the int64 labels, the DEVICE mix record (int32 [8]; only lam
    and 1 - lam are read), the smoothed one-hot values and C.  `losses.cross_entropy` / `VideoImageLoss` take it."""

    def __init__(self, labels, record, on, off, num_classes):
        if labels.dtype != torch.int64 or labels.dim() != 1:
            raise ValueError("MixedLabels needs int64 [B] labels, got %s %s" % (labels.dtype, tuple(labels.shape)))
        if record.dtype != torch.int32 or record.numel() != 8:
            raise ValueError("the mix record is int32 [8]")
        self.labels, self.record = labels, record
        self.on, self.off, self.num_classes = float(on), float(off), int(num_classes)

    def dense(self):
        """the [B,C] soft target the reference would have built (on the labels' device; no host sync)"""
        lam, oml = self.record.to(self.labels.device)[1:3].view(torch.float32).unbind(0)
        return dense_target(self.labels, self.num_classes, lam, oml, self.on, self.off)


class MixUp:
    """The reference's constructor surface and call; see the module docstring for the fused route."""

    def __init__(self, mixup_alpha=1.0, cutmix_alpha=0.0, mix_prob=1.0, switch_prob=0.5, correct_lam=True,
                 label_smoothing=0.1, num_classes=1000):
        if isinstance(num_classes, dict):
            raise NotImplementedError("dict-valued num_classes (the Epic-Kitchens noun / verb heads) is not supported")
        self.mixup_alpha, self.cutmix_alpha = mixup_alpha, cutmix_alpha
        self.mix_prob, self.switch_prob = mix_prob, switch_prob
        self.correct_lam = correct_lam
        self.label_smoothing = label_smoothing
        self.num_classes = int(num_classes)

    # ---- the draw (host, global np.random stream, the reference's order) ----------------------
    def draw(self, shape):
        """One step's MixRecord for a batch of `shape` ([..., H, W]).  Consumes np.random as the reference does: rand()
        against mix_prob; rand() against switch_prob only when both alphas are > 0; beta(a, a); for CutMix randint for
        the box centre's y, then x."""
        lam, cutmix = 1.0, False
        if np.random.rand() < self.mix_prob:
            if self.mixup_alpha > 0.0 and self.cutmix_alpha > 0.0:
                cutmix = bool(np.random.rand() < self.switch_prob)
            elif self.cutmix_alpha > 0.0:
                cutmix = True
            elif not self.mixup_alpha > 0.0:
                raise ValueError("MixUp with mix_prob > 0 needs mixup_alpha > 0 or cutmix_alpha > 0")
            a = self.cutmix_alpha if cutmix else self.mixup_alpha
            lam = float(np.random.beta(a, a))
        if lam == 1.0:
            return NO_MIX
        if not cutmix:
            return MixRecord(MODE_MIXUP, lam, 0, 0, 0, 0)
        H, W = int(shape[-2]), int(shape[-1])
        ratio = math.sqrt(1 - lam)
        cut_h, cut_w = int(H * ratio), int(W * ratio)
        cy = int(np.random.randint(0, H))
        cx = int(np.random.randint(0, W))
        yl, yh = min(max(cy - cut_h // 2, 0), H), min(max(cy + cut_h // 2, 0), H)
        xl, xh = min(max(cx - cut_w // 2, 0), W), min(max(cx + cut_w // 2, 0), W)
        if self.correct_lam:
            lam = 1.0 - (yh - yl) * (xh - xl) / float(H * W)
        return MixRecord(MODE_CUTMIX, float(lam), yl, yh, xl, xh)

    # ---- applying a record ---------------------------------------------------------------------
    @staticmethod
    def _mix_host(x, rec):
        """plain torch ops (host tensors, or any tensor the kernel does not take): what the reference does"""
        if rec.mode == MODE_CUTMIX:
            yl, yh, xl, xh = rec.box
            x[..., yl:yh, xl:xh] = x.flip(0)[..., yl:yh, xl:xh]
        elif rec.mode == MODE_MIXUP:
            partner = x.flip(0) * (1.0 - rec.lam)
            x.mul_(rec.lam).add_(partner)
        return x

    def _mix_tensor(self, x, rec, dev_rec=None):
        if x.is_cuda and x.dtype == torch.float32:
            from . import ops
            if not x.is_contiguous():
                raise hip.SvitHipError("MixUp mixes in place: the device clip must be contiguous")
            if dev_rec is None:
                dev_rec = torch.from_numpy(rec.pack()).to(x.device)
            ops.mixup_clips(x, dev_rec)
            return x
        return self._mix_host(x, rec)

    def __call__(self, x, target):
        """The reference's call: mixes x in place, returns (x, dense [B,C] f32 target)."""
        assert len(x) > 1, "Batch size should be greater than 1 for mixup."
        if isinstance(target, dict):
            raise NotImplementedError("dict-valued targets (Epic-Kitchens) are not supported")
        rec = self.draw(x.shape)
        self._mix_tensor(x, rec)
        on, off = smoothed_one_hot_values(self.label_smoothing, self.num_classes)
        return x, dense_target(target, self.num_classes, rec.lam, 1.0 - rec.lam, on, off)

    def labels(self, labels, dev_rec):
        """MixedLabels over `labels` and a device record (GraphedTrainStep: its static buffers)"""
        on, off = smoothed_one_hot_values(self.label_smoothing, self.num_classes)
        return MixedLabels(labels, dev_rec, on, off, self.num_classes)

    def mix(self, x, labels, record=None):
        """The fused route: uploads the record (drawn now unless given), mixes an fp32 clip tensor in place -- or tags a
        U8Clips / AugClips, whose im2col then mixes between normalisation and bf16 rounding -- and returns (x, MixedLabels)."""
        from .augment import AugClips
        from .input import U8Clips
        assert x.shape[0] > 1, "Batch size should be greater than 1 for mixup."
        rec = self.draw(x.shape) if record is None else record
        dev_rec = torch.from_numpy(rec.pack()).to(labels.device)
        if isinstance(x, (U8Clips, AugClips)):
            x.lut_f32                         # (built here, outside any capture)
            x.mix = dev_rec.to(x.device)
        else:
            self._mix_tensor(x, rec, dev_rec if dev_rec.device == x.device else None)
        return x, self.labels(labels, dev_rec)


def build_mixup(cfg):
    """MixUp from cfg.MIXUP.* and cfg.MODEL.NUM_CLASSES, or None when the tree has no MIXUP section (it is not a key of
    this build's default tree; the reference's yaml brings it) or MIXUP.ENABLE is false."""
    m = getattr(cfg, "MIXUP", None)
    if m is None or not getattr(m, "ENABLE", False):
        return None
    return MixUp(mixup_alpha=getattr(m, "ALPHA", 0.8), cutmix_alpha=getattr(m, "CUTMIX_ALPHA", 1.0),
                 mix_prob=getattr(m, "PROB", 1.0), switch_prob=getattr(m, "SWITCH_PROB", 0.5),
                 label_smoothing=getattr(m, "LABEL_SMOOTH_VALUE", 0.1), num_classes=cfg.MODEL.NUM_CLASSES)
