"""Per-range learning-rate scales of the fused optimizer tails: layer-wise lr decay (`cfg.SOLVER.LAYER_DECAY`) and
per-prefix multipliers (`cfg.SVIT.LR_MULT`).

    layer id 0          cls_token, pos_embed*, patch_embed*
    layer id 1 + i      blocks.i.*
    layer id depth + 1  everything else: norm.*, head.*, object_queries

    scale(name) = LAYER_DECAY ** (depth + 1 - layer_id(name)) * mult(name)       (Python doubles, rounded once to fp32)

`object_queries` sits with the head on purpose (freeze.position puts it with the stem): a freshly initialised token
must not get the smallest step.  The flat buffers are laid out [decayed | not decayed], each in readiness order, so
every (scale, weight-decay group) is a handful of contiguous ranges: the table svit_adamw_step_guarded_lr carries in
its kernel arguments.  Host code only.
"""
import math

import numpy as np

from . import freeze


def layer_id(name, depth):
    if name == "cls_token" or name.startswith("pos_embed") or name.startswith("patch_embed"):
        return 0
    if name.startswith("blocks."):
        return 1 + int(name.split(".")[1])
    return depth + 1


def check_layer_decay(value):
    d = float(value)
    if not (math.isfinite(d) and 0.0 < d <= 1.0):
        raise ValueError("SOLVER.LAYER_DECAY must be finite and in (0, 1], got %r" % (value,))
    return d


def check_multipliers(pairs):
    out = []
    for pair in pairs or ():
        if len(pair) != 2 or not isinstance(pair[0], str):
            raise ValueError("SVIT.LR_MULT is a list of [prefix, factor] pairs, got %r" % (pair,))
        f = float(pair[1])
        if not (math.isfinite(f) and f > 0.0):
            raise ValueError("SVIT.LR_MULT: the factor of %r must be finite and > 0, got %r" % (pair[0], pair[1]))
        out.append((pair[0], f))
    return tuple(out)


def make_scale(depth, layer_decay=1.0, lr_mult=()):
    """name -> scale as a Python double"""
    decay, mults = check_layer_decay(layer_decay), check_multipliers(lr_mult)

    def scale(name):
        s = decay ** (depth + 1 - layer_id(name, depth))
        for prefix, f in mults:
            if name.startswith(prefix):
                return s * f
        return s
    return scale


def lr_scale_from_cfg(cfg):
    """the `lr_scale` callable of the optimizers from cfg.SOLVER.LAYER_DECAY (default 1.0) and cfg.SVIT.LR_MULT (default
    none), neither a key of the default tree; None when they say nothing"""
    decay = check_layer_decay(getattr(cfg.SOLVER, "LAYER_DECAY", 1.0))
    mults = check_multipliers(getattr(cfg.SVIT, "LR_MULT", ()))
    if decay == 1.0 and not mults:
        return None
    return make_scale(cfg.MVIT.DEPTH, decay, mults)


def name_scales(names, lr_scale):
    """{name: np.float32 scale}; ValueError for a scale that is not finite and > 0"""
    out = {}
    for n in names:
        s = np.float32(lr_scale(n))
        if not (np.isfinite(s) and s > 0):
            raise ValueError("lr_scale(%r) = %r: a scale must be finite and > 0 in fp32" % (n, lr_scale(n)))
        out[n] = s
    return out


def table(slots, n_decay, scales, trainable=None, align=8):
    """(segs int64 [S, 2], scales float32 [S]) of the flat buffers, or None when every trainable scale is 1.0.
    slots: FlatParams.slots; scales: name_scales(); trainable: the segment table of a frozen cut, or None.
    A slot covers its alignment padding (as freeze.segments has it); neighbours with equal (scale, weight-decay group)
    merge; under a cut the ranges are intersected with the trainable segments.  Ascending, disjoint, every bound a
    multiple of 4, none across n_decay, the union exactly the trainable slots."""
    ranges = []                                          # [begin, end, scale]
    for n in sorted(slots, key=lambda k: slots[k][0]):
        a = slots[n][0]
        b = a + (slots[n][1] + align - 1) // align * align
        s = scales[n]
        if ranges and ranges[-1][1] == a and ranges[-1][2] == s and a != n_decay:
            ranges[-1][1] = b
        else:
            ranges.append([a, b, s])
    if trainable is not None:
        ranges = [[lo, hi, s] for a, b, s in ranges for lo, hi in freeze.intersect([(a, b)], trainable)]
    if all(r[2] == np.float32(1.0) for r in ranges):
        return None
    if len(ranges) > freeze.MAX_SEGS:
        raise NotImplementedError("the learning-rate scales form %d ranges of the flat buffer; at most %d are supported"
                                  % (len(ranges), freeze.MAX_SEGS))
    segs = np.array([r[:2] for r in ranges], dtype=np.int64).reshape(-1, 2)
    return np.ascontiguousarray(segs), np.array([r[2] for r in ranges], dtype=np.float32)
