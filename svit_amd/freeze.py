"""Frozen parameters (`requires_grad = False`): which sets the engine supports and what they mean for the flat buffers.

The reference leaves such parameters out of the optimizer (slowfast/models/optimizer.py:39-76), autograd gives them no
gradient and stops where nothing below needs one.  Here the supported sets are exactly "everything below a cut" in
network order:

    position 0          stem: patch_embed.proj.*, cls_token, object_queries, pos_embed_temporal
    position 1 + i      block i
    position depth + 1  norm.*
    position depth + 2  head.*

`cut` = the lowest trainable position; cut 0 freezes nothing.  The flat layout orders each weight-decay group by
gradient-readiness rank (head and final norm, blocks depth-1 .. 0, stem), so the trainable set of a cut is a couple of
contiguous ranges: the segment table the optimizer tail and the gradient exchange work on.  Host code only.
"""
import numpy as np

MAX_SEGS = 64       # SVIT_MAX_SEGS of include/svit_hip.h


def position(name, depth):
    """network position of a parameter (see the module text)"""
    if name.startswith("head."):
        return depth + 2
    if name.startswith("norm."):
        return depth + 1
    if name.startswith("blocks."):
        return 1 + int(name.split(".")[1])
    return 0


def find_cut(flags, depth):
    """flags: (name, requires_grad) pairs in named_parameters() order -> the cut they describe.
    ValueError (torch.optim.AdamW's, for an empty parameter list) when nothing is trainable; NotImplementedError
    naming the first parameter whose flag does not fit "everything below a cut is frozen, the rest is not"."""
    flags = [(n, bool(r)) for n, r in flags]
    trainable = [position(n, depth) for n, r in flags if r]
    if not trainable:
        raise ValueError("optimizer got an empty parameter list")
    cut = min(trainable)
    for n, r in flags:
        if r != (position(n, depth) >= cut):
            raise NotImplementedError(
                "svit_amd supports frozen parameters only as \"everything below a cut\" (stem, blocks 0..k-1 [, norm]), "
                "whole positions: %s has requires_grad=%s while position %d is the lowest trainable one"
                % (n, r, cut))
    return cut


def model_cut(model):
    """the cut the flags of an SViT describe right now"""
    return find_cut(((n, p.requires_grad) for n, p in model.named_parameters()), len(model.plan.blocks))


def trainable_names(names, depth, cut):
    return [n for n in names if position(n, depth) >= cut]


def segments(slots, n_decay, names, align=8):
    """int64 numpy [S, 2]: the slots of `names` with their alignment padding as sorted, disjoint (begin, end) ranges of
    the flat buffers, adjacent ones merged, none crossing n_decay (slots themselves never do)."""
    spans = sorted((slots[n][0], slots[n][0] + (slots[n][1] + align - 1) // align * align) for n in names)
    out = []
    for a, b in spans:
        if out and out[-1][1] == a and a != n_decay:
            out[-1][1] = b
        else:
            out.append([a, b])
    if not 1 <= len(out) <= MAX_SEGS:
        raise NotImplementedError("the trainable parameters form %d ranges of the flat buffer; 1..%d are supported"
                                  % (len(out), MAX_SEGS))
    return np.array(out, dtype=np.int64).reshape(-1, 2)


def intersect(ranges, segs):
    """the parts of the (begin, end) `ranges` that lie inside the segment table"""
    out = []
    for a, b in ranges:
        for s, e in segs:
            lo, hi = max(a, int(s)), min(b, int(e))
            if lo < hi:
                out.append((lo, hi))
    return out


def complement(segs, total):
    """the (begin, end) ranges of [0, total) outside the segment table: the frozen part"""
    out, at = [], 0
    for s, e in segs:
        if int(s) > at:
            out.append((at, int(s)))
        at = int(e)
    if at < total:
        out.append((at, total))
    return out
