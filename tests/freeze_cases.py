"""Shared cases of the frozen-parameter tests (tests/test_freeze_cpu.py, tests/test_freeze_gpu.py): the cuts, the
unsupported patterns of `requires_grad` flags with the parameter each refusal must name, and the flat-buffer masks
the segment checks compare."""
import numpy as np

DEPTH = 16
# 7 is no multiple of the engine's RED_GROUP (4); DEPTH + 1 = final norm + head, DEPTH + 2 = head only
CUTS_CPU = (0, 1, 4, 7, DEPTH + 1, DEPTH + 2)
CUTS_GPU = (1, 4, 7, DEPTH + 1, DEPTH + 2)

STEM = ("patch_embed.proj.weight", "patch_embed.proj.bias", "cls_token", "object_queries", "pos_embed_temporal")


def position(name, depth=DEPTH):
    """network position as the issue's table gives it (written out here independently of svit_amd/freeze.py)"""
    if name in STEM:
        return 0
    head = name.split(".")[0]
    if head == "blocks":
        return 1 + int(name.split(".")[1])
    return {"norm": depth + 1, "head": depth + 2}[head]


def flags_for_cut(names, cut, depth=DEPTH):
    return {n: position(n, depth) >= cut for n in names}


def unsupported_patterns(names, depth=DEPTH):
    """[(label, {name: requires_grad}, the first offending parameter in named_parameters() order)]"""
    out = []
    f = {n: not n.startswith("blocks.5.") for n in names}
    out.append(("one block frozen in the middle", f, "blocks.5.norm1.weight"))
    f = {n: not n.startswith("patch_embed.") for n in names}
    out.append(("patch_embed without the tokens", f, "patch_embed.proj.weight"))
    f = {n: not n.startswith("norm.") for n in names}
    out.append(("norm frozen under trainable blocks", f, "norm.weight"))
    f = {n: n != "blocks.3.attn.qkv.weight" for n in names}
    out.append(("a single tensor", f, "blocks.3.attn.qkv.weight"))
    f = flags_for_cut(names, 4, depth)
    f["blocks.3.mlp.fc2.bias"] = False
    out.append(("a position frozen in part", f, "blocks.3.mlp.fc2.bias"))
    f = flags_for_cut(names, 4, depth)
    f["blocks.1.norm2.weight"] = True
    # the lowest trainable position is block 1 then: the first parameter that does not fit is block 1's first frozen one
    out.append(("a trainable tensor below the cut", f, "blocks.1.norm1.weight"))
    return out


def _align(n, a=8):
    return (n + a - 1) // a * a


def slot_mask(slots, names, total):
    """bool [total]: the slots of `names` with their alignment padding"""
    m = np.zeros(total, dtype=bool)
    for n in names:
        off, numel = slots[n][0], slots[n][1]
        m[off:off + _align(numel)] = True
    return m


def seg_mask(segs, total):
    m = np.zeros(total, dtype=bool)
    for a, b in segs:
        assert not m[a:b].any(), "segments overlap"
        m[a:b] = True
    return m
