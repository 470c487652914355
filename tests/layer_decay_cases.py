"""Shared cases of the layer-wise lr decay tests (tests/test_layer_decay_cpu.py, tests/test_layer_decay_gpu.py): the
rule restated independently of svit_amd/lrscale.py, the named examples, and the table checks."""
import numpy as np

DEPTH = 16
DECAY = 0.75
LR_MULT = [["object_queries", 4.0], ["head.", 2.0]]
MAX_SEGS = 64

# name -> layer id at depth 16 (the issue's table)
EXAMPLES = {
    "cls_token": 0,
    "pos_embed_temporal": 0,
    "patch_embed.proj.bias": 0,
    "patch_embed.proj.weight": 0,
    "object_queries": DEPTH + 1,
    "blocks.0.norm1.weight": 1,
    "blocks.0.attn.qkv.weight": 1,
    "blocks.15.mlp.fc2.bias": 16,
    "blocks.15.attn.rel_pos_h": 16,
    "norm.weight": DEPTH + 1,
    "head.contact_mlp.bias": DEPTH + 1,
}


def layer_id(name, depth=DEPTH):
    top = name.split(".")[0]
    if top == "blocks":
        return int(name.split(".")[1]) + 1
    if top in ("cls_token", "patch_embed") or top[:9] == "pos_embed":
        return 0
    return depth + 1


def scale(name, decay=DECAY, mult=(), depth=DEPTH):
    """float32(decay ** (depth + 1 - layer id) * first matching factor), the product formed in Python doubles"""
    s = decay ** (depth + 1 - layer_id(name, depth))
    for prefix, factor in mult:
        if name[:len(prefix)] == prefix:
            s = s * factor
            break
    return np.float32(s)


def _align(n, a=8):
    return (n + a - 1) // a * a


def element_scales(slots, names, total, decay=DECAY, mult=()):
    """float32 [total]: the scale of every element of the slots of `names` (alignment padding included), 0 elsewhere"""
    out = np.zeros(total, dtype=np.float32)
    for n in names:
        off, numel = slots[n][0], slots[n][1]
        out[off:off + _align(numel)] = scale(n, decay, mult)
    return out


def check_table(segs, scales, want, n_decay):
    """the list of the issue's step 1 against `want` = element_scales(...) of the trainable names"""
    assert segs.dtype == np.int64 and segs.ndim == 2 and segs.shape[1] == 2 and segs.flags["C_CONTIGUOUS"]
    assert scales.dtype == np.float32 and scales.shape == (len(segs),)
    assert 1 <= len(segs) <= MAX_SEGS
    got = np.zeros_like(want)
    prev = 0
    for i, ((a, b), c) in enumerate(zip(segs, scales)):
        assert prev <= a < b <= len(want), "range %d not ascending / disjoint / non-empty" % i
        assert a % 4 == 0 and b % 4 == 0
        assert not (a < n_decay < b), "range %d crosses n_decay" % i
        assert np.isfinite(c) and c > 0
        if i and a == prev and a != n_decay:
            assert c != scales[i - 1], "ranges %d and %d touch, share a scale and a group and are not merged" % (i - 1, i)
        got[a:b] = c
        prev = b
    assert np.array_equal(got, want), "the union of the ranges is not the trainable slots, or a scale is misplaced"
