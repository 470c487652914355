"""svit_amd/augment.py on the host: the sampler reproduces the reference's draws (tests/golden/augment.npz, written by
tools/gen_augment_golden.py from the unmodified reference), records pack and validate.  No GPU."""
import os
import random

import numpy as np
import pytest
import torch

from svit_amd import augment
from svit_amd.augment import AugRecord, SpatialSampler, build_sampler
from svit_amd.config import CfgNode, ssv2_cfg

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module")
def gold():
    return dict(np.load(os.path.join(GOLDEN, "augment.npz")))


def set_cfg(gold, s):
    """the cfg of parameter set s: ssv2_cfg() + what the set changes (AUG only where the set has it)"""
    cfg = ssv2_cfg()
    d = cfg.DATA
    d.TRAIN_JITTER_SCALES = [int(v) for v in gold["set_scales"][s]]
    d.RANDOM_FLIP, d.INV_UNIFORM_SAMPLE = bool(gold["set_flip"][s]), bool(gold["set_inv"][s])
    d.TRAIN_CROP_SIZE = int(gold["crop"])
    assert list(d.TRAIN_JITTER_SCALES_RELATIVE) == list(gold["rel_scale"])
    assert list(d.TRAIN_JITTER_ASPECT_RELATIVE) == list(gold["rel_aspect"])
    if gold["set_aug"][s]:
        cfg.AUG = CfgNode({"ENABLE": True, "RE_PROB": float(gold["set_re_prob"][s]), "RE_MODE": str(gold["set_re_mode"][s]),
                           "RE_COUNT": 1})
    return cfg


def replay(gold, s, k, sampler):
    """seed both streams as the generator did, draw -> (record, trace, random tail, np tail)"""
    Hs, Ws = (int(v) for v in gold["sizes"][k % len(gold["sizes"])])
    random.seed(k)
    np.random.seed(k)
    rec = sampler.draw(Hs, Ws, video=3)
    return rec, dict(sampler.trace), random.random(), np.random.uniform()


def test_sets_are_the_ones_the_issue_names(gold):
    assert list(gold["set_names"]) == ["ssv2", "jitter", "flip", "const", "jitter_inv"]
    assert gold["draws"].shape[:2] == (5, 32)
    # the first set is the shipped yaml: its AUG / DATA values come out of the file itself
    cfg = ssv2_cfg()
    cfg.merge_from_file(os.path.join(GOLDEN, "ssv2.yaml"))
    assert cfg.AUG.RE_PROB == gold["set_re_prob"][0] and cfg.AUG.RE_MODE == gold["set_re_mode"][0] and cfg.AUG.ENABLE
    assert cfg.DATA.RANDOM_FLIP == bool(gold["set_flip"][0])
    assert list(cfg.DATA.TRAIN_JITTER_SCALES_RELATIVE) == list(gold["rel_scale"])
    assert list(cfg.DATA.TRAIN_JITTER_ASPECT_RELATIVE) == list(gold["rel_aspect"])
    a, b = build_sampler(cfg), build_sampler(set_cfg(gold, 0))
    assert vars(a) == vars(b)


@pytest.mark.parametrize("s", range(5))
def test_sampler_reproduces_the_reference_draws(gold, s):
    keys = list(gold["keys"])
    sampler = build_sampler(set_cfg(gold, s), "train")
    noise = str(gold["set_re_mode"][s]) in ("rand", "pixel")
    for k in range(gold["draws"].shape[1]):
        g = dict(zip(keys, (int(v) for v in gold["draws"][s, k])))
        rec, trace, r_tail, np_tail = replay(gold, s, k, sampler)
        assert rec.video == 3
        got = rec._asdict()
        for name in ("i", "j", "h", "w", "out_h", "out_w", "oy", "ox", "flip", "et", "el", "eh", "ew"):
            assert got[name] == g[name], (s, k, name, got, g)
        assert (rec.erase_mode != 0) == bool(g["erased"]), (s, k)
        if g["erased"]:
            assert rec.erase_mode == augment.ERASE_MODES[str(gold["set_re_mode"][s])]
        # both streams stand where the reference left them -- plus the ONE documented extra draw, the noise seed
        ref_r, ref_np, ref_seed, ref_r_after_seed = gold["tail"][s, k]
        assert np_tail == ref_np, (s, k)
        if g["erased"] and noise:
            assert rec.seed == int(ref_seed) and r_tail == ref_r_after_seed, (s, k)
        else:
            assert rec.seed == 0 and r_tail == ref_r, (s, k)
        assert bool(trace.get("fallback", False)) == bool(g["fallback"]), (s, k)
        assert bool(trace.get("jitter_identity", False)) == bool(g["jitter_identity"]), (s, k)


def test_fixture_keeps_the_rare_branches(gold):
    """the central fallback of _get_param_spatial_crop, a success after several tries, the jitter's short side == size
    early return, the crop that draws one offset only, flips both ways, erased and not erased"""
    d = {k: gold["draws"][..., c] for c, k in enumerate(gold["keys"])}
    rrc = gold["set_aug"].astype(bool)
    assert d["fallback"][rrc].any() and not d["fallback"][~rrc].any()
    assert d["jitter_identity"][1].any() and not d["jitter_identity"][rrc].any()
    ident = d["jitter_identity"][1].astype(bool)
    assert ((d["out_h"][1][ident] == int(gold["crop"])) & (d["oy"][1][ident] == 0)).all()      # no y draw there
    assert d["flip"][2].any() and (d["flip"][2] == 0).any() and d["flip"][4].any() and (d["flip"][4] == 0).any()
    assert not d["flip"][0].any() and not d["flip"][1].any()
    assert d["erased"][0].any() and (d["erased"][0] == 0).any() and d["erased"][3].all()
    assert not d["erased"][1].any() and not d["erased"][4].any()
    # the sampler walks the same branches (trace) -- and a several-tries success occurs
    sampler = build_sampler(set_cfg(gold, 0))
    tries = [replay(gold, 0, k, sampler)[1]["tries"] for k in range(32)]
    assert max(t for t, f in zip(tries, d["fallback"][0]) if not f) > 1
    assert all(t == 10 for t, f in zip(tries, d["fallback"][0]) if f)


def test_fallback_formula_all_three_cases():
    sp = SpatialSampler(8, scale=(4.0, 5.0), aspect=(0.75, 1.3333), random_flip=False)    # area > frame: every try fails
    random.seed(0)
    np.random.seed(0)
    assert sp.draw(30, 90)[1:5] == (0, 25, 30, 40) and sp.trace["fallback"]      # wide: h = H, w = round(H * 1.3333)
    assert sp.draw(90, 30)[1:5] == (25, 0, 40, 30)                                # tall: w = W, h = round(W / 0.75)
    assert sp.draw(30, 32)[1:5] == (0, 0, 30, 32)                                 # in range: the whole frame


def test_test_mode_uniform_crop():
    cfg = ssv2_cfg()
    sp = build_sampler(cfg, "test")
    S = cfg.DATA.TEST_CROP_SIZE
    np.random.seed(5)
    fourth = np.random.uniform(size=4)[3]
    np.random.seed(5)
    recs = [sp.draw(240, 320, video=1, spatial_idx=i) for i in range(3)]
    assert np.random.uniform() == fourth           # one (degenerate) jitter-size uniform per draw, as the reference
    new_w = int(np.floor(320 / 240 * S))
    assert [r[1:7] for r in recs] == [(0, 0, 240, 320, S, new_w)] * 3
    assert [(r.oy, r.ox) for r in recs] == [(0, 0), (0, int(np.ceil((new_w - S) / 2))), (0, new_w - S)]
    tall = [sp.draw(320, 240, spatial_idx=i) for i in range(3)]
    assert [(r.oy, r.ox) for r in tall] == [(0, 0), (int(np.ceil((new_w - S) / 2)), 0), (new_w - S, 0)]
    assert all(r.flip == 0 and r.erase_mode == 0 for r in recs + tall)


def test_build_sampler_with_and_without_aug_node():
    cfg = ssv2_cfg()
    assert "AUG" not in cfg                                   # not a key of the default tree
    plain = build_sampler(cfg)
    assert plain.scale is None and plain.re_prob == 0.0 and plain.size == cfg.DATA.TRAIN_CROP_SIZE
    assert (plain.min_scale, plain.max_scale) == tuple(cfg.DATA.TRAIN_JITTER_SCALES)
    cfg.AUG = CfgNode({"ENABLE": True})                       # the reference's defaults for what the node leaves out
    on = build_sampler(cfg)
    assert on.scale == (0.08, 1.0) and on.aspect == (0.75, 1.3333)
    assert on.re_prob == 0.25 and on.re_mode == augment.ERASE_PIXEL
    assert build_sampler(cfg, "val").scale is None            # AUG applies to "train" only
    cfg.AUG.ENABLE = False
    assert build_sampler(cfg).scale is None
    cfg.AUG = CfgNode({"ENABLE": True, "RE_COUNT": 2})
    with pytest.raises(NotImplementedError):
        build_sampler(cfg)
    cfg.AUG = CfgNode({"ENABLE": True})
    cfg.DATA.TRAIN_JITTER_MOTION_SHIFT = True
    with pytest.raises(NotImplementedError):
        build_sampler(cfg)


def test_record_packing_round_trips():
    rec = AugRecord(2, 3, 5, 17, 19, 32, 40, 1, 8, 1, 3, 4, 6, 7, 9, 0x7FFFFFFF)
    words = rec.pack()
    assert words.dtype == np.int32 and words.shape == (16,) and words.nbytes == 64
    assert list(words) == list(rec)
    assert AugRecord.unpack(words) == rec
    table = augment.pack_records([rec, AugRecord.identity(1, 4, 6, 32)])
    assert table.dtype == torch.int32 and tuple(table.shape) == (2, 16)
    assert augment.unpack_records(table) == [rec, AugRecord(1, 4, 6, 32, 32, 32, 32, 0, 0, 0, 0, 0, 0, 0, 0, 0)]
    assert torch.equal(augment.pack_records(table.numpy()), table) and torch.equal(augment.pack_records(table), table)
    with pytest.raises(ValueError):
        augment.pack_records(np.zeros((2, 15), dtype=np.int32))


def test_validation_rejects_what_lies_outside():
    V, Hs, Ws, S = 2, 40, 56, 32
    good = AugRecord(1, 8, 24, 32, 32, 32, 32, 0, 0, 0, 1, 0, 0, 32, 32, 0)       # ends at the last row and column
    augment.validate_records(augment.pack_records([good]), V, Hs, Ws, S)
    assert torch.equal(augment.clamp_records(augment.pack_records([good]), V, Hs, Ws, S), augment.pack_records([good]))
    bad = {
        "rectangle past the bottom": good._replace(i=9),
        "rectangle past the right": good._replace(j=25),
        "negative origin": good._replace(i=-1),
        "empty rectangle": good._replace(h=0),
        "video": good._replace(video=2),
        "window past the resampled image": good._replace(oy=1),
        "resampled size": good._replace(out_w=0),
        "erase box": good._replace(el=1),
        "erase mode": good._replace(erase_mode=4),
    }
    for what, rec in bad.items():
        with pytest.raises(ValueError):
            augment.validate_records(augment.pack_records([good, rec]), V, Hs, Ws, S)
        # what the kernels make of it: the rectangle lies in the frame, and clamping again changes nothing
        once = augment.clamp_records(augment.pack_records([rec]), V, Hs, Ws, S)
        c = AugRecord.unpack(once[0])
        assert 0 <= c.video < V and c.h >= 1 and c.w >= 1 and 0 <= c.i <= Hs - c.h and 0 <= c.j <= Ws - c.w, what
        assert torch.equal(augment.clamp_records(once, V, Hs, Ws, S), once), what
