"""The host side of the captured evaluation steps (no GPU): evaluate.head_eval_host -- the float64 restatement of
svit_head_eval -- against SViTHead in eval mode, the bar the GPU test holds the kernel to (tests/eval_u8_cases.py), and
evaluate.test_views against the reference's uniform_crop rule."""
import math

import numpy as np
import pytest
import torch

from tests import eval_u8_cases as EC

# B = 3 clips, seven patch rows between the cls row and the T*O objects; C = 768 is the model's final width (the tiny
# configuration's too), C = 100 a width that is no multiple of a wave's 256-channel step
SHAPES = [dict(B=3, T=2, O=4, C=100, n_cls=174), dict(B=3, T=1, O=4, C=100, n_cls=5), dict(B=3, T=2, O=4, C=768, n_cls=174)]


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "T%(T)d-C%(C)d-cls%(n_cls)d" % s)
@pytest.mark.parametrize("act", [0, 1])
def test_host_restatement_equals_the_eval_head_in_float64(shape, act):
    from svit_amd.evaluate import head_eval_host
    B, T, O, C, n_cls = (shape[k] for k in ("B", "T", "O", "C", "n_cls"))
    tokens, params = EC.make_case(B, 1 + 7 + T * O, C, T, O, n_cls, seed=11)
    want = EC.aten_head(tokens, params, T, O, act, dtype=torch.float64)
    got = head_eval_host(tokens, params, T, O, act)
    for g, w in zip(got, want):
        assert g.dtype == np.float64 and g.shape == tuple(w.shape)
        assert float(np.abs(g - w.numpy()).max()) <= 1e-13
    assert np.array_equal(got[3], tokens[:, -T * O:].reshape(B, T, O, C).astype(np.float64))
    if act == 0:
        assert abs(got[0][B - 1, 0] - 1.0) < 1e-12          # the +120 row: a softmax that did not overflow
    assert all(np.isfinite(g).all() for g in got)
    assert EC.cold_outputs(got, n_cls, act) == [0.0] * (3 if act == 1 else 2)      # the -800 rows: 0, not NaN
    assert EC.cold_outputs(want, n_cls, act) == [0.0] * (3 if act == 1 else 2)
    with pytest.raises(ValueError):
        head_eval_host(tokens[:, :T * O], params, T, O, act)
    with pytest.raises(ValueError):
        head_eval_host(tokens, params, T, O, 2)


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "T%(T)d-C%(C)d-cls%(n_cls)d" % s)
def test_the_bar_passes_the_fp32_head_and_catches_every_mutant(shape):
    """the bar of tests/test_eval_u8_gpu.py, fixed without the kernel: 4 x the error of the stock fp32 eval head; the
    fp32 restatement sits inside it, every mutant at least 10 x above it"""
    from svit_amd.evaluate import head_eval_host
    B, T, O, C, n_cls = (shape[k] for k in ("B", "T", "O", "C", "n_cls"))
    tokens, params = EC.make_case(B, 1 + 7 + T * O, C, T, O, n_cls, seed=12)
    for act in (0, 1):
        want64 = head_eval_host(tokens, params, T, O, act)
        yard = EC.errors(EC.aten_head(tokens, params, T, O, act), want64)
        bars = EC.bar(yard)
        own = EC.errors(head_eval_host(tokens, params, T, O, act, dtype=np.float32), want64)
        print("act %d yardstick %s fp32 restatement %s" % (act, yard, own))
        assert all(math.isfinite(y) and y < 1e-5 for y in yard), yard
        assert all(e <= b for e, b in zip(own, bars)), (own, bars)
        for name in EC.MUTANTS:
            ratio = EC.caught(name, tokens, params, T, O, act, want64, bars)
            print("act %d mutant %s: %.3g x the bar" % (act, name, ratio))
            assert ratio >= 10.0, (name, act, ratio)


def test_test_views_follow_uniform_crop():
    """record order, `video` fields, clip ids and offsets of the test-time views at S = 64: landscape, portrait (new_h >
    new_w: the crops run top to bottom), square and a source that is rescaled (72x96 -> 64x85)"""
    from svit_amd import config
    from svit_amd.augment import build_sampler
    from svit_amd.evaluate import test_views, uniform_crop_offsets
    cfg = config.ssv2_cfg(num_frames=4, crop=64)
    sampler = build_sampler(cfg, "test")
    assert sampler.size == 64
    sizes = [(64, 88), (88, 64), (64, 64), (72, 96)]
    rescaled = [(64, 88), (88, 64), (64, 64), (64, 85)]
    records, ids = test_views(sampler, sizes, first_video=5, num_crops=3)
    assert len(records) == 12 and ids.dtype == torch.int64
    assert ids.tolist() == [(5 + v) * 3 + j for v in range(4) for j in range(3)]
    for v, ((h, w), (nh, nw)) in enumerate(zip(sizes, rescaled)):
        for s in range(3):
            rec = records[v * 3 + s]
            assert rec.video == v and (rec.i, rec.j, rec.h, rec.w) == (0, 0, h, w)
            assert (rec.out_h, rec.out_w) == (nh, nw)
            assert (rec.oy, rec.ox) == uniform_crop_offsets(nh, nw, 64, s)
            assert rec.flip == 0 and rec.erase_mode == 0
    assert [r.oy for r in records[3:6]] == [0, 12, 24] and [r.ox for r in records[0:3]] == [0, 12, 24]
    centre, ids1 = test_views(sampler, sizes, first_video=5, num_crops=1)
    assert ids1.tolist() == [5, 6, 7, 8] and [r.video for r in centre] == [0, 1, 2, 3]
    for rec, (nh, nw) in zip(centre, rescaled):
        assert (rec.oy, rec.ox) == uniform_crop_offsets(nh, nw, 64, 1)
