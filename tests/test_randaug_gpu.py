"""The RandAugment kernels (csrc/randaug.hip) against PIL's recorded bytes (tests/golden/randaug.npz) and against
`randaug.apply_host`, byte for byte; the chain inside AugClips and a captured step.  Shapes are the fixture's 24 x 32 and
32 x 24, 17 x 23 (row bytes no multiple of 4) and 70 x 150 (42 blocks of 256 pixels per frame, the last one partial)."""
import os
import random

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import procedural as P
from tests import randaug_cases as C
from tests import smoke_impl as SM

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module")
def ra():
    from svit_amd import hip, randaug
    hip.load()
    return randaug


@pytest.fixture(scope="module")
def gold():
    return dict(np.load(os.path.join(GOLDEN, "randaug.npz")))


def device_apply(ra, src_np, table):
    """the 2N kernels on a NumPy clip -> NumPy; dst and tmp start poisoned, src must come back unchanged"""
    table = ra.pack_table(table)
    src = torch.from_numpy(np.ascontiguousarray(src_np)).cuda()
    keep = src.clone()
    dst, tmp = torch.full_like(src, 77), torch.full_like(src, 99)
    ws = torch.zeros(ra.workspace_bytes(src.shape[0], src.shape[1]), dtype=torch.uint8, device="cuda")
    out = ra.apply(src, torch.from_numpy(table).cuda(), dst, tmp if table.shape[1] > 1 else None, ws)
    torch.cuda.synchronize()
    assert out is dst and torch.equal(src, keep)
    return dst.cpu().numpy()


def diff(a, b):
    return int((a != b).sum())


@pytest.mark.parametrize("si", range(2))
def test_single_operations_equal_pil(ra, gold, si):
    """every case in ONE launch pair: the cases are the videos of a [cases,1,H,W,3] clip over the same frame"""
    one = C.single_source(si)
    Hs, Ws = one.shape[2:4]
    cases = C.single_cases(si)
    src = np.repeat(one, len(cases), axis=0)
    table = [[ra.make_op(name, args, () if filt is None else (filt,), Hs, Ws)] for name, args, filt in cases]
    got = device_apply(ra, src, table)
    for k, case in enumerate(cases):
        assert np.array_equal(got[k, 0], gold["single_%d" % si][k]), (case, diff(got[k, 0], gold["single_%d" % si][k]))


def test_special_frames_equal_pil(ra, gold):
    """identity tables on a single colour, Equalize step == 0, the Equalize quotient of 256 that PIL clamps"""
    sp = C.special_frames()
    for j, op in enumerate((ra.OP_AUTOCONTRAST, ra.OP_EQUALIZE)):
        got = device_apply(ra, sp, [[ra.RandAugOp(op)]] * 3)
        for f in range(3):
            assert np.array_equal(got[f, 0], gold["special"][f, j]), (f, op)


@pytest.mark.parametrize("s", range(len(C.SETS)))
def test_chains_equal_pil(ra, gold, s):
    aa, interp = C.SETS[s]
    sampler = ra.RandAugSampler(aa, interp)
    for k in range(C.N_CHAINS):
        src = C.source(C.SHAPES[k % 2])[k % 2:k % 2 + 1]
        random.seed(k)
        np.random.seed(k)
        ops = sampler.draw(*src.shape[1:4])
        got = device_apply(ra, src, [ops])[0]
        ref = gold["chain_%d_%d" % (s, k)]
        assert np.array_equal(got, ref), (s, k, sampler.trace, diff(got, ref))


def _mixed_table(ra, Hs, Ws):
    """two videos, different operations in every layer, a mixed bicubic_mask across the frames"""
    rot = ra.rotate_matrix(-17.3, Ws, Hs)
    return [
        [ra.RandAugOp(ra.OP_AFFINE, bicubic_mask=0b101, m=rot), ra.RandAugOp(ra.OP_EQUALIZE),
         ra.make_op("SharpnessIncreasing", (1.63,), (), Hs, Ws), ra.make_op("ShearX", (-0.21,), (1, 0, 0), Hs, Ws)],
        [ra.make_op("ContrastIncreasing", (0.37,), (), Hs, Ws), ra.make_op("TranslateYRel", (0.315,), (0, 1, 1), Hs, Ws),
         ra.RandAugOp(ra.OP_AUTOCONTRAST), ra.make_op("ColorIncreasing", (1.81,), (), Hs, Ws)],
    ]


@pytest.mark.parametrize("N", [1, 2, 3, 4])
def test_every_layer_count_lands_in_dst(ra, N):
    src = C.source(C.SHAPES[0])
    table = [layers[:N] for layers in _mixed_table(ra, 24, 32)]
    want = ra.apply_host(src, table)
    assert diff(want, src) > 0
    got = device_apply(ra, src, table)          # (asserts src unchanged and that the result is dst)
    assert np.array_equal(got, want), diff(got, want)


@pytest.mark.parametrize("shape", [(1, 2, 17, 23, 3), (1, 1, 70, 150, 3)])
def test_odd_shapes_equal_apply_host(ra, shape):
    src = C.source(shape)
    Hs, Ws = shape[2:4]
    T = shape[1]
    tables = [[[ra.make_op(name, args, () if filt is None else (filt,) * T, Hs, Ws)]] for name, args, filt in C.single_cases()]
    tables.append([_mixed_table(ra, Hs, Ws)[0]])
    tables.append([_mixed_table(ra, Hs, Ws)[1]])
    # one launch pair for all the single cases: the cases as videos
    singles = [t[0] for t in tables[:-2]]
    big = np.repeat(src, len(singles), axis=0)
    want, got = ra.apply_host(big, singles), device_apply(ra, big, singles)
    for k in range(len(singles)):
        assert np.array_equal(got[k], want[k]), (C.single_cases()[k], diff(got[k], want[k]))
    for t in tables[-2:]:
        want, got = ra.apply_host(src, t), device_apply(ra, src, t)
        assert np.array_equal(got, want), diff(got, want)


def test_any_record_is_safe(ra):
    """op = 99 is NONE; coefficients of +-1e300 and NaN give the fill everywhere -- and what apply_host gives"""
    src = C.source((1, 2, 17, 23, 3))
    nan, big = float("nan"), 1e300
    recs = [ra.RandAugOp(99), ra.RandAugOp(-1)]
    for m in ((big, 0, 0, 0, big, 0), (-big, 0, 0, 0, -big, 0), (nan,) * 6, (1, 0, nan, 0, 1, 0), (1, 0, 0, 0, 1, big),
              (big, -big, 0, 0, 1, 0)):
        recs += [ra.RandAugOp(ra.OP_AFFINE, bicubic_mask=mask, m=m) for mask in (0, 3)]
    recs += [ra.RandAugOp(ra.OP_POSTERIZE, arg_i=-5), ra.RandAugOp(ra.OP_POSTERIZE, arg_i=2 ** 31 - 1),
             ra.RandAugOp(ra.OP_SOLARIZE, arg_i=-2 ** 31), ra.RandAugOp(ra.OP_SOLARIZE_ADD, arg_i=2 ** 31 - 1),
             ra.RandAugOp(ra.OP_BRIGHTNESS, arg_f=nan), ra.RandAugOp(ra.OP_COLOR, arg_f=3e38),
             ra.RandAugOp(ra.OP_SHARPNESS, arg_f=-3e38)]
    table = [[r] for r in recs]
    clip = np.repeat(src, len(recs), axis=0)
    want, got = ra.apply_host(clip, table), device_apply(ra, clip, table)
    assert np.array_equal(got[0], src[0]) and np.array_equal(got[1], src[0])
    for k in range(2, 12):
        assert (got[k] == 128).all(), recs[k]
    for k in range(len(recs)):
        assert np.array_equal(got[k], want[k]), (recs[k], diff(got[k], want[k]))


def test_entry_points_refuse_bad_arguments(ra):
    from svit_amd import hip
    lib = hip.load()
    assert lib.svit_randaug_stats(None, None, 0, None, 1, 1, 8, 8, 1, None) == -4
    assert lib.svit_randaug_stats(16, 16, 1, 16, 1, 1, 8, 8, 1, None) == -4          # layer outside [0, N)
    assert lib.svit_randaug_stats(16, 16, 0, 16, 1, 1, 2, 8, 1, None) == -2          # smaller than 3 x 3
    assert lib.svit_randaug_stats(16, 12, 0, 16, 1, 1, 8, 8, 1, None) == -3          # records not 8-byte aligned
    assert lib.svit_randaug_apply(16, 16, 16, 0, 16, 1, 1, 8, 8, 1, None) == -4      # src == dst


def test_augclips_runs_the_chain_ahead_of_every_read(ra):
    """render() and the im2col operand of AugClips(randaug=table) are those of an AugClips over apply_host's frames;
    clone / copy_ / set_randaug carry the table; without a table nothing is added"""
    from svit_amd import ops
    from svit_amd.augment import AugClips, AugRecord
    shape = (2, 4, 24, 32, 3)
    src = C.source(shape)
    S = 16
    recs = [AugRecord(1, 2, 3, 20, 24, S, S, 0, 0, 1, 0, 0, 0, 0, 0, 0), AugRecord.identity(0, 4, 9, S)]
    tables = [_mixed_table(ra, 24, 32), [l[::-1] for l in _mixed_table(ra, 24, 32)]]
    u8 = torch.from_numpy(src).cuda()
    clips = AugClips(u8, S, recs, randaug=tables[0])
    for k, table in enumerate(tables):
        if k:
            clips.set_randaug(table)
        want = AugClips(torch.from_numpy(ra.apply_host(src, table)).cuda(), S, recs)
        assert torch.equal(clips.render(), want.render())
        assert torch.equal(ops.im2col_patch_u8_aug(clips)[0], ops.im2col_patch_u8_aug(want)[0])
        assert torch.equal(clips.raw, u8) and torch.equal(clips.frames, want.frames)
    twin = clips.clone()
    assert twin.raw.data_ptr() != clips.raw.data_ptr() and torch.equal(twin.ra_table, clips.ra_table)
    assert torch.equal(twin.render(), want.render())
    other = AugClips(u8.flip(0).contiguous(), S, recs, randaug=tables[0])
    other.copy_(clips)
    assert torch.equal(other.render(), want.render())
    plain = AugClips(u8, S, recs)
    assert plain.raw is None and plain.frames.data_ptr() == u8.data_ptr()
    with pytest.raises(ValueError):
        plain.copy_(clips)
    with pytest.raises(ValueError):
        plain.set_randaug(tables[0])


def test_graph_replay_reads_the_table_at_replay_time(ra):
    """GraphedTrainStep over AugClips(randaug=...): two replays with different tables give the losses of eager steps
    over AugClips built from apply_host's frames, bit for bit (the forward pass is bit-reproducible)"""
    from svit_amd import losses
    from svit_amd.augment import AugClips, AugRecord
    from svit_amd.graph import GraphedTrainStep
    cfg, model, spec, sd = SM.build_hip_model(4, 64)
    video = P.frames(2, 4, 96)
    u8 = ((video * 0.225 + 0.45) * 255.0).round().clamp(0, 255).to(torch.uint8).permute(0, 2, 3, 4, 1).contiguous()
    src = u8.numpy()
    y = P.labels(2).cuda()
    S = 64
    recs = [AugRecord(0, 3, 5, 80, 70, S, S, 0, 0, 1, 0, 0, 0, 0, 0, 0), AugRecord.identity(1, 6, 26, S)]
    sampler = ra.RandAugSampler("rand-m7-n4-mstd0.5-inc1", "random")
    tables = []
    for seed in (3, 4, 5):
        random.seed(seed)
        np.random.seed(seed)
        tables.append([sampler.draw(4, 96, 96, video=v) for v in range(2)])
    assert all(any(o.op != ra.OP_NONE for layers in t for o in layers) for t in tables)

    def loss_fun(preds, extra, labels):
        return losses.cross_entropy(preds, labels)

    def eager(table):
        clips = AugClips(torch.from_numpy(ra.apply_host(src, table)).cuda(), S, recs)
        model.flat.grad.zero_()
        logits, _ = model([clips], {})
        loss = losses.cross_entropy(logits, y)
        loss.backward()
        torch.cuda.synchronize()
        return loss.detach().clone()

    step = GraphedTrainStep(model, loss_fun, [AugClips(u8.cuda(), S, recs, randaug=tables[0])], y)
    seen = []
    for table in tables[1:]:
        want = eager(table)
        loss, _ = step([AugClips(u8.cuda(), S, recs, randaug=table)], y)
        torch.cuda.synchronize()
        assert torch.equal(loss, want), table
        seen.append(float(loss))
    assert seen[0] != seen[1]
