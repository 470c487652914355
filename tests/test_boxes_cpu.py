"""The box side of the image ranks' augmentation on the host (svit_amd/randaug.py `draw(..., boxes=)` / `boxes_layer`,
svit_amd/augment.py `draw(..., boxes=)` / `boxes_through` / `haog_targets` / `draw_still`) against tests/golden/boxes.npz,
written by tools/gen_boxes_golden.py from the unmodified reference.  The Rotate arrays of the fixture were recorded through
a computing cv2 stand-in and the Shear boxes are not the reference's at all (the fixture holds none unless it was written
with --record-shear): see the tool's docstring.  No GPU."""
import os
import random

import numpy as np
import pytest
import torch

from svit_amd import augment, randaug
from svit_amd.augment import build_sampler
from tests.test_augment_cpu import set_cfg

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
ROTATE_BAR = 1e-3       # px: coordinates stay below 512, where a float32 ulp is 6e-5, a dozen operations deep
#                         measured maximum: 0 px, single operations and chains alike
SHEAR_CAP = 0.40        # share of the chains of one policy string whose boxes the fixture cannot hold


@pytest.fixture(scope="module")
def gold():
    return dict(np.load(os.path.join(GOLDEN, "boxes.npz")))


@pytest.fixture(scope="module")
def aug_gold():
    return dict(np.load(os.path.join(GOLDEN, "augment.npz")))


def bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float32)).view(np.int32)


def seed(k):
    random.seed(k)
    np.random.seed(k)


def level_args(arg):
    return () if np.isnan(arg) else (float(arg),)


# ------------------------------------------------------------------------------------------ 1. the spatial pipeline ----
@pytest.mark.parametrize("s", range(5))
def test_spatial_boxes_and_targets_are_the_reference_bits(gold, aug_gold, s):
    sampler = build_sampler(set_cfg(aug_gold, s))
    S = int(aug_gold["crop"])
    noise = str(aug_gold["set_re_mode"][s]) in ("rand", "pixel")
    kept = 0
    for k in range(gold["spatial_in"].shape[1]):
        Hs, Ws = (int(v) for v in aug_gold["sizes"][k % len(aug_gold["sizes"])])
        seed(k)
        rec, moved = sampler.draw(Hs, Ws, video=3, boxes=gold["spatial_in"][s, k])
        assert isinstance(rec, augment.AugRecord) and moved.dtype == np.float32 and moved.shape == (1, 4, 4)
        assert np.array_equal(bits(moved), bits(gold["spatial_out"][s, k])), (s, k, moved, gold["spatial_out"][s, k])
        target = augment.haog_targets(moved, S)
        assert target.dtype == torch.float32 and tuple(target.shape) == (1, 4, 4)
        assert np.array_equal(bits(target.numpy()), bits(gold["spatial_targets"][s, k])), (s, k)
        # the four rows are what the fixture was built for: inside, crossing, a sliver (zeroed), absent (zero)
        nz = (target.numpy() != 0).any(-1)[0]
        assert nz.tolist() == [True, True, False, False], (s, k, target)
        kept += int(nz.sum())
        # both streams stand where the reference left them after the erasing (plus the documented noise-seed draw)
        ref_r, ref_np, ref_seed, ref_r_after_seed = gold["spatial_tail"][s, k]
        assert np.random.uniform() == ref_np, (s, k)
        if rec.erase_mode and noise:
            assert rec.seed == int(ref_seed) and random.random() == ref_r_after_seed, (s, k)
        else:
            assert random.random() == ref_r, (s, k)
    assert kept == 2 * gold["spatial_in"].shape[1]


def test_test_time_boxes_and_targets_are_the_reference_bits(gold, aug_gold):
    """val / test: `utils.spatial_sampling(spatial_idx=0 / 1 / 2, boxes=)` as recorded -- the short-side rescale (one
    factor for both axes, none where the short side is the crop already) and `uniform_crop`"""
    S = int(aug_gold["crop"])
    sampler = augment.SpatialSampler(S, spatial_sampling="uniform", random_flip=False)
    sizes = gold["uniform_sizes"].tolist()
    assert [240, 320] in sizes and [320, 240] in sizes and [224, 300] in sizes and [300, 224] in sizes
    for z, (Hs, Ws) in enumerate(sizes):
        for idx in range(3):
            seed(z)
            rec, moved = sampler.draw(Hs, Ws, spatial_idx=idx, boxes=gold["uniform_in"][z, idx])
            assert np.array_equal(bits(moved), bits(gold["uniform_out"][z, idx])), (Hs, Ws, idx, moved)
            target = augment.haog_targets(moved, S).numpy()
            assert np.array_equal(bits(target), bits(gold["uniform_targets"][z, idx])), (Hs, Ws, idx)
            assert [random.random(), np.random.uniform()] == gold["uniform_tail"][z, idx].tolist()
    assert len({gold["uniform_out"][0, i].tobytes() for i in range(3)}) == 3        # the three crops differ


def test_uniform_crop_boxes_follow_the_scale_and_the_window():
    """val / test: the short-side rescale (one factor for both axes) and `crop_clip_boxes` with the crop's offsets,
    restated here in float32 step by step"""
    sampler = augment.SpatialSampler(64, spatial_sampling="uniform", random_flip=False)
    b = np.array([[[10.25, 5.5, 90.0, 70.75], [-4.0, 60.0, 300.0, 250.0], [0, 0, 0, 0]]], dtype=np.float32)
    for (Hs, Ws), idx in (((128, 192), 0), ((128, 192), 2), ((200, 100), 1), ((64, 96), 1)):
        seed(0)
        rec, moved = sampler.draw(Hs, Ws, spatial_idx=idx, boxes=b)
        want = b.reshape(-1, 4).copy()
        if (rec.out_h, rec.out_w) != (Hs, Ws):
            f, n = (np.float32(rec.out_h), Hs) if Ws < Hs else (np.float32(rec.out_w), Ws)
            want = (want * f) / np.float32(n)
        want[:, 0::2] = np.clip(want[:, 0::2] - np.float32(rec.ox), 0, 64)
        want[:, 1::2] = np.clip(want[:, 1::2] - np.float32(rec.oy), 0, 64)
        assert np.array_equal(bits(moved), bits(want.reshape(1, 3, 4))), (Hs, Ws, idx)
        assert moved.min() >= 0 and moved.max() <= 64 and not moved[0, 2].any()


def test_haog_targets_zero_what_is_empty():
    t = augment.haog_targets(np.array([[[0, 0, 64, 64], [10, 10, 13.2, 40], [10, 10, 40, 13.3], [70, -3, 90, 20]]],
                                      dtype=np.float32), 64).numpy()
    assert t[0, 0].tolist() == [0.5, 0.5, 1.0, 1.0]
    assert not t[0, 1].any() and t[0, 2].any() and not t[0, 3].any()      # 3.2 / 64 = 0.05 is empty, 3.3 / 64 is not
    with pytest.raises(ValueError):
        augment.haog_targets(np.array([[[30, 0, 10, 5]]], dtype=np.float32), 64)


# ------------------------------------------------------------------------------------- 2. RandAugment, one operation ----
def test_single_operations_move_the_boxes_as_the_reference(gold):
    names = [str(n) for n in gold["names"]]
    worst, seen = 0.0, set()
    for r in range(len(gold["op_name"])):
        name = names[int(gold["op_name"][r])]
        Hs, Ws = (int(v) for v in gold["stills"][int(gold["op_size"][r])])
        args = level_args(gold["op_arg"][r])
        src = gold["op_in"][r]
        before = src.copy()
        got = randaug.boxes_layer(name, args, src, Hs, Ws)
        assert np.array_equal(src, before)                                   # the input is never written
        assert got.dtype == np.float32 and got.shape == src.shape
        if name in ("ShearX", "ShearY"):
            assert bool(gold["op_shear"][r])                                 # recorded as draws only (geometric here)
            continue
        assert not bool(gold["op_shear"][r])
        seen.add(name)
        want = gold["op_out"][r]
        assert not np.isnan(want).any()
        if name == "Rotate":
            worst = max(worst, float(np.abs(got - want).max()))
            assert np.array_equal(got == 0, want == 0), (name, args)          # the same rows were dropped
        else:
            assert np.array_equal(bits(got), bits(want)), (name, args, (Hs, Ws))
            if name not in ("TranslateXRel", "TranslateYRel"):
                assert got is src or np.array_equal(bits(got), bits(src))
    print("Rotate boxes against the recording: max |diff| %.3g px (bar %.0e)" % (worst, ROTATE_BAR))
    # measured: 0 (the restatement and the stand-in the recording went through evaluate the same closed form)
    assert worst <= ROTATE_BAR
    assert {"Rotate", "TranslateXRel", "TranslateYRel", "AutoContrast", "SolarizeIncreasing", "Posterize"} <= seen
    rot = [r for r in range(len(gold["op_name"])) if names[int(gold["op_name"][r])] == "Rotate"]
    assert any((gold["op_out"][r][:, :3] == 0).all(-1).any() for r in rot), "no rotation dropped a box"
    assert all((gold["op_out"][r][:, 3] == 0).all() for r in rot)


# ------------------------------------------------------------------------------------------ 3. RandAugment, chains ----
@pytest.mark.parametrize("s", range(5))
def test_chains_draw_and_move_boxes_as_the_reference(gold, s):
    """sets 0-3: the share of chains whose boxes the fixture cannot hold is capped; set 4, the three-layer weighted
    policy (about half of its chains apply a shear whatever the seeds), is held to its draws and stream positions for
    every chain and to its boxes wherever no shear ran, without a cap"""
    names = [str(n) for n in gold["names"]]
    aa, interp = str(gold["set_aa"][s]), str(gold["set_interp"][s])
    sampler = randaug.RandAugSampler(aa, interp)
    shear = gold["chain_applied_shear"][s]
    share = float(shear.mean())
    capped = bool(gold["chain_capped"][s])
    assert gold["chain_capped"].tolist() == [True, True, True, True, False]
    print("%s: %.1f %% of the chains applied a shear to the boxes (cap %s)"
          % (aa, 100 * share, "%.0f %%" % (100 * SHEAR_CAP) if capped else "none"))
    assert share <= SHEAR_CAP or not capped
    worst, compared = 0.0, 0
    for k in range(shear.shape[0]):
        for z, (Hs, Ws) in enumerate(gold["stills"].tolist()):
            seed(k)
            ops, moved = sampler.draw(1, Hs, Ws, boxes=gold["chain_in"][z])
            assert len(ops) == sampler.num_layers == int((gold["chain_op"][s, k, z] > -2).sum())
            for n, (name, args, _) in enumerate(sampler.trace):
                op, arg = int(gold["chain_op"][s, k, z, n]), gold["chain_arg"][s, k, z, n]
                assert (names[op] if op >= 0 else "") == name, (s, k, z, n)
                assert args == (level_args(arg) if op >= 0 else ()), (s, k, z, n)
            assert [random.random(), np.random.uniform()] == gold["chain_tail"][s, k, z].tolist(), (s, k, z)
            sheared = any(name in ("ShearX", "ShearY") and args[0] != 0 for name, args, _ in sampler.trace)
            assert sheared == bool(shear[k, z]), (s, k, z)
            want = gold["chain_boxes"][s, k, z]
            if sheared:
                assert bool(gold["shear_recorded"]) or np.isnan(want).all()
                continue
            compared += 1
            if any(name == "Rotate" for name, _, _ in sampler.trace):
                worst = max(worst, float(np.abs(moved - want).max()))
                assert np.array_equal(moved == 0, want == 0), (s, k, z)
            else:
                assert np.array_equal(bits(moved), bits(want)), (s, k, z)
            assert not moved[0, 3].any()
    print("%s: boxes of %d chains compared, with a Rotate max |diff| %.3g px" % (aa, compared, worst))
    assert worst <= ROTATE_BAR and compared == int((~shear).sum()) and compared > 0
    assert compared >= (1 - SHEAR_CAP) * shear.size or not capped


# ---------------------------------------------------------------------------------------------- 4. the Shear boxes ----
def shear_closed_form(b, f, Hs, Ws, axis):
    """float64: the four corners through x' = x - f y (axis 1: y' = y - f x), their enclosing box, clipped"""
    out = []
    for x0, y0, x1, y1 in np.asarray(b, dtype=np.float64).reshape(-1, 4):
        pts = [(x, y) for x in (x0, x1) for y in (y0, y1)]
        pts = [(x - f * y, y) if axis == 0 else (x, y - f * x) for x, y in pts]
        xs, ys = [p[0] for p in pts], [p[1] for p in pts]
        out.append([min(max(min(xs), 0), Ws), min(max(min(ys), 0), Hs), min(max(max(xs), 0), Ws), min(max(max(ys), 0), Hs)])
    return np.array(out, dtype=np.float64).astype(np.float32)


def test_shear_boxes_are_the_geometric_closed_form(gold):
    for z, (Hs, Ws) in enumerate(gold["stills"].tolist()):
        src = np.concatenate([gold["chain_in"][z], gold["chain_in"][z] + np.float32(1.625)], axis=0)
        src[:, 3] = 0
        for name, axis in (("ShearX", 0), ("ShearY", 1)):
            same = randaug.boxes_layer(name, (0.0,), src, Hs, Ws)
            assert np.array_equal(bits(same), bits(src))                              # factor 0 is the identity
            for f in (0.09, -0.09, 0.21, -0.21, 0.3, -0.3):
                got = randaug.boxes_layer(name, (f,), src, Hs, Ws)
                want = shear_closed_form(src, f, Hs, Ws, axis).reshape(src.shape)
                want[:, 3] = 0
                assert np.array_equal(bits(got), bits(want)), (name, f, (Hs, Ws))
                assert not got[:, 3].any()                                             # zero rows stay zero
                assert got[..., 0::2].min() >= 0 and got[..., 0::2].max() <= Ws
                assert got[..., 1::2].min() >= 0 and got[..., 1::2].max() <= Hs
                assert (got[..., 2] >= got[..., 0]).all() and (got[..., 3] >= got[..., 1]).all()
                assert not np.array_equal(got, src)


def test_shear_boxes_against_the_reference_where_it_was_recorded(gold):
    """Only a fixture written with --record-shear (imgaug and cv2 installed) holds the reference's Shear boxes.  They are
    NOT expected to equal the geometric ones.  Both enclose the same sheared region, but they anchor it differently: PIL's
    matrix keeps row 0 (column 0) in place, the reference shears by tan(f) on imgaug's fitted canvas and then keeps the
    left or the right `w` columns (top or bottom `h` rows) of it.  So along the sheared axis they may lie apart by up to
    the whole displacement of the shear, tan|f| x the OTHER side, plus 1 px for the canvas' integer size; along the other
    axis only by the canvas rounding and by what the clip to the image, which only the geometric box gets on that axis,
takes off a box that leaves the image (the fixture's boxes leave it by less than 1 px).  That is the bar below; it was worked out, not measured -- the recording cannot
    run where imgaug is absent -- and every case prints its deviation, so that the first recording shows how much of
    the bar is used.  Zero rows are zero in both."""
    if "shear_op_out" not in gold:
        pytest.skip("tests/golden/boxes.npz was recorded without imgaug: it holds no Shear boxes of the reference")
    names = [str(n) for n in gold["names"]]
    rows = [r for r in range(len(gold["op_name"])) if bool(gold["op_shear"][r])]
    assert len(rows) == len(gold["shear_op_out"]) > 0
    assert len(gold["shear_chain_boxes"]) == int(gold["chain_applied_shear"].sum())
    for r, want in zip(rows, gold["shear_op_out"]):
        name = names[int(gold["op_name"][r])]
        Hs, Ws = (int(v) for v in gold["stills"][int(gold["op_size"][r])])
        f = float(gold["op_arg"][r])
        got = randaug.boxes_layer(name, (f,), gold["op_in"][r], Hs, Ws)
        along, across = ((0, 2), (1, 3)) if name == "ShearX" else ((1, 3), (0, 2))
        dev_along = float(np.abs(got - want)[..., along].max())
        dev_across = float(np.abs(got - want)[..., across].max())
        bar = np.tan(abs(f)) * (Hs if name == "ShearX" else Ws) + 1
        print("%s f=%+.3f %dx%d: |geometric - reference| %.3f px along the shear (bar %.1f), %.3f px across (bar 1)"
              % (name, f, Hs, Ws, dev_along, bar, dev_across))
        assert dev_along <= bar and dev_across <= 1
        assert not want[:, 3].any() and not got[:, 3].any()


# --------------------------------------------------------------------------------- 5. boxes=None: nothing changed ----
@pytest.mark.parametrize("s", range(4))
def test_randaug_draw_without_boxes_is_untouched(gold, s):
    sampler = randaug.RandAugSampler(str(gold["set_aa"][s]), str(gold["set_interp"][s]))
    for k in range(8):
        seed(k)
        plain = sampler.draw(3, 24, 32, video=1)
        tail = (random.random(), np.random.uniform())
        assert isinstance(plain, list) and all(isinstance(o, randaug.RandAugOp) for o in plain)
        seed(k)
        ops, moved = sampler.draw(3, 24, 32, video=1, boxes=np.zeros((3, 2, 4), dtype=np.float32))
        assert ops == plain and tail == (random.random(), np.random.uniform())
        assert not moved.any()
        # and the draws are the ones the plain transform's fixture pins for a T = 1 still (same seeds, same sizes)
        seed(k)
        assert sampler.draw(1, 24, 32) == sampler_draw_reference(sampler, 1, 24, 32, k)


def sampler_draw_reference(sampler, T, Hs, Ws, k):
    """the body of RandAugSampler.draw as it was before boxes existed, restated from its docstring"""
    seed(k)
    picks = np.random.choice(len(sampler.transforms), sampler.num_layers, replace=sampler.weights is None, p=sampler.weights)
    ops = []
    for p in picks:
        name = sampler.transforms[int(p)]
        if random.random() > 0.5:
            ops.append(randaug.RandAugOp(randaug.OP_NONE))
            continue
        m = random.gauss(sampler.magnitude, sampler.magnitude_std) if sampler.magnitude_std > 0 else sampler.magnitude
        args = randaug._level_args(name, min(randaug.MAX_LEVEL, max(0, m)))
        filters = ()
        if name in randaug.GEOMETRIC:
            filters = tuple(random.choice((0, 1)) for _ in range(T)) if sampler.filter is None else (sampler.filter,) * T
        ops.append(randaug.make_op(name, args, filters, Hs, Ws))
    return ops


@pytest.mark.parametrize("s", range(5))
def test_spatial_draw_without_boxes_is_untouched(aug_gold, s):
    sampler = build_sampler(set_cfg(aug_gold, s))
    for k in range(8):
        Hs, Ws = (int(v) for v in aug_gold["sizes"][k % len(aug_gold["sizes"])])
        seed(k)
        plain = sampler.draw(Hs, Ws, video=2)
        tail = (random.random(), np.random.uniform())
        assert type(plain) is augment.AugRecord
        seed(k)
        rec, _ = sampler.draw(Hs, Ws, video=2, boxes=np.zeros((1, 4, 4), dtype=np.float32))
        assert rec == plain and tail == (random.random(), np.random.uniform())
    test = augment.SpatialSampler(224, spatial_sampling="uniform", random_flip=False)
    assert type(test.draw(240, 320, spatial_idx=2)) is augment.AugRecord


def test_motion_shift_stays_refused(aug_gold):
    cfg = set_cfg(aug_gold, 0)
    cfg.DATA.TRAIN_JITTER_MOTION_SHIFT = True
    with pytest.raises(NotImplementedError):
        build_sampler(cfg)


# ------------------------------------------------------------------------------------------------ 6. one whole still ----
def test_draw_still_is_the_three_stages_in_the_reference_order(aug_gold):
    cfg = set_cfg(aug_gold, 0)
    cfg.AUG.AA_TYPE, cfg.AUG.INTERPOLATION = "rand-m7-n4-mstd0.5-inc1", "bicubic"
    ra, sampler = randaug.build_randaug(cfg), build_sampler(cfg)
    b = np.array([[[60.5, 40, 200, 180], [100, 90, 150.25, 170], [0, 0, 0, 0], [250, 10, 318, 200]]], dtype=np.float32)
    for k in range(6):
        seed(k)
        ops, rec, target = augment.draw_still(ra, sampler, 240, 320, b, video=5)
        tail = (random.random(), np.random.uniform())
        seed(k)
        ops2, moved = ra.draw(1, 240, 320, video=5, boxes=b)
        rec2, moved = sampler.draw(240, 320, video=5, boxes=moved)
        assert ops == ops2 and rec == rec2 and rec.video == 5 and tail == (random.random(), np.random.uniform())
        assert torch.equal(target, augment.haog_targets(moved, sampler.size))
        assert tuple(target.shape) == (1, 4, 4) and not target[0, 2].any()
        assert float(target.min()) >= 0 and float(target.max()) <= 1
    seed(0)
    ops, rec, target = augment.draw_still(None, sampler, 240, 320, b)
    assert ops is None and type(rec) is augment.AugRecord
