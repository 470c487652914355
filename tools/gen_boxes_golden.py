"""Generate tests/golden/boxes.npz: the box side of the image ranks' augmentation, recorded from the UNMODIFIED reference
`slowfast/datasets/{utils,transform}.py`, `slowfast/utils/box_ops.py` and `slowfast/datasets/ssv2_MF/{autoaugment,
boxes_autoaugment}.py`, `ssv2_MF/boxes_aug/bbox_util.py` (development machine only: needs a reference checkout and PIL;
the tests read the fixture, never the reference).

    python tools/gen_boxes_golden.py [--reference /path/to/reference] [--record-shear]

The reference modules are loaded from their files and RUN (as tools/gen_augment_golden.py does); only arrays they
produced are written.  Two packages the box code imports are absent from the development image and get stand-ins:

  cv2     `rotate_boxes` uses it for `getRotationMatrix2D` and for the SHAPE of a warped zero image.  The stand-in
          computes: OpenCV's documented closed form of the matrix (alpha = cos a, beta = sin a; [[alpha, beta,
          (1 - alpha) cx - beta cy], [-beta, alpha, beta cx + (1 - alpha) cy]]) and a `warpAffine` that returns zeros of
          the requested size.  THE ROTATE ARRAYS WERE RECORDED THROUGH THIS STAND-IN (`rotate_through_standin`).
  imgaug  `shear_x_iaa` / `shear_y_iaa` go through its fitted canvas.  The stand-in is INERT: it hands the boxes back
          and notes that a shear ran (`applied_shear`), so that the rest of a chain still draws what it draws.  Boxes that
          went through it are NOT recorded -- only the draws and the stream position of such a case.

--record-shear (where imgaug and cv2 exist): nothing is stood in for and the reference's own Shear boxes are added
(`shear_op_out`, `shear_chain_boxes`, `shear_recorded`); tests/test_boxes_cpu.py compares them when they are present.

Spatial cases.  The five parameter sets, 32 seeds and four sizes of gen_augment_golden.py.  Per seed four boxes [1,4,4] in
source pixels, placed against the window that seed draws (read from svit_amd's sampler, whose records
tests/test_augment_cpu.py pins to the reference): one inside it, one crossing its left border, one with a sliver inside
(empty after the crop, zeroed in the targets) and an all-zero row.  Recorded: the boxes after `utils.spatial_sampling(...,
boxes=)`, the targets after the stage of ssv2_frames.py:347-353 (`box_ops.box_xyxy_to_cxcywh`, `zero_empty_boxes`) and
the position of both streams after the erasing that follows (gen_augment_golden.stream_tail).

RandAugment cases.  Every operation of both sets through `AugmentOp.__call__` (prob 1) at magnitudes 3 and 7 and, where
the level function negates, both signs, on T = 2 frames of 24 x 32 and 240 x 320: level argument, boxes before and after.
Whole chains: the four policy strings of CHAIN_SETS x 32 seeds on a 24 x 32 and a 240 x 320 still through
`create_random_augment(..., with_boxes=True)`: per layer the operation and its argument, the final boxes, the stream
position and `applied_shear` (a ShearX / ShearY layer ran with a level argument other than 0: read off the recorded
layer, with and without stand-ins).  CHAIN_SETS are the sets of tests/randaug_cases.py with ONE layer in the weighted one: a
uniform pick applies a shear in 1 - (1 - (2/15) 0.5)^n of the chains (24 % at n = 4), which leaves enough chains with
recorded boxes; the `w0` weights give the two shears 40 % of the mass, so three picks without replacement apply one in
about half of the chains whatever the seeds -- with one pick it is 0.4 x 0.5 = 20 % and the weighted, non-replacing
`np.random.choice` is still what is drawn.  The three-layer weighted policy of randaug_cases.py is recorded as a fifth
set WITHOUT a cap: draws and stream positions for every chain, boxes where no shear ran.

Test-time cases.  `utils.spatial_sampling(spatial_idx=0 / 1 / 2, min_scale = max_scale = crop_size, boxes=)` -- the
short-side rescale and `uniform_crop` -- on UNIFORM_SIZES (wide, very wide, tall, short side == crop both ways) with the
first seed's boxes of each size: boxes, targets, stream position.
"""
import argparse
import importlib
import math
import os
import random
import sys
import types

sys.dont_write_bytecode = True

import numpy as np
import torch
from PIL import Image

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
OUT = os.path.join(ROOT, "tests", "golden", "boxes.npz")

from tests import randaug_cases as C          # noqa: E402
from tools import gen_augment_golden as G     # noqa: E402

N_SEEDS = 32
STILLS = [(24, 32), (240, 320)]
LEVELS = (3, 7)
STATE = {"shear": False, "idle": False}      # "shear": the inert stand-in was asked for a shear; idle None: no stand-in
CHAIN_SETS = C.SETS[:3] + [("rand-m5-n1-w0", "bicubic"), C.SETS[3]]
CHAIN_CAPPED = [True, True, True, True, False]      # the share of chains left out is capped for these
SHEARS = ("ShearX", "ShearY")
UNIFORM_SIZES = G.SIZES + [(300, 224)]
ENH = ("ColorIncreasing", "ContrastIncreasing", "BrightnessIncreasing", "SharpnessIncreasing")
NEGATING = ("Rotate", "ShearX", "ShearY", "TranslateXRel", "TranslateYRel") + ENH


# ---- stand-ins ------------------------------------------------------------------------------------------------------
def cv2_standin():
    m = types.ModuleType("cv2")

    def getRotationMatrix2D(center, angle, scale):
        a = math.radians(angle)
        alpha, beta = scale * math.cos(a), scale * math.sin(a)
        cx, cy = float(center[0]), float(center[1])
        return np.array([[alpha, beta, (1 - alpha) * cx - beta * cy], [-beta, alpha, beta * cx + (1 - alpha) * cy]],
                        dtype=np.float64)

    def warpAffine(img, M, dsize, *a, **kw):
        return np.zeros((int(dsize[1]), int(dsize[0])) + tuple(img.shape[2:]), dtype=img.dtype)

    m.getRotationMatrix2D, m.warpAffine = getRotationMatrix2D, warpAffine
    return m


def imgaug_standin():
    """inert: boxes come back as they went in; STATE["shear"] notes that the reference asked for a shear"""
    class BoundingBox:
        def __init__(self, x1, y1, x2, y2):
            self.c = (x1, y1, x2, y2)

    class BoundingBoxesOnImage:
        def __init__(self, boxes, shape):
            self.boxes, self.height, self.width = boxes, shape[0], shape[1]

        def to_xyxy_array(self):
            return np.array([b.c for b in self.boxes], dtype=np.float32).reshape(-1, 4)

    class Shear:
        def __init__(self, *a, **kw):
            pass

        def to_deterministic(self):
            return self

        def augment_bounding_boxes(self, lst):
            STATE["shear"] = True
            return lst

    mods = {n: types.ModuleType(n) for n in ("imgaug", "imgaug.augmenters", "imgaug.augmentables", "imgaug.augmentables.bbs")}
    mods["imgaug.augmenters"].geometric = types.SimpleNamespace(ShearX=Shear, ShearY=Shear)
    mods["imgaug.augmenters"].size = types.SimpleNamespace(Resize=Shear)
    mods["imgaug.augmentables.bbs"].BoundingBox = BoundingBox
    mods["imgaug.augmentables.bbs"].BoundingBoxesOnImage = BoundingBoxesOnImage
    mods["imgaug"].augmenters, mods["imgaug"].augmentables = mods["imgaug.augmenters"], mods["imgaug.augmentables"]
    mods["imgaug.augmentables"].bbs = mods["imgaug.augmentables.bbs"]
    return mods


def load(root, record_shear):
    if record_shear:
        import cv2        # noqa: F401  (the real ones, or this mode cannot run)
        import imgaug     # noqa: F401
        STATE["idle"] = None
    else:
        for name in ("cv2", "imgaug"):
            try:
                importlib.import_module(name)
                raise SystemExit("%s is installed: run with --record-shear, nothing needs a stand-in" % name)
            except ImportError:
                pass
        sys.modules["cv2"] = cv2_standin()
        sys.modules.update(imgaug_standin())
    utils, transform, erasing = G.load_reference(root)
    mf = importlib.import_module("slowfast.datasets.ssv2_MF.autoaugment")
    box_ops = importlib.import_module("slowfast.utils.box_ops")
    for m in (mf, box_ops):
        assert os.path.realpath(m.__file__).startswith(os.path.realpath(root))
    assert transform.rand_augment_transform_with_boxes is mf.rand_augment_transform
    return utils, transform, erasing, mf, box_ops


# ---- spatial cases --------------------------------------------------------------------------------------------------
def sampler_of(p):
    from svit_amd.augment import SpatialSampler
    kw = dict(scale=G.REL_SCALE, aspect=G.REL_ASPECT) if p["aug"] else {}
    return SpatialSampler(G.CROP, jitter_scales=p["scales"], random_flip=p["flip"], inverse_uniform_sampling=p["inv"],
                          re_prob=p["re_prob"], re_mode=p["re_mode"], **kw)


def boxes_for(rec, k):
    """[1,4,4] xyxy in source pixels against the window of record `rec` (module docstring); fractional coordinates"""
    fy, fx = rec.out_h / rec.h, rec.out_w / rec.w
    x0, y0 = rec.j + rec.ox / fx, rec.i + rec.oy / fy
    w, h = G.CROP / fx, G.CROP / fy
    e = (k % 7) / 7.0
    rows = [(x0 + 0.30 * w + e, y0 + 0.25 * h, x0 + 0.70 * w, y0 + 0.80 * h + e),
            (x0 - 0.30 * w, y0 + 0.20 * h + e, x0 + 0.30 * w + e, y0 + 0.60 * h),
            (x0 - 0.50 * w - e, y0 + 0.10 * h, x0 + 0.02 * w, y0 + 0.90 * h),
            (0.0, 0.0, 0.0, 0.0)]
    return np.array(rows, dtype=np.float32).reshape(1, 4, 4)


def targets(box_ops, boxes, S):
    """the stage of ssv2_frames.py:347-353 on the reference's own functions"""
    b = boxes.copy()
    b[..., 0::2] = b[..., 0::2] / S
    b[..., 1::2] = b[..., 1::2] / S
    t = torch.from_numpy(np.clip(b, 0, 1))
    return box_ops.zero_empty_boxes(box_ops.box_xyxy_to_cxcywh(t), mode="cxcywh").numpy()


def spatial_cases(utils, erasing, box_ops):
    nS = len(G.SETS)
    b_in = np.zeros((nS, N_SEEDS, 1, 4, 4), dtype=np.float32)
    b_out, b_tar = np.zeros_like(b_in), np.zeros_like(b_in)
    tail = np.zeros((nS, N_SEEDS, 4), dtype=np.float64)
    for s, p in enumerate(G.SETS):
        for k in range(N_SEEDS):
            H, W = G.SIZES[k % len(G.SIZES)]
            random.seed(k)
            np.random.seed(k)
            rec = sampler_of(p).draw(H, W)
            boxes = boxes_for(rec, k)
            random.seed(k)
            np.random.seed(k)
            kw = dict(spatial_idx=-1, min_scale=p["scales"][0], max_scale=p["scales"][1], crop_size=G.CROP,
                      random_horizontal_flip=p["flip"], inverse_uniform_sampling=p["inv"])
            if p["aug"]:
                kw.update(aspect_ratio=G.REL_ASPECT, scale=G.REL_SCALE, motion_shift=False)
            out, moved = utils.spatial_sampling(torch.zeros(3, 1, H, W), boxes=boxes.reshape(-1, 4).copy(), **kw)
            if p["re_prob"] > 0:
                er = erasing.RandomErasing(p["re_prob"], mode=p["re_mode"], max_count=1, num_splits=1, device="cpu")
                state = torch.get_rng_state()
                er(out.permute(1, 0, 2, 3).clone())
                torch.set_rng_state(state)
            tail[s, k] = G.stream_tail()
            b_in[s, k], b_out[s, k] = boxes, moved.reshape(1, 4, 4)
            b_tar[s, k] = targets(box_ops, b_out[s, k], G.CROP)
    kept = (b_tar != 0).any(-1)[:, :, 0]
    assert kept[:, :, 0].all() and kept[:, :, 1].all() and not kept[:, :, 2].any() and not kept[:, :, 3].any(), kept.sum(1)
    nZ = len(UNIFORM_SIZES)
    u_in = np.zeros((nZ, 3, 1, 4, 4), dtype=np.float32)
    u_out, u_tar = np.zeros_like(u_in), np.zeros_like(u_in)
    u_tail = np.zeros((nZ, 3, 2), dtype=np.float64)
    from svit_amd.augment import SpatialSampler
    for z, (H, W) in enumerate(UNIFORM_SIZES):
        for idx in range(3):
            random.seed(z)
            np.random.seed(z)
            rec = SpatialSampler(G.CROP, spatial_sampling="uniform", random_flip=False).draw(H, W, spatial_idx=idx)
            boxes = boxes_for(rec, z + idx)
            random.seed(z)
            np.random.seed(z)
            _, moved = utils.spatial_sampling(torch.zeros(3, 1, H, W), boxes=boxes.reshape(-1, 4).copy(), spatial_idx=idx,
                                              min_scale=G.CROP, max_scale=G.CROP, crop_size=G.CROP)
            u_tail[z, idx] = [random.random(), np.random.uniform()]
            u_in[z, idx], u_out[z, idx] = boxes, np.asarray(moved, dtype=np.float32).reshape(1, 4, 4)
            u_tar[z, idx] = targets(box_ops, u_out[z, idx], G.CROP)
    assert (u_tar[:, :, 0, 0] != 0).any(-1).all() and not u_tar[:, :, 0, 3].any()
    return dict(spatial_in=b_in, spatial_out=b_out, spatial_targets=b_tar, spatial_tail=tail,
                uniform_sizes=np.array(UNIFORM_SIZES, dtype=np.int32), uniform_in=u_in, uniform_out=u_out,
                uniform_targets=u_tar, uniform_tail=u_tail)


# ---- RandAugment cases ----------------------------------------------------------------------------------------------
def still_boxes(H, W, T):
    """[T,4,4]: a central box, a box in the far corner (a rotation pushes most of it out), a thin box on the left edge
    and an all-zero row; frame t shifted by t pixels"""
    rows = np.array([(0.30 * W + 0.25, 0.35 * H, 0.70 * W, 0.75 * H + 0.5),
                     (0.90 * W, 0.88 * H + 0.125, 0.995 * W, 0.99 * H),
                     (0.0, 0.10 * H, 0.06 * W + 0.375, 0.90 * H),
                     (0.0, 0.0, 0.0, 0.0)], dtype=np.float32)
    out = np.stack([rows + np.float32(t) for t in range(T)])
    out[:, 3] = 0
    return out


class Layers:
    """wraps, inside the loaded module, every entry of NAME_TO_OP (operation name and level arguments) and
    AugmentOp.__call__ (one call per layer; a layer the reference skipped makes no call of its function)"""

    def __init__(self, mf, names):
        self.layers, self.calls, self.names = [], [], names
        rec = self
        for name, fn in list(mf.NAME_TO_OP.items()):
            def wrapped(img, *args, _fn=fn, _name=name, **kw):
                rec.calls.append((_name, tuple(args)))
                return _fn(img, *args, **kw)
            mf.NAME_TO_OP[name] = wrapped
        orig_call = mf.AugmentOp.__call__

        def call(op, img_list, boxes=None, clean_img=None):
            rec.calls = []
            out = orig_call(op, img_list, boxes=boxes, clean_img=clean_img)
            if rec.calls:
                name, args = rec.calls[0]
                rec.layers.append((names.index(name), float(args[0]) if args else float("nan")))
            else:
                rec.layers.append((-1, float("nan")))
            return out
        mf.AugmentOp.__call__ = call


def op_cases(mf, rec, names):
    ALL = sorted(mf.NAME_TO_OP)
    rows = []
    hp = {"translate_const": 10, "interpolation": Image.BILINEAR}
    for name in names:
        for size_index, (H, W) in enumerate(STILLS):
            imgs = [Image.new("RGB", (W, H))] * 2
            boxes = still_boxes(H, W, 2)
            for lvl in LEVELS:
                signs = set()
                for seed in range(64):
                    random.seed(seed)
                    np.random.seed(seed)
                    rec.layers, STATE["shear"] = [], STATE["idle"]
                    _, out, _ = mf.AugmentOp(name, prob=1.0, magnitude=lvl, hparams=hp)(imgs, boxes=boxes.copy())
                    (idx, arg), = rec.layers
                    assert ALL[idx] == name
                    sign = 0 if name not in NEGATING else -1 if arg < (1 if name in ENH else 0) else 1
                    if sign in signs:
                        continue
                    signs.add(sign)
                    sheared = name in SHEARS and arg != 0
                    assert STATE["shear"] in (sheared, None), (name, arg)     # (None: the real imgaug ran, nothing to note)
                    rows.append((idx, size_index, arg, boxes, np.asarray(out, dtype=np.float32), sheared))
                    if len(signs) == (2 if name in NEGATING else 1):
                        break
                assert len(signs) == (2 if name in NEGATING else 1), (name, signs)
    return rows


def chain_cases(transform, rec):
    nS, nZ = len(CHAIN_SETS), len(STILLS)
    d_op = np.full((nS, N_SEEDS, nZ, 4), -2, dtype=np.int32)
    d_arg = np.full((nS, N_SEEDS, nZ, 4), np.nan, dtype=np.float64)
    out = np.zeros((nS, N_SEEDS, nZ, 1, 4, 4), dtype=np.float32)
    tail = np.zeros((nS, N_SEEDS, nZ, 2), dtype=np.float64)
    shear = np.zeros((nS, N_SEEDS, nZ), dtype=bool)
    for s, (aa, interp) in enumerate(CHAIN_SETS):
        for k in range(N_SEEDS):
            for z, (H, W) in enumerate(STILLS):
                random.seed(k)
                np.random.seed(k)
                rec.layers, STATE["shear"] = [], STATE["idle"]
                tf = transform.create_random_augment(input_size=(H, W), auto_augment=aa, interpolation=interp,
                                                     with_boxes=True)
                _, moved, _ = tf([Image.new("RGB", (W, H))], boxes=still_boxes(H, W, 1))
                tail[s, k, z] = [random.random(), np.random.uniform()]
                for n, (op, arg) in enumerate(rec.layers):
                    d_op[s, k, z, n], d_arg[s, k, z, n] = op, arg
                out[s, k, z] = moved
                shear[s, k, z] = any(op >= 0 and rec.names[op] in SHEARS and arg != 0 for op, arg in rec.layers)
                assert STATE["shear"] in (bool(shear[s, k, z]), None), (s, k, z)
    return d_op, d_arg, out, tail, shear


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", default=os.environ.get("SVIT_REFERENCE_ROOT"))
    ap.add_argument("--record-shear", action="store_true")
    args = ap.parse_args()
    root = args.reference
    if root is None:
        from oracle import ref_shim
        root = ref_shim.REFERENCE_ROOT
    utils, transform, erasing, mf, box_ops = load(root, args.record_shear)
    arrays = spatial_cases(utils, erasing, box_ops)

    names = sorted(mf.NAME_TO_OP)
    rec = Layers(mf, names)
    both_sets = sorted(set(mf._RAND_TRANSFORMS) | set(mf._RAND_INCREASING_TRANSFORMS))
    rows = op_cases(mf, rec, both_sets)
    d_op, d_arg, c_out, c_tail, c_shear = chain_cases(transform, rec)
    share = c_shear.mean((1, 2))
    assert all(c_shear[s].any() and (~c_shear[s]).any() for s in range(len(CHAIN_SETS)))
    assert all(sh <= 0.40 for sh, capped in zip(share, CHAIN_CAPPED) if capped), share
    op_shear = np.array([r[5] for r in rows])
    op_out = np.stack([r[4] for r in rows])
    chain_boxes = c_out.copy()
    if not args.record_shear:
        # boxes that went through the inert stand-in are not the reference's: they are not written
        op_out[op_shear] = np.nan
        chain_boxes[c_shear] = np.nan
    else:
        arrays.update(shear_op_out=op_out[op_shear], shear_chain_boxes=c_out[c_shear])
    arrays.update(
        names=np.array(names), stills=np.array(STILLS, dtype=np.int32),
        op_name=np.array([r[0] for r in rows], dtype=np.int32), op_size=np.array([r[1] for r in rows], dtype=np.int32),
        op_arg=np.array([r[2] for r in rows], dtype=np.float64), op_in=np.stack([r[3] for r in rows]), op_out=op_out,
        op_shear=op_shear, chain_op=d_op, chain_arg=d_arg, chain_boxes=chain_boxes, chain_tail=c_tail,
        chain_applied_shear=c_shear, chain_capped=np.array(CHAIN_CAPPED), chain_in=np.stack([still_boxes(H, W, 1) for H, W in STILLS]),
        set_aa=np.array([a for a, _ in CHAIN_SETS]), set_interp=np.array([i for _, i in CHAIN_SETS]),
        rotate_through_standin=np.array(not args.record_shear), shear_recorded=np.array(bool(args.record_shear)),
        note=np.array("Rotate boxes recorded through a computing cv2 stand-in (OpenCV's closed form of getRotationMatrix2D, "
                      "warpAffine -> zeros of the requested size); Shear boxes through an inert imgaug stand-in are NaN"
                      if not args.record_shear else "recorded with the real cv2 and imgaug"))
    np.savez_compressed(OUT, **arrays)
    print("wrote %s (%d bytes): %d single-op cases (%d shear), share of chains with a shear per policy %s"
          % (OUT, os.path.getsize(OUT), len(rows), int(op_shear.sum()), np.round(share, 3).tolist()))


if __name__ == "__main__":
    main()
