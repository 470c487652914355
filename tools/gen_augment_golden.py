"""Generate tests/golden/augment.npz from the UNMODIFIED reference `slowfast/datasets/{utils,transform,random_erasing}.py`
(development machine only: needs a reference checkout; the tests read the fixture, never the reference).

    python tools/gen_augment_golden.py [--reference /path/to/reference]

The reference modules are loaded from their files and RUN; only arrays they produced are written.  Packages the image lacks
(cv2, torchvision, iopath -- imported by those files, never used by the functions called here) get empty stand-ins.

Draws.  Per parameter set and seed 0..31 the pipeline of ssv2.py:345-426 -- `utils.spatial_sampling`, then
`RandomErasing` where the set has it -- runs on a zero clip [3,2,Hs,Ws] after `random.seed(s)`, `np.random.seed(s)`, with
(Hs, Ws) = SIZES[s % 4].  Every number the reference drew is recorded by wrapping, inside the loaded modules,
`_get_param_spatial_crop` (its return value, and whether it called `random.randint`: it does not on the central
fallback), `torch.nn.functional.interpolate` (the size asked for; not called = the jitter's early return) and `_get_pixels` (the erase box's size; top / left are read from the region the
reference wrote in a NaN-marked clip); crop offsets and flip are read from the output of a coordinate clip.  After the
pipeline the position of both streams is recorded too (`stream_tail`) -- a sampler that consumed a different number of
draws does not reproduce it.

Sets: the reference's configs/ssv2.yaml values; scale jitter without AUG (scales 224..228 so that the short side == size
early return occurs); ssv2.yaml with RANDOM_FLIP on; ssv2.yaml with RE_MODE const, RE_PROB 1; scale jitter 256..320 with
INV_UNIFORM_SAMPLE and RANDOM_FLIP.

Outputs.  For the first N_OUT seeds of three sets, the reference's own result on the closed-form uint8 clip `frames_u8()`
[2,4,40,56,3] at S = 32 (normalised as utils.tensor_normalize does): `spatial_sampling` with the set's parameters scaled to
that size, then const-mode erasing with probability 1.
"""
import argparse
import importlib
import os
import random
import sys
import types

sys.dont_write_bytecode = True

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden", "augment.npz")

N_SEEDS, N_OUT = 32, 4
SIZES = [(240, 320), (32, 224), (320, 240), (224, 300)]
SET_NAMES = ["ssv2", "jitter", "flip", "const", "jitter_inv"]
# aug (AUG.ENABLE), TRAIN_JITTER_SCALES, RANDOM_FLIP, INV_UNIFORM_SAMPLE, RE_PROB, RE_MODE
SETS = [
    dict(aug=True, scales=(256, 320), flip=False, inv=False, re_prob=0.25, re_mode="pixel"),
    dict(aug=False, scales=(224, 228), flip=False, inv=False, re_prob=0.0, re_mode="const"),
    dict(aug=True, scales=(256, 320), flip=True, inv=False, re_prob=0.25, re_mode="pixel"),
    dict(aug=True, scales=(256, 320), flip=False, inv=False, re_prob=1.0, re_mode="const"),
    dict(aug=False, scales=(256, 320), flip=True, inv=True, re_prob=0.0, re_mode="const"),
]
REL_SCALE, REL_ASPECT, CROP = [0.08, 1.0], [0.75, 1.3333], 224
MEAN, STD = [0.45, 0.45, 0.45], [0.225, 0.225, 0.225]
# the output cases: (set index, jitter scales at the small size)
OUT_SHAPE, OUT_S = (2, 4, 40, 56, 3), 32
OUT_SETS = [(2, None), (1, (36, 44)), (4, (36, 44))]


def frames_u8():
    """closed form: ((131 i) mod 251 + 3 (i mod 2)) mod 256 over the flat index"""
    n = int(np.prod(OUT_SHAPE))
    i = np.arange(n, dtype=np.int64)
    return (((i * 131) % 251 + 3 * (i % 2)) % 256).astype(np.uint8).reshape(OUT_SHAPE)


class _Stub(types.ModuleType):
    """an absent plumbing package: any name imported from it is None (nothing called here uses one)"""

    def __getattr__(self, name):
        if name.startswith("__"):
            raise AttributeError(name)
        return None


def load_reference(root):
    for name in ("cv2", "torchvision", "torchvision.transforms", "torchvision.transforms.functional", "iopath",
                 "iopath.common", "iopath.common.file_io", "torchvision.ops", "torchvision.ops.boxes"):
        if name not in sys.modules:
            try:
                importlib.import_module(name)
            except ImportError:
                sys.modules[name] = _Stub(name)
    fio = sys.modules["iopath.common.file_io"]
    if getattr(fio, "PathManagerFactory", None) is None:
        fio.PathManagerFactory = type("PathManagerFactory", (), {"get": staticmethod(lambda *a, **k: None)})
    tv = sys.modules["torchvision"]
    if getattr(tv, "transforms", None) is None:
        tv.transforms = sys.modules["torchvision.transforms"]
    if getattr(tv.transforms, "functional", None) is None:
        tv.transforms.functional = sys.modules["torchvision.transforms.functional"]
    # the packages as bare namespaces over the reference's directories: their __init__ files (which import every
    # dataset) do not run
    for pkg, sub in (("slowfast", "slowfast"), ("slowfast.datasets", "slowfast/datasets"), ("slowfast.utils", "slowfast/utils")):
        if pkg not in sys.modules:
            m = types.ModuleType(pkg)
            m.__path__ = [os.path.join(root, sub)]
            sys.modules[pkg] = m
    utils = importlib.import_module("slowfast.datasets.utils")
    transform = importlib.import_module("slowfast.datasets.transform")
    erasing = importlib.import_module("slowfast.datasets.random_erasing")
    assert os.path.realpath(utils.__file__).startswith(os.path.realpath(root))
    return utils, transform, erasing


class Recorder:
    """wraps what the reference calls inside its own modules; remembers the numbers"""

    def __init__(self, transform, erasing):
        self.t, self.e = transform, erasing
        self.reset()
        orig_param = transform._get_param_spatial_crop
        orig_interp = torch.nn.functional.interpolate
        orig_pixels = erasing._get_pixels
        rec = self

        def param(*a, **kw):
            calls = []
            orig_randint = random.randint
            random.randint = lambda lo, hi: (calls.append(1), orig_randint(lo, hi))[1]
            try:
                out = orig_param(*a, **kw)
            finally:
                random.randint = orig_randint
            rec.rrc, rec.fallback = tuple(int(v) for v in out), not calls
            return out

        def interp(x, size=None, **kw):
            rec.interp_sizes.append(tuple(int(v) for v in size))
            return orig_interp(x, size=size, **kw)

        def pixels(per_pixel, rand_color, patch_size, **kw):
            rec.erase_hw = (int(patch_size[1]), int(patch_size[2]))
            return orig_pixels(per_pixel, rand_color, patch_size, **kw)

        transform._get_param_spatial_crop = param
        # (transform.py calls torch.nn.functional.interpolate through the torch module: wrap it there for the run)
        self._interp, self._orig_interp = interp, orig_interp
        erasing._get_pixels = pixels

    def reset(self):
        self.rrc, self.fallback, self.interp_sizes, self.erase_hw = None, False, [], None

    def __enter__(self):
        torch.nn.functional.interpolate = self._interp
        return self

    def __exit__(self, *exc):
        torch.nn.functional.interpolate = self._orig_interp


def run(utils, erasing, rec, p, seed, clip, crop, scales):
    """the reference's pipeline on `clip` f32 [3,T,H,W] -> (numbers dict, output [3,T,crop,crop])"""
    rec.reset()
    random.seed(seed)
    np.random.seed(seed)
    H, W = clip.shape[2], clip.shape[3]
    kw = dict(spatial_idx=-1, min_scale=scales[0], max_scale=scales[1], crop_size=crop,
              random_horizontal_flip=p["flip"], inverse_uniform_sampling=p["inv"])
    if p["aug"]:
        kw.update(aspect_ratio=REL_ASPECT, scale=REL_SCALE, motion_shift=False)
    with rec:
        out = utils.spatial_sampling(clip.clone(), **kw)
    n = dict(i=0, j=0, h=H, w=W, out_h=H, out_w=W, oy=0, ox=0, flip=0, erased=0, et=0, el=0, eh=0, ew=0, fallback=0,
             jitter_identity=0)
    if p["aug"]:
        n.update(i=rec.rrc[0], j=rec.rrc[1], h=rec.rrc[2], w=rec.rrc[3], out_h=crop, out_w=crop, fallback=int(rec.fallback))
        assert rec.interp_sizes == [(crop, crop)]
    else:
        if rec.interp_sizes:
            (n["out_h"], n["out_w"]), = rec.interp_sizes
        else:
            n["jitter_identity"] = 1
    if p["re_prob"] > 0:
        er = erasing.RandomErasing(p["re_prob"], mode=p["re_mode"], max_count=1, num_splits=1, device="cpu")
        marked = out.permute(1, 0, 2, 3).clone()
        marked[:] = float("nan")
        state = random.getstate()
        er(marked)
        random.setstate(state)
        out = er(out.permute(1, 0, 2, 3).clone()).permute(1, 0, 2, 3)
        hit = ~torch.isnan(marked[0, 0])
        if rec.erase_hw is not None:
            n["erased"] = 1
            n["eh"], n["ew"] = rec.erase_hw
            ys, xs = hit.any(1).nonzero().flatten(), hit.any(0).nonzero().flatten()
            n["et"], n["el"] = (int(ys[0]), int(xs[0])) if len(ys) else (0, 0)
            assert int(hit.sum()) == n["eh"] * n["ew"]
    return n, out


def locate(ref_out, resampled, flip, erased_box):
    """(oy, ox, flip) of the reference's crop: the window of `resampled` [3,T,h,w] that equals `ref_out` outside the box"""
    S = ref_out.shape[-1]
    mask = torch.ones(S, S, dtype=torch.bool)
    if erased_box is not None:
        t, l, h, w = erased_box
        mask[t:t + h, l:l + w] = False
    found = []
    for f in ((0, 1) if flip else (0,)):
        r = ref_out.flip(-1) if f else ref_out
        m = mask.flip(-1) if f else mask
        for oy in range(resampled.shape[2] - S + 1):
            for ox in range(resampled.shape[3] - S + 1):
                if torch.equal(resampled[:, :, oy:oy + S, ox:ox + S][..., m], r[..., m]):
                    found.append((oy, ox, f))
    return found


def locate_coord(out, resampled, S):
    """the same for a coordinate clip (channel 0 = row index, channel 1 = column index before the rescale): the
    window is read off its first row / column"""
    rows, cols = resampled[0, 0, :, 0], resampled[1, 0, 0, :]
    line = out[1, 0, 0]
    flip = int(line[0] > line[-1])
    # (an upscale repeats the border rows / columns: several candidates there, one of them gives the window)
    found = []
    for oy in (rows == out[0, 0, 0, 0]).nonzero().flatten().tolist():
        for ox in (cols == (line[-1] if flip else line[0])).nonzero().flatten().tolist():
            win = resampled[:, :, oy:oy + S, ox:ox + S]
            if win.shape[-2:] == out.shape[-2:] and torch.equal(win.flip(-1) if flip else win, out):
                found.append((oy, ox))
    assert len(found) == 1, found
    (oy, ox), = found
    return oy, ox, flip


def stream_tail():
    """position of both streams after the reference's pipeline: the next random.random() and np.random.uniform(); and,
    from the same position of `random`, getrandbits(31) followed by random.random() -- what a sampler that draws its
    noise seed there must show"""
    state = random.getstate()
    r = random.random()
    random.setstate(state)
    seed = random.getrandbits(31)
    r2 = random.random()
    return [r, np.random.uniform(), float(seed), r2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", default=os.environ.get("SVIT_REFERENCE_ROOT"))
    args = ap.parse_args()
    root = args.reference
    if root is None:
        sys.path.insert(0, ROOT)
        from oracle import ref_shim
        root = ref_shim.REFERENCE_ROOT
    utils, transform, erasing = load_reference(root)
    rec = Recorder(transform, erasing)
    keys = ["i", "j", "h", "w", "out_h", "out_w", "oy", "ox", "flip", "erased", "et", "el", "eh", "ew", "fallback",
            "jitter_identity"]
    nS = len(SETS)
    draws = np.zeros((nS, N_SEEDS, len(keys)), dtype=np.int32)
    tail = np.zeros((nS, N_SEEDS, 4), dtype=np.float64)
    for s, p in enumerate(SETS):
        for k in range(N_SEEDS):
            H, W = SIZES[k % len(SIZES)]
            clip = torch.zeros(3, 2, H, W)
            if not p["aug"]:
                # the crop offsets and the flip are not returned by the reference: a coordinate clip makes them readable
                clip[0] = torch.arange(H, dtype=torch.float32)[None, :, None]
                clip[1] = torch.arange(W, dtype=torch.float32)[None, None, :]
            n, out = run(utils, erasing, rec, p, k, clip, CROP, p["scales"])
            tail[s, k] = stream_tail()
            if not p["aug"]:
                # rows / columns of the rescaled coordinate clip are monotone: the window is where the output starts
                resampled = clip if n["jitter_identity"] else torch.nn.functional.interpolate(
                    clip, size=(n["out_h"], n["out_w"]), mode="bilinear", align_corners=False)
                n["oy"], n["ox"], n["flip"] = locate_coord(out, resampled, CROP)
                assert p["flip"] or not n["flip"]
            elif p["flip"]:
                # random-resized crop: re-run with a coordinate clip to read the flip
                clip[1] = torch.arange(W, dtype=torch.float32)[None, None, :]
                _, out2 = run(utils, erasing, rec, dict(p, re_prob=0.0), k, clip, CROP, p["scales"])
                row = out2[1, 0, 0]
                n["flip"] = int(row[0] > row[-1])
            draws[s, k] = [n[key] for key in keys]

    # ---- the reference's outputs on the closed-form clip -------------------------------------
    fr = frames_u8()
    out_meta, out_vals = [], []
    for s, scales in OUT_SETS:
        p = dict(SETS[s], re_prob=1.0, re_mode="const")
        for k in range(N_OUT):
            v = k % OUT_SHAPE[0]
            clip = utils.tensor_normalize(torch.from_numpy(fr[v]), MEAN, STD).permute(3, 0, 1, 2)
            n, out = run(utils, erasing, rec, p, k, clip, OUT_S, scales or p["scales"])
            box = (n["et"], n["el"], n["eh"], n["ew"]) if n["erased"] else None
            if not p["aug"]:
                resampled = clip if n["jitter_identity"] else torch.nn.functional.interpolate(
                    clip, size=(n["out_h"], n["out_w"]), mode="bilinear", align_corners=False)
                found = locate(out, resampled, p["flip"], box)
                assert len(found) == 1, (s, k, found)
                n["oy"], n["ox"], n["flip"] = found[0]
            elif p["flip"]:
                resampled = torch.nn.functional.interpolate(
                    clip[:, :, n["i"]:n["i"] + n["h"], n["j"]:n["j"] + n["w"]], size=(OUT_S, OUT_S), mode="bilinear",
                    align_corners=False)
                found = locate(out, resampled, True, box)
                assert len(found) == 1, (s, k, found)
                n["flip"] = found[0][2]
            out_meta.append([s, k, v] + [n[key] for key in keys])
            out_vals.append(out.numpy().astype(np.float32))

    d = {key: draws[..., c] for c, key in enumerate(keys)}
    assert d["fallback"].any(), "no central-fallback draw"
    assert d["jitter_identity"].any(), "no short side == size early return"
    assert (~d["fallback"].astype(bool))[0].any() and d["erased"][0].any() and (1 - d["erased"][0]).any()
    assert d["flip"][2].any() and (1 - d["flip"][2]).any()
    assert d["erased"][3].all()
    np.savez_compressed(
        OUT, set_names=np.array(SET_NAMES), keys=np.array(keys), sizes=np.array(SIZES, dtype=np.int32),
        set_aug=np.array([p["aug"] for p in SETS]), set_scales=np.array([p["scales"] for p in SETS], dtype=np.int32),
        set_flip=np.array([p["flip"] for p in SETS]), set_inv=np.array([p["inv"] for p in SETS]),
        set_re_prob=np.array([p["re_prob"] for p in SETS]), set_re_mode=np.array([p["re_mode"] for p in SETS]),
        rel_scale=np.array(REL_SCALE), rel_aspect=np.array(REL_ASPECT), crop=np.int32(CROP),
        mean=np.array(MEAN), std=np.array(STD), draws=draws, tail=tail,
        out_size=np.int32(OUT_S), out_keys=np.array(["set", "seed", "video"] + keys),
        out_jitter_scales=np.array([sc or (0, 0) for _, sc in OUT_SETS], dtype=np.int32),
        out_sets=np.array([s for s, _ in OUT_SETS], dtype=np.int32),
        out_meta=np.array(out_meta, dtype=np.int32), out_clips=np.stack(out_vals))
    print("wrote %s (%d bytes): fallback %d, jitter identity %d, erased %s, flips %s"
          % (OUT, os.path.getsize(OUT), int(d["fallback"].sum()), int(d["jitter_identity"].sum()),
             d["erased"].sum(1).tolist(), d["flip"].sum(1).tolist()))


if __name__ == "__main__":
    main()
