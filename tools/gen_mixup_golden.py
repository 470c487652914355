"""Generate tests/golden/mixup.npz from the UNMODIFIED reference `slowfast/datasets/mixup.py` (development machine
only: needs a reference checkout; the tests read the fixture, never the reference).

    python tools/gen_mixup_golden.py [--reference /path/to/reference]

The reference module is loaded by path with importlib and RUN; only arrays it produced are written.  Per parameter set
(the reference's configs/ssv2.yaml values; PROB 0.5; mixup only; CutMix only) and seed 0..31, after `np.random.seed(s)`:
the lambda `MixUp._mix_batch` returned (float64; area-corrected for CutMix), whether it took the CutMix branch, the box it
drew for a 224 x 224 clip, and the [4,174] soft target of `MixUp.__call__` for four fixed labels.  For four seeds per set:
the tiny clip [4,3,2,16,16] (closed-form input, `tiny_clip()` below) after `MixUp.__call__`, with its lambda / flag / box
/ target.  The tiny seeds are the first ones of 0..255 that show an empty box (where the set has CutMix), then the
smallest others.
"""
import argparse
import importlib.util
import os
import sys

sys.dont_write_bytecode = True

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden", "mixup.npz")

NUM_CLASSES, SMOOTHING = 174, 0.1
LABELS = [3, 171, 42, 3]            # (two equal labels on purpose: rows 0 and 3 are partners)
SET_NAMES = ["ssv2", "prob05", "mixup_only", "cutmix_only"]
# (ALPHA, CUTMIX_ALPHA, PROB, SWITCH_PROB)
SET_PARAMS = [(0.8, 1.0, 1.0, 0.5), (0.8, 1.0, 0.5, 0.5), (0.8, 0.0, 1.0, 0.5), (0.0, 1.0, 1.0, 0.5)]
N_SEEDS, N_TINY, TINY_SCAN = 32, 4, 256
BIG, TINY = (4, 1, 1, 224, 224), (4, 3, 2, 16, 16)


def tiny_clip():
    """closed form, exact in fp32: ((37 i) mod 101 - 50) / 16 over the flat index"""
    n = int(np.prod(TINY))
    v = ((np.arange(n, dtype=np.int64) * 37) % 101 - 50).astype(np.float32) / np.float32(16)
    return v.reshape(TINY)


def load_reference(root):
    path = os.path.join(root, "slowfast", "datasets", "mixup.py")
    spec = importlib.util.spec_from_file_location("_reference_mixup", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


class BoxRecorder:
    """wraps the reference's get_cutmix_bbox inside the loaded module: remembers the box it returned"""

    def __init__(self, mod):
        self.orig, self.box = mod.get_cutmix_bbox, None
        mod.get_cutmix_bbox = self

    def __call__(self, *a, **kw):
        (yl, yh, xl, xh), lam = self.orig(*a, **kw)
        self.box = (int(yl), int(yh), int(xl), int(xh))
        return (yl, yh, xl, xh), lam


def run(mod, rec, params, seed, x):
    """-> (lam float64, cutmix flag, box, target [4,C] f32, mixed x) of the reference for this seed"""
    alpha, cm_alpha, prob, switch = params
    fn = mod.MixUp(mixup_alpha=alpha, cutmix_alpha=cm_alpha, mix_prob=prob, switch_prob=switch,
                   label_smoothing=SMOOTHING, num_classes=NUM_CLASSES)
    labels = torch.tensor(LABELS)
    rec.box = None
    np.random.seed(seed)
    lam = float(fn._mix_batch(torch.zeros(x.shape)))
    box_a = rec.box
    rec.box = None
    np.random.seed(seed)
    xm, target = fn(torch.from_numpy(x.copy()), labels)
    assert rec.box == box_a
    cutmix = rec.box is not None
    return lam, cutmix, rec.box or (0, 0, 0, 0), target.numpy().astype(np.float32), xm.numpy()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", default=os.environ.get("SVIT_REFERENCE_ROOT"))
    args = ap.parse_args()
    root = args.reference
    if root is None:
        sys.path.insert(0, ROOT)
        from oracle import ref_shim
        root = ref_shim.REFERENCE_ROOT
    mod = load_reference(root)
    rec = BoxRecorder(mod)
    S, K = len(SET_PARAMS), N_SEEDS
    out = {
        "set_names": np.array(SET_NAMES), "set_params": np.array(SET_PARAMS, dtype=np.float64),
        "labels": np.array(LABELS, dtype=np.int64), "num_classes": np.int64(NUM_CLASSES),
        "smoothing": np.float64(SMOOTHING),
        "lam": np.zeros((S, K)), "cutmix": np.zeros((S, K), dtype=np.bool_),
        "box": np.zeros((S, K, 4), dtype=np.int32), "target": np.zeros((S, K, 4, NUM_CLASSES), dtype=np.float32),
        "tiny_seeds": np.zeros((S, N_TINY), dtype=np.int64), "tiny_lam": np.zeros((S, N_TINY)),
        "tiny_cutmix": np.zeros((S, N_TINY), dtype=np.bool_), "tiny_box": np.zeros((S, N_TINY, 4), dtype=np.int32),
        "tiny_target": np.zeros((S, N_TINY, 4, NUM_CLASSES), dtype=np.float32),
        "tiny_mixed": np.zeros((S, N_TINY) + TINY, dtype=np.float32),
    }
    big = np.zeros(BIG, dtype=np.float32)
    tiny = tiny_clip()
    for s, params in enumerate(SET_PARAMS):
        for k in range(K):
            lam, cm, box, target, _ = run(mod, rec, params, k, big)
            out["lam"][s, k], out["cutmix"][s, k], out["box"][s, k], out["target"][s, k] = lam, cm, box, target
        scan = [run(mod, rec, params, k, tiny) for k in range(TINY_SCAN)]
        empty = [k for k, r in enumerate(scan) if r[1] and (r[2][0] == r[2][1] or r[2][2] == r[2][3])][:1]
        seeds = sorted(empty + [k for k in range(TINY_SCAN) if k not in empty][:N_TINY - len(empty)])
        for j, k in enumerate(seeds):
            lam, cm, box, target, xm = scan[k]
            out["tiny_seeds"][s, j], out["tiny_lam"][s, j], out["tiny_cutmix"][s, j] = k, lam, cm
            out["tiny_box"][s, j], out["tiny_target"][s, j], out["tiny_mixed"][s, j] = box, target, xm

    # the set must contain the cases the tests are there for
    lam, cm, box = out["lam"], out["cutmix"], out["box"].astype(np.int64)
    assert (~cm & (lam != 1.0)).any(), "no mixup draw"
    area = (box[..., 1] - box[..., 0]) * (box[..., 3] - box[..., 2])
    touches = (box[..., 0] == 0) | (box[..., 1] == 224) | (box[..., 2] == 0) | (box[..., 3] == 224)
    height, width = box[..., 1] - box[..., 0], box[..., 3] - box[..., 2]
    clipped = cm & touches & (height != width)            # a square box cut by a border: lam was area-corrected
    assert clipped.any(), "no CutMix box clipped by a border"
    assert np.allclose(lam[clipped], 1.0 - area[clipped] / (224.0 * 224.0), rtol=0, atol=0)
    assert (lam == 1.0).any(), "no lam == 1.0 draw"
    tb = out["tiny_box"].astype(np.int64)
    tiny_empty = out["tiny_cutmix"] & ((tb[..., 0] == tb[..., 1]) | (tb[..., 2] == tb[..., 3]))
    assert tiny_empty.any(), "no empty box"
    assert (out["tiny_lam"][tiny_empty] == 1.0).all()
    np.savez_compressed(OUT, **out)
    print("wrote %s (%d bytes): %d mixup, %d CutMix (%d clipped), %d unmixed draws; tiny seeds %s"
          % (OUT, os.path.getsize(OUT), int((~cm & (lam != 1.0)).sum()), int(cm.sum()), int(clipped.sum()),
             int((lam == 1.0).sum()), out["tiny_seeds"].tolist()))


if __name__ == "__main__":
    main()
