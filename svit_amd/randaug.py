"""Device-side RandAugment for uint8 clips (cfg.AUG.AA_TYPE / cfg.AUG.INTERPOLATION), byte-equal to PIL.

The reference's loader sends every training clip through `create_random_augment(...)` first (ssv2.py:345-375,
datasets/rand_augment.py): N randomly chosen PIL operations on each uint8 frame at source resolution, before normalisation
and the spatial pipeline of svit_amd/augment.py.  Here what was drawn for a clip is N 64-byte RECORDS (`RandAugOp`,
`struct SvitRandAugOp` of include/svit_hip.h) in device memory and two kernels per layer (csrc/randaug.hip) apply them to
the frames where they lie: `svit_randaug_stats` (per-frame histogram -> AutoContrast / Equalize table, Contrast mean) and
`svit_randaug_apply`.  Every operation is integer, fp32 or fp64 arithmetic in PIL's own order, so the result is PIL's to
the byte; `apply_host` is the same arithmetic in NumPy and the kernels' yardstick.  PIL is not imported here.

    ra = build_randaug(cfg)                                             # None unless cfg.AUG.ENABLE
    table = pack_table([ra.draw(T, Hs, Ws, video=v) for v in range(V)]) # int32 [V,N,16]; BEFORE SpatialSampler.draw
    clips = AugClips(frames_u8, size, records, mean, std, randaug=table)

The draws.  `RandAugSampler.draw` consumes `np.random` and `random` as the reference does for one clip: one
`np.random.choice` of the N operations (weighted and without replacement under `w0`), then per layer `random.random()`
against the operation's probability 0.5 (a skip draws nothing more), `random.gauss(m, mstd)` where mstd > 0, the clip to
[0, 10], the level function (one `random.random()` where it negates) and, for the geometric operations under
INTERPOLATION "random", one `random.choice` PER FRAME.  Two quirks of the reference's grammar are kept: `inc0` selects the
increasing set (`bool("0")`), and the `w0` weights are listed by the plain set's names whichever set is used.  The
reference also sets `translate_const = int(min(Hs, Ws) * 0.45)`; only the absolute translations read it and neither set
holds one.

Videos of different sizes in one batch: the buffer is padded to a common [V,T,Hs,Ws,3] and `extents` int32 [V,2] =
(h_v, w_v) says where each video lies (top-left corner, pitch Ws; `augment.pack_videos` builds both).  Draw each clip for
its OWN size -- `ra.draw(T, h_v, w_v)` -- and pass the table to `apply(..., extents=)` / `apply_host(..., extents=)`:
inside its extent every video gets the bytes it would get alone as a tight h_v x w_v clip (histograms, the Contrast mean,
the affine fill boundary and tap clamps, the Sharpness border ring); the padding is copied.  None: every video fills the
buffer, the launches and bytes of before.

Boxes (the image ranks: `Ssv2_frames` sends every still through `create_random_augment(..., with_boxes=True)`,
ssv2_frames.py:373-398, and its hand / object boxes move with the pixels).  `ra.draw(T, Hs, Ws, boxes=b)` with b float32
[T,O,4] (xyxy, source pixels) returns `(records, boxes_out)`; the draws are those of the box-aware transform
(ssv2_MF/autoaugment.py), which consumes both streams exactly as the plain one.  Per layer (`boxes_layer`) the
photometric operations leave the boxes, TranslateXRel / TranslateYRel and Rotate are the reference's arithmetic
(boxes_autoaugment.py, boxes_aug/bbox_util.py::rotate_boxes with its `clip_box(..., 0.25)` zeroing), and all-zero rows
are zero again after every layer.  ShearX / ShearY are NOT the reference's numbers: its box functions go through imgaug's
fitted canvas; here the box is the enclosing box of the four corners under the affine map the pixel kernel applies for
that record (x' = x - f y; ShearY y' = y - f x), clipped to the image -- consistent with the pixels produced, a
documented deviation for 2 of the 15 operations.

Out of scope: AUG.NUM_SAMPLE > 1, AUG.COLOR_JITTER (the reference's loader never reads it),
policies other than `rand-...`, frames smaller than 3 x 3.
"""
import collections
import math
import random
import re

import numpy as np

OP_NONE, OP_AUTOCONTRAST, OP_EQUALIZE, OP_INVERT, OP_POSTERIZE, OP_SOLARIZE, OP_SOLARIZE_ADD = 0, 1, 2, 3, 4, 5, 6
OP_COLOR, OP_CONTRAST, OP_BRIGHTNESS, OP_SHARPNESS, OP_AFFINE = 7, 8, 9, 10, 11
BILINEAR, BICUBIC = 0, 1
FILL = 128
MAX_LEVEL = 10.0
SLOT_BYTES = 1024           # workspace per (video, frame): 3 x 256 table bytes, the Contrast mean as int32 at byte 768

RAND_TRANSFORMS = ["AutoContrast", "Equalize", "Invert", "Rotate", "Posterize", "Solarize", "SolarizeAdd", "Color",
                   "Contrast", "Brightness", "Sharpness", "ShearX", "ShearY", "TranslateXRel", "TranslateYRel"]
RAND_INCREASING_TRANSFORMS = ["AutoContrast", "Equalize", "Invert", "Rotate", "PosterizeIncreasing", "SolarizeIncreasing",
                              "SolarizeAdd", "ColorIncreasing", "ContrastIncreasing", "BrightnessIncreasing",
                              "SharpnessIncreasing", "ShearX", "ShearY", "TranslateXRel", "TranslateYRel"]
RAND_CHOICE_WEIGHTS_0 = {"Rotate": 0.3, "ShearX": 0.2, "ShearY": 0.2, "TranslateXRel": 0.1, "TranslateYRel": 0.1,
                         "Color": 0.025, "Sharpness": 0.025, "AutoContrast": 0.025, "Solarize": 0.005,
                         "SolarizeAdd": 0.005, "Contrast": 0.005, "Brightness": 0.005, "Equalize": 0.005, "Posterize": 0,
                         "Invert": 0}
GEOMETRIC = ("Rotate", "ShearX", "ShearY", "TranslateXRel", "TranslateYRel")
ENHANCE = {"Color": OP_COLOR, "Contrast": OP_CONTRAST, "Brightness": OP_BRIGHTNESS, "Sharpness": OP_SHARPNESS}
IDENTITY = (1.0, 0.0, 0.0, 0.0, 1.0, 0.0)


class RandAugOp(collections.namedtuple("RandAugOp", "op arg_i arg_f bicubic_mask m")):
    """One layer of one clip, the 64 bytes of `struct SvitRandAugOp`: op; arg_i (bits kept / threshold / addend); arg_f
    (the enhancement factor, fp32); bicubic_mask (bit t: frame t is resampled bicubically); m, six float64 of the
    output -> input affine map."""
    __slots__ = ()

    def __new__(cls, op=OP_NONE, arg_i=0, arg_f=0.0, bicubic_mask=0, m=IDENTITY):
        return super().__new__(cls, int(op), int(arg_i), float(arg_f), int(bicubic_mask), tuple(float(v) for v in m))

    def pack(self):
        w = np.zeros(16, dtype=np.int32)
        w[0], w[1] = self.op, self.arg_i
        w[2:3] = np.array([self.arg_f], dtype=np.float32).view(np.int32)
        w[3:4] = np.array([self.bicubic_mask & 0xFFFFFFFF], dtype=np.uint32).view(np.int32)
        w[4:16] = np.array(self.m, dtype=np.float64).view(np.int32)
        return w

    @classmethod
    def unpack(cls, words):
        w = np.ascontiguousarray(np.asarray(words, dtype=np.int32).reshape(16))
        return cls(int(w[0]), int(w[1]), float(w[2:3].view(np.float32)[0]), int(w[3:4].view(np.uint32)[0]),
                   w[4:16].view(np.float64).tolist())


def pack_table(ops):
    """V lists of N RandAugOp (or an int [V,N,16] array) -> int32 [V,N,16] NumPy array"""
    if isinstance(ops, np.ndarray):
        t = np.ascontiguousarray(ops.astype(np.int32))
    else:
        t = np.stack([np.stack([RandAugOp(*o).pack() for o in layers]) for layers in ops])
    if t.ndim != 3 or t.shape[2] != 16 or t.shape[1] < 1:
        raise ValueError("the RandAugment table is int32 [V,N,16] with N >= 1, got %s" % (tuple(t.shape),))
    return t


# ---- the reference's grammar (rand_augment.py:483-533) -------------------------------------------------------------
def parse_aa_type(s):
    """'rand-m7-n4-mstd0.5-inc1' -> dict(magnitude, num_layers, magnitude_std, transforms, weights)"""
    config = str(s).split("-")
    if config[0] != "rand":
        raise NotImplementedError("AUG.AA_TYPE %r: only the rand-... policies are supported" % (s,))
    out = dict(magnitude=int(MAX_LEVEL), num_layers=2, magnitude_std=0.0, transforms=list(RAND_TRANSFORMS), weights=None)
    mstd = None
    for c in config[1:]:
        cs = re.split(r"(\d.*)", c)
        if len(cs) < 2:
            continue
        key, val = cs[:2]
        if key == "mstd":
            if mstd is None:                    # (the reference's hparams.setdefault: the first one holds)
                mstd = float(val)
        elif key == "inc":
            if bool(val):                       # the reference's quirk: val is a string, so inc0 is true as well
                out["transforms"] = list(RAND_INCREASING_TRANSFORMS)
        elif key == "m":
            out["magnitude"] = int(val)
        elif key == "n":
            out["num_layers"] = int(val)
        elif key == "w":
            if int(val) != 0:
                raise ValueError("AUG.AA_TYPE %r: only the weight set 0 exists" % (s,))
            # the reference's quirk: the weights are listed by the PLAIN set's names, position by position
            probs = [RAND_CHOICE_WEIGHTS_0[k] for k in RAND_TRANSFORMS]
            out["weights"] = probs / np.sum(probs)
    out["magnitude_std"] = mstd or 0.0
    return out


def _negate(v):
    return -v if random.random() > 0.5 else v


def _level_args(name, level):
    """the reference's LEVEL_TO_ARG functions, in its float arithmetic"""
    base = name.replace("Increasing", "")
    inc = name.endswith("Increasing")
    if base in ("AutoContrast", "Equalize", "Invert"):
        return ()
    if base == "Rotate":
        return (_negate((level / MAX_LEVEL) * 30.0),)
    if base in ENHANCE:
        return (1.0 + _negate((level / MAX_LEVEL) * 0.9),) if inc else ((level / MAX_LEVEL) * 1.8 + 0.1,)
    if base in ("ShearX", "ShearY"):
        return (_negate((level / MAX_LEVEL) * 0.3),)
    if base in ("TranslateXRel", "TranslateYRel"):
        return (_negate((level / MAX_LEVEL) * 0.45),)
    if base == "Posterize":
        v = int((level / MAX_LEVEL) * 4)
        return (4 - v,) if inc else (v,)
    if base == "Solarize":
        v = int((level / MAX_LEVEL) * 256)
        return (256 - v,) if inc else (v,)
    if base == "SolarizeAdd":
        return (int((level / MAX_LEVEL) * 110),)
    raise ValueError(name)


def rotate_matrix(degrees, width, height):
    """PIL's Image.rotate about the centre -> the six coefficients (None: the angle is a multiple of 360, a copy)"""
    angle = degrees % 360.0
    if angle == 0:
        return None
    cx, cy = width / 2.0, height / 2.0
    angle = -math.radians(angle)
    m = [round(math.cos(angle), 15), round(math.sin(angle), 15), 0.0,
         round(-math.sin(angle), 15), round(math.cos(angle), 15), 0.0]
    a, b, c, d, e, f = m
    m[2], m[5] = a * -cx + b * -cy + c, d * -cx + e * -cy + f
    m[2] += cx
    m[5] += cy
    return tuple(m)


def make_op(name, args, filters, Hs, Ws):
    """operation name + level arguments + per-frame filters (0 bilinear / 1 bicubic) -> RandAugOp"""
    base = name.replace("Increasing", "")
    if base == "AutoContrast":
        return RandAugOp(OP_AUTOCONTRAST)
    if base == "Equalize":
        return RandAugOp(OP_EQUALIZE)
    if base == "Invert":
        return RandAugOp(OP_INVERT)
    if base == "Posterize":
        return RandAugOp(OP_POSTERIZE, arg_i=args[0])
    if base == "Solarize":
        return RandAugOp(OP_SOLARIZE, arg_i=args[0])
    if base == "SolarizeAdd":
        return RandAugOp(OP_SOLARIZE_ADD, arg_i=args[0])
    if base in ENHANCE:
        return RandAugOp(ENHANCE[base], arg_f=float(np.float32(args[0])))
    v = args[0]
    if base == "Rotate":
        m = rotate_matrix(v, Ws, Hs)
        if m is None:
            return RandAugOp(OP_NONE)
    elif base == "ShearX":
        m = (1, v, 0, 0, 1, 0)
    elif base == "ShearY":
        m = (1, 0, 0, v, 1, 0)
    elif base == "TranslateXRel":
        m = (1, 0, v * Ws, 0, 1, 0)
    elif base == "TranslateYRel":
        m = (1, 0, 0, 0, 1, v * Hs)
    else:
        raise ValueError(name)
    mask = 0
    for t, f in enumerate(filters):
        mask |= (1 if f else 0) << (t & 31)
    return RandAugOp(OP_AFFINE, bicubic_mask=mask, m=m)


# ---- the box side of a layer (ssv2_MF/autoaugment.py::AugmentOp.__call__, boxes_autoaugment.py, boxes_aug/bbox_util.py) ----
def as_boxes(boxes, ndim=None):
    """a tensor or array of boxes -> a float32 NumPy copy [..., 4] (ndim: the rank it must have)"""
    b = np.array(boxes.detach().cpu().numpy() if hasattr(boxes, "detach") else boxes, dtype=np.float32)
    if b.shape[-1:] != (4,) or (ndim is not None and b.ndim != ndim):
        raise ValueError("boxes are float32 %s (xyxy), got %s" % ("[T,O,4]" if ndim == 3 else "[..., 4]", tuple(b.shape)))
    return b


def rotate_boxes(boxes, degrees, Hs, Ws):
    """`bbox_util.rotate_boxes` restated for float32 [N,4]: the corners through OpenCV's rotation matrix about
    (Ws // 2, Hs // 2) on the fitted canvas, their enclosing box, the centre crop back to Ws x Hs and `clip_box(...,
    0.25)` -- a box that keeps less than a quarter of its area inside the image (or has none) becomes a zero row."""
    b = np.asarray(boxes, dtype=np.float32).reshape(-1, 4)
    w, h = int(Ws), int(Hs)
    cx, cy = w // 2, h // 2
    a = math.radians(degrees)
    alpha, beta = math.cos(a), math.sin(a)
    nW, nH = int(h * abs(beta) + w * abs(alpha)), int(h * abs(alpha) + w * abs(beta))
    M = np.array([[alpha, beta, (1 - alpha) * cx - beta * cy + (nW / 2 - cx)],
                  [-beta, alpha, beta * cx + (1 - alpha) * cy + (nH / 2 - cy)]], dtype=np.float64)
    x1, y1 = b[:, 0], b[:, 1]
    x2, y3 = x1 + (b[:, 2] - b[:, 0]), y1 + (b[:, 3] - b[:, 1])
    px = np.stack([x1, x2, x1, b[:, 2]], axis=1)                               # the reference's corner order
    py = np.stack([y1, y1, y3, b[:, 3]], axis=1)
    pts = np.stack([px, py, np.ones_like(px)], axis=2).reshape(-1, 3)         # float32 [4N,3]
    moved = np.dot(M, pts.T).T.reshape(-1, 4, 2).astype(np.float32)
    out = np.stack([moved[..., 0].min(1), moved[..., 1].min(1), moved[..., 0].max(1), moved[..., 1].max(1)], axis=1)
    w_delta, h_delta = (nW - w) / 2, (nH - h) / 2
    out[:, [0, 2]] = np.clip(out[:, [0, 2]], w_delta, nW - w_delta) - w_delta
    out[:, [1, 3]] = np.clip(out[:, [1, 3]], h_delta, nH - h_delta) - h_delta
    with np.errstate(all="ignore"):
        area = (out[:, 2] - out[:, 0]) * (out[:, 3] - out[:, 1])
        cl = np.stack([np.maximum(out[:, 0], 0), np.maximum(out[:, 1], 0), np.minimum(out[:, 2], w),
                       np.minimum(out[:, 3], h)], axis=1)
        lost = (area - (cl[:, 2] - cl[:, 0]) * (cl[:, 3] - cl[:, 1])) / area
        cl[~(lost < 1 - 0.25)] = 0
    return cl


def shear_boxes(boxes, factor, Hs, Ws, axis):
    """The GEOMETRIC box side of ShearX (axis 0) / ShearY (axis 1): the enclosing box of the four corners moved by the
    map the pixels of that record follow -- PIL's (1, f, 0, 0, 1, 0) takes output to source, so x' = x - f y (ShearY:
    y' = y - f x) -- in float64, clipped to [0, Ws] x [0, Hs], one rounding to float32.  Factor 0 returns the boxes.
    NOT the reference's numbers: its `shear_x_iaa` / `shear_y_iaa` go through imgaug's fitted canvas."""
    b = np.asarray(boxes, dtype=np.float32).reshape(-1, 4)
    if factor == 0:
        return b.copy()
    d = b.astype(np.float64)
    f = float(factor)
    out = d.copy()
    if axis == 0:
        out[:, 0] = np.minimum(d[:, 0] - f * d[:, 1], d[:, 0] - f * d[:, 3])
        out[:, 2] = np.maximum(d[:, 2] - f * d[:, 1], d[:, 2] - f * d[:, 3])
    else:
        out[:, 1] = np.minimum(d[:, 1] - f * d[:, 0], d[:, 1] - f * d[:, 2])
        out[:, 3] = np.maximum(d[:, 3] - f * d[:, 0], d[:, 3] - f * d[:, 2])
    out[:, [0, 2]] = np.clip(out[:, [0, 2]], 0, Ws)
    out[:, [1, 3]] = np.clip(out[:, [1, 3]], 0, Hs)
    return out.astype(np.float32)


def boxes_layer(name, args, boxes, Hs, Ws):
    """One layer's box side, a pure function of (operation name, level arguments, size): boxes float32 [T,O,4] xyxy ->
    a new array.  Photometric operations leave them; TranslateXRel / TranslateYRel and Rotate are the reference's
    arithmetic (float32); ShearX / ShearY are `shear_boxes`.  Rows that were all zero (absent objects) are zero again
    afterwards, as AugmentOp.__call__ restores them."""
    base = name.replace("Increasing", "")
    if base not in GEOMETRIC:
        return boxes
    zero = (boxes == 0).all(axis=-1)
    b = boxes.reshape(-1, 4)
    v = args[0]
    if base == "Rotate":
        out = rotate_boxes(b, v, Hs, Ws)
    elif base == "ShearX":
        out = shear_boxes(b, v, Hs, Ws, 0)
    elif base == "ShearY":
        out = shear_boxes(b, v, Hs, Ws, 1)
    else:
        out = b.copy()
        if base == "TranslateXRel":
            out[:, [0, 2]] = b[:, [0, 2]] - Ws * v
        else:
            out[:, [1, 3]] = b[:, [1, 3]] - Hs * v
    out = out.reshape(boxes.shape)
    out[zero] = 0
    return out


class RandAugSampler:
    """The reference's `create_random_augment(...)` for one clip as N RandAugOp."""

    def __init__(self, aa_type="rand-m9-mstd0.5-inc1", interpolation="bicubic", prob=0.5):
        p = parse_aa_type(aa_type)
        self.aa_type, self.interpolation = str(aa_type), interpolation
        self.magnitude, self.num_layers, self.magnitude_std = p["magnitude"], p["num_layers"], p["magnitude_std"]
        self.transforms, self.weights = p["transforms"], p["weights"]
        self.prob = float(prob)
        # a fixed filter as transform._pil_interp reads it; None: drawn per frame
        self.filter = None if (interpolation == "random" or not interpolation) else \
            BICUBIC if interpolation == "bicubic" else BILINEAR
        if interpolation in ("lanczos", "hamming"):
            raise NotImplementedError("AUG.INTERPOLATION %r: PIL's affine transform refuses it too" % (interpolation,))
        self.trace = []         # what the last draw() chose: [(name, level arguments, per-frame filters)] per layer

    def draw(self, T, Hs, Ws, video=0, boxes=None):
        """One clip's N records for T frames of Hs x Ws (`video` names the table row they are meant for).
        boxes: float32 [T,O,4] xyxy in source pixels -> (records, boxes_out): the boxes moved through the same layers
        (`boxes_layer`; the draws are the same with and without them)."""
        if self.filter is None and T > 32:
            raise NotImplementedError("INTERPOLATION random draws one filter per frame: T <= 32 (bicubic_mask is 32 bits)")
        if boxes is not None:
            boxes = as_boxes(boxes, 3)
        picks = np.random.choice(len(self.transforms), self.num_layers, replace=self.weights is None, p=self.weights)
        self.trace, ops = [], []
        for k in picks:
            name = self.transforms[int(k)]
            if self.prob < 1.0 and random.random() > self.prob:
                self.trace.append(("", (), ()))
                ops.append(RandAugOp(OP_NONE))
                continue
            magnitude = self.magnitude
            if self.magnitude_std and self.magnitude_std > 0:
                magnitude = random.gauss(magnitude, self.magnitude_std)
            magnitude = min(MAX_LEVEL, max(0, magnitude))
            args = _level_args(name, magnitude)
            filters = ()
            if name in GEOMETRIC:
                if self.filter is None:
                    filters = tuple(random.choice((BILINEAR, BICUBIC)) for _ in range(T))
                else:
                    filters = (self.filter,) * T
            self.trace.append((name, args, filters))
            ops.append(make_op(name, args, filters, Hs, Ws))
            if boxes is not None:
                boxes = boxes_layer(name, args, boxes, Hs, Ws)
        return ops if boxes is None else (ops, boxes)


def build_randaug(cfg):
    """RandAugSampler from cfg.AUG as the reference's dataset reads it (ssv2.py:355-360); None unless AUG.ENABLE.  AUG
    is not a key of this build's default tree (the reference's yaml brings it): absent = the reference's defaults."""
    a = getattr(cfg, "AUG", None)
    if a is None or not bool(getattr(a, "ENABLE", False)):
        return None
    if int(getattr(a, "NUM_SAMPLE", 1)) > 1:
        raise NotImplementedError("AUG.NUM_SAMPLE > 1 is not supported")
    aa = getattr(a, "AA_TYPE", "rand-m9-mstd0.5-inc1")
    if not aa:
        raise NotImplementedError("AUG.ENABLE without AUG.AA_TYPE (the reference raises as well)")
    return RandAugSampler(aa, getattr(a, "INTERPOLATION", "bicubic"))


# ---- the arithmetic, in NumPy: what the kernels are held to ---------------------------------------------------------
_ID = np.arange(256, dtype=np.uint8)
_F32 = np.float32


def _luma(img):
    p = img.astype(np.int64)
    return ((19595 * p[..., 0] + 38470 * p[..., 1] + 7471 * p[..., 2] + 32768) >> 16).astype(np.uint8)


def _autocontrast_lut(h):
    nz = np.nonzero(h)[0]
    lo, hi = int(nz[0]), int(nz[-1])
    if hi <= lo:
        return _ID
    scale = 255.0 / (hi - lo)
    off = -lo * scale
    i = np.arange(256, dtype=np.float64)
    return np.clip(np.trunc(i * scale + off), 0, 255).astype(np.uint8)


def _equalize_lut(h):
    nz = np.nonzero(h)[0]
    if nz.size <= 1:
        return _ID
    step = (int(h.sum()) - int(h[nz[-1]])) // 255
    if step == 0:
        return _ID
    n = step // 2 + np.concatenate(([0], np.cumsum(h[:-1]))).astype(np.int64)
    return np.minimum(n // step, 255).astype(np.uint8)


def _clip8(t):
    """PIL's clip8 on a float array: 0 up to 0 (and for a NaN), 255 from 255, truncation between"""
    with np.errstate(invalid="ignore"):
        mid = (t > 0) & (t < 255)
        return np.where(mid, np.where(mid, t, 0).astype(np.int64), np.where(t >= 255, 255, 0)).astype(np.uint8)


def _blend(a, b, f):
    """ImagingBlend(degenerate a, image b, factor f) in fp32, product and sum rounded separately"""
    f = _F32(f)
    with np.errstate(all="ignore"):
        t = a.astype(_F32) + f * (b.astype(np.int32) - a.astype(np.int32)).astype(_F32)
    if 0 <= f <= 1:
        return t.astype(np.int64).astype(np.uint8)
    return _clip8(t)


def _smooth(img):
    """ImageFilter.SMOOTH: the border ring is the source, inside the 3x3 kernel (1 1 1 / 1 5 1 / 1 1 1) / 13 in fp32"""
    H, W, _ = img.shape
    out = img.copy()
    if H < 3 or W < 3:
        return out
    p = img.astype(_F32)
    k1, k5 = _F32(1) / _F32(13), _F32(5) / _F32(13)
    ss = np.full((H - 2, W - 2, 3), 0.5, dtype=_F32)
    for dy, (a, b, c) in ((1, (k1, k1, k1)), (0, (k1, k5, k1)), (-1, (k1, k1, k1))):
        r = p[1 + dy:H - 1 + dy]
        ss = ss + ((r[:, 0:W - 2] * a + r[:, 1:W - 1] * b) + r[:, 2:W] * c)
    out[1:H - 1, 1:W - 1] = _clip8(ss)
    return out


def _cubic(v1, v2, v3, v4, d):
    p1 = v2
    p2 = -v1 + v3
    p3 = 2 * (v1 - v2) + v3 - v4
    p4 = -v1 + v2 - v3 + v4
    return p1 + d * (p2 + d * (p3 + d * p4))


def _affine(img, m, bicubic):
    """PIL's ImagingGenericTransform with affine_transform and its bilinear / bicubic filter, fill (128,128,128)"""
    H, W, _ = img.shape
    m = [np.float64(v) for v in m]
    with np.errstate(all="ignore"):
        xin = (np.arange(W, dtype=np.float64) + 0.5)[None, :]
        yin = (np.arange(H, dtype=np.float64) + 0.5)[:, None]
        xo = m[0] * xin + m[1] * yin + m[2]
        yo = m[3] * xin + m[4] * yin + m[5]
        inside = (xo >= 0) & (xo < W) & (yo >= 0) & (yo < H)
    xo = np.where(inside, xo, 0.5) - 0.5
    yo = np.where(inside, yo, 0.5) - 0.5
    fx, fy = np.floor(xo), np.floor(yo)
    dx, dy = (xo - fx)[..., None], (yo - fy)[..., None]
    ix, iy = fx.astype(np.int64), fy.astype(np.int64)
    src = img.astype(np.float64)

    def row(y, cols, prev):
        """the filter along x on row y where it lies inside the frame, else the previous row's value"""
        ok = ((y >= 0) & (y < H))[..., None]
        yc = np.clip(y, 0, H - 1)
        taps = [src[yc, np.clip(ix + c, 0, W - 1)] for c in cols]
        v = _cubic(*taps, dx) if bicubic else taps[0] + (taps[1] - taps[0]) * dx
        return v if prev is None else np.where(ok, v, prev)

    if bicubic:
        cols = (-1, 0, 1, 2)
        v1 = row(np.clip(iy - 1, 0, H - 1), cols, None)
        v2 = row(iy, cols, v1)
        v3 = row(iy + 1, cols, v2)
        v4 = row(iy + 2, cols, v3)
        out = _clip8(_cubic(v1, v2, v3, v4, dy))
    else:
        v1 = row(np.clip(iy, 0, H - 1), (0, 1), None)
        v2 = row(iy + 1, (0, 1), v1)
        out = (v1 + (v2 - v1) * dy).astype(np.int64).astype(np.uint8)
    return np.where(inside[..., None], out, np.uint8(FILL))


def apply_frame(img, rec, t=0):
    """one RandAugOp on one frame u8 [H,W,3] (frame index t picks the filter bit) -> a new u8 [H,W,3]"""
    op = rec.op
    if op in (OP_AUTOCONTRAST, OP_EQUALIZE):
        fn = _autocontrast_lut if op == OP_AUTOCONTRAST else _equalize_lut
        out = np.empty_like(img)
        for c in range(3):
            out[..., c] = fn(np.bincount(img[..., c].ravel(), minlength=256))[img[..., c]]
        return out
    if op == OP_INVERT:
        return 255 - img
    if op == OP_POSTERIZE:
        bits = min(max(rec.arg_i, 0), 8)
        return img & np.uint8(~((1 << (8 - bits)) - 1) & 0xFF)
    if op == OP_SOLARIZE:
        return np.where(img.astype(np.int64) < rec.arg_i, img, 255 - img).astype(np.uint8)
    if op == OP_SOLARIZE_ADD:
        return np.where(img < 128, np.clip(img.astype(np.int64) + rec.arg_i, 0, 255), img).astype(np.uint8)
    if op == OP_BRIGHTNESS:
        return _blend(np.zeros_like(img), img, rec.arg_f)
    if op == OP_COLOR:
        return _blend(np.repeat(_luma(img)[..., None], 3, axis=2), img, rec.arg_f)
    if op == OP_CONTRAST:
        mean = int(float(_luma(img).sum(dtype=np.int64)) / float(img.shape[0] * img.shape[1]) + 0.5)
        return _blend(np.full_like(img, mean), img, rec.arg_f)
    if op == OP_SHARPNESS:
        return _blend(_smooth(img), img, rec.arg_f)
    if op == OP_AFFINE:
        return _affine(img, rec.m, bool((rec.bicubic_mask >> (t & 31)) & 1))
    return img.copy()


def pack_extents(extents, V, Hs, Ws, min_side=1):
    """list of (h, w) or an int [V,2] array -> int32 [V,2] NumPy array; ValueError unless min_side <= h_v <= Hs and
    min_side <= w_v <= Ws for every video (RandAugment needs 3 x 3, as it does of the frames)"""
    e = np.asarray(extents.detach().cpu().numpy() if hasattr(extents, "detach") else extents)
    if e.dtype.kind not in "iu" or e.shape != (V, 2):
        raise ValueError("extents are int [%d,2] = (h, w) per video, got %s %s" % (V, e.dtype, tuple(e.shape)))
    e = np.ascontiguousarray(e.astype(np.int64))
    for v in range(V):
        h, w = int(e[v, 0]), int(e[v, 1])
        if h > Hs or w > Ws:
            raise ValueError("extent %d: %dx%d is larger than the %dx%d buffer" % (v, h, w, Hs, Ws))
        if h < min_side or w < min_side:
            raise ValueError("extent %d: %dx%d is smaller than %dx%d" % (v, h, w, min_side, min_side))
    return e.astype(np.int32)


def apply_host(frames, table, extents=None):
    """frames u8 [V,T,Hs,Ws,3] (NumPy) through the N layers of `table` (int32 [V,N,16] or lists of RandAugOp).
    extents (int [V,2] or None): video v is its tight [h_v, w_v] slice and goes through the chain as that image; the
    padding around it comes out as it went in."""
    frames = np.asarray(frames)
    if frames.dtype != np.uint8 or frames.ndim != 5 or frames.shape[-1] != 3:
        raise ValueError("frames must be uint8 [V,T,H,W,3]")
    table = pack_table(table)
    if table.shape[0] != frames.shape[0]:
        raise ValueError("the table has %d rows for %d videos" % (table.shape[0], frames.shape[0]))
    Hs, Ws = frames.shape[2:4]
    if extents is not None:
        extents = pack_extents(extents, frames.shape[0], Hs, Ws, min_side=3)
    out = frames.copy()
    for v in range(frames.shape[0]):
        recs = [RandAugOp.unpack(w) for w in table[v]]
        h, w = (Hs, Ws) if extents is None else (int(extents[v, 0]), int(extents[v, 1]))
        for t in range(frames.shape[1]):
            img = frames[v, t, :h, :w]
            for rec in recs:
                img = apply_frame(img, rec, t)
            out[v, t, :h, :w] = img
    return out


# ---- the device side ------------------------------------------------------------------------------------------------
def workspace_bytes(V, T):
    return V * T * SLOT_BYTES


def apply(src, table, dst, tmp, workspace, extents=None):
    """Launch the 2N kernels: src u8 [V,T,Hs,Ws,3] through the N layers of `table` (int32 [V,N,16] on the device) into
    dst.  The layers ping-pong between tmp and dst so that the LAST one lands in dst; src is never written.  tmp (same
    shape; None is fine for N == 1) and workspace (uint8, workspace_bytes(V, T)) are scratch.
    extents: int32 [V,2] = (h_v, w_v) on the device (`svit_randaug_*_ext`; the kernels read it at run time and clamp it
    into the buffer, range checks are the caller's: `pack_extents`); None: the plain entry points."""
    import torch
    from . import hip
    V, T, Hs, Ws, _ = src.shape
    N = table.shape[1]
    if table.dtype != torch.int32 or table.dim() != 3 or tuple(table.shape) != (V, N, 16) or not table.is_contiguous():
        raise hip.SvitHipError("the RandAugment table must be contiguous int32 [%d,N,16], got %s %s"
                               % (V, table.dtype, tuple(table.shape)))
    bufs = [src, dst] if tmp is None else [src, dst, tmp]
    for b in bufs + [table, workspace]:
        if not b.is_cuda or b.device != src.device or not b.is_contiguous():
            raise hip.SvitHipError("RandAugment buffers must be contiguous tensors on %s" % (src.device,))
    for b in bufs:
        if b.dtype != torch.uint8 or b.shape != src.shape:
            raise hip.SvitHipError("RandAugment frame buffers must be uint8 %s" % (tuple(src.shape),))
    if N > 1 and tmp is None:
        raise hip.SvitHipError("RandAugment with %d layers needs the scratch buffer" % N)
    if len({b.data_ptr() for b in bufs}) != len(bufs):
        raise hip.SvitHipError("RandAugment src, dst and tmp must be distinct buffers")
    if workspace.dtype != torch.uint8 or workspace.numel() < workspace_bytes(V, T):
        raise hip.SvitHipError("RandAugment workspace must be uint8 with %d bytes" % workspace_bytes(V, T))
    ext, suffix = (), ""
    if extents is not None:
        if (extents.dtype != torch.int32 or tuple(extents.shape) != (V, 2) or not extents.is_contiguous()
                or extents.device != src.device):
            raise hip.SvitHipError("the extents must be contiguous int32 [%d,2] on %s, got %s %s on %s"
                                   % (V, src.device, extents.dtype, tuple(extents.shape), extents.device))
        ext, suffix = (hip.ptr(extents),), "_ext"
    cur = src
    for k in range(N):
        out = dst if (N - 1 - k) % 2 == 0 else tmp
        hip.call("svit_randaug_stats" + suffix, hip.ptr(cur), hip.ptr(table), *ext, k, hip.ptr(workspace), V, T, Hs, Ws, N)
        hip.call("svit_randaug_apply" + suffix, hip.ptr(cur), hip.ptr(out), hip.ptr(table), *ext, k, hip.ptr(workspace),
                 V, T, Hs, Ws, N)
        cur = out
    return dst
